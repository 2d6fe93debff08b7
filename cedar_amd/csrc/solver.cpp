// C-ABI layer 2: device-resident multilevel hierarchy and V-cycle.
// Restates the orchestration of the reference's serial solvers on top of the
// HIP kernels; every level array lives in HBM for the whole solve, only norms
// (one double per iteration) cross PCIe.
//   level sizing / allocation : include/cedar/2d/solver.h:57-116, include/cedar/3d/solver.h:54-123
//   set-up loop               : include/cedar/multilevel.h:243-265 (interp -> Galerkin -> relax set-up)
//   V-cycle                   : include/cedar/cycle/vcycle.h:57-115
//   smoothers                 : include/cedar/multilevel.h:165-222 (pre = DOWN, post = UP; line-xy: x,y / y,x)
//   solve loop                : include/cedar/multilevel.h:268-298
// The V-cycle is a fixed launch sequence for a given (x,b) pair; it is captured
// once into a hipGraph and replayed, which removes the per-launch host cost
// that dominates the coarse levels (a 2D 4096^2 cycle is ~130 launches).
#include "../../include/cedar_amd.h"
#include "common.h"
#include "stage.h"
#include "relax3_psum.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

using namespace cedar_amd;

namespace {

struct Level {
	int nx = 0, ny = 0, nz = 1;
	int II = 0, JJ = 0, KK = 1;
	int nst = 0;
	size_t npts = 0;
	real_t *A = nullptr;
	bool ownA = true;
	real_t *P = nullptr;
	real_t *x = nullptr, *b = nullptr, *res = nullptr;
	real_t *SOR0 = nullptr, *SOR1 = nullptr;
	real_t *yscr = nullptr; // y-line scratch
	// y-lines on transposed arrays (Dirichlet; lines.hip relax_lines_yt): transposed operator planes, transposed
	// right-hand side, scratch for the transposed x; bt_fresh: bt holds the transpose of this visit's b
	real_t *At = nullptr, *bt = nullptr, *xt = nullptr;
	mutable bool bt_fresh = false;
	// scan-ordered copies of the line factors (lines.hip line_pttrs_pf): PFx of the x-line factors, PFy of the y-line
	// factors when the y sweeps run on the transposed arrays; nullptr = the kernels read SOR directly
	real_t *PFx = nullptr, *PFy = nullptr;
	// 3D 27-point: row-interleaved solve copy of A and 1/diag (common.h Op3) read by relax and residual
	real_t *Ailv = nullptr;
	// the same copy in single precision (common.h Op3f) after cedar_amd_solver_use_fp32_operator: it replaces Ailv, and
	// the level's sweeps and the cycle's residual read it; A itself stays FP64
	float *A32 = nullptr;
	// 3D 7-point (level 0): the single-precision copy of A and 1/diag (common.h Op7f) after
	// cedar_amd_solver_use_fp32_operator_all; the level's sweeps and the cycle's residual read it, A itself stays FP64
	float *A7f = nullptr;
	// 2D, Dirichlet point relaxation: the single-precision copy of A and 1/diag (common.h Op2f) after
	// cedar_amd_solver_use_fp32_operator_2d; the level's sweeps and the cycle's residual read it, A itself stays FP64.  Its
	// presence alone decides that: a level that keeps it runs the row kernels, never the LDS-resident small-level ones
	float *A2f = nullptr;
	// 2D, Dirichlet line relaxation after cedar_amd_solver_use_fp32_operator_lines (linesf.hip): A2f is
	// the copy of A with a zero 1/diag slot-row (the x-line right-hand sides and the cycle's residual read it), At2f the
	// same form of the transposed planes At where the level runs y lines, and the factors of each direction in use are
	// floats in the form the FP64 kernel of that direction reads: the scan-ordered copy (PFx32 / PFy32) where the level
	// keeps PFx / PFy, else the plain image of the two SOR planes (Fx32 / Fy32).  A, At, SOR*, PF* stay
	float *At2f = nullptr, *Fx32 = nullptr, *Fy32 = nullptr, *PFx32 = nullptr, *PFy32 = nullptr;
	// the single-precision copy of P (common.h Ci3f; transferf.hip) after
	// cedar_amd_solver_use_fp32_interpolation: the cycle's transfers between this level and the next finer one read it, P
	// itself stays FP64.  Never kept where the LDS-resident small-level kernels serve the finer level
	float *P32 = nullptr;
	// 3D 27-point: partial-sum scratch of the relax sweep (relax3d_psum.hip), one vector
	real_t *T = nullptr;
	// the set-up products (A, P, SOR, At, PF*) belong to another solver of the same operator (plane relaxation:
	// every plane solver of a direction is built from the same 2D operator); this level owns only its vectors
	bool shared = false;
	// plane relaxation (3D): the plane solvers of this level, one set per direction in use (xy, xz, yz)
	struct PlaneSet *pl[3] = {nullptr, nullptr, nullptr};
};

// Which stored form of a 27-point level's operator a kernel reads is decided by these two selectors and nowhere else.
// The exact view: the operator the caller gave, as the reported residual and the Krylov passes read it -- the
// row-interleaved copy (the same doubles) where the level keeps one, else the Cedar planes; never the float copy.
Op3 exact_view27(const Level &L)
{
	return L.Ailv ? op3_ilv(L.Ailv, L.II, L.JJ, L.KK) : op3_cedar(L.A, L.SOR0, L.II, L.JJ, L.KK);
}

// The cycle's view, as the sweeps and the cycle's residual read it: the float copy where the level keeps it (it has
// released Ailv, so the exact view there is the unrounded planes, which the cycle must not mix in), else the exact view.
// f takes const auto &: Op3f or Op3, served by the overloads of relax3_gs27_op, residual27_op and the *_many pair.
template <class F> void with_cycle_view27(const Level &L, F &&f)
{
	if (L.A32) f(op3f_ilv(L.A32, L.II, L.JJ, L.KK));
	else f(exact_view27(L));
}

// The same choice for a 7-point level, made here and nowhere else: f(Op7f) on the float copy where the level keeps it, else
// g() on the Cedar planes L.A / L.SOR0 -- the exact operator, which residual_true, the Krylov passes and interp_add3's
// diagonal always read.
template <class F, class G> void with_cycle_view7(const Level &L, F &&f, G &&g)
{
	if (L.A7f) f(op7f_view(L.A7f, L.II, L.JJ, L.KK));
	else g();
}

// The same choice for a 2D level, made here and nowhere else: f(Op2f) on the float copy where the level keeps it, else g()
// on the Cedar planes L.A / L.SOR0 -- the exact operator, which residual_true, the Krylov passes, interp_add2's diagonal,
// restriction and the coarsest solve always read.
template <class F, class G> void with_cycle_view2(const Level &L, F &&f, G &&g)
{
	if (L.A2f) f(op2f_view(L.A2f, L.II, L.nst));
	else g();
}

// The same choice for one direction of a line-relaxed 2D level, made here and nowhere else: f(operator copy, float
// factors, their scan-ordered copy) where the level keeps the float copies -- for y lines the copy of the transposed
// planes -- else g() on today's FP64 arrays.
template <class F, class G> void with_line_view(const Level &L, bool ylines, F &&f, G &&g)
{
	if (!L.A2f) g();
	else if (ylines) f(op2f_view(L.At2f, L.JJ, L.nst), L.Fy32, L.PFy32);
	else f(op2f_view(L.A2f, L.II, L.nst), L.Fx32, L.PFx32);
}

// include/cedar/3d/relax_planes.h:164-246.  The reference keeps one 2D solver per plane; copy_coeff gives all of
// them the same operator (planes.hip), so one hierarchy is set up and the others share its set-up products.  Planes
// of one colour are independent: instance q serves the planes 2q+1 and 2q+2 (one of each colour) on fixed 2D vectors
// (slot q of x2s / b2s), so its V-cycle is captured into a hipGraph once and replayed; the replays of a colour are
// spread over a few streams.
struct PlaneSet {
	int dir = 0, np = 0, I2 = 0, J2 = 0;
	size_t P2 = 0;
	real_t *so2 = nullptr, *x2s = nullptr, *b2s = nullptr;
	std::vector<cedar_amd_solver *> inst;
};

real_t *dalloc_raw(size_t n) // not cleared: the caller writes every element
{
	void *p = nullptr;
	CEDAR_HIP_CHECK(hipMalloc(&p, (n ? n : 1) * sizeof(real_t)));
	return static_cast<real_t *>(p);
}

real_t *dalloc(size_t n)
{
	void *p = nullptr;
	size_t bytes = (n ? n : 1) * sizeof(real_t);
	CEDAR_HIP_CHECK(hipMalloc(&p, bytes));
	zero_fill(static_cast<real_t *>(p), bytes / sizeof(real_t), current_stream());
	return static_cast<real_t *>(p);
}

} // namespace

// cedar_amd_solver_create with a batch capacity (plane relaxation builds its 2D solvers with one: planes_setup)
static cedar_amd_solver *solver_create(int nd, len_t nx, len_t ny, len_t nz, int nstencil, const real_t *so, int own_device_so,
                                       const cedar_amd_settings *settings, int batch, bool periodic_batch = false,
                                       bool semidef = false);

struct cedar_amd_solver {
	int nd = 2;
	cedar_amd_settings st;
	std::vector<Level> lv;
	real_t *ABD = nullptr, *bbd = nullptr;
	int nabd1 = 0, nabd2 = 0;
	int *dinfo = nullptr;
	real_t *red = nullptr; // reduction scratch (4096 partials + result)
	// captured V-cycle
	hipGraphExec_t gexec = nullptr;
	const real_t *gx = nullptr, *gb = nullptr;
	int gnb = 1; // batch count the graph was captured for
	hipStream_t gstream = nullptr;
	bool use_graph = true;
	// batch of independent right-hand sides on this one hierarchy (Dirichlet, V-cycle; 2D, and 3D point relaxation;
	// plane relaxation runs the planes of a colour as one batch, cedar_amd_solver_*_many the caller's right-hand sides):
	// every level's vectors hold nb_alloc items, a cycle works on the first nb.  3D with nb > 1: the kernels of many3d.hip
	// in the reference order; nb == 1: the single-vector kernels, whatever nb_alloc is
	int nb_alloc = 1, nb = 1;
	// a periodic 3D handle of cedar_amd_solver_create_many_periodic or a periodic 2D handle of
	// cedar_amd_solver_create_many_periodic2: its levels hold nb_alloc items too, and a batch runs the kernels of
	// periodic_many3d.hip / periodic_many2d.hip.  A periodic handle made any other way holds one item and the _many calls
	// refuse it
	bool per_batch = false;
	// a handle of cedar_amd_solver_create_semidefinite: the operator is singular with the constants as null space.  Its
	// coarsest factor is that of the coarsest matrix with the last diagonal entry doubled and every coarsest solve removes
	// the mean (ibc == 0 too); only cedar_amd_solver_fcg_semidefinite / _many run a Krylov iteration on it.  pm: scratch
	// of project_mean_many for nb_alloc items
	bool semidef = false;
	real_t *pm = nullptr;
	// a second captured cycle: the two colours of a plane sweep may differ by one plane
	hipGraphExec_t gexec2 = nullptr;
	int gnb2 = 0;
	bool shared_abd = false; // ABD belongs to the solver this one was cloned from
	// plane relaxation: side streams and their fork / join events
	std::vector<hipStream_t> pstreams;
	std::vector<hipEvent_t> pevents;
	hipEvent_t pfork = nullptr;
	// preconditioned conjugate gradient (cedar_amd_solver_pcg), allocated on the first call: level-0 vectors r, z, w and
	// the pair of directions (p is read at the stencil neighbours while p' is written), partial-sum slab, device scalars
	real_t *kr = nullptr, *kz = nullptr, *kw = nullptr, *kp[2] = {nullptr, nullptr};
	real_t *kslab = nullptr, *ksc = nullptr;
	int kitems = 0; // items each of them holds: 1, or nb_alloc after the first cedar_amd_solver_pcg_many (item-major)
};

namespace {

int compute_num_levels(int nd, len_t nx, len_t ny, len_t nz, int min_coarse)
{
	// float nxc = (nx-1)/(1<<ng) + 1 with unsigned integer division; do { } while (min >= min_coarse)
	int ng = 0;
	float m;
	do {
		ng++;
		float nxc = (float)((nx - 1) / (1u << ng) + 1);
		float nyc = (float)((ny - 1) / (1u << ng) + 1);
		m = nxc < nyc ? nxc : nyc;
		if (nd == 3) {
			float nzc = (float)((nz - 1) / (1u << ng) + 1);
			m = m < nzc ? m : nzc;
		}
	} while (m >= (float)min_coarse);
	return ng;
}

void level_init(Level &L, int nd, int nx, int ny, int nz, int nst, bool coarse, bool lines_y, bool lines_yt, int nb = 1)
{
	L.nx = nx; L.ny = ny; L.nz = nd == 3 ? nz : 1;
	L.II = nx + 2; L.JJ = ny + 2; L.KK = nd == 3 ? nz + 2 : 1;
	L.nst = nst;
	L.npts = (size_t)L.II * L.JJ * L.KK;
	L.res = dalloc(L.npts * nb);
	L.SOR0 = dalloc(L.npts * 2);
	if (lines_y) {
		L.SOR1 = dalloc(L.npts * 2);
		L.yscr = dalloc(ylines_scratch_doubles(L.II, L.JJ));
	}
	if (lines_yt) {
		L.At = dalloc(L.npts * nst);
		L.bt = dalloc(L.npts * nb);
		L.xt = dalloc(L.npts * nb);
	}
	if (coarse) {
		L.A = dalloc(L.npts * nst);
		L.P = dalloc(L.npts * (nd == 3 ? 26 : 8));
		L.x = dalloc(L.npts * nb);
		L.b = dalloc(L.npts * nb);
	}
}

// clear a level array inside the cycle.  The library's own kernel; CEDAR_AMD_DEBUG_MEMSET=1 switches back to
// hipMemsetAsync to reproduce the runtime defect recorded in DESIGN.md section 7 (tools/memset_rootcause.py).
void clear(real_t *p, size_t n, hipStream_t st)
{
	static const bool dbg = getenv("CEDAR_AMD_DEBUG_MEMSET") && atoi(getenv("CEDAR_AMD_DEBUG_MEMSET")) != 0;
	if (dbg) CEDAR_HIP_CHECK(hipMemsetAsync(p, 0, n * sizeof(real_t), st));
	else zero_fill(p, n, st);
}

// the cycle's residual on a level.  3D 27-point: through the cycle's view; a single vector on a level without a copy of
// its own, and 7-point levels, go through residual3, which finds a copy that the operator's owner registered (relax3d.hip)
void residual(const cedar_amd_solver *s, const Level &L, const real_t *x, const real_t *b, real_t *r, hipStream_t st)
{
	const Batch bt{s->nb, L.npts};
	if (s->nd == 2)
		with_cycle_view2(
		    L, [&](const Op2f &A) { residual2_op(A, b, x, r, L.II, L.JJ, L.nst, st, bt); },
		    [&]() { residual2(L.A, b, x, r, L.II, L.JJ, L.nst, st, bt); });
	else if (L.nst != 14 && (s->nb > 1 || L.A7f)) // (a single vector only for the float view: op7f.hip)
		with_cycle_view7(
		    L,
		    [&](const Op7f &A) {
			    if (s->nb > 1) residual7_many(A, b, x, r, L.II, L.JJ, L.KK, st, bt);
			    else residual7_op(A, b, x, r, L.II, L.JJ, L.KK, st);
		    },
		    [&]() { residual7_many(L.A, b, x, r, L.II, L.JJ, L.KK, st, bt); });
	else if (s->nb > 1) with_cycle_view27(L, [&](const auto &A) { residual27_many(A, b, x, r, L.II, L.JJ, L.KK, st, bt); });
	else if (L.A32 || L.Ailv) with_cycle_view27(L, [&](const auto &A) { residual27_op(A, b, x, r, L.II, L.JJ, L.KK, st); });
	else residual3(L.A, b, x, r, L.II, L.JJ, L.KK, L.nst, st);
}

// r = b - A x with the operator the caller gave: what a solve reports and what the Krylov recurrence starts from.  The
// cycle's residual, except on a level that keeps the float copy: there the same launches on the exact view
void residual_true(const cedar_amd_solver *s, const Level &L, const real_t *x, const real_t *b, real_t *r, hipStream_t st)
{
	if (!L.A32 && !L.A7f && !L.A2f) residual(s, L, x, b, r, st);
	else if (s->nd == 2) residual2(L.A, b, x, r, L.II, L.JJ, L.nst, st, Batch{s->nb, L.npts});
	else if (s->nb > 1 && L.nst != 14) residual7_many(L.A, b, x, r, L.II, L.JJ, L.KK, st, Batch{s->nb, L.npts});
	else if (s->nb > 1) residual27_many(exact_view27(L), b, x, r, L.II, L.JJ, L.KK, st, Batch{s->nb, L.npts});
	else residual3(L.A, b, x, r, L.II, L.JJ, L.KK, L.nst, st);
}

// one y-line sweep: on the transposed arrays when the level keeps them
void lines_y(const Level &L, real_t *x, const real_t *b, const real_t *sor, int updown, int ipn, hipStream_t st, Batch bt = Batch())
{
	if (!L.At) {
		// Dirichlet batches always keep the transposed arrays (cedar_amd_solver_create); a periodic 2D batch walks its items
		// through the gather / solve / scatter pipeline on the level's one scratch, in stream order
		for (int m = 0; m < bt.n; m++)
			relax_lines_y(L.A, b + m * bt.stride, x + m * bt.stride, sor, L.yscr, L.II, L.JJ, L.nst, updown, st, ipn);
		return;
	}
	if (!L.bt_fresh) {
		transpose2(b, L.bt, L.II, L.JJ, st, bt);
		L.bt_fresh = true;
	}
	with_line_view(
	    L, true,
	    [&](const Op2f &At, const float *f, const float *pf) {
		    relax_lines_yt_op(At, L.bt, x, L.xt, f, L.II, L.JJ, L.nst, updown, st, pf, bt);
	    },
	    [&]() { relax_lines_yt(L.At, L.bt, x, L.xt, sor, L.II, L.JJ, L.nst, updown, st, L.PFy, bt); });
}

// one x-line sweep
void lines_x(const Level &L, real_t *x, const real_t *b, int updown, int ipn, hipStream_t st, Batch bt)
{
	with_line_view(
	    L, false,
	    [&](const Op2f &A, const float *f, const float *pf) { relax_lines_x_op(A, b, x, f, L.II, L.JJ, L.nst, updown, st, pf, bt); },
	    [&]() { relax_lines_x(L.A, b, x, L.SOR0, L.II, L.JJ, L.nst, updown, st, ipn, L.PFx, bt); });
}

double l2_dev(cedar_amd_solver *s, const Level &L, const real_t *v)
{
	sumsq_interior(v, L.II, L.JJ, L.KK, s->red, s->red + 4096, current_stream());
	double ss = 0;
	CEDAR_HIP_CHECK(hipMemcpyAsync(&ss, s->red + 4096, sizeof(double), hipMemcpyDeviceToHost, current_stream()));
	CEDAR_HIP_CHECK(hipStreamSynchronize(current_stream()));
	return std::sqrt(ss);
}

// ------------------------------------------------------------------ plane relaxation
// a plane sweep runs cycles of its 2D solvers, and a 3D cycle runs plane sweeps: the two below are defined after the cycle
void cycle_on(cedar_amd_solver *s, real_t *x, const real_t *b, hipStream_t st);
bool graph_prepare(cedar_amd_solver *s, real_t *x, const real_t *b, hipStream_t st);

bool graph_ready(const cedar_amd_solver *s, const real_t *x, const real_t *b)
{
	return !s->use_graph || (s->gexec && s->gx == x && s->gb == b && s->gnb == s->nb);
}

// a solver on the same operator as `proto` that shares its set-up products and owns only its vectors
cedar_amd_solver *clone_vectors(const cedar_amd_solver *proto)
{
	cedar_amd_solver *c = new cedar_amd_solver;
	c->nd = proto->nd; c->st = proto->st; c->use_graph = proto->use_graph;
	c->lv = proto->lv; // pointers to the shared products; the vectors are replaced below
	for (size_t l = 0; l < c->lv.size(); l++) {
		Level &L = c->lv[l];
		L.shared = true; L.ownA = false;
		L.res = dalloc(L.npts);
		if (L.yscr) L.yscr = dalloc(ylines_scratch_doubles(L.II, L.JJ));
		if (L.bt) { L.bt = dalloc(L.npts); L.xt = dalloc(L.npts); }
		L.bt_fresh = false;
		if (l > 0) { L.x = dalloc(L.npts); L.b = dalloc(L.npts); }
	}
	c->ABD = proto->ABD; c->shared_abd = true;
	c->nabd1 = proto->nabd1; c->nabd2 = proto->nabd2;
	c->bbd = dalloc(c->nabd2);
	c->red = dalloc(4100);
	CEDAR_HIP_CHECK(hipMalloc((void **)&c->dinfo, 64));
	return c;
}

// kman->setup<plane_relax<dir>>(so): the 2D operator, one full 2D set-up, vector-only clones for the other instances
PlaneSet *planes_setup(int dir, const real_t *so3, int II, int JJ, int KK, int nst, const cedar_amd_settings &pst, hipStream_t st)
{
	PlaneSet *ps = new PlaneSet;
	ps->dir = dir;
	ps->I2 = dir == 2 ? JJ : II;
	ps->J2 = dir == 0 ? JJ : KK;
	ps->np = (dir == 0 ? KK : dir == 1 ? JJ : II) - 2;
	ps->P2 = (size_t)ps->I2 * ps->J2;
	const int nst2 = nst == 14 ? 5 : 3, ninst = (ps->np + 1) / 2;
	ps->so2 = dalloc_raw(ps->P2 * nst2);
	plane_operator(dir, nst, so3, ps->so2, II, JJ, KK, st);
	ps->x2s = dalloc(ps->P2 * ninst);
	ps->b2s = dalloc(ps->P2 * ninst); // ghost entries stay zero: plane_gather writes interiors only
	// one cycle per plane (the reference's default plane configuration): the planes of a colour run as ONE batch through
	// the 2D kernels (common.h Batch) -- the hierarchy is shared anyway, only the vectors differ.  CEDAR_AMD_PLANE_BATCH=0,
	// or a plane configuration with max-iter > 1 (per-plane early exit), keeps one solver instance per pair of planes.
	const char *eb = getenv("CEDAR_AMD_PLANE_BATCH");
	const bool want_batch = pst.max_iter == 1 && !(eb && atoi(eb) == 0);
	cedar_amd_solver *first = solver_create(2, ps->I2 - 2, ps->J2 - 2, 1, nst2, ps->so2, 1, &pst, want_batch ? ninst : 1);
	if (!first) {
		(void)hipFree(ps->so2); (void)hipFree(ps->x2s); (void)hipFree(ps->b2s);
		delete ps;
		return nullptr;
	}
	ps->inst.push_back(first);
	if (first->nb_alloc < ninst)
		for (int q = 1; q < ninst; q++) ps->inst.push_back(clone_vectors(first));
	return ps;
}

void planes_destroy(PlaneSet *ps)
{
	if (!ps) return;
	for (size_t q = ps->inst.size(); q-- > 0;) cedar_amd_solver_destroy(ps->inst[q]); // clones before the owner of the products
	(void)hipFree(ps->so2); (void)hipFree(ps->x2s); (void)hipFree(ps->b2s);
	delete ps;
}

// relax_planes (relax_planes.h:36-72): DOWN = the odd planes (1, 3, ..), then the even ones; UP = even, then odd.
// Per colour: gather all its planes and right-hand sides (one launch), one 2D solve per plane, scatter (one launch).
// Plane configuration max-iter 1 (the reference's default): the solve is one V-cycle whatever the norms are, replayed
// from the instance's graph on a side stream; otherwise multilevel::solve's loop with its host-side tolerance test.
void planes_relax(cedar_amd_solver *s3, PlaneSet &ps, const Level &L, real_t *x, const real_t *b, int updown, hipStream_t st)
{
	const int order[2] = {updown == BMG_DOWN ? 1 : 2, updown == BMG_DOWN ? 2 : 1};
	for (int c = 0; c < 2; c++) {
		const int beg = order[c];
		const int n = beg > ps.np ? 0 : (ps.np - beg) / 2 + 1;
		if (n == 0) continue;
		plane_gather(ps.dir, L.nst, L.A, x, b, ps.x2s, ps.b2s, L.II, L.JJ, L.KK, beg, n, st);
		const int maxit = ps.inst[0]->st.max_iter;
		if (maxit == 1 && ps.inst[0]->nb_alloc >= n) { // the colour as one batch: one graph replay on the solver's stream
			ps.inst[0]->nb = n;
			cycle_on(ps.inst[0], ps.x2s, ps.b2s, st);
		} else if (maxit == 1) {
			const int S = (int)s3->pstreams.size() < n ? (int)s3->pstreams.size() : n;
			if (S <= 1) {
				for (int q = 0; q < n; q++) cycle_on(ps.inst[q], ps.x2s + ps.P2 * q, ps.b2s + ps.P2 * q, st);
			} else {
				// Every instance's graph is recorded and instantiated BEFORE the first replay of this colour is launched,
				// with the device idle: capture / hipGraphInstantiate never run beside replays in flight on the side streams
				// (the first visit used to interleave them; DESIGN.md section 6, the rocprofv3 abort of round 2).
				bool missing = false;
				for (int q = 0; q < n; q++)
					missing = missing || !graph_ready(ps.inst[q], ps.x2s + ps.P2 * q, ps.b2s + ps.P2 * q);
				if (missing) {
					CEDAR_HIP_CHECK(hipDeviceSynchronize());
					for (int q = 0; q < n; q++)
						if (ps.inst[q]->use_graph) graph_prepare(ps.inst[q], ps.x2s + ps.P2 * q, ps.b2s + ps.P2 * q, s3->pstreams[q % S]);
				}
				CEDAR_HIP_CHECK(hipEventRecord(s3->pfork, st));
				for (int t = 0; t < S; t++) CEDAR_HIP_CHECK(hipStreamWaitEvent(s3->pstreams[t], s3->pfork, 0));
				for (int q = 0; q < n; q++) cycle_on(ps.inst[q], ps.x2s + ps.P2 * q, ps.b2s + ps.P2 * q, s3->pstreams[q % S]);
				for (int t = 0; t < S; t++) {
					CEDAR_HIP_CHECK(hipEventRecord(s3->pevents[t], s3->pstreams[t]));
					CEDAR_HIP_CHECK(hipStreamWaitEvent(st, s3->pevents[t], 0));
				}
			}
		} else {
			for (int q = 0; q < n; q++) { // multilevel.h:277-298
				cedar_amd_solver *p = ps.inst[q];
				Level &L2 = p->lv[0];
				real_t *x2 = ps.x2s + ps.P2 * q;
				const real_t *b2 = ps.b2s + ps.P2 * q;
				residual(p, L2, x2, b2, L2.res, st);
				const double res0 = l2_dev(p, L2, L2.res);
				for (int it = 0; it < maxit; it++) {
					cycle_on(p, x2, b2, st);
					residual(p, L2, x2, b2, L2.res, st);
					if (l2_dev(p, L2, L2.res) / res0 < p->st.tol) break;
				}
			}
		}
		plane_scatter(ps.dir, ps.x2s, x, L.II, L.JJ, L.KK, beg, n, st);
	}
}

void smooth(const cedar_amd_solver *s, const Level &L, real_t *x, const real_t *b, int updown, int n, hipStream_t st)
{
	if (s->nd == 2 && s->st.ibc == 0 && s->st.relaxation >= CEDAR_AMD_RELAX_LINE_X && s->st.relaxation <= CEDAR_AMD_RELAX_LINE_XY
	    && !L.A2f && lines_small_ok(L.II, L.JJ)) {
		// a small level: every sweep of this visit in one launch, the level resident in LDS (lines_small.hip)
		const int kind = s->st.relaxation == CEDAR_AMD_RELAX_LINE_X ? 1 : s->st.relaxation == CEDAR_AMD_RELAX_LINE_Y ? 2 : 3;
		relax_lines_small(L.A, b, x, L.SOR0, kind == 2 ? L.SOR0 : L.SOR1, L.II, L.JJ, L.nst, kind, updown, n, st, Batch{s->nb, L.npts});
		return;
	}
	if (s->nd == 2 && s->st.ibc == 0 && s->st.relaxation == CEDAR_AMD_RELAX_POINT && !L.A2f && lines_small_ok(L.II, L.JJ)) {
		relax_points_small(L.A, b, x, L.SOR0, L.II, L.JJ, L.nst, updown, n, st, Batch{s->nb, L.npts});
		return;
	}
	for (int it = 0; it < n; it++) {
		if (s->nd == 3 && s->st.relaxation >= CEDAR_AMD_RELAX_PLANE_XY) { // multilevel.h:179-189, :208-218
			static const int down[3] = {0, 2, 1}, up[3] = {1, 2, 0}; // xy, yz, xz on the way down; xz, yz, xy on the way up
			for (int t = 0; t < 3; t++) {
				const int d = updown == BMG_DOWN ? down[t] : up[t];
				if (L.pl[d]) planes_relax(const_cast<cedar_amd_solver *>(s), *L.pl[d], L, x, b, updown, st);
			}
			continue;
		}
		if (s->nd == 3 && s->st.ibc) {
			// the ghosts of x hold the periodic image after any sweep, after interp_add, and on a coarse level (x starts
			// from zero); the first pre-smoothing sweep on level 0 sees the caller's x and makes no such assumption
			const bool consistent = it > 0 || updown == BMG_UP || &L != &s->lv[0];
			if (s->nb > 1) // a batch (periodic_many3d.hip): the same rule for every item
				relax3_gs_per_many(L.A, b, x, L.SOR0, L.II, L.JJ, L.KK, L.nst, updown, s->st.ibc, st, consistent, Batch{s->nb, L.npts});
			else relax3_gs_per(L.A, b, x, L.SOR0, L.II, L.JJ, L.KK, L.nst, updown, s->st.ibc, st, consistent);
			continue;
		}
		if (s->nd == 3 && s->nb > 1) { // a batch of right-hand sides: reference order, operator fetched once (many3d.hip)
			const Batch bt{s->nb, L.npts};
			if (L.nst != 14)
				with_cycle_view7(
				    L, [&](const Op7f &A) { relax3_gs7_many(A, b, x, L.II, L.JJ, L.KK, updown, st, bt); },
				    [&]() { relax3_gs7_many(L.A, b, x, L.SOR0, L.II, L.JJ, L.KK, updown, st, bt); });
			else with_cycle_view27(L, [&](const auto &A) { relax3_gs27_many(A, b, x, L.II, L.JJ, L.KK, updown, st, bt); });
			continue;
		}
		if (s->nd == 3) { // without a copy or scratch of its own: relax3_gs, which finds what the operator's owner registered
			if (L.nst != 14)
				with_cycle_view7(
				    L, [&](const Op7f &A) { relax3_gs7_op(A, b, x, L.II, L.JJ, L.KK, updown, st); },
				    [&]() { relax3_gs(L.A, b, x, L.SOR0, L.II, L.JJ, L.KK, L.nst, updown, st); });
			else if (!L.A32 && !L.Ailv && !L.T) relax3_gs(L.A, b, x, L.SOR0, L.II, L.JJ, L.KK, L.nst, updown, st);
			else with_cycle_view27(L, [&](const auto &A) { relax3_gs27_op(A, b, x, L.II, L.JJ, L.KK, updown, st, L.T); });
			continue;
		}
		const int ipn = s->st.ibc;
		if (ipn && s->st.relaxation == CEDAR_AMD_RELAX_POINT) { // periodic point relaxation; a batch: periodic_many2d.hip
			if (s->nb > 1) relax2_gs_per_many(L.A, b, x, L.SOR0, L.II, L.JJ, L.nst, updown, ipn, st, Batch{s->nb, L.npts});
			else relax2_gs_per(L.A, b, x, L.SOR0, L.II, L.JJ, L.nst, updown, ipn, st);
			continue;
		}
		const Batch bt{s->nb, L.npts};
		switch (s->st.relaxation) {
		case CEDAR_AMD_RELAX_POINT:
			// nine-point levels of at least 4096 rows: the band-fused sweep with inter-row partial sums (relax2d.hip)
			with_cycle_view2(
			    L,
			    [&](const Op2f &A) {
				    if (L.nst == 5 && relax2_psum_wanted(L.II, L.JJ)) relax2_gs9_psum_op(A, b, x, L.II, L.JJ, updown, st, bt);
				    else relax2_gs_op(A, b, x, L.II, L.JJ, L.nst, updown, st, bt);
			    },
			    [&]() {
				    if (L.nst == 5 && relax2_psum_wanted(L.II, L.JJ)) relax2_gs9_psum(L.A, b, x, L.SOR0, L.II, L.JJ, updown, st, bt);
				    else relax2_gs(L.A, b, x, L.SOR0, L.II, L.JJ, L.nst, updown, st, bt);
			    });
			break;
		case CEDAR_AMD_RELAX_LINE_X: lines_x(L, x, b, updown, ipn, st, bt); break;
		case CEDAR_AMD_RELAX_LINE_Y: lines_y(L, x, b, L.SOR0, updown, ipn, st, bt); break;
		default:
			if (updown == BMG_DOWN) {
				lines_x(L, x, b, updown, ipn, st, bt);
				lines_y(L, x, b, L.SOR1, updown, ipn, st, bt);
			} else {
				lines_y(L, x, b, L.SOR1, updown, ipn, st, bt);
				lines_x(L, x, b, updown, ipn, st, bt);
			}
		}
	}
}

// the side streams of plane relaxation with their fork / join events; CEDAR_AMD_PLANE_STREAMS: how many (1 .. 64, default 8)
void plane_streams_create(cedar_amd_solver *s)
{
	const char *es = getenv("CEDAR_AMD_PLANE_STREAMS");
	int S = es ? atoi(es) : 8;
	S = S < 1 ? 1 : S > 64 ? 64 : S;
	s->pstreams.resize(S);
	s->pevents.resize(S);
	for (int t = 0; t < S; t++) {
		CEDAR_HIP_CHECK(hipStreamCreateWithFlags(&s->pstreams[t], hipStreamNonBlocking));
		CEDAR_HIP_CHECK(hipEventCreateWithFlags(&s->pevents[t], hipEventDisableTiming));
	}
	CEDAR_HIP_CHECK(hipEventCreateWithFlags(&s->pfork, hipEventDisableTiming));
}

void coarse_solve(cedar_amd_solver *s, real_t *x, const real_t *b, hipStream_t st)
{
	const Level &C = s->lv.back();
	const Batch bt{s->nb, C.npts};
	if (s->nd == 2 && s->st.ibc) solve_cg2_per(x, b, C.II, C.JJ, s->ABD, s->bbd, s->nabd1, s->st.ibc, st, bt);
	else if (s->nd == 2) solve_cg2(x, b, C.II, C.JJ, s->ABD, s->bbd, s->nabd1, s->nabd2, st, bt, s->semidef);
	else if (s->st.ibc) solve_cg3_per(x, b, C.II, C.JJ, C.KK, s->ABD, s->bbd, s->nabd1, s->st.ibc, st, bt);
	else solve_cg3(x, b, C.II, C.JJ, C.KK, s->ABD, s->bbd, s->nabd1, s->nabd2, st, bt, s->semidef);
}

// The LDS-resident small-level kernels serve the visit of 2D level L (lines_small.hip): each half of the visit is one launch
// that fuses the transfers and reads the FP64 K.P.  A level that keeps a float copy of its operator runs the row kernels on
// it: the copy's presence decides, before the small-level path.
bool visit_fused(const cedar_amd_solver *s, const Level &L)
{
	return s->nd == 2 && s->st.ibc == 0 && s->st.relaxation <= CEDAR_AMD_RELAX_LINE_XY && !L.A2f && lines_small_ok(L.II, L.JJ);
}

// The transfers between a level L and the next coarser K, the one place that chooses their kernels by dimension, boundary
// code and batch count.  restrict_to: K.b := P^T src; the periodic kernels first refresh the ghosts of src (restrict.f90:
// 78-103), so it is not const.  interp_add_from: x += P K.x, with the residual correction from L.res.  Where K keeps the
// single-precision copy of its weights (cedar_amd_solver_use_fp32_interpolation: Dirichlet handles only) both read it;
// the diagonal interp_add divides by is the FP64 one always.  A level pair whose visit is fused never took the copy; should
// its fine level return to that path (cedar_amd_solver_set dropped its operator copy), the F-cycle's transfers follow it.
void restrict_to(const cedar_amd_solver *s, const Level &L, const Level &K, real_t *src, hipStream_t st)
{
	const int ibc = s->st.ibc;
	const Batch bf{s->nb, L.npts}, bc{s->nb, K.npts};
	const bool p32 = K.P32 && !visit_fused(s, L);
	if (p32 && s->nd == 2) restrict2_ci(ci32_view(K.P32, K.II, K.JJ), src, K.b, L.II, L.JJ, K.II, K.JJ, st, bf, bc);
	else if (p32) restrict3_ci(ci32_view(K.P32, K.II, K.JJ, K.KK), src, K.b, L.II, L.JJ, L.KK, K.II, K.JJ, K.KK, st, bf, bc);
	else if (s->nd == 2 && ibc) restrict2_per(src, K.b, K.P, L.II, L.JJ, K.II, K.JJ, ibc, st, bf, bc);
	else if (s->nd == 2) restrict2(src, K.b, K.P, L.II, L.JJ, K.II, K.JJ, st, bf, bc);
	else if (ibc && s->nb > 1) restrict3_per_many(src, K.b, K.P, L.II, L.JJ, L.KK, K.II, K.JJ, K.KK, ibc, st, bf, bc);
	else if (ibc) restrict3_per(src, K.b, K.P, L.II, L.JJ, L.KK, K.II, K.JJ, K.KK, ibc, st);
	else if (s->nb > 1) restrict3_many(src, K.b, K.P, L.II, L.JJ, L.KK, K.II, K.JJ, K.KK, st, bf, bc);
	else restrict3(src, K.b, K.P, L.II, L.JJ, L.KK, K.II, K.JJ, K.KK, st);
}

void interp_add_from(const cedar_amd_solver *s, const Level &L, const Level &K, real_t *x, hipStream_t st)
{
	const int ibc = s->st.ibc;
	const Batch bf{s->nb, L.npts}, bc{s->nb, K.npts};
	const bool p32 = K.P32 && !visit_fused(s, L);
	if (p32 && s->nd == 2) interp_add2_ci(ci32_view(K.P32, K.II, K.JJ), x, K.x, L.res, L.A, K.II, K.JJ, L.II, L.JJ, st, bf, bc);
	else if (p32)
		interp_add3_ci(ci32_view(K.P32, K.II, K.JJ, K.KK), x, K.x, L.A, L.res, K.II, K.JJ, K.KK, L.II, L.JJ, L.KK, st, bf, bc);
	else if (s->nd == 2 && ibc) interp_add2_per(x, K.x, L.res, L.A, K.P, K.II, K.JJ, L.II, L.JJ, ibc, st, bf, bc);
	else if (s->nd == 2) interp_add2(x, K.x, L.res, L.A, K.P, K.II, K.JJ, L.II, L.JJ, st, bf, bc);
	else if (ibc && s->nb > 1)
		interp_add3_per_many(x, K.x, L.A, L.res, K.P, K.II, K.JJ, K.KK, L.II, L.JJ, L.KK, ibc, st, bf, bc);
	else if (ibc) interp_add3_per(x, K.x, L.A, L.res, K.P, K.II, K.JJ, K.KK, L.II, L.JJ, L.KK, ibc, st);
	else if (s->nb > 1) interp_add3_many(x, K.x, L.A, L.res, K.P, K.II, K.JJ, K.KK, L.II, L.JJ, L.KK, st, bf, bc);
	else interp_add3(x, K.x, L.A, L.res, K.P, K.II, K.JJ, K.KK, L.II, L.JJ, L.KK, st);
}

void ncycle(cedar_amd_solver *s, int lvl, real_t *x, const real_t *b, hipStream_t st)
{
	Level &L = s->lv[lvl], &K = s->lv[lvl + 1];
	L.bt_fresh = false; // b of this visit has not been transposed yet
	// a small 2D level: each half of the visit is one launch with the level resident in LDS (lines_small.hip)
	const bool small = visit_fused(s, L);
	const int kind = s->st.relaxation == CEDAR_AMD_RELAX_POINT ? 0 : s->st.relaxation == CEDAR_AMD_RELAX_LINE_X ? 1
	               : s->st.relaxation == CEDAR_AMD_RELAX_LINE_Y ? 2 : 3;
	const real_t *sory = kind == 2 ? L.SOR0 : L.SOR1;
	if (small) {
		visit_small(1, L.A, b, x, L.res, L.SOR0, sory, L.II, L.JJ, L.nst, kind, s->st.nrelax_pre, K.P, K.b, K.x, K.II, K.JJ, st,
		            Batch{s->nb, L.npts}, Batch{s->nb, K.npts});
	} else {
	smooth(s, L, x, b, BMG_DOWN, s->st.nrelax_pre, st);
	residual(s, L, x, b, L.res, st);
	restrict_to(s, L, K, L.res, st);
	clear(K.x, K.npts * (size_t)s->nb, st); // coarse_x.set(0.0)
	}
	if (lvl + 1 == (int)s->lv.size() - 1) coarse_solve(s, K.x, K.b, st);
	else ncycle(s, lvl + 1, K.x, K.b, st);
	if (small) {
		visit_small(0, L.A, b, x, L.res, L.SOR0, sory, L.II, L.JJ, L.nst, kind, s->st.nrelax_post, K.P, nullptr, K.x, K.II, K.JJ, st,
		            Batch{s->nb, L.npts}, Batch{s->nb, K.npts});
		return;
	}
	interp_add_from(s, L, K, x, st);
	smooth(s, L, x, b, BMG_UP, s->st.nrelax_post, st);
}

// full-multigrid cycle, include/cedar/cycle/fcycle.h:49-83: restrict the right-hand side itself down
// to the coarsest level, solve there, and on the way up interpolate (x = P x_c: interp_add onto
// x = 0 with a zero "residual") and run one V-cycle from that level.
void fmg_cycle(cedar_amd_solver *s, int lvl, real_t *x, const real_t *b, hipStream_t st)
{
	if (lvl == (int)s->lv.size() - 1) {
		coarse_solve(s, x, b, st);
		return;
	}
	Level &L = s->lv[lvl], &K = s->lv[lvl + 1];
	// the transfers of the V-cycle (an F-cycle handle holds one right-hand side: solver_create); the periodic restriction
	// refreshes the ghosts of the vector it restricts -- here the right-hand side itself, which the reference's binding
	// reaches through a const_cast
	restrict_to(s, L, K, const_cast<real_t *>(b), st);
	fmg_cycle(s, lvl + 1, K.x, K.b, st);
	zero_fill(x, L.npts, st);
	zero_fill(L.res, L.npts, st);
	interp_add_from(s, L, K, x, st);
	ncycle(s, lvl, x, b, st);
}

void cycle_launch(cedar_amd_solver *s, real_t *x, const real_t *b, hipStream_t st)
{
	if (s->lv.size() == 1) coarse_solve(s, x, b, st); // vcycle.h:37-38, fcycle.h:42-43
	else if (s->st.cycle == 1) fmg_cycle(s, 0, x, b, st);
	else ncycle(s, 0, x, b, st);
}

// milliseconds, by HIP events, of what fn enqueues on st
template <class F> float timed(hipStream_t st, F fn)
{
	hipEvent_t e0, e1;
	CEDAR_HIP_CHECK(hipEventCreate(&e0));
	CEDAR_HIP_CHECK(hipEventCreate(&e1));
	CEDAR_HIP_CHECK(hipEventRecord(e0, st));
	fn();
	CEDAR_HIP_CHECK(hipEventRecord(e1, st));
	CEDAR_HIP_CHECK(hipEventSynchronize(e1));
	float ms = 0;
	CEDAR_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
	(void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
	return ms;
}

// run one V-cycle on device pointers: graph replay when possible
void cycle_dev(cedar_amd_solver *s, real_t *x, const real_t *b) { cycle_on(s, x, b, current_stream()); }

// make s->gexec the instantiated graph of one cycle on (x, b) with the current batch count; returns true if it had to be
// recorded.  `st`: the stream earlier replays of this solver's graph were launched on (drained before a stale graph goes).
bool graph_prepare(cedar_amd_solver *s, real_t *x, const real_t *b, hipStream_t st)
{
	if (s->gexec && (s->gx != x || s->gb != b)) {
		CEDAR_HIP_CHECK(hipStreamSynchronize(st)); // a replay of the old graph may still be running
		CEDAR_HIP_CHECK(hipGraphExecDestroy(s->gexec));
		s->gexec = nullptr;
		if (s->gexec2) CEDAR_HIP_CHECK(hipGraphExecDestroy(s->gexec2));
		s->gexec2 = nullptr;
	}
	if (s->gexec && s->gnb != s->nb) { // the other captured batch count (the two colours of a plane sweep)
		if (s->gexec2 && s->gnb2 == s->nb) {
			std::swap(s->gexec, s->gexec2);
			std::swap(s->gnb, s->gnb2);
		} else {
			if (s->gexec2) CEDAR_HIP_CHECK(hipGraphExecDestroy(s->gexec2));
			s->gexec2 = s->gexec; s->gnb2 = s->gnb;
			s->gexec = nullptr;
		}
	}
	if (s->gexec) return false;
	{
		// one capture stream for the process: captures are recorded synchronously (thread-local mode), and plane
		// relaxation keeps hundreds of small solvers whose graphs are all recorded through here
		static hipStream_t capture_stream = nullptr;
		if (!capture_stream) CEDAR_HIP_CHECK(hipStreamCreateWithFlags(&capture_stream, hipStreamNonBlocking));
		s->gstream = capture_stream;
		// one eager cycle first is NOT wanted (it would change x); capture records without executing
		CEDAR_HIP_CHECK(hipStreamSynchronize(st));
		hipGraph_t g = nullptr;
		CEDAR_HIP_CHECK(hipStreamBeginCapture(s->gstream, hipStreamCaptureModeThreadLocal));
		cycle_launch(s, x, b, s->gstream);
		CEDAR_HIP_CHECK(hipStreamEndCapture(s->gstream, &g));
		CEDAR_HIP_CHECK(hipGraphInstantiate(&s->gexec, g, nullptr, nullptr, 0));
		CEDAR_HIP_CHECK(hipGraphDestroy(g));
		s->gx = x; s->gb = b; s->gnb = s->nb;
	}
	return true;
}

void cycle_on(cedar_amd_solver *s, real_t *x, const real_t *b, hipStream_t st)
{
	if (!s->use_graph) {
		cycle_launch(s, x, b, st);
		return;
	}
	graph_prepare(s, x, b, st);
	CEDAR_HIP_CHECK(hipGraphLaunch(s->gexec, st));
}

} // namespace

// cedar_amd_solver_create_semidefinite's condition on the operator, checked on level 0 before any set-up: A 1 with the
// vector of ones wrapped in the periodic directions and zero in the other ghosts, by the matrix-vector kernels the
// cycle's tests use.  max_i |(A 1)_i| <= 1024 eps max_i |a_ii|: a row has at most 27 terms, so its rounded sum lies within
// 54 eps of the diagonal; the factor of about 20 on top covers how callers assemble their coefficients.  A condition, not
// a measurement.
static bool null_space_is_constants(const cedar_amd_solver *s, hipStream_t st)
{
	const Level &L = s->lv[0];
	const PerDirs pd = per_dirs(s->nd, s->st.ibc);
	std::vector<real_t> h(L.npts);
	for (int k = 0; k < L.KK; k++)
		for (int j = 0; j < L.JJ; j++)
			for (int i = 0; i < L.II; i++) {
				const bool in = (pd.x || (i > 0 && i < L.II - 1)) && (pd.y || (j > 0 && j < L.JJ - 1))
				                && (pd.z || s->nd == 2 || (k > 0 && k < L.KK - 1));
				h[(size_t)i + (size_t)L.II * ((size_t)j + (size_t)L.JJ * k)] = in ? 1.0 : 0.0;
			}
	// set-up only: two level-0 vectors on the device and two on the host for the length of this call (a failing
	// CEDAR_HIP_CHECK aborts the process, so there is no path that returns without the two frees below); a max-reduction
	// on the device would spare the host copies
	real_t *ones = dalloc_raw(L.npts), *a1 = dalloc(L.npts);
	CEDAR_HIP_CHECK(hipMemcpyAsync(ones, h.data(), L.npts * sizeof(real_t), hipMemcpyHostToDevice, st));
	if (s->nd == 2) matvec2(L.A, ones, a1, L.II, L.JJ, L.nst, st);
	else matvec3(L.A, ones, a1, L.II, L.JJ, L.KK, L.nst, st);
	std::vector<real_t> d(L.npts);
	CEDAR_HIP_CHECK(hipMemcpyAsync(h.data(), a1, L.npts * sizeof(real_t), hipMemcpyDeviceToHost, st));
	CEDAR_HIP_CHECK(hipMemcpyAsync(d.data(), L.A, L.npts * sizeof(real_t), hipMemcpyDeviceToHost, st)); // the diagonal: slot 0
	CEDAR_HIP_CHECK(hipStreamSynchronize(st));
	(void)hipFree(ones); (void)hipFree(a1);
	real_t worst = 0.0, diag = 0.0;
	bool finite = true;
	for (int k = s->nd == 3 ? 1 : 0; k < (s->nd == 3 ? L.KK - 1 : 1); k++)
		for (int j = 1; j < L.JJ - 1; j++)
			for (int i = 1; i < L.II - 1; i++) {
				const size_t x = (size_t)i + (size_t)L.II * ((size_t)j + (size_t)L.JJ * k);
				finite = finite && std::isfinite(h[x]) && std::isfinite(d[x]);
				worst = std::max(worst, std::fabs(h[x]));
				diag = std::max(diag, std::fabs(d[x]));
			}
	return finite && worst <= 1024.0 * std::numeric_limits<real_t>::epsilon() * diag;
}

extern "C" {

void cedar_amd_default_settings(cedar_amd_settings *s)
{
	s->relaxation = CEDAR_AMD_RELAX_POINT;
	s->nrelax_pre = 2;
	s->nrelax_post = 1;
	s->num_levels = -1;
	s->max_iter = 10;
	s->tol = 1e-8;
	s->min_coarse = 3;
	s->cycle = 0;
	s->ibc = 0;
	s->plane_relaxation = CEDAR_AMD_RELAX_LINE_XY; // src/kernel_params.cc:72-78
	s->plane_nrelax_pre = 2;
	s->plane_nrelax_post = 1;
	s->plane_max_iter = 1;
	s->plane_min_coarse = 3;
	s->plane_tol = 1e-8;
}

cedar_amd_solver *cedar_amd_solver_create(int nd, len_t nx, len_t ny, len_t nz, int nstencil,
                                          const real_t *so, int own_device_so,
                                          const cedar_amd_settings *settings)
{
	return solver_create(nd, nx, ny, nz, nstencil, so, own_device_so, settings, 1);
}

} // extern "C"

static cedar_amd_solver *solver_create(int nd, len_t nx, len_t ny, len_t nz, int nstencil, const real_t *so, int own_device_so,
                                       const cedar_amd_settings *settings, int batch, bool periodic_batch, bool semidef)
{
	hipStream_t st = current_stream();
	cedar_amd_solver *s = new cedar_amd_solver;
	s->nd = nd;
	s->nb_alloc = batch < 1 ? 1 : batch;
	if (settings) s->st = *settings;
	else cedar_amd_default_settings(&s->st);
	const bool planes = s->st.relaxation >= CEDAR_AMD_RELAX_PLANE_XY && s->st.relaxation <= CEDAR_AMD_RELAX_PLANE_XYZ;
	if ((nd == 3 && s->st.relaxation != CEDAR_AMD_RELAX_POINT && !planes) || (nd == 2 && planes)
	    || (planes && (s->st.ibc != 0 || s->st.plane_relaxation >= CEDAR_AMD_RELAX_PLANE_XY))) {
		char msg[] = "cedar_amd_solver_create: relaxation must be point / line-x / line-y / line-xy in 2D and point or "
		             "plane-xy / -xz / -yz / -xyz in 3D (planes: Dirichlet boundaries, a 2D relaxation in the plane "
		             "configuration); point relaxation is used";
		print_error(msg);
		s->st.relaxation = CEDAR_AMD_RELAX_POINT;
	}
	if (s->st.relaxation >= CEDAR_AMD_RELAX_PLANE_XY) {
		// the plane solves of a colour run on side streams and replay graphs of their own: the 3D cycle is launched
		// eagerly (capturing it would nest graph launches)
		s->use_graph = false;
		plane_streams_create(s);
	}
	if (s->st.ibc != 0) {
		// periodic boundary conditions (V- and F-cycles).  2D: ibc 1..3, point relaxation keeps a row in the default LDS
		// window; 3D: ibc 1..3, 5..8 (BMG_get_bc.f90:13-20), even extents in the periodic directions on every level
		// that is coarsened (checked below, once the level sizes are known)
		const bool ok2 = nd == 2 && s->st.ibc >= 1 && s->st.ibc <= 3
		                 && (s->st.relaxation != CEDAR_AMD_RELAX_POINT || (size_t)(nx + 2) * sizeof(real_t) <= 64 * 1024);
		const bool ok3 = nd == 3 && s->st.ibc > 0 && periodic3_code_ok(s->st.ibc);
		if (!ok2 && !ok3) {
			char msg[] = "cedar_amd_solver_create: periodic boundary conditions are implemented for the definite periodic codes "
			             "(2D: ibc 1..3, point relaxation: rows up to 8190 points; 3D: ibc 1..3, 5..8); no solver created";
			print_error(msg);
			delete s;
			return nullptr;
		}
	}
	if (const char *e = getenv("CEDAR_AMD_NO_GRAPH")) s->use_graph = s->use_graph && !(e[0] == '1');
	int nlev = compute_num_levels(nd, nx, ny, nz, s->st.min_coarse);
	if (s->st.num_levels > 0) {
		if (s->st.num_levels > nlev) {
			char msg[] = "too many levels specified";
			print_error(msg);
		} else
			nlev = s->st.num_levels;
	}
	s->lv.resize(nlev);
	const bool ly = nd == 2 && (s->st.relaxation == CEDAR_AMD_RELAX_LINE_XY || s->st.relaxation == CEDAR_AMD_RELAX_LINE_Y);
	// y-lines run on transposed arrays unless periodic (the wraps and the cyclic closure stay on relax_lines_y);
	// CEDAR_AMD_YLINES_TRANSPOSED=0 keeps the gather / solve / scatter pipeline for cross-checks
	const char *eyt = getenv("CEDAR_AMD_YLINES_TRANSPOSED");
	const bool lyt = ly && s->st.ibc == 0 && !(eyt && atoi(eyt) == 0);
	// batches (see the struct): Dirichlet V-cycles; 2D with the y-lines on transposed arrays, 3D point relaxation; periodic
	// only where cedar_amd_solver_create_many_periodic (3D) or _periodic2 (2D) asked (they have checked cycle and
	// relaxation); a periodic 2D batch keeps its y-lines on relax_lines_y and walks the items through it
	s->per_batch = periodic_batch && s->st.ibc != 0;
	if (s->nb_alloc > 1 && ((s->st.ibc != 0 && !s->per_batch) || s->st.cycle != 0 || (ly && !lyt && !s->per_batch) || (nd == 3 && s->st.relaxation != CEDAR_AMD_RELAX_POINT)))
		s->nb_alloc = 1;
	level_init(s->lv[0], nd, (int)nx, (int)ny, (int)nz, nstencil, false, ly, lyt, s->nb_alloc);
	Level &F0 = s->lv[0];
	if (own_device_so && is_device_ptr(so)) {
		F0.A = const_cast<real_t *>(so);
		F0.ownA = false;
	} else {
		F0.A = dalloc(F0.npts * nstencil);
		CEDAR_HIP_CHECK(hipMemcpyAsync(F0.A, so, F0.npts * nstencil * sizeof(real_t),
		                               is_device_ptr(so) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
	}
	if (semidef) {
		// before any set-up: the null space must be the constants (null_space_is_constants)
		if (!null_space_is_constants(s, st)) {
			char msg[] = "cedar_amd_solver_create_semidefinite: the operator's null space is not the constants: max |A 1| "
			             "exceeds 1024 eps max |a_ii| (ones wrapped in the periodic directions, zero in the other ghosts); "
			             "no solver created";
			print_error(msg);
			cedar_amd_solver_destroy(s);
			return nullptr;
		}
		s->semidef = true;
		s->pm = dalloc_raw(project_mean_doubles(s->nb_alloc));
	}
	for (int l = 1; l < nlev; l++) {
		const Level &F = s->lv[l - 1];
		int nxc = (int)((F.nx - 1) / 2. + 1), nyc = (int)((F.ny - 1) / 2. + 1);
		int nzc = nd == 3 ? (int)((F.nz - 1) / 2. + 1) : 1;
		level_init(s->lv[l], nd, nxc, nyc, nzc, nd == 3 ? 14 : 5, true, ly, lyt, s->nb_alloc);
	}
	const Level &C = s->lv.back();
	// periodic: the coarsest operator is stored dense (include/cedar/2d/solver.h:110-114)
	if (nd == 2) { s->nabd1 = s->st.ibc ? C.nx * C.ny : C.nx + 2; s->nabd2 = C.nx * C.ny; }
	else { s->nabd1 = s->st.ibc ? C.nx * C.ny * C.nz : C.nx * (C.ny + 1) + 2; s->nabd2 = C.nx * C.ny * C.nz; } // 3d/solver.h:118-121
	if (nd == 3 && s->st.ibc) {
		const PerDirs pd = per_dirs(3, s->st.ibc);
		bool ok = (size_t)s->nabd2 <= 2048; // dense factor in ONE workgroup: n^2 doubles, n^3/3 flops (2048: ~3 GFlop, about a second)
		for (int l = 0; l + 1 < nlev; l++)
			ok = ok && !(pd.x && (s->lv[l].nx & 1)) && !(pd.y && (s->lv[l].ny & 1)) && !(pd.z && (s->lv[l].nz & 1));
		if (!ok) {
			char msg[] = "cedar_amd_solver_create: 3D periodic boundary conditions need an even extent in every periodic "
			             "direction on each level that is coarsened (choose the extents or num_levels accordingly) and at "
			             "most 2048 unknowns on the coarsest level (it is factored densely by one workgroup: use more levels); no solver created";
			print_error(msg);
			cedar_amd_solver_destroy(s); // releases the levels allocated so far
			return nullptr;
		}
	}
	s->ABD = dalloc((size_t)s->nabd1 * s->nabd2);
	s->bbd = dalloc((size_t)s->nabd2 * s->nb_alloc);
	s->red = dalloc(4100 + (size_t)s->nb_alloc); // 4096 partials, then one sum of squares per batch item
	CEDAR_HIP_CHECK(hipMalloc((void **)&s->dinfo, 64));
	CEDAR_HIP_CHECK(hipMemsetAsync(s->dinfo, 0, 64, st));

	for (int l = 0; l < nlev - 1; l++) {
		Level &F = s->lv[l], &K = s->lv[l + 1];
		if (nd == 2) {
			int ifd = F.nst == 3;
			if (s->st.ibc) {
				setup_interp2_per(F.A, K.P, F.II, F.JJ, K.II, K.JJ, ifd, s->st.ibc, st);
				galerkin2_per(F.A, K.A, K.P, F.II, F.JJ, K.II, K.JJ, ifd, s->st.ibc, st);
			} else {
				setup_interp2(F.A, K.P, F.II, F.JJ, K.II, K.JJ, ifd, st);
				galerkin2(F.A, K.A, K.P, F.II, F.JJ, K.II, K.JJ, ifd, st);
			}
			switch (s->st.relaxation) {
			case CEDAR_AMD_RELAX_POINT: setup_recip(F.A, F.SOR0 + F.npts, F.II, F.JJ, 1, st); break;
			case CEDAR_AMD_RELAX_LINE_X: setup_lines_x(F.A, F.SOR0, F.II, F.JJ, st, per_dirs(2, s->st.ibc).x); break;
			case CEDAR_AMD_RELAX_LINE_Y: setup_lines_y(F.A, F.SOR0, F.II, F.JJ, st, per_dirs(2, s->st.ibc).y); break;
			default:
				setup_lines_x(F.A, F.SOR0, F.II, F.JJ, st, per_dirs(2, s->st.ibc).x);
				setup_lines_y(F.A, F.SOR1, F.II, F.JJ, st, per_dirs(2, s->st.ibc).y);
			}
			if (F.At) setup_lines_yt(F.A, F.At, F.II, F.JJ, F.nst, st);
			if (s->st.ibc == 0 && !(getenv("CEDAR_AMD_LINE_PERM") && atoi(getenv("CEDAR_AMD_LINE_PERM")) == 0)) {
				// scan-ordered factor copies for the long-line kernel (Dirichlet; periodic lines keep the SOR reads)
				const int rx = s->st.relaxation;
				if (rx == CEDAR_AMD_RELAX_LINE_X || rx == CEDAR_AMD_RELAX_LINE_XY) {
					const size_t nd_ = lines_permuted_doubles(F.II - 2, F.JJ - 2);
					if (nd_) { F.PFx = dalloc_raw(nd_); lines_permute(F.SOR0, F.PFx, F.II - 2, F.II, F.JJ - 2, F.npts, st); }
				}
				if (F.At) { // y factors: SOR(JJ,II,2) in SOR0 (line-y) or SOR1 (line-xy)
					const real_t *sy = rx == CEDAR_AMD_RELAX_LINE_Y ? F.SOR0 : F.SOR1;
					const size_t nd_ = lines_permuted_doubles(F.JJ - 2, F.II - 2);
					if (nd_) { F.PFy = dalloc_raw(nd_); lines_permute(sy, F.PFy, F.JJ - 2, F.JJ, F.II - 2, F.npts, st); }
				}
			}
		} else {
			int ifd = F.nst == 4;
			if (s->st.ibc) {
				setup_interp3_per(F.A, K.P, F.II, F.JJ, F.KK, K.II, K.JJ, K.KK, ifd, s->st.ibc, st);
				galerkin3_per(F.A, K.A, K.P, F.II, F.JJ, F.KK, K.II, K.JJ, K.KK, ifd, s->st.ibc, st);
			} else {
				setup_interp3(F.A, K.P, F.II, F.JJ, F.KK, K.II, K.JJ, K.KK, ifd, st);
				galerkin3(F.A, K.A, K.P, F.II, F.JJ, F.KK, K.II, K.JJ, K.KK, ifd, st);
			}
			if (s->st.relaxation >= CEDAR_AMD_RELAX_PLANE_XY) { // multilevel.h:149-159
				cedar_amd_settings pst;
				cedar_amd_default_settings(&pst);
				pst.relaxation = s->st.plane_relaxation; pst.nrelax_pre = s->st.plane_nrelax_pre;
				pst.nrelax_post = s->st.plane_nrelax_post; pst.max_iter = s->st.plane_max_iter;
				pst.tol = s->st.plane_tol; pst.min_coarse = s->st.plane_min_coarse;
				for (int d = 0; d < 3; d++)
					if (s->st.relaxation == CEDAR_AMD_RELAX_PLANE_XYZ || s->st.relaxation == CEDAR_AMD_RELAX_PLANE_XY + d)
						F.pl[d] = planes_setup(d, F.A, F.II, F.JJ, F.KK, F.nst, pst, st);
				continue;
			}
			setup_recip(F.A, F.SOR0 + F.npts, F.II, F.JJ, F.KK, st);
			if (F.nst == 14 && !s->st.ibc && ilv_level_wanted(F.II, F.JJ, F.KK, ilv_min_rows_env())) {
				F.Ailv = dalloc_raw(ilv_doubles(F.II, F.JJ, F.KK));
				ilv_build(F.A, F.SOR0 + F.npts, F.Ailv, F.II, F.JJ, F.KK, st);
			}
			// partial-sum scratch of the relax sweep: T is read only where the sweep wrote it, not cleared
			if (F.nst == 14 && !s->st.ibc && relax3_psum_wanted(F.II, F.JJ, F.KK)) F.T = dalloc_raw(F.npts);
		}
	}
	// (a semidefinite handle: the last unknown's diagonal entry is doubled before the factorisation)
	if (nd == 2 && s->st.ibc) setup_cg2_per(C.A, C.II, C.JJ, C.nst, s->ABD, s->nabd1, s->st.ibc, s->dinfo, st, s->semidef);
	else if (nd == 2) setup_cg2(C.A, C.II, C.JJ, C.nst, s->ABD, s->nabd1, s->nabd2, s->dinfo, st, s->semidef);
	else if (s->st.ibc) setup_cg3_per(C.A, C.II, C.JJ, C.KK, s->ABD, s->nabd1, s->st.ibc, s->dinfo, st, C.nst, s->semidef);
	else setup_cg3(C.A, C.II, C.JJ, C.KK, C.nst, s->ABD, s->nabd1, s->nabd2, s->dinfo, st, s->semidef);
	int info = 0;
	CEDAR_HIP_CHECK(hipMemcpyAsync(&info, s->dinfo, sizeof(int), hipMemcpyDeviceToHost, st));
	CEDAR_HIP_CHECK(hipStreamSynchronize(st));
	if (info != 0) {
		char msg[] = "Coarse grid Cholesky decomp failed!";
		print_error(msg);
	}
	launch_check("cedar_amd_solver_create");
	return s;
}

extern "C" {

void cedar_amd_solver_destroy(cedar_amd_solver *s)
{
	if (!s) return;
	CEDAR_HIP_CHECK(hipDeviceSynchronize());
	if (s->gexec) CEDAR_HIP_CHECK(hipGraphExecDestroy(s->gexec));
	if (s->gexec2) CEDAR_HIP_CHECK(hipGraphExecDestroy(s->gexec2));
	for (size_t l = 0; l < s->lv.size(); l++) {
		Level &L = s->lv[l];
		for (int d = 0; d < 3; d++) planes_destroy(L.pl[d]);
		if (L.ownA) (void)hipFree(L.A);
		if (!L.shared) {
			(void)hipFree(L.P); (void)hipFree(L.SOR0); (void)hipFree(L.SOR1); (void)hipFree(L.At); (void)hipFree(L.Ailv);
			(void)hipFree(L.A32);
			(void)hipFree(L.A7f);
			(void)hipFree(L.A2f);
			(void)hipFree(L.P32);
			(void)hipFree(L.At2f); (void)hipFree(L.Fx32); (void)hipFree(L.Fy32); (void)hipFree(L.PFx32); (void)hipFree(L.PFy32);
			(void)hipFree(L.PFx); (void)hipFree(L.PFy);
		}
		(void)hipFree(L.res); (void)hipFree(L.yscr); (void)hipFree(L.bt); (void)hipFree(L.xt); (void)hipFree(L.T);
		if (l > 0) { (void)hipFree(L.x); (void)hipFree(L.b); }
	}
	(void)hipFree(s->kr); (void)hipFree(s->kz); (void)hipFree(s->kw); (void)hipFree(s->kp[0]); (void)hipFree(s->kp[1]);
	(void)hipFree(s->kslab); (void)hipFree(s->ksc);
	if (!s->shared_abd) (void)hipFree(s->ABD);
	(void)hipFree(s->bbd); (void)hipFree(s->red); (void)hipFree(s->dinfo); (void)hipFree(s->pm);
	for (auto t : s->pstreams) (void)hipStreamDestroy(t);
	for (auto e : s->pevents) (void)hipEventDestroy(e);
	if (s->pfork) (void)hipEventDestroy(s->pfork);
	delete s;
}

// every entry point below tolerates the NULL that cedar_amd_solver_create returns for unsupported settings:
// it reports through print_error and does nothing (the reference never aborts either)
static bool null_handle(const void *s, const char *who)
{
	if (s) return false;
	char msg[160];
	snprintf(msg, sizeof(msg), "%s: NULL solver handle (cedar_amd_solver_create reported why no solver was created)", who);
	print_error(msg);
	return true;
}

// what a handle of cedar_amd_solver_create_semidefinite is not served by: the Krylov calls that do not project, the bare
// preconditioner and the single-precision switches.  Reported, nothing written
static bool semidef_refused(const cedar_amd_solver *s, const char *who, const char *tail = "nothing done")
{
	if (!s->semidef) return false;
	char msg[256];
	snprintf(msg, sizeof(msg), "%s: a semidefinite handle (cedar_amd_solver_create_semidefinite) is served by "
	                           "cedar_amd_solver_fcg_semidefinite / _many only; %s", who, tail);
	print_error(msg);
	return true;
}

int cedar_amd_solver_nlevels(const cedar_amd_solver *s) { return null_handle(s, "cedar_amd_solver_nlevels") ? 0 : (int)s->lv.size(); }

void cedar_amd_solver_level_dims(const cedar_amd_solver *s, int lvl, len_t *nx, len_t *ny, len_t *nz)
{
	*nx = *ny = *nz = 0;
	if (null_handle(s, "cedar_amd_solver_level_dims") || lvl < 0 || lvl >= (int)s->lv.size()) return;
	*nx = s->lv[lvl].nx; *ny = s->lv[lvl].ny; *nz = s->lv[lvl].nz;
}

size_t cedar_amd_solver_get(const cedar_amd_solver *s, int lvl, const char *what, real_t *out)
{
	if (null_handle(s, "cedar_amd_solver_get") || lvl < 0 || lvl >= (int)s->lv.size()) return 0;
	const Level &L = s->lv[lvl];
	const real_t *src = nullptr;
	size_t n = 0;
	if (!strcmp(what, "A")) { src = L.A; n = L.npts * L.nst; }
	else if (!strcmp(what, "P")) { src = L.P; n = L.P ? L.npts * (s->nd == 3 ? 26 : 8) : 0; }
	else if (!strcmp(what, "SOR0")) { src = L.SOR0; n = L.npts * 2; }
	else if (!strcmp(what, "SOR1")) { src = L.SOR1; n = L.SOR1 ? L.npts * 2 : 0; }
	else if (!strcmp(what, "ABD")) { src = s->ABD; n = (size_t)s->nabd1 * s->nabd2; }
	else if (!strcmp(what, "res")) { src = L.res; n = L.npts; }
	else if (!strcmp(what, "x")) { src = L.x; n = L.x ? L.npts : 0; } // coarse levels only: level 0 uses the caller's
	else if (!strcmp(what, "b")) { src = L.b; n = L.b ? L.npts : 0; }
	if (out && n) cedar_amd_memcpy_d2h(out, src, n * sizeof(real_t));
	return n;
}

static void pcg_alloc(cedar_amd_solver *s, int items = 1);
static void pcg_precondition(cedar_amd_solver *s, int nmg, hipStream_t st);

// ---- single-precision operator copies (include/cedar_amd.h cedar_amd_solver_use_fp32_operator)
static int fp32_count(const cedar_amd_solver *s)
{
	int n = 0;
	for (const Level &L : s->lv) n += (L.A32 || L.A7f || L.A2f) ? 1 : 0;
	return n;
}

// no captured cycle survives a change of the arrays its launches name
static void graphs_drop(cedar_amd_solver *s)
{
	CEDAR_HIP_CHECK(hipDeviceSynchronize());
	if (s->gexec) CEDAR_HIP_CHECK(hipGraphExecDestroy(s->gexec));
	if (s->gexec2) CEDAR_HIP_CHECK(hipGraphExecDestroy(s->gexec2));
	s->gexec = s->gexec2 = nullptr;
}

// (re)build the float copy of a level into `out`; true = an entry of A or 1/diag does not fit float
static bool op32_build(cedar_amd_solver *s, const Level &L, float *out, hipStream_t st)
{
	int *flag = s->dinfo + 1, host = 0; // (dinfo[0]: the coarse factorisation's info)
	CEDAR_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(int), st));
	if (s->nd == 2) op2f_build(L.A, L.SOR0 + L.npts, out, L.II, L.JJ, L.nst, flag, st);
	else if (L.nst == 14) ilv32_build(L.A, L.SOR0 + L.npts, out, L.II, L.JJ, L.KK, flag, st);
	else op7f_build(L.A, L.SOR0 + L.npts, out, L.II, L.JJ, L.KK, flag, st);
	CEDAR_HIP_CHECK(hipMemcpyAsync(&host, flag, sizeof(int), hipMemcpyDeviceToHost, st));
	CEDAR_HIP_CHECK(hipStreamSynchronize(st));
	return host != 0;
}

// Smallest row count from which a level takes the copy by default.  Measured (tools/op32_time.py, profiles/op32_time.json;
// DESIGN.md section 12): adding the level with 128 rows shortens the V-cycle on every handle measured, adding the one with
// 64 rows lengthens it (such a level is launch-bound, and the Cedar-layout kernels it otherwise runs are the better fit)
// A batch handle (cedar_amd_solver_use_fp32_operator_many) has the same break-even level at 1, 2, 4 and 8 right-hand sides
// (tools/op32_many_time.py, profiles/op32_many_time.json) and takes the same default
enum { OP32_DEFAULT_MIN_ROWS = 128 };
// The same for the 7-point level under cedar_amd_solver_use_fp32_operator_all(s, 0) (0 here would leave it in FP64 unless
// min_rows > 0 is given).  Measured (tools/op32_7pt_time.py, profiles/op32_7pt_time.json): the
// switched V(1,1) / V(2,1) cycle runs in 0.72 / 0.69 of the FP64 one at 512^3, 0.87 / 0.88 at 256^3 and 0.95 / 0.94 at
// 128^3, each gain many times the spread of the repetitions; nothing smaller was measured, so nothing smaller is taken
enum { OP32_7PT_DEFAULT_MIN_ROWS = 128 };

int cedar_amd_solver_fp32_levels(const cedar_amd_solver *s)
{
	return null_handle(s, "cedar_amd_solver_fp32_levels") ? 0 : fp32_count(s);
}

// the body of cedar_amd_solver_use_fp32_operator (batch false: a handle of cedar_amd_solver_create_many is refused) and
// of cedar_amd_solver_use_fp32_operator_many on a batch handle; seven: the 7-point level takes its copy as well
// (cedar_amd_solver_use_fp32_operator_all)
static int op32_switch(cedar_amd_solver *s, int min_rows, bool batch, const char *who, bool seven = false)
{
	if (null_handle(s, who) || semidef_refused(s, who, "the handle is unchanged")) return -1;
	const char *why = nullptr;
	if (s->nd != 3) why = "2D handles are not supported";
	else if (s->st.ibc != 0) why = "periodic boundary conditions (ibc != 0) are not supported";
	else if (s->st.relaxation != CEDAR_AMD_RELAX_POINT) why = "plane relaxation is not supported";
	else if (s->nb_alloc > 1 && !batch) why = "handles of cedar_amd_solver_create_many are not supported";
	else if (min_rows < 0) why = "min_rows must not be negative";
	auto refuse = [&](const char *reason) {
		char msg[256];
		snprintf(msg, sizeof(msg), "%s: %s; the handle is unchanged", who, reason);
		print_error(msg);
		return -1;
	};
	if (why) return refuse(why);
	// the 7-point level (level 0; rows of any length): an explicit min_rows counts as given, 0 = its own measured default
	const int min_rows7 = !seven ? 0 : min_rows > 0 ? min_rows : (int)OP32_7PT_DEFAULT_MIN_ROWS;
	if (min_rows == 0) {
		const char *e = getenv("CEDAR_AMD_OP32_MIN_ROWS"); // read per call, like CEDAR_AMD_PSUM
		min_rows = e && atoi(e) > 0 ? atoi(e) : (int)OP32_DEFAULT_MIN_ROWS;
	}
	// every smoothed 27-point level (all but the coarsest) with at least min_rows rows, rows within the row kernels' reach;
	// all copies are built and checked before the handle changes
	hipStream_t st = current_stream();
	std::vector<std::pair<int, float *>> fresh;
	auto undo = [&]() {
		for (auto &f : fresh) (void)hipFree(f.second);
	};
	for (int l = 0; l + 1 < (int)s->lv.size(); l++) {
		const Level &L = s->lv[l];
		const bool take7 = s->nd == 3 && L.nst != 14 && !L.A7f && min_rows7 > 0 && L.ny >= min_rows7;
		if (!take7 && (L.A32 || L.nst != 14 || L.ny < min_rows || (L.II - 2 + 1) / 2 > 512)) continue;
		float *c = nullptr;
		const size_t nfl = take7 ? op7f_floats(L.II, L.JJ, L.KK) : ilv32_floats(L.II, L.JJ, L.KK);
		if (hipMalloc((void **)&c, nfl * sizeof(float)) != hipSuccess) {
			(void)hipGetLastError();
			undo();
			return refuse("out of device memory for the single-precision copy");
		}
		fresh.emplace_back(l, c);
		if (op32_build(s, L, c, st)) {
			undo();
			return refuse("an entry of the operator or of 1/diag overflows single precision");
		}
	}
	if (!fresh.empty()) {
		graphs_drop(s);
		for (auto &f : fresh) {
			Level &L = s->lv[f.first];
			if (L.nst != 14) {
				L.A7f = f.second;
				continue;
			}
			L.A32 = f.second;
			(void)hipFree(L.Ailv);
			L.Ailv = nullptr;
		}
	}
	launch_check(who);
	return fp32_count(s);
}

int cedar_amd_solver_use_fp32_operator(cedar_amd_solver *s, int min_rows)
{
	return op32_switch(s, min_rows, false, "cedar_amd_solver_use_fp32_operator");
}

// A batch handle takes the same copies: its batched sweeps and residual (many3d.hip) read them through the same view.  A
// handle that holds one right-hand side -- made so, or a batch request the handle could not serve (periodic, planes) --
// goes through the single call, refusals included.
int cedar_amd_solver_use_fp32_operator_many(cedar_amd_solver *s, int min_rows)
{
	const char *who = "cedar_amd_solver_use_fp32_operator_many";
	if (null_handle(s, who)) return -1;
	if (s->nb_alloc == 1) return cedar_amd_solver_use_fp32_operator(s, min_rows);
	return op32_switch(s, min_rows, true, who);
}

// Either kind of handle, and the 7-point level as well: what the two calls above do, plus the float copy of a 7-point
// level 0 (op7f.hip).  The two calls above keep leaving a 7-point level in FP64.
int cedar_amd_solver_use_fp32_operator_all(cedar_amd_solver *s, int min_rows)
{
	const char *who = "cedar_amd_solver_use_fp32_operator_all";
	if (null_handle(s, who)) return -1;
	return op32_switch(s, min_rows, s->nb_alloc > 1, who, true);
}

// The switch for 2D handles, single or batch (Dirichlet, point relaxation, V- or F-cycle): every smoothed level with at
// least min_rows rows, five-point level 0 and nine-point levels alike, takes a float copy (common.h Op2f, op2f.hip).
// Written after op32_switch; the two share fp32_count, graphs_drop and op32_build.
// min_rows = 0, the default: levels of at least 1024 rows.  Measured (tools/op32_2d_time.py, profiles/op32_2d_time.json;
// DESIGN.md section 16) on the nine-point varcoef9 and the five-point gallery::poisson: with level 0 alone switched the
// V(1,1) / V(2,1) cycle runs in 0.93 / 0.93 and 0.89 / 0.87 of its FP64 time at 4096^2, 0.88 / 0.87 and 0.91 / 0.91 at
// 2048^2, 0.95 / 0.94 and 0.96 / 0.94 at 1024^2, each gain several times the spread of the repetitions; at 512^2 it is
// 1.00 / 1.00 and 0.99 / 0.99, inside the spread, and adding a level of 512 rows to a larger handle's set gains nothing
// (4096^2) or loses (1024^2: 0.951 -> 0.963).  So levels of 512 rows and fewer stay FP64 unless min_rows > 0 asks.
enum { OP32_2D_DEFAULT_MIN_ROWS = 1024 };

int cedar_amd_solver_use_fp32_operator_2d(cedar_amd_solver *s, int min_rows)
{
	const char *who = "cedar_amd_solver_use_fp32_operator_2d";
	if (null_handle(s, who) || semidef_refused(s, who, "the handle is unchanged")) return -1;
	auto refuse = [&](const char *reason) {
		char msg[256];
		snprintf(msg, sizeof(msg), "%s: %s; the handle is unchanged", who, reason);
		print_error(msg);
		return -1;
	};
	if (s->nd != 2) return refuse("3D handles are not supported (use cedar_amd_solver_use_fp32_operator_all)");
	if (s->st.ibc != 0) return refuse("periodic boundary conditions (ibc != 0) are not supported");
	if (s->st.relaxation != CEDAR_AMD_RELAX_POINT) return refuse("line relaxation is not supported");
	if (min_rows < 0) return refuse("min_rows must not be negative");
	if (min_rows == 0) {
		const char *e = getenv("CEDAR_AMD_OP32_MIN_ROWS"); // read per call, like CEDAR_AMD_PSUM
		min_rows = e && atoi(e) > 0 ? atoi(e) : (int)OP32_2D_DEFAULT_MIN_ROWS;
	}
	// all copies are built and checked before the handle changes
	hipStream_t st = current_stream();
	std::vector<std::pair<int, float *>> fresh;
	auto undo = [&]() {
		for (auto &f : fresh) (void)hipFree(f.second);
	};
	for (int l = 0; min_rows > 0 && l + 1 < (int)s->lv.size(); l++) {
		const Level &L = s->lv[l];
		if (L.A2f || L.ny < min_rows) continue;
		float *c = nullptr;
		if (hipMalloc((void **)&c, op2f_floats(L.II, L.JJ, L.nst) * sizeof(float)) != hipSuccess) {
			(void)hipGetLastError();
			undo();
			return refuse("out of device memory for the single-precision copy");
		}
		fresh.emplace_back(l, c);
		if (op32_build(s, L, c, st)) {
			undo();
			return refuse("an entry of the operator or of 1/diag overflows single precision");
		}
	}
	if (!fresh.empty()) {
		graphs_drop(s);
		for (auto &f : fresh) s->lv[f.first].A2f = f.second;
	}
	launch_check(who);
	return fp32_count(s);
}

// ---- the switch for 2D handles with line relaxation (single or batch, Dirichlet, V- or F-cycle; linesf.hip)
// the float copies of one level: what the level's fields of the same names hold
struct Lines32 {
	float *A2f = nullptr, *At2f = nullptr, *Fx32 = nullptr, *Fy32 = nullptr, *PFx32 = nullptr, *PFy32 = nullptr;
	void release()
	{
		(void)hipFree(A2f); (void)hipFree(At2f); (void)hipFree(Fx32); (void)hipFree(Fy32); (void)hipFree(PFx32); (void)hipFree(PFy32);
		*this = Lines32();
	}
};
enum { LINES32_A = 1, LINES32_X = 2, LINES32_Y = 4 };

static bool lines_x_used(const cedar_amd_solver *s) { return s->st.relaxation == CEDAR_AMD_RELAX_LINE_X || s->st.relaxation == CEDAR_AMD_RELAX_LINE_XY; }
static bool lines_y_used(const cedar_amd_solver *s) { return s->st.relaxation == CEDAR_AMD_RELAX_LINE_Y || s->st.relaxation == CEDAR_AMD_RELAX_LINE_XY; }
// the y factors SOR(JJ,II,2): SOR0 of a line-y handle, SOR1 of a line-xy one
static const real_t *lines_y_sor(const cedar_amd_solver *s, const Level &L) { return s->st.relaxation == CEDAR_AMD_RELAX_LINE_Y ? L.SOR0 : L.SOR1; }

// allocate the copies a level needs; false = out of device memory (nothing kept)
static bool lines32_alloc(const cedar_amd_solver *s, const Level &L, Lines32 &c)
{
	auto get = [&](float *&p, size_t nfl) {
		if (hipMalloc((void **)&p, (nfl ? nfl : 1) * sizeof(float)) == hipSuccess) return true;
		(void)hipGetLastError();
		p = nullptr;
		return false;
	};
	bool ok = get(c.A2f, op2f_floats(L.II, L.JJ, L.nst));
	if (ok && lines_y_used(s)) ok = get(c.At2f, op2f_floats(L.JJ, L.II, L.nst));
	if (ok && lines_x_used(s))
		ok = L.PFx ? get(c.PFx32, lines_permuted_doubles(L.nx, L.ny)) : get(c.Fx32, L.npts * 2);
	if (ok && lines_y_used(s))
		ok = L.PFy ? get(c.PFy32, lines_permuted_doubles(L.ny, L.nx)) : get(c.Fy32, L.npts * 2);
	if (!ok) c.release();
	return ok;
}

// (re)build the copies named by `what` (LINES32_*) from the level's FP64 arrays, all values rounded to nearest even; true =
// an entry of A or of a factor does not fit float
static bool lines32_build(cedar_amd_solver *s, const Level &L, const Lines32 &c, int what, hipStream_t st)
{
	int *flag = s->dinfo + 1, host = 0; // (dinfo[0]: the coarse factorisation's info)
	CEDAR_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(int), st));
	if (what & LINES32_A) {
		op2f_build(L.A, nullptr, c.A2f, L.II, L.JJ, L.nst, flag, st);
		if (c.At2f) op2f_build(L.At, nullptr, c.At2f, L.JJ, L.II, L.nst, flag, st); // the transposed grid is JJ fast
	}
	if (what & LINES32_X) {
		if (c.PFx32) linesf_permute(L.SOR0, c.PFx32, L.nx, L.II, L.ny, L.npts, flag, st);
		if (c.Fx32) linesf_image(L.SOR0, c.Fx32, L.II, L.JJ, flag, st);
	}
	if (what & LINES32_Y) {
		if (c.PFy32) linesf_permute(lines_y_sor(s, L), c.PFy32, L.ny, L.JJ, L.nx, L.npts, flag, st);
		if (c.Fy32) linesf_image(lines_y_sor(s, L), c.Fy32, L.II, L.JJ, flag, st);
	}
	CEDAR_HIP_CHECK(hipMemcpyAsync(&host, flag, sizeof(int), hipMemcpyDeviceToHost, st));
	CEDAR_HIP_CHECK(hipStreamSynchronize(st));
	return host != 0;
}

static Lines32 lines32_of(const Level &L) { return Lines32{L.A2f, L.At2f, L.Fx32, L.Fy32, L.PFx32, L.PFy32}; }
static void lines32_put(Level &L, const Lines32 &c)
{
	L.A2f = c.A2f; L.At2f = c.At2f; L.Fx32 = c.Fx32; L.Fy32 = c.Fy32; L.PFx32 = c.PFx32; L.PFy32 = c.PFy32;
}

// min_rows = 0, the default: levels of at least 1024 rows.  Measured (tools/op32_lines_time.py, profiles/op32_lines_time.json;
// DESIGN.md section 17) on the nine-point varcoef9 and the five-point gallery::poisson under line-xy: with level 0 alone
// switched the V(1,1) / V(2,1) cycle runs in 0.86 / 0.85 and 0.93 / 0.90 of its FP64 time at 8192^2, 0.85 / 0.85 and
// 0.91 / 0.89 at 4096^2, 0.91 / 0.91 and 0.96 / 0.95 at 2048^2, 0.93 / 0.92 and 0.94 / 0.96 at 1024^2, each gain many times
// the spread of the repetitions; at 512^2 it is 1.00 / 1.00 and 1.01 / 1.00, and adding a level of 512 rows to a larger
// handle's set gains nothing (2048^2: 0.882 -> 0.883) or loses (1024^2 V(2,1): 0.924 -> 0.942).  So levels of 512 rows and
// fewer stay FP64 unless min_rows > 0 asks.
enum { OP32_LINES_DEFAULT_MIN_ROWS = 1024 };

int cedar_amd_solver_use_fp32_operator_lines(cedar_amd_solver *s, int min_rows)
{
	const char *who = "cedar_amd_solver_use_fp32_operator_lines";
	if (null_handle(s, who) || semidef_refused(s, who, "the handle is unchanged")) return -1;
	auto refuse = [&](const char *reason) {
		char msg[256];
		snprintf(msg, sizeof(msg), "%s: %s; the handle is unchanged", who, reason);
		print_error(msg);
		return -1;
	};
	if (s->nd != 2) return refuse("3D handles are not supported (use cedar_amd_solver_use_fp32_operator_all)");
	if (s->st.relaxation == CEDAR_AMD_RELAX_POINT) return refuse("point relaxation is not supported (use cedar_amd_solver_use_fp32_operator_2d)");
	if (s->st.ibc != 0) return refuse("periodic boundary conditions (ibc != 0) are not supported");
	if (lines_y_used(s) && !s->lv[0].At)
		return refuse("y lines that do not keep transposed arrays (CEDAR_AMD_YLINES_TRANSPOSED=0) are not supported");
	if (min_rows < 0) return refuse("min_rows must not be negative");
	if (min_rows == 0) {
		const char *e = getenv("CEDAR_AMD_OP32_MIN_ROWS"); // read per call, like CEDAR_AMD_PSUM
		min_rows = e && atoi(e) > 0 ? atoi(e) : (int)OP32_LINES_DEFAULT_MIN_ROWS;
	}
	// every smoothed level with at least min_rows rows that the LDS-resident small-level kernels do not serve; all copies
	// are built and checked before the handle changes
	hipStream_t st = current_stream();
	std::vector<std::pair<int, Lines32>> fresh;
	auto undo = [&]() {
		for (auto &f : fresh) f.second.release();
	};
	for (int l = 0; min_rows > 0 && l + 1 < (int)s->lv.size(); l++) {
		const Level &L = s->lv[l];
		if (L.A2f || L.ny < min_rows || lines_small_ok(L.II, L.JJ)) continue;
		Lines32 c;
		if (!lines32_alloc(s, L, c)) {
			undo();
			return refuse("out of device memory for the single-precision copies");
		}
		fresh.emplace_back(l, c);
		if (lines32_build(s, L, c, LINES32_A | LINES32_X | LINES32_Y, st)) {
			undo();
			return refuse("an entry of the operator or of a line factor overflows single precision");
		}
	}
	if (!fresh.empty()) {
		graphs_drop(s);
		for (auto &f : fresh) lines32_put(s->lv[f.first], f.second);
	}
	launch_check(who);
	return fp32_count(s);
}

// ---- single-precision interpolation weights (include/cedar_amd.h cedar_amd_solver_use_fp32_interpolation; transferf.hip;
// DESIGN.md section 18)
static int ci32_count(const cedar_amd_solver *s)
{
	int n = 0;
	for (const Level &L : s->lv) n += L.P32 ? 1 : 0;
	return n;
}

// (re)build the float copy of K.P into `out`; true = a finite weight does not fit float
static bool ci32_rebuild(cedar_amd_solver *s, const Level &K, float *out, hipStream_t st)
{
	int *flag = s->dinfo + 1, host = 0; // (dinfo[0]: the coarse factorisation's info)
	CEDAR_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(int), st));
	ci32_build(K.P, out, K.II, K.JJ, K.KK, s->nd == 3 ? 26 : 8, flag, st);
	CEDAR_HIP_CHECK(hipMemcpyAsync(&host, flag, sizeof(int), hipMemcpyDeviceToHost, st));
	CEDAR_HIP_CHECK(hipStreamSynchronize(st));
	return host != 0;
}

// Smallest row count of the fine level from which a level pair takes the copy by default, per dimension: the defaults of
// the operator switches, kept after the measurement of tools/ci32_time.py (profiles/ci32_time.json).
// The level-0 restriction runs in 0.73 - 0.75 of its FP64 time at 512^3, 0.77 - 0.82 at 256^3 and 0.81 - 0.83 at 128^3,
// interpolation-and-add in 0.77 - 0.91, 0.84 - 0.86 and 0.92 - 0.93; 2D 0.74 - 0.86 and 0.81 - 0.91 from 4096^2 down to
// 1024^2.  The cycle gains 1 - 6 %, which is within what two FP64 handles of one operator differ by (up to 4.6 % at
// 512^3), so the rule is "not slower beyond that spread": it holds at every size measured, and nothing smaller was measured
enum { CI32_DEFAULT_MIN_ROWS_3D = 128, CI32_DEFAULT_MIN_ROWS_2D = 1024 };

int cedar_amd_solver_fp32_interp_levels(const cedar_amd_solver *s)
{
	return null_handle(s, "cedar_amd_solver_fp32_interp_levels") ? 0 : ci32_count(s);
}

int cedar_amd_solver_use_fp32_interpolation(cedar_amd_solver *s, int min_rows)
{
	const char *who = "cedar_amd_solver_use_fp32_interpolation";
	if (null_handle(s, who) || semidef_refused(s, who, "the handle is unchanged")) return -1;
	auto refuse = [&](const char *reason) {
		char msg[256];
		snprintf(msg, sizeof(msg), "%s: %s; the handle is unchanged", who, reason);
		print_error(msg);
		return -1;
	};
	if (s->st.ibc != 0) return refuse("periodic boundary conditions (ibc != 0) are not supported");
	if (s->nd == 3 && s->st.relaxation != CEDAR_AMD_RELAX_POINT) return refuse("plane relaxation is not supported");
	if (min_rows < 0) return refuse("min_rows must not be negative");
	if (min_rows == 0) {
		const char *e = getenv("CEDAR_AMD_CI32_MIN_ROWS"); // read per call, like CEDAR_AMD_OP32_MIN_ROWS
		min_rows = e && atoi(e) > 0 ? atoi(e) : s->nd == 3 ? (int)CI32_DEFAULT_MIN_ROWS_3D : (int)CI32_DEFAULT_MIN_ROWS_2D;
	}
	// every pair (fine L, coarse K) whose fine level has at least min_rows rows and runs the transfer kernels; all copies
	// are built and checked before the handle changes
	hipStream_t st = current_stream();
	std::vector<std::pair<int, float *>> fresh;
	auto undo = [&]() {
		for (auto &f : fresh) (void)hipFree(f.second);
	};
	for (int l = 0; l + 1 < (int)s->lv.size(); l++) {
		const Level &L = s->lv[l], &K = s->lv[l + 1];
		if (K.P32 || !K.P || L.ny < min_rows || visit_fused(s, L)) continue;
		float *c = nullptr;
		if (hipMalloc((void **)&c, ci32_floats(K.II, K.JJ, K.KK, s->nd == 3 ? 26 : 8) * sizeof(float)) != hipSuccess) {
			(void)hipGetLastError();
			undo();
			return refuse("out of device memory for the single-precision copy");
		}
		fresh.emplace_back(l + 1, c);
		if (ci32_rebuild(s, K, c, st)) {
			undo();
			return refuse("an interpolation weight overflows single precision");
		}
	}
	if (!fresh.empty()) {
		graphs_drop(s);
		for (auto &f : fresh) s->lv[f.first].P32 = f.second;
	}
	launch_check(who);
	return ci32_count(s);
}

// levels[lvl].A / .P / .SOR / ABD are public members of the reference's solver (include/cedar/level.h:14-41,
// include/cedar/2d/solver.h:56): a caller may replace a set-up product.  Solver-internal copies that derive from the
// array (row-interleaved solve copy, transposed y-line planes, scan-ordered line factors) are rebuilt.
size_t cedar_amd_solver_set(cedar_amd_solver *s, int lvl, const char *what, const real_t *in)
{
	if (null_handle(s, "cedar_amd_solver_set") || lvl < 0 || lvl >= (int)s->lv.size() || !in) return 0;
	Level &L = s->lv[lvl];
	hipStream_t st = current_stream();
	real_t *dst = nullptr;
	size_t n = 0;
	if (!strcmp(what, "A")) { dst = L.A; n = L.npts * L.nst; }
	else if (!strcmp(what, "P")) { dst = L.P; n = L.P ? L.npts * (s->nd == 3 ? 26 : 8) : 0; }
	else if (!strcmp(what, "SOR0")) { dst = L.SOR0; n = L.npts * 2; }
	else if (!strcmp(what, "SOR1")) { dst = L.SOR1; n = L.SOR1 ? L.npts * 2 : 0; }
	else if (!strcmp(what, "ABD")) { dst = s->ABD; n = (size_t)s->nabd1 * s->nabd2; }
	if (!dst || !n) return 0;
	CEDAR_HIP_CHECK(hipDeviceSynchronize()); // no cycle in flight while a product changes
	if (is_device_ptr(in)) cedar_amd_memcpy_d2d(dst, in, n * sizeof(real_t));
	else cedar_amd_memcpy_h2d(dst, in, n * sizeof(real_t));
	if (L.Ailv && (!strcmp(what, "A") || !strcmp(what, "SOR0")))
		ilv_build(L.A, L.SOR0 + L.npts, L.Ailv, L.II, L.JJ, L.KK, st);
	const bool lines32 = s->nd == 2 && L.A2f && s->st.relaxation != CEDAR_AMD_RELAX_POINT; // rebuilt below, after At
	float *&c32 = s->nd == 2 ? L.A2f : L.nst == 14 ? L.A32 : L.A7f; // the level's float copy, of any kind
	if (!lines32 && c32 && (!strcmp(what, "A") || !strcmp(what, "SOR0")) && op32_build(s, L, c32, st)) {
		// the new entries do not fit float: the level goes back to the FP64 planes (the captured cycle names the copy)
		char msg[] = "cedar_amd_solver_set: an entry of the new array overflows single precision; the level reads the FP64 "
		             "operator again";
		print_error(msg);
		graphs_drop(s);
		(void)hipFree(c32);
		c32 = nullptr;
	}
	if (L.P32 && !strcmp(what, "P") && ci32_rebuild(s, L, L.P32, st)) {
		char msg[] = "cedar_amd_solver_set: a weight of the new array overflows single precision; the level's transfers read the "
		             "FP64 weights again";
		print_error(msg);
		graphs_drop(s);
		(void)hipFree(L.P32);
		L.P32 = nullptr;
	}
	if (L.At && !strcmp(what, "A")) setup_lines_yt(L.A, L.At, L.II, L.JJ, L.nst, st);
	if (L.PFx && !strcmp(what, "SOR0")) lines_permute(L.SOR0, L.PFx, L.nx, L.II, L.ny, L.npts, st);
	if (L.PFy && !strcmp(what, s->st.relaxation == CEDAR_AMD_RELAX_LINE_Y ? "SOR0" : "SOR1"))
		lines_permute(s->st.relaxation == CEDAR_AMD_RELAX_LINE_Y ? L.SOR0 : L.SOR1, L.PFy, L.ny, L.JJ, L.nx, L.npts, st);
	if (lines32) {
		// a line level's float copies: "A" feeds both operator copies, "SOR0" / "SOR1" the factor copies of their direction
		const bool yfac = lines_y_used(s) && !strcmp(what, s->st.relaxation == CEDAR_AMD_RELAX_LINE_Y ? "SOR0" : "SOR1");
		const int which = (!strcmp(what, "A") ? LINES32_A : 0) | (lines_x_used(s) && !strcmp(what, "SOR0") ? LINES32_X : 0)
		                  | (yfac ? LINES32_Y : 0);
		if (which && lines32_build(s, L, lines32_of(L), which, st)) {
			char msg[] = "cedar_amd_solver_set: an entry of the new array overflows single precision; the level reads the FP64 "
			             "operator and factors again";
			print_error(msg);
			graphs_drop(s);
			Lines32 c = lines32_of(L);
			c.release();
			lines32_put(L, c);
		}
	}
	CEDAR_HIP_CHECK(hipStreamSynchronize(st));
	launch_check("cedar_amd_solver_set");
	return n;
}

void cedar_amd_solver_vcycle(cedar_amd_solver *s, real_t *x, const real_t *b)
{
	if (null_handle(s, "cedar_amd_solver_vcycle")) return;
	const Level &L = s->lv[0];
	Staged sx(x, L.npts, true, true), sb(b, L.npts, true, false);
	if (sx.staged() || sb.staged()) {
		// staging buffers change from call to call: launch eagerly
		cycle_launch(s, sx.get(), sb.get(), current_stream());
	} else
		cycle_dev(s, sx.get(), sb.get());
	launch_check("cedar_amd_solver_vcycle");
}

int cedar_amd_solver_solve(cedar_amd_solver *s, const real_t *b, real_t *x, real_t *rel)
{
	if (null_handle(s, "cedar_amd_solver_solve")) return 0;
	Level &L = s->lv[0];
	Staged sx(x, L.npts, true, true), sb(b, L.npts, true, false);
	hipStream_t st = current_stream();
	// A handle whose cycle reads a single-precision operator (cedar_amd_solver_use_fp32_operator) iterates in
	// defect-correction form on the Krylov storage: r = b - A x with the FP64 operator (the residual the norm needs
	// anyway), z = cycle(0, r), x += z -- the fixed point is the solution of A, not of the rounded operator.  An F-cycle
	// starts every cycle from x = 0 (fmg_cycle), so there is no iterate to correct: it keeps the plain form.
	const bool defect = s->st.cycle == 0 && s->lv.size() > 1 && fp32_count(s) > 0;
	if (defect) pcg_alloc(s);
	real_t *res = defect ? s->kr : L.res;
	residual_true(s, L, sx.get(), sb.get(), res, st);
	const double res0 = l2_dev(s, L, res);
	rel[0] = res0;
	int it = 0;
	for (it = 0; it < s->st.max_iter; it++) {
		if (defect) {
			pcg_precondition(s, 1, st);
			vec_add(sx.get(), s->kz, L.npts, st);
		} else
			cycle_dev(s, sx.get(), sb.get());
		residual_true(s, L, sx.get(), sb.get(), res, st);
		const double r = l2_dev(s, L, res) / res0;
		rel[it + 1] = r;
		if (r < s->st.tol) { it++; break; }
	}
	launch_check("cedar_amd_solver_solve");
	return it;
}

// ---- several right-hand sides at once on the one resident hierarchy (include/cedar_amd.h): the operator, 1/diag and the
// interpolation weights are the same for every right-hand side, so the kernels fetch them once per workgroup task
cedar_amd_solver *cedar_amd_solver_create_many(int nd, len_t nx, len_t ny, len_t nz, int nstencil, const real_t *so,
                                               int own_device_so, const cedar_amd_settings *settings, int max_rhs)
{
	if (max_rhs < 1 || max_rhs > CEDAR_AMD_MAX_RHS) {
		char msg[] = "cedar_amd_solver_create_many: max_rhs must be 1 .. 32; no solver created";
		print_error(msg);
		return nullptr;
	}
	return solver_create(nd, nx, ny, nz, nstencil, so, own_device_so, settings, max_rhs);
}

// cedar_amd_solver_create_many for a periodic 3D handle (include/cedar_amd.h).  What solver_create would quietly turn into
// something else -- an F-cycle or plane relaxation with a batch, 2D periodic -- is refused here instead
cedar_amd_solver *cedar_amd_solver_create_many_periodic(int nd, len_t nx, len_t ny, len_t nz, int nstencil, const real_t *so,
                                                        int own_device_so, const cedar_amd_settings *settings, int max_rhs)
{
	cedar_amd_settings st;
	if (settings) st = *settings;
	else cedar_amd_default_settings(&st);
	if (st.ibc == 0) return cedar_amd_solver_create_many(nd, nx, ny, nz, nstencil, so, own_device_so, settings, max_rhs);
	const char *why = nullptr;
	if (max_rhs < 1 || max_rhs > CEDAR_AMD_MAX_RHS) why = "max_rhs must be 1 .. 32";
	else if (nd != 3) why = "periodic batches are served in 3D only";
	else if (st.cycle != 0) why = "only the V-cycle is supported";
	else if (st.relaxation != CEDAR_AMD_RELAX_POINT) why = "only point relaxation is supported";
	if (why) {
		char msg[256];
		snprintf(msg, sizeof(msg), "cedar_amd_solver_create_many_periodic: %s; no solver created", why);
		print_error(msg);
		return nullptr;
	}
	cedar_amd_solver *s = solver_create(nd, nx, ny, nz, nstencil, so, own_device_so, settings, max_rhs, true);
	if (!s) { // what cedar_amd_solver_create refuses for a periodic handle, reported above under its name
		char msg[] = "cedar_amd_solver_create_many_periodic: refused as cedar_amd_solver_create refuses it; no solver created";
		print_error(msg);
	}
	return s;
}

// cedar_amd_solver_create_many for a periodic 2D handle (include/cedar_amd.h): point and line relaxation, V-cycle
cedar_amd_solver *cedar_amd_solver_create_many_periodic2(len_t nx, len_t ny, int nstencil, const real_t *so, int own_device_so,
                                                         const cedar_amd_settings *settings, int max_rhs)
{
	cedar_amd_settings st;
	if (settings) st = *settings;
	else cedar_amd_default_settings(&st);
	if (st.ibc == 0) return cedar_amd_solver_create_many(2, nx, ny, 1, nstencil, so, own_device_so, settings, max_rhs);
	const char *why = nullptr;
	if (max_rhs < 1 || max_rhs > CEDAR_AMD_MAX_RHS) why = "max_rhs must be 1 .. 32";
	else if (st.ibc < 1 || st.ibc > 3) why = "the 2D boundary codes are 0 and 1 .. 3";
	else if (st.cycle != 0) why = "only the V-cycle is supported";
	if (why) {
		char msg[256];
		snprintf(msg, sizeof(msg), "cedar_amd_solver_create_many_periodic2: %s; no solver created", why);
		print_error(msg);
		return nullptr;
	}
	cedar_amd_solver *s = solver_create(2, nx, ny, 1, nstencil, so, own_device_so, settings, max_rhs, true);
	if (!s) { // what cedar_amd_solver_create refuses for a periodic handle, reported above under its name
		char msg[] = "cedar_amd_solver_create_many_periodic2: refused as cedar_amd_solver_create refuses it; no solver created";
		print_error(msg);
	}
	return s;
}

// A semidefinite operator whose null space is the constants (pure Neumann, fully periodic; include/cedar_amd.h).  The
// boundary code keeps its meaning -- codes below zero stay refused everywhere -- and the request is this call.  What the
// creation call for (nd, ibc, max_rhs) refuses is refused here under its name first; solver_create then checks the null
// space, doubles the last diagonal entry of the coarsest matrix and marks the handle
cedar_amd_solver *cedar_amd_solver_create_semidefinite(int nd, len_t nx, len_t ny, len_t nz, int nstencil, const real_t *so,
                                                       int own_device_so, const cedar_amd_settings *settings, int max_rhs)
{
	cedar_amd_settings st;
	if (settings) st = *settings;
	else cedar_amd_default_settings(&st);
	auto refuse = [](const char *why) {
		char msg[256];
		snprintf(msg, sizeof(msg), "cedar_amd_solver_create_semidefinite: %s; no solver created", why);
		print_error(msg);
		return (cedar_amd_solver *)nullptr;
	};
	if (max_rhs < 1 || max_rhs > CEDAR_AMD_MAX_RHS) return refuse("max_rhs must be 1 .. 32");
	if (nd != 2 && nd != 3) return refuse("nd must be 2 or 3");
	if (st.ibc < 0) return refuse("boundary codes below zero are not served (ibc keeps its meaning: 0, 2D 1..3, 3D 1..3 and 5..8)");
	if (st.relaxation >= CEDAR_AMD_RELAX_PLANE_XY) return refuse("plane relaxation is not served on a semidefinite operator");
	// a batch: what cedar_amd_solver_create_many_periodic / _periodic2 refuse beyond solver_create (for ibc == 0 too: a
	// batch handle that quietly held one right-hand side would not be what was asked for).  These two rules restate
	// theirs, because this call must reach solver_create itself to pass the semidefinite flag: keep them in step
	if (max_rhs > 1 && st.cycle != 0) return refuse("max_rhs > 1: only the V-cycle is supported");
	if (max_rhs > 1 && nd == 3 && st.relaxation != CEDAR_AMD_RELAX_POINT) return refuse("max_rhs > 1: only point relaxation is supported");
	cedar_amd_solver *s = solver_create(nd, nx, ny, nz, nstencil, so, own_device_so, settings, max_rhs, max_rhs > 1 && st.ibc != 0, true);
	if (!s) return refuse("refused as reported above");
	return s;
}

int cedar_amd_solver_max_rhs(const cedar_amd_solver *s) { return null_handle(s, "cedar_amd_solver_max_rhs") ? 0 : s->nb_alloc; }

// what the batched entry points cannot do: reported, nothing written
static bool many_refused(const cedar_amd_solver *s, int nrhs, const char *who)
{
	const char *why = nullptr;
	if (nrhs < 1) why = "nrhs must be at least 1";
	else if (s->st.ibc != 0 && !s->per_batch) why = "periodic boundary conditions (ibc != 0) are not supported";
	else if (s->st.cycle != 0) why = "only the V-cycle is supported";
	else if (s->nd == 3 && s->st.relaxation != CEDAR_AMD_RELAX_POINT) why = "3D plane relaxation is not supported";
	else if (nrhs > s->nb_alloc) why = "nrhs exceeds the handle's max_rhs (cedar_amd_solver_create_many)";
	if (!why) return false;
	char msg[256];
	snprintf(msg, sizeof(msg), "%s: %s; nothing done", who, why);
	print_error(msg);
	return true;
}

// the batch count holds for the duration of one _many call: every other entry point works on item 0
struct BatchScope {
	cedar_amd_solver *s;
	BatchScope(cedar_amd_solver *s_, int nrhs) : s(s_) { s->nb = nrhs; }
	~BatchScope() { s->nb = 1; }
};

// ||v_m||_2 of the first s->nb items of a level-0 vector: one host read of nb doubles
static void l2_many(cedar_amd_solver *s, const Level &L, const real_t *v, double *out)
{
	hipStream_t st = current_stream();
	sumsq_interior_many(v, L.II, L.JJ, L.KK, s->red, s->red + 4096, st, Batch{s->nb, L.npts});
	CEDAR_HIP_CHECK(hipMemcpyAsync(out, s->red + 4096, (size_t)s->nb * sizeof(double), hipMemcpyDeviceToHost, st));
	CEDAR_HIP_CHECK(hipStreamSynchronize(st));
	for (int m = 0; m < s->nb; m++) out[m] = std::sqrt(out[m]);
}

int cedar_amd_solver_vcycle_many(cedar_amd_solver *s, int nrhs, real_t *x, const real_t *b)
{
	if (null_handle(s, "cedar_amd_solver_vcycle_many") || many_refused(s, nrhs, "cedar_amd_solver_vcycle_many")) return -1;
	const Level &L = s->lv[0];
	BatchScope scope(s, nrhs);
	Staged sx(x, L.npts * nrhs, true, true), sb(b, L.npts * nrhs, true, false);
	if (sx.staged() || sb.staged()) cycle_launch(s, sx.get(), sb.get(), current_stream()); // staging buffers change from call to call
	else cycle_dev(s, sx.get(), sb.get());
	launch_check("cedar_amd_solver_vcycle_many");
	return 0;
}

int cedar_amd_solver_solve_many(cedar_amd_solver *s, int nrhs, const real_t *b, real_t *x, real_t *rel, int *iters)
{
	if (null_handle(s, "cedar_amd_solver_solve_many") || many_refused(s, nrhs, "cedar_amd_solver_solve_many")) return -1;
	Level &L = s->lv[0];
	BatchScope scope(s, nrhs);
	Staged sx(x, L.npts * nrhs, true, true), sb(b, L.npts * nrhs, true, false);
	hipStream_t st = current_stream();
	const int maxit = s->st.max_iter;
	const size_t ld = (size_t)(maxit > 0 ? maxit : 0) + 1; // row length of rel
	double res0[CEDAR_AMD_MAX_RHS], nrm[CEDAR_AMD_MAX_RHS];
	bool met[CEDAR_AMD_MAX_RHS];
	// a handle whose cycle reads a single-precision operator: defect correction on the Krylov storage, as
	// cedar_amd_solver_solve does -- r = b - A x with the FP64 operator on every item, z = cycle(0, r) batched, x += z
	const bool defect = s->lv.size() > 1 && fp32_count(s) > 0;
	if (defect) pcg_alloc(s, nrhs == 1 ? 1 : s->nb_alloc);
	real_t *res = defect ? s->kr : L.res;
	residual_true(s, L, sx.get(), sb.get(), res, st);
	l2_many(s, L, res, res0);
	int open = 0;
	for (int m = 0; m < nrhs; m++) {
		rel[m * ld] = res0[m];
		met[m] = res0[m] == 0.0; // a zero residual: converged from the start (a single solve would record 0/0)
		if (iters) iters[m] = met[m] ? 0 : maxit;
		open += met[m] ? 0 : 1;
	}
	int it = 0;
	while (open > 0 && it < maxit) {
		if (defect) {
			pcg_precondition(s, 1, st);
			vec_add(sx.get(), s->kz, L.npts * (size_t)nrhs, st); // items back to back in both
		} else
			cycle_dev(s, sx.get(), sb.get());
		residual_true(s, L, sx.get(), sb.get(), res, st);
		l2_many(s, L, res, nrm);
		it++;
		for (int m = 0; m < nrhs; m++) {
			const double r = res0[m] == 0.0 ? 0.0 : nrm[m] / res0[m];
			rel[m * ld + it] = r;
			if (!met[m] && r < s->st.tol) {
				met[m] = true;
				if (iters) iters[m] = it;
				open--;
			}
		}
	}
	launch_check("cedar_amd_solver_solve_many");
	return it;
}

float cedar_amd_solver_time_vcycles_many(cedar_amd_solver *s, int nrhs, real_t *x_dev, const real_t *b_dev, int n)
{
	if (null_handle(s, "cedar_amd_solver_time_vcycles_many") || many_refused(s, nrhs, "cedar_amd_solver_time_vcycles_many")) return -1.f;
	BatchScope scope(s, nrhs);
	return cedar_amd_solver_time_vcycles(s, x_dev, b_dev, n);
}

// ---- preconditioned conjugate gradient (BoxMG's PCG: src/{2d,3d}/ftn/BMG_PCG_parameters_f90.h) on the resident
// hierarchy.  The multigrid preconditioner z = M^-1 r is nmg_cycles cycles from z = 0 on the solver's own (z, r) pair,
// so its captured graph is recorded once.  The vector work is krylov.hip; per iteration the host reads the device
// scalars once (PCG_NSC doubles) for the stop test.
void cedar_amd_default_pcg_settings(cedar_amd_pcg_settings *p)
{
	p->max_iter = 50;
	p->tol = 1e-8;
	p->stop_test = CEDAR_AMD_PCG_STOP_REL_RES_L2;
	p->precon = CEDAR_AMD_PCG_PRECON_BMG;
	p->nmg_cycles = 1;
}

// settings the solver cannot honour: reported, and the caller's vectors are left alone
static bool pcg_refused(const cedar_amd_solver *s, const cedar_amd_pcg_settings &p, const char *who)
{
	const char *why = nullptr;
	if (s->st.ibc != 0) why = "periodic boundary conditions (ibc != 0) are not supported";
	else if (p.stop_test < CEDAR_AMD_PCG_STOP_ABS_RES_L2 || p.stop_test > CEDAR_AMD_PCG_STOP_REL_RES_M2) why = "stop_test must be 0..3";
	else if (p.precon < CEDAR_AMD_PCG_PRECON_NONE || p.precon > CEDAR_AMD_PCG_PRECON_BMG) why = "precon must be 1..3";
	else if (p.max_iter < 0) why = "max_iter must not be negative";
	else if (p.precon == CEDAR_AMD_PCG_PRECON_BMG) {
		if (s->st.cycle != 0) why = "the multigrid preconditioner must be a V-cycle (an F-cycle is not symmetric)";
		else if (s->st.nrelax_pre != s->st.nrelax_post) why = "the multigrid preconditioner needs nrelax_pre == nrelax_post (symmetric V-cycle)";
		else if (s->st.relaxation >= CEDAR_AMD_RELAX_PLANE_XY && s->st.plane_nrelax_pre != s->st.plane_nrelax_post)
			why = "plane relaxation in the preconditioner needs plane_nrelax_pre == plane_nrelax_post (symmetric plane solves)";
		else if (p.nmg_cycles < 1) why = "nmg_cycles must be at least 1";
	}
	if (!why) return false;
	char msg[256];
	snprintf(msg, sizeof(msg), "%s: %s; nothing done", who, why);
	print_error(msg);
	return true;
}

// the Krylov storage for `items` right-hand sides (item-major; the single-vector calls work on item 0's set).  Growing it
// frees the smaller set first: a captured cycle on the old (z, r) pair is re-recorded by graph_prepare when they moved.
static void pcg_alloc(cedar_amd_solver *s, int items)
{
	if (s->kr && s->kitems >= items) return;
	if (s->kr) {
		CEDAR_HIP_CHECK(hipStreamSynchronize(current_stream()));
		(void)hipFree(s->kr); (void)hipFree(s->kz); (void)hipFree(s->kw); (void)hipFree(s->kp[0]); (void)hipFree(s->kp[1]);
		(void)hipFree(s->kslab); (void)hipFree(s->ksc);
	}
	const Level &L = s->lv[0];
	const size_t n = L.npts * (size_t)items;
	// zero-filled: ghost entries stay zero (the kernels write interiors only)
	s->kr = dalloc(n); s->kz = dalloc(n); s->kw = dalloc(n);
	s->kp[0] = dalloc(n); s->kp[1] = dalloc(n);
	s->kslab = dalloc_raw(pcg_slab_doubles(s->nd, L.nst, L.II, L.JJ, L.KK) * (size_t)items);
	s->ksc = dalloc((size_t)PCG_NSC * items);
	s->kitems = items;
}

// z = M^-1 r on the solver's own vectors: z = 0, then nmg V-cycles
static void pcg_precondition(cedar_amd_solver *s, int nmg, hipStream_t st)
{
	clear(s->kz, s->lv[0].npts * (size_t)s->nb, st);
	for (int c = 0; c < nmg; c++) cycle_on(s, s->kz, s->kr, st);
}

// The iteration of cedar_amd_solver_pcg / _pcg_many on nrhs right-hand sides in lockstep.  nrhs == 1: the single-vector
// passes of krylov.hip and the single-vector cycle (partial-sum sweeps included) on item 0's storage; else every pass
// batched (krylov.hip *_many) and the preconditioner the batched cycle on the handle's own nrhs pairs (z, r).  One host
// read of nrhs scalar blocks per iteration.  An item that met its stop test, broke down or had nothing to do leaves the
// `active` mask: its x, r, scalars stay as they are from then on (it still rides through the batched cycle, which has no
// mask; its z is unused).  hist: rows of max_iter + 1 entries, those after an item's last iteration unwritten; iters
// (may be null): the items' counts.  Returns the largest.
// flexible (cedar_amd_solver_fcg / _fcg_many, multigrid preconditioner only): the dots after the preconditioner also form
// w.z -- s->kw is still w_k = A p_k there, the next direction pass has not run -- and beta is the Polak-Ribiere one
// (krylov.hip pcg_rho_flex), which needs no symmetry of M.  Nothing else of the loop changes.
// project (cedar_amd_solver_fcg_semidefinite / _many): A x = P b with mean(x) = 0, P v = v - mean_interior(v) 1.  r0 := P r0
// once it is formed (b is not written) and x := P x of every item before the final wrap; in between x's constant part
// drifts and the recurrence does not see it.  The multigrid preconditioner is applied as P M P: r := P r before the cycle
// and z := P z after it, on the active items.  In exact arithmetic that changes nothing the recurrence sees (w = A p has
// no constant part), in floating point it is what makes the history reproducible: the rounding of w leaves a constant
// in r that never shrinks, the cycle answers a constant with a large smooth correction, and the constant the cycle
// leaves in z is cancellation noise in the next w.  Measured on the statement: a relative 1e-16
// change of z moves the history entries above 1e-10 by 4e-7 to 4e-6 without the two projections and by 1e-13 with them.
static int pcg_run(cedar_amd_solver *s, int nrhs, const real_t *b, real_t *x, const cedar_amd_pcg_settings &p, real_t *hist,
                   int *iters, const char *who, bool flexible = false, bool project = false)
{
	pcg_alloc(s, nrhs == 1 ? 1 : s->nb_alloc);
	Level &L = s->lv[0];
	hipStream_t st = current_stream();
	BatchScope scope(s, nrhs);
	Staged sx(x, L.npts * nrhs, true, true), sb(b, L.npts * nrhs, true, false);
	real_t *X = sx.get();
	const Batch bt{nrhs, L.npts};
	const PcgRule rule = pcg_rule(p);
	const int zm = rule.zm;
	real_t *Z = zm == 0 ? s->kr : s->kz;
	const Op3 view = exact_view27(L);
	const Op3 *op27 = L.Ailv ? &view : nullptr; // (nullptr: the passes read the planes L.A themselves)
	const size_t ld = (size_t)p.max_iter + 1; // row length of hist
	double sc[CEDAR_AMD_MAX_RHS * PCG_NSC], r0[CEDAR_AMD_MAX_RHS], m0[CEDAR_AMD_MAX_RHS];
	int itm[CEDAR_AMD_MAX_RHS];
	unsigned active = nrhs >= 32 ? ~0u : (1u << nrhs) - 1u;
	// a periodic handle (cedar_amd_solver_fcg_periodic, one right-hand side; _fcg_periodic_many, a batch): every item's x gets
	// the periodic image in its ghost layers before the residual reads them and again on return; the direction pass wraps
	// its own reads (krylov.hip)
	const int ibc = s->st.ibc;
	auto wrap_x = [&]() {
		if (ibc && s->nd == 2) wrap2(X, L.II, L.JJ, nrhs, per_dirs(2, ibc).y, per_dirs(2, ibc).x, st);
		else if (ibc) wrap3(X, L.II, L.JJ, L.KK, nrhs, ibc, st);
	};
	// the two passes on the active items; update: pn = nullptr leaves x and r where they are (dot products only)
	auto direction = [&](const real_t *pold, real_t *pn, bool first) {
		if (ibc && nrhs > 1)
			pcg_direction_periodic_many(L.A, Z, pold, pn, s->kw, s->nd, L.nst, L.II, L.JJ, L.KK, ibc, first, s->kslab, s->ksc, st, bt, active);
		else if (ibc)
			pcg_direction_periodic(L.A, Z, pold, pn, s->kw, s->nd, L.nst, L.II, L.JJ, L.KK, ibc, first, s->kslab, s->ksc, st);
		else if (nrhs == 1)
			pcg_direction(L.A, op27, Z, pold, pn, s->kw, s->nd, L.nst, L.II, L.JJ, L.KK, first, s->kslab, s->ksc, st);
		else
			pcg_direction_many(L.A, op27, Z, pold, pn, s->kw, s->nd, L.nst, L.II, L.JJ, L.KK, first, s->kslab, s->ksc, st, bt, active);
	};
	auto update = [&](int zmode, const real_t *pn, bool first) {
		const real_t *w = pn ? s->kw : nullptr;
		if (nrhs == 1) pcg_update(zmode, pn != nullptr, X, s->kr, pn, w, Z, L.A, L.II, L.JJ, L.KK, first, s->kslab, s->ksc, st);
		else pcg_update_many(zmode, pn != nullptr, X, s->kr, pn, w, Z, L.A, L.II, L.JJ, L.KK, first, s->kslab, s->ksc, st, bt, active);
	};
	// z = M^-1 r of the new residuals, then their dots (flexible: w.z with them)
	auto precondition = [&](bool r_projected) {
		if (project && !r_projected) project_mean_many(s->kr, L.II, L.JJ, L.KK, s->pm, st, bt, active);
		pcg_precondition(s, p.nmg_cycles, st);
		if (project) project_mean_many(s->kz, L.II, L.JJ, L.KK, s->pm, st, bt, active);
	};
	auto precondition_dots = [&]() {
		precondition(false);
		if (!flexible) update(2, nullptr, false);
		else if (nrhs == 1) pcg_dots_wz(s->kr, Z, s->kw, L.II, L.JJ, L.KK, false, s->kslab, s->ksc, st);
		else pcg_dots_wz_many(s->kr, Z, s->kw, L.II, L.JJ, L.KK, false, s->kslab, s->ksc, st, bt, active);
	};
	auto scalars = [&]() {
		CEDAR_HIP_CHECK(hipMemcpyAsync(sc, s->ksc, (size_t)nrhs * PCG_NSC * sizeof(double), hipMemcpyDeviceToHost, st));
		CEDAR_HIP_CHECK(hipStreamSynchronize(st));
	};

	// r0 = b - A x0, z0 = M^-1 r0, rho0 = r0.z0 of every item (the update pass without the update)
	zero_fill(s->ksc, (size_t)PCG_NSC * nrhs, st);
	wrap_x();
	residual_true(s, L, X, sb.get(), s->kr, st);
	if (project) project_mean_many(s->kr, L.II, L.JJ, L.KK, s->pm, st, bt, active);
	if (zm == 2) precondition(project); // (r0 has just been projected)
	update(zm, nullptr, true);
	scalars();
	for (int m = 0; m < nrhs; m++) {
		const double *q = sc + (size_t)m * PCG_NSC;
		r0[m] = std::sqrt(q[PCG_RR]);
		m0[m] = std::sqrt(q[PCG_RZ] > 0 ? q[PCG_RZ] : 0.0);
		itm[m] = 0;
		if (hist) hist[m * ld] = r0[m];
		// b = A x0 exactly, r0.z0 <= 0 (M not positive definite on r0), or already converged: nothing to do for this item
		if (r0[m] == 0.0 || !(q[PCG_RZ] > 0) || rule.stop(q[PCG_RR], q[PCG_RZ], r0[m], m0[m])) active &= ~(1u << m);
	}
	for (int k = 0; k < p.max_iter && active; k++) {
		real_t *pold = s->kp[(k + 1) & 1], *pn = s->kp[k & 1];
		direction(pold, pn, k == 0);
		update(zm == 2 ? 3 : zm, pn, false);
		if (zm == 2 && rule.mnorm) precondition_dots(); // the M-norm of the new residuals needs their preconditioned form first
		scalars();
		for (int m = 0; m < nrhs; m++) {
			if (!((active >> m) & 1u)) continue;
			const double *q = sc + (size_t)m * PCG_NSC;
			if (q[PCG_FLAG] != 0) { active &= ~(1u << m); continue; } // breakdown (p.Ap <= 0 or rho = 0): alpha was 0, x is as it was
			itm[m] = k + 1;
			if (hist) hist[m * ld + itm[m]] = std::sqrt(q[PCG_RR]) / r0[m];
			if (rule.stop(q[PCG_RR], q[PCG_RZ], r0[m], m0[m])) active &= ~(1u << m);
		}
		if (zm == 2 && !rule.mnorm && k + 1 < p.max_iter && active) precondition_dots(); // z of the new residuals, for the next direction
	}
	if (project) project_mean_many(X, L.II, L.JJ, L.KK, s->pm, st, bt, nrhs >= 32 ? ~0u : (1u << nrhs) - 1u);
	wrap_x();
	launch_check(who);
	int most = 0;
	for (int m = 0; m < nrhs; m++) {
		if (iters) iters[m] = itm[m];
		most = std::max(most, itm[m]);
	}
	return most;
}

int cedar_amd_solver_pcg(cedar_amd_solver *s, const real_t *b, real_t *x, const cedar_amd_pcg_settings *settings, real_t *hist)
{
	const char *who = "cedar_amd_solver_pcg";
	if (null_handle(s, who) || semidef_refused(s, who)) return -1;
	const cedar_amd_pcg_settings p = pcg_settings_or_default(settings);
	if (pcg_refused(s, p, who)) return -1;
	return pcg_run(s, 1, b, x, p, hist, nullptr, who);
}

// served where the other batched entry points are (many_refused); one right-hand side takes the single-vector path
int cedar_amd_solver_pcg_many(cedar_amd_solver *s, int nrhs, const real_t *b, real_t *x, const cedar_amd_pcg_settings *settings,
                              real_t *hist, int *iters)
{
	const char *who = "cedar_amd_solver_pcg_many";
	if (null_handle(s, who) || semidef_refused(s, who) || many_refused(s, nrhs, who)) return -1;
	const cedar_amd_pcg_settings p = pcg_settings_or_default(settings);
	if (pcg_refused(s, p, who)) return -1;
	return pcg_run(s, nrhs, b, x, p, hist, iters, who);
}

// Flexible CG: what cedar_amd_solver_pcg refuses of the multigrid preconditioner for its lack of symmetry is served here
static bool fcg_refused(const cedar_amd_solver *s, const cedar_amd_pcg_settings &p, const char *who, bool periodic_ok = false)
{
	const char *why = nullptr;
	if (s->st.ibc != 0 && !periodic_ok) why = "periodic boundary conditions (ibc != 0) are not supported";
	else if (p.stop_test < CEDAR_AMD_PCG_STOP_ABS_RES_L2 || p.stop_test > CEDAR_AMD_PCG_STOP_REL_RES_M2) why = "stop_test must be 0..3";
	else if (p.precon < CEDAR_AMD_PCG_PRECON_NONE || p.precon > CEDAR_AMD_PCG_PRECON_BMG) why = "precon must be 1..3";
	else if (p.max_iter < 0) why = "max_iter must not be negative";
	else if (p.precon == CEDAR_AMD_PCG_PRECON_BMG) {
		if (p.nmg_cycles < 1) why = "nmg_cycles must be at least 1";
		else if (s->st.nrelax_pre + s->st.nrelax_post < 1) why = "the multigrid preconditioner needs at least one relaxation sweep";
	}
	if (!why) return false;
	char msg[256];
	snprintf(msg, sizeof(msg), "%s: %s; nothing done", who, why);
	print_error(msg);
	return true;
}

// precon none / diag: M is exactly symmetric, the recurrence is cedar_amd_solver_pcg's own (bit for bit)
int cedar_amd_solver_fcg(cedar_amd_solver *s, const real_t *b, real_t *x, const cedar_amd_pcg_settings *settings, real_t *hist)
{
	const char *who = "cedar_amd_solver_fcg";
	if (null_handle(s, who) || semidef_refused(s, who)) return -1;
	const cedar_amd_pcg_settings p = pcg_settings_or_default(settings);
	if (fcg_refused(s, p, who)) return -1;
	return pcg_run(s, 1, b, x, p, hist, nullptr, who, p.precon == CEDAR_AMD_PCG_PRECON_BMG);
}

int cedar_amd_solver_fcg_many(cedar_amd_solver *s, int nrhs, const real_t *b, real_t *x, const cedar_amd_pcg_settings *settings,
                              real_t *hist, int *iters)
{
	const char *who = "cedar_amd_solver_fcg_many";
	if (null_handle(s, who) || semidef_refused(s, who) || many_refused(s, nrhs, who)) return -1;
	const cedar_amd_pcg_settings p = pcg_settings_or_default(settings);
	if (fcg_refused(s, p, who)) return -1;
	return pcg_run(s, nrhs, b, x, p, hist, iters, who, p.precon == CEDAR_AMD_PCG_PRECON_BMG);
}

// Flexible CG on a periodic handle.  The periodic cycle is not a symmetric operator (its coarsest solve removes the mean,
// its sweeps are ordered with the ghost refreshes), so only the flexible beta is offered with it; precon none / diag are
// exactly symmetric and keep the standard beta, as in cedar_amd_solver_fcg.  Every configuration solver_create accepts
// with ibc != 0 holds one right-hand side; a batch handle (max_rhs > 1) is refused.
int cedar_amd_solver_fcg_periodic(cedar_amd_solver *s, const real_t *b, real_t *x, const cedar_amd_pcg_settings *settings,
                                  real_t *hist)
{
	const char *who = "cedar_amd_solver_fcg_periodic";
	if (null_handle(s, who) || semidef_refused(s, who)) return -1;
	const char *why = nullptr;
	if (s->nb_alloc > 1) why = "handles of cedar_amd_solver_create_many with max_rhs > 1 are not supported";
	else if (!b || !x) why = "b and x must not be NULL";
	if (why) {
		char msg[256];
		snprintf(msg, sizeof(msg), "%s: %s; nothing done", who, why);
		print_error(msg);
		return -1;
	}
	if (s->st.ibc == 0) return cedar_amd_solver_fcg(s, b, x, settings, hist);
	const cedar_amd_pcg_settings p = pcg_settings_or_default(settings);
	if (fcg_refused(s, p, who, true)) return -1;
	return pcg_run(s, 1, b, x, p, hist, nullptr, who, p.precon == CEDAR_AMD_PCG_PRECON_BMG);
}

// cedar_amd_solver_fcg_periodic on the first nrhs items of a handle of cedar_amd_solver_create_many_periodic (3D) or
// cedar_amd_solver_create_many_periodic2 (2D), in lockstep
// (the contract of cedar_amd_solver_fcg_many); one right-hand side takes the single-vector path
int cedar_amd_solver_fcg_periodic_many(cedar_amd_solver *s, int nrhs, const real_t *b, real_t *x,
                                       const cedar_amd_pcg_settings *settings, real_t *hist, int *iters)
{
	const char *who = "cedar_amd_solver_fcg_periodic_many";
	if (null_handle(s, who) || semidef_refused(s, who)) return -1;
	if (s->st.ibc == 0) return cedar_amd_solver_fcg_many(s, nrhs, b, x, settings, hist, iters);
	if (many_refused(s, nrhs, who)) return -1;
	if (!b || !x) {
		char msg[256];
		snprintf(msg, sizeof(msg), "%s: b and x must not be NULL; nothing done", who);
		print_error(msg);
		return -1;
	}
	const cedar_amd_pcg_settings p = pcg_settings_or_default(settings);
	if (fcg_refused(s, p, who, true)) return -1;
	return pcg_run(s, nrhs, b, x, p, hist, iters, who, p.precon == CEDAR_AMD_PCG_PRECON_BMG);
}

// Flexible CG on a handle of cedar_amd_solver_create_semidefinite (include/cedar_amd.h): cedar_amd_solver_fcg_periodic's
// rules with the projections of pcg_run; the direction pass follows ibc (Dirichlet forms for 0, wrap-around otherwise)
static bool semidef_wanted(const cedar_amd_solver *s, const real_t *b, const real_t *x, const char *who)
{
	const char *why = nullptr;
	if (!s->semidef) why = "the handle was not made by cedar_amd_solver_create_semidefinite";
	else if (!b || !x) why = "b and x must not be NULL";
	if (!why) return true;
	char msg[256];
	snprintf(msg, sizeof(msg), "%s: %s; nothing done", who, why);
	print_error(msg);
	return false;
}

int cedar_amd_solver_fcg_semidefinite(cedar_amd_solver *s, const real_t *b, real_t *x, const cedar_amd_pcg_settings *settings,
                                      real_t *hist)
{
	const char *who = "cedar_amd_solver_fcg_semidefinite";
	if (null_handle(s, who) || !semidef_wanted(s, b, x, who)) return -1;
	const cedar_amd_pcg_settings p = pcg_settings_or_default(settings);
	if (fcg_refused(s, p, who, true)) return -1;
	return pcg_run(s, 1, b, x, p, hist, nullptr, who, p.precon == CEDAR_AMD_PCG_PRECON_BMG, true);
}

int cedar_amd_solver_fcg_semidefinite_many(cedar_amd_solver *s, int nrhs, const real_t *b, real_t *x,
                                           const cedar_amd_pcg_settings *settings, real_t *hist, int *iters)
{
	const char *who = "cedar_amd_solver_fcg_semidefinite_many";
	if (null_handle(s, who) || !semidef_wanted(s, b, x, who) || many_refused(s, nrhs, who)) return -1;
	const cedar_amd_pcg_settings p = pcg_settings_or_default(settings);
	if (fcg_refused(s, p, who, true)) return -1;
	return pcg_run(s, nrhs, b, x, p, hist, iters, who, p.precon == CEDAR_AMD_PCG_PRECON_BMG, true);
}

void cedar_amd_solver_precondition(cedar_amd_solver *s, real_t *z, const real_t *r)
{
	if (null_handle(s, "cedar_amd_solver_precondition") || semidef_refused(s, "cedar_amd_solver_precondition")) return;
	if (pcg_refused(s, pcg_settings_or_default(nullptr), "cedar_amd_solver_precondition")) return;
	pcg_alloc(s);
	const Level &L = s->lv[0];
	hipStream_t st = current_stream();
	Staged sz(z, L.npts, false, true), sr(r, L.npts, true, false);
	CEDAR_HIP_CHECK(hipMemcpyAsync(s->kr, sr.get(), L.npts * sizeof(real_t), hipMemcpyDeviceToDevice, st));
	pcg_precondition(s, 1, st);
	CEDAR_HIP_CHECK(hipMemcpyAsync(sz.get(), s->kz, L.npts * sizeof(real_t), hipMemcpyDeviceToDevice, st));
	CEDAR_HIP_CHECK(hipStreamSynchronize(st));
	launch_check("cedar_amd_solver_precondition");
}

// ---- plane relaxation as a kernel of its own: kernels::plane_relax<stypes, rdir>::setup / run
// (include/cedar/kernels/plane_relax.h:10-33, include/cedar/3d/relax_planes.h:164-246)
struct cedar_amd_planes {
	cedar_amd_solver *host = nullptr; // carries the side streams
	PlaneSet *ps = nullptr;
	Level L;                          // extents and stencil of the 3D operator
};

cedar_amd_planes *cedar_amd_planes_create(int dir, len_t nx, len_t ny, len_t nz, int nstencil, const real_t *so,
                                          const cedar_amd_settings *plane_settings)
{
	if (dir < 0 || dir > 2 || (nstencil != 4 && nstencil != 14)) {
		char msg[] = "cedar_amd_planes_create: dir must be 0 (xy), 1 (xz) or 2 (yz), nstencil 4 or 14";
		print_error(msg);
		return nullptr;
	}
	hipStream_t st = current_stream();
	cedar_amd_settings pst;
	if (plane_settings) pst = *plane_settings;
	else { // the reference's default plane configuration, src/kernel_params.cc:72-78
		cedar_amd_default_settings(&pst);
		pst.relaxation = CEDAR_AMD_RELAX_LINE_XY;
		pst.max_iter = 1;
	}
	cedar_amd_planes *p = new cedar_amd_planes;
	p->L.nx = (int)nx; p->L.ny = (int)ny; p->L.nz = (int)nz;
	p->L.II = (int)nx + 2; p->L.JJ = (int)ny + 2; p->L.KK = (int)nz + 2;
	p->L.nst = nstencil;
	p->L.npts = (size_t)p->L.II * p->L.JJ * p->L.KK;
	p->host = new cedar_amd_solver;
	p->host->nd = 3;
	plane_streams_create(p->host);
	{
		Staged sso(so, p->L.npts * nstencil, true, false);
		p->ps = planes_setup(dir, sso.get(), p->L.II, p->L.JJ, p->L.KK, nstencil, pst, st);
	}
	if (!p->ps) {
		cedar_amd_solver_destroy(p->host);
		delete p;
		return nullptr;
	}
	return p;
}

void cedar_amd_planes_run(cedar_amd_planes *p, const real_t *so, real_t *x, const real_t *b, int updown)
{
	if (null_handle(p, "cedar_amd_planes_run")) return;
	Staged sso(so, p->L.npts * p->L.nst, true, false), sx(x, p->L.npts, true, true), sb(b, p->L.npts, true, false);
	Level L = p->L;
	L.A = sso.get();
	planes_relax(p->host, *p->ps, L, sx.get(), sb.get(), updown, current_stream());
}

void cedar_amd_planes_destroy(cedar_amd_planes *p)
{
	if (!p) return;
	CEDAR_HIP_CHECK(hipDeviceSynchronize());
	planes_destroy(p->ps);
	cedar_amd_solver_destroy(p->host);
	delete p;
}

float cedar_amd_solver_time_vcycles(cedar_amd_solver *s, real_t *x_dev, const real_t *b_dev, int n)
{
	if (null_handle(s, "cedar_amd_solver_time_vcycles")) return 0.f;
	return timed(current_stream(), [&] {
		for (int i = 0; i < n; i++) cycle_dev(s, x_dev, b_dev);
	});
}

float cedar_amd_solver_time_relax(cedar_amd_solver *s, real_t *x_dev, const real_t *b_dev, int n)
{
	if (null_handle(s, "cedar_amd_solver_time_relax")) return 0.f;
	hipStream_t st = current_stream();
	const Level &L = s->lv[0];
	return timed(st, [&] {
		for (int i = 0; i < n; i++) {
			L.bt_fresh = false; // every timed sweep pays for its own transpose of b (a V(2,1) visit pays two per three sweeps)
			smooth(s, L, x_dev, b_dev, (i & 1) ? BMG_UP : BMG_DOWN, 1, st);
		}
	});
}

// n launches of one level-0 transfer / residual kernel: op 1 = residual (res := b - A x), 2 = restriction of res to level 1,
// 3 = interpolation-and-add from level 1 (overwrites x and res: timing only)
float cedar_amd_solver_time_op(cedar_amd_solver *s, real_t *x_dev, const real_t *b_dev, int op, int n)
{
	if (null_handle(s, "cedar_amd_solver_time_op")) return 0.f;
	if (s->lv.size() < 2 || op < 1 || op > 3) return 0.f;
	hipStream_t st = current_stream();
	Level &L = s->lv[0], &K = s->lv[1];
	const float ms = timed(st, [&] {
		for (int i = 0; i < n; i++) {
			if (op == 1) residual(s, L, x_dev, b_dev, L.res, st);
			else if (op == 2) restrict_to(s, L, K, L.res, st);
			else interp_add_from(s, L, K, x_dev, st);
		}
	});
	launch_check("cedar_amd_solver_time_op");
	return ms;
}

} // extern "C"
