// The driver the two domain-decomposed solvers share (dist3.cpp: 3D, dist2.cpp: 2D): what a level and a handle hold in
// either dimension, the gather of the coarsest distributed level with the single-domain solver that takes over there, the
// planning of the levels in create, the cycle and the solve loop.  2D is the KK = 1, n[2] = -1 convention of halo_init and
// halo_exchange_x: one plane k = 0 without ghost planes, p[2] = 1, coord[2] = 0.
//
// The cycle, the solve loop and the wrappers are templates over the handle type H (a HandleBase with a vector `lv` of its
// own levels).  They call what the including file declares for its levels:
//   smooth(d, L, x, b, updown, nsweeps)      residual(L, x, b, r)
//   restrict_residual(L, K)                  interp_add(L, K, x)
#pragma once
#include "dist_common.h"
#include <cmath>

namespace cedar_amd {
namespace dist {

struct LevelBase {
	int n[3] = {0, 0, 0};
	int II = 0, JJ = 0, KK = 0, nst = 0;
	size_t npts = 0;
	real_t *A = nullptr, *P = nullptr, *x = nullptr, *b = nullptr, *res = nullptr, *sor = nullptr;
	bool ownA = true;
	Halo halo;
};

struct HandleBase : RankCtx {
	int nd = 3;
	int pre = 2, post = 1, max_iter = 10, min_coarse = 3, agglomerate_below = 64;
	double tol = 1e-8;
	int nlev_global = 1, la = 0;
	int cn[3] = {0, 0, 0}; // owned cells of this rank's block of level la (2D: cn[2] = 1)
	int gII = 0, gJJ = 0, gKK = 0;
	real_t *gA = nullptr, *gx = nullptr, *gb = nullptr, *cs_tmp = nullptr;
	cedar_amd_solver *serial = nullptr;
	std::map<long, std::pair<real_t *, real_t *>> gbuf;
};

// what differs between the two create calls before the first level is set up
struct CreateSpec {
	const char *who;       // the entry point's name: the prefix of every message
	const char *operators; // the operators level 0 may hold, as the message names them
	const char *grid_rule; // what the rank grid has to satisfy, as the message says it
	int nd, nst0[2];       // stencil planes level 0 may have
	int max_ranks;         // per direction (0: no limit)
	int nst_coarse, interp_planes; // stencil and interpolation planes of the levels below level 0
};

static inline void exch(RankCtx *d, LevelBase &L, real_t *arr, int nplanes) { halo_exchange(d, L.halo, L.II, L.JJ, L.KK, arr, nplanes, 0); }

// ---- gather of a level onto every rank (replaces the reference's redistribution solver)
static inline void gather_into(HandleBase *d, real_t *local, const LevelBase &L, int nplanes, real_t *glob)
{
	const int nx = d->cn[0], ny = d->cn[1], nz = d->cn[2], k0 = d->nd == 2 ? 0 : 1;
	const size_t blk = (size_t)nx * ny * nz;
	auto it = d->gbuf.find(nplanes);
	if (it == d->gbuf.end())
		it = d->gbuf.emplace((long)nplanes, std::make_pair(dmalloc(blk * nplanes), dmalloc(blk * nplanes * d->world))).first;
	real_t *sb = it->second.first, *rb = it->second.second;
	const int own[6] = {1, 1, k0, nx, ny, nz};
	const unsigned long long zero = 0;
	cedar_amd_box_copy(local, L.II, L.JJ, L.KK, nplanes, 1, own, &zero, sb, 0);
	tp_allgather(d, sb, rb, blk * nplanes);
	// unpack every rank's block at its place; the box table of one launch holds 26 boxes
	for (int r0 = 0; r0 < d->world; r0 += 26) {
		const int nb = d->world - r0 < 26 ? d->world - r0 : 26;
		int boxes[26 * 6];
		unsigned long long offs[26];
		for (int i = 0; i < nb; i++) {
			const int r = r0 + i, ci = r % d->p[0], cj = (r / d->p[0]) % d->p[1], ck = r / (d->p[0] * d->p[1]);
			const int b[6] = {1 + ci * nx, 1 + cj * ny, k0 + ck * nz, nx, ny, nz};
			memcpy(boxes + 6 * i, b, sizeof(b));
			offs[i] = (unsigned long long)r * blk;
		}
		cedar_amd_box_copy(glob, d->gII, d->gJJ, d->gKK, nplanes, nb, boxes, offs, rb, 1);
	}
}

// levels la.. : gather the right-hand side, one single-domain cycle (or the direct solve) from a zero initial guess,
// keep the own block + ghosts straight from the global solution
static inline void coarse_solve(HandleBase *d, LevelBase &C, real_t *x, real_t *b)
{
	gather_into(d, b, C, 1, d->gb);
	cedar_amd_memset(d->gx, 0, (size_t)d->gII * d->gJJ * d->gKK * sizeof(real_t));
	cedar_amd_solver_vcycle(d->serial, d->gx, d->gb);
	const int nx = d->cn[0], ny = d->cn[1], nz = d->cn[2], gz = d->nd == 2 ? 0 : 2; // no ghost planes around the one 2D plane
	const unsigned long long zero = 0;
	const int from[6] = {d->coord[0] * nx, d->coord[1] * ny, d->coord[2] * nz, nx + 2, ny + 2, nz + gz};
	const int to[6] = {0, 0, 0, nx + 2, ny + 2, nz + gz};
	cedar_amd_box_copy(d->gx, d->gII, d->gJJ, d->gKK, 1, 1, from, &zero, d->cs_tmp, 0);
	cedar_amd_box_copy(x, C.II, C.JJ, C.KK, 1, 1, to, &zero, d->cs_tmp, 1);
}

static inline double norm(HandleBase *d, LevelBase &L, const real_t *r)
{
	const double v = cedar_amd_l2norm(r, L.II, L.JJ, L.KK);
	return std::sqrt(tp_allreduce_sum(d, v * v));
}

// ---- create
// The refusals that need no handle, then the handle with its place in the rank grid and its settings (`st`: what the
// caller goes on reading).  pg: the rank grid, three entries.  NULL after a printed reason.
template <class H>
H *create_handle(const CreateSpec &S, cedar_amd_comm *comm, const cedar_amd_transport *transport, int rank, int world, const int pg[3],
                 const real_t *A_local, int nstencil, const cedar_amd_settings *settings, int agglomerate_below, cedar_amd_settings &st)
{
	char msg[160];
	if (!A_local || !is_device_ptr(A_local) || (nstencil != S.nst0[0] && nstencil != S.nst0[1]) || world < 1 || rank < 0 || rank >= world) {
		snprintf(msg, sizeof(msg), "%s: A_local must be a device array of a %s operator, 0 <= rank < world", S.who, S.operators);
		print_error(msg);
		return nullptr;
	}
	if (world > 1 && !comm && !(transport && transport->exchange && transport->allgather && transport->allreduce_sum)) {
		snprintf(msg, sizeof(msg), "%s: more than one rank needs a communicator (cedar_amd_comm_create) or a transport table", S.who);
		print_error(msg);
		return nullptr;
	}
	bool fits = pg[0] * pg[1] * pg[2] == world;
	for (int t = 0; t < 3; t++) fits = fits && (S.max_ranks == 0 || pg[t] <= S.max_ranks);
	if (!fits) {
		snprintf(msg, sizeof(msg), "%s: the rank grid %s", S.who, S.grid_rule);
		print_error(msg);
		return nullptr;
	}
	H *d = new H;
	d->nd = S.nd;
	d->comm = comm;
	if (transport && transport->exchange) { d->tp = *transport; d->has_tp = true; }
	d->rank = rank; d->world = world;
	for (int t = 0; t < 3; t++) d->p[t] = pg[t];
	d->coord[0] = rank % d->p[0]; d->coord[1] = (rank / d->p[0]) % d->p[1]; d->coord[2] = rank / (d->p[0] * d->p[1]);
	if (settings) st = *settings;
	else cedar_amd_default_settings(&st);
	d->pre = st.nrelax_pre; d->post = st.nrelax_post; d->max_iter = st.max_iter; d->tol = st.tol; d->min_coarse = st.min_coarse;
	d->agglomerate_below = agglomerate_below > 0 ? agglomerate_below : 64;
	return d;
}

// The levels of the handle from the local extents n of level 0: the global level count, the distributed levels 0 .. la
// with their halo and their arrays.  False after a printed reason (the caller destroys the handle: levels may exist).
template <class H>
bool plan_levels(H *d, const CreateSpec &S, real_t *A_local, int nstencil, const int n0[3])
{
	const int nd = S.nd;
	d->scal = dmalloc(8);
	int n[3] = {n0[0], n0[1], nd == 2 ? -1 : n0[2]};
	auto coarsen = [&](int *v) {
		for (int t = 0; t < nd; t++) v[t] = d->p[t] == 1 ? (int)((v[t] - 1) / 2.0 + 1) : v[t] / 2;
	};
	// number of levels from the GLOBAL extents (include/cedar/3d/solver.h:54-72, include/cedar/2d/solver.h:57-73)
	int ng = 0;
	for (;;) {
		ng++;
		int m = 1 << 30;
		for (int t = 0; t < nd; t++) {
			const int g = n[t] * d->p[t], c = (g - 1) / (1 << ng) + 1;
			if (c < m) m = c;
		}
		if (m < d->min_coarse) break;
	}
	d->nlev_global = ng;
	// distributed levels 0 .. la; level la is gathered and handed to the single-domain solver
	int la = ng - 1, m[3] = {n[0], n[1], n[2]};
	for (int l = 1; l < ng; l++) {
		coarsen(m);
		int mn = 1 << 30;
		for (int t = 0; t < nd; t++)
			if (m[t] < mn) mn = m[t];
		if (mn <= d->agglomerate_below) { la = l; break; }
	}
	d->la = ng > 1 ? (la > 1 ? la : 1) : 0;
	for (int l = 0; l <= d->la; l++) {
		for (int t = 0; t < nd; t++)
			if (d->p[t] > 1 && l < d->la && (n[t] & 1)) {
				char msg[160];
				snprintf(msg, sizeof(msg), "%s: level %d: local extent %d along a split direction must be even", S.who, l, n[t]);
				print_error(msg);
				return false;
			}
		d->lv.emplace_back();
		auto &R = d->lv.back();
		for (int t = 0; t < 3; t++) R.n[t] = n[t];
		R.II = n[0] + 2; R.JJ = n[1] + 2; R.KK = nd == 2 ? 1 : n[2] + 2;
		R.npts = (size_t)R.II * R.JJ * R.KK;
		halo_init(d, R.halo, n);
		R.res = dmalloc(R.npts);
		R.sor = dmalloc(2 * R.npts);
		if (l == 0) {
			R.A = A_local; R.ownA = false; R.nst = nstencil;
		} else {
			R.nst = S.nst_coarse;
			R.A = dmalloc(S.nst_coarse * R.npts);
			R.P = dmalloc(S.interp_planes * R.npts);
			R.x = dmalloc(R.npts);
			R.b = dmalloc(R.npts);
		}
		coarsen(n);
	}
	return true;
}

// the end of set-up -- level la: the global operator on every rank; the single-domain device-resident solver takes over
// from there
static inline void setup_serial(HandleBase *d, LevelBase &C, int relaxation)
{
	const int gz = d->nd == 2 ? 0 : 2;
	d->cn[0] = C.n[0]; d->cn[1] = C.n[1]; d->cn[2] = d->nd == 2 ? 1 : C.n[2];
	d->gII = d->cn[0] * d->p[0] + 2; d->gJJ = d->cn[1] * d->p[1] + 2; d->gKK = d->cn[2] * d->p[2] + gz;
	const size_t gp = (size_t)d->gII * d->gJJ * d->gKK;
	d->gA = dmalloc(gp * C.nst);
	gather_into(d, C.A, C, C.nst, d->gA);
	d->gx = dmalloc(gp);
	d->gb = dmalloc(gp);
	d->cs_tmp = dmalloc((size_t)(d->cn[0] + 2) * (d->cn[1] + 2) * (d->cn[2] + gz));
	cedar_amd_settings st;
	cedar_amd_default_settings(&st);
	st.relaxation = relaxation;
	st.nrelax_pre = d->pre; st.nrelax_post = d->post; st.min_coarse = d->min_coarse;
	st.num_levels = d->nlev_global - d->la;
	d->serial = cedar_amd_solver_create(d->nd, (len_t)(d->gII - 2), (len_t)(d->gJJ - 2), (len_t)(d->gKK - gz), C.nst, d->gA, 1, &st);
}

// what both handles own, after a device sync; the caller frees what only its levels have, then deletes the handle
template <class H>
void destroy_shared(H *d)
{
	cedar_amd_device_sync();
	if (d->serial) cedar_amd_solver_destroy(d->serial);
	for (auto &L : d->lv) {
		if (L.ownA) cedar_amd_free(L.A);
		cedar_amd_free(L.P); cedar_amd_free(L.x); cedar_amd_free(L.b); cedar_amd_free(L.res); cedar_amd_free(L.sor);
		for (auto &kv : L.halo.bufs) { cedar_amd_free(kv.second.first); cedar_amd_free(kv.second.second); }
	}
	for (auto &kv : d->gbuf) { cedar_amd_free(kv.second.first); cedar_amd_free(kv.second.second); }
	cedar_amd_free(d->gA); cedar_amd_free(d->gx); cedar_amd_free(d->gb); cedar_amd_free(d->cs_tmp); cedar_amd_free(d->scal);
	krylov_free(d);
	if (d->side) cedar_amd_stream_destroy(d->side);
}

// ---- cycle
template <class H>
void cycle(H *d, int l, real_t *x, real_t *b)
{
	auto &L = d->lv[l], &K = d->lv[l + 1];
	smooth(d, L, x, b, BMG_DOWN, d->pre);
	residual(L, x, b, L.res);
	exch(d, L, L.res, 1);
	restrict_residual(L, K);
	cedar_amd_memset(K.x, 0, K.npts * sizeof(real_t));
	if (l + 1 == (int)d->lv.size() - 1) coarse_solve(d, K, K.x, K.b);
	else cycle(d, l + 1, K.x, K.b);
	interp_add(L, K, x);
	exch(d, L, x, 1);
	smooth(d, L, x, b, BMG_UP, d->post);
}

template <class H>
void vcycle(H *d, real_t *x, real_t *b)
{
	if (d->lv.size() == 1) coarse_solve(d, d->lv[0], x, b);
	else cycle(d, 0, x, b);
}

// multilevel::solve (multilevel.h:277-298) after mpi::solver::solve's halo of the iterate (3d/mpi/solver.h:76-89);
// rel[0] = ||r0||_2, rel[i] = ||r_i||_2 / ||r0||_2; returns the number of cycles run
template <class H>
int solve(H *d, real_t *b, real_t *x, real_t *rel, const char *who)
{
	auto &L = d->lv[0];
	exch(d, L, x, 1);
	residual(L, x, b, L.res);
	const double r0 = norm(d, L, L.res);
	rel[0] = r0;
	int it = 0;
	while (it < d->max_iter) {
		vcycle(d, x, b);
		residual(L, x, b, L.res);
		const double r = norm(d, L, L.res) / r0;
		rel[++it] = r;
		if (r < d->tol) break;
	}
	launch_check(who);
	return it;
}

// preconditioned conjugate gradient on the rank grid (dist_common.h dist_pcg) on the level-0 box, the distributed V-cycle
// as the preconditioner; op27: the row-interleaved copy of a 27-point operator where set-up registered one, or NULL
template <class H>
int pcg(H *d, real_t *b, real_t *x, const cedar_amd_pcg_settings *p, real_t *hist, const Op3 *op27, const char *who)
{
	auto &L = d->lv[0];
	const PcgBox B{d->nd, L.nst, L.II, L.JJ, L.KK, L.npts, L.A, op27, &L.halo};
	const int it = dist_pcg(d, B, d->pre, d->post, b, x, p, hist, who,
	                        [&](real_t *xx, const real_t *bb, real_t *r) { residual(L, xx, const_cast<real_t *>(bb), r); },
	                        [&](real_t *xx, real_t *bb) { vcycle(d, xx, bb); });
	launch_check(who);
	return it;
}

template <class H>
void precondition(H *d, real_t *z, real_t *r, const char *who)
{
	auto &L = d->lv[0];
	const PcgBox B{d->nd, L.nst, L.II, L.JJ, L.KK, L.npts, L.A, nullptr, &L.halo};
	dist_precondition(d, B, d->pre, d->post, z, r, who, [&](real_t *xx, real_t *bb) { vcycle(d, xx, bb); });
	launch_check(who);
}

// n level-0 relax sweeps alternating DOWN / UP with their halo exchanges (the roofline microbenchmark of the
// decomposed path); elapsed milliseconds by HIP events on the library's stream
template <class H>
float time_relax(H *d, real_t *x, real_t *b, int n)
{
	void *e0 = cedar_amd_event_record();
	for (int i = 0; i < n; i++) smooth(d, d->lv[0], x, b, (i & 1) ? BMG_UP : BMG_DOWN, 1);
	void *e1 = cedar_amd_event_record();
	const float ms = cedar_amd_event_elapsed_ms(e0, e1);
	cedar_amd_event_destroy(e0);
	cedar_amd_event_destroy(e1);
	return ms;
}

} // namespace dist
} // namespace cedar_amd
