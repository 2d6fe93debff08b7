// Shared pieces of the domain-decomposed solvers (dist3.cpp: 3D, dist2.cpp: 2D on (1, JJ, II) boxes): the rank's place in
// the grid, the transport (RCCL communicator or a caller-supplied table), the ghost-layer exchange and the side stream.
#pragma once
#include "../../include/cedar_amd.h"
#include "common.h"
#include "stage.h"
#include <cstring>
#include <map>
#include <utility>
#include <vector>

namespace cedar_amd {
namespace dist {

struct HaloEntry {
	int o[3];
	int peer;
	int sbox[6], rbox[6];
	size_t size, off;
};

struct HaloGroup {
	std::vector<int> idx;          // entries of the group
	std::vector<int> sboxes, rboxes; // 6 ints per entry
	std::vector<unsigned long long> offs;
};

struct Halo {
	int n[3] = {0, 0, 0};
	std::vector<HaloEntry> nb;
	size_t total = 0;
	HaloGroup grp[5]; // 0 = every neighbour, 1 = across an x face / edge / corner, 2 = the others (y/z),
	                  // 3 = the neighbours in the rank's own z layer (x / y faces and the four edges between them), 4 = the others
	std::map<long, std::pair<real_t *, real_t *>> bufs;
};

// the level-0 vectors of the preconditioned conjugate gradient (dist_pcg), allocated on its first call
struct Krylov {
	real_t *r = nullptr, *z = nullptr, *w = nullptr, *p[2] = {nullptr, nullptr};
	real_t *slab = nullptr, *sc = nullptr;
	real_t *part = nullptr, *gath = nullptr; // this rank's partial sums (2 doubles) and every rank's (2 x world), rank order
	ShellBoxes shell;                        // the ghost cells the neighbours own
};

// what a rank knows about itself and how it talks to the others
struct RankCtx {
	cedar_amd_comm *comm = nullptr;
	cedar_amd_transport tp{};
	bool has_tp = false;
	int rank = 0, world = 1, p[3] = {1, 1, 1}, coord[3] = {0, 0, 0};
	void *side = nullptr; // non-blocking side stream of the overlapped y/z halo
	bool pending = false;
	real_t *scal = nullptr;
	Krylov kry;
};

static inline real_t *dmalloc(size_t n)
{
	return static_cast<real_t *>(cedar_amd_malloc((n ? n : 1) * sizeof(real_t))); // cleared
}

// index range along one axis of extent n+2 for neighbour offset d (cedar_amd/dist.py _rng): d != 0: send = the owned
// layer next to that side, recv = the ghost layer; d == 0: the owned cells plus the ghost cell on every side that is a
// PHYSICAL boundary (those ghosts carry values the serial kernels compute for even extents)
static inline void rng(int d, int n, bool recv, bool has_minus, bool has_plus, int &lo, int &hi)
{
	if (d == 0) { lo = has_minus ? 1 : 0; hi = has_plus ? n + 1 : n + 2; }
	else if (d < 0) { lo = recv ? 0 : 1; hi = lo + 1; }
	else { lo = recv ? n + 1 : n; hi = lo + 1; }
}

static inline bool has_nb(const RankCtx *d, int dim, int side) { return d->coord[dim] + side >= 0 && d->coord[dim] + side < d->p[dim]; }
static inline int rank_of(const RankCtx *d, int ci, int cj, int ck) { return ci + d->p[0] * (cj + d->p[1] * ck); }

// ---- transport
static inline int tp_exchange(RankCtx *d, int ns, const int *speer, const real_t *const *sbuf, const size_t *scount,
                int nr, const int *rpeer, real_t *const *rbuf, const size_t *rcount)
{
	if (ns + nr == 0) return 0;
	if (d->has_tp) return d->tp.exchange(d->tp.ctx, ns, speer, sbuf, scount, nr, rpeer, rbuf, rcount);
	return cedar_amd_comm_exchange(d->comm, ns, speer, sbuf, scount, nr, rpeer, rbuf, rcount);
}

static inline void tp_allgather(RankCtx *d, const real_t *send, real_t *recv, size_t count)
{
	if (d->world == 1) {
		cedar_amd_memcpy_d2d(recv, send, count * sizeof(real_t));
		return;
	}
	const int rc = d->has_tp ? d->tp.allgather(d->tp.ctx, send, recv, count) : cedar_amd_comm_allgather(d->comm, send, recv, count);
	if (rc) { char m[] = "cedar_amd_dist3: all-gather failed"; print_error(m); }
}

static inline double tp_allreduce_sum(RankCtx *d, double v)
{
	if (d->world == 1) return v;
	if (d->has_tp) {
		if (d->tp.allreduce_sum(d->tp.ctx, &v, 1)) { char m[] = "cedar_amd_dist3: all-reduce failed"; print_error(m); }
		return v;
	}
	cedar_amd_memcpy_h2d(d->scal, &v, sizeof(double));
	if (cedar_amd_comm_allreduce_sum(d->comm, d->scal, 1)) { char m[] = "cedar_amd_dist3: all-reduce failed"; print_error(m); }
	cedar_amd_memcpy_d2h(&v, d->scal, sizeof(double));
	return v;
}

// ---- halo (cedar_amd/dist.py Halo)
static inline void halo_init(RankCtx *d, Halo &h, const int n[3])
{
	for (int t = 0; t < 3; t++) h.n[t] = n[t];
	bool hm[3], hp[3];
	for (int t = 0; t < 3; t++) { hm[t] = has_nb(d, t, -1); hp[t] = has_nb(d, t, +1); }
	size_t off = 0;
	// neighbours in the order of the sorted offsets (dx, dy, dz), as dist.py: both ends of a message agree on the layout
	for (int dx = -1; dx <= 1; dx++)
		for (int dy = -1; dy <= 1; dy++)
			for (int dz = -1; dz <= 1; dz++) {
				if (!dx && !dy && !dz) continue;
				const int c[3] = {d->coord[0] + dx, d->coord[1] + dy, d->coord[2] + dz};
				if (c[0] < 0 || c[0] >= d->p[0] || c[1] < 0 || c[1] >= d->p[1] || c[2] < 0 || c[2] >= d->p[2]) continue;
				HaloEntry e;
				e.o[0] = dx; e.o[1] = dy; e.o[2] = dz;
				e.peer = rank_of(d, c[0], c[1], c[2]);
				int lo[3], hi[3];
				for (int t = 0; t < 3; t++) rng(e.o[t], n[t], false, hm[t], hp[t], lo[t], hi[t]);
				for (int t = 0; t < 3; t++) { e.sbox[t] = lo[t]; e.sbox[3 + t] = hi[t] - lo[t]; }
				for (int t = 0; t < 3; t++) rng(e.o[t], n[t], true, hm[t], hp[t], lo[t], hi[t]);
				for (int t = 0; t < 3; t++) { e.rbox[t] = lo[t]; e.rbox[3 + t] = hi[t] - lo[t]; }
				e.size = (size_t)e.sbox[3] * e.sbox[4] * e.sbox[5];
				e.off = off;
				off += e.size;
				h.nb.push_back(e);
			}
	h.total = off;
	for (int g = 0; g < 5; g++) {
		HaloGroup &G = h.grp[g];
		for (size_t i = 0; i < h.nb.size(); i++) {
			const HaloEntry &e = h.nb[i];
			if ((g == 1 && e.o[0] == 0) || (g == 2 && e.o[0] != 0) || (g == 3 && e.o[2] != 0) || (g == 4 && e.o[2] == 0)) continue;
			G.idx.push_back((int)i);
			for (int t = 0; t < 6; t++) { G.sboxes.push_back(e.sbox[t]); G.rboxes.push_back(e.rbox[t]); }
			G.offs.push_back((unsigned long long)e.off);
		}
	}
}

static inline std::pair<real_t *, real_t *> &halo_bufs(Halo &h, long key, size_t count)
{
	auto it = h.bufs.find(key);
	if (it == h.bufs.end()) it = h.bufs.emplace(key, std::make_pair(dmalloc(count), dmalloc(count))).first;
	return it->second;
}

// fill every ghost cell owned by a neighbour of the group: pack (one launch) -> one grouped exchange -> unpack
static inline void halo_exchange(RankCtx *d, Halo &h, int II, int JJ, int KK, real_t *arr, int nplanes, int group)
{
	HaloGroup &G = h.grp[group];
	if (G.idx.empty()) return;
	auto &bp = halo_bufs(h, nplanes, h.total * (size_t)nplanes);
	real_t *sb = bp.first, *rb = bp.second;
	const int nbx = (int)G.idx.size();
	cedar_amd_box_copy(arr, II, JJ, KK, nplanes, nbx, G.sboxes.data(), G.offs.data(), sb, 0);
	int peer[26];
	const real_t *sp[26];
	real_t *rp[26];
	size_t cnt[26];
	for (int i = 0; i < nbx; i++) {
		const HaloEntry &e = h.nb[G.idx[i]];
		peer[i] = e.peer;
		sp[i] = sb + e.off * (size_t)nplanes;
		rp[i] = rb + e.off * (size_t)nplanes;
		cnt[i] = e.size * (size_t)nplanes;
	}
	if (tp_exchange(d, nbx, peer, sp, cnt, nbx, peer, rp, cnt)) { char m[] = "cedar_amd_dist3: halo exchange failed"; print_error(m); }
	cedar_amd_box_copy(arr, II, JJ, KK, nplanes, nbx, G.rboxes.data(), G.offs.data(), rb, 1);
}

// The ghost cells of this rank's own z layer / across z that one stage of the boundary-first chain has changed: of the
// messages selected by `send` / `recv` (neighbour offsets) only the rows with index parity jpar_of(offset) and the planes
// with index parity kpar (-1: all).  Local extents are even along split directions, so a row or plane has the same parity on both
// ends of a message and both ends find the same boxes (an empty one is no message).
template <class FS, class FR, class FJ>
static inline void halo_exchange_sub(RankCtx *d, Halo &h, int II, int JJ, int KK, real_t *arr, FS send, FR recv, FJ jpar_of, int kpar)
{
	if (h.nb.empty()) return;
	auto &bp = halo_bufs(h, 1, h.total);
	real_t *sb = bp.first, *rb = bp.second;
	int sboxes[26 * 8], rboxes[26 * 8], speer[26], rpeer[26], ns = 0, nr = 0;
	unsigned long long soffs[26], roffs[26];
	const real_t *sp[26];
	real_t *rp[26];
	size_t scnt[26], rcnt[26];
	auto restrict_box = [&](const int *box, int *out, int jpar) -> size_t {
		int j0 = box[1], nj = box[4], sj = 1, k0 = box[2], nk = box[5], sk = 1;
		if (jpar >= 0) { const int f = ((j0 & 1) == jpar) ? j0 : j0 + 1; nj = (j0 + nj - f + 1) / 2; j0 = f; sj = 2; }
		if (kpar >= 0) { const int f = ((k0 & 1) == kpar) ? k0 : k0 + 1; nk = (k0 + nk - f + 1) / 2; k0 = f; sk = 2; }
		if (nj < 0) nj = 0;
		if (nk < 0) nk = 0;
		out[0] = box[0]; out[1] = j0; out[2] = k0; out[3] = box[3]; out[4] = nj; out[5] = nk; out[6] = sj; out[7] = sk;
		return (size_t)box[3] * nj * nk;
	};
	for (const HaloEntry &e : h.nb) {
		if (send(e.o)) {
			const size_t c = restrict_box(e.sbox, sboxes + 8 * ns, jpar_of(e.o));
			if (c) { speer[ns] = e.peer; soffs[ns] = e.off; sp[ns] = sb + e.off; scnt[ns] = c; ns++; }
		}
		if (recv(e.o)) {
			const size_t c = restrict_box(e.rbox, rboxes + 8 * nr, jpar_of(e.o));
			if (c) { rpeer[nr] = e.peer; roffs[nr] = e.off; rp[nr] = rb + e.off; rcnt[nr] = c; nr++; }
		}
	}
	if (ns) cedar_amd_box_copy_strided(arr, II, JJ, KK, 1, ns, sboxes, soffs, sb, 0);
	if (tp_exchange(d, ns, speer, sp, scnt, nr, rpeer, rp, rcnt)) { char m[] = "cedar_amd_dist3: halo exchange failed"; print_error(m); }
	if (nr) cedar_amd_box_copy_strided(arr, II, JJ, KK, 1, nr, rboxes, roffs, rb, 1);
}

// x faces only (owned j,k): to_minus: first owned column to the -x neighbour, the +x neighbour's into the high ghost
// column (UP order); else the mirror image.  Returns true if a column was received.
static inline bool halo_exchange_x(RankCtx *d, Halo &h, int II, int JJ, int KK, real_t *arr, bool to_minus)
{
	const int nx = h.n[0], ny = h.n[1], nz = h.n[2] < 1 ? 1 : h.n[2], k0 = h.n[2] < 1 ? 0 : 1; // 2D boxes: the one plane k = 0
	const int send_to = to_minus ? -1 : +1, send_col = to_minus ? 1 : nx, recv_from = -send_to, recv_col = to_minus ? nx + 1 : 0;
	auto &bp = halo_bufs(h, to_minus ? -1 : -2, (size_t)ny * nz);
	const unsigned long long zero = 0;
	int speer = 0, rpeer = 0, ns = 0, nr = 0;
	const real_t *sp = bp.first;
	real_t *rp = bp.second;
	size_t cnt = (size_t)ny * nz;
	if (has_nb(d, 0, send_to)) {
		const int box[6] = {send_col, 1, k0, 1, ny, nz};
		cedar_amd_box_copy(arr, II, JJ, KK, 1, 1, box, &zero, bp.first, 0);
		speer = rank_of(d, d->coord[0] + send_to, d->coord[1], d->coord[2]);
		ns = 1;
	}
	if (has_nb(d, 0, recv_from)) {
		rpeer = rank_of(d, d->coord[0] + recv_from, d->coord[1], d->coord[2]);
		nr = 1;
	}
	if (tp_exchange(d, ns, &speer, &sp, &cnt, nr, &rpeer, &rp, &cnt)) { char m[] = "cedar_amd_dist3: x-face exchange failed"; print_error(m); }
	if (nr) {
		const int box[6] = {recv_col, 1, k0, 1, ny, nz};
		cedar_amd_box_copy(arr, II, JJ, KK, 1, 1, box, &zero, bp.second, 1);
	}
	return nr != 0;
}

// ---- side stream: work issued between side_begin / side_end goes to the side stream, ordered after everything
// already queued on the main stream; side_wait orders the main stream after it
static inline void *side_begin(RankCtx *d)
{
	if (!d->side) d->side = cedar_amd_stream_create();
	void *main_st = cedar_amd_get_stream();
	cedar_amd_stream_wait(d->side, main_st);
	cedar_amd_set_stream(d->side);
	return main_st;
}
static inline void side_end(RankCtx *d, void *main_st)
{
	cedar_amd_set_stream(main_st);
	d->pending = true;
}
static inline void side_wait(RankCtx *d)
{
	if (!d->pending) return;
	cedar_amd_stream_wait(cedar_amd_get_stream(), d->side);
	d->pending = false;
}

// ---- preconditioned conjugate gradient on a rank grid (cedar_amd_dist3_pcg / cedar_amd_dist2_pcg).
// The serial iteration (solver.cpp cedar_amd_solver_pcg) on the rank's level-0 box with krylov.hip's passes, plus:
//  - z's ghosts by one halo exchange once z is formed; p' = z + beta p on the ghost shell by pcg_ghost_shell (the value
//    the owning neighbour forms, beta being the same everywhere), so the direction pass reads current ghosts of both;
//  - every scalar from this rank's slab sums, all-gathered and summed in rank order on the device: the same bits on every
//    rank, hence the same stop / breakdown decision.  Two all-gathers per iteration: p'.w, then r.r with r.z after the
//    preconditioner (the serial stop test reads r.r before it; here the stop test waits for the preconditioned residual).
struct PcgBox { // what the driver needs of level 0
	int nd, nst, II, JJ, KK;
	size_t npts;
	const real_t *A;
	const Op3 *op27;
	Halo *halo;
};

// settings a rank grid cannot honour, decided from the handle's settings and p alone (every rank decides alike, before
// any communication)
static inline bool dist_pcg_refused(int pre, int post, const cedar_amd_pcg_settings &p, const char *who)
{
	const char *why = nullptr;
	if (p.stop_test < CEDAR_AMD_PCG_STOP_ABS_RES_L2 || p.stop_test > CEDAR_AMD_PCG_STOP_REL_RES_M2) why = "stop_test must be 0..3";
	else if (p.precon < CEDAR_AMD_PCG_PRECON_NONE || p.precon > CEDAR_AMD_PCG_PRECON_BMG) why = "precon must be 1..3";
	else if (p.max_iter < 0) why = "max_iter must not be negative";
	else if (p.precon == CEDAR_AMD_PCG_PRECON_BMG) {
		if (pre != post) why = "the multigrid preconditioner needs nrelax_pre == nrelax_post (symmetric V-cycle)";
		else if (p.nmg_cycles < 1) why = "nmg_cycles must be at least 1";
	}
	if (!why) return false;
	char msg[256];
	snprintf(msg, sizeof(msg), "%s: %s; nothing done", who, why);
	print_error(msg);
	return true;
}

static inline void krylov_alloc(RankCtx *d, const PcgBox &B)
{
	Krylov &K = d->kry;
	if (K.r) return;
	// zero-filled: the physical-boundary ghosts of every vector stay zero (the kernels write interiors and the shell)
	K.r = dmalloc(B.npts); K.z = dmalloc(B.npts); K.w = dmalloc(B.npts);
	K.p[0] = dmalloc(B.npts); K.p[1] = dmalloc(B.npts);
	K.slab = dmalloc(pcg_slab_doubles(B.nd, B.nst, B.II, B.JJ, B.KK));
	K.sc = dmalloc(PCG_NSC);
	K.part = dmalloc(2);
	K.gath = dmalloc(2 * (size_t)d->world);
	// the halo's receive boxes, cut to the owned range along the directions the message does not cross
	const Halo &h = *B.halo;
	K.shell.n = 0;
	for (const HaloEntry &e : h.nb) {
		int *o = K.shell.box + 6 * K.shell.n++;
		for (int t = 0; t < 3; t++) {
			o[t] = e.rbox[t]; o[3 + t] = e.rbox[3 + t];
			if (e.o[t] == 0 && h.n[t] >= 1) { o[t] = 1; o[3 + t] = h.n[t]; }
		}
	}
}

static inline void krylov_free(RankCtx *d)
{
	Krylov &K = d->kry;
	cedar_amd_free(K.r); cedar_amd_free(K.z); cedar_amd_free(K.w); cedar_amd_free(K.p[0]); cedar_amd_free(K.p[1]);
	cedar_amd_free(K.slab); cedar_amd_free(K.sc); cedar_amd_free(K.part); cedar_amd_free(K.gath);
	K = Krylov();
}

// resid(x, b, r): r = b - A x on the interior (x's ghosts current); vcycle(x, b): one cycle of the rank grid
template <class Resid, class Cycle>
int dist_pcg(RankCtx *d, const PcgBox &B, int pre, int post, const real_t *b, real_t *x, const cedar_amd_pcg_settings *settings,
             real_t *hist, const char *who, Resid resid, Cycle vcycle)
{
	const cedar_amd_pcg_settings p = pcg_settings_or_default(settings);
	if (dist_pcg_refused(pre, post, p, who)) return -1;
	krylov_alloc(d, B);
	Krylov &K = d->kry;
	hipStream_t st = current_stream();
	const PcgRule rule = pcg_rule(p);
	const int zm = rule.zm;
	real_t *Z = zm == 0 ? K.r : K.z;
	auto exch = [&](real_t *a) { halo_exchange(d, *B.halo, B.II, B.JJ, B.KK, a, 1, 0); };
	auto precondition = [&]() {
		CEDAR_HIP_CHECK(hipMemsetAsync(K.z, 0, B.npts * sizeof(real_t), st));
		for (int c = 0; c < p.nmg_cycles; c++) vcycle(K.z, K.r);
	};
	// r.r and r.z of the current residual over all ranks (rho, beta on the device), z's ghosts, then the one host read
	double sc[PCG_NSC];
	auto dots = [&](int zmode, bool move, const real_t *pn, bool first) {
		pcg_update(zmode, move, x, K.r, pn, K.w, Z, B.A, B.II, B.JJ, B.KK, first, K.slab, K.sc, st, K.part);
		tp_allgather(d, K.part, K.gath, 2);
		pcg_ranks_rho(zmode, K.gath, d->world, 2, first, K.sc, st);
		exch(Z);
		CEDAR_HIP_CHECK(hipMemcpyAsync(sc, K.sc, PCG_NSC * sizeof(double), hipMemcpyDeviceToHost, st));
		CEDAR_HIP_CHECK(hipStreamSynchronize(st));
	};

	CEDAR_HIP_CHECK(hipMemsetAsync(K.sc, 0, PCG_NSC * sizeof(real_t), st));
	exch(x);
	resid(x, b, K.r);
	if (zm == 2) precondition();
	dots(zm, false, nullptr, true);
	const double r0 = std::sqrt(sc[PCG_RR]), m0 = std::sqrt(sc[PCG_RZ] > 0 ? sc[PCG_RZ] : 0.0);
	if (hist) hist[0] = r0;
	int it = 0;
	if (!(r0 == 0.0 || !(sc[PCG_RZ] > 0) || rule.stop(sc[PCG_RR], sc[PCG_RZ], r0, m0)))
		for (int k = 0; k < p.max_iter; k++) {
			real_t *pold = K.p[(k + 1) & 1], *pn = K.p[k & 1];
			pcg_direction(B.A, B.op27, Z, pold, pn, K.w, B.nd, B.nst, B.II, B.JJ, B.KK, k == 0, K.slab, K.sc, st, K.part);
			tp_allgather(d, K.part, K.gath, 1);
			pcg_ranks_alpha(K.gath, d->world, 1, K.sc, st);
			pcg_ghost_shell(Z, pold, pn, K.sc, K.shell, B.II, B.JJ, k == 0, st); // before the update changes z (zm 0, 1)
			if (zm == 2) {
				pcg_update(3, true, x, K.r, pn, K.w, Z, B.A, B.II, B.JJ, B.KK, false, K.slab, K.sc, st, K.part);
				precondition();
				dots(2, false, nullptr, false);
			} else
				dots(zm, true, pn, false);
			if (sc[PCG_FLAG] != 0) break; // breakdown (p.Ap <= 0 or rho = 0): alpha was 0, x is as it was
			it = k + 1;
			if (hist) hist[it] = std::sqrt(sc[PCG_RR]) / r0;
			if (rule.stop(sc[PCG_RR], sc[PCG_RZ], r0, m0)) break;
		}
	exch(x); // the caller's box as cedar_amd_dist*_solve leaves it: ghosts current
	return it;
}

// z = M^-1 r: one cycle of the rank grid from z = 0, z's ghosts exchanged
template <class Cycle>
void dist_precondition(RankCtx *d, const PcgBox &B, int pre, int post, real_t *z, real_t *r, const char *who, Cycle vcycle)
{
	if (dist_pcg_refused(pre, post, pcg_settings_or_default(nullptr), who)) return;
	CEDAR_HIP_CHECK(hipMemsetAsync(z, 0, B.npts * sizeof(real_t), current_stream()));
	vcycle(z, r);
	halo_exchange(d, *B.halo, B.II, B.JJ, B.KK, z, 1, 0);
}


} // namespace dist
} // namespace cedar_amd
