// Krylov kernels of the multigrid-preconditioned conjugate gradient (solver.cpp cedar_amd_solver_pcg): the vector
// work of one CG iteration in three streaming passes, with the scalars (alpha, beta) computed on the device.
//
//   pcg_direction  p' = z + beta p, w = A p', sigma = p'.w          (p' in the other buffer of a pair: p is read at
//                  the stencil neighbours, so it cannot be overwritten in place)
//   pcg_direction_periodic   the same pass on a level with periodic directions (cedar_amd_solver_fcg_periodic): the
//                  neighbours across a periodic boundary are read at the opposite interior end; same bytes per point
//   pcg_update    x += alpha p', r -= alpha w, r.r  [precon = diag: z = r / a_ii and r.z fused]
//                  or, without the x / r update: r.r and r.z of the preconditioned residual
//
// Every pass streams the interior only, leaves one partial sum per workgroup in a slab and is followed by a
// one-workgroup kernel that sums the slab in a fixed order and writes the scalars (pcg_* slots of `sc`).  No float
// atomics anywhere: a solve is bitwise reproducible run to run.  A q = matvec2 / matvec3 of residual.hip term for term
// (diagonal first, then the neighbours subtracted in the reference's order), so w equals what matvec would give for p'.
//
// Algorithmic bytes per interior point (FP64; operator planes read once, neighbour re-reads are cache hits):
//   pcg_direction   27-pt: 14 slots x 8 = 112 (row-interleaved copy: 15 x 8 = 120, slot 14 = 1/diag is not read)
//                          + z, p read 16 + p', w written 16                                   = 144 B (152 interleaved)
//                   7-pt: 4 x 8 + 32 = 64 B;   2D 9-pt: 5 x 8 + 32 = 72 B;   5-pt: 3 x 8 + 32 = 56 B
//                   first iteration (p' = z, p not read): 8 B less
//   pcg_update      x, r read and written 32 + p', w read 16                                    = 48 B
//                   precon = diag: + a_ii read 8 + z written 8                                  = 64 B
//   pcg_dots        (pcg_update without the update) r, z read                                   = 16 B
//   pcg_dots_wz     (flexible CG, cedar_amd_solver_fcg: the same dots and w.z) r, z, w read     = 24 B
#include "common.h"
#include "relax27_dev.h"
#include <algorithm>
#include <type_traits>

namespace cedar_amd {

namespace {

constexpr int RED_BS = 1024; // the one-workgroup second stage

// block-wide sum, fixed order (wave shuffles, then the waves in index order); valid in thread 0.  lds: BS / 64 doubles
template <int BS>
__device__ __forceinline__ real_t block_sum_k(real_t v, real_t *lds)
{
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
	const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
	if (l == 0) lds[w] = v;
	__syncthreads();
	real_t r = 0.0;
	if (threadIdx.x == 0)
		for (int t = 0; t < (int)(blockDim.x + 63) / 64; t++) r += lds[t];
	__syncthreads(); // lds may be reused by a second sum
	return r;
}

// matvec3's 27-point term order (residual.hip residual3_kernel<true, true>) on the row kernels' coefficient set
__device__ __forceinline__ real_t mv27(real_t d, const C27 &c, const real_t (&qq)[3][3][3])
{
	real_t s = d * qq[1][1][1];
	s = s - c.pw * qq[1][1][0];
	s = s - c.pnw_n * qq[1][2][0];
	s = s - c.ps_n * qq[1][2][1];
	s = s - c.psw_ne * qq[1][2][2];
	s = s - c.pw_e * qq[1][1][2];
	s = s - c.pnw_e * qq[1][0][2];
	s = s - c.ps * qq[1][0][1];
	s = s - c.psw * qq[1][0][0];
	s = s - c.b * qq[0][1][1];
	s = s - c.bw * qq[0][1][0];
	s = s - c.bnw_n * qq[0][2][0];
	s = s - c.bn_n * qq[0][2][1];
	s = s - c.bne_ne * qq[0][2][2];
	s = s - c.be_e * qq[0][1][2];
	s = s - c.bse_e * qq[0][0][2];
	s = s - c.bs * qq[0][0][1];
	s = s - c.bsw * qq[0][0][0];
	s = s - c.b_t * qq[2][1][1];
	s = s - c.be_t * qq[2][1][0];
	s = s - c.bse_nt * qq[2][2][0];
	s = s - c.bs_nt * qq[2][2][1];
	s = s - c.bsw_net * qq[2][2][2];
	s = s - c.bw_et * qq[2][1][2];
	s = s - c.bnw_et * qq[2][0][2];
	s = s - c.bn_t * qq[2][0][1];
	s = s - c.bne_t * qq[2][0][0];
	return s;
}

// ---------------------------------------------------------------- p' = z + beta p, w = A p', partial p'.w
// Where the 2D and 7-point bodies read z / p at the neighbours of point x = (i, j, k) -- the one thing in which a level
// with periodic directions (pcg_direction_periodic) differs.  There a neighbour index on the ghost layer of a periodic
// direction becomes the opposite interior end: 0 -> extent - 2, extent - 1 -> 1.  Only the ADDRESS of z / p changes --
// the expression z + beta p, the operator entries (read at the same places; their ghost layers hold the periodic image)
// and the term order are the same, so w has the bits of matvec2 / matvec3 on a vector whose ghosts were wrapped first.
// pd is uniform over the launch.  2D: k = 0, KK = 1 (B and T unused).
// Both policies have the same methods on a point q = (address, column): W / E give the neighbour in the row, again as a
// point, so that a 2D corner is S(W(q)); S / N / B / T give an address.  AdjPlain's are literally x - 1, x + 1, x -+ sj,
// x -+ sk; AdjPer's are row + wrapped column and wrapped row + column.  The bodies below write the stencil terms out
// where they are used: passed through a shared seven-term helper, pcg_dir7<first> needs two VGPRs more.
__device__ __forceinline__ int wrap_lo(int i, int n, int per) { return per && i == 0 ? n - 2 : i; }     // i - 1 of a point
__device__ __forceinline__ int wrap_hi(int i, int n, int per) { return per && i == n - 1 ? 1 : i; }     // i + 1 of a point

struct Pt {
	size_t x; // address
	int i;    // column
};

struct AdjPlain {
	size_t sj, sk;
	__device__ __forceinline__ AdjPlain(PerDirs, int, int, int II, int JJ, int) : sj(II), sk((size_t)II * JJ) {}
	__device__ __forceinline__ Pt W(Pt q) const { return Pt{q.x - 1, q.i - 1}; }
	__device__ __forceinline__ Pt E(Pt q) const { return Pt{q.x + 1, q.i + 1}; }
	__device__ __forceinline__ size_t S(Pt q) const { return q.x - sj; }
	__device__ __forceinline__ size_t N(Pt q) const { return q.x + sj; }
	__device__ __forceinline__ size_t B(Pt q) const { return q.x - sk; }
	__device__ __forceinline__ size_t T(Pt q) const { return q.x + sk; }
};

struct AdjPer {
	size_t row, rs, rn, rb, rt; // the row of the point and its four neighbour rows, wrapped (uniform over the workgroup)
	int II, px;
	__device__ __forceinline__ AdjPer(PerDirs pd, int j, int k, int II_, int JJ, int KK) : II(II_), px(pd.x)
	{
		const size_t sj = II, sk = (size_t)II * JJ;
		row = sj * (size_t)j + sk * (size_t)k;
		rs = sj * (size_t)wrap_lo(j - 1, JJ, pd.y) + sk * (size_t)k, rn = sj * (size_t)wrap_hi(j + 1, JJ, pd.y) + sk * (size_t)k;
		rb = sj * (size_t)j + sk * (size_t)wrap_lo(k - 1, KK, pd.z), rt = sj * (size_t)j + sk * (size_t)wrap_hi(k + 1, KK, pd.z);
	}
	__device__ __forceinline__ Pt at(int c) const { return Pt{row + (size_t)c, c}; }
	__device__ __forceinline__ Pt W(Pt q) const { return at(wrap_lo(q.i - 1, II, px)); }
	__device__ __forceinline__ Pt E(Pt q) const { return at(wrap_hi(q.i + 1, II, px)); }
	__device__ __forceinline__ size_t S(Pt q) const { return rs + (size_t)q.i; }
	__device__ __forceinline__ size_t N(Pt q) const { return rn + (size_t)q.i; }
	__device__ __forceinline__ size_t B(Pt q) const { return rb + (size_t)q.i; }
	__device__ __forceinline__ size_t T(Pt q) const { return rt + (size_t)q.i; }
};

// 2D: one lane per point, one workgroup per 256-point segment of a row (residual2_kernel's layout)
template <bool NINE, bool FIRST, class ADJ>
__device__ __forceinline__ void dir2_segment(const real_t *__restrict__ so, const real_t *__restrict__ z,
                                             const real_t *__restrict__ p, real_t *__restrict__ pn, real_t *__restrict__ w,
                                             const real_t *__restrict__ sc, int II, int JJ, PerDirs pd,
                                             real_t *__restrict__ part)
{
	__shared__ real_t lds[4];
	const int i = blockIdx.x * blockDim.x + threadIdx.x + 1;
	const int j = blockIdx.y + 1;
	const real_t beta = FIRST ? 0.0 : sc[PCG_BETA];
	real_t acc = 0.0;
	if (i <= II - 2) {
		const size_t sj = II, PS = (size_t)II * JJ;
		const ADJ a(pd, j, 0, II, JJ, 1);
		const size_t x = (size_t)i + sj * (size_t)j;
		auto P = [&](size_t y) -> real_t { return FIRST ? z[y] : z[y] + beta * p[y]; };
		const Pt q{x, i};
		const real_t pc = P(x);
		real_t s = so[KO * PS + x] * pc;
		s = s - so[KW * PS + x] * P(a.W(q).x);
		s = s - so[KW * PS + x + 1] * P(a.E(q).x);
		s = s - so[KS * PS + x] * P(a.S(q));
		s = s - so[KS * PS + x + sj] * P(a.N(q));
		if (NINE) {
			s = s - so[KSW * PS + x] * P(a.S(a.W(q)));
			s = s - so[KNW * PS + x + 1] * P(a.S(a.E(q)));
			s = s - so[KNW * PS + x + sj] * P(a.N(a.W(q)));
			s = s - so[KSW * PS + x + 1 + sj] * P(a.N(a.E(q)));
		}
		pn[x] = pc;
		w[x] = s;
		acc = pc * s;
	}
	const real_t t = block_sum_k<256>(acc, lds);
	if (threadIdx.x == 0) part[blockIdx.x + (size_t)gridDim.x * blockIdx.y] = t;
}

template <bool NINE, bool FIRST>
__global__ __launch_bounds__(256) void pcg_dir2(const real_t *__restrict__ so, const real_t *__restrict__ z,
                                                const real_t *__restrict__ p, real_t *__restrict__ pn,
                                                real_t *__restrict__ w, const real_t *__restrict__ sc, int II, int JJ,
                                                real_t *__restrict__ part)
{
	dir2_segment<NINE, FIRST, AdjPlain>(so, z, p, pn, w, sc, II, JJ, PerDirs{}, part);
}

template <bool NINE, bool FIRST>
__global__ __launch_bounds__(256) void pcg_dir2_per(const real_t *__restrict__ so, const real_t *__restrict__ z,
                                                    const real_t *__restrict__ p, real_t *__restrict__ pn,
                                                    real_t *__restrict__ w, const real_t *__restrict__ sc, int II, int JJ,
                                                    PerDirs pd, real_t *__restrict__ part)
{
	dir2_segment<NINE, FIRST, AdjPer>(so, z, p, pn, w, sc, II, JJ, pd, part);
}

// 3D 7-point: one workgroup per grid row (residual3_kernel's layout); partial of logical row L at part[L]
template <bool FIRST, class ADJ>
__device__ __forceinline__ void dir7_row(const real_t *__restrict__ so, const real_t *__restrict__ z,
                                         const real_t *__restrict__ p, real_t *__restrict__ pn, real_t *__restrict__ w,
                                         const real_t *__restrict__ sc, int II, int JJ, int KK, unsigned nrows, PerDirs pd,
                                         real_t *__restrict__ part)
{
	__shared__ real_t lds[4];
	const unsigned L = xcd_remap(blockIdx.x, nrows);
	if (L >= nrows) return; // grid padding of xcd_grid: no slab entry
	const int j = (int)(L % (unsigned)(JJ - 2)) + 1, k = (int)(L / (unsigned)(JJ - 2)) + 1;
	const size_t sj = II, sk = (size_t)II * JJ, PS = sk * KK;
	const ADJ a(pd, j, k, II, JJ, KK);
	const real_t beta = FIRST ? 0.0 : sc[PCG_BETA];
	auto P = [&](size_t y) -> real_t { return FIRST ? z[y] : z[y] + beta * p[y]; };
	real_t acc = 0.0;
	for (int i = threadIdx.x + 1; i <= II - 2; i += blockDim.x) {
		const size_t x = (size_t)i + sj * (size_t)j + sk * (size_t)k;
		const real_t pc = P(x);
		const Pt q{x, i};
		real_t s = so[KP * PS + x] * pc;
		s = s - so[KPW * PS + x] * P(a.W(q).x);
		s = s - so[KPS * PS + x + sj] * P(a.N(q));
		s = s - so[KPW * PS + x + 1] * P(a.E(q).x);
		s = s - so[KPS * PS + x] * P(a.S(q));
		s = s - so[KB * PS + x] * P(a.B(q));
		s = s - so[KB * PS + x + sk] * P(a.T(q));
		pn[x] = pc;
		w[x] = s;
		acc += pc * s;
	}
	const real_t t = block_sum_k<256>(acc, lds);
	if (threadIdx.x == 0) part[L] = t;
}

template <bool FIRST>
__global__ __launch_bounds__(256) void pcg_dir7(const real_t *__restrict__ so, const real_t *__restrict__ z,
                                                const real_t *__restrict__ p, real_t *__restrict__ pn,
                                                real_t *__restrict__ w, const real_t *__restrict__ sc, int II, int JJ,
                                                int KK, unsigned nrows, real_t *__restrict__ part)
{
	dir7_row<FIRST, AdjPlain>(so, z, p, pn, w, sc, II, JJ, KK, nrows, PerDirs{}, part);
}

template <bool FIRST>
__global__ __launch_bounds__(256) void pcg_dir7_per(const real_t *__restrict__ so, const real_t *__restrict__ z,
                                                    const real_t *__restrict__ p, real_t *__restrict__ pn,
                                                    real_t *__restrict__ w, const real_t *__restrict__ sc, int II, int JJ,
                                                    int KK, unsigned nrows, PerDirs pd, real_t *__restrict__ part)
{
	dir7_row<FIRST, AdjPer>(so, z, p, pn, w, sc, II, JJ, KK, nrows, pd, part);
}

// The end of a 27-point task: w = A p' at the even and the odd point of the pair (mv27 on the finished windows), their
// share of p'.w added to acc, and w and p' stored at off + row + ie (off: the item's offset; 16-byte stores, or a row's
// last half pair).  Used by pcg_dir27, pcg_dir27_many and pcg_dir27_per_many, which compile to the code they had with the
// text in place.  pcg_dir27_per keeps its own copy: with this call the allocator, at 256 VGPRs, spills four VGPRs more.
__device__ __forceinline__ void dir27_emit(real_t de, real_t dn, const C27 &ce, const C27 &co, const real_t (&qe)[3][3][3],
                                           const real_t (&qo)[3][3][3], bool o_ok, real_t *__restrict__ w,
                                           real_t *__restrict__ pn, size_t off, size_t row, int ie, real_t &acc)
{
	const real_t we = mv27(de, ce, qe);
	const real_t pe = qe[1][1][1];
	acc += pe * we;
	if (o_ok) {
		const real_t wo = mv27(dn, co, qo);
		const real_t po = qo[1][1][1];
		acc += po * wo;
		d2u v; v.x = we; v.y = wo;
		*reinterpret_cast<d2u *>(w + off + row + ie) = v;
		v.x = pe; v.y = po;
		*reinterpret_cast<d2u *>(pn + off + row + ie) = v;
	} else {
		w[off + row + ie] = we;
		pn[off + row + ie] = pe;
	}
}

// 3D 27-point: residual27_rows' layout -- lane p owns the pair (2p+1, 2p+2) of its row, 16-byte loads and stores,
// rows walked in (j,k) tiles; the operator through an Op3 view (Cedar planes or the solver's row-interleaved copy)
template <int BS, bool FIRST>
__global__ __launch_bounds__(BS) __attribute__((amdgpu_waves_per_eu(2))) void pcg_dir27(const Op3 A, const real_t *__restrict__ z, const real_t *__restrict__ p,
                                                real_t *__restrict__ pn, real_t *__restrict__ w,
                                                const real_t *__restrict__ sc, int II, int JJ, int KK, unsigned nblk,
                                                TileShape ts, real_t *__restrict__ part)
{
	__shared__ real_t lds[(BS + 63) / 64];
	const unsigned L = xcd_remap(blockIdx.x, nblk);
	if (L >= nblk) return; // grid padding: no slab entry
	unsigned jr, kr;
	real_t acc = 0.0;
	if (tile_rows(L, (unsigned)(JJ - 2), (unsigned)(KK - 2), ts, jr, kr)) {
		const real_t beta = FIRST ? 0.0 : sc[PCG_BETA];
		const size_t j = (size_t)jr + 1, k = (size_t)kr + 1;
		const size_t sj = (size_t)II, sk = (size_t)II * JJ;
		const size_t row = j * sj + k * sk, rowA = j * A.SJ + k * A.SK;
		for (int q = threadIdx.x; 2 * q + 1 <= II - 2; q += BS) {
			const int ie = 2 * q + 1, io = 2 * q + 2;
			const bool o_ok = io <= II - 2, two = io + 1 <= II - 1;
			C27 ce, co;
			real_t qe[3][3][3], qo[3][3][3], zfe, zfo, de, dn;
			// operator coefficients and the 3x3 windows of p (FIRST: of z); qf = z (own pair, a cache hit below)
			load_pair27<false, false, false>(A, z, FIRST ? z : p, rowA, row, sj, sk, ie, io, two, ce, co, qe, qo, zfe, zfo);
			ldpair(A.so + rowA + ie, true, de, dn); // KP plane
			if (!FIRST) {
#pragma unroll
				for (int dk = 0; dk < 3; dk++)
#pragma unroll
					for (int dj = 0; dj < 3; dj++) {
						const real_t *r = z + row + (ptrdiff_t)(dj - 1) * (ptrdiff_t)sj + (ptrdiff_t)(dk - 1) * (ptrdiff_t)sk;
						real_t w0, w1, w2, w3;
						ldpair(r + ie - 1, true, w0, w1);
						ldpair(r + io, two, w2, w3);
						qe[dk][dj][0] = w0 + beta * qe[dk][dj][0];
						qe[dk][dj][1] = w1 + beta * qe[dk][dj][1];
						qe[dk][dj][2] = w2 + beta * qe[dk][dj][2];
						qo[dk][dj][0] = qe[dk][dj][1];
						qo[dk][dj][1] = qe[dk][dj][2];
						qo[dk][dj][2] = w3 + beta * qo[dk][dj][2];
					}
			}
			dir27_emit(de, dn, ce, co, qe, qo, o_ok, w, pn, 0, row, ie, acc);
		}
	}
	const real_t t = block_sum_k<BS>(acc, lds);
	if (threadIdx.x == 0) part[L] = t;
}

// pcg_dir27 on a level with periodic directions.  Wrapping j and k changes the row pointer of a window row (uniform over
// the workgroup).  Wrapping i concerns two elements of a row's windows only: the left element of the lane that owns point 1
// and the right element of the lane that owns the last point (an odd nx ends in a half pair: its right neighbour, the
// element ldpair read at io, is the wrap) -- those are replaced by z + beta p at the wrapped address after the pair loads,
// so nothing formed from a ghost value reaches w, pn or the sum.  The coefficients: load_coef27 on the Cedar planes, as
// pcg_dir27 (a periodic level has no row-interleaved copy).  The tail is dir27_emit's text (see there).
template <int BS, bool FIRST>
__global__ __launch_bounds__(BS) __attribute__((amdgpu_waves_per_eu(2))) void pcg_dir27_per(
    const Op3 A, const real_t *__restrict__ z, const real_t *__restrict__ p, real_t *__restrict__ pn, real_t *__restrict__ w,
    const real_t *__restrict__ sc, int II, int JJ, int KK, unsigned nblk, TileShape ts, PerDirs pd, real_t *__restrict__ part)
{
	__shared__ real_t lds[(BS + 63) / 64];
	const unsigned L = xcd_remap(blockIdx.x, nblk);
	if (L >= nblk) return; // grid padding: no slab entry
	unsigned jr, kr;
	real_t acc = 0.0;
	if (tile_rows(L, (unsigned)(JJ - 2), (unsigned)(KK - 2), ts, jr, kr)) {
		const real_t beta = FIRST ? 0.0 : sc[PCG_BETA];
		const int j = (int)jr + 1, k = (int)kr + 1;
		const size_t sj = (size_t)II, sk = (size_t)II * JJ;
		const size_t row = (size_t)j * sj + (size_t)k * sk, rowA = (size_t)j * A.SJ + (size_t)k * A.SK;
		// the window rows (j-1, j, j+1) x (k-1, k, k+1), wrapped
		const size_t oj[3] = {sj * (size_t)wrap_lo(j - 1, JJ, pd.y), sj * (size_t)j, sj * (size_t)wrap_hi(j + 1, JJ, pd.y)};
		const size_t ok[3] = {sk * (size_t)wrap_lo(k - 1, KK, pd.z), sk * (size_t)k, sk * (size_t)wrap_hi(k + 1, KK, pd.z)};
		for (int q = threadIdx.x; 2 * q + 1 <= II - 2; q += BS) {
			const int ie = 2 * q + 1, io = 2 * q + 2;
			const bool o_ok = io <= II - 2, two = io + 1 <= II - 1;
			C27 ce, co;
			real_t qe[3][3][3], qo[3][3][3], de, dn;
			load_coef27<false, false, false>(A, rowA, ie, io, two, ce, co);
			ldpair(A.so + rowA + ie, true, de, dn); // KP plane
			// the nine window rows as pcg_dir27 loads them (every load of the task issued before any patch below)
#pragma unroll
			for (int dk = 0; dk < 3; dk++)
#pragma unroll
				for (int dj = 0; dj < 3; dj++) {
					const size_t y = oj[dj] + ok[dk];
					real_t w0, w1, w2, w3;
					ldpair(z + y + ie - 1, true, w0, w1);
					ldpair(z + y + io, two, w2, w3);
					if (!FIRST) {
						real_t p0, p1, p2, p3;
						ldpair(p + y + ie - 1, true, p0, p1);
						ldpair(p + y + io, two, p2, p3);
						w0 = w0 + beta * p0;
						w1 = w1 + beta * p1;
						w2 = w2 + beta * p2;
						w3 = w3 + beta * p3;
					}
					qe[dk][dj][0] = w0; qe[dk][dj][1] = w1; qe[dk][dj][2] = w2;
					qo[dk][dj][0] = w1; qo[dk][dj][1] = w2; qo[dk][dj][2] = w3;
				}
			// periodic x (uniform branch): the window elements formed from a ghost of the row -- index 0 in the lane of point
			// 1; index II - 1 in the lane of the last point, its w3, or its w2 when the row ends in a half pair -- are
			// replaced by the same expression at the wrapped address, so what was formed from the ghost is dropped unused
			if (pd.x) {
				auto P = [&](size_t y) -> real_t { return FIRST ? z[y] : z[y] + beta * p[y]; };
				if (ie == 1) {
#pragma unroll
					for (int dk = 0; dk < 3; dk++)
#pragma unroll
						for (int dj = 0; dj < 3; dj++) qe[dk][dj][0] = P(oj[dj] + ok[dk] + II - 2);
				}
				if (io + 1 >= II - 1) {
#pragma unroll
					for (int dk = 0; dk < 3; dk++)
#pragma unroll
						for (int dj = 0; dj < 3; dj++) {
							const real_t v = P(oj[dj] + ok[dk] + 1);
							if (two) qo[dk][dj][2] = v;
							else qe[dk][dj][2] = v;
						}
				}
			}
			const real_t we = mv27(de, ce, qe);
			const real_t pe = qe[1][1][1];
			acc += pe * we;
			if (o_ok) {
				const real_t wo = mv27(dn, co, qo);
				const real_t po = qo[1][1][1];
				acc += po * wo;
				d2u v; v.x = we; v.y = wo;
				*reinterpret_cast<d2u *>(w + row + ie) = v;
				v.x = pe; v.y = po;
				*reinterpret_cast<d2u *>(pn + row + ie) = v;
			} else {
				w[row + ie] = we;
				pn[row + ie] = pe;
			}
		}
	}
	const real_t t = block_sum_k<BS>(acc, lds);
	if (threadIdx.x == 0) part[L] = t;
}

// ---------------------------------------------------------------- x / r update and the dots
// ZM (what z is): 0 = r itself (no preconditioner), 1 = r / a_ii written here (diagonal), 2 = read (multigrid, after
// the preconditioner), 3 = not involved (multigrid, before it: r.r only).  MOVE: x += alpha p', r -= alpha w first.
// Rows dealt to a fixed number of workgroups in a fixed pattern; lane q owns the pair (2q+1, 2q+2) of a row.
template <int ZM, bool MOVE>
__global__ __launch_bounds__(256) void pcg_upd(real_t *__restrict__ x, real_t *__restrict__ r,
                                               const real_t *__restrict__ p, const real_t *__restrict__ w,
                                               real_t *__restrict__ z, const real_t *__restrict__ diag,
                                               const real_t *__restrict__ sc, int II, int JJ, int KK,
                                               real_t *__restrict__ part)
{
	__shared__ real_t lds[4];
	const int nj = JJ - 2, nk = KK == 1 ? 1 : KK - 2;
	const size_t nrows = (size_t)nj * nk;
	const real_t a = MOVE ? sc[PCG_ALPHA] : 0.0;
	const bool mv = MOVE && a != 0.0; // alpha = 0 (breakdown): x and r stay as they are
	real_t rr = 0.0, rz = 0.0;
	for (size_t t = blockIdx.x; t < nrows; t += gridDim.x) {
		const size_t j = t % nj + 1, k = KK == 1 ? 0 : t / nj + 1;
		const size_t row = (size_t)II * (j + (size_t)JJ * k);
		for (int q = threadIdx.x; 2 * q + 1 <= II - 2; q += blockDim.x) {
			const size_t ie = row + 2 * q + 1;
			const bool two = 2 * q + 2 <= II - 2;
			real_t r0, r1;
			ldpair(r + ie, two, r0, r1);
			if (mv) {
				real_t x0, x1, p0, p1, w0, w1;
				ldpair(x + ie, two, x0, x1);
				ldpair(p + ie, two, p0, p1);
				ldpair(w + ie, two, w0, w1);
				x0 = x0 + a * p0; x1 = x1 + a * p1;
				r0 = r0 - a * w0; r1 = r1 - a * w1;
				if (two) {
					d2u v; v.x = x0; v.y = x1; *reinterpret_cast<d2u *>(x + ie) = v;
					v.x = r0; v.y = r1; *reinterpret_cast<d2u *>(r + ie) = v;
				} else {
					x[ie] = x0; r[ie] = r0;
				}
			}
			rr += r0 * r0;
			if (two) rr += r1 * r1;
			if (ZM == 1) {
				real_t d0, d1;
				ldpair(diag + ie, two, d0, d1);
				const real_t z0 = r0 / d0, z1 = two ? r1 / d1 : 0.0;
				if (two) { d2u v; v.x = z0; v.y = z1; *reinterpret_cast<d2u *>(z + ie) = v; }
				else z[ie] = z0;
				rz += r0 * z0;
				if (two) rz += r1 * z1;
			} else if (ZM == 2) {
				real_t z0, z1;
				ldpair(z + ie, two, z0, z1);
				rz += r0 * z0;
				if (two) rz += r1 * z1;
			}
		}
	}
	const real_t s0 = block_sum_k<256>(rr, lds);
	const real_t s1 = (ZM == 1 || ZM == 2) ? block_sum_k<256>(rz, lds) : 0.0;
	if (threadIdx.x == 0) {
		part[blockIdx.x] = s0;
		part[gridDim.x + blockIdx.x] = s1;
	}
}

// The dots of flexible CG after the preconditioner: pcg_upd<2, false> (same row dealing, pair loop and sums, so r.r and
// r.z have its bits) that also reads w = A p, still in its buffer, for w.z -- a third slab section.  Nothing is written
// but the slab.
__global__ __launch_bounds__(256) void pcg_dwz(const real_t *__restrict__ r, const real_t *__restrict__ z,
                                               const real_t *__restrict__ w, int II, int JJ, int KK,
                                               real_t *__restrict__ part)
{
	__shared__ real_t lds[4];
	const int nj = JJ - 2, nk = KK == 1 ? 1 : KK - 2;
	const size_t nrows = (size_t)nj * nk;
	real_t rr = 0.0, rz = 0.0, wz = 0.0;
	for (size_t t = blockIdx.x; t < nrows; t += gridDim.x) {
		const size_t j = t % nj + 1, k = KK == 1 ? 0 : t / nj + 1;
		const size_t row = (size_t)II * (j + (size_t)JJ * k);
		for (int q = threadIdx.x; 2 * q + 1 <= II - 2; q += blockDim.x) {
			const size_t ie = row + 2 * q + 1;
			const bool two = 2 * q + 2 <= II - 2;
			real_t r0, r1, z0, z1, w0, w1;
			ldpair(r + ie, two, r0, r1);
			ldpair(z + ie, two, z0, z1);
			ldpair(w + ie, two, w0, w1);
			rr += r0 * r0;
			if (two) rr += r1 * r1;
			rz += r0 * z0;
			if (two) rz += r1 * z1;
			wz += w0 * z0;
			if (two) wz += w1 * z1;
		}
	}
	const real_t s0 = block_sum_k<256>(rr, lds);
	const real_t s1 = block_sum_k<256>(rz, lds);
	const real_t s2 = block_sum_k<256>(wz, lds);
	if (threadIdx.x == 0) {
		part[blockIdx.x] = s0;
		part[gridDim.x + blockIdx.x] = s1;
		part[2 * gridDim.x + blockIdx.x] = s2;
	}
}

// ---------------------------------------------------------------- second stages (one workgroup)
__device__ __forceinline__ real_t slab_sum(const real_t *__restrict__ part, unsigned n, real_t *lds)
{
	real_t acc = 0.0;
	for (unsigned i = threadIdx.x; i < n; i += RED_BS) acc += part[i];
	return block_sum_k<RED_BS>(acc, lds);
}

// the scalars of a second stage, thread 0 only: sigma -> alpha (0 with the breakdown flag when sigma <= 0 or not
// finite, or rho = 0); r.r / r.z -> rho, beta (first: 0)
__device__ __forceinline__ void set_alpha(real_t sigma, real_t *__restrict__ sc)
{
	const real_t rho = sc[PCG_RHO];
	const bool ok = sigma > 0.0 && sigma <= 1.7976931348623157e308 && rho != 0.0;
	sc[PCG_SIGMA] = sigma;
	sc[PCG_ALPHA] = ok ? rho / sigma : 0.0;
	if (!ok) sc[PCG_FLAG] = 1.0;
}

__device__ __forceinline__ void set_rho(real_t rr, real_t rz, int has_rz, int first, real_t *__restrict__ sc)
{
	sc[PCG_RR] = rr;
	if (has_rz) {
		const real_t rho = sc[PCG_RHO];
		sc[PCG_RZ] = rz;
		sc[PCG_BETA] = first || rho == 0.0 ? 0.0 : rz / rho;
		sc[PCG_RHO] = rz;
	}
}

// sigma = sum of the slab, then alpha
__global__ __launch_bounds__(RED_BS) void pcg_alpha(const real_t *__restrict__ part, unsigned n, real_t *__restrict__ sc)
{
	__shared__ real_t lds[RED_BS / 64];
	const real_t sigma = slab_sum(part, n, lds);
	if (threadIdx.x == 0) set_alpha(sigma, sc);
}

// r.r (slab 0) and, when has_rz, r.z (slab 1; zm0: r.z = r.r): the new rho, beta = rho_new / rho_old (first: 0)
__global__ __launch_bounds__(RED_BS) void pcg_rho(const real_t *__restrict__ part, unsigned n, int has_rz, int first,
                                                  real_t *__restrict__ sc)
{
	__shared__ real_t lds[RED_BS / 64];
	const real_t rr = slab_sum(part, n, lds);
	const real_t rz = has_rz == 1 ? slab_sum(part + n, n, lds) : rr;
	if (threadIdx.x == 0) set_rho(rr, rz, has_rz, first, sc);
}

// flexible CG (Polak-Ribiere beta): with r_k - r_k+1 = alpha w, beta = z_k+1.(r_k+1 - r_k) / rho_k = -(alpha w.z) / rho_k;
// two roundings, then an exact negation.  alpha, sigma and the flag stay as the direction pass left them.
__device__ __forceinline__ void set_rho_flex(real_t rr, real_t rz, real_t wz, int first, real_t *__restrict__ sc)
{
	const real_t rho = sc[PCG_RHO], alpha = sc[PCG_ALPHA];
	sc[PCG_RR] = rr;
	sc[PCG_RZ] = rz;
	sc[PCG_WZ] = wz;
	sc[PCG_BETA] = first || rho == 0.0 ? 0.0 : -((alpha * wz) / rho);
	sc[PCG_RHO] = rz;
}

// r.r (slab 0), r.z (slab 1), w.z (slab 2) of pcg_dwz: the new rho and the flexible beta
__global__ __launch_bounds__(RED_BS) void pcg_rho_flex(const real_t *__restrict__ part, unsigned n, int first,
                                                       real_t *__restrict__ sc)
{
	__shared__ real_t lds[RED_BS / 64];
	const real_t rr = slab_sum(part, n, lds);
	const real_t rz = slab_sum(part + n, n, lds);
	const real_t wz = slab_sum(part + 2 * (size_t)n, n, lds);
	if (threadIdx.x == 0) set_rho_flex(rr, rz, wz, first, sc);
}

// ---------------------------------------------------------------- the same second stages on a rank grid
// (a) this rank's slab sums (the sums pcg_alpha / pcg_rho form, same order) into out[0 .. nslab-1], the send buffer of
// the all-gather; (b) after it, one thread sums the world ranks' partials (stride doubles per rank) in rank order and
// sets the scalars as the one-rank stages do.  world = 1: (b) takes the partial as it is, the one-rank values bit for bit.
__global__ __launch_bounds__(RED_BS) void pcg_partial(const real_t *__restrict__ part, unsigned n, int nslab,
                                                      real_t *__restrict__ out)
{
	__shared__ real_t lds[RED_BS / 64];
	for (int t = 0; t < nslab; t++) {
		const real_t v = slab_sum(part + (size_t)t * n, n, lds);
		if (threadIdx.x == 0) out[t] = v;
	}
}

__device__ __forceinline__ real_t rank_sum(const real_t *__restrict__ g, int world, int stride, int t)
{
	real_t v = g[t];
	for (int r = 1; r < world; r++) v += g[(size_t)r * stride + t];
	return v;
}

__global__ void pcg_alpha_ranks(const real_t *__restrict__ g, int world, int stride, real_t *__restrict__ sc)
{
	if (threadIdx.x == 0) set_alpha(rank_sum(g, world, stride, 0), sc);
}

__global__ void pcg_rho_ranks(const real_t *__restrict__ g, int world, int stride, int has_rz, int first,
                              real_t *__restrict__ sc)
{
	if (threadIdx.x != 0) return;
	const real_t rr = rank_sum(g, world, stride, 0);
	set_rho(rr, has_rz == 1 ? rank_sum(g, world, stride, 1) : rr, has_rz, first, sc);
}

// ---------------------------------------------------------------- p' = z + beta p on the ghost shell of a rank box
// The ghost cells a neighbouring rank owns (boxes of the halo's receive side, without the physical-boundary ghosts): the
// value that neighbour's pcg_direction forms for its own point (same expression, same beta on every rank, no FMA
// contraction in this build), so the next direction pass finds p current at its stencil neighbours without an exchange.
template <bool FIRST>
__global__ __launch_bounds__(256) void pcg_shell(const real_t *__restrict__ z, const real_t *__restrict__ p,
                                                 real_t *__restrict__ pn, const real_t *__restrict__ sc, ShellBoxes bx,
                                                 int II, int JJ)
{
	const int b = blockIdx.y;
	const int *B = bx.box + 6 * b;
	const size_t cnt = (size_t)B[3] * B[4] * B[5];
	const real_t beta = FIRST ? 0.0 : sc[PCG_BETA];
	for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < cnt; t += (size_t)gridDim.x * blockDim.x) {
		const size_t i = B[0] + t % B[3], j = B[1] + (t / B[3]) % B[4], k = B[2] + t / ((size_t)B[3] * B[4]);
		const size_t y = i + (size_t)II * (j + (size_t)JJ * k);
		pn[y] = FIRST ? z[y] : z[y] + beta * p[y];
	}
}

constexpr unsigned UPD_NB = 2048;

// ================================================================ the same passes on a batch of right-hand sides
// (solver.cpp cedar_amd_solver_pcg_many): nrhs independent CG recurrences on ONE operator.  Vectors are item-major with
// the stride of common.h Batch; item m has its own scalar block sc + m * PCG_NSC and its own slab part + m * n (n = the
// single pass' partial count).  Each pass keeps the single pass' geometry per item -- same workgroup width, same tile
// walk, same row dealing, block_sum_k per item, slab_sum per item -- and the build has no FMA contraction, so every
// vector AND every scalar of item m has the bits the single-vector pass gives on item m alone.  What a batch saves is
// the operator: a workgroup task fetches its coefficients once and applies them to every item from registers.
// `active`: bit m clear = item m is skipped by the vector pass and by its second stage (nothing of it is read or
// written); a kernel argument, so that freezing an item costs no copy.
//
// Algorithmic bytes per interior point for n items:
//   pcg_dir27_many  operator once 112 (interleaved copy 120) + n x (z, p read 16 + p', w written 16)  = 120 + 32 n
//   pcg_dir7_many   4 x 8 + 32 n;   pcg_dir2_many  as pcg_dir2 per item (the item comes from the launch grid)
//   pcg_dir2_per_many (periodic 2D levels: the items walked inside the workgroup)  5 x 8 (five-point: 3 x 8) + 32 n
//   pcg_upd_many    48 n; precon = diag: 8 + 56 n
constexpr int ITEM_CHUNK = 8; // items of one workgroup of pcg_dir7_many / pcg_upd_many (their per-lane sums live in LDS)

__device__ __forceinline__ bool item_on(unsigned active, int m) { return (active >> m) & 1u; }

// 2D: pcg_dir2 with the item in blockIdx.z (no operator reuse, as the 2D kernels of a batched cycle)
template <bool NINE, bool FIRST>
__global__ __launch_bounds__(256) void pcg_dir2_many(const real_t *__restrict__ so, const real_t *__restrict__ z,
                                                     const real_t *__restrict__ p, real_t *__restrict__ pn,
                                                     real_t *__restrict__ w, const real_t *__restrict__ sc, int II, int JJ,
                                                     real_t *__restrict__ part, size_t stride, unsigned active)
{
	const int m = blockIdx.z;
	if (!item_on(active, m)) return;
	const size_t off = (size_t)m * stride;
	dir2_segment<NINE, FIRST, AdjPlain>(so, z + off, FIRST ? z : p + off, pn + off, w + off, sc + (size_t)m * PCG_NSC, II, JJ,
	                                    PerDirs{}, part + (size_t)m * gridDim.x * gridDim.y);
}

// 2D on a level with periodic directions (cedar_amd_solver_fcg_periodic_many on a 2D handle): dir2_segment's task -- one
// lane per point, one workgroup per 256-point segment of a row -- with all items walked inside it: the point's five or
// nine operator entries and its (wrapped) neighbour addresses are formed once and applied to every active item, whose
// sum is taken by block_sum_k as dir2_segment takes it.  Item m's pn, w and slab have the bits of pcg_direction_periodic
// on item m alone; a masked item is neither read nor written.
template <bool NINE, bool FIRST, class ADJ>
__device__ __forceinline__ void dir2_items(const real_t *__restrict__ so, const real_t *__restrict__ z,
                                           const real_t *__restrict__ p, real_t *__restrict__ pn, real_t *__restrict__ w,
                                           const real_t *__restrict__ sc, int II, int JJ, PerDirs pd, real_t *__restrict__ part,
                                           int nrhs, size_t stride, unsigned active)
{
	__shared__ real_t lds[4];
	const int i = blockIdx.x * blockDim.x + threadIdx.x + 1;
	const int j = blockIdx.y + 1;
	const bool on = i <= II - 2;
	const size_t sj = II, PS = (size_t)II * JJ;
	const size_t n = (size_t)gridDim.x * gridDim.y; // slab entries of one item
	const ADJ a(pd, j, 0, II, JJ, 1);
	const int ic = on ? i : 1; // (a lane past the row forms the addresses of the first point and uses none)
	const size_t x = (size_t)ic + sj * (size_t)j;
	const Pt q{x, ic};
	const size_t xw = a.W(q).x, xe = a.E(q).x, xs = a.S(q), xn = a.N(q);
	const size_t xsw = NINE ? a.S(a.W(q)) : x, xse = NINE ? a.S(a.E(q)) : x, xnw = NINE ? a.N(a.W(q)) : x, xne = NINE ? a.N(a.E(q)) : x;
	real_t co = 0, cw = 0, ce = 0, cs = 0, cn = 0, csw = 0, cse = 0, cnw = 0, cne = 0;
	if (on) {
		co = so[KO * PS + x], cw = so[KW * PS + x], ce = so[KW * PS + x + 1], cs = so[KS * PS + x], cn = so[KS * PS + x + sj];
		if (NINE) csw = so[KSW * PS + x], cse = so[KNW * PS + x + 1], cnw = so[KNW * PS + x + sj], cne = so[KSW * PS + x + 1 + sj];
	}
#pragma unroll 1
	for (int m = 0; m < nrhs; m++) {
		if (!item_on(active, m)) continue; // uniform over the workgroup
		const size_t off = (size_t)m * stride;
		const real_t *__restrict__ zm = z + off, *__restrict__ pm = FIRST ? zm : p + off;
		const real_t beta = FIRST ? 0.0 : sc[(size_t)m * PCG_NSC + PCG_BETA];
		auto P = [&](size_t y) -> real_t { return FIRST ? zm[y] : zm[y] + beta * pm[y]; };
		real_t acc = 0.0;
		if (on) {
			const real_t pc = P(x);
			real_t s = co * pc;
			s = s - cw * P(xw);
			s = s - ce * P(xe);
			s = s - cs * P(xs);
			s = s - cn * P(xn);
			if (NINE) {
				s = s - csw * P(xsw);
				s = s - cse * P(xse);
				s = s - cnw * P(xnw);
				s = s - cne * P(xne);
			}
			pn[off + x] = pc;
			w[off + x] = s;
			acc = pc * s;
		}
		const real_t t = block_sum_k<256>(acc, lds);
		if (threadIdx.x == 0) part[(size_t)m * n + blockIdx.x + (size_t)gridDim.x * blockIdx.y] = t;
	}
}

template <bool NINE, bool FIRST>
__global__ __launch_bounds__(256) void pcg_dir2_per_many(const real_t *__restrict__ so, const real_t *__restrict__ z,
                                                         const real_t *__restrict__ p, real_t *__restrict__ pn,
                                                         real_t *__restrict__ w, const real_t *__restrict__ sc, int II, int JJ,
                                                         PerDirs pd, real_t *__restrict__ part, int nrhs, size_t stride,
                                                         unsigned active)
{
	dir2_items<NINE, FIRST, AdjPer>(so, z, p, pn, w, sc, II, JJ, pd, part, nrhs, stride, active);
}

// 3D 7-point: dir7_row with the seven operator entries a point reads in registers across the items m0 .. m0 + nitems-1
// (m0 = ITEM_CHUNK * blockIdx.y).  A lane's sum runs over the trips of a row longer than the workgroup, per item: one
// LDS column per lane (accl[item][lane], lane-private, so no barrier), summed per item exactly as dir7_row sums acc.
// With AdjPer: the direction pass of a periodic level on a batch (cedar_amd_solver_fcg_periodic_many); item m's pn, w and
// slab have the bits of pcg_direction_periodic on item m alone.
template <bool FIRST, class ADJ>
__device__ __forceinline__ void dir7_items(const real_t *__restrict__ so, const real_t *__restrict__ z,
                                           const real_t *__restrict__ p, real_t *__restrict__ pn, real_t *__restrict__ w,
                                           const real_t *__restrict__ sc, int II, int JJ, int KK, unsigned nrows, PerDirs pd,
                                           real_t *__restrict__ part, int nrhs, size_t stride, unsigned active)
{
	__shared__ real_t lds[4];
	__shared__ real_t accl[ITEM_CHUNK][256];
	const unsigned L = xcd_remap(blockIdx.x, nrows);
	if (L >= nrows) return; // grid padding of xcd_grid: no slab entry
	const int m0 = ITEM_CHUNK * (int)blockIdx.y, nitems = min(ITEM_CHUNK, nrhs - m0);
	const int j = (int)(L % (unsigned)(JJ - 2)) + 1, k = (int)(L / (unsigned)(JJ - 2)) + 1;
	const size_t sj = II, sk = (size_t)II * JJ, PS = sk * KK;
	const ADJ a(pd, j, k, II, JJ, KK);
	for (int t = 0; t < nitems; t++) accl[t][threadIdx.x] = 0.0;
	for (int i = threadIdx.x + 1; i <= II - 2; i += blockDim.x) {
		const size_t x = (size_t)i + sj * (size_t)j + sk * (size_t)k;
		const Pt q{x, i};
		const real_t cp = so[KP * PS + x], cw = so[KPW * PS + x], cn = so[KPS * PS + x + sj], ce = so[KPW * PS + x + 1];
		const real_t cs = so[KPS * PS + x], cb = so[KB * PS + x], ct = so[KB * PS + x + sk];
#pragma unroll 1
		for (int t = 0; t < nitems; t++) {
			const int m = m0 + t;
			if (!item_on(active, m)) continue;
			const size_t off = (size_t)m * stride;
			const real_t *__restrict__ zm = z + off, *__restrict__ pm = FIRST ? zm : p + off;
			const real_t beta = FIRST ? 0.0 : sc[(size_t)m * PCG_NSC + PCG_BETA];
			auto P = [&](size_t y) -> real_t { return FIRST ? zm[y] : zm[y] + beta * pm[y]; };
			const real_t pc = P(x);
			real_t s = cp * pc;
			s = s - cw * P(a.W(q).x);
			s = s - cn * P(a.N(q));
			s = s - ce * P(a.E(q).x);
			s = s - cs * P(a.S(q));
			s = s - cb * P(a.B(q));
			s = s - ct * P(a.T(q));
			pn[off + x] = pc;
			w[off + x] = s;
			accl[t][threadIdx.x] += pc * s;
		}
	}
	for (int t = 0; t < nitems; t++) {
		const int m = m0 + t;
		if (!item_on(active, m)) continue; // uniform over the workgroup
		const real_t v = block_sum_k<256>(accl[t][threadIdx.x], lds);
		if (threadIdx.x == 0) part[(size_t)m * nrows + L] = v;
	}
}

template <bool FIRST>
__global__ __launch_bounds__(256) void pcg_dir7_many(const real_t *__restrict__ so, const real_t *__restrict__ z,
                                                     const real_t *__restrict__ p, real_t *__restrict__ pn,
                                                     real_t *__restrict__ w, const real_t *__restrict__ sc, int II, int JJ,
                                                     int KK, unsigned nrows, real_t *__restrict__ part, int nrhs,
                                                     size_t stride, unsigned active)
{
	dir7_items<FIRST, AdjPlain>(so, z, p, pn, w, sc, II, JJ, KK, nrows, PerDirs{}, part, nrhs, stride, active);
}

template <bool FIRST>
__global__ __launch_bounds__(256) void pcg_dir7_per_many(const real_t *__restrict__ so, const real_t *__restrict__ z,
                                                         const real_t *__restrict__ p, real_t *__restrict__ pn,
                                                         real_t *__restrict__ w, const real_t *__restrict__ sc, int II, int JJ,
                                                         int KK, unsigned nrows, PerDirs pd, real_t *__restrict__ part, int nrhs,
                                                         size_t stride, unsigned active)
{
	dir7_items<FIRST, AdjPer>(so, z, p, pn, w, sc, II, JJ, KK, nrows, pd, part, nrhs, stride, active);
}

// 3D 27-point: pcg_dir27 for rows of one trip (at most 2 BS points; longer rows go through pcg_dir27 item by item, see
// pcg_direction_many), so that a lane's sum of an item is one register and not a run-time indexed array.  The 52
// coefficients and the diagonal pair stay in registers across the item loop; one window set is live at a time.
template <int BS, bool FIRST>
__global__ __launch_bounds__(BS) __attribute__((amdgpu_waves_per_eu(2))) void pcg_dir27_many(
    const Op3 A, const real_t *__restrict__ z, const real_t *__restrict__ p, real_t *__restrict__ pn, real_t *__restrict__ w,
    const real_t *__restrict__ sc, int II, int JJ, int KK, unsigned nblk, TileShape ts, real_t *__restrict__ part, int nrhs,
    size_t stride, unsigned active)
{
	__shared__ real_t lds[(BS + 63) / 64];
	const unsigned L = xcd_remap(blockIdx.x, nblk);
	if (L >= nblk) return; // grid padding: no slab entry
	unsigned jr, kr;
	const bool have = tile_rows(L, (unsigned)(JJ - 2), (unsigned)(KK - 2), ts, jr, kr);
	const int q = threadIdx.x;
	const bool mine = have && 2 * q + 1 <= II - 2;
	const int ie = 2 * q + 1, io = 2 * q + 2;
	const bool o_ok = io <= II - 2, two = io + 1 <= II - 1;
	const size_t j = (size_t)jr + 1, k = (size_t)kr + 1;
	const size_t sj = (size_t)II, sk = (size_t)II * JJ;
	const size_t row = j * sj + k * sk, rowA = j * A.SJ + k * A.SK;
	C27 ce, co;
	real_t de = 0.0, dn = 0.0;
	if (mine) {
		load_coef27<false, false, false>(A, rowA, ie, io, two, ce, co);
		co.pw = ce.pw_e; // both are the operator entry (KPW, io): one register pair less across the item loop
		ldpair(A.so + rowA + ie, true, de, dn); // KP plane
	}
#pragma unroll 1
	for (int m = 0; m < nrhs; m++) {
		if (!item_on(active, m)) continue; // uniform over the workgroup
		real_t acc = 0.0;
		if (mine) {
			const size_t off = (size_t)m * stride;
			const real_t *__restrict__ zm = z + off;
			real_t qe[3][3][3], qo[3][3][3];
			if (FIRST) { // the 3x3 windows of z
				real_t zfe, zfo;
				load_vec27<0>(zm, zm, row, sj, sk, ie, io, two, qe, qo, zfe, zfo);
			} else { // of z + beta p, row by row: pcg_dir27's expression per element
				const real_t beta = sc[(size_t)m * PCG_NSC + PCG_BETA];
				const real_t *__restrict__ pm = p + off;
#pragma unroll
				for (int dk = 0; dk < 3; dk++)
#pragma unroll
					for (int dj = 0; dj < 3; dj++) {
						const size_t y = row + (ptrdiff_t)(dj - 1) * (ptrdiff_t)sj + (ptrdiff_t)(dk - 1) * (ptrdiff_t)sk;
						real_t w0, w1, w2, w3, p0, p1, p2, p3;
						ldpair(pm + y + ie - 1, true, p0, p1);
						ldpair(pm + y + io, two, p2, p3);
						ldpair(zm + y + ie - 1, true, w0, w1);
						ldpair(zm + y + io, two, w2, w3);
						qe[dk][dj][0] = w0 + beta * p0;
						qe[dk][dj][1] = w1 + beta * p1;
						qe[dk][dj][2] = w2 + beta * p2;
						qo[dk][dj][0] = qe[dk][dj][1];
						qo[dk][dj][1] = qe[dk][dj][2];
						qo[dk][dj][2] = w3 + beta * p3;
					}
			}
			dir27_emit(de, dn, ce, co, qe, qo, o_ok, w, pn, off, row, ie, acc);
		}
		const real_t t = block_sum_k<BS>(acc, lds);
		if (threadIdx.x == 0) part[(size_t)m * nblk + L] = t;
	}
}

// 27-point on a batch of a periodic level (cedar_amd_solver_fcg_periodic_many): pcg_dir27_per's wrap rule with
// pcg_dir27_many's item loop; per item the expressions, their order and the sums are pcg_dir27_per's.  Rows of one trip
// (longer rows: pcg_dir27_per item by item, pcg_direction_periodic_many).  The 52 coefficients
// and the diagonal pair are fetched once, from the Cedar planes (a periodic level has no row-interleaved copy), and stay
// in registers across the items; one window set is live at a time.  Per item the nine window rows are loaded as
// pcg_dir27_per loads them, every load before any patch; the i patch follows under the uniform `if (pd.x)`.
template <int BS, bool FIRST>
__global__ __launch_bounds__(BS) __attribute__((amdgpu_waves_per_eu(2))) void pcg_dir27_per_many(
    const Op3 A, const real_t *__restrict__ z, const real_t *__restrict__ p, real_t *__restrict__ pn, real_t *__restrict__ w,
    const real_t *__restrict__ sc, int II, int JJ, int KK, unsigned nblk, TileShape ts, PerDirs pd, real_t *__restrict__ part,
    int nrhs, size_t stride, unsigned active)
{
	__shared__ real_t lds[(BS + 63) / 64];
	const unsigned L = xcd_remap(blockIdx.x, nblk);
	if (L >= nblk) return; // grid padding: no slab entry
	unsigned jr, kr;
	const bool have = tile_rows(L, (unsigned)(JJ - 2), (unsigned)(KK - 2), ts, jr, kr);
	const int q = threadIdx.x;
	const bool mine = have && 2 * q + 1 <= II - 2;
	const int ie = 2 * q + 1, io = 2 * q + 2;
	const bool o_ok = io <= II - 2, two = io + 1 <= II - 1;
	const int j = have ? (int)jr + 1 : 1, k = have ? (int)kr + 1 : 1;
	const size_t sj = (size_t)II, sk = (size_t)II * JJ;
	const size_t row = (size_t)j * sj + (size_t)k * sk, rowA = (size_t)j * A.SJ + (size_t)k * A.SK;
	// the window rows (j-1, j, j+1) x (k-1, k, k+1), wrapped
	const size_t oj[3] = {sj * (size_t)wrap_lo(j - 1, JJ, pd.y), sj * (size_t)j, sj * (size_t)wrap_hi(j + 1, JJ, pd.y)};
	const size_t ok[3] = {sk * (size_t)wrap_lo(k - 1, KK, pd.z), sk * (size_t)k, sk * (size_t)wrap_hi(k + 1, KK, pd.z)};
	C27 ce, co;
	real_t de = 0.0, dn = 0.0;
	if (mine) {
		load_coef27<false, false, false>(A, rowA, ie, io, two, ce, co);
		co.pw = ce.pw_e; // both are the operator entry (KPW, io): one register pair less across the item loop
		ldpair(A.so + rowA + ie, true, de, dn); // KP plane
	}
#pragma unroll 1
	for (int m = 0; m < nrhs; m++) {
		if (!item_on(active, m)) continue; // uniform over the workgroup
		real_t acc = 0.0;
		if (mine) {
			const size_t off = (size_t)m * stride;
			const real_t *__restrict__ zm = z + off, *__restrict__ pm = FIRST ? zm : p + off;
			const real_t beta = FIRST ? 0.0 : sc[(size_t)m * PCG_NSC + PCG_BETA];
			real_t qe[3][3][3], qo[3][3][3];
#pragma unroll
			for (int dk = 0; dk < 3; dk++)
#pragma unroll
				for (int dj = 0; dj < 3; dj++) {
					const size_t y = oj[dj] + ok[dk];
					real_t w0, w1, w2, w3;
					ldpair(zm + y + ie - 1, true, w0, w1);
					ldpair(zm + y + io, two, w2, w3);
					if (!FIRST) {
						real_t p0, p1, p2, p3;
						ldpair(pm + y + ie - 1, true, p0, p1);
						ldpair(pm + y + io, two, p2, p3);
						w0 = w0 + beta * p0;
						w1 = w1 + beta * p1;
						w2 = w2 + beta * p2;
						w3 = w3 + beta * p3;
					}
					qe[dk][dj][0] = w0; qe[dk][dj][1] = w1; qe[dk][dj][2] = w2;
					qo[dk][dj][0] = w1; qo[dk][dj][1] = w2; qo[dk][dj][2] = w3;
				}
			// periodic x (uniform branch): what was formed from a ghost of the row is replaced by the same expression at the
			// wrapped address (pcg_dir27_per)
			if (pd.x) {
				auto P = [&](size_t y) -> real_t { return FIRST ? zm[y] : zm[y] + beta * pm[y]; };
				if (ie == 1) {
#pragma unroll
					for (int dk = 0; dk < 3; dk++)
#pragma unroll
						for (int dj = 0; dj < 3; dj++) qe[dk][dj][0] = P(oj[dj] + ok[dk] + II - 2);
				}
				if (io + 1 >= II - 1) {
#pragma unroll
					for (int dk = 0; dk < 3; dk++)
#pragma unroll
						for (int dj = 0; dj < 3; dj++) {
							const real_t v = P(oj[dj] + ok[dk] + 1);
							if (two) qo[dk][dj][2] = v;
							else qe[dk][dj][2] = v;
						}
				}
			}
			dir27_emit(de, dn, ce, co, qe, qo, o_ok, w, pn, off, row, ie, acc);
		}
		const real_t t = block_sum_k<BS>(acc, lds);
		if (threadIdx.x == 0) part[(size_t)m * nblk + L] = t;
	}
}

// pcg_upd on the items m0 .. m0 + nitems-1 (m0 = ITEM_CHUNK * blockIdx.y): the same UPD_NB workgroups and row dealing, the
// item loop inside the pair loop so that diag (ZM 1) is read once per pair.  A lane's r.r / r.z of an item run over all
// the rows dealt to the workgroup: LDS columns (lane-private), summed per item as pcg_upd sums rr and rz.  Item m's slab:
// part[2 m gridDim.x + ..] (r.r), part[(2 m + 1) gridDim.x + ..] (r.z).
template <int ZM, bool MOVE>
__global__ __launch_bounds__(256) void pcg_upd_many(real_t *__restrict__ x, real_t *__restrict__ r,
                                                    const real_t *__restrict__ p, const real_t *__restrict__ w,
                                                    real_t *__restrict__ z, const real_t *__restrict__ diag,
                                                    const real_t *__restrict__ sc, int II, int JJ, int KK,
                                                    real_t *__restrict__ part, int nrhs, size_t stride, unsigned active)
{
	__shared__ real_t lds[4];
	__shared__ real_t rrl[ITEM_CHUNK][256], rzl[(ZM == 1 || ZM == 2) ? ITEM_CHUNK : 1][256];
	const int m0 = ITEM_CHUNK * (int)blockIdx.y, nitems = min(ITEM_CHUNK, nrhs - m0);
	const int nj = JJ - 2, nk = KK == 1 ? 1 : KK - 2;
	const size_t nrows = (size_t)nj * nk;
	for (int t = 0; t < nitems; t++) {
		rrl[t][threadIdx.x] = 0.0;
		if (ZM == 1 || ZM == 2) rzl[t][threadIdx.x] = 0.0;
	}
	for (size_t tr = blockIdx.x; tr < nrows; tr += gridDim.x) {
		const size_t j = tr % nj + 1, k = KK == 1 ? 0 : tr / nj + 1;
		const size_t row = (size_t)II * (j + (size_t)JJ * k);
		for (int q = threadIdx.x; 2 * q + 1 <= II - 2; q += blockDim.x) {
			const size_t ip = row + 2 * q + 1;
			const bool two = 2 * q + 2 <= II - 2;
			real_t d0 = 0.0, d1 = 0.0;
			if (ZM == 1) ldpair(diag + ip, two, d0, d1);
#pragma unroll 1
			for (int t = 0; t < nitems; t++) {
				const int m = m0 + t;
				if (!item_on(active, m)) continue;
				const size_t ie = (size_t)m * stride + ip;
				const real_t a = MOVE ? sc[(size_t)m * PCG_NSC + PCG_ALPHA] : 0.0;
				const bool mv = MOVE && a != 0.0; // alpha = 0 (breakdown): x and r stay as they are
				real_t rr = rrl[t][threadIdx.x], rz = (ZM == 1 || ZM == 2) ? rzl[t][threadIdx.x] : 0.0;
				real_t r0, r1;
				ldpair(r + ie, two, r0, r1);
				if (mv) {
					real_t x0, x1, p0, p1, w0, w1;
					ldpair(x + ie, two, x0, x1);
					ldpair(p + ie, two, p0, p1);
					ldpair(w + ie, two, w0, w1);
					x0 = x0 + a * p0; x1 = x1 + a * p1;
					r0 = r0 - a * w0; r1 = r1 - a * w1;
					if (two) {
						d2u v; v.x = x0; v.y = x1; *reinterpret_cast<d2u *>(x + ie) = v;
						v.x = r0; v.y = r1; *reinterpret_cast<d2u *>(r + ie) = v;
					} else {
						x[ie] = x0; r[ie] = r0;
					}
				}
				rr += r0 * r0;
				if (two) rr += r1 * r1;
				if (ZM == 1) {
					const real_t z0 = r0 / d0, z1 = two ? r1 / d1 : 0.0;
					if (two) { d2u v; v.x = z0; v.y = z1; *reinterpret_cast<d2u *>(z + ie) = v; }
					else z[ie] = z0;
					rz += r0 * z0;
					if (two) rz += r1 * z1;
				} else if (ZM == 2) {
					real_t z0, z1;
					ldpair(z + ie, two, z0, z1);
					rz += r0 * z0;
					if (two) rz += r1 * z1;
				}
				rrl[t][threadIdx.x] = rr;
				if (ZM == 1 || ZM == 2) rzl[t][threadIdx.x] = rz;
			}
		}
	}
	for (int t = 0; t < nitems; t++) {
		const int m = m0 + t;
		if (!item_on(active, m)) continue; // uniform over the workgroup
		const real_t s0 = block_sum_k<256>(rrl[t][threadIdx.x], lds);
		const real_t s1 = (ZM == 1 || ZM == 2) ? block_sum_k<256>(rzl[t][threadIdx.x], lds) : 0.0;
		if (threadIdx.x == 0) {
			part[(size_t)(2 * m) * gridDim.x + blockIdx.x] = s0;
			part[(size_t)(2 * m + 1) * gridDim.x + blockIdx.x] = s1;
		}
	}
}

// second stages: workgroup m is pcg_alpha / pcg_rho on item m's slab (item stride `ld` doubles) and scalar block
__global__ __launch_bounds__(RED_BS) void pcg_alpha_many(const real_t *__restrict__ part, unsigned n, size_t ld,
                                                         real_t *__restrict__ sc, unsigned active)
{
	__shared__ real_t lds[RED_BS / 64];
	const int m = blockIdx.x;
	if (!item_on(active, m)) return;
	const real_t sigma = slab_sum(part + (size_t)m * ld, n, lds);
	if (threadIdx.x == 0) set_alpha(sigma, sc + (size_t)m * PCG_NSC);
}

__global__ __launch_bounds__(RED_BS) void pcg_rho_many(const real_t *__restrict__ part, unsigned n, size_t ld, int has_rz,
                                                       int first, real_t *__restrict__ sc, unsigned active)
{
	__shared__ real_t lds[RED_BS / 64];
	const int m = blockIdx.x;
	if (!item_on(active, m)) return;
	const real_t *__restrict__ pm = part + (size_t)m * ld;
	const real_t rr = slab_sum(pm, n, lds);
	const real_t rz = has_rz == 1 ? slab_sum(pm + n, n, lds) : rr;
	if (threadIdx.x == 0) set_rho(rr, rz, has_rz, first, sc + (size_t)m * PCG_NSC);
}

// pcg_dwz on the items m0 .. m0 + nitems-1, laid out as pcg_upd_many<2, false> (same workgroups, row dealing, item loop
// inside the pair loop, LDS columns per lane) with a third column for w.z.  Item m's slab: three sections of gridDim.x
// from part[3 m gridDim.x]: r.r, r.z, w.z.
__global__ __launch_bounds__(256) void pcg_dwz_many(const real_t *__restrict__ r, const real_t *__restrict__ z,
                                                    const real_t *__restrict__ w, int II, int JJ, int KK,
                                                    real_t *__restrict__ part, int nrhs, size_t stride, unsigned active)
{
	__shared__ real_t lds[4];
	__shared__ real_t rrl[ITEM_CHUNK][256], rzl[ITEM_CHUNK][256], wzl[ITEM_CHUNK][256];
	const int m0 = ITEM_CHUNK * (int)blockIdx.y, nitems = min(ITEM_CHUNK, nrhs - m0);
	const int nj = JJ - 2, nk = KK == 1 ? 1 : KK - 2;
	const size_t nrows = (size_t)nj * nk;
	for (int t = 0; t < nitems; t++) {
		rrl[t][threadIdx.x] = 0.0;
		rzl[t][threadIdx.x] = 0.0;
		wzl[t][threadIdx.x] = 0.0;
	}
	for (size_t tr = blockIdx.x; tr < nrows; tr += gridDim.x) {
		const size_t j = tr % nj + 1, k = KK == 1 ? 0 : tr / nj + 1;
		const size_t row = (size_t)II * (j + (size_t)JJ * k);
		for (int q = threadIdx.x; 2 * q + 1 <= II - 2; q += blockDim.x) {
			const size_t ip = row + 2 * q + 1;
			const bool two = 2 * q + 2 <= II - 2;
#pragma unroll 1
			for (int t = 0; t < nitems; t++) {
				const int m = m0 + t;
				if (!item_on(active, m)) continue;
				const size_t ie = (size_t)m * stride + ip;
				real_t rr = rrl[t][threadIdx.x], rz = rzl[t][threadIdx.x], wz = wzl[t][threadIdx.x];
				real_t r0, r1, z0, z1, w0, w1;
				ldpair(r + ie, two, r0, r1);
				ldpair(z + ie, two, z0, z1);
				ldpair(w + ie, two, w0, w1);
				rr += r0 * r0;
				if (two) rr += r1 * r1;
				rz += r0 * z0;
				if (two) rz += r1 * z1;
				wz += w0 * z0;
				if (two) wz += w1 * z1;
				rrl[t][threadIdx.x] = rr;
				rzl[t][threadIdx.x] = rz;
				wzl[t][threadIdx.x] = wz;
			}
		}
	}
	for (int t = 0; t < nitems; t++) {
		const int m = m0 + t;
		if (!item_on(active, m)) continue; // uniform over the workgroup
		const real_t s0 = block_sum_k<256>(rrl[t][threadIdx.x], lds);
		const real_t s1 = block_sum_k<256>(rzl[t][threadIdx.x], lds);
		const real_t s2 = block_sum_k<256>(wzl[t][threadIdx.x], lds);
		if (threadIdx.x == 0) {
			part[(size_t)(3 * m) * gridDim.x + blockIdx.x] = s0;
			part[(size_t)(3 * m + 1) * gridDim.x + blockIdx.x] = s1;
			part[(size_t)(3 * m + 2) * gridDim.x + blockIdx.x] = s2;
		}
	}
}

// workgroup m is pcg_rho_flex on item m's slab and scalar block
__global__ __launch_bounds__(RED_BS) void pcg_rho_flex_many(const real_t *__restrict__ part, unsigned n, size_t ld, int first,
                                                            real_t *__restrict__ sc, unsigned active)
{
	__shared__ real_t lds[RED_BS / 64];
	const int m = blockIdx.x;
	if (!item_on(active, m)) return;
	const real_t *__restrict__ pm = part + (size_t)m * ld;
	const real_t rr = slab_sum(pm, n, lds);
	const real_t rz = slab_sum(pm + n, n, lds);
	const real_t wz = slab_sum(pm + 2 * (size_t)n, n, lds);
	if (threadIdx.x == 0) set_rho_flex(rr, rz, wz, first, sc + (size_t)m * PCG_NSC);
}

// ---------------------------------------------------------------- launchers
// a run-time switch as a compile-time constant: f(std::bool_constant<b>), f(std::integral_constant<int, V>) for the V
// that v equals (none: the last)
template <class F>
void with_bool(bool b, F &&f) { b ? f(std::true_type{}) : f(std::false_type{}); }

template <int V, int... Vs, class F>
void with_int(int v, F &&f)
{
	if constexpr (sizeof...(Vs) > 0) {
		if (v != V) return with_int<Vs...>(v, f);
	}
	f(std::integral_constant<int, V>{});
}

unsigned item_chunks(int nrhs) { return (unsigned)((nrhs + ITEM_CHUNK - 1) / ITEM_CHUNK); }

// The launch geometry of a direction pass on nrhs items (the single pass: 1) and its slab layout: one partial per
// workgroup task, n per item.  2D: the item in grid.z; 7-point: the item chunk in grid.y; 27-point: the items are walked
// inside the workgroup, which is as wide as the row's pairs need.
struct DirGeom {
	int nd, nst;
	dim3 grid;
	int bs;     // workgroup width
	unsigned n; // slab entries of one item
	Op3 A;      // 27-point: the operator view, the tile walk and the pairs of a row
	TileShape ts;
	int npairs;
};

DirGeom dir_geom(const real_t *so, const Op3 *op27, int nd, int nst, int II, int JJ, int KK, int nrhs)
{
	DirGeom g{};
	g.nd = nd, g.nst = nst;
	if (nd == 2) {
		g.grid = dim3((II - 2 + 255) / 256, JJ - 2, nrhs);
		g.bs = 256;
		g.n = g.grid.x * g.grid.y;
	} else if (nst == 4) {
		g.n = (unsigned)(JJ - 2) * (unsigned)(KK - 2);
		g.bs = II - 2 >= 256 ? 256 : (II - 2 > 64 ? 128 : 64);
		g.grid = dim3(xcd_grid(g.n), item_chunks(nrhs));
	} else {
		g.A = op27 ? *op27 : op3_cedar(so, nullptr, II, JJ, KK);
		g.ts = tile_shape_resid();
		g.n = tile_blocks((unsigned)(JJ - 2), (unsigned)(KK - 2), g.ts);
		g.npairs = (II - 2 + 1) / 2;
		g.bs = g.npairs <= 64 ? 64 : g.npairs <= 128 ? 128 : 256;
		g.grid = dim3(xcd_grid(g.n));
	}
	return g;
}

// launches the direction kernel of g: k2(NINE, FIRST), k7(FIRST) or k27(BS, FIRST) launches its instantiation
template <class K2, class K7, class K27>
void dir_launch(const DirGeom &g, bool first, K2 &&k2, K7 &&k7, K27 &&k27)
{
	with_bool(first, [&](auto F) {
		if (g.nd == 2) with_bool(g.nst == 5, [&](auto NINE) { k2(NINE, F); });
		else if (g.nst == 4) k7(F);
		else with_int<64, 128, 256>(g.bs, [&](auto BS) { k27(BS, F); });
	});
}

// A batched pass and its second stage.  The batched 27-point kernels take rows of one trip; longer rows go through the
// single pass item by item (its second stage included): one(m, slab_m, sc_m).
template <class ONE, class K2, class K7, class K27>
void dir_launch_many(const DirGeom &g, bool first, size_t ld, real_t *slab, real_t *sc, hipStream_t st, Batch bt, unsigned active,
                     ONE &&one, K2 &&k2, K7 &&k7, K27 &&k27)
{
	if (g.npairs > 256) {
		for (int m = 0; m < bt.n; m++)
			if ((active >> m) & 1u) one(m, slab + m * ld, sc + (size_t)m * PCG_NSC);
		return;
	}
	dir_launch(g, first, k2, k7, k27);
	hipLaunchKernelGGL(pcg_alpha_many, dim3(bt.n), dim3(RED_BS), 0, st, slab, g.n, (size_t)g.n, sc, active);
}

// the workgroups of pcg_upd / pcg_dwz and their batched forms: one per row up to UPD_NB
unsigned upd_blocks(int JJ, int KK)
{
	const size_t nrows = (size_t)(JJ - 2) * (KK == 1 ? 1 : KK - 2);
	return (unsigned)std::min<size_t>(UPD_NB, nrows);
}

// the rho stages' has_rz of a zmode: 0 r.r only (zmode 3), 1 r.z in the second slab section, 2 r.z = r.r (zmode 0)
int has_rz(int zmode) { return zmode == 3 ? 0 : zmode == 0 ? 2 : 1; }

} // namespace

size_t pcg_slab_doubles(int nd, int nst, int II, int JJ, int KK)
{
	return std::max(3 * (size_t)UPD_NB, (size_t)dir_geom(nullptr, nullptr, nd, nst, II, JJ, KK, 1).n); // pcg_dots_wz: three sections
}

void pcg_direction(const real_t *so, const Op3 *op27, const real_t *z, const real_t *p, real_t *pn, real_t *w, int nd,
                   int nst, int II, int JJ, int KK, bool first, real_t *slab, real_t *sc, hipStream_t st,
                   real_t *partial)
{
	const DirGeom g = dir_geom(so, op27, nd, nst, II, JJ, KK, 1);
	dir_launch(
	    g, first,
	    [&](auto NINE, auto F) { hipLaunchKernelGGL((pcg_dir2<NINE(), F()>), g.grid, dim3(g.bs), 0, st, so, z, p, pn, w, sc, II, JJ, slab); },
	    [&](auto F) { hipLaunchKernelGGL(pcg_dir7<F()>, g.grid, dim3(g.bs), 0, st, so, z, p, pn, w, sc, II, JJ, KK, g.n, slab); },
	    [&](auto BS, auto F) { hipLaunchKernelGGL((pcg_dir27<BS(), F()>), g.grid, dim3(g.bs), 0, st, g.A, z, p, pn, w, sc, II, JJ, KK, g.n, g.ts, slab); });
	if (partial) hipLaunchKernelGGL(pcg_partial, dim3(1), dim3(RED_BS), 0, st, slab, g.n, 1, partial);
	else hipLaunchKernelGGL(pcg_alpha, dim3(1), dim3(RED_BS), 0, st, slab, g.n, sc);
}

void pcg_direction_periodic(const real_t *so, const real_t *z, const real_t *p, real_t *pn, real_t *w, int nd, int nst, int II,
                            int JJ, int KK, int ibc, bool first, real_t *slab, real_t *sc, hipStream_t st, real_t *partial)
{
	const PerDirs pd = per_dirs(nd, ibc);
	const DirGeom g = dir_geom(so, nullptr, nd, nst, II, JJ, KK, 1); // a periodic level is read from its Cedar planes
	dir_launch(
	    g, first,
	    [&](auto NINE, auto F) { hipLaunchKernelGGL((pcg_dir2_per<NINE(), F()>), g.grid, dim3(g.bs), 0, st, so, z, p, pn, w, sc, II, JJ, pd, slab); },
	    [&](auto F) { hipLaunchKernelGGL(pcg_dir7_per<F()>, g.grid, dim3(g.bs), 0, st, so, z, p, pn, w, sc, II, JJ, KK, g.n, pd, slab); },
	    [&](auto BS, auto F) { hipLaunchKernelGGL((pcg_dir27_per<BS(), F()>), g.grid, dim3(g.bs), 0, st, g.A, z, p, pn, w, sc, II, JJ, KK, g.n, g.ts, pd, slab); });
	if (partial) hipLaunchKernelGGL(pcg_partial, dim3(1), dim3(RED_BS), 0, st, slab, g.n, 1, partial);
	else hipLaunchKernelGGL(pcg_alpha, dim3(1), dim3(RED_BS), 0, st, slab, g.n, sc);
}

void pcg_update(int zmode, bool move, real_t *x, real_t *r, const real_t *p, const real_t *w, real_t *z,
                const real_t *diag, int II, int JJ, int KK, bool first, real_t *slab, real_t *sc, hipStream_t st,
                real_t *partial)
{
	const unsigned nb = upd_blocks(JJ, KK);
	with_int<0, 1, 2, 3>(zmode, [&](auto ZM) {
		with_bool(move, [&](auto MV) {
			hipLaunchKernelGGL((pcg_upd<ZM(), MV()>), dim3(nb), dim3(256), 0, st, x, r, p, w, z, diag, sc, II, JJ, KK, slab);
		});
	});
	if (!partial) hipLaunchKernelGGL(pcg_rho, dim3(1), dim3(RED_BS), 0, st, slab, nb, has_rz(zmode), first ? 1 : 0, sc);
	else if (zmode != 3) hipLaunchKernelGGL(pcg_partial, dim3(1), dim3(RED_BS), 0, st, slab, nb, has_rz(zmode) == 1 ? 2 : 1, partial);
}

void pcg_direction_many(const real_t *so, const Op3 *op27, const real_t *z, const real_t *p, real_t *pn, real_t *w, int nd,
                        int nst, int II, int JJ, int KK, bool first, real_t *slab, real_t *sc, hipStream_t st, Batch bt,
                        unsigned active)
{
	const DirGeom g = dir_geom(so, op27, nd, nst, II, JJ, KK, bt.n);
	dir_launch_many(
	    g, first, pcg_slab_doubles(nd, nst, II, JJ, KK), slab, sc, st, bt, active,
	    [&](int m, real_t *slab_m, real_t *sc_m) {
		    pcg_direction(so, op27, z + m * bt.stride, first ? nullptr : p + m * bt.stride, pn + m * bt.stride, w + m * bt.stride, nd,
		                  nst, II, JJ, KK, first, slab_m, sc_m, st);
	    },
	    [&](auto NINE, auto F) { hipLaunchKernelGGL((pcg_dir2_many<NINE(), F()>), g.grid, dim3(g.bs), 0, st, so, z, p, pn, w, sc, II, JJ, slab, bt.stride, active); },
	    [&](auto F) { hipLaunchKernelGGL(pcg_dir7_many<F()>, g.grid, dim3(g.bs), 0, st, so, z, p, pn, w, sc, II, JJ, KK, g.n, slab, bt.n, bt.stride, active); },
	    [&](auto BS, auto F) { hipLaunchKernelGGL((pcg_dir27_many<BS(), F()>), g.grid, dim3(g.bs), 0, st, g.A, z, p, pn, w, sc, II, JJ, KK, g.n, g.ts, slab, bt.n, bt.stride, active); });
}

// a periodic level is read from its Cedar planes.  2D: the items are walked inside the workgroup (pcg_dir2_per_many), so the
// launch grid is the single pass' own
void pcg_direction_periodic_many(const real_t *so, const real_t *z, const real_t *p, real_t *pn, real_t *w, int nd, int nst, int II,
                                 int JJ, int KK, int ibc, bool first, real_t *slab, real_t *sc, hipStream_t st, Batch bt,
                                 unsigned active)
{
	const PerDirs pd = per_dirs(nd, ibc);
	const DirGeom g = dir_geom(so, nullptr, nd, nst, II, JJ, KK, nd == 2 ? 1 : bt.n);
	dir_launch_many(
	    g, first, pcg_slab_doubles(nd, nst, II, JJ, KK), slab, sc, st, bt, active,
	    [&](int m, real_t *slab_m, real_t *sc_m) {
		    pcg_direction_periodic(so, z + m * bt.stride, first ? nullptr : p + m * bt.stride, pn + m * bt.stride, w + m * bt.stride, nd,
		                           nst, II, JJ, KK, ibc, first, slab_m, sc_m, st);
	    },
	    [&](auto NINE, auto F) { hipLaunchKernelGGL((pcg_dir2_per_many<NINE(), F()>), g.grid, dim3(g.bs), 0, st, so, z, p, pn, w, sc, II, JJ, pd, slab, bt.n, bt.stride, active); },
	    [&](auto F) { hipLaunchKernelGGL(pcg_dir7_per_many<F()>, g.grid, dim3(g.bs), 0, st, so, z, p, pn, w, sc, II, JJ, KK, g.n, pd, slab, bt.n, bt.stride, active); },
	    [&](auto BS, auto F) { hipLaunchKernelGGL((pcg_dir27_per_many<BS(), F()>), g.grid, dim3(g.bs), 0, st, g.A, z, p, pn, w, sc, II, JJ, KK, g.n, g.ts, pd, slab, bt.n, bt.stride, active); });
}

void pcg_update_many(int zmode, bool move, real_t *x, real_t *r, const real_t *p, const real_t *w, real_t *z,
                     const real_t *diag, int II, int JJ, int KK, bool first, real_t *slab, real_t *sc, hipStream_t st,
                     Batch bt, unsigned active)
{
	const unsigned nb = upd_blocks(JJ, KK);
	const dim3 grid(nb, item_chunks(bt.n));
	with_int<0, 1, 2, 3>(zmode, [&](auto ZM) {
		with_bool(move, [&](auto MV) {
			hipLaunchKernelGGL((pcg_upd_many<ZM(), MV()>), grid, dim3(256), 0, st, x, r, p, w, z, diag, sc, II, JJ, KK, slab, bt.n, bt.stride, active);
		});
	});
	hipLaunchKernelGGL(pcg_rho_many, dim3(bt.n), dim3(RED_BS), 0, st, slab, nb, (size_t)2 * nb, has_rz(zmode), first ? 1 : 0, sc, active);
}

void pcg_dots_wz(const real_t *r, const real_t *z, const real_t *w, int II, int JJ, int KK, bool first, real_t *slab,
                 real_t *sc, hipStream_t st)
{
	const unsigned nb = upd_blocks(JJ, KK);
	hipLaunchKernelGGL(pcg_dwz, dim3(nb), dim3(256), 0, st, r, z, w, II, JJ, KK, slab);
	hipLaunchKernelGGL(pcg_rho_flex, dim3(1), dim3(RED_BS), 0, st, slab, nb, first ? 1 : 0, sc);
}

void pcg_dots_wz_many(const real_t *r, const real_t *z, const real_t *w, int II, int JJ, int KK, bool first, real_t *slab,
                      real_t *sc, hipStream_t st, Batch bt, unsigned active)
{
	const unsigned nb = upd_blocks(JJ, KK);
	const dim3 grid(nb, item_chunks(bt.n));
	hipLaunchKernelGGL(pcg_dwz_many, grid, dim3(256), 0, st, r, z, w, II, JJ, KK, slab, bt.n, bt.stride, active);
	hipLaunchKernelGGL(pcg_rho_flex_many, dim3(bt.n), dim3(RED_BS), 0, st, slab, nb, (size_t)3 * nb, first ? 1 : 0, sc, active);
}

void pcg_ranks_alpha(const real_t *gathered, int world, int stride, real_t *sc, hipStream_t st)
{
	hipLaunchKernelGGL(pcg_alpha_ranks, dim3(1), dim3(64), 0, st, gathered, world, stride, sc);
}

void pcg_ranks_rho(int zmode, const real_t *gathered, int world, int stride, bool first, real_t *sc, hipStream_t st)
{
	hipLaunchKernelGGL(pcg_rho_ranks, dim3(1), dim3(64), 0, st, gathered, world, stride, has_rz(zmode), first ? 1 : 0, sc);
}

void pcg_ghost_shell(const real_t *z, const real_t *p, real_t *pn, const real_t *sc, const ShellBoxes &bx, int II, int JJ,
                     bool first, hipStream_t st)
{
	if (bx.n == 0) return;
	size_t most = 0;
	for (int b = 0; b < bx.n; b++) most = std::max(most, (size_t)bx.box[6 * b + 3] * bx.box[6 * b + 4] * bx.box[6 * b + 5]);
	const dim3 grid((unsigned)std::min<size_t>((most + 255) / 256, 1024), (unsigned)bx.n);
	if (first) hipLaunchKernelGGL(pcg_shell<true>, grid, dim3(256), 0, st, z, p, pn, sc, bx, II, JJ);
	else hipLaunchKernelGGL(pcg_shell<false>, grid, dim3(256), 0, st, z, p, pn, sc, bx, II, JJ);
}

} // namespace cedar_amd
