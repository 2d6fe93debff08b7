// Device bodies of the zebra line kernels -- the affine scan, both DPTTRS forms (factors read in place, and from the
// scan-ordered copy), the right-hand-side formation and the x-line kernel body -- written once for two views of the
// operator and two element types of the factors:
//   Op2c + real_t  the FP64 Cedar planes and factors of the boundary (lines.hip);
//   Op2f + float   the row-interleaved single-precision copy and float factors (linesf.hip).
// An operator entry or a factor is promoted to double when it is loaded (exact); vectors, LDS, the scan and all
// arithmetic are FP64 in the same term order and the same chunking.  So a kernel on (Op2f, float) has the bits of the
// same kernel on (Op2c, real_t) over the operator and the factor arrays each rounded to float.  Only the mapping of
// unknowns to lanes while the right-hand sides are formed differs between the two (every right-hand side is
// independent of the others): pairs of doubles there, aligned quads of floats here.
#pragma once
#include "common.h"
#include "relax2_dev.h"
#include <type_traits>

namespace cedar_amd {

// ------------------------------------------------------------------ affine scan
// Every lane owns CH consecutive unknowns of the line.  A sweep over a tile of BS*CH unknowns is
//   (1) lane-local: compose the CH maps  y -> a*y + c  of the chunk            (sequential, exact order)
//   (2) workgroup scan of the BS composites: Kogge-Stone over wavefront shuffles, cross-wave fix-up
//       through LDS, scalar carry from the previous tile
//   (3) lane-local: re-run the chunk from the value entering it.
// Only step (2) re-associates the recurrence.
constexpr int CH = 8;
__device__ __forceinline__ int lpad(int i) { return i + (i >> 3); } // LDS index: one pad per 8 -> stride-9 chunks, no bank conflicts

// (p[0], p[1]) with one 16-byte load (8-byte aligned)
__device__ __forceinline__ void ldpair2(const real_t *__restrict__ p, real_t *out)
{
	const d2u v = *reinterpret_cast<const d2u *>(p);
	out[0] = v.x; out[1] = v.y;
}
// four floats on a 16-byte boundary
typedef float f4v __attribute__((ext_vector_type(4)));

template <int BS>
__device__ __forceinline__ void affine_scan(real_t a, real_t c, real_t carry, real_t *wa, real_t *wc,
                                            real_t &y_in, real_t &y_last)
{
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
	for (int off = 1; off < 64; off <<= 1) {
		const real_t ap = __shfl_up(a, off, 64), cp = __shfl_up(c, off, 64);
		if (lane >= off) {
			c = a * cp + c;
			a = a * ap;
		}
	}
	real_t ae = __shfl_up(a, 1, 64), ce = __shfl_up(c, 1, 64); // composite of the lanes before this one
	if (lane == 0) { ae = 1.0; ce = 0.0; }
	constexpr int NW = BS / 64;
	if (NW > 1) {
		if (lane == 63) { wa[w] = a; wc[w] = c; }
		__syncthreads();
		real_t y = carry;
		for (int u = 0; u < w; u++) y = wa[u] * y + wc[u];
		carry = y;
	}
	y_in = ae * carry + ce;
	y_last = a * carry + c;
}

// Solve L D L^T x = y for the line held in LDS (padded index lpad(i)); d[0..n), e[0..n-1) in HBM, doubles or floats.
template <int BS, class FT>
__device__ __forceinline__ void line_pttrs(real_t *y, int n, const FT *__restrict__ d, const FT *__restrict__ e,
                                           real_t *wa, real_t *wc, real_t *carry_slot)
{
	// forward: y_i = y_i - e_{i-1} y_{i-1}
	real_t carry = 0.0;
	for (int base = 0; base < n; base += BS * CH) {
		const int i0 = base + (int)threadIdx.x * CH;
		real_t a[CH], c[CH];
#pragma unroll
		for (int m = 0; m < CH; m++) {
			const int i = i0 + m;
			if (i < n) { c[m] = y[lpad(i)]; a[m] = i > 0 ? -(real_t)e[i - 1] : 0.0; }
			else { c[m] = 0.0; a[m] = 0.0; }
		}
		real_t A = 1.0, Cc = 0.0;
#pragma unroll
		for (int m = 0; m < CH; m++) { Cc = a[m] * Cc + c[m]; A = a[m] * A; }
		real_t v, last;
		affine_scan<BS>(A, Cc, carry, wa, wc, v, last);
#pragma unroll
		for (int m = 0; m < CH; m++) {
			v = a[m] * v + c[m];
			if (i0 + m < n) y[lpad(i0 + m)] = v;
		}
		if (threadIdx.x == BS - 1) *carry_slot = last;
		__syncthreads();
		carry = *carry_slot;
		__syncthreads();
	}
	// backward: x_i = y_i/d_i - e_i x_{i+1}; reversed position r <-> i = n-1-r
	carry = 0.0;
	for (int base = 0; base < n; base += BS * CH) {
		const int r0 = base + (int)threadIdx.x * CH;
		real_t a[CH], c[CH];
#pragma unroll
		for (int m = 0; m < CH; m++) {
			const int r = r0 + m, i = n - 1 - r;
			if (r < n) { c[m] = y[lpad(i)] / (real_t)d[i]; a[m] = r > 0 ? -(real_t)e[i] : 0.0; }
			else { c[m] = 0.0; a[m] = 0.0; }
		}
		real_t A = 1.0, Cc = 0.0;
#pragma unroll
		for (int m = 0; m < CH; m++) { Cc = a[m] * Cc + c[m]; A = a[m] * A; }
		real_t v, last;
		affine_scan<BS>(A, Cc, carry, wa, wc, v, last);
#pragma unroll
		for (int m = 0; m < CH; m++) {
			v = a[m] * v + c[m];
			if (r0 + m < n) y[lpad(n - 1 - r0 - m)] = v;
		}
		if (threadIdx.x == BS - 1) *carry_slot = last;
		__syncthreads();
		carry = *carry_slot;
		__syncthreads();
	}
}

// The same solve on a scan-ordered copy of the factors (resident solver, lines longer than a wavefront tile).
// line_pttrs reads e / d where the scan needs them: lane L owns unknowns 8L .. 8L+7 of a tile, so one wave
// instruction gathers 64 x 8 bytes spread over 4 KB -- 32 cache lines for 512 useful bytes -- and the sweeps of a
// line wait on eight such gathers.  Measured at 8192^2 (profiles/r02_experiment_line_relax.log): 0.52 of the 1.34 ms
// of an x sweep is this solve, 0.22 ms of it the gathers alone.  The copy stores, per line and tile of BS*CH unknowns,
// the forward multipliers a = -e(i-1), the backward multipliers a = -e(i) and the pivots d(i) in the order the lanes
// consume them: [tile][kind][m/W][lane][m%W] with W the elements of a 16-byte load (2 doubles, 4 floats), so every
// load is a coalesced 16-byte-per-lane stream, and the next tile's factors are requested before the current tile is
// scanned.  Same values, same chunks, same scan => bit-identical to line_pttrs.
template <int BS> __host__ __device__ inline size_t pf_tiles(int n) { return (size_t)(n + BS * CH - 1) / (BS * CH); }
template <int BS> __host__ __device__ inline size_t pf_line_doubles(int n) { return pf_tiles<BS>(n) * 3 * CH * BS; } // elements
template <int BS, class FT = real_t> __device__ __forceinline__ size_t pf_off(int t, int kind, int m, int lane)
{
	constexpr int W = 16 / (int)sizeof(FT);
	return ((((size_t)t * 3 + kind) * (CH / W) + (m / W)) * BS + lane) * W + (m % W);
}

template <int BS>
__device__ __forceinline__ void pf_load(const real_t *__restrict__ pfl, int t, int kind, real_t (&v)[CH])
{
#pragma unroll
	for (int mp = 0; mp < CH / 2; mp++) {
		const d2u w = *reinterpret_cast<const d2u *>(pfl + pf_off<BS>(t, kind, 2 * mp, threadIdx.x));
		v[2 * mp] = w.x; v[2 * mp + 1] = w.y;
	}
}
// the float copy: a lane's eight values of a kind are two aligned 16-byte loads
template <int BS>
__device__ __forceinline__ void pf_load(const float *__restrict__ pfl, int t, int kind, real_t (&v)[CH])
{
#pragma unroll
	for (int mq = 0; mq < CH / 4; mq++) {
		const f4v w = *reinterpret_cast<const f4v *>(pfl + pf_off<BS, float>(t, kind, 4 * mq, threadIdx.x));
		v[4 * mq] = (real_t)w.x; v[4 * mq + 1] = (real_t)w.y; v[4 * mq + 2] = (real_t)w.z; v[4 * mq + 3] = (real_t)w.w;
	}
}

template <int BS, class FT>
__device__ __forceinline__ void line_pttrs_pf(real_t *y, int n, const FT *__restrict__ pfl,
                                              real_t *wa, real_t *wc, real_t *carry_slot)
{
	const int nt = (int)pf_tiles<BS>(n);
	real_t a[CH], an[CH], dn[CH], dd[CH];
	pf_load<BS>(pfl, 0, 0, a);
	real_t carry = 0.0;
	for (int t = 0; t < nt; t++) {
		if (t + 1 < nt) pf_load<BS>(pfl, t + 1, 0, an); // next tile, or ...
		else { pf_load<BS>(pfl, 0, 1, an); pf_load<BS>(pfl, 0, 2, dn); } // ... the first backward tile
		const int i0 = t * BS * CH + (int)threadIdx.x * CH;
		real_t c[CH];
#pragma unroll
		for (int m = 0; m < CH; m++) c[m] = i0 + m < n ? y[lpad(i0 + m)] : 0.0;
		real_t A = 1.0, Cc = 0.0;
#pragma unroll
		for (int m = 0; m < CH; m++) { Cc = a[m] * Cc + c[m]; A = a[m] * A; }
		real_t v, last;
		affine_scan<BS>(A, Cc, carry, wa, wc, v, last);
#pragma unroll
		for (int m = 0; m < CH; m++) {
			v = a[m] * v + c[m];
			if (i0 + m < n) y[lpad(i0 + m)] = v;
		}
		if (threadIdx.x == BS - 1) *carry_slot = last;
		__syncthreads();
		carry = *carry_slot;
		__syncthreads();
#pragma unroll
		for (int m = 0; m < CH; m++) a[m] = an[m];
	}
#pragma unroll
	for (int m = 0; m < CH; m++) dd[m] = dn[m];
	carry = 0.0;
	for (int t = 0; t < nt; t++) {
		if (t + 1 < nt) { pf_load<BS>(pfl, t + 1, 1, an); pf_load<BS>(pfl, t + 1, 2, dn); }
		const int r0 = t * BS * CH + (int)threadIdx.x * CH;
		real_t c[CH];
#pragma unroll
		for (int m = 0; m < CH; m++) {
			const int r = r0 + m;
			c[m] = r < n ? y[lpad(n - 1 - r)] / dd[m] : 0.0;
		}
		real_t A = 1.0, Cc = 0.0;
#pragma unroll
		for (int m = 0; m < CH; m++) { Cc = a[m] * Cc + c[m]; A = a[m] * A; }
		real_t v, last;
		affine_scan<BS>(A, Cc, carry, wa, wc, v, last);
#pragma unroll
		for (int m = 0; m < CH; m++) {
			v = a[m] * v + c[m];
			if (r0 + m < n) y[lpad(n - 1 - r0 - m)] = v;
		}
		if (threadIdx.x == BS - 1) *carry_slot = last;
		__syncthreads();
		carry = *carry_slot;
		__syncthreads();
#pragma unroll
		for (int m = 0; m < CH; m++) { a[m] = an[m]; dd[m] = dn[m]; }
	}
}

// doubles of LDS a line of n unknowns needs (padded line + scan scratch)
static inline size_t line_lds_doubles(int n) { return (size_t)n + (size_t)(n >> 3) + 40; } // line + 16 + 16 wave aggregates + carry

// ------------------------------------------------------------------ x-lines
// Sherman-Morrison closure of a cyclic line held in LDS: y holds the solution of the folded system;
// a second solve with the rank-one column u (-c_first at the first, -c_last at the last unknown),
// alpha = u_1 + u_n, beta = (y_1 + y_n) / (1 + alpha), x = y - beta u (relax_lines_x.f90:212-226).
// On return `y` holds u and every lane holds beta; ys[t] (lane-strided) kept the first solution.
template <int BS>
__device__ __forceinline__ real_t line_sherman_morrison(real_t *y, int n, const real_t *__restrict__ d,
                                                        const real_t *__restrict__ e, real_t cfirst, real_t clast,
                                                        real_t *wa, real_t *wc, real_t *cs, real_t &y1, real_t &yn)
{
	y1 = y[lpad(0)];
	yn = y[lpad(n - 1)];
	__syncthreads();
	for (int t = threadIdx.x; t < n; t += BS) y[lpad(t)] = 0.0;
	__syncthreads();
	if (threadIdx.x == 0) {
		y[lpad(0)] = -cfirst;
		y[lpad(n - 1)] = -clast; // n == 1: the second assignment wins, as in the reference
	}
	__syncthreads();
	line_pttrs<BS>(y, n, d, e, wa, wc, cs);
	const real_t alpha = y[lpad(0)] + y[lpad(n - 1)];
	real_t beta = y1 + yn;
	beta = beta / (1.0 + alpha);
	return beta;
}

// Right-hand sides of line jr (grid row jr, n = II - 2 unknowns) into y, wide loads, on the FP64 planes: every lane
// forms the right-hand side of RU pairs of unknowns per pass with 16-byte loads, all 11 x RU loads of a pass requested
// before the first is used.  With one point per lane and pass (the scalar loop of the kernel body) a wave waits out one
// HBM round trip per 64 unknowns -- 72 % of the wave cycles of this kernel were such waits
// (profiles/r02_lines_sq_counters.txt).  The unknowns [lo, hi) are done on return; the scalar loop takes the others.
template <int BS, bool NINE, bool YT>
__device__ __forceinline__ void lines_rhs_wide(const Op2c &A, const real_t *__restrict__ qf, const real_t *__restrict__ q,
                                               size_t jr, int II, real_t *y, int &lo, int &hi)
{
	constexpr int RU = 4;
	const size_t sj = II, row = jr * sj;
	const int n = II - 2, npair = n >> 1;
	for (int pb0 = 0; pb0 < npair; pb0 += BS * RU) {
		real_t f[RU][2], ks[RU][2], ksn[RU][2], ksw[RU][2], knwe[RU][2], knwn[RU][2], kswne[RU][2], qs[RU][4], qn[RU][4];
#pragma unroll
		for (int u = 0; u < RU; u++) {
			const int pr = pb0 + u * BS + (int)threadIdx.x;
			if (pr < npair) {
				const size_t i = 1 + 2 * (size_t)pr, x = row + i;
				ldpair2(qf + x, f[u]);
				ldpair2(A.row(KS, jr) + i, ks[u]);
				ldpair2(A.row(KS, jr + 1) + i, ksn[u]);
				ldpair2(q + x - 1 - sj, &qs[u][0]); ldpair2(q + x + 1 - sj, &qs[u][2]);
				ldpair2(q + x - 1 + sj, &qn[u][0]); ldpair2(q + x + 1 + sj, &qn[u][2]);
				if (NINE) {
					ldpair2(A.row(KSW, jr) + i, ksw[u]);
					ldpair2(A.row(KNW, jr) + i + 1, knwe[u]);
					ldpair2(A.row(KNW, jr + 1) + i, knwn[u]);
					ldpair2(A.row(KSW, jr + 1) + i + 1, kswne[u]);
				}
			}
		}
#pragma unroll
		for (int u = 0; u < RU; u++) {
			const int pr = pb0 + u * BS + (int)threadIdx.x;
			if (pr < npair) {
#pragma unroll
				for (int h = 0; h < 2; h++) {
					real_t s = f[u][h];
					s = s + ks[u][h] * qs[u][1 + h];
					s = s + ksn[u][h] * qn[u][1 + h];
					if (NINE) {
						s = s + ksw[u][h] * qs[u][h];
						if (YT) {
							s = s + knwn[u][h] * qn[u][h];
							s = s + knwe[u][h] * qs[u][2 + h];
						} else {
							s = s + knwe[u][h] * qs[u][2 + h];
							s = s + knwn[u][h] * qn[u][h];
						}
						s = s + kswne[u][h] * qn[u][2 + h];
					}
					y[lpad(2 * pr + h)] = s;
				}
			}
		}
	}
	lo = 0;
	hi = npair * 2; // an odd last unknown goes through the scalar loop
}

// The same on the float copy.  Element i of a slot-row sits at float offset i + 1, so the aligned 16-byte quads of a
// slot-row hold the grid points i = 4k-1 .. 4k+2: a lane forms the right-hand sides of such a quad.  The four entries
// stored at the point itself (KS and KSW of row jr, KS and KNW of row jr+1) are one aligned 16-byte load each; the two
// stored at i+1 (KNW of row jr, KSW of row jr+1) are the same aligned quad shifted by one, its last element a 4-byte load
// -- never a misaligned wide load.  The vectors are three 16-byte pairs per neighbour row and two of qf.  Quads k = 1 ..
// (II-4)/4 lie wholly inside the line with all their neighbours inside the row; the points i = 1, 2 before them and the
// up to three after them go through the scalar loop.  Each right-hand side has the term order of the FP64 kernels.
template <int BS, bool NINE, bool YT>
__device__ __forceinline__ void lines_rhs_wide(const Op2f &A, const real_t *__restrict__ qf, const real_t *__restrict__ q,
                                               size_t jr, int II, real_t *y, int &lo, int &hi)
{
	constexpr int RU = BS >= 1024 ? 1 : 2; // 1024 lanes: 128 registers a lane
	const size_t sj = II, row = jr * sj;
	const int nq = (II - 4) / 4;
	if (nq <= 0) { lo = hi = 0; return; }
	const float *pks = A.row(KS, jr), *pksn = A.row(KS, jr + 1);
	const float *pksw = A.row(KSW, jr), *pknw = A.row(KNW, jr), *pknwn = A.row(KNW, jr + 1), *pkswn = A.row(KSW, jr + 1);
	for (int qb0 = 0; qb0 < nq; qb0 += BS * RU) {
		f4v ks[RU], ksn[RU], ksw[RU], knw[RU], knwn[RU], kswn[RU];
		float knw4[RU], kswn4[RU];
		real_t f[RU][4], qs[RU][6], qn[RU][6];
#pragma unroll
		for (int u = 0; u < RU; u++) {
			const int k = 1 + qb0 + u * BS + (int)threadIdx.x;
			if (k <= nq) {
				const size_t i = 4 * (size_t)k - 1, x = row + i;
				ldpair2(qf + x, &f[u][0]); ldpair2(qf + x + 2, &f[u][2]);
				ks[u] = *reinterpret_cast<const f4v *>(pks + i);
				ksn[u] = *reinterpret_cast<const f4v *>(pksn + i);
#pragma unroll
				for (int p = 0; p < 3; p++) {
					ldpair2(q + x - 1 - sj + 2 * p, &qs[u][2 * p]);
					ldpair2(q + x - 1 + sj + 2 * p, &qn[u][2 * p]);
				}
				if (NINE) {
					ksw[u] = *reinterpret_cast<const f4v *>(pksw + i);
					knw[u] = *reinterpret_cast<const f4v *>(pknw + i); knw4[u] = pknw[i + 4];
					knwn[u] = *reinterpret_cast<const f4v *>(pknwn + i);
					kswn[u] = *reinterpret_cast<const f4v *>(pkswn + i); kswn4[u] = pkswn[i + 4];
				}
			}
		}
#pragma unroll
		for (int u = 0; u < RU; u++) {
			const int k = 1 + qb0 + u * BS + (int)threadIdx.x;
			if (k <= nq) {
#pragma unroll
				for (int h = 0; h < 4; h++) {
					real_t s = f[u][h];
					s = s + (real_t)ks[u][h] * qs[u][1 + h];
					s = s + (real_t)ksn[u][h] * qn[u][1 + h];
					if (NINE) {
						const real_t knwe = (real_t)(h < 3 ? knw[u][(h + 1) & 3] : knw4[u]);
						const real_t kswne = (real_t)(h < 3 ? kswn[u][(h + 1) & 3] : kswn4[u]);
						s = s + (real_t)ksw[u][h] * qs[u][h];
						if (YT) {
							s = s + (real_t)knwn[u][h] * qn[u][h];
							s = s + knwe * qs[u][2 + h];
						} else {
							s = s + knwe * qs[u][2 + h];
							s = s + (real_t)knwn[u][h] * qn[u][h];
						}
						s = s + kswne * qn[u][2 + h];
					}
					y[lpad(4 * k - 2 + h)] = s; // unknown t = i - 1
				}
			}
		}
	}
	lo = 2;
	hi = 4 * nq + 2;
}

// The x-line kernel body: one workgroup owns line L of the colour jb (grid row 1 + jb + 2L), held in LDS.
// YT: the arrays are the transposed ones of a y-line sweep (setup_lines_yt): rows are the y lines, and the two
// cross terms are added in relax_lines_y.f90's order.  V: Op2c | Op2f; FT: the factors' element type, real_t | float
// (sor: the two SOR planes, PERM: pf is their scan-ordered copy).  dbg: timing experiments (1: no solve, 2: no
// right-hand side).
template <int BS, bool NINE, bool SM, bool YT, bool PERM, class V, class FT>
__device__ __forceinline__ void relax_lines_x_body(const V &A, const real_t *__restrict__ qf, real_t *__restrict__ q,
                                                   const FT *__restrict__ sor, int II, int JJ, int jb, int nlines, int dbg,
                                                   const FT *__restrict__ pf, size_t bstride, real_t *lds)
{
	const int npad = (II - 2) + ((II - 2) >> 3) + 1;
	real_t *y = lds, *wa = lds + npad, *wc = wa + 16, *cs = wc + 16;
	const unsigned L = xcd_remap(blockIdx.x, (unsigned)nlines);
	if (L >= (unsigned)nlines) return;
	qf += bstride * blockIdx.y; q += bstride * blockIdx.y; // batch item (common.h Batch)
	const size_t sj = II, PS = (size_t)II * JJ;
	const size_t jr = (size_t)(1 + jb + 2 * (int)L);
	const size_t row = jr * sj;
	const int n = II - 2;
	// right-hand side (relax_lines_x.f90:106-111 / :128-129), reference term order.  Lines longer than a wavefront tile
	// take the wide loads of lines_rhs_wide for the unknowns [lo, hi)
	int lo = 0, hi = 0;
	if (dbg & 2) hi = n; // experiment: no right-hand side (LDS left as is)
	else if (BS >= 256) lines_rhs_wide<BS, NINE, YT>(A, qf, q, jr, II, y, lo, hi);
	const int nleft = lo + (n - hi);
	for (int u = threadIdx.x; u < nleft; u += BS) {
		const int t = u < lo ? u : hi + (u - lo);
		const size_t i = 1 + (size_t)t, x = row + i;
		real_t s = qf[x];
		s = s + (real_t)A.row(KS, jr)[i] * q[x - sj];
		s = s + (real_t)A.row(KS, jr + 1)[i] * q[x + sj];
		if (NINE) {
			s = s + (real_t)A.row(KSW, jr)[i] * q[x - 1 - sj];
			if (YT) { // (i+1,j-1) is (row+1, col-1) of the transposed arrays and comes first
				s = s + (real_t)A.row(KNW, jr + 1)[i] * q[x - 1 + sj];
				s = s + (real_t)A.row(KNW, jr)[i + 1] * q[x + 1 - sj];
			} else {
				s = s + (real_t)A.row(KNW, jr)[i + 1] * q[x + 1 - sj];
				s = s + (real_t)A.row(KNW, jr + 1)[i] * q[x - 1 + sj];
			}
			s = s + (real_t)A.row(KSW, jr + 1)[i + 1] * q[x + 1 + sj];
		}
		y[lpad(t)] = s;
	}
	__syncthreads();
	if (dbg & 1) { /* experiment: no solve */ }
	else if (PERM) line_pttrs_pf<BS>(y, n, pf + (size_t)(jb + 2 * (int)L) * pf_line_doubles<BS>(n), wa, wc, cs);
	else line_pttrs<BS>(y, n, sor + row + 1, sor + PS + row + 2, wa, wc, cs);
	for (int t = threadIdx.x; t < n; t += BS) q[row + 1 + t] = y[lpad(t)];
	if constexpr (SM) {
		real_t y1, yn;
		const real_t beta = line_sherman_morrison<BS>(y, n, sor + row + 1, sor + PS + row + 2, A.row(KW, jr)[1],
		                                              A.row(KW, jr)[II - 1], wa, wc, cs, y1, yn);
		for (int t = threadIdx.x; t < n; t += BS) q[row + 1 + t] = q[row + 1 + t] - beta * y[lpad(t)]; // same lane wrote it
	}
}

// lanes per line: one wavefront up to 512 unknowns, else CEDAR_AMD_LINE_BS (256 / 512 / 1024).  The size fixes the
// association of the scan, so every launcher of a line solve takes it from here.
static inline int line_bs(int n)
{
	if (n <= 512) return 64;
	static const int e = getenv("CEDAR_AMD_LINE_BS") ? atoi(getenv("CEDAR_AMD_LINE_BS")) : 256;
	return (e == 512 || e == 1024) ? e : 256;
}

// a line must fit the 160 KB of LDS (up to ~18,000 unknowns)
static inline bool line_fits_lds(int n) { return line_lds_doubles(n) * sizeof(real_t) <= 160 * 1024 - 512; }
} // namespace cedar_amd
// longer lines are refused through the host's print_error callback like every other unsupported request, the sweep is skipped
extern "C" void print_error(char *msg);
namespace cedar_amd {
static inline bool lds_ok(int n, const char *who)
{
	if (!line_fits_lds(n)) {
		char buf[160];
		snprintf(buf, sizeof(buf), "%s: a line of %d unknowns does not fit the 160 KB LDS of a CU; sweep skipped", who, n);
		print_error(buf);
		return false;
	}
	return true;
}

// ------------------------------------------------------------------ kernels and launchers, instantiated by lines.hip on
// (Op2c, real_t) and by linesf.hip on (Op2f, float)
template <int BS, bool NINE, bool SM, bool YT, bool PERM, class V, class FT>
__global__ __launch_bounds__(BS) void relax_lines_x_kernel(const V A, const real_t *__restrict__ qf, real_t *__restrict__ q,
                                                            const FT *__restrict__ sor, int II, int JJ, int jb, int nlines,
                                                            int dbg, const FT *__restrict__ pf, size_t bstride)
{
	extern __shared__ __attribute__((aligned(16))) real_t lds[];
	relax_lines_x_body<BS, NINE, SM, YT, PERM>(A, qf, q, sor, II, JJ, jb, nlines, dbg, pf, bstride, lds);
}

// the scan-ordered copy of the factors of `sor` (doubles) in doubles or, rounded to nearest even, in floats; a finite
// factor that leaves float's range raises *overflow (when given; an ordinary store of 1)
template <int BS, class FT>
__global__ __launch_bounds__(BS) void lines_permute_kernel(const real_t *__restrict__ sor, FT *__restrict__ pf,
                                                            int n, int ld, size_t PS, int *__restrict__ overflow)
{
	const int l = blockIdx.x;
	const real_t *d = sor + (size_t)ld * (l + 1) + 1, *e = sor + PS + (size_t)ld * (l + 1) + 2;
	FT *out = pf + (size_t)l * pf_line_doubles<BS>(n);
	const int nt = (int)pf_tiles<BS>(n);
	bool bad = false;
	for (int t = 0; t < nt; t++)
		for (int m = 0; m < CH; m++) {
			const int r = t * BS * CH + (int)threadIdx.x * CH + m, i = n - 1 - r; // forward position r, backward unknown i
			const real_t v0 = (r < n && r > 0) ? -e[r - 1] : 0.0, v1 = (r < n && r > 0) ? -e[i] : 0.0, v2 = r < n ? d[i] : 1.0;
			const FT f0 = (FT)v0, f1 = (FT)v1, f2 = (FT)v2;
			bad = bad || (isinf(f0) && !isinf(v0)) || (isinf(f1) && !isinf(v1)) || (isinf(f2) && !isinf(v2));
			out[pf_off<BS, FT>(t, 0, m, threadIdx.x)] = f0;
			out[pf_off<BS, FT>(t, 1, m, threadIdx.x)] = f1;
			out[pf_off<BS, FT>(t, 2, m, threadIdx.x)] = f2;
		}
	if (overflow && bad) *overflow = 1;
}

template <class FT>
static void lines_permute_t(const real_t *sor, FT *pf, int n, int ld, int nlines, size_t PS, int *overflow, hipStream_t st)
{
	if (nlines <= 0 || n <= 0) return;
	switch (line_bs(n)) {
	case 256: hipLaunchKernelGGL((lines_permute_kernel<256, FT>), dim3(nlines), dim3(256), 0, st, sor, pf, n, ld, PS, overflow); break;
	case 512: hipLaunchKernelGGL((lines_permute_kernel<512, FT>), dim3(nlines), dim3(512), 0, st, sor, pf, n, ld, PS, overflow); break;
	case 1024: hipLaunchKernelGGL((lines_permute_kernel<1024, FT>), dim3(nlines), dim3(1024), 0, st, sor, pf, n, ld, PS, overflow); break;
	default: break;
	}
}

template <int BS, bool NINE, bool SM, bool YT, bool PERM, class V, class FT>
static void launch_x_kp(const V &A, const real_t *qf, real_t *q, const FT *sor, int II, int JJ, int jb, int nlines,
                        hipStream_t st, const FT *pf, Batch bt)
{
	size_t shm = line_lds_doubles(II - 2) * sizeof(real_t);
	auto k = relax_lines_x_kernel<BS, NINE, SM, YT, PERM, V, FT>;
	if (shm > 64 * 1024) CEDAR_HIP_CHECK(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
	const char *ed = getenv("CEDAR_AMD_LINE_DBG"); // timing experiments only (1: no solve, 2: no right-hand side)
	hipLaunchKernelGGL(k, dim3(xcd_grid(nlines), bt.n), dim3(BS), shm, st, A, qf, q, sor, II, JJ, jb, nlines, ed ? atoi(ed) : 0, pf,
	                   bt.stride);
}

// pf != nullptr: the scan-ordered factor copy of this line direction (lines_permute), Dirichlet lines of the 256-lane kernel
template <int BS, bool NINE, bool SM, bool YT, class V, class FT>
static void launch_x_k(const V &A, const real_t *qf, real_t *q, const FT *sor, int II, int JJ, int jb, int nlines,
                       hipStream_t st, const FT *pf, Batch bt)
{
	if (!SM && pf && BS >= 256) launch_x_kp<BS, NINE, false, YT, true>(A, qf, q, sor, II, JJ, jb, nlines, st, pf, bt);
	else launch_x_kp<BS, NINE, SM, YT, false>(A, qf, q, sor, II, JJ, jb, nlines, st, (const FT *)nullptr, bt);
}

template <int BS, class V, class FT>
static void launch_x_n(const V &A, const real_t *qf, real_t *q, const FT *sor, int II, int JJ,
                       int nstncl, int jb, hipStream_t st, bool sm, bool yt, const FT *pf, Batch bt)
{
	int nlines = (JJ - 2 - jb + 1) / 2;
	if (nlines <= 0) return;
	if (yt) { // Dirichlet only
		if (nstncl == 5) launch_x_k<BS, true, false, true>(A, qf, q, sor, II, JJ, jb, nlines, st, pf, bt);
		else launch_x_k<BS, false, false, true>(A, qf, q, sor, II, JJ, jb, nlines, st, pf, bt);
		return;
	}
	if constexpr (std::is_same<FT, real_t>::value) { // cyclic lines (Sherman-Morrison): the FP64 planes only
		if (sm) {
			if (nstncl == 5) launch_x_k<BS, true, true, false>(A, qf, q, sor, II, JJ, jb, nlines, st, pf, bt);
			else launch_x_k<BS, false, true, false>(A, qf, q, sor, II, JJ, jb, nlines, st, pf, bt);
			return;
		}
	}
	if (nstncl == 5) launch_x_k<BS, true, false, false>(A, qf, q, sor, II, JJ, jb, nlines, st, pf, bt);
	else launch_x_k<BS, false, false, false>(A, qf, q, sor, II, JJ, jb, nlines, st, pf, bt);
}

// one colour (lines jb, jb + 2, ..) of the grid II x JJ
template <class V, class FT>
static void launch_x(const V &A, const real_t *qf, real_t *q, const FT *sor, int II, int JJ,
                     int nstncl, int jb, hipStream_t st, bool sm, bool yt, const FT *pf, Batch bt)
{
	switch (line_bs(II - 2)) {
	case 64: launch_x_n<64>(A, qf, q, sor, II, JJ, nstncl, jb, st, sm, yt, pf, bt); break;
	case 512: launch_x_n<512>(A, qf, q, sor, II, JJ, nstncl, jb, st, sm, yt, pf, bt); break;
	case 1024: launch_x_n<1024>(A, qf, q, sor, II, JJ, nstncl, jb, st, sm, yt, pf, bt); break;
	default: launch_x_n<256>(A, qf, q, sor, II, JJ, nstncl, jb, st, sm, yt, pf, bt);
	}
}

} // namespace cedar_amd
