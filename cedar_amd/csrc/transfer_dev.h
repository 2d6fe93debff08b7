// Device bodies of the inter-grid transfers, written on a view of the interpolation weights (common.h CiW<T>): the
// element type T is real_t for the Cedar-layout weights (transfer.hip, many3d.hip) and float for the single-precision
// copy (transferf.hip).  A weight is promoted to double when it is used -- exact -- and every
// expression keeps the reference's term order (-ffp-contract=off), so a kernel on the float view has the bits of the
// FP64 kernel on the weights rounded to float.  The per-point sums do not depend on which lane owns a point.
#pragma once
#include "common.h"

namespace cedar_amd {

template <class T> struct ci_pair; // two adjacent weights of a row, moved by one 8- / 16-byte load at an 8-byte boundary
template <> struct ci_pair<float> { typedef float type __attribute__((ext_vector_type(2), aligned(8))); };
template <> struct ci_pair<real_t> { typedef d2u type; };

// ------------------------------------------------------------------ restriction
// Term t of b_c = P^T r at a coarse point, in the reference's order (BMG2_SymStd_restrict.f90:73-92,
// BMG3_SymStd_restrict.f90:115-150): the fine point at offset (t%3 - 1, (t/3)%3 - 1) of plane 0, -1, +1 (t/9 = 0, 1, 2);
// its weight is entry R*_SLOT[t] of the coarse point at offset (+1 where the fine offset is +1, else 0).  Term 4, the
// point itself, has weight one.
#define CEDAR_R2_SLOTS {LNE, LA, LNW, LR, -1, LL, LSE, LB, LSW}
#define CEDAR_R3_SLOTS                                                                                                  \
	{LXYNE, LXYA,  LXYNW, LXYR,  -1,   LXYL,  LXYSE, LXYB,  LXYSW, LTNE, LYZNW, LTNW, LXZNE, LXZA,                     \
	 LXZNW, LTSE,  LYZNE, LTSW,  LBNE, LYZSW, LBNW,  LXZSE, LXZB,  LXZSW, LBSE, LYZSE, LBSW}

// the weights of the coarse point at wc (offset in the view) into w[], one load per term
template <int NT, class T> __device__ __forceinline__ void restrict_weights(T (&w)[NT], const CiW<T> &W, size_t wc)
{
	constexpr int s2[9] = CEDAR_R2_SLOTS, s3[27] = CEDAR_R3_SLOTS;
#pragma unroll
	for (int t = 0; t < NT; t++) {
		const int slot = NT == 9 ? s2[t % 9] : s3[t];
		if (slot < 0) { w[t] = (T)1; continue; }
		const int x = t % 3, y = (t / 3) % 3, z = t / 9;
		w[t] = W.p[(size_t)slot * W.ss + wc + (x == 2 ? 1 : 0) + (y == 2 ? W.sj : 0) + (z == 2 ? W.sk : 0)];
	}
}

// the weights of the coarse points ic and ic + 1 of a row (wc: offset of ic, at an 8-byte boundary of the view): terms at
// coarse offset 0 are one pair load; terms at offset +1 take ic + 1 from the pair and ic + 2 by one more load, which
// hits the line the neighbouring lane's pair brings in
template <int NT, class T>
__device__ __forceinline__ void restrict_weights_pair(T (&w0)[NT], T (&w1)[NT], const CiW<T> &W, size_t wc)
{
	typedef typename ci_pair<T>::type pair_t;
	constexpr int s2[9] = CEDAR_R2_SLOTS, s3[27] = CEDAR_R3_SLOTS;
#pragma unroll
	for (int t = 0; t < NT; t++) {
		const int slot = NT == 9 ? s2[t % 9] : s3[t];
		if (slot < 0) { w0[t] = w1[t] = (T)1; continue; }
		const int x = t % 3, y = (t / 3) % 3, z = t / 9;
		const T *r = W.p + (size_t)slot * W.ss + wc + (y == 2 ? W.sj : 0) + (z == 2 ? W.sk : 0);
		const pair_t a = *reinterpret_cast<const pair_t *>(r);
		if (x == 2) { w0[t] = a.y; w1[t] = r[2]; }
		else { w0[t] = a.x; w1[t] = a.y; }
	}
}

// the sum at the coarse point whose fine point is q[f]; sf / tf: fine row / plane strides (NT = 9: tf unused)
template <int NT, class T>
__device__ __forceinline__ real_t restrict_sum(const T (&w)[NT], const real_t *__restrict__ q, size_t f, size_t sf, size_t tf)
{
	real_t s = 0.0;
#pragma unroll
	for (int t = 0; t < NT; t++) {
		const int x = t % 3, y = (t / 3) % 3, z = t / 9;
		size_t g = f;
		if (x == 0) g -= 1;
		if (x == 2) g += 1;
		if (y == 0) g -= sf;
		if (y == 2) g += sf;
		if (z == 1) g -= tf;
		if (z == 2) g += tf;
		if (t == 0) s = (real_t)w[0] * q[g];
		else if (t == 4) s = s + q[g];
		else s = s + (real_t)w[t] * q[g];
	}
	return s;
}

// one lane per coarse point (gather, unit stride in the coarse row); batch item from blockIdx.z
template <class T>
__global__ __launch_bounds__(256) void restrict2_kernel(const real_t *__restrict__ q, real_t *__restrict__ qc, const CiW<T> W,
                                                         int II, int JJ, int IIC, int JJC, size_t bsf, size_t bsc)
{
	const int ic = blockIdx.x * blockDim.x + threadIdx.x + 1; // 0-based incl. ghost
	const int jc = blockIdx.y + 1;
	if (ic > IIC - 2) return;
	q += bsf * blockIdx.z; qc += bsc * blockIdx.z; // batch item (common.h Batch)
	const size_t sc = IIC, sf = II;
	const size_t c = (size_t)ic + sc * jc;
	const size_t f = (size_t)(2 * ic - 1) + sf * (size_t)(2 * jc - 1); // 1-based i = 2(ic1-1) -> 0-based 2*ic-1
	T w[9];
	restrict_weights<9>(w, W, (size_t)ic + W.sj * jc);
	qc[c] = restrict_sum<9>(w, q, f, sf, 0);
}

// one lane per pair of coarse points (ic, ic + 1), ic odd: the weights move as pairs
template <class T>
__global__ __launch_bounds__(256) void restrict2_pairs_kernel(const real_t *__restrict__ q, real_t *__restrict__ qc,
                                                               const CiW<T> W, int II, int JJ, int IIC, int JJC, size_t bsf,
                                                               size_t bsc)
{
	const int ic = 2 * (blockIdx.x * blockDim.x + threadIdx.x) + 1;
	const int jc = blockIdx.y + 1;
	if (ic > IIC - 2) return;
	q += bsf * blockIdx.z; qc += bsc * blockIdx.z;
	const size_t sc = IIC, sf = II;
	const size_t c = (size_t)ic + sc * jc;
	const size_t f = (size_t)(2 * ic - 1) + sf * (size_t)(2 * jc - 1);
	T w0[9], w1[9];
	restrict_weights_pair<9>(w0, w1, W, (size_t)ic + W.sj * jc);
	const real_t s0 = restrict_sum<9>(w0, q, f, sf, 0);
	if (ic + 1 <= IIC - 2) {
		d2u t; t.x = s0; t.y = restrict_sum<9>(w1, q, f + 2, sf, 0);
		*reinterpret_cast<d2u *>(qc + c) = t;
	} else
		qc[c] = s0;
}

template <class T>
__global__ __launch_bounds__(128) void restrict3_kernel(const real_t *__restrict__ q, real_t *__restrict__ qc, const CiW<T> W,
                                                         int II, int JJ, int KK, int IIC, int JJC, int KKC)
{
	const int ic = blockIdx.x * blockDim.x + threadIdx.x + 1;
	const int jc = blockIdx.y + 1, kc = blockIdx.z + 1;
	if (ic > IIC - 2) return;
	const size_t sc = IIC, tc = (size_t)IIC * JJC;
	const size_t sf = II, tf = (size_t)II * JJ;
	const size_t c = (size_t)ic + sc * jc + tc * kc;
	const size_t f = (size_t)(2 * ic - 1) + sf * (size_t)(2 * jc - 1) + tf * (size_t)(2 * kc - 1);
	T w[27];
	restrict_weights<27>(w, W, (size_t)ic + W.sj * jc + W.sk * kc);
	qc[c] = restrict_sum<27>(w, q, f, sf, tf);
}

// restrict3_kernel on a batch: the 26 CI entries of a coarse point once, the items inside
template <class T>
__global__ __launch_bounds__(128) void restrict3_many_kernel(const real_t *__restrict__ q, real_t *__restrict__ qc,
                                                              const CiW<T> W, int II, int JJ, int KK, int IIC, int JJC, int KKC,
                                                              int nitems, size_t bsf, size_t bsc)
{
	const int ic = blockIdx.x * blockDim.x + threadIdx.x + 1;
	const int jc = blockIdx.y + 1, kc = blockIdx.z + 1;
	if (ic > IIC - 2) return;
	const size_t sc = IIC, tc = (size_t)IIC * JJC;
	const size_t sf = II, tf = (size_t)II * JJ;
	const size_t c = (size_t)ic + sc * jc + tc * kc;
	const size_t f = (size_t)(2 * ic - 1) + sf * (size_t)(2 * jc - 1) + tf * (size_t)(2 * kc - 1);
	T w[27];
	restrict_weights<27>(w, W, (size_t)ic + W.sj * jc + W.sk * kc);
	for (int m = 0; m < nitems; m++) qc[(size_t)m * bsc + c] = restrict_sum<27>(w, q + (size_t)m * bsf, f, sf, tf);
}

// one lane per pair of coarse points (ic, ic + 1), ic odd, the weights as pairs; one vector or a batch
template <class T>
__global__ __launch_bounds__(128) void restrict3_pairs_kernel(const real_t *__restrict__ q, real_t *__restrict__ qc,
                                                               const CiW<T> W, int II, int JJ, int KK, int IIC, int JJC, int KKC,
                                                               int nitems, size_t bsf, size_t bsc)
{
	const int ic = 2 * (blockIdx.x * blockDim.x + threadIdx.x) + 1;
	const int jc = blockIdx.y + 1, kc = blockIdx.z + 1;
	if (ic > IIC - 2) return;
	const size_t sc = IIC, tc = (size_t)IIC * JJC;
	const size_t sf = II, tf = (size_t)II * JJ;
	const size_t c = (size_t)ic + sc * jc + tc * kc;
	const size_t f = (size_t)(2 * ic - 1) + sf * (size_t)(2 * jc - 1) + tf * (size_t)(2 * kc - 1);
	const bool two = ic + 1 <= IIC - 2;
	T w0[27], w1[27];
	restrict_weights_pair<27>(w0, w1, W, (size_t)ic + W.sj * jc + W.sk * kc);
	for (int m = 0; m < nitems; m++) {
		const real_t *qm = q + (size_t)m * bsf;
		real_t *qcm = qc + (size_t)m * bsc;
		const real_t s0 = restrict_sum<27>(w0, qm, f, sf, tf);
		if (two) {
			d2u t; t.x = s0; t.y = restrict_sum<27>(w1, qm, f + 2, sf, tf);
			*reinterpret_cast<d2u *>(qcm + c) = t;
		} else
			qcm[c] = s0;
	}
}

// ------------------------------------------------------------------ interp_add 2D
template <class T>
__global__ __launch_bounds__(256) void interp_add2_kernel(real_t *__restrict__ q, const real_t *__restrict__ qc,
                                                           real_t *__restrict__ res, const real_t *__restrict__ so_diag,
                                                           const CiW<T> W, int IIC, int JJC, int IIF, int JJF, int imax, int jmax,
                                                           size_t bsf, size_t bsc)
{
	// 1-based fine indices as in the reference
	const int i = blockIdx.x * blockDim.x + threadIdx.x + 2;
	const int j = blockIdx.y + 2;
	if (i > IIF) return;
	q += bsf * blockIdx.z; res += bsf * blockIdx.z; qc += bsc * blockIdx.z; // batch item (common.h Batch)
	const size_t sf = IIF, sc = IIC;
	const size_t x = (size_t)(i - 1) + sf * (size_t)(j - 1);
	const bool interior = i <= IIF - 1 && j <= JJF - 1;
	real_t r = 0.0;
	if (interior || (i <= imax && j <= jmax)) r = res[x];
	if (interior) {
		r = r / so_diag[x];
		res[x] = r;
	}
	if (i > imax || j > jmax) return;
	const bool io = i & 1, jo = j & 1;
	const int ic = io ? (i + 1) / 2 + 1 : i / 2 + 1, jc = jo ? (j + 1) / 2 + 1 : j / 2 + 1; // 1-based coarse
	const size_t c = (size_t)(ic - 1) + sc * (size_t)(jc - 1);
	const T *ci = W.p + (size_t)(ic - 1) + W.sj * (size_t)(jc - 1);
#define CIw(slot) (real_t) ci[(size_t)(slot)*W.ss]
	real_t v = q[x];
	if (!io && !jo) {
		v = v + qc[c];
	} else if (io && !jo) {
		real_t a = CIw(LR) * qc[c] + CIw(LL) * qc[c - 1];
		v = v + a + r;
	} else if (!io && jo) {
		real_t a = CIw(LA) * qc[c] + CIw(LB) * qc[c - sc];
		v = v + a + r;
	} else {
		real_t a = CIw(LSW) * qc[c - 1 - sc] + CIw(LNW) * qc[c - 1] + CIw(LNE) * qc[c] + CIw(LSE) * qc[c - sc];
		v = v + a + r;
	}
#undef CIw
	q[x] = v;
}

// ------------------------------------------------------------------ interp_add 3D
// One workgroup per fine row (j,k), lane p owns the pair of 1-based columns (2p+2, 2p+3): an even
// (coincides with / lies above a coarse column) and an odd one (between two coarse columns).  The
// (j,k) parities are uniform over the row, so every lane runs the same two formulas: no divergence,
// the fine arrays move as 16-byte pairs, the CI / coarse-q entries of a row as consecutive elements.
// Expressions and their evaluation order are those of BMG3_SymStd_interp_add.f90:88-240 (scatter in
// the reference, gathered per fine point here); the written index ranges -- including the ghost
// column / row / plane the reference touches for even extents -- are passed in by the host.
// The CI entries of a lane's pair: up to 4 for the even column, 8 for the odd one, by the (j,k) parity of the row.
template <class T> struct InterpCoef {
	T e[4], o[8];
};

// we: offset in the view of the even column's coarse point (the odd column's is we + 1)
template <bool KO, bool JO, class T>
__device__ __forceinline__ void interp_coef3(InterpCoef<T> &w, bool upd_e, bool upd_o, const CiW<T> &W, size_t we)
{
#define CIe(slot) W.p[(size_t)(slot)*W.ss + we]
#define CIo(slot) W.p[(size_t)(slot)*W.ss + we + 1]
	if (!KO) {
		if (!JO) {
			if (upd_o) { w.o[0] = CIo(LXYR); w.o[1] = CIo(LXYL); }
		} else {
			if (upd_e) { w.e[0] = CIe(LXYA); w.e[1] = CIe(LXYB); }
			if (upd_o) { w.o[0] = CIo(LXYSW); w.o[1] = CIo(LXYNW); w.o[2] = CIo(LXYNE); w.o[3] = CIo(LXYSE); }
		}
	} else {
		if (!JO) {
			if (upd_e) { w.e[0] = CIe(LXZA); w.e[1] = CIe(LXZB); }
			if (upd_o) { w.o[0] = CIo(LXZNW); w.o[1] = CIo(LXZNE); w.o[2] = CIo(LXZSW); w.o[3] = CIo(LXZSE); }
		} else {
			if (upd_e) { w.e[0] = CIe(LYZNW); w.e[1] = CIe(LYZNE); w.e[2] = CIe(LYZSW); w.e[3] = CIe(LYZSE); }
			if (upd_o) {
				w.o[0] = CIo(LTNW); w.o[1] = CIo(LTNE); w.o[2] = CIo(LTSW); w.o[3] = CIo(LTSE);
				w.o[4] = CIo(LBNW); w.o[5] = CIo(LBNE); w.o[6] = CIo(LBSW); w.o[7] = CIo(LBSE);
			}
		}
	}
#undef CIe
#undef CIo
}

template <bool KO, bool JO, class T>
__device__ __forceinline__ void interp_apply3(const InterpCoef<T> &w, real_t &ve, real_t &vo, real_t re, real_t ro, bool upd_e,
                                              bool upd_o, const real_t *__restrict__ qc, size_t ce, size_t sc, size_t tc)
{
	const size_t co = ce + 1;
#define E(n) (real_t) w.e[n]
#define O(n) (real_t) w.o[n]
	if (!KO) {
		if (!JO) {
			if (upd_e) ve = ve + qc[ce];
			if (upd_o) {
				real_t a = O(0) * qc[co] + O(1) * qc[co - 1];
				vo = vo + a + ro;
			}
		} else {
			if (upd_e) {
				real_t a = E(0) * qc[ce] + E(1) * qc[ce - sc];
				ve = ve + a + re;
			}
			if (upd_o) {
				real_t a = O(0) * qc[co - 1 - sc] + O(1) * qc[co - 1] + O(2) * qc[co] + O(3) * qc[co - sc];
				vo = vo + a + ro;
			}
		}
	} else {
		if (!JO) {
			if (upd_e) ve = ve + E(0) * qc[ce] + E(1) * qc[ce - tc] + re;
			if (upd_o) vo = vo + O(0) * qc[co - 1] + O(1) * qc[co] + O(2) * qc[co - 1 - tc] + O(3) * qc[co - tc] + ro;
		} else {
			if (upd_e) ve = ve + E(0) * qc[ce] + E(1) * qc[ce - sc] + E(2) * qc[ce - tc] + E(3) * qc[ce - sc - tc] + re;
			if (upd_o)
				vo = vo + O(0) * qc[co - 1] + O(1) * qc[co] + O(2) * qc[co - 1 - sc] + O(3) * qc[co - sc]
				     + O(4) * qc[co - 1 - tc] + O(5) * qc[co - tc] + O(6) * qc[co - 1 - sc - tc] + O(7) * qc[co - sc - tc] + ro;
		}
	}
#undef E
#undef O
}

// one fine row for one vector (nitems = 1, strides unused) or a batch: the weights and the two diagonal entries of a
// lane's pair stay in registers across the item loop
template <bool KO, bool JO, class T>
__device__ __forceinline__ void interp_add3_row(real_t *__restrict__ q, const real_t *__restrict__ qc,
                                                const real_t *__restrict__ so_diag, real_t *__restrict__ res, const CiW<T> &W,
                                                int IIF, size_t rowf, size_t rowc, size_t roww, size_t sc, size_t tc,
                                                bool row_in_range, bool row_interior, int imax_e, int imax_all, int nitems,
                                                size_t bsf, size_t bsc)
{
	for (int p = threadIdx.x; 2 * p + 2 <= IIF; p += blockDim.x) {
		const int ie = 2 * p + 2, io = ie + 1; // 1-based
		const bool have_o = io <= IIF;
		const size_t x = rowf + (size_t)(ie - 1);
		const bool int_e = row_interior && ie <= IIF - 1, int_o = row_interior && have_o && io <= IIF - 1;
		// written range of this plane type: even planes i in [2, imax_all] (all parities);
		// odd planes: even i up to imax_e, odd i up to imax_all-1
		const bool upd_e = row_in_range && (KO ? ie <= imax_e : ie <= imax_all);
		const bool upd_o = row_in_range && have_o && (KO ? io <= imax_all - 1 : io <= imax_all);
		if (!(int_e || int_o || upd_e || upd_o)) continue;
		real_t de = 1.0, dn = 1.0;
		if (have_o) {
			d2u t = *reinterpret_cast<const d2u *>(so_diag + x); de = t.x; dn = t.y;
		} else
			de = so_diag[x];
		const size_t ce = rowc + (size_t)(ie / 2); // 0-based: ic-1 = i/2
		InterpCoef<T> w;
		interp_coef3<KO, JO>(w, upd_e, upd_o, W, roww + (size_t)(ie / 2));
		for (int m = 0; m < nitems; m++) {
			real_t *qm = q + (size_t)m * bsf, *rm = res + (size_t)m * bsf;
			real_t re = 0.0, ro = 0.0, ve = 0.0, vo = 0.0;
			if (have_o) {
				d2u t = *reinterpret_cast<const d2u *>(rm + x); re = t.x; ro = t.y;
				t = *reinterpret_cast<const d2u *>(qm + x); ve = t.x; vo = t.y;
			} else {
				re = rm[x]; ve = qm[x];
			}
			if (int_e) re = re / de;
			if (int_o) ro = ro / dn;
			if (int_e && int_o) {
				d2u t; t.x = re; t.y = ro;
				*reinterpret_cast<d2u *>(rm + x) = t;
			} else {
				if (int_e) rm[x] = re;
				if (int_o) rm[x + 1] = ro;
			}
			if (!(upd_e || upd_o)) continue;
			interp_apply3<KO, JO>(w, ve, vo, re, ro, upd_e, upd_o, qc + (size_t)m * bsc, ce, sc, tc);
			if (upd_e && upd_o) {
				d2u t; t.x = ve; t.y = vo;
				*reinterpret_cast<d2u *>(qm + x) = t;
			} else {
				if (upd_e) qm[x] = ve;
				if (upd_o) qm[x + 1] = vo;
			}
		}
	}
}

// the rows of a launch: workgroup -> fine row (j,k), its parities and ranges, then the row body
template <class T>
__device__ __forceinline__ void interp_add3_rows(real_t *__restrict__ q, const real_t *__restrict__ qc,
                                                 const real_t *__restrict__ so_diag, real_t *__restrict__ res, const CiW<T> &W,
                                                 int IIC, int JJC, int KKC, int IIF, int JJF, int KKF, int imax_e, int imax_all,
                                                 int jmax, int kmax_e, int kmax_o, unsigned nrows, int nitems, size_t bsf,
                                                 size_t bsc)
{
	const unsigned L = xcd_remap(blockIdx.x, nrows);
	if (L >= nrows) return;
	const int j = (int)(L % (unsigned)(JJF - 1)) + 2, k = (int)(L / (unsigned)(JJF - 1)) + 2; // 1-based, 2..JJF / 2..KKF
	const size_t sf = IIF, tf = (size_t)IIF * JJF;
	const size_t sc = IIC, tc = (size_t)IIC * JJC;
	const bool jo = j & 1, ko = k & 1;
	const int jc = jo ? (j + 1) / 2 + 1 : j / 2 + 1, kc = ko ? (k + 1) / 2 + 1 : k / 2 + 1;
	const bool row_in_range = j <= jmax && k <= (ko ? kmax_o : kmax_e);
	const bool row_interior = j <= JJF - 1 && k <= KKF - 1;
	const size_t rowf = sf * (size_t)(j - 1) + tf * (size_t)(k - 1);
	const size_t rowc = sc * (size_t)(jc - 1) + tc * (size_t)(kc - 1);
	const size_t roww = W.sj * (size_t)(jc - 1) + W.sk * (size_t)(kc - 1);
#define ROW(KOv, JOv)                                                                                                       \
	interp_add3_row<KOv, JOv>(q, qc, so_diag, res, W, IIF, rowf, rowc, roww, sc, tc, row_in_range, row_interior, imax_e,    \
	                          imax_all, nitems, bsf, bsc)
	if (ko) {
		if (jo) ROW(true, true);
		else ROW(true, false);
	} else {
		if (jo) ROW(false, true);
		else ROW(false, false);
	}
#undef ROW
}

template <class T>
__global__ __launch_bounds__(256) void interp_add3_kernel(real_t *__restrict__ q, const real_t *__restrict__ qc,
                                                           const real_t *__restrict__ so_diag, real_t *__restrict__ res,
                                                           const CiW<T> W, int IIC, int JJC, int KKC, int IIF, int JJF, int KKF,
                                                           int imax_e, int imax_all, int jmax, int kmax_e, int kmax_o,
                                                           unsigned nrows)
{
	interp_add3_rows(q, qc, so_diag, res, W, IIC, JJC, KKC, IIF, JJF, KKF, imax_e, imax_all, jmax, kmax_e, kmax_o, nrows, 1, 0, 0);
}

template <class T>
__global__ __launch_bounds__(256) void interp_add3_many_kernel(real_t *__restrict__ q, const real_t *__restrict__ qc,
                                                                const real_t *__restrict__ so_diag, real_t *__restrict__ res,
                                                                const CiW<T> W, int IIC, int JJC, int KKC, int IIF, int JJF,
                                                                int KKF, int imax_e, int imax_all, int jmax, int kmax_e,
                                                                int kmax_o, unsigned nrows, int nitems, size_t bsf, size_t bsc)
{
	interp_add3_rows(q, qc, so_diag, res, W, IIC, JJC, KKC, IIF, JJF, KKF, imax_e, imax_all, jmax, kmax_e, kmax_o, nrows, nitems,
	                 bsf, bsc);
}

// the written index ranges of interp_add3 (BMG3_SymStd_interp_add.f90), shared by the launchers
struct InterpRanges3 {
	int imax_e, imax_all, jmax, kmax_e, kmax_o, bs;
	unsigned nrows;
};
static inline InterpRanges3 interp_ranges3(int IIC, int JJC, int KKC, int IIF, int JJF, int KKF)
{
	const int iicf1 = (IIF - 2) / 2 + 2, jjcf1 = (JJF - 2) / 2 + 2, kkcf1 = (KKF - 2) / 2 + 2;
	InterpRanges3 r;
	r.imax_all = 2 * (iicf1 - 1);   // even planes, and odd-i bound + 1 on odd planes
	r.imax_e = 2 * (IIC - 2);       // even i on odd planes: ic = 2..iic1
	r.jmax = 2 * (jjcf1 - 1);
	r.kmax_e = 2 * (KKC - 2);       // coarse planes kc = 2..kkc1
	r.kmax_o = 2 * (kkcf1 - 1) - 1; // odd planes kc = 3..kkcf1
	r.nrows = (unsigned)(JJF - 1) * (unsigned)(KKF - 1);
	r.bs = IIF / 2 >= 256 ? 256 : (IIF / 2 > 64 ? 128 : 64); // one lane per column pair
	(void)JJC;
	return r;
}

} // namespace cedar_amd
