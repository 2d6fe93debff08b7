// Device bodies of the 2D point-relaxed level's row kernels -- the nine-point row task with its LDS neighbour exchange
// and chunk carry, the band-fused walk, the partial-sum F and S tasks, the nine-point residual row and the five-point
// sum -- written once for two views of the operator:
//   Op2c  the FP64 Cedar planes of the boundary (relax2d.hip, residual.hip);
//   Op2f  the row-interleaved single-precision copy (common.h; op2f.hip).
// A view gives the start of a slot-row, row(slot, j), and of the 1/diag row, rd(j); an entry is promoted to double when
// it is loaded (exact), vectors and arithmetic are FP64 in the reference's term order.  So a kernel on Op2f has the bits
// of the same kernel on Op2c over the operator and 1/diag rounded to float.
#pragma once
#include "common.h"

namespace cedar_amd {

struct Op2c {
	const real_t *so, *sor;
	size_t sj, PS;
	__device__ __forceinline__ const real_t *row(int slot, size_t j) const { return so + (size_t)slot * PS + j * sj; }
	__device__ __forceinline__ const real_t *rd(size_t j) const { return sor + PS + j * sj; }
};
__host__ __device__ static inline Op2c op2_cedar(const real_t *so, const real_t *sor, int II, int JJ)
{
	return Op2c{so, sor, (size_t)II, (size_t)II * JJ};
}

struct C9 {
	real_t w, s, sw;        // stored at X:        kw, ks, ksw
	real_t s_n, nw_n;       // stored at X+(0,1):  ks, knw
	real_t w_e, nw_e;       // stored at X+(1,0):  kw, knw
	real_t sw_ne;           // stored at X+(1,1):  ksw
};

// qq[dj+1][di+1]; term order of BMG2_SymStd_relax_GS.f90:98-107 (= residual.f90:90-98)
__device__ __forceinline__ real_t offdiag9(real_t qf, const C9 &c, const real_t (&qq)[3][3])
{
	real_t s = qf;
	s = s + c.w * qq[1][0];
	s = s + c.w_e * qq[1][2];
	s = s + c.s * qq[0][1];
	s = s + c.s_n * qq[2][1];
	s = s + c.sw * qq[0][0];
	s = s + c.nw_e * qq[0][2];
	s = s + c.nw_n * qq[2][0];
	s = s + c.sw_ne * qq[2][2];
	return s;
}

__device__ __forceinline__ void ldpair2(const real_t *__restrict__ p, bool two, real_t &a, real_t &b)
{
	if (two) {
		d2u v = *reinterpret_cast<const d2u *>(p);
		a = v.x; b = v.y;
	} else {
		a = p[0]; b = 0.0;
	}
}
// the float view's pair: one 8-byte load, promoted
__device__ __forceinline__ void ldpair2(const float *__restrict__ p, bool two, real_t &a, real_t &b)
{
	if (two) {
		f2u v = *reinterpret_cast<const f2u *>(p);
		a = (real_t)v.x; b = (real_t)v.y;
	} else {
		a = (real_t)p[0]; b = 0.0;
	}
}

// all operands of the pair (ie, io) of grid row j (row = j * sj): pair loads; `two`: element io+1 inside the row
template <class V>
__device__ __forceinline__ void load_pair9(const V &A, const real_t *__restrict__ qf, const real_t *__restrict__ q, size_t j,
                                           size_t row, size_t sj, int ie, int io, bool two, C9 &ce, C9 &co,
                                           real_t (&qe)[3][3], real_t (&qo)[3][3], real_t &qfe, real_t &qfo)
{
	real_t a, b;
	ldpair2(A.row(KW, j) + ie, true, a, b); ce.w = a; co.w = b; ce.w_e = b;
	ldpair2(A.row(KS, j) + ie, true, a, b); ce.s = a; co.s = b;
	ldpair2(A.row(KSW, j) + ie, true, a, b); ce.sw = a; co.sw = b;
	ldpair2(A.row(KS, j + 1) + ie, true, a, b); ce.s_n = a; co.s_n = b;
	ldpair2(A.row(KNW, j + 1) + ie, true, a, b); ce.nw_n = a; co.nw_n = b;
	ldpair2(A.row(KNW, j) + io, two, a, b); ce.nw_e = a; co.nw_e = b;
	ldpair2(A.row(KSW, j + 1) + io, two, a, b); ce.sw_ne = a; co.sw_ne = b;
	co.w_e = two ? (real_t)A.row(KW, j)[io + 1] : 0.0;
	ldpair2(qf + row + ie, true, qfe, qfo);
#pragma unroll
	for (int dj = 0; dj < 3; dj++) {
		const real_t *r = q + row + (ptrdiff_t)(dj - 1) * (ptrdiff_t)sj;
		real_t w0, w1, w2, w3;
		ldpair2(r + ie - 1, true, w0, w1);
		ldpair2(r + io, two, w2, w3);
		qe[dj][0] = w0; qe[dj][1] = w1; qe[dj][2] = w2;
		qo[dj][0] = w1; qo[dj][1] = w2; qo[dj][2] = w3;
	}
}

// EFIRST: even 1-based i first (DOWN in 2D), else odd i first (UP).
// One workgroup per grid row; lane p of chunk c owns the pair (i_e,i_o) = (2P+2, 2P+3), P = c*BS+p.
// Within a chunk the fresh first-colour values reach the neighbouring lane through LDS; between
// chunks one value is carried: the chunks of a row are walked downwards for EFIRST (the last odd
// point of a chunk needs the first even point of the next chunk, already relaxed) and upwards
// otherwise.  In-place is safe: a launch writes rows of one parity only, and inside a row every
// value that a later chunk still has to read "old" has not been written yet.
template <int BS, bool EFIRST, class V>
__device__ __forceinline__ void relax9_row_task(const V &A, const real_t *__restrict__ qf, real_t *__restrict__ q, int II,
                                                size_t j, real_t *xch, real_t *carry_s)
{
	const size_t sj = II, row = j * sj;
	const int npairs = (II - 2 + 1) / 2;
	const int nchunks = (npairs + BS - 1) / BS;
	const int t = threadIdx.x;
	for (int cc = 0; cc < nchunks; cc++) {
		const int c = EFIRST ? nchunks - 1 - cc : cc;
		const int p = c * BS + t;
		const int ie = 2 * p + 1, io = ie + 1;
		const bool e_ok = ie <= II - 2, o_ok = io <= II - 2, two = io + 1 <= II - 1;
		C9 ce, co;
		real_t qe[3][3], qo[3][3], qfe = 0, qfo = 0, sre = 0, sro = 0, e_new = 0, o_new = 0;
		if (e_ok) {
			load_pair9(A, qf, q, j, row, sj, ie, io, two, ce, co, qe, qo, qfe, qfo);
			ldpair2(A.rd(j) + ie, true, sre, sro);
		}
		const real_t carry = *carry_s; // written by the previous chunk iteration (unused in the first)
		if (EFIRST) {
			if (e_ok) { e_new = offdiag9(qfe, ce, qe) * sre; xch[t] = e_new; }
			__syncthreads();
			if (o_ok) {
				qo[1][0] = e_new;
				if (io + 1 <= II - 2) qo[1][2] = (t < BS - 1) ? xch[t + 1] : carry; // next pair's fresh even point
				o_new = offdiag9(qfo, co, qo) * sro;
			}
			if (t == 0) *carry_s = e_new; // first even point of this chunk, for the chunk below
		} else {
			if (o_ok) { o_new = offdiag9(qfo, co, qo) * sro; xch[t + 1] = o_new; }
			__syncthreads();
			if (e_ok) {
				if (p > 0) qe[1][0] = (t > 0) ? xch[t] : carry; // previous pair's fresh odd point
				if (o_ok) qe[1][2] = o_new;
				e_new = offdiag9(qfe, ce, qe) * sre;
			}
			if (t == BS - 1) *carry_s = o_new;
		}
		if (e_ok) {
			if (o_ok) {
				d2u v; v.x = e_new; v.y = o_new;
				*reinterpret_cast<d2u *>(q + row + ie) = v;
			} else
				q[row + ie] = e_new;
		}
		__syncthreads(); // stores + carry visible before the next chunk loads / reads them
	}
}

// Band-fused sweep: both row classes in ONE launch.  The sweep relaxes the rows of class F (parity jbF) before those
// of class S; an S row reads the fresh values of its two F neighbours and nothing else changes under it.  A workgroup
// owns a run of consecutive F rows [f0, f1) and walks F(f0), F(f0+1), S between them, F(f0+2), S, ...: the three
// operator rows both classes need (ks, ksw, knw of the upper row: 3 of the 8 slot-rows a row task reads) and the q rows
// are used again one task later instead of being streamed once per launch.  The S row between two runs has its F
// neighbours in different workgroups and is left to a small second launch (the rows kernel, jstep = 2*frun).  Same
// arithmetic per point on the same values => identical to the two-launch order.  (2D analogue of relax27_plane.)
template <int BS, bool EFIRST, class V>
__device__ __forceinline__ void relax9_band_body(const V &A, const real_t *__restrict__ qf, real_t *__restrict__ q, int II,
                                                 int JJ, int jbF, int frun, int run, real_t *xch, real_t *carry_s)
{
	const int nF = (JJ - 2 - jbF + 1) / 2, nS = (JJ - 2 - (1 - jbF) + 1) / 2;
	const int f0 = run * frun, f1 = min(nF, f0 + frun);
	for (int f = f0; f < f1; f++) {
		relax9_row_task<BS, EFIRST>(A, qf, q, II, (size_t)(1 + jbF + 2 * f), xch, carry_s);
		// the S row both of whose F neighbours are now done (a missing neighbour = ghost row):
		//   jbF = 0: S row g (j = 2+2g) lies between F rows g, g+1  -> after F(f): g = f-1 (f > f0)
		//   jbF = 1: S row g (j = 1+2g) lies between F rows g-1, g  -> after F(f): g = f   (f > f0, or f = 0)
		const int g = jbF ? f : f - 1;
		const bool have = jbF ? (f > f0 || f == 0) : (f > f0);
		if (have && g >= 0 && g < nS) // (the row task ends with a barrier: the F stores are visible)
			relax9_row_task<BS, EFIRST>(A, qf, q, II, (size_t)(2 - jbF + 2 * g), xch, carry_s);
	}
	if (f1 == nF && f1 > f0) { // the S row beyond the last F row (its other neighbour is the ghost row)
		const int g = jbF ? nF : nF - 1;
		if (g < nS) relax9_row_task<BS, EFIRST>(A, qf, q, II, (size_t)(2 - jbF + 2 * g), xch, carry_s);
	}
}

// ------------------------------------------------------------------ band-fused sweep with inter-row partial sums
// The 2D analogue of relax3d_psum.hip, with the partial sums kept in LDS.  north_star's contract (histories within 1e-10),
// not bit for bit: BMG2_SymStd_relax_GS stays on the reference order (relax2_gs).
// An S row reads, besides its own row, the three operator rows (ks, ksw, knw) that couple it to the F row below and the
// three that couple it to the F row above -- rows the two F tasks of the same workgroup have just streamed for their own
// updates -- plus the two fresh F rows.  Here each F task multiplies its fresh values with those coefficients while it
// holds them in registers and adds the products into an LDS row T of the S row above / below (position-wise: own column,
// then the column to the right, then to the left, a barrier between the three so that every T entry has one writer at a
// time and a fixed order of additions); the S task between two F rows of the run then computes
//     q = (qf + w q(i-1) + w_e q(i+1) + T) / diag
// from ONE operator row (kw), 1/diag, qf and its own row: 5 row streams instead of 14.  S rows whose two F neighbours do
// not both belong to the run (rows between runs: second small launch; row 1 / the row beyond the last F row: in place) keep
// the reference order.  LDS: two T rows of II doubles (the S row being filled and the one being consumed).
template <int BS, bool EFIRST, class V>
__device__ __forceinline__ void relax9_row_task_F(const V &A, const real_t *__restrict__ qf, real_t *__restrict__ q, int II,
                                                  size_t j, real_t *xch, real_t *carry_s, real_t *Tup, real_t *Tdn)
{
	const size_t sj = II, row = j * sj;
	const int npairs = (II - 2 + 1) / 2;
	const int nchunks = (npairs + BS - 1) / BS;
	const int t = threadIdx.x;
	if (Tup) { // this F row is the first contributor of the S row above: start its sums from zero
		for (int i = t; i < II; i += BS) Tup[i] = 0.0;
		__syncthreads();
	}
	for (int cc = 0; cc < nchunks; cc++) {
		const int c = EFIRST ? nchunks - 1 - cc : cc;
		const int p = c * BS + t;
		const int ie = 2 * p + 1, io = ie + 1;
		const bool e_ok = ie <= II - 2, o_ok = io <= II - 2, two = io + 1 <= II - 1;
		C9 ce, co;
		real_t qe[3][3], qo[3][3], qfe = 0, qfo = 0, sre = 0, sro = 0, e_new = 0, o_new = 0;
		if (e_ok) {
			load_pair9(A, qf, q, j, row, sj, ie, io, two, ce, co, qe, qo, qfe, qfo);
			ldpair2(A.rd(j) + ie, true, sre, sro);
		}
		const real_t ghostL = qe[1][0], ghostR = o_ok ? qo[1][2] : qe[1][2]; // old values of the ghost columns (p = 0 / last lane)
		const real_t carry = *carry_s;
		if (EFIRST) {
			if (e_ok) { e_new = offdiag9(qfe, ce, qe) * sre; xch[t] = e_new; }
			__syncthreads();
			if (o_ok) {
				qo[1][0] = e_new;
				if (io + 1 <= II - 2) qo[1][2] = (t < BS - 1) ? xch[t + 1] : carry;
				o_new = offdiag9(qfo, co, qo) * sro;
			}
			if (t == 0) *carry_s = e_new;
		} else {
			if (o_ok) { o_new = offdiag9(qfo, co, qo) * sro; xch[t + 1] = o_new; }
			__syncthreads();
			if (e_ok) {
				if (p > 0) qe[1][0] = (t > 0) ? xch[t] : carry;
				if (o_ok) qe[1][2] = o_new;
				e_new = offdiag9(qfe, ce, qe) * sre;
			}
			if (t == BS - 1) *carry_s = o_new;
		}
		if (e_ok) {
			if (o_ok) {
				d2u v; v.x = e_new; v.y = o_new;
				*reinterpret_cast<d2u *>(q + row + ie) = v;
			} else
				q[row + ie] = e_new;
		}
		// ---- contributions of this chunk's sources to the S rows above (Tup) and below (Tdn).  Sources: e, o (fresh); the
		// right ghost column as `o` when the row ends on e (old value, only its contribution to the left counts); the left
		// ghost column with lane p = 0, the right one with the lane of the last interior point when that is an o.
		const real_t so_v = o_ok ? o_new : ghostR;
		const bool o_src = o_ok || (e_ok && io == II - 1);
		if (e_ok) { // own column
			if (Tup) { Tup[ie] += e_new * ce.s_n; if (o_ok) Tup[io] += o_new * co.s_n; }
			if (Tdn) { Tdn[ie] += e_new * ce.s; if (o_ok) Tdn[io] += o_new * co.s; }
		}
		__syncthreads();
		if (e_ok) { // the column to the right of each source (targets io and io+1; lane 0 also: ghost column 0 -> column 1)
			if (Tup) {
				if (o_ok) Tup[io] += e_new * ce.sw_ne;
				if (o_ok && io + 1 <= II - 2) Tup[io + 1] += o_new * co.sw_ne;
				if (p == 0) Tup[1] += ghostL * (real_t)A.row(KSW, j + 1)[1];
			}
			if (Tdn) {
				if (o_ok) Tdn[io] += e_new * ce.nw_e;
				if (o_ok && io + 1 <= II - 2) Tdn[io + 1] += o_new * co.nw_e;
				if (p == 0) Tdn[1] += ghostL * (real_t)A.row(KNW, j)[1];
			}
		}
		__syncthreads();
		if (e_ok) { // the column to the left of each source (targets ie-1 and ie; the last lane also: ghost column II-1 -> II-2)
			if (Tup) {
				if (ie - 1 >= 1) Tup[ie - 1] += e_new * ce.nw_n;
				if (o_src) Tup[ie] += so_v * co.nw_n;
				if (o_ok && io == II - 2) Tup[io] += ghostR * (real_t)A.row(KNW, j + 1)[II - 1];
			}
			if (Tdn) {
				if (ie - 1 >= 1) Tdn[ie - 1] += e_new * ce.sw;
				if (o_src) Tdn[ie] += so_v * co.sw;
				if (o_ok && io == II - 2) Tdn[io] += ghostR * (real_t)A.row(KSW, j)[II - 1];
			}
		}
		__syncthreads(); // stores, carry and sums visible before the next chunk
	}
}

// S row from its partial sums: term order qf, w, w_e (relax_GS.f90:98-99), then T
template <int BS, bool EFIRST, class V>
__device__ __forceinline__ void relax9_row_task_S(const V &A, const real_t *__restrict__ qf, real_t *__restrict__ q, int II,
                                                  size_t j, real_t *xch, real_t *carry_s, const real_t *T)
{
	const size_t row = j * (size_t)II;
	const int npairs = (II - 2 + 1) / 2;
	const int nchunks = (npairs + BS - 1) / BS;
	const int t = threadIdx.x;
	for (int cc = 0; cc < nchunks; cc++) {
		const int c = EFIRST ? nchunks - 1 - cc : cc;
		const int p = c * BS + t;
		const int ie = 2 * p + 1, io = ie + 1;
		const bool e_ok = ie <= II - 2, o_ok = io <= II - 2, two = io + 1 <= II - 1;
		real_t we = 0, wo = 0, wee = 0, weo = 0, qfe = 0, qfo = 0, sre = 0, sro = 0, e_new = 0, o_new = 0;
		real_t w0 = 0, w1 = 0, w2 = 0, w3 = 0, te = 0, to = 0;
		if (e_ok) {
			ldpair2(A.row(KW, j) + ie, true, we, wo);
			wee = wo;
			weo = two ? (real_t)A.row(KW, j)[io + 1] : 0.0;
			ldpair2(qf + row + ie, true, qfe, qfo);
			ldpair2(A.rd(j) + ie, true, sre, sro);
			ldpair2(q + row + ie - 1, true, w0, w1);
			ldpair2(q + row + io, two, w2, w3);
			te = T[ie];
			to = o_ok ? T[io] : 0.0;
		}
		const real_t carry = *carry_s;
		if (EFIRST) {
			if (e_ok) { e_new = (((qfe + we * w0) + wee * w2) + te) * sre; xch[t] = e_new; }
			__syncthreads();
			if (o_ok) {
				real_t east = w3;
				if (io + 1 <= II - 2) east = (t < BS - 1) ? xch[t + 1] : carry;
				o_new = (((qfo + wo * e_new) + weo * east) + to) * sro;
			}
			if (t == 0) *carry_s = e_new;
		} else {
			if (o_ok) { o_new = (((qfo + wo * w1) + weo * w3) + to) * sro; xch[t + 1] = o_new; }
			__syncthreads();
			if (e_ok) {
				real_t west = w0;
				if (p > 0) west = (t > 0) ? xch[t] : carry;
				e_new = (((qfe + we * west) + wee * (o_ok ? o_new : w2)) + te) * sre;
			}
			if (t == BS - 1) *carry_s = o_new;
		}
		if (e_ok) {
			if (o_ok) {
				d2u v; v.x = e_new; v.y = o_new;
				*reinterpret_cast<d2u *>(q + row + ie) = v;
			} else
				q[row + ie] = e_new;
		}
		__syncthreads();
	}
}

// the walk of one run of the partial-sum sweep; T0 / T1: two LDS rows of II doubles
template <int BS, bool EFIRST, class V>
__device__ __forceinline__ void relax9_band_psum_body(const V &A, const real_t *__restrict__ qf, real_t *__restrict__ q, int II,
                                                      int JJ, int jbF, int frun, int run, real_t *T0, real_t *T1, real_t *xch,
                                                      real_t *carry_s)
{
	const int nF = (JJ - 2 - jbF + 1) / 2, nS = (JJ - 2 - (1 - jbF) + 1) / 2;
	const int f0 = run * frun, f1 = min(nF, f0 + frun);
	for (int f = f0; f < f1; f++) {
		// F(f) starts the sums of the S row between F(f) and F(f+1) (slot f & 1) and completes those of the S row between
		// F(f-1) and F(f) (slot (f-1) & 1), when that neighbour belongs to the run
		real_t *Tup = f + 1 <= f1 - 1 ? ((f & 1) ? T1 : T0) : nullptr;
		real_t *Tdn = f - 1 >= f0 ? (((f - 1) & 1) ? T1 : T0) : nullptr;
		relax9_row_task_F<BS, EFIRST>(A, qf, q, II, (size_t)(1 + jbF + 2 * f), xch, carry_s, Tup, Tdn);
		const int g = jbF ? f : f - 1;
		const bool have = jbF ? (f > f0 || f == 0) : (f > f0);
		if (have && g >= 0 && g < nS) {
			const size_t jS = (size_t)(2 - jbF + 2 * g);
			if (f > f0) relax9_row_task_S<BS, EFIRST>(A, qf, q, II, jS, xch, carry_s, ((f - 1) & 1) ? T1 : T0);
			else relax9_row_task<BS, EFIRST>(A, qf, q, II, jS, xch, carry_s); // row 1 below the first F row (jbF = 1)
		}
	}
	if (f1 == nF && f1 > f0) { // the S row beyond the last F row (its other neighbour is the ghost row): reference order
		const int g = jbF ? nF : nF - 1;
		if (g < nS) relax9_row_task<BS, EFIRST>(A, qf, q, II, (size_t)(2 - jbF + 2 * g), xch, carry_s);
	}
}

// 9-point residual of grid row j, pair per lane (BMG2_SymStd_residual.f90:88-99)
template <class V>
__device__ __forceinline__ void residual9_row_body(const V &A, const real_t *__restrict__ qf, const real_t *__restrict__ q,
                                                   real_t *__restrict__ res, int II, size_t j)
{
	const size_t sj = II, row = j * sj;
	for (int p = threadIdx.x; 2 * p + 1 <= II - 2; p += blockDim.x) {
		const int ie = 2 * p + 1, io = ie + 1;
		const bool o_ok = io <= II - 2, two = io + 1 <= II - 1;
		C9 ce, co;
		real_t qe[3][3], qo[3][3], qfe, qfo, de, dn;
		load_pair9(A, qf, q, j, row, sj, ie, io, two, ce, co, qe, qo, qfe, qfo);
		ldpair2(A.row(KO, j) + ie, true, de, dn);
		const real_t re = offdiag9(qfe, ce, qe) - de * qe[1][1];
		if (o_ok) {
			const real_t ro = offdiag9(qfo, co, qo) - dn * qo[1][1];
			d2u v; v.x = re; v.y = ro;
			*reinterpret_cast<d2u *>(res + row + ie) = v;
		} else
			res[row + ie] = re;
	}
}

// five-point: qf + the four off-diagonal terms of point (i, j), x = i + j * sj (relax_GS.f90:120-135, residual.f90:104-113)
template <class V>
__device__ __forceinline__ real_t offdiag5(const V &A, const real_t *__restrict__ qf, const real_t *__restrict__ q, int i,
                                           size_t j, size_t x, size_t sj)
{
	real_t s = qf[x];
	s = s + (real_t)A.row(KW, j)[i] * q[x - 1];
	s = s + (real_t)A.row(KW, j)[i + 1] * q[x + 1];
	s = s + (real_t)A.row(KS, j)[i] * q[x - sj];
	s = s + (real_t)A.row(KS, j + 1)[i] * q[x + sj];
	return s;
}

// run lengths of the band-fused and the partial-sum sweep (relax2d.hip): 0 = two row-class launches / reference order
int band_frun(int II, int JJ);
int band_psum_frun(int II, int JJ);

} // namespace cedar_amd
