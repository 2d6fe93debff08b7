// Zebra line relaxation in 2D (x- and y-lines) and its factorisation set-up.
// Replaces BMG2_SymStd_SETUP_lines_x/_y (src/2d/ftn/BMG2_SymStd_SETUP_lines_x.f90:68-87,
// ..._y.f90:69-87), BMG2_SymStd_relax_lines_x (..._relax_lines_x.f90:82-162) and
// BMG2_SymStd_relax_lines_y (..._relax_lines_y.f90:77-168), plus the LAPACK
// calls inside them (DPTTRF / DPTTRS; system LAPACK in the reference, not
// vendored -- the published netlib recurrences are restated here:
//   factor: e_i <- e_i/d_i ; d_{i+1} <- d_{i+1} - e_i*(e_i d_i)
//   solve : b_i <- b_i - b_{i-1} e_{i-1} ;  b_n <- b_n/d_n ; b_i <- b_i/d_i - b_{i+1} e_i ).
//
// Set-up (once per solve): one lane per line runs the DPTTRF recurrence
// sequentially in the reference's operation order => bit-identical factors.
//
// Relaxation (hot path, 64 algorithmic B/DOF per direction): all lines of one
// colour are independent.  One workgroup owns one line held in LDS (<= 64 KB);
// both DPTTRS sweeps are first-order affine recurrences y_i = a_i y_{i-1} + c_i.
// Every lane owns 8 consecutive unknowns (sequential, reference order); the
// lanes' composite maps are combined with a Kogge-Stone scan over wavefront
// shuffles, a 4-entry cross-wave fix-up in LDS and a scalar carry between
// tiles of 2048 unknowns.  The scan re-associates the recurrence, so
// results agree with the sequential DPTTRS to rounding (like one vendor LAPACK
// against another), not bit-for-bit; tolerances are stated in tests/.
// y-lines are strided in memory: their right-hand sides are gathered through
// an LDS tile transpose into a line-contiguous scratch (the same transposed
// layout the reference uses for the y factors, SOR(JJ,II,2)), solved by the
// same kernel, and scattered back.
#include "common.h"
#include "lines_dev.h"

namespace cedar_amd {

// ------------------------------------------------------------------ set-up
__global__ void lines_fill_x(const real_t *__restrict__ so, real_t *__restrict__ sor, int II, int JJ)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x + 1, j = blockIdx.y + 1;
	if (i > II - 2) return;
	const size_t PS = (size_t)II * JJ, x = (size_t)i + (size_t)II * j;
	sor[PS + x] = -so[KW * PS + x];
	sor[x] = so[KO * PS + x];
}

__global__ void lines_fill_y(const real_t *__restrict__ so, real_t *__restrict__ sor, int II, int JJ)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x + 1, j = blockIdx.y + 1;
	if (i > II - 2) return;
	const size_t PS = (size_t)II * JJ, x = (size_t)i + (size_t)II * j;
	const size_t xt = (size_t)j + (size_t)JJ * i; // SOR(JJ,II,2)
	sor[PS + xt] = -so[KS * PS + x];
	sor[xt] = so[KO * PS + x];
}

// one lane per line; d = sor(:,line,1) from index 1 (0-based), e = sor(:,line,2) from index 2
__global__ void lines_factor(real_t *__restrict__ sor, int n /*unknowns*/, int ld /*line stride*/, int nlines, size_t PS)
{
	const int l = blockIdx.x * blockDim.x + threadIdx.x;
	if (l >= nlines) return;
	real_t *d = sor + (size_t)ld * (l + 1) + 1;
	real_t *e = sor + PS + (size_t)ld * (l + 1) + 2;
	real_t di = d[0];
	for (int i = 0; i < n - 1; i++) {
		if (di <= 0.0) return; // DPTTRF: INFO = i+1, factorisation stops
		const real_t ei = e[i];
		const real_t en = ei / di;
		e[i] = en;
		di = d[i + 1] - en * ei;
		d[i + 1] = di;
	}
}

// periodic lines: the wrap-around coupling is folded into the two end diagonals before the
// factorisation (SETUP_lines_x.f90:76-83, SETUP_lines_y.f90:78-85); the solves undo it with a
// Sherman-Morrison correction (relax_lines_x.f90:209-226)
__global__ void lines_fold_x(const real_t *__restrict__ so, real_t *__restrict__ sor, int II, int JJ)
{
	const int j = blockIdx.x * blockDim.x + threadIdx.x + 1; // 0-based interior row
	if (j > JJ - 2) return;
	const size_t PS = (size_t)II * JJ, r = (size_t)II * j;
	sor[r + 1] = sor[r + 1] + so[KW * PS + r + 1];
	sor[r + II - 2] = sor[r + II - 2] + so[KW * PS + r + II - 1];
}

__global__ void lines_fold_y(const real_t *__restrict__ so, real_t *__restrict__ sor, int II, int JJ)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x + 1;
	if (i > II - 2) return;
	const size_t PS = (size_t)II * JJ, c = (size_t)JJ * i; // SOR(JJ,II,2): column i
	sor[c + 1] = sor[c + 1] + so[KS * PS + (size_t)i + (size_t)II];
	sor[c + JJ - 2] = sor[c + JJ - 2] + so[KS * PS + (size_t)i + (size_t)II * (JJ - 1)];
}

void setup_lines_x(const real_t *so, real_t *sor, int II, int JJ, hipStream_t st, int fold)
{
	if (II < 3 || JJ < 3) return;
	dim3 grid((II - 2 + 255) / 256, JJ - 2);
	hipLaunchKernelGGL(lines_fill_x, grid, dim3(256), 0, st, so, sor, II, JJ);
	if (fold) hipLaunchKernelGGL(lines_fold_x, dim3((JJ - 2 + 63) / 64), dim3(64), 0, st, so, sor, II, JJ);
	hipLaunchKernelGGL(lines_factor, dim3((JJ - 2 + 63) / 64), dim3(64), 0, st, sor, II - 2, II, JJ - 2, (size_t)II * JJ);
}

void setup_lines_y(const real_t *so, real_t *sor, int II, int JJ, hipStream_t st, int fold)
{
	if (II < 3 || JJ < 3) return;
	dim3 grid((II - 2 + 255) / 256, JJ - 2);
	hipLaunchKernelGGL(lines_fill_y, grid, dim3(256), 0, st, so, sor, II, JJ);
	if (fold) hipLaunchKernelGGL(lines_fold_y, dim3((II - 2 + 63) / 64), dim3(64), 0, st, so, sor, II, JJ);
	hipLaunchKernelGGL(lines_factor, dim3((II - 2 + 63) / 64), dim3(64), 0, st, sor, JJ - 2, JJ, II - 2, (size_t)II * JJ);
}

// ------------------------------------------------------------------ line solves
// The affine scan, both DPTTRS forms, the right-hand-side formation, the x-line kernel and its launchers are in
// lines_dev.h, shared with the single-precision instantiations of linesf.hip; this file instantiates the FP64 forms.

// Generic first-order recurrence over line-contiguous data, one workgroup per line:
//   forward  (reverse = 0): y_i = a_i * y_{i-1} + c_i,  i = 0..n-1,   y_{-1} = 0
//   backward (reverse = 1): y_i = a_i * y_{i+1} + c_i,  i = n-1..0,   y_n    = 0
// with c_i = y_i on entry, divided by div_i when div != nullptr.  The two sweeps of DPTTRS are the cases
// (a = -e', div = nullptr) and (a = -e'_next, div = d', reverse); the domain-decomposed line relaxation
// (cedar_amd/dist2d.py) runs them per segment and joins the segments' carries across ranks.
template <int BS>
__global__ __launch_bounds__(BS) void affine_lines_kernel(real_t *__restrict__ y, const real_t *__restrict__ a,
                                                           const real_t *__restrict__ div, int n, int ld, int reverse)
{
	__shared__ real_t wa[4], wc[4], cs;
	real_t *line = y + (size_t)blockIdx.x * ld;
	const real_t *al = a + (size_t)blockIdx.x * ld;
	const real_t *dl = div ? div + (size_t)blockIdx.x * ld : nullptr;
	real_t carry = 0.0;
	for (int base = 0; base < n; base += BS * CH) {
		const int r0 = base + (int)threadIdx.x * CH;
		real_t am[CH], cm[CH];
#pragma unroll
		for (int m = 0; m < CH; m++) {
			const int r = r0 + m, i = reverse ? n - 1 - r : r;
			if (r < n) { cm[m] = dl ? line[i] / dl[i] : line[i]; am[m] = al[i]; }
			else { cm[m] = 0.0; am[m] = 0.0; }
		}
		real_t A = 1.0, Cc = 0.0;
#pragma unroll
		for (int m = 0; m < CH; m++) { Cc = am[m] * Cc + cm[m]; A = am[m] * A; }
		real_t v, last;
		affine_scan<BS>(A, Cc, carry, wa, wc, v, last);
#pragma unroll
		for (int m = 0; m < CH; m++) {
			v = am[m] * v + cm[m];
			const int r = r0 + m;
			if (r < n) line[reverse ? n - 1 - r : r] = v;
		}
		if (threadIdx.x == BS - 1) cs = last;
		__syncthreads();
		carry = cs;
		__syncthreads();
	}
}

void affine_lines(real_t *y, const real_t *a, const real_t *div, int nlines, int n, int ld, int reverse, hipStream_t st)
{
	if (nlines <= 0 || n <= 0) return;
	if (n <= 512) hipLaunchKernelGGL(affine_lines_kernel<64>, dim3(nlines), dim3(64), 0, st, y, a, div, n, ld, reverse);
	else hipLaunchKernelGGL(affine_lines_kernel<256>, dim3(nlines), dim3(256), 0, st, y, a, div, n, ld, reverse);
}

// ipn: 0 Dirichlet; 1 periodic in y only: ordinary solves, one y wrap after the sweep (relax_lines_x.f90:75-176);
// 2 / 3 periodic in x (/ and y): cyclic lines, y then x wrap after each colour (:178-300)
// scan-ordered factor copy for the lines of `sor` (n unknowns per line, line stride ld, nlines lines): 0 doubles when
// the line kernel would not use it (lines of at most 512 unknowns run on one wavefront)
size_t lines_permuted_doubles(int n, int nlines)
{
	switch (line_bs(n)) {
	case 256: return pf_line_doubles<256>(n) * (size_t)nlines;
	case 512: return pf_line_doubles<512>(n) * (size_t)nlines;
	case 1024: return pf_line_doubles<1024>(n) * (size_t)nlines;
	default: return 0;
	}
}

bool line_fits_lds_host(int n) { return line_fits_lds(n); }

void lines_permute(const real_t *sor, real_t *pf, int n, int ld, int nlines, size_t PS, hipStream_t st)
{
	lines_permute_t<real_t>(sor, pf, n, ld, nlines, PS, nullptr, st);
}

void relax_lines_x(const real_t *so, const real_t *qf, real_t *q, const real_t *sor,
                   int II, int JJ, int nstncl, int updown, hipStream_t st, int ipn, const real_t *pf, Batch bt)
{
	if (II < 3 || JJ < 3) return;
	if (!lds_ok(II - 2, "relax_lines_x")) return;
	const bool sm = per_dirs(2, ipn).x;
	for (int c = 0; c < 2; c++) {
		// DOWN: lines J = 3,5,.. first (0-based rows 2,4,.. => jb = 1), then J = 2,4,..
		int jb = (updown == BMG_DOWN) ? 1 - c : c;
		launch_x(op2_cedar(so, nullptr, II, JJ), qf, q, sor, II, JJ, nstncl, jb, st, sm, false, sm ? nullptr : pf, bt);
		if (sm) wrap2(q, II, JJ, bt.n, ipn == 3, 1, st); // (a batch: every item is a plane of the wrap)
	}
	if (ipn == 1) wrap2(q, II, JJ, bt.n, 1, 0, st);
}

// ------------------------------------------------------------------ y-lines
// gather: bt[l*ldt + (j-1)] = rhs(i_l, j) for the colour's lines i_l = 1+ib+2l (0-based), j = 1..JJ-2
template <bool NINE>
__global__ __launch_bounds__(256) void ylines_rhs_T(const real_t *__restrict__ so, const real_t *__restrict__ qf,
                                                     const real_t *__restrict__ q, real_t *__restrict__ bt,
                                                     int II, int JJ, int ib, int nlines, int ldt, int lofs)
{
	__shared__ real_t tile[32][33];
	const int l0 = blockIdx.x * 32, j0 = blockIdx.y * 32; // tile origin (line index within the chunk, j-1)
	const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5; // 32 x 8
	const size_t sj = II, PS = (size_t)II * JJ;
	for (int r = ty; r < 32; r += 8) {
		const int l = l0 + tx, j = j0 + r + 1;
		real_t s = 0.0;
		if (l < nlines && j <= JJ - 2) {
			const size_t x = (size_t)(1 + ib + 2 * (lofs + l)) + sj * (size_t)j;
			// relax_lines_y.f90:103-107 / :133-134, reference term order
			s = qf[x];
			s = s + so[KW * PS + x] * q[x - 1];
			s = s + so[KW * PS + x + 1] * q[x + 1];
			if (NINE) {
				s = s + so[KSW * PS + x] * q[x - 1 - sj];
				s = s + so[KNW * PS + x + 1] * q[x + 1 - sj];
				s = s + so[KNW * PS + x + sj] * q[x - 1 + sj];
				s = s + so[KSW * PS + x + 1 + sj] * q[x + 1 + sj];
			}
		}
		tile[r][tx] = s;
	}
	__syncthreads();
	for (int r = ty; r < 32; r += 8) {
		const int l = l0 + r, jj = j0 + tx; // jj = j-1
		if (l < nlines && jj < JJ - 2) bt[(size_t)l * ldt + jj] = tile[tx][r];
	}
}

template <int BS, bool SM = false>
__global__ __launch_bounds__(BS) void ylines_solve(real_t *__restrict__ bt, const real_t *__restrict__ sor,
                                                    int II, int JJ, int ib, int nlines, int ldt,
                                                    const real_t *__restrict__ so, int lofs)
{
	extern __shared__ __attribute__((aligned(16))) real_t lds[];
	const int n = JJ - 2;
	const int npad = n + (n >> 3) + 1;
	real_t *y = lds, *wa = lds + npad, *wc = wa + 16, *cs = wc + 16;
	const unsigned L = blockIdx.x;
	if (L >= (unsigned)nlines) return;
	const size_t PS = (size_t)II * JJ;
	const int i = 1 + ib + 2 * (lofs + (int)L); // 0-based line position
	real_t *line = bt + (size_t)L * ldt;
	for (int t = threadIdx.x; t < n; t += BS) y[lpad(t)] = line[t];
	__syncthreads();
	// SOR(JJ,II,2): d = SOR(2.., i) , e = SOR(3.., i, 2)
	line_pttrs<BS>(y, n, sor + (size_t)JJ * i + 1, sor + PS + (size_t)JJ * i + 2, wa, wc, cs);
	for (int t = threadIdx.x; t < n; t += BS) line[t] = y[lpad(t)];
	if (SM) { // relax_lines_y.f90:196-207: u = -SO(I,2,KS) e_first - SO(I,JJ,KS) e_last
		real_t y1, yn;
		const real_t beta = line_sherman_morrison<BS>(y, n, sor + (size_t)JJ * i + 1, sor + PS + (size_t)JJ * i + 2,
		                                              so[KS * PS + (size_t)i + (size_t)II], so[KS * PS + (size_t)i + (size_t)II * (JJ - 1)],
		                                              wa, wc, cs, y1, yn);
		for (int t = threadIdx.x; t < n; t += BS) line[t] = line[t] - beta * y[lpad(t)];
	}
}

__global__ __launch_bounds__(256) void ylines_scatter_T(const real_t *__restrict__ bt, real_t *__restrict__ q,
                                                         int II, int JJ, int ib, int nlines, int ldt, int lofs)
{
	__shared__ real_t tile[32][33];
	const int l0 = blockIdx.x * 32, j0 = blockIdx.y * 32;
	const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
	for (int r = ty; r < 32; r += 8) {
		const int l = l0 + r, jj = j0 + tx;
		tile[r][tx] = (l < nlines && jj < JJ - 2) ? bt[(size_t)l * ldt + jj] : 0.0;
	}
	__syncthreads();
	for (int r = ty; r < 32; r += 8) {
		const int l = l0 + tx, j = j0 + r + 1;
		if (l < nlines && j <= JJ - 2) q[(size_t)(1 + ib + 2 * (lofs + l)) + (size_t)II * j] = tile[tx][r];
	}
}

template <int BS>
static void launch_ysolve_n(real_t *bt, const real_t *sor, int II, int JJ, int ib, int nlines, int ldt, const real_t *so,
                            int lofs, size_t shm, bool sm, hipStream_t st)
{
	if (sm) {
		auto k = ylines_solve<BS, true>;
		if (shm > 64 * 1024) CEDAR_HIP_CHECK(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
		hipLaunchKernelGGL(k, dim3(nlines), dim3(BS), shm, st, bt, sor, II, JJ, ib, nlines, ldt, so, lofs);
	} else {
		auto k = ylines_solve<BS, false>;
		if (shm > 64 * 1024) CEDAR_HIP_CHECK(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
		hipLaunchKernelGGL(k, dim3(nlines), dim3(BS), shm, st, bt, sor, II, JJ, ib, nlines, ldt, so, lofs);
	}
}

static void launch_ysolve(real_t *bt, const real_t *sor, int II, int JJ, int ib, int nlines, int ldt, const real_t *so,
                          int lofs, size_t shm, bool sm, hipStream_t st)
{
	switch (line_bs(JJ - 2)) {
	case 64: launch_ysolve_n<64>(bt, sor, II, JJ, ib, nlines, ldt, so, lofs, shm, sm, st); break;
	case 512: launch_ysolve_n<512>(bt, sor, II, JJ, ib, nlines, ldt, so, lofs, shm, sm, st); break;
	case 1024: launch_ysolve_n<1024>(bt, sor, II, JJ, ib, nlines, ldt, so, lofs, shm, sm, st); break;
	default: launch_ysolve_n<256>(bt, sor, II, JJ, ib, nlines, ldt, so, lofs, shm, sm, st);
	}
}

size_t ylines_scratch_doubles(int II, int JJ)
{
	const int n = JJ - 2;
	return (size_t)((II - 2 + 1) / 2) * (size_t)((n + 15) & ~15) + 16;
}

// ipn: 0 Dirichlet; 2 periodic in x only: ordinary solves, one x wrap after the sweep (relax_lines_y.f90:77-176);
// 1 / 3 periodic in y (/ and x): cyclic lines, y then x wrap after each colour (:178-300)
void relax_lines_y(const real_t *so, const real_t *qf, real_t *q, const real_t *sor, real_t *bt,
                   int II, int JJ, int nstncl, int updown, hipStream_t st, int ipn)
{
	const bool sm = per_dirs(2, ipn).y;
	if (II < 3 || JJ < 3) return;
	if (!lds_ok(JJ - 2, "relax_lines_y")) return;
	const int n = JJ - 2;
	const int ldt = (n + 15) & ~15;
	const size_t shm = line_lds_doubles(n) * sizeof(real_t);
	// the lines of a colour go through gather -> solve -> scatter in chunks whose line-contiguous scratch
	// (chunk * ldt doubles) stays in the Infinity Cache between the three kernels
	const char *ce = getenv("CEDAR_AMD_YCHUNK");
	const int chunk_lines = ce ? atoi(ce) : 512; // 8192^2: 20.6 (whole colour) -> 19.8 ms per V-cycle (profiles/r01_experiment_yline_chunks.log)
	for (int c = 0; c < 2; c++) {
		int ib = (updown == BMG_DOWN) ? 1 - c : c; // DOWN: I = 3,5,.. first
		int nall = (II - 2 - ib + 1) / 2;
		if (nall <= 0) continue;
		const int step = chunk_lines > 0 ? chunk_lines : nall;
		for (int lofs = 0; lofs < nall; lofs += step) {
			const int nlines = nall - lofs < step ? nall - lofs : step;
			dim3 tg((nlines + 31) / 32, (n + 31) / 32);
			if (nstncl == 5)
				hipLaunchKernelGGL(ylines_rhs_T<true>, tg, dim3(256), 0, st, so, qf, q, bt, II, JJ, ib, nlines, ldt, lofs);
			else
				hipLaunchKernelGGL(ylines_rhs_T<false>, tg, dim3(256), 0, st, so, qf, q, bt, II, JJ, ib, nlines, ldt, lofs);
			launch_ysolve(bt, sor, II, JJ, ib, nlines, ldt, so, lofs, shm, sm, st);
			hipLaunchKernelGGL(ylines_scatter_T, tg, dim3(256), 0, st, bt, q, II, JJ, ib, nlines, ldt, lofs);
		}
		if (sm) wrap2(q, II, JJ, 1, 1, ipn == 3, st);
	}
	if (ipn == 2) wrap2(q, II, JJ, 1, 0, 1, st);
}

// ---- y-lines on transposed arrays (the solver's resident path, Dirichlet): the operator planes the right-hand
// side needs are kept transposed (setup_lines_yt), q is transposed around the sweep, and both colours run through
// the x-line kernel -- rows of the transposed arrays are the y lines, and SOR(JJ,II,2) already is the x layout of
// the transposed grid.  Same right-hand-side term order, same scan: bit-identical to relax_lines_y.  8192^2:
// 2 x 1534 us (gather + solve + scatter per colour) -> 2 x 750 us + two transposes of q.
// out(j,i) = in(i,j), whole arrays with ghosts: in is (II fast, JJ), out is (JJ fast, II)
__global__ __launch_bounds__(256) void transpose2_kernel(const real_t *__restrict__ in, real_t *__restrict__ out, int II, int JJ,
                                                         size_t bstride)
{
	__shared__ real_t tile[64][65];
	in += bstride * blockIdx.z; out += bstride * blockIdx.z; // batch item (common.h Batch)
	const int i0 = blockIdx.x * 64, j0 = blockIdx.y * 64;
	const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6; // 64 x 4
	for (int r = ty; r < 64; r += 4) {
		const int i = i0 + tx, j = j0 + r;
		if (i < II && j < JJ) tile[r][tx] = in[(size_t)i + (size_t)II * j];
	}
	__syncthreads();
	for (int r = ty; r < 64; r += 4) {
		const int i = i0 + r, j = j0 + tx;
		if (i < II && j < JJ) out[(size_t)j + (size_t)JJ * i] = tile[tx][r];
	}
}

// the same with 16-byte accesses on both sides (even extents, 16-byte aligned arrays): a lane moves two neighbouring
// columns of a row in and two neighbouring rows of a column out
__global__ __launch_bounds__(256) void transpose2_pairs_kernel(const real_t *__restrict__ in, real_t *__restrict__ out, int II, int JJ,
                                                               size_t bstride)
{
	__shared__ real_t tile[64][65];
	in += bstride * blockIdx.z; out += bstride * blockIdx.z;
	const int i0 = blockIdx.x * 64, j0 = blockIdx.y * 64;
	const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5; // 32 pairs x 8
	for (int r = r0; r < 64; r += 8) {
		const int i = i0 + 2 * c, j = j0 + r;
		if (i < II && j < JJ) {
			const d2u v = *reinterpret_cast<const d2u *>(in + (size_t)i + (size_t)II * j);
			tile[r][2 * c] = v.x; tile[r][2 * c + 1] = v.y;
		}
	}
	__syncthreads();
	for (int r = r0; r < 64; r += 8) {
		const int i = i0 + r, j = j0 + 2 * c;
		if (i < II && j < JJ) {
			d2u v; v.x = tile[2 * c][r]; v.y = tile[2 * c + 1][r];
			*reinterpret_cast<d2u *>(out + (size_t)j + (size_t)JJ * i) = v;
		}
	}
}

void transpose2(const real_t *in, real_t *out, int II, int JJ, hipStream_t st, Batch bt)
{
	// CEDAR_AMD_TRANSPOSE_PAIRS=0: 8-byte accesses (round 2).  8192^2, 49 transposes of a line-xy V-cycle: 2.63 -> 2.28 ms; a
	// 64 x 128 tile (1 KB output rows, 66 KB of LDS) measured 2.65 ms and was dropped
	const char *e = getenv("CEDAR_AMD_TRANSPOSE_PAIRS");
	const bool pairs = !(e && atoi(e) == 0) && !(II & 1) && !(JJ & 1) && !(bt.stride & 1) && !(((uintptr_t)in | (uintptr_t)out) & 15);
	if (pairs) hipLaunchKernelGGL(transpose2_pairs_kernel, dim3((II + 63) / 64, (JJ + 63) / 64, bt.n), dim3(256), 0, st, in, out, II, JJ, bt.stride);
	else hipLaunchKernelGGL(transpose2_kernel, dim3((II + 63) / 64, (JJ + 63) / 64, bt.n), dim3(256), 0, st, in, out, II, JJ, bt.stride);
}

// sot (JJ fast, II, nstncl planes): plane KS = KW^T, KW = KS^T, KSW = KSW^T, KNW = KNW^T; KO is not read by the sweep
void setup_lines_yt(const real_t *so, real_t *sot, int II, int JJ, int nstncl, hipStream_t st)
{
	const size_t PS = (size_t)II * JJ;
	transpose2(so + KW * PS, sot + KS * PS, II, JJ, st);
	transpose2(so + KS * PS, sot + KW * PS, II, JJ, st);
	if (nstncl == 5) {
		transpose2(so + KSW * PS, sot + KSW * PS, II, JJ, st);
		transpose2(so + KNW * PS, sot + KNW * PS, II, JJ, st);
	}
}

// qft = transposed right-hand side (the caller keeps it while qf is unchanged), qt = scratch for the transposed q
void relax_lines_yt(const real_t *sot, const real_t *qft, real_t *q, real_t *qt, const real_t *sor,
                    int II, int JJ, int nstncl, int updown, hipStream_t st, const real_t *pf, Batch bt)
{
	if (II < 3 || JJ < 3) return;
	if (!lds_ok(JJ - 2, "relax_lines_y")) return;
	transpose2(q, qt, II, JJ, st, bt);
	for (int c = 0; c < 2; c++) {
		const int ib = (updown == BMG_DOWN) ? 1 - c : c; // DOWN: I = 3,5,.. first
		const int nlines = (II - 2 - ib + 1) / 2;
		if (nlines <= 0) continue;
		// transposed grid: JJ is the fast extent, II the number of rows
		launch_x(op2_cedar(sot, nullptr, JJ, II), qft, qt, sor, JJ, II, nstncl, ib, st, false, true, pf, bt);
	}
	transpose2(qt, q, JJ, II, st, bt);
}

// ---- pieces of the domain-decomposed line relaxation (cedar_amd/dist2d.py): right-hand sides of the
// lines of one zebra colour into a line-contiguous buffer, the carry correction, and the way back.
template <bool NINE>
__global__ __launch_bounds__(256) void xlines_rhs_kernel(const real_t *__restrict__ so, const real_t *__restrict__ qf,
                                                          const real_t *__restrict__ q, real_t *__restrict__ out,
                                                          int II, int JJ, int lb, int ld)
{
	const int l = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x; // line of the colour, position
	if (t >= II - 2) return;
	const size_t sj = II, PS = (size_t)II * JJ;
	const size_t x = (size_t)(1 + lb + 2 * l) * sj + 1 + t;
	real_t s = qf[x]; // relax_lines_x.f90:106-111 / :128-129, reference term order
	s = s + so[KS * PS + x] * q[x - sj];
	s = s + so[KS * PS + x + sj] * q[x + sj];
	if (NINE) {
		s = s + so[KSW * PS + x] * q[x - 1 - sj];
		s = s + so[KNW * PS + x + 1] * q[x + 1 - sj];
		s = s + so[KNW * PS + x + sj] * q[x - 1 + sj];
		s = s + so[KSW * PS + x + 1 + sj] * q[x + 1 + sj];
	}
	out[(size_t)l * ld + t] = s;
}

__global__ __launch_bounds__(256) void xlines_store_kernel(const real_t *__restrict__ in, real_t *__restrict__ q,
                                                            int II, int lb, int ld)
{
	const int l = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= II - 2) return;
	q[(size_t)(1 + lb + 2 * l) * II + 1 + t] = in[(size_t)l * ld + t];
}

// y[l][i] = y[l][i] + p[l][i] * c[l]: the carry entering a line segment times the running product of its multipliers
__global__ __launch_bounds__(256) void lines_carry_kernel(real_t *__restrict__ y, const real_t *__restrict__ p,
                                                           const real_t *__restrict__ c, int n, int ld)
{
	const int l = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= n) return;
	const size_t x = (size_t)l * ld + t;
	y[x] = y[x] + p[x] * c[l];
}

// dir 0: x lines (rows 1+lb, 3+lb, ..), dir 1: y lines (columns 1+lb, 3+lb, ..); out / in: (lines, positions), ld = positions
void lines_rhs2(const real_t *so, const real_t *qf, const real_t *q, real_t *out, int II, int JJ, int nstncl, int dir, int lb,
                hipStream_t st)
{
	const int nlines = dir == 0 ? (JJ - 2 - lb + 1) / 2 : (II - 2 - lb + 1) / 2;
	const int n = dir == 0 ? II - 2 : JJ - 2;
	if (nlines <= 0 || n <= 0) return;
	if (dir == 0) {
		dim3 grid((n + 255) / 256, nlines);
		if (nstncl == 5) hipLaunchKernelGGL(xlines_rhs_kernel<true>, grid, dim3(256), 0, st, so, qf, q, out, II, JJ, lb, n);
		else hipLaunchKernelGGL(xlines_rhs_kernel<false>, grid, dim3(256), 0, st, so, qf, q, out, II, JJ, lb, n);
	} else {
		dim3 tg((nlines + 31) / 32, (n + 31) / 32);
		if (nstncl == 5) hipLaunchKernelGGL(ylines_rhs_T<true>, tg, dim3(256), 0, st, so, qf, q, out, II, JJ, lb, nlines, n, 0);
		else hipLaunchKernelGGL(ylines_rhs_T<false>, tg, dim3(256), 0, st, so, qf, q, out, II, JJ, lb, nlines, n, 0);
	}
}

void lines_store2(const real_t *in, real_t *q, int II, int JJ, int dir, int lb, hipStream_t st)
{
	const int nlines = dir == 0 ? (JJ - 2 - lb + 1) / 2 : (II - 2 - lb + 1) / 2;
	const int n = dir == 0 ? II - 2 : JJ - 2;
	if (nlines <= 0 || n <= 0) return;
	if (dir == 0) hipLaunchKernelGGL(xlines_store_kernel, dim3((n + 255) / 256, nlines), dim3(256), 0, st, in, q, II, lb, n);
	else hipLaunchKernelGGL(ylines_scatter_T, dim3((nlines + 31) / 32, (n + 31) / 32), dim3(256), 0, st, in, q, II, JJ, lb, nlines, n, 0);
}

void lines_carry(real_t *y, const real_t *p, const real_t *c, int nlines, int n, int ld, hipStream_t st)
{
	if (nlines <= 0 || n <= 0) return;
	hipLaunchKernelGGL(lines_carry_kernel, dim3((n + 255) / 256, nlines), dim3(256), 0, st, y, p, c, n, ld);
}

} // namespace cedar_amd
