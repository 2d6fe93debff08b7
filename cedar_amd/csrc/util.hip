// Small device utilities of the library.
#include "common.h"

namespace cedar_amd {

__global__ __launch_bounds__(256) void zero_fill_kernel(real_t *__restrict__ p, size_t n)
{
	for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = 0.0;
}

void zero_fill(real_t *p, size_t n, hipStream_t st)
{
	if (!n) return;
	size_t blocks = (n + 255) / 256;
	if (blocks > 4096) blocks = 4096;
	hipLaunchKernelGGL(zero_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, st, p, n);
}

__global__ __launch_bounds__(256) void vec_add_kernel(real_t *__restrict__ x, const real_t *__restrict__ z, size_t n)
{
	for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) x[i] = x[i] + z[i];
}

void vec_add(real_t *x, const real_t *z, size_t n, hipStream_t st)
{
	if (!n) return;
	size_t blocks = (n + 255) / 256;
	if (blocks > 4096) blocks = 4096;
	hipLaunchKernelGGL(vec_add_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, z, n);
}

// ---------------------------------------------------------------- v := v - mean_interior(v) * 1
// The projection onto the zero-mean vectors that cedar_amd_solver_fcg_semidefinite applies to r0 and to the final x
// (solver.cpp pcg_run) and to r and z around every cycle: 8 bytes per point in the sum and 16 in the shift.  A
// workgroup of 256 threads is pm_lanes(nx) lanes along the row by 256 / lanes rows; rows longer than 256 points are
// walked in trips.  Stage 1: a fixed number of workgroups per item, each over a fixed strided set of row groups, shuffle + LDS tree; stage 2: one
// workgroup per item sums the partials in a fixed order and divides.  No atomics, and nothing in an item's order of
// operations depends on the batch: item m of a batch is bit for bit the single-vector call, whatever nrhs and `active`.
// The sum is carried in two doubles (Knuth's two-sum: the rounding error of every addition goes to the low word), so
// the mean is the correctly rounded one whatever the order, but for ties at the 2^-100 level.  That is not a luxury: the
// cycle answers a constant left in r0 with a large smooth correction (the coarsest solve turns the constant into a
// point source of n times its size), so one unit in the last place of the mean removed from r0 moves the
// entries of the residual history near 1e-10 by 1e-6 of their value; with the exact mean the
// history does not depend on how the points are distributed over lanes and workgroups.

// lanes along the row; the host uses it too, for the number of row groups (project_mean_many)
__host__ __device__ __forceinline__ int pm_lanes(int nx) { return nx <= 64 ? 64 : nx <= 128 ? 128 : 256; }

struct Sum2 {
	real_t hi, lo;
};

__device__ __forceinline__ void sum2_add(Sum2 &s, real_t v)
{
	const real_t t = s.hi + v, bb = t - s.hi;
	s.lo += (s.hi - (t - bb)) + (v - bb); // what the addition rounded away
	s.hi = t;
}

__device__ __forceinline__ void sum2_add(Sum2 &s, const Sum2 &o)
{
	sum2_add(s, o.hi);
	s.lo += o.lo;
}

// the workgroup's sum in thread 0 (256 threads)
__device__ __forceinline__ Sum2 pm_block_sum(Sum2 v, Sum2 *lds)
{
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) {
		Sum2 u;
		u.hi = __shfl_down(v.hi, o, 64);
		u.lo = __shfl_down(v.lo, o, 64);
		sum2_add(v, u);
	}
	const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
	if (l == 0) lds[w] = v;
	__syncthreads();
	Sum2 r{0.0, 0.0};
	if (threadIdx.x == 0)
		for (int t = 0; t < 4; t++) sum2_add(r, lds[t]);
	return r;
}

// part: PROJECT_MEAN_NB pairs (hi, lo) per item
__global__ __launch_bounds__(256) void project_mean_stage1(const real_t *__restrict__ v, int II, int JJ, int KK, size_t stride,
                                                            unsigned active, real_t *__restrict__ part)
{
	__shared__ Sum2 lds[4];
	const int m = blockIdx.y;
	if (!((active >> m) & 1u)) return;
	v += stride * m;
	const int nx = II - 2, nj = JJ - 2, nk = KK == 1 ? 1 : KK - 2;
	const int lanes = pm_lanes(nx), ty = 256 / lanes;
	const int lx = threadIdx.x % lanes, ly = threadIdx.x / lanes;
	const size_t nrows = (size_t)nj * nk;
	Sum2 acc{0.0, 0.0};
	for (size_t r = (size_t)blockIdx.x * ty + ly; r < nrows; r += (size_t)gridDim.x * ty) {
		const size_t j = r % nj + 1, k = KK == 1 ? 0 : r / nj + 1;
		const real_t *row = v + (size_t)II * (j + (size_t)JJ * k);
		for (int i = lx + 1; i <= nx; i += lanes) sum2_add(acc, row[i]);
	}
	const Sum2 s = pm_block_sum(acc, lds);
	if (threadIdx.x == 0) {
		part[2 * ((size_t)m * PROJECT_MEAN_NB + blockIdx.x)] = s.hi;
		part[2 * ((size_t)m * PROJECT_MEAN_NB + blockIdx.x) + 1] = s.lo;
	}
}

// mean[m] = (sum of item m's nb partials) / count; 0 for an item outside `active`
__global__ __launch_bounds__(256) void project_mean_stage2(const real_t *__restrict__ part, int nb, real_t count, unsigned active,
                                                            real_t *__restrict__ mean)
{
	__shared__ Sum2 lds[4];
	const int m = blockIdx.x;
	if (!((active >> m) & 1u)) {
		if (threadIdx.x == 0) mean[m] = 0.0;
		return;
	}
	Sum2 acc{0.0, 0.0};
	for (int i = threadIdx.x; i < nb; i += blockDim.x) {
		const real_t *q = part + 2 * ((size_t)m * PROJECT_MEAN_NB + i);
		sum2_add(acc, Sum2{q[0], q[1]});
	}
	const Sum2 s = pm_block_sum(acc, lds);
	if (threadIdx.x == 0) mean[m] = (s.hi + s.lo) / count;
}

__global__ __launch_bounds__(256) void project_mean_shift(real_t *__restrict__ v, int II, int JJ, int KK, size_t stride,
                                                           unsigned active, const real_t *__restrict__ mean)
{
	const int m = blockIdx.y;
	if (!((active >> m) & 1u)) return;
	v += stride * m;
	const real_t c = mean[m];
	const int nx = II - 2, nj = JJ - 2, nk = KK == 1 ? 1 : KK - 2;
	const int lanes = pm_lanes(nx), ty = 256 / lanes;
	const int lx = threadIdx.x % lanes, ly = threadIdx.x / lanes;
	const size_t nrows = (size_t)nj * nk;
	for (size_t r = (size_t)blockIdx.x * ty + ly; r < nrows; r += (size_t)gridDim.x * ty) {
		const size_t j = r % nj + 1, k = KK == 1 ? 0 : r / nj + 1;
		real_t *row = v + (size_t)II * (j + (size_t)JJ * k);
		for (int i = lx + 1; i <= nx; i += lanes) row[i] = row[i] - c;
	}
}

void project_mean_many(real_t *v, int II, int JJ, int KK, real_t *scratch, hipStream_t st, Batch bt, unsigned active)
{
	const int nx = II - 2, ty = 256 / pm_lanes(nx);
	const size_t nrows = (size_t)(JJ - 2) * (KK == 1 ? 1 : KK - 2), groups = (nrows + ty - 1) / ty;
	// the workgroup count is a function of the extents alone (it fixes the order of the sum)
	const int nb = groups < (size_t)PROJECT_MEAN_NB ? (int)groups : (int)PROJECT_MEAN_NB;
	real_t *mean = scratch + 2 * (size_t)bt.n * PROJECT_MEAN_NB;
	const real_t count = (real_t)nx * (real_t)nrows;
	hipLaunchKernelGGL(project_mean_stage1, dim3(nb, bt.n), dim3(256), 0, st, v, II, JJ, KK, bt.stride, active, scratch);
	hipLaunchKernelGGL(project_mean_stage2, dim3(bt.n), dim3(256), 0, st, scratch, nb, count, active, mean);
	hipLaunchKernelGGL(project_mean_shift, dim3(nb, bt.n), dim3(256), 0, st, v, II, JJ, KK, bt.stride, active, mean);
}

void project_mean(real_t *v, int II, int JJ, int KK, real_t *scratch, hipStream_t st)
{
	project_mean_many(v, II, JJ, KK, scratch, st, Batch{1, 0}, 1u);
}

} // namespace cedar_amd
