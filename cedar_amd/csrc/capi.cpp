// C-ABI layer 1: the BMG2_/BMG3_SymStd_* drop-in entry points, the device
// memory helpers and the library-wide runtime state (stream, staging pool,
// error callback).  Declarations + reference citations: include/cedar_amd.h.
#include "../../include/cedar_amd.h"
#include "common.h"
#include "stage.h"
#include "relax3_psum.h"
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>

using namespace cedar_amd;

// ------------------------------------------------------------------ error callback
// The reference's kernels import print_error from the host program
// (src/2d/ftn/ModInterface.f90:4-9).  Same contract here: a host definition wins
// over this weak default.
extern "C" __attribute__((weak)) void print_error(char *msg)
{
	fprintf(stderr, "[cedar_amd] %s\n", msg);
}

namespace cedar_amd {

static hipStream_t g_stream = nullptr;
hipStream_t current_stream() { return g_stream; }

bool is_device_ptr(const void *p)
{
	hipPointerAttribute_t attr;
	hipError_t e = hipPointerGetAttributes(&attr, p);
	if (e != hipSuccess) {
		(void)hipGetLastError(); // plain host memory: clear the sticky error
		return false;
	}
	return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

// tiny size-bucketed pool so that per-call staging does not hipMalloc every time
static std::multimap<size_t, void *> g_pool;
static size_t g_pool_bytes = 0;
static const size_t POOL_CAP = (size_t)8 << 30;

void *pool_get(size_t bytes)
{
	auto it = g_pool.lower_bound(bytes);
	if (it != g_pool.end() && it->first <= bytes + bytes / 4 + 4096) {
		void *p = it->second;
		g_pool_bytes -= it->first;
		g_pool.erase(it);
		return p;
	}
	void *p = nullptr;
	CEDAR_HIP_CHECK(hipMalloc(&p, bytes));
	return p;
}

void pool_put(void *p, size_t bytes)
{
	// the true capacity of a recycled block is unknown; blocks are re-keyed by
	// the size they were last requested with (always <= capacity)
	if (g_pool_bytes + bytes > POOL_CAP) {
		CEDAR_HIP_CHECK(hipFree(p));
		return;
	}
	g_pool.emplace(bytes, p);
	g_pool_bytes += bytes;
}

void launch_check(const char *who)
{
	const hipError_t e = hipGetLastError(); // clears it
	if (e == hipSuccess) return;
	char buf[256];
	snprintf(buf, sizeof(buf), "%s: a kernel launch was rejected by the HIP runtime (%s: %s); results are incomplete", who,
	         hipGetErrorName(e), hipGetErrorString(e));
	print_error(buf);
}

static void report(const char *msg)
{
	char buf[256];
	strncpy(buf, msg, sizeof(buf) - 1);
	buf[sizeof(buf) - 1] = 0;
	print_error(buf);
}

// 2D kernels with a periodic branch on the GPU path: |jpn| in {1 per_y, 2 per_x, 3 per_xy}.  Returns
// -1 after reporting when the code is not served (indefinite variants, 3D codes), else |jpn|.
static int bc2(int jpn, const char *who)
{
	if (jpn >= 0 && jpn <= 3) return jpn;
	char buf[200];
	snprintf(buf, sizeof(buf), "%s: boundary code %d is not implemented on the GPU path (0 definite, 1..3 periodic y/x/xy)", who, jpn);
	report(buf);
	return -1;
}

// 3D boundary code of BMG_get_bc (0, 1 y, 2 x, 3 xy, 5 z, 6 xz, 7 yz, 8 xyz); the indefinite (negative) codes
// and -4 are not implemented
static bool bc3(int jpn, const char *who)
{
	if (jpn >= 0 && periodic3_code_ok(jpn)) return true;
	char buf[200];
	snprintf(buf, sizeof(buf), "%s: boundary code %d is not implemented on the GPU path (0 and the definite periodic codes are)",
	         who, jpn);
	report(buf);
	return false;
}

// the periodic interpolation set-up and Galerkin product coarsen a periodic direction by pairs: its extent must
// be even (the reference's example uses even extents; odd ones are refused rather than guessed)
static bool even_periodic(int ipn, len_t iif, len_t jjf, len_t kkf, const char *who)
{
	const PerDirs pd = per_dirs(3, ipn);
	if ((pd.x && (iif & 1)) || (pd.y && (jjf & 1)) || (pd.z && (kkf & 1))) {
		char buf[200];
		snprintf(buf, sizeof(buf), "%s: a periodic direction needs an even extent (got %u x %u x %u, code %d)", who,
		         (unsigned)iif - 2, (unsigned)jjf - 2, (unsigned)kkf - 2, ipn);
		report(buf);
		return false;
	}
	return true;
}

// run f(Op3f, stream) on a temporary float copy (common.h Op3f) of so and sor's reciprocal plane: built for the call, back
// in the pool once the stream has drained.  false = refused (reported), f not run
template <class F>
static bool with_op32_copy(const real_t *so, const real_t *sor_msor, int II, int JJ, int KK, const char *who, F &&f)
{
	char buf[200];
	if (II < 3 || JJ < 3 || KK < 3 || (II - 2 + 1) / 2 > 512) {
		snprintf(buf, sizeof(buf), "%s: extents %d x %d x %d (ghosts included) are not served (rows of 1 .. 1024 points); nothing done",
		         who, II, JJ, KK);
		report(buf);
		return false;
	}
	hipStream_t st = current_stream();
	const size_t bytes = ilv32_floats(II, JJ, KK) * sizeof(float);
	float *c = static_cast<float *>(pool_get(bytes));
	int *flag = static_cast<int *>(pool_get(sizeof(int))), host = 0;
	CEDAR_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(int), st));
	ilv32_build(so, sor_msor, c, II, JJ, KK, flag, st);
	CEDAR_HIP_CHECK(hipMemcpyAsync(&host, flag, sizeof(int), hipMemcpyDeviceToHost, st));
	CEDAR_HIP_CHECK(hipStreamSynchronize(st));
	pool_put(flag, sizeof(int));
	if (host) {
		snprintf(buf, sizeof(buf), "%s: an entry of the operator or of 1/diag overflows single precision; nothing done", who);
		report(buf);
	} else {
		f(op3f_ilv(c, II, JJ, KK), st);
		CEDAR_HIP_CHECK(hipStreamSynchronize(st));
	}
	pool_put(c, bytes);
	return !host;
}

// run f(weights view, stream) on a temporary float copy (common.h Ci3f) of the weights ci: built for the call, back in the
// pool once the stream has drained.  false = refused (reported), f not run
template <class F>
static bool with_ci32_copy(const real_t *ci, int IIC, int JJC, int KKC, int nslots, const char *who, F &&f)
{
	hipStream_t st = current_stream();
	const size_t bytes = ci32_floats(IIC, JJC, KKC, nslots) * sizeof(float);
	float *c = static_cast<float *>(pool_get(bytes));
	int *flag = static_cast<int *>(pool_get(sizeof(int))), host = 0;
	CEDAR_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(int), st));
	ci32_build(ci, c, IIC, JJC, KKC, nslots, flag, st);
	CEDAR_HIP_CHECK(hipMemcpyAsync(&host, flag, sizeof(int), hipMemcpyDeviceToHost, st));
	CEDAR_HIP_CHECK(hipStreamSynchronize(st));
	pool_put(flag, sizeof(int));
	if (host) {
		char buf[200];
		snprintf(buf, sizeof(buf), "%s: an interpolation weight overflows single precision; nothing done", who);
		report(buf);
	} else {
		f(ci32_view(c, IIC, JJC, KKC), st);
		CEDAR_HIP_CHECK(hipStreamSynchronize(st));
	}
	pool_put(c, bytes);
	return !host;
}

// extents (ghosts included) and arrays a _ci32 entry point serves; nst_ok: the stencil code where the call takes one
static bool ci32_args_refused(bool arrays_ok, bool extents_ok, bool nst_ok, const char *who)
{
	const char *why = !arrays_ok ? "a required array is NULL" : !extents_ok ? "every extent (ghosts included) must be at least 3"
	                  : !nst_ok ? "nstncl is not a stencil code of this dimension" : nullptr;
	if (!why) return false;
	char msg[200];
	snprintf(msg, sizeof(msg), "%s: %s; nothing done", who, why);
	print_error(msg);
	return true;
}

// the same for a 7-point operator (common.h Op7f, op7f.hip): rows of any length
template <class F>
static bool with_op7f_copy(const real_t *so, const real_t *sor_msor, int II, int JJ, int KK, const char *who, F &&f)
{
	char buf[200];
	if (II < 3 || JJ < 3 || KK < 3) {
		snprintf(buf, sizeof(buf), "%s: extents %d x %d x %d (ghosts included) are not served; nothing done", who, II, JJ, KK);
		report(buf);
		return false;
	}
	hipStream_t st = current_stream();
	const size_t bytes = op7f_floats(II, JJ, KK) * sizeof(float);
	float *c = static_cast<float *>(pool_get(bytes));
	int *flag = static_cast<int *>(pool_get(sizeof(int))), host = 0;
	CEDAR_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(int), st));
	op7f_build(so, sor_msor, c, II, JJ, KK, flag, st);
	CEDAR_HIP_CHECK(hipMemcpyAsync(&host, flag, sizeof(int), hipMemcpyDeviceToHost, st));
	CEDAR_HIP_CHECK(hipStreamSynchronize(st));
	pool_put(flag, sizeof(int));
	if (host) {
		snprintf(buf, sizeof(buf), "%s: an entry of the operator or of 1/diag overflows single precision; nothing done", who);
		report(buf);
	} else {
		f(op7f_view(c, II, JJ, KK), st);
		CEDAR_HIP_CHECK(hipStreamSynchronize(st));
	}
	pool_put(c, bytes);
	return !host;
}

} // namespace cedar_amd

extern "C" {

const char *cedar_amd_version(void) { return "cedar_amd 0.1 (gfx950)"; }

// src/2d/ftn/BMG_get_bc.f90:11-22 with include/cedar/2d/ftn/BMG_parameters_c.h values
void BMG_get_bc(int per_mask, int *ibc)
{
	// values: src/3d/ftn/BMG_parameters_f90.h:345-360
	static const int bcmap[8] = { 0 /*definite*/, 2 /*per_x*/, 1 /*per_y*/, 3 /*per_xy*/,
		                          5 /*per_z*/, 6 /*per_xz*/, 7 /*per_yz*/, 8 /*per_xyz*/ };
	*ibc = bcmap[per_mask & 7];
}

// ------------------------------------------------------------------ memory helpers
int cedar_amd_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) {
		(void)hipGetLastError();
		return 0;
	}
	return n;
}
int cedar_amd_set_device(int dev) { return hipSetDevice(dev) == hipSuccess ? 0 : 1; }
void cedar_amd_memset(void *dst, int value, size_t bytes);
void *cedar_amd_malloc(size_t bytes)
{
	void *p = nullptr;
	CEDAR_HIP_CHECK(hipMalloc(&p, bytes ? bytes : 8));
	cedar_amd_memset(p, 0, bytes);
	return p;
}
void cedar_amd_free(void *p)
{
	if (!p) return;
	relax3_release(static_cast<const real_t *>(p)); // an operator registered with cedar_amd_relax3_prepare goes with its copy
	CEDAR_HIP_CHECK(hipFree(p));
}
void cedar_amd_memcpy_h2d(void *dst, const void *src, size_t bytes)
{
	CEDAR_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, current_stream()));
	CEDAR_HIP_CHECK(hipStreamSynchronize(current_stream()));
}
void cedar_amd_memcpy_d2h(void *dst, const void *src, size_t bytes)
{
	CEDAR_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, current_stream()));
	CEDAR_HIP_CHECK(hipStreamSynchronize(current_stream()));
}
void cedar_amd_memcpy_d2d(void *dst, const void *src, size_t bytes)
{
	CEDAR_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, current_stream()));
}
void cedar_amd_memset(void *dst, int value, size_t bytes)
{
	// zeroing whole doubles (every use the library itself makes) goes through its own kernel, see common.h zero_fill
	if (value == 0 && bytes % sizeof(real_t) == 0 && (uintptr_t)dst % sizeof(real_t) == 0)
		zero_fill(static_cast<real_t *>(dst), bytes / sizeof(real_t), current_stream());
	else
		CEDAR_HIP_CHECK(hipMemsetAsync(dst, value, bytes, current_stream()));
}
void cedar_amd_sync(void) { CEDAR_HIP_CHECK(hipStreamSynchronize(current_stream())); }
void cedar_amd_set_stream(void *s) { cedar_amd::g_stream = static_cast<hipStream_t>(s); }
void *cedar_amd_get_stream(void) { return cedar_amd::g_stream; }

void cedar_amd_matvec2(const real_t *so, const real_t *q, real_t *qf, len_t II, len_t JJ, int nstncl)
{
	const size_t P = (size_t)II * JJ;
	Staged sso(so, P * nstncl, true, false), sq(q, P, true, false), sqf(qf, P, true, true);
	matvec2(sso.get(), sq.get(), sqf.get(), (int)II, (int)JJ, nstncl, current_stream());
}

void cedar_amd_matvec3(const real_t *so, const real_t *q, real_t *qf, len_t II, len_t JJ, len_t KK, int nstncl)
{
	const size_t P = (size_t)II * JJ * KK;
	Staged sso(so, P * nstncl, true, false), sq(q, P, true, false), sqf(qf, P, true, true);
	matvec3(sso.get(), sq.get(), sqf.get(), (int)II, (int)JJ, (int)KK, nstncl, current_stream());
}

double cedar_amd_l2norm(const real_t *v, len_t II, len_t JJ, len_t KK)
{
	size_t n = (size_t)II * JJ * KK;
	Staged sv(v, n, true, false);
	real_t *scratch = static_cast<real_t *>(pool_get(4100 * sizeof(real_t)));
	sumsq_interior(sv.get(), (int)II, (int)JJ, (int)KK, scratch, scratch + 4096, current_stream());
	double ss = 0;
	cedar_amd_memcpy_d2h(&ss, scratch + 4096, sizeof(double));
	pool_put(scratch, 4100 * sizeof(real_t));
	return std::sqrt(ss);
}

void cedar_amd_gallery(int which, real_t *so, real_t *b, len_t nx, len_t ny, len_t nz, const double *params)
{
	static const int nst_of[13] = { 3, 3, 5, 0, 0, 0, 0, 0, 0, 0, 4, 4, 14 };
	const int which_in = which;
	if (which >= 100) which -= 100; /* placed inside a global grid, see gallery.hip */
	if (which < 0 || which > 12 || nst_of[which] == 0) {
		report("cedar_amd_gallery: unknown operator");
		return;
	}
	bool d3 = which >= 10;
	size_t npts = (size_t)(nx + 2) * (ny + 2) * (d3 ? nz + 2 : 1);
	Staged sso(so, npts * nst_of[which], false, true);
	Staged sb(b, npts, false, true);
	zero_fill(sso.get(), npts * nst_of[which], current_stream());
	if (b) zero_fill(sb.get(), npts, current_stream());
	gallery_fill(which_in, sso.get(), sb.get(), (int)nx, (int)ny, d3 ? (int)nz : 1, params, current_stream());
}

// ------------------------------------------------------------------ 2D drop-ins
void BMG2_SymStd_SETUP_recip(real_t *so, real_t *sor, len_t nx, len_t ny, int nstncl, int nsor_v)
{
	(void)nsor_v;
	size_t P = (size_t)nx * ny; // nx,ny are the array extents incl. ghosts (so.len())
	Staged sso(so, P * nstncl, true, false), ssor(sor, P * 2, true, true);
	setup_recip(sso.get() + KO * P, ssor.get() + P, nx, ny, 1, current_stream());
}

void BMG2_SymStd_relax_GS(int k, real_t *SO, real_t *QF, real_t *Q, real_t *SOR, len_t II, len_t JJ,
                          int kf, int ifd, int nstncl, int nsorv, int irelax_sym, int updown, int jpn)
{
	(void)nsorv;
	const int ipn = bc2(jpn, "BMG2_SymStd_relax_GS");
	if (ipn < 0) return;
	size_t P = (size_t)II * JJ;
	// reference branch: 9-point when K < KF or IFD != 1 (relax_GS.f90:89)
	int nst_eff = (k < kf || ifd != 1) ? 5 : 3;
	if (nst_eff > nstncl) nst_eff = nstncl;
	// NONSYM always uses the DOWN ordering (relax_GS.f90:78-87)
	int ud = (irelax_sym == 0) ? BMG_DOWN : updown;
	Staged sso(SO, P * nstncl, true, false), sqf(QF, P, true, false), sq(Q, P, true, true), ssor(SOR, P * 2, true, false);
	if (ipn == 0)
		relax2_gs(sso.get(), sqf.get(), sq.get(), ssor.get(), (int)II, (int)JJ, nst_eff, ud, current_stream());
	else if (relax2_gs_per(sso.get(), sqf.get(), sq.get(), ssor.get(), (int)II, (int)JJ, nst_eff, ud, ipn, current_stream()))
		report("BMG2_SymStd_relax_GS: periodic rows longer than 8192 points are not supported");
}

void BMG2_SymStd_residual(int *k, real_t *SO, real_t *QF, real_t *Q, real_t *RES, len_t *II, len_t *JJ,
                          int *kf, int *ifd, int *nstncl, int *ibc, int *irelax, int *irelax_sym, int *updown)
{
	(void)ibc; (void)irelax; (void)irelax_sym; (void)updown;
	size_t P = (size_t)(*II) * (*JJ);
	int nst_eff = (*k < *kf || *ifd != 1) ? 5 : 3;
	if (nst_eff > *nstncl) nst_eff = *nstncl;
	Staged sso(SO, P * (*nstncl), true, false), sqf(QF, P, true, false), sq(Q, P, true, false), sr(RES, P, true, true);
	residual2(sso.get(), sqf.get(), sq.get(), sr.get(), (int)*II, (int)*JJ, nst_eff, current_stream());
}

void BMG2_SymStd_SETUP_lines_x(real_t *SO, real_t *SOR, len_t Nx, len_t Ny, int NStncl, int JPN)
{
	const int ipn = bc2(JPN, "BMG2_SymStd_SETUP_lines_x");
	if (ipn < 0) return;
	size_t P = (size_t)Nx * Ny;
	Staged sso(SO, P * NStncl, true, false), ssor(SOR, P * 2, true, true);
	setup_lines_x(sso.get(), ssor.get(), (int)Nx, (int)Ny, current_stream(), per_dirs(2, ipn).x);
}

void BMG2_SymStd_SETUP_lines_y(real_t *SO, real_t *SOR, len_t Nx, len_t Ny, int NStncl, int JPN)
{
	const int ipn = bc2(JPN, "BMG2_SymStd_SETUP_lines_y");
	if (ipn < 0) return;
	size_t P = (size_t)Nx * Ny;
	Staged sso(SO, P * NStncl, true, false), ssor(SOR, P * 2, true, true);
	setup_lines_y(sso.get(), ssor.get(), (int)Nx, (int)Ny, current_stream(), per_dirs(2, ipn).y);
}

void BMG2_SymStd_relax_lines_x(int k, real_t *SO, real_t *QF, real_t *Q, real_t *SOR, real_t *B,
                               len_t II, len_t JJ, int kf, int ifd, int nstencil, int irelax_sym,
                               int updown, int jpn)
{
	(void)B;
	const int ipn = bc2(jpn, "BMG2_SymStd_relax_lines_x");
	if (ipn < 0) return;
	size_t P = (size_t)II * JJ;
	int nst_eff = (k < kf || ifd != 1) ? 5 : 3;
	if (nst_eff > nstencil) nst_eff = nstencil;
	int ud = (irelax_sym == 0) ? BMG_DOWN : updown;
	Staged sso(SO, P * nstencil, true, false), sqf(QF, P, true, false), sq(Q, P, true, true), ssor(SOR, P * 2, true, false);
	relax_lines_x(sso.get(), sqf.get(), sq.get(), ssor.get(), (int)II, (int)JJ, nst_eff, ud, current_stream(), ipn);
}

void BMG2_SymStd_relax_lines_y(int k, real_t *SO, real_t *QF, real_t *Q, real_t *SOR, real_t *B,
                               len_t II, len_t JJ, int kf, int ifd, int nstencil, int irelax_sym,
                               int updown, int jpn)
{
	(void)B; // the reference's 2*JJ per-line scratch is too small for a whole colour: own HBM scratch
	const int ipn = bc2(jpn, "BMG2_SymStd_relax_lines_y");
	if (ipn < 0) return;
	size_t P = (size_t)II * JJ;
	int nst_eff = (k < kf || ifd != 1) ? 5 : 3;
	if (nst_eff > nstencil) nst_eff = nstencil;
	int ud = (irelax_sym == 0) ? BMG_DOWN : updown;
	size_t nscr = ylines_scratch_doubles((int)II, (int)JJ);
	real_t *scr = static_cast<real_t *>(pool_get(nscr * sizeof(real_t)));
	{
		Staged sso(SO, P * nstencil, true, false), sqf(QF, P, true, false), sq(Q, P, true, true), ssor(SOR, P * 2, true, false);
		relax_lines_y(sso.get(), sqf.get(), sq.get(), ssor.get(), scr, (int)II, (int)JJ, nst_eff, ud, current_stream(), ipn);
	}
	CEDAR_HIP_CHECK(hipStreamSynchronize(current_stream()));
	pool_put(scr, nscr * sizeof(real_t));
}

void BMG2_SymStd_restrict(real_t *Q, real_t *QC, real_t *CI, int Nx, int Ny, int Nxc, int Nyc, int jpn)
{
	const int ipn = bc2(jpn, "BMG2_SymStd_restrict");
	if (ipn < 0) return;
	size_t P = (size_t)Nx * Ny, PC = (size_t)Nxc * Nyc;
	// the periodic branch refreshes the fine vector's ghosts in place (restrict.f90:100-111)
	Staged sq(Q, P, true, ipn != 0), sqc(QC, PC, true, true), sci(CI, PC * 8, true, false);
	if (ipn == 0) restrict2(sq.get(), sqc.get(), sci.get(), Nx, Ny, Nxc, Nyc, current_stream());
	else restrict2_per(sq.get(), sqc.get(), sci.get(), Nx, Ny, Nxc, Nyc, ipn, current_stream());
}

void BMG2_SymStd_interp_add(real_t *Q, real_t *QC, real_t *RES, real_t *SO, real_t *CI,
                            len_t IIC, len_t JJC, len_t IIF, len_t JJF, int nstncl, int jpn)
{
	const int ipn = bc2(jpn, "BMG2_SymStd_interp_add");
	if (ipn < 0) return;
	size_t P = (size_t)IIF * JJF, PC = (size_t)IIC * JJC;
	Staged sq(Q, P, true, true), sqc(QC, PC, true, false), sr(RES, P, true, true),
	    sso(SO, P * nstncl, true, false), sci(CI, PC * 8, true, false);
	if (ipn == 0)
		interp_add2(sq.get(), sqc.get(), sr.get(), sso.get(), sci.get(), (int)IIC, (int)JJC, (int)IIF, (int)JJF, current_stream());
	else
		interp_add2_per(sq.get(), sqc.get(), sr.get(), sso.get(), sci.get(), (int)IIC, (int)JJC, (int)IIF, (int)JJF, ipn,
		                current_stream());
}

void BMG2_SymStd_SETUP_interp_OI(real_t *so, real_t *soc, real_t *ci, len_t iif, len_t jjf,
                                 len_t iic, len_t jjc, int ifd, int nstncl, int jpn, int irelax)
{
	(void)soc; (void)irelax;
	const int ipn = bc2(jpn, "BMG2_SymStd_SETUP_interp_OI");
	if (ipn < 0) return;
	size_t P = (size_t)iif * jjf, PC = (size_t)iic * jjc;
	Staged sso(so, P * nstncl, true, false), sci(ci, PC * 8, true, true);
	if (ipn == 0) setup_interp2(sso.get(), sci.get(), (int)iif, (int)jjf, (int)iic, (int)jjc, ifd, current_stream());
	else setup_interp2_per(sso.get(), sci.get(), (int)iif, (int)jjf, (int)iic, (int)jjc, ifd, ipn, current_stream());
}

void BMG2_SymStd_SETUP_ITLI_ex(real_t *so, real_t *soc, real_t *ci, len_t iif, len_t jjf,
                               len_t iic, len_t jjc, int ifd, int nstncl, int ipn)
{
	const int bc = bc2(ipn, "BMG2_SymStd_SETUP_ITLI_ex");
	if (bc < 0) return;
	size_t P = (size_t)iif * jjf, PC = (size_t)iic * jjc;
	Staged sso(so, P * nstncl, true, false), ssoc(soc, PC * 5, true, true), sci(ci, PC * 8, true, false);
	if (bc == 0) galerkin2(sso.get(), ssoc.get(), sci.get(), (int)iif, (int)jjf, (int)iic, (int)jjc, ifd, current_stream());
	else galerkin2_per(sso.get(), ssoc.get(), sci.get(), (int)iif, (int)jjf, (int)iic, (int)jjc, ifd, bc, current_stream());
}

static void cg_info(int *dinfo, const char *who)
{
	int info = 0;
	cedar_amd_memcpy_d2h(&info, dinfo, sizeof(int));
	if (info != 0) report(who);
}

void BMG2_SymStd_SETUP_cg_LU(real_t *so, len_t *ii, len_t *jj, int *nstncl, real_t *abd,
                             len_t *nabd1, len_t *nabd2, int *ibc)
{
	const int bc = bc2(*ibc, "BMG2_SymStd_SETUP_cg_LU");
	if (bc < 0) return;
	size_t P = (size_t)(*ii) * (*jj), NA = (size_t)(*nabd1) * (*nabd2);
	if (bc && ((size_t)*nabd1 < (size_t)(*ii - 2) * (*jj - 2) || (size_t)*nabd2 < (size_t)(*ii - 2) * (*jj - 2))) {
		report("BMG2_SymStd_SETUP_cg_LU: the periodic coarsest operator is dense, ABD(n,n)");
		return;
	}
	Staged sso(so, P * (*nstncl), true, false), sabd(abd, NA, true, true);
	int *dinfo = static_cast<int *>(pool_get(64));
	if (bc == 0) setup_cg2(sso.get(), (int)*ii, (int)*jj, *nstncl, sabd.get(), (int)*nabd1, (int)*nabd2, dinfo, current_stream());
	else setup_cg2_per(sso.get(), (int)*ii, (int)*jj, *nstncl, sabd.get(), (int)*nabd1, bc, dinfo, current_stream());
	cg_info(dinfo, "Coarse grid Cholesky decomp failed!");
	pool_put(dinfo, 64);
}

void BMG2_SymStd_SOLVE_cg(real_t *q, real_t *qf, len_t ii, len_t jj, real_t *abd, real_t *bbd,
                          len_t nabd1, len_t nabd2, int ibc)
{
	const int bc = bc2(ibc, "BMG2_SymStd_SOLVE_cg");
	if (bc < 0) return;
	size_t P = (size_t)ii * jj, NA = (size_t)nabd1 * nabd2;
	Staged sq(q, P, true, true), sqf(qf, P, true, false), sabd(abd, NA, true, false), sb(bbd, nabd2, false, true);
	if (bc == 0) solve_cg2(sq.get(), sqf.get(), (int)ii, (int)jj, sabd.get(), sb.get(), (int)nabd1, (int)nabd2, current_stream());
	else solve_cg2_per(sq.get(), sqf.get(), (int)ii, (int)jj, sabd.get(), sb.get(), (int)nabd1, bc, current_stream());
}

// ------------------------------------------------------------------ domain-decomposition pieces
void cedar_amd_relax3_pass(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, len_t kk,
                           int jb, int kb, int efirst)
{
	size_t P = (size_t)ii * jj * kk;
	Staged sso(so, P * 14, true, false), sqf(qf, P, true, false), sq(q, P, true, true), ssor(sor, P * 2, true, false);
	relax3_pass27(sso.get(), sqf.get(), sq.get(), ssor.get(), (int)ii, (int)jj, (int)kk, jb, kb, efirst, current_stream());
}

void cedar_amd_relax3_pass_part(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, len_t kk,
                                int jb, int kb, int efirst, int part)
{
	size_t P = (size_t)ii * jj * kk;
	Staged sso(so, P * 14, true, false), sqf(qf, P, true, false), sq(q, P, true, true), ssor(sor, P * 2, true, false);
	relax3_pass27(sso.get(), sqf.get(), sq.get(), ssor.get(), (int)ii, (int)jj, (int)kk, jb, kb, efirst, current_stream(), part);
}

void cedar_amd_relax2_pass(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, int jb, int efirst)
{
	size_t P = (size_t)ii * jj;
	Staged sso(so, P * 5, true, false), sqf(qf, P, true, false), sq(q, P, true, true), ssor(sor, P * 2, true, false);
	relax2_pass9(sso.get(), sqf.get(), sq.get(), ssor.get(), (int)ii, (int)jj, jb, efirst, current_stream());
}

void cedar_amd_relax2_fixup(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, int icol, int jb)
{
	size_t P = (size_t)ii * jj;
	Staged sso(so, P * 5, true, false), sqf(qf, P, true, false), sq(q, P, true, true), ssor(sor, P * 2, true, false);
	relax2_fixup9(sso.get(), sqf.get(), sq.get(), ssor.get(), (int)ii, (int)jj, icol, jb, current_stream());
}

void cedar_amd_relax2_colour5(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, int jo)
{
	size_t P = (size_t)ii * jj;
	Staged sso(so, P * 3, true, false), sqf(qf, P, true, false), sq(q, P, true, true), ssor(sor, P * 2, true, false);
	relax2_colour5(sso.get(), sqf.get(), sq.get(), ssor.get(), (int)ii, (int)jj, jo, current_stream());
}

void cedar_amd_setup_interp2_phase(real_t *so, real_t *ci, len_t iif, len_t jjf, len_t iic, len_t jjc,
                                   int ifd, int nstncl, int phase, int ilo, int jlo)
{
	size_t P = (size_t)iif * jjf, PC = (size_t)iic * jjc;
	Staged sso(so, P * nstncl, true, false), sci(ci, PC * 8, true, true);
	setup_interp2_phase(sso.get(), sci.get(), (int)iif, (int)jjf, (int)iic, (int)jjc, ifd, phase, ilo, jlo, current_stream());
}

void cedar_amd_lines_rhs2(const real_t *so, const real_t *qf, const real_t *q, real_t *out, len_t ii, len_t jj,
                          int nstncl, int dir, int lb)
{
	lines_rhs2(so, qf, q, out, (int)ii, (int)jj, nstncl, dir, lb, current_stream());
}

void cedar_amd_lines_carry(real_t *y, const real_t *p, const real_t *c, int nlines, int n, int ld)
{
	lines_carry(y, p, c, nlines, n, ld, current_stream());
}

void cedar_amd_lines_store2(const real_t *in, real_t *q, len_t ii, len_t jj, int dir, int lb)
{
	lines_store2(in, q, (int)ii, (int)jj, dir, lb, current_stream());
}

void cedar_amd_affine_lines(real_t *y, const real_t *a, const real_t *div, int nlines, int n, int ld, int reverse)
{
	affine_lines(y, a, div, nlines, n, ld, reverse, current_stream());
}

void cedar_amd_relax3_planes(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, len_t kk,
                             int kb, int up, int part)
{
	size_t P = (size_t)ii * jj * kk;
	Staged sso(so, P * 14, true, false), sqf(qf, P, true, false), sq(q, P, true, true), ssor(sor, P * 2, true, false);
	relax3_planes27(sso.get(), sqf.get(), sq.get(), ssor.get(), (int)ii, (int)jj, (int)kk, kb, up, part, current_stream());
}

void cedar_amd_relax3_fixup(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, len_t kk,
                            int icol, int jb, int kb)
{
	size_t P = (size_t)ii * jj * kk;
	Staged sso(so, P * 14, true, false), sqf(qf, P, true, false), sq(q, P, true, true), ssor(sor, P * 2, true, false);
	relax3_fixup27(sso.get(), sqf.get(), sq.get(), ssor.get(), (int)ii, (int)jj, (int)kk, icol, jb, kb, current_stream());
}

void cedar_amd_relax3_rows(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, len_t kk, int j0, int jstep,
                           int nrj, int kb, int efirst)
{
	size_t P = (size_t)ii * jj * kk;
	Staged sso(so, P * 14, true, false), sqf(qf, P, true, false), sq(q, P, true, true), ssor(sor, P * 2, true, false);
	relax3_rows27(sso.get(), sqf.get(), sq.get(), ssor.get(), (int)ii, (int)jj, (int)kk, j0, jstep, nrj, kb, efirst, current_stream());
}

void cedar_amd_relax3_cols(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, len_t kk, int jb, int kb,
                           int ncol, const int *cols, int xrow0, int xrow1)
{
	size_t P = (size_t)ii * jj * kk;
	Staged sso(so, P * 14, true, false), sqf(qf, P, true, false), sq(q, P, true, true), ssor(sor, P * 2, true, false);
	relax3_cols27(sso.get(), sqf.get(), sq.get(), ssor.get(), (int)ii, (int)jj, (int)kk, jb, kb, ncol, cols, xrow0, xrow1,
	              current_stream());
}

size_t cedar_amd_relax3_strip_doubles(len_t jj, len_t kk) { return relax3_strip_doubles((int)jj, (int)kk); }

void cedar_amd_relax3_strip_build(const real_t *so, const real_t *sor, len_t ii, len_t jj, len_t kk, int side, real_t *out)
{
	relax3_strip_build(so, sor, (int)ii, (int)jj, (int)kk, side, out, current_stream());
}

void cedar_amd_relax3_cols_strip(const real_t *strip_lo, const real_t *strip_hi, real_t *qf, real_t *q, len_t ii, len_t jj, len_t kk,
                                 int jb, int kb, int ncol, const int *cols, int xrow0, int xrow1)
{
	relax3_cols27_strip(strip_lo, strip_hi, qf, q, (int)ii, (int)jj, (int)kk, jb, kb, ncol, cols, xrow0, xrow1, current_stream());
}

int cedar_amd_relax3_masked_ok(const real_t *so, len_t ii, len_t jj, len_t kk)
{
	return (!so || is_device_ptr(so)) && relax3_masked_ok(so, (int)ii, (int)jj, (int)kk) ? 1 : 0;
}

int cedar_amd_relax3_planes_masked(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, len_t kk, int kb,
                                   int up, unsigned cols_f, unsigned cols_s, const int *rows)
{
	if (!is_device_ptr(so) || !is_device_ptr(q) || !is_device_ptr(qf) || !is_device_ptr(sor)) return 0; // registered operators only
	if (!relax3_masked_ok(so, (int)ii, (int)jj, (int)kk)) return 0;
	PsumSkip sk = psum_skip_none();
	sk.colsF = cols_f & 0xffu; sk.colsS = cols_s & 0xffu;
	for (int t = 0; t < 3; t++) sk.rows[t] = rows ? rows[t] : -1;
	return relax3_planes27_masked(so, qf, q, sor, (int)ii, (int)jj, (int)kk, kb, up, sk, current_stream()) ? 1 : 0;
}

int cedar_amd_relax3_prepare(const real_t *so, const real_t *sor, len_t ii, len_t jj, len_t kk)
{
	if (!is_device_ptr(so) || !is_device_ptr(sor)) return 0; // staged host arrays change address from call to call
	// CEDAR_AMD_ILV=0: no solve copy (the partial-sum scratch is still registered where the sweep wants it)
	return relax3_prepare(so, sor, (int)ii, (int)jj, (int)kk, ilv_min_rows_env(), current_stream());
}

int cedar_amd_relax3_prepare_rows(const real_t *so, const real_t *sor, len_t ii, len_t jj, len_t kk, int psum_min_rows)
{
	if (!is_device_ptr(so) || !is_device_ptr(sor)) return 0;
	return relax3_prepare_rows(so, sor, (int)ii, (int)jj, (int)kk, ilv_min_rows_env(), psum_min_rows, current_stream());
}

void cedar_amd_relax3_release(const real_t *so) { relax3_release(so); }

int cedar_amd_relax2_gs_psum(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, int updown)
{
	const size_t P = (size_t)ii * jj;
	Staged sso(so, P * 5, true, false), sqf(qf, P, true, false), sq(q, P, true, true), ssor(sor, P * 2, true, false);
	const int took = relax2_psum_wanted((int)ii, (int)jj) ? 1 : 0;
	relax2_gs9_psum(sso.get(), sqf.get(), sq.get(), ssor.get(), (int)ii, (int)jj, updown, current_stream());
	return took;
}

int cedar_amd_relax3_gs_psum(real_t *so, real_t *qf, real_t *q, real_t *sor, real_t *scratch, len_t ii, len_t jj, len_t kk,
                             int updown)
{
	const size_t P = (size_t)ii * jj * kk;
	const int frun = relax3_psum_frun((int)jj);
	Staged sso(so, P * 14, true, false), sqf(qf, P, true, false), sq(q, P, true, true), ssor(sor, P * 2, true, false);
	if (!relax3_psum_ok((int)ii, (int)jj, (int)kk, frun)) {
		relax3_gs(sso.get(), sqf.get(), sq.get(), ssor.get(), (int)ii, (int)jj, (int)kk, 14, updown, current_stream());
		return 0;
	}
	const ScratchLoan T(scratch, P);
	relax3_gs27_psum(op3_cedar(sso.get(), ssor.get(), (int)ii, (int)jj, (int)kk), sqf.get(), sq.get(), T.p, (int)ii, (int)jj,
	                 (int)kk, updown, frun, current_stream());
	return 1;
}

// ---- the 27-point sweep and residual on a single-precision copy of the operator (include/cedar_amd.h): the copy is
// built for the call and dropped after it (with_op32_copy)
int cedar_amd_relax3_gs_op32(real_t *so, real_t *qf, real_t *q, real_t *sor, real_t *scratch, len_t ii, len_t jj, len_t kk,
                             int updown, int frun)
{
	const int II = (int)ii, JJ = (int)jj, KK = (int)kk;
	const size_t P = (size_t)ii * jj * kk;
	Staged sso(so, P * 14, true, false), sqf(qf, P, true, false), sq(q, P, true, true), ssor(sor, P * 2, true, false);
	// the run length as relax3_psum_frun applies CEDAR_AMD_FRUN: a plane needs at least four runs
	const int run = (frun > 0 && JJ - 2 >= 4 * frun) ? frun : 0;
	const bool psum = relax3_psum_ok(II, JJ, KK, run);
	const bool ran = with_op32_copy(sso.get(), ssor.get() + P, II, JJ, KK, "cedar_amd_relax3_gs_op32", [&](const Op3f &A, hipStream_t st) {
		if (psum) {
			const ScratchLoan T(scratch, P);
			relax3_gs27_psum(A, sqf.get(), sq.get(), T.p, II, JJ, KK, updown, run, st);
		} else relax3_gs27_op(A, sqf.get(), sq.get(), II, JJ, KK, updown, st); // reference order: plane-fused or row kernels
	});
	return ran ? (psum ? 1 : 0) : -1;
}

int cedar_amd_residual3_op32(real_t *so, real_t *qf, real_t *q, real_t *res, len_t ii, len_t jj, len_t kk)
{
	const int II = (int)ii, JJ = (int)jj, KK = (int)kk;
	const size_t P = (size_t)ii * jj * kk;
	Staged sso(so, P * 14, true, false), sqf(qf, P, true, false), sq(q, P, true, false), sres(res, P, true, true);
	// 1/diag is not read by the residual: the copy's reciprocal row is filled from the operator's centre plane
	const bool ran = with_op32_copy(sso.get(), sso.get(), II, JJ, KK, "cedar_amd_residual3_op32", [&](const Op3f &A, hipStream_t st) {
		residual27_op(A, sqf.get(), sq.get(), sres.get(), II, JJ, KK, st);
	});
	return ran ? 0 : -1;
}

void cedar_amd_relax3_colour7(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, len_t kk, int pts)
{
	size_t P = (size_t)ii * jj * kk;
	Staged sso(so, P * 4, true, false), sqf(qf, P, true, false), sq(q, P, true, true), ssor(sor, P * 2, true, false);
	relax3_colour7(sso.get(), sqf.get(), sq.get(), ssor.get(), (int)ii, (int)jj, (int)kk, pts, current_stream());
}

void cedar_amd_setup_interp3_phase(real_t *so, real_t *ci, len_t iif, len_t jjf, len_t kkf,
                                   len_t iic, len_t jjc, len_t kkc, int ifd, int nstncl, int phase,
                                   int ilo, int jlo, int klo)
{
	size_t P = (size_t)iif * jjf * kkf, PC = (size_t)iic * jjc * kkc;
	Staged sso(so, P * nstncl, true, false), sci(ci, PC * 26, true, true);
	setup_interp3_phase(sso.get(), sci.get(), (int)iif, (int)jjf, (int)kkf, (int)iic, (int)jjc, (int)kkc, ifd,
	                    phase, ilo, jlo, klo, current_stream());
}

void cedar_amd_box_copy(real_t *arr, len_t ii, len_t jj, len_t kk, int nplanes, int nboxes,
                        const int *boxes, const unsigned long long *offsets, real_t *buf, int unpack)
{
	box_copy(arr, (int)ii, (int)jj, (int)kk, nplanes, nboxes, boxes, offsets, buf, unpack, current_stream());
}

void cedar_amd_box_copy_strided(real_t *arr, len_t ii, len_t jj, len_t kk, int nplanes, int nboxes,
                                const int *boxes, const unsigned long long *offsets, real_t *buf, int unpack)
{
	box_copy(arr, (int)ii, (int)jj, (int)kk, nplanes, nboxes, boxes, offsets, buf, unpack, current_stream(), 1);
}

// ------------------------------------------------------------------ the passes of a CG iteration (krylov.hip)
static_assert(CEDAR_AMD_PCG_RHO == PCG_RHO && CEDAR_AMD_PCG_SIGMA == PCG_SIGMA && CEDAR_AMD_PCG_ALPHA == PCG_ALPHA
                  && CEDAR_AMD_PCG_BETA == PCG_BETA && CEDAR_AMD_PCG_RR == PCG_RR && CEDAR_AMD_PCG_RZ == PCG_RZ
                  && CEDAR_AMD_PCG_FLAG == PCG_FLAG && CEDAR_AMD_PCG_WZ == PCG_WZ && CEDAR_AMD_PCG_NSC == PCG_NSC,
              "the scalar slots of include/cedar_amd.h are those of common.h");

namespace {

bool pcg_shape_refused(len_t ii, len_t jj, len_t kk, const char *who)
{
	if (ii >= 3 && jj >= 3 && (kk == 1 || kk >= 3) && (size_t)ii * jj * kk < ((size_t)1 << 31)) return false;
	char buf[200];
	snprintf(buf, sizeof(buf), "%s: extents %u x %u x %u (ghosts included) are not served; nothing done", who, (unsigned)ii,
	         (unsigned)jj, (unsigned)kk);
	report(buf);
	return true;
}

bool pcg_refuse(const char *who, const char *why)
{
	char buf[200];
	snprintf(buf, sizeof(buf), "%s: %s; nothing done", who, why);
	report(buf);
	return true;
}

// the partial-sum slab of one call: from the pool, every double a NaN (all bits set) before the launch
struct NanSlab {
	size_t n;
	real_t *dev;
	std::vector<uint64_t> host;
	explicit NanSlab(size_t doubles) : n(doubles), dev(static_cast<real_t *>(pool_get(doubles * sizeof(real_t)))), host(doubles, ~(uint64_t)0)
	{
		CEDAR_HIP_CHECK(hipMemcpyAsync(dev, host.data(), n * sizeof(real_t), hipMemcpyHostToDevice, current_stream()));
	}
	~NanSlab()
	{
		CEDAR_HIP_CHECK(hipStreamSynchronize(current_stream()));
		pool_put(dev, n * sizeof(real_t));
	}
};

} // namespace

int cedar_amd_pcg_direction(const real_t *so, const real_t *z, const real_t *p, real_t *pn, real_t *w, len_t ii, len_t jj,
                            len_t kk, int nstncl, int first, real_t *sc, real_t *partial)
{
	const char *who = "cedar_amd_pcg_direction";
	if (pcg_shape_refused(ii, jj, kk, who)) return -1;
	const int nd = kk == 1 ? 2 : 3;
	if (nd == 2 ? (nstncl != 3 && nstncl != 5) : (nstncl != 4 && nstncl != 14)) return pcg_refuse(who, "nstncl must be 3|5 (2D), 4|14 (3D)"), -1;
	if (!so || !z || !pn || !w || !sc || (!first && !p)) return pcg_refuse(who, "a required array is NULL"), -1;
	const size_t P = (size_t)ii * jj * kk;
	NanSlab slab(pcg_slab_doubles(nd, nstncl, (int)ii, (int)jj, (int)kk));
	Staged sso(so, P * nstncl, true, false), sz(z, P, true, false), sp(first ? nullptr : p, P, true, false),
	    spn(pn, P, true, true), sw(w, P, true, true), ssc(sc, PCG_NSC, true, partial == nullptr), spart(partial, 1, true, true);
	// the view the solvers hand over: the row-interleaved copy of a registered 27-point operator, else the planes
	const Op3 view = nstncl == 14 ? relax3_op_view(sso.get(), (int)ii, (int)jj, (int)kk) : Op3{};
	pcg_direction(sso.get(), nstncl == 14 ? &view : nullptr, sz.get(), sp.get(), spn.get(), sw.get(), nd, nstncl, (int)ii,
	              (int)jj, (int)kk, first != 0, slab.dev, ssc.get(), current_stream(), spart.get());
	return 0;
}

// the pass of a periodic level (krylov.hip pcg_direction_periodic); a 27-point operator is read from its Cedar planes
int cedar_amd_pcg_direction_periodic(const real_t *so, const real_t *z, const real_t *p, real_t *pn, real_t *w, len_t ii,
                                     len_t jj, len_t kk, int nstncl, int ibc, int first, real_t *sc, real_t *partial)
{
	const char *who = "cedar_amd_pcg_direction_periodic";
	if (ibc == 0) return cedar_amd_pcg_direction(so, z, p, pn, w, ii, jj, kk, nstncl, first, sc, partial);
	if (pcg_shape_refused(ii, jj, kk, who)) return -1;
	const int nd = kk == 1 ? 2 : 3;
	if (nd == 2 ? (ibc < 1 || ibc > 3) : (ibc < 1 || !periodic3_code_ok(ibc)))
		return pcg_refuse(who, "ibc must be 0..3 (2D), 0..3 or 5..8 (3D)"), -1;
	if (nd == 2 ? (nstncl != 3 && nstncl != 5) : (nstncl != 4 && nstncl != 14)) return pcg_refuse(who, "nstncl must be 3|5 (2D), 4|14 (3D)"), -1;
	if (!so || !z || !pn || !w || !sc || (!first && !p)) return pcg_refuse(who, "a required array is NULL"), -1;
	const size_t P = (size_t)ii * jj * kk;
	NanSlab slab(pcg_slab_doubles(nd, nstncl, (int)ii, (int)jj, (int)kk));
	Staged sso(so, P * nstncl, true, false), sz(z, P, true, false), sp(first ? nullptr : p, P, true, false),
	    spn(pn, P, true, true), sw(w, P, true, true), ssc(sc, PCG_NSC, true, partial == nullptr), spart(partial, 1, true, true);
	pcg_direction_periodic(sso.get(), sz.get(), sp.get(), spn.get(), sw.get(), nd, nstncl, (int)ii, (int)jj, (int)kk, ibc,
	                       first != 0, slab.dev, ssc.get(), current_stream(), spart.get());
	return 0;
}

int cedar_amd_pcg_update(int zmode, int move, real_t *x, real_t *r, const real_t *p, const real_t *w, real_t *z,
                         const real_t *diag, len_t ii, len_t jj, len_t kk, int first, real_t *sc, real_t *partial)
{
	const char *who = "cedar_amd_pcg_update";
	if (pcg_shape_refused(ii, jj, kk, who)) return -1;
	if (zmode < 0 || zmode > 3) return pcg_refuse(who, "zmode must be 0..3"), -1;
	if (!r || !sc || (move && (!x || !p || !w)) || ((zmode == 1 || zmode == 2) && !z) || (zmode == 1 && !diag))
		return pcg_refuse(who, "a required array is NULL"), -1;
	const size_t P = (size_t)ii * jj * kk;
	NanSlab slab(pcg_slab_doubles(kk == 1 ? 2 : 3, kk == 1 ? 3 : 4, (int)ii, (int)jj, (int)kk)); // any stencil: at least the update's share
	const bool mv = move != 0;
	Staged sx(mv ? x : nullptr, P, true, true), sr(r, P, true, mv), sp(mv ? p : nullptr, P, true, false),
	    sw(mv ? w : nullptr, P, true, false), sz(zmode == 1 || zmode == 2 ? z : nullptr, P, true, zmode == 1),
	    sd(zmode == 1 ? diag : nullptr, P, true, false), ssc(sc, PCG_NSC, true, partial == nullptr), spart(partial, 2, true, true);
	pcg_update(zmode, mv, sx.get(), sr.get(), sp.get(), sw.get(), sz.get(), sd.get(), (int)ii, (int)jj, (int)kk, first != 0,
	           slab.dev, ssc.get(), current_stream(), spart.get());
	return 0;
}

// the same two passes on nrhs items (krylov.hip *_many); every item's slab NaN-filled
int cedar_amd_pcg_direction_many(int nrhs, unsigned active, const real_t *so, const real_t *z, const real_t *p, real_t *pn,
                                 real_t *w, len_t ii, len_t jj, len_t kk, int nstncl, int first, real_t *sc)
{
	const char *who = "cedar_amd_pcg_direction_many";
	if (nrhs < 1 || nrhs > CEDAR_AMD_MAX_RHS) return pcg_refuse(who, "nrhs must be 1 .. 32"), -1;
	if (pcg_shape_refused(ii, jj, kk, who)) return -1;
	const int nd = kk == 1 ? 2 : 3;
	if (nd == 2 ? (nstncl != 3 && nstncl != 5) : (nstncl != 4 && nstncl != 14)) return pcg_refuse(who, "nstncl must be 3|5 (2D), 4|14 (3D)"), -1;
	if (!so || !z || !pn || !w || !sc || (!first && !p)) return pcg_refuse(who, "a required array is NULL"), -1;
	const size_t P = (size_t)ii * jj * kk, N = P * nrhs;
	NanSlab slab(pcg_slab_doubles(nd, nstncl, (int)ii, (int)jj, (int)kk) * nrhs);
	Staged sso(so, P * nstncl, true, false), sz(z, N, true, false), sp(first ? nullptr : p, N, true, false),
	    spn(pn, N, true, true), sw(w, N, true, true), ssc(sc, (size_t)PCG_NSC * nrhs, true, true);
	const Op3 view = nstncl == 14 ? relax3_op_view(sso.get(), (int)ii, (int)jj, (int)kk) : Op3{};
	pcg_direction_many(sso.get(), nstncl == 14 ? &view : nullptr, sz.get(), sp.get(), spn.get(), sw.get(), nd, nstncl, (int)ii,
	                   (int)jj, (int)kk, first != 0, slab.dev, ssc.get(), current_stream(), Batch{nrhs, P}, active);
	return 0;
}

int cedar_amd_pcg_update_many(int nrhs, unsigned active, int zmode, int move, real_t *x, real_t *r, const real_t *p,
                              const real_t *w, real_t *z, const real_t *diag, len_t ii, len_t jj, len_t kk, int first,
                              real_t *sc)
{
	const char *who = "cedar_amd_pcg_update_many";
	if (nrhs < 1 || nrhs > CEDAR_AMD_MAX_RHS) return pcg_refuse(who, "nrhs must be 1 .. 32"), -1;
	if (pcg_shape_refused(ii, jj, kk, who)) return -1;
	if (zmode < 0 || zmode > 3) return pcg_refuse(who, "zmode must be 0..3"), -1;
	if (!r || !sc || (move && (!x || !p || !w)) || ((zmode == 1 || zmode == 2) && !z) || (zmode == 1 && !diag))
		return pcg_refuse(who, "a required array is NULL"), -1;
	const size_t P = (size_t)ii * jj * kk, N = P * nrhs;
	NanSlab slab(pcg_slab_doubles(kk == 1 ? 2 : 3, kk == 1 ? 3 : 4, (int)ii, (int)jj, (int)kk) * nrhs);
	const bool mv = move != 0;
	Staged sx(mv ? x : nullptr, N, true, true), sr(r, N, true, mv), sp(mv ? p : nullptr, N, true, false),
	    sw(mv ? w : nullptr, N, true, false), sz(zmode == 1 || zmode == 2 ? z : nullptr, N, true, zmode == 1),
	    sd(zmode == 1 ? diag : nullptr, P, true, false), ssc(sc, (size_t)PCG_NSC * nrhs, true, true);
	pcg_update_many(zmode, mv, sx.get(), sr.get(), sp.get(), sw.get(), sz.get(), sd.get(), (int)ii, (int)jj, (int)kk,
	                first != 0, slab.dev, ssc.get(), current_stream(), Batch{nrhs, P}, active);
	return 0;
}

// the dots of flexible CG after the preconditioner (krylov.hip pcg_dwz / pcg_dwz_many); no vector is written
int cedar_amd_pcg_dots_wz(const real_t *r, const real_t *z, const real_t *w, len_t ii, len_t jj, len_t kk, int first, real_t *sc)
{
	const char *who = "cedar_amd_pcg_dots_wz";
	if (pcg_shape_refused(ii, jj, kk, who)) return -1;
	if (!r || !z || !w || !sc) return pcg_refuse(who, "a required array is NULL"), -1;
	const size_t P = (size_t)ii * jj * kk;
	NanSlab slab(pcg_slab_doubles(kk == 1 ? 2 : 3, kk == 1 ? 3 : 4, (int)ii, (int)jj, (int)kk));
	Staged sr(r, P, true, false), sz(z, P, true, false), sw(w, P, true, false), ssc(sc, PCG_NSC, true, true);
	pcg_dots_wz(sr.get(), sz.get(), sw.get(), (int)ii, (int)jj, (int)kk, first != 0, slab.dev, ssc.get(), current_stream());
	return 0;
}

int cedar_amd_pcg_dots_wz_many(int nrhs, unsigned active, const real_t *r, const real_t *z, const real_t *w, len_t ii, len_t jj,
                               len_t kk, int first, real_t *sc)
{
	const char *who = "cedar_amd_pcg_dots_wz_many";
	if (nrhs < 1 || nrhs > CEDAR_AMD_MAX_RHS) return pcg_refuse(who, "nrhs must be 1 .. 32"), -1;
	if (pcg_shape_refused(ii, jj, kk, who)) return -1;
	if (!r || !z || !w || !sc) return pcg_refuse(who, "a required array is NULL"), -1;
	const size_t P = (size_t)ii * jj * kk, N = P * nrhs;
	NanSlab slab(pcg_slab_doubles(kk == 1 ? 2 : 3, kk == 1 ? 3 : 4, (int)ii, (int)jj, (int)kk) * nrhs);
	Staged sr(r, N, true, false), sz(z, N, true, false), sw(w, N, true, false), ssc(sc, (size_t)PCG_NSC * nrhs, true, true);
	pcg_dots_wz_many(sr.get(), sz.get(), sw.get(), (int)ii, (int)jj, (int)kk, first != 0, slab.dev, ssc.get(), current_stream(),
	                 Batch{nrhs, P}, active);
	return 0;
}

int cedar_amd_pcg_rank_scalars(int which, int zmode, const real_t *gathered, int world, int stride, int first, real_t *sc)
{
	const char *who = "cedar_amd_pcg_rank_scalars";
	if (which < 0 || which > 1 || zmode < 0 || zmode > 3) return pcg_refuse(who, "which must be 0|1 and zmode 0..3"), -1;
	const int need = which == 1 && (zmode == 1 || zmode == 2) ? 2 : 1; // doubles read per rank
	if (!gathered || !sc || world < 1 || stride < need) return pcg_refuse(who, "world must be at least 1 and stride cover the partials"), -1;
	Staged sg(gathered, (size_t)world * stride, true, false), ssc(sc, PCG_NSC, true, true);
	if (which == 0) pcg_ranks_alpha(sg.get(), world, stride, ssc.get(), current_stream());
	else pcg_ranks_rho(zmode, sg.get(), world, stride, first != 0, ssc.get(), current_stream());
	return 0;
}

int cedar_amd_pcg_ghost_shell(const real_t *z, const real_t *p, real_t *pn, len_t ii, len_t jj, len_t kk, int first,
                              const real_t *sc, const int *boxes, int nboxes)
{
	const char *who = "cedar_amd_pcg_ghost_shell";
	if (pcg_shape_refused(ii, jj, kk, who)) return -1;
	if (!z || !pn || !sc || (!first && !p) || nboxes < 0 || nboxes > 26 || (nboxes && !boxes))
		return pcg_refuse(who, "a required array is NULL or there are more than 26 boxes"), -1;
	ShellBoxes bx;
	const long ext[3] = { (long)ii, (long)jj, (long)kk };
	for (int b = 0; b < nboxes; b++)
		for (int t = 0; t < 3; t++) {
			const long lo = boxes[6 * b + t], n = boxes[6 * b + 3 + t];
			if (lo < 0 || n < 1 || lo + n > ext[t]) return pcg_refuse(who, "a box reaches outside the array"), -1;
			bx.box[6 * b + t] = (int)lo;
			bx.box[6 * b + 3 + t] = (int)n;
		}
	bx.n = nboxes;
	const size_t P = (size_t)ii * jj * kk;
	Staged sz(z, P, true, false), sp(first ? nullptr : p, P, true, false), spn(pn, P, true, true), ssc(sc, PCG_NSC, true, false);
	pcg_ghost_shell(sz.get(), sp.get(), spn.get(), ssc.get(), bx, (int)ii, (int)jj, first != 0, current_stream());
	return 0;
}

// ------------------------------------------------------------------ the batched 3D kernels (many3d.hip), one launcher each
static bool many_args_refused(int nrhs, bool arrays_ok, bool nst_ok, const char *who)
{
	const char *why = nrhs < 1 || nrhs > CEDAR_AMD_MAX_RHS ? "nrhs must be 1 .. 32" : !nst_ok ? "nstncl must be 4 or 14"
	                  : !arrays_ok ? "a required array is NULL" : nullptr;
	if (!why) return false;
	char msg[200];
	snprintf(msg, sizeof(msg), "%s: %s; nothing done", who, why);
	print_error(msg);
	return true;
}

int cedar_amd_relax3_gs_many(int nrhs, real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, len_t kk, int nstncl,
                             int updown)
{
	if (many_args_refused(nrhs, so && qf && q && sor, nstncl == 4 || nstncl == 14, "cedar_amd_relax3_gs_many")) return -1;
	const size_t P = (size_t)ii * jj * kk;
	Staged sso(so, P * nstncl, true, false), sqf(qf, P * nrhs, true, false), sq(q, P * nrhs, true, true), ssor(sor, P * 2, true, false);
	const Batch bt{nrhs, P};
	if (nstncl == 14)
		relax3_gs27_many(op3_cedar(sso.get(), ssor.get(), (int)ii, (int)jj, (int)kk), sqf.get(), sq.get(), (int)ii, (int)jj, (int)kk,
		                 updown, current_stream(), bt);
	else relax3_gs7_many(sso.get(), sqf.get(), sq.get(), ssor.get(), (int)ii, (int)jj, (int)kk, updown, current_stream(), bt);
	return 0;
}

int cedar_amd_residual3_many(int nrhs, real_t *so, real_t *qf, real_t *q, real_t *res, len_t ii, len_t jj, len_t kk, int nstncl)
{
	if (many_args_refused(nrhs, so && qf && q && res, nstncl == 4 || nstncl == 14, "cedar_amd_residual3_many")) return -1;
	const size_t P = (size_t)ii * jj * kk;
	Staged sso(so, P * nstncl, true, false), sqf(qf, P * nrhs, true, false), sq(q, P * nrhs, true, false), sr(res, P * nrhs, true, true);
	const Batch bt{nrhs, P};
	if (nstncl == 14)
		residual27_many(op3_cedar(sso.get(), nullptr, (int)ii, (int)jj, (int)kk), sqf.get(), sq.get(), sr.get(), (int)ii, (int)jj,
		                (int)kk, current_stream(), bt);
	else residual7_many(sso.get(), sqf.get(), sq.get(), sr.get(), (int)ii, (int)jj, (int)kk, current_stream(), bt);
	return 0;
}

// the two 27-point ones on a single-precision copy of the operator built for the call (with_op32_copy), reference order
int cedar_amd_relax3_gs_many_op32(int nrhs, real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, len_t kk, int updown)
{
	const char *who = "cedar_amd_relax3_gs_many_op32";
	if (many_args_refused(nrhs, so && qf && q && sor, true, who)) return -1;
	const int II = (int)ii, JJ = (int)jj, KK = (int)kk;
	const size_t P = (size_t)ii * jj * kk;
	Staged sso(so, P * 14, true, false), sqf(qf, P * nrhs, true, false), sq(q, P * nrhs, true, true), ssor(sor, P * 2, true, false);
	const bool ran = with_op32_copy(sso.get(), ssor.get() + P, II, JJ, KK, who, [&](const Op3f &A, hipStream_t st) {
		relax3_gs27_many(A, sqf.get(), sq.get(), II, JJ, KK, updown, st, Batch{nrhs, P});
	});
	return ran ? 0 : -1;
}

int cedar_amd_residual3_many_op32(int nrhs, real_t *so, real_t *qf, real_t *q, real_t *res, len_t ii, len_t jj, len_t kk)
{
	const char *who = "cedar_amd_residual3_many_op32";
	if (many_args_refused(nrhs, so && qf && q && res, true, who)) return -1;
	const int II = (int)ii, JJ = (int)jj, KK = (int)kk;
	const size_t P = (size_t)ii * jj * kk;
	Staged sso(so, P * 14, true, false), sqf(qf, P * nrhs, true, false), sq(q, P * nrhs, true, false), sr(res, P * nrhs, true, true);
	// 1/diag is not read by the residual: the copy's reciprocal row is filled from the operator's centre plane
	const bool ran = with_op32_copy(sso.get(), sso.get(), II, JJ, KK, who, [&](const Op3f &A, hipStream_t st) {
		residual27_many(A, sqf.get(), sq.get(), sr.get(), II, JJ, KK, st, Batch{nrhs, P});
	});
	return ran ? 0 : -1;
}

// ---- the 7-point sweep and residual on a single-precision copy of the operator built for the call (with_op7f_copy;
// include/cedar_amd.h); many: the batched kernel (the _many entry points, also with nrhs = 1), else the single-vector one
static int relax7_op32(const char *who, bool many, int nrhs, real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, len_t kk, int updown)
{
	if (many_args_refused(nrhs, so && qf && q && sor, true, who)) return -1;
	const int II = (int)ii, JJ = (int)jj, KK = (int)kk;
	const size_t P = (size_t)ii * jj * kk;
	Staged sso(so, P * 4, true, false), sqf(qf, P * nrhs, true, false), sq(q, P * nrhs, true, true), ssor(sor, P * 2, true, false);
	const bool ran = with_op7f_copy(sso.get(), ssor.get() + P, II, JJ, KK, who, [&](const Op7f &A, hipStream_t st) {
		if (many) relax3_gs7_many(A, sqf.get(), sq.get(), II, JJ, KK, updown, st, Batch{nrhs, P});
		else relax3_gs7_op(A, sqf.get(), sq.get(), II, JJ, KK, updown, st);
	});
	return ran ? 0 : -1;
}

static int residual7_op32(const char *who, bool many, int nrhs, real_t *so, real_t *qf, real_t *q, real_t *res, len_t ii, len_t jj, len_t kk)
{
	if (many_args_refused(nrhs, so && qf && q && res, true, who)) return -1;
	const int II = (int)ii, JJ = (int)jj, KK = (int)kk;
	const size_t P = (size_t)ii * jj * kk;
	Staged sso(so, P * 4, true, false), sqf(qf, P * nrhs, true, false), sq(q, P * nrhs, true, false), sr(res, P * nrhs, true, true);
	// 1/diag is not read by the residual: the copy's reciprocal row is filled from the operator's centre plane
	const bool ran = with_op7f_copy(sso.get(), sso.get(), II, JJ, KK, who, [&](const Op7f &A, hipStream_t st) {
		if (many) residual7_many(A, sqf.get(), sq.get(), sr.get(), II, JJ, KK, st, Batch{nrhs, P});
		else residual7_op(A, sqf.get(), sq.get(), sr.get(), II, JJ, KK, st);
	});
	return ran ? 0 : -1;
}

int cedar_amd_relax7_gs_op32(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, len_t kk, int updown)
{
	return relax7_op32("cedar_amd_relax7_gs_op32", false, 1, so, qf, q, sor, ii, jj, kk, updown);
}

int cedar_amd_residual7_op32(real_t *so, real_t *qf, real_t *q, real_t *res, len_t ii, len_t jj, len_t kk)
{
	return residual7_op32("cedar_amd_residual7_op32", false, 1, so, qf, q, res, ii, jj, kk);
}

int cedar_amd_relax7_gs_many_op32(int nrhs, real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, len_t kk, int updown)
{
	return relax7_op32("cedar_amd_relax7_gs_many_op32", true, nrhs, so, qf, q, sor, ii, jj, kk, updown);
}

int cedar_amd_residual7_many_op32(int nrhs, real_t *so, real_t *qf, real_t *q, real_t *res, len_t ii, len_t jj, len_t kk)
{
	return residual7_op32("cedar_amd_residual7_many_op32", true, nrhs, so, qf, q, res, ii, jj, kk);
}

// ---- the 2D point sweep and residual on a single-precision copy of the operator built for the call (common.h Op2f,
// op2f.hip; include/cedar_amd.h).  kind 0: reference-order sweep, 1: partial-sum sweep (returns 1 where it ran), 2: residual
static int op32_2d(const char *who, int kind, int nrhs, real_t *so, real_t *qf, real_t *q, real_t *out, len_t ii, len_t jj,
                   int nstncl, int updown)
{
	const char *why = nrhs < 1 || nrhs > CEDAR_AMD_MAX_RHS ? "nrhs must be 1 .. 32"
	                  : nstncl != 3 && nstncl != 5 ? "nstncl must be 3 or 5"
	                  : !(so && qf && q && out) ? "a required array is NULL" : nullptr;
	char buf[200];
	if (why) {
		snprintf(buf, sizeof(buf), "%s: %s; nothing done", who, why);
		report(buf);
		return -1;
	}
	const int II = (int)ii, JJ = (int)jj;
	const size_t P = (size_t)ii * jj;
	const bool resid = kind == 2;
	// `out`: 1/diag's array for the sweeps (read), the residual's result (written)
	Staged sso(so, P * nstncl, true, false), sqf(qf, P * nrhs, true, false), sq(q, P * nrhs, true, !resid),
	    sout(out, resid ? P * nrhs : P * 2, true, resid);
	hipStream_t st = current_stream();
	const size_t bytes = op2f_floats(II, JJ, nstncl) * sizeof(float);
	float *c = static_cast<float *>(pool_get(bytes));
	int *flag = static_cast<int *>(pool_get(sizeof(int))), host = 0;
	CEDAR_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(int), st));
	// 1/diag is not read by the residual: the copy's reciprocal row is filled from the operator's centre plane
	op2f_build(sso.get(), resid ? sso.get() : sout.get() + P, c, II, JJ, nstncl, flag, st);
	CEDAR_HIP_CHECK(hipMemcpyAsync(&host, flag, sizeof(int), hipMemcpyDeviceToHost, st));
	CEDAR_HIP_CHECK(hipStreamSynchronize(st));
	pool_put(flag, sizeof(int));
	int ret = 0;
	if (host) {
		snprintf(buf, sizeof(buf), "%s: an entry of the operator or of 1/diag overflows single precision; nothing done", who);
		report(buf);
		ret = -1; // (staged host arrays go back as they came)
	} else {
		const Op2f A = op2f_view(c, II, nstncl);
		const Batch bt{nrhs, P};
		if (kind == 0) relax2_gs_op(A, sqf.get(), sq.get(), II, JJ, nstncl, updown, st, bt);
		else if (kind == 1) {
			ret = relax2_psum_wanted(II, JJ) ? 1 : 0;
			relax2_gs9_psum_op(A, sqf.get(), sq.get(), II, JJ, updown, st, bt);
		} else residual2_op(A, sqf.get(), sq.get(), sout.get(), II, JJ, nstncl, st, bt);
		CEDAR_HIP_CHECK(hipStreamSynchronize(st));
	}
	pool_put(c, bytes);
	return ret;
}

int cedar_amd_relax2_gs_op32(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, int nstncl, int updown)
{
	return op32_2d("cedar_amd_relax2_gs_op32", 0, 1, so, qf, q, sor, ii, jj, nstncl, updown);
}

int cedar_amd_relax2_gs_psum_op32(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, int updown)
{
	return op32_2d("cedar_amd_relax2_gs_psum_op32", 1, 1, so, qf, q, sor, ii, jj, 5, updown);
}

int cedar_amd_residual2_op32(real_t *so, real_t *qf, real_t *q, real_t *res, len_t ii, len_t jj, int nstncl)
{
	return op32_2d("cedar_amd_residual2_op32", 2, 1, so, qf, q, res, ii, jj, nstncl, 0);
}

int cedar_amd_relax2_gs_many_op32(int nrhs, real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, int nstncl, int updown)
{
	return op32_2d("cedar_amd_relax2_gs_many_op32", 0, nrhs, so, qf, q, sor, ii, jj, nstncl, updown);
}

int cedar_amd_residual2_many_op32(int nrhs, real_t *so, real_t *qf, real_t *q, real_t *res, len_t ii, len_t jj, int nstncl)
{
	return op32_2d("cedar_amd_residual2_many_op32", 2, nrhs, so, qf, q, res, ii, jj, nstncl, 0);
}

// ---- one zebra line sweep on single-precision copies of the operator and the line factors built for the call
// (linesf.hip; include/cedar_amd.h).  dir 0: x lines; dir 1: y lines on transposed arrays (sor = SOR(JJ,II,2))
static int op32_lines(const char *who, int nrhs, real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, int nstncl,
                      int dir, int updown)
{
	const int II = (int)ii, JJ = (int)jj;
	const int n = dir ? JJ - 2 : II - 2, nlines = dir ? II - 2 : JJ - 2; // unknowns of a line, lines
	const char *why = nrhs < 1 || nrhs > CEDAR_AMD_MAX_RHS ? "nrhs must be 1 .. 32"
	                  : nstncl != 3 && nstncl != 5 ? "nstncl must be 3 or 5"
	                  : !(so && qf && q && sor) ? "a required array is NULL"
	                  : dir != 0 && dir != 1 ? "dir must be 0 (x lines) or 1 (y lines)"
	                  : n > 0 && !line_fits_lds_host(n) ? "a line does not fit the 160 KB LDS of a CU" : nullptr;
	char buf[200];
	if (why) {
		snprintf(buf, sizeof(buf), "%s: %s; nothing done", who, why);
		report(buf);
		return -1;
	}
	if (II < 3 || JJ < 3) return 0; // no unknowns
	const size_t P = (size_t)ii * jj;
	Staged sso(so, P * nstncl, true, false), sqf(qf, P * nrhs, true, false), sq(q, P * nrhs, true, true), ssor(sor, P * 2, true, false);
	hipStream_t st = current_stream();
	// the grid the kernel sees: for y lines the transposed one (JJ fast)
	const int GI = dir ? JJ : II, GJ = dir ? II : JJ;
	const size_t abytes = op2f_floats(GI, GJ, nstncl) * sizeof(float);
	const size_t npf = lines_permuted_doubles(n, nlines);
	const size_t fbytes = (npf ? npf : P * 2) * sizeof(float);
	const size_t tbytes = dir ? P * sizeof(real_t) : 0; // transposed planes, right-hand sides and scratch for q^T
	float *c = static_cast<float *>(pool_get(abytes)), *f = static_cast<float *>(pool_get(fbytes));
	real_t *sot = dir ? static_cast<real_t *>(pool_get(tbytes * nstncl)) : nullptr;
	real_t *qft = dir ? static_cast<real_t *>(pool_get(tbytes * nrhs)) : nullptr, *qt = dir ? static_cast<real_t *>(pool_get(tbytes * nrhs)) : nullptr;
	int *flag = static_cast<int *>(pool_get(sizeof(int))), host = 0;
	CEDAR_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(int), st));
	const Batch bt{nrhs, P};
	if (dir) {
		zero_fill(sot, P * nstncl, st); // (the centre plane is not transposed: setup_lines_yt)
		setup_lines_yt(sso.get(), sot, II, JJ, nstncl, st);
		transpose2(sqf.get(), qft, II, JJ, st, bt);
	}
	op2f_build(dir ? sot : sso.get(), nullptr, c, GI, GJ, nstncl, flag, st);
	if (npf) linesf_permute(ssor.get(), f, n, GI, nlines, P, flag, st);
	else linesf_image(ssor.get(), f, II, JJ, flag, st);
	CEDAR_HIP_CHECK(hipMemcpyAsync(&host, flag, sizeof(int), hipMemcpyDeviceToHost, st));
	CEDAR_HIP_CHECK(hipStreamSynchronize(st));
	pool_put(flag, sizeof(int));
	int ret = 0;
	if (host) {
		snprintf(buf, sizeof(buf), "%s: an entry of the operator or of a line factor overflows single precision; nothing done", who);
		report(buf);
		ret = -1; // (staged host arrays go back as they came)
	} else {
		const Op2f A = op2f_view(c, GI, nstncl);
		const float *fs = npf ? nullptr : f, *fp = npf ? f : nullptr;
		if (dir) relax_lines_yt_op(A, qft, sq.get(), qt, fs, II, JJ, nstncl, updown, st, fp, bt);
		else relax_lines_x_op(A, sqf.get(), sq.get(), fs, II, JJ, nstncl, updown, st, fp, bt);
		CEDAR_HIP_CHECK(hipStreamSynchronize(st));
	}
	if (dir) { pool_put(sot, tbytes * nstncl); pool_put(qft, tbytes * nrhs); pool_put(qt, tbytes * nrhs); }
	pool_put(c, abytes); pool_put(f, fbytes);
	return ret;
}

int cedar_amd_relax2_lines_op32(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, int nstncl, int dir, int updown)
{
	return op32_lines("cedar_amd_relax2_lines_op32", 1, so, qf, q, sor, ii, jj, nstncl, dir, updown);
}

int cedar_amd_relax2_lines_many_op32(int nrhs, real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, int nstncl,
                                     int dir, int updown)
{
	return op32_lines("cedar_amd_relax2_lines_many_op32", nrhs, so, qf, q, sor, ii, jj, nstncl, dir, updown);
}

int cedar_amd_restrict3_many(int nrhs, real_t *q, real_t *qc, real_t *ci, len_t ii, len_t jj, len_t kk, len_t iic, len_t jjc,
                             len_t kkc)
{
	if (many_args_refused(nrhs, q && qc && ci, true, "cedar_amd_restrict3_many")) return -1;
	const size_t P = (size_t)ii * jj * kk, PC = (size_t)iic * jjc * kkc;
	Staged sq(q, P * nrhs, true, false), sqc(qc, PC * nrhs, true, true), sci(ci, PC * 26, true, false);
	restrict3_many(sq.get(), sqc.get(), sci.get(), (int)ii, (int)jj, (int)kk, (int)iic, (int)jjc, (int)kkc, current_stream(),
	               Batch{nrhs, P}, Batch{nrhs, PC});
	return 0;
}

int cedar_amd_interp_add3_many(int nrhs, real_t *q, real_t *qc, real_t *so, real_t *res, real_t *ci, len_t iic, len_t jjc,
                               len_t kkc, len_t iif, len_t jjf, len_t kkf, int nstncl)
{
	if (many_args_refused(nrhs, q && qc && so && res && ci, nstncl == 4 || nstncl == 14, "cedar_amd_interp_add3_many")) return -1;
	const size_t P = (size_t)iif * jjf * kkf, PC = (size_t)iic * jjc * kkc;
	Staged sq(q, P * nrhs, true, true), sqc(qc, PC * nrhs, true, false), sso(so, P * nstncl, true, false),
	    sr(res, P * nrhs, true, true), sci(ci, PC * 26, true, false);
	interp_add3_many(sq.get(), sqc.get(), sso.get(), sr.get(), sci.get(), (int)iic, (int)jjc, (int)kkc, (int)iif, (int)jjf,
	                 (int)kkf, current_stream(), Batch{nrhs, P}, Batch{nrhs, PC});
	return 0;
}

// ------------------------------------------------------------------ the batched periodic 3D kernels (periodic_many3d.hip,
// periodic3d.hip's coarsest solve, krylov.hip), one launcher each: nrhs items back to back, the operator arrays shared;
// ibc = 0 forwards to the Dirichlet call where one exists
static bool per_many_refused(int nrhs, bool arrays_ok, bool nst_ok, int ibc, const char *who)
{
	if (many_args_refused(nrhs, arrays_ok, nst_ok, who)) return true;
	if (ibc >= 0 && periodic3_code_ok(ibc)) return false;
	char msg[200];
	snprintf(msg, sizeof(msg), "%s: boundary code %d is not a 3D code (0, 1..3, 5..8); nothing done", who, ibc);
	print_error(msg);
	return true;
}

int cedar_amd_relax3_gs_periodic_many(int nrhs, real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, len_t kk,
                                      int nstncl, int updown, int ibc, int ghosts_consistent)
{
	if (per_many_refused(nrhs, so && qf && q && sor, nstncl == 4 || nstncl == 14, ibc, "cedar_amd_relax3_gs_periodic_many")) return -1;
	if (ibc == 0) return cedar_amd_relax3_gs_many(nrhs, so, qf, q, sor, ii, jj, kk, nstncl, updown);
	const size_t P = (size_t)ii * jj * kk;
	Staged sso(so, P * nstncl, true, false), sqf(qf, P * nrhs, true, false), sq(q, P * nrhs, true, true), ssor(sor, P * 2, true, false);
	relax3_gs_per_many(sso.get(), sqf.get(), sq.get(), ssor.get(), (int)ii, (int)jj, (int)kk, nstncl, updown, ibc, current_stream(),
	                   ghosts_consistent, Batch{nrhs, P});
	return 0;
}

// the fine vectors get their ghosts refreshed first, so q is an output too
int cedar_amd_restrict3_periodic_many(int nrhs, real_t *q, real_t *qc, real_t *ci, len_t ii, len_t jj, len_t kk, len_t iic,
                                      len_t jjc, len_t kkc, int ibc)
{
	if (per_many_refused(nrhs, q && qc && ci, true, ibc, "cedar_amd_restrict3_periodic_many")) return -1;
	if (ibc == 0) return cedar_amd_restrict3_many(nrhs, q, qc, ci, ii, jj, kk, iic, jjc, kkc);
	const size_t P = (size_t)ii * jj * kk, PC = (size_t)iic * jjc * kkc;
	Staged sq(q, P * nrhs, true, true), sqc(qc, PC * nrhs, true, true), sci(ci, PC * 26, true, false);
	restrict3_per_many(sq.get(), sqc.get(), sci.get(), (int)ii, (int)jj, (int)kk, (int)iic, (int)jjc, (int)kkc, ibc,
	                   current_stream(), Batch{nrhs, P}, Batch{nrhs, PC});
	return 0;
}

int cedar_amd_interp_add3_periodic_many(int nrhs, real_t *q, real_t *qc, real_t *so, real_t *res, real_t *ci, len_t iic,
                                        len_t jjc, len_t kkc, len_t iif, len_t jjf, len_t kkf, int nstncl, int ibc)
{
	if (per_many_refused(nrhs, q && qc && so && res && ci, nstncl == 4 || nstncl == 14, ibc, "cedar_amd_interp_add3_periodic_many"))
		return -1;
	if (ibc == 0) return cedar_amd_interp_add3_many(nrhs, q, qc, so, res, ci, iic, jjc, kkc, iif, jjf, kkf, nstncl);
	const size_t P = (size_t)iif * jjf * kkf, PC = (size_t)iic * jjc * kkc;
	Staged sq(q, P * nrhs, true, true), sqc(qc, PC * nrhs, true, false), sso(so, P * nstncl, true, false),
	    sr(res, P * nrhs, true, true), sci(ci, PC * 26, true, false);
	interp_add3_per_many(sq.get(), sqc.get(), sso.get(), sr.get(), sci.get(), (int)iic, (int)jjc, (int)kkc, (int)iif, (int)jjf,
	                     (int)kkf, ibc, current_stream(), Batch{nrhs, P}, Batch{nrhs, PC});
	return 0;
}

// abd: the dense factor of BMG3_SymStd_SETUP_cg_LU with a periodic code, nabd1 >= the number of unknowns; bbd: nrhs
// segments of that many doubles.  There is no batched Dirichlet coarsest solve behind a kernel-level call: ibc = 0 is refused
int cedar_amd_solve_cg3_periodic_many(int nrhs, real_t *q, real_t *qf, len_t ii, len_t jj, len_t kk, real_t *abd, real_t *bbd,
                                      len_t nabd1, int ibc)
{
	const char *who = "cedar_amd_solve_cg3_periodic_many";
	if (per_many_refused(nrhs, q && qf && abd && bbd, true, ibc, who)) return -1;
	const size_t N = ii >= 3 && jj >= 3 && kk >= 3 ? (size_t)(ii - 2) * (jj - 2) * (kk - 2) : 0;
	if (ibc == 0 || N == 0 || N > 2048 || (size_t)nabd1 < N) {
		char msg[200];
		snprintf(msg, sizeof(msg), "%s: needs a periodic code, 1 .. 2048 unknowns and the dense factor ABD(n,n); nothing done", who);
		print_error(msg);
		return -1;
	}
	const size_t P = (size_t)ii * jj * kk;
	Staged sq(q, P * nrhs, true, true), sqf(qf, P * nrhs, true, false), sabd(abd, (size_t)nabd1 * N, true, false),
	    sb(bbd, N * nrhs, false, true);
	solve_cg3_per(sq.get(), sqf.get(), (int)ii, (int)jj, (int)kk, sabd.get(), sb.get(), (int)nabd1, ibc, current_stream(),
	              Batch{nrhs, P});
	return 0;
}

// the direction pass of a periodic 3D level on nrhs items; every item's slab NaN-filled
int cedar_amd_pcg_direction_periodic_many(int nrhs, unsigned active, const real_t *so, const real_t *z, const real_t *p,
                                          real_t *pn, real_t *w, len_t ii, len_t jj, len_t kk, int nstncl, int ibc, int first,
                                          real_t *sc)
{
	const char *who = "cedar_amd_pcg_direction_periodic_many";
	if (per_many_refused(nrhs, so && z && pn && w && sc && (first || p), nstncl == 4 || nstncl == 14, ibc, who)) return -1;
	if (ibc == 0) return cedar_amd_pcg_direction_many(nrhs, active, so, z, p, pn, w, ii, jj, kk, nstncl, first, sc);
	if (kk == 1 || pcg_shape_refused(ii, jj, kk, who)) return kk == 1 ? (pcg_refuse(who, "3D only"), -1) : -1;
	const size_t P = (size_t)ii * jj * kk, N = P * nrhs;
	NanSlab slab(pcg_slab_doubles(3, nstncl, (int)ii, (int)jj, (int)kk) * nrhs);
	Staged sso(so, P * nstncl, true, false), sz(z, N, true, false), sp(first ? nullptr : p, N, true, false),
	    spn(pn, N, true, true), sw(w, N, true, true), ssc(sc, (size_t)PCG_NSC * nrhs, true, true);
	pcg_direction_periodic_many(sso.get(), sz.get(), sp.get(), spn.get(), sw.get(), 3, nstncl, (int)ii, (int)jj, (int)kk, ibc,
	                            first != 0, slab.dev, ssc.get(), current_stream(), Batch{nrhs, P}, active);
	return 0;
}

// ------------------------------------------------------------------ the batched periodic 2D kernels (periodic_many2d.hip,
// periodic2d.hip's transfers and coarsest solve, krylov.hip), one launcher each: nrhs items back to back with stride ii*jj,
// the operator arrays shared.  Only the direction pass has a Dirichlet batched twin behind a kernel-level call: the other
// four refuse ibc = 0
static bool per_many2_refused(int nrhs, bool arrays_ok, bool nst_ok, int ibc, bool dirichlet_twin, const char *who)
{
	const char *why = nrhs < 1 || nrhs > CEDAR_AMD_MAX_RHS ? "nrhs must be 1 .. 32" : !nst_ok ? "nstncl must be 3 or 5"
	                  : !arrays_ok ? "a required array is NULL" : ibc < 0 || ibc > 3 ? "the 2D boundary codes are 0 .. 3"
	                  : ibc == 0 && !dirichlet_twin ? "ibc = 0 has no batched Dirichlet kernel-level call to go to" : nullptr;
	if (!why) return false;
	char msg[200];
	snprintf(msg, sizeof(msg), "%s: %s; nothing done", who, why);
	print_error(msg);
	return true;
}

int cedar_amd_relax2_gs_periodic_many(int nrhs, real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, int nstncl,
                                      int updown, int ibc)
{
	const char *who = "cedar_amd_relax2_gs_periodic_many";
	if (per_many2_refused(nrhs, so && qf && q && sor, nstncl == 3 || nstncl == 5, ibc, false, who)) return -1;
	if ((size_t)ii * sizeof(real_t) > 64 * 1024) {
		char msg[200];
		snprintf(msg, sizeof(msg), "%s: periodic rows longer than 8192 points are not supported; nothing done", who);
		print_error(msg);
		return -1;
	}
	const size_t P = (size_t)ii * jj;
	Staged sso(so, P * nstncl, true, false), sqf(qf, P * nrhs, true, false), sq(q, P * nrhs, true, true), ssor(sor, P * 2, true, false);
	relax2_gs_per_many(sso.get(), sqf.get(), sq.get(), ssor.get(), (int)ii, (int)jj, nstncl, updown, ibc, current_stream(),
	                   Batch{nrhs, P});
	return 0;
}

// the fine vectors get their ghosts refreshed first, so q is an output too
int cedar_amd_restrict2_periodic_many(int nrhs, real_t *q, real_t *qc, real_t *ci, len_t ii, len_t jj, len_t iic, len_t jjc, int ibc)
{
	if (per_many2_refused(nrhs, q && qc && ci, true, ibc, false, "cedar_amd_restrict2_periodic_many")) return -1;
	const size_t P = (size_t)ii * jj, PC = (size_t)iic * jjc;
	Staged sq(q, P * nrhs, true, true), sqc(qc, PC * nrhs, true, true), sci(ci, PC * 8, true, false);
	restrict2_per(sq.get(), sqc.get(), sci.get(), (int)ii, (int)jj, (int)iic, (int)jjc, ibc, current_stream(), Batch{nrhs, P},
	              Batch{nrhs, PC});
	return 0;
}

int cedar_amd_interp_add2_periodic_many(int nrhs, real_t *q, real_t *qc, real_t *res, real_t *so, real_t *ci, len_t iic, len_t jjc,
                                        len_t ii, len_t jj, int nstncl, int ibc)
{
	const char *who = "cedar_amd_interp_add2_periodic_many";
	if (per_many2_refused(nrhs, q && qc && res && so && ci, nstncl == 3 || nstncl == 5, ibc, false, who)) return -1;
	const size_t P = (size_t)ii * jj, PC = (size_t)iic * jjc;
	Staged sq(q, P * nrhs, true, true), sqc(qc, PC * nrhs, true, false), sr(res, P * nrhs, true, true),
	    sso(so, P * nstncl, true, false), sci(ci, PC * 8, true, false);
	interp_add2_per(sq.get(), sqc.get(), sr.get(), sso.get(), sci.get(), (int)iic, (int)jjc, (int)ii, (int)jj, ibc,
	                current_stream(), Batch{nrhs, P}, Batch{nrhs, PC});
	return 0;
}

// abd: the dense factor of BMG2_SymStd_SETUP_cg_LU with a periodic code, nabd1 >= the number of unknowns; bbd: nrhs segments
// of that many doubles
int cedar_amd_solve_cg2_periodic_many(int nrhs, real_t *q, real_t *qf, len_t ii, len_t jj, real_t *abd, real_t *bbd, len_t nabd1,
                                      int ibc)
{
	const char *who = "cedar_amd_solve_cg2_periodic_many";
	if (per_many2_refused(nrhs, q && qf && abd && bbd, true, ibc, false, who)) return -1;
	const size_t N = ii >= 3 && jj >= 3 ? (size_t)(ii - 2) * (jj - 2) : 0;
	if (N == 0 || (size_t)nabd1 < N) {
		char msg[200];
		snprintf(msg, sizeof(msg), "%s: needs at least one unknown and the dense factor ABD(n,n); nothing done", who);
		print_error(msg);
		return -1;
	}
	const size_t P = (size_t)ii * jj;
	Staged sq(q, P * nrhs, true, true), sqf(qf, P * nrhs, true, false), sabd(abd, (size_t)nabd1 * N, true, false),
	    sb(bbd, N * nrhs, false, true);
	solve_cg2_per(sq.get(), sqf.get(), (int)ii, (int)jj, sabd.get(), sb.get(), (int)nabd1, ibc, current_stream(),
	              Batch{nrhs, P});
	return 0;
}

// v := v - mean_interior(v) on the items of `active` (util.hip project_mean_many); kk = 1: a 2D level
int cedar_amd_project_mean(int nrhs, unsigned active, real_t *v, len_t ii, len_t jj, len_t kk, real_t *mean)
{
	if (nrhs < 1 || nrhs > CEDAR_AMD_MAX_RHS || !v || ii < 3 || jj < 3 || (kk != 1 && kk < 3)) {
		char msg[] = "cedar_amd_project_mean: nrhs must be 1 .. 32, v not NULL and every extent at least 3 (kk = 1: 2D); nothing done";
		print_error(msg);
		return -1;
	}
	const size_t P = (size_t)ii * jj * kk;
	Staged sv(v, P * nrhs, true, true);
	ScratchLoan scratch(nullptr, project_mean_doubles(nrhs));
	hipStream_t st = current_stream();
	project_mean_many(sv.get(), (int)ii, (int)jj, (int)kk, scratch.p, st, Batch{nrhs, P}, active);
	if (mean) {
		CEDAR_HIP_CHECK(hipMemcpyAsync(mean, scratch.p + 2 * (size_t)nrhs * PROJECT_MEAN_NB, nrhs * sizeof(real_t), hipMemcpyDefault, st));
		CEDAR_HIP_CHECK(hipStreamSynchronize(st));
	}
	return 0;
}

// the direction pass of a periodic 2D level on nrhs items; every item's slab NaN-filled
int cedar_amd_pcg_direction2_periodic_many(int nrhs, unsigned active, const real_t *so, const real_t *z, const real_t *p,
                                           real_t *pn, real_t *w, len_t ii, len_t jj, int nstncl, int ibc, int first, real_t *sc)
{
	const char *who = "cedar_amd_pcg_direction2_periodic_many";
	if (per_many2_refused(nrhs, so && z && pn && w && sc && (first || p), nstncl == 3 || nstncl == 5, ibc, true, who)) return -1;
	if (ibc == 0) return cedar_amd_pcg_direction_many(nrhs, active, so, z, p, pn, w, ii, jj, 1, nstncl, first, sc);
	if (pcg_shape_refused(ii, jj, 1, who)) return -1;
	const size_t P = (size_t)ii * jj, N = P * nrhs;
	NanSlab slab(pcg_slab_doubles(2, nstncl, (int)ii, (int)jj, 1) * nrhs);
	Staged sso(so, P * nstncl, true, false), sz(z, N, true, false), sp(first ? nullptr : p, N, true, false),
	    spn(pn, N, true, true), sw(w, N, true, true), ssc(sc, (size_t)PCG_NSC * nrhs, true, true);
	pcg_direction_periodic_many(sso.get(), sz.get(), sp.get(), spn.get(), sw.get(), 2, nstncl, (int)ii, (int)jj, 1, ibc, first != 0,
	                            slab.dev, ssc.get(), current_stream(), Batch{nrhs, P}, active);
	return 0;
}

// ------------------------------------------------------------------ transfers on single-precision weights
int cedar_amd_restrict2_ci32(real_t *q, real_t *qc, real_t *ci, int ii, int jj, int iic, int jjc)
{
	const char *who = "cedar_amd_restrict2_ci32";
	if (ci32_args_refused(q && qc && ci, ii >= 3 && jj >= 3 && iic >= 3 && jjc >= 3, true, who)) return -1;
	const size_t P = (size_t)ii * jj, PC = (size_t)iic * jjc;
	Staged sq(q, P, true, false), sqc(qc, PC, true, true), sci(ci, PC * 8, true, false);
	return with_ci32_copy(sci.get(), iic, jjc, 1, 8, who, [&](const Ci2f &W, hipStream_t st) {
		restrict2_ci(W, sq.get(), sqc.get(), ii, jj, iic, jjc, st);
	}) ? 0 : -1;
}

int cedar_amd_interp_add2_ci32(real_t *q, real_t *qc, real_t *res, real_t *so, real_t *ci, len_t iic, len_t jjc, len_t ii,
                               len_t jj, int nstncl)
{
	const char *who = "cedar_amd_interp_add2_ci32";
	if (ci32_args_refused(q && qc && res && so && ci, ii >= 3 && jj >= 3 && iic >= 3 && jjc >= 3, nstncl == 3 || nstncl == 5, who))
		return -1;
	const size_t P = (size_t)ii * jj, PC = (size_t)iic * jjc;
	Staged sq(q, P, true, true), sqc(qc, PC, true, false), sr(res, P, true, true), sso(so, P * nstncl, true, false),
	    sci(ci, PC * 8, true, false);
	return with_ci32_copy(sci.get(), (int)iic, (int)jjc, 1, 8, who, [&](const Ci2f &W, hipStream_t st) {
		interp_add2_ci(W, sq.get(), sqc.get(), sr.get(), sso.get(), (int)iic, (int)jjc, (int)ii, (int)jj, st);
	}) ? 0 : -1;
}

int cedar_amd_restrict3_many_ci32(int nrhs, real_t *q, real_t *qc, real_t *ci, len_t ii, len_t jj, len_t kk, len_t iic, len_t jjc,
                                  len_t kkc)
{
	const char *who = "cedar_amd_restrict3_many_ci32";
	if (many_args_refused(nrhs, q && qc && ci, true, who)) return -1;
	if (ci32_args_refused(true, ii >= 3 && jj >= 3 && kk >= 3 && iic >= 3 && jjc >= 3 && kkc >= 3, true, who)) return -1;
	const size_t P = (size_t)ii * jj * kk, PC = (size_t)iic * jjc * kkc;
	Staged sq(q, P * nrhs, true, false), sqc(qc, PC * nrhs, true, true), sci(ci, PC * 26, true, false);
	return with_ci32_copy(sci.get(), (int)iic, (int)jjc, (int)kkc, 26, who, [&](const Ci3f &W, hipStream_t st) {
		restrict3_ci(W, sq.get(), sqc.get(), (int)ii, (int)jj, (int)kk, (int)iic, (int)jjc, (int)kkc, st, Batch{nrhs, P},
		             Batch{nrhs, PC});
	}) ? 0 : -1;
}

int cedar_amd_interp_add3_many_ci32(int nrhs, real_t *q, real_t *qc, real_t *so, real_t *res, real_t *ci, len_t iic, len_t jjc,
                                    len_t kkc, len_t iif, len_t jjf, len_t kkf, int nstncl)
{
	const char *who = "cedar_amd_interp_add3_many_ci32";
	if (many_args_refused(nrhs, q && qc && so && res && ci, nstncl == 4 || nstncl == 14, who)) return -1;
	if (ci32_args_refused(true, iif >= 3 && jjf >= 3 && kkf >= 3 && iic >= 3 && jjc >= 3 && kkc >= 3, true, who)) return -1;
	const size_t P = (size_t)iif * jjf * kkf, PC = (size_t)iic * jjc * kkc;
	Staged sq(q, P * nrhs, true, true), sqc(qc, PC * nrhs, true, false), sso(so, P * nstncl, true, false),
	    sr(res, P * nrhs, true, true), sci(ci, PC * 26, true, false);
	return with_ci32_copy(sci.get(), (int)iic, (int)jjc, (int)kkc, 26, who, [&](const Ci3f &W, hipStream_t st) {
		interp_add3_ci(W, sq.get(), sqc.get(), sso.get(), sr.get(), (int)iic, (int)jjc, (int)kkc, (int)iif, (int)jjf, (int)kkf, st,
		               Batch{nrhs, P}, Batch{nrhs, PC});
	}) ? 0 : -1;
}

// the single-vector pair: one item of the batched entry points (nrhs = 1 runs the single-vector kernels)
int cedar_amd_restrict3_ci32(real_t *q, real_t *qc, real_t *ci, len_t ii, len_t jj, len_t kk, len_t iic, len_t jjc, len_t kkc)
{
	return cedar_amd_restrict3_many_ci32(1, q, qc, ci, ii, jj, kk, iic, jjc, kkc);
}

int cedar_amd_interp_add3_ci32(real_t *q, real_t *qc, real_t *so, real_t *res, real_t *ci, len_t iic, len_t jjc, len_t kkc,
                               len_t ii, len_t jj, len_t kk, int nstncl)
{
	return cedar_amd_interp_add3_many_ci32(1, q, qc, so, res, ci, iic, jjc, kkc, ii, jj, kk, nstncl);
}

// ------------------------------------------------------------------ 3D drop-ins
void BMG3_SymStd_SETUP_recip(real_t *so, real_t *sor, len_t nx, len_t ny, len_t nz, int nstencl, int nsorv)
{
	(void)nsorv;
	size_t P = (size_t)nx * ny * nz;
	Staged sso(so, P * nstencl, true, false), ssor(sor, P * 2, true, true);
	setup_recip(sso.get() + KP * P, ssor.get() + P, nx, ny, nz, current_stream());
}

void BMG3_SymStd_relax_GS(int kg, real_t *so, real_t *qf, real_t *q, real_t *sor,
                          len_t ii, len_t jj, len_t kk, int ifd, int nstncl, int nsorv,
                          int irelax_sym, int updown, int jpn)
{
	(void)kg; (void)nsorv;
	if (!bc3(jpn, "BMG3_SymStd_relax_GS")) return;
	size_t P = (size_t)ii * jj * kk;
	int nst_eff = (ifd != 1) ? 14 : 4;
	if (nst_eff > nstncl) nst_eff = nstncl;
	// NONSYM always sweeps in the UP order in 3D (relax_GS.f90:85-94)
	int ud = (irelax_sym == 0) ? BMG_UP : updown;
	Staged sso(so, P * nstncl, true, false), sqf(qf, P, true, false), sq(q, P, true, true), ssor(sor, P * 2, true, false);
	if (jpn)
		relax3_gs_per(sso.get(), sqf.get(), sq.get(), ssor.get(), (int)ii, (int)jj, (int)kk, nst_eff, ud, jpn, current_stream());
	else
		relax3_gs(sso.get(), sqf.get(), sq.get(), ssor.get(), (int)ii, (int)jj, (int)kk, nst_eff, ud, current_stream());
}

void BMG3_SymStd_residual(int kg, int NOG, int ifd, real_t *q, real_t *qf, real_t *so, real_t *RES,
                          len_t ii, len_t jj, len_t kk, int NStncl)
{
	size_t P = (size_t)ii * jj * kk;
	int nst_eff = (kg < NOG || ifd != 1) ? 14 : 4; // residual.f90:67
	if (nst_eff > NStncl) nst_eff = NStncl;
	Staged sso(so, P * NStncl, true, false), sqf(qf, P, true, false), sq(q, P, true, false), sr(RES, P, true, true);
	residual3(sso.get(), sqf.get(), sq.get(), sr.get(), (int)ii, (int)jj, (int)kk, nst_eff, current_stream());
}

void BMG3_SymStd_restrict(real_t *q, real_t *qc, real_t *ci, len_t nx, len_t ny, len_t nz,
                          len_t nxc, len_t nyc, len_t nzc, int jpn)
{
	if (!bc3(jpn, "BMG3_SymStd_restrict")) return;
	size_t P = (size_t)nx * ny * nz, PC = (size_t)nxc * nyc * nzc;
	// periodic: the fine vector gets its ghosts refreshed first (restrict.f90:78-103), so it is an output too
	Staged sq(q, P, true, jpn != 0), sqc(qc, PC, true, true), sci(ci, PC * 26, true, false);
	if (jpn)
		restrict3_per(sq.get(), sqc.get(), sci.get(), (int)nx, (int)ny, (int)nz, (int)nxc, (int)nyc, (int)nzc, jpn, current_stream());
	else
		restrict3(sq.get(), sqc.get(), sci.get(), (int)nx, (int)ny, (int)nz, (int)nxc, (int)nyc, (int)nzc, current_stream());
}

void BMG3_SymStd_interp_add(real_t *q, real_t *qc, real_t *so, real_t *res, real_t *ci,
                            len_t iic, len_t jjc, len_t kkc, len_t iif, len_t jjf, len_t kkf,
                            int NStncl, int jpn)
{
	if (!bc3(jpn, "BMG3_SymStd_interp_add")) return;
	size_t P = (size_t)iif * jjf * kkf, PC = (size_t)iic * jjc * kkc;
	Staged sq(q, P, true, true), sqc(qc, PC, true, false), sso(so, P * NStncl, true, false),
	    sr(res, P, true, true), sci(ci, PC * 26, true, false);
	if (jpn)
		interp_add3_per(sq.get(), sqc.get(), sso.get(), sr.get(), sci.get(), (int)iic, (int)jjc, (int)kkc,
		                (int)iif, (int)jjf, (int)kkf, jpn, current_stream());
	else
		interp_add3(sq.get(), sqc.get(), sso.get(), sr.get(), sci.get(), (int)iic, (int)jjc, (int)kkc,
		            (int)iif, (int)jjf, (int)kkf, current_stream());
}

void BMG3_SymStd_SETUP_interp_OI(real_t *so, real_t *soc, real_t *ci, len_t iif, len_t jjf, len_t kkf,
                                 len_t iic, len_t jjc, len_t kkc, int ifd, int nstncl, int irelax,
                                 int jpn, real_t *yo)
{
	(void)soc; (void)irelax; (void)yo;
	if (!bc3(jpn, "BMG3_SymStd_SETUP_interp_OI") || !even_periodic(jpn, iif, jjf, kkf, "BMG3_SymStd_SETUP_interp_OI")) return;
	size_t P = (size_t)iif * jjf * kkf, PC = (size_t)iic * jjc * kkc;
	Staged sso(so, P * nstncl, true, false), sci(ci, PC * 26, true, true);
	if (jpn)
		setup_interp3_per(sso.get(), sci.get(), (int)iif, (int)jjf, (int)kkf, (int)iic, (int)jjc, (int)kkc, ifd, jpn, current_stream());
	else
		setup_interp3(sso.get(), sci.get(), (int)iif, (int)jjf, (int)kkf, (int)iic, (int)jjc, (int)kkc, ifd, current_stream());
}

static void itli3(real_t *so, real_t *soc, real_t *ci, len_t iif, len_t jjf, len_t kkf,
                  len_t iic, len_t jjc, len_t kkc, int ipn, int nst)
{
	if (!bc3(ipn, "BMG3_SymStd_SETUP_ITLI_ex") || !even_periodic(ipn, iif, jjf, kkf, "BMG3_SymStd_SETUP_ITLI_ex")) return;
	size_t P = (size_t)iif * jjf * kkf, PC = (size_t)iic * jjc * kkc;
	Staged sso(so, P * nst, true, false), ssoc(soc, PC * 14, true, true), sci(ci, PC * 26, true, false);
	if (ipn)
		galerkin3_per(sso.get(), ssoc.get(), sci.get(), (int)iif, (int)jjf, (int)kkf, (int)iic, (int)jjc, (int)kkc,
		              nst == 4, ipn, current_stream());
	else
		galerkin3(sso.get(), ssoc.get(), sci.get(), (int)iif, (int)jjf, (int)kkf, (int)iic, (int)jjc, (int)kkc,
		          nst == 4, current_stream());
}

void BMG3_SymStd_SETUP_ITLI07_ex(real_t *so, real_t *soc, real_t *ci, len_t iif, len_t jjf, len_t kkf,
                                 len_t iic, len_t jjc, len_t kkc, int ipn)
{
	itli3(so, soc, ci, iif, jjf, kkf, iic, jjc, kkc, ipn, 4);
}

void BMG3_SymStd_SETUP_ITLI27_ex(real_t *so, real_t *soc, real_t *ci, len_t iif, len_t jjf, len_t kkf,
                                 len_t iic, len_t jjc, len_t kkc, int ipn)
{
	itli3(so, soc, ci, iif, jjf, kkf, iic, jjc, kkc, ipn, 14);
}

void BMG3_SymStd_SETUP_cg_LU(real_t *so, len_t ii, len_t jj, len_t kk, int NStncl, real_t *abd,
                             len_t nabd1, len_t nabd2, int ibc)
{
	if (!bc3(ibc, "BMG3_SymStd_SETUP_cg_LU")) return;
	if ((NStncl != 14 && NStncl != 4) || (ibc && NStncl != 14)) { // the periodic branch knows 14 only (:235, :596)
		report("Cholesky decomp failed! (incorrect NStncl)");
		return;
	}
	size_t P = (size_t)ii * jj * kk, NA = (size_t)nabd1 * nabd2;
	if (ibc && ((size_t)nabd1 < (size_t)(ii - 2) * (jj - 2) * (kk - 2) || (size_t)nabd2 < (size_t)(ii - 2) * (jj - 2) * (kk - 2))) {
		report("BMG3_SymStd_SETUP_cg_LU: the periodic coarsest operator is dense, ABD(n,n) (include/cedar/3d/solver.h:118-121)");
		return;
	}
	Staged sso(so, P * NStncl, true, false), sabd(abd, NA, true, true);
	int *dinfo = static_cast<int *>(pool_get(64));
	if (ibc)
		setup_cg3_per(sso.get(), (int)ii, (int)jj, (int)kk, sabd.get(), (int)nabd1, ibc, dinfo, current_stream());
	else
		setup_cg3(sso.get(), (int)ii, (int)jj, (int)kk, NStncl, sabd.get(), (int)nabd1, (int)nabd2, dinfo, current_stream());
	cg_info(dinfo, "Coarse grid Cholesky decomp failed!");
	pool_put(dinfo, 64);
}

void BMG3_SymStd_SOLVE_cg(real_t *q, real_t *qf, len_t ii, len_t jj, len_t kk, real_t *abd,
                          real_t *bbd, len_t nabd1, len_t nabd2, int ibc)
{
	if (!bc3(ibc, "BMG3_SymStd_SOLVE_cg")) return;
	size_t P = (size_t)ii * jj * kk, NA = (size_t)nabd1 * nabd2;
	Staged sq(q, P, true, true), sqf(qf, P, true, false), sabd(abd, NA, true, false), sb(bbd, nabd2, false, true);
	if (ibc)
		solve_cg3_per(sq.get(), sqf.get(), (int)ii, (int)jj, (int)kk, sabd.get(), sb.get(), (int)nabd1, ibc, current_stream());
	else
		solve_cg3(sq.get(), sqf.get(), (int)ii, (int)jj, (int)kk, sabd.get(), sb.get(), (int)nabd1, (int)nabd2, current_stream());
}

} // extern "C"
