// cedar_amd -- MI355X-native BoxMG V-cycle hot path.
// Shared declarations for the HIP kernels (gfx950 only) and the C-ABI.
//
// Data layout (identical to the reference so that the drop-in boundary needs
// no conversion): FP64, Fortran order (first index fastest), one ghost layer on
// every side, II = nx+2 ...; stencil operators are SoA "planes", slot s at
// offset s*II*JJ[*KK] (include/cedar/array.h:67-74, stencil_op_nd.h:41-78 of
// the reference).  All device code is compiled with -ffp-contract=off and keeps
// the reference's term order, so the solve-phase kernels round exactly like
// the reference's FMA-free CPU build.
#pragma once
#include "../../include/cedar_amd.h"
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

namespace cedar_amd {

typedef double real_t;
typedef unsigned int len_t;

enum { BMG_DOWN = 0, BMG_UP = 1 };
// 2D slots (src/2d/ftn/BMG_stencils_f90.h:29-37, 0-based)
enum { KO = 0, KW = 1, KS = 2, KSW = 3, KNW = 4 };
enum { LL = 0, LR = 1, LA = 2, LB = 3, LSW = 4, LNW = 5, LNE = 6, LSE = 7 };
// 3D slots (:43-64)
enum { KP = 0, KPW = 1, KPS = 2, KB = 3, KPSW = 4, KPNW = 5, KBW = 6, KBNW = 7,
       KBN = 8, KBNE = 9, KBE = 10, KBSE = 11, KBS = 12, KBSW = 13 };
enum { LXYL = 0, LXYR = 1, LXYA = 2, LXYB = 3, LXZA = 4, LXZB = 5,
       LXYNE = 6, LXYSE = 7, LXYSW = 8, LXYNW = 9, LXZSW = 10, LXZNW = 11,
       LXZNE = 12, LXZSE = 13, LYZSW = 14, LYZNW = 15, LYZNE = 16, LYZSE = 17,
       LBSW = 18, LBNW = 19, LBNE = 20, LBSE = 21,
       LTSW = 22, LTNW = 23, LTNE = 24, LTSE = 25 };

#define CEDAR_HIP_CHECK(expr)                                                         \
	do {                                                                              \
		hipError_t e_ = (expr);                                                       \
		if (e_ != hipSuccess) {                                                       \
			fprintf(stderr, "[cedar_amd] HIP error %s at %s:%d: %s\n",                \
			        hipGetErrorName(e_), __FILE__, __LINE__, hipGetErrorString(e_)); \
			abort();                                                                  \
		}                                                                             \
	} while (0)

// 8-byte-aligned pair of doubles: rows start at arbitrary parity, the hardware
// handles the unaligned dwordx4.
typedef double d2u __attribute__((ext_vector_type(2), aligned(8)));

// View of a 3D operator for the solve-phase kernels (27-point relax / residual): entry (slot, i, j, k) =
// so[slot*SS + j*SJ + k*SK + i], reciprocal diagonal (SOR plane msor) = sor[j*rSJ + k*rSK + i].
//   Cedar layout (the boundary):  SS = II*JJ*KK, SJ = II, SK = II*JJ; sor = SOR + II*JJ*KK, same strides.
//   row-interleaved copy (solver-internal, op3_ilv): the NS3 = 16 slot-rows of grid row (j,k) are contiguous
//   (14 operator slots, 1/diag, one pad row), rows padded to RS doubles (a multiple of 16 => every slot-row
//   starts on a 128-byte line): SS = RS, SJ = 16*RS, SK = 16*RS*JJ, sor = so + 14*RS.
struct Op3 {
	const real_t *so;
	size_t SS, SJ, SK;
	const real_t *sor;
	size_t rSJ, rSK;
};
enum { NS3 = 16, ILV_SOR = 14 };
static inline Op3 op3_cedar(const real_t *so, const real_t *sor, int II, int JJ, int KK)
{
	const size_t sk = (size_t)II * JJ, PS = sk * (size_t)KK;
	return Op3{so, PS, (size_t)II, sk, sor ? sor + PS : nullptr, (size_t)II, sk};
}
static inline size_t ilv_row_stride(int II) { return ((size_t)II + 15) / 16 * 16; }
static inline size_t ilv_doubles(int II, int JJ, int KK) { return ilv_row_stride(II) * NS3 * (size_t)JJ * KK; }
static inline Op3 op3_ilv(const real_t *a, int II, int JJ, int KK)
{
	const size_t RS = ilv_row_stride(II);
	(void)KK;
	return Op3{a, RS, NS3 * RS, NS3 * RS * (size_t)JJ, a + ILV_SOR * RS, NS3 * RS, NS3 * RS * (size_t)JJ};
}
// The row-interleaved copy with the entries kept in single precision (cedar_amd_solver_use_fp32_operator; DESIGN.md
// section 12): same 16 slot-rows per grid row, rows padded to a multiple of 32 floats (every slot-row on a 128-byte
// line).  The kernels promote an entry to double when they load it -- exact -- so a sweep on this view is the FP64
// sweep on the operator rounded to float, bit for bit, at 84 instead of 136 bytes per point.
struct Op3f {
	const float *so;
	size_t SS, SJ, SK;
	const float *sor;
	size_t rSJ, rSK;
};
// pair of floats at any element offset: the [i]-pattern pairs start at odd offsets (4-byte aligned dwordx2)
typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));
static inline size_t ilv32_row_stride(int II) { return ((size_t)II + 31) / 32 * 32; }
static inline size_t ilv32_floats(int II, int JJ, int KK) { return ilv32_row_stride(II) * NS3 * (size_t)JJ * KK; }
static inline Op3f op3f_ilv(const float *a, int II, int JJ, int KK)
{
	const size_t RS = ilv32_row_stride(II);
	(void)KK;
	return Op3f{a, RS, NS3 * RS, NS3 * RS * (size_t)JJ, a + ILV_SOR * RS, NS3 * RS, NS3 * RS * (size_t)JJ};
}
// build it (round to nearest even); *overflow (device int, cleared by the caller) is set to 1 when a finite entry of the
// operator or of 1/diag rounds to +-inf (relax3d.hip)
void ilv32_build(const real_t *so, const real_t *sor_msor, float *ilv, int II, int JJ, int KK, int *overflow, hipStream_t st);
// register / drop a row-interleaved solve copy for an operator outside a resident solver (relax3d.hip); prepare
// returns 1 when a copy was built (levels with at least min_rows rows that fit the card's free memory)
int relax3_prepare(const real_t *so, const real_t *sor, int II, int JJ, int KK, int min_rows, hipStream_t st);
void relax3_release(const real_t *so);
// CEDAR_AMD_ILV as relax3_prepare's min_rows: -1 never (0), 0 every 27-point level (1), n levels of at least n rows
// (n >= 2); default 320.  Read on every call
int ilv_min_rows_env();
// does a 27-point level of these extents (ghosts included) take the row-interleaved copy: min_rows >= 0, at least
// min_rows rows, at most 512 row pairs, and the copy fits beside a 10 % reserve of the card
bool ilv_level_wanted(int II, int JJ, int KK, int min_rows);
// the operator view the sweeps of a registered operator read: its row-interleaved copy where there is one, else the planes
Op3 relax3_op_view(const real_t *so, int II, int JJ, int KK);
// build the row-interleaved copy from the Cedar-layout operator (14 slots) and 1/diag plane (relax3d.hip)
void ilv_build(const real_t *so, const real_t *sor_msor, real_t *ilv, int II, int JJ, int KK, hipStream_t st);

// A batch of independent problems on ONE operator (plane relaxation: the planes of one colour, solver.cpp): the 2D
// solve-phase kernels take the batch item from blockIdx.y (row kernels with a one-dimensional grid) or blockIdx.z and
// offset their VECTOR arguments by `stride` doubles per item; operator arrays are shared.  n = 1: a single problem.
struct Batch {
	int n = 1;
	size_t stride = 0;
};

// The single-precision copy of a 7-point level (cedar_amd_solver_use_fp32_operator_all; op7f.hip):
// the NS7 = 5 slot-rows of grid row (j,k) -- KPW, KPS, KB, the diagonal KP, 1/diag -- are contiguous, rows padded to RS
// floats (a multiple of 32 => every slot-row starts on a 128-byte line).  Entry (slot, i, j, k) = a[j*SJ + k*SK + slot*RS
// + i]; SJ = 5*RS, SK = 5*RS*JJ.  Ghost rows and columns are kept (the sweep reads KPW at i+1, KPS at j+1, KB at k+1).
struct Op7f {
	const float *a;
	size_t RS, SJ, SK;
};
enum { NS7 = 5, O7_PW = 0, O7_PS = 1, O7_B = 2, O7_P = 3, O7_RD = 4 };
static inline size_t op7f_floats(int II, int JJ, int KK) { return ilv32_row_stride(II) * NS7 * (size_t)JJ * KK; }
static inline Op7f op7f_view(const float *a, int II, int JJ, int KK)
{
	const size_t RS = ilv32_row_stride(II);
	(void)KK;
	return Op7f{a, RS, NS7 * RS, NS7 * RS * (size_t)JJ};
}
// build it from the Cedar planes (4 slots) and the 1/diag plane (round to nearest even); *overflow as for ilv32_build
void op7f_build(const real_t *so, const real_t *sor_msor, float *out, int II, int JJ, int KK, int *overflow, hipStream_t st);
// the 7-point sweep (two colour launches, UP = 0,1; DOWN = 1,0) and residual on that view, and their batched twins
// (operator entries fetched once per point, the items inside): bit for bit relax3_gs / residual3 / relax3_gs7_many /
// residual7_many on the rounded arrays; rows of any length
void relax3_gs7_op(const Op7f &A, const real_t *qf, real_t *q, int II, int JJ, int KK, int updown, hipStream_t st);
void residual7_op(const Op7f &A, const real_t *qf, const real_t *q, real_t *res, int II, int JJ, int KK, hipStream_t st);
void relax3_gs7_many(const Op7f &A, const real_t *qf, real_t *q, int II, int JJ, int KK, int updown, hipStream_t st, Batch bt);
void residual7_many(const Op7f &A, const real_t *qf, const real_t *q, real_t *res, int II, int JJ, int KK, hipStream_t st, Batch bt);

// The single-precision copy of a 2D level (cedar_amd_solver_use_fp32_operator_2d; op2f.hip): the
// slot-rows of grid row j lie back to back -- nine-point (ns = 6): KW, KS, KSW, KNW, KO, 1/diag; five-point (ns = 4): KW,
// KS, KO, 1/diag -- each padded to RS floats (a multiple of 32 => every slot-row starts on a 128-byte line).  Element i of
// a slot-row sits at offset i + 1: the sweep's pairs start at odd i, so the one float of lead puts them on 8-byte
// boundaries and no pair straddles a line.  Ghost rows and columns are kept (the sweep reads KW at i+1 and KS / KSW / KNW
// of row j+1).  row(slot, j) takes the Cedar slot number (KO .. KNW) and points at element i = 0.
struct Op2f {
	const float *a;
	size_t RS, SJ;
	int ns;
	__host__ __device__ __forceinline__ const float *row(int slot, size_t j) const
	{
		return a + j * SJ + (size_t)(slot == KO ? ns - 2 : slot - 1) * RS + 1;
	}
	__host__ __device__ __forceinline__ const float *rd(size_t j) const { return a + j * SJ + (size_t)(ns - 1) * RS + 1; }
};
static inline int op2f_slots(int nstncl) { return nstncl == 5 ? 6 : 4; }
static inline size_t op2f_row_stride(int II) { return ilv32_row_stride(II + 1); }
static inline size_t op2f_floats(int II, int JJ, int nstncl) { return op2f_row_stride(II) * op2f_slots(nstncl) * (size_t)JJ; }
static inline Op2f op2f_view(const float *a, int II, int nstncl)
{
	const size_t RS = op2f_row_stride(II);
	return Op2f{a, RS, RS * op2f_slots(nstncl), op2f_slots(nstncl)};
}
// build it from the Cedar planes (nstncl 5 | 3 of them) and the 1/diag plane (round to nearest even); *overflow as for
// ilv32_build
// sor_msor == nullptr (a line-relaxed level, which has no 1/diag plane): that slot-row is zeros
void op2f_build(const real_t *so, const real_t *sor_msor, float *out, int II, int JJ, int nstncl, int *overflow, hipStream_t st);
// The 2D point sweep and residual on that view, batches as for the FP64 kernels (the item from the launch grid):
// relax2_gs_op -- reference order (CEDAR_AMD_FRUN2 picks band-fused or two launches, as relax2_gs does); relax2_gs9_psum_op --
// the partial-sum sweep where relax2_gs9_psum would run it (same run length), else relax2_gs_op.  Bit for bit the FP64
// kernels of relax2d.hip / residual.hip on the rounded arrays (the device bodies are the same code: relax2_dev.h)
void relax2_gs_op(const Op2f &A, const real_t *qf, real_t *q, int II, int JJ, int nstncl, int updown, hipStream_t st,
                  Batch bt = Batch());
void relax2_gs9_psum_op(const Op2f &A, const real_t *qf, real_t *q, int II, int JJ, int updown, hipStream_t st, Batch bt = Batch());
void residual2_op(const Op2f &A, const real_t *qf, const real_t *q, real_t *res, int II, int JJ, int nstncl, hipStream_t st,
                  Batch bt = Batch());

// Line relaxation on such copies (cedar_amd_solver_use_fp32_operator_lines; linesf.hip): the operator
// as Op2f (the 1/diag slot-row zeros), for y lines the Op2f of the transposed planes (setup_lines_yt) on the transposed grid;
// the factors as floats in the two forms the FP64 kernels read -- linesf_image: the two SOR planes, element for element;
// linesf_permute: the scan-ordered copy (lines_permuted_doubles elements; a lane's eight values of a kind are two 16-byte
// loads).  Both round the FP64 factors to nearest even and raise *overflow as op2f_build does.  relax_lines_x_op /
// relax_lines_yt_op: relax_lines_x / relax_lines_yt (Dirichlet) on these arrays, bit for bit the FP64 kernels on the rounded
// operator and factors (the device bodies are the same code: lines_dev.h); pff == nullptr: the factors are read from sorf
void linesf_image(const real_t *sor, float *out, int II, int JJ, int *overflow, hipStream_t st);
void linesf_permute(const real_t *sor, float *pf, int n, int ld, int nlines, size_t PS, int *overflow, hipStream_t st);
void relax_lines_x_op(const Op2f &A, const real_t *qf, real_t *q, const float *sorf, int II, int JJ, int nstncl, int updown,
                      hipStream_t st, const float *pff = nullptr, Batch bt = Batch());
void relax_lines_yt_op(const Op2f &At, const real_t *qft, real_t *q, real_t *qt, const float *sorf, int II, int JJ, int nstncl,
                       int updown, hipStream_t st, const float *pff = nullptr, Batch bt = Batch());
bool line_fits_lds_host(int n); // lines.hip: a line of n unknowns fits the LDS of a CU

// View of a level's interpolation weights for the transfer kernels (transfer_dev.h): entry (slot, ic, jc, kc) =
// p[slot*ss + kc*sk + jc*sj + ic], coarse indices 0-based with the ghosts; 2D: kc = 0.
//   Cedar layout (the boundary), T = real_t: sj = IIC, sk = IIC*JJC, ss = IIC*JJC*KKC.
//   single-precision copy (cedar_amd_solver_use_fp32_interpolation; transferf.hip), T = float: the
//   slots stay in planes, every coarse row padded to RS floats (a multiple of 32 => every row of every slot starts on a
//   128-byte line).  Element ic of a row sits at offset ic + 1: the restrictions give a lane the coarse columns (ic, ic+1)
//   with ic odd, so the one float of lead puts its pairs on 8-byte boundaries; RS >= IIC + 3, so the element ic + 2 a lane
//   reads beside its last pair stays in the row.  p points at element 0 of the first row.
template <class T> struct CiW {
	const T *p;
	size_t sj, sk, ss;
};
typedef CiW<real_t> Ci3d; // 2D and 3D alike
typedef CiW<float> Ci3f;
typedef Ci3f Ci2f;
static inline Ci3d ci_cedar(const real_t *ci, int IIC, int JJC, int KKC = 1)
{
	const size_t sk = (size_t)IIC * JJC;
	return Ci3d{ci, (size_t)IIC, sk, sk * (size_t)KKC};
}
static inline size_t ci32_row_stride(int IIC) { return ilv32_row_stride(IIC + 3); }
static inline size_t ci32_floats(int IIC, int JJC, int KKC, int nslots) { return ci32_row_stride(IIC) * (size_t)JJC * KKC * nslots; }
static inline Ci3f ci32_view(const float *a, int IIC, int JJC, int KKC = 1)
{
	const size_t RS = ci32_row_stride(IIC);
	return Ci3f{a + 1, RS, RS * (size_t)JJC, RS * (size_t)JJC * KKC};
}
// build it from the Cedar-layout weights (nslots 26 | 8; round to nearest even; lead and tail of every row zero); *overflow
// as for ilv32_build
void ci32_build(const real_t *ci, float *out, int IIC, int JJC, int KKC, int nslots, int *overflow, hipStream_t st);
// The transfers on that view (transferf.hip), bit for bit restrict2 / interp_add2 / restrict3 / interp_add3 and the _many
// pair on the rounded weights (the device bodies are the same code: transfer_dev.h).  The 3D pair takes a batch: bf.n = 1
// is the single-vector kernel's work.
void restrict2_ci(const Ci2f &W, const real_t *q, real_t *qc, int II, int JJ, int IIC, int JJC, hipStream_t st,
                  Batch bf = Batch(), Batch bc = Batch());
void interp_add2_ci(const Ci2f &W, real_t *q, const real_t *qc, real_t *res, const real_t *so, int IIC, int JJC, int IIF, int JJF,
                    hipStream_t st, Batch bf = Batch(), Batch bc = Batch());
void restrict3_ci(const Ci3f &W, const real_t *q, real_t *qc, int II, int JJ, int KK, int IIC, int JJC, int KKC, hipStream_t st,
                  Batch bf = Batch(), Batch bc = Batch());
void interp_add3_ci(const Ci3f &W, real_t *q, const real_t *qc, const real_t *so, real_t *res, int IIC, int JJC, int KKC,
                    int IIF, int JJF, int KKF, hipStream_t st, Batch bf = Batch(), Batch bc = Batch());

// ---- kernel launchers (device pointers, asynchronous on `st`) ----
// relax3d.hip
void setup_recip(const real_t *so_diag, real_t *sor_msor, size_t II, size_t JJ, size_t KK, hipStream_t st);
void relax3_gs(const real_t *so, const real_t *qf, real_t *q, const real_t *sor,
               int II, int JJ, int KK, int nstncl, int updown, hipStream_t st);
// 27-point sweep / residual on an operator view (the solver's row-interleaved copy)
// T: scratch of the vector's size for the partial-sum sweep (relax3d_psum.hip), nullptr = reference order always
void relax3_gs27_op(const Op3 &A, const real_t *qf, real_t *q, int II, int JJ, int KK, int updown, hipStream_t st,
                    real_t *T = nullptr);
void residual27_op(const Op3 &A, const real_t *qf, const real_t *q, real_t *res, int II, int JJ, int KK, hipStream_t st);
// the same kernels on the single-precision view (rows of at most 1024 points: the row kernels only)
void relax3_gs27_op(const Op3f &A, const real_t *qf, real_t *q, int II, int JJ, int KK, int updown, hipStream_t st,
                    real_t *T = nullptr);
void residual27_op(const Op3f &A, const real_t *qf, const real_t *q, real_t *res, int II, int JJ, int KK, hipStream_t st);
void relax3_planes27(const real_t *so, const real_t *qf, real_t *q, const real_t *sor,
                     int II, int JJ, int KK, int kb, int up, int part, hipStream_t st);
void relax3_pass27(const real_t *so, const real_t *qf, real_t *q, const real_t *sor,
                   int II, int JJ, int KK, int jb, int kb, int efirst, hipStream_t st, int part = 0);
void relax3_fixup27(const real_t *so, const real_t *qf, real_t *q, const real_t *sor,
                    int II, int JJ, int KK, int icol, int jb, int kb, hipStream_t st);
void relax3_colour7(const real_t *so, const real_t *qf, real_t *q, const real_t *sor,
                    int II, int JJ, int KK, int pts, hipStream_t st);
// relax2d.hip
void relax2_gs(const real_t *so, const real_t *qf, real_t *q, const real_t *sor,
               int II, int JJ, int nstncl, int updown, hipStream_t st, Batch bt = Batch());
// residual.hip
void residual2(const real_t *so, const real_t *qf, const real_t *q, real_t *res,
               int II, int JJ, int nstncl, hipStream_t st, Batch bt = Batch());
void residual3(const real_t *so, const real_t *qf, const real_t *q, real_t *res,
               int II, int JJ, int KK, int nstncl, hipStream_t st);
// pieces of the 2D sweep / set-up for domain-decomposed runs (relax2d.hip, setup_interp.hip)
void relax2_pass9(const real_t *so, const real_t *qf, real_t *q, const real_t *sor,
                  int II, int JJ, int jb, int efirst, hipStream_t st);
void relax2_fixup9(const real_t *so, const real_t *qf, real_t *q, const real_t *sor,
                   int II, int JJ, int icol, int jb, hipStream_t st);
void relax2_colour5(const real_t *so, const real_t *qf, real_t *q, const real_t *sor,
                    int II, int JJ, int jo, hipStream_t st);
void setup_interp2_phase(const real_t *so, real_t *ci, int IIF, int JJF, int IIC, int JJC, int ifd, int phase,
                         int ilo, int jlo, hipStream_t st);
void lines_rhs2(const real_t *so, const real_t *qf, const real_t *q, real_t *out, int II, int JJ, int nstncl, int dir, int lb,
                hipStream_t st);
void lines_store2(const real_t *in, real_t *q, int II, int JJ, int dir, int lb, hipStream_t st);
void lines_carry(real_t *y, const real_t *p, const real_t *c, int nlines, int n, int ld, hipStream_t st);
void affine_lines(real_t *y, const real_t *a, const real_t *div, int nlines, int n, int ld, int reverse, hipStream_t st);
// The one table of the boundary codes: the periodic directions of a code (2D: 1 y, 2 x, 3 xy; 3D: 1 y, 2 x, 3 xy, 5 z, 6 xz,
// 7 yz, 8 xyz).  Host code asks it where it needs a direction; kernels take the PerDirs as an argument or ask it themselves.
struct PerDirs {
	int x, y, z;
};
__host__ __device__ static inline PerDirs per_dirs(int nd, int ibc)
{
	return PerDirs{ibc == 2 || ibc == 3 || (nd == 3 && (ibc == 6 || ibc == 8)), ibc == 1 || ibc == 3 || (nd == 3 && (ibc == 7 || ibc == 8)),
	               nd == 3 && ibc >= 5 && ibc <= 8};
}
// the 3D code with x taken out (0, 1 y, 5 z, 7 yz): what is left to refresh behind a kernel that did the x ghosts itself
__host__ __device__ static inline int per3_without_x(int ibc)
{
	const PerDirs pd = per_dirs(3, ibc);
	return pd.z ? (pd.y ? 7 : 5) : (pd.y ? 1 : 0);
}
// 2D periodic boundary conditions (periodic2d.hip); ipn = 1 per_y, 2 per_x, 3 per_xy
void wrap2(real_t *q, int II, int JJ, int nplanes, int do_y, int do_x, hipStream_t st);
int relax2_gs_per(const real_t *so, const real_t *qf, real_t *q, const real_t *sor,
                  int II, int JJ, int nstncl, int updown, int ipn, hipStream_t st); // 1 = rows too long
// the two transfers and the coarsest solve take a batch stored with the level's stride II*JJ (wrap2 takes the items as
// planes); item m has the bits of the call on item m alone
void restrict2_per(real_t *q, real_t *qc, const real_t *ci, int Nx, int Ny, int Nxc, int Nyc, int ipn, hipStream_t st,
                   Batch bf = Batch(), Batch bc = Batch());
void interp_add2_per(real_t *q, const real_t *qc, real_t *res, const real_t *so, const real_t *ci,
                     int IIC, int JJC, int IIF, int JJF, int ipn, hipStream_t st, Batch bf = Batch(), Batch bc = Batch());
void galerkin2_per(const real_t *so, real_t *soc, const real_t *ci, int IIF, int JJF, int IIC, int JJC, int ifd, int ipn,
                   hipStream_t st);
void setup_interp2_per(const real_t *so, real_t *ci, int IIF, int JJF, int IIC, int JJC, int ifd, int ipn, hipStream_t st);
// semidef (here and in setup_cg3_per, setup_cg2, setup_cg3): the last unknown's diagonal entry is doubled before the
// factorisation -- a semidefinite operator whose null space is the constants (cedar_amd_solver_create_semidefinite)
void setup_cg2_per(const real_t *so, int II, int JJ, int nstncl, real_t *abd, int nabd1, int ipn, int *info, hipStream_t st,
                   int semidef = 0);
void solve_cg2_per(real_t *q, const real_t *qf, int II, int JJ, const real_t *abd, real_t *bbd, int nabd1, int ipn, hipStream_t st,
                   Batch bt = Batch()); // one lane per item, the factor shared; bbd: bt.n segments of (II-2)(JJ-2) doubles
// 3D periodic boundary conditions (periodic3d.hip, relax3d.hip); ipn = 1 y, 2 x, 3 xy, 5 z, 6 xz, 7 yz, 8 xyz
bool periodic3_code_ok(int ipn);
void wrap3(real_t *a, int II, int JJ, int KK, int narrays, int ipn, hipStream_t st);
void wrap3_colour(real_t *q, int II, int JJ, int KK, int jb, int kb, int ipn, hipStream_t st, int narrays = 1);
void wrap3_sweep_end(real_t *q, int II, int JJ, int KK, int ipn, hipStream_t st, int narrays = 1);
void relax3_gs_per(const real_t *so, const real_t *qf, real_t *q, const real_t *sor,
                   int II, int JJ, int KK, int nstncl, int updown, int ipn, hipStream_t st, int ghosts_consistent = 0);
void restrict3_per(real_t *q, real_t *qc, const real_t *ci, int II, int JJ, int KK, int IIC, int JJC, int KKC, int ipn,
                   hipStream_t st);
void interp_add3_per(real_t *q, const real_t *qc, const real_t *so, real_t *res, const real_t *ci,
                     int IIC, int JJC, int KKC, int IIF, int JJF, int KKF, int ipn, hipStream_t st);
void setup_interp3_per(const real_t *so, real_t *ci, int IIF, int JJF, int KKF, int IIC, int JJC, int KKC, int ifd, int ipn,
                       hipStream_t st);
void galerkin3_per(const real_t *so, real_t *soc, const real_t *ci, int IIF, int JJF, int KKF, int IIC, int JJC, int KKC,
                   int ifd, int ipn, hipStream_t st);
void setup_cg3_per(const real_t *so, int II, int JJ, int KK, real_t *abd, int nabd1, int ipn, int *info, hipStream_t st,
                   int nst = 14, int semidef = 0); // nst: slots of so, 4 for a one-level seven-point handle
void solve_cg3_per(real_t *q, const real_t *qf, int II, int JJ, int KK, const real_t *abd, real_t *bbd, int nabd1, int ipn,
                   hipStream_t st, Batch bt = Batch()); // one workgroup per item, the factor shared; bbd: bt.n segments of N doubles
// plane relaxation, the 3D side (planes.hip); dir 0 xy, 1 xz, 2 yz; stacked 2D arrays, slot q = plane beg + 2q
void plane_operator(int dir, int nst, const real_t *so, real_t *so2, int II, int JJ, int KK, hipStream_t st);
void plane_gather(int dir, int nst, const real_t *so, const real_t *x, const real_t *b, real_t *x2s, real_t *b2s,
                  int II, int JJ, int KK, int beg, int nslots, hipStream_t st);
void plane_scatter(int dir, const real_t *x2s, real_t *x, int II, int JJ, int KK, int beg, int nslots, hipStream_t st);
// qf = A q (operator application with Cedar's sign convention), residual.hip
void matvec2(const real_t *so, const real_t *q, real_t *qf, int II, int JJ, int nstncl, hipStream_t st);
void matvec3(const real_t *so, const real_t *q, real_t *qf, int II, int JJ, int KK, int nstncl, hipStream_t st);
// sum of squares over the interior -> *out (deterministic two-stage tree); scratch >= 4096 doubles
void sumsq_interior(const real_t *v, int II, int JJ, int KK, real_t *scratch, real_t *out, hipStream_t st);
// the same for each item of a batch, one after the other on `st` (each item in sumsq_interior's order): out[m]
void sumsq_interior_many(const real_t *v, int II, int JJ, int KK, real_t *scratch, real_t *out, hipStream_t st, Batch bt);
// transfer.hip
void restrict2(const real_t *q, real_t *qc, const real_t *ci, int II, int JJ, int IIC, int JJC, hipStream_t st,
               Batch bf = Batch(), Batch bc = Batch()); // batch strides of the fine / coarse vectors
void restrict3(const real_t *q, real_t *qc, const real_t *ci, int II, int JJ, int KK,
               int IIC, int JJC, int KKC, hipStream_t st);
void interp_add2(real_t *q, const real_t *qc, real_t *res, const real_t *so, const real_t *ci,
                 int IIC, int JJC, int IIF, int JJF, hipStream_t st, Batch bf = Batch(), Batch bc = Batch());
void interp_add3(real_t *q, const real_t *qc, const real_t *so, real_t *res, const real_t *ci,
                 int IIC, int JJC, int KKC, int IIF, int JJF, int KKF, hipStream_t st);
void box_copy(real_t *arr, int II, int JJ, int KK, int nplanes, int nboxes, const int *boxes,
              const unsigned long long *offsets, real_t *buf, int unpack, hipStream_t st, int strided = 0);
// setup_interp.hip
void setup_interp2(const real_t *so, real_t *ci, int IIF, int JJF, int IIC, int JJC, int ifd, hipStream_t st);
void setup_interp3(const real_t *so, real_t *ci, int IIF, int JJF, int KKF,
                   int IIC, int JJC, int KKC, int ifd, hipStream_t st);
void setup_interp3_phase(const real_t *so, real_t *ci, int IIF, int JJF, int KKF,
                         int IIC, int JJC, int KKC, int ifd, int phase, int ilo, int jlo, int klo, hipStream_t st);
// galerkin.hip
void galerkin2(const real_t *so, real_t *soc, const real_t *ci, int IIF, int JJF, int IIC, int JJC,
               int ifd, hipStream_t st);
void galerkin3_fused27(const real_t *so, real_t *soc, const real_t *ci, int IIF, int JJF, int KKF,
                       int IIC, int JJC, int KKC, hipStream_t st);
void galerkin3_fused7(const real_t *so, real_t *soc, const real_t *ci, int IIF, int JJF, int KKF,
                      int IIC, int JJC, int KKC, hipStream_t st);
bool galerkin3_tiled(const real_t *so, real_t *soc, const real_t *ci, int IIF, int JJF, int KKF,
                     int IIC, int JJC, int KKC, int ifd, hipStream_t st);
bool galerkin3_rows(const real_t *so, real_t *soc, const real_t *ci, int IIF, int JJF, int KKF,
                    int IIC, int JJC, int KKC, int ifd, hipStream_t st);
void galerkin3_rows_release(); // frees the kept ring of row sums
bool galerkin3_rows_pairs(const real_t *so, int IIF); // the row sums can read the operator as aligned pairs
void galerkin3(const real_t *so, real_t *soc, const real_t *ci, int IIF, int JJF, int KKF,
               int IIC, int JJC, int KKC, int ifd, hipStream_t st);
// util.hip: zero fill by a kernel of the library.  hipMemsetAsync is not used on solver data: under the HIP runtime
// that PyTorch loads first (the multi-GPU path always imports torch) it left non-zero bit patterns in the cleared
// arrays (profiles/r01_memset_under_torch_runtime.log)
void zero_fill(real_t *p, size_t n, hipStream_t st);
void vec_add(real_t *x, const real_t *z, size_t n, hipStream_t st); // x += z
// util.hip: v := v - mean_interior(v) on every item of `active` (bit m = item m; items bt.stride doubles apart, ghosts
// included and not written).  Deterministic two-stage sum whose order depends on the extents alone, carried in two
// doubles (the mean is the correctly rounded one): item m of a batch is bit for bit the single-vector call.  scratch: project_mean_doubles(bt.n) doubles; the means are left in its last bt.n
// entries (0 for an item outside `active`)
enum { PROJECT_MEAN_NB = 1024 };
static inline size_t project_mean_doubles(int nrhs) { return (size_t)nrhs * (2 * PROJECT_MEAN_NB + 1); }
void project_mean(real_t *v, int II, int JJ, int KK, real_t *scratch, hipStream_t st);
void project_mean_many(real_t *v, int II, int JJ, int KK, real_t *scratch, hipStream_t st, Batch bt, unsigned active);
// lines.hip
void setup_lines_x(const real_t *so, real_t *sor, int II, int JJ, hipStream_t st, int fold = 0);
void setup_lines_y(const real_t *so, real_t *sor, int II, int JJ, hipStream_t st, int fold = 0);
void relax_lines_x(const real_t *so, const real_t *qf, real_t *q, const real_t *sor,
                   int II, int JJ, int nstncl, int updown, hipStream_t st, int ipn = 0, const real_t *pf = nullptr,
                   Batch bt = Batch()); // batches: stride II*JJ when ipn != 0 (the wraps take the items as planes)
// scan-ordered copy of the line factors for the resident solver (lines.hip line_pttrs_pf); 0 doubles = not used
size_t lines_permuted_doubles(int n, int nlines);
void lines_permute(const real_t *sor, real_t *pf, int n, int ld, int nlines, size_t PS, hipStream_t st);
// scratch: line-contiguous buffer of ylines_scratch_doubles(II,JJ) doubles in HBM
size_t ylines_scratch_doubles(int II, int JJ);
void relax_lines_y(const real_t *so, const real_t *qf, real_t *q, const real_t *sor, real_t *scratch,
                   int II, int JJ, int nstncl, int updown, hipStream_t st, int ipn = 0);
// y-lines on transposed arrays (lines.hip): transposed operator planes, transposed right-hand side, scratch for q^T
void transpose2(const real_t *in, real_t *out, int II, int JJ, hipStream_t st, Batch bt = Batch());
// lines_small.hip: all line sweeps of one visit of a level of at most 64 x 64 unknowns in one launch
bool lines_small_ok(int II, int JJ);
// one half of a V-cycle visit of such a level in one launch: pre != 0: pre-smoothing, residual, restriction, coarse x := 0;
// else interpolation-and-add, post-smoothing.  kind: 0 point relaxation (sorx = reciprocals), 1 / 2 / 3 = x / y / xy lines
void visit_small(int pre, const real_t *so, const real_t *qf, real_t *q, real_t *res, const real_t *sorx, const real_t *sory,
                 int II, int JJ, int nstncl, int kind, int nsweeps, const real_t *ci, real_t *cb, real_t *cx, int IIC, int JJC,
                 hipStream_t st, Batch bf = Batch(), Batch bc = Batch());
void relax_points_small(const real_t *so, const real_t *qf, real_t *q, const real_t *sor, int II, int JJ, int nstncl,
                        int updown, int nsweeps, hipStream_t st, Batch bt = Batch());
void relax_lines_small(const real_t *so, const real_t *qf, real_t *q, const real_t *sorx, const real_t *sory,
                       int II, int JJ, int nstncl, int kind, int updown, int nsweeps, hipStream_t st, Batch bt = Batch());
void setup_lines_yt(const real_t *so, real_t *sot, int II, int JJ, int nstncl, hipStream_t st);
void relax_lines_yt(const real_t *sot, const real_t *qft, real_t *q, real_t *qt, const real_t *sor,
                    int II, int JJ, int nstncl, int updown, hipStream_t st, const real_t *pf = nullptr, Batch bt = Batch());
// cgsolve.hip
void setup_cg2(const real_t *so, int II, int JJ, int nstncl, real_t *abd, int nabd1, int nabd2, int *info, hipStream_t st,
               int semidef = 0);
void solve_cg2(real_t *q, const real_t *qf, int II, int JJ, const real_t *abd, real_t *bbd, int nabd1, int nabd2, hipStream_t st,
               Batch bt = Batch(), int semidef = 0); // bbd: nabd2 doubles per batch item; semidef: the solution's mean is removed
void setup_cg3(const real_t *so, int II, int JJ, int KK, int nstncl, real_t *abd, int nabd1, int nabd2, int *info, hipStream_t st,
               int semidef = 0);
void solve_cg3(real_t *q, const real_t *qf, int II, int JJ, int KK, const real_t *abd, real_t *bbd, int nabd1, int nabd2, hipStream_t st,
               Batch bt = Batch(), int semidef = 0); // bbd: nabd2 doubles per batch item; semidef: the solution's mean is removed
// krylov.hip: the vector work of the preconditioned conjugate gradient (solver.cpp cedar_amd_solver_pcg).  The scalars
// of a run live on the device in sc[PCG_NSC]; the kernels read alpha / beta from there and write them back.
enum { PCG_RHO = 0, PCG_SIGMA = 1, PCG_ALPHA = 2, PCG_BETA = 3, PCG_RR = 4, PCG_RZ = 5, PCG_FLAG = 6, PCG_WZ = 7, PCG_NSC = 8 };
// What a run's settings decide on the host, for the resident solver and the rank grid alike (solver.cpp pcg_run,
// dist_common.h dist_pcg).  zm: where z = M^-1 r comes from, 0 z = r, 1 z = r / diag, 2 the multigrid cycle; the stop test
// is on ||r||_2, or with mnorm on sqrt(r.z), relative (rel) to its initial value or absolute.
struct PcgRule {
	int zm;
	bool mnorm, rel;
	double tol;
	// rr = r.r and rz = r.z of the current residual, r0 = ||r0||_2, m0 = sqrt(r0.z0)
	bool stop(double rr, double rz, double r0, double m0) const
	{
		const double v = mnorm ? std::sqrt(rz > 0 ? rz : 0.0) : std::sqrt(rr);
		return (rel ? v / (mnorm ? m0 : r0) : v) < tol;
	}
};
static inline PcgRule pcg_rule(const cedar_amd_pcg_settings &p)
{
	return PcgRule{p.precon == CEDAR_AMD_PCG_PRECON_NONE ? 0 : p.precon == CEDAR_AMD_PCG_PRECON_DIAG ? 1 : 2,
	               p.stop_test >= CEDAR_AMD_PCG_STOP_ABS_RES_M2,
	               p.stop_test == CEDAR_AMD_PCG_STOP_REL_RES_L2 || p.stop_test == CEDAR_AMD_PCG_STOP_REL_RES_M2, p.tol};
}
static inline cedar_amd_pcg_settings pcg_settings_or_default(const cedar_amd_pcg_settings *settings)
{
	cedar_amd_pcg_settings p;
	if (settings) p = *settings;
	else cedar_amd_default_pcg_settings(&p);
	return p;
}
size_t pcg_slab_doubles(int nd, int nst, int II, int JJ, int KK); // partial-sum slab of the two launchers below
// pn = z + beta p (first: pn = z), w = A pn, sigma = pn.w, alpha = rho / sigma (0 and PCG_FLAG = 1 when sigma <= 0 or
// rho = 0); op27: the operator view of a 27-point level (nullptr: the Cedar planes of so)
void pcg_direction(const real_t *so, const Op3 *op27, const real_t *z, const real_t *p, real_t *pn, real_t *w, int nd,
                   int nst, int II, int JJ, int KK, bool first, real_t *slab, real_t *sc, hipStream_t st,
                   real_t *partial = nullptr);
// The same pass on a level with periodic directions (cedar_amd_solver_fcg_periodic): a stencil neighbour that falls on the
// ghost layer of a periodic direction is read at the opposite interior end (index 0 -> extent - 2, extent - 1 -> 1, edges
// and corners in every combination), so no ghost cell of z or p in a periodic direction contributes to a result; ghosts
// of the other directions are read as in pcg_direction.  Operator entries are read where pcg_direction reads them (their
// ghost layers hold the periodic image, as the periodic cycle requires).  Same slab, same second stage; 27-point: the
// Cedar planes.
void pcg_direction_periodic(const real_t *so, const real_t *z, const real_t *p, real_t *pn, real_t *w, int nd, int nst, int II,
                            int JJ, int KK, int ibc, bool first, real_t *slab, real_t *sc, hipStream_t st,
                            real_t *partial = nullptr);
// move: x += alpha p, r -= alpha w; then r.r and by zmode 0 (z = r) / 1 (z = r / diag, written) / 2 (z read) r.z with
// the new rho and beta (first: beta = 0); zmode 3: r.r only.  diag: the operator's centre slot.  KK = 1 for 2D.
void pcg_update(int zmode, bool move, real_t *x, real_t *r, const real_t *p, const real_t *w, real_t *z,
                const real_t *diag, int II, int JJ, int KK, bool first, real_t *slab, real_t *sc, hipStream_t st,
                real_t *partial = nullptr);
// The two passes on a batch of right-hand sides (cedar_amd_solver_pcg_many): vectors item-major with bt.stride, item m's
// scalars at sc + m * PCG_NSC, slab of bt.n * pcg_slab_doubles(..) doubles.  Bit m of `active` clear: item m is skipped
// (vectors, slab, scalars untouched).  Item m's vectors and scalars have the bits of the single pass on item m alone.
void pcg_direction_many(const real_t *so, const Op3 *op27, const real_t *z, const real_t *p, real_t *pn, real_t *w, int nd,
                        int nst, int II, int JJ, int KK, bool first, real_t *slab, real_t *sc, hipStream_t st, Batch bt,
                        unsigned active);
// the direction pass of a periodic level (2D or 3D) on a batch: pcg_direction_periodic per item, the operator fetched once
void pcg_direction_periodic_many(const real_t *so, const real_t *z, const real_t *p, real_t *pn, real_t *w, int nd, int nst, int II,
                                 int JJ, int KK, int ibc, bool first, real_t *slab, real_t *sc, hipStream_t st, Batch bt,
                                 unsigned active);
void pcg_update_many(int zmode, bool move, real_t *x, real_t *r, const real_t *p, const real_t *w, real_t *z,
                     const real_t *diag, int II, int JJ, int KK, bool first, real_t *slab, real_t *sc, hipStream_t st,
                     Batch bt, unsigned active);
// The dots of flexible CG (cedar_amd_solver_fcg) after the preconditioner, no vector written: r.r, r.z and w.z with w = A p
// still in its buffer, then sc[PCG_WZ] = w.z, beta = -((alpha w.z) / rho) (first or rho = 0: 0) and rho = r.z.  r.r and r.z
// have the bits of pcg_update(2, false, ..); alpha, sigma and the flag are left alone.  _many: per active item.
void pcg_dots_wz(const real_t *r, const real_t *z, const real_t *w, int II, int JJ, int KK, bool first, real_t *slab,
                 real_t *sc, hipStream_t st);
void pcg_dots_wz_many(const real_t *r, const real_t *z, const real_t *w, int II, int JJ, int KK, bool first, real_t *slab,
                      real_t *sc, hipStream_t st, Batch bt, unsigned active);
// On a rank grid (dist_common.h dist_pcg) pcg_direction and pcg_update get `partial`: instead of the one-rank second stage they
// leave this rank's slab sums there (direction: sigma; update: r.r, and r.z unless zmode 0; zmode 3: nothing -- r.r is
// gathered with r.z after the preconditioner).  After the all-gather of `stride` doubles per rank, the _ranks kernels
// sum the partials in rank order and set the scalars as the one-rank stages do (world = 1: the same values bit for bit).
void pcg_ranks_alpha(const real_t *gathered, int world, int stride, real_t *sc, hipStream_t st);
void pcg_ranks_rho(int zmode, const real_t *gathered, int world, int stride, bool first, real_t *sc, hipStream_t st);
// pn = z + beta p (first: pn = z) on up to 26 boxes (i0, j0, k0, ni, nj, nk) of a box of II x JJ rows: the ghost cells
// of a rank box that its neighbours own
struct ShellBoxes {
	int n = 0;
	int box[26 * 6];
};
void pcg_ghost_shell(const real_t *z, const real_t *p, real_t *pn, const real_t *sc, const ShellBoxes &bx, int II, int JJ,
                     bool first, hipStream_t st);
// many3d.hip: the 3D solve-phase kernels on a batch of right-hand sides (cedar_amd_solver_*_many): the operator entries of a
// workgroup task are fetched once and applied to every item from registers; reference term order, so item m has the bits
// of the single-vector reference-order kernels on item m alone.  bf / bc: batch strides of the fine / coarse vectors.
void relax3_gs27_many(const Op3 &A, const real_t *qf, real_t *q, int II, int JJ, int KK, int updown, hipStream_t st, Batch bt);
void residual27_many(const Op3 &A, const real_t *qf, const real_t *q, real_t *res, int II, int JJ, int KK, hipStream_t st, Batch bt);
// the same two on the single-precision view; the sweep serves rows of at most 1024 points and launches nothing on longer
// ones (no level with such rows takes the float copy, and cedar_amd_relax3_gs_many_op32 refuses them)
void relax3_gs27_many(const Op3f &A, const real_t *qf, real_t *q, int II, int JJ, int KK, int updown, hipStream_t st, Batch bt);
void residual27_many(const Op3f &A, const real_t *qf, const real_t *q, real_t *res, int II, int JJ, int KK, hipStream_t st, Batch bt);
void relax3_gs7_many(const real_t *so, const real_t *qf, real_t *q, const real_t *sor, int II, int JJ, int KK, int updown,
                     hipStream_t st, Batch bt);
void residual7_many(const real_t *so, const real_t *qf, const real_t *q, real_t *res, int II, int JJ, int KK, hipStream_t st, Batch bt);
void restrict3_many(const real_t *q, real_t *qc, const real_t *ci, int II, int JJ, int KK, int IIC, int JJC, int KKC,
                    hipStream_t st, Batch bf, Batch bc);
void interp_add3_many(real_t *q, const real_t *qc, const real_t *so, real_t *res, const real_t *ci,
                      int IIC, int JJC, int KKC, int IIF, int JJF, int KKF, hipStream_t st, Batch bf, Batch bc);
// one row class / one colour of the two batched sweeps (the periodic batch refreshes ghosts in between); perx: x is
// periodic with an even number of points and the row task refreshes the x ghosts of its row per item
void relax3_class27_many(const Op3 &A, const real_t *qf, real_t *q, int II, int JJ, int KK, int jb, int kb, bool efirst,
                         hipStream_t st, Batch bt, bool perx = false);
void relax3_colour7_many(const real_t *so, const real_t *qf, real_t *q, const real_t *sor, int II, int JJ, int KK, int pts,
                         hipStream_t st, Batch bt);
// periodic_many3d.hip: the periodic 3D sweep and transfers on a batch stored with stride II*JJ*KK (ipn as above).  Item m of
// every result has the bits of the single-vector periodic call on item m alone.  (The coarsest solve of a batch is
// solve_cg3_per.)
void relax3_gs_per_many(const real_t *so, const real_t *qf, real_t *q, const real_t *sor, int II, int JJ, int KK, int nstncl,
                        int updown, int ipn, hipStream_t st, int ghosts_consistent, Batch bt);
void restrict3_per_many(real_t *q, real_t *qc, const real_t *ci, int II, int JJ, int KK, int IIC, int JJC, int KKC, int ipn,
                        hipStream_t st, Batch bf, Batch bc);
void interp_add3_per_many(real_t *q, const real_t *qc, const real_t *so, real_t *res, const real_t *ci, int IIC, int JJC,
                          int KKC, int IIF, int JJF, int KKF, int ipn, hipStream_t st, Batch bf, Batch bc);
// periodic_many2d.hip: the periodic 2D sweep on a batch stored with stride II*JJ (ipn = 1 per_y, 2 per_x, 3 per_xy), bit for
// bit relax2_gs_per per item.  1 = rows too long; a batch with another stride walks its items through relax2_gs_per.  (The
// transfers and the coarsest solve of a batch are restrict2_per, interp_add2_per and solve_cg2_per.)
int relax2_gs_per_many(const real_t *so, const real_t *qf, real_t *q, const real_t *sor, int II, int JJ, int nstncl, int updown,
                       int ipn, hipStream_t st, Batch bt);
// gallery.hip (device-side generators of the reference's gallery operators)
void gallery_fill(int which, real_t *so, real_t *b, int nx, int ny, int nz, const double *params, hipStream_t st);

// XCD-aware block remap: consecutive logical blocks land on the same XCD
// (blocks b and b+8 share an XCD under round-robin dispatch; speed only).
__device__ __forceinline__ unsigned xcd_remap(unsigned b, unsigned nblk)
{
	unsigned chunk = (nblk + 7u) >> 3;
	return (b & 7u) * chunk + (b >> 3);
}
static inline unsigned xcd_grid(unsigned nblk) { return ((nblk + 7u) >> 3) << 3; }

// Row (jr,kr) owned by logical workgroup L: rows are walked in 2^tjl x 2^tkl (j,k) tiles so that
// the ~64 workgroups an XCD has in flight form a compact patch of rows and find each other's rows
// (q rows j+-1,k+-1; operator rows stored at j+1 / k+1) in that XCD's L2 instead of HBM.
// tkl = 0 degenerates to the plain j-fastest walk.
struct TileShape { unsigned tjl, tkl; };
__device__ __forceinline__ bool tile_rows(unsigned L, unsigned nj, unsigned nk, TileShape ts, unsigned &jr, unsigned &kr)
{
	const unsigned ntj = (nj + (1u << ts.tjl) - 1u) >> ts.tjl;
	const unsigned tile = L >> (ts.tjl + ts.tkl), w = L & ((1u << (ts.tjl + ts.tkl)) - 1u);
	jr = ((tile % ntj) << ts.tjl) + (w & ((1u << ts.tjl) - 1u));
	kr = ((tile / ntj) << ts.tkl) + (w >> ts.tjl);
	return jr < nj && kr < nk;
}
__host__ __device__ static inline unsigned tile_blocks(unsigned nj, unsigned nk, TileShape ts)
{
	return (((nj + (1u << ts.tjl) - 1u) >> ts.tjl) * ((nk + (1u << ts.tkl) - 1u) >> ts.tkl)) << (ts.tjl + ts.tkl);
}
// default shapes (measured on MI355X, profiles/): overridable for experiments with
// CEDAR_AMD_TILE_RELAX="tjl,tkl" / CEDAR_AMD_TILE_RESID="tjl,tkl"
TileShape tile_shape_relax();
TileShape tile_shape_resid();

} // namespace cedar_amd
