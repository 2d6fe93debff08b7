/* cedar_amd -- C ABI of the MI355X-native BoxMG V-cycle hot path.
 *
 * Two layers, both plain C (pointers + sizes, no C++/torch types):
 *
 * 1. Kernel drop-ins.  Exactly the `extern "C"` symbols that Cedar's C++
 *    binding classes call into its Fortran library;
 *    same names, argument order, by-value/by-pointer conventions and array
 *    layouts (FP64, Fortran order, one ghost layer, pointer to the first
 *    element including ghosts).  Each array argument may be a host pointer
 *    (the library stages it through HBM: correct, PCIe-bound) or a device
 *    pointer obtained from cedar_amd_malloc/hipMalloc (operated on in place).
 *    Linking Cedar against libcedar_amd.so instead of its Fortran objects
 *    therefore routes the whole hot path to the GPU without source changes.
 *    Boundary codes (jpn / ibc, what BMG_get_bc returns for grid.periodic): 0 definite and the definite
 *    periodic codes -- 2D 1 (y), 2 (x), 3 (xy); 3D also 5 (z), 6 (xz), 7 (yz), 8 (xyz), with even extents in the
 *    periodic directions for the two 3D set-up routines.  The indefinite codes (< 0) report through print_error
 *    and return.  3D: where the reference's periodic Fortran is not self-consistent (the ghost loops of
 *    BMG3_SymStd_interp_add.f90:253-272, dense-matrix entries of SETUP_cg_LU for xz / xyz / xy with nx != ny) the
 *    library applies the periodic operator itself; DESIGN.md section 6 has the evidence.
 *
 * 2. Handle API.  Device-resident hierarchy, modelled on Cedar's own C
 *    interface (include/cedar/2d/interface/c/solver.h: bmg2_solver_create /
 *    _run / _destroy): create uploads the fine operator and runs the whole
 *    set-up phase on the GPU, run/vcycle keep every level in HBM.
 *
 * Errors: like the reference, kernels report through the host-supplied
 * callback `print_error(char*)` (src/2d/ftn/ModInterface.f90:4-9); if the
 * host program does not define it the library's weak default writes to stderr.
 * Threading: none (one solver per process/rank, like the reference).
 */
#ifndef CEDAR_AMD_H
#define CEDAR_AMD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef double real_t;
typedef unsigned int len_t;

/* ------------------------------------------------------------------ 1. drop-ins */

/* replaces src/2d/ftn/BMG_get_bc.f90:1-24 (decl. include/cedar/2d/relax.h:24) */
void BMG_get_bc(int per_mask, int *ibc);

/* include/cedar/2d/relax.h:13  <- src/2d/ftn/BMG2_SymStd_SETUP_recip.f90 */
void BMG2_SymStd_SETUP_recip(real_t *so, real_t *sor, len_t nx, len_t ny, int nstncl, int nsor_v);
/* include/cedar/2d/relax.h:14-15 <- BMG2_SymStd_SETUP_lines_x/_y.f90 */
void BMG2_SymStd_SETUP_lines_x(real_t *SO, real_t *SOR, len_t Nx, len_t Ny, int NStncl, int JPN);
void BMG2_SymStd_SETUP_lines_y(real_t *SO, real_t *SOR, len_t Nx, len_t Ny, int NStncl, int JPN);
/* include/cedar/2d/relax.h:16-17 <- BMG2_SymStd_relax_GS.f90 */
void BMG2_SymStd_relax_GS(int k, real_t *SO, real_t *QF, real_t *Q, real_t *SOR, len_t II, len_t JJ,
                          int kf, int ifd, int nstncl, int nsorv, int irelax_sym, int updown, int jpn);
/* include/cedar/2d/relax.h:18-23 <- BMG2_SymStd_relax_lines_x/_y.f90 */
void BMG2_SymStd_relax_lines_x(int k, real_t *SO, real_t *QF, real_t *Q, real_t *SOR, real_t *B,
                               len_t II, len_t JJ, int kf, int ifd, int nstencil, int irelax_sym,
                               int updown, int jpn);
void BMG2_SymStd_relax_lines_y(int k, real_t *SO, real_t *QF, real_t *Q, real_t *SOR, real_t *B,
                               len_t II, len_t JJ, int kf, int ifd, int nstencil, int irelax_sym,
                               int updown, int jpn);
/* include/cedar/2d/residual.h:9-10 <- BMG2_SymStd_residual.f90 (everything by pointer) */
void BMG2_SymStd_residual(int *k, real_t *SO, real_t *QF, real_t *Q, real_t *RES, len_t *II, len_t *JJ,
                          int *kf, int *ifd, int *nstncl, int *ibc, int *irelax, int *irelax_sym,
                          int *updown);
/* src/2d/restrict.cc:6-7 <- BMG2_SymStd_restrict.f90 */
void BMG2_SymStd_restrict(real_t *Q, real_t *QC, real_t *CI, int Nx, int Ny, int Nxc, int Nyc, int jpn);
/* src/2d/interp.cc:8-9 <- BMG2_SymStd_interp_add.f90 */
void BMG2_SymStd_interp_add(real_t *Q, real_t *QC, real_t *RES, real_t *SO, real_t *CI,
                            len_t IIC, len_t JJC, len_t IIF, len_t JJF, int nstncl, int jpn);
/* src/2d/interp.cc:10-12 <- BMG2_SymStd_SETUP_interp_OI.f90 */
void BMG2_SymStd_SETUP_interp_OI(real_t *so, real_t *soc, real_t *ci, len_t iif, len_t jjf,
                                 len_t iic, len_t jjc, int ifd, int nstncl, int jpn, int irelax);
/* include/cedar/2d/coarsen.h:10-12 <- BMG2_SymStd_SETUP_ITLI_ex.f90 */
void BMG2_SymStd_SETUP_ITLI_ex(real_t *so, real_t *soc, real_t *ci, len_t iif, len_t jjf,
                               len_t iic, len_t jjc, int ifd, int nstncl, int ipn);
/* include/cedar/2d/solve_cg.h:10 <- BMG2_SymStd_SETUP_cg_LU.f90 (everything by pointer) */
void BMG2_SymStd_SETUP_cg_LU(real_t *so, len_t *ii, len_t *jj, int *nstncl, real_t *abd,
                             len_t *nabd1, len_t *nabd2, int *ibc);
/* src/2d/solve_cg.cc:6 <- BMG2_SymStd_SOLVE_cg.f90 */
void BMG2_SymStd_SOLVE_cg(real_t *q, real_t *qf, len_t ii, len_t jj, real_t *abd, real_t *bbd,
                          len_t nabd1, len_t nabd2, int ibc);

/* include/cedar/3d/relax.h:11-16 */
void BMG3_SymStd_SETUP_recip(real_t *so, real_t *sor, len_t nx, len_t ny, len_t nz, int nstencl, int nsorv);
void BMG3_SymStd_relax_GS(int kg, real_t *so, real_t *qf, real_t *q, real_t *sor,
                          len_t ii, len_t jj, len_t kk, int ifd, int nstncl, int nsorv,
                          int irelax_sym, int updown, int jpn);
/* include/cedar/3d/residual.h:10-13 */
void BMG3_SymStd_residual(int kg, int NOG, int ifd, real_t *q, real_t *qf, real_t *so, real_t *RES,
                          len_t ii, len_t jj, len_t kk, int NStncl);
/* src/3d/restrict.cc:7-10 */
void BMG3_SymStd_restrict(real_t *q, real_t *qc, real_t *ci, len_t nx, len_t ny, len_t nz,
                          len_t nxc, len_t nyc, len_t nzc, int jpn);
/* src/3d/interp.cc:7-11 (NB: so,res order differs from 2D) */
void BMG3_SymStd_interp_add(real_t *q, real_t *qc, real_t *so, real_t *res, real_t *ci,
                            len_t iic, len_t jjc, len_t kkc, len_t iif, len_t jjf, len_t kkf,
                            int NStncl, int jpn);
/* include/cedar/3d/interp.h:11-15 (yo is scratch of the reference and is not touched) */
void BMG3_SymStd_SETUP_interp_OI(real_t *so, real_t *soc, real_t *ci, len_t iif, len_t jjf, len_t kkf,
                                 len_t iic, len_t jjc, len_t kkc, int ifd, int nstncl, int irelax,
                                 int jpn, real_t *yo);
/* include/cedar/3d/coarsen.h:12-16 */
void BMG3_SymStd_SETUP_ITLI07_ex(real_t *so, real_t *soc, real_t *ci, len_t iif, len_t jjf, len_t kkf,
                                 len_t iic, len_t jjc, len_t kkc, int ipn);
void BMG3_SymStd_SETUP_ITLI27_ex(real_t *so, real_t *soc, real_t *ci, len_t iif, len_t jjf, len_t kkf,
                                 len_t iic, len_t jjc, len_t kkc, int ipn);
/* include/cedar/3d/solve_cg.h:10-11, src/3d/solve_cg.cc:6-9 */
void BMG3_SymStd_SETUP_cg_LU(real_t *so, len_t ii, len_t jj, len_t kk, int NStncl, real_t *abd,
                             len_t nabd1, len_t nabd2, int ibc);
void BMG3_SymStd_SOLVE_cg(real_t *q, real_t *qf, len_t ii, len_t jj, len_t kk, real_t *abd,
                          real_t *bbd, len_t nabd1, len_t nabd2, int ibc);

/* ------------------------------------------------------------------ device memory helpers */
int cedar_amd_device_count(void);                 /* 0 when no GPU is visible (no HIP context made) */
int cedar_amd_set_device(int dev);                /* 0 on success */
void *cedar_amd_malloc(size_t bytes);             /* zero-filled HBM */
void cedar_amd_free(void *dptr);
void cedar_amd_memcpy_h2d(void *dst, const void *src, size_t bytes);
void cedar_amd_memcpy_d2h(void *dst, const void *src, size_t bytes);
void cedar_amd_memcpy_d2d(void *dst, const void *src, size_t bytes);
void cedar_amd_memset(void *dst, int value, size_t bytes);
void cedar_amd_sync(void);
/* all launches of this library go to this stream (default: the null stream) */
void cedar_amd_set_stream(void *hip_stream);
void *cedar_amd_get_stream(void);
/* ||v||_2 over the interior (grid_func::lp_norm<2>); v host or device; KK = 1 for 2D */
double cedar_amd_l2norm(const real_t *v, len_t II, len_t JJ, len_t KK);

/* qf = A q on the interior (kernels::matvec; arithmetic of src/2d/ftn/mpi/BMG2_SymStd_UTILS_matvec.f90:84-118
 * and src/3d/ftn/mpi/BMG3_SymStd_UTILS_matvec.f90:80-127, on the serial array layout of this header:
 * SO(II,JJ[,KK],nstncl)); nstncl = 3|5 (2D), 4|14 (3D); host or device pointers. */
void cedar_amd_matvec2(const real_t *so, const real_t *q, real_t *qf, len_t II, len_t JJ, int nstncl);
void cedar_amd_matvec3(const real_t *so, const real_t *q, real_t *qf, len_t II, len_t JJ, len_t KK, int nstncl);

/* device-side gallery (src/2d/gallery.cc, src/3d/gallery.cc); `so`/`b` device or host.
 * which: 0 poisson2, 1 diag_diffusion2(dx,dy), 2 fe2, 10 poisson3, 11 diag_diffusion3, 12 fe3;
 * b (may be NULL) receives the examples' rhs (examples/basic-2d-ser/poisson.cc:15-37). */
void cedar_amd_gallery(int which, real_t *so, real_t *b, len_t nx, len_t ny, len_t nz,
                       const double *params);

/* ------------------------------------------------------------------ 1b. pieces for domain-decomposed runs
 * The MPI flavour of the reference interleaves halo exchanges with the colours of a sweep and
 * with the phases of the interpolation set-up (src/3d/ftn/mpi/BMG3_SymStd_relax_GS.f90:102-147,
 * src/3d/ftn/mpi/BMG3_SymStd_SETUP_interp_OI.f90:418-1074).  These entry points expose the same
 * granularity so that a host (cedar_amd/dist.py) can place RCCL exchanges between them.
 * Arrays: host or device, local subdomain incl. one ghost layer, Cedar layout. */
/* one row class (jb,kb in {0,1}: parity of 1-based j,k minus 2) of the 27-point sweep: both i-colours,
 * efirst != 0: even 1-based i first (the UP order) */
void cedar_amd_relax3_pass(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, len_t kk,
                           int jb, int kb, int efirst);
/* the same restricted to a part of the class rows: part 1 = rows none of whose j,k neighbours is a
 * ghost row (they do not read the y/z ghost layers and may run while those are being exchanged),
 * part 2 = the remaining shell, part 0 = all.  Rows of a class do not couple: 1 then 2 equals 0.
 * part may carry, shifted left by 4, the faces of the box that have a neighbouring rank (bit 0 -y, 1 +y, 2 -z,
 * 3 +z): rows next to a face without one read no exchanged ghost and count as interior; no bit set = all four. */
void cedar_amd_relax3_pass_part(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, len_t kk,
                                int jb, int kb, int efirst, int part);
/* both row classes of the planes of k-parity kb in sweep order (up != 0: the UP order): the unit between two
 * halo exchanges on a slab decomposition (rank grid 1 x 1 x pz), run with the plane-fused kernel on big
 * levels.  part: 0 = all planes of the parity, 1 = planes whose k-neighbours are both owned, 2 = the others;
 * the -z / +z bits of the face mask of cedar_amd_relax3_pass_part apply (part | sides << 4). */
void cedar_amd_relax3_planes(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, len_t kk,
                             int kb, int up, int part);
/* Register the 27-point operator `so` (device pointer, with its SETUP_recip output `sor`) with the library: on levels
 * with at least 320 rows the pieces above and BMG3_SymStd_relax_GS / _residual then read a row-interleaved solve copy
 *  instead of the fourteen Cedar-layout planes, and cedar_amd_relax3_planes runs the sweep with
 * inter-plane partial sums (cedar_amd_relax3_gs_psum below; levels with at least 160 rows, CEDAR_AMD_PSUM=0: never) on a
 * scratch vector kept with the registration.  Returns bit 0: a solve copy was made, bit 1: the scratch was.  Call again
 * after the operator changed; release before freeing it.  The resident solver (section 2) does this by itself. */
int cedar_amd_relax3_prepare(const real_t *so, const real_t *sor, len_t ii, len_t jj, len_t kk);
/* the same with the partial-sum sweep registered from psum_min_rows rows on (runs of 8 rows below 160 rows) for
 * cedar_amd_relax3_planes_masked: on a rank grid with an x / y split the alternative to it is not four row-class launches but
 * four passes with an exchange after each, and the sweep pays from 128 rows on (what cedar_amd_dist3_* registers) */
int cedar_amd_relax3_prepare_rows(const real_t *so, const real_t *sor, len_t ii, len_t jj, len_t kk, int psum_min_rows);
void cedar_amd_relax3_release(const real_t *so);
/* One 27-point sweep (BMG3_SymStd_relax_GS.f90:80-138, Dirichlet) with INTER-PLANE PARTIAL SUMS: the planes of the
 * first k-parity are relaxed in the reference's order and leave, per point of the planes between them, the sums of the
 * nine products towards the plane below and above; the second k-parity adds those two sums to its eight in-plane terms
 * instead of re-reading eighteen operator slot-rows.  Same products as the reference, the 26-term sum of :104-131
 * re-associated for the second k-parity: results agree with BMG3_SymStd_relax_GS to rounding (not bit for bit); this is
 * the sweep the resident solver runs on levels with at least 320 rows (CEDAR_AMD_PSUM=0: reference order).  scratch: a
 * device array of the vector's size, or NULL (the library takes one from its pool).  Run length: CEDAR_AMD_FRUN.
 * Returns 1, or 0 when the level cannot take it (rows longer than 512 points, fewer than four runs per plane) and the
 * reference-order sweep was run instead. */
int cedar_amd_relax3_gs_psum(real_t *so, real_t *qf, real_t *q, real_t *sor, real_t *scratch, len_t ii, len_t jj, len_t kk,
                             int updown);
/* One 27-point sweep / residual with the operator and 1/diag rounded to single precision (what a level of a solver
 * after cedar_amd_solver_use_fp32_operator runs): a row-interleaved float copy is built for the call, the kernels
 * promote its entries to double on load, vectors and arithmetic stay FP64 -- bit for bit the FP64 kernels on the
 * rounded arrays.  frun > 0: the partial-sum sweep with runs of frun rows where the level can take it (at least four
 * runs per plane, rows of at most 512 points; returns 1), else -- and with frun = 0 -- the reference order (returns 0;
 * CEDAR_AMD_FRUN picks the plane-fused or the row kernels as for BMG3_SymStd_relax_GS).  Rows longer than 1024 points
 * or an entry that overflows float: print_error, -1, q / res untouched.  scratch as for cedar_amd_relax3_gs_psum. */
int cedar_amd_relax3_gs_op32(real_t *so, real_t *qf, real_t *q, real_t *sor, real_t *scratch, len_t ii, len_t jj, len_t kk,
                             int updown, int frun);
int cedar_amd_residual3_op32(real_t *so, real_t *qf, real_t *q, real_t *res, len_t ii, len_t jj, len_t kk);
/* The same for a 7-point operator (so: 4 planes; what the 7-point level of a solver runs after
 * cedar_amd_solver_use_fp32_operator_all): a row-interleaved float copy of KPW, KPS, KB, the diagonal and 1/diag is built
 * for the call and dropped after it.  The sweep is two colour launches in the reference's order (updown 1 = UP: colours
 * 0, 1; 0 = DOWN: 1, 0; BMG3_SymStd_relax_GS.f90:144-184), the residual keeps BMG3_SymStd_residual's term order; entries
 * are promoted to double on load, vectors and arithmetic stay FP64 -- bit for bit BMG3_SymStd_relax_GS /
 * BMG3_SymStd_residual on so and sor rounded to float.  Rows of any length.  Returns 0; a NULL array or an entry that
 * overflows float: print_error, -1, q / res untouched. */
int cedar_amd_relax7_gs_op32(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, len_t kk, int updown);
int cedar_amd_residual7_op32(real_t *so, real_t *qf, real_t *q, real_t *res, len_t ii, len_t jj, len_t kk);
/* The 2D analogue for nine-point operators (BMG2_SymStd_relax_GS.f90:89-114): the band-fused sweep whose S rows take the
 * six couplings to the two neighbouring F rows as ONE partial-sum row kept in LDS by the workgroup that has just relaxed
 * those F rows.  Same contract as cedar_amd_relax3_gs_psum; the resident solver runs it on levels with at least 4096 rows
 * (rows of 2048 to 4350 points; CEDAR_AMD_FRUN2 = run length).  Returns 1, or 0 when the reference-order sweep ran. */
int cedar_amd_relax2_gs_psum(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, int updown);
/* The 2D point sweep and residual on the operator and 1/diag rounded to single precision (so: nstncl = 5 | 3 planes; what
 * a 2D level runs after cedar_amd_solver_use_fp32_operator_2d): a row-interleaved float copy of KW, KS, [KSW, KNW,] KO and
 * 1/diag is built for the call and dropped after it; entries are promoted to double on load, vectors and arithmetic stay
 * FP64 -- bit for bit BMG2_SymStd_relax_GS / BMG2_SymStd_residual (and cedar_amd_relax2_gs_psum, at the same run length)
 * on so and sor rounded to float.  Rows of any length.
 *   cedar_amd_relax2_gs_op32       reference order (CEDAR_AMD_FRUN2 picks band-fused or two launches as for
 *                                  BMG2_SymStd_relax_GS); returns 0;
 *   cedar_amd_relax2_gs_psum_op32  nine-point only; returns 1, or 0 when the reference-order sweep ran, as
 *                                  cedar_amd_relax2_gs_psum does;
 *   cedar_amd_residual2_op32       returns 0.
 * A NULL array, nstncl other than 3 / 5, or an entry that overflows float: print_error, -1, q / res untouched. */
int cedar_amd_relax2_gs_op32(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, int nstncl, int updown);
int cedar_amd_relax2_gs_psum_op32(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, int updown);
int cedar_amd_residual2_op32(real_t *so, real_t *qf, real_t *q, real_t *res, len_t ii, len_t jj, int nstncl);
/* the same on nrhs (1 .. 32) items stored back to back, the operator shared: item m has the bits of the single call on
 * item m alone; nrhs outside 1 .. 32: print_error, -1 */
int cedar_amd_relax2_gs_many_op32(int nrhs, real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, int nstncl,
                                  int updown);
int cedar_amd_residual2_many_op32(int nrhs, real_t *so, real_t *qf, real_t *q, real_t *res, len_t ii, len_t jj, int nstncl);
/* One zebra line sweep (both colours) on the operator and the line factors rounded to single precision (so: nstncl = 5 | 3
 * planes; what a 2D level runs after cedar_amd_solver_use_fp32_operator_lines): the row-interleaved float copy of the
 * operator and float copies of the factors are built for the call and dropped after it; entries and factors are promoted to
 * double on load, vectors, the scan and all arithmetic stay FP64 -- bit for bit BMG2_SymStd_relax_lines_x / _y (Dirichlet)
 * on so and sor rounded to float.
 *   dir 0: x lines, sor as BMG2_SymStd_SETUP_lines_x leaves it;
 *   dir 1: y lines, sor the transposed SOR(JJ,II,2) of BMG2_SymStd_SETUP_lines_y; runs on transposed arrays, as the
 *          resident solver does.
 * _many: nrhs (1 .. 32) items stored back to back, operator and factors shared; item m has the bits of the single call on
 * item m alone.  Returns 0; a NULL array, nrhs outside 1 .. 32, nstncl other than 3 / 5, an entry or factor that
 * overflows float, or a line that does not fit the LDS of a CU: print_error, -1, q untouched. */
int cedar_amd_relax2_lines_op32(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, int nstncl, int dir,
                                int updown);
int cedar_amd_relax2_lines_many_op32(int nrhs, real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, int nstncl,
                                     int dir, int updown);
/* recompute column icol (0-based incl. ghost) of that row class after its x-neighbour column changed */
void cedar_amd_relax3_fixup(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, len_t kk,
                            int icol, int jb, int kb);
/* Boundary-first pieces of a k-parity of planes on a rank grid with an x / y split (what cedar_amd_dist3_* runs where the
 * level takes the partial-sum sweep; the MPI flavour of the reference exchanges after every colour,
 * src/3d/ftn/mpi/BMG3_SymStd_relax_GS.f90:102-147).  The few columns and rows whose values a neighbouring rank waits for,
 * or which wait for a neighbour's, are relaxed stage by stage in the reference order with the exchanges between the
 * stages; one launch then relaxes everything else of the parity and leaves those points as they are:
 *   _rows: rows j0, j0+jstep, .. (nrj rows, 0-based incl. ghost) of every plane of parity kb, both i-colours;
 *   _cols: the points of the listed columns (0-based incl. ghost, relaxed in the order given) in every row of class
 *          (jb,kb) except the rows xrow0 / xrow1 (-1: none);
 *   _planes_masked: cedar_amd_relax3_planes for all planes of the parity, with the points named by the masks skipped --
 *          cols_f / cols_s for the first / second row class of the sweep order: bits 0..3 = columns 1..4, bits 4..7 = the
 *          last four owned columns; rows[3]: whole rows (-1: unused).  Needs even nx and ny, 8 to 512 columns and the
 *          registration of cedar_amd_relax3_prepare with its scratch (cedar_amd_relax3_masked_ok); returns 0 (nothing done,
 *          q untouched) otherwise. */
void cedar_amd_relax3_rows(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, len_t kk, int j0, int jstep,
                           int nrj, int kb, int efirst);
void cedar_amd_relax3_cols(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, len_t kk, int jb, int kb,
                           int ncol, const int *cols, int xrow0, int xrow1);
int cedar_amd_relax3_planes_masked(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, len_t kk, int kb,
                                   int up, unsigned cols_f, unsigned cols_s, const int *rows);
/* The predicate of _planes_masked, which applies it before it launches: 1 where ii-2 and jj-2 are even, a row has 8 to 512
 * points and `so` is registered with its partial-sum scratch for this shape; so = NULL: the shape alone.  cedar_amd_dist3_*
 * decides with it which levels take the boundary-first chain, so the driver and the launch cannot disagree. */
int cedar_amd_relax3_masked_ok(const real_t *so, len_t ii, len_t jj, len_t kk);
/* _cols on a dense copy of the six operator columns next to an x face (device pointers only; at least 12 columns per row):
 * _strip_build fills out[_strip_doubles(jj,kk)] for the low (side 0: columns 0..5) or the high (side 1: ii-6..ii-1) face from
 * the operator and its SETUP_recip output; _cols_strip takes the copies of the sides its columns lie on (the other may be
 * NULL).  Same arithmetic as _cols, a fraction of its memory traffic. */
size_t cedar_amd_relax3_strip_doubles(len_t jj, len_t kk);
void cedar_amd_relax3_strip_build(const real_t *so, const real_t *sor, len_t ii, len_t jj, len_t kk, int side, real_t *out);
void cedar_amd_relax3_cols_strip(const real_t *strip_lo, const real_t *strip_hi, real_t *qf, real_t *q, len_t ii, len_t jj, len_t kk,
                                 int jb, int kb, int ncol, const int *cols, int xrow0, int xrow1);
/* one colour of the 7-point red-black sweep (pts = 0|1, BMG3_SymStd_relax_GS.f90:155-184) */
void cedar_amd_relax3_colour7(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, len_t kk,
                              int pts);
/* one phase (0 edges, 1 faces, 2 centres) of BMG3_SymStd_SETUP_interp_OI with lower loop bounds
 * ilo,jlo,klo (3 = serial / physical boundary, 2 = a neighbouring subdomain owns coarse point 1) */
void cedar_amd_setup_interp3_phase(real_t *so, real_t *ci, len_t iif, len_t jjf, len_t kkf,
                                   len_t iic, len_t jjc, len_t kkc, int ifd, int nstncl, int phase,
                                   int ilo, int jlo, int klo);

/* the 2D counterparts (src/2d/ftn/mpi/BMG2_SymStd_relax_GS.f90, ..._SETUP_interp_OI.f90): one row class of
 * the nine-point sweep (jb in {0,1}; efirst != 0: even 1-based i first = the 2D DOWN order), the column
 * fix-up after the x-neighbour's first colour arrived, one colour of the five-point sweep (jo in {2,3}),
 * one phase (0 edges, 1 centres) of the interpolation set-up with lower loop bounds ilo, jlo (3 | 2) */
void cedar_amd_relax2_pass(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, int jb, int efirst);
void cedar_amd_relax2_fixup(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, int icol, int jb);
void cedar_amd_relax2_colour5(real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, int jo);
void cedar_amd_setup_interp2_phase(real_t *so, real_t *ci, len_t iif, len_t jjf, len_t iic, len_t jjc,
                                   int ifd, int nstncl, int phase, int ilo, int jlo);
/* first-order recurrences over `nlines` line-contiguous vectors (leading dimension ld), in place, device
 * pointers: forward y_i = a_i y_{i-1} + c_i (reverse = 0) or backward y_i = a_i y_{i+1} + c_i (reverse = 1)
 * from a zero carry, c_i = y_i on entry (divided by div_i when div != NULL).  The two sweeps of DPTTRS per
 * line segment for the domain-decomposed line relaxation (src/2d/ftn/mpi/BMG2_SymStd_relax_lines_x.f90). */
void cedar_amd_affine_lines(real_t *y, const real_t *a, const real_t *div, int nlines, int n, int ld, int reverse);
/* around it (device pointers): right-hand sides b - (off-line part of A) x of the lines of zebra colour lb
 * (0-based interior parity) in direction dir (0 = x lines, 1 = y lines) into out[line][position]
 * (relax_lines_x.f90:104-109, relax_lines_y.f90:103-107); y[l][i] += p[l][i] * c[l] (the carry entering a
 * segment times the running product of its multipliers); and the solved lines back into q */
void cedar_amd_lines_rhs2(const real_t *so, const real_t *qf, const real_t *q, real_t *out, len_t ii, len_t jj,
                          int nstncl, int dir, int lb);
void cedar_amd_lines_carry(real_t *y, const real_t *p, const real_t *c, int nlines, int n, int ld);
void cedar_amd_lines_store2(const real_t *in, real_t *q, len_t ii, len_t jj, int dir, int lb);
/* pack (unpack = 0) / unpack (1) up to 26 sub-boxes of a device array (nplanes x kk x jj x ii) to /
 * from one contiguous device buffer in one launch: boxes = {i0,j0,k0,ni,nj,nk} per box (0-based incl.
 * ghost), offsets[b] = start of box b in the buffer in doubles per plane (box b occupies
 * offsets[b]*nplanes .. ).  Device pointers only. */
void cedar_amd_box_copy(real_t *arr, len_t ii, len_t jj, len_t kk, int nplanes, int nboxes,
                        const int *boxes, const unsigned long long *offsets, real_t *buf, int unpack);
/* the same with boxes = {i0,j0,k0,ni,nj,nk,sj,sk}: row j0 + j*sj, plane k0 + k*sk (the rows of one class / planes of one
 * k-parity of a face: what one stage of the boundary-first chain has changed) */
void cedar_amd_box_copy_strided(real_t *arr, len_t ii, len_t jj, len_t kk, int nplanes, int nboxes,
                                const int *boxes, const unsigned long long *offsets, real_t *buf, int unpack);

/* The passes of one conjugate-gradient iteration (krylov.hip), exactly as cedar_amd_solver_pcg and cedar_amd_dist{2,3}_pcg
 * launch them, on caller arrays: host or device pointers, Cedar layout incl. one ghost layer, kk = 1 for 2D.  They read
 * and write interiors only (the ghost shell pass: its boxes only); every other cell of an output array stays as given.
 * sc: the scalar block of a run, CEDAR_AMD_PCG_NSC doubles, slots below.  Each call takes its partial-sum slab from the
 * library's pool and fills it with NaN bit patterns first, so a slab entry that the second stage sums but no workgroup
 * wrote shows in the scalars.  All return 0, or -1 (nothing done, reported through print_error) on arguments they do
 * not serve. */
enum { CEDAR_AMD_PCG_RHO = 0, CEDAR_AMD_PCG_SIGMA = 1, CEDAR_AMD_PCG_ALPHA = 2, CEDAR_AMD_PCG_BETA = 3, CEDAR_AMD_PCG_RR = 4,
       CEDAR_AMD_PCG_RZ = 5, CEDAR_AMD_PCG_FLAG = 6, CEDAR_AMD_PCG_WZ = 7, CEDAR_AMD_PCG_NSC = 8 };
/* pn = z + beta p (first != 0: pn = z, p is not read and may be NULL), w = A pn with the terms of cedar_amd_matvec2 / 3
 * in their order, sigma = pn.w; nstncl = 3|5 (2D), 4|14 (3D).  beta = sc[BETA]; the neighbours of a point are
 * z + beta p of the input arrays, ghost cells included.  partial == NULL: the one-rank second stage -- sc[SIGMA] = sigma,
 * sc[ALPHA] = sc[RHO] / sigma, or 0 with sc[FLAG] = 1 (breakdown) when sigma <= 0, sigma is not finite or sc[RHO] = 0.
 * partial != NULL (rank grids): partial[0] = sigma and sc is only read.  A 27-point operator registered with
 * cedar_amd_relax3_prepare is read through its row-interleaved copy where it has one, as the solvers do. */
int cedar_amd_pcg_direction(const real_t *so, const real_t *z, const real_t *p, real_t *pn, real_t *w, len_t ii, len_t jj,
                            len_t kk, int nstncl, int first, real_t *sc, real_t *partial);
/* The same pass on a level with periodic directions, as cedar_amd_solver_fcg_periodic launches it.  ibc: the boundary code
 * of cedar_amd_settings (2D 1 = y, 2 = x, 3 = xy; 3D also 5 = z, 6 = xz, 7 = yz, 8 = xyz).  In a periodic direction a
 * stencil neighbour on the ghost layer is read at the opposite interior end (index 0 -> extent - 2, extent - 1 -> 1; edge
 * and corner neighbours in every combination): w is cedar_amd_matvec2 / 3 of pn with those ghosts wrapped, bit for bit,
 * and NO ghost cell of z or p in a periodic direction contributes to any result.  Ghosts of the other directions are read
 * as above.  The
 * operator is read where cedar_amd_pcg_direction reads it: its ghost layers must hold the periodic image, as the periodic
 * cycle requires.  A 27-point operator is read from its Cedar planes (a periodic level keeps no row-interleaved copy).
 * Everything else -- pn and w written in the interior only, the NaN-filled slab, sc, partial, the return values -- is
 * cedar_amd_pcg_direction's; ibc = 0 forwards to it; an ibc the dimension does not define is refused (-1). */
int cedar_amd_pcg_direction_periodic(const real_t *so, const real_t *z, const real_t *p, real_t *pn, real_t *w, len_t ii,
                                     len_t jj, len_t kk, int nstncl, int ibc, int first, real_t *sc, real_t *partial);
/* move != 0: x += alpha p, r -= alpha w with alpha = sc[ALPHA] (alpha = 0, the breakdown value: x and r are not touched,
 * whatever p and w hold); then r.r and r.z by zmode: 0 z = r (r.z = r.r), 1 z = r / diag written here (diag: the
 * operator's centre plane), 2 z read, 3 r.r only.  partial == NULL: sc[RR] = r.r and, unless zmode 3, sc[RZ] = r.z,
 * sc[BETA] = r.z / sc[RHO] (0 when first != 0 or sc[RHO] = 0), then sc[RHO] = r.z.  partial != NULL: partial[0] = r.r,
 * zmode 1 | 2 also partial[1] = r.z, zmode 3 nothing; sc is only read.  Arrays a mode does not use may be NULL. */
int cedar_amd_pcg_update(int zmode, int move, real_t *x, real_t *r, const real_t *p, const real_t *w, real_t *z,
                         const real_t *diag, len_t ii, len_t jj, len_t kk, int first, real_t *sc, real_t *partial);
/* The dots of flexible CG (cedar_amd_solver_fcg) after the preconditioner, one pass over r, z = M^-1 r and w = A p of the
 * iteration just made: sc[RR] = r.r, sc[RZ] = r.z (both with the bits of cedar_amd_pcg_update(2, 0, ..)), sc[WZ] = w.z,
 * sc[BETA] = -((sc[ALPHA] * w.z) / sc[RHO]) -- two roundings and an exact negation; 0 when first != 0 or sc[RHO] = 0 --
 * then sc[RHO] = r.z.  sc[ALPHA], sc[SIGMA], sc[FLAG] and the three arrays are only read. */
int cedar_amd_pcg_dots_wz(const real_t *r, const real_t *z, const real_t *w, len_t ii, len_t jj, len_t kk, int first,
                          real_t *sc);
/* the second stages of a rank grid: the ranks' partials (gathered[rank * stride + t], t = 0: sigma or r.r, t = 1: r.z)
 * summed in rank order, then the scalars as above; which = 0: alpha from sigma, 1: rho / beta by zmode.  world = 1 gives
 * the one-rank values bit for bit. */
int cedar_amd_pcg_rank_scalars(int which, int zmode, const real_t *gathered, int world, int stride, int first, real_t *sc);
/* pn = z + beta p (first != 0: pn = z) on up to 26 boxes {i0,j0,k0,ni,nj,nk} (0-based incl. ghost; host ints) of the
 * array: the ghost cells of a rank box that neighbouring ranks own */
int cedar_amd_pcg_ghost_shell(const real_t *z, const real_t *p, real_t *pn, len_t ii, len_t jj, len_t kk, int first,
                              const real_t *sc, const int *boxes, int nboxes);

/* ------------------------------------------------------------------ 2. handle API */
typedef struct cedar_amd_solver cedar_amd_solver;

enum { CEDAR_AMD_RELAX_POINT = 0, CEDAR_AMD_RELAX_LINE_X = 1, CEDAR_AMD_RELAX_LINE_Y = 2,
       CEDAR_AMD_RELAX_LINE_XY = 3,
       /* 3D plane relaxation, include/cedar/multilevel.h:149-159 ("plane-xy" .. "plane-xyz", src/multilevel_settings.cc:10-13) */
       CEDAR_AMD_RELAX_PLANE_XY = 4, CEDAR_AMD_RELAX_PLANE_XZ = 5, CEDAR_AMD_RELAX_PLANE_YZ = 6, CEDAR_AMD_RELAX_PLANE_XYZ = 7 };

typedef struct {
	int relaxation;   /* solver.relaxation   (default point)  src/multilevel_settings.cc:15-28 */
	int nrelax_pre;   /* solver.cycle.nrelax-pre  (2)   :38 */
	int nrelax_post;  /* solver.cycle.nrelax-post (1)   :39 */
	int num_levels;   /* solver.num-levels (-1 = automatic) :40 */
	int max_iter;     /* solver.max-iter (10) :41 */
	double tol;       /* solver.tol (1e-8) :42 */
	int min_coarse;   /* solver.min_coarse (3) :43 */
	int cycle;        /* solver.cycle.type: 0 = "v" (default), 1 = "f" (include/cedar/cycle/fcycle.h:49-83) :30-36 */
	int ibc;          /* boundary code of BMG_get_bc(per_mask) from grid.periodic (src/kernel_params.cc): 0 definite,
	                     1 periodic in y, 2 in x, 3 in xy; 3D also 5 z, 6 xz, 7 yz, 8 xyz (V-cycle; 3D: even extents in
	                     the periodic directions on every level that is coarsened) */
	/* "plane-config" of plane relaxation (src/kernel_params.cc:72-78: line-xy, max-iter 1 unless the configuration
	 * carries its own block; the other keys default like the solver's) */
	int plane_relaxation, plane_nrelax_pre, plane_nrelax_post, plane_max_iter, plane_min_coarse;
	double plane_tol;
} cedar_amd_settings;

void cedar_amd_default_settings(cedar_amd_settings *s);

/* nd = 2|3; nstencil = 3|5 (2D five/nine point), 4|14 (3D seven/xxvii point).
 * `so` (host or device) is the fine operator in Cedar's layout; it is copied
 * unless own_device_so != 0 and so is a device pointer, in which case the
 * solver uses it in place and the caller must keep it alive (level 0 holds a
 * reference in the reference too, include/cedar/level.h:25,31). */
cedar_amd_solver *cedar_amd_solver_create(int nd, len_t nx, len_t ny, len_t nz, int nstencil,
                                          const real_t *so, int own_device_so,
                                          const cedar_amd_settings *settings);
void cedar_amd_solver_destroy(cedar_amd_solver *s);
int cedar_amd_solver_nlevels(const cedar_amd_solver *s);
void cedar_amd_solver_level_dims(const cedar_amd_solver *s, int lvl, len_t *nx, len_t *ny, len_t *nz);
/* copy a level array to the host for inspection: what = "A","P","SOR0","SOR1","ABD","res", and on coarse
 * levels "x","b" (level 0 works on the caller's x and b);
 * returns the number of doubles written (0 if absent); out may be NULL to query. */
size_t cedar_amd_solver_get(const cedar_amd_solver *s, int lvl, const char *what, real_t *out);
/* replace a set-up product of a level (what = "A","P","SOR0","SOR1","ABD"; `in` host or device, the array's full size):
 * the reference's `levels` container exposes these as public members (include/cedar/level.h:14-41).  Copies the solver
 * derives from the array are rebuilt.  Returns the number of doubles taken (0: no such array). */
size_t cedar_amd_solver_set(cedar_amd_solver *s, int lvl, const char *what, const real_t *in);
/* one V-cycle, cycle->run(x,b): x,b host or device */
void cedar_amd_solver_vcycle(cedar_amd_solver *s, real_t *x, const real_t *b);
/* multilevel::solve(b,x): rel[0] = ||r0||_2, rel[i] = ||r_i||_2/||r0||_2; returns cycles run */
int cedar_amd_solver_solve(cedar_amd_solver *s, const real_t *b, real_t *x, real_t *rel);
/* timing helper for benchmarks: n V-cycles back to back on device-resident x,b; returns
 * elapsed milliseconds measured with HIP events on the library's stream */
float cedar_amd_solver_time_vcycles(cedar_amd_solver *s, real_t *x_dev, const real_t *b_dev, int n);
/* n relax sweeps on level 0 alternating DOWN/UP (the roofline microbenchmark);
 * returns elapsed milliseconds (HIP events on the library's stream) */
float cedar_amd_solver_time_relax(cedar_amd_solver *s, real_t *x_dev, const real_t *b_dev, int n);
/* n launches of one level-0 kernel of the cycle besides the sweep: op 1 = residual, 2 = restriction of the residual to
 * level 1, 3 = interpolation-and-add from level 1 (overwrites x and the residual: a timing aid, not a solver step);
 * returns elapsed milliseconds (HIP events on the library's stream) */
float cedar_amd_solver_time_op(cedar_amd_solver *s, real_t *x_dev, const real_t *b_dev, int op, int n);

/* Conjugate gradients preconditioned by the solver's multigrid cycle (BoxMG's PCG).  The numbering is BoxMG's,
 * src/{2d,3d}/ftn/BMG_PCG_parameters_f90.h:
 *   stop_test  BMG_PCG_STOP_ABS_RES_L2 = 0, BMG_PCG_STOP_REL_RES_L2 = 1 (||r||_2 absolute / relative to ||r0||_2),
 *              BMG_PCG_STOP_ABS_RES_M2 = 2, BMG_PCG_STOP_REL_RES_M2 = 3 (the M-norm sqrt(r.z), z = M^-1 r);
 *   precon     BMG_PCG_PRECON_NONE = 1, BMG_PCG_PRECON_DIAG = 2 (z = r / a_ii), BMG_PCG_PRECON_BMG = 3 (z = nmg_cycles
 *              cycles of the solver from z = 0).
 * The multigrid preconditioner must be symmetric: a V-cycle with nrelax_pre == nrelax_post (any relaxation; plane
 * relaxation also plane_nrelax_pre == plane_nrelax_post).  F-cycles, V(m,n) with m != n and periodic boundaries
 * (ibc != 0) are refused: print_error, x untouched, return -1.  Plane relaxation builds every plane solver of a level
 * from the coefficients of its last plane (as the reference does), so the preconditioner is exactly symmetric only
 * where the planes of each smoothed level share their coefficients. */
enum { CEDAR_AMD_PCG_STOP_ABS_RES_L2 = 0, CEDAR_AMD_PCG_STOP_REL_RES_L2 = 1,
       CEDAR_AMD_PCG_STOP_ABS_RES_M2 = 2, CEDAR_AMD_PCG_STOP_REL_RES_M2 = 3 };
enum { CEDAR_AMD_PCG_PRECON_NONE = 1, CEDAR_AMD_PCG_PRECON_DIAG = 2, CEDAR_AMD_PCG_PRECON_BMG = 3 };
typedef struct {
	int max_iter;     /* MAX_ITERS (50) */
	double tol;       /* STOP_TOL (1e-8) */
	int stop_test;    /* STOP_TEST (1: relative L2) */
	int precon;       /* PRECON (3: multigrid) */
	int nmg_cycles;   /* NMG_CYCLES (1) */
} cedar_amd_pcg_settings;
void cedar_amd_default_pcg_settings(cedar_amd_pcg_settings *p);
/* Solve A x = b from the x given.  hist (max_iter + 1 entries, may be NULL): hist[0] = ||r0||_2,
 * hist[i] = ||r_i||_2 / ||r0||_2 (as cedar_amd_solver_solve).  b, x host or device; p NULL = the defaults.
 * Returns the iterations run, -1 when refused.  Stops early on breakdown (p.Ap <= 0 or r.z = 0) with x finite.
 * The first call allocates five level-0 vectors that the handle keeps until cedar_amd_solver_destroy. */
int cedar_amd_solver_pcg(cedar_amd_solver *s, const real_t *b, real_t *x, const cedar_amd_pcg_settings *p, real_t *hist);
/* z = M^-1 r: one cycle of the solver from z = 0 (the preconditioner of cedar_amd_solver_pcg with nmg_cycles = 1);
 * z, r host or device.  Refused (z untouched) on the settings cedar_amd_solver_pcg refuses for precon = 3. */
void cedar_amd_solver_precondition(cedar_amd_solver *s, real_t *z, const real_t *r);
/* Flexible conjugate gradients (Golub-Ye 1999, Notay 2000, FCG(1)): cedar_amd_solver_pcg with the one change that
 * beta = z_k+1.(r_k+1 - r_k) / (r_k.z_k) = -(alpha_k (A p_k).z_k+1) / rho_k instead of r_k+1.z_k+1 / rho_k -- one more dot
 * product in the pass that reads r and z after the preconditioner, no extra vector or operator pass (DESIGN.md section
 * 14).  The two agree when M is symmetric and the flexible one does not need it, so with precon = 3 ANY cycle of the
 * handle is served: V(m,n) with m + n >= 1 (the default V(2,1) included), F-cycles, point, line and plane relaxation with
 * any plane sweep counts, handles switched by cedar_amd_solver_use_fp32_operator (the recurrence keeps the FP64
 * operator).  precon = 1 | 2 (M exactly symmetric) run cedar_amd_solver_pcg itself: its results bit for bit.
 * Same settings, hist, return value, stop tests, breakdown rules and storage as cedar_amd_solver_pcg.  Refused
 * (print_error, -1, nothing written): a NULL handle, ibc != 0 (see cedar_amd_solver_fcg_periodic), stop_test or precon
 * out of range, max_iter < 0, and with precon = 3 nmg_cycles < 1 or a cycle without any relaxation sweep. */
int cedar_amd_solver_fcg(cedar_amd_solver *s, const real_t *b, real_t *x, const cedar_amd_pcg_settings *p, real_t *hist);
/* Flexible CG on a periodic handle (ibc != 0): every configuration cedar_amd_solver_create accepts with periodic
 * boundaries -- 2D point and line relaxation, 3D point relaxation, V(m,n) with m + n >= 1, F-cycles -- with precon 1, 2, 3
 * and all four stop tests.  The periodic cycle is not a symmetric operator (its coarsest solve removes the mean, its
 * sweeps are ordered with the ghost refreshes: |<Mu,v> - <u,Mv>| / |<Mu,v>| is a few per cent even for V(1,1), DESIGN.md
 * section 19), so the standard beta is not offered with it: precon = 3 runs the flexible beta, precon = 1 | 2 (M exactly
 * symmetric) the standard one, as cedar_amd_solver_fcg does.  The operator pass wraps its own reads
 * (cedar_amd_pcg_direction_periodic); there is no ghost refresh between the Krylov passes.
 * The ghost layers of the caller's x and b do not influence the result: x gets the periodic image in its ghost layers
 * before the first residual, and carries it on return, like x after cedar_amd_solver_solve.  The operator given to
 * cedar_amd_solver_create holds the periodic image in its ghost layers, as for the cycle.
 * The operator must be definite, as for the cycle itself: a fully periodic operator with zero row sums (the pure
 * Laplacian) is singular and the coarsest factorisation fails on it here; such problems are served by
 * cedar_amd_solver_create_semidefinite and cedar_amd_solver_fcg_semidefinite below.
 * A handle with ibc = 0 forwards to cedar_amd_solver_fcg (results bit for bit, refusals its own).  Refused (print_error,
 * -1, nothing written): a NULL handle, b or x NULL, a handle of cedar_amd_solver_create_many that holds more than one
 * right-hand side, and the settings cedar_amd_solver_fcg refuses.  cedar_amd_solver_pcg, _fcg, _precondition and the
 * batch calls keep refusing ibc != 0. */
int cedar_amd_solver_fcg_periodic(cedar_amd_solver *s, const real_t *b, real_t *x, const cedar_amd_pcg_settings *p,
                                  real_t *hist);

/* Keep the 27-point operator of the cycle in single precision (3D, Dirichlet, point relaxation).  Every smoothed
 * 27-point level (all but the coarsest) with at least min_rows rows gets a row-interleaved copy of A and 1/diag rounded
 * to float (round to nearest even; rows of at most 1024 points) and releases its FP64 solve copy; the level's sweeps
 * and the cycle's residual then stream 84 instead of 136 bytes per point.  The kernels promote an entry to double when
 * they load it and do all arithmetic, and keep all vectors, in FP64: the cycle is exactly the FP64 cycle of the
 * rounded operator.  Interpolation, restriction, the coarsest solve and 7-point levels are unchanged.
 *   min_rows 0 = the default (128; CEDAR_AMD_OP32_MIN_ROWS overrides it, read at the call).
 * Returns the number of levels that now read a float copy (0 is valid; the call may be repeated and never switches a
 * level back).  Refused -- print_error, -1, handle unchanged -- for a NULL or 2D handle, ibc != 0, plane relaxation, a
 * handle of cedar_amd_solver_create_many (those take cedar_amd_solver_use_fp32_operator_many below), and when an entry
 * of A or 1/diag overflows float.
 * What the other calls do on such a handle:
 *   cedar_amd_solver_vcycle        the plain cycle of the ROUNDED operator: iterating it converges to the rounded
 *                                  operator's solution (relative error of order 6e-8 times the condition number);
 *   cedar_amd_solver_pcg, _precondition  the cycle is the preconditioner; the Krylov recurrence and its residuals use
 *                                  the FP64 operator given at creation, so the solve converges to its solution;
 *   cedar_amd_solver_solve         V-cycle handles iterate in defect-correction form, r = b - A x with the FP64
 *                                  operator, x += cycle(0, r), and report that residual; the first call allocates the
 *                                  vectors of cedar_amd_solver_pcg.  F-cycle handles start every cycle from x = 0 as
 *                                  before and report the FP64 residual;
 *   cedar_amd_solver_set           "A" / "SOR0" on a switched level rebuild its float copy (an overflow is reported
 *                                  and the level goes back to the FP64 arrays). */
int cedar_amd_solver_use_fp32_operator(cedar_amd_solver *s, int min_rows);
/* the number of levels whose cycle reads a float copy (0 before the call above, or for a NULL handle) */
int cedar_amd_solver_fp32_levels(const cedar_amd_solver *s);
/* The same switch for a handle of cedar_amd_solver_create_many (3D, Dirichlet, point relaxation): the batched sweeps and
 * the batched residual of the cycle (many3d.hip) read the float copies, so the operator bytes are both halved and paid
 * once per workgroup task for all right-hand sides.  On a handle that holds one right-hand side (max_rhs 1: made by
 * cedar_amd_solver_create, or a batch request the handle could not serve -- periodic, plane relaxation) the call forwards
 * to cedar_amd_solver_use_fp32_operator, so a caller may always use this one.
 *   Level selection, min_rows (0 = the default, 128; CEDAR_AMD_OP32_MIN_ROWS overrides it), the return value, repetition
 *   and cedar_amd_solver_fp32_levels are those of cedar_amd_solver_use_fp32_operator; every copy is built and checked
 *   before the handle changes.  Refused -- print_error, -1, handle unchanged -- for a NULL or 2D handle, ibc != 0, plane
 *   relaxation, a negative min_rows, and when an entry of A or 1/diag overflows float.
 * What the other calls do on a switched batch handle:
 *   cedar_amd_solver_vcycle_many   the plain batched cycle of the ROUNDED operator (reference order; item m has the bits
 *                                  of cedar_amd_solver_vcycle on a switched single-vector handle under CEDAR_AMD_PSUM=0);
 *   cedar_amd_solver_pcg_many      the batched cycle is the preconditioner; the recurrences and their residuals use the
 *                                  FP64 operator given at creation on every item;
 *   cedar_amd_solver_solve_many    defect correction in lockstep: r = b - A x with the FP64 operator on all items,
 *                                  z = cycle(0, r) batched on the storage of cedar_amd_solver_pcg_many (allocated by the
 *                                  first call), x += z; the norms are those of that residual.  Converged items keep
 *                                  cycling and a zero initial residual counts as converged, as on any batch handle;
 *   nrhs == 1 and every single-vector entry point (_vcycle, _solve, _pcg, _precondition, _time_*) run the single-vector
 *                                  float kernels, partial sums included, exactly as on a handle switched by
 *                                  cedar_amd_solver_use_fp32_operator;
 *   cedar_amd_solver_set           "A" / "SOR0" on a switched level rebuild its float copy, as above.
 * cedar_amd_solver_use_fp32_operator itself keeps refusing batch handles. */
int cedar_amd_solver_use_fp32_operator_many(cedar_amd_solver *s, int min_rows);
/* The switch for any 3D handle, 7-point level included.  On a batch handle it does what
 * cedar_amd_solver_use_fp32_operator_many does, on a handle with one right-hand side what
 * cedar_amd_solver_use_fp32_operator does; in both cases a 7-point level 0 (coarse levels are always 27-point) also takes
 * a float copy -- KPW, KPS, KB, the diagonal and 1/diag, row-interleaved -- which its sweeps and
 * the cycle's residual read: single vector, batch, and nrhs == 1 on a batch handle.  The reported residual, the Krylov
 * passes and interpolation's diagonal keep reading the FP64 operator, and cedar_amd_solver_solve / _solve_many go to
 * defect-correction form as described above.  Rows of any length.
 *   min_rows > 0: every smoothed level with at least min_rows rows, the 7-point level among them.
 *   min_rows 0  : the 27-point levels by their default (128 rows, CEDAR_AMD_OP32_MIN_ROWS); the 7-point level by its own
 *                 measured default, 128 rows as well (the V-cycle of gallery::poisson runs in
 *                 0.72 / 0.87 / 0.95 of its FP64 time at 512^3 / 256^3 / 128^3; smaller levels were not measured and stay
 *                 FP64 unless min_rows > 0 asks for them).
 * Copies are built and checked before the handle changes, captured graphs are dropped, the call may be repeated; returns
 * cedar_amd_solver_fp32_levels, which counts the 7-point level.  Refused -- print_error, -1, handle unchanged -- for a
 * NULL or 2D handle, ibc != 0, plane relaxation, a negative min_rows, and when an entry overflows float.
 * cedar_amd_solver_set "A" / "SOR0" on level 0 rebuild the copy (overflow: reported, the level reads FP64 again).
 * The two calls above are unchanged: on a 7-point handle they switch the 27-point levels only. */
int cedar_amd_solver_use_fp32_operator_all(cedar_amd_solver *s, int min_rows);
/* The switch for a 2D handle, single or of cedar_amd_solver_create_many: Dirichlet (ibc == 0), point relaxation, V- or
 * F-cycle.  Every smoothed level (all but the coarsest) that the call takes -- the five-point level 0 and the nine-point
 * levels alike -- gets a row-interleaved float copy of its operator and 1/diag (KW, KS, [KSW, KNW,] KO, 1/diag; DESIGN.md
 * section 16), which its sweeps (two row-class launches, band-fused, or the partial-sum sweep where the level would run
 * it in FP64, at the same run length) and the cycle's residual read; the reported residual, the Krylov passes,
 * interpolation's diagonal, restriction and the coarsest solve keep reading the FP64 operator.  The presence of a level's
 * copy alone decides what its sweeps and the cycle's residual read: a level of at most 64 x 64 unknowns that took a copy
 * runs the row kernels instead of the LDS-resident small-level kernels.
 *   min_rows > 0: every smoothed level with at least min_rows rows.
 *   min_rows 0  : the measured default, levels of at least 1024 rows (CEDAR_AMD_OP32_MIN_ROWS overrides it, read at the
 *                 call).  DESIGN.md section 16: with level 0 switched the V-cycle runs in 0.87 .. 0.93 of its FP64 time
 *                 at 4096^2, 0.87 .. 0.91 at 2048^2 and 0.94 .. 0.96 at 1024^2 (nine- and five-point, V(1,1) and
 *                 V(2,1)); at 512^2 the two are equal within the spread, so smaller levels stay FP64 unless min_rows > 0
 *                 asks for them.
 * Copies are built and checked before the handle changes, captured graphs are dropped, the call may be repeated and never
 * switches a level back; returns cedar_amd_solver_fp32_levels.  Refused -- print_error, -1, handle unchanged -- for a NULL
 * handle, a 3D handle (use cedar_amd_solver_use_fp32_operator_all), ibc != 0, line relaxation, a negative min_rows, an
 * entry of A or 1/diag that overflows float, and out of device memory.  The other calls behave as on a switched 3D
 * handle (above): _vcycle / _vcycle_many run the cycle of the rounded operator, _pcg / _fcg / _pcg_many / _fcg_many /
 * _precondition precondition with it and run the recurrence on the FP64 operator, _solve / _solve_many go to
 * defect-correction form, an F-cycle handle's _solve starts each cycle from x = 0 and reports the FP64 residual, and
 * cedar_amd_solver_set "A" / "SOR0" on a switched level rebuild its copy (overflow: reported, the level reads FP64 again).
 * The three calls above keep refusing 2D handles. */
int cedar_amd_solver_use_fp32_operator_2d(cedar_amd_solver *s, int min_rows);
/* The switch for a 2D handle with line relaxation (line-x, line-y or line-xy), single or of cedar_amd_solver_create_many:
 * Dirichlet (ibc == 0), V- or F-cycle.  A smoothed level (all but the coarsest) that the call takes keeps, beside its
 * FP64 arrays:
 *   - a row-interleaved float copy of its operator (KW, KS, [KSW, KNW,] KO and a slot-row of zeros where a point-relaxed
 *     level keeps 1/diag), which the x-line right-hand sides and the cycle's residual read;
 *   - where it runs y lines, the same form of the transposed operator planes;
 *   - its line factors as floats in the form the FP64 kernel of that direction reads: the scan-ordered copy where the
 *     level keeps one (lines of more than 512 unknowns), else the plain image of the two SOR planes.
 * All values are the FP64 ones rounded to nearest even; the factors are those of the unrounded operator.  Every sweep has
 * the bits of the FP64 line kernel on the rounded operator and factors.  The reported residual, the Krylov passes,
 * interpolation's diagonal, restriction and the coarsest solve keep reading the FP64 operator.  Levels that the
 * LDS-resident small-level kernels serve (at most 64 x 64 unknowns) always stay FP64 and are never counted.
 *   min_rows > 0: every smoothed level with at least min_rows rows that is not such a small level.
 *   min_rows 0  : the measured default, levels of at least 1024 rows (CEDAR_AMD_OP32_MIN_ROWS overrides it, read at the
 *                 call).  DESIGN.md section 17, profiles/op32_lines_time.json: with level 0 switched the line-xy V-cycle
 *                 runs in 0.85 .. 0.93 of its FP64 time at 8192^2 (V(2,1) nine-point, the benchmark's third configuration:
 *                 15.6 -> 13.3 ms) and 4096^2, 0.91 .. 0.96 at 2048^2, 0.92 .. 0.96 at 1024^2 (nine- and five-point,
 *                 V(1,1) and V(2,1)); a level-0 x sweep alone in 0.69 .. 0.85, where the byte model says 0.65 (nine-point)
 *                 and 0.78 (five-point).  At 512^2 the two are equal within 1 %, so smaller levels stay FP64 unless
 *                 min_rows > 0 asks for them.
 * The copies take about 72 bytes per unknown of a nine-point line-xy level (5 GB at 8192^2).
 * Copies are built and checked before the handle changes, captured graphs are dropped, the call may be repeated and never
 * switches a level back; returns cedar_amd_solver_fp32_levels.  Refused -- print_error, -1, handle unchanged -- for a NULL
 * handle, a 3D handle, point relaxation (use cedar_amd_solver_use_fp32_operator_2d), ibc != 0, y lines that do not keep
 * transposed arrays (CEDAR_AMD_YLINES_TRANSPOSED=0), a negative min_rows, an entry of A or of a factor that overflows
 * float, and out of device memory.  The other calls behave as on a handle switched by the _2d call: _vcycle /
 * _vcycle_many run the cycle that reads the rounded arrays, _pcg / _fcg / _pcg_many / _fcg_many / _precondition
 * precondition with that cycle and run their recurrence on the FP64 operator, _solve / _solve_many go to
 * defect-correction form, an F-cycle handle's _solve starts each cycle from x = 0 and reports the FP64 residual.
 * cedar_amd_solver_set on a switched level: "A" rebuilds both operator copies, "SOR0" / "SOR1" the factor copies they
 * feed (overflow: reported, the level drops its float copies and reads FP64 again).  The four calls above are unchanged
 * and keep refusing what they refuse. */
int cedar_amd_solver_use_fp32_operator_lines(cedar_amd_solver *s, int min_rows);
/* Single-precision interpolation weights for the cycle's grid transfers (transferf.hip): 2D and 3D,
 * 5/9/7/27-point, Dirichlet (ibc == 0), point relaxation in 3D, point and line relaxation in 2D, V- and F-cycles, handles
 * of cedar_amd_solver_create and _create_many.  For every pair (fine level L, coarse level K) whose fine level has at least
 * min_rows rows, K keeps a float copy of its weights K.P (rounded to nearest even; slot planes, every coarse row on a
 * 128-byte line), and the cycle's restriction and interpolation-and-add between the two read it: each has the bits of the
 * FP64 kernel on the rounded weights.  K.P stays FP64 and unrounded (cedar_amd_solver_get "P" returns it as before), and
 * the diagonal that interpolation-and-add divides by stays the FP64 one.  A 2D pair whose fine level the LDS-resident
 * small-level kernels serve (they fuse the transfers) keeps FP64 weights and is not counted; the copy never moves a level
 * off that path.
 * The weights enter a cycle through the coarse-grid correction only, never through the residual, and R = P^T uses the
 * same rounded weights.  So cedar_amd_solver_solve / _solve_many stay plain iterations of the cycle and converge to the
 * solution of the operator given (no defect-correction form), the preconditioner stays symmetric and _pcg serves it;
 * _vcycle / _vcycle_many run the cycle with the rounded weights; _pcg / _fcg, their _many forms and _precondition use it
 * as the preconditioner, their Krylov passes are untouched.
 * The switch is independent of the five operator switches above: it may be called before or after any of them, and each
 * keeps its own count (cedar_amd_solver_fp32_levels does not count weights, cedar_amd_solver_fp32_interp_levels does not
 * count operators).
 *   min_rows > 0: every pair whose fine level has at least min_rows rows.
 *   min_rows 0  : the default, fine levels of at least 128 rows in 3D and 1024 rows in 2D (CEDAR_AMD_CI32_MIN_ROWS overrides
 *                 it, read at the call); DESIGN.md section 18 and profiles/ci32_time.json hold what it rests on.
 * Copies are built and checked before the handle changes, captured graphs are dropped, the call may be repeated and never
 * switches a pair back; returns the number of level pairs that read a float copy (0 is valid), which
 * cedar_amd_solver_fp32_interp_levels reports too.  Refused -- print_error, -1, handle unchanged -- for a NULL handle,
 * ibc != 0, 3D plane relaxation, a negative min_rows, a weight that is finite in FP64 and not in float, and out of device
 * memory.  cedar_amd_solver_set "P" on a switched level rebuilds its copy (overflow: reported, the level's transfers read
 * the FP64 weights again). */
int cedar_amd_solver_use_fp32_interpolation(cedar_amd_solver *s, int min_rows);
int cedar_amd_solver_fp32_interp_levels(const cedar_amd_solver *s);
/* The transfer kernels on a float copy of the weights built for the call (for tests): the arguments of
 * BMG2_/BMG3_SymStd_restrict, _interp_add (Dirichlet: no boundary code), cedar_amd_restrict3_many and
 * cedar_amd_interp_add3_many; every result has the bits of that entry point on the weights rounded to float.  0 when
 * served; non-zero, with nothing written, when refused (a NULL array, an extent below 3, a weight that overflows float). */
int cedar_amd_restrict2_ci32(real_t *q, real_t *qc, real_t *ci, int ii, int jj, int iic, int jjc);
int cedar_amd_interp_add2_ci32(real_t *q, real_t *qc, real_t *res, real_t *so, real_t *ci, len_t iic, len_t jjc, len_t ii,
                               len_t jj, int nstncl);
int cedar_amd_restrict3_ci32(real_t *q, real_t *qc, real_t *ci, len_t ii, len_t jj, len_t kk, len_t iic, len_t jjc, len_t kkc);
int cedar_amd_interp_add3_ci32(real_t *q, real_t *qc, real_t *so, real_t *res, real_t *ci, len_t iic, len_t jjc, len_t kkc,
                               len_t ii, len_t jj, len_t kk, int nstncl);
int cedar_amd_restrict3_many_ci32(int nrhs, real_t *q, real_t *qc, real_t *ci, len_t ii, len_t jj, len_t kk, len_t iic,
                                  len_t jjc, len_t kkc);
int cedar_amd_interp_add3_many_ci32(int nrhs, real_t *q, real_t *qc, real_t *so, real_t *res, real_t *ci, len_t iic, len_t jjc,
                                    len_t kkc, len_t iif, len_t jjf, len_t kkf, int nstncl);

/* Several right-hand sides at once on one resident hierarchy.  The operator, 1/diag and the interpolation weights are
 * the same for every right-hand side, so the batched 3D kernels (many3d.hip) fetch them once per workgroup task and apply
 * them to all items from registers; the 2D kernels take the item from the launch grid.
 * Storage: the vectors of a batch are stored item-major, back to back: item m of a level-0 vector starts at
 * m * (nx+2)(ny+2)(nz+2) doubles (2D: (nx+2)(ny+2)).  Host or device pointers.
 * Exactness: the batched kernels keep the reference's term order on every level, so item m of any batched result has the
 * bits of the single-vector reference-order computation on item m alone (what cedar_amd_solver_vcycle / _solve give
 * where no level takes the partial-sum sweep, i.e. no 27-point level of 160 rows or more, or under CEDAR_AMD_PSUM=0).
 *  - A handle made with max_rhs > 1 still serves every single-vector entry point (_solve, _vcycle, _pcg, _precondition,
 *    _get, _set, _time_*) on item 0, unchanged: those calls run the single-vector kernels.
 *  - Supported: 3D 7- and 27-point and 2D 5- and 9-point, Dirichlet (ibc == 0), V-cycle; 3D point relaxation; 2D point
 *    and line relaxation.  The _many calls are refused (print_error, return -1, nothing written) for nrhs < 1,
 *    nrhs > max_rhs, ibc != 0, an F-cycle and 3D plane relaxation; such a handle reports max_rhs 1.
 *  - Items nrhs .. max_rhs-1 are not touched (the solver's own level vectors of the unused items may hold anything).
 *  - Conjugate gradients on a batch: cedar_amd_solver_pcg_many below.
 *  - Not offered: the domain-decomposed solvers, the bmg2_/bmg3_ C interface. */
enum { CEDAR_AMD_MAX_RHS = 32 };
/* as cedar_amd_solver_create, with room for max_rhs right-hand sides (1 .. 32) on every level; max_rhs outside that range:
 * print_error, NULL */
cedar_amd_solver *cedar_amd_solver_create_many(int nd, len_t nx, len_t ny, len_t nz, int nstencil,
                                               const real_t *so, int own_device_so,
                                               const cedar_amd_settings *settings, int max_rhs);
int cedar_amd_solver_max_rhs(const cedar_amd_solver *s); /* 1 for cedar_amd_solver_create */
/* one cycle on each of the first nrhs items; 0, or -1 when refused (nothing written) */
int cedar_amd_solver_vcycle_many(cedar_amd_solver *s, int nrhs, real_t *x, const real_t *b);
/* multilevel::solve for nrhs right-hand sides in lockstep.
 * rel: nrhs rows of max_iter+1 entries, row m as cedar_amd_solver_solve writes it for item m;
 * iters[m]: cycles after which item m first met tol (max_iter if it never did); may be NULL.
 * All items are cycled until every one has met tol or max_iter is reached: an item that met tol early keeps being cycled
 * and its rel row keeps being written; entries of rel beyond the cycles run are not touched.  An item whose initial
 * residual norm is exactly 0 counts as converged from the start (iters[m] = 0, its rel row is 0, 0, ... for the cycles
 * run), so that one zero column does not hold the batch for max_iter cycles: the one deliberate difference from calling
 * cedar_amd_solver_solve per item, which would record 0/0.  Returns the cycles run, -1 when refused. */
int cedar_amd_solver_solve_many(cedar_amd_solver *s, int nrhs, const real_t *b, real_t *x, real_t *rel, int *iters);
/* timing aid next to cedar_amd_solver_time_vcycles: n cycles on nrhs device-resident items, HIP-event ms (-1: refused) */
float cedar_amd_solver_time_vcycles_many(cedar_amd_solver *s, int nrhs, real_t *x_dev, const real_t *b_dev, int n);
/* cedar_amd_solver_pcg on the first nrhs items of b, x (item-major) in lockstep on a handle made with
 * cedar_amd_solver_create_many: nrhs independent CG recurrences that share the operator fetches of every pass (krylov.hip
 * *_many) and the batched cycle as preconditioner -- not a block CG, the items share no search space.
 * hist: nrhs rows of p->max_iter + 1 entries (may be NULL), row m as cedar_amd_solver_pcg writes it for item m; iters[m]
 * (may be NULL): the value that call would return for item m.  Returns the largest iters[m], -1 when refused.
 *  - An item is frozen when it meets the stop test, breaks down, or starts with r0 == 0, r0.z0 <= 0 or converged: from
 *    then on its x, its hist row beyond iters[m] and iters[m] are exactly what the single call leaves, and the loop ends
 *    when no item is active or max_iter is reached.  This differs from cedar_amd_solver_solve_many, which keeps cycling
 *    converged items: a CG item that goes on after convergence runs into rho -> 0 and the breakdown branch, and x equal
 *    to the single call's bit for bit is worth more.  Frozen items still ride through the batched preconditioner cycle
 *    (the cycle has no item mask; their z is not used): the known cost of lockstep.
 *  - Bits: item m's x, hist row and iters[m] equal those of cedar_amd_solver_pcg on item m alone on a single-vector handle
 *    in reference order (the default path where no 27-point level has 160 rows or more, CEDAR_AMD_PSUM=0 otherwise).
 *    nrhs == 1 runs the single-vector path itself (partial-sum sweeps included) and equals cedar_amd_solver_pcg on any handle.
 *  - Storage: five level-0 vectors per item plus slabs and scalar blocks for max_rhs items, allocated on the first call
 *    and kept until cedar_amd_solver_destroy; cedar_amd_solver_pcg on the same handle works on item 0's set.
 *  - Refused (print_error, -1, x / hist / iters untouched, the handle stays usable), decided before any allocation or
 *    launch: whatever the other _many calls refuse and whatever cedar_amd_solver_pcg refuses.  Served: every precon and
 *    stop_test; 3D 7- and 27-point with point relaxation, 2D 5- and 9-point with point and line relaxation.
 *  - Out of scope: the domain-decomposed drivers, periodic boundaries, F-cycles, 3D plane relaxation, the bmg2_/bmg3_ C
 *    interface, a true block CG. */
int cedar_amd_solver_pcg_many(cedar_amd_solver *s, int nrhs, const real_t *b, real_t *x,
                              const cedar_amd_pcg_settings *p, real_t *hist, int *iters);
/* the batched passes one by one on caller arrays, as cedar_amd_pcg_direction / _update do for one vector (no rank-grid
 * `partial`): vectors hold at least nrhs items back to back, the operator (and diag) is shared; sc = nrhs blocks of
 * CEDAR_AMD_PCG_NSC doubles, item m reads beta / alpha from and writes its scalars to block m; slabs NaN-filled before the
 * launch.  `active`: bit m clear = item m is skipped, its outputs and its block stay as given.  Item m's vectors and
 * scalars have the bits the single-vector call gives on item m alone.  0, or -1 (print_error, nothing done) for nrhs
 * outside 1 .. 32 or arguments the single-vector calls refuse. */
int cedar_amd_pcg_direction_many(int nrhs, unsigned active, const real_t *so, const real_t *z, const real_t *p,
                                 real_t *pn, real_t *w, len_t ii, len_t jj, len_t kk, int nstncl, int first, real_t *sc);
int cedar_amd_pcg_update_many(int nrhs, unsigned active, int zmode, int move, real_t *x, real_t *r, const real_t *p,
                              const real_t *w, real_t *z, const real_t *diag, len_t ii, len_t jj, len_t kk, int first,
                              real_t *sc);
/* cedar_amd_solver_fcg on the first nrhs items in lockstep: the contract of cedar_amd_solver_pcg_many (hist rows, iters,
 * freezing of items, storage, bits: item m equals cedar_amd_solver_fcg on item m alone in reference order; nrhs == 1 runs
 * the single-vector path) with the flexible beta.  Refused: whatever the other _many calls refuse (F-cycles and 3D plane
 * relaxation among it) and whatever cedar_amd_solver_fcg refuses. */
int cedar_amd_solver_fcg_many(cedar_amd_solver *s, int nrhs, const real_t *b, real_t *x,
                              const cedar_amd_pcg_settings *p, real_t *hist, int *iters);
/* cedar_amd_pcg_dots_wz on nrhs items (r, z, w item-major, sc = nrhs blocks): item m's five scalars have the bits of the
 * single call on item m; bit m of `active` clear = item m's block stays as given */
int cedar_amd_pcg_dots_wz_many(int nrhs, unsigned active, const real_t *r, const real_t *z, const real_t *w, len_t ii,
                               len_t jj, len_t kk, int first, real_t *sc);
/* The batched 3D kernels one by one on caller arrays (host or device; vectors hold nrhs items back to back, operator
 * arrays are shared); argument order of the BMG3_SymStd_* drop-ins, nstncl = 4|14, Dirichlet.  interp_add3 keeps the
 * reference's side effect (res /= so(kp)) per item.  0, or -1 (print_error, nothing done) for nrhs outside 1 .. 32, an
 * nstncl they do not serve or a NULL array. */
int cedar_amd_relax3_gs_many(int nrhs, real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, len_t kk, int nstncl,
                             int updown);
int cedar_amd_residual3_many(int nrhs, real_t *so, real_t *qf, real_t *q, real_t *res, len_t ii, len_t jj, len_t kk, int nstncl);
/* The batched 27-point sweep / residual with the operator and 1/diag rounded to single precision (what a level of a batch
 * handle runs after cedar_amd_solver_use_fp32_operator_many): the contract of cedar_amd_relax3_gs_op32 /
 * cedar_amd_residual3_op32 on nrhs items back to back.  The float copy is built for the call; always the reference order
 * (the batch has no partial sums), so item m has the bits of cedar_amd_relax3_gs_op32(frun = 0) / cedar_amd_residual3_op32
 * on item m alone, and of cedar_amd_relax3_gs_many / cedar_amd_residual3_many on the rounded arrays.  0, or -1 (print_error,
 * q / res untouched) for nrhs outside 1 .. 32, a NULL array, rows longer than 1024 points, or an entry of so or 1/diag
 * that overflows float. */
int cedar_amd_relax3_gs_many_op32(int nrhs, real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, len_t kk,
                                  int updown);
int cedar_amd_residual3_many_op32(int nrhs, real_t *so, real_t *qf, real_t *q, real_t *res, len_t ii, len_t jj, len_t kk);
/* The 7-point pair on a batch (what the 7-point level of a batch handle runs after
 * cedar_amd_solver_use_fp32_operator_all): cedar_amd_relax7_gs_op32 / cedar_amd_residual7_op32 on nrhs items stored back
 * to back; a point's coefficients are fetched from the float copy once and applied to every item, so item m has the bits
 * of the single call on item m alone, and of cedar_amd_relax3_gs_many / cedar_amd_residual3_many on the rounded arrays.
 * Returns 0; nrhs outside 1 .. 32, a NULL array or an entry that overflows float: print_error, -1, q / res untouched. */
int cedar_amd_relax7_gs_many_op32(int nrhs, real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, len_t kk,
                                  int updown);
int cedar_amd_residual7_many_op32(int nrhs, real_t *so, real_t *qf, real_t *q, real_t *res, len_t ii, len_t jj, len_t kk);
int cedar_amd_restrict3_many(int nrhs, real_t *q, real_t *qc, real_t *ci, len_t ii, len_t jj, len_t kk, len_t iic, len_t jjc,
                             len_t kkc);
int cedar_amd_interp_add3_many(int nrhs, real_t *q, real_t *qc, real_t *so, real_t *res, real_t *ci, len_t iic, len_t jjc,
                               len_t kkc, len_t iif, len_t jjf, len_t kkf, int nstncl);

/* Several right-hand sides at once on a PERIODIC 3D handle (periodic_many3d.hip, krylov.hip *_per_many).
 * cedar_amd_solver_create_many_periodic is cedar_amd_solver_create_many for a periodic 3D handle: every level, the
 * coarsest right-hand-side workspace and later the Krylov storage have room for max_rhs items, and
 * cedar_amd_solver_max_rhs reports max_rhs.  cedar_amd_solver_create_many itself is unchanged: a periodic handle asked for
 * through it still holds one item, and the _many calls keep refusing it.
 *  - Served: 3D, ibc 1..3 and 5..8, 7- and 27-point, point relaxation, V(m,n), max_rhs 1 .. 32.  On such a handle
 *    cedar_amd_solver_vcycle_many, _solve_many and _time_vcycles_many work with the contracts they have above; every item's
 *    x comes back with the periodic image in its ghost layers.  Every single-vector entry point (_solve, _vcycle, _get,
 *    _set, _time_*) still works on item 0 with the single-vector kernels, unchanged.
 *  - Forwarded: ibc == 0 goes to cedar_amd_solver_create_many; cedar_amd_solver_fcg_periodic_many on a Dirichlet batch
 *    handle goes to cedar_amd_solver_fcg_many; the kernel-level calls below with ibc = 0 go to their Dirichlet _many twin.
 *  - Refused by the creation call (print_error, NULL): nd == 2 with ibc != 0, an F-cycle, plane (any non-point)
 *    relaxation, max_rhs outside 1 .. 32, and everything cedar_amd_solver_create refuses for a periodic handle (a boundary
 *    code 3D does not define, an odd periodic extent on a coarsened level, more than 2048 coarsest unknowns).
 *  - Refused on the handle (print_error, -1, nothing written): nrhs < 1 or nrhs > max_rhs; cedar_amd_solver_pcg_many and
 *    cedar_amd_solver_fcg_many (periodic boundaries, as before); cedar_amd_solver_fcg_periodic when max_rhs > 1 (use
 *    cedar_amd_solver_fcg_periodic_many with nrhs == 1); the single-precision switches.
 *  - Bits: item m of every result -- x, rel rows, iters -- has the bits of the single-vector periodic call on item m alone
 *    on a handle of cedar_amd_solver_create with the same settings.  The single-vector periodic path has no partial-sum
 *    sweep, so this holds at every size with no environment switch.
 *  - Out of scope: 2D periodic batches, periodic F-cycles on a batch, singular fully periodic operators (those take
 *    cedar_amd_solver_create_semidefinite with max_rhs > 1), the rank-grid
 *    solvers. */
cedar_amd_solver *cedar_amd_solver_create_many_periodic(int nd, len_t nx, len_t ny, len_t nz, int nstencil,
                                                        const real_t *so, int own_device_so,
                                                        const cedar_amd_settings *settings, int max_rhs);
/* cedar_amd_solver_fcg_periodic on the first nrhs items in lockstep, with the contract of cedar_amd_solver_fcg_many (hist
 * rows, iters, freezing of stopped or broken-down items, storage for max_rhs items): flexible beta with precon 3, the
 * standard recurrence with precon 1 / 2, all four stop tests; every item's x is wrapped before the first residual and on
 * return, the ghosts of b are never read.  Item m's x, hist row and iters[m] equal those of cedar_amd_solver_fcg_periodic
 * on item m alone, bit for bit; nrhs == 1 runs the single-vector path itself.  A Dirichlet batch handle is forwarded to
 * cedar_amd_solver_fcg_many; a periodic handle not made by cedar_amd_solver_create_many_periodic is refused as the other
 * _many calls refuse it. */
int cedar_amd_solver_fcg_periodic_many(cedar_amd_solver *s, int nrhs, const real_t *b, real_t *x,
                                       const cedar_amd_pcg_settings *p, real_t *hist, int *iters);
/* The batched periodic 3D kernels one by one on caller arrays (host or device; nrhs items back to back, operator arrays
 * shared; argument order of the Dirichlet _many calls, then the boundary code).  Item m has the bits of the single-vector
 * periodic drop-in (BMG3_SymStd_relax_GS / _restrict / _interp_add / _SOLVE_cg, cedar_amd_pcg_direction_periodic) on item
 * m alone.  0, or -1 (print_error, nothing written) for nrhs outside 1 .. 32, a NULL array, an nstncl other than 4 | 14 or
 * a boundary code 3D does not define.  ibc = 0 forwards to the Dirichlet _many call (cedar_amd_solve_cg3_periodic_many has
 * none and refuses it).
 *  - relax3_gs: ghosts_consistent != 0 tells the sweep that the y ghost rows of q hold the periodic image on entry (the
 *    row-class path needs it when y is periodic); 0 is always correct.
 *  - restrict3 refreshes the ghosts of the nrhs fine vectors first (q is written); interp_add3 keeps res /= so(kp).
 *  - solve_cg3: abd = the dense factor of BMG3_SymStd_SETUP_cg_LU with the same code (shared), bbd = nrhs segments of
 *    (ii-2)(jj-2)(kk-2) doubles; one workgroup per item.
 *  - pcg_direction: as cedar_amd_pcg_direction_many, reads wrapped; a masked item is neither read nor written. */
int cedar_amd_relax3_gs_periodic_many(int nrhs, real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, len_t kk,
                                      int nstncl, int updown, int ibc, int ghosts_consistent);
int cedar_amd_restrict3_periodic_many(int nrhs, real_t *q, real_t *qc, real_t *ci, len_t ii, len_t jj, len_t kk, len_t iic,
                                      len_t jjc, len_t kkc, int ibc);
int cedar_amd_interp_add3_periodic_many(int nrhs, real_t *q, real_t *qc, real_t *so, real_t *res, real_t *ci, len_t iic,
                                        len_t jjc, len_t kkc, len_t iif, len_t jjf, len_t kkf, int nstncl, int ibc);
int cedar_amd_solve_cg3_periodic_many(int nrhs, real_t *q, real_t *qf, len_t ii, len_t jj, len_t kk, real_t *abd, real_t *bbd,
                                      len_t nabd1, int ibc);
int cedar_amd_pcg_direction_periodic_many(int nrhs, unsigned active, const real_t *so, const real_t *z, const real_t *p,
                                          real_t *pn, real_t *w, len_t ii, len_t jj, len_t kk, int nstncl, int ibc, int first,
                                          real_t *sc);

/* Several right-hand sides at once on a PERIODIC 2D handle (periodic_many2d.hip, krylov.hip pcg_dir2_per_many): the 2D
 * case the block above leaves out is served by a call of its own, cedar_amd_solver_create_many_periodic2.  It is
 * cedar_amd_solver_create_many for a periodic 2D handle: every level, the coarsest right-hand-side workspace and later the
 * Krylov storage have room for max_rhs items, and cedar_amd_solver_max_rhs reports max_rhs.  cedar_amd_solver_create_many
 * and cedar_amd_solver_create_many_periodic are unchanged: a periodic 2D handle asked for through the first still holds one
 * item and the _many calls keep refusing it, the second keeps refusing nd == 2.
 *  - Served: 2D, ibc 1..3, 5- and 9-point, V(m,n), max_rhs 1 .. 32; point relaxation (rows up to the 8190 points the
 *    single-vector handle serves) and line-x, line-y, line-xy relaxation.  On such a handle cedar_amd_solver_vcycle_many,
 *    _solve_many and _time_vcycles_many work with the contracts they have above, and cedar_amd_solver_fcg_periodic_many
 *    runs flexible CG on the items in lockstep (all nrhs items of x are wrapped before the first residual and on return,
 *    the ghosts of b are never read, nrhs == 1 runs the single-vector path itself).  Every single-vector entry point
 *    (_solve, _vcycle, _get, _set, _time_*) still works on item 0 with exactly the launches it takes on a handle of
 *    cedar_amd_solver_create.
 *  - How a batch runs: the point sweep, the transfers, the coarsest solve, the x-line sweep and every Krylov pass take all
 *    items in one launch; the point sweep and the direction pass fetch the operator once per task and apply it to every
 *    item.  Periodic y-lines stay on the gather / solve / scatter pipeline, which the items walk one after the other (a
 *    batched periodic y-line pipeline is out of scope).
 *  - Forwarded: ibc == 0 goes to cedar_amd_solver_create_many(2, ...); cedar_amd_solver_fcg_periodic_many on a Dirichlet
 *    batch handle goes to cedar_amd_solver_fcg_many.
 *  - Refused by the creation call (print_error, NULL, the message names cedar_amd_solver_create_many_periodic2): an
 *    F-cycle, max_rhs outside 1 .. 32, a boundary code 2D does not define, and everything cedar_amd_solver_create refuses
 *    for a periodic 2D handle (point relaxation with rows longer than 8190 points): its message first, then a line that
 *    names this call.
 *  - Refused on the handle (print_error, -1, nothing written): nrhs < 1 or nrhs > max_rhs; cedar_amd_solver_pcg_many and
 *    cedar_amd_solver_fcg_many (periodic boundaries, as before); cedar_amd_solver_fcg_periodic when max_rhs > 1 (use
 *    cedar_amd_solver_fcg_periodic_many with nrhs == 1); every single-precision switch.
 *  - Bits: item m of every result -- x, rel / hist rows, iters -- has the bits of the single-vector periodic call on item m
 *    alone on a handle of cedar_amd_solver_create with the same settings.  The 2D periodic single-vector path has no
 *    partial-sum sweep and no float view, so this holds at every size with no environment switch.
 *  - Out of scope: periodic F-cycles on a batch, a batched periodic y-line pipeline, the single-precision switches on
 *    periodic handles, singular fully periodic operators (cedar_amd_solver_create_semidefinite serves them), the
 *    rank-grid solvers. */
cedar_amd_solver *cedar_amd_solver_create_many_periodic2(len_t nx, len_t ny, int nstencil, const real_t *so,
                                                         int own_device_so, const cedar_amd_settings *settings, int max_rhs);
/* The batched periodic 2D kernels one at a time on caller arrays (host or device; the nrhs items lie back to back with
 * stride ii*jj, the operator arrays are shared; argument order of the single-vector 2D calls, then the boundary code).
 * Item m has the bits of the single-vector periodic drop-in (BMG2_SymStd_relax_GS / _restrict / _interp_add / _SOLVE_cg,
 * cedar_amd_pcg_direction_periodic) on item m alone.  0, or -1 (print_error, nothing written) for nrhs outside 1 .. 32, a
 * NULL array, an nstncl other than 3 | 5 or ibc outside 0 .. 3.  ibc = 0: cedar_amd_pcg_direction2_periodic_many forwards
 * to cedar_amd_pcg_direction_many, its Dirichlet batched twin; relax2_gs, restrict2, interp_add2 and solve_cg2 have no
 * Dirichlet batched kernel-level call to go to and refuse it.
 *  - relax2_gs: nstncl 3 = the five-point sweep, 5 = the nine-point one; updown as BMG2_SymStd_relax_GS; rows of more than
 *    8192 points (ghosts included) are refused.  Up to 512 interior points one workgroup per grid row serves all items;
 *    longer rows take one launch per i-colour with a lane per point.  Either way a lane keeps the coefficients of its
 *    points in registers across the items.
 *  - restrict2 refreshes the ghosts of the nrhs fine vectors first (q is written) under the single call's conditions;
 *    interp_add2 keeps its side effect on res per item and wraps every item's q.
 *  - solve_cg2: abd = the dense factor of BMG2_SymStd_SETUP_cg_LU with the same code (shared), nabd1 >= (ii-2)(jj-2);
 *    bbd = nrhs segments of (ii-2)(jj-2) doubles; one lane per item.
 *  - pcg_direction2: as cedar_amd_pcg_direction_many on a 2D level, reads wrapped; a masked item is neither read nor
 *    written.  cedar_amd_pcg_direction_periodic_many keeps refusing nstncl 3 | 5. */
int cedar_amd_relax2_gs_periodic_many(int nrhs, real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, int nstncl,
                                      int updown, int ibc);
int cedar_amd_restrict2_periodic_many(int nrhs, real_t *q, real_t *qc, real_t *ci, len_t ii, len_t jj, len_t iic, len_t jjc,
                                      int ibc);
int cedar_amd_interp_add2_periodic_many(int nrhs, real_t *q, real_t *qc, real_t *res, real_t *so, real_t *ci, len_t iic,
                                        len_t jjc, len_t ii, len_t jj, int nstncl, int ibc);
int cedar_amd_solve_cg2_periodic_many(int nrhs, real_t *q, real_t *qf, len_t ii, len_t jj, real_t *abd, real_t *bbd,
                                      len_t nabd1, int ibc);
int cedar_amd_pcg_direction2_periodic_many(int nrhs, unsigned active, const real_t *so, const real_t *z, const real_t *p,
                                           real_t *pn, real_t *w, len_t ii, len_t jj, int nstncl, int ibc, int first,
                                           real_t *sc);

/* Singular problems: a symmetric positive SEMIdefinite operator whose null space is the constants -- the pressure or
 * potential Poisson equation with pure Neumann or fully periodic boundaries, zero row sums.
 *  - Requested by this creation call, not by a boundary code: settings->ibc keeps its meaning (0: no periodic direction,
 *    for example pure Neumann; 1 .. 3 in 2D; 1 .. 3 and 5 .. 8 in 3D) and codes below zero stay refused everywhere.  The
 *    reference's negative codes BMG_BCs_indef_* change exactly two rules, and a semidefinite handle applies those two:
 *    the coarsest matrix is assembled as always and the diagonal entry of its LAST unknown is doubled before the
 *    factorisation (BMG3_SymStd_SETUP_cg_LU.f90:143-145, 179-181, 590-593 and the 2D file likewise), and every coarsest
 *    solve removes the mean of its solution over the interior, for ibc == 0 too (BMG3_SymStd_SOLVE_cg.f90:150-172; one lane
 *    sums sequentially, i fastest, then j, then k).  Sweeps, transfers, the Galerkin product, line factors and ghost
 *    refreshes are those of ibc.  On a residual with zero sum this coarse solve is exact.
 *  - Served: max_rhs == 1: everything cedar_amd_solver_create accepts for that ibc except 3D plane relaxation -- 2D point
 *    and line relaxation, 3D point relaxation, V(m,n), F-cycles, any num_levels.  max_rhs > 1: what the batch creation
 *    call for that nd and ibc serves (cedar_amd_solver_create_many, _create_many_periodic, _create_many_periodic2),
 *    V-cycles only.
 *  - The operator: zero row sums, checked before any set-up -- max_i |(A 1)_i| <= 1024 eps max_i |a_ii| on level 0, the
 *    vector of ones wrapped in the periodic directions and zero in the other ghosts.  A periodic operator must hold the
 *    periodic image in ALL its ghost cells, the corners (and in 3D the edges) included: the periodic interpolation set-up
 *    reads them.
 *  - Refused (print_error, NULL, the message names cedar_amd_solver_create_semidefinite): whatever the corresponding
 *    creation call refuses (its message first), ibc < 0, plane relaxation (it diverged on a semidefinite 27-point
 *    operator when tried with the reference's rules; not served), max_rhs outside 1 .. 32, an F-cycle with max_rhs > 1, an
 *    operator whose null space is not the constants.
 *  - On such a handle cedar_amd_solver_vcycle, _solve, _vcycle_many, _solve_many, _get, _nlevels and _level_dims work
 *    unchanged and run the semidefinite cycle.  cedar_amd_solver_solve needs a COMPATIBLE b (zero sum over the interior)
 *    and does not project; its iterate's mean is whatever the cycles leave.  cedar_amd_solver_pcg, _fcg, _fcg_periodic,
 *    their _many forms, _precondition and every use_fp32_* switch refuse it (print_error, -1, nothing written; the message
 *    names cedar_amd_solver_fcg_semidefinite).
 *  - Not offered: the bmg2_ / bmg3_ C interface, the rank-grid (domain-decomposed) solvers, the BMG*_SymStd_* drop-ins
 *    (they keep refusing negative codes). */
cedar_amd_solver *cedar_amd_solver_create_semidefinite(int nd, len_t nx, len_t ny, len_t nz, int nstencil,
                                                       const real_t *so, int own_device_so,
                                                       const cedar_amd_settings *settings, int max_rhs);
/* Flexible CG on a semidefinite handle: solves A x = P b with mean(x) = 0, where P v = v - mean_interior(v) 1.  The
 * rules of cedar_amd_solver_fcg_periodic / _fcg_periodic_many carry over: settings, hist layout, return value, stop tests,
 * breakdown rules, host or device storage; precon = 3 takes the flexible beta, precon = 1 | 2 the standard one.  The
 * direction pass follows ibc: the Dirichlet forms for 0, the wrap-around forms otherwise, single or batched.
 * Projections: r0 = b - A x0 is replaced by P r0 (b itself is not written and need not be
 * compatible; hist[0] = |P (b - A x0)|_2), and x by P x before it is returned (an item that froze early gets it once, at
 * the end).  In between the iterate's constant part drifts freely; the recurrence does not see it.  The multigrid
 * preconditioner (precon = 3) is applied as P M P -- r is projected before the cycle and z after it, in every iteration:
 * the recurrence is the same in exact arithmetic, and in floating point its history no longer depends on rounding
 * through the constants (1e-13 instead of 1e-6 of an entry near 1e-10).  2 n + 1 projections for n
 * iterations, 24 bytes per point each.
 * Refused (print_error, -1, nothing written): a NULL handle, a handle not made by cedar_amd_solver_create_semidefinite,
 * b or x NULL, the settings cedar_amd_solver_fcg refuses, and for _many what the batched calls refuse (nrhs < 1 or above
 * max_rhs, an F-cycle).  Item m of a batch has the bits of the single-vector call on item m alone. */
int cedar_amd_solver_fcg_semidefinite(cedar_amd_solver *s, const real_t *b, real_t *x, const cedar_amd_pcg_settings *p,
                                      real_t *hist);
int cedar_amd_solver_fcg_semidefinite_many(cedar_amd_solver *s, int nrhs, const real_t *b, real_t *x,
                                           const cedar_amd_pcg_settings *p, real_t *hist, int *iters);
/* The projection as a kernel of its own: v := v - mean_interior(v) on each item m of `active` (bit m) among nrhs level
 * vectors of ii x jj x kk doubles, ghosts included, back to back (kk = 1: a 2D level); host or device.  Ghost cells and
 * items outside `active` are not written.  mean (nrhs doubles, may be NULL) receives the means, 0 for an item outside
 * `active`.  A two-stage sum in a fixed order without atomics: an item's result depends on its extents and values only,
 * not on nrhs or `active`.  It moves 8 bytes per point in the sum and 16 in the shift.  0, or -1 (print_error, nothing
 * written) for nrhs outside 1 .. 32, a NULL v or an extent below 3. */
int cedar_amd_project_mean(int nrhs, unsigned active, real_t *v, len_t ii, len_t jj, len_t kk, real_t *mean);

/* plane relaxation as a kernel of its own -- kernels::plane_relax<stypes, rdir>::setup(so) / run(so, x, b, dir)
 * (include/cedar/kernels/plane_relax.h:10-33; include/cedar/3d/relax_planes.h:164-246, src/3d/relax_planes.cc).
 * dir 0 = xy planes, 1 = xz, 2 = yz; plane_settings = the 2D solvers' configuration (NULL: the reference's default
 * plane-config, line-xy relaxation and one cycle per plane).  so / x / b host or device.  Like the reference, every
 * plane solver of a direction is built from the coefficients of the LAST plane (copy_coeff, relax_planes.h:80-160). */
typedef struct cedar_amd_planes cedar_amd_planes;
cedar_amd_planes *cedar_amd_planes_create(int dir, len_t nx, len_t ny, len_t nz, int nstencil, const real_t *so,
                                          const cedar_amd_settings *plane_settings);
void cedar_amd_planes_run(cedar_amd_planes *p, const real_t *so, real_t *x, const real_t *b, int updown);
void cedar_amd_planes_destroy(cedar_amd_planes *p);

/* ------------------------------------------------------------------ 3. rank-to-rank transport (RCCL over xGMI)
 * What the reference's MPI flavour does through its MSG library and MPI collectives -- the ghost-layer exchange
 * after each colour / residual / interp_add (src/3d/ftn/mpi/BMG3_SymStd_relax_GS.f90:102-147,
 * src/3d/mpi/msg_exchanger.cc:188-197, src/2d/ftn/mpi/mpi_msg.F:425-550), the norm all-reduce
 * (include/cedar/3d/mpi/grid_func.h:41) and the coarse gather (include/cedar/3d/mpi/redist_solver.h:221-224) --
 * as RCCL calls issued by the library itself on its current stream (cedar_amd_set_stream).  One communicator per
 * process / GPU; the 128-byte unique id is made by rank 0 and handed to every rank by the launcher (any channel:
 * cedar_amd/comm.py uses a TCP socket).  librccl.so.1 is loaded on first use; all buffers are device pointers.
 * Functions returning int return 0 on success and report through print_error otherwise. */
#define CEDAR_AMD_COMM_ID_BYTES 128
typedef struct cedar_amd_comm cedar_amd_comm;
int cedar_amd_comm_available(void);                      /* 1 if librccl.so.1 could be loaded */
const char *cedar_amd_comm_why_unavailable(void);
int cedar_amd_comm_unique_id(void *id128);               /* ncclGetUniqueId */
cedar_amd_comm *cedar_amd_comm_create(const void *id128, int rank, int world);  /* ncclCommInitRank on the current device */
void cedar_amd_comm_destroy(cedar_amd_comm *c);
/* the launcher's part in compiled code, for hosts without Python or MPI: rank 0 makes the unique id and serves it over TCP
 * on MASTER_ADDR next to MASTER_PORT, the other ranks fetch it; the handshake carries a job tag (MASTER_PORT, world size,
 * CEDAR_AMD_RUN_ID / TORCHELASTIC_RUN_ID), the wire format is that of cedar_amd/comm.py.  _bootstrap = _bootstrap_id +
 * cedar_amd_comm_create; returns NULL / non-zero on failure (reported through print_error). */
int cedar_amd_comm_bootstrap_id(void *id128, int rank, int world);
cedar_amd_comm *cedar_amd_comm_bootstrap(int rank, int world);
int cedar_amd_comm_rank(const cedar_amd_comm *c);
int cedar_amd_comm_size(const cedar_amd_comm *c);
/* one grouped point-to-point exchange: ncclGroupStart; ncclRecv x nrecv; ncclSend x nsend; ncclGroupEnd (counts in doubles) */
int cedar_amd_comm_exchange(cedar_amd_comm *c, int nsend, const int *speer, const real_t *const *sbuf, const size_t *scount,
                            int nrecv, const int *rpeer, real_t *const *rbuf, const size_t *rcount);
int cedar_amd_comm_allreduce_sum(cedar_amd_comm *c, real_t *buf, size_t n);     /* in place */
int cedar_amd_comm_allreduce_max(cedar_amd_comm *c, real_t *buf, size_t n);
int cedar_amd_comm_allgather(cedar_amd_comm *c, const real_t *send, real_t *recv, size_t count); /* recv: world*count */
int cedar_amd_comm_broadcast(cedar_amd_comm *c, real_t *buf, size_t count, int root);
/* streams for the overlapped halo exchange: a non-blocking side stream; `waiter` waits for what is queued on `waited` now */
void *cedar_amd_stream_create(void);
void cedar_amd_stream_destroy(void *stream);
void cedar_amd_stream_wait(void *waiter, void *waited);
void cedar_amd_device_sync(void);
/* Releases the device scratch the library keeps between calls (the ring of row sums of the 3D Galerkin product: 4.4 GB
 * after a 512^3 set-up; it is re-allocated by the next product that needs it).  Waits for the device first. */
void cedar_amd_release_scratch(void);
/* HIP events on the library's current stream: record returns a new event; elapsed waits for e1 */
void *cedar_amd_event_record(void);
float cedar_amd_event_elapsed_ms(void *e0, void *e1);
void cedar_amd_event_destroy(void *event);

const char *cedar_amd_version(void);

/* ------------------------------------------------------------------ 4. the domain-decomposed 3D solver (one rank per GPU)
 * cdr3::mpi::solver of the reference (include/cedar/3d/mpi/solver.h:76-89,232-233) for Dirichlet problems, point
 * relaxation, V(pre,post): Cartesian block decomposition with one ghost layer, global-parity colouring, a ghost
 * exchange after every row class of a sweep / residual / interp_add and between the phases of the set-up
 * (src/3d/ftn/mpi/BMG3_SymStd_relax_GS.f90:102-147, ..._residual.f90:130, ..._interp_add.f90:308,
 * ..._SETUP_interp_OI.f90:418-1074, ..._SETUP_ITLI27_ex.f90:1803), norm all-reduce (3d/mpi/grid_func.h:41), coarse levels
 * gathered onto every rank (in place of 3d/mpi/redist_solver.h:221-224).  The whole cycle is orchestrated below this ABI
 * (cedar_amd/csrc/dist3.cpp); a rank process only creates the handle and calls it.  rank = k*px*py + j*px + i
 * (src/3d/util/topo.cc:82-84).  Along every SPLIT direction the local extent must be even on every distributed level
 * below the gathered one (create fails otherwise); along an unsplit direction it may be odd on any level.  On a rank grid
 * with an x / y split a 27-point level relaxes by the boundary-first chain where cedar_amd_relax3_masked_ok admits it (nx
 * and ny even, 8 to 512 points per row, at least 8 rows and 128 rows or CEDAR_AMD_FRUN runs for the partial-sum sweep);
 * every other level, those with an odd unsplit nx or ny among them, keeps the reference-order row-class passes.
 * Transport: `comm` (section 3, RCCL) -- or `transport`, a caller-supplied table, the counterpart of the reference's
 * halo_exchanger plug-in (include/cedar/kernel.h:25-37, kernel_manager::add_halo): exchange has the contract of
 * cedar_amd_comm_exchange (device buffers, ordered with the library's current stream), allgather that of
 * cedar_amd_comm_allgather, allreduce_sum sums n HOST doubles in place over the ranks.  Each returns 0 on success. */
typedef struct {
	void *ctx;
	int (*exchange)(void *ctx, int nsend, const int *speer, const real_t *const *sbuf, const size_t *scount,
	                int nrecv, const int *rpeer, real_t *const *rbuf, const size_t *rcount);
	int (*allgather)(void *ctx, const real_t *send, real_t *recv, size_t count);
	int (*allreduce_sum)(void *ctx, double *host_values, int n);
} cedar_amd_transport;
/* a transport that talks to itself (device-to-device copies in place of send / receive): one rank of a `world`-rank grid
 * on a single GPU, for measuring what a rank costs beside its messages; ghost values are meaningless */
void cedar_amd_transport_loopback(cedar_amd_transport *out, int world);
typedef struct cedar_amd_dist3 cedar_amd_dist3;
/* the rank grid used when pgrid is NULL: 1x1xN z slabs up to 4 ranks, 2x2x2 for 8 (BASELINE config 5), else the most
 * cubic factorisation */
void cedar_amd_dist3_rank_grid(int world, int pgrid[3]);
/* A_local: DEVICE array (nstencil, nz+2, ny+2, nx+2) of this rank's part of the global operator (entries coupling to a
 * neighbouring rank present; its ghost layers are filled here); it must outlive the handle.  settings: nrelax_pre /
 * nrelax_post / max_iter / tol / min_coarse are used.  agglomerate_below (0 = 64): a level with at most that many
 * points per direction and rank is gathered and continued on the single-domain solver.  overlap_min (0 = 96): levels
 * with at least that many points per direction run the y/z halo of a row class on a side stream under the interior
 * rows of the next.  Collective: every rank of the communicator calls it. */
cedar_amd_dist3 *cedar_amd_dist3_create(cedar_amd_comm *comm, const cedar_amd_transport *transport, int rank, int world,
                                        const int pgrid[3], real_t *A_local, len_t nx, len_t ny, len_t nz, int nstencil,
                                        const cedar_amd_settings *settings, int agglomerate_below, int overlap_min);
void cedar_amd_dist3_destroy(cedar_amd_dist3 *d);
int cedar_amd_dist3_nlevels(const cedar_amd_dist3 *d);            /* levels of the global hierarchy */
int cedar_amd_dist3_distributed_levels(const cedar_amd_dist3 *d); /* of which this many are distributed (the last one gathered) */
/* distributed levels of a rank grid with an x / y split that relax with the partial-sum sweep behind a boundary-first
 * chain (cedar_amd_relax3_planes_masked; levels it would refuse -- odd nx or ny -- are not counted: they keep the
 * reference-order row-class passes, as every level does with CEDAR_AMD_DIST_CHAIN=0) */
int cedar_amd_dist3_chain_levels(const cedar_amd_dist3 *d);
/* one V-cycle on this rank's device-resident x, b (local boxes incl. ghost layer) */
void cedar_amd_dist3_vcycle(cedar_amd_dist3 *d, real_t *x_dev, real_t *b_dev);
/* mpi::solver::solve: rel[0] = ||r0||_2, rel[i] = ||r_i||_2 / ||r0||_2 (global norms); returns the cycles run */
int cedar_amd_dist3_solve(cedar_amd_dist3 *d, real_t *b_dev, real_t *x_dev, real_t *rel);
/* n level-0 sweeps (alternating DOWN / UP) with their halo exchanges; elapsed ms by HIP events */
float cedar_amd_dist3_time_relax(cedar_amd_dist3 *d, real_t *x_dev, real_t *b_dev, int n);
/* Conjugate gradients preconditioned by the distributed V-cycle (cedar_amd_solver_pcg on a rank grid).
 * Collective, on this rank's device-resident local boxes (ghost layer included) as cedar_amd_dist3_solve.  p as for
 * cedar_amd_solver_pcg (NULL: the defaults); hist (p->max_iter + 1 entries, may be NULL): hist[0] = ||r0||_2,
 * hist[i] = ||r_i||_2 / ||r0||_2 with global norms.  Every scalar is summed over the ranks in rank order, so hist, the
 * return value (the iterations run) and every stop or breakdown decision are the same bits on every rank, and a run
 * repeats bit for bit.  Refused with precon = 3 and nrelax_pre != nrelax_post (the drivers run V-cycles only), or on
 * settings out of range: every rank refuses before any communication, print_error, x untouched, -1.  Breakdown
 * (p.Ap <= 0 or r.z = 0) stops early with x finite.  x's ghosts are current on return.  The first call allocates five
 * level-0 vectors that the handle keeps until cedar_amd_dist3_destroy. */
int cedar_amd_dist3_pcg(cedar_amd_dist3 *d, real_t *b_dev, real_t *x_dev, const cedar_amd_pcg_settings *p, real_t *hist);
/* z = M^-1 r: one distributed V-cycle from z = 0, z's ghosts exchanged (collective; local device boxes).  Refused
 * (z untouched) when nrelax_pre != nrelax_post. */
void cedar_amd_dist3_precondition(cedar_amd_dist3 *d, real_t *z_dev, real_t *r_dev);

/* ------------------------------------------------------------------ 4b. the domain-decomposed 2D solver
 * cdr2::mpi::solver of the reference (include/cedar/2d/mpi/solver.h) for Dirichlet problems on a px x py rank grid
 * (rank = j*px + i), V(pre,post), point relaxation or zebra line relaxation in x, y or both with the lines cut by the
 * ranks of a row / column of the grid -- the reference's distributed tridiagonal solves
 * (src/2d/ftn/mpi/BMG2_SymStd_relax_lines_x.f90:163-307, include/cedar/2d/mpi/ml_relax.h) as a chain of segments whose
 * carries the ranks of a line hand each other (cedar_amd/csrc/dist_lines.hip).  Orchestrated below this ABI
 * (cedar_amd/csrc/dist2.cpp), no torch in a rank process; transport and arguments as for cedar_amd_dist3_create
 * (settings->relaxation selects the smoother).  A_local: device array (nstencil = 3 | 5, ny+2, nx+2). */
typedef struct cedar_amd_dist2 cedar_amd_dist2;
void cedar_amd_dist2_rank_grid(int world, int pgrid[2]);   /* 1x1, 1x2, 2x2, 2x4: y is split first */
cedar_amd_dist2 *cedar_amd_dist2_create(cedar_amd_comm *comm, const cedar_amd_transport *transport, int rank, int world,
                                        const int pgrid[2], real_t *A_local, len_t nx, len_t ny, int nstencil,
                                        const cedar_amd_settings *settings, int agglomerate_below);
void cedar_amd_dist2_destroy(cedar_amd_dist2 *d);
int cedar_amd_dist2_nlevels(const cedar_amd_dist2 *d);
void cedar_amd_dist2_vcycle(cedar_amd_dist2 *d, real_t *x_dev, real_t *b_dev);
int cedar_amd_dist2_solve(cedar_amd_dist2 *d, real_t *b_dev, real_t *x_dev, real_t *rel);
float cedar_amd_dist2_time_relax(cedar_amd_dist2 *d, real_t *x_dev, real_t *b_dev, int n);
/* cedar_amd_dist3_pcg / _precondition for the 2D driver: same contract, any of its smoothers in the preconditioner */
int cedar_amd_dist2_pcg(cedar_amd_dist2 *d, real_t *b_dev, real_t *x_dev, const cedar_amd_pcg_settings *p, real_t *hist);
void cedar_amd_dist2_precondition(cedar_amd_dist2 *d, real_t *z_dev, real_t *r_dev);

/* Cedar's C interface (include/cedar/capi.h: bmg2_* / bmg3_*) with nprocx * nprocy [* nprocz] > 1 runs on the two drivers
 * above, as the reference runs it on its MPI solvers (src/2d/interface/c/solver.cc:10-60).  The MPI_Comm argument is not
 * dereferenced: the rank comes from the launcher's environment (RANK / PMI_RANK / OMPI_COMM_WORLD_RANK / SLURM_PROCID and
 * the matching size variables) or from cedar_amd_bmg_set_rank; the transport is an RCCL communicator the interface
 * bootstraps itself (cedar_amd_comm_bootstrap) unless a table is handed in. */
void cedar_amd_bmg_set_rank(int rank, int world);
void cedar_amd_bmg_set_transport(const cedar_amd_transport *tp);   /* NULL: back to RCCL */

#ifdef __cplusplus
}
#endif
#endif
