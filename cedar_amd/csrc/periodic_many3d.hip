// The 3D periodic sweep and transfers on a batch of right-hand sides that share ONE operator (solver.cpp: handles of
// cedar_amd_solver_create_many_periodic).  periodic3d.hip is the Dirichlet kernels plus ghost
// refreshes; this unit is many3d.hip plus the same refreshes, taken for all items in one launch (wrap3_xy_kernel and
// wrap3_z_kernel take the array from blockIdx.y with the stride of one level vector, so a batch must be stored with
// stride II*JJ*KK -- every caller here does):
//   relax3_gs_per_many    27-point: the four row-class launches of many3d.hip; with x periodic its row task refreshes the x
//                         ghosts of its row per item (relax27_row_task_many<.., PERX>); after each class the y refresh of
//                         the rows and planes it visited, at the end of the sweep the z refresh.  7-point:
//                         relax7_colour_many per colour, each followed by the x / y refresh.
//   restrict3_per_many    ghost refresh of the fine vectors (y, x, z), then restrict3_many
//   interp_add3_per_many  interp_add3_many, then the refresh
// The dense coarsest solve of a batch is solve_cg3_per (periodic3d.hip): one workgroup per item, the factor shared.
// Arithmetic: per item exactly the expressions and the operation order of the single-vector periodic kernels
// (relax27_row_task<.., PERX>), -ffp-contract=off: item m's result has the bits of the single-vector periodic call on
// item m alone.
#include "common.h"

namespace cedar_amd {

// relax3_gs_per (relax3d.hip) on a batch.  The conditions of the row-class path are its own: 27-point, even extents in
// the periodic directions, y ghosts consistent on entry when y is periodic, at most 512 pairs per row.  Where they do
// not hold the items walk through the single-vector colour launches one by one (relax3_gs_per itself: the first
// pre-smoothing sweep on a caller's x with y periodic, odd periodic extents, rows longer than 1024 points).
void relax3_gs_per_many(const real_t *so, const real_t *qf, real_t *q, const real_t *sor, int II, int JJ, int KK, int nstncl,
                        int updown, int ipn, hipStream_t st, int ghosts_consistent, Batch bt)
{
	if (II < 3 || JJ < 3 || KK < 3 || bt.n < 1) return;
	const bool up = (updown == BMG_UP);
	const PerDirs pd = per_dirs(3, ipn); // the one table of the boundary codes (common.h)
	const bool px = pd.x, py = pd.y, pz = pd.z;
	const bool batched = bt.stride == (size_t)II * JJ * KK; // the refresh kernels' array stride
	if (nstncl != 14 && batched) {
		for (int c = 0; c < 2; c++) {
			relax3_colour7_many(so, qf, q, sor, II, JJ, KK, up ? c : 1 - c, st, bt);
			wrap3_colour(q, II, JJ, KK, -1, -1, ipn, st, bt.n);
		}
		wrap3_sweep_end(q, II, JJ, KK, ipn, st, bt.n);
		return;
	}
	if (nstncl == 14 && batched && !(px && (II & 1)) && (!py || ghosts_consistent) && !(py && (JJ & 1)) && !(pz && (KK & 1))
	    && (II - 2 + 1) / 2 <= 512) {
		const Op3 A = op3_cedar(so, sor, II, JJ, KK);
		for (int c = 0; c < 4; c++) {
			const int cc = up ? c : 3 - c, jb = cc & 1, kb = cc >> 1;
			relax3_class27_many(A, qf, q, II, JJ, KK, jb, kb, up, st, bt, px);
			wrap3_colour(q, II, JJ, KK, jb, kb, per3_without_x(ipn), st, bt.n); // x: the row task did it, or it is not periodic
		}
		wrap3_sweep_end(q, II, JJ, KK, ipn, st, bt.n);
		return;
	}
	for (int m = 0; m < bt.n; m++)
		relax3_gs_per(so, qf + m * bt.stride, q + m * bt.stride, sor, II, JJ, KK, nstncl, updown, ipn, st, ghosts_consistent);
}

// ------------------------------------------------------------------ transfers
// (not folded into restrict3_per / interp_add3_per: those launch the single-vector Dirichlet kernels, these the batched ones)
void restrict3_per_many(real_t *q, real_t *qc, const real_t *ci, int II, int JJ, int KK, int IIC, int JJC, int KKC, int ipn,
                        hipStream_t st, Batch bf, Batch bc)
{
	wrap3(q, II, JJ, KK, bf.n, ipn, st);
	restrict3_many(q, qc, ci, II, JJ, KK, IIC, JJC, KKC, st, bf, bc);
}

void interp_add3_per_many(real_t *q, const real_t *qc, const real_t *so, real_t *res, const real_t *ci, int IIC, int JJC,
                          int KKC, int IIF, int JJF, int KKF, int ipn, hipStream_t st, Batch bf, Batch bc)
{
	interp_add3_many(q, qc, so, res, ci, IIC, JJC, KKC, IIF, JJF, KKF, st, bf, bc);
	wrap3(q, IIF, JJF, KKF, bf.n, ipn, st);
}

} // namespace cedar_amd
