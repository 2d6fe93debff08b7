"""The semidefinite solve cases shared by tests/test_semidefinite_statement.py (oracle, CPU) and
tests/test_gpu_semidefinite.py: name -> (operator builder, ibc, cycle settings).  Every operator has zero row sums and
carries the periodic image in ALL its ghost cells (periodic_poisson2 leaves the four ghost corners empty, which the
periodic interpolation set-up reads: it is wrapped once more here)."""
import problems as pb


def wrapped_poisson2(nx, ny):
    so = pb.periodic_poisson2(nx, ny, (1, 1))
    pb.wrap3(so[:, None], (1, 1, 0))
    return so


V21 = dict(nrelax_pre=2, nrelax_post=1)
V11 = dict(nrelax_pre=1, nrelax_post=1)

CASES = {
    "perpoisson5_64x48_v21": (lambda: wrapped_poisson2(64, 48), 3, dict(V21)),
    "perpoisson5_64x48_v11": (lambda: wrapped_poisson2(64, 48), 3, dict(V11)),
    "perpoisson5_64x48_linex": (lambda: wrapped_poisson2(64, 48), 3, dict(V21, relax="line-x")),
    "perpoisson5_64x48_linexy": (lambda: wrapped_poisson2(64, 48), 3, dict(V21, relax="line-xy")),
    "perpoisson5_64x48_f21": (lambda: wrapped_poisson2(64, 48), 3, dict(V21, cycle="f")),
    "perpoisson5_32_v21": (lambda: wrapped_poisson2(32, 32), 3, dict(V21)),
    "perregime9_xy_48x32_v21": (lambda: pb.regime_op((34, 50), 5, 7, p_zero=1, per=(1, 1)), 3, dict(V21)),
    "perregime9_xy_48x32_linexy": (lambda: pb.regime_op((34, 50), 5, 7, p_zero=1, per=(1, 1)), 3, dict(V21, relax="line-xy")),
    "perregime9_x_48x33_v21": (lambda: pb.regime_op((35, 50), 5, 7, p_zero=1, per=(1, 0)), 2, dict(V21)),
    "neumann9_33x29_v21": (lambda: pb.regime_op((31, 35), 5, 9, p_zero=1), 0, dict(V21)),
    "neumann5_40x36_linexy": (lambda: pb.regime_op((38, 42), 3, 9, p_zero=1), 0, dict(V21, relax="line-xy")),
    "neumann9_40x36_f21": (lambda: pb.regime_op((38, 42), 5, 9, p_zero=1), 0, dict(V21, cycle="f")),
    "perpoisson7_xyz_32x16x24_v21": (lambda: pb.periodic_poisson3(32, 16, 24, (1, 1, 1)), 8, dict(V21)),
    "perpoisson7_xyz_16_v21": (lambda: pb.periodic_poisson3(16, 16, 16, (1, 1, 1)), 8, dict(V21)),
    "perregime27_xyz_16x24x16_v21": (lambda: pb.regime_op((18, 26, 18), 14, 5, p_zero=1, per=(1, 1, 1)), 8, dict(V21)),
    "perregime27_z_16x13x16_v21": (lambda: pb.regime_op((18, 15, 18), 14, 5, p_zero=1, per=(0, 0, 1)), 5, dict(V21)),
    "neumann27_17x13x11_v21": (lambda: pb.regime_op((13, 15, 19), 14, 5, p_zero=1), 0, dict(V21)),
    "neumann27_17x13x11_v11": (lambda: pb.regime_op((13, 15, 19), 14, 5, p_zero=1), 0, dict(V11)),
    "neumann7_17x13x11_v21": (lambda: pb.regime_op((13, 15, 19), 4, 5, p_zero=1), 0, dict(V21)),
}

TOL, MAX_ITER = 1e-10, 40
