"""ctypes bindings of include/cedar_amd.h.

`Kernels` exposes the BMG2_/BMG3_SymStd_* drop-ins under the method names the
parity suites use (tests/cases.py); numpy arrays are passed as host pointers and
staged through HBM by the library, `DeviceArray`s are passed as device pointers
and operated on in place.  `Solver` wraps the device-resident handle API.

There is no CPU fallback: a missing library is an ImportError, a missing GPU
makes every compute call abort inside HIP.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIBPATH = os.environ.get("CEDAR_AMD_LIBPATH") or os.path.join(HERE, "lib", "libcedar_amd.so")  # override: A/B of two builds
if not os.path.exists(LIBPATH):
    # not built yet (fresh checkout): compile the HIP sources in-tree; still no CPU fallback
    import shutil
    import subprocess
    if shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"):
        subprocess.call(["make", "-s", "-j8", "-C", os.path.join(HERE, "csrc")])
if not os.path.exists(LIBPATH):
    raise ImportError(
        f"{LIBPATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "(hipcc --offload-arch=gfx950); cedar_amd has no CPU fallback")

lib = C.CDLL(LIBPATH)
P = C.POINTER(C.c_double)
u = C.c_uint
DOWN, UP = 0, 1
RELAX = {"point": 0, "line-x": 1, "line-y": 2, "line-xy": 3, "plane-xy": 4, "plane-xz": 5, "plane-yz": 6, "plane-xyz": 7}
PLANE_DIR = {"xy": 0, "xz": 1, "yz": 2}

lib.cedar_amd_malloc.restype = C.c_void_p
lib.cedar_amd_malloc.argtypes = [C.c_size_t]
lib.cedar_amd_free.argtypes = [C.c_void_p]
lib.cedar_amd_memcpy_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
lib.cedar_amd_memcpy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
lib.cedar_amd_memcpy_d2d.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
lib.cedar_amd_memset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
lib.cedar_amd_l2norm.restype = C.c_double
lib.cedar_amd_l2norm.argtypes = [C.c_void_p, u, u, u]
lib.cedar_amd_version.restype = C.c_char_p
lib.cedar_amd_get_stream.restype = C.c_void_p
lib.cedar_amd_set_stream.argtypes = [C.c_void_p]


class Settings(C.Structure):
    _fields_ = [("relaxation", C.c_int), ("nrelax_pre", C.c_int), ("nrelax_post", C.c_int),
                ("num_levels", C.c_int), ("max_iter", C.c_int), ("tol", C.c_double),
                ("min_coarse", C.c_int), ("cycle", C.c_int), ("ibc", C.c_int),
                ("plane_relaxation", C.c_int), ("plane_nrelax_pre", C.c_int), ("plane_nrelax_post", C.c_int),
                ("plane_max_iter", C.c_int), ("plane_min_coarse", C.c_int), ("plane_tol", C.c_double)]


def plane_settings(st, plane):
    """fill the "plane-config" part of a Settings from plane = dict(relax=, nrelax_pre=, nrelax_post=, max_iter=,
    min_coarse=, tol=) or None (the reference's default: line-xy, one cycle per plane)"""
    plane = plane or {}
    st.plane_relaxation = RELAX[plane.get("relax", "line-xy")]
    st.plane_nrelax_pre, st.plane_nrelax_post = plane.get("nrelax_pre", 2), plane.get("nrelax_post", 1)
    st.plane_max_iter, st.plane_min_coarse = plane.get("max_iter", 1), plane.get("min_coarse", 3)
    st.plane_tol = float(plane.get("tol", 1e-8))
    return st


def device_count():
    return lib.cedar_amd_device_count()


def set_device(dev):
    if lib.cedar_amd_set_device(int(dev)) != 0:
        raise RuntimeError(f"hipSetDevice({dev}) failed")


def release_scratch():
    """frees the device scratch the library keeps between calls (cedar_amd_release_scratch)"""
    lib.cedar_amd_release_scratch()


def sync():
    lib.cedar_amd_sync()


class DeviceArray:
    """FP64 array resident in HBM (shape = reversed Fortran shape, like the numpy side)."""

    def __init__(self, shape):
        self.shape = tuple(int(s) for s in shape)
        self.size = int(np.prod(self.shape))
        self.ptr = lib.cedar_amd_malloc(self.size * 8)
        if not self.ptr:
            raise MemoryError("cedar_amd_malloc failed")

    @classmethod
    def from_numpy(cls, a):
        d = cls(a.shape)
        d.upload(a)
        return d

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert a.size == self.size
        lib.cedar_amd_memcpy_h2d(self.ptr, a.ctypes.data, self.size * 8)

    def numpy(self):
        out = np.empty(self.shape)
        lib.cedar_amd_memcpy_d2h(out.ctypes.data, self.ptr, self.size * 8)
        return out

    def zero(self):
        lib.cedar_amd_memset(self.ptr, 0, self.size * 8)

    def copy_from(self, other):
        assert other.size == self.size
        lib.cedar_amd_memcpy_d2d(self.ptr, other.ptr, self.size * 8)

    def free(self):
        if self.ptr:
            lib.cedar_amd_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _p(a):
    """host numpy array or DeviceArray -> pointer argument"""
    if a is None:
        return None
    if isinstance(a, DeviceArray):
        return C.cast(a.ptr, P)
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(P)


def l2norm(v):
    shp = v.shape
    KK = shp[0] if len(shp) == 3 else 1
    ptr = v.ptr if isinstance(v, DeviceArray) else v.ctypes.data
    return lib.cedar_amd_l2norm(ptr, shp[-1], shp[-2], KK)


class Kernels:
    """The BMG*_SymStd_* entry points, argument marshalling exactly as in the
    reference's binding classes (include/cedar/{2d,3d}/relax.h etc.)."""

    L = lib

    # ---- 2D
    def setup_recip2(self, so, sor):
        nst, JJ, II = so.shape
        lib.BMG2_SymStd_SETUP_recip(_p(so), _p(sor), u(II), u(JJ), nst, 2)

    # ibc: the boundary code the reference's bindings obtain from BMG_get_bc(per_mask) and hand to every
    # kernel (0 definite, 1 periodic in y, 2 in x, 3 in both; include/cedar/2d/relax.h:97 ...)
    def relax2(self, so, qf, q, sor, updown, ibc=0):
        nst, JJ, II = so.shape
        lib.BMG2_SymStd_relax_GS(1, _p(so), _p(qf), _p(q), _p(sor), u(II), u(JJ), 1, int(nst == 3), nst, 2, 1, updown, ibc)

    def relax2_psum(self, so, qf, q, sor, updown):
        """nine-point sweep with inter-row partial sums (cedar_amd_relax2_gs_psum); returns 1 if that path ran"""
        nst, JJ, II = so.shape
        assert nst == 5
        return lib.cedar_amd_relax2_gs_psum(_p(so), _p(qf), _p(q), _p(sor), u(II), u(JJ), updown)

    def relax2_op32(self, so, qf, q, sor, updown):
        """2D point sweep (nine- or five-point) on the operator and 1/diag rounded to single precision
        (cedar_amd_relax2_gs_op32), reference order; 0, or -1 if refused (q untouched)"""
        nst, JJ, II = so.shape
        return lib.cedar_amd_relax2_gs_op32(_p(so), _p(qf), _p(q), _p(sor), u(II), u(JJ), nst, updown)

    def relax2_psum_op32(self, so, qf, q, sor, updown):
        """nine-point partial-sum sweep on the rounded operator (cedar_amd_relax2_gs_psum_op32); 1 if that path ran, 0 if
        the reference-order sweep ran, -1 if refused"""
        nst, JJ, II = so.shape
        assert nst == 5
        return lib.cedar_amd_relax2_gs_psum_op32(_p(so), _p(qf), _p(q), _p(sor), u(II), u(JJ), updown)

    def residual2_op32(self, so, qf, q, res):
        """2D residual on the operator rounded to single precision (cedar_amd_residual2_op32); 0, or -1 if refused"""
        nst, JJ, II = so.shape
        return lib.cedar_amd_residual2_op32(_p(so), _p(qf), _p(q), _p(res), u(II), u(JJ), nst)

    def relax2_many_op32(self, so, qf, q, sor, updown, nrhs=None):
        """relax2_op32 on the items of qf, q of shape (nrhs,) + grid (cedar_amd_relax2_gs_many_op32); 0, or -1 if refused"""
        nst, JJ, II = so.shape
        return lib.cedar_amd_relax2_gs_many_op32(q.shape[0] if nrhs is None else nrhs, _p(so), _p(qf), _p(q), _p(sor),
                                                 u(II), u(JJ), nst, updown)

    def relax2_lines_op32(self, so, qf, q, sor, dir, updown):
        """one zebra line sweep (dir 0: x lines, 1: y lines with sor = SOR(JJ,II,2)) on the operator and the line factors
        rounded to single precision (cedar_amd_relax2_lines_op32); 0, or -1 if refused (q untouched)"""
        nst, JJ, II = so.shape
        return lib.cedar_amd_relax2_lines_op32(_p(so), _p(qf), _p(q), _p(sor), u(II), u(JJ), nst, dir, updown)

    def relax2_lines_many_op32(self, so, qf, q, sor, dir, updown, nrhs=None):
        """relax2_lines_op32 on the items of qf, q of shape (nrhs,) + grid (cedar_amd_relax2_lines_many_op32); 0, or -1 if
        refused"""
        nst, JJ, II = so.shape
        return lib.cedar_amd_relax2_lines_many_op32(q.shape[0] if nrhs is None else nrhs, _p(so), _p(qf), _p(q), _p(sor),
                                                    u(II), u(JJ), nst, dir, updown)

    def residual2_many_op32(self, so, qf, q, res, nrhs=None):
        """residual2_op32 on the items of qf, q, res (cedar_amd_residual2_many_op32); 0, or -1 if refused"""
        nst, JJ, II = so.shape
        return lib.cedar_amd_residual2_many_op32(q.shape[0] if nrhs is None else nrhs, _p(so), _p(qf), _p(q), _p(res),
                                                 u(II), u(JJ), nst)

    def setup_lines2(self, so, sor, d, ibc=0):
        nst, JJ, II = so.shape
        f = lib.BMG2_SymStd_SETUP_lines_x if d == "x" else lib.BMG2_SymStd_SETUP_lines_y
        f(_p(so), _p(sor), u(II), u(JJ), nst, ibc)

    def relax_lines2(self, so, qf, q, sor, updown, d, ibc=0):
        nst, JJ, II = so.shape
        f = lib.BMG2_SymStd_relax_lines_x if d == "x" else lib.BMG2_SymStd_relax_lines_y
        f(1, _p(so), _p(qf), _p(q), _p(sor), None, u(II), u(JJ), 1, int(nst == 3), nst, 1, updown, ibc)

    def residual2(self, so, qf, q, res):
        nst, JJ, II = so.shape
        i = lambda v: C.byref(C.c_int(v))
        lib.BMG2_SymStd_residual(i(0), _p(so), _p(qf), _p(q), _p(res), C.byref(u(II)), C.byref(u(JJ)),
                                 i(0), i(int(nst == 3)), i(nst), i(0), i(0), i(0), i(0))

    def matvec2(self, so, q, qf):
        nst, JJ, II = so.shape
        lib.cedar_amd_matvec2(_p(so), _p(q), _p(qf), u(II), u(JJ), nst)

    def matvec3(self, so, q, qf):
        nst, KK, JJ, II = so.shape
        lib.cedar_amd_matvec3(_p(so), _p(q), _p(qf), u(II), u(JJ), u(KK), nst)

    def restrict2(self, q, qc, ci, ibc=0):
        JJ, II = q.shape
        JJC, IIC = qc.shape
        lib.BMG2_SymStd_restrict(_p(q), _p(qc), _p(ci), II, JJ, IIC, JJC, ibc)

    def interp_add2(self, q, qc, res, so, ci, ibc=0):
        JJ, II = q.shape
        JJC, IIC = qc.shape
        lib.BMG2_SymStd_interp_add(_p(q), _p(qc), _p(res), _p(so), _p(ci), u(IIC), u(JJC), u(II), u(JJ), so.shape[0], ibc)

    def setup_interp2(self, so, ci, ibc=0):
        nst, JJ, II = so.shape
        _, JJC, IIC = ci.shape
        lib.BMG2_SymStd_SETUP_interp_OI(_p(so), None, _p(ci), u(II), u(JJ), u(IIC), u(JJC), int(nst == 3), nst, ibc, 0)

    def galerkin2(self, so, soc, ci, ibc=0):
        nst, JJ, II = so.shape
        _, JJC, IIC = ci.shape
        lib.BMG2_SymStd_SETUP_ITLI_ex(_p(so), _p(soc), _p(ci), u(II), u(JJ), u(IIC), u(JJC), int(nst == 3), nst, ibc)

    def setup_cg2(self, so, abd, ibc=0):
        nst, JJ, II = so.shape
        n2, n1 = abd.shape
        r = lambda v: C.byref(u(v))
        lib.BMG2_SymStd_SETUP_cg_LU(_p(so), r(II), r(JJ), C.byref(C.c_int(nst)), _p(abd), r(n1), r(n2), C.byref(C.c_int(ibc)))

    def solve_cg2(self, q, qf, abd, ibc=0):
        JJ, II = q.shape
        n2, n1 = abd.shape
        bbd = np.zeros(n2)
        lib.BMG2_SymStd_SOLVE_cg(_p(q), _p(qf), u(II), u(JJ), _p(abd), _p(bbd), u(n1), u(n2), ibc)

    # ---- 3D
    def setup_recip3(self, so, sor):
        nst, KK, JJ, II = so.shape
        lib.BMG3_SymStd_SETUP_recip(_p(so), _p(sor), u(II), u(JJ), u(KK), nst, 2)

    def relax3(self, so, qf, q, sor, updown, ibc=0):
        nst, KK, JJ, II = so.shape
        lib.BMG3_SymStd_relax_GS(1, _p(so), _p(qf), _p(q), _p(sor), u(II), u(JJ), u(KK), int(nst == 4), nst, 2, 1, updown, ibc)

    def relax3_psum(self, so, qf, q, sor, updown):
        """27-point sweep with inter-plane partial sums (cedar_amd_relax3_gs_psum); returns 1 if that path ran"""
        nst, KK, JJ, II = so.shape
        assert nst == 14
        return lib.cedar_amd_relax3_gs_psum(_p(so), _p(qf), _p(q), _p(sor), C.cast(None, P), u(II), u(JJ), u(KK), updown)

    def relax3_op32(self, so, qf, q, sor, updown, frun=0):
        """27-point sweep on the operator and 1/diag rounded to single precision (cedar_amd_relax3_gs_op32): frun > 0 the
        partial-sum sweep with that run length, 0 the reference order; returns 1 if the partial-sum path ran, -1 if refused"""
        nst, KK, JJ, II = so.shape
        assert nst == 14
        return lib.cedar_amd_relax3_gs_op32(_p(so), _p(qf), _p(q), _p(sor), C.cast(None, P), u(II), u(JJ), u(KK), updown, int(frun))

    def residual3_op32(self, so, qf, q, res):
        """27-point residual on the operator rounded to single precision (cedar_amd_residual3_op32); -1 if refused"""
        nst, KK, JJ, II = so.shape
        assert nst == 14
        return lib.cedar_amd_residual3_op32(_p(so), _p(qf), _p(q), _p(res), u(II), u(JJ), u(KK))

    def relax7_op32(self, so, qf, q, sor, updown):
        """7-point sweep on the operator and 1/diag rounded to single precision (cedar_amd_relax7_gs_op32); 0, or -1 if
        refused (q untouched)"""
        nst, KK, JJ, II = so.shape
        assert nst == 4
        return lib.cedar_amd_relax7_gs_op32(_p(so), _p(qf), _p(q), _p(sor), u(II), u(JJ), u(KK), updown)

    def residual7_op32(self, so, qf, q, res):
        """7-point residual on the operator rounded to single precision (cedar_amd_residual7_op32); -1 if refused"""
        nst, KK, JJ, II = so.shape
        assert nst == 4
        return lib.cedar_amd_residual7_op32(_p(so), _p(qf), _p(q), _p(res), u(II), u(JJ), u(KK))

    def residual3(self, so, qf, q, res):
        nst, KK, JJ, II = so.shape
        lib.BMG3_SymStd_residual(1, 1, int(nst == 4), _p(q), _p(qf), _p(so), _p(res), u(II), u(JJ), u(KK), nst)

    def restrict3(self, q, qc, ci, ibc=0):
        KK, JJ, II = q.shape
        KKC, JJC, IIC = qc.shape
        lib.BMG3_SymStd_restrict(_p(q), _p(qc), _p(ci), u(II), u(JJ), u(KK), u(IIC), u(JJC), u(KKC), ibc)

    def interp_add3(self, q, qc, so, res, ci, ibc=0):
        KK, JJ, II = q.shape
        KKC, JJC, IIC = qc.shape
        lib.BMG3_SymStd_interp_add(_p(q), _p(qc), _p(so), _p(res), _p(ci), u(IIC), u(JJC), u(KKC), u(II), u(JJ), u(KK), so.shape[0], ibc)

    def setup_interp3(self, so, ci, ibc=0):
        nst, KK, JJ, II = so.shape
        _, KKC, JJC, IIC = ci.shape
        lib.BMG3_SymStd_SETUP_interp_OI(_p(so), None, _p(ci), u(II), u(JJ), u(KK), u(IIC), u(JJC), u(KKC),
                                        int(nst == 4), nst, 1, ibc, None)

    def galerkin3(self, so, soc, ci, ibc=0):
        nst, KK, JJ, II = so.shape
        _, KKC, JJC, IIC = ci.shape
        f = lib.BMG3_SymStd_SETUP_ITLI07_ex if nst == 4 else lib.BMG3_SymStd_SETUP_ITLI27_ex
        f(_p(so), _p(soc), _p(ci), u(II), u(JJ), u(KK), u(IIC), u(JJC), u(KKC), ibc)

    def setup_cg3(self, so, abd, ibc=0):
        nst, KK, JJ, II = so.shape
        n2, n1 = abd.shape
        lib.BMG3_SymStd_SETUP_cg_LU(_p(so), u(II), u(JJ), u(KK), nst, _p(abd), u(n1), u(n2), ibc)

    def solve_cg3(self, q, qf, abd, ibc=0):
        KK, JJ, II = q.shape
        n2, n1 = abd.shape
        bbd = np.zeros(n2)
        lib.BMG3_SymStd_SOLVE_cg(_p(q), _p(qf), u(II), u(JJ), u(KK), _p(abd), _p(bbd), u(n1), u(n2), ibc)

    def relax_planes3(self, so, x, b, d, updown, plane=None):
        """kman->setup<plane_relax<d>>(so); kman->run<plane_relax<d>>(so, x, b, updown) (cedar_amd_planes_*)"""
        nst, KK, JJ, II = so.shape
        st = None
        if plane is not None:
            st = Settings()
            lib.cedar_amd_default_settings(C.byref(st))
            st.relaxation = RELAX[plane.get("relax", "line-xy")]
            st.nrelax_pre, st.nrelax_post = plane.get("nrelax_pre", 2), plane.get("nrelax_post", 1)
            st.max_iter, st.min_coarse, st.tol = plane.get("max_iter", 1), plane.get("min_coarse", 3), float(plane.get("tol", 1e-8))
        lib.cedar_amd_planes_create.restype = C.c_void_p
        h = lib.cedar_amd_planes_create(PLANE_DIR[d], u(II - 2), u(JJ - 2), u(KK - 2), nst, _p(so), C.byref(st) if st else None)
        if not h:
            raise RuntimeError("cedar_amd_planes_create failed")
        h = C.c_void_p(h)
        lib.cedar_amd_planes_run(h, _p(so), _p(x), _p(b), updown)
        lib.cedar_amd_planes_destroy(h)

    # ---- the batched 3D kernels (many3d.hip): vectors of shape (nrhs,) + grid, item-major; operator arrays are shared.
    # nrhs: work on the first nrhs items only (default: all the arrays hold)
    @staticmethod
    def _many(name, rc):
        if rc != 0:
            raise RuntimeError(f"{name} refused")

    def relax3_many(self, so, qf, q, sor, updown, nrhs=None):
        nst, KK, JJ, II = so.shape
        assert qf.shape == q.shape and tuple(q.shape[1:]) == (KK, JJ, II)
        self._many("cedar_amd_relax3_gs_many",
                   lib.cedar_amd_relax3_gs_many(q.shape[0] if nrhs is None else nrhs, _p(so), _p(qf), _p(q), _p(sor), u(II), u(JJ), u(KK), nst, updown))

    def residual3_many(self, so, qf, q, res, nrhs=None):
        nst, KK, JJ, II = so.shape
        assert qf.shape == q.shape == res.shape and tuple(q.shape[1:]) == (KK, JJ, II)
        self._many("cedar_amd_residual3_many",
                   lib.cedar_amd_residual3_many(q.shape[0] if nrhs is None else nrhs, _p(so), _p(qf), _p(q), _p(res), u(II), u(JJ), u(KK), nst))

    def relax3_many_op32(self, so, qf, q, sor, updown, nrhs=None):
        """the batched 27-point sweep on the operator and 1/diag rounded to single precision
        (cedar_amd_relax3_gs_many_op32), reference order; 0, or -1 if refused (q untouched)"""
        grid = q.shape[1:]
        KK, JJ, II = grid
        return lib.cedar_amd_relax3_gs_many_op32(q.shape[0] if nrhs is None else nrhs, _p(so), _p(qf), _p(q), _p(sor), u(II), u(JJ), u(KK), updown)

    def residual3_many_op32(self, so, qf, q, res, nrhs=None):
        """the batched 27-point residual on the operator rounded to single precision (cedar_amd_residual3_many_op32);
        0, or -1 if refused (res untouched)"""
        grid = q.shape[1:]
        KK, JJ, II = grid
        return lib.cedar_amd_residual3_many_op32(q.shape[0] if nrhs is None else nrhs, _p(so), _p(qf), _p(q), _p(res), u(II), u(JJ), u(KK))

    def relax7_many_op32(self, so, qf, q, sor, updown, nrhs=None):
        """the batched 7-point sweep on the operator and 1/diag rounded to single precision
        (cedar_amd_relax7_gs_many_op32); 0, or -1 if refused (q untouched)"""
        KK, JJ, II = q.shape[1:]
        return lib.cedar_amd_relax7_gs_many_op32(q.shape[0] if nrhs is None else nrhs, _p(so), _p(qf), _p(q), _p(sor), u(II), u(JJ), u(KK), updown)

    def residual7_many_op32(self, so, qf, q, res, nrhs=None):
        """the batched 7-point residual on the operator rounded to single precision (cedar_amd_residual7_many_op32);
        0, or -1 if refused (res untouched)"""
        KK, JJ, II = q.shape[1:]
        return lib.cedar_amd_residual7_many_op32(q.shape[0] if nrhs is None else nrhs, _p(so), _p(qf), _p(q), _p(res), u(II), u(JJ), u(KK))

    def restrict3_many(self, q, qc, ci, nrhs=None):
        n, KK, JJ, II = q.shape
        nc, KKC, JJC, IIC = qc.shape
        assert n == nc
        self._many("cedar_amd_restrict3_many",
                   lib.cedar_amd_restrict3_many(n if nrhs is None else nrhs, _p(q), _p(qc), _p(ci), u(II), u(JJ), u(KK), u(IIC), u(JJC), u(KKC)))

    def interp_add3_many(self, q, qc, so, res, ci, nrhs=None):
        n, KK, JJ, II = q.shape
        nc, KKC, JJC, IIC = qc.shape
        assert n == nc and res.shape == q.shape
        self._many("cedar_amd_interp_add3_many",
                   lib.cedar_amd_interp_add3_many(n if nrhs is None else nrhs, _p(q), _p(qc), _p(so), _p(res), _p(ci), u(IIC), u(JJC), u(KKC),
                                                  u(II), u(JJ), u(KK), so.shape[0]))

    # ---- the batched periodic 3D kernels (periodic_many3d.hip, krylov.hip): the arguments of the Dirichlet _many methods
    # plus the boundary code ibc (1..3, 5..8; 0 forwards to the Dirichlet call).  Item m gets the bits of the single-vector
    # periodic drop-in on item m alone.  RuntimeError when the library refuses (nothing written)
    def relax3_periodic_many(self, so, qf, q, sor, updown, ibc, ghosts_consistent=0, nrhs=None):
        """ghosts_consistent: the y ghost rows of q hold the periodic image on entry (lets a y-periodic 27-point sweep take
        the row-class path); 0 is always correct"""
        nst, KK, JJ, II = so.shape
        assert qf.shape == q.shape and tuple(q.shape[1:]) == (KK, JJ, II)
        self._many("cedar_amd_relax3_gs_periodic_many",
                   lib.cedar_amd_relax3_gs_periodic_many(q.shape[0] if nrhs is None else nrhs, _p(so), _p(qf), _p(q), _p(sor), u(II),
                                                         u(JJ), u(KK), nst, updown, int(ibc), int(ghosts_consistent)))

    def restrict3_periodic_many(self, q, qc, ci, ibc, nrhs=None):
        """the ghosts of the fine vectors are refreshed first: q is written too"""
        n, KK, JJ, II = q.shape
        nc, KKC, JJC, IIC = qc.shape
        assert n == nc
        self._many("cedar_amd_restrict3_periodic_many",
                   lib.cedar_amd_restrict3_periodic_many(n if nrhs is None else nrhs, _p(q), _p(qc), _p(ci), u(II), u(JJ), u(KK),
                                                         u(IIC), u(JJC), u(KKC), int(ibc)))

    def interp_add3_periodic_many(self, q, qc, so, res, ci, ibc, nrhs=None):
        n, KK, JJ, II = q.shape
        nc, KKC, JJC, IIC = qc.shape
        assert n == nc and res.shape == q.shape
        self._many("cedar_amd_interp_add3_periodic_many",
                   lib.cedar_amd_interp_add3_periodic_many(n if nrhs is None else nrhs, _p(q), _p(qc), _p(so), _p(res), _p(ci), u(IIC),
                                                           u(JJC), u(KKC), u(II), u(JJ), u(KK), so.shape[0], int(ibc)))

    def solve_cg3_periodic_many(self, q, qf, abd, ibc, nrhs=None):
        """abd: the dense factor setup_cg3(so, abd, ibc) left, shared by the items; one workgroup per item"""
        n, KK, JJ, II = q.shape
        assert qf.shape == q.shape
        n = n if nrhs is None else nrhs
        bbd = np.zeros(max(n, 1) * abd.shape[0])
        self._many("cedar_amd_solve_cg3_periodic_many",
                   lib.cedar_amd_solve_cg3_periodic_many(n, _p(q), _p(qf), u(II), u(JJ), u(KK), _p(abd), _p(bbd), u(abd.shape[1]),
                                                         int(ibc)))

    def pcg_direction_periodic_many(self, so, z, p, pn, w, ibc, first, sc, nrhs=None, active=None):
        """pcg_direction_many on a periodic 3D level: per item m the reads of pcg_direction_periodic"""
        assert tuple(so.shape[1:]) == tuple(z.shape[1:]) and all(a is None or a.shape == z.shape for a in (p, pn, w))
        n, act = self._batch(z, sc, nrhs, active)
        grid = z.shape[1:]
        if lib.cedar_amd_pcg_direction_periodic_many(n, act, _p(so), _p(z), _p(p), _p(pn), _p(w), u(grid[-1]), u(grid[-2]),
                                                     u(grid[0] if len(grid) == 3 else 1), so.shape[0], int(ibc), int(first),
                                                     _p(sc)) != 0:
            raise RuntimeError("cedar_amd_pcg_direction_periodic_many refused")

    # ---- the batched periodic 2D kernels (periodic_many2d.hip, krylov.hip): the arguments of the single-vector 2D methods
    # on vectors of shape (nrhs,) + grid, plus the boundary code ibc (1..3; 0 is refused except by the direction pass, which
    # forwards to pcg_direction_many).  Item m gets the bits of the single-vector periodic method on item m alone.
    # RuntimeError when the library refuses (nothing written)
    def relax2_periodic_many(self, so, qf, q, sor, updown, ibc, nrhs=None):
        nst, JJ, II = so.shape
        assert qf.shape == q.shape and tuple(q.shape[1:]) == (JJ, II)
        self._many("cedar_amd_relax2_gs_periodic_many",
                   lib.cedar_amd_relax2_gs_periodic_many(q.shape[0] if nrhs is None else nrhs, _p(so), _p(qf), _p(q), _p(sor), u(II),
                                                         u(JJ), nst, updown, int(ibc)))

    def restrict2_periodic_many(self, q, qc, ci, ibc, nrhs=None):
        """the ghosts of the fine vectors are refreshed first: q is written too"""
        n, JJ, II = q.shape
        nc, JJC, IIC = qc.shape
        assert n == nc
        self._many("cedar_amd_restrict2_periodic_many",
                   lib.cedar_amd_restrict2_periodic_many(n if nrhs is None else nrhs, _p(q), _p(qc), _p(ci), u(II), u(JJ), u(IIC),
                                                         u(JJC), int(ibc)))

    def interp_add2_periodic_many(self, q, qc, res, so, ci, ibc, nrhs=None):
        n, JJ, II = q.shape
        nc, JJC, IIC = qc.shape
        assert n == nc and res.shape == q.shape
        self._many("cedar_amd_interp_add2_periodic_many",
                   lib.cedar_amd_interp_add2_periodic_many(n if nrhs is None else nrhs, _p(q), _p(qc), _p(res), _p(so), _p(ci), u(IIC),
                                                           u(JJC), u(II), u(JJ), so.shape[0], int(ibc)))

    def solve_cg2_periodic_many(self, q, qf, abd, ibc, nrhs=None):
        """abd: the dense factor setup_cg2(so, abd, ibc) left, shared by the items; one lane per item"""
        n, JJ, II = q.shape
        assert qf.shape == q.shape
        n = n if nrhs is None else nrhs
        bbd = np.zeros(max(n, 1) * abd.shape[0])
        self._many("cedar_amd_solve_cg2_periodic_many",
                   lib.cedar_amd_solve_cg2_periodic_many(n, _p(q), _p(qf), u(II), u(JJ), _p(abd), _p(bbd), u(abd.shape[1]), int(ibc)))

    def pcg_direction2_periodic_many(self, so, z, p, pn, w, ibc, first, sc, nrhs=None, active=None):
        """pcg_direction_many on a periodic 2D level: per item m the reads of pcg_direction_periodic"""
        assert tuple(so.shape[1:]) == tuple(z.shape[1:]) and all(a is None or a.shape == z.shape for a in (p, pn, w))
        n, act = self._batch(z, sc, nrhs, active)
        JJ, II = z.shape[1:]
        if lib.cedar_amd_pcg_direction2_periodic_many(n, act, _p(so), _p(z), _p(p), _p(pn), _p(w), u(II), u(JJ), so.shape[0],
                                                      int(ibc), int(first), _p(sc)) != 0:
            raise RuntimeError("cedar_amd_pcg_direction2_periodic_many refused")

    # ---- the transfers on the interpolation weights rounded to single precision (transferf.hip): a float copy of ci is built
    # for the call; arguments as the FP64 methods above (Dirichlet).  0 when served, non-zero when refused (nothing written)
    def restrict2_ci32(self, q, qc, ci):
        JJ, II = q.shape
        JJC, IIC = qc.shape
        return lib.cedar_amd_restrict2_ci32(_p(q), _p(qc), _p(ci), II, JJ, IIC, JJC)

    def interp_add2_ci32(self, q, qc, res, so, ci):
        JJ, II = q.shape
        JJC, IIC = qc.shape
        return lib.cedar_amd_interp_add2_ci32(_p(q), _p(qc), _p(res), _p(so), _p(ci), u(IIC), u(JJC), u(II), u(JJ), so.shape[0])

    def restrict3_ci32(self, q, qc, ci):
        KK, JJ, II = q.shape
        KKC, JJC, IIC = qc.shape
        return lib.cedar_amd_restrict3_ci32(_p(q), _p(qc), _p(ci), u(II), u(JJ), u(KK), u(IIC), u(JJC), u(KKC))

    def interp_add3_ci32(self, q, qc, so, res, ci):
        KK, JJ, II = q.shape
        KKC, JJC, IIC = qc.shape
        return lib.cedar_amd_interp_add3_ci32(_p(q), _p(qc), _p(so), _p(res), _p(ci), u(IIC), u(JJC), u(KKC), u(II), u(JJ), u(KK),
                                              so.shape[0])

    def restrict3_many_ci32(self, q, qc, ci, nrhs=None):
        n, KK, JJ, II = q.shape
        nc, KKC, JJC, IIC = qc.shape
        assert n == nc
        return lib.cedar_amd_restrict3_many_ci32(n if nrhs is None else nrhs, _p(q), _p(qc), _p(ci), u(II), u(JJ), u(KK), u(IIC),
                                                 u(JJC), u(KKC))

    def interp_add3_many_ci32(self, q, qc, so, res, ci, nrhs=None):
        n, KK, JJ, II = q.shape
        nc, KKC, JJC, IIC = qc.shape
        assert n == nc and res.shape == q.shape
        return lib.cedar_amd_interp_add3_many_ci32(n if nrhs is None else nrhs, _p(q), _p(qc), _p(so), _p(res), _p(ci), u(IIC),
                                                   u(JJC), u(KKC), u(II), u(JJ), u(KK), so.shape[0])

    # ---- the passes of a CG iteration (krylov.hip), one launcher each; sc: the PCG_NSC scalar block, in and out
    @staticmethod
    def _dims(a):
        shp = a.shape
        return (u(shp[-1]), u(shp[-2]), u(shp[0] if len(shp) == 3 else 1))

    def pcg_direction(self, so, z, p, pn, w, first, sc, partial=None):
        """pn = z + beta p (first: z), w = A pn, sigma = pn.w -> sc (or partial[0], sc untouched)"""
        assert tuple(so.shape[1:]) == tuple(z.shape) and all(a is None or a.shape == z.shape for a in (p, pn, w))
        assert sc.size == 8 and (partial is None or partial.size >= 1)
        if lib.cedar_amd_pcg_direction(_p(so), _p(z), _p(p), _p(pn), _p(w), *self._dims(z), so.shape[0], int(first),
                                       _p(sc), _p(partial)) != 0:
            raise RuntimeError("cedar_amd_pcg_direction refused")

    def pcg_direction_periodic(self, so, z, p, pn, w, ibc, first, sc, partial=None):
        """pcg_direction on a level with the periodic directions of boundary code ibc: a neighbour on the ghost layer of
        a periodic direction is read at the opposite interior end; no such ghost of z or p contributes to a result"""
        assert tuple(so.shape[1:]) == tuple(z.shape) and all(a is None or a.shape == z.shape for a in (p, pn, w))
        assert sc.size == 8 and (partial is None or partial.size >= 1)
        if lib.cedar_amd_pcg_direction_periodic(_p(so), _p(z), _p(p), _p(pn), _p(w), *self._dims(z), so.shape[0], int(ibc),
                                                int(first), _p(sc), _p(partial)) != 0:
            raise RuntimeError("cedar_amd_pcg_direction_periodic refused")

    def pcg_update(self, zmode, move, x, r, p, w, z, diag, first, sc, partial=None):
        """x += alpha p, r -= alpha w (move), r.r and r.z by zmode -> sc (or partial[0:2], sc untouched)"""
        assert all(a is None or a.shape == r.shape for a in (x, p, w, z, diag))
        assert sc.size == 8 and (partial is None or partial.size >= 2)
        if lib.cedar_amd_pcg_update(int(zmode), int(move), _p(x), _p(r), _p(p), _p(w), _p(z), _p(diag), *self._dims(r),
                                    int(first), _p(sc), _p(partial)) != 0:
            raise RuntimeError("cedar_amd_pcg_update refused")

    # the same two passes on a batch: vectors of shape (items,) + grid, item-major, sc of shape (items, 8); nrhs: work on
    # the first nrhs items only (default: all); active: bit mask of the items that take part (default: all nrhs)
    @staticmethod
    def _batch(v, sc, nrhs, active):
        n = int(v.shape[0] if nrhs is None else nrhs)
        assert sc.size >= 8 * n and v.shape[0] >= n
        return n, u((1 << n) - 1 if active is None else int(active))

    def pcg_direction_many(self, so, z, p, pn, w, first, sc, nrhs=None, active=None):
        """per item m: pn = z + beta_m p (first: z), w = A pn, sigma = pn.w -> sc[m]"""
        assert tuple(so.shape[1:]) == tuple(z.shape[1:]) and all(a is None or a.shape == z.shape for a in (p, pn, w))
        n, act = self._batch(z, sc, nrhs, active)
        grid = z.shape[1:]
        if lib.cedar_amd_pcg_direction_many(n, act, _p(so), _p(z), _p(p), _p(pn), _p(w), u(grid[-1]), u(grid[-2]),
                                            u(grid[0] if len(grid) == 3 else 1), so.shape[0], int(first), _p(sc)) != 0:
            raise RuntimeError("cedar_amd_pcg_direction_many refused")

    def pcg_update_many(self, zmode, move, x, r, p, w, z, diag, first, sc, nrhs=None, active=None):
        """per item m: x += alpha_m p, r -= alpha_m w (move), r.r and r.z by zmode -> sc[m]; diag is shared"""
        assert all(a is None or a.shape == r.shape for a in (x, p, w, z)) and (diag is None or diag.shape == r.shape[1:])
        n, act = self._batch(r, sc, nrhs, active)
        grid = r.shape[1:]
        if lib.cedar_amd_pcg_update_many(n, act, int(zmode), int(move), _p(x), _p(r), _p(p), _p(w), _p(z), _p(diag),
                                         u(grid[-1]), u(grid[-2]), u(grid[0] if len(grid) == 3 else 1), int(first), _p(sc)) != 0:
            raise RuntimeError("cedar_amd_pcg_update_many refused")

    def pcg_dots_wz(self, r, z, w, first, sc):
        """flexible CG's dots after the preconditioner: r.r, r.z, w.z, beta = -((alpha w.z) / rho), rho = r.z -> sc"""
        assert all(a is None or a.shape == r.shape for a in (z, w)) and sc.size == 8
        if lib.cedar_amd_pcg_dots_wz(_p(r), _p(z), _p(w), *self._dims(r), int(first), _p(sc)) != 0:
            raise RuntimeError("cedar_amd_pcg_dots_wz refused")

    def pcg_dots_wz_many(self, r, z, w, first, sc, nrhs=None, active=None):
        """per item m: pcg_dots_wz -> sc[m]"""
        assert all(a is None or a.shape == r.shape for a in (z, w))
        n, act = self._batch(r, sc, nrhs, active)
        grid = r.shape[1:]
        if lib.cedar_amd_pcg_dots_wz_many(n, act, _p(r), _p(z), _p(w), u(grid[-1]), u(grid[-2]),
                                          u(grid[0] if len(grid) == 3 else 1), int(first), _p(sc)) != 0:
            raise RuntimeError("cedar_amd_pcg_dots_wz_many refused")

    def pcg_rank_scalars(self, which, zmode, gathered, world, stride, first, sc):
        """which 0: alpha from the ranks' sigma; 1: rho / beta from their r.r (and r.z); summed in rank order"""
        assert sc.size == 8 and gathered.size >= world * stride
        if lib.cedar_amd_pcg_rank_scalars(int(which), int(zmode), _p(gathered), int(world), int(stride), int(first), _p(sc)) != 0:
            raise RuntimeError("cedar_amd_pcg_rank_scalars refused")

    def pcg_ghost_shell(self, z, p, pn, first, sc, boxes):
        """pn = z + beta p (first: z) on boxes = [(i0, j0, k0, ni, nj, nk), ...]"""
        bx = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 6)
        assert len(z.shape) == 3 and sc.size == 8 and all(a is None or a.shape == z.shape for a in (p, pn))
        if lib.cedar_amd_pcg_ghost_shell(_p(z), _p(p), _p(pn), *self._dims(z), int(first), _p(sc),
                                         bx.ctypes.data_as(C.POINTER(C.c_int)), len(bx)) != 0:
            raise RuntimeError("cedar_amd_pcg_ghost_shell refused")

    def project_mean(self, v, nrhs=None, active=None):
        """v := v - mean_interior(v) (cedar_amd_project_mean).  nrhs None: v is one level vector; else v has shape
        (items,) + grid and the items of the bit mask active (default: all nrhs) are projected.  Returns the means
        (0 for an item outside active)"""
        grid = v.shape if nrhs is None else v.shape[1:]
        n = 1 if nrhs is None else int(nrhs)
        assert nrhs is None or v.shape[0] >= n
        mean = np.zeros(n)
        act = u((1 << n) - 1 if active is None else int(active))
        if lib.cedar_amd_project_mean(n, act, _p(v), u(grid[-1]), u(grid[-2]), u(grid[0] if len(grid) == 3 else 1),
                                      mean.ctypes.data) != 0:
            raise RuntimeError("cedar_amd_project_mean refused")
        return mean

    def l2(self, v):
        return l2norm(v)


# ---------------------------------------------------------------- handle API
lib.cedar_amd_solver_create.restype = C.c_void_p
lib.cedar_amd_solver_create.argtypes = [C.c_int, u, u, u, C.c_int, C.c_void_p, C.c_int, C.POINTER(Settings)]
lib.cedar_amd_solver_destroy.argtypes = [C.c_void_p]
lib.cedar_amd_solver_nlevels.argtypes = [C.c_void_p]
lib.cedar_amd_solver_level_dims.argtypes = [C.c_void_p, C.c_int, C.POINTER(u), C.POINTER(u), C.POINTER(u)]
lib.cedar_amd_solver_get.restype = C.c_size_t
lib.cedar_amd_solver_get.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_void_p]
lib.cedar_amd_solver_set.restype = C.c_size_t
lib.cedar_amd_solver_set.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_void_p]
lib.cedar_amd_solver_vcycle.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
lib.cedar_amd_solver_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
lib.cedar_amd_solver_time_vcycles.restype = C.c_float
lib.cedar_amd_solver_time_vcycles.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
lib.cedar_amd_solver_time_relax.restype = C.c_float
lib.cedar_amd_solver_time_relax.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
lib.cedar_amd_solver_time_op.restype = C.c_float
lib.cedar_amd_solver_time_op.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
lib.cedar_amd_gallery.argtypes = [C.c_int, C.c_void_p, C.c_void_p, u, u, u, C.c_void_p]
lib.cedar_amd_solver_create_many.restype = C.c_void_p
lib.cedar_amd_solver_create_many.argtypes = [C.c_int, u, u, u, C.c_int, C.c_void_p, C.c_int, C.POINTER(Settings), C.c_int]
lib.cedar_amd_solver_max_rhs.argtypes = [C.c_void_p]
lib.cedar_amd_solver_vcycle_many.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
lib.cedar_amd_solver_solve_many.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
lib.cedar_amd_solver_time_vcycles_many.restype = C.c_float
lib.cedar_amd_solver_time_vcycles_many.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
for _f in (lib.cedar_amd_relax3_gs_many, lib.cedar_amd_residual3_many, lib.cedar_amd_restrict3_many, lib.cedar_amd_interp_add3_many):
    _f.restype = C.c_int
lib.cedar_amd_solver_create_many_periodic.restype = C.c_void_p
lib.cedar_amd_solver_create_many_periodic.argtypes = lib.cedar_amd_solver_create_many.argtypes
lib.cedar_amd_solver_create_many_periodic2.restype = C.c_void_p
lib.cedar_amd_solver_create_many_periodic2.argtypes = [u, u, C.c_int, C.c_void_p, C.c_int, C.POINTER(Settings), C.c_int]
lib.cedar_amd_solver_create_semidefinite.restype = C.c_void_p
lib.cedar_amd_solver_create_semidefinite.argtypes = lib.cedar_amd_solver_create_many.argtypes
lib.cedar_amd_project_mean.restype = C.c_int
lib.cedar_amd_project_mean.argtypes = [C.c_int, C.c_uint, C.c_void_p, u, u, u, C.c_void_p]
for _f in (lib.cedar_amd_relax2_gs_periodic_many, lib.cedar_amd_restrict2_periodic_many, lib.cedar_amd_interp_add2_periodic_many,
           lib.cedar_amd_solve_cg2_periodic_many, lib.cedar_amd_pcg_direction2_periodic_many):
    _f.restype = C.c_int


def _vp(a):
    if a is None:
        return None
    if isinstance(a, DeviceArray):
        return a.ptr
    if hasattr(a, "data_ptr"):  # torch tensor (device or host), contiguous float64
        return a.data_ptr()
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data


GALLERY = {"poisson2": (0, 3), "diag_diffusion2": (1, 3), "fe2": (2, 5),
           "poisson3": (10, 4), "diag_diffusion3": (11, 4), "fe3": (12, 14)}


def gallery(name, n, params=None, with_rhs=True, device=True):
    """build a gallery operator (+ example rhs) in HBM; returns (so, b)"""
    which, nst = GALLERY[name]
    n = tuple(int(v) for v in n)
    g = tuple(v + 2 for v in n[::-1])
    mk = DeviceArray if device else (lambda s: np.zeros(s))
    so, b = mk((nst,) + g), (mk(g) if with_rhs else None)
    pp = None
    if params is not None:
        pp = (C.c_double * len(params))(*params)
    nx, ny = n[0], n[1]
    nz = n[2] if len(n) == 3 else 1
    lib.cedar_amd_gallery(which, _vp(so), _vp(b), nx, ny, nz, pp)
    return so, b


class PcgSettings(C.Structure):
    _fields_ = [("max_iter", C.c_int), ("tol", C.c_double), ("stop_test", C.c_int), ("precon", C.c_int),
                ("nmg_cycles", C.c_int)]


# BoxMG's numbering (src/{2d,3d}/ftn/BMG_PCG_parameters_f90.h)
PCG_STOP = {"abs_l2": 0, "rel_l2": 1, "abs_m": 2, "rel_m": 3}
PCG_PRECON = {"none": 1, "diag": 2, "mg": 3}
lib.cedar_amd_solver_pcg.restype = C.c_int
lib.cedar_amd_solver_pcg.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PcgSettings), C.c_void_p]
lib.cedar_amd_solver_precondition.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
lib.cedar_amd_solver_pcg_many.restype = C.c_int
lib.cedar_amd_solver_pcg_many.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(PcgSettings), C.c_void_p,
                                          C.POINTER(C.c_int)]
lib.cedar_amd_solver_fcg.restype = C.c_int
lib.cedar_amd_solver_fcg.argtypes = lib.cedar_amd_solver_pcg.argtypes
lib.cedar_amd_solver_fcg_many.restype = C.c_int
lib.cedar_amd_solver_fcg_many.argtypes = lib.cedar_amd_solver_pcg_many.argtypes
lib.cedar_amd_solver_fcg_periodic.restype = C.c_int
lib.cedar_amd_solver_fcg_periodic.argtypes = lib.cedar_amd_solver_pcg.argtypes
lib.cedar_amd_solver_fcg_periodic_many.restype = C.c_int
lib.cedar_amd_solver_fcg_periodic_many.argtypes = lib.cedar_amd_solver_pcg_many.argtypes
lib.cedar_amd_solver_fcg_semidefinite.restype = C.c_int
lib.cedar_amd_solver_fcg_semidefinite.argtypes = lib.cedar_amd_solver_pcg.argtypes
lib.cedar_amd_solver_fcg_semidefinite_many.restype = C.c_int
lib.cedar_amd_solver_fcg_semidefinite_many.argtypes = lib.cedar_amd_solver_pcg_many.argtypes
lib.cedar_amd_solver_use_fp32_operator.restype = C.c_int
lib.cedar_amd_solver_use_fp32_operator.argtypes = [C.c_void_p, C.c_int]
lib.cedar_amd_solver_use_fp32_operator_many.restype = C.c_int
lib.cedar_amd_solver_use_fp32_operator_many.argtypes = [C.c_void_p, C.c_int]
lib.cedar_amd_solver_use_fp32_operator_all.restype = C.c_int
lib.cedar_amd_solver_use_fp32_operator_all.argtypes = [C.c_void_p, C.c_int]
lib.cedar_amd_solver_use_fp32_operator_2d.restype = C.c_int
lib.cedar_amd_solver_use_fp32_operator_2d.argtypes = [C.c_void_p, C.c_int]
lib.cedar_amd_solver_use_fp32_operator_lines.restype = C.c_int
lib.cedar_amd_solver_use_fp32_operator_lines.argtypes = [C.c_void_p, C.c_int]
lib.cedar_amd_solver_fp32_levels.restype = C.c_int
lib.cedar_amd_solver_fp32_levels.argtypes = [C.c_void_p]
lib.cedar_amd_solver_use_fp32_interpolation.restype = C.c_int
lib.cedar_amd_solver_use_fp32_interpolation.argtypes = [C.c_void_p, C.c_int]
lib.cedar_amd_solver_fp32_interp_levels.restype = C.c_int
lib.cedar_amd_solver_fp32_interp_levels.argtypes = [C.c_void_p]
for _f in (lib.cedar_amd_restrict2_ci32, lib.cedar_amd_interp_add2_ci32, lib.cedar_amd_restrict3_ci32, lib.cedar_amd_interp_add3_ci32,
           lib.cedar_amd_restrict3_many_ci32, lib.cedar_amd_interp_add3_many_ci32):
    _f.restype = C.c_int


class Solver:
    """cedar::cdr2::solver / cdr3::solver on the device (include/cedar_amd.h, handle API)."""

    def __init__(self, so, relax="point", nrelax_pre=2, nrelax_post=1, num_levels=-1,
                 max_iter=10, tol=1e-8, min_coarse=3, share_operator=False, cycle="v", ibc=0, plane=None, max_rhs=1,
                 periodic_batch=False, periodic_batch2d=False, semidefinite=False):
        shp = so.shape
        self.nd = len(shp) - 1
        nst = shp[0]
        nx, ny = shp[-1] - 2, shp[-2] - 2
        nz = shp[1] - 2 if self.nd == 3 else 1
        self.shape = tuple(shp[1:])
        st = Settings(RELAX[relax], nrelax_pre, nrelax_post, num_levels, max_iter, tol, min_coarse,
                      {"v": 0, "f": 1}[cycle], ibc)
        plane_settings(st, plane)
        self.max_iter = max_iter
        self._so = so if share_operator else None  # keep the shared operator alive
        if semidefinite:
            # a singular operator whose null space is the constants -- pure Neumann, fully periodic; ibc keeps its meaning
            # (cedar_amd_solver_create_semidefinite); max_rhs > 1: a batch handle of the kind nd and ibc call for
            self.h = lib.cedar_amd_solver_create_semidefinite(self.nd, nx, ny, nz, nst, _vp(so), int(share_operator),
                                                              C.byref(st), int(max_rhs))
        elif periodic_batch2d:  # a periodic 2D handle with room for max_rhs right-hand sides (ibc = 0: as max_rhs alone)
            if self.nd != 2:
                raise ValueError("periodic_batch2d is for 2D operators; periodic_batch serves 3D")
            self.h = lib.cedar_amd_solver_create_many_periodic2(nx, ny, nst, _vp(so), int(share_operator), C.byref(st),
                                                                int(max_rhs))
        elif periodic_batch:  # a periodic 3D handle with room for max_rhs right-hand sides (ibc = 0: as max_rhs alone)
            self.h = lib.cedar_amd_solver_create_many_periodic(self.nd, nx, ny, nz, nst, _vp(so), int(share_operator),
                                                               C.byref(st), int(max_rhs))
        elif max_rhs == 1:
            self.h = lib.cedar_amd_solver_create(self.nd, nx, ny, nz, nst, _vp(so), int(share_operator), C.byref(st))
        else:  # room for max_rhs right-hand sides on every level (vcycle_many / solve_many)
            self.h = lib.cedar_amd_solver_create_many(self.nd, nx, ny, nz, nst, _vp(so), int(share_operator), C.byref(st),
                                                      int(max_rhs))
        if not self.h:
            raise RuntimeError("cedar_amd_solver_create failed")

    def max_rhs(self):
        return lib.cedar_amd_solver_max_rhs(self.h)

    def _nrhs(self, x, b):
        assert tuple(x.shape) == tuple(b.shape) and tuple(x.shape[1:]) == self.shape, (x.shape, b.shape, self.shape)
        return int(x.shape[0])

    def vcycle_many(self, x, b):
        """one cycle on every item of x, b of shape (nrhs,) + grid (cedar_amd_solver_vcycle_many); RuntimeError when
        the library refuses (x untouched)"""
        if lib.cedar_amd_solver_vcycle_many(self.h, self._nrhs(x, b), _vp(x), _vp(b)) != 0:
            raise RuntimeError("cedar_amd_solver_vcycle_many refused (see the printed reason)")

    def solve_many(self, b, x, rel=None):
        """multilevel::solve for the items of b, x of shape (nrhs,) + grid in lockstep (cedar_amd_solver_solve_many).
        Returns (rel, iters): rel a list of the items' histories cut to the cycles run, iters[m] the cycles after which
        item m first met tol.  rel: optional (nrhs, max_iter + 1) array the library writes into.  RuntimeError when the
        library refuses (x and rel untouched)."""
        nrhs = self._nrhs(x, b)
        if rel is None:
            rel = np.zeros((nrhs, self.max_iter + 1))
        assert rel.shape == (nrhs, self.max_iter + 1) and rel.dtype == np.float64 and rel.flags["C_CONTIGUOUS"]
        iters = np.zeros(nrhs, dtype=np.int32)
        n = lib.cedar_amd_solver_solve_many(self.h, nrhs, _vp(b), _vp(x), rel.ctypes.data, iters.ctypes.data_as(C.POINTER(C.c_int)))
        if n < 0:
            raise RuntimeError("cedar_amd_solver_solve_many refused (see the printed reason)")
        return [rel[m, : n + 1] for m in range(nrhs)], [int(v) for v in iters]

    def time_vcycles_many(self, x, b, n):
        """n cycles on the items of the DeviceArrays x, b of shape (nrhs,) + grid; elapsed ms"""
        ms = lib.cedar_amd_solver_time_vcycles_many(self.h, self._nrhs(x, b), x.ptr, b.ptr, n)
        if ms < 0:
            raise RuntimeError("cedar_amd_solver_time_vcycles_many refused (see the printed reason)")
        return ms

    def nlevels(self):
        return lib.cedar_amd_solver_nlevels(self.h)

    def dims(self, lvl):
        a, b, c = u(), u(), u()
        lib.cedar_amd_solver_level_dims(self.h, lvl, C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    def array(self, lvl, what):
        n = lib.cedar_amd_solver_get(self.h, lvl, what.encode(), None)
        if n == 0:
            return None
        out = np.empty(n)
        lib.cedar_amd_solver_get(self.h, lvl, what.encode(), out.ctypes.data)
        if what == "ABD":
            return out
        nx, ny, nz = self.dims(lvl)
        shp = (ny + 2, nx + 2) if self.nd == 2 else (nz + 2, ny + 2, nx + 2)
        return out.reshape((-1,) + shp)

    def set_array(self, lvl, what, a):
        """replace a set-up product of a level (cedar_amd_solver_set); a: numpy array of the product's full size"""
        a = np.ascontiguousarray(a, dtype=np.float64)
        n = lib.cedar_amd_solver_get(self.h, lvl, what.encode(), None)
        assert n == a.size, (what, lvl, n, a.size)
        assert lib.cedar_amd_solver_set(self.h, lvl, what.encode(), a.ctypes.data) == n

    def vcycle(self, x, b):
        lib.cedar_amd_solver_vcycle(self.h, _vp(x), _vp(b))

    def solve(self, b, x):
        rel = np.zeros(self.max_iter + 1)
        n = lib.cedar_amd_solver_solve(self.h, _vp(b), _vp(x), rel.ctypes.data)
        return rel[: n + 1]

    def _cg(self, call, b, x, max_iter, tol, stop, precon, nmg_cycles):
        ps = PcgSettings(int(max_iter), float(tol), PCG_STOP[stop], PCG_PRECON[precon], int(nmg_cycles))
        hist = np.zeros(max(int(max_iter), 0) + 1)
        n = getattr(lib, call)(self.h, _vp(b), _vp(x), C.byref(ps), hist.ctypes.data)
        if n < 0:
            raise RuntimeError(call + " refused the settings (see the printed reason)")
        return hist[: n + 1]

    def _cg_many(self, call, b, x, max_iter, tol, stop, precon, nmg_cycles, hist):
        nrhs = self._nrhs(x, b)
        ps = PcgSettings(int(max_iter), float(tol), PCG_STOP[stop], PCG_PRECON[precon], int(nmg_cycles))
        ld = max(int(max_iter), 0) + 1
        if hist is None:
            hist = np.zeros((nrhs, ld))
        assert hist.shape == (nrhs, ld) and hist.dtype == np.float64 and hist.flags["C_CONTIGUOUS"]
        iters = np.zeros(nrhs, dtype=np.int32)
        n = getattr(lib, call)(self.h, nrhs, _vp(b), _vp(x), C.byref(ps), hist.ctypes.data,
                               iters.ctypes.data_as(C.POINTER(C.c_int)))
        if n < 0:
            raise RuntimeError(call + " refused (see the printed reason)")
        return [hist[m, : int(iters[m]) + 1] for m in range(nrhs)], [int(v) for v in iters]

    def pcg(self, b, x, max_iter=50, tol=1e-8, stop="rel_l2", precon="mg", nmg_cycles=1):
        """conjugate gradients preconditioned by the cycle (cedar_amd_solver_pcg): x updated in place; returns the
        history [||r0||, ||r1||/||r0||, ...]; RuntimeError when the library refuses the settings (x untouched)"""
        return self._cg("cedar_amd_solver_pcg", b, x, max_iter, tol, stop, precon, nmg_cycles)

    def pcg_many(self, b, x, max_iter=50, tol=1e-8, stop="rel_l2", precon="mg", nmg_cycles=1, hist=None):
        """pcg for the items of b, x of shape (nrhs,) + grid in lockstep (cedar_amd_solver_pcg_many): an item that has
        stopped is left alone, so x[m] and its history are those of pcg on item m.  Returns (hist_rows, iters): row m cut
        to iters[m] + 1 entries.  hist: optional (nrhs, max_iter + 1) array the library writes into.  RuntimeError when
        the library refuses (x and hist untouched)."""
        return self._cg_many("cedar_amd_solver_pcg_many", b, x, max_iter, tol, stop, precon, nmg_cycles, hist)

    def fcg(self, b, x, max_iter=50, tol=1e-8, stop="rel_l2", precon="mg", nmg_cycles=1):
        """flexible conjugate gradients (cedar_amd_solver_fcg): pcg with the Polak-Ribiere beta, so any cycle of the
        handle may be the preconditioner -- V(m,n), F-cycles, plane relaxation.  Same arguments and return as pcg"""
        return self._cg("cedar_amd_solver_fcg", b, x, max_iter, tol, stop, precon, nmg_cycles)

    def fcg_periodic(self, b, x, max_iter=50, tol=1e-8, stop="rel_l2", precon="mg", nmg_cycles=1):
        """flexible conjugate gradients on a handle made with ibc != 0 (cedar_amd_solver_fcg_periodic): the operator pass
        wraps around in the periodic directions, the ghost layers of b and x do not matter and x comes back with the
        periodic image in its ghosts.  A handle with ibc = 0 is served by fcg.  Same arguments and return as pcg"""
        return self._cg("cedar_amd_solver_fcg_periodic", b, x, max_iter, tol, stop, precon, nmg_cycles)

    def fcg_many(self, b, x, max_iter=50, tol=1e-8, stop="rel_l2", precon="mg", nmg_cycles=1, hist=None):
        """fcg for the items of b, x in lockstep (cedar_amd_solver_fcg_many); same arguments and return as pcg_many"""
        return self._cg_many("cedar_amd_solver_fcg_many", b, x, max_iter, tol, stop, precon, nmg_cycles, hist)

    def fcg_periodic_many(self, b, x, max_iter=50, tol=1e-8, stop="rel_l2", precon="mg", nmg_cycles=1, hist=None):
        """fcg_periodic for the items of b, x in lockstep on a handle made with periodic_batch=True (3D) or
        periodic_batch2d=True (2D)
        (cedar_amd_solver_fcg_periodic_many); same arguments and return as fcg_many"""
        return self._cg_many("cedar_amd_solver_fcg_periodic_many", b, x, max_iter, tol, stop, precon, nmg_cycles, hist)

    def fcg_semidefinite(self, b, x, max_iter=50, tol=1e-8, stop="rel_l2", precon="mg", nmg_cycles=1):
        """flexible conjugate gradients on a handle made with semidefinite=True (cedar_amd_solver_fcg_semidefinite):
        solves A x = P b with mean(x) = 0, P v = v - mean_interior(v); b need not be compatible and is not written,
        hist[0] = |P (b - A x0)|; the cycle is applied as P M P.  Same arguments and return as pcg"""
        return self._cg("cedar_amd_solver_fcg_semidefinite", b, x, max_iter, tol, stop, precon, nmg_cycles)

    def fcg_semidefinite_many(self, b, x, max_iter=50, tol=1e-8, stop="rel_l2", precon="mg", nmg_cycles=1, hist=None):
        """fcg_semidefinite for the items of b, x in lockstep on a handle made with semidefinite=True and max_rhs > 1
        (cedar_amd_solver_fcg_semidefinite_many); same arguments and return as fcg_many"""
        return self._cg_many("cedar_amd_solver_fcg_semidefinite_many", b, x, max_iter, tol, stop, precon, nmg_cycles, hist)

    def precondition(self, z, r):
        """z = M^-1 r: one cycle from z = 0 (cedar_amd_solver_precondition)"""
        lib.cedar_amd_solver_precondition(self.h, _vp(z), _vp(r))

    def use_fp32_operator(self, min_rows=0):
        """keep the 27-point operator of the cycle in single precision on every smoothed level with at least min_rows
        rows (0: the default; cedar_amd_solver_use_fp32_operator).  Returns the number of levels that read a float copy,
        -1 when the library refuses (the reason is printed, the handle is unchanged)"""
        return lib.cedar_amd_solver_use_fp32_operator(self.h, int(min_rows))

    def use_fp32_operator_many(self, min_rows=0):
        """use_fp32_operator for a handle made with max_rhs > 1 (cedar_amd_solver_use_fp32_operator_many): the batched cycle
        of vcycle_many / solve_many / pcg_many then reads the float copies.  With max_rhs == 1 it is use_fp32_operator"""
        return lib.cedar_amd_solver_use_fp32_operator_many(self.h, int(min_rows))

    def use_fp32_operator_all(self, min_rows=0):
        """the switch for any 3D handle, a 7-point level 0 included (cedar_amd_solver_use_fp32_operator_all): min_rows > 0
        switches every smoothed level with at least that many rows; 0 takes the measured defaults (128 rows for either
        kind of level).  Returns the number of levels that read a float copy, -1 if refused"""
        return lib.cedar_amd_solver_use_fp32_operator_all(self.h, int(min_rows))

    def use_fp32_operator_2d(self, min_rows=0):
        """the switch for a 2D handle, single or batch, Dirichlet point relaxation (cedar_amd_solver_use_fp32_operator_2d):
        min_rows > 0 switches every smoothed level with at least that many rows, five- and nine-point alike; 0 takes the
        measured default (levels of at least 1024 rows).  Returns the number of levels that read a float copy, -1 if refused"""
        return lib.cedar_amd_solver_use_fp32_operator_2d(self.h, int(min_rows))

    def use_fp32_operator_lines(self, min_rows=0):
        """the switch for a 2D handle, single or batch, Dirichlet line relaxation (cedar_amd_solver_use_fp32_operator_lines):
        min_rows > 0 switches every smoothed level with at least that many rows that the small-level kernels do not serve
        (more than 64 x 64 unknowns); 0 takes the measured default.  Returns the number of levels that read float copies,
        -1 if refused"""
        return lib.cedar_amd_solver_use_fp32_operator_lines(self.h, int(min_rows))

    def fp32_levels(self):
        return lib.cedar_amd_solver_fp32_levels(self.h)

    def use_fp32_interpolation(self, min_rows=0):
        """keep the interpolation weights that the cycle's restriction and interpolation-and-add read in single precision
        (cedar_amd_solver_use_fp32_interpolation): every level pair whose fine level has at least min_rows rows (0: the
        default, 128 rows in 3D, 1024 in 2D) and is not served by the small-level kernels.  Independent of the
        use_fp32_operator* switches.  Returns the number of level pairs that read a float copy, -1 if refused (the reason
        is printed, the handle is unchanged)"""
        return lib.cedar_amd_solver_use_fp32_interpolation(self.h, int(min_rows))

    def fp32_interp_levels(self):
        return lib.cedar_amd_solver_fp32_interp_levels(self.h)

    def time_vcycles(self, x, b, n):
        return lib.cedar_amd_solver_time_vcycles(self.h, x.ptr, b.ptr, n)

    def time_relax(self, x, b, n):
        return lib.cedar_amd_solver_time_relax(self.h, x.ptr, b.ptr, n)

    def time_op(self, x, b, op, n):
        """n launches of a level-0 kernel: op 'residual' | 'restrict' | 'interp_add' (overwrites x); elapsed ms"""
        return lib.cedar_amd_solver_time_op(self.h, x.ptr, b.ptr, {"residual": 1, "restrict": 2, "interp_add": 3}[op], n)

    def close(self):
        if self.h:
            lib.cedar_amd_solver_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
