"""Guard bands around the caller's arrays of one library call.

`Arena` lays the arrays of a call out in ONE allocation with a poisoned band before, between and after them, so that
  * a store outside an array lands in a band and `check()` finds it (array name, before/after, distance);
  * a value consumed from outside an array is poison, not the zero or the plausible stale number that fresh device
    memory and recycled pool blocks hold, so the result differs from the same call on plain arrays;
  * with placement "dev8" every array starts at an odd element offset of a 256-byte aligned block: 8-byte aligned
    only, the side of the library's alignment dispatch that pointers from the allocator never reach.

Two poisons, every case runs with both: a quiet NaN with a recognisable payload poisons every arithmetic result it
meets but is dropped by a comparison (`max`, `ajj > 0`, `bbd != 0`); the finite 2**1000 survives those.

What the bands cannot see: a load whose value a select then drops (the result is the same with any poison), and the
library's own scratch (its partial-sum slabs carry their own NaN fill, NanSlab).
"""
import numpy as np

POISON_NAN = 0x7FF8DEADBEEF0001
POISON_BIG = int(np.array([2.0 ** 1000]).view(np.uint64)[0])
POISONS = {"nan": POISON_NAN, "big": POISON_BIG}
PLACEMENTS = ("host", "dev16", "dev8")
MIN_BAND = 64


def band_need(shape, nd):
    """doubles a band next to an array of this shape must hold: two rows plus two elements in 2D, one plane plus one row
    plus two elements in 3D (a one-dimensional array counts as one row)"""
    shape = tuple(int(s) for s in shape)
    row = shape[-1]
    if nd == 2 or len(shape) < 2:
        return 2 * row + 2
    return shape[-2] * row + row + 2


_VIEW = None


def device_view(ptr, shape):
    """a window of a device allocation that someone else owns: an instance of a subclass of capi.DeviceArray (made on
    first use, so that this module imports without the library), which capi._p / capi._vp and every Kernels and Solver
    method take as a DeviceArray"""
    global _VIEW
    if _VIEW is None:
        from cedar_amd import capi

        class View(capi.DeviceArray):
            def __init__(self, ptr, shape):
                self.shape = tuple(int(s) for s in shape)
                self.size = int(np.prod(self.shape))
                self.ptr = ptr

            def free(self):  # the owner frees the memory
                pass

        _VIEW = View
    return _VIEW(ptr, shape)


class Arena:
    """specs: [(name, shape), ...]; poison: a uint64 bit pattern (POISONS); placement: "host" | "dev16" | "dev8" (PLACEMENTS,
    what the GPU tests run) or "host8", the odd element offsets of "dev8" in a numpy buffer (the CPU statement test);
    nd: 2 or 3, the dimension of the grids the arrays hold (decides the band width)"""

    def __init__(self, specs, poison, placement, nd=2):
        assert placement in PLACEMENTS + ("host8",) and nd in (2, 3)
        self.placement, self.poison, self.nd = placement, np.uint64(poison), nd
        self.names = [n for n, _ in specs]
        self.shapes = {n: tuple(int(s) for s in shp) for n, shp in specs}
        assert len(set(self.names)) == len(self.names)
        parity = 1 if placement in ("dev8", "host8") else 0
        need = [band_need(self.shapes[n], nd) for n in self.names]
        self.start, self.stop = {}, {}
        pos = 0
        for i, n in enumerate(self.names):
            band = max(MIN_BAND, need[i], need[i - 1] if i else 0)
            pos += band
            pos += (pos & 1) ^ parity  # even element offset: 16-byte aligned; odd: 8-byte aligned only
            self.start[n] = pos
            pos += int(np.prod(self.shapes[n]))
            self.stop[n] = pos
        self.total = pos + max(MIN_BAND, need[-1]) + 1
        self.total += self.total & 1
        self.buf = np.empty(self.total, dtype=np.float64)
        self.bits = self.buf.view(np.uint64)
        self.bits[:] = self.poison
        self.is_band = np.ones(self.total, dtype=bool)
        for n in self.names:
            self.is_band[self.start[n]:self.stop[n]] = False
        self.dev = None
        self.views = {}
        if placement in ("host", "host8"):
            for n in self.names:
                self.views[n] = self.buf[self.start[n]:self.stop[n]].reshape(self.shapes[n])
                assert self.views[n].flags["C_CONTIGUOUS"] and self.views[n].base is not None
        else:
            from cedar_amd import capi
            self.dev = capi.DeviceArray((self.total,))
            assert self.dev.ptr % 256 == 0, "the allocator's blocks are 256-byte aligned"
            self.dev.upload(self.buf)
            for n in self.names:
                ptr = self.dev.ptr + 8 * self.start[n]
                assert ptr % 16 == (8 if placement == "dev8" else 0)
                self.views[n] = device_view(ptr, self.shapes[n])

    def __getitem__(self, name):
        return self.views[name]

    def fill(self, name, a):
        """the array's initial content"""
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert a.shape == self.shapes[name], (name, a.shape, self.shapes[name])
        if self.dev is None:
            self.views[name][...] = a
        else:
            self.views[name].upload(a)

    def download(self):
        """one copy of the whole allocation (device placements); the host buffer is its own copy"""
        if self.dev is not None:
            self.buf[:] = self.dev.numpy()
        return self.buf

    def array(self, name):
        """the array as of the last download (a copy)"""
        return self.buf[self.start[name]:self.stop[name]].reshape(self.shapes[name]).copy()

    def clobbered(self):
        """None, or (name, "before" | "after", distance, count) of the first band element that lost its poison"""
        bad = np.flatnonzero(self.is_band & (self.bits != self.poison))
        if bad.size == 0:
            return None
        p = int(bad[0])
        best = None
        for n in self.names:
            for side, d in (("before", self.start[n] - p), ("after", p - self.stop[n] + 1)):
                if d >= 1 and (best is None or d < best[2]):
                    best = (n, side, d)
        return best + (int(bad.size),)

    def check(self):
        """downloads once; AssertionError naming the first clobbered band element"""
        self.download()
        c = self.clobbered()
        if c is not None:
            p = self.start[c[0]] - c[2] if c[1] == "before" else self.stop[c[0]] + c[2] - 1
            raise AssertionError(f"guard band clobbered: {c[2]} element(s) {c[1]} array '{c[0]}' ({c[3]} band elements in all, "
                                 f"first holds {int(self.bits[p]):#018x}, {self.placement})")

    def close(self):
        if self.dev is not None:
            self.dev.free()
            self.dev = None


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class GuardedImpl:
    """wraps a host implementation object (the oracle): every call's numpy array arguments are placed in one host
    arena ("host" or "host8"), the call runs on the views, the bands are checked and the arrays copied back -- so the
    case suites of tests/cases.py run unchanged between guard bands.  A method whose name ends in 2 (or holds '2_')
    works on 2D grids, any other on 3D grids."""

    def __init__(self, impl, poison, placement="host"):
        assert placement in ("host", "host8")
        self.impl, self.poison, self.placement = impl, poison, placement
        self.calls = 0

    @staticmethod
    def _nd(name):
        return 2 if name.endswith("2") or "2_" in name else 3

    def __getattr__(self, name):
        f = getattr(self.impl, name)

        def call(*args, **kw):
            idx = [i for i, a in enumerate(args) if isinstance(a, np.ndarray)]
            if not idx:
                return f(*args, **kw)
            uniq = []
            for i in idx:  # the same array passed twice is one array
                if not any(args[i] is args[j] for j in uniq):
                    uniq.append(i)
            ar = Arena([(f"arg{i}", args[i].shape) for i in uniq], self.poison, self.placement, self._nd(name))
            try:
                for i in uniq:
                    ar.fill(f"arg{i}", args[i])
                new = list(args)
                for i in idx:
                    j = next(j for j in uniq if args[j] is args[i])
                    new[i] = ar[f"arg{j}"]
                rc = f(*new, **kw)
                try:
                    ar.check()
                except AssertionError as e:
                    raise AssertionError(f"{name}: {e}") from None
                for i in uniq:
                    args[i][...] = ar.array(f"arg{i}")
                self.calls += 1
                return rc
            finally:
                ar.close()

        return call
