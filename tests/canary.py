"""The harness of the per-element GPU kernel tests (tests/test_gpu_elementwise_q.py and the eight modules after it): buffers
whose surroundings hold a NaN canary, the ledger that holds every comparison to its bound and keeps the module's table, and
the module-scoped device fixture.  tests/test_canary.py runs all of it on a host-memory stand-in for the device.

Every buffer class has ``base`` / ``span`` (address and bytes of its allocation), ``inside`` (the halfword mask of what the
kernels may write), ``stray()`` (positions outside the mask that no longer hold the canary), ``same()`` (an input still holds
the bits it was given) and ``numpy()``.  The layouts are part of what the tests assert -- offset, sample stride, piece stride,
guard and tail decide which alignment and vector paths a kernel takes -- so each family keeps its own arithmetic, as one
constructor of the shared class."""
import time

import numpy as np
import pytest

from tests.conv_s2_ref import FRONT, view_layout
from tests.elementwise_q_ref import (CANARY, PLANES, REL_L2, U, bits_equal, canary_changed, canary_fill, f32_inside, q_inside,
                                     rel, worst)

GUARD = 4 * FRONT                   # bytes of canary in front of and behind a Bytes buffer, a named View and a named QView
PATTERN2 = 0x4248                   # finite as bf16 (50), as fp16 (3.14) and, twice, as fp32 (50.07): what ``repaint`` writes


# ---- buffers ----
class View:
    """an fp32 [N, C, H, W] tensor ``el0`` elements into a canary-filled allocation of ``total`` elements, its samples
    ``nstride`` elements apart; ``t`` is the DevTensor, ``ptr`` the allocation"""
    unit = "halfword"

    def __init__(self, gpu, shape, layout, data=None):
        self.dev, _, D = gpu
        if len(shape) == 1:
            shape = (1, shape[0], 1, 1)
        N, C, H, W = shape
        el0, ns, self.total = layout
        self.ptr = self.base = self.dev.alloc(4 * self.total)
        self.span = 4 * self.total
        assert self.ptr % 16 == 0
        canary_fill(self.dev, self.ptr, self.span)
        self.t = D.DevTensor(self.dev, self.ptr + 4 * el0, shape, ns)
        self.inside = f32_inside(N, ns, el0, C * H * W, self.total)
        self.data = None
        if data is not None:
            self.set(data)

    @classmethod
    def free(cls, gpu, shape, spec=(0, 0), data=None):
        """``spec`` = (elements in front, elements between the samples); 8 elements behind the last sample"""
        chw = int(np.prod(shape[-3:]))
        ns = chw + spec[1]
        return cls(gpu, shape, (spec[0], ns, spec[0] + ((shape[0] if len(shape) == 4 else 1) - 1) * ns + chw + 8), data)

    @classmethod
    def named(cls, gpu, shape, view, data=None):
        """'whole' | 'slice' | 'offset' | 'off4' of tests/conv_s2_ref.py's view_layout: 4 KB of canary on both sides"""
        if len(shape) == 1:
            shape = (1, shape[0], 1, 1)
        el0, ns, total = view_layout(shape, view)
        assert el0 >= FRONT and total - (el0 + (shape[0] - 1) * ns + int(np.prod(shape[1:]))) >= FRONT
        return cls(gpu, shape, (el0, ns, total), data)

    @classmethod
    def framed(cls, gpu, shape, mode, data=None):
        """a channel slice of a tensor one channel wider on both sides ('slice'), or a contiguous tensor with a tail of one
        plane (four elements at least) behind it ('whole')"""
        N, C, H, W = shape
        HW = H * W
        if mode == 'slice':
            return cls(gpu, shape, (HW, (C + 2) * HW, N * (C + 2) * HW), data)
        assert mode == 'whole'
        return cls(gpu, shape, (0, C * HW, N * C * HW + max(HW, 4)), data)

    def set(self, data):
        self.data = np.ascontiguousarray(data, np.float32).reshape(self.t.shape).copy()
        self.t.set(self.data)
        return self

    def numpy(self):
        return self.t.numpy()

    def stray(self):
        return canary_changed(self.dev, self.base, self.span, self.inside)

    def same(self):
        return bits_equal(self.numpy(), np.reshape(self.data, self.t.shape))


class Bytes:
    """``nbytes`` of device memory, exactly, between two guards of 4 KB of canary in one allocation (``base``; the buffer is at
    ``ptr``): packed weights, masks, per-channel vectors, workspaces.  ``stray`` counts in bytes, so the odd byte behind a
    buffer of odd size is watched too"""
    unit = "byte"

    def __init__(self, gpu, nbytes, data=None, dtype=None):
        self.dev, self.D, self.dtype = gpu[0], gpu[2], dtype
        self.nbytes = int(nbytes)
        assert self.nbytes > 0
        self.total = self.span = 2 * GUARD + (self.nbytes + 1) // 2 * 2
        self.base = self.dev.alloc(self.total)
        canary_fill(self.dev, self.base, self.total)
        self.ptr = self.base + GUARD
        self.inside = np.zeros(self.total // 2, bool)
        self.inside[GUARD // 2:(GUARD + self.nbytes + 1) // 2] = True
        self.data = None
        if data is not None:
            self.set(data)

    @classmethod
    def rounded(cls, gpu, nbytes, data=None):
        """the size rounded up to 16 bytes (16 at least), the data taken as fp32"""
        return cls(gpu, (max(int(nbytes), 16) + 15) // 16 * 16, data, np.float32)

    t = property(lambda s: s.tensor((1, s.nbytes // 4, 1, 1)))

    def tensor(self, shape, offset=0):
        return self.D.DevTensor(self.dev, self.ptr + 4 * offset, shape)

    def set(self, data):
        self.data = np.ascontiguousarray(data, self.dtype).reshape(-1).view(np.uint8).copy()
        assert self.data.nbytes == self.nbytes, (self.data.nbytes, self.nbytes)
        self.dev.h2d(self.ptr, self.data)
        return self

    def bytes(self):
        out = np.empty(self.nbytes, np.uint8)
        self.dev.d2h(out, self.ptr, self.nbytes)
        return out

    def numpy(self):
        return self.bytes().view(np.float32)

    def snapshot(self):
        self.data = self.bytes()

    def stray(self):
        raw = np.empty(self.total, np.uint8)
        self.dev.d2h(raw, self.base, self.total)
        bad = raw != np.full(self.total // 2, CANARY, np.uint16).view(np.uint8)
        bad[GUARD:GUARD + self.nbytes] = False
        return np.flatnonzero(bad)

    def same(self):
        return np.array_equal(self.bytes(), self.data)

    def untouched(self):
        return np.array_equal(self.bytes(), np.full((self.nbytes + 1) // 2, CANARY, np.uint16).view(np.uint8)[:self.nbytes])


class QView:
    """a q tensor ``unit0`` 16-byte units into a canary-filled allocation of ``total_units``, its samples ``nstride`` units and
    its piece planes N * nstride units apart (the piece stride of the allocation, as the q outputs require); ``wide`` channels
    lie between two samples, the view being channels [c0, c0 + C) of them"""
    unit = "halfword"

    def __init__(self, gpu, shape, dtype, front, wide, c0, total_units):
        self.dev, _, D = gpu
        N, C, H, W = shape
        hw, self.planes = H * W, PLANES[dtype]
        ns = wide // 8 * hw
        self.total_units = total_units(self.planes * N * ns)
        self.ptr = self.base = self.dev.alloc(16 * self.total_units)
        self.span = 16 * self.total_units
        canary_fill(self.dev, self.ptr, self.span)
        whole = D.QTensor(self.dev, self.ptr + 16 * front, (N, wide, H, W), dtype)
        self.q = whole.channels(c0, c0 + C) if wide != C else whole
        self.inside = q_inside(self.planes, N, ns, N * ns, front + c0 // 8 * hw, C // 8 * hw, self.total_units)
        self.data = None

    @classmethod
    def named(cls, gpu, shape, dtype, view):
        """whole, a channel slice [8, 8 + C) of C + 16 channels, or starting one unit further in ('offset'); 4 KB of canary in
        front of the first plane and behind the last"""
        units = GUARD // 16
        front = units + (1 if view == 'offset' else 0)
        wide, c0 = (shape[1] + 16, 8) if view == 'slice' else (shape[1], 0)
        return cls(gpu, shape, dtype, front, wide, c0, lambda planes: front + planes + units)

    @classmethod
    def framed(cls, gpu, shape, dtype, mode):
        """a channel slice in the middle of a buffer 8 channels wider on both sides, or a whole allocation that ends after its
        last plane with a tail of one more plane's size behind it; no guard in front"""
        N, C, H, W = shape
        if mode == 'slice':
            return cls(gpu, shape, dtype, 0, C + 16, 8, lambda planes: planes)
        assert mode == 'whole'
        return cls(gpu, shape, dtype, 0, C, 0, lambda planes: planes + N * (C // 8) * H * W)

    def pieces(self):
        """the stored pieces as float32 arrays"""
        return [self.q.numpy(piece=p) for p in range(self.planes)]

    def raw(self):
        out = np.empty(8 * self.total_units, np.uint16)
        self.dev.d2h(out, self.ptr, out.nbytes)
        return out

    def snapshot(self):
        self.data = self.raw()

    def stray(self):
        return canary_changed(self.dev, self.base, self.span, self.inside)

    def same(self):
        return np.array_equal(self.raw(), self.data)


def repaint(dev, *bufs):
    """everything outside the views / buffers of these allocations becomes PATTERN2"""
    for o in bufs:
        raw = np.empty(o.span // 2, np.uint16)
        dev.d2h(raw, o.base, o.span)
        raw[~o.inside] = PATTERN2
        dev.h2d(o.base, raw)


def clean(what, *bufs):
    """no canary changed round any of these"""
    for i, v in enumerate(bufs):
        s = v.stray()
        assert s.size == 0, (what, "buffer %d: %d %ss outside it were written, first at %s %d of its allocation"
                             % (i, s.size, v.unit, v.unit, s[0] if s.size else -1))


def unchanged(what, *bufs):
    """``clean``, and every one of these inputs still holds, bit for bit, what it was given"""
    clean(what, *bufs)
    for i, v in enumerate(bufs):
        assert v.same(), (what, "input %d was modified" % i)


def fl32_sum(prev, inc):
    """fl32(previous + increment): what an accumulate form must give, bit for bit"""
    return (np.asarray(prev, np.float32) + np.asarray(inc, np.float32)).astype(np.float32)


# ---- the ledger ----
class Ledger:
    """one module's comparisons: ``measured`` {key: (worst k, worst rel-L2)} and ``count`` {key: comparisons}.

    bound      key -> k, for the calls that pass none
    rel_limit  a number, or key -> number: the limit of the second figure
    maxabs     key -> bool: the second figure is max |got - ref| / max |ref| there, not the rel-L2
    describe   (at, index, shape) -> the border / parity class of an element, for the failure messages; ``at`` is what the
               call passes (the kind, the geometry)
    line       (key, worst k, second figure, count) -> the key's line of the table
    order      measured -> the keys in the table's order;  header / footer: a line before the table, () -> a line after it"""

    def __init__(self, line, bound=None, rel_limit=REL_L2, maxabs=None, describe=None, order=sorted, header=None, footer=None):
        self.line, self.bound, self.rel_limit, self.maxabs, self.describe = line, bound, rel_limit, maxabs, describe
        self.order, self.header, self.footer = order, header, footer
        self.measured, self.count = {}, {}

    def tally(self, key, n=1):
        self.count[key] = self.count.get(key, 0) + n

    def record(self, key, w=0.0, r=0.0):
        old = self.measured.get(key, (0.0, 0.0))
        self.measured[key] = (max(old[0], w), max(old[1], r))
        self.tally(key)

    def _where(self, at, i, shape):
        return " (%s)" % self.describe(at, i, shape) if self.describe is not None and at is not None else ""

    def note(self, key, got, ref, M, what, k=None, at=None, rel_limit=True, record=True):
        """per element |got - ref| <= k 2^-24 M, the output finite, and the second figure within its limit; the figures are
        printed before they are asserted and kept for the table.  rel_limit: a number for this call, None to print and keep
        the second figure without a limit, False to leave it out (a reference that may cancel as a whole).  record False: the
        call counts, its figures stay out of the table (a bound widened for the call)"""
        name = key if isinstance(key, str) else " ".join(key)
        k = self.bound(key) if k is None else k
        got, ref, M = np.asarray(got), np.asarray(ref, np.float64), np.asarray(M, np.float64)
        assert got.shape == ref.shape, (name, what, got.shape, ref.shape)
        w, r, second = worst(got, ref, M), 0.0, ""
        if rel_limit is not False:
            if self.maxabs is not None and self.maxabs(key):
                r, second = float(np.abs(got - ref).max() / np.abs(ref).max()), "max-abs/scale"
            else:
                r, second = rel(got, ref), "rel-L2"
        if rel_limit is True:
            rel_limit = self.rel_limit(key) if callable(self.rel_limit) else self.rel_limit
        print("%s %s: worst k %.3f (bound %s)" % (name, what, w, k) + ("  %s %.2e" % (second, r) if second else ""))
        if record:
            self.record(key, w, r)
        else:
            self.tally(key)
        assert np.isfinite(got).all(), (name, what, "the output is not finite everywhere: %d elements" % (~np.isfinite(got)).sum())
        if w > k:
            err = np.abs(got.astype(np.float64) - ref) / (U * np.maximum(M, 1e-300))
            i = tuple(int(v) for v in np.unravel_index(np.argmax(np.where(got == ref, 0, err)), got.shape))
            pytest.fail("%s %s: element %s%s got %r ref %r: %.2f x 2^-24 M > k = %s"
                        % (name, what, i, self._where(at, i, got.shape), got[i], ref[i], w, k))
        if rel_limit is not None and rel_limit is not False:
            assert r <= rel_limit, (name, what, second, r)

    def exact(self, key, got, want, what, at=None, zero_sign=True):
        """bit for bit; zero_sign False: a zero of either sign is a zero (relu: the epilogues that fold it into a piece-wise
        linear slope return v * 0 = -0 for a negative v, the others max(v, 0) = +0)"""
        name = key if isinstance(key, str) else " ".join(key)
        self.record(key)
        got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
        assert got.shape == want.shape, (name, what, got.shape, want.shape)
        if not zero_sign:
            got, want = np.where(got == 0, np.float32(0), got), np.where(want == 0, np.float32(0), want)
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        if len(bad):
            i = tuple(int(v) for v in bad[0])
            pytest.fail("%s %s: %d of %d elements differ in bits, first at %s%s: got %r, expected %r"
                        % (name, what, len(bad), got.size, i, self._where(at, i, got.shape), got[i], want[i]))

    def table(self):
        if self.header is not None:
            print(self.header)
        for key in self.order(self.measured):
            print(self.line(key, *self.measured[key], self.count[key]))
        if self.footer is not None:
            print(self.footer())


# ---- fixtures ----
def cached(cache, key, fn, keep=None):
    """the float64 references, computed once per module; with ``keep`` the oldest leave (they can be tens of MB each)"""
    if key not in cache:
        cache[key] = fn()
        while keep is not None and len(cache) > keep:
            del cache[next(iter(cache))]
    return cache[key]


def fixtures(ledger=None, cache=None, loss_scale=False):
    """-> the module-scoped ``gpu`` fixture -- (dev, ops, the device module); no device is a failure, not a skip; when the
    module is done the device closes and, for a module with a ledger, ``cache`` empties and the ledger's table and the wall
    time are printed -- and the per-test ``mem`` fixture, which frees what a test allocated.  loss_scale: both leave no
    loss-scale state attached"""

    @pytest.fixture(scope="module")
    def gpu():
        from gan_heightmaps_amd import device
        if device.device_count() == 0:
            pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
        dev = device.Device(0)
        t0 = time.time()
        yield dev, device.Ops(dev), device
        if loss_scale:
            dev.set_loss_scale_state(None)
        dev.close()
        if ledger is not None:
            cache.clear()
            ledger.table()
            print("module wall time %.1f s" % (time.time() - t0))

    @pytest.fixture
    def mem(gpu):
        dev = gpu[0]
        before = set(dev._allocs)
        yield
        if loss_scale:
            dev.set_loss_scale_state(None)
        dev.sync()
        for p in set(dev._allocs) - before:
            dev.free(p)

    return gpu, mem
