"""Device context and tensors over libghm.so (thin, explicit; no torch)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import ConvDesc, call

ACT_CODES = {'linear': 0, 'relu': 1, 'lrelu': 2, 'sigmoid': 3, 'tanh': 4}
DTYPE_CODES = {'f32': 0, 'bf16': 1, 'f16': 2}       # GHM_DTYPE_* (include/ghm.h)
# 'bf16x3': fp32 arithmetic on the bf16 matrix cores by operand splitting (csrc/conv_split.hip) -- a host-side name: Ops
# routes the *_lp / *_lp_q calls made with it to the ghm_*_split entry points, and a QTensor of this dtype is three planes
SPLIT = 'bf16x3'
DTYPE_CODES[SPLIT] = 3     # understood by the q-epilogue producers (csrc/elementwise_q.hip) only
# 'bf16x2': the same machinery with TWO pieces per operand and three products (x0 w0 + x1 w0 + x0 w1): 16-bit operands at half
# the matrix-core time of 'bf16x3' -- BASELINE config 4's arithmetic (plain bf16 operands miss north_star's 1e-3 on the outputs)
SPLIT2 = 'bf16x2'
DTYPE_CODES[SPLIT2] = 4
SPLITS = {SPLIT: 3, SPLIT2: 2}     # split dtypes -> pieces per operand (the ``pieces`` argument of the ghm_*_split entry points)


def device_count():
    n = C.c_int32(0)
    call("ghm_device_count", C.byref(n))
    return n.value


class DevTensor:
    """fp32 [N, C, H, W] view in HBM with an explicit sample stride (elements)."""
    __slots__ = ("dev", "ptr", "shape", "nstride", "base")

    def __init__(self, dev, ptr, shape, nstride=None, base=None):
        self.dev = dev
        self.ptr = int(ptr)
        shape = tuple(int(s) for s in shape)
        if len(shape) == 2:
            shape = (shape[0], shape[1], 1, 1)
        assert len(shape) == 4
        self.shape = shape
        self.nstride = int(nstride) if nstride is not None else shape[1] * shape[2] * shape[3]
        self.base = base

    N = property(lambda s: s.shape[0])
    Cc = property(lambda s: s.shape[1])
    H = property(lambda s: s.shape[2])
    W = property(lambda s: s.shape[3])
    HW = property(lambda s: s.shape[2] * s.shape[3])
    size = property(lambda s: s.shape[0] * s.shape[1] * s.shape[2] * s.shape[3])
    contiguous = property(lambda s: s.nstride == s.shape[1] * s.shape[2] * s.shape[3])

    def channels(self, c0, c1):
        """View of channels [c0, c1) (ConcatLayer axis=1 without a copy)."""
        assert 0 <= c0 < c1 <= self.shape[1]
        return DevTensor(self.dev, self.ptr + 4 * c0 * self.HW, (self.N, c1 - c0, self.H, self.W), self.nstride,
                         self.base if self.base is not None else self)

    def samples(self, n0, n1):
        assert 0 <= n0 < n1 <= self.shape[0]
        return DevTensor(self.dev, self.ptr + 4 * n0 * self.nstride, (n1 - n0,) + self.shape[1:], self.nstride,
                         self.base if self.base is not None else self)

    def reshape(self, shape):
        assert self.contiguous
        t = DevTensor(self.dev, self.ptr, shape, None, self.base if self.base is not None else self)
        assert t.size == self.size
        return t

    def numpy(self):
        n, c, h, w = self.shape
        out = np.empty(self.shape, np.float32)
        if self.contiguous:
            self.dev.d2h(out, self.ptr, out.nbytes)
        else:
            for i in range(n):
                self.dev.d2h(out[i], self.ptr + 4 * i * self.nstride, out[i].nbytes)
        return out

    def set(self, arr):
        arr = np.ascontiguousarray(arr, np.float32).reshape(self.shape)
        if self.contiguous:
            self.dev.h2d(self.ptr, arr)
        else:
            for i in range(self.N):
                self.dev.h2d(self.ptr + 4 * i * self.nstride, arr[i])
        return self


class QTensor:
    """bf16 / fp16 copy of a [N, C, H, W] tensor in HBM in the channel-block-of-8 layout of include/ghm.h ("q tensor"):
    16-byte units = 8 channels of one pixel; ``nstride`` counts UNITS between samples, so a channel slice (multiple of 8)
    of a wider buffer is a view."""
    __slots__ = ("dev", "ptr", "shape", "nstride", "dtype", "base", "pstride")

    def __init__(self, dev, ptr, shape, dtype, nstride=None, base=None, pstride=None):
        self.dev, self.ptr, self.dtype, self.base = dev, int(ptr), dtype, base
        self.shape = tuple(int(v) for v in shape)
        assert len(self.shape) == 4 and self.shape[1] % 8 == 0, self.shape
        self.nstride = int(nstride) if nstride is not None else self.shape[1] // 8 * self.shape[2] * self.shape[3]
        # 'bf16x3' (split fp32): units between the three piece planes -- a property of the allocation, kept by every view
        self.pstride = int(pstride) if pstride is not None else self.shape[0] * self.nstride

    N = property(lambda s: s.shape[0])
    Cc = property(lambda s: s.shape[1])
    H = property(lambda s: s.shape[2])
    W = property(lambda s: s.shape[3])
    HW = property(lambda s: s.shape[2] * s.shape[3])
    contiguous = property(lambda s: s.nstride == s.shape[1] // 8 * s.shape[2] * s.shape[3])
    nbytes = property(lambda s: 16 * s.nstride * s.shape[0])

    @staticmethod
    def empty(dev, shape, dtype):
        shape = tuple(int(v) for v in shape)
        planes = SPLITS.get(dtype, 1)
        return QTensor(dev, dev.alloc(planes * 16 * shape[0] * (shape[1] // 8) * shape[2] * shape[3]), shape, dtype)

    def channels(self, c0, c1):
        assert 0 <= c0 < c1 <= self.shape[1] and c0 % 8 == 0 and (c1 - c0) % 8 == 0
        return QTensor(self.dev, self.ptr + 16 * (c0 // 8) * self.HW, (self.N, c1 - c0, self.H, self.W), self.dtype,
                       self.nstride, self.base if self.base is not None else self, self.pstride)

    def samples(self, n0, n1):
        assert 0 <= n0 < n1 <= self.shape[0]
        return QTensor(self.dev, self.ptr + 16 * n0 * self.nstride, (n1 - n0,) + self.shape[1:], self.dtype, self.nstride,
                       self.base if self.base is not None else self, self.pstride)

    def reshape(self, shape):
        """[N, 4K, H, W] <-> [4N, K, H, W] (the parity-planar view of the collapsed up-sample convolutions)"""
        assert self.contiguous
        t = QTensor(self.dev, self.ptr, shape, self.dtype, None, self.base if self.base is not None else self, self.pstride)
        assert t.nbytes == self.nbytes
        return t

    def numpy(self, piece=None):
        """-> float32 [N, C, H, W] (the exact values of the stored halfwords); 'bf16x3': the sum of the three pieces (in
        float64, rounded once: the fp32 value that was split), or one piece"""
        if self.dtype in SPLITS and piece is None:
            return sum(self.numpy(p).astype(np.float64) for p in range(SPLITS[self.dtype])).astype(np.float32)
        raw = np.empty((self.N, self.Cc * self.HW), np.uint16)       # a sample's channel blocks are contiguous planes
        for n in range(self.N):
            self.dev.d2h(raw[n], self.ptr + 16 * ((piece or 0) * self.pstride + n * self.nstride), raw[n].nbytes)
        raw = raw.reshape(self.N, self.Cc // 8, self.HW, 8).transpose(0, 1, 3, 2)
        raw = np.ascontiguousarray(raw).reshape(self.shape)
        if self.dtype == 'bf16' or self.dtype in SPLITS:
            return (raw.astype(np.uint32) << 16).view(np.float32)
        return raw.view(np.float16).astype(np.float32)


class PinnedArray:
    """page-locked host memory seen as a numpy array (ghm_host_alloc): the source of asynchronous uploads"""

    def __init__(self, shape, dtype=np.float32):
        self.shape = tuple(int(s) for s in shape)
        dt = np.dtype(dtype)
        n = int(np.prod(self.shape))
        p = C.c_void_p()
        call("ghm_host_alloc", max(n * dt.itemsize, 16), C.byref(p))
        self.ptr = p.value
        raw = np.ctypeslib.as_array(C.cast(C.c_void_p(self.ptr), C.POINTER(C.c_uint8)), shape=(max(n * dt.itemsize, 16),))
        self.array = raw[:n * dt.itemsize].view(dt).reshape(self.shape)

    def close(self):
        if self.ptr:
            self.array = None
            call("ghm_host_free", C.c_void_p(self.ptr))
            self.ptr = None


class Device:
    def __init__(self, index=0):
        _lib.load()
        h = C.c_void_p()
        call("ghm_ctx_create", int(index), C.byref(h))
        self.h = h
        self.index = index
        self._allocs = {}
        self.bytes_allocated = 0

    @classmethod
    def with_priority(cls, index, priority):
        """a context whose stream has the given HIP priority (negative = more urgent)"""
        self = cls.__new__(cls)
        _lib.load()
        h = C.c_void_p()
        call("ghm_ctx_create_prio", int(index), int(priority), C.byref(h))
        self.h, self.index, self._allocs, self.bytes_allocated = h, index, {}, 0
        return self

    # ---- memory ----
    def alloc(self, nbytes):
        p = C.c_void_p()
        call("ghm_alloc", self.h, int(max(nbytes, 16)), C.byref(p))
        self._allocs[p.value] = nbytes
        self.bytes_allocated += nbytes
        return p.value

    def free(self, ptr):
        if ptr in self._allocs:
            self.bytes_allocated -= self._allocs.pop(ptr)
            call("ghm_free", self.h, C.c_void_p(ptr))

    def empty(self, shape):
        shape = tuple(int(s) for s in shape)
        n = int(np.prod(shape)) if len(shape) else 1
        return DevTensor(self, self.alloc(4 * n), shape if len(shape) in (2, 4) else (1, n, 1, 1))

    def zeros(self, shape):
        t = self.empty(shape)
        self.memset_zero(t.ptr, 4 * t.size)
        return t

    def tensor(self, arr):
        arr = np.ascontiguousarray(arr, np.float32)
        shape = arr.shape
        if arr.ndim == 1:
            shape = (1, arr.shape[0], 1, 1)
        elif arr.ndim == 0:
            shape = (1, 1, 1, 1)
        elif arr.ndim == 3:
            shape = (1,) + arr.shape
        t = self.empty(shape)
        self.h2d(t.ptr, arr)
        return t

    def h2d(self, ptr, arr):
        arr = np.ascontiguousarray(arr)
        call("ghm_h2d", self.h, C.c_void_p(ptr), arr.ctypes.data_as(C.c_void_p), arr.nbytes)

    def queue_interference(self, other, probe, spin_us=1500):
        """microseconds a trivial kernel on ``other`` needs to finish while THIS context's stream sits in a wait for a
        ~spin_us spin kernel on ``probe``: ~spin_us if the two streams share a hardware queue, a few microseconds if not"""
        us = C.c_float()
        call("ghm_queue_interference", self.h, other.h, probe.h, int(spin_us), C.byref(us))
        return us.value

    def event_create(self):
        e = C.c_void_p()
        call("ghm_event_create", self.h, C.byref(e))
        return e

    def event_record(self, ev):
        call("ghm_event_record", self.h, ev)

    def event_wait(self, ev):
        """later work on this context's stream waits for the point ``ev`` marks (on whichever stream it was recorded)"""
        call("ghm_event_wait", self.h, ev)

    @staticmethod
    def event_sync(ev):
        call("ghm_event_sync", ev)

    @staticmethod
    def event_destroy(ev):
        call("ghm_event_destroy", ev)

    def h2d_async(self, ptr, pinned, nbytes=None):
        """copy a PinnedArray (its first ``nbytes``) to the device, ordered on this context's stream, without waiting for it"""
        n = pinned.array.nbytes if nbytes is None else int(nbytes)
        assert n <= pinned.array.nbytes
        call("ghm_h2d_async", self.h, C.c_void_p(ptr), C.c_void_p(pinned.ptr), n)

    def d2h_async(self, pinned, ptr, nbytes):
        """copy ``nbytes`` from the device into a PinnedArray, ordered on this context's stream, without waiting for it
        (read the array only after an event recorded behind the copy has passed)"""
        assert int(nbytes) <= pinned.array.nbytes
        call("ghm_d2h_async", self.h, C.c_void_p(pinned.ptr), C.c_void_p(ptr), int(nbytes))

    def d2h(self, arr, ptr, nbytes):
        assert arr.flags['C_CONTIGUOUS']
        call("ghm_d2h", self.h, arr.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), int(nbytes))

    def d2d(self, dst, src, nbytes):
        call("ghm_d2d", self.h, C.c_void_p(dst), C.c_void_p(src), int(nbytes))

    def memset_zero(self, ptr, nbytes):
        call("ghm_memset_zero", self.h, C.c_void_p(ptr), int(nbytes))

    def sync(self):
        call("ghm_sync", self.h)

    def scratch_info(self):
        """(bytes of the library workspace, bytes of retired blocks, recorded steps / graphs pinning them)"""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int32()
        call("ghm_scratch_info", self.h, C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    def set_loss_scale_state(self, state):
        """attach (DevTensor of 8 floats) / detach (None) the dynamic loss-scale state of this context"""
        call("ghm_set_loss_scale_state", self.h, _vp(state))

    def wait_for(self, other):
        """later work on this context's stream waits for everything already enqueued on ``other``'s stream"""
        call("ghm_stream_wait", self.h, other.h)

    def info(self):
        name = C.create_string_buffer(256)
        cu, hbm = C.c_int32(), C.c_int64()
        call("ghm_device_info", self.h, name, 256, C.byref(cu), C.byref(hbm))
        return {"name": name.value.decode(), "num_cu": cu.value, "hbm_bytes": hbm.value}

    # ---- graph capture / timers ----
    def capture_begin(self):
        call("ghm_capture_begin", self.h)

    def capture_end(self):
        g = C.c_void_p()
        call("ghm_capture_end", self.h, C.byref(g))
        return g

    def graph_launch(self, g):
        call("ghm_graph_launch", self.h, g)

    def graph_destroy(self, g):
        call("ghm_graph_destroy", g)

    @staticmethod
    def step_build(stages):
        """stages: [(Device, graph handle)] -> step handle: ghm_step_run launches every stage graph in one call"""
        n = len(stages)
        ctxs = (C.c_void_p * n)(*[d.h for d, _ in stages])
        graphs = (C.c_void_p * n)(*[g for _, g in stages])
        st = C.c_void_p()
        call("ghm_step_build", n, ctxs, graphs, C.byref(st))
        return st

    @staticmethod
    def step_record_begin(devs):
        """every operation issued on ``devs`` from now on is appended to the returned step instead of being executed
        (ghm_step_record_begin); end with step_record_end, replay with step_run"""
        n = len(devs)
        ctxs = (C.c_void_p * n)(*[d.h for d in devs])
        st = C.c_void_p()
        call("ghm_step_record_begin", n, ctxs, C.byref(st))
        return st

    @staticmethod
    def step_record_end(st):
        call("ghm_step_record_end", st)

    @staticmethod
    def step_timer_stride(st, stride):
        call("ghm_step_timer_stride", st, int(stride))

    @staticmethod
    def step_run(st):
        call("ghm_step_run", st)

    @staticmethod
    def step_destroy(st):
        call("ghm_step_destroy", st)

    def timer_start(self, slot=0):
        call("ghm_timer_start", self.h, slot)

    def timer_stop(self, slot=0):
        call("ghm_timer_stop", self.h, slot)

    def timer_ms(self, slot=0):
        ms = C.c_float()
        call("ghm_timer_elapsed_ms", self.h, slot, C.byref(ms))
        return ms.value

    def close(self):
        if self.h is not None:
            for p in list(self._allocs):
                self.free(p)
            call("ghm_ctx_destroy", self.h)
            self.h = None


# ---- weight layout (include/ghm.h): wp[c][a*kw+b][k] = W[k][c][kh-1-a][kw-1-b] -------------------

def pack_conv_w(W):
    """lasagne Conv2DLayer W[K, C, kh, kw] (or Deconv2DLayer W[Cin=K, Cout=C, kh, kw]) -> packed [C, kh*kw, K]."""
    K, Cc, kh, kw = W.shape
    return np.ascontiguousarray(W[:, :, ::-1, ::-1].transpose(1, 2, 3, 0)).reshape(Cc, kh * kw, K).astype(np.float32)


def unpack_conv_w(wp, K, Cc, kh, kw):
    return np.ascontiguousarray(np.asarray(wp).reshape(Cc, kh, kw, K).transpose(3, 0, 1, 2)[:, :, ::-1, ::-1])


def conv_desc(N, Cc, H, W, K, kh, kw, stride, pad, x_nstride=None, y_nstride=None):
    Ho = (H + 2 * pad - kh) // stride + 1
    Wo = (W + 2 * pad - kw) // stride + 1
    return ConvDesc(N, Cc, H, W, K, Ho, Wo, kh, kw, stride, pad,
                    x_nstride if x_nstride is not None else Cc * H * W,
                    y_nstride if y_nstride is not None else K * Ho * Wo)


# rule ids of ghm_opt_update (GHM_OPT_* in include/ghm.h)
OPT_RULES = {'sgd': 0, 'momentum': 1, 'nesterov_momentum': 2, 'adagrad': 3, 'adadelta': 4, 'adamax': 5, 'amsgrad': 6}


class WorldTile(C.Structure):
    """ghm_world_tile (include/ghm.h)"""
    _fields_ = [("chunk", C.c_void_p * 4), ("y0", C.c_int32), ("x0", C.c_int32)]


class MaxMip:
    """the maximum pyramid of one scene (Ops.render_maxmip): the device buffer and the size it was built for"""
    __slots__ = ("ptr", "H", "W", "elems")

    def __init__(self, ptr, H, W, elems):
        self.ptr, self.H, self.W, self.elems = ptr, H, W, elems


def render_params(pos, yaw, pitch, fov, size, height_scale, step, max_dist, sun_azimuth, sun_elevation, shadows, softness,
                  ambient, haze, horizon, zenith, accel=True, out_u8=False):
    """a ghm_render_params (include/ghm.h); pos is the scene-local (y, x, z)"""
    p = _lib.RenderParams()
    p.pos[:] = [float(v) for v in pos]
    p.yaw, p.pitch, p.fov = float(yaw), float(pitch), float(fov)
    p.Hi, p.Wi = int(size[0]), int(size[1])
    p.height_scale, p.step, p.max_dist = float(height_scale), float(step), float(max_dist)
    p.sun_azimuth, p.sun_elevation = float(sun_azimuth), float(sun_elevation)
    p.shadows, p.softness, p.ambient, p.haze = int(bool(shadows)), float(softness), float(ambient), float(haze)
    p.horizon[:] = [float(v) for v in horizon]
    p.zenith[:] = [float(v) for v in zenith]
    p.accel, p.out_u8 = int(bool(accel)), int(bool(out_u8))
    return p


EROSION_PLANES = 7                 # GHM_EROSION_PLANES (include/ghm.h): b, d, s, fL, fR, fT, fB


def erosion_params(**kw):
    """a ghm_erosion_params (include/ghm.h) from its twelve fields by name"""
    p = _lib.ErosionParams()
    for k, _ in p._fields_:
        setattr(p, k, float(kw.pop(k)))
    if kw:
        raise TypeError("unknown erosion parameters: %s" % sorted(kw))
    return p


def _vp(x):
    if x is None:
        return C.c_void_p(0)
    if isinstance(x, DevTensor):
        return C.c_void_p(x.ptr)
    return C.c_void_p(int(x))


class Ops:
    """Python spellings of the C-ABI ops on DevTensors (each is one asynchronous call)."""

    def __init__(self, dev):
        self.dev = dev
        self.h = dev.h

    def conv2d_fwd(self, d, x, wp, bias, y, act='linear', alpha=0.0, accumulate=False):
        call("ghm_conv2d_fwd", self.h, C.byref(d), _vp(x), _vp(wp), _vp(bias), _vp(y), ACT_CODES[act], alpha,
             int(accumulate))

    def conv2d_dgrad(self, d, dy, wp, dx, bias=None, act='linear', alpha=0.0, accumulate=False):
        call("ghm_conv2d_dgrad", self.h, C.byref(d), _vp(dy), _vp(wp), _vp(bias), _vp(dx), ACT_CODES[act], alpha,
             int(accumulate))

    def dgrad_t_supported(self, d):
        return bool(_lib.load().ghm_dgrad_t_supported(C.byref(d)))

    def transpose_weights(self, d, wp, wpT):
        call("ghm_conv2d_transpose_weights", self.h, C.byref(d), _vp(wp), _vp(wpT))

    def collapse_table(self, items):
        """items: [(wp5, bias, wpc, bias4 DevTensors, C, K[, mode])] -> (device table ptr, n, total blocks) for
        upconv_collapse_batched (uploaded once: the pointers are fixed for the life of a plan); mode 1 = the bilinear form"""
        rec = np.zeros(len(items), dtype=[('wp5', '<u8'), ('bias', '<u8'), ('wpc', '<u8'), ('b4', '<u8'), ('C', '<i4'),
                                          ('K', '<i4'), ('b0', '<i4'), ('pad', '<i4')])
        b0 = 0
        for i, (w5, b, wpc, b4, Cc, K, *mode) in enumerate(items):
            rec[i] = (w5.ptr, b.ptr if b is not None else 0, wpc.ptr, b4.ptr if b4 is not None else 0, Cc, K, b0, mode[0] if mode else 0)
            b0 += (36 * Cc * K + 4 * K + 255) // 256
        ptr = self.dev.alloc(max(rec.nbytes, 40))
        self.dev.h2d(ptr, rec.view(np.uint8))
        return ptr, len(items), b0

    def upconv_collapse_batched(self, table):
        ptr, n, blocks = table
        call("ghm_upconv_collapse_batched", self.h, C.c_void_p(ptr), n, blocks)

    def expand_table(self, items):
        """items: [(dwpc, dwp5 DevTensors, C, K)] -> (device table ptr, n, total blocks) for upconv_expand_batched"""
        rec = np.zeros(len(items), dtype=[('dwpc', '<u8'), ('dwp5', '<u8'), ('C', '<i4'), ('K', '<i4'), ('b0', '<i4'),
                                          ('pad', '<i4')])
        b0 = 0
        for i, (dwpc, dwp5, Cc, K, *mode) in enumerate(items):
            rec[i] = (dwpc.ptr, dwp5.ptr, Cc, K, b0, mode[0] if mode else 0)
            b0 += (25 * Cc * K + 255) // 256
        ptr = self.dev.alloc(max(rec.nbytes, 32))
        self.dev.h2d(ptr, rec.view(np.uint8))
        return ptr, len(items), b0

    def upconv_expand_batched(self, table, accumulate=False):
        ptr, n, blocks = table
        call("ghm_upconv_expand_batched", self.h, C.c_void_p(ptr), n, blocks, int(accumulate))

    # ---- BilinearUpsample2DLayer(2) -> 3x3 conv: the frame the collapsed convolution leaves out (csrc/conv_bilinear.hip) ----
    def blconv_supported(self, N, Cc, K, n1, n2):
        return bool(_lib.load().ghm_blconv_supported(int(N), int(Cc), int(K), int(n1), int(n2)))

    def blconv_frame_sizes(self, N, Cc, K, n1, n2):
        a, b = C.c_int64(), C.c_int64()
        call("ghm_blconv_frame_sizes", int(N), int(Cc), int(K), int(n1), int(n2), C.byref(a), C.byref(b))
        return a.value, b.value

    def blconv_frame_splits(self, N, Cc, K, n1, n2):
        """(forward, data-gradient, weight-gradient) split-K counts the frame products launch with on this device"""
        out = (C.c_int32 * 3)()
        call("ghm_blconv_frame_splits", self.h, int(N), int(Cc), int(K), int(n1), int(n2), out)
        return tuple(out)

    def blconv_frame_fwd(self, x, wp, y_pp, K, FL):
        """y_pp [N, 4K, n1, n2] += conv3x3(frame of x); x: the coarse fp32 input; wp: the layer's packed 3x3 weights"""
        call("ghm_blconv_frame_fwd", self.h, _vp(x), x.nstride, _vp(wp), _vp(y_pp), y_pp.nstride, x.N, x.Cc, int(K), x.H, x.W, _vp(FL))

    def blconv_frame_gather(self, dy_pp, Cc, K, DYL):
        call("ghm_blconv_frame_gather", self.h, _vp(dy_pp), dy_pp.nstride, dy_pp.N, int(Cc), int(K), dy_pp.H, dy_pp.W, _vp(DYL))

    def blconv_frame_dgrad(self, DYL, wp, dx, K):
        call("ghm_blconv_frame_dgrad", self.h, _vp(DYL), _vp(wp), _vp(dx), dx.nstride, dx.N, dx.Cc, int(K), dx.H, dx.W)

    def blconv_frame_wgrad(self, DYL, FL, dwp, N, Cc, K, n1, n2):
        call("ghm_blconv_frame_wgrad", self.h, _vp(DYL), _vp(FL), _vp(dwp), int(N), int(Cc), int(K), int(n1), int(n2))

    def blconv_split_supported(self, d, kind, dtype):
        """may the collapsed bilinear convolution ``d`` (4K filters) run with its structural zero taps skipped?"""
        return dtype in SPLITS and bool(_lib.load().ghm_blconv_split_supported(C.byref(d), int(kind)))

    def blconv_fwd_split(self, d, xq, wq, bias, y, dtype):
        call("ghm_blconv_fwd_split", self.h, C.byref(d), C.c_void_p(xq.ptr), xq.nstride, xq.pstride, _vp(wq), _vp(bias), _vp(y),
             SPLITS[dtype])

    def blconv_dgrad_split(self, d, dyq, wqT, dx, dtype, accumulate=False):
        call("ghm_blconv_dgrad_split", self.h, C.byref(d), C.c_void_p(dyq.ptr), dyq.nstride, dyq.pstride, _vp(wqT), _vp(dx),
             int(accumulate), SPLITS[dtype])

    def blconv_wgrad_split(self, d, xq, dyq, dwp, ws, dtype, accumulate=False):
        call("ghm_blconv_wgrad_split", self.h, C.byref(d), C.c_void_p(xq.ptr), xq.nstride, xq.pstride, C.c_void_p(dyq.ptr),
             dyq.nstride, dyq.pstride, _vp(dwp), _vp(ws), int(accumulate), SPLITS[dtype])

    def transpose_table(self, items):
        """items: [(wp DevTensor, wpT DevTensor, C, T, K)] -> (device table ptr, n, total blocks) for
        transpose_weights_batched (uploaded once: the pointers are fixed for the life of a plan)"""
        rec = np.zeros(len(items), dtype=[('wp', '<u8'), ('wpT', '<u8'), ('C', '<i4'), ('T', '<i4'), ('K', '<i4'),
                                          ('b0', '<i4')])
        b0 = 0
        for i, (wp, wpT, Cc, T, K) in enumerate(items):
            rec[i] = (wp.ptr, wpT.ptr, Cc, T, K, b0)
            b0 += T * ((Cc + 31) // 32) * ((K + 31) // 32)
        ptr = self.dev.alloc(max(rec.nbytes, 32))
        self.dev.h2d(ptr, rec.view(np.uint8))
        return ptr, len(items), b0

    def transpose_weights_batched(self, table):
        ptr, n, blocks = table
        call("ghm_transpose_weights_batched", self.h, C.c_void_p(ptr), n, blocks)

    def conv2d_dgrad_t(self, d, dy, wpT, dx, bias=None, act='linear', alpha=0.0, accumulate=False):
        call("ghm_conv2d_dgrad_t", self.h, C.byref(d), _vp(dy), _vp(wpT), _vp(bias), _vp(dx), ACT_CODES[act], alpha,
             int(accumulate))

    def dgrad_dact_supported(self, d, dtype='f32'):
        """0: not served; 1 / 2 / 3: served, reading the fp32 packed wp / the fp32 wpT / the low-precision wqT"""
        if dtype in SPLITS:
            if _lib.load().ghm_split_dgrad_dact_supported(C.byref(d)):
                return 3
            dtype = 'f32'
        return int(_lib.load().ghm_dgrad_dact_supported(C.byref(d), DTYPE_CODES[dtype]))

    def conv2d_dgrad_dact(self, d, dy, w, dx, y, act, alpha, dtype='f32'):
        """dx = conv^T(dy) * act'(y): the data gradient with the producer's activation backward in its epilogue"""
        assert y.shape == dx.shape
        if dtype in SPLITS:
            # a split weight pack has no fp32-operand form of this product: ghm_conv2d_dgrad_dact would read it as an fp32 /
            # low-precision pack.  The split data gradient with the activation backward takes the q copy of dy
            raise ValueError("conv2d_dgrad_dact(dtype='bf16x3'): use conv2d_dgrad_dact_lp_q with the split q tensor of dy")
        call("ghm_conv2d_dgrad_dact", self.h, C.byref(d), _vp(dy), _vp(w), _vp(dx), _vp(y), y.nstride, ACT_CODES[act], alpha,
             DTYPE_CODES[dtype])

    def wgrad_workspace(self, d):
        n = C.c_size_t()
        call("ghm_conv2d_wgrad_workspace", C.byref(d), C.byref(n))
        return n.value

    def conv2d_wgrad(self, d, x, dy, dwp, ws, accumulate=False):
        call("ghm_conv2d_wgrad", self.h, C.byref(d), _vp(x), _vp(dy), _vp(dwp), _vp(ws), int(accumulate))

    # ---- bf16 / fp16 matrix-core convolutions (fp32 tensors in HBM; include/ghm.h GHM_DTYPE_*) ----
    def lp_supported(self, d, kind, dtype):
        if dtype in SPLITS:
            return self.split_supported(d, kind)
        return bool(_lib.load().ghm_lp_supported(C.byref(d), int(kind), DTYPE_CODES[dtype]))

    # ---- fp32 on the bf16 matrix cores by operand splitting (csrc/conv_split.hip; opt-in) ----
    def split_supported(self, d, kind):
        return bool(_lib.load().ghm_split_supported(C.byref(d), int(kind)))

    def split_weight_bytes(self, d, transposed=False, pieces=3):
        n = C.c_size_t()
        call("ghm_split_weight_bytes", C.byref(d), int(transposed), C.byref(n), pieces)
        return n.value

    def split_pack_weights(self, d, wp, wq, transposed=False, pieces=3):
        call("ghm_split_pack_weights", self.h, C.byref(d), _vp(wp), _vp(wq), int(transposed), pieces)

    def split_pack(self, x, q_ptr, q_nstride=None, q_pstride=None, pieces=3):
        """fp32 view -> split q tensor (``pieces`` planes) at q_ptr; returns (nstride, pstride) in 16-byte units"""
        ns = (x.Cc // 8) * x.HW if q_nstride is None else q_nstride
        ps = x.N * ns if q_pstride is None else q_pstride
        call("ghm_split_pack", self.h, _vp(x), x.nstride, x.N, x.Cc, x.HW, C.c_void_p(int(q_ptr)), ns, ps, pieces)
        return ns, ps

    def split_q_direct(self, d, kind):
        return bool(_lib.load().ghm_split_q_direct(C.byref(d), int(kind)))

    def conv2d_fwd_split(self, d, x, wq, bias, y, act='linear', alpha=0.0, accumulate=False, xq=None, yq=None, pieces=3):
        """xq = (ptr, nstride, pstride) of the input already split, or None (the entry point splits x); yq: a whole split
        QTensor (or a channel slice of one) that also receives the result; y may then be None"""
        q = xq or (None, 0, 0)
        assert yq is None or yq.pstride == yq.N * yq.nstride
        call("ghm_conv2d_fwd_split", self.h, C.byref(d), _vp(x), C.c_void_p(int(q[0])) if q[0] else None, q[1], q[2],
             _vp(wq), _vp(bias), _vp(y), C.c_void_p(yq.ptr) if yq is not None else None, yq.nstride if yq is not None else 0,
             ACT_CODES[act], alpha, int(accumulate), pieces)

    def conv2d_dgrad_split(self, d, dy, wqT, dx, bias=None, act='linear', alpha=0.0, accumulate=False, dyq=None, dxq=None,
                           pieces=3):
        q = dyq or (None, 0, 0)
        assert dxq is None or dxq.pstride == dxq.N * dxq.nstride
        call("ghm_conv2d_dgrad_split", self.h, C.byref(d), _vp(dy), C.c_void_p(int(q[0])) if q[0] else None, q[1], q[2],
             _vp(wqT), _vp(bias), _vp(dx), C.c_void_p(dxq.ptr) if dxq is not None else None,
             dxq.nstride if dxq is not None else 0, ACT_CODES[act], alpha, int(accumulate), pieces)

    def lp_weight_bytes(self, d, transposed=False, dtype=None):
        if dtype in SPLITS:
            return self.split_weight_bytes(d, transposed, SPLITS[dtype])
        n = C.c_size_t()
        call("ghm_lp_weight_bytes", C.byref(d), int(transposed), C.byref(n))
        return n.value

    def lp_pack_weights(self, d, wp, wq, dtype, transposed=False):
        if dtype in SPLITS:
            return self.split_pack_weights(d, wp, wq, transposed, SPLITS[dtype])
        call("ghm_lp_pack_weights", self.h, C.byref(d), _vp(wp), _vp(wq), DTYPE_CODES[dtype], int(transposed))

    def lp_pack_table(self, items):
        """items: [(wp DevTensor | ptr, wq ptr, red, T, rows, transposed)] -> (device table ptr, n, total blocks) for
        lp_pack_batched (uploaded once: the pointers are fixed for the life of a plan).  The kernels store 16-byte units and the
        entry point cannot see the device table's pointers: a wq that is not 16-byte aligned is refused here"""
        for it in items:
            if int(it[1]) % 16:
                raise ValueError("lp_pack_table: wq %#x is not 16-byte aligned (the pack is stored in 16-byte units)" % int(it[1]))
        rec = np.zeros(len(items), dtype=[('wp', '<u8'), ('wq', '<u8'), ('red', '<i4'), ('T', '<i4'), ('rows', '<i4'),
                                          ('nblk', '<i4'), ('rpad', '<i4'), ('tr', '<i4'), ('b0', '<i4'), ('pad', '<i4')])
        b0 = 0
        for i, (wp, wq, red, T, rows, tr) in enumerate(items):
            nblk, rpad = (red + 15) // 16 * 2, (rows + 127) // 128 * 128
            rec[i] = (wp.ptr if isinstance(wp, DevTensor) else int(wp), int(wq), red, T, rows, nblk, rpad, int(tr), b0, 0)
            b0 += (nblk * T * rpad + 255) // 256
        ptr = self.dev.alloc(max(rec.nbytes, 48))
        self.dev.h2d(ptr, rec.view(np.uint8))
        return ptr, len(items), b0

    def lp_pack_batched(self, table, dtype):
        ptr, n, blocks = table
        if dtype in SPLITS:
            return call("ghm_split_pack_batched", self.h, C.c_void_p(ptr), n, blocks, SPLITS[dtype])
        call("ghm_lp_pack_batched", self.h, C.c_void_p(ptr), n, blocks, DTYPE_CODES[dtype])

    def conv2d_fwd_lp(self, d, x, wq, bias, y, dtype, act='linear', alpha=0.0, accumulate=False):
        if dtype in SPLITS:
            return self.conv2d_fwd_split(d, x, wq, bias, y, act, alpha, accumulate, pieces=SPLITS[dtype])
        call("ghm_conv2d_fwd_lp", self.h, C.byref(d), _vp(x), _vp(wq), _vp(bias), _vp(y), ACT_CODES[act], alpha,
             int(accumulate), DTYPE_CODES[dtype])

    def conv2d_dgrad_lp(self, d, dy, wqT, dx, dtype, bias=None, act='linear', alpha=0.0, accumulate=False):
        if dtype in SPLITS:
            return self.conv2d_dgrad_split(d, dy, wqT, dx, bias, act, alpha, accumulate, pieces=SPLITS[dtype])
        call("ghm_conv2d_dgrad_lp", self.h, C.byref(d), _vp(dy), _vp(wqT), _vp(bias), _vp(dx), ACT_CODES[act], alpha,
             int(accumulate), DTYPE_CODES[dtype])

    def wgrad_lp_workspace(self, d):
        n, m = C.c_size_t(), C.c_size_t()
        call("ghm_conv2d_wgrad_lp_workspace", C.byref(d), C.byref(n))
        call("ghm_conv2d_wgrad_split_workspace", C.byref(d), C.byref(m))
        return max(n.value, m.value)

    def conv2d_wgrad_lp(self, d, x, dy, dwp, ws, dtype, accumulate=False):
        call("ghm_conv2d_wgrad_lp", self.h, C.byref(d), _vp(x), _vp(dy), _vp(dwp), _vp(ws), int(accumulate),
             DTYPE_CODES[dtype])

    # ---- q tensors (include/ghm.h): low-precision products on operands rounded once at their producer ----
    def q_pack(self, x, q):
        assert x.shape == q.shape
        if q.dtype in SPLITS:
            return self.split_pack(x, q.ptr, q.nstride, q.pstride, SPLITS[q.dtype])
        call("ghm_q_pack", self.h, _vp(x), x.nstride, x.N, x.Cc, x.HW, C.c_void_p(q.ptr), q.nstride, DTYPE_CODES[q.dtype])

    def q_unpack(self, q, x):
        assert x.shape == q.shape
        call("ghm_q_unpack", self.h, C.c_void_p(q.ptr), q.nstride, q.N, q.Cc, q.HW, _vp(x), x.nstride, DTYPE_CODES[q.dtype])

    def lp_q_direct(self, d, kind, dtype):
        if dtype in SPLITS:
            return self.split_q_direct(d, kind)
        return bool(_lib.load().ghm_lp_q_direct(C.byref(d), int(kind), DTYPE_CODES[dtype]))

    def conv_variant_lp(self, d, kind, dtype):
        """kernel family serving low-precision product ``kind`` (0 forward, 1 data gradient, 2 weight gradient)"""
        if dtype in SPLITS:
            w = d.W if kind == 1 and d.stride == 1 else d.Wo          # width of the pixel grid the kernel tiles
            if kind == 1 and d.stride == 2:
                return "sp_dgrad_s2_kernel"
            return ("sp_wgrad_kernel<%d, %d>%s" if kind == 2 else "sp_conv2_kernel<%d, %d>%s") % (
                d.kh, d.stride, "" if w % 32 == 0 else " narrow")
        out = C.create_string_buffer(128)
        call("ghm_lp_variant", C.byref(d), int(kind), DTYPE_CODES[dtype], out, 128)
        return out.value.decode()

    def conv_bn_fused_supported(self, d, dtype):
        if dtype in SPLITS:
            return False
        if dtype == 'f32':
            return bool(_lib.load().ghm_conv_bn_fused_supported_f32(C.byref(d)))
        return bool(_lib.load().ghm_conv_bn_fused_supported(C.byref(d), DTYPE_CODES[dtype]))

    def conv2d_bn_fwd(self, d, x, wp, bias, conv_out, y, gamma, beta, mean, inv, run_mean, run_inv, eps, run_alpha,
                      act='linear', alpha=0.0):
        """fp32: y = act(bn(conv(x) + bias)) with batch statistics; conv_out keeps conv(x) + bias for the backward"""
        assert conv_out.nstride == d.y_nstride
        call("ghm_conv2d_bn_fwd", self.h, C.byref(d), _vp(x), _vp(wp), _vp(bias), _vp(conv_out), _vp(y), y.nstride, _vp(gamma),
             _vp(beta), _vp(mean), _vp(inv), _vp(run_mean), _vp(run_inv), eps, run_alpha, ACT_CODES[act], alpha)

    def conv2d_bn_fwd_lp_q(self, d, xq, wq, bias, conv_out, y, yq, gamma, beta, mean, inv, run_mean, run_inv, eps, run_alpha,
                           dtype, act='linear', alpha=0.0):
        """y / yq = act(bn(conv(xq) + bias)) with batch statistics; conv_out (fp32) keeps conv(xq) + bias for the backward"""
        assert conv_out.nstride == d.y_nstride
        call("ghm_conv2d_bn_fwd_lp_q", self.h, C.byref(d), C.c_void_p(xq.ptr), xq.nstride, _vp(wq), _vp(bias), _vp(conv_out),
             _vp(y), y.nstride if y is not None else 0, C.c_void_p(yq.ptr if yq is not None else 0),
             yq.nstride if yq is not None else 0, _vp(gamma), _vp(beta), _vp(mean), _vp(inv), _vp(run_mean), _vp(run_inv),
             eps, run_alpha, ACT_CODES[act], alpha, DTYPE_CODES[dtype])

    def conv2d_fwd_lp_q(self, d, xq, wq, bias, y, yq, dtype, act='linear', alpha=0.0, accumulate=False):
        if dtype in SPLITS:
            return self.conv2d_fwd_split(d, None, wq, bias, y, act, alpha, accumulate, xq=(xq.ptr, xq.nstride, xq.pstride), yq=yq,
                                         pieces=SPLITS[dtype])
        call("ghm_conv2d_fwd_lp_q", self.h, C.byref(d), C.c_void_p(xq.ptr), xq.nstride, _vp(wq), _vp(bias), _vp(y),
             C.c_void_p(yq.ptr if yq is not None else 0), yq.nstride if yq is not None else 0, ACT_CODES[act], alpha,
             int(accumulate), DTYPE_CODES[dtype])

    def conv2d_dgrad_lp_q(self, d, dyq, wqT, dx, dxq, dtype, bias=None, act='linear', alpha=0.0, accumulate=False):
        if dtype in SPLITS:
            return self.conv2d_dgrad_split(d, None, wqT, dx, bias, act, alpha, accumulate,
                                           dyq=(dyq.ptr, dyq.nstride, dyq.pstride), dxq=dxq, pieces=SPLITS[dtype])
        call("ghm_conv2d_dgrad_lp_q", self.h, C.byref(d), C.c_void_p(dyq.ptr), dyq.nstride, _vp(wqT), _vp(bias), _vp(dx),
             C.c_void_p(dxq.ptr if dxq is not None else 0), dxq.nstride if dxq is not None else 0, ACT_CODES[act], alpha,
             int(accumulate), DTYPE_CODES[dtype])

    def conv2d_dgrad_dact_lp_q(self, d, dyq, wqT, dx, dxq, y, act, alpha, dtype):
        if dtype in SPLITS:
            assert dxq is None or dxq.pstride == dxq.N * dxq.nstride
            if isinstance(y, QTensor):          # the slope from the sign of the producer's q copy (its first piece plane)
                assert y.dtype == dtype and y.shape[1:] == (d.C, d.H, d.W)
                return call("ghm_conv2d_dgrad_dact_split_q", self.h, C.byref(d), C.c_void_p(dyq.ptr), dyq.nstride, dyq.pstride,
                            _vp(wqT), _vp(dx), C.c_void_p(dxq.ptr) if dxq is not None else None,
                            dxq.nstride if dxq is not None else 0, C.c_void_p(y.ptr), y.nstride, ACT_CODES[act], alpha,
                            SPLITS[dtype])
            return call("ghm_conv2d_dgrad_dact_split", self.h, C.byref(d), C.c_void_p(dyq.ptr), dyq.nstride, dyq.pstride,
                        _vp(wqT), _vp(dx), C.c_void_p(dxq.ptr) if dxq is not None else None,
                        dxq.nstride if dxq is not None else 0, _vp(y), y.nstride, ACT_CODES[act], alpha, SPLITS[dtype])
        call("ghm_conv2d_dgrad_dact_lp_q", self.h, C.byref(d), C.c_void_p(dyq.ptr), dyq.nstride, _vp(wqT), _vp(dx),
             C.c_void_p(dxq.ptr if dxq is not None else 0), dxq.nstride if dxq is not None else 0, _vp(y), y.nstride,
             ACT_CODES[act], alpha, DTYPE_CODES[dtype])

    @staticmethod
    def _whole_planes(q):
        """the q epilogues of the element-wise producers place the piece planes of a split q tensor N x nstride units apart: a
        sample-sliced view (which keeps the allocation's pstride) would have pieces 1 and 2 written over other samples' data"""
        assert q is None or q.dtype not in SPLITS or q.pstride == q.N * q.nstride, \
            "split q tensor: a sample slice cannot be the target of an element-wise q epilogue"

    def bn_apply_q(self, x, y, mean, inv, gamma, beta, yq, act='linear', alpha=0.0):
        self._whole_planes(yq)
        call("ghm_bn_apply_q", self.h, _vp(x), x.nstride, _vp(y), y.nstride if y is not None else 0, x.N, x.Cc, x.HW, _vp(mean),
             _vp(inv), _vp(gamma), _vp(beta), ACT_CODES[act], alpha, C.c_void_p(yq.ptr), yq.nstride, DTYPE_CODES[yq.dtype])

    def bn_backward_q(self, dout, y, x, dx, mean, inv, gamma, dgamma, dbeta, ws, dxq, act='linear', alpha=0.0, accumulate=False,
                      beta=None):
        """y may be None when beta is given: the layer output is recomputed from x"""
        self._whole_planes(dxq)
        call("ghm_bn_backward_q", self.h, _vp(dout), dout.nstride, _vp(y), y.nstride if y is not None else 0, _vp(x), x.nstride,
             _vp(dx), dx.nstride if dx is not None else 0, x.N, x.Cc, x.HW, _vp(mean), _vp(inv), _vp(gamma), _vp(beta),
             _vp(dgamma), _vp(dbeta), ACT_CODES[act], alpha, int(accumulate), _vp(ws), C.c_void_p(dxq.ptr), dxq.nstride,
             DTYPE_CODES[dxq.dtype])

    def bn_backward_x(self, dout, x, dx, mean, inv, gamma, beta, dgamma, dbeta, ws, act='linear', alpha=0.0, accumulate=False):
        """ghm_bn_backward without reading y (recomputed from x, bit-identical to the forward pass's value)"""
        call("ghm_bn_backward_x", self.h, _vp(dout), dout.nstride, _vp(x), x.nstride, _vp(dx), dx.nstride, x.N, x.Cc, x.HW,
             _vp(mean), _vp(inv), _vp(gamma), _vp(beta), _vp(dgamma), _vp(dbeta), ACT_CODES[act], alpha, int(accumulate), _vp(ws))

    def upsample_bilinear2_fwd_q(self, x, y, yq):
        assert y is None or y.contiguous
        self._whole_planes(yq)
        call("ghm_upsample_bilinear2_fwd_q", self.h, _vp(x), x.nstride, _vp(y), x.N, x.Cc, x.H, x.W, C.c_void_p(yq.ptr),
             yq.nstride, DTYPE_CODES[yq.dtype])

    def pp_to_hi_q(self, pp, hi, hiq):
        self._whole_planes(hiq)
        assert pp.contiguous and pp.N == 4 * hiq.N
        call("ghm_pp_to_hi_q", self.h, _vp(pp), _vp(hi), hi.nstride if hi is not None else 0, hiq.N, pp.Cc, pp.H, pp.W,
             C.c_void_p(hiq.ptr), hiq.nstride, DTYPE_CODES[hiq.dtype])

    def bn_apply_hi(self, x_pp, hi, hiq, mean, inv, gamma, beta, act='linear', alpha=0.0):
        """BatchNorm + activation of a parity-planar tensor written straight in the interleaved layout (hi and / or hiq)"""
        self._whole_planes(hiq)
        assert x_pp.contiguous and (hi is not None or hiq is not None)
        call("ghm_bn_apply_hi", self.h, _vp(x_pp), _vp(hi), hi.nstride if hi is not None else 0, x_pp.N // 4, x_pp.Cc, x_pp.H,
             x_pp.W, _vp(mean), _vp(inv), _vp(gamma), _vp(beta), ACT_CODES[act], alpha,
             C.c_void_p(hiq.ptr if hiq is not None else 0), hiq.nstride if hiq is not None else 0,
             DTYPE_CODES[hiq.dtype] if hiq is not None else 0)

    def bn_backward_hi(self, dhi, x_pp, dx_pp, dxq, mean, inv, gamma, beta, dgamma, dbeta, ws, act='linear', alpha=0.0,
                       accumulate=False):
        """backward of bn_apply_hi: dhi in the interleaved layout, dx (fp32 and / or q) parity-planar"""
        self._whole_planes(dxq)
        assert x_pp.contiguous and (dx_pp is None or dx_pp.contiguous) and (dx_pp is not None or dxq is not None)
        assert dxq is None or dxq.contiguous
        call("ghm_bn_backward_hi", self.h, _vp(dhi), dhi.nstride, _vp(x_pp), _vp(dx_pp), x_pp.N // 4, x_pp.Cc, x_pp.H, x_pp.W,
             _vp(mean), _vp(inv), _vp(gamma), _vp(beta), _vp(dgamma), _vp(dbeta), ACT_CODES[act], alpha, int(accumulate), _vp(ws),
             C.c_void_p(dxq.ptr if dxq is not None else 0), DTYPE_CODES[dxq.dtype] if dxq is not None else 0)

    def maxpool2_mask_bwd_q(self, mask_ptr, y, dy, dx, dxq, act, alpha, dbias=None, accumulate=False):
        self._whole_planes(dxq)
        N, Cc, H, W = dxq.shape
        call("ghm_maxpool2_mask_bwd_q", self.h, C.c_void_p(int(mask_ptr)), _vp(y), _vp(dy), _vp(dx), N, Cc, H, W,
             ACT_CODES[act], alpha, _vp(dbias), int(accumulate), C.c_void_p(dxq.ptr), dxq.nstride, DTYPE_CODES[dxq.dtype])

    def maxpool2_mask_bwd_compress_q(self, mask_ptr, y, dy, cq, idx, flags, act, alpha):
        """the same gradient as half-width rows + column bits (the sparse matrix instruction's operand; ghm.h); ``cq`` is a
        QTensor of shape (N, C, H, W / 2), ``idx`` (N * C / 8 * H * W / 32 units of 16 bytes) and ``flags`` (N * H int32) raw"""
        N, Cc, H, Wh = cq.shape
        call("ghm_maxpool2_mask_bwd_compress_q", self.h, C.c_void_p(int(mask_ptr)), _vp(y), _vp(dy), N, Cc, H, 2 * Wh,
             ACT_CODES[act], alpha, C.c_void_p(cq.ptr), cq.nstride, _vp(idx), _vp(flags), DTYPE_CODES[cq.dtype])

    def wgrad_pooled_split_supported(self, d, dtype):
        return dtype in SPLITS and bool(_lib.load().ghm_conv2d_wgrad_pooled_split_supported(C.byref(d)))

    def conv2d_wgrad_pooled_split(self, d, xq, dyq, cq, idx, flags, dwp, ws, dtype, accumulate=False):
        call("ghm_conv2d_wgrad_pooled_split", self.h, C.byref(d), C.c_void_p(xq.ptr), xq.nstride, xq.pstride, C.c_void_p(dyq.ptr),
             dyq.nstride, dyq.pstride, C.c_void_p(cq.ptr), cq.nstride, cq.pstride, _vp(idx), _vp(flags), _vp(dwp), _vp(ws),
             int(accumulate), SPLITS[dtype])

    def lp_wgrad_q_supported(self, d, dtype):
        if dtype in SPLITS:
            return self.split_supported(d, 2)
        return bool(_lib.load().ghm_lp_wgrad_q_supported(C.byref(d), DTYPE_CODES[dtype]))

    def conv2d_wgrad_lp_q(self, d, xq, dyq, dwp, ws, dtype, accumulate=False):
        if dtype in SPLITS:
            return call("ghm_conv2d_wgrad_split", self.h, C.byref(d), C.c_void_p(xq.ptr), xq.nstride, xq.pstride,
                        C.c_void_p(dyq.ptr), dyq.nstride, dyq.pstride, _vp(dwp), _vp(ws), int(accumulate), SPLITS[dtype])
        call("ghm_conv2d_wgrad_lp_q", self.h, C.byref(d), C.c_void_p(xq.ptr), xq.nstride, C.c_void_p(dyq.ptr), dyq.nstride,
             _vp(dwp), _vp(ws), int(accumulate), DTYPE_CODES[dtype])

    def conv2d_fwd_pool_lp_q(self, d, xq, wq, bias, pooled, pooledq, mask_ptr, act, alpha, dtype):
        if dtype in SPLITS:
            assert pooledq is None or pooledq.pstride == pooledq.N * pooledq.nstride
            return call("ghm_conv2d_fwd_pool_split", self.h, C.byref(d), None, C.c_void_p(xq.ptr), xq.nstride, xq.pstride,
                        _vp(wq), _vp(bias), _vp(pooled), C.c_void_p(pooledq.ptr) if pooledq is not None else None,
                        pooledq.nstride if pooledq is not None else 0, C.c_void_p(int(mask_ptr)), ACT_CODES[act], alpha,
                        SPLITS[dtype])
        call("ghm_conv2d_fwd_pool_lp_q", self.h, C.byref(d), C.c_void_p(xq.ptr), xq.nstride, _vp(wq), _vp(bias), _vp(pooled),
             C.c_void_p(pooledq.ptr if pooledq is not None else 0), pooledq.nstride if pooledq is not None else 0,
             C.c_void_p(int(mask_ptr)), ACT_CODES[act], alpha, DTYPE_CODES[dtype])

    # ---- conv + activation + 2x2 max-pool fused (architectures/dcgan.py:42-47) ----
    def conv_pool_supported(self, d, act, dtype='f32'):
        """0: not served; 1: served with the fp32 packed weights; 2: served with the low-precision pack"""
        if dtype in SPLITS:
            if d.C > 4 and _lib.load().ghm_split_pool_supported(C.byref(d), ACT_CODES[act]):
                return 2
            dtype = 'f32'
        return int(_lib.load().ghm_conv2d_pool_supported(C.byref(d), ACT_CODES[act], DTYPE_CODES[dtype]))

    def conv2d_fwd_pool(self, d, x, w, bias, pooled, mask_ptr, act, alpha, dtype='f32'):
        assert pooled.contiguous
        if dtype in SPLITS:
            return call("ghm_conv2d_fwd_pool_split", self.h, C.byref(d), _vp(x), None, 0, 0, _vp(w), _vp(bias), _vp(pooled),
                        None, 0, C.c_void_p(int(mask_ptr)), ACT_CODES[act], alpha, SPLITS[dtype])
        call("ghm_conv2d_fwd_pool", self.h, C.byref(d), _vp(x), _vp(w), _vp(bias), _vp(pooled), C.c_void_p(int(mask_ptr)),
             ACT_CODES[act], alpha, DTYPE_CODES[dtype])

    def maxpool2_mask_bwd(self, mask_ptr, y, dy, dx, act, alpha, dbias=None, accumulate=False):
        """y, dy: pooled [N,C,H/2,W/2]; dx: full-resolution [N,C,H,W]; dbias: also (+)= the per-channel sum of dx"""
        assert (y is None or y.contiguous) and dy.contiguous and dx.contiguous      # y None: slope from the mask's sign bit
        if dbias is None:
            call("ghm_maxpool2_mask_bwd", self.h, C.c_void_p(int(mask_ptr)), _vp(y), _vp(dy), _vp(dx), dx.N, dx.Cc, dx.H,
                 dx.W, ACT_CODES[act], alpha)
        else:
            call("ghm_maxpool2_mask_bwd_bias", self.h, C.c_void_p(int(mask_ptr)), _vp(y), _vp(dy), _vp(dx), dx.N, dx.Cc,
                 dx.H, dx.W, ACT_CODES[act], alpha, _vp(dbias), int(accumulate))

    def thin_fwd_q_supported(self, d, act, pooled, dtype):
        return bool(_lib.load().ghm_thin_fwd_q_supported(C.byref(d), ACT_CODES[act], int(pooled), DTYPE_CODES[dtype]))

    def thin_pool_lp_served(self, d, act, alpha, dtype):
        """the pooled first-layer forward runs on the bf16 / fp16 matrix cores (rounded operands) for this layer"""
        return bool(_lib.load().ghm_thin_pool_lp_served(C.byref(d), ACT_CODES[act], alpha, DTYPE_CODES[dtype]))

    def conv2d_fwd_thin_q(self, d, x, w, bias, y, yq, act='linear', alpha=0.0):
        """first-layer forward (<= 4 input channels) writing its fp32 result and the q copy in one pass"""
        call("ghm_conv2d_fwd_thin_q", self.h, C.byref(d), _vp(x), _vp(w), _vp(bias), _vp(y), ACT_CODES[act], alpha,
             C.c_void_p(yq.ptr), yq.nstride, DTYPE_CODES[yq.dtype])

    def conv2d_fwd_pool_thin_q(self, d, x, w, bias, pooled, mask_ptr, yq, act, alpha):
        assert pooled is None or pooled.contiguous      # None: only the q copy and the mask are written
        call("ghm_conv2d_fwd_pool_thin_q", self.h, C.byref(d), _vp(x), _vp(w), _vp(bias), _vp(pooled),
             C.c_void_p(int(mask_ptr)), ACT_CODES[act], alpha, C.c_void_p(yq.ptr), yq.nstride, DTYPE_CODES[yq.dtype])

    def pool_bwd_sparse_supported(self, d, act):
        """bit 0: weight + bias gradient, bit 1: data gradient of a fused conv + act + pool layer from the pooled operands"""
        return int(_lib.load().ghm_conv2d_pool_bwd_sparse_supported(C.byref(d), ACT_CODES[act]))

    def pool_wgrad_sparse_workspace(self, d):
        n = C.c_size_t()
        call("ghm_conv2d_pool_wgrad_sparse_workspace", C.byref(d), C.byref(n))
        return n.value

    def conv2d_pool_wgrad_sparse(self, d, x, mask_ptr, yp, gp, dwp, dbias, ws, act, alpha, accumulate=False):
        assert (yp is None or yp.contiguous) and gp.contiguous       # yp None: slope from the mask's sign bit
        call("ghm_conv2d_pool_wgrad_sparse", self.h, C.byref(d), _vp(x), C.c_void_p(int(mask_ptr)), _vp(yp), _vp(gp), _vp(dwp),
             _vp(dbias), ACT_CODES[act], alpha, int(accumulate), _vp(ws))

    def conv2d_pool_dgrad_sparse(self, d, mask_ptr, yp, gp, wp, dx, act, alpha, accumulate=False):
        assert (yp is None or yp.contiguous) and gp.contiguous
        call("ghm_conv2d_pool_dgrad_sparse", self.h, C.byref(d), C.c_void_p(int(mask_ptr)), _vp(yp), _vp(gp), _vp(wp), _vp(dx),
             ACT_CODES[act], alpha, int(accumulate))

    def channel_sum(self, x, out, accumulate=False):
        call("ghm_channel_sum", self.h, _vp(x), x.N, x.Cc, x.HW, x.nstride, _vp(out), int(accumulate))

    def bn_workspace(self, Cc):
        return _lib.load().ghm_bn_workspace(Cc)

    def bn_stats(self, x, mean, inv, ws, run_mean=None, run_inv=None, eps=1e-4, run_alpha=0.1):
        call("ghm_bn_stats", self.h, _vp(x), x.N, x.Cc, x.HW, x.nstride, eps, _vp(mean), _vp(inv), _vp(run_mean),
             _vp(run_inv), run_alpha, _vp(ws))

    def bn_apply(self, x, y, mean, inv, gamma, beta, act='linear', alpha=0.0):
        call("ghm_bn_apply", self.h, _vp(x), x.nstride, _vp(y), y.nstride, x.N, x.Cc, x.HW, _vp(mean), _vp(inv),
             _vp(gamma), _vp(beta), ACT_CODES[act], alpha)

    def bn_forward(self, x, y, mean, inv, gamma, beta, ws, run_mean=None, run_inv=None, eps=1e-4, run_alpha=0.1,
                   act='linear', alpha=0.0):
        """batch statistics (+ running update) and normalise + activation: one launch for small tensors"""
        call("ghm_bn_forward", self.h, _vp(x), x.nstride, _vp(y), y.nstride, x.N, x.Cc, x.HW, eps, _vp(mean), _vp(inv),
             _vp(run_mean), _vp(run_inv), run_alpha, _vp(gamma), _vp(beta), ACT_CODES[act], alpha, _vp(ws))

    def instance_norm_fwd(self, x, y, mean, inv, gamma, beta, ws, eps=1e-4, act='linear', alpha=0.0, group=1):
        """InstanceNorm: BatchNorm's statistics per (instance, channel); mean / inv: [N / group, C]"""
        call("ghm_instance_norm_fwd", self.h, _vp(x), x.nstride, _vp(y), y.nstride, x.N, x.Cc, x.HW, eps, _vp(mean), _vp(inv),
             _vp(gamma), _vp(beta), ACT_CODES[act], alpha, _vp(ws), group)

    def instance_norm_bwd(self, dout, x, dx, mean, inv, gamma, beta, dgamma, dbeta, ws, act='linear', alpha=0.0,
                          accumulate=False, group=1):
        call("ghm_instance_norm_bwd", self.h, _vp(dout), dout.nstride, _vp(x), x.nstride, _vp(dx), dx.nstride, x.N, x.Cc, x.HW,
             _vp(mean), _vp(inv), _vp(gamma), _vp(beta), _vp(dgamma), _vp(dbeta), ACT_CODES[act], alpha, int(accumulate), _vp(ws),
             group)

    def bn_backward(self, dout, y, x, dx, mean, inv, gamma, dgamma, dbeta, ws, act='linear', alpha=0.0,
                    accumulate=False):
        call("ghm_bn_backward", self.h, _vp(dout), dout.nstride, _vp(y), y.nstride, _vp(x), x.nstride, _vp(dx),
             dx.nstride, x.N, x.Cc, x.HW, _vp(mean), _vp(inv), _vp(gamma), _vp(dgamma), _vp(dbeta), ACT_CODES[act],
             alpha, int(accumulate), _vp(ws))

    def act_fwd(self, x, y, act, alpha=0.0):
        call("ghm_act_fwd", self.h, _vp(x), x.nstride, _vp(y), y.nstride, x.N, x.Cc, x.HW, ACT_CODES[act], alpha)

    def act_bwd(self, dout, y, dx, act, alpha=0.0, accumulate=False):
        call("ghm_act_bwd", self.h, _vp(dout), dout.nstride, _vp(y), y.nstride, _vp(dx), dx.nstride, y.N, y.Cc, y.HW,
             ACT_CODES[act], alpha, int(accumulate))

    def maxpool2_fwd(self, x, y):
        assert x.contiguous and y.contiguous
        call("ghm_maxpool2_fwd", self.h, _vp(x), _vp(y), x.N, x.Cc, x.H, x.W)

    def maxpool2_bwd(self, x, y, dy, dx, act='linear', alpha=0.0):
        assert x.contiguous and y.contiguous and dy.contiguous and dx.contiguous
        call("ghm_maxpool2_bwd", self.h, _vp(x), _vp(y), _vp(dy), _vp(dx), x.N, x.Cc, x.H, x.W, ACT_CODES[act], alpha)

    def avgpool_fwd(self, x, y, p):
        assert x.contiguous and y.contiguous
        call("ghm_avgpool_fwd", self.h, _vp(x), _vp(y), x.N, x.Cc, x.H, x.W, p)

    def avgpool_bwd(self, dy, dx, p):
        assert dy.contiguous and dx.contiguous
        call("ghm_avgpool_bwd", self.h, _vp(dy), _vp(dx), dx.N, dx.Cc, dx.H, dx.W, p)

    def dropout(self, x, y, p, key, counter):
        """y = dropout(x); with x = dy it is the backward (same mask: same key, same counter value)"""
        call("ghm_dropout", self.h, _vp(x), x.nstride, _vp(y), y.nstride, x.N, x.Cc, x.HW, float(p), int(key) & 0xffffffff,
             _vp(counter))

    def counter_tick(self, counter):
        call("ghm_counter_tick", self.h, _vp(counter))

    def upconv_collapse_weights(self, wp5, bias, wpc, bias4, C, K):
        call("ghm_upconv_collapse_weights", self.h, _vp(wp5), _vp(bias), _vp(wpc), _vp(bias4), C, K)

    def upconv_expand_wgrad(self, dwpc, dwp5, C, K, accumulate=False):
        call("ghm_upconv_expand_wgrad", self.h, _vp(dwpc), _vp(dwp5), C, K, int(accumulate))

    def pp_to_hi(self, pp, hi):
        """pp [4N,K,H,W] (contiguous) -> hi [N,K,2H,2W]"""
        assert pp.contiguous and pp.N == 4 * hi.N
        call("ghm_pp_to_hi", self.h, _vp(pp), _vp(hi), hi.nstride, hi.N, pp.Cc, pp.H, pp.W)

    def hi_to_pp(self, hi, pp):
        assert pp.contiguous and pp.N == 4 * hi.N
        call("ghm_hi_to_pp", self.h, _vp(hi), hi.nstride, _vp(pp), hi.N, pp.Cc, pp.H, pp.W)

    def upsample_nearest2_fwd(self, x, y):
        assert y.contiguous
        call("ghm_upsample_nearest2_fwd", self.h, _vp(x), x.nstride, _vp(y), x.N, x.Cc, x.H, x.W)

    def upsample_nearest2_bwd(self, dy, dx, accumulate=False):
        assert dy.contiguous
        call("ghm_upsample_nearest2_bwd", self.h, _vp(dy), _vp(dx), dx.nstride, dx.N, dx.Cc, dx.H, dx.W,
             int(accumulate))

    def upsample_bilinear2_fwd(self, x, y):
        assert y.contiguous
        call("ghm_upsample_bilinear2_fwd", self.h, _vp(x), x.nstride, _vp(y), x.N, x.Cc, x.H, x.W)

    def upsample_bilinear2_bwd(self, dy, dx, accumulate=False):
        assert dy.contiguous
        call("ghm_upsample_bilinear2_bwd", self.h, _vp(dy), _vp(dx), dx.nstride, dx.N, dx.Cc, dx.H, dx.W,
             int(accumulate))

    def copy_view(self, x, y, accumulate=False):
        assert x.shape == y.shape
        call("ghm_copy_view", self.h, _vp(x), x.nstride, _vp(y), y.nstride, x.N, x.Cc, x.HW, int(accumulate))

    def scale_samples(self, x, num, den):
        """x[n] *= num[n] / den[n] (0 where den[n] == 0); num, den: one value per sample"""
        assert num.N == x.N and den.N == x.N and num.Cc * num.HW == 1 and den.Cc * den.HW == 1
        call("ghm_scale_samples", self.h, _vp(x), x.nstride, x.N, x.Cc, x.HW, _vp(num), num.nstride, _vp(den), den.nstride)

    def axpby(self, a, x, b, y, n):
        call("ghm_axpby", self.h, a, _vp(x), b, _vp(y), int(n))

    def image_batch(self, src_u8_ptr, N, H, W, Cc, xform_ptr, tanh_range, dst):
        call("ghm_image_batch", self.h, C.c_void_p(int(src_u8_ptr)), N, H, W, Cc, C.c_void_p(int(xform_ptr)),
             int(tanh_range), _vp(dst), dst.nstride)

    # tiled inference (csrc/texture.hip, gan_heightmaps_amd/texture.py)
    def texture_gather(self, band_ptr, band_u8, Cc, band_rows, band_row0, H, W, y0, x0, stride, n_valid, tanh_range, dst):
        call("ghm_texture_gather", self.h, C.c_void_p(int(band_ptr)), int(band_u8), Cc, band_rows, band_row0, H, W, y0, x0,
             stride, n_valid, dst.N, dst.H, int(tanh_range), _vp(dst), dst.nstride)

    def texture_blend(self, acc_ptr, W, T, Cc, u, nb, iy, ny, j0, nx, pad_x, overlap):
        assert u.H == T and u.W == T and u.Cc == Cc and nb <= u.N
        call("ghm_texture_blend", self.h, C.c_void_p(int(acc_ptr)), W, T, Cc, _vp(u), u.nstride, nb, iy, ny, j0, nx, pad_x,
             overlap)

    def texture_finalize(self, acc_ptr, W, T, Cc, r0, nrows, yc0, ny, pad_y, nx, pad_x, overlap, out_u8, b_grey, out_ptr):
        call("ghm_texture_finalize", self.h, C.c_void_p(int(acc_ptr)), W, T, Cc, r0, nrows, yc0, ny, pad_y, nx, pad_x,
             overlap, int(out_u8), int(b_grey), C.c_void_p(int(out_ptr)))

    def texture_finalize_scene(self, acc_ptr, W, T, Cc, r0, nrows, yc0, ny, pad_y, nx, pad_x, overlap, b_grey, tex_ptr, H, Ws,
                               flag_ptr):
        """texture_finalize's fp32 values of the same rows, mapped to [0, 1] as render.Scene maps a texture, -> rows
        yc0 + r0 + ... of the scene texture fp32 [3, H, Ws] at tex_ptr; a non-finite value sets the int32 at flag_ptr"""
        call("ghm_texture_finalize_scene", self.h, _vp(acc_ptr), W, T, Cc, r0, nrows, yc0, ny, pad_y, nx, pad_x, overlap,
             int(b_grey), _vp(tex_ptr), H, Ws, _vp(flag_ptr))

    # heightmaps of any size (csrc/terrain.hip, gan_heightmaps_amd/terrain.py)
    def terrain_seed(self, P, gy, gx, s, row0, rows, blend, dst):
        """canvas seed rows [row0, row0 + rows) of the per-cell maps P [gy gx, C s s] -> dst [1, C, rows, s gx]"""
        C = dst.Cc
        assert P.N == gy * gx and P.Cc * P.HW == C * s * s and dst.N == 1 and dst.H == rows and dst.W == s * gx
        call("ghm_terrain_seed", self.h, _vp(P), P.nstride, gy, gx, C, s, row0, rows, int(blend), _vp(dst), dst.nstride)

    def terrain_emit(self, src, r0, n, out_u8, grey, out_ptr):
        """rows [r0, r0 + n) of src [1, C, H, W] -> fp32 [C, n, W] or uint8 [n, W] / [n, W, 3] at out_ptr"""
        assert src.N == 1
        call("ghm_terrain_emit", self.h, _vp(src), src.Cc, src.H, src.W, r0, n, int(out_u8), int(grey),
             C.c_void_p(int(out_ptr)))

    # regions of an unbounded world (csrc/world.hip, gan_heightmaps_amd/world.py)
    def world_seed(self, P, ci0, cj0, ncy, ncx, s, y0, x0, blend, dst):
        """the seed rectangle [y0, y0 + dst.H) x [x0, x0 + dst.W) of the unbounded canvas -> dst [1, C, rows, cols]; P
        [ncy ncx, C s s] holds the head maps of the cell block [ci0, ci0 + ncy) x [cj0, cj0 + ncx)"""
        C = dst.Cc
        assert P.N == ncy * ncx and P.Cc * P.HW == C * s * s and dst.N == 1
        call("ghm_world_seed", self.h, _vp(P), P.nstride, ci0, cj0, ncy, ncx, C, s, y0, x0, dst.H, dst.W, int(blend),
             _vp(dst), dst.nstride)

    def world_emit(self, src, r0, c0, K, chunk_ptr):
        """rows [r0, r0 + K) x columns [c0, c0 + K) of src [1, C, H, W] -> fp32 [C, K, K] at chunk_ptr"""
        assert src.N == 1
        call("ghm_world_emit", self.h, _vp(src), src.Cc, src.H, src.W, r0, c0, K, C.c_void_p(int(chunk_ptr)))

    def world_crop(self, chunk_ptr, Cc, K, r0, c0, nr, nc, out_u8, grey, out_ptr, pitch, xoff):
        """rows [r0, r0 + nr) x columns [c0, c0 + nc) of a chunk [Cc, K, K] -> columns [xoff, xoff + nc) of the staging
        buffer at out_ptr (rows of ``pitch`` pixels): fp32 [Cc, nr, pitch] or uint8 [nr, pitch] / [nr, pitch, 3]"""
        call("ghm_world_crop", self.h, C.c_void_p(int(chunk_ptr)), Cc, K, r0, c0, nr, nc, int(out_u8), int(grey),
             C.c_void_p(int(out_ptr)), pitch, xoff)

    def world_scene_height(self, chunk_ptr, Cc, K, r0, c0, nr, nc, grey, hm_ptr, H, W, y, x, flag_ptr):
        """rows [r0, r0 + nr) x columns [c0, c0 + nc) of a chunk [Cc, K, K], mapped to [0, 1] as render.Scene maps a
        heightmap (three channels: their mean), -> rows [y, y + nr) x columns [x, x + nc) of the scene's height plane fp32
        [H, W] at hm_ptr; a non-finite input sets the int32 at flag_ptr"""
        call("ghm_world_scene_height", self.h, _vp(chunk_ptr), Cc, K, r0, c0, nr, nc, int(grey), _vp(hm_ptr), H, W, y, x,
             _vp(flag_ptr))

    def world_gather(self, tiles, K, dst):
        """tiles: [((p00, p01, p10, p11), y0, x0)] -- chunk pointers [Cc, K, K] (0 where the tile does not reach) and the
        tile's origin in the first -> dst [B, Cc, T, T]; slots past len(tiles) repeat the last tile"""
        tab = (WorldTile * len(tiles))()
        for t, (ptrs, y0, x0) in zip(tab, tiles):
            for i, p in enumerate(ptrs):
                t.chunk[i] = int(p)
            t.y0, t.x0 = y0, x0
        assert dst.H == dst.W
        call("ghm_world_gather", self.h, tab, len(tiles), dst.N, dst.Cc, dst.H, K, _vp(dst), dst.nstride)

    # camera views of a heightfield (csrc/render.hip, gan_heightmaps_amd/render.py)
    def render_maxmip(self, hm_ptr, H, W):
        """the maximum pyramid of the fp32 [H, W] map at hm_ptr -> a MaxMip (a new device buffer; free it with
        dev.free(mip.ptr))"""
        n = _lib.load().ghm_render_maxmip_elems(int(H), int(W))
        if n < 0:
            raise _lib.GhmError("ghm_render_maxmip_elems: scene %d x %d out of range" % (H, W))
        ptr = self.dev.alloc(4 * n)
        try:
            call("ghm_render_maxmip", self.h, C.c_void_p(int(hm_ptr)), int(H), int(W), C.c_void_p(ptr), n)
        except Exception:
            self.dev.free(ptr)
            raise
        return MaxMip(ptr, int(H), int(W), n)

    def render_view(self, params, hm_ptr, tex_ptr, H, W, mip, out_ptr, depth_ptr=None):
        """one image of the scene (hm fp32 [H, W], tex fp32 [3, H, W]) -> out_ptr: fp32 [3, Hi, Wi], or uint8 [Hi, Wi, 3]
        with params.out_u8; depth_ptr (optional): fp32 [Hi, Wi], t_hit or +inf.  params: a RenderParams (render_params());
        mip: the scene's MaxMip, or None with params.accel = 0"""
        call("ghm_render_view", self.h, C.byref(params) if params is not None else None, _vp(hm_ptr), _vp(tex_ptr), int(H),
             int(W), _vp(mip.ptr if mip is not None else None), mip.H if mip is not None else 0,
             mip.W if mip is not None else 0, _vp(out_ptr), _vp(depth_ptr))

    def render_view_sky(self, params, hm_ptr, tex_ptr, sky_ptr, H, W, mip, out_ptr, depth_ptr=None):
        """render_view with the baked light of the sky: sky_ptr is a fp32 [H, W] plane (skylight_bake's), and a hit's
        ambient term becomes ambient * bilinear(sky); None gives render_view's bits"""
        call("ghm_render_view_sky", self.h, C.byref(params) if params is not None else None, _vp(hm_ptr), _vp(tex_ptr),
             _vp(sky_ptr), int(H), int(W), _vp(mip.ptr if mip is not None else None), mip.H if mip is not None else 0,
             mip.W if mip is not None else 0, _vp(out_ptr), _vp(depth_ptr))

    # the light of the sky (csrc/skylight.hip, gan_heightmaps_amd/skylight.py)
    SKY_TABLES = 8                 # tables a context keeps (a table is at most 64 x 256 x 20 bytes)

    @staticmethod
    def skylight_lds_bytes(reach):
        """bytes of LDS a block of the tiled form needs for this reach, or -1 where the form is refused"""
        return int(_lib.load().ghm_skylight_lds_bytes(int(reach)))

    def skylight_table(self, sky):
        """the device copy of ``sky.table()`` (a skylight.SkyLight): uploaded once per SkyLight and context, freed with the
        context (the least recently used leaves when more than SKY_TABLES are alive)"""
        cache = self.dev.__dict__.setdefault("_sky_tables", {})
        ptr = cache.pop(sky, None)
        if ptr is None:
            tab = np.ascontiguousarray(sky.table())
            ptr = self.dev.alloc(tab.nbytes)
            self.dev.h2d(ptr, tab)
            while len(cache) >= self.SKY_TABLES:
                self.dev.sync()
                self.dev.free(cache.pop(next(iter(cache))))
        cache[sky] = ptr
        return ptr

    def skylight_bake(self, src_ptr, rows, cols, pitch, table_ptr, directions, steps, reach, y0, x0, h, w, height_scale,
                      strength, tiled, out_u8, out_ptr, out_pitch):
        """the sky light of the texels [y0, y0 + h) x [x0, x0 + w) of the fp32 plane at src_ptr (rows x cols, rows of
        ``pitch`` cells; indices are clamped to it) -> out_ptr (rows of out_pitch cells), fp32 or uint8.  table_ptr:
        skylight_table(); reach: the table's"""
        call("ghm_skylight_bake", self.h, _vp(src_ptr), int(rows), int(cols), int(pitch), _vp(table_ptr), int(directions),
             int(steps), int(reach), int(y0), int(x0), int(h), int(w), float(height_scale), float(strength), int(bool(tiled)),
             int(bool(out_u8)), _vp(out_ptr), int(out_pitch))

    # adaptive triangle meshes (csrc/mesh.hip, gan_heightmaps_amd/mesh.py)
    @staticmethod
    def mesh_workspace(h, w):
        """bytes of device workspace mesh_count and mesh_extract need for a rectangle of h x w pixels, or -1"""
        return int(_lib.load().ghm_mesh_workspace(int(h), int(w)))

    def mesh_errors(self, src_ptr, rows, cols, pitch, tile_log2, fused, err_ptr, err_pitch):
        """the error of every vertex of the fp32 height plane at src_ptr ((R T + 1) x (C T + 1), T = 2^tile_log2, rows of
        ``pitch`` cells) -> the fp32 plane at err_ptr (rows of err_pitch cells); fused: the LDS form of the finest scales"""
        call("ghm_mesh_errors", self.h, _vp(src_ptr), int(rows), int(cols), int(pitch), int(tile_log2), int(bool(fused)),
             _vp(err_ptr), int(err_pitch))

    def mesh_count(self, err_ptr, rows, cols, err_pitch, tile_log2, y0, x0, h, w, max_error, workspace_ptr):
        """(vertices, triangles) of the mesh of the tiles [y0, y0 + h] x [x0, x0 + w] at max_error; waits for the stream"""
        V, F = C.c_int64(0), C.c_int64(0)
        call("ghm_mesh_count", self.h, _vp(err_ptr), int(rows), int(cols), int(err_pitch), int(tile_log2), int(y0), int(x0),
             int(h), int(w), float(max_error), _vp(workspace_ptr), C.byref(V), C.byref(F))
        return int(V.value), int(F.value)

    def mesh_extract(self, src_ptr, pitch, err_ptr, rows, cols, err_pitch, tile_log2, y0, x0, h, w, max_error, workspace_ptr,
                     index_ptr, grid_ptr, heights_ptr, triangles_ptr, vertices, triangles):
        """the same mesh -> index int32 [(h + 1) (w + 1)], grid int32 [vertices, 2], heights fp32 [vertices], triangles
        uint32 [triangles, 3]; the totals are mesh_count's"""
        call("ghm_mesh_extract", self.h, _vp(src_ptr), int(pitch), _vp(err_ptr), int(rows), int(cols), int(err_pitch),
             int(tile_log2), int(y0), int(x0), int(h), int(w), float(max_error), _vp(workspace_ptr), _vp(index_ptr),
             _vp(grid_ptr), _vp(heights_ptr), _vp(triangles_ptr), int(vertices), int(triangles))

    # hydrology (csrc/hydrology.hip, gan_heightmaps_amd/hydrology.py)
    @staticmethod
    def hydrology_workspace(H, W):
        """bytes of device workspace the hydrology entry points need for a plane of H x W, or -1"""
        return int(_lib.load().ghm_hydrology_workspace(int(H), int(W)))

    def hydrology_fill(self, h_ptr, H, W, pitch, tiled, filled_ptr, f_pitch, workspace_ptr, resume=False):
        """the filled surface of the fp32 plane at h_ptr (H x W, rows of ``pitch`` cells) -> the fp32 plane at filled_ptr;
        resume: filled_ptr already holds a surface at or above the answer.  Returns (sweeps, changed); waits for the stream"""
        sweeps, changed = C.c_int64(0), C.c_int32(0)
        call("ghm_hydrology_fill", self.h, _vp(h_ptr), int(H), int(W), int(pitch), int(bool(tiled)), int(bool(resume)),
             _vp(filled_ptr), int(f_pitch), _vp(workspace_ptr), C.byref(sweeps), C.byref(changed))
        return int(sweeps.value), bool(changed.value)

    def hydrology_flats(self, filled_ptr, H, W, f_pitch, tiled, flat_ptr, d_pitch, workspace_ptr):
        """the distance of every cell to the draining rim of its flat -> the int32 plane at flat_ptr.  Returns the sweeps;
        waits for the stream"""
        sweeps = C.c_int64(0)
        call("ghm_hydrology_flats", self.h, _vp(filled_ptr), int(H), int(W), int(f_pitch), int(bool(tiled)), _vp(flat_ptr),
             int(d_pitch), _vp(workspace_ptr), C.byref(sweeps))
        return int(sweeps.value)

    def hydrology_directions(self, filled_ptr, f_pitch, flat_ptr, d_pitch, H, W, dir_ptr, dir_pitch):
        """one of the eight directions, or -1 at an outlet, per cell -> the int8 plane at dir_ptr; asynchronous"""
        call("ghm_hydrology_directions", self.h, _vp(filled_ptr), int(f_pitch), _vp(flat_ptr), int(d_pitch), int(H), int(W),
             _vp(dir_ptr), int(dir_pitch))

    def hydrology_accumulate(self, dir_ptr, dir_pitch, H, W, acc_ptr, a_pitch, basin_ptr, b_pitch, workspace_ptr):
        """the drainage area (uint32) and the outlet (int32, a flat index) of every cell.  Returns the doubling rounds;
        waits for the stream"""
        rounds = C.c_int32(0)
        call("ghm_hydrology_accumulate", self.h, _vp(dir_ptr), int(dir_pitch), int(H), int(W), _vp(acc_ptr), int(a_pitch),
             _vp(basin_ptr), int(b_pitch), _vp(workspace_ptr), C.byref(rounds))
        return int(rounds.value)

    def hydrology_paint(self, depth_ptr, depth_pitch, acc_ptr, a_pitch, H, W, tex_ptr, tex_pitch, channels, colour, opacity,
                        lake_min_depth, river_threshold, river_width, out_u8, out_ptr, out_pitch):
        """the water on a texture of ``channels`` fp32 planes -> out_ptr, fp32 or uint8; colour: three values in the
        texture's range; asynchronous"""
        call("ghm_hydrology_paint", self.h, _vp(depth_ptr), int(depth_pitch), _vp(acc_ptr), int(a_pitch), int(H), int(W),
             _vp(tex_ptr), int(tex_pitch), int(channels), float(colour[0]), float(colour[1]), float(colour[2]),
             float(opacity), float(lake_min_depth), int(river_threshold), int(river_width), int(bool(out_u8)), _vp(out_ptr),
             int(out_pitch))

    # least-cost travel (csrc/route.hip, gan_heightmaps_amd/route.py)
    @staticmethod
    def route_workspace(H, W):
        """bytes of device workspace the route entry points need for a plane of H x W, or -1"""
        return int(_lib.load().ghm_route_workspace(int(H), int(W)))

    def route_weights(self, h_ptr, H, W, pitch, height_scale, grade, lake, ford, river_threshold, lake_min_depth, workspace_ptr,
                      penalty_ptr=None, p_pitch=0, depth_ptr=None, depth_pitch=0, acc_ptr=None, a_pitch=0):
        """the four edge planes of the fp32 plane at h_ptr (H x W, rows of ``pitch`` cells) -> the workspace; penalty (fp32),
        depth (fp32) and accumulation (uint32) planes are optional, None means "not given"; asynchronous"""
        call("ghm_route_weights", self.h, _vp(h_ptr), int(H), int(W), int(pitch), _vp(penalty_ptr), int(p_pitch), _vp(depth_ptr),
             int(depth_pitch), _vp(acc_ptr), int(a_pitch), float(height_scale), float(grade), float(lake), float(ford),
             int(river_threshold), float(lake_min_depth), _vp(workspace_ptr))

    def route_relax(self, H, W, sources, tiled, cost_ptr, c_pitch, workspace_ptr, resume=False):
        """the least cost from ``sources`` (flat indices i W + j) to every cell -> the uint32 plane at cost_ptr, over the edge
        planes route_weights left in the workspace; resume: cost_ptr already holds a plane at or above the answer.  Returns
        (sweeps, changed); waits for the stream"""
        src = np.ascontiguousarray(sources, np.int64).reshape(-1)
        if src.size and (src.min() < -(1 << 31) or src.max() >= 1 << 31):
            raise ValueError("route_relax: a source index does not fit 32 bits")
        src = src.astype(np.int32)
        sweeps, changed = C.c_int64(0), C.c_int32(0)
        call("ghm_route_relax", self.h, int(H), int(W), src.ctypes.data_as(C.POINTER(C.c_int32)) if src.size else None,
             int(src.size), int(bool(tiled)), int(bool(resume)), _vp(cost_ptr), int(c_pitch), _vp(workspace_ptr),
             C.byref(sweeps), C.byref(changed))
        return int(sweeps.value), bool(changed.value)

    def route_parents(self, cost_ptr, c_pitch, H, W, parent_ptr, p_pitch, workspace_ptr):
        """the neighbour every cell leaves through -> the int8 plane at parent_ptr (-1 a source, -2 unreached), in the encoding
        of hydrology_accumulate's directions; asynchronous"""
        call("ghm_route_parents", self.h, _vp(cost_ptr), int(c_pitch), int(H), int(W), _vp(parent_ptr), int(p_pitch),
             _vp(workspace_ptr))

    # earthworks (csrc/earthworks.hip, gan_heightmaps_amd/earthworks.py)
    @staticmethod
    def earthworks_lds_bytes(reach):
        """bytes of LDS a block of the tiled nearest-mark form uses for this reach, or -1 for a reach out of range"""
        return int(_lib.load().ghm_earthworks_lds_bytes(int(reach)))

    def earthworks_nearest(self, marks_ptr, m_pitch, H, W, threshold, reach, tiled, nearest_ptr, n_pitch, dist2_ptr, d_pitch):
        """the nearest marked cell (marks >= threshold, a uint32 plane of H x W in rows of m_pitch cells) within ``reach`` of
        every cell -> its flat index in the int32 plane at nearest_ptr and its squared distance in the one at dist2_ptr, -1 where
        there is none; asynchronous"""
        call("ghm_earthworks_nearest", self.h, _vp(marks_ptr), int(m_pitch), int(H), int(W), int(threshold), int(reach),
             int(bool(tiled)), _vp(nearest_ptr), int(n_pitch), _vp(dist2_ptr), int(d_pitch))

    def earthworks_shape(self, h_ptr, h_pitch, nearest_ptr, n_pitch, dist2_ptr, d_pitch, target_ptr, t_pitch, table_ptr, reach,
                         mode, H, W, out_ptr, o_pitch):
        """the fp32 heights at h_ptr blended towards target[nearest] by the (keep, take) pairs at table_ptr (reach^2 + 1 of
        them, indexed by dist2) -> the fp32 plane at out_ptr; mode 0 both, 1 cut, 2 fill; asynchronous"""
        call("ghm_earthworks_shape", self.h, _vp(h_ptr), int(h_pitch), _vp(nearest_ptr), int(n_pitch), _vp(dist2_ptr),
             int(d_pitch), _vp(target_ptr), int(t_pitch), _vp(table_ptr), int(reach), int(mode), int(H), int(W), _vp(out_ptr),
             int(o_pitch))

    # scatter (csrc/scatter.hip, gan_heightmaps_amd/scatter.py)
    @staticmethod
    def scatter_workspace(H, W):
        """bytes of device workspace scatter_thin needs for a plane of H x W, or -1"""
        return int(_lib.load().ghm_scatter_workspace(int(H), int(W)))

    @staticmethod
    def scatter_lds_bytes(s2):
        """bytes of LDS a block of the tiled thinning uses for this squared spacing, or -1 for an s2 out of range"""
        return int(_lib.load().ghm_scatter_lds_bytes(int(s2)))

    def scatter_chance(self, h_ptr, h_pitch, H, W, tables_ptr, height_scale, density, chance_ptr, c_pitch, dist2_ptr=None,
                       d_pitch=0, water_ptr=None, water_n=0, blocked_ptr=None, b_pitch=0, threshold=1):
        """the chance of every cell of the fp32 plane at h_ptr to be a candidate, in units of 2^-24 -> the uint32 plane at
        chance_ptr; tables_ptr: the 384 fp32 of altitude weights, slope bounds and slope weights; dist2 (int32) with the
        water_n + 1 fp32 weights at water_ptr, and blocked (uint32, >= threshold) are optional; asynchronous"""
        call("ghm_scatter_chance", self.h, _vp(h_ptr), int(h_pitch), int(H), int(W), _vp(tables_ptr), float(height_scale),
             float(density), _vp(dist2_ptr), int(d_pitch), _vp(water_ptr), int(water_n), _vp(blocked_ptr), int(b_pitch),
             int(threshold), _vp(chance_ptr), int(c_pitch))

    def scatter_candidates(self, chance_ptr, c_pitch, H, W, seed, origin, state_ptr, s_pitch, priority_ptr, p_pitch):
        """the candidates (uint8: 1 or 0) and priorities (uint32) of the cells of a plane whose cell [0, 0] lies at the world
        position ``origin`` = (row, col), hashed from the 64-bit seed and the world position; asynchronous"""
        call("ghm_scatter_candidates", self.h, _vp(chance_ptr), int(c_pitch), int(H), int(W), int(seed) & ((1 << 64) - 1),
             int(origin[0]), int(origin[1]), _vp(state_ptr), int(s_pitch), _vp(priority_ptr), int(p_pitch))

    def scatter_thin(self, priority_ptr, p_pitch, state_ptr, s_pitch, H, W, s2, tiled, workspace_ptr):
        """the Poisson-disk thinning of the candidates in the uint8 plane at state_ptr (1 -> 2 kept or 3 rejected), in place:
        no two kept cells with dy^2 + dx^2 < s2, the greedy choice in (priority, row, col) order.  Returns the launches
        issued; waits for the stream"""
        sweeps = C.c_int64(0)
        call("ghm_scatter_thin", self.h, _vp(priority_ptr), int(p_pitch), _vp(state_ptr), int(s_pitch), int(H), int(W), int(s2),
             int(bool(tiled)), _vp(workspace_ptr), C.byref(sweeps))
        return int(sweeps.value)

    # viewshed (csrc/viewshed.hip, gan_heightmaps_amd/viewshed.py)
    @staticmethod
    def viewshed_top_elems(H, W):
        """elements of the int32 plane of block maxima for a plane of H x W, or -1 for a size out of range"""
        return int(_lib.load().ghm_viewshed_top_elems(int(H), int(W)))

    def viewshed_quantise(self, h_ptr, h_pitch, H, W, height_scale, zq_ptr, z_pitch):
        """the fp32 heights at h_ptr (finite, in [0, 1]) -> the int32 plane at zq_ptr, rint(h float32(height_scale 256)), in
        1/256 cell; asynchronous"""
        call("ghm_viewshed_quantise", self.h, _vp(h_ptr), int(h_pitch), int(H), int(W), float(height_scale), _vp(zq_ptr),
             int(z_pitch))

    def viewshed_top(self, zq_ptr, z_pitch, H, W, top_ptr, top_elems):
        """the largest zq of every block of 16 x 16 cells -> the int32 [ceil(H / 16), ceil(W / 16)] at top_ptr; asynchronous"""
        call("ghm_viewshed_top", self.h, _vp(zq_ptr), int(z_pitch), int(H), int(W), _vp(top_ptr), int(top_elems))

    @staticmethod
    def _viewshed_table(observers):
        obs = np.ascontiguousarray(observers, np.int64)
        if obs.ndim != 2 or obs.shape[1] != 4:
            raise ValueError("viewshed: the observers are an integer table [n, 4] of (row, col, eye_q, radius2), got %s" % (obs.shape,))
        if obs.size and (obs.min() < -(1 << 31) or obs.max() >= 1 << 31):
            raise ValueError("viewshed: an observer's field does not fit 32 bits")
        obs = obs.astype(np.int32)
        return obs, (obs.ctypes.data_as(C.POINTER(C.c_int32)) if obs.size else None)

    def viewshed_sight(self, zq_ptr, z_pitch, H, W, observers, target_q, accel, top_ptr, count_ptr, c_pitch, mask_ptr=None,
                       m_pitch=0):
        """the number of ``observers`` -- a host table [n, 4] of (row, col, eye_q, radius2) -- that see each cell of the int32
        plane at zq_ptr -> the uint32 plane at count_ptr, and bit i for observer i -> the one at mask_ptr (optional, n <= 32);
        accel: jump runs of steps the block maxima at top_ptr prove clear (the same bits); asynchronous"""
        obs, ptr = self._viewshed_table(observers)
        call("ghm_viewshed_sight", self.h, _vp(zq_ptr), int(z_pitch), int(H), int(W), ptr, int(obs.shape[0]), int(target_q),
             int(bool(accel)), _vp(top_ptr), _vp(count_ptr), int(c_pitch), _vp(mask_ptr), int(m_pitch))

    def viewshed_steps(self, zq_ptr, z_pitch, H, W, observers, target_q, accel, top_ptr, steps_ptr, s_pitch):
        """viewshed_sight's launches with the steps tested per cell, over all observers -> the uint32 plane at steps_ptr (a
        measuring aid); asynchronous"""
        obs, ptr = self._viewshed_table(observers)
        call("ghm_viewshed_steps", self.h, _vp(zq_ptr), int(z_pitch), int(H), int(W), ptr, int(obs.shape[0]), int(target_q),
             int(bool(accel)), _vp(top_ptr), _vp(steps_ptr), int(s_pitch))

    # sunlight (csrc/sunlight.hip, gan_heightmaps_amd/sunlight.py)
    @staticmethod
    def _sunlight_table(table):
        t = np.ascontiguousarray(table, np.int64)
        if t.ndim != 2 or t.shape[1] != 9:
            raise ValueError("sunlight: the positions are an integer table [n, 9] of (rows, gmaj, gmin, m_q, rise_q, s_y, s_x, s_z, w_q), "
                             "got %s" % (t.shape,))
        return t, (t.ctypes.data_as(C.POINTER(C.c_int64)) if t.size else None)

    def sunlight_zmax(self, top_ptr, top_elems, zmax_ptr):
        """the largest of the block maxima at top_ptr -> the int32 word at zmax_ptr; asynchronous"""
        call("ghm_sunlight_zmax", self.h, _vp(top_ptr), int(top_elems), _vp(zmax_ptr))

    def sunlight_sun(self, zq_ptr, z_pitch, H, W, table, target_q, accel, top_ptr, zmax_ptr, lit_ptr, l_pitch, mask_ptr, m_pitch,
                     hours_ptr, h_pitch, energy_ptr, e_pitch):
        """the sun positions of ``table`` -- a host table [n, 9] of (rows, gmaj, gmin, m_q, rise_q, s_y, s_x, s_z, w_q) -- over the
        int32 plane at zq_ptr -> four uint32 planes: the positions that light each cell at lit_ptr, bit i for position i at
        mask_ptr (optional, n <= 32), their hours in 1/256 at hours_ptr and the energy on the cell's slope at energy_ptr; accel:
        jump runs of steps the block maxima at top_ptr prove clear (the same bits); zmax_ptr: sunlight_zmax's word; asynchronous"""
        t, ptr = self._sunlight_table(table)
        call("ghm_sunlight_sun", self.h, _vp(zq_ptr), int(z_pitch), int(H), int(W), ptr, int(t.shape[0]), int(target_q),
             int(bool(accel)), _vp(top_ptr), _vp(zmax_ptr), _vp(lit_ptr), int(l_pitch), _vp(mask_ptr), int(m_pitch), _vp(hours_ptr),
             int(h_pitch), _vp(energy_ptr), int(e_pitch))

    def sunlight_steps(self, zq_ptr, z_pitch, H, W, table, target_q, accel, top_ptr, zmax_ptr, steps_ptr, s_pitch):
        """sunlight_sun's launches with the steps tested per cell, over all positions -> the uint32 plane at steps_ptr (a
        measuring aid); asynchronous"""
        t, ptr = self._sunlight_table(table)
        call("ghm_sunlight_steps", self.h, _vp(zq_ptr), int(z_pitch), int(H), int(W), ptr, int(t.shape[0]), int(target_q),
             int(bool(accel)), _vp(top_ptr), _vp(zmax_ptr), _vp(steps_ptr), int(s_pitch))

    # contours (csrc/contour.hip, gan_heightmaps_amd/contour.py)
    @staticmethod
    def contour_cells_bytes(H, W):
        """bytes of the cells' buffer contour_count fills for a plane of H x W, or -1 for a size out of range"""
        return int(_lib.load().ghm_contour_cells_bytes(int(H), int(W)))

    @staticmethod
    def contour_workspace(H, W, segments):
        """bytes of device workspace contour_trace needs for a plane of H x W with this many segments, or -1"""
        return int(_lib.load().ghm_contour_workspace(int(H), int(W), int(segments)))

    def contour_count(self, zq_ptr, z_pitch, H, W, base_q, interval_q, count, cells_ptr):
        """the contour segments of every cell of the int32 plane at zq_ptr for the levels 2 (base_q + j interval_q) + 1 (count:
        -1 for every j, or the j in [0, count)) and their exclusive scan -> the buffer at cells_ptr.  Returns their number; waits
        for the stream"""
        segments = C.c_int64(0)
        call("ghm_contour_count", self.h, _vp(zq_ptr), int(z_pitch), int(H), int(W), int(base_q), int(interval_q), int(count),
             _vp(cells_ptr), C.byref(segments))
        return int(segments.value)

    def contour_trace(self, zq_ptr, z_pitch, H, W, base_q, interval_q, count, cells_ptr, workspace_ptr, segments):
        """links the segments contour_count counted and ranks them along their lines, in the workspace.  Returns (lines,
        vertices, the ranking's doubling rounds); waits for the stream"""
        lines, vertices, rounds = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        call("ghm_contour_trace", self.h, _vp(zq_ptr), int(z_pitch), int(H), int(W), int(base_q), int(interval_q), int(count),
             _vp(cells_ptr), _vp(workspace_ptr), int(segments), C.byref(lines), C.byref(vertices), C.byref(rounds))
        return int(lines.value), int(vertices.value), int(rounds.value)

    def contour_extract(self, zq_ptr, z_pitch, H, W, base_q, interval_q, count, cells_ptr, workspace_ptr, segments, lines, vertices,
                        edge_ptr, t_ptr, offsets_ptr, level_ptr, closed_ptr):
        """the traced lines -> edge int32 [V, 3], t float64 [V], offsets int64 [L + 1], level int32 [L], closed uint8 [L]; the
        totals are contour_trace's; asynchronous once it has compared them with the workspace's"""
        call("ghm_contour_extract", self.h, _vp(zq_ptr), int(z_pitch), int(H), int(W), int(base_q), int(interval_q), int(count),
             _vp(cells_ptr), _vp(workspace_ptr), int(segments), int(lines), int(vertices), _vp(edge_ptr), _vp(t_ptr),
             _vp(offsets_ptr), _vp(level_ptr), _vp(closed_ptr))

    def contour_marks(self, zq_ptr, z_pitch, H, W, base_q, interval_q, count, index_every, marks_ptr, m_pitch):
        """0, 1 (a level between a cell and its right or lower neighbour) or 2 (an index contour: j % index_every == 0) -> the
        uint32 plane at marks_ptr; asynchronous"""
        call("ghm_contour_marks", self.h, _vp(zq_ptr), int(z_pitch), int(H), int(W), int(base_q), int(interval_q), int(count),
             int(index_every), _vp(marks_ptr), int(m_pitch))

    # peaks (csrc/peaks.hip, gan_heightmaps_amd/peaks.py)
    @staticmethod
    def peaks_workspace(H, W):
        """bytes of device workspace peaks_count / peaks_tree / peaks_extract need for a plane of H x W, or -1"""
        return int(_lib.load().ghm_peaks_workspace(int(H), int(W)))

    @staticmethod
    def peaks_list_bytes(edges):
        """bytes of the list buffer the list form of peaks_tree needs for this many edges, or -1"""
        return int(_lib.load().ghm_peaks_list_bytes(int(edges)))

    def peaks_ascent(self, zq_ptr, z_pitch, H, W, ascent_ptr, a_pitch):
        """the direction of every cell's neighbour of greatest key (zq, row W + col) if that is above its own, else -1 (a
        summit) -> the int8 plane at ascent_ptr, in hydrology_accumulate's encoding; asynchronous"""
        call("ghm_peaks_ascent", self.h, _vp(zq_ptr), int(z_pitch), int(H), int(W), _vp(ascent_ptr), int(a_pitch))

    def peaks_count(self, zq_ptr, z_pitch, label_ptr, l_pitch, H, W, workspace_ptr):
        """numbers the summits (label == the cell's own index) and the edges between regions in the workspace.  Returns
        (summits, edges); waits for the stream"""
        summits, edges = C.c_int64(0), C.c_int64(0)
        call("ghm_peaks_count", self.h, _vp(zq_ptr), int(z_pitch), _vp(label_ptr), int(l_pitch), int(H), int(W), _vp(workspace_ptr),
             C.byref(summits), C.byref(edges))
        return int(summits.value), int(edges.value)

    def peaks_tree(self, zq_ptr, z_pitch, label_ptr, l_pitch, H, W, form, mask_ptr, m_pitch, workspace_ptr, list_ptr, summits,
                   edges, max_rounds=32):
        """the maximum spanning tree of the summits by Boruvka rounds, its edges marked in the uint32 plane at mask_ptr (bit k of
        cell c); form: 0 plain, 1 list (list_ptr: peaks_list_bytes(edges) bytes; else None).  Returns the rounds; waits for
        the stream"""
        rounds = C.c_int32(0)
        call("ghm_peaks_tree", self.h, _vp(zq_ptr), int(z_pitch), _vp(label_ptr), int(l_pitch), int(H), int(W), int(form),
             int(max_rounds), _vp(mask_ptr), int(m_pitch), _vp(workspace_ptr), _vp(list_ptr), int(summits), int(edges),
             C.byref(rounds))
        return int(rounds.value)

    def peaks_extract(self, label_ptr, l_pitch, area_ptr, a_pitch, mask_ptr, m_pitch, H, W, workspace_ptr, summits, summit_ptr,
                      area_out_ptr, tree_ptr):
        """the summits int32 [P] (flat indices, ascending), their areas uint32 [P] and the tree's rows int32 [P - 1, 3] = (cell,
        its label, the label across) from the workspace of peaks_tree; asynchronous once it has read the totals"""
        call("ghm_peaks_extract", self.h, _vp(label_ptr), int(l_pitch), _vp(area_ptr), int(a_pitch), _vp(mask_ptr), int(m_pitch),
             int(H), int(W), _vp(workspace_ptr), int(summits), _vp(summit_ptr), _vp(area_out_ptr), _vp(tree_ptr))

    @staticmethod
    def peaks_merge(summit, summit_zq, tree, saddle_zq, min_zq):
        """the host's part (no device): every summit's col (flat index or -1), parent (a summit's number or -1) and prominence
        in quanta from the extracted summits and tree rows and the heights at both.  Returns (col, parent, prominence_q), int32"""
        summit, summit_zq = np.ascontiguousarray(summit, np.int32), np.ascontiguousarray(summit_zq, np.int32)
        tree, saddle_zq = np.ascontiguousarray(tree, np.int32).reshape(-1, 3), np.ascontiguousarray(saddle_zq, np.int32)
        P, T = summit.shape[0], tree.shape[0]
        if summit_zq.shape != (P,) or saddle_zq.shape != (T,):
            raise ValueError("peaks_merge: %d summits with %d heights, %d edges with %d" % (P, summit_zq.size, T, saddle_zq.size))
        col, parent, prom = np.empty(P, np.int32), np.empty(P, np.int32), np.empty(P, np.int32)
        _lib.load()
        call("ghm_peaks_merge", summit.ctypes.data, summit_zq.ctypes.data, P, tree.ctypes.data if T else None,
             saddle_zq.ctypes.data if T else None, T, int(min_zq), col.ctypes.data, parent.ctypes.data, prom.ctypes.data)
        return col, parent, prom

    # rivers (csrc/rivers.hip, gan_heightmaps_amd/rivers.py)
    @staticmethod
    def rivers_workspace(H, W):
        """bytes of device workspace rivers_count / rivers_trace / rivers_extract need for a plane of H x W, or -1"""
        return int(_lib.load().ghm_rivers_workspace(int(H), int(W)))

    @staticmethod
    def rivers_list_bytes(cells):
        """bytes of the list buffer the list form of rivers_trace needs for this many stream cells, or -1"""
        return int(_lib.load().ghm_rivers_list_bytes(int(cells)))

    def rivers_count(self, dir_ptr, d_pitch, acc_ptr, a_pitch, H, W, threshold, kind_ptr, k_pitch, workspace_ptr):
        """the stream cells (accumulation >= threshold) of the int8 direction and uint32 accumulation planes: their kind -> the
        uint8 plane at kind_ptr, the reach starts and the stream cells numbered in the workspace.  Returns (cells, reaches,
        sources, confluences, mouths, isolated); waits for the stream"""
        counts = (C.c_int64 * 6)()
        call("ghm_rivers_count", self.h, _vp(dir_ptr), int(d_pitch), _vp(acc_ptr), int(a_pitch), int(H), int(W), int(threshold),
             _vp(kind_ptr), int(k_pitch), _vp(workspace_ptr), counts)
        return tuple(int(v) for v in counts)

    def rivers_trace(self, dir_ptr, d_pitch, kind_ptr, k_pitch, H, W, form, workspace_ptr, list_ptr, cells, reaches, max_rounds=32):
        """ranks the cells along their reaches by pointer doubling and stores every reach's length and downstream reach in the
        workspace; form: 0 plain, 1 list (list_ptr: rivers_list_bytes(cells) bytes; else None).  Returns (vertices, the rounds
        that moved a pointer); waits for the stream"""
        vertices, rounds = C.c_int64(0), C.c_int32(0)
        call("ghm_rivers_trace", self.h, _vp(dir_ptr), int(d_pitch), _vp(kind_ptr), int(k_pitch), int(H), int(W), int(form),
             int(max_rounds), _vp(workspace_ptr), _vp(list_ptr), int(cells), int(reaches), C.byref(vertices), C.byref(rounds))
        return int(vertices.value), int(rounds.value)

    def rivers_extract(self, dir_ptr, d_pitch, kind_ptr, k_pitch, H, W, workspace_ptr, list_ptr, cells, reaches, vertices, vertex_ptr,
                       offsets_ptr, downstream_ptr):
        """the traced reaches -> vertex int32 [V] (flat indices, reach by reach, downstream), offsets int64 [R + 1], downstream
        int32 [R]; the totals are rivers_count's and rivers_trace's; asynchronous once it has compared them with the workspace's"""
        call("ghm_rivers_extract", self.h, _vp(dir_ptr), int(d_pitch), _vp(kind_ptr), int(k_pitch), int(H), int(W), _vp(workspace_ptr),
             _vp(list_ptr), int(cells), int(reaches), int(vertices), _vp(vertex_ptr), _vp(offsets_ptr), _vp(downstream_ptr))

    @staticmethod
    def rivers_order(downstream, area):
        """the host's part (no device): every reach's Strahler order, Shreve magnitude (int32 each) and whether it is the main
        stem where it ends (uint8), from the reaches' downstream reach (or -1) and their areas.  Returns (order, magnitude, main)"""
        downstream, area = np.ascontiguousarray(downstream, np.int32), np.ascontiguousarray(area, np.uint32)
        R = downstream.shape[0]
        if downstream.ndim != 1 or area.shape != (R,):
            raise ValueError("rivers_order: %d reaches with %d areas" % (downstream.size, area.size))
        order, magnitude, main = np.empty(R, np.int32), np.empty(R, np.int32), np.empty(R, np.uint8)
        _lib.load()
        call("ghm_rivers_order", downstream.ctypes.data if R else None, area.ctypes.data if R else None, R,
             order.ctypes.data if R else None, magnitude.ctypes.data if R else None, main.ctypes.data if R else None)
        return order, magnitude, main

    # regions (csrc/regions.hip, gan_heightmaps_amd/regions.py)
    @staticmethod
    def regions_workspace(H, W):
        """bytes of device workspace regions_label / _count / _trace / _extract need for a plane of H x W, or -1"""
        return int(_lib.load().ghm_regions_workspace(int(H), int(W)))

    @staticmethod
    def regions_trace_bytes(edges):
        """bytes of the per-edge buffers regions_trace needs for this many boundary edges, or -1"""
        return int(_lib.load().ghm_regions_trace_bytes(int(edges)))

    def regions_label(self, labels_ptr, l_pitch, H, W, form, component_ptr, c_pitch, workspace_ptr):
        """the int32 label plane (negative: no region) -> the int32 component plane: the least flat index of every cell's
        4-connected component of equal labels, -1 for none; form: 0 sweep, 1 union, the same bits.  Returns the sweeps issued, 0
        if no cell has a region; waits for the stream"""
        sweeps = C.c_int64(0)
        call("ghm_regions_label", self.h, _vp(labels_ptr), int(l_pitch), int(H), int(W), int(form), _vp(component_ptr), int(c_pitch),
             _vp(workspace_ptr), C.byref(sweeps))
        return int(sweeps.value)

    def regions_count(self, labels_ptr, l_pitch, component_ptr, c_pitch, H, W, workspace_ptr, max_edges=(1 << 31) - 1):
        """numbers the boundary edges and the polygons of a labelled plane in the workspace and counts the polygons' cells; more
        than max_edges edges are refused.  Returns (edges, polygons); waits for the stream"""
        counts = (C.c_int64 * 2)()
        call("ghm_regions_count", self.h, _vp(labels_ptr), int(l_pitch), _vp(component_ptr), int(c_pitch), int(H), int(W),
             int(max_edges), _vp(workspace_ptr), counts)
        return int(counts[0]), int(counts[1])

    def regions_trace(self, H, W, workspace_ptr, trace_ptr, edges, polygons, max_rounds=32):
        """links the counted edges into rings, finds every ring's least edge and ranks the edges with their corner counts by
        pointer doubling, in the buffer at trace_ptr (regions_trace_bytes(edges) bytes).  Returns (rings, vertices, the ranking's
        rounds that moved a pointer); waits for the stream"""
        counts, rounds = (C.c_int64 * 2)(), C.c_int32(0)
        call("ghm_regions_trace", self.h, int(H), int(W), int(max_rounds), _vp(workspace_ptr), _vp(trace_ptr), int(edges), int(polygons),
             counts, C.byref(rounds))
        return int(counts[0]), int(counts[1]), int(rounds.value)

    def regions_extract(self, labels_ptr, l_pitch, component_ptr, c_pitch, H, W, workspace_ptr, trace_ptr, edges, polygons, rings,
                        vertices, vertex_ptr, ring_offsets_ptr, ring_polygon_ptr, ring_hole_ptr, seed_ptr, label_ptr, cells_ptr,
                        polygon_ptr=None, p_pitch=0):
        """the traced rings -> vertex int32 [V] (grid corners row (W + 1) + col), ring_offsets int64 [R + 1], ring_polygon int32
        [R], ring_hole uint8 [R], seed and label int32 [P], cells uint32 [P] and, if polygon_ptr is given, the polygon of every
        cell, int32 in rows of p_pitch cells; the totals are regions_count's and regions_trace's; asynchronous once it has
        compared them with the workspace's"""
        call("ghm_regions_extract", self.h, _vp(labels_ptr), int(l_pitch), _vp(component_ptr), int(c_pitch), int(H), int(W),
             _vp(workspace_ptr), _vp(trace_ptr), int(edges), int(polygons), int(rings), int(vertices), _vp(vertex_ptr),
             _vp(ring_offsets_ptr), _vp(ring_polygon_ptr), _vp(ring_hole_ptr), _vp(seed_ptr), _vp(label_ptr), _vp(cells_ptr),
             _vp(polygon_ptr), int(p_pitch))

    # climate (csrc/climate.hip, gan_heightmaps_amd/climate.py)
    @staticmethod
    def climate_workspace(H, W):
        """bytes of device workspace climate_discharge needs for a plane of H x W, or -1"""
        return int(_lib.load().ghm_climate_workspace(int(H), int(W)))

    def climate_transport(self, zq_ptr, z_pitch, H, W, wind, form, sea_q, hum_q, evap_q, base_q, up_q, rec_q, raw_ptr, r_pitch):
        """the rain every wind line drops, cell by cell: the int32 plane of quantised heights -> the uint32 plane at raw_ptr.
        wind: 0 .. 7 = N NE E SE S SW W NW, where it comes from; form: 0 line, 1 staged, the same bits; asynchronous"""
        call("ghm_climate_transport", self.h, _vp(zq_ptr), int(z_pitch), int(H), int(W), int(wind), int(form), int(sea_q), int(hum_q),
             int(evap_q), int(base_q), int(up_q), int(rec_q), _vp(raw_ptr), int(r_pitch))

    def climate_spread(self, raw_ptr, r_pitch, H, W, spread, rain_ptr, o_pitch):
        """the floor of the mean of raw over the (2 spread + 1)^2 window, clamped at the edges -> the uint32 plane at rain_ptr;
        asynchronous"""
        call("ghm_climate_spread", self.h, _vp(raw_ptr), int(r_pitch), int(H), int(W), int(spread), _vp(rain_ptr), int(o_pitch))

    def climate_biome(self, zq_ptr, z_pitch, rain_ptr, r_pitch, H, W, sea_q, t0_q, lapse_q, lat_q, origin_row, t_edges, r_edges, table,
                      ocean, temperature_ptr, t_pitch, biome_ptr, b_pitch):
        """temperature (int32, 1/256 degree) and the biome label (int32) of every cell; t_edges, r_edges: quantised edges, ascending;
        table: (len(t_edges) + 1) x (len(r_edges) + 1) labels, row-major; they travel by value; asynchronous"""
        te, re_, tb = (np.ascontiguousarray(x, np.int32).reshape(-1) for x in (t_edges, r_edges, table))
        if tb.size != (te.size + 1) * (re_.size + 1):
            raise ValueError("the table has %d labels for %d x %d edges" % (tb.size, te.size, re_.size))
        call("ghm_climate_biome", self.h, _vp(zq_ptr), int(z_pitch), _vp(rain_ptr), int(r_pitch), int(H), int(W), int(sea_q), int(t0_q),
             int(lapse_q), int(lat_q), int(origin_row), te.ctypes.data if te.size else None, int(te.size),
             re_.ctypes.data if re_.size else None, int(re_.size), tb.ctypes.data, int(ocean), _vp(temperature_ptr), int(t_pitch),
             _vp(biome_ptr), int(b_pitch))

    def climate_discharge(self, dir_ptr, d_pitch, rain_ptr, r_pitch, H, W, ref_q, discharge_ptr, q_pitch, effective_ptr, e_pitch,
                          workspace_ptr):
        """the rain that drains through every cell (uint64) and min(that // ref_q, 2^32 - 1) (uint32) over the hydrology's
        directions.  Returns the doubling rounds; waits for the stream"""
        rounds = C.c_int32(0)
        call("ghm_climate_discharge", self.h, _vp(dir_ptr), int(d_pitch), _vp(rain_ptr), int(r_pitch), int(H), int(W), int(ref_q),
             _vp(discharge_ptr), int(q_pitch), _vp(effective_ptr), int(e_pitch), _vp(workspace_ptr), C.byref(rounds))
        return int(rounds.value)

    def climate_paint(self, biome_ptr, b_pitch, H, W, tex_ptr, tex_pitch, channels, palette, opacity, out_u8, out_ptr, out_pitch):
        """the biomes on a texture of ``channels`` fp32 planes -> out_ptr, fp32 or uint8; palette: float32 [labels, 4] on the host,
        (r, g, b, has) in the texture's range, a row with has <= 0 leaves its biome's pixels alone; asynchronous"""
        pal = np.ascontiguousarray(palette, np.float32).reshape(-1, 4)
        call("ghm_climate_paint", self.h, _vp(biome_ptr), int(b_pitch), int(H), int(W), _vp(tex_ptr), int(tex_pitch), int(channels),
             pal.ctypes.data if pal.size else None, int(pal.shape[0]), float(opacity), int(bool(out_u8)), _vp(out_ptr), int(out_pitch))

    # hydraulic erosion (csrc/erosion.hip, gan_heightmaps_amd/erosion.py)
    @staticmethod
    def erosion_tile():
        """(rows, columns) of the fused form's tile"""
        lib = _lib.load()
        return int(lib.ghm_erosion_tile(0)), int(lib.ghm_erosion_tile(1))

    def erosion_init(self, hm_ptr, H, W, src_pitch, height_scale, state_ptr, pitch):
        """the fp32 heightmap at hm_ptr (H rows of src_pitch cells, in [0, 1]) -> the state at state_ptr: EROSION_PLANES
        planes of H rows of ``pitch`` cells, b = heightmap * height_scale, the rest 0"""
        call("ghm_erosion_init", self.h, _vp(hm_ptr), int(H), int(W), int(src_pitch), float(height_scale), _vp(state_ptr),
             int(pitch))

    def erosion_iterate(self, params, state0, state1, tmp, H, W, pitch, iterations, fused):
        """``iterations`` steps from state0, alternating between the two states -> the pointer of the state that holds the
        result.  params: an ErosionParams (erosion_params()); tmp: three planes, needed by the plain form only"""
        call("ghm_erosion_iterate", self.h, C.byref(params) if params is not None else None, _vp(state0), _vp(state1),
             _vp(tmp), int(H), int(W), int(pitch), int(iterations), int(bool(fused)))
        return state0 if iterations % 2 == 0 else state1

    def erosion_emit(self, state_ptr, H, W, pitch, height_scale, r0, c0, nr, nc, out_u8, out_ptr, out_rows, out_pitch,
                     yoff=0, xoff=0):
        """clamp(b / height_scale, 0, 1) of rows [r0, r0 + nr) x columns [c0, c0 + nc) of the state -> rows yoff ..,
        columns xoff .. of the plane at out_ptr (out_rows rows of out_pitch cells), fp32 or uint8"""
        call("ghm_erosion_emit", self.h, _vp(state_ptr), int(H), int(W), int(pitch), float(height_scale), int(r0), int(c0),
             int(nr), int(nc), int(bool(out_u8)), _vp(out_ptr), int(out_rows), int(out_pitch), int(yoff), int(xoff))

    # sliced Wasserstein distance (csrc/swd.hip, gan_heightmaps_amd/swd.py)
    @staticmethod
    def swd_workspace():
        """bytes of device workspace swd_stats and swd_l1 need"""
        return int(_lib.load().ghm_swd_workspace())

    @staticmethod
    def swd_sort_max_chunk():
        """the longest (padded) column one workgroup sorts in LDS"""
        return int(_lib.load().ghm_swd_sort_max_chunk())

    def swd_pyramid_level(self, g, pitch, g_next_ptr, next_pitch, lap_ptr, lap_pitch):
        """g: a DevTensor view [n, C, H, W] of level G_i whose rows lie ``pitch`` cells apart (None: W) -> G_{i+1} at
        g_next_ptr ([n, C, H/2, next_pitch]; None: the coarsest level, Lap = G) and Lap_i at lap_ptr ([n, C, H, lap_pitch])"""
        n, Cc, H, W = g.shape
        pitch = W if pitch is None else int(pitch)
        call("ghm_swd_pyramid_level", self.h, _vp(g.ptr), n, Cc, H, W, g.nstride, H * pitch, pitch, _vp(g_next_ptr),
             int(next_pitch), _vp(lap_ptr), int(lap_pitch))

    def swd_gather(self, img_ptr, n, Cc, H, W, pitch, corners_ptr, patches, desc_ptr, row_offset, total_rows):
        """the C x 7 x 7 windows of the images at img_ptr ([n, C, H, pitch]) at the int32 (row, column) corners on the device
        -> rows row_offset .. of the [total_rows, 49 C] matrix at desc_ptr"""
        call("ghm_swd_gather", self.h, _vp(img_ptr), int(n), int(Cc), int(H), int(W), int(pitch), _vp(corners_ptr),
             int(patches), _vp(desc_ptr), int(row_offset), int(total_rows))

    def swd_stats(self, desc_ptr, N, Cc, stats_ptr, workspace_ptr):
        """(mean, population standard deviation) per channel of the [N, 49 C] matrix -> 2 C floats at stats_ptr"""
        call("ghm_swd_stats", self.h, _vp(desc_ptr), int(N), int(Cc), _vp(stats_ptr), _vp(workspace_ptr))

    def swd_project(self, desc_ptr, N, Cc, dirs_ptr, M, stats_ptr, out_ptr):
        """the normalised [N, 49 C] descriptors times the [49 C, M] directions -> [M, N] at out_ptr"""
        call("ghm_swd_project", self.h, _vp(desc_ptr), int(N), int(Cc), _vp(dirs_ptr), int(M), _vp(stats_ptr), _vp(out_ptr))

    def swd_sort_columns(self, data_ptr, N, M, chunk=0):
        """sort each of the M columns of N floats at data_ptr ([M, N]) ascending in place; chunk: the cells a workgroup holds in
        LDS (0: the largest) -- a longer column goes through the global form"""
        call("ghm_swd_sort_columns", self.h, _vp(data_ptr), int(N), int(M), int(chunk))

    def swd_l1(self, a_ptr, b_ptr, n, workspace_ptr):
        """mean |a - b| over n floats, as a Python float (waits for the stream)"""
        r = C.c_double(0.0)
        call("ghm_swd_l1", self.h, _vp(a_ptr), _vp(b_ptr), int(n), _vp(workspace_ptr), C.byref(r))
        return r.value

    def lsgan_loss(self, d, target, loss_out, grad=None, grad_scale=1.0, accumulate_loss=False):
        assert d.contiguous
        call("ghm_lsgan_loss", self.h, _vp(d), d.size, target, _vp(loss_out), _vp(grad), grad_scale,
             int(accumulate_loss))

    def bce_loss(self, d, target, loss_out, grad=None, grad_scale=1.0, accumulate_loss=False):
        assert d.contiguous
        call("ghm_bce_loss", self.h, _vp(d), d.size, target, _vp(loss_out), _vp(grad), grad_scale,
             int(accumulate_loss))

    def recon_loss(self, a, b, loss_out, grad=None, grad_scale=1.0, l2=False, accumulate_grad=False):
        call("ghm_recon_loss", self.h, _vp(a), a.nstride, _vp(b), b.nstride, a.N, a.Cc, a.HW, int(l2), _vp(loss_out),
             _vp(grad), grad.nstride if grad is not None else 0, grad_scale, int(accumulate_grad))

    def rmsprop(self, p, g, acc, n, hyper, rho=0.9, eps=1e-6, grad_scale=1.0):
        call("ghm_rmsprop", self.h, _vp(p), _vp(g), _vp(acc), int(n), _vp(hyper), rho, eps, grad_scale)

    def adam(self, p, g, m, v, n, hyper, b1=0.9, b2=0.999, eps=1e-8, grad_scale=1.0):
        call("ghm_adam", self.h, _vp(p), _vp(g), _vp(m), _vp(v), int(n), _vp(hyper), b1, b2, eps, grad_scale)

    def adam_tick(self, hyper):
        call("ghm_adam_tick", self.h, _vp(hyper))

    def opt_update(self, rule, p, g, states, n, hyper, h=(), grad_scale=1.0):
        """ghm_opt_update: ``rule`` a key of OPT_RULES, ``states`` its state buffers in the header's s0.. order, ``h`` its
        constants h0.. (the table in include/ghm.h)"""
        s = list(states) + [None] * (3 - len(states))
        h = [float(v) for v in h] + [0.0] * (3 - len(h))
        call("ghm_opt_update", self.h, OPT_RULES[rule], _vp(p), _vp(g), _vp(s[0]), _vp(s[1]), _vp(s[2]), int(n), _vp(hyper),
             h[0], h[1], h[2], grad_scale)

    def ema_update(self, ema, w, n, decay):
        """ghm_ema_update: ema[:n] = decay * ema[:n] + (1 - decay) * w[:n] (skipped with the update of an overflowed fp16 step)"""
        call("ghm_ema_update", self.h, _vp(ema), _vp(w), int(n), float(decay))

    def swap_f32(self, a, b, n):
        """ghm_swap_f32: exchange a[:n] and b[:n], bit for bit"""
        call("ghm_swap_f32", self.h, _vp(a), _vp(b), int(n))

    def grad_check(self, g, n):
        call("ghm_grad_check", self.h, _vp(g), int(n))

    def loss_scale_update(self, growth_interval=2000, min_scale=1.0, max_scale=2.0 ** 24):
        call("ghm_loss_scale_update", self.h, int(growth_interval), float(min_scale), float(max_scale))

    def allreduce_sum(self, buf, n):
        call("ghm_allreduce_sum", self.h, _vp(buf), int(n))

    def allreduce_sum_bf16(self, buf, n, scratch_ptr):
        """the sum through a bf16 exchange buffer (``scratch_ptr``: n halfwords of device memory): half the bytes, reduced precision"""
        call("ghm_allreduce_sum_bf16", self.h, _vp(buf), int(n), C.c_void_p(int(scratch_ptr)))

    def reduce_scatter_sum(self, buf, shard):
        """buf = world x shard elements: this rank's shard receives the sum over the ranks (in place)"""
        call("ghm_reduce_scatter_sum", self.h, _vp(buf), int(shard))

    def all_gather(self, buf, shard):
        """buf = world x shard elements: every rank's shard is made whole on every rank (in place)"""
        call("ghm_all_gather", self.h, _vp(buf), int(shard))

    def allreduce_max(self, buf, n):
        call("ghm_allreduce_max", self.h, _vp(buf), int(n))

    def conv_variant(self, d, kind):
        out = C.create_string_buffer(128)
        call("ghm_conv2d_variant", C.byref(d), kind, out, 128)
        return out.value.decode()
