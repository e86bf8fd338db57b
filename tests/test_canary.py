"""tests/canary.py on a host-memory stand-in for the device: that a stray write is reported where it should be and only
there, that a flipped input bit is noticed, that the ledger fails just above its bound and counts every comparison, and that
the buffers of every family lie in their allocations exactly where the kernel tests' former classes put them (the literal
numbers below were computed with those classes on this stand-in before they were replaced)."""
import zlib

import numpy as np
import pytest

from gan_heightmaps_amd import device as D
from tests import canary
from tests.elementwise_q_ref import CANARY, U


class HostDevice:
    """alloc / free / h2d / d2h / sync / _allocs of device.Device over a bytearray, addresses 16-byte aligned.  DevTensor and
    QTensor move their data through h2d / d2h alone, so they work on it unchanged"""

    def __init__(self, nbytes=1 << 23):
        self.mem = bytearray(nbytes)
        self._allocs = {}
        self._next = 4096

    def alloc(self, nbytes):
        p = self._next
        self._next += (max(int(nbytes), 16) + 15) // 16 * 16
        assert self._next <= len(self.mem)
        self._allocs[p] = nbytes
        return p

    def free(self, ptr):
        self._allocs.pop(ptr, None)

    def h2d(self, ptr, arr):
        raw = np.ascontiguousarray(arr).tobytes()
        self.mem[ptr:ptr + len(raw)] = raw

    def d2h(self, arr, ptr, nbytes):
        arr.reshape(-1).view(np.uint8)[:nbytes] = np.frombuffer(self.mem, np.uint8, nbytes, ptr)

    def sync(self):
        pass

    def poke(self, ptr, halfword=0x3c00):
        """what a kernel's stray 16-bit store does"""
        self.h2d(ptr, np.array([halfword], np.uint16))


    def close(self):
        self.closed = True


# the module's ``gpu`` and ``mem`` come from the harness's own factory, over the stand-in
LEDGER = canary.Ledger(lambda key, w, r, n: "measured %s %.3f %.2e %d" % (key, w, r, n))
CACHE = {}
DEVICES = []
gpu, mem = canary.fixtures(LEDGER, CACHE)


@pytest.fixture(scope="module", autouse=True)
def host_device():
    """device.Device / Ops / device_count answer with the stand-in while this module runs; afterwards: the device the factory
    made was closed, the cache emptied"""
    saved = D.device_count, D.Device, D.Ops
    D.device_count, D.Device, D.Ops = (lambda: 1), (lambda index: DEVICES.append(HostDevice()) or DEVICES[-1]), (lambda dev: None)
    yield
    D.device_count, D.Device, D.Ops = saved


def crc(mask):
    return zlib.crc32(np.packbits(mask).tobytes())


# ---- layouts: (bytes from the allocation to the view, strides, total, halfwords inside, crc32 of the packed mask) ----
def test_fp32_view_layouts(gpu, mem):
    rows = [(canary.View.free, ((3, 5, 7, 9), (0, 0)), (0, 315, 953, 1890, 0xb48ccd3a)),
            (canary.View.free, ((3, 5, 7, 9), (3, 5)), (12, 320, 966, 1890, 0xacfe5ae2)),
            (canary.View.free, ((7,), (3, 0)), (12, 7, 18, 14, 0xea43f8ec)),
            (canary.View.named, ((2, 8, 4, 4), 'whole'), (4096, 128, 2304, 512, 0xb55b7931)),
            (canary.View.named, ((2, 8, 4, 4), 'slice'), (4608, 384, 2816, 512, 0xed180e48)),
            (canary.View.named, ((2, 8, 4, 4), 'offset'), (4176, 128, 2324, 512, 0xd100f620)),
            (canary.View.framed, ((2, 6, 16, 12), 'slice'), (768, 1536, 3072, 4608, 0xaeadcf5b)),
            (canary.View.framed, ((2, 6, 16, 12), 'whole'), (0, 1152, 2496, 4608, 0x5a4fc2f0))]
    for make, args, want in rows:
        v = make(gpu, *args)
        assert (v.t.ptr - v.ptr, v.t.nstride, v.total, int(v.inside.sum()), crc(v.inside)) == want, (make.__name__, args)
        assert v.span == 4 * v.total == gpu[0]._allocs[v.base] and v.inside.size == 2 * v.total
        assert v.stray().size == 0 and np.isnan(v.numpy()).all()


def test_q_view_layouts(gpu, mem):
    rows = [(canary.QView.named, ((2, 16, 4, 4), 'bf16x3', 'slice'), (4352, 64, 128, 896, 1536, 0x2243a484)),
            (canary.QView.named, ((2, 16, 4, 4), 'bf16x3', 'offset'), (4112, 32, 64, 705, 1536, 0xc11e9961)),
            (canary.QView.named, ((2, 16, 4, 4), 'bf16x3', 'whole'), (4096, 32, 64, 704, 1536, 0xf0c611fb)),
            (canary.QView.framed, ((2, 16, 4, 4), 'bf16x2', 'whole'), (0, 32, 64, 192, 1024, 0x70e76ac1)),
            (canary.QView.framed, ((2, 16, 4, 4), 'bf16x2', 'slice'), (256, 64, 128, 256, 1024, 0xdd1444a4))]
    for make, args, want in rows:
        v = make(gpu, *args)
        assert (v.q.ptr - v.ptr, v.q.nstride, v.q.pstride, v.total_units, int(v.inside.sum()), crc(v.inside)) == want, (make.__name__, args)
        assert v.q.shape == args[0] and v.span == 16 * v.total_units == gpu[0]._allocs[v.base] and v.inside.size == 8 * v.total_units
        assert v.stray().size == 0 and len(v.pieces()) == v.planes


def test_byte_buffer_layouts(gpu, mem):
    raw, buf = canary.Bytes.rounded(gpu, 100), canary.Bytes(gpu, 101)
    assert (raw.ptr - raw.base, raw.nbytes, raw.total, int(raw.inside.sum()), crc(raw.inside)) == (4096, 112, 8304, 56, 0x4dfbcb32)
    assert (buf.ptr - buf.base, buf.nbytes, buf.total, int(buf.inside.sum()), crc(buf.inside)) == (4096, 101, 8294, 51, 0xccd0d415)
    assert raw.t.shape == (1, 28, 1, 1) and raw.numpy().shape == (28,) and buf.bytes().shape == (101,)
    assert raw.untouched() and buf.untouched() and raw.stray().size == 0 and buf.stray().size == 0


# ---- stray writes ----
def test_a_halfword_outside_an_fp32_view_is_reported_with_its_position(gpu, mem):
    dev = gpu[0]
    for make, args in ((canary.View.free, ((3, 5, 7, 9), (3, 5))), (canary.View.named, ((2, 8, 4, 4), 'slice')),
                       (canary.View.framed, ((2, 6, 16, 12), 'slice'))):
        v = make(gpu, *args)
        first, chw = (v.t.ptr - v.base) // 2, 2 * int(np.prod(v.t.shape[1:]))
        spots = {"before": first - 1, "in the gap between two samples": first + chw, "after": first + 2 * (v.t.shape[0] - 1) * v.t.nstride + chw}
        for name, h in spots.items():
            assert not v.inside[h], name
            dev.poke(v.base + 2 * h)
            assert list(v.stray()) == [h], name
            with pytest.raises(AssertionError, match="first at halfword %d " % h):
                canary.clean(name, v)
            dev.poke(v.base + 2 * h, CANARY)
            canary.clean(name, v)
        for h in (first, first + chw - 1, spots["after"] - 1):                  # inside: not reported
            assert v.inside[h]
            dev.poke(v.base + 2 * h)
        v.t.set(np.ones(v.t.shape))
        canary.clean("written inside", v)


def test_a_write_into_another_piece_plane_outside_a_q_slice_is_reported(gpu, mem):
    dev = gpu[0]
    v = canary.QView.named(gpu, (2, 16, 4, 4), 'bf16x3', 'slice')
    first, units = (v.q.ptr - v.base) // 16, 2 * 16                             # the slice: two channel blocks of 16 pixels
    inside = [first + p * v.q.pstride + n * v.q.nstride + u for p in range(3) for n in range(2) for u in (0, units - 1)]
    outside = [first + v.q.pstride - 1, first + v.q.pstride + units, first + 2 * v.q.pstride + v.q.nstride - 16, first - 1]
    assert all(v.inside[8 * u] for u in inside) and not any(v.inside[8 * u] for u in outside)
    for u in inside:
        dev.poke(v.base + 16 * u)
    canary.clean("inside the slice", v)
    for u in outside:
        dev.poke(v.base + 16 * u + 6)
        assert list(v.stray()) == [8 * u + 3]
        with pytest.raises(AssertionError, match="first at halfword %d " % (8 * u + 3)):
            canary.clean("another plane", v)
        dev.poke(v.base + 16 * u + 6, CANARY)


def test_a_byte_behind_a_buffer_of_odd_size_is_reported(gpu, mem):
    dev = gpu[0]
    b = canary.Bytes(gpu, 101, np.arange(101, dtype=np.uint8))
    canary.unchanged("fresh", b)
    for at in (canary.GUARD - 1, canary.GUARD + 101, b.total - 1):
        old = dev.mem[b.base + at]
        dev.mem[b.base + at] = 0
        assert list(b.stray()) == [at]
        with pytest.raises(AssertionError, match="first at byte %d " % at):
            canary.clean("odd", b)
        dev.mem[b.base + at] = old
    dev.mem[b.ptr + 100] ^= 1
    canary.clean("inside", b)
    with pytest.raises(AssertionError, match="input 0 was modified"):
        canary.unchanged("inside", b)


def test_unchanged_fails_when_one_bit_of_an_input_flips(gpu, mem):
    dev = gpu[0]
    data = np.random.RandomState(0).randn(2, 8, 4, 4).astype(np.float32)
    v, r = canary.View.named(gpu, data.shape, 'offset', data), canary.Bytes.rounded(gpu, 4 * 28, np.arange(28))
    q = canary.QView.named(gpu, data.shape, 'bf16', 'slice')
    q.snapshot()
    canary.unchanged("fresh", v, r, q)
    for buf, at in ((v, v.t.ptr + 4 * v.t.nstride + 7), (r, r.ptr + 111), (q, q.q.ptr + 16 * q.q.nstride)):
        dev.mem[at] ^= 0x10
        with pytest.raises(AssertionError, match="input 0 was modified"):
            canary.unchanged("flipped", buf)
        canary.clean("flipped", buf)
        dev.mem[at] ^= 0x10
        canary.unchanged("restored", buf)
    assert v.same() and np.array_equal(r.numpy(), np.arange(28, dtype=np.float32))


def test_repaint_leaves_the_views_and_replaces_the_canary(gpu, mem):
    dev = gpu[0]
    data = np.random.RandomState(1).randn(2, 8, 4, 4).astype(np.float32)
    v, b, q = canary.View.named(gpu, data.shape, 'slice', data), canary.Bytes(gpu, 6, b"abcdef"), canary.QView.named(gpu, data.shape, 'bf16x2', 'offset')
    q.snapshot()
    canary.repaint(dev, v, b, q)
    assert v.same() and b.same()
    for o in (v, b, q):
        raw = np.empty(o.span // 2, np.uint16)
        dev.d2h(raw, o.base, o.span)
        assert (raw[~o.inside] == canary.PATTERN2).all() and (raw[o.inside] != canary.PATTERN2).all()


# ---- the ledger ----
def ledger(**kw):
    return canary.Ledger(lambda key, w, r, n: "measured %s %.3f %.2e %d" % (key, w, r, n), **kw)


def test_note_fails_just_above_k_and_passes_at_k(gpu, mem, capsys):
    L = ledger(bound={'op': 4}.__getitem__, describe=lambda at, i, shape: "class of %s %s" % (at, i))
    ref = np.array([[1.0, 2.0], [4.0, 8.0]])
    at_k = ref.astype(np.float32)
    at_k[1, 0] += np.float32(4 * U * 4.0)                                       # 4 units of 2^-24 M at M = |ref|: two ulps
    L.note('op', at_k, ref, np.abs(ref), "at k")
    assert L.measured['op'][0] == 4.0 and "op at k: worst k 4.000 (bound 4)" in capsys.readouterr().out
    above = at_k.copy()
    above[1, 0] = np.nextafter(above[1, 0], np.float32(9))
    with pytest.raises(pytest.fail.Exception, match=r"element \(1, 0\) \(class of geometry \(1, 0\)\) got .* > k = 4"):
        L.note('op', above, ref, np.abs(ref), "above k", at="geometry")
    assert L.measured['op'] == (6.0, canary.rel(above, ref))                    # (the figures are kept before they are asserted)
    above[1, 0] = np.nextafter(above[1, 0], np.float32(9))
    L.note('op', above, ref, np.abs(ref), "a wider bound for the call", k=8, record=False)
    assert L.count == {'op': 3} and L.measured['op'][0] == 6.0


def test_note_fails_on_a_non_finite_output_and_on_the_second_figure(gpu, mem):
    L = ledger(rel_limit=1e-5, maxabs=lambda key: key == 'abs')
    ref = np.ones(4)
    for bad in (np.nan, np.inf):
        got = ref.astype(np.float32)
        got[2] = bad
        with pytest.raises(AssertionError, match="not finite everywhere: 1 elements"):
            L.note('op', got, ref, np.full(4, np.inf), "non-finite", k=1)
    got = ref.astype(np.float32) * np.float32(1 + 2e-5)
    with pytest.raises(AssertionError, match="rel-L2"):
        L.note('op', got, ref, ref, "rel-L2 over its limit", k=1000)
    with pytest.raises(AssertionError, match="max-abs/scale"):
        L.note('abs', got, ref, ref, "max-abs over its limit", k=1000)
    L.note('op', got, ref, ref, "a limit for the call", k=1000, rel_limit=1e-4)
    L.note('op', got, ref, ref, "kept, not limited", k=1000, rel_limit=None)
    before = L.measured['op']
    L.note('op', got * 2, ref, ref, "left out", k=2 ** 25, rel_limit=False)
    assert L.measured['op'][1] == before[1] and L.measured['op'][0] > before[0]
    with pytest.raises(AssertionError):
        L.note('op', np.ones((2, 2), np.float32), ref, ref, "another shape", k=1)


def test_note_keeps_the_maximum_of_two_calls_and_their_count(gpu, mem, capsys):
    L = ledger(order=lambda m: sorted(m, key=str), header="before", footer=lambda: "after")
    ref = np.ones(8)
    small, large = ref.astype(np.float32), ref.astype(np.float32)
    small[0] += np.float32(2 * U)
    large[5] += np.float32(6 * U)
    L.note('op', large, ref, ref, "large", k=6)
    L.note('op', small, ref, ref, "small", k=6)
    L.note(('two', 'words'), small, ref, ref, "small", k=2)
    assert L.measured['op'] == (6.0, canary.rel(large, ref)) and L.count == {'op': 2, ('two', 'words'): 1}
    L.tally('op', 2)
    L.record('other', 1.5, 0.25)
    capsys.readouterr()
    L.table()
    assert capsys.readouterr().out.splitlines() == ["before", "measured ('two', 'words') 2.000 %.2e 1" % canary.rel(small, ref),
                                                    "measured op 6.000 %.2e 4" % canary.rel(large, ref), "measured other 1.500 2.50e-01 1", "after"]


def test_exact_tells_the_zeros_apart_unless_told_not_to_and_counts(gpu, mem):
    L = ledger(describe=lambda at, i, shape: "column %d of %s" % (i[-1], at))
    want = np.array([[0.0, 1.0, -0.0]], np.float32)
    L.exact('op', want.copy(), want, "the same bits")
    got = np.array([[-0.0, 1.0, -0.0]], np.float32)
    with pytest.raises(pytest.fail.Exception, match=r"1 of 3 elements differ in bits, first at \(0, 0\) \(column 0 of relu\): got \S*-0\.0\S*, expected \S*0\.0"):
        L.exact('op', got, want, "signed zero", at="relu")
    L.exact('op', got, want, "either zero", zero_sign=False)
    with pytest.raises(pytest.fail.Exception, match="1 of 3 elements differ"):
        L.exact('op', np.array([[0.0, np.nextafter(np.float32(1), np.float32(2)), -0.0]], np.float32), want, "one ulp", zero_sign=False)
    with pytest.raises(AssertionError):
        L.exact('op', want[0], want, "another shape")
    assert L.count == {'op': 5} and L.measured == {'op': (0.0, 0.0)}


def test_the_factory_made_one_device_and_mem_freed_what_the_tests_allocated(gpu):
    dev = gpu[0]
    assert DEVICES == [dev] and gpu[1] is None and gpu[2] is D and not dev._allocs and dev._next > 4096
    CACHE['kept until the module ends'] = 1
    LEDGER.record('the table is printed when the module ends', 1.0, 0.5)


def test_cached_computes_once_and_keeps_the_newest(gpu, mem):
    cache, calls = {}, []
    for key in (1, 2, 1, 3, 1):
        assert canary.cached(cache, key, lambda: calls.append(key) or key * 10, keep=2) == key * 10
    assert calls == [1, 2, 3, 1] and list(cache) == [3, 1]
    assert canary.cached(cache, 4, lambda: 40) == 40 and list(cache) == [3, 1, 4]
    assert np.array_equal(canary.fl32_sum(np.float32(1), 2.0 ** -25), np.float32(1))
