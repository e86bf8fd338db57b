"""The helpers the terrain tools share (gan_heightmaps_amd/planes.py): the one heightmap intake, as each of the five tools
calls it, over a table of inputs, and the call-scoped device scratch on a device whose allocations fail.  No device.

The expected outcomes are literals.  They were recorded once by running the five ``_as_plane`` functions the tools had
before the intake was shared over this table; they say what each tool took, returned and refused, message by message."""
import numpy as np
import pytest

from gan_heightmaps_amd import erosion, hydrology, mesh, route, skylight
from gan_heightmaps_amd.planes import as_plane, check_size, scratch

TOOLS = [("erosion", erosion._plane), ("skylight", skylight._plane), ("mesh", mesh._plane),
         ("hydrology", hydrology._as_plane), ("route", route._as_plane)]


def strided(shape):
    """a plane of zeros of any size that is one float in memory"""
    return np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), shape=shape, strides=(0, 0), writeable=False)


def inputs():
    f64 = np.array([[0.0, 0.25, 0.5], [0.75, 1.0, 0.125]], np.float64)

    def with_value(v):
        x = f64.astype(np.float32)
        x[1, 1] = v
        return x
    return [("uint8", np.arange(0, 60, 10, dtype=np.uint8).reshape(2, 3)),
            ("float64", f64),
            ("list", f64.tolist()),
            ("(1, H, W)", f64[None]),
            ("uint8 (1, H, W)", np.arange(0, 60, 10, dtype=np.uint8).reshape(1, 2, 3)),
            ("(2, H, W)", np.zeros((2, 2, 3), np.float32)),
            ("1-D", np.zeros(3, np.float32)),
            ("4-D", np.zeros((1, 1, 2, 3), np.float32)),
            ("(0, W)", np.zeros((0, 3), np.float32)),
            ("(H, 0)", np.zeros((2, 0), np.uint8)),
            ("(1, 0, W)", np.zeros((1, 0, 3), np.float32)),
            ("int32", np.zeros((2, 3), np.int32)),
            ("nan", with_value(np.nan)),
            ("+inf", with_value(np.inf)),
            ("-inf", with_value(-np.inf)),
            ("1.5", with_value(1.5)),
            ("1.5 and nan", np.array([[1.5, np.nan]], np.float32)),
            ("-0.0", with_value(-0.0)),
            ("tall", strided((4 * 65535 + 1, 2))),
            ("huge", strided((1 << 16, 1 << 15)))]


def outcome(intake, x):
    """'dtype shape bits' (little-endian hex; a larger plane of +0 as its byte count), erosion's with its answer about the
    leading axis, or the refusal"""
    try:
        r = intake(x)
    except ValueError as e:
        return "ValueError: %s" % e
    a, lead = r if isinstance(r, tuple) else (r, None)
    assert a.flags['C_CONTIGUOUS']
    bits = a.tobytes().hex() if a.size <= 16 else "%d x 00" % a.nbytes if not a.any() and not np.signbit(a).any() else "?"
    return "%s %s %s%s" % (a.dtype, a.shape, bits, "" if lead is None else " lead=%s" % lead)


U8 = 'float32 (2, 3) 00000000a1a0203da1a0a03df1f0f03da1a0203ec9c8483e'
F64 = 'float32 (2, 3) 000000000000803e0000003f0000403f0000803f0000003e'
ONE_FIVE = 'float32 (2, 3) 000000000000803e0000003f0000403f0000c03f0000003e'
MINUS_ZERO = 'float32 (2, 3) 000000000000803e0000003f0000403f000000800000003e'
PLUS_ZERO = 'float32 (2, 3) 000000000000803e0000003f0000403f000000000000003e'
TALL = 'float32 (262141, 2) 2097128 x 00'
SHAPE = 'ValueError: heightmap must be (H, W) or (1, H, W), got %s'
SHAPE_2D = 'ValueError: heightmap must be (H, W), got %s'
SIZE = 'ValueError: heightmap size %d x %d out of range (H W < 2^31, H <= 262140)'
DTYPE = 'ValueError: heightmap must be uint8 or floating point in [0, 1], got int32'
NON_FINITE = 'ValueError: the heightmap has non-finite values'
UNIT = 'ValueError: a floating-point heightmap must lie in [0, 1]'
# erosion, skylight and mesh read all 2^31 elements, 8 GiB, before their tools check the size: not run
READS_ALL = None

# input -> the outcomes for erosion, skylight, mesh, hydrology, route
EXPECTED = {
    'uint8': [U8 + ' lead=False', U8, U8, U8, U8],
    'float64': [F64 + ' lead=False', F64, F64, F64, F64],
    'list': [F64 + ' lead=False', F64, F64, F64, F64],
    '(1, H, W)': [F64 + ' lead=True', SHAPE_2D % '(1, 2, 3)', F64, F64, F64],
    'uint8 (1, H, W)': [U8 + ' lead=True', SHAPE_2D % '(1, 2, 3)', U8, U8, U8],
    '(2, H, W)': ['ValueError: erosion needs one height per pixel: a (H, W) or (1, H, W) heightmap, got (2, 2, 3)',
                  SHAPE_2D % '(2, 2, 3)', SHAPE % '(2, 2, 3)', SHAPE % '(2, 2, 3)', SHAPE % '(2, 2, 3)'],
    '1-D': [SHAPE % '(3,)', SHAPE_2D % '(3,)', SHAPE % '(3,)', SHAPE % '(3,)', SHAPE % '(3,)'],
    '4-D': [SHAPE % '(1, 1, 2, 3)', SHAPE_2D % '(1, 1, 2, 3)', SHAPE % '(1, 1, 2, 3)', SHAPE % '(1, 1, 2, 3)',
            SHAPE % '(1, 1, 2, 3)'],
    '(0, W)': [SHAPE % '(0, 3)', SHAPE_2D % '(0, 3)', SHAPE % '(0, 3)', SIZE % (0, 3), SIZE % (0, 3)],
    '(H, 0)': [SHAPE % '(2, 0)', SHAPE_2D % '(2, 0)', SHAPE % '(2, 0)', SIZE % (2, 0), SIZE % (2, 0)],
    '(1, 0, W)': [SHAPE % '(1, 0, 3)', SHAPE_2D % '(1, 0, 3)', SHAPE % '(1, 0, 3)', SIZE % (0, 3), SIZE % (0, 3)],
    'int32': [DTYPE, DTYPE, DTYPE, 'ValueError: heightmap must be uint8 or floating point, got int32',
              'ValueError: heightmap must be uint8 or floating point, got int32'],
    'nan': [NON_FINITE] * 5,
    '+inf': [NON_FINITE, NON_FINITE, UNIT, NON_FINITE, NON_FINITE],
    '-inf': [NON_FINITE, NON_FINITE, UNIT, NON_FINITE, NON_FINITE],
    '1.5': [ONE_FIVE + ' lead=False', ONE_FIVE, UNIT, ONE_FIVE, ONE_FIVE],
    '1.5 and nan': [NON_FINITE] * 5,
    '-0.0': [MINUS_ZERO + ' lead=False', MINUS_ZERO, MINUS_ZERO, PLUS_ZERO, PLUS_ZERO],
    'tall': [TALL + ' lead=False', TALL, TALL, SIZE % (262141, 2), SIZE % (262141, 2)],
    'huge': [READS_ALL, READS_ALL, READS_ALL, SIZE % (65536, 32768), SIZE % (65536, 32768)],
}


def test_every_tool_takes_returns_and_refuses_what_it_did():
    table = inputs()
    assert [name for name, _ in table] == list(EXPECTED)
    for name, x in table:
        for (tool, intake), want in zip(TOOLS, EXPECTED[name]):
            if want is not READS_ALL:
                assert outcome(intake, x) == want, (name, tool)


def test_the_size_limit_and_its_three_messages():
    for H, W in ((1, 1), (4 * 65535, 2), (1 << 15, (1 << 16) - 1)):
        check_size(H, W)
    for H, W in ((0, 1), (1, 0), (4 * 65535 + 1, 1), (1 << 15, 1 << 16)):
        with pytest.raises(ValueError, match=r"^heightmap size %d x %d out of range$" % (H, W)):
            check_size(H, W)
        with pytest.raises(ValueError, match=r"^heightmap size %d x %d out of range \(H W < 2\^31, H <= 262140\)$" % (H, W)):
            check_size(H, W, limits=True)
    # skylight's: the plane with its margin is counted and named, the rows of the launch are the interior's
    check_size(4 * 65535, 2, plane=(4 * 65535 + 6, 8))
    with pytest.raises(ValueError, match=r"^heightmap size 262147 x 8 out of range$"):
        check_size(4 * 65535 + 1, 2, plane=(4 * 65535 + 7, 8))
    with pytest.raises(ValueError, match=r"^heightmap size 65536 x 32768 out of range$"):
        check_size((1 << 16) - 6, (1 << 15) - 6, plane=(1 << 16, 1 << 15))
    # the options are keywords: a second positional argument is a mistake, not a lead
    with pytest.raises(TypeError):
        as_plane(np.zeros((2, 3), np.float32), False)


# ---- scratch ------------------------------------------------------------------------------------------------------------
class FailingDevice:
    """alloc, free and sync, logged; the ``fail``-th alloc (from 1) raises MemoryError"""

    def __init__(self, fail=None):
        self.fail, self.log, self.n = fail, [], 0

    def alloc(self, nbytes):
        self.n += 1
        if self.n == self.fail:
            raise MemoryError("alloc %d" % self.n)
        self.log.append(("alloc", self.n, nbytes))
        return 1000 * self.n

    def free(self, p):
        self.log.append(("free", p))

    def sync(self):
        self.log.append(("sync",))


def test_scratch_frees_what_it_handed_out_once_the_device_is_idle():
    dev = FailingDevice()
    with scratch(dev) as alloc:
        assert [alloc(8), alloc(16), alloc(0)] == [1000, 2000, 3000]
        assert dev.log == [("alloc", 1, 8), ("alloc", 2, 16), ("alloc", 3, 0)]          # one at a time, nothing else yet
    assert dev.log[3:] == [("sync",), ("free", 1000), ("free", 2000), ("free", 3000)]
    dev = FailingDevice()
    with scratch(dev):
        pass
    assert dev.log == [("sync",)]


@pytest.mark.parametrize("k", [1, 2, 4])
def test_scratch_frees_the_first_allocations_when_the_kth_fails(k):
    dev = FailingDevice(fail=k)
    got = []
    with pytest.raises(MemoryError, match="alloc %d" % k):
        with scratch(dev) as alloc:
            for n in (8, 16, 24, 32):
                got.append(alloc(n))
    assert got == [1000 * i for i in range(1, k)]
    assert dev.log == [("alloc", i, 8 * i) for i in range(1, k)] + [("sync",)] + [("free", p) for p in got]


def test_scratch_frees_when_the_body_fails_and_without_a_sync_when_told():
    dev = FailingDevice()
    with pytest.raises(KeyError):
        with scratch(dev) as alloc:
            alloc(8), alloc(16)
            raise KeyError("the body")
    assert dev.log[2:] == [("sync",), ("free", 1000), ("free", 2000)]
    for fail in (None, 3):
        dev = FailingDevice(fail)
        try:
            with scratch(dev, sync=False) as alloc:
                alloc(8), alloc(16), alloc(24)
        except MemoryError:
            pass
        assert [e for e in dev.log if e[0] != "alloc"] == [("free", 1000), ("free", 2000)] + [("free", 3000)] * (fail is None)


def test_scratch_keeps_what_the_caller_takes_over():
    dev = FailingDevice()
    with scratch(dev) as alloc:
        a, b, c = alloc(8), alloc(16), alloc(24)
        alloc.keep(a, c)
    assert dev.log[3:] == [("sync",), ("free", b)]
    with pytest.raises(ValueError):
        with scratch(dev) as alloc:
            alloc.keep(12345)                                             # not handed out by this scratch
