"""Definitions of the weight operands every convolution of the hot path reads instead of the fp32 master weights -- the fp32
transposed copy (csrc/conv_igemm.hip: ghm_conv2d_transpose_weights / ghm_transpose_weights_batched), the bf16 / fp16 packs
(csrc/conv_lp.hip: ghm_lp_pack_weights / ghm_lp_pack_batched), the split packs of two or three planes (csrc/conv_split.hip:
ghm_split_pack_weights / ghm_split_pack_batched), the collapsed up-sample weights and the expansion of their gradient
(csrc/elementwise.hip: ghm_upconv_collapse_weights / _batched, ghm_upconv_expand_wgrad / _batched) -- the launcher and table
arithmetic restated in Python, and the row tables and input sets of tests/test_gpu_weight_operands.py (shared with
tests/test_weight_operand_ref.py, which validates the definitions, the tables, the inputs and the bounds on the CPU).
numpy only; built on oracle/lp.py for the roundings and on the two predecessors for the helpers (tests/elementwise_q_ref.py:
pieces, the canary helpers, worst, rel, bits_equal; tests/bn_f32_ref.py: BF16_BITS, rne_bf16_bits).

Every definition takes the packed fp32 wp[C][T][K] (device.pack_conv_w: wp[c][a kw + b][k] = the CORRELATION tap (a, b) of
filter k on channel c).  The kernels only move, round and add a few values:
  transposes and packs   bit for bit;
  collapse and expand    a ``restate32_*`` form -- the kernel's sums in float32, in the kernel's order -- bit for bit, and the
                         float64 definition within |got - ref| <= k 2^-24 M per element, k = the number of additions of that
                         element (terms - 1, + 1 when the previous value is added), M = the sum of |term| (+ |previous|).  The
                         mode-1 coefficients are 1, 1/2 and 1/4: a product by them is exact (no input is small enough to leave
                         the normal range), so a multiply-add contracted by the compiler rounds like the separate operations.
"""
import numpy as np

from oracle import lp as LP
from tests.bn_f32_ref import BF16_BITS, rne_bf16_bits  # noqa: F401
from tests.elementwise_q_ref import (U, REL_L2, PLANES, CANARY, canary_fill, canary_changed, f32_inside, worst, rel, bits_equal,  # noqa: F401
                                     pieces)

LP_DTYPES = ('bf16', 'f16')
SPLIT_DTYPES = ('bf16x3', 'bf16x2')
UNIT = 8                            # halfwords of a 16-byte unit: 8 consecutive reduction channels
BLOCK = 256                         # threads of a block of every kernel here: units (packs) or elements (collapse, expand)


def ceil_div(a, b):
    return -(-a // b)


# ---- the fp32 transposed copy ----
def transpose(wp):
    """wp[C][T][K] -> wpT[K][T][C], wpT[k][T - 1 - tap][c] = wp[c][tap][k]: the packed weights of the adjoint convolution"""
    return np.ascontiguousarray(np.asarray(wp)[:, ::-1, :].transpose(2, 1, 0))


# ---- bf16 / fp16 / split packs ----
def lp_geometry(red, rows):
    """-> (nblk, rpad): channel blocks of 8 (whole slabs of 16), rows padded to 128"""
    return ceil_div(red, 16) * 2, ceil_div(rows, 128) * 128


def plane_units(red, T, rows):
    nblk, rpad = lp_geometry(red, rows)
    return nblk * T * rpad


def operand(wp, red, T, rows, transposed):
    """the fp32 values of a pack, A[c][tap][r] over the reduction channel c < red and the row r < rows: wp itself (red = C, rows
    = K), or for the data-gradient operand the transposed copy (red = K, rows = C, taps flipped)"""
    wp = np.asarray(wp, np.float32)
    A = transpose(wp) if transposed else wp
    assert A.shape == (red, T, rows), (A.shape, (red, T, rows))
    return A


def halfwords(v, dtype):
    """the 16 bits stored for float32 values that ARE bf16 / fp16 numbers"""
    v = np.ascontiguousarray(v, np.float32)
    if dtype == 'f16':
        return v.astype(np.float16).view(np.uint16)
    return (v.view(np.uint32) >> 16).astype(np.uint16)


def lp_pack(wp, red, T, rows, transposed, dtype):
    """-> the uint16 halfwords of the whole pack: PLANES[dtype] planes, one after the other, of wq[c / 8][tap][rpad][8], +0
    wherever c >= red or r >= rows; rounding by oracle.lp (``pieces``)"""
    nblk, rpad = lp_geometry(red, rows)
    full = np.zeros((nblk * UNIT, T, rpad), np.float32)
    full[:red, :, :rows] = operand(wp, red, T, rows, transposed)
    with np.errstate(over='ignore'):
        planes = pieces(full, dtype)
    kind = 'f16' if dtype == 'f16' else 'bf16'
    out = [halfwords(p, kind).reshape(nblk, UNIT, T, rpad).transpose(0, 2, 3, 1) for p in planes]
    return np.ascontiguousarray(np.stack(out)).reshape(-1)


def lp_unpack(h, red, T, rows, dtype):
    """the inverse view: halfwords -> float32 values [planes][nblk 8][T][rpad] (padding included)"""
    nblk, rpad = lp_geometry(red, rows)
    h = np.asarray(h, np.uint16).reshape(PLANES[dtype], nblk, T, rpad, UNIT).transpose(0, 1, 4, 2, 3)
    h = np.ascontiguousarray(h).reshape(PLANES[dtype], nblk * UNIT, T, rpad)
    if dtype == 'f16':
        return h.view(np.float16).astype(np.float32)
    return (h.astype(np.uint32) << 16).view(np.float32)


# ---- collapse / expand: the tap maps of csrc/elementwise.hip ----
def upconv_group(p, a):
    """low-resolution offset + 1 of the 5x5 correlation tap a for output parity p: tap a (offset a - 2) of output row 2 i + p
    reads low-res row i + floor((p + a - 2) / 2):   p = 0: {0, 1} -> 0, {2, 3} -> 1, {4} -> 2;   p = 1: {0} -> 0, {1, 2} -> 1,
    {3, 4} -> 2"""
    return (p + a - 2) // 2 + 1


def blconv_coef(p, r, a):
    """coefficient of the fine 3x3 correlation tap a (offset a - 1) in the coarse tap r (offset r - 1) for output parity p, on
    the zero-extended coarse grid:
      p = 0 (u[2m-1], u[2m], u[2m+1] = (x[m-1] + x[m]) / 2, x[m], (x[m] + x[m+1]) / 2):  r = 0: (1/2, 0, 0)  1: (1/2, 1, 1/2)  2: (0, 0, 1/2)
      p = 1 (u[2m], u[2m+1], u[2m+2] = x[m], (x[m] + x[m+1]) / 2, x[m+1]):              r = 0: none         1: (1, 1/2, 0)    2: (0, 1/2, 1)"""
    return (((.5, 0, 0), (.5, 1, .5), (0, 0, .5)), ((0, 0, 0), (1, .5, 0), (0, .5, 1)))[p][r][a]


TAPS = {0: 5, 1: 3}                 # filter size per mode: 0 = Upscale2D (nearest) -> 5x5, 1 = BilinearUpsample2D -> 3x3


def tap_coef(mode):
    """[p][r][a]: the weight of fine tap a in coarse tap r for parity p, per axis"""
    n = TAPS[mode]
    f = (lambda p, r, a: float(upconv_group(p, a) == r)) if mode == 0 else blconv_coef
    return np.array([[[f(p, r, a) for a in range(n)] for r in range(3)] for p in range(2)], np.float64)


def coef(mode):
    """[rs][pq][ab]: the coefficient of fine tap ab = a n + b in collapsed tap rs = 3 r + s of parity class pq = 2 p + q"""
    c, n = tap_coef(mode), TAPS[mode]
    return np.einsum('pra,qsb->rspqab', c, c).reshape(9, 4, n * n)


def collapse_terms(mode):
    """[rs][pq]: the number of fine taps that land in a collapsed tap"""
    return (coef(mode) != 0).sum(-1)


def expand_terms(mode):
    """[ab]: the number of collapsed taps a fine tap lands in"""
    return (coef(mode) != 0).sum((0, 1))


def collapse(wp, mode):
    """wp[C][n n][K] -> wpc[c][rs][pq][k] in float64: a packed 3x3 convolution with 4 K filters ordered (parity class, k)"""
    return np.einsum('rpt,ctk->crpk', coef(mode), np.asarray(wp, np.float64))


def expand(dwpc, mode):
    """the transposed tap map: dwpc[C][9][4][K] -> dwp[c][ab][k] in float64"""
    return np.einsum('rpt,crpk->ctk', coef(mode), np.asarray(dwpc, np.float64))


def collapse_M(wp, mode):
    return collapse(np.abs(np.asarray(wp, np.float64)), mode)


def expand_M(dwpc, mode, prev=None):
    M = expand(np.abs(np.asarray(dwpc, np.float64)), mode)
    return M if prev is None else M + np.abs(np.asarray(prev, np.float64))


def collapse_k(mode, C, K):
    """additions per element of wpc[C][9][4][K]: terms - 1 (the first term is added to +0, exactly)"""
    return np.broadcast_to(np.maximum(collapse_terms(mode) - 1, 0)[None, :, :, None], (C, 9, 4, K))


def expand_k(mode, C, K, accumulate):
    k = np.maximum(expand_terms(mode) - 1, 0) + (1 if accumulate else 0)
    return np.broadcast_to(k[None, :, None], (C, TAPS[mode] ** 2, K))


def restate32_collapse(wp, mode):
    """upconv_collapse(_batched)_kernel in float32: v = +0, then the terms in the kernel's order (a outer, b inner)"""
    wp = np.asarray(wp, np.float32)
    C, T, K = wp.shape
    cf = coef(mode).astype(np.float32)
    out = np.empty((C, 9, 4, K), np.float32)
    for rs in range(9):
        for pq in range(4):
            v = np.zeros((C, K), np.float32)
            for ab in range(T):
                if cf[rs, pq, ab] != 0:
                    v = v + cf[rs, pq, ab] * wp[:, ab, :]
            out[:, rs, pq, :] = v
    return out


def restate32_expand(dwpc, mode, prev=None):
    """upconv_expand(_batched)_kernel in float32: v = +0, then the terms with pq outer and rs inner; the previous value is added
    last when accumulating"""
    dwpc = np.asarray(dwpc, np.float32)
    C, _, _, K = dwpc.shape
    cf = coef(mode).astype(np.float32)
    T = TAPS[mode] ** 2
    out = np.empty((C, T, K), np.float32)
    for ab in range(T):
        v = np.zeros((C, K), np.float32)
        for pq in range(4):
            for rs in range(9):
                if cf[rs, pq, ab] != 0:
                    v = v + cf[rs, pq, ab] * dwpc[:, rs, pq, :]
        out[:, ab, :] = v
    if prev is not None:
        out = np.asarray(prev, np.float32).reshape(out.shape) + out
    assert out.dtype == np.float32
    return out


def bias4(bias):
    return np.tile(np.asarray(bias, np.float32), 4)


# ---- launcher and table arithmetic restated (device.Ops.*_table, the ghm_*_weight_bytes entry points) ----
def pack_blocks(red, T, rows):
    return ceil_div(plane_units(red, T, rows), BLOCK)


def transpose_blocks(C, T, K):
    return T * ceil_div(C, 32) * ceil_div(K, 32)


def collapse_blocks(C, K):
    return ceil_div(36 * C * K + 4 * K, BLOCK)


def expand_blocks(C, K, mode=0):
    """ceil(25 C K / 256) in BOTH modes: a mode-1 item (9 C K elements) ends with blocks that write nothing"""
    return ceil_div(25 * C * K, BLOCK)


def lp_weight_bytes(red, T, rows):
    return plane_units(red, T, rows) * 16


def split_weight_bytes(red, T, rows, planes):
    return planes * lp_weight_bytes(red, T, rows)


def weight_bytes(red, T, rows, dtype):
    return PLANES[dtype] * lp_weight_bytes(red, T, rows)


def begins(blocks):
    """-> (block_begin of every item: the running sum, the total)"""
    b = np.concatenate([[0], np.cumsum(blocks)]).astype(np.int64)
    return b[:-1], int(b[-1])


# record layouts of include/ghm.h: (name, numpy type, byte offset), the record's size
LP_RECORD = ([('wp', '<u8', 0), ('wq', '<u8', 8), ('red', '<i4', 16), ('T', '<i4', 20), ('rows', '<i4', 24), ('nblk', '<i4', 28),
              ('rpad', '<i4', 32), ('transposed', '<i4', 36), ('block_begin', '<i4', 40), ('zero', '<i4', 44)], 48)
TRANSPOSE_RECORD = ([('wp', '<u8', 0), ('wpT', '<u8', 8), ('C', '<i4', 16), ('T', '<i4', 20), ('K', '<i4', 24),
                     ('block_begin', '<i4', 28)], 32)
COLLAPSE_RECORD = ([('wp5', '<u8', 0), ('bias', '<u8', 8), ('wpc', '<u8', 16), ('bias4', '<u8', 24), ('C', '<i4', 32), ('K', '<i4', 36),
                    ('block_begin', '<i4', 40), ('mode', '<i4', 44)], 48)
EXPAND_RECORD = ([('dwpc', '<u8', 0), ('dwp5', '<u8', 8), ('C', '<i4', 16), ('K', '<i4', 20), ('block_begin', '<i4', 24),
                  ('mode', '<i4', 28)], 32)


def decode(raw, record):
    """bytes of a device table -> a numpy record array, the fields at the offsets include/ghm.h states"""
    fields, size = record
    dt = np.dtype(dict(names=[f[0] for f in fields], formats=[f[1] for f in fields], offsets=[f[2] for f in fields], itemsize=size))
    raw = np.ascontiguousarray(raw, np.uint8)
    assert raw.size % size == 0, (raw.size, size)
    return raw.view(dt)


# ---- row tables: each row says which branch or edge it reaches; tests/test_weight_operand_ref.py asserts every claim ----
# packs: (red, T, rows, transposed) -- red / rows = (C, K) of the convolution for a forward pack, (K, C) for a transposed one.
# nblk is even and rpad a multiple of 128, so the units of a plane are a multiple of 256 in EVERY row (remainder 0, asserted): an
# item always ends on a block boundary, no block of a table is partly idle, and a wrong table scan cannot hide in an idle tail --
# it shows as the first block of item i + 1 handled with item i's record (its geometry, its pointers).  So neighbours in
# PACK_TABLE_ORDER differ in T, in rpad and in transposed, forwards and backwards; the last three rows exist for that.
PACK_ROWS = [
    ((16, 9, 128, 0), "nothing ragged: one slab, one row block, no zero halfword"),
    ((5, 9, 7, 0), "red < 8: the second channel block is all zeros, three zero channels in the first; 121 zero rows"),
    ((24, 25, 200, 0), "the last channel block of the second slab is zero; rpad = 256; 100 blocks, the largest item"),
    ((40, 9, 48, 1), "transposed, ragged on both sides: 40 = 2 slabs + 8, the last block zero; 80 zero rows"),
    ((17, 1, 129, 1), "transposed, T = 1 (the flip is the identity); one channel past a slab; one row past 128"),
    ((8, 4, 3, 0), "T = 4, the 2x2 kernels; red = 8: the second block all zeros; three rows"),
    ((1000, 1, 96, 0), "the dense layer as a 1x1 convolution; red % 16 = 8: the last block zero; 63 blocks"),
    ((32, 1, 600, 1), "transposed, T = 1, rpad = 640: five row blocks, 40 zero rows"),
    ((12, 9, 130, 1), "transposed, T = 9, rpad = 256: the taps flip; four zero channels"),
    ((3, 4, 260, 1), "transposed, T = 4 (an even tap count flips without a fixed tap), rpad = 384"),
]
PACK_TABLE_ORDER = (0, 4, 1, 7, 5, 8, 6, 9, 2, 3)


def pack_wp_shape(row):
    """(C, T, K) of the fp32 source of a pack row"""
    red, T, rows, tr = row
    return (rows, T, red) if tr else (red, T, rows)


def pack_desc_args(row):
    """(C, K, kh, kw) of the convolution whose pack the row is"""
    C, T, K = pack_wp_shape(row)
    k = {1: 1, 4: 2, 9: 3, 25: 5}[T]
    return C, K, k, k


# transposes: (C, T, K); the kernels move 32 x 32 tiles of (c, k) per tap
TRANSPOSE_ROWS = [
    ((5, 9, 7), "one tile, ragged on both sides: C < 32 and K < 32"),
    ((48, 9, 40), "2 x 2 tiles, ragged on both sides"),
    ((33, 25, 32), "ragged on the C side only (one channel past a tile), K one whole tile; T = 25"),
    ((1000, 1, 96), "T = 1: the dense layer; 32 x 3 tiles, C ragged (1000 = 31 * 32 + 8), K whole"),
    ((64, 4, 3), "K < 32: ragged on the K side only, C two whole tiles; T = 4"),
    ((32, 9, 32), "ragged on neither side: one whole tile"),
]

# collapse: (C, K, mode, bias?)
COLLAPSE_ROWS = [
    ((5, 1, 0, True), "weights and bias share one block: 180 + 4 elements"),
    ((8, 8, 0, True), "36 C K = 2304 is a whole number of blocks (9): the bias starts a block of its own"),
    ((3, 7, 1, True), "mode 1; 36 C K % 256 = 244 and 4 K = 28: the bias straddles two blocks"),
    ((16, 128, 1, True), "mode 1; 4 K = 512: the bias covers two whole blocks; 290 blocks in all, the largest row"),
    ((4, 32, 0, False), "no bias: bias4 keeps its canary; 18 blocks of weights and a nineteenth that writes nothing"),
]

# expand: (C, K, mode); each runs plain and accumulating
EXPAND_ROWS = [
    ((5, 1, 0), "one block, 125 elements"),
    ((8, 8, 1), "mode 1: 576 elements in 3 of the 7 blocks reserved: four blocks write nothing"),
    ((3, 7, 1), "mode 1: 189 elements in 1 of the 3 blocks reserved"),
    ((16, 128, 0), "25 C K = 51200: 200 whole blocks, the largest row"),
    ((4, 32, 1), "mode 1: 1152 elements in 5 of the 13 blocks reserved, the fifth half idle"),
]


# ---- input sets ----
def _rng(key, salt):
    import zlib
    return np.random.RandomState((zlib.crc32(repr(key).encode()) + salt) % (2 ** 31))


def f32_source(shape, salt=0):
    """randn / sqrt(C T), seeded per row, every 16th element an exact zero and every 41st a -0.0"""
    C, T, K = shape[0], shape[1], shape[-1]
    w = (_rng(tuple(shape), salt).randn(*shape) / np.sqrt(C * T)).astype(np.float32)
    f = w.reshape(-1)
    f[::16] = 0.0
    f[5::41] = -0.0
    return w


NONFINITE_CLASSES = ('inf', 'quiet NaN', 'NaN, payload in the low half only')


def both_signs(bits):
    out = []
    for b in bits:
        for v in (b, b ^ 0x80000000):
            if v not in out:
                out.append(v)
    return np.array(out, np.uint32)


def bf16_special_bits():
    """the finite classes of bn_f32_ref.BF16_BITS in both signs: ties on even and odd upper halves, one ulp either side, +-0,
    denormals, FLT_MAX (-> inf), ordinary values"""
    return both_signs(sum((v for k, v in BF16_BITS.items() if k not in NONFINITE_CLASSES), []))


def _f(x):
    return np.float32(x)


def f16_special_values():
    """name -> float32 value; the fp16 classes: the largest finite, the tie to inf, ties to zero and between denormals, the
    smallest normal and its neighbours, ties on even and odd mantissas"""
    up = lambda x: np.nextafter(_f(x), _f(np.inf))
    dn = lambda x: np.nextafter(_f(x), _f(0))
    return {
        '65504': _f(65504), '65520: tie to inf': _f(65520), 'below 65520': dn(65520), 'FLT_MAX': _f(3.4028234663852886e38),
        '2^-24': _f(2.0 ** -24), '2^-25: tie to 0': _f(2.0 ** -25), 'above 2^-25': up(2.0 ** -25), 'below 2^-25': dn(2.0 ** -25),
        '1.5 2^-24: tie to 2^-23': _f(1.5 * 2.0 ** -24), '2.5 2^-24: tie to 2^-23': _f(2.5 * 2.0 ** -24),
        '2^-14': _f(2.0 ** -14), 'above 2^-14': up(2.0 ** -14), 'below 2^-14': dn(2.0 ** -14),
        '2^-14 (1 - 2^-11): tie to 2^-14': _f(2.0 ** -14 * (1 - 2.0 ** -11)), '1023 2^-24: the largest denormal': _f(1023 * 2.0 ** -24),
        '1 + 2^-11: tie to 1': _f(1 + 2.0 ** -11), '1 + 3 2^-11: tie to 1 + 2^-9': _f(1 + 3 * 2.0 ** -11),
        'above 1 + 2^-11': up(1 + 2.0 ** -11), 'below 1 + 2^-11': dn(1 + 2.0 ** -11),
        '0': _f(0), 'fp32 denormal': _f(1e-42), '1': _f(1), 'pi': _f(np.pi), '1/3': _f(1 / 3), '123.456': _f(123.456),
    }


def f16_special_bits():
    return both_signs(np.array(list(f16_special_values().values()), np.float32).view(np.uint32).tolist())


SPLIT_SPECIALS = [0.0, -0.0, 1.0, -1.0, 3.0e38, -3.0e38, 1.0000001, 0.33333334]


def split_values(shape, salt=0):
    """the value set of tests/test_gpu_split.py::test_three_bf16_pieces_are_the_fp32_value: values across the fp32 exponent range
    in both signs, zeros of both signs, +-3e38, values with full mantissas in front"""
    r = _rng(tuple(shape), 50 + salt)
    x = (r.randn(*shape) * np.exp2(r.randint(-60, 60, size=shape))).astype(np.float32)
    f = x.reshape(-1)
    f[:len(SPLIT_SPECIALS)] = SPLIT_SPECIALS
    return x


def pack_inputs(row, dtype):
    """wp[C][T][K] of a pack row: the conversion classes of the dtype in front (the split dtypes: the value set of the split
    test), ordinary weights with zeros of both signs behind them"""
    shape = pack_wp_shape(row)
    if dtype in SPLIT_DTYPES:
        return split_values(shape)
    w = f32_source(shape, 1)
    special = bf16_special_bits() if dtype == 'bf16' else f16_special_bits()
    assert special.size <= w.size
    w.reshape(-1)[:special.size] = special.view(np.float32)
    return w


def collapse_inputs(row):
    C, K, mode, has_bias = row
    w = f32_source((C, TAPS[mode] ** 2, K), 2)
    return dict(wp=w, bias=_rng(row, 3).randn(K).astype(np.float32) if has_bias else None)


def expand_inputs(row):
    C, K, mode = row
    g = f32_source((C, 9, 4, K), 4)
    return dict(dwpc=g, prev=_rng(row, 5).randn(C, TAPS[mode] ** 2, K).astype(np.float32))
