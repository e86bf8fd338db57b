"""tests/weight_operand_ref.py held to account on the CPU, before tests/test_gpu_weight_operands.py holds the kernels to it: the
definitions against oracle/ops.py and against each other, the float32 restatements against the float64 forms within the bound
the GPU module asserts, every claim of the row tables, the conversion classes of the input sets, and the records that the four
real table builders of device.Ops upload (tests/fake_device.py replaces them, so no other CPU test sees them).

One figure of include/ghm.h did not survive this module: it called the collapse record "40-byte"; four pointers and four ints are
48 bytes, which is what device.Ops.collapse_table uploads and what the kernel's struct is.  The header says 48 now and the entry
point asserts it at compile time, as the pack and transpose entry points already did.
"""
import numpy as np
import pytest

from oracle import lp as LP
from oracle import ops as O
from tests import weight_operand_ref as R

DTYPES = R.LP_DTYPES + R.SPLIT_DTYPES


def corr_taps(wp, n):
    """wp[C][n n][K] -> correlation taps [K][C][n][n]"""
    C, T, K = wp.shape
    return np.ascontiguousarray(wp.reshape(C, n, n, K).transpose(3, 0, 1, 2))


# ---- round trips ----
@pytest.mark.parametrize("row,why", R.PACK_ROWS, ids=[str(r) for r, _ in R.PACK_ROWS])
def test_unpacking_a_pack_returns_the_rounded_operand_and_zeros(row, why):
    red, T, rows, tr = row
    for dtype in DTYPES:
        wp = R.pack_inputs(row, dtype)
        h = R.lp_pack(wp, red, T, rows, tr, dtype)
        assert h.dtype == np.uint16 and 2 * h.size == R.weight_bytes(red, T, rows, dtype)
        back = R.lp_unpack(h, red, T, rows, dtype)
        A = R.operand(wp, red, T, rows, tr)
        with np.errstate(over='ignore'):
            want = R.pieces(A, dtype)
        inside = np.zeros(back.shape[1:], bool)
        inside[:red, :, :rows] = True
        for p in range(R.PLANES[dtype]):
            assert R.bits_equal(back[p][:red, :, :rows], want[p]), (row, dtype, p)
            assert not back[p][~inside].view(np.uint32).any(), (row, dtype, p, "padding is +0 in bits")
        if dtype == 'bf16x3':       # the three planes are the value itself
            with np.errstate(over='ignore', invalid='ignore'):
                total = back.astype(np.float64).sum(0).astype(np.float32)
            assert np.array_equal(total[:red, :, :rows], A)
    # the transposed pack is the plain pack of the transposed copy
    if tr:
        wp = R.pack_inputs(row, 'bf16')
        assert np.array_equal(R.lp_pack(wp, red, T, rows, 1, 'bf16'), R.lp_pack(R.transpose(wp), red, T, rows, 0, 'bf16'))


@pytest.mark.parametrize("row,why", R.TRANSPOSE_ROWS, ids=[str(r) for r, _ in R.TRANSPOSE_ROWS])
def test_transposing_twice_is_the_identity(row, why):
    C, T, K = row
    wp = R.f32_source(row)
    wT = R.transpose(wp)
    assert wT.shape == (K, T, C) and wT.flags['C_CONTIGUOUS']
    assert R.bits_equal(R.transpose(wT), wp)
    c, t, k = C - 1, T // 3, K // 2
    assert wT[k, T - 1 - t, c] == wp[c, t, k]
    if T > 1:
        assert not R.bits_equal(wT, np.ascontiguousarray(wp.transpose(2, 1, 0))), "the taps flip"


# ---- collapse against the oracle's own operators ----
def test_collapse_mode_0_is_the_5x5_convolution_of_the_nearest_upsampling():
    r = np.random.RandomState(3)
    N, C, K, H, W = 2, 3, 4, 5, 6
    x = r.randn(N, C, H, W)
    wp = r.randn(C, 25, K)
    fine = O.corr2d_fwd(O.upscale_nearest_fwd(x), corr_taps(wp, 5), 1, 2)
    wpc = R.collapse(wp, 0)                                                     # [C][9][4][K]
    wc = np.ascontiguousarray(wpc.reshape(C, 3, 3, 4 * K).transpose(3, 0, 1, 2))  # filters ordered (pq, k)
    pp = O.corr2d_fwd(x, wc, 1, 1).reshape(N, 2, 2, K, H, W)                    # [n][p][q][k][i][j]
    hi = pp.transpose(0, 3, 4, 1, 5, 2).reshape(N, K, 2 * H, 2 * W)
    assert np.abs(hi - fine).max() <= 1e-12 * np.abs(fine).max()


def test_collapse_mode_1_is_the_oracles_bilinear_collapse():
    r = np.random.RandomState(4)
    C, K = 3, 5
    wp = r.randn(C, 9, K)
    want = O.bilinear_conv_collapse(corr_taps(wp, 3))                           # [pq][K, C, 3, 3]
    got = R.collapse(wp, 1).reshape(C, 3, 3, 4, K)
    for pq in range(4):
        assert np.allclose(got[:, :, :, pq, :].transpose(3, 0, 1, 2), want[pq], rtol=0, atol=1e-15), pq
    assert (R.collapse_terms(1) > 0).sum() == 25, "25 of the 36 collapsed taps are non-zero"
    dw = r.randn(C, 9, 4, K)
    back = O.bilinear_conv_expand([np.ascontiguousarray(dw.reshape(C, 3, 3, 4, K)[:, :, :, pq, :].transpose(3, 0, 1, 2)) for pq in range(4)])
    assert np.allclose(corr_taps(R.expand(dw, 1), 3), back, rtol=0, atol=1e-14)


@pytest.mark.parametrize("mode", [0, 1])
def test_expand_is_the_adjoint_of_collapse(mode):
    r = np.random.RandomState(5 + mode)
    C, K = 4, 3
    w, g = r.randn(C, R.TAPS[mode] ** 2, K), r.randn(C, 9, 4, K)
    a, b = (R.collapse(w, mode) * g).sum(), (w * R.expand(g, mode)).sum()
    assert abs(a - b) <= 1e-12 * max(abs(a), 1.0)


def test_term_counts_come_from_the_tap_maps():
    assert set(R.collapse_terms(0).ravel()) == {1, 2, 4}
    assert set(R.collapse_terms(1).ravel()) == {0, 1, 2, 3, 4, 6, 9}
    assert set(R.expand_terms(0).ravel()) == {4} and R.expand_terms(0).size == 25
    assert set(R.expand_terms(1).ravel()) == {9} and R.expand_terms(1).size == 9
    # the maps against the kernels' own spelling of them (csrc/elementwise.hip)
    grp = lambda p, a: (0 if a < 2 else (1 if a < 4 else 2)) if p == 0 else (0 if a < 1 else (1 if a < 3 else 2))
    assert all(R.upconv_group(p, a) == grp(p, a) for p in range(2) for a in range(5))

    def cf(p, r, a):
        if p == 0:
            return (1.0 if a == 1 else 0.5) if r == 1 else (0.5 if (r == 0 and a == 0) or (r == 2 and a == 2) else 0.0)
        return 0.0 if r == 0 else (0.5 if a == 1 else (1.0 if (r == 1 and a == 0) or (r == 2 and a == 2) else 0.0))
    assert all(R.blconv_coef(p, r, a) == cf(p, r, a) for p in range(2) for r in range(3) for a in range(3))
    assert np.array_equal(R.tap_coef(1), np.stack(O._BL_COEF))
    # every fine tap is spread with total weight 1 per parity class in mode 0, and the mode-1 coefficients are powers of two
    assert np.array_equal(R.coef(0).sum(0), np.ones((4, 25)))
    assert set(np.unique(R.coef(1))) == {0.0, 0.25, 0.5, 1.0}
    # mode 1: the outputs with parity 1 and coarse tap 0 have no term at all
    t = R.collapse_terms(1).reshape(3, 3, 2, 2)
    assert not t[0, :, 1, :].any() and not t[:, 0, :, 1].any() and (t == 0).sum() == 11


# ---- the float32 restatements inside the bound the GPU module asserts ----
def within(got, ref, M, k):
    err = np.abs(got.astype(np.float64) - ref)
    return bool((err <= k * R.U * M).all())


@pytest.mark.parametrize("row,why", R.COLLAPSE_ROWS, ids=[str(r) for r, _ in R.COLLAPSE_ROWS])
def test_restated_collapse_stays_inside_its_bound(row, why):
    C, K, mode, has_bias = row
    d = R.collapse_inputs(row)
    got, ref = R.restate32_collapse(d['wp'], mode), R.collapse(d['wp'], mode)
    assert got.dtype == np.float32 and got.shape == ref.shape == (C, 9, 4, K)
    assert within(got, ref, R.collapse_M(d['wp'], mode), R.collapse_k(mode, C, K))
    assert R.rel(got, ref) <= R.REL_L2
    none = np.broadcast_to((R.collapse_terms(mode) == 0)[None, :, :, None], got.shape)
    assert not got[none].view(np.uint32).any(), "an output without a term is +0.0 in bits"
    assert (none.any()) == (mode == 1)
    assert (d['wp'] == 0).any() and np.signbit(d['wp'][d['wp'] == 0]).any(), "exact zeros of both signs are in the input"
    if has_bias:
        assert R.bias4(d['bias']).shape == (4 * K,) and R.bits_equal(R.bias4(d['bias']).reshape(4, K)[3], d['bias'])


@pytest.mark.parametrize("row,why", R.EXPAND_ROWS, ids=[str(r) for r, _ in R.EXPAND_ROWS])
def test_restated_expand_stays_inside_its_bound(row, why):
    C, K, mode = row
    d = R.expand_inputs(row)
    plain = R.restate32_expand(d['dwpc'], mode)
    assert within(plain, R.expand(d['dwpc'], mode), R.expand_M(d['dwpc'], mode), R.expand_k(mode, C, K, False))
    acc = R.restate32_expand(d['dwpc'], mode, d['prev'])
    ref = R.expand(d['dwpc'], mode) + d['prev']
    assert within(acc, ref, R.expand_M(d['dwpc'], mode, d['prev']), R.expand_k(mode, C, K, True))
    assert R.bits_equal(acc, d['prev'] + plain), "accumulate = fl32(previous + increment)"
    assert R.rel(plain, R.expand(d['dwpc'], mode)) <= R.REL_L2


# ---- the conversion classes of the input sets ----
def test_bf16_inputs_carry_every_finite_class_and_round_to_nearest_even():
    bits = R.bf16_special_bits()
    x = bits.view(np.float32)
    assert np.isfinite(x).all() and bits.size == 42
    for name, vals in R.BF16_BITS.items():
        if name not in R.NONFINITE_CLASSES:
            assert all(v in bits and (v ^ 0x80000000) in bits for v in vals), name
    with np.errstate(over='ignore'):
        h = R.halfwords(LP.round_bf16(x), 'bf16')
    assert np.array_equal(h, R.rne_bf16_bits(bits))
    look = dict(zip(bits.tolist(), h.tolist()))
    assert look[0x3f808000] == 0x3f80 and look[0x3f818000] == 0x3f82          # ties: to the even upper half
    assert look[0x3f807fff] == 0x3f80 and look[0x3f808001] == 0x3f81
    assert look[0x00008000] == 0x0000 and look[0x00018000] == 0x0002 and look[0x007fffff] == 0x0080   # denormals are not flushed
    assert look[0x80000000] == 0x8000 and look[0x7f7fffff] == 0x7f80
    for row, _ in R.PACK_ROWS:
        assert np.array_equal(R.pack_inputs(row, 'bf16').reshape(-1)[:bits.size].view(np.uint32), bits), row


def test_fp16_inputs_carry_the_fp16_classes():
    v = R.f16_special_values()
    with np.errstate(over='ignore'):
        h = {k: int(R.halfwords(LP.round_f16(np.array([x], np.float32)), 'f16')[0]) for k, x in v.items()}
    assert h['65504'] == 0x7bff and h['65520: tie to inf'] == 0x7c00 and h['below 65520'] == 0x7bff and h['FLT_MAX'] == 0x7c00
    assert h['2^-24'] == 0x0001 and h['2^-25: tie to 0'] == 0x0000 and h['above 2^-25'] == 0x0001 and h['below 2^-25'] == 0x0000
    assert h['1.5 2^-24: tie to 2^-23'] == 0x0002 and h['2.5 2^-24: tie to 2^-23'] == 0x0002
    assert h['2^-14'] == 0x0400 and h['above 2^-14'] == 0x0400 and h['below 2^-14'] == 0x0400
    assert h['2^-14 (1 - 2^-11): tie to 2^-14'] == 0x0400 and h['1023 2^-24: the largest denormal'] == 0x03ff
    assert h['1 + 2^-11: tie to 1'] == 0x3c00 and h['1 + 3 2^-11: tie to 1 + 2^-9'] == 0x3c02
    assert h['above 1 + 2^-11'] == 0x3c01 and h['below 1 + 2^-11'] == 0x3c00
    assert h['0'] == 0 and h['fp32 denormal'] == 0
    bits = R.f16_special_bits()
    assert np.isfinite(bits.view(np.float32)).all() and bits.size == 2 * len(v)
    with np.errstate(over='ignore'):
        neg = R.halfwords(LP.round_f16(-np.array(list(v.values()), np.float32)), 'f16')
    assert np.array_equal(neg, np.array(list(h.values()), np.uint16) | 0x8000), "both signs round alike"
    for row, _ in R.PACK_ROWS:
        assert np.array_equal(R.pack_inputs(row, 'f16').reshape(-1)[:bits.size].view(np.uint32), bits), row


def test_split_inputs_are_the_split_tests_value_set():
    x = R.split_values((5, 9, 7))
    assert np.array_equal(x.reshape(-1)[:8], np.array(R.SPLIT_SPECIALS, np.float32)) and np.signbit(x.reshape(-1)[1])
    assert np.isfinite(x).all()
    e = np.log2(np.abs(x[x != 0]))
    assert e.min() < -40 and e.max() > 40, "the values span the exponent range"
    p = LP.split_bf16x3(x)
    assert np.array_equal((p[0].astype(np.float64) + p[1] + p[2]).astype(np.float32), x)


def test_no_input_set_holds_a_nan_or_an_inf():
    for row, _ in R.PACK_ROWS:
        for dtype in DTYPES:
            assert np.isfinite(R.pack_inputs(row, dtype)).all()
    for row, _ in R.COLLAPSE_ROWS:
        assert np.isfinite(R.collapse_inputs(row)['wp']).all()
    for row, _ in R.EXPAND_ROWS:
        d = R.expand_inputs(row)
        assert np.isfinite(d['dwpc']).all() and np.isfinite(d['prev']).all()
        assert (d['dwpc'] == 0).any() and np.signbit(d['dwpc'][d['dwpc'] == 0]).any()


# ---- every claim of the row tables ----
# (nblk, rpad, blocks, zero channels, zero rows, all-zero channel blocks)
PACK_FACTS = {
    (16, 9, 128, 0): (2, 128, 9, 0, 0, []),
    (5, 9, 7, 0): (2, 128, 9, 11, 121, [1]),
    (24, 25, 200, 0): (4, 256, 100, 8, 56, [3]),
    (40, 9, 48, 1): (6, 128, 27, 8, 80, [5]),
    (17, 1, 129, 1): (4, 256, 4, 15, 127, [3]),
    (8, 4, 3, 0): (2, 128, 4, 8, 125, [1]),
    (1000, 1, 96, 0): (126, 128, 63, 8, 32, [125]),
    (32, 1, 600, 1): (4, 640, 10, 0, 40, []),
    (12, 9, 130, 1): (2, 256, 18, 4, 126, []),
    (3, 4, 260, 1): (2, 384, 12, 13, 124, [1]),
}


def test_pack_rows_reach_what_they_claim():
    rows = [r for r, _ in R.PACK_ROWS]
    assert set(rows) == set(PACK_FACTS) and all(why for _, why in R.PACK_ROWS)
    for red, T, rows_, tr in rows:
        nblk, rpad, blocks, zc, zr, zb = PACK_FACTS[(red, T, rows_, tr)]
        assert R.lp_geometry(red, rows_) == (nblk, rpad) and nblk % 2 == 0 and rpad % 128 == 0
        assert R.plane_units(red, T, rows_) % R.BLOCK == 0, "an item ends on a block boundary"
        assert R.pack_blocks(red, T, rows_) == blocks == R.plane_units(red, T, rows_) // R.BLOCK
        assert nblk * 8 - red == zc and rpad - rows_ == zr
        C, T_, K = R.pack_wp_shape((red, T, rows_, tr))
        h = R.lp_unpack(R.lp_pack(np.ones((C, T_, K), np.float32), red, T, rows_, tr, 'bf16'), red, T, rows_, 'bf16')[0]
        blk = h.reshape(nblk, 8, T, rpad)
        assert [b for b in range(nblk) if not blk[b].any()] == zb
        assert (h == 0).sum() == (nblk * 8 * rpad - red * rows_) * T
        assert R.pack_desc_args((red, T, rows_, tr))[2] ** 2 == T
        assert R.lp_weight_bytes(red, T, rows_) == blocks * R.BLOCK * 16
        assert R.split_weight_bytes(red, T, rows_, 3) == 3 * blocks * R.BLOCK * 16
    assert max(PACK_FACTS[r][2] for r in rows) == 100 == PACK_FACTS[(24, 25, 200, 0)][2]
    assert (1000 % 16, 40 % 16, 17 % 16) == (8, 8, 1)
    # neighbours of the table differ in T, rpad and transposed, in both directions
    order = R.PACK_TABLE_ORDER
    assert sorted(order) == list(range(len(rows)))
    for a, b in zip(order, order[1:]):
        ra, rb = rows[a], rows[b]
        assert ra[1] != rb[1] and R.lp_geometry(ra[0], ra[2])[1] != R.lp_geometry(rb[0], rb[2])[1] and ra[3] != rb[3], (ra, rb)
    assert sum(PACK_FACTS[r][2] for r in rows) == 256 <= 290


# (tiles along C, tiles along K, C ragged, K ragged, blocks)
TRANSPOSE_FACTS = {(5, 9, 7): (1, 1, True, True, 9), (48, 9, 40): (2, 2, True, True, 36), (33, 25, 32): (2, 1, True, False, 50),
                   (1000, 1, 96): (32, 3, True, False, 96), (64, 4, 3): (2, 1, False, True, 8), (32, 9, 32): (1, 1, False, False, 9)}


def test_transpose_rows_reach_what_they_claim():
    assert [r for r, _ in R.TRANSPOSE_ROWS] == list(TRANSPOSE_FACTS)
    for (C, T, K), (ct, kt, rc, rk, blocks) in TRANSPOSE_FACTS.items():
        assert (R.ceil_div(C, 32), R.ceil_div(K, 32), C % 32 != 0, K % 32 != 0) == (ct, kt, rc, rk)
        assert R.transpose_blocks(C, T, K) == blocks == T * ct * kt
    assert 1000 == 31 * 32 + 8 and 33 == 32 + 1
    assert {(rc, rk) for _, _, rc, rk, _ in TRANSPOSE_FACTS.values()} == {(True, True), (True, False), (False, True), (False, False)}
    assert any(K < 32 for _, _, K in TRANSPOSE_FACTS) and any(T == 1 for _, T, _ in TRANSPOSE_FACTS)


def test_collapse_rows_reach_what_they_claim():
    rows = [r for r, _ in R.COLLAPSE_ROWS]
    assert rows == [(5, 1, 0, True), (8, 8, 0, True), (3, 7, 1, True), (16, 128, 1, True), (4, 32, 0, False)]
    blocks = [R.collapse_blocks(C, K) for C, K, _, _ in rows]
    assert blocks == [1, 10, 4, 290, 19] and max(blocks) == 290
    assert 36 * 5 * 1 + 4 * 1 == 184 <= 256                                    # weights and bias share one block
    assert 36 * 8 * 8 == 2304 == 9 * 256                                       # the bias starts block 9
    assert (36 * 3 * 7) % 256 == 244 and 4 * 7 == 28 and 244 + 28 > 256         # the bias straddles blocks 2 and 3
    assert 36 * 16 * 128 == 288 * 256 and 4 * 128 == 2 * 256                   # the bias is blocks 288 and 289
    assert 36 * 4 * 32 == 18 * 256 and R.collapse_blocks(4, 32) == 19          # the nineteenth block has nothing to write
    assert {m for _, _, m, _ in rows} == {0, 1}


def test_expand_rows_reach_what_they_claim():
    rows = [r for r, _ in R.EXPAND_ROWS]
    assert rows == [(5, 1, 0), (8, 8, 1), (3, 7, 1), (16, 128, 0), (4, 32, 1)]
    reserved = [R.expand_blocks(C, K, m) for C, K, m in rows]
    used = [R.ceil_div(R.TAPS[m] ** 2 * C * K, 256) for C, K, m in rows]
    assert reserved == [1, 7, 3, 200, 13] and used == [1, 3, 1, 200, 5]
    assert 25 * 16 * 128 == 200 * 256 and 9 * 4 * 32 == 4 * 256 + 128 and 9 * 8 * 8 == 576 and 9 * 3 * 7 == 189
    assert all(r > u for r, u, (_, _, m) in zip(reserved, used, rows) if m == 1)


# ---- the records the real table builders upload ----
class StubDev:
    """what device.Ops needs of a Device to build a table: made-up addresses, and the bytes of every upload kept"""
    h = None

    def __init__(self):
        self.next, self.uploads, self.sizes = 0x7f0000001000, {}, {}

    def alloc(self, nbytes):
        p = self.next
        self.next += (int(nbytes) + 255) // 256 * 256
        self.sizes[p] = int(nbytes)
        return p

    def h2d(self, ptr, arr):
        self.uploads[ptr] = np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()


@pytest.fixture
def stub():
    from gan_heightmaps_amd import device as D
    dev = StubDev()
    return dev, D.Ops(dev), D


def check_table(dev, table, record, n, blocks):
    ptr, count, total = table
    begin, want_total = R.begins(blocks)
    assert count == n and total == want_total, "the returned total is the sum of the restated blocks per item"
    raw = dev.uploads[ptr]
    assert raw.size == n * record[1] and dev.sizes[ptr] >= raw.size
    rec = R.decode(raw, record)
    assert np.array_equal(rec['block_begin'], begin), "block_begin is the running sum of the restated blocks per item"
    # the decoder reads each field at the offset the header states: rebuilt field by field, the bytes are the upload
    back = np.zeros(raw.size, np.uint8)
    for name, fmt, off in record[0]:
        w = np.dtype(fmt).itemsize
        for i in range(n):
            back[i * record[1] + off:i * record[1] + off + w] = np.array([rec[name][i]], fmt).view(np.uint8)
    assert np.array_equal(back, raw), "no byte of a record lies outside the fields of include/ghm.h"
    return rec


def test_lp_pack_table_writes_the_records_of_the_header(stub):
    dev, ops, D = stub
    rows = [R.PACK_ROWS[i][0] for i in R.PACK_TABLE_ORDER]
    items = []
    for i, (red, T, rows_, tr) in enumerate(rows):
        src = D.DevTensor(dev, 0x1000 + 64 * i + 4, (1, red * T * rows_, 1, 1)) if i % 2 else 0x1000 + 64 * i + 12
        items.append((src, 0x900000 + 0x10000 * i, red, T, rows_, tr))
    rec = check_table(dev, ops.lp_pack_table(items), R.LP_RECORD, len(rows), [R.pack_blocks(*r[:3]) for r in rows])
    assert R.LP_RECORD[1] == 48
    for i, (red, T, rows_, tr) in enumerate(rows):
        assert (rec['red'][i], rec['T'][i], rec['rows'][i], rec['transposed'][i], rec['zero'][i]) == (red, T, rows_, tr, 0)
        assert (rec['nblk'][i], rec['rpad'][i]) == R.lp_geometry(red, rows_)
        assert rec['wq'][i] == 0x900000 + 0x10000 * i and rec['wp'][i] == 0x1000 + 64 * i + (4 if i % 2 else 12)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.lp_pack_table([(0x1000, 0x900008, 16, 9, 128, 0)])


def test_transpose_table_writes_the_records_of_the_header(stub):
    dev, ops, D = stub
    rows = [r for r, _ in R.TRANSPOSE_ROWS]
    items = [(D.DevTensor(dev, 0x1000 * (i + 1) + 4, (1, C * T * K, 1, 1)), D.DevTensor(dev, 0x800000 + 0x1000 * i, (1, C * T * K, 1, 1)), C, T, K)
             for i, (C, T, K) in enumerate(rows)]
    rec = check_table(dev, ops.transpose_table(items), R.TRANSPOSE_RECORD, len(rows), [R.transpose_blocks(*r) for r in rows])
    assert R.TRANSPOSE_RECORD[1] == 32
    for i, (C, T, K) in enumerate(rows):
        assert (rec['C'][i], rec['T'][i], rec['K'][i]) == (C, T, K)
        assert (rec['wp'][i], rec['wpT'][i]) == (items[i][0].ptr, items[i][1].ptr)


def test_collapse_table_writes_the_records_of_the_header(stub):
    dev, ops, D = stub
    rows = [r for r, _ in R.COLLAPSE_ROWS]
    t = lambda p: D.DevTensor(dev, p, (1, 1, 1, 1))
    items = [(t(0x1000 * (i + 1)), t(0x100000 + 16 * i) if b else None, t(0x200000 + 0x1000 * i), t(0x300000 + 16 * i), C, K, mode)
             for i, (C, K, mode, b) in enumerate(rows)]
    rec = check_table(dev, ops.collapse_table(items), R.COLLAPSE_RECORD, len(rows), [R.collapse_blocks(C, K) for C, K, _, _ in rows])
    assert R.COLLAPSE_RECORD[1] == 48, "four pointers and four ints (include/ghm.h used to say 40)"
    for i, (C, K, mode, b) in enumerate(rows):
        assert (rec['C'][i], rec['K'][i], rec['mode'][i]) == (C, K, mode)
        assert (rec['wp5'][i], rec['wpc'][i], rec['bias4'][i]) == (items[i][0].ptr, items[i][2].ptr, items[i][3].ptr)
        assert rec['bias'][i] == (items[i][1].ptr if b else 0)
    # an item without a mode is mode 0
    assert R.decode(dev.uploads[ops.collapse_table([items[0][:6]])[0]], R.COLLAPSE_RECORD)['mode'][0] == 0


def test_expand_table_writes_the_records_of_the_header(stub):
    dev, ops, D = stub
    rows = [r for r, _ in R.EXPAND_ROWS]
    t = lambda p: D.DevTensor(dev, p, (1, 1, 1, 1))
    items = [(t(0x1000 * (i + 1)), t(0x200000 + 0x1000 * i), C, K, mode) for i, (C, K, mode) in enumerate(rows)]
    rec = check_table(dev, ops.expand_table(items), R.EXPAND_RECORD, len(rows), [R.expand_blocks(*r) for r in rows])
    assert R.EXPAND_RECORD[1] == 32
    for i, (C, K, mode) in enumerate(rows):
        assert (rec['C'][i], rec['K'][i], rec['mode'][i]) == (C, K, mode)
        assert (rec['dwpc'][i], rec['dwp5'][i]) == (items[i][0].ptr, items[i][1].ptr)
