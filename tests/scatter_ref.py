"""The scatter (gan_heightmaps_amd/scatter.py, csrc/scatter.hip) restated in numpy: the mixer in uint32 arithmetic, the
chance operation by operation in float32, the thinning as a sort by (priority, row, col) followed by greedy acceptance against an
occupancy grid -- and, independent of that, the Jacobi iteration of the local rule and the two invariants of a Poisson-disk
thinning.  The cases of the host build's and the device's tests are made here, once."""
import functools

import numpy as np

TILE = 32
MAX_S2 = 1024
ONE = 1 << 24
NONE, UNDECIDED, KEPT, REJECTED = 0, 1, 2, 3
MIX_A, MIX_B, MIX_STEP = 0x7feb352d, 0x846ca68b, 0x9e3779b9
TABLE_FLOATS = 384
DIST_NONE = -1

SHAPES = ((1, 1), (1, 300), (300, 1), (33, 65), (70, 45), (97, 130))
S2S = (1, 2, 3, 16, 50, 1024)
KINDS = ('random', 'sparse', 'equal', 'none', 'corner')


# ---- the mixer ----------------------------------------------------------------------------------------------------------------
def mix(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(MIX_A)
    x ^= x >> np.uint32(15)
    x *= np.uint32(MIX_B)
    x ^= x >> np.uint32(16)
    return x


def hash32(seed, stream, row, col):
    """seed: an integer, taken modulo 2^64; stream: an integer; row, col: integer arrays of world coordinates, taken modulo 2^32"""
    seed = int(seed) & ((1 << 64) - 1)
    row = (np.asarray(row, np.int64) & 0xFFFFFFFF).astype(np.uint32)
    col = (np.asarray(col, np.int64) & 0xFFFFFFFF).astype(np.uint32)
    row, col = np.broadcast_arrays(row, col)
    k = np.uint32(MIX_STEP)
    with np.errstate(over='ignore'):
        x = mix(np.uint32(seed & 0xFFFFFFFF) + k)
        x = mix((x ^ np.uint32(seed >> 32)) + k)
        x = mix((x ^ np.uint32(stream)) + k)
        x = mix((x ^ row) + k)
        return mix((x ^ col) + k)


def candidates(chance, seed, origin=(0, 0)):
    """-> (state uint8: 1 a candidate, 0 none; priority uint32)"""
    H, W = chance.shape
    row = origin[0] + np.arange(H, dtype=np.int64)[:, None]
    col = origin[1] + np.arange(W, dtype=np.int64)[None, :]
    state = ((hash32(seed, 0, row, col) >> np.uint32(8)) < np.asarray(chance, np.uint32)).astype(np.uint8)
    return state, hash32(seed, 1, row, col)


# ---- the chance ---------------------------------------------------------------------------------------------------------------
def slope_bounds():
    """the squared tangents of k 90 / 64 degrees, k = 1 .. 63, in float64, rounded once"""
    return (np.tan(np.radians(np.arange(1, 64, dtype=np.float64) * (90.0 / 64))) ** 2).astype(np.float32)


def tables(altitude, slope):
    """altitude: 256 weights, slope: 64 weights -> the 384 float32 the device reads"""
    t = np.zeros(TABLE_FLOATS, np.float32)
    t[:256] = np.asarray(altitude, np.float32)
    t[256:319] = slope_bounds()
    t[320:] = np.asarray(slope, np.float32)
    return t


def chance(h, tab, height_scale, density, dist2=None, water=None, blocked=None, threshold=1):
    f = np.float32
    h = np.asarray(h, f)
    H, W = h.shape
    with np.errstate(all='ignore'):
        t = (h * f(255.0)).astype(f) + f(0.5)
        ai = np.where(~(t >= 0), 0, np.where(t >= 255, 255, np.trunc(np.where(np.isfinite(t), t, 0)))).astype(np.int64)
        A = tab[ai]
        xs, ys = np.arange(W), np.arange(H)
        half = f(np.float64(height_scale) / 2)
        gx = ((h[:, np.minimum(xs + 1, W - 1)] - h[:, np.maximum(xs - 1, 0)]).astype(f) * half).astype(f)
        gy = ((h[np.minimum(ys + 1, H - 1), :] - h[np.maximum(ys - 1, 0), :]).astype(f) * half).astype(f)
        g2 = ((gx * gx).astype(f) + (gy * gy).astype(f)).astype(f)
        bins = (tab[256:319][None, None, :] <= g2[:, :, None]).sum(axis=2)
        p = (A * tab[320 + bins]).astype(f)
        if water is not None:
            water = np.asarray(water, f)
            n = water.size - 1
            d = np.asarray(dist2, np.int64)
            p = (p * water[np.where((d >= 0) & (d < n), d, n)]).astype(f)
        p = (p * f(density)).astype(f)
        v = (p * f(16777216.0)).astype(f)
        out = np.where(~(v >= 0), 0, np.where(v >= f(16777216.0), ONE, np.trunc(np.where(np.isfinite(v), v, 0)))).astype(np.uint32)
    if blocked is not None:
        out = np.where(np.asarray(blocked).astype(np.int64) >= threshold, np.uint32(0), out)
    return out.astype(np.uint32)


# ---- the thinning -------------------------------------------------------------------------------------------------------------
def reach(s2):
    R = 0
    while (R + 1) * (R + 1) < s2:
        R += 1
    return R


def disk(s2):
    """the offsets (dy, dx) with dy^2 + dx^2 < s2, the centre included"""
    R = reach(s2)
    dy, dx = np.mgrid[-R:R + 1, -R:R + 1]
    on = dy * dy + dx * dx < s2
    return dy[on], dx[on]


def thin(state, priority, s2):
    """sort by (priority, row, col), then greedy acceptance against an occupancy grid -> the states 0, 2, 3"""
    state = np.asarray(state, np.uint8)
    H, W = state.shape
    R = reach(s2)
    dy, dx = disk(s2)
    rows, cols = np.nonzero(state == UNDECIDED)
    order = np.lexsort((cols, rows, np.asarray(priority, np.uint32)[rows, cols]))
    taken = np.zeros((H + 2 * R, W + 2 * R), bool)
    out = np.where(state == UNDECIDED, REJECTED, NONE).astype(np.uint8)
    for k in order:
        r, c = int(rows[k]), int(cols[k])
        if not taken[r + R, c + R]:
            out[r, c] = KEPT
            taken[r + R + dy, c + R + dx] = True
    return out


def _shifted(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx], ``fill`` outside the plane"""
    H, W = a.shape
    b = np.full((H, W), fill, a.dtype)
    ys0, ys1 = max(0, -dy), min(H, H - dy)
    xs0, xs1 = max(0, -dx), min(W, W - dx)
    if ys0 < ys1 and xs0 < xs1:
        b[ys0:ys1, xs0:xs1] = a[ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx]
    return b


def jacobi(state, priority, s2, max_sweeps=None):
    """the local rule iterated from the old plane into a new one until a sweep changes nothing -> (states, sweeps: the last, which
    changed nothing, included)"""
    st = np.asarray(state, np.uint8).copy()
    pr = np.asarray(priority, np.uint32).astype(np.int64)
    dys, dxs = disk(s2)
    sweeps = 0
    while True:
        sweeps += 1
        rejected = np.zeros(st.shape, bool)
        pending = np.zeros(st.shape, bool)
        for dy, dx in zip(dys.tolist(), dxs.tolist()):
            if dy == 0 and dx == 0:
                continue
            ns = _shifted(st, dy, dx, NONE)
            npr = _shifted(pr, dy, dx, 0)
            earlier = (npr < pr) | ((npr == pr) & ((dy < 0) | ((dy == 0) & (dx < 0))))
            rejected |= earlier & (ns == KEPT)
            pending |= earlier & (ns == UNDECIDED)
        new = st.copy()
        und = st == UNDECIDED
        new[und & rejected] = REJECTED
        new[und & ~rejected & ~pending] = KEPT
        if np.array_equal(new, st):
            return st, sweeps
        st = new
        assert max_sweeps is None or sweeps <= max_sweeps


def invariants(state_in, priority, s2, out):
    """no two kept points conflict; every rejected candidate has an earlier kept candidate in conflict; every candidate is decided
    and nothing else is -> None, or a sentence that says what is wrong"""
    state_in, out = np.asarray(state_in), np.asarray(out)
    cand = state_in == UNDECIDED
    if not np.array_equal(out != NONE, cand) or (out == UNDECIDED).any():
        return "the decided cells are not the candidates"
    kept = out == KEPT
    pr = np.asarray(priority, np.uint32).astype(np.int64)
    dys, dxs = disk(s2)
    excused = np.zeros(out.shape, bool)
    for dy, dx in zip(dys.tolist(), dxs.tolist()):
        if dy == 0 and dx == 0:
            continue
        nk = _shifted(kept, dy, dx, False)
        if (kept & nk).any():
            return "two kept points within the spacing"
        npr = _shifted(pr, dy, dx, 0)
        earlier = (npr < pr) | ((npr == pr) & ((dy < 0) | ((dy == 0) & (dx < 0))))
        excused |= nk & earlier
    if ((out == REJECTED) & ~excused).any():
        return "a rejected candidate without an earlier kept one in conflict"
    return None


def points(out):
    """the kept cells, (row, col) in row-major order"""
    return np.argwhere(np.asarray(out) == KEPT).astype(np.int32)


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def thin_case(kind, shape, seed=0):
    """-> (state uint8, priority uint32)"""
    H, W = shape
    rng = np.random.RandomState(1000 * H + W + 7 * seed + KINDS.index(kind))
    prio = rng.randint(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)
    if kind == 'random':
        state = np.ones(shape, np.uint8)
    elif kind == 'sparse':
        state = (rng.rand(H, W) < 0.1).astype(np.uint8)
    elif kind == 'equal':
        state = (rng.rand(H, W) < 0.7).astype(np.uint8)
        prio[:] = 0x80000000
    elif kind == 'none':
        state = np.zeros(shape, np.uint8)
    elif kind == 'corner':
        state = np.zeros(shape, np.uint8)
        state[H - 1, W - 1] = 1
    else:
        raise ValueError(kind)
    return state, prio


def staircase(shape, rising):
    """every cell a candidate, priorities rising (or falling) along the line: with s2 = 2 one decision per Jacobi sweep"""
    H, W = shape
    n = H * W
    ramp = np.arange(n, dtype=np.uint32) * np.uint32(3) + np.uint32(5)
    prio = (ramp if rising else ramp[::-1]).reshape(shape).copy()
    return np.ones(shape, np.uint8), prio


@functools.lru_cache(maxsize=None)
def thin_expected(kind, shape, s2):
    state, prio = thin_case(kind, shape)
    return thin(state, prio, s2)


def heights(H, W, seed, lo=0.0, hi=1.0):
    """smooth hills with some roughness, float32, in about [lo, hi]"""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    z = 0.5 + 0.25 * np.sin(y / 7.0 + rng.rand() * 6) * np.cos(x / 5.0 + rng.rand() * 6) + 0.2 * np.sin((x + y) / 17.0)
    z += 0.02 * rng.randn(H, W)
    return (lo + (hi - lo) * z).astype(np.float32)


def habitat_tables(seed):
    """weights in [0, 1] with zeros, ones and fades -> (tables, water weights for reach 5)"""
    rng = np.random.RandomState(seed)
    alt = np.clip(1.5 - np.abs(np.arange(256) - 140) / 60.0, 0, 1)
    slope = np.clip(1.25 - np.arange(64) / 24.0, 0, 1)
    water = np.concatenate([np.clip(0.2 + 0.8 * (1 - np.sqrt(np.arange(26)) / 5.0), 0, 1), [0.2]])
    water[:2] = 0.0
    alt[rng.randint(0, 256, 5)] = rng.rand(5)
    return tables(alt, slope), water.astype(np.float32)
