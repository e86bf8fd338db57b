"""The viewshed's definition (include/ghm.h, section "viewshed") restated in numpy int64 and plain Python integers, on
its own: nothing here imports the package.  Two forms -- ``viewshed_loop``, a double loop over targets and steps in Python
integers, and ``viewshed``, vectorised over the targets per step -- and the case generators the host build's and the device's
tests share.  ``expected(name)`` computes a case's answer once.

    zq = int32(rint(float32(h) * float32(height_scale * 256)))                      one float32 product, one round-half-even
    O = (r0, c0) sees T = (r, c) iff (radius2 < 0 or dy^2 + dx^2 <= radius2) and no k in 1 .. n - 1 has A_k > k D, with
    n = max(|dy|, |dx|), m the other delta's magnitude, q, f = divmod(k m, n), a = k major and q minor steps from O, b = a and
    one more minor step if f > 0, A_k = zq[a] (n - f) + zq[b] f - E n, E = zq[O] + eye_q, D = zq[T] + target_q - E.
"""
import functools

import numpy as np

BLOCK = 16                   # GHM_VIEWSHED_BLOCK
CHUNK = 128                  # GHM_VIEWSHED_CHUNK
MAX_OBSERVERS = 4096         # GHM_VIEWSHED_MAX_OBSERVERS
SHAPES = ((1, 1), (1, 300), (300, 1), (33, 65), (97, 130))


def quantise(h, height_scale):
    h = np.asarray(h, np.float32)
    return np.rint(h * np.float32(float(height_scale) * 256.0)).astype(np.int32)


def top(zq):
    """the largest zq of every BLOCK x BLOCK block, ragged at the edge: int32 [ceil(H / B), ceil(W / B)]"""
    H, W = zq.shape
    out = np.empty(((H + BLOCK - 1) // BLOCK, (W + BLOCK - 1) // BLOCK), np.int32)
    for by in range(out.shape[0]):
        for bx in range(out.shape[1]):
            out[by, bx] = zq[by * BLOCK:(by + 1) * BLOCK, bx * BLOCK:(bx + 1) * BLOCK].max()
    return out


def table(observers):
    """int32 [n, 4] of (row, col, eye_q, radius2)"""
    return np.array(observers, np.int64).reshape(-1, 4).astype(np.int32)


def _sign(v):
    return (v > 0) - (v < 0)


def sees(zq, observer, target_q, r, c):
    """one line of sight, in Python integers"""
    r0, c0, eye_q, radius2 = (int(v) for v in observer)
    dy, dx = r - r0, c - c0
    if radius2 >= 0 and dy * dy + dx * dx > radius2:
        return False
    n = max(abs(dy), abs(dx))
    if n <= 1:
        return True
    rows = abs(dy) >= abs(dx)
    m = abs(dx) if rows else abs(dy)
    sy, sx = _sign(dy), _sign(dx)
    E = int(zq[r0, c0]) + eye_q
    D = int(zq[r, c]) + int(target_q) - E
    for k in range(1, n):
        q, f = divmod(k * m, n)
        if rows:
            ar, ac = r0 + sy * k, c0 + sx * q
            br, bc = ar, ac + (sx if f else 0)
        else:
            ar, ac = r0 + sy * q, c0 + sx * k
            br, bc = ar + (sy if f else 0), ac
        if int(zq[ar, ac]) * (n - f) + int(zq[br, bc]) * f - E * n > k * D:
            return False
    return True


def viewshed_loop(zq, observers, target_q):
    """-> (count uint32, mask uint32 or None beyond 32 observers): the plain double loop"""
    obs = table(observers)
    H, W = zq.shape
    count = np.zeros((H, W), np.uint32)
    mask = np.zeros((H, W), np.uint32) if len(obs) <= 32 else None
    for i, o in enumerate(obs):
        for r in range(H):
            for c in range(W):
                if sees(zq, o, target_q, r, c):
                    count[r, c] += 1
                    if mask is not None:
                        mask[r, c] |= np.uint32(1 << i)
    return count, mask


def visible_from(zq, observer, target_q):
    """bool [H, W]: the cells one observer sees, every target at once, step by step"""
    z = np.asarray(zq).astype(np.int64)
    H, W = z.shape
    r0, c0, eye_q, radius2 = (int(v) for v in observer)
    rr, cc = np.mgrid[0:H, 0:W].astype(np.int64)
    dy, dx = (rr - r0).ravel(), (cc - c0).ravel()
    ady, adx = np.abs(dy), np.abs(dx)
    n = np.maximum(ady, adx)
    rows = ady >= adx
    m = np.where(rows, adx, ady)
    sy, sx = np.sign(dy), np.sign(dx)
    E = int(z[r0, c0]) + eye_q
    D = z.ravel() + int(target_q) - E
    vis = np.ones(H * W, bool)
    if radius2 >= 0:
        vis &= dy * dy + dx * dx <= radius2
    for k in range(1, int(n.max())):
        idx = np.flatnonzero((n > k) & vis)
        if not idx.size:
            continue
        nn, rw = n[idx], rows[idx]
        q, f = np.divmod(k * m[idx], nn)
        ar = r0 + sy[idx] * np.where(rw, k, q)
        ac = c0 + sx[idx] * np.where(rw, q, k)
        more = (f > 0).astype(np.int64)
        br = ar + np.where(rw, 0, sy[idx] * more)
        bc = ac + np.where(rw, sx[idx] * more, 0)
        A = z[ar, ac] * (nn - f) + z[br, bc] * f - E * nn
        vis[idx[A > k * D[idx]]] = False
    return vis.reshape(H, W)


def viewshed(zq, observers, target_q):
    """-> (count uint32, mask uint32 or None beyond 32 observers): the vectorised form"""
    obs = table(observers)
    count = np.zeros(zq.shape, np.uint32)
    mask = np.zeros(zq.shape, np.uint32) if len(obs) <= 32 else None
    for i, o in enumerate(obs):
        v = visible_from(zq, o, target_q)
        count += v.astype(np.uint32)
        if mask is not None:
            mask |= v.astype(np.uint32) << np.uint32(i)
    return count, mask


def far(shape, observer):
    """bool [H, W]: the cells with n >= 2 from the observer, those a sight line has a step to"""
    rr, cc = np.mgrid[0:shape[0], 0:shape[1]]
    return np.maximum(np.abs(rr - int(observer[0])), np.abs(cc - int(observer[1]))) >= 2


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def heights(H, W, seed, cell=8):
    """float32 [H, W] in [0, 1]: value noise, bilinear between lattice values ``cell`` cells apart"""
    rng = np.random.RandomState(seed)
    g = rng.rand(H // cell + 2, W // cell + 2)
    y, x = np.arange(H) / float(cell), np.arange(W) / float(cell)
    iy, ix = y.astype(int), x.astype(int)
    fy, fx = (y - iy)[:, None], (x - ix)[None, :]
    a, b = g[iy][:, ix], g[iy][:, ix + 1]
    c, d = g[iy + 1][:, ix], g[iy + 1][:, ix + 1]
    return np.clip((a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy, 0.0, 1.0).astype(np.float32)


def stations(H, W, cut):
    """eight observers as (row, col, radius2): the four corners, one on an edge, the centre, and two more in one cell; the radii
    are none, 0, 1, 50 and ``cut``, which cuts the plane"""
    mid = (H // 2, W // 2)
    edge = (0, W // 3) if H > 1 else (0, (2 * W) // 3)
    at = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), edge, mid, (H // 3, (2 * W) // 3), (H // 3, (2 * W) // 3)]
    radii = [-1, cut, 50 * 50, -1, 1, -1, 0, cut]
    return [(r, c, r2) for (r, c), r2 in zip(at, radii)]


def _random_case(shape, seed, height_scale, eye_q, target_q):
    H, W = shape
    h = heights(H, W, seed)
    cut = (max(H, W) // 3) ** 2
    eyes = [eye_q, eye_q, 0, eye_q, eye_q, eye_q, eye_q, 3 * eye_q + 256]        # the two in one cell differ in their eyes
    obs = [(r, c, e, r2) for (r, c, r2), e in zip(stations(H, W, cut), eyes)]
    return dict(h=h, height_scale=height_scale, observers=table(obs), target_q=target_q, random=True)


def _many(shape, seed, height_scale, count):
    H, W = shape
    rng = np.random.RandomState(seed)
    obs = [(rng.randint(H), rng.randint(W), int(rng.randint(0, 4)) * 256, -1 if i % 3 else 40 * 40) for i in range(count)]
    return dict(h=heights(H, W, seed), height_scale=height_scale, observers=table(obs), target_q=64, random=True)


def _graze():
    """an equality case: a level plane, the eye two cells up, a wall one cell high 10 cells along the row: the target 20 cells
    along has the wall's top exactly on its sight line and is seen, every one behind it is hidden"""
    h = np.zeros((5, 64), np.float32)
    h[2, 13] = 1.0
    return dict(h=h, height_scale=1.0, observers=table([(2, 3, 512, -1), (2, 3, 511, -1)]), target_q=0, random=False)


def _row4096():
    """32-bit products would overflow: heights 0 and 1 in turn at height_scale 65536, zq = 0 or 2^24; the observers stand at one
    end, one with its eye 2^24 up: it sees the odd cells over the walls' tops (every step grazes or clears, 4094 steps to the far
    end, products of 2^36), the even ones lie behind a wall"""
    h = (np.arange(4096) % 2).astype(np.float32)[None, :]
    return dict(h=h, height_scale=65536.0, observers=table([(0, 0, 1 << 24, -1), (0, 0, 0, -1)]), target_q=1 << 23, random=False)


CASES = {
    "one": lambda: dict(h=np.full((1, 1), 0.5, np.float32), height_scale=64.0, observers=table([(0, 0, 0, -1), (0, 0, 512, 0)]),
                        target_q=0, random=False),
    "row": lambda: _random_case((1, 300), 11, 8.0, 512, 0),
    "column": lambda: _random_case((300, 1), 12, 8.0, 0, 0),
    "small": lambda: _random_case((33, 65), 13, 8.0, 512, 0),
    "small0": lambda: _random_case((33, 65), 14, 4.0, 0, 0),
    "wide": lambda: _random_case((97, 130), 15, 16.0, 512, 128),
    "wide0": lambda: _random_case((97, 130), 16, 6.0, 0, 0),
    "steep": lambda: _random_case((33, 65), 17, 64.0, 512, 0),
    "many32": lambda: _many((33, 65), 18, 8.0, 32),
    "many33": lambda: _many((33, 65), 19, 8.0, 33),
    "many300": lambda: _many((33, 65), 20, 8.0, 300),
    "graze": _graze,
    "row4096": _row4096,
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> the case's dict with ``zq`` added; shared, so nobody writes into it"""
    c = CASES[name]()
    c["zq"] = quantise(c["h"], c["height_scale"])
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> (count, mask or None) of a case by the vectorised form, computed once and shared"""
    c = case(name)
    count, mask = viewshed(c["zq"], c["observers"], c["target_q"])
    count.setflags(write=False)
    if mask is not None:
        mask.setflags(write=False)
    return count, mask
