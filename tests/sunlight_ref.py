"""The sunlight's definition (include/ghm.h, section "sunlight") restated in plain Python integers and in numpy int64,
on its own: nothing here imports the package.  Two forms -- ``sunlight_loop``, a double loop over cells and steps in Python
integers, and ``sunlight``, vectorised over the cells per step -- and ``lit_accel``, the block-maximum jumps restated ray by ray;
then the case generators the host build's and the device's tests share.  ``expected(name)`` computes a case's answer once.

    a position = (rows, gmaj, gmin, m_q, rise_q, s_y, s_x, s_z, w_q), built in float64 and rounded once per entry (``position``)
    g_y = zq[r + 1, c] - zq[r - 1, c], g_x likewise, indices clamped; norm = floor(sqrt(g_y^2 + g_x^2 + 512^2))
    dot = -g_y s_y - g_x s_x + 512 s_z; a cell with dot <= 0 shades itself; otherwise, for k = 1, 2, ...:
    ray = 256 (zq[T] + target_q) + k rise_q; q, f = divmod(k m_q, 65536); a = T + k major steps + q minor steps, b = a + one minor step
    lit at the first k whose a (or b, if f > 0) lies outside the plane; in shadow at the first k with
    zq[a] (65536 - f) + zq[b] f > 256 ray.  lit, mask, hours_q = sum w_q, energy = sum (w_q dot) // norm over the positions that light.

The restatement marches every ray to the plane's edge: the device's early exit (ray >= 256 zmax) is an option here, ``early=True``,
so that tests can show that it changes nothing.  (int64 holds 256 ray up to planes 4096 cells long at rise_q = 2^40.)
"""
import functools
import math

import numpy as np

from tests import viewshed_ref as V

BLOCK = V.BLOCK              # GHM_VIEWSHED_BLOCK
FIELDS = 9                   # GHM_SUNLIGHT_FIELDS
CHUNK = 64                   # GHM_SUNLIGHT_CHUNK
MAX_POSITIONS = 4096         # GHM_SUNLIGHT_MAX_POSITIONS
MAX_WEIGHT = 1 << 17         # GHM_SUNLIGHT_MAX_WEIGHT
ONE = 65536
MAX_RISE = 1 << 40

quantise = V.quantise
top = V.top


def _rint(v):
    return int(np.rint(v))


def position(azimuth_deg, elevation_deg, hours=1.0):
    """one row of the host table.  The direction to the sun is (dy, dx, dz) = (cos el cos az, cos el sin az, sin el), y down the
    rows; the ray's major axis is the larger of |cos az| and |sin az| (the rows on a tie)"""
    az, el = math.radians(float(azimuth_deg)), math.radians(float(elevation_deg))
    hy, hx = math.cos(az), math.sin(az)
    rows = abs(hy) >= abs(hx)
    major, minor = (hy, hx) if rows else (hx, hy)
    m_q = _rint(ONE * abs(minor) / abs(major))
    rise_q = int(min(max(np.rint(ONE * math.tan(el) / abs(major)), 1.0), float(MAX_RISE)))
    gmaj = 1 if major > 0 else -1
    gmin = 0 if m_q == 0 else (1 if minor > 0 else -1)
    c = math.cos(el)
    return (int(rows), gmaj, gmin, m_q, rise_q, _rint(16384 * c * hy), _rint(16384 * c * hx), _rint(16384 * math.sin(el)),
            _rint(256 * float(hours)))


def table(positions):
    """int64 [n, 9] from (azimuth, elevation[, hours]) tuples"""
    return np.array([position(*p) for p in positions], np.int64).reshape(-1, FIELDS)


def reach(tab, height_scale):
    """ceil(256 rint(256 height_scale) / min rise_q) + 1"""
    rise = int(np.asarray(tab)[:, 4].min())
    return -(-256 * _rint(256.0 * float(height_scale)) // rise) + 1


def slope(zq):
    """-> (g_y, g_x, norm), int64 [H, W]"""
    z = np.asarray(zq).astype(np.int64)
    H, W = z.shape
    r, c = np.arange(H), np.arange(W)
    gy = z[np.minimum(r + 1, H - 1)] - z[np.maximum(r - 1, 0)]
    gx = z[:, np.minimum(c + 1, W - 1)] - z[:, np.maximum(c - 1, 0)]
    s = gy * gy + gx * gx + 512 * 512
    n = np.floor(np.sqrt(s.astype(np.float64))).astype(np.int64)
    n = np.where(n * n > s, n - 1, n)
    n = np.where((n + 1) * (n + 1) <= s, n + 1, n)
    assert ((n * n <= s) & ((n + 1) * (n + 1) > s)).all()
    return gy, gx, n


# ---- one ray, in Python integers -------------------------------------------------------------------------------------------------
def _cells(pos, r, c, k, q):
    rows, gmaj, gmin = pos[0], pos[1], pos[2]
    if rows:
        return (r + gmaj * k, c + gmin * q), (r + gmaj * k, c + gmin * (q + 1))
    return (r + gmin * q, c + gmaj * k), (r + gmin * (q + 1), c + gmaj * k)


def lit_ray(zq, pos, target_q, r, c):
    """whether the ray of cell (r, c) under ``pos`` ends lit: the definition, step by step"""
    H, W = zq.shape
    pos = [int(v) for v in pos]
    m, rise = pos[3], pos[4]
    base = 256 * (int(zq[r, c]) + int(target_q))
    k = 0
    while True:
        k += 1
        q, f = divmod(k * m, ONE)
        (ar, ac), (br, bc) = _cells(pos, r, c, k, q)
        if not (0 <= ar < H and 0 <= ac < W) or (f and not (0 <= br < H and 0 <= bc < W)):
            return True
        za = int(zq[ar, ac])
        zb = int(zq[br, bc]) if f else za
        if za * (ONE - f) + zb * f > 256 * (base + k * rise):
            return False


def lit_accel(zq, tops, pos, target_q, r, c):
    """-> (lit, steps tested): the ray in runs inside one block of the major axis, a run jumped when the block maxima prove it
    clear, marched by the definition's own test otherwise; with the early exit.  csrc/sunlight.hip's accel form, ray by ray"""
    H, W = zq.shape
    pos = [int(v) for v in pos]
    rows, gmaj, gmin, m, rise = pos[:5]
    nmaj, nmin = (H, W) if rows else (W, H)
    tmaj, tmin = (r, c) if rows else (c, r)
    base = 256 * (int(zq[r, c]) + int(target_q))
    stop = 256 * int(zq.max())
    k = steps = 0
    while True:
        k += 1
        q, f = divmod(k * m, ONE)
        cmaj, cmin, ray = tmaj + gmaj * k, tmin + gmin * q, base + k * rise
        if not (0 <= cmaj < nmaj and 0 <= cmin < nmin) or ray >= stop:
            return True, steps
        inblock = BLOCK - 1 - cmaj % BLOCK if gmaj > 0 else cmaj % BLOCK
        inplane = nmaj - 1 - cmaj if gmaj > 0 else cmaj
        k1 = k + min(inblock, inplane)
        q1, f1 = divmod(k1 * m, ONE)
        e1 = tmin + gmin * (q1 + (f1 > 0))
        if 0 <= e1 < nmin:
            lo, hi = min(cmin, e1) // BLOCK, max(cmin, e1) // BLOCK
            assert hi - lo <= 2
            bm = cmaj // BLOCK
            M = max(int(tops[bm, b] if rows else tops[b, bm]) for b in range(lo, hi + 1))
            if M * ONE <= 256 * ray:
                k = k1
                continue
        while True:
            q, f = divmod(k * m, ONE)
            (ar, ac), (br, bc) = _cells(pos, r, c, k, q)
            if not (0 <= ar < H and 0 <= ac < W) or (f and not (0 <= br < H and 0 <= bc < W)) or base + k * rise >= stop:
                return True, steps
            steps += 1
            za = int(zq[ar, ac])
            zb = int(zq[br, bc]) if f else za
            if za * (ONE - f) + zb * f > 256 * (base + k * rise):
                return False, steps
            if k == k1:
                break
            k += 1


def sunlight_loop(zq, tab, target_q):
    """-> dict(lit, mask or None beyond 32 positions, hours_q, energy), uint32: the plain double loop in Python integers"""
    H, W = zq.shape
    tab = [[int(v) for v in p] for p in np.asarray(tab)]
    out = {k: np.zeros((H, W), np.uint32) for k in ("lit", "mask", "hours_q", "energy")}
    for r in range(H):
        for c in range(W):
            gy = int(zq[min(r + 1, H - 1), c]) - int(zq[max(r - 1, 0), c])
            gx = int(zq[r, min(c + 1, W - 1)]) - int(zq[r, max(c - 1, 0)])
            norm = math.isqrt(gy * gy + gx * gx + 512 * 512)
            lit = mask = hours = energy = 0
            for i, p in enumerate(tab):
                dot = -gy * p[5] - gx * p[6] + 512 * p[7]
                if dot <= 0 or not lit_ray(zq, p, target_q, r, c):
                    continue
                lit += 1
                mask |= 1 << (i & 31)
                hours += p[8]
                energy += (p[8] * dot) // norm
            out["lit"][r, c], out["mask"][r, c], out["hours_q"][r, c], out["energy"][r, c] = lit, mask, hours, energy
    if len(tab) > 32:
        out["mask"] = None
    return out


# ---- every cell at once, step by step --------------------------------------------------------------------------------------------
def lit_plane(zq, pos, target_q, active, early=False):
    """-> (bool [H, W]: the cells of ``active`` whose ray under ``pos`` ends lit, int64 [H, W]: the steps tested).  early: with the
    device's early exit, ray >= 256 zmax"""
    z = np.asarray(zq).astype(np.int64)
    H, W = z.shape
    rows, gmaj, gmin, m, rise = (int(v) for v in pos[:5])
    idx = np.flatnonzero(np.asarray(active).ravel())
    r0, c0 = idx // W, idx % W
    base = 256 * (z.ravel()[idx] + int(target_q))
    stop = 256 * int(z.max())
    lit, steps = np.zeros(H * W, bool), np.zeros(H * W, np.int64)
    alive = np.arange(idx.size)
    k = 0
    while alive.size:
        k += 1
        q, f = divmod(k * m, ONE)
        ray = base[alive] + k * rise
        if rows:
            ar, ac = r0[alive] + gmaj * k, c0[alive] + gmin * q
            br, bc = ar, ac + gmin
        else:
            ar, ac = r0[alive] + gmin * q, c0[alive] + gmaj * k
            br, bc = ar + gmin, ac
        out = (ar < 0) | (ar >= H) | (ac < 0) | (ac >= W)
        if f:
            out |= (br < 0) | (br >= H) | (bc < 0) | (bc >= W)
        if early:
            out |= ray >= stop
        lit[idx[alive[out]]] = True
        keep = ~out
        alive, ray, ar, ac, br, bc = alive[keep], ray[keep], ar[keep], ac[keep], br[keep], bc[keep]
        steps[idx[alive]] += 1
        za = z[ar, ac]
        zb = z[br, bc] if f else za
        alive = alive[~(za * (ONE - f) + zb * f > 256 * ray)]
    return lit.reshape(H, W), steps.reshape(H, W)


def sunlight(zq, tab, target_q, early=False):
    """-> dict(lit, mask or None beyond 32 positions, hours_q, energy: uint32; steps: int64): the vectorised form"""
    tab = np.asarray(tab, np.int64).reshape(-1, FIELDS)
    gy, gx, norm = slope(zq)
    shape = np.asarray(zq).shape
    lit, mask, hours, energy = (np.zeros(shape, np.int64) for _ in range(4))
    steps = np.zeros(shape, np.int64)
    for i, p in enumerate(tab):
        dot = -gy * int(p[5]) - gx * int(p[6]) + 512 * int(p[7])
        on, tested = lit_plane(zq, p, target_q, dot > 0, early)
        steps += tested
        lit += on
        mask |= on.astype(np.int64) << (i & 31)
        hours += on * int(p[8])
        energy += on * ((int(p[8]) * np.maximum(dot, 0)) // norm)
    assert energy.max() < 1 << 32
    out = dict(lit=lit.astype(np.uint32), mask=mask.astype(np.uint32) if len(tab) <= 32 else None, hours_q=hours.astype(np.uint32),
               energy=energy.astype(np.uint32), steps=steps)
    return out


PLANES = ("lit", "mask", "hours_q", "energy")


def same_planes(a, b):
    for k in PLANES:
        if (a[k] is None) != (b[k] is None) or (a[k] is not None and not (a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]))):
            return False
    return True


# ---- the cases ------------------------------------------------------------------------------------------------------------------
# the suns of the prototype, the eight axis and diagonal azimuths (m_q = 0 and m_q = 65536), an elevation of 90 degrees and one so
# low that rise_q clamps to 1; the hours differ so that hours_q and energy tell the positions apart
SUNS = ((0, 10), (90, 10), (225, 28), (200, 5), (33, 2), (290, 45), (135, 1), (77, 80))
AXES = tuple((45 * i, 20) for i in range(8))
ALL_SUNS = tuple((az, el, (0.5, 1.0, 2.25)[i % 3]) for i, (az, el) in enumerate(SUNS + AXES + ((123, 90), (10, 1e-7))))


def _noise(shape, seed, height_scale, target_q=0):
    return dict(h=V.heights(shape[0], shape[1], seed), height_scale=height_scale, table=table(ALL_SUNS), target_q=target_q)


def _many(count, seed):
    rng = np.random.RandomState(seed)
    suns = [(float(rng.uniform(0, 360)), float(rng.uniform(1, 60)), float(rng.randint(1, 5)) / 4) for _ in range(count)]
    return dict(h=V.heights(33, 65, seed), height_scale=8.0, table=table(suns), target_q=0)


WALL_AT, WALL_STEPS = 40, 16


def _wall():
    """the equality case: a level plane at 0, the sun due +x at tan(el) = 1/16, so rise_q = 4096; in row 1 a wall of zq = 256 and
    in row 3 one of zq = 257, both in column 40.  The ray of the cell 16 steps before the wall stands at 16 * 4096 = 65536 = 256 * 256
    there, exactly the lower wall's top: it grazes, and is lit; one unit of zq more on the wall shades it"""
    h = np.zeros((5, 64), np.float32)
    h[1, WALL_AT] = np.float32(256.0 / 257.0)
    h[3, WALL_AT] = 1.0
    el = math.degrees(math.atan(1.0 / WALL_STEPS))
    return dict(h=h, height_scale=257.0 / 256.0, table=table([(90, el), (90, 2 * el, 0.5), (270, el)]), target_q=0)


def _row4096():
    """32-bit products would overflow: heights 0 and 1 in turn at height_scale 65536, zq = 0 or 2^24, samples of 2^40 against
    256 ray up to 2^60 in the restatement, which marches the lit rays of the high cells to the row's end"""
    h = (np.arange(4096) % 2).astype(np.float32)[None, :]
    return dict(h=h, height_scale=65536.0, table=table([(90, 87.4), (270, 1e-7, 2.0), (90, 90, 0.25), (100, 89.0)]), target_q=1 << 16)


CASES = {
    "1x1": lambda: _noise((1, 1), 21, 8.0),
    "1x9": lambda: _noise((1, 9), 22, 8.0),
    "9x1": lambda: _noise((9, 1), 23, 8.0),
    "15x17": lambda: _noise((15, 17), 24, 8.0),
    "17x33": lambda: _noise((17, 33), 25, 8.0, 64),
    "33x65": lambda: _noise((33, 65), 26, 8.0),
    "37x70": lambda: _noise((37, 70), 27, 16.0),
    "70x37": lambda: _noise((70, 37), 28, 16.0, 128),
    "65x130": lambda: _noise((65, 130), 29, 32.0),
    "wall": _wall,
    "row4096": _row4096,
    "many33": lambda: _many(33, 31),
    "many300": lambda: _many(300, 32),
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
    """-> the planes of a case by the vectorised form, every ray marched to the plane's edge; computed once and shared"""
    c = case(name)
    out = sunlight(c["zq"], c["table"], c["target_q"])
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected_early(name):
    """-> the planes of a case with the device's early exit, and ``steps``, what the plain device form tests"""
    c = case(name)
    out = sunlight(c["zq"], c["table"], c["target_q"], early=True)
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    return out


def expected_steps(name):
    """-> int64 [H, W]: the steps the plain device form tests"""
    return expected_early(name)["steps"]
