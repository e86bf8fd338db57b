"""Host restatement of the pipe-model erosion (csrc/erosion.hip, gan_heightmaps_amd/erosion.py) in numpy,
parametrised by dtype: float64 is the reference the kernels are held to, float32 is the kernels' own arithmetic (every
product, sum, quotient and root rounded on its own, in the order written).  Also the seeded sine-octave terrain the tests
erode, and their parameter set P_TEST.

State of a cell: ground b (height units), water depth d, suspended sediment s, outflow fL fR fT fB towards columns j - 1,
j + 1 and rows i - 1, i + 1.  The array's edge is a closed wall."""
import numpy as np

FIELDS = ("b", "d", "s", "fL", "fR", "fT", "fB")

P_TEST = dict(dt=0.05, rain=0.02, evaporation=0.05, gravity=9.81, pipe=1.0, capacity=0.1, dissolve=0.05, deposit=0.05,
              min_tilt=0.01, max_speed=4.0, min_depth=0.05, height_scale=24.0)


def terrain(seed, H, W):
    """a seeded terrain in [0, 1], float64 [H, W]: five octaves of sines in random directions plus 2 % of white noise"""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    z = np.zeros((H, W))
    for o in range(5):
        th, ph = rng.uniform(0, 2 * np.pi, 2)
        lam = 48.0 / 2 ** o
        z += 0.5 ** o * np.sin(2 * np.pi * (np.cos(th) * y + np.sin(th) * x) / lam + ph)
    z = 0.5 + 0.4 * z / 1.9375                      # the octaves' amplitudes sum to 1.9375
    z += 0.02 * rng.uniform(-1, 1, (H, W))
    return np.clip(z, 0.0, 1.0)


def init_state(heightmap, p, dtype):
    """heightmap [H, W] in [0, 1] -> the state: b = heightmap * height_scale, everything else 0"""
    T = np.dtype(dtype).type
    hm = np.asarray(heightmap).astype(dtype)
    st = {k: np.zeros(hm.shape, dtype) for k in FIELDS}
    st["b"] = hm * T(p["height_scale"])
    return st


def _shift(a, dy, dx):
    """out[i, j] = a[i + dy, j + dx], 0 where that lies outside the array"""
    H, W = a.shape
    out = np.zeros_like(a)
    i0, i1 = max(0, -dy), H - max(0, dy)
    j0, j1 = max(0, -dx), W - max(0, dx)
    if i1 > i0 and j1 > j0:
        out[i0:i1, j0:j1] = a[i0 + dy:i1 + dy, j0 + dx:j1 + dx]
    return out


def _clamped(a, dy, dx):
    """out[i, j] = a[clamp(i + dy), clamp(j + dx)]"""
    H, W = a.shape
    ii = np.clip(np.arange(H) + dy, 0, H - 1)
    jj = np.clip(np.arange(W) + dx, 0, W - 1)
    return a[np.ix_(ii, jj)]


def _backtrace(vel, dt, idx, n):
    """one axis of step 5: (first corner, second corner, weight) of the backtraced position idx - clamp(vel dt, +-1),
    clamped to [0, n - 1].  The weight is formed from the displacement alone, never from the absolute index, so that it
    does not depend on where the window's origin lies (for idx < 2^24 the index arithmetic itself is exact)."""
    T = vel.dtype.type
    o = -np.clip(vel * dt, T(-1), T(1))
    o = np.where((idx == 0) & (o < 0), T(0), o)
    o = np.where((idx == n - 1) & (o > 0), T(0), o)
    neg = o < 0
    x0 = np.where(neg, idx - 1, idx)
    t = np.where(neg, o + T(1), o).astype(vel.dtype)
    return np.clip(x0, 0, n - 1), np.clip(x0 + 1, 0, n - 1), t


def step(st, p, dtype):
    """one iteration: a new state dict; ``st`` is left as it was"""
    T = np.dtype(dtype).type
    dt, rain, evap, grav, pipe = (T(p[k]) for k in ("dt", "rain", "evaporation", "gravity", "pipe"))
    Kc, Ks, Kd = (T(p[k]) for k in ("capacity", "dissolve", "deposit"))
    min_tilt, max_speed, min_depth = (T(p[k]) for k in ("min_tilt", "max_speed", "min_depth"))
    half, one, zero = T(0.5), T(1), T(0)
    b, d, s = st["b"], st["d"], st["s"]
    H, W = b.shape
    ii, jj = np.mgrid[0:H, 0:W]
    # 1. rain
    d1 = d + dt * rain
    # 2. flux
    h = b + d1
    k = (dt * pipe) * grav
    g = {}
    for name, dy, dx, has in (("fL", 0, -1, jj > 0), ("fR", 0, 1, jj < W - 1), ("fT", -1, 0, ii > 0),
                              ("fB", 1, 0, ii < H - 1)):
        g[name] = np.where(has, np.maximum(zero, st[name] + k * (h - _shift(h, dy, dx))), zero).astype(dtype)
    S = ((g["fL"] + g["fR"]) + (g["fT"] + g["fB"])) * dt
    with np.errstate(divide="ignore", invalid="ignore"):
        K = np.where(S > d1, d1 / S, one).astype(dtype)
    f = {name: K * g[name] for name in g}
    # 3. water and velocity
    inL, inR = _shift(f["fR"], 0, -1), _shift(f["fL"], 0, 1)
    inT, inB = _shift(f["fB"], -1, 0), _shift(f["fT"], 1, 0)
    inflow = (inL + inR) + (inT + inB)
    outflow = (f["fL"] + f["fR"]) + (f["fT"] + f["fB"])
    d2 = np.maximum(zero, d1 + dt * (inflow - outflow))
    wx = half * ((inL - f["fL"]) + (f["fR"] - inR))
    wy = half * ((inT - f["fT"]) + (f["fB"] - inB))
    dbar = np.maximum(half * (d1 + d2), min_depth)
    u = np.clip(wx / dbar, -max_speed, max_speed)
    v = np.clip(wy / dbar, -max_speed, max_speed)
    # 4. erosion and deposition
    gx = half * (_clamped(b, 0, 1) - _clamped(b, 0, -1))
    gy = half * (_clamped(b, 1, 0) - _clamped(b, -1, 0))
    g2 = gx * gx + gy * gy
    tilt = np.maximum(np.sqrt(g2 / (one + g2)), min_tilt)
    C = (Kc * tilt) * np.sqrt(u * u + v * v)
    D = C - s
    e = np.where(D > 0, Ks * D, Kd * D).astype(dtype)
    b2 = b - e
    s1 = s + e
    # 5. transport
    x0, x1, tx = _backtrace(u, dt, jj, W)
    y0, y1, ty = _backtrace(v, dt, ii, H)
    top = s1[y0, x0] + tx * (s1[y0, x1] - s1[y0, x0])
    bot = s1[y1, x0] + tx * (s1[y1, x1] - s1[y1, x0])
    s2 = top + ty * (bot - top)
    # 6. evaporation
    d3 = d2 * (one - evap * dt)
    out = dict(f, b=b2, d=d3, s=s2)
    assert all(out[k_].dtype == np.dtype(dtype) for k_ in FIELDS), {k_: out[k_].dtype for k_ in FIELDS}
    return out


def erode_state(heightmap, p, iterations, dtype, state=None):
    """the state after ``iterations`` steps from ``heightmap`` (or from ``state``)"""
    st = init_state(heightmap, p, dtype) if state is None else state
    for _ in range(iterations):
        st = step(st, p, dtype)
    return st


def emit(st, p, dtype=None):
    """the output heightmap: clamp(b / height_scale, 0, 1)"""
    b = st["b"]
    return np.clip(b / b.dtype.type(p["height_scale"]), 0, 1)


def erode(heightmap, p, iterations, dtype):
    return emit(erode_state(heightmap, p, iterations, dtype), p)
