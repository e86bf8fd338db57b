"""Sequential restatements of gan_heightmaps_amd/hydrology.py in numpy and plain Python, and the seeded planes
the hydrology tests share.

The kernels relax; these do not.  ``fill`` is a heap priority-flood seeded with the outlets, ``flats`` a queue BFS from the
draining cells, ``directions`` the rule as the module states it, ``accumulate`` one pass over the cells in decreasing (F, D),
``basins`` one pass in increasing (F, D).  ``relax_fill``, ``relax_flats`` and ``doubling`` restate what the kernels run (Jacobi
sweeps and pointer doubling) in numpy, to hold the two kinds against each other on the CPU and to count sweeps and rounds.
"""
import collections
import heapq

import numpy as np

OFFSETS = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))      # k = 0 .. 7: N NE E SE S SW W NW
DIAGONAL = np.float32(0.70710678)
WEIGHTS = tuple(np.float32(1) if dy == 0 or dx == 0 else DIAGONAL for dy, dx in OFFSETS)
SENTINEL = np.int32(0x3fffffff)

# (H, W, q, seed): value-noise planes, unquantised (q None) or in q levels
CASES = ((96, 80, None, 11), (96, 80, 32, 12), (64, 130, 8, 13), (33, 47, 255, 14))


def terrain(H, W, q=None, seed=0, octaves=5):
    """five octaves of bilinearly interpolated value noise, normalised to [0, 1], float32; q: quantised to q levels"""
    rs = np.random.RandomState(seed)
    t = np.zeros((H, W), np.float64)
    for o in range(octaves):
        n = 2 << o
        g = rs.rand(n + 1, n + 1)
        y = np.arange(H, dtype=np.float64) * n / H
        x = np.arange(W, dtype=np.float64) * n / W
        iy, ix = np.floor(y).astype(int), np.floor(x).astype(int)
        fy, fx = (y - iy)[:, None], (x - ix)[None, :]
        a, b = g[iy][:, ix], g[iy][:, ix + 1]
        c, e = g[iy + 1][:, ix], g[iy + 1][:, ix + 1]
        t += ((a + fx * (b - a)) * (1 - fy) + (c + fx * (e - c)) * fy) * 0.5 ** o
    span = t.max() - t.min()
    t = (t - t.min()) / (span if span > 0 else 1.0)
    if q is not None:
        t = np.rint(t * (q - 1)) / (q - 1)
    return np.ascontiguousarray(t, np.float32)


def canonical(h):
    """float32, -0 as +0 (what the kernels read)"""
    return np.ascontiguousarray(h, np.float32) + np.float32(0)


def is_outlet(H, W):
    m = np.zeros((H, W), bool)
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = True
    return m


def fill(h):
    """priority-flood: F[c] = the least, over the paths from c to an outlet, of the largest h on the path"""
    h = canonical(h)
    H, W = h.shape
    F = np.full((H, W), np.inf, np.float32)
    done = np.zeros((H, W), bool)
    heap = []
    for i, j in zip(*np.nonzero(is_outlet(H, W))):
        F[i, j] = h[i, j]
        done[i, j] = True
        heap.append((float(h[i, j]), int(i), int(j)))
    heapq.heapify(heap)
    while heap:
        v, i, j = heapq.heappop(heap)
        for dy, dx in OFFSETS:
            y, x = i + dy, j + dx
            if 0 <= y < H and 0 <= x < W and not done[y, x]:
                done[y, x] = True
                F[y, x] = max(float(h[y, x]), v)
                heapq.heappush(heap, (float(F[y, x]), y, x))
    return F


def draining(F):
    """outlets, and cells with a strictly lower neighbour"""
    H, W = F.shape
    m = is_outlet(H, W)
    P = np.pad(F, 1, constant_values=np.inf)
    for dy, dx in OFFSETS:
        m = m | (P[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] < F)
    return m


def flats(F):
    """BFS from the draining cells over neighbours of equal F"""
    H, W = F.shape
    D = np.full((H, W), SENTINEL, np.int32)
    queue = collections.deque()
    for i, j in zip(*np.nonzero(draining(F))):
        D[i, j] = 0
        queue.append((int(i), int(j)))
    while queue:
        i, j = queue.popleft()
        for dy, dx in OFFSETS:
            y, x = i + dy, j + dx
            if 0 <= y < H and 0 <= x < W and D[y, x] == SENTINEL and F[y, x] == F[i, j]:
                D[y, x] = D[i, j] + 1
                queue.append((y, x))
    return D


def directions(F, D):
    H, W = F.shape
    out = np.full((H, W), -1, np.int8)
    for i in range(1, H - 1):
        for j in range(1, W - 1):
            best, bk = np.float32(0), -1
            for k, (dy, dx) in enumerate(OFFSETS):
                f = F[i + dy, j + dx]
                if f < F[i, j]:
                    s = np.float32(np.float32(F[i, j] - f) * WEIGHTS[k])
                    if bk < 0 or s > best:
                        best, bk = s, k
            if bk < 0:
                for k, (dy, dx) in enumerate(OFFSETS):
                    if F[i + dy, j + dx] == F[i, j] and D[i + dy, j + dx] == D[i, j] - 1:
                        bk = k
                        break
            out[i, j] = bk
    return out


def receivers(direction):
    """flat index of the receiver, -1 for an outlet"""
    H, W = direction.shape
    dy = np.array([o[0] for o in OFFSETS] + [0])[direction]
    dx = np.array([o[1] for o in OFFSETS] + [0])[direction]
    i, j = np.mgrid[0:H, 0:W]
    return np.where(direction >= 0, (i + dy) * W + (j + dx), -1).astype(np.int64)


def _order(F, D):
    """flat indices in increasing (F, D)"""
    return np.lexsort((D.ravel(), F.ravel()))


def accumulate(F, D, direction):
    r = receivers(direction).ravel()
    A = np.ones(F.size, np.int64)
    for c in _order(F, D)[::-1]:
        if r[c] >= 0:
            A[r[c]] += A[c]
    return A.reshape(F.shape).astype(np.uint32)


def basins(F, D, direction):
    r = receivers(direction).ravel()
    B = np.arange(F.size, dtype=np.int64)
    for c in _order(F, D):
        if r[c] >= 0:
            B[c] = B[r[c]]
    return B.reshape(F.shape).astype(np.int32)


Result = collections.namedtuple("Result", "filled depth flat direction accumulation basin")


def analyse(h):
    h = canonical(h)
    F = fill(h)
    D = flats(F)
    d = directions(F, D)
    return Result(F, F - h, D, d, accumulate(F, D, d), basins(F, D, d))


# ---- what the kernels run, in numpy ------------------------------------------------------------------------------------------
def _neighbour_min(P, H, W):
    m = None
    for dy, dx in OFFSETS:
        v = P[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
        m = v if m is None else np.minimum(m, v)
    return m


def relax_fill(h):
    """Jacobi sweeps from +inf -> (F, sweeps): the sweeps run until one changes nothing, that one included"""
    h = canonical(h)
    H, W = h.shape
    out = is_outlet(H, W)
    F = np.where(out, h, np.float32(np.inf)).astype(np.float32)
    sweeps = 0
    while True:
        m = _neighbour_min(np.pad(F, 1, constant_values=np.inf), H, W)
        G = np.where(out, h, np.maximum(h, m)).astype(np.float32)
        sweeps += 1
        if np.array_equal(G, F):
            return F, sweeps
        F = G


def relax_flats(F):
    H, W = F.shape
    drain = draining(F)
    D = np.where(drain, 0, SENTINEL).astype(np.int32)
    PF = np.pad(F, 1, constant_values=np.nan)
    sweeps = 0
    while True:
        PD = np.pad(D, 1, constant_values=SENTINEL)
        m = np.full((H, W), SENTINEL, np.int32)
        for dy, dx in OFFSETS:
            same = PF[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] == F
            m = np.where(same, np.minimum(m, PD[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]), m)
        G = np.where(drain, 0, np.minimum(SENTINEL, m + 1)).astype(np.int32)
        sweeps += 1
        if np.array_equal(G, D):
            return D, sweeps
        D = G


def doubling(direction):
    """pointer doubling -> (A, basin, rounds)"""
    P = receivers(direction).ravel()
    n = P.size
    S = np.ones(n, np.int64)
    B = np.where(P >= 0, P, np.arange(n))
    rounds = 0
    while (P >= 0).any():
        live = P >= 0
        T = S.copy()
        np.add.at(T, P[live], S[live])
        Q = np.full(n, -1, np.int64)
        Q[live] = P[P[live]]
        S, P, B = T, Q, B[B]
        rounds += 1
    return S.reshape(direction.shape).astype(np.uint32), B.reshape(direction.shape).astype(np.int32), rounds


def largest_plateau(F, D):
    """cells of the largest connected set of non-draining cells of one F"""
    H, W = F.shape
    seen = D == 0
    best = 0
    for i0, j0 in zip(*np.nonzero(~seen)):
        if seen[i0, j0]:
            continue
        seen[i0, j0] = True
        stack, n = [(int(i0), int(j0))], 0
        while stack:
            i, j = stack.pop()
            n += 1
            for dy, dx in OFFSETS:
                y, x = i + dy, j + dx
                if 0 <= y < H and 0 <= x < W and not seen[y, x] and F[y, x] == F[i, j]:
                    seen[y, x] = True
                    stack.append((y, x))
        best = max(best, n)
    return best


def wet_mask(depth, A, river_threshold, river_width, lake_min_depth):
    H, W = depth.shape
    r = int(river_width)
    P = np.pad(A, r, mode="edge")
    m = np.zeros((H, W), A.dtype)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            m = np.maximum(m, P[dy:dy + H, dx:dx + W])
    return (depth > np.float32(lake_min_depth)) | (m >= river_threshold)


def paint_planes(planes, wet, colour, opacity):
    """float32 [C, H, W] planes and a colour per channel in the planes' value range -> painted planes"""
    out = planes.copy()
    op = np.float32(opacity)
    for c in range(planes.shape[0]):
        t = planes[c]
        v = (t + (op * (np.float32(colour[c]) - t)).astype(np.float32)).astype(np.float32)
        out[c] = np.where(wet, v, t)
    return out


# ---- hand-made planes --------------------------------------------------------------------------------------------------------
def serpentine(H=31, W=41):
    """walls of height 1 with a channel of height 0.25 that winds from a pit in one corner to a notch in the far edge: the
    lake's level has to travel the length of the channel, many times the plane's side"""
    h = np.ones((H, W), np.float32)
    rows = list(range(2, H - 2, 2))
    for n, i in enumerate(rows):
        h[i, 2:W - 2] = 0.25
        if n + 1 < len(rows):
            j = W - 3 if n % 2 == 0 else 2
            h[i + 1, j] = 0.25
    h[2, 2] = 0.0                                    # the pit at the channel's head
    last = rows[-1]
    if (len(rows) - 2) % 2 == 0:                     # the last row was entered at the right: it leaves at the left
        h[last, 0:2] = 0.25
        h[last, 0] = 0.125                           # the outlet cell, below the channel
    else:
        h[last, W - 2:W] = 0.25
        h[last, W - 1] = 0.125
    return h


def corner_pits(tile, tiles=2):
    """a gentle cone with one 2 x 2 pit on every corner where four tiles meet"""
    n = tile * tiles + 2
    i, j = np.mgrid[0:n, 0:n].astype(np.float32)
    c = np.float32(n - 1) / 2
    h = (np.float32(1) - (np.abs(i - c) + np.abs(j - c)) / np.float32(2 * n)).astype(np.float32)
    for a in range(1, tiles + 1):
        for b in range(1, tiles + 1):
            y, x = a * tile, b * tile
            if y + 1 < n - 1 and x + 1 < n - 1:
                h[y - 1:y + 1, x - 1:x + 1] = np.float32(0.01)
    return h
