"""Sequential restatements of gan_heightmaps_amd/route.py in numpy, heapq and plain Python, and the planes the route
tests share.

The definition, restated.  The plane is h[H, W], float32, read as h + 0.  Neighbours k = 0 .. 7 are N NE E SE S SW W NW.  Every
float32 operation is rounded on its own.
1. P[c] = ((penalty[c] lake_c) ford_c): penalty >= 1 or +inf (default 1); lake_c = travel.lake where a depth plane is given and
   depth[c] > travel.lake_min_depth, ford_c = travel.ford where an accumulation plane is given and accumulation[c] >=
   travel.river_threshold, otherwise 1.
2. Between a and its neighbour b in direction k, z = height_scale h: g = |z_a - z_b| R_k (R_k = 1 or float32(0.70710678)),
   s = g inv_grade (inv_grade = float32(1 / travel.grade)), f = 1 + s s, m = 0.5 (P_a + P_b), w = (L_k m) f (L_k = 1 or
   float32(1.41421356)); q_k(a) = 0 (no edge) if w is not finite, else max(1, rint(min(w UNIT, MAX_WEIGHT))), a uint32.
3. cost (uint32, units of 1 / UNIT): 0 at the sources, elsewhere the least over the present edges to reached neighbours of
   cost[n_k] + q_k(c), formed without wrapping and accepted only below UNREACHED.
4. parent (int8): -1 at a source, NO_PARENT at an unreached cell, elsewhere the lowest k with a present edge, a reached
   neighbour and cost[n_k] + q_k(c) == cost[c].

The kernels relax; ``dijkstra`` does not: it is a heap on Python integers.  ``jacobi`` restates what the plain form runs, to hold
the two against each other on the CPU and to count sweeps.  ``territory_traffic`` is one ordered pass over the cells by cost.
"""
import collections
import heapq

import numpy as np

from tests.hydrology_ref import OFFSETS, canonical, terrain, CASES as TERRAINS      # noqa: F401

UNIT = 64
MAX_WEIGHT = 1 << 24
UNREACHED = 0xFFFFFFFF
NO_PARENT = -2
DIAGONAL = np.float32(0.70710678)
ROOT2 = np.float32(1.41421356)
GROUP_PLAIN = 8                                    # sweeps the host issues per read of the device word, plain form

Travel = collections.namedtuple("Travel", "grade lake ford river_threshold lake_min_depth height_scale")
TRAVEL = Travel(0.15, 16.0, 4.0, 256, 1.0 / 512, 64.0)


def cell_penalty(shape, travel=TRAVEL, penalty=None, depth=None, accumulation=None):
    P = np.ones(shape, np.float32) if penalty is None else np.ascontiguousarray(penalty, np.float32)
    lake = np.ones(shape, np.float32)
    if depth is not None:
        lake = np.where(np.asarray(depth, np.float32) > np.float32(travel.lake_min_depth), np.float32(travel.lake), np.float32(1))
    ford = np.ones(shape, np.float32)
    if accumulation is not None:
        ford = np.where(np.asarray(accumulation) >= travel.river_threshold, np.float32(travel.ford), np.float32(1))
    return ((P * lake.astype(np.float32)).astype(np.float32) * ford.astype(np.float32)).astype(np.float32)


def weights(h, travel=TRAVEL, penalty=None, depth=None, accumulation=None):
    """-> q[8, H, W] uint32: q[k, i, j] is the weight of the edge between (i, j) and its neighbour k, 0 where there is none.
    Every direction is computed on its own, from the cell's side: nothing here assumes the symmetry"""
    h = canonical(h)
    H, W = h.shape
    z = (np.float32(travel.height_scale) * h).astype(np.float32)
    P = cell_penalty((H, W), travel, penalty, depth, accumulation)
    inv = np.float32(1.0 / travel.grade)
    q = np.zeros((8, H, W), np.uint32)
    with np.errstate(over="ignore", invalid="ignore"):
        for k, (dy, dx) in enumerate(OFFSETS):
            ya, xa = slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx))
            yb, xb = slice(max(0, dy), H + min(0, dy)), slice(max(0, dx), W + min(0, dx))
            diag = dy != 0 and dx != 0
            g = (np.abs((z[ya, xa] - z[yb, xb]).astype(np.float32)) * (DIAGONAL if diag else np.float32(1))).astype(np.float32)
            s = (g * inv).astype(np.float32)
            f = (np.float32(1) + (s * s).astype(np.float32)).astype(np.float32)
            m = (np.float32(0.5) * (P[ya, xa] + P[yb, xb]).astype(np.float32)).astype(np.float32)
            w = (((ROOT2 if diag else np.float32(1)) * m).astype(np.float32) * f).astype(np.float32)
            v = np.rint(np.minimum((w * np.float32(UNIT)).astype(np.float32), np.float32(MAX_WEIGHT)))
            v = np.where(np.isfinite(w), np.maximum(v, 1), 0)
            q[k, ya, xa] = v.astype(np.uint32)
    return q


def flat_sources(sources, W):
    return [int(r) * W + int(c) for r, c in sources]


def dijkstra(q, sources):
    """a heap on Python integers -> cost uint32 [H, W]"""
    _, H, W = q.shape
    dist = [UNREACHED] * (H * W)
    heap = []
    for s in flat_sources(sources, W):
        if dist[s] != 0:
            dist[s] = 0
            heap.append((0, s))
    heapq.heapify(heap)
    ql = q.reshape(8, -1).tolist()
    while heap:
        d, c = heapq.heappop(heap)
        if d != dist[c]:
            continue
        i, j = divmod(c, W)
        for k, (dy, dx) in enumerate(OFFSETS):
            w = ql[k][c]
            if w == 0:
                continue
            n = (i + dy) * W + (j + dx)
            nd = d + w
            if nd < UNREACHED and nd < dist[n]:
                dist[n] = nd
                heapq.heappush(heap, (nd, n))
    return np.array(dist, np.uint64).astype(np.uint32).reshape(H, W)


def jacobi(q, sources, start=None):
    """Jacobi sweeps from UNREACHED (or from ``start``, a plane at or above the fixed point) -> (cost, sweeps): the sweeps run
    until one changes nothing, that one included"""
    _, H, W = q.shape
    C = np.full((H, W), UNREACHED, np.int64) if start is None else np.asarray(start).astype(np.int64)
    for r, c in sources:
        C[r, c] = 0
    sweeps = 0
    while True:
        Pd = np.pad(C, 1, constant_values=UNREACHED)
        G = C.copy()
        for k, (dy, dx) in enumerate(OFFSETS):
            cn = Pd[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
            cand = cn + q[k].astype(np.int64)
            ok = (q[k] != 0) & (cn != UNREACHED) & (cand < UNREACHED)
            G = np.where(ok, np.minimum(G, cand), G)
        sweeps += 1
        if np.array_equal(G, C):
            return C.astype(np.uint32), sweeps
        C = G


def host_sweeps(jacobi_sweeps, cells, group=GROUP_PLAIN):
    """the launches the host's loop runs for a plain relaxation whose Jacobi count is ``jacobi_sweeps`` (the last of them changes
    nothing): groups of ``group``, the word read once per group, stop at the first group that changed nothing; sweep number
    ``cells`` goes out alone"""
    changing, done = jacobi_sweeps - 1, 0
    while True:
        assert done < cells
        left = cells - done - (1 if cells - done > 1 else 0)
        n = min(left, group)
        changed = done < changing                   # the group's first sweep is number done + 1
        done += n
        if not changed:
            return done


def parents(q, cost):
    _, H, W = q.shape
    C = cost.astype(np.int64)
    Pd = np.pad(C, 1, constant_values=UNREACHED)
    out = np.full((H, W), NO_PARENT, np.int8)
    out[C == 0] = -1
    open_ = (C != 0) & (C != UNREACHED)
    for k in range(7, -1, -1):
        dy, dx = OFFSETS[k]
        cn = Pd[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
        hit = open_ & (q[k] != 0) & (cn != UNREACHED) & (cn + q[k].astype(np.int64) == C)
        out[hit] = k
    return out


def territory_traffic(cost, parent, sources):
    """-> (territory int32: the ordinal of the source a cell travels to, duplicates keeping the lowest, -1 if unreached;
    traffic uint32: the cells whose way home passes through the cell, itself included, 0 if unreached), by one pass over the
    cells in increasing and one in decreasing cost"""
    H, W = cost.shape
    terr = np.full(H * W, -1, np.int64)
    for n, s in reversed(list(enumerate(flat_sources(sources, W)))):
        terr[s] = n
    traffic = (cost.ravel() != UNREACHED).astype(np.int64)
    par = parent.ravel()
    order = np.argsort(cost.ravel().astype(np.int64), kind="stable")
    recv = np.full(H * W, -1, np.int64)
    for c in range(H * W):
        if par[c] >= 0:
            dy, dx = OFFSETS[par[c]]
            recv[c] = c + dy * W + dx
    for c in order:
        if recv[c] >= 0:
            terr[c] = terr[recv[c]]
    for c in order[::-1]:
        if recv[c] >= 0:
            traffic[recv[c]] += traffic[c]
    return terr.reshape(H, W).astype(np.int32), traffic.reshape(H, W).astype(np.uint32)


Result = collections.namedtuple("Result", "q cost parent territory traffic")


def field(h, sources, travel=TRAVEL, penalty=None, depth=None, accumulation=None):
    q = weights(h, travel, penalty, depth, accumulation)
    cost = dijkstra(q, sources)
    par = parents(q, cost)
    terr, traffic = territory_traffic(cost, par, sources)
    return Result(q, cost, par, terr, traffic)


def walk(parent, cell):
    """the cells from ``cell`` to its source, [n, 2] int32"""
    i, j = int(cell[0]), int(cell[1])
    assert parent[i, j] != NO_PARENT
    out = [(i, j)]
    while parent[i, j] >= 0:
        dy, dx = OFFSETS[parent[i, j]]
        i, j = i + dy, j + dx
        out.append((i, j))
    return np.array(out, np.int32).reshape(-1, 2)


def raster(shape, paths):
    """uint32 plane: 1 on every cell of every path, 0 elsewhere"""
    m = np.zeros(shape, np.uint32)
    for p in paths:
        p = np.asarray(p).reshape(-1, 2)
        m[p[:, 0], p[:, 1]] = 1
    return m


# ---- the shared cases ----------------------------------------------------------------------------------------------------------
def sprinkled(H, W, seed):
    """a penalty plane: 10 % of the cells impassable, 10 % penalised by 2 .. 8, the rest 1"""
    rs = np.random.RandomState(1000 + seed)
    u = rs.rand(H, W)
    p = np.ones((H, W), np.float32)
    p[u < 0.2] = rs.uniform(2, 8, (H, W)).astype(np.float32)[u < 0.2]
    p[u < 0.1] = np.inf
    return p


def pick_sources(penalty, count, seed):
    """``count`` distinct passable cells, seeded"""
    rs = np.random.RandomState(2000 + seed)
    ok = np.argwhere(np.isfinite(penalty))
    return [tuple(int(v) for v in ok[i]) for i in rs.choice(len(ok), count, replace=False)]


def case(n, count):
    """shared case n with ``count`` sources -> (h, penalty, sources)"""
    H, W, q, seed = TERRAINS[n]
    pen = sprinkled(H, W, seed)
    return terrain(H, W, q, seed), pen, pick_sources(pen, count, seed + count)


# ---- adversarial planes ----------------------------------------------------------------------------------------------------------
def serpentine(n=67):
    """a flat n x n plane (n odd) whose impassable walls leave one corridor, one cell wide: every even row, joined to the next
    even row by one cell at alternating ends -> (h, penalty, source, far end, the far end's cost in units).  Along a row only
    straight steps exist (64 each); a turn is cut by two diagonal steps through the joining cell (91 each)"""
    h = np.zeros((n, n), np.float32)
    pen = np.full((n, n), np.inf, np.float32)
    rows = list(range(0, n, 2))
    for a, i in enumerate(rows):
        pen[i, :] = 1
        if a + 1 < len(rows):
            pen[i + 1, n - 1 if a % 2 == 0 else 0] = 1
    R = len(rows)
    end = (rows[-1], n - 1 if (R - 1) % 2 == 0 else 0)
    units = 64 * (2 * (n - 2) + (R - 2) * (n - 3)) + 91 * 2 * (R - 1)
    return h, pen, (0, 0), end, units


def walled_in(H=40, W=45, at=(20, 22)):
    """a flat plane whose source sits inside a closed ring of impassable cells"""
    pen = np.ones((H, W), np.float32)
    i, j = at
    pen[i - 1:i + 2, j - 1:j + 2] = np.inf
    pen[i, j] = 1
    return np.zeros((H, W), np.float32), pen, at


def lake_plane(H=36, W=40):
    """a flat plane with a rectangular lake in its middle: -> (h, depth)"""
    depth = np.zeros((H, W), np.float32)
    depth[8:H - 8, 12:W - 12] = 0.5
    return np.zeros((H, W), np.float32), depth


def saturated_strip(W=300):
    """a flat 1 x W strip with penalty 1e9 everywhere but the source at column 0: every edge clamps to MAX_WEIGHT"""
    pen = np.full((1, W), 1e9, np.float32)
    pen[0, 0] = 1
    return np.zeros((1, W), np.float32), pen, (0, 0)
