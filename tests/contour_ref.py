"""The contours' definition (include/ghm.h, section "contour") restated in numpy and plain Python integers, on its own:
nothing here imports the package.  ``segments`` lists every segment of every cell in key order, ``trace`` links them into lines,
``marks`` is the plane the paint reads; then the case generators the host build's and the device's tests share.
``expected(name)`` computes a case's answer once.

    zq = int32(rint(float32(h) * float32(height_scale * 256)))      the viewshed's quantisation;  Z = 2 zq, even
    level j: lam_j = 2 (base_q + j interval_q) + 1, odd; with ``count`` only j in [0, count)
    cell (r, c), r < H - 1, c < W - 1, corners TL, TR, BR, BL = Z[r, c], Z[r, c + 1], Z[r + 1, c + 1], Z[r + 1, c];
    edges 0 top (TL - TR), 1 right (TR - BR), 2 bottom (BR - BL), 3 left (BL - TL), in the clockwise order of the corners.
    A level with min < lam < max crosses the cell.  Going round clockwise, an edge that leads from a corner above lam to one below
    is an entry edge, one that leads from below to above an exit edge: a segment runs from an entry to an exit, higher ground on
    one fixed side.  A saddle has two of each; its centre is above iff TL + TR + BR + BL > 4 lam, and the entry e leaves through
    e + 1 (centre above: the corner below is cut off) or e - 1 (centre below or level: the corner above is cut off).
    A vertex is (r, c, axis, t): axis 0 the edge (r, c) - (r, c + 1), axis 1 the edge (r, c) - (r + 1, c); t = float64(lam - Z_first) /
    float64(Z_second - Z_first), one division.
"""
import functools

import numpy as np

from tests import viewshed_ref as V

quantise = V.quantise
heights = V.heights

# the cell across an edge, and the corners (dr, dc) an edge leads from and to, clockwise
ACROSS = ((-1, 0), (0, 1), (1, 0), (0, -1))
CORNERS = ((0, 0), (0, 1), (1, 1), (1, 0))


def lam(j, base_q, interval_q):
    return 2 * (int(base_q) + int(j) * int(interval_q)) + 1


def level_range(zlo, zhi, base_q, interval_q, count=None):
    """the levels j with zlo < lam_j < zhi (Z units), as range(lo, hi), clipped to [0, count)"""
    b2, i2 = 2 * int(base_q) + 1, 2 * int(interval_q)
    lo = (int(zlo) - b2) // i2 + 1                 # the least j with b2 + j i2 > zlo
    hi = -((b2 - int(zhi)) // i2)                  # the least j with b2 + j i2 >= zhi  (never equal: lam is odd, Z even)
    if count is not None:
        lo, hi = max(lo, 0), min(hi, int(count))
    return range(lo, max(lo, hi))


def vertex(Z, r, c, e, lm):
    """the crossing of level lm with edge e of cell (r, c): (row, col, axis, t)"""
    vr, vc, axis = ((r, c, 0), (r, c + 1, 1), (r + 1, c, 0), (r, c, 1))[e]
    a = int(Z[vr, vc])
    b = int(Z[vr, vc + 1]) if axis == 0 else int(Z[vr + 1, vc])
    return vr, vc, axis, float(lm - a) / float(b - a)


def cell_segments(Z, r, c, base_q, interval_q, count=None):
    """the segments of one cell in key order: (key, entry vertex, exit vertex, exit edge), key = (r, c, j, entry edge)"""
    z = [int(Z[r + dr, c + dc]) for dr, dc in CORNERS]
    out = []
    for j in level_range(min(z), max(z), base_q, interval_q, count):
        lm = lam(j, base_q, interval_q)
        up = [v > lm for v in z]
        entries = [e for e in range(4) if up[e] and not up[(e + 1) % 4]]
        exits = [e for e in range(4) if not up[e] and up[(e + 1) % 4]]
        if len(entries) == 2:
            step = 1 if sum(z) > 4 * lm else 3
            pairs = [(e, (e + step) % 4) for e in entries]
        else:
            pairs = [(entries[0], exits[0])]
        for e, x in pairs:
            out.append(((r, c, j, e), vertex(Z, r, c, e, lm), vertex(Z, r, c, x, lm), x))
    return out


def segments(zq, base_q, interval_q, count=None):
    Z = 2 * np.asarray(zq).astype(np.int64)
    H, W = Z.shape
    out = []
    for r in range(H - 1):
        for c in range(W - 1):
            out += cell_segments(Z, r, c, base_q, interval_q, count)
    return out


def link(segs, shape):
    """-> (succ, pred): ids in key order, -1 where the line leaves the plane"""
    H, W = shape
    at = {s[0]: i for i, s in enumerate(segs)}
    succ = [-1] * len(segs)
    pred = [-1] * len(segs)
    for i, ((r, c, j, e), _, _, x) in enumerate(segs):
        nr, nc = r + ACROSS[x][0], c + ACROSS[x][1]
        if 0 <= nr < H - 1 and 0 <= nc < W - 1:
            n = at[(nr, nc, j, (x + 2) % 4)]          # it exists and is unique: the shared edge is crossed by level j
            assert pred[n] == -1
            succ[i], pred[n] = n, i
    return succ, pred


def lines_of(segs, shape):
    """-> [(closed, [segment ids in order])], ordered by the start segment's id"""
    succ, pred = link(segs, shape)
    seen = [False] * len(segs)
    out = []
    for i in range(len(segs)):                        # the open lines: from a segment without a predecessor
        if pred[i] == -1:
            ids = []
            while i != -1:
                seen[i] = True
                ids.append(i)
                i = succ[i]
            out.append((False, ids))
    for i in range(len(segs)):                        # the loops: the first unseen id is its loop's least
        if not seen[i]:
            ids = []
            k = i
            while not seen[k]:
                seen[k] = True
                ids.append(k)
                k = succ[k]
            assert k == i
            out.append((True, ids))
    out.sort(key=lambda l: l[1][0])
    return out


def trace(zq, base_q, interval_q, count=None):
    """-> dict(edge int32 [V, 3], t float64 [V], offsets int64 [L + 1], level int32 [L], closed uint8 [L], segments, longest)"""
    shape = np.asarray(zq).shape
    segs = segments(zq, base_q, interval_q, count)
    lines = lines_of(segs, shape)
    edge, t, offsets, level, closed = [], [], [0], [], []
    for cl, ids in lines:
        vs = [segs[i][1] for i in ids]
        if not cl:
            vs.append(segs[ids[-1]][2])
        else:
            assert segs[ids[-1]][2] == segs[ids[0]][1]
        edge += [v[:3] for v in vs]
        t += [v[3] for v in vs]
        offsets.append(len(edge))
        level.append(segs[ids[0]][0][2])
        closed.append(1 if cl else 0)
    return dict(edge=np.array(edge, np.int32).reshape(-1, 3), t=np.array(t, np.float64), offsets=np.array(offsets, np.int64),
                level=np.array(level, np.int32), closed=np.array(closed, np.uint8), segments=len(segs),
                longest=max([len(ids) for _, ids in lines] + [0]))


def marks(zq, base_q, interval_q, count=None, index_every=5):
    """uint32 [H, W]: 0 where no level separates Z[r, c] from Z[r, c + 1] and from Z[r + 1, c], 2 where an index contour does, else 1"""
    Z = 2 * np.asarray(zq).astype(np.int64)
    H, W = Z.shape
    out = np.zeros((H, W), np.uint32)
    for r in range(H):
        for c in range(W):
            m = 0
            for nr, nc in ((r, c + 1), (r + 1, c)):
                if nr < H and nc < W:
                    a, b = int(Z[r, c]), int(Z[nr, nc])
                    js = level_range(min(a, b), max(a, b), base_q, interval_q, count)
                    if len(js):
                        first = -((-js[0]) // index_every) * index_every          # the least multiple of index_every >= js[0]
                        m = max(m, 2 if first < js[-1] + 1 else 1)
            out[r, c] = m
    return out


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def serpentine(open_end=False, n=97):
    """zq [n, n]: a ridge 1024 high, one cell wide, along the rows 2, 6, ... between the columns 2 and n - 3, joined at alternating
    ends; open_end: the first row runs off the left edge"""
    z = np.zeros((n, n), np.int32)
    rows = list(range(2, n - 2, 4))
    for k, r in enumerate(rows):
        z[r, 2:n - 2] = 1024
        if k + 1 < len(rows):
            col = n - 3 if k % 2 == 0 else 2
            z[r:r + 5, col] = 1024
    if open_end:
        z[2, :2] = 1024
    return z


def code_cell(code):
    """zq [2, 2] whose corners TL, TR, BR, BL lie above level 0 (base_q 0, interval_q 1) where bit 3, 2, 1, 0 of code is set"""
    tl, tr, br, bl = ((code >> k) & 1 for k in (3, 2, 1, 0))
    return np.array([[tl, tr], [bl, br]], np.int32)


def _noise(H, W, seed, interval_q, **kw):
    return dict(zq=quantise(heights(H, W, seed), 64.0), base_q=0, interval_q=interval_q, count=None, index_every=5, **kw)


def _case(zq, base_q=0, interval_q=1, count=1, index_every=5):
    return dict(zq=np.asarray(zq, np.int32), base_q=base_q, interval_q=interval_q, count=count, index_every=index_every)


CASES = {
    "row": lambda: _case(np.arange(7, dtype=np.int32)[None, :] * 300, 0, 256, None),
    "column": lambda: _case(np.arange(7, dtype=np.int32)[:, None] * 300, 0, 256, None),
    "peak": lambda: _case([[0, 0, 0], [0, 1024, 0], [0, 0, 0]], 0, 256, None),
    "steep": lambda: _case([[0, 16384], [0, 16384]], 0, 256, None),
    "steep_diag": lambda: _case([[5000, 0], [0, 16384]], 0, 256, None),           # the levels 0 .. 19 cross a saddle
    "saddle_a_above": lambda: _case([[4, 0], [0, 4]], 1, 1, 1),          # lam = 3: the corners' sum 16 > 12
    "saddle_a_below": lambda: _case([[2, 0], [0, 2]], 1, 1, 1),          # 8 < 12
    "saddle_b_above": lambda: _case([[0, 4], [4, 0]], 1, 1, 1),
    "saddle_b_below": lambda: _case([[0, 2], [2, 0]], 1, 1, 1),
    "tie": lambda: _case([[0, 1], [1, 0]], 0, 1, 1),                     # lam = 1: 4 == 4, the centre counts as below
    "noise37": lambda: _noise(37, 53, 3, 256),
    "noise37_512": lambda: _noise(37, 53, 3, 512),
    "noise96": lambda: _noise(96, 131, 7, 256),
    "noise96_512": lambda: _noise(96, 131, 7, 512),
    "integers": lambda: _case(np.random.RandomState(23).randint(0, 64, (33, 29)).astype(np.int32) * 300, 0, 256, None, 3),
    "serpentine": lambda: _case(serpentine(False), 512, 256, 1),
    "serpentine_open": lambda: _case(serpentine(True), 512, 256, 1),
    "clipped": lambda: dict(_noise(37, 53, 24, 256), base_q=4000, count=6, index_every=2),
    "negative_base": lambda: dict(_noise(37, 53, 25, 384), base_q=-1000, index_every=4),
}
for _code in range(16):
    CASES["code%02d" % _code] = functools.partial(lambda k: _case(code_cell(k), 0, 1, 1), _code)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> the case's dict; shared, so nobody writes into it"""
    c = CASES[name]()
    c["zq"].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> (trace, marks) of a case, computed once and shared"""
    c = case(name)
    tr = trace(c["zq"], c["base_q"], c["interval_q"], c["count"])
    mk = marks(c["zq"], c["base_q"], c["interval_q"], c["count"], c["index_every"])
    for v in list(tr.values()) + [mk]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return tr, mk
