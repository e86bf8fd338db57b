"""A numpy restatement of the earthworks (gan_heightmaps_amd/earthworks.py, csrc/earthworks.hip), written from the
text of the module's docstring and sharing no code with it.

The nearest mark: the offsets (dy, dx) of the window with dy^2 + dx^2 <= R^2 are visited in the order (d2, dy, dx) and every cell
keeps its first hit -- for one cell dy orders the rows and dx the columns, so this is the least (d2, row, col).  The shaping: numpy
float32 arithmetic, one operation per statement.  Profile's table in float64, rounded once.  The two target builders walk cell by
cell in Python integers and floats: they are small."""
import functools
import math

import numpy as np

NONE = -1
MAX_REACH = 32
TILE = 32
OFFSETS = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))      # k = 0 .. 7: N NE E SE S SW W NW
MODES = ('both', 'cut', 'fill')

# the planes of the device and host-build tests: the smallest where indexing, tile edges and the window can go wrong
PLANES = ((1, 1), (1, 40), (40, 1), (31, 33), (33, 65), (64, 64), (70, 45))
REACHES = (0, 1, 5)
BIG = ((33, 65), 32)                                     # a window larger than the plane
KINDS = ('none', 'all', 'corners', 'checker', 'pairs', 'scatter', 'values')


def offsets(R):
    """[(d2, dy, dx)] of the window, in the order of the search"""
    return sorted((dy * dy + dx * dx, dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1) if dy * dy + dx * dx <= R * R)


def _shifted(marked, dy, dx):
    """s[y, x] = marked[y + dy, x + dx], False outside the plane"""
    H, W = marked.shape
    s = np.zeros((H, W), bool)
    ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
    if ys.start < ys.stop and xs.start < xs.stop:
        s[ys, xs] = marked[ys.start + dy:ys.stop + dy, xs.start + dx:xs.stop + dx]
    return s


def nearest(marks, R, threshold=1):
    """-> (nearest, dist2) int32"""
    marked = np.asarray(marks).astype(np.int64) >= threshold
    H, W = marked.shape
    near, dist2 = np.full((H, W), NONE, np.int32), np.full((H, W), NONE, np.int32)
    i, j = np.indices((H, W))
    for d2, dy, dx in offsets(R):
        hit = _shifted(marked, dy, dx) & (near == NONE)
        near[hit] = ((i + dy) * W + (j + dx))[hit]
        dist2[hit] = d2
    return near, dist2


def ties(marks, R, threshold, dist2):
    """the number of cells with more than one marked cell at their least distance"""
    marked = np.asarray(marks).astype(np.int64) >= threshold
    count = np.zeros(marked.shape, np.int64)
    for d2, dy, dx in offsets(R):
        count += _shifted(marked, dy, dx) & (dist2 == d2)
    return int((count > 1).sum())


def table(core, reach):
    """float32 [R^2 + 1, 2] of (keep, take)"""
    R = int(math.floor(reach))
    rows = []
    for d2 in range(R * R + 1):
        r = math.sqrt(d2)
        if reach == core:
            s = 0.0 if r <= core else 1.0
        else:
            s = min(1.0, max(0.0, (r - core) / (reach - core)))
        take = 1.0 - (s * s) * (3.0 - 2.0 * s)
        rows.append((np.float32(1.0 - take), np.float32(take)))
    return np.array(rows, np.float32).reshape(-1, 2)


def shape(h, near, dist2, target, tab, mode):
    """float32, op by op"""
    h = np.asarray(h, np.float32)
    H, W = h.shape
    found = near != NONE
    d2 = np.where(found, dist2, 0)
    keep, take = tab[d2, 0], tab[d2, 1]
    touched = found & (take != 0)
    t = np.asarray(target, np.float32).reshape(-1)[np.where(found, near, 0)]
    with np.errstate(invalid="ignore", over="ignore"):
        kh = (keep * h).astype(np.float32)
        tt = (take * t).astype(np.float32)
        v = (kh + tt).astype(np.float32)
    if mode == 1:
        v = np.where(v < h, v, h)
    elif mode == 2:
        v = np.where(v > h, v, h)
    return np.where(touched, v, h).astype(np.float32)


def carve(h, marks, target, core, reach, mode='both', threshold=1):
    R = int(math.floor(reach))
    near, dist2 = nearest(marks, R, threshold)
    return shape(h, near, dist2, target, table(core, reach), MODES.index(mode)), near, dist2


def channel_targets(filled, depth, accumulation, river_threshold=256, lake_min_depth=1.0 / 512, depth0=0.5, growth=0.25,
                    max_depth=3.0, height_scale=64.0):
    """-> (marks uint32, target float32, NaN off the marks), cell by cell"""
    H, W = filled.shape
    marks, target = np.zeros((H, W), np.uint32), np.full((H, W), np.nan, np.float32)
    for y in range(H):
        for x in range(W):
            acc = int(accumulation[y, x])
            if acc >= river_threshold and not depth[y, x] > np.float32(lake_min_depth):
                b = (acc // river_threshold).bit_length() - 1
                D = min(max_depth, depth0 + growth * b)
                marks[y, x] = 1
                target[y, x] = np.float32(filled[y, x]) - np.float32(D / height_scale)
    return marks, target


def parent_of(parent, y, x):
    """the cell (y, x) leaves to, or None at a source, an unreached cell and the plane's edge"""
    k = int(parent[y, x])
    if not 0 <= k < 8:
        return None
    y, x = y + OFFSETS[k][0], x + OFFSETS[k][1]
    return (y, x) if 0 <= y < parent.shape[0] and 0 <= x < parent.shape[1] else None


def road_targets(h, parent, seeds, smooth=8):
    """-> (marks uint32, target float32, NaN off the marks), a walk per cell"""
    H, W = h.shape
    marked = np.zeros((H, W), bool)
    for y, x in np.argwhere(seeds):
        c = (int(y), int(x))
        while c is not None and not marked[c]:
            marked[c] = True
            c = parent_of(parent, *c)
    target = np.full((H, W), np.nan, np.float32)
    for y, x in np.argwhere(marked):
        c = (int(y), int(x))
        total, count = float(h[c]), 1
        for _ in range(smooth):
            c = parent_of(parent, *c)
            if c is None:
                break
            total += float(h[c])
            count += 1
        target[y, x] = np.float32(total / count)
    return marked.astype(np.uint32), target


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def marks_case(kind, H, W):
    """-> (marks uint32 [H, W], threshold)"""
    m = np.zeros((H, W), np.uint32)
    if kind == 'none':
        return m, 1
    if kind == 'all':
        return m + np.uint32(7), 7
    if kind == 'corners':
        for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (31, 31), (32, 32)):
            if y < H and x < W:
                m[y, x] = 1
        return m, 1
    if kind == 'checker':
        i, j = np.indices((H, W))
        return (((i + j) & 1) == 0).astype(np.uint32), 1
    if kind == 'pairs':
        # two marks a cell apart from a middle cell: across, up and down, and along a diagonal, by the tile's edge where it fits
        for (y, x), (dy, dx) in (((H // 4, W // 2), (0, 2)), ((H // 2, W // 4), (2, 0)), ((3 * H // 4, 3 * W // 4), (1, 1)),
                                 ((31, 31), (1, -1))):
            for s in (-1, 1):
                yy, xx = y + s * dy, x + s * dx
                if 0 <= yy < H and 0 <= xx < W:
                    m[yy, xx] = 1
        return m, 1
    if kind == 'scatter':
        rs = np.random.RandomState(1000 * H + W)
        m = (rs.rand(H, W) < 0.01).astype(np.uint32) * np.uint32(0xFFFFFFFF)
        m[rs.randint(H), rs.randint(W)] = 0xFFFFFFFF
        return m, 0x80000000
    if kind == 'values':
        return np.random.RandomState(2000 * H + W).randint(0, 6, (H, W)).astype(np.uint32), 3
    raise ValueError(kind)


def nearest_cases():
    """[((H, W), R)]: every plane at every reach, and the big window"""
    return [(s, R) for s in PLANES for R in REACHES] + [BIG]


@functools.lru_cache(maxsize=None)
def nearest_case(kind, shape_, R):
    """-> (marks, threshold, nearest, dist2), computed once and shared; read-only"""
    m, thr = marks_case(kind, *shape_)
    near, dist2 = nearest(m, R, thr)
    for a in (m, near, dist2):
        a.setflags(write=False)
    return m, thr, near, dist2


def heights(H, W, seed):
    """finite heights with negatives, both zeros' neighbourhood and denormals"""
    rs = np.random.RandomState(seed)
    h = (rs.rand(H, W).astype(np.float32) - np.float32(0.5)) * np.float32(3)
    flat = h.reshape(-1)
    flat[::7] = np.float32(1e-41) * rs.randint(-9, 10, flat[::7].size).astype(np.float32)      # denormals and zeros
    flat[3::11] *= np.float32(1e-3)
    return h


def shape_case(shape_, R, seed):
    """-> (h, marks, threshold, target with NaN off the marks)"""
    H, W = shape_
    m, thr = marks_case('scatter' if H * W > 64 else 'corners', H, W)
    rs = np.random.RandomState(seed + 1)
    t = (rs.rand(H, W).astype(np.float32) - np.float32(0.5)) * np.float32(2)
    t[m.astype(np.int64) < thr] = np.nan
    return heights(H, W, seed), m, thr, t
