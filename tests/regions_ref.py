"""The regions' definition (include/ghm.h, section "regions"; gan_heightmaps_amd/regions.py) restated in plain Python:
the components by a breadth-first search, the boundary edges cell by cell, the successor by its three candidates, the rings by
walking the successor.  Integers throughout; the device code is held to it bit for bit.

Cells are flat-indexed row W + col, grid corners row (W + 1) + col.  The sides of a cell go clockwise on screen (rows down):
N (r, c) -> (r, c + 1), E (r, c + 1) -> (r + 1, c + 1), S (r + 1, c + 1) -> (r + 1, c), W (r + 1, c) -> (r, c)."""
import functools
from collections import deque

import numpy as np

from tests.contour_ref import heights, quantise

ACROSS = ((-1, 0), (0, 1), (1, 0), (0, -1))         # the cell across side N, E, S, W
START = ((0, 0), (0, 1), (1, 1), (1, 0))            # the corner a side starts at, relative to the cell


def components(L):
    """-> component int32 [H, W]: the least flat index of the cell's component, -1 where L < 0"""
    H, W = L.shape
    comp = np.full((H, W), -1, np.int32)
    for r0 in range(H):
        for c0 in range(W):
            if L[r0, c0] < 0 or comp[r0, c0] >= 0:
                continue
            seed = r0 * W + c0                       # raster order: the first cell met is the least
            comp[r0, c0] = seed
            todo = deque([(r0, c0)])
            while todo:
                r, c = todo.popleft()
                for dr, dc in ACROSS:
                    y, x = r + dr, c + dc
                    if 0 <= y < H and 0 <= x < W and comp[y, x] < 0 and L[y, x] == L[r0, c0]:
                        comp[y, x] = seed
                        todo.append((y, x))
    return comp


def is_edge(L, r, c, s):
    H, W = L.shape
    if not (0 <= r < H and 0 <= c < W) or L[r, c] < 0:
        return False
    y, x = r + ACROSS[s][0], c + ACROSS[s][1]
    return not (0 <= y < H and 0 <= x < W) or L[y, x] != L[r, c]


def successor(L, r, c, s):
    """the edge that starts where edge (r, c, s) ends: turn right, else straight on, else turn left"""
    t = (s + 1) % 4
    if is_edge(L, r, c, t):
        return r, c, t
    r, c = r + ACROSS[t][0], c + ACROSS[t][1]
    if is_edge(L, r, c, s):
        return r, c, s
    r, c = r + ACROSS[s][0], c + ACROSS[s][1]
    assert is_edge(L, r, c, (s + 3) % 4)
    return r, c, (s + 3) % 4


def definition(L):
    """-> dict of every array and count the device gives for the label plane L"""
    L = np.asarray(L, np.int32)
    H, W = L.shape
    comp = components(L)
    flat = comp.ravel()
    seed = np.flatnonzero(flat == np.arange(H * W)).astype(np.int32)
    number = {int(s): p for p, s in enumerate(seed)}
    polygon = np.array([number[int(v)] if v >= 0 else -1 for v in flat], np.int32).reshape(H, W)
    cells = np.bincount(polygon[polygon >= 0], minlength=len(seed)).astype(np.uint32)
    keys = [(r, c, s) for r in range(H) for c in range(W) for s in range(4) if is_edge(L, r, c, s)]
    eid = {k: i for i, k in enumerate(keys)}
    succ = np.array([eid[successor(L, *k)] for k in keys], np.int64)
    pred = np.full(len(keys), -1, np.int64)
    pred[succ] = np.arange(len(keys))
    ring_of = np.full(len(keys), -1, np.int64)
    vertex, offsets, ring_polygon, ring_hole, ring_edges = [], [0], [], [], []
    for e0 in range(len(keys)):                      # ascending: e0 is its ring's least edge
        if ring_of[e0] >= 0:
            continue
        k, e, n = len(ring_polygon), e0, 0
        while ring_of[e] < 0:
            ring_of[e] = k
            r, c, s = keys[e]
            if keys[int(pred[e])][2] != s:           # a corner edge: its start corner is a vertex
                vertex.append((r + START[s][0]) * (W + 1) + c + START[s][1])
            e, n = int(succ[e]), n + 1
        assert e == e0
        r, c, s = keys[e0]
        ring_polygon.append(int(polygon[r, c]))
        ring_hole.append(0 if (s == 0 and r * W + c == comp[r, c]) else 1)
        ring_edges.append(n)
        offsets.append(len(vertex))
    longest = max(ring_edges) if ring_edges else 0
    rounds = 0
    while (1 << rounds) < longest - 1:               # the greatest rank is the longest ring's length - 1
        rounds += 1
    return dict(component=comp, polygon=polygon, seed=seed, label=L.ravel()[seed].astype(np.int32), cells=cells,
                vertex=np.array(vertex, np.int32), ring_offsets=np.array(offsets, np.int64),
                ring_polygon=np.array(ring_polygon, np.int32), ring_hole=np.array(ring_hole, np.uint8),
                edges=len(keys), rings=len(ring_polygon), polygons=len(seed), holes=int(sum(ring_hole)), vertices=len(vertex),
                rounds=rounds, ring_edges=np.array(ring_edges, np.int64), succ=succ)


def doubled_areas(e, W):
    """int64 [R]: twice the signed shoelace area of every ring in (x = col, y = row); positive for the clockwise-on-screen outer
    rings"""
    out = np.zeros(e["rings"], np.int64)
    for k in range(e["rings"]):
        v = e["vertex"][e["ring_offsets"][k]:e["ring_offsets"][k + 1]].astype(np.int64)
        y, x = v // (W + 1), v % (W + 1)
        out[k] = int((x * np.roll(y, -1) - np.roll(x, -1) * y).sum())
    return out


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def serpentine():
    L = np.full((33, 35), -1, np.int32)
    L[0::2] = 0
    for k in range(16):
        L[2 * k + 1, 34 if k % 2 == 0 else 0] = 0
    return L


def moat():
    """the serpentine as label 1 inside a frame of label 0 that its gaps join: the frame's one hole is the serpentine's ring"""
    L = np.zeros((35, 37), np.int32)
    L[1:34, 1:36] = np.where(serpentine() == 0, 1, 0)
    return L


def nested(a=0, b=1):
    L = np.full((5, 5), a, np.int32)
    L[1:4, 1:4] = b
    L[2, 2] = a
    return L


def hole_pinch():
    L = np.zeros((4, 4), np.int32)
    L[1, 1] = L[2, 2] = 1
    return L


def pinch():
    L = np.full((4, 4), -1, np.int32)
    L[0:2, 0:2] = L[2:4, 2:4] = 0
    return L


def land(H, W, seed, sea_q=2048):
    """the value noise of the contour tests above a sea level: 0 on land, -1 in the sea"""
    return np.where(quantise(heights(H, W, seed), 64.0) > sea_q, 0, -1).astype(np.int32)


def bands(H, W, seed, interval_q=2048):
    """the number of contour levels (multiples of interval_q from 0 on) below a cell"""
    zq = quantise(heights(H, W, seed), 64.0).astype(np.int64)
    return np.maximum((zq + interval_q - 1) // interval_q, 0).astype(np.int32)


CASES = {
    "one": lambda: np.array([[0]], np.int32),
    "checker2": lambda: np.array([[0, 1], [1, 0]], np.int32),
    "diag": lambda: np.array([[0, -1], [-1, 0]], np.int32),
    # four edges a cell on more than 32 x 256 cells: the scan over the edges has four times the blocks of a scan over the cells
    "checker96": lambda: (np.add.outer(np.arange(96), np.arange(96)) % 2).astype(np.int32),
    "checker7x9": lambda: (np.add.outer(np.arange(7), np.arange(9)) % 2).astype(np.int32),
    "nested": nested,
    "nested_7_max": lambda: nested(7, 2 ** 31 - 1),
    "hole_pinch": hole_pinch,
    "pinch": pinch,
    "serpentine": serpentine,
    "moat": moat,
    "random3": lambda: (np.random.RandomState(23).randint(0, 3, (33, 29)) - 1).astype(np.int32),
    "empty": lambda: np.full((5, 7), -3, np.int32),
    "row": lambda: (np.arange(41) // 5 % 3 - 1).astype(np.int32)[None, :],
    "column": lambda: (np.arange(37) // 4 % 2).astype(np.int32)[:, None],
    "land37": lambda: land(37, 53, 3),
    "bands37": lambda: bands(37, 53, 3, 2048),
    "land96": lambda: land(96, 131, 7),
    "bands96": lambda: bands(96, 131, 0, 2048),
}
# the issue's table: edges, rings, polygons, holes, vertices
TABLE = {"one": (4, 1, 1, 0, 4), "checker2": (16, 4, 4, 0, 16), "diag": (8, 2, 2, 0, 8), "checker7x9": (252, 63, 63, 0, 252),
         "nested": (52, 5, 3, 2, 20), "hole_pinch": (32, 4, 3, 1, 20), "pinch": (16, 2, 2, 0, 8), "serpentine": (1224, 1, 1, 0, 68),
         "random3": (1710, 263, 263, 0, 1336)}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> the case's label plane; shared, so nobody writes into it"""
    L = np.ascontiguousarray(CASES[name](), np.int32)
    L.setflags(write=False)
    return L


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> the definition of a case, computed once and shared"""
    e = definition(case(name))
    for v in e.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return e
