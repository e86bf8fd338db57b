"""How to get from here to there on a heightmap, and where the roads would run: least-cost travel fields from a set of sources,
computed on the device (csrc/route.hip).

The plane is h[H, W], float32 and finite (it is read as h + 0; uint8 is read as v / 255).  The eight neighbours of a cell are
k = 0 .. 7 in the order N, NE, E, SE, S, SW, W, NW -- the hydrology's.  Every float32 operation below is rounded on its own, and
none of them is a division.

1. The cell penalty P[c] = ((penalty[c] lake_c) ford_c), in that order.  ``penalty`` is an optional float32 plane with values
   >= 1, or +inf for impassable ground; it defaults to 1.  lake_c = travel.lake where a ``depth`` plane is given and depth[c] >
   travel.lake_min_depth, otherwise 1; ford_c = travel.ford where an ``accumulation`` plane is given and accumulation[c] >=
   travel.river_threshold, otherwise 1.  lake and ford are >= 1, and lake may be +inf.
2. The edge weight between a cell a and its neighbour b in direction k, with z = height_scale h:
   g = |z_a - z_b| R_k, R_k = 1 or float32(0.70710678);  s = g inv_grade, inv_grade = float32(1 / travel.grade);  f = 1 + s s;
   m = 0.5 (P_a + P_b);  w = (L_k m) f, L_k = 1 or float32(1.41421356).  q_k(a) is a uint32: 0, no edge, if w is not finite,
   otherwise max(1, rint(min(w UNIT, MAX_WEIGHT))), UNIT = 64 and MAX_WEIGHT = 2^24.  The weight is symmetric bit for bit,
   q_k(a) = q_{k+4}(b), so four planes (E, SE, S, SW) hold all edges.  travel.grade is the grade at which a step costs twice
   its flat cost; steeper steps cost quadratically more, which is what makes roads wind.
3. ``cost`` is a uint32 plane in units of 1 / UNIT: 0 at the sources, elsewhere the least, over the present edges to neighbours
   that are reached, of cost[n_k] + q_k(c); the sum is formed without wrapping and accepted only if it is < 0xFFFFFFFF
   (UNREACHED).  It is relaxed downward from UNREACHED.  All weights are positive integers, so there is one fixed point -- the
   one a heap Dijkstra gives -- whatever the order of the sweeps.  Cells behind impassable ground, or beyond 2^32 units, stay
   UNREACHED.
4. ``parent`` is an int8 plane: -1 at a source, -2 (NO_PARENT) at an unreached cell, elsewhere the lowest k with a present edge,
   a reached neighbour and cost[n_k] + q_k(c) == cost[c].  Weights are >= 1, so parents strictly descend in cost and form a
   forest rooted at the sources, in the encoding of the hydrology's ``direction`` plane.
5. ``territory`` (int32) is the ordinal, in ``sources``, of the source a cell travels to (duplicates keep the lowest), -1 where
   the cell is unreached; ``traffic`` (uint32) is the number of cells whose cheapest way home passes through the cell, itself
   included, 0 where it is unreached.  Both come from one call of the hydrology's accumulation over the parent plane.

The relaxation has two forms with the same bits: ``plain``, one Jacobi sweep per launch between two global planes, and ``tiled``,
32 x 32 tiles swept in LDS up to 32 times per launch.  The host launches in groups, reads one device word per group and stops at
the first group that changed nothing; needing more than H W sweeps is an error, not a hang.

``paint`` draws roads on a texture with the hydrology's paint kernel: the cells of the given paths, or with
``Road.traffic_threshold`` every cell whose traffic reaches it -- the trail network that emerges towards the towns.

    python -m gan_heightmaps_amd.route IN OUT_PREFIX --from R,C [--from R,C ...] [--to R,C ...] [--hydrology]
        [--texture F --painted OUT] [--road-width N] [--traffic-threshold N] [--grade X] [--lake X] [--ford X]
        [--river-threshold N] [--lake-min-depth X] [--height-scale X] [--plain | --tiled]
"""
import argparse
import dataclasses
import math
import re
import sys

import numpy as np

from . import hydrology as _hy
from .hydrology import MAX_RIVER_WIDTH, _as_plane
from .planes import check_keep, scratch
from .util import form_choice, is_int as _is_int, is_number as _number, read_image

__all__ = ["DEFAULT_TILED", "KEEP", "UNIT", "MAX_WEIGHT", "UNREACHED", "NO_PARENT", "MAX_SOURCES", "Travel", "Road", "CostField",
           "field", "paint", "raster", "parse_args", "main"]

UNIT = 64                    # GHM_ROUTE_UNIT (include/ghm.h)
MAX_WEIGHT = 1 << 24         # GHM_ROUTE_MAX_WEIGHT
UNREACHED = 0xFFFFFFFF       # GHM_ROUTE_UNREACHED
NO_PARENT = -2               # GHM_ROUTE_NO_PARENT
MAX_SOURCES = 65536          # GHM_ROUTE_MAX_SOURCES
KEEP = ('cost', 'parent', 'territory', 'traffic')
OFFSETS = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))
# the form ``field`` runs by default: the one tools/route_bench.py shows faster on the MI355X -- the tiled one, for a 4096 x 4096
# plane 37.2 against 758 ms with one source and 7.36 against 189 ms with 64 (DESIGN §4u has the line); both give the same bits
DEFAULT_TILED = True


@dataclasses.dataclass(frozen=True)
class Travel:
    """What travel costs, validated and frozen.  ``grade``: the grade (rise over run, heights times ``height_scale``, a cell one
    unit wide) at which a step costs twice its flat cost; ``lake`` (>= 1, may be inf: impassable) and ``ford`` (>= 1, finite)
    multiply the penalty of a cell whose filled depth exceeds ``lake_min_depth`` (>= 0) or whose drainage area reaches
    ``river_threshold`` cells (an integer in [1, 2^32)).  The defaults are chosen, not measured."""
    grade: float = 0.15
    lake: float = 16.0
    ford: float = 4.0
    river_threshold: int = 256
    lake_min_depth: float = 1.0 / 512
    height_scale: float = 64.0

    def __post_init__(self):
        for name in ("grade", "height_scale"):
            v = getattr(self, name)
            if not _number(v) or not 0 < v < 3e38 or not 1.0 / v < 3e38:           # 1 / grade is a float32 on the device
                raise ValueError("%s must be a positive finite number, got %r" % (name, v))
        v = self.lake
        if not _number(v, finite=False) or math.isnan(v) or not v >= 1:
            raise ValueError("lake must be a number >= 1 (inf: impassable), got %r" % (v,))
        if not _number(self.ford) or not 1 <= self.ford < 3e38:
            raise ValueError("ford must be a finite number >= 1, got %r" % (self.ford,))
        if not _is_int(self.river_threshold) or not 1 <= self.river_threshold < 1 << 32:
            raise ValueError("river_threshold must be an integer in [1, 2^32), got %r" % (self.river_threshold,))
        if not _number(self.lake_min_depth) or not 0 <= self.lake_min_depth < 3e38:
            raise ValueError("lake_min_depth must be a finite number >= 0, got %r" % (self.lake_min_depth,))
        for name in ("grade", "lake", "ford", "lake_min_depth", "height_scale"):
            object.__setattr__(self, name, float(getattr(self, name)))
        object.__setattr__(self, "river_threshold", int(self.river_threshold))


@dataclasses.dataclass(frozen=True)
class Road:
    """How ``paint`` shows roads, validated and frozen: path cells (or, with ``traffic_threshold``, an integer in [1, 2^32), the
    cells whose traffic reaches it) widened by ``width`` pixels (0 .. 4) are blended towards ``colour`` (three values in [0, 1])
    with ``opacity`` in [0, 1]."""
    width: int = 1
    colour: tuple = (0.35, 0.30, 0.25)
    opacity: float = 0.9
    traffic_threshold: object = None

    def __post_init__(self):
        if not _is_int(self.width) or not 0 <= self.width <= MAX_RIVER_WIDTH:
            raise ValueError("width must be an integer in [0, %d], got %r" % (MAX_RIVER_WIDTH, self.width))
        _hy._check_blend(self)
        t = self.traffic_threshold
        if t is not None and (not _is_int(t) or not 1 <= t < 1 << 32):
            raise ValueError("traffic_threshold must be None or an integer in [1, 2^32), got %r" % (t,))
        object.__setattr__(self, "width", int(self.width))
        object.__setattr__(self, "traffic_threshold", None if t is None else int(t))


class CostField:
    """What ``field`` returns: the planes it was asked to keep as numpy arrays (the others are None) -- ``cost`` uint32 in units
    of 1 / ``unit``, ``parent`` int8, ``territory`` int32, ``traffic`` uint32 -- the ``shape``, the ``origin`` (the coordinates of
    cell [0, 0]: cells go in and paths come out with it added), the ``sources`` as given, the ``sweeps`` (launches) the
    relaxation ran and its form ``tiled``."""
    unit = UNIT

    def __init__(self, shape, sources=(), origin=(0, 0), sweeps=0, tiled=False, **planes):
        self.shape = tuple(shape)
        self.sources = tuple(sources)
        self.origin = (int(origin[0]), int(origin[1]))
        self.sweeps = sweeps
        self.tiled = tiled
        for k in KEEP:
            setattr(self, k, planes.get(k))

    def __repr__(self):
        return "CostField(%d x %d at %r, %d sources, sweeps=%r, planes=%s)" % (
            self.shape + (self.origin, len(self.sources), self.sweeps, [k for k in KEEP if getattr(self, k) is not None]))

    def _local(self, cell):
        try:
            i, j = cell
            ok = _is_int(i) and _is_int(j)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError("a cell is (row, col), two integers, got %r" % (cell,))
        i, j = int(i) - self.origin[0], int(j) - self.origin[1]
        if not (0 <= i < self.shape[0] and 0 <= j < self.shape[1]):
            raise ValueError("cell %r lies outside the field of %d x %d at %r" % ((cell,) + self.shape + (self.origin,)))
        return i, j

    def travel_cost(self, cell):
        """the least cost from ``cell`` to a source, in cost units (a flat orthogonal step costs 1); inf if unreached"""
        if self.cost is None:
            raise ValueError("the field did not keep 'cost'")
        v = int(self.cost[self._local(cell)])
        return math.inf if v == UNREACHED else v / float(UNIT)

    def path(self, cell):
        """the cells from ``cell`` to its source, both included: int32 [n, 2] of (row, col) with the origin added.  A walk over
        ``parent`` on the host; ValueError if the cell is unreached"""
        if self.parent is None:
            raise ValueError("the field did not keep 'parent'")
        i, j = self._local(cell)
        par, (H, W) = self.parent, self.shape
        if par[i, j] == NO_PARENT:
            raise ValueError("cell %r is unreached: no path" % (cell,))
        out = [(i, j)]
        while par[i, j] >= 0:
            dy, dx = OFFSETS[par[i, j]]
            i, j = i + dy, j + dx
            if not (0 <= i < H and 0 <= j < W) or len(out) > H * W:
                raise ValueError("the parent plane is no forest inside the field")
            out.append((i, j))
        return (np.array(out, np.int64).reshape(-1, 2) + np.array(self.origin, np.int64)).astype(np.int32)

    def paths(self, cells):
        """[path(c) for c in cells]"""
        return [self.path(c) for c in cells]


def raster(shape, paths, origin=(0, 0)):
    """uint32 plane of ``shape``: 1 on every cell of every path ([n, 2] arrays of (row, col), ``origin`` included), 0 elsewhere;
    ValueError for a cell outside the plane"""
    H, W = shape
    m = np.zeros((H, W), np.uint32)
    for p in paths:
        p = np.asarray(p)
        if p.ndim != 2 or p.shape[1] != 2 or p.dtype.kind not in "iu":
            raise ValueError("a path is an integer array [n, 2] of (row, col), got %s %s" % (p.dtype, p.shape))
        i, j = p[:, 0].astype(np.int64) - int(origin[0]), p[:, 1].astype(np.int64) - int(origin[1])
        if p.shape[0] and (i.min() < 0 or j.min() < 0 or i.max() >= H or j.max() >= W):
            raise ValueError("a path leaves the plane of %d x %d at %r" % (H, W, tuple(origin)))
        m[i, j] = 1
    return m


def _check_travel(travel):
    travel = Travel() if travel is None else travel
    if not isinstance(travel, Travel):
        raise ValueError("travel must be a Travel, got %r" % (travel,))
    return travel


def _check_road(road):
    road = Road() if road is None else road
    if not isinstance(road, Road):
        raise ValueError("road must be a Road, got %r" % (road,))
    return road


def _check_sources(sources, H, W, origin=(0, 0)):
    """-> ([(row, col)] as given, int32 flat indices inside the plane)"""
    try:
        src = [tuple(s) for s in sources]
        ok = all(len(s) == 2 and _is_int(s[0]) and _is_int(s[1]) for s in src)
    except TypeError:
        ok = False
    if not ok:
        raise ValueError("sources must be a sequence of (row, col) integer pairs, got %r" % (sources,))
    if not 1 <= len(src) <= MAX_SOURCES:
        raise ValueError("%d sources: 1 .. %d are taken" % (len(src), MAX_SOURCES))
    flat = []
    for r, c in src:
        i, j = int(r) - origin[0], int(c) - origin[1]
        if not (0 <= i < H and 0 <= j < W):
            raise ValueError("source %r lies outside the plane of %d x %d at %r" % ((r, c), H, W, tuple(origin)))
        flat.append(i * W + j)
    return [(int(r), int(c)) for r, c in src], np.array(flat, np.int32)


def _check_penalty(penalty, H, W):
    if penalty is None:
        return None
    p = np.asarray(penalty)
    if p.shape != (H, W) or p.dtype.kind != "f":
        raise ValueError("penalty must be a floating-point plane of %d x %d, got %s %s" % (H, W, p.dtype, p.shape))
    p = np.ascontiguousarray(p, np.float32)
    if not (p >= 1).all():                               # NaN fails too; +inf passes: impassable
        raise ValueError("penalty values must be >= 1 (inf: impassable)")
    return p


def territory_traffic(basin, accumulation, cost, flat_sources):
    """what the hydrology's accumulation over the parent plane gives (``basin``: the flat index of the root of a cell's chain;
    ``accumulation``: the size of its upstream tree) -> (territory, traffic).  An unreached cell is a root of its own, and no
    source"""
    H, W = basin.shape
    ordinal = np.full(H * W, -1, np.int32)
    ordinal[np.asarray(flat_sources)[::-1]] = np.arange(len(flat_sources), dtype=np.int32)[::-1]     # the lowest ordinal last
    reached = cost != np.uint32(UNREACHED)
    territory = np.where(reached, ordinal[basin], np.int32(-1)).astype(np.int32)
    traffic = np.where(reached, accumulation, np.uint32(0)).astype(np.uint32)
    return territory, traffic


def field(ops, heightmap, sources, travel=None, hydro=None, penalty=None, tiled=None, keep=KEEP, origin=(0, 0)):
    """The least-cost travel field of a heightmap: upload, one weights launch, the relaxation, one parents launch, the doubling
    rounds of the hydrology's accumulation, download.
    ops: a device.Ops; heightmap: (H, W) or (1, H, W), floating point and finite, or uint8; sources: a sequence of (row, col),
    1 .. 65536 of them; travel: a Travel (default Travel()); hydro: a hydrology.Hydrology that kept ``depth`` and
    ``accumulation``, whose lakes and rivers then cost travel.lake and travel.ford -- intended use
    ``field(ops, hydro.filled, towns, hydro=hydro)``; penalty: a float plane, >= 1 or inf (impassable); tiled: the LDS form of the
    relaxation (True) or the plain one (False): the same bits; default DEFAULT_TILED.  keep: the planes to return.  origin: the
    coordinates of cell [0, 0], in which ``sources`` are given and paths come back.  Returns a CostField."""
    keep = check_keep(keep, KEEP)
    travel = _check_travel(travel)
    a = _as_plane(heightmap)
    H, W = a.shape
    origin = (int(origin[0]), int(origin[1]))
    src, flat = _check_sources(sources, H, W, origin)
    pen = _check_penalty(penalty, H, W)
    depth = acc = None
    if hydro is not None:
        if not isinstance(hydro, _hy.Hydrology) or hydro.depth is None or hydro.accumulation is None:
            raise ValueError("hydro must be a Hydrology that kept 'depth' and 'accumulation'")
        if tuple(hydro.shape) != (H, W):
            raise ValueError("heightmap %s and hydrology %s differ in size" % ((H, W), tuple(hydro.shape)))
        depth = np.ascontiguousarray(hydro.depth, np.float32)
        acc = np.ascontiguousarray(hydro.accumulation, np.uint32)
    tiled = DEFAULT_TILED if tiled is None else bool(tiled)
    n = H * W
    graph = 'territory' in keep or 'traffic' in keep
    dev = ops.dev
    out = {}
    with scratch(dev) as alloc:
        sizes = dict(h=4 * n, cost=4 * n, parent=n, ws=ops.route_workspace(H, W))
        for name, x in (('pen', pen), ('depth', depth), ('acc', acc)):
            if x is not None:
                sizes[name] = x.nbytes
        if graph:
            sizes.update(traffic=4 * n, basin=4 * n, hws=ops.hydrology_workspace(H, W))
        bufs = {name: alloc(nbytes) for name, nbytes in sizes.items()}
        for name, x in (('h', a), ('pen', pen), ('depth', depth), ('acc', acc)):
            if x is not None:
                dev.h2d(bufs[name], x)
        ops.route_weights(bufs['h'], H, W, W, travel.height_scale, travel.grade, travel.lake, travel.ford, travel.river_threshold,
                          travel.lake_min_depth, bufs['ws'], bufs.get('pen'), W, bufs.get('depth'), W, bufs.get('acc'), W)
        sweeps, _ = ops.route_relax(H, W, flat, tiled, bufs['cost'], W, bufs['ws'])
        ops.route_parents(bufs['cost'], W, H, W, bufs['parent'], W, bufs['ws'])
        if graph:
            ops.hydrology_accumulate(bufs['parent'], W, H, W, bufs['traffic'], W, bufs['basin'], W, bufs['hws'])
        dev.sync()
        want = [('cost', np.uint32, 'cost' in keep or graph), ('parent', np.int8, 'parent' in keep),
                ('traffic', np.uint32, graph), ('basin', np.int32, graph)]
        for name, dtype, wanted in want:
            if wanted:
                out[name] = np.empty((H, W), dtype)
                dev.d2h(out[name], bufs[name], out[name].nbytes)
    if graph:
        out['territory'], out['traffic'] = territory_traffic(out.pop('basin'), out['traffic'], out['cost'], flat)
    planes = {k: out[k] for k in keep}
    return CostField((H, W), src, origin, sweeps, tiled, **planes)


def paint(ops, texture, cost_field, paths=(), road=None, value_range=None):
    """Roads painted on a texture of the field's size with the hydrology's paint kernel.  paths: [n, 2] arrays of (row, col) as
    CostField.path returns them (the field's origin included), rasterised into a plane of ones; with road.traffic_threshold the
    field's ``traffic`` plane and that threshold are taken instead: the trail network that emerges towards the towns.  A pixel
    within road.width pixels of such a cell is blended towards road.colour.  texture, value_range and the result: as
    hydrology.paint's; untouched pixels keep their bits.  road: a Road (default Road())."""
    road = _check_road(road)
    if not isinstance(cost_field, CostField):
        raise ValueError("cost_field must be a CostField, got %r" % (cost_field,))
    H, W = cost_field.shape
    if road.traffic_threshold is not None:
        if cost_field.traffic is None:
            raise ValueError("road.traffic_threshold needs a CostField that kept 'traffic'")
        marks, threshold = cost_field.traffic, road.traffic_threshold
    else:
        marks, threshold = raster((H, W), paths, cost_field.origin), 1
    return _hy._paint(ops, texture, value_range, "cost field", (H, W), None, marks, threshold, road.width, road.colour,
                      road.opacity)                        # no lakes: a depth of zeros and a minimum depth of 0


# ---- command line -------------------------------------------------------------------------------------------------------
def parse_cell(text):
    m = re.fullmatch(r"\s*([+-]?\d+)\s*,\s*([+-]?\d+)\s*", text)
    if not m:
        raise argparse.ArgumentTypeError("a cell is R,C (two integers), got %r" % (text,))
    return int(m.group(1)), int(m.group(2))


def parse_args(argv):
    p = argparse.ArgumentParser(prog="python -m gan_heightmaps_amd.route",
                                description="Least-cost travel from a set of cells over a heightmap, and the roads (on the GPU).")
    p.add_argument("input", help="heightmap: 8-bit PNG (read as greyscale), or .npy (uint8 or float, (H, W))")
    p.add_argument("out_prefix", help="writes OUT_PREFIX.cost.npy, .parent.npy, .territory.npy, .traffic.npy and .path<i>.npy")
    p.add_argument("--from", dest="sources", type=parse_cell, action="append", metavar="R,C", required=True,
                   help="a source (a town); repeat for more")
    p.add_argument("--to", dest="targets", type=parse_cell, action="append", metavar="R,C", default=[],
                   help="a cell whose path to its source is written as OUT_PREFIX.path<i>.npy and painted; repeat for more")
    p.add_argument("--hydrology", action="store_true", help="fill the lakes first and route on the filled surface: lakes and "
                                                            "rivers cost --lake and --ford")
    p.add_argument("--texture", help="a texture of the heightmap's size to paint the roads on: PNG, or .npy")
    p.add_argument("--painted", help="the painted texture, as PNG (needs --texture)")
    r = Road()
    p.add_argument("--road-width", type=int, default=r.width, help="pixels a road is widened by, 0 .. %d" % MAX_RIVER_WIDTH)
    p.add_argument("--traffic-threshold", type=int, default=None,
                   help="paint every cell that at least this many cells travel through, instead of the --to paths")
    d = Travel()
    p.add_argument("--grade", type=float, default=d.grade, help="the grade at which a step costs twice its flat cost")
    p.add_argument("--lake", type=float, default=d.lake, help="penalty factor of lake cells (>= 1; inf: impassable)")
    p.add_argument("--ford", type=float, default=d.ford, help="penalty factor of river cells (>= 1)")
    p.add_argument("--river-threshold", type=int, default=d.river_threshold, help="cells of drainage area that make a river")
    p.add_argument("--lake-min-depth", type=float, default=d.lake_min_depth, help="filled depth above which a cell is a lake")
    p.add_argument("--height-scale", type=float, default=d.height_scale, help="cells of height per unit of the heightmap")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--plain", action="store_true", help="one Jacobi sweep per launch")
    g.add_argument("--tiled", action="store_true", help="tiles swept in LDS (the same bits)")
    a = p.parse_args(argv)
    if (a.texture is None) != (a.painted is None):
        p.error("--texture and --painted go together")
    if a.texture is None and (a.road_width != r.width or a.traffic_threshold is not None):
        p.error("--road-width / --traffic-threshold need --texture")
    try:
        a.travel = Travel(grade=a.grade, lake=a.lake, ford=a.ford, river_threshold=a.river_threshold,
                          lake_min_depth=a.lake_min_depth, height_scale=a.height_scale)
        a.road = Road(width=a.road_width, traffic_threshold=a.traffic_threshold)
    except ValueError as e:
        p.error(str(e))
    a.form = form_choice(a.tiled, a.plain)
    return a


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    from .device import Device, Ops
    x = read_image(a.input, "L", mmap=False)
    tex = read_image(a.texture, mmap=False) if a.texture else None
    dev = Device(0)
    try:
        ops = Ops(dev)
        hydro = _hy.analyse(ops, x, tiled=a.form) if a.hydrology else None
        cf = field(ops, x if hydro is None else hydro.filled, a.sources, a.travel, hydro=hydro, tiled=a.form)
        paths = cf.paths(a.targets)
        painted = paint(ops, tex, cf, paths, a.road) if tex is not None else None
    finally:
        dev.close()
    for k in KEEP:
        np.save("%s.%s.npy" % (a.out_prefix, k), getattr(cf, k))
    for i, path in enumerate(paths):
        np.save("%s.path%d.npy" % (a.out_prefix, i), path)
    if painted is not None:
        _hy._save_painted(a.painted, painted)
    return 0


if __name__ == "__main__":
    sys.exit(main())
