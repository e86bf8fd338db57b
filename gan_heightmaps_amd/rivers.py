"""Rivers: the stream network of a drainage as ordered reaches with their Strahler orders, Shreve magnitudes and main stems, traced
on the device (csrc/rivers.hip).  The hydrology says where the water is as planes; this says where the rivers are as
rivers: centre lines for a spline tool, confluences and mouths as places for towns, the blue lines of the contour sheet, "the main
river of this region and its tributaries, ranked".  Integers throughout, and equal to a definition in plain Python
(tests/rivers_ref.py) bit for bit.

The planes are a Hydrology's ``direction`` (int8, k = 0 .. 7 = N NE E SE S SW W NW, -1: the water leaves the plane) and
``accumulation`` (uint32).

1. A cell is a stream cell iff its accumulation reaches ``river_threshold``.  The stream cells that flow into a cell are its inflows;
   a stream cell is a mouth if its direction is -1, a source without inflows, a confluence with two or more.
2. A reach starts at every source and confluence that is no mouth and follows the receivers up to and including the first cell after
   its start that is a confluence or a mouth, its end: consecutive reaches share a vertex and the polylines join.  Reaches are
   numbered by their start's row W + col; ``downstream`` is the reach that starts at the end, or -1 at a mouth.  A stream cell that
   is source and mouth belongs to no reach: it is isolated.
3. On the host: a reach without an upstream reach has order 1 (Strahler 1957) and magnitude 1 (Shreve 1966); otherwise the order
   is the greatest order upstream, plus 1 if at least two upstream reaches have it, and the magnitude the sum of the upstream
   magnitudes.  Of the reaches that end in one cell the main one has the greatest (area, then lowest number); so has every reach
   that ends in a mouth.

    python -m gan_heightmaps_amd.rivers IN OUT.{svg,geojson,npz} [--river-threshold N] [--min-order N] [--lake-min-depth X]
        [--texture F --painted OUT [--width N] [--colour R,G,B] [--opacity X]] [--plain | --list]
"""
import argparse
import dataclasses
import sys

import numpy as np

from . import hydrology as _hy
from .planes import check_keep, check_size, scratch
from .util import is_int as _is_int, is_number as _number, read_image
from .viewshed import _check_colour, _check_opacity, _check_origin, _colour

__all__ = ["KEEP", "FORMS", "DEFAULT_FORM", "STREAM", "SOURCE", "CONFLUENCE", "MOUTH", "Network", "Rivers", "rivers", "report", "paint",
           "parse_args", "main"]

KEEP = ('kind',)
FORMS = ('plain', 'list')
# tools/rivers_bench.py, 4096 x 4096 value noise at a threshold of 256, one run on the MI355X, the forms alternated: the trace takes
# 1.06 ms plain and 0.49 ms list (at a threshold of 16: 1.28 and 1.12); DESIGN §4za has the line
DEFAULT_FORM = 'list'
STREAM, SOURCE, CONFLUENCE, MOUTH = 1, 2, 4, 8          # the bits of ``kind``; inflows = kind >> 4


@dataclasses.dataclass(frozen=True)
class Network:
    """Which rivers are reported, validated and frozen.  ``river_threshold``: the drainage area, in cells, at which a cell is a
    stream cell, an integer in [1, 2^32) (Water's); ``min_order``: reaches of a lower Strahler order are not reported, an integer in
    [1, 64]; ``lake_min_depth``: a vertex lies in a lake where the filled depth exceeds it, >= 0, in height units (Water's).  The
    defaults are chosen, not measured."""
    river_threshold: int = 256
    min_order: int = 1
    lake_min_depth: float = 1.0 / 512

    def __post_init__(self):
        if not _is_int(self.river_threshold) or not 1 <= self.river_threshold < 1 << 32:
            raise ValueError("river_threshold must be an integer in [1, 2^32), got %r" % (self.river_threshold,))
        if not _is_int(self.min_order) or not 1 <= self.min_order <= 64:
            raise ValueError("min_order must be an integer in [1, 64], got %r" % (self.min_order,))
        if not _number(self.lake_min_depth) or not 0 <= self.lake_min_depth < 3e38:
            raise ValueError("lake_min_depth must be a finite number >= 0, got %r" % (self.lake_min_depth,))
        object.__setattr__(self, "river_threshold", int(self.river_threshold))
        object.__setattr__(self, "min_order", int(self.min_order))
        object.__setattr__(self, "lake_min_depth", float(self.lake_min_depth))


def _check_network(network):
    network = Network() if network is None else network
    if not isinstance(network, Network):
        raise ValueError("network must be a Network, got %r" % (network,))
    return network


def _check_form(form):
    form = DEFAULT_FORM if form is None else form
    if form not in FORMS:
        raise ValueError("form must be one of %r or None, got %r" % (FORMS, form))
    return form


def _check_min_order(v):
    if not _is_int(v) or not 1 <= v <= 64:
        raise ValueError("min_order must be an integer in [1, 64], got %r" % (v,))
    return int(v)


class Rivers:
    """What ``rivers`` returns, R reaches with V vertices.  ``vertex`` int32 [V], row W + col inside the plane, reach by reach, each
    in downstream order; ``offsets`` int64 [R + 1]; ``points`` int64 [V, 2], (row, col) in ``origin``'s coordinates;
    ``downstream`` int32 [R], the reach that starts where this one ends, or -1 at a mouth; ``order`` (Strahler) and ``magnitude``
    (Shreve) int32 [R]; ``main`` uint8 [R], 1 for the main stem among the reaches that end together; ``area`` uint32 [R], the
    drainage area at the reach's last cell of its own; ``length`` float64 [R], in cells; ``height`` float32 [V], the filled height,
    and ``lake`` uint8 [V], 1 where the filled depth exceeds the network's ``lake_min_depth``, if the hydrology kept these planes,
    else None; ``sources_count``, ``confluences_count``, ``mouths_count`` and ``isolated``, the plane's, before ``min_order``;
    ``rounds``, the ranking's doubling rounds that moved a pointer; ``form``; ``network``; ``origin``; ``shape``; ``kind`` uint8
    [H, W] if kept."""

    def __init__(self, vertex, offsets, downstream, order, magnitude, main, area, network, origin, shape, height=None, lake=None,
                 sources_count=0, confluences_count=0, mouths_count=0, isolated=0, rounds=0, form=None, kind=None):
        self.vertex, self.offsets, self.downstream = vertex, offsets, downstream
        self.order, self.magnitude, self.main, self.area = order, magnitude, main, area
        self.network, self.form, self.kind, self.height, self.lake = network, form, kind, height, lake
        self.origin = (int(origin[0]), int(origin[1]))
        self.shape = (int(shape[0]), int(shape[1]))
        self.sources_count, self.confluences_count, self.mouths_count = int(sources_count), int(confluences_count), int(mouths_count)
        self.isolated, self.rounds = int(isolated), int(rounds)
        W = self.shape[1]
        v = vertex.astype(np.int64)
        self.points = np.stack([self.origin[0] + v // W, self.origin[1] + v % W], 1) if len(v) else np.zeros((0, 2), np.int64)
        # the steps of a reach: straight ones and diagonal ones, counted; one product and one sum
        # (the step from one reach's end to the next one's start lies in no reach's range)
        step = np.abs(np.diff(self.points, axis=0)).sum(1) if len(v) > 1 else np.zeros(0, np.int64)
        straight = np.concatenate([[0], np.cumsum(step == 1)]).astype(np.int64)
        diagonal = np.concatenate([[0], np.cumsum(step == 2)]).astype(np.int64)
        lo, hi = offsets[:-1], offsets[1:] - 1
        self.length = (straight[hi] - straight[lo]) + (diagonal[hi] - diagonal[lo]) * np.sqrt(2.0)

    def __len__(self):
        return int(self.downstream.shape[0])

    def __repr__(self):
        return "Rivers(%d x %d at %r, %d reaches of order up to %d)" % (
            self.shape + (self.origin, len(self), int(self.order.max()) if len(self) else 0))

    def _check(self, i):
        if not _is_int(i) or not 0 <= i < len(self):
            raise ValueError("reach %r: there are %d" % (i, len(self)))
        return int(i)

    def line(self, i):
        """reach i as int64 [n, 2], (row, col) in downstream order"""
        i = self._check(i)
        return self.points[self.offsets[i]:self.offsets[i + 1]]

    def lines(self, min_order=1):
        """[(reach number, its line)] of the reaches of at least this order"""
        min_order = _check_min_order(min_order)
        return [(i, self.line(i)) for i in range(len(self)) if self.order[i] >= min_order]

    def stem(self, i):
        """[i, its downstream reach, ...]: it ends at a mouth"""
        out = [self._check(i)]
        while self.downstream[out[-1]] >= 0:
            out.append(int(self.downstream[out[-1]]))
        return out

    def tributaries(self, i):
        """the reaches that end where reach i starts, ascending"""
        i = self._check(i)
        return [int(r) for r in np.flatnonzero(self.downstream == i)]

    def _cells(self, at):
        return [(int(r), int(c)) for r, c in self.points[at]]

    def sources(self):
        """the starts of the reaches without an upstream reach as [(row, col)]: ``sources`` for ``heightmap_routes``"""
        fed = np.zeros(len(self), bool)
        fed[self.downstream[self.downstream >= 0]] = True
        return self._cells(self.offsets[:-1][~fed])

    def confluences(self):
        """the distinct ends where a reach goes on as [(row, col)], in the order of their first reach"""
        seen, out = set(), []
        for p in self._cells((self.offsets[1:] - 1)[self.downstream >= 0]):
            if p not in seen:
                seen.add(p)
                out.append(p)
        return out

    def mouths(self):
        """the distinct ends where the water leaves the plane as [(row, col)], in the order of their first reach"""
        seen, out = set(), []
        for p in self._cells((self.offsets[1:] - 1)[self.downstream < 0]):
            if p not in seen:
                seen.add(p)
                out.append(p)
        return out

    def raster(self):
        """uint32 (H, W): the greatest order of the reaches through a cell, 0 where there is none"""
        m = np.zeros(self.shape[0] * self.shape[1], np.uint32)
        np.maximum.at(m, self.vertex, np.repeat(self.order.astype(np.uint32), np.diff(self.offsets)))
        return m.reshape(self.shape)

    # ---- writers ----------------------------------------------------------------------------------------------------------
    def features(self):
        """the GeoJSON LineString features, coordinates [col, row]"""
        out = []
        for i in range(len(self)):
            out.append({"type": "Feature", "geometry": {"type": "LineString", "coordinates": [[int(c), int(r)] for r, c in self.line(i)]},
                        "properties": {"order": int(self.order[i]), "magnitude": int(self.magnitude[i]), "main": bool(self.main[i]),
                                       "area": int(self.area[i]), "length": float(self.length[i]), "downstream": int(self.downstream[i])}})
        return out

    def _svg_paths(self):
        out = []
        for i in range(len(self)):
            d = "M" + " L".join("%d %d" % (c, r) for r, c in self.line(i))
            out.append('<path class="river" data-order="%d" fill="none" stroke="#22497a" stroke-linecap="round" stroke-width="%s" d="%s"/>' % (
                int(self.order[i]), repr(0.25 + 0.25 * int(self.order[i])), d))
        return "".join(line + "\n" for line in out)

    def save(self, path):
        """.npz: the arrays, origin, shape and the network; .svg: one <path class="river" data-order=...> per reach in pixel
        coordinates (x = col, y = row) with a stroke width that grows with the order; .geojson: LineString features with ``order``,
        ``magnitude``, ``main``, ``area``, ``length`` and ``downstream`` properties, coordinates [col, row]"""
        low = path.lower()
        if low.endswith(".npz"):
            nw = self.network
            extra = {k: getattr(self, k) for k in ("height", "lake") if getattr(self, k) is not None}
            np.savez(path, vertex=self.vertex, offsets=self.offsets, points=self.points, downstream=self.downstream, order=self.order,
                     magnitude=self.magnitude, main=self.main, area=self.area, length=self.length,
                     origin=np.array(self.origin, np.int64), shape=np.array(self.shape, np.int64),
                     network=np.array([nw.river_threshold, nw.min_order, nw.lake_min_depth]), **extra)
        elif low.endswith(".svg"):
            H, W = self.shape
            with open(path, "w") as f:
                f.write('<svg xmlns="http://www.w3.org/2000/svg" viewBox="%d %d %d %d" fill="none">\n' % (
                    self.origin[1], self.origin[0], W - 1, H - 1) + self._svg_paths() + "</svg>\n")
        elif low.endswith(".geojson"):
            import json
            with open(path, "w") as f:
                json.dump({"type": "FeatureCollection", "features": self.features()}, f)
        else:
            raise ValueError("rivers are saved as .npz, .svg or .geojson, got %r" % (path,))


def _check_max_reaches(v):
    if not _is_int(v) or not 0 <= v < 1 << 31:
        raise ValueError("max_reaches must be an integer in [0, 2^31), got %r" % (v,))
    return int(v)


def reach_areas(vertex, offsets, downstream, direction, accumulation):
    """uint32 [R]: the accumulation at every reach's last cell of its own -- the end if that is a mouth with one inflow, which is an
    end of one reach alone, else the vertex before the end"""
    if len(downstream) == 0:
        return np.zeros(0, np.uint32)
    ends = vertex[offsets[1:] - 1]
    _, inverse, counts = np.unique(ends, return_inverse=True, return_counts=True)
    own = (direction.ravel()[ends] == -1) & (counts[inverse] == 1)
    return accumulation.ravel()[np.where(own, ends, vertex[offsets[1:] - 2])].astype(np.uint32)


def report(vertex, offsets, downstream, order, magnitude, main, area, network, origin, shape, filled=None, depth=None, **kw):
    """the Rivers of a plane from its reaches' arrays: the reaches below ``network.min_order`` dropped -- orders never fall
    downstream, so what is kept is closed downstream -- and ``downstream`` renumbered; the vertices' heights and lakes"""
    keep = np.flatnonzero(order >= network.min_order)
    if len(keep) != len(order):
        place = np.full(len(order) + 1, -1, np.int32)
        place[keep] = np.arange(len(keep), dtype=np.int32)
        n = np.diff(offsets)[keep]
        new = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
        take = np.repeat(offsets[:-1][keep] - new[:-1], n) + np.arange(new[-1])
        vertex, offsets, downstream = vertex[take], new, place[downstream[keep]]
        order, magnitude, main, area = order[keep], magnitude[keep], main[keep], area[keep]
    height = None if filled is None else np.ascontiguousarray(filled, np.float32).ravel()[vertex]
    lake = None if depth is None else (np.ascontiguousarray(depth, np.float32).ravel()[vertex] > np.float32(network.lake_min_depth)).astype(np.uint8)
    return Rivers(vertex, offsets, downstream, order, magnitude, main, area, network, origin, shape, height=height, lake=lake, **kw)


def rivers(ops, hydro, network=None, origin=(0, 0), form=None, max_reaches=1 << 24, keep=()):
    """The rivers of a drainage: upload, the count, the trace, the extraction, download, inside one scratch; then the orders on the
    host.  ops: a device.Ops; hydro: a hydrology.Hydrology that kept 'direction' and 'accumulation' ('filled' and 'depth' give the
    vertices' heights and lakes); network: a Network (default Network()); origin: the coordinates of cell [0, 0]; form: 'plain' or
    'list', the same bits (default DEFAULT_FORM); max_reaches: a plane with more reaches is refused with a ValueError that names their
    number, before the trace and before the extraction's arrays are allocated -- a condition, not a measurement; the default is
    chosen; keep: of 'kind'.  Returns a Rivers."""
    keep = check_keep(keep, KEEP)
    network = _check_network(network)
    origin = _check_origin(origin)
    form = _check_form(form)
    max_reaches = _check_max_reaches(max_reaches)
    if not isinstance(hydro, _hy.Hydrology) or hydro.direction is None or hydro.accumulation is None:
        raise ValueError("hydro must be a Hydrology that kept 'direction' and 'accumulation'")
    H, W = hydro.shape
    check_size(H, W, limits=True)
    direction = np.ascontiguousarray(hydro.direction, np.int8)
    acc = np.ascontiguousarray(hydro.accumulation, np.uint32)
    if direction.shape != (H, W) or acc.shape != (H, W):
        raise ValueError("the hydrology's planes must be %d x %d, got %s and %s" % (H, W, direction.shape, acc.shape))
    n = H * W
    kind = np.empty((H, W), np.uint8) if 'kind' in keep else None
    dev = ops.dev
    with scratch(dev) as alloc:
        d_dir, d_acc, d_kind, d_w = alloc(n), alloc(4 * n), alloc(n), alloc(ops.rivers_workspace(H, W))
        dev.h2d(d_dir, direction)
        dev.h2d(d_acc, acc)
        cells, R, sources, confluences, mouths, isolated = ops.rivers_count(d_dir, W, d_acc, W, H, W, network.river_threshold, d_kind, W,
                                                                             d_w)
        if R > max_reaches:
            raise ValueError("the plane of %d x %d has %d reaches, more than max_reaches = %d: raise river_threshold, or max_reaches" % (
                H, W, R, max_reaches))
        d_l = alloc(max(ops.rivers_list_bytes(cells), 16)) if form == 'list' else None
        V, rounds = ops.rivers_trace(d_dir, W, d_kind, W, H, W, FORMS.index(form), d_w, d_l, cells, R)
        out = (np.empty(V, np.int32), np.empty(R + 1, np.int64), np.empty(R, np.int32))
        ptrs = [alloc(max(x.nbytes, 16)) for x in out]
        ops.rivers_extract(d_dir, W, d_kind, W, H, W, d_w, d_l, cells, R, V, *ptrs)
        dev.sync()
        for x, p in zip(out, ptrs):
            if x.nbytes:
                dev.d2h(x, p, x.nbytes)
        if kind is not None:
            dev.d2h(kind, d_kind, kind.nbytes)
    vertex, offsets, downstream = out
    area = reach_areas(vertex, offsets, downstream, direction, acc)
    order, magnitude, main = ops.rivers_order(downstream, area)
    return report(vertex, offsets, downstream, order, magnitude, main, area, network, origin, (H, W), filled=hydro.filled,
                  depth=hydro.depth, sources_count=sources, confluences_count=confluences, mouths_count=mouths, isolated=isolated,
                  rounds=rounds, form=form, kind=kind)


def _check_width(width):
    if not _is_int(width) or not 0 <= width <= _hy.MAX_RIVER_WIDTH:
        raise ValueError("width must be an integer in [0, %d], got %r" % (_hy.MAX_RIVER_WIDTH, width))
    return int(width)


def paint(ops, texture, rivers, min_order=1, width=0, colour=_hy.Water().colour, opacity=0.85, value_range=None):
    """The reaches of a Rivers of at least ``min_order`` painted on a texture of its plane's size with the hydrology's paint kernel:
    a pixel within ``width`` pixels (0 .. 4) of such a reach is blended towards ``colour`` (three numbers in [0, 1]) with
    ``opacity``.  texture, value_range and the result: as hydrology.paint's; unpainted pixels keep their bits."""
    if not isinstance(rivers, Rivers):
        raise ValueError("rivers must be a Rivers, got %r" % (rivers,))
    min_order, width = _check_min_order(min_order), _check_width(width)
    colour, opacity = _check_colour(colour), _check_opacity(opacity)
    return _hy._paint(ops, texture, value_range, "rivers", rivers.shape, None, rivers.raster(), min_order, width, colour, opacity)


# ---- command line -------------------------------------------------------------------------------------------------------
def add_network_arguments(p):
    d = Network()
    p.add_argument("--river-threshold", type=int, default=d.river_threshold, metavar="N",
                   help="cells of drainage area at which a cell is a stream cell (default %d)" % d.river_threshold)
    p.add_argument("--min-order", type=int, default=d.min_order, metavar="N",
                   help="reaches of a lower Strahler order are dropped (default %d)" % d.min_order)


def parse_args(argv):
    p = argparse.ArgumentParser(prog="python -m gan_heightmaps_amd.rivers",
                                description="The rivers of a heightmap: ordered reaches with Strahler orders (on the GPU).")
    p.add_argument("input", help="heightmap: 8-bit PNG (read as greyscale), or .npy (uint8 or float, (H, W))")
    p.add_argument("output", help="the rivers: .svg, .geojson or .npz")
    add_network_arguments(p)
    p.add_argument("--lake-min-depth", type=float, default=Network().lake_min_depth, metavar="X",
                   help="filled depth above which a vertex lies in a lake")
    p.add_argument("--texture", default=None, metavar="F", help="a texture of the heightmap's size, what --painted draws the rivers on")
    p.add_argument("--painted", default=None, metavar="OUT", help="where the texture with the rivers painted on goes (PNG)")
    p.add_argument("--width", type=int, default=0, metavar="N", help="pixels around a reach that are painted (0 .. 4)")
    p.add_argument("--colour", type=_colour, default=_hy.Water().colour, metavar="R,G,B", help="the paint's colour, in [0, 1]")
    p.add_argument("--opacity", type=float, default=0.85, metavar="X", help="the paint's opacity, in [0, 1]")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--plain", dest="form", action="store_const", const="plain", default=None, help="every round sweeps the plane")
    g.add_argument("--list", dest="form", action="store_const", const="list", help="the rounds run over a list of the stream cells")
    a = p.parse_args(argv)
    if (a.painted is None) != (a.texture is None):
        p.error("--painted and --texture go together")
    if not a.output.lower().endswith((".svg", ".geojson", ".npz")):
        p.error("the output is .svg, .geojson or .npz")
    try:
        a.network = Network(a.river_threshold, a.min_order, a.lake_min_depth)
        _check_colour(a.colour)
        _check_width(a.width)
        _check_opacity(a.opacity)
    except ValueError as e:
        p.error(str(e))
    return a


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    from .device import Device, Ops
    x = read_image(a.input, "L", mmap=False)
    texture = None if a.texture is None else read_image(a.texture, mmap=False)
    dev = Device(0)
    try:
        ops = Ops(dev)
        got = rivers(ops, _hy.analyse(ops, x), a.network, form=a.form)
        painted = None if a.painted is None else paint(ops, texture, got, 1, a.width, a.colour, a.opacity)
    finally:
        dev.close()
    got.save(a.output)
    if painted is not None:
        _hy._save_painted(a.painted, painted)
    print("%d reaches of order up to %d, %d rounds" % (len(got), int(got.order.max()) if len(got) else 0, got.rounds))
    return 0


if __name__ == "__main__":
    sys.exit(main())
