"""Regions: lakes, basins and territories as polygons with holes, labelled and traced on the device (csrc/regions.hip).
The other terrain tools say what is where as planes, points (peaks) and lines (contours, rivers); this says which areas there are
as areas: an outer ring and its holes, in order, with the number of cells -- a GIS layer, an engine's water or zone volume, the
filled lakes of an SVG sheet.  Integers throughout, and equal to a definition in plain Python (tests/regions_ref.py) bit for bit.

The plane is a label plane: int32 (H, W), a negative label means "no region".  ``lakes``, ``basins``, ``territories``, ``covered``,
``land``, ``bands`` and ``biomes`` make one on the host from what the other tools return.

1. Two cells belong together when they are 4-neighbours with equal non-negative labels.  A polygon is such a component; polygons are
   numbered in the order of their least cell (row W + col), the seed.
2. The boundary of a polygon follows the cracks between cells, clockwise on screen (rows down) with the polygon on its right, and
   turns right first where it has a choice: two cells of a region that touch only at a corner are kept apart there, and two holes
   that touch only at a corner form one ring that passes that corner twice.  Rings may touch themselves at a corner and never cross.
3. A ring's vertices are grid corners (row, col) -- cell (r, c) covers [r, r + 1] x [c, c + 1] -- where the boundary turns;
   collinear corners are never emitted.  A polygon has exactly one outer ring, of positive shoelace area in (x = col, y = row); every
   other ring is a hole, of negative area; the areas sum to the polygon's cells.

    python -m gan_heightmaps_amd.regions IN OUT.{geojson,svg,npz} (--lakes | --basins | --land SEA | --bands [--interval X --base X] |
        --labels) [--min-cells N] [--no-holes] [--texture F --painted OUT [--colour R,G,B] [--opacity X] [--outline]] [--sweep | --union]
"""
import argparse
import dataclasses
import sys

import numpy as np

from . import hydrology as _hy
from .planes import as_plane, check_keep, check_size, scratch
from .util import is_int as _is_int, is_number as _number, read_image
from .viewshed import _check_colour, _check_opacity, _check_origin, _colour

__all__ = ["KEEP", "FORMS", "DEFAULT_FORM", "Areas", "Regions", "regions", "report", "paint", "lakes", "basins", "territories", "covered",
           "land", "bands", "biomes", "parse_args", "main"]

KEEP = ('polygon',)
FORMS = ('sweep', 'union')
# tools/regions_bench.py, 4096 x 4096 value noise as bands of the default levels, one run on the MI355X, the forms alternated: the
# labelling takes 19.95 ms sweep (105 sweeps) and 2.66 ms union (as land: 7.49 and 1.92); DESIGN §4zb has the line
DEFAULT_FORM = 'union'
MAX_EDGES = (1 << 31) - 1


@dataclasses.dataclass(frozen=True)
class Areas:
    """Which polygons are reported, validated and frozen.  ``min_cells``: polygons of fewer cells are not reported, an integer in
    [1, 2^31); ``holes``: False drops every hole ring, so that a polygon is its outer ring alone.  The defaults are chosen, not
    measured."""
    min_cells: int = 1
    holes: bool = True

    def __post_init__(self):
        if not _is_int(self.min_cells) or not 1 <= self.min_cells < 1 << 31:
            raise ValueError("min_cells must be an integer in [1, 2^31), got %r" % (self.min_cells,))
        if not isinstance(self.holes, (bool, np.bool_)):
            raise ValueError("holes must be True or False, got %r" % (self.holes,))
        object.__setattr__(self, "min_cells", int(self.min_cells))
        object.__setattr__(self, "holes", bool(self.holes))


def _check_areas(areas):
    areas = Areas() if areas is None else areas
    if not isinstance(areas, Areas):
        raise ValueError("areas must be an Areas, got %r" % (areas,))
    return areas


def _check_form(form):
    form = DEFAULT_FORM if form is None else form
    if not isinstance(form, str) or form not in FORMS:
        raise ValueError("form must be one of %r or None, got %r" % (FORMS, form))
    return form


def _check_max_edges(v):
    if v is None:
        return MAX_EDGES
    if not _is_int(v) or not 0 <= v < 1 << 31:
        raise ValueError("max_edges must be None or an integer in [0, 2^31), got %r" % (v,))
    return int(v)


def _check_labels(labels):
    a = labels if hasattr(labels, "dtype") and hasattr(labels, "shape") else np.asarray(labels)
    if a.ndim != 2 or a.dtype.kind not in "iu" or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("labels must be an integer plane (H, W), got %s %s" % (getattr(a, "dtype", None), tuple(a.shape)))
    H, W = a.shape
    check_size(H, W, limits=True)
    if (H + 1) * (W + 1) >= 1 << 31:
        raise ValueError("a label plane of %d x %d has 2^31 grid corners or more" % (H, W))
    if a.dtype != np.int32:
        if a.size and (int(a.max()) > 0x7fffffff or int(a.min()) < -0x80000000):
            raise ValueError("labels must fit int32")
        a = a.astype(np.int32)
    return np.ascontiguousarray(a)


class Regions:
    """What ``regions`` returns, P polygons with R rings of V vertices.  ``vertex`` int32 [V], grid corners row (W + 1) + col inside
    the plane, ring by ring, each clockwise on screen from its cut; ``ring_offsets`` int64 [R + 1]; ``points`` int64 [V, 2],
    (row, col) in ``origin``'s coordinates; ``ring_polygon`` int32 [R]; ``hole`` uint8 [R], 0 for a polygon's one outer ring;
    ``seed`` int32 [P], the polygon's least cell, row W + col; ``label`` int32 [P]; ``cells`` uint32 [P]; ``bbox`` int64 [P, 4],
    (row0, col0, row1, col1) of the outer ring's corners in ``origin``'s coordinates; ``perimeter`` int64 [P], the length of the
    polygon's rings in cell sides, the reported holes included; ``rounds``, the ranking's doubling rounds that moved a pointer;
    ``sweeps``, the labelling's; ``form``; ``areas``; ``origin``; ``shape``; ``polygon_plane`` int32 [H, W] if 'polygon' was kept:
    the polygon of every cell, -1 for none or for one that ``areas`` dropped."""

    def __init__(self, vertex, ring_offsets, ring_polygon, hole, seed, label, cells, areas, origin, shape, rounds=0, sweeps=0, form=None,
                 polygon_plane=None):
        self.vertex, self.ring_offsets, self.ring_polygon, self.hole = vertex, ring_offsets, ring_polygon, hole
        self.seed, self.label, self.cells = seed, label, cells
        self.areas, self.form, self.polygon_plane = areas, form, polygon_plane
        self.origin = (int(origin[0]), int(origin[1]))
        self.shape = (int(shape[0]), int(shape[1]))
        self.rounds, self.sweeps = int(rounds), int(sweeps)
        W1 = self.shape[1] + 1
        v = vertex.astype(np.int64)
        self.points = np.stack([self.origin[0] + v // W1, self.origin[1] + v % W1], 1) if len(v) else np.zeros((0, 2), np.int64)
        P, R = len(seed), len(ring_polygon)
        # a ring's length: the steps between its vertices and from the last back to the first, all along one axis
        self.bbox, self.perimeter = np.zeros((P, 4), np.int64), np.zeros(P, np.int64)
        if R:                                    # (every ring has four vertices at least, so no segment of a reduceat is empty)
            lo = ring_offsets[:-1]
            after = np.arange(len(v)) + 1
            after[ring_offsets[1:] - 1] = lo     # the vertex after a ring's last is its first
            length = np.add.reduceat(np.abs(self.points - self.points[after]).sum(1), lo)
            np.add.at(self.perimeter, ring_polygon, length)
            outer = hole == 0
            box = np.concatenate([np.minimum.reduceat(self.points, lo), np.maximum.reduceat(self.points, lo)], 1)
            self.bbox[ring_polygon[outer]] = box[outer]
        order = np.lexsort((np.arange(R), hole, ring_polygon)) if R else np.zeros(0, np.int64)      # per polygon: the outer ring, then its holes
        self._rings = order.astype(np.int64)
        self._first = np.searchsorted(ring_polygon[order], np.arange(P + 1)) if R else np.zeros(P + 1, np.int64)

    def __len__(self):
        return int(self.seed.shape[0])

    def __repr__(self):
        return "Regions(%d x %d at %r, %d polygons with %d holes, %d vertices)" % (
            self.shape + (self.origin, len(self), int(self.hole.sum()), len(self.vertex)))

    def _check(self, p):
        if not _is_int(p) or not 0 <= p < len(self):
            raise ValueError("polygon %r: there are %d" % (p, len(self)))
        return int(p)

    def ring(self, k):
        """ring k as int64 [n, 2], (row, col) corners clockwise on screen; the last joins the first"""
        if not _is_int(k) or not 0 <= k < len(self.ring_polygon):
            raise ValueError("ring %r: there are %d" % (k, len(self.ring_polygon)))
        return self.points[self.ring_offsets[k]:self.ring_offsets[k + 1]]

    def rings_of(self, p):
        """the rings of polygon p: the outer ring first, then the holes by their least edge"""
        p = self._check(p)
        return [int(k) for k in self._rings[self._first[p]:self._first[p + 1]]]

    def polygon(self, p):
        """polygon p as a list of int64 [n, 2] rings: the outer ring, then the holes"""
        return [self.ring(k) for k in self.rings_of(p)]

    def at(self, row, col):
        """the polygon of the cell (row, col) in ``origin``'s coordinates, -1 for none; needs keep=('polygon',)"""
        if self.polygon_plane is None:
            raise ValueError("at() needs the polygon plane: keep=('polygon',)")
        r, c = row - self.origin[0], col - self.origin[1]
        if not (_is_int(row) and _is_int(col) and 0 <= r < self.shape[0] and 0 <= c < self.shape[1]):
            raise ValueError("cell %r lies outside the plane %d x %d at %r" % (((row, col),) + self.shape + (self.origin,)))
        return int(self.polygon_plane[r, c])

    def largest(self, n=1):
        """the numbers of the n polygons with the most cells, the greatest first, the lower number first among equals"""
        if not _is_int(n) or n < 0:
            raise ValueError("n must be an integer >= 0, got %r" % (n,))
        return [int(p) for p in np.lexsort((np.arange(len(self)), -self.cells.astype(np.int64)))[:n]]

    def raster(self, outline=False):
        """uint32 (H, W) marks: 1 on the cells inside the reported rings (winding numbers summed over the rings, so a dropped
        hole is filled and nested polygons add up); outline: 1 only on the polygons' cells along a ring"""
        H, W = self.shape
        if outline:
            m = np.zeros((H, W), np.uint32)
        else:
            toggles = np.zeros((H, W + 1), np.int64)
        y0, x0 = self.origin
        for k in range(len(self.ring_polygon)):
            pts = self.ring(k)
            for (r0, c0), (r1, c1) in zip(pts, np.roll(pts, -1, axis=0)):
                r0, c0, r1, c1 = int(r0) - y0, int(c0) - x0, int(r1) - y0, int(c1) - x0
                if outline:                      # the polygon lies on the right of its ring
                    if r0 == r1:
                        m[(r0 if c1 > c0 else r0 - 1), min(c0, c1):max(c0, c1)] = 1
                    else:
                        m[min(r0, r1):max(r0, r1), (c0 - 1 if r1 > r0 else c0)] = 1
                elif c0 == c1:                   # northwards on the polygon's left, southwards on its right
                    toggles[min(r0, r1):max(r0, r1), c0] += 1 if r1 < r0 else -1
        if outline:
            return m
        return (np.cumsum(toggles, axis=1)[:, :W] > 0).astype(np.uint32)

    # ---- writers ----------------------------------------------------------------------------------------------------------
    def features(self):
        """the GeoJSON Polygon features, coordinates [col, row], every ring closed by its first point"""
        out = []
        for p in range(len(self)):
            rings = [[[int(c), int(r)] for r, c in ring] for ring in self.polygon(p)]
            out.append({"type": "Feature", "geometry": {"type": "Polygon", "coordinates": [ring + ring[:1] for ring in rings]},
                        "properties": {"label": int(self.label[p]), "cells": int(self.cells[p]), "holes": len(rings) - 1}})
        return out

    def _svg_paths(self):
        out = []
        for p in range(len(self)):
            d = " ".join("M" + " L".join("%d %d" % (c, r) for r, c in ring) + " Z" for ring in self.polygon(p))
            out.append('<path class="region" data-label="%d" data-cells="%d" fill="#7fa8c9" fill-opacity="0.6" fill-rule="evenodd" '
                       'stroke="none" d="%s"/>' % (int(self.label[p]), int(self.cells[p]), d))
        return "".join(line + "\n" for line in out)

    def save(self, path, texture=None):
        """.npz: the arrays, origin, shape and the areas; .svg: one even-odd <path class="region"> per polygon in corner
        coordinates (x = col, y = row), ``texture`` (uint8 (H, W) or (H, W, 3)) embedded as a PNG if given; .geojson: Polygon
        features with ``label``, ``cells`` and ``holes`` properties, coordinates [col, row]"""
        low = path.lower()
        if low.endswith(".npz"):
            extra = {} if self.polygon_plane is None else {"polygon_plane": self.polygon_plane}
            np.savez(path, vertex=self.vertex, ring_offsets=self.ring_offsets, points=self.points, ring_polygon=self.ring_polygon,
                     hole=self.hole, seed=self.seed, label=self.label, cells=self.cells, bbox=self.bbox, perimeter=self.perimeter,
                     origin=np.array(self.origin, np.int64), shape=np.array(self.shape, np.int64),
                     areas=np.array([self.areas.min_cells, int(self.areas.holes)], np.int64), **extra)
        elif low.endswith(".svg"):
            H, W = self.shape
            head = '<svg xmlns="http://www.w3.org/2000/svg" xmlns:xlink="http://www.w3.org/1999/xlink" viewBox="%d %d %d %d">\n' % (
                self.origin[1], self.origin[0], W, H)
            with open(path, "w") as f:
                f.write(head + self._svg_image(texture) + self._svg_paths() + "</svg>\n")
        elif low.endswith(".geojson"):
            import json
            with open(path, "w") as f:
                json.dump({"type": "FeatureCollection", "features": self.features()}, f)
        else:
            raise ValueError("regions are saved as .npz, .svg or .geojson, got %r" % (path,))

    def _svg_image(self, texture):
        if texture is None:
            return ""
        import base64
        import io
        from PIL import Image
        H, W = self.shape
        tex = np.ascontiguousarray(texture)
        if tex.dtype != np.uint8 or tex.shape[:2] != (H, W):
            raise ValueError("the texture must be uint8 of the regions' size %s, got %s %s" % ((H, W), tex.dtype, tex.shape))
        buf = io.BytesIO()
        Image.fromarray(tex[:, :, 0] if tex.ndim == 3 and tex.shape[2] == 1 else tex).save(buf, format="PNG")
        # corners are the coordinates: cell (r, c) covers [r, r + 1] x [c, c + 1]
        return '<image x="%d" y="%d" width="%d" height="%d" preserveAspectRatio="none" xlink:href="data:image/png;base64,%s"/>\n' % (
            self.origin[1], self.origin[0], W, H, base64.b64encode(buf.getvalue()).decode("ascii"))


def report(vertex, ring_offsets, ring_polygon, ring_hole, seed, label, cells, areas, origin, shape, polygon_plane=None, **kw):
    """the Regions of a plane from the device's arrays: the polygons below ``areas.min_cells`` dropped with their rings and the
    rest renumbered, the hole rings dropped unless ``areas.holes``"""
    keep_p = cells >= areas.min_cells
    keep_r = keep_p[ring_polygon] & ((ring_hole == 0) | areas.holes) if len(ring_polygon) else np.zeros(0, bool)
    if not keep_p.all() or not keep_r.all():
        place = np.full(len(seed) + 1, -1, np.int32)
        place[np.flatnonzero(keep_p)] = np.arange(int(keep_p.sum()), dtype=np.int32)
        rings = np.flatnonzero(keep_r)
        n = np.diff(ring_offsets)[rings]
        new = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
        take = np.repeat(ring_offsets[:-1][rings] - new[:-1], n) + np.arange(new[-1])
        vertex, ring_offsets = vertex[take], new
        ring_polygon, ring_hole = place[ring_polygon[rings]], ring_hole[rings]
        seed, label, cells = seed[keep_p], label[keep_p], cells[keep_p]
        if polygon_plane is not None:
            polygon_plane = place[polygon_plane]                  # -1 reads the last entry, which is -1
    return Regions(vertex, ring_offsets, ring_polygon, ring_hole, seed, label, cells, areas, origin, shape, polygon_plane=polygon_plane, **kw)


def _empty(areas, origin, shape, form, polygon_plane):
    z = np.zeros
    return Regions(z(0, np.int32), z(1, np.int64), z(0, np.int32), z(0, np.uint8), z(0, np.int32), z(0, np.int32), z(0, np.uint32), areas,
                   origin, shape, rounds=0, sweeps=0, form=form, polygon_plane=polygon_plane)


def regions(ops, labels, areas=None, origin=(0, 0), form=None, keep=(), max_edges=None):
    """The polygons of a label plane: upload, the labelling, the count, the trace, the extraction, download, inside one scratch.
    ops: a device.Ops; labels: an integer plane (H, W), negative for "no region"; areas: an Areas (default Areas()); origin: the
    coordinates of cell [0, 0]; form: 'sweep' or 'union', the labelling's two forms, the same bits (default DEFAULT_FORM);
    keep: of 'polygon', the polygon of every cell; max_edges: a plane with more boundary edges is refused by the count, before the
    per-edge buffers are allocated (None: no limit below 2^31).  A plane without a region costs the labelling alone.  Returns a
    Regions."""
    keep = check_keep(keep, KEEP)
    areas = _check_areas(areas)
    origin = _check_origin(origin)
    form = _check_form(form)
    max_edges = _check_max_edges(max_edges)
    labels = _check_labels(labels)
    H, W = labels.shape
    n = H * W
    plane = np.empty((H, W), np.int32) if 'polygon' in keep else None
    dev = ops.dev
    with scratch(dev) as alloc:
        d_l, d_c, d_w = alloc(4 * n), alloc(4 * n), alloc(ops.regions_workspace(H, W))
        dev.h2d(d_l, labels)
        sweeps = ops.regions_label(d_l, W, H, W, FORMS.index(form), d_c, W, d_w)
        if sweeps == 0:
            if plane is not None:
                plane[:] = -1
            return _empty(areas, origin, (H, W), form, plane)
        E, P = ops.regions_count(d_l, W, d_c, W, H, W, d_w, max_edges)
        d_t = alloc(max(ops.regions_trace_bytes(E), 16))
        R, V, rounds = ops.regions_trace(H, W, d_w, d_t, E, P)
        out = (np.empty(V, np.int32), np.empty(R + 1, np.int64), np.empty(R, np.int32), np.empty(R, np.uint8), np.empty(P, np.int32),
               np.empty(P, np.int32), np.empty(P, np.uint32))
        ptrs = [alloc(max(x.nbytes, 16)) for x in out]
        d_p = alloc(4 * n) if plane is not None else None
        ops.regions_extract(d_l, W, d_c, W, H, W, d_w, d_t, E, P, R, V, *ptrs, d_p, W)
        dev.sync()
        for x, p in zip(out, ptrs):
            if x.nbytes:
                dev.d2h(x, p, x.nbytes)
        if plane is not None:
            dev.d2h(plane, d_p, plane.nbytes)
    return report(*out, areas, origin, (H, W), polygon_plane=plane, rounds=rounds, sweeps=sweeps, form=form)


def paint(ops, texture, regions, colour=_hy.Water().colour, opacity=0.6, outline=False, value_range=None):
    """The polygons of a Regions painted on a texture of its plane's size with the hydrology's paint kernel: a pixel of a reported
    polygon -- ``outline``: of its cells along a ring -- is blended towards ``colour`` (three numbers in [0, 1]) with ``opacity``.
    texture, value_range and the result: as hydrology.paint's; unpainted pixels keep their bits."""
    if not isinstance(regions, Regions):
        raise ValueError("regions must be a Regions, got %r" % (regions,))
    colour, opacity = _check_colour(colour), _check_opacity(opacity)
    if not isinstance(outline, (bool, np.bool_)):
        raise ValueError("outline must be True or False, got %r" % (outline,))
    return _hy._paint(ops, texture, value_range, "regions", regions.shape, None, regions.raster(bool(outline)), 1, 0, colour, opacity)


# ---- label planes, made on the host ---------------------------------------------------------------------------------------
def _quantise(heightmap, height_scale):
    """the viewshed's quantisation: zq = int32(rint(h float32(height_scale 256))), one float32 product, rounded once"""
    if not _number(height_scale) or not 0 < height_scale <= 65536:
        raise ValueError("height_scale must be a number in (0, 65536], got %r" % (height_scale,))
    h = as_plane(heightmap, lead=True, unit_range=True, raw=True)
    return np.rint(h * np.float32(float(height_scale) * 256.0)).astype(np.int32)


def lakes(hydro, lake_min_depth=1.0 / 512):
    """0 where the filled depth of a Hydrology that kept 'depth' exceeds lake_min_depth, -1 elsewhere: a polygon per lake, its
    islands as holes"""
    if not isinstance(hydro, _hy.Hydrology) or hydro.depth is None:
        raise ValueError("hydro must be a Hydrology that kept 'depth'")
    if not _number(lake_min_depth) or not 0 <= lake_min_depth < 3e38:
        raise ValueError("lake_min_depth must be a finite number >= 0, got %r" % (lake_min_depth,))
    return np.where(np.asarray(hydro.depth, np.float32) > np.float32(lake_min_depth), 0, -1).astype(np.int32)


def basins(hydro):
    """the outlet every cell drains to, of a Hydrology that kept 'basin': a polygon per catchment (or several, where one outlet's
    cells touch only at corners)"""
    if not isinstance(hydro, _hy.Hydrology) or hydro.basin is None:
        raise ValueError("hydro must be a Hydrology that kept 'basin'")
    return np.ascontiguousarray(hydro.basin, np.int32)


def territories(cost_field):
    """the source every cell travels to, of a route.CostField that kept 'territory'; an unreached cell is no region"""
    from .route import CostField
    if not isinstance(cost_field, CostField) or cost_field.territory is None:
        raise ValueError("cost_field must be a CostField that kept 'territory'")
    return np.ascontiguousarray(cost_field.territory, np.int32)


def covered(viewshed, hidden=False):
    """0 on the cells at least one observer of a viewshed.Viewshed sees, -1 elsewhere; hidden: the other way round"""
    from .viewshed import Viewshed
    if not isinstance(viewshed, Viewshed):
        raise ValueError("viewshed must be a Viewshed, got %r" % (viewshed,))
    if not isinstance(hidden, (bool, np.bool_)):
        raise ValueError("hidden must be True or False, got %r" % (hidden,))
    return np.where(viewshed.seen() != bool(hidden), 0, -1).astype(np.int32)


def land(heightmap, sea_level, height_scale=64.0):
    """0 where the heightmap (as_plane's: uint8 or float in [0, 1]) lies above sea_level (a number in [0, 1], in the heightmap's
    units), -1 in the sea; both quantised as the viewshed quantises heights"""
    if not _number(sea_level) or not 0 <= sea_level <= 1:
        raise ValueError("sea_level must be a number in [0, 1], got %r" % (sea_level,))
    zq = _quantise(heightmap, height_scale)
    sea_q = int(np.rint(np.float32(sea_level) * np.float32(float(height_scale) * 256.0)))
    return np.where(zq > sea_q, 0, -1).astype(np.int32)


def bands(heightmap, levels=None):
    """the number of a contour.Levels' levels that lie below each cell (level j at base + j interval, j in [0, count)): a polygon
    per elevation band, bounded by the lines ``contours`` draws for the same levels"""
    from .contour import _check_levels
    levels = _check_levels(levels)
    zq = _quantise(heightmap, levels.height_scale).astype(np.int64)
    below = np.maximum((zq - levels.base_q + levels.interval_q - 1) // levels.interval_q, 0)
    if levels.count is not None:
        below = np.minimum(below, levels.count)
    return below.astype(np.int32)


def biomes(climate):
    """the biome label of every land cell of a climate.Climate that kept 'biome', -1 in the sea: a polygon per patch of one biome,
    with ``Regions.label`` the chart's label"""
    from .climate import Climate
    if not isinstance(climate, Climate) or climate.biome is None:
        raise ValueError("climate must be a Climate that kept 'biome'")
    b = np.asarray(climate.biome, np.int32)
    return np.where(b == climate.biomes.ocean, -1, b).astype(np.int32)


# ---- command line -------------------------------------------------------------------------------------------------------
def add_area_arguments(p):
    d = Areas()
    p.add_argument("--min-cells", type=int, default=d.min_cells, metavar="N", help="polygons of fewer cells are dropped (default %d)" % d.min_cells)
    p.add_argument("--no-holes", dest="holes", action="store_false", help="drop the hole rings")


def parse_args(argv):
    from .contour import Levels
    p = argparse.ArgumentParser(prog="python -m gan_heightmaps_amd.regions",
                                description="The areas of a heightmap or a label plane as polygons with holes (on the GPU).")
    p.add_argument("input", help="heightmap: 8-bit PNG (read as greyscale) or .npy (uint8 or float, (H, W)); with --labels an integer .npy")
    p.add_argument("output", help="the polygons: .geojson, .svg or .npz")
    g = p.add_mutually_exclusive_group(required=True)
    g.add_argument("--lakes", dest="of", action="store_const", const="lakes", help="the filled lakes, islands as holes")
    g.add_argument("--basins", dest="of", action="store_const", const="basins", help="the catchments")
    g.add_argument("--land", dest="sea", type=float, default=None, metavar="SEA", help="land above this sea level, in [0, 1]")
    g.add_argument("--bands", dest="of", action="store_const", const="bands", help="the elevation bands between contour levels")
    g.add_argument("--labels", dest="of", action="store_const", const="labels", help="the input is a label plane")
    p.add_argument("--interval", type=float, default=None, metavar="X", help="--bands: cells of height between two levels")
    p.add_argument("--base", type=float, default=None, metavar="X", help="--bands: the height of level 0, in cells")
    add_area_arguments(p)
    p.add_argument("--texture", default=None, metavar="F", help="a texture of the plane's size, what --painted draws the polygons on")
    p.add_argument("--painted", default=None, metavar="OUT", help="where the texture with the polygons painted on goes (PNG)")
    p.add_argument("--colour", type=_colour, default=_hy.Water().colour, metavar="R,G,B", help="the paint's colour, in [0, 1]")
    p.add_argument("--opacity", type=float, default=0.6, metavar="X", help="the paint's opacity, in [0, 1]")
    p.add_argument("--outline", action="store_true", help="paint the polygons' cells along their rings only")
    f = p.add_mutually_exclusive_group()
    f.add_argument("--sweep", dest="form", action="store_const", const="sweep", default=None, help="label by tile sweeps")
    f.add_argument("--union", dest="form", action="store_const", const="union", help="label by a union-find")
    a = p.parse_args(argv)
    if a.sea is not None:
        a.of = "land"
    if (a.painted is None) != (a.texture is None):
        p.error("--painted and --texture go together")
    if a.outline and a.painted is None:
        p.error("--outline goes with --painted")
    if (a.interval is not None or a.base is not None) and a.of != "bands":
        p.error("--interval and --base go with --bands")
    if not a.output.lower().endswith((".svg", ".geojson", ".npz")):
        p.error("the output is .svg, .geojson or .npz")
    try:
        a.areas = Areas(a.min_cells, a.holes)
        d = Levels()
        a.levels = Levels(d.interval if a.interval is None else a.interval, d.base if a.base is None else a.base)
        _check_colour(a.colour)
        _check_opacity(a.opacity)
        if a.sea is not None and not 0 <= a.sea <= 1:
            raise ValueError("--land takes a sea level in [0, 1], got %r" % (a.sea,))
    except ValueError as e:
        p.error(str(e))
    return a


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    from .device import Device, Ops
    texture = None if a.texture is None else read_image(a.texture, mmap=False)
    x = np.load(a.input) if a.of == "labels" else read_image(a.input, "L", mmap=False)
    dev = Device(0)
    try:
        ops = Ops(dev)
        if a.of == "labels":
            labels = x
        elif a.of == "land":
            labels = land(x, a.sea)
        elif a.of == "bands":
            labels = bands(x, a.levels)
        else:
            hydro = _hy.analyse(ops, x)
            labels = lakes(hydro) if a.of == "lakes" else basins(hydro)
        got = regions(ops, labels, a.areas, form=a.form)
        painted = None if a.painted is None else paint(ops, texture, got, a.colour, a.opacity, a.outline)
    finally:
        dev.close()
    got.save(a.output)
    if painted is not None:
        _hy._save_painted(a.painted, painted)
    print("%d polygons with %d holes, %d vertices, %d rounds, %d sweeps" % (len(got), int(got.hole.sum()), len(got.vertex), got.rounds,
                                                                          got.sweeps))
    return 0


if __name__ == "__main__":
    sys.exit(main())
