"""Contours: the topographic isolines of a heightmap as ordered polylines, traced on the device (csrc/contour.hip).
The hydrology (§4t), the routes (§4u) and the viewshed (§4x) answer with planes; this is the first terrain tool whose answer is
vector geometry -- lines for an SVG sheet, a GeoJSON layer, an engine's spline tool, a coastline at a chosen sea level.
Integers throughout but for one IEEE double division per vertex, and equal to a definition in numpy and plain Python
(tests/contour_ref.py) bit for bit.

The plane is h[H, W], float32, finite and in [0, 1] (uint8 is read as v / 255).

1. The heights are the viewshed's: zq = int32(rint(h float32(height_scale 256))), in 1/256 cell.  The work is done on Z = 2 zq,
   which is even.
2. Level j is lam_j = 2 (base_q + j interval_q) + 1 with interval_q = rint(interval 256) and base_q = rint(base 256): odd, so no
   vertex of the grid ever lies on a level, every crossing is strictly inside a grid edge and no segment is degenerate.  Its
   nominal height is base + j interval; the line is drawn 1/512 cell above it.  ``count`` keeps the levels j in [0, count).
3. In a cell, a level between the least and the largest of its four corners gives one segment, or two at a saddle, which its
   centre resolves (the mean of the corners; a tie counts as below).  A vertex (r, c, axis, t) lies on the edge (r, c) - (r, c + 1)
   (axis 0, at (r, c + t)) or (r, c) - (r + 1, c) (axis 1, at (r + t, c)), t = double(lam - Z_first) / double(Z_second - Z_first).
   A segment runs from its entry to its exit vertex with the higher ground on a fixed side.
4. The successor of a segment is the segment of its level across its exit edge.  A segment without a predecessor starts an open
   line, from border to border; the others form closed loops, which start at their least segment.  Lines are ordered by their
   start segment's key (cell row, cell col, level, entry edge).

    python -m gan_heightmaps_amd.contour IN OUT.{svg,geojson,npz} [--interval X] [--base X] [--count N] [--index-every N]
        [--height-scale X] [--texture F [--painted OUT] [--colour R,G,B] [--opacity X]]
"""
import argparse
import dataclasses
import sys

import numpy as np

from . import hydrology as _hy
from .planes import as_plane, check_keep, scratch
from .util import is_int as _is_int, is_number as _number, read_image
from .viewshed import MAX_HEIGHT, _check_colour, _check_opacity, _check_origin, _colour, quantum

__all__ = ["KEEP", "MAX_HEIGHT", "Levels", "Contours", "contours", "marks", "paint", "parse_args", "main"]

KEEP = ('zq',)
SEGMENT = np.dtype([("level", np.int32), ("edge_p", np.int64, (3,)), ("t_p", np.float64), ("edge_q", np.int64, (3,)),
                    ("t_q", np.float64)])


@dataclasses.dataclass(frozen=True)
class Levels:
    """Which levels are drawn, validated and frozen.  ``interval``: cells of height between two levels, in (0, 65536], at least
    1/256 after rounding; ``base``: the nominal height of level 0 in cells, in [-65536, 65536]; ``count``: None for every level,
    or an integer >= 1 that keeps the levels j in [0, count) -- count=1 is a single isoline at ``base``, a coastline;
    ``index_every``: level j is an index contour iff j % index_every == 0; ``height_scale``: cells of height per unit of the
    heightmap, in (0, 65536].  Heights are kept to 1/256 cell.  The defaults are chosen, not measured."""
    interval: float = 4.0
    base: float = 0.0
    count: object = None
    index_every: int = 5
    height_scale: float = 64.0

    def __post_init__(self):
        if not _number(self.interval) or not 0 < self.interval <= MAX_HEIGHT or quantum(self.interval) < 1:
            raise ValueError("interval must be a number in [1/256, %g], got %r" % (MAX_HEIGHT, self.interval))
        object.__setattr__(self, "interval", float(self.interval))
        if not _number(self.base) or not -MAX_HEIGHT <= self.base <= MAX_HEIGHT:
            raise ValueError("base must be a number in [-%g, %g], got %r" % (MAX_HEIGHT, MAX_HEIGHT, self.base))
        object.__setattr__(self, "base", float(self.base))
        if self.count is not None:
            if not _is_int(self.count) or not 1 <= self.count <= 1 << 28:
                raise ValueError("count must be None or an integer in [1, 2^28], got %r" % (self.count,))
            object.__setattr__(self, "count", int(self.count))
        if not _is_int(self.index_every) or not 1 <= self.index_every < 1 << 31:
            raise ValueError("index_every must be an integer >= 1, got %r" % (self.index_every,))
        object.__setattr__(self, "index_every", int(self.index_every))
        if not _number(self.height_scale) or not 0 < self.height_scale <= MAX_HEIGHT:
            raise ValueError("height_scale must be a number in (0, %g], got %r" % (MAX_HEIGHT, self.height_scale))
        object.__setattr__(self, "height_scale", float(self.height_scale))

    @property
    def interval_q(self):
        return quantum(self.interval)

    @property
    def base_q(self):
        return quantum(self.base)

    def height(self, j):
        """the nominal height of level j, in cells"""
        return self.base + int(j) * self.interval

    def is_index(self, j):
        return int(j) % self.index_every == 0


def _check_levels(levels):
    levels = Levels() if levels is None else levels
    if not isinstance(levels, Levels):
        raise ValueError("levels must be a Levels, got %r" % (levels,))
    return levels


class Contours:
    """What ``contours`` returns.  ``edge`` int32 [V, 3], (r, c, axis) of every vertex in the plane's own coordinates; ``t`` float64
    [V]; ``offsets`` int64 [L + 1]: line i owns the vertices offsets[i] .. offsets[i + 1]; ``level`` int32 [L], its j; ``closed``
    uint8 [L]; ``levels``; ``origin``, the coordinates of cell [0, 0]; ``shape``; ``points`` float64 [V, 2], (row, col) in
    ``origin``'s coordinates; ``rounds``, the doubling rounds the ranking took; ``zq`` if it was kept."""

    def __init__(self, edge, t, offsets, level, closed, levels, origin, shape, rounds=0, zq=None):
        self.edge, self.t, self.offsets, self.level, self.closed = edge, t, offsets, level, closed
        self.levels, self.rounds, self.zq = levels, int(rounds), zq
        self.origin = (int(origin[0]), int(origin[1]))
        self.shape = (int(shape[0]), int(shape[1]))
        along = self.edge[:, 2].astype(bool)
        self.points = np.empty((len(self.t), 2), np.float64)
        self.points[:, 0] = (self.origin[0] + self.edge[:, 0].astype(np.int64)) + np.where(along, self.t, 0.0)
        self.points[:, 1] = (self.origin[1] + self.edge[:, 1].astype(np.int64)) + np.where(along, 0.0, self.t)

    def __len__(self):
        return int(self.level.shape[0])

    def __repr__(self):
        return "Contours(%d x %d at %r, %d lines, %d closed, %d vertices)" % (
            self.shape + (self.origin, len(self), int(self.closed.sum()), len(self.t)))

    def _check(self, i):
        if not _is_int(i) or not 0 <= i < len(self):
            raise ValueError("line %r: there are %d" % (i, len(self)))
        return int(i)

    def line(self, i):
        """float64 [n, 2]: the points of line i, (row, col); a closed one does not repeat its first point"""
        i = self._check(i)
        return self.points[int(self.offsets[i]):int(self.offsets[i + 1])]

    def height(self, i):
        """the nominal height of line i, in cells"""
        return self.levels.height(self.level[self._check(i)])

    def is_index(self, i):
        return self.levels.is_index(self.level[self._check(i)])

    def lines(self, level=None, index_only=False):
        """the numbers of the lines of level ``level`` (default: of every level); index_only: of the index contours alone"""
        keep = np.ones(len(self), bool)
        if level is not None:
            keep &= self.level == int(level)
        if index_only:
            keep &= self.level.astype(np.int64) % self.levels.index_every == 0
        return [int(i) for i in np.flatnonzero(keep)]

    def segments(self, within=None):
        """a structured array of (level, edge_p, t_p, edge_q, t_q), one row per segment, edges as (row, col, axis) in ``origin``'s
        coordinates, sorted: what two rectangles of one world agree on, bit for bit, in every cell both contain.  within:
        (y0, x0, h, w), a rectangle of pixels in ``origin``'s coordinates: only the segments of the cells inside it."""
        first, last = self.offsets[:-1], self.offsets[1:]
        n = last - first
        p = np.concatenate([np.arange(a, b - (0 if c else 1)) for a, b, c in zip(first, last, self.closed)] or [np.zeros(0, np.int64)])
        line = np.repeat(np.arange(len(self)), n - (1 - self.closed.astype(np.int64)))
        q = p + 1
        wrap = q == last[line]
        q[wrap] = first[line][wrap]
        out = np.empty(len(p), SEGMENT)
        world = self.edge.astype(np.int64) + np.array([self.origin[0], self.origin[1], 0], np.int64)
        out["level"], out["edge_p"], out["t_p"], out["edge_q"], out["t_q"] = self.level[line], world[p], self.t[p], world[q], self.t[q]
        if within is not None:
            y0, x0, h, w = (int(v) for v in within)
            ep, eq = out["edge_p"], out["edge_q"]
            row = np.where(ep[:, 2] == 1, ep[:, 0], np.where(eq[:, 2] == 1, eq[:, 0], np.minimum(ep[:, 0], eq[:, 0])))
            col = np.where(ep[:, 2] == 0, ep[:, 1], np.where(eq[:, 2] == 0, eq[:, 1], np.minimum(ep[:, 1], eq[:, 1])))
            out = out[(row >= y0) & (row < y0 + h - 1) & (col >= x0) & (col < x0 + w - 1)]
        keys = [out["t_q"]] + [out["edge_q"][:, k] for k in (2, 1, 0)] + [out["t_p"]] + [out["edge_p"][:, k] for k in (2, 1, 0)]
        return out[np.lexsort(keys + [out["level"]])]

    # ---- writers ----------------------------------------------------------------------------------------------------------
    def save(self, path, texture=None, peaks=None, rivers=None, regions=None):
        """.npz: the five arrays, origin, shape and the levels; .svg: one <path> per line in pixel coordinates (x = col, y = row),
        index contours in a heavier stroke, Z on the closed ones, ``texture`` (uint8 (H, W) or (H, W, 3)) embedded as a PNG if
        given; .geojson: LineString features with ``level``, ``height``, ``index`` and ``closed`` properties, coordinates
        [col, row], a closed line repeating its first point.  peaks: a peaks.Peaks of the same plane -- the sheet's spot heights:
        the .svg gains one <circle class="peak"> and one <text> with the height in cells per peak, the .geojson the peaks' Point
        features; without it both files are what they were.  rivers: a rivers.Rivers of the same plane -- the sheet's blue lines:
        the .svg gains one <path class="river"> per reach before the peaks' marks, the .geojson the reaches' LineString features
        after the contours' and before the peaks'; without it both files are what they were.  regions: a regions.Regions of the
        same plane -- the sheet's filled areas: the .svg gains one even-odd <path class="region"> per polygon beneath the lines
        (after the texture, before the first line), the .geojson the polygons' Polygon features in front of the contours';
        without it both files are what they were"""
        low = path.lower()
        if regions is not None:
            from .regions import Regions
            if not isinstance(regions, Regions) or regions.shape != self.shape or regions.origin != self.origin:
                raise ValueError("regions must be a Regions of the contours' plane, %d x %d at %r, got %r" % (self.shape + (self.origin, regions)))
            if low.endswith(".npz"):
                raise ValueError("an .npz holds the contours alone: save the regions on their own")
        if rivers is not None:
            from .rivers import Rivers
            if not isinstance(rivers, Rivers) or rivers.shape != self.shape or rivers.origin != self.origin:
                raise ValueError("rivers must be a Rivers of the contours' plane, %d x %d at %r, got %r" % (self.shape + (self.origin, rivers)))
            if low.endswith(".npz"):
                raise ValueError("an .npz holds the contours alone: save the rivers on their own")
        if peaks is not None:
            from .peaks import Peaks
            if not isinstance(peaks, Peaks) or peaks.shape != self.shape or peaks.origin != self.origin:
                raise ValueError("peaks must be a Peaks of the contours' plane, %d x %d at %r, got %r" % (self.shape + (self.origin, peaks)))
            if low.endswith(".npz"):
                raise ValueError("an .npz holds the contours alone: save the peaks on their own")
        if low.endswith(".npz"):
            lv = self.levels
            np.savez(path, edge=self.edge, t=self.t, offsets=self.offsets, level=self.level, closed=self.closed,
                     origin=np.array(self.origin, np.int64), shape=np.array(self.shape, np.int64),
                     levels=np.array([lv.interval, lv.base, -1 if lv.count is None else lv.count, lv.index_every, lv.height_scale]))
        elif low.endswith(".svg"):
            text = self._svg(texture)
            if regions is not None:
                # a cell's centre is its position on the sheet, so its corners lie half a cell before it
                at = text.index("\n", text.index("<image") if texture is not None else 0) + 1
                text = text[:at] + '<g transform="translate(-0.5 -0.5)">\n' + regions._svg_paths() + "</g>\n" + text[at:]
            if rivers is not None:
                text = text[:-len("</svg>\n")] + rivers._svg_paths() + "</svg>\n"
            if peaks is not None:
                text = text[:-len("</svg>\n")] + self._svg_peaks(peaks) + "</svg>\n"
            with open(path, "w") as f:
                f.write(text)
        elif low.endswith(".geojson"):
            import json
            doc = self._geojson()
            if regions is not None:
                doc["features"] = regions.features() + doc["features"]
            if rivers is not None:
                doc["features"] += rivers.features()
            if peaks is not None:
                doc["features"] += peaks.features()
            with open(path, "w") as f:
                json.dump(doc, f)
        else:
            raise ValueError("contours are saved as .npz, .svg or .geojson, got %r" % (path,))

    @staticmethod
    def _svg_peaks(peaks):
        out = []
        for (r, c), h in zip(peaks.cell, peaks.height):
            out.append('<circle class="peak" cx="%d" cy="%d" r="0.8" fill="#4d2e12" stroke="none"/>' % (c, r))
            out.append('<text class="peak" x="%s" y="%s" font-size="3" fill="#4d2e12" stroke="none">%s</text>' % (
                repr(int(c) + 1.2), repr(int(r) + 1.0), ("%.1f" % float(h)).rstrip("0").rstrip(".")))
        return "".join(line + "\n" for line in out)

    def _svg(self, texture):
        H, W = self.shape
        y0, x0 = self.origin
        out = ['<svg xmlns="http://www.w3.org/2000/svg" xmlns:xlink="http://www.w3.org/1999/xlink" viewBox="%d %d %d %d" '
               'fill="none" stroke="#4d2e12">' % (x0, y0, W - 1, H - 1)]
        if texture is not None:
            import base64
            import io
            from PIL import Image
            tex = np.ascontiguousarray(texture)
            if tex.dtype != np.uint8 or tex.shape[:2] != (H, W):
                raise ValueError("the texture must be uint8 of the contours' size %s, got %s %s" % ((H, W), tex.dtype, tex.shape))
            buf = io.BytesIO()
            Image.fromarray(tex[:, :, 0] if tex.ndim == 3 and tex.shape[2] == 1 else tex).save(buf, format="PNG")
            # a pixel's centre is its cell's position: the image starts half a pixel before the origin
            out.append('<image x="%g" y="%g" width="%d" height="%d" preserveAspectRatio="none" xlink:href="data:image/png;base64,%s"/>'
                       % (x0 - 0.5, y0 - 0.5, W, H, base64.b64encode(buf.getvalue()).decode("ascii")))
        for i in range(len(self)):
            pts = self.line(i)
            d = "M" + " L".join("%s %s" % (repr(float(c)), repr(float(r))) for r, c in pts) + (" Z" if self.closed[i] else "")
            out.append('<path class="%s" data-level="%d" stroke-width="%s" d="%s"/>' % (
                "index" if self.is_index(i) else "line", int(self.level[i]), "0.6" if self.is_index(i) else "0.25", d))
        out.append("</svg>")
        return "\n".join(out) + "\n"

    def _geojson(self):
        feats = []
        for i in range(len(self)):
            pts = self.line(i)
            xy = [[float(c), float(r)] for r, c in pts]
            if self.closed[i]:
                xy.append(xy[0])
            feats.append({"type": "Feature", "geometry": {"type": "LineString", "coordinates": xy},
                          "properties": {"level": int(self.level[i]), "height": float(self.height(i)), "index": bool(self.is_index(i)),
                                         "closed": bool(self.closed[i])}})
        return {"type": "FeatureCollection", "features": feats}


def _check_max_segments(v):
    if not _is_int(v) or not 0 <= v < 1 << 31:
        raise ValueError("max_segments must be an integer in [0, 2^31), got %r" % (v,))
    return int(v)


def _level_args(levels):
    return levels.base_q, levels.interval_q, -1 if levels.count is None else levels.count


def contours(ops, heightmap, levels=None, origin=(0, 0), max_segments=1 << 26, keep=()):
    """The contour lines of a heightmap: upload, the quantisation, the count, the trace, the extraction, download, inside one
    scratch.  ops: a device.Ops; heightmap: (H, W) or (1, H, W), floating point, finite and in [0, 1], or uint8; levels: a Levels
    (default Levels()); origin: the coordinates of cell [0, 0]; max_segments: a plane with more segments is refused with a
    ValueError that names their number, before the workspace (28 bytes a segment) is allocated -- a condition, not a
    measurement; the default is chosen; keep: 'zq', to return the quantised heights.  A plane with H < 2 or W < 2 has no cells
    and no lines.  Returns a Contours."""
    keep = check_keep(keep, KEEP)
    levels = _check_levels(levels)
    origin = _check_origin(origin)
    max_segments = _check_max_segments(max_segments)
    a = as_plane(heightmap, unit_range=True, raw=True)
    H, W = a.shape
    n = H * W
    lv = _level_args(levels)
    zq = np.empty((H, W), np.int32) if 'zq' in keep else None
    dev = ops.dev
    with scratch(dev) as alloc:
        d_h, d_z = alloc(4 * n), alloc(4 * n)
        dev.h2d(d_h, a)
        ops.viewshed_quantise(d_h, W, H, W, levels.height_scale, d_z, W)
        d_c = alloc(ops.contour_cells_bytes(H, W))
        S = ops.contour_count(d_z, W, H, W, *lv, d_c)
        if S > max_segments:
            raise ValueError("the plane of %d x %d has %d contour segments, more than max_segments = %d: widen the interval, "
                             "or raise max_segments" % (H, W, S, max_segments))
        d_w = alloc(ops.contour_workspace(H, W, S))
        L, V, rounds = ops.contour_trace(d_z, W, H, W, *lv, d_c, d_w, S)
        out = (np.empty((V, 3), np.int32), np.empty(V, np.float64), np.empty(L + 1, np.int64), np.empty(L, np.int32),
               np.empty(L, np.uint8))
        ptrs = [alloc(max(x.nbytes, 16)) for x in out]
        ops.contour_extract(d_z, W, H, W, *lv, d_c, d_w, S, L, V, *ptrs)
        dev.sync()
        for x, p in zip(out, ptrs):
            if x.nbytes:
                dev.d2h(x, p, x.nbytes)
        if zq is not None:
            dev.d2h(zq, d_z, zq.nbytes)
    return Contours(*out, levels, origin, (H, W), rounds, zq)


def marks(ops, heightmap, levels=None):
    """uint32 (H, W): 0 where no level separates a pixel's height from its right and its lower neighbour's, 2 where an index contour
    does, else 1 -- what ``paint`` blends; one launch"""
    levels = _check_levels(levels)
    a = as_plane(heightmap, unit_range=True, raw=True)
    H, W = a.shape
    out = np.empty((H, W), np.uint32)
    dev = ops.dev
    with scratch(dev) as alloc:
        d_h, d_z, d_m = alloc(4 * H * W), alloc(4 * H * W), alloc(4 * H * W)
        dev.h2d(d_h, a)
        ops.viewshed_quantise(d_h, W, H, W, levels.height_scale, d_z, W)
        ops.contour_marks(d_z, W, H, W, *_level_args(levels), levels.index_every, d_m, W)
        dev.sync()
        dev.d2h(out, d_m, out.nbytes)
    return out


def paint(ops, texture, heightmap_or_contours, levels=None, colour=(0.25, 0.15, 0.05), opacity=0.6, index_opacity=0.9,
          value_range=None):
    """The contour lines of a heightmap drawn on a texture of its size, a pixel wide: the marks (ghm_contour_marks) blended with
    the hydrology's paint kernel towards ``colour`` (three numbers in [0, 1]), every marked pixel with ``opacity`` and, in a second
    pass over the first's result, the index contours' with ``index_opacity``.  heightmap_or_contours: the heightmap, or a
    Contours that kept its 'zq' (its levels are taken unless ``levels`` is given).  texture, value_range and the result: as
    hydrology.paint's; unpainted pixels keep their bits."""
    colour, opacity, index_opacity = _check_colour(colour), _check_opacity(opacity), _check_opacity(index_opacity)
    if isinstance(heightmap_or_contours, Contours):
        c = heightmap_or_contours
        if c.zq is None:
            raise ValueError("paint needs the heights: a Contours that kept 'zq', or the heightmap")
        levels = _check_levels(c.levels if levels is None else levels)
        if levels.height_scale != c.levels.height_scale:
            raise ValueError("the Contours' heights were quantised at height_scale %g, the levels say %g" % (
                c.levels.height_scale, levels.height_scale))
        _hy._texture_planes(texture, value_range)                       # the texture's form, before the device is read
        H, W = c.zq.shape
        m = np.empty((H, W), np.uint32)
        dev = ops.dev
        with scratch(dev) as alloc:
            d_z, d_m = alloc(c.zq.nbytes), alloc(m.nbytes)
            dev.h2d(d_z, np.ascontiguousarray(c.zq, np.int32))
            ops.contour_marks(d_z, W, H, W, *_level_args(levels), levels.index_every, d_m, W)
            dev.sync()
            dev.d2h(m, d_m, m.nbytes)
    else:
        levels = _check_levels(levels)
        _hy._texture_planes(texture, value_range)
        m = marks(ops, heightmap_or_contours, levels)
    once = _hy._paint(ops, texture, value_range, "heightmap", m.shape, None, m, 1, 0, colour, opacity)
    return _hy._paint(ops, once, value_range, "heightmap", m.shape, None, m, 2, 0, colour, index_opacity)


# ---- command line -------------------------------------------------------------------------------------------------------
def add_level_arguments(p):
    d = Levels()
    p.add_argument("--interval", type=float, default=d.interval, help="cells of height between two levels (default %g)" % d.interval)
    p.add_argument("--base", type=float, default=d.base, help="the height of level 0, in cells (default 0)")
    p.add_argument("--count", type=int, default=None, metavar="N", help="keep the levels 0 .. N - 1 (1: one isoline at --base)")
    p.add_argument("--index-every", type=int, default=d.index_every, metavar="N",
                   help="every N-th level is an index contour (default %d)" % d.index_every)


def parse_args(argv):
    p = argparse.ArgumentParser(prog="python -m gan_heightmaps_amd.contour",
                                description="The contour lines of a heightmap as ordered polylines (on the GPU).")
    p.add_argument("input", help="heightmap: 8-bit PNG (read as greyscale), or .npy (uint8 or float in [0, 1], (H, W))")
    p.add_argument("output", help="the lines: .svg, .geojson or .npz")
    add_level_arguments(p)
    p.add_argument("--height-scale", type=float, default=Levels().height_scale, help="cells of height per unit of the heightmap")
    p.add_argument("--texture", default=None, metavar="F", help="a texture of the heightmap's size: embedded in an .svg, and what "
                                                                 "--painted draws the lines on")
    p.add_argument("--painted", default=None, metavar="OUT", help="where the texture with the lines painted on goes (PNG)")
    p.add_argument("--colour", type=_colour, default=(0.25, 0.15, 0.05), metavar="R,G,B", help="the paint's colour, in [0, 1]")
    p.add_argument("--opacity", type=float, default=0.6, help="how far painted pixels go towards the colour, in [0, 1]")
    # a base that starts with a minus sign would read as an option: hand it over in the --base=... form
    argv = list(argv)
    for i in range(len(argv) - 2, -1, -1):
        if argv[i] == "--base" and argv[i + 1].lstrip()[:1] == "-":
            argv[i:i + 2] = ["--base=" + argv[i + 1]]
    a = p.parse_args(argv)
    if a.painted is not None and a.texture is None:
        p.error("--painted needs --texture")
    if not a.output.lower().endswith((".svg", ".geojson", ".npz")):
        p.error("the output is .svg, .geojson or .npz")
    try:
        a.levels = Levels(a.interval, a.base, a.count, a.index_every, a.height_scale)
        _check_colour(a.colour)
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
        got = contours(ops, x, a.levels, keep='zq' if a.painted else ())
        painted = None if a.painted is None else paint(ops, texture, got, colour=a.colour, opacity=a.opacity,
                                                       index_opacity=min(1.0, 1.5 * a.opacity))
    finally:
        dev.close()
    got.save(a.output, texture=texture if a.output.lower().endswith(".svg") else None)
    if painted is not None:
        _hy._save_painted(a.painted, painted)
    print("%d lines (%d closed), %d vertices" % (len(got), int(got.closed.sum()), len(got.t)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
