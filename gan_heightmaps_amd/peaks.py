"""Peaks: the summits of a heightmap with their prominence, key col and parent, found on the device (csrc/peaks.hip).
The other terrain tools answer with planes, lines and meshes; this one says where the mountains are: spot heights for the contour
sheet, observers for the viewshed, passes for the routes, "the ten most important mountains of this region".  Integers
throughout, and equal to a definition in numpy and plain Python (tests/peaks_ref.py) bit for bit.

The plane is h[H, W], float32, finite and in [0, 1] (uint8 is read as v / 255).

1. The heights are the viewshed's: zq = int32(rint(h float32(height_scale 256))), in 1/256 cell.  Cells are totally ordered by
   key(c) = (zq[c], row W + col): of two cells of one height the later is the higher.  Neighbours are the hydrology's eight.
2. Visit the cells in descending key over a union-find of the visited ones.  A cell without a visited neighbour is a summit and
   the top of a new component.  A cell that touches several components joins them: the one whose top has the greatest key
   survives; every other top gets that cell as its key col, its height above it as its prominence, and the survivor's top as its
   parent.  The highest cell has no col and no parent; its prominence is its height above the plane's lowest cell.
3. A summit is reported iff its prominence is at least max(1/256, min_prominence): the several local maxima of one plateau have
   prominence 0 and never are.  Peaks are sorted by (prominence, key), descending; a peak's parent stands before it.

    python -m gan_heightmaps_amd.peaks IN OUT.{geojson,csv,npz} [--min-prominence X] [--top N] [--height-scale X]
        [--texture F --painted OUT [--colour R,G,B] [--radius N] [--cols]] [--plain | --list]
"""
import argparse
import dataclasses
import sys

import numpy as np

from . import hydrology as _hy
from .planes import as_plane, check_keep, scratch
from .util import is_int as _is_int, is_number as _number, read_image
from .viewshed import MAX_HEIGHT, _check_colour, _check_origin, _colour, quantum

__all__ = ["KEEP", "FORMS", "DEFAULT_FORM", "MAX_HEIGHT", "Prominence", "Peaks", "peaks", "report", "raster", "paint", "parse_args",
           "main"]

KEEP = ('zq', 'label')
FORMS = ('plain', 'list')
# tools/peaks_bench.py, 4096 x 4096 value noise, one run: DESIGN §4z has both forms' times
DEFAULT_FORM = 'list'


@dataclasses.dataclass(frozen=True)
class Prominence:
    """Which summits are reported, validated and frozen.  ``min_prominence``: cells of height a summit must rise above its key
    col, in [0, 65536]; whatever it is, a summit of prominence 0 is never reported; ``top``: None, or an integer >= 1 that keeps
    the first N after sorting; ``height_scale``: cells of height per unit of the heightmap, in (0, 65536].  Heights are kept to
    1/256 cell.  The defaults are chosen, not measured."""
    min_prominence: float = 8.0
    top: object = None
    height_scale: float = 64.0

    def __post_init__(self):
        if not _number(self.min_prominence) or not 0 <= self.min_prominence <= MAX_HEIGHT:
            raise ValueError("min_prominence must be a number in [0, %g], got %r" % (MAX_HEIGHT, self.min_prominence))
        object.__setattr__(self, "min_prominence", float(self.min_prominence))
        if self.top is not None:
            if not _is_int(self.top) or not 1 <= self.top < 1 << 31:
                raise ValueError("top must be None or an integer >= 1, got %r" % (self.top,))
            object.__setattr__(self, "top", int(self.top))
        if not _number(self.height_scale) or not 0 < self.height_scale <= MAX_HEIGHT:
            raise ValueError("height_scale must be a number in (0, %g], got %r" % (MAX_HEIGHT, self.height_scale))
        object.__setattr__(self, "height_scale", float(self.height_scale))

    @property
    def min_q(self):
        """the least prominence that is reported, in 1/256 cell"""
        return max(1, quantum(self.min_prominence))


def _check_prominence(prominence):
    prominence = Prominence() if prominence is None else prominence
    if not isinstance(prominence, Prominence):
        raise ValueError("prominence must be a Prominence, got %r" % (prominence,))
    return prominence


def _check_form(form):
    form = DEFAULT_FORM if form is None else form
    if form not in FORMS:
        raise ValueError("form must be one of %r or None, got %r" % (FORMS, form))
    return form


class Peaks:
    """What ``peaks`` returns, n peaks sorted by (prominence, key) descending.  ``cell`` int64 [n, 2], (row, col) in ``origin``'s
    coordinates; ``height``, ``prominence``, ``col_height`` float64 [n], in cells (``col_height``: nan where there is no col);
    ``col`` int64 [n, 2], the key col, or (-1, -1) for the plane's highest peak; ``parent`` int32 [n], the place of the peak's
    parent among these peaks, always before the peak's own, or -1; ``area`` uint32 [n], the cells that climb to the summit;
    ``on_edge`` uint8 [n], 1 where the summit lies on the plane's border -- such a summit is probably a slope the border cut;
    ``summits``, the plane's summits before filtering; ``rounds``, the tree's Boruvka rounds; ``form``; ``prominence_rule``, the
    Prominence; ``origin``; ``shape``; ``zq`` int32 and ``label`` int32 [H, W] (every cell's summit as row W + col), if kept."""

    def __init__(self, cell, height, prominence, col_height, col, parent, area, on_edge, prominence_rule, origin, shape, summits=0,
                 rounds=0, form=None, zq=None, label=None):
        self.cell, self.height, self.prominence, self.col_height = cell, height, prominence, col_height
        self.col, self.parent, self.area, self.on_edge = col, parent, area, on_edge
        self.prominence_rule, self.summits, self.rounds, self.form = prominence_rule, int(summits), int(rounds), form
        self.origin = (int(origin[0]), int(origin[1]))
        self.shape = (int(shape[0]), int(shape[1]))
        self.zq, self.label = zq, label

    def __len__(self):
        return int(self.parent.shape[0])

    def __repr__(self):
        return "Peaks(%d x %d at %r, %d peaks of %d summits)" % (self.shape + (self.origin, len(self), self.summits))

    def _check(self, i):
        if not _is_int(i) or not 0 <= i < len(self):
            raise ValueError("peak %r: there are %d" % (i, len(self)))
        return int(i)

    def observers(self, eye_height=None):
        """the peaks as ``heightmap_viewshed`` observers: [(row, col)] or, with an eye height, [(row, col, eye_height)]"""
        if eye_height is None:
            return [(int(r), int(c)) for r, c in self.cell]
        return [(int(r), int(c), float(eye_height)) for r, c in self.cell]

    def passes(self):
        """the distinct key cols as [(row, col)], in the order of their first peak: targets for ``heightmap_routes``"""
        seen, out = set(), []
        for r, c in self.col[np.isfinite(self.col_height)]:          # (-1, -1) may be a cell of a plane with another origin
            if (int(r), int(c)) not in seen:
                seen.add((int(r), int(c)))
                out.append((int(r), int(c)))
        return out

    def lineage(self, i):
        """[i, its parent, its parent's parent, ...]: it ends at the peak without one"""
        i = self._check(i)
        out = [i]
        while self.parent[out[-1]] >= 0:
            out.append(int(self.parent[out[-1]]))
        return out

    # ---- writers ----------------------------------------------------------------------------------------------------------
    def features(self):
        """the GeoJSON Point features, coordinates [col, row]"""
        out = []
        for i in range(len(self)):
            has = bool(np.isfinite(self.col_height[i]))
            out.append({"type": "Feature", "geometry": {"type": "Point", "coordinates": [int(self.cell[i, 1]), int(self.cell[i, 0])]},
                        "properties": {"height": float(self.height[i]), "prominence": float(self.prominence[i]),
                                       "col": [int(self.col[i, 1]), int(self.col[i, 0])] if has else None,
                                       "col_height": float(self.col_height[i]) if has else None, "parent": int(self.parent[i]),
                                       "area": int(self.area[i]), "on_edge": bool(self.on_edge[i])}})
        return out

    def save(self, path):
        """.npz: the arrays, origin, shape and the rule; .csv: one row per peak; .geojson: Point features with ``height``,
        ``prominence``, ``col``, ``col_height``, ``parent``, ``area`` and ``on_edge`` properties, coordinates [col, row]"""
        low = path.lower()
        if low.endswith(".npz"):
            pr = self.prominence_rule
            np.savez(path, cell=self.cell, height=self.height, prominence=self.prominence, col_height=self.col_height, col=self.col,
                     parent=self.parent, area=self.area, on_edge=self.on_edge, origin=np.array(self.origin, np.int64),
                     shape=np.array(self.shape, np.int64), summits=np.int64(self.summits),
                     rule=np.array([pr.min_prominence, -1 if pr.top is None else pr.top, pr.height_scale]))
        elif low.endswith(".csv"):
            with open(path, "w") as f:
                f.write("row,col,height,prominence,col_row,col_col,col_height,parent,area,on_edge\n")
                for i in range(len(self)):
                    f.write("%d,%d,%r,%r,%d,%d,%r,%d,%d,%d\n" % (
                        self.cell[i, 0], self.cell[i, 1], float(self.height[i]), float(self.prominence[i]), self.col[i, 0],
                        self.col[i, 1], float(self.col_height[i]), self.parent[i], self.area[i], self.on_edge[i]))
        elif low.endswith(".geojson"):
            import json
            with open(path, "w") as f:
                json.dump({"type": "FeatureCollection", "features": self.features()}, f)
        else:
            raise ValueError("peaks are saved as .npz, .csv or .geojson, got %r" % (path,))


def _check_max_summits(v):
    if not _is_int(v) or not 0 <= v < 1 << 31:
        raise ValueError("max_summits must be an integer in [0, 2^31), got %r" % (v,))
    return int(v)


def report(summit, summit_zq, col, col_zq, parent, prominence_q, area, rule, origin, shape, **kw):
    """the Peaks of a plane from its summits' arrays (flat indices; parents as summits' numbers): the filter, the order, the
    parents as places in that order"""
    H, W = shape
    keep = np.flatnonzero(prominence_q >= rule.min_q)
    order = np.lexsort((-summit[keep].astype(np.int64), -summit_zq[keep].astype(np.int64), -prominence_q[keep].astype(np.int64)))
    keep = keep[order][:rule.top]
    place = np.full(len(summit) + 1, -1, np.int32)
    place[keep] = np.arange(len(keep), dtype=np.int32)
    s = summit[keep].astype(np.int64)
    c = col[keep].astype(np.int64)
    has = c >= 0
    cell = np.stack([origin[0] + s // W, origin[1] + s % W], 1) if len(keep) else np.zeros((0, 2), np.int64)
    cols = np.full((len(keep), 2), -1, np.int64)
    cols[has, 0], cols[has, 1] = origin[0] + c[has] // W, origin[1] + c[has] % W
    on_edge = ((s // W == 0) | (s // W == H - 1) | (s % W == 0) | (s % W == W - 1)).astype(np.uint8)
    return Peaks(cell, summit_zq[keep] / 256.0, prominence_q[keep] / 256.0, np.where(has, col_zq[keep] / 256.0, np.nan), cols,
                 place[parent[keep]], area[keep].astype(np.uint32), on_edge, rule, origin, shape, summits=len(summit), **kw)


def peaks(ops, heightmap, prominence=None, origin=(0, 0), form=None, max_summits=1 << 26, keep=()):
    """The peaks of a heightmap: upload, the quantisation, the ascent, the labels and areas (the hydrology's accumulation over
    the ascent), the count, the tree, the extraction, download, inside one scratch; then the merge on the host.  ops: a
    device.Ops; heightmap: (H, W) or (1, H, W), floating point, finite and in [0, 1], or uint8; prominence: a Prominence (default
    Prominence()); origin: the coordinates of cell [0, 0]; form: 'plain' or 'list', the same bits (default DEFAULT_FORM);
    max_summits: a plane with more summits is refused with a ValueError that names their number, before the tree is built and the
    extraction's arrays are allocated -- a condition, not a measurement; the default is chosen; keep: of 'zq' and 'label'.
    Returns a Peaks."""
    keep = check_keep(keep, KEEP)
    rule = _check_prominence(prominence)
    origin = _check_origin(origin)
    form = _check_form(form)
    max_summits = _check_max_summits(max_summits)
    a = as_plane(heightmap, unit_range=True, raw=True)
    H, W = a.shape
    n = H * W
    zq = np.empty((H, W), np.int32)
    label = np.empty((H, W), np.int32) if 'label' in keep else None
    dev = ops.dev
    with scratch(dev) as alloc:
        d_h, d_z = alloc(4 * n), alloc(4 * n)
        dev.h2d(d_h, a)
        ops.viewshed_quantise(d_h, W, H, W, rule.height_scale, d_z, W)
        d_dir, d_area, d_label, d_hw = alloc(n), alloc(4 * n), alloc(4 * n), alloc(ops.hydrology_workspace(H, W))
        ops.peaks_ascent(d_z, W, H, W, d_dir, W)
        ops.hydrology_accumulate(d_dir, W, H, W, d_area, W, d_label, W, d_hw)
        d_w = alloc(ops.peaks_workspace(H, W))
        P, E = ops.peaks_count(d_z, W, d_label, W, H, W, d_w)
        if P > max_summits:
            raise ValueError("the plane of %d x %d has %d summits, more than max_summits = %d: smooth it, or raise max_summits" % (
                H, W, P, max_summits))
        d_m = alloc(4 * n)
        d_l = alloc(max(ops.peaks_list_bytes(E), 16)) if form == 'list' else None
        rounds = ops.peaks_tree(d_z, W, d_label, W, H, W, FORMS.index(form), d_m, W, d_w, d_l, P, E)
        out = (np.empty(P, np.int32), np.empty(P, np.uint32), np.empty((P - 1, 3), np.int32))
        ptrs = [alloc(max(x.nbytes, 16)) for x in out]
        ops.peaks_extract(d_label, W, d_area, W, d_m, W, H, W, d_w, P, *ptrs)
        dev.sync()
        for x, p in zip(out, ptrs):
            if x.nbytes:
                dev.d2h(x, p, x.nbytes)
        dev.d2h(zq, d_z, zq.nbytes)
        if label is not None:
            dev.d2h(label, d_label, label.nbytes)
    summit, area, tree = out
    z = zq.ravel()
    col, parent, prom = ops.peaks_merge(summit, z[summit], tree, z[tree[:, 0]], int(z.min()))
    return report(summit, z[summit], col, z[np.maximum(col, 0)], parent, prom, area, rule, origin, (H, W), rounds=rounds, form=form,
                  zq=zq if 'zq' in keep else None, label=label)


def _check_radius(radius):
    if not _is_int(radius) or not 0 <= radius <= _hy.MAX_RIVER_WIDTH:
        raise ValueError("radius must be an integer in [0, %d], got %r" % (_hy.MAX_RIVER_WIDTH, radius))
    return int(radius)


def raster(found, cols=False):
    """uint32 (H, W): 1 at the peaks' cells (cols: at their key cols instead), 0 elsewhere"""
    if not isinstance(found, Peaks):
        raise ValueError("peaks must be a Peaks, got %r" % (found,))
    m = np.zeros(found.shape, np.uint32)
    at = np.array(found.passes(), np.int64).reshape(-1, 2) if cols else found.cell
    m[at[:, 0] - found.origin[0], at[:, 1] - found.origin[1]] = 1
    return m


def paint(ops, texture, found, colour=(0.9, 0.1, 0.1), radius=2, cols=False, opacity=1.0, value_range=None):
    """The peaks of a Peaks painted on a texture of its plane's size with the hydrology's paint kernel: a pixel within ``radius``
    pixels (0 .. 4) of a peak -- cols: of a key col -- is blended towards ``colour`` (three numbers in [0, 1]).  texture,
    value_range and the result: as hydrology.paint's; unpainted pixels keep their bits."""
    colour, radius = _check_colour(colour), _check_radius(radius)
    if not _number(opacity) or not 0 <= opacity <= 1:
        raise ValueError("opacity must lie in [0, 1], got %r" % (opacity,))
    marks = raster(found, cols)
    return _hy._paint(ops, texture, value_range, "peaks", found.shape, None, marks, 1, radius, colour, float(opacity))


# ---- command line -------------------------------------------------------------------------------------------------------
def add_prominence_arguments(p):
    d = Prominence()
    p.add_argument("--min-prominence", type=float, default=d.min_prominence,
                   help="cells of height a peak must rise above its key col (default %g)" % d.min_prominence)
    p.add_argument("--top", type=int, default=None, metavar="N", help="keep the N most prominent peaks")


def parse_args(argv):
    p = argparse.ArgumentParser(prog="python -m gan_heightmaps_amd.peaks",
                                description="The peaks of a heightmap: prominence, key cols and parents (on the GPU).")
    p.add_argument("input", help="heightmap: 8-bit PNG (read as greyscale), or .npy (uint8 or float in [0, 1], (H, W))")
    p.add_argument("output", help="the peaks: .geojson, .csv or .npz")
    add_prominence_arguments(p)
    p.add_argument("--height-scale", type=float, default=Prominence().height_scale, help="cells of height per unit of the heightmap")
    p.add_argument("--texture", default=None, metavar="F", help="a texture of the heightmap's size, what --painted draws the peaks on")
    p.add_argument("--painted", default=None, metavar="OUT", help="where the texture with the peaks painted on goes (PNG)")
    p.add_argument("--colour", type=_colour, default=(0.9, 0.1, 0.1), metavar="R,G,B", help="the paint's colour, in [0, 1]")
    p.add_argument("--radius", type=int, default=2, metavar="N", help="pixels around a peak that are painted (0 .. 4)")
    p.add_argument("--cols", action="store_true", help="paint the key cols instead of the peaks")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--plain", dest="form", action="store_const", const="plain", default=None, help="every round sweeps the plane")
    g.add_argument("--list", dest="form", action="store_const", const="list", help="the rounds run over a list of edges")
    a = p.parse_args(argv)
    if (a.painted is None) != (a.texture is None):
        p.error("--painted and --texture go together")
    if not a.output.lower().endswith((".geojson", ".csv", ".npz")):
        p.error("the output is .geojson, .csv or .npz")
    try:
        a.prominence = Prominence(a.min_prominence, a.top, a.height_scale)
        _check_colour(a.colour)
        _check_radius(a.radius)
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
        got = peaks(ops, x, a.prominence, form=a.form)
        painted = None if a.painted is None else paint(ops, texture, got, a.colour, a.radius, a.cols)
    finally:
        dev.close()
    got.save(a.output)
    if painted is not None:
        _hy._save_painted(a.painted, painted)
    print("%d peaks of %d summits, %d rounds" % (len(got), got.summits, got.rounds))
    return 0


if __name__ == "__main__":
    sys.exit(main())
