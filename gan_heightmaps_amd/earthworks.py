"""Earthworks: river channels cut and roadbeds graded into a heightmap, on the device (csrc/earthworks.hip).  The
hydrology (§4t) knows where the rivers run and the routes (§4u) where the roads do; this is the step that tells the ground.

The plane is h[H, W], float32 and finite, taken in by the hydrology's intake (read as h + 0; uint8 is read as v / 255).

1. The nearest mark -- an exact, bounded Euclidean feature transform, in integers.  ``marks`` is a uint32 plane; a cell c is
   marked iff marks[c] >= threshold (the paint kernel's convention, so a ``traffic`` or ``accumulation`` plane goes in with its
   threshold, a raster of ones with 1).  For an integer reach R in [0, 32], nearest[y, x] is the flat index i W + j of the
   marked cell (i, j) of the plane with |i - y| <= R, |j - x| <= R and d2 = (i - y)^2 + (j - x)^2 <= R^2 that minimises the
   triple (d2, i, j) lexicographically, and dist2[y, x] that d2; both are NONE = -1 where there is no such cell.  The plane's
   edge ends the search.  Two forms with the same bits: ``plain``, one thread per cell scanning its (2R + 1)^2 window in
   row-major order and keeping a candidate only on a strictly smaller d2, and ``tiled``, 32 x 32 tiles whose (32 + 2R)^2 window
   of marks is staged in LDS, a column pass (per window column and tile row the nearest mark of the column within R rows, the
   upper on equal distance) and a row pass (the least (dx^2 + dy^2, row, col) over the 2R + 1 columns); a tile whose window
   holds no mark skips both.
2. The table of a ``Profile(core, reach, mode)``, 0 <= core <= reach <= 32: R = floor(reach), and for d2 = 0 .. R^2, in float64,
   r = sqrt(d2), s = clamp((r - core) / (reach - core), 0, 1) -- with reach == core, s = 0 where r <= core and 1 elsewhere --,
   take = 1 - (s s) (3 - 2 s) and keep = 1 - take, each rounded once to float32.  Inside the core keep = 0 and take = 1.
3. The shaping, float32, every operation rounded on its own, no sqrt and no division on the device.  Where nearest is NONE or
   take[dist2] == 0 the cell keeps its bits.  Elsewhere v = (keep[dist2] h) + (take[dist2] target[nearest]); mode 'both' gives
   v, 'cut' gives v where v < h and h elsewhere, 'fill' gives v where v > h and h elsewhere.  ``target`` is a float32 plane
   that is read at marked cells alone: elsewhere it may hold anything, NaN included.  A core cell gets its target's bits.
4. The targets are made on the host (numpy, small).  ``Channel``: the cells with accumulation >= river_threshold that are no
   lake (not depth > lake_min_depth: lakes stay flat) are marked; with the exact integers k = accumulation // river_threshold
   and b = k.bit_length() - 1, D = min(max_depth, depth + growth b) in float64 and target = float32(filled -
   float32(D / height_scale)), a float32 subtraction; the mode is 'cut'.  ``Roadbed``: the cells of the given paths -- or those
   whose traffic reaches ``traffic_threshold`` -- and, repeatedly, the parents of marked cells are marked; the target of a marked
   cell is the mean, summed in float64 from the cell on and rounded once to float32, of h over the cell and up to ``smooth``
   cells following ``parent`` towards the source, where the window stops.  One definition for paths and networks, whatever the
   order of the paths.

    python -m gan_heightmaps_amd.earthworks IN OUT [--rivers] [--from R,C ... --to R,C ...] [--traffic-threshold N]
        [--channel-depth X --channel-growth X --channel-max-depth X --river-threshold N --lake-min-depth X --river-core X
        --river-reach X] [--road-core X --road-reach X --road-smooth N --road-mode both|cut|fill] [--height-scale X]
        [--plain | --tiled]
"""
import argparse
import dataclasses
import math
import sys

import numpy as np

from . import hydrology as _hy
from . import route as _rt
from .planes import as_plane, check_keep, check_size, scratch
from .util import form_choice, is_int as _is_int, is_number as _number, read_image, save_png, to_uint8

__all__ = ["DEFAULT_TILED", "KEEP", "MAX_REACH", "NONE", "TILE", "MODES", "Profile", "Channel", "Roadbed", "Earthworks", "nearest",
           "carve", "channel_targets", "road_targets", "cut_rivers", "grade_roads", "parse_args", "main"]

TILE = 32                    # GHM_EARTHWORKS_TILE (include/ghm.h)
MAX_REACH = 32               # GHM_EARTHWORKS_MAX_REACH
NONE = -1                    # GHM_EARTHWORKS_NONE
MAX_SMOOTH = 4096
MODES = ('both', 'cut', 'fill')
KEEP = ('height', 'nearest', 'dist2')
# the form ``nearest`` and ``carve`` run by default: the one tools/earthworks_bench.py shows faster on the MI355X -- the tiled one, for
# a 4096 x 4096 plane with its river cells as marks 0.130 against 0.427 ms at reach 4 and 1.31 against 14.8 ms at reach 32 (DESIGN
# §4v has the line); both give the same bits
DEFAULT_TILED = True


def _check_core_reach(core, reach):
    for name, v in (("core", core), ("reach", reach)):
        if not _number(v) or not 0 <= v <= MAX_REACH:
            raise ValueError("%s must be a finite number in [0, %d], got %r" % (name, MAX_REACH, v))
    if core > reach:
        raise ValueError("core must not exceed reach, got core=%r, reach=%r" % (core, reach))


def _check_mode(mode):
    if mode not in MODES:
        raise ValueError("mode must be one of %s, got %r" % (", ".join(MODES), mode))


@dataclasses.dataclass(frozen=True)
class Profile:
    """The cross-section of an earthwork, validated and frozen: within ``core`` cells of a marked cell the ground takes the
    target, from there to ``reach`` cells it blends back into the land by a smoothstep (0 <= core <= reach <= 32, finite
    numbers); ``mode``: 'both', 'cut' (never raises the ground) or 'fill' (never lowers it).  ``R`` = floor(reach) is the
    reach of the nearest-mark search, ``table()`` the (keep, take) pairs by squared distance the device blends with."""
    core: float
    reach: float
    mode: str = 'both'

    def __post_init__(self):
        _check_core_reach(self.core, self.reach)
        _check_mode(self.mode)
        object.__setattr__(self, "core", float(self.core))
        object.__setattr__(self, "reach", float(self.reach))

    @property
    def R(self):
        return int(math.floor(self.reach))

    @property
    def mode_index(self):
        return MODES.index(self.mode)

    def table(self):
        """float32 [R^2 + 1, 2]: (keep[d2], take[d2]), computed in float64 and rounded once each"""
        r = np.sqrt(np.arange(self.R * self.R + 1, dtype=np.float64))
        if self.reach == self.core:
            s = np.where(r <= self.core, 0.0, 1.0)
        else:
            s = np.clip((r - self.core) / (self.reach - self.core), 0.0, 1.0)
        take = 1.0 - (s * s) * (3.0 - 2.0 * s)
        keep = 1.0 - take
        return np.ascontiguousarray(np.stack([keep.astype(np.float32), take.astype(np.float32)], axis=1))


@dataclasses.dataclass(frozen=True)
class Channel:
    """How ``cut_rivers`` cuts a river bed, validated and frozen.  A cell is a river where its drainage area reaches
    ``river_threshold`` cells (an integer in [1, 2^32)) and its filled depth does not exceed ``lake_min_depth`` (>= 0: lakes
    stay flat).  The bed lies ``depth`` + ``growth`` per doubling of the area beyond the threshold, at most ``max_depth``,
    below the filled surface, in cells of height (all >= 0, finite): ``height_scale`` (> 0) cells of height per unit of the
    heightmap.  ``core`` and ``reach``: the channel's Profile, in mode 'cut'.  The defaults are chosen, not measured."""
    river_threshold: int = 256
    lake_min_depth: float = 1.0 / 512
    depth: float = 0.5
    growth: float = 0.25
    max_depth: float = 3.0
    core: float = 0.0
    reach: float = 4.0
    height_scale: float = 64.0

    def __post_init__(self):
        if not _is_int(self.river_threshold) or not 1 <= self.river_threshold < 1 << 32:
            raise ValueError("river_threshold must be an integer in [1, 2^32), got %r" % (self.river_threshold,))
        for name in ("lake_min_depth", "depth", "growth", "max_depth"):
            v = getattr(self, name)
            if not _number(v) or not 0 <= v < 3e38:
                raise ValueError("%s must be a finite number >= 0, got %r" % (name, v))
        v = self.height_scale
        if not _number(v) or not 0 < v < 3e38 or not 1.0 / v < 3e38:
            raise ValueError("height_scale must be a positive finite number, got %r" % (v,))
        _check_core_reach(self.core, self.reach)
        for name in ("lake_min_depth", "depth", "growth", "max_depth", "core", "reach", "height_scale"):
            object.__setattr__(self, name, float(getattr(self, name)))
        object.__setattr__(self, "river_threshold", int(self.river_threshold))

    @property
    def profile(self):
        return Profile(self.core, self.reach, 'cut')


@dataclasses.dataclass(frozen=True)
class Roadbed:
    """How ``grade_roads`` levels a roadbed, validated and frozen.  ``core`` and ``reach``: the bed's Profile; ``smooth`` (an
    integer in [0, 4096]): the cells ahead, towards the source, over which a road cell's target height is averaged -- 0 keeps
    the ground's own height along the road; ``mode``: 'both' cuts and fills, 'cut' and 'fill' do one.  The defaults are chosen,
    not measured."""
    core: float = 1.0
    reach: float = 6.0
    smooth: int = 8
    mode: str = 'both'

    def __post_init__(self):
        _check_core_reach(self.core, self.reach)
        _check_mode(self.mode)
        if not _is_int(self.smooth) or not 0 <= self.smooth <= MAX_SMOOTH:
            raise ValueError("smooth must be an integer in [0, %d], got %r" % (MAX_SMOOTH, self.smooth))
        object.__setattr__(self, "core", float(self.core))
        object.__setattr__(self, "reach", float(self.reach))
        object.__setattr__(self, "smooth", int(self.smooth))

    @property
    def profile(self):
        return Profile(self.core, self.reach, self.mode)


class Earthworks:
    """What ``carve`` returns: the planes it was asked to keep as numpy arrays (the others are None) -- ``height`` float32,
    ``nearest`` and ``dist2`` int32 --, the ``shape``, the ``origin`` (the coordinates of cell [0, 0]), the form ``tiled`` of
    the nearest-mark search, and ``cut`` / ``fill``: the volumes removed and added, in cells times units of the heightmap,
    float64, summed on the host from the plane before and after."""

    def __init__(self, shape, origin=(0, 0), tiled=False, cut=0.0, fill=0.0, **planes):
        self.shape = tuple(shape)
        self.origin = (int(origin[0]), int(origin[1]))
        self.tiled = tiled
        self.cut = cut
        self.fill = fill
        for k in KEEP:
            setattr(self, k, planes.get(k))

    def __repr__(self):
        return "Earthworks(%d x %d at %r, cut=%g, fill=%g, planes=%s)" % (
            self.shape + (self.origin, self.cut, self.fill, [k for k in KEEP if getattr(self, k) is not None]))


def _check(value, kind, name):
    value = kind() if value is None else value
    if not isinstance(value, kind):
        raise ValueError("%s must be a %s, got %r" % (name, kind.__name__, value))
    return value


def _check_threshold(threshold):
    if not _is_int(threshold) or not 1 <= threshold < 1 << 32:
        raise ValueError("threshold must be an integer in [1, 2^32), got %r" % (threshold,))
    return int(threshold)


def _check_marks(marks, shape=None):
    m = np.asarray(marks)
    if m.ndim != 2 or m.dtype.kind not in "iub" or (shape is not None and m.shape != tuple(shape)):
        raise ValueError("marks must be an integer plane%s, got %s %s" % (
            "" if shape is None else " of %d x %d" % tuple(shape), m.dtype, m.shape))
    if shape is None:
        check_size(m.shape[0], m.shape[1], limits=True)
    if m.size and (m.min() < 0 or m.max() >= 1 << 32):
        raise ValueError("marks must lie in [0, 2^32)")
    return np.ascontiguousarray(m, np.uint32)


def _check_reach(reach):
    if not _is_int(reach) or not 0 <= reach <= MAX_REACH:
        raise ValueError("reach must be an integer in [0, %d], got %r" % (MAX_REACH, reach))
    return int(reach)


def nearest(ops, marks, reach, threshold=1, tiled=None):
    """The nearest marked cell within ``reach`` of every cell: upload, one launch, download.  ops: a device.Ops; marks: an
    integer plane (H, W), marked where >= threshold (an integer in [1, 2^32)); reach: an integer in [0, 32]; tiled: the LDS
    form (True) or the plain one (False): the same bits; default DEFAULT_TILED.  Returns (nearest, dist2), int32 planes: the
    flat index i W + j and the squared distance of the nearest marked cell, ties to the least (row, col); -1 where none lies
    within the reach."""
    m = _check_marks(marks)
    R, threshold = _check_reach(reach), _check_threshold(threshold)
    tiled = DEFAULT_TILED if tiled is None else bool(tiled)
    H, W = m.shape
    dev = ops.dev
    near, d2 = np.empty((H, W), np.int32), np.empty((H, W), np.int32)
    with scratch(dev) as alloc:
        d_m, d_n, d_d = alloc(m.nbytes), alloc(near.nbytes), alloc(d2.nbytes)
        dev.h2d(d_m, m)
        ops.earthworks_nearest(d_m, W, H, W, threshold, R, tiled, d_n, W, d_d, W)
        dev.sync()
        dev.d2h(near, d_n, near.nbytes)
        dev.d2h(d2, d_d, d2.nbytes)
    return near, d2


def carve(ops, heightmap, marks, target, profile, threshold=1, tiled=None, keep=('height',), origin=(0, 0)):
    """A heightmap shaped towards ``target`` around the marked cells: upload, the nearest-mark launch, the shaping launch,
    download.  ops: a device.Ops; heightmap: (H, W) or (1, H, W), floating point and finite, or uint8; marks: an integer plane,
    marked where >= threshold; target: a floating-point plane, finite at the marked cells and read nowhere else; profile: a
    Profile; tiled: the form of the nearest-mark search; keep: the planes to return out of 'height', 'nearest', 'dist2';
    origin: the coordinates of cell [0, 0], passed on.  Returns an Earthworks; a cell beyond the profile's reach of every mark
    keeps its bits."""
    keep = check_keep(keep, KEEP)
    if not isinstance(profile, Profile):
        raise ValueError("profile must be a Profile, got %r" % (profile,))
    threshold = _check_threshold(threshold)
    a = as_plane(heightmap, raw=True)
    H, W = a.shape
    m = _check_marks(marks, (H, W))
    t = np.asarray(target)
    if t.shape != (H, W) or t.dtype.kind != "f":
        raise ValueError("target must be a floating-point plane of %d x %d, got %s %s" % (H, W, t.dtype, t.shape))
    t = np.ascontiguousarray(t, np.float32)
    if not np.isfinite(t[m >= threshold]).all():
        raise ValueError("the target has non-finite values at marked cells")
    origin = (int(origin[0]), int(origin[1]))
    tiled = DEFAULT_TILED if tiled is None else bool(tiled)
    table = profile.table()
    n = H * W
    dev = ops.dev
    out = {}
    with scratch(dev) as alloc:
        bufs = {name: alloc(nbytes) for name, nbytes in (('h', 4 * n), ('marks', 4 * n), ('target', 4 * n), ('nearest', 4 * n),
                                                        ('dist2', 4 * n), ('height', 4 * n), ('table', table.nbytes))}
        for name, x in (('h', a), ('marks', m), ('target', t), ('table', table)):
            dev.h2d(bufs[name], x)
        ops.earthworks_nearest(bufs['marks'], W, H, W, threshold, profile.R, tiled, bufs['nearest'], W, bufs['dist2'], W)
        ops.earthworks_shape(bufs['h'], W, bufs['nearest'], W, bufs['dist2'], W, bufs['target'], W, bufs['table'], profile.R,
                             profile.mode_index, H, W, bufs['height'], W)
        dev.sync()
        for name, dtype in (('height', np.float32), ('nearest', np.int32), ('dist2', np.int32)):
            if name in keep or name == 'height':
                out[name] = np.empty((H, W), dtype)
                dev.d2h(out[name], bufs[name], out[name].nbytes)
    diff = out['height'].astype(np.float64) - a.astype(np.float64)
    cut, fill = float(-diff[diff < 0].sum()) + 0.0, float(diff[diff > 0].sum())      # (+ 0.0: no cut is 0, not -0)
    return Earthworks((H, W), origin, tiled, cut, fill, **{k: out[k] for k in keep})


def channel_targets(filled, depth, accumulation, channel=None):
    """-> (marks uint32: 1 on the river cells that are no lake, target float32: the bed's height there, NaN elsewhere); the
    module docstring's point 4"""
    channel = _check(channel, Channel, "channel")
    filled = np.asarray(filled, np.float32)
    acc = np.asarray(accumulation).astype(np.int64)
    marked = (acc >= channel.river_threshold) & ~(np.asarray(depth, np.float32) > np.float32(channel.lake_min_depth))
    k = acc // channel.river_threshold
    b = np.zeros(k.shape, np.int64)
    for s in range(1, 33):                               # bit_length(k) - 1 for k >= 1, in integers
        b += (k >> s) > 0
    D = np.minimum(channel.max_depth, channel.depth + channel.growth * b.astype(np.float64))
    drop = (D / channel.height_scale).astype(np.float32)
    target = np.where(marked, filled - drop, np.float32(np.nan)).astype(np.float32)
    return marked.astype(np.uint32), target


def _parent_index(parent):
    """the flat index of every cell's parent, -1 where it has none (a source, an unreached cell, a step off the plane)"""
    H, W = parent.shape
    p = np.asarray(parent).astype(np.int64)
    dy = np.array([o[0] for o in _rt.OFFSETS] + [0], np.int64)
    dx = np.array([o[1] for o in _rt.OFFSETS] + [0], np.int64)
    k = np.where((p >= 0) & (p < 8), p, 8)
    i, j = np.indices((H, W), dtype=np.int64)
    y, x = i + dy[k], j + dx[k]
    ok = (k < 8) & (y >= 0) & (y < H) & (x >= 0) & (x < W)
    return np.where(ok, y * W + x, -1).reshape(-1)


def road_targets(h, parent, seeds, roadbed=None):
    """h: the float32 plane; parent: a CostField's; seeds: a boolean plane of the road's cells -> (marks uint32: 1 on the seeds
    and, repeatedly, on the parents of marked cells, target float32: the smoothed height there, NaN elsewhere); the module
    docstring's point 4"""
    roadbed = _check(roadbed, Roadbed, "roadbed")
    h = np.asarray(h, np.float32)
    H, W = h.shape
    up = _parent_index(parent)
    marked = np.asarray(seeds, bool).reshape(-1).copy()
    front = np.flatnonzero(marked)
    while front.size:
        nxt = up[front]
        nxt = np.unique(nxt[nxt >= 0])
        front = nxt[~marked[nxt]]
        marked[front] = True
    cells = np.flatnonzero(marked)
    flat = h.reshape(-1).astype(np.float64)
    total, count = flat[cells].copy(), np.ones(cells.size, np.int64)
    cur, alive = cells.copy(), np.ones(cells.size, bool)
    for _ in range(roadbed.smooth):
        nxt = up[cur]
        alive &= nxt >= 0
        if not alive.any():
            break
        cur = np.where(alive, nxt, cur)
        total += np.where(alive, flat[cur], 0.0)
        count += alive
    target = np.full(H * W, np.nan, np.float32)
    target[cells] = (total / count).astype(np.float32)
    return marked.reshape(H, W).astype(np.uint32), target.reshape(H, W)


def cut_rivers(ops, hydro, channel=None, **kw):
    """River channels cut into ``hydro.filled``.  hydro: a hydrology.Hydrology that kept ``filled``, ``depth`` and
    ``accumulation``; channel: a Channel (default Channel()); kw: carve's (tiled, keep, origin).  Returns an Earthworks whose
    ``fill`` is 0: lakes stay flat, and a bed never lies above the ground."""
    channel = _check(channel, Channel, "channel")
    if not isinstance(hydro, _hy.Hydrology) or any(getattr(hydro, k) is None for k in ('filled', 'depth', 'accumulation')):
        raise ValueError("hydro must be a Hydrology that kept 'filled', 'depth' and 'accumulation'")
    marks, target = channel_targets(hydro.filled, hydro.depth, hydro.accumulation, channel)
    return carve(ops, hydro.filled, marks, target, channel.profile, **kw)


def grade_roads(ops, heightmap, cost_field, paths=(), roadbed=None, traffic_threshold=None, **kw):
    """Roadbeds graded into a heightmap of the field's size.  cost_field: a route.CostField that kept ``parent``; paths:
    [n, 2] arrays of (row, col) as CostField.path returns them (the field's origin included); with ``traffic_threshold`` (an
    integer in [1, 2^32), route.Road's) the cells whose traffic reaches it are taken instead, and the field must have kept
    ``traffic``.  roadbed: a Roadbed (default Roadbed()); kw: carve's (tiled, keep, origin -- default the field's).  Returns an
    Earthworks."""
    roadbed = _check(roadbed, Roadbed, "roadbed")
    if not isinstance(cost_field, _rt.CostField) or cost_field.parent is None:
        raise ValueError("cost_field must be a CostField that kept 'parent'")
    a = as_plane(heightmap, raw=True)
    if a.shape != tuple(cost_field.shape):
        raise ValueError("heightmap %s and cost field %s differ in size" % (a.shape, tuple(cost_field.shape)))
    if traffic_threshold is not None:
        if not _is_int(traffic_threshold) or not 1 <= traffic_threshold < 1 << 32:
            raise ValueError("traffic_threshold must be None or an integer in [1, 2^32), got %r" % (traffic_threshold,))
        if cost_field.traffic is None:
            raise ValueError("traffic_threshold needs a CostField that kept 'traffic'")
        seeds = cost_field.traffic >= traffic_threshold
    else:
        seeds = _rt.raster(a.shape, paths, cost_field.origin) != 0
    marks, target = road_targets(a, cost_field.parent, seeds, roadbed)
    kw.setdefault('origin', cost_field.origin)
    return carve(ops, a, marks, target, roadbed.profile, **kw)


# ---- command line -------------------------------------------------------------------------------------------------------
def parse_args(argv):
    p = argparse.ArgumentParser(prog="python -m gan_heightmaps_amd.earthworks",
                                description="Cut river channels and grade roads into a heightmap (on the GPU).")
    p.add_argument("input", help="heightmap: 8-bit PNG (read as greyscale), or .npy (uint8 or float, (H, W))")
    p.add_argument("output", help="the carved heightmap: .npy (float32), or PNG (8 bits, heights clipped to [0, 1])")
    p.add_argument("--rivers", action="store_true", help="fill the lakes, find the rivers and cut their channels")
    p.add_argument("--from", dest="sources", type=_rt.parse_cell, action="append", metavar="R,C", default=[],
                   help="a source of the roads (a town); repeat for more")
    p.add_argument("--to", dest="targets", type=_rt.parse_cell, action="append", metavar="R,C", default=[],
                   help="a cell whose road to its source is graded; repeat for more")
    p.add_argument("--traffic-threshold", type=int, default=None,
                   help="grade every cell that at least this many cells travel through, instead of the --to roads")
    c, r = Channel(), Roadbed()
    p.add_argument("--channel-depth", type=float, default=c.depth, help="depth of the smallest river's bed, in cells of height")
    p.add_argument("--channel-growth", type=float, default=c.growth, help="depth added per doubling of the drainage area")
    p.add_argument("--channel-max-depth", type=float, default=c.max_depth, help="the deepest bed")
    p.add_argument("--river-threshold", type=int, default=c.river_threshold, help="cells of drainage area that make a river")
    p.add_argument("--lake-min-depth", type=float, default=c.lake_min_depth, help="filled depth above which a cell is a lake")
    p.add_argument("--river-core", type=float, default=c.core, help="cells from the river that take the bed's height")
    p.add_argument("--river-reach", type=float, default=c.reach, help="cells from the river at which the banks meet the land")
    p.add_argument("--road-core", type=float, default=r.core, help="cells from the road that take the bed's height")
    p.add_argument("--road-reach", type=float, default=r.reach, help="cells from the road at which the slopes meet the land")
    p.add_argument("--road-smooth", type=int, default=r.smooth, help="cells ahead over which the road's height is averaged")
    p.add_argument("--road-mode", default=r.mode, choices=list(MODES), help="cut and fill, or one of them")
    p.add_argument("--height-scale", type=float, default=c.height_scale, help="cells of height per unit of the heightmap")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--plain", action="store_true", help="the nearest mark by one window scan per cell")
    g.add_argument("--tiled", action="store_true", help="the nearest mark by tiles in LDS (the same bits)")
    a = p.parse_args(argv)
    if not a.rivers and not a.sources:
        p.error("nothing to do: give --rivers, or --from R,C with --to R,C or --traffic-threshold N")
    if not a.sources and (a.targets or a.traffic_threshold is not None):
        p.error("--to / --traffic-threshold need --from")
    if a.sources and not a.targets and a.traffic_threshold is None:
        p.error("--from needs --to R,C or --traffic-threshold N")
    try:
        a.channel = Channel(river_threshold=a.river_threshold, lake_min_depth=a.lake_min_depth, depth=a.channel_depth,
                            growth=a.channel_growth, max_depth=a.channel_max_depth, core=a.river_core, reach=a.river_reach,
                            height_scale=a.height_scale)
        a.roadbed = Roadbed(core=a.road_core, reach=a.road_reach, smooth=a.road_smooth, mode=a.road_mode)
        a.travel = _rt.Travel(river_threshold=a.river_threshold, lake_min_depth=a.lake_min_depth, height_scale=a.height_scale)
        if a.traffic_threshold is not None:
            _rt.Road(traffic_threshold=a.traffic_threshold)
    except ValueError as e:
        p.error(str(e))
    a.form = form_choice(a.tiled, a.plain)
    return a


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    from .device import Device, Ops
    x = read_image(a.input, "L", mmap=False)
    dev = Device(0)
    cut = fill = 0.0
    try:
        ops = Ops(dev)
        hydro = _hy.analyse(ops, x) if a.rivers else None
        height = as_plane(x, raw=True)
        if hydro is not None:
            e = cut_rivers(ops, hydro, a.channel, tiled=a.form)
            height, cut, fill = e.height, cut + e.cut, fill + e.fill
        if a.sources:
            cf = _rt.field(ops, height if hydro is None else hydro.filled, a.sources, a.travel, hydro=hydro)
            e = grade_roads(ops, height, cf, cf.paths(a.targets), a.roadbed, a.traffic_threshold, tiled=a.form)
            height, cut, fill = e.height, cut + e.cut, fill + e.fill
    finally:
        dev.close()
    if a.output.endswith(".npy"):
        np.save(a.output, height)
    else:
        save_png(a.output, to_uint8(height))
    print("cut %.6g, fill %.6g (cells x heightmap units)" % (cut, fill))
    return 0


if __name__ == "__main__":
    sys.exit(main())
