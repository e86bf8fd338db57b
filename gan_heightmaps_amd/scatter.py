"""Scatter: where trees and rocks stand on a heightmap -- a Poisson-disk point set whose density follows the terrain, on the device
(csrc/scatter.hip).  The hydrology (§4t), the routes (§4u) and the earthworks (§4v) shape the ground; this is the layer
above it.  Deterministic from a seed and from world coordinates, and equal to a definition in numpy (tests/scatter_ref.py) bit
for bit.

The plane is h[H, W], float32 and finite, taken in by the hydrology's intake (read as h + 0; uint8 is read as v / 255).

1. The chance, a uint32 plane in [0, 2^24]: the probability, in units of 2^-24, that a cell is a candidate.  Float32, every
   operation rounded on its own, no division and no sqrt on the device: a ``Habitat`` builds three tables in float64, each entry
   rounded once.
     altitude : 256 weights; the cell's is the one at clamp(trunc(h 255 + 0.5), 0, 255).
     slope    : 64 weights by the bin of the central difference's squared length g2 = gx^2 + gy^2, gx = (h[y, x + 1] -
                h[y, x - 1]) float32(height_scale / 2), the plane's edge repeated; bin k holds the angles from k 90 / 64 to
                (k + 1) 90 / 64 degrees and takes the weight of its middle.
     water    : optional; weights by the squared distance to the nearest wet cell (a lake or a river of ``hydro``), which
                ``earthworks.nearest`` finds, and one more for "none within reach".
   chance = trunc(((altitude slope) water) density 2^24); 0 on blocked ground: within a clearance of a lake, a river or a road
   (``earthworks.nearest`` again), or where the caller says so.
2. The candidates: hash = the chained lowbias32 mixer of include/ghm.h over (seed, stream, world row, world col).  A cell is a
   candidate iff hash(stream 0) >> 8 < chance; its priority is hash(stream 1).  Both are functions of the seed and the world
   position alone: two planes that overlap in the world agree on them where their chances agree.
3. The thinning: two cells conflict iff dy^2 + dx^2 < s2 = ceil(spacing^2).  The kept candidates are those that dart throwing in
   (priority, row, col) order keeps; the device reaches them as the fixed point of a local rule (csrc/scatter.hip has the argument)
   in two forms with the same bits, ``plain`` (one launch per Jacobi sweep) and ``tiled`` (32 x 32 tiles swept in LDS).
4. The points are collected on the host from the downloaded state plane, in row-major order; yaw and scale are hashed per point
   from streams 2 and 3.

    python -m gan_heightmaps_amd.scatter IN OUT.{npz,csv} --spacing X [--density X] [--altitude LO,HI] [--altitude-fade X]
        [--slope LO,HI] [--slope-fade X] [--water GAIN,REACH] [--lake-clearance X] [--river-clearance X] [--river-threshold N]
        [--lake-min-depth X] [--height-scale X] [--scale LO,HI] [--name S] [--seed N] [--hydrology] [--texture F --painted OUT
        [--colour R,G,B] [--radius N]] [--plain | --tiled]
"""
import argparse
import dataclasses
import math
import sys

import numpy as np

from . import earthworks as _ew
from . import hydrology as _hy
from .planes import as_plane, check_keep, check_size, scratch
from .util import form_choice, is_int as _is_int, is_number as _number, read_image

__all__ = ["DEFAULT_TILED", "KEEP", "MAX_SPACING", "MAX_S2", "ONE", "TILE", "NONE", "UNDECIDED", "KEPT", "REJECTED", "Habitat", "Species",
           "Layer", "Scatter", "mix", "hash32", "slope_bounds", "chance", "thin", "scatter", "paint", "parse_args", "main"]

TILE = 32                    # GHM_SCATTER_TILE (include/ghm.h)
MAX_S2 = 1024                # GHM_SCATTER_MAX_S2
MAX_SPACING = 32
MAX_REACH = _ew.MAX_REACH
ONE = 1 << 24                # GHM_SCATTER_ONE: the chance that is certainty
NONE, UNDECIDED, KEPT, REJECTED = 0, 1, 2, 3
MIX_A, MIX_B, MIX_STEP = 0x7feb352d, 0x846ca68b, 0x9e3779b9          # GHM_SCATTER_MIX_*
KEEP = ('chance', 'priority', 'state')
# the form ``thin`` and ``scatter`` run by default: the one tools/scatter_bench.py shows faster on the MI355X -- the plain one, for a
# 4096 x 4096 plane with every cell a candidate 1.93 against 2.12 ms at spacing 2, 15.7 against 26.1 ms at spacing 8 and 169 against
# 303 ms at spacing 32; the tiled one wins only where candidates are few and the spacing small (a tenth of the cells, spacing 2:
# 0.62 against 0.91 ms) (DESIGN §4w has the line); both give the same bits
DEFAULT_TILED = False


# ---- the mixer, on the host (yaw and scale; tests/scatter_ref.py restates it on its own) ---------------------------------------
def mix(x):
    x = np.array(x, np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(MIX_A)
    x ^= x >> np.uint32(15)
    x *= np.uint32(MIX_B)
    x ^= x >> np.uint32(16)
    return x


def hash32(seed, stream, row, col):
    """the mixer chained over (seed, stream, row, col): seed modulo 2^64, row and col (integer arrays) modulo 2^32 -> uint32"""
    seed = int(seed) & ((1 << 64) - 1)
    row = (np.asarray(row, np.int64) & 0xFFFFFFFF).astype(np.uint32)
    col = (np.asarray(col, np.int64) & 0xFFFFFFFF).astype(np.uint32)
    row, col = np.broadcast_arrays(row, col)
    k = np.uint32(MIX_STEP)
    with np.errstate(over='ignore'):
        x = mix(np.uint32(seed & 0xFFFFFFFF) + k)
        x = mix((x ^ np.uint32(seed >> 32)) + k)
        x = mix((x ^ np.uint32(stream)) + k)
        x = mix((x ^ row) + k)
        return mix((x ^ col) + k)


def slope_bounds():
    """float32 [63]: the squared tangents of k 90 / 64 degrees, k = 1 .. 63, computed in float64 and rounded once"""
    return (np.tan(np.radians(np.arange(1, 64, dtype=np.float64) * (90.0 / 64))) ** 2).astype(np.float32)


def _band(x, lo, hi, fade):
    """1 inside [lo, hi], falling linearly to 0 over ``fade`` outside it; float64"""
    if fade == 0:
        return ((x >= lo) & (x <= hi)).astype(np.float64)
    return np.clip((x - (lo - fade)) / fade, 0.0, 1.0) * np.clip(((hi + fade) - x) / fade, 0.0, 1.0)


def _pair(v, name, lo, hi):
    try:
        a, b = v
        ok = _number(a) and _number(b) and lo <= a <= b <= hi
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("%s must be (low, high) with %g <= low <= high <= %g, got %r" % (name, lo, hi, v))
    return float(a), float(b)


@dataclasses.dataclass(frozen=True)
class Habitat:
    """Where a species grows, validated and frozen.  ``altitude``: the band (low, high) of heights, in units of the heightmap,
    inside which the weight is 1, falling to 0 over ``altitude_fade`` outside it; ``slope`` and ``slope_fade``: the same in
    degrees, 0 .. 90; ``density`` in [0, 1]: the share of the cells of ideal ground that become candidates.  ``water``: None, or
    (gain, reach) with gain in [0, 1] and reach in (0, 32] cells: the weight is 1 at a wet cell and falls linearly to 1 - gain at
    ``reach`` cells and beyond.  ``lake_clearance``, ``river_clearance``, ``road_clearance``: None, or a distance in [0, 32]
    cells within which nothing grows (0: on the cells themselves).  A cell is a lake where the filled depth exceeds
    ``lake_min_depth`` and a river where the drainage area reaches ``river_threshold`` cells.  The defaults are chosen, not
    measured."""
    altitude: tuple = (0.0, 1.0)
    altitude_fade: float = 0.05
    slope: tuple = (0.0, 30.0)
    slope_fade: float = 10.0
    density: float = 1.0
    water: object = None
    lake_clearance: object = 0.0
    river_clearance: object = 0.0
    road_clearance: object = 1.0
    river_threshold: int = 256
    lake_min_depth: float = 1.0 / 512

    def __post_init__(self):
        object.__setattr__(self, "altitude", _pair(self.altitude, "altitude", -3e38, 3e38))
        object.__setattr__(self, "slope", _pair(self.slope, "slope", 0.0, 90.0))
        for name, top in (("altitude_fade", 3e38), ("slope_fade", 90.0), ("lake_min_depth", 3e38)):
            v = getattr(self, name)
            if not _number(v) or not 0 <= v <= top:
                raise ValueError("%s must be a finite number in [0, %g], got %r" % (name, top, v))
            object.__setattr__(self, name, float(v))
        if not _number(self.density) or not 0 <= self.density <= 1:
            raise ValueError("density must lie in [0, 1], got %r" % (self.density,))
        object.__setattr__(self, "density", float(self.density))
        if self.water is not None:
            try:
                gain, reach = self.water
                ok = _number(gain) and _number(reach) and 0 <= gain <= 1 and 0 < reach <= MAX_REACH
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError("water must be None or (gain in [0, 1], reach in (0, %d]), got %r" % (MAX_REACH, self.water))
            object.__setattr__(self, "water", (float(gain), float(reach)))
        for name in ("lake_clearance", "river_clearance", "road_clearance"):
            v = getattr(self, name)
            if v is not None:
                if not _number(v) or not 0 <= v <= MAX_REACH:
                    raise ValueError("%s must be None or a number in [0, %d], got %r" % (name, MAX_REACH, v))
                object.__setattr__(self, name, float(v))
        if not _is_int(self.river_threshold) or not 1 <= self.river_threshold < 1 << 32:
            raise ValueError("river_threshold must be an integer in [1, 2^32), got %r" % (self.river_threshold,))
        object.__setattr__(self, "river_threshold", int(self.river_threshold))

    def altitude_table(self):
        """float32 [256]: the weight of the height i / 255"""
        return _band(np.arange(256, dtype=np.float64) / 255.0, self.altitude[0], self.altitude[1], self.altitude_fade).astype(np.float32)

    def slope_table(self):
        """float32 [64]: the weight of the angle (k + 1/2) 90 / 64 degrees"""
        mid = (np.arange(64, dtype=np.float64) + 0.5) * (90.0 / 64)
        return _band(mid, self.slope[0], self.slope[1], self.slope_fade).astype(np.float32)

    def tables(self):
        """float32 [384], what the device reads: the altitude weights, the 63 bounds of the slope bins and an unused entry, the slope
        weights"""
        t = np.zeros(384, np.float32)
        t[:256] = self.altitude_table()
        t[256:319] = slope_bounds()
        t[320:] = self.slope_table()
        return t

    @property
    def water_reach(self):
        return 0 if self.water is None else int(math.ceil(self.water[1]))

    def water_table(self):
        """None, or float32 [R^2 + 2], R = ceil(reach): the weight by the squared distance d2 = 0 .. R^2 to the nearest wet cell,
        and at [R^2 + 1] that of a cell with none within R"""
        if self.water is None:
            return None
        gain, reach = self.water
        r = np.sqrt(np.arange(self.water_reach ** 2 + 1, dtype=np.float64))
        w = (1.0 - gain) + gain * np.clip(1.0 - r / reach, 0.0, 1.0)
        return np.concatenate([w, [1.0 - gain]]).astype(np.float32)


@dataclasses.dataclass(frozen=True)
class Species:
    """What is placed, validated and frozen: a ``name`` (a non-empty string without commas), the ``spacing`` no two of its points
    come closer than, a real number in (0, 32] cells -- two cells conflict iff dy^2 + dx^2 < ``s2`` = ceil(spacing^2) --, its
    ``habitat`` (default Habitat()), the range ``scale`` = (low, high) of its instances' sizes, 0 < low <= high, and
    ``seed_stream``, an integer in [0, 2^32) that tells its draws from those of other species under the same seed."""
    name: str
    spacing: float
    habitat: Habitat = None
    scale: tuple = (0.8, 1.25)
    seed_stream: int = 0

    def __post_init__(self):
        if not isinstance(self.name, str) or not self.name or "," in self.name or "\n" in self.name:
            raise ValueError("name must be a non-empty string without commas, got %r" % (self.name,))
        if not _number(self.spacing) or not 0 < self.spacing <= MAX_SPACING:
            raise ValueError("spacing must be a number in (0, %d], got %r" % (MAX_SPACING, self.spacing))
        object.__setattr__(self, "spacing", float(self.spacing))
        habitat = Habitat() if self.habitat is None else self.habitat
        if not isinstance(habitat, Habitat):
            raise ValueError("habitat must be a Habitat, got %r" % (self.habitat,))
        object.__setattr__(self, "habitat", habitat)
        lo, hi = _pair(self.scale, "scale", 0.0, 3e38)
        if lo <= 0:
            raise ValueError("scale must be positive, got %r" % (self.scale,))
        object.__setattr__(self, "scale", (lo, hi))
        if not _is_int(self.seed_stream) or not 0 <= self.seed_stream < 1 << 32:
            raise ValueError("seed_stream must be an integer in [0, 2^32), got %r" % (self.seed_stream,))
        object.__setattr__(self, "seed_stream", int(self.seed_stream))

    @property
    def s2(self):
        return int(math.ceil(self.spacing * self.spacing))

    def seed(self, seed):
        """the 64-bit seed of this species' draws under the caller's ``seed``"""
        return (int(seed) + (self.seed_stream << 32) + self.seed_stream * MIX_STEP) & ((1 << 64) - 1)


class Layer:
    """One species of a Scatter: the ``species``; ``points`` int32 [n, 2], world (row, col) in row-major order; ``height`` float32
    [n], the heightmap there; ``yaw`` float32 [n] in [0, 2 pi) and ``scale`` float32 [n] in the species' range, hashed per point;
    ``candidates``, how many cells the thinning started from; ``sweeps``, the launches it took; the planes that were kept."""

    def __init__(self, species, points, height, yaw, scale, candidates, sweeps, **planes):
        self.species, self.points, self.height, self.yaw, self.scale = species, points, height, yaw, scale
        self.candidates, self.sweeps = candidates, sweeps
        for k in KEEP:
            setattr(self, k, planes.get(k))

    def __len__(self):
        return int(self.points.shape[0])


class Scatter:
    """What ``scatter`` returns: ``layers``, one Layer per species in the order given; the ``shape`` of the plane and the
    ``origin``, the world coordinates of its cell [0, 0]; the form ``tiled`` of the thinning; ``sweeps``, the launches per
    species."""

    def __init__(self, shape, origin, tiled, layers):
        self.shape = tuple(shape)
        self.origin = (int(origin[0]), int(origin[1]))
        self.tiled = tiled
        self.layers = list(layers)

    @property
    def sweeps(self):
        return tuple(l.sweeps for l in self.layers)

    def __getitem__(self, name):
        for l in self.layers:
            if l.species.name == name:
                return l
        raise KeyError(name)

    def __repr__(self):
        return "Scatter(%d x %d at %r, %s)" % (self.shape + (self.origin, ", ".join("%s: %d" % (l.species.name, len(l))
                                                                                     for l in self.layers)))

    def raster(self):
        """uint32 plane of ``shape``: k + 1 on the points of layer k, 0 elsewhere"""
        m = np.zeros(self.shape, np.uint32)
        for k, l in enumerate(self.layers):
            m[l.points[:, 0] - self.origin[0], l.points[:, 1] - self.origin[1]] = k + 1
        return m

    def save(self, path):
        """.npz: origin, shape, names and, per layer k, points_k, height_k, yaw_k, scale_k; .csv: a header and one line
        ``species,row,col,height,yaw,scale`` per point (floats with nine significant digits: float32 survives)"""
        if path.endswith(".npz"):
            out = dict(origin=np.array(self.origin, np.int64), shape=np.array(self.shape, np.int64),
                       names=np.array([l.species.name for l in self.layers]))
            for k, l in enumerate(self.layers):
                for f in ("points", "height", "yaw", "scale"):
                    out["%s_%d" % (f, k)] = getattr(l, f)
            np.savez(path, **out)
        elif path.endswith(".csv"):
            with open(path, "w") as f:
                f.write("species,row,col,height,yaw,scale\n")
                for l in self.layers:
                    for (r, c), h, y, s in zip(l.points.tolist(), l.height.tolist(), l.yaw.tolist(), l.scale.tolist()):
                        f.write("%s,%d,%d,%.9g,%.9g,%.9g\n" % (l.species.name, r, c, h, y, s))
        else:
            raise ValueError("a scatter is saved as .npz or .csv, got %r" % (path,))


# ---- checks ---------------------------------------------------------------------------------------------------------------------
def _check_s2(s2):
    if not _is_int(s2) or not 1 <= s2 <= MAX_S2:
        raise ValueError("s2 must be an integer in [1, %d], got %r" % (MAX_S2, s2))
    return int(s2)


def _check_seed(seed):
    if not _is_int(seed):
        raise ValueError("seed must be an integer, got %r" % (seed,))
    return int(seed) & ((1 << 64) - 1)


def _check_origin(origin):
    try:
        r, c = origin
        ok = _is_int(r) and _is_int(c) and abs(int(r)) < 1 << 62 and abs(int(c)) < 1 << 62
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("origin must be (row, col), two integers, got %r" % (origin,))
    return int(r), int(c)


def _check_height_scale(v):
    if not _number(v) or not 0 < v < 3e38 or not float(np.float32(v / 2.0)) > 0:
        raise ValueError("height_scale must be a positive finite number, got %r" % (v,))
    return float(v)


def _check_mask(m, shape, name):
    m = np.asarray(m)
    if m.shape != tuple(shape) or m.dtype.kind not in "iub":
        raise ValueError("%s must be an integer or boolean plane of %d x %d, got %s %s" % ((name,) + tuple(shape) + (m.dtype, m.shape)))
    return m != 0


def _check_species(species):
    one = isinstance(species, Species)
    todo = [species] if one else list(species) if isinstance(species, (list, tuple)) else None
    if not todo or not all(isinstance(s, Species) for s in todo):
        raise ValueError("species must be a Species or a non-empty list of them, got %r" % (species,))
    if len(set(s.name for s in todo)) != len(todo):
        raise ValueError("the species' names must differ")
    return todo


def _reach_of(s2):
    """the least reach R of earthworks.nearest, which finds marks up to d2 = R^2, that sees every conflict d2 < s2"""
    R = math.isqrt(s2 - 1)
    return R if R * R >= s2 - 1 else R + 1


def _within(ops, marks, clearance, tiled):
    """the cells within ``clearance`` of a marked cell, by earthworks.nearest"""
    if clearance == 0 or not marks.any():
        return marks
    d2 = _ew.nearest(ops, marks.astype(np.uint32), int(math.ceil(clearance)), tiled=tiled)[1]
    return (d2 >= 0) & (d2 <= clearance * clearance)


def _ground(ops, shape, habitat, hydro, roads, blocked, tiled):
    """-> (dist2 int32 or None, water table or None, blocked uint32 plane or None): what the chance launch takes beside the heights"""
    off = np.zeros(shape, bool)
    dist2 = table = None
    if blocked is not None:
        off |= blocked
    if hydro is not None:
        lakes = hydro.depth > np.float32(habitat.lake_min_depth)
        rivers = (hydro.accumulation >= habitat.river_threshold) & ~lakes
        if habitat.lake_clearance is not None:
            off |= _within(ops, lakes, habitat.lake_clearance, tiled)
        if habitat.river_clearance is not None:
            off |= _within(ops, rivers, habitat.river_clearance, tiled)
        if habitat.water is not None:
            dist2 = _ew.nearest(ops, (lakes | rivers).astype(np.uint32), habitat.water_reach, tiled=tiled)[1]
            table = habitat.water_table()
    if roads is not None and habitat.road_clearance is not None:
        off |= _within(ops, roads, habitat.road_clearance, tiled)
    return dist2, table, (off.astype(np.uint32) if off.any() else None)


def _check_ground(shape, hydro, roads, blocked):
    if hydro is not None:
        if not isinstance(hydro, _hy.Hydrology) or hydro.depth is None or hydro.accumulation is None:
            raise ValueError("hydro must be a Hydrology that kept 'depth' and 'accumulation'")
        if tuple(hydro.shape) != tuple(shape):
            raise ValueError("heightmap %s and hydrology %s differ in size" % (tuple(shape), tuple(hydro.shape)))
    roads = None if roads is None else _check_mask(roads, shape, "roads")
    blocked = None if blocked is None else _check_mask(blocked, shape, "blocked")
    return roads, blocked


def _run(ops, a, habitat, ground, height_scale, stages=None, keep=()):
    """upload, the chance launch and, with stages = (seed, origin, s2, tiled), the candidates and the thinning; download ->
    {'chance', 'priority', 'state' as asked for, 'candidates', 'sweeps'}"""
    H, W = a.shape
    n = H * W
    dist2, water, marks = ground
    tables = habitat.tables()
    dev = ops.dev
    out = {}
    with scratch(dev) as alloc:
        d_h, d_t, d_c = alloc(4 * n), alloc(tables.nbytes), alloc(4 * n)
        dev.h2d(d_h, a)
        dev.h2d(d_t, tables)
        d_d = d_w = d_b = None
        if water is not None:
            d_d, d_w = alloc(4 * n), alloc(water.nbytes)
            dev.h2d(d_d, np.ascontiguousarray(dist2, np.int32))
            dev.h2d(d_w, water)
        if marks is not None:
            d_b = alloc(4 * n)
            dev.h2d(d_b, marks)
        ops.scatter_chance(d_h, W, H, W, d_t, height_scale, habitat.density, d_c, W, d_d, W, d_w,
                           0 if water is None else water.size - 1, d_b, W, 1)
        want = [('chance', d_c, np.uint32)] if 'chance' in keep or stages is None else []
        if stages is not None:
            seed, origin, s2, tiled = stages
            d_s, d_p, ws = alloc(n), alloc(4 * n), alloc(ops.scatter_workspace(H, W))
            ops.scatter_candidates(d_c, W, H, W, seed, origin, d_s, W, d_p, W)
            out['sweeps'] = ops.scatter_thin(d_p, W, d_s, W, H, W, s2, tiled, ws)
            want += [('state', d_s, np.uint8)] + ([('priority', d_p, np.uint32)] if 'priority' in keep else [])
        dev.sync()
        for name, ptr, dtype in want:
            out[name] = np.empty((H, W), dtype)
            dev.d2h(out[name], ptr, out[name].nbytes)
    if stages is not None:
        out['candidates'] = int((out['state'] != NONE).sum())            # every candidate is decided, and nothing else is
    return out


# ---- the functions --------------------------------------------------------------------------------------------------------------
def chance(ops, heightmap, habitat=None, hydro=None, roads=None, blocked=None, height_scale=64.0, tiled=None):
    """The chance of every cell to be a candidate, in units of 2^-24: uint32 (H, W).  ops: a device.Ops; heightmap: (H, W) or
    (1, H, W), floating point and finite, or uint8; habitat: a Habitat (default Habitat()); hydro: a hydrology.Hydrology of the
    same plane that kept ``depth`` and ``accumulation`` -- its lakes and rivers are the wet cells of the habitat's water
    preference and clearances; roads, blocked: integer or boolean planes, non-zero on road cells and on ground where nothing may
    grow; height_scale: cells of height per unit of the heightmap (the slope's); tiled: the form of earthworks.nearest."""
    habitat = Habitat() if habitat is None else habitat
    if not isinstance(habitat, Habitat):
        raise ValueError("habitat must be a Habitat, got %r" % (habitat,))
    height_scale = _check_height_scale(height_scale)
    a = as_plane(heightmap, raw=True)
    roads, blocked = _check_ground(a.shape, hydro, roads, blocked)
    return _run(ops, a, habitat, _ground(ops, a.shape, habitat, hydro, roads, blocked, tiled), height_scale)['chance']


def thin(ops, state, priority, s2, tiled=None):
    """The Poisson-disk thinning of a plane of candidates: upload, the relaxation, download.  state: uint8 (H, W), 1 a candidate
    (2 and 3, kept and rejected, are taken as decided), 0 none; priority: uint32 (H, W); s2: an integer in [1, 1024]: two cells
    conflict iff dy^2 + dx^2 < s2; tiled: the LDS form (True) or the plain one (False): the same bits; default DEFAULT_TILED.
    Returns (state, sweeps): 2 on the kept candidates, 3 on the rejected ones, and the launches it took."""
    s2 = _check_s2(s2)
    st, pr = np.asarray(state), np.asarray(priority)
    if st.ndim != 2 or st.dtype != np.uint8 or pr.shape != st.shape or pr.dtype != np.uint32:
        raise ValueError("state must be a uint8 plane and priority a uint32 plane of its size, got %s %s and %s %s" % (
            st.dtype, st.shape, pr.dtype, pr.shape))
    check_size(st.shape[0], st.shape[1], limits=True)
    tiled = DEFAULT_TILED if tiled is None else bool(tiled)
    H, W = st.shape
    st, pr = np.ascontiguousarray(st), np.ascontiguousarray(pr)
    out = np.empty((H, W), np.uint8)
    dev = ops.dev
    with scratch(dev) as alloc:
        d_s, d_p, ws = alloc(st.nbytes), alloc(pr.nbytes), alloc(ops.scatter_workspace(H, W))
        dev.h2d(d_s, st)
        dev.h2d(d_p, pr)
        sweeps = ops.scatter_thin(d_p, W, d_s, W, H, W, s2, tiled, ws)
        dev.d2h(out, d_s, out.nbytes)
    return out, sweeps


def _instances(species, seed, points):
    """yaw in [0, 2 pi) and scale in the species' range: streams 2 and 3 of the mixer at the points' world positions, the top 24 bits
    as a fraction, computed in float64 and rounded once"""
    u = (hash32(seed, 2, points[:, 0], points[:, 1]) >> np.uint32(8)).astype(np.float64) / ONE
    v = (hash32(seed, 3, points[:, 0], points[:, 1]) >> np.uint32(8)).astype(np.float64) / ONE
    lo, hi = species.scale
    return (u * (2.0 * math.pi)).astype(np.float32), (lo + (hi - lo) * v).astype(np.float32)


def scatter(ops, heightmap, species, seed=0, origin=(0, 0), hydro=None, roads=None, blocked=None, height_scale=64.0, tiled=None,
            keep=()):
    """Points placed on a heightmap: per species the chance launch, the candidates launch, the thinning, one download.  ops: a
    device.Ops; heightmap, hydro, roads, blocked, height_scale: ``chance``'s; species: a Species or a list of them -- in a list
    every later species is also blocked within its own spacing of the points already placed, so the widest spacing goes
    first; seed: an integer, taken modulo 2^64; origin: the world coordinates of cell [0, 0], with which the plane must lie
    inside the int32 range: candidates and priorities are functions of the seed and the world position; tiled: the form of
    the thinning, default DEFAULT_TILED (given, it is also that of earthworks.nearest, which else takes its own default); keep:
    the planes to return per layer out of 'chance', 'priority', 'state'.  Returns a Scatter."""
    keep = check_keep(keep, KEEP)
    todo = _check_species(species)
    seed, origin = _check_seed(seed), _check_origin(origin)
    height_scale = _check_height_scale(height_scale)
    a = as_plane(heightmap, raw=True)
    H, W = a.shape
    if not (-(1 << 31) <= origin[0] and origin[0] + H <= 1 << 31 and -(1 << 31) <= origin[1] and origin[1] + W <= 1 << 31):
        raise ValueError("origin %r puts the plane of %d x %d outside the int32 range of the points" % (origin, H, W))
    roads, blocked = _check_ground(a.shape, hydro, roads, blocked)
    near_form, tiled = tiled, DEFAULT_TILED if tiled is None else bool(tiled)
    placed = np.zeros((H, W), bool)
    layers = []
    for sp in todo:
        off = blocked
        if placed.any():
            d2 = _ew.nearest(ops, placed.astype(np.uint32), _reach_of(sp.s2), tiled=near_form)[1]
            near = (d2 >= 0) & (d2 < sp.s2)
            off = near if off is None else off | near
        ground = _ground(ops, a.shape, sp.habitat, hydro, roads, off, near_form)
        sseed = sp.seed(seed)
        out = _run(ops, a, sp.habitat, ground, height_scale, (sseed, origin, sp.s2, tiled), keep)
        local = np.argwhere(out['state'] == KEPT)
        placed[local[:, 0], local[:, 1]] = True
        points = (local + np.array(origin, np.int64)).astype(np.int64)
        yaw, scale = _instances(sp, sseed, points)
        layers.append(Layer(sp, points.astype(np.int32), a[local[:, 0], local[:, 1]], yaw, scale, out['candidates'], out['sweeps'],
                            **{k: out[k] for k in keep}))
    return Scatter((H, W), origin, tiled, layers)


def _check_colours(colours, n):
    try:
        flat = len(colours) == 3 and all(_number(c) for c in colours)
        colours = [tuple(colours)] * n if flat else [tuple(c) for c in colours]
        ok = len(colours) == n and all(len(c) == 3 and all(_number(v) and 0 <= v <= 1 for v in c) for c in colours)
    except TypeError:
        ok = False
    if not ok:
        raise ValueError("colours must be three numbers in [0, 1], or one such triple per species (%d), got %r" % (n, colours))
    return colours


def paint(ops, texture, placed, colours=(0.10, 0.28, 0.12), radius=1, opacity=0.9, value_range=None):
    """The points of a Scatter painted on a texture of its size with the hydrology's paint kernel, layer after layer: a pixel
    within ``radius`` pixels (0 .. 4) of a point is blended towards the layer's colour.  colours: three numbers in [0, 1], or
    one such triple per layer.  texture, value_range and the result: as hydrology.paint's; untouched pixels keep their bits."""
    if not isinstance(placed, Scatter):
        raise ValueError("scatter must be a Scatter, got %r" % (placed,))
    colours = _check_colours(colours, len(placed.layers))
    if not _is_int(radius) or not 0 <= radius <= _hy.MAX_RIVER_WIDTH:
        raise ValueError("radius must be an integer in [0, %d], got %r" % (_hy.MAX_RIVER_WIDTH, radius))
    if not _number(opacity) or not 0 <= opacity <= 1:
        raise ValueError("opacity must lie in [0, 1], got %r" % (opacity,))
    marks = placed.raster()
    for k, colour in enumerate(colours):
        texture = _hy._paint(ops, texture, value_range, "scatter", placed.shape, None, (marks == k + 1).astype(np.uint32), 1,
                             int(radius), colour, float(opacity))
    return texture


# ---- command line -------------------------------------------------------------------------------------------------------
def _numbers(count):
    def parse(text):
        try:
            v = tuple(float(t) for t in text.split(","))
        except ValueError:
            v = ()
        if len(v) != count:
            raise argparse.ArgumentTypeError("%d numbers separated by commas, got %r" % (count, text))
        return v
    return parse


def parse_args(argv):
    p = argparse.ArgumentParser(prog="python -m gan_heightmaps_amd.scatter",
                                description="Place one species on a heightmap by Poisson-disk sampling (on the GPU).")
    p.add_argument("input", help="heightmap: 8-bit PNG (read as greyscale), or .npy (uint8 or float, (H, W))")
    p.add_argument("output", help="the points: .npz or .csv")
    h = Habitat()
    p.add_argument("--spacing", type=float, required=True, help="no two points come closer than this many cells (0 < X <= 32)")
    p.add_argument("--density", type=float, default=h.density, help="share of the cells of ideal ground that become candidates")
    p.add_argument("--altitude", type=_numbers(2), default=h.altitude, metavar="LO,HI", help="the band of heights")
    p.add_argument("--altitude-fade", type=float, default=h.altitude_fade, help="height over which the weight falls to 0")
    p.add_argument("--slope", type=_numbers(2), default=h.slope, metavar="LO,HI", help="the band of slopes, in degrees")
    p.add_argument("--slope-fade", type=float, default=h.slope_fade, help="degrees over which the weight falls to 0")
    p.add_argument("--water", type=_numbers(2), default=None, metavar="GAIN,REACH", help="preference for wet ground (--hydrology)")
    p.add_argument("--lake-clearance", type=float, default=h.lake_clearance, help="cells from a lake within which nothing grows")
    p.add_argument("--river-clearance", type=float, default=h.river_clearance, help="cells from a river within which nothing grows")
    p.add_argument("--river-threshold", type=int, default=h.river_threshold, help="cells of drainage area that make a river")
    p.add_argument("--lake-min-depth", type=float, default=h.lake_min_depth, help="filled depth above which a cell is a lake")
    p.add_argument("--height-scale", type=float, default=64.0, help="cells of height per unit of the heightmap")
    p.add_argument("--scale", type=_numbers(2), default=(0.8, 1.25), metavar="LO,HI", help="the range of the instances' sizes")
    p.add_argument("--name", default="tree", help="the species' name")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--hydrology", action="store_true", help="analyse the heightmap's lakes and rivers and keep clear of them")
    p.add_argument("--texture", default=None, metavar="F", help="a texture of the heightmap's size to paint the points on")
    p.add_argument("--painted", default=None, metavar="OUT", help="where the painted texture goes (PNG)")
    p.add_argument("--colour", type=_numbers(3), default=(0.10, 0.28, 0.12), metavar="R,G,B", help="the points' colour, in [0, 1]")
    p.add_argument("--radius", type=int, default=1, help="pixels around a point that are painted (0 .. 4)")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--plain", action="store_true", help="thin by one launch per sweep")
    g.add_argument("--tiled", action="store_true", help="thin by tiles in LDS (the same bits)")
    a = p.parse_args(argv)
    if (a.texture is None) != (a.painted is None):
        p.error("--texture and --painted go together")
    if a.water is not None and not a.hydrology:
        p.error("--water needs --hydrology")
    if not (a.output.endswith(".npz") or a.output.endswith(".csv")):
        p.error("the output is .npz or .csv")
    try:
        habitat = Habitat(altitude=a.altitude, altitude_fade=a.altitude_fade, slope=a.slope, slope_fade=a.slope_fade,
                          density=a.density, water=a.water, lake_clearance=a.lake_clearance, river_clearance=a.river_clearance,
                          river_threshold=a.river_threshold, lake_min_depth=a.lake_min_depth)
        a.species = Species(a.name, a.spacing, habitat, a.scale)
        _check_height_scale(a.height_scale)
        _check_colours(a.colour, 1)
        if not 0 <= a.radius <= _hy.MAX_RIVER_WIDTH:
            raise ValueError("radius must be an integer in [0, %d], got %r" % (_hy.MAX_RIVER_WIDTH, a.radius))
    except ValueError as e:
        p.error(str(e))
    a.form = form_choice(a.tiled, a.plain)
    return a


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    from .device import Device, Ops
    x = read_image(a.input, "L", mmap=False)
    texture = None if a.texture is None else read_image(a.texture, mmap=False)
    dev = Device(0)
    try:
        ops = Ops(dev)
        hydro = _hy.analyse(ops, x, keep=('depth', 'accumulation')) if a.hydrology else None
        placed = scatter(ops, x, a.species, seed=a.seed, hydro=hydro, height_scale=a.height_scale, tiled=a.form)
        painted = None if texture is None else paint(ops, texture, placed, a.colour, a.radius)
    finally:
        dev.close()
    placed.save(a.output)
    if painted is not None:
        _hy._save_painted(a.painted, painted)
    layer = placed.layers[0]
    print("%d points of %d candidates, %d launches" % (len(layer), layer.candidates, layer.sweeps))
    return 0


if __name__ == "__main__":
    sys.exit(main())
