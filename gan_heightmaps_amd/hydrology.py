"""Where the water is on a heightmap: filled lakes, flow directions, drainage area and basins, computed on the device
(csrc/hydrology.hip).

The plane is h[H, W], float32 and finite (uint8 is read as v / 255; -0 as +0).  The eight neighbours of a cell are k = 0 .. 7 in
the order N, NE, E, SE, S, SW, W, NW: (dy, dx) = (-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1).  The cells
of the first and last row and column are *outlets*: water leaves the map there.

1. ``filled`` F is the smallest surface >= h in which every cell that is no outlet has a neighbour that is not higher:
   F = h at the outlets and F[c] = max(h[c], min_k F[n_k]) elsewhere.  The kernels relax it from F = +inf; only max and min are
   involved, so every sweep order reaches the same fixed point in the same bits -- the one a priority-flood from the outlets
   gives.  ``depth`` = F - h, one float32 subtraction, is the depth of the lakes.
2. The flat distance D (int32): a cell is *draining* if it is an outlet or has a neighbour with F strictly lower, and then
   D = 0; otherwise D[c] = 1 + min D[n] over the neighbours with F[n] == F[c].  Again a relaxation, from a large sentinel, with
   one fixed point.  Every plateau of a filled surface holds a draining cell, so D is finite everywhere.
3. ``direction`` (int8): -1 at an outlet.  A draining cell takes the k with the largest slope s_k = (F[c] - F[n_k]) w_k, w_k = 1
   for N, E, S, W and float32(0.70710678) for the diagonals, the subtraction and the product each rounded on their own in float32;
   only neighbours with F[n_k] < F[c] count, and ties go to the lowest k.  Any other cell takes the lowest k with
   F[n_k] == F[c] and D[n_k] == D[c] - 1.  The receiver's (F, D) is lexicographically smaller than the cell's, so the directions
   form a forest rooted at the outlets.
4. ``accumulation`` A (uint32): the number of cells that drain through a cell, itself included (H W < 2^31).  By pointer
   doubling: S_0 = 1, P_0 = the receiver or -1 at an outlet; S_{k+1}[c] = S_k[c] + sum of S_k[d] over P_k(d) = c and
   P_{k+1}(d) = P_k(P_k(d)), until no pointer is alive, which takes at most ceil(log2(H W)) rounds.  The sums are 32-bit integer
   atomic adds: exact and the same in any order.
5. ``basin`` (int32): the flat index i W + j of the outlet a cell drains to, from the same rounds.

Steps 1 and 2 have two forms with the same bits: ``plain``, one Jacobi sweep per launch between two global planes, and
``tiled``, 32 x 32 tiles swept in LDS up to 32 times per launch.  The host launches in groups, reads one device word per group,
and stops at the first group that changed nothing; more than H W sweeps is an error, not a hang.

``paint`` puts the water on a texture: a pixel is wet if depth > lake_min_depth, or if the largest A in its
(2 river_width + 1)^2 window, clamped at the edges, is >= river_threshold; a wet pixel becomes t + opacity (colour - t) per
channel in float32, the subtraction, the product and the sum each rounded on their own; dry pixels pass through untouched.

    python -m gan_heightmaps_amd.hydrology IN OUT_PREFIX [--texture F --painted OUT] [--river-threshold N] [--river-width N]
        [--lake-min-depth X] [--opacity X] [--plain | --tiled]
"""
import argparse
import dataclasses
import functools
import sys

import numpy as np

from .planes import as_plane, check_keep, scratch
from .util import form_choice, is_int as _is_int, is_number as _number, read_image

__all__ = ["DEFAULT_TILED", "KEEP", "MAX_RIVER_WIDTH", "Water", "Hydrology", "analyse", "paint", "parse_args", "main"]

MAX_RIVER_WIDTH = 4          # GHM_HYDROLOGY_MAX_RIVER_WIDTH (include/ghm.h)
KEEP = ('filled', 'depth', 'direction', 'accumulation', 'basin')
# the form ``analyse`` runs by default: the one tools/hydrology_bench.py shows faster on the MI355X -- the tiled one, for a
# 4096 x 4096 plane 8.71 against 132 ms for the fill and 7.92 against 222 ms for the flat distance (DESIGN §4t has the line);
# both give the same bits
DEFAULT_TILED = True


def _check_blend(paint):
    """the part of a Water and a Road that says how marked pixels are blended: ``opacity`` in [0, 1] and ``colour``, three
    numbers in [0, 1], checked and frozen as a float and a tuple of floats"""
    if not _number(paint.opacity) or not 0.0 <= paint.opacity <= 1.0:
        raise ValueError("opacity must lie in [0, 1], got %r" % (paint.opacity,))
    try:
        colour = tuple(paint.colour)
    except TypeError:
        colour = ()
    if len(colour) != 3 or not all(_number(c) and 0.0 <= c <= 1.0 for c in colour):
        raise ValueError("colour must be three numbers in [0, 1], got %r" % (paint.colour,))
    object.__setattr__(paint, "opacity", float(paint.opacity))
    object.__setattr__(paint, "colour", tuple(float(c) for c in colour))


@dataclasses.dataclass(frozen=True)
class Water:
    """How ``paint`` shows the water, validated and frozen: a pixel is a river where the drainage area reaches
    ``river_threshold`` cells (an integer in [1, 2^32)) within ``river_width`` pixels (0 .. 4), a lake where the filled depth
    exceeds ``lake_min_depth`` (>= 0, in height units); wet pixels are blended towards ``colour`` (three values in [0, 1]) with
    ``opacity`` in [0, 1]."""
    river_threshold: int = 256
    river_width: int = 1
    lake_min_depth: float = 1.0 / 512
    colour: tuple = (0.13, 0.29, 0.45)
    opacity: float = 0.85

    def __post_init__(self):
        if not _is_int(self.river_threshold) or not 1 <= self.river_threshold < 1 << 32:
            raise ValueError("river_threshold must be an integer in [1, 2^32), got %r" % (self.river_threshold,))
        if not _is_int(self.river_width) or not 0 <= self.river_width <= MAX_RIVER_WIDTH:
            raise ValueError("river_width must be an integer in [0, %d], got %r" % (MAX_RIVER_WIDTH, self.river_width))
        if not _number(self.lake_min_depth) or not 0 <= self.lake_min_depth < 3e38:
            raise ValueError("lake_min_depth must be a finite number >= 0, got %r" % (self.lake_min_depth,))
        _check_blend(self)
        object.__setattr__(self, "river_threshold", int(self.river_threshold))
        object.__setattr__(self, "river_width", int(self.river_width))
        object.__setattr__(self, "lake_min_depth", float(self.lake_min_depth))


class Hydrology:
    """What ``analyse`` returns: the planes it was asked to keep as numpy arrays (the others are None) -- ``filled`` and
    ``depth`` float32, ``direction`` int8, ``accumulation`` uint32, ``basin`` int32 -- the ``shape``, and the counts actually
    run: ``sweeps`` = (launches of the fill, launches of the flat distance) and ``rounds`` of pointer doubling."""

    def __init__(self, shape, sweeps, rounds, tiled, **planes):
        self.shape = shape
        self.sweeps = sweeps
        self.rounds = rounds
        self.tiled = tiled
        for k in KEEP:
            setattr(self, k, planes.get(k))

    def __repr__(self):
        return "Hydrology(%d x %d, sweeps=%r, rounds=%d, planes=%s)" % (
            self.shape + (self.sweeps, self.rounds, [k for k in KEEP if getattr(self, k) is not None]))


def _check_water(water):
    water = Water() if water is None else water
    if not isinstance(water, Water):
        raise ValueError("water must be a Water, got %r" % (water,))
    return water


_as_plane = functools.partial(as_plane, raw=True)          # (route's intake too)


def analyse(ops, heightmap, tiled=None, keep=KEEP):
    """The hydrology of a heightmap: upload, the relaxations, one direction launch, the doubling rounds, download.
    ops: a device.Ops; heightmap: (H, W) or (1, H, W), floating point and finite, or uint8; tiled: the LDS form of the two
    relaxations (True) or the plain one (False): the same bits; default DEFAULT_TILED.  keep: the planes to download.
    Returns a Hydrology."""
    keep = check_keep(keep, KEEP)
    a = _as_plane(heightmap)
    H, W = a.shape
    tiled = DEFAULT_TILED if tiled is None else bool(tiled)
    n = H * W
    dev = ops.dev
    out = {}
    with scratch(dev) as alloc:
        d_h, d_f, d_d, d_dir, d_a, d_b, ws = [alloc(nbytes) for nbytes in (4 * n, 4 * n, 4 * n, n, 4 * n, 4 * n,
                                                                           ops.hydrology_workspace(H, W))]
        dev.h2d(d_h, a)
        fill_sweeps, _ = ops.hydrology_fill(d_h, H, W, W, tiled, d_f, W, ws)
        flat_sweeps = ops.hydrology_flats(d_f, H, W, W, tiled, d_d, W, ws)
        ops.hydrology_directions(d_f, W, d_d, W, H, W, d_dir, W)
        rounds = ops.hydrology_accumulate(d_dir, W, H, W, d_a, W, d_b, W, ws)
        dev.sync()
        for name, ptr, dtype in (('filled', d_f, np.float32), ('direction', d_dir, np.int8), ('accumulation', d_a, np.uint32),
                                 ('basin', d_b, np.int32)):
            if name in keep or (name == 'filled' and 'depth' in keep):
                out[name] = np.empty((H, W), dtype)
                dev.d2h(out[name], ptr, out[name].nbytes)
    if 'depth' in keep:
        out['depth'] = out['filled'] - a
    if 'filled' not in keep:
        out.pop('filled', None)
    return Hydrology((H, W), (fill_sweeps, flat_sweeps), rounds, tiled, **out)


def _texture_planes(texture, value_range):
    """a texture in one of the forms render.Scene takes -> (fp32 planes [C, H, W] to paint, unit, uint8): uint8 images through
    the scene's own map to [0, 1]; float32 ones validated by it and painted in their own value range (``unit``: [0, 1],
    otherwise the tanh range)"""
    from .render import _unit_planes
    a = np.asarray(texture)
    unit = bool(value_range) if value_range is not None else (a.ndim == 2 or a.shape[0] == 1)
    planes = _unit_planes(a, unit, "texture")
    if a.dtype == np.uint8:
        return planes, True, True
    return np.ascontiguousarray(a[None] if a.ndim == 2 else a), unit, False


def texture_colour(colour, unit):
    """the water's colour in the value range of a float texture: as it is, or mapped to the tanh range by the inverse of
    (127.5 v + 127.5) / 255, in float32"""
    c = np.asarray(colour, np.float32)
    if not unit:
        c = (c * np.float32(255) - np.float32(127.5)) / np.float32(127.5)
    return tuple(float(v) for v in c)


def paint(ops, texture, hydro, water=None, value_range=None):
    """The water of ``hydro`` (a Hydrology with ``depth`` and ``accumulation``) painted on a texture of the same size.
    texture: what render.Scene takes -- uint8 (H, W) / (H, W, C), or float32 (H, W) / (C, H, W), C = 1 or 3; value_range: whether
    a float texture is already in [0, 1] (True) or in the tanh range (False); None takes one channel as unit and three as tanh,
    like the scene.  water: a Water (default Water()).  Returns the painted texture in the form, dtype and value range it came
    in; dry pixels are bit-identical to the input."""
    water = _check_water(water)
    if not isinstance(hydro, Hydrology) or hydro.depth is None or hydro.accumulation is None:
        raise ValueError("hydro must be a Hydrology that kept 'depth' and 'accumulation'")
    return _paint(ops, texture, value_range, "hydrology", hydro.shape, hydro.depth, hydro.accumulation, water.river_threshold,
                  water.river_width, water.colour, water.opacity, water.lake_min_depth)


def _paint(ops, texture, value_range, noun, shape, depth, marks, threshold, width, colour, opacity, lake_min_depth=0.0):
    """the one paint, of water and of roads (route.paint): a pixel is marked where ``depth`` > lake_min_depth -- depth=None:
    a plane of zeros, which exceeds no minimum depth of 0 -- or where the largest of ``marks`` within ``width`` pixels is >=
    threshold, and blended towards ``colour`` with ``opacity``.  The texture's form, then its size against ``shape``
    (the ``noun``'s), are checked before the device is read; upload, one launch, download, in the texture's own form"""
    planes, unit, u8 = _texture_planes(texture, value_range)
    C_, H, W = planes.shape
    if (H, W) != tuple(shape):
        raise ValueError("texture %s and %s %s differ in size" % ((H, W), noun, tuple(shape)))
    depth = np.zeros((H, W), np.float32) if depth is None else np.ascontiguousarray(depth, np.float32)
    marks = np.ascontiguousarray(marks, np.uint32)
    res = np.empty((C_, H, W), np.uint8 if u8 else np.float32)
    dev = ops.dev
    with scratch(dev) as alloc:
        bufs = [alloc(x.nbytes) for x in (depth, marks, planes, res)]
        for p, x in zip(bufs, (depth, marks, planes)):
            dev.h2d(p, x)
        ops.hydrology_paint(bufs[0], W, bufs[1], W, H, W, bufs[2], W, C_, texture_colour(colour, unit), opacity,
                            lake_min_depth, threshold, width, u8, bufs[3], W)
        dev.sync()
        dev.d2h(res, bufs[3], res.nbytes)
    a = np.asarray(texture)
    if u8:
        return np.ascontiguousarray(res[0] if a.ndim == 2 else res.transpose(1, 2, 0))
    return res[0] if a.ndim == 2 else res


def _save_painted(path, painted):
    """what ``paint`` returned, as a PNG: uint8 as it is; a float texture with one channel as unit, with three as tanh"""
    from .util import convert_to_rgb, save_png, to_uint8
    if painted.dtype != np.uint8:
        planes = painted[None] if painted.ndim == 2 else painted
        painted = to_uint8(convert_to_rgb(planes, is_grayscale=planes.shape[0] == 1))
    save_png(path, painted[:, :, 0] if painted.ndim == 3 and painted.shape[2] == 1 else painted)


# ---- command line -------------------------------------------------------------------------------------------------------
def parse_args(argv):
    p = argparse.ArgumentParser(prog="python -m gan_heightmaps_amd.hydrology",
                                description="Fill the lakes of a heightmap, route the flow and accumulate the rivers (on the GPU).")
    p.add_argument("input", help="heightmap: 8-bit PNG (read as greyscale), or .npy (uint8 or float, (H, W))")
    p.add_argument("out_prefix", help="writes OUT_PREFIX.filled.npy, .depth.npy, .accumulation.npy, .direction.npy, .basin.npy")
    p.add_argument("--texture", help="a texture of the heightmap's size to paint the water on: PNG, or .npy")
    p.add_argument("--painted", help="the painted texture, as PNG (needs --texture)")
    d = Water()
    p.add_argument("--river-threshold", type=int, default=d.river_threshold,
                   help="cells of drainage area that make a river (default %d)" % d.river_threshold)
    p.add_argument("--river-width", type=int, default=d.river_width, help="pixels a river is widened by, 0 .. %d" % MAX_RIVER_WIDTH)
    p.add_argument("--lake-min-depth", type=float, default=d.lake_min_depth, help="filled depth above which a pixel is a lake")
    p.add_argument("--opacity", type=float, default=d.opacity, help="how far wet pixels go towards the water's colour, in [0, 1]")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--plain", action="store_true", help="one Jacobi sweep per launch")
    g.add_argument("--tiled", action="store_true", help="tiles swept in LDS (the same bits)")
    a = p.parse_args(argv)
    if (a.texture is None) != (a.painted is None):
        p.error("--texture and --painted go together")
    try:
        a.water = Water(river_threshold=a.river_threshold, river_width=a.river_width, lake_min_depth=a.lake_min_depth,
                        opacity=a.opacity)
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
        hydro = analyse(ops, x, tiled=a.form)
        painted = paint(ops, tex, hydro, a.water) if tex is not None else None
    finally:
        dev.close()
    for k in KEEP:
        np.save("%s.%s.npy" % (a.out_prefix, k), getattr(hydro, k))
    if painted is not None:
        _save_painted(a.painted, painted)
    return 0


if __name__ == "__main__":
    sys.exit(main())
