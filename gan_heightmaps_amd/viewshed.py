"""Viewshed: which cells of a heightmap a set of observers can see, by exact lines of sight, on the device (csrc/viewshed.hip,
DESIGN §4x).  The hydrology (§4t) says where water runs and the routes (§4u) what it costs to travel; this is the third raster
analysis, visibility.  Integers throughout, and equal to a definition in numpy (tests/viewshed_ref.py) bit for bit.

The plane is h[H, W], float32, finite and in [0, 1] (uint8 is read as v / 255).

1. The heights are quantised to 1/256 cell: zq = int32(rint(h float32(height_scale 256))), one float32 product, rounded once.
2. An observer is (row, col, eye_q, radius2): eye_q = rint(eye_height 256), radius2 = floor(max_dist^2) or -1 for no limit.
3. The line of sight from O = (r0, c0) to T = (r, c) takes n = max(|dy|, |dx|) steps along its major axis.  Step k = 1 .. n - 1
   stands q, f = divmod(k m, n) along the minor axis (m the other delta's magnitude), between cell a and, if f > 0, the next cell
   b; it blocks iff zq[a] (n - f) + zq[b] f - E n > k D, with E = zq[O] + eye_q and D = zq[T] + target_q - E.  T is seen iff no
   step blocks and T lies within the radius; grazing is seeing.  With eye_height == target_height seeing is symmetric.  A sight
   line reads only cells of the bounding box of O and T: visibility between two cells is a property of the ground between
   them, not of the plane they were cut from.
4. ``count`` is the number of observers that see a cell, ``mask`` has bit i for observer i (up to 32 observers).  Two device
   forms with the same bits: ``plain`` marches every step; ``accel`` jumps runs of steps that the maxima of 16 x 16 blocks
   prove clear (csrc/viewshed.hip has the proof).

    python -m gan_heightmaps_amd.viewshed IN OUT.{npz,png} --from R,C[,EYE[,DIST]] [--from ...] [--eye X] [--target X]
        [--max-dist X] [--height-scale X] [--texture F --painted OUT [--hidden] [--colour R,G,B] [--opacity X]] [--plain | --accel]
"""
import argparse
import dataclasses
import math
import sys

import numpy as np

from . import hydrology as _hy
from .planes import as_plane, check_keep, scratch
from .util import form_choice, is_int as _is_int, is_number as _number, read_image

__all__ = ["BLOCK", "DEFAULT_ACCEL", "KEEP", "MAX_HEIGHT", "MAX_OBSERVERS", "Sight", "Viewshed", "observer_table", "viewshed", "paint",
           "parse_observer", "parse_args", "main"]

BLOCK = 16                   # GHM_VIEWSHED_BLOCK (include/ghm.h)
MAX_OBSERVERS = 4096         # GHM_VIEWSHED_MAX_OBSERVERS
MAX_HEIGHT = 65536.0         # of height_scale, eye_height and target_height: zq, eye_q and target_q stay <= 2^24
KEEP = ('zq',)
# the form ``viewshed`` runs by default: the one tools/viewshed_bench.py shows faster on the MI355X -- the accel one, on a
# 4096 x 4096 plane of value noise 0.075 against 0.139 ms for one observer within 256 cells, 2.04 against 14.3 ms for one without a
# limit, 13.9 against 75.6 ms for 64 within 1024 cells and 117 against 872 ms for 64 without a limit: it tests 4 to 24 % of the plain
# form's steps (DESIGN §4x has the line); both give the same bits
DEFAULT_ACCEL = True


def _check_origin(origin):
    try:
        r, c = origin
        ok = _is_int(r) and _is_int(c) and abs(int(r)) < 1 << 62 and abs(int(c)) < 1 << 62
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("origin must be (row, col), two integers, got %r" % (origin,))
    return int(r), int(c)


def _check_height(v, name):
    if not _number(v) or not 0 <= v <= MAX_HEIGHT:
        raise ValueError("%s must be a number in [0, %g], got %r" % (name, MAX_HEIGHT, v))
    return float(v)


def _check_dist(v, name="max_dist"):
    if v is None:
        return None
    if not _number(v) or v < 0:
        raise ValueError("%s must be None or a number >= 0, got %r" % (name, v))
    return float(v)


def quantum(height):
    """a height in cells -> units of 1/256 cell: rint(height 256), half to even"""
    return int(np.rint(float(height) * 256.0))


def _radius2(max_dist, H, W):
    """floor(max_dist^2), or -1 for no limit -- also where the radius covers every pair of cells of the plane"""
    if max_dist is None:
        return -1
    r2 = int(math.floor(max_dist * max_dist))
    if r2 >= (H - 1) ** 2 + (W - 1) ** 2:
        return -1
    return r2


@dataclasses.dataclass(frozen=True)
class Sight:
    """How the observers look, validated and frozen.  ``eye_height``: cells above the ground at the observer, in [0, 65536] (an
    observer may bring its own); ``target_height``: cells above the ground at the target, in [0, 65536]; ``max_dist``: None, or the
    distance in cells beyond which nothing counts as seen (dy^2 + dx^2 <= floor(max_dist^2); an observer may bring its own);
    ``height_scale``: cells of height per unit of the heightmap, in (0, 65536].  Heights are kept to 1/256 cell.  The defaults are
    chosen, not measured."""
    eye_height: float = 2.0
    target_height: float = 0.0
    max_dist: object = None
    height_scale: float = 64.0

    def __post_init__(self):
        object.__setattr__(self, "eye_height", _check_height(self.eye_height, "eye_height"))
        object.__setattr__(self, "target_height", _check_height(self.target_height, "target_height"))
        object.__setattr__(self, "max_dist", _check_dist(self.max_dist))
        if not _number(self.height_scale) or not 0 < self.height_scale <= MAX_HEIGHT:
            raise ValueError("height_scale must be a number in (0, %g], got %r" % (MAX_HEIGHT, self.height_scale))
        object.__setattr__(self, "height_scale", float(self.height_scale))

    @property
    def eye_q(self):
        return quantum(self.eye_height)

    @property
    def target_q(self):
        return quantum(self.target_height)


def _check_sight(sight):
    sight = Sight() if sight is None else sight
    if not isinstance(sight, Sight):
        raise ValueError("sight must be a Sight, got %r" % (sight,))
    return sight


def _observer_fields(i, o, sight):
    """(row, col, eye_height, max_dist) of observer i, what it leaves out (or gives as None) taken from the ``sight``"""
    if not 2 <= len(o) <= 4 or not _is_int(o[0]) or not _is_int(o[1]):
        raise ValueError("observer %d must be (row, col[, eye_height[, max_dist]]) with an integer row and col, got %r" % (i, o))
    eye = sight.eye_height if len(o) < 3 or o[2] is None else _check_height(o[2], "observer %d's eye_height" % i)
    dist = sight.max_dist if len(o) < 4 or o[3] is None else _check_dist(o[3], "observer %d's max_dist" % i)
    return int(o[0]), int(o[1]), eye, dist


def observer_table(observers, sight, shape, origin=(0, 0)):
    """The host's table of the observers, int32 [n, 4] of (row, col, eye_q, radius2) in the plane's own coordinates.  observers:
    1 .. 4096 of (row, col), (row, col, eye_height) or (row, col, eye_height, max_dist), in ``origin``'s coordinates and inside
    the plane of ``shape``; what an observer leaves out (or gives as None) is the ``sight``'s."""
    H, W = shape
    try:
        rows = [tuple(o) for o in observers]
    except TypeError:
        rows = None
    if not rows or len(rows) > MAX_OBSERVERS:
        raise ValueError("observers must be 1 .. %d of (row, col[, eye_height[, max_dist]]), got %r" % (
            MAX_OBSERVERS, observers if rows is None or not rows else len(rows)))
    out = np.empty((len(rows), 4), np.int64)
    for i, o in enumerate(rows):
        row, col, eye, dist = _observer_fields(i, o, sight)
        r, c = row - origin[0], col - origin[1]
        if not (0 <= r < H and 0 <= c < W):
            raise ValueError("observer %d at (%d, %d) lies outside the plane of %d x %d at %r" % (i, row, col, H, W, tuple(origin)))
        out[i] = (r, c, quantum(eye), _radius2(dist, H, W))
    if out[:, 3].max() >= 1 << 31:                   # a plane longer than 46340 cells and a radius that cuts it beyond them
        raise ValueError("max_dist: a radius beyond 46340 cells must cover the plane")
    return out.astype(np.int32)


class Viewshed:
    """What ``viewshed`` returns: ``count`` uint32 (H, W), the number of observers that see each cell; ``mask`` uint32 (H, W), bit
    i for observer i, or None beyond 32 observers; ``observers`` int32 [n, 4], (row, col, eye_q, radius2) with row and col in
    ``origin``'s coordinates; ``origin``, the coordinates of cell [0, 0]; ``sight``; the form ``accel``; ``zq`` if it was kept."""

    def __init__(self, count, mask, observers, origin, sight, accel, zq=None):
        self.count, self.mask, self.observers, self.sight, self.accel, self.zq = count, mask, observers, sight, accel, zq
        self.origin = (int(origin[0]), int(origin[1]))

    @property
    def shape(self):
        return tuple(self.count.shape)

    def __len__(self):
        return int(self.observers.shape[0])

    def __repr__(self):
        return "Viewshed(%d x %d at %r, %d observers, %.1f %% seen)" % (self.shape + (self.origin, len(self), 100.0 * self.share()))

    def visible(self, i):
        """bool (H, W): what observer i sees (from the mask: up to 32 observers)"""
        if not _is_int(i) or not 0 <= i < len(self):
            raise ValueError("observer %r: there are %d" % (i, len(self)))
        if self.mask is None:
            raise ValueError("beyond 32 observers no mask is kept: run observer %d on its own" % i)
        return (self.mask >> np.uint32(i)) & np.uint32(1) != 0

    def seen(self):
        """bool (H, W): the cells at least one observer sees"""
        return self.count > 0

    def share(self):
        """the share of the cells that at least one observer sees"""
        return float(self.seen().mean())

    def save(self, path):
        """.npz: count, mask (if any), observers, origin; .png: 8-bit greyscale, 255 on the cells that are seen, 0 on the others"""
        if path.endswith(".npz"):
            out = dict(count=self.count, observers=self.observers, origin=np.array(self.origin, np.int64))
            if self.mask is not None:
                out["mask"] = self.mask
            np.savez(path, **out)
        elif path.lower().endswith(".png"):
            from .util import save_png
            save_png(path, self.seen().astype(np.uint8) * np.uint8(255))
        else:
            raise ValueError("a viewshed is saved as .npz or .png, got %r" % (path,))


def viewshed(ops, heightmap, observers, sight=None, accel=None, origin=(0, 0), keep=()):
    """What the observers see of a heightmap: upload, the quantisation, (accel) the block maxima, the sight lines, download.
    ops: a device.Ops; heightmap: (H, W) or (1, H, W), floating point, finite and in [0, 1], or uint8; observers: 1 .. 4096 of
    (row, col), (row, col, eye_height) or (row, col, eye_height, max_dist) in ``origin``'s coordinates, inside the plane; sight:
    a Sight (default Sight()); accel: jump the runs of steps that block maxima prove clear (True) or march every step (False):
    the same bits; default DEFAULT_ACCEL; origin: the coordinates of cell [0, 0]; keep: 'zq', to return the quantised heights.
    Returns a Viewshed."""
    keep = check_keep(keep, KEEP)
    sight = _check_sight(sight)
    origin = _check_origin(origin)
    a = as_plane(heightmap, unit_range=True, raw=True)
    H, W = a.shape
    table = observer_table(observers, sight, (H, W), origin)
    accel = DEFAULT_ACCEL if accel is None else bool(accel)
    n = H * W
    masked = len(table) <= 32
    count = np.empty((H, W), np.uint32)
    mask = np.empty((H, W), np.uint32) if masked else None
    zq = np.empty((H, W), np.int32) if 'zq' in keep else None
    dev = ops.dev
    with scratch(dev) as alloc:
        d_h, d_z, d_c = alloc(4 * n), alloc(4 * n), alloc(4 * n)
        d_m = alloc(4 * n) if masked else None
        dev.h2d(d_h, a)
        ops.viewshed_quantise(d_h, W, H, W, sight.height_scale, d_z, W)
        d_t = None
        if accel:
            elems = ops.viewshed_top_elems(H, W)
            d_t = alloc(4 * elems)
            ops.viewshed_top(d_z, W, H, W, d_t, elems)
        ops.viewshed_sight(d_z, W, H, W, table, sight.target_q, accel, d_t, d_c, W, d_m, W)
        dev.sync()
        dev.d2h(count, d_c, count.nbytes)
        if masked:
            dev.d2h(mask, d_m, mask.nbytes)
        if zq is not None:
            dev.d2h(zq, d_z, zq.nbytes)
    world = table.copy()
    world[:, 0] += origin[0]
    world[:, 1] += origin[1]
    return Viewshed(count, mask, world, origin, sight, accel, zq)


def _check_colour(colour):
    try:
        ok = len(colour) == 3 and all(_number(v) and 0 <= v <= 1 for v in colour)
    except TypeError:
        ok = False
    if not ok:
        raise ValueError("colour must be three numbers in [0, 1], got %r" % (colour,))
    return tuple(float(v) for v in colour)


def _check_opacity(opacity):
    if not _number(opacity) or not 0 <= opacity <= 1:
        raise ValueError("opacity must lie in [0, 1], got %r" % (opacity,))
    return float(opacity)


def paint(ops, texture, seen, colour=(1.0, 0.85, 0.2), opacity=0.5, hidden=False, value_range=None):
    """The ground a Viewshed's observers see -- hidden=True: the ground none of them sees -- painted on a texture of its size
    with the hydrology's paint kernel: such a pixel is blended towards ``colour`` (three numbers in [0, 1]) with ``opacity``.
    texture, value_range and the result: as hydrology.paint's; unpainted pixels keep their bits."""
    if not isinstance(seen, Viewshed):
        raise ValueError("viewshed must be a Viewshed, got %r" % (seen,))
    colour, opacity = _check_colour(colour), _check_opacity(opacity)
    marks = (seen.seen() != bool(hidden)).astype(np.uint32)
    return _hy._paint(ops, texture, value_range, "viewshed", seen.shape, None, marks, 1, 0, colour, opacity)


# ---- command line -------------------------------------------------------------------------------------------------------
def parse_observer(text):
    """R,C[,EYE[,DIST]] -> (row, col[, eye_height[, max_dist]])"""
    parts = [t.strip() for t in text.split(",")]
    try:
        if not 2 <= len(parts) <= 4:
            raise ValueError
        return (int(parts[0]), int(parts[1])) + tuple(float(t) for t in parts[2:])
    except ValueError:
        raise argparse.ArgumentTypeError("an observer is R,C[,EYE[,DIST]] (two integers and up to two numbers), got %r" % (text,))


def _colour(text):
    try:
        v = tuple(float(t) for t in text.split(","))
    except ValueError:
        v = ()
    if len(v) != 3:
        raise argparse.ArgumentTypeError("3 numbers separated by commas, got %r" % (text,))
    return v


def parse_args(argv):
    p = argparse.ArgumentParser(prog="python -m gan_heightmaps_amd.viewshed",
                                description="What a set of observers can see of a heightmap, by exact lines of sight (on the GPU).")
    p.add_argument("input", help="heightmap: 8-bit PNG (read as greyscale), or .npy (uint8 or float in [0, 1], (H, W))")
    p.add_argument("output", help="the viewshed: .npz (count, mask, observers) or .png (255 where seen)")
    d = Sight()
    p.add_argument("--from", dest="observers", type=parse_observer, action="append", metavar="R,C[,EYE[,DIST]]", required=True,
                   help="an observer: its cell, and optionally its own eye height and distance limit; repeat for more")
    p.add_argument("--eye", type=float, default=d.eye_height, help="cells the eye is above the ground (default %g)" % d.eye_height)
    p.add_argument("--target", type=float, default=d.target_height, help="cells a target is above the ground (default 0)")
    p.add_argument("--max-dist", type=float, default=None, help="cells beyond which nothing counts as seen (default: no limit)")
    p.add_argument("--height-scale", type=float, default=d.height_scale, help="cells of height per unit of the heightmap")
    p.add_argument("--texture", default=None, metavar="F", help="a texture of the heightmap's size to paint the seen ground on")
    p.add_argument("--painted", default=None, metavar="OUT", help="where the painted texture goes (PNG)")
    p.add_argument("--hidden", action="store_true", help="paint the ground nobody sees instead")
    p.add_argument("--colour", type=_colour, default=(1.0, 0.85, 0.2), metavar="R,G,B", help="the paint's colour, in [0, 1]")
    p.add_argument("--opacity", type=float, default=0.5, help="how far painted pixels go towards the colour, in [0, 1]")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--plain", action="store_true", help="march every step of every sight line")
    g.add_argument("--accel", action="store_true", help="jump runs of steps that block maxima prove clear (the same bits)")
    # an observer that starts with a negative number would read as an option: hand it over in the --from=... form
    argv = list(argv)
    for i in range(len(argv) - 2, -1, -1):
        if argv[i] == "--from" and argv[i + 1].lstrip()[:1] == "-" and argv[i + 1].lstrip()[1:2].isdigit():
            argv[i:i + 2] = ["--from=" + argv[i + 1]]
    a = p.parse_args(argv)
    if (a.texture is None) != (a.painted is None):
        p.error("--texture and --painted go together")
    if a.hidden and a.texture is None:
        p.error("--hidden needs --texture and --painted")
    if not (a.output.endswith(".npz") or a.output.lower().endswith(".png")):
        p.error("the output is .npz or .png")
    try:
        a.sight = Sight(a.eye, a.target, a.max_dist, a.height_scale)
        for i, o in enumerate(a.observers):                                # the fields; the plane comes later
            _observer_fields(i, o, a.sight)
        _check_colour(a.colour)
        _check_opacity(a.opacity)
    except ValueError as e:
        p.error(str(e))
    a.form = form_choice(a.accel, a.plain)
    return a


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    from .device import Device, Ops
    x = read_image(a.input, "L", mmap=False)
    texture = None if a.texture is None else read_image(a.texture, mmap=False)
    dev = Device(0)
    try:
        ops = Ops(dev)
        seen = viewshed(ops, x, a.observers, a.sight, accel=a.form)
        painted = None if texture is None else paint(ops, texture, seen, a.colour, a.opacity, a.hidden)
    finally:
        dev.close()
    seen.save(a.output)
    if painted is not None:
        _hy._save_painted(a.painted, painted)
    print("%d observers see %d of %d cells" % (len(seen), int(seen.seen().sum()), seen.count.size))
    return 0


if __name__ == "__main__":
    sys.exit(main())
