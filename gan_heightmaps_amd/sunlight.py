"""Sunlight: for a list of sun positions -- a day's, or any -- which of them light each cell of a heightmap, for how many hours, and
how much energy the cell's slope receives, by exact shadow rays on the device (csrc/sunlight.hip).  The viewshed (§4x)
says what can be seen and the skylight (§4s) how much of the sky a texel receives; this says where the sun shines.  Integers
throughout, and equal to a definition in plain Python (tests/sunlight_ref.py) bit for bit.

The plane is h[H, W], float32, finite and in [0, 1] (uint8 is read as v / 255).

1. The heights are the viewshed's: zq = int32(rint(h float32(height_scale 256))), in 1/256 cell.
2. A sun position is (azimuth, elevation, hours), in render.Scene.render's convention: the direction to the sun is (dy, dx, dz) =
   (cos el cos az, cos el sin az, sin el), y down the rows.  The host turns it, in float64 and rounded once per entry, into
   (rows, gmaj, gmin, m_q, rise_q, s_y, s_x, s_z, w_q): the ray's major axis and the signs of its steps, m_q = rint(65536 |minor| /
   |major|) of the azimuth's two components, rise_q = clamp(rint(65536 tan(el) / |major|), 1, 2^40), s = rint(2^14 (dy, dx, dz)),
   w_q = rint(256 hours).
3. The shadow ray of cell T: for k = 1, 2, ... ray = 256 (zq[T] + target_q) + k rise_q; q, f = divmod(k m_q, 65536); cell a lies k
   major and q minor steps from T, cell b one minor step further.  The ray ends lit at the first k whose a (or b, if f > 0) lies
   outside the plane, in shadow at the first k with zq[a] (65536 - f) + zq[b] f > 256 ray; grazing is lit.
4. The slope: g_y = zq[r + 1, c] - zq[r - 1, c], g_x likewise (indices clamped), n = (-g_y, -g_x, 512), norm = floor(|n|), dot = n . s.
   A cell with dot <= 0 shades itself and casts no ray.
5. ``lit`` counts the positions that light a cell, ``mask`` has bit i for position i (up to 32 positions), ``hours_q`` sums their
   w_q and ``energy`` their (w_q dot) // norm.  Two device forms with the same bits: ``plain`` marches every step; ``accel`` jumps
   runs of steps that the maxima of 16 x 16 blocks prove clear (csrc/sunlight.hip has the proof).
6. ``Sun.reach`` = ceil(256 rint(256 height_scale) / min rise_q) + 1 cells: no ray reads further from its cell before it clears
   any terrain the height scale allows, so a window grown by the reach gives the larger map's planes bit for bit.

    python -m gan_heightmaps_amd.sunlight IN OUT.{npz,png} (--sun AZ,EL[,HOURS] ... | --day [--latitude X --declination X
        --step-minutes N --min-elevation X]) [--target X] [--height-scale X]
        [--texture F --painted OUT [--max-hours X --colour R,G,B --opacity X]] [--plain | --accel]
"""
import argparse
import dataclasses
import math
import sys

import numpy as np

from . import hydrology as _hy
from .planes import as_plane, check_keep, scratch
from .util import is_int as _is_int, is_number as _number, read_image
from .viewshed import MAX_HEIGHT, _check_colour, _check_height, _check_opacity, _check_origin, _colour, quantum

__all__ = ["DEFAULT_FORM", "FORMS", "KEEP", "MAX_POSITIONS", "MAX_WEIGHT", "Day", "Sun", "Sunlight", "sunlight", "paint", "parse_sun",
           "parse_args", "main"]

MAX_POSITIONS = 4096         # GHM_SUNLIGHT_MAX_POSITIONS (include/ghm.h)
MAX_WEIGHT = 1 << 17         # GHM_SUNLIGHT_MAX_WEIGHT: the w_q of a Sun sum to at most this, so that energy fits 32 bits
MAX_RISE = 1 << 40
ONE = 65536
KEEP = ('zq',)
FORMS = ('plain', 'accel')
# the form ``sunlight`` runs by default: the one tools/sunlight_bench.py shows faster under Day() on the MI355X -- the accel one, on a
# 4096 x 4096 plane of value noise at height scale 64 15.08 against 33.92 ms under Day() (24 positions), 0.454 against 0.572 ms under
# one sun 28 degrees up and 1.914 against 5.417 ms under one 3 degrees up: it tests 4 to 5 % of the plain form's steps (one run,
# medians of 5; DESIGN §4zd has the line); both give the same bits
DEFAULT_FORM = 'accel'


def _position(i, p):
    try:
        p = tuple(p)
    except TypeError:
        p = ()
    if not 2 <= len(p) <= 3:
        raise ValueError("positions: position %d must be (azimuth, elevation[, hours]), got %r" % (i, p))
    az, el = p[0], p[1]
    hours = 1.0 if len(p) < 3 else p[2]
    if not _number(az) or not math.isfinite(az) or abs(az) > 1e6:
        raise ValueError("azimuth of position %d must be a finite number of degrees, got %r" % (i, az))
    if not _number(el) or not 0 < el <= 90:
        raise ValueError("elevation of position %d must lie in (0, 90] degrees, got %r" % (i, el))
    if not _number(hours) or not 0 <= hours <= MAX_WEIGHT / 256.0:
        raise ValueError("hours of position %d must lie in [0, %g], got %r" % (i, MAX_WEIGHT / 256.0, hours))
    return float(az), float(el), float(hours)


def _row(az, el, hours):
    """one row of the table, in float64, every entry rounded once (tests/sunlight_ref.position restates it)"""
    a, e = math.radians(az), math.radians(el)
    hy, hx = math.cos(a), math.sin(a)
    rows = abs(hy) >= abs(hx)
    major, minor = (hy, hx) if rows else (hx, hy)
    m_q = int(np.rint(ONE * abs(minor) / abs(major)))
    rise_q = int(min(max(np.rint(ONE * math.tan(e) / abs(major)), 1.0), float(MAX_RISE)))
    c = math.cos(e)
    return (int(rows), 1 if major > 0 else -1, 0 if m_q == 0 else (1 if minor > 0 else -1), m_q, rise_q, int(np.rint(16384 * c * hy)),
            int(np.rint(16384 * c * hx)), int(np.rint(16384 * math.sin(e))), int(np.rint(256 * hours)))


@dataclasses.dataclass(frozen=True)
class Sun:
    """Where the sun stands, validated and frozen.  ``positions``: 1 .. 4096 of (azimuth_deg, elevation_deg[, hours = 1]) in
    render.Scene.render's convention -- the direction to the sun is (cos el cos az, cos el sin az, sin el) along (y, x, z), y down
    the rows -- with the elevation in (0, 90] and hours that sum to at most 512; ``target_height``: cells above the ground at
    which a cell counts as lit, in [0, 65536]; ``height_scale``: cells of height per unit of the heightmap, in (0, 65536].  The
    defaults are chosen, not measured."""
    positions: tuple
    target_height: float = 0.0
    height_scale: float = 64.0

    def __post_init__(self):
        try:
            rows = list(self.positions)
        except TypeError:
            rows = None
        if not rows or len(rows) > MAX_POSITIONS:
            raise ValueError("positions must be 1 .. %d of (azimuth, elevation[, hours]), got %r" % (
                MAX_POSITIONS, self.positions if not rows else len(rows)))
        rows = tuple(_position(i, p) for i, p in enumerate(rows))
        object.__setattr__(self, "positions", rows)
        if sum(int(np.rint(256 * p[2])) for p in rows) > MAX_WEIGHT:
            raise ValueError("hours: the positions' hours sum to more than %g" % (MAX_WEIGHT / 256.0))
        object.__setattr__(self, "target_height", _check_height(self.target_height, "target_height"))
        if not _number(self.height_scale) or not 0 < self.height_scale <= MAX_HEIGHT:
            raise ValueError("height_scale must be a number in (0, %g], got %r" % (MAX_HEIGHT, self.height_scale))
        object.__setattr__(self, "height_scale", float(self.height_scale))

    def __len__(self):
        return len(self.positions)

    @property
    def target_q(self):
        return quantum(self.target_height)

    def table(self):
        """int64 [n, 9] of (rows, gmaj, gmin, m_q, rise_q, s_y, s_x, s_z, w_q)"""
        return np.array([_row(*p) for p in self.positions], np.int64).reshape(-1, 9)

    @property
    def reach(self):
        """the cells a ray can read away from its cell before it clears any terrain the height scale allows"""
        rise = int(self.table()[:, 4].min())
        return -(-256 * int(np.rint(256.0 * self.height_scale)) // rise) + 1

    @property
    def level(self):
        """the energy of an unshaded level cell, sum of w_q s_z"""
        t = self.table()
        return int((t[:, 8] * t[:, 7]).sum())


@dataclasses.dataclass(frozen=True)
class Day:
    """The sun's path over one day, a host helper in float64.  ``latitude`` and ``declination`` in degrees (declination 0: an
    equinox, +23.44: the northern midsummer); the day's 24 hours are cut into steps of ``step_minutes`` (a divisor of 1440) and the
    sun stands at each step's midpoint; the positions at or above ``min_elevation`` degrees are kept, each with hours = the step.
    North is up the rows, so a compass bearing b maps to the azimuth 180 - b.  The defaults are chosen, not measured."""
    latitude: float = 45.0
    declination: float = 0.0
    step_minutes: int = 30
    min_elevation: float = 2.0

    def __post_init__(self):
        if not _number(self.latitude) or not -90 <= self.latitude <= 90:
            raise ValueError("latitude must lie in [-90, 90] degrees, got %r" % (self.latitude,))
        if not _number(self.declination) or not -90 <= self.declination <= 90:
            raise ValueError("declination must lie in [-90, 90] degrees, got %r" % (self.declination,))
        if not _is_int(self.step_minutes) or not 1 <= self.step_minutes <= 720 or 1440 % int(self.step_minutes):
            raise ValueError("step_minutes must be an integer divisor of 1440 in 1 .. 720, got %r" % (self.step_minutes,))
        if not _number(self.min_elevation) or not 0 < self.min_elevation <= 90:
            raise ValueError("min_elevation must lie in (0, 90] degrees, got %r" % (self.min_elevation,))
        object.__setattr__(self, "latitude", float(self.latitude))
        object.__setattr__(self, "declination", float(self.declination))
        object.__setattr__(self, "step_minutes", int(self.step_minutes))
        object.__setattr__(self, "min_elevation", float(self.min_elevation))

    def position(self, hour):
        """(azimuth, elevation) in degrees at the local solar time ``hour`` (12: noon); the elevation may be negative"""
        lat, dec, ha = math.radians(self.latitude), math.radians(self.declination), math.radians(15.0 * (float(hour) - 12.0))
        up = math.sin(lat) * math.sin(dec) + math.cos(lat) * math.cos(dec) * math.cos(ha)
        east = -math.cos(dec) * math.sin(ha)
        north = math.sin(dec) * math.cos(lat) - math.cos(dec) * math.sin(lat) * math.cos(ha)
        bearing = math.degrees(math.atan2(east, north))
        return (180.0 - bearing) % 360.0, math.degrees(math.asin(max(-1.0, min(1.0, up))))

    def positions(self):
        """((azimuth, elevation, hours), ...) of the steps whose midpoint stands at or above min_elevation"""
        step = self.step_minutes / 60.0
        out = []
        for i in range(1440 // self.step_minutes):
            az, el = self.position((i + 0.5) * step)
            if el >= self.min_elevation:
                out.append((az, min(el, 90.0), step))
        return tuple(out)

    def sun(self, target_height=0.0, height_scale=64.0):
        at = self.positions()
        if not at:
            raise ValueError("min_elevation: the sun never stands %g degrees high at latitude %g and declination %g" % (
                self.min_elevation, self.latitude, self.declination))
        return Sun(at, target_height, height_scale)


def _check_sun(sun):
    sun = Day().sun() if sun is None else sun
    if not isinstance(sun, Sun):
        raise ValueError("sun must be a Sun, got %r" % (sun,))
    return sun


def _check_form(form):
    if form is None:
        return DEFAULT_FORM
    if form not in FORMS:
        raise ValueError("form must be one of %r, got %r" % (FORMS, form))
    return form


class Sunlight:
    """What ``sunlight`` returns, planes of (H, W): ``lit`` uint32, the positions that light each cell; ``mask`` uint32, bit i for
    position i, or None beyond 32 positions; ``hours_q`` uint32, their hours in 1/256; ``energy`` uint32, the sum of (w_q dot) //
    norm over them; ``sun``; ``origin``, the coordinates of cell [0, 0]; ``form``; ``exact``: False where a world's rectangle was
    analysed with a margin below the sun's reach, so that the planes belong to the rectangle; ``zq`` if it was kept."""

    def __init__(self, lit, mask, hours_q, energy, sun, origin=(0, 0), form=None, exact=True, zq=None):
        self.lit, self.mask, self.hours_q, self.energy, self.sun, self.form, self.zq = lit, mask, hours_q, energy, sun, form, zq
        self.origin = (int(origin[0]), int(origin[1]))
        self.exact = bool(exact)

    @property
    def shape(self):
        return tuple(self.lit.shape)

    def __len__(self):
        return len(self.sun)

    def __repr__(self):
        s = self.share()
        return "Sunlight(%d x %d at %r, %d positions, %.1f %% lit at some time, %.2f hours on average)" % (
            self.shape + (self.origin, len(self), 100.0 * s["lit"], s["mean_hours"]))

    def hours(self):
        """float64 (H, W): the hours of direct sun"""
        return self.hours_q.astype(np.float64) / 256.0

    def insolation(self):
        """float64 (H, W): the energy on the cell's slope in full-sun hours, one being an hour of sun straight along the normal"""
        return self.energy.astype(np.float64) / float(1 << 22)

    def exposure(self):
        """float64 (H, W): the insolation over that of an unshaded level cell under the same sun"""
        level = self.sun.level
        if level <= 0:
            raise ValueError("exposure: a level cell receives nothing under this sun")
        return self.energy.astype(np.float64) / float(level)

    def shaded(self, i):
        """bool (H, W): the cells position i does not light (from the mask: up to 32 positions)"""
        if not _is_int(i) or not 0 <= i < len(self):
            raise ValueError("position %r: there are %d" % (i, len(self)))
        if self.mask is None:
            raise ValueError("beyond 32 positions no mask is kept: run position %d on its own" % i)
        return (self.mask >> np.uint32(i)) & np.uint32(1) == 0

    def mask_hours(self, min_hours):
        """bool (H, W): the cells with at least ``min_hours`` of direct sun -- ``scatter_heightmap(blocked=~...)`` keeps a species
        on them, and it serves as a routes ``penalty=``"""
        if not _number(min_hours) or min_hours < 0:
            raise ValueError("min_hours must be a number >= 0, got %r" % (min_hours,))
        return self.hours_q.astype(np.int64) >= int(np.rint(256.0 * float(min_hours)))

    def share(self):
        """a summary: the share of the cells some position lights, the mean and the largest hours, the mean exposure"""
        level = self.sun.level
        return dict(lit=float((self.lit > 0).mean()), mean_hours=float(self.hours().mean()), max_hours=float(self.hours().max()),
                    mean_exposure=float(self.energy.astype(np.float64).mean() / level) if level > 0 else 0.0)

    def crop(self, r0, c0, h, w, exact=True):
        """the rectangle of h x w cells at (r0, c0) of these planes as a Sunlight of its own"""
        s = (slice(r0, r0 + h), slice(c0, c0 + w))

        def cut(p):
            return None if p is None else np.ascontiguousarray(p[s])
        return Sunlight(cut(self.lit), cut(self.mask), cut(self.hours_q), cut(self.energy), self.sun,
                        (self.origin[0] + r0, self.origin[1] + c0), self.form, exact and self.exact, cut(self.zq))

    def save(self, path):
        """.npz: lit, mask (if any), hours_q, energy, table, origin; .png: 8-bit greyscale, the hours over the sun's total"""
        if path.endswith(".npz"):
            out = dict(lit=self.lit, hours_q=self.hours_q, energy=self.energy, table=self.sun.table(),
                       origin=np.array(self.origin, np.int64), exact=np.array(self.exact))
            if self.mask is not None:
                out["mask"] = self.mask
            np.savez(path, **out)
        elif path.lower().endswith(".png"):
            from .util import save_png
            total = max(int(self.sun.table()[:, 8].sum()), 1)
            save_png(path, np.rint(self.hours_q.astype(np.float64) * (255.0 / total)).astype(np.uint8))
        else:
            raise ValueError("sunlight is saved as .npz or .png, got %r" % (path,))


def sunlight(ops, heightmap, sun=None, form=None, origin=(0, 0), keep=()):
    """Where the sun shines on a heightmap: upload, the viewshed's quantisation and block maxima, their maximum, the shadow rays,
    download, inside one scratch.  ops: a device.Ops; heightmap: (H, W) or (1, H, W), floating point, finite and in [0, 1], or
    uint8; sun: a Sun (default Day().sun()); form: 'plain' marches every step, 'accel' jumps the runs of steps that block maxima
    prove clear: the same bits; default DEFAULT_FORM; origin: the coordinates of cell [0, 0]; keep: 'zq', to return the
    quantised heights.  Returns a Sunlight."""
    keep = check_keep(keep, KEEP)
    sun = _check_sun(sun)
    form = _check_form(form)
    origin = _check_origin(origin)
    a = as_plane(heightmap, unit_range=True, raw=True)
    H, W = a.shape
    table = sun.table()
    n = H * W
    masked = len(table) <= 32
    lit, hours_q, energy = (np.empty((H, W), np.uint32) for _ in range(3))
    mask = np.empty((H, W), np.uint32) if masked else None
    zq = np.empty((H, W), np.int32) if 'zq' in keep else None
    dev = ops.dev
    with scratch(dev) as alloc:
        d_h, d_z, d_l, d_q, d_e = (alloc(4 * n) for _ in range(5))
        d_m = alloc(4 * n) if masked else None
        elems = ops.viewshed_top_elems(H, W)
        d_t, d_x = alloc(4 * elems), alloc(4)
        dev.h2d(d_h, a)
        ops.viewshed_quantise(d_h, W, H, W, sun.height_scale, d_z, W)
        ops.viewshed_top(d_z, W, H, W, d_t, elems)
        ops.sunlight_zmax(d_t, elems, d_x)
        ops.sunlight_sun(d_z, W, H, W, table, sun.target_q, form == 'accel', d_t, d_x, d_l, W, d_m, W, d_q, W, d_e, W)
        dev.sync()
        for host, ptr in ((lit, d_l), (hours_q, d_q), (energy, d_e), (mask, d_m), (zq, d_z)):
            if host is not None:
                dev.d2h(host, ptr, host.nbytes)
    return Sunlight(lit, mask, hours_q, energy, sun, origin, form, True, zq)


def paint(ops, texture, light, max_hours, colour=(0.05, 0.05, 0.2), opacity=0.5, value_range=None):
    """The cells of a Sunlight that are lit fewer than ``max_hours`` hours, darkened on a texture of its size with the hydrology's
    paint kernel: such a pixel is blended towards ``colour`` (three numbers in [0, 1]) with ``opacity``.  texture, value_range and
    the result: as hydrology.paint's; unpainted pixels keep their bits."""
    if not isinstance(light, Sunlight):
        raise ValueError("sunlight must be a Sunlight, got %r" % (light,))
    if not _number(max_hours) or max_hours < 0:
        raise ValueError("max_hours must be a number >= 0, got %r" % (max_hours,))
    colour, opacity = _check_colour(colour), _check_opacity(opacity)
    marks = (~light.mask_hours(max_hours)).astype(np.uint32)
    return _hy._paint(ops, texture, value_range, "sunlight", light.shape, None, marks, 1, 0, colour, opacity)


# ---- command line -------------------------------------------------------------------------------------------------------
def parse_sun(text):
    """AZ,EL[,HOURS] -> (azimuth, elevation[, hours])"""
    parts = [t.strip() for t in text.split(",")]
    try:
        if not 2 <= len(parts) <= 3:
            raise ValueError
        return tuple(float(t) for t in parts)
    except ValueError:
        raise argparse.ArgumentTypeError("a sun position is AZ,EL[,HOURS] (two or three numbers), got %r" % (text,))


def parse_args(argv):
    p = argparse.ArgumentParser(prog="python -m gan_heightmaps_amd.sunlight",
                                description="Hours of direct sun and insolation per cell of a heightmap, by exact shadow rays (on the GPU).")
    p.add_argument("input", help="heightmap: 8-bit PNG (read as greyscale), or .npy (uint8 or float in [0, 1], (H, W))")
    p.add_argument("output", help="the sunlight: .npz (lit, mask, hours_q, energy, table) or .png (the hours, scaled to 8 bits)")
    p.add_argument("--sun", dest="suns", type=parse_sun, action="append", metavar="AZ,EL[,HOURS]", default=None,
                   help="a sun position in degrees, azimuth 0 down the rows and 90 along them, and its hours (default 1); repeat for more")
    p.add_argument("--day", action="store_true", help="the positions of one day (--latitude, --declination, --step-minutes, --min-elevation)")
    d = Day()
    p.add_argument("--latitude", type=float, default=None, help="--day: degrees north (default %g)" % d.latitude)
    p.add_argument("--declination", type=float, default=None, help="--day: the sun's declination in degrees (default %g)" % d.declination)
    p.add_argument("--step-minutes", type=int, default=None, help="--day: minutes between positions (default %d)" % d.step_minutes)
    p.add_argument("--min-elevation", type=float, default=None, help="--day: the lowest elevation kept (default %g)" % d.min_elevation)
    p.add_argument("--target", type=float, default=0.0, help="cells above the ground at which a cell counts as lit (default 0)")
    p.add_argument("--height-scale", type=float, default=64.0, help="cells of height per unit of the heightmap")
    p.add_argument("--texture", default=None, metavar="F", help="a texture of the heightmap's size to darken the shaded ground on")
    p.add_argument("--painted", default=None, metavar="OUT", help="where the painted texture goes (PNG)")
    p.add_argument("--max-hours", type=float, default=None, help="--painted: cells lit fewer hours are darkened (default: half the sun's hours)")
    p.add_argument("--colour", type=_colour, default=(0.05, 0.05, 0.2), metavar="R,G,B", help="the paint's colour, in [0, 1]")
    p.add_argument("--opacity", type=float, default=0.5, help="how far painted pixels go towards the colour, in [0, 1]")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--plain", action="store_true", help="march every step of every shadow ray")
    g.add_argument("--accel", action="store_true", help="jump runs of steps that block maxima prove clear (the same bits)")
    # a position that starts with a negative number would read as an option: hand it over in the --sun=... form
    argv = list(argv)
    for i in range(len(argv) - 2, -1, -1):
        if argv[i] == "--sun" and argv[i + 1].lstrip()[:1] == "-" and argv[i + 1].lstrip()[1:2].isdigit():
            argv[i:i + 2] = ["--sun=" + argv[i + 1]]
    a = p.parse_args(argv)
    if bool(a.suns) == bool(a.day):
        p.error("one of --sun AZ,EL[,HOURS] (repeated) and --day is required")
    chosen = dict(latitude=a.latitude, declination=a.declination, step_minutes=a.step_minutes, min_elevation=a.min_elevation)
    if not a.day and any(v is not None for v in chosen.values()):
        p.error("--latitude / --declination / --step-minutes / --min-elevation need --day")
    if (a.texture is None) != (a.painted is None):
        p.error("--texture and --painted go together")
    if a.max_hours is not None and a.painted is None:
        p.error("--max-hours goes with --painted")
    if not (a.output.endswith(".npz") or a.output.lower().endswith(".png")):
        p.error("the output is .npz or .png")
    try:
        if a.day:
            a.sun_ = Day(**{k: v for k, v in chosen.items() if v is not None}).sun(a.target, a.height_scale)
        else:
            a.sun_ = Sun(tuple(a.suns), a.target, a.height_scale)
        _check_colour(a.colour)
        _check_opacity(a.opacity)
        if a.max_hours is None:
            a.max_hours = float(a.sun_.table()[:, 8].sum()) / 512.0
        elif a.max_hours < 0:
            raise ValueError("max_hours must be a number >= 0, got %r" % (a.max_hours,))
    except ValueError as e:
        p.error(str(e))
    a.form = 'accel' if a.accel else 'plain' if a.plain else None
    return a


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    from .device import Device, Ops
    x = read_image(a.input, "L", mmap=False)
    texture = None if a.texture is None else read_image(a.texture, mmap=False)
    dev = Device(0)
    try:
        ops = Ops(dev)
        light = sunlight(ops, x, a.sun_, form=a.form)
        painted = None if texture is None else paint(ops, texture, light, a.max_hours, a.colour, a.opacity)
    finally:
        dev.close()
    light.save(a.output)
    if painted is not None:
        _hy._save_painted(a.painted, painted)
    s = light.share()
    print("%d positions light %d of %d cells at some time, %.2f hours on average" % (
        len(light), int((light.lit > 0).sum()), light.lit.size, s["mean_hours"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
