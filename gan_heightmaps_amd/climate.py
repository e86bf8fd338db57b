"""Climate: wind-borne rain, temperature, biomes and discharge of a heightmap, computed on the device (csrc/climate.hip).
The other terrain tools read the terrain's shape alone; this says how wet and how warm every cell is, which biome that makes it, and
how much of the rain drains through it.  Integers throughout, and equal to a definition in plain Python (tests/climate_ref.py) bit
for bit.

Heights are quantised as the viewshed's, zq = int32(rint(h float32(height_scale 256))), and so is ``sea_level`` (sea_q); a cell is sea
when zq <= sea_q.

1. Transport.  The plane is cut into wind lines: rows for E and W, columns for N and S, the H + W - 1 diagonals for the others.  A line
   is walked from its upwind end with the vapour m = hum_q: over the sea m gains ((65536 - m) evap_q) >> 16; the share that falls is
   rate = min(base_q + ((lift up_q) >> 8), 65536) with lift the climb from the cell before (the sea counts as sea_q), so
   raw = (m rate) >> 16 leaves m; over land (raw rec_q) >> 16 of it returns.  A range drains the air on its windward side and leaves
   the lee dry: the rain shadow.
2. ``rain`` = the floor of the mean of raw over a (2 spread + 1)^2 window, clamped at the edges.
3. ``temperature`` = t0_q - ((max(zq - sea_q, 0) lapse_q) >> 16) - (((origin row + r) lat_q) >> 16), int32 in 1/256 degree.
4. ``biome``: on land table[#{e : temperature >= e}][#{e : rain >= e}] over a Biomes' edges, ``ocean`` in the sea; int32.
5. ``discharge`` (uint64), with a Hydrology that kept 'direction': the rain of a cell and of every cell that drains through it;
   ``effective_area`` = min(discharge // ref_q, 2^32 - 1), uint32: the drainage area in cells of reference rain, which a Hydrology
   takes in place of its accumulation (``Climate.hydrology``) so that rivers, paint, channels and fords follow the rain.

The transport has two forms with the same bits: ``line``, a lane per wind line on global memory, and ``staged``, 64 lines per block
with tiles of 64 steps moved through LDS row-wise.

    python -m gan_heightmaps_amd.climate IN OUT_PREFIX [--wind D] [--sea-level X] [--humidity X] [--evaporation X] [--drizzle X]
        [--uplift X] [--recycle X] [--spread N] [--sea-temperature X] [--lapse X] [--latitude X] [--reference-rain X]
        [--height-scale X] [--hydrology] [--texture F --painted OUT [--opacity X]] [--line | --staged]
"""
import argparse
import dataclasses
import sys

import numpy as np

from . import hydrology as _hy
from .planes import as_plane, check_keep, scratch
from .util import is_int as _is_int, is_number as _number, read_image
from .viewshed import _check_opacity, _check_origin

__all__ = ["WINDS", "KEEP", "PLANES", "FORMS", "DEFAULT_FORM", "MAX_SPREAD", "MAX_EDGES", "MAX_LABELS", "Weather", "Biomes", "Climate",
           "analyse", "paint", "parse_args", "main"]

WINDS = ('N', 'NE', 'E', 'SE', 'S', 'SW', 'W', 'NW')          # the side the wind comes from; the hydrology's neighbour order
KEEP = ('rain', 'temperature', 'biome', 'discharge', 'effective_area')
PLANES = ('raw',) + KEEP
FORMS = ('line', 'staged')
# tools/climate_bench.py, 4096 x 4096 value noise, every wind, one run on the MI355X, the forms alternated: the transport takes
# 1.23 (N, S), 1.31 (E, W) and 1.35 .. 1.37 ms (the diagonals) line against 0.56 and 0.73 ms staged, summed over the eight winds
# 10.54 against 5.16 ms; DESIGN §4zc has the line
DEFAULT_FORM = 'staged'
MAX_SPREAD, MAX_EDGES, MAX_LABELS = 8, 8, 64                 # GHM_CLIMATE_MAX_* (include/ghm.h)
MAX_ORIGIN_ROW = 1 << 31


def _unit(x):
    return _number(x) and 0 <= x <= 1


@dataclasses.dataclass(frozen=True)
class Weather:
    """The weather of ``analyse``, validated and frozen.  ``wind``: one of WINDS, the side the wind comes from; ``sea_level`` in
    [0, 1], in the heightmap's units; ``humidity`` in [0, 1], the vapour that enters at the upwind edge; ``evaporation`` in [0, 1],
    the share of the missing vapour a sea cell restores; ``drizzle`` in [0, 1], the share of the vapour that falls per cell on level
    ground; ``uplift`` in [0, 16], the extra share per cell of climb; ``recycle`` in [0, 1], the share of land rain that returns to
    vapour; ``spread``, an integer in [0, 8], the half-width of the window the rain is averaged over; ``sea_temperature`` in
    [-100, 100] degrees at sea level in world row 0; ``lapse`` in [0, 16], degrees lost per cell of height; ``latitude`` in [-1, 1],
    degrees lost per world row; ``reference_rain`` in (0, 1], the rain of a cell that counts as one cell of drainage area;
    ``height_scale`` in (0, 65536], cells per unit of height.  The defaults are chosen, not measured: a westerly over terrain a
    quarter under water, a coast at 24 degrees and a summit near freezing."""
    wind: str = 'W'
    sea_level: float = 0.25
    humidity: float = 0.6
    evaporation: float = 0.05
    drizzle: float = 0.02
    uplift: float = 0.05
    recycle: float = 0.3
    spread: int = 1
    sea_temperature: float = 24.0
    lapse: float = 0.6
    latitude: float = 0.0
    reference_rain: float = 0.01
    height_scale: float = 64.0

    def __post_init__(self):
        if not isinstance(self.wind, str) or self.wind not in WINDS:
            raise ValueError("wind must be one of %s, got %r" % (", ".join(WINDS), self.wind))
        for name in ("sea_level", "humidity", "evaporation", "drizzle", "recycle"):
            if not _unit(getattr(self, name)):
                raise ValueError("%s must be a number in [0, 1], got %r" % (name, getattr(self, name)))
        for name, lo, hi in (("uplift", 0, 16), ("lapse", 0, 16), ("sea_temperature", -100, 100), ("latitude", -1, 1)):
            v = getattr(self, name)
            if not _number(v) or not lo <= v <= hi:
                raise ValueError("%s must be a number in [%d, %d], got %r" % (name, lo, hi, v))
        if not _is_int(self.spread) or not 0 <= self.spread <= MAX_SPREAD:
            raise ValueError("spread must be an integer in [0, %d], got %r" % (MAX_SPREAD, self.spread))
        if not _number(self.reference_rain) or not 0 < self.reference_rain <= 1:
            raise ValueError("reference_rain must be a number in (0, 1], got %r" % (self.reference_rain,))
        if not _number(self.height_scale) or not 0 < self.height_scale <= 65536:
            raise ValueError("height_scale must be a number in (0, 65536], got %r" % (self.height_scale,))
        for f in dataclasses.fields(self):
            if f.name != "wind":
                object.__setattr__(self, f.name, (int if f.name == "spread" else float)(getattr(self, f.name)))

    def quantised(self):
        """the integers the kernels take: wind 0 .. 7, sea_q, hum_q, evap_q, base_q, up_q, rec_q, spread, t0_q, lapse_q, lat_q, ref_q"""
        def q(x, one):
            return int(np.rint(x * one))
        return dict(wind=WINDS.index(self.wind), sea_q=int(np.rint(np.float32(self.sea_level) * np.float32(self.height_scale * 256.0))),
                    hum_q=q(self.humidity, 65536), evap_q=q(self.evaporation, 65536), base_q=q(self.drizzle, 65536),
                    up_q=q(self.uplift, 65536), rec_q=q(self.recycle, 65536), spread=self.spread, t0_q=q(self.sea_temperature, 256),
                    lapse_q=q(self.lapse, 65536), lat_q=q(self.latitude, 1 << 24), ref_q=max(q(self.reference_rain, 65536), 1))


_NAMES = ('ocean', 'ice', 'tundra', 'taiga', 'grassland', 'desert', 'shrubland', 'temperate forest', 'savanna', 'rainforest',
          'temperate rainforest', 'seasonal forest')
_COLOURS = ((0.10, 0.25, 0.50), (0.95, 0.97, 1.00), (0.62, 0.66, 0.58), (0.25, 0.42, 0.35), (0.62, 0.72, 0.35), (0.85, 0.75, 0.50),
            (0.68, 0.62, 0.40), (0.25, 0.55, 0.25), (0.75, 0.70, 0.30), (0.05, 0.40, 0.15), (0.15, 0.48, 0.35), (0.40, 0.60, 0.25))
_TABLE = ((1, 1, 1, 1, 1),            # below -10 degrees
          (2, 2, 2, 2, 2),            # -10 .. 0
          (5, 4, 3, 3, 3),            # 0 .. 8
          (5, 4, 6, 7, 10),           # 8 .. 20
          (5, 8, 8, 11, 9))           # 20 and above


@dataclasses.dataclass(frozen=True)
class Biomes:
    """A biome chart, validated and frozen.  ``temperature_edges``: ascending degrees, at most 8, quantised x 256;
    ``rain_edges``: ascending rain in [0, 1] (the share of a full parcel of vapour that falls on the cell), at most 8, quantised
    x 65536; ``table``: (len(temperature_edges) + 1) rows of (len(rain_edges) + 1) labels, coldest row and driest column first;
    ``names``: the name of label k, at most 64; ``colours``: per label three numbers in [0, 1] or None for a biome ``paint`` leaves
    alone; ``ocean``: the label of every sea cell, which the table may not hold.  The default is a Whittaker-like chart of ice,
    tundra, taiga, grassland, desert, shrubland, temperate forest, savanna, rainforest, temperate rainforest and seasonal forest;
    it is chosen, not measured."""
    temperature_edges: tuple = (-10.0, 0.0, 8.0, 20.0)
    rain_edges: tuple = (0.004, 0.01, 0.02, 0.04)
    table: tuple = _TABLE
    names: tuple = _NAMES
    colours: tuple = _COLOURS
    ocean: int = 0

    def __post_init__(self):
        def edges(name, lo, hi, one):
            try:
                v = tuple(getattr(self, name))
            except TypeError:
                v = None
            if v is None or len(v) > MAX_EDGES or not all(_number(e) and lo <= e <= hi for e in v):
                raise ValueError("%s must be at most %d numbers in [%g, %g], got %r" % (name, MAX_EDGES, lo, hi, getattr(self, name)))
            q = [int(np.rint(float(e) * one)) for e in v]
            if any(a >= b for a, b in zip(q, q[1:])):
                raise ValueError("%s must ascend, got %r" % (name, v))
            object.__setattr__(self, name, tuple(float(e) for e in v))
            return len(v)
        nt, nr = edges("temperature_edges", -100, 100, 256), edges("rain_edges", 0, 1, 65536)
        try:
            names = tuple(self.names)
        except TypeError:
            names = ()
        if not 1 <= len(names) <= MAX_LABELS or not all(isinstance(n, str) and n for n in names) or len(set(names)) != len(names):
            raise ValueError("names must be 1 to %d different non-empty strings, got %r" % (MAX_LABELS, self.names))
        if not _is_int(self.ocean) or not 0 <= self.ocean < len(names):
            raise ValueError("ocean must be a label in [0, %d), got %r" % (len(names), self.ocean))
        try:
            table = tuple(tuple(row) for row in self.table)
        except TypeError:
            table = ()
        if len(table) != nt + 1 or any(len(row) != nr + 1 for row in table):
            raise ValueError("table must have %d rows of %d labels" % (nt + 1, nr + 1))
        for row in table:
            for v in row:
                if not _is_int(v) or not 0 <= v < len(names) or v == self.ocean:
                    raise ValueError("a table entry must be a label in [0, %d) other than ocean's, got %r" % (len(names), v))
        try:
            colours = tuple(self.colours)
        except TypeError:
            colours = ()
        if len(colours) != len(names):
            raise ValueError("colours must hold one entry per name, three numbers in [0, 1] or None")
        fixed = []
        for c in colours:
            if c is not None:
                try:
                    ok = len(c) == 3 and all(_unit(v) for v in c)
                except TypeError:
                    ok = False
                if not ok:
                    raise ValueError("a colour must be three numbers in [0, 1] or None, got %r" % (c,))
                c = tuple(float(v) for v in c)
            fixed.append(c)
        object.__setattr__(self, "names", names)
        object.__setattr__(self, "ocean", int(self.ocean))
        object.__setattr__(self, "table", tuple(tuple(int(v) for v in row) for row in table))
        object.__setattr__(self, "colours", tuple(fixed))

    def quantised(self):
        """(temperature edges x 256, rain edges x 65536, the table) as int32 arrays"""
        return (np.array([np.rint(e * 256) for e in self.temperature_edges], np.int32),
                np.array([np.rint(e * 65536) for e in self.rain_edges], np.int32), np.array(self.table, np.int32))

    def label(self, name):
        if name not in self.names:
            raise ValueError("no biome is called %r: the names are %s" % (name, ", ".join(self.names)))
        return self.names.index(name)


def _check_weather(weather):
    weather = Weather() if weather is None else weather
    if not isinstance(weather, Weather):
        raise ValueError("weather must be a Weather, got %r" % (weather,))
    return weather


def _check_biomes(biomes):
    biomes = Biomes() if biomes is None else biomes
    if not isinstance(biomes, Biomes):
        raise ValueError("biomes must be a Biomes, got %r" % (biomes,))
    return biomes


def _check_form(form):
    form = DEFAULT_FORM if form is None else form
    if not isinstance(form, str) or form not in FORMS:
        raise ValueError("form must be one of %r or None, got %r" % (FORMS, form))
    return form


class Climate:
    """What ``analyse`` returns: the planes it was asked to keep as numpy arrays (the others are None) -- ``raw`` and ``rain``
    uint32 in 1/65536 of a full parcel of vapour, ``temperature`` int32 in 1/256 degree, ``biome`` int32 labels of ``biomes``,
    and with a hydrology ``discharge`` uint64 and ``effective_area`` uint32 --, the ``shape``, the ``origin`` (the world
    coordinates of cell [0, 0]), the ``weather``, the ``biomes``, the transport's ``form`` and the discharge's doubling
    ``rounds``."""

    def __init__(self, shape, origin, weather, biomes, form=None, rounds=0, **planes):
        self.shape = (int(shape[0]), int(shape[1]))
        self.origin = (int(origin[0]), int(origin[1]))
        self.weather, self.biomes, self.form, self.rounds = weather, biomes, form, int(rounds)
        for k in PLANES:
            setattr(self, k, planes.get(k))

    def __repr__(self):
        return "Climate(%d x %d at %r, wind %s, planes=%s)" % (self.shape + (self.origin, self.weather.wind,
                                                                            [k for k in PLANES if getattr(self, k) is not None]))

    def _need(self, name):
        v = getattr(self, name)
        if v is None:
            raise ValueError("this needs the %s plane: keep=(%r, ...)%s" % (name, name, ", and a hydrology" if name in KEEP[3:] else ""))
        return v

    def celsius(self):
        """the temperature in degrees, float64"""
        return self._need('temperature').astype(np.float64) / 256.0

    def mask(self, *names):
        """True on the cells of the named biomes: ``scatter_heightmap(blocked=~mask)`` keeps a species to them, and a float of it
        is a ``penalty=`` for routes"""
        if not names:
            raise ValueError("mask needs one biome name at least")
        return np.isin(self._need('biome'), [self.biomes.label(n) for n in names])

    def share(self):
        """{name: the fraction of the land's cells that are this biome}, every name of the chart but the ocean's; 0.0 throughout
        on a plane without land"""
        b = self._need('biome')
        land = int((b != self.biomes.ocean).sum())
        return {n: (float((b == k).sum()) / land if land else 0.0) for k, n in enumerate(self.biomes.names) if k != self.biomes.ocean}

    def hydrology(self, hydro):
        """``hydro`` with the effective area as its accumulation, and everything else as it was: rivers, ``paint_water``,
        ``cut_rivers`` and routes' fords then see rivers that are thin on the dry side.  With rain equal to the reference rain
        everywhere it is ``hydro`` itself."""
        area = self._need('effective_area')
        if not isinstance(hydro, _hy.Hydrology) or tuple(hydro.shape) != self.shape:
            raise ValueError("hydro must be a Hydrology of the climate's size %s" % (self.shape,))
        planes = {k: getattr(hydro, k) for k in _hy.KEEP}
        planes['accumulation'] = area
        return _hy.Hydrology(hydro.shape, hydro.sweeps, hydro.rounds, hydro.tiled, **planes)

    def save(self, path):
        """a path that ends in .npz: one archive of the kept planes with origin, shape, wind and the chart's names; anything
        else is a prefix: PREFIX.rain.npy, PREFIX.temperature.npy, ... one file per kept plane"""
        kept = {k: getattr(self, k) for k in PLANES if getattr(self, k) is not None}
        if path.lower().endswith(".npz"):
            np.savez(path, origin=np.array(self.origin, np.int64), shape=np.array(self.shape, np.int64), wind=np.array(self.weather.wind),
                     names=np.array(self.biomes.names), ocean=np.array(self.biomes.ocean, np.int64), **kept)
        else:
            for k, v in kept.items():
                np.save("%s.%s.npy" % (path, k), v)


def analyse(ops, heightmap, weather=None, biomes=None, origin=(0, 0), hydro=None, form=None, keep=KEEP):
    """The climate of a heightmap: upload, the transport, the spread, temperature and biome in one launch, the discharge's doubling
    rounds if a hydrology is given, download, inside one scratch.  ops: a device.Ops; heightmap: as the viewshed takes it, (H, W) or
    (1, H, W), uint8 or floats in [0, 1]; weather: a Weather; biomes: a Biomes; origin: the world coordinates of cell [0, 0], whose
    row enters the temperature; hydro: a hydrology.Hydrology of the same plane that kept 'direction'; form: 'line' or 'staged', the
    transport's two forms, the same bits (default DEFAULT_FORM); keep: of PLANES -- 'discharge' and 'effective_area' are kept only
    with a hydrology.  Returns a Climate."""
    keep = check_keep(keep, PLANES)
    weather, biomes = _check_weather(weather), _check_biomes(biomes)
    origin = _check_origin(origin)
    if abs(origin[0]) > MAX_ORIGIN_ROW:
        raise ValueError("the origin's row must lie within 2^31 of row 0, got %d" % origin[0])
    form = _check_form(form)
    h = as_plane(heightmap, lead=True, unit_range=True, raw=True)
    H, W = h.shape
    if hydro is not None and (not isinstance(hydro, _hy.Hydrology) or hydro.direction is None or tuple(hydro.shape) != (H, W)):
        raise ValueError("hydro must be a Hydrology of the heightmap's size %s that kept 'direction'" % ((H, W),))
    q = weather.quantised()
    zq = np.rint(h * np.float32(weather.height_scale * 256.0)).astype(np.int32)
    t_edges, r_edges, table = biomes.quantised()
    n = H * W
    out, rounds = {}, 0
    dev = ops.dev
    with scratch(dev) as alloc:
        d_z, d_raw, d_rain, d_t, d_b = (alloc(4 * n) for _ in range(5))
        dev.h2d(d_z, zq)
        ops.climate_transport(d_z, W, H, W, q['wind'], FORMS.index(form), q['sea_q'], q['hum_q'], q['evap_q'], q['base_q'], q['up_q'],
                              q['rec_q'], d_raw, W)
        ops.climate_spread(d_raw, W, H, W, q['spread'], d_rain, W)
        ops.climate_biome(d_z, W, d_rain, W, H, W, q['sea_q'], q['t0_q'], q['lapse_q'], q['lat_q'], origin[0], t_edges, r_edges, table,
                          biomes.ocean, d_t, W, d_b, W)
        got = [('raw', d_raw, np.uint32), ('rain', d_rain, np.uint32), ('temperature', d_t, np.int32), ('biome', d_b, np.int32)]
        if hydro is not None:
            d_dir, d_q, d_e, d_w = alloc(n), alloc(8 * n), alloc(4 * n), alloc(ops.climate_workspace(H, W))
            dev.h2d(d_dir, np.ascontiguousarray(hydro.direction, np.int8))
            rounds = ops.climate_discharge(d_dir, W, d_rain, W, H, W, q['ref_q'], d_q, W, d_e, W, d_w)
            got += [('discharge', d_q, np.uint64), ('effective_area', d_e, np.uint32)]
        dev.sync()
        for name, ptr, dtype in got:
            if name in keep:
                out[name] = np.empty((H, W), dtype)
                dev.d2h(out[name], ptr, out[name].nbytes)
    return Climate((H, W), origin, weather, biomes, form=form, rounds=rounds, **out)


def paint(ops, texture, climate, opacity=0.6, value_range=None):
    """The biomes of a Climate painted on a texture of its plane's size: a pixel whose biome has a colour in the chart is blended
    towards it with ``opacity``, t + opacity (colour - t) per channel in float32, rounded as the hydrology's paint rounds; the
    pixels of a biome without a colour keep their bits.  texture, value_range and the result: as hydrology.paint's."""
    if not isinstance(climate, Climate) or climate.biome is None:
        raise ValueError("climate must be a Climate that kept 'biome'")
    opacity = _check_opacity(opacity)
    planes, unit, u8 = _hy._texture_planes(texture, value_range)
    C_, H, W = planes.shape
    if (H, W) != climate.shape:
        raise ValueError("texture %s and climate %s differ in size" % ((H, W), climate.shape))
    palette = np.zeros((len(climate.biomes.names), 4), np.float32)
    for k, c in enumerate(climate.biomes.colours):
        if c is not None:
            palette[k] = _hy.texture_colour(c, unit) + (1.0,)
    labels = np.ascontiguousarray(climate.biome, np.int32)
    res = np.empty((C_, H, W), np.uint8 if u8 else np.float32)
    dev = ops.dev
    with scratch(dev) as alloc:
        bufs = [alloc(x.nbytes) for x in (labels, planes, res)]
        dev.h2d(bufs[0], labels)
        dev.h2d(bufs[1], planes)
        ops.climate_paint(bufs[0], W, H, W, bufs[1], W, C_, palette, opacity, u8, bufs[2], W)
        dev.sync()
        dev.d2h(res, bufs[2], res.nbytes)
    a = np.asarray(texture)
    if u8:
        return np.ascontiguousarray(res[0] if a.ndim == 2 else res.transpose(1, 2, 0))
    return res[0] if a.ndim == 2 else res


# ---- command line -------------------------------------------------------------------------------------------------------
_FLAGS = (("sea_level", "--sea-level", float), ("humidity", "--humidity", float), ("evaporation", "--evaporation", float),
          ("drizzle", "--drizzle", float), ("uplift", "--uplift", float), ("recycle", "--recycle", float), ("spread", "--spread", int),
          ("sea_temperature", "--sea-temperature", float), ("lapse", "--lapse", float), ("latitude", "--latitude", float),
          ("reference_rain", "--reference-rain", float), ("height_scale", "--height-scale", float))


def add_weather_arguments(p, fields=None):
    """one flag per Weather field (``fields``: only these), default the Weather's"""
    d = Weather()
    p.add_argument("--wind", default=d.wind, metavar="D", help="the side the wind comes from: %s (default %s)" % (", ".join(WINDS), d.wind))
    for name, flag, kind in _FLAGS:
        if fields is None or name in fields:
            p.add_argument(flag, dest=name, type=kind, default=getattr(d, name), metavar="N" if kind is int else "X",
                           help="Weather.%s (default %r)" % (name, getattr(d, name)))


def parse_args(argv):
    p = argparse.ArgumentParser(prog="python -m gan_heightmaps_amd.climate",
                                description="Rain carried along the wind, temperature, biomes and discharge of a heightmap (on the GPU).")
    p.add_argument("input", help="heightmap: 8-bit PNG (read as greyscale), or .npy (uint8 or float in [0, 1], (H, W))")
    p.add_argument("out_prefix", help="writes OUT_PREFIX.rain.npy, .temperature.npy, .biome.npy and, with --hydrology, .discharge.npy and "
                                      ".effective_area.npy; a name that ends in .npz: one archive")
    add_weather_arguments(p)
    p.add_argument("--hydrology", action="store_true", help="analyse the drainage first and write the rain-weighted discharge")
    p.add_argument("--texture", default=None, metavar="F", help="a texture of the heightmap's size to paint the biomes on: PNG, or .npy")
    p.add_argument("--painted", default=None, metavar="OUT", help="the painted texture, as PNG (needs --texture)")
    p.add_argument("--opacity", type=float, default=None, metavar="X", help="how far painted pixels go towards their biome's colour (default 0.6)")
    f = p.add_mutually_exclusive_group()
    f.add_argument("--line", dest="form", action="store_const", const="line", default=None, help="a lane per wind line on global memory")
    f.add_argument("--staged", dest="form", action="store_const", const="staged", help="tiles of the lines through LDS (the same bits)")
    a = p.parse_args(argv)
    if (a.texture is None) != (a.painted is None):
        p.error("--texture and --painted go together")
    if a.opacity is not None and a.painted is None:
        p.error("--opacity goes with --painted")
    a.opacity = 0.6 if a.opacity is None else a.opacity
    try:
        a.weather = Weather(wind=a.wind, **{name: getattr(a, name) for name, _, _ in _FLAGS})
        _check_opacity(a.opacity)
    except ValueError as e:
        p.error(str(e))
    return a


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    from .device import Device, Ops
    x = read_image(a.input, "L", mmap=False)
    tex = read_image(a.texture, mmap=False) if a.texture else None
    dev = Device(0)
    try:
        ops = Ops(dev)
        hydro = _hy.analyse(ops, x, keep=('direction',)) if a.hydrology else None
        got = analyse(ops, x, a.weather, hydro=hydro, form=a.form)
        painted = paint(ops, tex, got, a.opacity) if tex is not None else None
    finally:
        dev.close()
    got.save(a.out_prefix)
    if painted is not None:
        _hy._save_painted(a.painted, painted)
    share = got.share()
    print("wind %s, %d x %d: %s" % (a.weather.wind, got.shape[0], got.shape[1],
                                   ", ".join("%s %.1f%%" % (n, 100 * s) for n, s in sorted(share.items(), key=lambda t: -t[1]) if s > 0) or "no land"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
