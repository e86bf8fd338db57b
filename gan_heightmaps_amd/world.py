"""Any region of an unbounded seeded world, chunk by chunk.

``generate_terrain`` (§4k) grows one finite canvas; a ``TerrainWorld`` is that canvas without borders.  A pixel of it is a
pure function of (weights, seed, coordinates): ask for any rectangle, at any time, in any order, and rectangles that
overlap agree bit for bit.

    latent(i, j)   the latent vector of cell (i, j), any integers: the model's sampler after numpy's global RNG is seeded
                   with the array [seed, i, j] (mod 2^32); the global stream is saved and restored around the draw.
    S[c, y, x]     the seed canvas over all of Z^2: §4k's blends with no clamping (``mosaic``: cell (y // s, x // s);
                   ``bilinear``: cells floor(u), floor(u) + 1 per axis, u = (y + 0.5)/s - 0.5, weights from y mod s alone).
    Hm = trunk(S)  no border anywhere.

The world is cut into square chunks of K = chunk_cells * in_shp output pixels; chunk (a, b) is the pixels
[aK, (a+1)K) x [bK, (b+1)K) and comes from exactly ONE trunk pass over the seed window
[a c s - halo, (a+1) c s + halo)^2, whose centre K x K is kept.  The window's shape and place do not depend on the request,
so neither do the values; a request is assembled from the chunks it touches.  Chunks stay in HBM in an LRU cache that is
dropped whenever the engine's parameters may have changed.

Textures: U-Net tiles of T = in_shp pixels are anchored to the world too, tile (p, q) covering
[p st, p st + T) x [q st, q st + T), st = T - overlap; with an overlap every tile ramps on all four sides (§4j's ramps),
Tex = sum(w U(tile)) / sum(w) in row-major tile order.  Tile q of a tile row always runs in slot q mod batch_size of its
forward pass.  The tiles are gathered on the device from the resident chunks: the heightmap never visits the host.

Rendering: ``scene`` hands a rectangle to the ray caster -- through the host, or with resident=True
assembled on the device by sinks that write a render.Scene's planes --, and ``flight`` renders a camera path of any length
from one bounded scene window after the other (``flight_plan``: the window rule).

Erosion: with ``erosion=`` the world IS the eroded one.  What ``_compute`` makes becomes a raw layer; chunk
(a, b) of ``_chunks`` is erosion.erode's simulation over the raw rectangle [aK - E, (a+1)K + E)^2, E = erosion.halo, gathered
on the device from the at most nine raw chunks it touches, with the centre K x K emitted into the chunk buffer.  The window does
not depend on the request and a cell E from every wall does not feel it, so requests still agree bit for bit; everything
downstream of ``_acquire`` -- crops, textures, scenes, flights -- reads the eroded chunks through the code it has.

    python -m gan_heightmaps_amd.world EXPERIMENT MODEL OUT --seed N --region Y0,X0,H,W [--chunk-cells C]
        [--blend mosaic|bilinear] [--dtype D] [--texture OUT_TEX [--overlap N] [--batch-size B]] [--erode N]
        [--routes OUT_PREFIX --from Y,X [--from Y,X ...] [--to Y,X ...]] [--earthworks OUT] [--scatter OUT --spacing X]
        [--viewshed OUT --from Y,X [--from Y,X ...]]
        [--contours OUT.{svg,geojson,npz} [--interval X] [--base X] [--count N] [--index-every N]]
        [--peaks OUT.{geojson,csv,npz} [--min-prominence X] [--top N]]
        [--rivers OUT.{svg,geojson,npz} [--river-threshold N] [--min-order N]]
        [--regions OUT.{svg,geojson,npz} --of {lakes,basins,land,bands} [--sea-level X] [--min-cells N] [--no-holes]]
        [--climate OUT_PREFIX [--wind D] [--sea-level X]]
        [--sunlight OUT.{npz,png} [--latitude X] [--declination X]]
"""
import argparse
import collections
import contextlib
import os
import re
import sys
from collections import OrderedDict

import numpy as np

from . import erosion as _erosion
from . import skylight as _skylight
from . import layers as L
from .chunk_cache import ChunkCache
from .streaming import DownloadRing, check_uint8_channels, output_array, shift_accumulator, store_rows
from .terrain import BLENDS, INT32_LIMIT, TerrainGeometry
from . import terrain as _terrain
from .texture import check_overlap
from .planes import scratch
from .util import is_int as _is_int, is_number as _is_number

__all__ = ["HEAD_BLOCK", "MAX_BATCH", "SCENE_BYTES_PER_PIXEL", "SKY_SCENE_BYTES_PER_PIXEL", "world_latent", "axis_chunks", "axis_tiles", "seed_cells",
           "window_elements", "default_chunk_cells", "slot_batches", "erosion_sources", "snap_out", "plan_windows", "TerrainWorld",
           "WorldEarthworks",
           "parse_region",
           "parse_args", "main"]

# what TerrainWorld.earthworks returns: the carved ground, the hydrology and the travel field it came from, the graded paths
WorldEarthworks = collections.namedtuple("WorldEarthworks", "height hydro cost_field paths")

HEAD_BLOCK = 8                   # the head runs over world-aligned blocks of HEAD_BLOCK x HEAD_BLOCK cells, one pass each
MAX_BATCH = 32                   # GHM_WORLD_MAX_TILES (include/ghm.h): tiles per forward pass


def world_latent(seed, i, j, sampler, latent_dim):
    """the latent vector of cell (i, j) of world ``seed``: ``sampler(1, latent_dim)[0]`` as float32 after seeding numpy's
    global RNG with [seed, i, j] (each mod 2^32); the global stream is left exactly as it was"""
    state = np.random.get_state()
    try:
        np.random.seed(np.array([seed % (1 << 32), i % (1 << 32), j % (1 << 32)], np.uint32))
        return np.asarray(sampler(1, latent_dim), np.float32)[0]
    finally:
        np.random.set_state(state)


def axis_chunks(y0, n, K):
    """(first, last) chunk index of an axis touched by pixels [y0, y0 + n): exact and minimal, floor division"""
    return y0 // K, (y0 + n - 1) // K


def axis_tiles(y0, n, T, o):
    """(first, last) index of the world-anchored tiles (tile p = [p st, p st + T), st = T - o) that cover a pixel of
    [y0, y0 + n)"""
    st = T - o
    return (y0 - T) // st + 1, (y0 + n - 1) // st


def seed_cells(y0, n, s, bilinear):
    """(first, last) cell index of an axis read by seed pixels [y0, y0 + n) of the unbounded canvas"""
    if not bilinear:
        return y0 // s, (y0 + n - 1) // s

    def lo(y):
        return y // s + int(np.floor((y % s + 0.5) / s - 0.5))
    return lo(y0), lo(y0 + n - 1) + 1


def window_elements(geo, chunk_cells):
    """elements of the largest trunk activation (the input included) of one chunk window"""
    win = chunk_cells * geo.s + 2 * geo.halo
    return (geo.per_row // geo.Ws) * win * win


def default_chunk_cells(geo):
    """the largest power of two whose window keeps the largest trunk activation within terrain.WINDOW_BUDGET bytes (fp32) and
    under 2^31 elements; ``geo`` is any TerrainGeometry of the generator"""
    c = 1
    while window_elements(geo, 2 * c) * 4 <= _terrain.WINDOW_BUDGET and window_elements(geo, 2 * c) < INT32_LIMIT:
        c *= 2
    return c


def slot_batches(q_lo, q_hi, B):
    """the forward passes of one tile row covering tiles q_lo .. q_hi: [(tiles of the B slots, first real slot, real tiles)].
    Tile q always sits in slot q mod B of pass q // B; slots whose tile lies outside the range repeat the nearest one."""
    out = []
    for k in range(q_lo // B, q_hi // B + 1):
        lo, hi = max(B * k, q_lo), min(B * k + B - 1, q_hi)
        out.append(([min(max(B * k + j, q_lo), q_hi) for j in range(B)], lo - B * k, hi - lo + 1))
    return out


def erosion_sources(a, b, K, E):
    """what the eroded chunk (a, b) is made from: the raw chunks that the window [aK - E, (a+1)K + E)^2 touches, row-major,
    as [((ra, rb), r0, c0, nr, nc, wy, wx)] -- rows [r0, r0 + nr) x columns [c0, c0 + nc) of raw chunk (ra, rb) go to rows
    wy .., columns wx .. of the window.  With 0 < E <= K these are the nine chunks around (a, b), negative indices included."""
    y0, x0, n = a * K - E, b * K - E, K + 2 * E
    (a_lo, a_hi), (b_lo, b_hi) = axis_chunks(y0, n, K), axis_chunks(x0, n, K)
    out = []
    for ra in range(a_lo, a_hi + 1):
        ya, yb = max(y0, ra * K), min(y0 + n, (ra + 1) * K)
        for rb in range(b_lo, b_hi + 1):
            xa, xb = max(x0, rb * K), min(x0 + n, (rb + 1) * K)
            out.append(((ra, rb), ya - ra * K, xa - rb * K, yb - ya, xb - xa, ya - y0, xa - x0))
    return out


# bytes of device memory a render scene keeps per pixel: the height plane (4), the three texture planes (12) and
# the maximum pyramid (4/3 of the map, 16/3 bytes), rounded up
SCENE_BYTES_PER_PIXEL = 22
# a scene lit from the sky keeps its baked plane too (4)
SKY_SCENE_BYTES_PER_PIXEL = SCENE_BYTES_PER_PIXEL + 4


def _check_sky(sky):
    if sky is not None and not isinstance(sky, _skylight.SkyLight):
        raise ValueError("sky must be a skylight.SkyLight, got %r" % (sky,))
    return sky


def snap_out(rect, snap):
    """the rectangle (y0, x0, h, w) expanded outward to multiples of ``snap`` (floor and ceiling, so negative coordinates move
    away from zero as positive ones do)"""
    y0, x0, h, w = rect
    ya, xa = y0 // snap * snap, x0 // snap * snap
    yb, xb = -(-(y0 + h) // snap) * snap, -(-(x0 + w) // snap) * snap
    return ya, xa, yb - ya, xb - xa


def plan_windows(footprints, snap, max_pixels):
    """the scene windows of a camera path: [(rect, first_frame, last_frame)].  Starting at frame i a window takes the longest
    run of consecutive frames i .. j whose footprints' union, expanded outward to multiples of ``snap``, has at most
    ``max_pixels`` pixels; the next window starts at j + 1.  A frame whose own snapped footprint is larger is a ValueError."""
    if not _is_int(snap) or snap < 1:
        raise ValueError("snap must be a positive integer, got %r" % (snap,))
    out, i, n = [], 0, len(footprints)
    while i < n:
        rect = snap_out(footprints[i], snap)
        if rect[2] * rect[3] > max_pixels:
            raise ValueError("frame %d alone needs a window of %d x %d = %d pixels, the cap is %d: raise window_mb"
                             % (i, rect[2], rect[3], rect[2] * rect[3], max_pixels))
        j = i
        while j + 1 < n:
            f = footprints[j + 1]
            y0, x0 = min(rect[0], f[0]), min(rect[1], f[1])
            y1, x1 = max(rect[0] + rect[2], f[0] + f[2]), max(rect[1] + rect[3], f[1] + f[3])
            grown = snap_out((y0, x0, y1 - y0, x1 - x0), snap)
            if grown[2] * grown[3] > max_pixels:
                break
            rect, j = grown, j + 1
        out.append((rect, i, j))
        i = j + 1
    return out


class _HostSinks:
    """Where a request's finished rows go, and which it wants (``want_hm``, ``want_tex``), the host form: one download ring
    per output (streaming.DownloadRing) into the caller's arrays -- ``out_hm`` and ``out_tex``, made here where the caller
    gave none --, both on one copy stream of their own so that finished rows go down while the next chunks run."""

    def __init__(self, *, hm=False, tex=False, out_hm=None, out_tex=None, hm_u8=False, tex_u8=False):
        self.want_hm, self.want_tex = hm, tex
        self.out_hm, self.out_tex, self.hm_u8, self.tex_u8 = out_hm, out_tex, hm_u8, tex_u8
        self.cp = self.hm = self.tex = None

    outs = property(lambda self: (self.out_hm, self.out_tex))

    def plan_hm(self):
        C, (h, w) = self.world._geo.channels, self.rect[2:]
        if self.hm_u8:
            check_uint8_channels(C)
        shape = ((h, w) if C == 1 else (h, w, 3)) if self.hm_u8 else (C, h, w)
        self.out_hm = output_array(self.out_hm, shape, np.uint8 if self.hm_u8 else np.float32)

    def plan_tex(self, c_out):
        h, w = self.rect[2:]
        if self.tex_u8:
            check_uint8_channels(c_out)
        self.out_tex = output_array(self.out_tex, (h, w, 3) if self.tex_u8 else (c_out, h, w),
                                    np.uint8 if self.tex_u8 else np.float32)

    def open(self):
        self.cp = type(self.world._dev)(self.world._dev.index)

    def begin_hm(self):
        wd, (y0, x0, h, w), out = self.world, self.rect, self.out_hm
        C = wd._geo.channels
        self.hbpp = (1 if C == 1 else 3) if self.hm_u8 else 4 * C
        self.hm = DownloadRing(wd._dev, self.cp, min(wd._K, h) * w * self.hbpp,
                               lambda buf, ya, yb: store_rows(out, buf, ya, yb, w))

    def begin_tex(self, c_out, Wp):
        wd, w, out = self.world, self.rect[3], self.out_tex
        self.c_out, self.Wp = c_out, Wp
        self.tbpp = 3 if self.tex_u8 else 4 * c_out
        self.tex = DownloadRing(wd._udev, self.cp, wd._geo.out * Wp * self.tbpp,
                                lambda buf, ya, yb: store_rows(out, buf, ya, yb, Wp, w))

    def hm_row(self, a, b_lo, b_hi):
        """the request's rows inside chunk row a (its chunks are resident) -> a stage -> the host"""
        wd, (y0, x0, h, w) = self.world, self.rect
        K, C = wd._K, wd._geo.channels
        ra, rb = max(y0, a * K), min(y0 + h, (a + 1) * K)
        stage = self.hm.stage()
        for b in range(b_lo, b_hi + 1):
            ca, cb = max(x0, b * K), min(x0 + w, (b + 1) * K)
            wd._ops.world_crop(wd._chunks[(a, b)], C, K, ra - a * K, ca - b * K, rb - ra, cb - ca, self.hm_u8,
                               wd.model.is_a_grayscale, stage, w, ca - x0)
        self.hm.send((rb - ra) * w * self.hbpp, ra - y0, rb - y0)
        self.hdone.append(a)
        self.hm.poll()

    def tex_rows(self, acc, r_lo, n, yr, ny, pad_y, nx, pad_x):
        """rows [r_lo, r_lo + n) of the accumulator, the request's rows yr + r_lo ..., finalized -> a stage -> the host"""
        wd = self.world
        wd._uops.texture_finalize(acc, self.Wp, wd._geo.out, self.c_out, r_lo, n, yr, ny, pad_y, nx, pad_x, wd.overlap,
                                  self.tex_u8, wd.model.is_b_grayscale, self.tex.stage())
        self.tex.send(n * self.Wp * self.tbpp, yr + r_lo, yr + r_lo + n)

    def tex_poll(self):
        self.tex.poll()

    def finish(self):
        for ring in (self.tex, self.hm):
            if ring is not None:
                ring.finish()

    def close(self):
        self.cp.sync()
        for ring in (self.hm, self.tex):
            if ring is not None:
                ring.close()
        self.cp.close()


class _SceneSinks:
    """Where a request's finished rows go, the resident form: straight into the planes of a render scene on the
    device -- hm fp32 [h, w] at hm_ptr, tex fp32 [3, h, w] at tex_ptr (None: not wanted), mapped to [0, 1] by the sinks'
    kernels as render.Scene maps them on the host.  No array to make, no stage, no pinned buffer, no copy stream; a
    non-finite value sets the int32 at flag_ptr."""

    def __init__(self, *, hm_ptr, tex_ptr, flag_ptr):
        self.want_hm, self.want_tex = hm_ptr is not None, tex_ptr is not None
        self.hm_ptr, self.tex_ptr, self.flag_ptr = hm_ptr, tex_ptr, flag_ptr

    plan_hm = plan_tex = open = tex_poll = finish = close = lambda self, *args: None

    def begin_hm(self):
        if self.world._geo.channels not in (1, 3):
            raise ValueError("a scene needs a 1- or 3-channel heightmap generator, this one has %d"
                             % self.world._geo.channels)

    def begin_tex(self, c_out, Wp):
        if c_out not in (1, 3):
            raise ValueError("a scene needs a 1- or 3-channel texture generator, this one has %d" % c_out)
        self.c_out, self.Wp = c_out, Wp

    def hm_row(self, a, b_lo, b_hi):
        wd, (y0, x0, h, w) = self.world, self.rect
        K = wd._K
        ra, rb = max(y0, a * K), min(y0 + h, (a + 1) * K)
        for b in range(b_lo, b_hi + 1):
            ca, cb = max(x0, b * K), min(x0 + w, (b + 1) * K)
            wd._ops.world_scene_height(wd._chunks[(a, b)], wd._geo.channels, K, ra - a * K, ca - b * K, rb - ra, cb - ca,
                                       wd.model.is_a_grayscale, self.hm_ptr, h, w, ra - y0, ca - x0, self.flag_ptr)
        self.hdone.append(a)

    def tex_rows(self, acc, r_lo, n, yr, ny, pad_y, nx, pad_x):
        wd, (y0, x0, h, w) = self.world, self.rect
        wd._uops.texture_finalize_scene(acc, self.Wp, wd._geo.out, self.c_out, r_lo, n, yr, ny, pad_y, nx, pad_x, wd.overlap,
                                        wd.model.is_b_grayscale, self.tex_ptr, h, w, self.flag_ptr)


@contextlib.contextmanager
def _flagged_planes(dev, sizes, sync):
    """device planes of ``sizes`` bytes for requests through _SceneSinks and, last, their int32 flag, zeroed, in a
    planes.scratch(dev, sync): -> [the allocator, the planes ..., the flag]"""
    with scratch(dev, sync) as alloc:
        bufs = [alloc(n) for n in sizes + (4,)]
        dev.memset_zero(bufs[-1], 4)
        dev.sync()
        yield [alloc] + bufs


class TerrainWorld:
    """An unbounded terrain addressed by pixel coordinates.  See Pix2Pix.terrain_world and the module docstring."""

    def __init__(self, model, seed, chunk_cells=None, blend='bilinear', overlap=None, batch_size=4, cache_mb=1024,
                 latent_fn=None, deterministic=True, verbose=False, erosion=None):
        if not deterministic:
            raise NotImplementedError("terrain_world needs deterministic=True: with batch statistics a pixel would depend "
                                      "on what shares its pass, not on (weights, seed, coordinates) alone")
        if not _is_int(seed):
            raise ValueError("seed must be an integer, got %r" % (seed,))
        if blend not in BLENDS:
            raise ValueError("blend must be one of %s, got %r" % (BLENDS, blend))
        if not _is_int(batch_size) or not 1 <= batch_size <= MAX_BATCH:
            raise ValueError("batch_size must be an integer in [1, %d], got %r" % (MAX_BATCH, batch_size))
        if not _is_number(cache_mb, finite=False) or cache_mb < 0:
            raise ValueError("cache_mb must be a number >= 0, got %r" % (cache_mb,))
        if latent_fn is not None and not callable(latent_fn):
            raise ValueError("latent_fn must be callable as latent_fn(i, j)")
        self.model, self.seed, self.blend = model, int(seed), blend
        self.batch_size, self.latent_fn = int(batch_size), latent_fn
        geo = TerrainGeometry(model.dcgan['gen'], 1, 1)          # refuses what split_generator refuses
        if 2 * geo.halo < geo.s:
            raise NotImplementedError("terrain_world: the trunk's halo (%d) is below half a cell (%d)" % (geo.halo, geo.s))
        if chunk_cells is None:
            chunk_cells = default_chunk_cells(geo)
        elif not _is_int(chunk_cells) or chunk_cells < 1:
            raise ValueError("chunk_cells must be a positive integer, got %r" % (chunk_cells,))
        if window_elements(geo, chunk_cells) >= INT32_LIMIT:
            raise ValueError("terrain_world: chunk_cells=%d makes a window tensor of %d elements; the kernels index up to 2^31"
                             % (chunk_cells, window_elements(geo, chunk_cells)))
        self._geo, self._c = geo, int(chunk_cells)
        self._K = self._c * geo.out
        self._win = self._c * geo.s + 2 * geo.halo
        self.overlap = check_overlap(geo.out, overlap)
        self._cache = ChunkCache(lambda n: self._dev.alloc(n), lambda p: self._dev.free(p),
                                 geo.channels * self._K * self._K * 4, cache_mb)
        self._heads = OrderedDict()                               # (I, J) -> DevTensor [HEAD_BLOCK^2, nch s s]
        self._table, self._version, self._closed = None, None, False
        self.computed = 0                                         # raw chunks computed so far (a cache hit computes nothing)
        # ---- the eroded layer: _chunks holds eroded chunks, _raw what _compute makes; one LRU over both ----
        if erosion is not None:
            if not isinstance(erosion, _erosion.Erosion):
                raise ValueError("erosion must be an erosion.Erosion, got %r" % (erosion,))
            if geo.channels != 1:
                raise ValueError("erosion needs one height per pixel, this generator has %d channels" % geo.channels)
            if erosion.halo > self._K:
                raise ValueError("erosion: %d iterations reach %d pixels, more than a chunk of %d: a window would read "
                                 "beyond the nine chunks around its own; raise chunk_cells or lower iterations"
                                 % (erosion.iterations, erosion.halo, self._K))
            n = self._K + 2 * erosion.halo
            if n * n >= INT32_LIMIT or n > 4 * 65535:
                raise ValueError("erosion: a window of %d x %d cells is beyond the kernels' range" % (n, n))
        self.erosion = erosion
        self.eroded = 0                                           # erosions run so far
        self._ero, self._fused = None, _erosion.DEFAULT_FUSED     # one window's states, allocated once; the kernels' form
        if verbose:
            print("terrain_world: seed %d, chunk_cells %d (%d px), blend %s, overlap %d%s"
                  % (self.seed, self._c, self._K, blend, self.overlap,
                     "" if erosion is None else ", eroded %d iterations" % erosion.iterations))

    chunk_cells = property(lambda self: self._c)
    chunk_px = property(lambda self: self._K)
    geometry = property(lambda self: self._geo)
    cache_mb = property(lambda self: self._cache.cache_mb)
    _chunks = property(lambda self: self._cache.layers['e'])
    _raw = property(lambda self: self._cache.layers['r'])

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def latent(self, i, j):
        """the latent vector [latent_dim] of cell (i, j), any integers"""
        if not _is_int(i) or not _is_int(j):
            raise ValueError("cell indices must be integers, got %r, %r" % (i, j))
        if self.latent_fn is not None:
            z = np.asarray(self.latent_fn(int(i), int(j)), np.float32)
            if z.shape != (self.model.latent_dim,):
                raise ValueError("latent_fn must return [%d], got %s" % (self.model.latent_dim, z.shape))
            return z
        return world_latent(self.seed, int(i), int(j), self.model.sampler, self.model.latent_dim)

    # ---- the device side ------------------------------------------------------------------------------------------------
    def _bind(self):
        from .step import LANE_OF
        if self._closed:
            raise ValueError("this TerrainWorld is closed")
        eng = self.model.engine
        self._eng = eng
        lg, lu = LANE_OF['dcgan_gen'], LANE_OF['p2p_gen']
        self._dev, self._ops = eng.devs[lg], eng.ops[lg]
        self._udev, self._uops = eng.devs[lu], eng.ops[lu]
        geo = self._geo
        self._hplan, self._hprog = eng._subgraph_plan('dcgan_gen', ('head',), HEAD_BLOCK * HEAD_BLOCK, lambda: geo.head)

        def trunk_graph():
            inp = L.InputLayer((None, geo.nch, self._win, self._win))
            return L.clone_chain(geo.trunk[-1], geo.reshape, inp)
        self._tplan, self._tprog = eng._subgraph_plan('dcgan_gen', ('world', self._win), 1, trunk_graph)
        u = self._tplan.out
        assert u.shape == (1, geo.channels, self._win * geo.F, self._win * geo.F), u.shape
        if eng.param_version != self._version:                   # never serve a chunk of other parameters
            self._drop()
            self._version = eng.param_version

    def _drop(self):
        self._cache.drop()
        for t in self._heads.values():
            self._dev.free(t.ptr)
        self._heads.clear()

    def _head_block(self, I, J):
        if (I, J) in self._heads:
            self._heads.move_to_end((I, J))
            return self._heads[(I, J)]
        n, d = HEAD_BLOCK, self.model.latent_dim
        z = np.empty((n * n, d), np.float32)
        for k in range(n * n):
            z[k] = self.latent(I * n + k // n, J * n + k % n)
        self._hplan.input_nodes[0].out.set(z)
        for e in self._hprog:
            e[1]()
        P = self._dev.empty((n * n, self._geo.nch * self._geo.s * self._geo.s, 1, 1))
        self._ops.copy_view(self._hplan.out, P)
        self._heads[(I, J)] = P
        return P

    def _trim_heads(self, keep):
        while len(self._heads) > keep:
            _, t = self._heads.popitem(last=False)
            self._dev.sync()
            self._dev.free(t.ptr)

    def _compute(self, a, b):
        geo, c, n = self._geo, self._c, HEAD_BLOCK
        bil = self.blend == 'bilinear'
        wy0, wx0 = a * c * geo.s - geo.halo, b * c * geo.s - geo.halo
        i_lo, i_hi = seed_cells(wy0, self._win, geo.s, bil)
        j_lo, j_hi = seed_cells(wx0, self._win, geo.s, bil)
        ncy, ncx = i_hi - i_lo + 1, j_hi - j_lo + 1
        if self._table is None:                                   # every window reads a cell block of this one shape
            self._table = self._dev.empty((ncy * ncx, geo.nch * geo.s * geo.s, 1, 1))
        table = self._table
        assert table.N == ncy * ncx
        for i in range(i_lo, i_hi + 1):
            j = j_lo
            while j <= j_hi:
                J = j // n
                j1 = min(j_hi, J * n + n - 1)                     # the run of this cell row inside head block (i // n, J)
                P = self._head_block(i // n, J)
                k0 = (i % n) * n + j % n
                t0 = (i - i_lo) * ncx + (j - j_lo)
                self._ops.copy_view(P.samples(k0, k0 + j1 - j + 1), table.samples(t0, t0 + j1 - j + 1))
                j = j1 + 1
        self._ops.world_seed(table, i_lo, j_lo, ncy, ncx, geo.s, wy0, wx0, bil, self._tplan.input_nodes[0].out)
        for e in self._tprog:
            e[1]()
        ptr = self._cache.buffer()
        self._ops.world_emit(self._tplan.out, geo.halo * geo.F, geo.halo * geo.F, self._K, ptr)
        self.computed += 1
        return ptr

    def _erode(self, srcs):
        """the window of one chunk: gathered from its resident raw chunks, eroded, its centre K x K -> a chunk buffer"""
        ero, K, dev, ops = self.erosion, self._K, self._dev, self._ops
        E = ero.halo
        n = K + 2 * E
        plane = 4 * n * n
        if self._ero is None:
            from .device import erosion_params
            self._ero = dev.alloc(_erosion.workspace_planes(self._fused) * plane)
            self._ero_params = erosion_params(**ero.as_dict())
        s0, s1 = self._ero, self._ero + _erosion.PLANES * plane
        tmp = None if self._fused else s1 + _erosion.PLANES * plane
        # the raw window lands in the second state's first plane, which nothing reads before the first step writes it
        for key, r0, c0, nr, nc, wy, wx in srcs:
            ops.world_crop(self._raw[key], 1, K, r0, c0, nr, nc, False, True, s1 + 4 * wy * n, n, wx)
        ops.erosion_init(s1, n, n, n, ero.height_scale, s0, n)
        fin = ops.erosion_iterate(self._ero_params, s0, s1, tmp, n, n, n, ero.iterations, self._fused)
        ptr = self._cache.buffer()
        ops.erosion_emit(fin, n, n, n, ero.height_scale, E, E, K, K, False, ptr, K, K)
        self.eroded += 1
        return ptr

    def _acquire(self, keys):
        """make the chunks ``keys`` resident (they stay so until the next _acquire), then evict down to the budget.  A missing
        chunk's sources (erosion_sources; none in a plain world) come first; they, these keys and the last call's are kept"""
        cache, chunks = self._cache, self._chunks
        missing = any(k not in chunks for k in keys)
        if missing and self._udev is not self._dev:
            self._dev.wait_for(self._udev)                        # a recycled buffer may still feed an earlier gather
        keep = {('e', k) for k in set(keys) | cache.pinned}
        for k in keys:
            srcs = [] if self.erosion is None or k in chunks else erosion_sources(k[0], k[1], self._K, self.erosion.halo)
            need = keep | {('r', s[0]) for s in srcs}
            for s in srcs:
                cache.get('r', s[0], need, lambda: self._compute(*s[0]))
            cache.get('e', k, need, lambda: self._erode(srcs) if srcs else self._compute(*k))
        cache.pinned = set(keys)
        cache.evict({('e', k) for k in keys})
        self._trim_heads(4 * HEAD_BLOCK if cache.capacity() else 0)
        if missing and self._udev is not self._dev:
            self._udev.wait_for(self._dev)

    def _release(self):
        """end of a request: nothing is pinned, the cache goes down to its budget, recycled buffers are freed"""
        self._cache.pinned = set()
        self._cache.evict(set())
        self._eng.sync()
        self._cache.free_pool()

    def clear(self):
        """drop every cached chunk and head map (the next request computes what it needs)"""
        if getattr(self, '_eng', None) is not None:
            self._drop()
            self._release()

    def close(self):
        if self._closed:
            return
        self._closed = True
        if getattr(self, '_eng', None) is None:
            return
        self._eng.sync()
        self._drop()
        self._cache.free_pool()
        if self._table is not None:
            self._dev.free(self._table.ptr)
            self._table = None
        if self._ero is not None:
            self._dev.free(self._ero)
            self._ero = None

    # ---- requests -------------------------------------------------------------------------------------------------------
    def _check_region(self, y0, x0, h, w):
        for name, v in (("y0", y0), ("x0", x0), ("h", h), ("w", w)):
            if not _is_int(v):
                raise ValueError("%s must be an integer, got %r" % (name, v))
        if h < 1 or w < 1:
            raise ValueError("the region must be at least 1 x 1, got %d x %d" % (h, w))
        if w >= 1 << 24:
            raise ValueError("the region is %d pixels wide; at most %d" % (w, (1 << 24) - 1))
        # the seed coordinates the kernels see are int32
        if max(abs(y0), abs(x0), abs(y0 + h), abs(x0 + w)) // self._geo.F + 2 * self._win >= 1 << 29:
            raise ValueError("the region (%d, %d, %d, %d) lies outside the kernels' int32 seed coordinates" % (y0, x0, h, w))
        return int(y0), int(x0), int(h), int(w)

    def heightmap(self, y0, x0, h, w, out=None, uint8=False):
        """pixels [y0, y0 + h) x [x0, x0 + w) of the heightmap: (C_a, h, w) float32, or with uint8=True
        util.to_uint8(util.convert_to_rgb(.)) as (h, w) for a greyscale generator, (h, w, 3) otherwise"""
        return self._request((y0, x0, h, w), _HostSinks(hm=True, out_hm=out, hm_u8=uint8)).out_hm

    def texture(self, y0, x0, h, w, out=None, uint8=False):
        """the same pixels of the textured world: (C_out, h, w) float32, or with uint8=True the (h, w, 3) uint8 RGB"""
        return self._request((y0, x0, h, w), _HostSinks(tex=True, out_tex=out, tex_u8=uint8)).out_tex

    def both(self, y0, x0, h, w, out_heightmap=None, out_texture=None, uint8=False):
        """(heightmap, texture) of one rectangle from one pass over the chunks; bit for bit the two separate calls"""
        return self._request((y0, x0, h, w), _HostSinks(hm=True, tex=True, out_hm=out_heightmap, out_tex=out_texture,
                                                        hm_u8=uint8, tex_u8=uint8)).outs

    def scene(self, y0, x0, h, w, resident=False, sky=None, **kw):
        """the rectangle as a render.Scene with origin (y0, x0): ``both`` in float32, uploaded once.  Cameras are
        given in world coordinates.  kw: height_scale.  Close it, or use it as a context manager.
        resident=True assembles the same scene on the device: the chunks' and the accumulator's rows are mapped
        and written straight into the scene's planes, nothing visits the host; the planes, and so every render, are bit for
        bit the default's.
        sky: a skylight.SkyLight: the scene is lit from the sky.  Its plane is baked from the heights of the
        rectangle grown by sky.reach all round (``heightmap`` of the grown rectangle; resident: a heightmap-only request into
        a transient device plane), from the same chunks, so the baked value of a world pixel does not depend on the scene
        that contains it."""
        from .render import Scene
        sky = _check_sky(sky)
        if resident:
            return self._resident_scene(y0, x0, h, w, sky=sky, **kw)
        if sky is None:
            hm, tex = self.both(y0, x0, h, w)
            margin = 0
        else:
            margin = sky.reach
            hm = self.heightmap(y0 - margin, x0 - margin, h + 2 * margin, w + 2 * margin)
            tex = self.texture(y0, x0, h, w)
        return Scene(hm, tex, origin=(y0, x0), value_range=(self.model.is_a_grayscale, self.model.is_b_grayscale),
                     device=self.model.device, sky=sky, margin=margin, **kw)

    def _fill_planes(self, dev, requests, flag, what):
        """requests [(rect, hm_ptr, tex_ptr)] into device planes (_flagged_planes), then one read of the flag they share"""
        for rect, hm, tex in requests:
            self._request(rect, _SceneSinks(hm_ptr=hm, tex_ptr=tex, flag_ptr=flag))
        seen = np.zeros(1, np.int32)
        dev.d2h(seen, flag, 4)
        if seen[0]:
            raise ValueError("%s non-finite values" % what)

    def _resident_scene(self, y0, x0, h, w, sky=None, **kw):
        from .render import Scene
        y0, x0, h, w = self._check_region(y0, x0, h, w)
        if h < 2 or w < 2 or h * w >= 1 << 31:
            raise ValueError("a scene is at least 2 x 2 and below 2^31 pixels, got %d x %d" % (h, w))
        if self._closed:
            raise ValueError("this TerrainWorld is closed")
        dev = self.model.device
        margin = 0 if sky is None else sky.reach
        # the height plane, three texture planes
        with _flagged_planes(dev, (4 * h * w, 12 * h * w), sync=False) as (alloc, hm, tex, flag):
            requests, grown = [((y0, x0, h, w), hm, tex)], None
            if sky is not None:
                # the height plane of the grown rectangle: the same chunks, mapped as the scene's own plane is
                gh, gw = h + 2 * margin, w + 2 * margin
                if gh * gw >= 1 << 31:
                    raise ValueError("the scene grown by the sky's reach, %d x %d, is beyond 2^31 pixels" % (gh, gw))
                grown = alloc(4 * gh * gw)
                requests.insert(0, ((y0 - margin, x0 - margin, gh, gw), grown, None))
            self._fill_planes(dev, requests, flag, "the heightmap or the texture has")
            alloc.keep(tex, *(plane for _, plane, _ in requests))    # all but the flag is the scene's from here
        return Scene.from_device(dev, hm, tex, h, w, origin=(y0, x0), sky=sky, sky_src=grown, margin=margin, **kw)

    def mesh(self, y0, x0, h, w, max_error, tile=256, texture=False, fused=None):
        """the rectangle as an adaptive triangle mesh (mesh.TerrainMesh) with the (h + 1) x (w + 1) vertices
        [y0, y0 + h] x [x0, x0 + w] and origin (y0, x0); heights in [0, 1], mapped as a scene's.  y0, x0, h, w are multiples
        of ``tile``.  The height plane of the rectangle grown by one ring of tiles is assembled on the device (a
        heightmap-only request into a transient plane, nothing visits the host), its error map is computed there, and the
        extraction is restricted to the inner tiles: the errors there are those of the unbounded forest, so meshes of
        neighbouring rectangles, made at any time, share their border vertices and edges bit for bit.  An eroded world
        meshes as the eroded world.  texture=True: returns (mesh, self.texture(y0, x0, h + 1, w + 1, uint8=True)).
        fused: mesh.ErrorMap's."""
        from . import mesh as _mesh
        _mesh._tile_log2(tile)
        tol = _mesh._check_error(max_error)
        tile = int(tile)
        for name, v in (("y0", y0), ("x0", x0), ("h", h), ("w", w)):
            if not _is_int(v) or v % tile:
                raise ValueError("%s must be a multiple of the tile (%d), got %r" % (name, tile, v))
        if h < tile or w < tile:
            raise ValueError("the region must be at least one tile (%d) each way, got %d x %d" % (tile, h, w))
        if self._closed:
            raise ValueError("this TerrainWorld is closed")
        gh, gw = h + 2 * tile + 1, w + 2 * tile + 1
        if gh * gw >= 1 << 31:
            raise ValueError("the region grown by a ring of tiles, %d x %d, is at or beyond 2^31 vertices" % (gh, gw))
        gy, gx, gh, gw = self._check_region(y0 - tile, x0 - tile, gh, gw)
        self._bind()
        with _flagged_planes(self._dev, (4 * gh * gw,), sync=True) as (_, grown, flag):
            self._fill_planes(self._dev, [((gy, gx, gh, gw), grown, None)], flag, "the heightmap has")
            with _mesh.ErrorMap(self._ops, _mesh.DevicePlane(grown, gh, gw), tile=tile, fused=fused, origin=(gy, gx),
                                own=False) as em:
                m = em.extract(tol, rect=(tile, tile, int(h), int(w)))
        if texture:
            return m, self.texture(int(y0), int(x0), int(h) + 1, int(w) + 1, uint8=True)
        return m

    def _unit_height(self, y0, x0, h, w):
        """``self.heightmap(y0, x0, h, w)`` as one float32 plane in [0, 1], mapped as a scene's (the channels' mean)"""
        from .render import _unit_planes
        hm = _unit_planes(self.heightmap(y0, x0, h, w), bool(self.model.is_a_grayscale), "heightmap")
        return hm[0] if hm.shape[0] == 1 else hm.astype(np.float64).mean(0).astype(np.float32)

    def hydrology(self, y0, x0, h, w, **kw):
        """the hydrology (hydrology.Hydrology) of ``self.heightmap(y0, x0, h, w)``, heights mapped as a scene's; a
        plain or an eroded world.  kw: hydrology.analyse's (tiled, keep).
        Drainage is a property of the rectangle, whose edge is the outlet: water that would flow on across the edge leaves
        the map there, lakes cut by the edge are not filled, and areas count cells of the rectangle alone.  Unlike every
        other query of the world, two rectangles do NOT agree where they overlap.  Nothing is cached and no seam is handled."""
        from .hydrology import analyse
        hm = self._unit_height(y0, x0, h, w)                      # (the first request binds _ops)
        return analyse(self._ops, hm, **kw)

    def routes(self, y0, x0, h, w, sources, hydrology=False, **kw):
        """the least-cost travel field (route.CostField) of ``self.heightmap(y0, x0, h, w)``, heights mapped as a
        scene's; a plain or an eroded world.  sources: (row, col) cells in world coordinates inside the rectangle; the field's
        ``origin`` is (y0, x0), so ``travel_cost`` and ``path`` take and return world coordinates too.  hydrology=True analyses
        the rectangle first (``self.hydrology``) and routes on its filled surface, lakes and rivers costing travel.lake and
        travel.ford.  kw: route.field's (travel, penalty, tiled, keep).
        Routes are a property of the rectangle: ways that would leave it and come back are not seen, and with hydrology=True
        the drainage is the rectangle's too.  Unlike every other query of the world, two rectangles do NOT agree where they
        overlap.  Nothing is cached and no seam is handled."""
        from .route import field
        y0, x0 = int(y0), int(x0)
        if hydrology:
            hydro = self.hydrology(y0, x0, h, w, tiled=kw.get('tiled'))
            return field(self._ops, hydro.filled, sources, hydro=hydro, origin=(y0, x0), **kw)
        hm = self._unit_height(y0, x0, h, w)
        return field(self._ops, hm, sources, origin=(y0, x0), **kw)

    def earthworks(self, y0, x0, h, w, sources=None, targets=(), rivers=True, channel=None, roadbed=None, travel=None, tiled=None):
        """the ground of ``self.heightmap(y0, x0, h, w)`` with its river channels cut and its roads graded (earthworks, DESIGN
        §4v), heights mapped as a scene's; a plain or an eroded world.  The rectangle's hydrology is analysed
        (``self.hydrology``) and, with rivers=True, the rivers are cut into its filled surface (channel: an
        earthworks.Channel).  With ``sources`` -- (row, col) cells in world coordinates inside the rectangle -- the travel field
        is computed on the filled surface with ``hydro=`` (travel: a route.Travel) and the paths from ``targets`` (world
        coordinates too) are graded into the river-cut surface (roadbed: an earthworks.Roadbed).  tiled: the form of every
        step.  Returns a WorldEarthworks record: ``height`` (float32 (h, w)), ``hydro``, ``cost_field`` (None without sources;
        its origin is (y0, x0)) and ``paths`` (world coordinates).
        Earthworks are a property of the rectangle, as its hydrology and its routes are: two rectangles do NOT agree where
        they overlap.  Nothing is cached and no seam is handled."""
        from . import earthworks as _ew
        from .route import field
        y0, x0 = int(y0), int(x0)
        hydro = self.hydrology(y0, x0, h, w, tiled=tiled)
        height = hydro.filled
        if rivers:
            height = _ew.cut_rivers(self._ops, hydro, channel, tiled=tiled, origin=(y0, x0)).height
        cf, paths = None, []
        if sources is not None:
            cf = field(self._ops, hydro.filled, sources, travel, hydro=hydro, tiled=tiled, origin=(y0, x0))
            paths = cf.paths(targets)
            if paths:
                height = _ew.grade_roads(self._ops, height, cf, paths, roadbed, tiled=tiled).height
        return WorldEarthworks(height, hydro, cf, paths)

    def scatter(self, y0, x0, h, w, species, hydrology=False, roads=None, seed=None, **kw):
        """trees and rocks placed on ``self.heightmap(y0, x0, h, w)`` (scatter.Scatter), heights mapped as a
        scene's; a plain or an eroded world.  species: a scatter.Species or a list of them; the points come in world
        coordinates (the Scatter's ``origin`` is (y0, x0)).  hydrology=True analyses the rectangle first (``self.hydrology``),
        places on its filled surface and keeps the habitats' clearances from its lakes and rivers; roads: an integer or
        boolean plane (h, w), non-zero on road cells -- ``route.raster(shape, paths, (y0, x0))`` of a field's paths, or its
        traffic against a threshold.  seed: the draws' seed, default the world's.  kw: scatter.scatter's (blocked,
        height_scale, tiled, keep).
        Candidates and priorities are functions of the seed and the world position, and the chance without hydrology and
        roads is one of the heights around a cell: two rectangles agree on them where they overlap (one cell inside the
        edge, where the slope sees the neighbour).  The thinned set is NOT: like drainage and routes it belongs to the
        rectangle, whose edge ends the search for conflicts, and with hydrology=True the wet ground is the rectangle's too.
        Nothing is cached and no seam is handled."""
        from .scatter import scatter
        y0, x0 = int(y0), int(x0)
        seed = self.seed if seed is None else seed
        if hydrology:
            hydro = self.hydrology(y0, x0, h, w, tiled=kw.get('tiled'), keep=('filled', 'depth', 'accumulation'))
            return scatter(self._ops, hydro.filled, species, seed=seed, origin=(y0, x0), hydro=hydro, roads=roads, **kw)
        hm = self._unit_height(y0, x0, h, w)
        return scatter(self._ops, hm, species, seed=seed, origin=(y0, x0), roads=roads, **kw)

    def viewshed(self, y0, x0, h, w, observers, sight=None, accel=None):
        """what ``observers`` see of ``self.heightmap(y0, x0, h, w)`` (viewshed.Viewshed), heights mapped as a
        scene's; a plain or an eroded world.  observers: (row, col), (row, col, eye_height) or (row, col, eye_height, max_dist)
        each, in world coordinates and inside the rectangle; the Viewshed's ``origin`` is (y0, x0) and its ``observers`` are in
        world coordinates.  sight: a viewshed.Sight; accel: the form.
        A sight line reads only the cells between its two ends, so visibility is a property of the world, not of the
        rectangle: unlike hydrology, routes, earthworks and scatter, two rectangles that both hold the observers agree bit
        for bit where they overlap, on ``count`` and on ``mask``.  Nothing is cached."""
        from .viewshed import viewshed
        y0, x0 = int(y0), int(x0)
        hm = self._unit_height(y0, x0, h, w)
        return viewshed(self._ops, hm, observers, sight, accel, origin=(y0, x0))

    def contours(self, y0, x0, h, w, levels=None):
        """the contour lines of ``self.heightmap(y0, x0, h, w)`` (contour.Contours), heights mapped as a scene's; a
        plain or an eroded world.  levels: a contour.Levels; the Contours' ``origin`` is (y0, x0) and its ``points`` are in world
        coordinates.
        A vertex reads the two cells at the ends of its grid edge and a segment the four corners of its cell, so the segments
        are a property of the world, not of the rectangle: two rectangles' ``segments()`` agree bit for bit on every cell both
        contain (``segments(within=...)`` keeps a rectangle's).  The lines themselves are NOT: they belong to the rectangle,
        which cuts them at its edge, so where they start, how they are numbered and whether they close depends on it.
        Nothing is cached."""
        from .contour import contours
        y0, x0 = int(y0), int(x0)
        hm = self._unit_height(y0, x0, h, w)
        return contours(self._ops, hm, levels, origin=(y0, x0))

    def peaks(self, y0, x0, h, w, prominence=None):
        """the peaks of ``self.heightmap(y0, x0, h, w)`` (peaks.Peaks), heights mapped as a scene's; a plain or an
        eroded world.  prominence: a peaks.Prominence; the Peaks' ``origin`` is (y0, x0), its ``cell`` and ``col`` are in world
        coordinates.
        Peaks belong to the rectangle, like drainage and routes: a mountain the edge cuts is ranked by what is inside (``on_edge``
        marks the summits on the border), ties between equal heights are broken by the rectangle's own cell order, and two
        rectangles do NOT agree where they overlap.  Nothing is cached."""
        from .peaks import peaks
        y0, x0 = int(y0), int(x0)
        hm = self._unit_height(y0, x0, h, w)
        return peaks(self._ops, hm, prominence, origin=(y0, x0))

    def rivers(self, y0, x0, h, w, network=None):
        """the rivers of ``self.heightmap(y0, x0, h, w)`` (rivers.Rivers): ``self.hydrology`` of the rectangle, then
        its stream network; a plain or an eroded world.  network: a rivers.Network; the Rivers' ``origin`` is (y0, x0) and its
        ``points`` are in world coordinates.
        Rivers belong to the rectangle, like the drainage they are built on: its edge is the outlet, areas count cells of the
        rectangle alone, so orders and main stems are the rectangle's and two rectangles do NOT agree where they overlap.
        Nothing is cached and no seam is handled."""
        from .rivers import rivers
        y0, x0 = int(y0), int(x0)
        hydro = self.hydrology(y0, x0, h, w, keep=('filled', 'depth', 'direction', 'accumulation'))
        return rivers(self._ops, hydro, network, origin=(y0, x0))

    def regions(self, y0, x0, h, w, of='lakes', areas=None, form=None, sea_level=None, levels=None, **kw):
        """the areas of ``self.heightmap(y0, x0, h, w)`` as polygons with holes (regions.Regions), heights mapped as
        a scene's; a plain or an eroded world.  of: 'lakes' or 'basins' (``self.hydrology`` of the rectangle first), 'land'
        (above sea_level, a number in [0, 1]) or 'bands' (between the levels of a contour.Levels); areas: a regions.Areas; kw:
        regions.regions' (keep, max_edges).  The Regions' ``origin`` is (y0, x0) and its ``points`` are in world coordinates.
        Polygons belong to the rectangle, whose edge closes them: a lake, a basin or a band the edge cuts ends there, with the
        edge as part of its ring, and its cells count the rectangle's alone; lakes and basins besides are the rectangle's
        drainage's.  Two rectangles do NOT agree where they overlap.  Nothing is cached and no seam is handled."""
        from . import regions as _rg
        y0, x0 = int(y0), int(x0)
        if of == 'lakes':
            labels = _rg.lakes(self.hydrology(y0, x0, h, w, keep=('depth',)))
        elif of == 'basins':
            labels = _rg.basins(self.hydrology(y0, x0, h, w, keep=('basin',)))
        elif of == 'land':
            if sea_level is None:
                raise ValueError("of='land' needs sea_level")
            labels = _rg.land(self._unit_height(y0, x0, h, w), sea_level)
        elif of == 'bands':
            labels = _rg.bands(self._unit_height(y0, x0, h, w), levels)
        else:
            raise ValueError("of must be 'lakes', 'basins', 'land' or 'bands', got %r" % (of,))
        return _rg.regions(self._ops, labels, areas, origin=(y0, x0), form=form, **kw)

    def climate(self, y0, x0, h, w, weather=None, biomes=None, hydrology=False, **kw):
        """the climate of ``self.heightmap(y0, x0, h, w)`` (climate.Climate), heights mapped as a scene's; a plain
        or an eroded world.  weather: a climate.Weather; biomes: a climate.Biomes; hydrology=True analyses the rectangle first
        (``self.hydrology``) and adds the rain-weighted discharge and the effective area; kw: climate.analyse's (form, keep).
        The Climate's ``origin`` is (y0, x0), and world row y0 + r enters the temperature of its row r.
        ``temperature`` reads the cell and its world row alone, so it is a property of the world: two rectangles agree on it bit
        for bit where they overlap.  ``rain``, ``biome``, ``discharge`` and ``effective_area`` are NOT: they belong to the
        rectangle, whose upwind edge is where the vapour enters with the weather's humidity, just as its edge is the outlet of
        its drainage.  Nothing is cached and no seam is handled."""
        from . import climate as _cl
        y0, x0 = int(y0), int(x0)
        hm = self._unit_height(y0, x0, h, w)                      # (the first request binds _ops)
        hydro = self.hydrology(y0, x0, h, w, keep=('direction',)) if hydrology else None
        return _cl.analyse(self._ops, hm, weather, biomes, origin=(y0, x0), hydro=hydro, **kw)

    def sunlight(self, y0, x0, h, w, sun=None, max_margin=1024, form=None):
        """where the sun shines on ``self.heightmap(y0, x0, h, w)`` (sunlight.Sunlight), heights mapped as a
        scene's; a plain or an eroded world.  sun: a sunlight.Sun (default sunlight.Day().sun()); form: the form.  The
        rectangle is analysed grown by min(sun.reach, max_margin) cells on every side and cropped; the Sunlight's ``origin`` is
        (y0, x0).  No ray reads further than the sun's reach from its cell, so where the reach fits the margin
        (``Sunlight.exact``) sunlight is a property of the world: two rectangles agree bit for bit where they overlap, on every
        plane.  Where the margin caps it the planes belong to the rectangle, whose grown edge lets the low sun in.  Nothing is
        cached."""
        from . import sunlight as _sl
        y0, x0, h, w = int(y0), int(x0), int(h), int(w)
        sun = _sl._check_sun(sun)
        if not _sl._is_int(max_margin) or max_margin < 0:
            raise ValueError("max_margin must be an integer >= 0, got %r" % (max_margin,))
        m = min(sun.reach, int(max_margin))
        hm = self._unit_height(y0 - m, x0 - m, h + 2 * m, w + 2 * m)
        whole = _sl.sunlight(self._ops, hm, sun, form, origin=(y0 - m, x0 - m))
        return whole.crop(m, m, h, w, exact=sun.reach <= int(max_margin))

    def flight_plan(self, cameras, max_dist, window_mb=1024, snap=None, sky=None):
        """the scene windows ``flight`` moves through: [((y0, x0, h, w), first_frame, last_frame)].  Pure arithmetic, no
        device.  Frame k's footprint is cameras[k].footprint(max_dist).  Starting at frame i, a window takes the longest run of
        consecutive frames i .. j such that the union of their footprints, expanded outward to multiples of ``snap``
        (default in_shp), has at most max_pixels = floor(window_mb 2^20 / 22) pixels: a scene keeps 22 bytes per pixel
        (SCENE_BYTES_PER_PIXEL: 4 of height, 12 of texture, 16/3 of pyramid, rounded up).  The next window starts at j + 1.  A
        frame whose own snapped footprint exceeds the cap is a ValueError.  Deterministic in its arguments alone.
        sky: a skylight.SkyLight: the windows are lit from the sky and planned with 26 bytes per pixel
        (SKY_SCENE_BYTES_PER_PIXEL: the 22 and the baked plane's 4).  The height plane grown by sky.reach that a window's bake
        reads is transient -- allocated before the bake, freed after it -- and outside this budget."""
        bpp = SCENE_BYTES_PER_PIXEL if _check_sky(sky) is None else SKY_SCENE_BYTES_PER_PIXEL
        if not _is_number(window_mb, finite=False) or not window_mb > 0:
            raise ValueError("window_mb must be a number > 0, got %r" % (window_mb,))
        snap = self._geo.out if snap is None else snap
        return plan_windows([c.footprint(max_dist) for c in cameras], snap, int(window_mb * (1 << 20)) // bpp)

    def flight(self, cameras, max_dist, window_mb=1024, snap=None, height_scale=None, sky=None, **render_kw):
        """the images of a camera path of any length, one per camera and in order, from bounded device memory:
        for each window of flight_plan one resident scene is built, its frames are rendered (one launch and one download
        each), and it is closed before the next is built; chunks that consecutive windows share come from the cache.
        Frame k is bit for bit Scene(*world.both(*rect), origin=rect[:2], ...).render(cameras[k], max_dist=max_dist, ...)
        for its window's rect.  The plan is made, and its refusals raised, by this call; the device works as the returned
        generator is consumed.  render_kw: Scene.render's.
        sky: a skylight.SkyLight: every window is lit from the sky, and frame k is bit for bit the host-path
        world.scene(*rect, sky=sky) rendered.  The plan counts the baked plane (flight_plan); the grown height plane of a
        window's bake lives only while the window is built and is outside window_mb."""
        cameras = list(cameras)
        if self._closed:
            raise ValueError("this TerrainWorld is closed")
        plan = self.flight_plan(cameras, max_dist, window_mb, snap, sky=sky)
        skw = {} if height_scale is None else {"height_scale": height_scale}

        def frames():
            for rect, i, j in plan:
                with self.scene(*rect, resident=True, sky=sky, **skw) as scene:
                    for k in range(i, j + 1):
                        yield scene.render(cameras[k], max_dist=max_dist, **render_kw)
        return frames()

    def view(self, camera, max_dist, height_scale=None, sky=None, **kw):
        """one image of the world from ``camera`` (world coordinates, negative ones included), rays ``max_dist`` long: the
        scene of camera.footprint(max_dist), rendered.  sky: a skylight.SkyLight, the scene is lit from the sky.  kw:
        Scene.render's."""
        skw = {} if height_scale is None else {"height_scale": height_scale}
        with self.scene(*camera.footprint(max_dist), sky=sky, **skw) as scene:
            return scene.render(camera, max_dist=max_dist, **kw)

    def _request(self, rect, sink):
        """the chunks, the tiles and the accumulator of one rectangle; finished rows leave through ``sink`` (returned), which
        says what is wanted: the host's arrays (_HostSinks), or the device planes of a render scene (_SceneSinks).  A sink
        plans its outputs (plan_hm before anything touches a device), is opened once the engine is idle, and closed"""
        y0, x0, h, w = rect = self._check_region(*rect)
        sink.world, sink.rect, sink.hdone = self, rect, []
        geo, K, C = self._geo, self._K, self._geo.channels
        want_hm, want_tex = sink.want_hm, sink.want_tex
        if want_hm:
            sink.plan_hm()
        self._bind()
        eng, udev, uops = self._eng, self._udev, self._uops
        T, o, B = geo.out, self.overlap, self.batch_size
        st = T - o
        if want_tex:
            plan, prog = eng._infer_plan('p2p_gen', B, True)
            inp, u = plan.input_nodes[0].out, plan.out
            c_out = u.Cc
            if (inp.H, inp.W, u.H, u.W) != (T, T, T, T) or inp.Cc != C:
                raise ValueError("the pix2pix generator takes %d x %d x %d tiles, the heightmap generator makes %d x %d x %d"
                                 % (inp.Cc, inp.H, inp.W, C, T, T))
            sink.plan_tex(c_out)
        a_lo, a_hi = axis_chunks(y0, h, K)
        b_lo, b_hi = axis_chunks(x0, w, K)
        eng.sync()
        acc = None
        sink.open()
        try:
            # ---- heightmap rows: one sink call per chunk row ----
            if want_hm:
                sink.begin_hm()
            if not want_tex:
                for a in range(a_lo, a_hi + 1):
                    self._acquire([(a, b) for b in range(b_lo, b_hi + 1)])
                    sink.hm_row(a, b_lo, b_hi)
            else:
                # ---- texture: §4j's executor over world-anchored tiles, as the interior of a plan one tile larger ----
                p_lo, p_hi = axis_tiles(y0, h, T, o)
                q_lo, q_hi = axis_tiles(x0, w, T, o)
                ny, nx = p_hi - p_lo + 3, q_hi - q_lo + 3
                pad_y, pad_x = y0 - p_lo * st + st, x0 - q_lo * st + st
                Wp = (w + 3) // 4 * 4                         # whole 16-byte groups per accumulator row
                tb_lo, tb_hi = (q_lo * st) // K, (q_hi * st + T - 1) // K
                batches = slot_batches(q_lo, q_hi, B)
                acc_bytes = c_out * T * Wp * 4
                acc = udev.alloc(acc_bytes)
                sink.begin_tex(c_out, Wp)
                udev.memset_zero(acc, acc_bytes)

                for p in range(p_lo, p_hi + 1):
                    ty = p * st
                    ta_lo, ta_hi = ty // K, (ty + T - 1) // K
                    self._acquire([(a, b) for a in range(ta_lo, ta_hi + 1) for b in range(tb_lo, tb_hi + 1)])
                    if want_hm:
                        for a in range(max(ta_lo, a_lo), min(ta_hi, a_hi) + 1):
                            if a not in sink.hdone:
                                sink.hm_row(a, b_lo, b_hi)
                    for qs, slot0, nb in batches:
                        tiles = []
                        for q in qs:
                            tx = q * st
                            a0, b0 = ta_lo, tx // K
                            ly, lx = ty - a0 * K, tx - b0 * K
                            down, right = ly + T > K, lx + T > K
                            tiles.append(((self._chunks[(a0, b0)], self._chunks[(a0, b0 + 1)] if right else 0,
                                           self._chunks[(a0 + 1, b0)] if down else 0,
                                           self._chunks[(a0 + 1, b0 + 1)] if down and right else 0), ly, lx))
                        uops.world_gather(tiles, K, inp)
                        for e in prog:
                            e[1]()
                        q0 = qs[slot0]
                        uops.texture_blend(acc, Wp, T, c_out, u.samples(slot0, B), nb, p - p_lo + 1, ny, q0 - q_lo + 1, nx,
                                           pad_x, o)
                    # rows no later tile row touches: the first st of the band (all of it for the last), inside the request
                    last = p == p_hi
                    yr = ty - y0
                    r_lo, r_hi = max(0, -yr), min(T if last else st, h - yr)
                    if r_hi > r_lo:
                        sink.tex_rows(acc, r_lo, r_hi - r_lo, yr, ny, pad_y, nx, pad_x)
                    if not last:
                        shift_accumulator(udev, acc, c_out, T, Wp * 4, o)
                    sink.tex_poll()
            sink.finish()
            eng.sync()
        finally:
            eng.sync()
            sink.close()
            if acc is not None:
                udev.free(acc)
            self._release()
        return sink


# ---- command line -------------------------------------------------------------------------------------------------------
def parse_region(text):
    m = re.fullmatch(r"\s*([+-]?\d+)\s*,\s*([+-]?\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*", text)
    if not m or int(m.group(3)) < 1 or int(m.group(4)) < 1:
        raise argparse.ArgumentTypeError("--region wants Y0,X0,H,W with H, W >= 1, got %r" % (text,))
    return tuple(int(g) for g in m.groups())


def parse_args(argv):
    p = argparse.ArgumentParser(prog="python -m gan_heightmaps_amd.world",
                                description="Write the H x W pixels at (Y0, X0) of the unbounded world of a seed, and "
                                            "optionally their texture.  Regions written at different times fit together.")
    p.add_argument("experiment", help="experiment name (gan_heightmaps_amd.experiments), e.g. test1_nobn_bilin_both")
    p.add_argument("model", help="checkpoint written by save_model / save_checkpoint")
    p.add_argument("output", help="heightmap: .png (8-bit), or .npy (float32 (C, H, W), written through open_memmap)")
    p.add_argument("--seed", type=int, required=True, help="the world's seed")
    p.add_argument("--region", type=parse_region, required=True, metavar="Y0,X0,H,W",
                   help="the rectangle in world pixels; the origin may be negative (write --region=-70,33,150,97)")
    p.add_argument("--chunk-cells", type=int, default=None,
                   help="generator cells per chunk side (default: the memory budget's); part of the world's identity")
    p.add_argument("--blend", default="bilinear", choices=list(BLENDS), help="how cells meet in the seed canvas")
    p.add_argument("--dtype", default="bf16x3", choices=["f32", "bf16x3", "bf16x2", "bf16", "f16"],
                   help="arithmetic of the convolutions (default bf16x3)")
    p.add_argument("--texture", default=None, metavar="OUT_TEX",
                   help="also texture the region with the pix2pix generator: .png, or .npy (uint8 (H, W, 3))")
    p.add_argument("--overlap", type=int, default=None, help="texture tile overlap in pixels (default in_shp / 4)")
    p.add_argument("--batch-size", type=int, default=4, help="texture tiles per forward pass (default 4)")
    p.add_argument("--erode", type=int, default=None, metavar="N",
                   help="erode the world with N iterations of the water simulation (erosion.Erosion's other defaults); "
                        "part of the world's identity")
    p.add_argument("--mesh", default=None, metavar="OUT_MESH",
                   help="also write the region as an adaptive triangle mesh: .glb, .obj or .npz, with the (H + 1) x (W + 1) "
                        "vertices [Y0, Y0 + H] x [X0, X0 + W]; the region must be made of whole tiles; with --texture the "
                        "mesh carries the texture")
    p.add_argument("--max-error", type=float, default=None, metavar="E",
                   help="the mesh's tolerance in height units (heights are in [0, 1]; default 0.01)")
    p.add_argument("--tile", type=int, default=None, metavar="T",
                   help="the mesh's root square side, a power of two (default 256)")
    from .route import parse_cell
    p.add_argument("--routes", default=None, metavar="OUT_PREFIX",
                   help="also write the least-cost travel field of the region from the --from cells (world coordinates): "
                        "OUT_PREFIX.cost.npy, .parent.npy, .territory.npy, .traffic.npy, and one OUT_PREFIX.path<i>.npy per --to")
    p.add_argument("--from", dest="sources", type=parse_cell, action="append", metavar="Y,X", default=[],
                   help="a source of --routes, inside the region; repeat for more")
    p.add_argument("--to", dest="targets", type=parse_cell, action="append", metavar="Y,X", default=[],
                   help="a cell whose path to its source --routes writes; repeat for more")
    p.add_argument("--earthworks", default=None, metavar="OUT",
                   help="also write the region's ground with its river channels cut and, with --routes, the roads from the --to "
                        "cells graded (earthworks' defaults): .npy (float32 (H, W)), or PNG")
    p.add_argument("--scatter", default=None, metavar="OUT",
                   help="also write the points of one species placed on the region by Poisson-disk sampling (scatter's "
                        "defaults, the world's seed): .npz or .csv; needs --spacing")
    p.add_argument("--spacing", type=float, default=None, metavar="X", help="the spacing of --scatter, in cells (0 < X <= 32)")
    p.add_argument("--viewshed", default=None, metavar="OUT",
                   help="also write what observers at the --from cells (world coordinates) see of the region (viewshed's "
                        "defaults): .npz (count, mask, observers) or .png (255 where seen)")
    p.add_argument("--contours", default=None, metavar="OUT",
                   help="also write the region's contour lines in world coordinates (contour's height scale): .svg, .geojson or "
                        ".npz; --interval, --base, --count and --index-every choose the levels")
    from . import contour as _contour
    _contour.add_level_arguments(p)
    p.add_argument("--peaks", default=None, metavar="OUT",
                   help="also write the region's peaks in world coordinates (peaks' height scale): .geojson, .csv or .npz; "
                        "--min-prominence and --top choose them; with --contours OUT.svg the sheet gets their spot heights")
    from . import peaks as _peaks
    _peaks.add_prominence_arguments(p)
    p.add_argument("--rivers", default=None, metavar="OUT",
                   help="also write the region's rivers in world coordinates, ordered reaches with their Strahler orders: .svg, "
                        ".geojson or .npz; --river-threshold and --min-order choose them; with --contours OUT.svg or OUT.geojson "
                        "the sheet gets their blue lines")
    from . import rivers as _rivers
    _rivers.add_network_arguments(p)
    p.add_argument("--regions", default=None, metavar="OUT",
                   help="also write the region's areas in world coordinates as polygons with holes: .svg, .geojson or .npz; --of "
                        "says which areas (bands takes the levels of --interval and --base); with --contours OUT.svg or OUT.geojson "
                        "the sheet gets them filled beneath its lines")
    p.add_argument("--of", default=None, choices=("lakes", "basins", "land", "bands"), help="the areas --regions writes")
    p.add_argument("--sea-level", type=float, default=None, metavar="X", help="--of land and --climate: the sea level, in [0, 1]")
    p.add_argument("--climate", default=None, metavar="OUT_PREFIX",
                   help="also write the region's climate: OUT_PREFIX.rain.npy, .temperature.npy and .biome.npy (a name that ends in "
                        ".npz: one archive); --wind and --sea-level choose the weather")
    p.add_argument("--wind", default=None, metavar="D", help="--climate: the side the wind comes from, N NE E SE S SW W or NW")
    p.add_argument("--sunlight", default=None, metavar="OUT",
                   help="also write where the sun shines on the region over one day (sunlight's .npz, or a .png of the hours); "
                        "--latitude and --declination choose the day")
    p.add_argument("--latitude", type=float, default=None, metavar="X", help="--sunlight: degrees north (default 45)")
    p.add_argument("--declination", type=float, default=None, metavar="X", help="--sunlight: the sun's declination in degrees (default 0)")
    from . import regions as _regions
    _regions.add_area_arguments(p)
    # a region or a cell that starts with a negative number would read as an option: hand it over in the --region=... form
    argv = list(argv)
    for i in range(len(argv) - 2, -1, -1):
        if argv[i] in ("--region", "--from", "--to", "--base") and re.match(r"\s*-\d", argv[i + 1]):
            argv[i:i + 2] = [argv[i] + "=" + argv[i + 1]]
    a = p.parse_args(argv)
    if a.routes is None and (a.targets or (a.sources and a.viewshed is None)):
        p.error("--from / --to need --routes (--from alone: or --viewshed)")
    if a.routes is not None or a.viewshed is not None:
        if not a.sources:
            p.error("--routes and --viewshed need at least one --from Y,X")
        y0, x0, h, w = a.region
        for y, x in a.sources + a.targets:
            if not (y0 <= y < y0 + h and x0 <= x < x0 + w):
                p.error("the cell %d,%d lies outside the region %s" % (y, x, (a.region,)))
    if a.viewshed is not None:
        from .viewshed import MAX_OBSERVERS
        if not (a.viewshed.endswith(".npz") or a.viewshed.lower().endswith(".png")):
            p.error("--viewshed writes .npz or .png")
        if len(a.sources) > MAX_OBSERVERS:
            p.error("--viewshed takes at most %d --from cells" % MAX_OBSERVERS)
    chosen = (a.interval, a.base, a.count, a.index_every)
    if a.regions is None:
        if a.of is not None or (a.sea_level is not None and a.climate is None) or (a.min_cells, a.holes) != (_regions.Areas().min_cells, True):
            p.error("--of / --sea-level / --min-cells / --no-holes need --regions")
    else:
        if not a.regions.lower().endswith((".svg", ".geojson", ".npz")):
            p.error("--regions writes .svg, .geojson or .npz")
        if a.of is None:
            p.error("--regions needs --of")
        if (a.of == "land") != (a.sea_level is not None) and not (a.of != "land" and a.climate is not None):
            p.error("--of land and --sea-level go together")
        try:
            a.areas = _regions.Areas(a.min_cells, a.holes)
            if a.sea_level is not None and not 0 <= a.sea_level <= 1:
                raise ValueError("--sea-level must lie in [0, 1], got %r" % (a.sea_level,))
            a.band_levels = _contour.Levels(a.interval, a.base)
        except ValueError as e:
            p.error(str(e))
    if a.climate is None:
        if a.wind is not None:
            p.error("--wind needs --climate")
    else:
        from . import climate as _climate
        try:
            d = _climate.Weather()
            a.weather = _climate.Weather(wind=d.wind if a.wind is None else a.wind, sea_level=d.sea_level if a.sea_level is None else a.sea_level)
        except ValueError as e:
            p.error(str(e))
    if a.sunlight is None:
        if a.latitude is not None or a.declination is not None:
            p.error("--latitude / --declination need --sunlight")
    else:
        from . import sunlight as _sunlight
        if not (a.sunlight.endswith(".npz") or a.sunlight.lower().endswith(".png")):
            p.error("--sunlight writes .npz or .png")
        try:
            d = _sunlight.Day()
            a.sun = _sunlight.Day(d.latitude if a.latitude is None else a.latitude,
                                  d.declination if a.declination is None else a.declination).sun()
        except ValueError as e:
            p.error(str(e))
    if a.contours is None:
        d = _contour.Levels()
        if chosen != (d.interval, d.base, d.count, d.index_every) and not (a.of == "bands" and chosen[2:] == (d.count, d.index_every)):
            p.error("--interval / --base / --count / --index-every need --contours")
    else:
        if not a.contours.lower().endswith((".svg", ".geojson", ".npz")):
            p.error("--contours writes .svg, .geojson or .npz")
        try:
            a.levels = _contour.Levels(*chosen)
        except ValueError as e:
            p.error(str(e))
    if a.peaks is None:
        if (a.min_prominence, a.top) != (_peaks.Prominence().min_prominence, None):
            p.error("--min-prominence / --top need --peaks")
    else:
        if not a.peaks.lower().endswith((".geojson", ".csv", ".npz")):
            p.error("--peaks writes .geojson, .csv or .npz")
        try:
            a.prominence = _peaks.Prominence(a.min_prominence, a.top)
        except ValueError as e:
            p.error(str(e))
    if a.rivers is None:
        if (a.river_threshold, a.min_order) != (_rivers.Network().river_threshold, _rivers.Network().min_order):
            p.error("--river-threshold / --min-order need --rivers")
    else:
        if not a.rivers.lower().endswith((".svg", ".geojson", ".npz")):
            p.error("--rivers writes .svg, .geojson or .npz")
        try:
            a.network = _rivers.Network(a.river_threshold, a.min_order)
        except ValueError as e:
            p.error(str(e))
    if (a.scatter is None) != (a.spacing is None):
        p.error("--scatter and --spacing go together")
    if a.scatter is not None:
        if not (a.scatter.endswith(".npz") or a.scatter.endswith(".csv")):
            p.error("--scatter writes .npz or .csv")
        from .scatter import Species
        try:
            a.species = Species("tree", a.spacing)
        except ValueError as e:
            p.error(str(e))
    if a.chunk_cells is not None and a.chunk_cells < 1:
        p.error("--chunk-cells must be >= 1")
    if not 1 <= a.batch_size <= MAX_BATCH:
        p.error("--batch-size must lie in [1, %d]" % MAX_BATCH)
    if a.overlap is not None and a.overlap < 0:
        p.error("--overlap must be >= 0")
    if a.texture is None and (a.overlap is not None or a.batch_size != 4):
        p.error("--overlap / --batch-size need --texture")
    if a.erode is not None and a.erode < 1:
        p.error("--erode must be >= 1")
    if a.mesh is None:
        if a.max_error is not None or a.tile is not None:
            p.error("--max-error / --tile need --mesh")
    else:
        from . import mesh as _mesh
        a.max_error = 0.01 if a.max_error is None else a.max_error
        a.tile = 256 if a.tile is None else a.tile
        if os.path.splitext(a.mesh)[1].lower() not in (".glb", ".obj", ".npz"):
            p.error("--mesh must be .glb, .obj or .npz")
        try:
            _mesh._tile_log2(a.tile)
            _mesh._check_error(a.max_error)
        except ValueError as e:
            p.error(str(e))
        if any(v % a.tile for v in a.region):
            p.error("--mesh needs a --region made of whole tiles: multiples of %d, got %s" % (a.tile, (a.region,)))
    return a


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    from . import util
    from .experiments import make_model
    model = make_model(a.experiment, dtype=a.dtype, verbose=False)
    model.load_model(a.model, mode='both' if a.texture else 'dcgan')
    y0, x0, h, w = a.region
    wkw = {} if a.erode is None else {"erosion": _erosion.Erosion(iterations=a.erode)}
    with model.terrain_world(a.seed, chunk_cells=a.chunk_cells, blend=a.blend, overlap=a.overlap,
                             batch_size=a.batch_size, verbose=True, **wkw) as world:
        C = world.geometry.channels
        hm = np.lib.format.open_memmap(a.output, mode="w+", dtype=np.float32, shape=(C, h, w)) \
            if a.output.endswith(".npy") else None
        tex = None
        if a.texture:
            tex = np.lib.format.open_memmap(a.texture, mode="w+", dtype=np.uint8, shape=(h, w, 3)) \
                if a.texture.endswith(".npy") else None
            hm, tex = world._request(a.region, _HostSinks(hm=True, tex=True, out_hm=hm, out_tex=tex, tex_u8=True)).outs
        else:
            hm = world.heightmap(y0, x0, h, w, out=hm)
        if a.mesh:
            m = world.mesh(y0, x0, h, w, a.max_error, tile=a.tile, texture=bool(a.texture))
            m, mtex = m if a.texture else (m, None)
            m.save(a.mesh, texture=mtex)
        if a.routes:
            cf = world.routes(y0, x0, h, w, a.sources)
            for k in ("cost", "parent", "territory", "traffic"):
                np.save("%s.%s.npy" % (a.routes, k), getattr(cf, k))
            for i, path in enumerate(cf.paths(a.targets)):
                np.save("%s.path%d.npy" % (a.routes, i), path)
        if a.scatter:
            world.scatter(y0, x0, h, w, a.species).save(a.scatter)
        if a.viewshed:
            world.viewshed(y0, x0, h, w, a.sources).save(a.viewshed)
        found = None
        if a.peaks:
            found = world.peaks(y0, x0, h, w, a.prominence)
            found.save(a.peaks)
        blue = None
        if a.rivers:
            blue = world.rivers(y0, x0, h, w, a.network)
            blue.save(a.rivers)
        if a.climate:
            world.climate(y0, x0, h, w, a.weather).save(a.climate)
        if a.sunlight:
            world.sunlight(y0, x0, h, w, a.sun).save(a.sunlight)
        areas = None
        if a.regions:
            areas = world.regions(y0, x0, h, w, a.of, a.areas, sea_level=a.sea_level, levels=a.band_levels)
            areas.save(a.regions)
        if a.contours:
            spot = found if a.contours.lower().endswith(".svg") else None
            flat = a.contours.lower().endswith(".npz")
            world.contours(y0, x0, h, w, a.levels).save(a.contours, peaks=spot, rivers=None if flat else blue,
                                                        **({} if flat or areas is None else {"regions": areas}))
        if a.earthworks:
            ground = world.earthworks(y0, x0, h, w, a.sources if a.routes else None, a.targets).height
            if a.earthworks.endswith(".npy"):
                np.save(a.earthworks, ground)
            else:
                util.save_png(a.earthworks, util.to_uint8(ground))
    if a.output.endswith(".npy"):
        hm.flush()
    else:
        img = util.to_uint8(util.convert_to_rgb(hm, is_grayscale=model.is_a_grayscale))
        util.save_png(a.output, img[:, :, 0] if C == 1 else img)
    if a.texture:
        if a.texture.endswith(".npy"):
            tex.flush()
        else:
            util.save_png(a.texture, tex)
    model.device.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
