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

    python -m gan_heightmaps_amd.world EXPERIMENT MODEL OUT --seed N --region Y0,X0,H,W [--chunk-cells C]
        [--blend mosaic|bilinear] [--dtype D] [--texture OUT_TEX [--overlap N] [--batch-size B]]
"""
import argparse
import re
import sys
from collections import OrderedDict

import numpy as np

from . import layers as L
from .terrain import BLENDS, INT32_LIMIT, TerrainGeometry
from . import terrain as _terrain
from .texture import check_overlap

__all__ = ["HEAD_BLOCK", "MAX_BATCH", "world_latent", "axis_chunks", "axis_tiles", "seed_cells", "window_elements",
           "default_chunk_cells", "slot_batches", "TerrainWorld", "parse_region", "parse_args", "main"]

HEAD_BLOCK = 8                   # the head runs over world-aligned blocks of HEAD_BLOCK x HEAD_BLOCK cells, one pass each
MAX_BATCH = 32                   # GHM_WORLD_MAX_TILES (include/ghm.h): tiles per forward pass


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


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


class TerrainWorld:
    """An unbounded terrain addressed by pixel coordinates.  See Pix2Pix.terrain_world and the module docstring."""

    def __init__(self, model, seed, chunk_cells=None, blend='bilinear', overlap=None, batch_size=4, cache_mb=1024,
                 latent_fn=None, deterministic=True, verbose=False):
        if not deterministic:
            raise NotImplementedError("terrain_world needs deterministic=True: with batch statistics a pixel would depend "
                                      "on what shares its pass, not on (weights, seed, coordinates) alone")
        if not _is_int(seed):
            raise ValueError("seed must be an integer, got %r" % (seed,))
        if blend not in BLENDS:
            raise ValueError("blend must be one of %s, got %r" % (BLENDS, blend))
        if not _is_int(batch_size) or not 1 <= batch_size <= MAX_BATCH:
            raise ValueError("batch_size must be an integer in [1, %d], got %r" % (MAX_BATCH, batch_size))
        if isinstance(cache_mb, bool) or not isinstance(cache_mb, (int, float, np.integer, np.floating)) or cache_mb < 0:
            raise ValueError("cache_mb must be a number >= 0, got %r" % (cache_mb,))
        if latent_fn is not None and not callable(latent_fn):
            raise ValueError("latent_fn must be callable as latent_fn(i, j)")
        self.model, self.seed, self.blend = model, int(seed), blend
        self.batch_size, self.cache_mb, self.latent_fn = int(batch_size), cache_mb, latent_fn
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
        self._chunk_bytes = geo.channels * self._K * self._K * 4
        self._chunks = OrderedDict()                              # (a, b) -> device pointer, least recently used first
        self._heads = OrderedDict()                               # (I, J) -> DevTensor [HEAD_BLOCK^2, nch s s]
        self._pool, self._pinned, self._table = [], set(), None
        self._version, self._closed = None, False
        self.computed = 0                                         # chunks computed so far (a cache hit computes nothing)
        if verbose:
            print("terrain_world: seed %d, chunk_cells %d (%d px), blend %s, overlap %d"
                  % (self.seed, self._c, self._K, blend, self.overlap))

    chunk_cells = property(lambda self: self._c)
    chunk_px = property(lambda self: self._K)
    geometry = property(lambda self: self._geo)

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
        for p in self._chunks.values():
            self._pool.append(p)
        self._chunks.clear()
        for t in self._heads.values():
            self._dev.free(t.ptr)
        self._heads.clear()
        self._pinned = set()

    def _capacity(self):
        return int(self.cache_mb * (1 << 20)) // self._chunk_bytes

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
        ptr = self._pool.pop() if self._pool else self._dev.alloc(self._chunk_bytes)
        self._ops.world_emit(self._tplan.out, geo.halo * geo.F, geo.halo * geo.F, self._K, ptr)
        self.computed += 1
        return ptr

    def _acquire(self, keys):
        """make the chunks ``keys`` resident (they stay so until the next _acquire), then evict down to the budget"""
        missing = [k for k in keys if k not in self._chunks]
        if missing and self._udev is not self._dev:
            self._dev.wait_for(self._udev)                        # a recycled buffer may still feed an earlier gather
        for k in keys:
            if k in self._chunks:
                self._chunks.move_to_end(k)
            else:
                # make room first: only what this call needs is held beyond the budget
                self._evict(set(keys) | self._pinned, len(self._chunks) + 1)
                self._chunks[k] = self._compute(*k)
        self._pinned = set(keys)
        self._evict(self._pinned, len(self._chunks))
        self._trim_heads(4 * HEAD_BLOCK if self._capacity() else 0)
        if missing and self._udev is not self._dev:
            self._udev.wait_for(self._dev)

    def _evict(self, keep, size):
        cap = self._capacity()
        for k in [k for k in self._chunks if k not in keep]:
            if size <= cap:
                break
            self._pool.append(self._chunks.pop(k))
            size -= 1

    def _release(self):
        """end of a request: nothing is pinned, the cache goes down to its budget, recycled buffers are freed"""
        self._pinned = set()
        self._evict(set(), len(self._chunks))
        self._eng.sync()
        for p in self._pool:
            self._dev.free(p)
        self._pool = []

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
        for p in self._pool:
            self._dev.free(p)
        self._pool = []
        if self._table is not None:
            self._dev.free(self._table.ptr)
            self._table = None

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

    @staticmethod
    def _out(out, shape, dtype):
        if out is None:
            return np.empty(shape, dtype)
        if tuple(out.shape) != shape or out.dtype != dtype:
            raise ValueError("out must be %s %s, got %s %s" % (np.dtype(dtype), shape, out.dtype, tuple(out.shape)))
        return out

    def heightmap(self, y0, x0, h, w, out=None, uint8=False):
        """pixels [y0, y0 + h) x [x0, x0 + w) of the heightmap: (C_a, h, w) float32, or with uint8=True
        util.to_uint8(util.convert_to_rgb(.)) as (h, w) for a greyscale generator, (h, w, 3) otherwise"""
        return self._request(y0, x0, h, w, True, False, out, None, uint8, False)[0]

    def texture(self, y0, x0, h, w, out=None, uint8=False):
        """the same pixels of the textured world: (C_out, h, w) float32, or with uint8=True the (h, w, 3) uint8 RGB"""
        return self._request(y0, x0, h, w, False, True, None, out, False, uint8)[1]

    def both(self, y0, x0, h, w, out_heightmap=None, out_texture=None, uint8=False):
        """(heightmap, texture) of one rectangle from one pass over the chunks; bit for bit the two separate calls"""
        return self._request(y0, x0, h, w, True, True, out_heightmap, out_texture, uint8, uint8)

    def scene(self, y0, x0, h, w, **kw):
        """the rectangle as a render.Scene with origin (y0, x0): ``both`` in float32, uploaded once.  Cameras are
        given in world coordinates.  kw: height_scale.  Close it, or use it as a context manager."""
        from .render import Scene
        hm, tex = self.both(y0, x0, h, w)
        return Scene(hm, tex, origin=(y0, x0), value_range=(self.model.is_a_grayscale, self.model.is_b_grayscale),
                     device=self.model.device, **kw)

    def view(self, camera, max_dist, height_scale=None, **kw):
        """one image of the world from ``camera`` (world coordinates, negative ones included), rays ``max_dist`` long: the
        scene of camera.footprint(max_dist), rendered.  kw: Scene.render's."""
        skw = {} if height_scale is None else {"height_scale": height_scale}
        with self.scene(*camera.footprint(max_dist), **skw) as scene:
            return scene.render(camera, max_dist=max_dist, **kw)

    def _request(self, y0, x0, h, w, want_hm, want_tex, out_hm, out_tex, hm_u8, tex_u8):
        from .device import PinnedArray
        y0, x0, h, w = self._check_region(y0, x0, h, w)
        geo, K, m = self._geo, self._K, self.model
        C = geo.channels
        if want_hm:
            if hm_u8 and C not in (1, 3):
                raise ValueError("uint8 output needs a 1- or 3-channel generator, this one has %d" % C)
            shape = ((h, w) if C == 1 else (h, w, 3)) if hm_u8 else (C, h, w)
            out_hm = self._out(out_hm, shape, np.uint8 if hm_u8 else np.float32)
        self._bind()
        eng, dev, ops, udev, uops = self._eng, self._dev, self._ops, self._udev, self._uops
        T, o, B = geo.out, self.overlap, self.batch_size
        st = T - o
        if want_tex:
            plan, prog = eng._infer_plan('p2p_gen', B, True)
            inp, u = plan.input_nodes[0].out, plan.out
            c_out = u.Cc
            if (inp.H, inp.W, u.H, u.W) != (T, T, T, T) or inp.Cc != C:
                raise ValueError("the pix2pix generator takes %d x %d x %d tiles, the heightmap generator makes %d x %d x %d"
                                 % (inp.Cc, inp.H, inp.W, C, T, T))
            if tex_u8 and c_out not in (1, 3):
                raise ValueError("uint8 output needs a 1- or 3-channel generator, this one has %d" % c_out)
            out_tex = self._out(out_tex, (h, w, 3) if tex_u8 else (c_out, h, w), np.uint8 if tex_u8 else np.float32)
        a_lo, a_hi = axis_chunks(y0, h, K)
        b_lo, b_hi = axis_chunks(x0, w, K)
        eng.sync()
        cp = type(dev)(dev.index)                # the copy stream: finished rows go down while the next chunks run
        devbufs, pins, events = [], [], []

        def alloc(d, n):
            devbufs.append((d, d.alloc(n)))
            return devbufs[-1][1]

        def pinned(n):
            pins.append(PinnedArray((n,), np.uint8))
            return pins[-1]

        def event(d):
            events.append(d.event_create())
            return events[-1]

        try:
            # ---- heightmap rows: one stage per chunk row ----
            if want_hm:
                hbpp = (1 if C == 1 else 3) if hm_u8 else 4 * C
                hrows = min(K, h)
                hstage = [alloc(dev, hrows * w * hbpp) for _ in range(2)]
                hpin = [pinned(hrows * w * hbpp) for _ in range(2)]
                hfin, hdown = [event(dev) for _ in range(2)], [event(cp) for _ in range(2)]
            hpending, hdone = [], []

            def hm_drain(item):
                slot, ya, yb = item
                dev.event_sync(hdown[slot])
                k = yb - ya
                a = hpin[slot].array[:k * w * hbpp]
                if not hm_u8:
                    out_hm[:, ya:yb, :] = a.view(np.float32).reshape(C, k, w)
                elif C == 1:
                    out_hm[ya:yb] = a.reshape(k, w)
                else:
                    out_hm[ya:yb] = a.reshape(k, w, 3)

            def hm_row(a):
                """the request's rows inside chunk row a (its chunks are resident) -> a stage -> the host"""
                slot = len(hdone) % 2
                ra, rb = max(y0, a * K), min(y0 + h, (a + 1) * K)
                if len(hdone) >= 2:
                    dev.event_wait(hdown[slot])              # the stage's previous download has left
                for b in range(b_lo, b_hi + 1):
                    ca, cb = max(x0, b * K), min(x0 + w, (b + 1) * K)
                    ops.world_crop(self._chunks[(a, b)], C, K, ra - a * K, ca - b * K, rb - ra, cb - ca, hm_u8,
                                   m.is_a_grayscale, hstage[slot], w, ca - x0)
                dev.event_record(hfin[slot])
                cp.event_wait(hfin[slot])
                cp.d2h_async(hpin[slot], hstage[slot], (rb - ra) * w * hbpp)
                cp.event_record(hdown[slot])
                hdone.append(a)
                hpending.append((slot, ra - y0, rb - y0))
                while len(hpending) > 1:
                    hm_drain(hpending.pop(0))

            if not want_tex:
                for a in range(a_lo, a_hi + 1):
                    self._acquire([(a, b) for b in range(b_lo, b_hi + 1)])
                    hm_row(a)
            else:
                # ---- texture: §4j's executor over world-anchored tiles, as the interior of a plan one tile larger ----
                p_lo, p_hi = axis_tiles(y0, h, T, o)
                q_lo, q_hi = axis_tiles(x0, w, T, o)
                ny, nx = p_hi - p_lo + 3, q_hi - q_lo + 3
                pad_y, pad_x = y0 - p_lo * st + st, x0 - q_lo * st + st
                Wp = (w + 3) // 4 * 4                         # whole 16-byte groups per accumulator row
                tb_lo, tb_hi = (q_lo * st) // K, (q_hi * st + T - 1) // K
                batches = slot_batches(q_lo, q_hi, B)
                tbpp = 3 if tex_u8 else 4 * c_out
                acc_bytes = c_out * T * Wp * 4
                acc = alloc(udev, acc_bytes)
                tstage = [alloc(udev, T * Wp * tbpp) for _ in range(2)]
                tpin = [pinned(T * Wp * tbpp) for _ in range(2)]
                tfin, tdown = [event(udev) for _ in range(2)], [event(cp) for _ in range(2)]
                udev.memset_zero(acc, acc_bytes)
                tpending, finals = [], 0

                def tex_drain(item):
                    slot, ya, yb = item
                    udev.event_sync(tdown[slot])
                    n = yb - ya
                    if tex_u8:
                        out_tex[ya:yb] = tpin[slot].array[:n * Wp * 3].reshape(n, Wp, 3)[:, :w]
                    else:
                        out_tex[:, ya:yb, :] = tpin[slot].array[:c_out * n * Wp * 4].view(np.float32) \
                            .reshape(c_out, n, Wp)[:, :, :w]

                for p in range(p_lo, p_hi + 1):
                    ty = p * st
                    ta_lo, ta_hi = ty // K, (ty + T - 1) // K
                    self._acquire([(a, b) for a in range(ta_lo, ta_hi + 1) for b in range(tb_lo, tb_hi + 1)])
                    if want_hm:
                        for a in range(max(ta_lo, a_lo), min(ta_hi, a_hi) + 1):
                            if a not in hdone:
                                hm_row(a)
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
                        slot = finals % 2
                        if finals >= 2:
                            udev.event_wait(tdown[slot])
                        uops.texture_finalize(acc, Wp, T, c_out, r_lo, r_hi - r_lo, yr, ny, pad_y, nx, pad_x, o, tex_u8,
                                              m.is_b_grayscale, tstage[slot])
                        udev.event_record(tfin[slot])
                        cp.event_wait(tfin[slot])
                        cp.d2h_async(tpin[slot], tstage[slot], (r_hi - r_lo) * Wp * tbpp)
                        cp.event_record(tdown[slot])
                        tpending.append((slot, yr + r_lo, yr + r_hi))
                        finals += 1
                    if not last:
                        row = Wp * 4
                        for c in range(c_out):
                            base = acc + c * T * row
                            if o:
                                udev.d2d(base, base + st * row, o * row)
                            udev.memset_zero(base + o * row, (T - o) * row)
                    while len(tpending) > 1:
                        tex_drain(tpending.pop(0))
                while tpending:
                    tex_drain(tpending.pop(0))
            while hpending:
                hm_drain(hpending.pop(0))
            eng.sync()
        finally:
            eng.sync()
            cp.sync()
            for e in events:
                dev.event_destroy(e)
            for p in pins:
                p.close()
            for d, p in devbufs:
                d.free(p)
            cp.close()
            self._release()
        return out_hm, out_tex


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
    # a region that starts with a negative number would read as an option: hand it over in the --region=... form
    argv = list(argv)
    for i, tok in enumerate(argv[:-1]):
        if tok == "--region" and re.match(r"\s*-\d", argv[i + 1]):
            argv[i:i + 2] = ["--region=" + argv[i + 1]]
            break
    a = p.parse_args(argv)
    if a.chunk_cells is not None and a.chunk_cells < 1:
        p.error("--chunk-cells must be >= 1")
    if not 1 <= a.batch_size <= MAX_BATCH:
        p.error("--batch-size must lie in [1, %d]" % MAX_BATCH)
    if a.overlap is not None and a.overlap < 0:
        p.error("--overlap must be >= 0")
    if a.texture is None and (a.overlap is not None or a.batch_size != 4):
        p.error("--overlap / --batch-size need --texture")
    return a


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    from . import util
    from .experiments import make_model
    from .terrain import _save_png
    model = make_model(a.experiment, dtype=a.dtype, verbose=False)
    model.load_model(a.model, mode='both' if a.texture else 'dcgan')
    y0, x0, h, w = a.region
    with model.terrain_world(a.seed, chunk_cells=a.chunk_cells, blend=a.blend, overlap=a.overlap,
                             batch_size=a.batch_size, verbose=True) as world:
        C = world.geometry.channels
        hm = np.lib.format.open_memmap(a.output, mode="w+", dtype=np.float32, shape=(C, h, w)) \
            if a.output.endswith(".npy") else None
        tex = None
        if a.texture:
            tex = np.lib.format.open_memmap(a.texture, mode="w+", dtype=np.uint8, shape=(h, w, 3)) \
                if a.texture.endswith(".npy") else None
            hm, tex = world._request(y0, x0, h, w, True, True, hm, tex, False, True)      # both(), fp32 + uint8
        else:
            hm = world.heightmap(y0, x0, h, w, out=hm)
    if a.output.endswith(".npy"):
        hm.flush()
    else:
        img = util.to_uint8(util.convert_to_rgb(hm, is_grayscale=model.is_a_grayscale))
        _save_png(a.output, img[:, :, 0] if C == 1 else img)
    if a.texture:
        if a.texture.endswith(".npy"):
            tex.flush()
        else:
            _save_png(a.texture, tex)
    model.device.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
