"""Heightmaps of any size from a grid of latent vectors.

After ``Dense -> BN -> Reshape(nch, s, s)`` the DCGAN generator is fully convolutional (stride-1 'same' convolutions, BN,
nonlinearities, x2 up-sampling).  A ``gy x gx`` grid of latent vectors goes through the head per cell,
``P[i, j] = head(z[i, j])`` of shape ``[nch, s, s]``, and the cells make one seed canvas ``S`` of ``nch x s gy x s gx``:
seed pixel (y, x) takes intra-cell position (y mod s, x mod s) from

  * ``mosaic``: cell (y // s, x // s) alone;
  * ``bilinear`` (default): the 2 x 2 nearest cells, cell coordinates u = (y + 0.5)/s - 0.5, v = (x + 0.5)/s - 0.5, corner
    indices clamped to the grid, corners that clamp onto one cell adding their weights (a 1-row / 1-column / 1 x 1 grid
    copies P exactly).  Dense is linear and deterministic BN per-unit affine, so this is the head run on a bilinearly
    interpolated latent field.

The trunk (the layers after the Reshape, re-rooted on an input of the canvas' shape, sharing the generator's Params) runs
over S as one image; zero 'same' padding applies only at the canvas border.  The output is ``[C_a, out gy, out gx]``.

Streaming: the trunk runs over windows of ``band + 2 halo`` seed rows of the full canvas width, ``halo`` being the trunk's
largest reach in seed rows (``trunk_halo``, from the graph itself); each window keeps the output rows at least ``halo`` seed
rows away from every window edge inside the canvas, and the kept ranges tile the canvas exactly once (``window_plan``).
Device memory is O(window), whatever the canvas height; outputs are written by rows only, so an ``open_memmap`` ``out``
takes maps larger than host RAM.

    python -m gan_heightmaps_amd.terrain EXPERIMENT MODEL OUT --cells GYxGX [--seed N] [--blend mosaic|bilinear]
        [--band N] [--dtype D] [--texture OUT_TEX [--overlap N] [--batch-size B]]
"""
import argparse
import re
import sys

import numpy as np

from . import layers as L
from . import util
from .architectures.layers import BilinearUpsample2DLayer
from .streaming import DownloadRing, check_uint8_channels, output_array, store_rows

_save_png = util.save_png          # (tools/render_bench.py imports the writer under this name)

__all__ = ["BLENDS", "WINDOW_BUDGET", "split_generator", "trunk_halo", "trunk_scale", "window_plan", "axis_blend",
           "TerrainGeometry", "generate_terrain", "parse_cells", "parse_args", "main"]

BLENDS = ('mosaic', 'bilinear')
# the default band keeps the largest trunk activation of one window under this many bytes (fp32): 4 GiB, i.e. 2^30 elements
WINDOW_BUDGET = 4 << 30
INT32_LIMIT = 1 << 31            # the kernels index within a sample in int32
HEAD_CHUNK = 1024                # cells per head forward pass


def split_generator(gen_out):
    """-> (head output layer, reshape layer, [trunk layers in order]) of a DCGAN generator ``... -> Reshape(-1, nch, s, s)
    -> trunk``.  NotImplementedError for a graph that is not a single chain through one such Reshape, or whose trunk holds
    anything but stride-1 'same' convolutions, BatchNorm, nonlinearities, dropout and x2 up-sampling (naming the layer)."""
    chain = L.get_all_layers(gen_out)
    for l in chain:
        if isinstance(l, L.MergeLayer):
            raise NotImplementedError("generate_terrain: the generator is not a single chain (%r)" % (l,))
    rs = [i for i, l in enumerate(chain) if isinstance(l, L.ReshapeLayer)]
    if len(rs) != 1 or len(chain[rs[0]].output_shape) != 4:
        raise NotImplementedError("generate_terrain: the generator needs exactly one Reshape to (-1, nch, s, s)")
    r = rs[0]
    shp = chain[r].output_shape
    if shp[2] != shp[3]:
        raise NotImplementedError("generate_terrain: the seed map is %d x %d, not square" % (shp[2], shp[3]))
    trunk = chain[r + 1:]
    for l in trunk:
        if isinstance(l, L.Conv2DLayer):
            k, p = l.filter_size, l.pad
            if l.stride != (1, 1) or k[0] != k[1] or 2 * p[0] != k[0] - 1:
                raise NotImplementedError("generate_terrain: %r is not a stride-1 'same' convolution" % (l,))
        elif isinstance(l, L.Upscale2DLayer):
            pass                                     # only x2 'repeat' exists
        elif isinstance(l, BilinearUpsample2DLayer):
            if l.factor != 2:
                raise NotImplementedError("generate_terrain: %r" % (l,))
        elif type(l) not in (L.BatchNormLayer, L.NonlinearityLayer, L.DropoutLayer):
            raise NotImplementedError("generate_terrain: the trunk layer %r has no windowed form" % (l,))
    return chain[r - 1], chain[r], trunk


def trunk_scale(trunk):
    """output pixels per seed pixel (2 per up-sampling layer)"""
    return 2 ** sum(isinstance(l, (L.Upscale2DLayer, BilinearUpsample2DLayer)) for l in trunk)


def trunk_halo(trunk):
    """the trunk's reach in whole seed rows: the largest distance, above or below, from a seed row to the seed rows its
    output rows depend on.  Row intervals are propagated backwards through the graph: a conv with filter k and pad p
    needs input rows [lo - p, hi + k - 1 - p]; nearest x2 [lo // 2, hi // 2]; bilinear x2 [lo // 2, (hi + 1) // 2]
    (fine row 2m reads coarse m, 2m + 1 reads m and m + 1)."""
    F = trunk_scale(trunk)
    y = 4 * len(trunk) + 8                           # any seed row far enough from the canvas edge: the rules are shift-free
    lo, hi = y * F, y * F + F - 1
    for l in reversed(trunk):
        if isinstance(l, L.Conv2DLayer):
            k, p = l.filter_size[0], l.pad[0]
            lo, hi = lo - p, hi + k - 1 - p
        elif isinstance(l, L.Upscale2DLayer):
            lo, hi = lo // 2, hi // 2
        elif isinstance(l, BilinearUpsample2DLayer):
            lo, hi = lo // 2, (hi + 1) // 2
    return max(y - lo, hi - y, 0)


def window_plan(H, band, halo):
    """[(w0, keep_lo, keep_hi)] in seed rows for a canvas of H seed rows: every window spans min(H, band + 2 halo) rows
    starting at w0 (clamped inside the canvas); it keeps rows [keep_lo, keep_hi), which lie at least ``halo`` rows from
    each of its edges that is not a canvas edge.  The kept ranges tile [0, H) exactly once."""
    if band < 1 or halo < 0 or H < 1:
        raise ValueError("window_plan: H=%r band=%r halo=%r" % (H, band, halo))
    win = min(H, band + 2 * halo)
    out, k = [], 0
    while k < H:
        w0 = max(0, min(k - halo, H - win))
        hi = H if w0 + win == H else w0 + win - halo
        out.append((w0, k, hi))
        k = hi
    return out


def axis_blend(n, s, bilinear):
    """per seed coordinate of an axis of n cells of s pixels: [(cell, weight)] in the kernel's order (float64)"""
    out = []
    for y in range(n * s):
        if not bilinear:
            out.append([(y // s, 1.0)])
            continue
        u = (y + 0.5) / s - 0.5
        i0 = int(np.floor(u))
        f = u - i0
        a, b = min(max(i0, 0), n - 1), min(max(i0 + 1, 0), n - 1)
        out.append([(a, 1.0)] if a == b else [(a, 1.0 - f), (b, f)])
    return out


class TerrainGeometry:
    """the sizes of one generate_terrain call: seed map s, channels, scale F, halo, band and the window height"""

    def __init__(self, gen_out, gy, gx, band=None):
        head, reshape, trunk = split_generator(gen_out)
        self.head, self.reshape, self.trunk = head, reshape, trunk
        _, self.nch, self.s, _ = reshape.output_shape
        self.gy, self.gx = int(gy), int(gx)
        self.F = trunk_scale(trunk)
        self.out = self.s * self.F
        self.halo = trunk_halo(trunk)
        self.Hs, self.Ws = self.s * self.gy, self.s * self.gx          # seed canvas
        self.H, self.W = self.out * self.gy, self.out * self.gx          # output canvas
        self.channels = trunk[-1].output_shape[1]
        # largest per-sample trunk tensor per seed row of the window (elements; the input included)
        per, f = self.nch * self.Ws, 1
        for l in trunk:
            if isinstance(l, (L.Upscale2DLayer, BilinearUpsample2DLayer)):
                f *= 2
            c = l.output_shape[1]
            per = max(per, c * f * f * self.Ws)
        self.per_row = per
        min_rows = min(self.Hs, 1 + 2 * self.halo)
        if min_rows * per >= INT32_LIMIT:
            widest = (INT32_LIMIT - 1) // (min_rows * (per // self.gx))
            raise ValueError("generate_terrain: a canvas %d cells (%d px) wide needs a trunk tensor of %d elements per "
                             "window, the kernels index up to 2^31; the widest canvas allowed is %d cells (%d px)"
                             % (self.gx, self.W, min_rows * per, widest, widest * self.out))
        if band is None:
            band = max(1, WINDOW_BUDGET // 4 // per - 2 * self.halo)
        elif isinstance(band, bool) or not isinstance(band, (int, np.integer)) or band < 1:
            raise ValueError("band must be a positive integer, got %r" % (band,))
        self.band = int(band)
        self.win = min(self.Hs, self.band + 2 * self.halo)
        if self.win * per >= INT32_LIMIT:
            raise ValueError("generate_terrain: band=%d makes a window tensor of %d elements; the kernels index up to 2^31"
                             % (self.band, self.win * per))
        self.windows = window_plan(self.Hs, self.band, self.halo)

    def trunk_graph(self):
        """the trunk re-rooted on a window of the seed canvas, sharing the generator's Params"""
        inp = L.InputLayer((None, self.nch, self.win, self.Ws))
        return L.clone_chain(self.trunk[-1], self.reshape, inp)


def _check_grid(grid, z, latent_dim):
    if z is not None:
        z = np.ascontiguousarray(z, np.float32)
        if z.ndim != 3 or z.shape[2] != latent_dim or z.shape[0] < 1 or z.shape[1] < 1:
            raise ValueError("z must be [gy, gx, %d], got %s" % (latent_dim, z.shape))
        if grid is not None and tuple(grid) != z.shape[:2]:
            raise ValueError("grid %r does not match z of shape %s" % (grid, z.shape))
        return z.shape[0], z.shape[1], z
    if grid is None:
        raise ValueError("give grid=(gy, gx) or z")
    gy, gx = grid
    if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1 for v in (gy, gx)):
        raise ValueError("grid must be two positive integers, got %r" % (grid,))
    return int(gy), int(gx), None


def generate_terrain(engine, gen_out, latent_dim, sampler, is_a_grayscale, grid=None, z=None, blend='bilinear', band=None,
                     out=None, uint8=False, deterministic=True):
    """A (out gy) x (out gx) heightmap from a grid of latent vectors with the DCGAN generator of ``engine`` (a GanStep).
    See Pix2Pix.generate_terrain."""
    from .step import LANE_OF
    if not deterministic:
        raise NotImplementedError("generate_terrain needs deterministic=True: with batch statistics a window's output would "
                                  "depend on which rows share its batch")
    if blend not in BLENDS:
        raise ValueError("blend must be one of %s, got %r" % (BLENDS, blend))
    gy, gx, z = _check_grid(grid, z, latent_dim)
    geo = TerrainGeometry(gen_out, gy, gx, band)
    C, H, W = geo.channels, geo.H, geo.W
    if uint8:
        check_uint8_channels(C)
        out = output_array(out, (H, W) if C == 1 else (H, W, 3), np.uint8)
    else:
        out = output_array(out, (C, H, W), np.float32)
    if z is None:
        z = np.asarray(sampler(gy * gx, latent_dim), np.float32).reshape(gy, gx, latent_dim)
    zf = np.ascontiguousarray(z.reshape(gy * gx, latent_dim), np.float32)

    key = 'dcgan_gen'
    lane = LANE_OF[key]
    dev, ops = engine.devs[lane], engine.ops[lane]
    n = gy * gx
    Bh = min(n, HEAD_CHUNK)
    hplan, hprog = engine._subgraph_plan(key, ('head',), Bh, lambda: geo.head)
    tplan, tprog = engine._subgraph_plan(key, ('trunk', geo.win, geo.Ws), 1, geo.trunk_graph)
    zin, hout = hplan.input_nodes[0].out, hplan.out
    inp, u = tplan.input_nodes[0].out, tplan.out
    assert u.shape == (1, C, geo.win * geo.F, W), (u.shape, geo.win, W)
    F, bpp = geo.F, (1 if C == 1 else 3) if uint8 else 4 * C
    stage_rows = geo.win * F
    engine.sync()
    P = dev.empty((n, geo.nch * geo.s * geo.s, 1, 1))
    cp = type(dev)(dev.index)                # the copy stream: finished rows go down while the next window runs
    down = None
    try:
        # the head, once for every cell: P stays resident
        for c0 in range(0, n, Bh):
            m = min(Bh, n - c0)
            zc = np.zeros((Bh, latent_dim), np.float32)
            zc[:m] = zf[c0:c0 + m]
            zin.set(zc)
            for e in hprog:
                e[1]()
            ops.copy_view(hout.samples(0, m), P.samples(c0, c0 + m))
        down = DownloadRing(dev, cp, stage_rows * W * bpp, lambda buf, ya, yb: store_rows(out, buf, ya, yb, W))
        for w0, klo, khi in geo.windows:
            ops.terrain_seed(P, gy, gx, geo.s, w0, geo.win, blend == 'bilinear', inp)
            for e in tprog:
                e[1]()
            r0, nr = (klo - w0) * F, (khi - klo) * F
            ops.terrain_emit(u, r0, nr, uint8, is_a_grayscale, down.stage())
            down.send(nr * W * bpp, klo * F, khi * F)
            down.poll()
        down.finish()
        engine.sync()
    finally:
        dev.sync()
        cp.sync()
        if down is not None:
            down.close()
        dev.free(P.ptr)
        cp.close()
    return out


def parse_cells(text):
    m = re.fullmatch(r"\s*(\d+)\s*[xX]\s*(\d+)\s*", text)
    if not m or int(m.group(1)) < 1 or int(m.group(2)) < 1:
        raise argparse.ArgumentTypeError("--cells wants GYxGX with two positive integers, got %r" % (text,))
    return int(m.group(1)), int(m.group(2))


def parse_args(argv):
    p = argparse.ArgumentParser(prog="python -m gan_heightmaps_amd.terrain",
                                description="Generate one seamless heightmap of GY x GX generator cells from a grid of "
                                            "latent vectors, and optionally texture it.")
    p.add_argument("experiment", help="experiment name (gan_heightmaps_amd.experiments), e.g. test1_nobn_bilin_both")
    p.add_argument("model", help="checkpoint written by save_model / save_checkpoint")
    p.add_argument("output", help="heightmap: .png (8-bit), or .npy (float32 (C, H, W), written through open_memmap)")
    p.add_argument("--cells", type=parse_cells, required=True, metavar="GYxGX", help="grid of latent vectors, e.g. 16x16")
    p.add_argument("--seed", type=int, default=None, help="seed of numpy's global RNG before the latent vectors are drawn")
    p.add_argument("--blend", default="bilinear", choices=list(BLENDS), help="how cells meet in the seed canvas")
    p.add_argument("--band", type=int, default=None, help="seed rows kept per window (default: the memory budget's)")
    p.add_argument("--dtype", default="bf16x3", choices=["f32", "bf16x3", "bf16x2", "bf16", "f16"],
                   help="arithmetic of the convolutions (default bf16x3)")
    p.add_argument("--texture", default=None, metavar="OUT_TEX",
                   help="also texture the heightmap with the pix2pix generator: .png, or .npy (uint8 (H, W, 3))")
    p.add_argument("--overlap", type=int, default=None, help="texture tile overlap in pixels (default in_shp / 4)")
    p.add_argument("--batch-size", type=int, default=4, help="texture tiles per forward pass (default 4)")
    a = p.parse_args(argv)
    if a.band is not None and a.band < 1:
        p.error("--band must be >= 1")
    if a.batch_size < 1:
        p.error("--batch-size must be >= 1")
    if a.overlap is not None and a.overlap < 0:
        p.error("--overlap must be >= 0")
    if a.texture is None and (a.overlap is not None or a.batch_size != 4):
        p.error("--overlap / --batch-size need --texture")
    return a


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    from .experiments import make_model
    model = make_model(a.experiment, dtype=a.dtype, verbose=False)
    model.load_model(a.model, mode='both' if a.texture else 'dcgan')
    gy, gx = a.cells
    geo = TerrainGeometry(model.dcgan['gen'], gy, gx, a.band)
    if a.seed is not None:
        np.random.seed(a.seed)
    shape = (geo.channels, geo.H, geo.W)
    hm = np.lib.format.open_memmap(a.output, mode="w+", dtype=np.float32, shape=shape) if a.output.endswith(".npy") \
        else None
    hm = model.generate_terrain(grid=(gy, gx), blend=a.blend, band=a.band, out=hm)
    if a.output.endswith(".npy"):
        hm.flush()
    else:
        img = util.to_uint8(util.convert_to_rgb(hm, is_grayscale=model.is_a_grayscale))
        util.save_png(a.output, img[:, :, 0] if geo.channels == 1 else img)
    if a.texture:
        tex = np.lib.format.open_memmap(a.texture, mode="w+", dtype=np.uint8, shape=(geo.H, geo.W, 3)) \
            if a.texture.endswith(".npy") else None
        tex = model.texture_heightmap(hm, overlap=a.overlap, batch_size=a.batch_size, out=tex, uint8=True)
        if a.texture.endswith(".npy"):
            tex.flush()
        else:
            util.save_png(a.texture, tex)
    model.device.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
