"""Texture heightmaps of any size: tiled U-Net inference with overlapping, cross-faded tiles.

``gen_fn`` / ``gen_fn_det`` take exactly one ``in_shp x in_shp`` crop.  A larger map is cut into tiles of that size that
overlap by ``o`` pixels; every tile goes through the forward plan ``gen_fn_det`` uses, and each pixel is the weighted mean
of the tiles that cover it, with separable linear ramps across the overlaps, so seams cross-fade instead of showing.

Per axis of length ``L`` (``T = in_shp``, ``0 <= o <= T/2``, stride ``s = T - o``):
    n = 1 + ceil(max(L - T, 0) / s) tiles, padded length L' = T + (n - 1) s, pad_before = (L' - L) // 2,
    tile i covers canvas coordinates [-pad_before + i s, -pad_before + i s + T).
Canvas coordinates outside [0, L) read the input through ghm_image_batch's half-sample-symmetric 'reflect' rule.  Tile i
weighs tile-local coordinate t with (t + 0.5)/o for t < o if i > 0, (T - t - 0.5)/o for t >= T - o if i < n - 1, and 1
elsewhere; a 2-D tile weighs w_y w_x.  Output = sum(w u) / sum(w), the terms summed in tile order (row-major).  A pixel that
one tile covers comes out as that tile's value exactly; o = 0 is plain cropping.

Tile batches hold consecutive tiles of ONE tile row, ``batch_size`` at a time; a ragged last batch repeats its last tile
(the repeats' outputs are discarded).

The executor streams the canvas tile row by tile row: device memory is O(in_shp x W) whatever H is, and inputs / outputs
are only sliced by rows, so ``np.memmap`` / ``open_memmap`` / HDF5 datasets larger than host RAM pass through.

    python -m gan_heightmaps_amd.texture EXPERIMENT MODEL IN OUT [--overlap N] [--batch-size B] [--dtype D]
"""
import argparse
import sys

import numpy as np

from .streaming import DownloadRing, check_uint8_channels, output_array, shift_accumulator, store_rows
from .util import read_image, save_png

__all__ = ["AxisPlan", "axis_plan", "axis_weights", "reflect_index", "tile_batches", "check_overlap", "texture_heightmap",
           "parse_args", "main"]


def check_overlap(T, overlap=None):
    """-> the overlap to use for tile size T (default T // 4); ValueError unless 0 <= overlap <= T / 2"""
    if isinstance(T, bool) or not isinstance(T, (int, np.integer)) or T < 1:
        raise ValueError("tile size must be a positive integer, got %r" % (T,))
    if overlap is None:
        return int(T) // 4
    if isinstance(overlap, bool) or not isinstance(overlap, (int, np.integer)):
        raise ValueError("overlap must be an integer, got %r" % (overlap,))
    if overlap < 0 or 2 * overlap > T:
        raise ValueError("overlap must lie in [0, %d] for tile size %d, got %d" % (T // 2, T, overlap))
    return int(overlap)


class AxisPlan:
    """the tiles of one axis: ``n`` tiles of size ``T`` at stride ``s``, tile i starting at ``start(i)``"""
    __slots__ = ("L", "T", "o", "s", "n", "padded", "pad")

    def __init__(self, L, T, o):
        self.L, self.T, self.o, self.s = L, T, o, T - o
        self.n = 1 + -(-max(L - T, 0) // self.s)
        self.padded = T + (self.n - 1) * self.s
        self.pad = (self.padded - L) // 2

    def start(self, i):
        return -self.pad + i * self.s

    @property
    def starts(self):
        return [self.start(i) for i in range(self.n)]

    def covering(self, y):
        """indices of the tiles covering canvas coordinate y, in tile order"""
        return [i for i in range(max(0, (y + self.pad - self.T) // self.s), self.n)
                if self.start(i) <= y < self.start(i) + self.T]

    def __repr__(self):
        return "AxisPlan(L=%d, T=%d, o=%d, n=%d, pad=%d)" % (self.L, self.T, self.o, self.n, self.pad)


def axis_plan(L, T, overlap=None):
    """the tiling of an axis of length L >= 1 by tiles of size T with the given overlap (ValueError if invalid)"""
    o = check_overlap(T, overlap)
    if isinstance(L, bool) or not isinstance(L, (int, np.integer)) or L < 1:
        raise ValueError("axis length must be a positive integer, got %r" % (L,))
    return AxisPlan(int(L), int(T), o)


def axis_weights(plan, i):
    """float32 [T]: the weights of tile i along its axis, evaluated as the kernels do (float32, correctly rounded)"""
    T, o = plan.T, plan.o
    w = np.ones(T, np.float32)
    if o > 0:
        t = np.arange(T)
        if i > 0:
            w[:o] = (t[:o].astype(np.float32) + np.float32(0.5)) / np.float32(o)
        if i < plan.n - 1:
            w[T - o:] = ((T - t[T - o:]).astype(np.float32) - np.float32(0.5)) / np.float32(o)
    return w


def reflect_index(c, L):
    """ghm_image_batch's 'reflect' border rule on integer coordinates (half-sample symmetric, period 2L)"""
    c = np.asarray(c, np.int64)
    if L <= 1:
        return np.zeros_like(c)
    m = np.mod(c, 2 * L)
    return np.where(m >= L, 2 * L - 1 - m, m)


def tile_batches(n, batch_size):
    """the forward batches of one tile row of n tiles: [(first tile, number of real tiles)]; each batch is padded to
    ``batch_size`` by repeating its last tile"""
    if batch_size < 1:
        raise ValueError("batch_size must be >= 1")
    return [(j0, min(batch_size, n - j0)) for j0 in range(0, n, batch_size)]


def _input_layout(heightmap, channels):
    """-> (H, W, is_uint8) of a (H, W) / (H, W, C) uint8 or (C, H, W) float32 heightmap"""
    a = heightmap
    if a.dtype == np.uint8 and a.ndim in (2, 3):
        H, W = a.shape[:2]
        c = 1 if a.ndim == 2 else a.shape[2]
        u8 = True
    elif a.dtype == np.float32 and a.ndim == 3:
        c, H, W = a.shape
        u8 = False
    else:
        raise ValueError("heightmap must be (H, W) / (H, W, C) uint8 or (C, H, W) float32, got %s %s"
                         % (a.dtype, a.shape))
    if c != channels:
        raise ValueError("the generator takes %d input channel(s), the heightmap has %d" % (channels, c))
    if H < 1 or W < 1 or H >= 2 ** 31 or W >= 2 ** 24:
        raise ValueError("heightmap size %d x %d out of range" % (H, W))
    return H, W, u8


class _Tiler:
    """the device and page-locked buffers of one texture_heightmap call (all O(T W), none depends on H): the input bands, the
    accumulator, and the download ring (``down``) that stores finished rows into ``out``"""

    def __init__(self, dev, W, T, c_in, c_out, u8_in, u8_out, out):
        from .device import PinnedArray
        mkpin = getattr(type(dev), 'pinned_array', PinnedArray)
        self.dev = dev
        self.cp = type(dev)(dev.index)         # the copy stream: uploads and downloads overlap the tile rows
        self.band_bytes = c_in * T * W * (1 if u8_in else 4)
        self.acc_bytes = c_out * T * W * 4
        self.band = [dev.alloc(self.band_bytes) for _ in range(2)]
        self.acc = dev.alloc(self.acc_bytes)
        self.down = DownloadRing(dev, self.cp, T * W * (3 if u8_out else 4 * c_out),
                                 lambda buf, ya, yb: store_rows(out, buf, ya, yb, W))
        self.pin_in = [mkpin((self.band_bytes,), np.uint8) for _ in range(2)]
        self.ev_land = [self.cp.event_create() for _ in range(2)]     # band upload landed (copy stream)
        self.ev_used = [dev.event_create() for _ in range(2)]         # last gather of a band (compute stream)

    def close(self):
        self.dev.sync()
        self.cp.sync()
        for e in self.ev_land + self.ev_used:
            self.dev.event_destroy(e)
        for p in self.pin_in:
            p.close()
        for p in self.band + [self.acc]:
            self.dev.free(p)
        self.down.close()
        self.cp.close()


def texture_heightmap(engine, heightmap, is_a_grayscale, is_b_grayscale, overlap=None, batch_size=4, out=None,
                      uint8=False, deterministic=True):
    """Texture a heightmap of any size with the p2p generator of ``engine`` (a GanStep).  See Pix2Pix.texture_heightmap."""
    from .step import LANE_OF
    if not deterministic:
        raise NotImplementedError("texture_heightmap needs deterministic=True: with batch statistics a tile's texture "
                                  "would depend on which tiles share its batch")
    if isinstance(batch_size, bool) or not isinstance(batch_size, (int, np.integer)) or batch_size < 1:
        raise ValueError("batch_size must be a positive integer, got %r" % (batch_size,))
    lane = LANE_OF['p2p_gen']
    dev, ops = engine.devs[lane], engine.ops[lane]
    plan, prog = engine._infer_plan('p2p_gen', int(batch_size), True)
    inp, u = plan.input_nodes[0].out, plan.out
    T, c_in, c_out = inp.H, inp.Cc, u.Cc
    assert inp.W == T and u.H == T and u.W == T
    o = check_overlap(T, overlap)
    heightmap = heightmap if hasattr(heightmap, 'dtype') else np.asarray(heightmap)
    H, W, u8_in = _input_layout(heightmap, c_in)
    py, px = axis_plan(H, T, o), axis_plan(W, T, o)
    if uint8:
        check_uint8_channels(c_out)
    out = output_array(out, *(((H, W, 3), np.uint8) if uint8 else ((c_out, H, W), np.float32)))
    s, ny, nx = T - o, py.n, px.n
    batches = tile_batches(nx, int(batch_size))
    engine.sync()
    tl = _Tiler(dev, W, T, c_in, c_out, u8_in, uint8, out)
    try:
        dev.memset_zero(tl.acc, tl.acc_bytes)
        def upload(iy, slot):
            rows = reflect_index(np.arange(py.start(iy), py.start(iy) + T), H)
            lo, hi = int(rows.min()), int(rows.max()) + 1
            if u8_in:
                src = np.asarray(heightmap[lo:hi]).reshape(hi - lo, W * c_in)
                nbytes = src.size
                tl.pin_in[slot].array[:nbytes].reshape(hi - lo, W * c_in)[...] = src
            else:
                nbytes = c_in * (hi - lo) * W * 4
                tl.pin_in[slot].array[:nbytes].view(np.float32).reshape(c_in, hi - lo, W)[...] = heightmap[:, lo:hi, :]
            tl.cp.h2d_async(tl.band[slot], tl.pin_in[slot], nbytes)
            tl.cp.event_record(tl.ev_land[slot])
            return lo, hi - lo

        bands = [upload(0, 0), None]
        used = [False, False]
        for iy in range(ny):
            slot, y0 = iy % 2, py.start(iy)
            band_row0, band_rows = bands[slot]
            dev.event_wait(tl.ev_land[slot])
            for j0, nv in batches:
                ops.texture_gather(tl.band[slot], u8_in, c_in, band_rows, band_row0, H, W, y0, px.start(j0), s, nv,
                                   not is_a_grayscale, inp)
                for e in prog:
                    e[1]()
                ops.texture_blend(tl.acc, W, T, c_out, u, nv, iy, ny, j0, nx, px.pad, o)
            dev.event_record(tl.ev_used[slot])
            used[slot] = True
            # rows no later tile row touches: the first s of the band (all of it for the last tile row), inside the canvas
            last = iy == ny - 1
            r_lo, r_hi = max(0, -y0), min(T if last else s, H - y0)
            if r_hi > r_lo:
                ops.texture_finalize(tl.acc, W, T, c_out, r_lo, r_hi - r_lo, y0, ny, py.pad, nx, px.pad, o, uint8,
                                     is_b_grayscale, tl.down.stage())
                tl.down.send((r_hi - r_lo) * W * (3 if uint8 else 4 * c_out), y0 + r_lo, y0 + r_hi)
            if not last:
                shift_accumulator(dev, tl.acc, c_out, T, W * 4, o)
                nslot = (iy + 1) % 2
                if used[nslot]:
                    tl.cp.event_wait(tl.ev_used[nslot])        # the band's previous tile row has gathered from it
                    dev.event_sync(tl.ev_land[nslot])          # and its page-locked source may be refilled
                bands[nslot] = upload(iy + 1, nslot)
            tl.down.poll()             # here, behind the shift and the next upload: the host blocks with work enqueued
        tl.down.finish()
        engine.sync()
    finally:
        tl.close()
    return out


def parse_args(argv):
    p = argparse.ArgumentParser(prog="python -m gan_heightmaps_amd.texture",
                                description="Texture a heightmap of any size with a trained pix2pix generator "
                                            "(overlapping, cross-faded in_shp x in_shp tiles).")
    p.add_argument("experiment", help="experiment name (gan_heightmaps_amd.experiments), e.g. test1_nobn_bilin_both")
    p.add_argument("model", help="checkpoint written by save_model / save_checkpoint (its p2p nets are loaded)")
    p.add_argument("input", help="heightmap: 8-bit PNG, or .npy (uint8 (H, W) / (H, W, C), read through mmap)")
    p.add_argument("output", help="texture: .png, or .npy (uint8 (H, W, 3), written through open_memmap)")
    p.add_argument("--overlap", type=int, default=None, help="tile overlap in pixels (default in_shp / 4)")
    p.add_argument("--batch-size", type=int, default=4, help="tiles per forward pass (default 4)")
    p.add_argument("--dtype", default="bf16x3", choices=["f32", "bf16x3", "bf16x2", "bf16", "f16"],
                   help="arithmetic of the generator's convolutions (default bf16x3)")
    a = p.parse_args(argv)
    if a.batch_size < 1:
        p.error("--batch-size must be >= 1")
    if a.overlap is not None and a.overlap < 0:
        p.error("--overlap must be >= 0")
    return a


def read_heightmap(path, channels):
    """PNG through PIL as grey or RGB, or .npy through mmap"""
    return read_image(path, "L" if channels == 1 else "RGB")


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    from .experiments import make_model
    model = make_model(a.experiment, dtype=a.dtype, verbose=False)
    model.load_model(a.model, mode='p2p')
    c_in = 1 if model.is_a_grayscale else 3
    x = read_heightmap(a.input, c_in)
    if x.ndim == 3 and c_in == 1 and x.shape[2] == 1:
        x = x[:, :, 0]
    H, W = x.shape[:2]
    out = None
    if a.output.endswith(".npy"):
        out = np.lib.format.open_memmap(a.output, mode="w+", dtype=np.uint8, shape=(H, W, 3))
    tex = model.texture_heightmap(x, overlap=a.overlap, batch_size=a.batch_size, out=out, uint8=True)
    if out is not None:
        out.flush()
    else:
        save_png(a.output, tex)
    model.device.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
