"""Host restatement of the unbounded world (gan_heightmaps_amd/world.py) in float64.

The contract's form: a region is the CROP of tests/terrain_ref.terrain over a block of cells with a margin (every kept pixel
at least ``halo + s/2`` seed pixels from the finite canvas' edge: margin_cells), with latents addressed by (i, j).  Beside it, for the tests
that hold the product's schedule to the contract: the unbounded seed canvas read directly (unclamped blends), one chunk from
its own window, and the world-anchored tile plan with its weights."""
import numpy as np

from gan_heightmaps_amd import terrain as TR
from tests import terrain_ref as R


def geometry(gen_out):
    return TR.TerrainGeometry(gen_out, 1, 1)


def latent_block(latent, i0, j0, ni, nj):
    """Z [ni, nj, latent_dim] (float64) of the cells [i0, i0 + ni) x [j0, j0 + nj); ``latent(i, j)`` -> [latent_dim]"""
    return np.stack([np.stack([np.asarray(latent(i0 + i, j0 + j), np.float64) for j in range(nj)]) for i in range(ni)])


def margin_cells(geo):
    """cells of margin around a region so that its pixels equal the unbounded world's: a finite canvas differs from the
    unbounded one in its zero padding (felt up to ``halo`` seed pixels in) AND in the seed pixels of its outer half cells,
    whose blend corners clamp (s/2 seed pixels, felt up to halo + s/2 in) -- so the margin is halo + s/2 seed pixels"""
    return -(-(geo.halo + geo.s // 2) // geo.s)


def covering_block(geo, y0, x0, h, w):
    """(i0, j0, ni, nj): the cells holding the pixels [y0, y0 + h) x [x0, x0 + w), plus the margin"""
    T, m = geo.out, margin_cells(geo)
    i0, i1 = y0 // T - m, (y0 + h - 1) // T + m
    j0, j1 = x0 // T - m, (x0 + w - 1) // T + m
    return i0, j0, i1 - i0 + 1, j1 - j0 + 1


def region(gen_out, latent, y0, x0, h, w, blend, dtype=np.float64):
    """Hm[:, y0:y0+h, x0:x0+w] of the unbounded world: the crop of the whole-canvas restatement over the covering block"""
    geo = geometry(gen_out)
    i0, j0, ni, nj = covering_block(geo, y0, x0, h, w)
    full = R.terrain(gen_out, latent_block(latent, i0, j0, ni, nj), blend, dtype)
    ya, xa = y0 - i0 * geo.out, x0 - j0 * geo.out
    return full[:, ya:ya + h, xa:xa + w]


# ---- the unbounded seed canvas, read directly ---------------------------------------------------------------------------
def axis_cover(y, s, bilinear):
    """[(cell, weight)] of seed coordinate y, any integer: no clamping, weights from y mod s alone"""
    if not bilinear:
        return [(y // s, 1.0)]
    u = (y % s + 0.5) / s - 0.5
    f = int(np.floor(u))
    return [(y // s + f, 1.0 - (u - f)), (y // s + f + 1, u - f)]


def seed_rect(head, y0, x0, rows, cols, s, blend):
    """S[:, y0:y0+rows, x0:x0+cols] of the unbounded seed canvas; ``head(i, j)`` -> [nch, s, s] (float64)"""
    bil = blend == 'bilinear'
    out = None
    for r in range(rows):
        for c in range(cols):
            y, x = y0 + r, x0 + c
            v = 0.0
            for i, wy in axis_cover(y, s, bil):
                for j, wx in axis_cover(x, s, bil):
                    v = v + wy * wx * head(i, j)[:, y % s, x % s]
            if out is None:
                out = np.zeros((v.shape[0], rows, cols))
            out[:, r, c] = v
    return out


def head_fn(gen_out, latent):
    """memoised head(i, j) -> [nch, s, s] in float64"""
    memo = {}

    def head(i, j):
        if (i, j) not in memo:
            memo[(i, j)] = R.head_maps(gen_out, np.asarray(latent(i, j), np.float64)[None, None])[0, 0]
        return memo[(i, j)]
    return head


def chunk(gen_out, latent, a, b, chunk_cells, blend):
    """chunk (a, b) the product's way: ONE trunk pass over its own seed window, the centre K x K kept"""
    geo = geometry(gen_out)
    c, s, halo, F = chunk_cells, geo.s, geo.halo, geo.F
    win = c * s + 2 * halo
    S = seed_rect(head_fn(gen_out, latent), a * c * s - halo, b * c * s - halo, win, win, s, blend)
    u = R.trunk(gen_out, S)
    K = c * geo.out
    return u[:, halo * F:halo * F + K, halo * F:halo * F + K]


def assemble(gen_out, latent, y0, x0, h, w, chunk_cells, blend):
    """a request assembled from the chunks it touches (world.axis_chunks), each from its own window"""
    from gan_heightmaps_amd import world as WD
    K = chunk_cells * geometry(gen_out).out
    (a0, a1), (b0, b1) = WD.axis_chunks(y0, h, K), WD.axis_chunks(x0, w, K)
    rows = [np.concatenate([chunk(gen_out, latent, a, b, chunk_cells, blend) for b in range(b0, b1 + 1)], axis=2)
            for a in range(a0, a1 + 1)]
    full = np.concatenate(rows, axis=1)
    return full[:, y0 - a0 * K:y0 - a0 * K + h, x0 - b0 * K:x0 - b0 * K + w]


# ---- world-anchored tiles -----------------------------------------------------------------------------------------------
def tile_weights(T, o):
    """float64 [T]: every tile ramps on both sides (float32 evaluation of the ramps, as the kernels')"""
    w = np.ones(T, np.float32)
    if o > 0:
        t = np.arange(T)
        w[:o] = (t[:o].astype(np.float32) + np.float32(0.5)) / np.float32(o)
        w[T - o:] = ((T - t[T - o:]).astype(np.float32) - np.float32(0.5)) / np.float32(o)
    return w.astype(np.float64)


def covering_tiles(y, T, o):
    """indices of the world-anchored tiles [p st, p st + T) that cover coordinate y, in order"""
    st = T - o
    return [p for p in range((y - T) // st + 1, y // st + 1) if p * st <= y < p * st + T]


def texture_region(hm, unet, y0, x0, h, w, T, o):
    """Tex[:, y0:y0+h, x0:x0+w] = sum(w U(tile)) / sum(w) over the anchored tiles in row-major order.
    ``hm(y0, x0, h, w)`` -> (C, h, w) of the world's heightmap; ``unet(tile [C, T, T])`` -> [C', T, T]"""
    st = T - o
    wt = tile_weights(T, o)
    p_lo, p_hi = (y0 - T) // st + 1, (y0 + h - 1) // st
    q_lo, q_hi = (x0 - T) // st + 1, (x0 + w - 1) // st
    num, den = None, np.zeros((h, w))
    for p in range(p_lo, p_hi + 1):
        for q in range(q_lo, q_hi + 1):
            u = np.asarray(unet(hm(p * st, q * st, T, T)), np.float64)
            if num is None:
                num = np.zeros((u.shape[0], h, w))
            ya, yb = max(y0, p * st), min(y0 + h, p * st + T)
            xa, xb = max(x0, q * st), min(x0 + w, q * st + T)
            wy, wx = wt[ya - p * st:yb - p * st], wt[xa - q * st:xb - q * st]
            ww = wy[:, None] * wx[None, :]
            num[:, ya - y0:yb - y0, xa - x0:xb - x0] += ww * u[:, ya - p * st:yb - p * st, xa - q * st:xb - q * st]
            den[ya - y0:yb - y0, xa - x0:xb - x0] += ww
    return num / den, den


def tile_aligned_expansion(y0, x0, h, w, T, o):
    """E = (ey, ex, eh, ew): the tile-aligned rectangle [p0 st, p1 st + T) x [q0 st, q1 st + T) that holds the request at
    least ``o`` pixels inside its border"""
    st = T - o
    p0, p1 = (y0 - o) // st, -(-(y0 + h + o - T) // st)
    q0, q1 = (x0 - o) // st, -(-(x0 + w + o - T) // st)
    p1, q1 = max(p1, p0), max(q1, q0)
    return p0 * st, q0 * st, (p1 - p0) * st + T, (q1 - q0) * st + T
