"""Host restatement of terrain generation (gan_heightmaps_amd/terrain.py) in float64 on the oracle's ops: the
generator head per cell, the seed canvas in both blends, and the trunk over a whole canvas or over the windows of a band
plan (the executor's schedule, to hold the halo to the whole-canvas result)."""
import numpy as np

from oracle import tape as TP
from gan_heightmaps_amd import layers as L
from gan_heightmaps_amd import terrain as TR
from gan_heightmaps_amd.architectures.layers import BilinearUpsample2DLayer


def _v(p, dtype):
    return np.asarray(p.get_value(), dtype)


def _run(layers, x, dtype):
    """interpret a chain of layers (deterministic: BN on running statistics, dropout the identity) on x"""
    node = TP.leaf(np.asarray(x, dtype))
    for l in layers:
        if isinstance(l, L.DenseLayer):
            node = TP.act(TP.dense(node, TP.leaf(_v(l.W, dtype)), TP.leaf(_v(l.b, dtype))), l.nonlinearity.kind,
                          l.nonlinearity.alpha)
        elif isinstance(l, L.Conv2DLayer):
            node = TP.act(TP.conv2d(node, TP.leaf(_v(l.W, dtype)), TP.leaf(_v(l.b, dtype)), 1, l.pad[0]),
                          l.nonlinearity.kind, l.nonlinearity.alpha)
        elif isinstance(l, L.BatchNormLayer):
            node = TP.bn_infer(node, TP.leaf(_v(l.beta, dtype)), TP.leaf(_v(l.gamma, dtype)), _v(l.mean, dtype),
                               _v(l.inv_std, dtype))
        elif isinstance(l, L.NonlinearityLayer):
            node = TP.act(node, l.nonlinearity.kind, l.nonlinearity.alpha)
        elif isinstance(l, L.DropoutLayer):
            pass
        elif isinstance(l, L.Upscale2DLayer):
            node = TP.upscale_nearest(node, 2)
        elif isinstance(l, BilinearUpsample2DLayer):
            node = TP.bilinear_up2(node)
        elif isinstance(l, L.ReshapeLayer):
            node = TP.reshape(node, (-1,) + tuple(l.shape[1:]))
        else:
            raise NotImplementedError(repr(l))
    return node.v


def head_maps(gen_out, z, dtype=np.float64):
    """P [gy, gx, nch, s, s] of z [gy, gx, latent]"""
    head, reshape, _ = TR.split_generator(gen_out)
    gy, gx, d = z.shape
    chain = [l for l in L.get_all_layers(head) if not isinstance(l, L.InputLayer)] + [reshape]
    P = _run(chain, z.reshape(gy * gx, d), dtype)
    return P.reshape((gy, gx) + P.shape[1:])


def seed_canvas(P, blend):
    """S [nch, s gy, s gx] of P [gy, gx, nch, s, s] with the contract's blend weights (terrain.axis_blend)"""
    gy, gx, C, s, _ = P.shape
    by, bx = TR.axis_blend(gy, s, blend == 'bilinear'), TR.axis_blend(gx, s, blend == 'bilinear')
    S = np.zeros((C, s * gy, s * gx), P.dtype)
    for y in range(s * gy):
        for x in range(s * gx):
            for i, wy in by[y]:
                for j, wx in bx[x]:
                    S[:, y, x] += wy * wx * P[i, j, :, y % s, x % s]
    return S


def trunk(gen_out, S, dtype=np.float64):
    """the trunk over a canvas S [nch, h, w] as one image -> [C_a, h F, w F]"""
    _, _, layers = TR.split_generator(gen_out)
    return _run(layers, S[None], dtype)[0]


def trunk_banded(gen_out, S, band, halo=None):
    """the trunk over the windows of window_plan(S rows, band, halo), each window's kept rows pasted into the result"""
    _, _, layers = TR.split_generator(gen_out)
    halo = TR.trunk_halo(layers) if halo is None else halo
    F = TR.trunk_scale(layers)
    Hs = S.shape[1]
    win = min(Hs, band + 2 * halo)
    out = None
    for w0, klo, khi in TR.window_plan(Hs, band, halo):
        u = trunk(gen_out, S[:, w0:w0 + win])
        if out is None:
            out = np.zeros((u.shape[0], Hs * F, u.shape[2]), u.dtype)
        out[:, klo * F:khi * F] = u[:, (klo - w0) * F:(khi - w0) * F]
    return out


def terrain(gen_out, z, blend, dtype=np.float64):
    """the whole map in one piece: trunk(seed_canvas(head_maps(z)))"""
    return trunk(gen_out, seed_canvas(head_maps(gen_out, z, dtype), blend), dtype)
