"""BASELINE.json sizes (512x512): parity through size-independent properties and sampled exact checks.

  * sampled-output parity of the heaviest layer geometries (forward, data gradient, weight gradient): a few
    hundred output elements of each are recomputed in float64 straight from the definition,
  * one FULL-SIZE joint train step of test1_nobn_bilin_both at batch 2 against the numpy oracle (the oracle
    needs ~30-60 s for it on the GPU box's host cores),
  * determinism and batching properties of the full-size batch-4 step."""
import zlib

import numpy as np
import pytest

from oracle import step as ostep
from tests import canary

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30)


gpu = canary.fixtures()[0]


HEAVY = [
    # name,            N, C,   H,   W,   K,  k, s, pad     (geometries of SURVEY.md 2.2 at the step's batch sizes)
    ("d_conv2",        8, 64,  256, 256, 128, 5, 1, 2),
    ("d_conv3",        8, 128, 128, 128, 128, 5, 1, 2),
    ("g_conv7",        4, 64,  256, 256, 64,  5, 1, 2),
    ("dconv8",         4, 256, 256, 256, 64,  3, 1, 1),
    ("dconv6",         4, 1024, 64, 64,  256, 3, 1, 1),
    ("pd_conv2",       8, 64,  256, 256, 128, 3, 2, 1),
    ("g_out",          4, 64,  512, 512, 1,   5, 1, 2),
    ("d_conv1",        8, 1,   512, 512, 64,  5, 1, 2),
]


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("case", HEAVY, ids=[c[0] for c in HEAVY])
def test_sampled_parity_at_full_size(gpu, case, dtype):
    """dtype f32: the fp32 kernels (<= 1e-5).  bf16 / f16 (BASELINE configs 4 / 5): the matrix-core kernels of
    csrc/conv_lp.hip wherever they serve the geometry, against the definition evaluated on operands rounded to
    bf16 / fp16 (exact given the rounding: <= 2e-5) -- the thin first / last layers are not served and stay fp32."""
    from oracle import lp as LP
    dev, ops, D = gpu
    _, N, C, H, W, K, k, s, pad = case
    if dtype != "f32":
        dchk = D.conv_desc(N, C, H, W, K, k, k, s, pad)
        served = [ops.lp_supported(dchk, kind, dtype) for kind in (0, 1, 2)]
        assert all(served) == (min(C, K) >= 32), (case[0], served)
        if not all(served):
            assert not any(served)
            pytest.skip("%s is a thin layer: fp32 kernels in every arithmetic mode" % case[0])
    rng = np.random.RandomState(zlib.crc32(case[0].encode()) & 0x7fffffff)     # stable across processes (str hashes are salted)
    x = rng.randn(N, C, H, W).astype(np.float32)
    Wt = (rng.randn(K, C, k, k) / np.sqrt(C * k * k)).astype(np.float32)
    b = rng.randn(K).astype(np.float32)
    d = D.conv_desc(N, C, H, W, K, k, k, s, pad)
    Ho, Wo = d.Ho, d.Wo
    dy = rng.randn(N, K, Ho, Wo).astype(np.float32)
    xd, wd, bd, dyd = dev.tensor(x), dev.tensor(D.pack_conv_w(Wt).ravel()), dev.tensor(b), dev.tensor(dy)
    yd, dxd = dev.empty((N, K, Ho, Wo)), dev.empty(x.shape)
    dwd = dev.zeros((1, C * k * k * K, 1, 1))
    ws = dev.alloc(max(ops.wgrad_workspace(d), ops.wgrad_lp_workspace(d)))
    if dtype != "f32":
        wq, wqT = dev.alloc(ops.lp_weight_bytes(d, False)), dev.alloc(ops.lp_weight_bytes(d, True))
        ops.lp_pack_weights(d, wd, wq, dtype, False)
        ops.lp_pack_weights(d, wd, wqT, dtype, True)
        ops.conv2d_fwd_lp(d, xd, wq, bd, yd, dtype)
        ops.conv2d_dgrad_lp(d, dyd, wqT, dxd, dtype)
        ops.conv2d_wgrad_lp(d, xd, dyd, dwd, ws, dtype)
        dev.free(wq)
        dev.free(wqT)
        x, Wt, dy = LP.ROUND[dtype](x), LP.ROUND[dtype](Wt), LP.ROUND[dtype](dy)      # the reference's operands
    elif s == 1 and C > 4:
        wT = dev.empty((1, C * k * k * K, 1, 1))
        ops.transpose_weights(d, wd, wT)
        ops.conv2d_dgrad_t(d, dyd, wT, dxd)
    else:
        ops.conv2d_dgrad(d, dyd, wd, dxd)
    if dtype == "f32":
        ops.conv2d_fwd(d, xd, wd, bd, yd)
        ops.conv2d_wgrad(d, xd, dyd, dwd, ws)
    y, dx = yd.numpy(), dxd.numpy()
    dW = D.unpack_conv_w(dwd.numpy().ravel(), K, C, k, k)
    x64, W64, dy64 = x.astype(np.float64), Wt.astype(np.float64), dy.astype(np.float64)
    xp = np.pad(x64, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    Wf = W64[:, :, ::-1, ::-1]                              # true convolution == correlation with the flipped filter
    got, ref = [], []
    for _ in range(200):                                    # forward samples (incl. image borders)
        n, co = rng.randint(N), rng.randint(K)
        i = rng.choice([0, Ho - 1, rng.randint(Ho)])
        j = rng.choice([0, Wo - 1, rng.randint(Wo)])
        ref.append(b[co] + (xp[n, :, i * s:i * s + k, j * s:j * s + k] * Wf[co]).sum())
        got.append(y[n, co, i, j])
    tol = 1e-5 if dtype == "f32" else 2e-5
    assert rel(got, ref) < tol
    dyp = dy64
    got, ref = [], []
    for _ in range(100):                                    # data-gradient samples
        n, c = rng.randint(N), rng.randint(C)
        u = rng.choice([0, H - 1, rng.randint(H)])
        v = rng.choice([0, W - 1, rng.randint(W)])
        acc = 0.0
        for a in range(k):
            for bb in range(k):
                ii, jj = u + pad - a, v + pad - bb
                if ii % s or jj % s:
                    continue
                ii, jj = ii // s, jj // s
                if 0 <= ii < Ho and 0 <= jj < Wo:
                    acc += (dyp[n, :, ii, jj] * Wf[:, c, a, bb]).sum()
        ref.append(acc)
        got.append(dx[n, c, u, v])
    assert rel(got, ref) < tol
    got, ref = [], []
    for _ in range(24):                                     # weight-gradient samples (full pixel reduction each)
        co, c, a, bb = rng.randint(K), rng.randint(C), rng.randint(k), rng.randint(k)
        win = xp[:, c, a:a + s * Ho:s, bb:bb + s * Wo:s]
        ref.append((win * dy64[:, co]).sum())
        got.append(dW[co, c, k - 1 - a, k - 1 - bb])         # dW is in lasagne (flipped) layout
    assert rel(got, ref) < 2e-5
    for t in (xd, wd, bd, dyd, yd, dxd, dwd):
        dev.free(t.ptr)
    dev.free(ws)


@pytest.fixture(scope="module")
def batch2_oracle():
    """one joint train step of the real 512x512 nets at batch 2 on the oracle: exact arithmetic (float64) and the float32 run of
    the same oracle -- how far ANY float32 implementation (the reference runs floatX=float32) sits from exact arithmetic on
    these nets: the deep small-batch BatchNorm generators are ill-conditioned (measured: 3e-3 / 7e-3 on the gradients of
    G / U-Net, 2e-4 / 7e-5 on the BatchNorm-free discriminators on this batch)"""
    cfg = ostep.default_cfg()
    Z, X, Y = ostep.synthetic_batch(2, cfg, seed=9)
    st64 = ostep.init_state(cfg, 0, np.float32)
    ref = ostep.train_step(st64, Z, X, Y, dtype=np.float64)
    st32 = ostep.init_state(cfg, 0, np.float32)
    fw32 = ostep.forward(st32, Z, X, Y, dtype=np.float32)
    g32 = ostep.gradients(fw32, st32)
    return (Z, X, Y), ref, st64, g32


@pytest.mark.parametrize("dtype", ["f32", "bf16x3"])
def test_full_size_step_matches_oracle_at_batch_2(gpu, dtype, batch2_oracle):
    """the real 512x512 nets of test1_nobn_bilin_both, one joint train_fn call, batch 2 (oracle-feasible; batch 1
    would make every BatchNorm over the batch axis degenerate), in both fp32 arithmetic modes with the same bounds.
    A discriminator's gradient is a function of its generator's OUTPUT (the fake half of its batch), so on these nets it
    inherits the generator chain's amplified rounding: between the fp32 MFMA mode and the split mode it moves by 1.2e-4 ... 2e-3
    from one batch to the next (tools/mode_agreement.py: 6 data seeds at batch 2) where the generators move by 2e-3 ... 8e-3 on
    every batch -- so the discriminators are bounded by their generator's float32-oracle spread, not by their own"""
    dev, ops, D = gpu
    from gan_heightmaps_amd.experiments import make_model
    from gan_heightmaps_amd import layers as L
    (Z, X, Y), ref, st64, g32 = batch2_oracle
    model = make_model('test1_nobn_bilin_both', device=dev, seed=0, verbose=False, dtype=dtype)
    got = model.train_fn(Z, X, Y)
    assert rel(got, ref['losses']) < 1e-5, (got, ref['losses'])
    nets = [('dcgan', 'gen', 'dcgan_gen'), ('dcgan', 'disc', 'dcgan_disc'), ('p2p', 'gen', 'p2p_gen'),
            ('p2p', 'disc', 'p2p_disc')]
    spread = {}
    for a, b, k in nets:                            # float32-vs-exact spread of the oracle itself, per net
        r = np.concatenate([x.ravel() for x in ref['grads'][(a, b)]])
        spread[(a, b)] = rel(np.concatenate([x.ravel() for x in g32[(a, b)]]), r)
    for a, b, k in nets:
        st = model.engine.stores[k]
        g = np.concatenate([st.download_grad(p).ravel()
                            for p in L.get_all_params(getattr(model, a)[b], trainable=True)])
        r = np.concatenate([x.ravel() for x in ref['grads'][(a, b)]])
        assert np.linalg.norm(r) > 0
        bound = 2 * max(spread[(a, b)], spread[(a, 'gen')]) + 1e-4
        assert rel(g, r) < bound, (dtype, k, rel(g, r), spread)
        p_new = np.concatenate([v.ravel() for v in L.get_all_param_values(getattr(model, a)[b])])
        p_ref = np.concatenate([np.asarray(v).ravel() for v in st64['params'][a][b]])
        assert rel(p_new, p_ref) < 1e-3, k                     # post-step parameters (RMSprop lr 1e-4)
    del model


@pytest.mark.parametrize("dtype", ["f32", "bf16x3"])
def test_full_size_batch4_step_against_the_float64_fixture(gpu, dtype):
    """(dtype 'bf16x3': the SAME test with the SAME bounds for the split-fp32 mode, csrc/conv_split.hip -- fp32 products as six
    bf16 piece products; it is held to everything the fp32 path is held to.)
    tests/golden/reference_step_fullsize_b4.npz (make_reference_step_fullsize_b4.py, build container): ONE joint
    train step of the four 512x512 test1_nobn_bilin_both networks at the reference's batch size 4 (experiments.py:121)
    on the float64 oracle.  No oracle runs on the GPU box.  Bounds (rel-L2; north_star: outputs within 1e-3):
      losses <= 1e-5;  G(z) and U(X) <= 1e-4 on a 64x64 lattice + one 64x64 full-resolution window per image;
      discriminator gradients <= 2e-4;  generator gradients <= 2 x (float32-oracle vs float64-oracle spread) + 1e-4
      (= 1.2e-3 / 4.3e-4: the deep small-batch BatchNorm chains amplify fp32 rounding, the fixture records by how
      much for a float32 run of the SAME oracle);  post-step parameter norms <= 1e-5."""
    import os
    dev, ops, D = gpu
    from gan_heightmaps_amd.experiments import make_model
    from gan_heightmaps_amd import layers as L
    fix = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_step_fullsize_b4.npz"))
    seed, batch, dseed, stride, win = (int(v) for v in fix["meta"])
    assert batch == 4
    cfg = ostep.default_cfg()
    model = make_model('test1_nobn_bilin_both', device=dev, seed=seed, verbose=False, use_graph=False, dtype=dtype)
    Z, X, Y = ostep.synthetic_batch(batch, cfg, seed=dseed)
    got = model.train_fn(Z, X, Y)
    assert rel(got, fix["losses64"]) < 1e-5, (got, fix["losses64"])
    b = model.engine.built(batch)
    if dtype != 'f32':          # the split kernels really are in the program
        names = {e[2]["kernel"] for lane in b.train_compute for e in lane if len(e) > 2 and e[2] is not None and e[2].get("dtype") == dtype}
        assert any(n.startswith("sp_conv2_kernel") for n in names) and any(n.startswith("sp_wgrad_kernel") for n in names), names
    for key, t in (("gz", b.G.out), ("ux", b.U.out)):          # the step's own forward outputs (pre-update parameters)
        a = t.numpy().astype(np.float64)
        lat = a[:, :, ::stride, ::stride]
        w = np.stack([a[n, :, 37 * (n + 1):37 * (n + 1) + win, 53 * (n + 1):53 * (n + 1) + win] for n in range(batch)])
        assert rel(lat, fix[key + "_sample64"]) < 1e-4, (key, rel(lat, fix[key + "_sample64"]))
        assert rel(w, fix[key + "_window64"]) < 1e-4, (key, rel(w, fix[key + "_window64"]))

    def summary(v):
        v64 = np.asarray(v, np.float64).ravel()
        idx = np.linspace(0, v64.size - 1, 8).astype(np.int64)
        return np.concatenate([[v64.sum(), np.sqrt((v64 * v64).sum())], v64[idx]])

    for a_, b_, k in [('dcgan', 'gen', 'dcgan_gen'), ('dcgan', 'disc', 'dcgan_disc'), ('p2p', 'gen', 'p2p_gen'),
                      ('p2p', 'disc', 'p2p_disc')]:
        st = model.engine.stores[k]
        params = L.get_all_params(getattr(model, a_)[b_], trainable=True)
        keys = sorted(q for q in fix.files if q.startswith("grad/%s/" % k))
        assert len(keys) == len(params)
        mine = [summary(st.download_grad(p)) for p in params]
        ref = [fix[q] for q in keys]
        r32 = [fix["grad32/" + q[5:]] for q in keys]
        live = [i for i, r in enumerate(ref) if r[1] > 1e-12]      # conv biases that feed a BatchNorm: exactly 0
        assert len(live) >= len(ref) // 2

        def cat(rows, sl):
            return np.concatenate([rows[i][sl] for i in live])
        spread = max(rel(cat(r32, slice(2, None)), cat(ref, slice(2, None))), rel(cat(r32, slice(1, 2)), cat(ref, slice(1, 2))))
        tol = 2e-4 if b_ == 'disc' else 2 * spread + 1e-4
        assert rel(cat(mine, slice(2, None)), cat(ref, slice(2, None))) < tol, (k, "sampled elements", tol)
        assert rel(cat(mine, slice(1, 2)), cat(ref, slice(1, 2))) < tol, (k, "per-tensor norms", tol)
        after = [summary(v) for v in L.get_all_param_values(getattr(model, a_)[b_])]
        akeys = sorted(q for q in fix.files if q.startswith("after/%s/" % k))
        assert len(akeys) == len(after)
        n_mine, n_ref = np.array([v[1] for v in after]), np.array([fix[q][1] for q in akeys])
        assert np.all(np.abs(n_mine - n_ref) <= 1e-5 * n_ref + 3e-6), k
    del model


@pytest.mark.parametrize("dtype", ["f32", "bf16x3"])
@pytest.mark.parametrize("mode", ["dcgan", "p2p"])
def test_full_size_batch4_single_stage_modes_against_the_fixture(gpu, mode, dtype):
    """(both fp32 arithmetic forms: bench.py reports configs 2 / 3 on the fp32 matrix instruction AND by operand splitting.)
    BASELINE configs 2 / 3: the same 512x512 nets with ``train_mode='dcgan'`` / ``'p2p'`` (pix2pix.py:136-141) given
    to the constructor, as bench.py --mode does.  Every loss and gradient root of the reference's step is evaluated at the
    pre-update parameters, so the trained stage's half of tests/golden/reference_step_fullsize_b4.npz (the JOINT step)
    is this mode's answer: all five losses, the trained stage's outputs, gradients and post-step parameters equal the
    fixture's; the other stage's parameters do not move (its fixture rows are the PRE-step norms + an update, so they
    must differ from the fixture's "after" rows by the RMSprop step that was not taken)."""
    import os
    dev, ops, D = gpu
    from gan_heightmaps_amd.experiments import make_model
    from gan_heightmaps_amd import layers as L
    fix = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_step_fullsize_b4.npz"))
    seed, batch, dseed, stride, win = (int(v) for v in fix["meta"])
    cfg = ostep.default_cfg()
    model = make_model('test1_nobn_bilin_both', device=dev, seed=seed, verbose=False, use_graph=False, train_mode=mode,
                       dtype=dtype)
    assert model.engine.train_mode == mode and model.engine.dtype == dtype
    Z, X, Y = ostep.synthetic_batch(batch, cfg, seed=dseed)
    frozen = ('p2p', 'dcgan')[mode == 'p2p']
    before = {(frozen, h): [v.copy() for v in L.get_all_param_values(getattr(model, frozen)[h])] for h in ('gen', 'disc')}
    got = model.train_fn(Z, X, Y)
    assert rel(got, fix["losses64"]) < 1e-5, (got, fix["losses64"])          # all five losses (pix2pix.py:142)
    b = model.engine.built(batch)
    key, t = (("gz", b.G.out), ("ux", b.U.out))[mode == 'p2p']
    a = t.numpy().astype(np.float64)
    assert rel(a[:, :, ::stride, ::stride], fix[key + "_sample64"]) < 1e-4

    def summary(v):
        v64 = np.asarray(v, np.float64).ravel()
        idx = np.linspace(0, v64.size - 1, 8).astype(np.int64)
        return np.concatenate([[v64.sum(), np.sqrt((v64 * v64).sum())], v64[idx]])

    for b_ in ('gen', 'disc'):
        k = "%s_%s" % (mode, b_)
        st = model.engine.stores[k]
        params = L.get_all_params(getattr(model, mode)[b_], trainable=True)
        keys = sorted(q for q in fix.files if q.startswith("grad/%s/" % k))
        assert len(keys) == len(params)
        mine = [summary(st.download_grad(p)) for p in params]
        ref = [fix[q] for q in keys]
        r32 = [fix["grad32/" + q[5:]] for q in keys]
        live = [i for i, r in enumerate(ref) if r[1] > 1e-12]

        def cat(rows, sl):
            return np.concatenate([rows[i][sl] for i in live])
        spread = max(rel(cat(r32, slice(2, None)), cat(ref, slice(2, None))), rel(cat(r32, slice(1, 2)), cat(ref, slice(1, 2))))
        tol = 2e-4 if b_ == 'disc' else 2 * spread + 1e-4
        assert rel(cat(mine, slice(2, None)), cat(ref, slice(2, None))) < tol, (k, tol)
        after = [summary(v) for v in L.get_all_param_values(getattr(model, mode)[b_])]
        akeys = sorted(q for q in fix.files if q.startswith("after/%s/" % k))
        n_mine, n_ref = np.array([v[1] for v in after]), np.array([fix[q][1] for q in akeys])
        assert np.all(np.abs(n_mine - n_ref) <= 1e-5 * n_ref + 3e-6), k
    for (a_, h), vals in before.items():                    # the other stage is evaluated, never updated
        now = L.get_all_param_values(getattr(model, a_)[h])
        trainable = {id(p) for p in L.get_all_params(getattr(model, a_)[h], trainable=True)}
        for p, v0, v1 in zip(L.get_all_params(getattr(model, a_)[h]), vals, now):
            if id(p) in trainable:
                assert np.array_equal(v0, v1), (a_, h, p.name)
    del model


# Bounds of the reduced-precision full-size step against the float64 fixture (rel-L2; "cos" = cosine of the sampled
# gradient elements to the exact ones).  ~2x what the MI355X measures (the test prints the measured values): operand
# rounding is 2^-9 (bf16) / 2^-12 (fp16) per product, accumulated over 9..25 x C products in fp32; the generators' deep
# batch-4 BatchNorm chains amplify it exactly as they amplify fp32 rounding (the fixture's own fp32-vs-fp64 spread is
# 1.2e-3 / 4.3e-4 there against 1e-7 per operation).
# Measured (MI355X): bf16 loss 6.0e-5, out 1.1e-2, disc 1.9e-3 (cos 0.9999996), gen 8.3e-2 (cos 0.997), after 3.7e-3.
# "after": post-step parameter norms; RMSprop's first step moves every element by lr*sqrt(10) in the direction of its
# gradient's SIGN, so elements whose gradient is below the rounding noise move the other way (zero-initialised biases
# most of all) -- a loose bound by nature.
LP_FULL_TOL = {'bf16': dict(loss=3e-4, out=3e-2, disc=5e-3, disc_cos=0.9999, gen=0.2, gen_cos=0.98, after=1e-2),
               # 'bf16x2' (two bf16 pieces per operand, three products): BASELINE config 4 inside north_star's 1e-3 on the
               # outputs, the losses and the discriminators' gradients
               'bf16x2': dict(loss=1e-4, out=1e-3, disc=1e-3, disc_cos=0.999999, gen=0.02, gen_cos=0.9998, after=1e-3),
               'f16': dict(loss=3e-5, out=5e-3, disc=2e-3, disc_cos=0.99999, gen=0.05, gen_cos=0.999, after=3e-3)}
# fp16 measured: loss 6.7e-6, out 1.5e-3, disc 7.1e-4, gen 1.8e-2 (cos 0.9999), after 9.2e-4.


@pytest.mark.parametrize("dtype", ["bf16", "f16", "bf16x2"])
def test_full_size_batch4_step_reduced_precision(gpu, dtype):
    """BASELINE config 4 (bf16) / the 512x512 half of config 5 (fp16) IN THEIR OWN ARITHMETIC at the reference's batch
    size (experiments.py:98-125): one joint train step of the four full-size test1_nobn_bilin_both networks with every
    served convolution on the bf16 / fp16 matrix cores, against the committed float64 fixture
    (tests/golden/reference_step_fullsize_b4.npz; no oracle runs on the GPU box).  Checked: the five losses, G(z) and
    U(X) on the lattice + window samples, the discriminators' gradients (sampled elements and per-tensor norms), the
    generators' gradients through their cosine to the exact gradient, the post-step parameter norms, and that the
    low-precision kernels really are in the program."""
    import os
    dev, ops, D = gpu
    from gan_heightmaps_amd.experiments import make_model
    from gan_heightmaps_amd import layers as L
    fix = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_step_fullsize_b4.npz"))
    seed, batch, dseed, stride, win = (int(v) for v in fix["meta"])
    cfg = ostep.default_cfg()
    model = make_model('test1_nobn_bilin_both', device=dev, seed=seed, verbose=False, use_graph=False, dtype=dtype)
    eng = model.engine
    b = eng.built(batch)
    lp_flops = all_flops = 0.0
    for lane in b.train_compute:
        for e in lane:
            if len(e) > 2 and e[2] is not None:
                all_flops += e[2]["flops"]
                if e[2].get("dtype") == dtype:
                    lp_flops += e[2]["flops"]
    assert lp_flops > 0.9 * all_flops, (lp_flops, all_flops)          # the step really runs on the low-precision kernels
    Z, X, Y = ostep.synthetic_batch(batch, cfg, seed=dseed)
    got = model.train_fn(Z, X, Y)
    tol = LP_FULL_TOL[dtype]
    m = dict(loss=rel(got, fix["losses64"]), out=0.0)
    for key, t in (("gz", b.G.out), ("ux", b.U.out)):
        a = t.numpy().astype(np.float64)
        lat = a[:, :, ::stride, ::stride]
        w = np.stack([a[n, :, 37 * (n + 1):37 * (n + 1) + win, 53 * (n + 1):53 * (n + 1) + win] for n in range(batch)])
        m['out'] = max(m['out'], rel(lat, fix[key + "_sample64"]), rel(w, fix[key + "_window64"]))

    def summary(v):
        v64 = np.asarray(v, np.float64).ravel()
        idx = np.linspace(0, v64.size - 1, 8).astype(np.int64)
        return np.concatenate([[v64.sum(), np.sqrt((v64 * v64).sum())], v64[idx]])

    m.update(disc=0.0, disc_cos=1.0, gen=0.0, gen_cos=1.0, after=0.0)
    for a_, b_, k in [('dcgan', 'gen', 'dcgan_gen'), ('dcgan', 'disc', 'dcgan_disc'), ('p2p', 'gen', 'p2p_gen'),
                      ('p2p', 'disc', 'p2p_disc')]:
        st = eng.stores[k]
        params = L.get_all_params(getattr(model, a_)[b_], trainable=True)
        keys = sorted(q for q in fix.files if q.startswith("grad/%s/" % k))
        assert len(keys) == len(params)
        mine = [summary(st.download_grad(p)) / eng.loss_scale for p in params]
        ref = [fix[q] for q in keys]
        live = [i for i, r in enumerate(ref) if r[1] > 1e-12]
        el_m = np.concatenate([mine[i][2:] for i in live])
        el_r = np.concatenate([ref[i][2:] for i in live])
        nm_m = np.array([mine[i][1] for i in live])
        nm_r = np.array([ref[i][1] for i in live])
        assert np.all(np.isfinite(el_m)) and np.all(np.isfinite(nm_m)), k
        which = 'disc' if b_ == 'disc' else 'gen'
        m[which] = max(m[which], rel(el_m, el_r), rel(nm_m, nm_r))
        m[which + '_cos'] = min(m[which + '_cos'], float(el_m @ el_r / (np.linalg.norm(el_m) * np.linalg.norm(el_r))))
        after = [summary(v) for v in L.get_all_param_values(getattr(model, a_)[b_])]
        akeys = sorted(q for q in fix.files if q.startswith("after/%s/" % k))
        n_mine, n_ref = np.array([v[1] for v in after]), np.array([fix[q][1] for q in akeys])
        m['after'] = max(m['after'], float(np.max(np.abs(n_mine - n_ref) / (n_ref + 3e-2))))
    print("full-size batch-4 step in %s vs float64 fixture: " % dtype + ", ".join("%s %.3g" % kv for kv in sorted(m.items())))
    for key, v in m.items():
        if key.endswith('_cos'):
            assert v > tol[key], (key, v, m)
        else:
            assert v < tol[key], (key, v, m)
    # master weights, gradients and optimiser state stay fp32; fp16 carries the loss scale
    assert eng.loss_scale == (32768.0 if dtype == 'f16' else 1.0)
    del model


def test_full_size_batch4_step_properties(gpu):
    dev, ops, D = gpu
    from gan_heightmaps_amd.experiments import make_model
    cfg = ostep.default_cfg()
    Z, X, Y = ostep.synthetic_batch(4, cfg, seed=3)
    runs = []
    for rep in range(2):
        m = make_model('test1_nobn_bilin_both', device=dev, seed=0, verbose=False)
        l0 = m.loss_fn(Z, X, Y)
        l1 = m.train_fn(Z, X, Y)
        l2 = m.train_fn(Z, X, Y)
        runs.append(np.array([l0, l1, l2], np.float64))
        if rep == 0:
            # loss_fn and train_fn report the same pre-update losses for the same inputs ...
            assert rel(l0, l1) < 1e-6
            # ... except that BN running statistics are not used in train mode, so they agree exactly in value
            assert np.all(np.isfinite(runs[0]))
            # one RMSprop step at lr 1e-4 moves the losses (the update really happened)
            assert not np.allclose(l1, l2)
            # generators: shapes and ranges of the forward-only functions at full size
            gz = m.z_fn(Z)
            ux = m.gen_fn(X)
            assert gz.shape == (4, 1, 512, 512) and gz.min() >= 0 and gz.max() <= 1          # sigmoid
            assert ux.shape == (4, 3, 512, 512) and np.abs(ux).max() <= 1                      # tanh
        del m
    # bit-for-bit repeatable from the same seed (split-K partials are reduced in a fixed order, no atomics on data)
    assert np.array_equal(runs[0], runs[1])


@pytest.mark.parametrize("dtype", ["f32", "bf16x3"])
def test_full_size_step_against_the_reference_executed_fixture(gpu, dtype):
    """(dtype 'bf16x3': the split-fp32 mode, csrc/conv_split.hip, held to the same bounds as the fp32 path.)
    tests/golden/reference_step_fullsize.npz: the reference's experiments.py -> Pix2Pix.__init__ -> its own 512x512
    architecture files, executed on the oracle's ops in float64 (tests/golden/make_reference_step_fullsize.py), one
    train_fn call at batch 2.  The HIP step must start from the same parameters (same RNG draws in the same order),
    return the same five losses and move every parameter tensor the same way."""
    import os
    dev, ops, D = gpu
    from gan_heightmaps_amd.experiments import make_model
    from gan_heightmaps_amd import layers as L
    fix = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_step_fullsize.npz"))
    seed, batch, dseed = (int(v) for v in fix["meta"])
    cfg = ostep.default_cfg()
    model = make_model('test1_nobn_bilin_both', device=dev, seed=seed, verbose=False, dtype=dtype)
    Z, X, Y = ostep.synthetic_batch(batch, cfg, seed=dseed)

    def summaries():
        out = {}
        for a in ("dcgan", "p2p"):
            for b in ("gen", "disc"):
                for i, v in enumerate(L.get_all_param_values(getattr(model, a)[b])):
                    v64 = np.asarray(v, np.float64).ravel()
                    idx = np.linspace(0, v64.size - 1, 8).astype(np.int64)
                    out["%s/%s/%03d" % (a, b, i)] = np.concatenate([[v64.sum(), np.sqrt((v64 * v64).sum())], v64[idx]])
        return out
    before = summaries()
    keys = sorted(k[len("before/"):] for k in fix.files if k.startswith("before/"))
    assert sorted(before) == keys and len(keys) == 180
    for k in keys:
        assert np.allclose(before[k], fix["before/" + k], rtol=1e-6, atol=1e-9), k      # identical initial parameters
    got = model.train_fn(Z, X, Y)
    assert rel(got, fix["train0"]) < 1e-5, (got, fix["train0"])
    after = summaries()
    # RMSprop's first step moves every element by lr * g / sqrt(0.1 g^2 + 1e-6): compare the movement itself
    d_hip = np.concatenate([(after[k] - before[k])[2:] for k in keys])
    d_ref = np.concatenate([(fix["after/" + k] - fix["before/" + k])[2:] for k in keys])
    assert np.linalg.norm(d_ref) > 0
    assert rel(d_hip, d_ref) < 2e-2, rel(d_hip, d_ref)
    assert np.mean(np.abs(d_hip - d_ref) < 2e-5) > 0.98
    # total movement per tensor (sum over all elements), relative to lr * sqrt(10) * size
    worst = 0.0
    for k in keys:
        ds_hip, ds_ref = (after[k] - before[k])[0], (fix["after/" + k] - fix["before/" + k])[0]
        scale = max(abs(ds_ref), 1e-4 * 3.2 * 8)
        worst = max(worst, abs(ds_hip - ds_ref) / scale)
    assert worst < 0.25, worst
    # norms after the step
    for k in keys:
        # (biases that feed a BatchNorm start at 0 and have an exactly-zero true gradient: they only carry the
        # summation-order noise of the BN backward reductions, RMSprop-amplified; hence the absolute term)
        assert abs(after[k][1] - fix["after/" + k][1]) <= 1e-4 * fix["after/" + k][1] + 3e-6, k
    del model


@pytest.mark.parametrize("name", ["test1_nobn", "test1_nobn_finetunep2p_bilin", "test1_nobn_bilin_both"])
def test_every_reference_experiment_steps_at_full_size(gpu, name):
    """experiments.py:22-131: the three registered experiments (k2-s2 deconv U-Net, p2p-only fine-tuning, the joint
    BASELINE config) build, take one 512x512 train step at batch 4 and generate, with finite results"""
    dev, ops, D = gpu
    from gan_heightmaps_amd.experiments import make_model
    cfg = ostep.default_cfg()
    Z, X, Y = ostep.synthetic_batch(4, cfg, seed=1)
    model = make_model(name, device=dev, seed=0, verbose=False)
    before = model.loss_fn(Z, X, Y)
    losses = model.train_fn(Z, X, Y)
    assert len(losses) == 5 and np.isfinite(losses).all() and np.isfinite(before).all()
    after = model.loss_fn(Z, X, Y)
    # the trained stage(s) moved, the untouched stage's losses did not (train_mode, pix2pix.py:131-141)
    if model.train_mode == 'p2p':
        assert after[0] == pytest.approx(before[0], rel=1e-3) and after[1] == pytest.approx(before[1], rel=1e-3)
    assert after[3] != before[3] or model.train_mode == 'dcgan'
    g, z = model.gen_fn_det(X), model.z_fn_det(Z)
    assert g.shape == (4, 3, 512, 512) and z.shape == (4, 1, 512, 512)
    assert np.isfinite(g).all() and np.isfinite(z).all() and np.abs(g).max() <= 1.0 and 0.0 <= z.min() <= z.max() <= 1.0
    del model


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_config5_geometry_1024(gpu, dtype):
    """BASELINE config 5 (beyond the reference: p2p.py:137 asserts 512): 1024x1024 crops need one more U-Net level and
    one more DCGAN stage; the same architecture functions build it and the engine steps it at the config's per-GPU
    batch (16 images on 8 GPUs = 2).  ``f16`` = the config's own arithmetic (fp16 matrix-core products, fp32
    accumulation, loss scale).  There is no parity target for this size, so the checks are the size-independent
    properties: the low-precision kernels carry the step, finite losses, output ranges of sigmoid / tanh, the update
    moves the losses, an fp16 step stays close to the fp32 step of the same parameters, and two runs from the same
    seed are bit-identical."""
    dev, ops, D = gpu
    from gan_heightmaps_amd import experiments as E
    from gan_heightmaps_amd.pix2pix import Pix2Pix

    def make(dt):
        kw = E.experiment_kwargs('test1_nobn_bilin_both')
        kw.update(in_shp=1024, device=dev, seed=0, verbose=False, dtype=dt)
        kw['gen_params_dcgan'] = {'num_repeats': 0, 'div': [2, 2, 4, 4, 8, 8, 8, 8], 'final_size': 1024}
        kw['disc_params_dcgan'] = dict(kw['disc_params_dcgan'], div=[8, 8, 4, 4, 4, 2, 2, 2], nch=1024)
        return Pix2Pix(**kw)

    rng = np.random.RandomState(0)
    Z = rng.rand(2, 1000).astype(np.float32)
    X = rng.rand(2, 1, 1024, 1024).astype(np.float32)
    Y = (rng.rand(2, 3, 1024, 1024) * 2 - 1).astype(np.float32)
    runs = []
    for rep in range(2 if dtype != 'f32' else 1):
        model = make(dtype)
        if dtype != 'f32' and rep == 0:
            b = model.engine.built(2)
            lp = sum(e[2]["flops"] for lane in b.train_compute for e in lane
                     if len(e) > 2 and e[2] is not None and e[2].get("dtype") == dtype)
            tot = sum(e[2]["flops"] for lane in b.train_compute for e in lane if len(e) > 2 and e[2] is not None)
            assert lp > 0.9 * tot, (lp, tot)
            assert model.engine.loss_scale == 32768.0
        l0 = model.loss_fn(Z, X, Y)
        l1 = model.train_fn(Z, X, Y)
        l2 = model.train_fn(Z, X, Y)
        l3 = model.train_fn(Z, X, Y)
        runs.append(np.array([l0, l1, l2, l3], np.float64))
        assert np.isfinite(runs[-1]).all(), runs[-1]
        if rep == 0:
            assert rel(l0, l1) < 1e-6                       # loss_fn and train_fn see the same pre-update losses
            assert not np.allclose(l1, l2)                  # the update happened
            assert l3[3] < l1[3]                            # the L1 reconstruction term goes down on a repeated batch
            g, z = model.gen_fn_det(X), model.z_fn_det(Z)
            assert g.shape == (2, 3, 1024, 1024) and z.shape == (2, 1, 1024, 1024)
            assert np.isfinite(g).all() and np.isfinite(z).all() and np.abs(g).max() <= 1.0 and 0.0 <= z.min() <= z.max() <= 1.0
        del model
    if dtype != 'f32':
        assert np.array_equal(runs[0], runs[1])              # bit-repeatable
        ref = make('f32')
        r1 = np.asarray(ref.train_fn(Z, X, Y), np.float64)
        print("config 5 (1024^2, batch 2) %s vs fp32 losses of the first step: rel-L2 %.3g" % (dtype, rel(runs[0][1], r1)))
        assert rel(runs[0][1], r1) < 5e-3, (runs[0][1], r1)
        del ref
