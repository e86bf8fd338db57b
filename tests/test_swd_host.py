"""The sliced Wasserstein distance on the host (gan_heightmaps_amd/swd.py, Pix2Pix.train's swd_every): the
parameter object, the memory estimate and its refusal, the shape / overflow / not-full / zero-variance errors (on
tests/fake_device.py with an Ops that only records), the swd.txt layout and the command line's arguments.  No GPU."""
import dataclasses

import numpy as np
import pytest

from gan_heightmaps_amd import swd as SW
from gan_heightmaps_amd.device import DevTensor
from gan_heightmaps_amd.pix2pix import Pix2Pix
from tests.fake_device import FakeDevice


class FakeOps:
    """records the swd calls; the FakeDevice behind it returns zeros for every download"""

    def __init__(self):
        self.dev = FakeDevice()
        self.calls = []

    def swd_workspace(self):
        return 16384

    def __getattr__(self, name):
        if not name.startswith("swd_"):
            raise AttributeError(name)
        return lambda *a: self.calls.append((name,) + a)


def test_the_parameter_object_is_validated_and_frozen():
    m = SW.SWD()
    assert (m.levels, m.patches_per_image, m.patch, m.directions, m.repeats, m.seed) == (None, 128, 7, 128, 4, 0)
    with pytest.raises(dataclasses.FrozenInstanceError):
        m.repeats = 2
    assert m == SW.SWD() and hash(m) == hash(SW.SWD()) and m != SW.SWD(seed=1)
    for bad in (5, 3, 8, None, 7.5):
        with pytest.raises(ValueError, match="only patch=7"):
            SW.SWD(patch=bad)
    for kw in (dict(patches_per_image=0), dict(directions=1.5), dict(repeats=True), dict(levels=0), dict(seed=-1),
               dict(seed=2 ** 32), dict(levels="2")):
        with pytest.raises(ValueError):
            SW.SWD(**kw)
    assert m.num_levels(512, 512) == 6 and m.sizes(64, 96) == [(64, 96), (32, 48), (16, 24)]
    assert m.num_levels(16, 16) == 1 and SW.SWD(levels=2).num_levels(512, 512) == 2
    for H, W, kw in ((15, 15, {}), (8, 64, {}), (32, 32, dict(levels=3)), (33, 32, dict(levels=2)), (66, 64, dict(levels=3))):
        with pytest.raises(ValueError, match="levels need"):
            SW.SWD(**kw).num_levels(H, W)


def test_the_memory_need_is_computed_up_front_and_refused_over_max_mb():
    m = SW.SWD()
    # the default Pix2Pix.swd call: 1024 images of 1 x 512 x 512, six levels of 2^17 descriptors of 49 floats and their
    # corners, and the workspace of 4 images: staging, Lap, G_1, G_2
    need = SW.Descriptors.need(m, 1024, 1, 512, 512, max_batch=4)
    img = 4 * 512 * 512
    assert need == 4 * (6 * 131072 * 49 + 6 * 131072 * 2 + img + img + img // 4 + img // 16)
    assert SW.Descriptors.need(m, 1024, 3, 512, 512, 4) > 2.9 * need
    ops = FakeOps()
    with pytest.raises(ValueError, match=r"need 162\.2 MB of device memory, over max_mb=100"):
        SW.Descriptors(ops, m, 0, 1024, 1, 512, 512, max_mb=100, max_batch=4)
    assert ops.dev.bytes_allocated == 0                          # refused before anything is allocated
    d = SW.Descriptors(ops, m, 0, 1024, 1, 512, 512, max_mb=163, max_batch=4)
    assert d.bytes == need == ops.dev.bytes_allocated and (d.N, d.K, d.L) == (131072, 49, 6)
    d.close()
    with pytest.raises(ValueError, match="closed"):
        d.add(np.zeros((1, 1, 512, 512), np.float32))
    for bad in (dict(set_index=2), dict(C=5), dict(n_images=0), dict(H=15), dict(metric="swd")):
        kw = dict(metric=m, set_index=0, n_images=4, C=1, H=32, W=32)
        kw.update(bad)
        with pytest.raises(ValueError):
            SW.Descriptors(FakeOps(), **kw)


def test_add_checks_shapes_and_overflow_and_issues_one_pass_per_level():
    m = SW.SWD(patches_per_image=4, directions=8, repeats=1)
    ops = FakeOps()
    with SW.Descriptors(ops, m, 1, 6, 3, 32, 64, max_batch=4) as d:
        for bad in ((2, 1, 32, 64), (2, 3, 64, 32), (3, 32, 64), (0, 3, 32, 64)):
            with pytest.raises(ValueError, match="a batch must be"):
                d.add(np.zeros(bad, np.float32))
        d.add(np.zeros((4, 3, 32, 64), np.float32))
        assert d.count == 4 and not d.full
        with pytest.raises(ValueError, match="3 images more than the 6"):
            d.add(np.zeros((3, 3, 32, 64), np.float32))
        names = [c[0] for c in ops.calls]
        assert names == ["swd_pyramid_level", "swd_gather"] * 2                  # two levels
        (_, g0, _, nxt0, np0, lap0, lp0), (_, g1, _, nxt1, _, _, lp1) = ops.calls[0], ops.calls[2]
        assert g0.shape == (4, 3, 32, 64) and g0.ptr == d._stage and (np0, lp0) == (32, 64) and nxt0 == d._g[0]
        assert g1.shape == (4, 3, 16, 32) and g1.ptr == d._g[0] and nxt1 is None and lp1 == 32
        assert ops.calls[1][1:] == (d._lap, 4, 3, 32, 64, 64, d._corners[0], 4, d.desc[0], 0, 24)
        ops.calls.clear()
        t = DevTensor(ops.dev, 4096, (2, 3, 32, 64), 77777)                      # a view with its own sample stride
        d.add(t)
        assert d.full and ops.calls[0][1].ptr == 4096 and ops.calls[0][1].nstride == 77777       # read where it lies
        # the second batch reads its rows of the one corner table, and appends below the first
        assert ops.calls[1][1:] == (d._lap, 2, 3, 32, 64, 64, d._corners[0] + 8 * 4 * 4, 4, d.desc[0], 16, 24)
        with pytest.raises(ValueError, match="more than the 6"):
            d.add(t)


def test_distance_refuses_sets_that_are_not_full_or_differ_and_zero_variance():
    m = SW.SWD(patches_per_image=4, directions=8, repeats=1)
    ops = FakeOps()
    a, b = SW.Descriptors(ops, m, 0, 4, 1, 32, 32), SW.Descriptors(ops, m, 1, 4, 1, 32, 32)
    a.add(np.zeros((4, 1, 32, 32), np.float32))
    b.add(np.zeros((2, 1, 32, 32), np.float32))
    with pytest.raises(ValueError, match="set 1 is not full: 2 of 4"):
        SW.distance(ops, a, b)
    b.add(np.zeros((2, 1, 32, 32), np.float32))
    for other in (SW.Descriptors(ops, m, 1, 4, 3, 32, 32), SW.Descriptors(ops, m, 1, 4, 1, 32, 64),
                  SW.Descriptors(ops, SW.SWD(patches_per_image=4, directions=8, repeats=2), 1, 4, 1, 32, 32)):
        other.count = other.n_images
        with pytest.raises(ValueError, match="the sets differ"):
            SW.distance(ops, a, other)
    with pytest.raises(ValueError, match="two open Descriptors"):
        SW.distance(ops, a, np.zeros((4, 1, 32, 32)))
    with pytest.raises(ValueError, match=r"need \d+\.\d MB of device memory, over max_mb=1e-05"):
        SW.distance(ops, a, b, max_mb=1e-5)
    # the fake device downloads zeros: a standard deviation of 0, refused on the host with level and channel
    with pytest.raises(ValueError, match="set 0, level 0, channel 0: the standard deviation"):
        SW.distance(ops, a, b)
    with pytest.raises(ValueError, match="one shape"):
        SW.compare(ops, np.zeros((4, 1, 32, 32)), np.zeros((4, 1, 32, 64)))


def test_train_refuses_the_training_iterators_as_swd_iterator(tmp_path):
    model = Pix2Pix.__new__(Pix2Pix)                             # the refusal comes before anything of the model is touched
    it_train, it_val = object(), object()
    for it in (it_train, it_val, None):
        with pytest.raises(ValueError, match="an iterator of its own"):
            model.train(it_train, it_val, 4, 1, str(tmp_path), swd_every=1, swd_iterator=it)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="swd_every"):
            model.train(it_train, it_val, 4, 1, str(tmp_path), swd_every=bad, swd_iterator=object())
    assert not list(tmp_path.iterdir())                          # and nothing was written


def test_swd_txt_layout():
    res = {"levels": [64, 32, 16], "swd": [1.5, 2.25, 0.1], "mean": (1.5 + 2.25 + 0.1) / 3}
    assert SW.header(res["levels"]) == ["epoch", "weights", "net", "swd_64", "swd_32", "swd_16", "mean"]
    r = SW.row(7, "ema", "p2p", res)
    assert r[:3] == ["7", "ema", "p2p"] and [float(v) for v in r[3:]] == res["swd"] + [res["mean"]]
    assert len(r) == len(SW.header(res["levels"]))


def test_swd_draws_z_from_its_own_random_state():
    model = Pix2Pix.__new__(Pix2Pix)
    model.latent_dim = 5
    for sampler, name in ((np.random.rand, "rand"), (np.random.randn, "randn"), (np.random.RandomState(3).rand, "rand")):
        model.sampler = sampler
        state = np.random.get_state()[1].copy()
        z = model._own_draw(np.random.RandomState(9), 4)
        assert z.dtype == np.float32 and np.array_equal(z, getattr(np.random.RandomState(9), name)(4, 5).astype(np.float32))
        assert np.array_equal(np.random.get_state()[1], state)   # numpy's global RNG did not move
    model.sampler = lambda n, d: np.zeros((n, d))
    with pytest.raises(ValueError, match="pass z="):
        model._own_draw(np.random.RandomState(9), 4)


def test_cli_arguments():
    a = SW.parse_args(["test1_nobn_bilin_both", "models/10.model"])
    assert (a.experiment, a.model, a.images, a.batch_size, a.which, a.seed, a.dtype, a.ema) == \
        ("test1_nobn_bilin_both", "models/10.model", 1024, 4, "both", 0, "bf16x3", False)
    assert a.metric == SW.SWD() and a.real is None and a.fake is None
    a = SW.parse_args(["EXP", "m/20.model", "--images", "64", "--batch-size", "8", "--which", "dcgan", "--seed", "5",
                       "--dtype", "f32", "--ema", "--patches", "32", "--directions", "16", "--repeats", "2", "--levels", "3"])
    assert (a.images, a.batch_size, a.which, a.seed, a.dtype, a.ema) == (64, 8, "dcgan", 5, "f32", True)
    assert a.model == "m/20.ema.model"                           # the file train writes beside 20.model
    assert a.metric == SW.SWD(levels=3, patches_per_image=32, directions=16, repeats=2, seed=5)
    assert SW.ema_path("m/20.ema.model") == "m/20.ema.model" and SW.ema_path("weights.pkl") == "weights.pkl"
    a = SW.parse_args(["--real", "dir_a", "--fake", "b.npy", "--seed", "2"])
    assert (a.real, a.fake, a.experiment, a.metric.seed) == ("dir_a", "b.npy", None, 2)
    for bad in ([], ["EXP"], ["--real", "a"], ["--fake", "b"], ["EXP", "m.model", "--real", "a", "--fake", "b"],
                ["--real", "a", "--fake", "b", "--ema"], ["EXP", "m.model", "--which", "all"],
                ["EXP", "m.model", "--images", "0"], ["EXP", "m.model", "--images", "2", "--batch-size", "4"],
                ["EXP", "m.model", "--patches", "0"]):
        with pytest.raises(SystemExit):
            SW.parse_args(bad)


def test_read_set_reads_npy_and_png_folders(tmp_path):
    x = np.random.RandomState(0).randint(0, 256, (3, 16, 16)).astype(np.uint8)
    np.save(tmp_path / "u8.npy", x)
    got = SW.read_set(str(tmp_path / "u8.npy"))
    assert got.shape == (3, 1, 16, 16) and got.dtype == np.float32 and np.array_equal(got[:, 0], x / np.float32(255))
    np.save(tmp_path / "f.npy", np.ones((2, 3, 16, 16)))
    assert SW.read_set(str(tmp_path / "f.npy")).shape == (2, 3, 16, 16)
    from PIL import Image
    (tmp_path / "png").mkdir()
    for i in range(3):
        Image.fromarray(x[i]).save(tmp_path / "png" / ("%d.png" % i))
    assert np.array_equal(SW.read_set(str(tmp_path / "png")), got)
    Image.fromarray(np.stack([x[0]] * 3, axis=-1)).save(tmp_path / "png" / "3.png")
    assert SW.read_set(str(tmp_path / "png")).shape == (4, 3, 16, 16)
    with pytest.raises(ValueError, match="no PNG"):
        SW.read_set(str(tmp_path))
