"""Erosion on the host (gan_heightmaps_amd/erosion.py, the eroded layer of gan_heightmaps_amd/world.py): the
Erosion object and its refusals, the raw chunks an eroded chunk is made from, the one LRU over both layers (on
tests/fake_device.py, with the two chunk makers replaced by counters), and the command lines' arguments.  No GPU."""
import dataclasses

import numpy as np
import pytest

from gan_heightmaps_amd import erosion as ER
from gan_heightmaps_amd import render as RN
from gan_heightmaps_amd import world as WD
from gan_heightmaps_amd.architectures import dcgan
from tests.fake_device import FakeDevice
from tests.test_terrain_plan import SMALL, _gen
from tests.test_world_plan import _Model, _world


# ---- the Erosion object -------------------------------------------------------------------------------------------------
def test_erosion_defaults_halo_and_freezing():
    e = ER.Erosion()
    assert ER.RADIUS == 3 and e.iterations == 32 and e.halo == 96 and e.height_scale == RN.DEFAULTS['height_scale'] == 64
    assert ER.Erosion(iterations=0).halo == 0 and ER.Erosion(iterations=np.int64(5)).halo == 15
    assert set(e.as_dict()) == set(ER.PARAMS) and "iterations" not in e.as_dict()
    assert all(isinstance(v, float) for v in ER.Erosion(gravity=10, pipe=np.float32(2)).as_dict().values())
    with pytest.raises(dataclasses.FrozenInstanceError):
        e.dt = 0.1
    assert e == ER.Erosion() and hash(e) == hash(ER.Erosion()) and e != ER.Erosion(rain=0.03)
    # the device structure carries the same twelve fields in the same order
    from gan_heightmaps_amd._lib import ErosionParams
    assert tuple(k for k, _ in ErosionParams._fields_) == ER.PARAMS
    assert ER.workspace_planes(True) == 14 and ER.workspace_planes(False) == 17


@pytest.mark.parametrize("kw,match", [
    (dict(min_depth=0.0), "min_depth"), (dict(min_depth=-1.0), "min_depth"),
    (dict(dt=0.05, max_speed=20.5), "dt \\* max_speed"), (dict(dt=0.5), "dt \\* max_speed"),
    (dict(iterations=2.0), "iterations"), (dict(iterations=True), "iterations"), (dict(iterations=-1), "iterations"),
    (dict(iterations="4"), "iterations"), (dict(dt=0.0), "dt"), (dict(max_speed=float("inf")), "max_speed"),
    (dict(rain=-0.1), "rain"), (dict(gravity=float("nan")), "gravity"), (dict(height_scale=0), "height_scale"),
    (dict(capacity="1"), "capacity"), (dict(evaporation=30.0), "evaporation"), (dict(max_speed=0.0), "max_speed")])
def test_erosion_refusals(kw, match):
    with pytest.raises(ValueError, match=match):
        ER.Erosion(**kw)


def test_the_backtrace_bound_is_inclusive():
    assert ER.Erosion(dt=0.25, max_speed=4.0).halo == 96          # dt max_speed = 1 exactly is allowed


def test_erode_refuses_before_it_touches_a_device():
    for bad in (np.zeros((3, 8, 8), np.float32), np.zeros((8, 8, 3), np.uint8), np.zeros((2, 1, 8, 8), np.float32),
                np.zeros(8, np.float32), np.zeros((0, 4), np.float32)):
        with pytest.raises(ValueError, match="one height|must be"):
            ER.erode(None, bad)
    with pytest.raises(ValueError, match="uint8 or floating"):
        ER.erode(None, np.zeros((4, 4), np.int32))
    with pytest.raises(ValueError, match="non-finite"):
        ER.erode(None, np.full((4, 4), np.inf))
    with pytest.raises(ValueError, match="must be an Erosion"):
        ER.erode(None, np.zeros((4, 4), np.float32), erosion=dict(iterations=3))


# ---- the eroded world's plan -------------------------------------------------------------------------------------------
def test_erosion_sources_cover_the_window_exactly():
    K = 64
    for E in (0, 1, 9, 63, 64):
        for a, b in ((0, 0), (-1, 2), (-3, -5), (7, -1)):
            srcs = WD.erosion_sources(a, b, K, E)
            n = K + 2 * E
            want = [(i, j) for i in range(a - (E > 0), a + (E > 0) + 1) for j in range(b - (E > 0), b + (E > 0) + 1)]
            assert [s[0] for s in srcs] == want                    # the nine around (a, b), row-major; itself for E = 0
            cover = np.zeros((n, n), int)
            for (ra, rb), r0, c0, nr, nc, wy, wx in srcs:
                assert 0 <= r0 and r0 + nr <= K and 0 <= c0 and c0 + nc <= K and nr > 0 and nc > 0
                cover[wy:wy + nr, wx:wx + nc] += 1
                # the rectangle's world coordinates are the window's
                assert ra * K + r0 == a * K - E + wy and rb * K + c0 == b * K - E + wx
            assert (cover == 1).all()
    assert WD.erosion_sources(-1, 0, 64, 9) == [
        ((-2, -1), 55, 55, 9, 9, 0, 0), ((-2, 0), 55, 0, 9, 64, 0, 9), ((-2, 1), 55, 0, 9, 9, 0, 73),
        ((-1, -1), 0, 55, 64, 9, 9, 0), ((-1, 0), 0, 0, 64, 64, 9, 9), ((-1, 1), 0, 0, 64, 9, 9, 73),
        ((0, -1), 0, 55, 9, 9, 73, 0), ((0, 0), 0, 0, 9, 64, 73, 9), ((0, 1), 0, 0, 9, 9, 73, 73)]


def test_world_refusals_at_construction():
    ero = ER.Erosion(iterations=3)
    w = _world(chunk_cells=2, erosion=ero)
    assert w.erosion is ero and w.eroded == 0 and w.computed == 0 and _world(chunk_cells=2).erosion is None
    assert _world(chunk_cells=1, erosion=ER.Erosion(iterations=10)).erosion.halo == 30            # E = 30 <= K = 32
    with pytest.raises(ValueError, match="more than a chunk"):
        _world(chunk_cells=1, erosion=ER.Erosion(iterations=11))                                    # E = 33 > K = 32
    with pytest.raises(ValueError, match="must be an erosion.Erosion"):
        _world(erosion=3)
    rgb = dcgan.default_generator(SMALL['latent_dim'], False, nch=SMALL['nch'], div=SMALL['div'])
    with pytest.raises(ValueError, match="one height"):
        _world(gen=rgb, erosion=ero)
    assert _world(gen=rgb).geometry.channels == 3                  # without erosion a 3-channel world is what it was


class _Counting(WD.TerrainWorld):
    """a TerrainWorld whose two chunk makers only count: the cache logic of _acquire on a FakeDevice"""

    def __init__(self, **kw):
        super().__init__(_Model(_gen(SMALL), SMALL['latent_dim']), 1, chunk_cells=2, **kw)
        self._dev = self._udev = FakeDevice()
        self.log = []

    def _compute(self, a, b):
        self.computed += 1
        self.log.append(('r', (a, b)))
        return self._cache.buffer()

    def _erode(self, srcs):
        assert all(s[0] in self._raw for s in srcs)               # every source is resident when its window is gathered
        self.eroded += 1
        self.log.append(('e', srcs[4][0]))
        return self._cache.buffer()

    def resident(self):
        assert len(self._cache.order) == len(self._chunks) + len(self._raw)
        return len(self._chunks) + len(self._raw)


def test_one_lru_bounds_raw_and_eroded_chunks_together():
    ero = ER.Erosion(iterations=3)
    w = _Counting(erosion=ero)
    keys = [(0, 0), (0, 1)]
    w._acquire(keys)
    assert (w.eroded, w.computed) == (2, 12) and w.resident() == 14            # 3 x 4 raw chunks serve both
    assert len(set(w._chunks.values()) | set(w._raw.values())) == 14           # no buffer is in two places
    w._acquire(keys)
    assert (w.eroded, w.computed) == (2, 12)                                   # warm: nothing runs
    w._acquire([(0, 2)])
    assert (w.eroded, w.computed) == (3, 15)                                   # one more raw column
    # a budget of 11 chunks of 16 KB: a window's nine raw chunks and the pinned eroded ones never leave mid-step
    w = _Counting(erosion=ero, cache_mb=11 * 16 / 1024)
    assert w._cache.capacity() == 11
    w._acquire(keys)
    assert (w.eroded, w.computed) == (2, 12) and w.resident() <= 11 and set(w._chunks) == set(keys)
    assert ('r', (-1, -1)) not in w._cache.order and ('r', (1, 2)) in w._cache.order       # the least recently used went first
    w._acquire([(5, 5)])
    assert set(w._chunks) >= {(5, 5)} and w.resident() <= 11
    w._cache.pinned = set()
    w._cache.evict(set())
    assert w.resident() <= 11
    # no budget at all: everything outside the step goes, a repeat recomputes
    w = _Counting(erosion=ero, cache_mb=0)
    w._acquire([(0, 0)])
    assert (w.eroded, w.computed) == (1, 9) and set(w._chunks) == {(0, 0)} and not w._raw
    w._acquire([(0, 1)])
    assert (w.eroded, w.computed) == (2, 18) and set(w._chunks) == {(0, 1)} and not w._raw
    w._drop()
    assert not w._chunks and not w._raw and not w._cache.order
    # without erosion the raw layer does not exist
    w = _Counting()
    w._acquire(keys)
    assert (w.eroded, w.computed) == (0, 2) and not w._raw and set(w._chunks) == set(keys)
    assert set(w._cache.order) == {('e', k) for k in keys}                    # the one LRU order holds no raw entry either


BUDGETS = (0, 1, 2, 3, 5, 8, 11, 20, 64)                          # chunks


def test_the_cache_follows_the_model_of_its_policy():
    """324 random request sequences (36 per budget), each on a plain and on an eroded world, against tests/world_cache_ref.py:
    after every call the same chunks were made in the same order, the same keys are resident in each layer, and no buffer
    is in two places (the layers and the recycling pool)"""
    from tests.world_cache_ref import CacheModel
    rng = np.random.RandomState(20)
    worlds = {(n, eroded): _Counting(cache_mb=n * 16 / 1024, **({"erosion": ER.Erosion(iterations=3)} if eroded else {}))
              for n in BUDGETS for eroded in (False, True)}
    evictions = 0
    for i in range(36 * len(BUDGETS)):
        n = BUDGETS[i % len(BUDGETS)]
        calls = []
        for _ in range(rng.randint(1, 13)):
            a, b, na, nb = rng.randint(-3, 6), rng.randint(-3, 4), rng.randint(1, 3), rng.randint(1, 5)
            calls.append([(a + i_, b + j) for i_ in range(na) for j in range(nb)])      # 1..2 x 1..4 keys in [-3, 6]^2
        for eroded in (False, True):
            w, model = worlds[(n, eroded)], CacheModel(n, eroded)
            assert w._cache.capacity() == n
            w._drop()                                             # an empty cache; what it held waits in the pool
            w.log = []
            for keys in calls:
                w._acquire(keys)
                model.acquire(keys)
                # (a plain world's chunks are what _compute makes, which _Counting logs as 'r')
                assert w.log == [(l if eroded else 'r', k) for l, k in model.made], (i, eroded, keys)
                assert set(w._chunks) == model.resident('e') and set(w._raw) == model.resident('r'), (i, eroded, keys)
                assert list(w._cache.order) == model.lru and w._cache.pinned == set(keys)
                ptrs = list(w._chunks.values()) + list(w._raw.values()) + w._cache.pool
                assert len(ptrs) == len(set(ptrs)), (i, eroded, keys)
            evictions += len(w.log) - len(set(w.log))
    assert evictions > 1000                                       # chunks were made again after they had been evicted


# ---- command lines --------------------------------------------------------------------------------------------------------
def test_erosion_cli_arguments():
    a = ER.parse_args(["in.png", "out.npy"])
    assert (a.input, a.output, a.water, a.plain, a.fused) == ("in.png", "out.npy", None, False, False)
    assert a.erosion == ER.Erosion() and ER.parse_args(["in.png", "out.npy", "--fused"]).fused
    a = ER.parse_args(["in.npy", "out.png", "--iterations", "7", "--water", "w.npy", "--min-depth", "0.1", "--dt", "0.1",
                       "--height-scale", "24", "--rain", "0.5", "--evaporation", "0", "--gravity", "5", "--pipe", "2",
                       "--capacity", "0.2", "--dissolve", "0.3", "--deposit", "0.4", "--min-tilt", "0.02", "--max-speed",
                       "8", "--plain"])
    assert a.erosion == ER.Erosion(iterations=7, dt=0.1, rain=0.5, evaporation=0.0, gravity=5.0, pipe=2.0, capacity=0.2,
                                   dissolve=0.3, deposit=0.4, min_tilt=0.02, max_speed=8.0, min_depth=0.1, height_scale=24.0)
    assert a.water == "w.npy" and a.plain and a.erosion.halo == 21
    for bad in (["in.npy"], ["a", "b", "--min-depth", "0"], ["a", "b", "--max-speed", "30"], ["a", "b", "--iterations", "2.5"],
                ["a", "b", "--iterations", "-2"], ["a", "b", "--plain", "--fused"]):
        with pytest.raises(SystemExit):
            ER.parse_args(bad)


def test_world_and_render_clis_take_erode():
    base = ["EXP", "m.model", "out.npy", "--seed", "4", "--region", "-70,33,90,61"]
    assert WD.parse_args(base).erode is None and WD.parse_args(base + ["--erode", "12"]).erode == 12
    with pytest.raises(SystemExit):
        WD.parse_args(base + ["--erode", "0"])
    cam = ["--pos", "1,2,3", "--yaw", "0", "--pitch", "-10"]
    wa = ["out.png", "--world", "EXP", "m.model", "--seed", "1", "--max-dist", "50"] + cam
    assert RN.parse_args(wa).erode is None and RN.parse_args(wa + ["--erode", "8"]).erode == 8
    with pytest.raises(SystemExit):
        RN.parse_args(wa + ["--erode", "0"])
    with pytest.raises(SystemExit):                                # --erode belongs to --world
        RN.parse_args(["out.png", "--heightmap", "h.png", "--texture", "t.png", "--erode", "8"] + cam)
