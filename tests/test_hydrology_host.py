"""The host side of the hydrology (gan_heightmaps_amd/hydrology.py): Water's validation, the refusals that are made
before the device is touched, the command line's parsing, and that the shared cases cover lakes and large flats.  No device."""
import numpy as np
import pytest

from gan_heightmaps_amd import hydrology as HY
from tests import hydrology_ref as R


def test_water_defaults_and_validation():
    w = HY.Water()
    assert (w.river_threshold, w.river_width, w.lake_min_depth, w.colour, w.opacity) == (256, 1, 1.0 / 512, (0.13, 0.29, 0.45), 0.85)
    assert HY.Water(river_threshold=np.int64(3), river_width=np.int32(4), colour=[0, 1, 0.5], opacity=1) == \
        HY.Water(river_threshold=3, river_width=4, colour=(0.0, 1.0, 0.5), opacity=1.0)
    assert hash(HY.Water()) == hash(HY.Water())
    with pytest.raises(Exception):
        w.opacity = 0.5                                                   # frozen
    for kw in (dict(river_threshold=0), dict(river_threshold=1 << 32), dict(river_threshold=2.0), dict(river_threshold=True),
               dict(river_width=-1), dict(river_width=5), dict(river_width=1.0), dict(lake_min_depth=-1e-3),
               dict(lake_min_depth=float("nan")), dict(lake_min_depth=float("inf")), dict(opacity=1.5), dict(opacity=-0.1),
               dict(opacity=None), dict(colour=(0.1, 0.2)), dict(colour=(0.1, 0.2, 1.5)), dict(colour=0.3),
               dict(colour=(0.1, 0.2, float("nan")))):
        with pytest.raises(ValueError):
            HY.Water(**kw)


def test_refusals_before_the_device_is_touched():
    ops = None                                                            # nothing may reach for it
    good = R.terrain(8, 9, None, 1)
    for bad in (np.zeros((2, 8, 9), np.float32), np.zeros(8, np.float32), np.zeros((1, 1, 8, 9), np.float32),
                np.zeros((8, 9), np.int32), np.zeros((0, 9), np.float32)):
        with pytest.raises(ValueError):
            HY.analyse(ops, bad)
    for v in (np.nan, np.inf, -np.inf):
        x = good.copy()
        x[3, 4] = v
        with pytest.raises(ValueError, match="non-finite"):
            HY.analyse(ops, x)
    # H W >= 2^31 by shape arithmetic alone: a view of one float, never read
    huge = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), shape=(1 << 16, 1 << 15), strides=(0, 0), writeable=False)
    with pytest.raises(ValueError, match="out of range"):
        HY.analyse(ops, huge)
    tall = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), shape=(4 * 65535 + 1, 2), strides=(0, 0), writeable=False)
    with pytest.raises(ValueError, match="out of range"):
        HY.analyse(ops, tall)
    with pytest.raises(ValueError, match="keep"):
        HY.analyse(ops, good, keep=("filled", "rivers"))
    # paint: the hydrology and the water are checked first, then the texture's form and size
    hydro = HY.Hydrology((8, 9), (1, 1), 1, False, depth=np.zeros((8, 9), np.float32), accumulation=np.ones((8, 9), np.uint32))
    tex = np.zeros((8, 9, 3), np.uint8)
    with pytest.raises(ValueError, match="Water"):
        HY.paint(ops, tex, hydro, water=dict(opacity=1))
    with pytest.raises(ValueError, match="depth"):
        HY.paint(ops, tex, HY.Hydrology((8, 9), (1, 1), 1, False, filled=good))
    with pytest.raises(ValueError, match="depth"):
        HY.paint(ops, tex, None)
    with pytest.raises(ValueError, match="differ in size"):
        HY.paint(ops, np.zeros((9, 8, 3), np.uint8), hydro)
    for bad in (np.zeros((8, 9, 2), np.uint8), np.zeros((2, 8, 9), np.float32), np.zeros((8, 9), np.float64),
                np.full((8, 9), np.nan, np.float32)):
        with pytest.raises(ValueError):
            HY.paint(ops, bad, hydro)


def test_the_heightmap_is_read_as_elsewhere():
    u8 = np.arange(12, dtype=np.uint8).reshape(3, 4)
    assert np.array_equal(HY._as_plane(u8), u8.astype(np.float32) / np.float32(255))
    x = np.array([[-0.0, 0.5], [1.0, -2.0]], np.float64)
    p = HY._as_plane(x[None])
    assert p.dtype == np.float32 and p.shape == (2, 2) and not np.signbit(p[0, 0]) and p[1, 1] == -2
    assert HY.texture_colour((0.0, 0.5, 1.0), True) == (0.0, 0.5, 1.0)
    assert HY.texture_colour((0.0, 0.5, 1.0), False) == (-1.0, 0.0, 1.0)


def test_command_line_parsing():
    a = HY.parse_args(["in.png", "out/prefix"])
    assert (a.input, a.out_prefix, a.texture, a.painted, a.form) == ("in.png", "out/prefix", None, None, None)
    assert a.water == HY.Water()
    a = HY.parse_args(["in.npy", "p", "--texture", "t.png", "--painted", "o.png", "--river-threshold", "64", "--river-width", "0",
                       "--lake-min-depth", "0.01", "--opacity", "0.5", "--tiled"])
    assert a.water == HY.Water(river_threshold=64, river_width=0, lake_min_depth=0.01, opacity=0.5)
    assert (a.texture, a.painted, a.form) == ("t.png", "o.png", True)
    assert HY.parse_args(["i", "p", "--plain"]).form is False
    for bad in (["i"], ["i", "p", "--plain", "--tiled"], ["i", "p", "--texture", "t.png"], ["i", "p", "--painted", "o.png"],
                ["i", "p", "--river-width", "5"], ["i", "p", "--opacity", "2"], ["i", "p", "--river-threshold", "0"]):
        with pytest.raises(SystemExit):
            HY.parse_args(bad)


def test_the_shared_cases_have_lakes_and_a_large_flat():
    """the device tests cannot pass on terrain without depressions to fill and flats to cross"""
    lakes, plateaus = [], []
    for H, W, q, seed in R.CASES:
        r = R.analyse(R.terrain(H, W, q, seed))
        lakes.append(int((r.depth > 0).sum()))
        plateaus.append(R.largest_plateau(r.filled, r.flat))
    print("lake cells %s, largest plateau of non-draining cells %s" % (lakes, plateaus))
    assert max(lakes) > 0 and max(plateaus) > 1000
    assert sum(n > 0 for n in lakes) >= 2 and min(p for p in plateaus) < 100       # and cases of the other kind
