"""The host side of the climate (gan_heightmaps_amd/climate.py) without a device: the validation of Weather and Biomes,
the Climate's methods and writers, regions.biomes, the command lines, and -- over tests/fake_device.py -- that ``analyse`` and ``paint``
send their launches inside one scratch and free it, on success and on failure.  Last, the device source of both transport forms
compiled for the CPU (tests/climate_host/harness.cpp) as a stand-alone program under the address and undefined-behaviour sanitizers."""
import numpy as np
import pytest

from gan_heightmaps_amd import climate as CL
from gan_heightmaps_amd import hydrology as HY
from gan_heightmaps_amd import regions as RG
from tests import climate_ref as R


# ---- Weather and Biomes ---------------------------------------------------------------------------------------------------------------
def test_weather_validation():
    w = CL.Weather()
    assert w == CL.Weather(wind='W') and hash(w) == hash(CL.Weather()) and w.spread == 1 and isinstance(w.spread, int)
    assert CL.Weather(spread=np.int64(3), humidity=np.float32(0.5)) == CL.Weather(spread=3, humidity=0.5)
    with pytest.raises(Exception):
        w.wind = 'E'                                                       # frozen
    for kw in (dict(wind='X'), dict(wind=3), dict(wind='n'), dict(sea_level=-0.1), dict(sea_level=1.1), dict(humidity=2), dict(humidity="wet"),
               dict(evaporation=-1), dict(drizzle=1.5), dict(uplift=-0.1), dict(uplift=16.5), dict(recycle=1.01), dict(spread=9),
               dict(spread=-1), dict(spread=1.5), dict(sea_temperature=101), dict(sea_temperature=-101), dict(lapse=-1), dict(lapse=17),
               dict(latitude=1.5), dict(latitude=-1.5), dict(reference_rain=0), dict(reference_rain=1.5), dict(height_scale=0),
               dict(height_scale=65537), dict(humidity=float("nan")), dict(lapse=None)):
        with pytest.raises(ValueError, match=list(kw)[0]):
            CL.Weather(**kw)
    q = CL.Weather(wind='SE', sea_level=0.5, humidity=1, evaporation=0.25, drizzle=0.5, uplift=16, recycle=1, spread=8, sea_temperature=-100,
                   lapse=16, latitude=-1, reference_rain=1e-9, height_scale=2).quantised()
    assert q == dict(wind=3, sea_q=256, hum_q=65536, evap_q=16384, base_q=32768, up_q=1 << 20, rec_q=65536, spread=8, t0_q=-25600,
                     lapse_q=1 << 20, lat_q=-(1 << 24), ref_q=1)
    assert CL.WINDS == R.WINDS and CL.FORMS == ('line', 'staged') and CL.DEFAULT_FORM in CL.FORMS


def test_biomes_validation():
    b = CL.Biomes()
    assert b == CL.Biomes() and hash(b) == hash(CL.Biomes()) and b.names[b.ocean] == 'ocean' and len(b.names) == len(b.colours) == 12
    for name in ("ice", "tundra", "taiga", "grassland", "desert", "shrubland", "temperate forest", "savanna", "rainforest"):
        assert any(b.label(name) in row for row in b.table), name
    te, re_, tb = b.quantised()
    assert te.dtype == re_.dtype == tb.dtype == np.int32 and tb.shape == (5, 5) and te.tolist() == [-2560, 0, 2048, 5120]
    with pytest.raises(Exception):
        b.ocean = 1
    two = dict(temperature_edges=(0,), rain_edges=(), table=((1,), (2,)), names=("sea", "cold", "warm"), colours=(None, (1, 1, 1), None), ocean=0)
    ok = CL.Biomes(**two)
    assert ok.table == ((1,), (2,)) and ok.colours == (None, (1.0, 1.0, 1.0), None) and ok.quantised()[1].size == 0
    assert CL.Biomes((), (), ((1,),), ("sea", "land"), (None, None), 0).table == ((1,),)
    for kw, match in ((dict(temperature_edges=(5, 5)), "ascend"), (dict(temperature_edges=(5, 1)), "ascend"), (dict(temperature_edges=(0, 0.001)), "ascend"),
                      (dict(temperature_edges=tuple(range(9))), "temperature_edges"), (dict(temperature_edges=(-101,)), "temperature_edges"),
                      (dict(temperature_edges=3), "temperature_edges"), (dict(rain_edges=(1.5,)), "rain_edges"), (dict(rain_edges=(-0.1,)), "rain_edges"),
                      (dict(rain_edges=(0.5, 0.2)), "ascend"), (dict(table=((1,),)), "table"), (dict(table=((1, 1), (2, 2))), "table"),
                      (dict(table=((1,), (3,))), "table entry"), (dict(table=((1,), (-1,))), "table entry"), (dict(table=((1,), (0,))), "table entry"),
                      (dict(table=((1,), (1.5,))), "table entry"), (dict(table=5), "table"), (dict(names=("a", "a", "b")), "names"),
                      (dict(names=()), "names"), (dict(names=("a", "", "b")), "names"), (dict(names=tuple("n%d" % i for i in range(65))), "names"),
                      (dict(colours=(None,)), "colours"), (dict(colours=(None, (1, 2, 3), None)), "colour"), (dict(colours=(None, (1, 1), None)), "colour"),
                      (dict(colours=(None, 4, None)), "colour"), (dict(ocean=3), "ocean"), (dict(ocean=-1), "ocean"), (dict(ocean=0.5), "ocean")):
        with pytest.raises(ValueError, match=match):
            CL.Biomes(**dict(two, **kw))
    with pytest.raises(ValueError, match="no biome is called 'swamp'"):
        b.label("swamp")


# ---- Climate ----------------------------------------------------------------------------------------------------------------------------
def hand_made(**kw):
    b = CL.Biomes()
    biome = np.array([[0, 0, 3, 3], [0, 5, 5, 7], [4, 4, 4, 7]], np.int32)
    planes = dict(rain=np.arange(12, dtype=np.uint32).reshape(3, 4) * 100, temperature=np.array([[5120] * 4, [0] * 4, [-384] * 4], np.int32),
                  biome=biome, discharge=np.arange(12, dtype=np.uint64).reshape(3, 4) << np.uint64(30),
                  effective_area=np.arange(12, dtype=np.uint32).reshape(3, 4) + 1)
    planes.update(kw)
    return CL.Climate((3, 4), (10, -20), CL.Weather(wind='NE'), b, form='line', rounds=2, **planes)


def test_climate_methods():
    c = hand_made()
    assert c.shape == (3, 4) and c.origin == (10, -20) and c.raw is None and c.rounds == 2 and "wind NE" in repr(c) and "biome" in repr(c)
    assert c.celsius().dtype == np.float64 and c.celsius()[:, 0].tolist() == [20.0, 0.0, -1.5]
    assert c.mask("taiga").tolist() == [[False, False, True, True], [False] * 4, [False] * 4] and c.mask("taiga").dtype == bool
    assert c.mask("desert", "temperate forest").sum() == 4 and not c.mask("ice").any() and c.mask("ocean").sum() == 3
    with pytest.raises(ValueError, match="no biome is called"):
        c.mask("taiga", "marsh")
    with pytest.raises(ValueError, match="one biome name"):
        c.mask()
    s = c.share()
    assert "ocean" not in s and set(s) == set(c.biomes.names) - {"ocean"} and abs(sum(s.values()) - 1) < 1e-12
    assert s["grassland"] == 3 / 9 and s["taiga"] == s["desert"] == s["temperate forest"] == 2 / 9 and s["ice"] == 0.0
    assert set(hand_made(biome=np.zeros((3, 4), np.int32)).share().values()) == {0.0}
    with pytest.raises(ValueError, match="needs the temperature plane"):
        hand_made(temperature=None).celsius()
    with pytest.raises(ValueError, match="needs the biome plane"):
        hand_made(biome=None).share()
    with pytest.raises(ValueError, match="needs the biome plane"):
        hand_made(biome=None).mask("ice")


def test_the_climates_hydrology_swaps_the_accumulation_alone():
    c = hand_made()
    planes = dict(filled=np.ones((3, 4), np.float32), depth=np.zeros((3, 4), np.float32), direction=np.full((3, 4), -1, np.int8),
                  accumulation=np.ones((3, 4), np.uint32), basin=np.arange(12, dtype=np.int32).reshape(3, 4))
    hydro = HY.Hydrology((3, 4), (5, 6), 3, True, **planes)
    got = c.hydrology(hydro)
    assert isinstance(got, HY.Hydrology) and got is not hydro and got.accumulation is c.effective_area
    assert (got.shape, got.sweeps, got.rounds, got.tiled) == ((3, 4), (5, 6), 3, True)
    for k in ("filled", "depth", "direction", "basin"):
        assert getattr(got, k) is planes[k]
    assert hydro.accumulation is planes["accumulation"]                   # the one that came in is as it was
    with pytest.raises(ValueError, match="needs the effective_area plane"):
        hand_made(effective_area=None).hydrology(hydro)
    with pytest.raises(ValueError, match="Hydrology of the climate's size"):
        c.hydrology(HY.Hydrology((4, 3), (1, 1), 1, True))
    with pytest.raises(ValueError, match="Hydrology of the climate's size"):
        c.hydrology(planes)


def test_save_round_trips(tmp_path):
    c = hand_made()
    c.save(str(tmp_path / "c.npz"))
    z = np.load(str(tmp_path / "c.npz"))
    for k in CL.KEEP:
        assert np.array_equal(z[k], getattr(c, k)) and z[k].dtype == getattr(c, k).dtype, k
    assert "raw" not in z.files and z["origin"].tolist() == [10, -20] and z["shape"].tolist() == [3, 4] and str(z["wind"]) == 'NE'
    assert z["names"].tolist() == list(c.biomes.names) and int(z["ocean"]) == 0
    hand_made(discharge=None, effective_area=None).save(str(tmp_path / "p"))
    assert sorted(f.name for f in tmp_path.iterdir() if f.name.startswith("p.")) == ["p.biome.npy", "p.rain.npy", "p.temperature.npy"]
    assert np.array_equal(np.load(str(tmp_path / "p.rain.npy")), c.rain) and np.load(str(tmp_path / "p.temperature.npy")).dtype == np.int32


def test_regions_biomes():
    c = hand_made()
    labels = RG.biomes(c)
    assert labels.dtype == np.int32 and labels.tolist() == [[-1, -1, 3, 3], [-1, 5, 5, 7], [4, 4, 4, 7]]
    assert np.array_equal(c.biome, hand_made().biome)                     # the climate's plane is untouched
    for bad in (hand_made(biome=None), c.biome, None):
        with pytest.raises(ValueError, match="Climate that kept 'biome'"):
            RG.biomes(bad)
    assert "biomes" in RG.__all__


# ---- analyse and paint over the fake device ----------------------------------------------------------------------------------------------
def recording(fail=None):
    from tests.fake_device import RecordingOps
    from tests.test_contour_host import Counting

    class Ops(RecordingOps):
        def climate_workspace(self, H, W):
            return 256 + 24 * H * W

        def climate_discharge(self, *args):
            self.calls.append(("climate_discharge", args, {}))
            return 7

        def __getattr__(self, name):
            rec = RecordingOps.__getattr__(self, name)
            if name == fail:
                def boom(*a, **k):
                    raise RuntimeError("the launch failed")
                return boom
            return rec

    return Ops(Counting())


def test_analyse_sends_its_launches_inside_one_scratch():
    h = R.case("37x70")
    H, W = h.shape
    ops = recording()
    w = CL.Weather(wind='SE', latitude=0.01)
    got = CL.analyse(ops, h, w, origin=(-5, 9), form='staged')
    assert ops.dev.live == 0 and ops.dev.sizes == [4 * H * W] * 5
    assert [c[0] for c in ops.calls] == ["climate_transport", "climate_spread", "climate_biome"]
    q = w.quantised()
    t = ops.calls[0][1]
    assert t[1:5] == (W, H, W, 3) and t[5] == 1 and t[6:12] == (q["sea_q"], q["hum_q"], q["evap_q"], q["base_q"], q["up_q"], q["rec_q"]) and t[13] == W
    assert ops.calls[1][1][1:5] == (W, H, W, 1) and ops.calls[2][1][10] == -5
    assert got.shape == (H, W) and got.origin == (-5, 9) and got.form == 'staged' and got.discharge is None and got.raw is None
    assert got.rain.dtype == np.uint32 and got.temperature.dtype == np.int32 and got.biome.dtype == np.int32 and got.rain.shape == (H, W)
    assert CL.analyse(ops, h).form == CL.DEFAULT_FORM and CL.analyse(ops, h, keep=('raw',)).rain is None
    # with a hydrology: the directions go up, the discharge runs in the same scratch
    ops = recording()
    hydro = HY.Hydrology((H, W), (1, 1), 1, True, direction=np.full((H, W), -1, np.int8))
    got = CL.analyse(ops, h[None], hydro=hydro)
    assert ops.dev.live == 0 and ops.dev.sizes[5:] == [H * W, 8 * H * W, 4 * H * W, 256 + 24 * H * W] and got.rounds == 7
    assert [c[0] for c in ops.calls][-1] == "climate_discharge" and ops.calls[-1][1][6] == q["ref_q"]
    assert got.discharge.dtype == np.uint64 and got.effective_area.dtype == np.uint32
    assert (np.asarray(h * 255, np.uint8).shape == (H, W)) and CL.analyse(recording(), np.asarray(h * 255, np.uint8)).shape == (H, W)


@pytest.mark.parametrize("fail", ["climate_transport", "climate_spread", "climate_biome"])
def test_analyse_frees_its_scratch_when_a_launch_fails(fail):
    ops = recording(fail)
    with pytest.raises(RuntimeError, match="the launch failed"):
        CL.analyse(ops, R.case("9x1"))
    assert ops.dev.live == 0 and len(ops.dev.sizes) == 5


def test_refusals_before_the_device_is_touched():
    ops = None
    h = R.case("flat")
    for kw, match in ((dict(weather="wet"), "Weather"), (dict(biomes=3), "Biomes"), (dict(origin=(1,)), "origin"), (dict(origin=(1.5, 0)), "origin"),
                      (dict(origin=((1 << 31) + 1, 0)), "origin"), (dict(form='tiled'), "form"), (dict(form=1), "form"), (dict(keep=('snow',)), "keep"),
                      (dict(hydro="h"), "Hydrology"), (dict(hydro=HY.Hydrology(h.shape, (1, 1), 1, True)), "kept 'direction'"),
                      (dict(hydro=HY.Hydrology((2, 2), (1, 1), 1, True, direction=np.zeros((2, 2), np.int8))), "heightmap's size")):
        with pytest.raises(ValueError, match=match):
            CL.analyse(ops, h, **kw)
    for bad in (h * 3, h[0], np.zeros((2, 3, 4), np.float32), h.astype(np.int32), np.full((2, 2), np.nan, np.float32)):
        with pytest.raises(ValueError):
            CL.analyse(ops, bad)
    c = hand_made()
    tex = np.zeros((3, 4, 3), np.uint8)
    for args, match in (((tex, "c"), "Climate that kept"), ((tex, hand_made(biome=None)), "Climate that kept"), ((tex, c, 1.5), "opacity"),
                        ((np.zeros((4, 4, 3), np.uint8), c), "differ in size")):
        with pytest.raises(ValueError, match=match):
            CL.paint(ops, *args)


def test_the_paint_sends_the_charts_palette():
    ops = recording()
    c = hand_made()
    tex = np.zeros((3, 4, 3), np.uint8)
    out = CL.paint(ops, tex, c, 0.25)
    assert out.shape == (3, 4, 3) and out.dtype == np.uint8 and ops.dev.live == 0 and len(ops.dev.sizes) == 3
    name, args, _ = ops.calls[0]
    assert name == "climate_paint" and args[1:4] == (4, 3, 4) and args[5:7] == (4, 3) and args[8] == 0.25 and args[9] is True
    pal = args[7]
    assert pal.shape == (12, 4) and pal.dtype == np.float32 and (pal[:, 3] == 1).all()
    assert np.array_equal(pal[:, :3], np.array(c.biomes.colours, np.float32))       # a uint8 texture is painted in [0, 1]
    # a float texture of three channels is in the tanh range; a biome without a colour has no row
    import dataclasses
    some = dataclasses.replace(c.biomes, colours=(None,) * 11 + ((1.0, 0.5, 0.0),))
    ops = recording()
    CL.paint(ops, np.zeros((3, 3, 4), np.float32), CL.Climate((3, 4), (0, 0), CL.Weather(), some, biome=c.biome))
    pal = ops.calls[0][1][7]
    assert (pal[:11] == 0).all() and pal[11].tolist() == [1.0, np.float32((127.5 - 127.5) / 127.5), -1.0, 1.0] and ops.calls[0][1][9] is False


# ---- the command lines -------------------------------------------------------------------------------------------------------------------
def test_command_line_parsing(capsys):
    a = CL.parse_args(["in.png", "out"])
    assert (a.input, a.out_prefix, a.weather, a.hydrology, a.texture, a.painted, a.opacity, a.form) == ("in.png", "out", CL.Weather(), False, None,
                                                                                                     None, 0.6, None)
    a = CL.parse_args(["in.npy", "o.npz", "--wind", "NE", "--sea-level", "0.4", "--humidity", "0.9", "--evaporation", "0.1", "--drizzle", "0.03",
                       "--uplift", "2", "--recycle", "0.5", "--spread", "4", "--sea-temperature", "-3.5", "--lapse", "1", "--latitude=-0.01",
                       "--reference-rain", "0.02", "--height-scale", "32", "--hydrology", "--texture", "t.png", "--painted", "p.png",
                       "--opacity", "0.3", "--staged"])
    assert a.weather == CL.Weather('NE', 0.4, 0.9, 0.1, 0.03, 2.0, 0.5, 4, -3.5, 1.0, -0.01, 0.02, 32.0)
    assert (a.hydrology, a.texture, a.painted, a.opacity, a.form) == (True, "t.png", "p.png", 0.3, "staged")
    assert CL.parse_args(["i", "o", "--line"]).form == "line"
    for bad, match in ((["i"], "required"), (["i", "o", "--wind", "up"], "wind must be one of"), (["i", "o", "--sea-level", "2"], "sea_level"),
                       (["i", "o", "--humidity", "-1"], "humidity"), (["i", "o", "--evaporation", "2"], "evaporation"),
                       (["i", "o", "--drizzle", "2"], "drizzle"), (["i", "o", "--uplift", "17"], "uplift"), (["i", "o", "--recycle", "2"], "recycle"),
                       (["i", "o", "--spread", "9"], "spread"), (["i", "o", "--spread", "1.5"], "invalid int"),
                       (["i", "o", "--sea-temperature", "200"], "sea_temperature"), (["i", "o", "--lapse", "-1"], "lapse"),
                       (["i", "o", "--latitude", "2"], "latitude"), (["i", "o", "--reference-rain", "0"], "reference_rain"),
                       (["i", "o", "--height-scale", "0"], "height_scale"), (["i", "o", "--texture", "t.png"], "go together"),
                       (["i", "o", "--painted", "p.png"], "go together"), (["i", "o", "--opacity", "0.5"], "goes with --painted"),
                       (["i", "o", "--texture", "t", "--painted", "p", "--opacity", "2"], "opacity"), (["i", "o", "--line", "--staged"], "not allowed with"),
                       (["i", "o", "--snow"], "unrecognized")):
        with pytest.raises(SystemExit):
            CL.parse_args(bad)
        assert match in capsys.readouterr().err, bad


def test_the_worlds_command_line_takes_the_climate(capsys):
    from gan_heightmaps_amd import world as WD
    base = ["exp", "model.npz", "out.png", "--seed", "3", "--region", "-70,33,150,97"]
    a = WD.parse_args(base)
    assert a.climate is None and a.wind is None
    a = WD.parse_args(base + ["--climate", "c"])
    assert a.climate == "c" and a.weather == CL.Weather()
    a = WD.parse_args(base + ["--climate", "c.npz", "--wind", "SE", "--sea-level", "0.4"])
    assert a.weather == CL.Weather(wind='SE', sea_level=0.4)
    a = WD.parse_args(base + ["--climate", "c", "--sea-level", "0.4", "--regions", "r.svg", "--of", "land"])
    assert a.weather.sea_level == 0.4 and a.of == "land" and a.sea_level == 0.4
    assert WD.parse_args(base + ["--climate", "c", "--sea-level", "0.4", "--regions", "r.svg", "--of", "lakes"]).of == "lakes"
    for bad, match in ((["--wind", "N"], "--wind needs --climate"), (["--climate", "c", "--wind", "X"], "wind must be one of"),
                       (["--climate", "c", "--sea-level", "3"], "sea_level"), (["--sea-level", "0.4"], "need --regions"),
                       (["--regions", "r.svg", "--of", "lakes", "--sea-level", "0.4"], "go together"),
                       (["--climate", "c", "--regions", "r.svg", "--of", "land"], "go together")):
        with pytest.raises(SystemExit):
            WD.parse_args(base + bad)
        assert match in capsys.readouterr().err, bad


# ---- the transport kernels' source on the host -------------------------------------------------------------------------------------------
def _build(d, name, extra=()):
    import os
    import subprocess
    from tests.test_render_host import CSRC, ROOT, _compiler
    head, sep, _ = open(os.path.join(CSRC, "climate.hip")).read().partition("#define CLM_PLANE_GRID")
    assert sep and '#include "common.h"' in head and '#include "relax.h"' in head
    inc = d / "climate.hip.inc"
    inc.write_text(head.replace('#include "common.h"', "").replace('#include "relax.h"', "") + "}  // namespace\n")
    exe = d / name
    cmd = [_compiler(), "-x", "c++", "-std=c++17", "-O1", "-pthread", "-I", os.path.join(ROOT, "include"),
           '-DCLIMATE_DEVICE_INC="%s"' % inc] + list(extra) + [os.path.join(ROOT, "tests", "climate_host", "harness.cpp"), "-o", str(exe)]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


def run_transport(d, exe, name, wind, form):
    """raw of a case through the host build: the heights in rows of W + 3 cells with a mountain in the padding, raw in rows of
    W + 3 cells whose padding must come back untouched"""
    import subprocess
    zq = R.quantise(R.case(name))
    H, W = zq.shape
    wide = np.full((H, W + 3), 1 << 22, np.int32)
    wide[:, :W] = zq
    (d / "in.bin").write_bytes(wide.tobytes())
    q = CL.Weather(wind=wind).quantised()
    args = [H, W, q['wind'], CL.FORMS.index(form), q['sea_q'], q['hum_q'], q['evap_q'], q['base_q'], q['up_q'], q['rec_q'], d / "in.bin", d / "out.bin"]
    r = subprocess.run([str(exe)] + [str(v) for v in args], capture_output=True, text=True)
    assert r.returncode == 0, (name, wind, form, r.returncode, r.stderr[-3000:])
    got = np.frombuffer((d / "out.bin").read_bytes(), np.uint32).reshape(H, W + 3)
    assert (got[:, W:] == 0xABABABAB).all(), "cells beyond a row's width were written"
    return got[:, :W]


def test_both_forms_on_the_host_build_under_the_sanitizers(tmp_path):
    """the device source of both transport forms as a stand-alone program with -fsanitize=address,undefined, a host thread per lane
    and a barrier for __syncthreads, run as a child process: an index past a plane or a tile and signed overflow in the recurrence end
    it.  The cases with unequal diagonals, the one that crosses both tile edges, a coast and a row, under every wind"""
    import subprocess
    from tests.test_render_host import _compiler
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    # only a compiler that cannot build and run an empty program with the sanitizers is a reason to skip
    (tmp_path / "empty.cpp").write_text("int main() { return 0; }\n")
    probe = subprocess.run([_compiler(), "-x", "c++"] + flags + [str(tmp_path / "empty.cpp"), "-o", str(tmp_path / "empty")],
                           capture_output=True, text=True)
    if probe.returncode != 0 or subprocess.run([str(tmp_path / "empty")]).returncode != 0:
        pytest.skip("the host compiler cannot link the sanitizer runtimes: " + probe.stderr[-300:])
    exe, r = _build(tmp_path, "climate_host_san", flags)
    assert r.returncode == 0, r.stderr[-3000:]
    for name in ("37x70", "65x130", "coast", "1x9"):
        for wind in R.WINDS:
            want = R.expected(name, wind)["raw"]
            for form in CL.FORMS:
                assert np.array_equal(run_transport(tmp_path, exe, name, wind, form), want), (name, wind, form)
