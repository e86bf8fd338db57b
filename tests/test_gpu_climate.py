"""The climate on the MI355X (csrc/climate.hip, gan_heightmaps_amd/climate.py): the transport in both forms, the spread,
temperature and biome, the discharge and the palette paint through the raw entry points against tests/climate_ref.py bit for bit -- the
definition is integer, so there are no tolerances.  Inputs go in with a pitch of W + 3 whose padding holds values that would change the
answer if read; outputs lie in canary canvases; the workspace is followed by canary bytes.  Then ``analyse``, the paint, the model's and
the world's methods, the command line, and the refusals of the raw entry points."""
import numpy as np
import pytest

from oracle import step as ostep
from gan_heightmaps_amd import climate as CL
from gan_heightmaps_amd import hydrology as HY
from gan_heightmaps_amd import regions as RG
from tests import climate_ref as R
from tests.gpu_common import build_model, CANARY, Canvas, dev, model_params, ops, padded, same, SMALL      # noqa: F401  (dev, ops: the fixtures)

pytestmark = pytest.mark.gpu

TAIL = 64                    # canary bytes behind the workspace
HIGH = 1 << 22               # a height in the padding: read as a neighbour it would lift the air, read as a cell it would be land


def raw_climate(dev, ops, h, weather, form, biomes=None, origin_row=0):
    """raw, rain, temperature and biome of a heightmap through the raw entry points"""
    biomes = CL.Biomes() if biomes is None else biomes
    q = weather.quantised()
    zq = R.quantise(h, weather.height_scale)
    H, W = zq.shape
    bufs = []
    try:
        d_z, pz = padded(dev, zq, np.int32, 3, HIGH)
        bufs.append(d_z)
        raw, rain, temp, biome = (Canvas(dev, H, W, dt) for dt in (np.uint32, np.uint32, np.int32, np.int32))
        bufs += [c.base for c in (raw, rain, temp, biome)]
        ops.climate_transport(d_z, pz, H, W, q['wind'], CL.FORMS.index(form), q['sea_q'], q['hum_q'], q['evap_q'], q['base_q'], q['up_q'],
                              q['rec_q'], raw.ptr, raw.pitch)
        ops.climate_spread(raw.ptr, raw.pitch, H, W, q['spread'], rain.ptr, rain.pitch)
        ops.climate_biome(d_z, pz, rain.ptr, rain.pitch, H, W, q['sea_q'], q['t0_q'], q['lapse_q'], q['lat_q'], origin_row,
                          *biomes.quantised(), biomes.ocean, temp.ptr, temp.pitch, biome.ptr, biome.pitch)
        dev.sync()
        return dict(raw=raw.read(), rain=rain.read(), temperature=temp.read(), biome=biome.read())
    finally:
        dev.sync()
        for b in bufs:
            dev.free(b)


# ---- 1. every case under every wind, in both forms ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("wind", R.WINDS)
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_every_plane_equals_the_restatement(dev, ops, name, wind):
    want = R.expected(name, wind)
    got = {form: raw_climate(dev, ops, R.case(name), CL.Weather(wind=wind), form) for form in CL.FORMS}
    for form in CL.FORMS:
        for k in ("raw", "rain", "temperature", "biome"):
            assert same(got[form][k], want[k]), (name, wind, form, k)
    assert same(got['line']['raw'], got['staged']['raw'])
    if name == "all_sea":
        assert (want["biome"] == 0).all()
    if name in ("37x70", "65x130"):
        assert len(np.unique(want["biome"])) >= 3 and want["raw"].max() > want["raw"].min()


def test_other_weather_and_another_chart(dev, ops):
    """the extremes of the parameters, a wide spread, a latitude with a far origin, a chart of one edge"""
    h = R.case("70x37")
    two = CL.Biomes(temperature_edges=(3.0,), rain_edges=(), table=((1,), (2,)), names=("sea", "cold", "warm"), colours=(None, None, None), ocean=0)
    for weather, biomes, row in ((CL.Weather('NE', 0.4, 1.0, 1.0, 1.0, 16.0, 1.0, 8, -100.0, 16.0, -1.0, 1.0, 65536.0), None, -(1 << 31)),
                                 (CL.Weather('S', 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 100.0, 0.0, 1.0, 1e-9, 1.0), None, 1 << 31),
                                 (CL.Weather('E', 0.5, 0.7, 0.3, 0.1, 0.5, 0.9, 3, 10.0, 0.3, 0.013, 0.01, 20.0), two, 12345)):
        want = R.definition(h, weather, CL.Biomes() if biomes is None else biomes, origin_row=row)
        for form in CL.FORMS:
            got = raw_climate(dev, ops, h, weather, form, biomes, row)
            for k in ("raw", "rain", "temperature", "biome"):
                assert same(got[k], want[k]), (weather.wind, form, k)


# ---- 2. the discharge --------------------------------------------------------------------------------------------------------------------
def raw_discharge(dev, ops, direction, rain, ref_q):
    H, W = rain.shape
    bufs = []
    try:
        d_d, pd = padded(dev, direction, np.int8, 3, 2)                    # (a direction in the padding would point back into the plane)
        d_r, pr = padded(dev, rain, np.uint32, 3, 0xffffffff)
        q, e = Canvas(dev, H, W, np.uint64), Canvas(dev, H, W, np.uint32)
        nbytes = ops.climate_workspace(H, W)
        whole = np.full(nbytes + TAIL, CANARY, np.uint8)
        d_w = dev.alloc(whole.nbytes)
        bufs += [d_d, d_r, q.base, e.base, d_w]
        dev.h2d(d_w, whole)
        rounds = ops.climate_discharge(d_d, pd, d_r, pr, H, W, ref_q, q.ptr, q.pitch, e.ptr, e.pitch, d_w)
        dev.sync()
        dev.d2h(whole, d_w, whole.nbytes)
        assert (whole[nbytes:] == CANARY).all(), "bytes behind the workspace were written"
        return q.read(), e.read(), rounds
    finally:
        dev.sync()
        for b in bufs:
            dev.free(b)


@pytest.mark.parametrize("name", ["37x70", "65x130", "coast", "1x9", "1x1"])
def test_the_discharge_equals_the_ordered_sum(dev, ops, name):
    h = R.case(name)
    hydro = HY.analyse(ops, h, keep=('direction', 'accumulation'))
    ref_q = CL.Weather().quantised()['ref_q']
    rain = R.expected(name, 'W')["rain"]
    want_q, want_e = R.discharge(hydro.direction, rain, ref_q)
    got_q, got_e, rounds = raw_discharge(dev, ops, hydro.direction, rain, ref_q)
    assert same(got_q, want_q) and same(got_e, want_e) and rounds == hydro.rounds
    # reference rain everywhere: the drainage area itself
    got_q, got_e, _ = raw_discharge(dev, ops, hydro.direction, np.full(h.shape, ref_q, np.uint32), ref_q)
    assert same(got_e, hydro.accumulation) and same(got_q, hydro.accumulation.astype(np.uint64) * np.uint64(ref_q))
    # weights near 2^32: sums past 32 bits, and an effective area that saturates
    heavy = (np.uint32(0xffffffff) - rain).astype(np.uint32)
    want_q, want_e = R.discharge(hydro.direction, heavy, 1)
    got_q, got_e, _ = raw_discharge(dev, ops, hydro.direction, heavy, 1)
    assert same(got_q, want_q) and same(got_e, want_e)
    if min(h.shape) > 2:                                                   # (a plane of border cells alone drains nowhere)
        assert int(hydro.accumulation.max()) > 1 and int(want_q.max()) > 1 << 32 and int(want_e.max()) == (1 << 32) - 1


def test_directions_with_a_cycle_are_refused(dev, ops):
    from gan_heightmaps_amd._lib import GhmError
    direction = np.full((4, 5), -1, np.int8)
    direction[1, 1], direction[1, 2] = 2, 6                                # east, and back west
    with pytest.raises(GhmError, match="no forest"):
        raw_discharge(dev, ops, direction, np.ones((4, 5), np.uint32), 1)


# ---- 3. analyse, the paint, the model's methods -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_model(dev):
    m = build_model(ostep.default_cfg(**SMALL), 5, dev, dtype="f32", use_graph=False)
    cfg = ostep.default_cfg(**SMALL)
    for s in range(3):                       # non-trivial BatchNorm running statistics (the deterministic pass reads them)
        m.z_fn(ostep.synthetic_batch(4, cfg, seed=40 + s)[0])
    return m


def same_climate(got, want, hydro=None, ref_q=None):
    for k in ("raw", "rain", "temperature", "biome"):
        if getattr(got, k) is not None:
            assert same(getattr(got, k), want[k]), k
    if hydro is not None:
        q, e = R.discharge(hydro.direction, want["rain"], ref_q)
        assert same(got.discharge, q) and same(got.effective_area, e)
    return True


def test_analyse_equals_the_definition(dev, ops):
    h = R.case("65x130")
    weather = CL.Weather(wind='SW', latitude=0.02, spread=2)
    want = R.definition(h, weather, CL.Biomes(), origin_row=-300)
    hydro = HY.analyse(ops, h)
    for form in CL.FORMS:
        got = CL.analyse(ops, h, weather, origin=(-300, 7), hydro=hydro, form=form, keep=CL.PLANES)
        assert same_climate(got, want, hydro, weather.quantised()['ref_q']) and got.form == form and got.origin == (-300, 7)
        assert got.rounds == hydro.rounds and got.shape == h.shape
    plain = CL.analyse(ops, (h * 255).astype(np.uint8)[None])             # the uint8 intake, the lead axis, the defaults
    u8 = (h * 255).astype(np.uint8).astype(np.float32) / np.float32(255)
    assert same_climate(plain, R.definition(u8, CL.Weather(), CL.Biomes())) and plain.raw is None and plain.discharge is None
    assert plain.form == CL.DEFAULT_FORM and abs(sum(plain.share().values()) - 1) < 1e-9
    # the effective area in the hydrology's place: what rivers, paint and channels read
    wet = got.hydrology(hydro)
    assert same(wet.accumulation, got.effective_area) and wet.direction is hydro.direction and not same(wet.accumulation, hydro.accumulation)
    labels = RG.biomes(got)
    assert (labels[want["biome"] == 0] == -1).all() and len(RG.regions(ops, labels)) >= 3


def blend(tex, biome, chart, opacity):
    """the numpy blend of a uint8 (H, W, 3) texture: float32 t + opacity (colour - t), each step rounded, then rint(v 255) half to even"""
    t = tex.astype(np.float32) / np.float32(255)
    out = tex.copy()
    on = np.zeros(biome.shape, bool)
    for k, colour in enumerate(chart.colours):
        if colour is None:
            continue
        m = biome == k
        on |= m
        c = np.asarray(colour, np.float32)
        d = (c[None, :] - t[m]).astype(np.float32)
        v = (t[m] + (np.float32(opacity) * d).astype(np.float32)).astype(np.float32)
        out[m] = np.rint(np.clip(v, 0, 1).astype(np.float64) * 255.0).astype(np.uint8)
    return out, on


def test_the_models_methods_and_the_paint(small_model, dev, ops):
    import dataclasses
    m = small_model
    before = model_params(m)
    h = R.case("37x70")
    weather = CL.Weather(wind='NW')
    want = R.expected("37x70", 'NW')
    c = m.heightmap_climate(h, weather, form='staged')
    assert same_climate(c, want) and c.discharge is None
    hydro = HY.analyse(ops, h)
    for arg in (True, hydro):
        c = m.heightmap_climate(h, weather, hydrology=arg)
        assert same_climate(c, want, hydro, weather.quantised()['ref_q'])
    tex = np.random.RandomState(3).randint(0, 256, h.shape + (3,)).astype(np.uint8)
    some = dataclasses.replace(c.biomes, colours=tuple(col if k % 2 else None for k, col in enumerate(c.biomes.colours)))
    for chart, opacity in ((c.biomes, 0.6), (some, 1.0), (some, 0.0)):
        cc = CL.Climate(c.shape, c.origin, c.weather, chart, biome=c.biome)
        expect, on = blend(tex, c.biome, chart, opacity)
        painted = m.paint_biomes(tex, cc, opacity)
        assert painted.dtype == np.uint8 and same(painted, expect) and same(painted[~on], tex[~on]) and on.any()
    assert not on.all()                                                    # some pixels had no colour, and kept their bits
    ftex = np.random.RandomState(4).rand(3, *h.shape).astype(np.float32) * 2 - 1
    fp = CL.paint(ops, ftex, CL.Climate(c.shape, c.origin, c.weather, some, biome=c.biome), 0.5)
    assert same(fp[:, ~on], ftex[:, ~on]) and (fp[:, on] != ftex[:, on]).any() and fp.dtype == np.float32
    after = model_params(m)
    for k in before:
        for x, y in zip(before[k], after[k]):
            assert np.array_equal(x, y), k


@pytest.mark.parametrize("u8", [False, True])
def test_the_raw_paint_inside_canaries(dev, ops, u8):
    """one channel through the raw entry point: labels and texture pitched W + 3, the padding a painted biome and another grey"""
    biome = R.expected("37x70", 'N')["biome"]
    H, W = biome.shape
    t = np.random.RandomState(9).rand(H, W).astype(np.float32)
    pal = np.zeros((12, 4), np.float32)
    for k in (3, 4, 5, 7):
        pal[k] = (0.1 * k, 0.0, 0.0, 1.0)
    bufs = []
    try:
        d_b, pb = padded(dev, biome, np.int32, 3, 4)
        d_t, pt = padded(dev, t, np.float32, 3, 0.5)
        out = Canvas(dev, H, W, np.uint8 if u8 else np.float32)
        bufs += [d_b, d_t, out.base]
        ops.climate_paint(d_b, pb, H, W, d_t, pt, 1, pal, 0.75, u8, out.ptr, out.pitch)
        dev.sync()
        got = out.read()
    finally:
        dev.sync()
        for b in bufs:
            dev.free(b)
    on = np.isin(biome, (3, 4, 5, 7))
    c = pal[np.clip(biome, 0, 11), 0]
    v = (t + (np.float32(0.75) * (c - t).astype(np.float32)).astype(np.float32)).astype(np.float32)
    want = np.where(on, v, t)
    if u8:
        want = np.rint(np.clip(want, 0, 1).astype(np.float64) * 255.0).astype(np.uint8)
    assert same(got, want) and on.any() and not on.all()


# ---- 4. the world -----------------------------------------------------------------------------------------------------------------------
def test_the_worlds_climate(small_model, dev, ops):
    from tests.gpu_common import ERO
    m = small_model
    weather = CL.Weather(wind='E', latitude=0.05, sea_level=0.45)
    with m.terrain_world(42, chunk_cells=2, erosion=ERO) as world:
        a = world.climate(-20, 10, 70, 90, weather, hydrology=True)
        b = world.climate(5, 40, 60, 80, weather)
        for c, (y0, x0, hh, ww) in ((a, (-20, 10, 70, 90)), (b, (5, 40, 60, 80))):
            hm = world._unit_height(y0, x0, hh, ww)
            assert c.origin == (y0, x0) and c.shape == (hh, ww)
            assert same_climate(c, R.definition(hm, weather, CL.Biomes(), origin_row=y0))
            direct = CL.analyse(ops, hm, weather, origin=(y0, x0))
            for k in ("rain", "temperature", "biome"):
                assert same(getattr(c, k), getattr(direct, k)), k
        # the overlap: world rows 5 .. 50, columns 40 .. 100
        assert same(a.temperature[25:70, 30:90], b.temperature[0:45, 0:60]) and len(np.unique(a.temperature[:, 0])) > 10
        assert a.discharge is not None and a.effective_area.dtype == np.uint32 and b.discharge is None
        hydro = world.hydrology(-20, 10, 70, 90, keep=('direction',))
        q, e = R.discharge(hydro.direction, a.rain, weather.quantised()['ref_q'])
        assert same(a.discharge, q) and same(a.effective_area, e)


# ---- 5. the command line ---------------------------------------------------------------------------------------------------------------
def test_command_line_end_to_end(ops, tmp_path, capsys):
    from gan_heightmaps_amd.util import read_image, save_png
    h = R.case("37x70")
    np.save(str(tmp_path / "h.npy"), h)
    tex = np.random.RandomState(3).randint(0, 256, h.shape + (3,)).astype(np.uint8)
    save_png(str(tmp_path / "t.png"), tex)
    args = [str(tmp_path / "h.npy"), str(tmp_path / "o"), "--wind", "SE", "--spread", "2", "--hydrology", "--staged",
            "--texture", str(tmp_path / "t.png"), "--painted", str(tmp_path / "p.png"), "--opacity", "1"]
    assert CL.main(args) == 0
    weather = CL.Weather(wind='SE', spread=2)
    want = R.definition(h, weather, CL.Biomes())
    assert capsys.readouterr().out.startswith("wind SE, 37 x 70: ")
    for k in ("rain", "temperature", "biome"):
        assert same(np.load(str(tmp_path / ("o.%s.npy" % k))), want[k]), k
    hydro = HY.analyse(ops, h, keep=('direction',))
    q, e = R.discharge(hydro.direction, want["rain"], weather.quantised()['ref_q'])
    assert same(np.load(str(tmp_path / "o.discharge.npy")), q) and same(np.load(str(tmp_path / "o.effective_area.npy")), e)
    expect, _ = blend(tex, want["biome"], CL.Biomes(), 1.0)
    assert same(read_image(str(tmp_path / "p.png")), expect)
    assert CL.main([str(tmp_path / "h.npy"), str(tmp_path / "o.npz")]) == 0
    z = np.load(str(tmp_path / "o.npz"))
    assert same(z["biome"], R.expected("37x70", 'W')["biome"]) and "discharge" not in z.files


# ---- 6. refusals of the raw entry points ----------------------------------------------------------------------------------------------
def test_refusals_of_the_entry_points(dev, ops):
    from gan_heightmaps_amd._lib import GhmError
    H, W = 9, 13
    n = H * W
    outs = [np.full(8 * n, CANARY, np.uint8) for _ in range(4)]
    d_o = [dev.alloc(o.nbytes) for o in outs]
    d_z, d_r, d_d, d_t = dev.alloc(4 * n), dev.alloc(4 * n), dev.alloc(n), dev.alloc(12 * n)
    d_w = dev.alloc(ops.climate_workspace(H, W))
    try:
        for p, o in zip(d_o, outs):
            dev.h2d(p, o)
        dev.h2d(d_z, R.quantise(R.case("flat")))
        dev.h2d(d_r, np.ones(n, np.uint32))
        dev.h2d(d_d, np.full(n, -1, np.int8))
        dev.h2d(d_t, np.zeros(3 * n, np.float32))
        assert ops.climate_workspace(0, 5) == -1 and ops.climate_workspace(1 << 16, 1 << 15) == -1 and ops.climate_workspace(4 * 65535 + 1, 1) == -1
        assert ops.climate_workspace(1, 9) >= 24 * 9
        big = dict(Hh=1 << 16, Ww=1 << 15, pz=1 << 15, po=1 << 15)

        def transport(z=d_z, pz=W, Hh=H, Ww=W, wind=6, form=0, sea=0, hum=100, evap=100, base=100, up=100, rec=100, o=d_o[0], po=W):
            ops.climate_transport(z, pz, Hh, Ww, wind, form, sea, hum, evap, base, up, rec, o, po)

        for kw, match in ((dict(z=None), "null"), (dict(o=None), "null"), (dict(pz=W - 1), "pitch"), (dict(po=W - 1), "pitch"), (dict(Hh=0), "out of range"),
                          (big, "out of range"), (dict(wind=8), "wind"), (dict(wind=-1), "wind"), (dict(form=2), "form"), (dict(form=-1), "form"),
                          (dict(hum=65537), "hum_q"), (dict(hum=-1), "hum_q"), (dict(evap=65537), "evap_q"), (dict(base=-1), "base_q"),
                          (dict(rec=65537), "rec_q"), (dict(up=(1 << 20) + 1), "up_q"), (dict(up=-1), "up_q")):
            with pytest.raises(GhmError, match=match):
                transport(**kw)

        def spread(r=d_r, pr=W, Hh=H, Ww=W, s=1, o=d_o[1], po=W):
            ops.climate_spread(r, pr, Hh, Ww, s, o, po)

        for kw, match in ((dict(r=None), "null"), (dict(o=None), "null"), (dict(pr=W - 1), "pitch"), (dict(po=W - 1), "pitch"), (dict(Ww=0), "out of range"),
                          (dict(s=9), "spread"), (dict(s=-1), "spread"), (dict(o=d_r), "may not be raw")):
            with pytest.raises(GhmError, match=match):
                spread(**kw)

        def biome(z=d_z, pz=W, r=d_r, pr=W, Hh=H, Ww=W, sea=0, t0=0, lapse=0, lat=0, row=0, te=(0,), re_=(5,), tb=(1, 2, 3, 4), ocean=0, t=d_o[2], pt=W,
                  b=d_o[3], pb=W):
            ops.climate_biome(z, pz, r, pr, Hh, Ww, sea, t0, lapse, lat, row, te, re_, tb, ocean, t, pt, b, pb)

        for kw, match in ((dict(z=None), "null"), (dict(r=None), "null"), (dict(t=None), "null"), (dict(b=None), "null"), (dict(pz=W - 1), "pitch"),
                          (dict(pr=W - 1), "pitch"), (dict(pt=W - 1), "pitch"), (dict(pb=W - 1), "pitch"), (dict(Hh=-1), "out of range"),
                          (dict(t0=25601), "t0_q"), (dict(t0=-25601), "t0_q"), (dict(lapse=-1), "lapse_q"), (dict(lapse=(1 << 20) + 1), "lapse_q"),
                          (dict(lat=(1 << 24) + 1), "lat_q"), (dict(lat=-(1 << 24) - 1), "lat_q"), (dict(row=(1 << 31) + 1), "origin_row"),
                          (dict(row=-(1 << 31) - 1), "origin_row"), (dict(te=tuple(range(9)), tb=tuple(range(1, 21))), "edges"),
                          (dict(te=(1, 1), tb=(1,) * 6), "do not ascend"), (dict(re_=(2, 1), tb=(1,) * 6), "do not ascend"), (dict(re_=(-1,)), "negative"),
                          (dict(ocean=-1), "ocean"), (dict(tb=(1, 2, -3, 4)), "table")):
            with pytest.raises(GhmError, match=match):
                biome(**kw)
        with pytest.raises(ValueError, match="the table has"):
            biome(tb=(1, 2, 3))

        def discharge(d=d_d, pd=W, r=d_r, pr=W, Hh=H, Ww=W, ref=1, q=d_o[0], pq=W, e=d_o[1], pe=W, w=d_w):
            return ops.climate_discharge(d, pd, r, pr, Hh, Ww, ref, q, pq, e, pe, w)

        for kw, match in ((dict(d=None), "null"), (dict(r=None), "null"), (dict(q=None), "null"), (dict(e=None), "null"), (dict(w=None), "null"),
                          (dict(pd=W - 1), "pitch"), (dict(pr=W - 1), "pitch"), (dict(pq=W - 1), "pitch"), (dict(pe=W - 1), "pitch"),
                          (dict(Hh=0), "out of range"), (dict(ref=0), "ref_q"), (dict(ref=65537), "ref_q")):
            with pytest.raises(GhmError, match=match):
                discharge(**kw)

        pal = np.ones((3, 4), np.float32)

        def paint(b=d_z, pb=W, Hh=H, Ww=W, t=d_t, pt=W, ch=3, p=pal, op=0.5, u8=False, o=d_o[2], po=W):
            ops.climate_paint(b, pb, Hh, Ww, t, pt, ch, p, op, u8, o, po)

        for kw, match in ((dict(b=None), "null"), (dict(t=None), "null"), (dict(o=None), "null"), (dict(pb=W - 1), "pitch"), (dict(pt=W - 1), "pitches"),
                          (dict(po=W - 1), "pitches"), (dict(ch=2), "channels"), (dict(op=1.5), "opacity"), (dict(op=-0.5), "opacity"),
                          (dict(p=np.ones((65, 4), np.float32)), "colours"), (dict(p=np.full((3, 4), np.inf, np.float32)), "not finite"),
                          (dict(Hh=0), "out of range")):
            with pytest.raises(GhmError, match=match):
                paint(**kw)
        dev.sync()
        for p, o in zip(d_o, outs):                                        # no refusal has touched the outputs
            dev.d2h(o, p, o.nbytes)
            assert (o == CANARY).all()
        assert discharge() == 0                                            # and what they refused runs: no direction, no round
        dev.sync()
        dev.d2h(outs[0], d_o[0], outs[0].nbytes)
        assert (outs[0].view(np.uint64) == 1).all()
    finally:
        dev.sync()
        for b in d_o + [d_z, d_r, d_d, d_t, d_w]:
            dev.free(b)
