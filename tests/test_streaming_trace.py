"""The calls texture_heightmap, generate_terrain and a TerrainWorld request make on their contexts and ops, in host order,
against tests/golden/streaming_trace.json (tests/fake_device.py: trace_device_class, TraceEngine).  The fixture was recorded
with this file (``python -m tests.test_streaming_trace``) before the three pipelines were given one download ring
(gan_heightmaps_amd/streaming.py): the ring, the row layouts and the accumulator shift enqueue, wait and block exactly where
the hand-written copies did.  tests/golden/world_trace.json holds three more world cases -- an eroded and a plain world under
a budget so tight that chunks are evicted and made again inside a request, and requests into a scene's device planes --,
recorded the same way before TerrainWorld was given one chunk cache and one request form (with ``_scene_request`` in the
spelling of that tree): the one ``_acquire`` and ``_request(rect, sink)`` make the calls the two copies made.  No GPU."""
import json
import os

import numpy as np
import pytest

from gan_heightmaps_amd import device
from gan_heightmaps_amd import terrain as TR
from gan_heightmaps_amd import texture as TX
from tests.fake_device import TraceEngine
from tests.test_terrain_plan import SMALL, _gen
from tests.test_world_plan import _Model, _world

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "streaming_trace.json")
WORLD_FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "world_trace.json")


def _texture(o, u8):
    # 40 x 37 with T = 16: three tile rows of three tiles, so batch_size=2 leaves a partial last batch
    eng = TraceEngine(unet=(16, 1, 3) if u8 else (16, 3, 3))
    rng = np.random.RandomState(0)
    x = rng.randint(0, 256, (40, 37)).astype(np.uint8) if u8 else rng.rand(3, 40, 37).astype(np.float32)
    out = TX.texture_heightmap(eng, x, True, False, overlap=o, batch_size=2, uint8=u8)
    assert out.shape == ((40, 37, 3) if u8 else (3, 40, 37)) and out.dtype == (np.uint8 if u8 else np.float32)
    return eng


def _terrain(u8):
    eng = TraceEngine()
    gen = _gen(SMALL)
    assert len(TR.TerrainGeometry(gen, 3, 2, 1).windows) >= 3
    z = np.random.RandomState(1).randn(3, 2, SMALL['latent_dim']).astype(np.float32)
    out = TR.generate_terrain(eng, gen, SMALL['latent_dim'], None, True, z=z, band=1, uint8=u8)
    assert out.shape == ((96, 64) if u8 else (1, 96, 64))
    return eng


def _world_both(u8):
    eng = TraceEngine(unet=(32, 1, 3))
    model = _Model(_gen(SMALL), SMALL['latent_dim'])
    model.engine = eng
    from gan_heightmaps_amd import world as WD
    with WD.TerrainWorld(model, 42, chunk_cells=1) as world:
        assert world.chunk_px == 32                      # (-37, -21, 70, 50) touches 3 x 3 chunks and four tile rows
        hm, tex = world.both(-37, -21, 70, 50, uint8=u8)
    assert hm.shape == ((70, 50) if u8 else (1, 70, 50)) and tex.shape == ((70, 50, 3) if u8 else (3, 70, 50))
    return eng


def _traced_world(**kw):
    eng = TraceEngine(unet=(32, 1, 3))
    model = _Model(_gen(SMALL), SMALL['latent_dim'])
    model.engine = eng
    from gan_heightmaps_amd import world as WD
    return eng, WD.TerrainWorld(model, 42, chunk_cells=1, **kw)


def _world_tight(eroded):
    # chunks of 4 KB; eroded: a halo of 9 and room for 11 chunks, a window's nine raw chunks and little else, so raw chunks
    # are evicted and computed again in the middle of a request; plain: room for 3 of the 3 x 3 chunks the first request touches
    from gan_heightmaps_amd.erosion import Erosion
    kw = dict(erosion=Erosion(iterations=3), cache_mb=11 * 4 / 1024) if eroded else dict(cache_mb=3 * 4 / 1024)
    eng, world = _traced_world(**kw)
    with world:
        assert world.chunk_px == 32
        hm = world.heightmap(-37, -21, 70, 50)
        second = (world.heightmap if eroded else world.texture)(-5, 10, 40, 60, uint8=True)
        assert (world.computed, world.eroded) == ((74, 17) if eroded else (16, 0))
    assert hm.shape == (1, 70, 50) and second.shape == ((40, 60) if eroded else (40, 60, 3))
    return eng


def _scene_request(world, rect, hm, tex, flag):
    """one request into the device planes of a scene (the line that differs from the tree the fixture was recorded on)"""
    from gan_heightmaps_amd.world import _SceneSinks
    world._request(rect, _SceneSinks(hm_ptr=hm, tex_ptr=tex, flag_ptr=flag))


def _world_scene():
    eng, world = _traced_world()
    with world:
        world._bind()
        dev = world._dev
        hm, tex, flag = dev.alloc(4 * 70 * 50), dev.alloc(12 * 70 * 50), dev.alloc(4)
        _scene_request(world, (-37, -21, 70, 50), hm, tex, flag)
        grown = dev.alloc(4 * 76 * 56)
        _scene_request(world, (-40, -24, 76, 56), grown, None, flag)
        for p in (hm, tex, flag, grown):
            dev.free(p)
    return eng


WORLD_CASES = {"world-eroded-tight": lambda: _world_tight(True), "world-plain-tight": lambda: _world_tight(False),
               "world-scene": _world_scene}
CASES = {"texture-o0-u8": lambda: _texture(0, True), "texture-o4-u8": lambda: _texture(4, True),
         "texture-o0-f32": lambda: _texture(0, False), "texture-o4-f32": lambda: _texture(4, False),
         "terrain-f32": lambda: _terrain(False), "terrain-u8": lambda: _terrain(True),
         "world-f32": lambda: _world_both(False), "world-u8": lambda: _world_both(True)}
CASES.update(WORLD_CASES)


def _record(case):
    # the fixture's recording ran on a tree whose pipelines name device.PinnedArray itself: there, and wherever a pipeline
    # still does, the page-locked buffers are the tracing device's
    real = device.PinnedArray
    device.PinnedArray = lambda shape, dtype=np.float32: TraceEngine.current.Device.pinned_array(shape, dtype)
    try:
        eng = CASES[case]()
    finally:
        device.PinnedArray = real
    return {"log": eng.log, "tally": sorted([list(k) if isinstance(k, tuple) else [k], n] for k, n in eng.tally.items())}


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f, open(WORLD_FIXTURE) as g:
        return dict(json.load(f), **json.load(g))


@pytest.mark.parametrize("case", sorted(CASES))
def test_call_trace_is_the_recorded_one(case, golden):
    got = json.loads(json.dumps(_record(case)))
    want = golden[case]
    # (a scene's rows stay on the device: its sinks' kernels take the place of the downloads)
    assert len(want["log"]) > 20 and any(r[0] == ("world_scene_height" if case == "world-scene" else "d2h_async")
                                         for r in want["log"])
    for i, (g, w) in enumerate(zip(got["log"], want["log"])):
        assert g == w, "call %d: %r, recorded %r" % (i, g, w)
    assert len(got["log"]) == len(want["log"])
    assert got["tally"] == want["tally"]


if __name__ == "__main__":
    for path, cases in ((FIXTURE, set(CASES) - set(WORLD_CASES)), (WORLD_FIXTURE, WORLD_CASES)):
        with open(path, "w") as f:
            json.dump({c: _record(c) for c in sorted(cases)}, f, separators=(",", ":"), sort_keys=True)
            f.write("\n")
