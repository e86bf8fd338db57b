"""bench.py --dump-outputs: what the last timed step computed, written as float32 / float64 .npy files under a size cap,
with the same sampled elements from run to run (checked on stand-in parameter stores: no GPU); and on the GPU, the same
outputs from a plain run as from a --full run."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Buf:
    def __init__(self, a):
        self.a = a

    def numpy(self):
        return self.a.reshape(1, -1, 1, 1)


class _Store:
    def __init__(self, n_train, n_state, seed):
        rng = np.random.RandomState(seed)
        self.n_train, self.n_state = n_train, n_state
        # padded like engine.ParamStore; a parameter's value is its index (exact in float32 below 2^24)
        self.w = _Buf(np.arange(n_train + 64, dtype=np.float32))
        self.g = _Buf(-self.w.a - seed)
        self.s = _Buf(rng.rand(max(n_state, 1)).astype(np.float32))


def _engine():
    return types.SimpleNamespace(sync=lambda: None, stores={
        "dcgan_gen": _Store(bench.DUMP_SAMPLE + 12345, 300, 0), "dcgan_disc": _Store(5000, 0, 1),
        "p2p_gen": _Store(7000, 40, 2), "p2p_disc": _Store(3 * bench.DUMP_SAMPLE, 0, 3)})


def test_dump_outputs_writes_the_step_results(tmp_path):
    eng = _engine()
    losses = [np.float32(v) for v in (0.5, 0.25, 1.5, 0.125, 2.0)]
    total = bench.dump_outputs(eng, losses, str(tmp_path / "a"))
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(["losses.npy"] + ["%s.%s.npy" % (k, w) for k in eng.stores for w in ("params", "grads")]
                           + ["dcgan_gen.bn_state.npy", "p2p_gen.bn_state.npy"])
    assert total == sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in files) <= bench.DUMP_LIMIT
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["losses"], np.array([0.5, 0.25, 1.5, 0.125, 2.0]))
    small = eng.stores["dcgan_disc"]
    assert np.array_equal(got["dcgan_disc.params"], small.w.a[:small.n_train])          # small stores whole, no padding
    assert np.array_equal(got["p2p_gen.bn_state"], eng.stores["p2p_gen"].s.a[:40])
    big = eng.stores["p2p_disc"]
    assert got["p2p_disc.params"].size == got["p2p_disc.grads"].size == bench.DUMP_SAMPLE
    # distinct elements inside the used range, parameters and gradients sampled at the same indices
    idx = got["p2p_disc.params"].astype(np.int64)
    assert (np.diff(idx) > 0).all() and idx[-1] < big.n_train
    assert np.array_equal(big.g.a[idx], got["p2p_disc.grads"])
    # the same arguments sample the same elements
    bench.dump_outputs(_engine(), losses, str(tmp_path / "b"))
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f


def test_dump_outputs_option():
    assert bench.parse_args([]).dump_outputs is None
    a = bench.parse_args(["--steps", "7", "--dump-outputs", "out"])
    assert a.dump_outputs == "out" and a.steps == 7


def test_full_option_is_off_by_default():
    assert not bench.parse_args([]).full
    assert bench.parse_args(["--full"]).full


@pytest.mark.gpu
def test_plain_run_dumps_what_a_full_run_dumps(tmp_path):
    """a plain run leaves out what --full measures beside the headline, but takes the same training steps before its timed
    region: the last timed step's outputs are bit-identical, and only the --full line carries the roofline"""
    lines = {}
    for name, extra in (("plain", []), ("full", ["--full", "--no-secondary", "--no-cpu-baseline", "--minimal",
                                                   "--side-file", str(tmp_path / "side.json")])):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "2",
                            "--dump-outputs", str(tmp_path / name)] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines[name] = json.loads(r.stdout.strip().splitlines()[-1])
    plain, full = lines["plain"], lines["full"]
    assert plain["roofline"] is None and "cpu_baseline" not in plain and "side_file" not in plain
    assert isinstance(full["roofline"], dict) and os.path.exists(tmp_path / "side.json")
    assert plain["steps"] == full["steps"] == 3 and plain["warmup"] == full["warmup"] == 2 and plain["value"] > 0
    assert plain["losses"] == full["losses"]
    files = sorted(os.listdir(tmp_path / "plain"))
    assert files == sorted(os.listdir(tmp_path / "full")) and "losses.npy" in files
    for f in files:
        assert np.array_equal(np.load(tmp_path / "plain" / f), np.load(tmp_path / "full" / f)), f
