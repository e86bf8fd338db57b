"""Resumed training continues bit for bit on the MI355X.  Run A trains K then M steps; run B trains the same K steps,
writes Pix2Pix.save_checkpoint, and a fresh model built from a DIFFERENT init seed loads it and trains the same M steps.
Every parameter, BatchNorm statistic, optimiser slot, step counter, dropout counter and the losses of the last M steps
must be equal -- for every lasagne.updates rule, the split-fp32 and fp16 arithmetic, the one-rank RCCL exchange forms and
the pipelined input, and for Pix2Pix.train end to end on the device iterator.  The contrast: a resume through
save_model / load_model (parameters only) does not reproduce run A."""
import os

import numpy as np
import pytest

from tests.gpu_common import K, M, NET_PAIRS, _iterators, assert_same, build, dev, split_run      # noqa: F401  (dev: the module-scoped fixture)

pytestmark = pytest.mark.gpu

RULES = ['sgd', 'momentum', 'nesterov_momentum', 'adagrad', 'rmsprop', 'adadelta', 'adam', 'adamax', 'amsgrad']
@pytest.mark.parametrize("kind", RULES)
def test_resume_is_bit_identical_f32(dev, tmp_path, kind):
    (la, sa), (lc, sc), _ = split_run(kind, dev, tmp_path, dtype='f32')
    assert np.array_equal(np.asarray(la), np.asarray(lc))
    assert_same(sa, sc)
    if kind in ('adam', 'adamax', 'amsgrad'):
        assert all(v['hyper'][1] == K + M for v in sc['state']['nets'].values())


@pytest.mark.parametrize("kind", ['rmsprop', 'adam', 'amsgrad'])
def test_resume_is_bit_identical_bf16x3(dev, tmp_path, kind):
    (la, sa), (lc, sc), _ = split_run(kind, dev, tmp_path, dtype='bf16x3')
    assert np.array_equal(np.asarray(la), np.asarray(lc))
    assert_same(sa, sc)


def test_resume_is_bit_identical_f16_mid_loss_scale_interval(dev, tmp_path):
    """saved with the dynamic loss scale between growth steps: a scale set by hand, clean steps counted since"""
    def mid(m):
        m.engine.set_loss_scale(1024.0)
    (la, sa), (lc, sc), b = split_run('adam', dev, tmp_path, mid=mid, dtype='f16')
    ls = b.engine.loss_scale_state()
    assert ls and all(st['scale'] == 1024.0 and st['clean_steps'] > 0 and st['skipped_steps'] == 0 for st in ls)
    assert np.array_equal(np.asarray(la), np.asarray(lc))
    assert_same(sa, sc)
    assert sc['state']['loss_scale'] == sa['state']['loss_scale']


@pytest.mark.parametrize("mode", ['rs_ag', 'allreduce'])
def test_resume_is_bit_identical_through_the_one_rank_exchange(dev, tmp_path, mode):
    from gan_heightmaps_amd import device, dist
    cdev = device.Device(dev.index)
    comm = dist.Comm(cdev, 0, 1, channels=(2, 4))
    try:
        (la, sa), (lc, sc), b = split_run('adam', dev, tmp_path, dtype='f32', comm=comm, force_exchange=True,
                                          use_graph='recorded', exchange_mode=mode, bucket_mb=2048.0 / 2 ** 20)
        assert b.engine.exchange and b.engine.sharded == (mode == 'rs_ag')
        assert np.array_equal(np.asarray(la), np.asarray(lc))
        assert_same(sa, sc)
    finally:
        comm.close()
        cdev.close()


@pytest.mark.parametrize("prefetch", [True, False])
def test_resume_is_bit_identical_with_and_without_the_input_pipeline(dev, tmp_path, prefetch):
    (la, sa), (lc, sc), _ = split_run('amsgrad', dev, tmp_path, feed='pipelined' if prefetch else 'call',
                                      dtype='bf16x3', prefetch=prefetch)
    assert np.array_equal(np.asarray(la), np.asarray(lc))
    assert_same(sa, sc)


def test_params_only_resume_does_not_reproduce_the_run(dev, tmp_path):
    """why the training state exists: Adam restarts its moments and t, dropout its masks"""
    (la, sa), (lc, sc), _ = split_run('adam', dev, tmp_path, via='params', dtype='f32')
    assert not np.array_equal(np.asarray(la), np.asarray(lc))
    assert any(not np.array_equal(x, y) for n in NET_PAIRS for x, y in zip(sa['params'][n], sc['params'][n]))


# ---- Pix2Pix.train end to end on the device iterator ------------------------------------------------------------------
def _rows(path):
    rows = [l.split(",") for l in open(path).read().strip().split("\n")]
    return [r[:-2] + r[-1:] for r in rows]          # (without the time column)


@pytest.mark.parametrize("prefetch", [True, False])
def test_train_resumed_from_a_state_checkpoint_continues_the_run(dev, tmp_path, prefetch):
    from gan_heightmaps_amd import layers as L
    out_a, out_b, models = str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "models")
    np.random.seed(5)
    a = build('adam', 7, dev, prefetch=prefetch)
    a.train(*_iterators(dev), batch_size=4, num_epochs=2, out_dir=out_a)
    np.random.seed(5)
    b = build('adam', 7, dev, prefetch=prefetch)
    b.train(*_iterators(dev), batch_size=4, num_epochs=1, out_dir=out_b, model_dir=models, save_every=1,
            checkpoint_state=True)
    np.random.seed(99)                      # (the checkpoint brings the sampler's RNG state)
    c = build('adam', 4321, dev, prefetch=prefetch)
    c.train(*_iterators(dev), batch_size=4, num_epochs=1, out_dir=out_b, model_dir=models, save_every=1,
            checkpoint_state=True, resume=models + "/1.model")
    ra, rb = _rows(out_a + "/results.txt"), _rows(out_b + "/results.txt")
    assert len(ra) == len(rb) == 3 and rb[2][0] == "2"
    assert ra == rb
    assert os.path.exists(models + "/2.model")
    for n in NET_PAIRS:
        for x, y in zip(L.get_all_param_values(getattr(a, n[0])[n[1]]), L.get_all_param_values(getattr(c, n[0])[n[1]])):
            assert np.array_equal(x, y), n
    sa, sc = a.engine.training_state(), c.engine.training_state()
    assert sa['rng_counters'] == sc['rng_counters'] and len(sa['rng_counters']) >= 3
