"""streaming.DownloadRing on the device: rows of a known pattern go through the ring's stages, its page-locked buffers and
the copy stream, and arrive exactly."""
import numpy as np
import pytest

from gan_heightmaps_amd.streaming import DownloadRing, store_rows
from tests.gpu_common import dev      # noqa: F401  (dev: the module-scoped fixture)

pytestmark = pytest.mark.gpu


def test_rows_arrive_exactly_through_the_copy_stream(dev):      # noqa: F811
    C, H, W = 3, 11, 37
    want = (np.arange(C * H * W, dtype=np.float32) * 0.5 - 100).reshape(C, H, W)
    out = np.full_like(want, -1)
    row = 4 * W
    cp = type(dev)(dev.index)
    src = dev.alloc(want.nbytes)
    ring = None
    try:
        dev.h2d(src, want)
        ring = DownloadRing(dev, cp, C * 4 * row, lambda buf, ya, yb: store_rows(out, buf, ya, yb, W))
        ya = 0
        for k in [3, 1, 4, 2, 1]:
            stage = ring.stage()
            for c in range(C):                                # the stage holds planar [C, k, W]
                dev.d2d(stage + c * k * row, src + (c * H + ya) * row, k * row)
            ring.send(C * k * row, ya, ya + k)
            ring.poll()
            ya += k
        ring.finish()
    finally:
        dev.sync()
        cp.sync()
        if ring is not None:
            ring.close()
        dev.free(src)
        cp.close()
    assert np.array_equal(out, want)
