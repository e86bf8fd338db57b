"""What the row-streaming pipelines share on the host (texture.py, terrain.py, world.py): the download ring that takes finished
rows from the device to the caller's array, the row layouts of its stages, the checks of the output array, and the
accumulator's shift between tile rows.
"""
import numpy as np

from .device import PinnedArray

__all__ = ["DownloadRing", "store_rows", "output_array", "check_uint8_channels", "shift_accumulator"]


class DownloadRing:
    """Finished rows -> a device stage -> a page-locked buffer -> ``store``, two of each, the copies on the stream of ``cp`` so
    that rows go down while ``dev`` computes the next ones.  Per group of rows: write them into ``stage()``, ``send`` them, and
    ``poll`` wherever the host may block for the download before.  ``store(buffer, ya, yb)`` gets the page-locked uint8 array,
    whose first bytes are the rows sent as (ya, yb).  The ring owns its stages, buffers and events, not the two contexts."""

    def __init__(self, dev, cp, stage_bytes, store):
        self.dev, self.cp, self.store = dev, cp, store
        self.stages, self.pins, self.finalized, self.downloaded = [], [], [], []
        self.pending, self.sent = [], 0                       # [(slot, ya, yb)] on their way down; groups sent so far
        mkpin = getattr(type(dev), 'pinned_array', PinnedArray)       # (host-memory test devices bring their own)
        try:
            for _ in range(2):
                self.stages.append(dev.alloc(stage_bytes))
            for _ in range(2):
                self.pins.append(mkpin((stage_bytes,), np.uint8))
            for _ in range(2):
                self.finalized.append(dev.event_create())
            for _ in range(2):
                self.downloaded.append(cp.event_create())
        except Exception:
            self.close()
            raise

    def stage(self):
        """the device pointer the next group of rows is written to"""
        slot = self.sent % 2
        # two slots are enough because of this: the download before last, which filled this slot's page-locked buffer, has
        # been stored, so the copy about to be enqueued overwrites nothing the host still has to read
        assert len(self.pending) <= 1, "DownloadRing: poll() after every send()"
        if self.sent >= 2:
            self.dev.event_wait(self.downloaded[slot])        # the stage's previous download has left
        return self.stages[slot]

    def send(self, nbytes, ya, yb):
        """the first ``nbytes`` of the current stage, complete on ``dev``'s stream as of now, start their way down"""
        slot = self.sent % 2
        self.dev.event_record(self.finalized[slot])
        self.cp.event_wait(self.finalized[slot])
        self.cp.d2h_async(self.pins[slot], self.stages[slot], nbytes)
        self.cp.event_record(self.downloaded[slot])
        self.pending.append((slot, ya, yb))
        self.sent += 1

    def _drain(self):
        slot, ya, yb = self.pending.pop(0)
        self.dev.event_sync(self.downloaded[slot])
        self.store(self.pins[slot].array, ya, yb)

    def poll(self):
        """store every download but the newest (blocks the host for them)"""
        while len(self.pending) > 1:
            self._drain()

    def finish(self):
        while self.pending:
            self._drain()

    def close(self):
        """after both streams have been synchronized"""
        for e in self.finalized + self.downloaded:
            self.dev.event_destroy(e)
        for p in self.pins:
            p.close()
        for p in self.stages:
            self.dev.free(p)
        self.stages, self.pins, self.finalized, self.downloaded = [], [], [], []


def store_rows(out, buf, ya, yb, pitch, w=None):
    """rows [ya, yb) of ``out`` from the first bytes of the uint8 array ``buf``, in the layout of ``out``: float32 (C, H, W)
    from planar [C, k, pitch], uint8 (H, W) from [k, pitch], uint8 (H, W, 3) from [k, pitch, 3]; the first ``w`` of each
    row's ``pitch`` pixels are taken (default: all)"""
    k = yb - ya
    if out.dtype == np.float32:
        C = out.shape[0]
        out[:, ya:yb, :] = buf[:C * k * pitch * 4].view(np.float32).reshape(C, k, pitch)[:, :, :w]
    elif out.ndim == 2:
        out[ya:yb] = buf[:k * pitch].reshape(k, pitch)[:, :w]
    else:
        out[ya:yb] = buf[:k * pitch * 3].reshape(k, pitch, 3)[:, :w]


def output_array(out, shape, dtype):
    """``out`` if it is the array asked for (ValueError if not), a new one if None"""
    if out is None:
        return np.empty(shape, dtype)
    if tuple(out.shape) != shape or out.dtype != dtype:
        raise ValueError("out must be %s %s, got %s %s" % (np.dtype(dtype), shape, out.dtype, tuple(out.shape)))
    return out


def check_uint8_channels(channels):
    if channels not in (1, 3):
        raise ValueError("uint8 output needs a 1- or 3-channel generator, this one has %d" % channels)


def shift_accumulator(dev, acc, channels, T, row_bytes, o):
    """between two tile rows of a [channels, T, row] accumulator: the ``o`` rows shared with the next tile row move to the top
    of each plane, the rest restarts at 0"""
    for c in range(channels):
        base = acc + c * T * row_bytes
        if o:
            dev.d2d(base, base + (T - o) * row_bytes, o * row_bytes)
        dev.memset_zero(base + o * row_bytes, (T - o) * row_bytes)
