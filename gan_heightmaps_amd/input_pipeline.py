"""The asynchronous input pipeline of step.GanStep (no reference counterpart: pix2pix.py:201-212 uploads, waits, steps, waits).

The input buffers of a plan are live until almost the end of its step (the first layers' weight gradients read z and
x last), and consecutive steps OVERLAP in the steady state (stage A of step i+1 starts while the gradient stream still
finishes step i): any hand-over that waits for "the previous step" is a barrier that costs more than the upload it
hides (measured: 10.2 ms per bf16 step with a staging set + device-to-device hand-over, against 6.2 resident).  So the
pipeline double-buffers the PLAN: two complete plans per batch size (slot 0 / 1: own activations and inputs, shared
parameter stores; +11 GB of 288), consecutive steps alternate, and the batch of step i+1 goes from page-locked host
staging straight into the other slot's input buffers on a COPY stream while step i runs.  Orderings, all by events:
  * the stage streams of step i wait for the event recorded right behind the upload of batch i (long passed, normally);
  * before the HOST starts an upload into a slot it waits (hipEventSynchronize) for the events recorded behind the step
    that last used that slot -- a host-side wait, two steps back, never a device-side one: a copy stream that sits in a
    hipStreamWaitEvent for the end of a step blocks its hardware queue, and whichever compute stream ROCm mapped onto
    the same queue stalls with it (measured: 6.2 -> 8.8 .. 9.9 ms per bf16 step depending on which stream it hit);
  * the host reuses a page-locked set only after its upload has passed (event sync).
Results are bit-identical to the synchronous loop (the two slots run the same program on the same parameters)."""
import os

import numpy as np

from .device import PinnedArray


class _Slot:
    """what the pipeline keeps per plan"""

    def __init__(self, b, cp, devs, mkpin):
        assert b.z.contiguous and b.x.contiguous and b.y.contiguous
        self.host = {k: mkpin(t.shape) for k, t in (('z', b.z), ('x', b.x), ('y', b.y))}      # page-locked staging set
        self.landed = cp.event_create()                     # behind the last upload into the plan's inputs
        self.uploads = 0                                    # uploads made from ``host``
        self.done = [(d, d.event_create()) for d in devs]   # behind the step that last ran on the plan, per stream
        self.used = False                                   # a step has run on the plan
        self.it_pinned = {}                                 # a device iterator's page-locked buffers for this plan


class InputPipeline:
    """the copy stream (opened at the first upload, closed by close()), a slot per plan, the three upload forms and the
    pipelined loops of engine ``eng``"""

    def __init__(self, eng):
        self.eng = eng
        self.dev = None                 # the copy stream's context while the pipeline is open
        self.slots = {}                 # {id(plan): _Slot}
        self.queue_probe_us = []        # worst interference measured per copy-stream candidate

    def _open(self):
        if self.dev is None:
            eng = self.eng
            mk = type(eng.devs[0])
            # the copy stream must not share a HARDWARE queue with a compute stream (a 16 MB upload in flight on a shared queue
            # holds that stream's kernels back for its whole duration: bf16 611 instead of 638 img/s on the boxes where ROCm
            # happened to map them together): probe candidates, keep the first one every compute stream is free of
            compute = [d for d in eng._all_devs() if d is not None]
            cp, rejects, report = None, [], []
            if hasattr(mk, 'queue_interference') and os.environ.get("GHM_NO_QUEUE_PROBE") is None:
                eng.sync()
                probe = mk(eng.devs[0].index)
                for _ in range(6):
                    cand = mk(eng.devs[0].index)
                    worst = max(max(cand.queue_interference(d, probe), d.queue_interference(cand, probe)) for d in compute)
                    report.append(round(worst, 1))
                    if worst < 300.0:               # (the spin is 1500 us; an unshared queue answers in tens of microseconds)
                        cp = cand
                        break
                    rejects.append(cand)
                for r in rejects[1:] + [probe]:
                    r.close()
                if cp is None:                      # every candidate shares a queue with somebody: take the first
                    cp = rejects[0]
                elif rejects:
                    rejects[0].close()
            else:
                cp = mk(eng.devs[0].index)
            self.dev, self.slots, self.queue_probe_us = cp, {}, report
        return self.dev

    def _slot(self, b):
        cp = self._open()
        if id(b) not in self.slots:
            mkpin = getattr(type(self.eng.devs[0]), 'pinned_array', PinnedArray)       # (host-memory test devices bring their own)
            self.slots[id(b)] = _Slot(b, cp, self.eng._all_devs(), mkpin)
        return self.slots[id(b)]

    def _claim(self, b, from_host):
        """-> (copy stream, slot of plan ``b``) once the host may overwrite the plan's inputs; ``from_host``: and its
        page-locked set"""
        cp, sl = self._open(), self._slot(b)
        if sl.used:
            for d, ev in sl.done:
                d.event_sync(ev)                # the step that last read these input buffers has finished
        if from_host and sl.uploads:
            cp.event_sync(sl.landed)            # the previous upload from this host set has passed
        return cp, sl

    def upload_async(self, b, Z, X, Y):
        """start the upload of a batch into plan ``b``'s input buffers on the copy stream; returns as soon as the copies
        are enqueued (it first waits, on the host, for the step that last ran on this plan)"""
        cp, sl = self._claim(b, True)
        for k, a, t in (('z', Z, b.z), ('x', X, b.x), ('y', Y, b.y)):
            np.copyto(sl.host[k].array, np.asarray(a, np.float32).reshape(sl.host[k].shape))
            cp.h2d_async(t.ptr, sl.host[k])
        cp.event_record(sl.landed)
        sl.uploads += 1

    def upload_resident_async(self, b, zt, xt, yt):
        """upload_async for a batch that already lies in HBM (three contiguous DevTensors): device-to-device copies into plan
        ``b``'s input buffers on the copy stream, same orderings (bench.py rotates resident synthetic batches through its timed
        steps this way, so that no step re-trains the batch of the step before it)"""
        cp, sl = self._claim(b, False)
        for src, dst in ((zt, b.z), (xt, b.x), (yt, b.y)):
            assert src.contiguous and dst.contiguous and src.size == dst.size
            cp.d2d(dst.ptr, src.ptr, 4 * dst.size)
        cp.event_record(sl.landed)

    def produce_async(self, b, it, Z_sampler):
        """like upload_async, with the (A, B) batch made on the device by a data.Hdf5Iterator: uint8 rows from page-locked
        staging + ghm_image_batch straight into plan ``b``'s inputs, all on the copy stream"""
        cp, sl = self._claim(b, True)
        # (the iterator's device-side staging buffers are per iterator, not per slot: the copy stream orders their reuse)
        n = it.next_into(b.x, b.y, via=cp, pinned=sl.it_pinned)
        assert n == b.B
        np.copyto(sl.host['z'].array, np.ascontiguousarray(Z_sampler(n), np.float32).reshape(sl.host['z'].shape))
        cp.h2d_async(b.z.ptr, sl.host['z'])
        cp.event_record(sl.landed)
        sl.uploads += 1

    def enqueue_train_uploaded(self, b, wrap=None):
        """one train step of plan ``b`` on the batch last handed to upload_async(b, ...) (asynchronous)"""
        sl = self._slot(b)
        for d in self.eng.devs[:1 if self.eng.devs[1] is self.eng.devs[0] else 2]:
            d.event_wait(sl.landed)
        self.eng.enqueue_train(b, wrap)
        for d, ev in sl.done:
            d.event_record(ev)
        sl.used = True

    def train_pipelined_from_iterator(self, it, Z_sampler, steps):
        """``steps`` train steps on batches of a data.Hdf5Iterator, batch i+1 produced while step i runs; yields the losses"""
        if steps <= 0:
            return
        b = self.eng.built(it.peek_n(), 0)
        self.produce_async(b, it, Z_sampler)
        for i in range(steps):
            self.enqueue_train_uploaded(b)
            nb = None
            if i + 1 < steps:
                nb = self.eng.built(it.peek_n(), (i + 1) & 1)
                self.produce_async(nb, it, Z_sampler)
            yield self.eng._read_losses()
            b = nb

    def train_pipelined(self, batches):
        """train_fn over an iterable of (Z, X, Y) host batches with the upload of batch i+1 under step i; yields the five
        losses of every step (what train(Z, X, Y) returns), bit-identical to calling train() batch by batch"""
        it = iter(batches)
        cur = next(it, None)
        i = 0
        if cur is None:
            return
        b = self.eng.built(int(np.shape(cur[1])[0]), 0)
        self.upload_async(b, *cur)
        while cur is not None:
            self.enqueue_train_uploaded(b)
            nxt = next(it, None)
            nb = None
            if nxt is not None:
                nb = self.eng.built(int(np.shape(nxt[1])[0]), (i + 1) & 1)
                self.upload_async(nb, *nxt)             # batch i+1 crosses PCIe while step i runs
            yield self.eng._read_losses()
            cur, b, i = nxt, nb, i + 1

    def sync(self):
        if self.dev is not None:        # no upload may outlive a GanStep.sync()
            self.dev.sync()

    def close(self):
        if self.dev is not None:
            self.dev.sync()
            for sl in self.slots.values():
                for h in list(sl.host.values()) + list(sl.it_pinned.values()):
                    h.close()
                self.dev.event_destroy(sl.landed)
                for d, ev in sl.done:
                    d.event_destroy(ev)
            self.dev.close()
            self.dev, self.slots = None, {}
