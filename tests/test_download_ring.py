"""streaming.DownloadRing by itself, on a deterministic simulator of two streams: each context is a FIFO, event_record enqueues a
marker, event_wait a dependency on the event's latest record, d2h_async the copy; a "kernel" is a closure that fills the stage.
LAZY runs queued work only when a host sync forces it (and then no more than that sync needs), EAGER as soon as its
dependencies allow: a missing wait, record or host sync shows as stale rows in one of the two.  Also the three row layouts
(streaming.store_rows), the invariant the ring asserts, and what close() releases.  No GPU."""
import numpy as np
import pytest

from gan_heightmaps_amd.streaming import DownloadRing, store_rows

GROUPS = [3, 1, 4, 2, 1]
H = sum(GROUPS)


def simulator(eager):
    class Event:
        def __init__(self):
            self.records, self.done = [], 0                   # [(context, queue index)] of its records; how many have run

    class Sim:
        mem, freed, pins, pin_closes, events, destroyed = {}, [], [], 0, 0, 0

    class Ctx:
        shared = Sim

        def __init__(self, index=0):
            self.index, self.q, self.head = index, [], 0
            Sim.ctxs = getattr(Sim, "ctxs", []) + [self]

        # ---- the queue ----
        def _push(self, item):
            self.q.append(item)
            if eager:
                progress = True
                while progress:
                    progress = any(c._step(False) for c in Sim.ctxs)

        def _step(self, force):
            """run the head item; a wait whose record has not run blocks, or with ``force`` runs the other queue up to it"""
            if self.head == len(self.q):
                return False
            kind, a, b = self.q[self.head]
            if kind == "wait" and a.done < b:
                if not force:
                    return False
                ctx, idx = a.records[b - 1]
                ctx._run_to(idx)
            elif kind == "record":
                a.done = b
            elif kind == "run":
                a()
            self.head += 1
            return True

        def _run_to(self, idx):
            while self.head <= idx:
                self._step(True)

        # ---- the device surface the ring uses ----
        def alloc(self, nbytes):
            p = 4096 * (len(Sim.mem) + len(Sim.freed) + 1)
            Sim.mem[p] = np.full(nbytes, 0xEE, np.uint8)
            return p

        def free(self, p):
            del Sim.mem[p]
            Sim.freed.append(p)

        class pinned_array:
            def __init__(self, shape, dtype):
                self.array = np.full(shape, 0xDD, dtype)
                Sim.pins.append(self)

            def close(self):
                assert self.array is not None
                self.array = None
                Sim.pin_closes += 1

        def event_create(self):
            Sim.events += 1
            return Event()

        @staticmethod
        def event_destroy(ev):
            Sim.destroyed += 1

        def event_record(self, ev):
            ev.records.append((self, len(self.q)))
            self._push(("record", ev, len(ev.records)))

        def event_wait(self, ev):
            if ev.records:
                self._push(("wait", ev, len(ev.records)))

        @staticmethod
        def event_sync(ev):
            if ev.records and ev.done < len(ev.records):
                ctx, idx = ev.records[-1]
                ctx._run_to(idx)

        def sync(self):
            self._run_to(len(self.q) - 1)

        def d2h_async(self, pinned, p, nbytes):
            def copy():
                pinned.array[:nbytes] = Sim.mem[p][:nbytes]
            self._push(("run", copy, None))

        def launch(self, fn):
            self._push(("run", fn, None))

    return Ctx


def _expected(layout, w):
    y, x = np.mgrid[0:H, 0:w]
    if layout == "f32":
        return np.stack([(1000 * c + 37 * y + x).astype(np.float32) + 0.25 for c in range(3)])
    if layout == "grey":
        return ((7 * y + 3 * x) % 251).astype(np.uint8)
    return np.stack([(7 * y + 3 * x + 50 * c) % 251 for c in range(3)], axis=2).astype(np.uint8)


def _stage_bytes(layout, want, ya, yb, pitch):
    """rows [ya, yb) of ``want`` as a kernel leaves them in a stage: each row padded to ``pitch`` pixels"""
    rows = want[:, ya:yb] if layout == "f32" else want[ya:yb]
    pad = [(0, 0)] * rows.ndim
    pad[2 if layout == "f32" else 1] = (0, pitch - rows.shape[2 if layout == "f32" else 1])
    return np.ascontiguousarray(np.pad(rows, pad, constant_values=99)).view(np.uint8).ravel()


def _run(eager, layout, w, pitch):
    Ctx = simulator(eager)
    sim = Ctx.shared
    dev, cp = Ctx(0), Ctx(0)
    want = _expected(layout, w)
    out = np.full_like(want, 0x55 if layout != "f32" else -1)
    bpp = {"f32": 12, "grey": 1, "rgb": 3}[layout]
    ring = DownloadRing(dev, cp, max(GROUPS) * pitch * bpp,
                        lambda buf, ya, yb: store_rows(out, buf, ya, yb, pitch, None if pitch == w else w))
    try:
        ya = 0
        for k in GROUPS:
            stage = ring.stage()

            def kernel(stage=stage, ya=ya, k=k):
                data = _stage_bytes(layout, want, ya, ya + k, pitch)
                sim.mem[stage][:] = 0xEE
                sim.mem[stage][:data.size] = data
            dev.launch(kernel)
            ring.send(k * pitch * bpp, ya, ya + k)
            ring.poll()
            ya += k
        ring.finish()
    finally:
        dev.sync()
        cp.sync()
        ring.close()
    return out, want, sim


@pytest.mark.parametrize("eager", [False, True], ids=["lazy", "eager"])
@pytest.mark.parametrize("layout,w,pitch", [(layout, w, w) for layout in ("f32", "grey", "rgb") for w in (37, 64)]
                         + [("f32", 37, 40), ("rgb", 37, 40)])
def test_rows_arrive_exactly(eager, layout, w, pitch):
    out, want, sim = _run(eager, layout, w, pitch)
    assert np.array_equal(out, want)
    assert sim.events == sim.destroyed == 4 and sim.pin_closes == len(sim.pins) == 2 and len(sim.freed) == 2 and not sim.mem


@pytest.mark.parametrize("eager", [False, True], ids=["lazy", "eager"])
@pytest.mark.parametrize("layout,w", [("f32", 37), ("rgb", 64)])
def test_polling_every_second_send_trips_the_assertion(eager, layout, w):
    """two downloads pending when a stage is asked for: its page-locked buffer may still hold rows nobody has stored.  The
    ring refuses; the rows sent until then are intact"""
    Ctx = simulator(eager)
    dev, cp = Ctx(0), Ctx(0)
    want = _expected(layout, w)
    out = np.full_like(want, 0x55 if layout != "f32" else -1)
    untouched = out.copy()
    bpp = {"f32": 12, "grey": 1, "rgb": 3}[layout]
    ring = DownloadRing(dev, cp, max(GROUPS) * w * bpp, lambda buf, ya, yb: store_rows(out, buf, ya, yb, w))
    ya, sent = 0, 0
    with pytest.raises(AssertionError, match="poll"):
        for i, k in enumerate(GROUPS):
            stage = ring.stage()

            def kernel(stage=stage, ya=ya, k=k):
                data = _stage_bytes(layout, want, ya, ya + k, w)
                Ctx.shared.mem[stage][:data.size] = data
            dev.launch(kernel)
            ring.send(k * w * bpp, ya, ya + k)
            if (i + 1) % 2 == 0:
                ring.poll()
            ya, sent = ya + k, sent + 1
    assert sent == 3                                          # groups 0 .. 2 went out, the stage for group 3 was refused
    ring.finish()
    rows = (slice(None), slice(0, ya)) if layout == "f32" else (slice(0, ya),)
    rest = (slice(None), slice(ya, None)) if layout == "f32" else (slice(ya, None),)
    assert np.array_equal(out[rows], want[rows]) and np.array_equal(out[rest], untouched[rest])
    ring.close()


@pytest.mark.parametrize("fail_at", [0, 2, 3])
def test_close_after_an_exception_releases_everything(fail_at):
    Ctx = simulator(False)
    sim = Ctx.shared
    dev, cp = Ctx(0), Ctx(0)
    ring = DownloadRing(dev, cp, 64, lambda buf, ya, yb: None)
    stages = list(ring.stages)
    try:
        for i in range(5):
            ring.stage()
            if i == fail_at:
                raise RuntimeError("mid-sequence")
            ring.send(16, i, i + 1)
            ring.poll()
    except RuntimeError:
        pass
    dev.sync()
    cp.sync()
    ring.close()
    assert sorted(sim.freed) == sorted(stages) and not sim.mem
    assert sim.pin_closes == 2 and all(p.array is None for p in sim.pins)
    assert sim.events == sim.destroyed == 4
    ring.close()                                              # a second close releases nothing twice
    assert len(sim.freed) == 2 and sim.pin_closes == 2 and sim.destroyed == 4


def test_a_failing_constructor_releases_what_it_made():
    Ctx = simulator(False)
    sim = Ctx.shared

    class Short(Ctx):
        def event_create(self):
            raise MemoryError("no more events")
    with pytest.raises(MemoryError):
        DownloadRing(Short(0), Ctx(0), 64, lambda buf, ya, yb: None)
    assert len(sim.freed) == 2 and not sim.mem and sim.pin_closes == 2
