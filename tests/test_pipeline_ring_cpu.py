"""The ring under bev_amd.pipeline.FramePipeline and SitePipeline (pipeline._Ring), on the stand-in runtime of
tests/test_pipeline_order_cpu.py: the literal sequence of runtime calls a slot's way through the ring makes, what a constructor that
fails half-way leaves for close(), and that every ring method has one body."""
import ctypes

import pytest

from bev_amd import _lib
from bev_amd import pipeline
from tests import test_pipeline_order_cpu as OC

H2D, D2H = 1, 2


class Logged(OC.Runtime):
    """The stand-in runtime with a log of what it was asked: (call, stream, event, a copy's (dst, src, bytes) / a launch's slot / None)."""

    def __init__(self, fail_create=None):
        super().__init__()
        self.log, self.created, self.fail_create = [], 0, fail_create

    def hipEventCreateWithFlags(self, ref, flags):
        assert flags == 2  # hipEventDisableTiming
        self.created += 1
        if self.created == self.fail_create:
            return 1
        self.log.append(("hipEventCreateWithFlags", None, ref._obj, None))
        return super().hipEventCreateWithFlags(ref, flags)

    def hipMemcpyAsync(self, dst, src, nbytes, kind, stream):
        self.log.append(("hipMemcpyAsync " + {H2D: "H2D", D2H: "D2H"}[kind], stream, None, (dst, src, nbytes)))
        return super().hipMemcpyAsync(dst, src, nbytes, kind, stream)

    def hipEventRecord(self, event, stream):
        self.log.append(("hipEventRecord", stream, event, None))
        return super().hipEventRecord(event, stream)

    def hipStreamWaitEvent(self, stream, event, flags):
        assert flags == 0
        self.log.append(("hipStreamWaitEvent", stream, event, None))
        return super().hipStreamWaitEvent(stream, event, flags)

    def hipEventSynchronize(self, event):
        self.log.append(("hipEventSynchronize", None, event, None))
        return super().hipEventSynchronize(event)

    def hipEventDestroy(self, event):
        self.log.append(("hipEventDestroy", None, event, None))
        return super().hipEventDestroy(event)

    def run_all(self, stream):  # (what stream.synchronize() comes to)
        self.log.append(("synchronize", stream, None, None))
        super().run_all(stream)

    def taken(self, pipe):
        """The log so far as (call, stream name, which ring's event, slot), and an empty log."""
        rings = {id(e): (name, slot) for name in ("ev_up", "ev_run", "ev_down") for slot, e in enumerate(getattr(pipe, name))}
        out = []
        for call, stream, event, copy in self.log:
            ring, slot = rings[id(event)] if event is not None else (None, None)
            if call.startswith("hipMemcpyAsync"):  # the slot whose buffers the copy names, and that it names one buffer's whole length
                dst, src, nbytes = copy
                dev, host = (dst, src) if call.endswith("H2D") else (src, dst)
                devs, hosts = (pipe.d_in, pipe.h_in) if call.endswith("H2D") else (pipe.d_out, pipe.h_out)
                (slot,) = [s for s in range(pipe.depth) for d, h in zip(pipeline._buffers(devs[s]), pipeline._buffers(hosts[s]))
                           if (d.data_ptr(), h.data_ptr(), d.numel() * d.element_size()) == (dev, host, nbytes)]
            elif call == "launch":
                slot = copy
            out.append((call, stream.name if stream is not None else None, ring, slot))
        self.log = []
        return out


@pytest.fixture
def ring(monkeypatch):
    """make(config name) -> (a pipeline of depth 2 on a logging runtime, that runtime)."""
    made = []

    def make(config):
        rt = Logged()
        monkeypatch.setattr(pipeline, "_hip", rt)
        cfg = OC.CONFIGS[config]
        monkeypatch.setattr(cfg, "rt", rt)
        p = cfg.make()
        # the prepared launches, logged as the runtime's calls are: the stand-in's arguments are (slot, blend)
        p._launch = [((lambda *a, fn=fn: rt.log.append(("launch", p.s_run, None, a[0])) or fn(*a)), args) for fn, args in p._launch]
        made.append((p, rt))
        return p, rt

    yield make
    for p, rt in made:
        p.close()
        rt.drain(p)


# ---- the literal sequence of runtime calls: written out from the ring's contract, one list per kind of output ----------------------------------------------
UPLOAD = ("hipMemcpyAsync H2D", "s_up", None, 0)  # one per input buffer of the slot
COMMIT_AND_RESULT = {
    "copy_down": [
        UPLOAD,
        ("hipEventRecord", "s_up", "ev_up", 0),
        ("hipStreamWaitEvent", "s_run", "ev_up", 0),
        ("launch", "s_run", None, 0),
        ("hipEventRecord", "s_run", "ev_run", 0),
        ("hipStreamWaitEvent", "s_down", "ev_run", 0),
        ("hipMemcpyAsync D2H", "s_down", None, 0),
        ("hipEventRecord", "s_down", "ev_down", 0),
        ("hipEventSynchronize", None, "ev_down", 0),  # result()
    ],
    "zero_copy": [
        UPLOAD,
        ("hipEventRecord", "s_up", "ev_up", 0),
        ("hipStreamWaitEvent", "s_run", "ev_up", 0),
        ("launch", "s_run", None, 0),
        ("hipEventRecord", "s_run", "ev_run", 0),
        ("hipEventSynchronize", None, "ev_run", 0),  # result()
    ],
    "on_device": [
        UPLOAD,
        ("hipEventRecord", "s_up", "ev_up", 0),
        ("hipStreamWaitEvent", "s_run", "ev_up", 0),
        ("launch", "s_run", None, 0),
        ("hipEventRecord", "s_run", "ev_run", 0),
        ("hipEventSynchronize", None, "ev_run", 0),  # result()
    ],
}
THIRD_NEXT_INPUT = {"copy_down": [("hipEventSynchronize", None, "ev_down", 0)], "zero_copy": [("hipEventSynchronize", None, "ev_run", 0)],
                    "on_device": [("hipEventSynchronize", None, "ev_run", 0)]}
FIVE = ["frame-copy_down", "frame-zero_copy", "frame-on_device", "site-copy_down", "site-on_device"]


def _uploads(config):
    return OC.N_CAMS if OC.CONFIGS[config].site else 1


def _next(p):
    return p.next_inputs() if isinstance(p, pipeline.SitePipeline) else [p.next_input()]


@pytest.mark.parametrize("config", FIVE)
def test_commit_and_result_make_these_calls_in_this_order(ring, config):
    p, rt = ring(config)
    opened = rt.taken(p)
    assert opened == [("hipEventCreateWithFlags", None, name, slot) for name in ("ev_up", "ev_run", "ev_down") for slot in range(OC.DEPTH)]
    assert _next(p) and rt.taken(p) == []  # (a slot that had no occupant: nothing to wait for)
    p.commit()
    p.result()
    expected = COMMIT_AND_RESULT[config.split("-")[1]]
    assert expected[0] is UPLOAD and UPLOAD not in expected[1:]
    assert rt.taken(p) == [UPLOAD] * _uploads(config) + expected[1:]  # both classes: the same list up to the number of uploads


@pytest.mark.parametrize("config", FIVE)
def test_the_third_next_input_waits_for_the_slots_last_event(ring, config):
    p, rt = ring(config)
    rt.taken(p)
    for _ in range(OC.DEPTH):
        assert _next(p) and rt.taken(p) == []
        p.commit()
        rt.taken(p)
    bufs = _next(p)
    assert rt.taken(p) == THIRD_NEXT_INPUT[config.split("-")[1]]
    assert [b.ctypes.data for b in bufs] == [t.data_ptr() for t in pipeline._buffers(p.h_in[0])]  # slot 0's pinned buffers again


def test_the_second_slot_names_its_own_events(ring):
    p, rt = ring("site-copy_down")
    rt.taken(p)
    p.commit()
    rt.taken(p)
    p.commit()
    p.result()
    p.result()
    at = lambda e: e[:3] + (1,) if e[3] == 0 else e  # noqa: E731
    assert rt.taken(p) == [at(e) for e in [UPLOAD] * OC.N_CAMS + COMMIT_AND_RESULT["copy_down"][1:-1]] + [
        ("hipEventSynchronize", None, "ev_down", 0), ("hipEventSynchronize", None, "ev_down", 1)]


def test_a_full_ring_refuses_in_each_classes_words(ring):
    for config, text in (("frame-on_device", "FramePipeline: 2 frames are in flight and none has been taken with result(); a ring of depth 2 "
                                             "holds at most 2 undelivered frames"),
                         ("site-on_device", "SitePipeline: 2 sets of frames are in flight and none has been taken with result(); a ring of depth 2 "
                                            "holds at most 2 undelivered results")):
        p, rt = ring(config)
        p.commit()
        p.commit()
        rt.taken(p)
        with pytest.raises(RuntimeError) as e:
            p.commit()
        assert str(e.value) == text and rt.taken(p) == [] and p.n_in == 2 and p.ready() == 2


# ---- a failing open ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [pipeline.FramePipeline, pipeline.SitePipeline])
@pytest.mark.parametrize("depth,k", [(d, k) for d in (2, 3) for k in (1, d + 1, 3 * d)])
def test_a_failing_open_leaves_close_what_exists(monkeypatch, cls, depth, k):
    """The k-th event cannot be made: the opener raises, and close() still drains the streams and releases the k - 1 events there are."""
    rt = Logged(fail_create=k)
    monkeypatch.setattr(pipeline, "_hip", rt)
    p = cls.__new__(cls)
    p.depth, p.download = depth, True
    streams = [OC._Stream(rt, name) for name in ("s_up", "s_run", "s_down")]
    with pytest.raises(_lib.BevWarpError):
        p._open(streams, streams)
    events = p.ev_up + p.ev_run + p.ev_down
    assert len(events) == k - 1 and [len(p.ev_up), len(p.ev_run), len(p.ev_down)] == [min(depth, max(0, k - 1 - i * depth)) for i in range(3)]
    assert all(isinstance(e, ctypes.c_void_p) for e in events) and [e[2] for e in rt.log] == events
    rt.log = []
    p.close()
    assert [(call, stream and stream.name) for call, stream, _, _ in rt.log] == [("synchronize", "s_up"), ("synchronize", "s_run"), ("synchronize", "s_down")] + [
        ("hipEventDestroy", None)] * (k - 1)
    assert [e[2] for e in rt.log[3:]] == events  # each of them, once
    before = rt.calls
    assert p.close() is None and rt.calls == before and len(rt.log) == 3 + k - 1  # a second close() makes no runtime call


def test_an_object_whose_constructor_never_reached_the_ring_closes_quietly():
    for cls in (pipeline.FramePipeline, pipeline.SitePipeline):
        p = cls.__new__(cls)
        assert p.close() is None  # (no streams, no events: nothing to do, and no AttributeError from __del__)


# ---- one body per ring method ------------------------------------------------------------------------------------------------------------------------------
RING_METHODS = ("commit", "close", "result", "ready", "run", "__enter__", "__exit__", "__del__")


def test_both_classes_share_the_ring_methods():
    for name in RING_METHODS + ("_open", "_start", "_allocate", "next_inputs"):
        assert getattr(pipeline.FramePipeline, name) is getattr(pipeline.SitePipeline, name), name
        assert name not in vars(pipeline.FramePipeline) and name not in vars(pipeline.SitePipeline), name
    for cls in (pipeline.FramePipeline, pipeline.SitePipeline):
        assert {"submit", "_launch_py", "_prepared", "__init__"} <= set(vars(cls))
    # the wait before a pinned slot is reused lives in next_inputs() alone; next_input() is FramePipeline's and hands out its one buffer
    assert "next_input" in vars(pipeline.FramePipeline) and not hasattr(pipeline.SitePipeline, "next_input")


def test_next_input_is_the_one_buffer_of_next_inputs(ring):
    p, rt = ring("frame-copy_down")
    one, many = p.next_input(), p.next_inputs()
    assert len(many) == 1 and one.ctypes.data == many[0].ctypes.data == p.h_in[0].data_ptr() and one.shape == many[0].shape == tuple(p.h_in[0].shape)


def test_the_nv12_single_buffer_rule():
    """(h * 3 / 2, w) bytes in one buffer: the (U, V) rows follow the Y rows, every row is w bytes, and the frame strides are 0 (one frame)."""
    import torch
    t = torch.zeros((6 * 3 // 2, 10), dtype=torch.uint8)
    assert pipeline._nv12(t, 6, 10) == ((t.data_ptr(), t.data_ptr() + 60), (0, 10, 0, 10))
