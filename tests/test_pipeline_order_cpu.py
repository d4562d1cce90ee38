"""tests/pipeline_order.py on the CPU: its checks pass the pipelines as they are and notice what they are for -- in the manner of
tests/test_launch_contexts_cpu.py.  This stands where a GPU mutation run would: nothing on the GPU removes an edge.

The code under test is the PRODUCTION commit(), result(), next_input(s)(), submit(), run(), close() and set_gains() of
bev_amd.pipeline.FramePipeline and SitePipeline -- one body each, in the ring both classes stand on.  The objects are made without their
constructors (which need a device): they are given CPU tensors as slots, and the ring's own opener (_open) makes the rest from queue
streams; bev_amd.pipeline._hip is replaced for the length of a test by a stand-in runtime:

  a stream                is a queue of deferred operations; nothing runs when it is enqueued
  hipMemcpyAsync          a deferred copy of the bytes between the two addresses
  the prepared launch     a deferred byte function of the slot's device inputs (stand_in), of the host values and of the gain words --
                          those two read when the launch is CALLED, as the library reads its host pointers and the camera table
  hipEventCreateWithFlags the handle the opener made becomes an event that was never recorded
  hipEventRecord          a marker in the stream's queue; a re-recorded event means its latest record, one never recorded is complete
  hipStreamWaitEvent      captures the event's latest record
  hipEventSynchronize     runs the minimal set of queued operations the record depends on: its stream up to the marker, and, for each wait
                          met on the way, the same for the record waited for -- nothing else
  stream.synchronize()    the same for everything in the stream's queue
  the final drain         what is still queued when a pipeline goes runs s_down before s_run before s_up, honouring waits only
  the delay               an operation that sets a flag

With the honest runtime every check passes on every configuration.  Then one call at a time is taken out of the runtime -- the wait of
s_run, the wait of s_down, the synchronise in result(), the synchronise in next_input(s)(), the record of ev_run, the stream synchronise in
close() -- and the host-value copy is reverted: each must fail its named check with an AssertionError."""
import ctypes
import sys

import numpy as np
import pytest
import torch

from bev_amd import _lib
from bev_amd import pipeline
from tests import pipeline_order as PO
from tests import stitch_gain_ref as SG

IN_SHAPE, OUT_SHAPE, N_CAMS, DEPTH = (6, 5, 3), (4, 7, 3), 2, 2
SCALE, BIAS, BORDER = (1 / 255.0, 0.5, 2.0), (0.0, -1.0, 3.5), (9.0, 200.0, 31.0)
REMOVALS = ("the s_run wait", "the s_down wait", "the synchronise in result()", "the synchronise in next_input(s)()", "the record of ev_run",
            "the stream synchronise in close()")


# ---- the stand-in runtime ---------------------------------------------------------------------------------------------------------------------------------
class _Record:
    def __init__(self, stream):
        self.stream, self.done = stream, False


class _Wait:
    def __init__(self, record):
        self.record = record


class _Event:
    """An event of the runtime's own tests below.  A pipeline's events are the ctypes handles its opener made, given this class's `latest`
    by hipEventCreateWithFlags."""
    latest = None  # (never recorded: complete)


class _Flag:
    done = False

    def set(self):
        self.done = True

    def query(self):
        return self.done


def _caller():
    """The production method a runtime call was made from."""
    return sys._getframe(2).f_code.co_name


class _Stream:
    def __init__(self, rt, name):
        self.rt, self.name, self.queue = rt, name, []

    def synchronize(self):
        self.rt.calls += 1
        if self.rt.removed == "the stream synchronise in close()" and _caller() == "close":
            return
        self.rt.run_all(self)


class Runtime:
    """What bev_amd.pipeline asks of libamdhip64, on queues.  removed: the one call this runtime ignores."""

    def __init__(self, removed=None):
        assert removed is None or removed in REMOVALS
        self.removed, self.calls = removed, 0

    # -- the calls
    def hipEventCreateWithFlags(self, ref, flags):
        self.calls += 1
        ref._obj.latest = _Event.latest  # (the opener's own handle is the event)
        return 0

    def hipMemcpyAsync(self, dst, src, nbytes, kind, stream):
        self.calls += 1
        stream.queue.append(lambda: ctypes.memmove(dst, src, nbytes))
        return 0

    def hipEventRecord(self, event, stream):
        self.calls += 1
        if self.removed == "the record of ev_run" and stream.name == "s_run":
            return 0
        event.latest = _Record(stream)
        stream.queue.append(event.latest)
        return 0

    def hipStreamWaitEvent(self, stream, event, flags):
        self.calls += 1
        if self.removed == "the %s wait" % stream.name:
            return 0
        if event.latest is not None:
            stream.queue.append(_Wait(event.latest))
        return 0

    def hipEventSynchronize(self, event):
        self.calls += 1
        if self.removed == "the synchronise in result()" and _caller() == "result":
            return 0
        if self.removed == "the synchronise in next_input(s)()" and _caller() in ("next_input", "next_inputs"):
            return 0
        if event.latest is not None:
            self.run_until(event.latest)
        return 0

    def hipEventDestroy(self, event):
        self.calls += 1
        return 0

    # -- the queues
    def _step(self, stream):
        op = stream.queue[0]
        if isinstance(op, _Wait):
            if not op.record.done:
                self.run_until(op.record)
            assert stream.queue.pop(0) is op
        elif isinstance(op, _Record):
            assert stream.queue.pop(0) is op
            op.done = True
        else:
            assert stream.queue.pop(0) is op
            op()

    def run_until(self, record):
        while not record.done:
            assert record in record.stream.queue, "a record that left its queue undone"
            self._step(record.stream)

    def run_all(self, stream):
        while stream.queue:
            self._step(stream)

    def drain(self, pipe):
        for stream in (pipe.s_down, pipe.s_run, pipe.s_up):
            self.run_all(stream)


# ---- the pipelines without their constructors ----------------------------------------------------------------------------------------------------------------
def stand_in(srcs, n_out, values, words):
    """The stand-in launch: n_out bytes, each of which depends on a byte of every source, on every host value and on every gain word."""
    acc = np.zeros(n_out, np.int64)
    for k, s in enumerate(srcs):
        acc += (2 * k + 3) * np.resize(np.asarray(s).reshape(-1).astype(np.int64), n_out)
    at = np.arange(n_out, dtype=np.int64)
    for j, v in enumerate(values):  # (a weight per byte and per value: no two sets of values give one offset)
        acc += ((at + j) % 13 + 1) * int(round(np.nan_to_num(float(v), nan=4321.7) * 16))
    for j, w in enumerate(words):
        acc += ((at + j) % 11 + 1) * (int(w) % 251)
    return (acc % 256).astype(np.uint8)


def _inputs(i, camera=0):
    return np.random.default_rng(100 + 10 * i + camera).integers(0, 256, IN_SHAPE, dtype=np.uint8)


def _words(gains):
    return [] if gains is None else [SG.word(g) for g in SG.quantize(gains, N_CAMS)]


class CpuConfig:
    """A pipeline of depth 2 on CPU tensors.  kind "frame" / "site"; download, zero_copy as the constructors' keywords; host: the pipeline has
    scale and bias (site: and a border value)."""

    def __init__(self, name, kind, download=True, zero_copy=False, host=False, gains=None):
        self.name, self.site, self.download, self.zero_copy, self.has_host, self.gains = name, kind == "site", download, bool(zero_copy and download), host, gains
        self.copy_down = download and not self.zero_copy
        self.rt = None  # the test's runtime

    def __repr__(self):
        return self.name

    def host_values(self):
        values = dict(scale=np.array(SCALE, dtype=np.float64), bias=np.array(BIAS, dtype=np.float64))
        if self.site:
            values["border_value"] = np.array(BORDER, dtype=np.float64)
        return values

    def _default_values(self):
        return list(SCALE) + list(BIAS) + (list(BORDER) if self.site else []) if self.has_host else []

    def inputs(self, i):
        return [_inputs(i, k) for k in range(N_CAMS)] if self.site else [_inputs(i)]

    def _expected_of(self, arrays, gains):
        gains = self.gains if gains is PO.DEFAULT else gains
        return stand_in(arrays, int(np.prod(OUT_SHAPE)), self._default_values(), _words(gains)).reshape(OUT_SHAPE)

    def expected(self, i, gains=PO.DEFAULT):
        return self._expected_of(self.inputs(i), gains)

    def expected_of_poisoned_input(self, gains=PO.DEFAULT):
        return self._expected_of([np.full_like(a, PO.POISON) for a in self.inputs(0)], gains)

    def compare(self, got, exp, what):
        np.testing.assert_array_equal(got.numpy(), exp, err_msg=what)

    def make(self, host=None, gains=PO.DEFAULT):
        rt = self.rt
        assert pipeline._hip is rt, "the stand-in runtime is not installed"
        cls = pipeline.SitePipeline if self.site else pipeline.FramePipeline
        p = cls.__new__(cls)
        u8 = lambda shape: torch.zeros(shape, dtype=torch.uint8)  # noqa: E731
        p.depth, p.download = DEPTH, self.download
        if self.site:
            p.h_in = [[u8(IN_SHAPE) for _ in range(N_CAMS)] for _ in range(DEPTH)]
            p.d_in = [[u8(IN_SHAPE) for _ in range(N_CAMS)] for _ in range(DEPTH)]
            p._in_bytes = [t.numel() for t in p.h_in[0]]
        else:
            p.zero_copy_out = self.zero_copy
            p.h_in, p.d_in = [u8(IN_SHAPE) for _ in range(DEPTH)], [u8(IN_SHAPE) for _ in range(DEPTH)]
            p._in_bytes = p.h_in[0].numel()
        p.d_out = [u8(OUT_SHAPE) for _ in range(DEPTH)]
        p.h_out = [u8(OUT_SHAPE) for _ in range(DEPTH)] if self.download else None
        p._out_bytes = p.d_out[0].numel()
        streams = [_Stream(rt, name) for name in ("s_up", "s_run", "s_down")]
        p._open(streams, streams)  # (the ring as the constructors open it: a queue is its own handle)
        # the host arrays the prepared launches point into, as the constructors make them: through the production helper
        values = dict(self.host_values(), **(host or {})) if self.has_host else {}
        p._keep = [pipeline._by_value(values[name], 3) for name in ("scale", "bias", "border_value") if name in values]
        # one prepared launch per slot: (callable, arguments); a site's arguments hold `blend` at _blend_at, which set_gains rewrites
        p._launch = [(self._launcher(p, slot), (slot, _lib.STITCH_FEATHER)) for slot in range(DEPTH)]
        if self.site:
            p.n_cams, p.blend, p.gains, p._blend_at = N_CAMS, "feather", None, 1
            p._cams = [(_lib.MapCamera * N_CAMS)() for _ in range(DEPTH)]
            gains = self.gains if gains is PO.DEFAULT else gains
            if gains is not None:
                p.set_gains(gains)  # (the production path to the camera tables and to the flag in `blend`)
        return p

    def _launcher(self, p, slot):
        rt, site, zero_copy = self.rt, self.site, self.zero_copy

        def launch(*args):
            rt.calls += 1
            values = [float(v) for a in p._keep for v in a]  # read through the host pointers NOW, as the library does at every commit()
            words = [cam.reserved for cam in p._cams[slot]] if site and args[p._blend_at] & _lib.STITCH_GAIN else []
            srcs = p.d_in[slot] if site else [p.d_in[slot]]
            dst = p.h_out[slot] if zero_copy else p.d_out[slot]
            p.s_run.queue.append(lambda: dst.copy_(torch.from_numpy(stand_in([s.numpy() for s in srcs], dst.numel(), values, words)).reshape(dst.shape)))
            return 0
        return launch


class Queues:
    """The backend of the checks on the CPU."""

    def __init__(self, rt):
        self.rt = rt

    def delay(self, pipe, i):
        flag = _Flag()
        pipe._streams[i].queue.append(flag.set)
        return flag

    def poison(self, t):
        t.fill_(PO.POISON)

    def host(self, r):
        return torch.from_numpy(np.array(r)) if isinstance(r, np.ndarray) else r.detach().clone()

    def activity(self):
        return self.rt.calls


CONFIGS = {c.name: c for c in (
    CpuConfig("frame-copy_down", "frame"), CpuConfig("frame-zero_copy", "frame", zero_copy=True), CpuConfig("frame-on_device", "frame", download=False),
    CpuConfig("frame-planar", "frame", zero_copy=True, host=True), CpuConfig("site-copy_down", "site", host=True),
    CpuConfig("site-on_device", "site", download=False, host=True), CpuConfig("site-gains", "site", host=True, gains=PO.G1))}


def _run(monkeypatch, check, config, removed=None):
    rt = Runtime(removed)
    monkeypatch.setattr(pipeline, "_hip", rt)
    cfg = CONFIGS[config]
    made, make = [], cfg.make
    monkeypatch.setattr(cfg, "rt", rt)
    monkeypatch.setattr(cfg, "make", lambda **kw: made.append(make(**kw)) or made[-1])
    try:
        return PO.CHECKS[check](cfg, Queues(rt))
    finally:
        for p in made:  # the final drain: what is still queued runs download first, honouring waits only
            p.close()
            rt.drain(p)
            assert not any(s.queue for s in p._streams)


# ---- the stand-in runtime itself ------------------------------------------------------------------------------------------------------------------------------
def test_the_runtime_runs_the_minimal_set_only():
    rt = Runtime()
    a, b, c = (_Stream(rt, name) for name in ("s_up", "s_run", "s_down"))
    log, e1, e2, never = [], _Event(), _Event(), _Event()
    a.queue.append(lambda: log.append("a0"))
    rt.hipEventRecord(e1, a)
    a.queue.append(lambda: log.append("a1"))
    rt.hipStreamWaitEvent(b, never, 0)  # never recorded: complete, no wait
    rt.hipStreamWaitEvent(b, e1, 0)
    b.queue.append(lambda: log.append("b0"))
    rt.hipEventRecord(e2, b)
    rt.hipEventRecord(e1, a)  # re-recorded: a synchronise now means this record, the wait above keeps the first
    c.queue.append(lambda: log.append("c0"))
    rt.hipEventSynchronize(never)
    assert log == []
    rt.hipEventSynchronize(e2)
    assert log == ["a0", "b0"]  # not a1 (behind the record waited for), not c0
    rt.hipEventSynchronize(e1)
    assert log == ["a0", "b0", "a1"]
    c.synchronize()
    assert log == ["a0", "b0", "a1", "c0"] and not (a.queue or b.queue or c.queue)


def test_the_stand_in_launch_sees_every_argument():
    srcs = [_inputs(0, 0), _inputs(0, 1)]
    base = stand_in(srcs, 84, [1.0, 2.0], [5, 6])
    for other in (stand_in([srcs[0], _inputs(1, 1)], 84, [1.0, 2.0], [5, 6]), stand_in(srcs, 84, [1.0, float("nan")], [5, 6]), stand_in(srcs, 84, [1.0, 2.5], [5, 6]),
                  stand_in(srcs, 84, [1.0, 2.0], [5, 7]), stand_in(srcs, 84, [1.0, 2.0], [])):
        assert not np.array_equal(base, other)


# ---- the checks pass the pipelines as they are ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config,check", [(c, k) for c in sorted(CONFIGS) for k in sorted(PO.CHECKS) if PO.applies(k, CONFIGS[c])])
def test_the_checks_pass_the_pipelines(monkeypatch, config, check):
    _run(monkeypatch, check, config)


# ---- ... and fail what they are for: one call removed at a time ------------------------------------------------------------------------------------------------------
# removal -> (the named check that must fail, the configurations: both classes)
FAILS = {
    "the s_run wait": ("upload edge", ("frame-copy_down", "frame-zero_copy", "site-copy_down", "site-on_device")),
    "the s_down wait": ("run edge", ("frame-copy_down", "site-copy_down")),
    "the synchronise in result()": ("result wait", ("frame-copy_down", "frame-zero_copy", "frame-on_device", "site-copy_down", "site-on_device")),
    "the synchronise in next_input(s)()": ("slot reuse", ("frame-copy_down", "frame-zero_copy", "frame-on_device", "site-copy_down", "site-on_device")),
    "the record of ev_run": ("run edge", ("frame-copy_down", "frame-zero_copy", "frame-on_device", "site-copy_down", "site-on_device")),
    "the stream synchronise in close()": ("close() drains", ("frame-copy_down", "frame-zero_copy", "frame-on_device", "site-copy_down", "site-on_device")),
}


def test_every_removal_has_a_named_check():
    assert set(FAILS) == set(REMOVALS)
    for check, configs in FAILS.values():
        assert check in PO.CHECKS and {CONFIGS[c].site for c in configs} == {False, True}


@pytest.mark.parametrize("removed,config", [(r, c) for r in REMOVALS for c in FAILS[r][1]])
def test_a_removed_call_fails_its_check(monkeypatch, removed, config):
    with pytest.raises(AssertionError, match=config):  # (a message of the check: each names its configuration)
        _run(monkeypatch, FAILS[removed][0], config, removed)


@pytest.mark.parametrize("config", ["frame-copy_down", "site-copy_down"])
def test_the_other_slots_event_fails_the_upload_edge(monkeypatch, config):
    """A wait of s_run that names the other slot's upload event: that event's latest record is an earlier frame's (or none)."""
    wait = Runtime.hipStreamWaitEvent

    def other_slot(self, stream, event, flags):
        if stream.name == "s_run":
            pipe = sys._getframe(1).f_locals["self"]
            event = pipe.ev_up[1 - pipe.ev_up.index(event)]
        return wait(self, stream, event, flags)

    monkeypatch.setattr(Runtime, "hipStreamWaitEvent", other_slot)
    with pytest.raises(AssertionError, match=config):
        _run(monkeypatch, "upload edge", config)


@pytest.mark.parametrize("config", ["frame-planar", "site-copy_down", "site-on_device", "site-gains"])
def test_a_view_of_the_callers_array_fails_the_host_values(monkeypatch, config):
    """The host-value copy reverted to what the constructors had: np.ascontiguousarray of a contiguous float64 array of the pipeline's
    length is that array."""
    view = lambda v, n: np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)))  # noqa: E731
    a = np.array(SCALE)
    assert np.shares_memory(view(a, 3), a) and not np.shares_memory(pipeline._by_value(a, 3), a)
    assert pipeline._by_value(a, 3).flags.c_contiguous and pipeline._by_value(0.5, 3).tolist() == [0.5, 0.5, 0.5] and pipeline._by_value(a, 3).flags.writeable
    monkeypatch.setattr(pipeline, "_by_value", view)
    with pytest.raises(AssertionError, match=config):
        _run(monkeypatch, "host values by value", config)


def test_the_constructors_go_through_the_copy():
    """Both constructors make their host arrays with _by_value and with nothing else (the stand-in objects above are filled the same way):
    SitePipeline in __init__, FramePipeline in the builder of its prepared launches, which __init__ runs once per pipeline -- outside
    the loop over the slots."""
    import inspect
    for cls, n in ((pipeline.FramePipeline, 2), (pipeline.SitePipeline, 1)):
        text = inspect.getsource(cls.__init__) + inspect.getsource(cls._prepared)
        assert "_by_value(" not in text[text.index("\n        for ", text.index("def _prepared")):], cls.__name__
        assert text.count("_by_value(") == n and "ascontiguousarray" not in text, cls.__name__
        assert "by value" in cls.__init__.__doc__


@pytest.mark.parametrize("check", ["upload edge", "run edge", "result wait", "slot reuse", "close() drains", "set_gains by value"])
def test_a_delay_that_is_over_fails_the_precondition(monkeypatch, check):
    """The precondition is no tolerance: a commit() that returns after the delay fails the check, though every result is right."""
    commit = pipeline.SitePipeline.commit

    def commit_and_wait(self):
        commit(self)
        for stream in self._streams:
            stream.synchronize()

    monkeypatch.setattr(pipeline.SitePipeline, "commit", commit_and_wait)
    with pytest.raises(AssertionError, match="proves nothing"):
        _run(monkeypatch, check, "site-gains")
