"""tests/launch_contexts.py on the CPU: its table is complete against the ABI, every case's preconditions hold on the host, and its checks
notice what they are for -- driven with CPU tensors, stand-in entries and a backend whose streams are queues, in the manner of
tests/test_parity_helper.py.  This stands where a GPU mutation run would: nothing here, and nothing on the GPU, launches on a wrong stream
or breaks a launch on purpose."""
import contextlib

import numpy as np
import pytest
import torch

from bev_amd import _lib
from tests import launch_contexts as LC

# symbol -> the test that captures it into a graph (and launches it on a side stream) already
COVERED_ELSEWHERE = {
    "bevwarp_warp": "tests/test_gpu_warp.py, tests/test_gpu_geom.py::test_config5_full_step_eager_and_graphed",
    "bevwarp_warp_classes": "tests/test_gpu_warp.py (a plan that carries a verdict table, captured and on two streams)",
    "bevwarp_warp_border": "tests/test_gpu_border.py::test_graph_capture_replicate, tests/test_gpu_cubic.py",
    "bevwarp_tracker_step": "tests/test_gpu_geom.py::test_config5_full_step_eager_and_graphed",
    "bevwarp_composite": "tests/test_gpu_geom.py::test_composite_maps_survive_cache_churn_under_a_captured_graph",
    "bevwarp_warp_composite": "tests/test_gpu_geom.py::test_composite_maps_survive_cache_churn_under_a_captured_graph",
}
# symbols that enqueue nothing a caller could capture: host arithmetic and queries, and the footprint, whose counts come back to the host
NOT_A_LAUNCH = ["bevwarp_version", "bevwarp_strerror", "bevwarp_last_hip_error", "bevwarp_invert_homography", "bevwarp_tile_classes_bytes", "bevwarp_footprint"]
# launching symbols without a case: tests/ holds no numpy definition their results equal by bits (tests/test_gpu_geom.py and
# tests/test_gpu_axes.py compare them within 1e-12), and the table compares by bits only
NO_BITWISE_DEFINITION = ["bevwarp_rbox_iou", "bevwarp_rbox_transform"]


def test_the_table_covers_every_symbol_of_the_abi():
    """A new entry point fails this until it has a case (or a reason under one of the three lists above)."""
    with_case = {c.symbol for c in LC.CASES}
    groups = [with_case, set(COVERED_ELSEWHERE), set(NOT_A_LAUNCH), set(NO_BITWISE_DEFINITION)]
    for i, a in enumerate(groups):
        for b in groups[:i]:
            assert not a & b, a & b
    assert set().union(*groups) == set(_lib.SYMBOLS), set().union(*groups) ^ set(_lib.SYMBOLS)
    names = [c.name for c in LC.CASES]
    assert len(set(names)) == len(names)
    by_name = {c.name: c for c in LC.CASES}
    for name in ("remap", "remap_stitch", "warp_stitch", "warp_perspective_lens"):
        assert by_name[name] in LC.COPIED_SOURCE
    assert {c.symbol for c in LC.NO_OUT} == {"bevwarp_warp_lens", "bevwarp_remap", "bevwarp_remap_nv12", "bevwarp_warp_stitch", "bevwarp_stitch_maps",
                                             "bevwarp_stitch_maps_nv12"}


@pytest.mark.parametrize("case", LC.CASES, ids=repr)
def test_preconditions_hold_on_the_host(case):
    """The two sets give different results (both replays, and the side stream, tell them apart); a stitch's pixels are covered 0, 1 and 2
    times; a no_out case writes some pixels of every frame and leaves some; expected results have the destination's shapes and hold no 77s
    only (a poisoned destination cannot pass)."""
    case.assert_preconditions()  # (what the GPU tests assert again before they run a case)
    exp_a, exp_b = case.expected("A", "A"), case.expected("B", "B")
    assert LC.differ(exp_a, exp_b)
    if case.inputs("A"):
        assert LC.differ(exp_a, case.expected("B", "A"))
        assert all(a.shape == b.shape and a.dtype == b.dtype for a, b in zip(case.inputs("A"), case.inputs("B")))
        assert all(set(case.host("A")) == set(case.host("B")) and np.array_equal(case.host("A")[k], v) for k, v in case.host("B").items())
    shapes = case.out_shapes or LC.PX
    assert [tuple(e.shape) for e in exp_a] == [tuple(s) for s, _ in shapes]
    for e in exp_a + exp_b:
        assert not (e == LC.POISON).all()
    for a in case.host("A").values():
        assert a.dtype == np.float64 and np.isfinite(a).all()  # (a NaN written over it afterwards is another value)
    if case.cover is not None:
        count = case.cover()
        assert count.shape == (LC.BATCH, LC.DH, LC.DW)
        for c in count:
            assert set(np.unique(c)) == {0, 1, 2}
    if case.no_out:
        written = case.written()
        assert written.shape == (LC.BATCH, LC.DH, LC.DW)
        for w, e in zip(written, exp_a[0]):
            assert w.any() and not w.all()
            assert (e[~w] == 0).all() and (e[w] != 0).any()  # the result starts from zeros: unwritten pixels are 0, not the poison
    else:
        assert case.written is None


# ---- what the second-device context is for, as far as a machine without devices can show it ---------------------------------------------------------
class _Plane:
    """What build_warp_map asks of a map plane, on a device that need not exist."""
    dtype = torch.int16

    def __init__(self, shape, device):
        self.shape, self.device = tuple(shape), torch.device(device)

    def stride(self, i):
        return int(np.prod(self.shape[i + 1:]))

    def data_ptr(self):
        return 4096


def _map_on(device):
    from bev_amd import warp as W
    m = W.WarpMap.__new__(W.WarpMap)
    m.xy, m.frac, m.interp, m.dsize = _Plane((1, 6, 5, 2), device), _Plane((1, 6, 5), device), W.INTER_LINEAR, (5, 6)
    return m


def test_build_warp_map_uploads_its_matrices_to_the_maps_device(monkeypatch):
    """build_warp_map(M, dsize, out=a map on cuda:1) with cuda:0 current: `device` defaults to a bare "cuda", and the matrices must not go
    to the current device -- the launch on cuda:1 would read them through an address of cuda:0."""
    from bev_amd import warp as W
    seen = []

    def device_inverse(M, device, inverse_given=False):
        seen.append(("matrices", torch.device(device)))
        return _Plane((1, 3, 3), device)

    monkeypatch.setattr(W, "device_inverse", device_inverse)
    monkeypatch.setattr(W._lib, "launch", lambda name, device, *args: seen.append((name, torch.device(device))))
    one = torch.device("cuda:1")
    for device in ({}, dict(device="cuda"), dict(device="cuda:1"), dict(device=one)):
        del seen[:]
        out = _map_on(one)
        assert W.build_warp_map(np.eye(3), (5, 6), out=out, **device) is out
        assert seen == [("matrices", one), ("bevwarp_build_map", one)], seen
    with pytest.raises(ValueError, match="out is on cuda:1, device is cuda:0"):
        W.build_warp_map(np.eye(3), (5, 6), out=_map_on(one), device="cuda:0")
    with pytest.raises(ValueError, match="out must be a WarpMap"):
        W.build_warp_map(np.eye(3), (5, 6), out=_map_on("cpu"))
    assert seen == [("matrices", one), ("bevwarp_build_map", one)]  # (the refused calls asked for nothing)


# ---- the checks against stand-ins ----------------------------------------------------------------------------------------------------------------
class Queues:
    """A backend without a GPU.  Work submitted on the default stream runs at once (the stream is idle: every check synchronises before
    it looks); work submitted inside side_stream() waits in the stream's queue until the stream is synchronised, the delay first; work
    submitted during capture() is recorded and runs at every replay."""
    device = torch.device("cpu")

    def __init__(self):
        self.stream, self.recording = None, None

    def submit(self, work):
        if self.recording is not None:
            self.recording.append(work)
        elif self.stream is not None:
            self.stream.queue.append(work)
        else:
            work()

    def empty(self, shape, dtype):
        return torch.zeros(tuple(shape), dtype=dtype)

    def staged(self, a):
        return torch.from_numpy(np.array(a))

    def copy_async(self, t, staged):
        self.submit(lambda: t.copy_(staged))

    def fill(self, t, value):
        self.submit(lambda: t.fill_(value))

    def synchronize(self):
        pass

    @contextlib.contextmanager
    def side_stream(self):
        outer, self.stream = self.stream, _Stream()
        try:
            yield self.stream
        finally:
            self.stream = outer

    def delay(self):
        e = _Event()
        self.submit(e.set)
        return e

    def capture(self, thunk):
        self.recording = []
        try:
            ret = thunk()
            return ret, _Graph(self.recording)
        finally:
            self.recording = None


class _Stream:
    def __init__(self):
        self.queue = []

    def synchronize(self):
        while self.queue:
            self.queue.pop(0)()


class _Event:
    done = False

    def set(self):
        self.done = True

    def query(self):
        return self.done


class _Graph:
    def __init__(self, works):
        self.works = list(works)

    def replay(self):
        for w in self.works:
            w()


def _ref(src, border):
    return (src * np.float32(2.0) + np.float32(border[0])).astype(np.float32)


class StandIn:
    """A case whose entry is dst = src * 2 + border[0] in float32 on CPU tensors.  `how` says what the entry does wrong."""
    name, symbol, sliceable, no_out, written, cover = "stand-in", None, (), False, None, None
    out_shapes = [((2, 4, 5), torch.float32)]

    def __init__(self, backend, how="honest"):
        self.backend, self.how = backend, how

    def inputs(self, which):
        return (np.random.default_rng(3 + LC.SETS.index(which)).random((2, 4, 5), dtype=np.float32),)

    def host(self, which="A"):
        return {"border": np.array([9.0, 200.0, 31.0])}

    def resident(self, device):
        return None

    def expected(self, which, host_which="A"):
        return [_ref(self.inputs(which)[0], self.host()["border"])]

    def compare(self, got, exp):
        np.testing.assert_array_equal(got[0].cpu().numpy(), exp[0])

    def call(self, tensors, resident, host, outs):
        src, dst, border = tensors[0], outs[0], host["border"]
        how, submit = self.how, self.backend.submit
        by_value = float(border[0])  # an honest entry takes the value when it is called
        if how == "honest":
            submit(lambda: dst.copy_(src * 2 + by_value))
        elif how == "wrong stream":  # the launch goes to the idle default stream: it runs at once, on what the inputs hold now
            if self.backend.recording is None:
                dst.copy_(src * 2 + by_value)
            else:
                submit(lambda: dst.copy_(src * 2 + by_value))
        elif how == "ignores rewritten inputs":  # (a staging copy that is no node of the graph)
            kept = src.clone()
            submit(lambda: dst.copy_(kept * 2 + by_value))
        elif how == "re-reads its host border":  # (a host pointer that outlives the call)
            submit(lambda: dst.copy_(src * 2 + float(border[0])))
        elif how == "leaves the destination untouched":
            submit(lambda: None)
        elif how == "runs while it is captured":
            dst.copy_(src * 2 + by_value)
            submit(lambda: dst.copy_(src * 2 + by_value))
        elif how == "waits for its stream":  # the host blocks until the delay is over: the side-stream run would prove nothing
            submit(lambda: dst.copy_(src * 2 + by_value))
            if self.backend.stream is not None:
                self.backend.stream.synchronize()
        else:
            raise ValueError(how)
        return [dst]


class AllocatingStandIn(StandIn):
    """The no_out shape: the entry allocates its result and zero-fills it -- as a node of the graph, or ("zeroes once") when it is called only --
    and writes the pixels of the upper half."""
    name, no_out, out_shapes = "allocating stand-in", True, None

    def expected(self, which, host_which="A"):
        e = _ref(self.inputs(which)[0], self.host()["border"])
        e[:, 2:] = 0
        return [e]

    def call(self, tensors, resident, host, outs):
        assert outs is None
        src, by_value, submit = tensors[0], float(host["border"][0]), self.backend.submit
        dst = torch.empty((2, 4, 5), dtype=torch.float32)
        if self.how == "zeroes once":
            dst.zero_()
        else:
            submit(lambda: dst.zero_())
        submit(lambda: dst[:, :2].copy_(src[:, :2] * 2 + by_value))
        return [dst]


def _stand_in(how="honest", kind=StandIn):
    backend = Queues()
    return kind(backend, how), backend


def test_the_checks_pass_an_honest_entry():
    case, backend = _stand_in()
    assert LC.check_side_stream(case, backend) >= 0.0
    LC.check_replays(case, backend)
    case, backend = _stand_in(kind=AllocatingStandIn)
    LC.check_replays(case, backend)
    LC.check_side_stream(case, backend)


@pytest.mark.parametrize("how", ["ignores rewritten inputs", "re-reads its host border", "leaves the destination untouched", "runs while it is captured"])
def test_the_replays_fail_a_wrong_entry(how):
    case, backend = _stand_in(how)
    with pytest.raises(AssertionError, match="the capture itself wrote" if how == "runs while it is captured" else "replay on set B"):
        LC.check_replays(case, backend)


def test_the_replays_fail_a_zero_fill_outside_the_graph():
    case, backend = _stand_in("zeroes once", AllocatingStandIn)
    with pytest.raises(AssertionError, match="replay on set B"):
        LC.check_replays(case, backend)


@pytest.mark.parametrize("how", ["wrong stream", "leaves the destination untouched"])
def test_the_side_stream_fails_a_wrong_entry(how):
    case, backend = _stand_in(how)
    with pytest.raises(AssertionError):
        LC.check_side_stream(case, backend)


def test_the_side_stream_fails_a_wrong_stream_that_reads_the_earlier_set():
    """Without the poison behind the delay, a launch on another stream would still show: it reads set A."""
    case, backend = _stand_in("wrong stream")
    fill, backend.fill = backend.fill, lambda t, value: fill(t, value) if backend.stream is None else None
    with pytest.raises(AssertionError):
        LC.check_side_stream(case, backend)


def test_the_side_stream_fails_a_run_whose_delay_was_over():
    """The precondition is no tolerance: a call that returns after the delay fails the case, though its result is right."""
    case, backend = _stand_in("waits for its stream")
    with pytest.raises(AssertionError, match="proves nothing"):
        LC.check_side_stream(case, backend)
