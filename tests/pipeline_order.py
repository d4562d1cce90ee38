"""The order in which FramePipeline's and SitePipeline's work reaches the device, for tests/test_gpu_pipeline_order.py and
tests/test_pipeline_order_cpu.py -- TEST INFRASTRUCTURE ONLY, a plain module like tests/launch_contexts.py: no fixtures, no conftest.

Both classes stand on one ring (bev_amd.pipeline._Ring), which builds its own stream graph: three private streams (upload, run,
download), three rings of events, raw hipMemcpyAsync / hipEventRecord / hipStreamWaitEvent / hipEventSynchronize.  Four edges per slot carry the correctness -- the launch waits for the upload,
the download waits for the launch, result() waits for the slot's last event, next_input(s)() waits before the host overwrites a pinned slot
-- and close() has to drain the streams.  On idle streams a frame of a few KB is through before the host issues its next call, so every one
of those waits could be missing, or name the other slot's event, and a test that pushes frames through idle streams would still pass.

The checks below hold ONE private stream behind a delay (an event behind it says whether it is still running), poison with 77 the buffer a
missing edge would expose, drive the public methods, and compare with expectations that come from the numpy definitions under tests/ and
oracle.cpu_oracle, never from the device.  Where a check says "pending" it asserts, as a precondition, that the delay was still running
when commit() returned: a run whose delay was over proves nothing (launch_contexts.check_side_stream's rule, and no tolerance).  From the
references alone each check also asserts that a frame's expectation is neither what a poisoned buffer gives nor the neighbouring frame's.

A check is written once and driven by a configuration and a backend:

  configuration  name, site (SitePipeline?), copy_down (result() waits for the download's event), has_host (scale / bias / border),
                 make(host=None, gains=DEFAULT) -> a pipeline of depth 2, inputs(i) -> the host arrays of frame (set) i, one per pinned
                 buffer, expected(i, gains=DEFAULT), expected_of_poisoned_input(gains=DEFAULT), compare(got, exp, what), host_values()
  backend        delay(pipe, i) -> an object with query(), poison(tensor), host(result) -> a CPU tensor of its own, activity()

GpuConfig / Gpu are the real pipelines on launch_contexts' shapes; tests/test_pipeline_order_cpu.py holds a stand-in runtime whose streams
are queues, so that each check is shown on the CPU to fail what it is for."""
import contextlib
import time

import numpy as np
import torch

POISON = 77
UP, RUN, DOWN = 0, 1, 2  # indices into pipe._streams
DEFAULT = "the configuration's own gains"
G1 = [[1.25, 0.8, 0.6], [0.5, 2.0, 1.5]]  # per camera, per channel, none of them 1
G2 = [[0.7, 1.9, 1.1], [3.5, 0.9, 0.2]]
N_FRAMES = 5


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------------------
def differ(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape != b.shape or not np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def assert_references_tell(cfg, n, gains=DEFAULT):
    """From the references alone: the first n expectations are no poison, not what poisoned inputs give, and differ from their neighbours."""
    exps = [cfg.expected(i, gains) for i in range(n)]
    for i, e in enumerate(exps):
        assert not (np.asarray(e) == POISON).all(), "%s: frame %d's expectation is the poison" % (cfg.name, i)
        assert differ(e, cfg.expected_of_poisoned_input(gains)), "%s: frame %d's expectation is a poisoned input's" % (cfg.name, i)
        assert i == 0 or differ(exps[i - 1], e), "%s: frames %d and %d have one expectation" % (cfg.name, i - 1, i)


def fill(pipe, cfg, i, bufs=None):
    """Frame (set) i into the next pinned buffers."""
    if bufs is None:
        bufs = pipe.next_inputs() if cfg.site else [pipe.next_input()]
    arrays = cfg.inputs(i)
    assert len(bufs) == len(arrays)
    for b, a in zip(bufs, arrays):
        assert b.shape == a.shape and b.dtype == a.dtype
        np.copyto(b, a)


def next_slot(pipe):
    return pipe.n_in % pipe.depth


def device_inputs(pipe, cfg, slot):
    return list(pipe.d_in[slot]) if cfg.site else [pipe.d_in[slot]]


def result_buffers(pipe, slot):
    """The slot's device result and (download) its pinned host slot: whichever of them result() hands out, last."""
    return [pipe.d_out[slot]] + ([pipe.h_out[slot]] if pipe.h_out is not None else [])


def commit_behind(pipe, cfg, e):
    """commit() with the delay `e` in front of one of its streams; returns the host seconds it took."""
    t0 = time.perf_counter()
    pipe.commit()
    host_s = time.perf_counter() - t0
    assert not e.query(), "%s: the delay was over when commit() returned after %.1f ms: this run proves nothing" % (cfg.name, host_s * 1e3)
    return host_s


def take(pipe, cfg, backend, exp, what):
    cfg.compare(backend.host(pipe.result()), exp, "%s: %s" % (cfg.name, what))


@contextlib.contextmanager
def made(cfg, **kw):
    pipe = cfg.make(**kw)
    try:
        yield pipe
    finally:
        pipe.close()


# ---- the checks -----------------------------------------------------------------------------------------------------------------------------------------
def _edge(cfg, backend, stream, poisoned, complete_at_result=False):
    """Frames 0 and 1 (both slots of the ring), each committed with `stream` held behind a delay and `poisoned(pipe, slot)` filled with
    77.  Returns the host seconds of the commits."""
    assert_references_tell(cfg, 2)
    times = []
    with made(cfg) as pipe:
        for i in range(2):
            for t in poisoned(pipe, next_slot(pipe)):
                backend.poison(t)
            fill(pipe, cfg, i)
            e = backend.delay(pipe, stream)
            times.append(commit_behind(pipe, cfg, e))
            got = pipe.result()
            if complete_at_result:
                assert e.query(), "%s: result() of frame %d returned while the delay in front of its last event was still running" % (cfg.name, i)
            cfg.compare(backend.host(got), cfg.expected(i), "%s: frame %d" % (cfg.name, i))
    return times


def check_upload_edge(cfg, backend):
    """The launch waits for the upload: the upload stream is held back and the device input is poisoned -- a launch that does not wait
    (or waits for the other slot's event) warps 77s."""
    return _edge(cfg, backend, UP, lambda pipe, slot: device_inputs(pipe, cfg, slot))


def check_run_edge(cfg, backend):
    """The download waits for the launch: the run stream is held back and the results are poisoned -- a download that does not wait
    copies 77s down."""
    return _edge(cfg, backend, RUN, result_buffers)


def check_result_wait(cfg, backend):
    """result() waits for the slot's LAST event: the download's with a copy down, the launch's otherwise.  The stream that event is
    recorded on is held back; result() may return only when the delay is over, with the frame."""
    return _edge(cfg, backend, DOWN if cfg.copy_down else RUN, result_buffers, complete_at_result=True)


def check_slot_reuse(cfg, backend):
    """next_input(s)() of a slot whose upload has not happened yet blocks: the upload stream is held back, both slots are committed, and the
    buffer of frame 2 is asked for -- it is frame 0's.  Filled with frame 2 at once, frame 0's result is still frame 0's."""
    assert_references_tell(cfg, 3)
    times = []
    with made(cfg) as pipe:
        fill(pipe, cfg, 0)
        e = backend.delay(pipe, UP)
        times.append(commit_behind(pipe, cfg, e))
        fill(pipe, cfg, 1)
        times.append(commit_behind(pipe, cfg, e))
        bufs = pipe.next_inputs() if cfg.site else [pipe.next_input()]
        assert e.query(), "%s: next_input() handed out slot 0 while its upload was still waiting behind the delay" % cfg.name
        fill(pipe, cfg, 2, bufs)
        take(pipe, cfg, backend, cfg.expected(0), "frame 0 after its pinned slot was refilled with frame 2")
        pipe.commit()
        take(pipe, cfg, backend, cfg.expected(1), "frame 1")
        take(pipe, cfg, backend, cfg.expected(2), "frame 2")
    return times


def check_close_drains(cfg, backend):
    """close() without result(): when it returns the streams are drained -- the delay is over and the result buffer, to which the test keeps
    its own reference, holds the frame.  A second close() does nothing."""
    assert_references_tell(cfg, 1)
    pipe = cfg.make()
    try:
        kept = result_buffers(pipe, 0)
        for t in kept:
            backend.poison(t)
        fill(pipe, cfg, 0)
        e = backend.delay(pipe, UP)
        times = [commit_behind(pipe, cfg, e)]
        pipe.close()
        assert e.query(), "%s: close() returned while the delay was still running: the buffers could be freed under the streams" % cfg.name
        cfg.compare(backend.host(kept[-1]), cfg.expected(0), "%s: the result buffer after close()" % cfg.name)
        before = backend.activity()
        assert pipe.close() is None and backend.activity() == before, "%s: a second close() reached the runtime" % cfg.name
    finally:
        pipe.close()
    return times


def check_run_in_order(cfg, backend):
    """run() over five frames through the ring of two, a different stream held back before each submit: the results in order."""
    assert_references_tell(cfg, N_FRAMES)
    with made(cfg) as pipe:
        def frames():
            for i in range(N_FRAMES):
                backend.delay(pipe, (UP, RUN, DOWN)[i % 3])
                arrays = cfg.inputs(i)
                yield arrays if cfg.site else arrays[0]

        got = [backend.host(r) for r in pipe.run(frames())]  # (a copy at once: a result is a view of the ring)
    assert len(got) == N_FRAMES
    for i, g in enumerate(got):
        cfg.compare(g, cfg.expected(i), "%s: frame %d of run()" % (cfg.name, i))
    return []


def check_host_values(cfg, backend):
    """scale, bias and border_value are taken by value: contiguous float64 arrays of exactly the pipeline's length -- what
    np.ascontiguousarray hands back as it is -- overwritten with NaNs once the constructor has returned."""
    assert cfg.has_host
    assert_references_tell(cfg, 3)
    values = cfg.host_values()
    with made(cfg, host=values) as pipe:
        for a in values.values():
            assert a.dtype == np.float64 and a.ndim == 1 and a.flags.c_contiguous and np.isfinite(a).all()
            a[...] = np.nan  # what the caller may do with its arrays once the constructor has returned
        for i in range(3):
            fill(pipe, cfg, i)
            pipe.commit()
            take(pipe, cfg, backend, cfg.expected(i), "frame %d after the caller's arrays were overwritten" % i)
    return []


def check_set_gains(cfg, backend):
    """set_gains between two commits, with the first still waiting behind a delay on the run stream: the committed set keeps the gains it
    was committed with, the next one has the new ones, and neither reads the caller's arrays again."""
    assert cfg.site
    for i, g in ((0, G1), (1, G2)):
        assert not (np.asarray(cfg.expected(i, g)) == POISON).all()
        assert differ(cfg.expected(i, g), cfg.expected(i, G2 if g is G1 else G1)) and differ(cfg.expected(i, g), cfg.expected(i, None))
    assert differ(cfg.expected(0, G1), cfg.expected(1, G1))
    g1, g2 = np.array(G1, dtype=np.float64), np.array(G2, dtype=np.float64)
    with made(cfg, gains=g1) as pipe:
        for t in result_buffers(pipe, 0) + result_buffers(pipe, 1):
            backend.poison(t)
        fill(pipe, cfg, 0)
        e = backend.delay(pipe, RUN)
        times = [commit_behind(pipe, cfg, e)]
        pipe.set_gains(g2)
        g1[...] = np.nan
        g2[...] = np.nan
        assert not e.query(), "%s: the delay was over when set_gains() returned: this run proves nothing" % cfg.name
        fill(pipe, cfg, 1)
        times.append(commit_behind(pipe, cfg, e))
        take(pipe, cfg, backend, cfg.expected(0, G1), "set 0, committed under the first gains")
        take(pipe, cfg, backend, cfg.expected(1, G2), "set 1, committed after set_gains")
    return times


CHECKS = {"upload edge": check_upload_edge, "run edge": check_run_edge, "result wait": check_result_wait, "slot reuse": check_slot_reuse,
          "close() drains": check_close_drains, "run() in order": check_run_in_order, "host values by value": check_host_values,
          "set_gains by value": check_set_gains}


def applies(check, cfg):
    return cfg.has_host if check == "host values by value" else cfg.site if check == "set_gains by value" else True


# ---- the GPU backend and the real pipelines ---------------------------------------------------------------------------------------------------------------
class Gpu:
    """Real streams: the delay is a torch.cuda._sleep of `sleep_cycles` on the pipeline's own stream, with an event behind it."""

    def __init__(self, sleep_cycles):
        self.sleep_cycles = int(sleep_cycles)

    def delay(self, pipe, i):
        with torch.cuda.stream(pipe._streams[i]):
            torch.cuda._sleep(self.sleep_cycles)
            e = torch.cuda.Event()
            e.record()
        return e

    def poison(self, t):
        t.fill_(POISON)
        if t.is_cuda:
            torch.cuda.synchronize(t.device)

    def host(self, r):
        return torch.from_numpy(np.array(r)) if isinstance(r, np.ndarray) else r.detach().cpu().clone()

    def activity(self):
        return 0


def same_bytes(got, exp, what):
    np.testing.assert_array_equal(got.numpy(), exp, err_msg=what)


def same_planes(dtype):
    from tests import remap_nv12_ref as RN

    def compare(got, exp, what):
        assert got.dtype == dtype, what
        RN.assert_planes_equal(got, exp, dtype, what)
    return compare


class GpuConfig:
    """A real pipeline of depth 2 on launch_contexts' shapes (40 x 24 sources, 36 x 20 destinations, its matrices, maps and cameras).
    kind "frame" / "site"; kw: the constructor's keywords; expected_of(arrays, G) -> the expectation of one frame (set) from the numpy
    definitions, G the quantised gains (256s: none)."""

    def __init__(self, name, kind, kw, inputs, expected_of, compare=same_bytes, has_host=False, gains=None):
        self.name, self.site, self.kw, self._inputs, self._expected_of, self.compare, self.has_host, self.gains = name, kind == "site", kw, inputs, expected_of, compare, has_host, gains
        self.copy_down = kw.get("download", True) and not (kind == "frame" and kw.get("zero_copy_out", True))
        self._cache = {}

    def __repr__(self):
        return self.name

    def host_values(self):
        from tests import launch_contexts as LC
        values = dict(scale=np.array(LC.SCALE, dtype=np.float64), bias=np.array(LC.BIAS, dtype=np.float64))
        if self.site:
            values["border_value"] = np.array(LC.BORDER, dtype=np.float64)
        return values

    def make(self, host=None, gains=DEFAULT):
        from bev_amd import pipeline
        from tests import launch_contexts as LC
        kw = dict(self.kw, depth=2)
        host = dict(host or {})
        if self.site:
            kw.update(border_value=LC.BORDER, scale=LC.SCALE, bias=LC.BIAS, gains=self.gains if gains is DEFAULT else gains)
            kw.update(host)
            return pipeline.SitePipeline([(LC.SH, LC.SW)] * 2, [one_frame_map(0), one_frame_map(1)], LC.DSIZE, blend="feather", feather=LC.FEATHER, **kw)
        if kw.get("planar"):
            kw.update(scale=LC.SCALE, bias=LC.BIAS)
            kw.update(host)
        if kw.pop("mapped", False):
            return pipeline.FramePipeline((LC.SH, LC.SW), 3, None, LC.DSIZE, warp_map=one_frame_map("A"), **kw)
        return pipeline.FramePipeline((LC.SH, LC.SW), 3, LC.MINVS["A"][0], LC.DSIZE, flags=LC.FLAGS, **kw)

    def inputs(self, i):
        return self._inputs(i)

    def _quantised(self, gains):
        from tests import stitch_gain_ref as SG
        gains = self.gains if gains is DEFAULT else gains
        return SG.quantize(np.ones((2, 3)) if gains is None else gains, 2)

    def _cached(self, key, arrays, gains):
        G = self._quantised(gains)
        key = (key, G.tobytes())
        if key not in self._cache:
            e = np.ascontiguousarray(self._expected_of(arrays, G))
            e.setflags(write=False)
            self._cache[key] = e
        return self._cache[key]

    def expected(self, i, gains=DEFAULT):
        """Computed once per frame and gains, shared by the checks, and left unchanged."""
        return self._cached(i, self.inputs(i), gains)

    def expected_of_poisoned_input(self, gains=DEFAULT):
        return self._cached("poison", [np.full_like(a, POISON) for a in self.inputs(0)], gains)


_maps = {}


def one_frame_map(key):
    """The WarpMap of frame 0 of launch_contexts.ref_maps(key) on cuda:0 (the pipelines take maps of one frame), built once by
    build_warp_map and checked against the reference by bits."""
    from bev_amd import warp as W
    from tests import launch_contexts as LC
    if key not in _maps:
        Ms = LC.MINVS[key] if key in LC.MINVS else LC.CAM_MINVS[key]
        m = W.build_warp_map(Ms[:1], LC.DSIZE, flags=LC.FLAGS, device="cuda:0")
        torch.cuda.synchronize()
        exy, efrac = LC.ref_maps(key)[0]
        assert m.n == 1
        np.testing.assert_array_equal(m.xy.cpu().numpy()[0], exy)
        np.testing.assert_array_equal(m.frac.cpu().numpy().view(np.uint16)[0], efrac)
        _maps[key] = m
    return _maps[key]


def gpu_configs():
    """The eight configurations of tests/test_gpu_pipeline_order.py.  Nothing here touches a device: the maps are built when a pipeline is."""
    from oracle import cpu_oracle as co
    from tests import launch_contexts as LC
    from tests import nv12_ref as NR
    from tests import remap_nv12_out_ref as RNO
    from tests import remap_nv12_ref as RN
    from tests import remap_ref as RR
    from tests import stitch_gain_ref as SG
    from tests import stitch_maps_ref as SM
    from tests import workloads as wl
    cache = {}

    def bgr(i, camera=0):  # (frames 0 and 1 are launch_contexts' set A)
        if ("bgr", i, camera) not in cache:
            a = wl.frame(500 + i + 100 * camera, LC.SH, LC.SW, np.uint8)
            a.setflags(write=False)
            cache[("bgr", i, camera)] = a
        return cache[("bgr", i, camera)]

    def nv12(i, camera=0):
        if ("nv12", i, camera) not in cache:
            a = NR.join(*NR.frame("phase", 40 + i + 100 * camera, LC.SH, LC.SW))
            a.setflags(write=False)
            cache[("nv12", i, camera)] = a
        return cache[("nv12", i, camera)]

    def split(a):
        return a[:LC.SH], a[LC.SH:].reshape(LC.SH // 2, LC.SW // 2, 2)

    M = LC.MINVS["A"][0]
    refs = lambda: [LC.ref_maps(0)[0], LC.ref_maps(1)[0]]  # noqa: E731
    warped = lambda arrays, G: co.warp_perspective(arrays[0], M, LC.DSIZE, co.LINEAR, m_is_inverse=True)  # noqa: E731
    one_bgr, one_nv12 = (lambda i: [bgr(i)]), (lambda i: [nv12(i)])
    two_bgr, two_nv12 = (lambda i: [bgr(i, 0), bgr(i, 1)]), (lambda i: [nv12(i, 0), nv12(i, 1)])
    stitch = (SM.FEATHER, LC.FEATHER)

    def site_nv12_planes(arrays, G):
        ys, uvs = zip(*[split(a) for a in arrays])
        return SG.stitch_nv12_planes(ys, uvs, G, refs(), LC.LINEAR, LC.SCALE, LC.BIAS, *stitch, LC.BORDER)

    return [
        GpuConfig("frame-bgr-copy_down", "frame", dict(zero_copy_out=False), one_bgr, warped),
        GpuConfig("frame-bgr-zero_copy", "frame", dict(zero_copy_out=True), one_bgr, warped),
        GpuConfig("frame-bgr-on_device", "frame", dict(download=False), one_bgr, warped),
        GpuConfig("frame-planar-float16", "frame", dict(planar=True, plane_dtype=torch.float16), one_bgr,
                  lambda arrays, G: RN.planes_f32(warped(arrays, G), LC.SCALE, LC.BIAS), same_planes(torch.float16), has_host=True),
        GpuConfig("frame-nv12-to-nv12-mapped", "frame", dict(mapped=True, src_format="nv12", dst_format="nv12", zero_copy_out=False), one_nv12,
                  lambda arrays, G: NR.join(*RNO.remap_nv12_to_nv12(*split(arrays[0]), *LC.ref_maps("A")[0], LC.LINEAR, RR.CONSTANT, 0.0))),
        GpuConfig("site-bgr", "site", dict(), two_bgr,
                  lambda arrays, G: SG.stitch(arrays, G, refs(), LC.LINEAR, *stitch, SM.CONSTANT, LC.BORDER)[0], has_host=True),
        GpuConfig("site-nv12-to-planes-on_device", "site", dict(src_format="nv12", dst_format="planes", download=False), two_nv12, site_nv12_planes,
                  same_planes(torch.float32), has_host=True),
        GpuConfig("site-bgr-to-nv12-gains", "site", dict(dst_format="nv12"), two_bgr,
                  lambda arrays, G: NR.join(*SG.stitch_to_nv12(arrays, G, refs(), LC.LINEAR, *stitch, LC.BORDER)), has_host=True, gains=G1),
    ]
