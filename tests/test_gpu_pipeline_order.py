"""The stream ordering of FramePipeline and SitePipeline on the GPU (tests/pipeline_order.py holds the configurations and the checks;
tests/test_pipeline_order_cpu.py shows on the CPU that each check fails what it is for):

  upload edge, run edge   one private stream held behind a delay of about 50 ms, the buffer a missing wait would expose poisoned with 77,
                          both slots of a ring of two
  result wait             the stream of the slot's last event held back: result() returns with the delay over, and with the frame
  slot reuse              both slots committed behind a held-back upload stream: next_input(s)() of the third frame blocks
  close() drains          a frame committed and never taken: the result buffer holds it when close() returns
  run() in order          five frames through the ring, a different stream held back before each submit
  host values, set_gains  the caller's scale / bias / border value / gains arrays overwritten with NaNs once the call has returned

Real pipelines on launch_contexts' shapes (40 x 24 sources, 36 x 20 destinations, its matrices, maps and two overlapping cameras), every
result compared by bits with the numpy definitions under tests/ and oracle.cpu_oracle.  The tests are positive only: no edge is removed
here, every delay stands in front of a commit() that completes.  Run on the GPU box:  python -m pytest tests -m gpu -q"""
import pytest
import torch

from tests import launch_contexts as LC
from tests import pipeline_order as PO

pytestmark = pytest.mark.gpu

CONFIGS = PO.gpu_configs()


@pytest.fixture(scope="module")
def delay():
    """(cycles, milliseconds) of the delay every check holds a stream behind: measured once, scaled to about 50 ms, measured again."""
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    cycles, ms = LC.sleep_cycles_for(50.0)
    print("torch.cuda._sleep(%d) takes %.1f ms" % (cycles, ms))
    assert ms >= 20.0, "the delay came out at %.2f ms: too short to enqueue a commit behind" % ms
    return cycles, ms


@pytest.mark.parametrize("cfg,check", [(c, k) for c in CONFIGS for k in PO.CHECKS if PO.applies(k, c)], ids=str)
def test_pipeline_order(cfg, check, delay):
    cycles, ms = delay
    times = PO.CHECKS[check](cfg, PO.Gpu(cycles))
    print("%s, %s: delay %.1f ms, commit() took %s ms on the host" % (cfg.name, check, ms, ", ".join("%.3f" % (t * 1e3) for t in times) or "-- (no commit is timed)"))


def test_the_configurations():
    """What the module is said to run, and that result() waits where the table says."""
    by_name = {c.name: c for c in CONFIGS}
    assert len(by_name) == len(CONFIGS) == 8
    assert [c.name for c in CONFIGS if c.copy_down] == ["frame-bgr-copy_down", "frame-nv12-to-nv12-mapped", "site-bgr", "site-bgr-to-nv12-gains"]
    with by_name["frame-bgr-zero_copy"].make() as pipe:
        assert pipe.zero_copy_out and pipe.download and pipe.depth == 2
    with by_name["frame-bgr-copy_down"].make() as pipe:
        assert not pipe.zero_copy_out and pipe.download
    with by_name["site-nv12-to-planes-on_device"].make() as pipe:
        assert not pipe.download and pipe.h_out is None and pipe.nv12 and pipe.d_out[0].dtype == torch.float32
    with by_name["site-bgr-to-nv12-gains"].make() as pipe:
        assert pipe.gains == PO.G1 and pipe._launch[0][1][pipe._blend_at] & 0x100
    with by_name["frame-planar-float16"].make() as pipe:
        assert pipe.planar and pipe.h_out[0].dtype == torch.float16 and pipe.zero_copy_out
    with by_name["frame-nv12-to-nv12-mapped"].make() as pipe:
        assert pipe.nv12 and pipe.nv12_out and pipe.warp_map is not None
