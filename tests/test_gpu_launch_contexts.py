"""Every launching entry point that no other test captures, in the contexts a camera loop runs it in (tests/launch_contexts.py holds the
cases and the checks; tests/test_launch_contexts_cpu.py shows on the CPU that the checks fail what they are for):

  side stream    on a fresh stream behind a delay of about 50 ms, set B copied over set A and the destination poisoned in stream order
  replays        captured into a graph, the caller's host arrays overwritten with NaNs, replayed on set B and on set A; once more with
                 the frames handed over as channel slices (the entry's contiguous copy is a node of the graph), and, where the entry
                 allocates its result (BORDER_TRANSPARENT: zeroed), as the no_out cases of the table
  second device  every tensor on cuda:1 while cuda:0 is current (skipped as one test on a machine with one device)

Every result is compared by bits with the numpy definitions under tests/.  Run on the GPU box:  python -m pytest tests -m gpu -q"""
import pytest
import torch

from tests import launch_contexts as LC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def delay():
    """(cycles, milliseconds) of the delay every side-stream case runs behind: measured once, scaled to about 50 ms, measured again."""
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    cycles, ms = LC.sleep_cycles_for(50.0)
    print("torch.cuda._sleep(%d) takes %.1f ms" % (cycles, ms))
    assert ms >= 20.0, "the delay came out at %.2f ms: too short to enqueue a call behind" % ms
    return cycles, ms


@pytest.mark.parametrize("case", LC.CASES, ids=repr)
def test_side_stream_behind_a_delay(case, delay):
    cycles, ms = delay
    case.assert_preconditions()
    host_s = LC.check_side_stream(case, LC.Gpu("cuda:0", cycles))
    print("%s: delay %.1f ms, the call took %.3f ms on the host" % (case.name, ms, host_s * 1e3))


@pytest.mark.parametrize("case", LC.CASES, ids=repr)
def test_capture_and_replay(case):
    case.assert_preconditions()
    LC.check_replays(case, LC.Gpu("cuda:0"))


@pytest.mark.parametrize("case", LC.COPIED_SOURCE, ids=repr)
def test_capture_and_replay_copied_source(case):
    case.assert_preconditions()
    LC.check_replays(case, LC.Gpu("cuda:0"), sliced=True)


def test_second_device():
    """All cases in one test: a machine with one device skips once."""
    if torch.cuda.device_count() < 2:
        pytest.skip("the second-device context needs two devices, this machine has %d" % torch.cuda.device_count())
    assert torch.cuda.current_device() == 0
    for case in LC.CASES:
        try:
            LC.check_second_device(case, LC.Gpu("cuda:1"))
        except AssertionError as err:
            raise AssertionError("%s on cuda:1: %s" % (case.name, err)) from None
