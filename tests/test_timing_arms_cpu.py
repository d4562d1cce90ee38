"""tools/arms.py, the timing scripts' one protocol, driven on the CPU: stand-in events on a fake clock and a counting launch give the exact
sequence of launches, event records and synchronises; the reduction against np.percentile; the tail into a temporary directory."""
import numpy as np
import pytest

from tools import arms

ARMS = ("a", "b", "c")

# rounds=3, per_round=2, warm=1: the sequence the loop of tools/time_lens.py produced before it moved into timed()
FIXED = """
a b c sync
rec a rec rec a rec sync   rec b rec rec b rec sync   rec c rec rec c rec sync
rec a rec rec a rec sync   rec b rec rec b rec sync   rec c rec rec c rec sync
rec a rec rec a rec sync   rec b rec rec b rec sync   rec c rec rec c rec sync
""".split()

ALTERNATE = """
a b c sync
rec a rec rec a rec sync   rec b rec rec b rec sync   rec c rec rec c rec sync
rec c rec rec c rec sync   rec b rec rec b rec sync   rec a rec rec a rec sync
rec a rec rec a rec sync   rec b rec rec b rec sync   rec c rec rec c rec sync
""".split()


class Bench:
    """A fake device: launch number n takes n ms of its clock; events read the clock when recorded."""

    def __init__(self):
        self.log, self.ms, self.launches, self.took = [], 0.0, 0, {arm: [] for arm in ARMS}
        bench = self

        class Event:
            def record(self):
                bench.log.append("rec")
                self.at = bench.ms

            def elapsed_time(self, other):
                return other.at - self.at

        self.Event = Event

    def launch(self, arm):
        self.log.append(arm)
        self.launches += 1
        self.ms += self.launches
        self.took[arm].append(self.launches * 1e3)

    def sync(self):
        self.log.append("sync")

    def timed(self, warm=1, **kw):
        t = arms.timed(ARMS, self.launch, 3, 2, warm, event=self.Event, sync=self.sync, **kw)
        timed_launches = {arm: self.took[arm][-6:] for arm in ARMS}  # (rounds * per_round per arm, in launch order)
        assert t == timed_launches and list(t) == list(ARMS)
        return t


def test_fixed_order_is_the_loop_of_time_lens():
    for kw in ({"order": "fixed"}, {}):  # ("fixed" is the default)
        b = Bench()
        b.timed(**kw)
        assert b.log == FIXED


def test_alternate_order_reverses_odd_rounds():
    b = Bench()
    b.timed(order="alternate")
    assert b.log == ALTERNATE
    with pytest.raises(AssertionError):
        Bench().timed(order="random")


def test_warm_arms_warms_a_subset_and_times_all():
    b = Bench()
    b.timed(warm=2, warm_arms=("c", "a"))
    assert b.log == "c c a a sync".split() + FIXED[4:]


def test_arms_may_be_any_hashable():
    log = []
    b = Bench()
    pairs = [("k", None), ("k", "brno")]
    t = arms.timed(pairs, log.append, 1, 1, 0, event=b.Event, sync=b.sync)
    assert list(t) == pairs and log == pairs


def test_event_us_is_the_single_arm_form():
    b = Bench()
    assert arms.event_us(lambda: b.launch("a"), 3, b.Event, b.sync) == [1e3, 2e3, 3e3]
    assert b.log == "rec a rec rec a rec rec a rec sync".split()


def test_reduction_is_np_percentile():
    t = {"a": [3.0, 1.0, 4.0, 1.0, 5.0, 9.0, 2.0, 6.0], ("k", None): [2.5, 0.5, 7.25]}
    q = arms.p10_50_90(t)
    assert list(q) == list(t)
    for arm, v in t.items():
        assert q[arm] == [np.percentile(v, 10), np.percentile(v, 50), np.percentile(v, 90)]
        assert q[arm][1] == np.median(v) and all(type(x) is float for x in q[arm])


def test_counts_and_parser():
    assert arms.counts(True) == arms.counts(True, (6, 10, 4)) == (2, 3, 2)
    assert arms.counts(False) == (7, 10, 5) and arms.counts(False, (8, 8, 4)) == (8, 8, 4)
    a = arms.parser("doc").parse_args(["--quick", "--out", "x.txt"])
    assert a.quick and a.out == "x.txt" and not hasattr(a, "step")
    a = arms.parser("doc", steps=("kernels", "pipeline")).parse_args(["--step", "pipeline", "--append"])
    assert (a.step, a.append, a.quick, a.out) == ("pipeline", True, False, None)
    with pytest.raises(SystemExit):
        arms.parser("doc", steps=("kernels", "pipeline")).parse_args([])
    assert arms.parser("doc", steps=("kernels", "all"), step="all").parse_args([]).step == "all"


def test_tail_writes_then_appends(tmp_path, capsys):
    out = tmp_path / "made" / "by" / "finish" / "table.txt"
    arms.finish(["# one", "two"], str(out))
    assert out.read_text() == "# one\ntwo\n" and capsys.readouterr().out == "# one\ntwo\n"
    arms.finish(["three"], str(out), append=True)
    assert out.read_text() == "# one\ntwo\nthree\n"
    arms.finish(["four"], str(out))
    assert out.read_text() == "four\n"
    arms.finish(["printed only"], None)
    assert capsys.readouterr().out == "three\nfour\nprinted only\n"


def test_scene_is_the_tests_lens_and_camera():
    K = arms.camera_K(arms.SW, arms.SH)
    assert (arms.B, arms.SH, arms.SW, arms.D, arms.C) == (32, 1080, 1920, 1024, 3)
    assert K.tolist() == [[1536.0, 0, 959.5], [0, 0.816 * 1920, 542.5], [0, 0, 1.0]]
    lens = arms.lens_array(K, arms.LENS_A)
    assert lens.dtype == np.float64 and lens.flags.c_contiguous
    assert lens.tolist() == [1536.0, 0.816 * 1920, 959.5, 542.5, -0.30, 0.10, 0.001, -0.0005, -0.01, 0.0, 0.0, 0.0]
    assert arms.lens_array(K, (-0.02, 0.004, -0.001, 0.0002)).tolist()[4:] == [-0.02, 0.004, -0.001, 0.0002, 0.0, 0.0, 0.0, 0.0]
    names = [(name, Ms.shape) for name, _, Ms in arms.footprints()]
    assert names == [("keystone", (32, 3, 3)), ("brno", (32, 3, 3))]
    assert len(arms.views()) == 3
