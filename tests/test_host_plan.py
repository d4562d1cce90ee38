"""The launch planning of the C ABI (bev_amd/csrc/host_plan.h) on the CPU: tests/host_plan_driver.cpp is compiled with g++ under the
address and undefined-behaviour sanitizers and run as a subprocess (tests/hostplan.py).  tests/golden/launch_plans.json pins every field of the plans
(recorded from the last commit that planned inside bevwarp_api.hip; tests/golden/make_launch_plans.py)."""
import json
import os

import numpy as np
import pytest

from bev_amd import _lib
from tests.hostplan import build_driver, built_lib, run_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "launch_plans.json")
PLAN_FIELDS = ("tile_h", "tiles_x", "tiles_per_frame", "total_tiles", "chunk", "stagger", "tail_split", "bw0", "tpf_magic", "tx_magic", "bw0_magic")
PERIOD_FIELDS = ("per_x", "off_x", "mag_x", "per_y", "off_y", "mag_y")
TOO_LARGE = -3


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)["cases"]


def launch_constants(fixture):
    """What the kernels tell the planner (tile width, rows per pass, resident workgroups, the composite's tallest tile) by case kind
    and pixel type, as the fixture recorded them."""
    out = {}
    for c in fixture:
        if c["plan"] and c["kind"] != "border":
            p = c["plan"]
            out.setdefault((c["kind"], c["args"][6] if c["kind"] == "rows" else 0), (p["tw"], p["rpp"], p["max_rows"], p["resident"]))
    return out


def driver_line(case, consts):
    a = case["args"]
    if case["kind"] == "rows":
        tw, rpp, _, resident = consts[("rows", a[6])]
        return "rows %d %d %d %d %d %d %d" % (a[0], a[3], a[4], a[6], tw, rpp, resident)
    if case["kind"] == "composite":
        tw, rpp, max_rows, cus = consts[("composite", 0)]
        return "composite %d %d %d %d %d %d" % (a[4], a[5], tw, rpp, max_rows, cus)
    return "border %d %d %d 256 4 %d %d %d" % (a[0], a[3], a[4], a[8], a[1], a[2])  # (kBorderTileW x kBorderTileH)


def plans_from_driver(exe, cases):
    """The fixture's records of `cases` as host_plan.h computes them now (make_launch_plans.py regenerates the fixture with this); the
    kernels' constants are carried over from the fixture."""
    consts = launch_constants(load_fixture())
    out = []
    for case, nums in zip(cases, run_driver(exe, [driver_line(c, consts) for c in cases], "plan")):
        plan = None
        if nums[0] == 0 and case["kind"] == "border":
            plan = dict(zip(PLAN_FIELDS + PERIOD_FIELDS, nums[1:]), tw=256)
            plan = {k: plan[k] for k in ("tw",) + PLAN_FIELDS + PERIOD_FIELDS if k not in ("chunk", "stagger", "tail_split")}  # (BorderArgs has none)
        elif nums[0] == 0:
            plan = dict(zip(("tw", "rpp", "max_rows", "resident"), consts[(case["kind"], case["args"][6] if case["kind"] == "rows" else 0)]))
            plan.update(zip(PLAN_FIELDS, nums[1:]))
        out.append(dict(kind=case["kind"], args=case["args"], status=nums[0], plan=plan))
    return out


@pytest.fixture(scope="module")
def driver():
    return build_driver()


@pytest.fixture(scope="module")
def lib():
    return built_lib()


def test_fixture_takes_every_branch_of_the_planner():
    """At least three recorded cases on either side of every decision, so that the comparison below is not hollow."""
    fixture = load_fixture()
    assert len(fixture) >= 300
    rows = [c for c in fixture if c["kind"] == "rows"]
    plans = [c["plan"] for c in rows if c["plan"]]
    rpp = plans[0]["rpp"]
    count = {
        "tile height halved down to one pass": sum(p["tile_h"] == rpp for p in plans),
        "16 rows": sum(p["tile_h"] == 4 * rpp == 16 for p in plans),
        "24 rows": sum(p["tile_h"] == 6 * rpp == 24 for p in plans),
        "no tail split": sum(p["tail_split"] == 0 for p in plans),
        "tail split": sum(p["tail_split"] > 0 for p in plans),
        "no stagger": sum(p["stagger"] == 0 for p in plans),
        "stagger": sum(p["stagger"] > 0 for p in plans),
        "too large by the item count": sum(c["status"] == TOO_LARGE and max(c["args"][3:5]) <= 1 << 20 for c in rows),
        "too large by a side of the destination": sum(c["status"] == TOO_LARGE and max(c["args"][3:5]) > 1 << 20 for c in rows),
    }
    for m in ("tpf_magic", "tx_magic", "bw0_magic"):
        count[m + " = 0 (divide)"] = sum(p[m] == 0 for p in plans)
        count[m + " != 0"] = sum(p[m] != 0 for p in plans)
    for kind in ("composite", "border"):
        count[kind] = sum(c["kind"] == kind and c["plan"] is not None for c in fixture)
    assert all(n >= 3 for n in count.values()), count
    assert {c["status"] for c in fixture} == {0, TOO_LARGE}
    for batch in (1, 2, 4, 12, 32, 64):
        assert {(c["args"][6], c["args"][7]) for c in rows if c["args"][0] == batch} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    sides = {tuple(c["args"][3:5]) for c in rows}
    assert {(8, 8), (77, 300), (1080, 1920), (4096, 4096), (1 << 20, 8), (8, 1 << 20)} <= sides
    named = [[1, 720, 1280, 512, 512, 3, 0, 1], [1, 720, 1280, 512, 512, 3, 0, 0], [1, 720, 1280, 512, 512, 3, 1, 1], [1, 240, 426, 512, 512, 3, 0, 1],
             [32, 1080, 1920, 1024, 1024, 3, 1, 1], [32, 1080, 1920, 1024, 1024, 3, 0, 1], [32, 2160, 3840, 2048, 2048, 3, 1, 1], [1, 1080, 1920, 1024, 1024, 3, 0, 1]]
    assert all(any(c["args"] == a for c in rows) for a in named)  # smoke(), BASELINE.json's configs, bench.py's shapes


def test_plans_equal_the_recorded_ones(driver, lib):
    """Fixture, planner and shipped library agree three ways: host_plan.h reproduces every field the parent's launches had, and
    bevwarp_tile_classes_bytes of the built library is 12 bytes per tile of the same plan (or its status)."""
    fixture = load_fixture()
    consts = launch_constants(fixture)
    got = run_driver(driver, [driver_line(c, consts) for c in fixture], "plan")
    for case, nums in zip(fixture, got):
        assert nums[0] == case["status"], (case, nums)
        if case["plan"]:
            computed = dict(zip(PLAN_FIELDS + (PERIOD_FIELDS if case["kind"] == "border" else ()), nums[1:]))
            recorded = {k: v for k, v in case["plan"].items() if k in computed}  # (BorderArgs has no chunk, stagger or tail split: a flat grid)
            assert len(recorded) == (14 if case["kind"] == "border" else 11) and recorded == {k: computed[k] for k in recorded}, (case, computed)
        if case["kind"] == "rows":
            assert lib.bevwarp_tile_classes_bytes(*case["args"]) == (12 * case["plan"]["total_tiles"] if case["plan"] else case["status"]), case


def test_tile_classes_bytes_sees_no_pointer(lib):
    """The size query used to run the launch path on placeholder pointers, and a batch x source frame above 0x6fff_ffff_f000 bytes made
    them `overlap` (-6).  It is answered from the sizes alone: 60000 one-tile frames have a 720000-byte table.  Neighbours unchanged."""
    assert lib.bevwarp_tile_classes_bytes(60000, 32767, 16000, 8, 8, 4, _lib.U8, 1) == 720000
    assert lib.bevwarp_tile_classes_bytes(2147483647, 8, 8, 64, 600, 3, _lib.U8, 1) == -3   # item count
    assert lib.bevwarp_tile_classes_bytes(1, 8, 8, 8, (1 << 20) + 1, 1, _lib.U8, 1) == -3   # destination side
    assert lib.bevwarp_tile_classes_bytes(32, 1080, 1920, 1024, 1024, 3, _lib.U8, 1) == 66048
    assert lib.bevwarp_tile_classes_bytes(1, 32768, 8, 8, 8, 1, _lib.U8, 1) == -3           # the source limits still apply
    assert lib.bevwarp_tile_classes_bytes(1, 8, 8, 8, 8, 1, 7, 1) == -2


def test_overlap_guard_under_the_sanitizer(driver):
    """regions_overlap against brute force on the layouts of test_abi.test_overlap_guard_has_no_false_negatives (same seed, same
    draws), then on addresses next to UINTPTR_MAX and strides next to the limits, where only the sanitizer's silence is asserted."""
    rng = np.random.default_rng(5)
    lines, truth = [], []
    for _ in range(3000):
        sw, sh, dw, dh = (int(v) for v in rng.integers(1, 7, 4))
        batch = int(rng.integers(1, 4))
        if rng.random() < 0.5:  # the refinement's class: one common row stride, frame strides multiples of it
            rs = int(rng.integers(max(sw, dw), 20))
            srs = drs = rs
            sfs, dfs = rs * int(rng.integers(sh, sh + 3)), rs * int(rng.integers(dh, dh + 3))
        else:
            srs, drs = int(rng.integers(sw, 20)), int(rng.integers(dw, 20))
            sfs, dfs = int(rng.integers(sh * srs, sh * srs + 30)), int(rng.integers(dh * drs, dh * drs + 30))
        s0, d0 = 4096 + int(rng.integers(0, 120)), 4096 + int(rng.integers(0, 120))
        sbytes = {s0 + f * sfs + r * srs + c for f in range(batch) for r in range(sh) for c in range(sw)}
        dbytes = {d0 + f * dfs + r * drs + c for f in range(batch) for r in range(dh) for c in range(dw)}
        lines.append("overlap %d %d %d %d %d %d %d %d %d %d %d" % (s0, sh, sw, srs, sfs, d0, dh, dw, drs, dfs, batch))
        truth.append(bool(sbytes & dbytes))
    got = [bool(v[0]) for v in run_driver(driver, lines, "plan")]
    assert all(g for g, t in zip(got, truth) if t)                 # no false negative
    assert sum(not g for g in got) > 300                           # and not simply refusing everything
    assert run_driver(driver, ["overlap 4096 4 6 16 64 4102 4 6 16 64 2"], "plan") == [[0]]  # side by side, interleaved bounding ranges
    top, imax = (1 << 64) - 1, (1 << 63) - 1
    edge = ["overlap %d 8 24 24 192 %d 8 24 24 192 4" % (top - 4096, top - 2048), "overlap %d 8 24 24 192 16 8 24 24 192 1" % (top - 100),
            "overlap 4096 32767 16 %d %d 8192 32767 16 %d %d 65535" % (imax, imax, imax, imax), "overlap 16 1 1 1 0 16 1 1 1 0 1",
            "overlap 4096 8 8 %d 0 4100 8 8 %d 0 1" % (1 << 62, 1 << 62), "overlap 0 1 1 1 1 %d 1 1 1 1 2147483647" % top]
    assert len(run_driver(driver, edge, "plan")) == len(edge)


def test_layout_and_size_checks_at_their_limits(driver):
    imax = (1 << 63) - 1
    cases = [("layout 16 8 24 24 192 2 1", 0), ("layout 16 8 24 23 192 2 1", -1), ("layout 16 8 24 24 191 2 1", -1), ("layout 16 8 24 24 0 1 1", 0),
             ("layout 16 8 96 96 768 2 4", 0), ("layout 18 8 96 96 768 2 4", -1), ("layout 16 8 96 98 800 2 4", -1), ("layout 16 8 96 96 770 1 4", -1),
             ("layout 16 8 24 -24 192 2 1", -1),
             # strides next to 2^63: rows * stride is not representable in 64 bits, and is still compared exactly
             ("layout 16 32767 24 %d %d 2 1" % (imax, imax), -1), ("layout 16 1 24 %d %d 2 1" % (imax, imax), 0), ("layout 16 2 24 %d %d 1 1" % (imax, -imax - 1), 0),
             ("size 32767 32767 %d 32767 32767 1" % ((1 << 24) - 1), -3), ("size 32767 32767 65539 32767 32767 1", -3), ("size 32767 32767 65538 32767 32767 1", 0),
             ("size 32768 8 8 32767 32767 1", -3), ("size 8 32768 8 32767 32767 1", -3), ("size 8 8 %d 32767 32767 1" % (1 << 24), -3),
             ("size 32767 8 %d 32767 32767 1" % imax, -3), ("size 2147483647 8 %d 2147483647 8 0" % imax, 0), ("size 65536 8 8 65535 16777216 0", -3)]
    assert [v[0] for v in run_driver(driver, [c for c, _ in cases], "plan")] == [st for _, st in cases]
    # destination sides beyond the limit are refused before any arithmetic on them
    big = ["rows 1 8 2147483647 0 256 4 1024", "rows 2147483647 2147483647 2147483647 1 128 4 1024", "border 2147483647 2147483647 2147483647 256 4 2 1 32767",
           "rows 2147483647 1048576 1048576 1 128 4 1024", "border 2147483647 1048576 1048576 256 4 4 32767 32767"]
    assert [v[0] for v in run_driver(driver, big, "plan")] == [TOO_LARGE] * len(big)


def test_div_magic_divides_exactly(driver):
    """The multiply-high of coords.h's fast_div with div_magic's constant against plain division: every n <= n_max for small divisors,
    and the last n_max that still gets a magic (n_max * d < 2^32) for large ones; beyond it the magic is 0 and the kernel divides."""
    lines = ["magic %d %d" % (n_max, d) for d in range(1, 70) for n_max in (1, 69, 70001)] + ["magic %d %d" % (((1 << 32) - 1) // d, d) for d in (255, 256, 641, 4099, 65537)]
    for (m, wrong), ln in zip(run_driver(driver, lines, "plan"), lines):
        d = int(ln.split()[2])
        assert (m, wrong) == ((0, -1) if d == 1 else ((1 << 32) // d + 1, 0)), ln
    edge = []
    for d in (2, 3, 7, 24, 25, 255, 4096, 65535, 65536, 65537, 1 << 20, (1 << 31) - 1, (1 << 31), (1 << 32) - 1):
        last = ((1 << 32) - 1) // d
        edge += [(last, d), (last + 1, d), (last - 1, d)]
    wrap = [((1 << 64) - 1, 3), (1 << 63, 2), (1 << 32, (1 << 32) - 1)]  # (a product beyond 64 bits wraps, unsigned: only the sanitizer's silence is asserted)
    got = run_driver(driver, ["magic_at %d %d" % (n, d) for n, d in edge + wrap], "plan")
    for (n, d), (m, q, exact) in zip(edge, got):
        assert (m != 0) == (n * d < 1 << 32 and d > 1) and q == exact == n // d, (n, d, m, q, exact)
