"""tests/box_ref.py against the upstream reference's own vectors and against bev_amd.rbox under every BEV axis convention, the
quadrilateral IoU helper, and the proof that every case tests/test_gpu_axes.py runs on the device can tell a wrong heading from a
right one.  No GPU."""
import numpy as np
import pytest

from bev_amd import rbox as host_rbox
from oracle import cpu_oracle as co
from tests import axis_cases as ac
from tests import box_ref

BAR = dict(rtol=1e-12, atol=1e-12)  # the bar tests/test_host_api.py holds the host code to on the same vectors


def test_box_ref_reproduces_the_reference_vectors(golden):
    g = golden["rbox"]
    Hwb, Hrefl, Hwi = np.array(g["H_world_bev"]), np.array(g["H_world_bev_refl"]), np.array(g["H_world_img"])
    boxes, world = np.array(g["boxes_bev"]), np.array(g["rbox_world_bev__bev2world"])
    assert np.linalg.det(Hwb[:2, :2]) > 0 > np.linalg.det(Hrefl[:2, :2] / Hrefl[2, 2]) and Hrefl[2, 2] != 1
    for fn in (box_ref.rbox_world_bev, box_ref.rbox_world_bev_points):
        box_ref.assert_boxes_close(fn(boxes, Hwb, "bev"), world, err_msg="bev2world", **BAR)
        box_ref.assert_boxes_close(fn(world, np.linalg.inv(Hwb), "world"), g["rbox_world_bev__world2bev"], err_msg="world2bev", **BAR)
        box_ref.assert_boxes_close(fn(boxes, Hrefl, "bev"), g["rbox_world_bev__bev2world_refl"], err_msg="bev2world_refl", **BAR)
    np.testing.assert_allclose(box_ref.centres_img(world, np.linalg.inv(Hwi)), np.array(g["rbox_world_img"]), **BAR)


@pytest.mark.parametrize("mult", ac.MULTIPLIERS)
@pytest.mark.parametrize("conv", ac.CONVENTIONS, ids=ac.CONVENTION_IDS)
def test_box_ref_agrees_with_the_host_code_under_every_convention(conv, mult):
    spec = ac.convention_spec(*conv)
    H = spec.gen_H_world_bev()
    assert (np.linalg.det(H[:2, :2]) > 0) == (ac.CONVENTIONS.index(conv) < 4)
    H = H * mult
    rng = np.random.default_rng(3)
    bev = ac.random_boxes_bev(rng, spec, 64, 0.0625)
    world = host_rbox.rbox_world_bev(bev, H, "bev")
    Hinv = np.linalg.inv(H) * mult
    for fn in (box_ref.rbox_world_bev, box_ref.rbox_world_bev_points):
        box_ref.assert_boxes_close(fn(bev, H, "bev"), world, err_msg="bev -> world", **BAR)
        box_ref.assert_boxes_close(fn(world, Hinv, "world"), host_rbox.rbox_world_bev(world, Hinv, "world"), err_msg="world -> bev", **BAR)
    # a last row that is small but accepted: the centre goes through the divide, the extent through the similarity part
    Hs = ac.small_last_row(H) * mult
    got = box_ref.rbox_world_bev(bev, Hs, "bev")
    box_ref.assert_boxes_close(got, host_rbox.rbox_world_bev(bev, Hs, "bev"), err_msg="small last row", **BAR)
    assert np.abs(got[:, :2] - world[:, :2]).max() > 1e-3  # (the divide by W is live)


def _sample_world_boxes(n, seed):
    rng = np.random.default_rng(seed)
    a = np.column_stack([rng.uniform(0, 12, (n, 2)), rng.uniform(1.6, 2.2, n), rng.uniform(3.5, 6, n), rng.uniform(-np.pi, np.pi, n)])
    return a, a + rng.normal(0, [0.6, 0.6, 0.05, 0.1, 0.3], (n, 5))


def test_iou_quads_equals_the_box_iou_and_survives_mirroring():
    pytest.importorskip("mpmath")
    from tests.exact_iou import iou, iou_quads
    a, b = _sample_world_boxes(24, 17)
    mirror = np.array([-1.0, 1.0])
    overlapping = 0
    for p, q in zip(a, b):
        want = iou(p, q)
        overlapping += want > 0.05
        P, Q = box_ref.quad(p, "world"), box_ref.quad(q, "world")
        assert abs(iou_quads(P, Q) - want) <= 1e-15
        assert abs(iou_quads(P[::-1], Q) - want) <= 1e-15 and abs(iou_quads(P, Q[::-1]) - want) <= 1e-15  # either sense, either argument
        assert abs(iou_quads(P * mirror, Q * mirror) - want) <= 1e-15  # mirrored quads arrive clockwise
    assert overlapping >= 20
    np.testing.assert_allclose([iou(p, q) for p, q in zip(a, b)], np.diag(co.rbox_iou(a, b)), rtol=0, atol=1e-12)
    # quad() of a BEV box, read in the raster's (u, v) plane, is the same rectangle: w across, h along the heading
    bev = np.array([[10.0, 20.0, 2.0, 5.0, 0.0]])
    np.testing.assert_allclose(sorted(map(tuple, box_ref.quad(bev[0], "bev"))), [(9, 17.5), (9, 22.5), (11, 17.5), (11, 22.5)], atol=1e-15)
    np.testing.assert_allclose(box_ref.points(bev, "bev")[0, 4], [10, 22.5], atol=1e-15)  # yaw 0 looks along +v


def test_shipped_configs_load_and_three_of_them_mirror():
    mirrored = set()
    for name in ac.SHIPPED:
        H = ac.shipped_spec(name).gen_H_world_bev()
        assert abs(H[2, 0]) + abs(H[2, 1]) < 1e-9 * abs(H[2, 2])
        if np.linalg.det(H[:2, :2] / H[2, 2]) < 0:
            mirrored.add(name)
    assert mirrored == ac.MIRRORED_SHIPPED


def _mutants(dets_world, H_world_bev):
    """Three ways a kernel can get a box's orientation wrong, applied to the host's correct world boxes."""
    Hn = H_world_bev / H_world_bev[2, 2]
    v_axis = np.arctan2(Hn[1, 1], Hn[0, 1])  # world direction of the raster's v axis
    mirrored, swapped, exchanged = dets_world.copy(), dets_world.copy(), dets_world.copy()
    mirrored[:, 4] = 2 * v_axis - dets_world[:, 4]
    swapped[:, [2, 3]] = dets_world[:, [3, 2]]
    exchanged[:, 4] = np.pi / 2 - dets_world[:, 4]  # atan2(a, b) for atan2(b, a)
    return {"heading mirrored about the v axis": mirrored, "w and h swapped": swapped, "atan2 arguments exchanged": exchanged}


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", ac.TRACKER_CASES, ids=ac.TRACKER_IDS)
def test_gpu_cases_discriminate(case, dtype):
    """A condition on the INPUTS of tests/test_gpu_axes.py's tracker cases, checked with the host reference alone: enough pairs
    overlap and pass the gate, and each orientation mistake moves at least 90 % of the gated pairs' IoU by more than 1e-3 -- a
    thousand times the float32 bar, 1e9 times the float64 one."""
    _, kind, key = case
    c = ac.tracker_case(kind, key, dtype)
    dets_world = host_rbox.rbox_world_bev(c["dets_bev"], c["H_world_bev"], "bev")
    box_ref.assert_boxes_close(box_ref.rbox_world_bev(c["dets_bev"], c["H_world_bev"], "bev"), dets_world, **BAR)
    exp = co.rbox_iou(dets_world, c["trks"][:, :5])
    gated, overlapping, ok = ac.non_vacuity(exp, c["threshold"])
    assert ok, (gated, overlapping)
    above = exp > c["threshold"]
    for name, wrong in _mutants(dets_world, c["H_world_bev"]).items():
        moved = np.abs(co.rbox_iou(wrong, c["trks"][:, :5]) - exp)[above] > 1e-3
        assert moved.mean() >= 0.9, "%s: only %d of %d gated pairs move" % (name, moved.sum(), above.sum())
