"""rbox_transform_kernel, tracker_step_kernel and rbox_iou_kernel under every BEV axis convention -- turning AND mirroring
similarities, H[2][2] != 1, a last row that is small but not zero -- against tests/box_ref.py (boxes as points: no yaw algebra
shared with the kernels), the IoU oracle and 50-digit arithmetic; their outputs written into guarded memory at the edges of the
64-lane workgroups.  The cases come from tests/axis_cases.py; tests/test_box_ref_cpu.py proves on the host that each of them would
notice a mirrored heading, swapped sizes or an atan2 with exchanged arguments.

The float32 bar.  The kernels compute in float64 and round once, and so does `float32(box_ref(float32-rounded inputs))`: the two
agree unless float64 noise flips a rounding, hence 1 float32 ulp (np.spacing of the expected value) per component.  A yaw is an
angle: it is compared modulo 2 pi, across the +-pi seam within 1 ulp at pi; and since the reference's own yaw carries the float64
bar of absolute error (1e-12: it is measured on points), a yaw whose ulp is smaller than that -- the images of exact multiples of
pi / 2 -- is held to 1e-12.  Each test prints its largest distance next to the bar."""
import numpy as np
import pytest
import torch

from oracle import cpu_oracle as co
from tests import axis_cases as ac
from tests import box_ref

pytestmark = pytest.mark.gpu

F64_BAR = dict(rtol=1e-12, atol=1e-12)
DTYPES = [np.float64, np.float32]
DTYPE_IDS = ["f64", "f32"]
PI32_ULP = float(np.spacing(np.float32(np.pi)))


def _cuda(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _f32_ulps(got, exp64, yaw_col=None):
    """Distance of float32 `got` from float32(exp64) in units of the bar (1 = one ulp of the expected value; see the module docstring)."""
    exp32 = np.asarray(exp64, dtype=np.float64).astype(np.float32)
    assert got.dtype == np.float32 and got.shape == exp32.shape
    diff = np.abs(got.astype(np.float64) - exp32.astype(np.float64))
    tol = np.spacing(np.abs(exp32)).astype(np.float64)
    if yaw_col is not None:
        seam = diff[:, yaw_col] > np.pi
        diff[:, yaw_col] = np.abs(box_ref.yaw_diff(got[:, yaw_col], exp32[:, yaw_col]))
        tol[:, yaw_col] = np.where(seam, PI32_ULP, np.maximum(tol[:, yaw_col], 1e-12))
    return diff / tol


def _check_boxes(got, exp64, dtype, what):
    """Device boxes against the reference at the bar of their precision; returns the largest distance in units of the bar."""
    if dtype == np.float64:
        assert got.dtype == np.float64
        box_ref.assert_boxes_close(got, exp64, err_msg=what, **F64_BAR)
        d = np.abs(got - exp64)
        d[:, 4] = np.abs(box_ref.yaw_diff(got[:, 4], exp64[:, 4]))
        worst = float((d / (1e-12 + 1e-12 * np.abs(exp64))).max())
    else:
        u = _f32_ulps(got, exp64, yaw_col=4)
        worst = float(u.max())
        r, c = np.unravel_index(u.argmax(), u.shape)
        assert worst <= 1.0, "%s: %.3g ulp off in component %d of row %d (got %r, expected %r)" % (what, worst, c, r, got[r, c], exp64[r, c])
    print("%s [%s]: %.3g of the bar" % (what, np.dtype(dtype).name, worst))
    return worst


def _check_points(got, exp64, dtype, what, f64_bar):
    if dtype == np.float64:
        np.testing.assert_allclose(got, exp64, err_msg=what, **f64_bar)
        worst = float((np.abs(got - exp64) / (f64_bar["atol"] + f64_bar["rtol"] * np.abs(exp64))).max())
    else:
        u = _f32_ulps(got, exp64)
        worst = float(u.max())
        assert worst <= 1.0, "%s: %.3g ulp off at %s" % (what, worst, np.unravel_index(u.argmax(), u.shape))
    print("%s [%s]: %.3g of the bar" % (what, np.dtype(dtype).name, worst))


# ---- a. the reference's own vectors on the device ------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_reference_vectors_on_the_device(golden, dtype):
    from bev_amd.tracker_geom import rbox_world_bev_device
    g = golden["rbox"]
    Hwb, Hrefl = np.array(g["H_world_bev"]), np.array(g["H_world_bev_refl"])
    boxes, world = np.array(g["boxes_bev"]), np.array(g["rbox_world_bev__bev2world"])
    runs = (("bev2world", boxes, Hwb, "bev", g["rbox_world_bev__bev2world"]), ("bev2world_refl", boxes, Hrefl, "bev", g["rbox_world_bev__bev2world_refl"]),
            ("world2bev", world, np.linalg.inv(Hwb), "world", g["rbox_world_bev__world2bev"]))
    for what, src_boxes, H, src, want in runs:
        got = rbox_world_bev_device(_cuda(src_boxes, dtype), H, src).cpu().numpy()
        if dtype == np.float64:
            _check_boxes(got, np.array(want), dtype, what)  # the reference's own numbers
        else:
            rounded = src_boxes.astype(np.float32).astype(np.float64)
            _check_boxes(got, box_ref.rbox_world_bev(rounded, H, src), dtype, what)
            box_ref.assert_boxes_close(got, np.array(want), rtol=2e-6, atol=2e-5, err_msg=what)  # ... which stay near the reference's


# ---- b. the conversions, full matrix --------------------------------------------------------------------------------------------

N_CONV = 257  # two workgroups of 256 with a ragged tail of one


def _special_yaws(dtype):
    """Exact multiples of pi / 2 (as `dtype` holds them) and their neighbours one ulp either side."""
    k = (np.arange(-4, 5) * (np.pi / 2)).astype(dtype)
    return np.concatenate([k, np.nextafter(k, dtype(np.inf)), np.nextafter(k, dtype(-np.inf))]).astype(np.float64)


def _conversion_rows(boxes5, dtype, rng):
    """(n, 7) rows of `dtype` values (held in float64): the boxes, special yaws in the first rows, two columns the kernel must skip."""
    rows = np.column_stack([boxes5, rng.normal(0, 1, (len(boxes5), 2))]).astype(dtype).astype(np.float64)
    ys = _special_yaws(dtype)
    rows[:len(ys), 4] = ys
    return rows


CONVERSIONS = [(i, c, mult, False) for i, c in zip(ac.CONVENTION_IDS, ac.CONVENTIONS) for mult in ac.MULTIPLIERS] + \
              [(ac.CONVENTION_IDS[k], ac.CONVENTIONS[k], -2.5, True) for k in (2, 7)]  # a turning and a mirroring H with a small last row


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("conv_id,conv,mult,small_row", CONVERSIONS, ids=["%s-x%g%s" % (c[0], c[2], "-lastrow" if c[3] else "") for c in CONVERSIONS])
def test_conversions_under_every_convention(conv_id, conv, mult, small_row, dtype):
    from bev_amd.tracker_geom import rbox_world_bev_device
    spec = ac.convention_spec(*conv)
    H = spec.gen_H_world_bev()
    Hinv = np.linalg.inv(H)
    if small_row:  # (each direction gets its own matrix: the inverse of a matrix with this last row has a last row beyond the 1e-5 gate)
        H, Hinv = ac.small_last_row(H), ac.small_last_row(Hinv)
    H, Hinv = H * mult, Hinv * mult
    rng = np.random.default_rng(31)
    bev = _conversion_rows(ac.random_boxes_bev(rng, spec, N_CONV, 0.0625), dtype, rng)
    world_ref = box_ref.rbox_world_bev(bev, H, "bev")
    t_bev = _cuda(bev, dtype)
    assert t_bev.shape == (N_CONV, 7) and t_bev.stride(0) == 7
    got_world = rbox_world_bev_device(t_bev, H, "bev")
    assert got_world.shape == (N_CONV, 5)
    _check_boxes(got_world.cpu().numpy(), world_ref, dtype, "bev -> world")
    if small_row:
        assert np.abs(world_ref[:, :2] - box_ref.rbox_world_bev(bev, spec.gen_H_world_bev(), "bev")[:, :2]).max() > 1e-3  # W is live
    # world -> bev on world rows of its own (the same special yaws, now as world yaws)
    world = _conversion_rows(world_ref, dtype, rng)
    got_bev = rbox_world_bev_device(_cuda(world, dtype), Hinv, "world").cpu().numpy()
    _check_boxes(got_bev, box_ref.rbox_world_bev(world, Hinv, "world"), dtype, "world -> bev")
    if small_row:
        return
    # bev -> world -> bev on the device returns the input
    back = rbox_world_bev_device(got_world, Hinv, "world").cpu().numpy().astype(np.float64)
    if dtype == np.float64:
        box_ref.assert_boxes_close(back, bev[:, :5], rtol=1e-9, atol=1e-8, err_msg="round trip")
    else:
        # two float32 roundings on the way (no float64 bar applies): half an ulp of the world value, carried back at 16 px / m, plus half
        # an ulp of the result -- bounded by whole ulps at the largest magnitudes; the yaw by an ulp at pi each way
        px_per_m = 16.0
        ulp_w = float(np.spacing(np.float32(np.abs(world_ref[:, :4]).max())))
        ulp_b = float(np.spacing(np.float32(np.abs(bev[:, :4]).max())))
        np.testing.assert_allclose(back[:, :4], bev[:, :4], rtol=0, atol=px_per_m * ulp_w + ulp_b, err_msg="round trip")
        assert np.abs(box_ref.yaw_diff(back[:, 4], bev[:, 4])).max() <= 2 * PI32_ULP


# ---- c. the tracker step ------------------------------------------------------------------------------------------------------

IOU_BAR = {np.float64: 1e-12, np.float32: 2e-6}  # the bars of tests/test_gpu_geom.py
MAX_EXACT_PAIRS = 250  # (50-digit arithmetic costs about a millisecond per pair)


def _check_step(out, c, what, exact=False):
    """The outputs of one tracker step against the reference, in the order: boxes, image centres, IoU (oracle on the device's own
    boxes), IoU (50-digit arithmetic on quads, float64 only), the gate."""
    dtype, thr = c["dtype"], c["threshold"]
    dets_bev, trks, H, Him = c["dets_bev"], c["trks"], c["H_world_bev"], c["H_img_world"]
    n, m = len(dets_bev), len(trks)
    torch_dtype = torch.float64 if dtype == np.float64 else torch.float32
    assert out["dets_world"].shape == (n, 5) and out["dets_img"].shape == (n, 2) and out["iou"].shape == (n, m) and out["candidates"].shape == (n, m)
    assert out["dets_world"].dtype == out["iou"].dtype == out["dets_img"].dtype == torch_dtype and out["candidates"].dtype == torch.bool
    dets_world, dets_img = out["dets_world"].cpu().numpy(), out["dets_img"].cpu().numpy()
    iou, cand = out["iou"].cpu().numpy(), out["candidates"].cpu().numpy()
    # 1. the output workgroups' route: sincos, H, atan2
    world_ref = box_ref.rbox_world_bev(dets_bev, H, "bev")
    _check_boxes(dets_world, world_ref, dtype, what + " dets_world")
    _check_points(dets_img, box_ref.centres_img(world_ref, Him), dtype, what + " dets_img", dict(rtol=1e-10, atol=1e-8))
    # 2. the scoring workgroups' route (the heading as a normalised vector, no yaw) against the route verified in 1
    exp_own = co.rbox_iou(dets_world.astype(np.float64), trks[:, :5])
    print("%s iou vs oracle on the device's boxes [%s]: %.3g (bar %g)" % (what, np.dtype(dtype).name, np.abs(iou - exp_own).max(), IOU_BAR[dtype]))
    np.testing.assert_allclose(iou, exp_own, rtol=0, atol=IOU_BAR[dtype], err_msg=what + " iou")
    # 3. 50-digit arithmetic on quadrilaterals: the detections' BEV corners through H, the trackers' world corners
    if exact and dtype == np.float64:
        pytest.importorskip("mpmath")
        from tests.exact_iou import iou_quads
        det_quads, trk_quads = box_ref.through(dets_bev, H, "bev")[:, :4], box_ref.quad(trks, "world")
        pairs = [tuple(p) for p in np.argwhere(np.abs(iou - exp_own) > 1e-13)] + [tuple(p) for p in np.argwhere(exp_own > 0)[::4]]
        pairs = sorted(set(pairs[:MAX_EXACT_PAIRS]))
        assert len(pairs) >= 35
        worst = max(abs(iou[i, j] - iou_quads(det_quads[i], trk_quads[j])) for i, j in pairs)
        print("%s iou vs 50-digit quads on %d pairs: %.3g (bar 1e-13)" % (what, len(pairs), worst))
        assert worst <= 1e-13, what
    # 4. the gate: the device's own IoU, thresholded; and the expected gate wherever the IoU is not within its bar of the threshold
    np.testing.assert_array_equal(cand, iou > dtype(thr), err_msg=what + " candidates")
    exp = co.rbox_iou(world_ref, trks[:, :5])
    clear = np.abs(exp - thr) > 5 * IOU_BAR[dtype]  # (float32: the device scores its float32-rounded boxes, a few 1e-6 of IoU away from `exp`)
    np.testing.assert_array_equal(cand[clear], (exp > thr)[clear], err_msg=what + " candidates vs the expected gate")
    return exp


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("case", ac.TRACKER_CASES, ids=ac.TRACKER_IDS)
def test_tracker_step_under_every_convention(case, dtype):
    from bev_amd.tracker_geom import tracker_geometry_step
    name, kind, key = case
    c = ac.tracker_case(kind, key, dtype)
    out = tracker_geometry_step(_cuda(c["dets_bev"], dtype), _cuda(c["trks"], dtype), c["H_world_bev"], c["threshold"], c["H_img_world"])
    exp = _check_step(out, c, name, exact=True)
    # 5. the case is not vacuous (tests/test_box_ref_cpu.py shows the same numbers discriminate)
    gated, overlapping, ok = ac.non_vacuity(exp, c["threshold"])
    assert ok, (gated, overlapping)


# ---- d. guarded outputs and the edges of the 64-lane workgroups -------------------------------------------------------------------

GUARD = 256
EDGE_SHAPES = [(n, m) for n in (1, 63, 64, 65) for m in (1, 63, 64, 65)] + [(129, 1), (1, 129)]
EDGE_H = [("turning", ("y", "-x")), ("mirroring", ("-y", "-x"))]


def _guarded(shape, dtype):
    """A contiguous `shape` view into the middle of a sentinel-filled allocation (NaN; 0xA5 bytes under a bool view), GUARD elements either side."""
    count = int(np.prod(shape))
    if dtype == torch.bool:
        buf = torch.full((GUARD + count + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        return buf, buf[GUARD:GUARD + count].view(torch.bool).view(shape)
    buf = torch.full((GUARD + count + GUARD,), float("nan"), dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + count].view(shape)


def _bits(buf):
    return buf.view({1: torch.uint8, 4: torch.int32, 8: torch.int64}[buf.element_size()]).cpu().numpy()


def _assert_guards_kept(buf, before, what):
    after = _bits(buf)
    assert np.array_equal(after[:GUARD], before[:GUARD]), what + ": wrote in front of the output"
    assert np.array_equal(after[-GUARD:], before[-GUARD:]), what + ": wrote behind the output"
    inner = after[GUARD:-GUARD]
    if buf.dtype == torch.uint8:
        assert ((inner == 0) | (inner == 1)).all(), what + ": a gate byte was not written"
    else:
        assert not torch.isnan(buf[GUARD:-GUARD]).any(), what + ": an element was not written"


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("h_name,conv", EDGE_H, ids=[h[0] for h in EDGE_H])
def test_guarded_outputs_at_workgroup_edges(h_name, conv, dtype):
    from bev_amd.iou import rbox_iou
    from bev_amd.tracker_geom import tracker_geometry_step
    td = torch.float64 if dtype == np.float64 else torch.float32
    for n, m in EDGE_SHAPES:
        what = "%s %dx%d" % (h_name, n, m)
        c = ac.tracker_case("convention", conv, dtype, n=n, m=m, seed=100 + n + 3 * m)
        bufs = {k: _guarded(shape, t) for k, shape, t in (("dets_world", (n, 5), td), ("iou", (n, m), td), ("candidates", (n, m), torch.bool), ("dets_img", (n, 2), td))}
        before = {k: _bits(b) for k, (b, _) in bufs.items()}
        out = {k: v for k, (_, v) in bufs.items()}
        d, t = _cuda(c["dets_bev"], dtype), _cuda(c["trks"], dtype)
        assert tracker_geometry_step(d, t, c["H_world_bev"], c["threshold"], c["H_img_world"], out=out) is out
        torch.cuda.synchronize()
        for k, (b, _) in bufs.items():
            _assert_guards_kept(b, before[k], what + " " + k)
        exp = _check_step(out, c, what)
        assert (exp[0] > 0).any()  # (the first tracker is the first detection, jittered: even 1 x 1 scores a real pair)
        # rbox_iou into a guarded tensor: the same pairs through the plain IoU kernel
        buf, io = _guarded((n, m), td)
        kept = _bits(buf)
        assert rbox_iou(out["dets_world"], t, out=io) is io
        torch.cuda.synchronize()
        _assert_guards_kept(buf, kept, what + " rbox_iou")
        np.testing.assert_allclose(io.cpu().numpy(), co.rbox_iou(out["dets_world"].double().cpu().numpy(), c["trks"][:, :5]), rtol=0, atol=IOU_BAR[dtype],
                                   err_msg=what + " rbox_iou")


def test_rbox_iou_is_symmetric_and_blind_to_mirroring():
    """The kernel treats its two box sets differently (A is moved into B's frame): IoU(a, b) == IoU(b, a)^T; and mirroring the world
    (x -> -x, yaw -> pi - yaw) changes no IoU."""
    from bev_amd.iou import rbox_iou
    c = ac.tracker_case("shipped", "5_3", np.float64)
    from bev_amd import rbox as host_rbox
    a = host_rbox.rbox_world_bev(c["dets_bev"], c["H_world_bev"], "bev")
    b = c["trks"][:, :5].copy()
    ab = rbox_iou(_cuda(a, np.float64), _cuda(b, np.float64)).cpu().numpy()
    ba = rbox_iou(_cuda(b, np.float64), _cuda(a, np.float64)).cpu().numpy()
    assert ((ab > 0).sum() >= ac.MIN_OVERLAPPING) and ab.shape == (ac.N_DETS, ac.N_TRKS)
    print("symmetry: %.3g (bar 1e-12)" % np.abs(ab - ba.T).max())
    np.testing.assert_allclose(ab, ba.T, rtol=0, atol=1e-12)
    am, bm = a.copy(), b.copy()
    for x in (am, bm):
        x[:, 0] = -x[:, 0]
        x[:, 4] = np.pi - x[:, 4]
    mirrored = rbox_iou(_cuda(am, np.float64), _cuda(bm, np.float64)).cpu().numpy()
    print("mirroring: %.3g (bar 1e-12)" % np.abs(ab - mirrored).max())
    np.testing.assert_allclose(mirrored, ab, rtol=0, atol=1e-12)
