"""The kernels on pixel values and on memory around their views that are not neutral (tests/pixels.py).

Float domain   every float32 pixel the other GPU modules feed a kernel lies in [0, 1): positive, normal, one binade.  Here the float
               kernels (bevwarp_warp, bevwarp_warp_planar, bevwarp_warp_border) run on frames of both signs and every binade, with
               subnormals, signed zeros, +-Inf, NaNs and +-FLT_MAX, and are compared BY BITS (same_float): a flush to zero, a dropped
               or quieted NaN, a skipped zero-weight tap (the oracle computes 0 * Inf = NaN there), another summation order, a
               nearest path that sends pixels through arithmetic -- none of them shows on [0, 1) under assert_array_equal.
               The contract: identical bits wherever the oracle's result is not NaN, a NaN of any payload where it
               is; nearest neighbour and border fills copy bits, payloads included.  tests/test_oracle_pixels.py holds the CPU side.
Padding        sources lie inside a larger allocation whose every other byte is 0xA5 (8-bit; the border value is 0 or 9) or NaN
               (float), destinations inside a holder of canary bytes: a tap taken from the row padding, the neighbouring row or frame
               instead of the border value, and a store that spills over the view, are caught by value.

What the geometries of the float-domain cases exercise in warp_rows:
  keystone 640x360 -> 512x80     FAST rows, row-affine tiles          short 100x60 -> 300x9    fewer than 16 rows
  brno     640x360 -> 300x37     edge, outside and patch tiles, ragged   horizon 96x64 -> 128x96  SLOW rows, the guarded sampler
  rotated  640x360 -> 300x77     the patch layout                     src2x2, src5x1           sources smaller than the load window
Run on the GPU box:  python -m pytest tests -m gpu -q"""
import contextlib

import numpy as np
import pytest
import torch

from oracle import cpu_oracle as co
from tests import border_ref as BR
from tests import parity as P
from tests import pixels as PX
from tests import workloads as wl
from tests.parity import report_comparisons  # noqa: F401  (oracle comparisons per launch mode, written at the module's end)
from tests.test_gpu_border import GEOMS as BORDER_GEOMS, MODES as BORDER_MODES

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]  # (numpy's: the references compute 0 * Inf on purpose)

CASES = PX.float_cases()
NAN = float("nan")


@pytest.fixture(scope="module")
def W():
    from bev_amd import warp
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return warp


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_gpu(src, M, dsize, flags, **kw):
    """The warp in both launch modes on a poisoned destination: {mode: host result}."""
    t = src if isinstance(src, torch.Tensor) else cuda(src)
    if "out" not in kw:
        kw = dict(kw, out=P.poisoned_out(t, dsize))
    return P.warp_modes(t, M, dsize, flags, **kw)


def by_bits(payload, msg=""):
    def cmp(got, exp):
        try:
            if exp.dtype == np.float32:
                PX.same_float(got.reshape(exp.shape), exp, payload=payload)
            else:
                np.testing.assert_array_equal(got.reshape(exp.shape), exp)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (msg, e)) from None
    return cmp


@contextlib.contextmanager
def _only(mode):
    keep = P.MODES
    P.MODES = (mode,)
    try:
        yield
    finally:
        P.MODES = keep


def run_canaried(src, M, dsize, flags, out, holder, what="", **kw):
    """warp_modes one launch mode at a time into the canaried `out` (77 before each), the canaries checked after each mode."""
    res = {}
    for mode in tuple(P.MODES):
        out.fill_(77)
        with _only(mode):
            res.update(P.warp_modes(src, M, dsize, flags, out=out, **kw))
        PX.assert_canaries_intact(holder, out, "%s %s mode" % (what, mode))
    return res


# ---- C1: the float domain, constant border --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_float_domain(W, case):
    cid, name, kind, interp, c, border = case
    sw, sh, dw, dh, M, _ = PX.geometries()[name]
    src = PX.float_frame(kind, PX.case_seed(name, kind, c), sh, sw, c)
    exp = co.warp_perspective(src, M, (dw, dh), interp, border_value=border)
    P.check_modes(run_gpu(src, M, (dw, dh), interp, border_value=border), exp, by_bits(interp == 0, cid))


def test_float_domain_full_height_tiles_batched(W):
    """32 frames 640x360 -> 512x768 through jittered keystones, "mixed", bilinear: the straight-line form of full-height tiles and
    the split tail at the end of every XCD's run."""
    B, sw, sh, dw, dh = 32, 640, 360, 512, 768
    uniq = [PX.float_frame("mixed", 70 + i, sh, sw, 3) for i in range(3)]
    Ms = np.stack([wl.jitter_H(wl.keystone_H(sw, sh, dw, dh), g) for g in range(B)])
    t = torch.stack([cuda(uniq[g % 3]) for g in range(B)])
    res = run_gpu(t, Ms, (dw, dh), 1)
    for g in range(B):
        exp = co.warp_perspective(uniq[g % 3], Ms[g], (dw, dh), 1, nthreads=8)
        P.check_modes({m: r[g] for m, r in res.items()}, exp, by_bits(False, "frame %d" % g))


@pytest.mark.parametrize("interp", [0, 1])
def test_blends_of_flt_max_stay_finite(W, interp):
    """Every one of the 1024 weight sets on four +-FLT_MAX taps (tests/test_oracle_pixels.py: the oracle's operation order cannot
    overflow there; another form of the blend can), and a checkerboard of +FLT_MAX and -FLT_MAX."""
    src = np.full((40, 40, 2), PX.FLT_MAX, np.float32)
    src[:, :, 1] = -PX.FLT_MAX
    Minv = np.array([[1 + 1 / 32, 0, 1.0], [0, 1 + 1 / 32, 1.0], [0, 0, 1.0]])
    for s in (src, np.where((np.indices((40, 40)).sum(0) % 2 == 0)[:, :, None], src, -src)):
        exp = co.warp_perspective(s, Minv, (32, 32), interp, m_is_inverse=True)
        assert np.isfinite(exp).all()
        P.check_modes(run_gpu(s, Minv, (32, 32), interp | 16), exp, by_bits(True))


# ---- C2: float planes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("kind", ["mixed", "tiny"])
@pytest.mark.parametrize("name", ["keystone", "brno", "rotated"])
def test_planar_float_domain(W, name, kind, c):
    """bevwarp_warp_planar's float arm: planes of float32(warp) * scale + bias (multiply, then add, each rounded) -- on "tiny" frames
    the products are subnormal, on "mixed" ones some overflow."""
    sw, sh, dw, dh, M, _ = PX.geometries()[name]
    src = PX.float_frame(kind, PX.case_seed(name, kind, c) + 5, sh, sw, c)
    scale, bias = np.linspace(0.5, 2.0, c), np.linspace(-1.0, 1.0, c)  # (c = 3: the middle plane's bias is 0, its products stay subnormal)
    for interp in (0, 1):
        out = torch.full((c, dh, dw), 77, dtype=torch.float32, device="cuda")
        got = W.warp_to_planar(cuda(src), M, (dw, dh), scale=scale, bias=bias, flags=interp, out=out).cpu().numpy()
        ref = co.warp_perspective(src, M, (dw, dh), interp).reshape(dh, dw, c)
        with np.errstate(all="ignore"):
            exp = ref.transpose(2, 0, 1) * scale.astype(np.float32)[:, None, None] + bias.astype(np.float32)[:, None, None]
        assert exp.dtype == np.float32
        by_bits(False, "%s %s c=%d interp=%d" % (name, kind, c, interp))(got, exp)


# ---- C3: the other border modes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", sorted(BORDER_GEOMS))
@pytest.mark.parametrize("mode", BORDER_MODES)
@pytest.mark.parametrize("interp", [0, 1])
def test_border_modes_float_domain(W, geom, mode, interp):
    sw, sh, dw, dh, M = BORDER_GEOMS[geom]
    canvas = np.float32(77)
    for c in (1, 3):
        src = PX.float_frame("mixed", 300 + c, sh, sw, c)
        out = torch.full((dh, dw, c), 77, dtype=torch.float32, device="cuda")
        got = W.warp_perspective(cuda(src), M, (dw, dh), flags=interp, out=out, border_mode=mode).cpu().numpy()
        exp = BR.warp(src, M, (dw, dh), interp, mode, canvas=np.full((dh, dw, c), canvas, np.float32))
        by_bits(interp == 0, "%s interp %d c=%d" % (BR.NAMES[mode], interp, c))(got, exp)
        if mode == BR.TRANSPARENT:  # the canvas keeps its bits where the reference writes nothing
            keep = ~BR.written_mask((sh, sw), M, (dw, dh), interp)
            assert keep.any() and (PX.bits(got)[keep] == PX.bits(canvas)).all()


# ---- C4: points ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("dim", [2, 3])
def test_project_points_degenerate_and_non_finite(dtype, dim):
    """project_points where the divide degenerates: Z exactly 0 with X != 0 (+-Inf), 0 / 0 (NaN), +-Inf and NaN coordinates, and
    images that overflow float32.  H holds signed powers of two, so every product is exact and Z is exactly 0 where it is meant to
    be, whatever the multiply-add form.  NaN masks equal, Inf equal in sign, finite values at test_project_points_config3's bars."""
    from bev_amd.points import project_points
    H = np.array([[2.0, -1.0, 4.0], [1.0, 4.0, -2.0], [1.0, -1.0, 1.0]])  # Z = x - y + w
    rng = np.random.default_rng(17)
    n = 4000
    pts = np.concatenate([rng.uniform(-2000, 2000, (n // 2, 2)), rng.integers(-50, 50, (n // 2, 2)).astype(np.float64)])
    w = np.ones((n, 1))
    if dim == 3:
        w = np.concatenate([rng.uniform(0.5, 2, (n // 2, 1)), rng.integers(-3, 4, (n // 2, 1)).astype(np.float64)])
    pts[2000:2100, 1] = pts[2000:2100, 0] + w[2000:2100, 0]   # y = x + w: Z = 0 exactly, X = x + 3 w, Y = 5 x + 2 w: +-Inf
    pts[2100:2110, 0] = -3.0 * w[2100:2110, 0]                # ... and x = -3 w: X = 0 too, 0 / 0
    pts[2100:2110, 1] = pts[2100:2110, 0] + w[2100:2110, 0]
    big = 3e38 if dtype == np.float32 else 1e308
    special = [np.inf, -np.inf, np.nan, big, -big, 1e30, 0.0, -0.0]
    for i, a in enumerate(special):
        for j, b in enumerate(special):
            pts[2200 + 8 * i + j] = (a, b)
    pts[2300:2400, 0] = 3e38 - np.arange(100) * 1e36                                      # Y = 5 x - 2 w overflows float32 (not float64)
    pts[2300:2400, 1] = pts[2300:2400, 0]
    if dim == 3:
        w[2400:2410, 0] = [np.inf, -np.inf, np.nan, 0.0, -0.0, 1e-300, -1e-300, 1e-40, 5e-324, big]
        pts[2410:2420] = 0.0
        w[2410:2420, 0] = 0.0                                                   # the homogeneous zero vector: 0 / 0 three times
        pts = np.concatenate([pts, w], axis=1)
    with np.errstate(all="ignore"):
        pts = pts.astype(dtype)
    got = project_points(torch.from_numpy(pts).cuda(), H).cpu().numpy()
    exp = co.project_points(pts, H)
    gn, en = np.isnan(got), np.isnan(exp)
    np.testing.assert_array_equal(gn, en)
    np.testing.assert_array_equal(np.where(np.isinf(got), np.sign(got), 0), np.where(np.isinf(exp), np.sign(exp), 0))
    fin = np.isfinite(exp)
    if dtype == np.float64:
        np.testing.assert_allclose(got[fin], exp[fin], rtol=1e-13, atol=0)
    else:
        np.testing.assert_array_equal(got[fin], exp[fin])
    assert en.sum() >= 20 and (exp == np.inf).sum() >= 20 and (exp == -np.inf).sum() >= 20 and fin.mean() > 0.9  # every kind of result occurs


# ---- C5: non-neutral padding and canaries ---------------------------------------------------------------------------------------
PAIR_MAPS = [np.array([[s, 0.0, 4.25 + k / 64], [0.0, 1.5, 30.0 + k / 64], [0.0, 0.0007 * k, 1.0]])
             for s in (0.3, 0.75, 1.0, 1.5, 1.875, 1.93, 1.9375, 1.94, 1.97) for k in (0, 1)] + [
    np.array([[1.99, 0.0, 1.0], [0.0, 1.5, 30.0], [0.0, -0.0004, 1.0]]),     # under the 2 - 1/16 limit at the top, over it at the bottom
    np.array([[-1.5, 0.0, 1000.0], [0.0, 1.5, 30.0], [0.0, 0.0, 1.0]]),      # mirrored
    np.array([[1.0, 0.0, 3.0], [0.0, 1.0, 5.0], [0.0, 0.0, 1.0]]),           # integer shift: every pixel a tie
    np.array([[1.875, 0.0, 0.0], [0.0, 2.0, 8.0], [0.0, 0.0, 1.0]]),         # reaches the frame's first column
    np.array([[1.5, 0.0, 251.75], [0.0, 1.5, 30.0], [0.0, 0.0, 1.0]]),       # x = 511: sx = 1018, the right taps are the last column exactly
    np.array([[1.5, 0.0, 253.25], [0.0, 1.5, 30.0], [0.0, 0.0, 1.0]]),       # ... and one past it: x = 511 takes the border value on the right
    np.array([[1.5, 0.0, 4.25], [0.0, 1.5, 156.0], [0.0, 0.0, 1.0]]),        # y = 95: sy = 298, the lower taps are the last row exactly
    np.array([[1.5, 0.0, 4.25], [0.0, 1.5, 157.0], [0.0, 0.0, 1.0]]),        # ... and one past it
]


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_pair_tiles_beside_padding_that_is_not_the_border(W, offset):
    """test_pair_tiles_scales_mirrors_and_alignments's maps (16-byte pair loads, aligned 12-byte windows) on a source whose padding is
    0xA5, base 0 .. 3 bytes off a 4-byte boundary, row stride a multiple of 4; the default border and border 9."""
    sw, sh, dw, dh = 1020, 300, 512, 96
    src = wl.frame(41 + offset, sh, sw, np.uint8)
    view = PX.padded_source(src, PX.U8_FILL, offset=offset)
    assert view.data_ptr() % 4 == offset and view.stride(0) % 4 == 0
    for i, M in enumerate(PAIR_MAPS):
        for border in (None, 9):
            exp = co.warp_perspective(src, M, (dw, dh), 1, m_is_inverse=True, border_value=border)
            P.check_modes(run_gpu(view, M, (dw, dh), 1 | 16, border_value=border), exp, by_bits(False, "map %d border %s" % (i, border)))


@pytest.mark.parametrize("sw", [637, 638, 639, 640])
def test_row_strides_of_every_residue_beside_padding(W, sw):
    """8-bit RGB bilinear, row strides of every residue mod 4 (RS4 and not) and bases of every residue, padding 0xA5."""
    M = wl.synth_brno_H(1920, 1080, 512, 48) @ np.diag([1920 / sw, 1080 / 359, 1.0])
    src = wl.frame(30, 359, sw, np.uint8)
    for border in (None, 9):
        exp = co.warp_perspective(src, M, (512, 48), 1, border_value=border)
        bases = set()
        for offset in (0, 1, 2, 3):
            view = PX.padded_source(src, PX.U8_FILL, offset=offset)
            assert view.stride(0) % 4 == (3 * sw) % 4
            bases.add(view.data_ptr() % 4)
            P.check_modes(run_gpu(view, M, (512, 48), 1, border_value=border), exp, by_bits(False, "offset %d border %s" % (offset, border)))
        assert bases == {0, 1, 2, 3}


@pytest.mark.parametrize("c", [1, 2, 3, 4])
@pytest.mark.parametrize("interp", [0, 1])
def test_u8_channels_and_nearest_beside_padding(W, c, interp):
    sw, sh, dw, dh = 640, 360, 300, 37
    M = wl.synth_brno_H(sw, sh, dw, dh)
    src = wl.frame(33, sh, sw, np.uint8, c)
    for border in (None, 9):
        exp = co.warp_perspective(src, M, (dw, dh), interp, border_value=border)
        for offset in (0, 1, 2, 3):
            view = PX.padded_source(src, PX.U8_FILL, offset=offset)
            P.check_modes(run_gpu(view, M, (dw, dh), interp, border_value=border), exp, by_bits(False, "offset %d border %s" % (offset, border)))


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("interp", [0, 1])
@pytest.mark.parametrize("name", ["keystone", "rotated"])
def test_float_beside_nan_padding(W, name, interp, c):
    """Ordinary [0, 1) frames inside NaN padding: any NaN in the result was fetched from beside the frame."""
    sw, sh, dw, dh, M, _ = PX.geometries()[name]
    src = wl.frame(34, sh, sw, np.float32, c)
    for border in (None, PX.BORDER[:c]):
        exp = co.warp_perspective(src, M, (dw, dh), interp, border_value=border)
        assert not np.isnan(exp).any()
        for offset in (0, 1, 2, 3):  # bases 0, 4, 8, 12 bytes off a 16-byte boundary
            view = PX.padded_source(src, NAN, offset=offset)
            P.check_modes(run_gpu(view, M, (dw, dh), interp, border_value=border), exp, by_bits(interp == 0, "offset %d border %s" % (offset, border)))


def _store_align(dtype, c):
    """The alignment bevwarp_warp's wide stores need of an interleaved destination (base, row and frame stride)."""
    return 16 if dtype == np.float32 else {1: 4, 2: 8, 3: 4, 4: 16}[c]


DST_GEOMS = {  # destination widths whose last lane is ragged
    301: (637, 355, 301, 45, wl.rotated_H(637, 355, 301, 45, 33.0, 1.7)),    # patches; reaches past the frame on two sides
    515: (640, 360, 515, 40, wl.rotated_H(640, 360, 515, 40, -12.0, 1.6)),  # three tiles wide, the last one 3 pixels
    130: (640, 360, 130, 16, wl.keystone_H(640, 360, 130, 16)),             # row segments
}


@pytest.mark.parametrize("dw", sorted(DST_GEOMS))
@pytest.mark.parametrize("dtype,c", [(np.uint8, 1), (np.uint8, 2), (np.uint8, 3), (np.uint8, 4), (np.float32, 1), (np.float32, 3)])
def test_wide_stores_stay_inside_padded_destinations(W, dw, dtype, c):
    """Destinations with padded rows that keep the alignment the wide stores need (dst_vec_ok holds: the ragged last lane must fall
    back to element stores) and that lose it, single frames and batches of 3 with a gap between the frames; sources inside
    non-neutral padding.  The canaries around the view are checked after each launch mode."""
    sw, sh, _, dh, M = DST_GEOMS[dw]
    B = 3
    frames = np.stack([wl.frame(50 + i, sh, sw, dtype, c) for i in range(B)])
    Ms = np.stack([wl.jitter_H(M, i, px=3.0) for i in range(B)])
    fill = PX.U8_FILL if dtype == np.uint8 else NAN
    view = PX.padded_source(frames, fill, offset=0)
    pad = 4 if (dtype == np.uint8 and c == 1) else 16
    for interp in (0, 1):
        exp = [co.warp_perspective(frames[i], Ms[i], (dw, dh), interp).reshape(dh, dw, c) for i in range(B)]
        for align in (_store_align(dtype, c), 0):
            what = "interp %d align %d" % (interp, align)
            out, holder = PX.canaried_out((dh, dw, c), dtype, pad, align=align)
            res = run_canaried(view[0], Ms[0], (dw, dh), interp, out, holder, what)
            P.check_modes(res, exp[0], by_bits(interp == 0, what))
            out, holder = PX.canaried_out((B, dh, dw, c), dtype, pad, align=align)
            res = run_canaried(view, Ms, (dw, dh), interp, out, holder, what + " batch")
            for i in range(B):
                P.check_modes({m: r[i] for m, r in res.items()}, exp[i], by_bits(interp == 0, what + " frame %d" % i))


@pytest.mark.parametrize("mode", BORDER_MODES)
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_border_modes_beside_padding_and_canaries(W, mode, dtype):
    """bevwarp_warp_border: the source-reading modes never leave the frame, so nothing of the padding may show; destination canaried."""
    sw, sh, dw, dh, M = BORDER_GEOMS["rotated_zoom_out"]
    for c in (1, 3):
        src = wl.frame(55, sh, sw, dtype, c)
        for offset in (0, 1):
            view = PX.padded_source(src, PX.U8_FILL if dtype == np.uint8 else NAN, offset=offset)
            for interp in (0, 1):
                exp = BR.warp(src, M, (dw, dh), interp, mode, canvas=np.full((dh, dw, c), 77, dtype))
                for align in (_store_align(dtype, c), 0):
                    what = "%s c=%d offset %d interp %d align %d" % (BR.NAMES[mode], c, offset, interp, align)
                    out, holder = PX.canaried_out((dh, dw, c), dtype, 16, align=align)
                    got = W.warp_perspective(view, M, (dw, dh), flags=interp, out=out, border_mode=mode)
                    torch.cuda.synchronize()
                    assert got is out
                    PX.assert_canaries_intact(holder, out, what)
                    by_bits(interp == 0, what)(out.cpu().numpy(), exp)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("name", ["keystone", "brno", "rotated"])
def test_planar_output_into_padded_planes(W, name, dtype):
    """warp_to_planar with `out` a view whose rows and planes are padded (aligned: 16-byte stores; not: element stores), batched."""
    sw, sh, dw, dh, M, _ = PX.geometries()[name]
    B = 2
    for c in (1, 3, 4):
        frames = np.stack([wl.frame(57 + i, sh, sw, dtype, c) for i in range(B)])
        view = PX.padded_source(frames, PX.U8_FILL if dtype == np.uint8 else NAN, offset=1)
        scale, bias = np.linspace(0.5, 2.0, c), np.linspace(-1.0, 1.0, c)
        for interp in (0, 1):
            exp = np.stack([co.warp_perspective(frames[i], M, (dw, dh), interp).reshape(dh, dw, c).transpose(2, 0, 1).astype(np.float32)
                            * scale.astype(np.float32)[:, None, None] + bias.astype(np.float32)[:, None, None] for i in range(B)])
            for align in (16, 0):
                what = "%s c=%d interp %d align %d" % (name, c, interp, align)
                out, holder = PX.canaried_out((B, c, dh, dw), np.float32, 16, align=align, planar=True)
                assert W.warp_to_planar(view, M, (dw, dh), scale=scale, bias=bias, flags=interp, out=out) is out
                torch.cuda.synchronize()
                PX.assert_canaries_intact(holder, out, what)
                by_bits(False, what)(out.cpu().numpy(), exp.astype(np.float32))


@pytest.mark.parametrize("c", [1, 3])
def test_composite_of_padded_views(c):
    """composite_bev_img with background, foreground and mask as views inside 0xA5 padding, at the first geometry of
    test_warp_composite_every_channel_count (guarded taps: a small odd-sized foreground, maps that leave the frames)."""
    from bev_amd.compo import composite_bev_img
    from bev_amd.homo import homo_from_KRt
    K = np.array([[400.0, 0, 159.0], [0, 395.0, 88.5], [0, 0, 1.0]])
    cth, sth = np.cos(0.8), np.sin(0.8)
    RT = np.array([[1, 0, 0, 0.0], [0, cth, -sth, 2.0], [0, sth, cth, 14.0], [0, 0, 0, 1.0]])
    H_world2bev = np.array([[0.0, 14.0, 250.0], [-14.0, 0.0, 60.0], [0.0, 0.0, 1.0]])
    H_img2world_fix = np.linalg.inv(homo_from_KRt(K, Rt_homo=RT)) @ np.array([[1, 0, 2.0], [0, 1, -1.0], [0, 0, 1]])
    fh, fw, dw, dh = 177, 319, 301, 517
    bg, fg, mask = wl.frame(20, 360, 640, np.uint8, c), wl.frame(21, fh, fw, np.uint8, c), wl.frame(22, fh, fw, np.uint8, c)
    Ks = np.diag([fw / 320.0, fh / 178.0, 1.0]) @ K
    for offset in (0, 1):
        views = [PX.padded_source(x, PX.U8_FILL, offset=offset) for x in (bg, fg, mask)]
        got, Hcam = composite_bev_img(views[0], views[1], views[2], H_world2bev, H_img2world_fix, Ks, RT, dw, dh)
        Hb, Hc = H_world2bev.dot(H_img2world_fix), H_world2bev.dot(np.linalg.inv(Hcam))
        fb, ff, fm = (co.warp_perspective(x, H, (dw, dh)).astype(np.float64).reshape(dh, dw, c) for x, H in ((bg, Hb), (fg, Hc), (mask, Hc)))
        exp = np.minimum((ff * (fm / 255) + fb * (1 - fm / 255)).round(), 255).astype(np.uint8)
        np.testing.assert_array_equal(got.cpu().numpy(), exp, err_msg="offset %d" % offset)
        assert 0.02 < (fm > 0).mean() < 1.0


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_resize_beside_padding_and_canaries(c):
    """bevwarp_resize's four-pixels-per-lane kernel (8-byte tap windows, dword stores) and its one-pixel kernel: three of the cases of
    test_resize_four_pixels_per_lane_kernel_corners -- a source row of 8 bytes, the 4 x magnification (one-tap columns at the row's
    end), a ragged last lane -- with the source inside 0xA5 padding and the destination canaried, aligned and not."""
    from bev_amd.resize import resize
    rng = np.random.default_rng(199)
    for sh, sw, dh, dw in ((33, (8 + c - 1) // c, 20, 64), (50, 97, 31, 400), (61, 45, 47, 4 * 37 + 4 // int(np.gcd(4, c)))):
        img = rng.integers(0, 256, (3, sh, sw, c), dtype=np.uint8)
        exp = np.stack([co.resize_linear_u8(img[i], (dw, dh)).reshape(dh, dw, c) for i in range(3)])
        for offset in (0, 3):
            view = PX.padded_source(img, PX.U8_FILL, offset=offset)
            for align in (4, 0):
                what = "%dx%dx%d -> %dx%d offset %d align %d" % (sw, sh, c, dw, dh, offset, align)
                out, holder = PX.canaried_out((3, dh, dw, c), np.uint8, 4, align=align)
                assert resize(view, (dw, dh), out=out) is out
                torch.cuda.synchronize()
                PX.assert_canaries_intact(holder, out, what)
                np.testing.assert_array_equal(out.cpu().numpy(), exp, err_msg=what)
