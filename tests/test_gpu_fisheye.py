"""The equidistant (fisheye) lens model on the GPU: bevwarp_warp_lens, bevwarp_build_map and bevwarp_project_points_lens under
BEVWARP_LENS_FISHEYE, and the Python entries' lens_model="fisheye", each result compared with the numpy definition tests/fisheye_ref.py
bit for bit (a stored NaN only has to be a NaN).  The samplers, the stitches and the NV12 route consume nothing but map entries, so one
test each shows that a fisheye map feeds them.  Run on the GPU box:  python -m pytest tests -m gpu -q"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from bev_amd import _lib
from tests import fisheye_ref as FR
from tests import launch_contexts as LC
from tests import nv12_ref as NR
from tests import points_lens_ref as PR
from tests import remap_nv12_out_ref as RNO
from tests import remap_ref as RR
from tests import stitch_maps_ref as SM

pytestmark = pytest.mark.gpu

NEAREST, LINEAR, INVERSE = 0, 1, 16
FISHEYE = FR.FISHEYE
DISTORT, UNDISTORT = 0, 1
INF = float("inf")
BORDER = (7.0, 200.0, 31.0, 99.0)
NP = {"f32": np.float32, "f64": np.float64}
PASS_LANES = 2048 * 256  # one pass of the point launch's grid (bev_amd/csrc/points_lens.h)

# ---- the destination that holds every special ray at once -------------------------------------------------------------------------------------
# Rays straight from a ray matrix: ray(x, y) = (0.5 (x - 2), 0.5 y, 1.5 - 0.25 x), every term exact in the first evaluation block.  Pixel
# (2, 0) lies on the optical axis (Xn == Yn == 0), W changes sign inside every row wider than 6, W == 0 at x == 6, and in row 0 the rays are beyond THETA_MAX
# from x == 50 on.  R_NAN has a NaN: every pixel of its map is invalid.  R_TURNED looks elsewhere.
SW, SH = 64, 48
K_SPECIAL = np.array([[14.0, 0, 31.5], [0, 14.0, 23.5], [0, 0, 1.0]])
LENS = FR.lens12(K_SPECIAL, FR.K_TEST)
THETA_MAX = 2.0
R_SPECIAL = np.array([[0.5, 0.0, -1.0], [0.0, 0.5, 0.0], [-0.25, 0.0, 1.5]])
R_NAN = R_SPECIAL.copy()
R_NAN[1, 1] = np.nan
R_TURNED = np.array([[0.03, -0.01, -0.9], [0.012, 0.028, -0.2], [0.001, -0.002, 1.0]])
RAYS = {1: R_SPECIAL[None], 3: np.stack([R_SPECIAL, R_NAN, R_TURNED])}


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def W():
    from bev_amd import warp
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return warp


@pytest.fixture(scope="module")
def P():
    from bev_amd import points
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return points


@functools.lru_cache(maxsize=None)
def _src(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, shape, dtype=np.uint8) if dtype == np.uint8 else rng.random(shape, dtype=np.float32)
    a.setflags(write=False)
    return a


def test_the_special_destination_holds_every_special_ray():
    """From the reference alone: what the map tests below are said to cover is there, in one destination (65 x 17, three matrices)."""
    Xn, Yn, Wd = FR.rays((65, 17), R_SPECIAL)
    assert Xn[0, 2] == 0 and Yn[0, 2] == 0 and Wd[0, 2] > 0          # on the optical axis
    assert Wd[3, 6] == 0 and (Wd[3, :6] > 0).all() and (Wd[3, 7:] < 0).all()  # W == 0, and both signs in one row
    u, v, theta = FR.chain((65, 17), R_SPECIAL, LENS)
    assert theta[0, 2] == 0 and (u[0, 2], v[0, 2]) == (31.5, 23.5)
    assert theta[0, 6] == FR.PIO2_HI and theta[3, 5] < FR.PIO2_HI < theta[3, 7]
    valid = FR.maps((65, 17), R_SPECIAL, LENS, THETA_MAX, LINEAR)[4]
    assert valid[0, :50].all() and not valid[0, 50:].any()           # beyond theta_max
    xy, _ = FR.build((65, 17), R_SPECIAL, LENS, THETA_MAX, LINEAR)
    inside = RR.written(xy, SW, SH, LINEAR)
    assert inside[:, :9].any() and inside[0, 7] and inside[0, 8]     # rays beyond 90 degrees land inside the frame
    assert not FR.maps((65, 17), R_NAN, LENS, THETA_MAX, LINEAR)[4].any()


# ---- map contents -------------------------------------------------------------------------------------------------------------------------------
def abi_build(R, lens, theta_max, interp, dw, dh, padded=True):
    """bevwarp_build_map | BEVWARP_LENS_FISHEYE on canaried planes; padded: unaligned views with padded rows.  Returns (xy, frac) as numpy
    (n, dh, dw, 2) int16 and (n, dh, dw) uint16 or None."""
    lib = _lib.load()
    n = len(R)
    Rd = torch.from_numpy(np.ascontiguousarray(R, np.float64)).cuda()
    px, pf = (3, 5) if padded else (0, 0)
    xy_buf = torch.full((n, dh + 1, dw + px, 2), 1234, dtype=torch.int16, device="cuda")
    fr_buf = torch.full((n, dh + 1, dw + pf), 1234, dtype=torch.int16, device="cuda")
    o = 1 if padded else 0
    xy, fr = xy_buf[:, :dh, o:o + dw], fr_buf[:, :dh, o:o + dw]
    assert not padded or (xy.data_ptr() % 16 and fr.data_ptr() % 8)
    lens = np.ascontiguousarray(lens, np.float64)
    st = lib.bevwarp_build_map(Rd.data_ptr(), n, ptr(lens), float(theta_max), interp | FISHEYE, xy.data_ptr(), fr.data_ptr() if interp == LINEAR else None, dh, dw,
                               xy.stride(0) * 2, xy.stride(1) * 2, fr.stride(0) * 2, fr.stride(1) * 2, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == 0, st
    xy_all, fr_all = xy_buf.cpu().numpy(), fr_buf.cpu().numpy()
    keep = np.ones(xy_all.shape[:3], bool)
    keep[:, :dh, o:o + dw] = False
    assert (xy_all[keep] == 1234).all(), "the builder wrote outside the xy view"
    if interp == LINEAR:
        keep = np.ones(fr_all.shape, bool)
        keep[:, :dh, o:o + dw] = False
        assert (fr_all[keep] == 1234).all(), "the builder wrote outside the frac view"
    else:
        assert (fr_all == 1234).all(), "a nearest map has no frac plane"
    return xy_all[:, :dh, o:o + dw], (fr_all[:, :dh, o:o + dw].view(np.uint16) if interp == LINEAR else None)


@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("dh", [1, 17])
@pytest.mark.parametrize("dw", [1, 63, 64, 65, 257])
def test_map_contents(interp, n, dh, dw):
    xy, frac = abi_build(RAYS[n], LENS, THETA_MAX, interp, dw, dh)
    for i, R in enumerate(RAYS[n]):
        exy, efrac = FR.build((dw, dh), R, LENS, THETA_MAX, interp)
        np.testing.assert_array_equal(xy[i], exy, err_msg="xy of map %d" % i)
        if interp == LINEAR:
            np.testing.assert_array_equal(frac[i], efrac, err_msg="frac of map %d" % i)


def test_map_contents_aligned_planes_and_no_limit():
    """The lane-wide stores (aligned tight planes), and theta_max = +inf: only the NaN map's pixels are invalid."""
    xy, frac = abi_build(RAYS[3], LENS, INF, LINEAR, 260, 5, padded=False)
    for i, R in enumerate(RAYS[3]):
        exy, efrac = FR.build((260, 5), R, LENS, INF, LINEAR)
        np.testing.assert_array_equal(xy[i], exy)
        np.testing.assert_array_equal(frac[i], efrac)
    assert (xy[1] == -32768).all() and (frac[1] == 0).all() and not (xy[0] == -32768).all()


# ---- the direct warp ------------------------------------------------------------------------------------------------------------------------------
# A camera that looks straight down on the destination's plane from height 1, above the destination's point `at` (fractions of its sides);
# the destination's longer side spans `reach` heights.  M is affine, as every BEVWorldSpec's is.
def bev_setup(sw, sh, dw, dh, turn=0.3, at=(0.45, 0.55), reach=6.0):
    """(K, M_inv): destination px -> UNDISTORTED source px of a pinhole camera K over the plane."""
    K = np.array([[0.45 * sw, 0, (sw - 1) / 2], [0, 0.47 * sw, (sh - 1) / 2 + 1], [0, 0, 1.0]])
    s = reach / max(dw, dh)
    c, sn = np.cos(turn), np.sin(turn)
    P = np.array([[c * s, -sn * s, -at[0] * dw * s], [sn * s, c * s, -at[1] * dh * s], [0, 0, 1.0]])  # destination px -> (X, Y, 1) = the ray
    return K, K @ P


WARP_GEOMS = {"small": (40, 24, 36, 20), "wide": (64, 48, 257, 17)}


def gpu_warp(W, src, Minv, dsize, K, dist, interp, mode, border_value, theta_max=None, canvas=77):
    t = torch.from_numpy(np.array(src)).cuda()
    out = torch.full((dsize[1], dsize[0]) + tuple(src.shape[2:]), canvas, dtype=t.dtype, device="cuda")
    got = W.warp_perspective_lens(t, Minv, dsize, K, dist, flags=interp | INVERSE, border_value=border_value, out=out, border_mode=mode, lens_model="fisheye",
                                  theta_max=theta_max)
    torch.cuda.synchronize()
    assert got is out
    return got.cpu().numpy()


@pytest.mark.parametrize("geom", sorted(WARP_GEOMS))
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
@pytest.mark.parametrize("mode", [RR.CONSTANT, RR.TRANSPARENT])
def test_direct_warp(W, geom, dtype, interp, mode):
    sw, sh, dw, dh = WARP_GEOMS[geom]
    K, Minv = bev_setup(sw, sh, dw, dh)
    R, lens = FR.ray_matrix(Minv, K, inverse_given=True), FR.lens12(K, FR.K_TEST)
    theta_max = 1.2  # (69 degrees: some of the destination is beyond it)
    valid = FR.maps((dw, dh), R, lens, theta_max, interp)[4]
    assert valid.any() and not valid.all()
    for c in (1, 3):
        src = _src((sh, sw, c), dtype, 10 + c)
        bv = BORDER[:c] if mode == RR.CONSTANT else None
        got = gpu_warp(W, src, Minv, (dw, dh), K, FR.K_TEST, interp, mode, bv, theta_max)
        canvas = np.full((dh, dw, c), 77, dtype)
        exp = FR.warp(src, R, lens, theta_max, (dw, dh), interp, mode, 0.0 if bv is None else bv, canvas)
        np.testing.assert_array_equal(got, exp, err_msg="%s c=%d" % (geom, c))
        written = RR.written(FR.build((dw, dh), R, lens, theta_max, interp)[0], sw, sh, interp)
        assert written.any() and not written.all()


def test_direct_warp_default_theta_max_and_minus_M(W):
    """theta_max None is fisheye_valid_theta (pi for this lens: every ray is valid), and -M is the same camera: the ray matrix is oriented."""
    sw, sh, dw, dh = WARP_GEOMS["small"]
    K, Minv = bev_setup(sw, sh, dw, dh)
    src = _src((sh, sw, 3), np.uint8, 3)
    R, lens = FR.ray_matrix(Minv, K, inverse_given=True), FR.lens12(K, FR.K_TEST)
    assert FR.valid_theta(FR.K_TEST) == np.pi == W.fisheye_valid_theta(FR.K_TEST)
    exp = FR.warp(src, R, lens, np.pi, (dw, dh), LINEAR, RR.CONSTANT, BORDER[:3])
    for sign in (1.0, -1.0):
        np.testing.assert_array_equal(gpu_warp(W, src, sign * Minv, (dw, dh), K, FR.K_TEST, LINEAR, RR.CONSTANT, BORDER[:3]), exp)


def abi_warp(src, R, lens, theta_max, dsize, interp, mode, border_value=None):
    """bevwarp_warp_lens | BEVWARP_LENS_FISHEYE itself on tight (B, H, W, C) frames, one ray matrix per frame."""
    lib = _lib.load()
    B, H, Wd, C = src.shape
    dw, dh = dsize
    t = torch.from_numpy(np.array(src)).cuda()
    out = torch.full((B, dh, dw, C), 77, dtype=t.dtype, device="cuda")
    Rd = torch.from_numpy(np.ascontiguousarray(R, np.float64)).cuda()
    lens = np.ascontiguousarray(lens, np.float64)
    bv = None if border_value is None else np.ascontiguousarray(border_value, np.float64)
    esz = t.element_size()
    st = lib.bevwarp_warp_lens(t.data_ptr(), out.data_ptr(), B, H, Wd, dh, dw, C, H * Wd * C * esz, Wd * C * esz, dh * dw * C * esz, dw * C * esz, Rd.data_ptr(),
                               len(R), ptr(lens), float(theta_max), _lib.U8 if t.dtype == torch.uint8 else _lib.F32, interp | FISHEYE, mode, ptr(bv),
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == 0, st
    return out.cpu().numpy()


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
@pytest.mark.parametrize("mode", [RR.CONSTANT, RR.TRANSPARENT])
def test_direct_warp_of_the_special_rays(dtype, interp, mode):
    """The special destination through the warp itself: per-frame ray matrices, one of them with a NaN."""
    dw, dh = 65, 17
    src = np.stack([_src((SH, SW, 3), dtype, 20 + i) for i in range(3)])
    bv = BORDER[:3] if mode == RR.CONSTANT else None
    got = abi_warp(src, RAYS[3], LENS, THETA_MAX, (dw, dh), interp, mode, bv)
    for i, R in enumerate(RAYS[3]):
        exp = FR.warp(src[i], R, LENS, THETA_MAX, (dw, dh), interp, mode, 0.0 if bv is None else bv, np.full((dh, dw, 3), 77, dtype))
        np.testing.assert_array_equal(got[i], exp, err_msg="frame %d" % i)


# ---- the warp against the maps, and the map consumers ------------------------------------------------------------------------------------------------
def fisheye_map(W, Minv, dsize, K, interp=LINEAR, theta_max=None):
    m = W.build_warp_map(Minv, dsize, flags=interp | INVERSE, K=K, dist_coeff=FR.K_TEST, lens_model="fisheye", theta_max=theta_max)
    torch.cuda.synchronize()
    return m


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
@pytest.mark.parametrize("mode", [RR.CONSTANT, RR.TRANSPARENT])
def test_remap_through_a_fisheye_map_equals_the_direct_warp(W, dtype, interp, mode):
    sw, sh, dw, dh = WARP_GEOMS["wide"]
    K, Minv = bev_setup(sw, sh, dw, dh)
    src = _src((sh, sw, 3), dtype, 40)
    bv = BORDER[:3] if mode == RR.CONSTANT else None
    direct = gpu_warp(W, src, Minv, (dw, dh), K, FR.K_TEST, interp, mode, bv, 1.2)
    m = fisheye_map(W, Minv, (dw, dh), K, interp, 1.2)
    exy, efrac = FR.build((dw, dh), FR.ray_matrix(Minv, K, inverse_given=True), FR.lens12(K, FR.K_TEST), 1.2, interp)
    np.testing.assert_array_equal(m.xy[0].cpu().numpy(), exy)
    if interp == LINEAR:
        np.testing.assert_array_equal(m.frac[0].cpu().numpy().view(np.uint16), efrac)
    out = torch.full((dh, dw, 3), 77, dtype=torch.from_numpy(np.zeros(0, dtype)).dtype, device="cuda")
    got = W.remap(torch.from_numpy(np.array(src)).cuda(), m, border_mode=mode, border_value=bv, out=out)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), direct)


@pytest.mark.parametrize("blend,feather", [("over", 64), ("feather", 8)])
def test_stitch_of_two_fisheye_cameras(W, blend, feather):
    sw, sh, dw, dh = 64, 48, 72, 40
    cams = [bev_setup(sw, sh, dw, dh, turn=0.2, at=(0.35, 0.5), reach=4.0), bev_setup(sw, sh, dw, dh, turn=-0.4, at=(0.65, 0.5), reach=4.0)]
    srcs = [_src((sh, sw, 3), np.uint8, 50 + i) for i in range(2)]
    theta_max = 0.9  # (each camera sees a disc of the canvas: the discs overlap, and the corners belong to neither)
    maps = [fisheye_map(W, Minv, (dw, dh), K, LINEAR, theta_max) for K, Minv in cams]
    refs = [FR.build((dw, dh), FR.ray_matrix(Minv, K, inverse_given=True), FR.lens12(K, FR.K_TEST), theta_max, LINEAR) for K, Minv in cams]
    exp, cover = SM.stitch(srcs, refs, LINEAR, SM.OVER if blend == "over" else SM.FEATHER, feather, RR.CONSTANT, BORDER[:3])
    assert set(np.unique(cover)) == {0, 1, 2}
    got = W.remap_stitch([torch.from_numpy(np.array(s)).cuda() for s in srcs], maps, blend=blend, feather=feather, border_value=BORDER[:3])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), exp)


def test_nv12_to_nv12_through_a_fisheye_map(W):
    sw, sh, dw, dh = 64, 48, 72, 40
    K, Minv = bev_setup(sw, sh, dw, dh, reach=4.0)
    y, uv = NR.frame("phase", 7, sh, sw)
    m = fisheye_map(W, Minv, (dw, dh), K, LINEAR, 1.2)
    exy, efrac = FR.build((dw, dh), FR.ray_matrix(Minv, K, inverse_given=True), FR.lens12(K, FR.K_TEST), 1.2, LINEAR)
    ey, euv = RNO.remap_nv12_to_nv12(y, uv, exy, efrac, LINEAR, RR.CONSTANT, BORDER[:3])
    gy, guv = W.split_nv12(W.remap_nv12_to_nv12(torch.from_numpy(np.array(y)).cuda(), torch.from_numpy(np.array(uv)).cuda(), m, border_value=BORDER[:3]))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(gy.cpu().numpy(), ey)
    np.testing.assert_array_equal(guv.cpu().numpy(), euv)


# ---- points ---------------------------------------------------------------------------------------------------------------------------------------------
PSW, PSH, PDW, PDH = 640, 360, 160, 120
PK, PMINV = bev_setup(PSW, PSH, PDW, PDH)
PLENS = FR.lens12(PK, FR.K_TEST)
# DISTORT: 74 degrees, which the far points of the plane exceed; UNDISTORT: 109 degrees -- raw pixels whose rays point away from the plane
PTHETA = {DISTORT: 1.3, UNDISTORT: 1.9}


def matrices(direction):
    """DISTORT: destination px -> ray (oriented).  UNDISTORT: ray -> destination px."""
    return FR.ray_matrix(PMINV, PK, inverse_given=True) if direction == DISTORT else np.linalg.inv(PMINV) @ PK


@functools.lru_cache(maxsize=None)
def points_for(direction, n, dtype, seed=0):
    """DISTORT: destination pixels in and well around the destination.  UNDISTORT: raw pixels in and around the frame, to beyond theta_max."""
    rng = np.random.default_rng(1000 * seed + 10 * n % 997 + direction)
    if direction == DISTORT:
        p = np.stack([rng.uniform(-100, PDW + 100, n), rng.uniform(-100, PDH + 100, n)], axis=1)
    else:
        p = np.stack([rng.uniform(-150, PSW + 150, n), rng.uniform(-150, PSH + 150, n)], axis=1)
    p = p.astype(NP[dtype])
    p.setflags(write=False)
    return p


def abi_points(direction, pts, out, res, n, H, lens, theta_max, iters=10, tol=1e-3):
    H, lens = np.ascontiguousarray(H, np.float64), np.ascontiguousarray(lens, np.float64)
    _lib.launch("bevwarp_project_points_lens", pts.device, pts.data_ptr(), out.data_ptr(), None if res is None else res.data_ptr(), n, ptr(H), ptr(lens),
                float(theta_max), direction | FISHEYE, iters, float(tol), _lib.F32 if pts.dtype == torch.float32 else _lib.F64)
    torch.cuda.synchronize()


def expect(direction, pts, H, lens, theta_max, iters=10, tol=1e-3):
    if direction == DISTORT:
        return FR.distort(pts, H, lens, theta_max), None
    return FR.undistort(pts, H, lens, theta_max, iters, tol)


def check_points(direction, pts, theta_max=None, iters=10, tol=1e-3, H=None, inplace=False, both_verdicts=False):
    H = matrices(direction) if H is None else H
    theta_max = PTHETA[direction] if theta_max is None else theta_max
    n = len(pts)
    t = torch.from_numpy(np.array(pts)).cuda()
    out = t if inplace else torch.full_like(t, 77)
    res = torch.full((n,), 77, dtype=t.dtype, device="cuda") if direction == UNDISTORT else None
    abi_points(direction, t, out, res, n, H, PLENS, theta_max, iters, tol)
    want, want_e = expect(direction, pts, H, PLENS, theta_max, iters, tol)
    assert PR.same_bits(out.cpu().numpy(), want), "out"
    if res is not None:
        assert PR.same_bits(res.cpu().numpy(), want_e), "residual"
    if both_verdicts:
        nan = np.isnan(want).any(axis=1)
        assert nan.any() and (~nan).any()
    return want, want_e


@pytest.mark.parametrize("direction", [DISTORT, UNDISTORT])
@pytest.mark.parametrize("dtype", sorted(NP))
@pytest.mark.parametrize("n", [1, 2, 129, 1000])
def test_points_sizes(direction, dtype, n):
    check_points(direction, points_for(direction, n, dtype), both_verdicts=n == 1000)


@pytest.mark.parametrize("direction", [DISTORT, UNDISTORT])
@pytest.mark.parametrize("dtype", sorted(NP))
def test_points_n_zero_touches_nothing(P, direction, dtype):
    t = torch.from_numpy(np.array(points_for(direction, 4, dtype))).cuda()
    out = torch.full_like(t, 77)
    res = torch.full((4,), 77, dtype=t.dtype, device="cuda") if direction == UNDISTORT else None
    abi_points(direction, t, out, res, 0, matrices(direction), PLENS, INF)
    assert (out == 77).all() and (res is None or (res == 77).all())
    empty = torch.empty((0, 2), dtype=t.dtype, device="cuda")
    assert P.distort_points(empty, PK, FR.K_TEST, lens_model="fisheye").shape == (0, 2)
    got, e = P.undistort_points(empty, PK, FR.K_TEST, return_residual=True, lens_model="fisheye")
    assert got.shape == (0, 2) and e.shape == (0,)


@pytest.mark.parametrize("direction", [DISTORT, UNDISTORT])
@pytest.mark.parametrize("case", ["f32_pairs", "f64"])
def test_points_grid_stride_second_step(direction, case):
    """n = one pass of the launch's grid plus 3.  (2 steps: the reference runs on a million points.)"""
    dtype = "f64" if case == "f64" else "f32"
    n = (2 * PASS_LANES if case == "f32_pairs" else PASS_LANES) + 3
    check_points(direction, points_for(direction, n, dtype), iters=2, tol=INF)


@pytest.mark.parametrize("direction", [DISTORT, UNDISTORT])
def test_points_float32_view_at_an_odd_point(P, direction):
    """A float32 view whose first point is the second of its buffer takes the 8-byte path; through the Python entries."""
    n = 301
    pts = points_for(direction, n, "f32")
    buf = torch.full((n + 1, 2), 77, dtype=torch.float32, device="cuda")
    t = buf[1:]
    t.copy_(torch.from_numpy(np.array(pts)))
    assert t.data_ptr() % 16 == 8
    H = matrices(direction)
    want, want_e = expect(direction, pts, H, PLENS, PTHETA[direction])
    if direction == DISTORT:
        got = P.distort_points(t, PK, FR.K_TEST, H=PMINV, theta_max=PTHETA[direction], lens_model="fisheye")
    else:
        got, e = P.undistort_points(t, PK, FR.K_TEST, H=np.linalg.inv(PMINV), theta_max=PTHETA[direction], return_residual=True, lens_model="fisheye")
    torch.cuda.synchronize()
    assert PR.same_bits(got.cpu().numpy(), want)
    if direction == UNDISTORT:
        assert PR.same_bits(e.cpu().numpy(), want_e)
    assert (buf[0] == 77).all()


@pytest.mark.parametrize("direction", [DISTORT, UNDISTORT])
@pytest.mark.parametrize("dtype", sorted(NP))
def test_points_in_place(direction, dtype):
    check_points(direction, points_for(direction, 1001, dtype), inplace=True)


@pytest.mark.parametrize("direction", [DISTORT, UNDISTORT])
@pytest.mark.parametrize("dtype", sorted(NP))
def test_points_special_inputs(direction, dtype):
    """NaN and +-inf coordinates, the optical axis itself, and (DISTORT) W == 0 and W < 0."""
    pts = np.array(points_for(direction, 64, dtype))
    pts[0], pts[1], pts[2], pts[3] = (np.nan, 5.0), (7.0, np.nan), (np.inf, 3.0), (2.0, -np.inf)
    if direction == DISTORT:
        pts[4], pts[5], pts[6] = (2.0, 0.0), (6.0, 3.0), (8.0, 1.0)  # of R_SPECIAL: on the axis, W == 0, beyond 90 degrees
        want, _ = check_points(direction, pts, theta_max=THETA_MAX, H=R_SPECIAL)
        assert (want[4] == np.array([PLENS[2], PLENS[3]], dtype=want.dtype)).all() and np.isfinite(want[5:7]).all()
    else:
        pts[4] = (PLENS[2], PLENS[3])  # the principal point: thd == 0
        want, want_e = check_points(direction, pts)
        assert np.isfinite(want[4]).all() and want_e[4] == 0
    assert np.isnan(want[:4]).any(axis=1).all()  # (a coordinate whose own chain stays finite is stored as it is: (2, -inf) has u = cx)


@pytest.mark.parametrize("dtype", sorted(NP))
@pytest.mark.parametrize("iters", [1, 100])
@pytest.mark.parametrize("tol", [0.0, INF])
def test_points_iters_and_tolerance(dtype, iters, tol):
    """The step count is part of the definition (1 step is far from converged, 100 steps are all taken), and so is the verdict: tol 0
    keeps only exact reprojections, inf every error that is not NaN."""
    pts = points_for(UNDISTORT, 500, dtype)
    want, want_e = check_points(UNDISTORT, pts, iters=iters, tol=tol)
    ok = ~np.isnan(want).any(axis=1)
    if tol == 0.0:
        assert (want_e[ok] == 0).all()
    else:
        assert (want_e[ok] > 0).any()
    if iters == 1:
        assert np.nanmax(want_e) > 1e-3


def test_points_tie_in_to_the_warp_coordinates():
    """DISTORT at the integer pixels of one evaluation block reproduces the warp's u, v and theta by bits: the map entries follow."""
    dw, dh = 60, 17  # (one block: bw0 = 64)
    R = matrices(DISTORT)
    yy, xx = np.mgrid[0:dh, 0:dw]
    pts = np.stack([xx.ravel(), yy.ravel()], axis=1).astype(np.float64)
    u, v, theta = FR.chain((dw, dh), R, PLENS)
    pu, pv, ptheta = FR.distort_chain(pts, R, PLENS)
    assert np.array_equal(pu.reshape(dh, dw), u) and np.array_equal(pv.reshape(dh, dw), v) and np.array_equal(ptheta.reshape(dh, dw), theta)
    t = torch.from_numpy(pts).cuda()
    out = torch.full_like(t, 77)
    abi_points(DISTORT, t, out, None, len(pts), R, PLENS, INF)
    got = out.cpu().numpy()
    assert PR.same_bits(got[:, 0].reshape(dh, dw), u) and PR.same_bits(got[:, 1].reshape(dh, dw), v)
    xy, _ = abi_build(R[None], PLENS, INF, NEAREST, dw, dh)
    np.testing.assert_array_equal(xy[0, ..., 0], np.clip(np.rint(got[:, 0]), -32768, 32767).reshape(dh, dw).astype(np.int16))
    np.testing.assert_array_equal(xy[0, ..., 1], np.clip(np.rint(got[:, 1]), -32768, 32767).reshape(dh, dw).astype(np.int16))


def test_world_round_trip_through_the_python_entries(P):
    """distort_points then undistort_points returns the destination pixels it started from, for rays up to theta_max."""
    pts = points_for(DISTORT, 2000, "f64")
    t = torch.from_numpy(np.array(pts)).cuda()
    raw = P.distort_points(t, PK, FR.K_TEST, H=PMINV, theta_max=1.3, lens_model="fisheye")
    back, e = P.undistort_points(raw, PK, FR.K_TEST, H=np.linalg.inv(PMINV), theta_max=1.3, return_residual=True, lens_model="fisheye")
    torch.cuda.synchronize()
    raw, back, e = raw.cpu().numpy(), back.cpu().numpy(), e.cpu().numpy()
    ok = ~np.isnan(raw).any(axis=1)
    assert ok.sum() > 100 and (~ok).any()
    theta = FR.distort_chain(pts, matrices(DISTORT), PLENS)[2]
    near = ok & (theta < 1.2)  # (towards 90 degrees the plane's pixels are ill-conditioned in the ray)
    assert near.sum() > 100 and np.nanmax(e[ok]) < 1e-9
    assert np.abs(back[near] - pts[near]).max() < 1e-6


# ---- launch contexts: the three flagged entries on a side stream and under graph replay ------------------------------------------------------------
def _context_cases():
    from bev_amd import points as PT
    from bev_amd import warp as Wm
    K3, dist, theta_max = LC.K3, np.array(FR.K_TEST), 1.0
    lens = FR.lens12(K3, dist)
    rays = lambda M: FR.ray_matrix(M, K3, inverse_given=True)  # noqa: E731
    cases = [LC.Case(
        "fisheye-warp_perspective_lens", "bevwarp_warp_lens", LC.frames, LC._values(M=LC.MINVS["A"], K=K3, dist=dist, border=LC.BORDER), LC.no_maps, LC.PX,
        lambda t, r, h, o: [Wm.warp_perspective_lens(t[0], h["M"], LC.DSIZE, h["K"], h["dist"], flags=LC.FLAGS, border_value=h["border"], out=o[0], lens_model="fisheye",
                                                     theta_max=theta_max)],
        lambda which, hw: LC._stack([FR.warp(f, rays(M), lens, theta_max, LC.DSIZE, LINEAR, RR.CONSTANT, LC.BORDER) for f, M in zip(LC.frames(which)[0], LC.MINVS["A"])]))]

    def built(t, r, h, o):
        m = Wm.build_warp_map(h["M"], LC.DSIZE, flags=LC.FLAGS, K=h["K"], dist_coeff=h["dist"], lens_model="fisheye", theta_max=theta_max,
                              out=Wm.WarpMap(o[0], o[1], LINEAR, LC.DSIZE))
        return [m.xy, m.frac]

    def built_ref(which, hw):
        ref = [FR.build(LC.DSIZE, rays(M), lens, theta_max, LINEAR) for M in LC.MINVS[hw]]
        return [np.stack([xy for xy, _ in ref]), np.stack([frac for _, frac in ref])]

    cases.append(LC.Case("fisheye-build_warp_map", "bevwarp_build_map", LC.no_inputs, lambda which: dict(M=LC.MINVS[which], K=K3, dist=dist), LC.no_maps, LC.MAP_OUT,
                         built, built_ref))
    H = LC.MINVS["A"][0]
    Hf = np.linalg.inv(H)
    cases.append(LC.Case(
        "fisheye-distort_points", "bevwarp_project_points_lens", lambda which: LC.points(which, DISTORT), LC._values(K=K3, dist=dist, H=H), LC.no_maps, LC.POINTS_OUT,
        lambda t, r, h, o: [PT.distort_points(t[0], h["K"], h["dist"], H=h["H"], theta_max=theta_max, out=o[0], lens_model="fisheye")],
        lambda which, hw: [FR.distort(LC.points(which, DISTORT)[0], rays(H), lens, theta_max)], LC.same_points))
    cases.append(LC.Case(
        "fisheye-undistort_points", "bevwarp_project_points_lens", lambda which: LC.points(which, UNDISTORT), LC._values(K=K3, dist=dist, H=Hf), LC.no_maps, LC.POINTS_OUT,
        lambda t, r, h, o: [PT.undistort_points(t[0], h["K"], h["dist"], H=h["H"], theta_max=theta_max, out=o[0], lens_model="fisheye")],
        lambda which, hw: [FR.undistort(LC.points(which, UNDISTORT)[0], Hf @ K3, lens, theta_max, 10, 1e-3)[0]], LC.same_points))
    return cases


CONTEXT_CASES = _context_cases()


@pytest.fixture(scope="module")
def delay():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    cycles, ms = LC.sleep_cycles_for(50.0)
    assert ms >= 20.0, "the delay came out at %.2f ms: too short to enqueue a call behind" % ms
    return cycles


@pytest.mark.parametrize("case", CONTEXT_CASES, ids=repr)
def test_side_stream_behind_a_delay(case, delay):
    LC.check_side_stream(case, LC.Gpu("cuda:0", delay))


@pytest.mark.parametrize("case", CONTEXT_CASES, ids=repr)
def test_capture_and_replay(case):
    LC.check_replays(case, LC.Gpu("cuda:0"))
