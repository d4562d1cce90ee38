"""The lens warp on the GPU (bev_amd.warp.warp_perspective_lens -> bevwarp_warp_lens), each result compared with the numpy
reference tests/lens_ref.py bit for bit.  Run on the GPU box:  python -m pytest tests -m gpu -q"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from bev_amd import _lib
from tests import lens_ref as LR
from tests import pixels as PX
from tests import workloads as wl

pytestmark = pytest.mark.gpu

LINEAR, NEAREST, INVERSE = 1, 0, 16
INF = float("inf")
GEOMS = {  # (src w, h, dst w, h, forward matrix): inside, edge-cut, outside and (brno, lens A) invalid pixels in one destination
    "rotated_zoom_out": (160, 96, 120, 100, wl.rotated_H(160, 96, 120, 100, 30.0, zoom=2.5)),
    "brno": (640, 360, 160, 120, wl.synth_brno_H(640, 360, 160, 120)),
}
LENSES = {"A": LR.LENS_A, "B": LR.LENS_B}
BORDER = (7.0, 200.0, 31.0, 99.0)  # a non-zero border value per channel


@pytest.fixture(scope="module")
def W():
    from bev_amd import warp
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return warp


@functools.lru_cache(maxsize=None)
def _src(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, shape, dtype=np.uint8) if dtype == np.uint8 else rng.random(shape, dtype=np.float32)


def _dst_shape(src, dsize):
    return (int(dsize[1]), int(dsize[0])) + tuple(src.shape[2:])


def gpu(W, src, M, dsize, K, dist, interp, mode, border_value=None, r2_max=None, canvas=77):
    """One warp_perspective_lens call on a destination filled with `canvas` (pixels a launch leaves unwritten do not pass as zeros)."""
    t = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    out = torch.full(_dst_shape(src, dsize), canvas, dtype=t.dtype, device=t.device)
    got = W.warp_perspective_lens(t, M, dsize, K, dist, flags=interp, border_value=border_value, out=out, border_mode=mode, r2_max=r2_max)
    torch.cuda.synchronize()
    assert got is out
    return got.cpu().numpy()


def ref(src, R, lens, r2_max, dsize, interp, mode, border_value=0.0, canvas=77):
    cv = np.full(_dst_shape(src, dsize), canvas, dtype=src.dtype)
    return LR.warp(src, R, lens, r2_max, dsize, interp, mode, border_value=border_value, canvas=cv)


def check(W, src, M, dsize, K, dist, interp, mode, r2_max=None, m_is_inverse=False):
    """The call against the reference, through the reference's own ray matrix, lens and default r2_max."""
    c = 1 if src.ndim == 2 else src.shape[2]
    bv = BORDER[:c] if mode == LR.CONSTANT else None
    got = gpu(W, src, M, dsize, K, dist, interp | (INVERSE if m_is_inverse else 0), mode, border_value=bv, r2_max=r2_max)
    R, lens = LR.ray_matrix(M, K, inverse_given=m_is_inverse), LR.lens12(K, dist)
    r2 = LR.lens_valid_r2(dist) if r2_max is None else r2_max
    exp = ref(src, R, lens, r2, dsize, interp, mode, border_value=0.0 if bv is None else bv)
    np.testing.assert_array_equal(got, exp, err_msg="mode %d interp %d %s %s" % (mode, interp, src.dtype, src.shape))
    if mode == LR.TRANSPARENT:  # the canvas keeps 77 exactly where the reference writes nothing
        keep = ~LR.written_mask(src.shape[:2], R, lens, r2, dsize, interp)
        assert (got[keep] == 77).all()
    return got


@pytest.mark.parametrize("geom", sorted(GEOMS))
@pytest.mark.parametrize("lens", sorted(LENSES))
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
@pytest.mark.parametrize("mode", [LR.CONSTANT, LR.TRANSPARENT])
def test_matrix(W, geom, lens, dtype, interp, mode):
    sw, sh, dw, dh, M = GEOMS[geom]
    K = LR.camera_K(sw, sh)
    for c in (1, 2, 3, 4):
        check(W, _src((sh, sw, c), dtype, c), M, (dw, dh), K, LENSES[lens], interp, mode)
    check(W, _src((sh, sw), dtype, 9), M, (dw, dh), K, LENSES[lens], interp, mode)  # (H, W) image


@pytest.mark.parametrize("mode", [LR.CONSTANT, LR.TRANSPARENT])
def test_guard_keeps_the_ghosts_out(W, mode):
    """brno with lens A: beyond lens_valid_r2 the model folds back, and without the guard destination pixels far outside the camera's
    view sample the inside of the frame.  r2_max=None (the guard) and r2_max=inf both equal the reference; the ghost pixels hold the border
    value / the canvas in the guarded result."""
    sw, sh, dw, dh, M = GEOMS["brno"]
    K = LR.camera_K(sw, sh)
    R, lens = LR.ray_matrix(M, K), LR.lens12(K, LR.LENS_A)
    sx, sy, _, _, open_valid = LR.maps((dw, dh), R, lens, INF, LINEAR)
    _, _, _, _, guarded_valid = LR.maps((dw, dh), R, lens, LR.lens_valid_r2(LR.LENS_A), LINEAR)
    ghosts = open_valid & LR.inliers(sx, sy, open_valid, sw, sh, LINEAR) & ~guarded_valid
    assert ghosts.sum() > 0
    src = _src((sh, sw, 3), np.uint8, 30)
    guarded = check(W, src, M, (dw, dh), K, LR.LENS_A, LINEAR, mode)
    unguarded = check(W, src, M, (dw, dh), K, LR.LENS_A, LINEAR, mode, r2_max=INF)
    want = np.array(BORDER[:3], np.uint8) if mode == LR.CONSTANT else np.array([77, 77, 77], np.uint8)
    assert (guarded[ghosts] == want).all()
    assert (unguarded[ghosts] != want).any()  # (the frame is random: its samples are not the border value)


def _abi(src_np, R, lens, r2_max, dsize, interp, mode, border_value=None, canvas=77):
    """bevwarp_warp_lens itself, on tight frames ((H, W, C) or (B, H, W, C)), one matrix or one per frame."""
    lib = _lib.load()
    s4 = src_np if src_np.ndim == 4 else src_np[None]
    B, H, Wd, C = s4.shape
    dw, dh = dsize
    t = torch.from_numpy(np.ascontiguousarray(s4)).cuda()
    out = torch.full((B, dh, dw, C), canvas, dtype=t.dtype, device="cuda")
    Rd = torch.from_numpy(np.ascontiguousarray(np.asarray(R, np.float64).reshape(-1, 3, 3))).cuda()
    lens = np.ascontiguousarray(lens, np.float64)
    bv = None if border_value is None else np.ascontiguousarray(border_value, np.float64)
    esz = t.element_size()
    st = lib.bevwarp_warp_lens(t.data_ptr(), out.data_ptr(), B, H, Wd, dh, dw, C, H * Wd * C * esz, Wd * C * esz, dh * dw * C * esz, dw * C * esz, Rd.data_ptr(),
                               Rd.shape[0], lens.ctypes.data_as(ctypes.c_void_p), r2_max, _lib.U8 if t.dtype == torch.uint8 else _lib.F32, interp, mode,
                               None if bv is None else bv.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == 0, st
    got = out.cpu().numpy()
    return got if src_np.ndim == 4 else got[0]


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_pole_zero_w_and_horizon(W, dtype, interp):
    """The rational model's pole at r^2 = 1 (k4 = -1): +-inf with k1 = 0, 0 / 0 with k1 = -1; W == 0 at x = 5, whose pixel samples the
    principal point; and a horizon inside the destination (W changes sign).  None needs a special case: +-inf and NaN round to
    INT_MAX / INT_MIN."""
    src = _src((17, 23, 3), dtype, 40)
    lens = lambda k1, k4: np.array([9.0, 7.0, 11.0, 8.0, k1, 0, 0, 0, 0, k4, 0, 0])  # noqa: E731
    for R in (np.array([[0.125, 0, 0], [0, 0.125, 0], [0, 0, 1.0]]), np.array([[1.0, 0, 0], [0, 1.0, 0], [1.0, 0, -5.0]])):
        for k1 in (0.0, -1.0):
            for mode in (LR.CONSTANT, LR.TRANSPARENT):
                got = _abi(src, R, lens(k1, -1.0), INF, (29, 21), interp, mode, border_value=BORDER[:3])
                np.testing.assert_array_equal(got, ref(src, R, lens(k1, -1.0), INF, (29, 21), interp, mode, border_value=BORDER[:3]))
    _, _, r2 = LR.chain((29, 21), np.array([[0.125, 0, 0], [0, 0.125, 0], [0, 0, 1.0]]), lens(0.0, -1.0))
    assert (r2 == 1.0).any()  # (the pole is hit exactly: x = 8, y = 0)
    got = _abi(src, np.array([[1.0, 0, 0], [0, 1.0, 0], [1.0, 0, -5.0]]), lens(0.0, 0.0), INF, (29, 21), NEAREST, LR.CONSTANT)
    np.testing.assert_array_equal(got[:, 5], np.broadcast_to(src[8, 11], (21, 3)))  # W == 0: (xn, yn) = (0, 0) -> (cx, cy)
    sw, sh = 120, 90
    K = LR.camera_K(sw, sh)
    Minv = np.array([[1.3, 0.2, -30.0], [0.1, 1.1, -20.0], [0.0, 0.02, -0.5]])  # tests/test_gpu_border.py's horizon at row 25
    big = _src((sh, sw, 3), dtype, 41)
    for dist in (LR.LENS_A, LR.LENS_B):
        for mode in (LR.CONSTANT, LR.TRANSPARENT):
            check(W, big, Minv, (96, 50), K, dist, interp, mode, m_is_inverse=True)
            check(W, big, Minv, (96, 50), K, dist, interp, mode, r2_max=INF, m_is_inverse=True)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_widths_and_tiny_sources(W, dtype, interp):
    """Destination widths 29 and 61 (no multiple of 4; the evaluation block's width is then no multiple of 4 either, and a lane's 4 pixels
    straddle two blocks), and 1 x 1, 1 x 9, 9 x 1 and 2 x 2 sources."""
    for dw, dh in ((29, 21), (61, 17)):
        sw, sh = 50, 40
        K = LR.camera_K(sw, sh)
        M = wl.rotated_H(sw, sh, dw, dh, 20.0, zoom=1.7)
        for mode in (LR.CONSTANT, LR.TRANSPARENT):
            check(W, _src((sh, sw, 3), dtype, 50), M, (dw, dh), K, LR.LENS_B, interp, mode)
    for sh, sw in ((1, 1), (1, 9), (9, 1), (2, 2)):
        K = np.array([[6.0, 0, (sw - 1) / 2], [0, 6.0, (sh - 1) / 2], [0, 0, 1.0]])
        Minv = np.array([[0.37, -0.21, -3.0], [0.18, 0.41, -2.5], [0.0005, 0.0, 1.0]])
        for mode in (LR.CONSTANT, LR.TRANSPARENT):
            check(W, _src((sh, sw, 3), dtype, sh * 10 + sw), Minv, (29, 21), K, LR.LENS_B, interp, mode, m_is_inverse=True)


@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
@pytest.mark.parametrize("mode", [LR.CONSTANT, LR.TRANSPARENT])
def test_two_frames_every_stride_padded(W, interp, mode):
    """Two frames with a matrix each, then with a shared one: row and frame strides of source and destination that all differ from the
    tight ones and from each other, a destination of two tile columns (260 > 256) and two tile rows (6 > 4)."""
    sw, sh, dw, dh = 12, 10, 260, 6
    host = np.stack([_src((sh, sw, 3), np.uint8, 60), _src((sh, sw, 3), np.uint8, 61)])
    K = LR.camera_K(sw, sh)
    H = wl.keystone_H(sw, sh, dw, dh)
    Ms = np.stack([wl.jitter_H(H, 1), wl.jitter_H(H, 2)])
    lens, r2 = LR.lens12(K, LR.LENS_B), LR.lens_valid_r2(LR.LENS_B)
    bv = BORDER[:3] if mode == LR.CONSTANT else None
    for M, per_frame in ((Ms, True), (Ms[1], False)):
        src, out = PX.strided(host, (40, 5)), PX.strided(np.full((2, dh, dw, 3), 77, np.uint8), (20, 7))
        assert len({src.stride(0), src.stride(1), out.stride(0), out.stride(1), sh * sw * 3, sw * 3, dh * dw * 3, dw * 3}) == 8
        W.warp_perspective_lens(src, M, (dw, dh), K, LR.LENS_B, flags=interp, border_value=bv, out=out, border_mode=mode)
        torch.cuda.synchronize()
        exp = [ref(host[i], LR.ray_matrix(M[i] if per_frame else M, K), lens, r2, (dw, dh), interp, mode, border_value=0.0 if bv is None else bv) for i in range(2)]
        np.testing.assert_array_equal(out.cpu().numpy(), np.stack(exp))
    assert not np.array_equal(ref(host[0], LR.ray_matrix(Ms[0], K), lens, r2, (dw, dh), interp, mode), ref(host[0], LR.ray_matrix(Ms[1], K), lens, r2, (dw, dh), interp, mode))


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("mode", [LR.CONSTANT, LR.TRANSPARENT])
def test_unaligned_out_view_with_guard_bytes(W, dtype, mode):
    """A destination one element off its allocation's alignment with a row stride that loses the wide stores, inside a holder of canary
    bytes: every pixel is stored on its own, and no byte beside the view is written."""
    sw, sh, dw, dh, M = GEOMS["rotated_zoom_out"]
    K = LR.camera_K(sw, sh)
    src = _src((sh, sw, 3), dtype, 70)
    out, holder = PX.canaried_out((dh, dw, 3), dtype, pad=5, align=0)
    bv = BORDER[:3] if mode == LR.CONSTANT else None
    W.warp_perspective_lens(torch.from_numpy(src).cuda(), M, (dw, dh), K, LR.LENS_A, border_value=bv, out=out, border_mode=mode)
    torch.cuda.synchronize()
    exp = ref(src, LR.ray_matrix(M, K), LR.lens12(K, LR.LENS_A), LR.lens_valid_r2(LR.LENS_A), (dw, dh), LINEAR, mode, border_value=0.0 if bv is None else bv)
    np.testing.assert_array_equal(out.cpu().numpy(), exp)
    PX.assert_canaries_intact(holder, out)


@pytest.mark.parametrize("geom", sorted(GEOMS))
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_identity_lens_through_the_abi_equals_warp_perspective(W, geom, dtype):
    """fx = fy = 1, cx = cy = 0, no distortion, M_ray = M_inv, nearest: the lens kernel against warp_rows, bit for bit."""
    sw, sh, dw, dh, M = GEOMS[geom]
    src = _src((sh, sw, 3), dtype, 80)
    Minv = W.invert_homography(M)
    got = _abi(src, Minv, [1.0, 1.0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], INF, (dw, dh), NEAREST, LR.CONSTANT, border_value=BORDER[:3])
    want = W.warp_perspective(torch.from_numpy(src).cuda(), M, (dw, dh), flags=NEAREST, border_value=BORDER[:3])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got, want.cpu().numpy())


def test_delegation_and_no_stale_lens(W):
    """dist_coeff None and all-zero ARE warp_perspective (bilinear, bit for bit); and a second call with another lens on the same tensors
    and matrices gets its own lens."""
    sw, sh, dw, dh, M = GEOMS["brno"]
    K = LR.camera_K(sw, sh)
    src = _src((sh, sw, 3), np.uint8, 90)
    t = torch.from_numpy(src).cuda()
    want = W.warp_perspective(t, M, (dw, dh), flags=LINEAR, border_value=BORDER[:3]).cpu().numpy()
    for dist in (None, np.zeros(4), np.zeros(5), np.zeros(8)):
        got = W.warp_perspective_lens(t, M, (dw, dh), K, dist, flags=LINEAR, border_value=BORDER[:3])
        np.testing.assert_array_equal(got.cpu().numpy(), want)
    out = torch.empty((dh, dw, 3), dtype=torch.uint8, device="cuda")
    R = LR.ray_matrix(M, K)
    results = []
    for dist in (LR.LENS_A, LR.LENS_B, LR.LENS_A):
        out.fill_(77)
        W.warp_perspective_lens(t, M, (dw, dh), K, dist, flags=LINEAR, out=out)
        torch.cuda.synchronize()
        results.append(out.cpu().numpy())
        np.testing.assert_array_equal(results[-1], ref(src, R, LR.lens12(K, dist), LR.lens_valid_r2(dist), (dw, dh), LINEAR, LR.CONSTANT))
    assert not np.array_equal(results[0], results[1])
