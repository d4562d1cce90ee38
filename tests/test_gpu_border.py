"""The warp's border modes on the GPU (bev_amd.warp.warp_perspective(border_mode=...) -> bevwarp_warp_border), each result
compared with the numpy reference tests/border_ref.py bit for bit.  Run on the GPU box:  python -m pytest tests -m gpu -q"""
import numpy as np
import pytest
import torch

from tests import border_ref as BR
from tests import workloads as wl

pytestmark = pytest.mark.gpu

LINEAR, NEAREST, INVERSE = 1, 0, 16


@pytest.fixture(scope="module")
def W():
    from bev_amd import warp
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return warp


def _src(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, shape, dtype=np.uint8) if dtype == np.uint8 else rng.random(shape, dtype=np.float32)


def _dst_shape(src, dsize):
    return (int(dsize[1]), int(dsize[0])) + tuple(src.shape[2:])


def gpu(W, src, M, dsize, interp, mode, canvas=77, **kw):
    """One warp_perspective call on a destination filled with `canvas` (pixels a launch leaves unwritten do not pass as zeros)."""
    t = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    out = torch.full(_dst_shape(src, dsize), canvas, dtype=t.dtype, device=t.device)
    got = W.warp_perspective(t, M, dsize, flags=interp, out=out, border_mode=mode, **kw)
    torch.cuda.synchronize()
    assert got is out
    return got.cpu().numpy()


def ref(src, M, dsize, interp, mode, canvas=77, m_is_inverse=False):
    cv = np.full(_dst_shape(src, dsize), canvas, dtype=src.dtype)
    return BR.warp(src, M, dsize, interp, mode, m_is_inverse=m_is_inverse, canvas=cv)


def check(W, src, M, dsize, interp, mode, m_is_inverse=False):
    got = gpu(W, src, M, dsize, interp | (INVERSE if m_is_inverse else 0), mode)
    exp = ref(src, M, dsize, interp, mode, m_is_inverse=m_is_inverse)
    np.testing.assert_array_equal(got, exp, err_msg="%s interp %d %s %s" % (BR.NAMES[mode], interp, src.dtype, src.shape))
    if mode == BR.TRANSPARENT:  # the canvas keeps 77 exactly where the reference writes nothing
        keep = ~BR.written_mask(src.shape[:2], M, dsize, interp, m_is_inverse)
        assert (got[keep] == 77).all()


MODES = (BR.REPLICATE, BR.REFLECT, BR.WRAP, BR.REFLECT_101, BR.TRANSPARENT)
GEOMS = {  # (src w, h, dst w, h, forward matrix): inside, edge and far-outside pixels in one destination
    "rotated_zoom_out": (160, 96, 120, 100, wl.rotated_H(160, 96, 120, 100, 30.0, zoom=2.5)),
    "brno": (640, 360, 160, 120, wl.synth_brno_H(640, 360, 160, 120)),
}


@pytest.mark.parametrize("geom", sorted(GEOMS))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_mode_matrix(W, geom, mode, dtype, interp):
    sw, sh, dw, dh, M = GEOMS[geom]
    for c in (1, 2, 3, 4):
        check(W, _src((sh, sw, c), dtype, seed=c), M, (dw, dh), interp, mode)
    check(W, _src((sh, sw), dtype, seed=9), M, (dw, dh), interp, mode)  # (H, W) image


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("mode", [BR.REPLICATE, BR.REFLECT_101])
@pytest.mark.parametrize("per_frame", [False, True])
def test_config1_full_size(W, dtype, mode, per_frame):
    """BASELINE configs[1]: 32 x 1080p -> 1024^2 keystone, bilinear, shared or jitter_H per-frame matrices."""
    B, sw, sh, dw, dh = 32, 1920, 1080, 1024, 1024
    H = wl.keystone_H(sw, sh, dw, dh)
    frames = [wl.frame(i, sh, sw, dtype) for i in range(4)]
    src = torch.from_numpy(np.stack([frames[i % 4] for i in range(B)])).cuda()
    M = np.stack([wl.jitter_H(H, i) for i in range(B)]) if per_frame else H
    got = W.warp_perspective(src, M, (dw, dh), flags=LINEAR, border_mode=mode)
    torch.cuda.synchronize()
    check_frames = (0, 1, 17, 31) if per_frame else range(B)
    exp = {}
    for i in check_frames:
        k = i if per_frame else i % 4
        if k not in exp:
            exp[k] = BR.warp(frames[i % 4], M[i] if per_frame else M, (dw, dh), LINEAR, mode)
        np.testing.assert_array_equal(got[i].cpu().numpy(), exp[k], err_msg="frame %d" % i)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_tiny_sources(W, dtype, interp):
    """1 x N, N x 1, 1 x 1 and 2 x 2 sources (len 1 maps every index to 0; REFLECT_101's period 2n - 2 is 0 there)."""
    for sh, sw in ((1, 9), (9, 1), (1, 1), (2, 2)):
        Minv = np.array([[0.37, -0.21, -3.0], [0.18, 0.41, -2.5], [0.0005, 0.0, 1.0]])
        for mode in MODES:
            check(W, _src((sh, sw, 3), dtype, seed=sh * 10 + sw), Minv, (29, 21), interp, mode, m_is_inverse=True)


@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_coordinates_beyond_int16(W, interp):
    """Source coordinates past +-32768 saturate to int16 BEFORE WRAP / REFLECT (a width that is not a power of two)."""
    src = _src((23, 37, 3), np.uint8, seed=7)
    for Minv in (np.array([[3.0, 0.5, 40000.0], [-0.25, 2.0, -50000.0], [0, 0, 1.0]]),
                 np.array([[900.0, 0.0, -20000.0], [0.0, -700.0, 9000.0], [0, 0, 1.0]])):  # crosses +-32768 inside the destination
        for mode in MODES:
            check(W, src, Minv, (64, 20), interp, mode, m_is_inverse=True)
            check(W, src.astype(np.float32) / 255, Minv, (64, 20), interp, mode, m_is_inverse=True)


def test_nan_coordinate(W):
    """A denormal W with a zero numerator: 32 / W overflows, 0 * inf is NaN, and the reference maps NaN to INT_MAX (not INT_MIN)."""
    src = _src((17, 23, 3), np.uint8, seed=8)
    Minv = np.array([[0.0, 0, 0], [0, 0.0, 0], [0, 0, 5e-324]])
    for interp in (NEAREST, LINEAR):
        for mode in (BR.REPLICATE, BR.WRAP, BR.REFLECT):
            check(W, src, Minv, (40, 6), interp, mode, m_is_inverse=True)
    got = gpu(W, src, Minv, (40, 6), LINEAR | INVERSE, BR.REPLICATE)
    assert (got == src[-1, -1]).all()  # sx = sy = 32767 -> the last pixel


@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_horizon_inside_destination(W, interp):
    """W changes sign inside the destination (a horizon at row 25): the rows beyond it map through negative W."""
    src = _src((90, 120, 3), np.float32, seed=10)
    Minv = np.array([[1.3, 0.2, -30.0], [0.1, 1.1, -20.0], [0.0, 0.02, -0.5]])
    for mode in MODES:
        check(W, src, Minv, (96, 50), interp, mode, m_is_inverse=True)
        check(W, (src * 255).astype(np.uint8), Minv, (96, 50), interp, mode, m_is_inverse=True)


def test_warp_inverse_map_equals_forward(W):
    sw, sh, dw, dh, M = GEOMS["brno"]
    src = _src((sh, sw, 3), np.uint8, seed=11)
    Minv = np.linalg.inv(M)
    for mode in MODES:
        check(W, src, Minv, (dw, dh), LINEAR, mode, m_is_inverse=True)


def test_strided_batch_and_unaligned_output(W):
    """A batch whose frames are windows of larger frames (row and frame strides of their own), per-frame matrices, and an 8-bit
    RGB destination at an odd address (every pixel stored on its own)."""
    B, sw, sh, dw, dh = 3, 150, 90, 77, 45
    big = _src((B, sh + 7, sw + 11, 3), np.uint8, seed=12)
    src = torch.from_numpy(big).cuda()[:, 3:3 + sh, 5:5 + sw, :]
    H = wl.rotated_H(sw, sh, dw, dh, 20.0, zoom=2.2)
    Ms = np.stack([wl.jitter_H(H, i, px=6.0) for i in range(B)])
    host = big[:, 3:3 + sh, 5:5 + sw, :]
    for mode in MODES:
        buf = torch.full((B * dh * dw * 3 + 1,), 77, dtype=torch.uint8, device="cuda")
        out = buf[1:].view(B, dh, dw, 3)
        assert out.data_ptr() % 2 == 1
        W.warp_perspective(src, Ms, (dw, dh), flags=LINEAR, out=out, border_mode=mode)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert buf[0].item() == 77
        for i in range(B):
            exp = BR.warp(host[i], Ms[i], (dw, dh), LINEAR, mode, canvas=np.full((dh, dw, 3), 77, np.uint8))
            np.testing.assert_array_equal(got[i], exp, err_msg="%s frame %d" % (BR.NAMES[mode], i))


@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_two_frames_two_matrices_every_stride_padded(W, interp):
    """What an entry point's argument filling can get wrong -- a swapped or dropped stride or pointer -- in the smallest shape that shows
    it: two frames with a matrix each, row and frame strides of source and destination that all differ from the tight ones and from each
    other, a destination of two tile columns (260 > 256) and two tile rows (6 > 4)."""
    from tests import pixels as PX
    sw, sh, dw, dh = 12, 10, 260, 6
    host = _src((2, sh, sw, 3), np.uint8, seed=19)
    H = wl.keystone_H(sw, sh, dw, dh)
    Ms = np.stack([wl.jitter_H(H, 1), wl.jitter_H(H, 2)])
    src, out = PX.strided(host, (40, 5)), PX.strided(np.full((2, dh, dw, 3), 77, np.uint8), (20, 7))
    assert len({src.stride(0), src.stride(1), out.stride(0), out.stride(1), sh * sw * 3, sw * 3, dh * dw * 3, dw * 3}) == 8
    W.warp_perspective(src, Ms, (dw, dh), flags=interp, out=out, border_mode=BR.REFLECT_101)
    torch.cuda.synchronize()
    exp = [ref(host[i], Ms[i], (dw, dh), interp, BR.REFLECT_101) for i in range(2)]
    np.testing.assert_array_equal(out.cpu().numpy(), np.stack(exp))
    assert not np.array_equal(exp[0], ref(host[0], Ms[1], (dw, dh), interp, BR.REFLECT_101))  # (the two matrices give different frames)


def test_transparent_two_camera_mosaic(W):
    """cv2's stitching idiom: warpPerspective(cam_k, H_k, dsize, dst=canvas, borderMode=BORDER_TRANSPARENT) per camera."""
    dw, dh = 200, 120
    cams = [_src((90, 160, 3), np.uint8, seed=13), _src((100, 140, 3), np.uint8, seed=14)]
    Hs = [np.array([[0.9, 0.1, 5.0], [-0.05, 1.0, 10.0], [0, 0, 1.0]]), np.array([[1.1, -0.1, 70.0], [0.08, 0.95, 20.0], [0.0002, 0, 1.0]])]
    canvas = torch.full((dh, dw, 3), 9, dtype=torch.uint8, device="cuda")
    exp = np.full((dh, dw, 3), 9, np.uint8)
    for cam, H in zip(cams, Hs):
        W.warp_perspective(torch.from_numpy(cam).cuda(), H, (dw, dh), flags=LINEAR, out=canvas, border_mode=W.BORDER_TRANSPARENT)
        exp = BR.warp(cam, H, (dw, dh), LINEAR, BR.TRANSPARENT, canvas=exp)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(canvas.cpu().numpy(), exp)
    assert (exp == 9).any() and (exp != 9).any()  # (the mosaic has uncovered and covered pixels)
    # without `out`, uncovered pixels are zero
    got = W.warp_perspective(torch.from_numpy(cams[0]).cuda(), Hs[0], (dw, dh), border_mode=W.BORDER_TRANSPARENT)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), BR.warp(cams[0], Hs[0], (dw, dh), LINEAR, BR.TRANSPARENT))


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_constant_keyword_is_the_default(W, dtype):
    sw, sh, dw, dh, M = GEOMS["brno"]
    t = torch.from_numpy(_src((sh, sw, 3), dtype, seed=15)).cuda()
    a = W.warp_perspective(t, M, (dw, dh), border_value=(3, 4, 5))
    b = W.warp_perspective(t, M, (dw, dh), border_value=(3, 4, 5), border_mode=W.BORDER_CONSTANT)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())


def test_plan_path_never_serves_another_mode(W):
    """The same (src, out, M_inv_device) buffers called CONSTANT -> REPLICATE -> CONSTANT -> REPLICATE: the validated-launch cache
    (plans) must give each call its own mode."""
    sw, sh, dw, dh, M = GEOMS["rotated_zoom_out"]
    src = _src((sh, sw, 3), np.uint8, seed=16)
    t = torch.from_numpy(src).cuda()
    out = torch.empty((dh, dw, 3), dtype=torch.uint8, device="cuda")
    minv = torch.from_numpy(np.linalg.inv(M)[None]).cuda()
    Minv = minv[0].cpu().numpy()
    for mode in (BR.CONSTANT, BR.REPLICATE, BR.CONSTANT, BR.REPLICATE, BR.WRAP):
        out.fill_(77)
        W.warp_perspective(t, None, (dw, dh), flags=LINEAR, out=out, M_inv_device=minv, border_mode=mode)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), ref(src, Minv, (dw, dh), LINEAR, mode, m_is_inverse=True), err_msg=BR.NAMES[mode])


def test_cv2_compat_numpy_in_out(W):
    from bev_amd import cv2_compat as cv2
    sw, sh, dw, dh, M = GEOMS["rotated_zoom_out"]
    src = _src((sh, sw, 3), np.uint8, seed=17)
    for mode in (cv2.BORDER_CONSTANT, cv2.BORDER_REPLICATE, cv2.BORDER_REFLECT, cv2.BORDER_WRAP, cv2.BORDER_REFLECT_101, cv2.BORDER_TRANSPARENT):
        got = cv2.warpPerspective(src, M, (dw, dh), flags=cv2.INTER_LINEAR, borderMode=mode, borderValue=(1, 2, 3))
        exp = BR.warp(src, M, (dw, dh), LINEAR, mode, border_value=(1, 2, 3))
        np.testing.assert_array_equal(got, exp, err_msg=BR.NAMES[mode])
    canvas = np.full((dh, dw, 3), 55, np.uint8)
    exp = BR.warp(src, M, (dw, dh), NEAREST, BR.TRANSPARENT, canvas=canvas)
    got = cv2.warpPerspective(src, M, (dw, dh), canvas, cv2.INTER_NEAREST, cv2.BORDER_TRANSPARENT)
    assert got is canvas
    np.testing.assert_array_equal(canvas, exp)
    with pytest.raises(ValueError):
        cv2.warpPerspective(src, M, (dw, dh), np.zeros((dh, dw + 1, 3), np.uint8), cv2.INTER_LINEAR, cv2.BORDER_TRANSPARENT)
    with pytest.raises(ValueError):
        cv2.warpPerspective(src, M, (dw, dh), np.zeros((dh, dw, 3), np.float32), cv2.INTER_LINEAR, cv2.BORDER_TRANSPARENT)


def test_graph_capture_replicate(W):
    """One torch.cuda.graph capture of a REPLICATE warp (M_inv_device given), one replay."""
    sw, sh, dw, dh, M = GEOMS["brno"]
    src = _src((sh, sw, 3), np.uint8, seed=18)
    t = torch.from_numpy(src).cuda()
    out = torch.empty((dh, dw, 3), dtype=torch.uint8, device="cuda")
    minv = torch.from_numpy(np.linalg.inv(M)[None]).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up (validates the call and makes its plan) on a side stream, as torch's capture recipe does
        W.warp_perspective(t, None, (dw, dh), out=out, M_inv_device=minv, border_mode=W.BORDER_REPLICATE)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    out.fill_(77)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        W.warp_perspective(t, None, (dw, dh), out=out, M_inv_device=minv, border_mode=W.BORDER_REPLICATE)
    g.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), ref(src, minv[0].cpu().numpy(), (dw, dh), LINEAR, BR.REPLICATE, m_is_inverse=True))
