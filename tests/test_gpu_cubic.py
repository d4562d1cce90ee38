"""The bicubic warp on the GPU (bev_amd.warp.warp_perspective(flags=INTER_CUBIC) -> bevwarp_warp_border -> warp_cubic_kernel), every
result compared with the numpy reference tests/cubic_ref.py bit for bit over all pixels.  Destinations are pre-filled with 77, so a
pixel a launch leaves unwritten does not pass as zero.  Run on the GPU box:  python -m pytest tests -m gpu -q"""
import ctypes

import numpy as np
import pytest
import torch

from tests import border_ref as BR
from tests import cubic_ref as CR
from tests import pixels as px
from tests import workloads as wl

pytestmark = pytest.mark.gpu

CUBIC, INVERSE = 2, 16
MODES = BR.MODES  # all six


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


def gpu(W, src, M, dsize, mode, flags=CUBIC, canvas=77, **kw):
    t = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    out = torch.full(_dst_shape(src, dsize), canvas, dtype=t.dtype, device=t.device)
    got = W.warp_perspective(t, M, dsize, flags=flags, out=out, border_mode=mode, **kw)
    torch.cuda.synchronize()
    assert got is out
    return got.cpu().numpy()


def ref(src, M, dsize, mode, m_is_inverse=False, border_value=0.0, canvas=77):
    cv = np.full(_dst_shape(src, dsize), canvas, dtype=src.dtype)
    return CR.warp(src, M, dsize, mode, m_is_inverse=m_is_inverse, border_value=border_value, canvas=cv)


def check(W, src, M, dsize, mode, m_is_inverse=False, border_value=None):
    got = gpu(W, src, M, dsize, mode, flags=CUBIC | (INVERSE if m_is_inverse else 0), border_value=border_value)
    exp = ref(src, M, dsize, mode, m_is_inverse, 0.0 if border_value is None else border_value)
    np.testing.assert_array_equal(got, exp, err_msg="%s %s %s" % (BR.NAMES[mode], src.dtype, src.shape))
    if mode == BR.TRANSPARENT:  # the canvas keeps 77 exactly where the reference writes nothing
        keep = ~CR.written_mask(src.shape[:2], M, dsize, m_is_inverse)
        assert (got[keep] == 77).all()


GEOMS = {  # (src w, h, dst w, h, forward matrix): the two geometries of tests/test_gpu_border.py
    "rotated_zoom_out": (160, 96, 120, 100, wl.rotated_H(160, 96, 120, 100, 30.0, zoom=2.5)),
    "brno": (640, 360, 160, 120, wl.synth_brno_H(640, 360, 160, 120)),
}


@pytest.mark.parametrize("geom", sorted(GEOMS))
def test_geometries_hold_every_pixel_class(geom):
    """Inliers, partial windows, windows wholly outside, TRANSPARENT's written non-inliers and all 1024 (fy, fx) pairs: asserted from the
    reference, so that a later change of geometry cannot empty a class."""
    sw, sh, dw, dh, M = GEOMS[geom]
    inl, partial, all_out, written = CR.classes((sh, sw), M, (dw, dh))
    counts = (int(inl.sum()), int(partial.sum()), int(all_out.sum()), int((written & ~inl).sum()))
    assert all(n > 0 for n in counts), counts
    assert counts == {"rotated_zoom_out": (2336, 244, 9420, 120), "brno": (9624, 529, 9047, 187)}[geom]
    _, _, fx, fy = CR.window((dw, dh), CR.invert3x3(M))
    assert len(set((fy * 32 + fx).ravel().tolist())) == 1024


@pytest.mark.parametrize("geom", sorted(GEOMS))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_mode_matrix(W, geom, mode, dtype):
    sw, sh, dw, dh, M = GEOMS[geom]
    for c in (1, 2, 3, 4):
        check(W, _src((sh, sw, c), dtype, seed=c), M, (dw, dh), mode)
    check(W, _src((sh, sw), dtype, seed=9), M, (dw, dh), mode)  # (H, W) image


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_constant_with_a_border_value(W, dtype):
    sw, sh, dw, dh, M = GEOMS["rotated_zoom_out"]
    bv = (7.0, 200.0, 31.5, 99.0) if dtype == np.uint8 else (0.3, -2.5, 7.0, 0.125)
    for c in (1, 3, 4):
        check(W, _src((sh, sw, c), dtype, seed=20 + c), M, (dw, dh), BR.CONSTANT, border_value=bv[:c])


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_bevwarp_warp_takes_cubic_directly(W, dtype):
    """bevwarp_warp(interp = 2) through ctypes: bicubic with the constant border."""
    from bev_amd import _lib
    sw, sh, dw, dh, M = GEOMS["brno"]
    src = _src((sh, sw, 3), dtype, seed=23)
    bv = np.array([12.0, 130.0, 250.0])
    t = torch.from_numpy(src).cuda()
    out = torch.full((dh, dw, 3), 77, dtype=t.dtype, device="cuda")
    minv = torch.from_numpy(np.ascontiguousarray(CR.invert3x3(M))).cuda()
    esz = t.element_size()
    st = _lib.load().bevwarp_warp(t.data_ptr(), out.data_ptr(), 1, sh, sw, dh, dw, 3, sh * sw * 3 * esz, sw * 3 * esz, dh * dw * 3 * esz, dw * 3 * esz,
                                  minv.data_ptr(), 1, _lib.U8 if dtype == np.uint8 else _lib.F32, CUBIC, bv.ctypes.data_as(ctypes.c_void_p),
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), ref(src, M, (dw, dh), BR.CONSTANT, border_value=bv))


SMALL = ((1, 9), (9, 1), (1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (4, 7))  # (h, w) around the inlier threshold w - 3
SMALL_MINV = np.array([[0.37, -0.21, -3.0], [0.18, 0.41, -2.5], [0.0005, 0.0, 1.0]])


def test_small_sources_inlier_counts():
    """Sides <= 3 have no inlier at all, 4 x 4 has 5 and 5 x 5 has 21."""
    n = {hw: int(CR.classes(hw, SMALL_MINV, (29, 21), m_is_inverse=True)[0].sum()) for hw in SMALL}
    assert all(n[hw] == 0 for hw in SMALL if min(hw) <= 3) and n[(4, 4)] == 5 and n[(5, 5)] == 21 and n[(4, 7)] > 0, n


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_small_sources(W, dtype):
    """A side of 1 makes REFLECT_101's period degenerate; sides up to 3 run the general path alone."""
    for sh, sw in SMALL:
        for mode in MODES:
            check(W, _src((sh, sw, 3), dtype, seed=sh * 10 + sw), SMALL_MINV, (29, 21), mode, m_is_inverse=True)


def test_coordinates_beyond_int16(W):
    """The maps saturate to int16 BEFORE the window is laid out and remapped: tap indices reach 32769 and -32769."""
    src = _src((23, 37, 3), np.uint8, seed=7)
    lo, hi = 0, 0
    for Minv in (np.array([[3.0, 0.5, 40000.0], [-0.25, 2.0, -50000.0], [0, 0, 1.0]]),
                 np.array([[900.0, 0.0, -20000.0], [0.0, -700.0, 9000.0], [0, 0, 1.0]])):  # crosses +-32768 inside the destination
        sx, sy, _, _ = CR.window((64, 20), Minv)
        lo, hi = min(lo, int(sx.min()), int(sy.min())), max(hi, int(sx.max()) + 3, int(sy.max()) + 3)
        for mode in MODES:
            check(W, src, Minv, (64, 20), mode, m_is_inverse=True)
            check(W, src.astype(np.float32) / 255, Minv, (64, 20), mode, m_is_inverse=True)
    assert (lo, hi) == (-32769, 32769)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("per_frame", [False, True])
def test_batch(W, dtype, per_frame):
    B, sw, sh, dw, dh = 3, 64, 48, 50, 40
    H = wl.rotated_H(sw, sh, dw, dh, 20.0, zoom=1.6)
    Ms = np.stack([wl.jitter_H(H, i, px=4.0) for i in range(B)]) if per_frame else H
    src = _src((B, sh, sw, 3), dtype, seed=30)
    for mode in (BR.CONSTANT, BR.REFLECT, BR.TRANSPARENT):
        out = torch.full((B, dh, dw, 3), 77, dtype=torch.from_numpy(src).dtype, device="cuda")
        W.warp_perspective(torch.from_numpy(src).cuda(), Ms, (dw, dh), flags=CUBIC, out=out, border_mode=mode)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for i in range(B):
            np.testing.assert_array_equal(got[i], ref(src[i], Ms[i] if per_frame else Ms, (dw, dh), mode), err_msg="%s frame %d" % (BR.NAMES[mode], i))


def test_two_frames_two_matrices_every_stride_padded(W):
    """What an entry point's argument filling can get wrong -- a swapped or dropped stride or pointer -- in the smallest shape that shows
    it: two frames with a matrix each, row and frame strides of source and destination that all differ from the tight ones and from each
    other, a destination of two tile columns (260 > 256) and two tile rows (6 > 4)."""
    sw, sh, dw, dh = 12, 10, 260, 6
    host = _src((2, sh, sw, 3), np.uint8, seed=31)
    H = wl.keystone_H(sw, sh, dw, dh)
    Ms = np.stack([wl.jitter_H(H, 1), wl.jitter_H(H, 2)])
    src, out = px.strided(host, (40, 5)), px.strided(np.full((2, dh, dw, 3), 77, np.uint8), (20, 7))
    assert len({src.stride(0), src.stride(1), out.stride(0), out.stride(1), sh * sw * 3, sw * 3, dh * dw * 3, dw * 3}) == 8
    W.warp_perspective(src, Ms, (dw, dh), flags=CUBIC, out=out, border_mode=BR.REFLECT)
    torch.cuda.synchronize()
    exp = [ref(host[i], Ms[i], (dw, dh), BR.REFLECT) for i in range(2)]
    np.testing.assert_array_equal(out.cpu().numpy(), np.stack(exp))
    assert not np.array_equal(exp[0], ref(host[0], Ms[1], (dw, dh), BR.REFLECT))  # (the two matrices give different frames)


def _source_at_the_end_of_its_allocation(frame, row_pad, lead):
    """A CUDA view of `frame` (H, W, C) with padded rows whose last element is the last element of its allocation, based `lead`
    elements into it; every other element holds a fill value that is no pixel of the frame's."""
    h, w, c = frame.shape
    rs = w * c + row_pad
    n = lead + (h - 1) * rs + w * c
    t = torch.from_numpy(frame)
    buf = torch.full((n,), px.U8_FILL if frame.dtype == np.uint8 else -7.5, dtype=t.dtype, device="cuda")
    view = torch.as_strided(buf, (h, w, c), (rs, c, 1), lead)
    view.copy_(t.cuda())
    assert view.data_ptr() + ((h - 1) * rs + w * c) * t.element_size() == buf.data_ptr() + n * t.element_size()
    return view


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_layouts(W, dtype, c):
    """Views with padded row strides whose bases are 0, 1, 2 and 3 elements off a 16-byte boundary: a destination that admits the wide
    stores and one that does not (canaries around both stay intact), a source whose tap windows start at every alignment, and a source
    that ends with its allocation (a window never reaches past the bytes of its own taps)."""
    sw, sh, dw, dh = 61, 40, 70, 33
    M = wl.rotated_H(sw, sh, dw, dh, 15.0, zoom=1.4)
    frame = _src((sh, sw, c), dtype, seed=40 + c)
    tdt = torch.from_numpy(frame).dtype
    for off in (0, 1, 2, 3):
        for mode in (BR.CONSTANT, BR.REPLICATE, BR.WRAP, BR.TRANSPARENT):
            exp = ref(frame, M, (dw, dh), mode)
            srcs = [px.padded_source(frame, px.U8_FILL if dtype == np.uint8 else -7.5, offset=off),
                    _source_at_the_end_of_its_allocation(frame, row_pad=off + 1, lead=4 + off)]
            for si, s in enumerate(srcs):
                for align in (16, 0):
                    view, holder = px.canaried_out((dh, dw, c), tdt, pad=24, align=align)
                    W.warp_perspective(s, M, (dw, dh), flags=CUBIC, out=view, border_mode=mode)
                    torch.cuda.synchronize()
                    what = "%s off %d source %d align %d" % (BR.NAMES[mode], off, si, align)
                    np.testing.assert_array_equal(view.cpu().numpy(), exp, err_msg=what)
                    px.assert_canaries_intact(holder, view, what)


def test_transparent_two_sources_one_canvas(W):
    dw, dh = 200, 120
    cams = [_src((90, 160, 3), np.uint8, seed=13), _src((100, 140, 3), np.uint8, seed=14)]
    Hs = [np.array([[0.9, 0.1, 5.0], [-0.05, 1.0, 10.0], [0, 0, 1.0]]), np.array([[1.1, -0.1, 70.0], [0.08, 0.95, 20.0], [0.0002, 0, 1.0]])]
    canvas = torch.full((dh, dw, 3), 77, dtype=torch.uint8, device="cuda")
    exp = np.full((dh, dw, 3), 77, np.uint8)
    covered = np.zeros((dh, dw), bool)
    for cam, H in zip(cams, Hs):
        W.warp_perspective(torch.from_numpy(cam).cuda(), H, (dw, dh), flags=CUBIC, out=canvas, border_mode=W.BORDER_TRANSPARENT)
        exp = CR.warp(cam, H, (dw, dh), BR.TRANSPARENT, canvas=exp)
        covered |= CR.written_mask(cam.shape[:2], H, (dw, dh))
    torch.cuda.synchronize()
    got = canvas.cpu().numpy()
    np.testing.assert_array_equal(got, exp)
    assert (got[~covered] == 77).all() and covered.any() and (~covered).any()


@pytest.mark.parametrize("kind", px.KINDS)
def test_float32_specials(W, kind):
    """+-inf, NaN, -0.0, subnormals and values next to FLT_MAX: NaN where the reference has NaN, every other pixel equal by bits (NaN
    signs and payloads are not pinned: the reference is numpy on the host)."""
    sw, sh, dw, dh, M = GEOMS["rotated_zoom_out"]
    for c, mode in ((1, BR.CONSTANT), (3, BR.REPLICATE), (4, BR.REFLECT_101), (2, BR.TRANSPARENT)):
        src = px.float_frame(kind, 50 + c, sh, sw, c)
        bv = px.BORDER[:c] if mode == BR.CONSTANT else None
        got = gpu(W, src, M, (dw, dh), mode, border_value=bv)
        px.same_float(got, ref(src, M, (dw, dh), mode, border_value=0.0 if bv is None else bv))


def test_graph_capture_and_plan_cache(W):
    """A steady-state call (out= and M_inv_device=) is served from the plan cache with the same bits, and one torch.cuda.graph capture
    of it replays."""
    sw, sh, dw, dh, M = GEOMS["brno"]
    src = _src((sh, sw, 3), np.uint8, seed=18)
    t = torch.from_numpy(src).cuda()
    out = torch.full((dh, dw, 3), 77, dtype=torch.uint8, device="cuda")
    minv = torch.from_numpy(np.linalg.inv(M)[None]).cuda()
    exp = ref(src, minv[0].cpu().numpy(), (dw, dh), BR.REFLECT, m_is_inverse=True)

    def call():
        return W.warp_perspective(t, None, (dw, dh), flags=CUBIC, out=out, M_inv_device=minv, border_mode=W.BORDER_REFLECT)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # the first call validates and makes the plan (on a side stream, as torch's capture recipe does)
        call()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), exp)
    key = [k for k in W._plans if k[0] == t.data_ptr() and k[1] == out.data_ptr() and k[-2] == CUBIC]
    assert len(key) == 1 and W._plans[key[0]][3] is None  # a plan without a verdict table
    plans = len(W._plans)
    out.fill_(77)
    call()  # the steady state
    torch.cuda.synchronize()
    assert len(W._plans) == plans
    np.testing.assert_array_equal(out.cpu().numpy(), exp)
    out.fill_(77)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    g.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), exp)


def test_cv2_compat_numpy_in_out(W):
    from bev_amd import cv2_compat as cv2
    sw, sh, dw, dh, M = GEOMS["rotated_zoom_out"]
    src = _src((sh, sw, 3), np.uint8, seed=17)
    for mode in (cv2.BORDER_CONSTANT, cv2.BORDER_REPLICATE, cv2.BORDER_REFLECT, cv2.BORDER_WRAP, cv2.BORDER_REFLECT_101, cv2.BORDER_TRANSPARENT):
        got = cv2.warpPerspective(src, M, (dw, dh), flags=cv2.INTER_CUBIC, borderMode=mode, borderValue=(1, 2, 3))
        np.testing.assert_array_equal(got, CR.warp(src, M, (dw, dh), mode, border_value=(1, 2, 3)), err_msg=BR.NAMES[mode])
    canvas = np.full((dh, dw, 3), 55, np.uint8)
    exp = CR.warp(src, M, (dw, dh), BR.TRANSPARENT, canvas=canvas)
    assert cv2.warpPerspective(src, M, (dw, dh), canvas, cv2.INTER_CUBIC, cv2.BORDER_TRANSPARENT) is canvas
    np.testing.assert_array_equal(canvas, exp)
