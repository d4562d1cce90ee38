"""The NV12 warp on the GPU (bev_amd.warp.warp_perspective_nv12 -> bevwarp_warp_nv12, FramePipeline(src_format="nv12"), cv2_compat.cvtColor):
every result is compared with tests/nv12_ref.py -- the oracle's warp of the converted frame -- on every pixel, bit for bit.
Run on the GPU box:  python -m pytest tests -m gpu -q"""
import functools

import numpy as np
import pytest
import torch

from tests import nv12_ref as R
from tests import pixels as PX
from tests import workloads as wl

pytestmark = pytest.mark.gpu

LINEAR, NEAREST, INVERSE = 1, 0, 16
BORDER = (10, 200, 77)


@pytest.fixture(scope="module")
def W():
    from bev_amd import warp
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return warp


def padded_planes(y, uv, y_offset=3, uv_offset=2):
    """Both planes inside larger allocations of their own whose every other byte is 0xA5 (PX.padded_source: guard rows above and below,
    64 bytes and more beside every row).  The pairs stay 2-byte aligned (an even offset)."""
    ty = PX.padded_source(y[..., None], PX.U8_FILL, offset=y_offset)[..., 0]
    tuv = PX.padded_source(uv, PX.U8_FILL, offset=uv_offset)
    assert tuv.data_ptr() % 2 == 0 and ty.stride(-1) == 1 and tuv.stride(-1) == 1 and tuv.stride(-2) == 2
    return ty, tuv


def planes(W, y, uv, layout):
    """The frame(s) on the device: "two" allocations, a "single" buffer split with split_nv12, "padded" (see padded_planes) or "rowpad":
    row strides of W + 7 (Y) and W + 6 (UV) bytes with 0xA5 between the rows."""
    if layout == "two":
        return torch.from_numpy(np.array(y)).cuda(), torch.from_numpy(np.array(uv)).cuda()  # (copies: the shared frames are read-only)
    if layout == "single":
        joined = np.stack([R.join(a, b) for a, b in zip(y, uv)]) if y.ndim == 3 else R.join(y, uv)
        ty, tuv = W.split_nv12(torch.from_numpy(joined).cuda())
        assert tuv.data_ptr() == ty.data_ptr() + y.shape[-2] * y.shape[-1]
        return ty, tuv
    if layout == "padded":
        return padded_planes(y, uv)
    assert layout == "rowpad" and y.ndim == 2
    h, w = y.shape
    by = torch.full((h * (w + 7),), PX.U8_FILL, dtype=torch.uint8, device="cuda")
    buv = torch.full((h // 2 * (w + 6),), PX.U8_FILL, dtype=torch.uint8, device="cuda")
    ty, tuv = torch.as_strided(by, (h, w), (w + 7, 1)), torch.as_strided(buv, (h // 2, w // 2, 2), (w + 6, 2, 1))
    ty.copy_(torch.from_numpy(y).cuda())
    tuv.copy_(torch.from_numpy(uv).cuda())
    return ty, tuv


def gpu(W, y, uv, M, dsize, interp, border=None, rgb=False, layout="two", out=None):
    ty, tuv = planes(W, y, uv, layout)
    if out is None:
        shape = ((y.shape[0],) if y.ndim == 3 else ()) + (int(dsize[1]), int(dsize[0]), 3)
        out = torch.full(shape, 33, dtype=torch.uint8, device="cuda")  # (pixels a launch leaves unwritten do not pass as zeros)
    got = W.warp_perspective_nv12(ty, tuv, M, dsize, flags=interp, border_value=border, out=out, rgb=rgb)
    torch.cuda.synchronize()
    assert got is out
    return got.cpu().numpy()


def check(W, y, uv, M, dsize, interp, border=None, rgb=False, layout="two", what=""):
    got = gpu(W, y, uv, M, dsize, interp, border, rgb, layout)
    exp = R.warp_nv12(y, uv, M, dsize, interp & 7, border_value=border, rgb=rgb, m_is_inverse=bool(interp & INVERSE))
    np.testing.assert_array_equal(got, exp, err_msg="%s interp %d rgb %d layout %s src %s dsize %s" % (what, interp, rgb, layout, y.shape, dsize))
    return exp


# ---- 1. the conversion alone: identity, nearest ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def domain_expected(rgb):
    y, uv = R.frame("domain", 0, 0, 0)
    exp = R.warp_nv12(y, uv, np.eye(3), (4096, 4096), NEAREST, rgb=rgb, nthreads=8)
    exp.setflags(write=False)
    return exp


@pytest.mark.parametrize("rgb", [False, True], ids=["bgr", "rgb"])
def test_every_yuv_value_converts_like_the_reference(W, rgb):
    y, uv = R.frame("domain", 0, 0, 0)
    got = gpu(W, y, uv, np.eye(3), (4096, 4096), NEAREST, rgb=rgb)
    exp = domain_expected(rgb)
    assert got.shape == exp.shape == (4096, 4096, 3)
    if not np.array_equal(got, exp):
        np.testing.assert_array_equal(got, exp)
    assert exp.min() == 0 and exp.max() == 255


@pytest.mark.parametrize("rgb", [False, True], ids=["bgr", "rgb"])
def test_identity_of_small_sources(W, rgb):
    for w, h in ((2, 2), (4, 2), (66, 34)):
        for kind in ("uniform", "video"):
            y, uv = R.frame(kind, w + h, h, w)
            exp = check(W, y, uv, np.eye(3), (w, h), NEAREST, rgb=rgb, what="identity")
            np.testing.assert_array_equal(exp, R.nv12_to_bgr(y, uv, rgb))  # (the reference's identity warp is the converted frame)
            check(W, y, uv, np.eye(3), (w, h), LINEAR, rgb=rgb, what="identity")
    b = R.nv12_to_bgr(*R.frame("video", 66 + 34, 34, 66))
    assert 16 <= b.min() and b.max() <= 231  # the unsaturated arithmetic is what "video" compares


# ---- 2. chroma phase -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", [NEAREST, LINEAR], ids=["nearest", "linear"])
def test_chroma_phase(W, interp):
    """Translations by (j + k / 32, i + l / 32): the tap origin has every parity in both axes, so a pixel's four taps share one, two or
    four (U, V) pairs; the chroma of the frame changes at every pair."""
    y, uv = R.frame("phase", 2, 18, 34)
    for i in (0, 1):
        for j in (0, 1):
            for k, l in ((0, 0), (5, 27), (31, 1)):
                M_inv = np.array([[1, 0, j + k / 32.0], [0, 1, i + l / 32.0], [0, 0, 1.0]])
                check(W, y, uv, M_inv, (32, 16), interp | INVERSE, what="phase %d %d %d %d" % (i, j, k, l))
                check(W, y, uv, M_inv, (32, 16), interp | INVERSE, rgb=True, layout="single", what="phase %d %d %d %d" % (i, j, k, l))


# ---- 3. edges ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rgb", [False, True], ids=["bgr", "rgb"])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR], ids=["nearest", "linear"])
def test_edges_with_a_border_value_inside_padded_allocations(W, interp, rgb):
    """Translations that put the tap pairs on (-1, 0) and on (w - 1, w) in x and in y -- the odd last column with its right tap outside --
    and a ring of pixels whose taps are all outside.  Both planes lie in allocations filled with 0xA5 around every row."""
    w, h = 34, 18
    y, uv = R.frame("phase", 5, h, w)
    for tx, ty in ((-1.0, -1.0), (-1 + 5 / 32.0, -1 + 27 / 32.0), (-2 + 31 / 32.0, -2 + 1 / 32.0), (-1 + 16 / 32.0, 0.0), (0.0, -1 + 16 / 32.0)):
        M_inv = np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1.0]])
        exp = check(W, y, uv, M_inv, (w + 4, h + 4), interp | INVERSE, border=BORDER, rgb=rgb, layout="padded", what="edge %r" % ((tx, ty),))
        assert exp[h + 3, w + 3].tolist() == list(BORDER)  # all taps outside: the border value as given, in either order
    # the reference shows B and R swapped with the order where a pixel has no border tap, and the border value unswapped
    M_inv = np.array([[1, 0, -1 + 5 / 32.0], [0, 1, -1 + 27 / 32.0], [0, 0, 1.0]])
    a = R.warp_nv12(y, uv, M_inv, (w + 4, h + 4), interp, border_value=BORDER, rgb=False, m_is_inverse=True)
    b = R.warp_nv12(y, uv, M_inv, (w + 4, h + 4), interp, border_value=BORDER, rgb=True, m_is_inverse=True)
    np.testing.assert_array_equal(a[2:h - 1, 2:w - 1], b[2:h - 1, 2:w - 1, ::-1])
    assert a[h + 3, w + 3].tolist() == b[h + 3, w + 3].tolist() == list(BORDER) and not np.array_equal(a, b[..., ::-1])


# ---- 4. geometries -------------------------------------------------------------------------------------------------------------------------
SW, SH = 130, 66
GEOMS = {"keystone": wl.keystone_H(SW, SH, 257, 5), "brno": wl.synth_brno_H(SW, SH, 257, 5), "rotated": wl.rotated_H(SW, SH, 257, 5, 30.0)}


@pytest.mark.parametrize("geom", sorted(GEOMS))
@pytest.mark.parametrize("interp", [NEAREST, LINEAR], ids=["nearest", "linear"])
def test_geometries_and_destination_sizes(W, geom, interp):
    """Destination widths around the 256-pixel wave segment and heights around the 4-row workgroup: one lane, ragged last lanes and
    last workgroups, more than one tile in both directions."""
    M = GEOMS[geom]
    cut = []
    for kind in ("video", "uniform"):
        y, uv = R.frame(kind, 11, SH, SW)
        for dw in (1, 255, 256, 257):
            for dh in (1, 4, 5):
                exp = check(W, y, uv, M, (dw, dh), interp, border=BORDER, what=geom + " " + kind)
                if dw >= 255 and dh >= 4:  # (every matrix is built for 257 x 5: row 0 and column 0 alone lie wholly outside the frame, a fraction of them says nothing)
                    cut.append(float((exp == np.array(BORDER, np.uint8)).all(-1).mean()))
    if geom == "brno":  # the frame's edge really crosses these destinations
        assert all(0.10 <= f <= 0.90 for f in cut), cut


# ---- 5. layouts ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", [NEAREST, LINEAR], ids=["nearest", "linear"])
def test_layouts(W, interp):
    M = wl.keystone_H(SW, SH, 120, 37)
    y, uv = R.frame("uniform", 21, SH, SW)
    exp = check(W, y, uv, M, (120, 37), interp, layout="two")
    for layout in ("single", "rowpad", "padded"):
        np.testing.assert_array_equal(gpu(W, y, uv, M, (120, 37), interp, layout=layout), exp, err_msg=layout)
    # a batch: one shared matrix, and a matrix per frame; as two allocations and as single buffers
    frames = [R.frame("uniform", 30 + i, SH, SW) for i in range(3)]
    ys, uvs = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    Ms = np.stack([wl.jitter_H(M, i) for i in range(3)])
    for mats in (M, Ms):
        want = np.stack([R.warp_nv12(ys[i], uvs[i], mats if mats.ndim == 2 else mats[i], (120, 37), interp) for i in range(3)])
        for layout in ("two", "single"):
            np.testing.assert_array_equal(gpu(W, ys, uvs, mats, (120, 37), interp, layout=layout), want, err_msg="batch %s %s" % (layout, mats.shape))
    assert not np.array_equal(R.warp_nv12(ys[1], uvs[1], Ms[1], (120, 37), interp), R.warp_nv12(ys[1], uvs[1], M, (120, 37), interp))


@pytest.mark.parametrize("interp", [NEAREST, LINEAR], ids=["nearest", "linear"])
def test_two_frames_two_matrices_every_stride_padded(W, interp):
    """What an entry point's argument filling can get wrong -- a swapped or dropped stride or pointer -- in the smallest shape that shows
    it: two frames with a matrix each, row and frame strides of every image that all differ from the tight ones and from each other, a
    destination of two tile columns (260 > 256) and two tile rows (6 > 4)."""
    sw, sh, dw, dh = 12, 10, 260, 6
    frames = [R.frame("uniform", 70 + i, sh, sw) for i in range(2)]
    ys, uvs = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    H = wl.keystone_H(sw, sh, dw, dh)
    Ms = np.stack([wl.jitter_H(H, 1), wl.jitter_H(H, 2)])
    ty, tuv = PX.strided(ys, (9, 5)), PX.strided(uvs, (10, 6))   # (the pairs' strides stay even)
    out = PX.strided(np.full((2, dh, dw, 3), 33, np.uint8), (20, 7))
    strides = [ty.stride(0), ty.stride(1), tuv.stride(0), tuv.stride(1), out.stride(0), out.stride(1)]
    assert len(set(strides + [sh * sw, sw, sh // 2 * sw, dh * dw * 3, dw * 3])) == 11
    assert W.warp_perspective_nv12(ty, tuv, Ms, (dw, dh), flags=interp, out=out) is out
    torch.cuda.synchronize()
    exp = [R.warp_nv12(ys[i], uvs[i], Ms[i], (dw, dh), interp) for i in range(2)]
    np.testing.assert_array_equal(out.cpu().numpy(), np.stack(exp))
    assert not np.array_equal(exp[0], R.warp_nv12(ys[0], uvs[0], Ms[1], (dw, dh), interp))  # (the two matrices give different frames)


@pytest.mark.parametrize("align", [16, 0], ids=["wide_stores", "pixel_stores"])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR], ids=["nearest", "linear"])
def test_destination_layouts_keep_their_canaries(W, interp, align):
    M = wl.synth_brno_H(SW, SH, 257, 9)
    frames = [R.frame("uniform", 40 + i, SH, SW) for i in range(2)]
    ys, uvs = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    for dw, dh in ((257, 9), (254, 5), (3, 2)):
        view, holder = PX.canaried_out((2, dh, dw, 3), torch.uint8, pad=5, align=align)
        got = gpu(W, ys, uvs, M, (dw, dh), interp, border=BORDER, out=view)
        want = np.stack([R.warp_nv12(ys[i], uvs[i], M, (dw, dh), interp, border_value=BORDER) for i in range(2)])
        np.testing.assert_array_equal(got, want, err_msg="align %d %dx%d" % (align, dw, dh))
        PX.assert_canaries_intact(holder, view, "nv12 align %d %dx%d" % (align, dw, dh))


# ---- 6. the pipeline -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("download", [True, False], ids=["download", "resident"])
def test_frame_pipeline_takes_nv12_slots(download):
    from bev_amd.pipeline import FramePipeline
    sw, sh, dw, dh = 64, 48, 40, 24
    M = wl.keystone_H(sw, sh, dw, dh)
    frames = [R.frame("uniform" if i % 2 else "video", 50 + i, sh, sw) for i in range(5)]
    with FramePipeline((sh, sw), 3, M, (dw, dh), src_format="nv12", download=download) as pipe:
        assert tuple(pipe.h_in[0].shape) == (sh * 3 // 2, sw) and pipe.h_in[0].dtype == torch.uint8 and pipe.h_in[0].is_pinned()
        assert tuple(pipe.d_in[0].shape) == (sh * 3 // 2, sw) and pipe._in_bytes == sh * sw * 3 // 2  # half of a BGR frame's upload
        assert pipe.next_input().shape == (sh * 3 // 2, sw)
        outs = []
        for res in pipe.run(R.join(y, uv) for y, uv in frames):
            outs.append(np.array(res.cpu().numpy() if isinstance(res, torch.Tensor) else res))
    assert len(outs) == 5
    for (y, uv), got in zip(frames, outs):
        np.testing.assert_array_equal(got, R.warp_nv12(y, uv, M, (dw, dh), LINEAR))


# ---- 7. cv2_compat.cvtColor ----------------------------------------------------------------------------------------------------------------
def test_cvtcolor_nv12():
    from bev_amd import cv2_compat as cv2
    y, uv = R.frame("uniform", 60, 34, 66)
    nv12 = R.join(y, uv)
    bgr = cv2.cvtColor(nv12, cv2.COLOR_YUV2BGR_NV12)
    rgb = cv2.cvtColor(nv12, cv2.COLOR_YUV2RGB_NV12)
    assert bgr.shape == rgb.shape == (34, 66, 3) and bgr.dtype == np.uint8
    np.testing.assert_array_equal(bgr, R.nv12_to_bgr(y, uv))
    np.testing.assert_array_equal(rgb, R.nv12_to_bgr(y, uv, rgb=True))
    np.testing.assert_array_equal(bgr, R.warp_nv12(y, uv, np.eye(3), (66, 34), NEAREST))
