"""The warps into NV12 on the GPU (bev_amd.warp.warp_perspective_to_nv12 -> bevwarp_warp_to_nv12, warp_nv12_to_nv12 ->
bevwarp_warp_nv12_to_nv12, FramePipeline(dst_format="nv12")): every result is compared with tests/nv12_out_ref.py -- BGR -> NV12 of the
oracle's warp -- on every byte of both planes, bit for bit.
Run on the GPU box:  python -m pytest tests -m gpu -q"""
import functools

import numpy as np
import pytest
import torch

from oracle import cpu_oracle
from tests import nv12_out_ref as R
from tests import nv12_ref as RI
from tests import pixels as PX
from tests import test_gpu_nv12 as N12   # (its source layouts: padded_planes, planes)
from tests import workloads as wl

pytestmark = pytest.mark.gpu

LINEAR, NEAREST, INVERSE = 1, 0, 16
BORDER = (10, 200, 77)
BORDER_YUV = (138, 63, 87)  # of BORDER read as B, G, R


@pytest.fixture(scope="module")
def W():
    from bev_amd import warp
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return warp


def fresh_out(batch, dh, dw):
    """A joined destination whose every byte a launch must overwrite (unwritten bytes do not pass as zeros)."""
    return torch.full(((batch,) if batch else ()) + (dh * 3 // 2, dw), 33, dtype=torch.uint8, device="cuda")


def host(W, out):
    """(y, uv) numpy arrays of a result: a joined buffer or a pair of planes."""
    torch.cuda.synchronize()
    y, uv = out if isinstance(out, (tuple, list)) else W.split_nv12(out)
    return y.cpu().numpy(), uv.cpu().numpy()


def gpu_bgr(W, src, M, dsize, interp, border=None, rgb=False, out=None, padded=False):
    t = PX.padded_source(src, PX.U8_FILL, offset=3) if padded else torch.from_numpy(np.array(src)).cuda()
    if out is None:
        out = fresh_out(src.shape[0] if src.ndim == 4 else 0, int(dsize[1]), int(dsize[0]))
    got = W.warp_perspective_to_nv12(t, M, dsize, flags=interp, border_value=border, out=out, rgb=rgb)
    assert got is out
    return host(W, got)


def gpu_nv12(W, y, uv, M, dsize, interp, border=None, out=None, layout="two"):
    ty, tuv = N12.planes(W, y, uv, layout)
    if out is None:
        out = fresh_out(y.shape[0] if y.ndim == 3 else 0, int(dsize[1]), int(dsize[0]))
    got = W.warp_nv12_to_nv12(ty, tuv, M, dsize, flags=interp, border_value=border, out=out)
    assert got is out
    return host(W, got)


def same(got, exp, what):
    for g, e, plane in zip(got, exp, ("Y", "UV")):
        assert g.shape == e.shape and g.dtype == e.dtype == np.uint8, (what, plane, g.shape, e.shape)
        np.testing.assert_array_equal(g, e, err_msg="%s plane %s" % (what, plane))


def check_bgr(W, src, M, dsize, interp, border=None, rgb=False, padded=False, what=""):
    exp = R.warp_to_nv12(src, M, dsize, interp & 7, border_value=border, rgb=rgb, m_is_inverse=bool(interp & INVERSE))
    same(gpu_bgr(W, src, M, dsize, interp, border, rgb, padded=padded), exp, "bgr source %s interp %d rgb %d src %s dsize %s" % (what, interp, rgb, src.shape, dsize))
    return exp


def check_nv12(W, y, uv, M, dsize, interp, border=None, layout="two", what=""):
    exp = R.warp_nv12_to_nv12(y, uv, M, dsize, interp & 7, border_value=border, m_is_inverse=bool(interp & INVERSE))
    same(gpu_nv12(W, y, uv, M, dsize, interp, border, layout=layout), exp, "nv12 source %s interp %d layout %s src %s dsize %s" % (what, interp, layout, y.shape, dsize))
    return exp


# ---- 1. the conversion over the whole domain: nearest, integer translations --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def domain_frame():
    """4096 x 4096 B, G, R pixels: every value exactly once (pixel i holds B = i & 255, G = (i >> 8) & 255, R = i >> 16)."""
    i = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    img = np.stack([i & 255, (i >> 8) & 255, i >> 16], axis=-1).astype(np.uint8)
    img.setflags(write=False)
    return img


def shift(dx, dy):
    return np.array([[1, 0, dx], [0, 1, dy], [0, 0, 1.0]])  # dst -> src: destination (x, y) takes source (x + dx, y + dy)


@functools.lru_cache(maxsize=None)
def domain_expected(dx, dy, rgb):
    exp = R.warp_to_nv12(domain_frame(), shift(dx, dy), (4096, 4096), NEAREST, rgb=rgb, m_is_inverse=True, nthreads=8)
    for a in exp:
        a.setflags(write=False)
    return exp


def test_the_four_shifts_put_every_value_on_an_even_position_once():
    seen = np.zeros((4096, 4096), np.int32)  # source pixels that give a (U, V) pair, over the four runs
    for dx in (0, 1):
        for dy in (0, 1):
            seen[dy::2, dx::2] += 1  # destination (2 j, 2 i) takes source (2 j + dx, 2 i + dy), all of them inside the frame
    assert (seen == 1).all()
    assert (np.bincount((domain_frame().astype(np.uint32) << np.array([0, 8, 16], np.uint32)).sum(-1).ravel(), minlength=1 << 24) == 1).all()


@pytest.mark.parametrize("dx,dy,rgb", [(0, 0, False), (1, 0, False), (0, 1, False), (1, 1, False), (0, 0, True)], ids=["00-bgr", "10-bgr", "01-bgr", "11-bgr", "00-rgb"])
def test_every_pixel_value_converts_like_the_reference(W, dx, dy, rgb):
    """Every value passes the Y formula in each run, and the chroma formula in the one run that puts it on an even column of an even row."""
    got = gpu_bgr(W, domain_frame(), shift(dx, dy), (4096, 4096), NEAREST | INVERSE, rgb=rgb)
    exp = domain_expected(dx, dy, rgb)
    for g, e in zip(got, exp):
        assert g.shape == e.shape
        if not np.array_equal(g, e):
            np.testing.assert_array_equal(g, e)
    assert exp[0].min() == 16 and exp[0].max() == 235  # (black and white are in every run; a run's pairs come from a quarter of the values)


# ---- 2. the smallest frames --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", [NEAREST, LINEAR], ids=["nearest", "linear"])
def test_identity_of_small_sources(W, interp):
    for w, h in ((2, 2), (4, 2), (66, 34)):
        for kind in ("uniform", "video"):
            y, uv = RI.frame(kind, w + h, h, w)
            bgr = RI.nv12_to_bgr(y, uv)
            for rgb in (False, True):
                exp = check_bgr(W, bgr, np.eye(3), (w, h), interp, rgb=rgb, what="identity")
                same(exp, R.bgr_to_nv12(bgr, rgb), "the reference's identity warp is the converted frame")
            exp = check_nv12(W, y, uv, np.eye(3), (w, h), interp, what="identity")
            same(exp, R.bgr_to_nv12(bgr), "the reference's identity warp of NV12 is the frame converted there and back")
            check_nv12(W, y, uv, np.eye(3), (w, h), interp, layout="single", what="identity")


# ---- 3. geometries and destination sizes -----------------------------------------------------------------------------------------------
SW, SH = 130, 66
GEOMS = {"keystone": wl.keystone_H(SW, SH, 258, 6), "brno": wl.synth_brno_H(SW, SH, 258, 6), "rotated": wl.rotated_H(SW, SH, 258, 6, 30.0)}
WIDTHS, HEIGHTS = (2, 254, 256, 258), (2, 4, 6)


def border_share(bgr):
    """The share of pixels that are wholly border, on all pixels and on those at even columns of even rows."""
    is_border = (bgr == np.array(BORDER, np.uint8)).all(-1)
    return float(is_border.mean()), float(is_border[0::2, 0::2].mean())


@pytest.mark.parametrize("geom", sorted(GEOMS))
@pytest.mark.parametrize("interp", [NEAREST, LINEAR], ids=["nearest", "linear"])
def test_geometries_and_destination_sizes(W, geom, interp):
    """Destination widths around the 256-pixel wave segment and heights around the 4-row workgroup: one lane, a last lane of 2 pixels, a
    second tile column of one lane, and (height 6) a chroma row whose two luma rows lie in different workgroups."""
    M = GEOMS[geom]
    for kind in ("video", "uniform"):
        y, uv = RI.frame(kind, 11, SH, SW)
        bgr = RI.nv12_to_bgr(y, uv)
        for dw in WIDTHS:
            for dh in HEIGHTS:
                check_bgr(W, bgr, M, (dw, dh), interp, border=BORDER, rgb=kind == "video", what=geom + " " + kind)
                ey, euv = check_nv12(W, y, uv, M, (dw, dh), interp, border=BORDER, what=geom + " " + kind)
                if geom in ("brno", "rotated") and dw >= 254 and dh >= 4:  # the frame's edge really crosses these destinations, luma and chroma
                    shares = border_share(RI.warp_nv12(y, uv, M, (dw, dh), interp, border_value=BORDER))
                    assert all(0.10 <= s <= 0.90 for s in shares), (geom, kind, dw, dh, shares)
                if geom == "brno" and dh == 2:  # (this destination's only chroma row lies wholly outside the frame: fine, and said here)
                    assert (euv == np.array(BORDER_YUV[1:], np.uint8)).all()


# ---- 4. the border ring ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", [NEAREST, LINEAR], ids=["nearest", "linear"])
def test_edges_with_a_border_value_inside_padded_allocations(W, interp):
    """Translations that put the tap pairs on (-1, 0) and on (w - 1, w) in x and in y, and a ring of pixels whose taps are all outside.
    Every source lies in an allocation filled with 0xA5 around every row."""
    w, h = 34, 18
    y, uv = RI.frame("phase", 5, h, w)
    bgr = RI.nv12_to_bgr(y, uv)
    for tx, ty in ((-1.0, -1.0), (-1 + 5 / 32.0, -1 + 27 / 32.0), (-2 + 31 / 32.0, -2 + 1 / 32.0), (-1 + 16 / 32.0, 0.0), (0.0, -1 + 16 / 32.0)):
        M_inv = np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1.0]])
        for rgb in (False, True):
            ey, euv = check_bgr(W, bgr, M_inv, (w + 4, h + 4), interp | INVERSE, border=BORDER, rgb=rgb, padded=True, what="edge %r" % ((tx, ty),))
            # all taps outside: the border PIXEL converted, in the source's channel order
            want = tuple(int(v) for v in (R.yuv(*BORDER) if rgb else R.yuv(*BORDER[::-1])))
            assert int(ey[h + 3, w + 3]) == want[0] and euv[(h + 2) // 2, (w + 2) // 2].tolist() == list(want[1:])
            assert rgb or want == BORDER_YUV
        ey, euv = check_nv12(W, y, uv, M_inv, (w + 4, h + 4), interp | INVERSE, border=BORDER, layout="padded", what="edge %r" % ((tx, ty),))
        assert int(ey[h + 3, w + 3]) == BORDER_YUV[0] and euv[(h + 2) // 2, (w + 2) // 2].tolist() == list(BORDER_YUV[1:])
    # the default border is the black pixel, not zero bytes
    ey, euv = check_bgr(W, bgr, np.array([[1, 0, -1.0], [0, 1, -1.0], [0, 0, 1.0]]), (w + 4, h + 4), interp | INVERSE, padded=True, what="default border")
    assert int(ey[0, 0]) == 16 and euv[0, 0].tolist() == [128, 128]


# ---- 5. destination layouts --------------------------------------------------------------------------------------------------------------
def rowpad_planes(batch, dh, dw):
    """Planes with row strides of dw + 7 (Y) and dw + 6 (UV) bytes, 0xA5 between the rows: ((y, uv) views, (Y buffer, UV buffer))."""
    by = torch.full((batch * dh * (dw + 7),), PX.U8_FILL, dtype=torch.uint8, device="cuda")
    buv = torch.full((batch * (dh // 2) * (dw + 6),), PX.U8_FILL, dtype=torch.uint8, device="cuda")
    ty = torch.as_strided(by, (batch, dh, dw), (dh * (dw + 7), dw + 7, 1))
    tuv = torch.as_strided(buv, (batch, dh // 2, dw // 2, 2), ((dh // 2) * (dw + 6), dw + 6, 2, 1))
    return (ty, tuv), (by, buv)


@pytest.mark.parametrize("interp", [NEAREST, LINEAR], ids=["nearest", "linear"])
def test_layouts(W, interp):
    dw, dh = 120, 38
    M = wl.keystone_H(SW, SH, dw, dh)
    y, uv = RI.frame("uniform", 21, SH, SW)
    bgr = RI.nv12_to_bgr(y, uv)
    exp_b, exp_n = check_bgr(W, bgr, M, (dw, dh), interp), check_nv12(W, y, uv, M, (dw, dh), interp)   # one joined buffer
    # two allocations, and row-padded planes whose padding stays as it was
    for run, exp in ((lambda out: gpu_bgr(W, bgr[None], M, (dw, dh), interp, out=out), exp_b), (lambda out: gpu_nv12(W, y[None], uv[None], M, (dw, dh), interp, out=out), exp_n)):
        two = (torch.full((1, dh, dw), 33, dtype=torch.uint8, device="cuda"), torch.full((1, dh // 2, dw // 2, 2), 33, dtype=torch.uint8, device="cuda"))
        gy, guv = run(two)
        same((gy[0], guv[0]), exp, "two allocations")
        (ty, tuv), (by, buv) = rowpad_planes(1, dh, dw)
        gy, guv = run((ty, tuv))
        same((gy[0], guv[0]), exp, "row-padded planes")
        assert (by.cpu().numpy().reshape(dh, dw + 7)[:, dw:] == PX.U8_FILL).all() and (buv.cpu().numpy().reshape(dh // 2, dw + 6)[:, dw:] == PX.U8_FILL).all()
    # a batch: one shared matrix, and a matrix per frame
    frames = [RI.frame("uniform", 30 + i, SH, SW) for i in range(3)]
    ys, uvs = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    bgrs = np.stack([RI.nv12_to_bgr(*f) for f in frames])
    Ms = np.stack([wl.jitter_H(M, i) for i in range(3)])
    for mats in (M, Ms):
        m = lambda i: mats if mats.ndim == 2 else mats[i]  # noqa: E731
        want_b = [R.warp_to_nv12(bgrs[i], m(i), (dw, dh), interp) for i in range(3)]
        want_n = [R.warp_nv12_to_nv12(ys[i], uvs[i], m(i), (dw, dh), interp) for i in range(3)]
        same(gpu_bgr(W, bgrs, mats, (dw, dh), interp), tuple(np.stack(p) for p in zip(*want_b)), "batch, bgr source %s" % (mats.shape,))
        same(gpu_nv12(W, ys, uvs, mats, (dw, dh), interp, layout="single"), tuple(np.stack(p) for p in zip(*want_n)), "batch, nv12 source %s" % (mats.shape,))
    assert not np.array_equal(R.warp_to_nv12(bgrs[1], Ms[1], (dw, dh), interp)[0], R.warp_to_nv12(bgrs[1], M, (dw, dh), interp)[0])


@pytest.mark.parametrize("source", ["bgr", "nv12"])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR], ids=["nearest", "linear"])
def test_two_frames_two_matrices_every_stride_padded(W, interp, source):
    """What an entry point's argument filling can get wrong -- a swapped or dropped stride or pointer -- in the smallest shape that shows
    it: two frames with a matrix each, row and frame strides of every image that all differ from the tight ones and from each other, a
    destination of two tile columns (260 > 256) and two tile rows (6 > 4)."""
    sw, sh, dw, dh = 12, 10, 260, 6
    frames = [RI.frame("uniform", 70 + i, sh, sw) for i in range(2)]
    ys, uvs = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    H = wl.keystone_H(sw, sh, dw, dh)
    Ms = np.stack([wl.jitter_H(H, 1), wl.jitter_H(H, 2)])
    ty, tuv = PX.strided(ys, (9, 5)), PX.strided(uvs, (10, 6))   # (the pairs' strides stay even)
    bgrs = np.stack([RI.nv12_to_bgr(*f) for f in frames])
    tb = PX.strided(bgrs, (40, 3))
    oy, ouv = PX.strided(np.full((2, dh, dw), 33, np.uint8), (11, 7)), PX.strided(np.full((2, dh // 2, dw // 2, 2), 33, np.uint8), (4, 8))
    strides = [t.stride(0) for t in (ty, tuv, tb, oy, ouv)] + [t.stride(1) for t in (ty, tuv, tb, oy, ouv)]
    assert len(set(strides + [sh * sw, sw, sh // 2 * sw, sh * sw * 3, sw * 3, dh * dw, dw, dh // 2 * dw])) == 18
    if source == "bgr":
        W.warp_perspective_to_nv12(tb, Ms, (dw, dh), flags=interp, out=(oy, ouv))
        ref = lambda i, k: R.warp_to_nv12(bgrs[i], Ms[k], (dw, dh), interp)  # noqa: E731
    else:
        W.warp_nv12_to_nv12(ty, tuv, Ms, (dw, dh), flags=interp, out=(oy, ouv))
        ref = lambda i, k: R.warp_nv12_to_nv12(ys[i], uvs[i], Ms[k], (dw, dh), interp)  # noqa: E731
    exp = [ref(i, i) for i in range(2)]
    same(host(W, (oy, ouv)), tuple(np.stack(p) for p in zip(*exp)), "%s source, padded strides" % source)
    assert not np.array_equal(exp[0][0], ref(0, 1)[0])  # (the two matrices give different frames)


def canaried_planes(batch, dh, dw, align):
    """Both destination planes inside holders of their own whose every other byte is PX.CANARY.  align 16: both admit the 4-byte stores;
    0: the Y plane's base and row stride are odd (byte stores) and the UV plane's base is 2 mod 4 (16-bit stores: 2 is the contract)."""
    y4, y_holder = PX.canaried_out((batch, dh, dw, 1), torch.uint8, pad=5, align=align)
    if align:
        uv, uv_holder = PX.canaried_out((batch, dh // 2, dw // 2, 2), torch.uint8, pad=6, align=align)
        uv_view = uv
    else:  # (pairs as 16-bit elements: the helper then leaves the base one ELEMENT off a multiple of 16 bytes, which is even and no multiple of 4)
        uv_view, uv_holder = PX.canaried_out((batch, dh // 2, dw // 2), torch.int16, pad=6, align=0, planar=True)
        uv = uv_view.view(torch.uint8).unflatten(-1, (dw // 2, 2))
        assert uv.data_ptr() == uv_view.data_ptr() and uv.data_ptr() % 4 == 2 and y4.data_ptr() % 2 == 1
    assert tuple(uv.shape) == (batch, dh // 2, dw // 2, 2) and uv.stride(-1) == 1 and uv.stride(-2) == 2
    return (y4[..., 0], uv), ((y_holder, y4), (uv_holder, uv_view))


@pytest.mark.parametrize("align", [16, 0], ids=["dword_stores", "narrow_stores"])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR], ids=["nearest", "linear"])
def test_destination_layouts_keep_their_canaries(W, interp, align):
    M = wl.synth_brno_H(SW, SH, 258, 10)
    frames = [RI.frame("uniform", 40 + i, SH, SW) for i in range(2)]
    ys, uvs = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    bgrs = np.stack([RI.nv12_to_bgr(*f) for f in frames])
    for dw, dh in ((258, 6), (254, 4), (2, 2)):
        want_b = tuple(np.stack(p) for p in zip(*[R.warp_to_nv12(bgrs[i], M, (dw, dh), interp, border_value=BORDER) for i in range(2)]))
        want_n = tuple(np.stack(p) for p in zip(*[R.warp_nv12_to_nv12(ys[i], uvs[i], M, (dw, dh), interp, border_value=BORDER) for i in range(2)]))
        for source, want in (("bgr", want_b), ("nv12", want_n)):
            out, holders = canaried_planes(2, dh, dw, align)
            got = gpu_bgr(W, bgrs, M, (dw, dh), interp, border=BORDER, out=out) if source == "bgr" else gpu_nv12(W, ys, uvs, M, (dw, dh), interp, border=BORDER, out=out)
            same(got, want, "%s source, align %d, %dx%d" % (source, align, dw, dh))
            for holder, view in holders:
                PX.assert_canaries_intact(holder, view, "%s source, align %d, %dx%d" % (source, align, dw, dh))


# ---- 6. feeding the result back -------------------------------------------------------------------------------------------------------
def test_the_result_is_a_source_of_the_nv12_warp(W):
    dw, dh = 120, 38
    M = wl.keystone_H(SW, SH, dw, dh)
    bgr = wl.frame(3, SH, SW, np.uint8)
    out = W.warp_perspective_to_nv12(torch.from_numpy(bgr).cuda(), M, (dw, dh))
    assert tuple(out.shape) == (dh * 3 // 2, dw) and out.dtype == torch.uint8
    y, uv = W.split_nv12(out)
    back = W.warp_perspective_nv12(y, uv, np.eye(3), (dw, dh), flags=NEAREST)
    ey, euv = R.warp_to_nv12(bgr, M, (dw, dh), LINEAR)
    same(host(W, out), (ey, euv), "a new joined buffer")
    np.testing.assert_array_equal(back.cpu().numpy(), RI.nv12_to_bgr(ey, euv))
    # ... and of the warp into NV12 itself, batched
    outs = W.warp_nv12_to_nv12(torch.stack([y, y]), torch.stack([uv, uv]), np.eye(3), (dw, dh), flags=NEAREST)
    assert tuple(outs.shape) == (2, dh * 3 // 2, dw)
    again = R.bgr_to_nv12(RI.nv12_to_bgr(ey, euv))
    for i in range(2):
        same(host(W, outs[i]), again, "frame %d" % i)


# ---- 7. the pipeline -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["zero_copy", "copy", "resident"])
@pytest.mark.parametrize("src_format", ["bgr", "nv12"])
def test_frame_pipeline_writes_nv12_slots(src_format, mode):
    from bev_amd.pipeline import FramePipeline
    sw, sh, dw, dh = 64, 48, 40, 24
    M = wl.keystone_H(sw, sh, dw, dh)
    frames = [RI.frame("uniform" if i % 2 else "video", 50 + i, sh, sw) for i in range(5)]
    if src_format == "bgr":
        inputs = [RI.nv12_to_bgr(y, uv) for y, uv in frames]
        want = [R.warp_to_nv12(f, M, (dw, dh), LINEAR) for f in inputs]
    else:
        inputs = [RI.join(y, uv) for y, uv in frames]
        want = [R.warp_nv12_to_nv12(y, uv, M, (dw, dh), LINEAR) for y, uv in frames]
    with FramePipeline((sh, sw), 3, M, (dw, dh), src_format=src_format, dst_format="nv12", download=mode != "resident", zero_copy_out=mode == "zero_copy") as pipe:
        assert tuple(pipe.d_out[0].shape) == (dh * 3 // 2, dw) and pipe.d_out[0].dtype == torch.uint8
        assert pipe._out_bytes == dh * dw * 3 // 2  # half of a BGR frame's download
        if mode == "resident":
            assert pipe.h_out is None
        else:
            assert tuple(pipe.h_out[0].shape) == (dh * 3 // 2, dw) and pipe.h_out[0].dtype == torch.uint8 and pipe.h_out[0].is_pinned()
        outs = []
        for res in pipe.run(inputs):
            outs.append(np.array(res.cpu().numpy() if isinstance(res, torch.Tensor) else res))
    assert len(outs) == 5
    for (ey, euv), got in zip(want, outs):
        assert got.shape == (dh * 3 // 2, dw)
        same((got[:dh], got[dh:].reshape(dh // 2, dw // 2, 2)), (ey, euv), "%s %s" % (src_format, mode))
