"""NV12 frames through a fixed camera's warp map on the GPU (bev_amd.warp.remap_nv12 -> bevwarp_remap_nv12, remap_nv12_to_planar ->
bevwarp_remap_nv12_planes): every pixel against the numpy definition (tests/remap_nv12_ref.py: remap_ref.remap of nv12_ref's converted
frame, planes16_ref's plane stage) bit for bit, and against the entries the one launch stands in for -- remap of the converted frame,
warp_perspective_nv12, warp_to_planar of remap_nv12's pixels -- device against device.  Every destination is canaried.
Run on the GPU box:  python -m pytest tests -m gpu -q"""
import functools

import numpy as np
import pytest
import torch

from oracle import warp_numpy as wn
from tests import lens_ref as LR
from tests import nv12_ref as NR
from tests import pixels as PX
from tests import remap_nv12_ref as RN
from tests import remap_ref as RR
from tests import workloads as wl
from tests.test_gpu_remap import _shifted_map
from tests.test_lens_cpu import GEOMS

pytestmark = pytest.mark.gpu

LINEAR, NEAREST = 1, 0
INF = float("inf")
BORDER = (7.0, 200.0, 31.0)  # a non-zero border value per channel, in the result's order
CANVAS = 77                  # what PX.canaried_out fills a destination with
WIDTHS = (1, 3, 4, 5, 255, 256, 257)
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
SCALE, BIAS = (1 / 255.0, 0.017, 3.0), (-0.4, 0.25, 11.5)


@pytest.fixture(scope="module")
def W():
    from bev_amd import warp
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return warp


@functools.lru_cache(maxsize=None)
def _ref_map(geom, kind, interp):
    """(xy, frac) of a geometry as remap_ref builds them: the pinhole chain, or lens A with its default r2_max."""
    sw, sh, dw, dh, M = GEOMS[geom]
    if kind == "pinhole":
        return RR.build((dw, dh), wn.invert3x3(M), None, INF, interp)
    K = LR.camera_K(sw, sh)
    return RR.build((dw, dh), LR.ray_matrix(M, K), LR.lens12(K, LR.LENS_A), LR.lens_valid_r2(LR.LENS_A), interp)


def _gpu_map(W, geom, kind, interp):
    sw, sh, dw, dh, M = GEOMS[geom]
    if kind == "pinhole":
        return W.build_warp_map(M, (dw, dh), flags=interp)
    return W.build_warp_map(M, (dw, dh), flags=interp, K=LR.camera_K(sw, sh), dist_coeff=LR.LENS_A)


def _wrap(W, xy, frac, interp):
    """A WarpMap of host planes: xy (dh, dw, 2) or (n, dh, dw, 2) int16, frac uint16 of the same leading shape."""
    xy = xy if xy.ndim == 4 else xy[None]
    txy = torch.from_numpy(np.ascontiguousarray(xy)).cuda()
    tfrac = None
    if interp == LINEAR:
        frac = frac if frac.ndim == 3 else frac[None]
        tfrac = torch.from_numpy(np.ascontiguousarray(frac).view(np.int16)).cuda()
    return W.WarpMap(txy, tfrac, interp, (xy.shape[2], xy.shape[1]))


def _planes_of(y, uv, layout="joined", fill=3):
    """(y, uv) device tensors of one frame (H, W) or a batch (B, H, W): views of one joined buffer (split_nv12), or two allocations whose
    rows are padded with `fill` (7 bytes behind a Y row, 3 pairs behind a row of pairs; the uv base stays even)."""
    from bev_amd import warp
    if layout == "joined":
        joined = np.concatenate([y, uv.reshape(uv.shape[:-2] + (-1,))], axis=-2)
        return warp.split_nv12(torch.from_numpy(np.ascontiguousarray(joined)).cuda())
    H, Wd = y.shape[-2:]
    hy = torch.full(y.shape[:-1] + (Wd + 7,), fill, dtype=torch.uint8, device="cuda")
    hy[..., :Wd] = torch.from_numpy(y).cuda()
    hu = torch.full(uv.shape[:-2] + (Wd // 2 + 3, 2), fill, dtype=torch.uint8, device="cuda")
    hu[..., :Wd // 2, :] = torch.from_numpy(uv).cuda()
    return hy[..., :Wd], hu[..., :Wd // 2, :]


def _run(W, ty, tuv, m, mode, shape, rgb=False, align=16):
    """remap_nv12 into a canaried `out` of `shape`: the result on the host, with the canaries around it checked."""
    out, holder = PX.canaried_out(shape, np.uint8, pad=5, canvas=CANVAS, align=align)
    assert W.remap_nv12(ty, tuv, m, border_mode=mode, border_value=BORDER if mode == RR.CONSTANT else None, out=out, rgb=rgb) is out
    torch.cuda.synchronize()
    PX.assert_canaries_intact(holder, out)
    return out


def _exp(y, uv, xy, frac, interp, mode, rgb=False):
    dh, dw = xy.shape[:2]
    return RN.remap_nv12(y, uv, xy, frac, interp, mode, BORDER, canvas=np.full((dh, dw, 3), CANVAS, np.uint8), rgb=rgb)


# ---- 1. the conversion: every (Y, U, V) once, through an identity map ----

@pytest.mark.parametrize("rgb", [False, True], ids=["bgr", "rgb"])
def test_every_yuv_value_converts_like_the_reference(W, rgb):
    y, uv = NR.frame("domain", 0, 0, 0)
    gx, gy = np.meshgrid(np.arange(4096, dtype=np.int16), np.arange(4096, dtype=np.int16))
    xy = np.stack([gx, gy], axis=-1)
    ty, tuv = _planes_of(y, uv)
    got = _run(W, ty, tuv, _wrap(W, xy, None, NEAREST), RR.CONSTANT, (4096, 4096, 3), rgb=rgb).cpu().numpy()
    exp = RN.remap_nv12(y, uv, xy, None, NEAREST, RR.CONSTANT, BORDER, rgb=rgb)
    if not np.array_equal(got, exp):
        np.testing.assert_array_equal(got, exp)
    assert exp.min() == 0 and exp.max() == 255


# ---- 2. the main matrix, against the numpy definition and against the entries the launch replaces ----

@pytest.mark.parametrize("geom", sorted(GEOMS))
@pytest.mark.parametrize("kind", ["pinhole", "A"])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_parity_matrix(W, geom, kind, interp):
    sw, sh, dw, dh, M = GEOMS[geom]
    m = _gpu_map(W, geom, kind, interp)
    xy, frac = _ref_map(geom, kind, interp)
    keep = ~RR.written(xy, sw, sh, interp)
    modes = RR.MODES if kind == "pinhole" else (RR.CONSTANT, RR.TRANSPARENT)
    for frame_kind in ("uniform", "phase"):
        y, uv = NR.frame(frame_kind, 11, sh, sw)
        ty, tuv = _planes_of(y, uv)
        for rgb in (False, True):
            bgr = torch.from_numpy(NR.nv12_to_bgr(y, uv, rgb)).cuda()
            for mode in modes:
                what = "%s %s %s mode %d interp %d rgb %d" % (geom, kind, frame_kind, mode, interp, rgb)
                out = _run(W, ty, tuv, m, mode, (dh, dw, 3), rgb=rgb)
                got = out.cpu().numpy()
                np.testing.assert_array_equal(got, _exp(y, uv, xy, frac, interp, mode, rgb), err_msg=what)
                # device against device: remap of the converted frame, on every border
                two = torch.full((dh, dw, 3), CANVAS, dtype=torch.uint8, device="cuda")
                W.remap(bgr, m, border_mode=mode, border_value=BORDER if mode == RR.CONSTANT else None, out=two)
                assert torch.equal(out, two), what
                if mode == RR.TRANSPARENT:  # the canvas survives exactly off the written mask
                    assert (got[keep] == CANVAS).all() and keep.any() and not keep.all()
                if kind == "pinhole" and mode == RR.CONSTANT:  # ... and the pinhole NV12 warp of the same matrix
                    assert torch.equal(out, W.warp_perspective_nv12(ty, tuv, M, (dw, dh), flags=interp, border_value=BORDER, rgb=rgb)), what
    # without `out`: a new tensor; TRANSPARENT starts from zeros
    got = W.remap_nv12(ty, tuv, m, border_mode=RR.TRANSPARENT)
    torch.cuda.synchronize()
    assert got.shape == (dh, dw, 3)
    np.testing.assert_array_equal(got.cpu().numpy(), RN.remap_nv12(y, uv, xy, frac, interp, RR.TRANSPARENT))


# ---- 3. batching ----

def _random_map(rng, n, dh, dw, sw, sh):
    """Entries around a sw x sh source; the first half of every row lies inside in x (adjacent columns: the lanes that take window loads),
    the second half strays up to 4 px outside on every side."""
    xy = np.empty((n, dh, dw, 2), np.int16)
    xy[..., 0] = rng.integers(-4, sw + 4, (n, dh, dw))
    xy[..., 1] = rng.integers(-4, sh + 4, (n, dh, dw))
    xy[:, :, :dw // 2, 0] = rng.integers(0, sw - 1, (n, dh, dw // 2))
    return xy, rng.integers(0, 1024, (n, dh, dw)).astype(np.uint16)


@pytest.mark.parametrize("batch,per_frame", [(1, False), (2, False), (3, False), (5, False), (3, True)])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_batches(W, batch, per_frame, interp):
    """Every frame different, through a shared map and through a map per frame, on a small destination (one frame per item) and on an
    8 x 16384 one: 4096 tiles per frame, so a shared map walks two frames per item (tests/test_remap_cpu.py pins plan_remap) -- one group
    (2 frames), and a short last group (3 and 5 frames)."""
    sw, sh = 40, 24
    frames = [NR.frame("uniform", 20 + b, sh, sw) for b in range(batch)]
    ty, tuv = _planes_of(np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), "padded")
    for dw, dh in ((36, 20), (8, 16384)):
        xy, frac = _random_map(np.random.default_rng(batch * 10 + dh), batch if per_frame else 1, dh, dw, sw, sh)
        m = _wrap(W, xy, frac, interp)
        for mode in (RR.CONSTANT, RR.REFLECT_101, RR.TRANSPARENT):
            got = _run(W, ty, tuv, m, mode, (batch, dh, dw, 3)).cpu().numpy()
            for b in range(batch):
                k = b if per_frame else 0
                np.testing.assert_array_equal(got[b], _exp(frames[b][0], frames[b][1], xy[k], frac[k], interp, mode),
                                              err_msg="frame %d of %d, mode %d, %d x %d, %d maps" % (b, batch, mode, dw, dh, m.n))


# ---- 4. destination widths and layouts ----

@pytest.mark.parametrize("dw", WIDTHS)
def test_widths_and_layouts(W, dw):
    """Rows that end inside a lane's 4 pixels, at a tile's edge and one past it, at a height of 5 (two tile rows): `out` as an unaligned
    padded view and in the wide-store layout, the map planes as unaligned padded views and as aligned ones."""
    sw, sh, dh = 32, 18, 5
    M = wl.rotated_H(sw, sh, dw, dh, 12.0, zoom=1.3)
    y, uv = NR.frame("phase", 30, sh, sw)
    ty, tuv = _planes_of(y, uv)
    for interp in (NEAREST, LINEAR):
        m = W.build_warp_map(M, (dw, dh), flags=interp)
        xy, frac = RR.build((dw, dh), wn.invert3x3(M), None, INF, interp)
        maps = [m, _shifted_map(W, m, 4, 2, 3)[0], _shifted_map(W, m, 16, 8, 0)[0], _shifted_map(W, m, 0, 0, 4)[0]]
        for mode in (RR.CONSTANT, RR.REPLICATE, RR.TRANSPARENT):
            exp = _exp(y, uv, xy, frac, interp, mode)
            for mm in maps:
                for align in (16, 0):
                    got = _run(W, ty, tuv, mm, mode, (dh, dw, 3), align=align).cpu().numpy()
                    np.testing.assert_array_equal(got, exp, err_msg="%d x %d mode %d interp %d align %d" % (dw, dh, mode, interp, align))


# ---- 5. source layouts and tiny sources ----

@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_source_layouts(W, interp):
    """One buffer through split_nv12 and two allocations with padded rows, single frames and a batch of 2 with a shared map."""
    sw, sh, dw, dh, M = GEOMS["rotated_zoom_out"]
    m = _gpu_map(W, "rotated_zoom_out", "pinhole", interp)
    xy, frac = _ref_map("rotated_zoom_out", "pinhole", interp)
    frames = [NR.frame("uniform", 40 + b, sh, sw) for b in range(2)]
    ys, uvs = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    for layout in ("joined", "padded"):
        for mode in (RR.CONSTANT, RR.WRAP):
            ty, tuv = _planes_of(ys, uvs, layout)
            got = _run(W, ty, tuv, m, mode, (2, dh, dw, 3)).cpu().numpy()
            for b in range(2):
                np.testing.assert_array_equal(got[b], _exp(frames[b][0], frames[b][1], xy, frac, interp, mode), err_msg="%s mode %d frame %d" % (layout, mode, b))
            ty, tuv = _planes_of(ys[1], uvs[1], layout)
            np.testing.assert_array_equal(_run(W, ty, tuv, m, mode, (dh, dw, 3)).cpu().numpy(), got[1])


@pytest.mark.parametrize("src_wh", [(2, 2), (4, 2), (2, 4), (4, 4), (6, 4)])
def test_tiny_sources_and_hand_made_maps(W, src_wh):
    """Hand-made maps over the whole int16 range, the sentinel and 32767 included, on sources of one, two and three pairs per row -- the
    sizes at which the window loads are refused (2 px), start at pair 0 only (4 px) or move (6 px).  A third of the entries lie inside in
    x with every lane's four side by side (window lanes).  Each case runs with the row padding of y and uv filled with 0 and with 255: a
    load that strays past src_w bytes of a row changes the answer."""
    sw, sh = src_wh
    dh, dw = 3, 261  # (two tile columns; few entries: the reference's index remap is a Python loop over the distinct indices)
    rng = np.random.default_rng(sw * 10 + sh)
    xy = rng.integers(-32768, 32768, (dh, dw, 2)).astype(np.int16)
    near = rng.integers(-3 * max(sw, sh) - 2, 3 * max(sw, sh) + 3, (dh, dw, 2)).astype(np.int16)
    xy[:, ::2] = near[:, ::2]
    xy[:, 88:176, 0] = rng.integers(0, sw - 1, (dh, 88))          # adjacent columns inside, rows anywhere near
    xy[:, 88:176, 1] = rng.integers(-2, sh + 2, (dh, 88))
    xy[2, 176:216, 0] = rng.integers(0, sw - 1, 40) + sw * rng.integers(-3, 4, 40)   # (WRAP: adjacent columns after the remap)
    xy[0, :8] = [[-32768, -32768], [32767, 32767], [-32768, 0], [0, -32768], [32767, 0], [0, 32767], [-1, -1], [0, 0]]
    frac = rng.integers(0, 65536, (dh, dw)).astype(np.uint16)
    frac[1, :4] = [0, 1023, 0xfc00, 0xffff]
    y, uv = NR.frame("phase", 50, sh, sw)
    for interp in (NEAREST, LINEAR):
        m = _wrap(W, xy, frac, interp)
        for mode in RR.MODES:
            exp = _exp(y, uv, xy, frac, interp, mode)
            for fill in (0, 255):
                ty, tuv = _planes_of(y, uv, "padded", fill)
                got = _run(W, ty, tuv, m, mode, (dh, dw, 3)).cpu().numpy()
                np.testing.assert_array_equal(got, exp, err_msg="%s mode %d interp %d padding %d" % (src_wh, mode, interp, fill))


# ---- 6. planes ----

def _plane_out(shape, dtype, align):
    """A canaried (3, dh, dw) / (B, 3, dh, dw) destination of `dtype`: (out, holder).  align 0: base and row stride off the wide stores."""
    carrier = torch.float32 if dtype == F32 else torch.int16
    view, holder = PX.canaried_out(shape, carrier, pad=6, align=align, planar=True)
    out = view.view(dtype)
    assert out.data_ptr() == view.data_ptr() and out.stride() == view.stride()
    return out, view, holder


def _run_planes(W, ty, tuv, m, mode, shape, dtype, rgb=False, align=16, scale=SCALE, bias=BIAS):
    out, view, holder = _plane_out(shape, dtype, align)
    assert W.remap_nv12_to_planar(ty, tuv, m, scale=scale, bias=bias, border_mode=mode, border_value=BORDER if mode == RR.CONSTANT else None, out=out, rgb=rgb,
                                  out_dtype=dtype) is out
    torch.cuda.synchronize()
    PX.assert_canaries_intact(holder, view)
    return out


@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_planes_parity(W, dtype, interp):
    """Per-channel scale and bias, the five borders, both channel orders: against the definition, and against warp_to_planar (identity,
    nearest) of remap_nv12's pixels, device against device."""
    sw, sh, dw, dh, M = GEOMS["rotated_zoom_out"]
    y, uv = NR.frame("uniform", 60, sh, sw)
    ty, tuv = _planes_of(y, uv)
    for kind, modes in (("pinhole", RR.MODES[:5]), ("A", (RR.CONSTANT,))):
        m = _gpu_map(W, "rotated_zoom_out", kind, interp)
        xy, frac = _ref_map("rotated_zoom_out", kind, interp)
        for mode in modes:
            for rgb in (False, True):
                what = "%s mode %d interp %d rgb %d %s" % (kind, mode, interp, rgb, dtype)
                out = _run_planes(W, ty, tuv, m, mode, (3, dh, dw), dtype, rgb=rgb)
                RN.assert_planes_equal(out, RN.remap_nv12_planes(y, uv, xy, frac, interp, mode, SCALE, BIAS, BORDER, rgb=rgb), dtype, what)
                pixels = W.remap_nv12(ty, tuv, m, border_mode=mode, border_value=BORDER if mode == RR.CONSTANT else None, rgb=rgb)
                two = W.warp_to_planar(pixels, np.eye(3), (dw, dh), scale=SCALE, bias=BIAS, flags=NEAREST, out_dtype=dtype)
                torch.cuda.synchronize()
                assert torch.equal(out.view(torch.int32 if dtype == F32 else torch.int16), two.view(torch.int32 if dtype == F32 else torch.int16)), what
    # without `out`, a batch of 3 through the shared map: (B, 3, h, w)
    frames = [NR.frame("uniform", 61 + b, sh, sw) for b in range(3)]
    ty, tuv = _planes_of(np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), "padded")
    got = W.remap_nv12_to_planar(ty, tuv, m, scale=SCALE, bias=BIAS, border_value=BORDER, out_dtype=dtype)
    torch.cuda.synchronize()
    assert got.shape == (3, 3, dh, dw) and got.dtype == dtype
    for b in range(3):
        RN.assert_planes_equal(got[b], RN.remap_nv12_planes(frames[b][0], frames[b][1], xy, frac, interp, RR.CONSTANT, SCALE, BIAS, BORDER), dtype, "frame %d" % b)


@pytest.mark.parametrize("dw", WIDTHS)
def test_planes_widths_and_layouts(W, dw):
    """The width set at a height of 5, planes padded and canaried, in the wide-store layout and off it."""
    sw, sh, dh = 32, 18, 5
    M = wl.rotated_H(sw, sh, dw, dh, 12.0, zoom=1.3)
    y, uv = NR.frame("phase", 30, sh, sw)
    ty, tuv = _planes_of(y, uv, "padded")
    for interp in (NEAREST, LINEAR):
        m = W.build_warp_map(M, (dw, dh), flags=interp)
        xy, frac = RR.build((dw, dh), wn.invert3x3(M), None, INF, interp)
        for mode in (RR.CONSTANT, RR.REFLECT):
            exp = RN.remap_nv12_planes(y, uv, xy, frac, interp, mode, SCALE, BIAS, BORDER)
            for dtype in (F32, F16, BF16):
                for align in (16, 0):
                    out = _run_planes(W, ty, tuv, m, mode, (3, dh, dw), dtype, align=align)
                    RN.assert_planes_equal(out, exp, dtype, "%d x %d mode %d interp %d %s align %d" % (dw, dh, mode, interp, dtype, align))
