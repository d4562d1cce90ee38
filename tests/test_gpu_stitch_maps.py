"""The multi-camera stitch through warp maps on the GPU (bev_amd.warp.remap_stitch / remap_stitch_nv12 -> bevwarp_stitch_maps /
bevwarp_stitch_maps_nv12), each result compared with the numpy definition tests/stitch_maps_ref.py bit for bit.  Destinations are
pre-filled with 77, so a pixel a launch leaves unwritten does not pass as zero.
Run on the GPU box:  python -m pytest tests -m gpu -q"""
import functools

import numpy as np
import pytest
import torch

from tests import float_domain as FD
from tests import lens_ref as LR
from tests import nv12_ref as NR
from tests import pixels as PX
from tests import remap_ref as RR
from tests import stitch_maps_ref as SM

pytestmark = pytest.mark.gpu

LINEAR, NEAREST, INVERSE = 1, 0, 16
# tests/test_gpu_stitch.py's three cameras on its 260 x 22 canvas (two tile columns, six tile rows, a ragged last lane), the third with
# even sides so that NV12 frames take the same scene: (w, h, inverse map, lens of the lens scene)
SCENE = [(40, 24, np.array([[0.30, 0.20, -4], [0.01, 0.90, -1], [0.0004, 0, 1]]), LR.LENS_A),
         (64, 18, np.array([[0.38, 0, -36], [0.02, 0.80, -3], [0, 0, 1]]), LR.LENS_B),
         (32, 34, np.array([[-0.35, 0, 80], [0, 1.40, -2], [0, 0.001, 1]]), LR.LENS_A)]
DSIZE = (260, 22)
BLENDS = (("over", 64), ("feather", 1), ("feather", 3), ("feather", 64))
MODES = (SM.CONSTANT, SM.TRANSPARENT)


@pytest.fixture(scope="module")
def W():
    from bev_amd import warp
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return warp


def _src(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, shape, dtype=np.uint8) if dtype == np.uint8 else rng.random(shape, dtype=np.float32)


def _sources(dtype, c=3):
    """The scene's sources ((h, w, c); c = 0: (h, w))."""
    return [_src((h, w, c) if c else (h, w), dtype, seed=30 + 4 * k + c) for k, (w, h, _, _) in enumerate(SCENE)]


@functools.lru_cache(maxsize=None)
def scene_maps(interp, lens, dsize=DSIZE):
    """The scene's maps from the definition (computed once, never modified): pinhole, or through each camera's lens with lens_valid_r2."""
    out = []
    for w, h, Minv, dist in SCENE:
        if lens:
            K = LR.camera_K(w, h)
            out.append(RR.build(dsize, LR.ray_matrix(Minv, K, inverse_given=True), LR.lens12(K, dist), LR.lens_valid_r2(dist), interp))
        else:
            out.append(RR.build(dsize, Minv, interp=interp))
    return out


def _bv(c):
    return (3.0, 200.0, 41.0, 117.0)[:max(c, 1)]


def dev_map(W, xy, frac, interp):
    """A WarpMap of n frames on the device from the definition's planes: (dh, dw, 2) + (dh, dw), or stacks of them."""
    xy = np.ascontiguousarray(xy)
    xy = xy if xy.ndim == 4 else xy[None]
    txy = torch.empty(xy.shape, dtype=torch.int16, device="cuda")  # (canonical strides, whatever numpy gives dimensions of 1)
    txy.copy_(torch.from_numpy(xy))
    tfr = None
    if interp == LINEAR:
        tfr = torch.empty(xy.shape[:3], dtype=torch.int16, device="cuda")
        tfr.copy_(torch.from_numpy(np.ascontiguousarray(frac).view(np.int16).reshape(xy.shape[:3])))
    return W.WarpMap(txy, tfr, interp, (txy.shape[2], txy.shape[1]))


def _canvas(maps, like, fill=77):
    dh, dw = maps[0][0].shape[-3:-1]
    return np.full((dh, dw) + tuple(like.shape[2:]), fill, like.dtype)


def gpu(W, srcs, maps, interp, blend, feather, mode, border_value=None):
    ts = [torch.from_numpy(np.ascontiguousarray(s)).cuda() for s in srcs]
    out = torch.from_numpy(_canvas(maps, srcs[0])).cuda()
    got = W.remap_stitch(ts, [dev_map(W, xy, frac, interp) for xy, frac in maps], blend=blend, feather=feather, border_value=border_value, out=out, border_mode=mode)
    torch.cuda.synchronize()
    assert got is out
    return got.cpu().numpy()


def ref(srcs, maps, interp, blend, feather, mode, border_value=0.0):
    return SM.stitch(srcs, maps, interp, SM.FEATHER if blend == "feather" else SM.OVER, feather, mode, border_value, _canvas(maps, srcs[0]))


def check(W, srcs, maps, interp, blend, feather, mode, border_value=0.0):
    got = gpu(W, srcs, maps, interp, blend, feather, mode, border_value)
    exp, count = ref(srcs, maps, interp, blend, feather, mode, border_value)
    np.testing.assert_array_equal(got, exp, err_msg="%s F=%d mode %d interp %d %s %s" % (blend, feather, mode, interp, srcs[0].dtype, srcs[0].shape))
    if mode == SM.TRANSPARENT:  # the canvas keeps 77 exactly where no camera covers
        assert (got[count == 0] == 77).all()
    return count


# ---- 1. the scene: every format, blend and border, pinhole and lens maps ----

@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
@pytest.mark.parametrize("lens", [False, True])
def test_scene_matrix(W, dtype, interp, lens):
    maps = scene_maps(interp, lens)
    for c in (1, 2, 3, 4, 0):  # (0: (H, W) sources)
        srcs = _sources(dtype, c)
        for blend, F in BLENDS:
            for mode in MODES:
                count = check(W, srcs, maps, interp, blend, F, mode, _bv(c))
    for n in range(4):  # the case cannot pass on an empty overlap
        assert (count == n).sum() >= 20, (n, int((count == n).sum()))
    assert (count[:, 256:] > 0).any()
    sentinels = [int(((xy[..., 0] == -32768) & (xy[..., 1] == -32768)).sum()) for xy, _ in maps]
    assert (max(sentinels) >= 100) == lens, sentinels  # a lens map's pixels beyond r2_max are no camera's


# ---- 2. the three identities, against the device's own routes ----

@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_pinhole_maps_equal_warp_stitch(W, dtype, interp):
    """(i): maps built on the device from the matrices give warp_stitch's canvas for every blend and border."""
    srcs = _sources(dtype)
    ts = [torch.from_numpy(s).cuda() for s in srcs]
    Ms = [M for _, _, M, _ in SCENE]
    built = [W.build_warp_map(M, DSIZE, flags=interp | INVERSE) for M in Ms]
    for blend, F in BLENDS:
        for mode in MODES:
            a = torch.full((DSIZE[1], DSIZE[0], 3), 77, dtype=ts[0].dtype, device="cuda")
            b = torch.full_like(a, 77)
            W.warp_stitch(ts, Ms, DSIZE, flags=interp | INVERSE, blend=blend, feather=F, border_value=_bv(3), out=a, border_mode=mode)
            W.remap_stitch(ts, built, blend=blend, feather=F, border_value=_bv(3), out=b, border_mode=mode)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(b.cpu().numpy().view(np.uint8), a.cpu().numpy().view(np.uint8), err_msg="%s F=%d mode %d" % (blend, F, mode))
    assert (a.cpu().numpy() != 77).any()


@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
@pytest.mark.parametrize("lens", [False, True])
def test_over_equals_the_sequence_of_transparent_remaps(W, interp, lens):
    """(ii), for frames of both types and for NV12 planes, in both list orders."""
    maps = [dev_map(W, xy, frac, interp) for xy, frac in scene_maps(interp, lens)]
    frames = [NR.frame("uniform", 11 + k, h, w) for k, (w, h, _, _) in enumerate(SCENE)]
    ys, uvs = [torch.from_numpy(y).cuda() for y, _ in frames], [torch.from_numpy(uv).cuda() for _, uv in frames]
    for dtype in (np.uint8, np.float32):
        ts = [torch.from_numpy(s).cuda() for s in _sources(dtype)]
        results = []
        for order in ((0, 1, 2), (2, 1, 0)):
            canvas = torch.full((DSIZE[1], DSIZE[0], 3), 77, dtype=ts[0].dtype, device="cuda")
            for k in order:
                W.remap(ts[k], maps[k], border_mode=W.BORDER_TRANSPARENT, out=canvas)
            one = torch.full_like(canvas, 77)
            W.remap_stitch([ts[k] for k in order], [maps[k] for k in order], blend="over", out=one, border_mode=W.BORDER_TRANSPARENT)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(one.cpu().numpy(), canvas.cpu().numpy())
            results.append(one.cpu().numpy())
        assert not np.array_equal(results[0], results[1]) and (results[0] == 77).any()
    for rgb in (False, True):
        canvas = torch.full((DSIZE[1], DSIZE[0], 3), 77, dtype=torch.uint8, device="cuda")
        for k in range(3):
            W.remap_nv12(ys[k], uvs[k], maps[k], border_mode=W.BORDER_TRANSPARENT, out=canvas, rgb=rgb)
        one = torch.full_like(canvas, 77)
        W.remap_stitch_nv12(ys, uvs, maps, blend="over", out=one, border_mode=W.BORDER_TRANSPARENT, rgb=rgb)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(one.cpu().numpy(), canvas.cpu().numpy())


# ---- 3. every NV12 instance ----

def _nv12_frame(seed, h, w):
    """Random planes that hold Y, U and V of 0 and 255 (both clamps of the conversion, and its largest sums)."""
    y, uv = NR.frame("uniform", seed, h, w)
    y, uv = y.copy(), uv.copy()
    y[0, :2], y[-1, -2:] = (0, 255), (255, 0)
    uv[0, 0], uv[-1, -1], uv[0, -1], uv[-1, 0] = (0, 0), (255, 255), (0, 255), (255, 0)
    return y, uv


def _nv12_devices(frames, layout):
    """joined: one buffer per camera, the rows of pairs behind the Y rows (split_nv12's views); padded: row-padded planes of their own."""
    from bev_amd import warp
    if layout == "joined":
        views = [warp.split_nv12(torch.from_numpy(NR.join(y, uv)).cuda()) for y, uv in frames]
        return [v[0] for v in views], [v[1] for v in views]
    return [PX.strided(y, (5 + 2 * k,)) for k, (y, _) in enumerate(frames)], [PX.strided(uv, (4 + 2 * k,)) for k, (_, uv) in enumerate(frames)]


@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
@pytest.mark.parametrize("blend,F", [("over", 64), ("feather", 3)])
@pytest.mark.parametrize("rgb", [False, True])
def test_nv12_instance(W, interp, blend, F, rgb):
    """One kernel instance per case: the definition, and (iii) the device's own remap_stitch of the converted frames."""
    frames = [_nv12_frame(20 + k, h, w) for k, (w, h, _, _) in enumerate(SCENE)]
    assert all(v in y and v in uv[..., 0] and v in uv[..., 1] for y, uv in frames for v in (0, 255))
    for lens, layout in ((False, "joined"), (True, "padded")):
        maps = scene_maps(interp, lens)
        dmaps = [dev_map(W, xy, frac, interp) for xy, frac in maps]
        ys, uvs = _nv12_devices(frames, layout)
        bgr = [torch.from_numpy(NR.nv12_to_bgr(y, uv, rgb)).cuda() for y, uv in frames]
        for mode in MODES:
            out = torch.full((DSIZE[1], DSIZE[0], 3), 77, dtype=torch.uint8, device="cuda")
            conv = torch.full_like(out, 77)
            got = W.remap_stitch_nv12(ys, uvs, dmaps, blend=blend, feather=F, border_value=_bv(3), out=out, border_mode=mode, rgb=rgb)
            W.remap_stitch(bgr, dmaps, blend=blend, feather=F, border_value=_bv(3), out=conv, border_mode=mode)
            torch.cuda.synchronize()
            assert got is out
            exp, count = SM.stitch_nv12([y for y, _ in frames], [uv for _, uv in frames], maps, interp, SM.FEATHER if blend == "feather" else SM.OVER, F, mode, _bv(3),
                                        np.full((DSIZE[1], DSIZE[0], 3), 77, np.uint8), rgb)
            np.testing.assert_array_equal(out.cpu().numpy(), exp, err_msg="lens %s mode %d" % (lens, mode))
            np.testing.assert_array_equal(out.cpu().numpy(), conv.cpu().numpy())
            assert all((count == n).any() for n in range(4))
    # sources of 2 x 2 and 4 x 2 px (w x h) through hand-made maps: one pair per row, and the narrowest row that holds a window of pairs
    for w, h in ((2, 2), (4, 2)):
        y, uv = _nv12_frame(40 + w, h, w)
        sx = np.array([[-1, 0, 1, 2, 3, 4, 0, w - 2, w - 1]], np.int16)
        xy = np.stack([np.repeat(sx, 3, 0), np.repeat(np.array([[0], [1], [-1]], np.int16), sx.shape[1], 1)], axis=-1)
        frac = (np.arange(27, dtype=np.uint16).reshape(3, 9) * 37 + 5) & 1023
        srcs2 = [(y, uv), (y[::-1].copy(), uv)]
        for mode in MODES:
            out = torch.full((3, 9, 3), 77, dtype=torch.uint8, device="cuda")
            W.remap_stitch_nv12([torch.from_numpy(a).cuda() for a, _ in srcs2], [torch.from_numpy(b).cuda() for _, b in srcs2], [dev_map(W, xy, frac, interp)] * 2, blend=blend,
                                feather=F, border_value=_bv(3), out=out, border_mode=mode, rgb=rgb)
            torch.cuda.synchronize()
            exp, count = SM.stitch_nv12([a for a, _ in srcs2], [b for _, b in srcs2], [(xy, frac)] * 2, interp, SM.FEATHER if blend == "feather" else SM.OVER, F, mode, _bv(3),
                                        np.full((3, 9, 3), 77, np.uint8), rgb)
            np.testing.assert_array_equal(out.cpu().numpy(), exp, err_msg="%d x %d mode %d" % (w, h, mode))
            assert (count == 2).any() and (count == 0).any()


# ---- 4. layouts and batches ----

def _jitter(M, i):
    return M + np.array([[0.01 * i, 0, 1.5 * i], [0, -0.02 * i, 0.75 * i], [0, 0, 0]])


@pytest.mark.parametrize("dtype,c", [(np.uint8, 3), (np.float32, 4)])
@pytest.mark.parametrize("blend,F", [("over", 64), ("feather", 3)])
def test_batch_strides_maps_and_destinations(W, dtype, c, blend, F):
    """A batch of 3.  Camera 0: a shared map in aligned planes; camera 1: a map per frame in row-padded planes at addresses that are no
    multiple of 16 / 8 (loads entry by entry, in the same launch as camera 0's lane-wide loads); camera 2: a shared lens map.  Every source
    a window of a larger tensor whose row and frame strides all differ.  An 8-bit destination at an odd address between two guard bytes
    (every pixel stored on its own) and an aligned float32 4-channel destination (the wide stores)."""
    B, (dw, dh) = 3, DSIZE
    host = [_src((B, h, w, c), dtype, seed=50 + k) for k, (w, h, _, _) in enumerate(SCENE)]
    srcs = [PX.strided(s, (37 + 8 * k, 3 + k)) for k, s in enumerate(host)]
    m0 = scene_maps(LINEAR, False)[0]
    m1 = [RR.build(DSIZE, _jitter(SCENE[1][2], i), interp=LINEAR) for i in range(B)]
    m2 = scene_maps(LINEAR, True)[2]
    xy1, fr1 = np.stack([m[0] for m in m1]), np.stack([m[1] for m in m1])
    d0, d2 = dev_map(W, *m0, LINEAR), dev_map(W, *m2, LINEAR)
    assert d0.xy.data_ptr() % 16 == 0 and d0.frac.data_ptr() % 8 == 0 and d0.xy.stride(1) * 2 % 16 == 0 and d0.frac.stride(1) * 2 % 8 == 0
    hx = torch.full((B * dh * (2 * dw + 6) + 2,), 0x7f7f, dtype=torch.int16, device="cuda")
    pxy = torch.as_strided(hx, (B, dh, dw, 2), (dh * (2 * dw + 6), 2 * dw + 6, 2, 1), 2)
    pxy.copy_(torch.from_numpy(xy1).cuda())
    hf = torch.full((B * dh * (dw + 3) + 1,), 0x7f7f, dtype=torch.int16, device="cuda")
    pfr = torch.as_strided(hf, (B, dh, dw), (dh * (dw + 3), dw + 3, 1), 1)
    pfr.copy_(torch.from_numpy(fr1.view(np.int16)).cuda())
    d1 = W.WarpMap(pxy, pfr, LINEAR, DSIZE)
    assert d1.xy.data_ptr() % 16 == 4 and d1.frac.data_ptr() % 8 == 2 and (d1.xy.stride(1) * 2) % 16 != 0 and d1.n == B
    n = B * dh * dw * c
    if dtype == np.uint8:
        buf = torch.full((n + 2,), 77, dtype=torch.uint8, device="cuda")
        out = buf[1:n + 1].view(B, dh, dw, c)
        assert out.data_ptr() % 2 == 1
    else:
        buf = torch.full((n,), 77, dtype=torch.float32, device="cuda")
        out = buf.view(B, dh, dw, c)
        assert out.data_ptr() % 16 == 0 and (dw * c * 4) % 16 == 0
    for mode in MODES:
        out.fill_(77)
        got = W.remap_stitch(srcs, [d0, d1, d2], blend=blend, feather=F, border_value=_bv(c), out=out, border_mode=mode)
        torch.cuda.synchronize()
        assert got is out and (dtype != np.uint8 or (buf[0].item() == 77 and buf[-1].item() == 77))
        frames = []
        for b in range(B):
            exp, count = ref([s[b] for s in host], [m0, m1[b], m2], LINEAR, blend, F, mode, _bv(c))
            np.testing.assert_array_equal(out[b].cpu().numpy(), exp, err_msg="frame %d mode %d" % (b, mode))
            assert (count >= 2).sum() >= 40
            frames.append(exp)
        assert not np.array_equal(frames[0], frames[1]) and not np.array_equal(frames[1], frames[2])  # (frames and maps differ)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_one_camera_and_eight(W, dtype, interp):
    w, h, M, _ = SCENE[0]
    s = _src((h, w, 3), dtype, seed=60)
    m = scene_maps(interp, False)[0]
    for blend, F in BLENDS:
        got = gpu(W, [s], [m], interp, blend, F, SM.TRANSPARENT)
        np.testing.assert_array_equal(got, RR.remap(s, m[0], m[1], interp, RR.TRANSPARENT, canvas=np.full((DSIZE[1], DSIZE[0], 3), 77, dtype)))
    # eight cameras over a common area: the scene's first map, shifted and sheared a little per camera
    sizes = [(40, 24), (33, 29), (64, 18), (25, 25), (47, 21), (31, 33), (52, 20), (38, 27)]
    srcs = [_src((hh, ww, 3), dtype, seed=61 + k) for k, (ww, hh) in enumerate(sizes)]
    maps = [RR.build(DSIZE, M + np.array([[0.01 * k, 0.005 * k, -1.5 * k], [0, 0.03 * k, -0.5 * k], [0, 0, 0]]), interp=interp) for k in range(8)]
    for blend, F in BLENDS:
        for mode in MODES:
            count = check(W, srcs, maps, interp, blend, F, mode, _bv(3))
    assert (count == 8).sum() >= 40 and (count == 0).sum() >= 40 and len(np.unique(count)) >= 6


@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_canvas_widths(W, interp):
    """1, 3, 4, 5 px and one tile of 256 px +- 1: ragged lanes at the row's end, in one and in two tile columns."""
    for dw in (1, 3, 4, 5, 255, 256, 257):
        T = np.array([[1.0, 0, 120.0 if dw <= 5 else 0.0], [0, 1, 0], [0, 0, 1]])  # (the narrow canvases lie where both cameras look)
        maps = [RR.build((dw, 7), SCENE[k][2] @ T, interp=interp) for k in (0, 1)]
        for dtype, c in ((np.uint8, 3), (np.float32, 1)):
            srcs = _sources(dtype, c)[:2]
            for blend, F in (("over", 64), ("feather", 3)):
                for mode in MODES:
                    count = check(W, srcs, maps, interp, blend, F, mode, _bv(c))
            assert count[:, -1].max() >= 1, dw  # the last column is covered


# ---- 5. extreme entries ----

@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_extreme_entries_and_tiny_sources(W, dtype, interp):
    """Hand-made maps over the whole int16 range, frac values with their high bits set, against sources of 1 x 1, 2 x 2 and 9 x 7 px."""
    rng = np.random.default_rng(5)
    edge = np.array([-32768, -32767, -2, -1, 0, 1, 2, 5, 6, 7, 8, 9, 32766, 32767], np.int16)
    for sw, sh in ((1, 1), (2, 2), (9, 7)):
        near = np.array([sw - 2, sw - 1, sw, sh - 2, sh - 1, sh], np.int16)
        vals = np.concatenate([edge, near])
        xy = np.stack(np.meshgrid(vals, vals), axis=-1).astype(np.int16)  # every pair of them, (-32768, -32768) and (32767, 32767) included
        assert xy.shape[1] == 20 and (xy.reshape(-1, 2) == (-32768, -32768)).all(1).any() and (xy.reshape(-1, 2) == (sw - 1, sh - 1)).all(1).any()
        frac = rng.integers(0, 65536, xy.shape[:2]).astype(np.uint16)
        frac[0, :4] = (0xffff, 0xfc00, 0x8421, 1023)
        srcs = [_src((sh, sw, 3), dtype, seed=80 + sw), _src((sh, sw, 3), dtype, seed=90 + sw)]
        maps = [(xy, frac), (xy, frac), (np.ascontiguousarray(xy[::-1, ::-1]), frac)]  # (two cameras share a map)
        srcs.append(_src((sh, sw, 3), dtype, seed=70 + sw))
        for blend, F in (("over", 64), ("feather", 1), ("feather", 2)):
            for mode in MODES:
                count = check(W, srcs, maps, interp, blend, F, mode, _bv(3))
        if interp == LINEAR and sw == 1:
            assert count.max() == 0  # bilinear never covers a 1-wide source
        else:
            assert count.max() >= 2 and (count == 0).any() and len(np.unique(count)) >= 3


def test_feather_sums_next_to_2_23(W):
    """F = 4096 and 8 cameras that all cover with w_k = 4096 (entries 4096 px from every edge of an 8192 x 8192 frame): W = 32768, and where
    all are 255 the sum is 8 * 4096 * 255 + 16384 = 8,372,224, just below 2^23."""
    n = 8192
    t = torch.full((n, n), 255, dtype=torch.uint8, device="cuda")
    t[4094:4098, 4094:4098] = torch.arange(16, dtype=torch.uint8, device="cuda").view(4, 4) * 16 + 3
    host = t.cpu().numpy()
    sx = np.array([4095, 4095, 4094, 4096, 4095, 4000, 4095], np.int16)
    sy = np.array([4095, 4000, 4095, 4095, 4096, 4000, 4094], np.int16)
    xy = np.stack([sx, sy], axis=-1)[None]
    frac = (np.arange(7, dtype=np.uint16) * 149 + 7)[None] & 1023
    for interp in (NEAREST, LINEAR):
        cams = SM.cameras([host] * 8, [(xy, frac)] * 8, interp, 4096)
        assert sum(wk for _, _, wk in cams)[0, 0] == 32768 and all(cover.all() for cover, _, _ in cams)
        out = torch.full((1, 7), 77, dtype=torch.uint8, device="cuda")
        W.remap_stitch([t] * 8, [dev_map(W, xy, frac, interp)] * 8, blend="feather", feather=4096, out=out)
        torch.cuda.synchronize()
        exp, _ = SM.stitch([host] * 8, [(xy, frac)] * 8, interp, SM.FEATHER, 4096)
        np.testing.assert_array_equal(out.cpu().numpy(), exp)
        assert exp[0, 1] == 255 and exp[0, 5] == 255 and exp[0, 0] != 255


# ---- 6. float32: specials in the sources ----

@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_float32_specials(W, interp):
    """NaN (quiet and signalling), +-inf, +-0 and denormals in the sources.  Every pixel that is a copy -- nearest under OVER or a single
    cover, the border fill, the canvas -- keeps all 32 bits; a computed pixel equals the definition by bits, or is some NaN where that is."""
    srcs = [PX.float_frame("mixed", 300 + k, h, w, 3) for k, (w, h, _, _) in enumerate(SCENE)]
    assert all(np.isnan(s).any() and np.isinf(s).any() and PX.is_subnormal(s).any() for s in srcs)
    maps = scene_maps(interp, True)
    dmaps = [dev_map(W, xy, frac, interp) for xy, frac in maps]
    ts = [torch.from_numpy(s).cuda() for s in srcs]
    for blend, F in BLENDS:
        for mode in MODES:
            out = torch.from_numpy(FD.canvas((DSIZE[1], DSIZE[0], 3))).cuda()
            W.remap_stitch(ts, dmaps, blend=blend, feather=F, border_value=PX.BORDER[:3], out=out, border_mode=mode)
            torch.cuda.synchronize()
            exp, count = SM.stitch(srcs, maps, interp, SM.FEATHER if blend == "feather" else SM.OVER, F, mode, PX.BORDER[:3], FD.canvas((DSIZE[1], DSIZE[0], 3)))
            computed = ((count >= 1) if interp == LINEAR else np.zeros(count.shape, bool)) | ((count >= 2) & (blend == "feather"))
            FD.compare(out.cpu().numpy(), exp, computed, "%s F=%d mode %d" % (blend, F, mode))
            if mode == SM.TRANSPARENT:
                assert (PX.bits(out.cpu().numpy()[count == 0]) == FD.CANVAS_BITS).all() and (count == 0).any()
            if blend == "feather":
                many = exp[count >= 2]
                assert np.isnan(many).any() and not np.isnan(many).all()  # a multi-cover NaN gives some NaN
            if blend == "feather" and interp == NEAREST:  # a single cover keeps the source's bits: the camera's own remap
                for k, (xy, frac) in enumerate(maps):
                    mine = RR.written(xy, srcs[k].shape[1], srcs[k].shape[0], interp) & (count == 1)
                    assert mine.sum() >= 20
                    PX.same_float(out.cpu().numpy()[mine], RR.remap(srcs[k], xy, frac, interp, RR.TRANSPARENT)[mine], payload=True)
