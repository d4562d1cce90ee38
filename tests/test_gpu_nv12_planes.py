"""NV12 frames warped straight to normalised channel planes on the GPU (bev_amd.warp.warp_nv12_to_planar -> bevwarp_warp_nv12_planes):
every result is compared, on every element and by its bits, with the project's two existing references in sequence --

    bgr = nv12_ref.nv12_to_bgr(y, uv, rgb)                                       (the converted frame)
    exp = planes16_ref.planes_f32(bgr, M, dsize, interp, scale, bias, border)    (the oracle's warp of it, as float32 planes)

float32 planes by their 32 bits, float16 / bfloat16 planes through planes16_ref.to_bits / assert_same16.  |scale| and |bias| stay far
below 1e30, so no NaN arises from 8-bit values.
Run on the GPU box:  python -m pytest tests -m gpu -q"""
import functools

import numpy as np
import pytest
import torch

from tests import nv12_ref as R
from tests import pixels as PX
from tests import planes16_ref as P
from tests import workloads as wl
from tests.test_gpu_nv12 import planes as device_planes

pytestmark = pytest.mark.gpu

LINEAR, NEAREST = 1, 0
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = (F32, F16, BF16)
SW, SH = 640, 360
MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
IMAGENET = (1.0 / (255.0 * STD), -MEAN / STD)
BORDER = (10, 200, 77)
ids16 = lambda d: str(d).replace("torch.", "")  # noqa: E731


@pytest.fixture(scope="module")
def W():
    from bev_amd import warp
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return warp


def expected(y, uv, M, dsize, interp, scale, bias, border=None, rgb=False):
    """(3, dh, dw) float32, or (B, 3, dh, dw) for a batch (M: one matrix for all frames, or one per frame)."""
    if y.ndim == 3:
        M = np.asarray(M)
        return np.stack([expected(y[i], uv[i], M if M.ndim == 2 else M[i], dsize, interp, scale, bias, border, rgb) for i in range(len(y))])
    return P.planes_f32(R.nv12_to_bgr(y, uv, rgb), M, dsize, interp, scale, bias, border)


def same(got, exp_f32, dtype, what):
    """Every element by its bits: 32 of them for float32 planes, the converted 16 otherwise."""
    assert got.dtype == dtype and tuple(got.shape) == exp_f32.shape and exp_f32.dtype == np.float32, (what, got.dtype, got.shape, exp_f32.shape)
    if dtype == F32:
        g, e = got.contiguous().cpu().numpy().view(np.uint32), np.ascontiguousarray(exp_f32).view(np.uint32)
        if not np.array_equal(g, e):
            idx = tuple(int(v[0]) for v in np.nonzero(g != e))
            raise AssertionError("%s: %d of %d float32 elements differ by bits; first at %s: got 0x%08x, expected 0x%08x"
                                 % (what, int((g != e).sum()), g.size, idx, int(g[idx]), int(e[idx])))
    else:
        P.assert_same16(P.gpu_bits(got), P.to_bits(exp_f32, dtype), dtype, what)


def run(W, y, uv, M, dsize, interp, scale, bias, border=None, rgb=False, dtype=F32, layout="two", out=None):
    ty, tuv = device_planes(W, y, uv, layout)
    got = W.warp_nv12_to_planar(ty, tuv, M, dsize, scale=scale, bias=bias, flags=interp, border_value=border, out=out, rgb=rgb, out_dtype=dtype)
    torch.cuda.synchronize()
    return got


def check(W, y, uv, M, dsize, interp, scale, bias, border=None, rgb=False, dtype=F32, layout="two", what="", exp=None):
    got = run(W, y, uv, M, dsize, interp, scale, bias, border, rgb, dtype, layout)
    exp = expected(y, uv, M, dsize, interp, scale, bias, border, rgb) if exp is None else exp
    same(got, exp, dtype, "%s interp %d rgb %d layout %s src %s dsize %s" % (what, interp, rgb, layout, y.shape, dsize))
    return exp


# ---- 1. channel extraction over the whole conversion domain ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,rgb", [(F32, False), (F16, True)], ids=["float32-bgr", "float16-rgb"])
def test_every_yuv_value_lands_in_its_plane(W, dtype, rgb):
    """An identity nearest warp of the frame that holds every (Y, U, V) once; scale and bias differ per channel, so a value that lands in
    another channel's plane (or takes another channel's constants) shows."""
    y, uv = R.frame("domain", 0, 0, 0)
    scale, bias = (1.0, 0.5, 0.25), (0.0, 300.0, -700.0)
    exp = expected(y, uv, np.eye(3), (4096, 4096), NEAREST, scale, bias, rgb=rgb)
    assert exp.shape == (3, 4096, 4096)
    for c in range(3):
        assert exp[c].min() == np.float32(bias[c]) and exp[c].max() == np.float32(255 * scale[c] + bias[c])  # disjoint ranges: [0, 255], [300, 427.5], [-700, -636.25]
    same(run(W, y, uv, np.eye(3), (4096, 4096), NEAREST, scale, bias, rgb=rgb, dtype=dtype), exp, dtype, "domain")


# ---- 2. store paths -----------------------------------------------------------------------------------------------------------------------
WIDTHS, HEIGHTS = (1, 3, 4, 5, 255, 256, 257, 260), (1, 4, 5)


def holder_for(shape, dtype, align):
    """A canaried (B, 3, dh, dw) destination of `dtype` whose base and three outer strides are multiples of `align` bytes and -- below 16 --
    of no larger power of two in the row stride; the smallest alignment (the element size) puts the base one element off as well."""
    esz = 4 if dtype == F32 else 2
    carrier = torch.float32 if esz == 4 else torch.int16
    for pad in range(16, 80, esz):
        view, holder = PX.canaried_out(shape, carrier, pad, align=0 if align == esz else align, planar=True)
        rs = view.stride(2) * esz
        if rs % align == 0 and (align == 16 or rs % (2 * align) != 0):
            break
    else:
        raise AssertionError((shape, dtype, align))
    strides = [s * esz for s in view.stride()[:3]]
    if align == esz:
        assert view.data_ptr() % (4 * esz) != 0 and view.data_ptr() % esz == 0
    else:
        assert all(v % align == 0 for v in strides + [view.data_ptr()])
    out = view.view(dtype)
    assert out.data_ptr() == view.data_ptr() and out.stride() == view.stride()
    return out, view, holder


@functools.lru_cache(maxsize=None)
def store_case(interp, dw, dh):
    """Two frames, a keystone footprint moved 2.5 px to the right (the first columns of every row lie outside the frame, the rest of every
    row inside), the float32 planes everything is compared against."""
    M = np.array([[1, 0, 2.5], [0, 1, 0], [0, 0, 1.0]]) @ wl.keystone_H(SW, SH, 260, 5)
    frames = [R.frame("uniform", 40 + i, SH, SW) for i in range(2)]
    ys, uvs = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    exp = expected(ys, uvs, M, (dw, dh), interp, IMAGENET[0], IMAGENET[1], BORDER)
    exp.setflags(write=False)
    return M, ys, uvs, exp


@pytest.mark.parametrize("dtype", DTYPES, ids=ids16)
@pytest.mark.parametrize("interp", [NEAREST, LINEAR], ids=["nearest", "linear"])
def test_store_paths_keep_their_canaries(W, interp, dtype):
    """Widths around the lane's 4 pixels and the wave's 256, heights around the workgroup's 4 rows; destinations whose layout admits the
    4-element store (16 bytes; for the 16-bit types 8 bytes too) and whose layout does not (the element size): equal results, nothing
    written beside the view."""
    aligns = (16, 4) if dtype == F32 else (16, 8, 2)
    for dw in WIDTHS:
        for dh in HEIGHTS:
            M, ys, uvs, exp = store_case(interp, dw, dh)
            ty, tuv = device_planes(W, ys, uvs, "two")
            for align in aligns:
                what = "%s %dx%d align %d" % (ids16(dtype), dw, dh, align)
                out, view, holder = holder_for((2, 3, dh, dw), dtype, align)
                got = W.warp_nv12_to_planar(ty, tuv, M, (dw, dh), scale=IMAGENET[0], bias=IMAGENET[1], flags=interp, border_value=BORDER, out=out, out_dtype=dtype)
                torch.cuda.synchronize()
                assert got is out
                PX.assert_canaries_intact(holder, view, what)
                same(out, exp, dtype, what)


# ---- 3. geometries -------------------------------------------------------------------------------------------------------------------------
GEOMS = {"brno": lambda dw, dh: wl.synth_brno_H(SW, SH, dw, dh), "keystone": lambda dw, dh: wl.keystone_H(SW, SH, dw, dh),
         "rotated": lambda dw, dh: wl.rotated_H(SW, SH, dw, dh, 30.0, 2.4)}
SIZES = [(512, 80), (300, 37), (70, 5)]
GEOM_BORDER = (9, 60, 200)


@pytest.mark.parametrize("rgb", [False, True], ids=["bgr", "rgb"])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR], ids=["nearest", "linear"])
@pytest.mark.parametrize("geom", sorted(GEOMS))
def test_geometries(W, geom, interp, rgb):
    """ImageNet constants and a border value per channel; a batch of 3 with one matrix per frame and with one shared matrix, into a
    preallocated `out`; a single frame comes back without the batch axis.  The plane types take turns over the sizes and all three
    see every geometry."""
    frames = [R.frame("uniform", 11 + i, SH, SW) for i in range(3)]
    ys, uvs = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    ty, tuv = device_planes(W, ys, uvs, "two")
    scale, bias = IMAGENET
    for (dw, dh) in SIZES:
        M = GEOMS[geom](dw, dh)
        Ms = np.stack([wl.jitter_H(M, i) for i in range(3)])
        exp_own, exp_shared = expected(ys, uvs, Ms, (dw, dh), interp, scale, bias, GEOM_BORDER, rgb), expected(ys, uvs, M, (dw, dh), interp, scale, bias, GEOM_BORDER, rgb)
        assert not np.array_equal(exp_own[1], exp_shared[1]) and np.array_equal(exp_own[0], exp_shared[0])  # (jitter_H leaves frame 0 alone)
        for dtype in DTYPES:
            what = "%s %dx%d %s" % (geom, dw, dh, ids16(dtype))
            for mats, exp in ((Ms, exp_own), (M, exp_shared)):
                out = torch.full((3, 3, dh, dw), 77, dtype=dtype, device="cuda")
                got = W.warp_nv12_to_planar(ty, tuv, mats, (dw, dh), scale=scale, bias=bias, flags=interp, border_value=GEOM_BORDER, out=out, rgb=rgb, out_dtype=dtype)
                assert got is out
                same(out, exp, dtype, what + " matrices %s" % (np.asarray(mats).shape,))
            one = W.warp_nv12_to_planar(ty[0], tuv[0], M, (dw, dh), scale=scale, bias=bias, flags=interp, border_value=GEOM_BORDER, rgb=rgb, out_dtype=dtype)
            assert tuple(one.shape) == (3, dh, dw)
            same(one, exp_shared[0], dtype, what + " single frame")
        if geom == "brno" and dh >= 37:  # the frame's edge really crosses these destinations (the border value is in the result's channel order)
            cut = float((exp_shared[0][0] == np.float32(np.float32(GEOM_BORDER[0]) * np.float32(scale[0]) + np.float32(bias[0]))).mean())
            assert 0.05 <= cut <= 0.95, cut


# ---- 4. source layouts ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=ids16)
@pytest.mark.parametrize("interp", [NEAREST, LINEAR], ids=["nearest", "linear"])
def test_source_layouts(W, interp, dtype):
    M = wl.keystone_H(SW, SH, 120, 37)
    y, uv = R.frame("uniform", 21, SH, SW)
    scale, bias = IMAGENET
    exp = check(W, y, uv, M, (120, 37), interp, scale, bias, dtype=dtype, layout="two")
    for layout in ("single", "rowpad", "padded"):
        check(W, y, uv, M, (120, 37), interp, scale, bias, dtype=dtype, layout=layout, exp=exp)
    # a batch as single buffers through split_nv12, and as two allocations
    frames = [R.frame("uniform", 30 + i, SH, SW) for i in range(3)]
    ys, uvs = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    Ms = np.stack([wl.jitter_H(M, i) for i in range(3)])
    exp = expected(ys, uvs, Ms, (120, 37), interp, scale, bias)
    for layout in ("two", "single"):
        check(W, ys, uvs, Ms, (120, 37), interp, scale, bias, dtype=dtype, layout=layout, exp=exp, what="batch")


@pytest.mark.parametrize("interp", [NEAREST, LINEAR], ids=["nearest", "linear"])
def test_two_frames_two_matrices_every_stride_padded(W, interp):
    """What an entry point's argument filling can get wrong -- a swapped or dropped stride or pointer -- in the smallest shape that shows
    it: two frames with a matrix each, row, plane and frame strides of every image that all differ from the tight ones and from each other, a
    destination of two tile columns (260 > 256) and two tile rows (6 > 4)."""
    sw, sh, dw, dh = 12, 10, 260, 6
    frames = [R.frame("uniform", 70 + i, sh, sw) for i in range(2)]
    ys, uvs = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    H = wl.keystone_H(sw, sh, dw, dh)
    Ms = np.stack([wl.jitter_H(H, 1), wl.jitter_H(H, 2)])
    ty, tuv = PX.strided(ys, (9, 5)), PX.strided(uvs, (10, 6))   # (the pairs' strides stay even)
    out = PX.strided(np.full((2, 3, dh, dw), -7.5, np.float32), (24, 12, 4), fill=-3.0)
    strides = [ty.stride(0), ty.stride(1), tuv.stride(0), tuv.stride(1)] + [4 * v for v in out.stride()[:3]]   # bytes
    assert len(set(strides + [sh * sw, sw, sh // 2 * sw, 4 * 3 * dh * dw, 4 * dh * dw, 4 * dw])) == 13
    scale, bias = IMAGENET
    got = W.warp_nv12_to_planar(ty, tuv, Ms, (dw, dh), scale=scale, bias=bias, flags=interp, out=out, rgb=True, out_dtype=F32)
    torch.cuda.synchronize()
    assert got is out
    exp = expected(ys, uvs, Ms, (dw, dh), interp, scale, bias, rgb=True)
    same(out, exp, F32, "padded strides")
    assert not np.array_equal(exp[0], expected(ys[0], uvs[0], Ms[1], (dw, dh), interp, scale, bias, rgb=True))  # (the two matrices give different frames)


@pytest.mark.parametrize("rgb", [False, True], ids=["bgr", "rgb"])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR], ids=["nearest", "linear"])
def test_edges_inside_padded_allocations(W, interp, rgb):
    """Translations that put the tap pairs on (-1, 0) and on (w - 1, w) in x and in y, and a ring of pixels whose taps are all outside; both
    planes are row-padded inside allocations filled with 0xA5.  (The forward matrix of a translation inverts exactly.)"""
    w, h = 34, 18
    y, uv = R.frame("phase", 5, h, w)
    scale, bias = (0.5, 1.0, 2.0), (-3.0, 0.25, 100.0)
    for i, (tx, ty) in enumerate(((-1.0, -1.0), (-1 + 5 / 32.0, -1 + 27 / 32.0), (-2 + 31 / 32.0, -2 + 1 / 32.0), (-1 + 16 / 32.0, 0.0), (0.0, -1 + 16 / 32.0))):
        M = np.array([[1, 0, -tx], [0, 1, -ty], [0, 0, 1.0]])
        dtype = DTYPES[i % 3]
        exp = check(W, y, uv, M, (w + 4, h + 4), interp, scale, bias, BORDER, rgb, dtype, layout="padded", what="edge %r" % ((tx, ty),))
        # all taps outside: convert(float32(border[c]) * scale[c] + bias[c]), the border value as given in either order
        assert exp[:, h + 3, w + 3].tolist() == [BORDER[c] * scale[c] + bias[c] for c in range(3)]
        blended = (exp[0] != np.float32(BORDER[0] * scale[0] + bias[0])).sum()
        assert blended >= w * h // 2  # (the frame is there)


@pytest.mark.parametrize("rgb", [False, True], ids=["bgr", "rgb"])
def test_small_sources(W, rgb):
    scale, bias = IMAGENET
    for w, h in ((2, 2), (4, 2), (66, 34)):
        y, uv = R.frame("uniform", w + h, h, w)
        for interp in (NEAREST, LINEAR):
            for dtype in DTYPES:
                check(W, y, uv, np.eye(3), (w, h), interp, scale, bias, rgb=rgb, dtype=dtype, what="identity")
                M = np.array([[1.5, 0.1, 1.25], [-0.05, 1.25, 0.75], [0, 0, 1.0]])  # reaches over every edge of the frame
                check(W, y, uv, M, (2 * w + 3, 2 * h + 3), interp, scale, bias, BORDER, rgb, dtype, what="stretched")


# ---- 5. rounding on the device ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def level_frame():
    """32 x 32 pixels whose channel B holds every 8-bit value, one 2 x 2 block (one (U, V) pair) per value in row-major order: no grey
    ramp has them all (220 luma steps of 1.164 skip levels), so each value takes a (Y, U) that converts to it, V = 128.
    -> (y, uv, the 32 x 32 values of channel B)"""
    Y, U = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    table = R.convert(Y, U, 128)[..., 0].astype(int)
    y, uv = np.zeros((32, 32), np.uint8), np.full((16, 16, 2), 128, np.uint8)
    for v in range(256):
        hits = np.argwhere(table == v)
        assert len(hits), v
        yy, uu = hits[len(hits) // 2]
        i, j = divmod(v, 16)
        y[2 * i:2 * i + 2, 2 * j:2 * j + 2], uv[i, j, 0] = yy, uu
    lv = R.nv12_to_bgr(y, uv)[..., 0].astype(int)
    assert (lv[::2, ::2].ravel() == np.arange(256)).all() and (lv[1::2, 1::2] == lv[::2, ::2]).all()
    return y, uv, lv


def test_rounding_on_the_device(W):
    """From 8-bit values, in channel B of a BGR result (the other two channels are compared with the reference like everything else)."""
    y, uv, lv = level_frame()

    def planes(dtype, scale, bias):
        got = run(W, y, uv, np.eye(3), (32, 32), NEAREST, scale, bias, dtype=dtype)
        same(got, expected(y, uv, np.eye(3), (32, 32), NEAREST, scale, bias), dtype, "rounding %s scale %r bias %r" % (ids16(dtype), scale, bias))
        return got if dtype == F32 else P.gpu_bits(got).astype(int)[0]

    # float16 subnormals: v * 2^-25 is v / 2 units of 2^-24 -- odd v are ties and go to even.  A negative scale gives the sign, and with
    # a bias of -0 the product's -0 stays -0
    half = lv // 2
    want = np.where(lv % 2 == 0, half, half + (half & 1))
    assert want.max() == 128 and (want[lv == 1] == 0).all() and (want[lv == 3] == 2).all() and (want[lv == 5] == 2).all()
    assert (planes(F16, 2.0 ** -25, 0.0) == want).all()
    assert (planes(F16, -2.0 ** -25, -0.0) == (want | 0x8000)).all()
    assert (planes(F16, -2.0 ** -25, 0.0) == np.where(lv == 0, 0, want | 0x8000)).all()  # (-0 + +0 = +0, as in the float32 planes; -2^-25 rounds to -0)
    # float16 overflow: 255 * 257 = 65535 >= 65520 is inf; 254 * 257 = 65278 is finite, though rounded (to 65280)
    assert float(np.float16(65278.0)) == 65280.0
    for sign in (1.0, -1.0):
        bits = planes(F16, sign * 257.0, 0.0)
        assert (bits[lv == 255] == (0x7c00 | (0x8000 if sign < 0 else 0))).all() and ((bits & 0x7fff)[lv == 254] == int(np.float16(65278.0).view(np.uint16))).all()
        assert ((bits & 0x7fff)[lv < 255] < 0x7c00).all()
    # bfloat16: 256 ... 511 need 9 bits, bfloat16 has 8: every odd one is a tie and goes to the multiple of 4
    want = P.bf16_bits((lv + 256).astype(np.float32)).astype(int)
    back = (want.astype(np.uint32) << 16).view(np.float32)
    assert (back[lv % 2 == 0] == (lv + 256)[lv % 2 == 0]).all() and (back[lv % 2 == 1] % 4 == 0).all() and (np.abs(back - (lv + 256)) <= 1).all()
    assert (planes(BF16, 1.0, 256.0) == want).all()
    assert (planes(BF16, -1.0, -256.0) == (want | 0x8000)).all()
    # float32 planes of the same frame are exact
    f = planes(F32, 257.0, 0.0).cpu().numpy()
    assert (f[0] == lv * 257).all()


# ---- 6. the two-pass route on the device -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=ids16)
def test_equals_the_two_pass_route_on_the_device(W, dtype):
    """warp_perspective_nv12, then warp_to_planar with the identity matrix and nearest interpolation: what the one launch replaces."""
    dw, dh = 300, 37
    frames = [R.frame("uniform", 70 + i, SH, SW) for i in range(2)]
    ys, uvs = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    ty, tuv = device_planes(W, ys, uvs, "single")
    scale, bias = IMAGENET
    for M in (wl.synth_brno_H(SW, SH, dw, dh), wl.rotated_H(SW, SH, dw, dh, 30.0, 2.4)):
        for interp in (NEAREST, LINEAR):
            for rgb in (False, True):
                bev = W.warp_perspective_nv12(ty, tuv, M, (dw, dh), flags=interp, border_value=BORDER, rgb=rgb)
                two = W.warp_to_planar(bev, np.eye(3), (dw, dh), scale=scale, bias=bias, flags=NEAREST, out_dtype=dtype)
                one = W.warp_nv12_to_planar(ty, tuv, M, (dw, dh), scale=scale, bias=bias, flags=interp, border_value=BORDER, rgb=rgb, out_dtype=dtype)
                assert one.dtype == two.dtype == dtype and one.shape == two.shape == (2, 3, dh, dw)
                carrier = torch.int32 if dtype == F32 else torch.int16
                assert torch.equal(one.view(carrier), two.view(carrier)), (interp, rgb)
