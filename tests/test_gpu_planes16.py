"""float16 / bfloat16 channel planes in one pass (bevwarp_warp_planes, warp_to_planar(out_dtype=...), FramePipeline(plane_dtype=...)) on
the GPU, against the CPU oracle: the float32 planes the planar tests build, converted by tests/planes16_ref.py (whose two conversions
tests/test_planes16_cpu.py holds against torch's) and compared by their 16 bits, a NaN for a NaN.

What the cases exercise in warp_rows_planes16 (rows_store.inc): the 8-byte store per channel of 8-bit sources (row-path tiles, ragged
tiles, the short-image path, the patch lane layout of turned footprints, both aligned-window instances), the 2-byte stores of float
sources, the element stores of layouts that lose the wide store, and the two conversion instructions at every rounding boundary.
Run on the GPU box:  python -m pytest tests -m gpu -q"""
import ctypes

import numpy as np
import pytest
import torch

from tests import pixels as PX
from tests import planes16_ref as R
from tests import workloads as wl

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]  # (numpy's: the references compute 0 * Inf on purpose)

DTYPES = (torch.float16, torch.bfloat16)
SW, SH = 640, 360
MEAN, STD = np.array([0.485, 0.456, 0.406, 0.5]), np.array([0.229, 0.224, 0.225, 0.25])
BORDER = [9, 60, 200, 17]


@pytest.fixture(scope="module")
def W():
    from bev_amd import warp
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return warp


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def imagenet(c, pixel_scale=255.0):
    return 1.0 / (pixel_scale * STD[:c]), -MEAN[:c] / STD[:c]


def check(got, exp_f32, dtype, what):
    assert got.dtype == dtype and tuple(got.shape) == exp_f32.shape, (got.dtype, got.shape, exp_f32.shape)
    R.assert_same16(R.gpu_bits(got), R.to_bits(exp_f32, dtype), dtype, "%s %s" % (what, R.kind_of(dtype)))


def both_types(W, src, M, dsize, interp, scale, bias, what, border_value=None):
    """warp_to_planar of one frame (numpy) in both 16-bit types against the converted float32 planes of the oracle."""
    exp = R.planes_f32(src, M, dsize, interp, scale, bias, border_value)
    t = cuda(src)
    for dtype in DTYPES:
        got = W.warp_to_planar(t, M, dsize, scale=scale, bias=bias, flags=interp, border_value=border_value, out_dtype=dtype)
        check(got, exp, dtype, what)


# ---- 1: uint8 parity --------------------------------------------------------------------------------------------------------------
U8_SHAPES = [(3, 512, 80), (3, 300, 37), (1, 256, 32), (4, 512, 16), (2, 70, 5)]


@pytest.mark.parametrize("interp", [0, 1])
@pytest.mark.parametrize("c,dw,dh", U8_SHAPES)
def test_uint8_parity(W, interp, c, dw, dh):
    """Row-path tiles, ragged tiles and the short-image path; interior, edge-cut and outside tiles (synth_brno_H); per-channel ImageNet
    scale and bias, a non-zero border value, a batch of 3 into a preallocated `out`."""
    M = wl.synth_brno_H(SW, SH, dw, dh)
    scale, bias = imagenet(c)
    frames = np.stack([wl.frame(11 + i, SH, SW, np.uint8, c) for i in range(3)])
    exp = np.stack([R.planes_f32(f, M, (dw, dh), interp, scale, bias, BORDER[:c]) for f in frames])
    t = cuda(frames)
    for dtype in DTYPES:
        out = torch.full((3, c, dh, dw), 77, dtype=dtype, device="cuda")
        assert W.warp_to_planar(t, M, (dw, dh), scale=scale, bias=bias, flags=interp, border_value=BORDER[:c], out=out, out_dtype=dtype) is out
        check(out, exp, dtype, "c=%d %dx%d interp %d" % (c, dw, dh, interp))
    got = W.warp_to_planar(t[0], M, (dw, dh), scale=scale, bias=bias, flags=interp, border_value=BORDER[:c], out_dtype=torch.float16)
    assert got.shape == (c, dh, dw)  # (a single frame comes back without the batch axis)
    check(got, exp[0], torch.float16, "single frame")


# ---- 2: turned footprints (the patch lane layout and its store indices) --------------------------------------------------------------
@pytest.mark.parametrize("np_dtype", [np.uint8, np.float32], ids=["uint8", "float32"])
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("deg,zoom,dw,dh", [(30.0, 2.4, 300, 77), (90.0, 0.8, 256, 48)])
def test_turned_footprints(W, deg, zoom, dw, dh, c, np_dtype):
    M = wl.rotated_H(SW, SH, dw, dh, deg, zoom)
    src = wl.frame(21, SH, SW, np_dtype, c)
    scale, bias = imagenet(c, 255.0 if np_dtype == np.uint8 else 1.0)
    for interp in (0, 1):
        both_types(W, src, M, (dw, dh), interp, scale, bias, "rotated %g c=%d interp %d" % (deg, c, interp))


# ---- 3: both aligned-window instances (RS4 and not) ----------------------------------------------------------------------------------
@pytest.mark.parametrize("sw", [637, 640])
def test_both_aligned_window_instances(W, sw):
    """8-bit RGB bilinear: a source row stride that is no multiple of 4 bytes (637 * 3) and one that is (640 * 3)."""
    assert (sw * 3 % 4 == 0) == (sw == 640)
    scale, bias = imagenet(3)
    for M, (dw, dh) in ((wl.synth_brno_H(sw, SH, 512, 80), (512, 80)), (wl.keystone_H(sw, SH, 300, 37), (300, 37))):
        both_types(W, wl.frame(31, SH, sw, np.uint8, 3), M, (dw, dh), 1, scale, bias, "source width %d -> %dx%d" % (sw, dw, dh), BORDER[:3])


# ---- 4: float32 sources -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dw,dh", [(512, 80), (300, 37), (130, 16), (70, 5)])
@pytest.mark.parametrize("name", ["keystone", "brno"])
def test_float32_sources(W, name, dw, dh):
    """keystone: frames in [0, 1) with ImageNet constants; brno: "mixed" frames (tests/pixels.py: both signs, every binade, subnormals,
    infinities, NaNs), whose planes overflow float16, fall into its subnormals and below them."""
    M = (wl.keystone_H if name == "keystone" else wl.synth_brno_H)(SW, SH, dw, dh)
    for c in (1, 2, 3, 4):
        if name == "keystone":
            src, (scale, bias) = wl.frame(41 + c, SH, SW, np.float32, c), imagenet(c, 1.0)
        else:
            src, scale, bias = PX.float_frame("mixed", 400 + c, SH, SW, c), np.linspace(0.5, 2.0, c), np.linspace(-1.0, 1.0, c)
        for interp in (0, 1):
            both_types(W, src, M, (dw, dh), interp, scale, bias, "%s c=%d %dx%d interp %d" % (name, c, dw, dh, interp))


# ---- 5: rounding boundaries on the device -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 3])
def test_rounding_boundaries_on_the_device(W, c):
    """An identity warp (nearest: the pixels' bits are copied) of a 16 x 128 frame that holds the boundary list of the CPU test, padded with
    seeded random bit patterns; scale 1, bias 0.  With a bias of -0.0 the float32 value IS the input element (x * 1 + -0.0 == x, signed
    zeros included), so every output element is the 16-bit conversion of the input element; with +0.0 the one difference is that -0
    becomes +0 before it is converted, as in the float32 planes."""
    rng = np.random.default_rng(160 + c)
    n = 16 * 128 * c
    pats = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    pats[:len(R.BOUNDARY_BITS)] = R.BOUNDARY_BITS
    if c == 3:  # every boundary value in every channel
        pats[:3 * len(R.BOUNDARY_BITS)] = np.repeat(R.BOUNDARY_BITS, 3)
    src = pats.view(np.float32).reshape(16, 128, c)
    t = cuda(src)
    x = np.ascontiguousarray(src.transpose(2, 0, 1))
    for dtype in DTYPES:
        got = W.warp_to_planar(t, np.eye(3), (128, 16), scale=1.0, bias=-0.0, flags=0, out_dtype=dtype)
        check(got, x, dtype, "bias -0.0, c=%d" % c)
        got = W.warp_to_planar(t, np.eye(3), (128, 16), scale=1.0, bias=0.0, flags=0, out_dtype=dtype)
        with np.errstate(all="ignore"):
            v = x * np.float32(1.0) + np.float32(0.0)
        check(got, v, dtype, "bias 0.0, c=%d" % c)
        neg0 = x.view(np.uint32) == 0x80000000
        assert neg0.any() and (R.gpu_bits(got)[neg0] == 0).all()
        got_bits = R.gpu_bits(W.warp_to_planar(t, np.eye(3), (128, 16), scale=1.0, bias=-0.0, flags=0, out_dtype=dtype))
        assert (got_bits[neg0] == 0x8000).all()  # -0 stays -0


# ---- 6: destination layouts ------------------------------------------------------------------------------------------------------------
def layout(kind, shape):
    """A canaried destination of 2-byte elements: "16" -- base and strides multiples of 16 bytes; "8" -- multiples of 8 and the row stride
    of 16 not; "2" -- the row stride is 2 mod 8 and the base is one element off: no wide store."""
    want = {"16": lambda v: v.stride(2) * 2 % 16 == 0, "8": lambda v: v.stride(2) * 2 % 16 == 8, "2": lambda v: v.stride(2) * 2 % 8 == 2}[kind]
    for pad in range(16, 64, 2):
        view, holder = PX.canaried_out(shape, torch.int16, pad, align={"16": 16, "8": 8, "2": 0}[kind], planar=True)
        if want(view):
            break
    assert want(view), (kind, view.stride())
    strides = [s * 2 for s in view.stride()[:3]]
    if kind == "2":
        assert view.data_ptr() % 8 != 0 and view.data_ptr() % 2 == 0
    else:
        assert all(v % int(kind) == 0 for v in strides + [view.data_ptr()])
    return view, holder


@pytest.mark.parametrize("np_dtype", [np.uint8, np.float32], ids=["uint8", "float32"])
@pytest.mark.parametrize("dw", [301, 512])
def test_destination_layouts(W, dw, np_dtype):
    """Canaried planes, batch 2, c = 3, 9 rows: equal results with the wide stores (two alignments) and without them, nothing written
    beside the view."""
    dh, c, B = 9, 3, 2
    M = wl.keystone_H(SW, SH, dw, dh)
    frames = np.stack([wl.frame(57 + i, SH, SW, np_dtype, c) for i in range(B)])
    scale, bias = imagenet(c, 255.0 if np_dtype == np.uint8 else 1.0)
    exp = np.stack([R.planes_f32(f, M, (dw, dh), 1, scale, bias) for f in frames])
    t = cuda(frames)
    for dtype in DTYPES:
        results = []
        for kind in ("16", "8", "2"):
            what = "dw %d layout %s" % (dw, kind)
            view, holder = layout(kind, (B, c, dh, dw))
            out = view.view(dtype)
            assert out.data_ptr() == view.data_ptr() and out.stride() == view.stride()
            assert W.warp_to_planar(t, M, (dw, dh), scale=scale, bias=bias, flags=1, out=out, out_dtype=dtype) is out
            torch.cuda.synchronize()
            PX.assert_canaries_intact(holder, view, what)
            check(out, exp, dtype, what)
            results.append(R.gpu_bits(out))
        assert np.array_equal(results[0], results[1]) and np.array_equal(results[0], results[2])


# ---- 7: the frame pipeline ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=R.kind_of)
@pytest.mark.parametrize("download", [True, False])
def test_frame_pipeline_plane_dtype(W, download, dtype):
    from bev_amd.pipeline import FramePipeline
    dw, dh = 256, 96
    M = wl.synth_brno_H(SW, SH, dw, dh)
    scale, bias = imagenet(3)
    frames = [wl.frame(60 + i, SH, SW, np.uint8) for i in range(2)]
    with FramePipeline((SH, SW), 3, M, (dw, dh), depth=2, planar=True, scale=scale, bias=bias, download=download, plane_dtype=dtype) as pipe:
        for f in frames:
            pipe.submit(f)
            r = pipe.result()
            ref = W.warp_to_planar(cuda(f), M, (dw, dh), scale=scale, bias=bias, out_dtype=dtype)
            if download:
                r = torch.from_numpy(r) if isinstance(r, np.ndarray) else r  # (numpy has no bfloat16: such a host slot is a torch tensor)
                assert not r.is_cuda
            else:
                assert r.is_cuda
            assert r.dtype == dtype and r.shape == (3, dh, dw)
            assert np.array_equal(R.gpu_bits(r), R.gpu_bits(ref))
            check(ref, R.planes_f32(f, M, (dw, dh), 1, scale, bias), dtype, "pipeline reference")


# ---- 8: float32 planes through the new entry ---------------------------------------------------------------------------------------------
def test_float32_planes_through_the_new_entry(W):
    """bevwarp_warp_planes(..., BEVWARP_F32) is bevwarp_warp_planar: bit for bit warp_to_planar's default, on a case of test_uint8_parity."""
    from bev_amd import _lib
    c, dw, dh = 3, 300, 37
    M = wl.synth_brno_H(SW, SH, dw, dh)
    scale, bias = imagenet(c)
    frames = cuda(np.stack([wl.frame(11 + i, SH, SW, np.uint8, c) for i in range(3)]))
    ref = W.warp_to_planar(frames, M, (dw, dh), scale=scale, bias=bias, border_value=BORDER[:c])
    assert ref.dtype == torch.float32
    out = torch.full((3, c, dh, dw), 77, dtype=torch.float32, device="cuda")
    minv = W.device_inverse(M, frames.device)
    sc, bi, bv = (np.ascontiguousarray(v, dtype=np.float64) for v in (scale, bias, BORDER[:c]))
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    st = _lib.load().bevwarp_warp_planes(frames.data_ptr(), out.data_ptr(), 3, SH, SW, dh, dw, c, frames.stride(0), frames.stride(1), out.stride(0) * 4,
                                         out.stride(1) * 4, out.stride(2) * 4, minv.data_ptr(), 1, _lib.U8, 1, ptr(bv), ptr(sc), ptr(bi), _lib.F32,
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    PX.same_float(out.cpu().numpy(), np.stack([R.planes_f32(f, M, (dw, dh), 1, scale, bias, BORDER[:c]) for f in frames.cpu().numpy()]))
