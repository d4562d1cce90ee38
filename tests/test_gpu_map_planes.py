"""The map samplers that write channel planes on the GPU (bev_amd.warp.remap_to_planar -> bevwarp_remap_planes, remap_stitch_to_planar ->
bevwarp_stitch_maps_planes, remap_stitch_nv12_to_planar -> bevwarp_stitch_maps_nv12_planes, bev_amd.pipeline.SitePipeline): every element
against the numpy definition (tests/map_planes_ref.py: remap_nv12_ref.planes_f32 of the definitions of remap and of the stitches), by
bits, and against the two-launch routes each launch stands in for, device against device.  Every destination lies inside canaries.
There is no tolerance anywhere.  Run on the GPU box:  python -m pytest tests -m gpu -q"""
import functools

import numpy as np
import pytest
import torch

from oracle import warp_numpy as wn
from tests import lens_ref as LR
from tests import map_planes_ref as MP
from tests import nv12_ref as NR
from tests import pixels as PX
from tests import remap_nv12_ref as RN
from tests import remap_ref as RR
from tests import stitch_maps_ref as SM
from tests import workloads as wl
from tests.test_gpu_remap import _shifted_map
from tests.test_gpu_remap_nv12 import _planes_of, _random_map, _wrap
from tests.test_gpu_stitch_maps import SCENE, DSIZE, dev_map, scene_maps

pytestmark = pytest.mark.gpu

LINEAR, NEAREST = 1, 0
INF = float("inf")
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
BORDER = (7.0, 200.0, 31.0)   # a non-zero 8-bit border pixel, in the planes' channel order
SCALE, BIAS = (1 / 255.0, 0.017, 3.0), (-0.4, 0.25, 11.5)
MODES = RR.MODES[:5]          # the five modes that write every pixel
WIDTHS = (1, 3, 4, 5, 255, 256, 257)
LAYOUTS = ("wide", "half", "off")
SOURCES = ("bgr", "nv12", "nv12rgb")  # the stitch's three source kinds: B, G, R frames; NV12 frames as B, G, R; NV12 frames as R, G, B
# (source w, h, destination w, h, angle, zoom): 6 x 8 to 24 x 32 px sources, destinations up to 20 x 12
SMALL = {"tall": (6, 8, 12, 7, 20.0, 0.8), "wide": (32, 24, 20, 12, 30.0, 2.2)}


@pytest.fixture(scope="module")
def W():
    from bev_amd import warp
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return warp


def _int(dtype):
    return torch.int32 if dtype == F32 else torch.int16


def _plane_out(shape, dtype, layout="wide"):
    """A canaried (3, dh, dw) / (B, 3, dh, dw) destination of `dtype`: (out, view, holder).
    wide  base and the three strides are multiples of the 4-element store (16 bytes of float32, 8 of a 16-bit type)
    half  the strides are, the base is half a store further: element stores from an aligned-looking layout
    off   the base is one element off and the row stride is no multiple of the store (pixels.canaried_out's align = 0)"""
    carrier = torch.float32 if dtype == F32 else torch.int16
    esz = 4 if dtype == F32 else 2
    if layout == "half":
        shape = tuple(shape)
        big, holder = PX.canaried_out(shape[:-1] + (shape[-1] + 2,), carrier, pad=6, align=4 * esz, planar=True)
        big.view(_int(dtype))[..., :2] = (0xC3C3C3C3 - (1 << 32)) if dtype == F32 else (0xC3C3 - (1 << 16))  # (the two elements before every row: canaries again)
        view = big[..., 2:]
        assert view.data_ptr() % (4 * esz) == 2 * esz and all((s * esz) % (4 * esz) == 0 for s in view.stride()[:-1])
    else:
        view, holder = PX.canaried_out(shape, carrier, pad=6, align=4 * esz if layout == "wide" else 0, planar=True)
    out = view.view(dtype)
    assert out.data_ptr() == view.data_ptr() and out.stride() == view.stride()
    return out, view, holder


def _same_bits(a, b, dtype, what):
    assert torch.equal(a.contiguous().view(_int(dtype)), b.contiguous().view(_int(dtype))), what


def _bgr(seed, sh, sw):
    return np.random.default_rng(9000 + seed).integers(0, 256, (sh, sw, 3), dtype=np.uint8)


def _run(W, src, m, mode, shape, dtype, layout="wide", scale=SCALE, bias=BIAS, border=BORDER, what=""):
    out, view, holder = _plane_out(shape, dtype, layout)
    assert W.remap_to_planar(src, m, scale=scale, bias=bias, border_mode=mode, border_value=border if mode == RR.CONSTANT else None, out=out, out_dtype=dtype) is out
    torch.cuda.synchronize()
    PX.assert_canaries_intact(holder, view, what)
    return out


@functools.lru_cache(maxsize=None)
def _small_maps(name, kind, interp):
    """(M, (xy, frac)) of a small geometry as remap_ref builds them: the pinhole chain, or lens A with its default r2_max."""
    sw, sh, dw, dh, angle, zoom = SMALL[name]
    M = wl.rotated_H(sw, sh, dw, dh, angle, zoom=zoom)
    if kind == "pinhole":
        return M, RR.build((dw, dh), wn.invert3x3(M), None, INF, interp)
    K = LR.camera_K(sw, sh)
    return M, RR.build((dw, dh), LR.ray_matrix(M, K), LR.lens12(K, LR.LENS_A), LR.lens_valid_r2(LR.LENS_A), interp)


# ---- 1. every single-camera instance, against the definition and against the launches it replaces ----

@pytest.mark.parametrize("name", sorted(SMALL))
@pytest.mark.parametrize("kind", ["pinhole", "A"])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_single_camera_instances(W, name, kind, interp):
    sw, sh, dw, dh, _, _ = SMALL[name]
    M, (xy, frac) = _small_maps(name, kind, interp)
    m = W.build_warp_map(M, (dw, dh), flags=interp, **({} if kind == "pinhole" else dict(K=LR.camera_K(sw, sh), dist_coeff=LR.LENS_A)))
    frame = _bgr(11, sh, sw)
    src = torch.from_numpy(frame).cuda()
    for mode in MODES:
        exp = MP.remap_planes(frame, xy, frac, interp, mode, SCALE, BIAS, BORDER)
        bv = BORDER if mode == RR.CONSTANT else None
        pixels = W.remap(src, m, border_mode=mode, border_value=bv)
        for dtype in (F32, F16, BF16):
            what = "%s %s mode %d interp %d %s" % (name, kind, mode, interp, dtype)
            out = _run(W, src, m, mode, (3, dh, dw), dtype, what=what)
            RN.assert_planes_equal(out, exp, dtype, what)
            two = W.warp_to_planar(pixels, np.eye(3), (dw, dh), scale=SCALE, bias=BIAS, flags=NEAREST, out_dtype=dtype)
            _same_bits(out, two, dtype, what + ", of the device's own remap")
            if kind == "pinhole" and mode == RR.CONSTANT:
                direct = W.warp_to_planar(src, M, (dw, dh), scale=SCALE, bias=BIAS, flags=interp, border_value=BORDER, out_dtype=dtype)
                _same_bits(out, direct, dtype, what + ", the matrix warp")
    # a float16 scale that overflows: 255 * 300 > 65520 is +inf, by the definition too; nothing is NaN
    big = (1.0, 300.0, 1.0)
    frame[0, 0] = (255, 255, 255)
    out = _run(W, torch.from_numpy(frame).cuda(), m, RR.REPLICATE, (3, dh, dw), F16, scale=big, bias=0.0)
    exp = MP.remap_planes(frame, xy, frac, interp, RR.REPLICATE, big, 0.0)
    RN.assert_planes_equal(out, exp, F16, "overflow")
    assert torch.isinf(out[1]).any() and not torch.isnan(out).any()
    # without `out`: (3, h, w) of a single frame, (B, 3, h, w) of a batch, float32 by default
    one = W.remap_to_planar(src, m)
    many = W.remap_to_planar(torch.stack([src, src]), m, out_dtype=BF16)
    assert tuple(one.shape) == (3, dh, dw) and one.dtype == F32 and tuple(many.shape) == (2, 3, dh, dw) and many.dtype == BF16
    RN.assert_planes_equal(one, MP.remap_planes(_bgr(11, sh, sw), xy, frac, interp, RR.CONSTANT, 1.0 / 255.0, 0.0), F32, "defaults")


# ---- 2. destination widths, heights and layouts ----

@pytest.mark.parametrize("dw", WIDTHS)
def test_widths_heights_and_layouts(W, dw):
    """The lane's 4 pixels and the 256-pixel tile row from both sides, heights 1 to 3, the three plane layouts for float32 and for a 16-bit
    type, the map planes aligned and as unaligned views, a row-padded source at an odd address."""
    sw, sh = 32, 18
    frame = _bgr(30, sh, sw)
    src = PX.padded_source(frame, 3, offset=3)
    for dh in (1, 2, 3):
        M = wl.rotated_H(sw, sh, dw, dh, 12.0, zoom=1.3)
        for interp in (NEAREST, LINEAR):
            m = W.build_warp_map(M, (dw, dh), flags=interp)
            xy, frac = RR.build((dw, dh), wn.invert3x3(M), None, INF, interp)
            maps = {"wide": m, "half": _shifted_map(W, m, 4, 2, 3)[0], "off": _shifted_map(W, m, 16, 8, 0)[0]}
            for mode in (RR.CONSTANT, RR.REFLECT):
                exp = MP.remap_planes(frame, xy, frac, interp, mode, SCALE, BIAS, BORDER)
                for dtype in (F32, F16 if dh != 2 else BF16):
                    for layout in LAYOUTS:
                        what = "%d x %d mode %d interp %d %s %s" % (dw, dh, mode, interp, dtype, layout)
                        out = _run(W, src, maps[layout], mode, (3, dh, dw), dtype, layout, what=what)
                        RN.assert_planes_equal(out, exp, dtype, what)


# ---- 3. batching ----

@pytest.mark.parametrize("per_frame", [False, True], ids=["shared", "per_frame"])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_batch_of_five(W, per_frame, interp):
    """Five different frames of a row-padded, offset source through a shared map and through a map per frame, on a small destination (one
    frame per item) and on an 8 x 16384 one: 4096 tiles per frame, so a shared map walks two frames per item with a short last group
    (tests/test_map_planes_cpu.py pins plan_remap)."""
    sw, sh, batch = 40, 24, 5
    frames = [_bgr(20 + b, sh, sw) for b in range(batch)]
    src = PX.padded_source(np.stack(frames), 3, offset=3)
    for (dw, dh), modes, dtype, layout in (((36, 20), (RR.CONSTANT, RR.REFLECT_101), F32, "off"), ((8, 16384), (RR.CONSTANT,), F16, "wide")):
        xy, frac = _random_map(np.random.default_rng(50 + dh), batch if per_frame else 1, dh, dw, sw, sh)
        m = _wrap(W, xy, frac, interp)
        for mode in modes:
            out = _run(W, src, m, mode, (batch, 3, dh, dw), dtype, layout)
            for b in range(batch):
                k = b if per_frame else 0
                RN.assert_planes_equal(out[b], MP.remap_planes(frames[b], xy[k], frac[k], interp, mode, SCALE, BIAS, BORDER), dtype,
                                       "frame %d of %d, mode %d, %d x %d, %d maps" % (b, batch, mode, dw, dh, m.n))


# ---- 4. tiny sources and hand-made maps ----

@pytest.mark.parametrize("src_wh", [(2, 2), (4, 2), (3, 5), (6, 4)])
def test_tiny_sources_and_hand_made_maps(W, src_wh):
    """Hand-made maps over the whole int16 range, the sentinel and 32767 included, on sources of 2 to 6 px -- the sizes at which a 6-byte
    pair load ends on a row's last byte.  A third of the entries lie inside in x with every lane's four side by side (pair lanes).  Each
    case runs with the padding around the source's rows filled with 0 and with 255: a load that strays past a row changes the answer."""
    sw, sh = src_wh
    dh, dw = 3, 261  # (two tile columns; few entries: the reference's index remap is a Python loop over the distinct indices)
    rng = np.random.default_rng(sw * 10 + sh)
    xy = rng.integers(-3 * max(sw, sh) - 2, 3 * max(sw, sh) + 3, (dh, dw, 2)).astype(np.int16)
    xy[1, 8:40] = rng.integers(-32768, 32768, (32, 2))
    xy[:, 88:176, 0] = rng.integers(0, sw - 1, (dh, 88))          # adjacent columns inside, rows anywhere near
    xy[:, 88:176, 1] = rng.integers(-2, sh + 2, (dh, 88))
    xy[2, 176:216, 0] = rng.integers(0, sw - 1, 40) + sw * rng.integers(-3, 4, 40)   # (WRAP: adjacent columns after the remap)
    xy[0, :8] = [[-32768, -32768], [32767, 32767], [-32768, 0], [0, -32768], [32767, 0], [0, 32767], [-1, -1], [0, 0]]
    frac = rng.integers(0, 65536, (dh, dw)).astype(np.uint16)
    frac[1, :4] = [0, 1023, 0xfc00, 0xffff]
    frame = _bgr(50, sh, sw)
    for interp in (NEAREST, LINEAR):
        m = _wrap(W, xy, frac, interp)
        for mode in MODES:
            exp = MP.remap_planes(frame, xy, frac, interp, mode, SCALE, BIAS, BORDER)
            for fill, dtype in ((0, F32), (255, F16)):
                out = _run(W, PX.padded_source(frame, fill, offset=1), m, mode, (3, dh, dw), dtype, "half")
                RN.assert_planes_equal(out, exp, dtype, "%s mode %d interp %d padding %d" % (src_wh, mode, interp, fill))
    # the sentinel under CONSTANT is the 8-bit border pixel, put through the plane stage
    exp = MP.remap_planes(frame, xy, frac, LINEAR, RR.CONSTANT, SCALE, BIAS, BORDER)
    want = (np.array(BORDER, np.float32) * np.array(SCALE, np.float32) + np.array(BIAS, np.float32)).astype(np.float32)
    assert exp[:, 0, 0].view(np.uint32).tolist() == want.view(np.uint32).tolist()


# ---- 5. the stitch ----

def _stitch_sources(source, k, batch=None):
    """Camera k of the scene as a source kind: (host frames, device tensors).  batch: that many different frames, stacked."""
    w, h = SCENE[k][0], SCENE[k][1]
    if source == "bgr":
        frames = [_bgr(100 + 10 * k + b, h, w) for b in range(batch or 1)]
        a = np.stack(frames)
        return frames, (PX.strided(a if batch else a[0], (9 + 2 * k,)) if k % 2 else torch.from_numpy(a if batch else a[0]).cuda(),)
    frames = [NR.frame("uniform", 100 + 10 * k + b, h, w) for b in range(batch or 1)]
    ys, uvs = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    return frames, _planes_of(ys if batch else ys[0], uvs if batch else uvs[0], "padded" if k % 2 else "joined")


def _stitch_run(W, source, devs, dmaps, blend, F, shape, dtype, layout="wide", what=""):
    out, view, holder = _plane_out(shape, dtype, layout)
    kw = dict(scale=SCALE, bias=BIAS, blend=blend, feather=F, border_value=BORDER, out=out, out_dtype=dtype)
    if source == "bgr":
        got = W.remap_stitch_to_planar([d[0] for d in devs], dmaps, **kw)
    else:
        got = W.remap_stitch_nv12_to_planar([d[0] for d in devs], [d[1] for d in devs], dmaps, rgb=source == "nv12rgb", **kw)
    assert got is out
    torch.cuda.synchronize()
    PX.assert_canaries_intact(holder, view, what)
    return out


def _stitch_exp(source, frames, maps, interp, blend, F):
    b = SM.FEATHER if blend == "feather" else SM.OVER
    if source == "bgr":
        return MP.stitch_planes(frames, maps, interp, SCALE, BIAS, b, F, BORDER)
    return MP.stitch_nv12_planes([f[0] for f in frames], [f[1] for f in frames], maps, interp, SCALE, BIAS, b, F, BORDER, rgb=source == "nv12rgb")


def _canvas(W, source, devs, dmaps, blend, F):
    """The 8-bit canvas of the device's own stitch: what the two-launch route keeps in memory."""
    if source == "bgr":
        return W.remap_stitch([d[0] for d in devs], dmaps, blend=blend, feather=F, border_value=BORDER)
    return W.remap_stitch_nv12([d[0] for d in devs], [d[1] for d in devs], dmaps, blend=blend, feather=F, border_value=BORDER, rgb=source == "nv12rgb")


@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
@pytest.mark.parametrize("lens", [False, True], ids=["pinhole", "lens"])
def test_stitch_scene(W, interp, lens):
    """1, 2 and 3 cameras of different sizes, "over" and "feather" with F = 1, 3 and 64, the three source kinds, float32 and 16-bit planes
    (every stitch instance): against the definition, and against warp_to_planar of the device's own remap_stitch / remap_stitch_nv12 canvas."""
    maps = scene_maps(interp, lens)
    dmaps = [dev_map(W, xy, frac, interp) for xy, frac in maps]
    dw, dh = DSIZE
    _, count = SM.stitch([np.zeros((h, w, 3), np.uint8) for w, h, _, _ in SCENE], maps, interp)
    assert all((count == n).sum() >= 20 for n in range(4))  # a region no camera covers, and overlaps of two and of three
    for source in SOURCES:
        cams = [_stitch_sources(source, k) for k in range(3)]
        for n in (1, 2, 3):
            frames, devs = [c[0][0] for c in cams[:n]], [c[1] for c in cams[:n]]
            for blend, F in (("over", 64), ("feather", 1), ("feather", 3), ("feather", 64)):
                exp = _stitch_exp(source, frames, maps[:n], interp, blend, F)
                canvas = _canvas(W, source, devs, dmaps[:n], blend, F)
                for dtype in (F32, F16 if n != 2 else BF16):
                    what = "%s, %d cameras, %s F=%d, interp %d, %s" % (source, n, blend, F, interp, dtype)
                    out = _stitch_run(W, source, devs, dmaps[:n], blend, F, (3, dh, dw), dtype, LAYOUTS[n - 1], what)
                    RN.assert_planes_equal(out, exp, dtype, what)
                    two = W.warp_to_planar(canvas, np.eye(3), (dw, dh), scale=SCALE, bias=BIAS, flags=NEAREST, out_dtype=dtype)
                    _same_bits(out, two, dtype, what + ", of the device's own canvas")
    # the pixel no camera covers is the 8-bit border pixel, put through the plane stage
    want = (np.array(BORDER, np.float32) * np.array(SCALE, np.float32) + np.array(BIAS, np.float32)).astype(np.float32)
    assert (exp[:, count == 0].view(np.uint32) == want.view(np.uint32)[:, None]).all()
    # without `out`: (3, h, w) of single frames, float32 by default
    got = W.remap_stitch_to_planar([c[1][0] for c in [_stitch_sources("bgr", k) for k in range(3)]], dmaps)
    assert tuple(got.shape) == (3, dh, dw) and got.dtype == F32


@pytest.mark.parametrize("source", SOURCES)
def test_stitch_eight_cameras(W, source):
    sizes = [(40, 24), (34, 28), (64, 18), (26, 26), (48, 22), (32, 34), (52, 20), (38, 28)]
    M = SCENE[0][2]
    dw, dh = DSIZE
    for interp in (NEAREST, LINEAR):
        maps = [RR.build(DSIZE, M + np.array([[0.01 * k, 0.005 * k, -1.5 * k], [0, 0.03 * k, -0.5 * k], [0, 0, 0]]), interp=interp) for k in range(8)]
        frames = [_bgr(200 + k, hh, ww) if source == "bgr" else NR.frame("uniform", 200 + k, hh, ww) for k, (ww, hh) in enumerate(sizes)]
        devs = [(torch.from_numpy(f).cuda(),) if source == "bgr" else _planes_of(f[0], f[1]) for f in frames]
        dmaps = [dev_map(W, xy, frac, interp) for xy, frac in maps]
        for (blend, F), dtype in ((("over", 64), F16), (("feather", 3), F32)):
            out = _stitch_run(W, source, devs, dmaps, blend, F, (3, dh, dw), dtype, "off")
            RN.assert_planes_equal(out, _stitch_exp(source, frames, maps, interp, blend, F), dtype, "%s, 8 cameras, %s, interp %d" % (source, blend, interp))
    _, count = SM.stitch([np.zeros((hh, ww, 3), np.uint8) for ww, hh in sizes], maps, interp)
    assert (count == 8).sum() >= 40 and (count == 0).sum() >= 40


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("blend,F", [("over", 64), ("feather", 3)])
def test_stitch_batch_of_two_with_mixed_map_planes(W, source, blend, F):
    """A batch of 2 with per-camera shared maps: camera 0's in aligned planes (lane-wide loads), camera 1's in row-padded planes at
    addresses that are no multiple of 16 / 8 (loads entry by entry, in the same launch), camera 2's a lens map."""
    interp = LINEAR
    pin, lens = scene_maps(interp, False), scene_maps(interp, True)
    maps = [pin[0], pin[1], lens[2]]
    d0, d1, d2 = dev_map(W, *maps[0], interp), _shifted_map(W, dev_map(W, *maps[1], interp), 4, 2, 3)[0], dev_map(W, *maps[2], interp)
    assert d0.xy.data_ptr() % 16 == 0 and d1.xy.data_ptr() % 16 == 4 and d1.frac.data_ptr() % 8 == 2 and d0.n == d1.n == d2.n == 1
    cams = [_stitch_sources(source, k, batch=2) for k in range(3)]
    dw, dh = DSIZE
    for dtype, layout in ((F32, "wide"), (BF16, "half")):
        out = _stitch_run(W, source, [c[1] for c in cams], [d0, d1, d2], blend, F, (2, 3, dh, dw), dtype, layout)
        for b in range(2):
            RN.assert_planes_equal(out[b], _stitch_exp(source, [c[0][b] for c in cams], maps, interp, blend, F), dtype, "%s frame %d %s %s" % (source, b, blend, layout))
    assert not torch.equal(out[0], out[1])


# ---- 6. the site's pipeline ----

def _site_case(W, src_format, dst_format, download):
    """Five sets of frames from two cameras of different sizes through a ring of two slots (it wraps twice): each result equals the
    resident call's on the same set, by bits."""
    from bev_amd.pipeline import SitePipeline
    interp, rgb = LINEAR, src_format == "nv12" and dst_format != "nv12"
    dw, dh = DSIZE
    maps = scene_maps(interp, True)[:2]
    dmaps = [dev_map(W, xy, frac, interp) for xy, frac in maps]
    hws = [(SCENE[k][1], SCENE[k][0]) for k in range(2)]
    sets = [[NR.frame("uniform", 300 + 10 * i + k, h, w) for k, (h, w) in enumerate(hws)] for i in range(5)]
    inputs = [[NR.join(y, uv) if src_format == "nv12" else NR.nv12_to_bgr(y, uv) for y, uv in s] for s in sets]
    kw = dict(blend="feather", feather=3, border_value=BORDER)
    with SitePipeline(hws, dmaps, DSIZE, depth=2, src_format=src_format, dst_format=dst_format, scale=SCALE, bias=BIAS, plane_dtype=F16, rgb=rgb, download=download,
                      **kw) as pipe:
        assert tuple(pipe.d_out[0].shape) == {"bgr": (dh, dw, 3), "nv12": (dh * 3 // 2, dw), "planes": (3, dh, dw)}[dst_format]
        assert [tuple(b.shape) for b in pipe.next_inputs()] == [((h * 3 // 2, w) if src_format == "nv12" else (h, w, 3)) for h, w in hws]
        outs = [res.cpu().clone() if isinstance(res, torch.Tensor) else torch.from_numpy(np.array(res)) for res in pipe.run(inputs)]
    assert len(outs) == 5
    for i, got in enumerate(outs):
        ts = [torch.from_numpy(a).cuda() for a in inputs[i]]
        if src_format == "nv12":
            ys, uvs = zip(*[W.split_nv12(t) for t in ts])
            if dst_format == "nv12":
                want = W.remap_stitch_nv12_to_nv12(ys, uvs, dmaps, **kw)
            elif dst_format == "planes":
                want = W.remap_stitch_nv12_to_planar(ys, uvs, dmaps, scale=SCALE, bias=BIAS, rgb=rgb, out_dtype=F16, **kw)
            else:
                want = W.remap_stitch_nv12(ys, uvs, dmaps, rgb=rgb, **kw)
        elif dst_format == "nv12":
            want = W.remap_stitch_to_nv12(ts, dmaps, **kw)
        elif dst_format == "planes":
            want = W.remap_stitch_to_planar(ts, dmaps, scale=SCALE, bias=BIAS, out_dtype=F16, **kw)
        else:
            want = W.remap_stitch(ts, dmaps, **kw)
        torch.cuda.synchronize()
        want = want.cpu()
        assert got.dtype == want.dtype and got.shape == want.shape
        bits = torch.int16 if got.dtype == F16 else torch.uint8
        assert torch.equal(got.view(bits), want.view(bits)), "set %d" % i
    assert not torch.equal(outs[0].view(torch.uint8), outs[1].view(torch.uint8))
    if dst_format == "planes":  # ... and the definition, once
        s = sets[4]
        if src_format == "nv12":
            exp = MP.stitch_nv12_planes([f[0] for f in s], [f[1] for f in s], maps, interp, SCALE, BIAS, SM.FEATHER, 3, BORDER, rgb=rgb)
        else:
            exp = MP.stitch_planes(inputs[4], maps, interp, SCALE, BIAS, SM.FEATHER, 3, BORDER)
        RN.assert_planes_equal(outs[4], exp, F16, "set 4, the definition")


@pytest.mark.parametrize("src_format", ["bgr", "nv12"])
@pytest.mark.parametrize("dst_format", ["bgr", "nv12", "planes"])
def test_site_pipeline(W, src_format, dst_format):
    _site_case(W, src_format, dst_format, True)


def test_site_pipeline_leaves_results_on_the_device(W):
    _site_case(W, "nv12", "planes", False)


def test_site_pipeline_commit_without_next_inputs(W):
    """commit() needs no next_inputs() call before it: five sets written straight into the pinned slots of a ring of two, two of them in
    flight at a time; a slot is reused only after its result has been taken, and each result is the resident call's."""
    from bev_amd.pipeline import SitePipeline
    maps = scene_maps(LINEAR, False)[:2]
    dmaps = [dev_map(W, xy, frac, LINEAR) for xy, frac in maps]
    hws = [(SCENE[k][1], SCENE[k][0]) for k in range(2)]
    sets = [[_bgr(400 + 10 * i + k, h, w) for k, (h, w) in enumerate(hws)] for i in range(5)]
    outs = []
    with SitePipeline(hws, dmaps, DSIZE, depth=2, border_value=BORDER) as pipe:
        for i, frames in enumerate(sets):
            if pipe.ready() == 2:
                outs.append(np.array(pipe.result()))
            for t, f in zip(pipe.h_in[i % 2], frames):
                t.numpy()[...] = f
            pipe.commit()
        with pytest.raises(RuntimeError, match="none has been taken"):
            pipe.commit()
        while pipe.ready():
            outs.append(np.array(pipe.result()))
    for i, (got, frames) in enumerate(zip(outs, sets)):
        want = W.remap_stitch([torch.from_numpy(f).cuda() for f in frames], dmaps, border_value=BORDER)
        np.testing.assert_array_equal(got, want.cpu().numpy(), err_msg="set %d" % i)
    assert len(outs) == 5
