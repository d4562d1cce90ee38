"""Per-camera exposure gains in the stitches through warp maps on the GPU (bev_amd.warp.remap_stitch*(..., gains=) -> the six
bevwarp_stitch_maps* entries under BEVWARP_STITCH_GAIN; bev_amd.pipeline.SitePipeline; bev_amd.exposure): every byte or element against
the numpy definition (tests/stitch_gain_ref.py: the plain definition of frames gained beforehand), and device against device against the
route the flag replaces -- bev_amd.exposure.apply_gains per camera, then the plain entry.  There is no tolerance anywhere.  Interleaved
canvases are pre-filled with 77, so a pixel a launch leaves unwritten does not pass as zero.  The flag adds no ABI symbol, so the table of
tests/launch_contexts.py does not ask for the gained kernels: CONTEXT_CASES below puts the six entries under gains on a side stream and
under graph replay with that module's checks (tests/test_stitch_gain_cpu.py holds the cases' preconditions on the host).
Run on the GPU box:  python -m pytest tests -m gpu -q"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import launch_contexts as LC
from tests import nv12_ref as NR
from tests import remap_nv12_ref as RN
from tests import remap_ref as RR
from tests import stitch_gain_ref as SG
from tests import stitch_maps_ref as SM
from tests.test_gpu_stitch_maps import DSIZE, SCENE, dev_map, scene_maps

pytestmark = pytest.mark.gpu

LINEAR, NEAREST = 1, 0
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
KINDS = ("maps", "nv12", "to_nv12", "nv12_to_nv12", "planes", "nv12_planes")
BLENDS = (("over", 64), ("feather", 1), ("feather", 3), ("feather", 64))
BORDER = (7.0, 200.0, 31.0)
SCALE, BIAS = (1 / 255.0, 0.017, 3.0), (-0.4, 0.25, 11.5)
# per camera and per channel: below and above 1, the identity, the largest gain, one that saturates most pixels
GAINS = [[1.25, 0.8, 1.0], [0.5, 2.0, 1023 / 256], [1.7, 1.0, 0.3], [0.996, 1.004, 3.0], [0.25, 0.75, 1.5], [1.1, 1.2, 1.3], [2.5, 0.1, 0.9], [1.0, 0.0, 1.0]]


@pytest.fixture(scope="module")
def W():
    from bev_amd import warp
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return warp


def _nv12_kind(kind):
    return kind.startswith("nv12")


def _host(kind, k, h, w, batch=None, seed=500):
    """Camera k's frames for an entry: (h, w, 3) uint8, or an NV12 (y, uv) pair; batch: a leading axis of that many frames."""
    rng = np.random.default_rng(seed + k)
    if _nv12_kind(kind):
        frames = [NR.frame("uniform", seed + 10 * k + b, h, w) for b in range(batch or 1)]
        return (np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])) if batch else frames[0]
    return rng.integers(0, 256, ((batch,) if batch else ()) + (h, w, 3), dtype=np.uint8)


def _scene_host(kind, n=3):
    return [_host(kind, k, h, w) for k, (w, h, _, _) in enumerate(SCENE[:n])]


def _bgr_of(kind, host, rgb):
    """The frames the sampler blends: the interleaved frames themselves, or the converted NV12 frames in the order `rgb` names."""
    return [NR.nv12_to_bgr(f[0], f[1], rgb) for f in host] if _nv12_kind(kind) else list(host)


def run(W, kind, host, dmaps, gains, blend, F, mode=SM.CONSTANT, rgb=False, dtype=F32, out=None):
    """One entry on the device: a numpy canvas (interleaved), a joined NV12 buffer as numpy, or the tensor of planes."""
    dw, dh = dmaps[0].dsize
    kw = dict(blend=blend, feather=F, border_value=BORDER, gains=gains)
    if _nv12_kind(kind):
        ys, uvs = [torch.from_numpy(np.ascontiguousarray(f[0])).cuda() for f in host], [torch.from_numpy(np.ascontiguousarray(f[1])).cuda() for f in host]
        lead = tuple(ys[0].shape[:-2])
    else:
        ts = [torch.from_numpy(np.ascontiguousarray(f)).cuda() if isinstance(f, np.ndarray) else f for f in host]
        lead = tuple(ts[0].shape[:-3])
    if kind in ("maps", "nv12"):
        if out is None:
            out = torch.full(lead + (dh, dw, 3), 77, dtype=torch.uint8, device="cuda")
        if kind == "maps":
            got = W.remap_stitch(ts, dmaps, out=out, border_mode=mode, **kw)
        else:
            got = W.remap_stitch_nv12(ys, uvs, dmaps, out=out, border_mode=mode, rgb=rgb, **kw)
        assert got is out
    elif kind == "to_nv12":
        got = W.remap_stitch_to_nv12(ts, dmaps, rgb=rgb, **kw)
    elif kind == "nv12_to_nv12":
        got = W.remap_stitch_nv12_to_nv12(ys, uvs, dmaps, **kw)
    elif kind == "planes":
        got = W.remap_stitch_to_planar(ts, dmaps, scale=SCALE, bias=BIAS, out_dtype=dtype, **kw)
    else:
        got = W.remap_stitch_nv12_to_planar(ys, uvs, dmaps, scale=SCALE, bias=BIAS, rgb=rgb, out_dtype=dtype, **kw)
    torch.cuda.synchronize()
    return got if "planes" in kind else got.cpu().numpy()


def route(W, kind, host, dmaps, G, blend, F, mode=SM.CONSTANT, rgb=False, dtype=F32):
    """What the flag replaces, on the device: bev_amd.exposure.apply_gains over every camera's frames (NV12: the converted frames), then
    the plain entry of interleaved frames."""
    from bev_amd import exposure
    plain = {"maps": "maps", "nv12": "maps", "to_nv12": "to_nv12", "nv12_to_nv12": "to_nv12", "planes": "planes", "nv12_planes": "planes"}[kind]
    gained = [exposure.apply_gains(torch.from_numpy(np.ascontiguousarray(f)).cuda(), g) for f, g in zip(_bgr_of(kind, host, rgb), G)]
    return run(W, plain, gained, dmaps, None, blend, F, mode, rgb and kind == "to_nv12", dtype)


def expect(kind, host, G, maps, interp, blend, F, mode=SM.CONSTANT, rgb=False):
    """The definition: a canvas, a joined NV12 buffer, or float32 planes; and the cover count."""
    b = SM.FEATHER if blend == "feather" else SM.OVER
    dh, dw = maps[0][0].shape[-3:-1]
    canvas, count = SG.stitch(_bgr_of(kind, host, rgb), G, maps, interp, b, F, mode, BORDER, np.full((dh, dw, 3), 77, np.uint8))
    if kind in ("maps", "nv12"):
        return canvas, count
    if kind == "to_nv12":
        return NR.join(*SG.stitch_to_nv12(host, G, maps, interp, b, F, BORDER, rgb)), count
    if kind == "nv12_to_nv12":
        return NR.join(*SG.stitch_nv12_to_nv12([f[0] for f in host], [f[1] for f in host], G, maps, interp, b, F, BORDER)), count
    if kind == "planes":
        return SG.stitch_planes(host, G, maps, interp, SCALE, BIAS, b, F, BORDER), count
    return SG.stitch_nv12_planes([f[0] for f in host], [f[1] for f in host], G, maps, interp, SCALE, BIAS, b, F, BORDER, rgb), count


def same(kind, got, exp, dtype=F32, what=""):
    if "planes" in kind:
        if isinstance(exp, torch.Tensor):  # device against device: the bits
            bits = torch.int32 if dtype == F32 else torch.int16
            assert torch.equal(got.view(bits), exp.view(bits)), what
        else:
            RN.assert_planes_equal(got, exp, dtype, what)
    else:
        np.testing.assert_array_equal(got, exp, err_msg=what)


def _modes(kind):
    return (SM.CONSTANT, SM.TRANSPARENT) if kind in ("maps", "nv12") else (SM.CONSTANT,)


# ---- 1. the scene: all six entries, both interpolations, OVER and FEATHER ----

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_scene_against_definition_and_route(W, kind, interp):
    """Three overlapping cameras (pixels covered 0, 1, 2 and 3 times) through lens maps, gains that differ per camera and per channel:
    every byte or element against the definition, and against apply_gains followed by the plain entry on the device."""
    maps = scene_maps(interp, True)
    dmaps = [dev_map(W, xy, frac, interp) for xy, frac in maps]
    host, gains = _scene_host(kind), GAINS[:3]
    G = SG.quantize(gains, 3)
    for i, (blend, F) in enumerate(BLENDS):
        rgb = bool(i & 1) and kind != "nv12_to_nv12"
        dtype = (F32, F16, F32, BF16)[i]
        for mode in _modes(kind):
            what = "%s interp %d %s F=%d mode %d rgb %s" % (kind, interp, blend, F, mode, rgb)
            got = run(W, kind, host, dmaps, gains, blend, F, mode, rgb, dtype)
            exp, count = expect(kind, host, G, maps, interp, blend, F, mode, rgb)
            same(kind, got, exp, dtype, what)
            same(kind, got, route(W, kind, host, dmaps, G, blend, F, mode, rgb, dtype), dtype, what + ", the route")
            if mode == SM.TRANSPARENT:  # the poisoned canvas survives exactly where no camera covers
                assert (got[count == 0] == 77).all() and (count == 0).sum() >= 20
    assert all((count == n).sum() >= 20 for n in range(4))
    plain, gained = (np.asarray(r.cpu() if isinstance(r, torch.Tensor) else r) for r in (run(W, kind, host, dmaps, g, "over", 64) for g in (None, gains)))
    assert not np.array_equal(plain, gained)  # (the gains are seen)


# ---- 2. identity, extremes, and `reserved` without the flag ----

@pytest.mark.parametrize("kind", KINDS)
def test_identity_gains_and_extremes(W, kind):
    interp = LINEAR
    maps = scene_maps(interp, True)
    dmaps = [dev_map(W, xy, frac, interp) for xy, frac in maps]
    host = _scene_host(kind)
    for blend, F in (("over", 64), ("feather", 3)):
        for mode in _modes(kind):
            plain = run(W, kind, host, dmaps, None, blend, F, mode)
            for ones in ([1.0, 1.0, 1.0], np.ones((3, 3)), [[1.0009, 0.9991, 1.0]] * 3):  # all quantise to 256: the flagless call, by bits
                same(kind, run(W, kind, host, dmaps, ones, blend, F, mode), plain, F32, "identity %s mode %d" % (blend, mode))
            # 0 and 1023: black, and the saturating end
            for gains in ([0.0, 1023 / 256, 1.0], [[0.0, 1023 / 256, 1.0], [1023 / 256, 0.0, 1023 / 256], [1 / 256, 1022 / 256, 0.0]]):
                G = SG.quantize(gains, 3)
                assert G.min() == 0 and G.max() == 1023
                got = run(W, kind, host, dmaps, gains, blend, F, mode)
                exp, count = expect(kind, host, G, maps, interp, blend, F, mode)
                same(kind, got, exp, F32, "extremes %s mode %d" % (blend, mode))
    if kind == "maps":  # camera 0 at gain 0 is black where it alone covers; the border pixel is not gained
        G = SG.quantize([0.0, 1.0, 1.0], 3)
        got = run(W, kind, host, dmaps, [0.0, 1.0, 1.0], "feather", 64)
        _, count = expect(kind, host, G, maps, interp, "feather", 64)
        only0 = RR.written(maps[0][0], SCENE[0][0], SCENE[0][1], interp) & (count == 1)
        assert only0.sum() >= 20 and (got[only0] == 0).all() and (got[count == 0] == np.array(BORDER, np.uint8)).all()


def test_reserved_is_not_looked_at_without_the_flag(W):
    """The C ABI called directly: a garbage `reserved` in every camera, no flag in `blend` -- the plain call's canvas, by bits."""
    from bev_amd import _lib
    interp = LINEAR
    maps = scene_maps(interp, False)
    dmaps = [dev_map(W, xy, frac, interp) for xy, frac in maps]
    host = _scene_host("maps")
    ts = [torch.from_numpy(f).cuda() for f in host]
    dw, dh = DSIZE
    lib = _lib.load()
    bv = np.array(BORDER, np.float64)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for blend, F in ((0, 0), (1, 3)):
        want = W.remap_stitch(ts, dmaps, blend="feather" if blend else "over", feather=3, border_value=BORDER)
        for garbage in (-1, 1 << 30, -(1 << 31), 0x12345678):
            cams = (_lib.MapCamera * 3)()
            for cam, t, m in zip(cams, ts, dmaps):
                W._fill_map_camera(cam, m, t[None])
                cam.reserved = garbage
            out = torch.full((dh, dw, 3), 77, dtype=torch.uint8, device="cuda")
            st = lib.bevwarp_stitch_maps(ctypes.addressof(cams), 3, out.data_ptr(), 1, dh, dw, 3, out.numel(), out.stride(0), 0, interp, blend, F, 0,
                                         bv.ctypes.data_as(ctypes.c_void_p), stream)
            assert st == 0
            torch.cuda.synchronize()
            assert torch.equal(out, want), (blend, garbage)
            if garbage >> 30:  # ... and under the flag such a word is refused before anything is launched
                assert lib.bevwarp_stitch_maps(ctypes.addressof(cams), 3, out.data_ptr(), 1, dh, dw, 3, out.numel(), out.stride(0), 0, interp, blend | 0x100, F, 0,
                                               bv.ctypes.data_as(ctypes.c_void_p), stream) == -1


# ---- 3. widths, layouts, batches, camera counts, narrow NV12 sources ----

@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_canvas_widths(W, interp):
    """1, 3, 4, 5 px and one tile of 256 px +- 1: ragged lanes at the row's end, in one and in two tile columns (NV12 canvases: the even ones)."""
    gains = GAINS[:2]
    G = SG.quantize(gains, 2)
    for dw in (1, 3, 4, 5, 255, 256, 257):
        T = np.array([[1.0, 0, 120.0 if dw <= 5 else 0.0], [0, 1, 0], [0, 0, 1]])  # (the narrow canvases lie where both cameras look)
        maps = [RR.build((dw, 6), SCENE[k][2] @ T, interp=interp) for k in (0, 1)]
        dmaps = [dev_map(W, xy, frac, interp) for xy, frac in maps]
        for kind in KINDS:
            if "to_nv12" in kind and dw % 2:
                continue
            host = _scene_host(kind, 2)
            for blend, F in (("over", 64), ("feather", 3)):
                for mode in _modes(kind):
                    got = run(W, kind, host, dmaps, gains, blend, F, mode, dtype=F16)
                    exp, count = expect(kind, host, G, maps, interp, blend, F, mode)
                    same(kind, got, exp, F16, "%s width %d %s mode %d" % (kind, dw, blend, mode))
            assert count[:, -1].max() >= 1, dw  # the last column is covered


@pytest.mark.parametrize("blend,F", [("over", 64), ("feather", 3)])
def test_unaligned_padded_destination_and_mixed_maps(W, blend, F):
    """A batch of 2 into a canvas that is a view at an odd address with padded rows, inside guard bytes (every pixel stored on its own);
    camera 0 with a map shared by the batch, camera 1 with a map per frame, camera 2 with a shared lens map."""
    interp, B, (dw, dh) = LINEAR, 2, DSIZE
    m0, m2 = scene_maps(interp, False)[0], scene_maps(interp, True)[2]
    m1 = [RR.build(DSIZE, SCENE[1][2] + np.array([[0.01 * i, 0, 1.5 * i], [0, -0.02 * i, 0.75 * i], [0, 0, 0]]), interp=interp) for i in range(B)]
    d1 = dev_map(W, np.stack([m[0] for m in m1]), np.stack([m[1] for m in m1]), interp)
    dmaps = [dev_map(W, *m0, interp), d1, dev_map(W, *m2, interp)]
    assert dmaps[0].n == 1 and d1.n == B
    gains = GAINS[:3]
    G = SG.quantize(gains, 3)
    for kind in ("maps", "nv12"):
        host = [_host(kind, k, h, w, batch=B) for k, (w, h, _, _) in enumerate(SCENE)]
        rs, fs = dw * 3 + 5, dh * (dw * 3 + 5) + 11
        holder = torch.full((B * fs + 2,), 0xC3, dtype=torch.uint8, device="cuda")
        out = torch.as_strided(holder, (B, dh, dw, 3), (fs, rs, 3, 1), 1)
        for mode in _modes(kind):
            out.fill_(77)
            got = run(W, kind, host, dmaps, gains, blend, F, mode, out=out)
            for b in range(B):
                frames = [(f[0][b], f[1][b]) if kind == "nv12" else f[b] for f in host]
                exp, count = expect(kind, frames, G, [m0, m1[b], m2], interp, blend, F, mode)
                np.testing.assert_array_equal(got[b], exp, err_msg="%s frame %d mode %d" % (kind, b, mode))
            assert not np.array_equal(got[0], got[1])
            written = torch.zeros_like(holder, dtype=torch.bool)
            torch.as_strided(written, (B, dh, dw, 3), (fs, rs, 3, 1), 1).fill_(True)
            assert (holder[~written] == 0xC3).all(), "a byte outside the view was written"
    # the plane and NV12 destinations of the same batch, per-frame maps included
    for kind in ("to_nv12", "nv12_planes"):
        host = [_host(kind, k, h, w, batch=B) for k, (w, h, _, _) in enumerate(SCENE)]
        got = run(W, kind, host, dmaps, gains, blend, F, dtype=F16)
        for b in range(B):
            frames = [(f[0][b], f[1][b]) if _nv12_kind(kind) else f[b] for f in host]
            exp, _ = expect(kind, frames, G, [m0, m1[b], m2], interp, blend, F)
            same(kind, got[b], exp, F16, "%s frame %d" % (kind, b))


@pytest.mark.parametrize("kind", KINDS)
def test_one_camera_and_eight(W, kind):
    interp = LINEAR
    sizes = [(40, 24), (34, 28), (64, 18), (26, 26), (48, 22), (32, 34), (52, 20), (38, 28)]
    M = SCENE[0][2]
    maps = [RR.build(DSIZE, M + np.array([[0.01 * k, 0.005 * k, -1.5 * k], [0, 0.03 * k, -0.5 * k], [0, 0, 0]]), interp=interp) for k in range(8)]
    dmaps = [dev_map(W, xy, frac, interp) for xy, frac in maps]
    host = [_host(kind, k, hh, ww, seed=700) for k, (ww, hh) in enumerate(sizes)]
    for n in (1, 8):
        G = SG.quantize(GAINS[:n], n)
        for blend, F in (("over", 64), ("feather", 64)):
            got = run(W, kind, host[:n], dmaps[:n], GAINS[:n], blend, F)
            exp, count = expect(kind, host[:n], G, maps[:n], interp, blend, F)
            same(kind, got, exp, F32, "%s, %d cameras, %s" % (kind, n, blend))
    assert (count == 8).sum() >= 40 and (count == 0).sum() >= 40


@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_nv12_sources_two_pixels_wide(W, interp):
    """Sources of 2 x 2 and 4 x 2 px (w x h) through hand-made maps: one pair per row, and the narrowest row that holds a window of pairs."""
    gains = [[1.5, 0.5, 1.0], [0.75, 3.0, 2.0]]
    G = SG.quantize(gains, 2)
    for w, h in ((2, 2), (4, 2)):
        y, uv = NR.frame("uniform", 40 + w, h, w)
        sx = np.array([[-1, 0, 1, 2, 3, 4, 0, w - 2, w - 1, 0]], np.int16)
        xy = np.stack([np.repeat(sx, 4, 0), np.repeat(np.array([[0], [1], [-1], [0]], np.int16), sx.shape[1], 1)], axis=-1)
        frac = (np.arange(40, dtype=np.uint16).reshape(4, 10) * 37 + 5) & 1023
        host = [(y, uv), (np.ascontiguousarray(y[::-1]), uv)]
        maps = [(xy, frac)] * 2
        dmaps = [dev_map(W, xy, frac, interp)] * 2
        for kind in ("nv12", "nv12_to_nv12", "nv12_planes"):
            for blend, F in (("over", 64), ("feather", 2)):
                for mode in _modes(kind):
                    got = run(W, kind, host, dmaps, gains, blend, F, mode, rgb=kind != "nv12_to_nv12")
                    exp, count = expect(kind, host, G, maps, interp, blend, F, mode, rgb=kind != "nv12_to_nv12")
                    same(kind, got, exp, F32, "%s %d x %d %s mode %d" % (kind, w, h, blend, mode))
        assert (count == 2).any() and (count == 0).any()


# ---- 4. SitePipeline ----

@pytest.mark.parametrize("src_format", ["bgr", "nv12"])
@pytest.mark.parametrize("dst_format", ["bgr", "nv12", "planes"])
def test_site_pipeline_gains_and_set_gains(W, src_format, dst_format):
    """Four sets through a ring of two slots: the first two with the constructor's gains, then set_gains between two committed sets -- the
    set already committed keeps its gains, the next one has the new ones -- then set_gains(None): each result is the resident call's."""
    from bev_amd.pipeline import SitePipeline
    interp, rgb = LINEAR, src_format == "nv12" and dst_format != "nv12"
    maps = scene_maps(interp, True)[:2]
    dmaps = [dev_map(W, xy, frac, interp) for xy, frac in maps]
    hws = [(SCENE[k][1], SCENE[k][0]) for k in range(2)]
    sets = [[NR.frame("uniform", 900 + 10 * i + k, h, w) for k, (h, w) in enumerate(hws)] for i in range(4)]
    inputs = [[NR.join(y, uv) if src_format == "nv12" else NR.nv12_to_bgr(y, uv) for y, uv in s] for s in sets]
    first, second = GAINS[:2], [[0.6, 1.9, 1.0], [3.5, 1.0, 0.2]]
    used = [first, first, second, None]
    kind = {("bgr", "bgr"): "maps", ("nv12", "bgr"): "nv12", ("bgr", "nv12"): "to_nv12", ("nv12", "nv12"): "nv12_to_nv12", ("bgr", "planes"): "planes",
            ("nv12", "planes"): "nv12_planes"}[(src_format, dst_format)]
    outs = []
    with SitePipeline(hws, dmaps, DSIZE, depth=2, blend="feather", feather=3, border_value=BORDER, src_format=src_format, dst_format=dst_format, scale=SCALE, bias=BIAS,
                      plane_dtype=F16, rgb=rgb, gains=first) as pipe:
        pipe.submit(inputs[0])
        outs.append(np.array(pipe.result()))
        pipe.submit(inputs[1])
        pipe.set_gains(second)            # set 1 is committed: it keeps the first gains
        pipe.submit(inputs[2])
        outs.append(np.array(pipe.result()))
        pipe.set_gains(None)
        pipe.submit(inputs[3])
        outs += [np.array(pipe.result()), np.array(pipe.result())]
        with pytest.raises(ValueError, match="3 gains for 2 cameras"):
            pipe.set_gains([1.0, 1.0, 1.0])
    for i, (got, gains) in enumerate(zip(outs, used)):
        host = [(y, uv) for y, uv in sets[i]] if src_format == "nv12" else inputs[i]
        want = run(W, kind, host, dmaps, gains, "feather", 3, rgb=rgb, dtype=F16)
        want = want.cpu().numpy() if isinstance(want, torch.Tensor) else want
        np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8), err_msg="set %d" % i)
    G = SG.quantize(second, 2)            # ... and the definition, once
    exp, _ = expect(kind, [(y, uv) for y, uv in sets[2]] if src_format == "nv12" else inputs[2], G, maps, interp, "feather", 3, rgb=rgb)
    if dst_format == "planes":
        RN.assert_planes_equal(torch.from_numpy(outs[2]), exp, F16, "set 2, the definition")
    else:
        np.testing.assert_array_equal(outs[2], exp)


# ---- 5. a captured graph takes the gains by value ----

def test_graph_replay_after_the_gain_array_was_overwritten(W):
    interp = LINEAR
    maps = scene_maps(interp, True)
    dmaps = [dev_map(W, xy, frac, interp) for xy, frac in maps]
    host = _scene_host("planes")
    ts = [torch.from_numpy(f).cuda() for f in host]
    dw, dh = DSIZE
    gains = np.array(GAINS[:3])
    G = SG.quantize(gains, 3)
    out = torch.zeros((3, dh, dw), dtype=F32, device="cuda")
    kw = dict(scale=SCALE, bias=BIAS, blend="feather", feather=3, border_value=BORDER, out=out)
    W.remap_stitch_to_planar(ts, dmaps, gains=gains, **kw)  # (the first launch loads the kernel: not under capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        W.remap_stitch_to_planar(ts, dmaps, gains=gains, **kw)
    gains[:] = 0.125                                        # the caller's array is its own again
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    exp, _ = expect("planes", host, G, maps, interp, "feather", 3)
    RN.assert_planes_equal(out, exp, F32, "replay")


# ---- 6. estimation ----

def test_overlap_stats_equal_the_numpy_twin(W):
    from bev_amd import exposure
    for interp in (NEAREST, LINEAR):
        maps = scene_maps(interp, True)
        dmaps = [dev_map(W, xy, frac, interp) for xy, frac in maps]
        host = [_host("maps", k, h, w, batch=2, seed=800) for k, (w, h, _, _) in enumerate(SCENE)]
        N, S = exposure.overlap_stats([torch.from_numpy(f).cuda() for f in host], dmaps)
        bevs = [np.stack([RR.remap(f[b], xy, frac, interp, RR.TRANSPARENT, canvas=np.zeros((DSIZE[1], DSIZE[0], 3), np.uint8)) for b in range(2)]) for f, (xy, frac) in zip(host, maps)]
        masks = [np.broadcast_to(RR.written(xy, w, h, interp), (2, DSIZE[1], DSIZE[0])) for (xy, _), (w, h, _, _) in zip(maps, SCENE)]
        Nn, Sn = SG.overlap_stats(bevs, masks)
        assert N.dtype == torch.int64 and S.dtype == torch.int64
        np.testing.assert_array_equal(N.numpy(), Nn)
        np.testing.assert_array_equal(S.numpy(), Sn)
        assert (Nn > 0).all()  # every pair of cameras overlaps
    single = exposure.overlap_stats([torch.from_numpy(f[0]).cuda() for f in host], dmaps)  # (H, W, 3) frames: one frame
    assert (single[0] * 2 == N).all()


def test_estimated_gains_close_the_step_between_two_cameras(W):
    """Two cameras that show constant colours, (120, 100, 80) and (60, 50, 40): with the estimated gains applied, the cameras differ by
    less in their overlap than the raw frames do, in every channel."""
    from bev_amd import exposure
    interp = LINEAR
    maps = scene_maps(interp, False)[:2]
    dmaps = [dev_map(W, xy, frac, interp) for xy, frac in maps]
    colours = [(120, 100, 80), (60, 50, 40)]
    host = [np.full((h, w, 3), c, np.uint8) for c, (w, h, _, _) in zip(colours, SCENE)]
    ts = [torch.from_numpy(f).cuda() for f in host]
    gains = exposure.estimate_gains(ts, dmaps)
    assert gains.shape == (2, 3) and (gains[0] < 1).all() and (gains[1] > 1).all()
    both = RR.written(maps[0][0], SCENE[0][0], SCENE[0][1], interp) & RR.written(maps[1][0], SCENE[1][0], SCENE[1][1], interp)
    assert both.sum() >= 100
    raw = [W.remap_stitch([t], [m], border_mode=W.BORDER_TRANSPARENT).cpu().numpy().astype(np.int64) for t, m in zip(ts, dmaps)]
    fixed = [W.remap_stitch([t], [m], border_mode=W.BORDER_TRANSPARENT, gains=gains[k:k + 1]).cpu().numpy().astype(np.int64) for k, (t, m) in enumerate(zip(ts, dmaps))]
    for c in range(3):
        before, after = np.abs(raw[0][both][:, c] - raw[1][both][:, c]), np.abs(fixed[0][both][:, c] - fixed[1][both][:, c])
        assert before.min() == before.max() == colours[0][c] - colours[1][c]
        assert after.max() < before.min(), (c, after.max(), before.min())
    # ... and the stitched canvas under "over" steps by less at the seam
    np.testing.assert_array_equal(W.remap_stitch(ts, dmaps, gains=gains).cpu().numpy()[both], fixed[1][both])


# ---- 7. launch contexts: the six gained entries on a side stream and under graph replay ----
# The gain words ride behind the plain kernel arguments through launch functions of their own (the three warp_stitch_gain*.hip units): a
# stream argument dropped there, or gains read from the caller's array at replay, shows here and nowhere else.
CONTEXT_GAINS = np.array([[1.25, 0.8, 0.6], [0.5, 2.0, 1.5]])  # per camera, per channel, none of them 1


def _context_cases():
    from bev_amd import warp as Wm
    G = SG.quantize(CONTEXT_GAINS, 2)
    MAPPED = LC._values(border=LC.BORDER, gains=CONTEXT_GAINS)
    MAPPED_PLANES = LC._values(border=LC.BORDER, scale=LC.SCALE, bias=LC.BIAS, gains=CONTEXT_GAINS)
    feather = (SM.FEATHER, LC.FEATHER)
    kw = lambda h: dict(blend="feather", feather=LC.FEATHER, border_value=h["border"], gains=h["gains"])  # noqa: E731
    cam_refs = lambda i: [LC.ref_maps(0)[i], LC.ref_maps(1)[i]]  # noqa: E731
    cam_frames = lambda which, i: [f[i] for f in LC.camera_frames(which)]  # noqa: E731
    per_frame = lambda one: [one(i) for i in range(LC.BATCH)]  # noqa: E731

    def cam_nv12(which, i):
        y0, y1, uv0, uv1 = LC.camera_nv12(which)
        return [y0[i], y1[i]], [uv0[i], uv1[i]]

    cover = functools.lru_cache(maxsize=None)(lambda: np.stack(per_frame(lambda i: SM.stitch(cam_frames("A", i), cam_refs(i), LINEAR)[1])))
    cases = []
    for no_out in (False, True):
        mode = SM.TRANSPARENT if no_out else SM.CONSTANT
        cases.append(LC.Case(
            "gains-remap_stitch" + "-no_out" * no_out, "bevwarp_stitch_maps", LC.camera_frames, MAPPED, LC.camera_maps, None if no_out else LC.PX,
            lambda t, r, h, o: [Wm.remap_stitch(t, r, out=LC._o(o), border_mode=LC._mode(o), **kw(h))],
            lambda which, hw, mode=mode: LC._stack(per_frame(lambda i: SG.stitch(cam_frames(which, i), G, cam_refs(i), LINEAR, *feather, mode, LC.BORDER)[0])),
            sliceable=(0, 1), written=(lambda: cover() > 0) if no_out else None, cover=cover))
    cases.append(LC.Case(
        "gains-remap_stitch_nv12", "bevwarp_stitch_maps_nv12", LC.camera_nv12, MAPPED, LC.camera_maps, LC.PX,
        lambda t, r, h, o: [Wm.remap_stitch_nv12(t[:2], t[2:], r, out=o[0], **kw(h))],
        lambda which, hw: LC._stack(per_frame(lambda i: SG.stitch_nv12(*cam_nv12(which, i), G, cam_refs(i), LINEAR, *feather, SM.CONSTANT, LC.BORDER)[0])), cover=cover))
    cases.append(LC.Case(
        "gains-remap_stitch_to_nv12", "bevwarp_stitch_maps_to_nv12", LC.camera_frames, MAPPED, LC.camera_maps, LC.NV12_OUT,
        lambda t, r, h, o: list(Wm.remap_stitch_to_nv12(t, r, out=tuple(o), **kw(h))),
        lambda which, hw: LC._stack_pairs(per_frame(lambda i: SG.stitch_to_nv12(cam_frames(which, i), G, cam_refs(i), LINEAR, *feather, LC.BORDER))),
        sliceable=(0, 1), cover=cover))
    cases.append(LC.Case(
        "gains-remap_stitch_nv12_to_nv12", "bevwarp_stitch_maps_nv12_to_nv12", LC.camera_nv12, MAPPED, LC.camera_maps, LC.NV12_OUT,
        lambda t, r, h, o: list(Wm.remap_stitch_nv12_to_nv12(t[:2], t[2:], r, out=tuple(o), **kw(h))),
        lambda which, hw: LC._stack_pairs(per_frame(lambda i: SG.stitch_nv12_to_nv12(*cam_nv12(which, i), G, cam_refs(i), LINEAR, *feather, LC.BORDER))), cover=cover))
    cases.append(LC.Case(
        "gains-remap_stitch_to_planar", "bevwarp_stitch_maps_planes", LC.camera_frames, MAPPED_PLANES, LC.camera_maps, LC.planes_out(F32),
        lambda t, r, h, o: [Wm.remap_stitch_to_planar(t, r, scale=h["scale"], bias=h["bias"], out=o[0], **kw(h))],
        lambda which, hw: LC._stack(per_frame(lambda i: SG.stitch_planes(cam_frames(which, i), G, cam_refs(i), LINEAR, LC.SCALE, LC.BIAS, *feather, LC.BORDER))),
        LC.same_planes(F32), sliceable=(0, 1), cover=cover))
    cases.append(LC.Case(
        "gains-remap_stitch_nv12_to_planar", "bevwarp_stitch_maps_nv12_planes", LC.camera_nv12, MAPPED_PLANES, LC.camera_maps, LC.planes_out(F32),
        lambda t, r, h, o: [Wm.remap_stitch_nv12_to_planar(t[:2], t[2:], r, scale=h["scale"], bias=h["bias"], out=o[0], **kw(h))],
        lambda which, hw: LC._stack(per_frame(lambda i: SG.stitch_nv12_planes(*cam_nv12(which, i), G, cam_refs(i), LINEAR, LC.SCALE, LC.BIAS, *feather, LC.BORDER))),
        LC.same_planes(F32), cover=cover))
    return cases


CONTEXT_CASES = _context_cases()
# the ungained case of tests/launch_contexts.py each of them stands beside
UNGAINED = {c.name: c.name[len("gains-"):] for c in CONTEXT_CASES}


@pytest.fixture(scope="module")
def delay():
    """(cycles, milliseconds) of the delay every side-stream case runs behind."""
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    cycles, ms = LC.sleep_cycles_for(50.0)
    print("torch.cuda._sleep(%d) takes %.1f ms" % (cycles, ms))
    assert ms >= 20.0, "the delay came out at %.2f ms: too short to enqueue a call behind" % ms
    return cycles, ms


@pytest.mark.parametrize("case", CONTEXT_CASES, ids=repr)
def test_side_stream_behind_a_delay(case, delay):
    cycles, ms = delay
    case.assert_preconditions()
    host_s = LC.check_side_stream(case, LC.Gpu("cuda:0", cycles))
    print("%s: delay %.1f ms, the call took %.3f ms on the host" % (case.name, ms, host_s * 1e3))


@pytest.mark.parametrize("case", CONTEXT_CASES, ids=repr)
def test_capture_and_replay(case):
    """The gains are one of the host arrays the replay check overwrites with NaNs after the capture."""
    case.assert_preconditions()
    assert "gains" in case.host("A")
    LC.check_replays(case, LC.Gpu("cuda:0"))


@pytest.mark.parametrize("case", [c for c in CONTEXT_CASES if c.sliceable], ids=repr)
def test_capture_and_replay_copied_source(case):
    case.assert_preconditions()
    LC.check_replays(case, LC.Gpu("cuda:0"), sliced=True)
