"""The map samplers that write NV12 on the GPU (bev_amd.warp.remap_to_nv12 -> bevwarp_remap_to_nv12, remap_nv12_to_nv12 ->
bevwarp_remap_nv12_to_nv12, remap_stitch_to_nv12 -> bevwarp_stitch_maps_to_nv12, remap_stitch_nv12_to_nv12 ->
bevwarp_stitch_maps_nv12_to_nv12, FramePipeline(warp_map=...) with NV12 slots): every byte of both planes against the numpy definition
(tests/remap_nv12_out_ref.py: nv12_out_ref.bgr_to_nv12 of the definitions of remap, remap_nv12 and the stitches), and against the
entries each launch stands in for, device against device.  Every destination lies inside canaries.  There is no tolerance anywhere.
Run on the GPU box:  python -m pytest tests -m gpu -q"""
import numpy as np
import pytest
import torch

from oracle import warp_numpy as wn
from tests import nv12_out_ref as NO
from tests import nv12_ref as NR
from tests import pixels as PX
from tests import remap_nv12_out_ref as RO
from tests import remap_ref as RR
from tests import stitch_maps_ref as SM
from tests import workloads as wl
from tests.test_gpu_nv12_out import canaried_planes, host, same
from tests.test_gpu_remap import _shifted_map
from tests.test_gpu_remap_nv12 import _gpu_map, _planes_of, _random_map, _ref_map, _wrap
from tests.test_gpu_stitch_maps import SCENE, DSIZE, dev_map, scene_maps
from tests.test_lens_cpu import GEOMS

pytestmark = pytest.mark.gpu

LINEAR, NEAREST = 1, 0
INF = float("inf")
BORDER = (7.0, 200.0, 31.0)   # a non-zero border pixel, in the sampled frame's channel order
MODES = RR.MODES[:5]          # the five modes that write every pixel
SOURCES = ("bgr", "rgb", "nv12")
LAYOUTS = ("joined", "narrow", "mixed")


@pytest.fixture(scope="module")
def W():
    from bev_amd import warp
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return warp


def _dst(batch, dh, dw, layout):
    """(out, [(holder, view) ...]): a canaried NV12 destination of `batch` frames.
    joined  one buffer per frame, the rows of pairs behind the Y rows, base and strides multiples of 16: 4-byte stores in both planes
    narrow  a (y, uv) pair: the Y base at an odd byte with padded rows of an odd stride (byte stores), the uv base 2 mod 4 (2-byte pair stores)
    mixed   a (y, uv) pair: that uv plane next to an aligned Y plane -- 4-byte Y stores and 2-byte pair stores in one launch"""
    if layout == "joined":
        v, holder = PX.canaried_out((batch, dh * 3 // 2, dw, 1), torch.uint8, pad=5, align=16)
        return v[..., 0], [(holder, v)]
    if layout == "narrow":
        out, holders = canaried_planes(batch, dh, dw, 0)
        return out, list(holders)
    (y, _), (hy, _) = canaried_planes(batch, dh, dw, 16)
    (_, uv), (_, huv) = canaried_planes(batch, dh, dw, 0)
    assert y.data_ptr() % 4 == 0 and uv.data_ptr() % 4 == 2
    return (y, uv), [hy, huv]


def _finish(W, out, holders, what):
    """(y, uv) of a result on the host, (B, dh, dw) and (B, dh / 2, dw / 2, 2), once the canaries around both planes are found intact."""
    got = host(W, out)
    for holder, view in holders:
        PX.assert_canaries_intact(holder, view, what)
    return got


def _device_frames(source, frames, layout="joined", fill=3):
    """The frames of one call on the device.  bgr / rgb: frames is a list of (H, W, 3) arrays -> (B, H, W, 3), tight ("joined") or inside
    a larger allocation filled with `fill`; nv12: a list of (y, uv) -> the two planes, one buffer or row-padded allocations."""
    if source == "nv12":
        return _planes_of(np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), layout, fill)
    a = np.stack(frames)
    return (PX.padded_source(a, fill, offset=3) if layout == "padded" else torch.from_numpy(a).cuda(),)


def _run(W, source, dev, m, mode, layout, batch, border=BORDER, what=""):
    dw, dh = m.dsize
    out, holders = _dst(batch, dh, dw, layout)
    bv = border if mode == RR.CONSTANT else None
    if source == "nv12":
        got = W.remap_nv12_to_nv12(dev[0], dev[1], m, border_mode=mode, border_value=bv, out=out)
    else:
        got = W.remap_to_nv12(dev[0], m, border_mode=mode, border_value=bv, out=out, rgb=source == "rgb")
    assert got is out
    return _finish(W, out, holders, what)


def _exp(source, frame, xy, frac, interp, mode, border=BORDER):
    if source == "nv12":
        return RO.remap_nv12_to_nv12(frame[0], frame[1], xy, frac, interp, mode, border)
    return RO.remap_to_nv12(frame, xy, frac, interp, mode, border, rgb=source == "rgb")


def _frame(source, seed, sh, sw, kind="uniform"):
    """One frame of a source kind: full-range random B, G, R (R, G, B) pixels, or full-range random NV12 planes."""
    if source == "nv12":
        return NR.frame(kind, seed, sh, sw)
    return np.random.default_rng(9000 + seed).integers(0, 256, (sh, sw, 3), dtype=np.uint8)


# ---- 1. the parity matrix: every single-camera instance, against the definition and against the entries the launch replaces ----

@pytest.mark.parametrize("geom", sorted(GEOMS))
@pytest.mark.parametrize("kind", ["pinhole", "A"])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_parity_matrix(W, geom, kind, interp):
    sw, sh, dw, dh, M = GEOMS[geom]
    m = _gpu_map(W, geom, kind, interp)
    xy, frac = _ref_map(geom, kind, interp)
    for source in SOURCES:
        frame = _frame(source, 11, sh, sw, "phase")
        dev = _device_frames(source, [frame])
        for mode in MODES:
            what = "%s %s %s mode %d interp %d" % (geom, kind, source, mode, interp)
            gy, guv = _run(W, source, dev, m, mode, "joined", 1, what=what)
            same((gy[0], guv[0]), _exp(source, frame, xy, frac, interp, mode), what)
            # device against device: BGR -> NV12 of what the composed entry writes
            bv = BORDER if mode == RR.CONSTANT else None
            if source == "nv12":
                pixels = W.remap_nv12(dev[0], dev[1], m, border_mode=mode, border_value=bv)
            else:
                pixels = W.remap(dev[0], m, border_mode=mode, border_value=bv)
            torch.cuda.synchronize()
            same((gy[0], guv[0]), NO.bgr_to_nv12(pixels[0].cpu().numpy(), source == "rgb"), what + ", of the device's own remap")
            if kind == "pinhole" and mode == RR.CONSTANT:  # ... and the matrix warp into NV12 of the same matrix
                if source == "nv12":
                    two = W.warp_nv12_to_nv12(dev[0], dev[1], M, (dw, dh), flags=interp, border_value=BORDER)
                else:
                    two = W.warp_perspective_to_nv12(dev[0], M, (dw, dh), flags=interp, border_value=BORDER, rgb=source == "rgb")
                ty, tuv = host(W, two)
                same((gy[0], guv[0]), (ty[0], tuv[0]), what + ", the matrix warp")
    # without `out`: a new joined buffer, of a single frame and of a batch
    one = W.remap_to_nv12(torch.from_numpy(_frame("bgr", 11, sh, sw)).cuda(), m)
    assert tuple(one.shape) == (dh * 3 // 2, dw) and one.dtype == torch.uint8
    same(host(W, one), _exp("bgr", _frame("bgr", 11, sh, sw), xy, frac, interp, RR.CONSTANT, 0.0), "a new joined buffer of one frame")
    two = W.remap_nv12_to_nv12(*_device_frames("nv12", [_frame("nv12", 11, sh, sw)] * 2), m)
    assert tuple(two.shape) == (2, dh * 3 // 2, dw)
    y2, uv2 = host(W, two)
    same((y2[1], uv2[1]), _exp("nv12", _frame("nv12", 11, sh, sw), xy, frac, interp, RR.CONSTANT, 0.0), "a new joined buffer")


# ---- 2. destination widths, heights and layouts ----

@pytest.mark.parametrize("dw", [2, 4, 6, 254, 256, 258])
def test_widths_heights_and_layouts(W, dw):
    """A half lane alone (2), a full lane (4), a full lane and a half (6), both sides of the 256-pixel tile; heights on both sides of the
    4-row tile, whose odd rows write no pair; each in the three destination layouts; the map planes aligned and as unaligned views."""
    sw, sh = 32, 18
    frames = {s: _frame(s, 30, sh, sw, "phase") for s in SOURCES}
    devs = {s: _device_frames(s, [frames[s]]) for s in SOURCES}
    for dh in (2, 4, 6):
        M = wl.rotated_H(sw, sh, dw, dh, 12.0, zoom=1.3)
        for interp in (NEAREST, LINEAR):
            m = W.build_warp_map(M, (dw, dh), flags=interp)
            xy, frac = RR.build((dw, dh), wn.invert3x3(M), None, INF, interp)
            maps = {"joined": m, "narrow": _shifted_map(W, m, 4, 2, 3)[0], "mixed": _shifted_map(W, m, 16, 8, 0)[0]}
            for mode in (RR.CONSTANT, RR.REFLECT_101):
                for source in SOURCES:
                    exp = _exp(source, frames[source], xy, frac, interp, mode)
                    for layout in LAYOUTS:
                        what = "%d x %d %s mode %d interp %d %s" % (dw, dh, source, mode, interp, layout)
                        gy, guv = _run(W, source, devs[source], maps[layout], mode, layout, 1, what=what)
                        same((gy[0], guv[0]), exp, what)


# ---- 3. batching ----

@pytest.mark.parametrize("batch,per_frame", [(1, False), (2, False), (3, False), (5, False), (3, True)])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_batches(W, batch, per_frame, interp):
    """Every frame different, through a shared map and through a map per frame, on a small destination (one frame per item) and on an
    8 x 16384 one: 4096 tiles per frame, so a shared map walks two frames per item (tests/test_remap_nv12_out_cpu.py pins plan_remap) --
    one group (2 frames), and a short last group (3 and 5 frames)."""
    sw, sh = 40, 24
    for source in SOURCES:
        frames = [_frame(source, 20 + b, sh, sw) for b in range(batch)]
        dev = _device_frames(source, frames, "padded")
        for (dw, dh), modes, layout in (((36, 20), (RR.CONSTANT, RR.REFLECT_101), "narrow"), ((8, 16384), (RR.CONSTANT,), "joined")):
            xy, frac = _random_map(np.random.default_rng(batch * 10 + dh), batch if per_frame else 1, dh, dw, sw, sh)
            m = _wrap(W, xy, frac, interp)
            for mode in modes:
                gy, guv = _run(W, source, dev, m, mode, layout, batch)
                for b in range(batch):
                    k = b if per_frame else 0
                    same((gy[b], guv[b]), _exp(source, frames[b], xy[k], frac[k], interp, mode), "%s frame %d of %d, mode %d, %d x %d, %d maps" % (source, b, batch, mode, dw, dh, m.n))


# ---- 4. tiny sources and hand-made maps ----

@pytest.mark.parametrize("src_wh", [(2, 2), (4, 2), (2, 4), (4, 4), (6, 4)])
def test_tiny_sources_and_hand_made_maps(W, src_wh):
    """Hand-made maps over the whole int16 range, the sentinel and 32767 included, on sources of one, two and three pairs per row -- the
    sizes at which the NV12 window loads are refused (2 px), start at pair 0 only (4 px) or move (6 px), and at which a 6-byte pair load
    ends on a BGR row's last byte.  A third of the entries lie inside in x with every lane's four side by side (pair and window lanes).
    Each case runs with the padding around the source's rows filled with 0 and with 255: a load that strays past a row changes the answer."""
    sw, sh = src_wh
    dh, dw = 4, 262  # (two tile columns, a last lane of 2 pixels, odd and even rows)
    rng = np.random.default_rng(sw * 10 + sh)
    xy = rng.integers(-3 * max(sw, sh) - 2, 3 * max(sw, sh) + 3, (dh, dw, 2)).astype(np.int16)
    xy[1::2, 8:40] = rng.integers(-32768, 32768, (dh // 2, 32, 2))  # (few of them: the reference's index remap is a Python loop over the distinct indices)
    xy[:, 88:176, 0] = rng.integers(0, sw - 1, (dh, 88))          # adjacent columns inside, rows anywhere near
    xy[:, 88:176, 1] = rng.integers(-2, sh + 2, (dh, 88))
    xy[2, 176:216, 0] = rng.integers(0, sw - 1, 40) + sw * rng.integers(-3, 4, 40)   # (WRAP: adjacent columns after the remap)
    xy[0, :8] = [[-32768, -32768], [32767, 32767], [-32768, 0], [0, -32768], [32767, 0], [0, 32767], [-1, -1], [0, 0]]
    frac = rng.integers(0, 65536, (dh, dw)).astype(np.uint16)
    frac[1, :4] = [0, 1023, 0xfc00, 0xffff]
    for source in SOURCES:
        frame = _frame(source, 50, sh, sw, "phase")
        for interp in (NEAREST, LINEAR):
            m = _wrap(W, xy, frac, interp)
            for mode in MODES:
                exp = _exp(source, frame, xy, frac, interp, mode)
                for fill in (0, 255):
                    gy, guv = _run(W, source, _device_frames(source, [frame], "padded", fill), m, mode, "mixed", 1)
                    same((gy[0], guv[0]), exp, "%s %s mode %d interp %d padding %d" % (src_wh, source, mode, interp, fill))
    by, bu, bv = (int(v) for v in NO.yuv(*BORDER[::-1]))
    ey, euv = _exp("bgr", _frame("bgr", 50, sh, sw), xy, frac, LINEAR, RR.CONSTANT)
    assert int(ey[0, 0]) == by and euv[0, 0].tolist() == [bu, bv]  # the sentinel under CONSTANT is the border pixel, converted: its Y and its block's pair


# ---- 5. pixel values ----

CORNERS = [(b, g, r) for b in (0, 255) for g in (0, 255) for r in (0, 255)]


@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_corner_colours_at_even_and_odd_positions(W, interp):
    """Full-range random pixels with the eight corners of the colour cube at even / even positions (which give a Y and their block's pair)
    and at odd / odd ones (a Y only), through the identity map: the conversion's largest and smallest sums, in both channel orders."""
    h, w = 8, 12
    img = np.random.default_rng(77).integers(0, 256, (h, w, 3), dtype=np.uint8)
    for i, c in enumerate(CORNERS):
        img[2 * (i // 4), 2 * (i % 4)] = c
        img[2 * (i // 4) + 5, 2 * (i % 4) + 1] = c
    gx, gy = np.meshgrid(np.arange(w, dtype=np.int16), np.arange(h, dtype=np.int16))
    xy, frac = np.stack([gx, gy], axis=-1), np.zeros((h, w), np.uint16)
    m = _wrap(W, xy, frac, interp)
    for source in ("bgr", "rgb"):
        for mode in (RR.CONSTANT, RR.REPLICATE):
            gyy, guv = _run(W, source, _device_frames(source, [img]), m, mode, "joined", 1)
            same((gyy[0], guv[0]), NO.bgr_to_nv12(img, source == "rgb"), "%s mode %d" % (source, mode))  # (frac 0: the frame itself)
            same((gyy[0], guv[0]), _exp(source, img, xy, frac, interp, mode), "%s mode %d, the definition" % (source, mode))
    assert gyy[0].min() == 16 and gyy[0].max() == 235 and guv[0].min() == 16 and guv[0].max() == 240


# ---- 6. the stitch ----

def _stitch_sources(source, k, batch=None):
    """Camera k of the scene as a source kind: (host frame(s), device tensors).  batch: that many different frames, stacked."""
    w, h = SCENE[k][0], SCENE[k][1]
    frames = [_frame(source, 100 + 10 * k + b, h, w) for b in range(batch or 1)]
    if source == "nv12":
        ys, uvs = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
        dev = _planes_of(ys if batch else ys[0], uvs if batch else uvs[0], "padded" if k % 2 else "joined")
    else:
        a = np.stack(frames)
        dev = (PX.strided(a if batch else a[0], (9 + 2 * k,)) if k % 2 else torch.from_numpy(a if batch else a[0]).cuda(),)
    return frames, dev


def _stitch_run(W, source, devs, dmaps, blend, F, layout, batch, border=BORDER, single=False):
    dw, dh = dmaps[0].dsize
    out, holders = _dst(batch, dh, dw, layout)
    o = out if not single else (out[0] if layout == "joined" else (out[0][0], out[1][0]))
    if source == "nv12":
        got = W.remap_stitch_nv12_to_nv12([d[0] for d in devs], [d[1] for d in devs], dmaps, blend=blend, feather=F, border_value=border, out=o)
    else:
        got = W.remap_stitch_to_nv12([d[0] for d in devs], dmaps, blend=blend, feather=F, border_value=border, out=o, rgb=source == "rgb")
    assert got is o
    return _finish(W, out, holders, "%s %s F=%d" % (source, blend, F))


def _stitch_exp(source, frames, maps, interp, blend, F, border=BORDER):
    b = SM.FEATHER if blend == "feather" else SM.OVER
    if source == "nv12":
        return RO.stitch_nv12_to_nv12([f[0] for f in frames], [f[1] for f in frames], maps, interp, b, F, border)
    return RO.stitch_to_nv12(frames, maps, interp, b, F, border, rgb=source == "rgb")


@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
@pytest.mark.parametrize("lens", [False, True], ids=["pinhole", "lens"])
def test_stitch_scene(W, interp, lens):
    """1, 2 and 3 cameras of the scene, "over" and "feather" with F = 1, 3 and 64, the three source kinds (every stitch instance), single
    frames: both planes against the definition, and against BGR -> NV12 of the device's own remap_stitch / remap_stitch_nv12 canvas."""
    maps = scene_maps(interp, lens)
    dmaps = [dev_map(W, xy, frac, interp) for xy, frac in maps]
    _, count = SM.stitch([np.zeros((h, w, 3), np.uint8) for w, h, _, _ in SCENE], maps, interp)
    assert all((count == n).sum() >= 20 for n in range(4))  # a region no camera covers, and overlaps of two and of three
    for source in SOURCES:
        cams = [_stitch_sources(source, k) for k in range(3)]
        for n in (1, 2, 3):
            frames, devs = [c[0][0] for c in cams[:n]], [c[1] for c in cams[:n]]
            for blend, F in (("over", 64), ("feather", 1), ("feather", 3), ("feather", 64)):
                what = "%s, %d cameras, %s F=%d, interp %d" % (source, n, blend, F, interp)
                gy, guv = _stitch_run(W, source, devs, dmaps[:n], blend, F, LAYOUTS[n - 1], 1, single=True)
                same((gy[0], guv[0]), _stitch_exp(source, frames, maps[:n], interp, blend, F), what)
                if source == "nv12":
                    canvas = W.remap_stitch_nv12([d[0] for d in devs], [d[1] for d in devs], dmaps[:n], blend=blend, feather=F, border_value=BORDER)
                else:
                    canvas = W.remap_stitch([d[0] for d in devs], dmaps[:n], blend=blend, feather=F, border_value=BORDER)
                torch.cuda.synchronize()
                same((gy[0], guv[0]), NO.bgr_to_nv12(canvas.cpu().numpy(), source == "rgb"), what + ", of the device's own canvas")
    # the pixel no camera covers is the border pixel, converted
    by, bu, bv = (int(v) for v in NO.yuv(*BORDER[::-1]))
    assert (gy[0][count == 0] == by).all() and (guv[0][(count == 0)[0::2, 0::2]] == (bu, bv)).all() and (count == 0)[0::2, 0::2].any()


@pytest.mark.parametrize("source", SOURCES)
def test_stitch_eight_cameras(W, source):
    sizes = [(40, 24), (34, 28), (64, 18), (26, 26), (48, 22), (32, 34), (52, 20), (38, 28)]
    M = SCENE[0][2]
    for interp in (NEAREST, LINEAR):
        maps = [RR.build(DSIZE, M + np.array([[0.01 * k, 0.005 * k, -1.5 * k], [0, 0.03 * k, -0.5 * k], [0, 0, 0]]), interp=interp) for k in range(8)]
        frames = [_frame(source, 200 + k, hh, ww) for k, (ww, hh) in enumerate(sizes)]
        devs = [_device_frames(source, [f]) for f in frames]
        devs = [tuple(t[0] for t in d) for d in devs]  # (single frames)
        dmaps = [dev_map(W, xy, frac, interp) for xy, frac in maps]
        for blend, F in (("over", 64), ("feather", 3)):
            gy, guv = _stitch_run(W, source, devs, dmaps, blend, F, "narrow", 1, single=True)
            same((gy[0], guv[0]), _stitch_exp(source, frames, maps, interp, blend, F), "%s, 8 cameras, %s, interp %d" % (source, blend, interp))
    _, count = SM.stitch([np.zeros((hh, ww, 3), np.uint8) for ww, hh in sizes], maps, interp)
    assert (count == 8).sum() >= 40 and (count == 0).sum() >= 40


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("blend,F", [("over", 64), ("feather", 3)])
def test_stitch_batch_of_two_with_mixed_map_planes(W, source, blend, F):
    """A batch of 2 with per-camera shared maps: camera 0's in aligned planes (lane-wide loads), camera 1's in row-padded planes at
    addresses that are no multiple of 16 / 8 (loads entry by entry, in the same launch), camera 2's a lens map; a non-zero border pixel
    where no camera covers; the joined destination, frame after frame."""
    interp = LINEAR
    pin, lens = scene_maps(interp, False), scene_maps(interp, True)
    maps = [pin[0], pin[1], lens[2]]
    d0, d1, d2 = dev_map(W, *maps[0], interp), _shifted_map(W, dev_map(W, *maps[1], interp), 4, 2, 3)[0], dev_map(W, *maps[2], interp)
    assert d0.xy.data_ptr() % 16 == 0 and d1.xy.data_ptr() % 16 == 4 and d1.frac.data_ptr() % 8 == 2 and d0.n == d1.n == d2.n == 1
    cams = [_stitch_sources(source, k, batch=2) for k in range(3)]
    for layout in ("joined", "mixed"):
        gy, guv = _stitch_run(W, source, [c[1] for c in cams], [d0, d1, d2], blend, F, layout, 2)
        for b in range(2):
            same((gy[b], guv[b]), _stitch_exp(source, [c[0][b] for c in cams], maps, interp, blend, F), "%s frame %d %s %s" % (source, b, blend, layout))
    assert not np.array_equal(gy[0], gy[1])


# ---- 7. the pipeline ----

@pytest.mark.parametrize("src_format,dst_format", [("bgr", "nv12"), ("nv12", "bgr"), ("nv12", "nv12")])
@pytest.mark.parametrize("download", [True, False], ids=["download", "resident"])
def test_frame_pipeline_with_a_map_and_nv12_slots(W, src_format, dst_format, download):
    """Four frames through a ring of two slots: each result equals the function call's on the same frame, and the definition."""
    from bev_amd.pipeline import FramePipeline
    sw, sh, dw, dh, M = GEOMS["rotated_zoom_out"]
    m = _gpu_map(W, "rotated_zoom_out", "A", LINEAR)
    xy, frac = _ref_map("rotated_zoom_out", "A", LINEAR)
    frames = [NR.frame("uniform", 60 + i, sh, sw) for i in range(4)]
    if src_format == "bgr":
        inputs = [NR.nv12_to_bgr(y, uv) for y, uv in frames]
    else:
        inputs = [NR.join(y, uv) for y, uv in frames]
    with FramePipeline((sh, sw), 3, None, (dw, dh), warp_map=m, src_format=src_format, dst_format=dst_format, depth=2, download=download) as pipe:
        assert tuple(pipe.d_out[0].shape) == ((dh * 3 // 2, dw) if dst_format == "nv12" else (dh, dw, 3))
        assert tuple(pipe.h_in[0].shape) == ((sh * 3 // 2, sw) if src_format == "nv12" else (sh, sw, 3))
        outs = [np.array(res.cpu().numpy() if isinstance(res, torch.Tensor) else res) for res in pipe.run(inputs)]
    assert len(outs) == 4
    for i, got in enumerate(outs):
        t = torch.from_numpy(inputs[i]).cuda()
        if src_format == "nv12":
            y, uv = W.split_nv12(t)
            want = W.remap_nv12_to_nv12(y, uv, m) if dst_format == "nv12" else W.remap_nv12(y, uv, m)
        else:
            want = W.remap_to_nv12(t, m)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got, want.cpu().numpy(), err_msg="frame %d" % i)
        if dst_format == "nv12":
            exp = _exp("nv12", frames[i], xy, frac, LINEAR, RR.CONSTANT, 0.0) if src_format == "nv12" else _exp("bgr", inputs[i], xy, frac, LINEAR, RR.CONSTANT, 0.0)
            same((got[:dh], got[dh:].reshape(dh // 2, dw // 2, 2)), exp, "frame %d, the definition" % i)
    assert not np.array_equal(outs[0], outs[1])
