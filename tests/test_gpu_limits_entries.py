"""The lens, NV12, map and stitch entries at the largest sizes and strides the C ABI admits -- what tests/test_gpu_limits.py does for
bevwarp_warp, the border, bicubic and plane kernels, for the 24 pixel entry points that came after it: bevwarp_warp_lens, _warp_stitch,
_warp_nv12, _warp_nv12_planes, _warp_to_nv12, _warp_nv12_to_nv12, _build_map, _remap, _remap_nv12, _remap_nv12_planes, _remap_to_nv12,
_remap_nv12_to_nv12, _remap_planes and the six _stitch_maps* entries, through the Python entries of bev_amd.warp with `out=` views.

Their addressing is their own: the map samplers form tap addresses as 32-bit offsets (right only because rows * stride < 2^31), the
8-bit x3 pair loads, the 2-byte Y windows and the 4-byte pair windows choose their path at the last column with two valid taps, the index
remap builds a fast_div magic per axis (largest at n = 32766 / 32767), and every store goes through 64-bit row, frame and plane terms.

  A, B   sources 32767 px (NV12: 32766 px) wide / tall; maps parked on either end of the long axis and over all of it
  C      row strides of 2^24 - 1 / 2^24 - 16 bytes (NV12: 2^24 - 1 and 2^24 - 2), rows * stride just below 2^31; one past either is refused
  D      source frames, destination frames, channel planes and map planes 2^32 + 4096 bytes apart
  E      destination and map rows 2^26 bytes apart, the last one beyond 4.5 GiB
  F      item counts on either side of fast_div's exactness bound, and remap's groups of frames with a short last group

Every comparison is bit for bit against the numpy references under tests/.  The large shapes are large only in stride (tests/limits_buffers.py:
canary-filled holders, the real rows copied in through the view, the reference fed the compact copy); shapes and layouts live in
tests/limits_cases.py, which tests/test_limits_cpu.py checks on the CPU.  At most one holder of about 8.6 GiB is alive per test."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

from bev_amd import _lib, warp as W
from oracle import cpu_oracle as co
from tests import border_ref as br
from tests import hostplan
from tests import lens_ref as LR
from tests import limits_cases as lc
from tests import map_planes_ref as MP
from tests import nv12_out_ref as NO
from tests import nv12_ref as NR
from tests import remap_nv12_out_ref as RNO
from tests import remap_nv12_ref as RN
from tests import remap_ref as RR
from tests import stitch_maps_ref as SM
from tests import stitch_ref as SR
from tests.limits_buffers import assert_only_the_view_was_written, byte_holder, nan_holder, same, strided

pytestmark = pytest.mark.gpu

INV = W.WARP_INVERSE_MAP
NEAREST, LINEAR = W.INTER_NEAREST, W.INTER_LINEAR
TOO_LARGE = -3
SCALE, BIAS = [1 / 255.0, 0.5, 2.0], [0.0, -1.0, 3.5]
WRITING = (RR.CONSTANT, RR.REPLICATE, RR.REFLECT, RR.WRAP, RR.REFLECT_101)  # the border modes that write every pixel
BLENDS = (("over", SR.OVER), ("feather", SR.FEATHER))
FEATHER = 64
PLANE_DTYPES = (torch.float32, torch.float16)
CANVAS_SEED = 60


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------------
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def frames(a, single_ndim):
    """The frames of a host array: itself when it is one image of `single_ndim` dimensions, else its first axis."""
    return [a] if a.ndim == single_ndim else list(a)


def matrices(M):
    M = np.asarray(M)
    return [M] if M.ndim == 2 else list(M)


def stacked(results, batched):
    return np.stack(results) if batched else results[0]


def bv(mode, c):
    return lc.BORDER[:c] if mode == RR.CONSTANT else None


def fill(out, value=77):
    for t in out if isinstance(out, (tuple, list)) else (out,):
        t.fill_(value)


def px_out(out, like, dsize, batch):
    """The interleaved destination of a call: the caller's strided view, or a compact one; poisoned."""
    if out is None:
        c = like.shape[-1]
        out = torch.empty(((batch,) if batch else ()) + (dsize[1], dsize[0], c), dtype=like.dtype, device="cuda")
    fill(out)
    return out


def nv12_out(out, dsize, batch):
    if out is None:
        lead = (batch,) if batch else ()
        out = (torch.empty(lead + (dsize[1], dsize[0]), dtype=torch.uint8, device="cuda"),
               torch.empty(lead + (dsize[1] // 2, dsize[0] // 2, 2), dtype=torch.uint8, device="cuda"))
    fill(out)
    return out


def planes_out(out_of, dtype):
    """The planar destination of a call: None (the entry allocates), or the caller's strided view out_of(dtype), poisoned."""
    if out_of is None:
        return None
    out = out_of(dtype)
    fill(out)
    return out


def same_nv12(out, exp):
    """out: the (y, uv) device pair; exp: [(y, uv)] per frame."""
    batched = out[0].dim() == 3
    np.testing.assert_array_equal(out[0].cpu().numpy(), stacked([e[0] for e in exp], batched))
    np.testing.assert_array_equal(out[1].cpu().numpy(), stacked([e[1] for e in exp], batched))


def same_planes(got, exp_f32, dtype):
    RN.assert_planes_equal(got, exp_f32, dtype)


class Maps:
    """The device map of a call and the reference's, per frame: built by bevwarp_build_map and compared with remap_ref.build on the way."""

    def __init__(self, Minv, dsize, interp, lens=None, out=None):
        self.interp, self.dsize = interp, dsize
        K, dist, r2_max = lens if lens is not None else (None, None, None)
        self.dev = W.build_warp_map(Minv, dsize, flags=interp | INV, K=K, dist_coeff=dist, r2_max=r2_max, out=out)
        if lens is None:
            self.ref = [RR.build(dsize, M, interp=interp) for M in matrices(Minv)]
        else:
            self.ref = [RR.build(dsize, LR.ray_matrix(M, K, inverse_given=True), LR.lens12(K, dist), r2_max, interp) for M in matrices(Minv)]
        assert self.dev.n == len(self.ref)
        torch.cuda.synchronize()
        xy = self.dev.xy.cpu().numpy()
        frac = None if interp == NEAREST else self.dev.frac.cpu().numpy().view(np.uint16)
        for i, (exy, efrac) in enumerate(self.ref):
            np.testing.assert_array_equal(xy[i], exy)
            if interp == LINEAR:
                np.testing.assert_array_equal(frac[i], efrac)

    def of(self, i):
        return self.ref[i if len(self.ref) > 1 else 0]


def both_maps(Minv, dsize, lens=None):
    return [Maps(Minv, dsize, interp, lens) for interp in (NEAREST, LINEAR)]


def assert_both_tap_paths(xy, w, h):
    """Coverage of the case, from the reference's map: a lane is 4 consecutive pixels of a destination row; some lanes lie wholly inside
    the frame (adjacent taps: the pair loads and 2-byte windows) and some hold a pixel at a clamped or remapped edge (tap by tap)."""
    sx, sy = xy[..., 0].astype(np.int64), xy[..., 1].astype(np.int64)
    inside = (sx >= 0) & (sx <= w - 2) & (sy >= 0) & (sy <= h - 2)
    n = inside.shape[1] // 4 * 4
    lanes = inside[:, :n].reshape(inside.shape[0], -1, 4)
    assert lanes.all(-1).any() and (~lanes).any(-1).any()


# ---- the entries of one source kind, against the references -------------------------------------------------------------------------------------
def run_remap(t, src, maps, modes, out=None):
    """bevwarp_remap in `modes`; TRANSPARENT over a patterned canvas."""
    batched = src.ndim == 4
    c = src.shape[-1]
    for m in maps:
        for mode in modes:
            o = px_out(out, t, m.dsize, src.shape[0] if batched else 0)
            canvas = lc.pixels(CANVAS_SEED, m.dsize[1], m.dsize[0], c, src.dtype)
            if mode == RR.TRANSPARENT:
                o.copy_(dev(canvas).expand_as(o) if batched else dev(canvas))
            assert W.remap(t, m.dev, border_mode=mode, border_value=bv(mode, c), out=o) is o
            exp = [RR.remap(f, *m.of(i), m.interp, mode, border_value=lc.BORDER[:c], canvas=canvas) for i, f in enumerate(frames(src, 3))]
            same(o.cpu().numpy(), stacked(exp, batched))


def run_lens(t, src, Minv, dsize, lens, out=None):
    """bevwarp_warp_lens, CONSTANT and TRANSPARENT: with the identity lens (the call is warp_perspective's: its kernels, not bevwarp_warp_lens) and the
    mild lens (lens = (K, dist, r2_max, the lens run's matrices))."""
    batched = src.ndim == 4
    c = src.shape[-1]
    canvas = lc.pixels(CANVAS_SEED, dsize[1], dsize[0], c, src.dtype)
    for interp in (NEAREST, LINEAR):
        for mode in (RR.CONSTANT, RR.TRANSPARENT):
            runs = [(None, Minv)] + ([] if lens is None else [(lens[:3], lens[3])])
            for ln, Mi in runs:
                o = px_out(out, t, dsize, src.shape[0] if batched else 0)
                if mode == RR.TRANSPARENT:
                    o.copy_(dev(canvas).expand_as(o) if batched else dev(canvas))
                K, dist, r2_max = ln if ln is not None else (lc.mild_lens(src.shape[-3:-1])[0], np.zeros(5), None)
                assert W.warp_perspective_lens(t, Mi, dsize, K, dist, flags=interp | INV, border_value=bv(mode, c), out=o, border_mode=mode, r2_max=r2_max) is o
                if ln is None:
                    exp = [br.warp(f, M, dsize, interp, mode, m_is_inverse=True, border_value=lc.BORDER[:c], canvas=canvas)
                           for f, M in zip(frames(src, 3), matrices(Mi) * len(frames(src, 3)))]
                else:
                    exp = [LR.warp(f, LR.ray_matrix(M, K, inverse_given=True), LR.lens12(K, dist), r2_max, dsize, interp, mode, border_value=lc.BORDER[:c], canvas=canvas)
                           for f, M in zip(frames(src, 3), matrices(Mi) * len(frames(src, 3)))]
                same(o.cpu().numpy(), stacked(exp, batched))


def run_bgr_to_nv12(t, src, Minv, maps, modes, out=None):
    """bevwarp_warp_to_nv12 (the constant border) and bevwarp_remap_to_nv12 in `modes`."""
    batched = src.ndim == 4
    B = src.shape[0] if batched else 0
    fr, Ms = frames(src, 3), matrices(Minv)
    for m in maps:
        o = nv12_out(out, m.dsize, B)
        W.warp_perspective_to_nv12(t, Minv, m.dsize, flags=m.interp | INV, border_value=lc.BORDER[:3], out=o)
        same_nv12(o, [NO.warp_to_nv12(f, Ms[i % len(Ms)], m.dsize, m.interp, border_value=lc.BORDER[:3], m_is_inverse=True) for i, f in enumerate(fr)])
        for mode in modes:
            o = nv12_out(out, m.dsize, B)
            W.remap_to_nv12(t, m.dev, border_mode=mode, border_value=bv(mode, 3), out=o)
            same_nv12(o, [RNO.remap_to_nv12(f, *m.of(i), m.interp, mode, lc.BORDER[:3]) for i, f in enumerate(fr)])


def run_bgr_to_planar(t, src, maps, modes, dtypes=PLANE_DTYPES, out_of=None):
    """bevwarp_remap_planes in `modes`, to float32 and float16 planes.  out_of(dtype): a strided destination."""
    batched = src.ndim == 4
    for m in maps:
        for mode in modes:
            exp = stacked([MP.remap_planes(f, *m.of(i), m.interp, mode, SCALE, BIAS, lc.BORDER[:3]) for i, f in enumerate(frames(src, 3))], batched)
            for dtype in dtypes:
                o = planes_out(out_of, dtype)
                got = W.remap_to_planar(t, m.dev, scale=SCALE, bias=BIAS, border_mode=mode, border_value=bv(mode, 3), out=o, out_dtype=dtype)
                assert o is None or got is o
                same_planes(got, exp, dtype)


def run_nv12_to_px(y, uv, hy, huv, Minv, maps, modes, out=None):
    """bevwarp_warp_nv12 (the constant border) and bevwarp_remap_nv12 in `modes`; TRANSPARENT over a patterned canvas."""
    batched = hy.ndim == 3
    B = hy.shape[0] if batched else 0
    fy, fuv, Ms = frames(hy, 2), frames(huv, 3), matrices(Minv)
    like = torch.empty((1, 1, 3), dtype=torch.uint8)
    for m in maps:
        o = px_out(out, like, m.dsize, B)
        assert W.warp_perspective_nv12(y, uv, Minv, m.dsize, flags=m.interp | INV, border_value=lc.BORDER[:3], out=o) is o
        exp = [NR.warp_nv12(a, b, Ms[i % len(Ms)], m.dsize, m.interp, border_value=lc.BORDER[:3], m_is_inverse=True) for i, (a, b) in enumerate(zip(fy, fuv))]
        same(o.cpu().numpy(), stacked(exp, batched))
        canvas = lc.pixels(CANVAS_SEED, m.dsize[1], m.dsize[0], 3, np.uint8)
        for mode in modes:
            o = px_out(out, like, m.dsize, B)
            if mode == RR.TRANSPARENT:
                o.copy_(dev(canvas).expand_as(o) if batched else dev(canvas))
            assert W.remap_nv12(y, uv, m.dev, border_mode=mode, border_value=bv(mode, 3), out=o) is o
            exp = [RN.remap_nv12(a, b, *m.of(i), m.interp, mode, lc.BORDER[:3], canvas) for i, (a, b) in enumerate(zip(fy, fuv))]
            same(o.cpu().numpy(), stacked(exp, batched))


def run_nv12_to_planar(y, uv, hy, huv, Minv, maps, modes, dtypes=PLANE_DTYPES, out_of=None):
    """bevwarp_warp_nv12_planes (the constant border) and bevwarp_remap_nv12_planes in `modes`."""
    batched = hy.ndim == 3
    fy, fuv, Ms = frames(hy, 2), frames(huv, 3), matrices(Minv)
    for m in maps:
        warped = [NR.warp_nv12(a, b, Ms[i % len(Ms)], m.dsize, m.interp, border_value=lc.BORDER[:3], m_is_inverse=True) for i, (a, b) in enumerate(zip(fy, fuv))]
        exp = stacked([RN.planes_f32(p, SCALE, BIAS) for p in warped], batched)
        for dtype in dtypes:
            o = planes_out(out_of, dtype)
            got = W.warp_nv12_to_planar(y, uv, Minv, m.dsize, scale=SCALE, bias=BIAS, flags=m.interp | INV, border_value=lc.BORDER[:3], out=o, out_dtype=dtype)
            assert o is None or got is o
            same_planes(got, exp, dtype)
        for mode in modes:
            exp = stacked([RN.remap_nv12_planes(a, b, *m.of(i), m.interp, mode, SCALE, BIAS, lc.BORDER[:3]) for i, (a, b) in enumerate(zip(fy, fuv))], batched)
            for dtype in dtypes:
                o = planes_out(out_of, dtype)
                got = W.remap_nv12_to_planar(y, uv, m.dev, scale=SCALE, bias=BIAS, border_mode=mode, border_value=bv(mode, 3), out=o, out_dtype=dtype)
                assert o is None or got is o
                same_planes(got, exp, dtype)


def run_nv12_to_nv12(y, uv, hy, huv, Minv, maps, modes, out=None):
    """bevwarp_warp_nv12_to_nv12 (the constant border) and bevwarp_remap_nv12_to_nv12 in `modes`."""
    batched = hy.ndim == 3
    B = hy.shape[0] if batched else 0
    fy, fuv, Ms = frames(hy, 2), frames(huv, 3), matrices(Minv)
    for m in maps:
        o = nv12_out(out, m.dsize, B)
        W.warp_nv12_to_nv12(y, uv, Minv, m.dsize, flags=m.interp | INV, border_value=lc.BORDER[:3], out=o)
        same_nv12(o, [NO.warp_nv12_to_nv12(a, b, Ms[i % len(Ms)], m.dsize, m.interp, border_value=lc.BORDER[:3], m_is_inverse=True)
                      for i, (a, b) in enumerate(zip(fy, fuv))])
        for mode in modes:
            o = nv12_out(out, m.dsize, B)
            W.remap_nv12_to_nv12(y, uv, m.dev, border_mode=mode, border_value=bv(mode, 3), out=o)
            same_nv12(o, [RNO.remap_nv12_to_nv12(a, b, *m.of(i), m.interp, mode, lc.BORDER[:3]) for i, (a, b) in enumerate(zip(fy, fuv))])


def run_stitch(ts, srcs, Minvs, dsize, out=None, nv12_out_=None, planes_of=None, kinds=("px", "nv12", "planes")):
    """The stitches of interleaved cameras in one launch, both blends, nearest and bilinear: bevwarp_warp_stitch and bevwarp_stitch_maps
    (kind "px"), and for 8-bit x3 cameras bevwarp_stitch_maps_to_nv12 ("nv12") and bevwarp_stitch_maps_planes ("planes").  Single frames."""
    c = srcs[0].shape[-1]
    u8x3 = srcs[0].dtype == np.uint8 and c == 3
    for interp in (NEAREST, LINEAR):
        maps = [Maps(M, dsize, interp) for M in Minvs]
        refs = [m.of(0) for m in maps]
        for blend, ref_blend in BLENDS:
            exp, count = SM.stitch(srcs, refs, interp, ref_blend, FEATHER, SM.CONSTANT, lc.BORDER[:c])
            assert (count >= 2).any() and (count == 1).any()
            if "px" in kinds:
                exp_w, _ = SR.stitch(srcs, Minvs, dsize, interp, ref_blend, FEATHER, SR.CONSTANT, lc.BORDER[:c])
                o = px_out(out, ts[0], dsize, 0)
                assert W.warp_stitch(ts, Minvs, dsize, flags=interp | INV, blend=blend, feather=FEATHER, border_value=lc.BORDER[:c], out=o) is o
                same(o.cpu().numpy(), exp_w)
                o = px_out(out, ts[0], dsize, 0)
                assert W.remap_stitch(ts, [m.dev for m in maps], blend=blend, feather=FEATHER, border_value=lc.BORDER[:c], out=o) is o
                same(o.cpu().numpy(), exp)
            if u8x3 and "nv12" in kinds:
                o = nv12_out(nv12_out_, dsize, 0)
                W.remap_stitch_to_nv12(ts, [m.dev for m in maps], blend=blend, feather=FEATHER, border_value=lc.BORDER[:3], out=o)
                same_nv12(o, [RNO.stitch_to_nv12(srcs, refs, interp, ref_blend, FEATHER, lc.BORDER[:3])])
            if u8x3 and "planes" in kinds:
                planes = MP.stitch_planes(srcs, refs, interp, SCALE, BIAS, ref_blend, FEATHER, lc.BORDER[:3])
                for dtype in PLANE_DTYPES:
                    o = planes_out(planes_of, dtype)
                    got = W.remap_stitch_to_planar(ts, [m.dev for m in maps], scale=SCALE, bias=BIAS, blend=blend, feather=FEATHER, border_value=lc.BORDER[:3], out=o,
                                                   out_dtype=dtype)
                    assert o is None or got is o
                    same_planes(got, planes, dtype)


def run_stitch_nv12(ys, uvs, hys, huvs, Minvs, dsize):
    """The stitches of NV12 cameras: bevwarp_stitch_maps_nv12, _stitch_maps_nv12_to_nv12 and _stitch_maps_nv12_planes."""
    for interp in (NEAREST, LINEAR):
        maps = [Maps(M, dsize, interp) for M in Minvs]
        refs, dmaps = [m.of(0) for m in maps], [m.dev for m in maps]
        for blend, ref_blend in BLENDS:
            exp, count = SM.stitch_nv12(hys, huvs, refs, interp, ref_blend, FEATHER, SM.CONSTANT, lc.BORDER[:3])
            assert (count >= 2).any() and (count == 1).any()
            o = px_out(None, torch.empty((1, 1, 3), dtype=torch.uint8), dsize, 0)
            assert W.remap_stitch_nv12(ys, uvs, dmaps, blend=blend, feather=FEATHER, border_value=lc.BORDER[:3], out=o) is o
            same(o.cpu().numpy(), exp)
            o = nv12_out(None, dsize, 0)
            W.remap_stitch_nv12_to_nv12(ys, uvs, dmaps, blend=blend, feather=FEATHER, border_value=lc.BORDER[:3], out=o)
            same_nv12(o, [RNO.stitch_nv12_to_nv12(hys, huvs, refs, interp, ref_blend, FEATHER, lc.BORDER[:3])])
            planes = MP.stitch_nv12_planes(hys, huvs, refs, interp, SCALE, BIAS, ref_blend, FEATHER, lc.BORDER[:3])
            for dtype in PLANE_DTYPES:
                got = W.remap_stitch_nv12_to_planar(ys, uvs, dmaps, scale=SCALE, bias=BIAS, blend=blend, feather=FEATHER, border_value=lc.BORDER[:3], out_dtype=dtype)
                same_planes(got, planes, dtype)


def lens_of(name, key):
    """(K, dist, r2_max, the lens run's inverse matrix) of case A / B under `key`: every map has a lens run of its own."""
    maps = lc.WIDE_LENS_MAPS if name == "wide" else lc.TALL_LENS_MAPS
    return lc.mild_lens(lc.entry_case(name)[0], key) + (maps[key],)


# ---- A, B: the widest and the tallest source ------------------------------------------------------------------------------------------------------
KEYS = sorted(lc.WIDE_ENTRY_MAPS)


@pytest.mark.parametrize("dtype,c", [(np.uint8, 3), (np.float32, 1)], ids=["uint8x3", "float32x1"])
@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("name", ["wide", "tall"])
def test_widest_and_tallest_source_interleaved(name, key, dtype, c):
    """Cases A and B, interleaved sources of 32767 px: the map builder (pinhole and lens), remap in all six borders, the lens warp, and for
    8-bit x3 the entries into NV12 and into channel planes in the five writing borders (REFLECT and WRAP run border_period at n = 32767)."""
    (h, w), dsize, maps_of, _ = lc.entry_case(name)
    Minv = maps_of[key]
    src = lc.pixels(13, h, w, c, dtype)
    t = dev(src)
    maps = both_maps(Minv, dsize)
    assert_both_tap_paths(maps[1].of(0)[0], w, h)
    run_remap(t, src, maps, RR.MODES)
    lens = lens_of(name, key)
    run_lens(t, src, Minv, dsize, lens)
    lens_maps = both_maps(lens[3], dsize, lens[:3])
    assert_both_tap_paths(lens_maps[1].of(0)[0], w, h)
    run_remap(t, src, lens_maps, (RR.CONSTANT, RR.TRANSPARENT))
    if dtype == np.uint8:
        run_bgr_to_nv12(t, src, Minv, maps, WRITING)
        run_bgr_to_planar(t, src, maps, WRITING)


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("name", ["wide", "tall"])
def test_widest_and_tallest_source_nv12(name, key):
    """Cases A and B, NV12 sources of 32766 px: the eight entries that read NV12 through matrices or maps."""
    (h, w), dsize, maps_of, _ = lc.entry_case(name, nv12=True)
    Minv = maps_of[key]
    hy, huv = NR.frame("phase", 14, h, w)
    y, uv = dev(hy), dev(huv)
    maps = both_maps(Minv, dsize)
    assert_both_tap_paths(maps[1].of(0)[0], w, h)
    run_nv12_to_px(y, uv, hy, huv, Minv, maps, RR.MODES)
    run_nv12_to_planar(y, uv, hy, huv, Minv, maps, WRITING)
    run_nv12_to_nv12(y, uv, hy, huv, Minv, maps, WRITING)


@pytest.mark.parametrize("kind", ["uint8x3", "float32x1", "nv12"])
def test_widest_and_tallest_source_stitched(kind):
    """Cases A and B in one launch: the widest source, the tallest one and a 96 x 700 frame stitched into one canvas all three reach."""
    cams = lc.stitch_cameras(nv12=kind == "nv12")
    Minvs = [M for _, M in cams]
    if kind == "nv12":
        planes = [NR.frame("phase", 15 + i, h, w) for i, ((h, w), _) in enumerate(cams)]
        hys, huvs = [p[0] for p in planes], [p[1] for p in planes]
        run_stitch_nv12([dev(a) for a in hys], [dev(a) for a in huvs], hys, huvs, Minvs, lc.STITCH_DSIZE)
    else:
        dtype, c = (np.uint8, 3) if kind == "uint8x3" else (np.float32, 1)
        srcs = [lc.pixels(15 + i, h, w, c, dtype) for i, ((h, w), _) in enumerate(cams)]
        run_stitch([dev(s) for s in srcs], srcs, Minvs, lc.STITCH_DSIZE)


# ---- C: the largest row stride ---------------------------------------------------------------------------------------------------------------------
STRIDE_ENTRY_FORMATS = [(np.uint8, 3, lc.STRIDE_ODD), (np.uint8, 4, lc.STRIDE_ALIGNED), (np.float32, 1, lc.STRIDE_ALIGNED)]
SECOND_CAMERA = lc.affine(1.1, 8.4, 1.4, -1.7)  # the 96 x 700 frame over case C's 600 x 64 destination


def stride_lens(rows):
    K, dist, _ = lc.mild_lens((rows, lc.STRIDE_W))
    return K, dist, float("inf"), lc.stride_map(rows)


@pytest.mark.parametrize("dtype,c,rs", STRIDE_ENTRY_FORMATS, ids=["uint8x3-odd", "uint8x4-aligned", "float32x1-aligned"])
def test_largest_row_stride_interleaved(dtype, c, rs):
    """Case C: rows 2^24 - 1 / 2^24 - 16 bytes apart, 128 of them; the map reads them from the first to the last, so the largest 32-bit tap
    offset the samplers form is just below 2^31.  Float32 rows lie in a holder of NaNs: a tap outside the copied rows poisons its pixel.
    One row more, or a stride of 2^24, is BEVWARP_ERR_TOO_LARGE for bevwarp_remap and bevwarp_warp_lens, with nothing launched."""
    esz, rows = np.dtype(dtype).itemsize, lc.max_rows(rs)
    assert rows * rs < lc.FRAME_LIMIT <= (rows + 1) * rs
    src = lc.pixels(16, rows, lc.STRIDE_W, c, dtype)
    Minv, dsize = lc.stride_map(rows), lc.STRIDE_DSIZE
    holder = view = None
    try:
        holder = (byte_holder if dtype == np.uint8 else nan_holder)(lc.source_reach(rows, lc.STRIDE_W, c, esz, rs))
        view = strided(holder, dtype, (rows, lc.STRIDE_W, c), (rs, c * esz, esz))
        view.copy_(dev(src))
        maps = both_maps(Minv, dsize)
        assert (maps[1].of(0)[0][..., 1] == rows - 1).any()  # the last row: the largest offset
        run_remap(view, src, maps, (RR.CONSTANT, RR.REFLECT_101))
        lens = stride_lens(rows)
        run_lens(view, src, Minv, dsize, lens)
        run_remap(view, src, both_maps(lens[3], dsize, lens[:3]), (RR.CONSTANT,))
        if dtype == np.uint8 and c == 3:
            run_bgr_to_nv12(view, src, Minv, maps, (RR.CONSTANT, RR.WRAP))
            run_bgr_to_planar(view, src, maps, (RR.CONSTANT, RR.REFLECT))
        second = lc.pixels(17, lc.BIG_SRC_HW[0], lc.BIG_SRC_HW[1], c, dtype)
        run_stitch([view, dev(second)], [src, second], [Minv, SECOND_CAMERA], dsize)
        # one past either limit: refused before anything is launched
        lib, m = _lib.load(), maps[1].dev
        out = px_out(None, view, dsize, 0)
        dw, dh = dsize
        minv = W.device_inverse(Minv, view.device, inverse_given=True)
        K, dist, _, _ = lens
        lens12 = np.ascontiguousarray(LR.lens12(K, dist), dtype=np.float64)

        def remap_status(n_rows, stride):
            return lib.bevwarp_remap(view.data_ptr(), out.data_ptr(), 1, n_rows, lc.STRIDE_W, dh, dw, c, 0, stride, 0, dw * c * esz, m.xy.data_ptr(), m.frac.data_ptr(), 1, 0,
                                     dw * 4, 0, dw * 2, W._DTYPES[view.dtype], LINEAR, 0, None, None)

        def lens_status(n_rows, stride):
            return lib.bevwarp_warp_lens(view.data_ptr(), out.data_ptr(), 1, n_rows, lc.STRIDE_W, dh, dw, c, 0, stride, 0, dw * c * esz, minv.data_ptr(), 1,
                                         lens12.ctypes.data_as(ctypes.c_void_p), float("inf"), W._DTYPES[view.dtype], LINEAR, 0, None, None)
        assert (rows - 1) * lc.ROW_LIMIT < lc.FRAME_LIMIT
        for status in (remap_status, lens_status):
            assert status(rows, rs) == 0  # (the admitted call itself, as the raw symbol takes it: the refusals below are the sizes')
            torch.cuda.synchronize()
            assert not bool((out == 77).all().item())
            fill(out)
            assert status(rows + 1, rs) == TOO_LARGE and status(rows - 1, lc.ROW_LIMIT) == TOO_LARGE
        torch.cuda.synchronize()
        assert bool((out == 77).all().item())
    finally:
        del holder, view
        torch.cuda.empty_cache()


def test_largest_row_stride_nv12():
    """Case C for NV12: Y rows 2^24 - 1 bytes apart (128 rows) and pair rows 2^24 - 2 bytes apart (64 rows), the largest the checks admit,
    each plane in a holder of its own (2 GiB and 1 GiB).  One row more or a stride of 2^24 in EITHER plane is BEVWARP_ERR_TOO_LARGE."""
    (y_rs, rows), (uv_rs, uv_rows) = lc.STRIDE_NV12["y"], lc.STRIDE_NV12["uv"]
    w = lc.STRIDE_W
    hy, huv = NR.frame("phase", 18, rows, w)
    Minv, dsize = lc.stride_map(rows), lc.STRIDE_DSIZE
    y_holder = uv_holder = y = uv = None
    try:
        y_holder, uv_holder = byte_holder(lc.source_reach(rows, w, 1, 1, y_rs)), byte_holder(lc.source_reach(uv_rows, w, 1, 1, uv_rs))
        y, uv = strided(y_holder, np.uint8, (rows, w), (y_rs, 1)), strided(uv_holder, np.uint8, (uv_rows, w // 2, 2), (uv_rs, 2, 1))
        y.copy_(dev(hy)), uv.copy_(dev(huv))
        maps = both_maps(Minv, dsize)
        run_nv12_to_px(y, uv, hy, huv, Minv, maps, (RR.CONSTANT, RR.REFLECT_101))
        run_nv12_to_planar(y, uv, hy, huv, Minv, maps, (RR.CONSTANT, RR.WRAP))
        run_nv12_to_nv12(y, uv, hy, huv, Minv, maps, (RR.CONSTANT, RR.REFLECT))
        second = NR.frame("phase", 19, *lc.BIG_SRC_HW)
        run_stitch_nv12([y, dev(second[0])], [uv, dev(second[1])], [hy, second[0]], [huv, second[1]], [Minv, SECOND_CAMERA], dsize)
        lib, m = _lib.load(), maps[1].dev
        out = px_out(None, torch.empty((1, 1, 3), dtype=torch.uint8), dsize, 0)
        dw, dh = dsize

        def status(n_rows, ys, uvs):
            return lib.bevwarp_remap_nv12(y.data_ptr(), uv.data_ptr(), out.data_ptr(), 1, n_rows, w, dh, dw, 0, ys, 0, uvs, 0, dw * 3, m.xy.data_ptr(), m.frac.data_ptr(), 1,
                                          0, dw * 4, 0, dw * 2, LINEAR, 0, 0, None, None)
        assert status(rows, y_rs, uv_rs) == 0          # (the admitted call itself, as the raw symbol takes it)
        torch.cuda.synchronize()
        fill(out)
        assert status(rows + 2, y_rs, uv_rs) == TOO_LARGE                       # the Y plane: 130 rows pass 2^31 (the pair plane's 65 do not)
        assert status(rows - 2, lc.ROW_LIMIT, uv_rs) == TOO_LARGE and (rows - 2) * lc.ROW_LIMIT < lc.FRAME_LIMIT
        assert status(rows, y_rs, lc.ROW_LIMIT) == TOO_LARGE and uv_rows * lc.ROW_LIMIT < lc.FRAME_LIMIT  # the pair plane alone
        torch.cuda.synchronize()
        assert bool((out == 77).all().item())
    finally:
        del y_holder, uv_holder, y, uv
        torch.cuda.empty_cache()


# ---- D: frames, planes and maps beyond 4 GiB ---------------------------------------------------------------------------------------------------------
def big_matrices():
    return np.stack([lc.jittered_inverse(lc.big_map(), i) for i in range(lc.BIG_BATCH)])


def big_frames(dtype, c, seed=20):
    h, w = lc.BIG_SRC_HW
    return np.stack([lc.pixels(seed + i, h, w, c, dtype) for i in range(lc.BIG_BATCH)])


def big_nv12(seed=24):
    planes = [NR.frame("phase", seed + i, *lc.BIG_SRC_HW) for i in range(lc.BIG_BATCH)]
    return np.stack([p[0] for p in planes]), np.stack([p[1] for p in planes])


@pytest.mark.parametrize("dtype,c", [(np.uint8, 3), (np.float32, 1)], ids=["uint8x3", "float32x1"])
def test_source_frames_beyond_4gib_interleaved(dtype, c):
    """Case D: three source frames 2^32 + 4096 bytes apart, a matrix and a map per frame, compact destinations."""
    esz = np.dtype(dtype).itemsize
    src, Ms = big_frames(dtype, c), big_matrices()
    B, h, w, _ = src.shape
    holder = view = None
    try:
        holder = (byte_holder if dtype == np.uint8 else nan_holder)(lc.source_reach(h, w, c, esz, w * c * esz, B, lc.BEYOND_4G))
        view = strided(holder, dtype, (B, h, w, c), (lc.BEYOND_4G, w * c * esz, c * esz, esz))
        view.copy_(dev(src))
        assert view[2].data_ptr() - view.data_ptr() == 2 * lc.BEYOND_4G
        maps = both_maps(Ms, lc.BIG_DSIZE)
        assert maps[0].dev.n == B
        run_remap(view, src, maps, (RR.CONSTANT, RR.REFLECT_101, RR.TRANSPARENT))
        K, dist, _ = lc.mild_lens((h, w))
        run_lens(view, src, Ms, lc.BIG_DSIZE, (K, dist, float("inf"), Ms))
        if dtype == np.uint8:
            run_bgr_to_nv12(view, src, Ms, maps, (RR.CONSTANT, RR.WRAP))
            run_bgr_to_planar(view, src, maps, (RR.CONSTANT, RR.REFLECT))
    finally:
        del holder, view
        torch.cuda.empty_cache()


def test_source_frames_beyond_4gib_nv12():
    """Case D for NV12: three joined frames (Y rows, then the pair rows) 2^32 + 4096 bytes apart -- one frame stride for both planes."""
    hy, huv = big_nv12()
    B, h, w = hy.shape
    Ms = big_matrices()
    lay = lc.nv12_joined(B, h, w, lc.BEYOND_4G)
    holder = y = uv = None
    try:
        holder = byte_holder(lay["bytes"])
        y, uv = strided(holder, np.uint8, *lay["y"]), strided(holder, np.uint8, *lay["uv"])
        y.copy_(dev(hy)), uv.copy_(dev(huv))
        assert y[2].data_ptr() - y.data_ptr() == uv[2].data_ptr() - uv.data_ptr() == 2 * lc.BEYOND_4G and uv.data_ptr() - y.data_ptr() == h * w
        maps = both_maps(Ms, lc.BIG_DSIZE)
        run_nv12_to_px(y, uv, hy, huv, Ms, maps, (RR.CONSTANT, RR.REFLECT_101, RR.TRANSPARENT))
        run_nv12_to_planar(y, uv, hy, huv, Ms, maps, (RR.CONSTANT, RR.WRAP))
        run_nv12_to_nv12(y, uv, hy, huv, Ms, maps, (RR.CONSTANT, RR.REFLECT))
    finally:
        del holder, y, uv
        torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype,c", [(np.uint8, 3), (np.float32, 1)], ids=["uint8x3", "float32x1"])
def test_destination_frames_beyond_4gib_interleaved(dtype, c):
    """Case D reversed: compact sources, interleaved destination frames 2^32 + 4096 bytes apart for bevwarp_warp_lens, _remap, _warp_nv12
    and _remap_nv12; nothing but the three frames is written."""
    esz = np.dtype(dtype).itemsize
    src, Ms = big_frames(dtype, c), big_matrices()
    dw, dh = lc.BIG_DSIZE
    t = dev(src)
    holder = out = None
    try:
        holder = byte_holder(lc.dest_reach(dh, dw, c, esz, dw * c * esz, lc.BIG_BATCH, lc.BEYOND_4G))
        out = strided(holder, dtype, (lc.BIG_BATCH, dh, dw, c), (lc.BEYOND_4G, dw * c * esz, c * esz, esz))
        maps = both_maps(Ms, lc.BIG_DSIZE)
        run_remap(t, src, maps, (RR.CONSTANT, RR.REPLICATE, RR.TRANSPARENT), out=out)
        K, dist, _ = lc.mild_lens(lc.BIG_SRC_HW)
        run_lens(t, src, Ms, lc.BIG_DSIZE, (K, dist, float("inf"), Ms), out=out)
        if dtype == np.uint8:
            hy, huv = big_nv12()
            run_nv12_to_px(dev(hy), dev(huv), hy, huv, Ms, maps, (RR.CONSTANT, RR.REFLECT, RR.TRANSPARENT), out=out)
        assert_only_the_view_was_written(holder, out, "interleaved destination frames beyond 4 GiB")
    finally:
        del holder, out
        torch.cuda.empty_cache()


def test_destination_frames_beyond_4gib_nv12():
    """Case D, NV12 destinations: three joined frames 2^32 + 4096 bytes apart, written by the four entries into NV12; written_planes_overlap
    admits the layout (a refused call raises), and nothing but the Y and pair rows is written."""
    src, Ms = big_frames(np.uint8, 3), big_matrices()
    hy, huv = big_nv12()
    dw, dh = lc.BIG_DSIZE
    lay = lc.nv12_joined(lc.BIG_BATCH, dh, dw, lc.BEYOND_4G)
    holder = out = None
    try:
        holder = byte_holder(lay["bytes"])
        out = (strided(holder, np.uint8, *lay["y"]), strided(holder, np.uint8, *lay["uv"]))
        maps = both_maps(Ms, lc.BIG_DSIZE)
        run_bgr_to_nv12(dev(src), src, Ms, maps, (RR.CONSTANT, RR.REFLECT_101), out=out)
        run_nv12_to_nv12(dev(hy), dev(huv), hy, huv, Ms, maps, (RR.CONSTANT, RR.WRAP), out=out)
        assert_only_the_view_was_written(holder, out, "NV12 destination frames beyond 4 GiB")
    finally:
        del holder, out
        torch.cuda.empty_cache()


@pytest.mark.parametrize("plane_dtype", PLANE_DTYPES, ids=["float32", "float16"])
def test_planes_beyond_4gib_entries(plane_dtype):
    """Case D, planar: three channel planes 2^32 + 4096 bytes apart for bevwarp_remap_planes, _warp_nv12_planes, _remap_nv12_planes and
    bevwarp_stitch_maps_planes (single frames: the plane term alone is large)."""
    h, w = lc.BIG_SRC_HW
    dw, dh = lc.BIG_DSIZE
    esz = 4 if plane_dtype == torch.float32 else 2
    src, Minv = lc.pixels(30, h, w, 3, np.uint8), lc.big_map()
    hy, huv = NR.frame("phase", 31, h, w)
    holder = out = None
    try:
        holder = byte_holder(lc.dest_reach(dh, dw, 3, esz, dw * esz, planes=3, ps=lc.BEYOND_4G))
        out = strided(holder, plane_dtype, (3, dh, dw), (lc.BEYOND_4G, dw * esz, esz))
        assert out[2].data_ptr() - out.data_ptr() == 2 * lc.BEYOND_4G
        maps = both_maps(Minv, lc.BIG_DSIZE)
        run_bgr_to_planar(dev(src), src, maps, (RR.CONSTANT, RR.REFLECT_101), (plane_dtype,), out_of=lambda _: out)
        run_nv12_to_planar(dev(hy), dev(huv), hy, huv, Minv, maps, (RR.CONSTANT, RR.WRAP), (plane_dtype,), out_of=lambda _: out)
        second = lc.pixels(32, h, w, 3, np.uint8)
        for interp in (NEAREST, LINEAR):
            two = [Maps(M, lc.BIG_DSIZE, interp) for M in (Minv, lc.jittered_inverse(Minv, 1, px=9.0))]
            for blend, ref_blend in BLENDS:
                planes = MP.stitch_planes([src, second], [m.of(0) for m in two], interp, SCALE, BIAS, ref_blend, FEATHER, lc.BORDER[:3])
                fill(out)
                got = W.remap_stitch_to_planar([dev(src), dev(second)], [m.dev for m in two], scale=SCALE, bias=BIAS, blend=blend, feather=FEATHER, border_value=lc.BORDER[:3],
                                               out=out, out_dtype=plane_dtype)
                assert got is out
                same_planes(out, planes, plane_dtype)
        assert_only_the_view_was_written(holder, out, "planes beyond 4 GiB")
    finally:
        del holder, out
        torch.cuda.empty_cache()


@pytest.mark.parametrize("plane_dtype", PLANE_DTYPES, ids=["float32", "float16"])
def test_plane_frames_beyond_4gib(plane_dtype):
    """Case D, planar destinations of a batch: three frames of three compact planes, the FRAMES 2^32 + 4096 bytes apart, for
    bevwarp_remap_planes, bevwarp_warp_nv12_planes and bevwarp_remap_nv12_planes with a matrix and a map per frame."""
    dw, dh = lc.BIG_DSIZE
    esz = 4 if plane_dtype == torch.float32 else 2
    src, Ms = big_frames(np.uint8, 3), big_matrices()
    hy, huv = big_nv12()
    holder = out = None
    try:
        holder = byte_holder(lc.dest_reach(dh, dw, 3, esz, dw * esz, lc.BIG_BATCH, lc.BEYOND_4G, planes=3, ps=dh * dw * esz))
        out = strided(holder, plane_dtype, (lc.BIG_BATCH, 3, dh, dw), (lc.BEYOND_4G, dh * dw * esz, dw * esz, esz))
        assert out[2].data_ptr() - out.data_ptr() == 2 * lc.BEYOND_4G
        maps = both_maps(Ms, lc.BIG_DSIZE)
        run_bgr_to_planar(dev(src), src, maps, (RR.CONSTANT, RR.REPLICATE), (plane_dtype,), out_of=lambda _: out)
        run_nv12_to_planar(dev(hy), dev(huv), hy, huv, Ms, maps, (RR.CONSTANT, RR.REFLECT), (plane_dtype,), out_of=lambda _: out)
        assert_only_the_view_was_written(holder, out, "plane frames beyond 4 GiB")
    finally:
        del holder, out
        torch.cuda.empty_cache()


def run_stitch_frames(ts, srcs, Minvs, dsize, out=None, nv12=None):
    """The stitches of a BATCH, a matrix and a map per frame and camera, both blends, nearest and bilinear.  Interleaved 8-bit x3 cameras
    (ts, srcs): bevwarp_warp_stitch and bevwarp_stitch_maps into `out` (or a compact destination), and into compact destinations
    bevwarp_stitch_maps_to_nv12 and _planes.  nv12 = (ys, uvs, hys, huvs): bevwarp_stitch_maps_nv12 into `out`, and into compact
    destinations bevwarp_stitch_maps_nv12_to_nv12 and _nv12_planes."""
    B = Minvs[0].shape[0]
    like = torch.empty((1, 1, 3), dtype=torch.uint8)
    for interp in (NEAREST, LINEAR):
        maps = [Maps(M, dsize, interp) for M in Minvs]
        dmaps = [m.dev for m in maps]
        for blend, ref_blend in BLENDS:
            if nv12 is None:
                exp = np.stack([SM.stitch([s[i] for s in srcs], [m.of(i) for m in maps], interp, ref_blend, FEATHER, SM.CONSTANT, lc.BORDER[:3])[0] for i in range(B)])
                exp_w = np.stack([SR.stitch([s[i] for s in srcs], [M[i] for M in Minvs], dsize, interp, ref_blend, FEATHER, SR.CONSTANT, lc.BORDER[:3])[0] for i in range(B)])
                o = px_out(out, like, dsize, B)
                assert W.warp_stitch(ts, Minvs, dsize, flags=interp | INV, blend=blend, feather=FEATHER, border_value=lc.BORDER[:3], out=o) is o
                same(o.cpu().numpy(), exp_w)
                o = px_out(out, like, dsize, B)
                assert W.remap_stitch(ts, dmaps, blend=blend, feather=FEATHER, border_value=lc.BORDER[:3], out=o) is o
                same(o.cpu().numpy(), exp)
                if out is None:
                    o = nv12_out(None, dsize, B)
                    W.remap_stitch_to_nv12(ts, dmaps, blend=blend, feather=FEATHER, border_value=lc.BORDER[:3], out=o)
                    same_nv12(o, [NO.bgr_to_nv12(e) for e in exp])
                    got = W.remap_stitch_to_planar(ts, dmaps, scale=SCALE, bias=BIAS, blend=blend, feather=FEATHER, border_value=lc.BORDER[:3])
                    same_planes(got, np.stack([RN.planes_f32(e, SCALE, BIAS) for e in exp]), torch.float32)
            else:
                ys, uvs, hys, huvs = nv12
                exp = np.stack([SM.stitch_nv12([a[i] for a in hys], [a[i] for a in huvs], [m.of(i) for m in maps], interp, ref_blend, FEATHER, SM.CONSTANT, lc.BORDER[:3])[0]
                                for i in range(B)])
                o = px_out(out, like, dsize, B)
                assert W.remap_stitch_nv12(ys, uvs, dmaps, blend=blend, feather=FEATHER, border_value=lc.BORDER[:3], out=o) is o
                same(o.cpu().numpy(), exp)
                if out is None:
                    o = nv12_out(None, dsize, B)
                    W.remap_stitch_nv12_to_nv12(ys, uvs, dmaps, blend=blend, feather=FEATHER, border_value=lc.BORDER[:3], out=o)
                    same_nv12(o, [NO.bgr_to_nv12(e) for e in exp])
                    got = W.remap_stitch_nv12_to_planar(ys, uvs, dmaps, scale=SCALE, bias=BIAS, blend=blend, feather=FEATHER, border_value=lc.BORDER[:3])
                    same_planes(got, np.stack([RN.planes_f32(e, SCALE, BIAS) for e in exp]), torch.float32)


def second_camera_matrices():
    return np.stack([lc.jittered_inverse(lc.big_map(), i + 1, px=9.0) for i in range(lc.BIG_BATCH)])


@pytest.mark.parametrize("kind", ["uint8x3", "nv12"])
def test_stitch_camera_frames_beyond_4gib(kind):
    """Case D for the stitches: the first camera's frames 2^32 + 4096 bytes apart (NV12: joined frames, one stride for both planes), a
    compact second camera, a matrix and a map per frame -- the per-camera frame term of all seven stitch kernels."""
    Ms = [big_matrices(), second_camera_matrices()]
    holder = view = uv = None
    try:
        if kind == "uint8x3":
            src, second = big_frames(np.uint8, 3), big_frames(np.uint8, 3, seed=33)
            B, h, w, _ = src.shape
            holder = byte_holder(lc.source_reach(h, w, 3, 1, w * 3, B, lc.BEYOND_4G))
            view = strided(holder, np.uint8, (B, h, w, 3), (lc.BEYOND_4G, w * 3, 3, 1))
            view.copy_(dev(src))
            run_stitch_frames([view, dev(second)], [src, second], Ms, lc.BIG_DSIZE)
        else:
            (hy, huv), (hy2, huv2) = big_nv12(), big_nv12(seed=36)
            B, h, w = hy.shape
            lay = lc.nv12_joined(B, h, w, lc.BEYOND_4G)
            holder = byte_holder(lay["bytes"])
            view, uv = strided(holder, np.uint8, *lay["y"]), strided(holder, np.uint8, *lay["uv"])
            view.copy_(dev(hy)), uv.copy_(dev(huv))
            run_stitch_frames(None, None, Ms, lc.BIG_DSIZE, nv12=([view, dev(hy2)], [uv, dev(huv2)], [hy, hy2], [huv, huv2]))
        assert view[2].data_ptr() - view.data_ptr() == 2 * lc.BEYOND_4G
    finally:
        del holder, view, uv
        torch.cuda.empty_cache()


def test_stitch_destination_frames_beyond_4gib():
    """Case D for the stitches, reversed: compact cameras, the canvas frames 2^32 + 4096 bytes apart, for bevwarp_warp_stitch,
    bevwarp_stitch_maps and bevwarp_stitch_maps_nv12; nothing but the three canvases is written."""
    Ms = [big_matrices(), second_camera_matrices()]
    src, second = big_frames(np.uint8, 3), big_frames(np.uint8, 3, seed=33)
    (hy, huv), (hy2, huv2) = big_nv12(), big_nv12(seed=36)
    dw, dh = lc.BIG_DSIZE
    holder = out = None
    try:
        holder = byte_holder(lc.dest_reach(dh, dw, 3, 1, dw * 3, lc.BIG_BATCH, lc.BEYOND_4G))
        out = strided(holder, np.uint8, (lc.BIG_BATCH, dh, dw, 3), (lc.BEYOND_4G, dw * 3, 3, 1))
        run_stitch_frames([dev(src), dev(second)], [src, second], Ms, lc.BIG_DSIZE, out=out)
        run_stitch_frames(None, None, Ms, lc.BIG_DSIZE, out=out, nv12=([dev(hy), dev(hy2)], [dev(huv), dev(huv2)], [hy, hy2], [huv, huv2]))
        assert_only_the_view_was_written(holder, out, "stitched canvases beyond 4 GiB")
    finally:
        del holder, out
        torch.cuda.empty_cache()


def map_views(holder, interp, n, dsize, xy_spec, frac_spec):
    """A WarpMap whose planes are views of `holder`; a spec is (strides in bytes of (frame, row), byte offset)."""
    dw, dh = dsize
    xy = strided(holder, torch.int16, (n, dh, dw, 2), (xy_spec[0][0], xy_spec[0][1], 4, 2), xy_spec[1])
    frac = None if interp == NEAREST else strided(holder, torch.int16, (n, dh, dw), (frac_spec[0][0], frac_spec[0][1], 2), frac_spec[1])
    return W.WarpMap(xy, frac, interp, dsize)


def test_map_planes_beyond_4gib():
    """Case D for the maps: per-frame map planes 2^32 + 4096 bytes apart, WRITTEN by bevwarp_build_map with three matrices and READ by
    bevwarp_remap and bevwarp_remap_nv12 with map_count == batch.  xy and frac share one holder: rows of both 4096 bytes apart (the frame
    stride is a multiple of it), frac beside xy in every row -- the side-by-side layout the builder's overlap check admits."""
    src, Ms = big_frames(np.uint8, 3), big_matrices()
    hy, huv = big_nv12()
    dw, dh = lc.BIG_DSIZE
    B, rs = lc.BIG_BATCH, 4096
    frac_off = dw * 4 + 32
    assert lc.BEYOND_4G % rs == 0 and frac_off + dw * 2 <= rs and frac_off % 8 == 0
    holder = m = None
    try:
        holder = byte_holder((B - 1) * lc.BEYOND_4G + dh * rs)
        for interp in (NEAREST, LINEAR):
            m = map_views(holder, interp, B, lc.BIG_DSIZE, ((lc.BEYOND_4G, rs), 0), ((lc.BEYOND_4G, rs), frac_off))
            assert m.xy[2].data_ptr() - m.xy.data_ptr() == 2 * lc.BEYOND_4G
            built = Maps(Ms, lc.BIG_DSIZE, interp, out=m)
            assert built.dev is m
            run_remap(dev(src), src, [built], (RR.CONSTANT, RR.REFLECT_101))
            run_nv12_to_px(dev(hy), dev(huv), hy, huv, Ms, [built], (RR.CONSTANT, RR.WRAP))
            assert_only_the_view_was_written(holder, [m.xy] + ([] if m.frac is None else [m.frac]), "map planes beyond 4 GiB")
    finally:
        del holder, m
        torch.cuda.empty_cache()


# ---- E: rows beyond 4 GiB inside one image -----------------------------------------------------------------------------------------------------------
ROWS_DSIZE = (lc.BIG_DSIZE[0], lc.ROWS_PAST_4G5)


@pytest.mark.parametrize("dtype,c", [(np.uint8, 3), (np.float32, 1)], ids=["uint8x3", "float32x1"])
def test_destination_rows_beyond_4gib_entries(dtype, c):
    """Case E, interleaved: destination rows 2^26 bytes apart, the last one beyond 4.5 GiB, for bevwarp_warp_lens, _remap, _warp_stitch and
    _stitch_maps; the stretch after every row keeps its canaries."""
    esz = np.dtype(dtype).itemsize
    h, w = lc.BIG_SRC_HW
    dw, dh = ROWS_DSIZE
    src, Minv = lc.pixels(40, h, w, c, dtype), lc.big_map()
    t = dev(src)
    holder = out = None
    try:
        holder = byte_holder(lc.dest_reach(dh, dw, c, esz, lc.ROW_64M))
        out = strided(holder, dtype, (dh, dw, c), (lc.ROW_64M, c * esz, esz))
        assert out[dh - 1].data_ptr() - out.data_ptr() > 4.5 * (1 << 30)
        maps = both_maps(Minv, ROWS_DSIZE)
        run_remap(t, src, maps, (RR.CONSTANT, RR.REFLECT_101, RR.TRANSPARENT), out=out)
        K, dist, _ = lc.mild_lens((h, w))
        run_lens(t, src, Minv, ROWS_DSIZE, (K, dist, float("inf"), Minv), out=out)
        second = lc.pixels(41, h, w, c, dtype)
        run_stitch([t, dev(second)], [src, second], [Minv, lc.jittered_inverse(Minv, 1, px=9.0)], ROWS_DSIZE, out=out, kinds=("px",))
        assert_only_the_view_was_written(holder, out, "destination rows beyond 4 GiB")
    finally:
        del holder, out
        torch.cuda.empty_cache()


def test_nv12_destination_rows_beyond_4gib():
    """Case E for NV12 destinations: Y rows 2^26 bytes apart and the pair rows beside them in the same stretches (one holder); the four
    single-camera entries into NV12 and the stitch into NV12."""
    h, w = lc.BIG_SRC_HW
    dw, dh = ROWS_DSIZE
    src, Minv = lc.pixels(42, h, w, 3, np.uint8), lc.big_map()
    hy, huv = NR.frame("phase", 43, h, w)
    lay = lc.nv12_beside(dh, dw, lc.ROW_64M, 1024)
    holder = out = None
    try:
        holder = byte_holder(lay["bytes"])
        out = (strided(holder, np.uint8, *lay["y"]), strided(holder, np.uint8, *lay["uv"]))
        assert out[0][dh - 1].data_ptr() - out[0].data_ptr() > 4.5 * (1 << 30) and out[1].data_ptr() - out[0].data_ptr() == 1024
        maps = both_maps(Minv, ROWS_DSIZE)
        run_bgr_to_nv12(dev(src), src, Minv, maps, (RR.CONSTANT, RR.REFLECT_101), out=out)
        run_nv12_to_nv12(dev(hy), dev(huv), hy, huv, Minv, maps, (RR.CONSTANT, RR.WRAP), out=out)
        second = lc.pixels(44, h, w, 3, np.uint8)
        run_stitch([dev(src), dev(second)], [src, second], [Minv, lc.jittered_inverse(Minv, 1, px=9.0)], ROWS_DSIZE, nv12_out_=out, kinds=("nv12",))
        assert_only_the_view_was_written(holder, out, "NV12 destination rows beyond 4 GiB")
    finally:
        del holder, out
        torch.cuda.empty_cache()


def test_map_rows_beyond_4gib():
    """Case E for the maps: map rows 2^26 bytes apart, xy and frac beside each other in one holder, built by bevwarp_build_map and read by
    bevwarp_remap and bevwarp_stitch_maps."""
    h, w = lc.BIG_SRC_HW
    dw, dh = ROWS_DSIZE
    src, Minv = lc.pixels(47, h, w, 3, np.uint8), lc.big_map()
    second = lc.pixels(48, h, w, 3, np.uint8)
    frac_off = dw * 4 + 64
    holder = m = None
    try:
        holder = byte_holder((dh - 1) * lc.ROW_64M + frac_off + dw * 2)
        for interp in (NEAREST, LINEAR):
            m = map_views(holder, interp, 1, ROWS_DSIZE, ((dh * lc.ROW_64M, lc.ROW_64M), 0), ((dh * lc.ROW_64M, lc.ROW_64M), frac_off))
            assert m.xy[0, dh - 1].data_ptr() - m.xy.data_ptr() > 4.5 * (1 << 30)
            built = Maps(Minv, ROWS_DSIZE, interp, out=m)
            run_remap(dev(src), src, [built], (RR.CONSTANT, RR.REFLECT_101))
            for blend, ref_blend in BLENDS:
                exp, _ = SM.stitch([src, second], [built.of(0), built.of(0)], interp, ref_blend, FEATHER, SM.CONSTANT, lc.BORDER[:3])
                got = W.remap_stitch([dev(src), dev(second)], [m, m], blend=blend, feather=FEATHER, border_value=lc.BORDER[:3])
                same(got.cpu().numpy(), exp)
            assert_only_the_view_was_written(holder, [m.xy] + ([] if m.frac is None else [m.frac]), "map rows beyond 4 GiB")
    finally:
        del holder, m
        torch.cuda.empty_cache()


# ---- F: item decoding at the edge of fast_div's exactness --------------------------------------------------------------------------------------------
DECODE_DH = lc.DECODE_TILES * 4  # flat tiles are 256 x 4


@pytest.fixture(scope="module")
def flat_plan():
    """plan_border's grid for a batch (tests/host_plan_driver.cpp, built plainly): the plan of every flat-grid entry."""
    exe = hostplan.build_driver(sanitize=False)

    def plan(batch, dw):
        r = subprocess.run([exe, "plan"], input="border %d %d %d 256 4 %d %d %d\n" % (batch, DECODE_DH, dw, br.REPLICATE, lc.DECODE_SRC_HW[0], lc.DECODE_SRC_HW[1]),
                           capture_output=True, text=True, timeout=60, check=True)
        v = [int(x) for x in r.stdout.split()]
        return dict(status=v[0], tile_h=v[1], tiles_per_frame=v[3], total_tiles=v[4], tpf_magic=v[9])
    return plan


@pytest.fixture(scope="module")
def remap_plan():
    """plan_remap (tests/host_plan_driver.cpp's `remap` family, built plainly) with the library's bounds: at most BEVWARP_REMAP_MAX_FPI
    frames per item, 4096 items to fill."""
    exe = hostplan.build_driver(sanitize=False)

    def plan(batch, map_count, dw):
        r = subprocess.run([exe, "remap"], input="plan %d %d %d %d 2 4096\n" % (batch, map_count, DECODE_DH, dw), capture_output=True, text=True, timeout=60, check=True)
        v = [int(x) for x in r.stdout.split()]
        return dict(status=v[0], frames_per_item=v[1], groups=v[2], total_tiles=v[3], covered=v[4])
    return plan


def assert_straddle(flat_plan, counts, dw):
    """The two item counts lie on either side of the bound: a magic below it, 0 (the kernel divides) above."""
    lo, hi = (flat_plan(n, dw) for n in counts)
    for p, n in ((lo, counts[0]), (hi, counts[1])):
        assert p["status"] == 0 and p["tile_h"] == 4 and p["tiles_per_frame"] == lc.DECODE_TILES and p["total_tiles"] == n * lc.DECODE_TILES
    n_lo, n_hi = lo["total_tiles"] * lc.DECODE_TILES, hi["total_tiles"] * lc.DECODE_TILES
    assert n_lo < 1 << 32 <= n_hi and (1 << 32) - n_lo < (1 << 32) // 100 and lo["tpf_magic"] != 0 and hi["tpf_magic"] == 0


def decode_batch(B, dh=DECODE_DH):
    h, w = lc.DECODE_SRC_HW
    src = np.stack([lc.pixels(50 + i, h, w, 3, np.uint8) for i in range(B)])
    # a matrix per frame: decode_map's, a fraction of a source pixel further along both axes frame by frame (every frame stays in its source)
    return src, np.stack([lc.affine(20.0, 2.2 + 0.37 * i, 61.0 / (dh - 1), 0.6 + 0.21 * i) for i in range(B)])


def differ_pairwise(exp):
    return all(not np.array_equal(exp[i], exp[j]) for i in range(len(exp)) for j in range(i))


@pytest.mark.parametrize("entry", ["lens", "nv12", "to_nv12"])
def test_item_decoding_flat_entries(flat_plan, entry):
    """Case F through the flat grid of bevwarp_warp_lens, _warp_nv12 and _warp_to_nv12: 37747 tiles per frame, 3 frames (a multiply-high
    decodes the items) and 4 (the kernel divides).  Every frame has its own content and matrix: a quotient off by one moves a tile into
    another frame."""
    dw = lc.DECODE_DW_EVEN if entry == "to_nv12" else lc.DECODE_DW
    dsize = (dw, DECODE_DH)
    assert_straddle(flat_plan, lc.DECODE_BATCHES, dw)
    for B in lc.DECODE_BATCHES:
        src, Ms = decode_batch(B)
        if entry == "lens":
            K, dist, _ = lc.mild_lens(lc.DECODE_SRC_HW)
            got = W.warp_perspective_lens(dev(src), Ms, dsize, K, dist, flags=LINEAR | INV, border_value=lc.BORDER[:3], r2_max=float("inf"))
            exp = np.stack([LR.warp(f, LR.ray_matrix(M, K, inverse_given=True), LR.lens12(K, dist), float("inf"), dsize, LINEAR, LR.CONSTANT, lc.BORDER[:3])
                            for f, M in zip(src, Ms)])
            assert differ_pairwise(exp)
            np.testing.assert_array_equal(got.cpu().numpy(), exp)
        elif entry == "nv12":
            planes = [NR.frame("phase", 55 + i, *lc.DECODE_SRC_HW) for i in range(B)]
            hy, huv = np.stack([p[0] for p in planes]), np.stack([p[1] for p in planes])
            got = W.warp_perspective_nv12(dev(hy), dev(huv), Ms, dsize, flags=LINEAR | INV, border_value=lc.BORDER[:3])
            exp = np.stack([NR.warp_nv12(a, b, M, dsize, co.LINEAR, border_value=lc.BORDER[:3], m_is_inverse=True, nthreads=8) for a, b, M in zip(hy, huv, Ms)])
            assert differ_pairwise(exp)
            np.testing.assert_array_equal(got.cpu().numpy(), exp)
        else:
            o = nv12_out(None, dsize, B)
            W.warp_perspective_to_nv12(dev(src), Ms, dsize, flags=LINEAR | INV, border_value=lc.BORDER[:3], out=o)
            exp = [NO.warp_to_nv12(f, M, dsize, co.LINEAR, border_value=lc.BORDER[:3], m_is_inverse=True, nthreads=8) for f, M in zip(src, Ms)]
            assert differ_pairwise([e[0] for e in exp])
            same_nv12(o, exp)


def test_item_decoding_stitch(flat_plan):
    """Case F through bevwarp_warp_stitch, two cameras: the same two batches."""
    dsize = (lc.DECODE_DW, DECODE_DH)
    assert_straddle(flat_plan, lc.DECODE_BATCHES, lc.DECODE_DW)
    for B in lc.DECODE_BATCHES:
        src, Ms = decode_batch(B)
        second = src[::-1].copy()
        M2 = np.stack([M @ np.diag([1.0, 2.0, 1.0]) for M in Ms])  # twice as fast down its source: the upper half of the canvas only
        got = W.warp_stitch([dev(src), dev(second)], [Ms, M2], dsize, flags=LINEAR | INV, blend="feather", feather=FEATHER, border_value=lc.BORDER[:3])
        exp = np.stack([SR.stitch([src[i], second[i]], [Ms[i], M2[i]], dsize, LINEAR, SR.FEATHER, FEATHER, SR.CONSTANT, lc.BORDER[:3])[0] for i in range(B)])
        assert differ_pairwise(exp)
        np.testing.assert_array_equal(got.cpu().numpy(), exp)


def test_item_decoding_maps(flat_plan, remap_plan):
    """Case F through bevwarp_build_map (3 and 4 maps) and bevwarp_remap: per-frame maps (3 and 4 frames, one frame per item), and ONE
    shared map with 6 and 7 frames -- two frames per item, so 3 and 4 groups, the second with a short last group."""
    dsize = (lc.DECODE_DW, DECODE_DH)
    assert_straddle(flat_plan, lc.DECODE_BATCHES, lc.DECODE_DW)
    for B in lc.DECODE_BATCHES:
        p = remap_plan(B, B, lc.DECODE_DW)
        assert p == dict(status=0, frames_per_item=1, groups=B, total_tiles=B * lc.DECODE_TILES, covered=1)
        src, Ms = decode_batch(B)
        m = Maps(Ms, dsize, LINEAR)  # (the builder's own decoding: its contents against the reference, map by map)
        got = W.remap(dev(src), m.dev, border_mode=RR.REPLICATE)
        exp = np.stack([RR.remap(f, *m.of(i), LINEAR, RR.REPLICATE) for i, f in enumerate(src)])
        assert differ_pairwise(exp)
        np.testing.assert_array_equal(got.cpu().numpy(), exp)
    shared = Maps(lc.decode_map(DECODE_DH), dsize, LINEAR)
    for B, groups in ((6, 3), (7, 4)):
        p = remap_plan(B, 1, lc.DECODE_DW)
        assert p == dict(status=0, frames_per_item=2, groups=groups, total_tiles=groups * lc.DECODE_TILES, covered=1)
        src, _ = decode_batch(B)
        got = W.remap(dev(src), shared.dev, border_mode=RR.CONSTANT, border_value=lc.BORDER[:3])
        exp = np.stack([RR.remap(f, *shared.of(0), LINEAR, RR.CONSTANT, lc.BORDER[:3]) for f in src])
        assert differ_pairwise(exp)
        np.testing.assert_array_equal(got.cpu().numpy(), exp)
    assert_straddle(flat_plan, (3, 4), lc.DECODE_DW)  # the groups are the plan's frames: 3 and 4 of them straddle the bound as well
