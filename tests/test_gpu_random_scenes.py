"""The seeded random scenes of tests/random_scenes.py on the GPU: the lens warp, the map builder and its six samplers, the direct NV12 and
plane entries, warp_stitch and the six remap_stitch* entries (half of them under gains), every byte or element against expected(case) --
uint8 by value, float32 by bits (pixels.same_float), planes by bits (remap_nv12_ref.assert_planes_equal).  Half of the cases run on padded,
offset sources and into guarded destinations whose canaries are checked after the call; a TRANSPARENT destination keeps its canvas.
One test per family and seed; a failure names (family, seed, index) and the whole parameter record, and
`-k "test_<family> and <seed>"` runs exactly that test again.  Run on the GPU box:  python -m pytest tests -m gpu -q"""
import contextlib

import numpy as np
import pytest
import torch

from tests import pixels as PX
from tests import random_scenes as RS
from tests import remap_nv12_ref as RN
from tests import remap_ref as RR

pytestmark = pytest.mark.gpu

INVERSE = 16
TORCH = {"u8": torch.uint8, "f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def W():
    from bev_amd import warp
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return warp


@contextlib.contextmanager
def named(case):
    """Whatever fails inside carries the case: family, seed, index and the whole parameter record."""
    try:
        yield
    except Exception as e:  # noqa: BLE001  (re-raised with the case in front)
        raise AssertionError("%s\n%s: %s" % (case, type(e).__name__, e)) from e


# ---- tensors of a case -------------------------------------------------------------------------------------------------------------------------

def _one(t, case):
    """Batches of one are given as single frames: the entries' other rank."""
    return t[0] if case.p.B == 1 else t


def frames_on_device(case, cam, k):
    """A camera's frames as the entry takes them: compact, or (layout cases) inside padded, offset allocations whose filling is not the border."""
    L = case.p.layout
    if isinstance(cam.frames, tuple):
        y, uv = cam.frames
        if L is None:
            return _one(torch.from_numpy(y).cuda(), case), _one(torch.from_numpy(uv).cuda(), case)
        a, b, c = L.pads
        return _one(PX.strided(y, (a + k, b + 2 * k)), case), _one(PX.strided(uv, (2 * c + 2 * k, 2 * a)), case)  # (uv strides stay even)
    if L is None:
        return _one(torch.from_numpy(cam.frames).cuda(), case)
    fill = PX.U8_FILL if cam.frames.dtype == np.uint8 else float("nan")
    return _one(PX.padded_source(cam.frames, fill, offset=L.offset, pad_rows=L.pad_rows), case)


def map_on_device(W, case, cam):
    """build_warp_map of a camera, into compact planes or (layout cases) into row- and frame-padded ones."""
    p, L = case.p, case.p.layout
    dw, dh = p.dsize
    kw = {}
    if cam.model == "rational":
        kw = dict(K=cam.K, dist_coeff=cam.dist, r2_max=cam.guard)
    elif cam.model == "fisheye":
        kw = dict(K=cam.K, dist_coeff=cam.dist, lens_model="fisheye", theta_max=cam.guard)
    if L is not None:
        a, b, c = L.pads
        xy = PX.strided(np.zeros((cam.n_m, dh, dw, 2), np.int16), (2 * a, 2 * b))
        frac = PX.strided(np.zeros((cam.n_m, dh, dw), np.int16), (c, a)) if p.interp == 1 else None
        kw["out"] = W.WarpMap(xy, frac, p.interp, p.dsize)
    return W.build_warp_map(cam.Minv, p.dsize, flags=p.interp | INVERSE, **kw)


def destination(case, c):
    """(out argument, read): compact cases pass out=None and read what the entry returns; layout cases pass guarded views and read them,
    after their canaries were checked.  read(returned) gives the result in expected()'s form, a list over the batch."""
    p, L = case.p, case.p.layout
    dw, dh = p.dsize
    kind = RS.kind_of_result(case)
    lead = () if p.B == 1 else (p.B,)

    def frames(t):
        return [t] if p.B == 1 else list(t)

    if kind == "pixels":
        if L is None:
            return None, lambda ret: [f.cpu().numpy() for f in frames(ret)]
        view, holder = PX.canaried_out(lead + (dh, dw, c), TORCH[p.dtype], L.pad, canvas=RS.CANVAS, align=L.align)

        def read(ret):
            assert ret is view
            PX.assert_canaries_intact(holder, view)
            return [f.cpu().numpy() for f in frames(view)]
        return view, read
    if kind == "planes":
        if L is None:
            return None, lambda ret: frames(ret)
        view, holder = PX.canaried_out(lead + (c, dh, dw), TORCH[p.plane], L.pad, canvas=RS.CANVAS, align=L.align, planar=True)

        def read(ret):
            assert ret is view
            PX.assert_canaries_intact(holder, view)
            return frames(view)
        return view, read
    if L is None:
        def read(ret):
            assert tuple(ret.shape) == lead + (dh * 3 // 2, dw)
            return [(f[:dh].cpu().numpy(), f[dh:].cpu().numpy().reshape(dh // 2, dw // 2, 2)) for f in frames(ret)]
        return None, read
    y, hy = PX.canaried_out(lead + (dh, dw), torch.uint8, L.pad, canvas=RS.CANVAS, align=L.align, planar=True)
    uv, huv = PX.canaried_out(lead + (dh // 2, dw // 2, 2), torch.uint8, L.pad, canvas=RS.CANVAS, align=max(L.align, 2))

    def read(ret):
        PX.assert_canaries_intact(hy, y, "y")
        PX.assert_canaries_intact(huv, uv, "uv")
        return [(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(frames(y), frames(uv))]
    return (y, uv), read


def compare(case, got, exp):
    """One frame of the batch against the definition, with the family's own comparison."""
    kind = RS.kind_of_result(case)
    if kind == "nv12":
        np.testing.assert_array_equal(got[0], exp[0], err_msg="the Y plane")
        np.testing.assert_array_equal(got[1], exp[1], err_msg="the plane of pairs")
    elif kind == "planes":
        RN.assert_planes_equal(got, exp, TORCH[case.p.plane])
    elif exp.dtype == np.float32:
        PX.same_float(got.reshape(exp.shape), exp)
    else:
        np.testing.assert_array_equal(got.reshape(exp.shape), exp)


def check(case, read, ret):
    torch.cuda.synchronize()
    got, exp = read(ret), RS.expected(case)
    assert len(got) == len(exp) == case.p.B
    for b, (g, e) in enumerate(zip(got, exp)):
        try:
            compare(case, g, e)
        except AssertionError as err:
            raise AssertionError("frame %d of the batch: %s" % (b, err)) from err


def _matrices(M):
    return M[0] if len(M) == 1 else M


def _lens_kw(cam):
    if cam.model == "fisheye":
        return dict(lens_model="fisheye", theta_max=cam.guard)
    return dict(r2_max=cam.guard)


# ---- the families -------------------------------------------------------------------------------------------------------------------------------

def run_lens(W, case):
    p, cam = case.p, RS.inputs(case)[0]
    out, read = destination(case, p.c)
    ret = W.warp_perspective_lens(frames_on_device(case, cam, 0), _matrices(cam.Minv), p.dsize, cam.K, cam.dist, flags=p.interp | INVERSE, border_value=list(p.border), out=out,
                                  border_mode=p.mode, **_lens_kw(cam))
    check(case, read, ret)


def run_map(W, case):
    p, cam = case.p, RS.inputs(case)[0]
    m = map_on_device(W, case, cam)
    torch.cuda.synchronize()
    defs = RS.maps_of(case)[0]
    np.testing.assert_array_equal(m.xy.cpu().numpy(), np.stack([xy for xy, _ in defs]), err_msg="the map's xy plane")
    if p.interp == 1:
        np.testing.assert_array_equal(m.frac.cpu().numpy().view(np.uint16), np.stack([frac for _, frac in defs]), err_msg="the map's frac plane")
    src = frames_on_device(case, cam, 0)
    out, read = destination(case, 3 if p.user != "remap" else p.c)
    bv = list(p.border) if p.mode == RR.CONSTANT else None
    scale, bias = RS.SCALES[p.sb][:3], RS.BIASES[p.sb][:3]
    if p.user == "remap":
        ret = W.remap(src, m, border_mode=p.mode, border_value=bv, out=out)
    elif p.user == "remap_nv12":
        ret = W.remap_nv12(*src, m, border_mode=p.mode, border_value=bv, out=out, rgb=p.rgb)
    elif p.user == "remap_to_nv12":
        ret = W.remap_to_nv12(src, m, border_mode=p.mode, border_value=bv, out=out, rgb=p.rgb)
    elif p.user == "remap_nv12_to_nv12":
        ret = W.remap_nv12_to_nv12(*src, m, border_mode=p.mode, border_value=bv, out=out)
    elif p.user == "remap_to_planar":
        ret = W.remap_to_planar(src, m, scale=scale, bias=bias, border_mode=p.mode, border_value=bv, out=out, out_dtype=TORCH[p.plane])
    else:
        ret = W.remap_nv12_to_planar(*src, m, scale=scale, bias=bias, border_mode=p.mode, border_value=bv, out=out, rgb=p.rgb, out_dtype=TORCH[p.plane])
    check(case, read, ret)


def run_nv12(W, case):
    p, cam = case.p, RS.inputs(case)[0]
    src = frames_on_device(case, cam, 0)
    out, read = destination(case, p.c)
    M, bv = _matrices(cam.M), list(p.border)
    scale, bias = RS.SCALES[p.sb][:p.c], RS.BIASES[p.sb][:p.c]
    if p.entry == "warp_perspective_nv12":
        ret = W.warp_perspective_nv12(*src, M, p.dsize, flags=p.interp, border_value=bv, out=out, rgb=p.rgb)
    elif p.entry == "warp_nv12_to_planar":
        ret = W.warp_nv12_to_planar(*src, M, p.dsize, scale=scale, bias=bias, flags=p.interp, border_value=bv, out=out, rgb=p.rgb, out_dtype=TORCH[p.plane])
    elif p.entry == "warp_perspective_to_nv12":
        ret = W.warp_perspective_to_nv12(src, M, p.dsize, flags=p.interp, border_value=bv, out=out, rgb=p.rgb)
    elif p.entry == "warp_nv12_to_nv12":
        ret = W.warp_nv12_to_nv12(*src, M, p.dsize, flags=p.interp, border_value=bv, out=out)
    else:
        ret = W.warp_to_planar(src, M, p.dsize, scale=scale, bias=bias, flags=p.interp, border_value=bv, out=out, out_dtype=TORCH[p.plane])
    check(case, read, ret)


def run_stitch(W, case):
    p, cams = case.p, RS.inputs(case)
    srcs = [frames_on_device(case, cam, k) for k, cam in enumerate(cams)]
    out, read = destination(case, p.c)
    kw = dict(blend="feather" if p.feather else "over", feather=p.feather or 64, border_value=list(p.border), out=out)
    if p.entry == "warp_stitch":
        ret = W.warp_stitch(srcs, [_matrices(cam.Minv) for cam in cams], p.dsize, flags=p.interp | INVERSE, border_mode=p.mode, **kw)
        return check(case, read, ret)
    maps = [map_on_device(W, case, cam) for cam in cams]
    kw["gains"] = RS.gains_of(case)
    scale, bias = RS.SCALES[p.sb][:3], RS.BIASES[p.sb][:3]
    ys, uvs = ([s[0] for s in srcs], [s[1] for s in srcs]) if p.entry.startswith("nv12") else (None, None)
    if p.entry == "maps":
        ret = W.remap_stitch(srcs, maps, border_mode=p.mode, **kw)
    elif p.entry == "nv12":
        ret = W.remap_stitch_nv12(ys, uvs, maps, border_mode=p.mode, rgb=p.rgb, **kw)
    elif p.entry == "to_nv12":
        ret = W.remap_stitch_to_nv12(srcs, maps, rgb=p.rgb, **kw)
    elif p.entry == "nv12_to_nv12":
        ret = W.remap_stitch_nv12_to_nv12(ys, uvs, maps, **kw)
    elif p.entry == "planes":
        ret = W.remap_stitch_to_planar(srcs, maps, scale=scale, bias=bias, out_dtype=TORCH[p.plane], **kw)
    else:
        ret = W.remap_stitch_nv12_to_planar(ys, uvs, maps, scale=scale, bias=bias, rgb=p.rgb, out_dtype=TORCH[p.plane], **kw)
    check(case, read, ret)


RUN = {"lens": run_lens, "map": run_map, "nv12": run_nv12, "stitch": run_stitch}


def sweep(W, family, seed):
    for case in RS.cases(family, seed):
        with named(case):
            RUN[family](W, case)


@pytest.mark.parametrize("seed", RS.SEEDS)
def test_lens(W, seed):
    """warp_perspective_lens: rational and fisheye lenses (rays beyond theta_max, rays behind the camera), both types, 1..4 channels, both
    interpolations, CONSTANT and TRANSPARENT, one matrix or one per frame."""
    sweep(W, "lens", seed)


@pytest.mark.parametrize("seed", RS.SEEDS)
def test_map(W, seed):
    """build_warp_map (pinhole, rational, fisheye; shared or per frame) against the definition's map, then one of the six samplers through it."""
    sweep(W, "map", seed)


@pytest.mark.parametrize("seed", RS.SEEDS)
def test_nv12(W, seed):
    """The direct entries: warp_perspective_nv12, warp_nv12_to_planar, warp_perspective_to_nv12, warp_nv12_to_nv12, warp_to_planar."""
    sweep(W, "nv12", seed)


@pytest.mark.parametrize("seed", RS.SEEDS)
def test_stitch(W, seed):
    """warp_stitch and the six remap_stitch* entries: 1..8 cameras with sizes and maps of their own (pinhole, rational, fisheye, shared or
    per frame), OVER and FEATHER, both borders, half of the map cases under gains."""
    sweep(W, "stitch", seed)
