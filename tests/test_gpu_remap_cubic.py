"""Bicubic sampling through bilinear warp maps on the GPU (bev_amd.warp.remap(interpolation=INTER_CUBIC) -> bevwarp_remap |
BEVWARP_MAP_BICUBIC; FramePipeline(map_interpolation=INTER_CUBIC)): every pixel against tests/remap_cubic_ref.remap_cubic by bits, and --
pinhole maps -- against warp_perspective(flags=INTER_CUBIC), device against device.  Every comparison is total.
Run on the GPU box:  python -m pytest tests -m gpu -q"""
import functools

import numpy as np
import pytest
import torch

from oracle import warp_numpy as wn
from tests import fisheye_ref as FR
from tests import lens_ref as LR
from tests import pixels as PX
from tests import remap_cubic_ref as RC
from tests import remap_ref as RR
from tests import workloads as wl
from tests.test_gpu_remap import _shifted_map
from tests.test_remap_cubic_cpu import BORDER, DH, DW, KEYSTONE, SH, SW, checkerboard

pytestmark = pytest.mark.gpu

CUBIC, LINEAR, NEAREST, INVERSE = 2, 1, 0, 16
CANARY = 77
TILE_W, TILE_H = 256, 4


@pytest.fixture(scope="module")
def W():
    from bev_amd import warp
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return warp


@functools.lru_cache(maxsize=None)
def _src(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, shape, dtype=np.uint8) if dtype == np.uint8 else (rng.random(shape, dtype=np.float32) * 4 - 2).astype(np.float32)


def _host(m):
    """A WarpMap's planes as the reference takes them: (n, dh, dw, 2) int16 and (n, dh, dw) uint16."""
    torch.cuda.synchronize()
    return m.xy.cpu().numpy(), m.frac.cpu().numpy().view(np.uint16)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, exp, what=""):
    assert got.dtype == exp.dtype and got.shape == exp.shape, (got.dtype, exp.dtype, got.shape, exp.shape)
    np.testing.assert_array_equal(_bits(got), _bits(exp), err_msg=what)


def _canvas(src, dh, dw):
    return np.full((dh, dw) + tuple(src.shape[2:]), CANARY, dtype=src.dtype)


def _out(src, dh, dw, batch=None):
    lead = () if batch is None else (batch,)
    return torch.full(lead + (dh, dw) + tuple(src.shape[-1:] if src.ndim > 2 else ()), CANARY, dtype=torch.from_numpy(src[:1]).dtype, device="cuda")


def _bv(mode, c):
    return BORDER[:c] if mode == RC.CONSTANT else None


def _check(W, src, m, xy, frac, mode, what=""):
    """One call on a canvas of 77s against the reference; returns the device result."""
    c = src.shape[2]
    dh, dw = xy.shape[:2]
    out = _out(src, dh, dw)
    assert W.remap(torch.from_numpy(src).cuda(), m, border_mode=mode, border_value=_bv(mode, c), out=out, interpolation=CUBIC) is out
    torch.cuda.synchronize()
    _same(out.cpu().numpy(), RC.remap_cubic(src, xy, frac, mode, BORDER[:c], _canvas(src, dh, dw)), "%s mode %d %s x %d" % (what, mode, src.dtype, c))
    return out


# ---- 1. pinhole maps: the reference, and the matrix kernel it stands in for ----

@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_pinhole_maps(W, dtype, c):
    m = W.build_warp_map(KEYSTONE, (DW, DH), flags=LINEAR | INVERSE)
    xy, frac = _host(m)
    exy, efrac = RR.build((DW, DH), KEYSTONE, interp=RR.LINEAR)
    np.testing.assert_array_equal(xy[0], exy)
    np.testing.assert_array_equal(frac[0], efrac)
    src = _src((SH, SW, c), dtype, 10 + c)
    t = torch.from_numpy(src).cuda()
    for mode in RC.MODES:
        out = _check(W, src, m, exy, efrac, mode, "pinhole")
        want = _out(src, DH, DW)
        W.warp_perspective(t, KEYSTONE, (DW, DH), flags=CUBIC | INVERSE, border_value=_bv(mode, c), out=want, border_mode=mode)
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.uint8), want.view(torch.uint8)), "warp_perspective(INTER_CUBIC) mode %d" % mode
    # the map's own interpolation, by name and by default, is the bilinear call it always was
    a, b = W.remap(t, m), W.remap(t, m, interpolation=LINEAR)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    _same(a.cpu().numpy(), RR.remap(src, exy, efrac, RR.LINEAR, RR.CONSTANT))


# ---- 2. lens maps: bicubic resampling of a raw distorted frame in one pass ----

@pytest.mark.parametrize("model", ["rational", "fisheye"])
def test_lens_maps(W, model):
    sw, sh = 64, 48
    M = wl.rotated_H(sw, sh, DW, DH, 15.0, zoom=1.6)
    K = LR.camera_K(sw, sh)
    if model == "rational":
        m = W.build_warp_map(M, (DW, DH), K=K, dist_coeff=LR.LENS_A, r2_max=0.35)
        exy, efrac = RR.build((DW, DH), LR.ray_matrix(M, K), LR.lens12(K, LR.LENS_A), 0.35, RR.LINEAR)
    else:
        m = W.build_warp_map(M, (DW, DH), K=K, dist_coeff=FR.K_TEST, lens_model="fisheye", theta_max=0.6)
        exy, efrac = FR.build((DW, DH), FR.ray_matrix(M, K), FR.lens12(K, FR.K_TEST), 0.6)
    xy, frac = _host(m)
    np.testing.assert_array_equal(xy[0], exy)
    np.testing.assert_array_equal(frac[0], efrac)
    sentinel = (exy == RR.SENTINEL).all(axis=-1)
    inl, partial, _, written = RC.classes(exy, sw, sh)
    assert sentinel.any() and not sentinel.all() and inl.any() and partial.any() and not (written & sentinel).any()
    for dtype, c in ((np.uint8, 3), (np.float32, 1)):
        src = _src((sh, sw, c), dtype, 30 + c)
        for mode in RC.MODES:
            out = _check(W, src, m, exy, efrac, mode, model).cpu().numpy()
            if mode == RC.CONSTANT:  # an invalid pixel is the border value itself
                assert (out[sentinel] == np.array(BORDER[:c]).astype(dtype)).all()
            if mode == RC.TRANSPARENT:
                assert (out[sentinel] == CANARY).all()


# ---- 3. hand-made maps: the whole int16 range, every frac word, sources smaller than the window ----

@pytest.mark.parametrize("src_hw", [(1, 1), (1, 5), (5, 1), (3, 7), (4, 4), (5, 4)])
def test_hand_made_maps(W, src_hw):
    """Entries -32768, -32767, -2, -1, 0, 1, n - 4 .. n, 32766, 32767 on both axes, in every combination; all 1024 frac words, plain and with
    bits 10-15 set.  The inlier threshold is max(n - 3, 0): none of the sources below 4 pixels on an axis has an inlier."""
    sh, sw = src_hw
    dh, dw = 9, TILE_W + 5  # (two tile columns)
    axis = lambda n: [-32768, -32767, -2, -1, 0, 1, n - 4, n - 3, n - 2, n - 1, n, 32766, 32767]  # noqa: E731
    combos = np.array([(x, y) for y in axis(sh) for x in axis(sw)], dtype=np.int16)
    n = dh * dw
    assert n >= 2048 and n - dw >= len(combos)
    rng = np.random.default_rng(sh * 10 + sw)
    xy = combos[(np.arange(n) * 7) % len(combos)].reshape(dh, dw, 2).copy()  # (7 and 169 are coprime: every combination, next to other fracs each time)
    xy[dh - 1] = rng.integers(-3, max(sw, sh) + 3, (dw, 2)).astype(np.int16)     # one row around the source
    frac = (np.arange(n) % 1024).astype(np.uint16)
    frac[1024:] |= (rng.integers(1, 64, n - 1024).astype(np.uint16) << 10)          # every word once as it is, once under high bits
    assert len(np.unique(frac[:1024])) == 1024 and len(np.unique(frac[1024:] & 1023)) == 1024 and (frac[1024:] >> 10).min() >= 1
    frac = frac.reshape(dh, dw)
    inl = RC.classes(xy, sw, sh)[0]
    assert inl.any() == (sw > 3 and sh > 3)
    txy = torch.from_numpy(xy).cuda()[None]
    tfrac = torch.from_numpy(frac.view(np.int16)).cuda()[None]
    m = W.WarpMap(txy, tfrac, LINEAR, (dw, dh))
    for dtype, c in ((np.uint8, 3), (np.uint8, 4), (np.float32, 1), (np.float32, 4)):
        src = _src((sh, sw, c), dtype, 600 + c)
        for mode in RC.MODES:
            _check(W, src, m, xy, frac, mode, "hand-made %s" % (src_hw,))


# ---- 4. layouts: rows that end inside a lane and at a tile's edge; both store, both load and both map-load paths ----

@pytest.mark.parametrize("dw", [1, 3, 4, 5, TILE_W - 1, TILE_W, TILE_W + 1])
def test_layouts(W, dw):
    sw, sh = 31, 17
    for dh in (1, TILE_H - 1, TILE_H, TILE_H + 1):
        M = wl.rotated_H(sw, sh, max(dw, 2), max(dh, 2), 12.0, zoom=1.3 * min(sw / max(dw, 2), 4.0))
        m = W.build_warp_map(M, (dw, dh))
        exy, efrac = RR.build((dw, dh), wn.invert3x3(M), interp=RR.LINEAR)
        xy, frac = _host(m)
        np.testing.assert_array_equal(xy[0], exy)
        for dtype, c in ((np.uint8, 4), (np.uint8, 3), (np.uint8, 2), (np.float32, 4), (np.float32, 1)):
            src = _src((sh, sw, c), dtype, 400 + c)
            for aligned in (True, False):
                # aligned: a 16-byte-aligned destination, an aligned source, map planes on 64-byte boundaries with rows of 4 k entries;
                # else: everything one element off, rows of odd lengths
                maps, _keep = _shifted_map(W, m, 0, 0, (-dw) % 4) if aligned else _shifted_map(W, m, 4, 2, 3)
                s = PX.padded_source(src, PX.U8_FILL if dtype == np.uint8 else 3.0, offset=0 if aligned else 1)
                if dtype == np.uint8 and c in (2, 4):  # (the pixels' own alignment decides between one load per tap and a load per byte)
                    assert (s.data_ptr() % c == 0) == aligned and s.stride(0) % c == 0
                for mode in (RC.CONSTANT, RC.WRAP, RC.TRANSPARENT):
                    out, holder = PX.canaried_out((dh, dw, c), dtype, pad=5, align=16 if aligned else 0)
                    W.remap(s, maps, border_mode=mode, border_value=_bv(mode, c), out=out, interpolation=CUBIC)
                    torch.cuda.synchronize()
                    _same(out.cpu().numpy(), RC.remap_cubic(src, exy, efrac, mode, BORDER[:c], _canvas(src, dh, dw)),
                          "%d x %d mode %d aligned %d %s x %d" % (dw, dh, mode, aligned, dtype, c))
                    PX.assert_canaries_intact(holder, out)


# ---- 5. frames: shared and per-frame maps, every frame different, the short last group of two-frame items ----

def _frames(n, sh, sw, c, dtype, seed):
    return np.stack([_src((sh, sw, c), dtype, seed + i) for i in range(n)])


@pytest.mark.parametrize("batch", [1, 2, 3, 7])
def test_frame_loop_small(W, batch):
    sw, sh, dw, dh = 40, 24, 36, 20
    H = wl.rotated_H(sw, sh, dw, dh, 15.0, zoom=1.4)
    shared = W.build_warp_map(H, (dw, dh))
    per_frame = W.build_warp_map(np.stack([wl.jitter_H(H, i + 1) for i in range(batch)]), (dw, dh))
    sxy, sfrac = _host(shared)
    pxy, pfrac = _host(per_frame)
    for dtype, c in ((np.uint8, 3), (np.float32, 4)):
        host = _frames(2 * batch, sh, sw, c, dtype, 100)
        dev = torch.from_numpy(host).cuda()
        for mode in (RC.CONSTANT, RC.REFLECT_101, RC.TRANSPARENT):
            for m, xy, frac in ((shared, sxy, sfrac), (per_frame, pxy, pfrac)):
                holder = torch.full((batch, dh + 3, dw + 2, c), CANARY, dtype=dev.dtype, device="cuda")
                out = holder[:, :dh, :dw]  # padded rows and frames
                W.remap(dev[::2], m, border_mode=mode, border_value=_bv(mode, c), out=out, interpolation=CUBIC)  # (a strided batch)
                torch.cuda.synchronize()
                got = holder.cpu().numpy()
                for b in range(batch):
                    k = b if m.n > 1 else 0
                    _same(got[b, :dh, :dw], RC.remap_cubic(host[2 * b], xy[k], frac[k], mode, BORDER[:c], _canvas(host[0], dh, dw)),
                          "frame %d of %d, mode %d, %d maps" % (b, batch, mode, m.n))
                assert (got[:, dh:] == CANARY).all() and (got[:, :, dw:] == CANARY).all()


@pytest.mark.parametrize("batch", [2, 3, 7])
def test_frame_loop_two_frames_per_item(W, batch):
    """A destination of 5 x 16384 pixels is 4096 tiles: a shared map then walks two frames per item from 2 frames on (plan_remap fills 4096
    items first; tests/test_remap_cpu.py pins the rule), and 3 and 7 frames end in a group of one."""
    sw, sh, dw, dh = 40, 24, 5, 16384
    Minv = np.array([[6.0, 0.002, -3.0], [0.5, 0.0016, -2.0], [0.0, 0.0, 1.0]])
    m = W.build_warp_map(Minv, (dw, dh), flags=LINEAR | INVERSE)
    xy, frac = _host(m)
    inl, partial, all_out, _ = RC.classes(xy[0], sw, sh)
    assert inl.any() and partial.any() and all_out.any()
    for dtype, c, modes in ((np.uint8, 3, (RC.CONSTANT, RC.TRANSPARENT)), (np.float32, 4, (RC.REPLICATE,))):
        host = _frames(batch, sh, sw, c, dtype, 300)
        dev = torch.from_numpy(host).cuda()
        for mode in modes:
            out = _out(host[0], dh, dw, batch)
            W.remap(dev, m, border_mode=mode, border_value=_bv(mode, c), out=out, interpolation=CUBIC)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            for b in range(batch):
                _same(got[b], RC.remap_cubic(host[b], xy[0], frac[0], mode, BORDER[:c], _canvas(host[0], dh, dw)), "frame %d of %d, mode %d" % (b, batch, mode))


# ---- 6. float32 specials ----

def _canon(a):
    """The 32 bits of every pixel, every NaN as one pattern: the definition leaves a NaN's sign and payload open ("some NaN"), and the
    reference's are numpy's on the host.  Nothing else is folded: -0.0 is not +0.0, a subnormal is not 0."""
    b = _bits(a).copy()
    b[np.isnan(a)] = 0x7fc00000
    return b


@pytest.mark.parametrize("kind,c", [("mixed", 1), ("mixed", 3), ("tiny", 4), ("huge", 2)])
def test_float32_specials(W, kind, c):
    """NaN, +-inf, -0.0, subnormals and values next to FLT_MAX in the source; -0.0, a subnormal and FLT_MAX as border values (a border value
    that is NaN or +-inf is BEVWARP_ERR_NOT_FINITE).  Compared as uint32, NaNs included: a NaN pixel must be a NaN pixel."""
    m = W.build_warp_map(KEYSTONE, (DW, DH), flags=LINEAR | INVERSE)
    xy, frac = _host(m)
    src = PX.float_frame(kind, 50 + c, SH, SW, c)
    t = torch.from_numpy(src).cuda()
    borders = ((-0.0, 1e-45, float(PX.FLT_MAX), -1e-40)[:c], (-0.0,) * c)
    nans = 0
    with np.errstate(all="ignore"):
        for mode in RC.MODES:
            for bv in borders if mode == RC.CONSTANT else (None,):
                out = torch.full((DH, DW, c), float(CANARY), dtype=torch.float32, device="cuda")
                W.remap(t, m, border_mode=mode, border_value=bv, out=out, interpolation=CUBIC)
                torch.cuda.synchronize()
                got = out.cpu().numpy()
                exp = RC.remap_cubic(src, xy[0], frac[0], mode, 0.0 if bv is None else bv, np.full((DH, DW, c), CANARY, np.float32))
                np.testing.assert_array_equal(_canon(got), _canon(exp), err_msg="%s x %d mode %d border %s" % (kind, c, mode, bv))
                nans += int(np.isnan(exp).sum())
    assert kind != "mixed" or nans > 0


# ---- 7. both 8-bit clamps ----

def test_checkerboard_clamps(W):
    src, xy, frac = checkerboard()
    dh, dw = xy.shape[:2]
    pre = RC.presums(src, xy, frac, RC.REPLICATE)
    assert ((pre + 16384) >> 15 < 0).any() and ((pre + 16384) >> 15 > 255).any()
    m = W.WarpMap(torch.from_numpy(xy).cuda()[None], torch.from_numpy(frac.view(np.int16)).cuda()[None], LINEAR, (dw, dh))
    for c in (1, 2, 3, 4):
        s = np.ascontiguousarray(np.repeat(src, c, axis=2))
        for mode in (RC.REPLICATE, RC.CONSTANT):
            out = _check(W, s, m, xy, frac, mode, "checkerboard").cpu().numpy()
            assert out.min() == 0 and out.max() == 255


# ---- 8. TRANSPARENT: what is not written is not touched ----

@pytest.mark.parametrize("dtype,c", [(np.uint8, 3), (np.uint8, 1), (np.float32, 4), (np.float32, 2)])
def test_transparent_canary(W, dtype, c):
    m = W.build_warp_map(KEYSTONE, (DW, DH), flags=LINEAR | INVERSE)
    xy, frac = _host(m)
    written = RC.classes(xy[0], SW, SH)[3]
    assert written.any() and (~written).any()
    src = _src((SH, SW, c), dtype, 800 + c)
    t = torch.from_numpy(src).cuda()
    for align in (16, 0):
        out, holder = PX.canaried_out((DH, DW, c), dtype, pad=5, align=align)
        W.remap(t, m, border_mode=RC.TRANSPARENT, out=out, interpolation=CUBIC)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        _same(got, RC.remap_cubic(src, xy[0], frac[0], RC.TRANSPARENT, canvas=_canvas(src, DH, DW)))
        assert (got[~written] == CANARY).all()
        PX.assert_canaries_intact(holder, out)
    got = W.remap(t, m, border_mode=RC.TRANSPARENT, interpolation=CUBIC)  # without `out`: from zeros
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    _same(got, RC.remap_cubic(src, xy[0], frac[0], RC.TRANSPARENT))
    assert (_bits(got)[~written] == 0).all()


# ---- 9. a side stream, and a captured graph ----

def test_side_stream_behind_input_writes(W):
    m = W.build_warp_map(KEYSTONE, (DW, DH), flags=LINEAR | INVERSE)
    xy, frac = _host(m)
    src = _src((SH, SW, 3), np.uint8, 900)
    staged = torch.from_numpy(np.array(src)).pin_memory()
    t = torch.zeros((SH, SW, 3), dtype=torch.uint8, device="cuda")
    out = _out(src, DH, DW)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t.fill_(255)
        t.copy_(staged, non_blocking=True)
        W.remap(t, m, border_mode=RC.REFLECT, out=out, interpolation=CUBIC)
    s.synchronize()
    _same(out.cpu().numpy(), RC.remap_cubic(src, xy[0], frac[0], RC.REFLECT))


def test_graph_replay(W):
    """One call captured (a single chain of nodes), replayed on two sets of frames written to the same addresses."""
    m = W.build_warp_map(KEYSTONE, (DW, DH), flags=LINEAR | INVERSE)
    xy, frac = _host(m)
    sets = [_frames(2, SH, SW, 3, np.uint8, 910 + 10 * k) for k in range(2)]
    t = torch.zeros((2, SH, SW, 3), dtype=torch.uint8, device="cuda")
    out = torch.full((2, DH, DW, 3), CANARY, dtype=torch.uint8, device="cuda")
    W.remap(t, m, border_mode=RC.CONSTANT, border_value=BORDER[:3], out=out, interpolation=CUBIC)  # (the library is loaded before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        W.remap(t, m, border_mode=RC.CONSTANT, border_value=BORDER[:3], out=out, interpolation=CUBIC)
    for frames in sets:
        t.copy_(torch.from_numpy(frames))
        out.fill_(CANARY)
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for b in range(2):
            _same(got[b], RC.remap_cubic(frames[b], xy[0], frac[0], RC.CONSTANT, BORDER[:3]), "frame %d" % b)


# ---- 10. FramePipeline ----

@pytest.mark.parametrize("download", [True, False])
def test_frame_pipeline(W, download):
    from bev_amd.pipeline import FramePipeline
    sw, sh, dw, dh = 40, 24, 36, 20
    M = wl.rotated_H(sw, sh, dw, dh, 15.0, zoom=1.4)
    K = LR.camera_K(sw, sh)
    m = W.build_warp_map(M, (dw, dh), K=K, dist_coeff=LR.LENS_A, r2_max=0.12)
    xy, frac = _host(m)
    assert (xy[0] == RR.SENTINEL).all(axis=-1).any()
    frames = _frames(3, sh, sw, 3, np.uint8, 700)
    with FramePipeline((sh, sw), 3, None, (dw, dh), warp_map=m, download=download, map_interpolation=CUBIC) as pipe:
        got = [np.array(r.cpu().numpy() if isinstance(r, torch.Tensor) else r) for r in pipe.run(list(frames))]
    assert len(got) == 3
    for b in range(3):
        _same(got[b], RC.remap_cubic(frames[b], xy[0], frac[0], RC.CONSTANT), "frame %d" % b)
    with FramePipeline((sh, sw), 3, None, (dw, dh), warp_map=m, download=download) as pipe:  # None: the bilinear pipeline, as it was
        bil = [np.array(r.cpu().numpy() if isinstance(r, torch.Tensor) else r) for r in pipe.run(list(frames))]
    _same(bil[1], RR.remap(frames[1], xy[0], frac[0], RR.LINEAR, RR.CONSTANT))
