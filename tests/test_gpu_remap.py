"""The fixed-camera warp maps on the GPU (bev_amd.warp.build_warp_map -> bevwarp_build_map, remap -> bevwarp_remap, cv2_compat.remap,
FramePipeline(warp_map=...)): the maps against tests/remap_ref.build and the pixels against tests/remap_ref.remap bit for bit, and
against the entries they stand in for -- warp_perspective(border_mode=...) and warp_perspective_lens -- device against device.
Run on the GPU box:  python -m pytest tests -m gpu -q"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from bev_amd import _lib
from oracle import warp_numpy as wn
from tests import lens_ref as LR
from tests import pixels as PX
from tests import remap_ref as RR
from tests import workloads as wl
from tests.test_lens_cpu import GEOMS

pytestmark = pytest.mark.gpu

LINEAR, NEAREST, INVERSE = 1, 0, 16
INF = float("inf")
LENSES = {"A": LR.LENS_A, "B": LR.LENS_B}
KINDS = ("pinhole", "A", "B")
BORDER = (7.0, 200.0, 31.0, 99.0)  # a non-zero border value per channel
CANARY = 77


@pytest.fixture(scope="module")
def W():
    from bev_amd import warp
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return warp


@functools.lru_cache(maxsize=None)
def _src(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, shape, dtype=np.uint8) if dtype == np.uint8 else rng.random(shape, dtype=np.float32)


def _chain(geom, kind):
    """(matrix for remap_ref.build, lens or None, default r2_max, K, dist) of a geometry under a lens kind."""
    sw, sh, dw, dh, M = GEOMS[geom]
    if kind == "pinhole":
        return wn.invert3x3(M), None, INF, None, None
    K = LR.camera_K(sw, sh)
    return LR.ray_matrix(M, K), LR.lens12(K, LENSES[kind]), LR.lens_valid_r2(LENSES[kind]), K, LENSES[kind]


@functools.lru_cache(maxsize=None)
def _ref_map(geom, kind, interp):
    sw, sh, dw, dh, M = GEOMS[geom]
    R, lens, r2, _, _ = _chain(geom, kind)
    return RR.build((dw, dh), R, lens, r2, interp)


def _host(m):
    """A WarpMap's planes as remap_ref has them: (n, dh, dw, 2) int16 and (n, dh, dw) uint16 (or None)."""
    torch.cuda.synchronize()
    return m.xy.cpu().numpy(), (None if m.frac is None else m.frac.cpu().numpy().view(np.uint16))


def _gpu_map(W, geom, kind, interp):
    sw, sh, dw, dh, M = GEOMS[geom]
    _, _, _, K, dist = _chain(geom, kind)
    return W.build_warp_map(M, (dw, dh), flags=interp, K=K, dist_coeff=dist)


def _out(src, dh, dw):
    return torch.full((dh, dw) + tuple(src.shape[2:]), CANARY, dtype=torch.from_numpy(src[:1]).dtype, device="cuda")


def _canvas(src, dh, dw):
    return np.full((dh, dw) + tuple(src.shape[2:]), CANARY, dtype=src.dtype)


# ---- 1. the maps ----

@pytest.mark.parametrize("geom", sorted(GEOMS))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_map_contents(W, geom, kind, interp):
    sw, sh, dw, dh, M = GEOMS[geom]
    m = _gpu_map(W, geom, kind, interp)
    assert m.n == 1 and m.dsize == (dw, dh) and m.interp == interp and m.xy.dtype == torch.int16 and (m.frac is None) == (interp == NEAREST)
    xy, frac = _host(m)
    exy, efrac = _ref_map(geom, kind, interp)
    np.testing.assert_array_equal(xy[0], exy)
    if interp == LINEAR:
        assert m.frac.dtype == torch.int16
        np.testing.assert_array_equal(frac[0], efrac)


@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_map_contents_matrices_flags_and_r2_max(W, interp):
    """(2, 3, 3) matrices, WARP_INVERSE_MAP, r2_max None / a number / inf, and `out`."""
    sw, sh, dw, dh, M = GEOMS["brno"]
    K = LR.camera_K(sw, sh)
    Ms = np.stack([M, wl.jitter_H(M, 3)])
    for dist in (None, LR.LENS_A):
        lens = None if dist is None else LR.lens12(K, dist)
        m = W.build_warp_map(Ms, (dw, dh), flags=interp, K=K, dist_coeff=dist)
        assert m.n == 2
        xy, frac = _host(m)
        for i in range(2):
            R = wn.invert3x3(Ms[i]) if dist is None else LR.ray_matrix(Ms[i], K)
            exy, efrac = RR.build((dw, dh), R, lens, INF if dist is None else LR.lens_valid_r2(dist), interp)
            np.testing.assert_array_equal(xy[i], exy)
            if interp == LINEAR:
                np.testing.assert_array_equal(frac[i], efrac)
        assert not np.array_equal(xy[0], xy[1])
        # the inverse given: the same entries
        mi = W.build_warp_map(wn.invert3x3(M), (dw, dh), flags=interp | INVERSE, K=K, dist_coeff=dist)
        R = wn.invert3x3(M) if dist is None else LR.ray_matrix(wn.invert3x3(M), K, inverse_given=True)
        np.testing.assert_array_equal(_host(mi)[0][0], RR.build((dw, dh), R, lens, INF if dist is None else LR.lens_valid_r2(dist), interp)[0])
    sentinels = {}
    for r2 in (0.05, INF):
        m = W.build_warp_map(M, (dw, dh), flags=interp, K=K, dist_coeff=LR.LENS_A, r2_max=r2)
        xy, frac = _host(m)
        exy, efrac = RR.build((dw, dh), LR.ray_matrix(M, K), LR.lens12(K, LR.LENS_A), r2, interp)
        np.testing.assert_array_equal(xy[0], exy)
        if interp == LINEAR:
            np.testing.assert_array_equal(frac[0], efrac)
        sentinels[r2] = int((xy[0] == -32768).all(axis=-1).sum())
    assert sentinels[0.05] > sentinels[INF]  # (without a limit only coordinates that saturate give that entry)
    # out=: written in place, zero distortion is the pinhole chain
    m = _gpu_map(W, "brno", "pinhole", interp)
    m2 = W.WarpMap(torch.zeros_like(m.xy), None if m.frac is None else torch.zeros_like(m.frac), interp, (dw, dh))
    assert W.build_warp_map(M, (dw, dh), flags=interp, K=K, dist_coeff=np.zeros(5), out=m2) is m2
    torch.cuda.synchronize()
    assert torch.equal(m2.xy, m.xy) and (m.frac is None or torch.equal(m2.frac, m.frac))


def _abi_build(R, lens, r2_max, dsize, interp):
    """bevwarp_build_map itself, tight planes."""
    lib = _lib.load()
    dw, dh = dsize
    Rd = torch.from_numpy(np.ascontiguousarray(np.asarray(R, np.float64).reshape(-1, 3, 3))).cuda()
    n = Rd.shape[0]
    xy = torch.full((n, dh, dw, 2), 1234, dtype=torch.int16, device="cuda")
    frac = torch.full((n, dh, dw), 1234, dtype=torch.int16, device="cuda")
    lens = None if lens is None else np.ascontiguousarray(lens, np.float64)
    st = lib.bevwarp_build_map(Rd.data_ptr(), n, None if lens is None else lens.ctypes.data_as(ctypes.c_void_p), r2_max, interp, xy.data_ptr(),
                               frac.data_ptr() if interp == LINEAR else None, dh, dw, dh * dw * 4, dw * 4, dh * dw * 2, dw * 2,
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == 0, st
    if interp == NEAREST:
        assert (frac == 1234).all()  # not written
    return xy.cpu().numpy(), frac.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_map_contents_pole_zero_w_and_horizon(W, interp):
    """tests/test_gpu_lens.py's matrices: the rational model's pole (+-inf, 0 / 0), W == 0 inside the destination, and a horizon; with a
    lens and as pinhole matrices.  None needs a special case: +-inf and NaN round to INT_MAX / INT_MIN and saturate."""
    lens = lambda k1, k4: np.array([9.0, 7.0, 11.0, 8.0, k1, 0, 0, 0, 0, k4, 0, 0])  # noqa: E731
    Rs = (np.array([[0.125, 0, 0], [0, 0.125, 0], [0, 0, 1.0]]), np.array([[1.0, 0, 0], [0, 1.0, 0], [1.0, 0, -5.0]]),
          np.array([[1.3, 0.2, -30.0], [0.1, 1.1, -20.0], [0.0, 0.02, -0.5]]))
    for R in Rs:
        for ln, r2 in ((lens(0.0, -1.0), INF), (lens(-1.0, -1.0), INF), (lens(-1.0, -1.0), 0.5), (None, INF)):
            xy, frac = _abi_build(R, ln, r2, (29, 21), interp)
            exy, efrac = RR.build((29, 21), R, ln, r2, interp)
            np.testing.assert_array_equal(xy[0], exy)
            if interp == LINEAR:
                np.testing.assert_array_equal(frac[0], efrac)


# ---- 2. and 3. the parity matrix, against the numpy definition and against the entries the route replaces ----

@pytest.mark.parametrize("geom", sorted(GEOMS))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_parity_matrix(W, geom, kind, dtype, interp):
    sw, sh, dw, dh, M = GEOMS[geom]
    _, _, _, K, dist = _chain(geom, kind)
    m = _gpu_map(W, geom, kind, interp)
    exy, efrac = _ref_map(geom, kind, interp)
    keep = ~RR.written(exy, sw, sh, interp)
    modes = RR.MODES if kind == "pinhole" else (RR.CONSTANT, RR.TRANSPARENT)
    for shape in [(sh, sw, c) for c in (1, 2, 3, 4)] + [(sh, sw)]:
        src = _src(shape, dtype, len(shape) * 10 + shape[-1])
        c = 1 if len(shape) == 2 else shape[2]
        t = torch.from_numpy(src).cuda()
        for mode in modes:
            bv = BORDER[:c] if mode == RR.CONSTANT else None
            out = _out(src, dh, dw)
            assert W.remap(t, m, border_mode=mode, border_value=bv, out=out) is out
            dev = _out(src, dh, dw)
            if kind == "pinhole":
                W.warp_perspective(t, M, (dw, dh), flags=interp, border_value=bv, out=dev, border_mode=mode)
            else:
                W.warp_perspective_lens(t, M, (dw, dh), K, dist, flags=interp, border_value=bv, out=dev, border_mode=mode)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            exp = RR.remap(src, exy, efrac, interp, mode, border_value=0.0 if bv is None else bv, canvas=_canvas(src, dh, dw))
            what = "%s %s mode %d interp %d %s %s" % (geom, kind, mode, interp, src.dtype, shape)
            np.testing.assert_array_equal(got, exp, err_msg=what)
            assert torch.equal(out, dev), what  # device against device, by bits
            if mode == RR.TRANSPARENT:  # the canary survives exactly off the written mask
                assert (got[keep] == CANARY).all() and keep.any() and not keep.all()
    # without `out`: a new tensor; TRANSPARENT starts from zeros
    src = _src((sh, sw, 3), dtype, 33)
    got = W.remap(torch.from_numpy(src).cuda(), m, border_mode=RR.TRANSPARENT)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), RR.remap(src, exy, efrac, interp, RR.TRANSPARENT))


# ---- 4. the frame loop ----

def _frames(n, sh, sw, c, dtype, seed):
    return np.stack([_src((sh, sw, c), dtype, seed + i) for i in range(n)])


@pytest.mark.parametrize("batch", [1, 2, 3, 7, 33])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_frame_loop_small(W, batch, interp):
    """40 x 24 -> 36 x 20, every frame different: a shared map and per-frame maps (a matrix per frame), a strided batch (src[::2]) and an
    `out` with padded frames."""
    sw, sh, dw, dh = 40, 24, 36, 20
    H = wl.rotated_H(sw, sh, dw, dh, 15.0, zoom=1.4)
    host = _frames(2 * batch, sh, sw, 3, np.uint8, 100)
    dev = torch.from_numpy(host).cuda()
    shared = W.build_warp_map(H, (dw, dh), flags=interp)
    Ms = np.stack([wl.jitter_H(H, i + 1) for i in range(batch)])
    per_frame = W.build_warp_map(Ms, (dw, dh), flags=interp)
    sxy, sfrac = _host(shared)
    pxy, pfrac = _host(per_frame)
    assert batch == 1 or not np.array_equal(pxy[0], pxy[1])
    for mode in (RR.CONSTANT, RR.REFLECT_101, RR.TRANSPARENT):
        bv = BORDER[:3] if mode == RR.CONSTANT else None
        for m, xy, frac in ((shared, sxy, sfrac), (per_frame, pxy, pfrac)):
            holder = torch.full((batch, dh + 3, dw + 2, 3), CANARY, dtype=torch.uint8, device="cuda")
            out = holder[:, :dh, :dw]  # padded rows and frames
            src = dev[::2]             # a strided batch
            W.remap(src, m, border_mode=mode, border_value=bv, out=out)
            torch.cuda.synchronize()
            got = holder.cpu().numpy()
            for b in range(batch):
                k = b if m.n > 1 else 0
                exp = RR.remap(host[2 * b], xy[k], None if frac is None else frac[k], interp, mode, border_value=0.0 if bv is None else bv, canvas=_canvas(host[0], dh, dw))
                np.testing.assert_array_equal(got[b, :dh, :dw], exp, err_msg="frame %d of %d, mode %d, %d maps" % (b, batch, mode, m.n))
            assert (got[:, dh:] == CANARY).all() and (got[:, :, dw:] == CANARY).all()


@pytest.mark.parametrize("dsize,batch", [((1024, 256), 33), ((1024, 1024), 33), ((1024, 1024), 7)])
def test_frame_loop_groups_of_frames(W, dsize, batch):
    """Launches large enough for the plan to walk several frames per item (tests/test_remap_cpu.py pins the plans of these shapes for
    up to 8 frames; the library asks for up to 2), with a short last group -- 33 and 7 frames: every frame equals warp_perspective's with the same border, device against device; three frames against the numpy definition."""
    sw, sh = 40, 24
    dw, dh = dsize
    H = wl.rotated_H(sw, sh, dw, dh, 10.0, zoom=1.2)
    host = _frames(batch, sh, sw, 1, np.uint8, 300)
    dev = torch.from_numpy(host).cuda()
    m = W.build_warp_map(H, dsize)
    xy, frac = _host(m)
    for mode in (RR.CONSTANT, RR.WRAP, RR.TRANSPARENT):
        out = torch.full((batch, dh, dw, 1), CANARY, dtype=torch.uint8, device="cuda")
        want = torch.full((batch, dh, dw, 1), CANARY, dtype=torch.uint8, device="cuda")
        W.remap(dev, m, border_mode=mode, border_value=9 if mode == RR.CONSTANT else None, out=out)
        W.warp_perspective(dev, H, dsize, border_value=9 if mode == RR.CONSTANT else None, out=want, border_mode=mode)
        torch.cuda.synchronize()
        assert torch.equal(out, want), mode
        for b in (0, batch - 2, batch - 1):
            exp = RR.remap(host[b], xy[0], frac[0], LINEAR, mode, border_value=9.0, canvas=np.full((dh, dw, 1), CANARY, np.uint8))
            np.testing.assert_array_equal(out[b].cpu().numpy(), exp)


# ---- 5. widths and tiles ----

@pytest.mark.parametrize("dw", [1, 3, 4, 5, 255, 256, 257, 259, 515])
@pytest.mark.parametrize("dh", [1, 5])
def test_widths_and_tiles(W, dw, dh):
    """Rows that end inside a lane's 4 pixels, at a tile's edge and one past it; the destination's row padding holds canaries."""
    sw, sh = 31, 17
    M = wl.rotated_H(sw, sh, dw, max(dh, 2), 12.0, zoom=1.3)
    for dtype in (np.uint8, np.float32):
        src = _src((sh, sw, 3), dtype, 400)
        t = torch.from_numpy(src).cuda()
        for interp in (NEAREST, LINEAR):
            m = W.build_warp_map(M, (dw, dh), flags=interp)
            exy, efrac = RR.build((dw, dh), wn.invert3x3(M), None, INF, interp)
            xy, frac = _host(m)
            np.testing.assert_array_equal(xy[0], exy)
            for mode in (RR.CONSTANT, RR.REPLICATE, RR.TRANSPARENT):
                for align in (16, 0):
                    out, holder = PX.canaried_out((dh, dw, 3), dtype, pad=5, align=align)
                    W.remap(t, m, border_mode=mode, border_value=BORDER[:3] if mode == RR.CONSTANT else None, out=out)
                    torch.cuda.synchronize()
                    exp = RR.remap(src, exy, efrac, interp, mode, border_value=BORDER[:3], canvas=_canvas(src, dh, dw))
                    np.testing.assert_array_equal(out.cpu().numpy(), exp, err_msg="%d x %d mode %d interp %d align %d %s" % (dw, dh, mode, interp, align, dtype))
                    PX.assert_canaries_intact(holder, out)


# ---- 6. layouts ----

def _shifted_map(W, m, xy_off_bytes, frac_off_bytes, row_pad):
    """The same entries in planes that are views: a base `*_off_bytes` off a 64-byte boundary and rows `row_pad` entries longer than dw."""
    n, dh, dw, _ = m.xy.shape
    hx = torch.full((64 + n * dh * (dw + row_pad) * 2 + 64,), 0x7abc, dtype=torch.int16, device="cuda")
    hf = torch.full((64 + n * dh * (dw + row_pad) + 64,), 0x7abc, dtype=torch.int16, device="cuda")
    ox = ((-hx.data_ptr()) % 64 + xy_off_bytes) // 2
    of = ((-hf.data_ptr()) % 64 + frac_off_bytes) // 2
    xy = torch.as_strided(hx, (n, dh, dw, 2), (dh * (dw + row_pad) * 2, (dw + row_pad) * 2, 2, 1), ox)
    frac = torch.as_strided(hf, (n, dh, dw), (dh * (dw + row_pad), dw + row_pad, 1), of)
    assert xy.data_ptr() % 64 == xy_off_bytes and frac.data_ptr() % 64 == frac_off_bytes
    xy.copy_(m.xy)
    if m.frac is not None:
        frac.copy_(m.frac)
    return W.WarpMap(xy, frac if m.frac is not None else None, m.interp, m.dsize), (hx, hf)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_layouts(W, dtype, interp):
    """Map planes as views (xy 4 bytes off a 16-byte boundary, frac 2 bytes off an 8-byte boundary, padded rows), a map BUILT into such
    views, an unaligned destination and a row-padded, channel-sliced source: all equal the aligned call."""
    sw, sh, dw, dh, M = GEOMS["rotated_zoom_out"]
    m = _gpu_map(W, "rotated_zoom_out", "pinhole", interp)
    src = _src((sh, sw, 3), dtype, 500)
    t = torch.from_numpy(src).cuda()
    big = torch.full((sh, sw + 7, 4), 3, dtype=t.dtype, device="cuda")
    big[:, 2:2 + sw, :3] = t
    padded = big[:, 2:2 + sw, :3]  # (copied by the entry: its pixels are not contiguous)
    rows = torch.full((sh, sw + 7, 3), 3, dtype=t.dtype, device="cuda")
    rows[:, 2:2 + sw] = t
    for mode in (RR.CONSTANT, RR.REFLECT, RR.TRANSPARENT):
        bv = BORDER[:3] if mode == RR.CONSTANT else None
        want = _out(src, dh, dw)
        W.remap(t, m, border_mode=mode, border_value=bv, out=want)
        for xo, fo, pad in ((4, 2, 3), (0, 0, 4), (16, 8, 0), (12, 6, 1)):
            shifted, _holders = _shifted_map(W, m, xo, fo, pad)
            for s in (t, padded, rows[:, 2:2 + sw]):
                out, holder = PX.canaried_out((dh, dw, 3), dtype, pad=5, align=0)
                W.remap(s, shifted, border_mode=mode, border_value=bv, out=out)
                torch.cuda.synchronize()
                assert torch.equal(out, want), (mode, xo, fo, pad)
                PX.assert_canaries_intact(holder, out)
    # build_warp_map into views: the same entries, and nothing beside them is written
    shifted, (hx, hf) = _shifted_map(W, m, 4, 2, 3)
    shifted.xy.fill_(0)
    W.build_warp_map(M, (dw, dh), flags=interp, out=shifted)
    torch.cuda.synchronize()
    assert torch.equal(shifted.xy, m.xy) and (m.frac is None or torch.equal(shifted.frac, m.frac))
    inside = torch.zeros_like(hx, dtype=torch.bool)
    torch.as_strided(inside, shifted.xy.shape, shifted.xy.stride(), shifted.xy.storage_offset()).fill_(True)
    assert (hx[~inside] == 0x7abc).all()
    if m.frac is not None:
        inside = torch.zeros_like(hf, dtype=torch.bool)
        torch.as_strided(inside, shifted.frac.shape, shifted.frac.stride(), shifted.frac.storage_offset()).fill_(True)
        assert (hf[~inside] == 0x7abc).all()


# ---- 7. hand-made maps ----

@pytest.mark.parametrize("src_hw", [(1, 1), (1, 2), (2, 1), (5, 3)])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_hand_made_maps(W, src_hw, dtype):
    """Seeded random int16 entries over the full range, -32768 and 32767 included, and around the source; frac with bits above 9 set; all
    six borders (REFLECT_101 of a 1-pixel axis maps every index to 0)."""
    sh, sw = src_hw
    dh, dw = 3, 261  # (two tile columns; few entries: the reference's index remap is a Python loop over the distinct indices)
    rng = np.random.default_rng(sh * 10 + sw)
    xy = rng.integers(-32768, 32768, (dh, dw, 2)).astype(np.int16)
    near = rng.integers(-3 * max(sw, sh) - 2, 3 * max(sw, sh) + 3, (dh, dw, 2)).astype(np.int16)
    xy[:, ::2] = near[:, ::2]
    xy[0, :8] = [[-32768, -32768], [32767, 32767], [-32768, 0], [0, -32768], [32767, 0], [0, 32767], [-1, -1], [0, 0]]
    frac = rng.integers(0, 65536, (dh, dw)).astype(np.uint16)
    frac[1, :4] = [0, 1023, 0xfc00, 0xffff]
    src = _src((sh, sw, 3), dtype, 600)
    t = torch.from_numpy(src).cuda()
    txy = torch.from_numpy(xy).cuda()[None]
    tfrac = torch.from_numpy(frac.view(np.int16)).cuda()[None]
    for interp in (NEAREST, LINEAR):
        m = W.WarpMap(txy, tfrac if interp == LINEAR else None, interp, (dw, dh))
        for mode in RR.MODES:
            out = _out(src, dh, dw)
            W.remap(t, m, border_mode=mode, border_value=BORDER[:3] if mode == RR.CONSTANT else None, out=out)
            torch.cuda.synchronize()
            exp = RR.remap(src, xy, frac, interp, mode, border_value=BORDER[:3], canvas=_canvas(src, dh, dw))
            np.testing.assert_array_equal(out.cpu().numpy(), exp, err_msg="%s mode %d interp %d" % (src_hw, mode, interp))


# ---- 8. FramePipeline ----

@pytest.mark.parametrize("download", [True, False])
def test_frame_pipeline_with_a_map(W, download):
    from bev_amd.pipeline import FramePipeline
    sw, sh, dw, dh, M = GEOMS["brno"]
    K = LR.camera_K(sw, sh)
    m = W.build_warp_map(M, (dw, dh), K=K, dist_coeff=LR.LENS_A)
    frames = _frames(5, sh, sw, 3, np.uint8, 700)
    want = W.remap(torch.from_numpy(frames).cuda(), m)
    torch.cuda.synchronize()
    with FramePipeline((sh, sw), 3, None, (dw, dh), warp_map=m, download=download) as pipe:
        got = [np.array(r.cpu().numpy() if isinstance(r, torch.Tensor) else r) for r in pipe.run(list(frames))]
    assert len(got) == 5
    np.testing.assert_array_equal(np.stack(got), want.cpu().numpy())
    exy, efrac = _ref_map("brno", "A", LINEAR)
    np.testing.assert_array_equal(got[3], RR.remap(frames[3], exy, efrac, LINEAR, RR.CONSTANT))


# ---- 9. cv2_compat.remap ----

@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_cv2_compat_remap(W, interp):
    from bev_amd import cv2_compat as cv2
    sw, sh, dw, dh, M = GEOMS["rotated_zoom_out"]
    K = LR.camera_K(sw, sh)
    u, v, _ = LR.chain((dw, dh), LR.ray_matrix(M, K), LR.lens12(K, LR.LENS_B))
    mapx, mapy = u.astype(np.float32), v.astype(np.float32)
    xy, frac = cv2.convertMaps(mapx, mapy, cv2.CV_16SC2, nninterpolation=interp == NEAREST)
    assert xy.dtype == np.int16 and xy.shape == (dh, dw, 2) and frac.dtype == np.uint16 and frac.shape == (dh, dw)
    for dtype in (np.uint8, np.float32):
        for shape in ((sh, sw, 3), (sh, sw)):
            src = _src(shape, dtype, 800)
            for mode in (cv2.BORDER_CONSTANT, cv2.BORDER_REFLECT_101, cv2.BORDER_TRANSPARENT):
                exp = RR.remap(src, xy, frac, interp, mode, border_value=(5.0, 0, 0)[:1 if len(shape) == 2 else 3])
                got = cv2.remap(src, xy, frac if interp == LINEAR else None, interp, borderMode=mode, borderValue=5)  # (a bare number: channel 0 only)
                assert isinstance(got, np.ndarray) and got.dtype == src.dtype
                np.testing.assert_array_equal(got, exp)
                np.testing.assert_array_equal(cv2.remap(src, mapx, mapy, interp, borderMode=mode, borderValue=5), exp)            # float32 pair
                np.testing.assert_array_equal(cv2.remap(src, np.stack([mapx, mapy], -1), None, interp, borderMode=mode, borderValue=5), exp)  # (H, W, 2)
    src = _src((sh, sw, 3), np.uint8, 801)
    dst = np.full((dh, dw, 3), CANARY, np.uint8)
    got = cv2.remap(src, xy, frac, interp, dst=dst, borderMode=cv2.BORDER_TRANSPARENT)
    assert got is dst
    np.testing.assert_array_equal(dst, RR.remap(src, xy, frac, interp, RR.TRANSPARENT, canvas=np.full((dh, dw, 3), CANARY, np.uint8)))
    dst2 = np.zeros((dh, dw, 3), np.uint8)
    assert cv2.remap(src, xy, frac, interp, dst=dst2) is dst2
    np.testing.assert_array_equal(dst2, RR.remap(src, xy, frac, interp, RR.CONSTANT))
