"""Parity of the HIP path (through the C ABI of include/bevwarp.h) with the CPU oracle.
Bars (BASELINE.json north_star): uint8 / nearest pixel-for-pixel; float32 bilinear within 1e-5 absolute
(inputs in [0,1)) -- the kernel keeps the oracle's operation order, so float results are asserted
bit-identical as well.  Run on the GPU box:  python -m pytest tests -m gpu -x -q"""
import numpy as np
import pytest
import torch

from oracle import cpu_oracle as co
from tests import parity as P
from tests.parity import report_comparisons  # noqa: F401  (oracle comparisons per launch mode, written at the module's end)
from tests import workloads as wl

pytestmark = pytest.mark.gpu

F32_TOL = 1e-5


@pytest.fixture(scope="module")
def W():
    from bev_amd import warp
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return warp


def run_gpu(W, src_np, M, dsize, interp, **kw):
    """The warp in both launch modes (tests/parity.py): {mode: host result}."""
    t = src_np if isinstance(src_np, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(src_np)).cuda()
    if "out" not in kw:
        kw = dict(kw, out=P.poisoned_out(t, dsize))  # unwritten pixels must not pass as zeros
    return P.warp_modes(t, M, dsize, interp, **kw)


def check_one(got, exp):
    if exp.dtype == np.float32:
        assert np.abs(got - exp).max() <= F32_TOL
    np.testing.assert_array_equal(got, exp)


def check(res, exp):
    """Each launch mode's result against the oracle's `exp`."""
    P.check_modes(res, exp, check_one)


SHAPES = [
    ("brno", 1280, 720, 512, 512),      # BASELINE configs[0]
    ("brno", 1920, 1080, 320, 640),     # a real BrnoCompSpeed BEV size
    ("keystone", 1920, 1080, 1024, 1024),  # one frame of configs[1]
    ("keystone", 640, 360, 256, 192),
    ("brno", 192, 108, 37, 53),         # ragged destination
    ("keystone", 100, 60, 300, 9),      # height < 16: evaluation blocks are 113 wide
    ("brno", 64, 36, 70, 1),
    ("brno", 853, 481, 200, 120),       # source row stride not a multiple of 4: the two tap rows of a window differ in alignment
]


@pytest.mark.parametrize("kind,sw,sh,dw,dh", SHAPES)
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("interp", [0, 1])
def test_single_frame_parity(W, kind, sw, sh, dw, dh, dtype, interp):
    if kind == "brno":
        M = wl.synth_brno_H(sw, sh, dw, dh) if (sw * 9 == sh * 16) else wl.synth_brno_H(1920, 1080, dw, dh) @ np.diag([1920 / sw, 1080 / sh, 1.0])
    else:
        M = wl.keystone_H(sw, sh, dw, dh)
    src = wl.frame(0, sh, sw, dtype)
    check(run_gpu(W, src, M, (dw, dh), interp), co.warp_perspective(src, M, (dw, dh), interp))


@pytest.mark.parametrize("c", [1, 2, 4])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("interp", [0, 1])
def test_channel_counts(W, c, dtype, interp):
    M = wl.synth_brno_H(640, 360, 160, 200)
    src = wl.frame(3, 360, 640, dtype, c)
    check(run_gpu(W, src, M, (160, 200), interp), co.warp_perspective(src, M, (160, 200), interp))
    g = src[:, :, 0]
    got = run_gpu(W, g, M, (160, 200), interp)
    assert all(r.shape == (200, 160) for r in got.values())
    check(got, co.warp_perspective(g, M, (160, 200), interp))


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_batch_per_frame_and_shared_matrix(W, dtype):
    B, sw, sh, dw, dh = 5, 640, 360, 192, 160
    base = wl.keystone_H(sw, sh, dw, dh)
    Ms = np.stack([wl.jitter_H(base, i) for i in range(B)])
    frames = np.stack([wl.frame(i, sh, sw, dtype) for i in range(B)])
    t = torch.from_numpy(frames).cuda()
    got = run_gpu(W, t, Ms, (dw, dh), W.INTER_LINEAR)
    for i in range(B):
        check({m: r[i] for m, r in got.items()}, co.warp_perspective(frames[i], Ms[i], (dw, dh)))
    got = run_gpu(W, t, base, (dw, dh), W.INTER_LINEAR)
    for i in range(B):
        check({m: r[i] for m, r in got.items()}, co.warp_perspective(frames[i], base, (dw, dh)))
    with pytest.raises(ValueError):
        W.warp_perspective(t, Ms[:3], (dw, dh))
    # WARP_INVERSE_MAP and preallocated output (poisoned: unwritten pixels must not pass)
    out = torch.full((B, dh, dw, 3), 77, dtype=t.dtype, device="cuda")
    got = run_gpu(W, t, co.invert3x3(base), (dw, dh), W.INTER_LINEAR | W.WARP_INVERSE_MAP, out=out)  # (asserts the call returns `out`)
    check({m: r[2] for m, r in got.items()}, co.warp_perspective(frames[2], base, (dw, dh)))


def test_row_padding_and_frame_views(W):
    """Strided (row-padded) sources and destinations; a crop view is warped without a copy."""
    sw, sh, dw, dh = 600, 300, 128, 96
    M = wl.synth_brno_H(1920, 1080, dw, dh) @ np.diag([1920 / sw, 1080 / sh, 1.0])
    big = torch.from_numpy(wl.frame(7, sh, sw + 40, np.uint8)).cuda()
    view = big[:, 8:8 + sw]  # rows keep the pitch of the parent: not 16-byte aligned
    assert not view.is_contiguous()
    check(run_gpu(W, view, M, (dw, dh), 1), co.warp_perspective(np.ascontiguousarray(view.cpu().numpy()), M, (dw, dh)))
    view4 = big[:, 16:16 + 576]
    check(run_gpu(W, view4, M, (dw, dh), 1), co.warp_perspective(np.ascontiguousarray(view4.cpu().numpy()), M, (dw, dh)))


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_border_value_identity_translation(W, dtype):
    src = wl.frame(1, 90, 150, dtype)
    eye = np.eye(3)
    check(run_gpu(W, src, eye, (100, 60), 1), src[:60, :100])
    M = np.array([[1, 0, 5.0], [0, 1, -3.0], [0, 0, 1]])
    for interp in (0, 1):
        check(run_gpu(W, src, M, (170, 100), interp, border_value=[7, 200.4, 300][:3]),
              co.warp_perspective(src, M, (170, 100), interp, border_value=[7, 200.4, 300]))
    M = np.array([[1, 0, 0.5], [0, 1, 0.25], [0, 0, 1.0]])
    check(run_gpu(W, src, M, (160, 100), 1, border_value=50), co.warp_perspective(src, M, (160, 100), 1, border_value=50))
    # rotation by 90 degrees and a flip: exact permutations
    h, w = src.shape[:2]
    R = np.array([[0, -1, h - 1.0], [1, 0, 0], [0, 0, 1]])
    check(run_gpu(W, src, R, (h, w), 1), np.rot90(src, -1))
    Fm = np.array([[-1, 0, w - 1.0], [0, 1, 0], [0, 0, 1]])
    check(run_gpu(W, src, Fm, (w, h), 0), src[:, ::-1])


def test_degenerate_homographies(W):
    src = wl.frame(2, 64, 96, np.uint8)
    # singular forward matrix -> inverse all zeros -> W == 0 everywhere -> every pixel samples (0, 0)
    check(run_gpu(W, src, np.ones((3, 3)), (40, 30), 1), co.warp_perspective(src, np.ones((3, 3)), (40, 30), 1))
    # horizon inside the destination: W changes sign across the tile
    M = np.array([[1.0, 0.2, 3.0], [0.1, 1.0, 2.0], [0.0, 0.02, -0.5]])
    for interp in (0, 1):
        check(run_gpu(W, src, M, (128, 96), interp), co.warp_perspective(src, M, (128, 96), interp))
    # far outside: nothing in bounds
    T = np.array([[1, 0, 1e6], [0, 1, 0], [0, 0, 1.0]])
    check(run_gpu(W, src, T, (64, 64), 1), np.zeros((64, 64, 3), np.uint8))
    with pytest.raises(ValueError):
        W.warp_perspective(torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda"), np.full((3, 3), np.nan), (8, 8))
    with pytest.raises(ValueError):
        W.warp_perspective(torch.zeros((8, 8, 3), dtype=torch.int16, device="cuda"), np.eye(3), (8, 8))
    with pytest.raises(ValueError):
        W.warp_perspective(torch.zeros((8, 8, 3), dtype=torch.uint8), np.eye(3), (8, 8))


def test_magnification_and_minification_extremes(W):
    """x8 zoom (tiny source region per tile) and /6 shrink (every tap pair in a cache line of its own)."""
    src = wl.frame(4, 720, 1280, np.uint8)
    Z = np.array([[8.0, 0, -300.0], [0, 8.0, -200.0], [0, 0, 1]])
    check(run_gpu(W, src, Z, (512, 256), 1), co.warp_perspective(src, Z, (512, 256), 1))
    S = np.array([[1 / 6.0, 0.01, 1.0], [0.0, 1 / 6.0, 2.0], [0, 1e-5, 1]])
    for dtype in (np.uint8, np.float32):
        s = wl.frame(4, 720, 1280, dtype)
        check(run_gpu(W, s, S, (256, 128), 1), co.warp_perspective(s, S, (256, 128), 1))


def test_numpy_cv2_call_shape(W):
    """bev.warp.warpPerspective(img, H, (u, v)) is the drop-in for the call at vis_homo.py:89."""
    import bev.warp as bw
    img = wl.frame(5, 720, 1280, np.uint8)
    M = wl.synth_brno_H(1280, 720, 512, 512)
    out = bw.warpPerspective(img, M, (512, 512))
    assert out.dtype == np.uint8 and out.shape == (512, 512, 3)
    check_one(out, co.warp_perspective(img, M, (512, 512)))
    out = bw.warpPerspective(img, M, (512, 512), flags=bw.INTER_NEAREST, borderValue=(1, 2, 3))
    check_one(out, co.warp_perspective(img, M, (512, 512), 0, border_value=[1, 2, 3]))


def test_footprint_matches_oracle(W):
    M = wl.keystone_H(1920, 1080, 1024, 1024)
    counts, touched = W.footprint((1080, 1920), np.stack([M, wl.jitter_H(M, 1)]), (1024, 1024))
    n0, t0 = co.footprint((1080, 1920), M, (1024, 1024))
    assert int(counts[0]) == n0
    np.testing.assert_array_equal(touched[0].cpu().numpy(), t0)
    n1, _ = co.footprint((1080, 1920), wl.jitter_H(M, 1), (1024, 1024))
    assert int(counts[1]) == n1
    c, _ = W.footprint((360, 640), wl.synth_brno_H(640, 360, 128, 128), (128, 128), flags=W.INTER_NEAREST)
    assert int(c[0]) == co.footprint((360, 640), wl.synth_brno_H(640, 360, 128, 128), (128, 128), 0)[0]


# ---- BASELINE.json full sizes: oracle on sampled frames + size-independent properties -----------------
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_config2_batch32_1080p_to_1024(W, dtype):
    B, sw, sh, dw, dh = 32, 1920, 1080, 1024, 1024
    base = wl.keystone_H(sw, sh, dw, dh)
    Ms = np.stack([wl.jitter_H(base, i) for i in range(B)])
    frames = torch.empty((B, sh, sw, 3), dtype=torch.uint8 if dtype == np.uint8 else torch.float32, device="cuda")
    host = {}
    for i in range(B):
        f = wl.frame(i, sh, sw, dtype)
        if i in (0, 13, 31):
            host[i] = f
        frames[i] = torch.from_numpy(f).cuda()
    res = run_gpu(W, frames, Ms, (dw, dh), 1)
    for i, f in host.items():
        check({m: r[i] for m, r in res.items()}, co.warp_perspective(f, Ms[i], (dw, dh), nthreads=8))
    np.testing.assert_array_equal(res["table"], res["plain"])  # (the frames without an oracle run: both modes agree)
    out = torch.from_numpy(res["plain"]).cuda()
    del res
    # property: same frames, same matrix -> identical outputs, regardless of batch position
    frames[5] = frames[0]
    Ms2 = Ms.copy()
    Ms2[5] = Ms[0]
    out2 = W.warp_perspective(frames, Ms2, (dw, dh))
    assert torch.equal(out2[5], out2[0]) and torch.equal(out2[0], out[0])
    # property: identity homography reproduces the top-left crop for every frame
    crop = W.warp_perspective(frames, np.eye(3), (dw, dh))
    assert torch.equal(crop, frames[:, :dh, :dw])
    if dtype == np.float32:
        # property: bilinear sampling is linear in the image
        a, b = frames[:4], frames[4:8]
        lhs = W.warp_perspective(0.25 * a + 0.5 * b, Ms[:4], (dw, dh))
        rhs = 0.25 * W.warp_perspective(a, Ms[:4], (dw, dh)) + 0.5 * W.warp_perspective(b, Ms[:4], (dw, dh))
        assert (lhs - rhs).abs().max().item() < 1e-6


@pytest.mark.parametrize("dtype,interp,kind", [(np.uint8, 0, "keystone"), (np.uint8, 0, "brno"), (np.uint8, 1, "brno"), (np.uint8, 1, "rot25"),
                                               (np.uint8, 0, "rot25"), (np.float32, 0, "keystone"), (np.float32, 1, "brno")])
def test_config2_size_other_paths(W, dtype, interp, kind):
    """configs[1]'s launch size (32 x 1080p -> 1024^2: 24-row tiles, full-height tiles as straight-line code, the tail split) on
    the paths test_config2_batch32_1080p_to_1024 does not take: nearest neighbour (every pass issued up front), the Brno-style and a
    25-degree footprint (patches, edge-cut and outside tiles).  Oracle on three frames of the batch."""
    B, sw, sh, dw, dh = 32, 1920, 1080, 1024, 1024
    base = {"keystone": wl.keystone_H, "brno": wl.synth_brno_H}[kind](sw, sh, dw, dh) if kind != "rot25" else wl.rotated_H(sw, sh, dw, dh, 25.0, 0.6)
    Ms = np.stack([wl.jitter_H(base, i) for i in range(B)])
    host = {i: wl.frame(60 + i, sh, sw, dtype) for i in (0, 17, 31)}
    frames = torch.empty((B, sh, sw, 3), dtype=torch.uint8 if dtype == np.uint8 else torch.float32, device="cuda")
    f0 = torch.from_numpy(host[0]).cuda()
    for i in range(B):
        frames[i] = torch.from_numpy(host[i]).cuda() if i in host else f0.flip(i % 2)
    res = run_gpu(W, frames, Ms, (dw, dh), interp)
    for i, f in host.items():
        check({m: r[i] for m, r in res.items()}, co.warp_perspective(f, Ms[i], (dw, dh), interp, nthreads=8))
    np.testing.assert_array_equal(res["table"], res["plain"])
    out = torch.from_numpy(res["plain"]).cuda()
    del res
    # a frame's result does not depend on its place in the batch (frames 1.. are flips of frame 0: redo one of them alone)
    j = 6
    alone = W.warp_perspective(frames[j:j + 1], Ms[j:j + 1], (dw, dh), flags=interp)
    assert torch.equal(alone[0], out[j])


def test_config4_single_4k_frame(W):
    """One frame of configs[3] (3840x2160 -> 2048x2048, uint8); the 8-GPU sharding is covered in test_shard.py."""
    sw, sh, dw, dh = 3840, 2160, 2048, 2048
    M = wl.keystone_H(sw, sh, dw, dh)
    f = wl.frame(0, sh, sw, np.uint8)
    check(run_gpu(W, f, M, (dw, dh), 1), co.warp_perspective(f, M, (dw, dh), nthreads=8))
    Mb = wl.synth_brno_H(sw, sh, dw, dh)
    check(run_gpu(W, f, Mb, (dw, dh), 1), co.warp_perspective(f, Mb, (dw, dh), nthreads=8))


# ---- every tile shape of the one kernel: ragged last tiles (destination width not a multiple of 256 / 128), fewer than
# ---- 16 rows (evaluation blocks wider than 64 px, lanes straddling them), destinations whose layout rules out the wide
# ---- stores, tiny frames -- all through the row-classified path, all bit-exact with the oracle.
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("interp", [0, 1])
def test_every_tile_shape_matches_oracle(W, dtype, interp):
    cases = [("keystone", 1920, 1080, 1024, 1024), ("brno", 1280, 720, 512, 512), ("brno", 192, 108, 37, 53),
             ("keystone", 856, 480, 300, 200), ("keystone", 100, 60, 300, 9), ("keystone", 640, 360, 1000, 3),
             ("brno", 640, 360, 333, 7), ("keystone", 640, 360, 257, 40), ("brno", 640, 360, 129, 33)]
    for kind, sw, sh, dw, dh in cases:
        M = (wl.synth_brno_H if kind == "brno" else wl.keystone_H)(sw, sh, dw, dh)
        src = wl.frame(2, sh, sw, dtype)
        check(run_gpu(W, src, M, (dw, dh), interp), co.warp_perspective(src, M, (dw, dh), interp))
    # 4-channel and 1-channel pixels, row-padded source view, border value
    M = wl.synth_brno_H(640, 360, 160, 200)
    for c in (1, 4):
        src = wl.frame(3, 360, 640, dtype, c)
        check(run_gpu(W, src, M, (160, 200), interp, border_value=9), co.warp_perspective(src, M, (160, 200), interp, border_value=9))
    big = torch.from_numpy(wl.frame(7, 300, 640, dtype)).cuda()
    view = big[:, 16:16 + 576]
    Mv = wl.keystone_H(576, 300, 128, 96)
    check(run_gpu(W, view, Mv, (128, 96), interp), co.warp_perspective(np.ascontiguousarray(view.cpu().numpy()), Mv, (128, 96), interp))
    # odd destination widths: rows start at byte offsets that rule out the wide stores
    for c in (1, 2, 3):
        src = wl.frame(5, 200, 320, dtype, c)
        Mo = wl.synth_brno_H(320, 200, 301, 41)
        check(run_gpu(W, src, Mo, (301, 41), interp), co.warp_perspective(src, Mo, (301, 41), interp))


def test_config4_full_per_gpu_shard_properties(W):
    """configs[3] at the size one GPU holds: 32 x (3840x2160 -> 2048x2048) uint8, per-frame homographies.  Oracle on three
    frames; size-independent properties on all of them (a frame's result does not depend on its batch position, the identity
    homography reproduces the crop, frames of one launch do not leak into each other)."""
    sw, sh, dw, dh, B = 3840, 2160, 2048, 2048, 32
    base = wl.keystone_H(sw, sh, dw, dh)
    Ms = np.stack([wl.jitter_H(base, i) for i in range(B)])
    uniq = [torch.from_numpy(wl.frame(80 + i, sh, sw, np.uint8)).cuda() for i in range(4)]
    frames = torch.empty((B, sh, sw, 3), dtype=torch.uint8, device="cuda")
    for i in range(B):
        frames[i] = uniq[i % 4] if i < 4 else uniq[i % 4].flip(i % 2)
    res = run_gpu(W, frames, Ms, (dw, dh), 1)
    for i in (0, 3, 31):
        exp = co.warp_perspective(frames[i].cpu().numpy(), Ms[i], (dw, dh), nthreads=8)
        P.check_modes({m: r[i] for m, r in res.items()}, exp, lambda got, exp: np.testing.assert_array_equal(got, exp, err_msg="frame %d" % i))
    np.testing.assert_array_equal(res["table"], res["plain"])
    out = torch.from_numpy(res["plain"]).cuda()
    del res
    # batch-position invariance: frame 5 and its homography moved to slot 29 (and the reverse) give the same pixels
    perm = list(range(B))
    perm[5], perm[29] = 29, 5
    out_p = W.warp_perspective(frames[perm], Ms[perm], (dw, dh))
    assert torch.equal(out_p[29], out[5]) and torch.equal(out_p[5], out[29]) and torch.equal(out_p[11], out[11])
    # a shard is the same as its frames one by one (no leakage between frames of a launch)
    for i in (7, 30):
        assert torch.equal(W.warp_perspective(frames[i], Ms[i], (dw, dh)), out[i])
    # identity homography: the top-left crop of every frame, nearest and bilinear
    for flags in (0, 1):
        crop = W.warp_perspective(frames, np.eye(3), (dw, dh), flags=flags)
        assert torch.equal(crop, frames[:, :dh, :dw])
    del frames, out, out_p, crop
    torch.cuda.empty_cache()


def test_side_by_side_rois_of_one_image(W):
    """warping the left-half ROI of an image into its right-half ROI (equal row strides, disjoint byte columns) is a
    call cv2.warpPerspective accepts; the overlap guard must not refuse it -- and must still refuse ROIs that share a column,
    with a message that names the overlap."""
    h, w = 240, 512
    for dtype in (np.uint8, np.float32):
        img = wl.frame(11, h, w, dtype)
        big = torch.from_numpy(img).cuda()
        left, right = big[:, :w // 2], big[:, w // 2:]
        M = wl.keystone_H(w // 2, h, w // 2, h)
        exp = co.warp_perspective(np.ascontiguousarray(img[:, :w // 2]), M, (w // 2, h))
        check(run_gpu(W, left, M, (w // 2, h), 1, out=right), exp)  # (asserts the call returns `right`)
        check_one(big[:, w // 2:].cpu().numpy(), exp)
        np.testing.assert_array_equal(big[:, :w // 2].cpu().numpy(), img[:, :w // 2])  # the source half is untouched
        with pytest.raises(ValueError, match="overlap"):
            W.warp_perspective(left, M, (w // 2, h), out=big[:, w // 2 - 1:w - 1])
        with pytest.raises(ValueError, match="overlap"):
            W.warp_perspective(big, np.eye(3), (w, h), out=big)


def test_validated_launch_cache_hits_and_misses(W):
    """the plan cache of warp_perspective (bev_amd/warp.py::_plans).  A second identical call takes the cached
    launch and equals the oracle; a matrix tensor of another dtype or on another device -- the allocator can hand a recycled
    address to either -- must still run into the slow path's validation; the cache clears itself at _PLANS_MAX."""
    sw, sh, dw, dh = 320, 180, 128, 96
    M = wl.synth_brno_H(sw, sh, dw, dh)
    f0, f1 = wl.frame(1, sh, sw, np.uint8), wl.frame(2, sh, sw, np.uint8)
    src, out = torch.from_numpy(f0).cuda(), torch.empty((dh, dw, 3), dtype=torch.uint8, device="cuda")
    minv = W.device_inverse(M, src.device)
    W._plans.clear()
    W.warp_perspective(src, None, (dw, dh), out=out, M_inv_device=minv)
    assert len(W._plans) == 1
    src.copy_(torch.from_numpy(f1).cuda())
    W.warp_perspective(src, None, (dw, dh), out=out, M_inv_device=minv)  # the hit: same buffers, new pixels
    torch.cuda.synchronize()
    assert len(W._plans) == 1
    check_one(out.cpu().numpy(), co.warp_perspective(f1, M, (dw, dh)))
    # same shape and strides, other dtype: 36-byte matrices must not be read as 72-byte ones
    with pytest.raises(ValueError):
        W.warp_perspective(src, None, (dw, dh), out=out, M_inv_device=minv.to(torch.float32))
    with pytest.raises(ValueError):
        W.warp_perspective(src, None, (dw, dh), out=out, M_inv_device=minv.cpu())
    # a key that differs only in the matrix tensor's dtype is a different key even at the same address (simulated: the real
    # thing needs the allocator to recycle the block)
    (key, plan), = list(W._plans.items())
    assert torch.float64 in key and src.device in key
    # the cache empties itself rather than grow without bound
    for i in range(W._PLANS_MAX + 3):
        W._plans[("filler", i)] = plan
    W.warp_perspective(src, None, (dw, dh), out=torch.empty_like(out), M_inv_device=minv)
    assert len(W._plans) <= 4
    W._plans.clear()


@pytest.mark.parametrize("shape,dsize", [((1080, 1920, 3), (852, 480)), ((720, 1280, 3), (640, 360)), ((37, 53, 1), (100, 64)), ((64, 48, 4), (31, 17)),
                                         ((5, 7, 3), (1, 1)), ((1, 1, 3), (9, 4)), ((480, 852, 2), (1920, 1080)), ((33, 65), (17, 9)), ((40, 64, 3), (32, 20))])
def test_resize_matches_the_oracle(shape, dsize):
    """bevwarp_resize == oracle/resize_oracle.c (cv2.resize INTER_LINEAR uint8 as called at vis_homo.py:90; parity unpinned) bit for bit:
    the reference's own 1080p -> 852 x 480, magnification, 1-4 channels, degenerate sizes, the exact 2 x 2 box-mean case."""
    from bev_amd.resize import cv2_resize, resize
    c = shape[2] if len(shape) == 3 else 1
    img = wl.frame(21, shape[0], shape[1], np.uint8, c)
    if len(shape) == 2:
        img = img[:, :, 0]
    exp = co.resize_linear_u8(img, dsize)
    got = resize(torch.from_numpy(img).cuda(), dsize)
    torch.cuda.synchronize()
    assert got.shape == exp.shape
    np.testing.assert_array_equal(got.cpu().numpy(), exp)
    np.testing.assert_array_equal(cv2_resize(img, dsize), exp)  # numpy in, numpy out: cv2's call shape


def test_resize_batches_views_and_errors():
    from bev_amd.resize import cv2_resize, resize
    frames = np.stack([wl.frame(30 + i, 90, 160, np.uint8) for i in range(5)])
    t = torch.from_numpy(frames).cuda()
    got = resize(t, (71, 40)).cpu().numpy()
    for i in range(5):
        np.testing.assert_array_equal(got[i], co.resize_linear_u8(frames[i], (71, 40)))
    big = torch.from_numpy(wl.frame(7, 90, 200, np.uint8)).cuda()
    view = big[:, 8:168]  # row-padded view, no copy
    out = torch.full((40, 71, 3), 77, dtype=torch.uint8, device="cuda")
    assert resize(view, (71, 40), out=out) is out
    np.testing.assert_array_equal(out.cpu().numpy(), co.resize_linear_u8(np.ascontiguousarray(view.cpu().numpy()), (71, 40)))
    np.testing.assert_array_equal(cv2_resize(frames[0], None, fx=0.5, fy=0.5), co.resize_linear_u8(frames[0], (80, 45)))  # exact 2 x 2: the box mean
    with pytest.raises(ValueError):
        resize(t.float(), (8, 8))
    with pytest.raises(ValueError):
        resize(t, (8, 8), interpolation=0)
    with pytest.raises(ValueError):
        resize(t, (0, 8))
    with pytest.raises(ValueError, match="overlap"):
        resize(big[:, :100], (100, 90), out=big[:, 50:150])


def test_two_step_small_branch_pixel_for_pixel():
    """vis_homo.py:73-78,90-91 as the reference runs it: resize to 852 x 480, then warp with the scaled calibration's homography; both
    steps on the device, compared with the oracle's two steps."""
    from bev_amd.resize import resize
    from bev_amd import warp
    img = wl.frame(0, 1080, 1920, np.uint8)
    M_small = wl.synth_brno_H(852, 480, 320, 640)
    t = torch.from_numpy(img).cuda()
    got = run_gpu(warp, resize(t, (852, 480)), M_small, (320, 640), 1)
    exp = co.warp_perspective(co.resize_linear_u8(img, (852, 480)), M_small, (320, 640), 1)
    check(got, exp)


def test_resize_random_shapes():
    """40 seeded random (source, destination, channels) triples -- strong minification, magnification, one-pixel sides, odd sizes --
    through bevwarp_resize against the oracle, bit for bit."""
    from bev_amd.resize import resize
    rng = np.random.default_rng(2024)
    for _ in range(40):
        sh, sw = int(rng.integers(1, 200)), int(rng.integers(1, 300))
        dh, dw = int(rng.integers(1, 260)), int(rng.integers(1, 400))
        c = int(rng.integers(1, 5))
        img = rng.integers(0, 256, (sh, sw, c), dtype=np.uint8)
        got = resize(torch.from_numpy(img).cuda(), (dw, dh)).cpu().numpy()
        np.testing.assert_array_equal(got, co.resize_linear_u8(img, (dw, dh)), err_msg="%dx%dx%d -> %dx%d" % (sw, sh, c, dw, dh))


@pytest.mark.gpu
def test_resize_four_pixels_per_lane_kernel_corners():
    """The batch form of bevwarp_resize (four destination pixels per lane, 8-byte tap windows, dword stores): every channel count, right edges of
    0-3 pixels beyond the last full lane, one-tap columns at the end of a row (strong magnification keeps many of them), source rows of
    exactly 8 bytes, a row-padded destination whose rows still start 4-byte aligned (fast kernel) and one whose rows do not (one-pixel
    kernel), batches -- bit for bit against the oracle."""
    from bev_amd.resize import resize
    rng = np.random.default_rng(99)
    cases = []
    for c in (1, 2, 3, 4):
        for dw in (4 * 37, 4 * 37 + 4 // np.gcd(4, c)):  # rows of dw * c bytes, multiples of 4: the fast kernel, full and ragged last lanes
            cases.append((61, max(8 // c, 3) + int(rng.integers(0, 90)), c, 47, dw))
        cases.append((33, (8 + c - 1) // c, c, 20, 64))      # a source row of 8 bytes (or the first count above it): magnification, one-tap columns
        cases.append((50, 97, c, 31, 400))                    # 4 x magnification
    for sh, sw, c, dh, dw in cases:
        img = rng.integers(0, 256, (3, sh, sw, c), dtype=np.uint8)
        got = resize(torch.from_numpy(img).cuda(), (dw, dh)).cpu().numpy()
        for i in range(3):
            np.testing.assert_array_equal(got[i], co.resize_linear_u8(img[i], (dw, dh)).reshape(dh, dw, c), err_msg="%dx%dx%d -> %dx%d" % (sw, sh, c, dw, dh))
    img = rng.integers(0, 256, (120, 213, 3), dtype=np.uint8)
    exp = co.resize_linear_u8(img, (100, 56))
    src_t = torch.from_numpy(img).cuda()
    for pad in (4, 3):  # padded destination rows: 100 * 3 + 12 bytes apart (aligned: fast kernel), 100 * 3 + 9 (not: one-pixel kernel)
        hold = torch.full((56, 100 + pad, 3), 9, dtype=torch.uint8, device="cuda")
        view = hold[:, :100]
        from bev_amd import _lib
        import ctypes
        st = _lib.load().bevwarp_resize(src_t.data_ptr(), view.data_ptr(), 1, 120, 213, 56, 100, 3, 120 * 213 * 3, 213 * 3, view.stride(0) * 56, view.stride(0),
                                        _lib.U8, _lib.INTER_LINEAR, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert st == 0
        torch.cuda.synchronize()
        np.testing.assert_array_equal(view.cpu().numpy(), exp)
        assert (hold[:, 100:].cpu().numpy() == 9).all()  # the padding is not written


def test_tile_verdict_tables_reproduce_the_plain_call():
    """bevwarp_warp_classes (ABI v7): a table filled once for given matrices and geometry, then read by later launches instead of
    classifying every tile again.  The filled launch writes no pixel; launches that use the table equal bevwarp_warp bit for bit --
    keystone (pair tiles, edge-cut tiles), Brno-style (turned, outside tiles), 8-bit and float, both interpolations; entries that
    were never filled fall back to classification; and the Python entry picks tables up by itself for matrices it owns."""
    import ctypes
    from bev_amd import _lib, warp
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for (B, sw, sh, dw, dh) in ((32, 640, 360, 512, 768), (3, 700, 420, 300, 77)):  # tall-tile launch with a split tail / a small one
        for kind in ("keystone", "brno"):
            base = (wl.keystone_H if kind == "keystone" else wl.synth_brno_H)(sw, sh, dw, dh)
            Ms = np.stack([wl.jitter_H(base, g) for g in range(B)])
            minv = warp.device_inverse(Ms, dev)
            for tdt, ndt, dt, esz in ((torch.uint8, np.uint8, 0, 1), (torch.float32, np.float32, 1, 4)):
                src = torch.stack([torch.from_numpy(wl.frame(70 + g % 3, sh, sw, ndt)) for g in range(B)]).to(dev)
                for interp in (1, 0):
                    n = lib.bevwarp_tile_classes_bytes(B, sh, sw, dh, dw, 3, dt, interp)
                    assert n > 0 and n % 12 == 0
                    table = torch.zeros(n // 4, dtype=torch.int32, device=dev)
                    ref = torch.full((B, dh, dw, 3), 7, dtype=tdt, device=dev)
                    got = torch.full((B, dh, dw, 3), 9, dtype=tdt, device=dev)
                    args = lambda d: (src.data_ptr(), d.data_ptr(), B, sh, sw, dh, dw, 3, src.stride(0) * esz, src.stride(1) * esz, d.stride(0) * esz,
                                      d.stride(1) * esz, minv.data_ptr(), B, dt, interp, None)
                    assert lib.bevwarp_warp(*args(ref), ctypes.c_void_p(stream)) == 0
                    assert lib.bevwarp_warp_classes(*args(got), table.data_ptr(), 1, ctypes.c_void_p(stream)) == 0  # fill: no pixel written
                    torch.cuda.synchronize()
                    assert bool((got == 9).all())
                    t = table.cpu().numpy().view(np.uint32)
                    assert ((t >> 31) == 1).sum() >= B * ((dw + 255) // 256)  # every launched workgroup left its verdict
                    assert lib.bevwarp_warp_classes(*args(got), table.data_ptr(), 0, ctypes.c_void_p(stream)) == 0
                    torch.cuda.synchronize()
                    assert torch.equal(got, ref), (kind, dt, interp)
                    # half the entries wiped: those tiles are classified as usual
                    table[::2] = 0
                    got.fill_(9)
                    assert lib.bevwarp_warp_classes(*args(got), table.data_ptr(), 0, ctypes.c_void_p(stream)) == 0
                    torch.cuda.synchronize()
                    assert torch.equal(got, ref)
    # the Python entry: matrices owned by device_inverse get a table on their first launch and use it from then on
    warp._class_tables.clear()
    sw, sh, dw, dh, B = 640, 360, 512, 96, 2
    Ms = np.stack([wl.jitter_H(wl.keystone_H(sw, sh, dw, dh), g) for g in range(B)])
    frames = np.stack([wl.frame(80 + g, sh, sw, np.uint8) for g in range(B)])
    t = torch.from_numpy(frames).to(dev)
    first = warp.warp_perspective(t, Ms, (dw, dh)).cpu().numpy()
    assert len(warp._class_tables) == 1
    second = warp.warp_perspective(t, Ms, (dw, dh)).cpu().numpy()
    assert len(warp._class_tables) == 1
    for g in range(B):
        exp = co.warp_perspective(frames[g], Ms[g], (dw, dh), 1)
        np.testing.assert_array_equal(first[g], exp)
        np.testing.assert_array_equal(second[g], exp)
    mine = warp.device_inverse(Ms, dev).clone()  # a tensor the caller owns: no table is kept for it
    warp.warp_perspective(t, None, (dw, dh), M_inv_device=mine)
    assert len(warp._class_tables) == 1


# ---- the verdict-table cache of the Python entry (bev_amd/warp.py::_tile_classes, _plans): a table is trusted by the kernel, so it
# ---- must never outlive the matrix contents, the memory or the fill it belongs to.
def _class_entry(W, minv):
    hits = [v for k, v in W._class_tables.items() if k[0] == minv.data_ptr() and v[1] is minv]
    assert len(hits) == 1
    return hits[0]


def test_verdict_tables_follow_in_place_writes_of_the_matrices(W):
    """A device_inverse tensor rewritten in place (minv.copy_) after its table was filled: the next launch -- through the slow path, and
    through a plan that carries the old table -- refills it and equals the oracle of the new matrices; the value cache stops handing the
    rewritten tensor out for the old key.  The matrices are chosen so that stale verdicts could only err on the safe side: the new map
    (a translation) keeps the whole destination deep inside the frame, the old one is the same map shifted right so that the right half
    of the destination leaves the frame -- a stale table says outside / edge-cut where the truth is interior (border pixels: a clean
    mismatch), never the reverse."""
    sw, sh, dw, dh = 640, 360, 512, 64
    dev = torch.device("cuda", 0)
    f = wl.frame(50, sh, sw, np.uint8)
    src = torch.from_numpy(f).to(dev)
    M2 = np.array([[1, 0, -40.0], [0, 1, -100.0], [0, 0, 1]])  # destination (x, y) samples source (x + 40, y + 100)
    exp = co.warp_perspective(f, M2, (dw, dh), 1)
    inv2 = torch.from_numpy(W.invert_homography(M2).reshape(1, 3, 3)).to(dev)
    for ty, path in ((100.0, "slow path"), (101.0, "plan")):
        M = np.array([[1, 0, -400.0], [0, 1, -ty], [0, 0, 1]])  # source x 400 .. 911: tiles right of x = 240 sample outside the frame
        minv = W.device_inverse(M, dev)
        out = torch.full((dh, dw, 3), 77, dtype=torch.uint8, device=dev)
        if path == "plan":
            W.warp_perspective(src, None, (dw, dh), out=out, M_inv_device=minv)  # fills the table, stores a plan that carries it
            assert any(p[3] is not None and p[4] is minv for p in W._plans.values())
        else:
            W.warp_perspective(src, None, (dw, dh), M_inv_device=minv)
        torch.cuda.synchronize()
        old = _class_entry(W, minv)
        minv.copy_(inv2)
        if path == "plan":
            got = W.warp_perspective(src, None, (dw, dh), out=out, M_inv_device=minv)
            assert got is out
        else:
            got = W.warp_perspective(src, None, (dw, dh), M_inv_device=minv)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got.cpu().numpy(), exp, err_msg=path)
        new = _class_entry(W, minv)
        assert new[0] is not old[0] and new[2] == minv._version  # refilled for the written contents
        again = W.device_inverse(M, dev)
        assert again is not minv
        np.testing.assert_array_equal(again.cpu().numpy(), W.invert_homography(M).reshape(1, 3, 3))


def _recording_lib(monkeypatch, on_call):
    """Installs a proxy of the loaded library as bev_amd._lib.load(): on_call(name, args) runs after every warp entry point's call.
    Installed before the calls under test, so their plans store the wrapped callables too."""
    from bev_amd import _lib
    real = _lib.load()

    class Recording:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if not name.startswith("bevwarp_warp"):
                return fn

            def call(*args):
                st = fn(*args)
                on_call(name, args)
                return st
            return call
    proxy = Recording()
    monkeypatch.setattr(_lib, "load", lambda: proxy)
    return real


def test_graph_capture_through_a_plan_with_a_table(W, monkeypatch):
    """tools.graphed_step.GraphedStep after eager warm-up calls that stored a plan carrying a verdict table: the capture must launch the
    plain entry point (a graph would replay the table's address, which nothing keeps alive).  Asserted on the host before the graph is
    ever replayed; then the table is dropped from every cache, the allocator hands its memory out again filled with bogus verdicts, and
    three replays on new frames equal the oracle."""
    from tools.graphed_step import GraphedStep
    launched = []
    real = _recording_lib(monkeypatch, lambda name, args: launched.append((name, torch.cuda.is_current_stream_capturing())))
    W._plans.clear()
    sw, sh, dw, dh = 640, 360, 512, 64
    M = wl.keystone_H(sw, sh, dw, dh)
    src = torch.zeros((sh, sw, 3), dtype=torch.uint8, device="cuda")
    out = torch.empty((dh, dw, 3), dtype=torch.uint8, device="cuda")
    minv = W.device_inverse(M, src.device)
    g = GraphedStep(lambda: W.warp_perspective(src, None, (dw, dh), out=out, M_inv_device=minv))
    eager = [n for n, capturing in launched if not capturing]
    captured = [n for n, capturing in launched if capturing]
    assert eager.count("bevwarp_warp_classes") >= 2  # warm-up: the fill, then launches reading the table (the last ones through the plan)
    assert any(p[3] is not None for p in W._plans.values())
    assert captured == ["bevwarp_warp"], captured
    nbytes = real.bevwarp_tile_classes_bytes(1, sh, sw, dh, dw, 3, 0, 1)
    W._plans.clear()
    W._class_tables.clear()
    churn = [torch.full((nbytes // 4,), -0x7ffffffe, dtype=torch.int32, device="cuda") for _ in range(16)]  # 0x80000002: "outside"
    torch.cuda.synchronize()
    for i in range(3):
        f = wl.frame(90 + i, sh, sw, np.uint8)
        src.copy_(torch.from_numpy(f).cuda())
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), co.warp_perspective(f, M, (dw, dh), 1))
    del churn
    W._plans.clear()  # (they hold the recording proxy's callables)


def test_verdict_table_filled_on_one_stream_is_used_on_another(W, monkeypatch):
    """The first call, on stream A held back by a spin of some tens of ms, fills the table; a call on stream B then finds it in the cache.
    The fill must have run before the table is cached -- asserted on the host before anything is launched on B -- and B's launch,
    which reads the table, equals the oracle."""
    dev = torch.device("cuda", 0)
    fills, uses = [], []

    def on_call(name, args):
        if name == "bevwarp_warp_classes":
            if args[-2] == 1:  # BEVWARP_CLASSES_FILL: mark the point right behind the fill on its stream
                ev = torch.cuda.Event()
                ev.record(torch.cuda.ExternalStream(args[-1].value, device=dev))
                fills.append(ev)
            else:
                uses.append(args[-1].value)
    _recording_lib(monkeypatch, on_call)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    torch.cuda._sleep(1000000)
    t1.record()
    t1.synchronize()
    cycles = int(min(max(1e6 * 40.0 / max(t0.elapsed_time(t1), 1e-3), 1e6), 5e8))  # ~40 ms, bounded
    sw, sh, dw, dh = 640, 360, 448, 72
    M = wl.jitter_H(wl.keystone_H(sw, sh, dw, dh), 3)
    f = wl.frame(95, sh, sw, np.uint8)
    src = torch.from_numpy(f).to(dev)
    W.device_inverse(M, dev)  # (uploaded now: the upload on a miss is a blocking copy, which would wait for the spin below by itself)
    a, b = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    a.wait_stream(torch.cuda.current_stream(dev))
    b.wait_stream(torch.cuda.current_stream(dev))
    spun = torch.cuda.Event()
    with torch.cuda.stream(a):
        torch.cuda._sleep(cycles)
        spun.record(a)
        assert not spun.query()  # (A is still held back when the fill is queued behind the spin)
        out_a = W.warp_perspective(src, M, (dw, dh))
    assert len(fills) == 1
    assert fills[0].query(), "the verdict table was cached before its fill had run"
    with torch.cuda.stream(b):
        out_b = W.warp_perspective(src, M, (dw, dh))
    assert len(fills) == 1 and uses[-1] == b.cuda_stream  # B read the cached table
    torch.cuda.synchronize()
    exp = co.warp_perspective(f, M, (dw, dh), 1)
    np.testing.assert_array_equal(out_b.cpu().numpy(), exp)
    np.testing.assert_array_equal(out_a.cpu().numpy(), exp)
    W._plans.clear()
