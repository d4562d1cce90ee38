"""The multi-camera warp on the GPU (bev_amd.warp.warp_stitch -> bevwarp_warp_stitch), each result compared with the numpy reference
tests/stitch_ref.py bit for bit.  Destinations are pre-filled with 77, so a pixel a launch leaves unwritten does not pass as zero.
Run on the GPU box:  python -m pytest tests -m gpu -q"""
import numpy as np
import pytest
import torch

from tests import border_ref as BR
from tests import pixels as PX
from tests import stitch_ref as SR

pytestmark = pytest.mark.gpu

LINEAR, NEAREST, INVERSE = 1, 0, 16
# three cameras on a 260 x 22 canvas (two tile columns, six tile rows, a ragged last lane): (w, h, inverse map)
SCENE = [(40, 24, np.array([[0.30, 0.20, -4], [0.01, 0.90, -1], [0.0004, 0, 1]])),
         (64, 18, np.array([[0.38, 0, -36], [0.02, 0.80, -3], [0, 0, 1]])),
         (31, 33, np.array([[-0.35, 0, 80], [0, 1.40, -2], [0, 0.001, 1]]))]
DSIZE = (260, 22)
BLENDS = (("over", 64), ("feather", 1), ("feather", 3), ("feather", 64))
MODES = (BR.CONSTANT, BR.TRANSPARENT)


@pytest.fixture(scope="module")
def W():
    from bev_amd import warp
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return warp


def _src(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, shape, dtype=np.uint8) if dtype == np.uint8 else rng.random(shape, dtype=np.float32)


def _scene(dtype, c=3):
    """The scene's sources ((h, w, c); c = 0: (h, w)) and inverse maps."""
    return [_src((h, w, c) if c else (h, w), dtype, seed=30 + 4 * k + c) for k, (w, h, _) in enumerate(SCENE)], [M for _, _, M in SCENE]


def _bv(c):
    return (3.0, 200.0, 41.0, 117.0)[:max(c, 1)]


def gpu(W, srcs, Ms, dsize, interp, blend, feather, mode, border_value=None):
    ts = [torch.from_numpy(np.ascontiguousarray(s)).cuda() for s in srcs]
    out = torch.full((int(dsize[1]), int(dsize[0])) + tuple(srcs[0].shape[2:]), 77, dtype=ts[0].dtype, device="cuda")
    got = W.warp_stitch(ts, Ms, dsize, flags=interp | INVERSE, blend=blend, feather=feather, border_value=border_value, out=out, border_mode=mode)
    torch.cuda.synchronize()
    assert got is out
    return got.cpu().numpy()


def ref(srcs, Ms, dsize, interp, blend, feather, mode, border_value=0.0):
    canvas = np.full((int(dsize[1]), int(dsize[0])) + tuple(srcs[0].shape[2:]), 77, srcs[0].dtype)
    return SR.stitch(srcs, Ms, dsize, interp, SR.FEATHER if blend == "feather" else SR.OVER, feather, mode, border_value, canvas)


def check(W, srcs, Ms, dsize, interp, blend, feather, mode, border_value=0.0):
    got = gpu(W, srcs, Ms, dsize, interp, blend, feather, mode, border_value)
    exp, count = ref(srcs, Ms, dsize, interp, blend, feather, mode, border_value)
    np.testing.assert_array_equal(got, exp, err_msg="%s F=%d mode %d interp %d %s %s" % (blend, feather, mode, interp, srcs[0].dtype, srcs[0].shape))
    if mode == BR.TRANSPARENT:  # the canvas keeps 77 exactly where no camera covers
        assert (got[count == 0] == 77).all()
    return count


# ---- 1. the scene: every format, blend and border ----

@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_scene_matrix(W, dtype, interp):
    for c in (1, 2, 3, 4, 0):  # (0: (H, W) sources)
        srcs, Ms = _scene(dtype, c)
        for blend, F in BLENDS:
            for mode in MODES:
                count = check(W, srcs, Ms, DSIZE, interp, blend, F, mode, _bv(c))
        for n in range(4):  # the case cannot pass on an empty overlap
            assert (count == n).sum() >= 40, (n, int((count == n).sum()))
        assert (count[:, 256:] > 0).any()


# ---- 2. OVER against the device's own one-call-per-camera route ----

@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_over_equals_the_sequence_of_transparent_warps(W, dtype, interp):
    srcs, Ms = _scene(dtype)
    ts = [torch.from_numpy(s).cuda() for s in srcs]
    results = []
    for order in ((0, 1, 2), (2, 1, 0)):
        canvas = torch.full((DSIZE[1], DSIZE[0], 3), 77, dtype=ts[0].dtype, device="cuda")
        for k in order:
            W.warp_perspective(ts[k], Ms[k], DSIZE, flags=interp | INVERSE, out=canvas, border_mode=W.BORDER_TRANSPARENT)
        one = torch.full_like(canvas, 77)
        W.warp_stitch([ts[k] for k in order], [Ms[k] for k in order], DSIZE, flags=interp | INVERSE, blend="over", out=one, border_mode=W.BORDER_TRANSPARENT)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(one.cpu().numpy(), canvas.cpu().numpy())
        exp, _ = ref([srcs[k] for k in order], [Ms[k] for k in order], DSIZE, interp, "over", 64, BR.TRANSPARENT)
        np.testing.assert_array_equal(one.cpu().numpy(), exp)
        results.append(exp)
    assert not np.array_equal(results[0], results[1])  # the reversed list is a different, equally correct canvas


# ---- 3. layouts ----

def _jitter(M, i):
    return M + np.array([[0.01 * i, 0, 1.5 * i], [0, -0.02 * i, 0.75 * i], [0, 0, 0]])


@pytest.mark.parametrize("dtype,c", [(np.uint8, 3), (np.float32, 4)])
@pytest.mark.parametrize("blend,F", [("over", 64), ("feather", 3)])
def test_batch_strides_and_destinations(W, dtype, c, blend, F):
    """A batch of 2; camera 1 with a matrix per frame, the others shared; every source a window of a larger tensor whose row and frame
    strides all differ; an 8-bit RGB destination at an odd address between two guard bytes (every pixel stored on its own), and an aligned
    float32 4-channel destination (the wide stores)."""
    B, (dw, dh) = 2, DSIZE
    host = [_src((B, h, w, c), dtype, seed=50 + k) for k, (w, h, _) in enumerate(SCENE)]
    srcs = [PX.strided(s, (37 + 8 * k, 3 + k)) for k, s in enumerate(host)]
    strides = [t.stride(i) for t in srcs for i in (0, 1)]
    assert len(set(strides)) == 6 and all(t.stride(1) != t.shape[2] * c and t.stride(0) != t.shape[1] * t.stride(1) for t in srcs)
    Ms = [SCENE[0][2], np.stack([_jitter(SCENE[1][2], i) for i in range(B)]), SCENE[2][2]]
    n = B * dh * dw * c
    if dtype == np.uint8:
        buf = torch.full((n + 2,), 77, dtype=torch.uint8, device="cuda")
        out = buf[1:n + 1].view(B, dh, dw, c)
        assert out.data_ptr() % 2 == 1
    else:
        buf = torch.full((n,), 77, dtype=torch.float32, device="cuda")
        out = buf.view(B, dh, dw, c)
        assert out.data_ptr() % 16 == 0 and (dw * c * 4) % 16 == 0
    for mode in MODES:
        out.fill_(77)
        got = W.warp_stitch(srcs, Ms, DSIZE, flags=LINEAR | INVERSE, blend=blend, feather=F, border_value=_bv(c), out=out, border_mode=mode)
        torch.cuda.synchronize()
        assert got is out and (dtype != np.uint8 or (buf[0].item() == 77 and buf[-1].item() == 77))
        frames = []
        for b in range(B):
            exp, count = ref([s[b] for s in host], [M if M.ndim == 2 else M[b] for M in Ms], DSIZE, LINEAR, blend, F, mode, _bv(c))
            np.testing.assert_array_equal(out[b].cpu().numpy(), exp, err_msg="frame %d mode %d" % (b, mode))
            assert (count >= 2).sum() >= 40
            frames.append(exp)
        assert not np.array_equal(frames[0], frames[1])  # (frames and matrices differ)


# ---- 4. camera counts ----

@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_one_camera_and_eight(W, dtype, interp):
    w, h, M = SCENE[0]
    s = _src((h, w, 3), dtype, seed=60)
    canvas = np.full((DSIZE[1], DSIZE[0], 3), 77, dtype)
    for blend, F in BLENDS:
        got = gpu(W, [s], [M], DSIZE, interp, blend, F, BR.TRANSPARENT)
        np.testing.assert_array_equal(got, BR.warp(s, M, DSIZE, interp, BR.TRANSPARENT, m_is_inverse=True, canvas=canvas))
    # eight cameras over a common area: the scene's first map, shifted and sheared a little per camera
    sizes = [(40, 24), (33, 29), (64, 18), (25, 25), (47, 21), (31, 33), (52, 20), (38, 27)]
    srcs = [_src((hh, ww, 3), dtype, seed=61 + k) for k, (ww, hh) in enumerate(sizes)]
    Ms = [M + np.array([[0.01 * k, 0.005 * k, -1.5 * k], [0, 0.03 * k, -0.5 * k], [0, 0, 0]]) for k in range(8)]
    for blend, F in BLENDS:
        for mode in MODES:
            count = check(W, srcs, Ms, DSIZE, interp, blend, F, mode, _bv(3))
    assert (count == 8).sum() >= 40 and (count == 0).sum() >= 40 and len(np.unique(count)) >= 6


# ---- 5. the largest weights and sums ----

@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_large_weights(W, dtype):
    """Two 8192 x 8192 sources, the canvas across their centres, F = 4096: w_k reaches 4096 in both at once (W = 8192), and where both
    sources are 255 the 8-bit sum is 255 * 8192 + 4096, the largest the definition admits for two cameras."""
    n, (dw, dh) = 8192, (300, 8)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    srcs = []
    for k in range(2):
        t = torch.randint(0, 256, (n, n), dtype=torch.uint8, device="cuda", generator=gen) if dtype == torch.uint8 else torch.rand((n, n), device="cuda", generator=gen)
        if dtype == torch.uint8:
            t[4090:4100, 4090:4100] = 255
        srcs.append(t)
    Ms = [np.array([[1.0, 0, 3946], [0, 1.0, 4092], [0, 0, 1]]), np.array([[0.9, 0.05, 3960.3], [0.02, 1.05, 4089.5], [0, 0, 1]])]
    host = [t.cpu().numpy() for t in srcs]
    for interp in (NEAREST, LINEAR):
        cams = SR.cameras(host, Ms, (dw, dh), interp, 4096)
        assert (cams[0][2] + cams[1][2]).max() == 8192 and all(cover.all() for cover, _, _ in cams)
        out = torch.full((dh, dw), 77, dtype=dtype, device="cuda")
        W.warp_stitch(srcs, Ms, (dw, dh), flags=interp | INVERSE, blend="feather", feather=4096, out=out)
        torch.cuda.synchronize()
        exp, _ = SR.stitch(host, Ms, (dw, dh), interp, SR.FEATHER, 4096)
        np.testing.assert_array_equal(out.cpu().numpy(), exp)
        if dtype == torch.uint8:
            assert exp[3, 150] == 255


# ---- 6. edge arithmetic ----

@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_edge_arithmetic(W, interp):
    for dtype in (np.uint8, np.float32):
        a, b = _src((90, 120, 3), dtype, seed=70), _src((23, 37, 3), dtype, seed=71)
        horizon = np.array([[1.3, 0.2, -30.0], [0.1, 1.1, -20.0], [0.0, 0.02, -0.5]])  # W changes sign at row 25 of the canvas
        plain = np.array([[0.4, 0.05, -3.0], [0.02, 0.5, -2.0], [0.0002, 0, 1.0]])
        zero = np.zeros((3, 3))  # covers every pixel with source pixel (0, 0), as TRANSPARENT does
        far = np.array([[900.0, 0.0, -20000.0], [0.0, -700.0, 9000.0], [0, 0, 1.0]])  # crosses +-32768 inside the canvas
        beyond = np.array([[3.0, 0.5, 40000.0], [-0.25, 2.0, -50000.0], [0, 0, 1.0]])
        nan = np.array([[0.0, 0, 0], [0, 0.0, 0], [0, 0, 5e-324]])  # 32 / W overflows, 0 * inf is NaN -> INT_MAX: outside every source
        for blend, F in (("over", 64), ("feather", 3)):
            for mode in MODES:
                count = check(W, [a, b], [horizon, plain], (96, 50), interp, blend, F, mode, _bv(3))
                assert (count == 2).any() and (count == 0).any()
                count = check(W, [b, a, b], [plain, zero, plain], (96, 50), interp, blend, F, mode)
                assert count.min() >= 1 and (count == 3).any()
                count = check(W, [b, a, b], [far, plain, beyond], (96, 50), interp, blend, F, mode)
                count = check(W, [a, b], [nan, plain], (96, 50), interp, blend, F, mode)
                assert count.max() == 1
                count = check(W, [a], [nan], (40, 6), interp, blend, F, mode, _bv(3))
                assert count.max() == 0


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_tiny_sources(W, dtype, interp):
    """1 x 1, 1 x 9, 9 x 1 and 2 x 2 sources: under bilinear the first three cover nothing (no pixel has a right and a lower neighbour)."""
    Minv = np.array([[0.37, -0.21, -3.0], [0.18, 0.41, -2.5], [0.0005, 0.0, 1.0]])
    srcs = [_src((sh, sw, 3), dtype, seed=sh * 10 + sw) for sh, sw in ((1, 1), (1, 9), (9, 1), (2, 2))]
    for blend, F in (("over", 64), ("feather", 1), ("feather", 2)):
        for mode in MODES:
            count = check(W, srcs, [Minv] * 4, (29, 21), interp, blend, F, mode, _bv(3))
            if interp == LINEAR:
                for s in srcs[:3]:
                    assert check(W, [s], [Minv], (29, 21), interp, blend, F, mode).max() == 0
                assert count.max() == 1
            else:
                assert count.max() == 4


# ---- 7. float32: a single cover stores the camera's own pixel ----

@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_float32_single_cover_is_the_transparent_warp(W, interp):
    srcs, Ms = _scene(np.float32)
    srcs = [s * np.float32(1e37) for s in srcs]  # ((w p) / w gives p back neither where w p overflows -- here, from w = 34 on -- nor, in general, where it rounds)
    for F in (3, 64):
        got = gpu(W, srcs, Ms, DSIZE, interp, "feather", F, BR.TRANSPARENT)
        _, count = ref(srcs, Ms, DSIZE, interp, "feather", F, BR.TRANSPARENT)
        for s, (w, h, M) in zip(srcs, SCENE):
            mine = BR.written_mask((h, w), M, DSIZE, interp, m_is_inverse=True) & (count == 1)
            assert mine.sum() >= 40
            alone = torch.full((DSIZE[1], DSIZE[0], 3), 77, dtype=torch.float32, device="cuda")
            W.warp_perspective(torch.from_numpy(s).cuda(), M, DSIZE, flags=interp | INVERSE, out=alone, border_mode=W.BORDER_TRANSPARENT)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(got[mine], alone.cpu().numpy()[mine])
            np.testing.assert_array_equal(got[mine], BR.warp(s, M, DSIZE, interp, BR.TRANSPARENT, m_is_inverse=True)[mine])
        assert (got[count == 0] == 77).all()
