"""The supersampled warp on the GPU (bev_amd.warp.warp_perspective_supersampled -> bevwarp_warp_border | BEVWARP_SUPERSAMPLE_*): every
result compared with the numpy reference tests/supersample_ref.py -- tests/border_ref.warp on the k times finer grid, then the box reduce --
by bits on every element (float32: NaNs as NaNs).  Context-sized shapes: 40 x 24 sources, 36 x 20 destinations, two frames.
Run on the GPU box:  python -m pytest tests -m gpu -q"""
import functools

import numpy as np
import pytest
import torch

from tests import border_ref as BR
from tests import launch_contexts as LC
from tests import pixels as PX
from tests import supersample_ref as SS
from tests import workloads as wl

pytestmark = pytest.mark.gpu

NEAREST, LINEAR, INVERSE = 0, 1, 16
SW, SH, DW, DH = 40, 24, 36, 20
DSIZE = (DW, DH)
# dst px -> src px, minifying 4x with a perspective term: the destination covers about 140 x 80 source pixels around the 40 x 24 frame
MINIFY = np.array([[4.0, 0.3, -30.0], [-0.2, 4.1, -20.0], [0.002, 0.004, 1.0]])
MINIFY2 = np.stack([MINIFY, np.array([[3.8, -0.25, -41.0], [0.15, 4.2, -27.0], [-0.001, 0.003, 1.0]])])
BORDER = (9.0, 200.0, 31.0, 77.0)


@pytest.fixture(scope="module")
def W():
    from bev_amd import warp
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return warp


@functools.lru_cache(maxsize=None)
def frames(dtype, c, n=2, seed=0):
    """(n, SH, SW, c) frames, read-only and shared by the tests."""
    rng = np.random.default_rng(1000 * seed + 10 * c + (dtype == np.uint8))
    shape = (n, SH, SW, c)
    a = rng.integers(0, 256, shape, dtype=np.uint8) if dtype == np.uint8 else (rng.random(shape, dtype=np.float32) * 255 - 64).astype(np.float32)
    a.setflags(write=False)
    return a


def expected(host, Ms, dsize, k, interp, mode, border=0.0):
    """The reference, frame by frame; Ms: one inverse matrix for all frames or one per frame."""
    Ms = np.asarray(Ms, np.float64).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):  # (the float32 domain: the reference computes 0 * Inf on purpose)
        return np.stack([SS.warp(f, Ms[i if len(Ms) > 1 else 0], dsize, k, interp, mode, m_is_inverse=True, border_value=border) for i, f in enumerate(host)])


def fused(W, src, Ms, dsize, k, interp, mode, border=None, canvas=77):
    """One call on a destination filled with `canvas` (a pixel the launch leaves unwritten does not pass as a zero)."""
    t = src if isinstance(src, torch.Tensor) else torch.from_numpy(np.array(src)).cuda()
    out = torch.full(t.shape[:-3] + (int(dsize[1]), int(dsize[0]), t.shape[-1]), canvas, dtype=t.dtype, device=t.device)
    got = W.warp_perspective_supersampled(t, Ms, dsize, supersample=k, flags=interp | INVERSE, border_value=border, out=out, border_mode=mode)
    torch.cuda.synchronize()
    assert got is out
    return got.cpu().numpy()


def check(W, host, Ms, dsize, k, interp, mode, border=None, src=None, what=""):
    got = fused(W, host if src is None else src, Ms, dsize, k, interp, mode, border)
    exp = expected(host, Ms, dsize, k, interp, mode, 0.0 if border is None else border)
    SS.assert_same(got, exp, err_msg="%s k=%d interp=%d %s %s %s" % (what, k, interp, BR.NAMES[mode], host.dtype, host.shape))
    return got, exp


@pytest.mark.parametrize("k", SS.FACTORS)
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_format_matrix(W, dtype, interp, k):
    """Every channel count and border, two frames with a matrix each; part of the destination lies outside the frame."""
    for c in (1, 2, 3, 4):
        for mode in SS.MODES:
            border = BORDER[:c] if mode == BR.CONSTANT else None
            got, exp = check(W, frames(dtype, c), MINIFY2, DSIZE, k, interp, mode, border)
            assert not np.array_equal(exp[0], exp[1])
    plain = np.stack([BR.warp(f, MINIFY2[i], DSIZE, interp, BR.REFLECT, m_is_inverse=True) for i, f in enumerate(frames(dtype, 3))])
    exp = expected(frames(dtype, 3), MINIFY2, DSIZE, k, interp, BR.REFLECT)
    assert (plain != exp).mean() > 0.5  # (the supersampled image is another image than the plain warp's)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_shared_matrix_and_strided_batch_of_three(W, dtype):
    """One matrix for all frames, and three frames that are windows of one larger allocation (row and frame strides of their own)."""
    host = frames(dtype, 3, n=3, seed=1)
    for k in (2, 4):
        check(W, host[:2], MINIFY, DSIZE, k, LINEAR, BR.WRAP, what="shared")
        check(W, host[:2], MINIFY[None], DSIZE, k, NEAREST, BR.CONSTANT, border=BORDER[:3], what="shared (1, 3, 3)")
        src = PX.padded_source(np.array(host), 0xA5 if dtype == np.uint8 else -7.0, offset=0, pad_rows=3)
        assert src.stride(0) != SH * src.stride(1) and src.stride(1) != SW * 3
        Ms = np.stack([MINIFY2[0], MINIFY2[1], MINIFY])
        check(W, host, Ms, DSIZE, k, LINEAR, BR.REFLECT_101, src=src, what="strided batch, per-frame")
        check(W, host, MINIFY, DSIZE, k, LINEAR, BR.REPLICATE, src=src, what="strided batch, shared")


@pytest.mark.parametrize("k", (2, 4))
def test_destination_widths(W, k):
    """Rows that end inside a lane's 4 pixels, at a wave's end and at a tile's end (256); height 5 is two tile rows."""
    for dw in (1, 3, 4, 5, 63, 64, 65, 255, 256, 257):
        M = np.array([[160.0 / dw, 0.3, -30.0], [-0.2, 16.0, -20.0], [0.002 * 36 / dw, 0.004, 1.0]])
        check(W, frames(np.uint8, 3), M, (dw, 5), k, LINEAR, BR.REFLECT_101, what="width %d" % dw)
        check(W, frames(np.float32, 1), M, (dw, 5), k, LINEAR, BR.CONSTANT, border=(5.5,), what="width %d" % dw)


@pytest.mark.parametrize("shape", [((50, 7), 2), ((30, 3), 4), ((70, 1), 2), ((70, 1), 4), ((70, 1), 8)], ids=str)
def test_sub_columns_straddle_evaluation_blocks(W, shape):
    """Fine grids whose evaluation block width is no multiple of k (73 and 85: tests/test_supersample_cpu.py): a pixel's sub-columns lie in
    two blocks, whose row terms differ in the last bits -- a perspective matrix with awkward entries shows a wrong block origin."""
    (dw, dh), k = shape
    M = np.array([[1.7 * 36 / dw, 0.31, -11.3], [-0.23, 1.9 * 20 / dh, -7.7], [0.0031 * 36 / dw, 0.0047, 1.0]])
    for dtype in (np.uint8, np.float32):
        for interp in (NEAREST, LINEAR):
            check(W, frames(dtype, 3), M, (dw, dh), k, interp, BR.REPLICATE, what="straddle")
            check(W, frames(dtype, 2), M, (dw, dh), k, interp, BR.CONSTANT, border=BORDER[:2], what="straddle")


@pytest.mark.parametrize("dtype,c", [(np.uint8, 1), (np.uint8, 2), (np.uint8, 3), (np.uint8, 4), (np.float32, 1), (np.float32, 3)])
def test_destination_views_and_canaries(W, dtype, c):
    """Aligned (wide stores), unaligned (every pixel on its own) and row-padded destinations of two frames inside a holder of canary bytes:
    the pixels are the reference's and no byte beside the rows or between the frames is written."""
    host = frames(dtype, c)
    for k, mode, dsize in ((2, BR.REFLECT, DSIZE), (4, BR.CONSTANT, (37, 6))):
        border = BORDER[:c] if mode == BR.CONSTANT else None
        exp = expected(host, MINIFY2, dsize, k, LINEAR, mode, 0.0 if border is None else border)
        src = torch.from_numpy(np.array(host)).cuda()
        for align, pad in ((16, 0), (16, 48), (0, 0), (0, 5)):
            view, holder = PX.canaried_out((2, dsize[1], dsize[0], c), dtype, pad, align=align)
            got = W.warp_perspective_supersampled(src, MINIFY2, dsize, supersample=k, flags=LINEAR | INVERSE, border_value=border, out=view, border_mode=mode)
            torch.cuda.synchronize()
            assert got is view
            SS.assert_same(view.cpu().numpy(), exp, err_msg="align %d pad %d k %d" % (align, pad, k))
            PX.assert_canaries_intact(holder, view, "align %d pad %d k %d" % (align, pad, k))


@pytest.mark.parametrize("dtype,c", [(np.uint8, 2), (np.uint8, 3), (np.uint8, 4), (np.float32, 3)])
def test_unaligned_source_view(W, dtype, c):
    """Source views at every residue of the base address: the whole-pixel loads of 2 and 4 channels need their alignment."""
    host = frames(dtype, c)
    for offset in ((1, 2, 3) if dtype == np.uint8 else (1, 3)):
        src = PX.padded_source(np.array(host), 0xA5 if dtype == np.uint8 else -7.0, offset=offset)
        for k, interp, mode in ((2, LINEAR, BR.WRAP), (4, NEAREST, BR.CONSTANT)):
            check(W, host, MINIFY2, DSIZE, k, interp, mode, border=BORDER[:c] if mode == BR.CONSTANT else None, src=src, what="offset %d" % offset)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_constant_border_value_and_wholly_outside(W, dtype, interp):
    """A non-zero border value blends into the pixels whose taps leave the frame; a destination wholly outside the source is the border
    value itself.  (float32: -2.5, 7.0 and the denormal 1e-40 -- values whose k^2-fold sums are exact, so that "itself" holds by bits.)"""
    host = frames(dtype, 3)
    border = (9.0, 200.0, 31.0) if dtype == np.uint8 else (-2.5, 7.0, 1e-40)
    far = MINIFY.copy()
    far[0, 2] += 3000.0
    for k in SS.FACTORS:
        got, exp = check(W, host, MINIFY2, DSIZE, k, interp, BR.CONSTANT, border=border)
        # (some pixels are the border value itself, and the value shows: a border of 0 gives another image)
        assert (exp == np.asarray(border, dtype)).all(axis=-1).any() and (exp != expected(host, MINIFY2, DSIZE, k, interp, BR.CONSTANT)).any()
        got, _ = check(W, host, far, DSIZE, k, interp, BR.CONSTANT, border=border, what="wholly outside")
        assert (PX.bits(got) == PX.bits(np.asarray(border, np.float32))).all() if dtype == np.float32 else (got == np.asarray(border, np.uint8)).all()


@pytest.mark.parametrize("kind", PX.KINDS + ("zeros",))
def test_float32_domain(W, kind):
    """Sources over the whole float32 format (tests/pixels.py): both signs, every binade, denormals, signed zeros, +-inf, NaNs, +-FLT_MAX."""
    host = np.stack([PX.zero_block_frame(40 + i, SH, SW, 3) if kind == "zeros" else PX.float_frame(kind, 40 + i, SH, SW, 3) for i in range(2)])
    M = np.stack([np.array([[1.1, 0.05, -2.0], [-0.04, 1.2, -1.5], [0.0005, 0.001, 1.0]]), MINIFY])  # (frame 0: taps mostly inside, zero squares kept whole)
    seen = set()
    for k in (2, 4):
        for interp in (NEAREST, LINEAR):
            for mode, border in ((BR.REFLECT, None), (BR.CONSTANT, PX.BORDER[:3])):
                got = fused(W, host, M, DSIZE, k, interp, mode, border)
                exp = expected(host, M, DSIZE, k, interp, mode, 0.0 if border is None else border)
                PX.same_float(got, exp)
                seen |= {name for name, there in (("-0", (PX.bits(exp) == 0x80000000).any()), ("nan", np.isnan(exp).any()), ("inf", np.isinf(exp).any()),
                                                  ("subnormal", PX.is_subnormal(exp).any())) if there}
    # what each kind is for is in the expected results (sums of -0 alone stay -0: an accumulator that started from +0 would show)
    assert {"mixed": {"nan", "inf"}, "tiny": {"subnormal"}, "huge": {"inf"}, "zeros": {"-0"}}[kind] <= seen


@pytest.mark.parametrize("k,y0,m22", [(2, 7, -3.25), (4, 13, -2.875), (8, 27, -2.9375)])
def test_w_zero_and_horizon_inside_destination(W, k, y0, m22):
    """W = F[2][1] y' + F[2][2] is exactly 0 on fine row y0 (the division is skipped: the coordinate is 0) and changes sign there."""
    M = np.array([[1.3, 0.2, -3.0], [0.1, 1.1, -2.0], [0.0, 1.0, m22]])
    F = SS.fine_matrix(M, k)
    assert F[2, 0] == 0 and F[2, 1] * y0 + F[2, 2] == 0 and 0 < y0 < k * DH
    for dtype in (np.uint8, np.float32):
        for interp in (NEAREST, LINEAR):
            for mode in (BR.CONSTANT, BR.REPLICATE, BR.WRAP):
                check(W, frames(dtype, 3), M, DSIZE, k, interp, mode, what="W == 0")
    for mode in SS.MODES:
        check(W, frames(np.uint8, 3), PX.HORIZON, DSIZE, k, LINEAR, mode, what="horizon")


@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_saturating_coordinates(W, interp):
    """Source coordinates past +-32768 saturate to int16 before the border's index remap; a NaN coordinate is INT_MAX."""
    host = frames(np.uint8, 3)
    fhost = frames(np.float32, 3)
    for M in (np.array([[3.0, 0.5, 40000.0], [-0.25, 2.0, -50000.0], [0, 0, 1.0]]), np.array([[900.0, 0.0, -20000.0], [0.0, -700.0, 9000.0], [0, 0, 1.0]]),
              np.array([[0.0, 0, 0], [0, 0.0, 0], [0, 0, 5e-324]])):
        for k in (2, 8):
            for mode in SS.MODES:
                check(W, host, M, DSIZE, k, interp, mode, what="saturating")
            check(W, fhost, M, DSIZE, k, interp, BR.WRAP, what="saturating")


def test_supersample_one_is_warp_perspective(W):
    for dtype in (np.uint8, np.float32):
        t = torch.from_numpy(np.array(frames(dtype, 3))).cuda()
        for mode in (W.BORDER_CONSTANT, W.BORDER_REFLECT, W.BORDER_TRANSPARENT):
            a = W.warp_perspective_supersampled(t, MINIFY2, DSIZE, supersample=1, flags=LINEAR | INVERSE, border_value=(1, 2, 3), border_mode=mode)
            b = W.warp_perspective(t, MINIFY2, DSIZE, flags=LINEAR | INVERSE, border_value=(1, 2, 3), border_mode=mode)
            torch.cuda.synchronize()
            assert torch.equal(a, b)
        a = W.warp_perspective_supersampled(t, MINIFY2, DSIZE, supersample=1, flags=W.INTER_CUBIC | INVERSE)  # (k = 1 keeps bicubic)
        assert torch.equal(a, W.warp_perspective(t, MINIFY2, DSIZE, flags=W.INTER_CUBIC | INVERSE))


def _two_pass(W, t, Ms, dsize, k, interp, mode, border):
    """The route the fused entry replaces: warp_perspective into k dsize with the fine matrices, then the box reduce in torch."""
    F = np.stack([SS.fine_matrix(M, k) for M in np.asarray(Ms).reshape(-1, 3, 3)])
    fine = W.warp_perspective(t, F, (k * dsize[0], k * dsize[1]), flags=interp | INVERSE, border_value=border, border_mode=mode)
    B, _, _, C = fine.shape
    cells = fine.view(B, dsize[1], k, dsize[0], k, C)
    if fine.dtype == torch.uint8:
        return ((cells.to(torch.int32).sum(dim=(2, 4)) + (k * k) // 2) >> (2 * int(np.log2(k)))).to(torch.uint8)
    acc = None
    for j in range(k):
        for i in range(k):
            s = cells[:, :, j, :, i]
            acc = s.clone() if acc is None else acc + s
    return acc * (1.0 / (k * k))


@pytest.mark.parametrize("k", SS.FACTORS)
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_fused_equals_the_two_pass_route(W, dtype, k):
    """Every border, both interpolations -- CONSTANT's fine frame comes from bevwarp_warp's own kernel, the others' from the border kernel."""
    t = torch.from_numpy(np.array(frames(dtype, 3))).cuda()
    for interp in (NEAREST, LINEAR):
        for mode in SS.MODES:
            border = BORDER[:3] if mode == BR.CONSTANT else None
            a = W.warp_perspective_supersampled(t, MINIFY2, DSIZE, supersample=k, flags=interp | INVERSE, border_value=border, border_mode=mode)
            b = _two_pass(W, t, MINIFY2, DSIZE, k, interp, mode, border)
            torch.cuda.synchronize()
            SS.assert_same(a.cpu().numpy(), b.cpu().numpy(), err_msg="%s interp %d" % (BR.NAMES[mode], interp))


def test_out_and_matrix_tensor_given(W):
    """`out=` is returned, `M_inv_device=` is read as it is (M is not looked at), (H, W) and (H, W, C) sources keep their shape."""
    host = frames(np.uint8, 3)
    t = torch.from_numpy(np.array(host)).cuda()
    minv = torch.from_numpy(MINIFY2.copy()).cuda()
    out = torch.full((2, DH, DW, 3), 77, dtype=torch.uint8, device="cuda")
    got = W.warp_perspective_supersampled(t, None, DSIZE, supersample=4, out=out, M_inv_device=minv, border_mode=W.BORDER_REPLICATE)
    torch.cuda.synchronize()
    assert got is out
    np.testing.assert_array_equal(out.cpu().numpy(), expected(host, MINIFY2, DSIZE, 4, LINEAR, BR.REPLICATE))
    one = W.warp_perspective_supersampled(t[0], None, DSIZE, supersample=2, M_inv_device=minv[:1], border_mode=W.BORDER_WRAP)
    gray = W.warp_perspective_supersampled(t[1, :, :, 0], MINIFY, DSIZE, supersample=2, flags=NEAREST | INVERSE)
    fwd = W.warp_perspective_supersampled(t[0], np.linalg.inv(MINIFY), DSIZE, supersample=2, border_mode=W.BORDER_WRAP)  # (a forward matrix is inverted on the host)
    torch.cuda.synchronize()
    assert one.shape == (DH, DW, 3) and gray.shape == (DH, DW) and fwd.shape == (DH, DW, 3)
    np.testing.assert_array_equal(one.cpu().numpy(), expected(host[:1], MINIFY, DSIZE, 2, LINEAR, BR.WRAP)[0])
    np.testing.assert_array_equal(gray.cpu().numpy(), expected(host[1:, :, :, :1], MINIFY, DSIZE, 2, NEAREST, BR.CONSTANT)[0, :, :, 0])
    Minv = np.asarray(W.invert_homography(np.linalg.inv(MINIFY)))
    np.testing.assert_array_equal(fwd.cpu().numpy(), expected(host[:1], Minv, DSIZE, 2, LINEAR, BR.WRAP)[0])
    for bad in (torch.empty((2, DH, DW, 3), dtype=torch.float32, device="cuda"), torch.empty((2, DH, DW + 1, 3), dtype=torch.uint8, device="cuda")):
        with pytest.raises(ValueError):
            W.warp_perspective_supersampled(t, MINIFY2, DSIZE, supersample=2, out=bad)


# ---- launch contexts, in the manner of tests/launch_contexts.py: a case of its table's kind, driven through its checks -----------------

def _context_case(k, mode):
    def frames_of(which):
        return (LC.frames(which)[0],)

    return LC.Case(
        "warp_perspective_supersampled-k%d-%s" % (k, BR.NAMES[mode]), "bevwarp_warp_border", frames_of, lambda which: dict(M=LC.MINVS["A"], border=np.array(LC.BORDER)),
        LC.no_maps, LC.PX,
        lambda t, r, h, o: [W_module().warp_perspective_supersampled(t[0], h["M"], LC.DSIZE, supersample=k, flags=LC.FLAGS, border_value=h["border"], out=o[0],
                                                                     border_mode=mode)],
        lambda which, hw: [expected(LC.frames(which)[0], LC.MINVS["A"], LC.DSIZE, k, LINEAR, mode, LC.BORDER)], sliceable=(0,))


def W_module():
    from bev_amd import warp
    return warp


CONTEXT_CASES = [_context_case(2, BR.CONSTANT), _context_case(4, BR.REFLECT_101)]


@pytest.fixture(scope="module")
def delay():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    cycles, ms = LC.sleep_cycles_for(50.0)
    assert ms >= 20.0, "the delay came out at %.2f ms: too short to enqueue a call behind" % ms
    return cycles


@pytest.mark.parametrize("case", CONTEXT_CASES, ids=repr)
def test_side_stream_behind_a_delay(case, delay):
    """On a fresh stream behind a delay, set B copied over set A and the destination poisoned in stream order."""
    LC.check_side_stream(case, LC.Gpu("cuda:0", delay))


@pytest.mark.parametrize("case", CONTEXT_CASES, ids=repr)
@pytest.mark.parametrize("sliced", [False, True], ids=["frames", "channel_slices"])
def test_capture_and_replay(case, sliced):
    """Captured into a graph, the caller's host arrays overwritten with NaNs, replayed on set B and on set A."""
    LC.check_replays(case, LC.Gpu("cuda:0"), sliced=sliced)
