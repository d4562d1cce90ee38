"""The lens warp, the map sampler and the multi-camera warp on the whole float32 domain (bevwarp_warp_lens, bevwarp_remap,
bevwarp_warp_stitch; DESIGN.md section 1's float32 contract).  Their own GPU modules feed them frames in [0, 1) -- positive, normal, one
binade -- and compare with assert_array_equal, under which -0.0 is +0.0: a flush to zero, a quieted or dropped NaN, a skipped zero-weight
tap, another summation order, an accumulator that does not start from +0, a nearest path that goes through arithmetic -- none of them
shows there (tests/test_float_domain_cpu.py's docstring has the table).  Here the same geometries run on tests/pixels.py's frames of
both signs and every binade with subnormals, signed zeros, +-Inf, quiet and signalling NaNs and +-FLT_MAX, and on frames with squares of
-0.0 and +0.0 (zero_block_frame), and every result is compared BY BITS with the family's numpy reference (tests/float_domain.py: the
cases, `compare`, and the preconditions that keep a case from passing vacuously):

    what the definition computes (a bilinear blend, a FEATHER mean)     same_float(payload=False): a NaN of any payload where the
                                                                        reference has one, identical bits everywhere else
    what it copies (nearest, border fills, OVER and single covers       same_float(payload=True): all 32 bits
    under nearest, everything BORDER_TRANSPARENT leaves alone)

Destinations are pre-filled with a signalling NaN (float_domain.CANVAS_BITS), so a pixel a launch must not write is known by its bits.
Run on the GPU box:  python -m pytest tests -m gpu -q"""

import numpy as np
import pytest
import torch

from tests import float_domain as FD
from tests import hostplan
from tests import lens_ref as LR
from tests import pixels as PX
from tests import remap_ref as RR

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]  # (numpy's: the references compute 0 * Inf on purpose)

NEAREST, LINEAR, INVERSE = FD.NEAREST, FD.LINEAR, 16
BY_KIND = [(kind, interp) for interp in (NEAREST, LINEAR) for kind in FD.kinds(interp)]
KIND_IDS = ["%s-%s" % (kind, ("nearest", "linear")[interp]) for kind, interp in BY_KIND]


@pytest.fixture(scope="module")
def W():
    from bev_amd import warp
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return warp


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def canvas(shape):
    """A destination whose every element is the signalling NaN CANVAS_BITS."""
    return torch.full(tuple(shape), FD.CANVAS_BITS - (1 << 32), dtype=torch.int32, device="cuda").view(torch.float32)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---- 1. the lens warp ----

def _lens_call(W, src, setup, interp, mode, bv, inverse=False):
    _, _, dw, dh, M, K, dist = setup[:7]
    out = canvas((dh, dw) + src.shape[2:])
    got = W.warp_perspective_lens(cuda(src), M, (dw, dh), K, dist, flags=interp | (INVERSE if inverse else 0), border_value=bv, out=out, border_mode=mode)
    assert got is out
    return host(out)


@pytest.mark.parametrize("kind,interp", BY_KIND, ids=KIND_IDS)
@pytest.mark.parametrize("setup", FD.LENS_SETUPS, ids=["-".join(s) for s in FD.LENS_SETUPS])
def test_lens(W, setup, kind, interp):
    """Both borders x 1-4 channels and an (H, W) image; the constant border's last value is subnormal."""
    st = FD.lens_setup(*setup)
    for cid, src, mode, bv in FD.lens_cases(setup[0], setup[1], kind, interp):
        exp, computed, kept, _ = FD.lens_expected(src, st, interp, mode, 0.0 if bv is None else bv)
        FD.preconditions(kind, interp, exp, computed, kept, what=cid)
        FD.compare(_lens_call(W, src, st, interp, mode, bv), exp, computed, cid)


@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_lens_tiny_sources(W, interp):
    """2 x 2 and 5 x 1 sources (under bilinear the second has no inlier: BORDER_TRANSPARENT writes nothing)."""
    for sh, sw in FD.TINY_SOURCES:
        st = FD.tiny_lens_setup(sh, sw)
        for cid, src, mode, bv in FD.tiny_lens_cases(sh, sw, interp):
            exp, computed, _, _ = FD.lens_expected(src, st, interp, mode, 0.0 if bv is None else bv)
            FD.compare(_lens_call(W, src, st, interp, mode, bv, inverse=True), exp, computed, cid)


@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_lens_border_value_with_a_nan_is_refused_and_nothing_is_written(W, interp):
    """include/bevwarp.h: a border value that is not finite is BEVWARP_ERR_NOT_FINITE.  A NaN with a payload in one channel: the call
    raises and the destination keeps its bits; under BORDER_TRANSPARENT, which reads no border value, the same call runs."""
    st = FD.lens_setup("rotated_zoom_out", "A")
    src = FD.frame("mixed", 1900, st[1], st[0], 3)
    bv = [0.3, float(np.uint32(0x7fc12345).view(np.float32)), 7.0]
    _, _, dw, dh, M, K, dist = st[:7]
    out = canvas((dh, dw, 3))
    with pytest.raises(ValueError, match="libbevwarp"):
        W.warp_perspective_lens(cuda(src), M, (dw, dh), K, dist, flags=interp, border_value=bv, out=out, border_mode=LR.CONSTANT)
    assert (PX.bits(host(out)) == FD.CANVAS_BITS).all()
    exp, computed, _, _ = FD.lens_expected(src, st, interp, LR.TRANSPARENT, 0.0)
    FD.compare(_lens_call(W, src, st, interp, LR.TRANSPARENT, bv), exp, computed)


# ---- 2. the map sampler ----

@pytest.fixture(scope="module")
def plan_driver():
    """tests/host_plan_driver.cpp, family `remap`, built plainly (tests/test_remap_cpu.py runs it under the sanitizers)."""
    return hostplan.build_driver(sanitize=False)


def _frames_per_item(plan_driver, B, sh, sw, dh, dw, c, interp, mode):
    """What bevwarp_remap's plan keeps per item for this call (tight float32 frames, one shared map).  The driver plans with up to 8
    frames per item, the library with fewer: both keep more than one under the same condition, the plan's first doubling."""
    line = "call 4096 %d %d %d %d %d %d %d %d %d %d %d %d %d 1 %d %d %d %d 1 %d %d" % (
        1 << 40, 1 << 44, 1 << 48, B, sh, sw, dh, dw, c, sh * sw * c * 4, sw * c * 4, dh * dw * c * 4, dw * c * 4, dh * dw * 4, dw * 4, dh * dw * 2, dw * 2, interp, mode)
    status, plan_status, fpi, _ = hostplan.run_driver(plan_driver, [line], "remap")[0]
    assert status == 0 and plan_status == 0, (line, status, plan_status)
    return fpi


def _same_on_device(got, exp, computed):
    """float_domain.compare's two rules for a batch, on the device: got (B, dh, dw, C) against exp (B, dh, dw, C), computed (dh, dw)."""
    gb, eb = got.view(torch.int32), exp.view(torch.int32)
    en = torch.isnan(exp)
    loose = (torch.isnan(got) != en) | (~en & (gb != eb))
    return not bool(torch.where(computed[None, :, :, None], loose, gb != eb).any())


def test_the_comparison_on_the_device_is_same_float():
    """-0.0 against +0.0, a subnormal against 0, a quiet against a signalling NaN, a NaN against a number: computed and copied."""
    u = lambda *v: np.array(v, np.uint32).view(np.float32).reshape(1, 1, -1, 1)  # noqa: E731
    exp = u(0x80000000, 0x00000001, FD.SNAN_BITS, 0x7fc00000, 0x3f800000)
    for got, loose, strict in ((exp, True, True), (u(0, 0x00000001, FD.SNAN_BITS, 0x7fc00000, 0x3f800000), False, False),
                               (u(0x80000000, 0, FD.SNAN_BITS, 0x7fc00000, 0x3f800000), False, False),
                               (u(0x80000000, 0x00000001, 0x7fc00000, 0xffc00001, 0x3f800000), True, False),
                               (u(0x80000000, 0x00000001, FD.SNAN_BITS, 0x3f800000, 0x3f800000), False, False),
                               (u(0x80000000, 0x00000001, FD.SNAN_BITS, 0x7fc00000, 0x7fc00000), False, False)):
        for computed, want in ((True, loose), (False, strict)):
            mask = np.full((1, 5), computed)
            assert _same_on_device(cuda(got), cuda(exp), cuda(mask)) == want, (PX.bits(got).ravel(), computed)
            host_says = True
            try:
                FD.compare(got[0], exp[0], mask)
            except AssertionError:
                host_says = False
            assert host_says == want


@pytest.mark.parametrize("c", [1, 2, 3, 4])
@pytest.mark.parametrize("kind,interp", BY_KIND, ids=KIND_IDS)
@pytest.mark.parametrize("setup", FD.REMAP_SETUPS, ids=["-".join(s) for s in FD.REMAP_SETUPS])
def test_remap(W, plan_driver, setup, kind, interp, c):
    """A map built on the device, all six borders: three frames one call each, then a batch that shares the map and is large enough for
    the plan to walk two frames per item with the entries and weights in registers (frame g is frame g % 3, the last group is short).
    Every frame of the batch is compared on the device, three of them on the host as well."""
    sw, sh, dw, dh, M, K, dist = FD.remap_setup(*setup)[:7]
    m = W.build_warp_map(M, (dw, dh), flags=interp, K=K, dist_coeff=dist)
    xy, frac = FD.ref_map(setup[0], setup[1], interp)
    np.testing.assert_array_equal(host(m.xy)[0], xy)
    if interp == LINEAR:
        np.testing.assert_array_equal(host(m.frac)[0].view(np.uint16), frac)
    B = FD.remap_batch(-(-dw // 256) * -(-dh // 4))
    pick = torch.arange(B, device="cuda") % FD.UNIQUE
    batch, cases = None, FD.remap_cases(setup[0], setup[1], kind, interp, (c,))
    assert [mode for _, _, mode, _ in cases] == list(RR.MODES)
    for cid, srcs, mode, bv in cases:
        exps = []
        for i, src in enumerate(srcs):
            exp, computed, kept, _ = FD.remap_expected(src, xy, frac, interp, mode, bv)
            FD.preconditions(kind, interp, exp, computed, kept, what="%s frame %d" % (cid, i))
            out = canvas((dh, dw, c))
            assert W.remap(cuda(src), m, border_mode=mode, border_value=bv, out=out) is out
            FD.compare(host(out), exp, computed, "%s frame %d alone" % (cid, i))
            exps.append(exp)
        assert _frames_per_item(plan_driver, B, sh, sw, dh, dw, c, interp, mode) > 1, (cid, B)
        batch = cuda(np.stack(srcs))[pick] if batch is None else batch  # (the borders share the frames)
        out = canvas((B, dh, dw, c))
        W.remap(batch, m, border_mode=mode, border_value=bv, out=out)
        torch.cuda.synchronize()
        for g in (0, 1, B - 1):
            FD.compare(out[g].cpu().numpy(), exps[g % FD.UNIQUE], computed, "%s frame %d of %d" % (cid, g, B))
        if not _same_on_device(out, cuda(np.stack(exps))[pick], cuda(computed)):
            for g in range(B):  # (the frame and the element, from the host's comparison)
                FD.compare(out[g].cpu().numpy(), exps[g % FD.UNIQUE], computed, "%s frame %d of %d" % (cid, g, B))
            raise AssertionError("%s: the device's comparison of the batch failed and the host's did not" % cid)


@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_remap_tiny_sources(W, interp):
    """2 x 2 and 5 x 1 sources under a map that reaches far outside them, all six borders."""
    xy, frac = FD.tiny_map(interp)
    m = W.build_warp_map(FD.TINY_MINV, FD.TINY_DSIZE, flags=interp | INVERSE)
    np.testing.assert_array_equal(host(m.xy)[0], xy)
    dw, dh = FD.TINY_DSIZE
    for sh, sw in FD.TINY_SOURCES:
        for cid, src, mode, bv in FD.tiny_remap_cases(sh, sw, interp):
            exp, computed, _, _ = FD.remap_expected(src, xy, frac, interp, mode, bv)
            out = canvas((dh, dw, 3))
            W.remap(cuda(src), m, border_mode=mode, border_value=bv, out=out)
            FD.compare(host(out), exp, computed, cid)


@pytest.mark.parametrize("kind,interp", BY_KIND, ids=KIND_IDS)
def test_remap_numpy_with_float_maps(W, kind, interp):
    """cv2_compat.remap / remap_numpy: float32 coordinate maps (lens B's chain on rotated_zoom_out) converted on the host, numpy in and
    out, the canvas of BORDER_TRANSPARENT given as `dst`."""
    from bev_amd import cv2_compat as cv2
    sw, sh, dw, dh, _, _, _, R, l12, _ = FD.lens_setup("rotated_zoom_out", "B")
    u, v, _ = LR.chain((dw, dh), R, l12)
    mapx, mapy = u.astype(np.float32), v.astype(np.float32)
    xy, frac = W.convert_maps(mapx, mapy, nearest=interp == NEAREST)  # (tests/test_remap_cpu.py holds it to the scalar restatement)
    src = FD.frame(kind, FD.seed(2800, kind, 3), sh, sw, 3)
    for mode in (RR.CONSTANT, RR.REFLECT_101, RR.TRANSPARENT):
        bv = FD.border(3) if mode == RR.CONSTANT else None
        exp, computed, kept, _ = FD.remap_expected(src, xy, frac, interp, mode, bv)
        FD.preconditions(kind, interp, exp, computed, kept, what="float maps %s mode %d" % (kind, mode))
        dst = FD.canvas((dh, dw, 3))
        got = cv2.remap(src, mapx, mapy, interp, dst=dst, borderMode=mode, borderValue=0 if bv is None else bv)
        assert got is dst
        FD.compare(got, exp, computed, "float maps %s mode %d" % (kind, mode))


# ---- 3. the multi-camera warp ----

@pytest.mark.parametrize("kind,interp", BY_KIND, ids=KIND_IDS)
def test_stitch(W, kind, interp):
    """OVER and FEATHER with F = 1, 3, 64 x both rules for uncovered pixels x 1-4 channels; pixels with 0, 1, 2 and 3 covering cameras
    all occur.  FEATHER's float32 arithmetic as the reference pins it: the sum starts from +0 (a mean of -0.0 pixels is +0.0), every
    product and sum rounds to float32 with subnormals kept, a sum that overflows gives +-Inf, one correctly rounded division."""
    scene, (dw, dh) = FD.stitch_scene()
    Ms = [M for _, _, M in scene]
    for cid, srcs, blend, F, mode, bv in FD.stitch_cases(kind, interp):
        exp, computed, kept, many, count = FD.stitch_expected(srcs, interp, blend, F, mode, bv)
        for n in range(4):  # the case cannot pass on an empty overlap
            assert (count == n).sum() >= 40, (cid, n, int((count == n).sum()))
        FD.preconditions(kind, interp, exp, computed, kept, many, F if blend == "feather" else 0, what=cid)
        out = canvas((dh, dw, srcs[0].shape[2]))
        got = W.warp_stitch([cuda(s) for s in srcs], Ms, (dw, dh), flags=interp | INVERSE, blend=blend, feather=F, border_value=bv, out=out, border_mode=mode)
        assert got is out
        FD.compare(host(out), exp, computed, cid)
