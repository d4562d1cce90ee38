"""The three CPU implementations of the warp (oracle/warp_oracle.c, its numpy twin oracle/warp_numpy.py, tests/border_ref.py in
CONSTANT mode) on float32 frames of the whole format (tests/pixels.py: float_frame), at the geometries that reach every tile class
of the warp kernel (tests/pixels.py: float_cases) -- so what a kernel is held to on such frames is agreed on by three separate
restatements: the NaN positions, and every bit of every
value that is not NaN (-0.0, subnormals and Inf included); for nearest neighbour every bit, NaN payloads too.  The payloads of NaNs
that bilinear COMPUTES differ between these implementations already (x86 propagates the first operand's payload, numpy's vector
loops another one), so they are not part of the contract.

Known answers fix the semantics, and non-vacuity floors make sure the frames do reach the special values in the results."""
import numpy as np
import pytest

from oracle import cpu_oracle as co
from oracle import warp_numpy as wn
from tests import border_ref as BR
from tests import pixels as PX

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")  # (numpy's: the references compute 0 * Inf and Inf - Inf on purpose)

CASES = PX.float_cases()
STATISTICAL = ("keystone", "brno", "rotated", "short")  # geometries with enough pixels inside the frame for the floors below


def _case(name, kind, c):
    sw, sh, dw, dh, M, _ = PX.geometries()[name]
    return PX.float_frame(kind, PX.case_seed(name, kind, c), sh, sw, c), M, (dw, dh)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_three_implementations_agree(case):
    _, name, kind, interp, c, border = case
    src, M, dsize = _case(name, kind, c)
    payload = interp == 0
    bv = 0.0 if border is None else border
    exp = co.warp_perspective(src, M, dsize, interp, border_value=border)
    PX.same_float(wn.warp_perspective(src, M, dsize, interp, border_value=bv), exp, payload=payload)
    PX.same_float(BR.warp(src, M, dsize, interp, BR.CONSTANT, border_value=bv), exp, payload=payload)
    # the same non-zero finite border value for every case (half of them ran with it above)
    if border is None:
        nz = co.warp_perspective(src, M, dsize, interp, border_value=PX.BORDER[:c])
        PX.same_float(BR.warp(src, M, dsize, interp, BR.CONSTANT, border_value=PX.BORDER[:c]), nz, payload=payload)
        PX.same_float(wn.warp_perspective(src, M, dsize, interp, border_value=PX.BORDER[:c]), nz, payload=payload)


@pytest.mark.parametrize("case", [c for c in CASES if c[1] in STATISTICAL], ids=[c[0] for c in CASES if c[1] in STATISTICAL])
def test_results_reach_the_special_values(case):
    """Asserted on the oracle's output alone: the results the kernels are compared with do hold NaNs, infinities, subnormals and
    negative zeros in numbers."""
    _, name, kind, interp, c, border = case
    src, M, dsize = _case(name, kind, c)
    exp = co.warp_perspective(src, M, dsize, interp, border_value=border)
    nan, inf, sub = np.isnan(exp).mean(), np.isinf(exp).mean(), PX.is_subnormal(exp).mean()
    print("%s: NaN %.4f Inf %.4f subnormal %.4f" % (case[0], nan, inf, sub))
    if kind == "mixed" and interp == 1:
        assert 0.005 <= nan <= 0.15 and inf >= 0.002, (nan, inf)
    if kind == "mixed" and interp == 0:
        assert sub >= 0.02 and (PX.bits(exp) == 0x80000000).any(), sub
    if kind == "tiny" and interp == 1:
        assert sub >= 0.2, sub
    if kind == "huge" and interp == 1:
        # (see test_a_blend_of_the_largest_values_does_not_overflow: no frame can make this kind produce an Inf)
        assert not np.isinf(src).any() and not np.isinf(exp).any() and not np.isnan(exp).any()
        assert (np.abs(exp) >= 2.0 ** 127).sum() >= 1  # 4.5 % of the source lies in the top binade: results there are reached


def test_a_blend_of_the_largest_values_does_not_overflow():
    """The four weights are exact products of multiples of 1/32 and sum to 1, every product v * w rounds towards zero or is exact
    when v is +-FLT_MAX ((2 ** 24 - 1) * k is k below a multiple of 2 ** 24), and partial sums of a convex combination stay below
    FLT_MAX: so ((v00 w00 + v01 w01) + v10 w10) + v11 w11 of four FLT_MAX is FLT_MAX or the float below it for each of the 1024
    weight sets, and no "huge" frame (no Inf, |v| <= FLT_MAX) can overflow under the oracle's operation order.  A kernel that blends in another form
    (a + t * (b - a), say) would: between +FLT_MAX and -FLT_MAX neighbours, which the "huge" frames hold.  The non-vacuity condition
    for "huge" is therefore that the results reach the top binade and hold NO Inf, not that they hold one."""
    src = np.full((40, 40, 2), PX.FLT_MAX, np.float32)
    src[:, :, 1] = -PX.FLT_MAX
    Minv = np.array([[1 + 1 / 32, 0, 1.0], [0, 1 + 1 / 32, 1.0], [0, 0, 1.0]])  # destination (x, y) has fx = x, fy = y (mod 32)
    sx, sy, fx, fy = wn.fixed_point_maps((32, 32), Minv, 1)
    assert len(set(zip(fx.ravel().tolist(), fy.ravel().tolist()))) == 1024
    exp = co.warp_perspective(src, Minv, (32, 32), 1, m_is_inverse=True)
    assert set(np.unique(PX.bits(exp)).tolist()) == {0x7f7fffff, 0x7f7ffffe, 0xff7fffff, 0xff7ffffe}
    assert (PX.bits(exp[:, :, 0]) == PX.bits(exp[:, :, 1]) ^ 0x80000000).all()
    PX.same_float(wn.warp_perspective(src, Minv, (32, 32), 1, m_is_inverse=True), exp, payload=True)


def _identity(src, interp, border=None):
    h, w = src.shape[:2]
    return co.warp_perspective(src, np.eye(3), (w, h), interp, border_value=border)


def test_identity_nearest_copies_bits():
    src = PX.float_frame("mixed", 1, 45, 67, 3)
    PX.same_float(_identity(src, 0), src, payload=True)
    PX.same_float(wn.warp_perspective(src, np.eye(3), (67, 45), 0), src, payload=True)


@pytest.mark.parametrize("border", [None, [0.3, -2.5, 7.0]])
def test_identity_bilinear_multiplies_every_tap(border):
    """Identity, bilinear: the weights are (1, 0, 0, 0), and all four taps are multiplied and summed in order --
    ((v00 * 1 + v01 * 0) + v10 * 0) + v11 * 0.  So a pixel whose right, lower or lower-right neighbour is +-Inf or NaN becomes NaN
    (0 * Inf); every other pixel keeps its bits, except that -0.0 becomes +0.0 as soon as one of the three products is +0.0 (a
    neighbour with a clear sign bit; -0.0 + -0.0 stays -0.0 when all three are negative).  The last column and row take the border
    value with weight 0: finite, so they stay finite and follow the same rule."""
    src = PX.float_frame("mixed", 2, 60, 90, 3)
    h, w, c = src.shape
    got = _identity(src, 1, border)
    cval = np.zeros(c, np.float32) if border is None else np.asarray(border, np.float32)
    ext = np.empty((h + 1, w + 1, c), np.float32)
    ext[...] = cval
    ext[:h, :w] = src
    nbrs = [ext[:h, 1:], ext[1:, :w], ext[1:, 1:]]
    poisoned = ~np.isfinite(nbrs[0]) | ~np.isfinite(nbrs[1]) | ~np.isfinite(nbrs[2])
    any_positive = (~np.signbit(nbrs[0])) | (~np.signbit(nbrs[1])) | (~np.signbit(nbrs[2]))
    neg_zero = PX.bits(src) == 0x80000000
    assert np.isnan(got[poisoned]).all()
    keep = ~poisoned & ~np.isnan(src)
    exp = src.copy()
    exp[neg_zero & any_positive] = 0.0
    np.testing.assert_array_equal(PX.bits(got)[keep], PX.bits(exp)[keep])
    assert np.isnan(got[np.isnan(src)]).all()
    # non-vacuity of the three statements, and the frame's last column / row
    assert poisoned.mean() > 0.02 and (neg_zero & any_positive & ~poisoned).sum() >= 3
    edge = np.zeros((h, w, c), bool)
    edge[-1], edge[:, -1] = True, True
    assert np.isfinite(got[edge & keep]).sum() == np.isfinite(src[edge & keep]).sum() > 100
    PX.same_float(wn.warp_perspective(src, np.eye(3), (w, h), 1, border_value=0.0 if border is None else border), got)


def test_identity_bilinear_negative_zero_by_hand():
    """The two outcomes of a -0.0 pixel under the identity: +0.0 beside a positive neighbour, -0.0 among negative ones."""
    nz = np.float32(-0.0)
    src = np.array([[nz, 1.0, nz], [-1.0, -2.0, -3.0], [nz, -4.0, -5.0], [-6.0, -7.0, -8.0]], np.float32)[:, :, None]
    got = _identity(src, 1, border=[-1.0])[:, :, 0]
    assert PX.bits(got[0, 0]) == 0x00000000  # right neighbour +1.0: -0.0 + 0.0
    assert PX.bits(got[2, 0]) == 0x80000000  # neighbours -4, -7, -6... all negative
    assert PX.bits(got[0, 2]) == 0x80000000  # last column: the border value -1.0 with weight 0 is -0.0 as well
    assert PX.bits(_identity(src, 1)[0, 2, 0]) == 0x00000000  # the default border +0.0


def test_same_float_sees_what_array_equal_does_not():
    a = np.array([0.0, np.nan, 1e-40, np.inf], np.float32)
    PX.same_float(a, a.copy())
    np.testing.assert_array_equal(np.array([-0.0], np.float32), np.array([0.0], np.float32))  # (the comparison the suite used)
    for i, v in ((0, -0.0), (1, 1.0), (2, 0.0), (3, -np.inf), (0, np.nan)):
        b = a.copy()
        b[i] = v
        with pytest.raises(AssertionError):
            PX.same_float(b, a)
    q = a.copy()
    q.view(np.uint32)[1] = 0xffc00001
    PX.same_float(q, a)  # a NaN of another payload and sign
    with pytest.raises(AssertionError):
        PX.same_float(q, a, payload=True)


def test_float_frame_is_what_it_says():
    for kind in PX.KINDS:
        f = PX.float_frame(kind, 3, 64, 64, 3)
        assert f.dtype == np.float32 and f.shape == (64, 64, 3)
        np.testing.assert_array_equal(PX.bits(f), PX.bits(PX.float_frame(kind, 3, 64, 64, 3)))
    m = PX.float_frame("mixed", 4, 200, 200, 3)
    assert set(np.unique(PX.bits(m))) >= set(PX.SPECIALS.tolist())
    assert 0.03 < np.isin(PX.bits(m), PX.SPECIALS).mean() < 0.05 and 0.4 < np.signbit(m).mean() < 0.6
    expo = ((PX.bits(m) >> 23) & 0xff)
    assert expo.min() == 0 and expo.max() == 255 and len(np.unique(expo)) > 250  # every binade
    t = PX.float_frame("tiny", 4, 200, 200, 3)
    assert 0.18 < (t == 0).mean() < 0.22 and np.signbit(t[t == 0]).any() and not np.signbit(t[t == 0]).all()
    assert np.abs(t).max() < 2.0 ** -117 and PX.is_subnormal(t).mean() > 0.4
    g = PX.float_frame("huge", 4, 200, 200, 3)
    assert np.isfinite(g).all() and np.abs(g).min() >= 2.0 ** 100 and 0.005 < (np.abs(g) == PX.FLT_MAX).mean() < 0.015


def test_padded_source_and_canaries_on_the_host():
    """The layout helpers, on CPU tensors: the frames sit where the view says, everything else is the fill; a write one element
    outside a canaried view -- after a row, before the base, between two frames -- is seen, writes inside are not."""
    import torch
    for dtype, fill in ((np.uint8, PX.U8_FILL), (np.float32, float("nan"))):
        frames = np.arange(2 * 5 * 7 * 3).reshape(2, 5, 7, 3).astype(dtype)
        for offset in (0, 1, 3):
            v = PX.padded_source(frames, fill, offset=offset, device="cpu")
            np.testing.assert_array_equal(v.numpy(), frames)
            esz = frames.itemsize
            assert v.stride(0) > 5 * v.stride(1) and v.stride(1) * esz >= 7 * 3 * esz + 128
            whole = v.as_strided((v.untyped_storage().nbytes() // esz,), (1,), 0).numpy().copy()
            assert v.storage_offset() >= 2 * v.stride(1) + 64 // esz
            inside = np.zeros(whole.size, bool)
            inside[(v.storage_offset() + np.arange(2)[:, None, None] * v.stride(0) + np.arange(5)[:, None] * v.stride(1) + np.arange(21)).ravel()] = True
            rest = whole[~inside]
            assert np.isnan(rest).all() if dtype == np.float32 else (rest == fill).all()
        one = PX.padded_source(frames[0], fill, device="cpu")
        assert one.shape == (5, 7, 3)
    for dtype in (np.uint8, np.float32):
        for shape, planar in (((6, 9, 3), False), ((3, 6, 9, 3), False), ((2, 3, 6, 9), True)):
            for align in (16, 4 if dtype == np.uint8 else 16, 0):
                view, holder = PX.canaried_out(shape, dtype, 16, align=align, planar=planar, device="cpu")
                esz = holder.element_size()
                assert tuple(view.shape) == shape and (view == 77).all() and view.stride(-1) == 1
                if align:
                    assert view.data_ptr() % align == 0 and all(s * esz % align == 0 for s in view.stride()[:-1 if planar else -2])
                else:
                    rs = view.stride(-2 if planar else -3) * esz
                    assert rs % (4 if esz == 1 else 16) != 0 and view.data_ptr() % (4 if esz == 1 else 16) != 0
                PX.assert_canaries_intact(holder, view)
                view.fill_(5)
                PX.assert_canaries_intact(holder, view)
                row_end = view.storage_offset() + int(np.prod(shape[-1:] if planar else shape[-2:]))
                last = view.storage_offset() + sum((n - 1) * s for n, s in zip(view.shape, view.stride()))
                for at in (row_end, view.storage_offset() - 1, last + 1, view.storage_offset() + view.stride(0) - 1):
                    keep = holder[at].clone()
                    holder[at] = 5
                    with pytest.raises(AssertionError, match="outside the destination view"):
                        PX.assert_canaries_intact(holder, view)
                    holder[at] = keep
                PX.assert_canaries_intact(holder, view)
