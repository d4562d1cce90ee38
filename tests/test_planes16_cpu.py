"""float16 / bfloat16 channel planes (bevwarp_warp_planes, warp_to_planar(out_dtype=...)) without a device: the reference conversions of
tests/planes16_ref.py against torch's CPU conversions (two independent statements of the rounding), the new entry point's argument
validation with pointers that are never dereferenced, warp_to_planar's argument checks, and host_plan.h's checks for 2-byte planes in a
stand-alone driver under the address and undefined-behaviour sanitizers (tests/host_plan_driver.cpp)."""
import ctypes
import os
import numpy as np
import pytest
import torch

from bev_amd import _lib
from tests import hostplan
from tests import planes16_ref as R
from tests.test_abi import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float16, torch.bfloat16]


@pytest.fixture(scope="module")
def lib():
    return hostplan.built_lib()


def torch_bits(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).view(torch.int16).numpy().view(np.uint16)


# ---- the reference conversions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=R.kind_of)
def test_reference_conversions_agree_with_torch(dtype):
    rng = np.random.default_rng(16)
    pats = np.concatenate([R.BOUNDARY_BITS, rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32)])
    f = pats.view(np.float32)
    got = R.to_bits(f, dtype)
    R.assert_same16(got, torch_bits(f, dtype), dtype, "reference against torch")
    assert R.is_nan16(got, dtype).sum() == np.isnan(f).sum() > 0


def test_boundary_list_holds_the_named_cases():
    f = lambda bits: np.array([bits], dtype=np.uint32).view(np.float32)  # noqa: E731
    h, b = lambda bits: int(R.f16_bits(f(bits))[0]), lambda bits: int(R.bf16_bits(f(bits))[0])  # noqa: E731
    assert float(f(0x477fe000)[0]) == 65504.0 and float(f(0x477ff000)[0]) == 65520.0 and float(f(0x33800000)[0]) == 2.0 ** -24
    assert float(f(0x387fc000)[0]) == 1023 * 2.0 ** -24 and float(f(0x387fe000)[0]) == 1023.5 * 2.0 ** -24
    # float16: ties to even around 1.0, overflow at 65520, subnormals kept, the 2^-25 tie to 0, -0 stays -0
    assert (h(0x3f7ff000), h(0x3f7fefff), h(0x3f801000), h(0x3f801001), h(0x3f803000)) == (0x3c00, 0x3bff, 0x3c00, 0x3c01, 0x3c02)
    assert (h(0x477fe000), h(0x477fefff), h(0x477ff000), h(0x47800000), h(0xc77ff000)) == (0x7bff, 0x7bff, 0x7c00, 0x7c00, 0xfc00)
    assert (h(0x33800000), h(0x33000000), h(0x33000001), h(0x33c00000), h(0x387fc000), h(0x387fe000), h(0x387fdfff)) == (1, 0, 1, 2, 0x03ff, 0x0400, 0x03ff)
    assert (h(0x80000000), h(0x00000001), h(0x80000001), h(0x7f800000)) == (0x8000, 0, 0x8000, 0x7c00)
    # bfloat16: ties to even, the carry into inf, float32 subnormals kept
    assert (b(0x3f808000), b(0x3f808001), b(0x3f818000), b(0x3f817fff)) == (0x3f80, 0x3f81, 0x3f82, 0x3f81)
    assert (b(0x7f7fffff), b(0x7f7f8000), b(0x7f7f7fff), b(0xff7fffff)) == (0x7f80, 0x7f80, 0x7f7f, 0xff80)
    assert (b(0x00000001), b(0x00008000), b(0x00008001), b(0x00018000), b(0x007fffff), b(0x80000000)) == (0, 0, 1, 2, 0x0080, 0x8000)
    for nan in (0x7fc00000, 0x7f800001, 0x7fa00123, 0xffc00001):
        assert R.is_nan16(h(nan), torch.float16) and R.is_nan16(b(nan), torch.bfloat16)
    for v in (0x00000000, 0x3f808000, 0x3f818000, 0x7f7fffff, 0x477ff000, 0x33000000, 0x33000001, 0x387fe000, 0x7f800000, 0x7fc00000):
        assert v in R.BOUNDARY_BITS and (v | 0x80000000) in R.BOUNDARY_BITS


# ---- the ABI without a device -------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_bound(lib):
    assert "bevwarp_warp_planes" in declared_symbols() and "bevwarp_warp_planes" in _lib.SYMBOLS
    assert getattr(ctypes.CDLL(_lib.LIB_PATH), "bevwarp_warp_planes") is not None
    assert lib.bevwarp_version() == _lib.ABI_VERSION == 7
    assert (_lib.F16, _lib.BF16) == (3, 4)
    with open(os.path.join(ROOT, "include", "bevwarp.h")) as f:
        text = f.read()
    assert "BEVWARP_F16 = 3" in text and "BEVWARP_BF16 = 4" in text


def test_argument_validation_without_a_device(lib):
    one, far = ctypes.c_void_p(16), ctypes.c_void_p(1 << 20)  # never dereferenced: validation fails first
    planes = lib.bevwarp_warp_planes
    # an 8 x 8 RGB source into three 8 x 8 planes of 2-byte elements: rows 16 bytes, planes 128, frames 384
    ok = [one, far, 1, 8, 8, 8, 8, 3, 192, 24, 384, 128, 16, one, 1, _lib.U8, 1, None, None, None, _lib.F16, None]
    nan_scale = ctypes.cast((ctypes.c_double * 3)(1.0, float("nan"), 1.0), ctypes.c_void_p)

    def call(**patch):
        a = list(ok)
        for k, v in patch.items():
            a[int(k[1:])] = v
        return planes(*a)

    for pd in (_lib.F16, _lib.BF16):
        assert call(a20=pd, a2=0) == 0                 # an empty batch is a no-op
        assert call(a20=pd, a18=nan_scale) == -4       # otherwise valid arguments: refused on the scale alone
        assert call(a20=pd, a19=nan_scale) == -4       # ... and on the bias
        assert call(a20=pd, a16=2) == -2               # BEVWARP_CUBIC, as for the float32 planes
        assert call(a20=pd, a12=17, a18=nan_scale) == -1    # odd row stride
        assert call(a20=pd, a11=129, a18=nan_scale) == -1   # odd plane stride
        assert call(a20=pd, a10=385, a2=2, a18=nan_scale) == -1   # odd frame stride
        assert call(a20=pd, a10=385, a18=nan_scale) == -1   # (asked of a single frame too, as the float32 planes do)
        assert call(a20=pd, a1=ctypes.c_void_p((1 << 20) + 1), a18=nan_scale) == -1  # odd base
        assert call(a20=pd, a12=14, a18=nan_scale) == -1    # row stride shorter than a row
        assert call(a20=pd, a12=18, a11=144, a10=432, a18=nan_scale) == -4  # multiples of 2 only (no wide stores) are accepted
        assert call(a20=pd, a1=ctypes.c_void_p(16 + 100)) == -6            # a destination inside the source
        assert call(a20=pd, a1=ctypes.c_void_p(16 + 192), a18=nan_scale) == -4   # adjacent is fine
        assert call(a20=pd, a0=ctypes.c_void_p((1 << 20) + 384), a18=nan_scale) == -4   # a source right behind the last plane's last element
        assert call(a20=pd, a0=ctypes.c_void_p((1 << 20) + 382)) == -6                  # ... and one that starts on that element
        assert call(a20=pd, a15=_lib.F16) == -2 and call(a20=pd, a15=_lib.BF16) == -2  # no 16-bit pixel type
        assert call(a20=pd, a0=None) == -1
    for pd in (_lib.U8, _lib.F64, 7, -1):
        assert call(a20=pd) == -2
        assert call(a20=pd, a18=nan_scale) == -2
    # float32 planes through the new entry are bevwarp_warp_planar, call for call
    f32 = dict(a20=_lib.F32, a12=32, a11=256, a10=768)
    planar = lib.bevwarp_warp_planar
    for patch in (dict(), dict(a12=34), dict(a11=258), dict(a10=770), dict(a18=nan_scale), dict(a1=ctypes.c_void_p(16 + 100)), dict(a2=0), dict(a16=2), dict(a7=5)):
        a = list(ok)
        for k, v in dict(f32, **patch).items():
            a[int(k[1:])] = v
        if not patch:
            a[18] = nan_scale  # (a valid call would launch: stop it on the scale)
        assert planes(*a) == planar(*(a[:20] + a[21:])), patch
    assert call(**dict(f32, a12=34, a18=nan_scale)) == -1 and call(**dict(f32, a11=258, a18=nan_scale)) == -1 and call(**dict(f32, a10=770, a18=nan_scale)) == -1
    assert call(**dict(f32, a18=nan_scale)) == -4 and call(**dict(f32, a16=2)) == -2
    # the existing entry points keep refusing the new enum values as a pixel or point type
    assert lib.bevwarp_warp(one, far, 1, 8, 8, 8, 8, 3, 192, 24, 192, 24, one, 1, _lib.F16, 1, None, None) == -2
    assert lib.bevwarp_warp_planar(*(ok[:15] + [_lib.BF16] + ok[16:20] + [None])) == -2
    assert lib.bevwarp_tile_classes_bytes(1, 8, 8, 8, 8, 3, _lib.F16, 1) == -2
    assert lib.bevwarp_project_points(one, one, 4, 2, np.eye(3).ctypes.data_as(ctypes.c_void_p), _lib.F16, None) == -2
    assert lib.bevwarp_rbox_iou(one, 1, 5, one, 1, 5, one, _lib.BF16, None) == -2


def test_warp_to_planar_checks_out_dtype_before_it_needs_a_device():
    from bev_amd import warp
    img = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match="out_dtype"):
        warp.warp_to_planar(img, np.eye(3), (8, 8), out_dtype=torch.float64)
    with pytest.raises(ValueError, match="out_dtype"):
        warp.warp_to_planar(img, np.eye(3), (8, 8), out_dtype=torch.uint8)
    with pytest.raises(ValueError, match="out must be"):
        warp.warp_to_planar(img, np.eye(3), (8, 8), out_dtype=torch.float16, out=torch.zeros((3, 8, 8), dtype=torch.float32))
    with pytest.raises(ValueError, match="out must be"):
        warp.warp_to_planar(img, np.eye(3), (8, 8), out=torch.zeros((3, 8, 8), dtype=torch.bfloat16))
    from bev_amd.pipeline import FramePipeline
    with pytest.raises(ValueError, match="plane_dtype"):
        FramePipeline((8, 8), 3, np.eye(3), (8, 8), planar=True, plane_dtype=torch.float64)


# ---- host_plan.h for 2-byte planes, under the sanitizers ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver():
    return hostplan.build_driver()


def run_driver(exe, cases):
    return hostplan.run_driver(exe, ["planes %d %d %d %d %d %d %d %d %d %d" % c for c in cases], "plan")


def model(src, dst, batch, c, dh, dw, fs, ps, rs, elem):
    """check_warp for planes, restated: (status, store alignment, wide stores, bytes of a row).  Exact integers: no case here wraps."""
    row = dw * elem
    wide = all(v % (4 * elem) == 0 for v in (dst, fs, ps, rs))
    res = lambda st: (st, 4 * elem, int(wide), row)  # noqa: E731
    if rs < row or ps < dh * rs or any(v % elem for v in (dst, rs, ps, fs)):
        return res(-1)
    if ps < 0 or (batch > 1 and fs < c * ps):
        return res(-1)
    if batch == 0:
        return res(0)
    s_end = src + (batch - 1) * 64 * c + 64 * c
    d_end = dst + (batch - 1) * fs + (dh - 1) * rs + row + (c - 1) * ps
    return res(-6 if (src < d_end and dst < s_end) else 0)


def test_plane_checks_for_two_byte_elements_under_the_sanitizer(driver):
    src = 1 << 30
    cases = []
    # alignments 2, 4, 8 and 16 (and 1: refused) of the base and of each stride, one at a time and all together; 301 x 9 planes, batch 2
    dh, dw, c = 9, 301, 3
    for elem in (2, 4):
        rs0 = 640 * elem // 2
        ps0, fs0 = 16 * rs0, 64 * rs0
        for off in (0, 1, 2, 4, 8, 16):
            for which in range(5):
                d = [1 << 20, fs0, ps0, rs0]
                if which < 4:
                    d[which] += off
                else:
                    d = [v + off for v in d]
                cases.append((src, d[0], 2, c, dh, dw, d[1], d[2], d[3], elem))
    # sizes at the limits: the widest destination row the planner takes, a row stride that exactly holds it, one byte less, one element more
    wmax = 1 << 20
    for elem in (2, 4):
        row = wmax * elem
        cases += [(src, 1 << 40, 1, 4, 2, wmax, 0, 2 * row, row, elem), (src, 1 << 40, 1, 4, 2, wmax, 0, 2 * row, row - elem, elem),
                  (src, 1 << 40, 2, 4, 2, wmax, 8 * row, 2 * row, row, elem), (src, 1 << 40, 2, 4, 2, wmax, 8 * row - elem, 2 * row, row, elem),
                  (src, 1 << 40, 2, 4, 2, wmax, 8 * row, 2 * row - elem, row, elem), (src, 1 << 40, 0, 4, 2, wmax, 8 * row, 2 * row, row, elem),
                  (src, 1 << 40, 1, 1, 1, 1, 0, elem, elem, elem), (src, 1 << 40, 1, 1, 1, 1, 0, elem, elem - 1, elem)]
    # strides next to 2^62: dh * rs and channels * ps are compared exactly although they are not representable in 64 bits
    big = 1 << 61
    cases += [(src, 1 << 40, 2, 4, 32767, 8, big, big // 4, 16, 2), (src, 1 << 40, 2, 4, 3, 8, 4 * big - 2, big, big // 2, 2), (src, 1 << 40, 2, 4, 3, 8, 4 * big - 2, big, big // 2 + 2, 2),
              (src, 1 << 40, 1, 2, 1, 8, 0, 2 * big, big, 2)]
    # overlap: the bounding range of ALL planes of all frames counts, in 2-byte elements
    cases += [(4096, 4096 + 192 * 2, 2, 3, 8, 8, 384, 128, 16, 2), (4096, 4096 + 192 * 2 - 2, 2, 3, 8, 8, 384, 128, 16, 2), (8192, 8192 - 768, 2, 3, 8, 8, 384, 128, 16, 2),
              (8192, 8192 - 768 + 2, 2, 3, 8, 8, 384, 128, 16, 2), (8192, 8192 - 1536 + 4, 2, 3, 8, 8, 768, 256, 32, 4), (8192, 8192 - 1536, 2, 3, 8, 8, 768, 256, 32, 4)]
    got = run_driver(driver, cases)
    for case, nums in zip(cases, got):
        assert tuple(nums) == model(*case), (case, nums)
    statuses = [n[0] for n in got]
    assert statuses.count(0) > 20 and statuses.count(-1) > 20 and statuses.count(-6) >= 3
    assert {(n[1], n[2]) for n in got} == {(8, 0), (8, 1), (16, 0), (16, 1)}
    # addresses next to UINTPTR_MAX: only the sanitizer's silence is asserted (unsigned sums wrap)
    top = (1 << 64) - 1
    assert len(run_driver(driver, [(src, top - 1, 2, 4, 8, 8, 1 << 62, 1 << 60, 1 << 50, 2), (top - 4096, top - 8191, 2, 3, 8, 8, 384, 128, 16, 2)])) == 2
