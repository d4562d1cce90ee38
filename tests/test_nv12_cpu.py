"""The NV12 warp (bevwarp_warp_nv12, warp_perspective_nv12, FramePipeline(src_format="nv12")) without a device: the conversion formula's
known answers and its whole domain, the entry point's argument validation with pointers that are never dereferenced, the Python layer's
argument errors, host_plan.h's checks of an nv12_call at their limits in a stand-alone driver under the address and undefined-behaviour
sanitizers (tests/host_plan_driver.cpp), and the compiled kernels' register and scratch figures."""
import ctypes
import os
import numpy as np
import pytest
import torch

from bev_amd import _lib
from tests import codeobj
from tests import hostplan
from tests import nv12_ref as R
from tests.test_abi import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KNOWN = [((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)), ((126, 128, 128), (128, 128, 128)), ((81, 90, 240), (0, 0, 254)),
         ((145, 54, 34), (1, 255, 0)), ((41, 240, 110), (255, 0, 0)), ((0, 0, 0), (0, 154, 0)), ((255, 255, 255), (255, 125, 255)),
         ((255, 0, 0), (20, 255, 74))]  # (Y, U, V) -> (B, G, R)


@pytest.fixture(scope="module")
def lib():
    return hostplan.built_lib()


# ---- the reference conversion ---------------------------------------------------------------------------------------------------------
def test_known_answers():
    for yuv, bgr in KNOWN:
        assert tuple(int(v) for v in R.convert(*yuv)) == bgr, yuv
        assert tuple(int(v) for v in R.convert(*yuv, rgb=True)) == bgr[::-1], yuv
    # through the frame layout: one pair serves a 2 x 2 block, pixel (x, y) takes pair (y >> 1, x >> 1)
    y = np.array([[16, 235, 81, 81], [126, 16, 81, 81]], np.uint8)
    uv = np.array([[[128, 128], [90, 240]]], np.uint8)
    got = R.nv12_to_bgr(y, uv)
    assert got.shape == (2, 4, 3) and got[0, 0].tolist() == [0, 0, 0] and got[0, 1].tolist() == [255, 255, 255] and got[1, 0].tolist() == [128, 128, 128]
    assert (got[:, 2:] == np.array([0, 0, 254], np.uint8)).all()
    np.testing.assert_array_equal(R.nv12_to_bgr(y, uv, rgb=True), got[..., ::-1])


def test_whole_domain_stays_inside_int32_and_both_clamps_are_live():
    Y, U, V = np.meshgrid(np.arange(256), np.arange(256), np.arange(256), indexing="ij")
    sums, vals = R.unclamped(Y, U, V)
    lo, hi = min(int(s.min()) for s in sums), max(int(s.max()) for s in sums)
    # B at (Y <= 16, U = 0) and at (Y = 255, U = 255): the extremes of all three sums (G alone spans -159,811,307 ... 452,045,421)
    assert (lo, hi) == (524288 - 2116026 * 128, 239 * 1220542 + 524288 + 2116026 * 127) == (-270327040, 560969128) and -2 ** 31 <= lo and hi < 2 ** 31
    assert int(sums[1].min()) == -159811307
    assert (min(int(v.min()) for v in vals), max(int(v.max()) for v in vals)) == (-258, 534)
    # the int32 conversion is the clamp of those values, on every (Y, U, V)
    got = R.convert(Y, U, V)
    for k, v in enumerate((vals[2], vals[1], vals[0])):  # B, G, R
        assert (got[..., k] == np.clip(v, 0, 255)).all()


def test_frame_generators():
    y, uv = R.frame("domain", 0, 0, 0)
    assert y.shape == (4096, 4096) and uv.shape == (2048, 2048, 2)
    full = np.repeat(np.repeat(uv, 2, axis=0), 2, axis=1).astype(np.uint32)
    codes = (y.astype(np.uint32) << 16) | (full[..., 1] << 8) | full[..., 0]
    assert (np.bincount(codes.ravel(), minlength=1 << 24) == 1).all()  # every (Y, U, V) exactly once
    # "video": no channel saturates on any value the generator can draw, and its frames show it
    Y, U, V = np.meshgrid(np.arange(64, 181), np.arange(108, 149), np.arange(108, 149), indexing="ij")
    _, vals = R.unclamped(Y, U, V)
    assert (min(int(v.min()) for v in vals), max(int(v.max()) for v in vals)) == (16, 231)
    b = R.nv12_to_bgr(*R.frame("video", 1, 66, 130))
    assert 16 <= b.min() and b.max() <= 231
    yv, uvv = R.frame("video", 1, 66, 130)
    assert 64 <= yv.min() and yv.max() <= 180 and 108 <= uvv.min() and uvv.max() <= 148
    # "uniform": a quarter to under a half of the channel values saturate
    sat = [float(((c == 0) | (c == 255)).mean()) for c in (R.nv12_to_bgr(*R.frame("uniform", s, 66, 130)) for s in range(4))]
    assert all(0.25 <= s <= 0.45 for s in sat), sat
    # "phase": every pair differs from its eight neighbours in U and in V
    _, p = R.frame("phase", 3, 18, 34)
    p = p.astype(int)
    h2, w2 = p.shape[:2]
    for di, dj in ((0, 1), (1, 0), (1, 1), (1, -1)):
        a, b2 = p[:h2 - di, max(0, -dj):w2 - max(0, dj)], p[di:, max(0, dj):w2 - max(0, -dj)]
        assert a.shape == b2.shape and a.size and (a != b2).all(), (di, dj)
    # join: the single-buffer layout
    y, uv = R.frame("uniform", 0, 4, 6)
    j = R.join(y, uv)
    assert j.shape == (6, 6) and (j[:4] == y).all() and (j[4:].reshape(2, 3, 2) == uv).all()


# ---- the ABI without a device -------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_bound(lib):
    assert "bevwarp_warp_nv12" in declared_symbols() and "bevwarp_warp_nv12" in _lib.SYMBOLS
    assert getattr(ctypes.CDLL(_lib.LIB_PATH), "bevwarp_warp_nv12") is not None
    assert len(_lib.SYMBOLS["bevwarp_warp_nv12"][1]) == 20
    assert lib.bevwarp_version() == _lib.ABI_VERSION == 7
    with open(os.path.join(ROOT, "include", "bevwarp.h")) as f:
        text = f.read()
    assert "#define BEVWARP_ABI_VERSION 7" in text and "vis_homo.py:86-89" in text and "parity with OpenCV is unpinned" in text
    for k in ("1220542", "1673527", "852492", "409993", "2116026", "524288"):
        assert k in text


def test_argument_validation_without_a_device(lib):
    nv12 = lib.bevwarp_warp_nv12
    P = ctypes.c_void_p
    nan_border = ctypes.cast((ctypes.c_double * 3)(1.0, float("nan"), 1.0), P)
    # an 8 x 8 frame: Y 64 bytes at 4096, four rows of four pairs at 8192, an 8 x 8 x 3 destination far behind them; never dereferenced
    # index:  0 y     1 uv     2 dst       3 batch 4 sh 5 sw 6 dh 7 dw 8 yfs 9 yrs 10 uvfs 11 uvrs 12 dfs 13 drs 14 M  15 mc 16 interp 17 rgb 18 border 19 stream
    ok = [P(4096), P(8192), P(1 << 40), 1, 8, 8, 8, 8, 64, 8, 32, 8, 192, 24, P(16), 1, 1, 0, nan_border, None]

    def call(**patch):
        a = list(ok)
        for k, v in patch.items():
            a[int(k[1:])] = v
        return nv12(*a)

    assert call() == -4                                # otherwise valid: refused on the border value alone, before any launch
    assert call(a3=0) == 0 and call(a3=0, a18=None) == 0   # an empty batch is a no-op
    # BEVWARP_ERR_BAD_ARG
    for k in (0, 1, 2, 14):
        assert call(**{"a%d" % k: None}) == -1         # null pointers
    for k in (4, 5, 6, 7):
        assert call(**{"a%d" % k: 0}) == -1 and call(**{"a%d" % k: -2}) == -1
    assert call(a3=-1) == -1
    assert call(a4=7) == -1 and call(a5=7) == -1       # odd source sides
    assert call(a4=9, a16=2) == -1                     # ... before the interpolation is looked at
    assert call(a9=7) == -1 and call(a11=7) == -1 and call(a11=6) == -1    # row strides below src_w, either plane
    assert call(a13=23) == -1                          # ... and below a destination row
    assert call(a1=P(8193)) == -1 and call(a11=9) == -1 and call(a10=33) == -1   # odd uv base, row stride, frame stride (a single frame too)
    assert call(a3=2, a10=33) == -1 and call(a3=2, a10=30) == -1 and call(a3=2, a8=63) == -1 and call(a3=2, a12=191) == -1   # frames that overlap their successors
    assert call(a15=2) == -1 and call(a15=0) == -1 and call(a3=3, a15=2) == -1   # m_count not 1 or batch
    assert call(a3=2, a15=2) == -4 and call(a3=2, a15=1) == -4
    assert call(a15=2, a16=2) == -1                    # bad arguments come before unsupported ones
    # BEVWARP_ERR_UNSUPPORTED
    for interp in (2, 3, -1, 7):
        assert call(a16=interp) == -2
    for order in (2, -1, 91):
        assert call(a17=order) == -2
    assert call(a16=0) == -4 and call(a17=1) == -4 and call(a16=0, a17=1) == -4
    assert call(a16=2, a5=32768, a9=32768, a11=32768) == -2    # ... before the size limits
    # BEVWARP_ERR_TOO_LARGE, per plane
    assert call(a5=32768, a9=32768, a11=32768) == -3 and call(a4=32768) == -3
    assert call(a5=32766, a9=32766, a11=32766) == -4 and call(a4=32766) == -4
    assert call(a9=1 << 24) == -3 and call(a9=(1 << 24) - 1) == -4      # Y row stride
    assert call(a11=1 << 24) == -3 and call(a11=(1 << 24) - 2) == -4    # UV row stride
    assert call(a4=32766, a9=65541) == -3 and call(a4=32766, a9=65540) == -4        # the Y plane reaches 2 GiB (32766 x 65541 bytes) or stays 8 bytes below
    assert call(a4=32766, a11=131082) == -3 and call(a4=32766, a11=131080) == -4    # ... and the UV plane, 16383 rows
    assert call(a6=(1 << 20) + 1, a12=0) == -3 and call(a7=(1 << 20) + 1, a13=3 * ((1 << 20) + 1)) == -3   # destination sides (the launch plan's limit)
    assert call(a5=32768, a9=32768, a11=32768, a2=P(4096)) == -3   # ... before overlap
    # BEVWARP_ERR_OVERLAP: the destination against the Y image and against the UV image, each alone
    assert call(a2=P(4096 + 63)) == -6 and call(a2=P(4096 + 64)) == -4 and call(a2=P(4096 - 192)) == -4 and call(a2=P(4096 - 191)) == -6
    assert call(a2=P(8192 + 16)) == -6 and call(a2=P(8192 + 31)) == -6 and call(a2=P(8192 + 32)) == -4   # only the UV plane
    assert call(a2=P(8192 - 192)) == -4 and call(a2=P(8192 - 191)) == -6
    assert call(a2=P(4096 + 63), a18=None) == -6
    # the planes may overlap each other, and the single-buffer layout (uv = y + src_h * y_row_stride) is accepted
    assert call(a1=P(4096 + 64)) == -4 and call(a1=P(4096)) == -4 and call(a1=P(4096 + 2)) == -4
    assert call(a3=2, a1=P(4096 + 64), a8=96, a10=96) == -4       # ... for a batch: frames of 96 bytes
    assert call(a9=16, a1=P(4096 + 8 * 16), a11=16) == -4          # ... and with padded rows
    # BEVWARP_ERR_NOT_FINITE is the last one, for any of the three values
    for i in range(3):
        v = [1.0, 2.0, 3.0]
        v[i] = float("inf")
        assert call(a18=ctypes.cast((ctypes.c_double * 3)(*v), P)) == -4


def test_python_argument_errors_without_a_device():
    from bev_amd import cv2_compat as cv2, warp
    from bev_amd.pipeline import FramePipeline
    y, uv = torch.zeros((8, 8), dtype=torch.uint8), torch.zeros((4, 4, 2), dtype=torch.uint8)
    with pytest.raises(ValueError, match="CUDA"):
        warp.warp_perspective_nv12(y, uv, np.eye(3), (8, 8))
    with pytest.raises(ValueError, match="CUDA"):
        warp.warp_perspective_nv12(y.numpy(), uv.numpy(), np.eye(3), (8, 8))
    with pytest.raises(ValueError, match="interpolation"):
        warp.warp_perspective_nv12(y, uv, np.eye(3), (8, 8), flags=warp.INTER_CUBIC)
    # split_nv12: views of the caller's buffer, no copy
    f = torch.arange(12 * 6, dtype=torch.uint8).reshape(12, 6)
    sy, suv = warp.split_nv12(f)
    assert tuple(sy.shape) == (8, 6) and tuple(suv.shape) == (4, 3, 2) and sy.data_ptr() == f.data_ptr() and suv.data_ptr() == f.data_ptr() + 48
    assert suv.stride() == (6, 2, 1) and torch.equal(suv.reshape(4, 6), f[8:]) and torch.equal(sy, f[:8])
    fb = torch.arange(2 * 6 * 4, dtype=torch.uint8).reshape(2, 6, 4)
    by, buv = warp.split_nv12(fb)
    assert tuple(by.shape) == (2, 4, 4) and tuple(buv.shape) == (2, 2, 2, 2) and buv.stride() == (24, 4, 2, 1) and buv.data_ptr() == fb.data_ptr() + 16
    assert torch.equal(buv.reshape(2, 2, 4), fb[:, 4:])
    for bad in (torch.zeros((7, 6), dtype=torch.uint8), torch.zeros((12, 5), dtype=torch.uint8), torch.zeros((0, 6), dtype=torch.uint8),
                torch.zeros((12, 6), dtype=torch.float32), torch.zeros((12,), dtype=torch.uint8), np.zeros((12, 6), np.uint8)):
        with pytest.raises(ValueError, match="split_nv12"):
            warp.split_nv12(bad)
    with pytest.raises(ValueError, match="contiguous"):
        warp.split_nv12(torch.zeros((12, 12), dtype=torch.uint8)[:, ::2])
    # the pipeline refuses what it has no kernel for before it touches a device
    with pytest.raises(ValueError, match="planar"):
        FramePipeline((8, 8), 3, np.eye(3), (8, 8), src_format="nv12", planar=True)
    with pytest.raises(ValueError, match="channels"):
        FramePipeline((8, 8), 4, np.eye(3), (8, 8), src_format="nv12")
    with pytest.raises(ValueError, match="even"):
        FramePipeline((7, 8), 3, np.eye(3), (8, 8), src_format="nv12")
    with pytest.raises(ValueError, match="src_format"):
        FramePipeline((8, 8), 3, np.eye(3), (8, 8), src_format="nv21")
    # cvtColor: the two NV12 codes only; anything else is named
    assert (cv2.COLOR_YUV2BGR_NV12, cv2.COLOR_YUV2RGB_NV12) == (91, 90)
    with pytest.raises(NotImplementedError, match="6"):
        cv2.cvtColor(np.zeros((8, 8, 3), np.uint8), 6)  # COLOR_BGR2GRAY
    with pytest.raises(ValueError, match="NV12"):
        cv2.cvtColor(np.zeros((12, 8, 3), np.uint8), cv2.COLOR_YUV2BGR_NV12)


# ---- host_plan.h's checks of an nv12_call under the sanitizers ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver():
    return hostplan.build_driver()


def run_driver(exe, cases):
    return hostplan.run_driver(exe, ["nv12 " + " ".join(str(int(v)) for v in c) for c in cases], "plan")


def model(y, uv, dst, batch, sh, sw, dh, dw, yfs, yrs, uvfs, uvrs, dfs, drs, mc, interp, rgb):
    """check_warp_nv12 restated in exact integers (no case given to it wraps an address): the status."""
    if not y or not uv or not dst:
        return -1
    if batch < 0 or min(sh, sw, dh, dw) <= 0 or sh % 2 or sw % 2:
        return -1
    images = ((y, sh, sw, yrs, yfs, 1), (uv, sh // 2, sw, uvrs, uvfs, 2), (dst, dh, 3 * dw, drs, dfs, 1))
    for base, rows, row_bytes, rs, fs, elem in images:
        if rs < row_bytes or (batch > 1 and fs < rows * rs) or rs % elem or fs % elem or base % elem:
            return -1
    if mc != 1 and mc != batch:
        return -1
    if interp not in (0, 1) or rgb not in (0, 1):
        return -2
    for (base, rows, row_bytes, rs, fs, elem), cols in zip(images[:2], (sw, sw // 2)):
        if cols > 32767 or rows > 32767 or rs >= 1 << 24 or rows * rs >= 1 << 31:
            return -3
    if batch == 0:
        return 0

    def end(im):
        return im[0] + (batch - 1) * im[4] + (im[1] - 1) * im[3] + im[2]

    def overlap(s, d):
        if not (s[0] < end(d) and d[0] < end(s)):
            return False
        S = s[3]
        if S == d[3] and S > 0 and (batch == 1 or (s[4] % S == 0 and d[4] % S == 0)) and s[2] + d[2] <= S:
            a, b = s[0] % S, d[0] % S
            if (b - a) % S >= s[2] and (a - b) % S >= d[2]:
                return False
        return True

    return -6 if overlap(images[0], images[2]) or overlap(images[1], images[2]) else 0


def test_check_warp_nv12_at_its_limits_under_the_sanitizer(driver):
    Y0, UV0, D0 = 1 << 32, 1 << 36, 1 << 40
    cases = []

    def add(y=Y0, uv=UV0, dst=D0, batch=1, sh=8, sw=8, dh=8, dw=8, yfs=None, yrs=None, uvfs=None, uvrs=None, dfs=None, drs=None, mc=1, interp=1, rgb=0):
        yrs = sw if yrs is None else yrs
        uvrs = sw if uvrs is None else uvrs
        drs = 3 * dw if drs is None else drs
        tight = lambda rows, rs: rows * rs if abs(rows * rs) < 1 << 62 else 0  # noqa: E731  (frames back to back, where that is a 64-bit number)
        cases.append((y, uv, dst, batch, sh, sw, dh, dw, tight(sh, yrs) if yfs is None else yfs, yrs, tight(sh // 2, uvrs) if uvfs is None else uvfs, uvrs,
                      tight(dh, drs) if dfs is None else dfs, drs, mc, interp, rgb))

    # sides: the largest even side, the first refused one, and odd ones around them
    for side in (2, 32764, 32765, 32766, 32767, 32768, 65536, (1 << 31) - 2):
        add(sw=side)
        add(sh=side, yrs=8)
        add(sh=side, sw=side)
    # row strides next to 2^24, per plane, and planes next to 2^31
    for rs in ((1 << 24) - 2, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 24) + 2):
        add(yrs=rs)
        add(uvrs=rs)
        add(yrs=rs, uvrs=rs, batch=2)
    for sh, rs in ((32766, 65540), (32766, 65541), (32766, 1 << 16), (32766, 131080), (32766, 131082), (32766, 131084), (128, (1 << 24) - 1), (256, (1 << 24) - 2)):
        add(sh=sh, yrs=rs)
        add(sh=sh, uvrs=rs)
    # strides next to 2^63 (rows * stride does not fit 64 bits: compared exactly) and negative ones
    big = (1 << 63) - 1
    for v in (big, big - 1, 1 << 62, -1, -2, -(1 << 63)):
        add(yrs=v)
        add(uvrs=v)
        add(drs=v)
        add(yfs=v, batch=2)
        add(uvfs=v, batch=2)
        add(dfs=v, batch=2)
        add(uvfs=v)           # a single frame's uv frame stride is only asked to be even
    # odd strides and bases
    for off in (0, 1, 2, 3):
        add(uv=UV0 + off)
        add(uvrs=8 + off)
        add(uvfs=32 + off, batch=2)
        add(uvfs=32 + off)
        add(yrs=8 + off, y=Y0 + off, yfs=64 + 8 * off + off, batch=2)   # the Y plane takes any of them
        add(dst=D0 + off, drs=24 + off)
    # formats and counts
    for interp in (-1, 0, 1, 2, 3):
        for rgb in (-1, 0, 1, 2):
            add(interp=interp, rgb=rgb)
    for batch, mc in ((0, 1), (0, 0), (0, 5), (1, 0), (1, 2), (3, 1), (3, 3), (3, 2), (-1, 1)):
        add(batch=batch, mc=mc)
    add(y=0), add(uv=0), add(dst=0)
    for k in ("sh", "sw", "dh", "dw"):
        add(**{k: 0}), add(**{k: -8})
    # overlap: the destination next to and on either plane, batches, shared strides (column-disjoint regions of one allocation)
    for d in (Y0 - 192, Y0 - 191, Y0, Y0 + 63, Y0 + 64, UV0 - 192, UV0 - 191, UV0 + 31, UV0 + 32):
        add(dst=d)
        add(dst=d, y=Y0, uv=Y0 + 64)  # the single buffer
    add(y=Y0, uv=Y0 + 64, dst=Y0 + 96), add(y=Y0, uv=Y0 + 64, dst=Y0 + 95)
    add(y=Y0, uv=Y0 + 8 * 64, yrs=64, uvrs=64, dst=Y0 + 8, drs=64, dw=8), add(y=Y0, uv=Y0 + 8 * 64, yrs=64, uvrs=64, dst=Y0 + 40, drs=64, dw=8)   # beside both planes' columns
    add(y=Y0, uv=Y0 + 8 * 64, yrs=64, uvrs=64, dst=Y0 + 41, drs=64, dw=8), add(y=Y0, uv=Y0 + 8 * 64, yrs=64, uvrs=64, dst=Y0 + 7, drs=64, dw=8)
    add(batch=3, yfs=1 << 20, uvfs=1 << 20, dfs=1 << 20, dst=Y0 + (1 << 19)), add(batch=3, yfs=1 << 20, uvfs=1 << 20, dfs=1 << 20, dst=Y0 + (2 << 20) + 63)
    # destinations at the launch plan's limit
    add(dw=1 << 20, dh=1), add(dw=(1 << 20) + 1, dh=1), add(dh=1 << 20, dw=1), add(dh=(1 << 20) + 1, dw=1), add(dw=1 << 20, dh=1 << 20, batch=3, mc=3)
    got = run_driver(driver, cases)
    for case, nums in zip(cases, got):
        assert nums[0] == model(*case), (case, nums)
        assert nums[1] == int(all(v % 4 == 0 for v in (case[2], case[12], case[13]))), (case, nums)
        if nums[0] == 0 and case[3] > 0:
            dh, dw = case[6], case[7]
            if dh > 1 << 20 or dw > 1 << 20 or case[3] * (-(-dw // 256)) * (-(-dh // 4)) > 0x7fffffff:
                assert nums[2] == -3, (case, nums)
            else:
                assert nums[2:] == [0, case[3] * (-(-dw // 256)) * (-(-dh // 4))], (case, nums)
    statuses = [n[0] for n in got]
    assert statuses.count(0) > 40 and statuses.count(-1) > 40 and statuses.count(-2) >= 10 and statuses.count(-3) >= 15 and statuses.count(-6) >= 8
    assert any(n[2] == -3 for n in got)
    # addresses next to the top of the address space: only the sanitizer's silence is asserted (unsigned sums wrap)
    top = (1 << 64) - 1
    wrap = []
    cases = wrap
    add(y=top - 63, uv=top - 31, dst=top - 191), add(y=top - 1, uv=top - 1, dst=top), add(y=top, uv=top - 1, dst=1, batch=2, yfs=1 << 62, uvfs=1 << 62, dfs=1 << 62)
    add(y=top - 4096, uv=top - 2048, dst=8, batch=65535, yfs=big - 1, uvfs=big - 1, dfs=big, mc=65535), add(sh=32766, sw=32766, y=top - 1, uv=top - 1, dst=top - 1)
    assert len(run_driver(driver, wrap)) == len(wrap)


# ---- the compiled kernels ---------------------------------------------------------------------------------------------------------------
def test_nv12_kernels_code_object(tmp_path):
    unit = codeobj.kernels("warp_nv12.hip", tmp_path, header="warp_nv12.h")
    kernels = {n: k for n, k in unit.items() if "warp_nv12_kernel" in n}
    assert len(kernels) == len(unit) == 2 * 2, sorted(unit)  # interpolation x channel order, and nothing else in the unit
    codeobj.assert_lean(kernels)
