"""The warps into NV12 (bevwarp_warp_to_nv12, bevwarp_warp_nv12_to_nv12; warp_perspective_to_nv12, warp_nv12_to_nv12;
FramePipeline(dst_format="nv12")) without a device: the conversion formula's known answers, its whole domain and its chroma siting, the
entry points' argument validation with pointers that are never dereferenced, the Python layer's argument errors, host_plan.h's
checks of a to_nv12_call / nv12_to_nv12_call at their limits in a stand-alone driver under the address and undefined-behaviour sanitizers
(tests/host_plan_driver.cpp), and the compiled kernels' register and scratch figures."""
import ctypes
import os
import numpy as np
import pytest
import torch

from bev_amd import _lib
from tests import codeobj
from tests import hostplan
from tests import nv12_out_ref as R
from tests import nv12_ref
from tests.test_abi import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KNOWN = [((0, 0, 0), (16, 128, 128)), ((255, 255, 255), (235, 128, 128)), ((128, 128, 128), (126, 128, 128)), ((0, 0, 255), (82, 90, 240)),
         ((0, 255, 0), (145, 54, 34)), ((255, 0, 0), (41, 240, 110)), ((10, 200, 77), (138, 63, 87)), ((255, 255, 0), (170, 166, 16)),
         ((1, 2, 3), (18, 127, 129))]  # (B, G, R) -> (Y, U, V)


@pytest.fixture(scope="module")
def lib():
    return hostplan.built_lib()


# ---- the reference conversion ---------------------------------------------------------------------------------------------------------
def test_known_answers():
    for bgr, want in KNOWN:
        b, g, r = bgr
        assert tuple(int(v) for v in R.yuv(r, g, b)) == want, bgr
        # through the frame layout, in either channel order: a 2 x 2 frame of one colour
        for rgb in (False, True):
            px = np.array(bgr[::-1] if rgb else bgr, np.uint8)
            y, uv = R.bgr_to_nv12(np.broadcast_to(px, (2, 2, 3)), rgb=rgb)
            assert y.shape == (2, 2) and uv.shape == (1, 1, 2) and y.dtype == uv.dtype == np.uint8
            assert (y == want[0]).all() and uv[0, 0].tolist() == list(want[1:]), (bgr, rgb)


@pytest.fixture(scope="module")
def domain():
    """Every (R, G, B) once, as three flat arrays."""
    v = np.arange(1 << 24, dtype=np.int32)
    return v >> 16, (v >> 8) & 255, v & 255


def test_whole_domain_stays_inside_int32_and_no_clamp_is_live(domain):
    r, g, b = domain
    sy, su, sv = R.sums(r, g, b)
    assert (int(sy.min()), int(sy.max())) == (17301504, 246986634)
    assert (min(int(su.min()), int(sv.min())), max(int(su.max()), int(sv.max()))) == (17359651, 252124636)
    assert all(0 <= int(s.min()) and int(s.max()) < 2 ** 31 for s in (sy, su, sv))  # int32 holds every sum, and no sum is negative
    y, u, v = R.yuv(r, g, b)
    assert (int(y.min()), int(y.max())) == (16, 235)
    assert (int(u.min()), int(u.max())) == (16, 240) and (int(v.min()), int(v.max())) == (16, 240)
    for got, s in zip((y, u, v), (sy, su, sv)):  # the int32 conversion is the shifted sum itself: saturate_cast is never live
        assert (got == (s >> 20)).all()


def test_chroma_is_the_top_left_pixel_of_the_block():
    img = np.array([[[0, 0, 255], [0, 255, 0]], [[255, 0, 0], [10, 200, 77]]], np.uint8)  # four different pixels, B, G, R
    y, uv = R.bgr_to_nv12(img)
    assert y.tolist() == [[82, 145], [41, 138]] and uv.tolist() == [[[90, 240]]]  # (0, 0, 255)'s pair, not a mean (which would be 111.75, 117.75)
    # two blocks side by side and on top of each other
    rng = np.random.default_rng(5)
    big = rng.integers(0, 256, (6, 8, 3), dtype=np.uint8)
    y, uv = R.bgr_to_nv12(big)
    for i in range(3):
        for j in range(4):
            b, g, r = (int(c) for c in big[2 * i, 2 * j])
            assert uv[i, j].tolist() == [int(c) for c in R.yuv(r, g, b)[1:]]
    yr, uvr = R.bgr_to_nv12(big[..., ::-1], rgb=True)
    assert (yr == y).all() and (uvr == uv).all()


def test_consistency_with_the_inverse_conversion(domain):
    r, g, b = domain
    y, u, v = R.yuv(r, g, b)
    back = nv12_ref.convert(y, u, v).astype(np.int32)  # B, G, R
    err = np.abs(back - np.stack([b, g, r], axis=-1))
    assert int(err.max()) == 2  # (at most 2 per channel, and 2 occurs)
    assert all(int(err[:, k].max()) <= 2 for k in range(3))


# ---- the ABI without a device -------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("bevwarp_warp_to_nv12", 20), ("bevwarp_warp_nv12_to_nv12", 22)):
        assert name in declared_symbols() and name in _lib.SYMBOLS
        assert getattr(raw, name) is not None
        assert len(_lib.SYMBOLS[name][1]) == nargs
    assert lib.bevwarp_version() == _lib.ABI_VERSION == 7
    with open(os.path.join(ROOT, "include", "bevwarp.h")) as f:
        text = f.read()
    assert "#define BEVWARP_ABI_VERSION 7" in text and "vis_homo.py:109-111" in text and "bev/io/utils.py:89-99" in text
    assert "parity with OpenCV is unpinned" in text
    for k in ("269484", "528482", "102760", "155188", "305135", "460324", "385875", "74448"):
        assert k in text


P = ctypes.c_void_p
D0 = 1 << 40


def nan_border():
    return ctypes.cast((ctypes.c_double * 3)(1.0, float("nan"), 1.0), P)


def caller(fn, ok):
    def call(**patch):
        a = list(ok)
        for k, v in patch.items():
            a[int(k[1:])] = v
        return fn(*a)
    return call


def test_argument_validation_of_the_bgr_source_without_a_device(lib):
    # an 8 x 8 x 3 source of 192 bytes at 4096; an 8 x 8 destination in one buffer far behind it: Y 64 bytes, then four rows of four pairs; never dereferenced
    # index:  0 src   1 dst_y 2 dst_uv    3 batch 4 sh 5 sw 6 dh 7 dw 8 sfs 9 srs 10 yfs 11 yrs 12 uvfs 13 uvrs 14 M 15 mc 16 interp 17 rgb 18 border 19 stream
    border = nan_border()
    call = caller(lib.bevwarp_warp_to_nv12, [P(4096), P(D0), P(D0 + 64), 1, 8, 8, 8, 8, 192, 24, 64, 8, 32, 8, P(16), 1, 1, 0, border, None])
    assert call() == -4                                # otherwise valid (the single-buffer layout): refused on the border value alone, before any launch
    assert call(a3=0) == 0 and call(a3=0, a18=None) == 0   # an empty batch is a no-op
    # BEVWARP_ERR_BAD_ARG
    for k in (0, 1, 2, 14):
        assert call(**{"a%d" % k: None}) == -1         # null pointers
    for k in (4, 5, 6, 7):
        assert call(**{"a%d" % k: 0}) == -1 and call(**{"a%d" % k: -2}) == -1
    assert call(a3=-1) == -1
    assert call(a6=6) == -4 and call(a7=6) == -4 and call(a4=7, a5=5) == -4      # smaller even destinations; odd SOURCE sides are fine here
    assert call(a6=7) == -1 and call(a7=7) == -1       # odd destination sides
    assert call(a6=7, a16=2) == -1 and call(a7=5, a17=3) == -1    # ... before the interpolation and the order are looked at
    assert call(a9=23) == -1 and call(a11=7) == -1 and call(a13=7) == -1 and call(a13=6) == -1   # row strides below a row: source, Y, UV
    assert call(a2=P(D0 + 65)) == -1 and call(a13=9) == -1 and call(a12=33) == -1   # odd uv base, row stride, frame stride (a single frame too)
    assert call(a3=2, a8=191) == -1 and call(a3=2, a10=63) == -1 and call(a3=2, a12=30) == -1   # frames that overlap their successors
    assert call(a15=2) == -1 and call(a15=0) == -1 and call(a3=3, a10=96, a12=96, a15=2) == -1   # m_count not 1 or batch
    assert call(a3=2, a10=96, a12=96, a15=2) == -4 and call(a3=3, a10=96, a12=96, a15=1) == -4   # batches of single buffers, 96 bytes a frame
    assert call(a15=2, a16=2) == -1                    # bad arguments come before unsupported ones
    # BEVWARP_ERR_UNSUPPORTED
    for interp in (2, 3, -1, 7):
        assert call(a16=interp) == -2
    for order in (2, -1, 91):
        assert call(a17=order) == -2
    assert call(a16=0) == -4 and call(a17=1) == -4 and call(a16=0, a17=1) == -4
    assert call(a16=2, a5=32768, a9=98304) == -2       # ... before the size limits
    # BEVWARP_ERR_TOO_LARGE: bevwarp_warp's source limits
    assert call(a5=32768, a9=98304) == -3 and call(a4=32768) == -3
    assert call(a5=32767, a9=98301) == -4 and call(a4=32767) == -4
    assert call(a9=1 << 24) == -3 and call(a9=(1 << 24) - 1) == -4
    assert call(a4=32767, a9=65539) == -3 and call(a4=32767, a9=65538) == -4   # the frame reaches 2 GiB or stays below
    assert call(a5=32768, a9=98304, a1=P(4096)) == -3  # ... before overlap
    # BEVWARP_ERR_OVERLAP: either destination plane against the source ...
    assert call(a1=P(4096 + 191)) == -6 and call(a1=P(4096 + 192)) == -4 and call(a1=P(4096 - 64)) == -4 and call(a1=P(4096 - 63)) == -6
    assert call(a2=P(4096 + 190)) == -6 and call(a2=P(4096 + 192)) == -4 and call(a2=P(4096 - 32)) == -4 and call(a2=P(4096 - 30)) == -6
    assert call(a1=P(4096 + 191), a18=None) == -6
    # ... the side-by-side refinement: source rows of 24 bytes and Y rows of 8 bytes in one allocation of 64-byte rows
    assert call(a9=64, a11=64, a1=P(4096 + 24)) == -4 and call(a9=64, a11=64, a1=P(4096 + 23)) == -6 and call(a9=64, a11=64, a1=P(4096 + 56)) == -4
    assert call(a9=64, a11=64, a1=P(4096 + 57)) == -6
    # ... and the two destination planes against each other: adjacent is fine, a shared byte is not
    assert call(a2=P(D0 + 62)) == -6 and call(a2=P(D0)) == -6 and call(a2=P(D0 - 30)) == -6 and call(a2=P(D0 - 32)) == -4
    assert call(a3=2, a10=96, a12=96, a2=P(D0 + 62)) == -6 and call(a3=2, a10=96, a12=96, a2=P(D0 + 96)) == -6   # (frame 0's pairs on frame 1's Y)
    assert call(a3=2, a2=P(D0 + 64)) == -6             # two frames of Y back to back run over the pairs
    assert call(a3=2, a2=P(1 << 41)) == -4             # two allocations
    assert call(a3=2, a11=16, a13=16, a2=P(D0 + 128), a10=192, a12=192) == -4   # single buffers with padded rows
    # BEVWARP_ERR_TOO_LARGE again: destination sides, the launch plan's limit, after the overlap
    far = P(1 << 41)
    assert call(a6=(1 << 20) + 2, a2=far) == -3 and call(a7=(1 << 20) + 2, a11=(1 << 20) + 2, a13=(1 << 20) + 2, a2=far) == -3
    assert call(a6=1 << 20, a2=far) == -4 and call(a6=(1 << 20) + 2, a2=P(D0 + 64)) == -6
    # BEVWARP_ERR_NOT_FINITE is the last one, for any of the three values
    for i in range(3):
        v = [1.0, 2.0, 3.0]
        v[i] = float("inf")
        assert call(a18=ctypes.cast((ctypes.c_double * 3)(*v), P)) == -4
    assert call(a6=(1 << 20) + 2, a2=far, a18=None) == -3


def test_argument_validation_of_the_nv12_source_without_a_device(lib):
    # an 8 x 8 source: Y 64 bytes at 4096, four rows of four pairs at 8192; the destination as above
    # index: 0 y 1 uv 2 dst_y 3 dst_uv 4 batch 5 sh 6 sw 7 dh 8 dw 9 yfs 10 yrs 11 uvfs 12 uvrs 13 dyfs 14 dyrs 15 duvfs 16 duvrs 17 M 18 mc 19 interp 20 border 21 stream
    border = nan_border()
    call = caller(lib.bevwarp_warp_nv12_to_nv12, [P(4096), P(8192), P(D0), P(D0 + 64), 1, 8, 8, 8, 8, 64, 8, 32, 8, 64, 8, 32, 8, P(16), 1, 1, border, None])
    assert call() == -4
    assert call(a4=0) == 0 and call(a4=0, a20=None) == 0
    for k in (0, 1, 2, 3, 17):
        assert call(**{"a%d" % k: None}) == -1
    for k in (5, 6, 7, 8):
        assert call(**{"a%d" % k: 0}) == -1 and call(**{"a%d" % k: -2}) == -1
    assert call(a4=-1) == -1
    assert call(a5=7) == -1 and call(a6=7) == -1 and call(a7=7) == -1 and call(a8=7) == -1   # odd sides, source and destination
    assert call(a5=6) == -4 and call(a6=6) == -4 and call(a7=6) == -4 and call(a8=6) == -4
    assert call(a7=7, a19=2) == -1
    assert call(a10=7) == -1 and call(a12=6) == -1 and call(a14=7) == -1 and call(a16=6) == -1   # row strides below a row, all four planes
    assert call(a1=P(8193)) == -1 and call(a12=9) == -1 and call(a11=33) == -1       # odd uv base / row stride / frame stride of the source ...
    assert call(a3=P(D0 + 65)) == -1 and call(a16=9) == -1 and call(a15=33) == -1    # ... and of the destination
    assert call(a4=2, a9=63) == -1 and call(a4=2, a11=30) == -1 and call(a4=2, a13=63) == -1 and call(a4=2, a15=30) == -1
    assert call(a18=2) == -1 and call(a18=0) == -1
    assert call(a4=2, a13=96, a15=96, a18=2) == -4 and call(a4=2, a13=96, a15=96) == -4
    for interp in (2, 3, -1, 7):
        assert call(a19=interp) == -2
    assert call(a19=0) == -4
    assert call(a19=2, a6=32768, a10=32768, a12=32768) == -2
    assert call(a6=32768, a10=32768, a12=32768) == -3 and call(a5=32768) == -3 and call(a6=32766, a10=32766, a12=32766) == -4
    assert call(a10=1 << 24) == -3 and call(a12=1 << 24) == -3 and call(a12=(1 << 24) - 2) == -4
    assert call(a6=32768, a10=32768, a12=32768, a2=P(4096)) == -3
    # overlap: each destination plane against each source plane
    assert call(a2=P(4096 + 63)) == -6 and call(a2=P(4096 + 64)) == -4 and call(a2=P(8192 - 63)) == -6 and call(a2=P(8192 - 64)) == -4
    assert call(a3=P(4096 + 62)) == -6 and call(a3=P(4096 + 64)) == -4 and call(a3=P(8192 + 30)) == -6 and call(a3=P(8192 + 32)) == -4
    assert call(a2=P(4096 + 63), a20=None) == -6
    # the source planes may overlap each other and the source's single-buffer layout is accepted; the destination planes may not
    assert call(a1=P(4096)) == -4 and call(a1=P(4096 + 2)) == -4 and call(a1=P(4096 + 64)) == -4
    assert call(a3=P(D0)) == -6 and call(a3=P(D0 + 62)) == -6 and call(a3=P(D0 - 32)) == -4
    far = P(1 << 41)
    assert call(a7=(1 << 20) + 2, a3=far) == -3 and call(a7=1 << 20, a3=far) == -4
    for i in range(3):
        v = [1.0, 2.0, 3.0]
        v[i] = float("-inf")
        assert call(a20=ctypes.cast((ctypes.c_double * 3)(*v), P)) == -4


def test_python_argument_errors_without_a_device():
    from bev_amd import warp
    from bev_amd.pipeline import FramePipeline
    src = torch.zeros((8, 8, 3), dtype=torch.uint8)
    y, uv = torch.zeros((8, 8), dtype=torch.uint8), torch.zeros((4, 4, 2), dtype=torch.uint8)
    with pytest.raises(ValueError, match="CUDA"):
        warp.warp_perspective_to_nv12(src, np.eye(3), (8, 8))
    with pytest.raises(ValueError, match="CUDA"):
        warp.warp_perspective_to_nv12(src.numpy(), np.eye(3), (8, 8))
    with pytest.raises(ValueError, match="CUDA"):
        warp.warp_nv12_to_nv12(y, uv, np.eye(3), (8, 8))
    for fn, args in ((warp.warp_perspective_to_nv12, (src,)), (warp.warp_nv12_to_nv12, (y, uv))):
        with pytest.raises(ValueError, match="interpolation"):
            fn(*args, np.eye(3), (8, 8), flags=warp.INTER_CUBIC)
        for dsize in ((7, 8), (8, 7), (0, 8), (8, -2)):
            with pytest.raises(ValueError, match="even"):
                fn(*args, np.eye(3), dsize)
    # the pipeline refuses what it has no kernel for before it touches a device
    with pytest.raises(ValueError, match="dst_format"):
        FramePipeline((8, 8), 3, np.eye(3), (8, 8), dst_format="i420")
    with pytest.raises(ValueError, match="planar"):
        FramePipeline((8, 8), 3, np.eye(3), (8, 8), dst_format="nv12", planar=True)
    with pytest.raises(ValueError, match="channels"):
        FramePipeline((8, 8), 4, np.eye(3), (8, 8), dst_format="nv12")
    with pytest.raises(ValueError, match="dtype"):
        FramePipeline((8, 8), 3, np.eye(3), (8, 8), dst_format="nv12", dtype=torch.float32)
    for dsize in ((7, 8), (8, 7)):
        with pytest.raises(ValueError, match="even dsize"):
            FramePipeline((8, 8), 3, np.eye(3), dsize, dst_format="nv12")
        with pytest.raises(ValueError, match="even dsize"):
            FramePipeline((8, 8), 3, np.eye(3), dsize, dst_format="nv12", src_format="nv12")
    with pytest.raises(ValueError, match="INTER"):
        FramePipeline((8, 8), 3, np.eye(3), (8, 8), dst_format="nv12", flags=warp.INTER_CUBIC)
    with pytest.raises(ValueError, match="planar"):  # (as before)
        FramePipeline((8, 8), 3, np.eye(3), (8, 8), src_format="nv12", planar=True)


# ---- host_plan.h's checks under the sanitizers ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver():
    return hostplan.build_driver()


def run_driver(exe, cases):
    return hostplan.run_driver(exe, [c[0] + " " + " ".join(str(int(v)) for v in c[1:]) for c in cases], "plan")


def model(sources, dsts, batch, sh, sw, dh, dw, mc, interp, rgb, nv12):
    """check_warp_to_nv12 / check_warp_nv12_to_nv12 restated in exact integers (no case given to it wraps an address): the status.
    An image is (base, rows, row bytes, row stride, frame stride, element size); `sources` come with their columns."""
    images = [s[0] for s in sources] + list(dsts)
    if any(not im[0] for im in images):
        return -1
    if batch < 0 or min(sh, sw, dh, dw) <= 0 or dh % 2 or dw % 2 or (nv12 and (sh % 2 or sw % 2)):
        return -1
    for base, rows, row_bytes, rs, fs, elem in images:
        if rs < row_bytes or (batch > 1 and fs < rows * rs) or rs % elem or fs % elem or base % elem:
            return -1
    if mc != 1 and mc != batch:
        return -1
    if interp not in (0, 1) or rgb not in (0, 1):
        return -2
    for (base, rows, row_bytes, rs, fs, elem), cols in sources:
        if cols > 32767 or rows > 32767 or rs >= 1 << 24 or rows * rs >= 1 << 31:
            return -3
    if batch == 0:
        return 0

    def end(im, n):
        return im[0] + (n - 1) * im[4] + (im[1] - 1) * im[3] + im[2]

    def overlap(s, d, n=batch):
        if not (s[0] < end(d, n) and d[0] < end(s, n)):
            return False
        S = s[3]
        if S == d[3] and S > 0 and (n == 1 or (s[4] % S == 0 and d[4] % S == 0)) and s[2] + d[2] <= S:
            a, b = s[0] % S, d[0] % S
            if (b - a) % S >= s[2] and (a - b) % S >= d[2]:
                return False
        return True

    def written(a, b):
        if batch > 1 and a[4] == b[4] and max(end(a, 1), end(b, 1)) - min(a[0], b[0]) <= a[4]:
            return overlap(a, b, 1)
        return overlap(a, b)

    if any(overlap(s[0], d) for s in sources for d in dsts) or written(dsts[0], dsts[1]):
        return -6
    return 0


def test_checks_at_their_limits_under_the_sanitizer(driver):
    S0, Y0, UV0, DY0, DUV0 = 1 << 32, 1 << 33, 1 << 34, 1 << 40, 1 << 41
    cases, expect = [], []
    tight = lambda rows, rs: rows * rs if abs(rows * rs) < 1 << 62 else 0  # noqa: E731  (frames back to back, where that is a 64-bit number)

    def add(nv12, src=S0, y=Y0, uv=UV0, dy=DY0, duv=DUV0, batch=1, sh=8, sw=8, dh=8, dw=8, sfs=None, srs=None, yfs=None, yrs=None, uvfs=None, uvrs=None,
            dyfs=None, dyrs=None, duvfs=None, duvrs=None, mc=1, interp=1, rgb=0):
        srs = 3 * sw if srs is None else srs
        yrs, uvrs = (sw if yrs is None else yrs), (sw if uvrs is None else uvrs)
        dyrs, duvrs = (dw if dyrs is None else dyrs), (dw if duvrs is None else duvrs)
        sfs = tight(sh, srs) if sfs is None else sfs
        yfs, uvfs = (tight(sh, yrs) if yfs is None else yfs), (tight(sh // 2, uvrs) if uvfs is None else uvfs)
        dyfs, duvfs = (tight(dh, dyrs) if dyfs is None else dyfs), (tight(dh // 2, duvrs) if duvfs is None else duvfs)
        dsts = [(dy, dh, dw, dyrs, dyfs, 1), (duv, dh // 2 if dh >= 0 else -(-dh // 2), dw, duvrs, duvfs, 2)]
        if nv12:
            cases.append(("nv12_to_nv12", y, uv, dy, duv, batch, sh, sw, dh, dw, yfs, yrs, uvfs, uvrs, dyfs, dyrs, duvfs, duvrs, mc, interp))
            sources = [((y, sh, sw, yrs, yfs, 1), sw), ((uv, sh // 2, sw, uvrs, uvfs, 2), sw // 2)]
            rgb = 0
        else:
            cases.append(("to_nv12", src, dy, duv, batch, sh, sw, dh, dw, sfs, srs, dyfs, dyrs, duvfs, duvrs, mc, interp, rgb))
            sources = [((src, sh, 3 * sw, srs, sfs, 1), sw)]
        expect.append((model(sources, dsts, batch, sh, sw, dh, dw, mc, interp, rgb, nv12), dsts, batch, dh, dw))

    for nv12 in (False, True):
        # sides: the largest admitted side, the first refused one, and odd ones around them
        for side in (2, 3, 32765, 32766, 32767, 32768, 65536, (1 << 31) - 2):
            add(nv12, sw=side)
            add(nv12, sh=side, srs=24, yrs=8)
            add(nv12, sh=side, sw=side)
        for side in (1, 2, 3, 4, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 20) + 2):
            add(nv12, dw=side, dh=2), add(nv12, dh=side, dw=2)
        add(nv12, dw=1 << 20, dh=1 << 20, batch=3, mc=3, dyfs=1 << 42, duvfs=1 << 42, dy=1 << 50, duv=1 << 60)
        # row strides next to 2^24 and frames next to 2^31
        for rs in ((1 << 24) - 2, (1 << 24) - 1, 1 << 24, (1 << 24) + 2):
            add(nv12, srs=rs, yrs=rs), add(nv12, uvrs=rs), add(nv12, srs=rs, yrs=rs, uvrs=rs, batch=2)
        for sh, rs in ((32766, 65540), (32766, 65541), (32766, 1 << 16), (32766, 131080), (32766, 131082), (32767, 65538), (32767, 65539), (256, (1 << 24) - 2)):
            add(nv12, sh=sh, srs=rs, yrs=rs), add(nv12, sh=sh, uvrs=rs)
        # strides next to 2^63 (rows * stride does not fit 64 bits: compared exactly) and negative ones
        big = (1 << 63) - 1
        for v in (big, big - 1, 1 << 62, -1, -2, -(1 << 63)):
            for k in ("srs", "yrs", "uvrs", "dyrs", "duvrs"):
                add(nv12, **{k: v})
            for k in ("sfs", "yfs", "uvfs", "dyfs", "duvfs"):
                add(nv12, batch=2, **{k: v})
            add(nv12, uvfs=v), add(nv12, duvfs=v)   # a single frame's uv frame strides are only asked to be even
        # odd strides and bases
        for off in (0, 1, 2, 3):
            add(nv12, uv=UV0 + off), add(nv12, uvrs=8 + off), add(nv12, uvfs=32 + off)
            add(nv12, duv=DUV0 + off), add(nv12, duvrs=8 + off), add(nv12, duvfs=32 + off), add(nv12, duvfs=32 + off, batch=2)
            add(nv12, dy=DY0 + off, dyrs=8 + off, dyfs=64 + 9 * off, batch=2)   # the Y plane takes any of them (and loses the wide stores)
            add(nv12, src=S0 + off, srs=24 + off, y=Y0 + off, yrs=8 + off)
        # formats and counts
        for interp in (-1, 0, 1, 2, 3):
            for rgb in (-1, 0, 1, 2):
                add(nv12, interp=interp, rgb=rgb)
        for batch, mc in ((0, 1), (0, 0), (0, 5), (1, 0), (1, 2), (3, 1), (3, 3), (3, 2), (-1, 1)):
            add(nv12, batch=batch, mc=mc, dyfs=1 << 20, duvfs=1 << 20)
        add(nv12, src=0, y=0), add(nv12, src=0, uv=0), add(nv12, dy=0), add(nv12, duv=0)
        for k in ("sh", "sw", "dh", "dw"):
            add(nv12, **{k: 0}), add(nv12, **{k: -8})
        # overlap: either destination plane next to and on every source image
        for s, n in ((S0, 192), (Y0, 64), (UV0, 32)):
            for d in (s - 64, s - 63, s, s + n - 1, s + n):
                add(nv12, dy=d)
            for d in (s - 32, s - 30, s, s + n - 2, s + n):
                add(nv12, duv=d)
        # ... column-disjoint regions of one allocation with 64-byte rows
        for off in (23, 24, 32, 56, 57):
            add(nv12, srs=64, dyrs=64, dy=S0 + off), add(nv12, yrs=64, uvrs=64, dyrs=64, duvrs=64, uv=Y0 + 8 * 64, dy=Y0 + off, duv=Y0 + off + 8)
        # ... and the destination planes against each other: single buffers, batches of them, padded rows, planes run together
        for d in (DY0 - 32, DY0 - 30, DY0, DY0 + 2, DY0 + 62, DY0 + 64, DY0 + 66):
            add(nv12, duv=d)
            for fs in (96, 98, 128, 1 << 20):
                add(nv12, duv=d, batch=3, dyfs=fs, duvfs=fs)
            add(nv12, duv=d, batch=2)   # Y frames back to back, the pairs behind frame 0
            add(nv12, duv=d, batch=2, dyfs=96, duvfs=100)
        add(nv12, batch=3, dyrs=16, duvrs=16, duv=DY0 + 128, dyfs=192, duvfs=192), add(nv12, batch=3, dyrs=16, duvrs=16, duv=DY0 + 120, dyfs=192, duvfs=192)
        add(nv12, batch=3, dyrs=16, duvrs=16, duv=DY0 + 8, dyfs=192, duvfs=192), add(nv12, batch=3, dyrs=16, duvrs=16, duv=DY0 + 6, dyfs=192, duvfs=192)
        add(nv12, batch=2, dyfs=96, duvfs=96, duv=DY0 + 96), add(nv12, batch=2, dyfs=128, duvfs=128, duv=DY0 + 96), add(nv12, batch=2, dyfs=128, duvfs=128, duv=DY0 + 98)
    got = run_driver(driver, cases)
    for case, (want, dsts, batch, dh, dw), nums in zip(cases, expect, got):
        assert nums[0] == want, (case, nums, want)
        for k in (0, 1):   # wide stores, per plane: base and both strides multiples of 4
            assert nums[1 + k] == int(all(v % 4 == 0 for v in (dsts[k][0], dsts[k][3], dsts[k][4]))), (case, nums)
        if nums[0] == 0 and batch > 0:
            tiles = batch * (-(-dw // 256)) * (-(-dh // 4))
            if dh > 1 << 20 or dw > 1 << 20 or tiles > 0x7fffffff:
                assert nums[3] == -3, (case, nums)
            else:
                assert nums[3:] == [0, tiles], (case, nums)
    for kind in ("to_nv12", "nv12_to_nv12"):
        statuses = [n[0] for c, n in zip(cases, got) if c[0] == kind]
        assert statuses.count(0) > 60 and statuses.count(-1) > 40 and statuses.count(-2) >= 10 and statuses.count(-3) >= 10 and statuses.count(-6) >= 30, \
            (kind, [statuses.count(s) for s in (0, -1, -2, -3, -6)])
    assert any(n[3] == -3 for n in got) and any(n[1] != n[2] for n in got)
    # addresses next to the top of the address space: only the sanitizer's silence is asserted (unsigned sums wrap)
    top = (1 << 64) - 1
    cases, expect = [], []
    for nv12 in (False, True):
        add(nv12, src=top - 191, y=top - 63, uv=top - 31, dy=top - 63, duv=top - 31), add(nv12, src=top, y=top, uv=top - 1, dy=top, duv=top - 1)
        add(nv12, src=top, y=top, uv=top - 1, dy=1, duv=2, batch=2, sfs=1 << 62, yfs=1 << 62, uvfs=1 << 62, dyfs=1 << 62, duvfs=1 << 62)
        add(nv12, dy=top - 4096, duv=top - 2047, batch=65535, dyfs=big - 1, duvfs=big - 1, sfs=big, yfs=big, uvfs=big - 1, mc=65535)
        add(nv12, dy=top - 95, duv=top - 31, batch=3, dyfs=96, duvfs=96)
    assert len(run_driver(driver, cases)) == len(cases)


# ---- the compiled kernels ---------------------------------------------------------------------------------------------------------------
def test_nv12_out_kernels_code_object(tmp_path):
    unit = codeobj.kernels("warp_nv12_out.hip", tmp_path, header="warp_nv12_out.h")
    kernels = {n: k for n, k in unit.items() if "warp_nv12_out_kernel" in n}
    assert len(kernels) == len(unit) == 2 * 2 + 2, sorted(unit)  # BGR source: interpolation x channel order; NV12 source: interpolation; nothing else
    codeobj.assert_lean(kernels)
    codeobj.makefile_flags("warp_nv12_out.hip", "nv12_out.h")  # (the conversion's header rebuilds the unit too)
