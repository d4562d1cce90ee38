"""NV12 frames warped straight to channel planes (bevwarp_warp_nv12_planes, warp_nv12_to_planar) without a device: the symbol, the entry
point's argument validation with pointers that are never dereferenced (one case per status, in the documented order), the Python layer's
argument errors, host_plan.h's checks of an nv12_planes_call at their limits in a stand-alone driver under the address and undefined-behaviour
sanitizers (tests/host_plan_driver.cpp) against an exact-integer model, and the compiled kernels' register, scratch and LDS
figures."""
import ctypes
import os
import re
import numpy as np
import pytest
import torch

from bev_amd import _lib
from tests import codeobj
from tests import hostplan
from tests.test_abi import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "bevwarp_warp_nv12_planes"
ELEM = {_lib.F32: 4, _lib.F16: 2, _lib.BF16: 2}  # bytes of a plane element; any other plane type: 1 (no alignment is asked of it)


@pytest.fixture(scope="module")
def lib():
    return hostplan.built_lib()


# ---- the ABI without a device -------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_bound(lib):
    assert NAME in declared_symbols() and NAME in _lib.SYMBOLS
    assert getattr(ctypes.CDLL(_lib.LIB_PATH), NAME) is not None
    assert len(_lib.SYMBOLS[NAME][1]) == 24
    assert lib.bevwarp_version() == _lib.ABI_VERSION == 7
    with open(os.path.join(ROOT, "include", "bevwarp.h")) as f:
        text = f.read()
    assert "#define BEVWARP_ABI_VERSION 7" in text
    decl = text[text.index("int " + NAME):]
    decl = decl[:decl.index(";")]
    assert decl.count("int64_t") == 7 and "dst_plane_stride" in decl and "plane_dtype" in decl and "rgb_order" in decl
    from bev import warp as dropin
    from bev_amd import warp
    assert dropin.warp_nv12_to_planar is warp.warp_nv12_to_planar


def test_argument_validation_without_a_device(lib):
    fn = getattr(lib, NAME)
    P = ctypes.c_void_p
    vec = lambda *v: ctypes.cast((ctypes.c_double * 3)(*v), P)  # noqa: E731
    nan_border = vec(1.0, float("nan"), 1.0)
    # an 8 x 8 frame: Y 64 bytes at 4096, four rows of four pairs at 8192, three 8 x 8 float16 planes far behind them (rows 16 bytes,
    # planes 128, frames 384); never dereferenced
    # index: 0 y  1 uv  2 dst  3 batch 4 sh 5 sw 6 dh 7 dw 8 yfs 9 yrs 10 uvfs 11 uvrs 12 dfs 13 dps 14 drs 15 M 16 mc 17 interp 18 rgb 19 border 20 scale 21 bias
    #        22 plane_dtype 23 stream
    ok = [P(4096), P(8192), P(1 << 40), 1, 8, 8, 8, 8, 64, 8, 32, 8, 384, 128, 16, P(16), 1, 1, 0, nan_border, None, None, _lib.F16, None]

    def call(**patch):
        a = list(ok)
        for k, v in patch.items():
            a[int(k[1:])] = v
        return fn(*a)

    assert call() == -4                                # otherwise valid: refused on the border value alone, before any launch
    assert call(a3=0) == 0 and call(a3=0, a19=None) == 0   # an empty batch is a no-op
    for pd in (_lib.F16, _lib.BF16):
        assert call(a22=pd) == -4
    f32 = dict(a22=_lib.F32, a14=32, a13=256, a12=768)
    assert call(**f32) == -4
    # 1. BEVWARP_ERR_BAD_ARG
    for k in (0, 1, 2, 15):
        assert call(**{"a%d" % k: None}) == -1         # null pointers
    for k in (4, 5, 6, 7):
        assert call(**{"a%d" % k: 0}) == -1 and call(**{"a%d" % k: -2}) == -1
    assert call(a3=-1) == -1
    assert call(a4=7) == -1 and call(a5=7) == -1       # odd source sides
    assert call(a9=7) == -1 and call(a11=7) == -1 and call(a11=6) == -1    # source row strides below src_w, either plane
    assert call(a1=P(8193)) == -1 and call(a11=9) == -1 and call(a10=33) == -1   # odd uv base, row stride, frame stride
    assert call(a3=2, a10=30) == -1 and call(a3=2, a8=63) == -1              # source frames that overlap their successors
    assert call(a14=17) == -1 and call(a13=129) == -1 and call(a12=385) == -1 and call(a2=P((1 << 40) + 1)) == -1   # not multiples of 2 bytes
    assert call(**dict(f32, a14=34)) == -1 and call(**dict(f32, a13=258)) == -1 and call(**dict(f32, a12=770)) == -1 and call(**dict(f32, a2=P((1 << 40) + 2))) == -1
    assert call(a14=14) == -1 and call(**dict(f32, a14=28)) == -1            # a row stride below dst_w elements
    assert call(a13=126) == -1 and call(a13=112) == -1                        # planes that overlap their successors (asked of ... a lone frame too)
    assert call(a3=2, a12=382) == -1 and call(a3=2, a12=384) == -4           # frames that overlap their successors
    assert call(a14=18, a13=144, a12=432) == -4                               # multiples of 2 only (no wide stores) are accepted
    assert call(a16=2) == -1 and call(a16=0) == -1 and call(a3=3, a12=384, a8=64, a10=32, a16=2) == -1   # m_count not 1 or batch
    assert call(a16=2, a17=2) == -1 and call(a14=14, a22=_lib.F32) == -1     # bad arguments come before unsupported ones ...
    assert call(a14=14, a22=7) == -2 and call(a14=7, a22=7) == -1            # (an unknown plane type: elements of one byte, then refused)
    # 2. BEVWARP_ERR_UNSUPPORTED
    for interp in (2, 3, -1, 7):
        assert call(a17=interp) == -2
    for order in (2, -1, 91):
        assert call(a18=order) == -2
    for pd in (_lib.U8, _lib.F64, 5, -1):
        assert call(a22=pd) == -2
    assert call(a17=0) == -4 and call(a18=1) == -4
    assert call(a17=2, a5=32768, a9=32768, a11=32768) == -2    # ... before the size limits
    # 3. BEVWARP_ERR_TOO_LARGE, per source plane
    assert call(a5=32768, a9=32768, a11=32768) == -3 and call(a4=32768) == -3
    assert call(a9=1 << 24) == -3 and call(a9=(1 << 24) - 1) == -4
    assert call(a11=1 << 24) == -3 and call(a11=(1 << 24) - 2) == -4
    assert call(a4=32766, a9=65541) == -3 and call(a4=32766, a9=65540) == -4
    assert call(a5=32768, a9=32768, a11=32768, a2=P(4096)) == -3   # ... before overlap
    # 4. BEVWARP_ERR_OVERLAP: the bounding byte range of all three planes (384 bytes) against the Y image and against the UV image
    assert call(a2=P(4096 + 62)) == -6 and call(a2=P(4096 + 64)) == -4 and call(a2=P(4096 - 384)) == -4 and call(a2=P(4096 - 382)) == -6
    assert call(a2=P(8192 + 30)) == -6 and call(a2=P(8192 + 32)) == -4 and call(a2=P(8192 - 384)) == -4 and call(a2=P(8192 - 382)) == -6
    assert call(a2=P(4096 - 382), a19=None) == -6
    assert call(a2=P(4096), a6=(1 << 20) + 1, a13=16 * ((1 << 20) + 1)) == -6   # ... before the launch plan's limit
    # 5. BEVWARP_ERR_TOO_LARGE from the launch plan
    assert call(a6=(1 << 20) + 1, a13=16 * ((1 << 20) + 1)) == -3 and call(a7=(1 << 20) + 1, a14=2 * ((1 << 20) + 2), a13=16 * ((1 << 20) + 2)) == -3
    assert call(a6=(1 << 20) + 1, a13=16 * ((1 << 20) + 1), a20=vec(1.0, float("inf"), 1.0)) == -3   # ... before the constants are looked at
    # 6. BEVWARP_ERR_NOT_FINITE: each of the three arrays, each of their values
    good = vec(1.0, 2.0, 3.0)
    for slot in (19, 20, 21):
        for i in range(3):
            v = [1.0, 2.0, 3.0]
            v[i] = float("inf") if i else float("nan")
            assert call(**{"a19": good, "a%d" % slot: vec(*v)}) == -4


class _ClaimsCuda(torch.Tensor):
    """A host tensor that answers is_cuda: the shape checks run without a device (nothing after them is reached)."""
    is_cuda = property(lambda self: True)


def test_python_argument_errors_without_a_device():
    from bev_amd import warp
    from bev_amd.pipeline import FramePipeline
    f = warp.warp_nv12_to_planar
    y, uv = torch.zeros((8, 8), dtype=torch.uint8), torch.zeros((4, 4, 2), dtype=torch.uint8)
    with pytest.raises(ValueError, match="CUDA"):
        f(y, uv, np.eye(3), (8, 8))
    with pytest.raises(ValueError, match="CUDA"):
        f(y.numpy(), uv.numpy(), np.eye(3), (8, 8))
    with pytest.raises(ValueError, match="interpolation"):
        f(y, uv, np.eye(3), (8, 8), flags=warp.INTER_CUBIC)
    with pytest.raises(ValueError, match="out_dtype"):
        f(y, uv, np.eye(3), (8, 8), out_dtype=torch.float64)
    with pytest.raises(ValueError, match="out_dtype"):
        f(y, uv, np.eye(3), (8, 8), out_dtype=torch.uint8)
    with pytest.raises(ValueError, match="out must be"):
        f(y, uv, np.eye(3), (8, 8), out_dtype=torch.float16, out=torch.zeros((3, 8, 8), dtype=torch.float32))
    with pytest.raises(ValueError, match="out must be"):
        f(y, uv, np.eye(3), (8, 8), out=torch.zeros((3, 8, 8), dtype=torch.bfloat16))
    fake = lambda *shape: torch.zeros(shape, dtype=torch.uint8).as_subclass(_ClaimsCuda)  # noqa: E731
    assert fake(2, 2).is_cuda
    for ys, uvs in (((7, 8), (3, 4, 2)), ((8, 6 + 1), (4, 3, 2)), ((2, 7, 8), (2, 3, 4, 2))):   # odd sides
        with pytest.raises(ValueError, match="even sides"):
            f(fake(*ys), fake(*uvs), np.eye(3), (8, 8))
    for ys, uvs in (((8, 8), (4, 4, 3)), ((8, 8), (8, 4, 2)), ((8, 8), (4, 8, 2)), ((2, 8, 8), (1, 4, 4, 2))):   # a wrong uv shape
        with pytest.raises(ValueError, match="uv of shape"):
            f(fake(*ys), fake(*uvs), np.eye(3), (8, 8))
    for ys, uvs in (((8, 8), (4, 8)), ((8,), (4, 2)), ((2, 8, 8), (4, 4, 2))):   # ... of the wrong rank
        with pytest.raises(ValueError, match="y must be"):
            f(fake(*ys), fake(*uvs), np.eye(3), (8, 8))
    with pytest.raises(ValueError, match="contiguous"):
        f(fake(8, 16)[:, ::2], fake(4, 4, 2), np.eye(3), (8, 8))
    # the pipeline keeps refusing NV12 slots with planar results: streaming callers use warp_nv12_to_planar(out=, M_inv_device=)
    with pytest.raises(ValueError, match="planar"):
        FramePipeline((8, 8), 3, np.eye(3), (8, 8), src_format="nv12", planar=True)
    assert "FramePipeline" in f.__doc__ and "M_inv_device" in f.__doc__


# ---- host_plan.h's checks of an nv12_planes_call under the sanitizers ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver():
    return hostplan.build_driver()


def run_driver(exe, cases):
    return hostplan.run_driver(exe, ["nv12p " + " ".join(str(int(v)) for v in c) for c in cases], "plan")


def model(y, uv, dst, batch, sh, sw, dh, dw, yfs, yrs, uvfs, uvrs, dfs, dps, drs, mc, interp, rgb, pd):
    """check_warp_nv12_planes restated in exact integers (no case given to it wraps an address): (status, wide stores admitted)."""
    e = ELEM.get(pd, 1)
    wide = int(all(v % (4 * e) == 0 for v in (dst, dfs, dps, drs)))

    def status():
        if not y or not uv or not dst:
            return -1
        if batch < 0 or min(sh, sw, dh, dw) <= 0 or sh % 2 or sw % 2:
            return -1
        sources = ((y, sh, sw, yrs, yfs, 1), (uv, sh // 2, sw, uvrs, uvfs, 2))
        for base, rows, row_bytes, rs, fs, elem in sources:
            if rs < row_bytes or (batch > 1 and fs < rows * rs) or rs % elem or fs % elem or base % elem:
                return -1
        row = dw * e
        if drs < row or dps < dh * drs or (batch > 1 and dfs < 3 * dps) or any(v % e for v in (dst, drs, dps, dfs)):
            return -1
        if mc != 1 and mc != batch:
            return -1
        if interp not in (0, 1) or rgb not in (0, 1) or pd not in ELEM:
            return -2
        for (base, rows, row_bytes, rs, fs, elem), cols in zip(sources, (sw, sw // 2)):
            if cols > 32767 or rows > 32767 or rs >= 1 << 24 or rows * rs >= 1 << 31:
                return -3
        if batch == 0:
            return 0
        d_end = dst + (batch - 1) * dfs + 2 * dps + (dh - 1) * drs + row
        for base, rows, row_bytes, rs, fs, elem in sources:
            if base < d_end and dst < base + (batch - 1) * fs + (rows - 1) * rs + row_bytes:
                return -6
        return 0

    return status(), wide


def test_check_warp_nv12_planes_at_its_limits_under_the_sanitizer(driver):
    Y0, UV0, D0 = 1 << 32, 1 << 36, 1 << 40
    cases = []

    def add(y=Y0, uv=UV0, dst=D0, batch=1, sh=8, sw=8, dh=8, dw=8, yfs=None, yrs=None, uvfs=None, uvrs=None, dfs=None, dps=None, drs=None, mc=1, interp=1, rgb=0,
            pd=_lib.F16):
        e = ELEM.get(pd, 1)
        yrs = sw if yrs is None else yrs
        uvrs = sw if uvrs is None else uvrs
        drs = e * dw if drs is None else drs
        tight = lambda rows, rs: rows * rs if abs(rows * rs) < 1 << 61 else 0  # noqa: E731  (images back to back, where that is a 64-bit number)
        dps = tight(dh, drs) if dps is None else dps
        cases.append((y, uv, dst, batch, sh, sw, dh, dw, tight(sh, yrs) if yfs is None else yfs, yrs, tight(sh // 2, uvrs) if uvfs is None else uvfs, uvrs,
                      tight(3, dps) if dfs is None else dfs, dps, drs, mc, interp, rgb, pd))

    PDS = (_lib.F32, _lib.F16, _lib.BF16)
    # source sides: the largest even side, the first refused one, and odd ones around them
    for side in (2, 32765, 32766, 32767, 32768, 65536, (1 << 31) - 2):
        add(sw=side), add(sh=side, yrs=8), add(sh=side, sw=side)
    # source row strides next to 2^24, per plane, and planes next to 2 GiB
    for rs in ((1 << 24) - 2, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 24) + 2):
        add(yrs=rs), add(uvrs=rs), add(yrs=rs, uvrs=rs, batch=2)
    for sh, rs in ((32766, 65540), (32766, 65541), (32766, 1 << 16), (32766, 131080), (32766, 131082), (32766, 131084), (128, (1 << 24) - 1), (256, (1 << 24) - 2)):
        add(sh=sh, yrs=rs), add(sh=sh, uvrs=rs)
    # strides next to 2^63 (rows * stride does not fit 64 bits: compared exactly) and negative ones, every stride of the call
    big = (1 << 63) - 1
    for v in (big, big - 1, big - 3, 1 << 62, (1 << 62) + 4, -1, -2, -4, -16, -(1 << 63)):
        add(yrs=v), add(uvrs=v), add(yfs=v, batch=2), add(uvfs=v, batch=2), add(uvfs=v)
        for pd in PDS:
            add(drs=v, pd=pd), add(dps=v, pd=pd), add(dfs=v, pd=pd), add(dfs=v, batch=2, pd=pd), add(dps=v, dfs=v, batch=2, pd=pd)
    # planes next to 2 GiB and beyond (the destination has no such limit), rows of 2^20 elements
    for pd in PDS:
        e = ELEM[pd]
        for dh, drs in ((1 << 15, 1 << 16), ((1 << 15) + 1, 1 << 16), (1 << 20, 4096), (3, (1 << 31) - 4), (3, 1 << 31), (3, (1 << 31) + 4)):
            add(dh=dh, dw=8, drs=drs, pd=pd), add(dh=dh, dw=8, drs=drs, pd=pd, batch=3, mc=3)
        # destinations at the launch plan's limit
        add(dw=1 << 20, dh=1, pd=pd), add(dw=(1 << 20) + 1, dh=1, pd=pd), add(dh=1 << 20, dw=1, pd=pd), add(dh=(1 << 20) + 1, dw=1, pd=pd)
        add(dw=1 << 20, dh=1 << 20, batch=3, mc=3, pd=pd), add(dw=(1 << 20) + 1, dh=(1 << 20) + 1, pd=pd)
        add(dw=1 << 20, dh=2, drs=(e << 20) - e, pd=pd), add(dw=1 << 20, dh=2, drs=(e << 20) + e, pd=pd)
        # element-size misalignment, of the base and of each stride, one at a time and all together; what the wide stores ask for as well
        for off in (0, 1, 2, 3, 4, 6, 8, 12, 16):
            for which in range(5):
                d = [D0, 64 * 80 * e, 16 * 80 * e, 80 * e]  # base, frame, plane, row: 9 rows of 70 elements
                if which < 4:
                    d[which] += off
                else:
                    d = [v + off for v in d]
                add(dst=d[0], dfs=d[1], dps=d[2], drs=d[3], dh=9, dw=70, batch=2, mc=2, pd=pd)
        # rows, planes and frames that just hold their contents, and one element less
        for drs, dps, dfs in ((8 * e, 64 * e, 192 * e), (7 * e, 64 * e, 192 * e), (8 * e, 63 * e, 192 * e), (8 * e, 64 * e, 191 * e), (8 * e, 64 * e, 128 * e + 63 * e)):
            add(drs=drs, dps=dps, dfs=dfs, batch=2, pd=pd), add(drs=drs, dps=dps, dfs=dfs, pd=pd)
    # odd uv strides and bases (the Y plane takes any)
    for off in (0, 1, 2, 3):
        add(uv=UV0 + off), add(uvrs=8 + off), add(uvfs=32 + off, batch=2), add(uvfs=32 + off)
        add(yrs=8 + off, y=Y0 + off, yfs=64 + 8 * off + off, batch=2)
    # formats and counts; a plane type outside the three asks no alignment and is refused after the layout
    for interp in (-1, 0, 1, 2, 3):
        for rgb in (-1, 0, 1, 2):
            add(interp=interp, rgb=rgb)
    for pd in (-1, 0, 1, 2, 3, 4, 5, 77):
        add(pd=pd), add(pd=pd, interp=2), add(pd=pd, drs=9, dps=73, dfs=221), add(pd=pd, sw=32768), add(pd=pd, drs=7)
    for batch, mc in ((0, 1), (0, 0), (0, 5), (1, 0), (1, 2), (3, 1), (3, 3), (3, 2), (-1, 1)):
        add(batch=batch, mc=mc)
    add(y=0), add(uv=0), add(dst=0)
    for k in ("sh", "sw", "dh", "dw"):
        add(**{k: 0}), add(**{k: -8})
    # overlap: the planes' bounding range (3 x 128 bytes; batches: 2 frames) next to and on either source image
    for d in (Y0 - 384, Y0 - 382, Y0, Y0 + 62, Y0 + 64, UV0 - 384, UV0 - 382, UV0 + 30, UV0 + 32):
        add(dst=d), add(dst=d, y=Y0, uv=Y0 + 64)
        add(dst=d - 384, batch=2, mc=2), add(dst=d, batch=2, mc=1, dfs=768)
    add(dst=Y0 - 768, pd=_lib.F32), add(dst=Y0 - 764, pd=_lib.F32)
    add(batch=3, yfs=1 << 20, uvfs=1 << 20, dfs=1 << 20, dst=Y0 + (1 << 19)), add(batch=3, yfs=1 << 20, uvfs=1 << 20, dfs=1 << 20, dst=Y0 + (2 << 20) + 62)
    got = run_driver(driver, cases)
    for case, nums in zip(cases, got):
        st, wide = model(*case)
        assert nums[0] == st and nums[1] == wide, (case, nums, st, wide)
        if st == 0 and case[3] > 0:
            dh, dw = case[6], case[7]
            if dh > 1 << 20 or dw > 1 << 20 or case[3] * (-(-dw // 256)) * (-(-dh // 4)) > 0x7fffffff:
                assert nums[2] == -3, (case, nums)
            else:
                assert nums[2:] == [0, case[3] * (-(-dw // 256)) * (-(-dh // 4))], (case, nums)
    statuses = [n[0] for n in got]
    assert statuses.count(0) > 60 and statuses.count(-1) > 100 and statuses.count(-2) >= 20 and statuses.count(-3) >= 15 and statuses.count(-6) >= 10, \
        [statuses.count(v) for v in (0, -1, -2, -3, -6)]
    assert sum(n[2] == -3 for n in got) >= 6
    for pd in PDS:  # each plane type is refused for its own misalignment, and both wide-store verdicts occur among its accepted cases
        mine = [(c, n) for c, n in zip(cases, got) if c[18] == pd and c[6:8] == (9, 70)]
        assert {n[0] for c, n in mine} == {0, -1} and {n[1] for c, n in mine if n[0] == 0} == {0, 1}, pd
    # addresses next to the top of the address space: only the sanitizer's silence is asserted (unsigned sums wrap)
    top = (1 << 64) - 1
    wrap = []
    cases = wrap
    add(y=top - 63, uv=top - 31, dst=top - 383), add(y=top - 1, uv=top - 1, dst=top - 1), add(y=top, uv=top - 1, dst=2, batch=2, yfs=1 << 62, uvfs=1 << 62, dfs=1 << 62)
    add(y=top - 4096, uv=top - 2048, dst=8, batch=65535, yfs=big - 1, uvfs=big - 1, dfs=big - 1, dps=1 << 60, mc=65535), add(sh=32766, sw=32766, y=top - 1, uv=top - 1, dst=top - 1)
    add(dst=top - 1, dps=1 << 62, dfs=big - 1, batch=2, pd=_lib.F32), add(dst=top - 3, dps=(1 << 63) - 4, pd=_lib.F32)
    assert len(run_driver(driver, wrap)) == len(wrap)


# ---- the compiled kernels ---------------------------------------------------------------------------------------------------------------
def test_nv12_planes_kernels_code_object(tmp_path):
    kernels = codeobj.kernels("warp_nv12_planes.hip", tmp_path, header="nv12_sample.h")
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        stated = re.search(r"warp_nv12_planes\.hip[^\n]*?\b(\d+) kernels", f.read())
    assert stated and len(kernels) == int(stated.group(1)) == 2 * 2, (sorted(kernels), stated)  # interpolation x (float32 | 16-bit planes)
    assert all("nv12_planes_kernel" in n and "warp_nv12_kernel" not in n for n in kernels), sorted(kernels)
    codeobj.assert_lean(kernels)
