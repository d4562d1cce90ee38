"""Every kernel at the largest sizes and strides the C ABI admits (include/bevwarp.h, bev_amd/csrc/host_plan.h): source sides of 32767 px,
row strides just below 16 MiB with frames just below 2 GiB, frame / plane strides and in-frame destination offsets beyond 2^32 bytes, item
counts on either side of fast_div's exactness bound, grid dimensions of 65535.  tests/test_abi.py and tests/test_host_plan.py pin the host
checks that admit these calls; here the kernels run them.

The large shapes are large only in stride: views of one device buffer filled with a canary on the device, the few real rows or frames
copied in through the view, the oracle fed the compact copy, and the destination's canaries checked by reductions on the device.  Shapes,
strides and matrices live in tests/limits_cases.py, which tests/test_limits_cpu.py checks on the CPU (the oracle against its numpy
restatement on the same shapes, every layout against its buffer, the 24-bit tap address against the plain product).

Memory: the cases beyond 4 GiB hold one buffer of 4.1 to 8.6 GiB (three frames 2^32 + 4096 bytes apart cannot take less), the stride
cases one of 2 GiB; each is dropped in a `finally`."""
import os
import subprocess

import numpy as np
import pytest
import torch

from bev_amd import _lib, warp as W
from oracle import cpu_oracle as co
from tests import border_ref as br
from tests import hostplan
from tests import cubic_ref as cr
from tests import limits_cases as lc
from tests import pixels as px
from tests import planes16_ref as p16
from tests import workloads as wl
from tests.limits_buffers import assert_only_the_view_was_written, byte_holder, nan_holder, per_frame, same, strided
from tests.parity import check_modes, poisoned_out, report_comparisons, warp_modes  # noqa: F401  (report_comparisons: a module fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = W.WARP_INVERSE_MAP
TOO_LARGE = -3
SCALE, BIAS = [1 / 255.0, 0.5, 2.0, 1.0], [0.0, -1.0, 3.5, 0.25]


# ---- expected values (the buffer helpers live in tests/limits_buffers.py) --------------------------------------------------------------------
def run_both_interps(t, src, Minv, dsize, out=None):
    """bevwarp_warp, nearest and bilinear, in both launch modes, against the oracle.  Returns the bilinear expectation."""
    c = src.shape[-1]
    for interp in (W.INTER_NEAREST, W.INTER_LINEAR):
        exp = per_frame(lambda f, M: co.warp_perspective(f, M, dsize, interp, m_is_inverse=True, border_value=lc.BORDER[:c]), src, Minv)
        o = poisoned_out(t, dsize) if out is None else out
        if out is not None:
            out.fill_(77)
        check_modes(warp_modes(t, Minv, dsize, flags=interp | INV, border_value=lc.BORDER[:c], out=o), exp, same)
    return exp


def run_other_kernels(t, src, Minv, dsize, out=None, planes_out=None):
    """One configuration each of the border kernel (REPLICATE and REFLECT_101, bilinear), the bicubic kernel with the constant border, and
    warp_to_planar to float32 and to float16 planes, on the same source and map.  `out` / `planes_out(dtype)`: strided destinations."""
    c = src.shape[-1]
    for mode in (br.REPLICATE, br.REFLECT_101):
        exp = per_frame(lambda f, M: br.warp(f, M, dsize, br.LINEAR, mode, m_is_inverse=True), src, Minv)
        got = W.warp_perspective(t, Minv, dsize, flags=W.INTER_LINEAR | INV, border_mode=mode, out=out)
        same(got.cpu().numpy(), exp)
    exp = per_frame(lambda f, M: cr.warp(f, M, dsize, br.CONSTANT, m_is_inverse=True, border_value=lc.BORDER[:c]), src, Minv)
    got = W.warp_perspective(t, Minv, dsize, flags=W.INTER_CUBIC | INV, border_value=lc.BORDER[:c], out=out)
    same(got.cpu().numpy(), exp)
    # (planes16_ref takes forward matrices: both sides invert the same one with the same closed form)
    fwd = np.linalg.inv(Minv)
    planes = per_frame(lambda f, M: p16.planes_f32(f, M, dsize, co.LINEAR, SCALE[:c], BIAS[:c], border_value=lc.BORDER[:c]), src, fwd)
    for dtype in (torch.float32, torch.float16):
        got = W.warp_to_planar(t, fwd, dsize, scale=SCALE[:c], bias=BIAS[:c], border_value=lc.BORDER[:c], out_dtype=dtype,
                               out=None if planes_out is None else planes_out(dtype))
        if dtype == torch.float32:
            px.same_float(got.cpu().numpy(), planes)
        else:
            p16.assert_same16(p16.gpu_bits(got), p16.to_bits(planes, dtype), dtype)


def tile_kinds(t, Minv, dsize, interp):
    """{"in", "out", "cut"}: the verdicts the table-mode launch of this call filled (coverage of the case, not an expected value)."""
    minv = W.device_inverse(Minv, t.device, inverse_given=True)
    h, w, c = t.shape[-3:]
    key = (minv.data_ptr(), minv.shape[0], 1 if t.dim() == 3 else t.shape[0], h, w, int(dsize[1]), int(dsize[0]), c, W._DTYPES[t.dtype], interp)
    f = W._class_tables[key][0].cpu().numpy().view(np.uint32)
    f = f[(f >> 31) != 0]
    return {"in" if v & 1 else ("out" if v & 2 else "cut") for v in f.tolist()}


# ---- A, B: the widest and the tallest source --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,c", lc.WIDE_FORMATS, ids=lambda v: getattr(v, "__name__", str(v)))
@pytest.mark.parametrize("key", sorted(lc.WIDE_MAPS))
@pytest.mark.parametrize("name", ["wide", "tall"])
def test_widest_and_tallest_source(name, key, dtype, c):
    """Cases A and B: a side of 32767 px.  `right_end` parks the destination on the source's far end (tiles inside the frame, cut by its
    edge and beyond it -- asserted from the verdict table), `minify64` runs over the whole side."""
    (h, w), dsize, maps = (lc.WIDE_HW, lc.WIDE_DSIZE, lc.WIDE_MAPS) if name == "wide" else (lc.TALL_HW, lc.TALL_DSIZE, lc.TALL_MAPS)
    Minv = maps[key]
    src = lc.pixels(11, h, w, c, dtype)
    t = torch.from_numpy(src).cuda()
    exp = run_both_interps(t, src, Minv, dsize)
    border = (exp == per_channel_border(exp.dtype, c)).all(-1)
    assert border.any() and not border.all()  # border pixels and pixels of the frame
    for interp in (co.NEAREST, co.LINEAR):
        sxy, _ = co.warp_maps(dsize, Minv, interp)
        s = sxy[..., 0] if name == "wide" else sxy[..., 1]
        assert (s == lc.MAX_SIDE - 2).any() and (s == 32767).any()  # the last index with two valid taps, and the saturated one
    if key == "right_end":
        assert tile_kinds(t, Minv, dsize, W.INTER_LINEAR) == {"in", "out", "cut"}
    else:
        assert "in" in tile_kinds(t, Minv, dsize, W.INTER_LINEAR)
    if (np.dtype(dtype), c) in ((np.dtype(np.uint8), 3), (np.dtype(np.float32), 1)):
        run_other_kernels(t, src, Minv, dsize)


def per_channel_border(dtype, c):
    return np.asarray(lc.BORDER[:c], dtype=dtype)


# ---- C: the largest row stride -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,c,rs", lc.STRIDE_FORMATS, ids=lambda v: getattr(v, "__name__", str(v)))
def test_largest_row_stride(dtype, c, rs):
    """Case C: rows 2^24 - 16 (aligned) or 2^24 - 1 (odd) bytes apart, as many as rows * stride < 2^31 admits; the map reads them from the
    first to the last.  One row more, or a stride of 2^24, is BEVWARP_ERR_TOO_LARGE."""
    esz, rows = np.dtype(dtype).itemsize, lc.max_rows(rs)
    assert rows * rs < lc.FRAME_LIMIT <= (rows + 1) * rs
    src = lc.pixels(12, rows, lc.STRIDE_W, c, dtype)
    Minv = lc.stride_map(rows)
    holder = view = None
    try:
        holder = (byte_holder if dtype == np.uint8 else nan_holder)(lc.source_reach(rows, lc.STRIDE_W, c, esz, rs))
        view = strided(holder, dtype, (rows, lc.STRIDE_W, c), (rs, c * esz, esz))
        view.copy_(torch.from_numpy(src).cuda())
        run_both_interps(view, src, Minv, lc.STRIDE_DSIZE)
        assert "in" in tile_kinds(view, Minv, lc.STRIDE_DSIZE, W.INTER_LINEAR)
        if (np.dtype(dtype), c) in ((np.dtype(np.uint8), 3), (np.dtype(np.float32), 1)):
            run_other_kernels(view, src, Minv, lc.STRIDE_DSIZE)
        # one past either limit: refused before anything is launched
        lib, minv = _lib.load(), W.device_inverse(Minv, view.device, inverse_given=True)
        out = poisoned_out(view, lc.STRIDE_DSIZE)
        dw, dh = lc.STRIDE_DSIZE

        def status(n_rows, stride):
            return lib.bevwarp_warp(view.data_ptr(), out.data_ptr(), 1, n_rows, lc.STRIDE_W, dh, dw, c, 0, stride, 0, dw * c * esz, minv.data_ptr(), 1,
                                    W._DTYPES[view.dtype], 1, None, None)
        assert status(rows + 1, rs) == TOO_LARGE
        assert status(rows - 1, lc.ROW_LIMIT) == TOO_LARGE and (rows - 1) * lc.ROW_LIMIT < lc.FRAME_LIMIT
        torch.cuda.synchronize()
        assert bool((out == 77).all().item())
    finally:
        del holder, view
        torch.cuda.empty_cache()


# ---- D: frames, planes and matrices beyond 4 GiB -----------------------------------------------------------------------------------------------
def big_batch(dtype, c):
    h, w = lc.BIG_SRC_HW
    src = np.stack([lc.pixels(20 + i, h, w, c, dtype) for i in range(lc.BIG_BATCH)])
    return src, np.stack([lc.jittered_inverse(lc.big_map(), i) for i in range(lc.BIG_BATCH)])


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["uint8", "float32"])
def test_source_frames_beyond_4gib(dtype):
    """Case D: three source frames 2^32 + 4096 bytes apart, a matrix per frame, a compact destination."""
    c, esz = 3, np.dtype(dtype).itemsize
    src, Ms = big_batch(dtype, c)
    B, h, w, _ = src.shape
    holder = view = None
    try:
        holder = (byte_holder if dtype == np.uint8 else nan_holder)(lc.source_reach(h, w, c, esz, w * c * esz, B, lc.BEYOND_4G))
        view = strided(holder, dtype, (B, h, w, c), (lc.BEYOND_4G, w * c * esz, c * esz, esz))
        view.copy_(torch.from_numpy(src).cuda())
        assert view[2].data_ptr() - view.data_ptr() == 2 * lc.BEYOND_4G
        run_both_interps(view, src, Ms, lc.BIG_DSIZE)
        run_other_kernels(view, src, Ms, lc.BIG_DSIZE)
    finally:
        del holder, view
        torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["uint8", "float32"])
def test_destination_frames_beyond_4gib(dtype):
    """Case D reversed: compact source frames, destination frames 2^32 + 4096 bytes apart; nothing but the three frames is written."""
    c, esz = 3, np.dtype(dtype).itemsize
    src, Ms = big_batch(dtype, c)
    dw, dh = lc.BIG_DSIZE
    t = torch.from_numpy(src).cuda()
    holder = out = None
    try:
        holder = byte_holder(lc.dest_reach(dh, dw, c, esz, dw * c * esz, lc.BIG_BATCH, lc.BEYOND_4G))
        out = strided(holder, dtype, (lc.BIG_BATCH, dh, dw, c), (lc.BEYOND_4G, dw * c * esz, c * esz, esz))
        run_both_interps(t, src, Ms, lc.BIG_DSIZE, out=out)
        for mode in (br.REPLICATE, br.REFLECT_101):  # the border kernel's and the bicubic kernel's frame terms
            exp = per_frame(lambda f, M: br.warp(f, M, lc.BIG_DSIZE, br.LINEAR, mode, m_is_inverse=True), src, Ms)
            same(W.warp_perspective(t, Ms, lc.BIG_DSIZE, flags=W.INTER_LINEAR | INV, border_mode=mode, out=out).cpu().numpy(), exp)
        exp = per_frame(lambda f, M: cr.warp(f, M, lc.BIG_DSIZE, br.CONSTANT, m_is_inverse=True, border_value=lc.BORDER[:c]), src, Ms)
        same(W.warp_perspective(t, Ms, lc.BIG_DSIZE, flags=W.INTER_CUBIC | INV, border_value=lc.BORDER[:c], out=out).cpu().numpy(), exp)
        assert_only_the_view_was_written(holder, out, "destination frames beyond 4 GiB")
    finally:
        del holder, out
        torch.cuda.empty_cache()


@pytest.mark.parametrize("plane_dtype", [torch.float32, torch.float16], ids=["float32", "float16"])
def test_planes_beyond_4gib(plane_dtype):
    """Case D, planar: two channel planes 2^32 + 4096 bytes apart."""
    c = 2
    h, w = lc.BIG_SRC_HW
    dw, dh = lc.BIG_DSIZE
    src = lc.pixels(30, h, w, c, np.uint8)
    fwd = np.linalg.inv(lc.big_map())
    t = torch.from_numpy(src).cuda()
    esz = 4 if plane_dtype == torch.float32 else 2
    holder = out = None
    try:
        holder = byte_holder(lc.dest_reach(dh, dw, c, esz, dw * esz, planes=c, ps=lc.BEYOND_4G))
        out = strided(holder, plane_dtype, (c, dh, dw), (lc.BEYOND_4G, dw * esz, esz))
        for interp in (W.INTER_NEAREST, W.INTER_LINEAR):
            planes = p16.planes_f32(src, fwd, lc.BIG_DSIZE, interp, SCALE[:c], BIAS[:c], border_value=lc.BORDER[:c])
            got = W.warp_to_planar(t, fwd, lc.BIG_DSIZE, scale=SCALE[:c], bias=BIAS[:c], flags=interp, border_value=lc.BORDER[:c], out=out, out_dtype=plane_dtype)
            assert got is out
            if plane_dtype == torch.float32:
                px.same_float(out.cpu().numpy(), planes)
            else:
                p16.assert_same16(p16.gpu_bits(out), p16.to_bits(planes, plane_dtype), plane_dtype)
        assert_only_the_view_was_written(holder, out, "planes beyond 4 GiB")
    finally:
        del holder, out
        torch.cuda.empty_cache()


# ---- E: destination rows beyond 4 GiB inside one frame -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,c", [(np.uint8, 3), (np.float32, 1)], ids=["uint8x3", "float32x1"])
def test_destination_rows_beyond_4gib(dtype, c):
    """Case E, interleaved: destination rows 2^26 bytes apart, the last one beyond 4.5 GiB; the stretch after every row keeps its canaries."""
    esz = np.dtype(dtype).itemsize
    h, w = lc.BIG_SRC_HW
    dsize = (lc.BIG_DSIZE[0], lc.ROWS_PAST_4G5)
    dw, dh = dsize
    src = lc.pixels(40, h, w, c, dtype)
    Minv = lc.big_map()
    t = torch.from_numpy(src).cuda()
    holder = out = None
    try:
        holder = byte_holder(lc.dest_reach(dh, dw, c, esz, lc.ROW_64M))
        out = strided(holder, dtype, (dh, dw, c), (lc.ROW_64M, c * esz, esz))
        assert out[dh - 1].data_ptr() - out.data_ptr() > 4.5 * (1 << 30)
        run_both_interps(t, src, Minv, dsize, out=out)
        for mode in (br.REPLICATE, br.REFLECT_101):
            same(W.warp_perspective(t, Minv, dsize, flags=W.INTER_LINEAR | INV, border_mode=mode, out=out).cpu().numpy(),
                 br.warp(src, Minv, dsize, br.LINEAR, mode, m_is_inverse=True))
        same(W.warp_perspective(t, Minv, dsize, flags=W.INTER_CUBIC | INV, border_value=lc.BORDER[:c], out=out).cpu().numpy(),
             cr.warp(src, Minv, dsize, br.CONSTANT, m_is_inverse=True, border_value=lc.BORDER[:c]))
        assert_only_the_view_was_written(holder, out, "destination rows beyond 4 GiB")
    finally:
        del holder, out
        torch.cuda.empty_cache()


@pytest.mark.parametrize("plane_dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_plane_rows_beyond_4gib(plane_dtype):
    """Case E, planes: one plane whose rows are 2^26 bytes apart."""
    h, w = lc.BIG_SRC_HW
    dsize = (lc.BIG_DSIZE[0], lc.ROWS_PAST_4G5)
    dw, dh = dsize
    src = lc.pixels(41, h, w, 1, np.uint8)
    fwd = np.linalg.inv(lc.big_map())
    t = torch.from_numpy(src).cuda()
    esz = 4 if plane_dtype == torch.float32 else 2
    holder = out = None
    try:
        holder = byte_holder(lc.dest_reach(dh, dw, 1, esz, lc.ROW_64M))
        out = strided(holder, plane_dtype, (1, dh, dw), (dh * lc.ROW_64M, lc.ROW_64M, esz))
        planes = p16.planes_f32(src, fwd, dsize, co.LINEAR, SCALE[:1], BIAS[:1], border_value=lc.BORDER[:1])
        W.warp_to_planar(t, fwd, dsize, scale=SCALE[:1], bias=BIAS[:1], border_value=lc.BORDER[:1], out=out, out_dtype=plane_dtype)
        if plane_dtype == torch.float32:
            px.same_float(out.cpu().numpy(), planes)
        else:
            p16.assert_same16(p16.gpu_bits(out), p16.to_bits(planes, plane_dtype), plane_dtype)
        assert_only_the_view_was_written(holder, out, "plane rows beyond 4 GiB")
    finally:
        del holder, out
        torch.cuda.empty_cache()


# ---- F: item decoding at the edge of fast_div's exactness --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_driver():
    """tests/host_plan_driver.cpp (bev_amd/csrc/host_plan.h from the command line), built plainly."""
    exe = hostplan.build_driver(sanitize=False)

    def plan(line):
        r = subprocess.run([exe, "plan"], input=line + "\n", capture_output=True, text=True, timeout=60, check=True)
        v = [int(x) for x in r.stdout.split()]
        return dict(status=v[0], tile_h=v[1], tiles_x=v[2], tiles_per_frame=v[3], total_tiles=v[4], chunk=v[5], tpf_magic=v[9])
    return plan


def decode_batch(B, dh):
    h, w = lc.DECODE_SRC_HW
    src = np.stack([lc.pixels(50 + i, h, w, 1, np.uint8) for i in range(B)])
    fwd = np.linalg.inv(lc.decode_map(dh))
    return src, np.stack([wl.jitter_H(fwd, i) for i in range(B)])


def test_item_decoding_row_kernel(plan_driver):
    """Case F through bevwarp_warp: a 3-pixel-wide destination of 37747 tiles per frame.  Three frames keep total * tiles_per_frame just
    below 2^32 (a multiply-high decodes the items), four take it beyond (the kernel divides, by d > 1).  Every frame has its own matrix
    and content: a quotient off by one moves a tile into another frame."""
    lib = _lib.load()
    h, w = lc.DECODE_SRC_HW
    resident = torch.cuda.get_device_properties(0).multi_processor_count * 4
    tile_h = plan_driver("rows %d %d %d 0 256 4 %d" % (lc.DECODE_BATCHES[0], 1 << 20, lc.DECODE_DW, resident))["tile_h"]
    dh = lc.DECODE_TILES * tile_h
    magics = []
    for B in lc.DECODE_BATCHES:
        p = plan_driver("rows %d %d %d 0 256 4 %d" % (B, dh, lc.DECODE_DW, resident))
        # the plan is the library's: its table has 12 bytes per tile of this plan
        assert p["status"] == 0 and lib.bevwarp_tile_classes_bytes(B, h, w, dh, lc.DECODE_DW, 1, _lib.U8, 1) == 12 * p["total_tiles"]
        assert p["tiles_per_frame"] == lc.DECODE_TILES and p["tiles_x"] == 1 and p["total_tiles"] == B * lc.DECODE_TILES
        magics.append((8 * p["chunk"] * p["tiles_per_frame"], p["tpf_magic"]))
    (n_lo, magic_lo), (n_hi, magic_hi) = magics
    assert n_lo < 1 << 32 <= n_hi and (1 << 32) - n_lo < (1 << 32) // 100 and magic_lo != 0 and magic_hi == 0  # the two calls straddle the bound
    for B in lc.DECODE_BATCHES:
        src, Ms = decode_batch(B, dh)
        t = torch.from_numpy(src).cuda()
        exp = np.stack([co.warp_perspective(f, M, (lc.DECODE_DW, dh), 1, nthreads=8) for f, M in zip(src, Ms)])
        assert all(not np.array_equal(exp[i], exp[j]) for i in range(B) for j in range(i))
        check_modes(warp_modes(t, Ms, (lc.DECODE_DW, dh), out=poisoned_out(t, (lc.DECODE_DW, dh))), exp)


def test_item_decoding_border_kernel(plan_driver):
    """Case F through the border kernel's flat grid (256 x 4 tiles, one workgroup per item): the same two batches."""
    dh = lc.DECODE_TILES * 4
    magics = []
    for B in lc.DECODE_BATCHES:
        p = plan_driver("border %d %d %d 256 4 %d %d %d" % (B, dh, lc.DECODE_DW, br.REPLICATE, lc.DECODE_SRC_HW[0], lc.DECODE_SRC_HW[1]))
        assert p["status"] == 0 and p["tile_h"] == 4 and p["tiles_per_frame"] == lc.DECODE_TILES and p["total_tiles"] == B * lc.DECODE_TILES
        magics.append((p["total_tiles"] * p["tiles_per_frame"], p["tpf_magic"]))
    (n_lo, magic_lo), (n_hi, magic_hi) = magics
    assert n_lo < 1 << 32 <= n_hi and (1 << 32) - n_lo < (1 << 32) // 100 and magic_lo != 0 and magic_hi == 0
    for B in lc.DECODE_BATCHES:
        src, Ms = decode_batch(B, dh)
        t = torch.from_numpy(src).cuda()
        exp = np.stack([br.warp(f, M, (lc.DECODE_DW, dh), br.LINEAR, br.REPLICATE) for f, M in zip(src, Ms)])
        assert all(not np.array_equal(exp[i], exp[j]) for i in range(B) for j in range(i))
        got = W.warp_perspective(t, Ms, (lc.DECODE_DW, dh), border_mode=br.REPLICATE, out=poisoned_out(t, (lc.DECODE_DW, dh)))
        np.testing.assert_array_equal(got.cpu().numpy(), exp)


# ---- geometry and resize kernels at their grid limits ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("nb", [3, 65])
def test_rbox_iou_at_the_grid_limit(nb, dtype):
    """na = 65535 (the grid's y dimension), nb = 3 and 65 (two column blocks): sampled rows against the oracle, the whole matrix on the
    device against the same kernel launched as two halves; na = 65536 raises."""
    from bev_amd.iou import rbox_iou
    rng = np.random.default_rng(61)
    b = np.column_stack([rng.uniform(0, 100, (nb, 2)), rng.uniform(1.6, 2.2, nb), rng.uniform(3.5, 6, nb), rng.uniform(-np.pi, np.pi, nb)])
    a = lc.boxes_around(lc.GRID_MAX, b, 62)
    ta, tb = torch.from_numpy(a.astype(dtype)).cuda(), torch.from_numpy(b.astype(dtype)).cuda()
    full = rbox_iou(ta, tb)
    assert full.shape == (lc.GRID_MAX, nb)
    rows = lc.sample_rows(lc.GRID_MAX)
    assert {0, 63, 64, lc.GRID_MAX - 1} <= set(rows.tolist()) and len(rows) > 300
    exp = co.rbox_iou(a[rows].astype(dtype), b.astype(dtype))
    assert (exp > 0.2).sum() > 100
    np.testing.assert_allclose(full[torch.from_numpy(rows).cuda()].cpu().numpy(), exp, rtol=0, atol=1e-12 if dtype == np.float64 else 2e-6)
    half = lc.GRID_MAX // 2
    assert torch.equal(full, torch.cat([rbox_iou(ta[:half], tb), rbox_iou(ta[half:], tb)]))
    with pytest.raises(ValueError):
        rbox_iou(torch.zeros((lc.GRID_MAX + 1, 5), dtype=ta.dtype, device="cuda"), tb)


def test_tracker_step_at_the_grid_limit():
    """n = 64000 detections (64000 scoring rows + 1000 output rows of the grid), m = 3 tracks; n = 64001 raises."""
    from bev_amd import rbox as host_rbox
    from bev_amd.tracker_geom import tracker_geometry_step
    n, m = lc.TRACKER_MAX, 3
    dets_bev, trks, H_world_bev, H_img_world = lc.tracker_case(n, m)
    out = tracker_geometry_step(dets_bev, trks, H_world_bev, iou_threshold=0.3, H_img_world=H_img_world)
    dets_world_host = host_rbox.rbox_world_bev(dets_bev, H_world_bev, "bev")
    got_world = out["dets_world"].cpu().numpy()
    np.testing.assert_allclose(got_world, dets_world_host, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(out["dets_img"].cpu().numpy(), host_rbox.rbox_world_img(dets_world_host, H_img_world), rtol=1e-10, atol=1e-8)
    rows = lc.sample_rows(n)
    exp = co.rbox_iou(got_world[rows], trks[:, :5])
    assert (exp > 0.3).sum() > 100
    np.testing.assert_allclose(out["iou"].cpu().numpy()[rows], exp, rtol=0, atol=1e-12)
    assert torch.equal(out["candidates"], out["iou"] > 0.3) and out["iou"].shape == (n, m)
    with pytest.raises(ValueError):
        tracker_geometry_step(np.concatenate([dets_bev, dets_bev[:1]]), trks, H_world_bev, 0.3, H_img_world)


def resize_status(src, dst, batch, sh, sw, dh, dw, c):
    return _lib.load().bevwarp_resize(src.data_ptr(), dst.data_ptr(), batch, sh, sw, dh, dw, c, sh * sw * c, sw * c, dh * dw * c, dw * c, _lib.U8, 1, None)


def test_resize_at_the_grid_limits():
    """dst_h = 65535 and batch = 65535 (the grid's y and z dimensions), against the oracle; one past either returns BEVWARP_ERR_TOO_LARGE."""
    from bev_amd.resize import resize
    rng = np.random.default_rng(71)
    src = rng.integers(0, 256, (3, 7, 3), dtype=np.uint8)
    got = resize(torch.from_numpy(src).cuda(), (5, lc.GRID_MAX))
    np.testing.assert_array_equal(got.cpu().numpy(), co.resize_linear_u8(src, (5, lc.GRID_MAX)))
    # 65535 frames: 257 distinct ones, repeated (the oracle runs once per distinct frame)
    base = rng.integers(0, 256, (257, 2, 2, 3), dtype=np.uint8)
    idx = np.arange(lc.GRID_MAX) % 257
    frames = torch.from_numpy(base).cuda()[torch.from_numpy(idx).cuda()]
    exp = np.stack([co.resize_linear_u8(f, (3, 3)) for f in base])[idx]
    got = resize(frames, (3, 3))
    assert got.shape == (lc.GRID_MAX, 3, 3, 3)
    np.testing.assert_array_equal(got.cpu().numpy(), exp)
    dst = torch.empty(4096, dtype=torch.uint8, device="cuda")
    assert resize_status(frames, dst, 1, 3, 7, lc.GRID_MAX + 1, 5, 3) == TOO_LARGE
    assert resize_status(frames, dst, lc.GRID_MAX + 1, 2, 2, 3, 3, 3) == TOO_LARGE
    assert resize_status(frames, dst, 1, 1, lc.RESIZE_SIDE + 1, 1, 1000, 1) == TOO_LARGE
    assert resize_status(frames, dst, 1, lc.RESIZE_SIDE + 1, 1, 1000, 1, 1) == TOO_LARGE


@pytest.mark.parametrize("kernel", ["four_pixels", "one_pixel"])
def test_resize_widest_source(kernel):
    """A source row of 2^24 pixels to 1000: the four-pixel kernel (aligned destination), and the one-pixel kernel (a destination whose
    base is not 4-byte aligned takes it)."""
    from bev_amd.resize import resize
    src = np.random.default_rng(72).integers(0, 256, (1, lc.RESIZE_SIDE, 1), dtype=np.uint8)
    t = torch.from_numpy(src).cuda()
    holder = torch.full((1000 + 64,), lc.U8_CANARY, dtype=torch.uint8, device="cuda")
    off = 16 if kernel == "four_pixels" else 17
    out = holder[off:off + 1000].view(1, 1000, 1)
    assert (out.data_ptr() % 4 == 0) == (kernel == "four_pixels")
    resize(t, (1000, 1), out=out)
    np.testing.assert_array_equal(out.cpu().numpy(), co.resize_linear_u8(src, (1000, 1)))
    rest = torch.cat([holder[:off], holder[off + 1000:]])
    assert bool((rest == lc.U8_CANARY).all().item())


def test_footprint_at_the_grid_limits():
    """dst_h = 65535 and batch = 65535 against the oracle's footprint, counts and maps; one past either is BEVWARP_ERR_TOO_LARGE."""
    hw, dsize = (50, 70), (5, lc.GRID_MAX)
    Minv = lc.affine(9.0, 3.3, 51.0 / (lc.GRID_MAX - 1), -0.6)
    for interp in (W.INTER_LINEAR, W.INTER_NEAREST):
        counts, touched = W.footprint(hw, Minv, dsize, flags=interp | INV)
        n, t = co.footprint(hw, Minv, dsize, interp, m_is_inverse=True)
        assert int(counts[0]) == n and 0 < n < hw[0] * hw[1]
        np.testing.assert_array_equal(touched[0].cpu().numpy(), t)
    # 65535 matrices: 251 distinct ones, repeated
    hw, dsize = (6, 8), (4, 3)
    base = np.stack([lc.jittered_inverse(lc.affine(1.7, 0.4, 1.6, 0.3), i, px=3.0) for i in range(251)])
    idx = np.arange(lc.GRID_MAX) % 251
    counts, touched = W.footprint(hw, base[idx], dsize, flags=W.INTER_LINEAR | INV)
    exp = [co.footprint(hw, M, dsize, co.LINEAR, m_is_inverse=True) for M in base]
    assert len({n for n, _ in exp}) > 3
    np.testing.assert_array_equal(counts.cpu().numpy(), np.array([n for n, _ in exp])[idx])
    np.testing.assert_array_equal(touched.cpu().numpy(), np.stack([t for _, t in exp])[idx])
    lib, minv = _lib.load(), W.device_inverse(Minv, touched.device, inverse_given=True)
    assert lib.bevwarp_footprint(touched.data_ptr(), 1, 6, 8, lc.GRID_MAX + 1, 5, minv.data_ptr(), 1, 1, None) == TOO_LARGE
    assert lib.bevwarp_footprint(touched.data_ptr(), lc.GRID_MAX + 1, 6, 8, 3, 4, minv.data_ptr(), 1, 1, None) == TOO_LARGE
