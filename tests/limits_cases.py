"""Shapes, strides and matrices of the limit tests (a plain module): tests/test_gpu_limits.py runs the kernels on them, tests/test_limits_cpu.py
checks the oracle and the layouts on the same objects, so the two cannot drift apart.  No GPU, no oracle.

Every matrix here is an INVERSE map (destination pixel -> source pixel), the form the kernels consume: the warps are called with
WARP_INVERSE_MAP and the oracle with m_is_inverse=True, so no inversion stands between a case and the coordinates it is meant to hit.

The limits are the ones include/bevwarp.h and bev_amd/csrc/host_plan.h state: source sides <= 32767, a source row stride < 2^24 bytes and
rows * stride < 2^31 bytes (the fast tiles' 24-bit multiplies), destination sides <= 2^20, grid dimensions <= 65535."""
import numpy as np

MAX_SIDE = 32767            # source sides of a warp
ROW_LIMIT = 1 << 24         # a source row stride stays below this
FRAME_LIMIT = 1 << 31       # rows * row stride stays below this
BEYOND_4G = (1 << 32) + 4096  # the frame / plane stride of case D
ROW_64M = 1 << 26           # the destination row stride of case E
GRID_MAX = 65535            # rbox_iou's na, resize's and footprint's dst_h and batch
TRACKER_MAX = 64000         # tracker_step's n
RESIZE_SIDE = 1 << 24       # resize's source sides

U8_CANARY = 0xC3
F32_CANARY_BITS = 0x7fc00c3c  # a quiet NaN with a recognisable payload: a stray source read poisons the pixel, a stray store shows


def affine(ax, bx, ay, by):
    """sx = ax * x + bx, sy = ay * y + by as an inverse matrix."""
    return np.array([[ax, 0.0, bx], [0.0, ay, by], [0.0, 0.0, 1.0]])


# ---- A, B: the widest and the tallest source ------------------------------------------------------------------------------------------
WIDE_HW = (40, MAX_SIDE)
WIDE_DSIZE = (600, 40)
# "right_end": a 1:1 translation that parks the destination on the source's right end -- columns 32290 .. 32889, so 8-bit tiles (256 px)
# and float tiles (128 px) inside the frame, cut by its right edge and wholly beyond it; the top rows start 2.4 px above the frame.
# "minify64": 64 source pixels per destination pixel over the full width: x = 511 lands on sx = 32765, the last column with two valid
# taps, x = 512 on the saturated 32767.
WIDE_MAPS = {"right_end": affine(1.0, 32290.3, 1.0, -2.4), "minify64": affine(64.0, 61.25, 0.9, 0.8)}
TALL_HW = (MAX_SIDE, 40)
TALL_DSIZE = (40, 600)
# The transposes, except that x is compressed into the 40-pixel source: a tile is classified at its full width (256 / 128 px) whatever the
# destination's, so only then does a tile lie inside the frame -- and only tiles inside the frame form the 24-bit tap addresses.
TALL_MAPS = {"right_end": affine(0.1, 4.3, 1.0, 32290.3), "minify64": affine(0.1, 4.3, 64.0, 61.25)}

# The same two cases for the entries tests/test_gpu_limits_entries.py runs (lens, NV12, map and stitch kernels).  NV12 frames have even
# sides, so theirs is 32766 px: `right_end` is unchanged (columns 32290 .. 32889 pass the last column with two valid taps, 32764, the last
# column, 32765, and saturate at 32767), `minify64` starts a pixel earlier, so that x = 511 lands on sx = 32764 = w - 2 and x = 512 on the
# saturated 32767.  Neither map leaves the frame on the near side of the long axis, so both sets get `left_end`: a 1:1 translation that
# starts 20.6 px BEFORE the frame (indices -21 .. -1 on the long axis, -1 with one valid tap).
MAX_EVEN = 32766            # NV12 sides
WIDE_NV12_HW = (40, MAX_EVEN)
TALL_NV12_HW = (MAX_EVEN, 40)
WIDE_LEFT_END, TALL_LEFT_END = affine(1.0, -20.6, 1.0, -2.4), affine(0.1, 4.3, 1.0, -20.6)
WIDE_ENTRY_MAPS = dict(WIDE_MAPS, left_end=WIDE_LEFT_END)
TALL_ENTRY_MAPS = dict(TALL_MAPS, left_end=TALL_LEFT_END)
WIDE_NV12_MAPS = {"right_end": WIDE_MAPS["right_end"], "minify64": affine(64.0, 60.25, 0.9, 0.8), "left_end": WIDE_LEFT_END}
TALL_NV12_MAPS = {"right_end": TALL_MAPS["right_end"], "minify64": affine(0.1, 4.3, 64.0, 60.25), "left_end": TALL_LEFT_END}


def entry_case(name, nv12=False):
    """(source (H, W), destination (w, h), {map name: inverse matrix}, the long axis' index in (sx, sy)) of case A ("wide") or B ("tall")."""
    if name == "wide":
        return (WIDE_NV12_HW if nv12 else WIDE_HW), WIDE_DSIZE, (WIDE_NV12_MAPS if nv12 else WIDE_ENTRY_MAPS), 0
    return (TALL_NV12_HW if nv12 else TALL_HW), TALL_DSIZE, (TALL_NV12_MAPS if nv12 else TALL_ENTRY_MAPS), 1


LENS_R2 = {"right_end": 1.011, "left_end": 1.011, "minify64": 1.03}  # r2_max of a lens run, in units of the far corner's r2


def mild_lens(hw, key="right_end"):
    """(K, dist_coeff, r2_max) of a mild lens for a camera of hw = (H, W): lens_ref.camera_K of that size, and k1, p1 scaled to the squared
    radius r2 of the frame's far corner on the normalised plane -- k1 r2 = -0.004 pulls that corner about 0.4 % (some 60 px of 32767)
    towards the centre, p1 moves it about a pixel across.  With steps of about one source pixel per destination pixel the `right_end` and
    `left_end` maps therefore still pass every index next to the frame's ends.  r2_max (LENS_R2[key] corner radii) lies between the radius
    at which the map saturates and the radius of its last pixels: pixels beyond it are outside (tests/test_limits_cpu.py asserts that
    valid saturated pixels and pixels beyond r2_max both occur)."""
    from tests import lens_ref
    h, w = hw
    K = lens_ref.camera_K(w, h)
    r2 = ((w - 1 - K[0, 2]) / K[0, 0]) ** 2 + ((h - 1 - K[1, 2]) / K[1, 1]) ** 2
    return K, (-0.004 / r2, 0.0, 1.0 / (r2 * K[0, 0]), 0.0, 0.0), LENS_R2[key] * r2


# The maps of the lens runs (undistorted source pixels): `right_end` as it is; `left_end` starts 66 px earlier, which the lens gives back;
# `minify64` keeps its 64 px per destination pixel (about 63 after the lens) and starts where the lens lands a pixel on side - 2 = 32765
# for both interpolations (the coordinate falls in [32765, 32765.5)), the next one on the saturated 32767, still within r2_max.
WIDE_LENS_MAPS = {"right_end": WIDE_MAPS["right_end"], "left_end": affine(1.0, -86.6, 1.0, -2.4), "minify64": affine(64.0, 63.5, 0.9, 0.8)}
TALL_LENS_MAPS = {"right_end": TALL_MAPS["right_end"], "left_end": affine(0.1, 4.3, 1.0, -86.6), "minify64": affine(0.1, 4.3, 64.0, 60.25)}


# ---- C: the largest row stride ---------------------------------------------------------------------------------------------------------
STRIDE_W = 640
STRIDE_DSIZE = (600, 64)
STRIDE_ALIGNED = ROW_LIMIT - 16   # float32, and 8-bit RGBA
STRIDE_ODD = ROW_LIMIT - 1        # 8-bit, 1 and 3 channels: every row starts at another residue mod 4
# NV12 at the largest strides the checks admit: (row stride, rows) of the Y plane and of the plane of (U, V) pairs, whose strides are even
STRIDE_NV12 = {"y": (ROW_LIMIT - 1, 128), "uv": (ROW_LIMIT - 2, 64)}


def max_rows(stride):
    """The most rows check_warp admits for a row stride: rows * stride < 2^31."""
    return (FRAME_LIMIT - 1) // stride


def stride_map(rows):
    """Reads source rows 0 .. rows - 1 (the last destination row samples half a pixel into the last source row, so its lower taps are
    the border); with 64 destination rows over 128 source rows the tile of rows 56 .. 59 lies inside the frame, within its last 20 rows."""
    return affine(1.0, 10.3, (rows - 0.7) / (STRIDE_DSIZE[1] - 1), 0.2)


# (name, source (H, W), destination (w, h), {map name: inverse matrix}) of the compact copies of A, B and C
def compact_cases():
    rows = max_rows(STRIDE_ALIGNED)
    assert rows == max_rows(STRIDE_ODD) == 128
    return [("wide", WIDE_HW, WIDE_DSIZE, WIDE_MAPS), ("tall", TALL_HW, TALL_DSIZE, TALL_MAPS), ("stride", (rows, STRIDE_W), STRIDE_DSIZE, {"rows": stride_map(rows)})]


# (dtype, channels) of A and B; C takes its channels from the stride
WIDE_FORMATS = [(np.uint8, 1), (np.uint8, 3), (np.uint8, 4), (np.float32, 1), (np.float32, 4)]
STRIDE_FORMATS = [(np.float32, 1, STRIDE_ALIGNED), (np.float32, 4, STRIDE_ALIGNED), (np.uint8, 4, STRIDE_ALIGNED), (np.uint8, 1, STRIDE_ODD), (np.uint8, 3, STRIDE_ODD)]


def pixels(seed, h, w, c, dtype):
    """Seeded content: uint8 over the whole range; float32 in [0, 1) with signs, so no value is the canary or the border value."""
    rng = np.random.default_rng(7000 + seed)
    if np.dtype(dtype) == np.uint8:
        return rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    return (rng.random((h, w, c), dtype=np.float32) - np.float32(0.5)).astype(np.float32)


BORDER = [9.0, 200.0, 31.0, 77.0]  # a non-zero border value per channel: border pixels are told from unwritten and from zero ones


# ---- layouts -----------------------------------------------------------------------------------------------------------------------------
def extent_bytes(shape, strides_bytes, esz):
    """Bytes from a strided view's base to one past its last element: what its backing buffer must hold."""
    return sum((n - 1) * s for n, s in zip(shape, strides_bytes)) + esz


def source_reach(h, w, c, esz, rs, batch=1, fs=0):
    """The last byte + 1 a warp kernel may form for a source: (batch - 1) * fs + (h - 1) * rs + row bytes."""
    return (batch - 1) * fs + (h - 1) * rs + w * c * esz


def dest_reach(dh, dw, c, esz, rs, batch=1, fs=0, planes=1, ps=0):
    """The end of the last store: interleaved rows of dw * c elements, or `planes` planes of dw elements, `ps` bytes apart."""
    return (batch - 1) * fs + (planes - 1) * ps + (dh - 1) * rs + dw * (c if planes == 1 else 1) * esz


# NV12 frames in ONE holder.  Each helper returns {"y": spec, "uv": spec, "bytes": what the holder must hold}, a spec being the (shape,
# strides in bytes, byte offset) of a uint8 view of the holder -- (B, h, w) / (h, w) for Y, (B, h / 2, w / 2, 2) / (h / 2, w / 2, 2) for the pairs.
def _nv12_specs(y, uv):
    return {"y": y, "uv": uv, "bytes": max(off + extent_bytes(shape, strides, 1) for shape, strides, off in (y, uv))}


def nv12_joined(batch, h, w, fs):
    """`batch` frames `fs` bytes apart, each the decoders' single buffer: h rows of Y, then h / 2 rows of pairs, all w bytes apart --
    one frame stride for both planes."""
    assert h % 2 == 0 and w % 2 == 0 and fs >= h * 3 // 2 * w
    return _nv12_specs(((batch, h, w), (fs, w, 1), 0), ((batch, h // 2, w // 2, 2), (fs, w, 2, 1), h * w))


def nv12_beside(h, w, rs, uv_off):
    """One frame whose rows are `rs` bytes apart: row i of Y starts stretch i, row j of the pairs lies in stretch j too, `uv_off` bytes in
    (beyond the Y row): two planes side by side with one row stride."""
    assert h % 2 == 0 and w % 2 == 0 and uv_off % 2 == 0 and w <= uv_off and uv_off + w <= rs
    return _nv12_specs(((h, w), (rs, 1), 0), ((h // 2, w // 2, 2), (rs, 2, 1), uv_off))


def spec_rows(spec):
    """[(first byte, one past the last byte)] of every row of a spec'd view, frame by frame."""
    shape, strides, off = spec
    lead = [(n, s) for n, s in zip(shape, strides) if s > 2]  # (frame and row dimensions; a row's bytes are contiguous)
    row_bytes = extent_bytes(shape[len(lead):], strides[len(lead):], 1)
    starts = [off]
    for n, s in lead:
        starts = [b + i * s for b in starts for i in range(n)]
    return [(b, b + row_bytes) for b in starts]


# ---- D, E: strides beyond 4 GiB ------------------------------------------------------------------------------------------------------------
BIG_SRC_HW = (96, 700)
BIG_DSIZE = (600, 40)
BIG_BATCH = 3
ROWS_PAST_4G5 = int(4.5 * (1 << 30)) // ROW_64M + 2  # destination rows of case E: the last one is the first to start beyond 4.5 GiB


def big_map():
    return affine(1.1, 8.4, 2.3, -1.7)  # reaches above the frame and, on the right, just inside it


# The three cameras of the stitch runs over one 600 x 40 canvas: the widest source parked on its right end (it covers x <= 476), the tallest
# one on its lower end (sy = 32740 .. 32779: it covers y <= 26, or 25 for the 32766-row NV12 frame) and a 96 x 700 frame (it covers y >= 1,
# x <= 530); nothing covers the lower right corner.
STITCH_DSIZE = (600, 40)


def stitch_cameras(nv12=False):
    """[(source (H, W), inverse matrix)] of the three cameras; nv12: the even-sided sources."""
    return [(WIDE_NV12_HW if nv12 else WIDE_HW, WIDE_MAPS["right_end"]), (TALL_NV12_HW if nv12 else TALL_HW, affine(0.06, 1.3, 1.0, 32740.3)),
            (BIG_SRC_HW, affine(1.3, 8.4, 2.3, -1.7))]


def jittered_inverse(Minv, idx, px=2.0):
    """The inverse of workloads.jitter_H(forward, idx): a seeded translation of the destination, per frame."""
    rng = np.random.default_rng(99 + idx)
    tx, ty = rng.uniform(-px, px, 2) if idx > 0 else (0.0, 0.0)
    return Minv @ np.array([[1.0, 0.0, -tx], [0.0, 1.0, -ty], [0.0, 0.0, 1.0]])


# ---- F: item decoding at the edge of fast_div's exactness ----------------------------------------------------------------------------------
# With d tiles per frame and B frames the kernels divide items n < B d by d.  The multiply-high is exact while n_max * d < 2^32; beyond,
# the host hands out magic 0 and the kernel divides.  d = 37747: 3 d^2 is 0.5 % below 2^32, 4 d^2 above it, and d is chosen so that the
# multiply-high with the magic of d really is wrong for an item of the 4-frame launch (n = 4 d - 1 gives 4, not 3): a kernel that
# skipped the fallback would put the last tile of the last frame elsewhere.
DECODE_TILES = 37747
DECODE_BATCHES = (3, 4)
DECODE_SRC_HW = (64, 64)
DECODE_DW = 3
DECODE_DW_EVEN = 2  # for the entries that write NV12


def decode_map(dh):
    return affine(20.0, 2.2, 61.0 / (dh - 1), 0.6)


def multiply_high_is_exact(n_items, d):
    magic = (1 << 32) // d + 1
    return all((n * magic) >> 32 == n // d for k in range(1, n_items // d + 1) for n in (k * d - 1, k * d - d))


# ---- boxes ------------------------------------------------------------------------------------------------------------------------------------
def boxes_around(n, anchors, seed, every=2):
    """n world boxes [x, y, w, h, yaw]: every `every`-th one a jittered copy of an anchor (overlapping pairs), the rest scattered."""
    rng = np.random.default_rng(seed)
    out = np.column_stack([rng.uniform(0, 100, (n, 2)), rng.uniform(1.6, 2.2, n), rng.uniform(3.5, 6, n), rng.uniform(-np.pi, np.pi, n)])
    idx = np.arange(0, n, every)
    out[idx] = anchors[idx % len(anchors)] + rng.normal(0, [0.3, 0.3, 0.05, 0.1, 0.1], (len(idx), 5))
    return out


def tracker_case(n, m, seed=31):
    """(dets_bev (n, 5), trks_world (m, 7), H_world_bev, H_img_world): the calibration of tests/test_gpu_geom.py's tracker cases; every
    second detection is a tracker's box, jittered, taken back to the BEV raster by the host function."""
    import bev
    from bev_amd import rbox as host_rbox
    calib = bev.Calib(vp1=np.array([1200.0, -300.0]), vp2=np.array([-2500.0, -150.0]), pp=np.array([959.5, 539.5]), height=8, u_size=1920, v_size=1080)
    center = calib.gen_center_in_world()
    bspec = bev.BEVWorldSpec(u_size=1024, v_size=1024, u_axis="y", v_axis="-x", x_size=64, y_size=64, x_min=center[0] - 20, y_min=center[1] - 32)
    H_world_bev = bspec.gen_H_world_bev()
    H_img_world = np.linalg.inv(calib.gen_H_world_img())
    rng = np.random.default_rng(seed)
    trks = np.column_stack([rng.uniform([center[0] - 15, center[1] - 25], [center[0] + 35, center[1] + 25], (m, 2)), rng.uniform(1.6, 2.2, m), rng.uniform(3.5, 6, m),
                            rng.uniform(-np.pi, np.pi, m), rng.normal(0, 1, (m, 2))])
    world = boxes_around(n, trks[:, :5], seed + 1)
    world[1::2, :2] = rng.uniform([center[0] - 20, center[1] - 32], [center[0] + 44, center[1] + 32], (len(world[1::2]), 2))
    dets_bev = host_rbox.rbox_world_bev(world, np.linalg.inv(H_world_bev), "world")
    return dets_bev, trks, H_world_bev, H_img_world


def sample_rows(n, step=173):
    """Rows 0, 63, 64, n - 1 and every `step`-th one between."""
    return np.unique(np.concatenate([[0, 63, 64, n - 1], np.arange(0, n, step)]))
