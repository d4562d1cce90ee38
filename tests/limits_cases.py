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

# ---- C: the largest row stride ---------------------------------------------------------------------------------------------------------
STRIDE_W = 640
STRIDE_DSIZE = (600, 64)
STRIDE_ALIGNED = ROW_LIMIT - 16   # float32, and 8-bit RGBA
STRIDE_ODD = ROW_LIMIT - 1        # 8-bit, 1 and 3 channels: every row starts at another residue mod 4


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


# ---- D, E: strides beyond 4 GiB ------------------------------------------------------------------------------------------------------------
BIG_SRC_HW = (96, 700)
BIG_DSIZE = (600, 40)
BIG_BATCH = 3
ROWS_PAST_4G5 = int(4.5 * (1 << 30)) // ROW_64M + 2  # destination rows of case E: the last one is the first to start beyond 4.5 GiB


def big_map():
    return affine(1.1, 8.4, 2.3, -1.7)  # reaches above the frame and, on the right, just inside it


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
