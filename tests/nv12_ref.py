"""The reference of the NV12 warp (bevwarp_warp_nv12, bev_amd.warp.warp_perspective_nv12) -- TEST INFRASTRUCTURE ONLY, a plain module like
tests/border_ref.py.

nv12_to_bgr   OpenCV's 8-bit cvtYUV420sp2RGB (BT.601, limited range, 20-bit fixed point) in numpy int32: the formula of include/bevwarp.h,
              restated from memory like the rest of the warp (parity with OpenCV is unpinned)
warp_nv12     the definition everything is tested against: oracle.cpu_oracle.warp_perspective of the CONVERTED frame
frame         seeded NV12 frames: "uniform", "video", "domain", "phase"
"""
import functools

import numpy as np

from oracle import cpu_oracle

KY, KRV, KGV, KGU, KBU, ROUND, SHIFT = 1220542, 1673527, -852492, -409993, 2116026, 1 << 19, 20


def unclamped(Y, U, V):
    """(R, G, B) before the clamp, int64 sums (so that the caller can check that int32 holds them) -> (sums, shifted values)."""
    yy = np.maximum(0, np.asarray(Y, np.int64) - 16) * KY
    u, v = np.asarray(U, np.int64) - 128, np.asarray(V, np.int64) - 128
    sums = (yy + ROUND + KRV * v, yy + ROUND + KGV * v + KGU * u, yy + ROUND + KBU * u)
    return sums, tuple(s >> SHIFT for s in sums)


def convert(Y, U, V, rgb=False):
    """Arrays of Y, U, V bytes (broadcast against each other) -> (..., 3) uint8 in B, G, R order (rgb: R, G, B); int32 arithmetic."""
    yy = np.maximum(np.int32(0), np.asarray(Y).astype(np.int32) - np.int32(16)) * np.int32(KY)
    u, v = np.asarray(U).astype(np.int32) - np.int32(128), np.asarray(V).astype(np.int32) - np.int32(128)
    r = np.clip((yy + np.int32(ROUND) + np.int32(KRV) * v) >> SHIFT, 0, 255)
    g = np.clip((yy + np.int32(ROUND) + np.int32(KGV) * v + np.int32(KGU) * u) >> SHIFT, 0, 255)
    b = np.clip((yy + np.int32(ROUND) + np.int32(KBU) * u) >> SHIFT, 0, 255)
    assert r.dtype == np.int32 and g.dtype == np.int32 and b.dtype == np.int32
    return np.stack((r, g, b) if rgb else (b, g, r), axis=-1).astype(np.uint8)


def nv12_to_bgr(y, uv, rgb=False):
    """y (H, W) uint8, uv (H / 2, W / 2, 2) uint8 -> (H, W, 3): pixel (x, y) takes the pair (y >> 1, x >> 1)."""
    y, uv = np.asarray(y), np.asarray(uv)
    H, W = y.shape
    assert y.dtype == np.uint8 and uv.dtype == np.uint8 and H % 2 == 0 and W % 2 == 0 and uv.shape == (H // 2, W // 2, 2), (y.shape, uv.shape)
    full = np.repeat(np.repeat(uv, 2, axis=0), 2, axis=1)
    return convert(y, full[..., 0], full[..., 1], rgb)


def warp_nv12(y, uv, M, dsize, interp=cpu_oracle.LINEAR, border_value=None, rgb=False, m_is_inverse=False, nthreads=1):
    """bevwarp_warp of the converted frame.  border_value is in the result's channel order and is not converted."""
    return cpu_oracle.warp_perspective(nv12_to_bgr(y, uv, rgb), M, dsize, interp, m_is_inverse=m_is_inverse, border_value=border_value, nthreads=nthreads)


def join(y, uv):
    """The single-buffer layout: (H * 3 / 2, W), the rows of pairs behind the Y rows."""
    return np.concatenate([y, uv.reshape(uv.shape[0], -1)], axis=0)


@functools.lru_cache(maxsize=None)
def _domain():
    # pair i of the 2048 x 2048 takes the value i mod 65536 (U the low byte) and is block i // 65536 of that value: its four Y are 4 * block + 0 .. 3
    i = np.arange(2048 * 2048, dtype=np.int64).reshape(2048, 2048)
    uv = np.stack([i & 0xff, (i >> 8) & 0xff], axis=-1).astype(np.uint8)
    blk = (i >> 16).astype(np.int64) * 4
    y = np.empty((4096, 4096), np.uint8)
    y[0::2, 0::2], y[0::2, 1::2], y[1::2, 0::2], y[1::2, 1::2] = blk, blk + 1, blk + 2, blk + 3
    y.setflags(write=False)
    uv.setflags(write=False)
    return y, uv


def frame(kind, seed, h, w):
    """(y, uv) of one NV12 frame, h x w (both even).
    "uniform"  every byte random: about 25-45 % of the converted channel values saturate (both clamps are exercised)
    "video"    Y in [64, 180], U and V in [108, 148]: no channel saturates (results span 16 .. 231)
    "phase"    random, and made so that every pair differs from its four neighbours in U and in V: a tap that takes the wrong pair shows
    "domain"   4096 x 4096 (h, w are ignored): every (Y, U, V) occurs exactly once -- 65,536 pair values x 64 blocks of 4 Y values"""
    if kind == "domain":
        return _domain()
    assert h % 2 == 0 and w % 2 == 0 and h > 0 and w > 0
    rng = np.random.default_rng(7000 + seed)
    if kind == "uniform":
        return rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w // 2, 2), dtype=np.uint8)
    if kind == "video":
        return rng.integers(64, 181, (h, w), dtype=np.uint8), rng.integers(108, 149, (h // 2, w // 2, 2), dtype=np.uint8)
    if kind == "phase":
        jj, ii = np.meshgrid(np.arange(w // 2), np.arange(h // 2))
        # residues mod 5 of (i + 2 j) and of (2 i + j) differ between horizontal, vertical and both diagonal neighbours; the low part is random
        u = ((ii + 2 * jj) % 5) * 51 + rng.integers(0, 40, ii.shape)
        v = ((2 * ii + jj) % 5) * 51 + rng.integers(0, 40, ii.shape)
        return rng.integers(0, 256, (h, w), dtype=np.uint8), np.stack([u, v], axis=-1).astype(np.uint8)
    raise ValueError(kind)
