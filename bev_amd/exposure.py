"""Per-camera exposure gains for the stitches through warp maps (include/bevwarp.h, BEVWARP_STITCH_GAIN).

Cameras of one site run their own auto-exposure, so a stitch shows a brightness step at every seam.  The stitches take a gain per camera
and channel (`gains=` of bev_amd.warp.remap_stitch* and of bev_amd.pipeline.SitePipeline) and apply it to every tap in registers; this
module finds those gains.  Estimation is not per frame -- the overlaps are constants of the site, and the gains drift with the light --
so it is PyTorch plumbing around one TRANSPARENT remap per camera:

    G = estimate_gains(frames, warp_maps)                   # now and then
    canvas = remap_stitch(frames, warp_maps, gains=G)       # every batch

The Q8 fixed point of the gain step: a gain g is the integer G = rint(256 g) in 0..1023, and a byte p becomes min(255, (p G + 128) >> 8).
"""
import numpy as np
import torch

GAIN_ONE, GAIN_MAX = 256, 1023  # Q8: 1.0, and the largest gain 1023 / 256


def quantize_gains(gains, n_cams):
    """The gains as the stitches take them: an int64 array (n_cams, 3) of Q8 values rint(256 g) in 0..1023.

    gains   (n_cams,) floats -- one gain per camera, for all three channels -- or (n_cams, 3), channel c being channel c of the pixel the
            stitch blends (the frames' own order; NV12 frames: the order `rgb` names).  Finite, in [0, 1023 / 256]; anything else is a
            ValueError, as is another shape or count."""
    try:
        g = np.asarray(gains.detach().cpu().numpy() if isinstance(gains, torch.Tensor) else gains, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("gains must be (n_cams,) or (n_cams, 3) floats, got %r" % (gains,))
    if g.ndim not in (1, 2) or (g.ndim == 2 and g.shape[1] != 3):
        raise ValueError("gains must have shape (n_cams,) or (n_cams, 3), got %s" % (g.shape,))
    if g.shape[0] != n_cams:
        raise ValueError("got %d gains for %d cameras" % (g.shape[0], n_cams))
    if not np.isfinite(g).all() or (g < 0).any() or (g > GAIN_MAX / 256.0).any():
        raise ValueError("gains must be finite and lie in [0, 1023/256], got %s" % (g.tolist(),))
    G = np.rint(256.0 * g).astype(np.int64)
    return np.ascontiguousarray(np.broadcast_to(G[:, None] if G.ndim == 1 else G, (n_cams, 3)))


def gain_words(G):
    """The packed gain word of every camera, G0 | G1 << 10 | G2 << 20, from quantize_gains' array: bevwarp_map_camera.reserved under
    BEVWARP_STITCH_GAIN."""
    return [int(g[0]) | int(g[1]) << 10 | int(g[2]) << 20 for g in np.asarray(G)]


def apply_gains(frames, G):
    """The gain step as a pass of its own over one camera's frames, in torch integer ops: min(255, (p G_c + 128) >> 8) per channel.

    frames  (..., 3) uint8 tensor (any device).  G: that camera's 3 Q8 gains (a row of quantize_gains' array).
    This is the route the gained stitch replaces -- a stitch of apply_gains' frames equals the gained stitch of the raw ones, by bits --
    and so its reference on the device.  Returns a new uint8 tensor."""
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() < 1 or frames.shape[-1] != 3:
        raise ValueError("apply_gains needs a uint8 tensor (..., 3), got %s %s" % (getattr(frames, "dtype", type(frames)), tuple(getattr(frames, "shape", ()))))
    G = np.asarray(G, dtype=np.int64).reshape(-1)
    if G.shape != (3,) or (G < 0).any() or (G > GAIN_MAX).any():
        raise ValueError("G must be 3 Q8 gains in 0..1023, got %s" % (G.tolist(),))
    g = torch.tensor(G.tolist(), dtype=torch.int32, device=frames.device)
    return ((frames.to(torch.int32) * g + 128) >> 8).clamp_(max=255).to(torch.uint8)


def cover_mask(warp_map, src_hw):
    """Where a camera with frames of src_hw = (H, W) covers the canvas: BORDER_TRANSPARENT's inlier test of the map's entries, the
    stitches' cover test.  A bool tensor (n, dh, dw) on the map's device."""
    h, w = int(src_hw[0]), int(src_hw[1])
    sx, sy = warp_map.xy[..., 0].to(torch.int32), warp_map.xy[..., 1].to(torch.int32)
    edge = 1 if warp_map.interp == 1 else 0  # (bilinear: the taps sx + 1, sy + 1 are source pixels too)
    return (sx >= 0) & (sx < w - edge) & (sy >= 0) & (sy < h - edge)


def overlap_stats(frames, warp_maps):
    """What the gain estimate needs of a site, as exact integers.

    frames     one (H_k, W_k, 3) or (B, H_k, W_k, 3) uint8 CUDA tensor per camera (one B).
    warp_maps  the cameras' WarpMaps (n == 1 or B, one dsize).
    Each camera's BEV comes from one remap(..., BORDER_TRANSPARENT) into zeros, its cover mask from cover_mask.
    Returns (N, S), int64 CPU tensors: N[i][j] the canvas pixels (summed over the batch) that cameras i and j both cover (N[i][i]: camera
    i's own cover), and S[i][j][c] the sum of camera i's channel c over those pixels."""
    from bev_amd import warp
    frames, warp_maps = list(frames), list(warp_maps)
    if not frames or len(frames) != len(warp_maps):
        raise ValueError("overlap_stats needs one WarpMap per camera, got %d maps for %d cameras" % (len(warp_maps), len(frames)))
    bevs, masks = [], []
    for f, m in zip(frames, warp_maps):
        if not isinstance(f, torch.Tensor) or f.dtype != torch.uint8 or f.dim() not in (3, 4) or f.shape[-1] != 3:
            raise ValueError("overlap_stats needs uint8 tensors (H, W, 3) or (B, H, W, 3)")
        f4 = f if f.dim() == 4 else f[None]
        bevs.append(warp.remap(f4, m, border_mode=warp.BORDER_TRANSPARENT).to(torch.int64))
        masks.append(cover_mask(m, f4.shape[1:3]).expand(f4.shape[0], -1, -1))
    n = len(frames)
    N, S = torch.zeros((n, n), dtype=torch.int64), torch.zeros((n, n, 3), dtype=torch.int64)
    for i in range(n):
        for j in range(n):
            both = masks[i] & masks[j]
            N[i, j] = int(both.sum())
            S[i, j] = (bevs[i] * both[..., None]).sum(dim=(0, 1, 2)).cpu()
    return N, S


def solve_gains(N, S, alpha=0.01, beta=100.0, per_channel=True):
    """Brown and Lowe's gain compensation as OpenCV's GainCompensator sets it up (restated; parity with OpenCV is not pinned): the gains
    g that minimise  sum_ij N_ij (alpha (g_i I_ij - g_j I_ji)^2 + beta (1 - g_i)^2)  with I_ij = S_ij / N_ij the mean of camera i over
    its overlap with camera j.  The linear system, in float64:

        b_i  += beta N_ij,  A_ii += beta N_ij                               for every j (j == i included)
        A_ii += 2 alpha I_ij^2 N_ij,  A_ij -= 2 alpha I_ij I_ji N_ij        for j != i

    N (n, n), S (n, n, 3): overlap_stats' results (anything numpy reads).  per_channel: one solve per channel -- this also evens out white
    balance -- or one solve on the channel mean.  Returns a float64 array (n, 3); a camera that covers nothing gets 1."""
    N = np.asarray(N, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    n = N.shape[0]
    if N.shape != (n, n) or S.shape != (n, n, 3):
        raise ValueError("N must be (n, n) and S (n, n, 3), got %s and %s" % (N.shape, S.shape))
    I = S / np.maximum(N, 1.0)[..., None]  # noqa: E741  (no overlap: N = 0 takes the pair out of every sum)
    if not per_channel:
        I = I.mean(axis=2, keepdims=True)  # noqa: E741
    out = np.ones((n, I.shape[2]))
    for c in range(I.shape[2]):
        A, b = np.zeros((n, n)), np.zeros(n)
        for i in range(n):
            for j in range(n):
                b[i] += beta * N[i, j]
                A[i, i] += beta * N[i, j]
                if j != i:
                    A[i, i] += 2.0 * alpha * I[i, j, c] ** 2 * N[i, j]
                    A[i, j] -= 2.0 * alpha * I[i, j, c] * I[j, i, c] * N[i, j]
        seen = A.diagonal() > 0  # (a camera that covers nothing has an empty row: its gain stays 1)
        if seen.any():
            out[seen, c] = np.linalg.solve(A[np.ix_(seen, seen)], b[seen])
    return np.ascontiguousarray(np.broadcast_to(out, (n, 3)))


def estimate_gains(frames, warp_maps, alpha=0.01, beta=100.0, per_channel=True):
    """overlap_stats, then solve_gains, clipped to what the stitches take ([0, 1023 / 256]): the `gains=` of remap_stitch* and
    SitePipeline.set_gains for this light."""
    N, S = overlap_stats(frames, warp_maps)
    return np.clip(solve_gains(N.numpy(), S.numpy(), alpha, beta, per_channel), 0.0, GAIN_MAX / 256.0)
