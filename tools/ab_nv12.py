#!/usr/bin/env python3
"""The NV12 warp (bevwarp_warp_nv12) against the warps of the converted BGR frames, on BASELINE configs[1] -- 32 x 1080p -> 1024^2,
per-frame jitter_H matrices, bilinear -- with the keystone footprint and the Brno-like BEV (synth_brno_H):

    (a) bevwarp_warp          on the BGR frames, plain launch (caller-owned matrices, so no verdict tables): the yardstick
    (b) bevwarp_warp_border   BORDER_TRANSPARENT on the same frames: the kernel whose structure the NV12 kernel shares
    (c) bevwarp_warp_nv12     on the same frames as NV12 (1.5 bytes per source pixel instead of 3)

All arms run interleaved in one process after a warm-up, buffer sets rotated past the Infinity Cache as bench.py does; HIP-event time per
launch, median.  Then FramePipeline (pinned ring of depth 3, upload and warp overlapped, BEV frames stored into pinned host slots) over 200
frames of 1080p, BGR slots against NV12 slots: ms per frame.
GPU box:  python tools/ab_nv12.py [--quick] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bev_amd import warp  # noqa: E402
from bev_amd.pipeline import FramePipeline  # noqa: E402
from tests import workloads as wl  # noqa: E402


def to_nv12(bgr):
    """(B, H, W, 3) uint8 BGR on the device -> (B, H * 3 / 2, W) NV12: BT.601 limited range, chroma averaged over 2 x 2 (a stand-in for an
    encoder, so that the NV12 arm reads frames with the statistics of the BGR arm's; the timing does not depend on the values)."""
    f = bgr.float()
    b, g, r = f[..., 0], f[..., 1], f[..., 2]
    y = (0.257 * r + 0.504 * g + 0.098 * b + 16.0).round().clamp(0, 255)
    u = (-0.148 * r - 0.291 * g + 0.439 * b + 128.0)
    v = (0.439 * r - 0.368 * g - 0.071 * b + 128.0)
    B, H, W = y.shape
    pool = lambda p: p.reshape(B, H // 2, 2, W // 2, 2).mean(dim=(2, 4)).round().clamp(0, 255)  # noqa: E731
    uv = torch.stack([pool(u), pool(v)], dim=-1).reshape(B, H // 2, W)
    return torch.cat([y, uv], dim=1).to(torch.uint8).contiguous()


def pipeline_ms(pipe, frame, n):
    for _ in range(3):  # fill the slots once: afterwards the "decoder" finds its frame already in pinned memory (zero-copy ingest)
        pipe.next_input()[...] = frame
        pipe.commit()
    for _ in range(3):
        pipe.result()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        pipe.next_input()
        pipe.commit()
        if pipe.ready() >= 3:
            pipe.result()
    while pipe.ready():
        pipe.result()
    return (time.perf_counter() - t0) / n * 1e3


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--quick", action="store_true", help="a few launches per arm (for a profiler run)")
    p.add_argument("--out", default=None, help="also write the table to this file")
    a = p.parse_args()
    B, SH, SW, D = 32, 1080, 1920, 1024
    rounds, per_round, warm = (2, 3, 2) if a.quick else (7, 10, 5)
    dev = torch.device("cuda", 0)
    lines = ["# bevwarp_warp_nv12 vs bevwarp_warp and bevwarp_warp_border (TRANSPARENT), %d x %dx%d -> %dx%dx3, uint8, bilinear, per-frame jitter_H; median us per launch"
             % (B, SW, SH, D, D), "# %d rounds x %d launches per arm, arms interleaved; (a) is the plain launch, no verdict tables; %s" % (rounds, per_round, torch.cuda.get_device_name(dev))]
    nset = 3  # (3 x 199 MB of BGR sources, 3 x 100 MB of NV12 -- with the destinations past the 256 MB Infinity Cache)
    bgr = [torch.from_numpy(np.stack([wl.frame(B * s + i, SH, SW, np.uint8) for i in range(B)])).to(dev) for s in range(nset)]
    nv12 = [to_nv12(t) for t in bgr]
    planes = [warp.split_nv12(t) for t in nv12]
    outs = [torch.zeros((B, D, D, 3), dtype=torch.uint8, device=dev) for _ in range(nset)]
    for hname, hfn in (("keystone", wl.keystone_H), ("brno", wl.synth_brno_H)):
        H = hfn(SW, SH, D, D)
        minv = warp.device_inverse(np.stack([wl.jitter_H(H, i) for i in range(B)]), dev).clone()  # (caller-owned: the plain launch)
        k = [0]

        def launch(arm):
            i = k[0] % nset
            if arm == "nv12":
                warp.warp_perspective_nv12(planes[i][0], planes[i][1], None, (D, D), flags=warp.INTER_LINEAR, out=outs[i], M_inv_device=minv)
            else:
                warp.warp_perspective(bgr[i], None, (D, D), flags=warp.INTER_LINEAR, out=outs[i], M_inv_device=minv,
                                      border_mode=warp.BORDER_TRANSPARENT if arm == "transparent" else warp.BORDER_CONSTANT)
            k[0] += 1

        arms = ("warp", "transparent", "nv12")
        for arm in arms:
            for _ in range(warm):
                launch(arm)
        torch.cuda.synchronize()
        t = {arm: [] for arm in arms}
        for _ in range(rounds):
            for arm in arms:
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(per_round)]
                for e0, e1 in ev:
                    e0.record()
                    launch(arm)
                    e1.record()
                torch.cuda.synchronize()
                t[arm] += [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
        base = float(np.median(t["warp"]))
        for arm, label in zip(arms, ("(a) bevwarp_warp BGR, plain launch", "(b) warp_border TRANSPARENT BGR", "(c) bevwarp_warp_nv12")):
            med = float(np.median(t[arm]))
            lines.append("%-9s %-36s median %9.1f us  p10 %9.1f  p90 %9.1f  ratio to (a) %5.2f" % (
                hname, label, med, np.percentile(t[arm], 10), np.percentile(t[arm], 90), med / base))
    frame_bgr, frame_nv12 = bgr[0][0].cpu().numpy(), nv12[0][0].cpu().numpy()
    del bgr, nv12, planes, outs
    torch.cuda.empty_cache()

    # the ingest path: upload + warp + BEV frame into a pinned host slot, per frame
    n = 20 if a.quick else 200
    M = wl.synth_brno_H(SW, SH, D, D)
    lines.append("# FramePipeline, %d frames %dx%d -> %dx%d, depth 3, Brno-like BEV: ms per frame (host clock around the loop), 3 repeats, arms alternated" % (n, SW, SH, D, D))
    ms = {"bgr": [], "nv12": []}
    for _ in range(3):
        for fmt, frame in (("bgr", frame_bgr), ("nv12", frame_nv12)):
            with FramePipeline((SH, SW), 3, M, (D, D), depth=3, src_format=fmt) as pipe:
                ms[fmt].append(pipeline_ms(pipe, frame, n))
    for fmt, nbytes in (("bgr", frame_bgr.nbytes), ("nv12", frame_nv12.nbytes)):
        lines.append("pipeline  src_format=%-5s upload %5.2f MB/frame   ms per frame  median %7.4f  min %7.4f  max %7.4f" % (
            fmt, nbytes / 1e6, float(np.median(ms[fmt])), min(ms[fmt]), max(ms[fmt])))
    lines.append("pipeline  nv12 / bgr  %5.3f" % (float(np.median(ms["nv12"])) / float(np.median(ms["bgr"]))))
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
