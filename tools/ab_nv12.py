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
import numpy as np
import torch

import arms
from arms import B, D, SH, SW
from bev_amd import warp
from bev_amd.pipeline import FramePipeline
from tests import workloads as wl

ARMS = {"warp": "(a) bevwarp_warp BGR, plain launch", "transparent": "(b) warp_border TRANSPARENT BGR", "nv12": "(c) bevwarp_warp_nv12"}


def main():
    a = arms.parser(__doc__).parse_args()
    rounds, per_round, warm = arms.counts(a.quick)
    dev = torch.device("cuda", 0)
    lines = ["# bevwarp_warp_nv12 vs bevwarp_warp and bevwarp_warp_border (TRANSPARENT), %d x %dx%d -> %dx%dx3, uint8, bilinear, per-frame jitter_H; median us per launch"
             % (B, SW, SH, D, D), "# %d rounds x %d launches per arm, arms interleaved; (a) is the plain launch, no verdict tables; %s" % (rounds, per_round, torch.cuda.get_device_name(dev))]
    nset = 3  # (3 x 199 MB of BGR sources, 3 x 100 MB of NV12 -- with the destinations past the 256 MB Infinity Cache)
    bgr = arms.frame_sets(nset, dev)
    nv12 = [arms.to_nv12(t) for t in bgr]
    planes = [warp.split_nv12(t) for t in nv12]
    outs = arms.dest_sets(nset, dev)
    for hname, _, Ms in arms.footprints():
        minv = warp.device_inverse(Ms, dev).clone()  # (caller-owned: the plain launch)
        k = [0]

        def launch(arm):
            i = k[0] % nset
            if arm == "nv12":
                warp.warp_perspective_nv12(planes[i][0], planes[i][1], None, (D, D), flags=warp.INTER_LINEAR, out=outs[i], M_inv_device=minv)
            else:
                warp.warp_perspective(bgr[i], None, (D, D), flags=warp.INTER_LINEAR, out=outs[i], M_inv_device=minv,
                                      border_mode=warp.BORDER_TRANSPARENT if arm == "transparent" else warp.BORDER_CONSTANT)
            k[0] += 1

        q = arms.p10_50_90(arms.timed(ARMS, launch, rounds, per_round, warm))
        for arm, label in ARMS.items():
            lines.append("%-9s %-36s median %9.1f us  p10 %9.1f  p90 %9.1f  ratio to (a) %5.2f" % (hname, label, q[arm][1], q[arm][0], q[arm][2], q[arm][1] / q["warp"][1]))
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
                ms[fmt].append(arms.pipeline_ms(pipe, frame, n))
    for fmt, nbytes in (("bgr", frame_bgr.nbytes), ("nv12", frame_nv12.nbytes)):
        lines.append("pipeline  src_format=%-5s upload %5.2f MB/frame   ms per frame  median %7.4f  min %7.4f  max %7.4f" % (
            fmt, nbytes / 1e6, float(np.median(ms[fmt])), min(ms[fmt]), max(ms[fmt])))
    lines.append("pipeline  nv12 / bgr  %5.3f" % (float(np.median(ms["nv12"])) / float(np.median(ms["bgr"]))))
    arms.finish(lines, a.out)


if __name__ == "__main__":
    main()
