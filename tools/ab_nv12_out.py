#!/usr/bin/env python3
"""The warps into NV12 (bevwarp_warp_to_nv12, bevwarp_warp_nv12_to_nv12) against the kernels they share their frame with, on BASELINE
configs[1] -- 32 x 1080p -> 1024^2, per-frame jitter_H matrices, bilinear -- with the keystone footprint and the Brno-like BEV
(synth_brno_H):

    (a) bevwarp_warp               on the BGR frames, plain launch (caller-owned matrices, so no verdict tables)
    (b) bevwarp_warp_border        BORDER_TRANSPARENT on the same frames: the flat frame on a BGR source
    (c) bevwarp_warp_nv12          on the same frames as NV12
    (d) bevwarp_warp_to_nv12       BGR frames in, NV12 BEV out: shares frame, coordinate chain and tap loads with (b)
    (e) bevwarp_warp_nv12_to_nv12  NV12 frames in, NV12 BEV out: shares them with (c)

(a)-(c) are the yardstick.  Condition, set before the first run: (d)'s p10 does not lie above (b)'s p90, nor (e)'s above (c)'s, on both
footprints; the ratios to (a) are reported only.  All arms run interleaved in one process after a warm-up, three buffer sets rotated past
the Infinity Cache as bench.py does; HIP-event time per launch, 70 launches per arm.  `--step pipeline`: FramePipeline (pinned ring of
depth 3) over 200 frames of 1080p, every source format into BGR and into NV12 slots, alternated: ms per frame, reported only.
GPU box, each step under a time limit of its own and none tried again when it fails:
    timeout -k 10 400 python tools/ab_nv12_out.py --step kernels --out profiles/nv12_out_timing.txt && \\
    timeout -k 10 300 python tools/ab_nv12_out.py --step pipeline --out profiles/nv12_out_timing.txt --append"""
import numpy as np
import torch

import arms
from arms import B, D, SH, SW, pipeline_ms, to_nv12
from bev_amd import warp
from bev_amd.pipeline import FramePipeline
from tests import workloads as wl

ARMS = {"warp": "(a) bevwarp_warp BGR, plain launch", "transparent": "(b) warp_border TRANSPARENT BGR", "nv12": "(c) bevwarp_warp_nv12",
        "to_nv12": "(d) bevwarp_warp_to_nv12", "nv12_to_nv12": "(e) bevwarp_warp_nv12_to_nv12"}


def kernels(quick, dev):
    rounds, per_round, warm = arms.counts(quick)
    lines = ["# warps into NV12 vs bevwarp_warp, bevwarp_warp_border (TRANSPARENT) and bevwarp_warp_nv12, %d x %dx%d -> %dx%d, uint8, bilinear, per-frame jitter_H; us per launch"
             % (B, SW, SH, D, D), "# %d rounds x %d launches per arm, arms interleaved; (a) is the plain launch, no verdict tables; %s" % (rounds, per_round, torch.cuda.get_device_name(dev))]
    nset = 3  # (3 x 199 MB of BGR sources, 3 x 100 MB of NV12 -- with the destinations past the 256 MB Infinity Cache)
    bgr = arms.frame_sets(nset, dev)
    planes = [warp.split_nv12(to_nv12(t)) for t in bgr]
    outs = arms.dest_sets(nset, dev)
    outs_nv12 = arms.dest_sets(nset, dev, (B, D * 3 // 2, D))
    verdicts = []
    for hname, _, Ms in arms.footprints():
        minv = warp.device_inverse(Ms, dev).clone()  # (caller-owned: the plain launch)
        k = [0]

        def launch(arm):
            i = k[0] % nset
            if arm == "nv12":
                warp.warp_perspective_nv12(planes[i][0], planes[i][1], None, (D, D), flags=warp.INTER_LINEAR, out=outs[i], M_inv_device=minv)
            elif arm == "to_nv12":
                warp.warp_perspective_to_nv12(bgr[i], None, (D, D), flags=warp.INTER_LINEAR, out=outs_nv12[i], M_inv_device=minv)
            elif arm == "nv12_to_nv12":
                warp.warp_nv12_to_nv12(planes[i][0], planes[i][1], None, (D, D), flags=warp.INTER_LINEAR, out=outs_nv12[i], M_inv_device=minv)
            else:
                warp.warp_perspective(bgr[i], None, (D, D), flags=warp.INTER_LINEAR, out=outs[i], M_inv_device=minv,
                                      border_mode=warp.BORDER_TRANSPARENT if arm == "transparent" else warp.BORDER_CONSTANT)
            k[0] += 1

        q = arms.p10_50_90(arms.timed(ARMS, launch, rounds, per_round, warm))
        for arm, label in ARMS.items():
            lines.append("%-9s %-36s median %9.1f us  p10 %9.1f  p90 %9.1f  ratio to (a) %5.2f" % (hname, label, q[arm][1], q[arm][0], q[arm][2], q[arm][1] / q["warp"][1]))
        for new, old, tag in (("to_nv12", "transparent", "(d) p10 <= (b) p90"), ("nv12_to_nv12", "nv12", "(e) p10 <= (c) p90")):
            p10, p90 = q[new][0], q[old][2]
            verdicts.append("condition %-9s %s: %9.1f <= %9.1f  %s" % (hname, tag, p10, p90, "holds" if p10 <= p90 else "REFUTED"))
    return lines + verdicts


def pipeline(quick):
    n = 20 if quick else 200
    M = wl.synth_brno_H(SW, SH, D, D)
    frame_bgr = wl.frame(0, SH, SW, np.uint8)
    frame_nv12 = to_nv12(torch.from_numpy(frame_bgr)[None])[0].numpy()
    lines = ["# FramePipeline, %d frames %dx%d -> %dx%d, depth 3, Brno-like BEV: ms per frame (host clock around the loop), 3 repeats, arms alternated" % (n, SW, SH, D, D)]
    combos = [(s, d) for s in ("nv12", "bgr") for d in ("bgr", "nv12")]
    ms = {c: [] for c in combos}
    for _ in range(3):
        for src, dst in combos:
            with FramePipeline((SH, SW), 3, M, (D, D), depth=3, src_format=src, dst_format=dst) as pipe:
                ms[src, dst].append(pipeline_ms(pipe, frame_nv12 if src == "nv12" else frame_bgr, n))
    for src, dst in combos:
        up, down = (frame_nv12 if src == "nv12" else frame_bgr).nbytes, D * D * (3 if dst == "bgr" else 1.5)
        lines.append("pipeline  src_format=%-5s dst_format=%-5s upload %5.2f MB/frame  download %5.2f MB/frame   ms per frame  median %7.4f  min %7.4f  max %7.4f" % (
            src, dst, up / 1e6, down / 1e6, float(np.median(ms[src, dst])), min(ms[src, dst]), max(ms[src, dst])))
    for src in ("nv12", "bgr"):
        lines.append("pipeline  src_format=%-5s nv12 out / bgr out  %5.3f" % (src, float(np.median(ms[src, "nv12"])) / float(np.median(ms[src, "bgr"]))))
    return lines


def main():
    a = arms.parser(__doc__, steps=("kernels", "pipeline", "all"), step="all").parse_args()
    lines = []
    if a.step in ("kernels", "all"):
        lines += kernels(a.quick, torch.device("cuda", 0))
        torch.cuda.empty_cache()
    if a.step in ("pipeline", "all"):
        lines += pipeline(a.quick)
    arms.finish(lines, a.out, a.append)


if __name__ == "__main__":
    main()
