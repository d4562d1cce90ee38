#!/usr/bin/env python3
"""The border modes' kernel (bevwarp_warp_border) against the constant-border product kernel (bevwarp_warp, what bench.py times)
on BASELINE configs[1] -- 32 x 1080p -> 1024^2, per-frame jitter_H matrices -- with the keystone footprint and the Brno-like BEV
(synth_brno_H), uint8 and float32 RGB, bilinear.  All arms run interleaved in one process after a warm-up, buffer sets rotated
past the Infinity Cache; HIP-event time per launch, median and the ratio to CONSTANT.
GPU box:  python tools/time_border.py [--quick] [--out FILE]"""
import numpy as np
import torch

import arms
from arms import B, D, SH, SW
from bev_amd import warp

ARMS = {"CONSTANT": warp.BORDER_CONSTANT, "REPLICATE": warp.BORDER_REPLICATE, "REFLECT": warp.BORDER_REFLECT, "WRAP": warp.BORDER_WRAP,
        "REFLECT_101": warp.BORDER_REFLECT_101, "TRANSPARENT": warp.BORDER_TRANSPARENT}


def main():
    a = arms.parser(__doc__).parse_args()
    rounds, per_round, warm = arms.counts(a.quick)
    dev = torch.device("cuda", 0)
    lines = ["# bevwarp_warp_border vs bevwarp_warp (CONSTANT), %d x %dx%dx3 -> %dx%dx3, bilinear, per-frame jitter_H; median us per launch"
             % (B, SW, SH, D, D), "# %d rounds x %d launches per arm, arms interleaved; %s" % (rounds, per_round, torch.cuda.get_device_name(dev))]
    for dtype in (np.uint8, np.float32):
        nset = 3 if dtype == np.uint8 else 2  # (u8: 3 x 199 MB of sources, f32: 2 x 796 MB -- past the 256 MB Infinity Cache)
        srcs = arms.frame_sets(nset, dev, dtype)
        outs = arms.dest_sets(nset, dev, dtype=srcs[0].dtype)
        for hname, _, Ms in arms.footprints():
            minv = warp.device_inverse(Ms, dev).clone()  # (caller-owned: the plain launch)
            k = [0]

            def launch(name):
                i = k[0] % nset
                warp.warp_perspective(srcs[i], None, (D, D), flags=warp.INTER_LINEAR, out=outs[i], M_inv_device=minv, border_mode=ARMS[name])
                k[0] += 1

            q = arms.p10_50_90(arms.timed(ARMS, launch, rounds, per_round, warm))
            for name in ARMS:
                lines.append("%-8s %-9s %-12s median %9.1f us  p10 %9.1f  p90 %9.1f  ratio to CONSTANT %5.2f" % (
                    np.dtype(dtype).name, hname, name, q[name][1], q[name][0], q[name][2], q[name][1] / q["CONSTANT"][1]))
        del srcs, outs
        torch.cuda.empty_cache()
    arms.finish(lines, a.out)


if __name__ == "__main__":
    main()
