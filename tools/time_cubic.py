#!/usr/bin/env python3
"""The bicubic kernel (bevwarp_warp_border, interp = BEVWARP_CUBIC) against the bilinear kernels on BASELINE configs[1] -- 32 x 1080p ->
1024^2 RGB, per-frame jitter_H matrices, the keystone footprint -- uint8 and float32.  Arms: bilinear CONSTANT (warp_rows, what bench.py
times), bilinear REPLICATE (the border kernel: the yardstick, 16 taps against its 4), then bicubic CONSTANT, REPLICATE, REFLECT_101 and
TRANSPARENT.  All arms run interleaved in one process after a warm-up, buffer sets rotated past the Infinity Cache; HIP-event time per
launch, median and the ratio to bilinear REPLICATE.
GPU box:  python tools/time_cubic.py [--quick] [--out FILE]"""
import numpy as np
import torch

import arms
from arms import B, D, SH, SW
from bev_amd import warp

ARMS = {"linear CONSTANT": (warp.INTER_LINEAR, warp.BORDER_CONSTANT), "linear REPLICATE": (warp.INTER_LINEAR, warp.BORDER_REPLICATE),
        "cubic CONSTANT": (warp.INTER_CUBIC, warp.BORDER_CONSTANT), "cubic REPLICATE": (warp.INTER_CUBIC, warp.BORDER_REPLICATE),
        "cubic REFLECT_101": (warp.INTER_CUBIC, warp.BORDER_REFLECT_101), "cubic TRANSPARENT": (warp.INTER_CUBIC, warp.BORDER_TRANSPARENT)}
YARDSTICK = "linear REPLICATE"


def main():
    a = arms.parser(__doc__).parse_args()
    rounds, per_round, warm = arms.counts(a.quick)
    dev = torch.device("cuda", 0)
    lines = ["# bicubic (bevwarp_warp_border, interp 2) vs bilinear, %d x %dx%dx3 -> %dx%dx3, keystone, per-frame jitter_H; median us per launch"
             % (B, SW, SH, D, D), "# %d rounds x %d launches per arm, arms interleaved; %s" % (rounds, per_round, torch.cuda.get_device_name(dev))]
    _, _, Ms = next(arms.footprints())  # (the keystone footprint)
    for dtype in (np.uint8, np.float32):
        nset = 3 if dtype == np.uint8 else 2  # (u8: 3 x 199 MB of sources, f32: 2 x 796 MB -- past the 256 MB Infinity Cache)
        srcs = arms.frame_sets(nset, dev, dtype)
        outs = arms.dest_sets(nset, dev, dtype=srcs[0].dtype)
        minv = warp.device_inverse(Ms, dev).clone()  # (caller-owned: the plain launch)
        k = [0]

        def launch(name):
            i = k[0] % nset
            warp.warp_perspective(srcs[i], None, (D, D), flags=ARMS[name][0], out=outs[i], M_inv_device=minv, border_mode=ARMS[name][1])
            k[0] += 1

        q = arms.p10_50_90(arms.timed(ARMS, launch, rounds, per_round, warm))
        for name in ARMS:
            lines.append("%-8s %-18s median %9.1f us  p10 %9.1f  p90 %9.1f  ratio to %s %5.2f" % (
                np.dtype(dtype).name, name, q[name][1], q[name][0], q[name][2], YARDSTICK, q[name][1] / q[YARDSTICK][1]))
        del srcs, outs
        torch.cuda.empty_cache()
    arms.finish(lines, a.out)


if __name__ == "__main__":
    main()
