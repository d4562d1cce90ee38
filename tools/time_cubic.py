#!/usr/bin/env python3
"""The bicubic kernel (bevwarp_warp_border, interp = BEVWARP_CUBIC) against the bilinear kernels on BASELINE configs[1] -- 32 x 1080p ->
1024^2 RGB, per-frame jitter_H matrices, the keystone footprint -- uint8 and float32.  Arms: bilinear CONSTANT (warp_rows, what bench.py
times), bilinear REPLICATE (the border kernel: the yardstick, 16 taps against its 4), then bicubic CONSTANT, REPLICATE, REFLECT_101 and
TRANSPARENT.  All arms run interleaved in one process after a warm-up, buffer sets rotated past the Infinity Cache; HIP-event time per
launch, median and the ratio to bilinear REPLICATE.
GPU box:  python tools/time_cubic.py [--quick] [--out FILE]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bev_amd import warp  # noqa: E402
from tests import workloads as wl  # noqa: E402

ARMS = [("linear CONSTANT", warp.INTER_LINEAR, warp.BORDER_CONSTANT), ("linear REPLICATE", warp.INTER_LINEAR, warp.BORDER_REPLICATE),
        ("cubic CONSTANT", warp.INTER_CUBIC, warp.BORDER_CONSTANT), ("cubic REPLICATE", warp.INTER_CUBIC, warp.BORDER_REPLICATE),
        ("cubic REFLECT_101", warp.INTER_CUBIC, warp.BORDER_REFLECT_101), ("cubic TRANSPARENT", warp.INTER_CUBIC, warp.BORDER_TRANSPARENT)]
YARDSTICK = "linear REPLICATE"


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--quick", action="store_true", help="a few launches per arm (for a profiler run)")
    p.add_argument("--out", default=None, help="also write the table to this file")
    a = p.parse_args()
    B, SH, SW, D = 32, 1080, 1920, 1024
    rounds, per_round, warm = (2, 3, 2) if a.quick else (7, 10, 5)
    dev = torch.device("cuda", 0)
    lines = ["# bicubic (bevwarp_warp_border, interp 2) vs bilinear, %d x %dx%dx3 -> %dx%dx3, keystone, per-frame jitter_H; median us per launch"
             % (B, SW, SH, D, D), "# %d rounds x %d launches per arm, arms interleaved; %s" % (rounds, per_round, torch.cuda.get_device_name(dev))]
    H = wl.keystone_H(SW, SH, D, D)
    for dtype in (np.uint8, np.float32):
        nset = 3 if dtype == np.uint8 else 2  # (u8: 3 x 199 MB of sources, f32: 2 x 796 MB -- past the 256 MB Infinity Cache)
        srcs = [torch.from_numpy(np.stack([wl.frame(B * s + i, SH, SW, dtype) for i in range(B)])).to(dev) for s in range(nset)]
        outs = [torch.zeros((B, D, D, 3), dtype=srcs[0].dtype, device=dev) for _ in range(nset)]
        minv = warp.device_inverse(np.stack([wl.jitter_H(H, i) for i in range(B)]), dev).clone()  # (caller-owned: the plain launch)
        k = [0]

        def launch(flags, mode):
            i = k[0] % nset
            warp.warp_perspective(srcs[i], None, (D, D), flags=flags, out=outs[i], M_inv_device=minv, border_mode=mode)
            k[0] += 1

        for _, flags, mode in ARMS:
            for _ in range(warm):
                launch(flags, mode)
        torch.cuda.synchronize()
        t = {name: [] for name, _, _ in ARMS}
        for _ in range(rounds):
            for name, flags, mode in ARMS:
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(per_round)]
                for e0, e1 in ev:
                    e0.record()
                    launch(flags, mode)
                    e1.record()
                torch.cuda.synchronize()
                t[name] += [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
        base = float(np.median(t[YARDSTICK]))
        for name, _, _ in ARMS:
            med = float(np.median(t[name]))
            lines.append("%-8s %-18s median %9.1f us  p10 %9.1f  p90 %9.1f  ratio to %s %5.2f" % (
                np.dtype(dtype).name, name, med, np.percentile(t[name], 10), np.percentile(t[name], 90), YARDSTICK, med / base))
        del srcs, outs
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
