#!/usr/bin/env python3
"""The border modes' kernel (bevwarp_warp_border) against the constant-border product kernel (bevwarp_warp, what bench.py times)
on BASELINE configs[1] -- 32 x 1080p -> 1024^2, per-frame jitter_H matrices -- with the keystone footprint and the Brno-like BEV
(synth_brno_H), uint8 and float32 RGB, bilinear.  All arms run interleaved in one process after a warm-up, buffer sets rotated
past the Infinity Cache; HIP-event time per launch, median and the ratio to CONSTANT.
GPU box:  python tools/time_border.py [--quick] [--out FILE]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bev_amd import warp  # noqa: E402
from tests import workloads as wl  # noqa: E402

ARMS = [("CONSTANT", warp.BORDER_CONSTANT), ("REPLICATE", warp.BORDER_REPLICATE), ("REFLECT", warp.BORDER_REFLECT), ("WRAP", warp.BORDER_WRAP),
        ("REFLECT_101", warp.BORDER_REFLECT_101), ("TRANSPARENT", warp.BORDER_TRANSPARENT)]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--quick", action="store_true", help="a few launches per arm (for a profiler run)")
    p.add_argument("--out", default=None, help="also write the table to this file")
    a = p.parse_args()
    B, SH, SW, D = 32, 1080, 1920, 1024
    rounds, per_round, warm = (2, 3, 2) if a.quick else (7, 10, 5)
    dev = torch.device("cuda", 0)
    lines = ["# bevwarp_warp_border vs bevwarp_warp (CONSTANT), %d x %dx%dx3 -> %dx%dx3, bilinear, per-frame jitter_H; median us per launch"
             % (B, SW, SH, D, D), "# %d rounds x %d launches per arm, arms interleaved; %s" % (rounds, per_round, torch.cuda.get_device_name(dev))]
    for dtype in (np.uint8, np.float32):
        nset = 3 if dtype == np.uint8 else 2  # (u8: 3 x 199 MB of sources, f32: 2 x 796 MB -- past the 256 MB Infinity Cache)
        srcs = [torch.from_numpy(np.stack([wl.frame(B * s + i, SH, SW, dtype) for i in range(B)])).to(dev) for s in range(nset)]
        outs = [torch.zeros((B, D, D, 3), dtype=srcs[0].dtype, device=dev) for _ in range(nset)]
        for hname, hfn in (("keystone", wl.keystone_H), ("brno", wl.synth_brno_H)):
            H = hfn(SW, SH, D, D)
            minv = warp.device_inverse(np.stack([wl.jitter_H(H, i) for i in range(B)]), dev).clone()  # (caller-owned: the plain launch)
            k = [0]

            def launch(mode):
                i = k[0] % nset
                warp.warp_perspective(srcs[i], None, (D, D), flags=warp.INTER_LINEAR, out=outs[i], M_inv_device=minv, border_mode=mode)
                k[0] += 1

            for _, mode in ARMS:
                for _ in range(warm):
                    launch(mode)
            torch.cuda.synchronize()
            t = {name: [] for name, _ in ARMS}
            for _ in range(rounds):
                for name, mode in ARMS:
                    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(per_round)]
                    for e0, e1 in ev:
                        e0.record()
                        launch(mode)
                        e1.record()
                    torch.cuda.synchronize()
                    t[name] += [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
            base = float(np.median(t["CONSTANT"]))
            for name, _ in ARMS:
                med = float(np.median(t[name]))
                lines.append("%-8s %-9s %-12s median %9.1f us  p10 %9.1f  p90 %9.1f  ratio to CONSTANT %5.2f" % (
                    np.dtype(dtype).name, hname, name, med, np.percentile(t[name], 10), np.percentile(t[name], 90), med / base))
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
