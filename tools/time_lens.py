#!/usr/bin/env python3
"""The lens warp (bevwarp_warp_lens) against the same frame without the lens maths (bevwarp_warp_border, TRANSPARENT) and against the
constant-border product kernel (bevwarp_warp, what bench.py times) on BASELINE configs[1] -- 32 x 1080p -> 1024^2, per-frame jitter_H
matrices, uint8 RGB, bilinear -- with the keystone footprint and the Brno-like BEV (synth_brno_H).  The lens is the tests' lens A on the
tests' camera matrix at 1080p, r2_max = lens_valid_r2.  The three arms call the C ABI with bound arguments, interleaved in one process
after a warm-up, buffer sets rotated past the Infinity Cache; HIP-event time per launch, p10 / p50 / p90, and the two ratios.
Next to them the cost the lens warp replaces: a separate undistortion pass reads and writes every frame once -- at least that many
bytes at the box's streaming copy rate (profiles/r01_hbm_ceiling.txt), computed from the byte count, not measured.
GPU box:  python tools/time_lens.py [--quick] [--out FILE]"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bev_amd import _lib, warp  # noqa: E402
from tests import workloads as wl  # noqa: E402

LENS_A = (-0.30, 0.10, 0.001, -0.0005, -0.01)
COPY_RATE = 5.07e12  # bytes per second read + written by a streaming copy (profiles/r01_hbm_ceiling.txt)
ARMS = ("lens", "border_transparent", "warp")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--quick", action="store_true", help="a few launches per arm (for a profiler run)")
    p.add_argument("--out", default=None, help="also write the table to this file")
    a = p.parse_args()
    B, SH, SW, D, C = 32, 1080, 1920, 1024, 3
    rounds, per_round, warm = (2, 3, 2) if a.quick else (7, 10, 5)
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    K = np.array([[0.8 * SW, 0, (SW - 1) / 2], [0, 0.816 * SW, (SH - 1) / 2 + 3], [0, 0, 1.0]])
    lens = np.ascontiguousarray(np.concatenate([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]], LENS_A, [0.0, 0.0, 0.0]]))
    r2_max = warp.lens_valid_r2(LENS_A)
    border = np.zeros(C)
    nset = 3  # (3 x 199 MB of sources, 3 x 101 MB of destinations -- past the 256 MB Infinity Cache)
    srcs = [torch.from_numpy(np.stack([wl.frame(B * s + i, SH, SW, np.uint8) for i in range(B)])).to(dev) for s in range(nset)]
    outs = [torch.zeros((B, D, D, C), dtype=torch.uint8, device=dev) for _ in range(nset)]
    undistort_us = 2 * B * SH * SW * C / COPY_RATE * 1e6
    lines = ["# bevwarp_warp_lens vs bevwarp_warp_border (TRANSPARENT) vs bevwarp_warp, %d x %dx%dx%d -> %dx%dx%d, uint8, bilinear, per-frame jitter_H; us per launch"
             % (B, SW, SH, C, D, D, C), "# lens A %s, r2_max %.4f; %d rounds x %d launches per arm, arms interleaved; %s"
             % (LENS_A, r2_max, rounds, per_round, torch.cuda.get_device_name(dev)),
             "# a separate undistortion pass: %d frames x %d bytes read + written = %.1f MB, %.1f us at %.2f TB/s (computed, not measured)"
             % (B, SH * SW * C, 2 * B * SH * SW * C / 1e6, undistort_us, COPY_RATE / 1e12)]
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for hname, hfn in (("keystone", wl.keystone_H), ("brno", wl.synth_brno_H)):
        H = hfn(SW, SH, D, D)
        Ms = np.stack([wl.jitter_H(H, i) for i in range(B)])
        minv = torch.from_numpy(warp.invert_homography(Ms)).to(dev)
        mray = torch.from_numpy(np.ascontiguousarray(warp.ray_matrix(Ms, K))).to(dev)
        k = [0]

        def launch(arm):
            i = k[0] % nset
            k[0] += 1
            head = (srcs[i].data_ptr(), outs[i].data_ptr(), B, SH, SW, D, D, C, SH * SW * C, SW * C, D * D * C, D * C)
            if arm == "lens":
                st = lib.bevwarp_warp_lens(*head, mray.data_ptr(), B, lens.ctypes.data_as(ctypes.c_void_p), r2_max, _lib.U8, 1, warp.BORDER_CONSTANT,
                                           border.ctypes.data_as(ctypes.c_void_p), stream)
            elif arm == "border_transparent":
                st = lib.bevwarp_warp_border(*head, minv.data_ptr(), B, _lib.U8, 1, warp.BORDER_TRANSPARENT, None, stream)
            else:
                st = lib.bevwarp_warp(*head, minv.data_ptr(), B, _lib.U8, 1, border.ctypes.data_as(ctypes.c_void_p), stream)
            _lib.check(st)

        for arm in ARMS:
            for _ in range(warm):
                launch(arm)
        torch.cuda.synchronize()
        t = {arm: [] for arm in ARMS}
        for _ in range(rounds):
            for arm in ARMS:
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(per_round)]
                for e0, e1 in ev:
                    e0.record()
                    launch(arm)
                    e1.record()
                torch.cuda.synchronize()
                t[arm] += [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
        p50 = {arm: float(np.median(t[arm])) for arm in ARMS}
        for arm in ARMS:
            lines.append("%-9s %-19s p10 %8.1f  p50 %8.1f  p90 %8.1f us  (%d launches)" % (hname, arm, np.percentile(t[arm], 10), p50[arm], np.percentile(t[arm], 90), len(t[arm])))
        lines.append("%-9s lens / border_transparent %5.2f   lens / warp %5.2f   warp + undistortion pass %8.1f us -> one pass %s (%.2f)"
                     % (hname, p50["lens"] / p50["border_transparent"], p50["lens"] / p50["warp"], p50["warp"] + undistort_us,
                        "wins" if p50["lens"] < p50["warp"] + undistort_us else "loses", p50["lens"] / (p50["warp"] + undistort_us)))
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
