#!/usr/bin/env python3
"""The lens warp (bevwarp_warp_lens) against the same frame without the lens maths (bevwarp_warp_border, TRANSPARENT) and against the
constant-border product kernel (bevwarp_warp, what bench.py times) on BASELINE configs[1] -- 32 x 1080p -> 1024^2, per-frame jitter_H
matrices, uint8 RGB, bilinear -- with the keystone footprint and the Brno-like BEV (synth_brno_H).  The lens is the tests' lens A on the
tests' camera matrix at 1080p, r2_max = lens_valid_r2.  The three arms call the C ABI with bound arguments, interleaved in one process
after a warm-up, buffer sets rotated past the Infinity Cache; HIP-event time per launch, p10 / p50 / p90, and the two ratios.
Next to them the cost the lens warp replaces: a separate undistortion pass reads and writes every frame once -- at least that many
bytes at the box's streaming copy rate (profiles/r01_hbm_ceiling.txt), computed from the byte count, not measured.
GPU box:  python tools/time_lens.py [--quick] [--out FILE]"""
import ctypes

import numpy as np
import torch

import arms
from arms import B, C, D, LENS_A, SH, SW, ptr
from bev_amd import _lib, warp

COPY_RATE = 5.07e12  # bytes per second read + written by a streaming copy (profiles/r01_hbm_ceiling.txt)
ARMS = ("lens", "border_transparent", "warp")


def main():
    a = arms.parser(__doc__).parse_args()
    rounds, per_round, warm = arms.counts(a.quick)
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    K = arms.camera_K(SW, SH)
    lens = arms.lens_array(K, LENS_A)
    r2_max = warp.lens_valid_r2(LENS_A)
    border = np.zeros(C)
    nset = 3  # (3 x 199 MB of sources, 3 x 101 MB of destinations -- past the 256 MB Infinity Cache)
    srcs, outs = arms.frame_sets(nset, dev), arms.dest_sets(nset, dev)
    undistort_us = 2 * B * SH * SW * C / COPY_RATE * 1e6
    lines = ["# bevwarp_warp_lens vs bevwarp_warp_border (TRANSPARENT) vs bevwarp_warp, %d x %dx%dx%d -> %dx%dx%d, uint8, bilinear, per-frame jitter_H; us per launch"
             % (B, SW, SH, C, D, D, C), "# lens A %s, r2_max %.4f; %d rounds x %d launches per arm, arms interleaved; %s"
             % (LENS_A, r2_max, rounds, per_round, torch.cuda.get_device_name(dev)),
             "# a separate undistortion pass: %d frames x %d bytes read + written = %.1f MB, %.1f us at %.2f TB/s (computed, not measured)"
             % (B, SH * SW * C, 2 * B * SH * SW * C / 1e6, undistort_us, COPY_RATE / 1e12)]
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for hname, _, Ms in arms.footprints():
        minv = torch.from_numpy(warp.invert_homography(Ms)).to(dev)
        mray = torch.from_numpy(np.ascontiguousarray(warp.ray_matrix(Ms, K))).to(dev)
        k = [0]

        def launch(arm):
            i = k[0] % nset
            k[0] += 1
            head = (srcs[i].data_ptr(), outs[i].data_ptr(), B, SH, SW, D, D, C, SH * SW * C, SW * C, D * D * C, D * C)
            if arm == "lens":
                st = lib.bevwarp_warp_lens(*head, mray.data_ptr(), B, ptr(lens), r2_max, _lib.U8, 1, warp.BORDER_CONSTANT, ptr(border), stream)
            elif arm == "border_transparent":
                st = lib.bevwarp_warp_border(*head, minv.data_ptr(), B, _lib.U8, 1, warp.BORDER_TRANSPARENT, None, stream)
            else:
                st = lib.bevwarp_warp(*head, minv.data_ptr(), B, _lib.U8, 1, ptr(border), stream)
            _lib.check(st)

        t = arms.timed(ARMS, launch, rounds, per_round, warm)
        q = arms.p10_50_90(t)
        p50 = {arm: q[arm][1] for arm in ARMS}
        for arm in ARMS:
            lines.append("%-9s %-19s p10 %8.1f  p50 %8.1f  p90 %8.1f us  (%d launches)" % (hname, arm, q[arm][0], q[arm][1], q[arm][2], len(t[arm])))
        lines.append("%-9s lens / border_transparent %5.2f   lens / warp %5.2f   warp + undistortion pass %8.1f us -> one pass %s (%.2f)"
                     % (hname, p50["lens"] / p50["border_transparent"], p50["lens"] / p50["warp"], p50["warp"] + undistort_us,
                        "wins" if p50["lens"] < p50["warp"] + undistort_us else "loses", p50["lens"] / (p50["warp"] + undistort_us)))
    arms.finish(lines, a.out)


if __name__ == "__main__":
    main()
