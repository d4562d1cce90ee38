#!/usr/bin/env python3
"""The stitches through warp maps under BEVWARP_STITCH_GAIN against the plain entries and against the route the flag replaces, on
tools/time_remap.py's protocol: 3 cameras x 32 x 1080p -> 32 x 1024^2, bilinear, the tests' lens A at 1080p in every map, the cameras
side by side with overlaps.  Arms, interleaved in one process after a warm-up, buffer sets rotated past the Infinity Cache, HIP-event time
per call, p10 / p50 / p90, for three cases -- BGR -> BGR "over", BGR -> BGR "feather" F = 64, NV12 -> float16 planes "over":
    plain    the entry without gains
    gained   the entry with per-camera, per-channel gains (one launch)
    route    bev_amd.exposure.apply_gains over every camera's frames, then the plain entry.  (NV12 frames have no such pass of their own: the
             arm gains a converted-size stand-in per camera, so it leaves out the conversion pass a real route would also pay.)
The calls go through bev_amd.warp with out=: the host runs ahead of the device after the first launch of a round, so the events bracket
device time.  Derived: gained p90 against route p10 (the expectation DESIGN.md section 4.24 judges) and gained / plain (against the
instruction-count prediction there).
GPU box:  python tools/time_stitch_gain.py [--quick] [--out FILE]"""
import numpy as np
import torch

import arms
from arms import B, D, LENS_A, SH, SW
from bev_amd import exposure, warp

GAINS = [[1.25, 0.8, 1.0], [0.5, 2.0, 3.5], [1.7, 1.0, 0.3]]
ARMS = ("plain", "gained", "route")


def main():
    a = arms.parser(__doc__).parse_args()
    N = 3
    rounds, per_round, warm = arms.counts(a.quick, (7, 10, 3))
    dev = torch.device("cuda", 0)
    _, H, _ = next(arms.footprints())  # (the keystone footprint)
    # the cameras look at thirds of the canvas that overlap: the keystone footprint shifted by -D / 3, 0, +D / 3
    maps = [arms.lens_map(np.array([[1.0, 0, (k - 1) * D / 3.0], [0, 1, 0], [0, 0, 1]]) @ H, dev) for k in range(N)]
    G = exposure.quantize_gains(GAINS, N)
    nset = 2  # (2 x 3 x 199 MB of sources, 2 x 101 MB of canvases -- past the 256 MB Infinity Cache)
    base = arms.frame_set(0, dev)
    bgr = [[base.roll(shifts=(N * s + k) * 37 + 1, dims=2) for k in range(N)] for s in range(nset)]  # (the workload's frames, shifted per camera and set)
    ys = [[torch.randint(16, 236, (B, SH, SW), dtype=torch.uint8, device=dev) for _ in range(N)] for _ in range(nset)]
    uvs = [[torch.randint(16, 241, (B, SH // 2, SW // 2, 2), dtype=torch.uint8, device=dev) for _ in range(N)] for _ in range(nset)]
    canvases = arms.dest_sets(nset, dev)
    planes = arms.dest_sets(nset, dev, (B, 3, D, D), torch.float16)
    cover = [float(exposure.cover_mask(m, (SH, SW)).float().mean()) for m in maps]
    lines = ["# remap_stitch* with gains= (BEVWARP_STITCH_GAIN) vs the plain entry vs apply_gains + the plain entry; %d cameras x %d x %dx%d -> %d x %dx%d, bilinear, lens A %s; "
             "us per call" % (N, B, SW, SH, B, D, D, LENS_A),
             "# cover per camera %s; gains %s; %d rounds x %d calls per arm, arms interleaved; %s"
             % (", ".join("%.2f" % c for c in cover), GAINS, rounds, per_round, torch.cuda.get_device_name(dev))]
    k = [0]

    def call(case, arm):
        i = k[0] % nset
        k[0] += 1
        gains = GAINS if arm == "gained" else None
        if case == "nv12_planes":
            if arm == "route":
                for c in range(N):
                    exposure.apply_gains(bgr[i][c], G[c])
            warp.remap_stitch_nv12_to_planar(ys[i], uvs[i], maps, out=planes[i], out_dtype=torch.float16, gains=gains)
        else:
            srcs = [exposure.apply_gains(bgr[i][c], G[c]) for c in range(N)] if arm == "route" else bgr[i]
            warp.remap_stitch(srcs, maps, blend="feather" if case == "bgr_feather64" else "over", feather=64, out=canvases[i], gains=gains)

    for case in ("bgr_over", "bgr_feather64", "nv12_planes"):
        t = arms.timed(ARMS, lambda arm: call(case, arm), rounds, per_round, warm)
        q = arms.p10_50_90(t)
        for arm in ARMS:
            lines.append("%-14s %-7s p10 %9.1f  p50 %9.1f  p90 %9.1f us  (%d calls)" % (case, arm, q[arm][0], q[arm][1], q[arm][2], len(t[arm])))
        lines.append("%-14s gained p90 %.1f %s route p10 %.1f   gained / plain %5.3f (p50)   route / gained %5.2f (p50)"
                     % (case, q["gained"][2], "<=" if q["gained"][2] <= q["route"][0] else ">", q["route"][0], q["gained"][1] / q["plain"][1], q["route"][1] / q["gained"][1]))
    arms.finish(lines, a.out)


if __name__ == "__main__":
    main()
