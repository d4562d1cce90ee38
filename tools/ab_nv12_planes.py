#!/usr/bin/env python3
"""NV12 frames to normalised channel planes in one launch (bevwarp_warp_nv12_planes) against what it replaces, on BASELINE configs[1] --
32 x 1080p -> 1024^2, per-frame jitter_H matrices, bilinear, ImageNet scale and bias -- with the keystone footprint and the Brno-like BEV:

    (a)  bevwarp_warp_nv12 alone (8-bit BGR BEV frame): the same taps and blend, half the bytes the float16 planes store -- a lower bound
    (b)  bevwarp_warp_nv12_planes to float32, float16 and bfloat16 planes
    (c1) (a), then warp_to_planar of the BEV frame with the identity matrix, nearest, to float16 planes     } the two-pass routes,
    (c2) (a), then torch: permute / float / mul / add / half                                                } timed end to end

All arms run interleaved in one process after a warm-up, three buffer sets rotated past the Infinity Cache; HIP-event time per launch (per
pair of launches for (c)), 70 per arm; median, p10, p90.  The condition set beforehand: on both footprints the float16 and the bfloat16 arm
of (b) have a median below the median of the FASTER route of (c) in the same run.  The ratio of (b) to (a) is reported without a pass mark.
GPU box:  python tools/ab_nv12_planes.py [--quick] [--out FILE]"""
import numpy as np
import torch

import arms
from arms import B, D, SH, SW
from bev_amd import warp

MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
ARMS = {"nv12": "(a)  bevwarp_warp_nv12 (8-bit BGR)", torch.float32: "(b)  nv12_planes float32", torch.float16: "(b)  nv12_planes float16",
        torch.bfloat16: "(b)  nv12_planes bfloat16", "two_kernel": "(c1) nv12 + warp_to_planar identity f16", "two_torch": "(c2) nv12 + torch permute/float/mul/add/half"}


def main():
    a = arms.parser(__doc__).parse_args()
    rounds, per_round, warm = arms.counts(a.quick)
    dev = torch.device("cuda", 0)
    scale, bias = 1.0 / (255.0 * STD), -MEAN / STD
    lines = ["# bevwarp_warp_nv12_planes vs bevwarp_warp_nv12 and the two-pass routes, %d x %dx%d NV12 -> %dx%d x 3 planes, bilinear, per-frame jitter_H, ImageNet scale / bias"
             % (B, SW, SH, D, D), "# median us per launch (per pair of launches for (c)); %d rounds x %d launches per arm, arms interleaved, 3 buffer sets rotated; %s"
             % (rounds, per_round, torch.cuda.get_device_name(dev))]
    nset = 3
    # (the BGR frames are only the encoder stand-in's input: one set at a time)
    planes = [warp.split_nv12(arms.to_nv12(arms.frame_set(s, dev))) for s in range(nset)]
    bev = arms.dest_sets(nset, dev)
    outs = {dt: arms.dest_sets(nset, dev, (B, 3, D, D), dt) for dt in (torch.float32, torch.float16, torch.bfloat16)}
    eye = torch.eye(3, dtype=torch.float64, device=dev).reshape(1, 3, 3).contiguous()
    sc_t = torch.tensor(scale, dtype=torch.float32, device=dev).reshape(1, 3, 1, 1)
    bi_t = torch.tensor(bias, dtype=torch.float32, device=dev).reshape(1, 3, 1, 1)
    verdicts = []
    for hname, _, Ms in arms.footprints():
        minv = warp.device_inverse(Ms, dev).clone()  # (caller-owned)
        k = [0]

        def nv12(i):
            return warp.warp_perspective_nv12(planes[i][0], planes[i][1], None, (D, D), flags=warp.INTER_LINEAR, out=bev[i], M_inv_device=minv)

        def launch(arm):
            i = k[0] % nset
            if arm == "nv12":
                nv12(i)
            elif arm == "two_kernel":
                warp.warp_to_planar(nv12(i), None, (D, D), scale=scale, bias=bias, flags=warp.INTER_NEAREST, out=outs[torch.float16][i], M_inv_device=eye,
                                    out_dtype=torch.float16)
            elif arm == "two_torch":
                nv12(i).permute(0, 3, 1, 2).float().mul(sc_t).add(bi_t).half()
            else:
                warp.warp_nv12_to_planar(planes[i][0], planes[i][1], None, (D, D), scale=scale, bias=bias, flags=warp.INTER_LINEAR, out=outs[arm][i],
                                         M_inv_device=minv, out_dtype=arm)
            k[0] += 1

        q = arms.p10_50_90(arms.timed(ARMS, launch, rounds, per_round, warm))
        med = {arm: q[arm][1] for arm in ARMS}
        for arm, label in ARMS.items():
            lines.append("%-9s %-46s median %9.1f us  p10 %9.1f  p90 %9.1f  ratio to (a) %5.2f" % (hname, label, med[arm], q[arm][0], q[arm][2], med[arm] / med["nv12"]))
        faster = min(med["two_kernel"], med["two_torch"])
        ok = med[torch.float16] < faster and med[torch.bfloat16] < faster
        verdicts.append(ok)
        lines.append("%-9s condition: float16 %.1f and bfloat16 %.1f below the faster two-pass route %.1f -> %s (one launch / faster route: %.2f, %.2f)" % (
            hname, med[torch.float16], med[torch.bfloat16], faster, "holds" if ok else "DOES NOT HOLD", med[torch.float16] / faster, med[torch.bfloat16] / faster))
    lines.append("# the condition %s on both footprints" % ("holds" if all(verdicts) else "does NOT hold"))
    arms.finish(lines, a.out)


if __name__ == "__main__":
    main()
