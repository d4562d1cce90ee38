#!/usr/bin/env python3
"""The 16-bit plane kernels (bevwarp_warp_planes: float16, bfloat16) against the float32-plane kernel (bevwarp_warp_planar) they stand
beside, the interleaved uint8 warp (the same taps and blend: the lower bound) and what callers did before -- float32 planes followed by
a `.half()` pass -- on BASELINE configs[1]: 32 x 1080p -> 1024^2, per-frame jitter_H matrices, uint8 RGB bilinear, keystone footprint and
the Brno-like BEV (synth_brno_H).  All arms run interleaved in one process after a warm-up, buffer sets rotated past the 256 MB Infinity
Cache (the conversion pass writes into rotated buffers too, not into one the allocator hands back every time); HIP-event time per
launch.  Per arm: median, p10, p90, the algorithmic bytes (destination bytes + warp.footprint x 3 source bytes; the conversion pass adds
its read and its write), the TB/s they make, and the ratio to the float32-plane arm -- whose kernel is byte-identical to the parent's
(profiles/planes16_isa_identity.txt), so it is the baseline.
GPU box:  python tools/time_planes.py [--quick] [--out FILE]"""
import numpy as np
import torch

import arms
from arms import B, C, D, SH, SW
from bev_amd import warp

ARMS = ["uint8 interleaved", "float32 planes", "float16 planes", "bfloat16 planes", "float32 planes + .half()"]


def main():
    a = arms.parser(__doc__).parse_args()
    rounds, per_round, warm = arms.counts(a.quick)
    nset = 3  # (3 x 199 MB of sources; destinations: 3 x 101 MB interleaved, 3 x 403 MB float32 planes, 3 x 201 MB 16-bit planes)
    dev = torch.device("cuda", 0)
    scale, bias = 1.0 / (255.0 * np.array([0.229, 0.224, 0.225])), -np.array([0.485, 0.456, 0.406]) / np.array([0.229, 0.224, 0.225])
    lines = ["# plane formats of the one-pass warp, %d x %dx%dx3 uint8 -> %dx%d, bilinear, per-frame jitter_H, ImageNet scale and bias; us per launch" % (B, SW, SH, D, D),
             "# %d rounds x %d launches per arm, arms interleaved, %d buffer sets; %s" % (rounds, per_round, nset, torch.cuda.get_device_name(dev)),
             "# bytes: destination + footprint x 3 (the conversion pass: + its 4-byte read and 2-byte write); ratio: median / median of float32 planes"]
    srcs, out_u8 = arms.frame_sets(nset, dev), arms.dest_sets(nset, dev)
    out_f32 = arms.dest_sets(nset, dev, (B, C, D, D), torch.float32)
    out_16 = arms.dest_sets(nset, dev, (B, C, D, D), torch.int16)
    out_f16, out_bf16 = [t.view(torch.float16) for t in out_16], [t.view(torch.bfloat16) for t in out_16]
    planes = B * C * D * D
    verdict = []
    for hname, _, Ms in arms.footprints():
        minv = warp.device_inverse(Ms, dev).clone()  # (caller-owned: the plain launch)
        src_bytes = int(warp.footprint((SH, SW), Ms, (D, D), batch=B, device=dev)[0].sum().item()) * C
        nbytes = {ARMS[0]: planes + src_bytes, ARMS[1]: 4 * planes + src_bytes, ARMS[2]: 2 * planes + src_bytes, ARMS[3]: 2 * planes + src_bytes,
                  ARMS[4]: 4 * planes + src_bytes + 4 * planes + 2 * planes}
        k = [0]

        def launch(arm):
            i = k[0] % nset
            k[0] += 1
            if arm == ARMS[0]:
                warp.warp_perspective(srcs[i], None, (D, D), flags=warp.INTER_LINEAR, out=out_u8[i], M_inv_device=minv)
            elif arm == ARMS[1] or arm == ARMS[4]:
                warp.warp_to_planar(srcs[i], None, (D, D), scale=scale, bias=bias, out=out_f32[i], M_inv_device=minv)
                if arm == ARMS[4]:
                    out_f16[i].copy_(out_f32[i])  # (the `.half()` pass, into a rotated buffer)
            else:
                dt, outs = (torch.float16, out_f16) if arm == ARMS[2] else (torch.bfloat16, out_bf16)
                warp.warp_to_planar(srcs[i], None, (D, D), scale=scale, bias=bias, out=outs[i], M_inv_device=minv, out_dtype=dt)

        q = arms.p10_50_90(arms.timed(ARMS, launch, rounds, per_round, warm))
        med = {arm: q[arm][1] for arm in ARMS}
        for arm in ARMS:
            lines.append("%-9s %-25s median %7.1f us  p10 %7.1f  p90 %7.1f  bytes %6.1f MB  %5.2f TB/s  ratio to float32 planes %5.2f" % (
                hname, arm, med[arm], q[arm][0], q[arm][2], nbytes[arm] / 1e6, nbytes[arm] / med[arm] / 1e6, med[arm] / med[ARMS[1]]))
        for arm in ARMS[2:4]:
            if hname == "keystone":
                verdict.append("# %s, keystone: p90 %.1f us %s p10 of float32 planes %.1f us" % (
                    arm, q[arm][2], "<" if q[arm][2] < q[ARMS[1]][0] else "NOT BELOW", q[ARMS[1]][0]))
            verdict.append("# %s, %s: median %.1f us %s median of float32 planes + .half() %.1f us" % (
                arm, hname, med[arm], "<" if med[arm] < med[ARMS[4]] else "NOT BELOW", med[ARMS[4]]))
    arms.finish(lines + verdict, a.out)


if __name__ == "__main__":
    main()
