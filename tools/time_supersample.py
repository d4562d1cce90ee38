#!/usr/bin/env python3
"""The supersampled warp (bevwarp_warp_border | BEVWARP_SUPERSAMPLE_*) against the route it replaces, on BASELINE configs[1] -- 32 x 1080p
-> 1024^2, per-frame jitter_H matrices, the keystone footprint and the Brno-like BEV, uint8 RGB, bilinear.  Arms per k in {2, 4}:
  fused kK          warp_perspective_supersampled(supersample=K, BORDER_REPLICATE): one launch
  route kK          warp_perspective into (K 1024)^2 with the fine matrices and BORDER_REPLICATE, then the integer box reduce in torch (view, sum,
                    add, shift): the same pixels by bits, through a fine frame set written once and read once
  route kK const    the same with BORDER_CONSTANT: the first pass is the product kernel (bevwarp_warp), the fastest the library has
and `plain`, bevwarp_warp_border REPLICATE at 1024^2, as the unit.  All arms alternate in one process after a warm-up, source sets rotated
past the Infinity Cache; HIP-event time from the first launch of an arm to its last.
GPU box:  python tools/time_supersample.py [--quick] [--out FILE]"""
import numpy as np
import torch

import arms
from arms import B, C, D
from bev_amd import warp

KS = (2, 4)


def fine_matrices(Minv, k):
    """The fine matrix of include/bevwarp.h for each of the (n, 3, 3) inverse matrices (numpy float64: one rounding per operation)."""
    c = (1.0 - k) / (2.0 * k)
    F = Minv.copy()
    F[:, :, 0], F[:, :, 1] = Minv[:, :, 0] / k, Minv[:, :, 1] / k
    F[:, :, 2] = (Minv[:, :, 0] * c + Minv[:, :, 1] * c) + Minv[:, :, 2]
    return F


def main():
    a = arms.parser(__doc__).parse_args()
    rounds, per_round, warm = arms.counts(a.quick)
    dev = torch.device("cuda", 0)
    lines = ["# supersampled warp vs the two-pass route, %d x 1920x1080x3 -> %dx%dx3 uint8, bilinear, per-frame jitter_H; us per call" % (B, D, D),
             "# %d rounds x %d calls per arm, arms alternating; %s" % (rounds, per_round, torch.cuda.get_device_name(dev))]
    nset = 3  # (3 x 199 MB of sources: past the 256 MB Infinity Cache)
    srcs = arms.frame_sets(nset, dev)
    outs = arms.dest_sets(nset, dev)
    fine = {k: torch.empty((B, k * D, k * D, C), dtype=torch.uint8, device=dev) for k in KS}  # (k = 4: 1.6 GB)
    names = ["plain"] + [n % k for k in KS for n in ("fused k%d", "route k%d", "route k%d const")]
    for hname, _, Ms in arms.footprints():
        minv = warp.device_inverse(Ms, dev).clone()  # (caller-owned)
        fminv = {k: torch.from_numpy(fine_matrices(minv.cpu().numpy(), k)).to(dev) for k in KS}
        n = [0]

        def launch(name):
            i = n[0] % nset
            n[0] += 1
            if name == "plain":
                warp.warp_perspective(srcs[i], None, (D, D), out=outs[i], M_inv_device=minv, border_mode=warp.BORDER_REPLICATE)
                return
            k = int(name.split()[1][1:])
            if name.startswith("fused"):
                warp.warp_perspective_supersampled(srcs[i], None, (D, D), supersample=k, out=outs[i], M_inv_device=minv, border_mode=warp.BORDER_REPLICATE)
                return
            mode = warp.BORDER_CONSTANT if name.endswith("const") else warp.BORDER_REPLICATE
            warp.warp_perspective(srcs[i], None, (k * D, k * D), out=fine[k], M_inv_device=fminv[k], border_mode=mode)
            s = fine[k].view(B, D, k, D, k, C).sum(dim=(2, 4), dtype=torch.int32)
            outs[i].copy_((s + (k * k) // 2) >> (2 * (k.bit_length() - 1)))

        for k in KS:  # the arms compute one image (the route with REPLICATE: by bits)
            launch("fused k%d" % k)
            ref = outs[(n[0] - 1) % nset].clone()
            n[0] -= 1
            launch("route k%d" % k)
            assert torch.equal(ref, outs[(n[0] - 1) % nset]), "fused and route differ, k = %d" % k
        q = arms.p10_50_90(arms.timed(names, launch, rounds, per_round, warm, order="alternate"))
        for name in names:
            lines.append("%-9s %-15s p10 %10.1f  p50 %10.1f  p90 %10.1f  ratio to plain %6.2f" % (hname, name, q[name][0], q[name][1], q[name][2], q[name][1] / q["plain"][1]))
        for k in KS:
            f, r, rc = q["fused k%d" % k], q["route k%d" % k], q["route k%d const" % k]
            lines.append("%-9s k=%d: fused p90 %.1f vs route p10 %.1f (const: %.1f) -> fused p90 <= route p10: %s (const: %s); fused / plain %.2f (k^2 = %d)"
                         % (hname, k, f[2], r[0], rc[0], f[2] <= r[0], f[2] <= rc[0], f[1] / q["plain"][1], k * k))
    arms.finish(lines, a.out)


if __name__ == "__main__":
    main()
