#!/usr/bin/env python3
"""The multi-camera warp (bevwarp_warp_stitch) against the route it replaces: 3 cameras x 32 x 1080p -> 32 x 1024^2, uint8 RGB,
bilinear.  The views are three Brno-like ones (tests/workloads.synth_brno_H, turned and shifted on the canvas: a left, a centre and a
right camera with distinct matrices and substantial pairwise overlap; the cover classes are printed).  Arms, interleaved in one process on
the same buffers after a warm-up, buffer sets rotated past the Infinity Cache:
  (a) canvas.fill_(0) + three bevwarp_warp_border(..., BORDER_TRANSPARENT) calls -- the route that exists
  (b) bevwarp_warp_stitch, BEVWARP_STITCH_OVER, BORDER_CONSTANT 0 -- bit for bit (a)'s canvas, which the script checks before it times
  (c) bevwarp_warp_stitch, BEVWARP_STITCH_FEATHER with F = 64
HIP-event time per arm (the whole of (a): the fill and its three launches), p10 / p50 / p90, and the ratios.
GPU box:  python tools/stitch_timing.py [--quick] [--out FILE]"""
import ctypes

import numpy as np
import torch

import arms
from arms import B, C, D, SH, SW
from bev_amd import _lib, warp
from tests import border_ref
from tests import workloads as wl

ARMS = ("fill + 3 x border_transparent", "stitch over", "stitch feather 64")


def main():
    a = arms.parser(__doc__).parse_args()
    K = 3
    rounds, per_round, warm = arms.counts(a.quick)
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    Ms = arms.views()
    masks = [border_ref.written_mask((SH, SW), M, (D, D), 1) for M in Ms]
    count = sum(m.astype(np.int64) for m in masks)
    pair = [(i, j, float((masks[i] & masks[j]).sum()) / min(masks[i].sum(), masks[j].sum())) for i in range(K) for j in range(i + 1, K)]
    minvs = [torch.from_numpy(warp.invert_homography(M)[None]).to(dev) for M in Ms]
    nset = 2  # (2 x 597 MB of sources, 2 x 101 MB of canvases -- past the 256 MB Infinity Cache)
    srcs = []
    for s in range(nset):  # (four distinct frames per camera and set, repeated over the batch)
        four = [[wl.frame(97 * (K * s + k) + i, SH, SW, np.uint8) for i in range(4)] for k in range(K)]
        srcs.append([torch.from_numpy(np.stack([four[k][i % 4] for i in range(B)])).to(dev) for k in range(K)])
    outs = arms.dest_sets(nset, dev)
    cams = []
    for s in range(nset):
        arr = (_lib.Camera * K)()
        for k in range(K):
            arr[k] = _lib.Camera(srcs[s][k].data_ptr(), minvs[k].data_ptr(), SH * SW * C, SW * C, SH, SW, 1, 0)
        cams.append(arr)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    n = [0]

    def launch(arm, i=None):
        if i is None:
            i = n[0] % nset
            n[0] += 1
        tail = (B, D, D, C, D * D * C, D * C)
        if arm == ARMS[0]:
            outs[i].fill_(0)
            for k in range(K):
                _lib.check(lib.bevwarp_warp_border(srcs[i][k].data_ptr(), outs[i].data_ptr(), B, SH, SW, D, D, C, SH * SW * C, SW * C, D * D * C, D * C,
                                                   minvs[k].data_ptr(), 1, _lib.U8, 1, warp.BORDER_TRANSPARENT, None, stream))
        else:
            feather = arm == ARMS[2]
            _lib.check(lib.bevwarp_warp_stitch(ctypes.addressof(cams[i]), K, outs[i].data_ptr(), *tail, _lib.U8, 1, _lib.STITCH_FEATHER if feather else _lib.STITCH_OVER,
                                               64, warp.BORDER_CONSTANT, None, stream))

    # results must not change: (b) leaves what (a) leaves, at the timed size; (c) differs from it exactly where cameras overlap
    launch(ARMS[0], 0)
    route = outs[0].clone()
    launch(ARMS[1], 0)
    torch.cuda.synchronize()
    same = torch.equal(route, outs[0])
    launch(ARMS[2], 0)
    torch.cuda.synchronize()
    differs = (outs[0][0] != route[0]).any(dim=2).cpu().numpy()
    if not same or (differs & (count < 2)).any():
        raise SystemExit("the stitch kernel and the one-call-per-camera route disagree (over equal: %s)" % same)
    del route

    lines = ["# bevwarp_warp_stitch vs canvas fill + one bevwarp_warp_border(TRANSPARENT) per camera: %d cameras x %d x %dx%dx%d -> %d x %dx%dx%d, uint8, bilinear; us per canvas batch"
             % (K, B, SW, SH, C, B, D, D, C),
             "# views: synth_brno_H turned -12 / 0 / +12 degrees and shifted -180 / 0 / +180 px on the canvas, one matrix per camera; %d rounds x %d runs per arm, arms interleaved; %s"
             % (rounds, per_round, torch.cuda.get_device_name(dev)),
             "# canvas pixels covered by 0 / 1 / 2 / 3 cameras: %s %%; pairwise overlap (share of the smaller footprint): %s"
             % (" / ".join("%.1f" % (100.0 * (count == c).mean()) for c in range(4)), ", ".join("%d-%d %.0f %%" % (i, j, 100 * f) for i, j, f in pair)),
             "# arm (a)'s kernel, warp_border_kernel<uint8, 3, bilinear, TRANSPARENT>, is byte for byte the one of the commit before the stitch warp (profiles/stitch_isa_identity.txt)",
             "# checked before timing: 'stitch over' leaves bit for bit the canvas of arm (a); 'stitch feather 64' differs from it only where two or more cameras cover"]
    t = arms.timed(ARMS, launch, rounds, per_round, warm)
    q = arms.p10_50_90(t)
    for arm in ARMS:
        lines.append("%-30s p10 %8.1f  p50 %8.1f  p90 %8.1f us  (%d runs)" % ((arm,) + tuple(q[arm]) + (len(t[arm]),)))
    lines.append("over / route (p50) %.2f   feather / over (p50) %.2f   over's p90 %s the route's p10 (%.1f vs %.1f us): the expectation is %s"
                 % (q[ARMS[1]][1] / q[ARMS[0]][1], q[ARMS[2]][1] / q[ARMS[1]][1], "is not above" if q[ARMS[1]][2] <= q[ARMS[0]][0] else "is above",
                    q[ARMS[1]][2], q[ARMS[0]][0], "confirmed" if q[ARMS[1]][2] <= q[ARMS[0]][0] else "refuted"))
    arms.finish(lines, a.out)


if __name__ == "__main__":
    main()
