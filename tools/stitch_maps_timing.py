#!/usr/bin/env python3
"""The multi-camera stitch through warp maps (bevwarp_stitch_maps, bevwarp_stitch_maps_nv12) against the routes that exist:
3 cameras x 32 x 1080p -> 32 x 1024^2, uint8 x 3, bilinear, on tools/stitch_timing.py's three Brno-like views.  Arms, interleaved in one
process after a warm-up, buffer sets rotated past the Infinity Cache:
  (a) bevwarp_warp_stitch over -- the float64 chain per covered pixel, camera and frame
  (b) canvas.fill_(0) + three bevwarp_remap(..., BORDER_TRANSPARENT) calls through shared pinhole maps -- the map route that exists
  (c) bevwarp_stitch_maps over, the same maps -- checked equal to (a) and to (b) before it is timed
  (d) (c) with lens-A maps (tests/lens_ref.LENS_A, lens_valid_r2)
  (e) (c) with BEVWARP_STITCH_FEATHER, F = 64
  (f) canvas.fill_(0) + three bevwarp_remap_nv12(..., BORDER_TRANSPARENT) calls
  (g) bevwarp_stitch_maps_nv12 over -- checked equal to (f)
(a), (b) and (f) are entries this change does not touch: the baseline of the same run.  HIP-event time per arm (the whole of (b) and (f):
the fill and the three launches), p10 / p50 / p90, and the three expectations, each confirmed or refuted.
GPU box:  python tools/stitch_maps_timing.py [--quick] [--out FILE]"""
import ctypes

import numpy as np
import torch

import arms
from arms import B, C, D, SH, SW
from bev_amd import _lib, warp
from tests import nv12_ref
from tests import workloads as wl

ARMS = ("(a) warp_stitch over", "(b) fill + 3 x remap transparent", "(c) stitch_maps over", "(d) stitch_maps over, lens maps", "(e) stitch_maps feather 64",
        "(f) fill + 3 x remap_nv12 transparent", "(g) stitch_maps_nv12 over")


def main():
    a = arms.parser(__doc__).parse_args()
    K = 3
    rounds, per_round, warm = arms.counts(a.quick)
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    Ms = arms.views()
    minvs = [torch.from_numpy(warp.invert_homography(M)[None]).to(dev) for M in Ms]
    pin = [warp.build_warp_map(M, (D, D), device=dev) for M in Ms]
    lens = [arms.lens_map(M, dev) for M in Ms]
    torch.cuda.synchronize()
    covers = []
    for maps in (pin, lens):
        inl = [((m.xy[0, :, :, 0] >= 0) & (m.xy[0, :, :, 0] < SW - 1) & (m.xy[0, :, :, 1] >= 0) & (m.xy[0, :, :, 1] < SH - 1)) for m in maps]
        count = sum(i.to(torch.int64) for i in inl)
        covers.append(" / ".join("%.1f" % (100.0 * float((count == c).float().mean())) for c in range(4)))
    nset = 2  # (2 x 597 MB of frames, 2 x 299 MB of NV12 planes, 2 x 101 MB of canvases -- past the 256 MB Infinity Cache)
    srcs, ys, uvs = [], [], []
    for s in range(nset):  # (four distinct frames per camera and set, repeated over the batch)
        four = [[wl.frame(97 * (K * s + k) + i, SH, SW, np.uint8) for i in range(4)] for k in range(K)]
        srcs.append([torch.from_numpy(np.stack([four[k][i % 4] for i in range(B)])).to(dev) for k in range(K)])
        nv = [[nv12_ref.frame("video", 131 * (K * s + k) + i, SH, SW) for i in range(4)] for k in range(K)]
        ys.append([torch.from_numpy(np.stack([nv[k][i % 4][0] for i in range(B)])).to(dev) for k in range(K)])
        uvs.append([torch.from_numpy(np.stack([nv[k][i % 4][1] for i in range(B)])).to(dev) for k in range(K)])
    outs = arms.dest_sets(nset, dev)

    def map_cams(s, maps, nv12):
        arr = (_lib.MapCamera * K)()
        for k in range(K):
            xy_p, fr_p, xy_fs, xy_rs, fr_fs, fr_rs = maps[k]._planes()
            if nv12:
                arr[k] = _lib.MapCamera(ys[s][k].data_ptr(), uvs[s][k].data_ptr(), SH * SW, SW, SH * SW // 2, SW, xy_p, fr_p, xy_fs, xy_rs, fr_fs, fr_rs, SH, SW, 1, 0)
            else:
                arr[k] = _lib.MapCamera(srcs[s][k].data_ptr(), None, SH * SW * C, SW * C, 0, 0, xy_p, fr_p, xy_fs, xy_rs, fr_fs, fr_rs, SH, SW, 1, 0)
        return arr

    cams = []
    for s in range(nset):
        arr = (_lib.Camera * K)()
        for k in range(K):
            arr[k] = _lib.Camera(srcs[s][k].data_ptr(), minvs[k].data_ptr(), SH * SW * C, SW * C, SH, SW, 1, 0)
        cams.append(arr)
    pin_cams, lens_cams, nv_cams = ([map_cams(s, m, n) for s in range(nset)] for m, n in ((pin, False), (lens, False), (pin, True)))
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    n = [0]

    def launch(arm, i=None):
        if i is None:
            i = n[0] % nset
            n[0] += 1
        o = outs[i].data_ptr()
        k = ARMS.index(arm)
        if k == 0:
            _lib.check(lib.bevwarp_warp_stitch(ctypes.addressof(cams[i]), K, o, B, D, D, C, D * D * C, D * C, _lib.U8, 1, _lib.STITCH_OVER, 64, warp.BORDER_CONSTANT, None, stream))
        elif k == 1:
            outs[i].fill_(0)
            for c in range(K):
                xy_p, fr_p, xy_fs, xy_rs, fr_fs, fr_rs = pin[c]._planes()
                _lib.check(lib.bevwarp_remap(srcs[i][c].data_ptr(), o, B, SH, SW, D, D, C, SH * SW * C, SW * C, D * D * C, D * C, xy_p, fr_p, 1, xy_fs, xy_rs, fr_fs, fr_rs,
                                             _lib.U8, 1, warp.BORDER_TRANSPARENT, None, stream))
        elif k in (2, 3, 4):
            arr = (lens_cams if k == 3 else pin_cams)[i]
            _lib.check(lib.bevwarp_stitch_maps(ctypes.addressof(arr), K, o, B, D, D, C, D * D * C, D * C, _lib.U8, 1, _lib.STITCH_FEATHER if k == 4 else _lib.STITCH_OVER, 64,
                                               warp.BORDER_CONSTANT, None, stream))
        elif k == 5:
            outs[i].fill_(0)
            for c in range(K):
                xy_p, fr_p, xy_fs, xy_rs, fr_fs, fr_rs = pin[c]._planes()
                _lib.check(lib.bevwarp_remap_nv12(ys[i][c].data_ptr(), uvs[i][c].data_ptr(), o, B, SH, SW, D, D, SH * SW, SW, SH * SW // 2, SW, D * D * C, D * C, xy_p, fr_p, 1,
                                                  xy_fs, xy_rs, fr_fs, fr_rs, 1, warp.BORDER_TRANSPARENT, 0, None, stream))
        else:
            _lib.check(lib.bevwarp_stitch_maps_nv12(ctypes.addressof(nv_cams[i]), K, o, B, D, D, D * D * C, D * C, 1, _lib.STITCH_OVER, 64, 0, warp.BORDER_CONSTANT, None, stream))

    # results must not change: (c) leaves what (a) and (b) leave, (g) what (f) leaves, at the timed size
    kept = {}
    for arm in (ARMS[0], ARMS[1], ARMS[2], ARMS[5], ARMS[6]):
        launch(arm, 0)
        torch.cuda.synchronize()
        kept[arm] = outs[0].clone()
    if not (torch.equal(kept[ARMS[2]], kept[ARMS[0]]) and torch.equal(kept[ARMS[2]], kept[ARMS[1]]) and torch.equal(kept[ARMS[6]], kept[ARMS[5]])):
        raise SystemExit("the stitch through maps and the routes it replaces disagree")
    del kept

    lines = ["# bevwarp_stitch_maps / bevwarp_stitch_maps_nv12 vs bevwarp_warp_stitch and vs canvas fill + one bevwarp_remap / bevwarp_remap_nv12 (TRANSPARENT) per camera:",
             "# %d cameras x %d x %dx%dx%d (NV12: %dx%d planes) -> %d x %dx%dx%d, uint8, bilinear, one shared map per camera; us per canvas batch" % (K, B, SW, SH, C, SW, SH, B, D, D, C),
             "# views: tools/stitch_timing.py's; %d rounds x %d runs per arm, arms interleaved; %s" % (rounds, per_round, torch.cuda.get_device_name(dev)),
             "# canvas pixels covered by 0 / 1 / 2 / 3 cameras: pinhole maps %s %%; lens-A maps %s %%" % tuple(covers),
             "# checked before timing: (c) leaves bit for bit the canvas of (a) and of (b), (g) that of (f); (a), (b) and (f) are entries this change does not touch"]
    t = arms.timed(ARMS, launch, rounds, per_round, warm)
    q = arms.p10_50_90(t)
    for arm in ARMS:
        lines.append("%-40s p10 %8.1f  p50 %8.1f  p90 %8.1f us  (%d runs)" % ((arm,) + tuple(q[arm]) + (len(t[arm]),)))
    A, Bm, Cm, Dm, E, F, G = (q[arm] for arm in ARMS)
    verdict = lambda ok: "confirmed" if ok else "refuted"  # noqa: E731
    lines += ["(c) p90 not above (b) p10 (%.1f vs %.1f us): %s   (c) / (b) p50 %.2f" % (Cm[2], Bm[0], verdict(Cm[2] <= Bm[0]), Cm[1] / Bm[1]),
              "(c) p50 below (a) p50 (%.1f vs %.1f us): %s   (c) / (a) p50 %.2f" % (Cm[1], A[1], verdict(Cm[1] < A[1]), Cm[1] / A[1]),
              "(g) p90 not above (f) p10 (%.1f vs %.1f us): %s   (g) / (f) p50 %.2f" % (G[2], F[0], verdict(G[2] <= F[0]), G[1] / F[1]),
              "lens maps / pinhole maps (d) / (c) p50 %.2f   feather / over (e) / (c) p50 %.2f   NV12 / frames (g) / (c) p50 %.2f" % (Dm[1] / Cm[1], E[1] / Cm[1], G[1] / Cm[1])]
    arms.finish(lines, a.out)


if __name__ == "__main__":
    main()
