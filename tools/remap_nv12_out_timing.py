#!/usr/bin/env python3
"""The map samplers that write NV12 (bevwarp_remap_to_nv12, bevwarp_remap_nv12_to_nv12, bevwarp_stitch_maps_nv12_to_nv12) against the
routes that exist: 32 x 1080p -> 32 x 1024^2, bilinear, one shared lens-A map (tests/lens_ref.LENS_A, lens_valid_r2), on the keystone and
the Brno-like footprint.  `--step kernels`: arms interleaved in one process after a warm-up, buffer sets rotated past the Infinity
Cache, HIP-event time per arm, p10 / p50 / p90.  Per footprint:
  (a) bevwarp_remap_nv12_to_nv12      against  bevwarp_remap_nv12 into a BGR BEV + an identity bevwarp_warp_to_nv12 at the BEV size (nearest:
                                               the library's only BGR -> NV12 converter), and as a ratio to bevwarp_remap_nv12 alone and
                                               to the pinhole bevwarp_warp_nv12_to_nv12 of the same matrix
  (b) bevwarp_remap_to_nv12           against  bevwarp_remap + the identity conversion
and once, on tools/stitch_timing.py's three views, "over":
  (c) bevwarp_stitch_maps_nv12_to_nv12  against  bevwarp_stitch_maps_nv12 + the identity conversion
Every baseline is an existing entry measured in the same run.  Each new arm is checked equal, bit for bit, to the route it replaces
before anything is timed.  `--step pipeline`: (d) FramePipeline(warp_map=...) over 200 frames of 1080p with NV12 slots on both sides
against BGR slots on both sides, alternated: ms per frame.
GPU box, each step under a time limit of its own and none tried again when it fails:
    timeout -k 10 400 python tools/remap_nv12_out_timing.py --step kernels --out profiles/remap_nv12_out_timing.txt && \\
    timeout -k 10 300 python tools/remap_nv12_out_timing.py --step pipeline --out profiles/remap_nv12_out_timing.txt --append"""
import ctypes

import numpy as np
import torch

import arms
from arms import B, D, SH, SW, lens_map, pipeline_ms, views
from bev_amd import _lib, warp
from bev_amd.pipeline import FramePipeline
from tests import nv12_ref
from tests import workloads as wl

K = 3
NSET = 2  # (2 x 199 MB of BGR frames, 2 x 100 MB of NV12 planes per camera, 2 x 100 MB of BGR BEVs: past the 256 MB Infinity Cache)
SINGLE = (("a_two", "(a) remap_nv12 + identity warp_to_nv12"), ("a_new", "(a) remap_nv12_to_nv12"), ("a_pix", "    remap_nv12 alone"), ("a_pin", "    pinhole warp_nv12_to_nv12"),
          ("b_two", "(b) remap + identity warp_to_nv12"), ("b_new", "(b) remap_to_nv12"))
STITCH = (("c_two", "(c) stitch_maps_nv12 + identity warp_to_nv12"), ("c_new", "(c) stitch_maps_nv12_to_nv12"))
EXPECT = ("# expectations, stated before the numbers: (a) p90 of bevwarp_remap_nv12_to_nv12 is not above p10 of bevwarp_remap_nv12 + the identity conversion, on either footprint;",
          "#   (b) p90 of bevwarp_remap_to_nv12 is not above p10 of bevwarp_remap + the identity conversion, on either footprint;",
          "#   (c) p90 of bevwarp_stitch_maps_nv12_to_nv12 is not above p10 of bevwarp_stitch_maps_nv12 + the identity conversion")


def kernels(quick, dev):
    rounds, per_round, warm = arms.counts(quick)
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    foot = {name: H for name, H, _ in arms.footprints()}
    maps = {k: lens_map(M, dev) for k, M in foot.items()}
    minv = {k: torch.from_numpy(warp.invert_homography(M)[None]).to(dev) for k, M in foot.items()}
    cam_maps = [lens_map(M, dev) for M in views()]
    eye = torch.eye(3, dtype=torch.float64, device=dev)[None].contiguous()
    bgr4 = [wl.frame(97 + i, SH, SW, np.uint8) for i in range(4)]
    nv4 = [nv12_ref.frame("video", 131 + i, SH, SW) for i in range(4)]
    # (four distinct frames, repeated over the batch with a rotation of its own per set and camera: the timing does not depend on the values)
    pick = lambda four, r: torch.from_numpy(np.stack([four[(i + r) % 4] for i in range(B)])).to(dev)  # noqa: E731
    srcs = [pick(bgr4, s) for s in range(NSET)]
    ys = [[pick([f[0] for f in nv4], s + k) for k in range(K)] for s in range(NSET)]
    uvs = [[pick([f[1] for f in nv4], s + k) for k in range(K)] for s in range(NSET)]
    bev = arms.dest_sets(NSET, dev)
    out = arms.dest_sets(NSET, dev, (B, D * 3 // 2, D))
    cams = []
    for s in range(NSET):
        arr = (_lib.MapCamera * K)()
        for k in range(K):
            xy_p, fr_p, xy_fs, xy_rs, fr_fs, fr_rs = cam_maps[k]._planes()
            arr[k] = _lib.MapCamera(ys[s][k].data_ptr(), uvs[s][k].data_ptr(), SH * SW, SW, SH * SW // 2, SW, xy_p, fr_p, xy_fs, xy_rs, fr_fs, fr_rs, SH, SW, 1, 0)
        cams.append(arr)
    n = [0]
    CONSTANT = warp.BORDER_CONSTANT

    def launch(key, fp, i=None):
        if i is None:
            i = n[0] % NSET
            n[0] += 1
        oy, ouv, dst = out[i].data_ptr(), out[i].data_ptr() + D * D, (D * D * 3 // 2, D, D * D * 3 // 2, D)  # (the joined layout, frames D * 3 / 2 rows apart)
        y, uv, b = ys[i][0].data_ptr(), uvs[i][0].data_ptr(), bev[i].data_ptr()
        nv_src, bgr_src, bev_strides = (SH * SW, SW, SH * SW // 2, SW), (SH * SW * 3, SW * 3), (D * D * 3, D * 3)
        m = () if fp is None else maps[fp]._planes()[:2] + (1,) + maps[fp]._planes()[2:]
        identity = lambda: _lib.check(lib.bevwarp_warp_to_nv12(b, oy, ouv, B, D, D, D, D, *bev_strides, *dst, eye.data_ptr(), 1, 0, 0, None, stream))  # noqa: E731
        if key in ("a_two", "a_pix"):
            _lib.check(lib.bevwarp_remap_nv12(y, uv, b, B, SH, SW, D, D, *nv_src, *bev_strides, *m, 1, CONSTANT, 0, None, stream))
            if key == "a_two":
                identity()
        elif key == "a_new":
            _lib.check(lib.bevwarp_remap_nv12_to_nv12(y, uv, oy, ouv, B, SH, SW, D, D, *nv_src, *dst, *m, 1, CONSTANT, None, stream))
        elif key == "a_pin":
            _lib.check(lib.bevwarp_warp_nv12_to_nv12(y, uv, oy, ouv, B, SH, SW, D, D, *nv_src, *dst, minv[fp].data_ptr(), 1, 1, None, stream))
        elif key == "b_two":
            _lib.check(lib.bevwarp_remap(srcs[i].data_ptr(), b, B, SH, SW, D, D, 3, *bgr_src, *bev_strides, *m, _lib.U8, 1, CONSTANT, None, stream))
            identity()
        elif key == "b_new":
            _lib.check(lib.bevwarp_remap_to_nv12(srcs[i].data_ptr(), oy, ouv, B, SH, SW, D, D, *bgr_src, *dst, *m, 1, CONSTANT, 0, None, stream))
        elif key == "c_two":
            _lib.check(lib.bevwarp_stitch_maps_nv12(ctypes.addressof(cams[i]), K, b, B, D, D, *bev_strides, 1, _lib.STITCH_OVER, 64, 0, CONSTANT, None, stream))
            identity()
        else:
            _lib.check(lib.bevwarp_stitch_maps_nv12_to_nv12(ctypes.addressof(cams[i]), K, oy, ouv, B, D, D, *dst, 1, _lib.STITCH_OVER, 64, None, stream))

    # results must not change: every new arm leaves, bit for bit, the frame of the two-launch route it replaces, at the timed size
    rows = [(key, label, fp) for fp in foot for key, label in SINGLE] + [(key, label, None) for key, label in STITCH]
    for two, new, fps in (("a_two", "a_new", foot), ("b_two", "b_new", foot), ("c_two", "c_new", (None,))):
        for fp in fps:
            launch(two, fp, 0)
            torch.cuda.synchronize()
            kept = out[0].clone()
            out[0].fill_(33)
            launch(new, fp, 0)
            torch.cuda.synchronize()
            if not torch.equal(out[0], kept):
                raise SystemExit("%s and %s disagree on %s" % (two, new, fp))
    lines = ["# bevwarp_remap_nv12_to_nv12 / bevwarp_remap_to_nv12 / bevwarp_stitch_maps_nv12_to_nv12 vs the existing entry into a BGR BEV + an identity bevwarp_warp_to_nv12 (nearest):",
             "# %d x %dx%d (BGR, or NV12 planes) -> %d x %dx%d NV12 (joined layout), bilinear, one shared lens-A map per camera, BORDER_CONSTANT; us per batch" % (B, SW, SH, B, D, D),
             "# (c): %d cameras, tools/stitch_timing.py's views, over; %d rounds x %d runs per arm, arms interleaved; %s" % (K, rounds, per_round, torch.cuda.get_device_name(dev)),
             "# checked before timing: each new arm leaves bit for bit the NV12 frames of the two-launch route beside it; the baselines are entries this change does not touch"]
    lines += list(EXPECT)
    t = arms.timed([(key, fp) for key, _, fp in rows], lambda arm: launch(*arm), rounds, per_round, warm)
    q = arms.p10_50_90(t)
    for key, label, fp in rows:
        lines.append("%-9s %-46s p10 %8.1f  p50 %8.1f  p90 %8.1f us  (%d runs)" % ((fp or "3 views", label) + tuple(q[key, fp]) + (len(t[key, fp]),)))
    verdict = lambda ok: "confirmed" if ok else "refuted"  # noqa: E731
    for name, two, new, fps in (("(a)", "a_two", "a_new", foot), ("(b)", "b_two", "b_new", foot), ("(c)", "c_two", "c_new", (None,))):
        for fp in fps:
            T, N = q[two, fp], q[new, fp]
            lines.append("%s %-8s new p90 not above the two-launch route's p10 (%.1f vs %.1f us): %s   new / route p50 %.2f" % (name, fp or "3 views", N[2], T[0], verdict(N[2] <= T[0]), N[1] / T[1]))
    for fp in foot:
        lines.append("(a) %-8s remap_nv12_to_nv12 / remap_nv12 alone p50 %.2f   / pinhole warp_nv12_to_nv12 p50 %.2f" % (fp, q["a_new", fp][1] / q["a_pix", fp][1], q["a_new", fp][1] / q["a_pin", fp][1]))
    return lines


def pipeline(quick, dev):
    n = 40 if quick else 200
    m = lens_map(wl.synth_brno_H(SW, SH, D, D), dev)
    frame_bgr = wl.frame(3, SH, SW, np.uint8)
    frame_nv12 = nv12_ref.join(*nv12_ref.frame("video", 3, SH, SW))
    lines = ["# (d) FramePipeline(warp_map=lens-A map), %d frames %dx%d -> %dx%d, depth 3, Brno-like BEV: ms per frame (host clock around the loop), 3 repeats, arms alternated" % (n, SW, SH, D, D)]
    ms = {"nv12": [], "bgr": []}
    for _ in range(3):
        for fmt in ("nv12", "bgr"):
            with FramePipeline((SH, SW), 3, None, (D, D), depth=3, src_format=fmt, dst_format=fmt, warp_map=m) as pipe:
                ms[fmt].append(pipeline_ms(pipe, frame_nv12 if fmt == "nv12" else frame_bgr, n))
    for fmt in ("nv12", "bgr"):
        up, down = (frame_nv12 if fmt == "nv12" else frame_bgr).nbytes, D * D * (3 if fmt == "bgr" else 1.5)
        lines.append("pipeline  map, %-4s slots on both sides  upload %5.2f MB/frame  download %5.2f MB/frame   ms per frame  median %7.4f  min %7.4f  max %7.4f" % (
            fmt, up / 1e6, down / 1e6, float(np.median(ms[fmt])), min(ms[fmt]), max(ms[fmt])))
    lines.append("pipeline  NV12 slots - BGR slots  %+.4f ms per frame (median)   NV12 / BGR %5.3f" % (
        float(np.median(ms["nv12"])) - float(np.median(ms["bgr"])), float(np.median(ms["nv12"])) / float(np.median(ms["bgr"]))))
    return lines


def main():
    a = arms.parser(__doc__, steps=("kernels", "pipeline")).parse_args()
    dev = torch.device("cuda", 0)
    arms.finish((kernels if a.step == "kernels" else pipeline)(a.quick, dev), a.out, a.append)


if __name__ == "__main__":
    main()
