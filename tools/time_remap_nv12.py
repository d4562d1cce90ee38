#!/usr/bin/env python3
"""A decoder's NV12 frames through a fixed camera's lens map in ONE launch (bevwarp_remap_nv12, bevwarp_remap_nv12_planes) against the
routes they replace, on tools/time_remap.py's shapes and protocol -- 32 x 1080p -> 1024^2, bilinear, one lens-A map shared by the 32
frames, the keystone footprint and the Brno-like BEV.  Arms, interleaved in one process after a warm-up, buffer sets rotated past the
Infinity Cache, HIP-event time per arm (both launches of a two-launch arm inside one pair of events), p10 / p50 / p90:
    remap_nv12           bevwarp_remap_nv12
    remap_nv12@NAME      the same through another build of the library (--variant-lib, repeatable: variants/remap_nv12_taps.so loads every
                         tap on its own, no window loads)
    two_launch           an identity bevwarp_warp_nv12 (nearest) to a full-size BGR frame, then bevwarp_remap of that frame
    remap_bgr            bevwarp_remap on resident BGR frames (no conversion anywhere: the floor of the second launch)
    warp_nv12            bevwarp_warp_nv12 (pinhole, no lens: the float64 chain per pixel instead of the map)
    planes_f16           bevwarp_remap_nv12_planes to float16 planes
    two_launch_planes    bevwarp_remap_nv12, then bevwarp_warp_planes (identity, nearest) of its pixels to float16 planes
Derived: remap_nv12 p90 against two_launch p10 and planes_f16 p50 against two_launch_planes p50 (the expectations DESIGN.md section
4.19 judges), and each variant against remap_nv12.
GPU box:  python tools/time_remap_nv12.py [--quick] [--out FILE] [--variant-lib PATH]..."""
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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--quick", action="store_true", help="a few launches per arm (for a profiler run)")
    p.add_argument("--out", default=None, help="also write the table to this file")
    p.add_argument("--variant-lib", action="append", default=[], help="another build of libbevwarp.so: its bevwarp_remap_nv12 is timed as one more arm")
    a = p.parse_args()
    B, SH, SW, D = 32, 1080, 1920, 1024
    rounds, per_round, warm = (2, 3, 2) if a.quick else (7, 10, 5)
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    variants = {}
    for path in a.variant_lib:
        v = ctypes.CDLL(path)
        v.bevwarp_remap_nv12.restype, v.bevwarp_remap_nv12.argtypes = _lib.SYMBOLS["bevwarp_remap_nv12"]
        variants["remap_nv12@" + os.path.splitext(os.path.basename(path))[0]] = v
    arms = ["remap_nv12"] + list(variants) + ["two_launch", "remap_bgr", "warp_nv12", "planes_f16", "two_launch_planes"]
    K = np.array([[0.8 * SW, 0, (SW - 1) / 2], [0, 0.816 * SW, (SH - 1) / 2 + 3], [0, 0, 1.0]])
    border = np.zeros(3)
    bv = border.ctypes.data_as(ctypes.c_void_p)
    scale = np.full(3, 1.0 / 255.0)
    sc = scale.ctypes.data_as(ctypes.c_void_p)
    nset = 3  # (3 x 100 MB of NV12 frames, 3 x 199 MB of converted frames, 3 x 101 MB of pixels, 3 x 201 MB of planes: past the 256 MB Infinity Cache)
    rng = np.random.default_rng(0)
    nv12 = [torch.from_numpy(rng.integers(0, 256, (B, SH * 3 // 2, SW), dtype=np.uint8)).to(dev) for _ in range(nset)]
    planes = [warp.split_nv12(f) for f in nv12]
    bgr = [torch.zeros((B, SH, SW, 3), dtype=torch.uint8, device=dev) for _ in range(nset)]
    outs = [torch.zeros((B, D, D, 3), dtype=torch.uint8, device=dev) for _ in range(nset)]
    pl16 = [torch.zeros((B, 3, D, D), dtype=torch.float16, device=dev) for _ in range(nset)]
    eye = torch.eye(3, dtype=torch.float64, device=dev).reshape(1, 3, 3).contiguous()
    lines = ["# bevwarp_remap_nv12 / bevwarp_remap_nv12_planes vs the two-launch routes vs bevwarp_remap (resident BGR) vs bevwarp_warp_nv12, %d x %dx%d NV12 -> %dx%dx3, "
             "bilinear; us per arm" % (B, SW, SH, D, D),
             "# lens A %s, one shared map; %d rounds x %d launches per arm, arms interleaved; %s" % (LENS_A, rounds, per_round, torch.cuda.get_device_name(dev))]
    for path in a.variant_lib:
        lines.append("# variant: %s" % path)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for hname, hfn in (("keystone", wl.keystone_H), ("brno", wl.synth_brno_H)):
        H = hfn(SW, SH, D, D)
        minv = torch.from_numpy(warp.invert_homography(H[None])).to(dev)
        m = warp.build_warp_map(H, (D, D), K=K, dist_coeff=LENS_A)
        xy, fr, xy_fs, xy_rs, fr_fs, fr_rs = m._planes()
        maps = (xy, fr, 1, xy_fs, xy_rs, fr_fs, fr_rs)
        torch.cuda.synchronize()
        k = [0]

        def launch(arm):
            i = k[0] % nset
            k[0] += 1
            y, uv = planes[i]
            src = (y.data_ptr(), uv.data_ptr())
            strides = (y.stride(0), y.stride(1), uv.stride(0), uv.stride(1))
            pix = (outs[i].data_ptr(), B, SH, SW, D, D) + strides + (D * D * 3, D * 3)
            if arm == "remap_nv12" or arm in variants:
                fn = (variants[arm] if arm in variants else lib).bevwarp_remap_nv12
                st = fn(*src, *pix, *maps, 1, warp.BORDER_CONSTANT, 0, bv, stream)
            elif arm == "two_launch":
                st = lib.bevwarp_warp_nv12(*src, bgr[i].data_ptr(), B, SH, SW, SH, SW, *strides, SH * SW * 3, SW * 3, eye.data_ptr(), 1, 0, 0, bv, stream)
                _lib.check(st)
                st = lib.bevwarp_remap(bgr[i].data_ptr(), outs[i].data_ptr(), B, SH, SW, D, D, 3, SH * SW * 3, SW * 3, D * D * 3, D * 3, *maps, _lib.U8, 1,
                                       warp.BORDER_CONSTANT, bv, stream)
            elif arm == "remap_bgr":
                st = lib.bevwarp_remap(bgr[i].data_ptr(), outs[i].data_ptr(), B, SH, SW, D, D, 3, SH * SW * 3, SW * 3, D * D * 3, D * 3, *maps, _lib.U8, 1,
                                       warp.BORDER_CONSTANT, bv, stream)
            elif arm == "warp_nv12":
                st = lib.bevwarp_warp_nv12(*src, *pix, minv.data_ptr(), 1, 1, 0, bv, stream)
            elif arm == "planes_f16":
                st = lib.bevwarp_remap_nv12_planes(*src, pl16[i].data_ptr(), B, SH, SW, D, D, *strides, 3 * D * D * 2, D * D * 2, D * 2, *maps, 1, warp.BORDER_CONSTANT, 0,
                                                   bv, sc, None, _lib.F16, stream)
            else:
                st = lib.bevwarp_remap_nv12(*src, *pix, *maps, 1, warp.BORDER_CONSTANT, 0, bv, stream)
                _lib.check(st)
                st = lib.bevwarp_warp_planes(outs[i].data_ptr(), pl16[i].data_ptr(), B, D, D, D, D, 3, D * D * 3, D * 3, 3 * D * D * 2, D * D * 2, D * 2, eye.data_ptr(), 1,
                                             _lib.U8, 0, bv, sc, None, _lib.F16, stream)
            _lib.check(st)

        for arm in arms:
            for _ in range(warm):
                launch(arm)
        torch.cuda.synchronize()
        t = {arm: [] for arm in arms}
        for _ in range(rounds):
            for arm in arms:
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(per_round)]
                for e0, e1 in ev:
                    e0.record()
                    launch(arm)
                    e1.record()
                torch.cuda.synchronize()
                t[arm] += [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
        q = {arm: [float(np.percentile(t[arm], v)) for v in (10, 50, 90)] for arm in arms}
        for arm in arms:
            lines.append("%-9s %-26s p10 %8.1f  p50 %8.1f  p90 %8.1f us  (%d launches)" % (hname, arm, q[arm][0], q[arm][1], q[arm][2], len(t[arm])))
        lines.append("%-9s remap_nv12 p90 %.1f %s two_launch p10 %.1f   remap_nv12 / two_launch %5.2f   remap_nv12 / remap_bgr %5.2f   remap_nv12 / warp_nv12 %5.2f"
                     % (hname, q["remap_nv12"][2], "<=" if q["remap_nv12"][2] <= q["two_launch"][0] else ">", q["two_launch"][0], q["remap_nv12"][1] / q["two_launch"][1],
                        q["remap_nv12"][1] / q["remap_bgr"][1], q["remap_nv12"][1] / q["warp_nv12"][1]))
        lines.append("%-9s planes_f16 p50 %.1f %s two_launch_planes p50 %.1f   planes_f16 / two_launch_planes %5.2f   (p90 %.1f against p10 %.1f)"
                     % (hname, q["planes_f16"][1], "<" if q["planes_f16"][1] < q["two_launch_planes"][1] else ">=", q["two_launch_planes"][1],
                        q["planes_f16"][1] / q["two_launch_planes"][1], q["planes_f16"][2], q["two_launch_planes"][0]))
        for v in variants:
            lines.append("%-9s %s / remap_nv12 %5.2f" % (hname, v, q[v][1] / q["remap_nv12"][1]))
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
