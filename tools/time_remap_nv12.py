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
import ctypes
import os

import numpy as np
import torch

import arms
from arms import B, D, LENS_A, SH, SW, ptr
from bev_amd import _lib, warp


def main():
    p = arms.parser(__doc__)
    p.add_argument("--variant-lib", action="append", default=[], help="another build of libbevwarp.so: its bevwarp_remap_nv12 is timed as one more arm")
    a = p.parse_args()
    rounds, per_round, warm = arms.counts(a.quick)
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    variants = {}
    for path in a.variant_lib:
        v = ctypes.CDLL(path)
        v.bevwarp_remap_nv12.restype, v.bevwarp_remap_nv12.argtypes = _lib.SYMBOLS["bevwarp_remap_nv12"]
        variants["remap_nv12@" + os.path.splitext(os.path.basename(path))[0]] = v
    names = ["remap_nv12"] + list(variants) + ["two_launch", "remap_bgr", "warp_nv12", "planes_f16", "two_launch_planes"]
    border, scale = np.zeros(3), np.full(3, 1.0 / 255.0)
    bv, sc = ptr(border), ptr(scale)
    nset = 3  # (3 x 100 MB of NV12 frames, 3 x 199 MB of converted frames, 3 x 101 MB of pixels, 3 x 201 MB of planes: past the 256 MB Infinity Cache)
    rng = np.random.default_rng(0)
    nv12 = [torch.from_numpy(rng.integers(0, 256, (B, SH * 3 // 2, SW), dtype=np.uint8)).to(dev) for _ in range(nset)]
    planes = [warp.split_nv12(f) for f in nv12]
    bgr = arms.dest_sets(nset, dev, (B, SH, SW, 3))
    outs = arms.dest_sets(nset, dev)
    pl16 = arms.dest_sets(nset, dev, (B, 3, D, D), torch.float16)
    eye = torch.eye(3, dtype=torch.float64, device=dev).reshape(1, 3, 3).contiguous()
    lines = ["# bevwarp_remap_nv12 / bevwarp_remap_nv12_planes vs the two-launch routes vs bevwarp_remap (resident BGR) vs bevwarp_warp_nv12, %d x %dx%d NV12 -> %dx%dx3, "
             "bilinear; us per arm" % (B, SW, SH, D, D),
             "# lens A %s, one shared map; %d rounds x %d launches per arm, arms interleaved; %s" % (LENS_A, rounds, per_round, torch.cuda.get_device_name(dev))]
    for path in a.variant_lib:
        lines.append("# variant: %s" % path)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for hname, H, _ in arms.footprints():
        minv = torch.from_numpy(warp.invert_homography(H[None])).to(dev)
        m = arms.lens_map(H, dev)
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

        t = arms.timed(names, launch, rounds, per_round, warm)
        q = arms.p10_50_90(t)
        for arm in names:
            lines.append("%-9s %-26s p10 %8.1f  p50 %8.1f  p90 %8.1f us  (%d launches)" % (hname, arm, q[arm][0], q[arm][1], q[arm][2], len(t[arm])))
        lines.append("%-9s remap_nv12 p90 %.1f %s two_launch p10 %.1f   remap_nv12 / two_launch %5.2f   remap_nv12 / remap_bgr %5.2f   remap_nv12 / warp_nv12 %5.2f"
                     % (hname, q["remap_nv12"][2], "<=" if q["remap_nv12"][2] <= q["two_launch"][0] else ">", q["two_launch"][0], q["remap_nv12"][1] / q["two_launch"][1],
                        q["remap_nv12"][1] / q["remap_bgr"][1], q["remap_nv12"][1] / q["warp_nv12"][1]))
        lines.append("%-9s planes_f16 p50 %.1f %s two_launch_planes p50 %.1f   planes_f16 / two_launch_planes %5.2f   (p90 %.1f against p10 %.1f)"
                     % (hname, q["planes_f16"][1], "<" if q["planes_f16"][1] < q["two_launch_planes"][1] else ">=", q["two_launch_planes"][1],
                        q["planes_f16"][1] / q["two_launch_planes"][1], q["planes_f16"][2], q["two_launch_planes"][0]))
        for v in variants:
            lines.append("%-9s %s / remap_nv12 %5.2f" % (hname, v, q[v][1] / q["remap_nv12"][1]))
    arms.finish(lines, a.out)


if __name__ == "__main__":
    main()
