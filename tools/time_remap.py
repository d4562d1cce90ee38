#!/usr/bin/env python3
"""The fixed-camera route (bevwarp_build_map once, bevwarp_remap per batch) against the route it replaces (bevwarp_warp_lens: the whole
float64 chain per pixel of every frame) on tools/time_lens.py's shapes and protocol -- 32 x 1080p -> 1024^2, uint8 x 3, bilinear, the
keystone footprint and the Brno-like BEV, the tests' lens A at 1080p, r2_max = lens_valid_r2.  Arms, interleaved in one process after a
warm-up, buffer sets rotated past the Infinity Cache, HIP-event time per launch, p10 / p50 / p90:
    lens                 bevwarp_warp_lens, per-frame jitter_H matrices (the yardstick)
    remap_shared         bevwarp_remap, ONE lens map (matrix 0) shared by the 32 frames: the fixed camera
    remap_per_frame      bevwarp_remap, 32 lens maps (one per matrix): map traffic the frame loop cannot hide
    border_transparent   bevwarp_warp_border, TRANSPARENT: the same frame without lens maths and without maps
    warp                 bevwarp_warp (what bench.py times)
    build_map            one bevwarp_build_map call (one 1024^2 lens map)
    remap_shared@NAME    the shared-map arm through another build of the library (--variant-lib, repeatable: e.g. NAME.so made with
                         -DBEVWARP_REMAP_MAX_FPI=1, one frame per item, the map re-read per frame through the caches)
Derived: remap_shared p90 against lens p10 (the expectation DESIGN.md section 4.18 judges), the break-even number of batches
build / (lens - remap_shared), and remap_per_frame / remap_shared.
GPU box:  python tools/time_remap.py [--quick] [--out FILE] [--variant-lib PATH]..."""
import ctypes
import os

import numpy as np
import torch

import arms
from arms import B, C, D, LENS_A, SH, SW, ptr
from bev_amd import _lib, warp


def main():
    p = arms.parser(__doc__)
    p.add_argument("--variant-lib", action="append", default=[], help="another build of libbevwarp.so: its bevwarp_remap is timed as one more shared-map arm")
    a = p.parse_args()
    rounds, per_round, warm = arms.counts(a.quick)
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    variants = {}
    for path in a.variant_lib:
        v = ctypes.CDLL(path)
        v.bevwarp_remap.restype, v.bevwarp_remap.argtypes = _lib.SYMBOLS["bevwarp_remap"]
        variants["remap_shared@" + os.path.splitext(os.path.basename(path))[0]] = v
    names = ["lens", "remap_shared", "remap_per_frame", "border_transparent", "warp", "build_map"] + list(variants)
    K = arms.camera_K(SW, SH)
    lens = arms.lens_array(K, LENS_A)
    r2_max = warp.lens_valid_r2(LENS_A)
    border = np.zeros(C)
    nset = 3  # (3 x 199 MB of sources, 3 x 101 MB of destinations -- past the 256 MB Infinity Cache)
    srcs, outs = arms.frame_sets(nset, dev), arms.dest_sets(nset, dev)
    lines = ["# bevwarp_remap (bevwarp_build_map's lens maps) vs bevwarp_warp_lens vs bevwarp_warp_border (TRANSPARENT) vs bevwarp_warp, %d x %dx%dx%d -> %dx%dx%d, uint8, "
             "bilinear; us per launch" % (B, SW, SH, C, D, D, C),
             "# lens A %s, r2_max %.4f; %d rounds x %d launches per arm, arms interleaved; %s" % (LENS_A, r2_max, rounds, per_round, torch.cuda.get_device_name(dev)),
             "# a map: %d x %d x 6 bytes = %.1f MB; remap_shared reads one, remap_per_frame %d" % (D, D, D * D * 6 / 1e6, B)]
    for path in a.variant_lib:
        lines.append("# variant: %s" % path)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for hname, _, Ms in arms.footprints():
        minv = torch.from_numpy(warp.invert_homography(Ms)).to(dev)
        mray = torch.from_numpy(np.ascontiguousarray(warp.ray_matrix(Ms, K))).to(dev)
        shared = arms.lens_map(Ms[0], dev)
        per_frame = [arms.lens_map(Ms, dev) for _ in range(nset)]  # (rotated with the frames: 3 x 201 MB)
        scratch = arms.lens_map(Ms[0], dev)
        torch.cuda.synchronize()
        k = [0]

        def remap(fn, m, head):
            xy, fr, xy_fs, xy_rs, fr_fs, fr_rs = m._planes()
            return fn(*head, xy, fr, m.n, xy_fs, xy_rs, fr_fs, fr_rs, _lib.U8, 1, warp.BORDER_CONSTANT, ptr(border), stream)

        def launch(arm):
            i = k[0] % nset
            k[0] += 1
            head = (srcs[i].data_ptr(), outs[i].data_ptr(), B, SH, SW, D, D, C, SH * SW * C, SW * C, D * D * C, D * C)
            if arm == "lens":
                st = lib.bevwarp_warp_lens(*head, mray.data_ptr(), B, ptr(lens), r2_max, _lib.U8, 1, warp.BORDER_CONSTANT, ptr(border), stream)
            elif arm == "remap_shared":
                st = remap(lib.bevwarp_remap, shared, head)
            elif arm in variants:
                st = remap(variants[arm].bevwarp_remap, shared, head)
            elif arm == "remap_per_frame":
                st = remap(lib.bevwarp_remap, per_frame[i], head)
            elif arm == "border_transparent":
                st = lib.bevwarp_warp_border(*head, minv.data_ptr(), B, _lib.U8, 1, warp.BORDER_TRANSPARENT, None, stream)
            elif arm == "warp":
                st = lib.bevwarp_warp(*head, minv.data_ptr(), B, _lib.U8, 1, ptr(border), stream)
            else:
                xy, fr, xy_fs, xy_rs, fr_fs, fr_rs = scratch._planes()
                st = lib.bevwarp_build_map(mray.data_ptr(), 1, ptr(lens), r2_max, 1, xy, fr, D, D, xy_fs, xy_rs, fr_fs, fr_rs, stream)
            _lib.check(st)

        t = arms.timed(names, launch, rounds, per_round, warm)
        q = arms.p10_50_90(t)
        for arm in names:
            lines.append("%-9s %-21s p10 %8.1f  p50 %8.1f  p90 %8.1f us  (%d launches)" % (hname, arm, q[arm][0], q[arm][1], q[arm][2], len(t[arm])))
        gain = q["lens"][1] - q["remap_shared"][1]
        lines.append("%-9s remap_shared p90 %.1f %s lens p10 %.1f   remap_shared / lens %5.2f   remap_shared / warp %5.2f   remap_per_frame / remap_shared %5.2f   "
                     "break-even %s batches (build %.1f us / gain %.1f us)"
                     % (hname, q["remap_shared"][2], "<=" if q["remap_shared"][2] <= q["lens"][0] else ">", q["lens"][0], q["remap_shared"][1] / q["lens"][1],
                        q["remap_shared"][1] / q["warp"][1], q["remap_per_frame"][1] / q["remap_shared"][1],
                        "%.2f" % (q["build_map"][1] / gain) if gain > 0 else "no", q["build_map"][1], gain))
        for v in variants:
            lines.append("%-9s %s / remap_shared %5.2f" % (hname, v, q[v][1] / q["remap_shared"][1]))
        del per_frame
    arms.finish(lines, a.out)


if __name__ == "__main__":
    main()
