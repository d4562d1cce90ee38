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
    p.add_argument("--variant-lib", action="append", default=[], help="another build of libbevwarp.so: its bevwarp_remap is timed as one more shared-map arm")
    a = p.parse_args()
    B, SH, SW, D, C = 32, 1080, 1920, 1024, 3
    rounds, per_round, warm = (2, 3, 2) if a.quick else (7, 10, 5)
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    variants = {}
    for path in a.variant_lib:
        v = ctypes.CDLL(path)
        v.bevwarp_remap.restype, v.bevwarp_remap.argtypes = _lib.SYMBOLS["bevwarp_remap"]
        variants["remap_shared@" + os.path.splitext(os.path.basename(path))[0]] = v
    arms = ["lens", "remap_shared", "remap_per_frame", "border_transparent", "warp", "build_map"] + list(variants)
    K = np.array([[0.8 * SW, 0, (SW - 1) / 2], [0, 0.816 * SW, (SH - 1) / 2 + 3], [0, 0, 1.0]])
    lens = np.ascontiguousarray(np.concatenate([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]], LENS_A, [0.0, 0.0, 0.0]]))
    r2_max = warp.lens_valid_r2(LENS_A)
    border = np.zeros(C)
    nset = 3  # (3 x 199 MB of sources, 3 x 101 MB of destinations -- past the 256 MB Infinity Cache)
    srcs = [torch.from_numpy(np.stack([wl.frame(B * s + i, SH, SW, np.uint8) for i in range(B)])).to(dev) for s in range(nset)]
    outs = [torch.zeros((B, D, D, C), dtype=torch.uint8, device=dev) for _ in range(nset)]
    lines = ["# bevwarp_remap (bevwarp_build_map's lens maps) vs bevwarp_warp_lens vs bevwarp_warp_border (TRANSPARENT) vs bevwarp_warp, %d x %dx%dx%d -> %dx%dx%d, uint8, "
             "bilinear; us per launch" % (B, SW, SH, C, D, D, C),
             "# lens A %s, r2_max %.4f; %d rounds x %d launches per arm, arms interleaved; %s" % (LENS_A, r2_max, rounds, per_round, torch.cuda.get_device_name(dev)),
             "# a map: %d x %d x 6 bytes = %.1f MB; remap_shared reads one, remap_per_frame %d" % (D, D, D * D * 6 / 1e6, B)]
    for path in a.variant_lib:
        lines.append("# variant: %s" % path)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for hname, hfn in (("keystone", wl.keystone_H), ("brno", wl.synth_brno_H)):
        H = hfn(SW, SH, D, D)
        Ms = np.stack([wl.jitter_H(H, i) for i in range(B)])
        minv = torch.from_numpy(warp.invert_homography(Ms)).to(dev)
        mray = torch.from_numpy(np.ascontiguousarray(warp.ray_matrix(Ms, K))).to(dev)
        shared = warp.build_warp_map(Ms[0], (D, D), K=K, dist_coeff=LENS_A)
        per_frame = [warp.build_warp_map(Ms, (D, D), K=K, dist_coeff=LENS_A) for _ in range(nset)]  # (rotated with the frames: 3 x 201 MB)
        scratch = warp.build_warp_map(Ms[0], (D, D), K=K, dist_coeff=LENS_A)
        torch.cuda.synchronize()
        k = [0]

        def remap(fn, m, head):
            xy, fr, xy_fs, xy_rs, fr_fs, fr_rs = m._planes()
            return fn(*head, xy, fr, m.n, xy_fs, xy_rs, fr_fs, fr_rs, _lib.U8, 1, warp.BORDER_CONSTANT, border.ctypes.data_as(ctypes.c_void_p), stream)

        def launch(arm):
            i = k[0] % nset
            k[0] += 1
            head = (srcs[i].data_ptr(), outs[i].data_ptr(), B, SH, SW, D, D, C, SH * SW * C, SW * C, D * D * C, D * C)
            if arm == "lens":
                st = lib.bevwarp_warp_lens(*head, mray.data_ptr(), B, lens.ctypes.data_as(ctypes.c_void_p), r2_max, _lib.U8, 1, warp.BORDER_CONSTANT,
                                           border.ctypes.data_as(ctypes.c_void_p), stream)
            elif arm == "remap_shared":
                st = remap(lib.bevwarp_remap, shared, head)
            elif arm in variants:
                st = remap(variants[arm].bevwarp_remap, shared, head)
            elif arm == "remap_per_frame":
                st = remap(lib.bevwarp_remap, per_frame[i], head)
            elif arm == "border_transparent":
                st = lib.bevwarp_warp_border(*head, minv.data_ptr(), B, _lib.U8, 1, warp.BORDER_TRANSPARENT, None, stream)
            elif arm == "warp":
                st = lib.bevwarp_warp(*head, minv.data_ptr(), B, _lib.U8, 1, border.ctypes.data_as(ctypes.c_void_p), stream)
            else:
                xy, fr, xy_fs, xy_rs, fr_fs, fr_rs = scratch._planes()
                st = lib.bevwarp_build_map(mray.data_ptr(), 1, lens.ctypes.data_as(ctypes.c_void_p), r2_max, 1, xy, fr, D, D, xy_fs, xy_rs, fr_fs, fr_rs, stream)
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
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
