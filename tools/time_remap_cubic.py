#!/usr/bin/env python3
"""Bicubic sampling through a bilinear warp map (bevwarp_remap | BEVWARP_MAP_BICUBIC) against the routes around it, on tools/time_remap.py's
shapes and protocol -- 32 x 1080p -> 1024^2, uint8 x 3 (BASELINE.json configs[1]'s shape), the keystone footprint and the Brno-like BEV.
Arms, interleaved in one process after a warm-up, buffer sets rotated past the Infinity Cache, HIP-event time per launch, p10 / p50 / p90:
    cubic_map_pinhole    bevwarp_remap | BEVWARP_MAP_BICUBIC, ONE pinhole map (matrix 0) shared by the 32 frames, REPLICATE
    cubic_map_lens       the same through a lens-A map (r2_max = lens_valid_r2), CONSTANT: what no other entry offers
    cubic_matrix         bevwarp_warp_border(BEVWARP_CUBIC, REPLICATE), per-frame jitter_H matrices: what cubic_map_pinhole replaces for a
                         fixed camera (and the timing DESIGN.md section 4.10 never had)
    linear_map           bevwarp_remap, bilinear, REPLICATE, through the same pinhole map: 4 taps where bicubic has 16
Before the arms, the box's streaming figure: tools/libstreamprobe.so reading one launch's source bytes and writing its destination bytes
(plain loads, non-temporal stores), in this process on the arms' own buffers.
Derived: cubic_map_pinhole p90 against cubic_matrix p10 (the expectation DESIGN.md section 4.25 judges) and cubic_map_pinhole / linear_map.
GPU box:  python tools/time_remap_cubic.py [--quick] [--out FILE]"""
import ctypes
import os

import numpy as np
import torch

import arms
from arms import B, C, D, LENS_A, SH, SW
from bev_amd import _lib, warp

ARMS = ("cubic_map_pinhole", "cubic_map_lens", "cubic_matrix", "linear_map")


def streaming_probe(srcs, outs, stream):
    """(us, GB/s) of the best of two grids: median over 20 launches each, after 4 unmeasured ones."""
    lib = ctypes.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "libstreamprobe.so"))
    lib.probe_stream.restype = ctypes.c_int
    lib.probe_stream.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    read_b, write_b = srcs[0].numel() // 16 * 16, outs[0].numel() // 16 * 16
    clk = torch.zeros(3, dtype=torch.int64, device=srcs[0].device)
    best = None
    for grid in (4096, 8192):
        k = [0]

        def launch():
            i = k[0] % len(srcs)
            k[0] += 1
            if lib.probe_stream(srcs[i].data_ptr(), read_b, outs[i].data_ptr(), write_b, 0, 1, grid, stream, clk.data_ptr()):
                raise RuntimeError("probe_stream failed")

        arms.event_us(launch, 4)
        t = float(np.median(arms.event_us(launch, 20)))
        best = t if best is None else min(best, t)
    return best, (read_b + write_b) / best / 1e3, read_b, write_b


def main():
    a = arms.parser(__doc__).parse_args()
    rounds, per_round, warm = arms.counts(a.quick)
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    border = np.zeros(C)
    bptr = arms.ptr(border)
    nset = 3  # (3 x 199 MB of sources, 3 x 101 MB of destinations -- past the 256 MB Infinity Cache)
    srcs, outs = arms.frame_sets(nset, dev), arms.dest_sets(nset, dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lines = ["# bevwarp_remap | BEVWARP_MAP_BICUBIC vs bevwarp_warp_border(BEVWARP_CUBIC) vs bevwarp_remap (bilinear), %d x %dx%dx%d -> %dx%dx%d, uint8; us per launch"
             % (B, SW, SH, C, D, D, C),
             "# lens A %s; %d rounds x %d launches per arm, arms interleaved; %s" % (LENS_A, rounds, per_round, torch.cuda.get_device_name(dev))]
    us, gbs, rb, wb = streaming_probe(srcs, outs, stream)
    lines.append("# streaming probe (plain loads, nt stores; reads %d B, writes %d B of one launch's buffers): %.1f us, %.0f GB/s" % (rb, wb, us, gbs))
    for hname, _, Ms in arms.footprints():
        minv = torch.from_numpy(warp.invert_homography(Ms)).to(dev)
        pinhole = warp.build_warp_map(Ms[0], (D, D))
        lens = arms.lens_map(Ms[0], dev)
        torch.cuda.synchronize()
        k = [0]

        def remap(m, interp, mode, head):
            xy, fr, xy_fs, xy_rs, fr_fs, fr_rs = m._planes()
            return lib.bevwarp_remap(*head, xy, fr, m.n, xy_fs, xy_rs, fr_fs, fr_rs, _lib.U8, interp, mode, bptr, stream)

        def launch(arm):
            i = k[0] % nset
            k[0] += 1
            head = (srcs[i].data_ptr(), outs[i].data_ptr(), B, SH, SW, D, D, C, SH * SW * C, SW * C, D * D * C, D * C)
            if arm == "cubic_map_pinhole":
                st = remap(pinhole, _lib.INTER_LINEAR | _lib.MAP_BICUBIC, warp.BORDER_REPLICATE, head)
            elif arm == "cubic_map_lens":
                st = remap(lens, _lib.INTER_LINEAR | _lib.MAP_BICUBIC, warp.BORDER_CONSTANT, head)
            elif arm == "cubic_matrix":
                st = lib.bevwarp_warp_border(*head, minv.data_ptr(), B, _lib.U8, _lib.INTER_CUBIC, warp.BORDER_REPLICATE, None, stream)
            else:
                st = remap(pinhole, _lib.INTER_LINEAR, warp.BORDER_REPLICATE, head)
            _lib.check(st)

        t = arms.timed(ARMS, launch, rounds, per_round, warm)
        q = arms.p10_50_90(t)
        for arm in ARMS:
            lines.append("%-9s %-18s p10 %8.1f  p50 %8.1f  p90 %8.1f us  (%d launches)" % (hname, arm, q[arm][0], q[arm][1], q[arm][2], len(t[arm])))
        p90, p10 = q["cubic_map_pinhole"][2], q["cubic_matrix"][0]
        lines.append("%-9s cubic_map_pinhole p90 %.1f %s cubic_matrix p10 %.1f: expectation %s   cubic_map_pinhole / cubic_matrix %5.2f   cubic_map_pinhole / linear_map %5.2f "
                     "(16 taps against 4)   cubic_map_lens / cubic_map_pinhole %5.2f"
                     % (hname, p90, "<=" if p90 <= p10 else ">", p10, "confirmed" if p90 <= p10 else "refuted", q["cubic_map_pinhole"][1] / q["cubic_matrix"][1],
                        q["cubic_map_pinhole"][1] / q["linear_map"][1], q["cubic_map_lens"][1] / q["cubic_map_pinhole"][1]))
    arms.finish(lines, a.out)


if __name__ == "__main__":
    main()
