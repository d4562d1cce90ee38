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
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bev_amd import _lib, warp  # noqa: E402
from tests import workloads as wl  # noqa: E402

LENS_A = (-0.30, 0.10, 0.001, -0.0005, -0.01)
ARMS = ("cubic_map_pinhole", "cubic_map_lens", "cubic_matrix", "linear_map")


def event_us(launch, n):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in ev:
        e0.record()
        launch()
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]


def streaming_probe(srcs, outs, stream):
    """(us, GB/s) of the best of two grids: median over 20 launches each, after 4 unmeasured ones."""
    lib = ctypes.CDLL(os.path.join(ROOT, "tools", "libstreamprobe.so"))
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

        event_us(launch, 4)
        t = float(np.median(event_us(launch, 20)))
        best = t if best is None else min(best, t)
    return best, (read_b + write_b) / best / 1e3, read_b, write_b


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--quick", action="store_true", help="a few launches per arm")
    p.add_argument("--out", default=None, help="also write the table to this file")
    a = p.parse_args()
    B, SH, SW, D, C = 32, 1080, 1920, 1024, 3
    rounds, per_round, warm = (2, 3, 2) if a.quick else (7, 10, 5)
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    K = np.array([[0.8 * SW, 0, (SW - 1) / 2], [0, 0.816 * SW, (SH - 1) / 2 + 3], [0, 0, 1.0]])
    border = np.zeros(C)
    bptr = border.ctypes.data_as(ctypes.c_void_p)
    nset = 3  # (3 x 199 MB of sources, 3 x 101 MB of destinations -- past the 256 MB Infinity Cache)
    srcs = [torch.from_numpy(np.stack([wl.frame(B * s + i, SH, SW, np.uint8) for i in range(B)])).to(dev) for s in range(nset)]
    outs = [torch.zeros((B, D, D, C), dtype=torch.uint8, device=dev) for _ in range(nset)]
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lines = ["# bevwarp_remap | BEVWARP_MAP_BICUBIC vs bevwarp_warp_border(BEVWARP_CUBIC) vs bevwarp_remap (bilinear), %d x %dx%dx%d -> %dx%dx%d, uint8; us per launch"
             % (B, SW, SH, C, D, D, C),
             "# lens A %s; %d rounds x %d launches per arm, arms interleaved; %s" % (LENS_A, rounds, per_round, torch.cuda.get_device_name(dev))]
    us, gbs, rb, wb = streaming_probe(srcs, outs, stream)
    lines.append("# streaming probe (plain loads, nt stores; reads %d B, writes %d B of one launch's buffers): %.1f us, %.0f GB/s" % (rb, wb, us, gbs))
    for hname, hfn in (("keystone", wl.keystone_H), ("brno", wl.synth_brno_H)):
        H = hfn(SW, SH, D, D)
        Ms = np.stack([wl.jitter_H(H, i) for i in range(B)])
        minv = torch.from_numpy(warp.invert_homography(Ms)).to(dev)
        pinhole = warp.build_warp_map(Ms[0], (D, D))
        lens = warp.build_warp_map(Ms[0], (D, D), K=K, dist_coeff=LENS_A)
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

        for arm in ARMS:
            for _ in range(warm):
                launch(arm)
        torch.cuda.synchronize()
        t = {arm: [] for arm in ARMS}
        for _ in range(rounds):
            for arm in ARMS:
                t[arm] += event_us(lambda: launch(arm), per_round)
        q = {arm: [float(np.percentile(t[arm], v)) for v in (10, 50, 90)] for arm in ARMS}
        for arm in ARMS:
            lines.append("%-9s %-18s p10 %8.1f  p50 %8.1f  p90 %8.1f us  (%d launches)" % (hname, arm, q[arm][0], q[arm][1], q[arm][2], len(t[arm])))
        p90, p10 = q["cubic_map_pinhole"][2], q["cubic_matrix"][0]
        lines.append("%-9s cubic_map_pinhole p90 %.1f %s cubic_matrix p10 %.1f: expectation %s   cubic_map_pinhole / cubic_matrix %5.2f   cubic_map_pinhole / linear_map %5.2f "
                     "(16 taps against 4)   cubic_map_lens / cubic_map_pinhole %5.2f"
                     % (hname, p90, "<=" if p90 <= p10 else ">", p10, "confirmed" if p90 <= p10 else "refuted", q["cubic_map_pinhole"][1] / q["cubic_matrix"][1],
                        q["cubic_map_pinhole"][1] / q["linear_map"][1], q["cubic_map_lens"][1] / q["cubic_map_pinhole"][1]))
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
