#!/usr/bin/env python3
"""Times of the lens point projection against project_points, interleaved in one process: python tools/time_points_lens.py [N]

Arms, per dtype (float32, float64), N = 1e7 points of a 1920 x 1080 frame each: project_points (the baseline), DISTORT, UNDISTORT at
5 and at 20 steps.  Buffers are rotated over more than the 256 MB cache; every launch is timed on its own with device events; the
arms alternate round by round (forwards, backwards) so that drift hits them alike.  Prints p10 / p50 / p90 per arm and the p50 ratio
to project_points (profiles/points_lens_timing.txt)."""
import ctypes
import sys

import numpy as np
import torch

import arms
from arms import LENS_A as DIST, SH as H, SW as W, ptr
from bev_amd import _lib
from bev_amd.warp import lens_valid_r2, ray_matrix

N = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
ROUNDS, DISCARD = 44, 4
K = arms.camera_K(W, H)

assert torch.cuda.is_available(), "no HIP device: nothing to time"
lib = _lib.load()
dev = torch.device("cuda", 0)
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

H_plain = np.ascontiguousarray(np.array([[0.02, -0.001, -3.0], [0.0004, 0.05, -20.0], [1e-5, 0.0009, 0.4]]))  # tools/ab_points.py's
R = np.ascontiguousarray(ray_matrix(np.eye(3), K, inverse_given=True))  # undistorted pixels -> normalised plane
Kc = np.ascontiguousarray(K)                                          # normalised plane -> undistorted pixels
lens = arms.lens_array(K, DIST)
r2_max = lens_valid_r2(DIST)

print("device: %s, N = %d, %d timed launches per arm" % (torch.cuda.get_device_name(0), N, ROUNDS - DISCARD))
for tdt, code, esz in ((torch.float32, _lib.F32, 4), (torch.float64, _lib.F64, 8)):
    nbuf = max(2, int(np.ceil(600e6 / (N * 2 * esz * 2))))
    ins = [(torch.rand((N, 2), dtype=torch.float64, device=dev) * torch.tensor([W, H], dtype=torch.float64, device=dev)).to(tdt) for _ in range(nbuf)]
    outs = [torch.empty_like(x) for x in ins]

    def plain(i, o):
        return lib.bevwarp_project_points(i, o, N, 2, ptr(H_plain), code, stream)

    def distort(i, o):
        return lib.bevwarp_project_points_lens(i, o, None, N, ptr(R), ptr(lens), r2_max, 0, 0, 0.0, code, stream)

    def undistort(iters):
        return lambda i, o: lib.bevwarp_project_points_lens(i, o, None, N, ptr(Kc), ptr(lens), r2_max, 1, iters, 1e-3, code, stream)

    arms = [("project_points", plain), ("distort", distort), ("undistort_5", undistort(5)), ("undistort_20", undistort(20))]
    times = {label: [] for label, _ in arms}
    it = 0
    for r in range(ROUNDS):
        for label, fn in (arms if r % 2 == 0 else arms[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            assert fn(ins[it % nbuf].data_ptr(), outs[it % nbuf].data_ptr()) == 0
            e1.record()
            it += 1
            e1.synchronize()
            if r >= DISCARD:
                times[label].append(e0.elapsed_time(e1) * 1e3)
    base = np.median(times["project_points"])
    for label, _ in arms:
        t = np.array(times[label])
        p10, p50, p90 = np.percentile(t, [10, 50, 90])
        print("%s %-15s p10 %8.1f  p50 %8.1f  p90 %8.1f us   %.2f x project_points   %.2f TB/s (p50, in + out)" %
              (str(tdt)[6:], label, p10, p50, p90, p50 / base, N * 4 * esz / p50 / 1e6))
    del ins, outs
    torch.cuda.empty_cache()
