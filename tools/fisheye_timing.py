#!/usr/bin/env python3
"""The fisheye lens model (BEVWARP_LENS_FISHEYE) against the rational one, arm by arm, on BASELINE configs[1] -- 32 x 1080p -> 1024^2,
per-frame jitter_H matrices, uint8 BGR, bilinear -- with the keystone footprint and the Brno-like BEV (synth_brno_H):

  warp      bevwarp_warp_lens, rational | fisheye
  build     one bevwarp_build_map of a 1024^2 map, rational | fisheye
  remap     bevwarp_remap of the 32 frames through either map (the sampler is the same code: these two must tie)
  points    1e7 float64 points through bevwarp_project_points_lens: DISTORT, UNDISTORT at 5 and at 10 steps, rational | fisheye

The arms call the C ABI with bound arguments, interleaved in one process after a warm-up (forwards and backwards, so that drift hits them
alike), buffer sets rotated past the 256 MB Infinity Cache; HIP-event time per launch, p10 / p50 / p90, and fisheye / rational of the p50s.
The header states the prediction made from the kernels' static instruction counts before the first run.
GPU box:  python tools/fisheye_timing.py [--quick] [--out FILE]"""
import ctypes

import numpy as np
import torch

import arms
from arms import B, C, D, LENS_A, SH, SW, ptr
from bev_amd import _lib, warp

FISHEYE_K = (-0.02, 0.004, -0.001, 0.0002)
FISHEYE = warp.LENS_FISHEYE
PREDICTION = """# prediction (static instruction counts of the gfx950 code objects, all / float64, made before the first run):
#   build_map bilinear   rational 719 / 356, fisheye 1259 / 556 -> the builder is float64-bound: 1.55 - 1.75 x
#   warp_lens u8x3 bilinear constant   rational 1033 / 356, fisheye 1571 / 556 -> at most 1.5 x, less where the taps' latency hides it
#   remap through either map   the same kernel on maps of the same format: 1.00 x
#   points float64   DISTORT 117 / 73 -> 255 / 123: 1.7 - 2.2 x; UNDISTORT per step one division (rational) against three and
#   atan_pos (fisheye): 2 - 3 x at equal steps, so 10 fisheye steps cost about what 20 - 30 rational ones do"""


def report(lines, tag, t, pairs):
    q = arms.p10_50_90(t)
    for arm in t:
        lines.append("%-9s %-22s p10 %9.1f  p50 %9.1f  p90 %9.1f us  (%d launches)" % (tag, arm, q[arm][0], q[arm][1], q[arm][2], len(t[arm])))
    for num, den in pairs:
        lines.append("%-9s %s / %s  %.3f" % (tag, num, den, q[num][1] / q[den][1]))


def main():
    a = arms.parser(__doc__).parse_args()
    assert torch.cuda.is_available(), "no HIP device: nothing to time"
    rounds, per_round, warm = arms.counts(a.quick, (8, 8, 4))
    N = 1_000_000 if a.quick else 10_000_000  # (--quick: 1e6 points)

    def timed(names, launch):
        return arms.timed(names, launch, rounds, per_round, warm, order="alternate")

    dev = torch.device("cuda", 0)
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    K = arms.camera_K(SW, SH)
    lens = {"rational": arms.lens_array(K, LENS_A), "fisheye": arms.lens_array(K, FISHEYE_K)}
    limit = {"rational": warp.lens_valid_r2(LENS_A), "fisheye": warp.fisheye_valid_theta(FISHEYE_K)}
    flag = {"rational": 0, "fisheye": FISHEYE}
    border = np.zeros(C)
    nset = 3  # (3 x 199 MB of sources, 3 x 101 MB of destinations -- past the 256 MB Infinity Cache)
    gen = torch.Generator(device=dev).manual_seed(1)
    srcs = [torch.randint(0, 256, (B, SH, SW, C), dtype=torch.uint8, device=dev, generator=gen) for _ in range(nset)]
    outs = arms.dest_sets(nset, dev)
    lines = ["# BEVWARP_LENS_FISHEYE against the rational model, %d x %dx%dx%d -> %dx%dx%d, uint8, bilinear, per-frame jitter_H; us per launch" % (B, SW, SH, C, D, D, C),
             "# rational %s, r2_max %.4f; fisheye %s, theta_max %.4f; %d rounds x %d launches per arm, arms interleaved; %s"
             % (LENS_A, limit["rational"], FISHEYE_K, limit["fisheye"], rounds, per_round, torch.cuda.get_device_name(dev)), PREDICTION]
    models = ("rational", "fisheye")
    for hname, _, Ms in arms.footprints():
        mray = {"rational": torch.from_numpy(np.ascontiguousarray(warp.ray_matrix(Ms, K))).to(dev),
                "fisheye": torch.from_numpy(np.ascontiguousarray(warp.ray_matrix(Ms, K, oriented=True))).to(dev)}
        k = [0]

        def launch_warp(arm):
            i = k[0] % nset
            k[0] += 1
            _lib.check(lib.bevwarp_warp_lens(srcs[i].data_ptr(), outs[i].data_ptr(), B, SH, SW, D, D, C, SH * SW * C, SW * C, D * D * C, D * C, mray[arm].data_ptr(), B,
                                             ptr(lens[arm]), limit[arm], _lib.U8, 1 | flag[arm], warp.BORDER_CONSTANT, ptr(border), stream))

        report(lines, hname, timed(models, launch_warp), [("fisheye", "rational")])

        # one map of the first frame's matrix; 64 map sets (6 MB each) rotated past the cache for the builder
        nmap = 64
        xy = [torch.empty((1, D, D, 2), dtype=torch.int16, device=dev) for _ in range(nmap)]
        fr = [torch.empty((1, D, D), dtype=torch.int16, device=dev) for _ in range(nmap)]

        def launch_build(arm, j=None):
            j = k[0] % nmap if j is None else j
            k[0] += 1
            _lib.check(lib.bevwarp_build_map(mray[arm].data_ptr(), 1, ptr(lens[arm]), limit[arm], 1 | flag[arm], xy[j].data_ptr(), fr[j].data_ptr(), D, D, 0, D * 4, 0, D * 2,
                                             stream))

        report(lines, hname, {"build " + m: v for m, v in timed(models, launch_build).items()}, [("build fisheye", "build rational")])
        slot = {"rational": 0, "fisheye": 1}
        for m in models:
            launch_build(m, slot[m])
        torch.cuda.synchronize()

        def launch_remap(arm):
            i, j = k[0] % nset, slot[arm]
            k[0] += 1
            _lib.check(lib.bevwarp_remap(srcs[i].data_ptr(), outs[i].data_ptr(), B, SH, SW, D, D, C, SH * SW * C, SW * C, D * D * C, D * C, xy[j].data_ptr(), fr[j].data_ptr(), 1,
                                         0, D * 4, 0, D * 2, _lib.U8, 1, warp.BORDER_CONSTANT, ptr(border), stream))

        report(lines, hname, {"remap " + m: v for m, v in timed(models, launch_remap).items()}, [("remap fisheye", "remap rational")])
        del xy, fr
    del srcs, outs
    torch.cuda.empty_cache()

    # points: raw-frame pixels for UNDISTORT, the same coordinates as destination-plane points for DISTORT
    nbuf = max(2, int(np.ceil(600e6 / (N * 32))))
    wh = torch.tensor([SW, SH], dtype=torch.float64, device=dev)
    ins = [torch.rand((N, 2), dtype=torch.float64, device=dev) * wh for _ in range(nbuf)]
    pouts = [torch.empty_like(x) for x in ins]
    R = {"rational": np.ascontiguousarray(warp.ray_matrix(np.eye(3), K, inverse_given=True)), "fisheye": np.ascontiguousarray(warp.ray_matrix(np.eye(3), K, inverse_given=True, oriented=True))}
    Kc = np.ascontiguousarray(K)
    cases = [(m, d, it) for d, it in ((0, 0), (1, 5), (1, 10)) for m in models]
    names = {arm: "%s %s" % (("distort", "undistort_%d" % arm[2])[arm[1]], arm[0]) for arm in cases}
    k = [0]

    def launch_points(arm):
        m, d, it = arm
        i = k[0] % nbuf
        k[0] += 1
        _lib.check(lib.bevwarp_project_points_lens(ins[i].data_ptr(), pouts[i].data_ptr(), None, N, ptr(R[m]) if d == 0 else ptr(Kc), ptr(lens[m]), limit[m], d | flag[m], it, 1e-3,
                                                   _lib.F64, stream))

    t = timed(cases, launch_points)
    report(lines, "points", {names[arm]: v for arm, v in t.items()}, [(names[("fisheye", d, it)], names[("rational", d, it)]) for d, it in ((0, 0), (1, 5), (1, 10))])
    lines.append("# points: %d float64 points per launch" % N)
    arms.finish(lines, a.out)


if __name__ == "__main__":
    main()
