#!/usr/bin/env python3
"""The map samplers that write channel planes (bevwarp_remap_planes, bevwarp_stitch_maps_planes, bevwarp_stitch_maps_nv12_planes) against
the routes that exist: 32 x 1080p -> 32 x 3 x 1024^2 planes, bilinear, one shared lens-A map per camera (tests/lens_ref.LENS_A,
lens_valid_r2).  `--step kernels`: arms interleaved in one process after a warm-up, buffer sets rotated past the Infinity Cache, HIP-event
time per arm, p10 / p50 / p90.  On the keystone and the Brno-like footprint:
  (a) bevwarp_remap_planes, float16     against  bevwarp_remap into a BGR BEV + an identity bevwarp_warp_planes at the BEV size (nearest), and
                                                 as a ratio to bevwarp_remap alone and to bevwarp_remap_nv12_planes; float32 planes likewise
and once, on tools/stitch_timing.py's three views:
  (b) bevwarp_stitch_maps_planes        against  bevwarp_stitch_maps + the identity bevwarp_warp_planes: "over" to float16 and to float32,
                                                 "feather" (F = 64) to float16
  (c) bevwarp_stitch_maps_nv12_planes   against  bevwarp_stitch_maps_nv12 + the identity bevwarp_warp_planes, "over", float16
Every baseline is an existing entry measured in the same run.  Each new arm is checked equal, bit for bit, to the route it replaces
before anything is timed.  `--step pipeline`: (d) SitePipeline over 200 sets of 3 x 1080p NV12 frames into float16 planes against three
FramePipeline(warp_map=..., src_format="nv12") rings plus resident launches, both with up to three sets in flight, alternated: ms per set.
GPU box, each step under a time limit of its own and none tried again when it fails:
    timeout -k 10 400 python tools/map_planes_timing.py --step kernels --out profiles/map_planes_timing.txt && \\
    timeout -k 10 300 python tools/map_planes_timing.py --step pipeline --out profiles/map_planes_timing.txt --append"""
import ctypes
import time

import numpy as np
import torch

import arms
from arms import B, D, SH, SW, lens_map, views
from bev_amd import _lib, warp
from bev_amd.pipeline import FramePipeline, SitePipeline
from tests import nv12_ref
from tests import workloads as wl

K = 3
NSET = 2  # (2 x 199 MB of BGR frames per camera, 2 x 100 MB of NV12 planes per camera, 2 x 100 MB of BGR BEVs, 2 x 201 / 403 MB of planes: past the 256 MB Infinity Cache)
SINGLE = (("a_two", "(a) remap + identity warp_planes, f16"), ("a_new", "(a) remap_planes, f16"), ("a_pix", "    remap alone"), ("a_nvp", "    remap_nv12_planes, f16"),
          ("a_two32", "(a) remap + identity warp_planes, f32"), ("a_new32", "(a) remap_planes, f32"))
STITCH = (("b_two", "(b) stitch_maps + identity warp_planes, f16"), ("b_new", "(b) stitch_maps_planes, f16"),
          ("b_two32", "(b) stitch_maps + identity warp_planes, f32"), ("b_new32", "(b) stitch_maps_planes, f32"),
          ("b_twof", "(b) stitch_maps feather + identity warp_planes, f16"), ("b_newf", "(b) stitch_maps_planes feather, f16"),
          ("c_two", "(c) stitch_maps_nv12 + identity warp_planes, f16"), ("c_new", "(c) stitch_maps_nv12_planes, f16"))
PAIRS = (("(a)", "a_two", "a_new", True), ("(a) f32", "a_two32", "a_new32", True), ("(b)", "b_two", "b_new", False), ("(b) f32", "b_two32", "b_new32", False),
         ("(b) feather", "b_twof", "b_newf", False), ("(c)", "c_two", "c_new", False))
EXPECT = ("# expectations, stated before the numbers: (a) p90 of bevwarp_remap_planes (float16) is not above p10 of bevwarp_remap + the identity bevwarp_warp_planes, on either footprint;",
          "#   (b) p90 of bevwarp_stitch_maps_planes (over, float16) is not above p10 of bevwarp_stitch_maps + the identity bevwarp_warp_planes;",
          "#   (c) p90 of bevwarp_stitch_maps_nv12_planes (over, float16) is not above p10 of bevwarp_stitch_maps_nv12 + the identity bevwarp_warp_planes",
          "#   (the float32 and feather rows are reported with the same test, without an expectation of their own)")
SCALE, BIAS = (1 / 255.0, 1 / 255.0, 1 / 255.0), (-0.4, -0.45, -0.5)


def kernels(quick, dev):
    rounds, per_round, warm = arms.counts(quick, (6, 10, 4))
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    foot = {name: H for name, H, _ in arms.footprints()}
    maps = {k: lens_map(M, dev) for k, M in foot.items()}
    cam_maps = [lens_map(M, dev) for M in views()]
    eye = torch.eye(3, dtype=torch.float64, device=dev)[None].contiguous()
    bgr4 = [wl.frame(97 + i, SH, SW, np.uint8) for i in range(4)]
    nv4 = [nv12_ref.frame("video", 131 + i, SH, SW) for i in range(4)]
    # (four distinct frames, repeated over the batch with a rotation of its own per set and camera: the timing does not depend on the values)
    pick = lambda four, r: torch.from_numpy(np.stack([four[(i + r) % 4] for i in range(B)])).to(dev)  # noqa: E731
    srcs = [[pick(bgr4, s + k) for k in range(K)] for s in range(NSET)]
    ys = [[pick([f[0] for f in nv4], s + k) for k in range(K)] for s in range(NSET)]
    uvs = [[pick([f[1] for f in nv4], s + k) for k in range(K)] for s in range(NSET)]
    bev = arms.dest_sets(NSET, dev)
    out = {16: arms.dest_sets(NSET, dev, (B, 3, D, D), torch.float16), 32: arms.dest_sets(NSET, dev, (B, 3, D, D), torch.float32)}
    sc, bi = np.array(SCALE, np.float64), np.array(BIAS, np.float64)
    psc, pbi = arms.ptr(sc), arms.ptr(bi)
    cams = {"bgr": [], "nv12": []}
    for s in range(NSET):
        for kind in cams:
            arr = (_lib.MapCamera * K)()
            for k in range(K):
                xy_p, fr_p, xy_fs, xy_rs, fr_fs, fr_rs = cam_maps[k]._planes()
                if kind == "nv12":
                    arr[k] = _lib.MapCamera(ys[s][k].data_ptr(), uvs[s][k].data_ptr(), SH * SW, SW, SH * SW // 2, SW, xy_p, fr_p, xy_fs, xy_rs, fr_fs, fr_rs, SH, SW, 1, 0)
                else:
                    arr[k] = _lib.MapCamera(srcs[s][k].data_ptr(), None, SH * SW * 3, SW * 3, 0, 0, xy_p, fr_p, xy_fs, xy_rs, fr_fs, fr_rs, SH, SW, 1, 0)
            cams[kind].append(arr)
    n = [0]
    CONSTANT, OVER, FEATHER = warp.BORDER_CONSTANT, _lib.STITCH_OVER, _lib.STITCH_FEATHER

    def launch(key, fp, i=None):
        if i is None:
            i = n[0] % NSET
            n[0] += 1
        bits = 32 if key.endswith("32") else 16
        esz, pdt = bits // 8, (_lib.F32 if bits == 32 else _lib.F16)
        o, dst = out[bits][i].data_ptr(), (3 * D * D * esz, D * D * esz, D * esz)
        b, bev_strides = bev[i].data_ptr(), (D * D * 3, D * 3)
        nv_src, bgr_src = (SH * SW, SW, SH * SW // 2, SW), (SH * SW * 3, SW * 3)
        m = () if fp is None else maps[fp]._planes()[:2] + (1,) + maps[fp]._planes()[2:]
        planes_tail = (None, psc, pbi, pdt, stream)
        identity = lambda: _lib.check(lib.bevwarp_warp_planes(b, o, B, D, D, D, D, 3, *bev_strides, *dst, eye.data_ptr(), 1, _lib.U8, 0, *planes_tail))  # noqa: E731
        base = key[:5]
        if base in ("a_two", "a_pix"):
            _lib.check(lib.bevwarp_remap(srcs[i][0].data_ptr(), b, B, SH, SW, D, D, 3, *bgr_src, *bev_strides, *m, _lib.U8, 1, CONSTANT, None, stream))
            if base == "a_two":
                identity()
        elif base == "a_new":
            _lib.check(lib.bevwarp_remap_planes(srcs[i][0].data_ptr(), o, B, SH, SW, D, D, *bgr_src, *dst, *m, 1, CONSTANT, *planes_tail))
        elif base == "a_nvp":
            _lib.check(lib.bevwarp_remap_nv12_planes(ys[i][0].data_ptr(), uvs[i][0].data_ptr(), o, B, SH, SW, D, D, *nv_src, *dst, *m, 1, CONSTANT, 0, *planes_tail))
        elif base == "b_two":
            blend = FEATHER if key.endswith("f") else OVER
            _lib.check(lib.bevwarp_stitch_maps(ctypes.addressof(cams["bgr"][i]), K, b, B, D, D, 3, *bev_strides, _lib.U8, 1, blend, 64, CONSTANT, None, stream))
            identity()
        elif base == "b_new":
            blend = FEATHER if key.endswith("f") else OVER
            _lib.check(lib.bevwarp_stitch_maps_planes(ctypes.addressof(cams["bgr"][i]), K, o, B, D, D, *dst, 1, blend, 64, *planes_tail))
        elif base == "c_two":
            _lib.check(lib.bevwarp_stitch_maps_nv12(ctypes.addressof(cams["nv12"][i]), K, b, B, D, D, *bev_strides, 1, OVER, 64, 0, CONSTANT, None, stream))
            identity()
        else:
            _lib.check(lib.bevwarp_stitch_maps_nv12_planes(ctypes.addressof(cams["nv12"][i]), K, o, B, D, D, *dst, 1, OVER, 64, 0, *planes_tail))

    # results must not change: every new arm leaves, bit for bit, the planes of the two-launch route it replaces, at the timed size
    rows = [(key, label, fp) for fp in foot for key, label in SINGLE] + [(key, label, None) for key, label in STITCH]
    for _, two, new, single in PAIRS:
        for fp in (foot if single else (None,)):
            o = out[32 if two.endswith("32") else 16][0]
            launch(two, fp, 0)
            torch.cuda.synchronize()
            kept = o.clone()
            o.fill_(33)
            launch(new, fp, 0)
            torch.cuda.synchronize()
            if not torch.equal(o.view(torch.int16), kept.view(torch.int16)):
                raise SystemExit("%s and %s disagree on %s" % (two, new, fp))
            del kept
    lines = ["# bevwarp_remap_planes / bevwarp_stitch_maps_planes / bevwarp_stitch_maps_nv12_planes vs the existing entry into a BGR BEV + an identity bevwarp_warp_planes (nearest):",
             "# %d x %dx%d (BGR, or NV12 planes) -> %d x 3 x %dx%d planes, bilinear, one shared lens-A map per camera, BORDER_CONSTANT; us per batch" % (B, SW, SH, B, D, D),
             "# (b), (c): %d cameras, tools/stitch_timing.py's views; %d rounds x %d runs per arm, arms interleaved; %s" % (K, rounds, per_round, torch.cuda.get_device_name(dev)),
             "# checked before timing: each new arm leaves bit for bit the planes of the two-launch route beside it; the baselines are entries this change does not touch"]
    lines += list(EXPECT)
    t = arms.timed([(key, fp) for key, _, fp in rows], lambda arm: launch(*arm), rounds, per_round, warm)
    q = arms.p10_50_90(t)
    for key, label, fp in rows:
        lines.append("%-9s %-52s p10 %8.1f  p50 %8.1f  p90 %8.1f us  (%d runs)" % ((fp or "3 views", label) + tuple(q[key, fp]) + (len(t[key, fp]),)))
    for name, two, new, single in PAIRS:
        expected = name in ("(a)", "(b)", "(c)")
        for fp in (foot if single else (None,)):
            T, N = q[two, fp], q[new, fp]
            ok = N[2] <= T[0]
            verdict = ("confirmed" if ok else "refuted") if expected else ("holds" if ok else "does not hold")
            lines.append("%-11s %-8s new p90 not above the two-launch route's p10 (%.1f vs %.1f us): %s   new / route p50 %.2f" % (name, fp or "3 views", N[2], T[0], verdict, N[1] / T[1]))
    for fp in foot:
        lines.append("(a) %-8s remap_planes f16 / remap alone p50 %.2f   / remap_nv12_planes f16 p50 %.2f" % (fp, q["a_new", fp][1] / q["a_pix", fp][1], q["a_new", fp][1] / q["a_nvp", fp][1]))
    return lines


def site_ms(pipe, frames, n):
    for _ in range(3):  # fill the slots once: afterwards the "decoders" find their frames already in pinned memory
        for buf, f in zip(pipe.next_inputs(), frames):
            buf[...] = f
        pipe.commit()
    for _ in range(3):
        pipe.result()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        pipe.next_inputs()
        pipe.commit()
        if pipe.ready() >= 3:
            pipe.result()
    while pipe.ready():
        pipe.result()
    return (time.perf_counter() - t0) / n * 1e3


def rings_ms(rings, frames, n, dev):
    """What a site could build before SitePipeline: one FramePipeline(warp_map=..., src_format="nv12") ring of depth 3 per camera that
    leaves its BGR BEV on the device, then resident launches on the current stream -- bevwarp_warp_stitch of the three BEVs under identity
    matrices ("over") and an identity warp_to_planar to float16 -- and a copy of the planes into pinned memory.  Pipelined as a user would
    run it: set i + 1 and set i + 2 are committed before set i's BEVs are taken, so two sets' uploads and remaps are in flight while the host
    enqueues the resident launches of a third; an event per slot keeps a ring from overwriting a BEV those launches still read.  (The
    canvas is not the stitch's: a ring's BEV no longer says which pixels its camera covers.  The costs are what is compared.)"""
    eye = [np.eye(3)] * len(rings)
    host = torch.empty((3, D, D), dtype=torch.float16, pin_memory=True)
    planes = torch.empty((3, D, D), dtype=torch.float16, device=dev)
    read = [None] * 3  # per ring slot: the resident launches that read its BEVs have finished
    state = {"in": 0, "out": 0}

    def take():
        bevs = [ring.result() for ring in rings]
        canvas = warp.warp_stitch(bevs, eye, (D, D), flags=warp.INTER_NEAREST)
        warp.warp_to_planar(canvas, np.eye(3), (D, D), scale=SCALE, bias=BIAS, flags=warp.INTER_NEAREST, out=planes, out_dtype=torch.float16)
        host.copy_(planes, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        read[state["out"] % 3] = ev
        state["out"] += 1

    def one_set(fill):
        if read[state["in"] % 3] is not None:
            read[state["in"] % 3].synchronize()
        for ring, f in zip(rings, frames):
            buf = ring.next_input()
            if fill:
                buf[...] = f
            ring.commit()
        state["in"] += 1
        if rings[0].ready() >= 3:
            take()

    for _ in range(3):
        one_set(True)
    while rings[0].ready():
        take()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        one_set(False)
    while rings[0].ready():
        take()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def pipeline(quick, dev):
    n = 40 if quick else 200
    cam_maps = [lens_map(M, dev) for M in views()]
    frames = [nv12_ref.join(*nv12_ref.frame("video", 3 + k, SH, SW)) for k in range(K)]
    lines = ["# (d) %d sets of %d x %dx%d NV12 frames -> 3 x %dx%d float16 planes, lens-A maps on tools/stitch_timing.py's views, depth 3: ms per set (host clock around the loop), 3 repeats, arms alternated" % (
        n, K, SW, SH, D, D)]
    ms = {"site": [], "rings": []}
    for _ in range(3):
        with SitePipeline([(SH, SW)] * K, cam_maps, (D, D), depth=3, src_format="nv12", dst_format="planes", scale=SCALE, bias=BIAS, plane_dtype=torch.float16) as pipe:
            ms["site"].append(site_ms(pipe, frames, n))
        rings = [FramePipeline((SH, SW), 3, None, (D, D), depth=3, src_format="nv12", warp_map=m, download=False) for m in cam_maps]
        try:
            ms["rings"].append(rings_ms(rings, frames, n, dev))
        finally:
            for ring in rings:
                ring.close()
    lines.append("pipeline  SitePipeline, nv12 -> float16 planes: one stitch launch per set                       ms per set  median %7.4f  min %7.4f  max %7.4f" % (
        float(np.median(ms["site"])), min(ms["site"]), max(ms["site"])))
    lines.append("pipeline  3 FramePipeline(warp_map, nv12) rings, pipelined, + resident warp_stitch + warp_to_planar + D2H  ms per set  median %7.4f  min %7.4f  max %7.4f" % (
        float(np.median(ms["rings"])), min(ms["rings"]), max(ms["rings"])))
    lines.append("pipeline  SitePipeline - rings  %+.4f ms per set (median)   SitePipeline / rings %5.3f" % (
        float(np.median(ms["site"])) - float(np.median(ms["rings"])), float(np.median(ms["site"])) / float(np.median(ms["rings"]))))
    return lines


def main():
    a = arms.parser(__doc__, steps=("kernels", "pipeline")).parse_args()
    dev = torch.device("cuda", 0)
    arms.finish((kernels if a.step == "kernels" else pipeline)(a.quick, dev), a.out, a.append)


if __name__ == "__main__":
    main()
