"""What the interleaved-arm timing scripts of tools/ share, defined once: the measuring protocol and the scene of BASELINE configs[1].
No product code.  A script run as `python tools/NAME.py` imports it as `arms`; importing it puts the repository root on sys.path.

Protocol: every arm is warmed, then `rounds` rounds of `per_round` launches per arm, each launch between two HIP events, one synchronise
per arm and round; (7, 10, 5) rounds / launches / warm-ups unless the script says otherwise, (2, 3, 2) under --quick; p10 / p50 / p90 of
the times; the table printed and, with --out, written.  The order of the arms is the script's: "fixed", or "alternate" (reversed every
other round, so that drift hits the arms alike).

Scene: 32 x 1080p -> 1024^2 x 3; the tests' lens A on the tests' camera matrix; tests/workloads.frame(B * s + i) frames in `nset`
buffer sets that a launch rotates through, so that the working set stays past the 256 MB Infinity Cache; the keystone footprint and the
Brno-like BEV with per-frame jitter_H matrices; the three stitch views; the NV12 stand-in and the frame-pipeline loop."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import workloads as wl  # noqa: E402
from tests.lens_ref import LENS_A, camera_K, lens12  # noqa: E402, F401

B, SH, SW, D, C = 32, 1080, 1920, 1024, 3


# ---- protocol

def parser(doc, steps=None, step=None):
    """--quick and --out; with `steps`, --step (required unless `step` names the default) and --append."""
    p = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--quick", action="store_true", help="a few launches per arm (for a profiler run)")
    p.add_argument("--out", default=None, help="also write the table to this file")
    if steps:
        p.add_argument("--step", choices=steps, default=step, required=step is None)
        p.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    return p


def counts(quick, full=(7, 10, 5)):
    """(rounds, per_round, warm)."""
    return (2, 3, 2) if quick else full


def _cuda(event, sync):
    if event is None or sync is None:
        import torch
        event, sync = event or (lambda: torch.cuda.Event(enable_timing=True)), sync or torch.cuda.synchronize
    return event, sync


def event_us(launch, n, event=None, sync=None):
    """[us per launch] of n launch() calls, each between two events, one synchronise after the last."""
    event, sync = _cuda(event, sync)
    ev = [(event(), event()) for _ in range(n)]
    for e0, e1 in ev:
        e0.record()
        launch()
        e1.record()
    sync()
    return [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]


def timed(arms, launch, rounds, per_round, warm, order="fixed", warm_arms=None, event=None, sync=None):
    """{arm: [us per launch]}: `warm` launch(arm) calls per arm (of `warm_arms`, where given), arm by arm, and one synchronise; then
    `rounds` rounds of event_us(launch(arm), per_round) per arm, the arms in the given order ("fixed") or reversed every other round
    ("alternate")."""
    assert order in ("fixed", "alternate"), order
    event, sync = _cuda(event, sync)
    arms = list(arms)
    for arm in (arms if warm_arms is None else warm_arms):
        for _ in range(warm):
            launch(arm)
    sync()
    t = {arm: [] for arm in arms}
    for r in range(rounds):
        for arm in (arms[::-1] if order == "alternate" and r % 2 else arms):
            t[arm] += event_us(lambda: launch(arm), per_round, event, sync)
    return t


def p10_50_90(t):
    """{arm: [p10, p50, p90]} of timed()'s result."""
    return {arm: [float(x) for x in np.percentile(v, (10, 50, 90))] for arm, v in t.items()}


def finish(lines, out, append=False):
    """Print the table; with `out`, write it there too (or append it)."""
    text = "\n".join(lines)
    print(text, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a" if append else "w") as f:
            f.write(text + "\n")


# ---- scene

def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def lens_array(K, coeffs):
    """fx, fy, cx, cy and the coefficients, padded to the 12 doubles the C ABI reads."""
    return np.ascontiguousarray(lens12(K, coeffs))


def frame_set(s, dev, dtype=np.uint8):
    """Buffer set s: the B distinct 1080p frames B * s .. B * s + B - 1 of tests/workloads, on the device."""
    import torch
    return torch.from_numpy(np.stack([wl.frame(B * s + i, SH, SW, dtype) for i in range(B)])).to(dev)


def frame_sets(nset, dev, dtype=np.uint8):
    return [frame_set(s, dev, dtype) for s in range(nset)]


def dest_sets(nset, dev, shape=(B, D, D, C), dtype=None):
    import torch
    return [torch.zeros(shape, dtype=dtype or torch.uint8, device=dev) for _ in range(nset)]


def footprints():
    """(name, H, the B jittered matrices of H) of the keystone footprint and of the Brno-like BEV."""
    for name, fn in (("keystone", wl.keystone_H), ("brno", wl.synth_brno_H)):
        H = fn(SW, SH, D, D)
        yield name, H, np.stack([wl.jitter_H(H, i) for i in range(B)])


def views():
    """Forward matrices of the three stitch cameras: the Brno-like view turned by -12, 0 and +12 degrees about the canvas centre and
    shifted by -180, 0 and +180 canvas pixels."""
    H = wl.synth_brno_H(SW, SH, D, D)
    out = []
    for deg, dx in ((-12.0, -180.0), (0.0, 0.0), (12.0, 180.0)):
        t, c = np.deg2rad(deg), (D - 1) / 2.0
        R = np.array([[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1.0]])
        T0, T1 = np.array([[1, 0, -c], [0, 1, -c], [0, 0, 1.0]]), np.array([[1, 0, c + dx], [0, 1, c], [0, 0, 1.0]])
        out.append(T1 @ R @ T0 @ H)
    return out


def lens_map(M, dev):
    """The 1024^2 lens-A warp map of forward matrix M."""
    from bev_amd import warp
    return warp.build_warp_map(M, (D, D), K=camera_K(SW, SH), dist_coeff=LENS_A, device=dev)


def to_nv12(bgr):
    """(B, H, W, 3) uint8 BGR on the device -> (B, H * 3 / 2, W) NV12: BT.601 limited range, chroma averaged over 2 x 2 (a stand-in for an
    encoder, so that the NV12 arm reads frames with the statistics of the BGR arm's; the timing does not depend on the values)."""
    import torch
    f = bgr.float()
    b, g, r = f[..., 0], f[..., 1], f[..., 2]
    y = (0.257 * r + 0.504 * g + 0.098 * b + 16.0).round().clamp(0, 255)
    u = (-0.148 * r - 0.291 * g + 0.439 * b + 128.0)
    v = (0.439 * r - 0.368 * g - 0.071 * b + 128.0)
    B, H, W = y.shape
    pool = lambda p: p.reshape(B, H // 2, 2, W // 2, 2).mean(dim=(2, 4)).round().clamp(0, 255)  # noqa: E731
    uv = torch.stack([pool(u), pool(v)], dim=-1).reshape(B, H // 2, W)
    return torch.cat([y, uv], dim=1).to(torch.uint8).contiguous()


def pipeline_ms(pipe, frame, n):
    """ms per frame of a FramePipeline over n frames, host clock around the loop."""
    import torch
    for _ in range(3):  # fill the slots once: afterwards the "decoder" finds its frame already in pinned memory (zero-copy ingest)
        pipe.next_input()[...] = frame
        pipe.commit()
    for _ in range(3):
        pipe.result()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        pipe.next_input()
        pipe.commit()
        if pipe.ready() >= 3:
            pipe.result()
    while pipe.ready():
        pipe.result()
    return (time.perf_counter() - t0) / n * 1e3
