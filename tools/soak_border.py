#!/usr/bin/env python3
"""Bounded random soak of the border modes: seeded cases over mode (the five of bevwarp_warp_border), dtype, interpolation, channel
count, source and destination sizes, batch (shared or per-frame matrices, WARP_INVERSE_MAP) and random homographies -- rotation,
0.2 .. 4 x scale, perspective, shifts that push the window partly or wholly out of the frame -- each frame compared bit for bit
with the numpy reference tests/border_ref.py.  Exit status 1 on any mismatch.
GPU box:  python tools/soak_border.py [--cases 300] [--seed 0]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bev_amd import warp  # noqa: E402
from tests import border_ref as BR  # noqa: E402

MODES = (BR.REPLICATE, BR.REFLECT, BR.WRAP, BR.REFLECT_101, BR.TRANSPARENT)


def random_H(rng, sw, sh, dw, dh):
    """src -> dst map of a random window of the source (possibly far outside it)."""
    ang = rng.uniform(-np.pi, np.pi)
    zoom = float(np.exp(rng.uniform(np.log(0.2), np.log(4.0))))
    c, s = np.cos(ang) * zoom, np.sin(ang) * zoom
    A = np.array([[c, -s, 0.0], [s, c, 0.0], [rng.uniform(-3e-3, 3e-3), rng.uniform(-3e-3, 3e-3), 1.0]])
    T0 = np.array([[1, 0, -(dw - 1) / 2.0], [0, 1, -(dh - 1) / 2.0], [0, 0, 1.0]])
    T1 = np.array([[1, 0, (sw - 1) / 2.0 + rng.uniform(-1.5, 1.5) * sw], [0, 1, (sh - 1) / 2.0 + rng.uniform(-1.5, 1.5) * sh], [0, 0, 1.0]])
    return np.linalg.inv(T1 @ A @ T0)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--cases", type=int, default=300)
    p.add_argument("--seed", type=int, default=0)
    a = p.parse_args()
    rng = np.random.default_rng(a.seed)
    dev = torch.device("cuda", 0)
    bad, frames, t0 = 0, 0, time.time()
    counts = {}
    for case in range(a.cases):
        mode = int(rng.choice(MODES))
        dtype = np.uint8 if rng.random() < 0.5 else np.float32
        interp = int(rng.integers(0, 2))
        C = int(rng.integers(1, 5))
        sw, sh = (int(v) for v in (rng.integers(1, 300, 2) if rng.random() < 0.8 else rng.integers(1, 5, 2)))
        dw, dh = (int(v) for v in rng.integers(1, 200, 2))
        B = int(rng.integers(1, 4))
        per_frame = B > 1 and rng.random() < 0.5
        inverse = rng.random() < 0.2
        Ms = np.stack([random_H(rng, sw, sh, dw, dh) for _ in range(B if per_frame else 1)])
        if inverse:
            Ms = np.stack([BR.invert3x3(m) for m in Ms])
        src = (rng.integers(0, 256, (B, sh, sw, C), dtype=np.uint8) if dtype == np.uint8 else rng.random((B, sh, sw, C), dtype=np.float32))
        canvas = np.full((B, dh, dw, C), 77, dtype=dtype)
        out = torch.from_numpy(canvas).to(dev)
        flags = interp | (warp.WARP_INVERSE_MAP if inverse else 0)
        warp.warp_perspective(torch.from_numpy(src).to(dev), Ms if per_frame else Ms[0], (dw, dh), flags=flags, out=out, border_mode=mode)
        got = out.cpu().numpy()
        for i in range(B):
            exp = BR.warp(src[i], Ms[i if per_frame else 0], (dw, dh), interp, mode, m_is_inverse=inverse, canvas=canvas[i])
            frames += 1
            if not np.array_equal(got[i], exp):
                bad += 1
                n = int((got[i] != exp).any(axis=-1).sum())
                print("MISMATCH case %d frame %d: %s %s interp %d C %d src %dx%d dst %dx%d B %d per_frame %s inverse %s: %d px"
                      % (case, i, BR.NAMES[mode], np.dtype(dtype).name, interp, C, sw, sh, dw, dh, B, per_frame, inverse, n), flush=True)
        counts[BR.NAMES[mode]] = counts.get(BR.NAMES[mode], 0) + 1
    print("soak_border: %d cases, %d frames, %d mismatching frames (seed %d; cases per mode %s), %.0f s"
          % (a.cases, frames, bad, a.seed, counts, time.time() - t0), flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
