"""Pixel values and memory layouts that are not neutral -- TEST INFRASTRUCTURE ONLY, a plain module like tests/parity.py.

float_frame            float32 frames over the whole format: both signs, every binade, subnormals, signed zeros, +-Inf, quiet and
                       signalling NaNs, +-FLT_MAX (the frames of tests/workloads.py lie in [0, 1))
zero_block_frame       a "tiny" frame under squares of -0.0 and of +0.0: sums that are -0.0 only if nothing in them started from +0
same_float             the comparison that goes with them: by bit pattern, so -0.0 != +0.0 and a NaN equals only a NaN
padded_source          frames inside one larger allocation whose every other byte holds a fill value that is not the border value
strided                an array in an allocation of its own in which every outer stride is padded by an amount of the caller's choice
canaried_out,          a destination view inside a holder of canary bytes, and the check that the bytes around the view are intact
assert_canaries_intact

The guard bands lie inside the test's own allocation on all four sides of every frame and are wider than any window a kernel
fetches: a kernel that reads or writes beside its view is caught by value, never by a fault."""
import functools

import numpy as np

SPECIALS = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00001, 0x7fa00123,  # (0x7fa00123: signalling)
                     0x7f7fffff, 0xff7fffff, 0x00000001, 0x80000001, 0x00800000, 0x007fffff], dtype=np.uint32)
FLT_MAX = np.float32(3.4028234663852886e38)
KINDS = ("mixed", "tiny", "huge")
U8_FILL = 0xA5          # the padding of 8-bit sources (the default border value is 0)
CANARY = 0xC3           # every byte of a destination's holder outside the view (the canvas is 77)
_EXPONENTS = {"mixed": (-148.0, 127.0), "tiny": (-149.0, -118.0), "huge": (100.0, 127.99)}


def float_frame(kind, seed, h, w, c):
    """(h, w, c) float32.  Every element is sign * m * 2 ** floor(e), m ~ U[1, 2), rounded to float32 (values below 2 ** -126 land on
    subnormals), with e ~ U[-148, 127) for "mixed", U[-149, -118) for "tiny" (blends land in and around the subnormal range) and
    U[100, 127.99) for "huge" (sums of opposite signs next to FLT_MAX; a convex blend in the oracle's order cannot overflow, see
    tests/test_oracle_pixels.py).  Then "mixed" overwrites 4 % of the elements with a uniform pick of
    SPECIALS, "tiny" turns 20 % into +-0 and "huge" 1 % into +-FLT_MAX."""
    lo, hi = _EXPONENTS[kind]
    rng = np.random.default_rng(seed)
    shape = (h, w, c)
    sign = np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    m = rng.uniform(1.0, 2.0, shape)
    e = np.floor(rng.uniform(lo, hi, shape))
    with np.errstate(over="ignore"):
        out = (sign * m * np.exp2(e)).astype(np.float32)
    if kind == "mixed":
        pick = rng.random(shape) < 0.04
        out.view(np.uint32)[pick] = SPECIALS[rng.integers(0, len(SPECIALS), int(pick.sum()))]
    elif kind == "tiny":
        pick = rng.random(shape) < 0.20
        out.view(np.uint32)[pick] = np.where(rng.random(int(pick.sum())) < 0.5, 0x80000000, 0).astype(np.uint32)
    else:
        pick = rng.random(shape) < 0.01
        out[pick] = np.where(rng.random(int(pick.sum())) < 0.5, -FLT_MAX, FLT_MAX)
    return out


def zero_block_frame(seed, h, w, c, block=8):
    """(h, w, c) float32: float_frame("tiny", seed, h, w, c) -- a call of its own, the streams of the three kinds are untouched -- with
    block x block squares of signed zeros laid over it, one per cell of a lattice of pitch block + block // 2 that starts at the frame's
    corner (squares are cut at the far edges); three squares of every four are -0.0, the one whose lattice row and column are both odd
    is +0.0.  A bilinear blend whose four taps lie in one square is a sum of signed zeros: -0.0 only if every term is, in any order --
    so a result that starts from +0 (an accumulator, a masked-out tap, a flushed product) shows as +0.0 under same_float, and under
    nothing that compares values."""
    assert block >= 8
    out = float_frame("tiny", seed, h, w, c)
    pitch = block + block // 2
    yy, xx = np.indices((h, w))
    inside = (yy % pitch < block) & (xx % pitch < block)
    plus = ((yy // pitch) % 2 == 1) & ((xx // pitch) % 2 == 1)
    b = out.view(np.uint32)
    b[inside & ~plus] = 0x80000000
    b[inside & plus] = 0
    return out


BORDER = [0.3, -2.5, 7.0, 1e-40]  # a finite non-zero border value per channel (the last one is subnormal in float32)
HORIZON = np.array([[1.0, 0.2, 3.0], [0.1, 1.0, 2.0], [0.0, 0.02, -0.5]])  # W changes sign inside the destination


def tiny_source_H(sw, sh):
    return np.array([[200.0 / max(sw, 2), 3.0, 20.0], [1.0, 12.0 / max(sh, 2), 4.0], [0, 0, 1.0]])


@functools.lru_cache(maxsize=None)
def geometries():
    """name -> (src w, src h, dst w, dst h, forward matrix, channel counts).  In warp_rows: keystone -- FAST rows, row-affine tiles;
    brno -- edge, outside and patch tiles, ragged; rotated -- the patch layout; short -- fewer than 16 rows; horizon -- SLOW rows, the
    guarded sampler; src2x2, src5x1 -- sources smaller than the load window."""
    from tests import workloads as wl
    return {
        "keystone": (640, 360, 512, 80, wl.keystone_H(640, 360, 512, 80), (1, 2, 3, 4)),
        "brno": (640, 360, 300, 37, wl.synth_brno_H(640, 360, 300, 37), (1, 2, 3, 4)),
        "rotated": (640, 360, 300, 77, wl.rotated_H(640, 360, 300, 77, 30.0, 2.4), (3,)),
        "short": (100, 60, 300, 9, wl.keystone_H(100, 60, 300, 9), (3,)),
        "horizon": (96, 64, 128, 96, HORIZON, (3,)),
        "src2x2": (2, 2, 256, 32, tiny_source_H(2, 2), (3,)),
        "src5x1": (5, 1, 256, 32, tiny_source_H(5, 1), (3,)),
    }


def float_cases():
    """[(id, geometry name, kind, interp, c, border value or None)]: kinds x interpolations x the channel counts of each geometry;
    half of them with a finite non-zero border value."""
    out = []
    for name, g in geometries().items():
        for kind in KINDS:
            for interp in (0, 1):
                for c in g[5]:
                    out.append(("%s-%s-%s-c%d" % (name, kind, ("nearest", "linear")[interp], c), name, kind, interp, c, BORDER[:c] if (KINDS.index(kind) + interp + c) % 2 else None))
    return out


_SEED_BASE = {"brno": 0, "horizon": 1000, "keystone": 2000, "rotated": 3000, "short": 4000, "src2x2": 5000, "src5x1": 6000}  # fixed: a new geometry gets a new base, the others keep theirs


def case_seed(name, kind, c):
    return _SEED_BASE[name] + 10 * KINDS.index(kind) + c


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def is_subnormal(a):
    b = bits(a)
    return ((b & 0x7f800000) == 0) & ((b & 0x007fffff) != 0)


def same_float(got, exp, payload=False):
    """float32 arrays equal by bit pattern: the NaN masks are equal, and wherever `exp` is not NaN the 32 bits are (so -0.0 is not
    +0.0 and a subnormal is not 0).  payload=True: the bits are equal everywhere, NaN payloads and signs included."""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.dtype == np.float32 and exp.dtype == np.float32, (got.dtype, exp.dtype)
    assert got.shape == exp.shape, (got.shape, exp.shape)
    gb, eb = bits(got), bits(exp)
    gn, en = np.isnan(got), np.isnan(exp)
    bad = (gb != eb) if payload else ((gn != en) | (~en & (gb != eb)))
    if bad.any():
        idx = tuple(int(v[0]) for v in np.nonzero(bad))
        raise AssertionError("%d of %d float32 elements differ by bits%s (NaN where the other has none: %d); first at %s: got 0x%08x (%r), expected 0x%08x (%r)"
                             % (int(bad.sum()), bad.size, " (payloads compared)" if payload else "", int((gn != en).sum()), idx,
                                int(gb[idx]), float(got[idx]), int(eb[idx]), float(exp[idx])))


def _filled(n, torch_dtype, byte_or_value, device="cuda"):
    import torch
    return torch.full((n,), byte_or_value, dtype=torch_dtype, device=device)


def padded_source(frames_np, fill, offset=0, pad_rows=2, device="cuda"):
    """A CUDA view holding `frames_np` ((H, W, C) or (B, H, W, C), uint8 or float32) inside one larger allocation: `pad_rows` whole padded
    rows above and below every frame (so a batch's frame stride is larger than H * row stride), at least 64 bytes left and right of
    every row, and every element outside the frames equal to `fill`.  `offset` (elements, 0 .. 16 for uint8, 0 .. 4 for float32)
    shifts the view inside its rows: base addresses of every residue mod 4 (uint8) / of 0, 4, 8, 12 mod 16 (float32).  The row
    stride is W * C elements plus a multiple of 16 bytes, so it keeps the residue of W * C."""
    import torch
    f = np.ascontiguousarray(frames_np)
    f4 = f if f.ndim == 4 else f[None]
    B, H, W, C = f4.shape
    esz = f.dtype.itemsize
    side, slack = 64 // esz, 16 // esz
    assert 0 <= offset <= slack
    rs = W * C + 2 * side + slack
    fs = (H + 2 * pad_rows) * rs
    buf = _filled(B * fs, torch.from_numpy(f).dtype, fill, device)
    view = torch.as_strided(buf, (B, H, W, C), (fs, rs, C, 1), pad_rows * rs + side + offset)
    view.copy_(torch.from_numpy(f4).to(device))
    return view if f.ndim == 4 else view[0]


def strided(a_np, pads, fill=U8_FILL, device="cuda"):
    """A CUDA view holding `a_np` in one allocation of its own (every other element is `fill`) in which the stride of dimension k, for
    k < len(pads), is pads[k] elements more than the dimensions inside it need; the remaining dimensions are contiguous.  A caller that
    gives every image of a call pads of its own gets row, plane and frame strides that all differ from the tight ones and from each other:
    an entry point that swaps or drops one of them then reads or writes the wrong elements, and the comparison shows it."""
    import torch
    a = np.ascontiguousarray(a_np)
    strides = [1] * a.ndim
    for k in reversed(range(a.ndim - 1)):
        strides[k] = a.shape[k + 1] * strides[k + 1] + (pads[k] if k < len(pads) else 0)
    buf = _filled(a.shape[0] * strides[0], torch.from_numpy(a).dtype, fill, device)
    view = torch.as_strided(buf, a.shape, strides)
    view.copy_(torch.from_numpy(a).to(device))
    return view


def canaried_out(shape, dtype, pad, canvas=77, align=16, planar=False, gap_rows=2, device="cuda"):
    """(view, holder): a destination of `shape` filled with `canvas` inside a 1-D holder whose every other byte is CANARY.  Interleaved
    ((dh, dw, c) / (B, dh, dw, c)) or, with planar=True, planes ((C, dh, dw) / (B, C, dh, dw)); rows are at least `pad` bytes apart,
    frames (and planes) `gap_rows` padded rows, and two rows and 64 bytes lie before and after everything.
    align > 0: the base, the row stride and every outer stride are multiples of `align` bytes (the row padding grows to the next one):
               the layout keeps what the wide stores need.
    align = 0: the row stride is no multiple of 4 bytes (uint8) / 16 bytes (float32) and the base is one element off: it loses it."""
    import torch
    tdt = dtype if isinstance(dtype, torch.dtype) else torch.from_numpy(np.zeros(0, dtype)).dtype
    esz = torch.empty(0, dtype=tdt).element_size()
    shape = tuple(int(v) for v in shape)
    n_inner = 1 if planar else 2
    row = int(np.prod(shape[-n_inner:]))
    rows, outer = shape[-n_inner - 1], shape[:-n_inner - 1]
    rs = row + (pad + esz - 1) // esz
    if align:
        assert align % esz == 0
        rs = -(-rs * esz // align) * align // esz
        lead = -(-(2 * rs * esz + 64) // align) * align // esz
    else:
        while (rs * esz) % (4 if esz == 1 else 16) == 0:
            rs += 1
        lead = 2 * rs + 64 // esz + 1
        if (lead * esz) % (4 if esz == 1 else 16) == 0:
            lead += 1
    strides, span = [], (rows + gap_rows) * rs  # (span: elements from one image of this level to the next)
    for n in reversed(outer):
        strides.insert(0, span)
        span = n * span + gap_rows * rs
    inner = [1] if planar else [shape[-1], 1]
    strides = strides + [rs] + inner
    extent = sum((n - 1) * s for n, s in zip(shape, strides)) + 1
    holder = _filled((lead + extent + 2 * rs) * esz + 64, torch.uint8, CANARY, device)
    holder = holder[:holder.numel() // esz * esz].view(tdt)
    view = torch.as_strided(holder, shape, strides, lead)
    view.fill_(canvas)
    if align:
        assert view.data_ptr() % align == 0 and all((s * esz) % align == 0 for s in strides[:-n_inner])
    return view, holder


def assert_canaries_intact(holder, view, what=""):
    """Every byte of `holder` outside `view` still is CANARY (one comparison on the host)."""
    esz = holder.element_size()
    assert view.data_ptr() >= holder.data_ptr() and (view.data_ptr() - holder.data_ptr()) % esz == 0
    off = np.full((), (view.data_ptr() - holder.data_ptr()) // esz, dtype=np.int64)
    for n, s in zip(view.shape, view.stride()):
        off = off[..., None] + np.arange(n, dtype=np.int64) * s
    inside = np.zeros(holder.numel(), bool)
    inside[off.ravel()] = True
    import torch
    host = holder.view(-1).view(torch.uint8).cpu().numpy()  # (as bytes on the device: numpy has no bfloat16)
    bad = (host != CANARY) & ~np.repeat(inside, esz)
    if bad.any():
        first = int(np.flatnonzero(bad)[0])
        rel = first - (view.data_ptr() - holder.data_ptr())
        raise AssertionError("%s%d bytes outside the destination view were written; first at byte %d from the view's base (shape %s, strides in bytes %s), now 0x%02x"
                             % (what and what + ": ", int(bad.sum()), rel, tuple(view.shape), tuple(s * esz for s in view.stride()), int(host[first])))
