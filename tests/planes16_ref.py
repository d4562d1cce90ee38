"""The expected value of the 16-bit planes (bevwarp_warp_planes, warp_to_planar(out_dtype=...)) -- TEST INFRASTRUCTURE ONLY, a plain module
like tests/parity.py.

    planes_f32        the float32 planes as the planar tests build them from oracle.cpu_oracle.warp_perspective
    f16_bits          float32 -> the 16 bits of IEEE binary16, round to nearest even (numpy's conversion)
    bf16_bits         float32 -> the upper 16 bits, round to nearest even, in integer arithmetic on the bit pattern (numpy has no bfloat16)
    to_bits           either, by torch dtype
    assert_same16     the comparison: NaN on both sides, every other element by its 16 bits
    gpu_bits          a float16 / bfloat16 tensor's bits on the host
    BOUNDARY_BITS     float32 bit patterns at which a conversion can go wrong (both signs of each)

The double rounding -- float32 first, then 16 bits -- is part of the definition: it is what warp_to_planar(...).half() gives."""
import numpy as np

_POSITIVE = [
    0x00000000,                                      # 0 (and -0 below)
    0x3f7ff000, 0x3f7fefff, 0x3f7ff001,              # 1 - 2^-12: the float16 tie below 1.0 (up to even, 1.0), and its float32 neighbours
    0x3f801000, 0x3f800fff, 0x3f801001,              # 1 + 2^-11: the tie above 1.0 (down to even, 1.0), and its neighbours
    0x3f803000, 0x3f802fff, 0x3f803001,              # 1 + 3 * 2^-11: a tie that goes up to even
    0x3f800000,
    0x477fe000,                                      # 65504, the largest float16
    0x477fefff,                                      # 65519.996..., the last value that rounds to it
    0x477ff000,                                      # 65520, the first that rounds to inf
    0x47800000, 0x4f000000,                          # 65536, 2^31
    0x33800000,                                      # 2^-24, the smallest float16 subnormal
    0x33000000, 0x33000001, 0x32ffffff,              # 2^-25: the tie that goes to 0, its successor (2^-24) and its predecessor (0)
    0x337fffff, 0x33c00000, 0x33c00001,              # below 2^-24; 1.5 * 2^-24: a tie up to even (2^-23); its successor
    0x387fc000,                                      # 1023 * 2^-24, the largest float16 subnormal
    0x387fe000, 0x387fdfff, 0x387fe001,              # halfway to the smallest normal, 2^-14 (tie: up to even), and its neighbours
    0x38800000,                                      # 2^-14
    0x3f808000, 0x3f807fff, 0x3f808001,              # bfloat16 tie down to even (0x3f80), and its neighbours
    0x3f818000, 0x3f817fff, 0x3f818001,              # bfloat16 tie up to even (0x3f82)
    0x7f7fffff, 0x7f7f8000, 0x7f7f7fff,              # FLT_MAX carries to inf in bfloat16; the tie below it does too; its predecessor does not
    0x00000001, 0x007fffff, 0x00400000, 0x00008000, 0x00018000, 0x00007fff, 0x00008001, 0x007f8000,  # float32 subnormals (bfloat16 keeps them)
    0x00800000,                                      # FLT_MIN
    0x7f800000,                                      # inf
    0x7fc00000, 0x7fc00001, 0x7fa00123, 0x7f800001, 0x7fffffff,  # NaNs: quiet, signalling, one whose payload lies below bfloat16's 16 bits
]
BOUNDARY_BITS = np.array(_POSITIVE + [v | 0x80000000 for v in _POSITIVE], dtype=np.uint32)
NAMES = {"float16": "float16", "bfloat16": "bfloat16"}


def _f32(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32, a.dtype
    return a


def f16_bits(a):
    with np.errstate(all="ignore"):
        return _f32(a).astype(np.float16).view(np.uint16)


def bf16_bits(a):
    a = _f32(a)
    u = a.view(np.uint32).astype(np.uint64)
    out = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    out[np.isnan(a)] = 0x7fc0  # (the sum would carry a NaN of a small payload into inf or beyond)
    return out


def kind_of(dtype):
    """"float16" | "bfloat16" from a torch dtype or its name."""
    name = str(dtype).replace("torch.", "")
    assert name in NAMES, dtype
    return name


def to_bits(a, dtype):
    return f16_bits(a) if kind_of(dtype) == "float16" else bf16_bits(a)


def is_nan16(bits, dtype):
    bits = np.asarray(bits, dtype=np.uint16)
    if kind_of(dtype) == "float16":
        return ((bits & 0x7c00) == 0x7c00) & ((bits & 0x03ff) != 0)
    return ((bits & 0x7f80) == 0x7f80) & ((bits & 0x007f) != 0)


def assert_same16(got, exp, dtype, what=""):
    """uint16 arrays of float16 / bfloat16 bit patterns: the NaN masks are equal and every other element has the same 16 bits."""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.dtype == np.uint16 and exp.dtype == np.uint16, (got.dtype, exp.dtype)
    assert got.shape == exp.shape, (got.shape, exp.shape)
    gn, en = is_nan16(got, dtype), is_nan16(exp, dtype)
    bad = (gn != en) | (~en & (got != exp))
    if bad.any():
        idx = tuple(int(v[0]) for v in np.nonzero(bad))
        raise AssertionError("%s%d of %d %s elements differ by bits (NaN where the other has none: %d); first at %s: got 0x%04x, expected 0x%04x"
                             % (what and what + ": ", int(bad.sum()), bad.size, kind_of(dtype), int((gn != en).sum()), idx, int(got[idx]), int(exp[idx])))


def gpu_bits(t):
    import torch
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def planes_f32(src, M, dsize, interp, scale, bias, border_value=None):
    """(C, dh, dw) float32: float32(oracle warp) * float32(scale[c]) + float32(bias[c]), multiply then add, each rounded."""
    from oracle import cpu_oracle as co
    dw, dh = dsize
    c = 1 if src.ndim == 2 else src.shape[2]
    kw = {} if border_value is None else {"border_value": border_value}
    ref = co.warp_perspective(src, M, (dw, dh), interp, **kw).reshape(dh, dw, c)
    sc = np.broadcast_to(np.asarray(scale, dtype=np.float64), (c,)).astype(np.float32)[:, None, None]
    bi = np.broadcast_to(np.asarray(bias, dtype=np.float64), (c,)).astype(np.float32)[:, None, None]
    with np.errstate(all="ignore"):
        out = ref.transpose(2, 0, 1).astype(np.float32) * sc + bi
    assert out.dtype == np.float32
    return out
