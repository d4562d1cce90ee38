"""Device buffers of the limit tests (a plain module; tests/test_gpu_limits.py and tests/test_gpu_limits_entries.py share it): holders filled
with a canary on the device, strided views of them, the check that nothing but a view was written, and the comparison helpers.  The shapes
themselves live in tests/limits_cases.py."""
import numpy as np
import torch

from tests import limits_cases as lc
from tests import pixels as px

_BYTE_PATTERN = int(np.array([lc.U8_CANARY] * 4, np.uint8).view(np.int32)[0])


# ---- buffers -------------------------------------------------------------------------------------------------------------------------------
def byte_holder(nbytes):
    """A device buffer of at least `nbytes` bytes, every byte the canary."""
    return torch.full((-(-nbytes // 16) * 16,), lc.U8_CANARY, dtype=torch.uint8, device="cuda")


def nan_holder(nbytes):
    """The same for float32 sources: every element a NaN, so a tap read outside the rows that were copied in poisons its pixel."""
    return torch.full((-(-nbytes // 16) * 4,), lc.F32_CANARY_BITS, dtype=torch.int32, device="cuda").view(torch.uint8)


def strided(holder, dtype, shape, strides_bytes, offset=0):
    """A view of `holder` with the given shape and strides in bytes, starting `offset` bytes into it."""
    tdt = torch.from_numpy(np.zeros(0, dtype)).dtype if not isinstance(dtype, torch.dtype) else dtype
    esz = torch.empty(0, dtype=tdt).element_size()
    assert offset % esz == 0 and all(s % esz == 0 for s in strides_bytes) and offset + lc.extent_bytes(shape, strides_bytes, esz) <= holder.numel()
    return torch.as_strided(holder.view(tdt), tuple(shape), tuple(s // esz for s in strides_bytes), offset // esz)


def assert_only_the_view_was_written(holder, view, what):
    """Everything outside `view` (one view, or several) still is the canary: the views' own bytes are set back to it, then the whole buffer
    is compared on the device, a chunk at a time (the comparison's mask is the only temporary)."""
    for v in view if isinstance(view, (tuple, list)) else (view,):
        v.view(torch.uint8).fill_(lc.U8_CANARY)
    words = holder.view(torch.int32)
    step = 1 << 28
    flags = torch.stack([(words[i:i + step] != _BYTE_PATTERN).any() for i in range(0, words.numel(), step)])
    assert not bool(flags.any().item()), "%s: bytes outside the destination view were written" % what


# ---- expected values -----------------------------------------------------------------------------------------------------------------------
def per_frame(fn, src, Minv):
    """fn(frame, matrix) for a single image, or stacked over a batch with one matrix per frame."""
    if src.ndim == 3:
        return fn(src, Minv)
    return np.stack([fn(f, M) for f, M in zip(src, Minv)])


def same(got, exp):
    if exp.dtype == np.float32:
        px.same_float(got, exp)
    else:
        np.testing.assert_array_equal(got, exp)
