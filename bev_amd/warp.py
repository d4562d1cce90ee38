"""Device warp: the HIP replacement for `cv2.warpPerspective(img, H_bev_img, (u_size, v_size))`
(reference call sites vis_homo.py:89, :91; bev/tool/compo.py:38, :46, :47).

    dst = warp_perspective(src, M, (u_size, v_size))            # torch tensors on the GPU, batched
    dst = warpPerspective(img, M, (u_size, v_size))             # numpy in / numpy out, cv2 call shape

M is the FORWARD map (src px -> dst px) exactly as callers hand it to OpenCV; it is inverted on the
host with OpenCV's closed form and the inverse is cached on the device (calibrations are static per
camera).  All pixel work happens in bev_amd/csrc (HIP, gfx950) through the C ABI; nothing here
falls back to the CPU.
"""
import collections
import ctypes
import math

import numpy as np
import torch

from . import _lib
from . import exposure as _exposure

INTER_NEAREST = _lib.INTER_NEAREST
INTER_LINEAR = _lib.INTER_LINEAR
INTER_CUBIC = _lib.INTER_CUBIC  # bevwarp_warp_border's bicubic kernel, every border mode (BORDER_CONSTANT included)
WARP_INVERSE_MAP = 16  # cv2 flag value
# cv2 border modes (cv::BorderTypes values); BORDER_CONSTANT is the warp kernel's own, the others are bevwarp_warp_border
BORDER_CONSTANT = 0
BORDER_REPLICATE = 1
BORDER_REFLECT = 2
BORDER_WRAP = 3
BORDER_REFLECT_101 = 4
BORDER_REFLECT101 = BORDER_REFLECT_101
BORDER_DEFAULT = BORDER_REFLECT_101
BORDER_TRANSPARENT = 5
_BORDER_MODES = (BORDER_CONSTANT, BORDER_REPLICATE, BORDER_REFLECT, BORDER_WRAP, BORDER_REFLECT_101, BORDER_TRANSPARENT)

_DTYPES = {torch.uint8: _lib.U8, torch.float32: _lib.F32}
_PLANE_DTYPES = {torch.float32: _lib.F32, torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}  # what warp_to_planar writes


def invert_homography(M):
    """Host float64 inverse(s) of 3x3 matrices, OpenCV evaluation order.  (..., 3, 3) -> same shape."""
    M = np.ascontiguousarray(M, dtype=np.float64)
    assert M.shape[-2:] == (3, 3), M.shape
    out = np.empty_like(M)
    _lib.check(_lib.load().bevwarp_invert_homography(M.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p),
                                                     int(M.size // 9)))
    return out


_MINV_CACHE_MAX = 256
_MINV_PINNED_MAX = 4096
_minv_cache = collections.OrderedDict()  # (matrix bytes, device, inverse_given) -> device tensor, least recently used first
_minv_pinned = {}                        # entries whose address a hipGraph capture has seen: never evicted
_minv_retired = []                       # pinned entries written in place since: no longer looked up, still never freed


def device_inverse(M, device, inverse_given=False):
    """(n, 3, 3) float64 device tensor of inverse matrices for forward matrices M (cached by value).

    Lifetime rules (launches only ever receive the tensor's raw address): every use records the current stream on the
    tensor, so an evicted entry's memory is not handed out again before the launches that read it have run; an entry
    that is looked up while the current stream is being captured into a graph is pinned for the life of the process
    (the graph replays its address; 72 bytes per matrix, at most _MINV_PINNED_MAX entries -- re-capturing with ever new
    matrices beyond that raises: pass `M_inv_device`), and a cache MISS during capture raises -- upload the matrices before capturing
    (or pass `M_inv_device`, which the caller owns).

    The returned tensor is the cache entry itself.  Writing into it with an in-place torch op (`copy_`, `mul_`, ...) bumps its
    `_version`: the entry no longer holds the inverse of its key, so a later lookup drops it and uploads the key's matrices anew,
    and the verdict tables of the written tensor are refilled (_tile_classes).  Writes through its raw address are not seen: as for
    any matrix tensor whose verdicts are cached, keeping them away is the caller's job (include/bevwarp.h, bevwarp_warp_classes)."""
    if isinstance(M, torch.Tensor) and M.is_cuda and inverse_given:
        return M.to(torch.float64).reshape(-1, 3, 3).contiguous()
    device = torch.device(device)
    Mh = np.ascontiguousarray(M.detach().cpu().numpy() if isinstance(M, torch.Tensor) else M, dtype=np.float64).reshape(-1, 3, 3)
    key = (Mh.tobytes(), str(device), bool(inverse_given))
    capturing = False
    if device.type == "cuda" and torch.cuda.is_available():
        with torch.cuda.device(device):  # the capture state of THIS device's current stream, not of the default device's
            capturing = torch.cuda.is_current_stream_capturing()
    hit = _minv_pinned.get(key)
    if hit is not None:
        if hit._version == hit._bevwarp_version:
            return hit
        _minv_retired.append(_minv_pinned.pop(key))  # (written in place: a captured graph may still replay its address)
    hit = _minv_cache.get(key)
    if hit is not None and hit._version != hit._bevwarp_version:
        del _minv_cache[key]  # written in place: no longer the inverse of its key (every use recorded its stream, see below)
        hit = None
    if hit is None:
        if capturing:
            raise RuntimeError("device_inverse: homography not resident while a graph is being captured; call the step once "
                               "before capturing, or pass M_inv_device")
        inv = Mh if inverse_given else invert_homography(Mh)
        hit = torch.from_numpy(inv).to(device)
        hit._bevwarp_owned = True  # (cached by value: its tile verdicts may be cached too, _tile_classes)
        hit._bevwarp_version = hit._version
        _minv_cache[key] = hit
        while len(_minv_cache) > _MINV_CACHE_MAX:
            _minv_cache.popitem(last=False)  # (safe: every use recorded its stream, see below)
    else:
        _minv_cache.move_to_end(key)
    if capturing:
        if len(_minv_pinned) + len(_minv_retired) >= _MINV_PINNED_MAX:
            raise RuntimeError("device_inverse: %d homography sets are already pinned by graph captures; pass M_inv_device (a tensor the "
                               "caller owns) when capturing graphs with ever new matrices" % _MINV_PINNED_MAX)
        _minv_pinned[key] = _minv_cache.pop(key)
    elif hit.is_cuda:
        hit.record_stream(torch.cuda.current_stream(hit.device))
    return hit


try:  # the current stream's raw hipStream_t without building a torch.cuda.Stream object (~0.2 us instead of ~1.5)
    _raw_stream = torch._C._cuda_getCurrentRawStream
except AttributeError:  # pragma: no cover - older / CPU-only builds
    def _raw_stream(dev_index):
        return torch.cuda.current_stream(dev_index).cuda_stream

try:  # the current stream's capture state (torch.cuda.is_current_stream_capturing without its Python frame)
    _capturing = torch._C._cuda_isCurrentStreamCapturing
except AttributeError:  # pragma: no cover - older / CPU-only builds
    _capturing = torch.cuda.is_current_stream_capturing

_PLANS_MAX = 1024
_plans = {}  # validated launches by (addresses, shapes, strides, dtypes, dsize, flags) -> (entry point, bound arguments, device index)


def _check_minv(M_inv_device, device, B):
    """A caller-supplied matrix tensor goes to the kernel as a raw address: it must be exactly what the ABI reads."""
    t = M_inv_device
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or not t.is_contiguous() or t.device != device:
        raise ValueError("M_inv_device must be a contiguous float64 tensor on %s" % (device,))
    if t.dim() < 2 or tuple(t.shape[-2:]) != (3, 3) or t.numel() % 9:
        raise ValueError("M_inv_device must be (n, 3, 3), got %s" % (tuple(t.shape),))
    n_m = t.numel() // 9
    if n_m not in (1, B):
        raise ValueError("got %d homographies for a batch of %d" % (n_m, B))
    return n_m


def _check_out(out, dtype, device, numel):
    """A caller-supplied destination is written through its raw address with the SOURCE's element size."""
    if not isinstance(out, torch.Tensor) or out.dtype != dtype or out.device != device or out.numel() != numel:
        raise ValueError("out must be a %s tensor of %d elements on %s" % (dtype, numel, device))


def _per_channel(v, C):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (C,)))


def _border(border_value, C):
    return None if border_value is None else _per_channel(border_value, C)


def _ptr(a):
    """A host array (or None) as the ABI takes it."""
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


# What the launching entry points below share.  An entry point is its own checks, then these calls in this order, then _lib.launch
# (the validated-launch fast path of warp_perspective goes through none of them).


def _interp(who, flags, cubic=False):
    """The interpolation bits of `flags`, once they name a kernel `who` has (who: the caller as its message names it)."""
    interp = int(flags) & 7
    if interp not in ((INTER_NEAREST, INTER_LINEAR, INTER_CUBIC) if cubic else (INTER_NEAREST, INTER_LINEAR)):
        raise ValueError("unsupported interpolation flag %d (%sINTER_NEAREST, INTER_LINEAR%s)" % (interp, who and who + ": ", ", INTER_CUBIC" if cubic else ""))
    return interp


def _frames(who, src, dtypes, channels=None):
    """Interleaved frames as the ABI reads them: (s4, copied) -- `src` as (B, H, W, C) with channels-last rows, a contiguous copy
    (copied) where its rows are not.  dtypes: the element types `who` takes, None when the caller has judged the tensor with a message
    of its own; channels: the one channel count taken, and then no (H, W) frames."""
    if dtypes is not None and (not isinstance(src, torch.Tensor) or not src.is_cuda or src.dtype not in dtypes):
        raise ValueError("%s needs a %s CUDA (HIP) tensor" % (who, " or ".join(str(t)[6:] for t in dtypes)))
    if channels is not None and (src.dim() not in (3, 4) or src.shape[-1] != channels):
        raise ValueError("src must be (B, H, W, %d) or (H, W, %d)" % (channels, channels))
    if src.dim() == 2:
        s4 = src[None, :, :, None]
    elif src.dim() == 3:
        s4 = src[None]
    elif src.dim() == 4:
        s4 = src
    else:
        raise ValueError("src must be (B,H,W,C), (H,W,C) or (H,W)")
    copied = s4.stride(3) != 1 or s4.stride(2) != s4.shape[3]
    return (s4.contiguous() if copied else s4), copied


def _matrices(M, flags, M_inv_device, device, B):
    """(matrix tensor, number of matrices) of a call on B frames: the caller's `M_inv_device`, or the cached inverses of `M`."""
    if M_inv_device is None:
        M_inv_device = device_inverse(M, device, inverse_given=bool(int(flags) & WARP_INVERSE_MAP))
    return M_inv_device, _check_minv(M_inv_device, device, B)


def _pixel_dst(out, dtype, device, B, dh, dw, C, zeroed=False):
    """The (B, dh, dw, C) destination of a call that writes interleaved pixels: a new tensor, or the caller's `out` as it is."""
    if out is None:
        return (torch.zeros if zeroed else torch.empty)((B, dh, dw, C), dtype=dtype, device=device)
    _check_out(out, dtype, device, B * dh * dw * C)
    d4 = out.reshape(B, dh, dw, C)
    if d4.data_ptr() != out.data_ptr() or d4.stride(3) != 1 or d4.stride(2) != C:
        raise ValueError("out must be a contiguous-row channels-last tensor")
    return d4


def _like_src(d4, ndim, out):
    """What the caller gets back: `out`, or the 4-D result without the batch and channel axes a source of `ndim` dimensions did not have."""
    if out is not None:
        return out
    if ndim == 2:
        return d4[0, :, :, 0]
    return d4[0] if ndim == 3 else d4


_CLASSES_MAX = 64
_class_tables = collections.OrderedDict()  # (matrix tensor address, n matrices, batch, sizes, format) -> (verdict table, the matrix tensor, its _version)


def _tile_classes(M_inv_device, n_m, call_args, stream):
    """The per-tile verdict table (include/bevwarp.h, bevwarp_warp_classes) of a launch whose matrices are owned by device_inverse --
    cached by value, so verdicts derived from them once hold for every later launch with the same geometry: the camera loop of
    vis_homo.py:85-91 warps every frame of a video through one H_bev_img.  None for matrices the caller owns (their contents may change
    under the same address), while a graph is being captured (the fill would allocate, and a graph would replay the table's address:
    captured launches classify for themselves -- a plan that carries a table launches plain bevwarp_warp under capture too; tables are
    not pinned for graphs), and for launches the library keeps no table for.

    Contents: a table is kept with the matrix tensor's `_version`.  An in-place torch op on the tensor changes it, and the next launch
    refills the table (a plan that carries the table falls back to this path); writes through the raw address are not seen -- the
    caller's to avoid, as include/bevwarp.h says.
    Streams: filled on first use (one launch that writes no pixel), and the filling call then waits on the host until the fill has run
    (a one-time wait per matrices and geometry, the camera loop pays it on its first frame): a launch on any other stream that finds the
    table in the cache or in a plan reads finished verdicts."""
    if not getattr(M_inv_device, "_bevwarp_owned", False):
        return None
    (_, _, B, H, W, dh, dw, C, _, _, _, _, _, _, dtype, interp, _) = call_args
    key = (M_inv_device.data_ptr(), n_m, B, H, W, dh, dw, C, dtype, interp)
    with torch.cuda.device(M_inv_device.device):
        if torch.cuda.is_current_stream_capturing():
            return None
        hit = _class_tables.get(key)
        if hit is not None:
            if hit[2] == M_inv_device._version:
                _class_tables.move_to_end(key)
                return hit[0]
            del _class_tables[key]  # the matrices were written in place since the fill: these verdicts are not theirs
        lib = _lib.load()
        nbytes = lib.bevwarp_tile_classes_bytes(B, H, W, dh, dw, C, dtype, interp)
        if nbytes <= 0:
            return None
        table = torch.zeros(nbytes // 4, dtype=torch.int32, device=M_inv_device.device)
        _lib.check(lib.bevwarp_warp_classes(*call_args, table.data_ptr(), 1, ctypes.c_void_p(stream)))
        torch.cuda.current_stream().synchronize()  # (the stream `stream` is: cached verdicts are finished verdicts)
    _class_tables[key] = (table, M_inv_device, M_inv_device._version)  # (holding the matrix tensor keeps its address from being handed out again)
    while len(_class_tables) > _CLASSES_MAX:
        _class_tables.popitem(last=False)
    return table


def warp_perspective(src, M, dsize, flags=INTER_LINEAR, border_value=None, out=None, M_inv_device=None, border_mode=BORDER_CONSTANT):
    """Batched perspective warp on the GPU.

    src      (B, H, W, C) or (H, W, C) or (H, W) uint8 / float32 CUDA tensor, channels-last, rows contiguous.
    M        (3, 3) shared or (B, 3, 3) per-frame forward homography (numpy or tensor); with
             flags | WARP_INVERSE_MAP it is taken as the dst -> src map instead.
    dsize    (width, height) = (u_size, v_size), as OpenCV.
    flags    INTER_LINEAR (default), INTER_NEAREST or INTER_CUBIC, optionally | WARP_INVERSE_MAP.  INTER_CUBIC is OpenCV's classic
             remapBicubic (restated from memory, parity unpinned; include/bevwarp.h) for every border mode.
    out      optional preallocated result; M_inv_device optional (n, 3, 3) f64 CUDA tensor to skip the cache.
    border_mode  BORDER_CONSTANT (default; `border_value`), BORDER_REPLICATE, BORDER_REFLECT, BORDER_WRAP, BORDER_REFLECT_101
             (every tap reads a source pixel, border_value is ignored) or BORDER_TRANSPARENT: only pixels whose taps are all
             inside the source are written, every other pixel of `out` keeps its contents (warp several cameras into one
             canvas, one call each).  TRANSPARENT without `out` returns a zeroed result where it writes nothing (OpenCV would
             leave those pixels uninitialised).  With INTER_CUBIC, TRANSPARENT writes the pixels whose integer position lies in
             the source.  Semantics: include/bevwarp.h, bevwarp_warp_border.
    Returns a tensor shaped like src with (height, width) replaced.  Asynchronous on the current stream."""
    if out is not None and M_inv_device is not None and border_value is None:
        # Steady-state call of a camera loop: same buffers, same geometry as a call that has already been validated.  The
        # whole Python layer is then one dictionary lookup and the C call with its argument tuple bound (a single 720p -> 512^2
        # frame is a 10-us kernel: the general path below costs more host time than that).
        try:
            # (addresses can be recycled by the allocator: everything the slow path validates is part of the key -- dtypes and
            # devices of all three tensors included, or a float32 / CPU matrix tensor at a recycled address would skip _check_minv)
            key = (src.data_ptr(), out.data_ptr(), M_inv_device.data_ptr(), src.shape, src.stride(), out.shape, out.stride(), M_inv_device.shape,
                   M_inv_device.stride(), src.dtype, out.dtype, M_inv_device.dtype, src.device, out.device, M_inv_device.device, dsize[0], dsize[1], flags,
                   border_mode)  # (a plan serves the border mode it was made for only)
            plan = _plans.get(key)
        except (AttributeError, TypeError, IndexError):
            plan = None
        if plan is not None and plan[3] is not None and M_inv_device._version != plan[5]:
            plan = None  # verdicts of matrices since written in place: the slow path refills them
        if plan is not None:
            # (a plan with a verdict table launches the plain entry point while a graph is being captured: the graph would replay the
            # table's address, and nothing keeps the table alive for the graph's life)
            fn, args, dev_index, table = plan[:4]
            if torch.cuda.current_device() == dev_index:
                if table is not None and _capturing():
                    fn, args = plan[6], args[:-2]
                st = fn(*args, _raw_stream(dev_index))
            else:
                with torch.cuda.device(dev_index):
                    if table is not None and _capturing():
                        fn, args = plan[6], args[:-2]
                    st = fn(*args, _raw_stream(dev_index))
            if st:
                _lib.check(st)
            return out
    else:
        key = None
    if border_mode not in _BORDER_MODES:
        raise ValueError("unsupported border mode %r (BORDER_CONSTANT, _REPLICATE, _REFLECT, _WRAP, _REFLECT_101, _TRANSPARENT)" % (border_mode,))
    border_mode = int(border_mode)
    if not isinstance(src, torch.Tensor) or not src.is_cuda:
        raise ValueError("warp_perspective needs a CUDA (HIP) tensor; use warpPerspective for numpy images")
    if src.dtype not in _DTYPES:
        raise ValueError("unsupported dtype %s (uint8 / float32)" % src.dtype)
    interp = _interp("", flags, True)
    s4, copied = _frames("warp_perspective", src, None)
    B, H, W, C = s4.shape
    dw, dh = int(dsize[0]), int(dsize[1])
    esz = s4.element_size()
    M_inv_device, n_m = _matrices(M, flags, M_inv_device, s4.device, B)
    if out is None:  # (_pixel_dst's first branch, spelt out: this path is timed by tools/host_overhead.py, and the call was the dearest of the helpers')
        d4 = (torch.zeros if border_mode == BORDER_TRANSPARENT else torch.empty)((B, dh, dw, C), dtype=s4.dtype, device=s4.device)
    else:
        d4 = _pixel_dst(out, s4.dtype, s4.device, B, dh, dw, C)
    bv = _border(border_value, C) if border_mode == BORDER_CONSTANT else None  # (only the constant border reads it)
    stream = torch.cuda.current_stream(s4.device).cuda_stream
    args = (s4.data_ptr(), d4.data_ptr(), B, H, W, dh, dw, C, s4.stride(0) * esz, s4.stride(1) * esz, d4.stride(0) * esz, d4.stride(1) * esz,
            M_inv_device.data_ptr(), n_m, _DTYPES[s4.dtype], interp, _ptr(bv))
    if border_mode == BORDER_CONSTANT and interp != INTER_CUBIC:
        fn = plain = _lib.load().bevwarp_warp
        table = _tile_classes(M_inv_device, n_m, args, stream)
        if table is not None:  # verdicts of these very matrices and this geometry: the kernel reads them instead of deriving them
            table.record_stream(torch.cuda.current_stream(s4.device))
            fn, args = _lib.load().bevwarp_warp_classes, args + (table.data_ptr(), 0)
    else:  # the other borders, and bicubic with any border: kernels of their own, which classify no tiles (no verdict table)
        fn = plain = _lib.load().bevwarp_warp_border
        args, table = args[:-1] + (border_mode, args[-1]), None  # (border_value: None unless BORDER_CONSTANT, i.e. bicubic)
    with torch.cuda.device(s4.device):
        st = fn(*args, ctypes.c_void_p(stream))
    _lib.check(st)
    if key is not None and not copied:  # validated and launched: the next call with these very buffers skips the checks
        if len(_plans) >= _PLANS_MAX:
            _plans.clear()
        # (a plan with a verdict table keeps the table AND the matrices it belongs to alive -- their address must not be handed out again
        # while the plan can be hit -- and holds the matrices' _version it was filled for, and the plain entry point for graph captures)
        _plans[key] = (fn, args, s4.device.index if s4.device.index is not None else torch.cuda.current_device(), table,
                       M_inv_device if table is not None else None, M_inv_device._version if table is not None else None, plain)
    return _like_src(d4, src.dim(), out)


_SUPERSAMPLE = {2: _lib.SUPERSAMPLE_2, 4: _lib.SUPERSAMPLE_4, 8: _lib.SUPERSAMPLE_8}  # factor -> the field of the ABI's interp word
_SUPERSAMPLE_BORDERS = (BORDER_CONSTANT, BORDER_REPLICATE, BORDER_REFLECT, BORDER_WRAP, BORDER_REFLECT_101)


def warp_perspective_supersampled(src, M, dsize, supersample=2, flags=INTER_LINEAR, border_value=None, out=None, M_inv_device=None,
                                  border_mode=BORDER_CONSTANT):
    """warp_perspective with `supersample`^2 samples per destination pixel, in one pass: what warping into a BEV `supersample` times as
    large on each side and box-filtering it down is for, where the far half of the view is minified several times over and one sample per
    pixel aliases -- without the large frames in memory (include/bevwarp.h, BEVWARP_SUPERSAMPLE_*).  Each pixel is the average of the
    k x k pixels warp_perspective itself would write at the centres of the k x k fine pixels it covers: 8-bit (sum + k^2 / 2) >> 2 log2 k,
    float32 summed in float32 rows outermost and multiplied by 1 / k^2.  Bit-equal to that two-pass route.

    src, M, dsize, border_value, out, M_inv_device   as warp_perspective.
    supersample   1, 2, 4 or 8; 1 IS warp_perspective(src, M, dsize, ...).  Anything else: ValueError.
    flags    INTER_LINEAR (default) or INTER_NEAREST, optionally | WARP_INVERSE_MAP; INTER_CUBIC: ValueError.
    border_mode   BORDER_CONSTANT (default), BORDER_REPLICATE, BORDER_REFLECT, BORDER_WRAP or BORDER_REFLECT_101; BORDER_TRANSPARENT:
             ValueError (a pixel that is partly written has no average).
    For supersample > 1 an identity M does not return src: every pixel is a small box filter of its neighbourhood (the sub-samples sit
    off the pixel's centre).  The cost is about supersample^2 times warp_perspective's with a source-reading border.  No verdict tables, no
    plan cache.  Asynchronous on the current stream."""
    if isinstance(supersample, bool) or supersample not in (1, 2, 4, 8):
        raise ValueError("warp_perspective_supersampled: supersample must be 1, 2, 4 or 8, got %r" % (supersample,))
    k = int(supersample)
    if k == 1:
        return warp_perspective(src, M, dsize, flags=flags, border_value=border_value, out=out, M_inv_device=M_inv_device, border_mode=border_mode)
    if border_mode not in _SUPERSAMPLE_BORDERS:
        raise ValueError("unsupported border mode %r (warp_perspective_supersampled: BORDER_CONSTANT, _REPLICATE, _REFLECT, _WRAP, _REFLECT_101)" % (border_mode,))
    border_mode = int(border_mode)
    interp = _interp("warp_perspective_supersampled", flags)
    dw, dh = int(dsize[0]), int(dsize[1])
    if k * dw > 0x7fffffff or k * dh > 0x7fffffff:
        raise ValueError("warp_perspective_supersampled: the fine grid %d x %d has a side beyond 2^31 - 1" % (k * dw, k * dh))
    s4, _ = _frames("warp_perspective_supersampled", src, _DTYPES)
    B, H, W, C = s4.shape
    esz = s4.element_size()
    M_inv_device, n_m = _matrices(M, flags, M_inv_device, s4.device, B)
    d4 = _pixel_dst(out, s4.dtype, s4.device, B, dh, dw, C)
    bv = _border(border_value, C) if border_mode == BORDER_CONSTANT else None
    _lib.launch("bevwarp_warp_border", s4.device, s4.data_ptr(), d4.data_ptr(), B, H, W, dh, dw, C, s4.stride(0) * esz, s4.stride(1) * esz, d4.stride(0) * esz,
                d4.stride(1) * esz, M_inv_device.data_ptr(), n_m, _DTYPES[s4.dtype], interp | _SUPERSAMPLE[k], border_mode, _ptr(bv))
    return _like_src(d4, src.dim(), out)


def _intrinsics(K):
    """(fx, fy, cx, cy) of a 3x3 or 3x4 camera matrix without skew."""
    K = np.asarray(K, dtype=np.float64)
    if K.shape not in ((3, 3), (3, 4)):
        raise ValueError("K must be 3x3 or 3x4, got %s" % (K.shape,))
    if K[0, 1] != 0.0:
        raise ValueError("K has skew (K[0, 1] = %r): the lens warp takes fx, fy, cx, cy only" % (K[0, 1],))
    return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])


def ray_matrix(M, K, inverse_given=False, oriented=False):
    """The matrix bevwarp_warp_lens takes: destination pixel -> normalised undistorted camera plane, inv(K) @ inv(M) written out.
    M (3, 3) or (..., 3, 3): the forward map from UNDISTORTED source pixels to destination pixels (inverse_given: its inverse);
    K: 3x3 or 3x4 camera matrix, no skew (ValueError).  With rows m0, m1, m2 of the inverse:
    R = [(m0 - cx m2) / fx, (m1 - cy m2) / fy, m2], elementwise in float64.  Returns float64 of M's shape.
    oriented   the rational model divides the ray by its depth and does not see the sign of R; the fisheye model does not divide, and
               R (x, y, 1) has to point FORWARD for the pixels the camera sees.  True: R carries the sign of the third component of
               p = M (cx, cy, 1) (inverse_given: of the solution of M p = (cx, cy, 1)), the homogeneous destination point of the
               optical axis -- at the pixel p / p2 the ray is then (0, 0, 1 / |p2|), forward.  M and -M give the same R.  A homography
               is orientable only where its denominator keeps one sign; for an affine M (every BEVWorldSpec) that is everywhere.
               False (default): R as written above."""
    fx, fy, cx, cy = _intrinsics(K)
    Minv = np.ascontiguousarray(M, dtype=np.float64) if inverse_given else invert_homography(M)
    if Minv.shape[-2:] != (3, 3):
        raise ValueError("M must be (..., 3, 3), got %s" % (Minv.shape,))
    m0, m1, m2 = Minv[..., 0, :], Minv[..., 1, :], Minv[..., 2, :]
    R = np.stack([(m0 - cx * m2) / fx, (m1 - cy * m2) / fy, m2], axis=-2)
    if oriented:
        c = np.array([cx, cy, 1.0])
        p2 = np.linalg.solve(Minv, np.broadcast_to(c, Minv.shape[:-1])[..., None])[..., 2, 0] if inverse_given else (np.asarray(M, dtype=np.float64) @ c)[..., 2]
        R = R * np.where(p2 < 0.0, -1.0, 1.0)[..., None, None]
    return R


def _dist8(dist_coeff):
    """dist_coeff (None, or 4, 5 or 8 values in OpenCV's order) as (k1, k2, p1, p2, k3, k4, k5, k6)."""
    out = np.zeros(8, dtype=np.float64)
    if dist_coeff is not None:
        d = np.asarray(dist_coeff, dtype=np.float64).ravel()
        if d.size not in (4, 5, 8):
            raise ValueError("dist_coeff must hold 4, 5 or 8 values (k1, k2, p1, p2[, k3[, k4, k5, k6]]), got %d" % d.size)
        out[:d.size] = d
    return out


def lens_valid_r2(dist_coeff):
    """The squared radius (normalised camera plane) up to which the radial lens model is monotonic and finite: what
    warp_perspective_lens passes as r2_max.  With s = r^2, N = 1 + k1 s + k2 s^2 + k3 s^3 and D = 1 + k4 s + k5 s^2 + k6 s^3, the
    distorted radius r N / D stops growing where (N + 2 s N') D - 2 s N D' = 0 and has a pole where D = 0: the smallest positive
    real root of either, `inf` if there is none.  Beyond it the model folds back and maps far-away destination pixels INTO the
    frame -- ghost copies of it.  Host numpy (companion-matrix roots).  The tangential terms p1, p2 are ignored: they shift the
    fold by an amount of their own order, and the radius is a guard, not a calibration."""
    k1, k2, _, _, k3, k4, k5, k6 = _dist8(dist_coeff)
    P = np.polynomial.polynomial
    N, D = np.array([1.0, k1, k2, k3]), np.array([1.0, k4, k5, k6])
    s2 = np.array([0.0, 2.0])
    fold = P.polysub(P.polymul(P.polyadd(N, P.polymul(s2, P.polyder(N))), D), P.polymul(P.polymul(s2, N), P.polyder(D)))
    best = np.inf
    for poly in (fold, D):
        c = np.trim_zeros(poly, "b")
        if c.size < 2:
            continue
        for r in P.polyroots(c):
            if abs(r.imag) <= 1e-9 * max(1.0, abs(r.real)) and r.real > 0.0:
                best = min(best, float(r.real))
    return best


LENS_FISHEYE = 0x100  # BEVWARP_LENS_FISHEYE: ORed into the ABI's interp (direction) word


def _lens_model(who, lens_model, r2_max=None, theta_max=None):
    """lens_model ("rational" | "fisheye") as a bool, fisheye; each model has its own guard keyword."""
    if lens_model not in ("rational", "fisheye"):
        raise ValueError("%s: lens_model must be 'rational' or 'fisheye', got %r" % (who, lens_model))
    fisheye = lens_model == "fisheye"
    if fisheye and r2_max is not None:
        raise ValueError("%s: the fisheye model's guard is theta_max (radians), not r2_max" % who)
    if not fisheye and theta_max is not None:
        raise ValueError("%s: the rational model's guard is r2_max, not theta_max" % who)
    return fisheye


def _fisheye4(dist_coeff):
    """dist_coeff of the fisheye model (None, or cv2.fisheye's D: k1, k2, k3, k4) as 4 float64."""
    if dist_coeff is None:
        return np.zeros(4, dtype=np.float64)
    d = np.asarray(dist_coeff, dtype=np.float64).ravel()
    if d.size != 4:
        raise ValueError("dist_coeff must hold 4 values (k1, k2, k3, k4) for the fisheye model, got %d" % d.size)
    return d


def fisheye_valid_theta(dist_coeff):
    """The angle from the optical axis (radians) up to which the fisheye model theta (1 + k1 theta^2 + ... + k4 theta^8) is monotonic:
    the smallest positive real root of its derivative D = 1 + 3 k1 theta^2 + 5 k2 theta^4 + 7 k3 theta^6 + 9 k4 theta^8, capped at pi
    (no ray is further from the axis); pi when there is none.  The analogue of lens_valid_r2, and what the fisheye entries pass as
    theta_max.  Host numpy (companion-matrix roots in theta^2)."""
    k1, k2, k3, k4 = _fisheye4(dist_coeff)
    c = np.trim_zeros(np.array([1.0, 3.0 * k1, 5.0 * k2, 7.0 * k3, 9.0 * k4]), "b")
    best = math.pi
    if c.size >= 2:
        for r in np.polynomial.polynomial.polyroots(c):
            if abs(r.imag) <= 1e-9 * max(1.0, abs(r.real)) and r.real > 0.0:
                best = min(best, math.sqrt(float(r.real)))
    return best


def _fisheye_lens(who, K, dist_coeff, theta_max):
    """(lens of 12 doubles: fx, fy, cx, cy, k1..k4, four zeros; theta_max) as the ABI takes them under BEVWARP_LENS_FISHEYE."""
    if K is None:
        raise ValueError("%s: the fisheye model needs the camera matrix K" % who)
    d = _fisheye4(dist_coeff)
    lens = np.ascontiguousarray(np.concatenate([_intrinsics(K), d, np.zeros(4)]), dtype=np.float64)
    return lens, (fisheye_valid_theta(d) if theta_max is None else float(theta_max))


def lens_from_calib(calib):
    """(K, dist_coeff) of a Calib for warp_perspective_lens: calib.K as float64 and calib.dist_coeff (None gives five zeros).
    A Calib without K -- `from_pts` mode pins the homography alone -- raises ValueError."""
    if getattr(calib, "K", None) is None:
        raise ValueError("this Calib has no K (mode %r): a lens model needs the camera matrix" % (getattr(calib, "mode", None),))
    d = calib.dist_coeff
    return np.asarray(calib.K, dtype=np.float64), (np.zeros(5) if d is None else np.asarray(d, dtype=np.float64).ravel())


def warp_perspective_lens(src, M, dsize, K, dist_coeff, flags=INTER_LINEAR, border_value=None, out=None, border_mode=BORDER_CONSTANT, r2_max=None,
                          lens_model="rational", theta_max=None):
    """warp_perspective of the frames a distorted camera delivers: what cv2.undistort(src, K, dist_coeff) followed by
    cv2.warpPerspective(undistorted, M, dsize) is for, with the lens model folded into the coordinate chain -- one launch, one
    resampling of the raw frame, no undistorted frame in memory (include/bevwarp.h, bevwarp_warp_lens; not bit-equal to the cv2 pair,
    which resamples twice).

    src, dsize, border_value, out   as warp_perspective.
    M        forward map from UNDISTORTED source pixels to destination pixels, (3, 3) or (B, 3, 3) (host): exactly what
             warp_perspective takes for frames that went through cv2.undistort; flags | WARP_INVERSE_MAP: the dst -> src map.
    K        3x3 or 3x4 camera matrix of the raw frames, no skew.
    dist_coeff   None, or 4, 5 or 8 values in OpenCV's order (k1, k2, p1, p2[, k3[, k4, k5, k6]]): the rational model; thin-prism,
             tilt and fisheye terms are not taken.  None or all zero: the call IS warp_perspective(src, M, dsize, ...), bit for bit.
    flags    INTER_LINEAR (default) or INTER_NEAREST, optionally | WARP_INVERSE_MAP.
    border_mode   BORDER_CONSTANT (default) or BORDER_TRANSPARENT.
    r2_max   destination pixels whose squared radius on the normalised camera plane exceeds it are outside the frame; None:
             lens_valid_r2(dist_coeff), which keeps the model's fold-back from painting ghost copies; float("inf"): no limit.
    lens_model   "rational" (default: everything above), or "fisheye": the equidistant model of cv2.fisheye (include/bevwarp.h,
             BEVWARP_LENS_FISHEYE).  dist_coeff is then None or its 4 values (k1, k2, k3, k4); the guard is theta_max, the angle from the
             optical axis in radians (None: fisheye_valid_theta(dist_coeff); passing r2_max raises ValueError); the ray matrix is built
             oriented (ray_matrix), so rays at and beyond 90 degrees are pixels like any other; and a lens without distortion is still a
             fisheye lens -- nothing is handed to warp_perspective.
    Asynchronous on the current stream.  No verdict tables, no plan cache: the lens and r2_max travel with every call (the ray
    matrices are uploaded through device_inverse's by-value cache, which holds matrices only)."""
    fisheye = _lens_model("warp_perspective_lens", lens_model, r2_max, theta_max)
    if fisheye:
        lens, r2 = _fisheye_lens("warp_perspective_lens", K, dist_coeff, theta_max)
    else:
        dist = _dist8(dist_coeff)
    if not fisheye and not dist.any():
        return warp_perspective(src, M, dsize, flags=flags, border_value=border_value, out=out, border_mode=border_mode)
    if border_mode not in (BORDER_CONSTANT, BORDER_TRANSPARENT):
        raise ValueError("unsupported border mode %r (warp_perspective_lens: BORDER_CONSTANT, BORDER_TRANSPARENT)" % (border_mode,))
    border_mode = int(border_mode)
    interp = _interp("warp_perspective_lens", flags)
    s4, _ = _frames("warp_perspective_lens", src, _DTYPES)
    B, H, W, C = s4.shape
    dw, dh = int(dsize[0]), int(dsize[1])
    esz = s4.element_size()
    Mh = M.detach().cpu().numpy() if isinstance(M, torch.Tensor) else M
    R = ray_matrix(Mh, K, inverse_given=bool(int(flags) & WARP_INVERSE_MAP), oriented=fisheye)
    M_ray, n_m = _matrices(R, WARP_INVERSE_MAP, None, s4.device, B)
    if not fisheye:
        lens = np.ascontiguousarray(np.concatenate([_intrinsics(K), dist]), dtype=np.float64)
        r2 = lens_valid_r2(dist) if r2_max is None else float(r2_max)
    d4 = _pixel_dst(out, s4.dtype, s4.device, B, dh, dw, C, zeroed=border_mode == BORDER_TRANSPARENT)
    bv = _border(border_value, C) if border_mode == BORDER_CONSTANT else None
    _lib.launch("bevwarp_warp_lens", s4.device, s4.data_ptr(), d4.data_ptr(), B, H, W, dh, dw, C, s4.stride(0) * esz, s4.stride(1) * esz, d4.stride(0) * esz,
                d4.stride(1) * esz, M_ray.data_ptr(), n_m, _ptr(lens), r2, _DTYPES[s4.dtype], interp | (LENS_FISHEYE if fisheye else 0), border_mode, _ptr(bv))
    return _like_src(d4, src.dim(), out)


class WarpMap:
    """The coordinates of one warp, kept: OpenCV's fixed-point map pair (include/bevwarp.h, "THE MAP FORMAT") for `n` cameras or frames.

    xy       (n, dh, dw, 2) torch.int16: (sx, sy) per destination pixel (CV_16SC2).
    frac     (n, dh, dw) torch.int16 holding (fy << 5) | fx (CV_16UC1; the values are below 1024), or None for INTER_NEAREST.
    interp   INTER_NEAREST or INTER_LINEAR: the interpolation the map was built for (sx differs by it).  An INTER_LINEAR map also serves
             bicubic sampling: remap(..., interpolation=INTER_CUBIC) -- no map is built for INTER_CUBIC.
    dsize    (width, height).
    The planes may be views (padded rows, an offset base): their strides are passed through.  build_warp_map makes one on the device;
    a hand-made pair (cv2.convertMaps's output, say) is wrapped by calling the class."""

    def __init__(self, xy, frac, interp, dsize):
        interp = int(interp)
        if interp not in (INTER_NEAREST, INTER_LINEAR):
            raise ValueError("a WarpMap is built for INTER_NEAREST or INTER_LINEAR, got %r" % (interp,))
        dw, dh = int(dsize[0]), int(dsize[1])
        if not isinstance(xy, torch.Tensor) or xy.dtype != torch.int16 or xy.dim() != 4 or tuple(xy.shape[1:]) != (dh, dw, 2) or xy.shape[0] < 1:
            raise ValueError("xy must be an int16 tensor (n, %d, %d, 2), got %s %s" % (dh, dw, getattr(xy, "dtype", type(xy)), tuple(getattr(xy, "shape", ()))))
        if xy.stride(3) != 1 or xy.stride(2) != 2:
            raise ValueError("the (sx, sy) pairs of xy and the pairs of a row must be contiguous")
        if interp == INTER_LINEAR or frac is not None:
            if not isinstance(frac, torch.Tensor) or frac.dtype != torch.int16 or tuple(frac.shape) != (xy.shape[0], dh, dw) or frac.device != xy.device:
                raise ValueError("frac must be an int16 tensor %s on %s%s" % ((xy.shape[0], dh, dw), xy.device, "" if frac is not None else " (INTER_LINEAR needs one)"))
            if frac.stride(2) != 1:
                raise ValueError("the rows of frac must be contiguous")
        self.xy, self.frac, self.interp, self.dsize = xy, frac, interp, (dw, dh)

    @property
    def n(self):
        return int(self.xy.shape[0])

    @property
    def device(self):
        return self.xy.device

    def _planes(self):
        """(xy address, frac address or None, the four strides in bytes) as the ABI takes them."""
        f = self.frac if self.interp == INTER_LINEAR else None
        return (self.xy.data_ptr(), None if f is None else f.data_ptr(), self.xy.stride(0) * 2, self.xy.stride(1) * 2,
                0 if f is None else f.stride(0) * 2, 0 if f is None else f.stride(1) * 2)


def build_warp_map(M, dsize, flags=INTER_LINEAR, K=None, dist_coeff=None, r2_max=None, device="cuda", out=None, lens_model="rational", theta_max=None):
    """The coordinate chain of warp_perspective / warp_perspective_lens run ONCE, on the device, and kept as a WarpMap for remap():
    what cv2.initUndistortRectifyMap + cv2.convertMaps are for in a fixed camera's loop (include/bevwarp.h, bevwarp_build_map).

    M        (3, 3) or (n, 3, 3) forward map(s) (host), as warp_perspective / warp_perspective_lens take them; flags | WARP_INVERSE_MAP:
             the dst -> src map(s).  n matrices give a map of n frames.
    dsize    (width, height).  flags: INTER_LINEAR (default) or INTER_NEAREST, optionally | WARP_INVERSE_MAP.
    K, dist_coeff   the lens, as warp_perspective_lens takes it.  dist_coeff None or all zero: the pinhole chain (K is not looked at) --
             the rule by which warp_perspective_lens hands a lens without distortion to warp_perspective.
    r2_max   None: lens_valid_r2(dist_coeff); a pixel beyond it is stored as the entry whose taps are all outside.
    out      a WarpMap of this n, dsize and interpolation on `device` to write into (its planes may be views).  A `device` without an
             index (the default) then means the map's device, which need not be the current one.
    lens_model, theta_max   as warp_perspective_lens: "fisheye" builds the map of an equidistant lens (K is needed; dist_coeff None or 4
             values; theta_max None: fisheye_valid_theta(dist_coeff)).  The map's format is the same, so remap, the stitches and the
             pipelines serve a fisheye camera as they stand.
    remap(src, build_warp_map(...)) equals warp_perspective(src, ..., border_mode=m) for every border mode, and warp_perspective_lens
    for BORDER_CONSTANT and BORDER_TRANSPARENT, by bits.  flags=INTER_CUBIC stays a ValueError: bicubic samples the INTER_LINEAR map,
    remap(src, build_warp_map(..., flags=INTER_LINEAR), interpolation=INTER_CUBIC).  Asynchronous on the current stream."""
    fisheye = _lens_model("build_warp_map", lens_model, r2_max, theta_max)
    interp = _interp("build_warp_map", flags)
    dw, dh = int(dsize[0]), int(dsize[1])
    if dw <= 0 or dh <= 0:
        raise ValueError("build_warp_map: dsize must be positive, got %s" % ((dw, dh),))
    dist = np.zeros(8) if fisheye else _dist8(dist_coeff)
    inverse = bool(int(flags) & WARP_INVERSE_MAP)
    Mh = np.asarray(M.detach().cpu().numpy() if isinstance(M, torch.Tensor) else M, dtype=np.float64)
    if Mh.shape[-2:] != (3, 3) or Mh.ndim not in (2, 3):
        raise ValueError("M must be (3, 3) or (n, 3, 3), got %s" % (Mh.shape,))
    lens = None
    if fisheye:
        lens, r2 = _fisheye_lens("build_warp_map", K, dist_coeff, theta_max)
        Mh, inverse = ray_matrix(Mh, K, inverse_given=inverse, oriented=True), True
    elif dist.any():
        if K is None:
            raise ValueError("build_warp_map: a lens (dist_coeff) needs the camera matrix K")
        lens = np.ascontiguousarray(np.concatenate([_intrinsics(K), dist]), dtype=np.float64)
        r2 = lens_valid_r2(dist) if r2_max is None else float(r2_max)
        Mh, inverse = ray_matrix(Mh, K, inverse_given=inverse), True
    n = int(Mh.size // 9)
    device = torch.device(device)
    if out is not None:
        if not isinstance(out, WarpMap) or out.n != n or out.dsize != (dw, dh) or out.interp != interp or out.device.type != device.type:
            raise ValueError("out must be a WarpMap of %d frame(s), dsize %s and interpolation %d on %s" % (n, (dw, dh), interp, device))
        if device.index is None:
            device = out.device  # (the matrices go where the map is: "cuda" alone would upload them to the current device)
        elif out.device != device:
            raise ValueError("out is on %s, device is %s" % (out.device, device))
    if device.type != "cuda":
        raise ValueError("build_warp_map needs a CUDA (HIP) device, got %s" % (device,))
    minv = device_inverse(Mh, device, inverse_given=inverse)
    if out is None:
        xy = torch.empty((n, dh, dw, 2), dtype=torch.int16, device=minv.device)
        out = WarpMap(xy, torch.empty((n, dh, dw), dtype=torch.int16, device=minv.device) if interp == INTER_LINEAR else None, interp, (dw, dh))
    xy_p, fr_p, xy_fs, xy_rs, fr_fs, fr_rs = out._planes()
    _lib.launch("bevwarp_build_map", out.device, minv.data_ptr(), n, _ptr(lens), 0.0 if lens is None else r2, interp | (LENS_FISHEYE if fisheye else 0), xy_p, fr_p, dh, dw, xy_fs, xy_rs, fr_fs, fr_rs)
    return out


def _map_call(who, warp_map, border_mode):
    """What the entries that sample through a map check before they look at a tensor: the border mode as an int."""
    if not isinstance(warp_map, WarpMap):
        raise ValueError("%s needs a WarpMap (build_warp_map, or WarpMap(xy, frac, interp, dsize)), got %s" % (who, type(warp_map).__name__))
    if border_mode not in _BORDER_MODES:
        raise ValueError("unsupported border mode %r (BORDER_CONSTANT, _REPLICATE, _REFLECT, _WRAP, _REFLECT_101, _TRANSPARENT)" % (border_mode,))
    return int(border_mode)


def _map_fits(warp_map, B, device):
    """A map serves a batch of B frames on `device`: one frame shared by all or one per frame, on the frames' device."""
    if warp_map.n not in (1, B):
        raise ValueError("the map holds %d frames for a batch of %d (1 or the batch)" % (warp_map.n, B))
    if warp_map.device != device:
        raise ValueError("the map is on %s, the frames are on %s" % (warp_map.device, device))


def _map_interpolation(who, warp_map, interpolation):
    """The `interp` word of bevwarp_remap for a map sampled with `interpolation`: None or the map's own interpolation is the map's;
    INTER_CUBIC samples a bilinear map bicubically (BEVWARP_MAP_BICUBIC); anything else is refused before a tensor is touched."""
    if interpolation is None:
        return warp_map.interp
    if isinstance(interpolation, bool) or not isinstance(interpolation, (int, np.integer)):
        raise ValueError("%s: interpolation must be None, the map's own interpolation or INTER_CUBIC, got %r" % (who, interpolation))
    interpolation = int(interpolation)
    if interpolation == warp_map.interp:
        return warp_map.interp
    if interpolation == INTER_CUBIC:
        if warp_map.interp != INTER_LINEAR:
            raise ValueError("%s: bicubic samples a bilinear map (build_warp_map(flags=INTER_LINEAR)); this map was built for INTER_NEAREST" % who)
        return INTER_LINEAR | _lib.MAP_BICUBIC
    raise ValueError("%s: interpolation must be None, the map's own interpolation (%d) or INTER_CUBIC, got %r" % (who, warp_map.interp, interpolation))


def remap(src, warp_map, border_mode=BORDER_CONSTANT, border_value=None, out=None, interpolation=None):
    """cv2.remap on the GPU, batched: frames sampled through a WarpMap (include/bevwarp.h, bevwarp_remap) -- no coordinate is computed,
    no float64 is touched.  The per-frame half of a fixed camera's loop; build_warp_map is the other.

    src      (B, H, W, C), (H, W, C) or (H, W) uint8 / float32 CUDA tensor, as warp_perspective.
    warp_map a WarpMap on src's device with n == 1 (shared by all frames) or n == B; its interpolation is the call's.
    border_mode   any of the six BORDER_* modes; border_value (BORDER_CONSTANT only) a scalar or C values, None = 0.
    out      as warp_perspective; BORDER_TRANSPARENT without `out` starts from zeros.
    interpolation   None (default) or the map's own interpolation: the map's.  INTER_CUBIC with an INTER_LINEAR map: the map is sampled
             bicubically (BEVWARP_MAP_BICUBIC) -- cv2.INTER_CUBIC is defined on the bilinear map, so no map is built for it, and with a lens
             or fisheye map this is the bicubic resampling of a raw distorted frame in one pass.  With a pinhole map the result equals
             warp_perspective(flags=INTER_CUBIC, border_mode=m) by bits in all six modes.  INTER_CUBIC with an INTER_NEAREST map, and any
             other value, is a ValueError.
    Returns a tensor shaped like src with (height, width) replaced by the map's, or `out`.  Asynchronous on the current stream."""
    border_mode = _map_call("remap", warp_map, border_mode)
    interp = _map_interpolation("remap", warp_map, interpolation)
    if not isinstance(src, torch.Tensor) or src.dtype not in _DTYPES or src.dim() not in (2, 3, 4):
        raise ValueError("remap needs a uint8 or float32 tensor (B, H, W, C), (H, W, C) or (H, W)")
    B = src.shape[0] if src.dim() == 4 else 1
    C = 1 if src.dim() == 2 else src.shape[-1]
    dw, dh = warp_map.dsize
    _map_fits(warp_map, B, src.device)
    if isinstance(out, torch.Tensor) and out.dim() == src.dim():  # (an `out` of src's rank names a size: the map's, or the call is refused)
        hw = tuple(out.shape[-2:]) if src.dim() == 2 else tuple(out.shape[-3:-1])
        if hw != (dh, dw):
            raise ValueError("the map's dsize is %s, out is %s" % ((dw, dh), tuple(out.shape)))
    if isinstance(out, torch.Tensor) and out.numel() != B * dh * dw * C:
        raise ValueError("the map's dsize is %s (%d frames of %d channels): out has %d elements" % ((dw, dh), B, C, out.numel()))
    s4, _ = _frames("remap", src, _DTYPES)
    B, H, W, C = s4.shape
    esz = s4.element_size()
    d4 = _pixel_dst(out, s4.dtype, s4.device, B, dh, dw, C, zeroed=border_mode == BORDER_TRANSPARENT)
    bv = _border(border_value, C) if border_mode == BORDER_CONSTANT else None
    xy_p, fr_p, xy_fs, xy_rs, fr_fs, fr_rs = warp_map._planes()
    _lib.launch("bevwarp_remap", s4.device, s4.data_ptr(), d4.data_ptr(), B, H, W, dh, dw, C, s4.stride(0) * esz, s4.stride(1) * esz, d4.stride(0) * esz,
                d4.stride(1) * esz, xy_p, fr_p, warp_map.n, xy_fs, xy_rs, fr_fs, fr_rs, _DTYPES[s4.dtype], interp, border_mode, _ptr(bv))
    return _like_src(d4, src.dim(), out)


def convert_maps(map1, map2=None, nearest=False):
    """cv2.convertMaps(map1, map2, CV_16SC2, nninterpolation=nearest) on the host, in numpy: float32 coordinate maps -> the fixed-point
    pair (xy (H, W, 2) int16, frac (H, W) uint16; frac is None for nearest).  map1 is (H, W, 2) holding (x, y), or map1 / map2 are the
    (H, W) x and y maps.  Per coordinate: multiplied by 32 IN FLOAT32, rounded half to even, clamped to int32 (NaN: INT_MAX, as the
    warp's chain has it), then sx = sat16(X >> 5), fx = X & 31; nearest rounds the coordinate itself and sx = sat16(X).  Restated from
    memory of imgwarp.cpp: parity with an installed cv2 is unpinned, like the rest of the warp."""
    m1 = np.asarray(map1)
    if map2 is None:
        if m1.ndim != 3 or m1.shape[2] != 2:
            raise ValueError("convertMaps: map1 must be (H, W, 2) when map2 is absent, got %s" % (m1.shape,))
        x, y = m1[..., 0], m1[..., 1]
    else:
        x, y = m1, np.asarray(map2)
        if x.ndim != 2 or x.shape != y.shape:
            raise ValueError("convertMaps: map1 and map2 must be (H, W) maps of one shape, got %s and %s" % (x.shape, y.shape))
    if x.dtype != np.float32 or y.dtype != np.float32:
        raise ValueError("convertMaps: float32 maps are needed, got %s and %s" % (x.dtype, y.dtype))

    def fixed(c):
        with np.errstate(all="ignore"):
            v = (c if nearest else c * np.float32(32.0)).astype(np.float64)
            v = np.where(np.isnan(v), 2147483647.0, np.clip(np.rint(v), -2147483648.0, 2147483647.0))
        return v.astype(np.int64)

    X, Y = fixed(x), fixed(y)
    if nearest:
        return np.stack([np.clip(X, -32768, 32767), np.clip(Y, -32768, 32767)], axis=-1).astype(np.int16), None
    xy = np.stack([np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)], axis=-1).astype(np.int16)
    return xy, (((Y & 31) << 5) | (X & 31)).astype(np.uint16)


def remap_numpy(src, map1, map2, interpolation, dst=None, borderMode=BORDER_CONSTANT, borderValue=0, device="cuda"):
    """cv2.remap call shape for numpy images and maps: uploads, samples on the GPU, downloads (cv2_compat.remap).  Maps: (H, W, 2) int16
    + (H, W) uint16 (None for INTER_NEAREST) are taken as they are; float32 maps -- (H, W, 2), or an (H, W) pair -- go through
    convert_maps first.  With BORDER_TRANSPARENT a given `dst` is the canvas."""
    interp = _interp("remap", interpolation)
    if borderMode not in _BORDER_MODES:
        raise ValueError("unsupported borderMode %r (BORDER_CONSTANT, _REPLICATE, _REFLECT, _WRAP, _REFLECT_101, _TRANSPARENT)" % (borderMode,))
    img = np.asarray(src)
    if img.dtype not in (np.uint8, np.float32) or img.ndim not in (2, 3):
        raise ValueError("remap: a uint8 / float32 image (H, W) or (H, W, C) is needed, got %s %s" % (img.dtype, img.shape))
    m1 = np.asarray(map1)
    if m1.dtype == np.float32:
        xy, frac = convert_maps(m1, map2, nearest=interp == INTER_NEAREST)
    elif m1.dtype == np.int16 and m1.ndim == 3 and m1.shape[2] == 2:
        xy, frac = m1, None if map2 is None else np.asarray(map2)
        if interp == INTER_LINEAR and (frac is None or frac.dtype != np.uint16 or frac.shape != m1.shape[:2]):
            raise ValueError("remap: INTER_LINEAR with fixed-point maps needs map2 as uint16 %s" % (m1.shape[:2],))
    else:
        raise ValueError("remap: map1 must be float32 or (H, W, 2) int16, got %s %s" % (m1.dtype, m1.shape))
    dh, dw = xy.shape[:2]
    shape = (dh, dw) + tuple(img.shape[2:])
    canvas = None
    if borderMode == BORDER_TRANSPARENT and dst is not None:
        if not isinstance(dst, np.ndarray) or dst.shape != shape or dst.dtype != img.dtype:
            raise ValueError("dst must be a %s array of shape %s (the canvas BORDER_TRANSPARENT writes into)" % (img.dtype, shape))
        canvas = torch.from_numpy(np.ascontiguousarray(dst)).to(device)
    txy = torch.from_numpy(np.ascontiguousarray(xy)).to(device)[None]
    tfr = None if interp == INTER_NEAREST else torch.from_numpy(np.ascontiguousarray(frac).view(np.int16)).to(device)[None]
    t = torch.from_numpy(np.ascontiguousarray(img)).to(device)
    bv = scalar_border(borderValue, 1 if img.ndim == 2 else img.shape[2])
    res = remap(t, WarpMap(txy, tfr, interp, (dw, dh)), border_mode=borderMode, border_value=bv, out=canvas).cpu().numpy()
    if dst is not None:
        dst[...] = res
        return dst
    return res


_BLENDS = {"over": _lib.STITCH_OVER, "feather": _lib.STITCH_FEATHER}


def _one_kind(who, srcs):
    """The cameras of a stitch that takes any pixel type (tensors of rank 2..4) are of one kind, which is returned: (dtype, channels, batch,
    device).  Compared on the tensors as given, before anything asks for a device."""
    kinds = [(src.dtype, 1 if src.dim() == 2 else src.shape[-1], src.shape[0] if src.dim() == 4 else 1, src.device) for src in srcs]
    for k, kind in enumerate(kinds):
        if kind != kinds[0]:
            raise ValueError("camera %d has dtype %s, %d channels, batch %d on %s; camera 0 has dtype %s, %d channels, batch %d on %s "
                             "(%s: one dtype, channel count, batch and device)" % ((k,) + kind + kinds[0] + (who,)))
    return kinds[0]


def warp_stitch(srcs, Ms, dsize, flags=INTER_LINEAR, blend="over", feather=64, border_value=None, out=None, border_mode=BORDER_CONSTANT):
    """The cameras of one site warped into ONE canvas in one launch (include/bevwarp.h, bevwarp_warp_stitch): what one
    warp_perspective(..., border_mode=BORDER_TRANSPARENT, out=canvas) per camera is for, without a pass over the canvas per camera, and
    with a blend where cameras overlap.

    srcs     a sequence of 1..8 CUDA tensors, each (B, H_k, W_k, C), (H_k, W_k, C) or (H_k, W_k): one dtype (uint8 / float32), one C, one B
             and one device; sizes and strides may differ from camera to camera.
    Ms       as many forward maps, camera px -> canvas px, each (3, 3) or (B, 3, 3) (host); flags | WARP_INVERSE_MAP: all of them are
             canvas -> camera maps.
    dsize    (width, height) of the canvas.  flags: INTER_LINEAR (default) or INTER_NEAREST, optionally | WARP_INVERSE_MAP.
    blend    a camera covers a canvas pixel where BORDER_TRANSPARENT would write it.
             "over": the last covering camera of the list wins -- bit for bit the one-call-per-camera route;
             "feather": the covering cameras are averaged with integer weights min(d, feather), d the distance in whole source pixels
             to the nearest edge of the camera's frame: a camera fades out over its outermost `feather` (1..4096) pixels, and a pixel
             that one camera alone covers is that camera's pixel, by bits.  feather=1 is the plain mean.
    border_mode   BORDER_CONSTANT (default): pixels no camera covers are `border_value` (scalar or C values, None = 0);
             BORDER_TRANSPARENT: they keep what `out` held (zero without `out`).
    Returns a tensor shaped like srcs[0] with (height, width) replaced, or `out`.  Asynchronous on the current stream.  No verdict
    tables, no plan cache."""
    srcs, Ms = list(srcs), list(Ms)
    if not 1 <= len(srcs) <= _lib.STITCH_MAX_CAMERAS:
        raise ValueError("warp_stitch takes 1..%d cameras, got %d" % (_lib.STITCH_MAX_CAMERAS, len(srcs)))
    if len(Ms) != len(srcs):
        raise ValueError("got %d homography sets for %d cameras" % (len(Ms), len(srcs)))
    if blend not in _BLENDS:
        raise ValueError("unsupported blend %r (warp_stitch: \"over\", \"feather\")" % (blend,))
    if blend == "feather" and not 1 <= int(feather) <= 4096:
        raise ValueError("feather must lie in 1..4096, got %r" % (feather,))
    if border_mode not in (BORDER_CONSTANT, BORDER_TRANSPARENT):
        raise ValueError("unsupported border mode %r (warp_stitch: BORDER_CONSTANT, BORDER_TRANSPARENT)" % (border_mode,))
    border_mode = int(border_mode)
    interp = _interp("warp_stitch", flags)
    if all(isinstance(src, torch.Tensor) and src.dim() in (2, 3, 4) for src in srcs):  # (_frames refuses the others, one by one)
        _one_kind("warp_stitch", srcs)
    frames = [_frames("warp_stitch", src, _DTYPES)[0] for src in srcs]  # (a copy made here lives until the launch is enqueued)
    s0 = frames[0]
    B, C = s0.shape[0], s0.shape[3]
    dw, dh = int(dsize[0]), int(dsize[1])
    esz = s0.element_size()
    cams = (_lib.Camera * len(frames))()
    minvs = []
    for cam, s4, M in zip(cams, frames, Ms):
        minv, n_m = _matrices(M, flags, None, s4.device, B)
        minvs.append(minv)
        cam.src, cam.M_inv, cam.frame_stride, cam.row_stride = s4.data_ptr(), minv.data_ptr(), s4.stride(0) * esz, s4.stride(1) * esz
        cam.src_h, cam.src_w, cam.m_count, cam.reserved = s4.shape[1], s4.shape[2], n_m, 0
    d4 = _pixel_dst(out, s0.dtype, s0.device, B, dh, dw, C, zeroed=border_mode == BORDER_TRANSPARENT)
    bv = _border(border_value, C) if border_mode == BORDER_CONSTANT else None
    _lib.launch("bevwarp_warp_stitch", s0.device, ctypes.addressof(cams), len(frames), d4.data_ptr(), B, dh, dw, C, d4.stride(0) * esz, d4.stride(1) * esz,
                _DTYPES[s0.dtype], interp, _BLENDS[blend], int(feather) if blend == "feather" else 0, border_mode, _ptr(bv))  # ("over" ignores feather)
    return _like_src(d4, srcs[0].dim(), out)


def _stitch_maps_call(who, n_cams, warp_maps, blend, feather, border_mode):
    """What the stitches through maps check before they look at a tensor: the camera count, one WarpMap per camera of one dsize and
    interpolation, the blend and the border mode.  Returns (interpolation, (dw, dh), border mode as an int)."""
    if not 1 <= n_cams <= _lib.STITCH_MAX_CAMERAS:
        raise ValueError("%s takes 1..%d cameras, got %d" % (who, _lib.STITCH_MAX_CAMERAS, n_cams))
    if len(warp_maps) != n_cams:
        raise ValueError("got %d warp maps for %d cameras" % (len(warp_maps), n_cams))
    if blend not in _BLENDS:
        raise ValueError("unsupported blend %r (%s: \"over\", \"feather\")" % (blend, who))
    if blend == "feather" and not 1 <= int(feather) <= 4096:
        raise ValueError("feather must lie in 1..4096, got %r" % (feather,))
    if border_mode not in (BORDER_CONSTANT, BORDER_TRANSPARENT):
        raise ValueError("unsupported border mode %r (%s: BORDER_CONSTANT, BORDER_TRANSPARENT)" % (border_mode, who))
    for k, m in enumerate(warp_maps):
        if not isinstance(m, WarpMap):
            raise ValueError("%s needs a WarpMap per camera (build_warp_map, or WarpMap(xy, frac, interp, dsize)); camera %d has %s" % (who, k, type(m).__name__))
        if m.dsize != warp_maps[0].dsize or m.interp != warp_maps[0].interp:
            raise ValueError("the map of camera %d has dsize %s and interpolation %d; camera 0's has dsize %s and interpolation %d (%s: one canvas, one interpolation)"
                             % (k, m.dsize, m.interp, warp_maps[0].dsize, warp_maps[0].interp, who))
    return warp_maps[0].interp, warp_maps[0].dsize, int(border_mode)


def _stitch_gains(who, gains, n_cams, srcs=None):
    """`gains=` of the stitches through maps (bev_amd.exposure.quantize_gains: (n_cams,) or (n_cams, 3) floats in [0, 1023/256], None: no
    gains), checked before a tensor's device is looked at.  srcs: remap_stitch's frames, which under gains are uint8 with 3 channels.
    Returns (the flag to OR into `blend`, the cameras' gain words): (0, ()) without gains."""
    if gains is None:
        return 0, ()
    words = _exposure.gain_words(_exposure.quantize_gains(gains, n_cams))
    for k, src in enumerate(srcs or ()):
        if src.dtype != torch.uint8 or src.dim() < 3 or src.shape[-1] != 3:
            raise ValueError("%s: gains apply to uint8 frames of 3 channels; camera %d is %s %s" % (who, k, src.dtype, tuple(src.shape)))
    return _lib.STITCH_GAIN, words


def _set_gain_words(cams, words):
    """The gain words into the camera table (bevwarp_map_camera.reserved); the library reads them during the call only."""
    for cam, w in zip(cams, words):
        cam.reserved = w


def _stitch_maps_dst(out, ndim, B, dh, dw, C):
    """remap's rules for a caller's `out` against the maps' dsize; ndim: the rank of the result of a single camera."""
    if isinstance(out, torch.Tensor) and out.dim() == ndim and ndim >= 2:
        hw = tuple(out.shape[-2:]) if ndim == 2 else tuple(out.shape[-3:-1])
        if hw != (dh, dw):
            raise ValueError("the maps' dsize is %s, out is %s" % ((dw, dh), tuple(out.shape)))
    if isinstance(out, torch.Tensor) and out.numel() != B * dh * dw * C:
        raise ValueError("the maps' dsize is %s (%d frames of %d channels): out has %d elements" % ((dw, dh), B, C, out.numel()))


def _fill_map_camera(cam, warp_map, s=None, uv4=None):
    """One bevwarp_map_camera: its map, and its frames s (B, H, W, C) -- NV12: the Y planes (B, H, W), with the planes of pairs uv4.
    (s=None: the caller fills the frames itself.)"""
    xy_p, fr_p, cam.xy_frame_stride, cam.xy_row_stride, cam.frac_frame_stride, cam.frac_row_stride = warp_map._planes()
    cam.map_xy, cam.map_frac, cam.map_count, cam.reserved = xy_p, fr_p, warp_map.n, 0
    if s is not None:
        esz = s.element_size()
        cam.src, cam.uv, cam.frame_stride, cam.row_stride = s.data_ptr(), None if uv4 is None else uv4.data_ptr(), s.stride(0) * esz, s.stride(1) * esz
        cam.src_h, cam.src_w = s.shape[1], s.shape[2]
    if uv4 is not None:
        cam.uv_frame_stride, cam.uv_row_stride = uv4.stride(0), uv4.stride(1)


def _nv12_map_cameras(who, ys, uvs, warp_maps):
    """The NV12 cameras of a stitch through maps: a plane of pairs per camera, every camera's planes as _nv12_planes takes them, one batch
    and device, a map that serves them per camera.  Returns (planes, cams, B, device): the filled bevwarp_map_camera array, and the
    tensors it points into, which the caller keeps until the launch is enqueued."""
    if len(uvs) != len(ys):
        raise ValueError("got %d uv planes for %d cameras" % (len(uvs), len(ys)))
    planes = [_nv12_planes(who, y, uv) for y, uv in zip(ys, uvs)]
    B, device = planes[0][0].shape[0], planes[0][0].device
    for k, (y, (y3, _)) in enumerate(zip(ys, planes)):
        if y3.shape[0] != B or y3.device != device or y.dim() != ys[0].dim():
            raise ValueError("camera %d has %d frames (y of rank %d) on %s; camera 0 has %d (rank %d) on %s (%s: one batch and device)"
                             % (k, y3.shape[0], y.dim(), y3.device, B, ys[0].dim(), device, who))
    for m in warp_maps:
        _map_fits(m, B, device)
    cams = (_lib.MapCamera * len(planes))()
    for cam, (y3, uv4), m in zip(cams, planes, warp_maps):
        _fill_map_camera(cam, m, y3, uv4)
    return planes, cams, B, device


def remap_stitch(srcs, warp_maps, blend="over", feather=64, border_value=None, out=None, border_mode=BORDER_CONSTANT, gains=None):
    """The FIXED cameras of one site sampled through their warp maps into ONE canvas in one launch (include/bevwarp.h,
    bevwarp_stitch_maps): warp_stitch's cover test and blends over remap's map entries.  What a canvas fill plus one
    remap(..., border_mode=BORDER_TRANSPARENT, out=canvas) per camera is for, without a pass over the canvas per camera, with a blend
    where cameras overlap, with the lens in the maps, and with no coordinate computed and no float64 touched.

    srcs       a sequence of 1..8 CUDA tensors as warp_stitch takes them: one dtype (uint8 / float32), one C, one B and one device; sizes
               and strides may differ from camera to camera.
    warp_maps  as many WarpMaps (build_warp_map: pinhole or lens) on the frames' device, all of one dsize and interpolation, each with
               n == 1 (shared by the batch) or n == B.  Two cameras may share one map.  A camera covers a canvas pixel where its map
               entry is an inlier of its frame; a lens map's pixels beyond r2_max cover nothing.
    blend, feather, border_mode, border_value, out   as warp_stitch.
    gains      None, or per-camera exposure gains (BEVWARP_STITCH_GAIN): (n_cams,) or (n_cams, 3) floats in [0, 1023/256], quantised as
               rint(256 g); uint8 frames of 3 channels only.  Every tap of camera k is replaced, channel by channel, by
               min(255, (p G + 128) >> 8) before the interpolation: the result is remap_stitch's of frames put through
               bev_amd.exposure.apply_gains, by bits, without that pass.  The border pixel is not gained.  Taken by value at the call.
               bev_amd.exposure.estimate_gains finds gains that even out the cameras' exposure.  The other five remap_stitch* take the
               same argument.
    With pinhole maps the result is warp_stitch's for the same matrices, by bits; "over" is what the successive remap calls leave.
    Returns a tensor shaped like srcs[0] with (height, width) replaced by the maps', or `out`.  Asynchronous on the current stream."""
    srcs, warp_maps = list(srcs), list(warp_maps)
    interp, (dw, dh), border_mode = _stitch_maps_call("remap_stitch", len(srcs), warp_maps, blend, feather, border_mode)
    for k, src in enumerate(srcs):
        if not isinstance(src, torch.Tensor) or src.dtype not in _DTYPES or src.dim() not in (2, 3, 4):
            raise ValueError("remap_stitch needs uint8 or float32 tensors (B, H, W, C), (H, W, C) or (H, W); camera %d is %s" % (k, getattr(src, "dtype", type(src))))
    gain_flag, words = _stitch_gains("remap_stitch", gains, len(srcs), srcs)
    _, C, B, device = _one_kind("remap_stitch", srcs)
    for m in warp_maps:
        _map_fits(m, B, device)
    _stitch_maps_dst(out, srcs[0].dim(), B, dh, dw, C)
    frames = [_frames("remap_stitch", src, _DTYPES)[0] for src in srcs]  # (a copy made here lives until the launch is enqueued)
    s0 = frames[0]
    esz = s0.element_size()
    cams = (_lib.MapCamera * len(frames))()
    for cam, s4, m in zip(cams, frames, warp_maps):
        _fill_map_camera(cam, m, s4)
    _set_gain_words(cams, words)
    d4 = _pixel_dst(out, s0.dtype, s0.device, B, dh, dw, C, zeroed=border_mode == BORDER_TRANSPARENT)
    bv = _border(border_value, C) if border_mode == BORDER_CONSTANT else None
    _lib.launch("bevwarp_stitch_maps", s0.device, ctypes.addressof(cams), len(frames), d4.data_ptr(), B, dh, dw, C, d4.stride(0) * esz, d4.stride(1) * esz,
                _DTYPES[s0.dtype], interp, _BLENDS[blend] | gain_flag, int(feather) if blend == "feather" else 0, border_mode, _ptr(bv))  # ("over" ignores feather)
    return _like_src(d4, srcs[0].dim(), out)


def remap_stitch_nv12(ys, uvs, warp_maps, blend="over", feather=64, border_value=None, out=None, border_mode=BORDER_CONSTANT, rgb=False, gains=None):
    """remap_stitch of the decoders' NV12 frames, converted on the way: bit for bit

        remap_stitch([cvtColor(nv12_k, COLOR_YUV2BGR_NV12) ...], warp_maps, blend, feather, border_value, ...)   (rgb=True: COLOR_YUV2RGB_NV12)

    in one launch, without the converted frames (include/bevwarp.h, bevwarp_stitch_maps_nv12); every tap is converted before the blend.

    ys, uvs    sequences of 1..8 planes each, per camera as remap_nv12 takes them: (H_k, W_k) / (B, H_k, W_k) and (H_k / 2, W_k / 2, 2) /
               (B, H_k / 2, W_k / 2, 2) uint8 CUDA tensors, even sides; split_nv12's views and row-padded planes are taken as they are.
               One B and one device.
    warp_maps, blend, feather, border_mode, out   as remap_stitch.
    border_value   (BORDER_CONSTANT only) a scalar or 3 values in the RESULT's channel order, not converted; None = 0.
    gains      as remap_stitch, applied to every CONVERTED tap: channel c is channel c of the result (B, G, R; rgb=True: R, G, B).
    Returns (B, h, w, 3), or (h, w, 3) for single frames, or `out`.  Asynchronous on the current stream."""
    ys, uvs, warp_maps = list(ys), list(uvs), list(warp_maps)
    interp, (dw, dh), border_mode = _stitch_maps_call("remap_stitch_nv12", len(ys), warp_maps, blend, feather, border_mode)
    gain_flag, words = _stitch_gains("remap_stitch_nv12", gains, len(ys))
    planes, cams, B, device = _nv12_map_cameras("remap_stitch_nv12", ys, uvs, warp_maps)
    _set_gain_words(cams, words)
    _stitch_maps_dst(out, ys[0].dim() + 1, B, dh, dw, 3)
    d4 = _pixel_dst(out, torch.uint8, device, B, dh, dw, 3, zeroed=border_mode == BORDER_TRANSPARENT)
    bv = _border(border_value, 3) if border_mode == BORDER_CONSTANT else None
    _lib.launch("bevwarp_stitch_maps_nv12", device, ctypes.addressof(cams), len(planes), d4.data_ptr(), B, dh, dw, d4.stride(0), d4.stride(1), interp,
                _BLENDS[blend] | gain_flag, int(feather) if blend == "feather" else 0, 1 if rgb else 0, border_mode, _ptr(bv))
    return _like_src(d4, ys[0].dim() + 1, out)


def _plane_format(who, flags, out_dtype, out):
    """The interpolation of a call that writes channel planes, once its flags, plane type and `out` are what the plane kernels take."""
    interp = _interp(who, flags)  # (no bicubic kernel writes planes)
    if out_dtype not in _PLANE_DTYPES:
        raise ValueError("unsupported out_dtype %s (%s: torch.float32, torch.float16, torch.bfloat16)" % (out_dtype, who))
    if out is not None and getattr(out, "dtype", None) != out_dtype:
        raise ValueError("out must be a %s tensor (out_dtype), got %s" % (out_dtype, getattr(out, "dtype", type(out))))
    return interp


def _plane_dst(out, out_dtype, device, B, C, dh, dw):
    """The (B, C, dh, dw) destination of a call that writes channel planes: a new tensor, or the caller's `out` as it is."""
    if out is None:
        return torch.empty((B, C, dh, dw), dtype=out_dtype, device=device)
    _check_out(out, out_dtype, device, B * C * dh * dw)
    d4 = out.reshape(B, C, dh, dw)
    if d4.data_ptr() != out.data_ptr() or d4.stride(3) != 1:
        raise ValueError("out must be a %s (B, C, h, w) tensor with contiguous rows" % (out_dtype,))
    return d4


def warp_to_planar(src, M, dsize, scale=1.0 / 255.0, bias=0.0, flags=INTER_LINEAR, border_value=None, out=None, M_inv_device=None,
                   out_dtype=torch.float32):
    """Warp uint8 (or float32) frames and write them as normalised channel planes in the same pass (SURVEY.md 8(f2):
    the layout a detector takes, `(B, C, v_size, u_size)`), without materialising the interleaved BEV frame:

        out[b, c] = warp_perspective(src, M, dsize)[b, :, :, c].float() * scale[c] + bias[c]      (float32 mul, then add)

    src (B, H, W, C) / (H, W, C) / (H, W) uint8 or float32 CUDA tensor; scale / bias scalars or per-channel sequences (e.g.
    1 / (255 * std) and -mean / std); other arguments as warp_perspective.
    out_dtype  torch.float32 (default), torch.float16 or torch.bfloat16: the planes' element type.  The 16-bit types hold the float32
               value above rounded to nearest, ties to even -- bit for bit what `warp_to_planar(...).half()` / `.bfloat16()` gives (NaN
               payloads aside), without the conversion pass and with half the bytes stored (include/bevwarp.h, bevwarp_warp_planes).
               A given `out` must have this dtype.
    Returns (B, C, h, w), or (C, h, w) for a single frame.  Asynchronous on the current stream."""
    interp = _plane_format("warp_to_planar", flags, out_dtype, out)
    s4, _ = _frames("warp_to_planar", src, _DTYPES)
    B, H, W, C = s4.shape
    dw, dh = int(dsize[0]), int(dsize[1])
    M_inv_device, n_m = _matrices(M, flags, M_inv_device, s4.device, B)
    d4 = _plane_dst(out, out_dtype, s4.device, B, C, dh, dw)
    sc, bi, bv = _per_channel(scale, C), _per_channel(bias, C), _border(border_value, C)
    esz, desz = s4.element_size(), d4.element_size()
    args = (s4.data_ptr(), d4.data_ptr(), B, H, W, dh, dw, C, s4.stride(0) * esz, s4.stride(1) * esz, d4.stride(0) * desz, d4.stride(1) * desz,
            d4.stride(2) * desz, M_inv_device.data_ptr(), n_m, _DTYPES[s4.dtype], interp, _ptr(bv), _ptr(sc), _ptr(bi))
    if out_dtype == torch.float32:
        _lib.launch("bevwarp_warp_planar", s4.device, *args)
    else:  # float16 / bfloat16 planes: the kernels that convert on the way out
        _lib.launch("bevwarp_warp_planes", s4.device, *args, _PLANE_DTYPES[out_dtype])
    return _like_src(d4, max(src.dim(), 3), out)  # (the planes of an (H, W) source keep their channel axis)


def split_nv12(frame):
    """(y, uv) views, without a copy, of NV12 frames held in one buffer: a `(H * 3 / 2, W)` or `(B, H * 3 / 2, W)` uint8 tensor (torch, any
    device; rows contiguous) whose first H rows are the Y plane and whose last H / 2 rows are the interleaved (U, V) pairs.  y is
    `(H, W)` / `(B, H, W)`, uv is `(H / 2, W / 2, 2)` / `(B, H / 2, W / 2, 2)`: what warp_perspective_nv12 takes."""
    if not isinstance(frame, torch.Tensor) or frame.dtype != torch.uint8 or frame.dim() not in (2, 3):
        raise ValueError("split_nv12 needs a uint8 tensor (H * 3 / 2, W) or (B, H * 3 / 2, W)")
    rows, W = int(frame.shape[-2]), int(frame.shape[-1])
    if rows <= 0 or W <= 0 or rows % 3 or W % 2:
        raise ValueError("split_nv12: %d rows x %d bytes is no NV12 frame (rows = H * 3 / 2 with H and W even)" % (rows, W))
    if frame.stride(-1) != 1:
        raise ValueError("split_nv12: the rows must be contiguous")
    H = rows // 3 * 2
    y = frame[..., :H, :]
    c = frame[..., H:, :]
    uv = torch.as_strided(c, tuple(c.shape[:-1]) + (W // 2, 2), tuple(c.stride()[:-1]) + (2, 1), c.storage_offset())
    return y, uv


def _nv12_planes(who, y, uv):
    """The planes of an NV12 call as the ABI reads them: (y3, uv4), (B, H, W) and (B, H / 2, W / 2, 2) views, strides passed through."""
    for name, t in (("y", y), ("uv", uv)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8:
            raise ValueError("%s needs uint8 CUDA (HIP) tensors; %s is %s" % (who, name, getattr(t, "dtype", type(t))))
    if y.dim() not in (2, 3) or uv.dim() != y.dim() + 1 or uv.device != y.device:
        raise ValueError("y must be (H, W) or (B, H, W) and uv (H/2, W/2, 2) or (B, H/2, W/2, 2) on the same device")
    y3, uv4 = (y[None], uv[None]) if y.dim() == 2 else (y, uv)
    B, H, W = y3.shape
    if H % 2 or W % 2 or tuple(uv4.shape) != (B, H // 2, W // 2, 2):
        raise ValueError("NV12 needs even sides and uv of shape %s; got y %s, uv %s" % ((B, H // 2, W // 2, 2), tuple(y3.shape), tuple(uv4.shape)))
    if y3.stride(2) != 1 or uv4.stride(3) != 1 or uv4.stride(2) != 2:
        raise ValueError("the last dimension of y and of uv (pairs, and the pairs of a row) must be contiguous")
    return y3, uv4


def _nv12_source(who, y, uv, M, flags, M_inv_device):
    """_nv12_planes and the call's matrices: (y3, uv4, M_inv_device, number of matrices)."""
    y3, uv4 = _nv12_planes(who, y, uv)
    return (y3, uv4) + _matrices(M, flags, M_inv_device, y3.device, y3.shape[0])


def warp_perspective_nv12(y, uv, M, dsize, flags=INTER_LINEAR, border_value=None, out=None, M_inv_device=None, rgb=False):
    """warp_perspective of a video decoder's NV12 frames, converted on the way: bit for bit

        warp_perspective(cvtColor(nv12, COLOR_YUV2BGR_NV12), M, dsize, flags, border_value)       (rgb=True: COLOR_YUV2RGB_NV12)

    in one pass, without the converted frame (include/bevwarp.h, bevwarp_warp_nv12: OpenCV's 8-bit BT.601 limited-range fixed point,
    restated from memory, parity unpinned).

    y        (H, W) or (B, H, W) uint8 CUDA tensor, H and W even.
    uv       (H / 2, W / 2, 2) or (B, H / 2, W / 2, 2) uint8 CUDA tensor of (U, V) pairs on the same device.  The last dimension of
             each must be contiguous (for uv: the pairs and the row of pairs); the other strides are passed through, so the views of
             split_nv12 and row-padded planes are taken as they are.  The uv base and strides must be even.
    M, dsize, out, M_inv_device   as warp_perspective; flags INTER_LINEAR (default) or INTER_NEAREST, optionally | WARP_INVERSE_MAP.
    border_value   scalar or 3 values in the RESULT's channel order (not converted); BORDER_CONSTANT is the only border.
    Returns (B, h, w, 3), or (h, w, 3) for a single frame.  Asynchronous on the current stream.  No verdict tables, no plan cache."""
    interp = _interp("warp_perspective_nv12", flags)
    y3, uv4, M_inv_device, n_m = _nv12_source("warp_perspective_nv12", y, uv, M, flags, M_inv_device)
    B, H, W = y3.shape
    dw, dh = int(dsize[0]), int(dsize[1])
    d4 = _pixel_dst(out, torch.uint8, y3.device, B, dh, dw, 3)
    _lib.launch("bevwarp_warp_nv12", y3.device, y3.data_ptr(), uv4.data_ptr(), d4.data_ptr(), B, H, W, dh, dw, y3.stride(0), y3.stride(1), uv4.stride(0),
                uv4.stride(1), d4.stride(0), d4.stride(1), M_inv_device.data_ptr(), n_m, interp, 1 if rgb else 0, _ptr(_border(border_value, 3)))
    return _like_src(d4, y.dim() + 1, out)


def warp_nv12_to_planar(y, uv, M, dsize, scale=1.0 / 255.0, bias=0.0, flags=INTER_LINEAR, border_value=None, out=None, M_inv_device=None,
                        rgb=False, out_dtype=torch.float32):
    """A video decoder's NV12 frames warped straight to the normalised channel planes a detector takes, in one launch: bit for bit

        warp_to_planar(warp_perspective_nv12(y, uv, M, dsize, flags, border_value, rgb=rgb), identity, dsize, scale, bias,
                       flags=INTER_NEAREST, out_dtype=out_dtype)

    without the 8-bit BEV frame in between (include/bevwarp.h, bevwarp_warp_nv12_planes):

        out[b, c] = convert(float32(warp_perspective_nv12(...)[b, :, :, c]) * scale[c] + bias[c])      (float32 mul, then add, then out_dtype)

    y, uv, M, flags, M_inv_device, rgb   as warp_perspective_nv12 (strided planes are passed through; split_nv12's views are taken as they are).
    scale, bias, border_value   scalars or 3 values in the RESULT's channel order (B, G, R; rgb=True: R, G, B).
    out_dtype, out   as warp_to_planar: torch.float32 (default), torch.float16 or torch.bfloat16; a given `out` has this dtype and
                     contiguous rows, and is returned as it is.
    Returns (B, 3, h, w), or (3, h, w) for a single frame.  Asynchronous on the current stream.  No verdict tables, no plan cache.
    FramePipeline(src_format="nv12", planar=True) keeps refusing: a streaming caller calls this function with `out=` and `M_inv_device=`
    on a stream of its own."""
    interp = _plane_format("warp_nv12_to_planar", flags, out_dtype, out)
    y3, uv4, M_inv_device, n_m = _nv12_source("warp_nv12_to_planar", y, uv, M, flags, M_inv_device)
    B, H, W = y3.shape
    dw, dh = int(dsize[0]), int(dsize[1])
    d4 = _plane_dst(out, out_dtype, y3.device, B, 3, dh, dw)
    sc, bi, bv = _per_channel(scale, 3), _per_channel(bias, 3), _border(border_value, 3)
    esz = d4.element_size()
    _lib.launch("bevwarp_warp_nv12_planes", y3.device, y3.data_ptr(), uv4.data_ptr(), d4.data_ptr(), B, H, W, dh, dw, y3.stride(0), y3.stride(1),
                uv4.stride(0), uv4.stride(1), d4.stride(0) * esz, d4.stride(1) * esz, d4.stride(2) * esz, M_inv_device.data_ptr(), n_m, interp,
                1 if rgb else 0, _ptr(bv), _ptr(sc), _ptr(bi), _PLANE_DTYPES[out_dtype])
    return _like_src(d4, y.dim() + 1, out)


def remap_nv12(y, uv, warp_map, border_mode=BORDER_CONSTANT, border_value=None, out=None, rgb=False):
    """remap of a video decoder's NV12 frames, converted on the way: bit for bit

        remap(cvtColor(nv12, COLOR_YUV2BGR_NV12), warp_map, border_mode, border_value)       (rgb=True: COLOR_YUV2RGB_NV12)

    in one pass, without the converted frame (include/bevwarp.h, bevwarp_remap_nv12).  The per-frame half of a fixed camera's loop for
    frames that come from a decoder: the map carries the lens (build_warp_map), no coordinate is computed, no float64 is touched.

    y, uv    as warp_perspective_nv12: (H, W) / (B, H, W) and (H / 2, W / 2, 2) / (B, H / 2, W / 2, 2) uint8 CUDA tensors, H and W even;
             split_nv12's views and row-padded planes are taken as they are (strides passed through; uv base and strides even).
    warp_map a WarpMap on the frames' device with n == 1 (shared by all frames) or n == B; its interpolation is the call's.
    border_mode   any of the six BORDER_* modes; the index remap applies to the pixel index (luma and chroma follow it together).
    border_value  (BORDER_CONSTANT only) a scalar or 3 values in the RESULT's channel order, not converted; None = 0.
    out      as remap: BORDER_TRANSPARENT without `out` starts from zeros.
    Returns (B, h, w, 3), or (h, w, 3) for a single frame, or `out`.  Asynchronous on the current stream.  FramePipeline(warp_map=...,
    src_format="nv12") prepares this launch for every slot; a caller with a loop of its own calls this function with `out=` on a
    stream of its own."""
    border_mode = _map_call("remap_nv12", warp_map, border_mode)
    y3, uv4 = _nv12_planes("remap_nv12", y, uv)
    B, H, W = y3.shape
    dw, dh = warp_map.dsize
    _map_fits(warp_map, B, y3.device)
    if isinstance(out, torch.Tensor) and out.dim() == y.dim() + 1 and tuple(out.shape[-3:-1]) != (dh, dw):  # (remap's rule: an `out` of the result's rank names a size)
        raise ValueError("the map's dsize is %s, out is %s" % ((dw, dh), tuple(out.shape)))
    if isinstance(out, torch.Tensor) and out.numel() != B * dh * dw * 3:
        raise ValueError("the map's dsize is %s (%d frames of 3 channels): out has %d elements" % ((dw, dh), B, out.numel()))
    d4 = _pixel_dst(out, torch.uint8, y3.device, B, dh, dw, 3, zeroed=border_mode == BORDER_TRANSPARENT)
    bv = _border(border_value, 3) if border_mode == BORDER_CONSTANT else None
    xy_p, fr_p, xy_fs, xy_rs, fr_fs, fr_rs = warp_map._planes()
    _lib.launch("bevwarp_remap_nv12", y3.device, y3.data_ptr(), uv4.data_ptr(), d4.data_ptr(), B, H, W, dh, dw, y3.stride(0), y3.stride(1), uv4.stride(0),
                uv4.stride(1), d4.stride(0), d4.stride(1), xy_p, fr_p, warp_map.n, xy_fs, xy_rs, fr_fs, fr_rs, warp_map.interp, border_mode, 1 if rgb else 0,
                _ptr(bv))
    return _like_src(d4, y.dim() + 1, out)


def remap_nv12_to_planar(y, uv, warp_map, scale=1.0 / 255.0, bias=0.0, border_mode=BORDER_CONSTANT, border_value=None, out=None, rgb=False,
                         out_dtype=torch.float32):
    """A decoder's NV12 frames sampled through a fixed camera's map straight into the normalised channel planes a detector takes, in one
    launch (include/bevwarp.h, bevwarp_remap_nv12_planes): bit for bit

        out[b, c] = convert(float32(remap_nv12(y, uv, warp_map, border_mode, border_value, rgb=rgb)[b, :, :, c]) * scale[c] + bias[c])

    (float32 mul, then add, then out_dtype) -- warp_nv12_to_planar's plane stage -- without the 8-bit BEV frame in between.

    y, uv, warp_map, rgb   as remap_nv12.
    border_mode   BORDER_CONSTANT, _REPLICATE, _REFLECT, _WRAP or _REFLECT_101; BORDER_TRANSPARENT is refused (planes hold no canvas).
    scale, bias, border_value   scalars or 3 values in the RESULT's channel order (B, G, R; rgb=True: R, G, B).
    out_dtype, out   as warp_nv12_to_planar: torch.float32 (default), torch.float16 or torch.bfloat16; a given `out` has this dtype and
                     contiguous rows, and is returned as it is.
    Returns (B, 3, h, w), or (3, h, w) for a single frame.  Asynchronous on the current stream.  FramePipeline(warp_map=...,
    planar=True) keeps refusing: a streaming caller calls this function with `out=` on a stream of its own."""
    border_mode = _map_call("remap_nv12_to_planar", warp_map, border_mode)
    if border_mode == BORDER_TRANSPARENT:
        raise ValueError("remap_nv12_to_planar: BORDER_TRANSPARENT writes no planes (remap_nv12 into a canvas, then warp_to_planar)")
    _plane_format("remap_nv12_to_planar", warp_map.interp, out_dtype, out)
    y3, uv4 = _nv12_planes("remap_nv12_to_planar", y, uv)
    B, H, W = y3.shape
    dw, dh = warp_map.dsize
    _map_fits(warp_map, B, y3.device)
    if isinstance(out, torch.Tensor) and out.dim() == y.dim() + 1 and tuple(out.shape[-2:]) != (dh, dw):
        raise ValueError("the map's dsize is %s, out is %s" % ((dw, dh), tuple(out.shape)))
    d4 = _plane_dst(out, out_dtype, y3.device, B, 3, dh, dw)
    sc, bi = _per_channel(scale, 3), _per_channel(bias, 3)
    bv = _border(border_value, 3) if border_mode == BORDER_CONSTANT else None
    esz = d4.element_size()
    xy_p, fr_p, xy_fs, xy_rs, fr_fs, fr_rs = warp_map._planes()
    _lib.launch("bevwarp_remap_nv12_planes", y3.device, y3.data_ptr(), uv4.data_ptr(), d4.data_ptr(), B, H, W, dh, dw, y3.stride(0), y3.stride(1),
                uv4.stride(0), uv4.stride(1), d4.stride(0) * esz, d4.stride(1) * esz, d4.stride(2) * esz, xy_p, fr_p, warp_map.n, xy_fs, xy_rs, fr_fs, fr_rs,
                warp_map.interp, border_mode, 1 if rgb else 0, _ptr(bv), _ptr(sc), _ptr(bi), _PLANE_DTYPES[out_dtype])
    return _like_src(d4, y.dim() + 1, out)


def _nv12_out_format(who, flags, dsize):
    """What the warps into NV12 check before they look at a tensor: (interp, dw, dh)."""
    interp = _interp(who, flags)
    dw, dh = int(dsize[0]), int(dsize[1])
    if dw <= 0 or dh <= 0 or dw % 2 or dh % 2:
        raise ValueError("%s: an NV12 frame has even sides, got dsize %s" % (who, (dw, dh)))
    return interp, dw, dh


def _nv12_dst(who, out, device, B, dh, dw, single):
    """The destination planes of a warp into NV12 as the ABI writes them -- (B, dh, dw) and (B, dh / 2, dw / 2, 2) views, strides passed
    through -- and what the call returns: `out` itself, or a new joined (dh * 3 / 2, dw) / (B, dh * 3 / 2, dw) buffer."""
    if out is None:
        out = torch.empty((dh * 3 // 2, dw) if single else (B, dh * 3 // 2, dw), dtype=torch.uint8, device=device)
        y, uv = split_nv12(out)
    elif isinstance(out, (tuple, list)):
        if len(out) != 2:
            raise ValueError("%s: out is a joined (dh * 3 / 2, dw) buffer or a (y, uv) pair" % who)
        y, uv = out
    else:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.dim() not in (2, 3) or tuple(out.shape[-2:]) != (dh * 3 // 2, dw):
            raise ValueError("%s: a joined out must be a uint8 tensor (..., %d, %d)" % (who, dh * 3 // 2, dw))
        y, uv = split_nv12(out)
    for name, t in (("y", y), ("uv", uv)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.device != device:
            raise ValueError("%s: the %s plane of out must be a uint8 tensor on %s" % (who, name, device))
    if y.dim() not in (2, 3) or uv.dim() != y.dim() + 1:
        raise ValueError("%s: out planes must be y (dh, dw) or (B, dh, dw) and uv (dh/2, dw/2, 2) or (B, dh/2, dw/2, 2)" % who)
    y3, uv4 = (y[None], uv[None]) if y.dim() == 2 else (y, uv)
    if tuple(y3.shape) != (B, dh, dw) or tuple(uv4.shape) != (B, dh // 2, dw // 2, 2):
        raise ValueError("%s: out planes must be %s and %s; got y %s, uv %s" % (who, (B, dh, dw), (B, dh // 2, dw // 2, 2), tuple(y3.shape), tuple(uv4.shape)))
    if y3.stride(2) != 1 or uv4.stride(3) != 1 or uv4.stride(2) != 2:
        raise ValueError("%s: the last dimension of out's y and of its uv (pairs, and the pairs of a row) must be contiguous" % who)
    return y3, uv4, out


def warp_perspective_to_nv12(src, M, dsize, flags=INTER_LINEAR, border_value=None, out=None, M_inv_device=None, rgb=False):
    """warp_perspective of 8-bit BGR frames, written as the NV12 frame a video encoder takes: bit for bit

        BGR->NV12(warp_perspective(src, M, dsize, flags, border_value))               (rgb=True: the frames are R, G, B)

    in one pass, without the warped BGR frame (include/bevwarp.h, bevwarp_warp_to_nv12: OpenCV's 8-bit BT.601 limited-range RGB -> YUV 4:2:0
    fixed point, restated from memory, parity unpinned; a (U, V) pair is that of its 2 x 2 block's top-left pixel, nothing is averaged).

    src      (B, H, W, 3) or (H, W, 3) uint8 CUDA tensor, channels-last, rows contiguous.
    M, M_inv_device   as warp_perspective; flags INTER_LINEAR (default) or INTER_NEAREST, optionally | WARP_INVERSE_MAP.
    dsize    (width, height), both even.
    border_value   scalar or 3 values in the SOURCE's channel order: a pixel, converted like any other ((0, 0, 0) gives (16, 128, 128)).
    out      a joined uint8 buffer (dh * 3 / 2, dw) or (B, dh * 3 / 2, dw) -- the Y rows, then the rows of (U, V) pairs; split with
             split_nv12 -- or a (y, uv) pair of planes, (B, dh, dw) and (B, dh / 2, dw / 2, 2), whose strides are passed through (the uv
             base and strides must be even): exactly what warp_perspective_nv12 takes as its source.
    Returns `out` if given, otherwise a new joined buffer.  Asynchronous on the current stream.  No verdict tables, no plan cache."""
    interp, dw, dh = _nv12_out_format("warp_perspective_to_nv12", flags, dsize)
    if not isinstance(src, torch.Tensor) or not src.is_cuda or src.dtype != torch.uint8:
        raise ValueError("warp_perspective_to_nv12 needs a uint8 CUDA (HIP) tensor; src is %s" % (getattr(src, "dtype", type(src)),))
    s4, _ = _frames("warp_perspective_to_nv12", src, None, channels=3)
    B, H, W, _ = s4.shape
    M_inv_device, n_m = _matrices(M, flags, M_inv_device, s4.device, B)
    y3, uv4, ret = _nv12_dst("warp_perspective_to_nv12", out, s4.device, B, dh, dw, src.dim() == 3)
    _lib.launch("bevwarp_warp_to_nv12", s4.device, s4.data_ptr(), y3.data_ptr(), uv4.data_ptr(), B, H, W, dh, dw, s4.stride(0), s4.stride(1), y3.stride(0),
                y3.stride(1), uv4.stride(0), uv4.stride(1), M_inv_device.data_ptr(), n_m, interp, 1 if rgb else 0, _ptr(_border(border_value, 3)))
    return ret


def warp_nv12_to_nv12(y, uv, M, dsize, flags=INTER_LINEAR, border_value=None, out=None, M_inv_device=None):
    """A video decoder's NV12 frames warped straight to the NV12 frames a video encoder takes, in one launch: bit for bit

        BGR->NV12(warp_perspective_nv12(y, uv, M, dsize, flags, border_value))

    with no BGR frame in memory on either side (include/bevwarp.h, bevwarp_warp_nv12_to_nv12).  This is not a warp of the Y and UV planes:
    every tap is converted to BGR, blended there, and the blended pixel converted back.

    y, uv, M, flags, M_inv_device   as warp_perspective_nv12.  dsize (width, height), both even.
    border_value   scalar or 3 values in B, G, R order: a pixel, converted like any other.
    out      as warp_perspective_to_nv12: a joined buffer or a (y, uv) pair.
    Returns `out` if given, otherwise a new joined buffer.  Asynchronous on the current stream.  No verdict tables, no plan cache."""
    interp, dw, dh = _nv12_out_format("warp_nv12_to_nv12", flags, dsize)
    y3, uv4, M_inv_device, n_m = _nv12_source("warp_nv12_to_nv12", y, uv, M, flags, M_inv_device)
    B, H, W = y3.shape
    dy3, duv4, ret = _nv12_dst("warp_nv12_to_nv12", out, y3.device, B, dh, dw, y.dim() == 2)
    _lib.launch("bevwarp_warp_nv12_to_nv12", y3.device, y3.data_ptr(), uv4.data_ptr(), dy3.data_ptr(), duv4.data_ptr(), B, H, W, dh, dw, y3.stride(0),
                y3.stride(1), uv4.stride(0), uv4.stride(1), dy3.stride(0), dy3.stride(1), duv4.stride(0), duv4.stride(1), M_inv_device.data_ptr(), n_m,
                interp, _ptr(_border(border_value, 3)))
    return ret


def _map_nv12_out_call(who, warp_map, border_mode):
    """What the map samplers into NV12 check before they look at a tensor: _map_call's, a border mode that writes every pixel, and a
    map whose dsize is an NV12 frame's.  Returns the border mode as an int."""
    border_mode = _map_call(who, warp_map, border_mode)
    if border_mode == BORDER_TRANSPARENT:
        raise ValueError("%s: BORDER_TRANSPARENT writes no NV12 frame (a canvas is kept as 8-bit pixels: remap into it, then warp_perspective_to_nv12)" % who)
    if warp_map.dsize[0] % 2 or warp_map.dsize[1] % 2:
        raise ValueError("%s: an NV12 frame has even sides, the map's dsize is %s" % (who, warp_map.dsize))
    return border_mode


def _bgr_frames(who, src):
    """8-bit frames of 3 channels as the entries into NV12 take them: _frames' 4-D view."""
    if not isinstance(src, torch.Tensor) or not src.is_cuda or src.dtype != torch.uint8:
        raise ValueError("%s needs a uint8 CUDA (HIP) tensor; src is %s" % (who, getattr(src, "dtype", type(src))))
    return _frames(who, src, None, channels=3)[0]


def _bgr_map_cameras(who, srcs, warp_maps):
    """The 8-bit cameras of 3 channels of a stitch through maps: every camera's frames as _bgr_frames takes them, one batch and device, a
    map that serves them per camera.  Returns (frames, cams, B, device): the filled bevwarp_map_camera array, and the tensors it points
    into -- a copy _frames made may be among them -- which the caller keeps until the launch is enqueued."""
    frames = [_bgr_frames(who, src) for src in srcs]
    B, device = frames[0].shape[0], frames[0].device
    for k, (src, s4) in enumerate(zip(srcs, frames)):
        if s4.shape[0] != B or s4.device != device or src.dim() != srcs[0].dim():
            raise ValueError("camera %d has %d frames (rank %d) on %s; camera 0 has %d (rank %d) on %s (%s: one batch and device)"
                             % (k, s4.shape[0], src.dim(), s4.device, B, srcs[0].dim(), device, who))
    for m in warp_maps:
        _map_fits(m, B, device)
    cams = (_lib.MapCamera * len(frames))()
    for cam, s4, m in zip(cams, frames, warp_maps):
        _fill_map_camera(cam, m, s4)
    return frames, cams, B, device


def remap_to_nv12(src, warp_map, border_mode=BORDER_CONSTANT, border_value=None, out=None, rgb=False):
    """remap of 8-bit BGR frames, written as the NV12 frame a video encoder takes: bit for bit

        BGR->NV12(remap(src, warp_map, border_mode, border_value))               (rgb=True: the frames are R, G, B)

    in one pass, without the BEV frame in BGR (include/bevwarp.h, bevwarp_remap_to_nv12; the conversion is warp_perspective_to_nv12's).
    The per-frame half of a fixed camera's loop whose BEV goes to an encoder: the map carries the lens (build_warp_map).

    src      (B, H, W, 3) or (H, W, 3) uint8 CUDA tensor, channels-last, rows contiguous.
    warp_map a WarpMap on src's device with n == 1 (shared by all frames) or n == B and an even dsize; its interpolation is the call's.
    border_mode   BORDER_CONSTANT, _REPLICATE, _REFLECT, _WRAP or _REFLECT_101; BORDER_TRANSPARENT is refused (NV12 holds no canvas).
    border_value  (BORDER_CONSTANT only) a scalar or 3 values in the SOURCE's channel order: a pixel, converted like any other.
    out      as warp_perspective_to_nv12: a joined (dh * 3 / 2, dw) / (B, dh * 3 / 2, dw) buffer or a (y, uv) pair, strides passed through.
    Returns `out` if given, otherwise a new joined buffer.  Asynchronous on the current stream."""
    border_mode = _map_nv12_out_call("remap_to_nv12", warp_map, border_mode)
    s4 = _bgr_frames("remap_to_nv12", src)
    B, H, W, _ = s4.shape
    dw, dh = warp_map.dsize
    _map_fits(warp_map, B, s4.device)
    y3, uv4, ret = _nv12_dst("remap_to_nv12", out, s4.device, B, dh, dw, src.dim() == 3)
    bv = _border(border_value, 3) if border_mode == BORDER_CONSTANT else None
    xy_p, fr_p, xy_fs, xy_rs, fr_fs, fr_rs = warp_map._planes()
    _lib.launch("bevwarp_remap_to_nv12", s4.device, s4.data_ptr(), y3.data_ptr(), uv4.data_ptr(), B, H, W, dh, dw, s4.stride(0), s4.stride(1), y3.stride(0),
                y3.stride(1), uv4.stride(0), uv4.stride(1), xy_p, fr_p, warp_map.n, xy_fs, xy_rs, fr_fs, fr_rs, warp_map.interp, border_mode, 1 if rgb else 0,
                _ptr(bv))
    return ret


def remap_nv12_to_nv12(y, uv, warp_map, border_mode=BORDER_CONSTANT, border_value=None, out=None):
    """A video decoder's NV12 frames sampled through a fixed camera's map straight to the NV12 frames a video encoder takes, in one
    launch: bit for bit

        BGR->NV12(remap_nv12(y, uv, warp_map, border_mode, border_value))

    with no BGR frame in memory on either side (include/bevwarp.h, bevwarp_remap_nv12_to_nv12).  Every tap is converted to BGR, blended
    there, and the blended pixel converted back.

    y, uv, warp_map   as remap_nv12; the map's dsize is even.
    border_mode, out  as remap_to_nv12.  border_value: a scalar or 3 values in B, G, R order, a pixel, converted like any other.
    Returns `out` if given, otherwise a new joined buffer.  Asynchronous on the current stream."""
    border_mode = _map_nv12_out_call("remap_nv12_to_nv12", warp_map, border_mode)
    y3, uv4 = _nv12_planes("remap_nv12_to_nv12", y, uv)
    B, H, W = y3.shape
    dw, dh = warp_map.dsize
    _map_fits(warp_map, B, y3.device)
    dy3, duv4, ret = _nv12_dst("remap_nv12_to_nv12", out, y3.device, B, dh, dw, y.dim() == 2)
    bv = _border(border_value, 3) if border_mode == BORDER_CONSTANT else None
    xy_p, fr_p, xy_fs, xy_rs, fr_fs, fr_rs = warp_map._planes()
    _lib.launch("bevwarp_remap_nv12_to_nv12", y3.device, y3.data_ptr(), uv4.data_ptr(), dy3.data_ptr(), duv4.data_ptr(), B, H, W, dh, dw, y3.stride(0), y3.stride(1),
                uv4.stride(0), uv4.stride(1), dy3.stride(0), dy3.stride(1), duv4.stride(0), duv4.stride(1), xy_p, fr_p, warp_map.n, xy_fs, xy_rs, fr_fs, fr_rs,
                warp_map.interp, border_mode, _ptr(bv))
    return ret


def _stitch_maps_nv12_out_call(who, n_cams, warp_maps, blend, feather):
    """_stitch_maps_call for the stitches into NV12 (no border mode: what no camera covers is the border pixel) with an even canvas.
    Returns (interpolation, (dw, dh))."""
    interp, (dw, dh), _ = _stitch_maps_call(who, n_cams, warp_maps, blend, feather, BORDER_CONSTANT)
    if dw % 2 or dh % 2:
        raise ValueError("%s: an NV12 frame has even sides, the maps' dsize is %s" % (who, (dw, dh)))
    return interp, (dw, dh)


def remap_stitch_to_nv12(srcs, warp_maps, blend="over", feather=64, border_value=None, out=None, rgb=False, gains=None):
    """remap_stitch of 8-bit BGR cameras, written as the NV12 frame a video encoder takes: bit for bit

        BGR->NV12(remap_stitch(srcs, warp_maps, blend, feather, border_value))               (rgb=True: the frames are R, G, B)

    in one launch, without the canvas in BGR (include/bevwarp.h, bevwarp_stitch_maps_to_nv12).

    srcs       a sequence of 1..8 uint8 CUDA tensors, each (B, H_k, W_k, 3) or (H_k, W_k, 3): one B and one device.
    warp_maps, blend, feather   as remap_stitch; the maps' dsize is even.
    border_value   a scalar or 3 values in the SOURCES' channel order: the pixel that no camera covers, converted like any other.
    out        as warp_perspective_to_nv12: a joined buffer or a (y, uv) pair.
    gains      as remap_stitch: channel c is the frames' channel c.
    Returns `out` if given, otherwise a new joined buffer.  Asynchronous on the current stream."""
    srcs, warp_maps = list(srcs), list(warp_maps)
    interp, (dw, dh) = _stitch_maps_nv12_out_call("remap_stitch_to_nv12", len(srcs), warp_maps, blend, feather)
    gain_flag, words = _stitch_gains("remap_stitch_to_nv12", gains, len(srcs))
    frames, cams, B, device = _bgr_map_cameras("remap_stitch_to_nv12", srcs, warp_maps)
    _set_gain_words(cams, words)
    y3, uv4, ret = _nv12_dst("remap_stitch_to_nv12", out, device, B, dh, dw, srcs[0].dim() == 3)
    _lib.launch("bevwarp_stitch_maps_to_nv12", device, ctypes.addressof(cams), len(frames), y3.data_ptr(), uv4.data_ptr(), B, dh, dw, y3.stride(0), y3.stride(1),
                uv4.stride(0), uv4.stride(1), interp, _BLENDS[blend] | gain_flag, int(feather) if blend == "feather" else 0, 1 if rgb else 0,
                _ptr(_border(border_value, 3)))
    return ret


def remap_stitch_nv12_to_nv12(ys, uvs, warp_maps, blend="over", feather=64, border_value=None, out=None, gains=None):
    """remap_stitch_nv12 of the decoders' NV12 frames, written as the NV12 frame a video encoder takes: bit for bit

        BGR->NV12(remap_stitch_nv12(ys, uvs, warp_maps, blend, feather, border_value))

    in one launch, with no BGR frame in memory on either side (include/bevwarp.h, bevwarp_stitch_maps_nv12_to_nv12).

    ys, uvs, warp_maps, blend, feather   as remap_stitch_nv12; the maps' dsize is even.
    border_value   a scalar or 3 values in B, G, R order: the pixel that no camera covers, converted like any other.
    out        as warp_perspective_to_nv12: a joined buffer or a (y, uv) pair.
    gains      as remap_stitch, applied to every converted tap: channel c is B, G, R.
    Returns `out` if given, otherwise a new joined buffer.  Asynchronous on the current stream."""
    ys, uvs, warp_maps = list(ys), list(uvs), list(warp_maps)
    interp, (dw, dh) = _stitch_maps_nv12_out_call("remap_stitch_nv12_to_nv12", len(ys), warp_maps, blend, feather)
    gain_flag, words = _stitch_gains("remap_stitch_nv12_to_nv12", gains, len(ys))
    planes, cams, B, device = _nv12_map_cameras("remap_stitch_nv12_to_nv12", ys, uvs, warp_maps)
    _set_gain_words(cams, words)
    dy3, duv4, ret = _nv12_dst("remap_stitch_nv12_to_nv12", out, device, B, dh, dw, ys[0].dim() == 2)
    _lib.launch("bevwarp_stitch_maps_nv12_to_nv12", device, ctypes.addressof(cams), len(planes), dy3.data_ptr(), duv4.data_ptr(), B, dh, dw, dy3.stride(0),
                dy3.stride(1), duv4.stride(0), duv4.stride(1), interp, _BLENDS[blend] | gain_flag, int(feather) if blend == "feather" else 0,
                _ptr(_border(border_value, 3)))
    return ret


def _planes_out_fits(out, ndim, dw, dh, what="map's"):
    """remap_nv12_to_planar's rule for a caller's `out` of the result's rank `ndim`: its plane size is the map's."""
    if isinstance(out, torch.Tensor) and out.dim() == ndim and tuple(out.shape[-2:]) != (dh, dw):
        raise ValueError("the %s dsize is %s, out is %s" % (what, (dw, dh), tuple(out.shape)))


def remap_to_planar(src, warp_map, scale=1.0 / 255.0, bias=0.0, border_mode=BORDER_CONSTANT, border_value=None, out=None, out_dtype=torch.float32):
    """8-bit BGR frames sampled through a fixed camera's map straight into the normalised channel planes a detector takes, in one launch
    (include/bevwarp.h, bevwarp_remap_planes): bit for bit

        out[b, c] = convert(float32(remap(src, warp_map, border_mode, border_value)[b, :, :, c]) * scale[c] + bias[c])

    (float32 mul, then add, then out_dtype) -- warp_nv12_to_planar's plane stage -- without the 8-bit BEV frame in between and without the
    second launch of remap followed by an identity warp_to_planar.

    src      (B, H, W, 3) or (H, W, 3) uint8 CUDA tensor, channels-last, rows contiguous.  Plane c is channel c: there is no channel swap.
    warp_map a WarpMap on src's device with n == 1 (shared by all frames) or n == B; its interpolation is the call's.
    border_mode   BORDER_CONSTANT, _REPLICATE, _REFLECT, _WRAP or _REFLECT_101; BORDER_TRANSPARENT is refused (planes hold no canvas).
    scale, bias, border_value   scalars or 3 values in the frames' channel order; border_value (BORDER_CONSTANT only) is an 8-bit pixel
                                that passes through the plane stage like any other.
    out_dtype, out   as warp_nv12_to_planar: torch.float32 (default), torch.float16 or torch.bfloat16; a given `out` has this dtype and
                     contiguous rows, and is returned as it is.
    Returns (B, 3, h, w), or (3, h, w) for a single frame.  Asynchronous on the current stream."""
    border_mode = _map_call("remap_to_planar", warp_map, border_mode)
    if border_mode == BORDER_TRANSPARENT:
        raise ValueError("remap_to_planar: BORDER_TRANSPARENT writes no planes (remap into a canvas, then warp_to_planar)")
    _plane_format("remap_to_planar", warp_map.interp, out_dtype, out)
    s4 = _bgr_frames("remap_to_planar", src)
    B, H, W, _ = s4.shape
    dw, dh = warp_map.dsize
    _map_fits(warp_map, B, s4.device)
    _planes_out_fits(out, src.dim(), dw, dh)
    d4 = _plane_dst(out, out_dtype, s4.device, B, 3, dh, dw)
    sc, bi = _per_channel(scale, 3), _per_channel(bias, 3)
    bv = _border(border_value, 3) if border_mode == BORDER_CONSTANT else None
    esz = d4.element_size()
    xy_p, fr_p, xy_fs, xy_rs, fr_fs, fr_rs = warp_map._planes()
    _lib.launch("bevwarp_remap_planes", s4.device, s4.data_ptr(), d4.data_ptr(), B, H, W, dh, dw, s4.stride(0), s4.stride(1), d4.stride(0) * esz, d4.stride(1) * esz,
                d4.stride(2) * esz, xy_p, fr_p, warp_map.n, xy_fs, xy_rs, fr_fs, fr_rs, warp_map.interp, border_mode, _ptr(bv), _ptr(sc), _ptr(bi),
                _PLANE_DTYPES[out_dtype])
    return _like_src(d4, src.dim(), out)


def remap_stitch_to_planar(srcs, warp_maps, scale=1.0 / 255.0, bias=0.0, blend="over", feather=64, border_value=None, out=None, out_dtype=torch.float32,
                           gains=None):
    """remap_stitch of 8-bit BGR cameras, written as the normalised channel planes a detector takes: bit for bit

        out[b, c] = convert(float32(remap_stitch(srcs, warp_maps, blend, feather, border_value)[b, :, :, c]) * scale[c] + bias[c])

    in one launch, without the 8-bit canvas (include/bevwarp.h, bevwarp_stitch_maps_planes).

    srcs       a sequence of 1..8 uint8 CUDA tensors, each (B, H_k, W_k, 3) or (H_k, W_k, 3): one B and one device.  Plane c is channel c.
    warp_maps, blend, feather   as remap_stitch.
    scale, bias, border_value   scalars or 3 values in the frames' channel order; border_value is the 8-bit pixel that no camera covers,
                                put through the plane stage like any other.  "feather" is the 8-bit integer mean, then the plane stage.
    out_dtype, out   as remap_to_planar.
    gains      as remap_stitch: channel c is the frames' channel c, plane c.
    Returns (B, 3, h, w), or (3, h, w) for single frames.  Asynchronous on the current stream."""
    srcs, warp_maps = list(srcs), list(warp_maps)
    interp, (dw, dh), _ = _stitch_maps_call("remap_stitch_to_planar", len(srcs), warp_maps, blend, feather, BORDER_CONSTANT)
    _plane_format("remap_stitch_to_planar", interp, out_dtype, out)
    gain_flag, words = _stitch_gains("remap_stitch_to_planar", gains, len(srcs))
    frames, cams, B, device = _bgr_map_cameras("remap_stitch_to_planar", srcs, warp_maps)
    _set_gain_words(cams, words)
    _planes_out_fits(out, srcs[0].dim(), dw, dh, "maps'")
    d4 = _plane_dst(out, out_dtype, device, B, 3, dh, dw)
    sc, bi = _per_channel(scale, 3), _per_channel(bias, 3)
    esz = d4.element_size()
    _lib.launch("bevwarp_stitch_maps_planes", device, ctypes.addressof(cams), len(frames), d4.data_ptr(), B, dh, dw, d4.stride(0) * esz, d4.stride(1) * esz,
                d4.stride(2) * esz, interp, _BLENDS[blend] | gain_flag, int(feather) if blend == "feather" else 0, _ptr(_border(border_value, 3)), _ptr(sc), _ptr(bi),
                _PLANE_DTYPES[out_dtype])
    return _like_src(d4, srcs[0].dim(), out)


def remap_stitch_nv12_to_planar(ys, uvs, warp_maps, scale=1.0 / 255.0, bias=0.0, blend="over", feather=64, border_value=None, out=None, rgb=False,
                                out_dtype=torch.float32, gains=None):
    """remap_stitch_nv12 of the decoders' NV12 frames, written as the normalised channel planes a detector takes: bit for bit

        out[b, c] = convert(float32(remap_stitch_nv12(ys, uvs, warp_maps, blend, feather, border_value, rgb=rgb)[b, :, :, c]) * scale[c] + bias[c])

    in one launch, with neither the converted frames nor the 8-bit canvas in memory (include/bevwarp.h, bevwarp_stitch_maps_nv12_planes).

    ys, uvs, warp_maps, blend, feather, rgb   as remap_stitch_nv12.
    scale, bias, border_value   scalars or 3 values in the RESULT's channel order (B, G, R; rgb=True: R, G, B); border_value is the 8-bit
                                pixel that no camera covers, not converted, put through the plane stage like any other.
    out_dtype, out   as remap_to_planar.
    gains      as remap_stitch, applied to every converted tap: channel c is plane c (B, G, R; rgb=True: R, G, B).
    Returns (B, 3, h, w), or (3, h, w) for single frames.  Asynchronous on the current stream."""
    ys, uvs, warp_maps = list(ys), list(uvs), list(warp_maps)
    interp, (dw, dh), _ = _stitch_maps_call("remap_stitch_nv12_to_planar", len(ys), warp_maps, blend, feather, BORDER_CONSTANT)
    _plane_format("remap_stitch_nv12_to_planar", interp, out_dtype, out)
    gain_flag, words = _stitch_gains("remap_stitch_nv12_to_planar", gains, len(ys))
    planes, cams, B, device = _nv12_map_cameras("remap_stitch_nv12_to_planar", ys, uvs, warp_maps)
    _set_gain_words(cams, words)
    _planes_out_fits(out, ys[0].dim() + 1, dw, dh, "maps'")
    d4 = _plane_dst(out, out_dtype, device, B, 3, dh, dw)
    sc, bi = _per_channel(scale, 3), _per_channel(bias, 3)
    esz = d4.element_size()
    _lib.launch("bevwarp_stitch_maps_nv12_planes", device, ctypes.addressof(cams), len(planes), d4.data_ptr(), B, dh, dw, d4.stride(0) * esz, d4.stride(1) * esz,
                d4.stride(2) * esz, interp, _BLENDS[blend] | gain_flag, int(feather) if blend == "feather" else 0, 1 if rgb else 0, _ptr(_border(border_value, 3)), _ptr(sc),
                _ptr(bi), _PLANE_DTYPES[out_dtype])
    return _like_src(d4, ys[0].dim() + 1, out)


def footprint(src_hw, M, dsize, batch=None, flags=INTER_LINEAR, device="cuda"):
    """Exact count of distinct in-bounds source pixels the warp reads, per frame.
    Returns (counts int64 tensor [n], touched uint8 tensor [n, H, W])."""
    H, W = int(src_hw[0]), int(src_hw[1])
    minv = device_inverse(M, torch.device(device), inverse_given=bool(int(flags) & WARP_INVERSE_MAP))
    n = minv.shape[0] if batch is None else int(batch)
    touched = torch.zeros((n, H, W), dtype=torch.uint8, device=minv.device)
    _lib.launch("bevwarp_footprint", minv.device, touched.data_ptr(), n, H, W, int(dsize[1]), int(dsize[0]), minv.data_ptr(), minv.shape[0], int(flags) & 7)
    return touched.reshape(n, -1).sum(dim=1, dtype=torch.int64), touched


def scalar_border(borderValue, channels):
    """cv2 turns `borderValue` into a cv::Scalar: a bare number v means (v, 0, 0, 0) -- channel 0 only -- and a sequence
    fills the leading channels, the rest stay 0."""
    v = np.atleast_1d(np.asarray(borderValue, dtype=np.float64)).ravel()[:4]
    out = np.zeros(channels, dtype=np.float64)
    out[:min(len(v), channels)] = v[:channels]
    return out


def warpPerspective(src, M, dsize, dst=None, flags=INTER_LINEAR, borderMode=BORDER_CONSTANT, borderValue=0, device="cuda"):
    """cv2.warpPerspective call shape for numpy images: uploads, warps on the GPU, downloads.
    (The per-frame PCIe round trip dominates here; batch frames with warp_perspective for throughput.)
    flags: INTER_LINEAR, INTER_NEAREST or INTER_CUBIC, optionally | WARP_INVERSE_MAP.
    borderMode: any of the six BORDER_* modes above.  With BORDER_TRANSPARENT a given `dst` is the canvas: it is uploaded, the
    pixels the source covers are written into it and it is returned (several cameras stitched into one image, one call each);
    without one, uncovered pixels are 0."""
    if borderMode not in _BORDER_MODES:
        raise ValueError("unsupported borderMode %r (BORDER_CONSTANT, _REPLICATE, _REFLECT, _WRAP, _REFLECT_101, _TRANSPARENT)" % (borderMode,))
    img = np.asarray(src)
    if img.dtype not in (np.uint8, np.float32):
        raise ValueError("unsupported dtype %s (uint8 / float32)" % img.dtype)
    dw, dh = int(dsize[0]), int(dsize[1])
    shape = (dh, dw) + tuple(img.shape[2:])
    canvas = None
    if borderMode == BORDER_TRANSPARENT and dst is not None:
        if not isinstance(dst, np.ndarray) or dst.shape != shape or dst.dtype != img.dtype:
            raise ValueError("dst must be a %s array of shape %s (the canvas BORDER_TRANSPARENT writes into)" % (img.dtype, shape))
        canvas = torch.from_numpy(np.ascontiguousarray(dst)).to(device)
    t = torch.from_numpy(np.ascontiguousarray(img)).to(device)
    bv = scalar_border(borderValue, 1 if img.ndim == 2 else img.shape[2])
    res = warp_perspective(t, np.asarray(M, dtype=np.float64), dsize, flags=flags, border_value=bv, out=canvas, border_mode=borderMode).cpu().numpy()
    if dst is not None:
        dst[...] = res
        return dst
    return res


def resize_matrix(src_wh, new_wh, align_corners=False):
    """3x3 map from pixels of a (w, h) image to pixels of its resized (new_w, new_h) version, in the convention of
    the reference's Calib.scale (bev/calib.py:142-198): x' = (x + 0.5) * r - 0.5 (align_corners=False, what
    cv2.resize does) or x' = x * (new - 1) / (old - 1)."""
    (w, h), (nw, nh) = src_wh, new_wh
    if align_corners:
        ru, rv = (nw - 1) / (w - 1), (nh - 1) / (h - 1)
        return np.array([[ru, 0, 0], [0, rv, 0], [0, 0, 1.0]])
    ru, rv = nw / w, nh / h
    return np.array([[ru, 0, 0.5 * ru - 0.5], [0, rv, 0.5 * rv - 0.5], [0, 0, 1.0]])


def warp_perspective_resized(src, M_resized, dsize, new_wh, align_corners=False, **kw):
    """The "small" branch of vis_homo.py:73-78,90-91 -- cv2.resize(img, new_wh) followed by
    cv2.warpPerspective(img_small, H_bev_img_small, dsize) -- with the resize folded into the homography: the
    full-resolution frame is sampled once through M_resized @ resize_matrix(...), no intermediate image exists.
    `M_resized` maps pixels of the RESIZED image to the destination (H_bev_img_small).  The result is the warp of the
    full-resolution frame (sharper than the two-step path, which low-passes through the resize); it is bit-identical
    to warp_perspective(src, M_resized @ S, dsize).  Keyword arguments as for warp_perspective."""
    h, w = (src.shape[-3], src.shape[-2]) if src.dim() >= 3 else src.shape
    S = resize_matrix((w, h), new_wh, align_corners)
    return warp_perspective(src, np.asarray(M_resized, dtype=np.float64) @ S, dsize, **kw)

