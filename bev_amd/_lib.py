"""ctypes binding of bev_amd/csrc/libbevwarp.so (C ABI: include/bevwarp.h).

There is no CPU fallback: if the shared library is missing or a call fails, this raises.
`build()` compiles the library in-tree with hipcc for gfx950 (cross-compiles without a GPU).
"""
import ctypes
import os
import subprocess

import torch

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB_PATH = os.environ.get("BEVWARP_LIB") or os.path.join(_CSRC, "libbevwarp.so")  # override = A/B builds

U8, F32, F64, F16, BF16 = 0, 1, 2, 3, 4  # (F16, BF16: plane types of the entries that write channel planes only)
INTER_NEAREST, INTER_LINEAR, INTER_CUBIC = 0, 1, 2
ABI_VERSION = 7

# every symbol include/bevwarp.h declares: (name, restype, argtypes)
_c = ctypes
SYMBOLS = {
    "bevwarp_version": (_c.c_int, []),
    "bevwarp_strerror": (_c.c_char_p, [_c.c_int]),
    "bevwarp_last_hip_error": (_c.c_char_p, []),
    "bevwarp_invert_homography": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int]),
    "bevwarp_warp": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                _c.c_void_p, _c.c_void_p]),
    "bevwarp_warp_border": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                       _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                       _c.c_int, _c.c_void_p, _c.c_void_p]),
    "bevwarp_warp_lens": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                     _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_double,
                                     _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "bevwarp_build_map": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_double, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int64, _c.c_int64,
                                     _c.c_int64, _c.c_int64, _c.c_void_p]),
    "bevwarp_remap": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64,
                                 _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                 _c.c_void_p]),
    "bevwarp_warp_stitch": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int64, _c.c_int64, _c.c_int, _c.c_int,
                                       _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "bevwarp_stitch_maps": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int64, _c.c_int64, _c.c_int, _c.c_int,
                                       _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "bevwarp_stitch_maps_nv12": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int64, _c.c_int64, _c.c_int, _c.c_int, _c.c_int,
                                            _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "bevwarp_warp_classes": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                        _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                        _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p]),
    "bevwarp_tile_classes_bytes": (_c.c_int64, [_c.c_int] * 8),
    "bevwarp_warp_planar": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                       _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                       _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "bevwarp_warp_planes": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                       _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                       _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p]),
    "bevwarp_warp_nv12": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                     _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                     _c.c_void_p, _c.c_void_p]),
    "bevwarp_warp_nv12_planes": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                            _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_int, _c.c_int,
                                            _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p]),
    "bevwarp_remap_nv12": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                      _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_int,
                                      _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "bevwarp_remap_nv12_planes": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                             _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_void_p,
                                             _c.c_int, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                             _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p]),
    "bevwarp_warp_to_nv12": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                        _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                        _c.c_void_p, _c.c_void_p]),
    "bevwarp_warp_nv12_to_nv12": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                             _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_void_p,
                                             _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "bevwarp_remap_to_nv12": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                         _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_int,
                                         _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "bevwarp_remap_nv12_to_nv12": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                              _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_void_p,
                                              _c.c_void_p, _c.c_int, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "bevwarp_stitch_maps_to_nv12": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int64, _c.c_int64, _c.c_int64,
                                               _c.c_int64, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "bevwarp_stitch_maps_nv12_to_nv12": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int64, _c.c_int64,
                                                    _c.c_int64, _c.c_int64, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "bevwarp_remap_planes": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64,
                                        _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int, _c.c_int,
                                        _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p]),
    "bevwarp_stitch_maps_planes": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int,
                                              _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p]),
    "bevwarp_stitch_maps_nv12_planes": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int,
                                                   _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p]),
    "bevwarp_composite": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_void_p]),
    "bevwarp_warp_composite": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int64,
                                          _c.c_int64, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int64, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p]),
    "bevwarp_resize": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int64, _c.c_int64, _c.c_int64,
                                  _c.c_int64, _c.c_int, _c.c_int, _c.c_void_p]),
    "bevwarp_footprint": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int,
                                     _c.c_int, _c.c_void_p]),
    "bevwarp_project_points": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p]),
    "bevwarp_project_points_lens": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_double, _c.c_int, _c.c_int,
                                               _c.c_double, _c.c_int, _c.c_void_p]),
    "bevwarp_rbox_iou": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int,
                                    _c.c_void_p]),
    "bevwarp_rbox_transform": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p]),
    "bevwarp_tracker_step": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p,
                                        _c.c_double, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p]),
}


class Camera(_c.Structure):
    """bevwarp_camera (include/bevwarp.h): one camera of bevwarp_warp_stitch.  A host array of these is the call's first argument."""
    _fields_ = [("src", _c.c_void_p), ("M_inv", _c.c_void_p), ("frame_stride", _c.c_int64), ("row_stride", _c.c_int64), ("src_h", _c.c_int),
                ("src_w", _c.c_int), ("m_count", _c.c_int), ("reserved", _c.c_int)]


class MapCamera(_c.Structure):
    """bevwarp_map_camera (include/bevwarp.h): one camera of bevwarp_stitch_maps / bevwarp_stitch_maps_nv12.  A host array of these is the
    call's first argument."""
    _fields_ = [("src", _c.c_void_p), ("uv", _c.c_void_p), ("frame_stride", _c.c_int64), ("row_stride", _c.c_int64), ("uv_frame_stride", _c.c_int64),
                ("uv_row_stride", _c.c_int64), ("map_xy", _c.c_void_p), ("map_frac", _c.c_void_p), ("xy_frame_stride", _c.c_int64), ("xy_row_stride", _c.c_int64),
                ("frac_frame_stride", _c.c_int64), ("frac_row_stride", _c.c_int64), ("src_h", _c.c_int), ("src_w", _c.c_int), ("map_count", _c.c_int),
                ("reserved", _c.c_int)]


STITCH_OVER, STITCH_FEATHER, STITCH_MAX_CAMERAS = 0, 1, 8
MAP_BICUBIC = 0x200  # BEVWARP_MAP_BICUBIC, ORed into `interp` of bevwarp_remap alone: a bilinear map sampled bicubically
SUPERSAMPLE_2, SUPERSAMPLE_4, SUPERSAMPLE_8 = 0x1000, 0x2000, 0x3000  # BEVWARP_SUPERSAMPLE_*, ORed into `interp` of bevwarp_warp_border alone
STITCH_GAIN = 0x100  # BEVWARP_STITCH_GAIN, ORed into `blend` of the six stitches through maps: MapCamera.reserved is then the gain word

_lib = None


class BevWarpError(RuntimeError):
    pass


def build(force=False, verbose=False):
    """hipcc the HIP sources into csrc/libbevwarp.so (gfx950)."""
    cmd = ["make", "-C", _CSRC, "-j8"] + (["-B"] if force else [])
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(cmd, stdout=out)
    return LIB_PATH


def load():
    """The loaded library with typed entry points.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BevWarpError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(or `make -C bev_amd/csrc`).  There is no CPU fallback." % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SYMBOLS.items():
            fn = getattr(lib, name)  # AttributeError if the ABI and this table ever drift apart
            fn.restype = restype
            fn.argtypes = argtypes
        if lib.bevwarp_version() != ABI_VERSION:
            raise BevWarpError("libbevwarp ABI %d, expected %d" % (lib.bevwarp_version(), ABI_VERSION))
        _lib = lib
    return _lib


def check(status):
    if status != 0:
        lib = load()
        msg = lib.bevwarp_strerror(status).decode()
        if status == -5:
            raise BevWarpError("%s: %s" % (msg, lib.bevwarp_last_hip_error().decode()))
        raise ValueError("libbevwarp: " + msg)


def launch(name, device, *args):
    """One asynchronous launch: the symbol `name` called with `args` and, appended, the current stream of `device`, with that device
    current; a status other than 0 raises (check).  The general path of every Python entry point ends here; the validated-launch fast
    paths (warp.warp_perspective, iou.rbox_iou, tracker_geom.tracker_geometry_step) call their bound symbol themselves."""
    stream = torch.cuda.current_stream(device).cuda_stream
    with torch.cuda.device(device):
        st = getattr(load(), name)(*args, ctypes.c_void_p(stream))
    check(st)
