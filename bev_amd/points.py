"""Device point projection: pts_world_bev (reference bev/rbox.py:136-151) for large N on the GPU, and the same through a camera's lens
model (distort_points, undistort_points, world_to_raw, raw_to_world: include/bevwarp.h, bevwarp_project_points_lens)."""
import ctypes
import math

import numpy as np
import torch

from . import _lib

_DTYPES = {torch.float32: _lib.F32, torch.float64: _lib.F64}
LENS_DISTORT, LENS_UNDISTORT = 0, 1


def project_points(pts, H, out=None):
    """pts: (N, 2) or (N, 3) float32/float64 CUDA tensor, contiguous.  H: 3x3 (numpy / tensor / list).
    N x 2 -> N x 2 (dehomogenised);  N x 3 -> N x 3 (homogeneous in, last column 1 out).
    One pass over memory, float64 arithmetic.  `out` may alias `pts`."""
    if not isinstance(pts, torch.Tensor) or not pts.is_cuda:
        raise ValueError("project_points needs a CUDA (HIP) tensor; bev.rbox.pts_world_bev is the host version")
    if pts.dtype not in _DTYPES or pts.dim() != 2 or pts.shape[1] not in (2, 3):
        raise ValueError("pts must be (N, 2|3) float32/float64, got %s %s" % (tuple(pts.shape), pts.dtype))
    pts = pts.contiguous()
    if out is None:
        out = torch.empty_like(pts)
    elif out.shape != pts.shape or out.dtype != pts.dtype or not out.is_contiguous():
        raise ValueError("out must match pts")
    Hh = np.ascontiguousarray(H.detach().cpu().numpy() if isinstance(H, torch.Tensor) else H, dtype=np.float64).reshape(3, 3)
    _lib.launch("bevwarp_project_points", pts.device, pts.data_ptr(), out.data_ptr(), pts.shape[0], pts.shape[1], Hh.ctypes.data_as(ctypes.c_void_p),
                _DTYPES[pts.dtype])
    return out


def _host3x3(who, H):
    """H (numpy / tensor / list, None: the identity) as a contiguous float64 3x3."""
    if H is None:
        return np.eye(3)
    Hh = np.ascontiguousarray(H.detach().cpu().numpy() if isinstance(H, torch.Tensor) else H, dtype=np.float64)
    if Hh.shape != (3, 3):
        raise ValueError("%s: H must be 3x3, got %s" % (who, Hh.shape))
    return Hh


def _lens_call(who, pts, K, dist_coeff, r2_max, out, lens_model="rational", theta_max=None):
    """What the two lens entries check before any launch: (pts contiguous, out, lens of 12 doubles or None for no distortion, r2_max --
    under the fisheye model, which always has a lens, theta_max --, fisheye)."""
    from .warp import _dist8, _fisheye4, _intrinsics, _lens_model, fisheye_valid_theta, lens_valid_r2
    fisheye = _lens_model(who, lens_model, r2_max, theta_max)
    intr, dist = _intrinsics(K), (np.concatenate([_fisheye4(dist_coeff), np.zeros(4)]) if fisheye else _dist8(dist_coeff))
    if not np.isfinite(intr).all() or not np.isfinite(dist).all() or intr[0] == 0.0 or intr[1] == 0.0:
        raise ValueError("%s: K and dist_coeff must be finite, fx and fy non-zero" % who)
    if fisheye:
        r2 = fisheye_valid_theta(dist[:4]) if theta_max is None else float(theta_max)
        if not r2 >= 0.0:
            raise ValueError("%s: theta_max must be >= 0 radians (inf: no limit), got %r" % (who, theta_max))
    else:
        r2 = lens_valid_r2(dist) if r2_max is None else float(r2_max)
        if not r2 >= 0.0:
            raise ValueError("%s: r2_max must be >= 0 (inf: no limit), got %r" % (who, r2_max))
    if not isinstance(pts, torch.Tensor) or not pts.is_cuda:
        raise ValueError("%s needs a CUDA (HIP) tensor" % who)
    if pts.dtype not in _DTYPES or pts.dim() != 2 or pts.shape[1] != 2:
        raise ValueError("%s: pts must be (N, 2) float32/float64, got %s %s" % (who, tuple(pts.shape), pts.dtype))
    pts = pts.contiguous()
    if out is None:
        out = torch.empty_like(pts)
    elif not isinstance(out, torch.Tensor) or out.shape != pts.shape or out.dtype != pts.dtype or out.device != pts.device or not out.is_contiguous():
        raise ValueError("%s: out must match pts" % who)
    lens = np.ascontiguousarray(np.concatenate([intr, dist]), dtype=np.float64) if (fisheye or dist.any()) else None
    return pts, out, lens, r2, fisheye


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def distort_points(pts, K, dist_coeff, H=None, r2_max=None, out=None, lens_model="rational", theta_max=None):
    """Points -> pixels of the RAW frame of a distorted camera: what cv2.projectPoints is for (not bit-equal to it).
    pts      (N, 2) float32/float64 CUDA tensor.
    K        3x3 or 3x4 camera matrix of the raw frames, no skew.
    dist_coeff   None, or 4, 5 or 8 values in OpenCV's order (k1, k2, p1, p2[, k3[, k4, k5, k6]]).  None or all zero: the call IS
             project_points(pts, H).
    H        3x3 map from pts' coordinates to UNDISTORTED image pixels (H_img_world, say); None: pts are undistorted pixels.
    r2_max   points whose squared radius on the normalised camera plane exceeds it come back as NaN; None: lens_valid_r2(dist_coeff),
             float("inf"): no limit.
    lens_model   "rational" (default), or "fisheye": the equidistant model of cv2.fisheye (include/bevwarp.h, BEVWARP_LENS_FISHEYE).
             dist_coeff is then None or (k1, k2, k3, k4); the guard is theta_max, the angle from the optical axis in radians (None:
             fisheye_valid_theta(dist_coeff); passing r2_max raises ValueError); points at and beyond 90 degrees from the axis project
             like any other, the ray matrix being built oriented (warp.ray_matrix); nothing is handed to project_points.
    One launch, float64 arithmetic, asynchronous on the current stream.  `out` may alias `pts`."""
    from .warp import LENS_FISHEYE, ray_matrix
    Hh = _host3x3("distort_points", H)
    pts, out, lens, r2, fisheye = _lens_call("distort_points", pts, K, dist_coeff, r2_max, out, lens_model, theta_max)
    if lens is None:
        return project_points(pts, Hh, out=out)
    if pts.shape[0] == 0:  # (an empty tensor has no address to pass)
        return out
    R = np.ascontiguousarray(ray_matrix(Hh, K, inverse_given=True, oriented=fisheye))
    _lib.launch("bevwarp_project_points_lens", pts.device, pts.data_ptr(), out.data_ptr(), None, pts.shape[0], _ptr(R), _ptr(lens), r2,
                LENS_DISTORT | (LENS_FISHEYE if fisheye else 0), 0, 0.0, _DTYPES[pts.dtype])
    return out


def undistort_points(pts, K, dist_coeff, H=None, iters=None, tol_px=1e-3, r2_max=None, out=None, return_residual=False, lens_model="rational",
                     theta_max=None):
    """Pixels of the RAW frame of a distorted camera -> the plane behind the lens: what cv2.undistortPoints is for (not bit-equal to it).
    pts      (N, 2) float32/float64 CUDA tensor of raw-frame pixels.
    K, dist_coeff, r2_max   as distort_points.  No distortion: the call IS project_points(pts, H) (the residual is then 0).
    H        3x3 map from UNDISTORTED image pixels to the target (H_world_img, say); None: undistorted pixels come back.
    iters    1..100 fixed-point steps, all of them taken.  The default (None) is 20, not OpenCV's 5: 5 steps leave 0.1 px inside a
             640 x 360 frame of a moderately distorted lens, 20 leave less than 1e-6 px.  Under the fisheye model the steps are Newton's and
             the default is 10.
    tol_px   a point whose reprojection into the raw frame misses it by more than this, in pixels, comes back as NaN (the iteration
             did not converge: a point far outside the frame); float("inf") accepts every error that is not NaN.
    return_residual   also return the (N,) reprojection errors in pixels, written for valid and invalid points alike.
    lens_model, theta_max   as distort_points.  Under "fisheye" the plane behind the lens is reached through the RAY (x, y, z) of the pixel,
             not through a point divided by its depth: H (3x3, undistorted pixels -> target) is applied to K (x, y, z) and divided once.
    One launch, float64 arithmetic, asynchronous on the current stream.  `out` may alias `pts`."""
    from .warp import LENS_FISHEYE, _intrinsics
    if iters is None:
        iters = 10 if lens_model == "fisheye" else 20
    if isinstance(iters, bool) or int(iters) != iters or not 1 <= int(iters) <= 100:
        raise ValueError("undistort_points: iters must be an integer in 1..100, got %r" % (iters,))
    tol = float(tol_px)
    if math.isnan(tol) or tol < 0.0:
        raise ValueError("undistort_points: tol_px must be >= 0 (inf: accept any), got %r" % (tol_px,))
    Hh = _host3x3("undistort_points", H)
    pts, out, lens, r2, fisheye = _lens_call("undistort_points", pts, K, dist_coeff, r2_max, out, lens_model, theta_max)
    if lens is None:
        got = project_points(pts, Hh, out=out)
        return (got, torch.zeros(pts.shape[0], dtype=pts.dtype, device=pts.device)) if return_residual else got
    fx, fy, cx, cy = _intrinsics(K)
    Hk = np.ascontiguousarray(Hh @ np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]]))  # normalised plane -> target
    res = torch.empty(pts.shape[0], dtype=pts.dtype, device=pts.device) if return_residual else None
    if pts.shape[0] == 0:  # (an empty tensor has no address to pass)
        return (out, res) if return_residual else out
    _lib.launch("bevwarp_project_points_lens", pts.device, pts.data_ptr(), out.data_ptr(), None if res is None else res.data_ptr(), pts.shape[0], _ptr(Hk),
                _ptr(lens), r2, LENS_UNDISTORT | (LENS_FISHEYE if fisheye else 0), int(iters), tol, _DTYPES[pts.dtype])
    return (out, res) if return_residual else out


def _calib_lens(calib, lens_model):
    """(K, dist_coeff) of a Calib; under the fisheye model a Calib without coefficients has the 4 zeros of an ideal equidistant lens."""
    from .warp import lens_from_calib
    K, dist = lens_from_calib(calib)
    return K, (np.zeros(4) if lens_model == "fisheye" and calib.dist_coeff is None else dist)


def world_to_raw(calib, pts, r2_max=None, out=None, lens_model="rational", theta_max=None):
    """World points of the road plane (N, 2) -> pixels of the camera's RAW frame: rbox_world_img's projection (bev/rbox.py:221-226)
    through calib.dist_coeff.  calib: a Calib with K (lens_from_calib).  lens_model, theta_max: as distort_points."""
    K, dist = _calib_lens(calib, lens_model)
    H_img_world = np.linalg.inv(np.asarray(calib.gen_H_world_img(), dtype=np.float64))
    return distort_points(pts, K, dist, H=H_img_world, r2_max=r2_max, out=out, lens_model=lens_model, theta_max=theta_max)


def raw_to_world(calib, pts, iters=None, tol_px=1e-3, r2_max=None, out=None, return_residual=False, lens_model="rational", theta_max=None):
    """Pixels of the camera's RAW frame (N, 2) -> world points of the road plane: Calib.gen_center_in_world's projection
    (bev/calib.py:135-138) for any pixel, through calib.dist_coeff.  Pixels the lens model cannot invert come back as NaN.
    lens_model, theta_max: as undistort_points."""
    K, dist = _calib_lens(calib, lens_model)
    H_world_img = np.asarray(calib.gen_H_world_img(), dtype=np.float64)
    return undistort_points(pts, K, dist, H=H_world_img, iters=iters, tol_px=tol_px, r2_max=r2_max, out=out, return_residual=return_residual,
                            lens_model=lens_model, theta_max=theta_max)
