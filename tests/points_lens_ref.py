"""Numpy reference of the lens point projection (bev_amd.points.distort_points / undistort_points, include/bevwarp.h
bevwarp_project_points_lens) -- TEST INFRASTRUCTURE ONLY, a plain module like tests/lens_ref.py and independent of bev_amd.

The definition, restated one float64 operation per line in the header's order (numpy never fuses).  float32 points widen exactly
on the way in; `out` and `residual` are the float64 results rounded to nearest (astype)."""
import numpy as np

DISTORT, UNDISTORT = 0, 1


def plane(H, x, y):
    """(X Wr, Y Wr) of the header's plane(x, y)."""
    h = np.asarray(H, np.float64).ravel()
    a = h[1] * y
    a = a + h[2]
    b = h[0] * x
    X = a + b
    a = h[4] * y
    a = a + h[5]
    b = h[3] * x
    Y = a + b
    a = h[7] * y
    a = a + h[8]
    b = h[6] * x
    W = a + b
    nz = W != 0
    Wr = np.where(nz, 1.0 / np.where(nz, W, 1.0), 0.0)
    return X * Wr, Y * Wr


def _num_den(lens, r2):
    k1, k2, k3, k4, k5, k6 = lens[4], lens[5], lens[8], lens[9], lens[10], lens[11]
    n = k3 * r2
    n = n + k2
    n = n * r2
    n = n + k1
    n = n * r2
    num = 1.0 + n
    d = k6 * r2
    d = d + k5
    d = d * r2
    d = d + k4
    d = d * r2
    den = 1.0 + d
    return num, den


def lens_steps(lens, xn, yn):
    """(u, v, r2): the lens warp's lines `x2 = ...` to `v = fy yd + cy`."""
    fx, fy, cx, cy, p1, p2 = lens[0], lens[1], lens[2], lens[3], lens[6], lens[7]
    x2 = xn * xn
    y2 = yn * yn
    r2 = x2 + y2
    xy = xn * yn
    xy2 = 2.0 * xy
    num, den = _num_den(lens, r2)
    kr = num / den
    a = xn * kr
    b = p1 * xy2
    a = a + b
    b = 2.0 * x2
    b = r2 + b
    b = p2 * b
    xd = a + b
    a = yn * kr
    b = 2.0 * y2
    b = r2 + b
    b = p1 * b
    a = a + b
    b = p2 * xy2
    yd = a + b
    u = fx * xd
    u = u + cx
    v = fy * yd
    v = v + cy
    return u, v, r2


def _lens(lens):
    return [np.float64(v) for v in np.asarray(lens, np.float64).ravel()]


def distort_chain(pts, H, lens):
    """(u, v, r2) of BEVWARP_LENS_DISTORT before the verdict: float64 arrays of shape (N,)."""
    pts = np.asarray(pts)
    x, y = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        xn, yn = plane(H, x, y)
        return lens_steps(_lens(lens), xn, yn)


def distort(pts, H, lens, r2_max):
    """out of BEVWARP_LENS_DISTORT: (N, 2) of pts' dtype."""
    pts = np.asarray(pts)
    u, v, r2 = distort_chain(pts, H, lens)
    with np.errstate(all="ignore"):
        valid = r2 <= np.float64(r2_max)  # (False for NaN)
        out = np.stack([np.where(valid, u, np.nan), np.where(valid, v, np.nan)], axis=1)
        return out.astype(pts.dtype)


def undistort(pts, H, lens, r2_max, iters, tol_px):
    """(out, residual) of BEVWARP_LENS_UNDISTORT: (N, 2) and (N,) of pts' dtype."""
    pts = np.asarray(pts)
    lens = _lens(lens)
    fx, fy, cx, cy, p1, p2 = lens[0], lens[1], lens[2], lens[3], lens[6], lens[7]
    u, v = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        xd = u - cx
        xd = xd / fx
        yd = v - cy
        yd = yd / fy
        x, y = xd, yd
        for _ in range(int(iters)):
            x2 = x * x
            y2 = y * y
            r2 = x2 + y2
            xy = x * y
            xy2 = 2.0 * xy
            num, den = _num_den(lens, r2)
            ic = den / num
            a = p1 * xy2
            b = 2.0 * x2
            b = r2 + b
            b = p2 * b
            dx = a + b
            a = 2.0 * y2
            a = r2 + a
            a = p1 * a
            b = p2 * xy2
            dy = a + b
            x = xd - dx
            x = x * ic
            y = yd - dy
            y = y * ic
        u2, v2, r2 = lens_steps(lens, x, y)
        du = np.abs(u2 - u)
        dv = np.abs(v2 - v)
        e = np.maximum(du, dv)  # NaN if either is
        valid = (r2 <= np.float64(r2_max)) & (e <= np.float64(tol_px))
        wx, wy = plane(H, x, y)
        out = np.stack([np.where(valid, wx, np.nan), np.where(valid, wy, np.nan)], axis=1)
        return out.astype(pts.dtype), e.astype(pts.dtype)


def same_bits(got, want):
    """Equal bit for bit, but for NaNs, which only have to be NaNs (the header leaves their sign and payload open)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    nan = np.isnan(want)
    ints = np.int32 if got.dtype == np.float32 else np.int64
    return bool((np.isnan(got) == nan).all() and (got.view(ints)[~nan] == want.view(ints)[~nan]).all())
