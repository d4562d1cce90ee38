"""Numpy reference of the equidistant (fisheye) lens model (include/bevwarp.h, BEVWARP_LENS_FISHEYE: bevwarp_warp_lens, bevwarp_build_map,
bevwarp_project_points_lens under the flag) -- TEST INFRASTRUCTURE ONLY, a plain module like tests/lens_ref.py and independent of bev_amd.

The definition, restated one float64 operation per line in the header's order (numpy never fuses; numpy's sqrt and division are the
correctly rounded IEEE ones).  No library arctangent: atan_pos below is part of the definition, its constants stated here with
float.fromhex.  From the maps on, the sampling is tests/remap_ref's (which is tests/lens_ref's for the two borders the lens warp takes): a
pixel beyond theta_max is the map entry whose taps are all outside.
"""
import numpy as np

from oracle.warp_numpy import INTER_BITS, INTER_TAB_SIZE, LINEAR, NEAREST, _round_clamped, block_width, invert3x3
from tests import remap_ref as RR

FISHEYE = 0x100  # BEVWARP_LENS_FISHEYE
DISTORT, UNDISTORT = 0, 1
K_TEST = (-0.02, 0.004, -0.001, 0.0002)  # monotonic to 110 degrees

A = [float.fromhex(h) for h in ("0x0.0p+0", "0x1.fd5ba9aac2f6ep-4", "0x1.f5b75f92c80ddp-3", "0x1.6f61941e4def1p-2", "0x1.dac670561bb4fp-2",
                                "0x1.1e00babdefeb4p-1", "0x1.4978fa3269ee1p-1", "0x1.700a7c5784634p-1", "0x1.921fb54442d18p-1")]
PIO2_HI, PIO2_LO = float.fromhex("0x1.921fb54442d18p+0"), float.fromhex("0x1.1a62633145c07p-54")
PI_HI, PI_LO = float.fromhex("0x1.921fb54442d18p+1"), float.fromhex("0x1.1a62633145c07p-53")
C3, C5, C7, C9, C11, C13, C15 = (np.float64(1.0) / np.float64(n) for n in (3, 5, 7, 9, 11, 13, 15))


def atan_pos(t):
    """atan(t) of the definition for t >= 0, +inf and NaN admitted (arrays or scalars; float64)."""
    t = np.asarray(t, np.float64)
    with np.errstate(all="ignore"):
        big = t > 1.0
        r = np.where(big, 1.0 / np.where(big, t, 1.0), t)
        i = 8.0 * r
        i = np.rint(i)
        c = i / 8.0
        n = r - c
        d = r * c
        d = 1.0 + d
        z = n / d
        z2 = z * z
        p = C15
        for ck in (C13, C11, C9, C7, C5, C3):
            p = z2 * p
            p = ck - p
        zz = z * z2
        zz = zz * p
        zz = z - zz
        idx = np.clip(np.where(np.isnan(i), 8.0, i), 0.0, 8.0).astype(np.int64)
        a = np.asarray(A)[idx] + zz
        b = PIO2_HI - a
        b = b + PIO2_LO
        return np.where(big, b, a)


def lens12(K, dist_coeff):
    """fx, fy, cx, cy, k1, k2, k3, k4, 0, 0, 0, 0."""
    K = np.asarray(K, np.float64)
    d = np.zeros(4) if dist_coeff is None else np.asarray(dist_coeff, np.float64).ravel()
    assert d.size == 4, d.size
    return np.concatenate([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]], d, np.zeros(4)])


def ray_matrix(M, K, inverse_given=False):
    """The ORIENTED ray matrix: inv(K) inv(M), with the sign that makes the ray of the optical axis' destination pixel point forward."""
    K = np.asarray(K, np.float64)
    M = np.asarray(M, np.float64).reshape(3, 3)
    Minv = M if inverse_given else invert3x3(M)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    R = np.stack([(Minv[0] - cx * Minv[2]) / fx, (Minv[1] - cy * Minv[2]) / fy, Minv[2]])
    c = np.array([cx, cy, 1.0])
    p = np.linalg.solve(Minv, c) if inverse_given else M @ c
    return -R if p[2] < 0 else R


def valid_theta(dist_coeff):
    """Smallest positive real root of 1 + 3 k1 t^2 + 5 k2 t^4 + 7 k3 t^6 + 9 k4 t^8, capped at pi (numpy.roots, descending coefficients)."""
    k1, k2, k3, k4 = [float(v) for v in dist_coeff]
    best = np.pi
    for r in np.atleast_1d(np.roots([9 * k4, 7 * k3, 5 * k2, 3 * k1, 1.0])):
        if abs(r.imag) <= 1e-9 * max(1.0, abs(r.real)) and r.real > 0:
            best = min(best, float(np.sqrt(r.real)))
    return best


def steps(lens, Xn, Yn, W):
    """(u, v, theta) of the fisheye steps on rays (Xn, Yn, W), undivided."""
    fx, fy, cx, cy, k1, k2, k3, k4 = [np.float64(v) for v in np.asarray(lens, np.float64).ravel()[:8]]
    Xn, Yn, W = np.asarray(Xn, np.float64), np.asarray(Yn, np.float64), np.asarray(W, np.float64)
    with np.errstate(all="ignore"):
        a = Xn * Xn
        b = Yn * Yn
        q = a + b
        rho = np.sqrt(q)
        t = rho / np.abs(W)
        at = atan_pos(t)
        b = PI_HI - at
        b = b + PI_LO
        theta = np.where(W < 0, b, at)
        th2 = theta * theta
        p = k4 * th2
        p = p + k3
        p = p * th2
        p = p + k2
        p = p * th2
        p = p + k1
        p = p * th2
        poly = 1.0 + p
        thd = theta * poly
        nz = rho != 0
        g = np.where(nz, thd / np.where(nz, rho, 1.0), 0.0)
        xd = Xn * g
        yd = Yn * g
        u = fx * xd
        u = u + cx
        v = fy * yd
        v = v + cy
    return u, v, theta


def rays(dsize, R):
    """(Xn, Yn, W) of the evaluation-block row walk, shape (dst_h, dst_w)."""
    dw, dh = int(dsize[0]), int(dsize[1])
    M = np.asarray(R, np.float64).ravel()
    bw0 = block_width(dw, dh)
    x = np.arange(dw)
    bx = (x // bw0) * bw0
    x1 = (x - bx).astype(np.float64)[None, :]
    bx = bx.astype(np.float64)[None, :]
    y = np.arange(dh, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        X0 = (M[0] * bx + M[1] * y) + M[2]
        Y0 = (M[3] * bx + M[4] * y) + M[5]
        W0 = (M[6] * bx + M[7] * y) + M[8]
        return X0 + M[0] * x1, Y0 + M[3] * x1, W0 + M[6] * x1


def chain(dsize, R, lens):
    """(u, v, theta) float64 arrays of shape (dst_h, dst_w)."""
    return steps(lens, *rays(dsize, R))


def maps(dsize, R, lens, theta_max, interp):
    """(sx, sy, fx, fy, valid) as tests/lens_ref.maps gives them."""
    u, v, theta = chain(dsize, R, lens)
    with np.errstate(all="ignore"):
        if interp == NEAREST:
            X, Y = _round_clamped(u), _round_clamped(v)
            sx, sy, fx, fy = X, Y, np.zeros_like(X), np.zeros_like(Y)
        else:
            X, Y = _round_clamped(u * 32.0), _round_clamped(v * 32.0)
            sx, sy = X >> INTER_BITS, Y >> INTER_BITS
            fx, fy = X & (INTER_TAB_SIZE - 1), Y & (INTER_TAB_SIZE - 1)
        valid = theta <= np.float64(theta_max)  # (False for NaN)
    return np.clip(sx, -32768, 32767), np.clip(sy, -32768, 32767), fx, fy, valid


def build(dsize, R, lens, theta_max, interp=LINEAR):
    """(xy, frac) as tests/remap_ref.build gives them: an invalid pixel is the (-32768, -32768), frac 0 entry."""
    sx, sy, fx, fy, valid = maps(dsize, R, lens, theta_max, interp)
    sx, sy = np.where(valid, sx, RR.SENTINEL), np.where(valid, sy, RR.SENTINEL)
    xy = np.stack([sx, sy], axis=-1).astype(np.int16)
    if interp == NEAREST:
        return xy, None
    fx, fy = np.where(valid, fx, 0), np.where(valid, fy, 0)
    return xy, ((fy.astype(np.int64) << 5) | fx.astype(np.int64)).astype(np.uint16)


def warp(src, R, lens, theta_max, dsize, interp=LINEAR, mode=RR.CONSTANT, border_value=0.0, canvas=None):
    """The fisheye warp (CONSTANT or TRANSPARENT): the sampler through the maps -- "invalid is outside"."""
    assert mode in (RR.CONSTANT, RR.TRANSPARENT), mode
    xy, frac = build(dsize, R, lens, theta_max, interp)
    return RR.remap(src, xy, frac, interp, mode, border_value, canvas)


def _apply(H, x, y, z):
    """H (x, y, z) in plane()'s operand order, undivided."""
    h = np.asarray(H, np.float64).ravel()
    out = []
    for r in (0, 3, 6):
        a = h[r + 1] * y
        b = h[r + 2] * z
        a = a + b
        b = h[r] * x
        out.append(a + b)
    return out


def distort_chain(pts, H, lens):
    """(u, v, theta) of DISTORT before the verdict."""
    pts = np.asarray(pts)
    x, y = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        return steps(lens, *_apply(H, x, y, np.float64(1.0)))


def distort(pts, H, lens, theta_max):
    pts = np.asarray(pts)
    u, v, theta = distort_chain(pts, H, lens)
    with np.errstate(all="ignore"):
        valid = theta <= np.float64(theta_max)
        return np.stack([np.where(valid, u, np.nan), np.where(valid, v, np.nan)], axis=1).astype(pts.dtype)


def undistort_ray(pts, lens, iters):
    """(rx, ry, rz) of UNDISTORT after `iters` Newton steps in s = tan(theta / 2); float64."""
    fx, fy, cx, cy, k1, k2, k3, k4 = [np.float64(v) for v in np.asarray(lens, np.float64).ravel()[:8]]
    pts = np.asarray(pts)
    u, v = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        d1, d2, d3, d4 = 3.0 * k1, 5.0 * k2, 7.0 * k3, 9.0 * k4
        xd = u - cx
        xd = xd / fx
        yd = v - cy
        yd = yd / fy
        a = xd * xd
        b = yd * yd
        thd = np.sqrt(a + b)
        s = thd / 2.0
        for _ in range(int(iters)):
            theta = 2.0 * atan_pos(s)
            th2 = theta * theta
            p = k4 * th2
            p = p + k3
            p = p * th2
            p = p + k2
            p = p * th2
            p = p + k1
            p = p * th2
            poly = 1.0 + p
            f = theta * poly
            f = f - thd
            D = d4 * th2
            D = D + d3
            D = D * th2
            D = D + d2
            D = D * th2
            D = D + d1
            D = D * th2
            D = 1.0 + D
            a = s * s
            a = 1.0 + a
            a = f * a
            b = 2.0 * D
            a = a / b
            s = s - a
            s = np.where(s < 0, 0.0, s)
        off = thd != 0
        safe = np.where(off, thd, 1.0)
        s2 = 2.0 * s
        rx = np.where(off, s2 * (xd / safe), 0.0)
        ry = np.where(off, s2 * (yd / safe), 0.0)
        a = s * s
        rz = np.where(off, 1.0 - a, 1.0)
    return rx, ry, rz


def undistort(pts, H, lens, theta_max, iters, tol_px):
    """(out, residual) of UNDISTORT: (N, 2) and (N,) of pts' dtype."""
    pts = np.asarray(pts)
    u, v = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    rx, ry, rz = undistort_ray(pts, lens, iters)
    with np.errstate(all="ignore"):
        u2, v2, theta = steps(lens, rx, ry, rz)
        du = np.abs(u2 - u)
        dv = np.abs(v2 - v)
        e = np.maximum(du, dv)  # NaN if either is
        valid = (theta <= np.float64(theta_max)) & (e <= np.float64(tol_px))
        X, Y, W = _apply(H, rx, ry, rz)
        nz = W != 0
        Wr = np.where(nz, 1.0 / np.where(nz, W, 1.0), 0.0)
        out = np.stack([np.where(valid, X * Wr, np.nan), np.where(valid, Y * Wr, np.nan)], axis=1)
        return out.astype(pts.dtype), e.astype(pts.dtype)
