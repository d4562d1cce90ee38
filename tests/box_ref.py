"""Rotated boxes between the BEV raster and the world plane, stated with POINTS (float64 numpy): a reference for the device
kernels and for bev_amd.rbox that shares no yaw algebra with either.  Test infrastructure only.

Written from the frame conventions alone (the header of the upstream rbox.py):
  * BEV:   u runs right, v runs down; yaw = atan2(du, dv) of the heading, so yaw 0 looks along +v; at yaw 0 `w` spans u, `h` spans v.
  * world: right-handed x / y; yaw = atan2(dy, dx) of the heading, so yaw 0 looks along +x; at yaw 0 `h` spans x, `w` spans y.
  * a box is [x, y, w, h, yaw]: the length h runs along the heading, the width w across it.
A box is turned into five points -- its four corners and the midpoint of its front edge --, the points go through H, and the
target box is measured on the image points: centre = mean of the corners, h = front edge to back edge, w = along the front
edge, yaw = the target frame's atan2 of centre -> front.  Nothing here knows which way H turns, whether it mirrors, or how a
heading vector of one frame reads in the other: a mirrored H simply hands the corners over in the opposite sense, and the
measurements do not care.

What "through H" means for a box.  The upstream transform accepts any H whose normalised last row is (a, b, 1) with
|a| + |b| < 1e-5.  It sends the CENTRE through H as a point (homogeneous divide) and the box's extent through H's similarity
part (the heading as a direction, w = 0; the sizes by the column norm).  `through` states the same thing with points: the centre
is a point, the corners and the front are the centre's image plus the images of their OFFSETS as vectors.  For an exact
similarity (last row (0, 0, k)) that is the same as pushing all five points through H with the divide -- `through_points`, the
literal form; tests/test_box_ref_cpu.py holds the two together at 1e-12 on every exact similarity the suite uses -- and for a last
row that is small but not zero it is the only reading under which a box stays a rectangle."""
import numpy as np

_MODES = ("bev", "world")
# (along the heading, across it) of the corners, in the order back-left, front-left, front-right, back-right
_CORNERS = ((-1, -1), (1, -1), (1, 1), (-1, 1))


def other(mode):
    assert mode in _MODES
    return "world" if mode == "bev" else "bev"


def _axes(yaw, mode):
    """Unit heading and unit side vector of a box in its own frame, (n, 2) each."""
    s, c = np.sin(yaw), np.cos(yaw)
    if mode == "bev":   # yaw from +v towards +u; the side axis is +u at yaw 0 and turns with the heading
        return np.stack([s, c], axis=1), np.stack([c, -s], axis=1)
    return np.stack([c, s], axis=1), np.stack([-s, c], axis=1)  # yaw from +x towards +y; the side axis is +y at yaw 0


def offsets(boxes, mode):
    """(n, 5, 2): the four corners and the front midpoint of each box, relative to its centre."""
    assert mode in _MODES
    b = np.asarray(boxes, dtype=np.float64)[:, :5]
    d, s = _axes(b[:, 4], mode)
    half_h, half_w = 0.5 * b[:, 3:4], 0.5 * b[:, 2:3]
    rows = [sd * half_h * d + ss * half_w * s for sd, ss in _CORNERS] + [half_h * d]
    return np.stack(rows, axis=1)


def points(boxes, mode):
    """(n, 5, 2): the four corners and the front midpoint of each box in its own frame."""
    b = np.asarray(boxes, dtype=np.float64)[:, :5]
    return b[:, None, :2] + offsets(b, mode)


def quad(boxes, mode):
    """Corner list of boxes that have NOT been transformed: (4, 2) for one box, (n, 4, 2) for an (n, >=5) array."""
    b = np.asarray(boxes, dtype=np.float64)
    if b.ndim == 1:
        return points(b[None, :], mode)[0, :4]
    return points(b, mode)[:, :4]


def project(pts, H):
    """(..., 2) points through the 3 x 3 H with the homogeneous divide."""
    H = np.asarray(H, dtype=np.float64)
    p = np.asarray(pts, dtype=np.float64)
    X = H[0, 0] * p[..., 0] + H[0, 1] * p[..., 1] + H[0, 2]
    Y = H[1, 0] * p[..., 0] + H[1, 1] * p[..., 1] + H[1, 2]
    W = H[2, 0] * p[..., 0] + H[2, 1] * p[..., 1] + H[2, 2]
    return np.stack([X / W, Y / W], axis=-1)


def through(boxes, H, src):
    """(n, 5, 2): images of the boxes' five points in the other frame -- the centre as a point, the extent as vectors (see above)."""
    H = np.asarray(H, dtype=np.float64)
    Hn = H / H[2, 2]
    b = np.asarray(boxes, dtype=np.float64)[:, :5]
    off = offsets(b, src)
    centre = project(b[:, :2], Hn)
    vec = np.stack([Hn[0, 0] * off[..., 0] + Hn[0, 1] * off[..., 1], Hn[1, 0] * off[..., 0] + Hn[1, 1] * off[..., 1]], axis=-1)
    return centre[:, None, :] + vec


def through_points(boxes, H, src):
    """The literal form: all five points through H with the divide.  Equal to `through` when H's last row is (0, 0, k)."""
    return project(points(boxes, src), H)


def read_box(pts, mode):
    """(n, 5, 2) points (corners in the order of `points`, then the front midpoint) -> (n, 5) boxes of frame `mode`."""
    assert mode in _MODES
    p = np.asarray(pts, dtype=np.float64)
    centre = p[:, :4].mean(axis=1)
    back, front = 0.5 * (p[:, 0] + p[:, 3]), 0.5 * (p[:, 1] + p[:, 2])
    h = np.hypot(*(front - back).T)
    w = np.hypot(*(p[:, 2] - p[:, 1]).T)
    ahead = p[:, 4] - centre
    yaw = np.arctan2(ahead[:, 0], ahead[:, 1]) if mode == "bev" else np.arctan2(ahead[:, 1], ahead[:, 0])
    return np.column_stack([centre, w, h, yaw])


def rbox_world_bev(boxes, H, src):
    """(n, >=5) boxes of frame `src` ("bev" | "world") -> (n, 5) boxes of the other frame through H."""
    return read_box(through(boxes, H, src), other(src))


def rbox_world_bev_points(boxes, H, src):
    """The same with the literal five-point projection (exact similarities only)."""
    return read_box(through_points(boxes, H, src), other(src))


def centres_img(boxes_world, H_img_world):
    """(n, 2) image pixels of the world boxes' centres (H_img_world is a full homography)."""
    return project(np.asarray(boxes_world, dtype=np.float64)[:, :2], H_img_world)


def yaw_diff(a, b):
    """a - b as angles: wrapped into (-pi, pi]."""
    return np.angle(np.exp(1j * (np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))))


def assert_boxes_close(got, exp, rtol=1e-12, atol=1e-12, err_msg=""):
    """x, y, w, h as numbers, the yaw as an angle (modulo 2 pi)."""
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, (got.shape, exp.shape, err_msg)
    np.testing.assert_allclose(got[:, :4], exp[:, :4], rtol=rtol, atol=atol, err_msg=err_msg)
    miss = np.abs(yaw_diff(got[:, 4], exp[:, 4])) - (atol + rtol * np.abs(exp[:, 4]))
    assert (miss <= 0).all(), "%s yaw off by up to %.3g beyond the bar (row %d)" % (err_msg, miss.max(), int(miss.argmax()))
