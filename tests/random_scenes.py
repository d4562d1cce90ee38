"""Seeded random scenes for the lens, map, NV12 and stitch entries -- TEST INFRASTRUCTURE ONLY, a plain module like tests/pixels.py.

cases(family, seed)   the frozen case records of one seed: parameters and seeds only, every draw from numpy.random.default_rng, so that a
                      case is the same on any machine and is named by (family, seed, index)
inputs(case)          its host arrays, made on demand: frames, matrices (canvas px -> camera px), lenses, gains
expected(case)        what the entry has to give, frame by frame, from the numpy definitions that exist: lens_ref, fisheye_ref, remap_ref,
                      nv12_ref, nv12_out_ref, remap_nv12_ref, remap_nv12_out_ref, map_planes_ref, planes16_ref, stitch_ref, stitch_maps_ref,
                      stitch_gain_ref.  No arithmetic of its own.
census(case)          the paths the case reaches, counted from the definitions alone (tests/test_random_scenes_cpu.py holds the floors)

Sizes: sources 1..96 x 1..64 (NV12: even), canvases 1..130 x 1..40 (NV12 output: even), batches of 1, 2, 3 or 5, 1..8 cameras -- the
smallest shapes at which the paths still occur.  Every matrix a case hands to an entry is the INVERSE map (WARP_INVERSE_MAP), except in
the NV12 family, whose entries and definitions are given forward maps and invert them.  tests/test_gpu_random_scenes.py runs the cases on
the device."""
import dataclasses
import functools

import numpy as np

from oracle import cpu_oracle as co
from oracle.warp_numpy import LINEAR
from tests import fisheye_ref as FR
from tests import lens_ref as LR
from tests import map_planes_ref as MP
from tests import nv12_out_ref as NO
from tests import nv12_ref as NR
from tests import planes16_ref as P16
from tests import remap_nv12_out_ref as RNO
from tests import remap_nv12_ref as RN
from tests import remap_ref as RR
from tests import stitch_gain_ref as SG
from tests import stitch_maps_ref as SM
from tests import stitch_ref as SR

FAMILIES = ("lens", "map", "nv12", "stitch")
SEEDS = tuple(range(8))
N_CASES = 12
CANVAS = 77                      # what a destination of a layout case holds before the call
BATCHES = (1, 2, 3, 5)
FEATHERS = (1, 2, 3, 7, 64)
LENSES = {"A": LR.LENS_A, "B": LR.LENS_B}
SCALES = ((1 / 255.0, 0.017, 3.0, 0.5), (1.0, 1.0, 1.0, 1.0), (0.25, -2.0, 1 / 3.0, 7.0))
BIASES = ((-0.4, 0.25, 11.5, 0.0), (0.0, 0.0, 0.0, 0.0), (100.0, -0.001, 0.5, -3.0))
MAP_USERS = ("remap", "remap_nv12", "remap_to_nv12", "remap_nv12_to_nv12", "remap_to_planar", "remap_nv12_to_planar")
NV12_ENTRIES = ("warp_perspective_nv12", "warp_nv12_to_planar", "warp_perspective_to_nv12", "warp_nv12_to_nv12", "warp_to_planar")
STITCH_ENTRIES = ("warp_stitch", "maps", "nv12", "to_nv12", "nv12_to_nv12", "planes", "nv12_planes")
_FAMILY_BASE = {"lens": 11000, "map": 12000, "nv12": 13000, "stitch": 14000}  # fixed: a new family gets a new base


class Rec(tuple):
    """A frozen record: a tuple of (name, value) pairs whose values are read as attributes."""

    def __getattr__(self, name):
        for k, v in self:
            if k == name:
                return v
        raise AttributeError(name)


def rec(**kw):
    return Rec(tuple(kw.items()))


@dataclasses.dataclass(frozen=True)
class Case:
    family: str
    seed: int
    index: int
    p: Rec

    def __str__(self):
        return "%s seed %d case %d: %s" % (self.family, self.seed, self.index, " ".join("%s=%r" % kv for kv in self.p))


# ---- random matrices ------------------------------------------------------------------------------------------------------------------------

def _random_homography(rng, sw, sh, dw, dh):
    """src -> dst map of a random similarity-plus-perspective window: rotation, 0.4 .. 3 x scale, mild keystone, a shift that
    may push part of the window out of the frame."""
    ang = rng.uniform(-np.pi, np.pi) if rng.random() < 0.7 else rng.choice([0.0, np.pi / 2, np.pi, -np.pi / 2])
    zoom = float(np.exp(rng.uniform(np.log(0.4), np.log(3.0))))
    c, s = np.cos(ang) * zoom, np.sin(ang) * zoom
    A = np.array([[c, -s, 0.0], [s, c, 0.0], [rng.uniform(-2e-4, 2e-4), rng.uniform(-2e-4, 2e-4), 1.0]])
    T0 = np.array([[1, 0, -(dw - 1) / 2.0], [0, 1, -(dh - 1) / 2.0], [0, 0, 1.0]])
    T1 = np.array([[1, 0, (sw - 1) / 2.0 + rng.uniform(-0.4, 0.4) * sw], [0, 1, (sh - 1) / 2.0 + rng.uniform(-0.4, 0.4) * sh], [0, 0, 1.0]])
    if rng.random() < 0.25:  # integer-valued similarity: every coordinate on a tie boundary
        A = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]]) * [[1], [1], [1]]
        T1 = np.round(T1)
        T0 = np.round(T0)
    return np.linalg.inv(T1 @ A @ T0)


_QUARTER_TURNS = ([[1, 0], [0, 1]], [[0, -1], [1, 0]], [[-1, 0], [0, -1]], [[0, 1], [-1, 0]], [[-1, 0], [0, 1]], [[1, 0], [0, -1]])


def _part_view_inverse(rng, sw, sh, dw, dh, horizon=False):
    """canvas px -> camera px of a camera that sees only PART of a canvas: a random canvas anchor (it may lie a little outside) lands on the
    frame's centre, turned, 0.3 .. 2.5 source px per canvas px (fewer for frames under 24 px), projective terms up to 2e-3; one draw in four is integer-valued (a quarter
    turn or a mirror, an integer shift), so that every coordinate lies on a tie.  horizon: the denominator changes sign inside the canvas."""
    ax, ay = rng.uniform(-0.1, 1.1) * (dw - 1), rng.uniform(-0.1, 1.1) * (dh - 1)
    ang = rng.uniform(-np.pi, np.pi) if rng.random() < 0.7 else rng.choice([0.0, np.pi / 2, np.pi, -np.pi / 2])
    zoom = float(np.exp(rng.uniform(np.log(0.3), np.log(2.5)))) * min(1.0, max(sw, sh) / 24.0)  # (a small frame is magnified: it still meets the canvas)
    c, s = np.cos(ang) * zoom, np.sin(ang) * zoom
    A = np.array([[c, -s, 0.0], [s, c, 0.0], [rng.uniform(-2e-3, 2e-3), rng.uniform(-2e-3, 2e-3), 1.0]])
    T0 = np.array([[1, 0, -ax], [0, 1, -ay], [0, 0, 1.0]])
    T1 = np.array([[1, 0, (sw - 1) / 2.0], [0, 1, (sh - 1) / 2.0], [0, 0, 1.0]])
    integer = rng.random() < 0.25
    reach = rng.uniform(0.15, 0.6) * max(dw, 2) * (1.0 if rng.random() < 0.5 else -1.0)
    if horizon:
        A[2, 0], A[2, 1] = 1.0 / reach, 0.0
    elif integer:
        A = np.eye(3)
        A[:2, :2] = _QUARTER_TURNS[int(rng.integers(0, len(_QUARTER_TURNS)))]
        T0, T1 = np.round(T0), np.floor(T1)
    return T1 @ A @ T0


def _whole_view_inverse(rng, sw, sh, dw, dh, interp):
    """canvas px -> camera px of a camera that sees the WHOLE canvas: every coordinate an inlier (sw, sh >= 4), mirrored or not."""
    m = []
    for n_src, n_dst in ((sw, dw), (sh, dh)):
        lo, hi = 0.25, n_src - (2.25 if interp == LINEAR else 1.25)
        a, b = sorted(rng.uniform(lo, hi, 2))
        if rng.random() < 0.5:
            a, b = b, a
        m.append(((b - a) / max(n_dst - 1, 1), a))
    return np.array([[m[0][0], 0, m[0][1]], [0, m[1][0], m[1][1]], [0, 0, 1.0]])


def _no_view_inverse(rng):
    """A camera that sees nothing of the canvas: a shift far beyond every frame."""
    return np.array([[1.0, 0, 5000.0 + rng.uniform(0, 100)], [0, 1.0, -3000.0 - rng.uniform(0, 100)], [0, 0, 1.0]])


def view_inverses(view, mseed, n, sw, sh, dsize, interp):
    """(n, 3, 3): the inverse matrices of one camera, one per frame of its map; frames after the first are the first one jittered."""
    rng = np.random.default_rng(mseed)
    dw, dh = dsize
    if view == "whole":
        M = _whole_view_inverse(rng, sw, sh, dw, dh, interp)
    elif view == "none":
        M = _no_view_inverse(rng)
    elif view == "window":
        M = np.linalg.inv(_random_homography(rng, sw, sh, dw, dh))
    else:
        M = _part_view_inverse(rng, sw, sh, dw, dh, horizon=view == "horizon")
    out = [M]
    for i in range(1, n):
        if view == "whole":  # (a whole view stays one: a draw of its own per frame)
            out.append(_whole_view_inverse(rng, sw, sh, dw, dh, interp))
        else:
            out.append(M + np.array([[rng.uniform(-0.02, 0.02), 0, rng.uniform(-2, 2)], [0, rng.uniform(-0.02, 0.02), rng.uniform(-2, 2)], [0, 0, 0]]))
    return np.stack(out)


# ---- draws ----------------------------------------------------------------------------------------------------------------------------------

def _dim(rng, hi, even=False, lo=1):
    small = rng.random() < 0.2
    if even:
        return 2 * int(rng.integers(max(1, (lo + 1) // 2), 4 if small else hi // 2 + 1))
    return int(rng.integers(lo, max(lo + 1, 7) if small else hi + 1))


def _canvas(rng, even=False):
    return _dim(rng, 130, even), _dim(rng, 40, even)


def _seed(rng):
    return int(rng.integers(0, 2 ** 31))


def _border(rng, c):
    return tuple(int(v) for v in rng.integers(1, 256, c))


def _layout(rng, on):
    """The draws of a case that runs on padded, offset and guarded memory (None: compact tensors the entry allocates)."""
    if not on:
        return None
    return rec(offset=int(rng.integers(0, 5)), pad_rows=int(rng.integers(1, 4)), pad=int(rng.integers(0, 40)), align=int(rng.choice([0, 4, 16])),
               pads=tuple(int(v) for v in rng.integers(1, 24, 3)))


def _lens(rng, kinds):
    """A lens record: model pinhole | rational (lens A or B, r2_max default or inf) | fisheye (coefficients K_TEST times kscale; theta_max is
    the angle of the ray of canvas pixel `at`, given as fractions of the canvas: part of the canvas is beyond it, that pixel is on it;
    horizon: the rays of part of the canvas point backwards, and theta_max is then that angle if it is beyond 1.6, else 2.2)."""
    model = str(rng.choice(kinds))
    if model == "pinhole":
        return rec(model=model)
    if model == "rational":
        return rec(model=model, name=str(rng.choice(["A", "B"])), r2_inf=bool(rng.random() < 0.5))
    return rec(model=model, kscale=float(rng.choice([0.0, 0.5, 1.0, 2.0])), at=(float(rng.random()), float(rng.random())), horizon=bool(rng.random() < 0.25))


def _view(rng, lens):
    return "horizon" if lens.model == "fisheye" and lens.horizon else "part"


def _lens_case(rng, on):
    dtype = str(rng.choice(["u8", "f32"]))
    c = int(rng.integers(1, 5))
    B = int(rng.choice(BATCHES))
    lens = _lens(rng, ["rational", "fisheye"])
    return rec(sw=_dim(rng, 96), sh=_dim(rng, 64), dsize=_canvas(rng), B=B, dtype=dtype, c=c, interp=int(rng.integers(0, 2)),
               mode=int(rng.choice([RR.CONSTANT, RR.TRANSPARENT])), n_m=int(rng.choice([1, B])), lens=lens, view=_view(rng, lens), mseed=_seed(rng), dseed=_seed(rng),
               border=_border(rng, c), layout=_layout(rng, on))


def _map_case(rng, on):
    user = str(rng.choice(MAP_USERS, p=[0.3, 0.14, 0.14, 0.14, 0.14, 0.14]))  # (remap has the most formats: both types, 1..4 channels, six borders)
    nv12_in, nv12_out, planes = user.startswith("remap_nv12"), user.endswith("to_nv12"), user.endswith("planar")
    dtype, c = ("u8", 3) if user != "remap" else (str(rng.choice(["u8", "f32"])), int(rng.integers(1, 5)))
    B = int(rng.choice(BATCHES))
    lens = _lens(rng, ["pinhole", "rational", "fisheye"])
    modes = RR.MODES if user in ("remap", "remap_nv12") else RR.MODES[:5]
    return rec(user=user, sw=_dim(rng, 96, nv12_in), sh=_dim(rng, 64, nv12_in), dsize=_canvas(rng, nv12_out), B=B, dtype=dtype, c=c, interp=int(rng.integers(0, 2)),
               mode=RR.TRANSPARENT if (len(modes) == 6 and rng.random() < 0.3) else int(rng.choice(modes[:5])), n_m=int(rng.choice([1, B])), lens=lens,
               view=_view(rng, lens), mseed=_seed(rng), dseed=_seed(rng), border=_border(rng, c), rgb=bool(rng.random() < 0.5) and user != "remap_nv12_to_nv12" and user not in ("remap", "remap_to_planar"),
               plane=str(rng.choice(["f32", "f16", "bf16"])) if planes else None, sb=int(rng.integers(0, len(SCALES))), layout=_layout(rng, on))


def _nv12_case(rng, on):
    entry = str(rng.choice(NV12_ENTRIES))
    nv12_in, nv12_out = "nv12" in entry.replace("to_nv12", ""), entry.endswith("to_nv12")
    dtype, c = ("u8", 3) if entry != "warp_to_planar" else (str(rng.choice(["u8", "f32"])), int(rng.integers(1, 5)))
    B = int(rng.choice(BATCHES))
    return rec(entry=entry, sw=_dim(rng, 96, nv12_in), sh=_dim(rng, 64, nv12_in), dsize=_canvas(rng, nv12_out), B=B, dtype=dtype, c=c, interp=int(rng.integers(0, 2)),
               n_m=int(rng.choice([1, B])), view=str(rng.choice(["window", "part"])), mseed=_seed(rng), dseed=_seed(rng), border=_border(rng, c),
               rgb=bool(rng.random() < 0.5) and entry not in ("warp_nv12_to_nv12", "warp_to_planar"),
               plane=str(rng.choice(["f32", "f16", "bf16"])) if entry.endswith("planar") else None, sb=int(rng.integers(0, len(SCALES))), layout=_layout(rng, on))


def _gain(rng):
    r = rng.random()
    return 0.0 if r < 0.12 else 1.0 if r < 0.24 else 1023 / 256 if r < 0.36 else float(rng.uniform(0.25, 3.0))


def _stitch_case(rng, on):
    entry = str(rng.choice(STITCH_ENTRIES))
    nv12_in, nv12_out = entry.startswith("nv12"), entry.endswith("to_nv12")
    gained = entry != "warp_stitch" and bool(rng.random() < 0.5)
    dtype, c = ("u8", 3) if (gained or entry not in ("warp_stitch", "maps")) else (str(rng.choice(["u8", "f32"])), int(rng.integers(1, 5)))
    B = int(rng.choice(BATCHES))
    interp = int(rng.integers(0, 2))
    r = rng.random()
    scene = "all" if r < 1 / 8 else "blind" if r < 2 / 8 else "mixed"
    n = int(rng.choice([2, 5, 8, 8])) if scene == "all" else int(rng.integers(1, 9))
    blind = int(rng.integers(0, n)) if scene == "blind" else -1
    cams = []
    for k in range(n):
        lens = rec(model="pinhole") if (entry == "warp_stitch" or scene == "all") else _lens(rng, ["pinhole", "pinhole", "rational", "fisheye"])
        view = "whole" if scene == "all" else "none" if k == blind else _view(rng, lens)
        lo = 4 if scene == "all" else 1
        cams.append(rec(sw=_dim(rng, 96, nv12_in, lo), sh=_dim(rng, 64, nv12_in, lo), lens=lens, view=view, n_m=int(rng.choice([1, 1, B])), mseed=_seed(rng), dseed=_seed(rng),
                        gain=tuple(_gain(rng) for _ in range(3)) if gained else None))
    feather = int(rng.choice(FEATHERS)) if rng.random() < 0.6 else 0  # (0: OVER)
    return rec(entry=entry, cams=tuple(cams), dsize=_canvas(rng, nv12_out), B=B, dtype=dtype, c=c, interp=interp, feather=feather,
               mode=int(rng.choice([RR.CONSTANT, RR.TRANSPARENT])) if entry in ("warp_stitch", "maps", "nv12") else RR.CONSTANT, border=_border(rng, c),
               rgb=bool(rng.random() < 0.5) and entry in ("nv12", "to_nv12", "nv12_planes"), plane=str(rng.choice(["f32", "f16", "bf16"])) if "planes" in entry else None,
               sb=int(rng.integers(0, len(SCALES))), layout=_layout(rng, on))


_DRAW = {"lens": _lens_case, "map": _map_case, "nv12": _nv12_case, "stitch": _stitch_case}


def cases(family, seed):
    """The N_CASES case records of (family, seed); the cases with an odd index + seed run on padded, offset, guarded memory."""
    rng = np.random.default_rng(_FAMILY_BASE[family] + seed)
    return [Case(family, seed, i, _DRAW[family](rng, (i + seed) % 2 == 1)) for i in range(N_CASES)]


# ---- the arrays of a case ---------------------------------------------------------------------------------------------------------------------

def map_frame(n_m, b):
    """The frame of a camera's map (or the matrix of a call) that serves frame b of the batch: its own, or the shared one."""
    return b if n_m > 1 else 0


def _frames(dseed, B, sh, sw, dtype, c, nv12):
    """(B, sh, sw, c) uint8 / float32 frames, or NV12 planes ((B, sh, sw), (B, sh / 2, sw / 2, 2))."""
    rng = np.random.default_rng(dseed)
    if nv12:
        return rng.integers(0, 256, (B, sh, sw), dtype=np.uint8), rng.integers(0, 256, (B, sh // 2, sw // 2, 2), dtype=np.uint8)
    return rng.integers(0, 256, (B, sh, sw, c), dtype=np.uint8) if dtype == "u8" else rng.random((B, sh, sw, c), dtype=np.float32)


def fisheye_K(sw, sh):
    """The camera matrix the fisheye cameras use for a (sw, sh) source: about 130 degrees across the frame's width."""
    return np.array([[0.45 * sw, 0, (sw - 1) / 2], [0, 0.47 * sw, (sh - 1) / 2 + 1], [0, 0, 1.0]])


@dataclasses.dataclass
class Camera:
    """One camera of a case on the host.  Minv (n_m, 3, 3): canvas px -> (undistorted) camera px.  model pinhole: R is Minv and lens None;
    else R holds the ray matrices and lens the 12 values of the model's lens12; guard is r2_max or theta_max."""
    sw: int
    sh: int
    frames: object
    Minv: np.ndarray
    model: str
    K: object = None
    dist: object = None
    R: object = None
    lens: object = None
    guard: float = np.inf
    gain: object = None
    M: object = None  # (the NV12 family: the forward matrices the entry is given; Minv is the oracle's inverse of each)

    @property
    def n_m(self):
        return len(self.Minv)


def _camera(r, dsize, interp, B, dtype, c, nv12, n_m=None, view=None):
    Minv = view_inverses(view or r.view, r.mseed, n_m or r.n_m, r.sw, r.sh, dsize, interp)
    cam = Camera(r.sw, r.sh, _frames(r.dseed, B, r.sh, r.sw, dtype, c, nv12), Minv, r.lens.model if hasattr(r, "lens") else "pinhole", R=Minv,
                 gain=getattr(r, "gain", None))
    if cam.model == "rational":
        cam.K, cam.dist = LR.camera_K(r.sw, r.sh), LENSES[r.lens.name]
        cam.R = np.stack([LR.ray_matrix(M, cam.K, inverse_given=True) for M in Minv])
        cam.lens, cam.guard = LR.lens12(cam.K, cam.dist), (np.inf if r.lens.r2_inf else LR.lens_valid_r2(cam.dist))
    elif cam.model == "fisheye":
        cam.K, cam.dist = fisheye_K(r.sw, r.sh), tuple(r.lens.kscale * k for k in FR.K_TEST)
        cam.R = np.stack([FR.ray_matrix(M, cam.K, inverse_given=True) for M in Minv])
        cam.lens = FR.lens12(cam.K, cam.dist)
        theta = FR.chain(dsize, cam.R[0], cam.lens)[2]
        t = float(theta[min(int(r.lens.at[1] * dsize[1]), dsize[1] - 1), min(int(r.lens.at[0] * dsize[0]), dsize[0] - 1)])
        cam.guard = t if np.isfinite(t) else np.inf
        if r.lens.horizon and not t > 1.6:  # (rays behind the camera stay valid up to 126 degrees)
            cam.guard = 2.2
    return cam


@functools.lru_cache(maxsize=64)
def inputs(case):
    """The cameras of a case (one for the single-camera families)."""
    p = case.p
    if case.family == "stitch":
        return [_camera(r, p.dsize, p.interp, p.B, p.dtype, p.c, p.entry.startswith("nv12")) for r in p.cams]
    name = p.user if case.family == "map" else p.entry if case.family == "nv12" else ""
    cam = _camera(p, p.dsize, p.interp, p.B, p.dtype, p.c, "nv12" in name.replace("to_nv12", ""), p.n_m, p.view)
    if case.family == "nv12":
        cam.M = np.stack([np.linalg.inv(M) for M in cam.Minv])
        cam.Minv = cam.R = np.stack([co.invert3x3(M) for M in cam.M])
    return [cam]


def blend_of(p):
    return (SM.FEATHER, p.feather) if p.feather else (SM.OVER, 64)


def gains_of(case):
    """(n_cams, 3) floats, or None."""
    g = [r.gain for r in case.p.cams]
    return None if g[0] is None else np.array(g)


def canvas_of(case):
    """What a TRANSPARENT destination holds before the call: CANVAS in a layout case, zeros in a compact one."""
    return CANVAS if case.p.layout is not None else 0


# ---- the maps of a case, from the definitions ---------------------------------------------------------------------------------------------------

def camera_map(cam, i, dsize, interp):
    """(xy, frac) of frame i of a camera's map: remap_ref.build / fisheye_ref.build."""
    if cam.model == "pinhole":
        return RR.build(dsize, cam.Minv[i], interp=interp)
    if cam.model == "rational":
        return RR.build(dsize, cam.R[i], cam.lens, cam.guard, interp)
    return FR.build(dsize, cam.R[i], cam.lens, cam.guard, interp)


def maps_of(case):
    """Per camera, the list of its map's frames [(xy, frac), ...]."""
    return [[camera_map(cam, i, case.p.dsize, case.p.interp) for i in range(cam.n_m)] for cam in inputs(case)]


# ---- expected results ---------------------------------------------------------------------------------------------------------------------------

def _fr(cam, b, nv12):
    return (cam.frames[0][b], cam.frames[1][b]) if nv12 else cam.frames[b]


def _sb(p, c=3):
    return SCALES[p.sb][:c], BIASES[p.sb][:c]


def _expected_lens(case, b):
    p, cam = case.p, inputs(case)[0]
    dw, dh = p.dsize
    i = map_frame(cam.n_m, b)
    canvas = np.full((dh, dw, p.c), canvas_of(case), cam.frames.dtype)
    warp = LR.warp if cam.model == "rational" else FR.warp
    return warp(cam.frames[b], cam.R[i], cam.lens, cam.guard, p.dsize, p.interp, p.mode, p.border, canvas)


def _expected_map(case, b):
    p, cam = case.p, inputs(case)[0]
    dw, dh = p.dsize
    xy, frac = maps_of(case)[0][map_frame(cam.n_m, b)]
    scale, bias = _sb(p)
    if p.user == "remap":
        return RR.remap(cam.frames[b], xy, frac, p.interp, p.mode, p.border, np.full((dh, dw, p.c), canvas_of(case), cam.frames.dtype))
    if p.user == "remap_nv12":
        return RN.remap_nv12(*_fr(cam, b, True), xy, frac, p.interp, p.mode, p.border, np.full((dh, dw, 3), canvas_of(case), np.uint8), p.rgb)
    if p.user == "remap_to_nv12":
        return RNO.remap_to_nv12(cam.frames[b], xy, frac, p.interp, p.mode, p.border, p.rgb)
    if p.user == "remap_nv12_to_nv12":
        return RNO.remap_nv12_to_nv12(*_fr(cam, b, True), xy, frac, p.interp, p.mode, p.border)
    if p.user == "remap_to_planar":
        return MP.remap_planes(cam.frames[b], xy, frac, p.interp, p.mode, scale, bias, p.border)
    return RN.remap_nv12_planes(*_fr(cam, b, True), xy, frac, p.interp, p.mode, scale, bias, p.border, p.rgb)


def _expected_nv12(case, b):
    p, cam = case.p, inputs(case)[0]
    M = cam.M[map_frame(cam.n_m, b)]  # (the forward matrix: the definition inverts it, as the entry does)
    kw = dict(border_value=list(p.border))
    scale, bias = _sb(p, p.c)
    if p.entry == "warp_perspective_nv12":
        return NR.warp_nv12(*_fr(cam, b, True), M, p.dsize, p.interp, rgb=p.rgb, **kw)
    if p.entry == "warp_nv12_to_planar":
        return RN.planes_f32(NR.warp_nv12(*_fr(cam, b, True), M, p.dsize, p.interp, rgb=p.rgb, **kw), scale, bias)
    if p.entry == "warp_perspective_to_nv12":
        return NO.warp_to_nv12(cam.frames[b], M, p.dsize, p.interp, rgb=p.rgb, **kw)
    if p.entry == "warp_nv12_to_nv12":
        return NO.warp_nv12_to_nv12(*_fr(cam, b, True), M, p.dsize, p.interp, **kw)
    return P16.planes_f32(cam.frames[b], M, p.dsize, p.interp, scale, bias, list(p.border))


def _expected_stitch(case, b):
    p, cams = case.p, inputs(case)
    dw, dh = p.dsize
    blend, F = blend_of(p)
    nv12 = p.entry.startswith("nv12")
    srcs = [_fr(cam, b, nv12) for cam in cams]
    if p.entry == "warp_stitch":
        return SR.stitch(srcs, [cam.Minv[map_frame(cam.n_m, b)] for cam in cams], p.dsize, p.interp, blend, F, p.mode, p.border,
                         np.full((dh, dw, p.c), canvas_of(case), srcs[0].dtype))[0]
    maps = [m[map_frame(len(m), b)] for m in maps_of(case)]
    scale, bias = _sb(p)
    canvas = np.full((dh, dw, p.c), canvas_of(case), np.uint8 if p.dtype == "u8" else np.float32)
    ys, uvs = ([s[0] for s in srcs], [s[1] for s in srcs]) if nv12 else (None, None)
    gains = gains_of(case)
    if gains is None:
        if p.entry == "maps":
            return SM.stitch(srcs, maps, p.interp, blend, F, p.mode, p.border, canvas)[0]
        if p.entry == "nv12":
            return SM.stitch_nv12(ys, uvs, maps, p.interp, blend, F, p.mode, p.border, canvas, p.rgb)[0]
        if p.entry == "to_nv12":
            return RNO.stitch_to_nv12(srcs, maps, p.interp, blend, F, p.border, p.rgb)
        if p.entry == "nv12_to_nv12":
            return RNO.stitch_nv12_to_nv12(ys, uvs, maps, p.interp, blend, F, p.border)
        if p.entry == "planes":
            return MP.stitch_planes(srcs, maps, p.interp, scale, bias, blend, F, p.border)
        return MP.stitch_nv12_planes(ys, uvs, maps, p.interp, scale, bias, blend, F, p.border, p.rgb)
    G = SG.quantize(gains, len(cams))
    if p.entry == "maps":
        return SG.stitch(srcs, G, maps, p.interp, blend, F, p.mode, p.border, canvas)[0]
    if p.entry == "nv12":
        return SG.stitch_nv12(ys, uvs, G, maps, p.interp, blend, F, p.mode, p.border, canvas, p.rgb)[0]
    if p.entry == "to_nv12":
        return SG.stitch_to_nv12(srcs, G, maps, p.interp, blend, F, p.border, p.rgb)
    if p.entry == "nv12_to_nv12":
        return SG.stitch_nv12_to_nv12(ys, uvs, G, maps, p.interp, blend, F, p.border)
    if p.entry == "planes":
        return SG.stitch_planes(srcs, G, maps, p.interp, scale, bias, blend, F, p.border)
    return SG.stitch_nv12_planes(ys, uvs, G, maps, p.interp, scale, bias, blend, F, p.border, p.rgb)


_EXPECTED = {"lens": _expected_lens, "map": _expected_map, "nv12": _expected_nv12, "stitch": _expected_stitch}


def kind_of_result(case):
    """"pixels" ((dh, dw, C) of the source's type), "nv12" (a (y, uv) pair) or "planes" ((C, dh, dw) float32, to be rounded to case.p.plane)."""
    name = case.p.user if case.family == "map" else case.p.entry if case.family in ("nv12", "stitch") else ""
    return "nv12" if name.endswith("to_nv12") else "planes" if (name.endswith("planar") or "planes" in name) else "pixels"


def expected(case):
    """The expected result of every frame of the batch, in kind_of_result's form."""
    out = []
    for b in range(case.p.B):
        e = _EXPECTED[case.family](case, b)
        if kind_of_result(case) == "pixels":
            e = np.asarray(e).reshape(case.p.dsize[1], case.p.dsize[0], case.p.c)
        out.append(e)
    return out


# ---- census ---------------------------------------------------------------------------------------------------------------------------------

def census(case):
    """A dict of counts, from the definitions alone.
    cover[n]            canvas pixels (of every frame) covered by n cameras (stitch)
    left0, left_last    bilinear inliers whose left tap is column 0 / column src_w - 2
    clipped, unclipped  covering FEATHER weights with d >= F / d < F
    frac0               bilinear inliers with both fractions 0
    entries, sentinels  per lens or fisheye map (one list element each): its entries and how many of them are the sentinel
    behind              valid fisheye entries whose ray has W <= 0
    taps, saturated     gained cases: source samples, and how many the gain takes to 255
    gain0, gain_max     the case has a channel gain of 0 / of 1023 / 256
    nv12_2px            the case has an NV12 source 2 px wide
    writes_nothing      the launch writes no pixel at all"""
    p, cams, maps = case.p, inputs(case), maps_of(case)
    out = dict(cover=np.zeros(9, np.int64), left0=0, left_last=0, clipped=0, unclipped=0, frac0=0, lens_maps=[], behind=0, taps=0, saturated=0, gain0=False,
               gain_max=False, nv12_2px=False, writes_nothing=False)
    count = np.zeros((p.B, p.dsize[1], p.dsize[0]), np.int64)
    for cam, frames in zip(cams, maps):
        for i, (xy, frac) in enumerate(frames):
            inl = RR.written(xy, cam.sw, cam.sh, p.interp)
            if cam.n_m > 1:
                count[i] += inl
            else:
                count += inl[None]
            sent = (xy[..., 0] == RR.SENTINEL) & (xy[..., 1] == RR.SENTINEL)
            if cam.model != "pinhole":
                out["lens_maps"].append((int(sent.sum()), sent.size))
            if cam.model == "fisheye":
                out["behind"] += int((~sent & (FR.rays(p.dsize, cam.R[i])[2] <= 0)).sum())
            if p.interp == LINEAR:
                sx = xy[..., 0].astype(np.int64)
                out["left0"] += int((inl & (sx == 0)).sum())
                out["left_last"] += int((inl & (sx == cam.sw - 2)).sum())
                out["frac0"] += int((inl & (frac == 0)).sum())
            if case.family == "stitch" and p.feather:
                d = SR.edge_distance(xy[..., 0].astype(np.int64), xy[..., 1].astype(np.int64), cam.sw, cam.sh)
                out["clipped"] += int((inl & (d >= p.feather)).sum())
                out["unclipped"] += int((inl & (d < p.feather)).sum())
        if isinstance(cam.frames, tuple) and cam.sw == 2:
            out["nv12_2px"] = True
        if cam.gain is not None:
            G = SG.quantize([cam.gain], 1)[0]
            f = cam.frames if not isinstance(cam.frames, tuple) else np.stack([NR.nv12_to_bgr(y, uv, p.rgb) for y, uv in zip(*cam.frames)])
            out["taps"] += f.size
            out["saturated"] += int((SG.gain(f, G) >= 255).sum())
            out["gain0"] |= bool((G == 0).any())
            out["gain_max"] |= bool((G == 1023).any())
    if case.family == "stitch":
        out["cover"] = np.bincount(count.ravel(), minlength=9)
    out["writes_nothing"] = getattr(p, "mode", RR.CONSTANT) == RR.TRANSPARENT and not count.any()
    return out
