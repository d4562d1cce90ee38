"""The float-domain cases of the lens warp, the map sampler and the multi-camera warp -- TEST INFRASTRUCTURE ONLY, a plain module like
tests/pixels.py.  tests/test_gpu_float_domain.py runs them on the device, tests/test_float_domain_cpu.py checks without one that no case
passes vacuously and that every case set tells the mutants of its docstring apart.

A case is a source (tests/pixels.py: float_frame's three kinds, and "blocks" -- zero_block_frame, bilinear only), a geometry of the
family's own GPU module, and what the family's numpy reference gives on a canvas of CANVAS_BITS.  expected() of each family returns

    exp        the reference's result
    computed   (dh, dw) bool: the pixels whose value the definition COMPUTES (a bilinear blend, a FEATHER mean).  They are compared with
               same_float(payload=False): identical bits wherever the reference has no NaN, some NaN where it has one
    kept       (dh, dw) bool: the pixels a launch must not write (BORDER_TRANSPARENT)
    many       (dh, dw) bool: the pixels a FEATHER mean is taken at (two or more covering cameras); all False in the other families

Every pixel outside `computed` is a copy -- nearest neighbour, a border fill, an OVER pixel or a single cover under nearest, the canvas --
and is compared with same_float(payload=True): all 32 bits, NaN payloads and signalling NaNs included."""
import functools

import numpy as np

from oracle import warp_numpy as wn
from tests import border_ref as BR
from tests import lens_ref as LR
from tests import pixels as PX
from tests import remap_ref as RR
from tests import stitch_ref as SR
from tests.test_lens_cpu import GEOMS  # (tests/test_gpu_lens.py's and tests/test_gpu_remap.py's)

NEAREST, LINEAR = wn.NEAREST, wn.LINEAR
INF = float("inf")
CANVAS_BITS = 0xff9c0de5  # a signalling NaN that tests/pixels.py's SPECIALS do not hold: what a launch leaves alone is known by its bits
SNAN_BITS = 0x7fa00123    # SPECIALS' signalling NaN
MINUS_ZERO = 0x80000000
KINDS = PX.KINDS + ("blocks",)
LENSES = {"A": LR.LENS_A, "B": LR.LENS_B}
LENS_SETUPS = (("rotated_zoom_out", "A"), ("brno", "A"), ("brno", "B"))  # both geometries with lens A, lens B on one
REMAP_SETUPS = (("rotated_zoom_out", "pinhole"), ("brno", "A"))  # a footprint that leaves the frame on all four sides; a map with sentinels
TINY_SOURCES = ((2, 2), (1, 5))  # (h, w)
TINY_DSIZE = (29, 21)
TINY_MINV = np.array([[0.37, -0.21, -3.0], [0.18, 0.41, -2.5], [0.0005, 0.0, 1.0]])  # tests/test_gpu_lens.py::test_widths_and_tiny_sources'
BLENDS = (("over", 64), ("feather", 1), ("feather", 3), ("feather", 64))  # tests/test_gpu_stitch.py's
REMAP_SEED = 2003  # (2000: the pixel every sentinel reads under REFLECT_101 is a NaN in one frame -- 14 % of that result)
UNIQUE = 3  # distinct frames of a remap batch: frame g is frame g % 3, so each of them is walked first and second in an item of two


def kinds(interp):
    return KINDS if interp == LINEAR else PX.KINDS


def canvas(shape):
    return np.full(shape, CANVAS_BITS, np.uint32).view(np.float32)


def frame(kind, seed, h, w, c):
    """(h, w, c) float32, (h, w) for c = 0.  "blocks": squares of a fifth of the shorter side (8 at least)."""
    n = max(c, 1)
    f = PX.zero_block_frame(seed, h, w, n, block=max(8, min(h, w) // 5)) if kind == "blocks" else PX.float_frame(kind, seed, h, w, n)
    return f[:, :, 0] if c == 0 else f


def seed(base, kind, c, i=0):
    return base + 100 * KINDS.index(kind) + 10 * c + i


def border(c):
    return PX.BORDER[:max(c, 1)]


def _px(a, dh, dw):
    return np.asarray(a).reshape(dh, dw, -1)


def compare(got, exp, computed, what=""):
    """The two rules of this module's docstring."""
    dh, dw = computed.shape
    g, e = _px(got, dh, dw), _px(exp, dh, dw)
    try:
        PX.same_float(g[computed], e[computed], payload=False)
        PX.same_float(g[~computed], e[~computed], payload=True)
    except AssertionError as err:
        raise AssertionError("%s: %s" % (what, err)) from None


def preconditions(kind, interp, exp, computed, kept, many=None, feather=0, what=""):
    """What keeps a case from passing vacuously, from the reference alone.  The bounds are the issue's: NaNs in at most 10 % of the
    elements a launch writes; "tiny": at least 5 % of the computed elements subnormal; "huge" under FEATHER: at least 1 % of the means
    +-Inf; "mixed", nearest: a signalling NaN arrives; "blocks": at least 32 computed elements are -0.0.
    The 1 % of +-Inf holds for F = 3 and 64 (7-20 % of the means).  F = 1 is the plain mean: every weight is 1, so a sum overflows only
    where two pixels of one sign lie in the top binade -- 1 / 28 of the kind's exponents, and the 1 % of +-FLT_MAX -- which is 0.04-1.4 %
    of the means whatever the seed; float_frame("huge") cannot give 1 % there, and the case asks for one +-Inf at least."""
    dh, dw = computed.shape
    e = _px(exp, dh, dw)
    assert (PX.bits(e[kept]) == CANVAS_BITS).all() and not (PX.bits(e[~kept]) == CANVAS_BITS).any(), what
    assert (~kept).any(), what
    assert np.isnan(e[~kept]).mean() <= 0.10, (what, float(np.isnan(e[~kept]).mean()))
    if kind == "tiny" and computed.any():
        assert PX.is_subnormal(e[computed]).mean() >= 0.05, (what, float(PX.is_subnormal(e[computed]).mean()))
    if kind == "huge" and feather > 1:
        assert np.isinf(e[many]).mean() >= 0.01, (what, float(np.isinf(e[many]).mean()))
    if kind == "huge" and feather == 1:
        assert np.isinf(e[many]).any(), what
    if kind == "mixed" and interp == NEAREST:
        assert (PX.bits(e[~kept]) == SNAN_BITS).sum() >= 1, what
    if kind == "blocks":
        assert interp == LINEAR and (PX.bits(e[computed]) == MINUS_ZERO).sum() >= 32, (what, int((PX.bits(e[computed]) == MINUS_ZERO).sum()))


# ---- the lens warp ----

@functools.lru_cache(maxsize=None)
def lens_setup(geom, lens):
    """(sw, sh, dw, dh, M, K, dist, ray matrix, lens12, r2_max)."""
    sw, sh, dw, dh, M = GEOMS[geom]
    K = LR.camera_K(sw, sh)
    return sw, sh, dw, dh, M, K, LENSES[lens], LR.ray_matrix(M, K), LR.lens12(K, LENSES[lens]), LR.lens_valid_r2(LENSES[lens])


@functools.lru_cache(maxsize=None)
def tiny_lens_setup(sh, sw):
    """... of a source smaller than a tap window, through lens B; the matrix is the INVERSE one."""
    K = np.array([[6.0, 0, (sw - 1) / 2], [0, 6.0, (sh - 1) / 2], [0, 0, 1.0]])
    dw, dh = TINY_DSIZE
    return sw, sh, dw, dh, TINY_MINV, K, LR.LENS_B, LR.ray_matrix(TINY_MINV, K, inverse_given=True), LR.lens12(K, LR.LENS_B), LR.lens_valid_r2(LR.LENS_B)


def lens_expected(src, setup, interp, mode, border_value):
    sw, sh, dw, dh, _, _, _, R, l12, r2 = setup
    exp = LR.warp(src, R, l12, r2, (dw, dh), interp, mode, border_value=border_value, canvas=canvas((dh, dw) + src.shape[2:]))
    sx, sy, _, _, valid = LR.maps((dw, dh), R, l12, r2, interp)
    nothing = np.zeros((dh, dw), bool)
    if mode == LR.TRANSPARENT:
        written = LR.inliers(sx, sy, valid, sw, sh, interp)
        return exp, (written if interp == LINEAR else nothing), ~written, nothing
    all_out = ~valid | (sx >= sw) | (sx + 1 < 0) | (sy >= sh) | (sy + 1 < 0)
    return exp, (~all_out if interp == LINEAR else nothing), nothing, nothing


def lens_cases(geom, lens, kind, interp):
    """[(id, source, mode, border value or None)] of one parametrised test: both borders x channels 1-4 and an (H, W) image."""
    sw, sh = lens_setup(geom, lens)[:2]
    return [("%s-%s-%s-%d-mode%d-c%d" % (geom, lens, kind, interp, mode, c), frame(kind, seed(1000, kind, c), sh, sw, c), mode, border(c) if mode == LR.CONSTANT else None)
            for mode in (LR.CONSTANT, LR.TRANSPARENT) for c in (1, 2, 3, 4, 0)]


def tiny_lens_cases(sh, sw, interp):
    return [("src%dx%d-%s-%d-mode%d" % (sw, sh, kind, interp, mode), frame(kind, seed(1500 + 10 * sh + sw, kind, 3), sh, sw, 3), mode, border(3) if mode == LR.CONSTANT else None)
            for kind in PX.KINDS for mode in (LR.CONSTANT, LR.TRANSPARENT)]


# ---- the map sampler ----

@functools.lru_cache(maxsize=None)
def remap_setup(geom, kind):
    """(sw, sh, dw, dh, M, K, dist, matrix for remap_ref.build, lens12 or None, r2_max)."""
    sw, sh, dw, dh, M = GEOMS[geom]
    if kind == "pinhole":
        return sw, sh, dw, dh, M, None, None, wn.invert3x3(M), None, INF
    return lens_setup(geom, kind)


@functools.lru_cache(maxsize=None)
def ref_map(geom, kind, interp):
    _, _, dw, dh, _, _, _, R, l12, r2 = remap_setup(geom, kind)
    return RR.build((dw, dh), R, l12, r2, interp)


def remap_expected(src, xy, frac, interp, mode, border_value):
    sh, sw = src.shape[:2]
    dh, dw = xy.shape[:2]
    exp = RR.remap(src, xy, frac, interp, mode, border_value=0.0 if border_value is None else border_value, canvas=canvas((dh, dw) + src.shape[2:]))
    nothing = np.zeros((dh, dw), bool)
    written = RR.written(xy, sw, sh, interp)
    kept = ~written if mode == RR.TRANSPARENT else nothing
    if interp == NEAREST:
        return exp, nothing, kept, nothing
    if mode == RR.TRANSPARENT:
        return exp, written, kept, nothing
    if mode == RR.CONSTANT:  # all four taps outside: the border value itself, a copy
        sx, sy = xy[..., 0].astype(np.int64), xy[..., 1].astype(np.int64)
        return exp, ~((sx >= sw) | (sx + 1 < 0) | (sy >= sh) | (sy + 1 < 0)), kept, nothing
    return exp, ~nothing, kept, nothing


def remap_cases(geom, kind_of_map, kind, interp, channels=(1, 2, 3, 4)):
    """[(id, UNIQUE sources, mode, border value or None)]: all six borders x the channel counts (one list of sources per count)."""
    sw, sh = remap_setup(geom, kind_of_map)[:2]
    out = []
    for c in channels:
        srcs = [frame(kind, seed(REMAP_SEED, kind, c, i), sh, sw, c) for i in range(UNIQUE)]
        out += [("%s-%s-%s-%d-%s-c%d" % (geom, kind_of_map, kind, interp, BR.NAMES[mode], c), srcs, mode, border(c) if mode == RR.CONSTANT else None) for mode in RR.MODES]
    return out


def tiny_remap_cases(sh, sw, interp):
    return [("src%dx%d-%s-%d-%s" % (sw, sh, kind, interp, BR.NAMES[mode]), frame(kind, seed(2500 + 10 * sh + sw, kind, 3), sh, sw, 3), mode, border(3) if mode == RR.CONSTANT else None)
            for kind in PX.KINDS for mode in RR.MODES]


@functools.lru_cache(maxsize=None)
def tiny_map(interp):
    """The pinhole map of TINY_MINV: 29 x 21 entries around and far outside a source of a few pixels."""
    return RR.build(TINY_DSIZE, TINY_MINV, None, INF, interp)


def remap_batch(tiles_per_frame, fill=4096):
    """The smallest odd batch whose groups of two frames still make `fill` items (bev_amd/csrc/host_plan.h plan_remap): the last group
    is short.  The GPU module asks the plan itself whether it keeps more than one frame per item."""
    return 2 * -(-fill // tiles_per_frame) - 1


# ---- the multi-camera warp ----

def stitch_scene():
    from tests.test_gpu_stitch import DSIZE, SCENE
    return SCENE, DSIZE


def stitch_sources(kind, c):
    scene, _ = stitch_scene()
    return [frame(kind, seed(3000, kind, c, k), h, w, c) for k, (w, h, _) in enumerate(scene)]


def stitch_expected(srcs, interp, blend, feather, mode, border_value):
    scene, dsize = stitch_scene()
    dw, dh = dsize
    exp, count = SR.stitch(srcs, [M for _, _, M in scene], dsize, interp, SR.FEATHER if blend == "feather" else SR.OVER, feather, mode,
                           0.0 if border_value is None else border_value, canvas((dh, dw) + srcs[0].shape[2:]))
    nothing = np.zeros((dh, dw), bool)
    many = count >= 2 if blend == "feather" else nothing
    return exp, (count >= 1 if interp == LINEAR else many), (count == 0 if mode == SR.TRANSPARENT else nothing), many, count


def stitch_cases(kind, interp):
    """[(id, sources, blend, F, mode, border value or None)]: the four blends x both borders x channels 1-4."""
    out = []
    for c in (1, 2, 3, 4):
        srcs = stitch_sources(kind, c)
        out += [("stitch-%s-%d-%s%d-mode%d-c%d" % (kind, interp, blend, F, mode, c), srcs, blend, F, mode, border(c) if mode == SR.CONSTANT else None)
                for blend, F in BLENDS for mode in (SR.CONSTANT, SR.TRANSPARENT)]
    return out
