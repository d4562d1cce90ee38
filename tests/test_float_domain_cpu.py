"""The float-domain cases of tests/float_domain.py without a device: the references they are judged by tied to each other by bits on the
same frames, the preconditions that keep a case from passing vacuously, and the argument for the cases -- eight faults a float32 kernel
can have, each switched on in a COPY of the references' arithmetic (never in the product), must make tests/float_domain.compare fail on
at least one committed case of every family the fault exists in.

  (a) a zero-weight tap skipped                    (e) a single cover under FEATHER computed as (w p) / w
  (b) subnormal inputs and results flushed to zero (f) outside taps / uncovered pixels substituted by a 0 / 1 mask multiply, not a select
  (c) FEATHER's accumulator started from the first product instead of +0
  (d) FEATHER's division as a multiply by the float32 reciprocal
  (g) the four-tap sum associated as (t00 + t10) + (t01 + t11)      (h) nearest passed through x * 1.0f

Recorded, not gated (test_unit_interval_frames_record prints it; pytest -s shows it): the same faults on the [0, 1) frames the three families' own GPU modules
use (rng.random, assert_array_equal), same geometries, 3 channels, all borders and blends.  "-" is a fault those frames do NOT show:

    fault   lens   remap   stitch
    (a)      -       -       -        a skipped tap has weight 0: it adds +0 to a sum that is not -0
    (b)      -       -       -        no subnormal among products of [0, 1) values and weights >= 1 / 1024
    (c)                      -        differs from the definition in the sign of zero only
    (d)                      x
    (e)                      x
    (f)      -       -       -        finite pixels: v * 0 + border * 1 is the border value
    (g)      x       x       x
    (h)      -       -       -        no NaN to quiet

On the committed cases every entry is "x"."""
import fractions

import numpy as np
import pytest

from oracle import warp_numpy as wn
from tests import border_ref as BR
from tests import float_domain as FD
from tests import lens_ref as LR
from tests import pixels as PX
from tests import remap_ref as RR
from tests import stitch_ref as SR

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")  # (numpy's: the references compute 0 * Inf and overflow on purpose)

NEAREST, LINEAR, INF = FD.NEAREST, FD.LINEAR, FD.INF
F32 = np.float32
FAULTS = {"a": ("lens", "remap", "stitch"), "b": ("lens", "remap", "stitch"), "c": ("stitch",), "d": ("stitch",), "e": ("stitch",),
          "f": ("lens", "remap", "stitch"), "g": ("lens", "remap", "stitch"), "h": ("lens", "remap", "stitch")}


# ---- 1. no case passes vacuously: the preconditions, from the references alone ----

@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
@pytest.mark.parametrize("setup", FD.LENS_SETUPS, ids=["-".join(s) for s in FD.LENS_SETUPS])
def test_lens_cases_preconditions(setup, interp):
    st = FD.lens_setup(*setup)
    for kind in FD.kinds(interp):
        for cid, src, mode, bv in FD.lens_cases(setup[0], setup[1], kind, interp):
            exp, computed, kept, _ = FD.lens_expected(src, st, interp, mode, 0.0 if bv is None else bv)
            FD.preconditions(kind, interp, exp, computed, kept, what=cid)
            assert (mode == LR.TRANSPARENT) == bool(kept.any()) and computed.any() == (interp == LINEAR), cid


@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
@pytest.mark.parametrize("setup", FD.REMAP_SETUPS, ids=["-".join(s) for s in FD.REMAP_SETUPS])
def test_remap_cases_preconditions(setup, interp):
    xy, frac = FD.ref_map(setup[0], setup[1], interp)
    sw, sh = FD.remap_setup(*setup)[:2]
    sentinels = (xy == RR.SENTINEL).all(axis=-1)
    assert bool(sentinels.any()) == (setup[1] != "pinhole")
    sx, sy = xy[..., 0].astype(int), xy[..., 1].astype(int)
    if setup[1] == "pinhole":  # the footprint leaves the frame on all four sides
        assert (sx < -1).any() and (sx > sw).any() and (sy < -1).any() and (sy > sh).any()
    for kind in FD.kinds(interp):
        for cid, srcs, mode, bv in FD.remap_cases(setup[0], setup[1], kind, interp):
            for i, src in enumerate(srcs):
                exp, computed, kept, _ = FD.remap_expected(src, xy, frac, interp, mode, bv)
                FD.preconditions(kind, interp, exp, computed, kept, what="%s frame %d" % (cid, i))
            assert not any(np.array_equal(PX.bits(a), PX.bits(b)) for a, b in ((srcs[0], srcs[1]), (srcs[0], srcs[2]), (srcs[1], srcs[2])))


@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_stitch_cases_preconditions(interp):
    scene, (dw, dh) = FD.stitch_scene()
    for kind in FD.kinds(interp):
        for cid, srcs, blend, F, mode, bv in FD.stitch_cases(kind, interp):
            exp, computed, kept, many, count = FD.stitch_expected(srcs, interp, blend, F, mode, bv)
            for n in range(4):  # the case cannot pass on an empty overlap
                assert (count == n).sum() >= 40, (cid, n, int((count == n).sum()))
            FD.preconditions(kind, interp, exp, computed, kept, many, F if blend == "feather" else 0, what=cid)
        if kind == "blocks":  # a -0.0 square of every camera lies where two or more cameras cover
            _, _, _, _, count = FD.stitch_expected(srcs, interp, "feather", 64, SR.TRANSPARENT, None)
            for src, (w, h, Minv) in zip(srcs, scene):
                alone = BR.warp(src, Minv, (dw, dh), NEAREST, BR.TRANSPARENT, m_is_inverse=True, canvas=FD.canvas((dh, dw, src.shape[2])))
                assert ((PX.bits(alone)[..., 0] == FD.MINUS_ZERO) & (count >= 2)).sum() >= 8, cid


@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_tiny_source_cases_sample_something(interp):
    """2 x 2 and 5 x 1 sources: too few pixels for the shares above; what is asked is that the source is reached under nearest
    and that the canvas survives where it must."""
    xy, frac = FD.tiny_map(interp)
    for sh, sw in FD.TINY_SOURCES:
        st = FD.tiny_lens_setup(sh, sw)
        for cid, src, mode, bv in FD.tiny_lens_cases(sh, sw, interp):
            exp, computed, kept, _ = FD.lens_expected(src, st, interp, mode, 0.0 if bv is None else bv)
            assert (PX.bits(exp.reshape(kept.shape + (3,))[kept]) == FD.CANVAS_BITS).all(), cid
            if interp == NEAREST:
                assert np.isin(PX.bits(exp), PX.bits(src)).any(), cid
        for cid, src, mode, bv in FD.tiny_remap_cases(sh, sw, interp):
            exp, computed, kept, _ = FD.remap_expected(src, xy, frac, interp, mode, bv)
            assert (PX.bits(exp.reshape(kept.shape + (3,))[kept]) == FD.CANVAS_BITS).all(), cid
            if interp == NEAREST:
                assert np.isin(PX.bits(exp), PX.bits(src)).any(), cid


# ---- 2. the references tied to each other, by bits, on the same frames ----

def _frames(sh, sw, c=3):
    return [(kind, FD.frame(kind, FD.seed(4000, kind, c), sh, sw, c)) for kind in FD.KINDS]


@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
@pytest.mark.parametrize("geom", sorted(FD.GEOMS))
def test_remap_of_a_built_map_is_the_border_warp(geom, interp):
    sw, sh, dw, dh, M = FD.GEOMS[geom]
    Minv = wn.invert3x3(M)
    xy, frac = RR.build((dw, dh), Minv, None, INF, interp)
    for kind, src in _frames(sh, sw):
        for mode in RR.MODES:
            got, computed, _, _ = FD.remap_expected(src, xy, frac, interp, mode, FD.border(3))
            want = BR.warp(src, Minv, (dw, dh), interp, mode, m_is_inverse=True, border_value=FD.border(3), canvas=FD.canvas((dh, dw, 3)))
            FD.compare(got, want, computed, "%s %s %s" % (geom, kind, BR.NAMES[mode]))


@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
@pytest.mark.parametrize("geom", sorted(FD.GEOMS))
def test_identity_lens_is_the_border_warp(geom, interp):
    """fx = fy = 1, cx = cy = 0, no distortion, R = Minv.  Nearest: the maps are the pinhole ones.  Bilinear: (Xn / W) * 32 against
    Xn * (32 / W) round apart at a few pixels by construction (tests/test_lens_cpu.py); the pixels are compared where the maps agree."""
    sw, sh, dw, dh, M = FD.GEOMS[geom]
    Minv = wn.invert3x3(M)
    lens = np.array([1.0, 1.0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0])
    a, b = LR.maps((dw, dh), Minv, lens, INF, interp), wn.fixed_point_maps((dw, dh), Minv, interp)
    same = np.all([a[i] == b[i] for i in range(4)], axis=0) & a[4]
    assert same.all() if interp == NEAREST else same.mean() > 0.95
    for kind, src in _frames(sh, sw):
        for mode in (LR.CONSTANT, LR.TRANSPARENT):
            got = LR.warp(src, Minv, lens, INF, (dw, dh), interp, mode, border_value=FD.border(3), canvas=FD.canvas((dh, dw, 3)))
            want = BR.warp(src, Minv, (dw, dh), interp, mode, m_is_inverse=True, border_value=FD.border(3), canvas=FD.canvas((dh, dw, 3)))
            PX.same_float(got[same], want[same], payload=interp == NEAREST)


@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_stitch_of_one_camera_and_over_are_transparent_warps(interp):
    scene, (dw, dh) = FD.stitch_scene()
    Ms = [M for _, _, M in scene]
    for kind in FD.KINDS:
        srcs = FD.stitch_sources(kind, 3)
        for blend, F in ((SR.OVER, 64), (SR.FEATHER, 1), (SR.FEATHER, 64)):  # one camera: every cover is a single one
            got, _ = SR.stitch(srcs[:1], Ms[:1], (dw, dh), interp, blend, F, SR.TRANSPARENT, canvas=FD.canvas((dh, dw, 3)))
            PX.same_float(got, BR.warp(srcs[0], Ms[0], (dw, dh), interp, BR.TRANSPARENT, m_is_inverse=True, canvas=FD.canvas((dh, dw, 3))), payload=True)
        for order in ((0, 1, 2), (2, 0, 1)):
            want = FD.canvas((dh, dw, 3))
            for k in order:
                want = BR.warp(srcs[k], Ms[k], (dw, dh), interp, BR.TRANSPARENT, m_is_inverse=True, canvas=want)
            got, _ = SR.stitch([srcs[k] for k in order], [Ms[k] for k in order], (dw, dh), interp, SR.OVER, 64, SR.TRANSPARENT, canvas=FD.canvas((dh, dw, 3)))
            PX.same_float(got, want, payload=True)


def _nearest_quotient_is(q, num, den):
    """q (float32) is the float32 nearest num / den (a float32 and an integer), ties to even: in rationals."""
    exact = fractions.Fraction(float(num)) / int(den)
    lo, hi = np.nextafter(q, F32(-np.inf)), np.nextafter(q, F32(np.inf))
    dq = abs(exact - fractions.Fraction(float(q)))
    for other in (lo, hi):
        if np.isinf(other):  # beside +-FLT_MAX stands 2^128 for the purpose of rounding
            other_exact = fractions.Fraction(2) ** 128 * (1 if other > 0 else -1)
        else:
            other_exact = fractions.Fraction(float(other))
        d = abs(exact - other_exact)
        if dq > d or (dq == d and int(PX.bits(q).ravel()[0]) & 1):
            return False
    return True


def test_feather_division_is_correctly_rounded():
    """The reference's acc / float(W) on the committed frames: numpy's float32 division, checked in rationals on every finite (acc, W)
    pair of a seeded sample -- subnormal and near-overflow quotients among them."""
    scene, (dw, dh) = FD.stitch_scene()
    rng = np.random.default_rng(5)
    checked = {"subnormal": 0, "normal": 0}
    for kind in PX.KINDS:
        srcs = FD.stitch_sources(kind, 3)
        cams = SR.cameras(srcs, [M for _, _, M in scene], (dw, dh), LINEAR, 64)
        acc, W = _accumulate(cams, (dh, dw, 3))
        many = (sum(cover.astype(int) for cover, _, _ in cams) >= 2)[..., None] & np.isfinite(acc)
        mean = (acc / np.where(W > 0, W, 1).astype(F32)[..., None]).astype(F32)
        exp, _ = SR.stitch(srcs, [M for _, _, M in scene], (dw, dh), LINEAR, SR.FEATHER, 64, SR.TRANSPARENT)
        PX.same_float(exp[many], mean[many], payload=True)  # (the pairs below are the reference's own)
        idx = np.argwhere(many)
        for y, x, ch in idx[rng.permutation(len(idx))[:400]]:
            q = mean[y, x, ch]
            assert _nearest_quotient_is(q, acc[y, x, ch], W[y, x]), (kind, y, x, ch, float(acc[y, x, ch]), int(W[y, x]), float(q))
            checked["subnormal" if PX.is_subnormal(q) else "normal"] += 1
    assert checked["subnormal"] >= 50 and checked["normal"] >= 200, checked
    assert not _nearest_quotient_is(np.nextafter(F32(1.0) / F32(3.0), F32(1)), F32(1.0), 3)  # (the check can fail)


def _accumulate(cams, shape, first_product=False, flush=False):
    """FEATHER's sums as tests/stitch_ref.py takes them: (acc, W)."""
    acc, seen = np.zeros(shape, F32), np.zeros(shape[:2], bool)
    for cover, p, wk in cams:
        prod = (wk.astype(F32)[..., None] * p).astype(F32)
        if flush:
            prod = _flush(prod)
        nxt = (acc + prod).astype(F32)
        if first_product:
            nxt = np.where(seen[..., None], nxt, prod)
        acc = np.where(cover[..., None], _flush(nxt) if flush else nxt, acc)
        seen = seen | cover
    return acc, sum(wk for _, _, wk in cams)


# ---- 3. the faults ----

def _flush(a):
    return np.where(PX.is_subnormal(a), np.copysign(F32(0), a), a).astype(F32)


def sample(src, xy, frac, interp, mode, cval, base, fault=""):
    """tests/remap_ref.remap's float32 arm, restated with one fault switched on ("" -- none: then it IS that function, which the faults'
    tests assert first).  `base` is the canvas TRANSPARENT keeps."""
    s3 = src[:, :, None] if src.ndim == 2 else src
    h, w, c = s3.shape
    sx, sy = xy[..., 0].astype(np.int64), xy[..., 1].astype(np.int64)
    cval = np.broadcast_to(np.asarray(cval, np.float64), (c,)).astype(F32)

    def tap(px, py):
        qx, xin = RR._index(px, w, mode)
        qy, yin = RR._index(py, h, mode)
        inside, v = xin & yin, s3[qy, qx]
        if fault == "f":
            m = inside.astype(F32)[..., None]
            return (v * m + cval[None, None, :] * (F32(1) - m)).astype(F32), inside
        return np.where(inside[..., None], v, cval[None, None, :]), inside

    if interp == NEAREST:
        out, _ = tap(sx, sy)
        if fault == "h":
            out = out * F32(1.0)
    else:
        f = np.asarray(frac).astype(np.int64)
        fx, fy = f & 31, (f >> 5) & 31
        s = F32(1.0 / 32.0)
        tx1, ty1 = fx.astype(F32) * s, fy.astype(F32) * s
        tx0, ty0 = F32(1) - tx1, F32(1) - ty1
        taps = [tap(sx, sy), tap(sx + 1, sy), tap(sx, sy + 1), tap(sx + 1, sy + 1)]
        weights = [ty0 * tx0, ty0 * tx1, ty1 * tx0, ty1 * tx1]
        terms = []
        for (t, _), wt in zip(taps, weights):
            a = ((_flush(t) if fault == "b" else t) * wt[..., None]).astype(F32)
            if fault == "a":
                a = np.where((wt == 0)[..., None], F32(0), a)
            terms.append(_flush(a) if fault == "b" else a)
        add = (lambda p, q: _flush((p + q).astype(F32))) if fault == "b" else (lambda p, q: (p + q).astype(F32))
        out = add(add(terms[0], terms[2]), add(terms[1], terms[3])) if fault == "g" else add(add(add(terms[0], terms[1]), terms[2]), terms[3])
        if mode == RR.CONSTANT:
            none_in = ~(taps[0][1] | taps[1][1] | taps[2][1] | taps[3][1])
            out = np.where(none_in[..., None], cval[None, None, :], out)
    if mode == RR.TRANSPARENT:
        out = np.where(RR.written(xy, w, h, interp)[..., None], out, np.asarray(base, F32).reshape(out.shape))
    return out.astype(F32).reshape(xy.shape[:2] + src.shape[2:])


def stitch(srcs, interp, blend, feather, mode, border_value, fault=""):
    """tests/stitch_ref.stitch's float32 arm on the scene, restated over sample() with one fault switched on."""
    scene, (dw, dh) = FD.stitch_scene()
    c = srcs[0].shape[2]
    cams = []
    for src, (w, h, Minv) in zip(srcs, scene):
        xy, frac = RR.build((dw, dh), Minv, None, INF, interp)
        cover = RR.written(xy, w, h, interp)
        p = sample(src, xy, frac, interp, RR.TRANSPARENT, 0.0, np.zeros((dh, dw, c), F32), fault if fault in "abgh" else "")
        sx, sy = xy[..., 0].astype(np.int64), xy[..., 1].astype(np.int64)
        cams.append((cover, p, np.where(cover, np.minimum(SR.edge_distance(sx, sy, w, h), int(feather)), 0).astype(np.int64)))
    count = sum(cover.astype(np.int64) for cover, _, _ in cams)
    out = FD.canvas((dh, dw, c)) if mode == SR.TRANSPARENT else np.broadcast_to(np.asarray(border_value, np.float64).astype(F32), (dh, dw, c)).astype(F32)
    for cover, p, _ in cams:
        if fault == "f":
            m = cover.astype(F32)[..., None]
            out = (p * m + out * (F32(1) - m)).astype(F32)
        else:
            out = np.where(cover[..., None], p, out)
    if blend == "feather":
        acc, W = _accumulate(cams, (dh, dw, c), first_product=fault == "c", flush=fault == "b")
        blended = count >= (1 if fault == "e" else 2)
        Ws = np.where(blended, W, 1).astype(F32)[..., None]
        mean = (acc * (F32(1) / Ws)).astype(F32) if fault == "d" else (acc / Ws).astype(F32)
        out = np.where(blended[..., None], _flush(mean) if fault == "b" else mean, out)
    return out.astype(F32)


def _lens_runs(frames_of):
    """(id, interp, faulty(fault), exp, computed) of the lens family's cases -- through the map the lens chain gives, as bevwarp_remap's
    definition has it (tests/test_remap_cpu.py ties the two)."""
    for geom, lens in FD.LENS_SETUPS:
        st = FD.lens_setup(geom, lens)
        for interp in (NEAREST, LINEAR):
            xy, frac = RR.build((st[2], st[3]), st[7], st[8], st[9], interp)
            for kind in FD.kinds(interp):
                for cid, src, mode, bv in frames_of(FD.lens_cases(geom, lens, kind, interp)):
                    if src.ndim == 3:
                        exp, computed, _, _ = FD.lens_expected(src, st, interp, mode, 0.0 if bv is None else bv)
                        yield cid, interp, (lambda fault, a=(src, xy, frac, interp, mode, 0.0 if bv is None else bv, FD.canvas(exp.shape)): sample(*a, fault)), exp, computed


def _remap_runs(frames_of):
    for geom, km in FD.REMAP_SETUPS:
        for interp in (NEAREST, LINEAR):
            xy, frac = FD.ref_map(geom, km, interp)
            for kind in FD.kinds(interp):
                for cid, srcs, mode, bv in frames_of(FD.remap_cases(geom, km, kind, interp)):
                    exp, computed, _, _ = FD.remap_expected(srcs[0], xy, frac, interp, mode, bv)
                    yield cid, interp, (lambda fault, a=(srcs[0], xy, frac, interp, mode, 0.0 if bv is None else bv, FD.canvas(exp.shape)): sample(*a, fault)), exp, computed


def _stitch_runs(frames_of):
    for interp in (NEAREST, LINEAR):
        for kind in FD.kinds(interp):
            for cid, srcs, blend, F, mode, bv in frames_of(FD.stitch_cases(kind, interp)):
                exp, computed, _, _, _ = FD.stitch_expected(srcs, interp, blend, F, mode, bv)
                yield cid, interp, (lambda fault, a=(srcs, interp, blend, F, mode, 0.0 if bv is None else bv): stitch(*a, fault=fault)), exp, computed


RUNS = {"lens": _lens_runs, "remap": _remap_runs, "stitch": _stitch_runs}


def _committed(cases):
    return [c for c in cases if c[0].endswith("c3")]  # (3 channels of every kind, border and blend: a fault shows there or nowhere)


def _detected(family, frames_of, judge):
    """{fault: the first case of the family on which `judge` tells the faulty copy from the reference, or None}; the faultless copy
    must equal the reference on every case walked."""
    found = {f: None for f, fams in FAULTS.items() if family in fams}
    for cid, interp, faulty, exp, computed in RUNS[family](frames_of):
        if all(found.values()):
            break
        FD.compare(faulty(""), exp, computed, "the faultless copy, " + cid)
        for f in found:
            if found[f] is None and (f != "h" or interp == NEAREST) and not judge(faulty(f), exp, computed):
                found[f] = cid
    return found


def _same(got, exp, computed):
    try:
        FD.compare(got, exp, computed)
    except AssertionError:
        return False
    return True


@pytest.mark.parametrize("family", sorted(RUNS))
def test_committed_cases_tell_every_fault_apart(family):
    found = _detected(family, _committed, _same)
    assert all(found.values()), found


def test_zero_blocks_show_the_accumulator_start_under_bilinear():
    """Fault (c) differs from the definition only where every covering camera's pixel is -0.0: +0 + -0.0 is +0.0, the first product
    alone is -0.0.  Under bilinear a pixel is -0.0 only if all four of its taps are (or carry weight 0), which float_frame's scattered
    zeros give nowhere in the overlaps -- the squares of zero_block_frame do, for two cameras at once."""
    hits = [cid for cid, interp, faulty, exp, computed in _stitch_runs(_committed) if interp == LINEAR and "feather" in cid and not _same(faulty("c"), exp, computed)]
    assert any("-blocks-" in cid for cid in hits), hits


def _unit_interval(cases):
    """The cases' geometry, borders and blends on the frames the families' own GPU modules use."""
    out = []
    for case in _committed(cases):
        if "-mixed-" in case[0]:
            rng = np.random.default_rng(len(out))
            redo = lambda s: rng.random(s.shape, dtype=F32)  # noqa: E731
            out.append((case[0].replace("mixed", "unit"), [redo(s) for s in case[1]] if isinstance(case[1], list) else redo(case[1])) + tuple(case[2:]))
    return out


def test_unit_interval_frames_record(monkeypatch):
    """Not a gate: prints which faults frames in [0, 1) under assert_array_equal show (the table of this module's docstring).  The canvas
    is those modules' too: 77."""
    monkeypatch.setattr(FD, "CANVAS_BITS", 0x429a0000)
    for family in sorted(RUNS):
        found = _detected(family, _unit_interval, lambda got, exp, computed: np.array_equal(got, exp, equal_nan=True))
        print("[0, 1) frames, %s: %s" % (family, "  ".join("(%s) %s" % (f, "x" if v else "-") for f, v in sorted(found.items()))))
