"""tests/random_scenes.py without a device: the case lists are reproducible and pinned, the sweep reaches the paths it is said to reach
(counted from the numpy definitions, never from the library), and it tells ten wrong definitions from the right one.  The pinned list is
8 seeds x 12 cases per family, the list tests/test_gpu_random_scenes.py runs."""
import collections
import functools
import hashlib

import numpy as np
import pytest

from tests import border_ref as BR
from tests import fisheye_ref as FR
from tests import lens_ref as LR
from tests import nv12_out_ref as NO
from tests import nv12_ref as NR
from tests import random_scenes as RS
from tests import remap_ref as RR
from tests import stitch_gain_ref as SG
from tests import stitch_maps_ref as SM
from tests import stitch_ref as SR

# sha256 of repr() of the 96 case records of each family: an edit to the generator shows here
DIGESTS = {
    "lens": "0f6ffee94890de2d8535dd89d2ea8a865cc41960bce42d17aacee700b1b9bd87",
    "map": "ec2982c4810a669af04160a830e873ab00b01757e9d251b603436be35a66b138",
    "nv12": "4cc2ce040de58999654caedc2e01fae17d7e7a2fc74d544df34edb0d9ae4ec47",
    "stitch": "f2e6950d88a6975eaa98416ffcecc5f90860ca31d3a511507859c7a60789508f",
}


@functools.lru_cache(maxsize=None)
def all_cases(family):
    return tuple(c for seed in RS.SEEDS for c in RS.cases(family, seed))


def digest(family):
    return hashlib.sha256(repr(all_cases(family)).encode()).hexdigest()


# ---- (a) determinism ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", RS.FAMILIES)
def test_cases_are_reproducible_and_pinned(family):
    for seed in RS.SEEDS:
        a, b = RS.cases(family, seed), RS.cases(family, seed)
        assert a == b and len(a) == RS.N_CASES
        assert [(c.family, c.seed, c.index) for c in a] == [(family, seed, i) for i in range(RS.N_CASES)]
        hash(a[0])  # (frozen: parameters and seeds only)
    assert len(set(all_cases(family))) == len(RS.SEEDS) * RS.N_CASES
    assert digest(family) == DIGESTS[family], "the generator's draws for %r changed: %s" % (family, digest(family))


@pytest.mark.parametrize("family", RS.FAMILIES)
def test_half_of_the_cases_run_on_guarded_layouts_and_sizes_stay_in_range(family):
    cs = all_cases(family)
    assert sum(c.p.layout is not None for c in cs) * 2 == len(cs)
    for c in cs:
        p = c.p
        nv12_out = RS.kind_of_result(c) == "nv12"
        assert 1 <= p.dsize[0] <= 130 and 1 <= p.dsize[1] <= 40 and p.B in RS.BATCHES and (not nv12_out or (p.dsize[0] % 2 == 0 and p.dsize[1] % 2 == 0)), c
        cams = RS.inputs(c)
        assert 1 <= len(cams) <= 8
        for cam in cams:
            nv12 = isinstance(cam.frames, tuple)
            assert 1 <= cam.sw <= 96 and 1 <= cam.sh <= 64 and cam.n_m in (1, p.B) and (not nv12 or (cam.sw % 2 == 0 and cam.sh % 2 == 0)), c
        if family == "stitch":
            assert p.feather in (0,) + RS.FEATHERS and all(v != 0 for v in p.border)


# ---- (b) census ---------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def total_census():
    """The census summed over the pinned list, and per family what only a family has."""
    tot = collections.Counter()
    cover = np.zeros(9, np.int64)
    fam = {f: dict(sentinels=0, entries=0, writes_nothing=0, values=collections.defaultdict(collections.Counter)) for f in RS.FAMILIES}
    for family in RS.FAMILIES:
        for c in all_cases(family):
            cs = RS.census(c)
            cover += cs["cover"]
            for k in ("left0", "left_last", "clipped", "unclipped", "frac0", "behind", "taps", "saturated", "gain0", "gain_max", "nv12_2px"):
                tot[k] += int(cs[k])
            fam[family]["sentinels"] += sum(s for s, _ in cs["lens_maps"])
            fam[family]["entries"] += sum(n for _, n in cs["lens_maps"])
            fam[family]["writes_nothing"] += bool(cs["writes_nothing"])
            for name in ("mode", "dtype", "c", "plane", "rgb", "interp", "user", "entry"):
                v = getattr(c.p, name, None)
                if v is not None:
                    fam[family]["values"][name][v] += 1
    return tot, cover, fam


def test_census_cover_counts():
    _, cover, _ = total_census()
    print("canvas pixels by cover count 0..8:", cover.tolist())
    assert (cover >= 32).all(), cover.tolist()


def test_census_taps_weights_and_ties():
    tot, _, _ = total_census()
    print(dict(tot))
    assert tot["left0"] >= 500 and tot["left_last"] >= 500
    weights = tot["clipped"] + tot["unclipped"]
    assert tot["clipped"] >= 0.10 * weights and tot["unclipped"] >= 0.10 * weights
    assert tot["frac0"] >= 1000
    assert tot["behind"] >= 200
    assert 0.01 * tot["taps"] <= tot["saturated"] <= 0.50 * tot["taps"]
    assert tot["gain0"] >= 1 and tot["gain_max"] >= 1
    assert tot["nv12_2px"] >= 2


def test_census_per_family():
    _, _, fam = total_census()
    for family, f in fam.items():
        print(family, "sentinels %d of %d" % (f["sentinels"], f["entries"]), "cases that write nothing: %d" % f["writes_nothing"], {k: dict(v) for k, v in f["values"].items()})
        if family != "nv12":  # (the direct NV12 entries take no lens)
            assert 0.01 * f["entries"] <= f["sentinels"] <= 0.60 * f["entries"], family
        assert f["writes_nothing"] <= 0.05 * len(all_cases(family)), family
    want = {"lens": dict(mode=(0, 5), dtype=("u8", "f32"), c=(1, 2, 3, 4), interp=(0, 1)),
            "map": dict(mode=tuple(range(6)), dtype=("u8", "f32"), c=(1, 2, 3, 4), plane=("f32", "f16", "bf16"), rgb=(False, True), interp=(0, 1), user=RS.MAP_USERS),
            "nv12": dict(dtype=("u8", "f32"), c=(1, 2, 3, 4), plane=("f32", "f16", "bf16"), rgb=(False, True), interp=(0, 1), entry=RS.NV12_ENTRIES),
            "stitch": dict(mode=(0, 5), dtype=("u8", "f32"), c=(1, 2, 3, 4), plane=("f32", "f16", "bf16"), rgb=(False, True), interp=(0, 1), entry=RS.STITCH_ENTRIES)}
    for family, names in want.items():
        for name, values in names.items():
            for v in values:
                assert fam[family]["values"][name][v] >= 2, (family, name, v, dict(fam[family]["values"][name]))


def test_census_stitch_scenes():
    """Gains on about half of the map stitches, blends of both kinds with every F, cameras of every lens model, maps per frame and shared."""
    cs = all_cases("stitch")
    mapped = [c for c in cs if c.p.entry != "warp_stitch"]
    gained = [c for c in mapped if RS.gains_of(c) is not None]
    assert 0.3 * len(mapped) <= len(gained) <= 0.7 * len(mapped)
    assert {c.p.feather for c in cs} == {0} | set(RS.FEATHERS)
    assert {r.lens.model for c in cs for r in c.p.cams} == {"pinhole", "rational", "fisheye"}
    assert {len(c.p.cams) for c in cs} == set(range(1, 9))
    assert sum(any(r.view == "none" for r in c.p.cams) for c in cs) >= 3 and sum(all(r.view == "whole" for r in c.p.cams) for c in cs) >= 3
    assert sum(len({r.n_m for r in c.p.cams}) == 2 for c in cs) >= 3  # (a map per frame beside a shared one, in one launch)
    for entry in RS.STITCH_ENTRIES[1:]:  # fisheye maps and gains meet every NV12 and plane entry
        assert any(c.p.entry == entry and RS.gains_of(c) is not None and any(r.lens.model == "fisheye" for r in c.p.cams) for c in cs), entry


# ---- (c) the sweep tells wrong definitions apart ---------------------------------------------------------------------------------------------------

def _blob(e):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in (e if isinstance(e, tuple) else (e,)))


@functools.lru_cache(maxsize=None)
def baseline(family):
    return tuple(tuple(_blob(e) for e in RS.expected(c)) for c in all_cases(family))


def altered(families):
    """The cases whose expected result differs from the baseline's, under whatever is patched now."""
    out = []
    for family in families:
        for c, base in zip(all_cases(family), baseline(family)):
            if tuple(_blob(e) for e in RS.expected(c)) != base:
                out.append(c)
    return out


def _stitch_wrappers(monkeypatch, wrap):
    """Put wrap(original, cameras function) in place of stitch_maps_ref.stitch and stitch_ref.stitch."""
    monkeypatch.setattr(SM, "stitch", wrap(SM.stitch, lambda srcs, maps, *a: SM.cameras(srcs, maps, *a), False))
    monkeypatch.setattr(SR, "stitch", wrap(SR.stitch, lambda srcs, Ms, *a: SR.cameras(srcs, Ms, *a), True))


def test_mutant_camera_order_reversed_under_over(monkeypatch):
    def wrap(orig, _cams, direct):
        def stitch(srcs, maps, *a, **kw):
            blend = a[2 if direct else 1] if len(a) > (2 if direct else 1) else kw.get("blend", SM.OVER)
            return orig(srcs[::-1], maps[::-1], *a, **kw) if blend == SM.OVER else orig(srcs, maps, *a, **kw)
        return stitch
    baseline("stitch")
    _stitch_wrappers(monkeypatch, wrap)
    assert len(altered(["stitch"])) >= 3


def test_mutant_feather_weights_not_clipped(monkeypatch):
    baseline("stitch")
    sm, sr = SM.cameras, SR.cameras
    monkeypatch.setattr(SM, "cameras", lambda srcs, maps, interp, feather: sm(srcs, maps, interp, 1 << 20))
    monkeypatch.setattr(SR, "cameras", lambda srcs, Ms, dsize, interp, feather: sr(srcs, Ms, dsize, interp, 1 << 20))
    assert len(altered(["stitch"])) >= 3


def test_mutant_feather_rounding_term_dropped(monkeypatch):
    """The 8-bit mean without + (W >> 1): recomputed from the definition's own cameras and put where two or more cover."""
    baseline("stitch")

    def wrap(orig, cams_of, direct):
        def stitch(srcs, maps, *a, **kw):
            out, count = orig(srcs, maps, *a, **kw)
            names = (("dsize",) if direct else ()) + ("interp", "blend", "feather")
            args = dict(zip(names, a), **{k: v for k, v in kw.items() if k in names})
            if args.get("blend", SM.OVER) != SM.FEATHER or np.asarray(srcs[0]).dtype != np.uint8:
                return out, count
            pre = (args["dsize"],) if direct else ()
            cams = cams_of(srcs, maps, *pre, args["interp"], args["feather"])
            num = sum(wk[..., None] * p.astype(np.int64) for _, p, wk in cams)
            Ws = np.maximum(sum(wk for _, _, wk in cams), 1)
            mean = (num // Ws[..., None]).astype(np.uint8).reshape(count.shape + (-1,))
            return np.where((count >= 2)[..., None], mean, np.asarray(out).reshape(mean.shape)).reshape(np.shape(out)), count
        return stitch
    _stitch_wrappers(monkeypatch, wrap)
    assert len(altered(["stitch"])) >= 3


def test_mutant_gain_applied_after_the_interpolation(monkeypatch):
    """The gain on the camera's interpolated pixel instead of on every tap."""
    baseline("stitch")

    def stitch(srcs, G, maps, *a, **kw):
        orig = SM.cameras
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(SM, "cameras", lambda *b: [(cover, SG.apply_gain(p, g), wk) for (cover, p, wk), g in zip(orig(*b), G)])
            return SM.stitch(srcs, maps, *a, **kw)
    monkeypatch.setattr(SG, "stitch", stitch)
    assert len(altered(["stitch"])) >= 3


def test_mutant_gain_channels_reversed(monkeypatch):
    baseline("stitch")
    orig = SG.apply_gain
    monkeypatch.setattr(SG, "apply_gain", lambda frame, G3: orig(frame, np.asarray(G3).reshape(3)[::-1]))
    assert len(altered(["stitch"])) >= 3


def test_mutant_rgb_ignored(monkeypatch):
    for f in ("map", "nv12", "stitch"):
        baseline(f)
    to_bgr, to_nv12 = NR.nv12_to_bgr, NO.bgr_to_nv12
    monkeypatch.setattr(NR, "nv12_to_bgr", lambda y, uv, rgb=False: to_bgr(y, uv, False))
    monkeypatch.setattr(NO, "bgr_to_nv12", lambda img, rgb=False: to_nv12(img, False))
    for f in ("map", "nv12", "stitch"):
        assert len(altered([f])) >= 3, f


def test_mutant_bilinear_inliers_one_column_wider(monkeypatch):
    for f in ("lens", "map", "stitch"):
        baseline(f)

    def written(xy, w, h, interp):
        sx, sy = xy[..., 0].astype(np.int64), xy[..., 1].astype(np.int64)
        return BR.inliers(sx, sy, w, h, interp)

    def inliers(sx, sy, w, h, interp):
        if interp == 0:
            return (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
        return (sx >= 0) & (sx <= w - 1) & (sy >= 0) & (sy <= h - 2)
    monkeypatch.setattr(BR, "inliers", inliers)
    monkeypatch.setattr(RR, "written", written)
    monkeypatch.setattr(LR, "inliers", lambda sx, sy, valid, w, h, interp: valid & inliers(sx, sy, w, h, interp))
    for f in ("lens", "map", "stitch"):  # (the map family writes TRANSPARENT only through remap and remap_nv12)
        assert len(altered([f])) >= (3 if f != "map" else 1), f


def test_mutant_theta_max_comparison_strict(monkeypatch):
    for f in ("lens", "map", "stitch"):
        baseline(f)
    orig = FR.maps

    def maps(dsize, R, lens, theta_max, interp):
        sx, sy, fx, fy, valid = orig(dsize, R, lens, theta_max, interp)
        with np.errstate(all="ignore"):
            return sx, sy, fx, fy, valid & (FR.chain(dsize, R, lens)[2] < np.float64(theta_max))
    monkeypatch.setattr(FR, "maps", maps)
    assert len(altered(["lens", "map", "stitch"])) >= 3


def test_mutant_reflect_taken_for_reflect_101(monkeypatch):
    baseline("map")
    orig = BR.border_index
    monkeypatch.setattr(BR, "border_index", lambda p, n, mode: orig(p, n, BR.REFLECT if mode == BR.REFLECT_101 else mode))
    assert len(altered(["map"])) >= 3


def test_mutant_shared_map_for_every_frame(monkeypatch):
    for f in RS.FAMILIES:
        baseline(f)
    monkeypatch.setattr(RS, "map_frame", lambda n_m, b: 0)
    for f in RS.FAMILIES:
        assert len(altered([f])) >= 3, f
