"""The context a launch runs in, for tests/test_gpu_launch_contexts.py and tests/test_launch_contexts_cpu.py -- TEST INFRASTRUCTURE ONLY, a
plain module like tests/parity.py: no fixtures, no conftest.

CASES holds one case (or a few) per C ABI symbol that launches a kernel and is captured by no other test; tests/test_launch_contexts_cpu.py
keeps the table complete against bev_amd._lib.SYMBOLS.  A case is: two sets of device inputs "A" and "B" (host numpy arrays), the host
values the call is given (matrices, border value, scale, bias, the lens -- fresh arrays per call, so that a test can overwrite them
afterwards), what stays resident on the device (warp maps), the call itself, and the expected result of a set from the numpy definitions
under tests/ (never from the device).  Shapes are context-sized: 40 x 24 sources, 36 x 20 destinations, 2 frames, 2 overlapping cameras,
INTER_LINEAR, a non-zero constant border -- BORDER_TRANSPARENT without `out` where the case is marked no_out.

The three checks drive a case through a backend: Gpu (torch.cuda streams, events and graphs) or, on the CPU, the stand-in of
tests/test_launch_contexts_cpu.py, whose streams are queues -- so that what the checks are for is shown to fail them without a GPU.

  check_side_stream   behind a delay on a fresh stream: set B is copied over set A, the destination is poisoned and the entry is called,
                      all while the delay still runs (asserted: a precondition).  A launch enqueued on any other stream reads set A and
                      is overwritten by the poison.
  check_replays       the call captured into a graph (nothing runs: the poison stays), every host array it was given overwritten with
                      NaNs, then replayed on set B and, re-poisoned, on set A.  With `out` absent the entry allocates (and for
                      BORDER_TRANSPARENT zeroes) its result inside the capture: the returned tensor is poisoned before each replay, so
                      a zero fill that is no node of the graph leaves 77s where nothing is written.  sliced=True hands the frames over
                      as channel slices of 4-channel holders: the entry's contiguous copy must be a node of the graph too.
  check_second_device every tensor on another device than the current one; the current device stays what it was."""
import contextlib
import functools
import time

import numpy as np
import torch

from bev_amd import points as PT
from bev_amd import resize as RZ
from bev_amd import warp as W
from oracle import cpu_oracle as co
from tests import lens_ref as LR
from tests import map_planes_ref as MP
from tests import nv12_out_ref as NO
from tests import nv12_ref as NR
from tests import points_lens_ref as PR
from tests import remap_nv12_out_ref as RNO
from tests import remap_nv12_ref as RN
from tests import remap_ref as RR
from tests import stitch_maps_ref as SM
from tests import stitch_ref as SR
from tests import workloads as wl

SW, SH, DW, DH, BATCH = 40, 24, 36, 20, 2
DSIZE = (DW, DH)
LINEAR = W.INTER_LINEAR
FLAGS = W.INTER_LINEAR | W.WARP_INVERSE_MAP  # every matrix below is a dst -> src map
POISON = 77
BORDER = (9.0, 200.0, 31.0)
SCALE, BIAS = (1 / 255.0, 0.5, 2.0), (0.0, -1.0, 3.5)
FEATHER = 5  # (frames of 24 rows: a camera fades out over its outermost 5 pixels)
K = LR.camera_K(SW, SH)
K3 = np.array([[K[0, 0], 0, K[0, 2]], [0, K[1, 1], K[1, 2]], [0, 0, 1.0]])
DIST = np.array(LR.LENS_A)
R2_MAX = float(LR.lens_valid_r2(LR.LENS_A))  # passed to the call and to the reference alike
N_POINTS = 300
SETS = ("A", "B")


def _minv(degrees, zoom, at, shift=(0.0, 0.0)):
    """dst px -> src px: the destination turned by `degrees` about its centre (+ shift), `zoom` source pixels per pixel, landing on `at`."""
    t = np.deg2rad(degrees)
    c, s = np.cos(t) * zoom, np.sin(t) * zoom
    A = np.array([[c, -s, 0.0], [s, c, 0.0], [0, 0, 1.0]])
    T0 = np.array([[1, 0, -(DW - 1) / 2.0 - shift[0]], [0, 1, -(DH - 1) / 2.0 - shift[1]], [0, 0, 1.0]])
    T1 = np.array([[1, 0, at[0]], [0, 1, at[1]], [0, 0, 1.0]])
    return T1 @ A @ T0


def _per_frame(degrees, zoom, at, shift=(0.0, 0.0)):
    return np.stack([_minv(degrees, zoom, at, (shift[0] + 1.7 * i, shift[1] - 0.9 * i)) for i in range(BATCH)])


CENTRE = ((SW - 1) / 2.0, (SH - 1) / 2.0)
MINVS = {"A": _per_frame(15.0, 1.4, CENTRE), "B": _per_frame(-8.0, 1.3, CENTRE, (2.0, 1.0))}  # (B: build_warp_map's other matrices)
# two cameras of a stitch: the first sees the canvas's left two thirds, the second its right half, both end inside the canvas
CAM_MINVS = (_per_frame(6.0, 1.25, CENTRE, (-9.0, 0.5)), _per_frame(-11.0, 1.2, CENTRE, (8.0, -1.0)))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def _readonly(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def frames(which, camera=0):
    """((BATCH, SH, SW, 3) uint8,): the interleaved frames of a set."""
    seed = 500 + 10 * SETS.index(which) + 100 * camera
    return _readonly(np.stack([wl.frame(seed + i, SH, SW, np.uint8) for i in range(BATCH)]))


@functools.lru_cache(maxsize=None)
def nv12(which, camera=0):
    """(y (BATCH, SH, SW), uv (BATCH, SH / 2, SW / 2, 2)) uint8: the NV12 planes of a set."""
    seed = 40 + 10 * SETS.index(which) + 100 * camera
    planes = [NR.frame("phase", seed + i, SH, SW) for i in range(BATCH)]
    return _readonly(np.stack([p[0] for p in planes]), np.stack([p[1] for p in planes]))


def camera_frames(which):
    return frames(which, 0) + frames(which, 1)


def camera_nv12(which):
    """(y0, y1, uv0, uv1)."""
    (y0, uv0), (y1, uv1) = nv12(which, 0), nv12(which, 1)
    return y0, y1, uv0, uv1


@functools.lru_cache(maxsize=None)
def points(which, direction):
    """((N_POINTS, 2) float32,): destination pixels in and around the destination (distort), raw pixels in and around the frame (undistort)."""
    rng = np.random.default_rng(900 + 10 * SETS.index(which) + direction)
    if direction == PR.DISTORT:
        p = np.stack([rng.uniform(-8, DW + 8, N_POINTS), rng.uniform(-8, DH + 8, N_POINTS)], axis=1)
    else:
        p = np.stack([rng.uniform(-30, SW + 30, N_POINTS), rng.uniform(-30, SH + 30, N_POINTS)], axis=1)
    return _readonly(p.astype(np.float32))


def no_inputs(which):
    return ()


# ---- resident maps and their reference ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_maps(key="A", lens=False):
    """[(xy, frac)] per frame of the map build_warp_map makes of MINVS[key] (key 0 / 1: of a stitch's camera), from remap_ref.build."""
    Ms = MINVS[key] if key in MINVS else CAM_MINVS[key]
    if lens:
        return [RR.build(DSIZE, LR.ray_matrix(M, K, inverse_given=True), LR.lens12(K, DIST), R2_MAX, LINEAR) for M in Ms]
    return [RR.build(DSIZE, M, interp=LINEAR) for M in Ms]


_resident = {}


def device_maps(device, key="A"):
    """The WarpMap of ref_maps(key) on `device`, built once by build_warp_map and checked against the reference by bits."""
    device = torch.device(device)
    if (device, key) not in _resident:
        Ms = MINVS[key] if key in MINVS else CAM_MINVS[key]
        m = W.build_warp_map(Ms, DSIZE, flags=FLAGS, device=device)
        torch.cuda.synchronize(device)
        xy, frac = m.xy.cpu().numpy(), m.frac.cpu().numpy().view(np.uint16)
        for i, (exy, efrac) in enumerate(ref_maps(key)):
            np.testing.assert_array_equal(xy[i], exy)
            np.testing.assert_array_equal(frac[i], efrac)
        _resident[(device, key)] = m
    return _resident[(device, key)]


def one_map(device):
    return device_maps(device)


def camera_maps(device):
    return [device_maps(device, 0), device_maps(device, 1)]


def no_maps(device):
    return None


# ---- comparisons: device tensors against expected host arrays, by bits -------------------------------------------------------------------------------
def same_ints(got, exp):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        g = g.cpu().numpy()
        np.testing.assert_array_equal(g.view(np.uint16) if e.dtype == np.uint16 else g, e)


def same_planes(dtype):
    def compare(got, exp):
        assert len(got) == len(exp) == 1 and got[0].dtype == dtype
        RN.assert_planes_equal(got[0], exp[0], dtype)  # (float32: the 32 bits; float16: planes16_ref.assert_same16)
    return compare


def same_points(got, exp):
    assert len(got) == len(exp) == 1
    assert PR.same_bits(got[0].cpu().numpy(), exp[0]), "the points differ by bits"


def differ(a, b):
    """Two expected results are not the same data."""
    return any(not np.array_equal(x, y, equal_nan=x.dtype.kind == "f") for x, y in zip(a, b))


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------
class Case:
    """name      the test id
    symbol       the C ABI symbol the call reaches
    inputs       which -> tuple of host arrays: the device inputs of set "A" / "B"
    host         which -> dict of fresh float64 host arrays the call is given (the same values for both sets unless they ARE the input)
    resident     device -> what stays on the device (maps), handed to the call
    out_shapes   [(shape, torch dtype)] of the caller's destination tensors; None: no_out, the entry allocates
    call         (tensors, resident, host, outs) -> list of result tensors
    expected     (set of the device inputs, set of the host values) -> list of host arrays, one per result tensor
    compare      (result tensors, expected) raises AssertionError
    sliceable    indices of the inputs that are interleaved 3-channel frames (the copied_source variant slices them out of 4 channels)
    written      None, or () -> bool mask of the pixels set A's call writes (no_out cases)
    cover        None, or () -> the stitch reference's cover counts of set A"""

    def __init__(self, name, symbol, inputs, host, resident, out_shapes, call, expected, compare=same_ints, sliceable=(), written=None, cover=None):
        self.name, self.symbol, self.inputs, self._host, self.resident, self.out_shapes = name, symbol, inputs, host, resident, out_shapes
        self.call, self._expected, self.compare, self.sliceable, self.written, self.cover = call, expected, compare, tuple(sliceable), written, cover

    @property
    def no_out(self):
        return self.out_shapes is None

    def host(self, which="A"):
        return {k: np.array(v, dtype=np.float64) for k, v in self._host(which).items()}

    def expected(self, which, host_which="A"):
        if self._host("A") is self._host("B"):  # (_values: one set of host values for both input sets -- one computation)
            host_which = "A"
        return _expected(self, which, host_which)

    def assert_preconditions(self):
        """What a case needs in order to show anything, from the references alone: a stitch's pixels are covered 0, 1 and 2 times in every
        frame; a result the entry allocates has written and unwritten pixels in every frame."""
        if self.cover is not None:
            for count in self.cover():
                assert set(np.unique(count)) == {0, 1, 2}, "%s: cover counts %s" % (self.name, np.unique(count))
        if self.written is not None:
            for w in self.written():
                assert w.any() and not w.all(), "%s: the written mask is empty or full" % self.name

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=None)
def _expected(case, which, host_which):
    """Computed once per case and set, shared by the contexts, and left unchanged."""
    return _readonly(*[np.ascontiguousarray(a) for a in case._expected(which, host_which)])


def _values(**kw):
    return lambda which: kw


def _stack(per_frame):
    return [np.stack(per_frame)]


def _stack_pairs(per_frame):
    """[(y, uv)] per frame -> [y of the batch, uv of the batch]."""
    return [np.stack([p[0] for p in per_frame]), np.stack([p[1] for p in per_frame])]


PX = [((BATCH, DH, DW, 3), torch.uint8)]
NV12_OUT = [((BATCH, DH, DW), torch.uint8), ((BATCH, DH // 2, DW // 2, 2), torch.uint8)]
MAP_OUT = [((BATCH, DH, DW, 2), torch.int16), ((BATCH, DH, DW), torch.int16)]
POINTS_OUT = [((N_POINTS, 2), torch.float32)]


def planes_out(dtype):
    return [((BATCH, 3, DH, DW), dtype)]


def _o(outs):
    """`out=` of an entry that takes one tensor."""
    return None if outs is None else outs[0]


def _mode(outs):
    """The border of a call: the constant one into the caller's destination, BORDER_TRANSPARENT where the entry allocates."""
    return W.BORDER_TRANSPARENT if outs is None else W.BORDER_CONSTANT


def _ref_mode(no_out):
    return RR.TRANSPARENT if no_out else RR.CONSTANT


def _lens_rays(M):
    return LR.ray_matrix(M, K, inverse_given=True)


def _cases():
    cases = []
    MATS = _values(M=MINVS["A"], border=BORDER)
    PLANES = _values(M=MINVS["A"], border=BORDER, scale=SCALE, bias=BIAS)
    MAPPED = _values(border=BORDER)
    MAPPED_PLANES = _values(border=BORDER, scale=SCALE, bias=BIAS)
    STITCH_MATS = _values(M0=CAM_MINVS[0], M1=CAM_MINVS[1], border=BORDER)
    maps_a = ref_maps
    cam_refs = lambda i: [ref_maps(0)[i], ref_maps(1)[i]]  # noqa: E731
    stitch_cover = functools.lru_cache(maxsize=None)(lambda: np.stack([SM.stitch([f[i] for f in camera_frames("A")], cam_refs(i), LINEAR)[1] for i in range(BATCH)]))

    # -- the lens warp ---------------------------------------------------------------------------------------------------------------------------
    for no_out in (False, True):
        mode = LR.TRANSPARENT if no_out else LR.CONSTANT
        cases.append(Case(
            "warp_perspective_lens" + "-no_out" * no_out, "bevwarp_warp_lens", frames, _values(M=MINVS["A"], K=K3, dist=DIST, border=BORDER), no_maps,
            None if no_out else PX,
            lambda t, r, h, o: [W.warp_perspective_lens(t[0], h["M"], DSIZE, h["K"], h["dist"], flags=FLAGS, border_value=h["border"], out=_o(o), border_mode=_mode(o),
                                                        r2_max=R2_MAX)],
            lambda which, hw, mode=mode: _stack([LR.warp(f, _lens_rays(M), LR.lens12(K, DIST), R2_MAX, DSIZE, LINEAR, mode, BORDER) for f, M in zip(frames(which)[0], MINVS["A"])]),
            sliceable=(0,),
            written=(lambda: np.stack([LR.written_mask((SH, SW), _lens_rays(M), LR.lens12(K, DIST), R2_MAX, DSIZE, LINEAR) for M in MINVS["A"]])) if no_out else None))

    # -- the map builder: its inputs are host matrices, taken by value; the sets are two sets of matrices ------------------------------------------------
    def built(t, r, h, o, lens):  # (no `device=`: the map's own device is where the matrices have to go)
        m = W.build_warp_map(h["M"], DSIZE, flags=FLAGS, K=h["K"] if lens else None, dist_coeff=h["dist"] if lens else None, r2_max=R2_MAX if lens else None,
                             out=W.WarpMap(o[0], o[1], LINEAR, DSIZE))
        return [m.xy, m.frac]

    def built_ref(which, hw, lens):
        ref = ref_maps(hw, lens)
        return [np.stack([xy for xy, _ in ref]), np.stack([frac for _, frac in ref])]

    cases.append(Case("build_warp_map-pinhole", "bevwarp_build_map", no_inputs, lambda which: dict(M=MINVS[which]), no_maps, MAP_OUT,
                      lambda t, r, h, o: built(t, r, h, o, False), lambda which, hw: built_ref(which, hw, False)))
    cases.append(Case("build_warp_map-lens", "bevwarp_build_map", no_inputs, lambda which: dict(M=MINVS[which], K=K3, dist=DIST), no_maps, MAP_OUT,
                      lambda t, r, h, o: built(t, r, h, o, True), lambda which, hw: built_ref(which, hw, True)))

    # -- one camera through its map ------------------------------------------------------------------------------------------------------------------
    map_written = lambda: np.stack([RR.written(xy, SW, SH, LINEAR) for xy, _ in maps_a()])  # noqa: E731
    for no_out in (False, True):
        mode = _ref_mode(no_out)
        tag = "-no_out" * no_out
        cases.append(Case(
            "remap" + tag, "bevwarp_remap", frames, MAPPED, one_map, None if no_out else PX,
            lambda t, r, h, o: [W.remap(t[0], r, border_mode=_mode(o), border_value=h["border"], out=_o(o))],
            lambda which, hw, mode=mode: _stack([RR.remap(f, *maps_a()[i], LINEAR, mode, BORDER) for i, f in enumerate(frames(which)[0])]),
            sliceable=(0,), written=map_written if no_out else None))
        cases.append(Case(
            "remap_nv12" + tag, "bevwarp_remap_nv12", nv12, MAPPED, one_map, None if no_out else PX,
            lambda t, r, h, o: [W.remap_nv12(t[0], t[1], r, border_mode=_mode(o), border_value=h["border"], out=_o(o))],
            lambda which, hw, mode=mode: _stack([RN.remap_nv12(y, uv, *maps_a()[i], LINEAR, mode, BORDER) for i, (y, uv) in enumerate(zip(*nv12(which)))]),
            written=map_written if no_out else None))
    cases.append(Case(
        "remap_nv12_to_planar", "bevwarp_remap_nv12_planes", nv12, MAPPED_PLANES, one_map, planes_out(torch.float32),
        lambda t, r, h, o: [W.remap_nv12_to_planar(t[0], t[1], r, scale=h["scale"], bias=h["bias"], border_value=h["border"], out=o[0])],
        lambda which, hw: _stack([RN.remap_nv12_planes(y, uv, *maps_a()[i], LINEAR, RR.CONSTANT, SCALE, BIAS, BORDER) for i, (y, uv) in enumerate(zip(*nv12(which)))]),
        same_planes(torch.float32)))
    cases.append(Case(
        "remap_to_nv12", "bevwarp_remap_to_nv12", frames, MAPPED, one_map, NV12_OUT,
        lambda t, r, h, o: list(W.remap_to_nv12(t[0], r, border_value=h["border"], out=tuple(o))),
        lambda which, hw: _stack_pairs([RNO.remap_to_nv12(f, *maps_a()[i], LINEAR, RR.CONSTANT, BORDER) for i, f in enumerate(frames(which)[0])]), sliceable=(0,)))
    cases.append(Case(
        "remap_nv12_to_nv12", "bevwarp_remap_nv12_to_nv12", nv12, MAPPED, one_map, NV12_OUT,
        lambda t, r, h, o: list(W.remap_nv12_to_nv12(t[0], t[1], r, border_value=h["border"], out=tuple(o))),
        lambda which, hw: _stack_pairs([RNO.remap_nv12_to_nv12(y, uv, *maps_a()[i], LINEAR, RR.CONSTANT, BORDER) for i, (y, uv) in enumerate(zip(*nv12(which)))])))
    cases.append(Case(
        "remap_to_planar", "bevwarp_remap_planes", frames, MAPPED_PLANES, one_map, planes_out(torch.float32),
        lambda t, r, h, o: [W.remap_to_planar(t[0], r, scale=h["scale"], bias=h["bias"], border_value=h["border"], out=o[0])],
        lambda which, hw: _stack([MP.remap_planes(f, *maps_a()[i], LINEAR, RR.CONSTANT, SCALE, BIAS, BORDER) for i, f in enumerate(frames(which)[0])]),
        same_planes(torch.float32), sliceable=(0,)))

    # -- two overlapping cameras into one canvas, feathered -----------------------------------------------------------------------------------------------
    def cam_frames(which, i):
        return [f[i] for f in camera_frames(which)]

    def cam_nv12(which, i):
        y0, y1, uv0, uv1 = camera_nv12(which)
        return [y0[i], y1[i]], [uv0[i], uv1[i]]

    for no_out in (False, True):
        mode = SR.TRANSPARENT if no_out else SR.CONSTANT
        tag = "-no_out" * no_out
        cases.append(Case(
            "warp_stitch" + tag, "bevwarp_warp_stitch", camera_frames, STITCH_MATS, no_maps, None if no_out else PX,
            lambda t, r, h, o: [W.warp_stitch(t, [h["M0"], h["M1"]], DSIZE, flags=FLAGS, blend="feather", feather=FEATHER, border_value=h["border"], out=_o(o),
                                              border_mode=_mode(o))],
            lambda which, hw, mode=mode: _stack([SR.stitch(cam_frames(which, i), [CAM_MINVS[0][i], CAM_MINVS[1][i]], DSIZE, LINEAR, SR.FEATHER, FEATHER, mode, BORDER)[0]
                                                 for i in range(BATCH)]),
            sliceable=(0, 1), written=(lambda: stitch_cover() > 0) if no_out else None, cover=stitch_cover))
        cases.append(Case(
            "remap_stitch" + tag, "bevwarp_stitch_maps", camera_frames, MAPPED, camera_maps, None if no_out else PX,
            lambda t, r, h, o: [W.remap_stitch(t, r, blend="feather", feather=FEATHER, border_value=h["border"], out=_o(o), border_mode=_mode(o))],
            lambda which, hw, mode=mode: _stack([SM.stitch(cam_frames(which, i), cam_refs(i), LINEAR, SM.FEATHER, FEATHER, mode, BORDER)[0] for i in range(BATCH)]),
            sliceable=(0, 1), written=(lambda: stitch_cover() > 0) if no_out else None, cover=stitch_cover))
        cases.append(Case(
            "remap_stitch_nv12" + tag, "bevwarp_stitch_maps_nv12", camera_nv12, MAPPED, camera_maps, None if no_out else PX,
            lambda t, r, h, o: [W.remap_stitch_nv12(t[:2], t[2:], r, blend="feather", feather=FEATHER, border_value=h["border"], out=_o(o), border_mode=_mode(o))],
            lambda which, hw, mode=mode: _stack([SM.stitch_nv12(*cam_nv12(which, i), cam_refs(i), LINEAR, SM.FEATHER, FEATHER, mode, BORDER)[0] for i in range(BATCH)]),
            written=(lambda: stitch_cover() > 0) if no_out else None, cover=stitch_cover))
    cases.append(Case(
        "remap_stitch_to_nv12", "bevwarp_stitch_maps_to_nv12", camera_frames, MAPPED, camera_maps, NV12_OUT,
        lambda t, r, h, o: list(W.remap_stitch_to_nv12(t, r, blend="feather", feather=FEATHER, border_value=h["border"], out=tuple(o))),
        lambda which, hw: _stack_pairs([RNO.stitch_to_nv12(cam_frames(which, i), cam_refs(i), LINEAR, SM.FEATHER, FEATHER, BORDER) for i in range(BATCH)]),
        sliceable=(0, 1), cover=stitch_cover))
    cases.append(Case(
        "remap_stitch_nv12_to_nv12", "bevwarp_stitch_maps_nv12_to_nv12", camera_nv12, MAPPED, camera_maps, NV12_OUT,
        lambda t, r, h, o: list(W.remap_stitch_nv12_to_nv12(t[:2], t[2:], r, blend="feather", feather=FEATHER, border_value=h["border"], out=tuple(o))),
        lambda which, hw: _stack_pairs([RNO.stitch_nv12_to_nv12(*cam_nv12(which, i), cam_refs(i), LINEAR, SM.FEATHER, FEATHER, BORDER) for i in range(BATCH)]),
        cover=stitch_cover))
    cases.append(Case(
        "remap_stitch_to_planar", "bevwarp_stitch_maps_planes", camera_frames, MAPPED_PLANES, camera_maps, planes_out(torch.float32),
        lambda t, r, h, o: [W.remap_stitch_to_planar(t, r, scale=h["scale"], bias=h["bias"], blend="feather", feather=FEATHER, border_value=h["border"], out=o[0])],
        lambda which, hw: _stack([MP.stitch_planes(cam_frames(which, i), cam_refs(i), LINEAR, SCALE, BIAS, SM.FEATHER, FEATHER, BORDER) for i in range(BATCH)]),
        same_planes(torch.float32), sliceable=(0, 1), cover=stitch_cover))
    cases.append(Case(
        "remap_stitch_nv12_to_planar", "bevwarp_stitch_maps_nv12_planes", camera_nv12, MAPPED_PLANES, camera_maps, planes_out(torch.float32),
        lambda t, r, h, o: [W.remap_stitch_nv12_to_planar(t[:2], t[2:], r, scale=h["scale"], bias=h["bias"], blend="feather", feather=FEATHER, border_value=h["border"],
                                                          out=o[0])],
        lambda which, hw: _stack([MP.stitch_nv12_planes(*cam_nv12(which, i), cam_refs(i), LINEAR, SCALE, BIAS, SM.FEATHER, FEATHER, BORDER) for i in range(BATCH)]),
        same_planes(torch.float32), cover=stitch_cover))

    # -- one camera through its matrices: NV12 in, NV12 out, channel planes -----------------------------------------------------------------------------------
    def warped_nv12(which):
        return [NR.warp_nv12(y, uv, M, DSIZE, co.LINEAR, border_value=BORDER, m_is_inverse=True) for y, uv, M in zip(*nv12(which), MINVS["A"])]

    def warped(which):
        return [co.warp_perspective(f, M, DSIZE, co.LINEAR, m_is_inverse=True, border_value=BORDER) for f, M in zip(frames(which)[0], MINVS["A"])]

    cases.append(Case(
        "warp_perspective_nv12", "bevwarp_warp_nv12", nv12, MATS, no_maps, PX,
        lambda t, r, h, o: [W.warp_perspective_nv12(t[0], t[1], h["M"], DSIZE, flags=FLAGS, border_value=h["border"], out=o[0])],
        lambda which, hw: _stack(warped_nv12(which))))
    cases.append(Case(
        "warp_nv12_to_planar", "bevwarp_warp_nv12_planes", nv12, PLANES, no_maps, planes_out(torch.float32),
        lambda t, r, h, o: [W.warp_nv12_to_planar(t[0], t[1], h["M"], DSIZE, scale=h["scale"], bias=h["bias"], flags=FLAGS, border_value=h["border"], out=o[0])],
        lambda which, hw: _stack([RN.planes_f32(p, SCALE, BIAS) for p in warped_nv12(which)]), same_planes(torch.float32)))
    cases.append(Case(
        "warp_perspective_to_nv12", "bevwarp_warp_to_nv12", frames, MATS, no_maps, NV12_OUT,
        lambda t, r, h, o: list(W.warp_perspective_to_nv12(t[0], h["M"], DSIZE, flags=FLAGS, border_value=h["border"], out=tuple(o))),
        lambda which, hw: _stack_pairs([NO.warp_to_nv12(f, M, DSIZE, co.LINEAR, border_value=BORDER, m_is_inverse=True) for f, M in zip(frames(which)[0], MINVS["A"])]),
        sliceable=(0,)))
    cases.append(Case(
        "warp_nv12_to_nv12", "bevwarp_warp_nv12_to_nv12", nv12, MATS, no_maps, NV12_OUT,
        lambda t, r, h, o: list(W.warp_nv12_to_nv12(t[0], t[1], h["M"], DSIZE, flags=FLAGS, border_value=h["border"], out=tuple(o))),
        lambda which, hw: _stack_pairs([NO.warp_nv12_to_nv12(y, uv, M, DSIZE, co.LINEAR, border_value=BORDER, m_is_inverse=True) for y, uv, M in zip(*nv12(which), MINVS["A"])])))
    for dtype, symbol in ((torch.float32, "bevwarp_warp_planar"), (torch.float16, "bevwarp_warp_planes")):
        cases.append(Case(
            "warp_to_planar-" + str(dtype)[6:], symbol, frames, PLANES, no_maps, planes_out(dtype),
            lambda t, r, h, o, dtype=dtype: [W.warp_to_planar(t[0], h["M"], DSIZE, scale=h["scale"], bias=h["bias"], flags=FLAGS, border_value=h["border"], out=o[0],
                                                              out_dtype=dtype)],
            lambda which, hw: _stack([RN.planes_f32(p, SCALE, BIAS) for p in warped(which)]), same_planes(dtype), sliceable=(0,)))

    # -- resize and the points ---------------------------------------------------------------------------------------------------------------------------
    cases.append(Case(
        "resize", "bevwarp_resize", frames, _values(), no_maps, PX, lambda t, r, h, o: [RZ.resize(t[0], DSIZE, out=o[0])],
        lambda which, hw: _stack([co.resize_linear_u8(f, DSIZE) for f in frames(which)[0]]), sliceable=(0,)))
    H = MINVS["A"][0]
    cases.append(Case(
        "distort_points", "bevwarp_project_points_lens", lambda which: points(which, PR.DISTORT), _values(K=K3, dist=DIST, H=H), no_maps, POINTS_OUT,
        lambda t, r, h, o: [PT.distort_points(t[0], h["K"], h["dist"], H=h["H"], r2_max=R2_MAX, out=o[0])],
        lambda which, hw: [PR.distort(points(which, PR.DISTORT)[0], _lens_rays(H), LR.lens12(K, DIST), R2_MAX)], same_points))
    Hf = np.linalg.inv(H)  # undistorted source px -> destination px
    cases.append(Case(
        "undistort_points", "bevwarp_project_points_lens", lambda which: points(which, PR.UNDISTORT), _values(K=K3, dist=DIST, H=Hf), no_maps, POINTS_OUT,
        lambda t, r, h, o: [PT.undistort_points(t[0], h["K"], h["dist"], H=h["H"], r2_max=R2_MAX, out=o[0])],
        lambda which, hw: [PR.undistort(points(which, PR.UNDISTORT)[0], Hf @ K3, LR.lens12(K, DIST), R2_MAX, 20, 1e-3)[0]], same_points))
    cases.append(Case(
        "project_points", "bevwarp_project_points", lambda which: points(which, PR.DISTORT), _values(H=H), no_maps, POINTS_OUT,
        lambda t, r, h, o: [PT.project_points(t[0], h["H"], out=o[0])],
        lambda which, hw: [co.project_points(points(which, PR.DISTORT)[0], H)], same_points))  # (float32: the same float64 arithmetic, one rounding)
    return cases


CASES = _cases()
COPIED_SOURCE = [c for c in CASES if c.sliceable]
NO_OUT = [c for c in CASES if c.no_out]


# ---- the checks -------------------------------------------------------------------------------------------------------------------------------------
class Gpu:
    """The backend of the GPU tests: tensors on `device`, side streams, a delay of `sleep_cycles` behind an event, graph capture."""

    def __init__(self, device="cuda:0", sleep_cycles=0):
        self.device, self.sleep_cycles = torch.device(device), int(sleep_cycles)

    def empty(self, shape, dtype):
        return torch.empty(tuple(shape), dtype=dtype, device=self.device)

    def staged(self, a):
        return torch.from_numpy(np.array(a)).pin_memory()

    def copy_async(self, t, staged):
        t.copy_(staged, non_blocking=True)

    def fill(self, t, value):
        t.fill_(value)

    def synchronize(self):
        torch.cuda.synchronize(self.device)

    @contextlib.contextmanager
    def side_stream(self):
        s = torch.cuda.Stream(self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            yield s

    def delay(self):
        torch.cuda._sleep(self.sleep_cycles)
        e = torch.cuda.Event()
        e.record()
        return e

    def capture(self, thunk):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ret = thunk()
        return ret, g


def measure_sleep(cycles):
    """Milliseconds torch.cuda._sleep(cycles) takes on the current device, between two events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    torch.cuda._sleep(int(cycles))
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def sleep_cycles_for(target_ms=50.0):
    """(cycles, measured milliseconds) of a torch.cuda._sleep of about target_ms: nothing fixes the counter's rate in advance, so a probe of
    100,000 cycles is timed (once more ten times as long while it takes under 0.2 ms: a launch's own latency would dominate), the count is
    scaled, and the scaled delay is timed."""
    cycles = 100_000
    measure_sleep(cycles)  # (the kernel's first launch loads it)
    ms = measure_sleep(cycles)
    for _ in range(3):
        if ms >= 0.2:
            break
        cycles *= 10
        ms = measure_sleep(cycles)
    cycles = max(1, int(cycles * target_ms / max(ms, 1e-3)))
    return cycles, measure_sleep(cycles)


def _torch_dtype(a):
    return torch.from_numpy(np.zeros(0, a.dtype)).dtype


def input_tensors(case, backend, sliced=False):
    """The device tensors of a case's inputs, uninitialised; sliced: the interleaved frames are channels 0..2 of 4-channel holders."""
    tensors = []
    for i, a in enumerate(case.inputs("A")):
        if sliced and i in case.sliceable:
            holder = backend.empty(a.shape[:-1] + (4,), _torch_dtype(a))
            backend.fill(holder, POISON)
            tensors.append(holder[..., :3])
            assert not tensors[-1].is_contiguous()
        else:
            tensors.append(backend.empty(a.shape, _torch_dtype(a)))
    return tensors


def load(case, backend, tensors, which):
    """Set `which` copied into the input tensors in place."""
    for t, a in zip(tensors, case.inputs(which)):
        t.copy_(torch.from_numpy(np.array(a)))  # (a copy: the sets are read-only arrays)
    backend.synchronize()


def destination(case, backend):
    return None if case.no_out else [backend.empty(shape, dtype) for shape, dtype in case.out_shapes]


def poison(backend, tensors):
    for t in tensors or ():
        backend.fill(t, POISON)


def still_poisoned(tensors):
    return all(bool((t == POISON).all().item()) for t in tensors)


def check_side_stream(case, backend, sliced=False):
    """Returns (host seconds of the call, milliseconds the stream took from the start of the delay to the end of the launch)."""
    exp_a, exp_b = case.expected("A", "A"), case.expected("B", "B")
    assert differ(exp_a, exp_b), "%s: the two sets have one expected result" % case.name
    tensors, resident, outs = input_tensors(case, backend, sliced), case.resident(backend.device), destination(case, backend)
    load(case, backend, tensors, "A")
    for which in ("B", "A"):  # warm-up: the library is loaded and both sets' matrices are uploaded (device_inverse)
        case.call(tensors, resident, case.host(which), outs)
    backend.synchronize()
    poison(backend, outs)
    backend.synchronize()
    staged = [backend.staged(a) for a in case.inputs("B")]
    host_b = case.host("B")
    with backend.side_stream() as s:
        e = backend.delay()
        for t, p in zip(tensors, staged):
            backend.copy_async(t, p)
        poison(backend, outs)  # (in stream order: what a launch on another stream wrote in the meantime is overwritten)
        t0 = time.perf_counter()
        got = case.call(tensors, resident, host_b, outs)
        host_s = time.perf_counter() - t0
        pending = not e.query()
    assert pending, "%s: the delay was over when the call returned after %.1f ms: this run proves nothing" % (case.name, host_s * 1e3)
    s.synchronize()
    case.compare(got, exp_b)
    return host_s


def check_replays(case, backend, sliced=False):
    host = case.host("A")
    exp = {which: case.expected(which, "A") for which in SETS}
    if case.inputs("A"):
        assert differ(exp["A"], exp["B"]), "%s: the two sets have one expected result" % case.name
    tensors, resident, outs = input_tensors(case, backend, sliced), case.resident(backend.device), destination(case, backend)
    load(case, backend, tensors, "A")
    with backend.side_stream() as s:  # warm-up on a side stream, as torch's capture recipe does
        case.call(tensors, resident, host, outs)
        s.synchronize()
    backend.synchronize()
    poison(backend, outs)
    backend.synchronize()
    got, graph = backend.capture(lambda: case.call(tensors, resident, host, outs))
    backend.synchronize()
    if outs is not None:
        assert all(g is o for g, o in zip(got, outs)) and still_poisoned(outs), "%s: the capture itself wrote the destination" % case.name
    for a in host.values():  # what the caller may do with its arrays once the call has returned
        a[...] = np.nan
    for which in ("B", "A"):
        poison(backend, got)  # (a result allocated inside the capture too: its zero fill has to be a node of the graph)
        load(case, backend, tensors, which)
        graph.replay()
        backend.synchronize()
        try:
            case.compare(got, exp[which])
        except AssertionError as err:
            raise AssertionError("%s: replay on set %s: %s" % (case.name, which, err)) from None


def check_second_device(case, backend):
    """`backend` lives on another device than the current one, which must stay current."""
    current = torch.cuda.current_device()
    assert backend.device.index != current
    tensors, resident, outs = input_tensors(case, backend), case.resident(backend.device), destination(case, backend)
    load(case, backend, tensors, "A")
    poison(backend, outs)
    backend.synchronize()
    got = case.call(tensors, resident, case.host("A"), outs)
    backend.synchronize()
    case.compare(got, case.expected("A", "A"))
    assert all(g.device == backend.device for g in got)
    assert torch.cuda.current_device() == current
