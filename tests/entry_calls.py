"""What the Python warp entry points (bev_amd/warp.py, bev_amd/resize.py) hand to the C ABI, written down so that two runs compare equal.

`record_all(device)` runs a fixed list of calls with `bev_amd._lib._lib` replaced by a stub whose `bevwarp_*` attributes record
`(name, arguments)` and return 0: no kernel of the library runs, the entry points' own argument handling is all that is exercised.
tests/golden/make_entry_calls.py writes the records to tests/golden/entry_calls.json; tests/test_gpu_entry_calls.py regenerates them
and compares.  A GPU is needed because the entry points insist on CUDA tensors and a current stream.

How arguments are written down: an integer that is the address of a known tensor plus an offset becomes "name+offset" (the case's
inputs by name; the returned tensor "ret", the entries of _minv_cache "minv", the verdict table "table"; any other allocation of the
entry, e.g. the contiguous copy of a non-contiguous source, "new0", "new1", ... in order of appearance); the stream handle becomes
"stream"; host arrays are read back as float64 lists (HOST: where they sit and how long they are); None stays None."""
import ctypes

import numpy as np
import torch

from bev_amd import _lib, warp
from bev_amd import resize as rz

TABLE_BYTES = 48  # the stub's answer to bevwarp_tile_classes_bytes: warp_perspective's verdict-table branch is taken, with a small real table
_HOST_FNS = ("bevwarp_version", "bevwarp_strerror", "bevwarp_last_hip_error", "bevwarp_invert_homography")  # no launch: the real ones
# symbol -> {position of a host float64 array: its length, "C" = the channel count at position 7}
HOST = {
    "bevwarp_warp": {16: "C"}, "bevwarp_warp_classes": {16: "C"}, "bevwarp_warp_border": {17: "C"}, "bevwarp_warp_lens": {14: 12, 19: "C"},
    "bevwarp_warp_planar": {17: "C", 18: "C", 19: "C"}, "bevwarp_warp_planes": {17: "C", 18: "C", 19: "C"}, "bevwarp_warp_nv12": {18: 3},
    "bevwarp_warp_nv12_planes": {19: 3, 20: 3, 21: 3}, "bevwarp_warp_to_nv12": {18: 3}, "bevwarp_warp_nv12_to_nv12": {20: 3},
}
# symbol -> position of the destination address (the returned tensor's address is recorded relative to it)
DST = {"bevwarp_warp_nv12": 2, "bevwarp_warp_nv12_planes": 2, "bevwarp_warp_nv12_to_nv12": 2, "bevwarp_footprint": 0}

M1 = np.array([[1.1, 0.02, 0.5], [0.01, 0.9, -0.3], [1e-4, 2e-4, 1.0]])
M2 = np.stack([M1, M1 + np.diag([0.125, 0.0, 0.0])])
K33 = np.array([[7.0, 0.0, 4.0], [0.0, 7.5, 3.0], [0.0, 0.0, 1.0]])
K34 = np.hstack([K33, np.zeros((3, 1))])
DIST = {4: [-0.2, 0.05, 1e-3, -2e-3], 5: [-0.2, 0.05, 1e-3, -2e-3, 0.01], 8: [-0.2, 0.05, 1e-3, -2e-3, 0.01, 0.02, -0.01, 0.005]}
DS, DS12 = (6, 4), (4, 6)  # dsize (width, height): 6 x 8 sources -> 4 x 6, and 8 x 8 NV12 frames -> 6 x 4
U8, F32 = torch.uint8, torch.float32


def _extent(t):
    if t.numel() == 0:
        return 0
    return (sum((n - 1) * s for n, s in zip(t.shape, t.stride())) + 1) * t.element_size()


class StubLibrary:
    """Stands in for the loaded library: every launching symbol records its arguments (host arrays read on the spot) and succeeds."""

    def __init__(self, real):
        self.calls = []
        for name in _lib.SYMBOLS:
            setattr(self, name, getattr(real, name) if name in _HOST_FNS else self._entry(name))

    def _entry(self, name):
        def fn(*args):
            if name == "bevwarp_tile_classes_bytes":
                return TABLE_BYTES
            args = list(args)
            for pos, n in HOST.get(name, {}).items():
                if args[pos] is not None:
                    assert isinstance(args[pos], ctypes.c_void_p), (name, pos, args[pos])
                    args[pos] = list((ctypes.c_double * (args[7] if n == "C" else n)).from_address(args[pos].value))
            if isinstance(args[-1], ctypes.c_void_p):
                args[-1] = args[-1].value
            self.calls.append((name, args))
            return 0
        fn.__name__ = name
        return fn


class Recorder:
    def __init__(self, device, stub, stream):
        self.dev, self.stub, self.stream = device, stub, stream
        self.cases = {}

    def begin(self, cid, **named):
        assert cid not in self.cases, cid
        warp._plans.clear()
        warp._class_tables.clear()
        warp._minv_cache.clear()
        self.named, self.steps = dict(named), []
        self.cases[cid] = self.steps

    def _label(self, v, known, new):
        if isinstance(v, list):
            return [self._label(x, known, new) for x in v]
        if isinstance(v, bool) or not isinstance(v, int) or v < (1 << 24):
            return v
        for name, t in known:
            if t.data_ptr() <= v < t.data_ptr() + _extent(t):
                return "%s+%d" % (name, v - t.data_ptr())
        return new.setdefault(v, "new%d" % len(new))

    def _args(self, args, known, new):
        args = list(args)
        tail = ["stream"] if args and self.stream and args[-1] == self.stream else []
        return [self._label(a, known, new) for a in args[:len(args) - len(tail)]] + tail

    def call(self, fn, *args, zero=False, **kw):
        """One call of an entry point: its record is appended to the current case."""
        del self.stub.calls[:]
        before = dict(warp._plans)
        out = kw.get("out", kw.get("dst"))
        try:
            ret = fn(*args, **kw)
        except Exception as e:  # noqa: BLE001 -- the type and the text are the record
            self.steps.append({"raises": [type(e).__name__, str(e)]})
            return None
        known = list(self.named.items())
        rets = ret if isinstance(ret, tuple) and ret is not out else (ret,)
        known += [("ret%d" % k if len(rets) > 1 else "ret", t) for k, t in enumerate(rets) if isinstance(t, torch.Tensor)]
        known += [("minv%d" % k if k else "minv", t) for k, t in enumerate(warp._minv_cache.values())]
        known += [("table", e[0]) for e in warp._class_tables.values()]
        new = {}
        calls = list(self.stub.calls)
        rec = {"calls": [[name, self._args(a, known, new)] for name, a in calls]}
        dst = calls[-1][1][DST.get(calls[-1][0], 1)] if calls else 0
        rec["ret"] = [self._returned(t, out, dst) for t in rets]
        if zero:
            rec["zero"] = bool((torch.as_tensor(ret) == 0).all())
        gained = [k for k in warp._plans if k not in before]
        rec["plans"] = len(warp._plans) - len(before)
        if gained:
            plan = warp._plans[gained[0]]
            rec["plan"] = {"fn": plan[0].__name__, "args": self._args(plan[1], known, new), "table": plan[3] is not None, "plain": plan[6].__name__}
        self.steps.append(rec)
        return ret

    @staticmethod
    def _returned(t, out, dst):
        if isinstance(t, np.ndarray):
            return {"is_out": t is out, "numpy": [list(t.shape), str(t.dtype)]}
        if not isinstance(t, torch.Tensor):
            return {"is_out": t is out, "type": type(t).__name__}
        return {"is_out": t is out, "shape": list(t.shape), "stride": list(t.stride()), "dtype": str(t.dtype),
                "at": dst - t.data_ptr() if t.data_ptr() <= dst < t.data_ptr() + max(_extent(t), 1) else "elsewhere"}  # (of the destination argument within it)


def _cases(r):
    dev, cpu = r.dev, torch.device("cpu")
    wp, lens, planar = warp.warp_perspective, warp.warp_perspective_lens, warp.warp_to_planar
    nv12, nv12p, to12, n2n = warp.warp_perspective_nv12, warp.warp_nv12_to_planar, warp.warp_perspective_to_nv12, warp.warp_nv12_to_nv12
    T = warp.BORDER_TRANSPARENT

    def z(shape, dtype=U8, device=dev):
        return torch.zeros(tuple(shape), dtype=dtype, device=device)

    def minv(n=1):
        return torch.eye(3, dtype=torch.float64, device=dev).repeat(n, 1, 1)

    def one(cid, fn, *args, **kw):
        """A case of one call whose tensor arguments are known by their position or keyword."""
        named = {"a%d" % k: a for k, a in enumerate(args) if isinstance(a, torch.Tensor) and a.is_cuda}
        named.update({k: v for k, v in kw.items() if isinstance(v, torch.Tensor) and v.is_cuda})
        if isinstance(kw.get("out"), (tuple, list)):
            named.update({"out%d" % k: v for k, v in enumerate(kw["out"]) if isinstance(v, torch.Tensor) and v.is_cuda})
        r.begin(cid, **named)
        return r.call(fn, *args, **kw)

    # ---- warp_perspective
    shapes = [(6, 8)] + [(6, 8, c) for c in (1, 2, 3, 4)] + [(b, 6, 8, c) for b in (1, 2) for c in (1, 2, 3, 4)]
    for dt in (U8, F32):
        for s in shapes:
            one("wp/%s/%s" % (str(dt)[6:], "x".join(map(str, s))), wp, z(s, dt), M1, DS)
    for interp in (0, 1, 2):
        for mode in range(6):
            one("wp/interp%d/border%d" % (interp, mode), wp, z((6, 8, 3)), M1, DS, flags=interp, border_mode=mode, zero=mode == T)
    one("wp/inverse_map", wp, z((6, 8, 3)), M1, DS, flags=1 | warp.WARP_INVERSE_MAP)
    one("wp/flag_bits_above_7", wp, z((6, 8, 3)), M1, DS, flags=1 | 32)
    for name, bv in (("scalar", 7), ("per_channel", (1, 2, 3))):
        for interp, mode in ((1, 0), (2, 0), (1, 1), (2, T)):
            one("wp/border_value_%s/interp%d/border%d" % (name, interp, mode), wp, z((2, 6, 8, 3), F32), M2, DS, flags=interp, border_value=bv, border_mode=mode)
    for mode in (0, 1, T):
        one("wp/out/border%d" % mode, wp, z((2, 6, 8, 3)), M1, DS, out=z((2, 4, 6, 3)), border_mode=mode)
    one("wp/out_flat", wp, z((2, 6, 8, 3), F32), M1, DS, out=z((2 * 4 * 6 * 3,), F32))
    one("wp/out_for_2d", wp, z((6, 8)), M1, DS, out=z((4, 6)))
    one("wp/out_row_padded", wp, z((6, 8, 3)), M1, DS, out=z((4, 8, 3))[:, :6])
    for name, M, flags in (("cpu_tensor", torch.from_numpy(M1), 1), ("cpu_tensor_f32", torch.from_numpy(M2).float(), 1), ("cuda_tensor", torch.from_numpy(M1).to(dev), 1),
                           ("cuda_tensor_inverse", torch.from_numpy(M2).to(dev), 17), ("cuda_tensor_f32_inverse", torch.from_numpy(M1).float().to(dev), 17),
                           ("numpy_B", M2, 1), ("list", M1.tolist(), 1), ("numpy_1x3x3", M1[None], 17)):
        r.begin("wp/M_%s" % name, src=z((2, 6, 8, 3)), **({"M": M} if isinstance(M, torch.Tensor) and M.is_cuda else {}))
        r.call(wp, r.named["src"], M, DS, flags=flags)
    one("wp/M_inv_device", wp, z((2, 6, 8, 3)), None, DS, M_inv_device=minv(2))
    one("wp/M_inv_device_shared", wp, z((2, 6, 8, 1), F32), None, DS, M_inv_device=minv(1), border_value=3)
    big = z((2, 6, 16, 4))
    one("wp/src_channel_slice", wp, big[..., :8, :3], M1, DS)
    one("wp/src_column_step", wp, big[:, :, ::2], M1, DS)
    one("wp/src_row_padded", wp, big[:, :, 1:9], M1, DS)
    one("wp/src_row_padded_2d", wp, z((6, 16))[:, 3:11], M1, DS)
    one("wp/src_frame_step", wp, z((4, 6, 8, 3))[::2], M2, DS)
    # the camera loop: the same call again is served from the plan, with the same bound arguments
    for name, owned in (("owned", True), ("callers", False)):
        for mode, interp in ((0, 1), (0, 2), (1, 1), (T, 0)):
            r.begin("wp/twice_%s/interp%d/border%d" % (name, interp, mode), src=z((2, 6, 8, 3)), out=z((2, 4, 6, 3)))
            mi = warp.device_inverse(M2, dev) if owned else minv(2)
            if not owned:
                r.named["mi"] = mi
            for _ in range(3):
                r.call(wp, r.named["src"], None, DS, flags=interp, out=r.named["out"], M_inv_device=mi, border_mode=mode)
    r.begin("wp/twice_copied_source", src=z((6, 8, 4))[..., :3], out=z((4, 6, 3)), mi=minv())
    for _ in range(2):
        r.call(wp, r.named["src"], None, DS, out=r.named["out"], M_inv_device=r.named["mi"])
    r.begin("wp/twice_matrices_written_in_place", src=z((6, 8, 3)), out=z((4, 6, 3)))
    mi = warp.device_inverse(M1, dev)
    r.call(wp, r.named["src"], None, DS, out=r.named["out"], M_inv_device=mi)
    mi.mul_(1.0)
    r.call(wp, r.named["src"], None, DS, out=r.named["out"], M_inv_device=mi)

    # ---- warp_perspective_lens
    for name, d in (("none", None), ("zeros", np.zeros(5)), ("4", DIST[4]), ("5", DIST[5]), ("8", DIST[8])):
        for s in ((6, 8), (6, 8, 3), (2, 6, 8, 3)):
            one("lens/dist_%s/%s" % (name, "x".join(map(str, s))), lens, z(s), M1, DS, K33, d)
    for name, r2 in (("number", 0.75), ("inf", float("inf"))):
        one("lens/r2_%s" % name, lens, z((6, 8, 3), F32), M1, DS, K34, DIST[5], r2_max=r2)
    for interp in (0, 1):
        for mode in (0, T):
            one("lens/interp%d/border%d" % (interp, mode), lens, z((2, 6, 8, 3)), M2, DS, K33, DIST[8], flags=interp, border_mode=mode, border_value=(1, 2, 3), zero=mode == T)
    one("lens/inverse_map_tensor_M", lens, z((6, 8, 1), F32), torch.from_numpy(M1), DS, K33, DIST[4], flags=17)
    one("lens/out", lens, z((2, 6, 8, 3)), M1, DS, K33, DIST[5], out=z((2, 4, 6, 3)), border_mode=T)
    one("lens/out_flat_2d", lens, z((6, 8), F32), M1, DS, K33, DIST[5], out=z((24,), F32), border_value=2)
    one("lens/src_channel_slice", lens, z((6, 8, 4))[..., :3], M1, DS, K33, DIST[5])
    one("lens/src_row_padded", lens, z((6, 16, 3))[:, 4:12], M1, DS, K33, DIST[5])
    one("lens/zeros_forward_everything", lens, z((6, 8, 3)), M1, DS, K33, None, flags=2, border_value=5, out=z((4, 6, 3)), border_mode=1)

    # ---- warp_to_planar
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        tag = str(dt)[6:]
        one("planar/%s" % tag, planar, z((2, 6, 8, 3)), M1, DS, out_dtype=dt)
        one("planar/%s/out" % tag, planar, z((2, 6, 8, 3)), M2, DS, out=z((2, 3, 4, 6), dt), out_dtype=dt, scale=(0.5, 0.25, 0.125), bias=(-1, 0, 1))
        one("planar/%s/out_row_padded_single" % tag, planar, z((6, 8, 3), F32), M1, DS, out=z((3, 4, 8), dt)[..., :6], out_dtype=dt, flags=0, border_value=(1, 2, 3))
    one("planar/2d", planar, z((6, 8)), M1, DS, scale=2.0, bias=0.5, border_value=9)
    one("planar/single_frame", planar, z((6, 8, 4)), M1, DS, flags=17)
    one("planar/src_channel_slice", planar, z((2, 6, 8, 4))[..., :2], M1, DS, out_dtype=torch.float16)
    one("planar/M_inv_device", planar, z((2, 6, 8, 3)), None, DS, M_inv_device=minv(2))

    # ---- the NV12 sources: warp_perspective_nv12, warp_nv12_to_planar, warp_nv12_to_nv12
    def nv12_planes(kind, B):
        """(named tensors, y, uv) of 8 x 8 frames: views of one joined buffer, or separate row-padded planes"""
        lead = () if B == 0 else (B,)
        if kind == "joined":
            frame = z(lead + (12, 8))
            return {"frame": frame}, *warp.split_nv12(frame)
        y, uv = z(lead + (8, 16))[..., :8], z(lead + (4, 8, 2))[..., :4, :]
        return {"y": y, "uv": uv}, y, uv

    for kind in ("joined", "padded"):
        for B in (0, 1, 2):
            tag = "%s/B%d" % (kind, B)
            M = M2 if B == 2 else M1
            for rgb in (False, True):
                named, y, uv = nv12_planes(kind, B)
                r.begin("nv12/%s/rgb%d" % (tag, rgb), **named)
                r.call(nv12, y, uv, M, DS12, rgb=rgb, flags=int(rgb), border_value=(1, 2, 3) if rgb else None)
                r.begin("nv12p/%s/rgb%d" % (tag, rgb), **named)
                r.call(nv12p, y, uv, M, DS12, rgb=rgb, flags=int(rgb), scale=(1, 2, 3) if rgb else 1 / 255.0, bias=0.5 if rgb else (3, 2, 1),
                       out_dtype=torch.float16 if rgb else torch.float32)
            named, y, uv = nv12_planes(kind, B)
            r.begin("n2n/%s" % tag, **named)
            r.call(n2n, y, uv, M, DS12, flags=B % 2, border_value=None if B else 16)
    Bn = 2
    named, y, uv = nv12_planes("joined", Bn)
    r.begin("nv12/out", out=z((Bn, 6, 4, 3)), **named)
    r.call(nv12, y, uv, M1, DS12, out=r.named["out"])
    r.begin("nv12/out_flat_M_inv_device", out=z((Bn * 72,)), mi=minv(2), **named)
    r.call(nv12, y, uv, None, DS12, out=r.named["out"], M_inv_device=r.named["mi"], border_value=4)
    r.begin("nv12p/out_bf16", out=z((Bn, 3, 6, 4), torch.bfloat16), **named)
    r.call(nv12p, y, uv, M1, DS12, out=r.named["out"], out_dtype=torch.bfloat16, border_value=(3, 2, 1))
    r.begin("nv12p/out_row_padded", out=z((Bn, 3, 6, 8), F32)[..., :4], mi=minv(1), **named)
    r.call(nv12p, y, uv, None, DS12, out=r.named["out"], M_inv_device=r.named["mi"])

    # ---- the NV12 destinations: warp_perspective_to_nv12, warp_nv12_to_nv12
    def nv12_out(kind, B):
        lead = () if B == 0 else (B,)
        if kind == "absent":
            return None
        if kind == "joined":
            return z(lead + (9, 4))
        return (z(lead + (6, 8))[..., :4], z(lead + (3, 4, 2))[..., :2, :])

    for kind in ("absent", "joined", "pair"):
        for B in (0, 1, 2):
            tag = "%s/B%d" % (kind, B)
            M = M2 if B == 2 else M1
            one("to12/%s" % tag, to12, z(((B,) if B else ()) + (6, 8, 3)), M, DS12, out=nv12_out(kind, B), rgb=bool(B % 2), flags=B % 2, border_value=(1, 2, 3) if B else None)
            named, y, uv = nv12_planes("joined" if B else "padded", B)
            o = nv12_out(kind, B)
            named.update({} if o is None else {"out": o} if isinstance(o, torch.Tensor) else {"out0": o[0], "out1": o[1]})
            r.begin("n2n/out_%s" % tag, **named)
            r.call(n2n, y, uv, M, DS12, out=o)
    one("to12/src_channel_slice", to12, z((6, 8, 4))[..., :3], M1, DS12)
    one("to12/M_inv_device_list_pair", to12, z((2, 6, 8, 3)), None, DS12, M_inv_device=minv(2), out=list(nv12_out("pair", 2)))
    named, y, uv = nv12_planes("padded", 1)
    r.begin("n2n/out_M_inv_device", out=z((1, 9, 4)), mi=minv(1), **named)  # the streaming caller's call
    r.call(n2n, y, uv, None, DS12, out=r.named["out"], M_inv_device=r.named["mi"])

    # ---- footprint, resize, warp_perspective_resized, warpPerspective
    one("footprint/one", warp.footprint, (6, 8), M1, DS, device=dev)
    one("footprint/batch_nearest", warp.footprint, (6, 8), M1, DS, batch=3, flags=0, device="cuda")
    one("footprint/per_frame_inverse", warp.footprint, (6, 8), M2, DS, flags=17, device=dev)
    for s in ((6, 8), (6, 8, 3), (2, 6, 8, 4), (1, 6, 8, 1)):
        one("resize/%s" % "x".join(map(str, s)), rz.resize, z(s), DS)
    one("resize/out", rz.resize, z((2, 6, 8, 3)), DS, out=z((2, 4, 6, 3)))
    one("resize/out_flat_2d", rz.resize, z((6, 8)), DS, out=z((24,)))
    one("resize/src_channel_slice", rz.resize, z((6, 8, 4))[..., :3], DS)
    one("resize/src_row_padded", rz.resize, z((6, 16, 3))[:, :8], DS)
    one("resized/3d", warp.warp_perspective_resized, z((6, 8, 3)), M1, DS, (4, 3))
    one("resized/2d_align_corners", warp.warp_perspective_resized, z((6, 8), F32), M1, DS, (4, 3), align_corners=True, flags=0, out=z((4, 6), F32))
    img = np.zeros((6, 8, 3), dtype=np.uint8)
    one("cv/plain", warp.warpPerspective, img, M1, DS)
    one("cv/gray_f32_border", warp.warpPerspective, np.zeros((6, 8), dtype=np.float32), M1, DS, flags=2, borderMode=1, borderValue=7)
    one("cv/border_value", warp.warpPerspective, img, M1.tolist(), DS, borderValue=(1, 2))
    one("cv/dst", warp.warpPerspective, img, M1, DS, dst=np.ones((4, 6, 3), dtype=np.uint8))
    one("cv/transparent", warp.warpPerspective, img, M1, DS, borderMode=T, zero=True)
    one("cv/transparent_canvas", warp.warpPerspective, img, M1, DS, dst=np.ones((4, 6, 3), dtype=np.uint8), borderMode=T)

    # ---- every raise, per caller
    src3, out3 = z((2, 6, 8, 3)), z((2, 4, 6, 3))
    inter = {  # the entries that take interleaved frames, as f(src, **kw)
        "wp": lambda s, **kw: wp(s, kw.pop("M", M1), DS, **kw),
        "lens": lambda s, **kw: lens(s, kw.pop("M", M1), DS, K33, DIST[5], **kw),
        "planar": lambda s, **kw: planar(s, kw.pop("M", M1), DS, **kw),
        "to12": lambda s, **kw: to12(s, kw.pop("M", M1), DS12, **kw),
        "resize": lambda s, **kw: rz.resize(s, DS, **kw),
    }
    for who, f in inter.items():
        one("raises/%s/src_numpy" % who, f, np.zeros((6, 8, 3), dtype=np.uint8))
        one("raises/%s/src_cpu" % who, f, z((6, 8, 3), device=cpu))
        one("raises/%s/src_int32" % who, f, z((6, 8, 3), torch.int32))
        one("raises/%s/src_f16_bad_flag" % who, f, z((6, 8, 3), torch.float16), **({"interpolation": 0} if who == "resize" else {"flags": 3}))  # (the order of the two)
        one("raises/%s/src_5d" % who, f, z((1, 1, 6, 8, 3)))
        one("raises/%s/src_1d" % who, f, z((8,)))
        if who != "resize":
            one("raises/%s/flags_3" % who, f, None, flags=3)  # (judged before the tensor is looked at: wp looks at the tensor first)
            if who != "wp":  # (which has a bicubic kernel)
                one("raises/%s/flags_cubic" % who, f, src3, flags=2)
            one("raises/%s/three_matrices_for_two_frames" % who, f, src3, M=np.stack([M1] * 3))
        if who in ("wp", "planar", "to12"):
            one("raises/%s/minv_f32" % who, f, src3, M_inv_device=minv(2).float())
            one("raises/%s/minv_cpu" % who, f, src3, M_inv_device=minv(2).cpu())
            one("raises/%s/minv_numpy" % who, f, src3, M_inv_device=np.eye(3))
            one("raises/%s/minv_not_contiguous" % who, f, src3, M_inv_device=minv(2).transpose(1, 2))
            one("raises/%s/minv_2x9" % who, f, src3, M_inv_device=minv(2).reshape(2, 9))
            one("raises/%s/minv_flat_9" % who, f, src3, M_inv_device=minv(1).reshape(9))
            one("raises/%s/minv_three_for_two" % who, f, src3, M_inv_device=minv(3))
        if who in ("wp", "lens", "resize"):
            one("raises/%s/out_dtype" % who, f, src3, out=out3.float())
            one("raises/%s/out_numel" % who, f, src3, out=z((2, 4, 6, 4)))
            one("raises/%s/out_cpu" % who, f, src3, out=out3.cpu())
            one("raises/%s/out_numpy" % who, f, src3, out=np.zeros((2, 4, 6, 3), dtype=np.uint8))
            one("raises/%s/out_reshape_copies" % who, f, src3, out=z((2, 6, 4, 3)).transpose(1, 2))
            one("raises/%s/out_channel_slice" % who, f, src3, out=z((2, 4, 6, 4))[..., :3])
            one("raises/%s/out_column_step" % who, f, z((2, 6, 8, 1)), out=z((2, 4, 12, 1))[:, :, ::2])
    one("raises/wp/flags_3_after_the_tensor", wp, src3, M1, DS, flags=3)
    one("raises/wp/flags_7_inverse_map", wp, src3, M1, DS, flags=7 | 16, border_value=1)
    one("raises/wp/border_mode", wp, None, M1, DS, border_mode=6, flags=3)
    one("raises/wp/border_mode_str", wp, src3, M1, DS, border_mode="reflect")
    one("raises/wp/fast_path_arguments_fall_through", wp, src3, None, DS, out=np.zeros(3), M_inv_device=minv(2))
    one("raises/lens/dist_3_values", lens, None, M1, DS, None, [0.1, 0.2, 0.3], border_mode=9, flags=3)
    one("raises/lens/border_mode", lens, None, M1, DS, None, DIST[5], border_mode=1, flags=3)
    one("raises/lens/K_shape", lens, src3, M1, DS, np.eye(4), DIST[5])
    one("raises/lens/K_skew", lens, src3, M1, DS, K33 + np.array([[0, 0.5, 0], [0, 0, 0], [0, 0, 0]]), DIST[5])
    one("raises/lens/M_shape_inverse", lens, src3, np.eye(4), DS, K33, DIST[5], flags=17)
    one("raises/lens/M_shape", lens, src3, np.eye(4), DS, K33, DIST[5])
    one("raises/planar/out_dtype_unsupported", planar, None, M1, DS, out_dtype=torch.float64)
    one("raises/planar/out_of_another_dtype", planar, None, M1, DS, out=z((2, 3, 4, 6), torch.float16))
    one("raises/planar/out_numpy", planar, None, M1, DS, out=np.zeros(3))
    one("raises/planar/out_numel", planar, src3, M1, DS, out=z((2, 3, 4, 5), F32))
    one("raises/planar/out_cpu", planar, src3, M1, DS, out=z((2, 3, 4, 6), F32, cpu))
    one("raises/planar/out_reshape_copies", planar, src3, M1, DS, out=z((2, 3, 6, 4), F32).transpose(2, 3))
    one("raises/planar/out_column_step", planar, src3, M1, DS, out=z((2, 3, 4, 12), F32)[..., ::2])
    one("raises/to12/src_four_channels", to12, z((6, 8, 4)), M1, DS12)
    one("raises/to12/src_2d", to12, z((6, 8)), M1, DS12)
    one("raises/split_nv12/numpy", warp.split_nv12, np.zeros((12, 8), dtype=np.uint8))
    one("raises/split_nv12/f32", warp.split_nv12, z((12, 8), F32))
    one("raises/split_nv12/4d", warp.split_nv12, z((1, 1, 12, 8)))
    one("raises/split_nv12/rows", warp.split_nv12, z((10, 8)))
    one("raises/split_nv12/odd_width", warp.split_nv12, z((12, 7)))
    one("raises/split_nv12/column_step", warp.split_nv12, z((12, 16))[:, ::2])
    y2, uv2 = z((2, 8, 8)), z((2, 4, 4, 2))
    from12 = {"nv12": lambda y, uv, **kw: nv12(y, uv, kw.pop("M", M1), DS12, **kw), "nv12p": lambda y, uv, **kw: nv12p(y, uv, kw.pop("M", M1), DS12, **kw),
              "n2n": lambda y, uv, **kw: n2n(y, uv, kw.pop("M", M1), DS12, **kw)}
    for who, f in from12.items():
        one("raises/%s/flags_3" % who, f, None, None, flags=3)
        one("raises/%s/flags_cubic" % who, f, y2, uv2, flags=2)
        one("raises/%s/y_numpy" % who, f, np.zeros((8, 8), dtype=np.uint8), uv2)
        one("raises/%s/y_cpu" % who, f, y2.cpu(), uv2)
        one("raises/%s/uv_f32" % who, f, y2, uv2.float())
        one("raises/%s/uv_none" % who, f, y2, None)
        one("raises/%s/y_4d" % who, f, y2[None], uv2[None])
        one("raises/%s/uv_of_another_rank" % who, f, y2, uv2[0])
        one("raises/%s/odd_height" % who, f, z((2, 7, 8)), uv2)
        one("raises/%s/odd_width" % who, f, z((2, 8, 7)), uv2)
        one("raises/%s/uv_shape" % who, f, y2, z((2, 4, 8, 2)))
        one("raises/%s/uv_batch" % who, f, y2, z((1, 4, 4, 2)))
        one("raises/%s/y_column_step" % who, f, z((2, 8, 16))[..., ::2], uv2)
        one("raises/%s/uv_pair_step" % who, f, y2, z((2, 4, 4, 4))[..., ::2])
        one("raises/%s/uv_column_step" % who, f, y2, z((2, 4, 8, 2))[:, :, ::2])
        one("raises/%s/three_matrices_for_two_frames" % who, f, y2, uv2, M=np.stack([M1] * 3))
        one("raises/%s/minv_f32" % who, f, y2, uv2, M_inv_device=minv(2).float())
        one("raises/%s/minv_2x9" % who, f, y2, uv2, M_inv_device=minv(2).reshape(2, 9))
        one("raises/%s/minv_three_for_two" % who, f, y2, uv2, M_inv_device=minv(3))
    one("raises/nv12/out_dtype", nv12, y2, uv2, M1, DS12, out=z((2, 6, 4, 3), F32))
    one("raises/nv12/out_numel", nv12, y2, uv2, M1, DS12, out=z((2, 6, 4, 4)))
    one("raises/nv12/out_reshape_copies", nv12, y2, uv2, M1, DS12, out=z((2, 4, 6, 3)).transpose(1, 2))
    one("raises/nv12/out_channel_slice", nv12, y2, uv2, M1, DS12, out=z((2, 6, 4, 4))[..., :3])
    one("raises/nv12p/out_dtype_unsupported", nv12p, None, None, M1, DS12, out_dtype=torch.uint8)
    one("raises/nv12p/out_of_another_dtype", nv12p, None, None, M1, DS12, out=z((2, 3, 6, 4), F32), out_dtype=torch.float16)
    one("raises/nv12p/out_numel", nv12p, y2, uv2, M1, DS12, out=z((2, 3, 6, 5), F32))
    one("raises/nv12p/out_column_step", nv12p, y2, uv2, M1, DS12, out=z((2, 3, 6, 8), F32)[..., ::2])
    into12 = {"to12": lambda dsize=DS12, **kw: to12(src3, M1, dsize, **kw), "n2n": lambda dsize=DS12, **kw: n2n(y2, uv2, M1, dsize, **kw)}
    one("raises/to12/dsize_before_src", to12, None, M1, (5, 6))
    one("raises/n2n/dsize_before_planes", n2n, None, None, M1, (5, 6))
    for who, f in into12.items():
        one("raises/%s/dsize_odd_width" % who, f, dsize=(5, 6))
        one("raises/%s/dsize_odd_height" % who, f, dsize=(4, 3))
        one("raises/%s/dsize_zero" % who, f, dsize=(0, 6))
        one("raises/%s/flags_before_dsize" % who, f, dsize=(5, 6), flags=2)
        one("raises/%s/out_triple" % who, f, out=(z((2, 6, 4)), z((2, 3, 2, 2)), None))
        one("raises/%s/out_joined_numpy" % who, f, out=np.zeros((2, 9, 4), dtype=np.uint8))
        one("raises/%s/out_joined_f32" % who, f, out=z((2, 9, 4), F32))
        one("raises/%s/out_joined_4d" % who, f, out=z((1, 2, 9, 4)))
        one("raises/%s/out_joined_shape" % who, f, out=z((2, 6, 4)))
        one("raises/%s/out_joined_cpu" % who, f, out=z((2, 9, 4), device=cpu))
        one("raises/%s/out_joined_batch" % who, f, out=z((3, 9, 4)))
        one("raises/%s/out_joined_column_step" % who, f, out=z((2, 9, 8))[..., ::2])
        one("raises/%s/out_uv_f32" % who, f, out=(z((2, 6, 4)), z((2, 3, 2, 2), F32)))
        one("raises/%s/out_y_numpy" % who, f, out=(np.zeros((2, 6, 4), dtype=np.uint8), z((2, 3, 2, 2))))
        one("raises/%s/out_uv_cpu" % who, f, out=(z((2, 6, 4)), z((2, 3, 2, 2), device=cpu)))
        one("raises/%s/out_y_4d" % who, f, out=(z((1, 2, 6, 4)), z((1, 2, 3, 2, 2))))
        one("raises/%s/out_uv_of_another_rank" % who, f, out=(z((2, 6, 4)), z((3, 2, 2))))
        one("raises/%s/out_y_shape" % who, f, out=(z((2, 6, 6)), z((2, 3, 2, 2))))
        one("raises/%s/out_uv_shape" % who, f, out=(z((2, 6, 4)), z((2, 3, 4, 2))))
        one("raises/%s/out_y_column_step" % who, f, out=(z((2, 6, 8))[..., ::2], z((2, 3, 2, 2))))
        one("raises/%s/out_uv_pair_step" % who, f, out=(z((2, 6, 4)), z((2, 3, 2, 4))[..., ::2]))
    one("raises/resize/interpolation", rz.resize, z((6, 8, 3)), DS, interpolation=0)
    one("raises/resize/five_channels", rz.resize, z((6, 8, 5))[::1, ::2], DS)
    one("raises/resize/dsize_zero", rz.resize, z((6, 8, 3)), (0, 4))
    one("raises/resize/dsize_negative", rz.resize, z((6, 8, 3)), (6, -4), out=z((3,)))
    one("raises/cv/border_mode", warp.warpPerspective, None, M1, DS, borderMode=7)
    one("raises/cv/dtype", warp.warpPerspective, np.zeros((6, 8, 3), dtype=np.int16), M1, DS)
    one("raises/cv/canvas_shape", warp.warpPerspective, img, M1, DS, dst=np.zeros((4, 6), dtype=np.uint8), borderMode=T)
    one("raises/cv/canvas_dtype", warp.warpPerspective, img, M1, DS, dst=np.zeros((4, 6, 3), dtype=np.float32), borderMode=T)
    one("raises/cv/canvas_list", warp.warpPerspective, img, M1, DS, dst=[[0]], borderMode=T)


def record_all(device="cuda:0"):
    """{case id: [one record per call]} of every case, recorded through the stub on a stream of its own (so that the stream handle is
    no null pointer and is told apart from a zero).  Restores the library and empties the caches the calls filled."""
    device = torch.device(device)
    real = _lib.load()
    stub = StubLibrary(real)
    stream = torch.cuda.Stream(device)
    r = Recorder(device, stub, stream.cuda_stream)
    try:
        _lib._lib = stub
        with torch.cuda.device(device), torch.cuda.stream(stream):
            _cases(r)
    finally:
        _lib._lib = real
        warp._plans.clear()
        warp._class_tables.clear()
        warp._minv_cache.clear()
    torch.cuda.synchronize(device)
    return r.cases


def first_difference(got, want, path=""):
    """Where two records part, as text ('' if they are equal): the first argument that differs is named."""
    if type(got) is not type(want):
        return "%s: %r != %r" % (path, got, want)
    if isinstance(want, dict):
        for k in sorted(set(got) | set(want)):
            if k not in got or k not in want:
                return "%s.%s: %s" % (path, k, "missing" if k not in got else "unexpected")
            d = first_difference(got[k], want[k], "%s.%s" % (path, k))
            if d:
                return d
        return ""
    if isinstance(want, list):
        if len(got) != len(want):
            return "%s: %d entries != %d: %r != %r" % (path, len(got), len(want), got, want)
        for k, (g, w) in enumerate(zip(got, want)):
            d = first_difference(g, w, "%s[%d]" % (path, k))
            if d:
                return d
        return ""
    if got != want and not (isinstance(want, float) and got != got and want != want):
        return "%s: %r != %r" % (path, got, want)
    return ""
