"""One warp_perspective call in each of its two launch modes, for the GPU parity tests (a plain module, imported by them).

table  the matrices come from device_inverse (what every call that passes `M` gets): the call fills or finds a per-tile verdict table
       and launches bevwarp_warp_classes reading it.  Checked: the call launched that entry point in USE mode, and afterwards the
       table cache holds an entry for this very matrix tensor and geometry -- unless the library keeps no table for the geometry,
       in which case it must have launched bevwarp_warp.
plain  the caller owns the matrices (a clone): bevwarp_warp, every tile classifies itself in the kernel -- what bench.py times.
       Checked: the call launched bevwarp_warp and nothing else, and no table was created for the matrices.

Both share one kernel binary; what differs is where a tile's set-up runs, so each mode's result is compared with the oracle."""
import contextlib

import numpy as np
import pytest
import torch

from bev_amd import _lib, warp as W

MODES = ("table", "plain")
COMPARED = {m: 0 for m in MODES}  # oracle comparisons run per mode in this process (reported per module: report_comparisons)
_WARPS = ("bevwarp_warp", "bevwarp_warp_classes")


def poisoned_out(t, dsize):
    """A destination for warping `t` to `dsize`, filled with 77: pixels a launch leaves unwritten do not pass as zeros."""
    dw, dh = int(dsize[0]), int(dsize[1])
    shape = (dh, dw) if t.dim() == 2 else tuple(t.shape[:-3]) + (dh, dw, t.shape[-1])
    return torch.full(shape, 77, dtype=t.dtype, device=t.device)


class _Recording:
    """Stands in for the loaded library while one call runs: the warp entry points log (name, classes mode or None)."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in _WARPS:
            return fn
        log = self._log

        def call(*args):
            log.append((name, args[-2] if name == "bevwarp_warp_classes" else None))
            return fn(*args)
        return call


@contextlib.contextmanager
def _launches():
    log = []
    load = _lib.load
    proxy = _Recording(load(), log)
    _lib.load = lambda: proxy
    try:
        yield log
    finally:
        _lib.load = load


def _geometry(src, dsize, flags):
    s4 = src if src.dim() == 4 else (src[None] if src.dim() == 3 else src[None, :, :, None])
    B, H, Wd, C = s4.shape
    return B, H, Wd, int(dsize[1]), int(dsize[0]), C, W._DTYPES[src.dtype], int(flags) & 7


def _table_for(minv, geom):
    n_m = minv.numel() // 9
    return any(k[0] == minv.data_ptr() and k[1] == n_m and k[2:] == geom and v[1] is minv for k, v in W._class_tables.items())


def warp_modes(src, M, dsize, flags=W.INTER_LINEAR, border_value=None, out=None):
    """{"table": result, "plain": result} as host arrays.  `src` a CUDA tensor; `out`, if given, is written by both calls: its
    contents before the first call (a poison fill, say) are put back before the second, so pixels a mode leaves unwritten still show."""
    dev = src.device
    geom = _geometry(src, dsize, flags)
    inverse_given = bool(int(flags) & W.WARP_INVERSE_MAP)
    keep = None if out is None else out.clone()
    res = {}
    for mode in MODES:
        if out is not None and mode != MODES[0]:
            out.copy_(keep)
        if mode == "table":
            minv = W.device_inverse(M, dev, inverse_given=inverse_given)  # (the tensor the call below looks up)
            with _launches() as log:
                got = W.warp_perspective(src, M, dsize, flags=flags, border_value=border_value, out=out)
            torch.cuda.synchronize()
            if _lib.load().bevwarp_tile_classes_bytes(*geom) > 0:
                assert log in ([("bevwarp_warp_classes", 1), ("bevwarp_warp_classes", 0)], [("bevwarp_warp_classes", 0)]), \
                    "table mode: the call did not launch with a verdict table: %s" % log  # ((fill, then) a launch reading the table)
                assert _table_for(minv, geom), "table mode: no verdict table was kept for these matrices and this geometry"
            else:
                assert log == [("bevwarp_warp", None)], log
        else:
            before = dict(W._class_tables)
            mine = W.device_inverse(M, dev, inverse_given=inverse_given).clone()
            for k in [k for k in W._plans if len(k) > 2 and k[2] == mine.data_ptr()]:
                del W._plans[k]  # (a plan left at a recycled address would launch unseen by the log below)
            with _launches() as log:
                got = W.warp_perspective(src, None, dsize, flags=flags, border_value=border_value, out=out, M_inv_device=mine)
            torch.cuda.synchronize()
            assert log == [("bevwarp_warp", None)], "plain mode: the call launched %s" % log
            assert W._class_tables.keys() == before.keys() and not any(v[1] is mine for v in W._class_tables.values()), \
                "plain mode: a verdict table was created for matrices the caller owns"
        if out is not None:
            assert got is out
        res[mode] = got.cpu().numpy()
    return res


def check_modes(res, exp, cmp=np.testing.assert_array_equal):
    """cmp(result, exp) for each mode's result; the failure names the mode."""
    for mode, got in res.items():
        try:
            cmp(got, exp)
        except AssertionError as e:
            raise AssertionError("%s mode: %s" % (mode, e)) from None
        COMPARED[mode] += 1


@pytest.fixture(scope="module", autouse=True)
def report_comparisons(request):
    """Import into a test module: at its end, writes how many oracle comparisons ran in each launch mode and asserts they are equal."""
    start = dict(COMPARED)
    yield
    n = {m: COMPARED[m] - start[m] for m in MODES}
    tr, cap = (request.config.pluginmanager.get_plugin(name) for name in ("terminalreporter", "capturemanager"))
    if tr is not None:
        with cap.global_and_fixture_disabled() if cap is not None else contextlib.nullcontext():
            tr.write_line("%s: oracle comparisons per launch mode %s" % (request.module.__name__, n))
    assert n["table"] == n["plain"], n
