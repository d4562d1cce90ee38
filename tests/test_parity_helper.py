"""tests/parity.py has teeth: a "table" call that kept no verdict table, or a "plain" call that made one, fails the helper's own mode
assertion.  No GPU: the warp entry is replaced by a stand-in that keeps (or fails to keep) tables the way bev_amd/warp.py does."""
import numpy as np
import pytest
import torch

from bev_amd import warp as W
from tests import parity as P


class _Lib:
    @staticmethod
    def bevwarp_tile_classes_bytes(B, H, Wd, dh, dw, C, dtype, interp):
        return 12 * B

    @staticmethod
    def bevwarp_warp(*args):
        return 0

    @staticmethod
    def bevwarp_warp_classes(*args):
        return 0


def _stand_in(monkeypatch, tables_for, launch_with_table=None):
    """device_inverse / warp_perspective on the CPU; `tables_for(minv)` says whether the call keeps a table for those matrices,
    `launch_with_table(minv)` (default: the same) whether it launches reading one."""
    launch_with_table = launch_with_table or tables_for
    cache = {}

    def device_inverse(M, device, inverse_given=False):
        key = np.asarray(M, dtype=np.float64).tobytes()
        if key not in cache:
            cache[key] = torch.from_numpy(np.linalg.inv(np.asarray(M, dtype=np.float64)).reshape(-1, 3, 3).copy())
            cache[key]._bevwarp_owned = True
        return cache[key]

    def warp_perspective(src, M, dsize, flags=1, border_value=None, out=None, M_inv_device=None):
        minv = device_inverse(M, src.device) if M_inv_device is None else M_inv_device
        B, H, Wd, dh, dw, C, dt, interp = P._geometry(src, dsize, flags)
        key = (minv.data_ptr(), minv.numel() // 9, B, H, Wd, dh, dw, C, dt, interp)
        if tables_for(minv) and key not in W._class_tables:
            W._lib.load().bevwarp_warp_classes(1, 0)
            W._class_tables[key] = (torch.zeros(3), minv, minv._version)
        if launch_with_table(minv):
            W._lib.load().bevwarp_warp_classes(0, 0)
        else:
            W._lib.load().bevwarp_warp(0)
        res = torch.zeros((dh, dw) + tuple(src.shape[2:]), dtype=src.dtype) if out is None else out
        res.fill_(5)
        return res

    monkeypatch.setattr(W, "device_inverse", device_inverse)
    monkeypatch.setattr(W, "warp_perspective", warp_perspective)
    monkeypatch.setattr(W, "_class_tables", type(W._class_tables)())
    monkeypatch.setattr(P._lib, "load", lambda: _Lib)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)


def _call():
    src = torch.zeros((20, 30, 3), dtype=torch.uint8)
    out = torch.full((8, 10, 3), 77, dtype=torch.uint8)
    return P.warp_modes(src, np.diag([2.0, 2.0, 1.0]), (10, 8), out=out)


def test_helper_accepts_calls_in_their_modes(monkeypatch):
    _stand_in(monkeypatch, lambda minv: getattr(minv, "_bevwarp_owned", False))
    res = _call()
    assert sorted(res) == sorted(P.MODES) and all((r == 5).all() for r in res.values())


def test_helper_refuses_a_table_call_without_a_table(monkeypatch):
    _stand_in(monkeypatch, lambda minv: False)  # as if _tile_classes returned None
    with pytest.raises(AssertionError, match="table mode"):
        _call()


def test_helper_refuses_a_table_call_that_launched_without_it(monkeypatch):
    _stand_in(monkeypatch, lambda minv: getattr(minv, "_bevwarp_owned", False), lambda minv: False)  # a table cached earlier, not read
    with pytest.raises(AssertionError, match="table mode"):
        _call()


def test_helper_refuses_a_plain_call_with_a_table(monkeypatch):
    _stand_in(monkeypatch, lambda minv: True)  # as if tables were kept for matrices the caller owns
    with pytest.raises(AssertionError, match="plain mode"):
        _call()


def test_check_modes_names_the_failing_mode():
    exp = np.zeros((2, 2), np.uint8)
    with pytest.raises(AssertionError, match="plain mode"):
        P.check_modes({"table": exp.copy(), "plain": exp + 1}, exp)
