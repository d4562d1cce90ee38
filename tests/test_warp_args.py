"""Host-side argument validation of bev_amd.warp (no GPU): everything that reaches the kernel as a raw address or a
raw element size is checked first."""
import numpy as np
import pytest
import torch

from bev_amd import warp


def test_out_tensor_must_match_dtype_device_and_size():
    cpu = torch.device("cpu")
    ok = torch.empty((2, 8, 8, 3), dtype=torch.float32)
    warp._check_out(ok, torch.float32, cpu, 2 * 8 * 8 * 3)
    with pytest.raises(ValueError):  # a uint8 `out` for a float32 source would be overrun 4x
        warp._check_out(torch.empty((2, 8, 8, 3), dtype=torch.uint8), torch.float32, cpu, 2 * 8 * 8 * 3)
    with pytest.raises(ValueError):
        warp._check_out(ok, torch.float32, cpu, 2 * 8 * 8 * 3 + 1)
    with pytest.raises(ValueError):  # another device (a host pointer must never reach the kernel)
        warp._check_out(ok, torch.float32, torch.device("cuda", 0), 2 * 8 * 8 * 3)
    with pytest.raises(ValueError):
        warp._check_out(np.zeros(4), torch.float32, cpu, 4)


def test_matrix_tensor_must_be_contiguous_float64_3x3_on_the_device():
    cpu = torch.device("cpu")
    m = torch.eye(3, dtype=torch.float64).repeat(4, 1, 1)
    assert warp._check_minv(m, cpu, 4) == 4
    assert warp._check_minv(m[:1], cpu, 4) == 1
    with pytest.raises(ValueError):
        warp._check_minv(m.float(), cpu, 4)
    with pytest.raises(ValueError):
        warp._check_minv(m.transpose(1, 2), cpu, 4)  # not contiguous
    with pytest.raises(ValueError):
        warp._check_minv(m.reshape(4, 9), cpu, 4)
    with pytest.raises(ValueError):
        warp._check_minv(m[:3], cpu, 4)  # 3 matrices for 4 frames
    with pytest.raises(ValueError):
        warp._check_minv(m, torch.device("cuda", 0), 4)
    with pytest.raises(ValueError):
        warp._check_minv(m.numpy(), cpu, 4)


def test_interpolation_flags_per_caller():
    assert [warp._interp("", f, cubic=True) for f in (0, 1, 2)] == [warp.INTER_NEAREST, warp.INTER_LINEAR, warp.INTER_CUBIC]
    assert warp._interp("", 2 | warp.WARP_INVERSE_MAP | 32 | 1024, cubic=True) == warp.INTER_CUBIC  # bits above 7 are someone else's
    assert warp._interp("warp_to_planar", 1 | warp.WARP_INVERSE_MAP | 8) == warp.INTER_LINEAR
    for bad in (3, 4, 7, 3 | warp.WARP_INVERSE_MAP):
        with pytest.raises(ValueError) as e:
            warp._interp("", bad, cubic=True)
        assert str(e.value) == "unsupported interpolation flag %d (INTER_NEAREST, INTER_LINEAR, INTER_CUBIC)" % (bad & 7)
    for who in ("warp_perspective_lens", "warp_to_planar", "warp_nv12_to_planar", "warp_perspective_nv12", "warp_perspective_to_nv12", "warp_nv12_to_nv12"):
        assert [warp._interp(who, f) for f in (0, 1, 16, 17)] == [0, 1, 0, 1]
        for bad in (2, 3, 7, 2 | warp.WARP_INVERSE_MAP):  # no bicubic kernel behind these entries
            with pytest.raises(ValueError) as e:
                warp._interp(who, bad)
            assert str(e.value) == "unsupported interpolation flag %d (%s: INTER_NEAREST, INTER_LINEAR)" % (bad & 7, who)


def test_pixel_destination_is_new_or_the_callers_out_as_it_is():
    cpu, f32 = torch.device("cpu"), torch.float32
    new = warp._pixel_dst(None, torch.uint8, cpu, 2, 4, 6, 3)
    assert new.shape == (2, 4, 6, 3) and new.dtype == torch.uint8 and new.is_contiguous()
    zeroed = warp._pixel_dst(None, f32, cpu, 2, 4, 6, 3, zeroed=True)
    assert zeroed.shape == (2, 4, 6, 3) and zeroed.dtype == f32 and not zeroed.any()
    for out in (torch.empty((2, 4, 6, 3)), torch.empty(2 * 4 * 6 * 3), torch.empty((8, 6, 3))):  # the shape, or any view reshape need not copy
        d4 = warp._pixel_dst(out, f32, cpu, 2, 4, 6, 3)
        assert d4.data_ptr() == out.data_ptr() and d4.shape == (2, 4, 6, 3) and d4.stride() == (72, 18, 3, 1)
    padded = torch.empty((2, 4, 8, 3))[:, :, :6]  # padded rows: taken as they are, the row stride is passed on
    d4 = warp._pixel_dst(padded, f32, cpu, 2, 4, 6, 3)
    assert d4.data_ptr() == padded.data_ptr() and d4.stride() == (96, 24, 3, 1)
    for bad in (torch.empty((2, 4, 6, 3), dtype=torch.uint8),  # would be overrun 4x
                torch.empty((2, 4, 6, 4)), torch.empty((2, 4, 6, 3), device="meta"), np.zeros((2, 4, 6, 3), dtype=np.float32)):
        with pytest.raises(ValueError) as e:
            warp._pixel_dst(bad, f32, cpu, 2, 4, 6, 3)
        assert str(e.value) == "out must be a torch.float32 tensor of 144 elements on cpu"
    with pytest.raises(ValueError):
        warp._pixel_dst(torch.empty((2, 4, 6, 3)), f32, torch.device("cuda", 0), 2, 4, 6, 3)
    for bad in (torch.empty((2, 6, 4, 3)).transpose(1, 2),   # reshape would copy: the kernel would write a temporary
                torch.empty((2, 4, 6, 4))[..., :3],          # pixels not packed
                torch.empty((2, 4, 12, 3))[:, :, ::2]):      # every other pixel
        with pytest.raises(ValueError) as e:
            warp._pixel_dst(bad, f32, cpu, 2, 4, 6, 3)
        assert str(e.value) == "out must be a contiguous-row channels-last tensor"


def test_result_is_shaped_like_the_source():
    d4 = torch.arange(2 * 4 * 6 * 3).reshape(2, 4, 6, 3)
    one = d4[:1, :, :, :1]
    got = warp._like_src(one, 2, None)
    assert got.shape == (4, 6) and got.data_ptr() == one.data_ptr()
    got = warp._like_src(d4[:1], 3, None)
    assert got.shape == (4, 6, 3) and got.data_ptr() == d4.data_ptr()
    assert warp._like_src(d4, 4, None) is d4
    out = torch.empty(144)
    for ndim in (2, 3, 4):
        assert warp._like_src(d4, ndim, out) is out  # a given `out` comes back as it was given, whatever its shape


def test_frames_are_lifted_to_four_dimensions_and_copied_only_when_rows_are_not_channels_last():
    for shape, want in (((6, 8), (1, 6, 8, 1)), ((6, 8, 3), (1, 6, 8, 3)), ((2, 6, 8, 3), (2, 6, 8, 3))):
        src = torch.zeros(shape, dtype=torch.uint8)
        s4, copied = warp._frames("f", src, None)
        assert s4.shape == want and not copied and s4.data_ptr() == src.data_ptr()
    padded = torch.zeros((2, 6, 16, 3))[:, :, 2:10]  # padded rows are passed through
    s4, copied = warp._frames("f", padded, None)
    assert not copied and s4.data_ptr() == padded.data_ptr() and s4.stride() == (288, 48, 3, 1)
    for src in (torch.zeros((6, 8, 4))[..., :3], torch.zeros((6, 16, 3))[:, ::2], torch.zeros((8, 6)).t()):
        s4, copied = warp._frames("f", src, None)
        assert copied and s4.is_contiguous() and s4.data_ptr() != src.data_ptr()
    for bad in (torch.zeros(8), torch.zeros((1, 1, 6, 8, 3))):
        with pytest.raises(ValueError) as e:
            warp._frames("f", bad, None)
        assert str(e.value) == "src must be (B,H,W,C), (H,W,C) or (H,W)"
    for bad in (np.zeros((6, 8, 3), dtype=np.uint8), torch.zeros((6, 8, 3), dtype=torch.uint8), torch.zeros((6, 8, 3), dtype=torch.int32)):
        with pytest.raises(ValueError) as e:  # not a tensor, not on the GPU, not a type the kernels read
            warp._frames("warp_to_planar", bad, warp._DTYPES)
        assert str(e.value) == "warp_to_planar needs a uint8 or float32 CUDA (HIP) tensor"
    for bad in (torch.zeros((6, 8)), torch.zeros((6, 8, 4)), torch.zeros((1, 2, 6, 8, 3))):
        with pytest.raises(ValueError) as e:
            warp._frames("f", bad, None, channels=3)
        assert str(e.value) == "src must be (B, H, W, 3) or (H, W, 3)"
    assert warp._frames("f", torch.zeros((6, 8, 3)), None, channels=3)[0].shape == (1, 6, 8, 3)


def test_matrices_are_the_callers_or_the_cached_inverse():
    cpu = torch.device("cpu")
    warp._minv_cache.clear()
    mine = torch.eye(3, dtype=torch.float64).repeat(2, 1, 1)
    t, n_m = warp._matrices(None, warp.INTER_LINEAR, mine, cpu, 2)
    assert t is mine and n_m == 2 and not warp._minv_cache
    M = np.array([[2.0, 0, 1], [0, 4.0, -1], [0, 0, 1]])
    t, n_m = warp._matrices(M, warp.INTER_LINEAR, None, cpu, 4)
    assert n_m == 1 and t is warp.device_inverse(M, cpu)
    np.testing.assert_allclose(t.numpy()[0], np.linalg.inv(M), rtol=1e-15)
    t, n_m = warp._matrices(np.stack([M, M]), warp.INTER_LINEAR | warp.WARP_INVERSE_MAP, None, cpu, 2)
    assert n_m == 2
    np.testing.assert_array_equal(t.numpy(), np.stack([M, M]))
    with pytest.raises(ValueError):
        warp._matrices(np.stack([M] * 3), warp.INTER_LINEAR, None, cpu, 2)  # 3 matrices for 2 frames
    with pytest.raises(ValueError):
        warp._matrices(None, warp.INTER_LINEAR, mine.float(), cpu, 2)
    warp._minv_cache.clear()


def test_host_arrays_go_to_the_abi_as_pointers():
    import ctypes
    assert warp._ptr(None) is None
    a = np.array([1.0, 2.0, 3.0])
    p = warp._ptr(a)
    assert isinstance(p, ctypes.c_void_p) and p.value == a.ctypes.data


def test_scalar_border_follows_cv_scalar():
    np.testing.assert_array_equal(warp.scalar_border(7, 3), [7, 0, 0])          # cv::Scalar(7) = (7, 0, 0, 0)
    np.testing.assert_array_equal(warp.scalar_border((1, 2), 3), [1, 2, 0])     # shorter than C: the rest stay 0
    np.testing.assert_array_equal(warp.scalar_border((1, 2, 3, 4), 3), [1, 2, 3])
    np.testing.assert_array_equal(warp.scalar_border(0, 1), [0])
    np.testing.assert_array_equal(warp.scalar_border([5], 4), [5, 0, 0, 0])


def test_matrix_cache_is_a_bounded_lru_that_keeps_recent_entries(monkeypatch):
    monkeypatch.setattr(warp, "_MINV_CACHE_MAX", 4)
    warp._minv_cache.clear()
    mats = [np.eye(3) + np.diag([k, 0, 0]) for k in range(1, 8)]
    first = warp.device_inverse(mats[0], "cpu")
    for m in mats[1:4]:
        warp.device_inverse(m, "cpu")
    assert warp.device_inverse(mats[0], "cpu") is first          # hit: same tensor, now most recently used
    warp.device_inverse(mats[4], "cpu")                          # evicts mats[1], the least recently used
    assert len(warp._minv_cache) == 4
    assert warp.device_inverse(mats[0], "cpu") is first
    again = warp.device_inverse(mats[1], "cpu")
    np.testing.assert_allclose(again.numpy()[0], np.linalg.inv(mats[1]), rtol=1e-15)
    warp._minv_cache.clear()


def test_tracker_out_dict_is_validated_before_its_addresses_reach_the_kernel():
    from bev_amd import tracker_geom as tg
    cpu = torch.device("cpu")

    def mk(n, m, dt=torch.float64, img=True):
        d = {"dets_world": torch.empty((n, 5), dtype=dt), "iou": torch.empty((n, m), dtype=dt), "candidates": torch.empty((n, m), dtype=torch.bool)}
        if img:
            d["dets_img"] = torch.empty((n, 2), dtype=dt)
        return d

    tg._check_out_dict(mk(4, 6), 4, 6, torch.float64, cpu, True)
    tg._check_out_dict(mk(4, 6, img=False), 4, 6, torch.float64, cpu, False)
    for bad in (mk(4, 5), mk(3, 6), mk(4, 6, torch.float32), mk(4, 6, img=False), None, {"dets_world": np.zeros((4, 5))}):
        with pytest.raises(ValueError):  # another n / m, another dtype, no dets_img although H_img_world is given, not a dict of tensors
            tg._check_out_dict(bad, 4, 6, torch.float64, cpu, True)
    d = mk(4, 6)
    d["iou"] = torch.empty((6, 4), dtype=torch.float64).t()  # right shape, not contiguous
    with pytest.raises(ValueError):
        tg._check_out_dict(d, 4, 6, torch.float64, cpu, True)
    d = mk(4, 6)
    d["candidates"] = torch.empty((4, 6), dtype=torch.uint8)
    with pytest.raises(ValueError):
        tg._check_out_dict(d, 4, 6, torch.float64, cpu, True)
    with pytest.raises(ValueError):
        tg._check_out_dict(mk(4, 6), 4, 6, torch.float64, torch.device("cuda", 0), True)


def test_bw_mode_needs_three_channels():
    from bev_amd import compo
    with pytest.raises(ValueError):
        compo.gray_bgr(torch.zeros((4, 4, 1), dtype=torch.uint8))
    g = compo.gray_bgr(torch.tensor([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 20, 30]]], dtype=torch.uint8))
    assert g[0, :, 0].tolist() == [29, 150, 76, (1868 * 10 + 9617 * 20 + 4899 * 30 + 8192) >> 14] and (g[..., 0] == g[..., 2]).all()
