"""Straight-alpha (RGBA / LA) resizing without a GPU: the Pillow-made fixture, the premultiply / un-premultiply arithmetic the kernels
use, argument checks of the Python surface and the C-ABI."""
import ctypes

import numpy as np
import pytest
import torch

import kit_golden

M = kit_golden.generator("alpha")


@pytest.fixture(scope="module")
def fx():
    return kit_golden.fixture("alpha")


def test_fixture_inputs_regenerate(fx):
    for case, (h, w), (oh, ow), chans, seed in M.CASES:
        for c in chans:
            img = M.make_image(h, w, c, seed)
            assert M.crc(img) == M.expected(fx, case, c, "linear")[0], (case, c)
            a = img[:, :, -1]
            assert (a == 0).mean() > 0.2 and (a == 255).mean() > 0.2, (case, c)  # large transparent and opaque areas
            for name in M.FILTERS:
                _, _, samples = M.expected(fx, case, c, name)
                assert samples.shape == (len(M.sample_pixels(oh, ow)), c)
    assert fx["crcs"].shape == (sum(len(ch) for *_, ch, _ in M.CASES), 1 + len(M.FILTERS))


def test_formulas_equal_pillow_tables(fx):
    c, a = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    assert np.array_equal(M.premul_formula(c, a), fx["premul"])
    assert np.array_equal(M.unpremul_formula(c, a), fx["unpremul"])
    # truncating division is what Pillow does: rounding, or zeroing colour where alpha is 0, both differ
    rounded = np.where((a == 0) | (a == 255), c, np.minimum(255, (255 * c + np.maximum(a, 1) // 2) // np.maximum(a, 1)))
    assert not np.array_equal(rounded, fx["unpremul"])
    assert not np.array_equal(np.where(a == 0, 0, fx["unpremul"]), fx["unpremul"])


def _f32_ulps(x: np.float32, k: int) -> np.float32:
    return np.int32(np.float32(x).view(np.int32) + k).view(np.float32)


def _device_unpremul(c: int, a: int, rcp: np.float32) -> int:
    """aa_unpremul8 (aa_alpha.h) step by step in the same float32 / int32 arithmetic, with `rcp` standing for v_rcp_f32(a)."""
    if a == 0 or a == 255:
        return c
    if c >= a:
        return 255
    n = 255 * c
    q = int(np.float32(np.float32(n) * rcp))  # v_mul_f32 then v_cvt_u32_f32 (truncates)
    r = n - q * a
    q += (1 if r >= a else 0) - (1 if r < 0 else 0)
    return q


def test_device_division_helper_exhaustive(fx):
    """Every (c, a) pair, with the reciprocal anywhere within 2 ulp of 1/a (v_rcp_f32 is within 1): the corrected quotient is exact."""
    table = fx["unpremul"]
    for a in range(256):
        r0 = np.float32(1.0) / np.float32(max(a, 1))
        for k in (-2, -1, 0, 1, 2):
            rcp = _f32_ulps(r0, k)
            got = [_device_unpremul(c, a, rcp) for c in range(256)]
            assert got == table[:, a].tolist(), (a, k)


def test_alpha_argument_errors_without_gpu():
    from interpolate_antialiasing_amd import extension_interpolate as ext
    from interpolate_antialiasing_amd import functional

    x8 = torch.zeros((1, 4, 8, 8), dtype=torch.uint8)
    for fn in (ext.linear_forward, ext.cubic_forward, ext.nearest_forward, ext.lanczos_forward, ext.hamming_forward):
        with pytest.raises(ValueError, match="alpha"):
            fn(torch.zeros((1, 4, 8, 8)), [4, 4], alpha=True)
        with pytest.raises(ValueError, match="alpha"):
            fn(x8, [4, 4], alpha=True, uint8_mode="harness")
        with pytest.raises(ValueError, match="alpha"):
            fn(x8, [4, 4], alpha=True, out_dtype=torch.float32)
        for c in (1, 3, 5):
            with pytest.raises(ValueError, match="alpha"):
                fn(torch.zeros((1, c, 8, 8), dtype=torch.uint8), [4, 4], alpha=True)
        with pytest.raises(TypeError):
            fn(x8, [4, 4], False, True)  # keyword-only
    with pytest.raises(ValueError, match="alpha"):
        functional.interpolate_aa(torch.zeros((1, 3, 8, 8), dtype=torch.uint8), (4, 4), alpha=True)


def test_c_abi_flag_checks_without_gpu():
    from interpolate_antialiasing_amd import _lib

    L = _lib.load()
    assert _lib.FLAG_PREMUL_ALPHA == 2
    assert "aa_workspace_bytes_ex" in _lib.EXPORTS and hasattr(L, "aa_workspace_bytes_ex")
    assert L.aa_abi_version() == 3
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: the flag is checked before the axes and pointers are used
    ah = _lib.Axis(table_dev=fake.value, in_size=8, out_size=4, ksize=5, kind=_lib.TABLE_F32)
    aw = _lib.Axis(table_dev=fake.value, in_size=8, out_size=4, ksize=5, kind=_lib.TABLE_F32)
    for dtype, c, kind in ((_lib.F32, 4, _lib.TABLE_F32), (_lib.U8, 3, _lib.TABLE_PIL), (_lib.U8, 4, _lib.TABLE_F32),
                           (_lib.U8, 1, _lib.TABLE_PIL)):
        ah.kind = aw.kind = kind
        for layout in (_lib.NCHW, _lib.NHWC):
            rc = L.aa_resample_fwd_ex(fake, fake, None, 0, dtype, layout, 1, c, 8, 8, ctypes.byref(ah), ctypes.byref(aw),
                                      _lib.FLAG_PREMUL_ALPHA, None)
            assert rc == _lib.ERR_BAD_DTYPE, (dtype, c, kind, layout, rc)
            strides = (ctypes.c_int64 * 4)(c * 64, 1, 8 * c, c) if layout == _lib.NHWC else (ctypes.c_int64 * 4)(c * 64, 64, 8, 1)
            rc = L.aa_resample_fwd_strided(fake, fake, dtype, layout, 1, c, 8, 8, strides, ctypes.byref(ah), ctypes.byref(aw),
                                           _lib.FLAG_PREMUL_ALPHA, None)
            assert rc == _lib.ERR_BAD_DTYPE, (dtype, c, kind, layout, rc)
    assert L.aa_resample_fwd_ex(fake, fake, None, 0, _lib.U8, _lib.NHWC, 1, 4, 8, 8, ctypes.byref(ah), ctypes.byref(aw), 4, None) != 0
