"""float16 / bfloat16 output of the decode-adjacent forward without a GPU: the flag values, the C-ABI's flag checks (fake pointers, never
dereferenced) and the argument checks of the Python surface."""
import ctypes

import pytest
import torch


def _axes(_lib, kind):
    fake = 0x1000  # never dereferenced: the flags are checked before the tables and pointers are used
    ah = _lib.Axis(table_dev=fake, in_size=8, out_size=4, ksize=5, kind=kind)
    aw = _lib.Axis(table_dev=fake, in_size=8, out_size=4, ksize=5, kind=kind)
    return ctypes.c_void_p(fake), ah, aw


def test_flag_values_and_abi_version():
    from interpolate_antialiasing_amd import _lib

    assert _lib.FLAG_OUT_F16 == 4 and _lib.FLAG_OUT_BF16 == 8
    assert _lib.load().aa_abi_version() == 3
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    assert "#define AA_FLAG_OUT_F16 4u" in header and "#define AA_FLAG_OUT_BF16 8u" in header
    assert "#define AA_INTERP_ABI_VERSION 3" in header


def test_convert_flag_checks_without_gpu():
    from interpolate_antialiasing_amd import _lib

    L = _lib.load()
    fake, ah, aw = _axes(_lib, _lib.TABLE_F32)

    def call(flags, layout=_lib.NHWC):
        cv = _lib.Convert(out_layout=_lib.NCHW, normalize=0, flags=flags)
        return L.aa_resample_fwd_u8_to_f32(fake, fake, None, 0, layout, 1, 3, 8, 8, ctypes.byref(ah), ctypes.byref(aw), ctypes.byref(cv), None)

    both = _lib.FLAG_OUT_F16 | _lib.FLAG_OUT_BF16
    for layout in (_lib.NCHW, _lib.NHWC):
        assert call(both, layout) == _lib.ERR_BAD_DTYPE
        assert call(both | _lib.FLAG_FAST, layout) == _lib.ERR_BAD_DTYPE
        assert call(16, layout) != 0                       # an unknown bit
        assert call(16 | _lib.FLAG_OUT_BF16, layout) != 0
        assert call(_lib.FLAG_PREMUL_ALPHA, layout) != 0   # a flag of the other entry points
    assert L.aa_strerror(call(16)) == L.aa_strerror(-4)    # AA_ERR_BAD_SHAPE, as for every unknown bit


def test_other_entry_points_reject_the_bits():
    from interpolate_antialiasing_amd import _lib

    L = _lib.load()
    for kind, dtype in ((_lib.TABLE_F32, _lib.U8), (_lib.TABLE_PIL, _lib.U8), (_lib.TABLE_F32, _lib.F32)):
        fake, ah, aw = _axes(_lib, kind)
        for bit in (_lib.FLAG_OUT_F16, _lib.FLAG_OUT_BF16):
            for flags in (bit, bit | _lib.FLAG_FAST):
                rc = L.aa_resample_fwd_ex(fake, fake, None, 0, dtype, _lib.NHWC, 1, 3, 8, 8, ctypes.byref(ah), ctypes.byref(aw), flags, None)
                assert rc != 0, (kind, dtype, flags)
                strides = (ctypes.c_int64 * 4)(3 * 64, 1, 8 * 3, 3)
                rc = L.aa_resample_fwd_strided(fake, fake, dtype, _lib.NHWC, 1, 3, 8, 8, strides, ctypes.byref(ah), ctypes.byref(aw), flags, None)
                assert rc != 0, (kind, dtype, flags)


def test_python_argument_errors_without_gpu():
    from interpolate_antialiasing_amd import _lib
    from interpolate_antialiasing_amd import extension_interpolate as ext

    x3 = torch.zeros((1, 3, 8, 8), dtype=torch.uint8)
    x4 = torch.zeros((1, 4, 8, 8), dtype=torch.uint8)
    for fn in (ext.linear_forward, ext.cubic_forward, ext.nearest_forward, ext.lanczos_forward, ext.hamming_forward):
        for bad in (torch.float64, torch.int8, torch.uint8, torch.int32):
            with pytest.raises(NotImplementedError):
                fn(x3, [4, 4], out_dtype=bad)
        for dt in (torch.float16, torch.bfloat16):
            with pytest.raises(ValueError, match="alpha"):
                fn(x4, [4, 4], alpha=True, out_dtype=dt)
            with pytest.raises(NotImplementedError):      # float input: the fused conversion takes uint8
                fn(x3.float(), [4, 4], out_dtype=dt)
            with pytest.raises(NotImplementedError):      # Pillow's integers have no float output
                fn(x3, [4, 4], out_dtype=dt, uint8_mode="pil")
            with pytest.raises(_lib.AAInterpError):       # accepted by the argument checks: only the GPU is missing
                fn(x3, [4, 4], out_dtype=dt)
