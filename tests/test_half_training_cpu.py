"""float16 / bfloat16 gradients without a GPU: what the C-ABI's backward entry points answer before any GPU call (fake pointers, an
empty batch), and which error the Python surface raises for a CPU gradient: the library's "needs a GPU" for the dtypes the backward
takes, NotImplementedError for the atomic form in 16 bits and for every dtype it does not take, in the wording it always had."""
import ctypes

import pytest
import torch

HALVES = (torch.float16, torch.bfloat16)


def _axes(_lib, kind, h, oh, w, ow):
    """Transposed-table descriptors of a backward to (h, w) from gradients of (oh, ow); the pointers are never dereferenced."""
    fake = 0x1000
    trh = _lib.Axis(table_dev=fake, in_size=oh, out_size=h, ksize=3, kind=kind)
    trw = _lib.Axis(table_dev=fake, in_size=ow, out_size=w, ksize=3, kind=kind)
    return ctypes.c_void_p(fake), trh, trw


def test_c_abi_backward_takes_sixteen_bit_gradients():
    """aa_resample_bwd with AA_F16 / AA_BF16 and AA_TABLE_F32 axes, N = 0, both layouts: AA_OK (the empty batch is answered before any
    GPU call; the dtype check comes first and used to answer AA_ERR_BAD_DTYPE).  AA_TABLE_F64 axes, and the atomic form: still
    AA_ERR_BAD_DTYPE.  The ABI version stays 3: the change is additive."""
    from interpolate_antialiasing_amd import _lib

    L = _lib.load()
    assert L.aa_abi_version() == 3
    for dt in (_lib.F16, _lib.BF16):
        for layout in (_lib.NCHW, _lib.NHWC):
            fake, trh, trw = _axes(_lib, _lib.TABLE_F32, 8, 4, 8, 4)
            assert L.aa_resample_bwd(fake, fake, None, 0, dt, layout, 0, 3, 8, 8, ctypes.byref(trh), ctypes.byref(trw), None) == _lib.AA_OK
            fake, trh, trw = _axes(_lib, _lib.TABLE_F64, 8, 4, 8, 4)
            assert L.aa_resample_bwd(fake, fake, None, 0, dt, layout, 0, 3, 8, 8, ctypes.byref(trh), ctypes.byref(trw), None) == _lib.ERR_BAD_DTYPE
            # the atomic form reads the FORWARD tables (in_size = the input's)
            ah = _lib.Axis(table_dev=0x1000, in_size=8, out_size=4, ksize=5, kind=_lib.TABLE_F32)
            aw = _lib.Axis(table_dev=0x1000, in_size=8, out_size=4, ksize=5, kind=_lib.TABLE_F32)
            for n in (0, 1):
                assert L.aa_resample_bwd_atomic(fake, fake, fake, 1 << 20, dt, layout, n, 3, 8, 8, ctypes.byref(ah), ctypes.byref(aw),
                                                None) == _lib.ERR_BAD_DTYPE
    # what was there stays: fp32 with its tables is taken, uint8 gradients and mixed kinds are not
    fake, trh, trw = _axes(_lib, _lib.TABLE_F32, 8, 4, 8, 4)
    assert L.aa_resample_bwd(fake, fake, None, 0, _lib.F32, _lib.NCHW, 0, 3, 8, 8, ctypes.byref(trh), ctypes.byref(trw), None) == _lib.AA_OK
    assert L.aa_resample_bwd(fake, fake, None, 0, _lib.U8, _lib.NCHW, 0, 3, 8, 8, ctypes.byref(trh), ctypes.byref(trw), None) == _lib.ERR_BAD_DTYPE
    assert L.aa_resample_bwd(fake, fake, None, 0, 7, _lib.NCHW, 0, 3, 8, 8, ctypes.byref(trh), ctypes.byref(trw), None) == _lib.ERR_BAD_DTYPE


BWD_2D = ("linear_backward", "cubic_backward", "nearest_backward", "lanczos_backward", "hamming_backward")


@pytest.mark.parametrize("dt", HALVES)
def test_python_backward_takes_sixteen_bit_gradients(dt):
    """A CPU float16 / bfloat16 gradient gets as far as the device check: only the GPU is missing."""
    from interpolate_antialiasing_amd import _lib
    from interpolate_antialiasing_amd import extension_interpolate as aa

    g = torch.zeros(1, 2, 4, 5, dtype=dt)
    for name in BWD_2D:
        with pytest.raises(_lib.AAInterpError, match="expected a tensor on a ROCm GPU"):
            getattr(aa, name)(g, [4, 5], [1, 2, 9, 11])
        with pytest.raises(NotImplementedError, match=r"atomic=True takes float32 / float64.*gather form"):
            getattr(aa, name)(g, [4, 5], [1, 2, 9, 11], atomic=True)
    for name in ("linear_backward_nd", "cubic_backward_nd", "lanczos_backward_nd", "hamming_backward_nd"):
        with pytest.raises(_lib.AAInterpError, match="expected a tensor on a ROCm GPU"):
            getattr(aa, name)(torch.zeros(1, 2, 5, dtype=dt), [5], [1, 2, 11])
        with pytest.raises(_lib.AAInterpError, match="expected a tensor on a ROCm GPU"):
            getattr(aa, name)(torch.zeros(1, 2, 3, 4, 5, dtype=dt), [3, 4, 5], [1, 2, 6, 7, 8])
        with pytest.raises(_lib.AAInterpError, match="expected a tensor on a ROCm GPU"):
            getattr(aa, name)(g, [4, 5], [1, 2, 9, 11])


def test_python_backward_other_dtypes_keep_their_message():
    from interpolate_antialiasing_amd import extension_interpolate as aa

    text = "\"ti_upsample_bilinear2d_backward_cpu\" not implemented for '{}'"
    for dt, word in ((torch.int32, "Int"), (torch.uint8, "Byte"), (torch.int64, "Long")):
        g = torch.zeros(1, 2, 4, 5, dtype=dt)
        for atomic in (False, True):
            with pytest.raises(NotImplementedError) as e:
                aa.linear_backward(g, [4, 5], [1, 2, 9, 11], atomic=atomic)
            assert str(e.value) == text.format(word)
        with pytest.raises(NotImplementedError) as e:
            aa.linear_backward_nd(torch.zeros(1, 2, 5, dtype=dt), [5], [1, 2, 11])
        assert str(e.value) == text.format(word)


def test_docstrings_say_sixteen_bit_is_differentiable():
    from interpolate_antialiasing_amd import extension_interpolate as aa
    from interpolate_antialiasing_amd import interpolate_aa

    for doc in (aa.__doc__, interpolate_aa.__doc__, aa.linear_backward.__doc__, aa._backward_nd.__doc__):
        assert "float16 / bfloat16" in doc
