"""resize_many_to_float without a GPU: every argument error of the Python call (the tensors are on the CPU), the flip flag through the host
planner aa_many_plan, and the checks the new launch entry point makes before any launch."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from kit_golden import MEAN, STD  # noqa: E402

from interpolate_antialiasing_amd import _lib  # noqa: E402
from interpolate_antialiasing_amd import extension_interpolate as aa  # noqa: E402

BAD_DTYPE, BAD_SHAPE, WORKSPACE = -2, -4, -6


def _u8(c=3, h=20, w=30):
    return torch.zeros((c, h, w), dtype=torch.uint8)


# ---- the Python call ---------------------------------------------------------------------------------------------------------------------
def test_the_name_is_public():
    assert "resize_many_to_float" in aa.__all__ and callable(aa.resize_many_to_float)


@pytest.mark.parametrize("dt", [torch.float64, torch.uint8, torch.int32, None])
def test_out_dtype_outside_the_three_types_names_itself(dt):
    with pytest.raises(NotImplementedError, match="out_dtype"):
        aa.resize_many_to_float([_u8()], [10, 10], out_dtype=dt)


def test_mean_and_std_come_together():
    with pytest.raises(ValueError, match="mean and std must be given together"):
        aa.resize_many_to_float([_u8()], [10, 10], mean=MEAN[:3])
    with pytest.raises(ValueError, match="mean and std must be given together"):
        aa.resize_many_to_float([_u8()], [10, 10], std=STD[:3])


def test_mean_std_of_another_length_have_the_single_image_wording():
    with pytest.raises(RuntimeError, match=r"mean/std must hold one value per channel \(C = 3 <= 4\)"):
        aa.resize_many_to_float([_u8()], [10, 10], mean=MEAN[:2], std=STD[:3])
    with pytest.raises(RuntimeError, match=r"mean/std must hold one value per channel \(C = 3 <= 4\)"):
        aa.resize_many_to_float([_u8()], [10, 10], mean=MEAN[:3], std=STD[:4])
    with pytest.raises(RuntimeError, match=r"mean/std must hold one value per channel \(C = 1 <= 4\)"):
        aa.resize_many_to_float([_u8(1)], [10, 10], mean=MEAN[:3], std=STD[:3])


@pytest.mark.parametrize("bad", [0.0, float("inf"), float("nan"), -float("inf")])
def test_std_must_be_finite_and_not_zero(bad):
    with pytest.raises(ValueError, match=r"std\[1\]"):
        aa.resize_many_to_float([_u8()], [10, 10], mean=MEAN[:3], std=[58.395, bad, 57.375])


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_mean_must_be_finite(bad):
    with pytest.raises(ValueError, match=r"mean\[2\]"):
        aa.resize_many_to_float([_u8()], [10, 10], mean=[1.0, 2.0, bad], std=STD[:3])


def test_flips_hold_one_entry_per_image():
    with pytest.raises(ValueError, match=r"flips must hold one entry per image \(2\), got 1"):
        aa.resize_many_to_float([_u8(), _u8()], [10, 10], flips=[True])
    with pytest.raises(ValueError, match=r"flips must hold one entry per image \(1\), got 0"):
        aa.resize_many_to_float([_u8()], [10, 10], flips=[])


def test_bad_out_format_has_the_existing_wording():
    with pytest.raises(ValueError, match="out_format must be 'nchw', 'nhwc' or None"):
        aa.resize_many_to_float([_u8()], [10, 10], out_format="chw")


def test_the_checks_of_resize_many_hold_with_the_same_wording():
    with pytest.raises(ValueError, match="same C"):
        aa.resize_many_to_float([_u8(3), _u8(4)], [10, 10])
    with pytest.raises(NotImplementedError, match="float32"):
        aa.resize_many_to_float([_u8(3), torch.zeros((3, 20, 30))], [10, 10])
    with pytest.raises(ValueError, match="1 to 4 channels"):
        aa.resize_many_to_float([_u8(5)], [10, 10])
    with pytest.raises(ValueError, match="bilinearish"):
        aa.resize_many_to_float([_u8()], [10, 10], "bilinearish")
    with pytest.raises(ValueError, match="channels="):
        aa.resize_many_to_float([], [10, 10])
    with pytest.raises(ValueError, match="one entry per image"):
        aa.resize_many_to_float([_u8(), _u8()], [10, 10], boxes=[None])
    with pytest.raises(ValueError, match="box can't be empty"):
        aa.resize_many_to_float([_u8()], [10, 10], boxes=[(12, 5, 11, 9)])
    with pytest.raises(RuntimeError, match="output_size equals to 2"):
        aa.resize_many_to_float([_u8()], [10])


def test_harness_mode_set_globally_is_refused():
    prev = aa.get_uint8_mode()
    aa.set_uint8_mode("harness")
    try:
        with pytest.raises(NotImplementedError, match="harness"):
            aa.resize_many_to_float([_u8()], [10, 10])
    finally:
        aa.set_uint8_mode(prev)


@pytest.mark.parametrize("dt", [torch.float32, torch.float16, torch.bfloat16])
def test_valid_call_reaches_the_device_check_and_only_then(dt):
    with pytest.raises(_lib.AAInterpError, match="ROCm GPU"):
        aa.resize_many_to_float([_u8(), _u8(3, 7, 9)], [10, 10], "bicubic", boxes=[(1.5, 2, 20, 18), None], flips=[1, 0], out_dtype=dt,
                                out_format="nchw", mean=MEAN[:3], std=STD[:3])
    with pytest.raises(_lib.AAInterpError, match="ROCm GPU"):
        aa.resize_many_to_float(torch.zeros((2, 3, 20, 30), dtype=torch.uint8), [10, 10], out_dtype=dt)


@pytest.mark.parametrize("dt", [torch.float32, torch.float16, torch.bfloat16])
def test_empty_input_gives_an_empty_batch_of_out_dtype(dt):
    y = aa.resize_many_to_float(torch.zeros((0, 3, 20, 30), dtype=torch.uint8), [10, 12], out_dtype=dt, mean=MEAN[:3], std=STD[:3], flips=[])
    assert tuple(y.shape) == (0, 3, 10, 12) and y.dtype == dt
    y = aa.resize_many_to_float([], [10, 12], channels=2, out_dtype=dt)
    assert tuple(y.shape) == (0, 2, 10, 12) and y.dtype == dt


def test_resize_many_still_refuses_the_conversion_options():
    for kw in ({"out_dtype": torch.float32}, {"out_format": "nhwc"}, {"mean": [0.0] * 3, "std": [1.0] * 3}):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            aa.resize_many([_u8()], [10, 10], **kw)


def test_torch_op_has_a_meta_implementation():
    op = torch.ops.extension_interpolate.resize_many_to_float
    planar = [torch.empty((3, 20, 30), dtype=torch.uint8, device="meta"), torch.empty((3, 7, 9), dtype=torch.uint8, device="meta")]
    y = op(planar, [10, 12])
    assert tuple(y.shape) == (2, 3, 10, 12) and y.dtype == torch.float32 and y.is_contiguous()
    y = op(planar, [10, 12], "bicubic", None, [True, False], torch.bfloat16, "nhwc", MEAN[:3], STD[:3])
    assert y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=torch.channels_last) and not y.is_contiguous()
    inter = [torch.empty((20, 30, 3), dtype=torch.uint8, device="meta").permute(2, 0, 1),
             torch.empty((1, 7, 9, 3), dtype=torch.uint8, device="meta").permute(0, 3, 1, 2)]
    y = op(inter, [10, 12], "bicubic", [0.0, 0.0, 30.0, 20.0, 1.5, 2.0, 8.0, 6.5], None, torch.float16)
    assert y.dtype == torch.float16 and y.is_contiguous(memory_format=torch.channels_last) and not y.is_contiguous()
    y = op(inter, [10, 12], "bicubic", None, None, torch.float16, "nchw")
    assert tuple(y.shape) == (2, 3, 10, 12) and y.is_contiguous()


# ---- the C-ABI -----------------------------------------------------------------------------------------------------------------------------
def _plan(flags, layout=_lib.NCHW, c=3, oh=10, ow=10):
    """One 20 x 30 image per entry of `flags` -> (rc, buffer, header, items, workspace bytes); the data pointers are never dereferenced."""
    L = _lib.load()
    n = len(flags)
    recs = (_lib.ManyImage * max(n, 1))()
    for i, fl in enumerate(flags):
        r = recs[i]
        r.data_dev, r.H, r.W = 4096 + 4096 * i, 20, 30
        if layout == _lib.NHWC:
            r.stride_row, r.stride_px, r.stride_ch = 30 * c, c, 1
        else:
            r.stride_row, r.stride_px, r.stride_ch = 30, 1, 600
        r.flags = fl
    buf = (ctypes.c_uint8 * L.aa_many_desc_bytes(n))()
    ws = ctypes.c_size_t(0)
    rc = L.aa_many_plan(_lib.FILTER_LINEAR, layout, n, c, oh, ow, recs, ctypes.addressof(buf), len(buf), ctypes.byref(ws))
    hd, its, _ = _lib.many_desc_view(buf, n)
    return rc, buf, hd, its, ws.value


def test_abi_version_stays_3_and_the_symbol_is_exported():
    L = _lib.load()
    assert L.aa_abi_version() == 3
    assert "aa_resample_many_u8_to_float" in _lib.EXPORTS and hasattr(L, "aa_resample_many_u8_to_float")
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    assert "aa_resample_many_u8_to_float(" in header and "#define AA_MANY_FLIP_X 1" in header
    assert _lib.MANY_FLIP_X == 1
    assert ctypes.sizeof(_lib.ManyImage) == 88 and ctypes.sizeof(_lib.ManyItem) == 112 and ctypes.sizeof(_lib.ManyHeader) == 64


def test_plan_accepts_the_flip_flag_and_records_it_in_the_item():
    rc, _, hd, its, _ = _plan([0, _lib.MANY_FLIP_X, 0])
    assert rc == 0
    assert [it.flags for it in its] == [0, _lib.MANY_ITEM_FLIP, 0]
    assert hd.flips == 1  # some item flips
    rc, _, hd, its, _ = _plan([0, 0])
    assert rc == 0 and [it.flags for it in its] == [0, 0] and hd.flips == 0
    # the flag changes nothing else of the plan
    a, b = _plan([0, 0])[3], _plan([1, 1])[3]
    for x, y in zip(a, b):
        assert all(getattr(x, f) == getattr(y, f) for f, _ in _lib.ManyItem._fields_ if f != "reserved")


@pytest.mark.parametrize("bits", [2, 3, 4, 1 << 16, -1, -2])
def test_plan_rejects_other_flag_bits(bits):
    assert _plan([0, bits])[0] == BAD_SHAPE


def test_the_uint8_entry_point_refuses_a_flipped_plan():
    L = _lib.load()
    one = ctypes.c_void_p(4096)
    rc, buf, _, _, ws = _plan([0, 1])
    assert rc == 0
    assert L.aa_resample_many_u8(ctypes.addressof(buf), one, 2, 3, 10, 10, _lib.NCHW, one, one, ws, None) == BAD_SHAPE


def _cv(flags=0, out_layout=_lib.NCHW):
    cv = _lib.Convert()
    cv.out_layout, cv.normalize, cv.flags = out_layout, 0, flags
    return cv


def test_the_new_entry_point_rejects_bad_arguments_before_any_launch():
    L = _lib.load()
    f = L.aa_resample_many_u8_to_float
    one = ctypes.c_void_p(4096)
    rc, buf, _, _, ws = _plan([0, 1])
    assert rc == 0
    d = ctypes.addressof(buf)
    assert f(d, one, 2, 3, 10, 10, _lib.NCHW, one, one, ws, ctypes.byref(_cv(_lib.FLAG_OUT_F16 | _lib.FLAG_OUT_BF16)), None) == BAD_DTYPE
    assert f(d, one, 2, 3, 10, 10, _lib.NCHW, one, one, ws, ctypes.byref(_cv(_lib.FLAG_FAST)), None) == BAD_SHAPE
    assert f(d, one, 2, 3, 10, 10, _lib.NCHW, one, one, ws, ctypes.byref(_cv(_lib.FLAG_OUT_F16 | _lib.FLAG_FAST)), None) == BAD_SHAPE
    assert f(d, one, 2, 3, 10, 10, _lib.NCHW, one, one, ws, ctypes.byref(_cv(_lib.FLAG_PREMUL_ALPHA)), None) == BAD_SHAPE
    assert f(d, one, 2, 3, 10, 10, _lib.NCHW, one, one, ws, ctypes.byref(_cv(1 << 20)), None) == BAD_SHAPE
    for flags in (0, _lib.FLAG_OUT_F16, _lib.FLAG_OUT_BF16):
        cv = ctypes.byref(_cv(flags))
        assert f(d, one, 2, 3, 10, 10, _lib.NCHW, one, one, ws - 1, cv, None) == WORKSPACE  # a short workspace
        assert f(d, one, 3, 3, 10, 10, _lib.NCHW, one, one, ws, cv, None) == BAD_SHAPE  # another n
        assert f(d, one, 2, 3, 10, 11, _lib.NCHW, one, one, ws, cv, None) == BAD_SHAPE  # another oW
        assert f(d, one, 2, 3, 10, 10, _lib.NHWC, one, one, ws, cv, None) == BAD_SHAPE  # another class
        assert f(d, one, 2, 3, 10, 10, _lib.NCHW, ctypes.c_void_p(4097), one, ws, cv, None) == BAD_SHAPE  # out_dev not aligned to its element
        assert f(d, one, 2, 3, 10, 10, _lib.NCHW, one, ctypes.c_void_p(4104), ws, cv, None) == BAD_SHAPE  # the workspace: 16 bytes
        assert f(d, None, 2, 3, 10, 10, _lib.NCHW, one, one, ws, cv, None) == -5
    assert f(d, one, 2, 3, 10, 10, _lib.NCHW, ctypes.c_void_p(4098), one, ws, ctypes.byref(_cv(0)), None) == BAD_SHAPE  # float32: 4 bytes
    assert f(d, one, 2, 3, 10, 10, _lib.NCHW, one, one, ws, None, None) == -5  # no aa_convert
    assert f(d, one, 2, 3, 10, 10, _lib.NCHW, one, one, ws, ctypes.byref(_cv(0, 7)), None) == -3  # AA_ERR_BAD_LAYOUT


def test_the_new_entry_point_launches_nothing_for_an_empty_plan():
    L = _lib.load()
    rc, buf, _, _, ws = _plan([])
    assert rc == 0 and ws == 0
    for flags in (0, _lib.FLAG_OUT_F16, _lib.FLAG_OUT_BF16):
        assert L.aa_resample_many_u8_to_float(ctypes.addressof(buf), None, 0, 3, 10, 10, _lib.NCHW, None, None, 0, ctypes.byref(_cv(flags)),
                                              None) == 0
