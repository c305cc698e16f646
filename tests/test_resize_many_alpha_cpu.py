"""resize_many(alpha=True) without a GPU: the fixture and its numpy restatement, the plan through the C-ABI (the flag bit, the copy rule,
every other field unchanged), the constants, and the Python argument checks."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import resize_many_alpha_ref as ref  # noqa: E402

from interpolate_antialiasing_amd import _lib  # noqa: E402
from interpolate_antialiasing_amd import extension_interpolate as aa  # noqa: E402

G = ref.gen()
ENTRIES = list(G.entries())
FILTER_IDS = {"linear": _lib.FILTER_LINEAR, "cubic": _lib.FILTER_CUBIC, "box": _lib.FILTER_BOX, "hamming": _lib.FILTER_HAMMING,
              "lanczos": _lib.FILTER_LANCZOS}
ALPHA, FLIP = _lib.MANY_PREMUL_ALPHA, _lib.MANY_FLIP_X
BAD_SHAPE = -4


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
def test_fixture_holds_every_entry():
    fx = ref.fixture()
    assert len(fx["crcs"]) == len(ENTRIES) == len(fx["sample_counts"]) == len(fx["channels"])
    assert {cs[0] for cs in G.CASES} == {"a_rgba", "a_la", "a_copy4", "a_copy2", "a_copyp4", "a_copyp2", "a_placed4", "a_placed2"}


@pytest.mark.parametrize("name", [cs[0] for cs in G.CASES])
def test_inputs_regenerate_and_the_restatement_equals_pillow(name):
    cs = G.case(name)
    for f in cs[4]:
        for i in range(len(cs[5])):
            ref.assert_matches_fixture(f"{name}/{f}/{i}", ref.item(name, i), ref.restated(name, f, i))


def test_copies_are_the_untouched_input_and_a_round_trip_would_not_be():
    for name in ("a_copy4", "a_copy2"):
        for i in (0, 1):
            x = ref.item(name, i).transpose(1, 2, 0)
            assert np.array_equal(ref.restated(name, "cubic", i), x)
            rt = x.copy()
            rt[..., :-1] = G.unpremul_formula(G.premul_formula(x[..., :-1], x[..., -1:]), x[..., -1:])
            assert not np.array_equal(rt, x)
        assert not np.array_equal(ref.restated(name, "cubic", 2), ref.restated(name, "cubic", 2, False))  # (alpha changes a real resize)


# ---- the plan ------------------------------------------------------------------------------------------------------------------------
def _records(layout, c, items, flags):
    """items [(H, W, box or None)] -> aa_many_image records; the data pointers are never dereferenced."""
    recs = (_lib.ManyImage * max(len(items), 1))()
    for i, (h, w, box) in enumerate(items):
        r = recs[i]
        r.data_dev, r.H, r.W = 4096 + 65536 * i, h, w
        if layout == _lib.NHWC:
            r.stride_row, r.stride_px, r.stride_ch = w * c, c, 1
        else:
            r.stride_row, r.stride_px, r.stride_ch = w, 1, h * w
        if box is not None:
            r.has_box = 1
            for k in range(4):
                r.box[k] = box[k]
        r.flags = flags[i]
    return recs


def _plan(layout, c, oh, ow, items, flags, places=None, fill=None, f="cubic"):
    """-> (rc, header, items, prefix, placement records or None, workspace bytes, buffer)"""
    L = _lib.load()
    n = len(items)
    recs = _records(layout, c, items, flags)
    nbytes = L.aa_many_desc_bytes_placed(n)
    buf = (ctypes.c_uint8 * nbytes)()
    ws = ctypes.c_size_t(0)
    if places is None:
        rc = L.aa_many_plan(FILTER_IDS[f], layout, n, c, oh, ow, recs, ctypes.addressof(buf), nbytes, ctypes.byref(ws))
    else:
        precs = (_lib.ManyPlace * max(n, 1))()
        for i, p in enumerate(places):
            precs[i].vH, precs[i].vW, precs[i].oy, precs[i].ox = p
        fl = (ctypes.c_uint8 * 4)(*(list(fill or []) + [0] * (4 - len(fill or []))))
        rc = L.aa_many_plan_placed(FILTER_IDS[f], layout, n, c, oh, ow, recs, precs, fl, ctypes.addressof(buf), nbytes, ctypes.byref(ws))
    hd, its, prefix = _lib.many_desc_view(buf, n)
    pls = _lib.many_placed_view(buf, n) if (rc == 0 and hd.kind & _lib.MANY_PLAN_PLACED) else None
    return rc, hd, its, prefix, pls, ws.value, buf


def _fields(struct, skip=()):
    return {name: (list(v) if hasattr(v, "__len__") else v) for name, _ in struct._fields_ if name not in skip for v in [getattr(struct, name)]}


ONE = [(20, 30, None)]


@pytest.mark.parametrize("layout", [_lib.NHWC, _lib.NCHW])
@pytest.mark.parametrize("c", [2, 4])
def test_plan_accepts_the_flag_for_two_and_four_channels(layout, c):
    rc, hd, its, _, _, _, _ = _plan(layout, c, 10, 10, ONE, [ALPHA])
    assert rc == 0, _lib.load().aa_strerror(rc)
    assert its[0].flags == _lib.MANY_ITEM_ALPHA and hd.kind == _lib.MANY_PLAN_ALPHA and hd.flips == 0
    rc, hd, its, _, _, _, _ = _plan(layout, c, 10, 10, ONE * 3, [0, ALPHA | FLIP, FLIP])
    assert rc == 0
    assert [it.flags for it in its] == [0, _lib.MANY_ITEM_FLIP | _lib.MANY_ITEM_ALPHA, _lib.MANY_ITEM_FLIP] and hd.kind == _lib.MANY_PLAN_ALPHA and hd.flips == 1
    rc, hd, its, _, _, _, _ = _plan(layout, c, 10, 10, ONE, [0])
    assert rc == 0 and its[0].flags == 0 and hd.kind == 0


@pytest.mark.parametrize("layout", [_lib.NHWC, _lib.NCHW])
@pytest.mark.parametrize("c", [1, 3])
def test_plan_refuses_the_flag_for_other_channel_counts(layout, c):
    assert _plan(layout, c, 10, 10, ONE, [ALPHA])[0] == BAD_SHAPE
    assert _plan(layout, c, 10, 10, ONE, [ALPHA], places=[(12, 9, 1, -2)], fill=[1, 2, 3])[0] == BAD_SHAPE
    assert _plan(layout, c, 10, 10, ONE, [0])[0] == 0


def test_plan_refuses_every_other_bit():
    for bit in (4, 8, 1 << 30):
        assert _plan(_lib.NHWC, 4, 10, 10, ONE, [bit])[0] == BAD_SHAPE
        assert _plan(_lib.NHWC, 4, 10, 10, ONE, [ALPHA | bit])[0] == BAD_SHAPE


@pytest.mark.parametrize("layout", [_lib.NHWC, _lib.NCHW])
@pytest.mark.parametrize("c", [2, 4])
def test_copy_rule_plain(layout, c):
    items = [(19, 37, None), (19, 37, (0.0, 0.0, 37.0, 19.0)), (19, 37, (2.5, 1.0, 30.0, 17.5)), (40, 50, None), (19, 37, (0, 0, 37, 18.5))]
    rc, hd, its, _, _, _, _ = _plan(layout, c, 19, 37, items, [ALPHA] * 5)
    assert rc == 0
    assert [it.flags for it in its] == [0, 0, _lib.MANY_ITEM_ALPHA, _lib.MANY_ITEM_ALPHA, _lib.MANY_ITEM_ALPHA] and hd.kind == _lib.MANY_PLAN_ALPHA
    rc, hd, its, _, _, _, _ = _plan(layout, c, 19, 37, items[:2], [ALPHA | FLIP, ALPHA])  # nothing but copies: no alpha launch at all
    assert rc == 0 and [it.flags for it in its] == [_lib.MANY_ITEM_FLIP, 0] and hd.kind == 0 and hd.flips == 1


@pytest.mark.parametrize("layout", [_lib.NHWC, _lib.NCHW])
@pytest.mark.parametrize("c", [2, 4])
def test_copy_rule_placed(layout, c):
    cs = G.case("a_copyp4")
    items = [it[:3] for it in cs[5]] + [(30, 45, None)]
    places = [it[3] + it[4] for it in cs[5]] + [(12, 17, 0, 0)]  # the last: the canvas's size is not the item's own
    rc, hd, its, _, pls, _, _ = _plan(layout, c, 30, 45, items, [ALPHA] * 5, places=places, fill=[1, 2, 3, 4][:c])
    assert rc == 0 and pls is not None
    assert [it.flags for it in its] == [0, 0, _lib.MANY_ITEM_ALPHA, _lib.MANY_ITEM_ALPHA, _lib.MANY_ITEM_ALPHA] and hd.kind == _lib.MANY_PLAN_PLACED | _lib.MANY_PLAN_ALPHA
    # a placed call whose places are all the canvas plans plain: the copy rule sees (oH, oW)
    rc, hd, its, _, pls, _, _ = _plan(layout, c, 12, 17, items[:2], [ALPHA] * 2, places=[(12, 17, 0, 0)] * 2, fill=[0] * c)
    assert rc == 0 and pls is None and [it.flags for it in its] == [0, 0] and hd.kind == 0


@pytest.mark.parametrize("layout", [_lib.NHWC, _lib.NCHW])
@pytest.mark.parametrize("name", ["a_rgba", "a_la", "a_copy4", "a_copyp2", "a_placed4", "a_placed2"])
def test_the_flag_changes_no_other_field(name, layout):
    cs = G.case(name)
    items = [it[:3] for it in cs[5]]
    places = [it[3] + it[4] for it in cs[5]] if cs[7] else None
    for f in cs[4]:
        a = _plan(layout, cs[1], cs[2][0], cs[2][1], items, [ALPHA] * len(items), places, cs[3], f)
        b = _plan(layout, cs[1], cs[2][0], cs[2][1], items, [0] * len(items), places, cs[3], f)
        assert a[0] == 0 and b[0] == 0
        assert a[5] == b[5] and a[1].ws_bytes == b[1].ws_bytes
        assert _fields(a[1], ("reserved",)) == _fields(b[1], ("reserved",))
        assert a[1].kind == b[1].kind | _lib.MANY_PLAN_ALPHA and a[1].fill == b[1].fill
        assert list(a[3]) == list(b[3])
        for i in range(len(items)):
            assert _fields(a[2][i], ("reserved",)) == _fields(b[2][i], ("reserved",)), (name, f, i)
            h, w, box, size, _ = cs[5][i]
            assert a[2][i].flags == (0 if G.is_copy(h, w, size[0], size[1], box) else _lib.MANY_ITEM_ALPHA) and b[2][i].flags == 0
            if places is not None:
                assert _fields(a[4][i]) == _fields(b[4][i])


@pytest.mark.parametrize("layout", [_lib.NHWC, _lib.NCHW])
def test_patch_plan_refuses_the_flag(layout):
    L = _lib.load()
    c = 4
    for flags, want in (([0], 0), ([FLIP], 0), ([ALPHA], BAD_SHAPE), ([ALPHA | FLIP], BAD_SHAPE)):
        recs = _records(layout, c, [(20, 30, None)], flags)
        nbytes = L.aa_many_desc_bytes_patches(1)
        buf = (ctypes.c_uint8 * nbytes)()
        ws, rows = ctypes.c_size_t(0), ctypes.c_int64(-1)
        sizes = (ctypes.c_int64 * 2)(16, 32)
        rc = L.aa_many_plan_patches(_lib.FILTER_CUBIC, layout, 1, c, 8, 8, recs, sizes, 0, ctypes.addressof(buf), nbytes, ctypes.byref(ws),
                                    ctypes.byref(rows))
        assert rc == want, flags


def test_constants_header_and_struct_sizes():
    L = _lib.load()
    assert L.aa_abi_version() == 3
    assert _lib.MANY_PREMUL_ALPHA == 2 and _lib.MANY_FLIP_X == 1
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    assert "#define AA_MANY_PREMUL_ALPHA 2" in header and "#define AA_MANY_FLIP_X 1" in header
    assert ctypes.sizeof(_lib.ManyImage) == 88 and ctypes.sizeof(_lib.ManyItem) == 112 and ctypes.sizeof(_lib.ManyHeader) == 64


# ---- the Python call -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 3])
def test_alpha_needs_two_or_four_channels(c):
    x = [torch.zeros((c, 8, 9), dtype=torch.uint8)]
    with pytest.raises(NotImplementedError, match="alpha"):
        aa.resize_many(x, [4, 4], "bilinear", alpha=True)
    with pytest.raises(NotImplementedError, match="alpha.*2- or 4-channel"):
        aa.resize_many_to_float(x, [4, 4], "bilinear", alpha=True)
    with pytest.raises(NotImplementedError, match="alpha"):
        aa.resize_many([], [4, 4], "bilinear", alpha=True, channels=c)


@pytest.mark.parametrize("c", [2, 4])
def test_alpha_reaches_the_device_check_on_cpu_tensors(c):
    x = [torch.zeros((c, 8, 9), dtype=torch.uint8)]
    with pytest.raises(Exception, match="ROCm GPU"):
        aa.resize_many(x, [4, 4], "bilinear", alpha=True)
    with pytest.raises(Exception, match="ROCm GPU"):
        aa.resize_many_to_float(x, [4, 4], "bilinear", alpha=True, out_dtype=torch.bfloat16)


def test_empty_batch_with_alpha():
    y = aa.resize_many([], [5, 6], "bicubic", alpha=True, channels=4)
    assert tuple(y.shape) == (0, 4, 5, 6) and y.dtype == torch.uint8
    z = aa.resize_many_to_float([], [5, 6], "bicubic", alpha=True, channels=2, out_dtype=torch.float16)
    assert tuple(z.shape) == (0, 2, 5, 6) and z.dtype == torch.float16


def test_torch_op_meta_functions_take_alpha():
    inter = [torch.empty((8, 9, 4), dtype=torch.uint8, device="meta").permute(2, 0, 1), torch.empty((5, 7, 4), dtype=torch.uint8, device="meta").permute(2, 0, 1)]
    planar = [torch.empty((4, 8, 9), dtype=torch.uint8, device="meta")]
    y = torch.ops.extension_interpolate.resize_many(inter, [6, 5], "bicubic", alpha=True)
    assert tuple(y.shape) == (2, 4, 6, 5) and y.dtype == torch.uint8 and y.is_contiguous(memory_format=torch.channels_last)
    y = torch.ops.extension_interpolate.resize_many(planar, [6, 5], "bicubic", None, None, None, None, True)
    assert tuple(y.shape) == (1, 4, 6, 5) and y.is_contiguous()
    z = torch.ops.extension_interpolate.resize_many_to_float(inter, [6, 5], "bicubic", out_dtype=torch.bfloat16, out_format="nchw", alpha=True)
    assert tuple(z.shape) == (2, 4, 6, 5) and z.dtype == torch.bfloat16 and z.is_contiguous()
    z = torch.ops.extension_interpolate.resize_many_to_float(planar, [6, 5], alpha=True)
    assert z.dtype == torch.float32 and z.is_contiguous()
