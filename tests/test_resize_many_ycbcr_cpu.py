"""resize_many_ycbcr without a GPU: the restatement against the fixture, the conversion over all 2^24 triples (the Python tables and the
library's host function, which compiles the kernel's own inline code), the chroma helpers, the planner through ctypes (no device needed),
the Python call's argument errors, the exported symbols and the torch op's meta function."""
import ctypes
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kit_golden  # noqa: E402
import resize_many_ycbcr_ref as ref  # noqa: E402

from interpolate_antialiasing_amd import _lib, boxmath  # noqa: E402
from interpolate_antialiasing_amd import extension_interpolate as aa  # noqa: E402

G = ref.gen()
SHA = "71c995214d3efdbace5caebc1e25274c6d2822f0f675ce05f3bd9da47c9ebec6"  # Pillow's RGB bytes of all 2^24 triples, C order of [y, cb, cr]
NULL, BAD_SHAPE, WORKSPACE, STRIDES = -5, -4, -6, -10


# ---- the fixture and the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", G.keys())
def test_restatement_reproduces_the_fixture(key):
    name, f = key.split("/")
    assert np.array_equal(ref.restate(name, f), ref.expected(name, f))


def test_fixture_regenerates_from_pillow():
    pytest.importorskip("PIL")
    for key in G.keys():
        assert np.array_equal(G.pillow(*key.split("/")), ref.expected(*key.split("/"))), key
    lo, hi = G.clamp_shares()
    assert lo >= 0.05 and hi >= 0.05  # (the clamp case clamps on both sides, from Pillow's planes alone)


def test_fixture_is_small_and_stores_the_hash():
    assert os.path.getsize(os.path.join(kit_golden.GOLDEN, "resize_many_ycbcr.npz")) < 400 * 1024
    assert ref.stored_sha256() == SHA


# ---- the conversion, all 2^24 triples ---------------------------------------------------------------------------------------------------------
def test_python_tables_reproduce_the_hash():
    t = [np.array(x, np.int32) for x in boxmath.ycbcr_rgb_tables()]
    assert [len(x) for x in t] == [256] * 4 and all(np.array_equal(a, b) for a, b in zip(t, ref.tables()))
    ycc = G.all_triples()
    y, cb, cr = (ycc[..., k].astype(np.int32) for k in range(3))
    rgb = np.stack([y + (t[0][cr] >> 6), y + ((t[1][cb] + t[2][cr]) >> 6), y + (t[3][cb] >> 6)], axis=-1)
    assert int((rgb < 0).sum()) > 0 and int((rgb > 255).sum()) > 0
    assert hashlib.sha256(np.clip(rgb, 0, 255).astype(np.uint8).tobytes()).hexdigest() == SHA == ref.stored_sha256()


def test_library_host_conversion_reproduces_the_hash():
    L = _lib.load()
    ycc = G.all_triples()
    out = np.empty_like(ycc)
    assert L.aa_ycbcr_to_rgb_u8(ycc.ctypes.data, out.ctypes.data, ycc.size // 3) == 0
    assert hashlib.sha256(out.tobytes()).hexdigest() == SHA
    assert L.aa_ycbcr_to_rgb_u8(None, out.ctypes.data, 1) == NULL and L.aa_ycbcr_to_rgb_u8(None, None, 0) == 0
    assert L.aa_ycbcr_to_rgb_u8(ycc.ctypes.data, out.ctypes.data, -1) == BAD_SHAPE


# ---- the chroma helpers -----------------------------------------------------------------------------------------------------------------------
def test_chroma_shape_against_literal_values():
    assert boxmath.chroma_shape(37, 53, "420") == (19, 27) and boxmath.chroma_shape(37, 53, "422") == (37, 27)
    assert boxmath.chroma_shape(37, 53, "440") == (19, 53) and boxmath.chroma_shape(37, 53, "444") == (37, 53)
    assert boxmath.chroma_shape(1, 1, "420") == (1, 1) and boxmath.chroma_shape(2, 2, "420") == (1, 1) and boxmath.chroma_shape(3, 4, "420") == (2, 2)
    with pytest.raises(ValueError, match="subsampling"):
        boxmath.chroma_shape(4, 4, "411")


def test_chroma_box_is_the_float32_box_over_the_subsampling():
    f = lambda v: float(np.float32(v))  # noqa: E731
    box = (3.3, 2.2, 52.9, 36.1)
    got = boxmath.chroma_box(box, (37, 53), "420")
    want = tuple(float(np.float32(v) / np.float32(2)) for v in box)
    assert got == want == (f(3.3) / 2, f(2.2) / 2, f(52.9) / 2, f(36.1) / 2)
    assert got != tuple(v / 2 for v in box)  # (the float32 rounding comes first)
    assert got == (1.649999976158142, 1.100000023841858, 26.450000762939453, 18.049999237060547)
    assert boxmath.chroma_box(box, (37, 53), "422") == (f(3.3) / 2, f(2.2), f(52.9) / 2, f(36.1))
    assert boxmath.chroma_box(box, (37, 53), "440") == (f(3.3), f(2.2) / 2, f(52.9), f(36.1) / 2)
    assert boxmath.chroma_box(box, (37, 53), "444") == tuple(f(v) for v in box)
    # no box is still a proper chroma box for odd sizes: half a sample short of the [19, 27] plane
    assert boxmath.chroma_box(None, (37, 53), "420") == (0.0, 0.0, 26.5, 18.5)
    assert boxmath.chroma_box(None, (36, 52), "420") == (0.0, 0.0, 26.0, 18.0)
    for name, cs in G.CASES.items():
        for h, w, sub, bx in cs["items"]:
            assert boxmath.chroma_box(bx, (h, w), sub) == G.chroma_box(bx, h, w, sub) and boxmath.chroma_shape(h, w, sub) == G.chroma_shape(h, w, sub)


# ---- the planner through ctypes ---------------------------------------------------------------------------------------------------------------
def _records(items, px=1):
    """aa_ycbcr_image records of [(H, W, subsampling, box)] at made-up addresses (the planner never reads memory)."""
    recs = (_lib.YccImage * max(len(items), 1))()
    for i, (h, w, sub, bx) in enumerate(items):
        r = recs[i]
        ch, cw = boxmath.chroma_shape(h, w, sub)
        r.y_dev, r.cb_dev = 0x10000 + 0x100000 * i, 0x40001 + 0x100000 * i
        r.cr_dev = r.cb_dev + 1 if px == 2 else 0x70003 + 0x100000 * i
        r.H, r.W, r.cH, r.cW = h, w, ch, cw
        r.y_stride_row, r.cb_stride_row, r.cr_stride_row = w + 3, cw * px + 1, cw * px + (1 if px == 2 else 5)
        r.chroma_stride_px, r.subsampling = px, _lib.YCC_SUBSAMPLING[sub]
        if bx is not None:
            r.has_box = 1
            r.box[:] = bx
    return recs


def _plan(recs, n, oh, ow, f=_lib.FILTER_CUBIC, places=None, fill=None, nbytes=None):
    L = _lib.load()
    buf = (ctypes.c_uint8 * (L.aa_many_desc_bytes_ycbcr(n) if nbytes is None else nbytes))()
    ws = ctypes.c_size_t(0)
    cfill = (ctypes.c_uint8 * 3)(*fill) if fill is not None else None
    rc = L.aa_many_plan_ycbcr(f, n, oh, ow, recs, places, cfill, ctypes.addressof(buf), len(buf), ctypes.byref(ws))
    return rc, buf, ws.value


ITEMS = [(37, 53, "420", (3.3, 2.2, 52.9, 36.1)), (22, 30, "422", None), (9, 8, "444", None)]


def test_plan_composes_placed_plans_of_the_ragged_call():
    n = len(ITEMS)
    rc, buf, ws = _plan(_records(ITEMS), n, 20, 31, fill=(9, 250, 77))
    assert rc == 0 and ws > 0 and ws % 16 == 0
    hd = _lib.YccHeader.from_buffer(buf, 0)
    assert (hd.n, hd.oH, hd.oW, hd.interleaved, hd.off_a, hd.off_b, hd.fill, hd.ws_bytes) == (n, 20, 31, 0, 64, 0, 9 | 250 << 8 | 77 << 16, ws)
    # planar: ONE plan of 3 n single-channel items — the luma items, then Cb, then Cr, the chroma with the chroma box
    a = _lib.ManyHeader.from_buffer(buf, 64)
    assert (a.n, a.C, a.oH, a.oW, a.layout) == (3 * n, 1, 20, 31, _lib.NCHW) and a.kind == _lib.MANY_PLAN_PLACED
    items = (_lib.ManyItem * (3 * n)).from_buffer(buf, 64 + 64)
    cb = boxmath.chroma_box(ITEMS[0][3], (37, 53), "420")
    assert (items[0].in0_w, items[0].in0_h, items[0].in1_w, items[0].in1_h) == boxmath.box_f32(ITEMS[0][3]) and items[0].box_on == 1
    for k in (n, 2 * n):
        assert (items[k].in0_w, items[k].in0_h, items[k].in1_w, items[k].in1_h) == cb and items[k].box_on == 1
    assert items[1].box_on == 0 and items[n + 1].box_on == 0  # (even sizes and no box: the chroma box is the whole plane, i.e. none)
    assert items[n].src == 0x40001 and items[2 * n].src == 0x70003 and items[n].row_stride == 28 and items[2 * n].row_stride == 32
    # interleaved: the n luma items, and a second plan of n two-channel interleaved items behind it
    rc, buf, ws2 = _plan(_records(ITEMS, px=2), n, 20, 31)
    hd = _lib.YccHeader.from_buffer(buf, 0)
    assert rc == 0 and hd.interleaved == 1 and hd.off_b == 64 + _lib.load().aa_many_desc_bytes_placed(n) and 0 < hd.ws_b < hd.ws_bytes == ws2
    a, b = _lib.ManyHeader.from_buffer(buf, 64), _lib.ManyHeader.from_buffer(buf, hd.off_b)
    assert (a.n, a.C, a.layout, b.n, b.C, b.layout) == (n, 1, _lib.NCHW, n, 2, _lib.NHWC)


@pytest.mark.parametrize("key", G.keys())
@pytest.mark.parametrize("px", [1, 2])
def test_plan_accepts_every_fixture_case(key, px):
    name, f = key.split("/")
    cs = G.CASES[name]
    n = len(cs["items"])
    places = (_lib.ManyPlace * n)()
    for i, p in enumerate(G.places(name)):
        places[i].vH, places[i].vW, places[i].oy, places[i].ox = p
    rc, buf, ws = _plan(_records(cs["items"], px), n, *cs["canvas"], f=_lib.FILTER_IDS[f], places=places, fill=cs.get("fill"))
    assert rc == 0 and ws > 0
    # every item's vertical table and intermediate lie inside the workspace the plan asks for
    hd = _lib.YccHeader.from_buffer(buf, 0)
    for off, cnt, base, end in ((hd.off_a, n if px == 2 else 3 * n, 0, hd.ws_b), (hd.off_b, n if px == 2 else 0, hd.ws_b, hd.ws_bytes)):
        items = (_lib.ManyItem * cnt).from_buffer(buf, off + 64)
        assert all(0 <= it.tab_h <= it.tab_w <= it.inter <= end - base for it in items)


def test_plan_errors_come_before_any_launch():
    n = len(ITEMS)
    ok = lambda: _records(ITEMS)  # noqa: E731
    assert _plan(ok(), n, 20, 31)[0] == 0
    recs = ok()
    recs[1].cW += 1  # a wrong chroma shape
    assert _plan(recs, n, 20, 31)[0] == BAD_SHAPE
    recs = ok()
    recs[0].cH = 18  # floor instead of ceil
    assert _plan(recs, n, 20, 31)[0] == BAD_SHAPE
    for plane in ("y_dev", "cb_dev", "cr_dev"):  # a null plane
        recs = ok()
        setattr(recs[2], plane, None)
        assert _plan(recs, n, 20, 31)[0] == NULL
    recs = ok()
    recs[0].box[:] = (3.3, 2.2, 53.5, 36.1)  # a box beyond the image
    assert _plan(recs, n, 20, 31)[0] == BAD_SHAPE
    recs = ok()
    recs[0].box[:] = (5.0, 2.0, 5.0, 30.0)  # an empty box
    assert _plan(recs, n, 20, 31)[0] == BAD_SHAPE
    for sub in (-1, 4):  # a bad subsampling
        recs = ok()
        recs[1].subsampling = sub
        assert _plan(recs, n, 20, 31)[0] == BAD_SHAPE
    recs = ok()
    recs[1].chroma_stride_px = 2  # mixed arrangements
    assert _plan(recs, n, 20, 31)[0] == STRIDES
    recs = _records(ITEMS, px=2)
    recs[0].cr_dev += 1  # interleaved pairs whose Cr is not the byte after Cb
    assert _plan(recs, n, 20, 31)[0] == STRIDES
    recs = ok()
    recs[0].flags = 2  # only the flip bit
    assert _plan(recs, n, 20, 31)[0] == BAD_SHAPE
    assert _plan(ok(), n, 0, 31)[0] == BAD_SHAPE and _plan(ok(), n, 20, 31, f=9)[0] == -1
    assert _plan(ok(), n, 20, 31, nbytes=_lib.load().aa_many_desc_bytes_ycbcr(n) - 8)[0] == WORKSPACE
    assert _plan(None, n, 20, 31)[0] == NULL and _plan(ok(), -1, 20, 31, nbytes=64)[0] == BAD_SHAPE
    bad_place = (_lib.ManyPlace * n)()
    assert _plan(ok(), n, 20, 31, places=bad_place)[0] == BAD_SHAPE  # sizes of 0


def test_n_zero_plans_an_empty_block_that_launches_nothing():
    """n == 0 has the code of the other ragged planners: AA_OK, no workspace, and the launch returns at once without a device."""
    L = _lib.load()
    rc, buf, ws = _plan(None, 0, 20, 31)
    assert rc == 0 and ws == 0 and _lib.YccHeader.from_buffer(buf, 0).n == 0
    assert L.aa_resample_many_ycbcr(ctypes.addressof(buf), None, None, None, 0, None, _lib.NCHW, None) == 0
    assert L.aa_many_desc_bytes_ycbcr(0) >= 64 and L.aa_many_desc_bytes_ycbcr(-1) == 0


def test_launch_checks_come_before_any_launch():
    L = _lib.load()
    n = len(ITEMS)
    rc, buf, ws = _plan(_records(ITEMS), n, 20, 31)
    one, desc = ctypes.c_void_p(4096), ctypes.addressof(buf)
    launch = lambda **k: L.aa_resample_many_ycbcr(k.get("desc", desc), k.get("dev", one), k.get("out", one), k.get("ws_dev", one),  # noqa: E731
                                                  k.get("ws", ws), k.get("cv"), k.get("layout", _lib.NCHW), None)
    assert launch(dev=None) == NULL and launch(out=None) == NULL and launch(ws_dev=None) == NULL and launch(desc=None) == NULL
    assert launch(ws=ws - 1) == WORKSPACE and launch(ws_dev=ctypes.c_void_p(4104)) == BAD_SHAPE and launch(dev=ctypes.c_void_p(4100)) == BAD_SHAPE
    assert launch(layout=2) == -3
    cv = _lib.Convert()
    cv.flags = _lib.FLAG_OUT_F16 | _lib.FLAG_OUT_BF16
    assert launch(cv=ctypes.byref(cv)) == _lib.ERR_BAD_DTYPE
    cv.flags = 0
    assert launch(cv=ctypes.byref(cv), out=ctypes.c_void_p(4098)) == BAD_SHAPE  # a float32 output on a 2-byte boundary
    _lib.YccHeader.from_buffer(buf, 0).magic = 0
    assert launch() == BAD_SHAPE  # not a block of this plan


def test_abi_version_stays_3_and_the_symbols_are_exported():
    L = _lib.load()
    assert L.aa_abi_version() == 3
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    assert "#define AA_INTERP_ABI_VERSION 3 " in header and "} aa_ycbcr_image;" in header
    for sym in ("aa_many_desc_bytes_ycbcr", "aa_many_plan_ycbcr", "aa_resample_many_ycbcr", "aa_ycbcr_to_rgb_u8"):
        assert sym in _lib.EXPORTS and hasattr(L, sym) and sym + "(" in header
    assert ctypes.sizeof(_lib.YccImage) == 128 and ctypes.sizeof(_lib.YccHeader) == 64
    assert [f"#define AA_YCC_{k} {v}" in header for k, v in _lib.YCC_SUBSAMPLING.items()] == [True] * 4


# ---- argument errors of the Python call, all before any GPU use (the tensors are on the CPU) ------------------------------------------------
def _item(h=20, w=30, sub="420", interleaved=False, dtype=torch.uint8):
    ch, cw = boxmath.chroma_shape(h, w, sub)
    y = torch.zeros((h, w), dtype=dtype)
    if interleaved:
        return (y, torch.zeros((ch, cw, 2), dtype=dtype))
    return (y, torch.zeros((ch, cw), dtype=dtype), torch.zeros((ch, cw), dtype=dtype))


def test_each_bad_argument_raises_and_names_itself():
    call = aa.resize_many_ycbcr
    good = [_item(), _item(7, 9)]
    with pytest.raises(TypeError, match=r"images\[1\] Cb is torch.float32"):
        call([_item(), (good[1][0], good[1][1].float(), good[1][2])], [8, 8])
    with pytest.raises(TypeError, match=r"images\[0\] Y is torch.int16"):
        call([_item(dtype=torch.int16)], [8, 8])
    with pytest.raises(ValueError, match="one chroma arrangement per call"):
        call([_item(), _item(interleaved=True)], [8, 8])
    with pytest.raises(ValueError, match="fill must be one int or one per channel"):
        call(good, [8, 8], fill=(1, 2))
    with pytest.raises(ValueError, match="fill must be one int or one per channel"):
        call(good, [8, 8], fill=(1, 2, 3, 4))
    with pytest.raises(ValueError, match=r"its chroma must be \[10, 15\], got \[10, 16\]"):
        call([(torch.zeros((20, 30), dtype=torch.uint8), torch.zeros((10, 16), dtype=torch.uint8), torch.zeros((10, 16), dtype=torch.uint8))], [8, 8])
    with pytest.raises(ValueError, match=r"its chroma must be \[20, 15\]"):
        call([_item()], [8, 8], subsampling="422")
    with pytest.raises(ValueError, match="subsampling must be one of"):
        call(good, [8, 8], subsampling="411")
    with pytest.raises(ValueError, match="one string or one per image"):
        call(good, [8, 8], subsampling=["420"])
    with pytest.raises(TypeError, match="tuple"):
        call([torch.zeros((20, 30), dtype=torch.uint8)], [8, 8])
    with pytest.raises(ValueError, match=r"CbCr must be \[h, w, 2\]"):
        call([(good[0][0], torch.zeros((10, 15, 3), dtype=torch.uint8))], [8, 8])
    with pytest.raises(ValueError, match="mean and std must be given together"):
        call(good, [8, 8], out_dtype=torch.float32, mean=[1, 2, 3])
    with pytest.raises(ValueError, match="need a float out_dtype"):
        call(good, [8, 8], mean=[1, 2, 3], std=[1, 2, 3])
    with pytest.raises(ValueError, match="out_format"):
        call(good, [8, 8], out_format="hwc")
    with pytest.raises(NotImplementedError, match="out_dtype"):
        call(good, [8, 8], out_dtype=torch.float64)
    with pytest.raises(ValueError, match="boxes must hold one entry per image"):
        call(good, [8, 8], boxes=[None])
    with pytest.raises(ValueError):  # Pillow's wording for a box beyond the image
        call(good, [8, 8], boxes=[(0, 0, 31, 20), None])
    with pytest.raises(ValueError, match="flips must hold one entry per image"):
        call(good, [8, 8], flips=[True])
    with pytest.raises(ValueError, match=r"sizes\[0\]"):
        call(good, [8, 8], sizes=[(0, 4), (4, 4)])
    with pytest.raises(ValueError):
        call(good, [8, 8], "bilinearr")


def test_valid_call_reaches_the_device_check_and_only_then():
    with pytest.raises((RuntimeError, NotImplementedError, AssertionError)):
        aa.resize_many_ycbcr([_item(), _item(7, 9)], [8, 8], "bicubic", boxes=[(1.5, 0, 30, 20), None], fill=(1, 2, 3), flips=[True, False])


def test_empty_input_gives_an_empty_batch():
    y = aa.resize_many_ycbcr([], [5, 7])
    assert tuple(y.shape) == (0, 3, 5, 7) and y.dtype == torch.uint8
    assert aa.resize_many_ycbcr([], [5, 7], out_dtype=torch.bfloat16, mean=[1, 2, 3], std=[4, 5, 6]).dtype == torch.bfloat16


def test_the_torch_op_has_a_meta_implementation():
    op = torch.ops.extension_interpolate.resize_many_ycbcr
    m = lambda *s: torch.empty(s, dtype=torch.uint8, device="meta")  # noqa: E731
    y = op([m(20, 30), m(7, 9)], [m(10, 15), m(10, 15), m(4, 5), m(4, 5)], [8, 11])
    assert tuple(y.shape) == (2, 3, 8, 11) and y.dtype == torch.uint8 and y.is_contiguous() and y.device.type == "meta"
    y = op([m(20, 30)], [m(10, 15, 2)], [8, 11], "bicubic", out_dtype=torch.bfloat16, out_format="nhwc", mean=[1.0, 2.0, 3.0], std=[4.0, 5.0, 6.0])
    assert y.dtype == torch.bfloat16 and y.stride() == (8 * 11 * 3, 1, 11 * 3, 3)
    with pytest.raises((ValueError, RuntimeError), match="chroma must hold"):
        op([m(20, 30), m(7, 9)], [m(10, 15), m(10, 15), m(4, 5)], [8, 11])
