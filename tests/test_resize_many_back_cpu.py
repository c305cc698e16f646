"""resize_many_back without a GPU: the ABI, the planner (host arithmetic only), the launch checks that come before anything is enqueued,
the argument errors of the Python call, boxmath.placed_regions, and the CPU restatement of the definition (resize_many_back_ref)
against the dense float64 form."""
import ctypes

import numpy as np
import pytest
import torch

import resize_many_back_ref as ref
from interpolate_antialiasing_amd import _lib, boxmath
from interpolate_antialiasing_amd import extension_interpolate as aa

ERR_BAD_FILTER, ERR_BAD_DTYPE, ERR_BAD_LAYOUT, ERR_BAD_SHAPE, ERR_NULL, ERR_WORKSPACE, ERR_STRIDES = -1, -2, -3, -4, -5, -6, -10
MAX = (2 ** 31 - 1) // 4
PTR = 4096  # a dummy device address: the planner never follows it


def item(h=6, w=9, oh=3, ow=4, k=7, layout=_lib.NCHW, ptr=PTR, flags=0, strides=None):
    """One aa_back_item as a tuple (data_dev, stride_ch, stride_row, stride_px, h, w, oh, ow, flags) of a dense source in `layout`."""
    if strides is None:
        strides = (1, w * k, k) if layout == _lib.NHWC else (h * w, w, 1)
    return (ptr,) + tuple(strides) + (h, w, oh, ow, flags)


def plan(items, k=7, filt=_lib.FILTER_LINEAR, layout=_lib.NCHW, reduce=_lib.BACK_VALUES, out_dtype=_lib.F32, n=None, desc=True, short=0,
         null=()):
    L = _lib.load()
    n = len(items) if n is None else n
    nbytes = L.aa_back_many_desc_bytes(max(n, 0)) - short
    buf = (ctypes.c_uint8 * max(nbytes + short, 64))()
    recs = (_lib.BackItemIn * max(len(items), 1))()
    for r, it in zip(recs, items):
        r.data_dev, r.stride_ch, r.stride_row, r.stride_px, r.h, r.w, r.oh, r.ow, r.flags = it
    ws, arena = ctypes.c_size_t(0), ctypes.c_size_t(0)
    offs = (ctypes.c_int64 * max(len(items), 1))()
    rc = L.aa_back_many_plan(filt, layout, n, k, None if "items" in null else recs, reduce, out_dtype, ctypes.addressof(buf) if desc else None,
                             nbytes, None if "ws" in null else ctypes.byref(ws), None if "arena" in null else ctypes.byref(arena),
                             None if "offs" in null else offs)
    return rc, buf, ws.value, arena.value, list(offs)[:len(items)]


def table_bytes(out, ksize):
    return ((((64 + 8 * out + 15) & ~15) + 4 * out * ksize) + 15) & ~15


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------
def test_abi_is_additive():
    L = _lib.load()
    assert L.aa_abi_version() == 3
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    for sym in ("aa_back_many_desc_bytes", "aa_back_many_plan", "aa_resample_back_many"):
        assert sym in _lib.EXPORTS and hasattr(L, sym) and sym + "(" in header
    assert "aa_back_many_plan" in header.split("#define AA_INTERP_ABI_VERSION 3")[1].split("*/")[0]  # (listed in the version's comment)
    assert ctypes.sizeof(_lib.BackHeader) == 64 and ctypes.sizeof(_lib.BackItem) == 96 and ctypes.sizeof(_lib.BackItemIn) == 72
    assert L.aa_back_many_desc_bytes(3) == 64 + 3 * 96 + 4 * 8 and L.aa_back_many_desc_bytes(0) == 72 and L.aa_back_many_desc_bytes(-1) == 0
    assert "resize_many_back" in aa.__all__ and callable(aa.resize_many_back)


# ---- the planner ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduce,out_dtype,eb", [(_lib.BACK_VALUES, _lib.F32, 4), (_lib.BACK_VALUES, _lib.BF16, 2), (_lib.BACK_ARGMAX, _lib.U8, 1),
                                                 (_lib.BACK_ARGMAX, _lib.I64, 8), (_lib.BACK_GREATER, _lib.BOOL, 1)])
def test_plan_records_offsets_and_prefix(reduce, out_dtype, eb):
    L = _lib.load()
    k = 7
    shapes = list(zip(ref.BASE_REGIONS, ref.BASE_SIZES))
    items = [item(h, w, oh, ow, k, ptr=PTR + 4 * i, flags=i % 2, strides=(12 * 16, 16, 1)) for i, ((_, _, h, w), (oh, ow)) in enumerate(shapes)]
    rc, buf, ws, arena, offs = plan(items, k, _lib.FILTER_CUBIC, reduce=reduce, out_dtype=out_dtype)
    assert rc == 0
    hd, recs, prefix = _lib.back_desc_view(buf, len(items))
    assert (hd.n, hd.K, hd.filter, hd.layout, hd.reduce, hd.out_dtype, hd.ws_bytes, hd.arena_bytes) == (5, k, _lib.FILTER_CUBIC, _lib.NCHW, reduce,
                                                                                                    out_dtype, ws, arena)
    end, aend, units = 0, 0, 0
    for i, (it, ((_, _, h, w), (oh, ow))) in enumerate(zip(recs, shapes)):
        assert (it.src, it.h, it.w, it.oh, it.ow, it.flags) == (PTR + 4 * i, h, w, oh, ow, i % 2)
        # (the stride of an axis of one element is recorded as 0)
        assert (it.stride_ch, it.stride_row, it.stride_px) == (12 * 16, 16 if h > 1 else 0, 1 if w > 1 else 0)
        assert it.ksize_h == L.aa_table_ksize(_lib.FILTER_CUBIC, _lib.TABLE_F32, h, oh, 0, 0.0)
        assert it.ksize_w == L.aa_table_ksize(_lib.FILTER_CUBIC, _lib.TABLE_F32, w, ow, 0, 0.0)
        assert it.scale_h == np.float32(h) / np.float32(oh) and it.scale_w == np.float32(w) / np.float32(ow)
        # two tables one after the other, 16-byte aligned, none overlapping: header, xmin, xsize, rows of floats
        for off, (out, ks) in zip((it.tab_h, it.tab_w), ((oh, it.ksize_h), (ow, it.ksize_w))):
            assert off == end and off % 16 == 0
            end = off + table_bytes(out, ks)
        # the arena: every item on a 16-byte boundary, dense, in order
        aend = (aend + 15) & ~15
        assert it.out_off == offs[i] == aend
        aend += (1 if reduce == _lib.BACK_ARGMAX else k) * oh * ow * eb
        assert it.xtiles == -(-ow // _lib.BACK_TILE)
        assert prefix[i] == units
        units += oh * it.xtiles
    assert end == ws and aend == arena and prefix[len(items)] == units == hd.units
    assert units == 23 + 3 + 4 * 2 + 13 + 5


def test_plan_interleaved_and_one_element_axes():
    k = 8
    ok = item(6, 9, 3, 4, k, _lib.NHWC)
    assert plan([ok], k, layout=_lib.NHWC)[0] == 0
    assert plan([ok], k, layout=_lib.NCHW)[0] == ERR_STRIDES                                          # (not planes)
    assert plan([item(6, 9, 3, 4, k)], k, layout=_lib.NHWC)[0] == ERR_STRIDES                          # (not interleaved)
    assert plan([item(6, 9, 3, 4, k, _lib.NHWC, strides=(1, 100, k + 1))], k, layout=_lib.NHWC)[0] == ERR_STRIDES
    assert plan([item(6, 9, 3, 4, k, strides=(54, -9, 1))], k)[0] == ERR_STRIDES                        # (a negative stride)
    assert plan([item(6, 1, 3, 4, k, strides=(54, 9, 77))], k)[0] == 0                                 # (w == 1: stride_px is not looked at)
    assert plan([item(1, 9, 3, 4, k, strides=(54, -5, 1))], k)[0] == 0                                 # (h == 1: nor stride_row)
    for layout in (_lib.NCHW, _lib.NHWC):                                                              # (K == 1 is in both classes,
        assert plan([item(6, 9, 3, 4, 1, strides=(-3, 9, 1))], 1, layout=layout)[0] == 0               #  and stride_ch is not looked at)


def test_plan_empty():
    rc, buf, ws, arena, _ = plan([])
    assert (rc, ws, arena) == (0, 0, 0)
    hd, _, prefix = _lib.back_desc_view(buf, 0)
    assert hd.n == 0 and hd.units == 0 and list(prefix) == [0]
    L = _lib.load()
    assert L.aa_resample_back_many(ctypes.addressof(buf), None, _lib.F32, 0.0, None, 0, None, 0, None) == 0  # (nothing is launched)


def test_plan_error_codes_and_their_precedence():
    ok = [item()]
    bad_shape = [item(h=0)]
    assert plan(ok)[0] == 0
    # the filter before everything; then the layout; then n, K, reduce and K against a label type
    assert plan(bad_shape, filt=5, layout=7, n=-1, desc=False)[0] == ERR_BAD_FILTER
    assert plan(bad_shape, layout=7, n=-1, desc=False)[0] == ERR_BAD_LAYOUT
    assert plan(ok, n=-1, desc=False)[0] == ERR_BAD_SHAPE
    assert plan(ok, k=0, desc=False)[0] == ERR_BAD_SHAPE and plan(ok, k=MAX + 1)[0] == ERR_BAD_SHAPE
    assert plan(ok, reduce=3, desc=False)[0] == ERR_BAD_SHAPE and plan(ok, reduce=-1)[0] == ERR_BAD_SHAPE
    assert plan(ok, k=257, reduce=_lib.BACK_ARGMAX, out_dtype=_lib.U8, desc=False)[0] == ERR_BAD_SHAPE
    assert plan(ok, k=256, reduce=_lib.BACK_ARGMAX, out_dtype=_lib.U8)[0] == 0
    assert plan(ok, k=32769, reduce=_lib.BACK_ARGMAX, out_dtype=_lib.I16)[0] == ERR_BAD_SHAPE
    assert plan(ok, k=32768, reduce=_lib.BACK_ARGMAX, out_dtype=_lib.I16)[0] == 0
    assert plan(ok, k=32769, reduce=_lib.BACK_ARGMAX, out_dtype=_lib.I32)[0] == 0
    # the pointers, then the block's size, then the items
    for what in ("items", "ws", "arena", "offs"):
        assert plan(bad_shape, null=(what,), short=1)[0] == ERR_NULL, what
    assert plan(bad_shape, desc=False, short=1)[0] == ERR_NULL
    assert plan(bad_shape, short=1)[0] == ERR_WORKSPACE
    assert plan([item(ptr=None)])[0] == ERR_NULL
    for kw in ({"h": 0}, {"w": -1}, {"oh": 0}, {"ow": 0}, {"h": MAX + 1}, {"ow": MAX + 1}, {"flags": 2}, {"flags": 3}):
        assert plan([item(strides=(54, -9, 1), **kw)], out_dtype=_lib.F64)[0] == ERR_BAD_SHAPE, kw   # (before the strides and the dtype)
    assert plan([item(oh=1 << 20, ow=1 << 20)], k=2)[0] == ERR_BAD_SHAPE   # (K * oh * ow beyond 2^40)
    assert plan([item(oh=1 << 20, ow=1 << 19)], k=2)[0] == ERR_BAD_SHAPE   # (2^40 elements, but 2^31 work units: more than one grid holds)
    assert plan([item(oh=MAX, ow=8)] * 5, k=1)[0] == ERR_BAD_SHAPE         # (... and so are five times 2^29 - 1 rows)
    assert plan([item(strides=(54, -9, 1))], out_dtype=_lib.F64)[0] == ERR_STRIDES       # (the strides before the dtype)
    # the dtype a reduction stores, last
    for reduce, bad in ((_lib.BACK_VALUES, (_lib.U8, _lib.F64, _lib.I32, _lib.BOOL, 9, -1)), (_lib.BACK_ARGMAX, (_lib.F32, _lib.BOOL, _lib.F64)),
                        (_lib.BACK_GREATER, (_lib.F32, _lib.I16, _lib.I64))):
        for dt in bad:
            assert plan(ok, reduce=reduce, out_dtype=dt)[0] == ERR_BAD_DTYPE, (reduce, dt)


def test_a_2_40_element_item_plans():
    """The bounds are arithmetic only: the largest item the planner takes, and an arena offset beyond 2^31 after it."""
    rc, buf, ws, arena, offs = plan([item(h=3, w=3, oh=1 << 19, ow=1 << 19, k=4, strides=(9, 3, 1)), item(k=4)], k=4, reduce=_lib.BACK_ARGMAX,
                                    out_dtype=_lib.U8)
    assert rc == 0 and offs == [0, 1 << 38] and arena == (1 << 38) + 12
    _, _, prefix = _lib.back_desc_view(buf, 2)
    assert list(prefix) == [0, 1 << 30, (1 << 30) + 3]


# ---- the launch's checks, all before anything is enqueued (no device is touched) ------------------------------------------------------
def test_launch_checks():
    L = _lib.load()
    one = ctypes.c_void_p(256)
    blank = (ctypes.c_uint8 * 512)()
    call = L.aa_resample_back_many
    assert call(None, one, _lib.F32, 0.0, one, 1 << 20, one, 1 << 20, None) == ERR_NULL
    assert call(ctypes.addressof(blank), one, _lib.F32, 0.0, one, 1 << 20, one, 1 << 20, None) == ERR_BAD_SHAPE  # no plan's block
    rc, buf, ws, arena, _ = plan([item(ptr=256)], reduce=_lib.BACK_GREATER, out_dtype=_lib.BOOL)
    assert rc == 0
    d = ctypes.addressof(buf)
    for dt in (_lib.F64, _lib.U8, _lib.I32, 9):
        assert call(d, one, dt, 0.0, one, arena, one, ws, None) == ERR_BAD_DTYPE
    assert call(d, one, _lib.F32, float("nan"), one, arena, one, ws, None) == ERR_BAD_SHAPE
    assert call(d, one, _lib.F32, float("inf"), one, arena, one, ws, None) == ERR_BAD_SHAPE
    assert call(d, None, _lib.F32, 0.0, one, arena, one, ws, None) == ERR_NULL
    assert call(d, one, _lib.F32, 0.0, None, arena, one, ws, None) == ERR_NULL
    assert call(d, one, _lib.F32, 0.0, one, arena, None, ws, None) == ERR_NULL
    assert call(d, one, _lib.F32, 0.0, one, arena, one, ws - 1, None) == ERR_WORKSPACE
    assert call(d, one, _lib.F32, 0.0, one, arena - 1, one, ws, None) == ERR_WORKSPACE
    assert call(d, one, _lib.F32, 0.0, one, arena, ctypes.c_void_p(264), ws, None) == ERR_BAD_SHAPE   # (the workspace: 16 bytes)
    assert call(d, ctypes.c_void_p(260), _lib.F32, 0.0, one, arena, one, ws, None) == ERR_BAD_SHAPE   # (the device block: 8 bytes)
    # the arena against its element, the sources against theirs
    rc, buf, ws, arena, _ = plan([item(ptr=258)], reduce=_lib.BACK_VALUES, out_dtype=_lib.F32)
    d = ctypes.addressof(buf)
    assert call(d, one, _lib.BF16, 0.0, ctypes.c_void_p(258), arena, one, ws, None) == ERR_BAD_SHAPE
    assert call(d, one, _lib.F32, 0.0, one, arena, one, ws, None) == ERR_STRIDES
    # a block whose header was damaged after planning
    hd, _, _ = _lib.back_desc_view(buf, 1)
    hd.out_dtype = _lib.I16
    assert call(d, one, _lib.BF16, 0.0, one, arena, one, ws, None) == ERR_BAD_DTYPE
    hd.reduce = 5
    assert call(d, one, _lib.BF16, 0.0, one, arena, one, ws, None) == ERR_BAD_SHAPE


# ---- argument errors of the Python call, before any device work -------------------------------------------------------------------------
def test_argument_errors():
    p = torch.zeros(2, 7, 12, 16)
    sizes = [(5, 6), (7, 8)]
    call = aa.resize_many_back
    with pytest.raises(_lib.AAInterpError, match="no CPU implementation"):
        call(p, sizes)
    with pytest.raises(ValueError):
        call(p, sizes, mode="area")
    with pytest.raises(ValueError, match="reduce"):
        call(p, sizes, reduce="softmax")
    with pytest.raises(NotImplementedError, match=r"pred\[0\]"):
        call(p.double(), sizes)
    with pytest.raises(NotImplementedError, match=r"pred\[0\]"):
        call(p.to(torch.uint8), sizes)
    with pytest.raises(ValueError, match=r"\[N, K, H, W\]"):
        call(p[0], sizes)
    with pytest.raises(ValueError, match=r"same dtype: pred\[1\]"):
        call([p[0], p[1].half()], sizes)
    with pytest.raises(ValueError, match=r"same K: pred\[1\]"):
        call([p[0], p[1, :3]], sizes)
    with pytest.raises(ValueError, match=r"pred\[1\]"):
        call([p[0], p[1, 0]], sizes)
    with pytest.raises(TypeError, match=r"pred\[1\]"):
        call([p[0], None], sizes)
    with pytest.raises(ValueError, match="channels="):
        call([], [])
    assert call([], [], channels=19) == [] and call([], [], reduce="argmax", channels=19) == []
    with pytest.raises(ValueError, match="K must be"):
        call([], [], channels=0)
    with pytest.raises(ValueError, match="sizes must hold"):
        call(p, sizes[:1])
    with pytest.raises(ValueError, match=r"sizes\[1\]"):
        call(p, [(5, 6), (0, 8)])
    with pytest.raises(ValueError, match=r"sizes\[0\]"):
        call(p, [(5.5, 6), (7, 8)])
    with pytest.raises(ValueError, match=r"sizes\[1\].*beyond"):
        call(p, [(5, 6), (1 << 20, 1 << 18)])
    with pytest.raises(ValueError, match="regions must hold"):
        call(p, sizes, regions=[None])
    with pytest.raises(ValueError, match=r"regions\[1\].*four integers"):
        call(p, sizes, regions=[None, (0, 0, 3)])
    with pytest.raises(ValueError, match=r"regions\[1\].*four integers"):
        call(p, sizes, regions=[None, (0, 0, 3.5, 2)])
    with pytest.raises(ValueError, match=r"regions\[1\].*empty"):
        call(p, sizes, regions=[None, (0, 0, 0, 2)])
    for r in ((-1, 0, 3, 3), (0, 0, 13, 3), (10, 0, 3, 3), (0, 14, 3, 3)):
        with pytest.raises(ValueError, match=r"regions\[0\].*inside"):
            call(p, sizes, regions=[r, None])
    with pytest.raises(ValueError, match="flips"):
        call(p, sizes, flips=[True])
    for reduce, dt in ((None, torch.float64), (None, torch.uint8), ("argmax", torch.float32), ("argmax", torch.bool), ("greater", torch.int32)):
        with pytest.raises(NotImplementedError, match="out_dtype"):
            call(p, sizes, reduce=reduce, out_dtype=dt)
    big = torch.zeros(1, 300, 1, 1).expand(1, 300, 3, 3)
    with pytest.raises(ValueError, match="K = 300"):
        call(big, [(2, 2)], reduce="argmax", out_dtype=torch.uint8)
    with pytest.raises(ValueError, match="K = 32769"):
        call(torch.zeros(1, 1, 1, 1).expand(1, 32769, 2, 2), [(2, 2)], reduce="argmax", out_dtype=torch.int16)
    for thr in (float("nan"), float("inf"), 1e39, "x"):
        with pytest.raises(ValueError, match="threshold"):
            call(p, sizes, reduce="greater", threshold=thr)
    # everything in order: only the device is missing
    with pytest.raises(_lib.AAInterpError, match="no CPU implementation"):
        call(big, [(2, 2)], "lanczos", regions=[(1, 1, 2, 2)], flips=[True], reduce="argmax", out_dtype=torch.int16)


# ---- boxmath.placed_regions -----------------------------------------------------------------------------------------------------------
def cover(vh, vw, py, px, oh, ow):
    """aa_many_cover's rule (csrc/aa_many_host.h): -> (v0h, v0w, mh, mw, dy, dx), the covered part and where it starts on the canvas."""
    v0h, v0w = max(-py, 0), max(-px, 0)
    mh, mw = min(vh, oh - py) - v0h, min(vw, ow - px) - v0w
    return (v0h, v0w, mh, mw, v0h + py, v0w + px)


def test_placed_regions_against_the_cover_rule():
    out = (20, 32)
    sizes = [(20, 32), (10, 32), (20, 7), (1, 1), (13, 17), None]
    for offsets in (None, "center", [(0, 0), (10, 0), (0, 25), (19, 31), (3, 5), None]):
        got = boxmath.placed_regions(sizes, offsets, out)
        for i, (s, g) in enumerate(zip(sizes, got)):
            vh, vw = s or out
            py, px = ((boxmath.center_offset(vh, 20), boxmath.center_offset(vw, 32)) if offsets == "center" else
                      (0, 0) if offsets is None or offsets[i] is None else offsets[i])
            v0h, v0w, mh, mw, dy, dx = cover(vh, vw, py, px, *out)
            assert (v0h, v0w, mh, mw) == (0, 0, vh, vw), "the test's items lie wholly on the canvas"
            assert g == (dy, dx, vh, vw)
    assert boxmath.placed_regions([(10, 31)], "center", out) == [(5, 0, 10, 31)]  # (a pad: the smaller half first)
    assert boxmath.placed_regions(boxmath.fit_sizes([(480, 640), (1024, 768)], longer=32), "center", (32, 32)) == [(4, 0, 24, 32), (0, 4, 32, 24)]
    # overhanging or cropped items: where the cover rule gives less than the item
    for s, o in (((21, 32), None), ((20, 33), "center"), ((5, 5), [(-1, 0)]), ((5, 5), [(0, 28)]), ((5, 5), [(16, 0)]), ((5, 5), [(40, 40)])):
        py, px = (boxmath.center_offset(s[0], 20), boxmath.center_offset(s[1], 32)) if o == "center" else (0, 0) if o is None else o[0]
        c = cover(s[0], s[1], py, px, *out)
        assert (c[2], c[3]) != s
        with pytest.raises(ValueError, match="item 0"):
            boxmath.placed_regions([s], o, out)
    with pytest.raises(ValueError, match="item 1"):
        boxmath.placed_regions([(5, 5), (50, 5)], "center", out)
    with pytest.raises(ValueError):
        boxmath.placed_regions([(5, 5)], "middle", out)
    with pytest.raises(ValueError):
        boxmath.placed_regions([(5, 5)], [(0, 0), (1, 1)], out)
    with pytest.raises(ValueError):
        boxmath.placed_regions([(0, 5)], None, out)


# ---- the restatement against the dense float64 form -----------------------------------------------------------------------------------
_BASE = {}


def base(filt, canvas="base"):
    """(fp32 values, float64 values, bounds) of the base case, computed once per filter and canvas."""
    if (filt, canvas) not in _BASE:
        c = {"base": ref.BASE_CANVAS, "tie": ref.tie_canvas()}[canvas]
        _BASE[filt, canvas] = (ref.values(filt, c, ref.BASE_REGIONS, ref.BASE_SIZES),) + ref.dense_values(filt, c, ref.BASE_REGIONS, ref.BASE_SIZES)
    return _BASE[filt, canvas]


@pytest.mark.parametrize("filt", ref.ORACLE_FILTERS)
def test_restated_values_within_the_dense_bound(filt):
    got, want, bnd = base(filt)
    assert [g.shape for g in got] == [(7,) + s for s in ref.BASE_SIZES] and all(g.dtype == np.float32 for g in got)
    r = ref.worst_ratio(got, want, bnd)
    print(f"values {filt}: worst err / bound {r:.3f}")
    assert r <= 0.33
    # the identity item is the source's bits
    y0, x0, h, w = ref.BASE_REGIONS[ref.IDENTITY_ITEM]
    src = ref.BASE_CANVAS[ref.IDENTITY_ITEM][:, y0:y0 + h, x0:x0 + w]
    assert np.array_equal(got[ref.IDENTITY_ITEM].view(np.int32), np.ascontiguousarray(src).view(np.int32))


def test_restated_argmax_is_the_float64_argmax_at_every_pixel():
    """No pixel is left out: at each of the 3 x 2025 = 6075 pixels of the base case under the three filters, the float64 top-two margin
    exceeds twice the bound, so the argmax of ANY fp32 result within the bound is the float64 argmax."""
    pixels = excluded = 0
    for filt in ref.ORACLE_FILTERS:
        got, want, bnd = base(filt)
        ok, arg = ref.decided(want, bnd)
        pixels += sum(o.size for o in ok)
        excluded += sum(int((~o).sum()) for o in ok)
        for lab, a in zip(ref.labels(got), arg):
            assert np.array_equal(lab, a)
    print(f"argmax: {excluded} of {pixels} pixels within twice the bound of a tie")
    assert pixels == 3 * ref.BASE_PIXELS == 6075 and excluded == 0


def test_tie_case_needs_the_lowest_index():
    """Plane 4 is plane 2 and plane 6 is the constant 0.25: class 4 never wins, and wherever class 2 wins the maximum is attained twice,
    so a `>=` or a last-index rule answers 4 there.  The count: numpy gives 66 such pixels of the first item's 713 under the linear
    filter (class 6 wins 126 more, untied: the constant resamples to exactly 0.25); the 87 this case was first described with was not
    reproduced by any count tried (per filter, per class, over all items)."""
    got, _, _ = base("linear", "tie")
    v = got[0]
    lab = ref.labels(got)
    assert all(not (x == 4).any() for x in lab), "class 4 is a copy of class 2: the lowest index wins"
    assert np.array_equal(v[4].view(np.int32), v[2].view(np.int32)) and (v[6] == np.float32(0.25)).all()
    last = v.shape[0] - 1 - np.argmax(v[::-1], axis=0)
    tied = last != lab[0]
    print(f"tie case: {int(tied.sum())} of {lab[0].size} pixels of item 0 have a tied maximum; class 6 wins {int((lab[0] == 6).sum())}")
    assert lab[0].size == 713 and int(tied.sum()) == 66 and set(lab[0][tied].tolist()) == {2} and set(last[tied].tolist()) == {4}
    assert int((lab[0] == 6).sum()) == 126


@pytest.mark.parametrize("filt", ref.FILTERS)
def test_dense_form_has_all_five_filters(filt):
    want, bnd = ref.dense_values(filt, ref.BASE_CANVAS, ref.BASE_REGIONS, ref.BASE_SIZES, flips=[True, False, True, False, False])
    plain, _ = ref.dense_values(filt, ref.BASE_CANVAS, ref.BASE_REGIONS, ref.BASE_SIZES)
    assert all(np.array_equal(w[:, :, ::-1] if f else w, p) for w, p, f in zip(want, plain, [True, False, True, False, False]))
    assert all((b >= 0).all() and w.shape == b.shape for w, b in zip(want, bnd))


def test_further_cases_restated():
    for k in (1, 2, 8, 19):
        got = ref.values("cubic", ref.k_canvas(k), ref.BASE_REGIONS, ref.BASE_SIZES)
        want, bnd = ref.dense_values("cubic", ref.k_canvas(k), ref.BASE_REGIONS, ref.BASE_SIZES)
        assert ref.worst_ratio(got, want, bnd) <= 1.0
    c, regions, sizes = ref.k300_case()
    lab = ref.labels(ref.values("linear", c, regions, sizes))[0]
    assert lab.shape == (5, 4) and (lab == 299).any() and lab.max() > 255
    c, regions, sizes = ref.seventy_case()
    vals = ref.values("linear", c, regions, sizes)
    assert len(vals) == 70 and all(v.shape == (3,) + s for v, s in zip(vals, sizes))
    srcs, regions, sizes = ref.list_case()
    vals = ref.values("box", srcs, regions, sizes, flips=[True, False, False, True])
    plain = ref.values("box", srcs, regions, sizes)
    assert np.array_equal(vals[0], plain[0][:, :, ::-1]) and np.array_equal(vals[1], plain[1])
    # a NaN wins, the first one; +inf beats every number; a NaN is not greater
    nf = ref.values("linear", ref.nonfinite_canvas(), ref.BASE_REGIONS, ref.BASE_SIZES)
    lab, m = ref.labels(nf), ref.masks(nf, 0.0)
    nan0 = np.isnan(nf[0])
    assert nan0.any() and np.array_equal(lab[0][nan0.any(axis=0)], np.argmax(nan0, axis=0)[nan0.any(axis=0)])
    assert not m[0][nan0].any() and (m[0][np.isposinf(nf[0])]).all()
    assert ref.to_bf16_bits(np.array([1.0, 1.00390625, 1.01171875], np.float32)).tolist() == [0x3F80, 0x3F80, 0x3F82]
