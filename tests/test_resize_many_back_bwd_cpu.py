"""resize_many_back_backward without a GPU: the ABI, the planner (host arithmetic only), the argument errors of the Python call, and the
CPU restatement of the definition (resize_many_back_bwd_ref) against its dense float64 form and against the forward's restatement."""
import ctypes

import numpy as np
import pytest
import torch

import resize_many_back_bwd_ref as ref
import resize_many_back_ref as fwd_ref
from interpolate_antialiasing_amd import _lib
from interpolate_antialiasing_amd import extension_interpolate as aa

ERR_BAD_FILTER, ERR_BAD_DTYPE, ERR_BAD_LAYOUT, ERR_BAD_SHAPE, ERR_NULL, ERR_WORKSPACE, ERR_KSIZE, ERR_STRIDES = -1, -2, -3, -4, -5, -6, -7, -10
MAX = (2 ** 31 - 1) // 4
PTR = 4096  # a dummy device address: the planner never follows it


def item(canvas=(12, 16), region=(1, 2, 6, 9), size=(3, 4), k=7, ptr=PTR, flags=0, strides=None):
    """One aa_back_bwd_item as a tuple (grad_dev, stride_ch, stride_row, H, W, y0, x0, h, w, oh, ow, flags) of a dense gradient."""
    if strides is None:
        strides = (size[0] * size[1], size[1])
    return (ptr,) + tuple(strides) + tuple(canvas) + tuple(region) + tuple(size) + (flags,)


def plan(items, k=7, filt=_lib.FILTER_LINEAR, layout=_lib.NCHW, out_dtype=_lib.F32, dense=0, n=None, desc=True, short=0, null=()):
    L = _lib.load()
    n = len(items) if n is None else n
    nbytes = L.aa_back_many_bwd_desc_bytes(max(n, 0)) - short
    buf = (ctypes.c_uint8 * max(nbytes + short, 64))()
    recs = (_lib.BackBwdItemIn * max(len(items), 1))()
    for r, it in zip(recs, items):
        r.grad_dev, r.stride_ch, r.stride_row, r.H, r.W, r.y0, r.x0, r.h, r.w, r.oh, r.ow, r.flags = it
    ws, out = ctypes.c_size_t(0), ctypes.c_size_t(0)
    offs = (ctypes.c_int64 * max(len(items), 1))()
    rc = L.aa_back_many_bwd_plan(filt, layout, n, k, None if "items" in null else recs, out_dtype, dense, ctypes.addressof(buf) if desc else None,
                                 nbytes, None if "ws" in null else ctypes.byref(ws), None if "out" in null else ctypes.byref(out),
                                 None if "offs" in null else offs)
    return rc, buf, ws.value, out.value, list(offs)[:len(items)]


def table_bytes(rows, ksize):
    return ((((64 + 8 * rows + 15) & ~15) + 4 * rows * ksize) + 15) & ~15


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------
def test_abi_is_additive():
    L = _lib.load()
    assert L.aa_abi_version() == 3
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    version_comment = header.split("#define AA_INTERP_ABI_VERSION 3")[1].split("*/")[0]
    for sym in ("aa_back_many_bwd_desc_bytes", "aa_back_many_bwd_plan", "aa_resample_back_many_bwd"):
        assert sym in _lib.EXPORTS and hasattr(L, sym) and sym + "(" in header
        assert sym in version_comment  # (listed in the version's comment)
    assert ctypes.sizeof(_lib.BackBwdHeader) == 64 and ctypes.sizeof(_lib.BackBwdItem) == 128 and ctypes.sizeof(_lib.BackBwdItemIn) == 96
    assert L.aa_back_many_bwd_desc_bytes(3) == 64 + 3 * 128 + 4 * 8 and L.aa_back_many_bwd_desc_bytes(0) == 72
    assert L.aa_back_many_bwd_desc_bytes(-1) == 0
    assert "resize_many_back_backward" in aa.__all__ and callable(aa.resize_many_back_backward)


# ---- the planner ----------------------------------------------------------------------------------------------------------------------
def base_items(k, none=()):
    return [item(ref.BASE_HW, r, s, k, ptr=None if i in none else PTR + 4 * i, flags=int(ref.BASE_FLIPS[i]))
            for i, (r, s) in enumerate(zip(ref.BASE_REGIONS, ref.BASE_SIZES))]


@pytest.mark.parametrize("out_dtype,eb", [(_lib.F32, 4), (_lib.BF16, 2)])
@pytest.mark.parametrize("dense", (0, 1))
@pytest.mark.parametrize("k", (7, 3))
def test_plan_records_offsets_and_prefix(out_dtype, eb, dense, k):
    L = _lib.load()
    hh, ww = ref.BASE_HW
    items = base_items(k, none=(3,))
    rc, buf, ws, out, offs = plan(items, k, _lib.FILTER_CUBIC, _lib.NHWC, out_dtype, dense)
    assert rc == 0
    hd, recs, prefix = _lib.back_bwd_desc_view(buf, len(items))
    assert (hd.n, hd.K, hd.filter, hd.out_layout, hd.out_dtype, hd.dense, hd.ws_bytes, hd.out_bytes) == (5, k, _lib.FILTER_CUBIC, _lib.NHWC, out_dtype,
                                                                                                       dense, ws, out)
    end, oend, units = 0, 0, 0
    for i, (it, (y0, x0, h, w), (oh, ow)) in enumerate(zip(recs, ref.BASE_REGIONS, ref.BASE_SIZES)):
        assert (it.H, it.W) == (hh, ww)
        if i == 3:  # no gradient: no region, no sizes, no table bytes
            assert it.grad is None and (it.h, it.w, it.oh, it.ow, it.tab_h, it.tab_w, it.tr_h, it.tr_w) == (0,) * 8
        else:
            assert (it.grad, it.y0, it.x0, it.h, it.w, it.oh, it.ow, it.flags) == (PTR + 4 * i, y0, x0, h, w, oh, ow, int(ref.BASE_FLIPS[i]))
            # (the stride of an axis of one element is recorded as 0)
            assert (it.stride_ch, it.stride_row) == (oh * ow if k > 1 else 0, ow if oh > 1 else 0)
            assert it.ksize_h == L.aa_table_ksize(_lib.FILTER_CUBIC, _lib.TABLE_F32, h, oh, 0, 0.0)
            assert it.ksize_w == L.aa_table_ksize(_lib.FILTER_CUBIC, _lib.TABLE_F32, w, ow, 0, 0.0)
            assert it.trk_h == L.aa_table_transposed_ksize(_lib.FILTER_CUBIC, _lib.TABLE_F32, h, oh, 0, 0.0)
            assert it.trk_w == L.aa_table_transposed_ksize(_lib.FILTER_CUBIC, _lib.TABLE_F32, w, ow, 0, 0.0)
            assert it.scale_h == np.float32(h) / np.float32(oh) and it.scale_w == np.float32(w) / np.float32(ow)
            # four tables one after the other, 16-byte aligned, none overlapping: the forward pair, then their adjoints
            for off, (rows, ks) in zip((it.tab_h, it.tab_w, it.tr_h, it.tr_w), ((oh, it.ksize_h), (ow, it.ksize_w), (h, it.trk_h), (w, it.trk_w))):
                assert off == end and off % 16 == 0
                end = off + table_bytes(rows, ks)
        if not dense:
            oend = (oend + 15) & ~15
            assert offs[i] % 16 == 0
        assert it.out_off == offs[i] == oend
        oend += k * hh * ww * eb
        assert it.xtiles == -(-ww // _lib.BACK_BWD_COLS)
        assert prefix[i] == units
        units += -(-hh // _lib.BACK_BWD_ROWS) * it.xtiles
    assert end == ws and oend == out and prefix[len(items)] == units == hd.units
    assert all(prefix[i] <= prefix[i + 1] for i in range(len(items)))
    # a second plan of the same arguments is the same bytes
    assert bytes(plan(items, k, _lib.FILTER_CUBIC, _lib.NHWC, out_dtype, dense)[1]) == bytes(buf)


def test_plan_all_none_and_empty():
    rc, buf, ws, out, offs = plan(base_items(7, none=range(5)), 7)
    assert (rc, ws) == (0, 0) and out == 5 * 7 * 12 * 16 * 4 and offs == [i * 7 * 12 * 16 * 4 for i in range(5)]
    rc, buf, ws, out, _ = plan([])
    assert (rc, ws, out) == (0, 0, 0)
    hd, _, prefix = _lib.back_bwd_desc_view(buf, 0)
    assert hd.n == 0 and hd.units == 0 and list(prefix) == [0]
    L = _lib.load()
    assert L.aa_resample_back_many_bwd(ctypes.addressof(buf), None, _lib.F32, None, 0, None, 0, None) == 0  # (nothing is launched)


def test_plan_error_codes_and_their_precedence():
    ok = [item()]
    bad_shape = [item(canvas=(0, 16))]
    assert plan(ok)[0] == 0
    # the filter before everything; then the layout; then n, K and dense
    assert plan(bad_shape, filt=5, layout=7, n=-1, desc=False)[0] == ERR_BAD_FILTER
    assert plan(bad_shape, layout=7, n=-1, desc=False)[0] == ERR_BAD_LAYOUT
    assert plan(ok, n=-1, desc=False)[0] == ERR_BAD_SHAPE
    assert plan(ok, k=0, desc=False)[0] == ERR_BAD_SHAPE and plan(ok, k=MAX + 1)[0] == ERR_BAD_SHAPE
    assert plan(ok, dense=2, desc=False)[0] == ERR_BAD_SHAPE and plan(ok, dense=-1)[0] == ERR_BAD_SHAPE
    # the pointers, then the block's size, then the items
    for what in ("items", "ws", "out", "offs"):
        assert plan(bad_shape, null=(what,), short=1)[0] == ERR_NULL, what
    assert plan(bad_shape, desc=False, short=1)[0] == ERR_NULL
    assert plan(bad_shape, short=1)[0] == ERR_WORKSPACE
    # per item: the canvas and the flags; with a gradient its size and its region; before the strides and the dtype
    for kw in ({"canvas": (0, 16)}, {"canvas": (12, -1)}, {"canvas": (MAX + 1, 16)}, {"flags": 2}, {"size": (0, 4)}, {"size": (3, MAX + 1)},
               {"region": (1, 2, 0, 9)}, {"region": (-1, 2, 6, 9)}, {"region": (7, 2, 6, 9)}, {"region": (1, 8, 6, 9)}, {"region": (0, 0, 13, 16)}):
        assert plan([item(strides=(12, -4), **kw)], out_dtype=_lib.F64)[0] == ERR_BAD_SHAPE, kw
    assert plan([item(canvas=(1 << 20, 1 << 20), region=(0, 0, 2, 2))], k=2)[0] == ERR_BAD_SHAPE   # (K * H * W beyond 2^40)
    assert plan([item(size=(1 << 20, 1 << 20))], k=2)[0] == ERR_BAD_SHAPE                           # (K * oh * ow beyond 2^40)
    # an item without a gradient: nothing but its canvas and its flags is looked at
    assert plan([item(ptr=None, region=(-5, 99, 0, 0), size=(0, -3), strides=(-1, -1))])[0] == 0
    assert plan([item(ptr=None, canvas=(0, 16))])[0] == ERR_BAD_SHAPE
    assert plan([item(strides=(12, -4))], out_dtype=_lib.F64)[0] == ERR_STRIDES and plan([item(strides=(-12, 4))])[0] == ERR_STRIDES
    assert plan([item(size=(1, 4), strides=(4, -4))])[0] == 0     # (oh == 1: stride_row is not looked at)
    assert plan([item(k=1, strides=(-3, 4))], k=1)[0] == 0        # (K == 1: nor stride_ch)
    assert plan([item(canvas=(MAX, 64), region=(0, 0, 2, 2))] * 15, k=1)[0] == 0
    assert plan([item(canvas=(MAX, 64), region=(0, 0, 2, 2))] * 16, k=1)[0] == ERR_BAD_SHAPE  # (2^31 work units: more than one grid holds)
    # the dtype last
    for dt in (_lib.U8, _lib.F64, _lib.I32, _lib.BOOL, 9, -1):
        assert plan(ok, out_dtype=dt)[0] == ERR_BAD_DTYPE, dt


def test_launch_checks():
    """All before anything is enqueued: no device is touched."""
    L = _lib.load()
    one = ctypes.c_void_p(256)
    blank = (ctypes.c_uint8 * 512)()
    call = L.aa_resample_back_many_bwd
    assert call(None, one, _lib.F32, one, 1 << 20, one, 1 << 20, None) == ERR_NULL
    assert call(ctypes.addressof(blank), one, _lib.F32, one, 1 << 20, one, 1 << 20, None) == ERR_BAD_SHAPE  # no plan's block
    rc, buf, ws, out, _ = plan([item(ptr=258)])
    assert rc == 0
    d = ctypes.addressof(buf)
    for dt in (_lib.F64, _lib.U8, _lib.I32, 9):
        assert call(d, one, dt, one, out, one, ws, None) == ERR_BAD_DTYPE
    assert call(d, None, _lib.BF16, one, out, one, ws, None) == ERR_NULL
    assert call(d, one, _lib.BF16, None, out, one, ws, None) == ERR_NULL
    assert call(d, one, _lib.BF16, one, out, None, ws, None) == ERR_NULL
    assert call(d, one, _lib.BF16, one, out, one, ws - 1, None) == ERR_WORKSPACE
    assert call(d, one, _lib.BF16, one, out - 1, one, ws, None) == ERR_WORKSPACE
    assert call(d, one, _lib.BF16, one, out, ctypes.c_void_p(264), ws, None) == ERR_BAD_SHAPE   # (the workspace: 16 bytes)
    assert call(d, ctypes.c_void_p(260), _lib.BF16, one, out, one, ws, None) == ERR_BAD_SHAPE   # (the device block: 8 bytes)
    assert call(d, one, _lib.BF16, ctypes.c_void_p(258), out, one, ws, None) == ERR_BAD_SHAPE   # (the output against its element)
    assert call(d, one, _lib.F32, one, out, one, ws, None) == ERR_STRIDES                       # (the gradient against its element)


# ---- argument errors of the Python call, before any device work -------------------------------------------------------------------------
def test_argument_errors():
    g = [torch.zeros(7, 5, 6), torch.zeros(7, 7, 8)]
    call = aa.resize_many_back_backward
    with pytest.raises(_lib.AAInterpError, match="no CPU implementation"):
        call(g, (12, 16))
    with pytest.raises(_lib.AAInterpError, match="no CPU implementation"):
        call([None, None], (12, 16), channels=7, dtype=torch.float32, device="cpu")
    with pytest.raises(ValueError):
        call(g, (12, 16), mode="area")
    with pytest.raises(ValueError, match="out_format"):
        call(g, (12, 16), out_format="chw")
    with pytest.raises(ValueError, match="sequence"):
        call(torch.zeros(2, 7, 5, 6), (12, 16))
    with pytest.raises(ValueError, match="sequence"):
        call(5, (12, 16))
    with pytest.raises(TypeError, match=r"grads\[1\]"):
        call([g[0], 3.0], (12, 16))
    with pytest.raises(ValueError, match=r"grads\[1\] must be \[K, oh, ow\]"):
        call([g[0], g[1][None]], (12, 16))
    with pytest.raises(NotImplementedError, match=r"grads\[0\]"):
        call([g[0].double(), g[1].double()], (12, 16))
    with pytest.raises(ValueError, match=r"same dtype: grads\[1\]"):
        call([g[0], g[1].half()], (12, 16))
    with pytest.raises(ValueError, match=r"same K: grads\[1\]"):
        call([g[0], g[1][:3]], (12, 16))
    with pytest.raises(ValueError, match=r"same K: grads\[0\]"):
        call(g, (12, 16), channels=5)
    with pytest.raises(ValueError, match=r"grads\[1\] is empty"):
        call([g[0], g[1][:, :0]], (12, 16))
    with pytest.raises(ValueError, match=r"same device: grads\[1\]"):
        call([g[0], g[1].to("meta")], (12, 16))
    for kw in ({}, {"channels": 7}, {"channels": 7, "dtype": torch.float32}, {"dtype": torch.float32, "device": "cpu"}):
        with pytest.raises(ValueError, match="channels=, dtype= and device="):
            call([None, None], (12, 16), **kw)
    with pytest.raises(ValueError, match="channels="):
        call([], (12, 16))
    with pytest.raises(ValueError, match="K must be"):
        call([], (12, 16), channels=0, dtype=torch.float32)
    with pytest.raises(NotImplementedError, match="dtype"):
        call(g, (12, 16), dtype=torch.float64)
    # the canvas: one pair, or one pair per item
    for canvas in (12, (12,), (12, 16, 3), [(12, 16)], [(12, 16)] * 3):
        with pytest.raises(ValueError, match="canvas"):
            call(g, canvas)
    for canvas in ((0, 16), (12, 16.5), [(12, 16), (12, -1)], [(12, 16), (1 << 20, 1 << 18)]):
        with pytest.raises(ValueError, match=r"canvas\[\d\]"):
            call(g, canvas)
    # regions and flips: the forward's checks, against the canvas
    with pytest.raises(ValueError, match="regions must hold"):
        call(g, (12, 16), regions=[None])
    with pytest.raises(ValueError, match=r"regions\[1\].*four integers"):
        call(g, (12, 16), regions=[None, (0, 0, 3.5, 2)])
    with pytest.raises(ValueError, match=r"regions\[1\].*empty"):
        call(g, (12, 16), regions=[None, (0, 0, 0, 2)])
    for r in ((-1, 0, 3, 3), (0, 0, 13, 3), (10, 0, 3, 3), (0, 14, 3, 3)):
        with pytest.raises(ValueError, match=r"regions\[0\].*inside"):
            call(g, (12, 16), regions=[r, None])
    with pytest.raises(ValueError, match=r"regions\[1\].*inside"):
        call(g, [(12, 16), (4, 4)], regions=[None, (0, 0, 5, 4)])
    with pytest.raises(ValueError, match="flips"):
        call(g, (12, 16), flips=[True])
    # empty input needs no device
    y = call([], (12, 16), channels=7, dtype=torch.bfloat16, out_format="nhwc")
    assert tuple(y.shape) == (0, 7, 12, 16) and y.dtype == torch.bfloat16
    assert call([], [], channels=7, dtype=torch.float32) == []
    # everything in order: only the device is missing
    with pytest.raises(_lib.AAInterpError, match="no CPU implementation"):
        call([g[0], None], [(12, 16), (3, 3)], "lanczos", regions=[(1, 1, 2, 2), None], flips=[True, False], dtype=torch.float16, out_format="nhwc")


def test_forward_that_requires_grad_still_needs_the_device():
    p = torch.zeros(2, 7, 12, 16, requires_grad=True)
    with pytest.raises(_lib.AAInterpError, match="no CPU implementation"):
        aa.resize_many_back(p, [(5, 6), (7, 8)])


# ---- the restatement against its dense float64 form ---------------------------------------------------------------------------------------
_BASE = {}


def base(filt):
    """(oracle.backward's values, the gather form's, float64 values, bounds) of the base case, computed once per filter."""
    if filt not in _BASE:
        gs = ref.grads(ref.BASE_SIZES, ref.BASE_K)
        args = (gs, ref.BASE_HW, ref.BASE_REGIONS, ref.BASE_FLIPS)
        _BASE[filt] = (ref.backward(filt, *args), ref.gather_backward(filt, *args)) + ref.dense_backward(filt, *args)
    return _BASE[filt]


@pytest.mark.parametrize("filt", ref.ORACLE_FILTERS)
def test_restated_values_within_the_dense_bound(filt):
    got, gathered, want, bnd = base(filt)
    assert [g.shape for g in got] == [(ref.BASE_K,) + ref.BASE_HW] * 5 and all(g.dtype == np.float32 for g in got + gathered)
    r, rg = ref.worst_ratio(got, want, bnd), ref.worst_ratio(gathered, want, bnd)
    print(f"backward {filt}: worst err / bound {r:.3f} (oracle.backward), {rg:.3f} (the gather form)")
    assert r <= 1.0 and rg <= 1.0
    # outside the regions: the bits of +0.0; the identity item: the gradient's bits inside
    for i, ((y0, x0, h, w), g, q) in enumerate(zip(ref.BASE_REGIONS, got, gathered)):
        outside = np.ones(ref.BASE_HW, bool)
        outside[y0:y0 + h, x0:x0 + w] = False
        assert not g.view(np.int32)[:, outside].any() and not q.view(np.int32)[:, outside].any(), i
    y0, x0, h, w = ref.BASE_REGIONS[ref.IDENTITY_ITEM]
    gi = ref.grads(ref.BASE_SIZES, ref.BASE_K)[ref.IDENTITY_ITEM]
    for q in (got, gathered):
        assert np.array_equal(q[ref.IDENTITY_ITEM][:, y0:y0 + h, x0:x0 + w].view(np.int32), np.ascontiguousarray(gi).view(np.int32))


@pytest.mark.parametrize("filt", ref.ORACLE_FILTERS)
def test_adjoint_identity_with_the_forward_restatement(filt):
    """<R(x), G> == <x, B(G)> in float64, within the sum of the two bounds."""
    x = fwd_ref.BASE_CANVAS
    gs = ref.grads(ref.BASE_SIZES, ref.BASE_K)
    vals = fwd_ref.values(filt, x, ref.BASE_REGIONS, ref.BASE_SIZES, ref.BASE_FLIPS)
    _, fb = fwd_ref.dense_values(filt, x, ref.BASE_REGIONS, ref.BASE_SIZES, ref.BASE_FLIPS)
    got, gathered, _, bb = base(filt)
    lhs = sum(float((v.astype(np.float64) * g).sum()) for v, g in zip(vals, gs))
    allowed = sum(float((np.abs(g) * b).sum()) for g, b in zip(gs, fb)) + sum(float((np.abs(x[i].astype(np.float64)) * b).sum()) for i, b in enumerate(bb))
    for name, q in (("oracle.backward", got), ("the gather form", gathered)):
        rhs = sum(float((x[i].astype(np.float64) * b).sum()) for i, b in enumerate(q))
        print(f"{filt}, {name}: |{lhs:.9g} - {rhs:.9g}| / {allowed:.3g} = {abs(lhs - rhs) / allowed:.3f}")
        assert abs(lhs - rhs) <= allowed


@pytest.mark.parametrize("filt", ref.FILTERS)
def test_dense_form_has_all_five_filters_and_none_items(filt):
    gs = ref.grads(ref.BASE_SIZES, ref.BASE_K)
    want, bnd = ref.dense_backward(filt, [gs[0], None, gs[2], None, gs[4]], ref.BASE_HW, ref.BASE_REGIONS, ref.BASE_FLIPS)
    full, _ = ref.dense_backward(filt, gs, ref.BASE_HW, ref.BASE_REGIONS, ref.BASE_FLIPS)
    assert all(w.shape == b.shape == (ref.BASE_K,) + ref.BASE_HW and (b >= 0).all() for w, b in zip(want, bnd))
    assert not want[1].any() and not want[3].any() and not bnd[1].any() and np.array_equal(want[0], full[0]) and np.array_equal(want[4], full[4])


def test_further_cases_restated():
    for case in (ref.list_case(), ref.seventy_case(), ref.long_rows_case()):
        canvas, regions, sizes = case
        k = 2 if case[2] == [(5, 3)] else 3
        gs = ref.grads(sizes, k, seed=len(sizes))
        for filt in ("linear", "box"):
            got, gathered = ref.backward(filt, gs, canvas, regions), ref.gather_backward(filt, gs, canvas, regions)
            want, bnd = ref.dense_backward(filt, gs, canvas, regions)
            assert ref.worst_ratio(got, want, bnd) <= 1.0 and ref.worst_ratio(gathered, want, bnd) <= 1.0, (filt, len(sizes))
    # a 100-fold shrink: forward rows of 100 and more floats, adjoint rows of a few
    rows = ref.adjoint_rows("linear", 300, 3)
    assert max(len(w) for _, w in rows) <= 3 and oracle_ksize("linear", 300, 3) >= 200


def oracle_ksize(filt, n_in, n_out):
    import oracle

    return oracle.ksize(filt, n_in, n_out)
