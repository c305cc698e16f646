"""resize_embed_to_tokens without a GPU: the planner (host arithmetic only), the argument errors that come before any device work, and
the CPU restatement of the definition (resize_embed_ref) against the dense float64 forms."""
import ctypes

import numpy as np
import pytest
import torch

import resize_embed_ref as ref
from interpolate_antialiasing_amd import _lib
from interpolate_antialiasing_amd import extension_interpolate as aa

ERR_BAD_FILTER, ERR_BAD_SHAPE, ERR_NULL, ERR_WORKSPACE = -1, -4, -5, -6
MAX = (2 ** 31 - 1) // 4
ORACLE_FILTERS = ("linear", "cubic", "box")


def plan(grids, d=8, h0=5, w0=7, filt=_lib.FILTER_CUBIC, pad_to=0, n=None, desc=True, short=0):
    L = _lib.load()
    n = len(grids) if n is None else n
    nbytes = L.aa_embed_many_desc_bytes(max(n, 0)) - short
    buf = (ctypes.c_uint8 * max(nbytes, 64))()
    flat = (ctypes.c_int64 * max(2 * len(grids), 1))(*[v for g in grids for v in g])
    ws, rows = ctypes.c_size_t(0), ctypes.c_int64(-1)
    rc = L.aa_embed_many_plan(filt, n, d, h0, w0, flat if grids or n <= 0 else None, pad_to, ctypes.addressof(buf) if desc else None, nbytes,
                              ctypes.byref(ws), ctypes.byref(rows))
    return rc, buf, ws.value, rows.value


# ---- the planner ----------------------------------------------------------------------------------------------------------------------
def test_abi_is_additive():
    L = _lib.load()
    assert L.aa_abi_version() == 3
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    for sym in ("aa_embed_many_desc_bytes", "aa_embed_many_plan", "aa_resample_embed_many", "aa_resample_embed_many_bwd"):
        assert sym in _lib.EXPORTS and hasattr(L, sym) and sym + "(" in header
    assert ctypes.sizeof(_lib.EmbedHeader) == 64 and ctypes.sizeof(_lib.EmbedItem) == 64
    assert L.aa_embed_many_desc_bytes(3) == 64 + 3 * 64 + 4 * 8 and L.aa_embed_many_desc_bytes(-1) == 0


def test_plan_rows_prefix_and_records():
    L = _lib.load()
    grids = ref.BASE_GRIDS
    rc, buf, ws, rows = plan(grids)
    assert rc == 0
    hd, items, prefix = _lib.embed_desc_view(buf, len(grids))
    assert list(prefix) == ref.offsets(grids) and rows == prefix[len(grids)] == hd.out_rows
    assert (hd.n, hd.D, hd.H0, hd.W0, hd.filter, hd.pad_to, hd.ws_bytes) == (len(grids), 8, 5, 7, _lib.FILTER_CUBIC, 0, ws)
    end = 0
    for it, (gh, gw) in zip(items, grids):
        assert (it.gh, it.gw) == (gh, gw)
        assert it.ksize_h == L.aa_table_ksize(_lib.FILTER_CUBIC, _lib.TABLE_F32, 5, gh, 0, 0.0)
        assert it.ksize_w == L.aa_table_ksize(_lib.FILTER_CUBIC, _lib.TABLE_F32, 7, gw, 0, 0.0)
        assert it.trk_h == L.aa_table_transposed_ksize(_lib.FILTER_CUBIC, _lib.TABLE_F32, 5, gh, 0, 0.0)
        assert it.trk_w == L.aa_table_transposed_ksize(_lib.FILTER_CUBIC, _lib.TABLE_F32, 7, gw, 0, 0.0)
        assert it.scale_h == np.float32(5) / np.float32(gh) and it.scale_w == np.float32(7) / np.float32(gw)
        # four tables one after the other, 16-byte aligned, none overlapping: header, xmin, xsize, rows of floats
        sizes = [(gh, it.ksize_h), (gw, it.ksize_w), (5, it.trk_h), (7, it.trk_w)]
        for off, (out, k) in zip((it.tab_h, it.tab_w, it.tr_h, it.tr_w), sizes):
            assert off == end and off % 16 == 0
            end = off + ((((64 + 8 * out + 15) & ~15) + 4 * out * k + 15) & ~15)
    assert end == ws


def test_plan_pad_to():
    grids = ref.BASE_GRIDS
    longest = max(gh * gw for gh, gw in grids)
    rc, buf, _, rows = plan(grids, pad_to=longest)
    assert rc == 0 and rows == len(grids) * longest
    hd, _, prefix = _lib.embed_desc_view(buf, len(grids))
    assert hd.pad_to == longest and hd.out_rows == rows and list(prefix) == ref.offsets(grids)  # (the prefix stays the packed one)
    assert plan(grids, pad_to=longest - 1)[0] == ERR_BAD_SHAPE
    assert plan(grids, pad_to=-1)[0] == ERR_BAD_SHAPE


def test_plan_empty():
    rc, buf, ws, rows = plan([])
    assert (rc, ws, rows) == (0, 0, 0)
    rc, _, _, rows = plan([], pad_to=9)
    assert (rc, rows) == (0, 0)


@pytest.mark.parametrize("grids", [[(0, 3)], [(3, 0)], [(2, 2), (-1, 2)], [(MAX + 1, 1)], [(1, MAX + 1)], [(65536, 65536)]])
def test_plan_refuses_a_grid(grids):
    assert plan(grids)[0] == ERR_BAD_SHAPE


def test_plan_error_codes():
    L = _lib.load()
    ok = [(2, 3)]
    assert plan(ok, n=-1)[0] == ERR_BAD_SHAPE
    assert plan(ok, d=0)[0] == ERR_BAD_SHAPE and plan(ok, h0=0)[0] == ERR_BAD_SHAPE and plan(ok, w0=MAX + 1)[0] == ERR_BAD_SHAPE
    assert plan(ok, filt=5)[0] == ERR_BAD_FILTER
    assert plan(ok, desc=False)[0] == ERR_NULL
    assert plan(ok, short=1)[0] == ERR_WORKSPACE
    buf = (ctypes.c_uint8 * 256)()
    ws, rows = ctypes.c_size_t(0), ctypes.c_int64(0)
    flat = (ctypes.c_int64 * 2)(2, 3)
    assert L.aa_embed_many_plan(1, 1, 8, 5, 7, None, 0, ctypes.addressof(buf), 256, ctypes.byref(ws), ctypes.byref(rows)) == ERR_NULL
    assert L.aa_embed_many_plan(1, 1, 8, 5, 7, flat, 0, ctypes.addressof(buf), 256, None, ctypes.byref(rows)) == ERR_NULL
    assert L.aa_embed_many_plan(1, 1, 8, 5, 7, flat, 0, ctypes.addressof(buf), 256, ctypes.byref(ws), None) == ERR_NULL
    # the launches check the block and their pointers before anything is enqueued (no device is touched)
    one = ctypes.c_void_p(256)
    assert L.aa_resample_embed_many(None, one, one, _lib.F32, 56, 8, one, _lib.F32, one, 1 << 20, None) == ERR_NULL
    assert L.aa_resample_embed_many(ctypes.addressof(buf), one, one, _lib.F32, 56, 8, one, _lib.F32, one, 1 << 20, None) == ERR_BAD_SHAPE  # no plan's block
    assert L.aa_embed_many_plan(1, 1, 8, 5, 7, flat, 0, ctypes.addressof(buf), 256, ctypes.byref(ws), ctypes.byref(rows)) == 0
    assert L.aa_resample_embed_many(ctypes.addressof(buf), one, one, _lib.F64, 56, 8, one, _lib.F32, one, 1 << 20, None) == -2  # AA_ERR_BAD_DTYPE
    assert L.aa_resample_embed_many(ctypes.addressof(buf), one, one, _lib.F32, 56, 8, one, _lib.U8, one, 1 << 20, None) == -2
    assert L.aa_resample_embed_many(ctypes.addressof(buf), one, None, _lib.F32, 56, 8, one, _lib.F32, one, 1 << 20, None) == ERR_NULL
    assert L.aa_resample_embed_many(ctypes.addressof(buf), one, one, _lib.F32, 56, 8, one, _lib.F32, one, ws.value - 1, None) == ERR_WORKSPACE
    assert L.aa_resample_embed_many(ctypes.addressof(buf), one, one, _lib.F32, -56, 8, one, _lib.F32, one, 1 << 20, None) == _lib.ERR_STRIDES
    assert L.aa_resample_embed_many_bwd(ctypes.addressof(buf), one, None, _lib.F32, one, _lib.F32, one, 1 << 20, None) == ERR_NULL
    assert L.aa_resample_embed_many_bwd(ctypes.addressof(buf), one, one, _lib.F32, ctypes.c_void_p(258), _lib.F32, one, 1 << 20, None) == ERR_BAD_SHAPE


# ---- argument errors of the Python calls, before any device work ------------------------------------------------------------------------
def test_argument_errors():
    e = torch.zeros(5, 7, 8)
    with pytest.raises(NotImplementedError):
        aa.resize_embed_to_tokens(e.double(), [(2, 3)])
    with pytest.raises(NotImplementedError):
        aa.resize_embed_to_tokens(e, [(2, 3)], out_dtype=torch.float64)
    with pytest.raises(_lib.AAInterpError, match="no CPU implementation"):
        aa.resize_embed_to_tokens(e, [(2, 3)])
    with pytest.raises(ValueError, match="stride"):
        aa.resize_embed_to_tokens(torch.zeros(8, 5, 7).permute(1, 2, 0), [(2, 3)])
    with pytest.raises(ValueError):
        aa.resize_embed_to_tokens(e, [(2, 3)], mode="area")
    with pytest.raises(ValueError, match="pad_to"):
        aa.resize_embed_to_tokens(e, [(2, 3), (3, 3)], pad_to=8)
    with pytest.raises(ValueError):
        aa.resize_embed_to_tokens(e, [(0, 3)])
    with pytest.raises(ValueError):
        aa.resize_embed_to_tokens(e[0], [(2, 3)])
    g = torch.zeros(6, 8)
    with pytest.raises(NotImplementedError):
        aa.resize_embed_to_tokens_backward(g.double(), (5, 7, 8), [(2, 3)])
    with pytest.raises(NotImplementedError):
        aa.resize_embed_to_tokens_backward(g, (5, 7, 8), [(2, 3)], dtype=torch.float64)
    with pytest.raises(ValueError, match="expected"):
        aa.resize_embed_to_tokens_backward(g, (5, 7, 8), [(2, 4)])
    with pytest.raises(ValueError, match="pad_to"):
        aa.resize_embed_to_tokens_backward(torch.zeros(1, 5, 8), (5, 7, 8), [(2, 3)], pad_to=5)
    with pytest.raises(_lib.AAInterpError, match="no CPU implementation"):
        aa.resize_embed_to_tokens_backward(g, (5, 7, 8), [(2, 3)])


# ---- the restatement against the dense float64 forms ----------------------------------------------------------------------------------
CASES = [("base", ref.BASE_SOURCE, ref.BASE_GRIDS)] + [(k,) + v for k, v in ref.FURTHER.items()]


@pytest.mark.parametrize("filt", ORACLE_FILTERS)
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restated_forward_within_the_dense_bound(filt, case):
    _, (h0, w0), grids = case
    e = ref.embed_values(h0, w0, 6)
    got = ref.packed_forward(filt, e, grids)
    want, bnd = ref.dense_forward(filt, e, grids)
    assert got.shape == want.shape and got.dtype == np.float32
    r = ref.worst_ratio(got, want, bnd)
    print(f"forward {filt} {case[0]}: worst err / bound {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("filt", ORACLE_FILTERS)
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restated_backward_within_the_dense_bound(filt, case):
    _, (h0, w0), grids = case
    g = ref.grad_values(grids, 6)
    got = ref.ordered_backward(filt, g, (h0, w0, 6), grids)
    want, bnd = ref.dense_backward(filt, g, (h0, w0, 6), grids)
    assert got.shape == want.shape == (h0, w0, 6) and got.dtype == np.float32
    r = ref.worst_ratio(got, want, bnd)
    print(f"backward {filt} {case[0]}: worst err / bound {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("filt", ORACLE_FILTERS)
def test_the_identity_item_is_a_copy(filt):
    e = ref.embed_values(5, 7, 6)
    got = ref.item_forward(filt, e, (5, 7))
    assert np.array_equal(got.view(np.int32), e.reshape(35, 6).view(np.int32))


def test_pad_rows_and_empty():
    e = ref.embed_values(5, 7, 3)
    p = ref.packed_forward("cubic", e, [(2, 3), (1, 1)], pad_to=7)
    assert p.shape == (2, 7, 3) and not p[0, 6:].any() and not p[1, 1:].any() and not np.signbit(p[1, 1:]).any()
    assert ref.packed_forward("cubic", e, []).shape == (0, 3)
    assert not ref.ordered_backward("cubic", np.zeros((0, 3), np.float32), (5, 7, 3), []).any()
