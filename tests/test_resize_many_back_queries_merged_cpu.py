"""resize_many_back_queries(groups=...) without a GPU: the merged planner (host arithmetic only) through ctypes — the block's size and
sections, the workspace as the tables and then the packed weights, the error codes in their order — the Python refusals that come
before any GPU use, and the three symbols."""
import ctypes

import pytest
import torch

from interpolate_antialiasing_amd import _lib
from interpolate_antialiasing_amd import extension_interpolate as aa

ERR_BAD_DTYPE, ERR_BAD_SHAPE, ERR_NULL, ERR_WORKSPACE, ERR_STRIDES = -2, -4, -5, -6, -10
PTR = 4096  # a dummy device address: the planner never follows it
GROUPS, OW = [0, 1, 0, 1, 1], (300, 5)  # group 0: members 0, 2 at (3, 300); group 1: members 1, 3, 4 at (3, 5)


def plan(q=100, c=19, reduce=_lib.BACK_ARGMAX, dtype=_lib.U8, merge=1, groups=GROUPS, g=2, wptr=PTR, sq=19, ow3=None, short=0, weights=True):
    L = _lib.load()
    n = len(groups)
    recs, wts = (_lib.BackItemIn * n)(), (_lib.BackWeightsIn * n)()
    for i, (r, w) in enumerate(zip(recs, wts)):
        r.data_dev, r.stride_ch, r.stride_row, r.stride_px, r.h, r.w, r.oh, r.ow = PTR, 192, 16, 1, 12, 16, 3, OW[groups[i] % 2]
        w.data_dev, w.stride_q, w.stride_c = PTR + 4 * i, sq, 1
    wts[3].data_dev = wptr
    if ow3 is not None:
        recs[3].ow = ow3
    nbytes = L.aa_back_queries_merged_desc_bytes(n, g) - short
    buf = ctypes.create_string_buffer(nbytes + short)
    ws, arena, offs = ctypes.c_size_t(0), ctypes.c_size_t(0), (ctypes.c_int64 * max(g, 1))()
    rc = L.aa_back_queries_merged_plan(0, _lib.NCHW, n, q, c, recs, wts if weights else None, g, (ctypes.c_int64 * n)(*groups), merge, reduce, dtype,
                                       buf, nbytes, ctypes.byref(ws), ctypes.byref(arena), offs)
    return rc, buf, ws.value, arena.value, list(offs), recs


def test_the_block_the_workspace_and_the_planner_errors():
    L = _lib.load()
    size = L.aa_back_queries_merged_desc_bytes
    assert [size(5, 2), size(4, 4), size(0, 0)] == [L.aa_back_merged_desc_bytes(5, 2) + 5 * 32, L.aa_back_merged_desc_bytes(4, 4) + 4 * 32, 72]
    assert size(-1, 0) == 0 and size(1, -1) == 0 and ctypes.sizeof(_lib.BackQueriesMergedHeader) == 64
    rc, buf, ws, arena, offs, recs = plan()
    hd, items, groups, members, unit0, wts = _lib.back_queries_merged_desc_view(buf, 5, 2)
    assert rc == 0 and (hd.n, hd.Q, hd.C, hd.G, hd.merge, hd.reduce, hd.out_dtype) == (5, 100, 19, 2, 1, _lib.BACK_ARGMAX, _lib.U8)
    assert (hd.units, hd.ws_bytes, hd.arena_bytes) == (3 * 2 + 3, ws, arena) and offs == [0, 912] and arena == 912 + 15
    assert list(members) == [0, 2, 1, 3, 4] and list(unit0) == [0, 6, 9]
    assert [(g.first, g.count, g.oh, g.ow, g.xtiles, g.out_off) for g in groups] == [(0, 2, 3, 300, 2, 0), (2, 3, 3, 5, 1, 912)]
    assert [(it.oh, it.ow, it.out_off) for it in items] == [(3, (300, 5)[g], (0, 912)[g]) for g in GROUPS]
    assert [(w.w, w.stride_q, w.stride_c) for w in wts] == [(PTR if i == 3 else PTR + 4 * i, 19, 1) for i in range(5)]
    # the workspace: aa_back_merged_plan's tables for the same members (K = Q), rounded up to 16 bytes, then Cpad * Qpad float16 a member
    mbuf = ctypes.create_string_buffer(L.aa_back_merged_desc_bytes(5, 2))
    tables, marena, moffs = ctypes.c_size_t(0), ctypes.c_size_t(0), (ctypes.c_int64 * 2)()
    assert L.aa_back_merged_plan(0, _lib.NCHW, 5, 100, recs, 2, (ctypes.c_int64 * 5)(*GROUPS), 0, _lib.BACK_ARGMAX, _lib.U8, mbuf, len(mbuf),
                                 ctypes.byref(tables), ctypes.byref(marena), moffs) == 0
    assert tables.value > 0 and ws == (tables.value + 15) // 16 * 16 + 5 * 32 * 112 * 2
    assert [(it.tab_h, it.tab_w) for it in items] == [(it.tab_h, it.tab_w) for it in _lib.back_merged_desc_view(mbuf, 5, 2)[1]]
    assert plan(q=16, c=33)[2] - plan(q=16, c=32)[2] == 5 * 32 * 16 * 2 and plan(q=17, c=32)[2] - plan(q=16, c=32)[2] == 5 * 32 * 16 * 2
    rc, _, _, arena, offs, _ = plan(reduce=_lib.BACK_VALUES, dtype=_lib.F16, merge=0)
    assert rc == 0 and offs == [0, 19 * 900 * 2 + 8] and arena == offs[1] + 19 * 15 * 2
    # the statuses, each with everything before it in order
    assert plan(q=257)[0] == ERR_BAD_SHAPE and plan(c=0)[0] == ERR_BAD_SHAPE and plan(reduce=_lib.BACK_GREATER)[0] == ERR_BAD_SHAPE
    assert plan(merge=2)[0] == ERR_BAD_SHAPE and plan(g=6)[0] == ERR_BAD_SHAPE and plan(g=0)[0] == ERR_BAD_SHAPE
    assert plan(c=257)[0] == ERR_BAD_SHAPE and plan(c=257, dtype=_lib.I16)[0] == 0  # (a label type too small for C)
    assert plan(weights=False)[0] == ERR_NULL and plan(weights=False, c=257)[0] == ERR_BAD_SHAPE
    assert plan(short=1)[0] == ERR_WORKSPACE and plan(short=1, weights=False)[0] == ERR_NULL
    assert plan(groups=[0, 2, 0, 1, 1])[0] == ERR_BAD_SHAPE and plan(groups=[0, 0, 0, 0, 0])[0] == ERR_BAD_SHAPE  # (outside 0 .. G - 1; empty)
    assert plan(ow3=7)[0] == ERR_BAD_SHAPE and plan(ow3=7, wptr=None)[0] == ERR_BAD_SHAPE  # (the member's size comes before its weights)
    assert plan(wptr=None)[0] == ERR_NULL and plan(wptr=PTR + 2)[0] == ERR_STRIDES and plan(sq=-1)[0] == ERR_STRIDES
    assert plan(dtype=_lib.F32)[0] == ERR_BAD_DTYPE and plan(dtype=_lib.F32, sq=-1)[0] == ERR_STRIDES


def test_the_refusals_that_need_no_gpu():
    x, w = torch.zeros(4, 5, 6, 7), torch.zeros(4, 5, 3)
    for kw, words in ((dict(groups=[0, 1, 0]), "one entry per item"), (dict(groups=[0, 0, 0, 0]), "group 1 .* has no member"),
                      (dict(groups=[0, 1, 2, 0]), r"groups\[2\] = 2 is outside"), (dict(groups=[0, 1, 0, 1], merge="max"), "merge must be"),
                      (dict(merge="mean"), "needs groups"), (dict(groups=[0, 1, 0, 1], sizes=[(8, 9)] * 4), "group 2 .* has no member")):
        with pytest.raises(ValueError, match=words):
            aa.resize_many_back_queries(x, w, **{"sizes": [(8, 9), (3, 4)], **kw})
    with pytest.raises(NotImplementedError, match="not differentiable"):
        aa.resize_many_back_queries(x.requires_grad_(), w, [(8, 9), (3, 4)], groups=[0, 1, 0, 1], reduce=None)
    assert aa.resize_many_back_queries([], [], [], groups=[], merge="mean") == []


def test_abi_is_additive():
    L = _lib.load()
    assert L.aa_abi_version() == 3
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    for sym in ("aa_back_queries_merged_desc_bytes", "aa_back_queries_merged_plan", "aa_resample_back_queries_merged"):
        assert sym in _lib.EXPORTS and hasattr(L, sym) and sym + "(" in header
        assert sym in header.split("#define AA_INTERP_ABI_VERSION 3")[1].split("*/")[0]  # (listed in the version's comment)
