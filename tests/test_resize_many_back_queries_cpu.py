"""resize_many_back_queries without a GPU: the planner (host arithmetic only) through ctypes — the block's size, its records, the error
codes — and the reference's own sanity."""
import ctypes

import numpy as np

import resize_many_back_queries_ref as ref
from interpolate_antialiasing_amd import _lib

ERR_BAD_DTYPE, ERR_BAD_SHAPE, ERR_NULL, ERR_STRIDES = -2, -4, -5, -10
PTR = 4096  # a dummy device address: the planner never follows it


def plan(q=100, c=19, reduce=_lib.BACK_ARGMAX, dtype=_lib.U8, wptr=PTR, sq=19, sc=1):
    L = _lib.load()
    recs, wts = (_lib.BackItemIn * 2)(), (_lib.BackWeightsIn * 2)()
    for r, w, ow in zip(recs, wts, (300, 5)):
        r.data_dev, r.stride_ch, r.stride_row, r.stride_px, r.h, r.w, r.oh, r.ow = PTR, 192, 16, 1, 12, 16, 3, ow
        w.data_dev, w.stride_q, w.stride_c = wptr, sq, sc
    nbytes = L.aa_back_queries_desc_bytes(2)
    buf = ctypes.create_string_buffer(nbytes)
    ws, arena, offs = ctypes.c_size_t(0), ctypes.c_size_t(0), (ctypes.c_int64 * 2)()
    rc = L.aa_back_queries_plan(0, _lib.NCHW, 2, q, c, recs, wts, reduce, dtype, buf, nbytes, ctypes.byref(ws), ctypes.byref(arena), offs)
    return rc, buf, arena.value, list(offs)


def test_the_block_and_the_planner_errors():
    L = _lib.load()
    size = lambda n: ctypes.sizeof(_lib.BackQueriesHeader) + n * (ctypes.sizeof(_lib.BackItem) + ctypes.sizeof(_lib.BackQueryWeights)) + 8 * (n + 1)
    assert [L.aa_back_queries_desc_bytes(n) for n in (0, 2, 70)] == [size(0), size(2), size(70)]
    rc, buf, arena, offs = plan()
    hd = _lib.BackQueriesHeader.from_buffer(buf, 0)
    assert rc == 0 and (hd.n, hd.Q, hd.C, hd.units) == (2, 100, 19, 3 * 2 + 3) and offs == [0, 912] and arena == 912 + 15
    wts = (_lib.BackQueryWeights * 2).from_buffer(buf, size(2) - 2 * ctypes.sizeof(_lib.BackQueryWeights))
    assert all((w.w, w.stride_q, w.stride_c) == (PTR, 19, 1) for w in wts)
    rc, _, arena, offs = plan(reduce=_lib.BACK_VALUES, dtype=_lib.F16)
    assert rc == 0 and offs == [0, 19 * 900 * 2 + 8] and arena == offs[1] + 19 * 15 * 2
    assert plan(q=257)[0] == ERR_BAD_SHAPE and plan(q=256)[0] == 0 and plan(c=0)[0] == ERR_BAD_SHAPE and plan(reduce=_lib.BACK_GREATER)[0] == ERR_BAD_SHAPE
    assert plan(c=257)[0] == ERR_BAD_SHAPE and plan(c=257, dtype=_lib.I16)[0] == 0  # (a label type too small for C)
    assert plan(dtype=_lib.F32)[0] == ERR_BAD_DTYPE and plan(reduce=_lib.BACK_VALUES)[0] == ERR_BAD_DTYPE
    assert plan(wptr=None)[0] == ERR_NULL and plan(wptr=PTR + 2)[0] == ERR_STRIDES and plan(sq=-1)[0] == ERR_STRIDES


def test_the_bound_holds_for_an_fp32_accumulation():
    """The reference's sanity: numpy's own float32 sum of the same exact products lies within the bound, and above a hundredth of it
    somewhere (the bound is not idle)."""
    rng = np.random.default_rng(3)
    R, w = rng.uniform(-8, 8, (37, 9, 11)).astype(np.float32), ref.weights(1, 37, 35)[0]
    want, bnd = ref.scores(R, w)
    p, wh = ref.operands(R, w)
    got = np.zeros(want.shape, np.float32)
    for q in range(37):
        got = got + (wh[q].astype(np.float32)[:, None, None] * p[q].astype(np.float32)[None])
    ratio = np.abs(got - want) / bnd
    assert ratio.max() <= 1.0 and ratio.max() > 0.01
    ok, arg = ref.decided([want], [bnd])
    assert ok[0].mean() >= 0.9 and (np.argmax(got, 0)[ok[0]] == arg[0][ok[0]]).all()
