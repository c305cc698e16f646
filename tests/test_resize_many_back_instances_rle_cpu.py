"""resize_many_back_instances_rle without a GPU: the reference on cases worked by hand, the planner (host arithmetic only) through
ctypes — the block's fields, its offsets, the error codes — the Python refusals that come before any launch, and boxmath.coco_rles."""
import ctypes

import numpy as np
import pytest
import torch

import resize_many_back_instances_rle_ref as ref
from interpolate_antialiasing_amd import _lib, boxmath
from interpolate_antialiasing_amd import extension_interpolate as aa

ERR_BAD_SHAPE, ERR_NULL, ERR_STRIDES, ERR_WORKSPACE = -4, -5, -10, -6
PTR = 4096  # a dummy device address: the planner never follows it
OUTS = ((23, 300), (3, 5))


@pytest.mark.parametrize("mask,counts", (([[0, 1], [1, 1]], [1, 3]), (np.zeros((2, 3)), [6]), (np.ones((2, 3)), [0, 6]),
                                         ([[0, 1, 0], [1, 1, 0]], [1, 3, 2]),  # the run from (1, 0) crosses into column 1
                                         ([[1, 0, 0, 1], [0, 0, 1, 1], [1, 0, 1, 1]], [0, 1, 1, 1, 4, 5])))
def test_the_reference_on_cases_worked_by_hand(mask, counts):
    mask = np.array(mask, bool)
    assert ref.rle(mask) == counts and sum(counts) == mask.size
    back = np.repeat(np.arange(len(counts)) % 2 == 1, counts).reshape(mask.shape[::-1]).T  # decoded: the odd runs are the ones
    assert (back == mask).all()
    runs, nruns = ref.rows([mask, mask], 3)
    assert nruns.tolist() == [len(counts)] * 2 and runs[1].tolist() == (counts + [0, 0])[:3]


def plan(q=100, m=7, max_runs=64, filt=0, ptr=PTR, stride_px=1, short=0, outs=OUTS, n=2):
    L = _lib.load()
    recs = (_lib.BackItemIn * 2)()
    for r, (oh, ow) in zip(recs, outs):
        r.data_dev, r.stride_ch, r.stride_row, r.stride_px, r.h, r.w, r.oh, r.ow = ptr, 192, 16, stride_px, 12, 16, oh, ow
    nbytes = L.aa_back_instances_rle_desc_bytes(n) - short
    buf = ctypes.create_string_buffer(nbytes + short)
    ws, arena, n_off, s_off = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_int64(0), ctypes.c_int64(0)
    rc = L.aa_back_instances_rle_plan(filt, _lib.NCHW, n, q, m, recs, max_runs, buf, nbytes, ctypes.byref(ws), ctypes.byref(arena), ctypes.byref(n_off),
                                      ctypes.byref(s_off))
    return rc, buf, ws.value, arena.value, n_off.value, s_off.value


@pytest.mark.parametrize("q,m", ((100, 7), (3, 7)))
def test_the_block_and_the_planner_errors(q, m):
    L = _lib.load()
    size = lambda n: ctypes.sizeof(_lib.BackInstancesRleHeader) + n * ctypes.sizeof(_lib.BackItem) + 8 * (n + 1)
    assert ctypes.sizeof(_lib.BackInstancesRleHeader) == 104 and [L.aa_back_instances_rle_desc_bytes(n) for n in (0, 2, 70)] == [size(0), size(2), size(70)]
    rc, buf, ws, arena, n_off, s_off = plan(q=q, m=m)
    hd = _lib.BackInstancesRleHeader.from_buffer(buf, 0)
    units = [-(-oh // _lib.BACK_INSTANCES_ROWS) * -(-ow // _lib.BACK_TILE) for oh, ow in OUTS]
    assert rc == 0 and (hd.n, hd.Q, hd.M, hd.max_runs, hd.units, hd.max_ow) == (2, q, m, 64, sum(units), 300)
    assert list((ctypes.c_int64 * 3).from_buffer(buf, size(2) - 24)) == [0, units[0], sum(units)]
    up16 = lambda v: -(-v // 16) * 16
    # the workspace: the tables, the instance call's work lists, then min(Q, M) planes [oh][ceil(ow / 64)] of 8-byte words per item
    words = up16(4 * (2 + 2 * q + m)) // 4
    planes = [min(q, m) * oh * -(-ow // 64) * 8 for oh, ow in OUTS]
    assert hd.list_words == words and hd.lists_off == up16(hd.tables_bytes) and hd.planes_off == up16(hd.lists_off + 2 * words * 4)
    items = (_lib.BackItem * 2).from_buffer(buf, ctypes.sizeof(_lib.BackInstancesRleHeader))
    assert [it.out_off for it in items] == [0, up16(planes[0])] and ws == hd.planes_off + up16(planes[0]) + planes[1] == hd.ws_bytes
    # the arena: runs, nruns, stats
    assert n_off == up16(2 * m * 64 * 4) == hd.nruns_off and s_off == up16(n_off + 2 * m * 4) == hd.stats_off
    assert arena == s_off + 2 * m * 6 * 8 == hd.arena_bytes
    # the statuses, in the planner's order
    assert plan(filt=99, q=0)[0] == -1 and [plan(q=v)[0] for v in (0, 257, 256)] == [ERR_BAD_SHAPE, ERR_BAD_SHAPE, 0]
    assert [plan(m=v)[0] for v in (0, 257, 256)] == [ERR_BAD_SHAPE, ERR_BAD_SHAPE, 0]
    assert [plan(max_runs=v, ptr=None)[0] for v in (0, -1, (1 << 20) + 1)] == [ERR_BAD_SHAPE] * 3 and plan(max_runs=1 << 20)[0] == 0
    assert plan(short=8, ptr=None)[0] == ERR_WORKSPACE and plan(ptr=None)[0] == ERR_NULL and plan(stride_px=2)[0] == ERR_STRIDES
    # the widest item the scan's LDS holds; flat positions are int32
    assert plan(outs=((23, 4096), (3, 5)))[0] == 0 and plan(outs=((23, 4097), (3, 5)))[0] == ERR_BAD_SHAPE
    assert plan(q=1, outs=((1 << 19, 4095), (3, 5)))[0] == 0 and plan(q=1, outs=((1 << 19, 4096), (3, 5)))[0] == ERR_BAD_SHAPE
    rc, buf, ws, arena, n_off, s_off = plan(n=0)
    assert (rc, arena, n_off, s_off) == (0, 0, 0, 0) and _lib.BackInstancesRleHeader.from_buffer(buf, 0).units == 0


def test_the_refusals_before_any_launch():
    x, qs = torch.zeros(2, 5, 4, 4), torch.zeros(2, 3, dtype=torch.int64)
    for bad, words in ((dict(q=torch.zeros(2, 3)), "queries must be torch.int32 or torch.int64"), (dict(q=qs[0]), r"queries must be \[N, M\] = \[2, M\]"),
                       (dict(q=torch.zeros(2, 257, dtype=torch.int32)), "M must be in 1 .. 256"), (dict(x=torch.zeros(2, 257, 4, 4)), "Q must be in 1 .. 256"),
                       (dict(max_runs=0), "max_runs must be an int in 1 .. 1048576"), (dict(max_runs=(1 << 20) + 1), "max_runs must be"),
                       (dict(max_runs=8.0), "max_runs must be"), (dict(max_runs=True), "max_runs must be"), (dict(max_runs=None), "max_runs must be")):
        kw = {"x": x, "q": qs, "max_runs": 8, **bad}
        with pytest.raises(ValueError, match=words):
            aa.resize_many_back_instances_rle(kw.pop("x"), kw.pop("q"), [(3, 3), (4, 5)], **kw)
    with pytest.raises(TypeError, match="max_runs"):
        aa.resize_many_back_instances_rle(x, qs, [(3, 3), (4, 5)])
    with pytest.raises(NotImplementedError, match=r"torch\.no_grad\(\).*\.detach\(\)"):
        aa.resize_many_back_instances_rle(x.clone().requires_grad_(), qs, [(3, 3), (4, 5)], max_runs=8)
    runs, nruns, stats = aa.resize_many_back_instances_rle([], torch.zeros(0, 3, dtype=torch.int32), [], max_runs=8)
    assert (tuple(runs.shape), tuple(nruns.shape), tuple(stats.shape)) == ((0, 3, 8), (0, 3), (0, 3, 6))
    assert (runs.dtype, nruns.dtype, stats.dtype) == (torch.int32, torch.int32, torch.int64) and "resize_many_back_instances_rle" in aa.__all__


def test_coco_rles():
    masks = [np.array([[[0, 1], [1, 1]], [[0, 0], [0, 0]]], bool), np.array([[[1, 1, 1]], [[0, 1, 0]]], bool)]
    pairs = [ref.rows(m, 4) for m in masks]
    runs, nruns = torch.from_numpy(np.stack([r for r, _ in pairs])), torch.from_numpy(np.stack([k for _, k in pairs]))
    got = boxmath.coco_rles(runs, nruns, [(2, 2), (1, 3)])
    assert got == [[{"size": [2, 2], "counts": [1, 3]}, {"size": [2, 2], "counts": [4]}],
                   [{"size": [1, 3], "counts": [0, 3]}, {"size": [1, 3], "counts": [1, 1, 1]}]]
    with pytest.raises(ValueError, match="item 1 slot 1 has 3 runs"):
        boxmath.coco_rles(runs[:, :, :2], nruns, [(2, 2), (1, 3)])
