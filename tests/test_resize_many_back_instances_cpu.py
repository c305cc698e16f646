"""resize_many_back_instances without a GPU: the planner (host arithmetic only) through ctypes — the block's size, its prefix and
offsets, the error codes in their order — the Python refusals that come before any launch, and the reference on a case worked by hand."""
import ctypes

import numpy as np
import pytest
import torch

import resize_many_back_instances_ref as ref
from interpolate_antialiasing_amd import _lib, boxmath
from interpolate_antialiasing_amd import extension_interpolate as aa

ERR_BAD_SHAPE, ERR_NULL, ERR_STRIDES, ERR_WORKSPACE = -4, -5, -10, -6
PTR = 4096  # a dummy device address: the planner never follows it
OUTS = ((23, 300), (3, 5))


def plan(q=100, m=7, bits=0, filt=0, ptr=PTR, stride_px=1, short=0, outs=OUTS):
    L = _lib.load()
    recs = (_lib.BackItemIn * 2)()
    for r, (oh, ow) in zip(recs, outs):
        r.data_dev, r.stride_ch, r.stride_row, r.stride_px, r.h, r.w, r.oh, r.ow = ptr, 192, 16, stride_px, 12, 16, oh, ow
    nbytes = L.aa_back_instances_desc_bytes(2) - short
    buf = ctypes.create_string_buffer(nbytes + short)
    ws, arena, offs, s_off = ctypes.c_size_t(0), ctypes.c_size_t(0), (ctypes.c_int64 * 2)(), ctypes.c_int64(0)
    rc = L.aa_back_instances_plan(filt, _lib.NCHW, 2, q, m, recs, bits, buf, nbytes, ctypes.byref(ws), ctypes.byref(arena), offs, ctypes.byref(s_off))
    return rc, buf, ws.value, arena.value, list(offs), s_off.value


@pytest.mark.parametrize("bits", (0, 1))
def test_the_block_and_the_planner_errors(bits):
    L = _lib.load()
    size = lambda n: ctypes.sizeof(_lib.BackInstancesHeader) + n * ctypes.sizeof(_lib.BackItem) + 8 * (n + 1)
    assert ctypes.sizeof(_lib.BackInstancesHeader) == 80 and [L.aa_back_instances_desc_bytes(n) for n in (0, 2, 70)] == [size(0), size(2), size(70)]
    rc, buf, ws, arena, offs, s_off = plan(bits=bits)
    hd = _lib.BackInstancesHeader.from_buffer(buf, 0)
    units = [-(-oh // _lib.BACK_INSTANCES_ROWS) * -(-ow // _lib.BACK_TILE) for oh, ow in OUTS]
    assert rc == 0 and (hd.n, hd.Q, hd.M, hd.bits, hd.units) == (2, 100, 7, bits, sum(units)) and units == [6, 1]
    assert list((ctypes.c_int64 * 3).from_buffer(buf, size(2) - 24)) == [0, units[0], sum(units)]
    mask_bytes = [7 * oh * (-(-ow // 8) if bits else ow) for oh, ow in OUTS]
    up16 = lambda v: -(-v // 16) * 16
    assert offs == [0, up16(mask_bytes[0])] and s_off == up16(offs[1] + mask_bytes[1]) and arena == s_off + 2 * 7 * 6 * 8 == hd.arena_bytes
    assert hd.list_words == 212 and hd.lists_off == up16(hd.tables_bytes) and ws == hd.lists_off + 2 * 212 * 4 == hd.ws_bytes
    # the statuses, in the planner's order
    assert plan(filt=99, q=0)[0] == -1 and [plan(q=v)[0] for v in (0, 257, 256)] == [ERR_BAD_SHAPE, ERR_BAD_SHAPE, 0]
    assert [plan(m=v)[0] for v in (0, 257, 256)] == [ERR_BAD_SHAPE, ERR_BAD_SHAPE, 0] and plan(bits=2, ptr=None)[0] == ERR_BAD_SHAPE
    assert plan(short=8, ptr=None)[0] == ERR_WORKSPACE and plan(ptr=None)[0] == ERR_NULL and plan(stride_px=2)[0] == ERR_STRIDES
    # (Q * oh * ow passes the item's own check; M * oh * ow = 2^40 is the last that passes)
    assert plan(q=1, m=256, outs=((1 << 20, 1 << 12), (3, 5)))[0] == 0 and plan(q=1, m=256, outs=((1 << 20, (1 << 12) + 16), (3, 5)))[0] == ERR_BAD_SHAPE


def test_the_refusals_before_any_launch():
    x, qs = torch.zeros(2, 5, 4, 4), torch.zeros(2, 3, dtype=torch.int64)
    for bad, words in ((dict(q=torch.zeros(2, 3)), "queries must be torch.int32 or torch.int64"), (dict(q=qs[0]), r"queries must be \[N, M\] = \[2, M\]"),
                       (dict(q=qs[:1]), r"queries must be \[N, M\]"), (dict(q=torch.zeros(2, 257, dtype=torch.int32)), "M must be in 1 .. 256"),
                       (dict(x=torch.zeros(2, 257, 4, 4)), "Q must be in 1 .. 256"), (dict(mask_format="rle"), "mask_format must be")):
        kw = {"x": x, "q": qs, **bad}
        with pytest.raises(ValueError, match=words):
            aa.resize_many_back_instances(kw.pop("x"), kw.pop("q"), [(3, 3), (4, 5)], **kw)
    with pytest.raises(NotImplementedError, match=r"torch\.no_grad\(\).*\.detach\(\)"):
        aa.resize_many_back_instances(x.clone().requires_grad_(), qs, [(3, 3), (4, 5)])
    masks, stats = aa.resize_many_back_instances([], torch.zeros(0, 3, dtype=torch.int32), [])
    assert masks == [] and tuple(stats.shape) == (0, 3, 6) and stats.dtype == torch.int64


def test_the_reference_on_a_case_worked_by_hand():
    """Two queries on 2 x 9 pixels, five slots: query 1 twice, query 0, and -1 and Q as empty slots; a NaN is outside the mask."""
    r = np.full((2, 2, 9), -1.0, np.float32)
    p = np.full((2, 2, 9), 0.25, np.float32)
    r[0, 0, [0, 2, 5, 6, 8]], p[0, 0, [0, 2, 5, 6, 8]] = (1.0, 2.0, 1.0, 1.0, 4.0), (0.5, 0.75, 1.0, 0.625, 0.5)
    r[1, 0, 3] = np.nan
    r[1, 1, [4, 5]], p[1, 1, [4, 5]] = 1.0, 0.75
    masks, bits, stats = ref.instances(r, p, [1, -1, 0, 1, 2])
    assert masks.shape == (5, 2, 9) and bits.shape == (5, 2, 2) and bits.dtype == np.uint8
    assert masks[2].astype(int).tolist() == [[1, 0, 1, 0, 0, 1, 1, 0, 1], [0] * 9] and bits[2].tolist() == [[1 + 4 + 32 + 64, 1], [0, 0]]
    assert bits[0].tolist() == bits[3].tolist() == [[0, 0], [16 + 32, 0]] and not masks[[1, 4]].any()
    q1, q0, none = [2, int(1.5 * 2 ** 24), 4, 1, 6, 2], [5, int(3.375 * 2 ** 24), 0, 0, 9, 1], [0, 0, 9, 2, 0, 0]
    assert stats.tolist() == [q1, none, q0, q1, none]
    scores = boxmath.instance_scores(torch.from_numpy(stats)[None])
    assert scores.dtype == torch.float64 and scores[0].tolist() == [1.5 / (2 + 1e-6), 0.0, 3.375 / (5 + 1e-6), 1.5 / (2 + 1e-6), 0.0]
