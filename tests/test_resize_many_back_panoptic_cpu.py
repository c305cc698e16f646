"""resize_many_back_panoptic without a GPU: the planner (host arithmetic only) through ctypes — the block's size, its prefixes and
offsets, the error codes in their order — the Python refusals that come before any launch, and the reference's own sanity."""
import ctypes

import numpy as np
import pytest
import torch

import resize_many_back_panoptic_ref as ref
from interpolate_antialiasing_amd import _lib
from interpolate_antialiasing_amd import extension_interpolate as aa

ERR_BAD_DTYPE, ERR_BAD_SHAPE, ERR_NULL, ERR_STRIDES, ERR_WORKSPACE = -2, -4, -5, -10, -6
PTR = 4096  # a dummy device address: the planner never follows it
OUTS = ((23, 300), (3, 5))


def plan(q=100, dtype=_lib.I32, filt=0, ptr=PTR, stride_px=1, short=0):
    L = _lib.load()
    recs = (_lib.BackItemIn * 2)()
    for r, (oh, ow) in zip(recs, OUTS):
        r.data_dev, r.stride_ch, r.stride_row, r.stride_px, r.h, r.w, r.oh, r.ow = ptr, 192, 16, stride_px, 12, 16, oh, ow
    nbytes = L.aa_back_panoptic_desc_bytes(2) - short
    buf = ctypes.create_string_buffer(nbytes + short)
    ws, arena, offs, c_off, s_off = ctypes.c_size_t(0), ctypes.c_size_t(0), (ctypes.c_int64 * 2)(), ctypes.c_int64(0), ctypes.c_int64(0)
    rc = L.aa_back_panoptic_plan(filt, _lib.NCHW, 2, q, recs, dtype, buf, nbytes, ctypes.byref(ws), ctypes.byref(arena), offs, ctypes.byref(c_off),
                                 ctypes.byref(s_off))
    return rc, buf, ws.value, arena.value, list(offs), c_off.value, s_off.value


def test_the_block_and_the_planner_errors():
    L = _lib.load()
    size = lambda n: ctypes.sizeof(_lib.BackPanopticHeader) + n * ctypes.sizeof(_lib.BackItem) + 2 * 8 * (n + 1)
    assert ctypes.sizeof(_lib.BackPanopticHeader) == 96 and [L.aa_back_panoptic_desc_bytes(n) for n in (0, 2, 70)] == [size(0), size(2), size(70)]
    rc, buf, ws, arena, offs, c_off, s_off = plan()
    hd = _lib.BackPanopticHeader.from_buffer(buf, 0)
    rows, fin = _lib.BACK_PANOPTIC_ROWS, _lib.BACK_PANOPTIC_FIN_BYTES
    units = [-(-oh // rows) * -(-ow // _lib.BACK_TILE) for oh, ow in OUTS]
    fins = [-(-(oh * ow * 4 + 15) // fin) for oh, ow in OUTS]
    assert rc == 0 and (hd.n, hd.Q, hd.units, hd.fin_units) == (2, 100, sum(units), sum(fins)) and fins == [2, 1]
    prefix = (ctypes.c_int64 * 6).from_buffer(buf, size(2) - 48)
    assert list(prefix) == [0, units[0], sum(units), 0, fins[0], sum(fins)]
    assert offs == [0, 23 * 300 * 4] and c_off == offs[1] + 64 and s_off == c_off + 2 * 100 * 24 and arena == s_off + 200 == hd.arena_bytes
    assert hd.kept_words == 104 and hd.kept_off == -(-hd.tables_bytes // 16) * 16 and ws == hd.kept_off + 2 * 104 * 4 == hd.ws_bytes
    # the statuses, in the planner's order
    assert plan(filt=99, q=0)[0] == -1 and plan(q=0)[0] == ERR_BAD_SHAPE and plan(q=257)[0] == ERR_BAD_SHAPE and plan(q=256)[0] == 0
    assert plan(q=256, dtype=_lib.U8)[0] == ERR_BAD_SHAPE and plan(q=255, dtype=_lib.U8)[0] == 0
    assert plan(short=8, ptr=None)[0] == ERR_WORKSPACE and plan(ptr=None)[0] == ERR_NULL and plan(stride_px=2, dtype=_lib.F32)[0] == ERR_STRIDES
    assert plan(dtype=_lib.F32)[0] == ERR_BAD_DTYPE and plan(dtype=_lib.BOOL)[0] == ERR_BAD_DTYPE


def test_the_refusals_before_any_launch():
    x, s = torch.zeros(2, 5, 4, 4), torch.ones(2, 5)
    for bad, words in ((dict(s=torch.ones(2, 4)), r"scores must be \[N, Q\] = \[2, 5\]"), (dict(s=s.double()), "scores must be torch.float32"),
                       (dict(ids=torch.zeros(2, 5)), "ids must be torch.int32"), (dict(void=-1, out_dtype=torch.uint8), "void must be an int that"),
                       (dict(void=2 ** 15, out_dtype=torch.int16), "void must be an int that"), (dict(overlap_threshold=float("nan")), "must not be NaN"),
                       (dict(x=torch.zeros(2, 257, 4, 4), s=torch.ones(2, 257)), "Q must be in 1 .. 256"),
                       (dict(x=torch.zeros(2, 256, 4, 4), s=torch.ones(2, 256), void=0, out_dtype=torch.uint8), "got Q = 256")):
        kw = {"x": x, "s": s, **bad}
        with pytest.raises(ValueError, match=words):
            aa.resize_many_back_panoptic(kw.pop("x"), kw.pop("s"), [(3, 3), (4, 5)], **kw)
    with pytest.raises(NotImplementedError, match="out_dtype torch.float32 is not built"):
        aa.resize_many_back_panoptic(x, s, [(3, 3), (4, 5)], out_dtype=torch.float32)
    with pytest.raises(NotImplementedError, match=r"torch\.no_grad\(\).*\.detach\(\)"):
        aa.resize_many_back_panoptic(x, s.clone().requires_grad_(), [(3, 3), (4, 5)])
    maps, counts, survives = aa.resize_many_back_panoptic([], torch.ones(0, 5), [])
    assert maps == [] and tuple(counts.shape) == (0, 5, 3) and tuple(survives.shape) == (0, 5)


def test_the_reference_on_a_case_worked_by_hand():
    """Three queries on four pixels: query 0 dropped, 1 and 2 tie on pixel 0 (the lower wins), a NaN wins pixel 3 and is not inside."""
    p = np.array([[0.9, 0.9, 0.9, 0.9], [0.8, 0.6, 0.2, 0.7], [0.8, 0.7, 0.4, np.nan]], np.float32).reshape(3, 1, 4)
    scores = np.array([0.0, 0.5, 0.5], np.float32)
    m, c, s = ref.panoptic(p, scores, overlap_threshold=0.5)
    assert c.tolist() == [[0, 0, 0], [1, 3, 1], [3, 2, 1]] and s.tolist() == [False, False, True] and m.tolist() == [[-1, 2, -1, -1]]
    m, _, s = ref.panoptic(p, scores, ids=np.array([7, 8, 9], np.int32), void=255, overlap_threshold=1 / 3, dtype=np.uint8)
    assert s.tolist() == [False, True, True] and m.tolist() == [[8, 9, 255, 255]] and m.dtype == np.uint8
