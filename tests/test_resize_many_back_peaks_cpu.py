"""resize_many_back_peaks without a GPU: the reference on cases worked by hand, the planner (host arithmetic only) through ctypes —
the block's fields, its offsets, the error codes — the Python refusals that come before any launch, and boxmath.peak_points."""
import ctypes

import numpy as np
import pytest
import torch

import resize_many_back_peaks_ref as ref
from interpolate_antialiasing_amd import _lib, boxmath
from interpolate_antialiasing_amd import extension_interpolate as aa

ERR_BAD_SHAPE, ERR_NULL, ERR_STRIDES, ERR_WORKSPACE = -4, -5, -10, -6
PTR = 4096  # a dummy device address: the planner never follows it
OUTS = ((23, 300), (3, 5))
NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("r,xy,values", (
    ([[1, 5, 2], [5, 0, 5]], (1, 0), [5, 1, 2, 5, 0]),                 # a tie: the lower flat index; above the image: the peak itself
    ([[1, 7, NAN], [9, 0, 0]], (2, 0), [NAN, 7, NAN, NAN, 0]),         # a NaN after a larger number
    ([[0, NAN], [NAN, 3]], (1, 0), [NAN, 0, NAN, NAN, 3]),             # two NaNs: the first
    ([[-1, -0.0, 0.0]], (1, 0), [-0.0, -1, 0.0, -0.0, -0.0]),          # -0.0 before +0.0: equal, and the sign of the peak's zero kept
    ([[4]], (0, 0), [4, 4, 4, 4, 4]),                                  # 1 x 1: all five the peak
    ([[0, 1], [2, 8]], (1, 1), [8, 2, 8, 1, 8])))                      # a corner
def test_the_reference_on_cases_worked_by_hand(r, xy, values):
    got_xy, got = ref.peaks(np.array([r, r], np.float32))
    assert got_xy.tolist() == [list(xy)] * 2 and got.dtype == np.float32
    assert (got.view(np.uint32) == np.array([values, values], np.float32).view(np.uint32)).all(), got


def plan(k=17, filt=0, ptr=PTR, stride_px=1, short=0, outs=OUTS, n=2, layout=_lib.NCHW):
    L = _lib.load()
    recs = (_lib.BackItemIn * 2)()
    for r, (oh, ow) in zip(recs, outs):
        r.data_dev, r.stride_ch, r.stride_row, r.stride_px, r.h, r.w, r.oh, r.ow = ptr, 192, 16, stride_px, 12, 16, oh, ow
    nbytes = L.aa_back_peaks_desc_bytes(n) - short
    buf = ctypes.create_string_buffer(nbytes + short)
    ws, arena, v_off = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_int64(0)
    rc = L.aa_back_peaks_plan(filt, layout, n, k, recs, buf, nbytes, ctypes.byref(ws), ctypes.byref(arena), ctypes.byref(v_off))
    return rc, buf, ws.value, arena.value, v_off.value


def test_the_block_and_the_planner_errors():
    L = _lib.load()
    size = lambda n: ctypes.sizeof(_lib.BackPeaksHeader) + n * ctypes.sizeof(_lib.BackItem) + 8 * (n + 1)
    assert ctypes.sizeof(_lib.BackPeaksHeader) == 80 and [L.aa_back_peaks_desc_bytes(n) for n in (0, 2, 70)] == [size(0), size(2), size(70)]
    rc, buf, ws, arena, v_off = plan()
    hd = _lib.BackPeaksHeader.from_buffer(buf, 0)
    units = [-(-oh // _lib.BACK_PEAKS_ROWS) * -(-ow // _lib.BACK_TILE) for oh, ow in OUTS]
    assert rc == 0 and (hd.n, hd.K, hd.filter, hd.layout, hd.rows, hd.units) == (2, 17, 0, _lib.NCHW, _lib.BACK_PEAKS_ROWS, sum(units))
    assert list((ctypes.c_int64 * 3).from_buffer(buf, size(2) - 24)) == [0, units[0], sum(units)]
    up16 = lambda v: -(-v // 16) * 16
    # the workspace: resize_many_back's tables for the same items, then the keys; the arena: peaks, then values
    recs = (_lib.BackItemIn * 2)()
    for r, (oh, ow) in zip(recs, OUTS):
        r.data_dev, r.stride_ch, r.stride_row, r.stride_px, r.h, r.w, r.oh, r.ow = PTR, 192, 16, 1, 12, 16, oh, ow
    tables, other, offs = ctypes.c_size_t(0), ctypes.c_size_t(0), (ctypes.c_int64 * 2)()
    assert L.aa_back_many_plan(0, _lib.NCHW, 2, 17, recs, _lib.BACK_VALUES, _lib.F32, ctypes.create_string_buffer(1024), 1024, ctypes.byref(tables),
                               ctypes.byref(other), offs) == 0
    assert hd.tables_bytes == tables.value and hd.keys_off == up16(tables.value) and ws == hd.keys_off + 8 * 2 * 17 == hd.ws_bytes
    assert v_off == up16(2 * 17 * 2 * 4) == hd.values_off and arena == v_off + 2 * 17 * 5 * 4 == hd.arena_bytes
    # the statuses, in the planner's order
    assert plan(filt=99, k=0)[0] == -1 and plan(layout=7, k=0)[0] not in (0, ERR_BAD_SHAPE) and [plan(k=v, ptr=None)[0] for v in (0, -1)] == [ERR_BAD_SHAPE] * 2
    assert plan(short=8, ptr=None)[0] == ERR_WORKSPACE and plan(ptr=None)[0] == ERR_NULL and plan(stride_px=2)[0] == ERR_STRIDES
    # a flat index is 32 bits of the key.  2^31 - 1 is a prime, so no two sides give it: 2^31 - 2 = 42966 * 49981 is the most an item has
    assert 42966 * 49981 == 2 ** 31 - 2 and plan(k=1, outs=((42966, 49981), (3, 5)))[0] == 0
    assert plan(k=1, outs=((65536, 32768), (3, 5)))[0] == ERR_BAD_SHAPE and plan(k=1, outs=((3, 5), (32768, 65536)))[0] == ERR_BAD_SHAPE
    rc, buf, ws, arena, v_off = plan(n=0)
    assert (rc, arena, v_off) == (0, 0, 0) and _lib.BackPeaksHeader.from_buffer(buf, 0).units == 0


def test_the_refusals_before_any_launch():
    x = torch.zeros(2, 5, 4, 4)
    with pytest.raises(NotImplementedError, match=r"torch\.no_grad\(\).*\.detach\(\)"):
        aa.resize_many_back_peaks(x.clone().requires_grad_(), [(3, 3), (4, 5)])
    with pytest.raises(ValueError, match=r"sizes must hold one entry per item \(2\), got 1"):
        aa.resize_many_back_peaks(x, [(3, 3)])
    with pytest.raises(ValueError, match="more than 2\\^31 - 1 pixels"):
        aa.resize_many_back_peaks(x[:, :1], [(3, 3), (65536, 32768)])
    for pred, k in ((x[:0], 5), ([], 1)):
        peaks, values = aa.resize_many_back_peaks(pred, [])
        assert (tuple(peaks.shape), peaks.dtype, tuple(values.shape), values.dtype) == ((0, k, 2), torch.int32, (0, k, 5), torch.float32)
    assert "resize_many_back_peaks" in aa.__all__


def test_peak_points():
    peaks = torch.tensor([[[3, 1], [0, 2]], [[4, 0], [1, 1]]], dtype=torch.int32)
    # (peak, left, right, up, down): right > left and down == up; on the left border (left = the peak) with right < left; ...
    values = torch.tensor([[[9, 1, 2, 5, 5], [9, 9, 3, 4, 6]], [[9, 7, 7, 9, 1], [9, 2, 1, 8, 3]]], dtype=torch.float32)
    sizes = [(4, 8), (2, 5)]
    centre = boxmath.peak_points(peaks, values, sizes)
    assert centre.dtype == torch.float32 and centre.tolist() == [[[3.5, 1.5], [0.5, 2.5]], [[4.5, 0.5], [1.5, 1.5]]]
    quarter = boxmath.peak_points(peaks, values, sizes, refine="quarter")
    assert quarter.tolist() == [[[3.75, 1.5], [0.25, 2.75]], [[4.5, 0.25], [1.25, 1.25]]]
    boxed = boxmath.peak_points(peaks, values, sizes, boxes=[(10, 20, 26, 24), (0, 0, 10, 1)], refine="quarter")
    assert boxed.tolist() == [[[17.5, 21.5], [10.5, 22.75]], [[9.0, 0.125], [2.5, 0.625]]]
    with pytest.raises(ValueError, match="refine must be None or 'quarter'"):
        boxmath.peak_points(peaks, values, sizes, refine="taylor")
