"""resize_many_back_confusion without a GPU: the planners (host arithmetic only) through ctypes — records, row tiles, work units, block
offsets, error codes in their order —, the launch's checks with dummy pointers, and the argument errors of the Python call."""
import ctypes

import pytest
import torch

from interpolate_antialiasing_amd import _lib
from interpolate_antialiasing_amd import extension_interpolate as aa

ERR_BAD_FILTER, ERR_BAD_DTYPE, ERR_BAD_LAYOUT, ERR_BAD_SHAPE, ERR_NULL, ERR_WORKSPACE, ERR_STRIDES = -1, -2, -3, -4, -5, -6, -10
ROWS = _lib.BACK_CONF_ROWS
PTR = 4096  # a dummy device address: the planner never follows it
HEIGHTS = (ROWS - 1, ROWS, 2 * ROWS + 1)


def items(heights=HEIGHTS, ow=300, **over):
    recs = (_lib.BackItemIn * len(heights))()
    for r, oh in zip(recs, heights):
        r.data_dev, r.stride_ch, r.stride_row, r.stride_px, r.h, r.w, r.oh, r.ow = PTR, 192, 16, 1, 12, 16, oh, ow
        for f, v in over.items():
            setattr(r, f, v)
    return recs


def targets(n, ptr=PTR, stride=304):
    t = (_lib.BackTargetIn * n)()
    for r in t:
        r.data_dev, r.stride_row = ptr, stride
    return t


def plan(recs, tg, k=7, groups=None, g=None, filt=0, layout=_lib.NCHW, dtype=_lib.U8, act=0, merge=0, short=0, n=None):
    """-> (rc, the block, workspace bytes, conf elements) of the plain planner, or with groups of the merged one."""
    L = _lib.load()
    n = len(recs) if n is None else n
    ws, elems = ctypes.c_size_t(0), ctypes.c_int64(0)
    if groups is None:
        nbytes = L.aa_back_confusion_desc_bytes(max(n, 0))
        buf = ctypes.create_string_buffer(max(nbytes, 64))
        rc = L.aa_back_confusion_plan(filt, layout, n, k, recs, tg, dtype, act, buf, nbytes - short, ctypes.byref(ws), ctypes.byref(elems))
    else:
        nbytes = L.aa_back_merged_confusion_desc_bytes(n, g)
        buf = ctypes.create_string_buffer(max(nbytes, 64))
        rc = L.aa_back_merged_confusion_plan(filt, layout, n, k, recs, g, (ctypes.c_int64 * n)(*groups), merge, tg, dtype, act, buf, nbytes - short,
                                             ctypes.byref(ws), ctypes.byref(elems))
    return rc, buf, ws.value, elems.value


def test_plan_records_tiles_and_offsets():
    L = _lib.load()
    rc, buf, ws, elems = plan(items(), targets(3), k=7)
    assert rc == 0 and elems == 3 * 49
    hd, its, _, _, unit0, tgs = _lib.back_conf_desc_view(buf, 3)
    assert (hd.n, hd.K, hd.merged, hd.G, hd.target_dtype, hd.conf_elems, hd.ws_bytes) == (3, 7, 0, 0, _lib.U8, 147, ws)
    assert [t.ytiles for t in tgs] == [1, 1, 3] and [it.xtiles for it in its] == [2, 2, 2]
    assert list(unit0) == [0, 2, 4, 10] and hd.units == 10
    assert [t.conf_off for t in tgs] == [0, 49, 98] and all(t.tgt == PTR and t.stride_row == 304 for t in tgs)
    # the items and the workspace are aa_back_many_plan's for the same items
    ref_buf = ctypes.create_string_buffer(L.aa_back_many_desc_bytes(3))
    ref_ws, arena, offs = ctypes.c_size_t(0), ctypes.c_size_t(0), (ctypes.c_int64 * 3)()
    assert L.aa_back_many_plan(0, _lib.NCHW, 3, 7, items(), _lib.BACK_ARGMAX, _lib.I64, ref_buf, len(ref_buf), ctypes.byref(ref_ws),
                               ctypes.byref(arena), offs) == 0
    assert ref_ws.value == ws
    for a, b in zip(its, _lib.back_desc_view(ref_buf, 3)[1]):
        assert all(getattr(a, f) == getattr(b, f) for f, _ in _lib.BackItem._fields_ if f != "out_off")
    # merged: the outputs are the groups; members ascend within a group
    tall = 2 * ROWS + 1
    rc, buf, ws2, elems = plan(items((tall, 5, tall)), targets(2), groups=[1, 0, 1], g=2, merge=1, dtype=_lib.I32, act=1)
    assert rc == 0 and elems == 2 * 49 and ws2 > 0
    hd, its, groups, members, unit0, tgs = _lib.back_conf_desc_view(buf, 3, 2)
    assert (hd.merged, hd.G, hd.merge, hd.activation, hd.target_dtype) == (1, 2, 1, 1, _lib.I32)
    assert list(members) == [1, 0, 2] and [(g.first, g.count, g.oh) for g in groups] == [(0, 1, 5), (1, 2, tall)]
    assert [t.ytiles for t in tgs] == [1, 3] and list(unit0) == [0, 2, 8] and [t.conf_off for t in tgs] == [0, 49]
    # one row: its stride is not looked at; n == 0 plans nothing
    assert plan(items((1,)), targets(1, stride=-5))[0] == 0
    assert plan(items(()), targets(0), n=0)[:1] == (0,) and plan(items(()), targets(0), n=0)[3] == 0


def test_plan_errors_in_order():
    ok, tg = items(), targets(3)
    assert plan(ok, tg, filt=9, layout=5, k=0)[0] == ERR_BAD_FILTER
    assert plan(ok, tg, layout=5, k=0)[0] == ERR_BAD_LAYOUT
    assert plan(ok, tg, k=0, act=7)[0] == ERR_BAD_SHAPE and plan(ok, tg, act=3)[0] == ERR_BAD_SHAPE
    assert plan(ok, tg, k=2 ** 20)[0] == ERR_BAD_SHAPE  # (K * K * 3 beyond 2^40)
    assert plan(ok, tg, groups=[0, 0, 0], g=1, merge=2)[0] == ERR_BAD_SHAPE and plan(ok, tg, groups=[0, 0, 0], g=4)[0] == ERR_BAD_SHAPE
    assert plan(ok, None, short=8)[0] == ERR_NULL
    assert plan(ok, tg, short=8, dtype=_lib.F32)[0] == ERR_WORKSPACE
    assert plan(ok, tg, groups=[0, 2, 0], g=2)[0] == ERR_BAD_SHAPE and plan(ok, tg, groups=[0, 0, 0], g=2)[0] == ERR_BAD_SHAPE
    assert plan(items((5,) * 17), targets(1), groups=[0] * 17, g=1, act=1)[0] == ERR_BAD_SHAPE  # (a softmax group of 17)
    assert plan(items((5,) * 17), targets(1), groups=[0] * 17, g=1, act=2)[0] == 0
    assert plan(ok, tg, groups=[0, 1, 0], g=2)[0] == ERR_BAD_SHAPE  # (members of one group, two sizes)
    # per item: its own checks, then its target's
    assert plan(items(data_dev=None), targets(3, ptr=None))[0] == ERR_NULL
    assert plan(items(flags=2), targets(3, stride=-1))[0] == ERR_BAD_SHAPE
    assert plan(items(stride_row=-1), targets(3, ptr=None))[0] == ERR_STRIDES
    assert plan(ok, targets(3, ptr=None), dtype=_lib.F32)[0] == ERR_NULL
    assert plan(ok, targets(3, stride=-1), dtype=_lib.F32)[0] == ERR_STRIDES
    for dt in (_lib.F32, _lib.F16, _lib.BOOL, 99):
        assert plan(ok, tg, dtype=dt)[0] == ERR_BAD_DTYPE
    for dt in (_lib.U8, _lib.I16, _lib.I32, _lib.I64):
        assert plan(ok, tg, dtype=dt)[0] == 0


def test_launch_checks_come_before_any_launch():
    """Dummy pointers: every call returns at a check, so nothing is enqueued and no device is needed."""
    L = _lib.load()
    rc, buf, ws, elems = plan(items(), targets(3), dtype=_lib.I32)
    assert rc == 0

    def launch(b=buf, dev=PTR, in_dtype=_lib.F32, conf=PTR, n_conf=elems, wsp=PTR, ws_bytes=ws):
        return L.aa_resample_back_confusion(b, dev, in_dtype, conf, n_conf, wsp, ws_bytes, None)

    assert L.aa_resample_back_confusion(None, PTR, _lib.F32, PTR, elems, PTR, ws, None) == ERR_NULL
    other = ctypes.create_string_buffer(len(buf))
    assert launch(b=other) == ERR_BAD_SHAPE  # (not this planner's block)
    assert launch(in_dtype=_lib.U8) == ERR_BAD_DTYPE
    assert launch(dev=None) == ERR_NULL and launch(conf=None) == ERR_NULL and launch(wsp=None) == ERR_NULL
    assert launch(ws_bytes=ws - 1) == ERR_WORKSPACE
    assert launch(conf=PTR + 4) == ERR_BAD_SHAPE and launch(wsp=PTR + 8) == ERR_BAD_SHAPE
    assert launch(n_conf=elems - 1) == ERR_WORKSPACE
    assert launch(in_dtype=_lib.F16, b=plan(items(data_dev=PTR + 1), targets(3))[1]) == ERR_STRIDES
    assert launch(b=plan(items(), targets(3, ptr=PTR + 2), dtype=_lib.I32)[1]) == ERR_STRIDES  # (a target off its element)
    hd = _lib.back_conf_desc_view(buf, 3)[0]
    hd.conf_elems += 1
    assert launch() == ERR_BAD_SHAPE
    empty = plan(items(()), targets(0), n=0)[1]
    assert launch(b=empty, dev=None, conf=None, wsp=None, n_conf=0, ws_bytes=0) == 0  # (n == 0 launches nothing)


def test_argument_errors():
    p = torch.zeros(4, 7, 12, 16)
    t = [torch.zeros(5, 6, dtype=torch.int64) for _ in range(4)]
    call = aa.resize_many_back_confusion
    assert "resize_many_back_confusion" in aa.__all__
    with pytest.raises(_lib.AAInterpError, match="no CPU implementation"):
        call(p, t)
    with pytest.raises(ValueError, match=r"targets must hold one entry per item \(4\), got 3"):
        call(p, t[:3])
    with pytest.raises(TypeError, match=r"targets\[1\] of torch.float32 is not an integer target"):
        call(p, [t[0], t[1].float(), t[2], t[3]])
    with pytest.raises(ValueError, match=r"same dtype: targets\[2\] is torch.uint8"):
        call(p, [t[0], t[1], t[2].byte(), t[3]])
    with pytest.raises(ValueError, match=r"targets\[3\] must be a non-empty \[oh, ow\]"):
        call(p, t[:3] + [torch.zeros(1, 5, 6, dtype=torch.int64)])
    with pytest.raises(ValueError, match="activation"):
        call(p, t, activation="relu")
    with pytest.raises(ValueError, match="merge"):
        call(p, t, merge="max")
    # with groups the targets are the groups': an entry of groups beyond them, a group without a member, a softmax group of 17
    with pytest.raises(ValueError, match=r"groups\[3\] = 2 is outside 0 .. 1"):
        call(p, t[:2], groups=[0, 1, 0, 2])
    with pytest.raises(ValueError, match="group 1 .* has no member"):
        call(p, t[:2], groups=[0, 0, 0, 0])
    with pytest.raises(ValueError, match="at most 16"):
        call(torch.zeros(17, 3, 4, 4), t[:1], groups=[0] * 17, activation="softmax")
    with pytest.raises(ValueError, match="beyond the supported"):
        call(torch.zeros(2, 1, 2, 2).expand(2, 2 ** 20, 2, 2), t[:2])
    # never differentiable, an empty batch gives [0, K, K]
    out = call(torch.zeros(0, 7, 4, 4, requires_grad=True), [])
    assert tuple(out.shape) == (0, 7, 7) and out.dtype == torch.int64 and out.grad_fn is None
    assert tuple(call([], [], channels=3).shape) == (0, 3, 3)
