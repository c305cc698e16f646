"""resize_many_nearest without a GPU: the index rule against Pillow, the restatement against the fixture, the host planner
(aa_many_plan_nearest) through ctypes, the argument errors of the Python call and the torch op's meta implementation."""
import ctypes
import struct

import numpy as np
import pytest
import torch

import kit_golden
import resize_many_nearest_ref as ref
from interpolate_antialiasing_amd import _lib, boxmath
from interpolate_antialiasing_amd import extension_interpolate as aa

BAD_DTYPE, BAD_LAYOUT, BAD_SHAPE, NULL, WORKSPACE, STRIDES = -2, -3, -4, -5, -6, -10
KMAX = (2 ** 31 - 1) // 4


# ---- the fixture and the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.case_names())
def test_restatement_reproduces_the_fixture(name):
    cs = ref.gen().case(name)
    got = ref.restate(cs, ref.inputs(name))
    exp = ref.expected(name)
    assert got.dtype == exp.dtype and got.shape == exp.shape
    assert np.array_equal(got, exp)


def test_fixture_is_small_and_holds_every_case():
    import os

    path = os.path.join(kit_golden.GOLDEN, "resize_many_nearest.npz")
    assert os.path.getsize(path) < 100 * 1024
    assert set(ref.fixture()) == {n for name in ref.case_names() for n in (name, name + "__incrc")}


def test_discriminator_cases_tell_the_two_rules_apart():
    g = ref.gen()
    for name in ("acc_whole", "acc_whole_t", "acc_whole_c3", "acc_box", "acc_i32", "closed_i16"):
        cs = g.case(name)
        wrong = ref.restate(cs, ref.inputs(name), closed_form=not g.closed_form(cs))
        assert not np.array_equal(wrong, ref.expected(name)), name
    assert boxmath.nearest_indices(2, 7) == [0, 0, 0, 0, 1, 1, 1] and boxmath.nearest_indices(2, 7, closed_form=True) == [0, 0, 0, 1, 1, 1, 1]
    for o in (15, 21, 23):
        assert boxmath.nearest_indices(2, o) != boxmath.nearest_indices(2, o, closed_form=True)
    assert boxmath.nearest_indices(5, 5) == [0, 1, 2, 3, 4]  # Image.resize's copy shortcut needs no special case


def test_fixture_regenerates_from_pillow():
    pytest.importorskip("PIL")
    g = ref.gen()
    for name in ref.case_names():
        cs = g.case(name)
        assert np.array_equal(g.pillow(cs, ref.inputs(name)), ref.expected(name)), name


def test_nearest_indices_against_pillow_on_400_draws():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(2024)
    for t in range(400):
        h, w = (int(v) for v in rng.integers(1, 91, 2))
        oh, ow = (int(v) for v in rng.integers(1, 121, 2))
        c = (1, 3, 4)[t % 3]
        mode = ("u1", "u1", "u1", "i4", "i2")[t % 5] if c == 1 else "u1"
        kind = (t // 3) % 3
        if kind == 0:
            box = None
        elif kind == 1:
            x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
            box = (x0, y0, int(rng.integers(x0 + 1, w + 1)), int(rng.integers(y0 + 1, h + 1)))
        else:
            x0, y0 = float(rng.uniform(0, w - 0.5)), float(rng.uniform(0, h - 0.5))
            box = (x0, y0, float(rng.uniform(x0 + 0.25, w)), float(rng.uniform(y0 + 0.25, h)))
        if mode == "u1":
            x = rng.integers(0, 256, (c, h, w)).astype(np.uint8)
            im = Image.fromarray(x[0] if c == 1 else np.ascontiguousarray(x.transpose(1, 2, 0)))
        elif mode == "i4":
            x = rng.integers(-2 ** 31, 2 ** 31, (1, h, w)).astype(np.int32)
            im = Image.fromarray(x[0])
        else:
            x = rng.integers(-2 ** 15, 2 ** 15, (1, h, w)).astype(np.int16)
            im = Image.frombytes("I;16", (w, h), x[0].view(np.uint16).tobytes())
        r = np.asarray(im.resize((ow, oh), Image.NEAREST, box=box))
        if mode == "i2":
            r = r.view(np.int16)
        got = ref.resize_nearest(x, (oh, ow), box, closed_form=mode == "i2")
        assert np.array_equal(r.reshape(oh, ow, c), got), (t, h, w, oh, ow, box, mode)


# ---- the planner through ctypes -------------------------------------------------------------------------------------------------------------
def _align16(v):
    return (v + 15) & ~15


def _records(shapes, c, eb, interleaved, boxes=None, flips=None):
    recs = (_lib.ManyImage * len(shapes))()
    for i, (h, w) in enumerate(shapes):
        r = recs[i]
        r.data_dev = 4096 * (i + 1)  # (never dereferenced: the plan is host arithmetic)
        r.H, r.W = h, w
        if interleaved:
            r.stride_ch, r.stride_px, r.stride_row = 1, c * eb, w * c * eb + 8
        else:
            r.stride_ch, r.stride_px, r.stride_row = h * w * eb + 64, eb, w * eb + 4 * eb
        if boxes is not None and boxes[i] is not None:
            r.has_box = 1
            for k in range(4):
                r.box[k] = boxes[i][k]
        if flips is not None and flips[i]:
            r.flags = _lib.MANY_FLIP_X
    return recs


def _plan(layout, eb, c, oh, ow, recs, places=None, fill=None, n=None, desc_bytes=None):
    L = _lib.load()
    n = len(recs) if n is None else n
    buf = (ctypes.c_uint8 * max(L.aa_many_desc_bytes_nearest(max(n, 0)), 64))()
    precs = None
    if places is not None:
        precs = (_lib.ManyPlace * len(places))()
        for i, p in enumerate(places):
            precs[i].vH, precs[i].vW, precs[i].oy, precs[i].ox = p
    cf = (ctypes.c_int32 * 4)(*(list(fill) + [0] * (4 - len(fill)))) if fill is not None else None
    ws = ctypes.c_size_t(0)
    rc = L.aa_many_plan_nearest(layout, eb, n, c, oh, ow, recs, precs, cf, ctypes.addressof(buf), len(buf) if desc_bytes is None else desc_bytes,
                                ctypes.byref(ws))
    return rc, buf, ws.value


@pytest.mark.parametrize("name,interleaved", [(n, i) for n in ("plain_c3", "placed_c3", "placed_c1", "center", "seam1025", "i16", "i32", "acc_box", "w5_c3")
                                              for i in ((False, True) if ref.gen().case(n)[2] > 1 else (False,))])  # (one channel is one class)
def test_plan_doubles_ranges_and_workspace(name, interleaved):
    g = ref.gen()
    cs = g.case(name)
    c, (oh, ow) = cs[2], cs[3]
    eb = np.dtype(g.DTYPES[cs[1]]).itemsize
    n = g.n_items(cs)
    geo = [g.geometry(cs, i) for i in range(n)]
    flips = cs[6]
    recs = _records([(q[0], q[1]) for q in geo], c, eb, interleaved, [q[2] for q in geo], flips)
    places = [(q[3][0], q[3][1], q[4][0], q[4][1]) for q in geo]
    rc, buf, ws = _plan(_lib.NHWC if interleaved else _lib.NCHW, eb, c, oh, ow, recs, places, cs[4])
    assert rc == 0
    hd, items, prefix = _lib.near_desc_view(buf, n)
    up = c if interleaved else 1
    planes = 1 if interleaved else c
    ne = 4 // eb
    vstrips = (ow * up * eb + 1023) // 1024
    assert (hd.n, hd.C, hd.oH, hd.oW, hd.elem_bytes) == (n, c, oh, ow, eb) and list(hd.fill)[:c] == list(cs[4])
    assert list(prefix) == [i * planes * oh * vstrips for i in range(n + 1)] and hd.units == prefix[n]
    off = 0
    for i, (h, w, box, (vh, vw), (py, px)) in enumerate(geo):
        it = items[i]
        b = boxmath.box_f32(box) if box is not None else (None, None, None, None)
        a_h, xo_h = boxmath.nearest_axis(h, vh, b[1], b[3], closed_form=eb == 2)
        a_w, xo_w = boxmath.nearest_axis(w, vw, b[0], b[2], closed_form=eb == 2)
        assert struct.pack("4d", it.a_h, it.xo0_h, it.a_w, it.xo0_w) == struct.pack("4d", a_h, xo_h, a_w, xo_w), (name, i)  # bit-equal
        v0h, v0w = max(0, -py), max(0, -px)
        mh, mw = min(vh, oh - py) - v0h, min(vw, ow - px) - v0w
        if mh <= 0 or mw <= 0:
            assert (it.mh, it.mw) == (0, 0)
            mh = mw = 0
        else:
            flip = bool(flips is not None and flips[i])
            dx = v0w + px
            assert (it.vh, it.vw, it.v0h, it.v0w, it.mh, it.mw, it.dy, it.dx) == (vh, vw, v0h, v0w, mh, mw, v0h + py, dx)
            assert it.dxo == (ow - dx - mw if flip else dx) and it.flags == int(flip)
        assert (it.in_h, it.in_w) == (h, w)
        assert it.tab_h == off
        off += _align16(4 * mh)
        assert it.tab_w == off
        if mw:
            off += _align16(4 * ((it.dxo * up) % ne + mw * up))
    assert ws == off == hd.ws_bytes


def test_plan_without_places_is_the_whole_canvas():
    recs = _records([(9, 11), (20, 5)], 1, 1, False)
    rc, buf, ws = _plan(_lib.NCHW, 1, 1, 6, 7, recs)
    assert rc == 0
    _, items, _ = _lib.near_desc_view(buf, 2)
    for it in items:
        assert (it.vh, it.vw, it.v0h, it.v0w, it.mh, it.mw, it.dy, it.dx, it.dxo) == (6, 7, 0, 0, 6, 7, 0, 0, 0)
    assert ws == 2 * (_align16(4 * 6) + _align16(4 * 7))


def test_plan_error_codes():
    L = _lib.load()
    ok = lambda **kw: _plan(**{**dict(layout=_lib.NCHW, eb=1, c=3, oh=10, ow=10, recs=_records([(20, 30)], 3, 1, False)), **kw})[0]  # noqa: E731
    assert ok() == 0
    assert ok(layout=7) == BAD_LAYOUT
    assert ok(eb=3) == BAD_DTYPE and ok(eb=8) == BAD_DTYPE
    assert ok(c=0) == BAD_SHAPE and ok(c=5) == BAD_SHAPE and ok(oh=0) == BAD_SHAPE and ok(ow=KMAX + 1) == BAD_SHAPE and ok(n=-1) == BAD_SHAPE
    assert ok(eb=2, recs=_records([(20, 30)], 3, 2, False)) == BAD_SHAPE and ok(eb=4, recs=_records([(20, 30)], 3, 4, False)) == BAD_SHAPE  # C > 1
    assert ok(eb=2, c=1, recs=_records([(20, 30)], 1, 2, False)) == 0 and ok(eb=4, c=1, recs=_records([(20, 30)], 1, 4, False)) == 0
    assert ok(desc_bytes=L.aa_many_desc_bytes_nearest(1) - 1) == WORKSPACE
    assert ok(places=[(0, 5, 0, 0)]) == BAD_SHAPE and ok(places=[(5, KMAX + 1, 0, 0)]) == BAD_SHAPE and ok(places=[(5, 5, -KMAX - 1, 0)]) == BAD_SHAPE
    assert ok(places=[(5, 5, 100, 100)]) == 0  # wholly off the canvas is legal
    assert ok(fill=[0, 256, 0]) == BAD_SHAPE and ok(fill=[0, -129, 0]) == BAD_SHAPE and ok(fill=[255, -128, 0]) == 0
    assert ok(eb=2, c=1, recs=_records([(20, 30)], 1, 2, False), fill=[65536]) == BAD_SHAPE
    assert ok(eb=4, c=1, recs=_records([(20, 30)], 1, 4, False), fill=[-2 ** 31]) == 0
    # NULLs
    ws = ctypes.c_size_t(0)
    buf = (ctypes.c_uint8 * 1024)()
    recs = _records([(20, 30)], 3, 1, False)
    assert L.aa_many_plan_nearest(0, 1, 1, 3, 10, 10, recs, None, None, None, 1024, ctypes.byref(ws)) == NULL
    assert L.aa_many_plan_nearest(0, 1, 1, 3, 10, 10, None, None, None, ctypes.addressof(buf), 1024, ctypes.byref(ws)) == NULL
    assert L.aa_many_plan_nearest(0, 1, 1, 3, 10, 10, recs, None, None, ctypes.addressof(buf), 1024, None) == NULL
    recs[0].data_dev = None
    assert ok(recs=recs) == NULL
    # the struct: flags, sizes, strides, boxes
    for flags, rc in ((_lib.MANY_FLIP_X, 0), (_lib.MANY_PREMUL_ALPHA, BAD_SHAPE), (4, BAD_SHAPE)):
        recs = _records([(20, 30)], 3, 1, False)
        recs[0].flags = flags
        assert ok(recs=recs) == rc
    recs = _records([(20, 30)], 3, 1, False)
    recs[0].H = KMAX + 1
    assert ok(recs=recs) == BAD_SHAPE
    recs[0].H = 0
    assert ok(recs=recs) == BAD_SHAPE
    assert ok(layout=_lib.NHWC) == STRIDES  # planar records in the interleaved class
    assert ok(recs=_records([(20, 30)], 3, 1, True)) == STRIDES and ok(layout=_lib.NHWC, recs=_records([(20, 30)], 3, 1, True)) == 0
    recs = _records([(20, 30)], 1, 2, False)
    recs[0].data_dev = 4097
    assert ok(eb=2, c=1, recs=recs) == STRIDES  # an element that is not aligned to itself
    recs = _records([(20, 30)], 1, 4, False)
    recs[0].stride_row = 30 * 4 + 2
    assert ok(eb=4, c=1, recs=recs) == STRIDES
    for box in ((0, 0, 31, 20), (-1, 0, 30, 20), (5, 5, 5, 10), (0, 0, float("nan"), 20)):
        assert ok(recs=_records([(20, 30)], 3, 1, False, [box])) == BAD_SHAPE, box
    assert ok(recs=_records([(20, 30)], 3, 1, False, [(0.5, 0.25, 30, 20)])) == 0
    # more work units than one grid holds
    assert ok(c=4, oh=KMAX, ow=1025, recs=_records([(20, 30)], 4, 1, False)) == BAD_SHAPE
    assert L.aa_many_desc_bytes_nearest(3) == 64 + 3 * 128 + 4 * 8 and L.aa_many_desc_bytes_nearest(-1) == 0


def test_launch_checks_come_before_any_enqueue():
    L = _lib.load()
    one = ctypes.c_void_p(4096)
    rc, buf, ws = _plan(_lib.NCHW, 1, 3, 10, 10, _records([(20, 30)], 3, 1, False))
    assert rc == 0 and ws > 0
    d = ctypes.addressof(buf)
    assert L.aa_resample_many_nearest(None, one, one, one, ws, 1, None) == NULL
    assert L.aa_resample_many_nearest(d, one, one, one, ws, 2, None) == BAD_DTYPE
    assert L.aa_resample_many_nearest(d, one, one, one, ws, 8, None) == BAD_DTYPE  # int64 is for one channel
    assert L.aa_resample_many_nearest(d, None, one, one, ws, 1, None) == NULL
    assert L.aa_resample_many_nearest(d, one, None, one, ws, 1, None) == NULL
    assert L.aa_resample_many_nearest(d, one, one, None, ws, 1, None) == NULL
    assert L.aa_resample_many_nearest(d, one, one, one, ws - 1, 1, None) == WORKSPACE
    assert L.aa_resample_many_nearest(d, one, one, ctypes.c_void_p(4100), ws, 1, None) == BAD_SHAPE
    assert L.aa_resample_many_nearest(d, ctypes.c_void_p(4100), one, one, ws, 1, None) == BAD_SHAPE
    rc, buf1, ws1 = _plan(_lib.NCHW, 4, 1, 10, 10, _records([(20, 30)], 1, 4, False))
    assert rc == 0
    assert L.aa_resample_many_nearest(ctypes.addressof(buf1), one, ctypes.c_void_p(4098), one, ws1, 4, None) == BAD_SHAPE  # the output's alignment
    assert L.aa_resample_many_nearest(ctypes.addressof(buf1), one, ctypes.c_void_p(4100), one, ws1, 8, None) == BAD_SHAPE
    hd = _lib.NearHeader.from_buffer(buf, 0)
    hd.magic ^= 1
    assert L.aa_resample_many_nearest(d, one, one, one, ws, 1, None) == BAD_SHAPE
    rc, buf0, ws0 = _plan(_lib.NCHW, 1, 3, 10, 10, None, n=0)
    assert rc == 0 and ws0 == 0
    assert L.aa_resample_many_nearest(ctypes.addressof(buf0), None, None, None, 0, 1, None) == 0  # n == 0 launches nothing


def test_abi_version_stays_3_and_the_symbols_are_exported():
    L = _lib.load()
    assert L.aa_abi_version() == 3
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    assert "#define AA_INTERP_ABI_VERSION 3 " in header
    for sym in ("aa_many_desc_bytes_nearest", "aa_many_plan_nearest", "aa_resample_many_nearest"):
        assert sym in _lib.EXPORTS and hasattr(L, sym) and sym + "(" in header
    assert ctypes.sizeof(_lib.NearHeader) == 64 and ctypes.sizeof(_lib.NearItem) == 128


# ---- argument errors of the Python call, all before any GPU use (the tensors are on the CPU) --------------------------------------------
def _t(c=1, h=20, w=30, dtype=torch.uint8):
    return torch.zeros((c, h, w), dtype=dtype)


def test_python_argument_errors_name_their_argument():
    f = aa.resize_many_nearest
    with pytest.raises(NotImplementedError, match=r"images\[1\] is torch.float32"):
        f([_t(), _t(dtype=torch.float32)], (8, 8))
    with pytest.raises(NotImplementedError, match=r"images\[0\] is torch.int64"):
        f([_t(dtype=torch.int64)], (8, 8))
    with pytest.raises(NotImplementedError, match=r"images\[0\] is torch.int16 with C = 3"):
        f([_t(3, dtype=torch.int16)], (8, 8))
    with pytest.raises(NotImplementedError, match=r"images\[0\] is torch.int32 with C = 2"):
        f([_t(2, dtype=torch.int32)], (8, 8))
    with pytest.raises(ValueError, match=r"same dtype: images\[1\] is torch.int16"):
        f([_t(), _t(dtype=torch.int16)], (8, 8))
    with pytest.raises(ValueError, match=r"same C: images\[1\] has 3"):
        f([_t(), _t(3)], (8, 8))
    with pytest.raises(NotImplementedError, match="out_dtype torch.float32"):
        f([_t()], (8, 8), out_dtype=torch.float32)
    with pytest.raises(NotImplementedError, match="out_dtype torch.int64 is built for one channel"):
        f([_t(3)], (8, 8), out_dtype=torch.int64)
    with pytest.raises(ValueError, match=r"fill\[0\] = 256 is outside 0..255"):
        f([_t()], (8, 8), fill=256)
    with pytest.raises(ValueError, match=r"fill\[0\] = -1 is outside 0..255"):
        f([_t()], (8, 8), fill=-1)
    with pytest.raises(ValueError, match=r"fill\[0\] = 40000 is outside -32768..32767"):
        f([_t(dtype=torch.int16)], (8, 8), fill=40000)
    with pytest.raises(ValueError, match=r"fill\[0\] = 2147483648 is outside"):
        f([_t(dtype=torch.int32)], (8, 8), fill=2 ** 31)
    with pytest.raises(ValueError, match="fill must be one int or one per channel"):
        f([_t(3)], (8, 8), fill=[1, 2])
    with pytest.raises(ValueError, match="fill must be one int"):
        f([_t()], (8, 8), fill=1.5)
    with pytest.raises(ValueError, match=r"boxes must hold one entry per image \(1\)"):
        f([_t()], (8, 8), boxes=[None, None])
    with pytest.raises(ValueError, match="box can't exceed original image size"):
        f([_t()], (8, 8), boxes=[(0, 0, 31, 20)])
    with pytest.raises(ValueError, match="box offset can't be negative"):
        f([_t()], (8, 8), boxes=[(-1, 0, 30, 20)])
    with pytest.raises(ValueError, match=r"flips must hold one entry per image \(1\)"):
        f([_t()], (8, 8), flips=[True, False])
    with pytest.raises(ValueError, match=r"sizes must hold one entry per image \(1\)"):
        f([_t()], (8, 8), sizes=[(4, 4), (4, 4)])
    with pytest.raises(ValueError, match=r"sizes\[0\] = \(0, 4\) must be positive"):
        f([_t()], (8, 8), sizes=[(0, 4)])
    with pytest.raises(ValueError, match=r"offsets\[0\] must be two integers"):
        f([_t()], (8, 8), offsets=[(1.5, 0)])
    with pytest.raises(ValueError, match="offsets must be None, 'center'"):
        f([_t()], (8, 8), offsets="middle")
    with pytest.raises(ValueError, match="an empty list needs channels="):
        f([], (8, 8))
    with pytest.raises(RuntimeError, match="output_size equals to 2"):
        f([_t()], (8,))
    with pytest.raises(RuntimeError, match="greater than 0"):
        f([_t()], (0, 8))
    with pytest.raises(RuntimeError, match=r"images\[0\] must be \[C, H, W\]"):
        f([torch.zeros((20, 30), dtype=torch.uint8)], (8, 8))
    with pytest.raises(ValueError, match="1 to 4 channels"):
        f([_t(5)], (8, 8))
    with pytest.raises(RuntimeError):  # a CPU tensor: there is no CPU fallback
        f([_t()], (8, 8))


def test_empty_list_gives_an_empty_batch():
    y = aa.resize_many_nearest([], (8, 9), channels=1, out_dtype=torch.int64)
    assert tuple(y.shape) == (0, 1, 8, 9) and y.dtype == torch.int64
    y = aa.resize_many_nearest(torch.zeros((0, 3, 5, 5), dtype=torch.uint8), (8, 9))
    assert tuple(y.shape) == (0, 3, 8, 9) and y.dtype == torch.uint8
    y = aa.resize_many_nearest(torch.zeros((0, 1, 5, 5), dtype=torch.int16), (8, 9))
    assert y.dtype == torch.int16


# ---- the torch op's meta implementation -------------------------------------------------------------------------------------------------------
def test_torch_op_meta_shape_dtype_and_strides():
    op = torch.ops.extension_interpolate.resize_many_nearest
    planar = [torch.empty((3, 20, 30), dtype=torch.uint8, device="meta"), torch.empty((3, 9, 11), dtype=torch.uint8, device="meta")]
    y = op(planar, [8, 10])
    assert tuple(y.shape) == (2, 3, 8, 10) and y.dtype == torch.uint8 and y.is_contiguous()
    inter = [torch.empty((20, 30, 3), dtype=torch.uint8, device="meta").permute(2, 0, 1), torch.empty((9, 11, 3), dtype=torch.uint8, device="meta").permute(2, 0, 1)]
    y = op(inter, [8, 10], flips=[True, False], fill=[1, 2, 3])
    assert tuple(y.shape) == (2, 3, 8, 10) and y.stride() == (240, 1, 30, 3)
    m = [torch.empty((1, 20, 30), dtype=torch.int32, device="meta")]
    y = op(m, [8, 10], sizes=[4, 5], offsets=[1, -2], fill=[-1])
    assert y.dtype == torch.int32 and y.is_contiguous() and tuple(y.shape) == (1, 1, 8, 10)
    y = op(m, [8, 10], out_dtype=torch.int64)
    assert y.dtype == torch.int64 and y.stride() == (80, 80, 10, 1)
