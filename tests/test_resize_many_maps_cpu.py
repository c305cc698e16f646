"""resize_many_maps without a GPU: the numpy restatement of Pillow's "I;16" / "I" / "F" resize against the committed fixture and against
live Pillow, the host planner through ctypes (which passes run, hulls, ksize, workspace, table alignment, descriptor size), the Python
call's argument errors, the empty batch and the torch op's meta implementation."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import resize_many_maps_ref as ref  # noqa: E402

from interpolate_antialiasing_amd import _lib, boxmath  # noqa: E402
from interpolate_antialiasing_amd import extension_interpolate as aa  # noqa: E402

RESIZE_MANY_MAPS = aa.resize_many_maps  # (the module needs the call: every test here fails without it)
G = ref.gen()
COMBOS = [(case, name, dt) for case, cs in G.CASES.items() for dt in cs["dtypes"] for name in cs["filters"]]
BAD_FILTER, BAD_DTYPE, BAD_SHAPE, ERR_NULL, ERR_WORKSPACE, ERR_STRIDES = -1, -2, -4, -5, -6, -10
TORCH_DT = {"u16": torch.uint16, "i32": torch.int32, "f32": torch.float32}


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


# ---- the restatement is Pillow --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,name,dt", COMBOS)
def test_restatement_equals_the_fixture(case, name, dt):
    exp = ref.expected(case, name, dt)
    got = ref.restate(case, name, dt)
    assert got.dtype == exp.dtype == ref.DTYPES[dt] and np.array_equal(_bits(got), _bits(exp))


def test_restatement_equals_live_pillow_on_random_cases():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(2025)
    for dt in G.DTS:
        for t in range(6):
            h, w, vh, vw = (int(v) for v in rng.integers(1, 40, 4))
            box = None
            if t % 2:
                x0, y0 = float(rng.uniform(0, w / 2)), float(rng.uniform(0, h / 2))
                box = (x0, y0, x0 + float(rng.uniform(0.5, w / 2)), y0 + float(rng.uniform(0.5, h / 2)))
            name = G.ALL[int(rng.integers(0, 5))]
            x = G.as_dtype(rng.integers(0, 65536, (h, w)).astype(np.uint16), dt)
            pil = np.asarray(G._to_pil(x, dt).resize((vw, vh), getattr(Image, G.PIL_FILTER[name]), box=box)).reshape(vh, vw)
            got = ref.resize(x, (vh, vw), name, box)
            assert np.array_equal(_bits(got), _bits(pil.astype(x.dtype))), (dt, t, h, w, vh, vw, box, name)


def test_the_overflow_store_is_no_clamp_and_the_fma_case_tells_a_fused_sum():
    for case in ("over", "over_t"):
        pil = ref.expected(case, "bicubic", "u16")
        clamp = ref.restate(case, "bicubic", "u16", overflow="clamp")
        assert int((pil != clamp).sum()) >= 20  # (the wrapped values: 0xFF00 | (r & 255) where a clamp stores 65535)
        assert int(clamp.max()) == 65535 and ((pil != clamp) <= (clamp == 65535)).all()
    assert (ref.expected("over", "bicubic", "u16") == 65302).any()
    for name, rows in (("bilinear", slice(0, 6)), ("bicubic", slice(6, 8))):
        fused = ref.restate("fma", name, "u16", fused=True)
        assert (fused != ref.expected("fma", name, "u16")).any(axis=2)[0][rows].all()


def test_a_skipped_pass_is_not_an_identity_filter():
    """Lanczos at scale 1 has non-zero off-centre taps: running the kept axis of the width-kept item as a filter changes float bits."""
    x = ref.inputs("ragged", "f32")[2]
    h, w = x.shape
    _, xmin, xsize, k = ref.coeffs(w, w, 0.0, float(w), "lanczos")
    assert (k != 0).sum(axis=1).max() > 1
    assert ref.passes(h, w, (20, w), None)[:2] == (False, True)
    assert ref.passes(27, 35, (20, 23), (5, 4, 28, 24))[:2] == (False, False) and ref.passes(20, 35, (20, 23), None)[:2] == (True, False)


# ---- the planner, through ctypes ------------------------------------------------------------------------------------------------------------
def _records(cs, eb, flips=None, pitch_extra=0):
    n = len(cs["items"])
    recs = (_lib.ManyImage * n)()
    for i in range(n):
        h, w, box, _, _ = G.geometry(cs, i)
        r = recs[i]
        r.data_dev = 4096 * (i + 1)  # (never dereferenced: the plan is host arithmetic)
        r.H, r.W = h, w
        r.stride_px, r.stride_row, r.stride_ch = eb, (w + pitch_extra) * eb, 0
        if box is not None:
            r.has_box = 1
            r.box[:] = [float(v) for v in box]
        if flips is not None and flips[i]:
            r.flags = _lib.MANY_FLIP_X
    return recs


def _places(cs):
    if not cs.get("placed"):
        return None
    n = len(cs["items"])
    precs = (_lib.ManyPlace * n)()
    for i in range(n):
        _, _, _, (vh, vw), (py, px) = G.geometry(cs, i)
        precs[i].vH, precs[i].vW, precs[i].oy, precs[i].ox = vh, vw, py, px
    return precs


def _plan(name, elem, oh, ow, recs, places=None, fill=0.0, overflow=0, n=None, desc_bytes=None):
    L = _lib.load()
    n = len(recs) if n is None else n
    buf = (ctypes.c_uint8 * max(L.aa_many_desc_bytes_maps(max(n, 0)), 64))()
    ws = ctypes.c_size_t(0)
    rc = L.aa_many_plan_maps(_lib.FILTER_IDS.get(name, 99), elem, n, oh, ow, recs, places, fill, overflow, buf,
                             len(buf) if desc_bytes is None else desc_bytes, ctypes.byref(ws))
    return rc, buf, ws.value


def _align16(v):
    return (v + 15) & ~15


def _expected_axis(run, in_size, v, v0, m, b0, b1, name):
    """(o, hull, ksize) of one axis from boxmath and the restatement's windows."""
    if not run:
        return int(b0) + v0, m, 0
    ksize, xmin, xsize, _ = ref.coeffs(in_size, v, b0, b1, name)
    o, e = int(xmin[v0]), int(xmin[v0 + m - 1] + xsize[v0 + m - 1])
    if v0 == 0 and m == v:
        assert (o, e) == boxmath.axis_hull(in_size, v, b0, b1, name)
    return o, e - o, ksize


@pytest.mark.parametrize("case", ["ragged", "placed", "long_w", "halfpx"])
@pytest.mark.parametrize("elem,eb", [(_lib.MAPS_U16, 2), (_lib.MAPS_F32, 4)])
def test_plan_passes_hulls_ksize_and_workspace(case, elem, eb):
    cs = G.CASES[case]
    oh, ow = cs["canvas"]
    n = len(cs["items"])
    for name in cs["filters"]:
        rc, buf, ws = _plan(name, elem, oh, ow, _records(cs, eb, cs.get("flips")), _places(cs), fill=7.0)
        assert rc == 0
        hd, items, prefix = _lib.maps_desc_view(buf, n)
        assert (hd.n, hd.oH, hd.oW, hd.filter, hd.elem, hd.overflow) == (n, oh, ow, _lib.FILTER_IDS[name], elem, 0)
        off, units, inters = 0, 0, []
        for i in range(n):
            h, w, box, (vh, vw), (py, px) = G.geometry(cs, i)
            it = items[i]
            hrun, vrun, b = ref.passes(h, w, (vh, vw), box)
            v0h, v0w = max(0, -py), max(0, -px)
            mh, mw = min(vh, oh - py) - v0h, min(vw, ow - px) - v0w
            assert prefix[i] == units
            if mh <= 0 or mw <= 0:
                assert (it.mh, it.mw, it.flags & 6) == (0, 0, 0)
                continue
            assert (it.vh, it.vw, it.v0h, it.v0w, it.mh, it.mw, it.dy, it.dx) == (vh, vw, v0h, v0w, mh, mw, v0h + py, v0w + px)
            assert bool(it.flags & _lib.MAPS_ITEM_HPASS) == hrun and bool(it.flags & _lib.MAPS_ITEM_VPASS) == vrun, (case, i)
            assert bool(it.flags & _lib.MAPS_ITEM_FLIP) == bool(cs.get("flips") and cs["flips"][i])
            assert (it.oy, it.hull_h, it.ksize_h) == _expected_axis(vrun, h, vh, v0h, mh, b[1], b[3], name), (case, i)
            assert (it.ox, it.hull_w, it.ksize_w) == _expected_axis(hrun, w, vw, v0w, mw, b[0], b[2], name), (case, i)
            if vrun:  # [int32 xmin[m]][int32 xsize[m]][double w[m * ksize]], the doubles 8-byte aligned
                assert it.tab_h == off and it.tab_h % 16 == 0 and (it.tab_h + 8 * mh) % 8 == 0
                off += _align16(8 * mh + 8 * mh * it.ksize_h)
            if hrun:
                assert it.tab_w == off and it.tab_w % 16 == 0 and (it.tab_w + 8 * mw) % 8 == 0
                off += _align16(8 * mw + 8 * mw * it.ksize_w)
                units += ((it.hull_h + _lib.MAPS_HROWS - 1) // _lib.MAPS_HROWS) * ((mw + _lib.MANY_STRIP - 1) // _lib.MANY_STRIP)
                inters.append((i, it.hull_h * mw * eb))
        assert prefix[n] == units == hd.hunits
        for i, nbytes in inters:  # the intermediates follow the arena, in the item's element type, only the hull rows
            assert items[i].inter == off
            off += _align16(nbytes)
        assert ws == off == hd.ws_bytes


def test_plan_which_passes_run():
    cs = G.CASES["ragged"]
    rc, buf, _ = _plan("lanczos", _lib.MAPS_I32, 20, 23, _records(cs, 4))
    assert rc == 0
    _, items, prefix = _lib.maps_desc_view(buf, 5)
    H, V = _lib.MAPS_ITEM_HPASS, _lib.MAPS_ITEM_VPASS
    assert [it.flags for it in items] == [H | V, H | V, V, H, 0]  # fractional box, up-scaled, width kept, height kept, plain copy
    assert (items[4].oy, items[4].ox, items[4].hull_h, items[4].hull_w) == (4, 5, 20, 23) and items[4].ksize_h == items[4].ksize_w == 0
    assert (items[2].ox, items[2].hull_w, items[2].ksize_w) == (0, 23, 0) and (items[3].oy, items[3].hull_h, items[3].ksize_h) == (0, 20, 0)
    # one horizontal unit per 16 hull rows (23 columns are one strip): 70, 8 and 20 rows; none for items 2 and 4
    assert (items[0].hull_h, items[1].hull_h, _lib.MAPS_HROWS) == (70, 8, 16) and list(prefix) == [0, 5, 6, 6, 8, 8]
    assert items[0].ksize_w == int(math.ceil(3.0 * boxmath.f32(120.75 - 3.25) / 23)) * 2 + 1


def test_plan_descriptor_size_fill_and_errors():
    L = _lib.load()
    assert ctypes.sizeof(_lib.MapsHeader) == 64 and ctypes.sizeof(_lib.MapsItem) == 144
    for n in (0, 1, 7):
        assert L.aa_many_desc_bytes_maps(n) == 64 + 144 * n + 8 * (n + 1)
    cs = G.CASES["center"]
    recs = _records(cs, 2)
    ok = lambda **kw: _plan(**{**dict(name="bicubic", elem=_lib.MAPS_U16, oh=14, ow=14, recs=recs, places=_places(cs)), **kw})  # noqa: E731
    assert ok()[0] == 0
    assert _lib.maps_desc_view(ok(fill=65535.0, overflow=1)[1], 3)[0].fill == 65535 and _lib.maps_desc_view(ok(overflow=1)[1], 3)[0].overflow == 1
    assert _lib.maps_desc_view(ok(elem=_lib.MAPS_I32, recs=_records(cs, 4), fill=-7.0)[1], 3)[0].fill == 0xFFFFFFF9
    assert _lib.maps_desc_view(ok(elem=_lib.MAPS_F32, recs=_records(cs, 4), fill=-1.5)[1], 3)[0].fill == 0xBFC00000
    assert ok(name="sinc")[0] == BAD_FILTER
    assert ok(elem=3)[0] == BAD_DTYPE
    assert ok(overflow=2)[0] == BAD_SHAPE
    for fill in (-1.0, 65536.0, 1.5, float("nan")):
        assert ok(fill=fill)[0] == BAD_SHAPE
    assert ok(elem=_lib.MAPS_I32, recs=_records(cs, 4), fill=2.0 ** 31)[0] == BAD_SHAPE
    for fill in (float("inf"), float("nan"), 1e39):
        assert ok(elem=_lib.MAPS_F32, recs=_records(cs, 4), fill=fill)[0] == BAD_SHAPE
    assert ok(oh=0)[0] == BAD_SHAPE
    assert ok(desc_bytes=L.aa_many_desc_bytes_maps(3) - 1)[0] == ERR_WORKSPACE
    assert ok(recs=None, n=3)[0] == ERR_NULL
    odd = _records(cs, 2)
    odd[1].data_dev = 4097  # not aligned to the element
    assert ok(recs=odd)[0] == ERR_STRIDES
    odd = _records(cs, 2)
    odd[1].data_dev, odd[1].stride_row = 4098, 2 * 10 + 2  # 2-byte alignment and a pitch that is no multiple of 4 are served
    assert ok(recs=odd)[0] == 0
    bad = _records(cs, 2)
    bad[0].flags = 2  # (alpha is not this call's)
    assert ok(recs=bad)[0] == BAD_SHAPE
    bad = _records(cs, 2)
    bad[0].has_box = 1
    bad[0].box[:] = [0.0, 0.0, 36.0, 25.0]  # beyond the 25 x 35 image
    assert ok(recs=bad)[0] == BAD_SHAPE
    # an empty plan, and a launch of it without a device
    rc, buf0, ws0 = _plan("bilinear", _lib.MAPS_F32, 8, 9, None, n=0)
    assert (rc, ws0) == (0, 0)
    assert L.aa_resample_many_maps(ctypes.addressof(buf0), None, None, None, 0, None) == 0  # n == 0 launches nothing
    assert L.aa_resample_many_maps(None, None, None, None, 0, None) == ERR_NULL


def test_the_symbols_are_exported_and_declared():
    L = _lib.load()
    assert L.aa_abi_version() == 3
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    for sym in ("aa_many_desc_bytes_maps", "aa_many_plan_maps", "aa_resample_many_maps"):
        assert sym in _lib.EXPORTS and hasattr(L, sym) and sym + "(" in header


# ---- argument errors of the Python call, all before any GPU use (the tensors are on the CPU) --------------------------------------------
def _t(c=1, h=20, w=30, dtype=torch.uint16):
    return torch.zeros((c, h, w), dtype=dtype)


def test_python_argument_errors_name_their_argument():
    f = aa.resize_many_maps
    for bad in (torch.uint8, torch.int16, torch.float16, torch.float64, torch.int64):
        with pytest.raises(NotImplementedError, match=rf"images\[0\] is {bad}"):
            f([_t(dtype=bad)], (8, 8))
    with pytest.raises(NotImplementedError, match=r"images\[1\] is torch.int16; built for torch.uint16, torch.int32, torch.float32"):
        f([_t(), _t(dtype=torch.int16)], (8, 8))
    with pytest.raises(ValueError, match=r"same dtype: images\[1\] is torch.float32, images\[0\] torch.uint16"):
        f([_t(), _t(dtype=torch.float32)], (8, 8))
    for dtype in (torch.uint16, torch.int32, torch.float32):  # resize_many_nearest's wording for wide dtypes
        with pytest.raises(NotImplementedError, match=rf"images\[0\] is {dtype} with C = 3; {dtype} maps have one channel"):
            f([_t(3, dtype=dtype)], (8, 8))
    with pytest.raises(NotImplementedError, match="maps have one channel"):
        f([], (8, 8), channels=3)
    with pytest.raises(ValueError, match=r"fill\[0\] = 65536 is outside 0..65535 \(torch.uint16\)"):
        f([_t()], (8, 8), fill=65536)
    with pytest.raises(ValueError, match=r"fill\[0\] = -1 is outside 0..65535"):
        f([_t()], (8, 8), fill=-1)
    with pytest.raises(ValueError, match="fill must be one int"):
        f([_t()], (8, 8), fill=1.5)
    with pytest.raises(ValueError, match=r"fill\[0\] = 2147483648 is outside"):
        f([_t(dtype=torch.int32)], (8, 8), fill=2 ** 31)
    for fill in (float("inf"), float("nan"), 1e39):
        with pytest.raises(ValueError, match="is not finite as torch.float32"):
            f([_t(dtype=torch.float32)], (8, 8), fill=fill)
    with pytest.raises(ValueError, match="fill must be one finite float"):
        f([_t(dtype=torch.float32)], (8, 8), fill=[1.0, 2.0])
    with pytest.raises(ValueError, match="overflow must be 'pillow' or 'clamp', got 'wrap'"):
        f([_t()], (8, 8), overflow="wrap")
    with pytest.raises(ValueError, match="overflow must be"):
        f([_t(dtype=torch.float32)], (8, 8), overflow="saturate")
    with pytest.raises(ValueError, match="sinc"):
        f([_t()], (8, 8), "sinc")
    with pytest.raises(ValueError, match=r"boxes must hold one entry per image \(1\)"):
        f([_t()], (8, 8), boxes=[None, None])
    with pytest.raises(ValueError, match="box can't exceed original image size"):
        f([_t()], (8, 8), boxes=[(0, 0, 31, 20)])
    with pytest.raises(ValueError, match=r"flips must hold one entry per image \(1\)"):
        f([_t()], (8, 8), flips=[True, False])
    with pytest.raises(ValueError, match=r"sizes must hold one entry per image \(1\)"):
        f([_t()], (8, 8), sizes=[(4, 4), (4, 4)])
    with pytest.raises(ValueError, match=r"offsets\[0\] must be two integers"):
        f([_t()], (8, 8), offsets=[(1.5, 0)])
    with pytest.raises(ValueError, match="offsets must be None, 'center'"):
        f([_t()], (8, 8), offsets="middle")
    with pytest.raises(ValueError, match="an empty list needs channels="):
        f([], (8, 8))
    with pytest.raises(RuntimeError, match="output_size equals to 2"):
        f([_t()], (8,))
    for opt in ("alpha", "reducing_gap", "out_dtype", "mean", "std", "patch"):
        with pytest.raises(NotImplementedError, match=f"{opt} is not built for maps"):
            f([_t()], (8, 8), **{opt: 1})
    with pytest.raises(TypeError, match="unexpected keyword argument 'gamma'"):
        f([_t()], (8, 8), gamma=2.2)
    with pytest.raises(RuntimeError, match="no CPU implementation"):  # a CPU tensor: there is no CPU fallback
        f([_t()], (8, 8))


def test_resize_many_keeps_its_refusals():
    for dtype in (torch.float32, torch.float16, torch.uint16, torch.int32):
        with pytest.raises(NotImplementedError, match=rf"images\[0\] is {dtype}; a list of images is Pillow's uint8 resize only"):
            aa.resize_many([_t(3, dtype=dtype)], (8, 8))
    with pytest.raises(NotImplementedError, match=r"images\[0\] is torch.float32; built for torch.uint8, torch.int16, torch.int32"):
        aa.resize_many_nearest([_t(dtype=torch.float32)], (8, 8))
    assert RESIZE_MANY_MAPS is aa.resize_many_maps


def test_empty_batch_and_meta_shapes():
    y = aa.resize_many_maps([], (8, 9), channels=1)
    assert tuple(y.shape) == (0, 1, 8, 9) and y.dtype == torch.float32
    for dtype in (torch.uint16, torch.int32, torch.float32):
        y = aa.resize_many_maps(torch.zeros((0, 1, 5, 5), dtype=dtype), (8, 9), "lanczos", overflow="clamp")
        assert tuple(y.shape) == (0, 1, 8, 9) and y.dtype == dtype
    op = torch.ops.extension_interpolate.resize_many_maps
    for dtype in (torch.uint16, torch.int32, torch.float32):
        m = [torch.empty((1, 20, 30), dtype=dtype, device="meta"), torch.empty((1, 9, 11), dtype=dtype, device="meta")]
        y = op(m, [8, 10], "bicubic", sizes=[4, 5, 8, 10], offsets=[1, -2, 0, 0], flips=[True, False], fill=3.0, overflow="clamp")
        assert tuple(y.shape) == (2, 1, 8, 10) and y.dtype == dtype and y.is_contiguous() and y.device.type == "meta"
