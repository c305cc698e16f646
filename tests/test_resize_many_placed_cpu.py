"""The placed resize_many without a GPU: the numpy restatement against the fixture (and the fixture against Pillow where it imports),
fit_sizes and "center" against literal values, the host planner aa_many_plan_placed through ctypes against the restatement's windows,
plain plans unchanged byte for byte, and every argument error, each before the device check."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import resize_many_placed_ref as ref  # noqa: E402
import resize_many_ref as plain_ref  # noqa: E402

from interpolate_antialiasing_amd import _lib, boxmath  # noqa: E402
from interpolate_antialiasing_amd import extension_interpolate as aa  # noqa: E402

G = ref.gen()
BR = plain_ref.gen()._br  # make_golden_box_reduce: box_coeffs
FILTER_IDS = {"linear": _lib.FILTER_LINEAR, "cubic": _lib.FILTER_CUBIC, "box": _lib.FILTER_BOX, "hamming": _lib.FILTER_HAMMING,
              "lanczos": _lib.FILTER_LANCZOS}
CASE_NAMES = [cs[0] for cs in G.CASES]
MAX = (2 ** 31 - 1) // 4


@pytest.mark.parametrize("name", CASE_NAMES)
def test_restatement_reproduces_the_fixture(name):
    cs = G.case(name)
    for f in cs[4]:
        for i in range(len(cs[5])):
            x = ref.item(name, i)
            ref.assert_matches_fixture(f"{name}/{f}/{i}", x, G.restated(cs, f, i, x))


def test_fixture_regenerates_from_pillow():
    pytest.importorskip("PIL.Image")
    results = [(G.crc(ref.item(cs[0], i)), G.pillow(cs, f, i, ref.item(cs[0], i))) for _, cs, f, i in G.entries()]
    fx = ref.fixture()
    for key, arr in G.pack(results).items():
        assert np.array_equal(arr, fx[key]), key


# ---- fit_sizes and "center" ------------------------------------------------------------------------------------------------------------
def test_fit_sizes_against_literal_values():
    shapes = [(480, 640), (640, 480), (500, 500), (333, 1000), (1000, 3), (375, 500)]
    assert boxmath.fit_sizes(shapes, shorter=256) == [(256, 341), (341, 256), (256, 256), (256, 768), (85333, 256), (256, 341)]
    assert boxmath.fit_sizes(shapes, longer=640) == [(480, 640), (640, 480), (640, 640), (213, 640), (640, 1), (480, 640)]
    assert boxmath.fit_sizes([(1000, 1)], longer=64) == [(64, 1)]  # the short side never vanishes
    assert boxmath.fit_sizes([], shorter=7) == []
    for kw in ({}, {"shorter": 256, "longer": 640}):
        with pytest.raises(ValueError, match="exactly one"):
            boxmath.fit_sizes(shapes, **kw)


def test_center_offsets_against_literal_values():
    # a crop: torchvision's center_crop, Python's round (half to even), so .5 goes both ways
    assert boxmath.center_offset(229, 224) == -2   # v - o = 5 -> 2.5 -> 2
    assert boxmath.center_offset(231, 224) == -4   # v - o = 7 -> 3.5 -> 4
    assert boxmath.center_offset(256, 224) == -16
    assert boxmath.center_offset(224, 224) == 0
    # a pad: the smaller half first
    assert boxmath.center_offset(219, 224) == 2 and boxmath.center_offset(217, 224) == 3 and boxmath.center_offset(1, 640) == 319
    places = aa._many_places("resize_many", [(229, 231), None, (219, 300)], "center", 3, 224, 224)
    fills = aa._many_fill("resize_many", 114, 3)
    assert places == [(229, 231, -2, -4), (224, 224, 0, 0), (219, 300, 2, -38)] and fills == [114, 114, 114]


# ---- the host planner ------------------------------------------------------------------------------------------------------------------
def _records(layout, c, items):
    recs = (_lib.ManyImage * max(len(items), 1))()
    for i, it in enumerate(items):
        h, w, box = it[:3]
        r = recs[i]
        r.data_dev = 4096 + 16 * i
        r.H, r.W = h, w
        if layout == _lib.NHWC:
            r.stride_row, r.stride_px, r.stride_ch = w * c + 5, c, 1
        else:
            r.stride_row, r.stride_px, r.stride_ch = w + 3, 1, h * (w + 3) + 1
        if box is not None:
            r.has_box = 1
            for q in range(4):
                r.box[q] = box[q]
    return recs


def _plan_placed(filter_name, layout, c, oh, ow, items, places, fill, nbytes=None):
    """items [(H, W, box, ...)]; places None or [(vh, vw, py, px)] -> (rc, buffer, workspace bytes)."""
    L = _lib.load()
    n = len(items)
    recs = _records(layout, c, items)
    precs = None
    if places is not None:
        precs = (_lib.ManyPlace * max(n, 1))()
        for i, p in enumerate(places):
            precs[i].vH, precs[i].vW, precs[i].oy, precs[i].ox = p
    fl = None if fill is None else (ctypes.c_uint8 * 4)(*(list(fill) + [0] * (4 - len(fill))))
    nbytes = L.aa_many_desc_bytes_placed(n) if nbytes is None else nbytes
    buf = (ctypes.c_uint8 * nbytes)()
    ws = ctypes.c_size_t(0)
    rc = L.aa_many_plan_placed(FILTER_IDS[filter_name], layout, n, c, oh, ow, recs, precs, fl, ctypes.addressof(buf), nbytes, ctypes.byref(ws))
    return rc, buf, ws.value


def _axis_expect(f, in_size, v, o, p, in0, in1):
    """-> (v0, m, d, hull (o, e), ksize) of one axis: the covered range from the issue's formula, the hull from the restated windows."""
    v0, v1 = max(0, -p), min(v, o - p)
    if v1 <= v0:
        return None
    k, xmin, xsize, _ = BR.box_coeffs(f, in_size, in0, in1, v)
    lo, hi = int(xmin[v0:v1].min()), int((xmin[v0:v1] + xsize[v0:v1]).max())
    assert (lo, hi) == (int(xmin[v0]), int(xmin[v1 - 1] + xsize[v1 - 1]))  # the hull is the extent of the two extreme windows
    return v0, v1 - v0, v0 + p, (lo, hi), k


@pytest.mark.parametrize("layout", [_lib.NHWC, _lib.NCHW])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_plan_covered_ranges_hulls_ksizes_units_and_workspace(name, layout):
    _, c, (oh, ow), fill, filters, items, _, _ = G.case(name)
    e = c if layout == _lib.NHWC else 1
    planes = 1 if layout == _lib.NHWC else c
    n = len(items)
    assert _lib.load().aa_many_desc_bytes_placed(n) == _lib.load().aa_many_desc_bytes(n) + n * ctypes.sizeof(_lib.ManyPlaced)
    for f in filters:
        rc, buf, ws = _plan_placed(f, layout, c, oh, ow, items, [it[3] + it[4] for it in items], fill)
        assert rc == 0, (name, f, _lib.strerror(rc))
        hd, its, prefix = _lib.many_desc_view(buf, n)
        pls = _lib.many_placed_view(buf, n)
        assert (hd.n, hd.C, hd.oH, hd.oW, hd.filter, hd.layout, hd.ws_bytes) == (n, c, oh, ow, FILTER_IDS[f], layout, ws)
        assert hd.kind == _lib.MANY_PLAN_PLACED and hd.fill == sum(v << (8 * k) for k, v in enumerate(fill))
        spans, units = [], 0
        for i, (h, w, box, (vh, vw), (py, px)) in enumerate(items):
            it, pl = its[i], pls[i]
            bx = boxmath.box_f32(box) if box is not None else (0.0, 0.0, float(w), float(h))
            ay = _axis_expect(f, h, vh, oh, py, bx[1], bx[3])
            ax = _axis_expect(f, w, vw, ow, px, bx[0], bx[2])
            assert prefix[i] == units
            assert (pl.vh, pl.vw) == (vh, vw)
            if ay is None or ax is None:  # off the canvas: all fill, no table, no work unit
                assert (pl.mh, pl.mw, it.hull_h, it.hull_w, it.ksize_h, it.ksize_w) == (0, 0, 0, 0, 0, 0), (name, f, i)
                continue
            (v0h, mh, dy, (oy, ey), kh), (v0w, mw, dx, (ox, ex), kw) = ay, ax
            assert (pl.v0h, pl.mh, pl.dy, pl.v0w, pl.mw, pl.dx) == (v0h, mh, dy, v0w, mw, dx), (name, f, i)
            assert 0 <= dy and dy + mh <= oh and 0 <= dx and dx + mw <= ow
            assert (it.oy, it.hull_h, it.ox, it.hull_w) == (oy, ey - oy, ox, ex - ox), (name, f, i)
            assert (it.ksize_h, it.ksize_w) == (kh, kw), (name, f, i)
            assert (it.in0_w, it.in0_h, it.in1_w, it.in1_h) == bx and it.box_on == int(bx != (0.0, 0.0, float(w), float(h)))
            assert it.tab_h % 16 == 0 and it.tab_w % 16 == 0 and it.inter % 16 == 0
            # the intermediate: hull_h rows of the covered columns, led so that a canvas dword is a dword of the row
            pitch = ((dx * e) % 4 + mw * e + 3) // 4 * 4
            spans += [(it.tab_h, 4 * mh * (2 + kh)), (it.tab_w, 4 * mw * (2 + kw)), (it.inter, planes * it.hull_h * pitch)]
            units += planes * (ey - oy) * ((mw + _lib.MANY_STRIP - 1) // _lib.MANY_STRIP)
        assert prefix[n] == units == hd.hunits
        spans.sort()
        for (a, la), (b, _) in zip(spans, spans[1:]):
            assert a + la <= b, (name, f, "overlapping workspace regions")
        assert spans[0][0] >= 0 and spans[-1][0] + spans[-1][1] <= ws
        if name == "p_wide":
            assert 0 < its[0].hull_w < 1000  # a few hundred columns of the 3000-column row
        if name == "p_edges":
            assert prefix[5] - prefix[4] == 0 and pls[4].mh == 0  # item 4 lies off the canvas


@pytest.mark.parametrize("layout", [_lib.NHWC, _lib.NCHW])
@pytest.mark.parametrize("name", ["m_mixed", "m_batchbox"])
def test_plain_plans_are_unchanged_byte_for_byte(name, layout):
    PG = plain_ref.gen()
    _, c, (oh, ow), items, filters, _, _ = PG.case(name)
    L = _lib.load()
    n = len(items)
    nbytes = L.aa_many_desc_bytes(n)
    for f in filters:
        want = (ctypes.c_uint8 * nbytes)()
        ws = ctypes.c_size_t(0)
        assert L.aa_many_plan(FILTER_IDS[f], layout, n, c, oh, ow, _records(layout, c, items), ctypes.addressof(want), nbytes, ctypes.byref(ws)) == 0
        for places, fill in ((None, None), (None, (114, 7, 201)), ([(oh, ow, 0, 0)] * n, None), ([(oh, ow, 0, 0)] * n, (114, 7, 201))):
            rc, got, ws2 = _plan_placed(f, layout, c, oh, ow, items, places, fill, nbytes)
            assert rc == 0 and ws2 == ws.value and bytes(got) == bytes(want), (name, f, places is None, fill)


def test_plan_argument_errors():
    ok = [(20, 30, None)]
    bad_shape = -4
    assert _plan_placed("linear", _lib.NHWC, 3, 10, 10, ok, [(7, 9, -1, 2)], (1, 2, 3))[0] == 0
    for place in ((0, 9, 0, 0), (7, -1, 0, 0), (MAX + 1, 9, 0, 0), (7, 9, MAX + 1, 0), (7, 9, 0, -MAX - 1)):
        assert _plan_placed("linear", _lib.NHWC, 3, 10, 10, ok, [place], None)[0] == bad_shape, place
    assert _plan_placed("linear", _lib.NHWC, 3, 10, 10, ok, [(7, 9, MAX, -MAX)], None)[0] == 0  # the limit itself: off the canvas, all fill
    # a placed plan needs the larger block; a plain one planned through the new entry point does not
    small = _lib.load().aa_many_desc_bytes(1)
    assert _plan_placed("linear", _lib.NHWC, 3, 10, 10, ok, [(7, 9, 0, 0)], None, small)[0] == -6
    assert _plan_placed("linear", _lib.NHWC, 3, 10, 10, ok, [(10, 10, 0, 0)], None, small)[0] == 0
    assert _plan_placed("lanczos", _lib.NHWC, 3, 10, 10, [(20000, 30, None)], [(1, 10, 0, 0)], None)[0] == -7  # AA_ERR_KSIZE, from the item's own size


def test_abi_version_stays_3_and_the_symbols_are_exported():
    L = _lib.load()
    assert L.aa_abi_version() == 3
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    for sym in ("aa_many_plan_placed", "aa_many_desc_bytes_placed"):
        assert sym in _lib.EXPORTS and hasattr(L, sym) and sym + "(" in header
    assert "typedef struct aa_many_place { int64_t vH, vW, oy, ox; } aa_many_place;" in header
    assert ctypes.sizeof(_lib.ManyPlace) == 32 and ctypes.sizeof(_lib.ManyPlaced) == 32


# ---- argument errors of the Python calls, all before any GPU use (the tensors are on the CPU) --------------------------------------------
def _u8(c=3, h=20, w=30):
    return torch.zeros((c, h, w), dtype=torch.uint8)


CALLS = [aa.resize_many, aa.resize_many_to_float]


@pytest.mark.parametrize("call", CALLS)
def test_each_bad_argument_raises_and_names_itself(call):
    imgs = [_u8(), _u8(3, 7, 9)]
    for kw, match in (
            ({"sizes": [(5, 5)]}, r"sizes must hold one entry per image \(2\)"),
            ({"offsets": [(0, 0)] * 3}, r"offsets must hold one entry per image \(2\)"),
            ({"sizes": [None, (0, 5)]}, r"sizes\[1\]"),
            ({"sizes": [(5, -1), None]}, r"sizes\[0\]"),
            ({"sizes": [None, (5.5, 5)]}, r"sizes\[1\]"),
            ({"sizes": [None, (5, 5, 5)]}, r"sizes\[1\]"),
            ({"sizes": [None, (MAX + 1, 5)]}, r"sizes\[1\].*beyond"),
            ({"offsets": [None, (0.5, 1)]}, r"offsets\[1\]"),
            ({"offsets": [("a", 1), None]}, r"offsets\[0\]"),
            ({"offsets": [None, (0, -MAX - 1)]}, r"offsets\[1\].*beyond"),
            ({"offsets": "middle"}, "offsets"),
            ({"fill": 256}, r"fill\[0\]"),
            ({"fill": -1}, r"fill\[0\]"),
            ({"fill": (1, 2, 300)}, r"fill\[2\]"),
            ({"fill": (1, 2)}, r"fill must be one int or one per channel \(3\)"),
            ({"fill": 1.5}, "fill"),
            ({"sizes": [None, None], "fill": (1, 2, 3, 4)}, r"fill must be one int or one per channel \(3\)")):
        with pytest.raises(ValueError, match=match):
            call(imgs, [10, 10], **kw)


@pytest.mark.parametrize("call", CALLS)
def test_valid_placed_call_reaches_the_device_check_and_only_then(call):
    imgs = [_u8(), _u8(3, 7, 9)]
    for kw in ({"sizes": [(12, 18), None], "offsets": "center", "fill": 114}, {"offsets": [(-3, 2), None], "fill": (1, 2, 3)},
               {"sizes": [None, (1, 1)], "offsets": [(100, 100), (9, 9)]}, {"fill": 7}):
        with pytest.raises(_lib.AAInterpError, match="ROCm GPU"):
            call(imgs, [10, 10], "bicubic", boxes=[(1.5, 2, 20, 18), None], **kw)


def test_empty_input_gives_an_empty_batch():
    y = aa.resize_many(torch.zeros((0, 3, 20, 30), dtype=torch.uint8), [10, 12], sizes=[], offsets="center", fill=(1, 2, 3))
    assert tuple(y.shape) == (0, 3, 10, 12) and y.dtype == torch.uint8


def test_torch_ops_have_meta_implementations_with_the_new_arguments():
    op = torch.ops.extension_interpolate.resize_many
    planar = [torch.empty((3, 20, 30), dtype=torch.uint8, device="meta"), torch.empty((3, 7, 9), dtype=torch.uint8, device="meta")]
    y = op(planar, [10, 12], "bilinear", None, [12, 18, 5, 6], [-1, -3, 2, 3], [114])
    assert tuple(y.shape) == (2, 3, 10, 12) and y.dtype == torch.uint8 and y.is_contiguous()
    inter = [torch.empty((20, 30, 3), dtype=torch.uint8, device="meta").permute(2, 0, 1),
             torch.empty((1, 7, 9, 3), dtype=torch.uint8, device="meta").permute(0, 3, 1, 2)]
    y = op(inter, [10, 12], "bicubic", None, sizes=[12, 18, 5, 6], offsets=[0, 0, 2, 3], fill=[1, 2, 3])
    assert tuple(y.shape) == (2, 3, 10, 12) and y.is_contiguous(memory_format=torch.channels_last) and not y.is_contiguous()
    fop = torch.ops.extension_interpolate.resize_many_to_float
    y = fop(inter, [10, 12], "bicubic", sizes=[12, 18, 5, 6], offsets=[0, 0, 2, 3], fill=[1, 2, 3], out_dtype=torch.bfloat16)
    assert tuple(y.shape) == (2, 3, 10, 12) and y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=torch.channels_last)
    y = fop(inter, [10, 12], "bicubic", sizes=[12, 18, 5, 6], out_format="nchw")
    assert y.dtype == torch.float32 and y.is_contiguous()
