"""resize_many without a GPU: the numpy restatement against the fixture (and the fixture against Pillow where it imports), the host
planner aa_many_plan through ctypes against boxmath and the restatement's coefficients, and every argument error."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import resize_many_ref as ref  # noqa: E402

from interpolate_antialiasing_amd import _lib, boxmath  # noqa: E402
from interpolate_antialiasing_amd import extension_interpolate as aa  # noqa: E402

G = ref.gen()
BR = G._br  # make_golden_box_reduce: box_coeffs, axis_hull_from_coeffs
FILTER_IDS = {"linear": _lib.FILTER_LINEAR, "cubic": _lib.FILTER_CUBIC, "box": _lib.FILTER_BOX, "hamming": _lib.FILTER_HAMMING,
              "lanczos": _lib.FILTER_LANCZOS}
CASE_NAMES = [cs[0] for cs in G.CASES]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_restatement_reproduces_the_fixture(name):
    cs = G.case(name)
    for f in cs[4]:
        for i in range(len(cs[3])):
            x = ref.item(name, i)
            ref.assert_matches_fixture(f"{name}/{f}/{i}", x, G.restated(cs, f, i, x))


def test_fixture_regenerates_from_pillow():
    pytest.importorskip("PIL.Image")
    results = [(G.crc(ref.item(cs[0], i)), G.pillow(cs, f, i, ref.item(cs[0], i))) for _, cs, f, i in G.entries()]
    fx = ref.fixture()
    for key, arr in G.pack(results).items():
        assert np.array_equal(arr, fx[key]), key


def test_fixture_holds_every_case_of_the_issue():
    by = {cs[0]: cs for cs in G.CASES}
    assert [(h, w) for h, w, _ in by["m_mixed"][3]] == [(97, 131), (33, 200), (61, 29), (12, 17), (97, 131), (30, 45), (1, 1), (1, 300), (300, 1)]
    assert by["m_mixed"][3][1][2] == (10.5, 2.25, 180.0, 30.5) and by["m_mixed"][3][4][2] == (11, 5, 56, 35) and by["m_mixed"][2] == (30, 45)
    assert set(by["m_mixed"][4]) == set(FILTER_IDS)
    assert [(h, w) for h, w, _ in by["m_wide"][3]] == [(40, 3000), (2500, 33)] and by["m_wide"][2] == (7, 9)
    assert len(by["m_tiny37"][3]) == 37 and all(3 <= h <= 20 and 3 <= w <= 20 for h, w, _ in by["m_tiny37"][3])
    assert [(h, w) for h, w, _ in by["m_strips"][3]] == [(9, 517), (8, 64)] and by["m_strips"][2] == (4, 130)
    assert by["m_batchbox"][6] and sum(1 for it in by["m_batchbox"][3] if it[2] is None) == 1 and len(by["m_batchbox"][3]) == 5
    for c in (1, 2, 4):
        assert by[f"m_c{c}"][1] == c and sum(1 for it in by[f"m_c{c}"][3] if it[2] is not None) == 1


# ---- the host planner ----------------------------------------------------------------------------------------------------------------
def _plan(filter_name, layout, c, oh, ow, items):
    """items [(H, W, box or None)] -> (rc, header, item records, prefix, workspace bytes); the data pointers are never dereferenced."""
    L = _lib.load()
    n = len(items)
    recs = (_lib.ManyImage * max(n, 1))()
    for i, (h, w, box) in enumerate(items):
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
    nbytes = L.aa_many_desc_bytes(n)
    assert nbytes == ctypes.sizeof(_lib.ManyHeader) + n * ctypes.sizeof(_lib.ManyItem) + 8 * (n + 1)
    buf = (ctypes.c_uint8 * nbytes)()
    ws = ctypes.c_size_t(0)
    rc = L.aa_many_plan(FILTER_IDS[filter_name], layout, n, c, oh, ow, recs, ctypes.addressof(buf), nbytes, ctypes.byref(ws))
    hd, its, prefix = _lib.many_desc_view(buf, n)
    return rc, hd, its, prefix, ws.value


def _axis_expect(name, in_size, out, in0, in1):
    """-> (hull (o, e), ksize) of one axis from boxmath and from the restatement's coefficients, which must agree."""
    k, xmin, xsize, _ = BR.box_coeffs(name, in_size, in0, in1, out)
    hull = boxmath.axis_hull(in_size, out, in0, in1, name)
    assert hull == BR.axis_hull_from_coeffs(xmin, xsize)
    return hull, k


@pytest.mark.parametrize("layout", [_lib.NHWC, _lib.NCHW])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_plan_hulls_ksizes_offsets_and_prefix_sums(name, layout):
    _, c, (oh, ow), items, filters, _, _ = G.case(name)
    e = c if layout == _lib.NHWC else 1
    planes = 1 if layout == _lib.NHWC else c
    pitch = (ow * e + 3) // 4 * 4
    nstrips = (ow + _lib.MANY_STRIP - 1) // _lib.MANY_STRIP
    for f in filters:
        rc, hd, its, prefix, ws = _plan(f, layout, c, oh, ow, items)
        assert rc == 0, (name, f, _lib.strerror(rc))
        assert (hd.n, hd.C, hd.oH, hd.oW, hd.filter, hd.layout, hd.ws_bytes) == (len(items), c, oh, ow, FILTER_IDS[f], layout, ws)
        spans, units = [], 0
        for i, (h, w, box) in enumerate(items):
            it = its[i]
            bx = boxmath.box_f32(box) if box is not None else (0.0, 0.0, float(w), float(h))
            (oy, ey), kh = _axis_expect(f, h, oh, bx[1], bx[3])
            (ox, ex), kw = _axis_expect(f, w, ow, bx[0], bx[2])
            assert (it.oy, it.hull_h, it.ox, it.hull_w) == (oy, ey - oy, ox, ex - ox), (name, f, i)
            assert (it.ksize_h, it.ksize_w) == (kh, kw), (name, f, i)
            assert (it.in0_w, it.in0_h, it.in1_w, it.in1_h) == bx
            assert it.box_on == int(bx != (0.0, 0.0, float(w), float(h)))
            assert it.src == 4096 + 16 * i and it.row_stride == (w * c + 5 if layout == _lib.NHWC else w + 3)
            spans += [(it.tab_h, 4 * oh * (2 + kh)), (it.tab_w, 4 * ow * (2 + kw)), (it.inter, planes * it.hull_h * pitch)]
            assert it.tab_h % 16 == 0 and it.tab_w % 16 == 0 and it.inter % 16 == 0
            assert prefix[i] == units
            units += planes * (ey - oy) * nstrips
        assert prefix[len(items)] == units == hd.hunits
        spans.sort()
        for (a, la), (b, _) in zip(spans, spans[1:]):
            assert a + la <= b, (name, f, "overlapping workspace regions")
        assert spans[0][0] >= 0 and spans[-1][0] + spans[-1][1] <= ws


def _random_draws(count, seed):
    rng = np.random.default_rng(seed)
    names = ["linear", "cubic", "box", "hamming", "lanczos"]
    made = 0
    while made < count:
        w, h = int(rng.integers(1, 3000)), int(rng.integers(1, 3000))
        ow, oh = int(rng.integers(1, 300)), int(rng.integers(1, 300))
        x0, x1 = sorted(rng.uniform(0, w, 2))
        y0, y1 = sorted(rng.uniform(0, h, 2))
        pick = rng.random()
        if pick < 0.25:
            box = None
        elif pick < 0.5:
            box = (float(int(x0)), float(int(y0)), float(math.ceil(x1)), float(math.ceil(y1)))
        else:
            box = (x0, y0, x1, y1)
        if box is not None:
            b32 = tuple(boxmath.f32(v) for v in box)
            if b32[2] - b32[0] <= 0 or b32[3] - b32[1] <= 0 or b32[2] > w or b32[3] > h:
                continue
        made += 1
        yield w, h, ow, oh, box, names[int(rng.integers(0, 5))]


def test_plan_hull_is_the_extent_of_the_restated_windows_400_draws():
    checked = 0
    for w, h, ow, oh, box, f in _random_draws(440, 21):
        rc, hd, its, prefix, ws = _plan(f, _lib.NHWC, 3, oh, ow, [(h, w, box)])
        bx = boxmath.box_f32(box) if box is not None else (0.0, 0.0, float(w), float(h))
        widest = max(int(math.ceil(boxmath.SUPPORT[f] * max(boxmath.f32(b - a) / out, 1.0))) * 2 + 1
                     for a, b, out in ((bx[0], bx[2], ow), (bx[1], bx[3], oh)))
        if widest > 4096:  # AA_MAX_KSIZE, the library's bound on a window, as in the single-image call
            assert rc == -7, (w, h, ow, oh, box, f, rc)
            continue
        assert rc == 0, (w, h, ow, oh, box, f, rc)
        it = its[0]
        for in_size, out, a, b, o, hull, ks in ((w, ow, bx[0], bx[2], it.ox, it.hull_w, it.ksize_w), (h, oh, bx[1], bx[3], it.oy, it.hull_h, it.ksize_h)):
            k, xmin, xsize, _ = BR.box_coeffs(f, in_size, a, b, out)
            assert (o, o + hull) == BR.axis_hull_from_coeffs(xmin, xsize) == (int(xmin[0]), int(xmin[-1] + xsize[-1])), (w, h, ow, oh, box, f)
            assert ks == k and int(xsize.max()) <= k
        checked += 1
    assert checked >= 400


def test_plan_argument_errors():
    ok = [(20, 30, None)]
    assert _plan("linear", _lib.NHWC, 3, 10, 10, ok)[0] == 0
    assert _plan("linear", _lib.NHWC, 3, 10, 10, [])[0] == 0  # an empty list plans to an empty workspace
    assert _plan("linear", _lib.NHWC, 3, 10, 10, [])[4] == 0
    bad_shape = -4
    assert _plan("linear", _lib.NHWC, 5, 10, 10, ok)[0] == bad_shape  # C
    assert _plan("linear", _lib.NHWC, 0, 10, 10, ok)[0] == bad_shape
    assert _plan("linear", _lib.NHWC, 3, 0, 10, ok)[0] == bad_shape
    assert _plan("linear", _lib.NHWC, 3, 10, 10, [(20, 30, (12.0, 5.0, 12.0, 9.0))])[0] == bad_shape  # empty
    assert _plan("linear", _lib.NHWC, 3, 10, 10, [(20, 30, (12.0, 5.0, 12.0 + 1e-9, 9.0))])[0] == bad_shape  # empty as floats
    assert _plan("linear", _lib.NHWC, 3, 10, 10, [(20, 30, (0.0, 0.0, 30.5, 20.0))])[0] == bad_shape  # beyond the image
    assert _plan("linear", _lib.NHWC, 3, 10, 10, [(20, 30, (0.0, 0.0, 30.0, 21.0))])[0] == bad_shape  # (x first: 30 wide, 20 high)
    assert _plan("linear", _lib.NHWC, 3, 10, 10, [(20, 30, (-1.0, 0.0, 20.0, 20.0))])[0] == bad_shape
    assert _plan("linear", _lib.NHWC, 3, 10, 10, [(20, 30, (float("nan"), 0.0, 20.0, 20.0))])[0] == bad_shape
    assert _plan("linear", _lib.NHWC, 3, 10, 10, [(2 ** 29, 30, None)])[0] == bad_shape  # beyond int32 / 4 within one image
    assert _plan("lanczos", _lib.NHWC, 3, 1, 10, [(20000, 30, None)])[0] == -7  # AA_ERR_KSIZE
    L = _lib.load()
    recs = (_lib.ManyImage * 1)()
    recs[0].data_dev, recs[0].H, recs[0].W = 4096, 20, 30
    recs[0].stride_row, recs[0].stride_px, recs[0].stride_ch = 30, 1, 600  # planes handed to the interleaved class
    buf = (ctypes.c_uint8 * L.aa_many_desc_bytes(1))()
    ws = ctypes.c_size_t(0)
    assert L.aa_many_plan(0, _lib.NHWC, 1, 3, 10, 10, recs, ctypes.addressof(buf), len(buf), ctypes.byref(ws)) == _lib.ERR_STRIDES
    assert L.aa_many_plan(0, _lib.NCHW, 1, 3, 10, 10, recs, ctypes.addressof(buf), len(buf), ctypes.byref(ws)) == 0
    assert L.aa_many_plan(0, _lib.NCHW, 1, 3, 10, 10, recs, ctypes.addressof(buf), len(buf) - 1, ctypes.byref(ws)) == -6  # block too small
    assert L.aa_many_plan(9, _lib.NCHW, 1, 3, 10, 10, recs, ctypes.addressof(buf), len(buf), ctypes.byref(ws)) == -1
    for sym in ("aa_many_desc_bytes", "aa_many_plan", "aa_resample_many_u8"):
        assert sym in _lib.EXPORTS and hasattr(L, sym)
    # the launch entry point checks its arguments against the plan before anything else
    assert L.aa_many_plan(0, _lib.NCHW, 1, 3, 10, 10, recs, ctypes.addressof(buf), len(buf), ctypes.byref(ws)) == 0
    one = ctypes.c_void_p(4096)
    assert L.aa_resample_many_u8(ctypes.addressof(buf), one, 2, 3, 10, 10, _lib.NCHW, one, one, ws.value, None) == bad_shape  # another n
    assert L.aa_resample_many_u8(ctypes.addressof(buf), one, 1, 3, 10, 10, _lib.NCHW, one, one, ws.value - 1, None) == -6
    assert L.aa_resample_many_u8(ctypes.addressof(buf), None, 1, 3, 10, 10, _lib.NCHW, one, one, ws.value, None) == -5


# ---- argument errors of the Python call, all before any GPU use (the tensors are on the CPU) ---------------------------------------------
def _u8(c=3, h=20, w=30):
    return torch.zeros((c, h, w), dtype=torch.uint8)


def test_mixed_channels_and_wrong_dtype():
    with pytest.raises(ValueError, match="same C"):
        aa.resize_many([_u8(3), _u8(4)], [10, 10])
    with pytest.raises(NotImplementedError, match="float32"):
        aa.resize_many([_u8(3), torch.zeros((3, 20, 30))], [10, 10])
    with pytest.raises(NotImplementedError, match="float16"):
        aa.resize_many(torch.zeros((2, 3, 20, 30), dtype=torch.float16), [10, 10])
    with pytest.raises(ValueError, match="1 to 4 channels"):
        aa.resize_many([_u8(5)], [10, 10])
    with pytest.raises(RuntimeError, match=r"\[C, H, W\]"):
        aa.resize_many([torch.zeros((20, 30), dtype=torch.uint8)], [10, 10])
    with pytest.raises(ValueError, match="bilinearish"):
        aa.resize_many([_u8()], [10, 10], "bilinearish")
    with pytest.raises(ValueError, match="channels="):
        aa.resize_many([], [10, 10])
    with pytest.raises(ValueError, match="one entry per image"):
        aa.resize_many([_u8(), _u8()], [10, 10], boxes=[None])


def test_bad_boxes_have_pillows_wording():
    imgs = [_u8(), _u8()]
    with pytest.raises(ValueError, match="box offset can't be negative"):
        aa.resize_many(imgs, [10, 10], boxes=[None, (-1, 0, 20, 20)])
    with pytest.raises(ValueError, match="box can't exceed original image size"):
        aa.resize_many(imgs, [10, 10], boxes=[(0, 0, 30.5, 20), None])
    with pytest.raises(ValueError, match="box can't exceed original image size"):
        aa.resize_many(imgs, [10, 10], boxes=[None, (0, 0, 30, 21)])  # (x first: 30 wide, 20 high)
    with pytest.raises(ValueError, match="box can't be empty"):
        aa.resize_many(imgs, [10, 10], boxes=[(12, 5, 11, 9), None])
    with pytest.raises(ValueError, match="box can't be empty"):  # not empty in double, empty as the floats Pillow's C takes
        aa.resize_many(imgs, [10, 10], boxes=[None, (12.0, 5, 12.0 + 1e-9, 9)])
    with pytest.raises(ValueError, match="x0, y0, x1, y1"):
        aa.resize_many(imgs, [10, 10], boxes=[None, (1, 2, 3)])


@pytest.mark.parametrize("kw", [{"alpha": True}, {"reducing_gap": 2.0}, {"uint8_mode": "harness"}, {"out_dtype": torch.float32},
                                {"out_format": "nhwc"}, {"mean": [0.0] * 3, "std": [1.0] * 3}, {"align_corners": True},
                                {"scale_factors": [0.5, 0.5]}])
def test_each_unsupported_option_names_itself(kw):
    with pytest.raises(NotImplementedError, match=next(iter(kw))):
        aa.resize_many([_u8()], [10, 10], **kw)


def test_harness_mode_set_globally_is_refused():
    prev = aa.get_uint8_mode()
    aa.set_uint8_mode("harness")
    try:
        with pytest.raises(NotImplementedError, match="harness"):
            aa.resize_many([_u8()], [10, 10])
    finally:
        aa.set_uint8_mode(prev)


def test_valid_call_reaches_the_device_check_and_only_then():
    with pytest.raises(_lib.AAInterpError, match="ROCm GPU"):
        aa.resize_many([_u8(), _u8(3, 7, 9)], [10, 10], "bicubic", boxes=[(1.5, 2, 20, 18), None])
    with pytest.raises(_lib.AAInterpError, match="ROCm GPU"):
        aa.resize_many(torch.zeros((2, 3, 20, 30), dtype=torch.uint8), [10, 10])


def test_empty_input_gives_an_empty_batch():
    y = aa.resize_many(torch.zeros((0, 3, 20, 30), dtype=torch.uint8), [10, 12])
    assert tuple(y.shape) == (0, 3, 10, 12) and y.dtype == torch.uint8


def test_torch_op_has_a_meta_implementation():
    op = torch.ops.extension_interpolate.resize_many
    planar = [torch.empty((3, 20, 30), dtype=torch.uint8, device="meta"), torch.empty((3, 7, 9), dtype=torch.uint8, device="meta")]
    y = op(planar, [10, 12])
    assert tuple(y.shape) == (2, 3, 10, 12) and y.dtype == torch.uint8 and y.is_contiguous()
    inter = [torch.empty((20, 30, 3), dtype=torch.uint8, device="meta").permute(2, 0, 1),
             torch.empty((1, 7, 9, 3), dtype=torch.uint8, device="meta").permute(0, 3, 1, 2)]
    y = op(inter, [10, 12], "bicubic", [0.0, 0.0, 30.0, 20.0, 1.5, 2.0, 8.0, 6.5])
    assert tuple(y.shape) == (2, 3, 10, 12) and y.is_contiguous(memory_format=torch.channels_last) and not y.is_contiguous()
    gray = [torch.empty((1, 20, 30), dtype=torch.uint8, device="meta")]
    assert op(gray, [10, 12]).is_contiguous()
