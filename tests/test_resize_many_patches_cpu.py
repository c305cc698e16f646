"""resize_many_to_patches without a GPU: the numpy restatement and patchify against the fixture (and the fixture against Pillow where it
imports), the boxmath helpers against literal values, the host planner aa_many_plan_patches through ctypes (rows, work units, status
codes, workspace against the placed plan's), every argument error of the Python call before the device check, the Meta shapes of the
torch op, and N = 0."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import resize_many_patches_ref as ref  # noqa: E402

from interpolate_antialiasing_amd import _lib  # noqa: E402
from interpolate_antialiasing_amd import extension_interpolate as aa  # noqa: E402
from interpolate_antialiasing_amd.boxmath import fit_patch_sizes, patch_grids, token_offsets  # noqa: E402

G = ref.gen()
FILTER_IDS = {"linear": _lib.FILTER_LINEAR, "cubic": _lib.FILTER_CUBIC, "box": _lib.FILTER_BOX, "hamming": _lib.FILTER_HAMMING,
              "lanczos": _lib.FILTER_LANCZOS}
MAX = (2 ** 31 - 1) // 4
BAD_LAYOUT, BAD_SHAPE, NULL, WORKSPACE = -3, -4, -5, -6
VPIXELS = {1: 1024, 2: 512, 3: 256, 4: 256}  # pixels per image unit of the patch-writing pass, by bytes per pixel of a row
PAD_ELEMS = 4096                             # elements per pad unit


@pytest.mark.parametrize("name", ref.names())
def test_restatement_and_numpy_patchify_reproduce_the_fixture(name):
    for f in ref.case(name)[3]:
        for fmt in G.FORMATS:
            ref.assert_matches_fixture(f"{name}/{f}/{fmt}", ref.tokens(name, f, fmt))


def test_fixture_regenerates_from_pillow():
    pytest.importorskip("PIL.Image")
    fx = ref.fixture()
    for key, cs, f, fmt in G.entries():
        tok = G.pillow(cs, f, fmt, ref.inputs(cs[0]))
        _, out_crc, samples = G.expected(fx, key)
        assert G.crc(tok) == out_crc and np.array_equal(G.sample(tok).ravel(), samples), key


def test_patchify_against_a_hand_written_case():
    """[2, 4, 2] image, patch (1, 2): pixel value = 100 * y + 10 * x + c."""
    r = np.array([[[100 * y + 10 * x + c for c in range(2)] for x in range(4)] for y in range(2)], np.uint8)
    assert G.patchify(r, (1, 2), "cpp").tolist() == [[0, 10, 1, 11], [20, 30, 21, 31], [100, 110, 101, 111], [120, 130, 121, 131]]
    assert G.patchify(r, (1, 2), "ppc").tolist() == [[0, 1, 10, 11], [20, 21, 30, 31], [100, 101, 110, 111], [120, 121, 130, 131]]
    # the definition's own view / permute / reshape, in torch, on an NCHW float image
    t = torch.from_numpy(r.astype(np.float32)).permute(2, 0, 1)
    p = t.reshape(2, 2, 1, 2, 2)
    assert torch.equal(p.permute(1, 3, 0, 2, 4).reshape(4, 4), torch.from_numpy(G.patchify(r, (1, 2), "cpp").astype(np.float32)))
    assert torch.equal(p.permute(1, 3, 2, 4, 0).reshape(4, 4), torch.from_numpy(G.patchify(r, (1, 2), "ppc").astype(np.float32)))


# ---- boxmath ---------------------------------------------------------------------------------------------------------------------------
def test_fit_patch_sizes_known_answers():
    assert fit_patch_sizes([(480, 640), (1080, 1920), (20, 30), (7, 500), (333, 500)], (14, 14), min_tokens=4, max_tokens=256) == [
        (182, 252), (168, 294), (28, 42), (14, 504), (182, 266)]
    assert fit_patch_sizes([(480, 640), (1080, 1920)], (16, 16), min_tokens=1, max_tokens=1024) == [(432, 576), (384, 672)]
    assert fit_patch_sizes([], (14, 14)) == []
    assert fit_patch_sizes([(3, 3)], (14, 16)) == [(14, 16)]  # at least one patch per axis


def test_fit_patch_sizes_gives_multiples_within_the_token_bounds():
    rng = np.random.default_rng(5)
    shapes = [(int(rng.integers(30, 2000)), int(rng.integers(30, 2000))) for _ in range(200)]  # aspect ratios the bounds allow
    for patch, lo, hi in (((14, 14), 4, 256), ((16, 16), 1, 1024), ((8, 12), 16, 300)):
        out = fit_patch_sizes(shapes, patch, min_tokens=lo, max_tokens=hi)
        for (h, w), (vh, vw) in zip(shapes, out):
            assert vh % patch[0] == 0 and vw % patch[1] == 0 and vh > 0 and vw > 0
            assert lo <= (vh // patch[0]) * (vw // patch[1]) <= hi, ((h, w), (vh, vw), patch, lo, hi)


def test_patch_grids_and_token_offsets():
    sizes = [(42, 56), (14, 14), (70, 28)]
    assert patch_grids(sizes, (14, 14)) == [(3, 4), (1, 1), (5, 2)]
    assert token_offsets(sizes, (14, 14)) == [0, 12, 13, 23]
    assert token_offsets([], (2, 3)) == [0]
    assert patch_grids([(4, 9)], (2, 3)) == [(2, 3)]
    with pytest.raises(ValueError, match=r"sizes\[1\].*multiple of the patch"):
        patch_grids([(28, 28), (28, 30)], (14, 14))
    with pytest.raises(ValueError, match=r"sizes\[0\].*multiple of the patch"):
        token_offsets([(15, 28)], (14, 14))
    with pytest.raises(ValueError, match="patch"):
        patch_grids([(28, 28)], (0, 14))
    for name in ref.names():
        assert token_offsets(ref.sizes(name), ref.case(name)[2]) == [0] + list(np.cumsum(ref.token_counts(name)))


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
        if len(it) > 4 and it[4]:
            r.flags = _lib.MANY_FLIP_X
    return recs


def _plan(filter_id, layout, c, patch, items, sizes, pad_to=0, nbytes=None, n=None):
    """-> (rc, buffer, workspace bytes, rows)"""
    L = _lib.load()
    n = len(items) if n is None else n
    flat = (ctypes.c_int64 * max(2 * len(sizes), 1))(*[v for s in sizes for v in s])
    nbytes = L.aa_many_desc_bytes_patches(max(n, 0)) if nbytes is None else nbytes
    buf = (ctypes.c_uint8 * max(nbytes, 1))()
    ws, rows = ctypes.c_size_t(0), ctypes.c_int64(-1)
    rc = L.aa_many_plan_patches(filter_id, layout, n, c, patch[0], patch[1], _records(layout, c, items), flat, pad_to, ctypes.addressof(buf), nbytes,
                                ctypes.byref(ws), ctypes.byref(rows))
    return rc, buf, ws.value, rows.value


@pytest.mark.parametrize("layout", [_lib.NHWC, _lib.NCHW])
@pytest.mark.parametrize("name", ref.names())
def test_plan_rows_units_and_records(name, layout):
    _, c, (ph, pw), filters, items, _, _ = ref.case(name)
    n, sizes, counts = len(items), ref.sizes(name), ref.token_counts(name)
    e = c if layout == _lib.NHWC else 1
    planes = 1 if layout == _lib.NHWC else c
    d = c * ph * pw
    L = _lib.load()
    assert L.aa_many_desc_bytes_patches(n) == L.aa_many_desc_bytes_placed(n) + 16 * (n + 1) + 16
    for pad_to in (0, max(counts), max(counts) + 3):
        rc, buf, ws, rows = _plan(FILTER_IDS[filters[0]], layout, c, (ph, pw), items, sizes, pad_to)
        assert rc == 0, (name, _lib.strerror(rc))
        assert rows == (n * pad_to if pad_to else sum(counts))
        hd, its, _ = _lib.many_desc_view(buf, n)
        pls = _lib.many_placed_view(buf, n)
        vprefix, tok0 = _lib.many_patch_view(buf, n)
        assert (hd.n, hd.C, hd.layout, hd.ws_bytes, hd.kind) == (n, c, layout, ws, _lib.MANY_PLAN_PLACED | _lib.MANY_PLAN_PATCHES)
        assert (hd.oH, hd.oW) == (max(s[0] for s in sizes), max(s[1] for s in sizes))
        units, row = 0, 0
        for i, (vh, vw) in enumerate(sizes):
            assert (pls[i].vh, pls[i].vw, pls[i].v0h, pls[i].v0w, pls[i].mh, pls[i].mw, pls[i].dy, pls[i].dx) == (vh, vw, 0, 0, vh, vw, 0, 0)
            assert its[i].flags == int(items[i][4])
            assert vprefix[i] == units and tok0[i] == (i * pad_to if pad_to else row)
            units += planes * vh * ((vw + VPIXELS[e] - 1) // VPIXELS[e])
            if pad_to:
                units += ((pad_to - counts[i]) * d + PAD_ELEMS - 1) // PAD_ELEMS
            row += counts[i]
        assert vprefix[n] == units and tok0[n] == rows


@pytest.mark.parametrize("layout", [_lib.NHWC, _lib.NCHW])
def test_one_item_plans_the_workspace_of_the_placed_plan_on_its_own_canvas(layout):
    L = _lib.load()
    for f in ("linear", "lanczos"):
        for (h, w, box), (vh, vw), patch in (((97, 131, None), (42, 56), (14, 14)), ((33, 200, (10.5, 2.25, 180.0, 30.5)), (28, 84), (14, 14)),
                                              ((12, 17, None), (28, 42), (2, 3)), ((8, 2000, None), (2, 1026), (2, 3))):
            rc, _, ws, rows = _plan(FILTER_IDS[f], layout, 3, patch, [(h, w, box)], [(vh, vw)])
            assert rc == 0 and rows == (vh // patch[0]) * (vw // patch[1])
            nbytes = L.aa_many_desc_bytes_placed(1)
            buf = (ctypes.c_uint8 * nbytes)()
            place = (_lib.ManyPlace * 1)()
            place[0].vH, place[0].vW, place[0].oy, place[0].ox = vh, vw, 0, 0
            want = ctypes.c_size_t(0)
            assert L.aa_many_plan_placed(FILTER_IDS[f], layout, 1, 3, vh, vw, _records(layout, 3, [(h, w, box)]), place, None,
                                         ctypes.addressof(buf), nbytes, ctypes.byref(want)) == 0
            assert ws == want.value, (f, h, w, vh, vw)


def test_plan_status_codes():
    ok, size = [(20, 30, None)], [(28, 42)]
    lin = _lib.FILTER_LINEAR
    assert _plan(lin, _lib.NHWC, 3, (14, 14), ok, size)[0] == 0
    assert _plan(7, _lib.NHWC, 3, (14, 14), ok, size)[0] == -1                      # AA_ERR_BAD_FILTER
    assert _plan(lin, 2, 3, (14, 14), ok, size)[0] == BAD_LAYOUT
    for patch in ((0, 14), (14, -1), (MAX + 1, 14)):
        assert _plan(lin, _lib.NHWC, 3, patch, ok, size)[0] == BAD_SHAPE, patch
    for bad in ((28, 43), (27, 42), (0, 42), (28, -14), (14 * (MAX // 14 + 1), 14)):   # indivisible, non-positive, beyond the bound
        assert _plan(lin, _lib.NHWC, 3, (14, 14), ok, [bad])[0] == BAD_SHAPE, bad
    assert _plan(lin, _lib.NHWC, 5, (14, 14), ok, size)[0] == BAD_SHAPE               # C outside 1..4
    assert _plan(lin, _lib.NHWC, 3, (14, 14), ok, size, pad_to=6)[0] == 0             # T = 6 fits exactly
    assert _plan(lin, _lib.NHWC, 3, (14, 14), ok, size, pad_to=5)[0] == BAD_SHAPE     # T_i > pad_to
    assert _plan(lin, _lib.NHWC, 3, (14, 14), ok, size, pad_to=-1)[0] == BAD_SHAPE
    assert _plan(lin, _lib.NHWC, 3, (14, 14), ok, size, nbytes=_lib.load().aa_many_desc_bytes_placed(1))[0] == WORKSPACE
    assert _plan(lin, _lib.NHWC, 3, (14, 14), ok, size, n=-1)[0] == BAD_SHAPE
    assert _plan(lin, _lib.NHWC, 3, (14, 14), [(20, 30, (5, 5, 40, 10))], size)[0] == BAD_SHAPE   # the box beyond the image, as aa_many_plan
    # a grid beyond 2^31 - 1 units: one planar item of 3 planes x 536870910 rows x 1 strip fits, two do not; and the pad units of a huge pad_to
    tall = (MAX // 2) * 2
    assert _plan(lin, _lib.NCHW, 3, (2, 2), [(9, 11, None)], [(tall, 2)])[0] == 0
    assert _plan(lin, _lib.NCHW, 3, (2, 2), [(9, 11, None)] * 2, [(tall, 2)] * 2)[0] == BAD_SHAPE
    assert _plan(lin, _lib.NHWC, 4, (64, 64), [(9, 11, None)] * 400, [(64, 64)] * 400, pad_to=2 ** 31 - 1)[0] == BAD_SHAPE
    L = _lib.load()
    ws, rows = ctypes.c_size_t(0), ctypes.c_int64(0)
    assert L.aa_many_plan_patches(lin, _lib.NHWC, 1, 3, 14, 14, _records(_lib.NHWC, 3, ok), (ctypes.c_int64 * 2)(28, 42), 0, None, 4096,
                                  ctypes.byref(ws), ctypes.byref(rows)) == NULL


def test_launch_checks_come_before_any_launch():
    """No device here: every one of these must be refused by the argument checks (a launch would fail otherwise)."""
    L = _lib.load()
    rc, buf, ws, _ = _plan(_lib.FILTER_LINEAR, _lib.NHWC, 3, (14, 14), [(20, 30, None)], [(28, 42)])
    assert rc == 0
    host = ctypes.addressof(buf)
    cv = _lib.Convert()

    def launch(desc=host, conv=cv, fmt=_lib.PATCH_CPP, out=4096, ws_dev=8192, ws_bytes=1 << 30, dev=1024):
        return L.aa_resample_many_u8_to_patches(desc, dev, out, ws_dev, ws_bytes, ctypes.byref(conv) if conv is not None else None, fmt, None)

    assert launch(fmt=2) == BAD_LAYOUT                     # unknown patch format
    assert launch(desc=None) == NULL and launch(conv=None) == NULL
    cv.flags = _lib.FLAG_FAST
    assert launch() == BAD_SHAPE
    cv.flags = _lib.FLAG_OUT_F16 | _lib.FLAG_OUT_BF16
    assert launch() == _lib.ERR_BAD_DTYPE
    cv.flags = 0
    assert launch(out=4098) == BAD_SHAPE                   # a float32 output on a 2-byte boundary
    assert launch(ws_bytes=ws - 1) == WORKSPACE
    assert launch(ws_dev=8200) == BAD_SHAPE and launch(dev=1028) == BAD_SHAPE and launch(out=None) == NULL
    # a placed plan's block is not a patch plan's
    nbytes = L.aa_many_desc_bytes_patches(1)
    placed = (ctypes.c_uint8 * nbytes)()
    place = (_lib.ManyPlace * 1)()
    place[0].vH, place[0].vW, place[0].oy, place[0].ox = 28, 42, 1, 0
    w2 = ctypes.c_size_t(0)
    assert L.aa_many_plan_placed(_lib.FILTER_LINEAR, _lib.NHWC, 1, 3, 30, 45, _records(_lib.NHWC, 3, [(20, 30, None)]), place, None,
                                 ctypes.addressof(placed), nbytes, ctypes.byref(w2)) == 0
    assert launch(desc=ctypes.addressof(placed)) == BAD_SHAPE
    # n == 0 launches nothing
    rc, empty, _, rows = _plan(_lib.FILTER_LINEAR, _lib.NHWC, 3, (14, 14), [], [], pad_to=7)
    assert rc == 0 and rows == 0 and launch(desc=ctypes.addressof(empty), out=None, ws_dev=None, dev=None) == 0


def test_abi_version_stays_3_and_the_symbols_are_exported():
    L = _lib.load()
    assert L.aa_abi_version() == 3
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    for sym in ("aa_many_desc_bytes_patches", "aa_many_plan_patches", "aa_resample_many_u8_to_patches"):
        assert sym in _lib.EXPORTS and hasattr(L, sym) and sym + "(" in header
    assert ctypes.sizeof(_lib.Convert) == 44 and ctypes.sizeof(_lib.ManyImage) == 88 and ctypes.sizeof(_lib.ManyPlace) == 32


# ---- argument errors of the Python call, all before any GPU use (the tensors are on the CPU) ------------------------------------------------
def _u8(c=3, h=20, w=30):
    return torch.zeros((c, h, w), dtype=torch.uint8)


def test_each_bad_argument_raises_and_names_itself():
    imgs = [_u8(), _u8(3, 7, 9)]
    good = [(28, 42), (14, 14)]
    call = aa.resize_many_to_patches
    for args, kw, exc, match in (
            ((imgs, (14, 14)), {}, ValueError, "sizes is required"),
            ((imgs, (14, 14)), {"sizes": [(28, 42)]}, ValueError, r"sizes must hold one entry per image \(2\)"),
            ((imgs, (14, 14)), {"sizes": [(28, 42), (14, 15)]}, ValueError, r"sizes\[1\] = \(14, 15\) is not a multiple of the patch \(14, 14\)"),
            ((imgs, (14, 14)), {"sizes": [(27, 42), (14, 14)]}, ValueError, r"sizes\[0\]"),
            ((imgs, (14, 14)), {"sizes": [(28, 42), (0, 14)]}, ValueError, r"sizes\[1\].*positive"),
            ((imgs, (14, 14)), {"sizes": [(28, 42), (14.5, 14)]}, ValueError, r"sizes\[1\] must be two integers"),
            ((imgs, (14, 14)), {"sizes": [(28, 42), (14 * (MAX // 14 + 1), 14)]}, ValueError, r"sizes\[1\].*beyond"),
            ((imgs, (14,)), {"sizes": good}, ValueError, "patch must be two integers"),
            ((imgs, (0, 14)), {"sizes": good}, ValueError, "patch.*positive"),
            ((imgs, (14, 1.5)), {"sizes": good}, ValueError, "patch must be two integers"),
            ((imgs, (14, 14)), {"sizes": good, "pad_to": 5}, ValueError, r"sizes\[0\] = \(28, 42\) is 6 tokens, more than pad_to = 5"),
            ((imgs, (14, 14)), {"sizes": good, "pad_to": 0}, ValueError, "pad_to"),
            ((imgs, (14, 14)), {"sizes": good, "pad_to": 6.5}, ValueError, "pad_to"),
            ((imgs, (14, 14)), {"sizes": good, "patch_format": "pcp"}, ValueError, "patch_format"),
            ((imgs, (14, 14), "area"), {"sizes": good}, ValueError, "area"),
            ((imgs, (14, 14)), {"sizes": good, "boxes": [None]}, ValueError, r"boxes must hold one entry per image \(2\)"),
            ((imgs, (14, 14)), {"sizes": good, "boxes": [(0, 0, 31, 5), None]}, ValueError, "box can't exceed original image size"),
            ((imgs, (14, 14)), {"sizes": good, "flips": [True]}, ValueError, r"flips must hold one entry per image \(2\)"),
            ((imgs, (14, 14)), {"sizes": good, "mean": [1, 2, 3]}, ValueError, "mean and std must be given together"),
            ((imgs, (14, 14)), {"sizes": good, "mean": [1, 2, 3], "std": [1, 0, 1]}, ValueError, r"std\[1\]"),
            ((imgs, (14, 14)), {"sizes": good, "mean": [1, 2], "std": [1, 2]}, RuntimeError, "one value per channel"),
            ((imgs, (14, 14)), {"sizes": good, "out_dtype": torch.float64}, NotImplementedError, "out_dtype"),
            (([_u8(), _u8(4, 7, 9)], (14, 14)), {"sizes": good}, ValueError, "same C"),
            (([_u8(), _u8(3, 7, 9).float()], (14, 14)), {"sizes": good}, NotImplementedError, r"images\[1\] is torch.float32"),
            (([_u8(), torch.zeros((7, 9), dtype=torch.uint8)], (14, 14)), {"sizes": good}, RuntimeError, r"images\[1\] must be"),
            (([_u8(5)], (14, 14)), {"sizes": [(14, 14)]}, ValueError, "1 to 4 channels"),
            (([], (14, 14)), {"sizes": []}, ValueError, "channels="),
            ((torch.zeros((20, 30), dtype=torch.uint8), (14, 14)), {"sizes": []}, RuntimeError, "one tensor must be")):
        with pytest.raises(exc, match=match):
            call(*args, **kw)
    for bad in ("output_size", "offsets", "fill"):  # each item is its own canvas
        with pytest.raises(TypeError):
            call(imgs, (14, 14), sizes=good, **{bad: [10, 10]})


def test_valid_call_reaches_the_device_check_and_only_then():
    imgs = [_u8(), _u8(3, 7, 9)]
    for kw in ({"sizes": [(28, 42), (14, 14)]}, {"sizes": (28, 28)}, {"sizes": [(28, 42), (14, 14)], "pad_to": 6, "patch_format": "ppc"},
               {"sizes": [(28, 42), (14, 14)], "flips": [1, 0], "boxes": [(1.5, 2, 20, 18), None], "mean": [1, 2, 3], "std": [4, 5, 6],
                "out_dtype": torch.bfloat16}):
        with pytest.raises(_lib.AAInterpError, match="ROCm GPU"):
            aa.resize_many_to_patches(imgs, (14, 14), "bicubic", **kw)


def test_empty_input():
    y = aa.resize_many_to_patches(torch.zeros((0, 3, 20, 30), dtype=torch.uint8), (14, 16), sizes=[])
    assert tuple(y.shape) == (0, 3 * 14 * 16) and y.dtype == torch.float32
    y = aa.resize_many_to_patches([], (2, 3), sizes=[], channels=4, pad_to=9, out_dtype=torch.float16, patch_format="ppc")
    assert tuple(y.shape) == (0, 9, 24) and y.dtype == torch.float16
    with pytest.raises(ValueError, match="channels="):
        aa.resize_many_to_patches([], (2, 3), sizes=[])


def test_torch_op_has_a_meta_implementation_whose_shape_comes_from_the_sizes():
    op = torch.ops.extension_interpolate.resize_many_to_patches
    imgs = [torch.empty((3, 20, 30), dtype=torch.uint8, device="meta"), torch.empty((1, 3, 7, 9), dtype=torch.uint8, device="meta")]
    y = op(imgs, [14, 14], "bicubic", [28, 42, 14, 14], None, None, "cpp", None, None, None, None)
    assert tuple(y.shape) == (7, 588) and y.dtype == torch.float32 and y.is_contiguous()
    y = op(imgs, [14, 14], "bilinear", [28, 42, 14, 14], None, [True, False], "ppc", 9, torch.bfloat16, [1.0, 2.0, 3.0], [1.0, 2.0, 3.0])
    assert tuple(y.shape) == (2, 9, 588) and y.dtype == torch.bfloat16
    y = op(imgs, [2, 3], "bilinear", [4, 6], None, None, "cpp", None, torch.float16, None, None)  # one pair for all items
    assert tuple(y.shape) == (8, 18) and y.dtype == torch.float16
    with pytest.raises(ValueError, match=r"sizes\[1\]"):
        op(imgs, [14, 14], "bicubic", [28, 42, 14, 15], None, None, "cpp", None, None, None, None)
    with pytest.raises(ValueError, match="more than pad_to"):
        op(imgs, [14, 14], "bicubic", [28, 42, 14, 14], None, None, "cpp", 5, None, None, None)
