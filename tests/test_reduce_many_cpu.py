"""reduce_many / reduce_many_for_resize without a GPU: boxmath.reducing_plans against what the fixture recorded from Pillow, the
restatement against the fixture (and the fixture against Pillow where it imports), the host planner aa_reduce_many_plan through ctypes,
the torch op's Meta implementation, and every argument error, each before any GPU use."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kit_golden  # noqa: E402
import reduce_many_ref as ref  # noqa: E402

from interpolate_antialiasing_amd import _lib, boxmath  # noqa: E402
from interpolate_antialiasing_amd import extension_interpolate as aa  # noqa: E402

G = ref.gen()
ALL_CASES = [cs[0] for cs in G.CASES]


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES)
def test_restatement_reproduces_the_fixture(name):
    cs = G.case(name)
    for f in cs[5]:
        for i in range(len(cs[4])):
            key = f"{name}/{f}/{i}"
            out, red = G.restated(cs, f, i, ref.item(name, i))
            ref.assert_resize_matches_fixture(key, ref.item(name, i), out)
            assert (red is None) == (ref.plan(name, f, i) is None), key
            if red is not None:
                ref.assert_reduce_matches_fixture(key, red)


def test_fixture_regenerates_from_pillow():
    pytest.importorskip("PIL.Image")
    results = []
    for _, cs, f, i in G.entries():
        x = ref.item(cs[0], i)
        out, red = G.pillow(cs, f, i, x)
        factor, rb, sb = G.plan(cs, f, i)
        results.append((G.crc(x), out, red, (factor, rb, sb) if rb is not None else None))
    fx = ref.fixture()
    for key, arr in G.pack(results).items():
        assert np.array_equal(arr, fx[key]), key


def test_fixture_holds_every_case_of_the_issue():
    by = {cs[0]: cs for cs in G.CASES}
    assert [it[:2] for it in by["g_mixed"][4]] == [(400, 610), (97, 131), (300, 100), (64, 900), (401, 613), (30, 45), (1, 1)]
    assert by["g_mixed"][4][3][2] == (10.5, 2.25, 880.0, 60.5) and by["g_mixed"][4][4][2] == (11, 5, 560, 395)
    assert by["g_mixed"][2] == (30, 45) and by["g_mixed"][3] == 2.0 and set(by["g_mixed"][5]) == set(G.FILTER_NAMES)
    assert [it[:2] for it in by["g_seam"][4]] == [(9, 1501), (8, 64)] and by["g_seam"][2] == (4, 375)
    assert [it[:2] for it in by["g_tall"][4]] == [(530, 9), (5, 9)] and by["g_tall"][1] == 1 and by["g_tall"][3] == 1.0
    assert [it[:2] for it in by["g_wideblock"][4]] == [(7, 3001), (40, 33)] and by["g_wideblock"][2] == (3, 2)
    for c in (1, 2, 4):
        assert by[f"g_c{c}"][1] == c and by[f"g_c{c}"][2] == (19, 77) and by[f"g_c{c}"][5] == ("cubic", "box")
    assert len(by["g_tiny37"][4]) == 37 and all(3 <= h <= 60 and 3 <= w <= 60 for h, w, _ in by["g_tiny37"][4])
    assert by["g_batchbox"][7] and len(by["g_batchbox"][4]) == 5 and sum(1 for it in by["g_batchbox"][4] if it[2] is None) == 1
    # the factors the issue's table names, as the fixture recorded them from Pillow's own arithmetic
    for cs in G.CASES:
        for f in cs[5]:
            for i, want in cs[9].items():
                got = ref.plan(cs[0], f, i)
                assert (got[0] if got is not None else None) == want, (cs[0], f, i, got, want)
    assert ref.plan("g_mixed", "linear", 4)[1][2] - ref.plan("g_mixed", "linear", 4)[1][0] not in range(0, 10000, 6)  # a partial right block
    for name in ("g_fit", "g_patch"):
        assert len({ref.plan(name, by[name][5][0], i)[0] for i in range(7) if ref.plan(name, by[name][5][0], i) is not None}) >= 2
    assert by["g_fit"][8] == boxmath.fit_sizes(ref.shapes("g_fit"), shorter=40)
    assert by["g_patch"][8] == boxmath.fit_patch_sizes(ref.shapes("g_patch"), G.PATCH, max_tokens=48)
    assert os.path.getsize(os.path.join(kit_golden.GOLDEN, "reduce_many.npz")) < 100 * 1024


# ---- boxmath.reducing_plans ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES)
def test_reducing_plans_equal_what_pillow_computed(name):
    cs = G.case(name)
    for f in cs[5]:
        plans = boxmath.reducing_plans(ref.shapes(name), cs[2], ref.MODE[f], ref.boxes(name), cs[8], cs[3])
        assert len(plans) == ref.count(name)
        for i, p in enumerate(plans):
            want = ref.plan(name, f, i)
            if want is None:
                assert p is None, (name, f, i, p)
                continue
            assert tuple(p[0]) == want[0] and tuple(p[1]) == want[1], (name, f, i, p, want)
            assert tuple(p[2]) == want[2], (name, f, i, p[2], want[2])  # (the same double operations: equal, not close)
            assert all(isinstance(v, int) for v in p[1]) and all(isinstance(v, float) for v in p[2])
        one = [boxmath.reducing_plan(w, h, (cs[8][i] if cs[8] else cs[2])[1], (cs[8][i] if cs[8] else cs[2])[0], f,
                                     boxmath.check_box(b, w, h) if b is not None else (0.0, 0.0, float(w), float(h)), cs[3])
               for i, ((h, w), b) in enumerate(zip(ref.shapes(name), ref.boxes(name)))]
        for i, (p, q) in enumerate(zip(plans, one)):
            assert p == q or (p is None and ref.shapes(name)[i] == tuple(cs[8][i] if cs[8] else cs[2])), (name, f, i)  # per item: reducing_plan


def test_reducing_plans_a_copy_is_none_whatever_the_gap():
    assert boxmath.reducing_plans([(30, 45)], (30, 45), "bicubic", reducing_gap=1.0) == [None]
    assert boxmath.reducing_plans([(300, 450)], (30, 45), "bicubic", sizes=[(300, 450)], reducing_gap=1.0) == [None]
    assert boxmath.reducing_plans([(300, 450)], (30, 45), "bicubic", boxes=[(0, 0, 450, 300)], reducing_gap=1.0)[0][0] == (10, 10)
    assert boxmath.reducing_plans([], (30, 45), "bicubic") == []


def test_reducing_plans_errors_name_the_item():
    shapes = [(40, 50)] * 4
    with pytest.raises(ValueError, match=r"boxes\[3\].*exceed"):
        boxmath.reducing_plans(shapes, (4, 5), "bilinear", boxes=[None, None, None, (0, 0, 51, 40)])
    with pytest.raises(ValueError, match=r"boxes\[1\].*empty"):
        boxmath.reducing_plans(shapes, (4, 5), "bilinear", boxes=[None, (5, 5, 5, 9), None, None])
    with pytest.raises(ValueError, match="one entry per image"):
        boxmath.reducing_plans(shapes, (4, 5), "bilinear", boxes=[None])
    with pytest.raises(ValueError, match="one entry per image"):
        boxmath.reducing_plans(shapes, (4, 5), "bilinear", sizes=[(4, 5)])
    with pytest.raises(ValueError, match="reducing_gap must be 1.0 or greater"):
        boxmath.reducing_plans(shapes, (4, 5), "bilinear", reducing_gap=0.5)
    with pytest.raises(ValueError, match=r"images\[3\]: fx \* fy = \d+ beyond 65536"):
        boxmath.reducing_plans([(40, 50)] * 3 + [(1000, 1000)], (1, 1), "bilinear", reducing_gap=1.0)
    with pytest.raises(ValueError):
        boxmath.reducing_plans(shapes, (4, 5), "area")


# ---- the host planner ------------------------------------------------------------------------------------------------------------------------
def _plan(layout, c, items, desc_slack=0, n=None):
    """items [(H, W, box, (fx, fy))] -> (rc, header, records, prefix, arena bytes, offsets); the data pointers are never dereferenced."""
    L = _lib.load()
    n = len(items) if n is None else n
    recs = (_lib.ReduceItem * max(len(items), 1))()
    for r, (h, w, box, (fx, fy)) in zip(recs, items):
        r.data_dev = 1 << 20
        r.H, r.W = h, w
        if layout == _lib.NHWC:
            r.stride_row, r.stride_px, r.stride_ch = w * c, c, 1
        else:
            r.stride_row, r.stride_px, r.stride_ch = w, 1, h * w
        r.box[0], r.box[1], r.box[2], r.box[3] = box if box is not None else (0, 0, w, h)
        r.fx, r.fy = fx, fy
    size = L.aa_reduce_many_desc_bytes(n) + desc_slack
    buf = (ctypes.c_uint8 * max(size, 1))()
    arena = ctypes.c_size_t(0)
    offs = (ctypes.c_int64 * max(n, 1))()
    rc = L.aa_reduce_many_plan(layout, n, c, recs, ctypes.addressof(buf), size, ctypes.byref(arena), offs)
    hd, its, prefix = _lib.reduce_many_desc_view(buf, n) if rc == 0 else (None, None, None)
    return rc, hd, its, prefix, arena.value, list(offs)[:n], recs, buf


@pytest.mark.parametrize("layout", [_lib.NHWC, _lib.NCHW])
def test_plan_offsets_sizes_tiles_and_multipliers(layout):
    c = 3
    items = [(401, 613, (11, 5, 560, 395), (6, 6)), (9, 1501, None, (2, 1)), (7, 3001, None, (1500, 2)), (5, 9, None, (1, 1)), (530, 9, None, (2, 265))]
    rc, hd, its, prefix, arena, offs, _, _ = _plan(layout, c, items)
    assert rc == 0
    e, planes = (c, 1) if layout == _lib.NHWC else (1, c)
    assert (hd.n, hd.C, hd.layout, hd.E, hd.planes) == (len(items), c, layout, e, planes)
    end, units = 0, 0
    for i, (h, w, box, (fx, fy)) in enumerate(items):
        x0, y0, x1, y1 = box if box is not None else (0, 0, w, h)
        rw, rh = boxmath.reduced_size((x0, y0, x1, y1), (fx, fy))
        it = its[i]
        assert offs[i] % 16 == 0 and offs[i] >= end and it.out_off == offs[i]  # aligned, disjoint, in order
        end = offs[i] + c * rh * rw
        assert (it.bw, it.bh, it.fx, it.fy, it.rw, it.rh) == (x1 - x0, y1 - y0, fx, fy, rw, rh)
        assert it.src == (1 << 20) + y0 * (w * e) + x0 * e and it.row_pitch == w * e
        assert it.plane_pitch == (0 if layout == _lib.NHWC else h * w)
        sx = 4096 // (fx * e) if fx * e <= 4096 else 1
        assert it.sx == sx and it.xtiles == -(-rw // sx)
        fxr, fyb = (x1 - x0) % fx or fx, (y1 - y0) % fy or fy
        assert list(it.mult) == [G._br.reduce_mult(fx * fy), G._br.reduce_mult(fxr * fy), G._br.reduce_mult(fx * fyb), G._br.reduce_mult(fxr * fyb)]
        assert prefix[i] == units
        units += planes * rh * it.xtiles
    assert prefix[len(items)] == units == hd.units
    assert arena >= end and arena == hd.arena_bytes and arena % 16 == 0  # covers the last item


def test_plan_error_codes():
    ok = [(20, 30, None, (2, 2))]
    bad_shape, strides, null, workspace = -4, _lib.ERR_STRIDES, -5, -6
    assert _plan(_lib.NHWC, 3, ok)[0] == 0
    assert _plan(_lib.NHWC, 5, ok)[0] == bad_shape and _plan(_lib.NCHW, 0, ok)[0] == bad_shape          # C outside 1..4
    assert _plan(_lib.NHWC, 3, [(20, 30, (5, 5, 5, 9), (2, 2))])[0] == bad_shape                          # an empty box
    assert _plan(_lib.NHWC, 3, [(20, 30, (0, 0, 31, 20), (2, 2))])[0] == bad_shape                        # a box beyond the image
    assert _plan(_lib.NHWC, 3, [(20, 30, (-1, 0, 30, 20), (2, 2))])[0] == bad_shape
    assert _plan(_lib.NHWC, 3, [(20, 30, None, (0, 2))])[0] == bad_shape                                  # a factor below 1
    assert _plan(_lib.NHWC, 3, [(20, 30, None, (257, 256))])[0] == bad_shape                              # a block beyond 65536
    assert _plan(_lib.NHWC, 3, [(20, 30, None, (256, 256))])[0] == 0
    assert _plan(_lib.NCHW, 1, [(20, (2 ** 31 - 1) // 4 + 1, None, (2, 2))])[0] == bad_shape              # a size beyond INT32_MAX / 4
    big = ((2 ** 31 - 1) // 4, (2 ** 31 - 1) // 4, None, (1, 1))
    assert _plan(_lib.NCHW, 1, [big])[0] == bad_shape                                                     # more work units than one grid
    assert _plan(2, 3, ok)[0] == -3                                                                       # AA_ERR_BAD_LAYOUT
    assert _plan(_lib.NHWC, 3, ok, desc_slack=-1)[0] == workspace
    L = _lib.load()
    rc, _, _, _, _, _, recs, buf = _plan(_lib.NHWC, 3, ok)
    arena, offs = ctypes.c_size_t(0), (ctypes.c_int64 * 1)()
    assert L.aa_reduce_many_plan(_lib.NHWC, 1, 3, recs, None, len(buf), ctypes.byref(arena), offs) == null
    assert L.aa_reduce_many_plan(_lib.NHWC, 1, 3, None, ctypes.addressof(buf), len(buf), ctypes.byref(arena), offs) == null
    assert L.aa_reduce_many_plan(_lib.NHWC, 1, 3, recs, ctypes.addressof(buf), len(buf), None, offs) == null
    assert L.aa_reduce_many_plan(_lib.NHWC, 1, 3, recs, ctypes.addressof(buf), len(buf), ctypes.byref(arena), None) == null
    recs[0].data_dev = None
    assert L.aa_reduce_many_plan(_lib.NHWC, 1, 3, recs, ctypes.addressof(buf), len(buf), ctypes.byref(arena), offs) == null
    recs[0].data_dev = 1 << 20
    recs[0].stride_px = 4  # not the class's
    assert L.aa_reduce_many_plan(_lib.NHWC, 1, 3, recs, ctypes.addressof(buf), len(buf), ctypes.byref(arena), offs) == strides
    recs[0].stride_px, recs[0].stride_ch = 3, 2
    assert L.aa_reduce_many_plan(_lib.NHWC, 1, 3, recs, ctypes.addressof(buf), len(buf), ctypes.byref(arena), offs) == strides
    recs[0].stride_px, recs[0].stride_ch = 3, 1
    assert L.aa_reduce_many_plan(_lib.NCHW, 1, 3, recs, ctypes.addressof(buf), len(buf), ctypes.byref(arena), offs) == strides


def test_plan_of_nothing_and_the_launch_checks():
    L = _lib.load()
    rc, hd, _, prefix, arena, _, _, buf0 = _plan(_lib.NHWC, 3, [], n=0)
    assert rc == 0 and hd.n == 0 and arena == 0 and prefix[0] == 0
    assert L.aa_reduce_many_u8(ctypes.addressof(buf0), None, None, 0, None) == 0  # n == 0 launches nothing
    rc, hd, _, _, arena, _, _, buf = _plan(_lib.NHWC, 3, [(20, 30, None, (2, 2))])
    one = ctypes.c_void_p(4096)  # (never dereferenced: the checks come first)
    assert L.aa_reduce_many_u8(None, one, one, arena, None) == -5
    assert L.aa_reduce_many_u8(ctypes.addressof(buf), None, one, arena, None) == -5
    assert L.aa_reduce_many_u8(ctypes.addressof(buf), one, None, arena, None) == -5
    assert L.aa_reduce_many_u8(ctypes.addressof(buf), one, one, arena - 1, None) == -6
    assert L.aa_reduce_many_u8(ctypes.addressof(buf), one, ctypes.c_void_p(4104), arena, None) == -4  # the arena is not 16-byte aligned
    hd.magic = 0
    assert L.aa_reduce_many_u8(ctypes.addressof(buf), one, one, arena, None) == -4  # not a block of this plan


def test_abi_is_additive():
    L = _lib.load()
    assert L.aa_abi_version() == 3
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    assert "#define AA_INTERP_ABI_VERSION 3 " in header
    for sym in ("aa_reduce_many_desc_bytes", "aa_reduce_many_plan", "aa_reduce_many_u8"):
        assert sym in _lib.EXPORTS and hasattr(L, sym) and sym + "(" in header
    assert "} aa_reduce_item;" in header
    assert ctypes.sizeof(_lib.ReduceItem) == 88 and ctypes.sizeof(_lib.ReduceManyHeader) == 64 and ctypes.sizeof(_lib.ReduceManyItem) == 80
    assert L.aa_reduce_many_desc_bytes(3) == 64 + 3 * 80 + 4 * 8 and L.aa_reduce_many_desc_bytes(-1) == 0


# ---- the torch op -------------------------------------------------------------------------------------------------------------------------
def test_meta_implementation_gives_the_shapes_and_strides():
    hwc = torch.empty((40, 61, 3), dtype=torch.uint8, device="meta").permute(2, 0, 1)
    hwc2 = torch.empty((9, 1501, 3), dtype=torch.uint8, device="meta").permute(2, 0, 1)
    outs = torch.ops.extension_interpolate.reduce_many([hwc, hwc2], [6, 6, 2, 1], [11, 5, 56, 35, 0, 0, 1501, 9])
    assert [tuple(o.shape) for o in outs] == [(3, 5, 8), (3, 9, 751)]
    assert [o.stride() for o in outs] == [(1, 24, 3), (1, 2253, 3)] and all(o.dtype == torch.uint8 and o.device.type == "meta" for o in outs)
    planar = torch.empty((3, 40, 61), dtype=torch.uint8, device="meta")
    outs = torch.ops.extension_interpolate.reduce_many([planar, planar], [3], None)
    assert [tuple(o.shape) for o in outs] == [(3, 14, 21)] * 2 and outs[0].is_contiguous()
    outs = torch.ops.extension_interpolate.reduce_many([planar], [3, 5])
    assert tuple(outs[0].shape) == (3, 8, 21)
    with pytest.raises(ValueError, match="factors"):
        torch.ops.extension_interpolate.reduce_many([planar, planar, planar], [2, 2, 2, 2])
    with pytest.raises(ValueError, match="boxes"):
        torch.ops.extension_interpolate.reduce_many([planar], [2], [0, 0, 4])


# ---- argument errors of the Python calls, all before any GPU use (the tensors are on the CPU) ---------------------------------------------
def _u8(c=3, h=20, w=30):
    return torch.zeros((c, h, w), dtype=torch.uint8)


def test_nothing_in_nothing_out():
    assert aa.reduce_many([], 2) == []
    assert aa.reduce_many(torch.zeros((0, 3, 8, 8), dtype=torch.uint8), (2, 3)) == []
    assert aa.reduce_many_for_resize([], [10, 10], "bicubic") == ([], None)


def test_reduce_many_bad_arguments_name_themselves():
    imgs = [_u8(), _u8(3, 7, 9), _u8()]
    with pytest.raises(ValueError, match=r"factors\[1\].*greater than 0"):
        aa.reduce_many(imgs, [2, 0, 3])
    with pytest.raises(ValueError, match=r"factors\[2\].*65536"):
        aa.reduce_many(imgs, [2, 2, (257, 256)])
    with pytest.raises(ValueError, match="factors must be one int, one .fx, fy. or one entry per image .3., got 4"):
        aa.reduce_many(imgs, [2, 2, 2, 2])
    with pytest.raises(ValueError, match=r"boxes\[1\].*exceed"):
        aa.reduce_many(imgs, 2, boxes=[None, (0, 0, 10, 7), None])
    with pytest.raises(ValueError, match=r"boxes\[0\].*integers"):
        aa.reduce_many(imgs, 2, boxes=[(0.5, 0, 10, 7), None, None])
    with pytest.raises(ValueError, match="boxes must hold one entry per image"):
        aa.reduce_many(imgs, 2, boxes=[None])
    with pytest.raises(NotImplementedError, match=r"images\[1\] is torch.float32"):
        aa.reduce_many([_u8(), _u8().float()], 2)
    with pytest.raises(ValueError, match=r"same C: images\[1\] has 1"):
        aa.reduce_many([_u8(), _u8(1)], 2)
    with pytest.raises(ValueError, match="1 to 4 channels"):
        aa.reduce_many([_u8(5)], 2)
    with pytest.raises(TypeError, match=r"images\[0\] must be Tensor"):
        aa.reduce_many([np.zeros((3, 4, 4), np.uint8)], 2)
    with pytest.raises(_lib.AAInterpError, match="ROCm GPU"):  # everything else was fine: the device check comes last
        aa.reduce_many(imgs, [2, (1, 3), 5], boxes=[None, (1, 1, 8, 6), None])


def test_reduce_many_for_resize_checks_everything_before_the_device():
    imgs = [_u8(3, 200, 300), _u8(3, 20, 30)]
    call = aa.reduce_many_for_resize
    with pytest.raises(ValueError, match="area"):
        call(imgs, [10, 10], "area")
    with pytest.raises(RuntimeError, match="output_size equals to 2"):
        call(imgs, [10], "bicubic")
    with pytest.raises(RuntimeError, match="greater than 0"):
        call(imgs, [0, 10], "bicubic")
    with pytest.raises(ValueError, match="reducing_gap must be 1.0 or greater"):
        call(imgs, [10, 10], "bicubic", reducing_gap=0.99)
    with pytest.raises(ValueError, match=r"boxes\[1\].*exceed"):
        call(imgs, [10, 10], "bicubic", boxes=[None, (0, 0, 31, 20)])
    with pytest.raises(ValueError, match=r"sizes\[0\] must be two integers"):
        call(imgs, [10, 10], "bicubic", sizes=[(1.5, 2), None])
    with pytest.raises(ValueError, match=r"sizes\[1\] = \(0, 4\) must be positive"):
        call(imgs, [10, 10], "bicubic", sizes=[None, (0, 4)])
    with pytest.raises(ValueError, match="sizes must hold one entry per image"):
        call(imgs, [10, 10], "bicubic", sizes=[None])
    with pytest.raises(NotImplementedError, match=r"images\[1\] is torch.float16"):
        call([imgs[0], imgs[1].half()], [10, 10], "bicubic")
    with pytest.raises(ValueError, match=r"images\[1\]: fx \* fy = \d+ beyond 65536"):
        call([_u8(), _u8(1, 1000, 1000)[:, :, :].expand(3, 1000, 1000)], [1, 1], "bicubic", reducing_gap=1.0)
    with pytest.raises(TypeError):
        call(imgs, [10, 10], "bicubic", alpha=True)  # there is no alpha: Pillow drops reducing_gap for RGBA / LA
    with pytest.raises(_lib.AAInterpError, match="ROCm GPU"):  # the device check is reached only after all the others
        call(imgs, [10, 10], "bicubic", boxes=[(0.5, 0.5, 290.0, 190.0), None], sizes=[None, (5, 5)], reducing_gap=2.0)
    with pytest.raises(_lib.AAInterpError, match="ROCm GPU"):  # ... also when nothing would be reduced
        call([_u8()], [10, 10], "bicubic")


def test_harness_mode_set_globally_is_refused():
    prev = aa.get_uint8_mode()
    aa.set_uint8_mode("harness")
    try:
        with pytest.raises(NotImplementedError, match="harness"):
            aa.reduce_many([_u8()], 2)
        with pytest.raises(NotImplementedError, match="harness"):
            aa.reduce_many_for_resize([_u8()], [10, 10])
    finally:
        aa.set_uint8_mode(prev)


def test_resize_many_still_refuses_the_keyword_and_points_here():
    with pytest.raises(NotImplementedError, match="reducing_gap") as e:
        aa.resize_many([_u8()], [10, 10], reducing_gap=2.0)
    assert "reduce_many_for_resize" in str(e.value)
    assert "reduce_many" in aa.__all__ and "reduce_many_for_resize" in aa.__all__
