"""Launch-shape sweep (-m gpu): every fused family under every band count and strip grouping, against the oracle.

Which launch shape a call gets (csrc/aa_launch_shape.h) follows from the batch size and the card, so at the sizes the other tests use the
kernels run with the largest band count and, mostly, single-strip workgroups.  Here aa_set_launch_shape forces the others: for each case the
expected result is computed ONCE from oracle/ (Pillow's bytes, the reference-order float forward; the dense float64 adjoint of
tests/backward_ref.py for the gradients), then the product runs under

    ybands in {1, 2, 3, the largest the output height allows}  x  spb in {1, 2, the plan's own, one that leaves a short last group}

(the groupings whose rings fit a workgroup's 64 KiB of LDS: here all of them), and every run asserts

  (a) the result is BIT-IDENTICAL to the expected one — no kernel's per-pixel arithmetic depends on bands or grouping, so there is no
      tolerance (the tolerance mode and the gradients: bit-identical across shapes, and within their existing bound of the reference);
  (b) aa_last_launch_shape reports the family, spb and ybands that were asked for: every requested shape is honoured
      (tests/test_launch_shape_override_cpu.py shows that this does not depend on the device);
  (c) last_variant is the intended kernel;

under the guarded allocator of tests/guard_ref.py (no byte outside a buffer written, every output element written).  Shapes: output
heights of 41 (five uneven bands of 8 or 9 rows) from 86, and of 83 from 40 for growing heights (16 rows per band in the float kernel);
widths that give five strips, so that groups of 2 and of 4 leave a short last group, and one three-strip case per family.  The strip
count is read from aa_last_launch_shape, not restated.  Inputs are seeded noise with rows of all 0 / all 255 at the top, the bottom and
across the middle band seams (floats: rows a million times larger than their neighbours).  Batch 2."""
import functools
import itertools

import numpy as np
import pytest
import torch

import backward_ref as R
import box_reduce_ref as BR
import guard_ref as G
import kit_golden
import kit_gpu
import oracle
from kit_golden import MEAN, STD

pytestmark = pytest.mark.gpu

TAG = {torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32", torch.float64: "f64"}
ROWS_PER_BAND = {0: 8, 1: 8, 2: 8, 3: 16}  # aa_launch_family -> output rows a band has at least
SEEN = {}  # family -> shapes that ran, printed at the end of the module


def _report():
    from interpolate_antialiasing_amd import _lib

    _lib.set_launch_shape(0, 0)
    print("\nlaunch-shape sweep, (spb, ybands) that ran:", {k: sorted(v) for k, v in sorted(SEEN.items())})


aa = kit_gpu.aa_fixture(_report)
lib = kit_gpu.lib_fixture()


@pytest.fixture(autouse=True)
def knobs_restored(lib):
    """Every hook at its default before and after each test, whatever the test did."""
    prev = lib.set_fused(1), lib.set_store_form(-1), lib.set_plane_groups(1)
    lib.set_launch_shape(0, 0)
    yield
    lib.set_launch_shape(0, 0)
    lib.set_fused(prev[0])
    lib.set_store_form(prev[1])
    lib.set_plane_groups(prev[2])


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def _marked_rows(h):
    """(rows of the low extreme, rows of the high one): the image's first and last rows and runs across its middle, where the seams of
    2, 3 and 5 bands fall."""
    lo = [0, h - 2, h // 2, h // 2 + 1, h // 3 + 1, (3 * h) // 5]
    hi = [1, h - 1, h // 2 - 1, h // 2 - 2, h // 3, (2 * h) // 5, (4 * h) // 5]
    return lo, hi


@functools.lru_cache(maxsize=None)
def _u8(shape, seed):
    x = np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)
    lo, hi = _marked_rows(shape[2])
    x[:, :, lo, :] = 0
    x[:, :, hi, :] = 255
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _f32(shape, seed, big=1.0e6, signed=True):
    """Noise in [0, 255) with rows `big` times larger, of either sign unless signed is false, and rows of exact zeros."""
    x = (np.random.default_rng(seed).random(shape, dtype=np.float32) * 255).astype(np.float32)
    lo, hi = _marked_rows(shape[2])
    x[:, :, lo[:3], :] *= np.float32(-big if signed else big)
    x[:, :, lo[3:], :] = 0
    x[:, :, hi, :] *= np.float32(big)
    x.setflags(write=False)
    return x


def _float_input(shape, seed, dtype, cl=False, signed=True):
    """A finite float input of `dtype` (float16: large rows of 200 times their neighbours, inside its range) and the float32 / float64
    array the oracle resamples: the input itself, widened exactly."""
    x = torch.from_numpy(np.array(_f32(shape, seed, 200.0 if dtype == torch.float16 else 1.0e6, signed))).to(dtype)
    assert bool(torch.isfinite(x).all())
    wide = x.double().numpy() if dtype == torch.float64 else x.float().numpy()
    xg = x.cuda()
    return (xg.contiguous(memory_format=torch.channels_last) if cl else xg), np.ascontiguousarray(wide)


def _fwd(aa, filt):
    return {"linear": aa.linear_forward, "cubic": aa.cubic_forward, "lanczos": aa.lanczos_forward}[filt]


# ---- the sweep ------------------------------------------------------------------------------------------------------------------------
def _guarded(monkeypatch, lib, call, tag):
    """One call under the guarded allocator (uint8 results: into 0xFF- and into 0x00-filled memory) -> (result, variant, question,
    answer of the launch).  No byte outside a buffer changed and every output element was written."""
    runs = []
    for fill in (0xFF, 0x00):
        with G.guarded(monkeypatch, 0, fill) as rec:
            try:
                with kit_gpu.gpu_error_ends_the_session(tag):
                    y = call()
                    v = lib.last_variant()
                    shape = lib.last_launch_shape()
                    rec.check()
            except G.GuardViolation as e:
                raise AssertionError(f"{tag}: {e}") from None
        runs.append((y, v, shape))
        if y.dtype != torch.uint8:
            break
    y, v, shape = runs[0]
    if y.dtype == torch.uint8:
        n = G.unwritten_u8(y, runs[1][0])
        assert n == 0, f"{tag}: {n} of {y.numel()} output bytes were never written"
    else:
        n = G.unwritten_float(y)
        assert n == 0, f"{tag}: {n} of {y.numel()} output elements were never written (still the NaN fill)"
    assert shape is not None, (tag, v, "no fused launch")
    return y, v, shape[0], shape[1]


def _sweep(monkeypatch, lib, call, family, variant, verify, tag, nstrips=5, groupings=True, lds_differs_by=None):
    """call() under every shape of the sweep; verify(result, what) holds the result to the case's expectation.  -> {(spb, ybands): result}.
    The model's own shape runs first: its question names the strips, the plan's grouping and the LDS of a strip."""
    y, v, q, out = _guarded(monkeypatch, lib, call, (tag, "the model's shape"))
    assert v == variant and q.family == family, (tag, v, q.family)
    assert q.nstrips == nstrips, (tag, "strips", q.nstrips)
    verify(y, (tag, "the model's shape", out.strips_per_block, out.ybands))
    top = min(max(q.oH // ROWS_PER_BAND[family], 1), 64)
    assert top >= 4, (tag, q.oH)
    ybs = [1, 2, 3, top]
    if groupings:
        short = next(s for s in (4, 2, 3, 5, 6, 7, 8) if s < nstrips and nstrips % s != 0)
        spbs = sorted({1, 2, int(q.strips_per_block), short})
        assert nstrips % 2 != 0 and all(s <= min(nstrips, 8) and q.lds * s <= 65536 for s in spbs), (tag, spbs, q.lds)
    else:
        spbs = [0]
    got = {}
    if lds_differs_by is not None:
        assert q.lds - lds_differs_by[0] == lds_differs_by[1], (tag, q.lds, lds_differs_by)
    try:
        for s, yb in itertools.product(spbs, ybs):
            lib.set_launch_shape(s, yb)
            what = (tag, "spb", s, "ybands", yb)
            y, v, q2, out = _guarded(monkeypatch, lib, call, what)
            assert q2.family == family and q2.nstrips == nstrips, (what, q2.family, q2.nstrips)
            assert out.ybands == yb and out.strips_per_block == (s if groupings else 1), (what, "ran", out.strips_per_block, out.ybands)  # (b)
            assert out.groups == q2.items * yb
            assert v == variant, (what, v)  # (c)
            verify(y, what)  # (a)
            got[(s, yb)] = y
            SEEN.setdefault(family, set()).add((out.strips_per_block, out.ybands))
    finally:
        lib.set_launch_shape(0, 0)
    return got


def _exactly(want):
    want = want if isinstance(want, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(want))
    return lambda y, what: kit_gpu.assert_bits(y, want, what)


# ------------------------------------------------------------------------------------------------ 1. the fused uint8 kernel (v3)
# (id, C, channels_last, filter, (N, H, W), (oH, oW), strips, plane groups, keyword arguments)
V3_CASES = [
    ("nhwc3_periodic", 3, True, "linear", (2, 86, 600), (41, 300), 5, 1, {}),        # even W: eight rows are whole 16-byte pieces
    ("nhwc3_odd_w", 3, True, "linear", (2, 86, 601), (41, 300), 5, 1, {}),           # odd W: not periodic
    ("nhwc3_three_strips", 3, True, "linear", (2, 86, 301), (41, 150), 3, 1, {}),
    ("nhwc4", 4, True, "linear", (2, 86, 600), (41, 299), 5, 1, {}),
    ("c1", 1, False, "linear", (2, 86, 600), (41, 299), 5, 0, {}),
    ("nhwc3_cubic", 3, True, "cubic", (2, 86, 600), (41, 300), 5, 1, {}),            # clamped intermediate, four open rows
    ("nhwc3_lanczos_six", 3, True, "lanczos", (2, 86, 480), (41, 300), 5, 1, {}),    # six open rows
    ("nhwc3_wide", 3, True, "cubic", (2, 86, 1380), (41, 300), 5, 1, {}),            # 21 taps: route WIDE
    ("nhwc3_split", 3, True, "linear", (2, 86, 1520), (41, 80), 5, 1, {}),           # 38 taps: four lanes per pixel, strips of 16 columns
    ("nhwc3_up_linear", 3, True, "linear", (2, 40, 600), (83, 300), 5, 1, {}),       # growing heights, ring of 2
    ("nhwc3_up_cubic", 3, True, "cubic", (2, 40, 600), (83, 300), 5, 1, {}),         # growing heights, ring of 6
    ("planar_single_planes", 3, False, "cubic", (2, 86, 600), (41, 300), 5, 0, {}),
    ("plane_groups_4", 4, False, "linear", (1, 86, 600), (41, 300), 5, 1, {}),       # the last group holds one plane
    ("plane_groups_5", 5, False, "linear", (1, 86, 600), (41, 299), 5, 1, {}),       # ... two
    ("alpha", 4, True, "linear", (2, 86, 600), (41, 300), 5, 1, {"alpha": True}),
    ("harness", 3, True, "linear", (2, 86, 600), (41, 299), 5, 1, {"uint8_mode": "harness"}),
]


@functools.lru_cache(maxsize=None)
def _v3_expected(name):
    _, c, _, filt, (n, h, w), size, _, _, kw = next(cs for cs in V3_CASES if cs[0] == name)
    x = _u8((n, c, h, w), 31)
    if kw.get("alpha"):  # Pillow: premultiply, resize the four channels, un-premultiply (the formulas tests/golden/alpha.npz was made with)
        am = kit_golden.generator("alpha")
        a = x[:, 3:4]
        pre = np.concatenate([am.premul_formula(x[:, :3], np.broadcast_to(a, x[:, :3].shape)), a], axis=1)
        r = oracle.pil_resize_u8(filt, np.ascontiguousarray(pre), size)
        return np.concatenate([am.unpremul_formula(r[:, :3], np.broadcast_to(r[:, 3:4], r[:, :3].shape)), r[:, 3:4]], axis=1)
    if kw.get("uint8_mode") == "harness":
        return np.ascontiguousarray(oracle.harness_u8(filt, x, size))
    if filt in oracle.FILTERS:
        return np.ascontiguousarray(oracle.pil_resize_u8(filt, x, size))
    brg = BR.gen()
    return np.stack([brg.resize_box_restated(filt, np.ascontiguousarray(img.transpose(1, 2, 0)), size[0], size[1]).transpose(2, 0, 1) for img in x])


def _assert_route(lib, name, filt, h, w, oh, ow):
    """The routes of the fused uint8 kernel share a variant name: the table figures each follows from (Pillow-arithmetic cases)."""
    from interpolate_antialiasing_amd import tables

    dev = torch.device("cuda", torch.cuda.current_device())
    th = tables.get_table(lib.FILTER_IDS[filt], lib.TABLE_PIL, h, oh, False, 0.0, dev)
    tw = tables.get_table(lib.FILTER_IDS[filt], lib.TABLE_PIL, w, ow, False, 0.0, dev)
    taps, rows = tw.max_taps, th.scatter_max
    if "_up_" in name:
        assert h < oh and taps <= 16 and th.max_taps == (2 if filt == "linear" else 4), (name, taps, th.max_taps)  # rings of 2 and of 6 rows
    elif "six" in name:
        assert taps <= 16 and 5 <= rows <= 6, (name, taps, rows)
    elif "wide" in name:
        assert 17 <= taps <= 34 and 1 <= rows <= 6, (name, taps, rows)
    elif "split" in name:
        assert 35 <= taps <= 136 and 1 <= rows <= 6, (name, taps, rows)
    else:
        assert taps <= 16 and 1 <= rows <= 4 and (rows == 4) == (filt == "cubic"), (name, taps, rows)


@pytest.mark.parametrize("case", V3_CASES, ids=lambda c: c[0])
def test_fused_uint8_kernel(aa, lib, monkeypatch, case):
    name, c, cl, filt, (n, h, w), (oh, ow), strips, groups, kw = case
    x = kit_gpu.nchw_gpu(_u8((n, c, h, w), 31), cl)
    if "uint8_mode" not in kw:
        _assert_route(lib, name, filt, h, w, oh, ow)
    want = ("fused_u8_nhwc_pil_alpha_v3" if kw.get("alpha") else
            ("fused_u8_nhwc_harness_v3" if cl else "fused_u8_planar_harness_v3") if kw.get("uint8_mode") else
            "fused_u8_nhwc_pil_v3" if cl else "fused_u8_planar_pil_v3")
    lib.set_plane_groups(groups)
    _sweep(monkeypatch, lib, lambda: _fwd(aa, filt)(x, [oh, ow], **kw), lib.LAUNCH_V3, want, _exactly(_v3_expected(name)), name, strips)


@pytest.mark.parametrize("dtype,ow", [(torch.float32, 300), (torch.float16, 300), (torch.float16, 299), (torch.bfloat16, 300), (torch.bfloat16, 299)],
                         ids=["f32", "f16_pairs", "f16_singles", "bf16_pairs", "bf16_singles"])
@pytest.mark.parametrize("fmt", ["nchw", "nhwc"])
def test_fused_uint8_to_float(aa, lib, monkeypatch, fmt, dtype, ow):
    """uint8 to normalised float in one launch; 16-bit outputs leave in pairs where the rows are whole dwords (even oW)."""
    shape, size = (2, 3, 86, 600), (41, ow)
    x = kit_gpu.nchw_gpu(_u8(shape, 32), True)
    f32 = oracle.forward("linear", np.ascontiguousarray(_u8(shape, 32).astype(np.float32)), size)
    m32, s32 = np.asarray(MEAN[:3], np.float32).reshape(1, 3, 1, 1), np.asarray(STD[:3], np.float32).reshape(1, 3, 1, 1)
    exp = torch.from_numpy(np.array((f32 - m32) / s32)).to(dtype)
    _sweep(monkeypatch, lib, lambda: aa.linear_forward(x, list(size), out_dtype=dtype, out_format=fmt, mean=MEAN[:3], std=STD[:3]), lib.LAUNCH_V3,
           f"fused_u8_nhwc_to_{TAG[dtype]}_{fmt}_v3", _exactly(exp), (fmt, TAG[dtype], ow))


# ------------------------------------------------------------------------------------------------ 2. the first-generation kernel
def test_first_generation_kernel_bands_only(aa, lib, monkeypatch):
    """aa_set_fused(2): every band count, and a grouping request is not looked at (the kernel has one workgroup form)."""
    shape, size = (2, 3, 86, 200), (41, 92)  # (this kernel stores rows of whole dwords)
    x = kit_gpu.nchw_gpu(_u8(shape, 33), True)
    exp = _exactly(oracle.pil_resize_u8("linear", _u8(shape, 33), size))
    lib.set_fused(2)
    call = lambda: aa.linear_forward(x, list(size))  # noqa: E731
    _sweep(monkeypatch, lib, call, lib.LAUNCH_V1, "fused_u8_nhwc_pil", exp, "v1", nstrips=1, groupings=False)
    for s, yb in ((2, 0), (4, 3), (8, 1)):
        lib.set_launch_shape(0, yb)
        _, _, _, own = _guarded(monkeypatch, lib, call, ("v1", 0, yb))
        lib.set_launch_shape(s, yb)
        y, v, q, out = _guarded(monkeypatch, lib, call, ("v1", s, yb))
        assert v == "fused_u8_nhwc_pil" and q.family == lib.LAUNCH_V1
        assert (out.strips_per_block, out.ybands, out.groups, out.grid) == (1, own.ybands, own.groups, own.grid), (s, yb)
        exp(y, ("v1", s, yb))


# ------------------------------------------------------------------------------------------------ 3. float, shrinking heights
# (id, dtype, channels_last, filter, shape, size, strips, variant)
DOWN_CASES = [
    ("f32_linear", torch.float32, False, "linear", (2, 3, 86, 600), (41, 300), 5, "fused_f32_nchw"),
    ("f32_three_strips", torch.float32, False, "linear", (2, 3, 86, 301), (41, 150), 3, "fused_f32_nchw"),
    ("f32_cubic_21_taps", torch.float32, False, "cubic", (2, 3, 86, 1380), (41, 300), 5, "fused_f32_nchw"),
    ("f64", torch.float64, False, "linear", (2, 2, 86, 600), (41, 300), 5, "fused_f64_nchw"),
    ("f16_odd_w", torch.float16, False, "linear", (2, 3, 86, 601), (41, 300), 5, "fused_f16_nchw"),      # the last plane's last row: fix_row
    ("bf16_odd_w", torch.bfloat16, False, "cubic", (2, 3, 86, 601), (41, 300), 5, "fused_bf16_nchw"),
    ("f32_nhwc3", torch.float32, True, "linear", (2, 3, 86, 200), (41, 100), 5, "fused_f32_nhwc"),         # 300 elements a row
    ("f16_nhwc3_odd_row", torch.float16, True, "linear", (2, 3, 86, 201), (41, 100), 5, "fused_f16_nhwc"),  # W * C = 603 halves
    ("bf16_nhwc3_odd_row", torch.bfloat16, True, "linear", (2, 3, 86, 201), (41, 99), 5, "fused_bf16_nhwc"),
    ("f16_nhwc4_odd_w", torch.float16, True, "cubic", (2, 4, 86, 151), (41, 75), 5, "fused_f16_nhwc"),      # (W * 4 is even whatever W is)
    ("bf16_nhwc4_odd_w", torch.bfloat16, True, "linear", (2, 4, 86, 151), (41, 74), 5, "fused_bf16_nhwc"),
]


@pytest.mark.parametrize("case", DOWN_CASES, ids=lambda c: c[0])
def test_fused_float_shrinking_heights(aa, lib, monkeypatch, case):
    name, dtype, cl, filt, shape, size, strips, variant = case
    x, wide = _float_input(shape, 34, dtype, cl)
    if "taps" in name:
        from interpolate_antialiasing_amd import tables

        assert tables.get_table(lib.FILTER_IDS[filt], lib.TABLE_F32, shape[3], size[1], False, 0.0, x.device).max_taps > 12
    exp = torch.from_numpy(oracle.forward(filt, wide, size)).to(dtype)  # (16-bit: the float32 reference rounded once)
    _sweep(monkeypatch, lib, lambda: _fwd(aa, filt)(x, list(size)), lib.LAUNCH_F32_DOWN, variant, _exactly(exp), name, strips)


def test_tolerance_mode_is_the_same_under_every_shape(aa, lib, monkeypatch):
    """precision="fast": within its 1e-4 bar of the oracle, and one result whatever the shape.  The bar is relative to the result, so the
    large rows are of one sign here: where rows of 1e8 and of -1e8 meet, the mode's rounding is 1e-4 of the terms, not of their difference
    (measured at the model's own shape: 6 of 73800 elements, up to 5.8e-4 of the result)."""
    shape, size = (2, 3, 86, 600), (41, 300)
    x, wide = _float_input(shape, 35, torch.float32, signed=False)
    exp = oracle.forward("linear", wide, size)
    got = _sweep(monkeypatch, lib, lambda: aa.linear_forward(x, list(size), precision="fast"), lib.LAUNCH_F32_DOWN, "fused_f32_nchw_fast",
                 lambda y, what: np.testing.assert_allclose(y.cpu().numpy(), exp, rtol=1e-4, atol=1e-4 * 255, err_msg=str(what)), "fast")
    first = next(iter(got.values()))
    for shape_, y in got.items():
        kit_gpu.assert_bits(y, first, ("fast", shape_))


# ------------------------------------------------------------------------------------------------ 4. float, growing heights
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=lambda d: TAG[d])
@pytest.mark.parametrize("filt,shape,size,strips", [("linear", (2, 3, 40, 520), (83, 1100), 5), ("linear", (2, 2, 40, 290), (83, 600), 3),
                                                    ("cubic", (2, 2, 40, 290), (83, 600), 5)],  # (cubic: two columns a lane, strips of 128)
                         ids=["linear_five_strips", "linear_three_strips", "cubic_five_strips"])
def test_fused_float_growing_heights(aa, lib, monkeypatch, filt, shape, size, strips, dtype):
    x, wide = _float_input(shape, 36, dtype)
    exp = torch.from_numpy(oracle.forward(filt, wide, size)).to(dtype)
    _sweep(monkeypatch, lib, lambda: _fwd(aa, filt)(x, list(size)), lib.LAUNCH_F32_UP, f"fused_{TAG[dtype]}_nchw_up", _exactly(exp), (filt, TAG[dtype]),
           strips)


# (id, oW, strips, store form, bytes of LDS a strip has more than under the plain form): rows of whole 64-byte sectors stream whole; rows
# that are not stream their whole sectors only; rows that are 8- but not 16-byte aligned are cut into 240-column pieces at each row's own
# sector boundaries, through a 1088-byte area per strip
STORE_FORMS = [("plain_1100", 1100, 5, 0, 0), ("streaming_1104", 1104, 5, 1, 0), ("streaming_split_1100", 1100, 5, 1, 0),
               ("streaming_240_columns_1102", 1102, 5, 1, 1088), ("streaming_240_columns_602", 602, 3, 1, 1088)]


@pytest.mark.parametrize("case", STORE_FORMS, ids=lambda c: c[0])
def test_fused_float_growing_heights_store_forms(aa, lib, monkeypatch, case):
    name, ow, strips, form, extra = case
    shape, size = (2, 3, 40, 520 if ow > 1000 else 290), (83, ow)
    x, wide = _float_input(shape, 37, torch.float32)
    exp = _exactly(oracle.forward("linear", wide, size))
    call = lambda: aa.linear_forward(x, list(size))  # noqa: E731
    lib.set_store_form(0)
    _, _, plain, _ = _guarded(monkeypatch, lib, call, (name, "plain"))
    lib.set_store_form(form)
    _sweep(monkeypatch, lib, call, lib.LAUNCH_F32_UP, "fused_f32_nchw_up", exp, name, strips, lds_differs_by=(plain.lds, extra))


U16 = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
SUB = {torch.float16: 2.0 ** -25, torch.bfloat16: 0.0}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=lambda d: TAG[d])
def test_gather_backward_of_a_down_scale(aa, lib, monkeypatch, dtype):
    """The backward of [2, 3, 83, 1100] -> (40, 520) is the growing-heights kernel over the transposed tables: one result whatever the
    shape, inside the bound tests/test_backward_gpu.py (float32) and tests/test_half_training_gpu.py (16-bit) derive from the dense float64
    adjoint."""
    (n, c, h, w), (oh, ow) = (2, 3, 83, 1100), (40, 520)
    gen = torch.Generator(device="cpu").manual_seed(38)
    g0 = torch.randn(n, c, oh, ow, generator=gen) * 10.0
    lo, hi = _marked_rows(oh)
    g0[:, :, lo[:3], :] *= -1.0e4
    g0[:, :, hi, :] *= 1.0e4
    g0 = g0.to(dtype)
    g = g0.cuda()
    mats = [R.dense("linear", h, oh, False, np.float32), R.dense("linear", w, ow, False, np.float32)]
    gi, ab = R.backward_dense(mats, g0.float().numpy().astype(np.float64))
    b32 = R.bound(mats, ab, np.float32)
    bnd = b32 if dtype == torch.float32 else b32 + U16[dtype] * (ab + b32) + SUB[dtype]

    def verify(y, what):
        assert y.dtype == dtype
        gotn = y.float().cpu().numpy().astype(np.float64)
        assert np.all(gotn[ab == 0] == 0), ("an element no gradient reaches is not exactly 0", what)
        r = R.worst_ratio(gotn, gi, bnd)
        assert r <= 1.0, ("backward outside the derived bound", what, r)

    got = _sweep(monkeypatch, lib, lambda: aa.linear_backward(g, [oh, ow], [n, c, h, w]), lib.LAUNCH_F32_UP, f"fused_{TAG[dtype]}_nchw_up", verify,
                 ("backward", TAG[dtype]))
    first = next(iter(got.values()))
    for shape_, y in got.items():
        kit_gpu.assert_bits(y, first, ("backward", TAG[dtype], shape_))


def test_one_axis_pass(aa, lib, monkeypatch):
    """The depth pass of a 3-D resample, [2, 40, 4 x 160] -> 83: a stack of planes whose rows are 640 columns (five strips of 128), the
    identity table across."""
    shape, osizes = (1, 2, 40, 4, 160), (83, 4, 160)
    x_np = _f32((1, 2, 40, 640), 39).reshape(shape)
    x = kit_gpu.nchw_gpu(x_np)
    exp = x_np
    for axis in (4, 3, 2):
        exp = kit_gpu.oracle_axis("linear", exp, axis, osizes[axis - 2])
    _sweep(monkeypatch, lib, lambda: aa.linear_forward_nd(x, list(osizes)), lib.LAUNCH_F32_UP, "fused_f32_nchw_up", _exactly(exp), "depth pass", 5)
