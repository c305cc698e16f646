"""float16 / bfloat16 output of the decode-adjacent forward on the GPU (-m gpu).

Expected values never come from the code under test: the CPU oracle's fp32 forward of the image converted to float32, then
(y - mean) / std in numpy float32, then torch's CPU cast to the 16-bit type (round to nearest even) — compared as bit patterns.  Rounding
changes 28-100 % of the values at these shapes, so a float32 result cast by the test itself could not stand in for the feature."""
import ctypes

import numpy as np
import pytest
import torch

import kit_gpu
import oracle

pytestmark = pytest.mark.gpu

DTYPES = (torch.float16, torch.bfloat16)
TAG = {torch.float16: "f16", torch.bfloat16: "bf16"}
MEAN, STD = [123.675, 116.28, 103.53, 110.25], [58.395, 57.12, 57.375, 60.5]
VARIANTS = {}  # (what, dtype tag) -> variants seen, printed at the end of the module
aa = kit_gpu.aa_fixture(lambda: print("\n16-bit output, variants that ran:", {f"{k[0]}/{k[1]}": sorted(v) for k, v in sorted(VARIANTS.items())}))


def _fn(aa, filt):
    return {"linear": aa.linear_forward, "cubic": aa.cubic_forward, "box": aa.nearest_forward}[filt]


_F32 = {}


def _expected_f32(key, filt, chw_u8, size, norm):
    """The oracle's fp32 result for an NCHW uint8 array, computed once per (image, filter, size) and never modified."""
    k = (key, filt, tuple(size))
    if k not in _F32:
        y = oracle.forward(filt, np.ascontiguousarray(chw_u8).astype(np.float32), tuple(size), nthreads=4)
        y.setflags(write=False)
        _F32[k] = y
    y = _F32[k]
    if norm:
        c = chw_u8.shape[1]
        m32, s32 = np.asarray(MEAN[:c], np.float32).reshape(1, c, 1, 1), np.asarray(STD[:c], np.float32).reshape(1, c, 1, 1)
        y = (y - m32) / s32
        assert y.dtype == np.float32
    return y


def _expected16(key, filt, chw_u8, size, norm, dtype):
    e = torch.from_numpy(np.array(_expected_f32(key, filt, chw_u8, size, norm))).to(dtype)  # (a copy: the cached array is read-only)
    assert bool(torch.isfinite(e.float()).all())
    return e


def _bits_equal(got, exp16):
    g = got.cpu()
    return g.dtype == exp16.dtype and tuple(g.shape) == tuple(exp16.shape) and torch.equal(g.contiguous().view(torch.int16), exp16.contiguous().view(torch.int16))


def _norm_args(c, norm):
    return dict(mean=MEAN[:c], std=STD[:c]) if norm else {}


def _seeded(seed, n, c, h, w):
    return np.random.default_rng(seed).integers(0, 256, (n, c, h, w), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------- 1. the known-answer image
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: TAG[d])
@pytest.mark.parametrize("size", ([196, 320], [196, 319]), ids=lambda s: f"{s[0]}x{s[1]}")
def test_known_answer_image(aa, golden_kat, dtype, size):
    """The reference's image, 438 x 906 -> 196 x 320 (paired stores) and 196 x 319 (rows that do not start on dword boundaries: 2-byte
    stores), bilinear and bicubic, every layout pair, with and without mean / std.  HWC input and CHW -> nchw run fused; CHW -> nhwc has
    no fused kernel (a planar wave holds one channel) and runs the two-launch form."""
    from interpolate_antialiasing_amd import _lib

    rgb = golden_kat["rgb"]  # [438, 906, 3] uint8
    chw = np.ascontiguousarray(rgb.transpose(2, 0, 1))[None]
    hwc, planar = kit_gpu.nchw_gpu(chw, True), kit_gpu.nchw_gpu(chw, False)
    tag = TAG[dtype]
    for filt in ("linear", "cubic"):
        for x, fmts in ((hwc, ("nchw", "nhwc", None)), (planar, ("nchw", None, "nhwc"))):
            for fmt in fmts:
                for norm in (False, True):
                    y = _fn(aa, filt)(x, size, out_dtype=dtype, out_format=fmt, **_norm_args(3, norm))
                    v = _lib.last_variant()
                    VARIANTS.setdefault(("kat", tag), set()).add(v)
                    what = (filt, "hwc" if x is hwc else "chw", fmt, norm, v)
                    want_cl = (fmt == "nhwc") or (fmt is None and x is hwc)
                    assert y.is_contiguous(memory_format=torch.channels_last if want_cl else torch.contiguous_format), what
                    assert _bits_equal(y, _expected16("kat", filt, chw, size, norm, dtype)), what
                    if x is planar and fmt == "nhwc":
                        assert v == f"generic_2pass_u8_to_{tag}", what
                    else:
                        assert v.startswith("fused_") and f"_to_{tag}_" in v, what


# ---------------------------------------------------------------------------------------------- 2. small seeded shapes, batch 2
# (name, C, channels_last input, [H, W], [oH, oW]); every one with out_format nchw and nhwc (planar input: nchw), mean / std on and off
SMALL = [
    ("c3_one_strip_even", 3, True, [33, 70], [9, 34]),
    ("c3_one_strip_odd", 3, True, [33, 70], [9, 33]),
    ("c3_three_strips_even", 3, True, [40, 300], [13, 132]),
    ("c3_three_strips_odd", 3, True, [40, 300], [13, 131]),
    ("c4_even", 4, True, [40, 140], [12, 66]),
    ("c4_odd", 4, True, [40, 140], [12, 65]),
    ("c1", 1, True, [33, 70], [9, 34]),
    ("c3_growing_even", 3, True, [24, 70], [40, 34]),
    ("c3_growing_odd", 3, True, [24, 70], [40, 33]),
    # outputs narrower than a quad.  From 40 columns their windows are 27 .. 80 taps wide, beyond the fused 16-bit routes: the two-launch form
    # runs either way (asserted below); from 6 / 12 / 18 columns the windows fit and the fused forms store 1, 2 and 3 columns
    ("c3_ow1_generic", 3, True, [16, 40], [5, 1]),
    ("c3_ow2_generic", 3, True, [16, 40], [5, 2]),
    ("c3_ow3_generic", 3, True, [16, 40], [5, 3]),
    ("c3_ow1", 3, True, [16, 6], [5, 1]),
    ("c3_ow2", 3, True, [16, 12], [5, 2]),
    ("c3_ow3", 3, True, [16, 18], [5, 3]),
    ("planar_c3_even", 3, False, [33, 70], [9, 34]),
    ("planar_c3_odd", 3, False, [33, 70], [9, 33]),
]


def _run_small(aa, case, dtype, filt):
    from interpolate_antialiasing_amd import _lib

    name, c, cl, hw, size = case
    chw = _seeded(1000 + 7 * SMALL.index(case), 2, c, hw[0], hw[1])
    x = kit_gpu.nchw_gpu(chw, cl)
    seen = []
    for fmt in (("nchw", "nhwc") if cl else ("nchw",)):
        for norm in (True, False):
            exp = _expected16(name, filt, chw, size, norm, dtype)
            y = _fn(aa, filt)(x, size, out_dtype=dtype, out_format=fmt, **_norm_args(c, norm))
            v = _lib.last_variant()
            seen.append(v)
            assert _bits_equal(y, exp), (name, filt, fmt, norm, v)
    return seen


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: TAG[d])
@pytest.mark.parametrize("case", SMALL, ids=lambda c: c[0])
def test_small_shapes_fused_and_generic(aa, case, dtype):
    """Batch 2 (the second image starts img_out_bytes into the output), strips that end in whole and in ragged pairs, one and several
    strips, every channel count, growing heights (the route that counts its outstanding stores by hand), outputs narrower than a quad.
    Fused kernels on: the fused 16-bit forms run; off: the two-launch form.  Both equal the rounded oracle."""
    from interpolate_antialiasing_amd import _lib

    tag = TAG[dtype]
    filts = ("linear", "cubic", "box") if case[0] in ("c3_three_strips_even", "c3_three_strips_odd", "c4_odd") else ("linear",)
    for filt in filts:
        try:
            _lib.set_fused(1)
            on = _run_small(aa, case, dtype, filt)
            _lib.set_fused(0)
            off = _run_small(aa, case, dtype, filt)
        finally:
            _lib.set_fused(1)
        VARIANTS.setdefault((case[0], tag), set()).update(on)
        assert all(v == f"generic_2pass_u8_to_{tag}" for v in off), (case[0], filt, off)
        if case[0].endswith("_generic"):
            assert all(v == f"generic_2pass_u8_to_{tag}" for v in on), (case[0], filt, on)
        elif filt == "linear":  # (bicubic heights can hold five output rows open, which has no fused kernel: recorded, not asserted)
            assert all(v.startswith("fused_u8_") and f"_to_{tag}_" in v for v in on), (case[0], filt, on)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: TAG[d])
def test_plane_groups_on_and_off(aa, dtype):
    """Planar RGB: three planes per wave (the PL = 3 instantiations) and one wave per plane store the same bits."""
    from interpolate_antialiasing_amd import _lib

    for case in SMALL[-2:]:
        for groups in (1, 0):
            try:
                _lib.set_plane_groups(groups)
                seen = _run_small(aa, case, dtype, "linear")
            finally:
                _lib.set_plane_groups(1)
            VARIANTS.setdefault((f"{case[0]}_groups{groups}", TAG[dtype]), set()).update(seen)
            assert all(v == f"fused_u8_planar_to_{TAG[dtype]}_v3" for v in seen), (case[0], groups, seen)


# ---------------------------------------------------------------------------------------------- 3. unaligned output through the C-ABI
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: TAG[d])
def test_output_two_bytes_into_an_allocation(aa, dtype):
    """An output that starts on a 2-byte but not a 4-byte boundary: the same kernels with 2-byte stores, the same bits, nothing written
    outside the output, and the workspace answer (which never sees the pointer) is that of the aligned call: none."""
    from interpolate_antialiasing_amd import _lib, tables

    L = _lib.load()
    flag = _lib.FLAG_OUT_F16 if dtype == torch.float16 else _lib.FLAG_OUT_BF16
    stream = torch.cuda.current_stream().cuda_stream
    for name, c, cl, hw, size in (SMALL[0], SMALL[4], SMALL[-2]):
        chw = _seeded(77, 2, c, hw[0], hw[1])
        x = kit_gpu.nchw_gpu(chw, cl)
        layout = _lib.NHWC if cl else _lib.NCHW
        th, tw = tables.get_table_pair(_lib.FILTER_LINEAR, _lib.TABLE_F32, hw[0], size[0], hw[1], size[1], False, 0.0, 0.0, x.device)
        ah, aw = th.axis(), tw.axis()
        n_out = 2 * c * size[0] * size[1]
        for out_layout in ((_lib.NCHW, _lib.NHWC) if cl else (_lib.NCHW,)):
            cv = _lib.Convert(out_layout=out_layout, normalize=1, flags=flag)
            for i in range(c):
                cv.mean[i], cv.std[i] = MEAN[i], STD[i]
            ws = L.aa_workspace_bytes_u8_to_f32(layout, 2, c, hw[0], hw[1], ctypes.byref(ah), ctypes.byref(aw), ctypes.byref(cv))
            assert ws == 0, (name, ws)
            results = []
            for off in (0, 1):  # elements into the allocation
                buf = torch.full((n_out + 4,), 0x5A5A, dtype=torch.int16, device="cuda")
                assert buf.data_ptr() % 4 == 0
                rc = L.aa_resample_fwd_u8_to_f32(x.data_ptr(), buf.data_ptr() + 2 * off, None, 0, layout, 2, c, hw[0], hw[1], ctypes.byref(ah),
                                                 ctypes.byref(aw), ctypes.byref(cv), stream)
                assert rc == 0, (name, off, rc)
                v = _lib.last_variant()
                assert v.startswith("fused_u8_") and f"_to_{TAG[dtype]}_" in v, (name, off, v)
                b = buf.cpu()
                assert bool((b[:off] == 0x5A5A).all()) and bool((b[off + n_out:] == 0x5A5A).all()), (name, off)
                results.append(b[off:off + n_out])
            assert torch.equal(results[0], results[1]), (name, out_layout)
            exp = _expected16(("unaligned", name), "linear", chw, size, True, dtype)
            if out_layout == _lib.NHWC:
                exp = exp.permute(0, 2, 3, 1)
            assert torch.equal(results[0], exp.contiguous().view(torch.int16).reshape(-1)), (name, out_layout)
            # one byte off is no tensor of 2-byte elements: refused before anything is launched
            buf = torch.zeros(n_out + 4, dtype=torch.int16, device="cuda")
            rc = L.aa_resample_fwd_u8_to_f32(x.data_ptr(), buf.data_ptr() + 1, None, 0, layout, 2, c, hw[0], hw[1], ctypes.byref(ah),
                                             ctypes.byref(aw), ctypes.byref(cv), stream)
            assert rc == -4, (name, rc)


# ---------------------------------------------------------------------------------------------- 4. the tolerance mode
def _ulp16(e16):
    """One unit in the last place of the 16-bit type at |e| (finite values)."""
    a = e16.abs()
    up = (a.contiguous().view(torch.int16) + 1).view(e16.dtype)
    return up.float() - a.float()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: TAG[d])
def test_fast_precision(aa, golden_kat, dtype):
    """precision='fast' without normalisation: |got - expected16| <= 1e-4 * 255 (the project's fast-mode bar on values of 0 .. 255) + one
    unit in the last place of the 16-bit type at |expected| (rounding is monotone, and both types' ulps exceed 1e-4 relative)."""
    from interpolate_antialiasing_amd import _lib

    rgb = golden_kat["rgb"]
    chw = np.ascontiguousarray(rgb.transpose(2, 0, 1))[None]
    small = _seeded(5, 2, 3, 40, 300)
    for key, arr, size in (("kat", chw, [196, 320]), ("fast_small_even", small, [13, 132]), ("fast_small_odd", small, [13, 131])):
        for cl, fmt in ((True, "nchw"), (True, "nhwc"), (False, "nchw")):
            exp = _expected16(key, "linear", arr, size, False, dtype)
            y = aa.linear_forward(kit_gpu.nchw_gpu(arr, cl), size, out_dtype=dtype, out_format=fmt, precision="fast")
            v = _lib.last_variant()
            VARIANTS.setdefault(("fast", TAG[dtype]), set()).add(v)
            assert v.startswith("fused_u8_") and f"_to_{TAG[dtype]}_" in v and v.endswith("_fast"), (key, fmt, v)
            err = (y.cpu().float() - exp.float()).abs()
            bound = 1e-4 * 255 + _ulp16(exp)
            worst = float((err / bound).max())
            print(f"fast {TAG[dtype]} {key} {'hwc' if cl else 'chw'}->{fmt}: worst err / bound = {worst:.4f}")
            assert bool((err <= bound).all()), (key, fmt, v, worst)


# ---------------------------------------------------------------------------------------------- 5. unchanged paths
def test_float32_and_uint8_outputs_unchanged(aa):
    from interpolate_antialiasing_amd import _lib

    chw = _seeded(9, 2, 3, 40, 300)
    x = kit_gpu.nchw_gpu(chw, True)
    for fmt, variant in (("nchw", "fused_u8_nhwc_to_f32_nchw_v3"), ("nhwc", "fused_u8_nhwc_to_f32_nhwc_v3")):
        for norm in (False, True):
            y = aa.linear_forward(x, [13, 132], out_dtype=torch.float32, out_format=fmt, **_norm_args(3, norm))
            assert _lib.last_variant() == variant
            assert y.dtype == torch.float32 and np.array_equal(y.cpu().numpy(), _expected_f32("unchanged", "linear", chw, [13, 132], norm))
    y8 = aa.linear_forward(x, [13, 132], uint8_mode="pil")
    assert y8.dtype == torch.uint8 and np.array_equal(y8.cpu().numpy(), oracle.pil_resize_u8("linear", chw, (13, 132)))
    h8 = aa.linear_forward(x, [13, 132], uint8_mode="harness")
    assert np.array_equal(h8.cpu().numpy(), oracle.harness_u8("linear", chw, (13, 132)))
