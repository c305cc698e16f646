"""Image.resize(box=...) and Image.resize(reducing_gap=...) on the GPU (-m gpu): the five uint8 forwards equal Pillow bit for bit
(tests/golden/box_reduce.npz, made by tests/golden/make_golden_box_reduce.py with Pillow) in both layouts, on every route the box
tables can take, and the box tables stay out of the unbounded caches."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import box_reduce_ref as ref  # noqa: E402
import kit_gpu  # noqa: E402

pytestmark = pytest.mark.gpu
G = ref.gen()
aa = kit_gpu.aa_fixture()
BOX = {cs[0]: cs for cs in G.BOX_CASES}
GAP = {cs[0]: cs for cs in G.GAP_CASES}


def _op(aa, name):
    return {"box": aa.nearest_forward, "linear": aa.linear_forward, "cubic": aa.cubic_forward, "hamming": aa.hamming_forward,
            "lanczos": aa.lanczos_forward}[name]


def _nhwc(y):
    return y.permute(0, 2, 3, 1).contiguous().cpu().numpy()


def _layouts(c):
    return (False,) if c == 1 else (True, False)


BOX_PARAMS = [(name, f) for name, cs in BOX.items() if name != "b_headline" for f in cs[5]]


@pytest.mark.parametrize("name,flt", BOX_PARAMS)
def test_box_equals_pillow(aa, name, flt):
    _, shape, seed, (oh, ow), box, _, alpha = BOX[name]
    x = ref.batch(shape, seed)
    for cl in _layouts(shape[1]):
        y = _op(aa, flt)(kit_gpu.nchw_gpu(x, cl), [oh, ow], box=box, alpha=alpha)
        assert y.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
        ref.assert_matches_fixture(f"{name}/{flt}", x, _nhwc(y))


def test_wide_windows_take_the_generic_path(aa):
    """More than 136 taps: no fused kernel; the dense fallback copies the hull and runs the two launches."""
    _, shape, seed, (oh, ow), box, _, _ = BOX["b_wide"]
    aa.cubic_forward(kit_gpu.nchw_gpu(ref.batch(shape, seed), True), [oh, ow], box=box)
    assert not aa.last_variant().startswith("fused"), aa.last_variant()


@pytest.mark.parametrize("flt", G.FILTER_NAMES)
def test_headline_shape_stays_fused(aa, flt):
    """[2,3,438,906] channels_last -> (196, 320) with a box: Pillow's bytes, from a fused kernel reading the hull as a view; the same
    bytes with the fused kernels switched off."""
    from interpolate_antialiasing_amd import _lib

    _, shape, seed, (oh, ow), box, _, _ = BOX["b_headline"]
    x = ref.batch(shape, seed)
    t = kit_gpu.nchw_gpu(x, True)
    y = _op(aa, flt)(t, [oh, ow], box=box)
    variant = aa.last_variant()
    ref.assert_matches_fixture(f"b_headline/{flt}", x, _nhwc(y))
    assert variant.startswith("fused_u8_nhwc_pil"), variant
    prev = _lib.set_fused(0)
    try:
        y0 = _op(aa, flt)(t, [oh, ow], box=box)
        assert not aa.last_variant().startswith("fused"), aa.last_variant()
    finally:
        _lib.set_fused(prev)
    assert torch.equal(y0, y)


def test_full_box_is_the_plain_call(aa):
    from interpolate_antialiasing_amd import tables

    x = ref.batch((2, 3, 97, 131), 31)
    for cl in (True, False):
        t = kit_gpu.nchw_gpu(x, cl)
        for flt in G.FILTER_NAMES:
            plain = _op(aa, flt)(t, [30, 40])
            v = aa.last_variant()
            n_tables = len(tables._cache)
            boxed = _op(aa, flt)(t, [30, 40], box=(0, 0, 131, 97))
            assert aa.last_variant() == v and torch.equal(boxed, plain)
            assert len(tables._cache) == n_tables
            assert torch.equal(_op(aa, flt)(t, [97, 131], box=(0, 0, 131, 97)), _op(aa, flt)(t, [97, 131]))


def test_integer_box_of_the_output_size_is_a_crop(aa):
    t = kit_gpu.nchw_gpu(ref.batch((2, 3, 97, 131), 31), True)
    y = aa.lanczos_forward(t, [30, 40], box=(11, 5, 51, 35))
    assert torch.equal(y, t[:, :, 5:35, 11:51]) and y.is_contiguous(memory_format=torch.channels_last)


def test_box_on_a_view_of_a_larger_tensor(aa):
    """The input itself a crop: the hull is a view of a view."""
    rng = np.random.default_rng(8)
    big = kit_gpu.nchw_gpu(rng.integers(0, 256, (3, 3, 120, 160), dtype=np.uint8), True)
    crop = big[1:, :, 9:106, 13:144]
    box = G.BOX1
    for flt in ("linear", "cubic"):
        got = _op(aa, flt)(crop, [30, 40], box=box)
        assert torch.equal(got, _op(aa, flt)(crop.contiguous(memory_format=torch.channels_last), [30, 40], box=box))
        want = np.stack([G.resize_box_restated(flt, img, 30, 40, box) for img in _nhwc(crop)])
        assert np.array_equal(_nhwc(got), want)


def test_box_on_an_axis_too_long_for_the_paired_table_build(aa):
    """A hull beyond 32768 pixels: the two tables are built one after the other (as the plain call's are), not refused."""
    rng = np.random.default_rng(10)
    x = rng.integers(0, 256, (1, 1, 4, 40000), dtype=np.uint8)
    box = (10.5, 0, 39990.5, 4)
    got = _nhwc(aa.linear_forward(kit_gpu.nchw_gpu(x, False), [4, 100], box=box))
    want = G.resize_box_restated("linear", x[0].transpose(1, 2, 0), 4, 100, box)
    assert np.array_equal(got[0], want)


def test_box_on_a_view_no_kernel_reads(aa, monkeypatch):
    """A flipped image: only its hull is copied, and the result is that of the dense tensor.  Counted through the one copy function of
    the resample paths: a view no kernel reads costs the boxed call exactly one copy, of the hull's shape and not the image's, whether the
    view is refused at sight (rows not dense) or by the strided entry point (a crop, with the fused kernels off), and the fallback's
    result keeps the hull's layout."""
    from interpolate_antialiasing_amd import _lib, boxmath

    t = kit_gpu.nchw_gpu(ref.batch((2, 3, 97, 131), 31), False)
    flipped = t.flip(3)
    assert torch.equal(aa.cubic_forward(flipped, [30, 40], box=G.BOX1), aa.cubic_forward(flipped.contiguous(), [30, 40], box=G.BOX1))
    assert torch.equal(aa.reduce(flipped, (3, 5), (5, 7, 50, 36)), aa.reduce(flipped.contiguous(), (3, 5), (5, 7, 50, 36)))

    copies = []
    real = aa._memory_format
    monkeypatch.setattr(aa, "_memory_format", lambda v, *a: (copies.append(tuple(v.shape)), real(v, *a))[1])
    bx = boxmath.box_f32(G.BOX1)
    (oy, ey), (ox, ex) = boxmath.axis_hull(97, 30, bx[1], bx[3], "cubic"), boxmath.axis_hull(131, 40, bx[0], bx[2], "cubic")
    hull = (2, 3, ey - oy, ex - ox)
    assert hull[2] < 97 and hull[3] < 131
    want = aa.cubic_forward(t, [30, 40], box=G.BOX1)
    copies.clear()
    columns = t.transpose(2, 3).contiguous().transpose(2, 3)  # the same image stored column by column: no dense rows
    assert not columns.is_contiguous() and not columns.is_contiguous(memory_format=torch.channels_last)
    y = aa.cubic_forward(columns, [30, 40], box=G.BOX1)
    print("copies of a column-major image:", copies, "hull:", hull)
    assert copies == [hull]
    assert torch.equal(y, want)
    for cl in (False, True):
        mf = torch.channels_last if cl else torch.contiguous_format
        big = kit_gpu.nchw_gpu(ref.batch((2, 3, 120, 160), 32), cl)
        crop = big[:, :, 9:106, 13:144]
        assert not crop.is_contiguous() and not crop.is_contiguous(memory_format=torch.channels_last)
        try:
            _lib.set_fused(0)  # no kernel reads a pitched view now: the strided entry point answers AA_ERR_STRIDES
            want = aa.cubic_forward(crop.contiguous(memory_format=mf), [30, 40], box=G.BOX1)
            copies.clear()
            y = aa.cubic_forward(crop, [30, 40], box=G.BOX1)
        finally:
            _lib.set_fused(1)
        print("copies of a crop, channels_last", cl, ":", copies, "hull:", hull)
        assert copies == [hull]
        assert torch.equal(y, want) and y.is_contiguous(memory_format=mf)


def test_interpolate_aa_passes_box_and_gap(aa):
    from interpolate_antialiasing_amd.functional import interpolate_aa

    t = kit_gpu.nchw_gpu(ref.batch((2, 3, 97, 131), 31), True)
    assert torch.equal(interpolate_aa(t, [30, 40], "bicubic", box=G.BOX1), aa.cubic_forward(t, [30, 40], box=G.BOX1))
    assert torch.equal(interpolate_aa(t, [10, 12], "bilinear", reducing_gap=2.0), aa.linear_forward(t, [10, 12], reducing_gap=2.0))


def test_box_tables_have_a_bounded_cache_of_their_own(aa):
    """600 calls with distinct random boxes on one small image: the results stay right, device memory does not grow, and the unbounded
    table cache never sees them."""
    from interpolate_antialiasing_amd import tables

    rng = np.random.default_rng(9)
    x = ref.batch((1, 3, 97, 131), 44)
    t = kit_gpu.nchw_gpu(x, True)
    img = x[0].transpose(1, 2, 0)
    aa.cubic_forward(t, [30, 40], box=(1.5, 1.5, 100, 90))  # (warm: the library's own one-off allocations)
    torch.cuda.synchronize()
    n_tables = len(tables._cache)
    mem300 = None
    for i in range(1, 601):
        x0, y0 = rng.uniform(0, 60), rng.uniform(0, 40)
        box = (x0, y0, x0 + rng.uniform(35, 70), y0 + rng.uniform(35, 56))
        y = aa.cubic_forward(t, [30, 40], box=box)
        if i % 50 == 0:
            assert np.array_equal(_nhwc(y)[0], G.resize_box_restated("cubic", img, 30, 40, box)), (i, box)
        del y
        if i == 300:
            torch.cuda.synchronize()
            mem300 = torch.cuda.memory_allocated()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() <= mem300
    assert len(tables._cache) == n_tables
    assert len(tables._box_cache) <= tables.BOX_CACHE_SIZE


GAP_PARAMS = [(name, f) for name, cs in GAP.items() for f in cs[6]]


@pytest.mark.parametrize("name,flt", GAP_PARAMS)
def test_reducing_gap_equals_pillow(aa, name, flt):
    _, shape, seed, (oh, ow), box, gap, _ = GAP[name]
    x = ref.batch(shape, seed)
    for cl in (True, False):
        t = kit_gpu.nchw_gpu(x, cl)
        y = _op(aa, flt)(t, [oh, ow], box=box, reducing_gap=gap)
        assert y.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
        ref.assert_matches_fixture(f"{name}/{flt}", x, _nhwc(y))
        if name == "g_ones":  # both factors are 1: the plain call, bit for bit
            assert torch.equal(y, _op(aa, flt)(t, [oh, ow]))


def test_the_gap_cases_are_what_they_are_meant_to_be():
    """Factors 10, 5 and 3; fx = 15 with fy = 1; factors of 1; a safe box clipped by the image on all four sides."""
    from interpolate_antialiasing_amd import boxmath

    full = (0.0, 0.0, 411.0, 300.0)
    assert [boxmath.reducing_factors(full, 40, 30, g) for g in (1.0, 2.0, 3.0)] == [(10, 10), (5, 5), (3, 3)]
    assert boxmath.reducing_factors((0.0, 0.0, 900.0, 64.0), 30, 32, 2.0) == (15, 1)
    assert boxmath.reducing_plan(131, 97, 80, 60, "cubic", (0.0, 0.0, 131.0, 97.0), 2.0) is None
    assert boxmath.safe_box(411, 300, 40, 30, "cubic", full) == (0, 0, 411, 300)
    assert boxmath.safe_box(411, 300, 40, 30, "cubic", (20.5, 10.25, 400, 290)) != (0, 0, 411, 300)
