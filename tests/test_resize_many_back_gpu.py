"""resize_many_back on the GPU: values bit for bit against the CPU restatement and against the existing single-shape calls composed as
the definition says; label maps against numpy.argmax of the restatement; masks; the launch count; and a peak-memory bound that a float
[K, oh, ow] intermediate cannot meet."""
import numpy as np
import pytest
import torch

import kit_gpu
import resize_many_back_ref as ref
from kit_golden import MODE
from kit_gpu import assert_bits

pytestmark = pytest.mark.gpu

aa = kit_gpu.aa_fixture()

DTYPES = (torch.float32, torch.float16, torch.bfloat16)
LABELS = {torch.uint8: np.uint8, torch.int16: np.int16, torch.int32: np.int32, torch.int64: np.int64}
BASE_FLIPS = [True, False, True, True, False]
_RESTATED = {}


def restated(filt, canvas="base", flips=None):
    """The CPU restatement's fp32 values of the base regions and sizes on a canvas, computed once and shared."""
    key = (filt, canvas, None if flips is None else tuple(flips))
    if key not in _RESTATED:
        c = {"base": ref.BASE_CANVAS, "tie": ref.tie_canvas(), "nonfinite": ref.nonfinite_canvas()}[canvas]
        _RESTATED[key] = ref.values(filt, c, ref.BASE_REGIONS, ref.BASE_SIZES, flips)
    return _RESTATED[key]


def gpu(a, dtype=torch.float32, channels_last=False):
    t = torch.from_numpy(np.array(a)).cuda().to(dtype)
    return t.contiguous(memory_format=torch.channels_last) if channels_last else t


def call(aa, *args, **kw):
    with kit_gpu.gpu_error_ends_the_session("resize_many_back"):
        return aa.resize_many_back(*args, **kw)


def composed(filt, views, sizes, flips=None):
    """The definition with the existing calls, in fp32."""
    outs = []
    for i, (v, s) in enumerate(zip(views, sizes)):
        r = kit_gpu.FORWARD[filt](v.float()[None].contiguous(), list(s))[0]
        outs.append(r.flip(-1) if flips is not None and flips[i] else r)
    return outs


def region_views(items, regions):
    return [t if r is None else t[:, r[0]:r[0] + r[2], r[1]:r[1] + r[3]] for t, r in zip(items, regions)]


def check_arena(outs, shapes, dtype):
    """N contiguous tensors of the right shapes and dtype, views of one arena, each on a 16-byte boundary of it."""
    assert isinstance(outs, list) and [tuple(o.shape) for o in outs] == [tuple(s) for s in shapes]
    assert all(o.dtype == dtype and o.is_contiguous() and o.is_cuda for o in outs)
    base = outs[0].untyped_storage().data_ptr()
    assert all(o.untyped_storage().data_ptr() == base and (o.data_ptr() - outs[0].data_ptr()) % 16 == 0 for o in outs)


# ---- values ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels_last", (False, True), ids=("planar", "channels_last"))
@pytest.mark.parametrize("filt", ref.ORACLE_FILTERS)
def test_values_equal_the_restatement(aa, filt, channels_last):
    x = gpu(ref.BASE_CANVAS, channels_last=channels_last)
    for flips in (None, BASE_FLIPS):
        outs = call(aa, x, ref.BASE_SIZES, MODE[filt], regions=ref.BASE_REGIONS, flips=flips)
        check_arena(outs, [(7,) + s for s in ref.BASE_SIZES], torch.float32)
        for i, (o, w) in enumerate(zip(outs, restated(filt, flips=flips))):
            assert_bits(o, torch.from_numpy(w), f"{filt} item {i} flips {flips is not None}")
    # the identity item is its region's bits
    y0, x0, h, w = ref.BASE_REGIONS[ref.IDENTITY_ITEM]
    assert_bits(outs[ref.IDENTITY_ITEM], x[ref.IDENTITY_ITEM, :, y0:y0 + h, x0:x0 + w], f"{filt} identity")


@pytest.mark.parametrize("filt", ref.FILTERS)
def test_values_equal_the_existing_calls_for_every_dtype(aa, filt):
    for in_dtype in DTYPES:
        for channels_last in (False, True):
            x = gpu(ref.BASE_CANVAS, in_dtype, channels_last)
            want = composed(filt, region_views(list(x), ref.BASE_REGIONS), ref.BASE_SIZES, BASE_FLIPS)
            for out_dtype in (None,) + DTYPES:
                outs = call(aa, x, ref.BASE_SIZES, MODE[filt], regions=ref.BASE_REGIONS, flips=BASE_FLIPS, out_dtype=out_dtype)
                for i, (o, w) in enumerate(zip(outs, want)):
                    assert_bits(o, w.to(out_dtype or in_dtype), f"{filt} {in_dtype} -> {out_dtype} cl={channels_last} item {i}")
            # the identity item, unflipped, is its region's bits in every dtype
            y0, x0, h, w = ref.BASE_REGIONS[ref.IDENTITY_ITEM]
            same = call(aa, x, ref.BASE_SIZES, MODE[filt], regions=ref.BASE_REGIONS)[ref.IDENTITY_ITEM]
            assert_bits(same, x[ref.IDENTITY_ITEM, :, y0:y0 + h, x0:x0 + w].contiguous(), f"{filt} {in_dtype} cl={channels_last} identity")


@pytest.mark.parametrize("k", (1, 2, 8, 19))
def test_every_k_both_classes(aa, k):
    """K below, at and above the unroll, with and without a tail; K = 8 channels_last takes the vector loads, K = 2 and 19 do not."""
    c = ref.k_canvas(k)
    want = ref.values("cubic", c, ref.BASE_REGIONS, ref.BASE_SIZES)
    for channels_last in (False, True):
        x = gpu(c, channels_last=channels_last)
        outs = call(aa, x, ref.BASE_SIZES, "bicubic", regions=ref.BASE_REGIONS)
        labs = call(aa, x, ref.BASE_SIZES, "bicubic", regions=ref.BASE_REGIONS, reduce="argmax", out_dtype=torch.uint8)
        for i, (o, lab, w) in enumerate(zip(outs, labs, want)):
            assert_bits(o, torch.from_numpy(w), f"K={k} cl={channels_last} item {i}")
            assert_bits(lab, torch.from_numpy(np.argmax(w, axis=0).astype(np.uint8)), f"K={k} cl={channels_last} labels {i}")


def test_lists_views_and_copies(aa):
    """Separately allocated items of different sizes; a pitched crop of a larger allocation read where it lies; items of the other class
    and an item in neither class copied into the call's."""
    srcs, regions, sizes = ref.list_case()
    flips = [True, False, False, True]
    want = ref.values("linear", srcs, regions, sizes, flips)
    items = [gpu(s) for s in srcs]
    inter = [t.permute(1, 2, 0).contiguous().permute(2, 0, 1) for t in items]
    pitched = []  # (crops of larger allocations: odd element offsets and pitches, NaN all around)
    for t in items:
        big = torch.full((t.shape[0], t.shape[1] + 3, t.shape[2] + 5), float("nan"), device="cuda")
        big[:, 1:1 + t.shape[1], 3:3 + t.shape[2]] = t
        pitched.append(big[:, 1:1 + t.shape[1], 3:3 + t.shape[2]])
    neither = [t.permute(0, 2, 1).contiguous().permute(0, 2, 1) for t in items]  # (W-major storage)
    forms = {"planar": items, "interleaved": inter, "four_dims": [t[None] for t in items], "pitched": pitched, "neither": neither,
             # (two of each: a tie goes to the interleaved class, and the planar items are copied)
             "mixed": [inter[i] if i % 2 else t for i, t in enumerate(items)]}
    for form, lst in forms.items():
        outs = call(aa, lst, sizes, regions=regions, flips=flips)
        check_arena(outs, [(3,) + s for s in sizes], torch.float32)
        for i, (o, w) in enumerate(zip(outs, want)):
            assert_bits(o, torch.from_numpy(w), f"{form} item {i}")
    # a view is read where it lies: two launches; an item outside the class costs its copy
    for form, extra in (("planar", False), ("interleaved", False), ("pitched", False), ("neither", True), ("mixed", True)):
        names = kit_gpu.count_launches(lambda: aa.resize_many_back(forms[form], sizes, regions=regions))
        assert (len(names) > 2) == extra and len(names) >= 2, (form, names)


def test_one_item_and_seventy(aa):
    x = gpu(ref.BASE_CANVAS)
    outs = call(aa, x[:1], ref.BASE_SIZES[:1], "bicubic")
    assert_bits(outs[0], torch.from_numpy(ref.values("cubic", ref.BASE_CANVAS[:1], None, ref.BASE_SIZES[:1])[0]), "N = 1")
    c, regions, sizes = ref.seventy_case()
    want = ref.values("linear", c, regions, sizes)
    for channels_last in (False, True):
        x = gpu(c, channels_last=channels_last)
        outs = call(aa, x, sizes, regions=regions)
        labs = call(aa, x, sizes, regions=regions, reduce="argmax", out_dtype=torch.int16)
        assert len(outs) == len(labs) == 70
        for i in range(70):
            assert_bits(outs[i], torch.from_numpy(want[i]), f"seventy cl={channels_last} item {i}")
            assert_bits(labs[i], torch.from_numpy(np.argmax(want[i], axis=0).astype(np.int16)), f"seventy cl={channels_last} labels {i}")


# ---- argmax ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canvas", ("base", "tie", "nonfinite"))
@pytest.mark.parametrize("filt", ref.ORACLE_FILTERS)
def test_argmax_equals_numpy_argmax_of_the_restatement(aa, filt, canvas):
    c = {"base": ref.BASE_CANVAS, "tie": ref.tie_canvas(), "nonfinite": ref.nonfinite_canvas()}[canvas]
    vals = restated(filt, canvas, BASE_FLIPS)
    if canvas == "nonfinite":
        assert any(np.isnan(v).any() for v in vals) and any(np.isposinf(v).any() for v in vals)
    for channels_last in (False, True):
        x = gpu(c, channels_last=channels_last)
        own = call(aa, x, ref.BASE_SIZES, MODE[filt], regions=ref.BASE_REGIONS, flips=BASE_FLIPS, out_dtype=torch.float32)
        for dtype in (None,) + tuple(LABELS):
            labs = call(aa, x, ref.BASE_SIZES, MODE[filt], regions=ref.BASE_REGIONS, flips=BASE_FLIPS, reduce="argmax", out_dtype=dtype)
            check_arena(labs, ref.BASE_SIZES, dtype or torch.int64)
            for i, (lab, v, o) in enumerate(zip(labs, vals, own)):
                want = np.argmax(v, axis=0).astype(LABELS[dtype or torch.int64])
                assert_bits(lab, torch.from_numpy(want), f"{filt} {canvas} {dtype} cl={channels_last} item {i}")
                # ... and the argmax of the call's own float32 values (numpy's rule: torch.argmax does not promise the first NaN)
                assert np.array_equal(lab.cpu().numpy(), np.argmax(o.cpu().numpy(), axis=0)), f"{filt} {canvas} own values, item {i}"
    if canvas == "tie":
        assert all(not (lab == 4).any() for lab in labs)


def test_argmax_is_taken_before_the_rounding_to_16_bits(aa):
    """Two classes whose fp32 values differ by less than a bfloat16 step: the label follows the fp32 values."""
    c = np.zeros((1, 2, 2, 2), np.float32)
    c[0, 0], c[0, 1] = 1.0, 1.0
    c[0, 1, 0, 0] = np.float32(1.0) + np.float32(2.0 ** -20)
    x = gpu(c)
    lab = call(aa, x, [(2, 2)], reduce="argmax", out_dtype=torch.uint8)[0]
    val = call(aa, x, [(2, 2)], out_dtype=torch.bfloat16)[0]
    assert lab.cpu().tolist() == [[1, 0], [0, 0]] and torch.equal(val[0], val[1])


def test_labels_above_255(aa):
    c, regions, sizes = ref.k300_case()
    want = np.argmax(ref.values("linear", c, regions, sizes)[0], axis=0)
    assert want.max() == 299
    x = gpu(c)
    for dtype in (torch.int16, torch.int32, None):
        lab = call(aa, x, sizes, regions=regions, reduce="argmax", out_dtype=dtype)[0]
        assert_bits(lab, torch.from_numpy(want.astype(LABELS[dtype or torch.int64])), f"K = 300 {dtype}")
    with pytest.raises(ValueError, match="K = 300"):
        aa.resize_many_back(x, sizes, regions=regions, reduce="argmax", out_dtype=torch.uint8)


# ---- greater --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold", (0.0, 0.25))
@pytest.mark.parametrize("filt", ref.ORACLE_FILTERS)
def test_greater_equals_the_restatement(aa, filt, threshold):
    for canvas in ("base", "tie", "nonfinite"):
        c = {"base": ref.BASE_CANVAS, "tie": ref.tie_canvas(), "nonfinite": ref.nonfinite_canvas()}[canvas]
        vals = restated(filt, canvas, BASE_FLIPS)
        want = ref.masks(vals, threshold)
        for channels_last in (False, True):
            x = gpu(c, torch.float32, channels_last)
            for dtype in (None, torch.uint8):
                m = call(aa, x, ref.BASE_SIZES, MODE[filt], regions=ref.BASE_REGIONS, flips=BASE_FLIPS, reduce="greater", threshold=threshold,
                         out_dtype=dtype)
                check_arena(m, [(7,) + s for s in ref.BASE_SIZES], dtype or torch.bool)
                for i, (g, w, v) in enumerate(zip(m, want, vals)):
                    assert np.array_equal(g.cpu().numpy().astype(bool), w), f"{filt} {canvas} {threshold} {dtype} cl={channels_last} item {i}"
                    assert not g.cpu().numpy().astype(bool)[np.isnan(v)].any(), "a NaN is not greater"
                    assert set(np.unique(g.cpu().view(torch.uint8).numpy()).tolist()) <= {0, 1}


# ---- launches and memory --------------------------------------------------------------------------------------------------------------
def test_two_launches_whatever_n(aa):
    x1 = gpu(ref.BASE_CANVAS[:1])
    c, regions, sizes = ref.seventy_case()
    x70 = gpu(c)
    for reduce in (None, "argmax", "greater"):
        aa.resize_many_back(x1, ref.BASE_SIZES[:1], reduce=reduce), aa.resize_many_back(x70, sizes, regions=regions, reduce=reduce)  # (code objects loaded)
        one = kit_gpu.count_launches(lambda: aa.resize_many_back(x1, ref.BASE_SIZES[:1], reduce=reduce))
        seventy = kit_gpu.count_launches(lambda: aa.resize_many_back(x70, sizes, regions=regions, reduce=reduce))
        assert len(one) == 2 and len(seventy) == 2, (reduce, one, seventy)


def test_argmax_never_holds_the_float_values(aa):
    """One [16, 24, 32] source to (192, 256): the label map, two tables and the descriptor are about 60 KB; a float [K, oh, ow] would be
    3 MB.  The peak grows by less than a quarter of that."""
    k, oh, ow = 16, 192, 256
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((1, k, 24, 32)).astype(np.float32)).cuda()
    lab = call(aa, x, [(oh, ow)], reduce="argmax", out_dtype=torch.uint8)  # (code objects loaded, the pinned block cached)
    want = call(aa, x, [(oh, ow)])[0].argmax(0)
    del lab
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    lab = call(aa, x, [(oh, ow)], reduce="argmax", out_dtype=torch.uint8)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    print(f"peak memory grew by {grown} bytes; K * oh * ow * 4 = {k * oh * ow * 4}")
    assert grown < k * oh * ow * 4 // 4
    assert torch.equal(lab[0].long(), want)


def test_empty_list(aa):
    assert aa.resize_many_back([], [], channels=7) == []
    assert aa.resize_many_back(torch.zeros((0, 7, 4, 4), device="cuda"), [], reduce="argmax") == []
