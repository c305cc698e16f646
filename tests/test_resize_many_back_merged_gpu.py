"""resize_many_back_merged on the GPU: values bit for bit against the CPU restatement and against the existing single-shape calls
composed as the definition says; groups of one member against resize_many_back; label maps against numpy.argmax of the restated sums;
masks; the launch count; a peak-memory bound that a float [K, oh, ow] intermediate cannot meet; and autograd against the explicit
backward call."""
import numpy as np
import pytest
import torch

import kit_gpu
import resize_many_back_merged_ref as ref
from kit_golden import MODE
from kit_gpu import assert_bits

pytestmark = pytest.mark.gpu

aa = kit_gpu.aa_fixture()

DTYPES = (torch.float32, torch.float16, torch.bfloat16)
LABELS = {torch.uint8: np.uint8, torch.int16: np.int16, torch.int32: np.int32, torch.int64: np.int64}
MERGES = ("sum", "mean")
G = len(ref.BASE_SIZES)
_RESTATED = {}


def restated(filt, canvas="base", flips=ref.BASE_FLIPS, merge="sum"):
    """The CPU restatement's fp32 sums of the base case on a canvas, computed once and shared."""
    key = (filt, canvas, None if flips is None else tuple(flips), merge)
    if key not in _RESTATED:
        _RESTATED[key] = ref.merged_values(filt, ref.CANVASES[canvas](), ref.BASE_REGIONS, ref.BASE_GROUPS, ref.BASE_SIZES, flips, merge)
    return _RESTATED[key]


def gpu(a, dtype=torch.float32, channels_last=False):
    t = torch.from_numpy(np.array(a)).cuda().to(dtype)
    return t.contiguous(memory_format=torch.channels_last) if channels_last else t


def call(aa, *args, **kw):
    with kit_gpu.gpu_error_ends_the_session("resize_many_back_merged"):
        return aa.resize_many_back_merged(*args, **kw)


def base(aa, x, mode="bilinear", **kw):
    kw.setdefault("flips", ref.BASE_FLIPS)
    return call(aa, x, ref.BASE_GROUPS, ref.BASE_SIZES, mode, regions=ref.BASE_REGIONS, **kw)


def check_arena(outs, shapes, dtype):
    """G contiguous tensors of the right shapes and dtype, views of one arena, each on a 16-byte boundary of it."""
    assert isinstance(outs, list) and [tuple(o.shape) for o in outs] == [tuple(s) for s in shapes]
    assert all(o.dtype == dtype and o.is_contiguous() and o.is_cuda for o in outs)
    start = outs[0].untyped_storage().data_ptr()
    assert all(o.untyped_storage().data_ptr() == start and (o.data_ptr() - outs[0].data_ptr()) % 16 == 0 for o in outs)


def composed(filt, x, merge, out_dtype):
    """The definition with the existing calls: per member FORWARD[filt] on .float(), flip(-1), torch adds in ascending order, the mean's
    division, .to(out_dtype).  The division is numpy's on the CPU: torch divides a GPU tensor by a Python number as a multiplication
    by the reciprocal, which is not the correctly rounded quotient the definition asks for."""
    rs = []
    for i, ((y0, x0, h, w), g) in enumerate(zip(ref.BASE_REGIONS, ref.BASE_GROUPS)):
        r = kit_gpu.FORWARD[filt](x[i, :, y0:y0 + h, x0:x0 + w].float()[None].contiguous(), list(ref.BASE_SIZES[g]))[0]
        rs.append(r.flip(-1) if ref.BASE_FLIPS[i] else r)
    outs = []
    for g in range(G):
        idx = ref.members(ref.BASE_GROUPS, g)
        s = rs[idx[0]]
        for i in idx[1:]:
            s = s + rs[i]
        if merge == "mean":
            s = torch.from_numpy(s.cpu().numpy() / np.float32(len(idx)))
        outs.append(s.to(out_dtype))
    return outs


# ---- values ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels_last", (False, True), ids=("planar", "channels_last"))
@pytest.mark.parametrize("filt", ref.ORACLE_FILTERS)
def test_values_equal_the_restatement(aa, filt, channels_last):
    x = gpu(ref.BASE_CANVAS, channels_last=channels_last)
    for merge in MERGES:
        for flips in (None, ref.BASE_FLIPS):
            outs = base(aa, x, MODE[filt], flips=flips, merge=merge)
            check_arena(outs, [(7,) + s for s in ref.BASE_SIZES], torch.float32)
            for g, (o, w) in enumerate(zip(outs, restated(filt, flips=flips, merge=merge))):
                assert_bits(o, torch.from_numpy(w), f"{filt} {merge} group {g} flips {flips is not None}")


@pytest.mark.parametrize("filt", ref.FILTERS)
def test_values_equal_the_existing_calls_for_every_dtype(aa, filt):
    for in_dtype in DTYPES:
        x = gpu(ref.BASE_CANVAS, in_dtype)
        xl = x.contiguous(memory_format=torch.channels_last)
        for merge in MERGES:
            want = composed(filt, x, merge, torch.float32)
            for out_dtype in (None,) + DTYPES:
                for t in (x, xl):
                    outs = base(aa, t, MODE[filt], merge=merge, out_dtype=out_dtype)
                    for g, (o, w) in enumerate(zip(outs, want)):
                        assert_bits(o, w.to(out_dtype or in_dtype), f"{filt} {merge} {in_dtype} -> {out_dtype} cl={t is xl} group {g}")


@pytest.mark.parametrize("channels_last", (False, True), ids=("planar", "channels_last"))
def test_groups_of_one_member_are_resize_many_back(aa, channels_last):
    x = gpu(ref.BASE_CANVAS, channels_last=channels_last)
    sizes = [ref.BASE_SIZES[g] for g in ref.BASE_GROUPS]
    for reduce, dtype in ((None, None), (None, torch.bfloat16), ("argmax", None), ("argmax", torch.uint8), ("greater", None)):
        kw = dict(regions=ref.BASE_REGIONS, flips=ref.BASE_FLIPS, reduce=reduce, out_dtype=dtype, threshold=0.25)
        with kit_gpu.gpu_error_ends_the_session("resize_many_back"):
            want = aa.resize_many_back(x, sizes, "bicubic", **kw)
        for merge in MERGES:
            got = call(aa, x, list(range(7)), sizes, "bicubic", merge=merge, **kw)
            assert len(got) == 7
            for i, (g, w) in enumerate(zip(got, want)):
                assert_bits(g, w, f"reduce={reduce} {dtype} {merge} item {i}")
    # ... in any order of the groups: group j is item order[j]
    order = [3, 0, 6, 1, 5, 2, 4]
    groups = [order.index(i) for i in range(7)]
    got = call(aa, x, groups, [sizes[i] for i in order], "bicubic", regions=ref.BASE_REGIONS, flips=ref.BASE_FLIPS)
    with kit_gpu.gpu_error_ends_the_session("resize_many_back"):
        want = aa.resize_many_back(x, sizes, "bicubic", regions=ref.BASE_REGIONS, flips=ref.BASE_FLIPS)
    for j, i in enumerate(order):
        assert_bits(got[j], want[i], f"group {j} is item {i}")


@pytest.mark.parametrize("k", (1, 2, 8, 19))
def test_every_k_both_classes(aa, k):
    """K below, at and above the unroll, with and without a tail; K = 8 channels_last takes the vector loads, K = 2 and 19 the tail."""
    c = ref.k_canvas(k)
    want = {m: ref.merged_values("cubic", c, ref.BASE_REGIONS, ref.BASE_GROUPS, ref.BASE_SIZES, ref.BASE_FLIPS, m) for m in MERGES}
    for channels_last in (False, True):
        x = gpu(c, channels_last=channels_last)
        for merge in MERGES:
            outs = base(aa, x, "bicubic", merge=merge)
            labs = base(aa, x, "bicubic", merge=merge, reduce="argmax", out_dtype=torch.uint8)
            check_arena(labs, ref.BASE_SIZES, torch.uint8)
            for g, (o, lab, w) in enumerate(zip(outs, labs, want[merge])):
                assert_bits(o, torch.from_numpy(w), f"K={k} cl={channels_last} {merge} group {g}")
                assert_bits(lab, torch.from_numpy(np.argmax(w, axis=0).astype(np.uint8)), f"K={k} cl={channels_last} {merge} labels {g}")


def test_lists_views_and_copies(aa):
    """Separately allocated items of different sizes merged into two groups; pitched crops of larger allocations, NaN all around, read
    where they lie; items of the other class and an item in neither class copied into the call's."""
    srcs, regions, groups, sizes, flips = ref.list_case()
    want = {m: ref.merged_values("linear", srcs, regions, groups, sizes, flips, m) for m in MERGES}
    items = [gpu(s) for s in srcs]
    inter = [t.permute(1, 2, 0).contiguous().permute(2, 0, 1) for t in items]
    pitched = []  # (crops of larger allocations: odd element offsets and pitches, NaN all around)
    for t in items:
        big = torch.full((t.shape[0], t.shape[1] + 3, t.shape[2] + 5), float("nan"), device="cuda")
        big[:, 1:1 + t.shape[1], 3:3 + t.shape[2]] = t
        pitched.append(big[:, 1:1 + t.shape[1], 3:3 + t.shape[2]])
    pitched_inter = []
    for t in items:
        big = torch.full((t.shape[1] + 3, t.shape[2] + 5, t.shape[0]), float("nan"), device="cuda")
        big[1:1 + t.shape[1], 3:3 + t.shape[2]] = t.permute(1, 2, 0)
        pitched_inter.append(big[1:1 + t.shape[1], 3:3 + t.shape[2]].permute(2, 0, 1))
    neither = [t.permute(0, 2, 1).contiguous().permute(0, 2, 1) for t in items]  # (W-major storage)
    forms = {"planar": items, "interleaved": inter, "four_dims": [t[None] for t in items], "pitched": pitched, "pitched_interleaved": pitched_inter,
             "neither": neither,
             # (three interleaved, two planar: the planar items are copied)
             "mixed": [t if i % 2 else inter[i] for i, t in enumerate(items)]}
    for form, lst in forms.items():
        for merge in MERGES:
            outs = call(aa, lst, groups, sizes, regions=regions, flips=flips, merge=merge)
            check_arena(outs, [(3,) + s for s in sizes], torch.float32)
            for g, (o, w) in enumerate(zip(outs, want[merge])):
                assert_bits(o, torch.from_numpy(w), f"{form} {merge} group {g}")
    # a view is read where it lies: two launches; an item outside the class costs its copy
    for form, extra in (("planar", False), ("interleaved", False), ("pitched", False), ("pitched_interleaved", False), ("neither", True),
                        ("mixed", True)):
        names = kit_gpu.count_launches(lambda: aa.resize_many_back_merged(forms[form], groups, sizes, regions=regions))
        assert (len(names) > 2) == extra and len(names) >= 2, (form, names)


def test_seventy_groups(aa):
    c, regions, groups, sizes, flips = ref.seventy_case()
    want = {m: ref.merged_values("linear", c, regions, groups, sizes, flips, m) for m in MERGES}
    for channels_last in (False, True):
        x = gpu(c, channels_last=channels_last)
        for merge in MERGES:
            outs = call(aa, x, groups, sizes, regions=regions, flips=flips, merge=merge)
            labs = call(aa, x, groups, sizes, regions=regions, flips=flips, merge=merge, reduce="argmax", out_dtype=torch.int16)
            assert len(outs) == len(labs) == 70
            for g in range(70):
                assert_bits(outs[g], torch.from_numpy(want[merge][g]), f"seventy cl={channels_last} {merge} group {g}")
                assert_bits(labs[g], torch.from_numpy(np.argmax(want[merge][g], axis=0).astype(np.int16)),
                            f"seventy cl={channels_last} {merge} labels {g}")


# ---- argmax ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canvas", ("base", "tie", "nonfinite"))
@pytest.mark.parametrize("filt", ref.ORACLE_FILTERS)
def test_argmax_equals_numpy_argmax_of_the_restated_sum(aa, filt, canvas):
    for merge in MERGES:
        vals = restated(filt, canvas, merge=merge)
        if canvas == "nonfinite":
            assert any(np.isnan(v).any() for v in vals)
        for channels_last in (False, True):
            x = gpu(ref.CANVASES[canvas](), channels_last=channels_last)
            for dtype in (None,) + tuple(LABELS):
                labs = base(aa, x, MODE[filt], merge=merge, reduce="argmax", out_dtype=dtype)
                check_arena(labs, ref.BASE_SIZES, dtype or torch.int64)
                assert all(lab.grad_fn is None for lab in labs)
                for g, (lab, v) in enumerate(zip(labs, vals)):
                    want = np.argmax(v, axis=0).astype(LABELS[dtype or torch.int64])
                    assert_bits(lab, torch.from_numpy(want), f"{filt} {canvas} {merge} {dtype} cl={channels_last} group {g}")
        if canvas == "tie":
            assert all(not (lab == 4).any() for lab in labs) and any((lab == 2).any() for lab in labs)


def test_inf_and_minus_inf_give_the_nans_class(aa):
    """+inf in item 0 and -inf in item 5, members of group 0, at the same pixel and class: the sum is NaN there, and the NaN wins."""
    k = ref.INF_AT[0]
    member = ref.member_values("linear", ref.nonfinite_canvas(), ref.BASE_REGIONS, ref.BASE_GROUPS, ref.BASE_SIZES, ref.BASE_FLIPS)
    s = restated("linear", "nonfinite")[0]
    at = np.isposinf(member[0][k]) & ~np.isnan(s[:k]).any(axis=0)
    assert at.any() and np.isnan(s[k][at]).all() and np.isneginf(member[5][k]).all()
    x = gpu(ref.nonfinite_canvas())
    lab = base(aa, x, reduce="argmax", out_dtype=torch.uint8)[0].cpu().numpy()
    assert (lab[at] == k).all()
    val = base(aa, x)[0].cpu().numpy()
    assert np.isnan(val[k][at]).all() and np.array_equal(np.isnan(val), np.isnan(s))


def test_labels_above_255(aa):
    c, regions, groups, sizes = ref.k300_case()
    x = gpu(c)
    for merge in MERGES:
        want = np.argmax(ref.merged_values("linear", c, regions, groups, sizes, merge=merge)[0], axis=0)
        assert want.max() == 299
        for dtype in (torch.int16, torch.int32, None):
            lab = call(aa, x, groups, sizes, regions=regions, merge=merge, reduce="argmax", out_dtype=dtype)[0]
            assert_bits(lab, torch.from_numpy(want.astype(LABELS[dtype or torch.int64])), f"K = 300 {merge} {dtype}")
    with pytest.raises(ValueError, match="K = 300"):
        aa.resize_many_back_merged(x, groups, sizes, regions=regions, reduce="argmax", out_dtype=torch.uint8)


# ---- greater --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold", (0.0, 0.25))
@pytest.mark.parametrize("filt", ref.ORACLE_FILTERS)
def test_greater_equals_the_restatement(aa, filt, threshold):
    for canvas in ("base", "tie", "nonfinite"):
        for merge in MERGES:
            vals = restated(filt, canvas, merge=merge)
            want = ref.masks(vals, threshold)
            for channels_last in (False, True):
                x = gpu(ref.CANVASES[canvas](), torch.float32, channels_last)
                for dtype in (None, torch.uint8):
                    m = base(aa, x, MODE[filt], merge=merge, reduce="greater", threshold=threshold, out_dtype=dtype)
                    check_arena(m, [(7,) + s for s in ref.BASE_SIZES], dtype or torch.bool)
                    assert all(t.grad_fn is None for t in m)
                    for g, (got, w, v) in enumerate(zip(m, want, vals)):
                        got = got.cpu()
                        assert np.array_equal(got.numpy().astype(bool), w), f"{filt} {canvas} {merge} {threshold} {dtype} cl={channels_last} group {g}"
                        assert not got.numpy().astype(bool)[np.isnan(v)].any(), "a NaN is not greater"
                        assert set(np.unique(got.view(torch.uint8).numpy()).tolist()) <= {0, 1}


# ---- launches and memory --------------------------------------------------------------------------------------------------------------
def test_two_launches_whatever_n_and_g(aa):
    x7 = gpu(ref.BASE_CANVAS)
    c, regions, groups, sizes, flips = ref.seventy_case()
    x139 = gpu(c)
    for reduce in (None, "argmax", "greater"):
        for merge in MERGES:
            def seven():
                return aa.resize_many_back_merged(x7, ref.BASE_GROUPS, ref.BASE_SIZES, regions=ref.BASE_REGIONS, flips=ref.BASE_FLIPS, merge=merge,
                                                  reduce=reduce)

            def seventy():
                return aa.resize_many_back_merged(x139, groups, sizes, regions=regions, flips=flips, merge=merge, reduce=reduce)

            with kit_gpu.gpu_error_ends_the_session("resize_many_back_merged"):
                seven(), seventy()  # (code objects loaded)
                a, b = kit_gpu.count_launches(seven), kit_gpu.count_launches(seventy)
            assert len(a) == 2 and len(b) == 2, (reduce, merge, a, b)


def test_argmax_never_holds_a_float_plane_stack(aa):
    """K = 64, one group of three 12 x 16 members to (96, 128), int64 labels: the 98 KB label arena, six tables and the descriptor fit
    under K * oh * ow * 4 bytes; ONE float32 [K, oh, ow] — a member's values, or the sum — does not."""
    k, oh, ow = 64, 96, 128
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((3, k, 12, 16)).astype(np.float32)).cuda()
    args = (x, [0, 0, 0], [(oh, ow)])
    kw = dict(flips=[False, True, False], reduce="argmax", out_dtype=torch.int64)
    lab = call(aa, *args, **kw)  # (code objects loaded, the pinned block cached)
    want = sum((r.flip(-1) if f else r) for r, f in zip(aa.linear_forward(x, [oh, ow]), kw["flips"])).argmax(0)
    del lab
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    lab = call(aa, *args, **kw)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    print(f"peak memory grew by {grown} bytes; K * oh * ow * 4 = {k * oh * ow * 4}")
    assert grown < k * oh * ow * 4
    assert lab[0].dtype == torch.int64 and torch.equal(lab[0], want)  # (sum() adds in the members' order, from an exact 0 + r_0)


def test_empty(aa):
    assert aa.resize_many_back_merged([], [], [], channels=7) == []
    assert aa.resize_many_back_merged(torch.zeros((0, 7, 4, 4), device="cuda"), [], [], merge="mean", reduce="argmax") == []


# ---- autograd -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=("fp32", "bf16"))
@pytest.mark.parametrize("merge", MERGES)
def test_autograd_is_the_backward_call_on_the_groups_gradients(aa, merge, dtype):
    """The loss uses groups 0 and 2 only.  pred.grad is resize_many_back_backward with member i's gradient that of its group — the same
    tensor for the sum, G_g.float() / M_g for the mean — and None for group 1's members."""
    rng = np.random.default_rng(23)
    gs = {g: gpu(rng.standard_normal((7,) + ref.BASE_SIZES[g]).astype(np.float32), dtype) for g in (0, 2)}
    counts = [len(ref.members(ref.BASE_GROUPS, g)) for g in range(G)]
    for channels_last in (False, True):
        x = gpu(ref.BASE_CANVAS, dtype, channels_last)
        plain = base(aa, x, "bicubic", merge=merge)
        assert all(o.grad_fn is None for o in plain)
        pred = x.clone().requires_grad_()
        outs = base(aa, pred, "bicubic", merge=merge)
        assert all(o.grad_fn is not None for o in outs)
        check_arena(outs, [(7,) + s for s in ref.BASE_SIZES], dtype)
        for g, (a, b) in enumerate(zip(outs, plain)):
            assert_bits(a, b, f"{merge} {dtype} cl={channels_last} with and without grad, group {g}")
        with kit_gpu.gpu_error_ends_the_session("resize_many_back_merged backward"):
            torch.autograd.backward([outs[0], outs[2]], [gs[0], gs[2]])
            per_group = {g: (t if merge == "sum" else t.float() / counts[g]) for g, t in gs.items()}
            want = aa.resize_many_back_backward([per_group.get(g) for g in ref.BASE_GROUPS], (12, 16), "bicubic", regions=ref.BASE_REGIONS,
                                                flips=ref.BASE_FLIPS, channels=7, dtype=dtype, out_format="nhwc" if channels_last else "nchw")
        assert pred.grad.dtype == dtype and tuple(pred.grad.shape) == (7, 7, 12, 16)
        assert_bits(pred.grad, want, f"{merge} {dtype} cl={channels_last} pred.grad")
        for i in ref.members(ref.BASE_GROUPS, 1):
            assert not pred.grad[i].any(), "a member of a group the loss did not use has no gradient"
        assert pred.grad[0].any() and pred.grad[6].any()
        # a list's items each get their own gradient; an item that does not require grad gets none
        items = [t.clone().requires_grad_(i != 4) for i, t in enumerate(x)]
        outs = base(aa, items, "bicubic", merge=merge)
        with kit_gpu.gpu_error_ends_the_session("resize_many_back_merged backward"):
            torch.autograd.backward([outs[0], outs[2]], [gs[0], gs[2]])
        assert items[4].grad is None
        for i, t in enumerate(items):
            if i != 4:
                assert_bits(t.grad, want[i], f"{merge} {dtype} cl={channels_last} list item {i}")
    with torch.no_grad():
        assert all(o.grad_fn is None for o in base(aa, pred, merge=merge))
