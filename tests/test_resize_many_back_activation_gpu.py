"""activation="softmax" / "sigmoid" of resize_many_back and resize_many_back_merged on the GPU, bit for bit.  The expected values are the
numpy restatement (activation_ref) applied on the CPU to the fp32 R_i that the EXISTING call returns, resize_many_back(..., reduce=None,
out_dtype=torch.float32) — so all five filters are covered and there is no second source of truth for the resample — and, for the merged
call, the members' P added by resize_many_back_merged_ref.merge_members.  Everything is compared with assert_bits.  In the one test
with non-finite logits every NaN is first replaced by one NaN on both sides: a NaN's sign and payload are not part of the definition
(they follow the machine's propagation rule, and the CPU's is not the GPU's)."""
import numpy as np
import pytest
import torch

import activation_ref as act
import kit_gpu
import resize_many_back_merged_ref as ref
from kit_golden import MODE
from kit_gpu import assert_bits

pytestmark = pytest.mark.gpu

aa = kit_gpu.aa_fixture()

ACTIVATIONS = act.ACTIVATIONS
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
LABELS = {torch.uint8: np.uint8, torch.int16: np.int16, torch.int32: np.int32, torch.int64: np.int64}
MERGES = ("sum", "mean")
G = len(ref.BASE_SIZES)
ITEM_SIZES = [ref.BASE_SIZES[g] for g in ref.BASE_GROUPS]
_R = {}


def gpu(a, dtype=torch.float32, channels_last=False):
    t = torch.from_numpy(np.array(a)).cuda().to(dtype)
    return t.contiguous(memory_format=torch.channels_last) if channels_last else t


def back(aa, *args, **kw):
    with kit_gpu.gpu_error_ends_the_session("resize_many_back"):
        return aa.resize_many_back(*args, **kw)


def merged(aa, *args, **kw):
    with kit_gpu.gpu_error_ends_the_session("resize_many_back_merged"):
        return aa.resize_many_back_merged(*args, **kw)


def r_values(aa, x, sizes, mode="bilinear", regions=None, flips=None, key=None):
    """The fp32 R_i of the existing call, on the CPU as numpy arrays; with a key computed once and shared, read-only."""
    if key is None or key not in _R:
        vals = [o.cpu().numpy() for o in back(aa, x, sizes, mode, regions=regions, flips=flips, reduce=None, out_dtype=torch.float32)]
        for v in vals:
            v.setflags(write=False)
        if key is None:
            return vals
        _R[key] = vals
    return _R[key]


def base_r(aa, filt):
    return r_values(aa, gpu(ref.BASE_CANVAS), ITEM_SIZES, MODE[filt], ref.BASE_REGIONS, ref.BASE_FLIPS, key=("base", filt))


def merged_p(vals, groups, n_groups, activation, merge):
    return ref.merge_members([act.apply(activation, v) for v in vals], groups, n_groups, merge)


def one_nan(t):
    """Every NaN of a float tensor replaced by one NaN."""
    t = t.detach().cpu()
    return torch.where(t != t, torch.full_like(t, float("nan")), t) if t.is_floating_point() else t


def check_both_calls(aa, x, vals, groups, sizes, tag, activation, mode="bilinear", regions=None, flips=None, nans=False, **kw):
    """reduce=None in float32 of both calls against the restatement of vals (the members' R_i, each at its group's size)."""
    fix = one_nan if nans else (lambda t: t)
    outs = back(aa, x, [sizes[g] for g in groups], mode, regions=regions, flips=flips, activation=activation, **kw)
    assert len(outs) == len(vals)
    for i, (o, v) in enumerate(zip(outs, vals)):
        assert_bits(fix(o), fix(torch.from_numpy(act.apply(activation, v))), f"{tag} {activation} item {i}")
    for merge in MERGES:
        outs = merged(aa, x, groups, sizes, mode, regions=regions, flips=flips, merge=merge, activation=activation, **kw)
        want = merged_p(vals, groups, len(sizes), activation, merge)
        assert len(outs) == len(want)
        for g, (o, w) in enumerate(zip(outs, want)):
            assert_bits(fix(o), fix(torch.from_numpy(w)), f"{tag} {activation} {merge} group {g}")


# ---- values ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels_last", (False, True), ids=("planar", "channels_last"))
@pytest.mark.parametrize("filt", ref.FILTERS)
def test_base_case_every_filter(aa, filt, channels_last):
    """K = 7: one chunk of four classes and a tail of three; the (4, 300) outputs cross the 256-column tile; one-pixel and one-column
    sources, flips and cropped regions."""
    x = gpu(ref.BASE_CANVAS, channels_last=channels_last)
    for activation in ACTIVATIONS:
        check_both_calls(aa, x, base_r(aa, filt), ref.BASE_GROUPS, ref.BASE_SIZES, f"{filt} cl={channels_last}", activation, MODE[filt],
                         ref.BASE_REGIONS, ref.BASE_FLIPS)
    # the members of a group are not one another's copies, and a softmax is not a sigmoid: the case can tell them apart
    p = merged_p(base_r(aa, filt), ref.BASE_GROUPS, G, "softmax", "sum")
    q = merged_p(base_r(aa, filt), ref.BASE_GROUPS, G, "sigmoid", "sum")
    assert all(np.abs(a - b).max() > 0.1 for a, b in zip(p, q))


@pytest.mark.parametrize("channels_last", (False, True), ids=("planar", "channels_last"))
@pytest.mark.parametrize("k", (1, 3, 4, 5, 8))
def test_every_k_both_classes(aa, k, channels_last):
    """K below, at and above the chunk of four, with and without a tail; 16-byte-aligned channels_last tensors with K = 4 and 8 take the
    vector loads.  Values, and uint8 labels of both calls."""
    c = ref.k_canvas(k)
    x = gpu(c, channels_last=channels_last)
    vals = r_values(aa, gpu(c), ITEM_SIZES, "bicubic", ref.BASE_REGIONS, ref.BASE_FLIPS, key=("k", k))
    for activation in ACTIVATIONS:
        check_both_calls(aa, x, vals, ref.BASE_GROUPS, ref.BASE_SIZES, f"K={k} cl={channels_last}", activation, "bicubic", ref.BASE_REGIONS,
                         ref.BASE_FLIPS)
        kw = dict(regions=ref.BASE_REGIONS, flips=ref.BASE_FLIPS, reduce="argmax", out_dtype=torch.uint8, activation=activation)
        for i, (lab, v) in enumerate(zip(back(aa, x, ITEM_SIZES, "bicubic", **kw), vals)):
            assert_bits(lab, torch.from_numpy(np.argmax(act.apply(activation, v), axis=0).astype(np.uint8)), f"K={k} {activation} labels {i}")
        for merge in MERGES:
            labs = merged(aa, x, ref.BASE_GROUPS, ref.BASE_SIZES, "bicubic", merge=merge, **kw)
            for g, (lab, w) in enumerate(zip(labs, merged_p(vals, ref.BASE_GROUPS, G, activation, merge))):
                assert_bits(lab, torch.from_numpy(np.argmax(w, axis=0).astype(np.uint8)), f"K={k} {activation} {merge} labels {g}")


def test_separately_allocated_items(aa):
    srcs, regions, groups, sizes, flips = ref.list_case()
    items = [gpu(s) for s in srcs]
    inter = [t.permute(1, 2, 0).contiguous().permute(2, 0, 1) for t in items]
    vals = r_values(aa, items, [sizes[g] for g in groups], "bilinear", regions, flips)
    for form, lst in (("planar", items), ("interleaved", inter), ("mixed", [t if i % 2 else inter[i] for i, t in enumerate(items)])):
        for activation in ACTIVATIONS:
            check_both_calls(aa, lst, vals, groups, sizes, f"list {form}", activation, "bilinear", regions, flips)


def test_labels_above_255_and_a_long_class_loop(aa):
    c, regions, groups, sizes = ref.k300_case()
    x = gpu(c)
    vals = r_values(aa, x, [sizes[g] for g in groups], "bilinear", regions)
    for activation in ACTIVATIONS:
        check_both_calls(aa, x, vals, groups, sizes, "K = 300", activation, "bilinear", regions)
        for merge in MERGES:
            want = np.argmax(merged_p(vals, groups, 1, activation, merge)[0], axis=0)
            assert want.max() == 299
            for dtype in (torch.int16, torch.int32, None):
                lab = merged(aa, x, groups, sizes, regions=regions, merge=merge, reduce="argmax", out_dtype=dtype, activation=activation)[0]
                assert_bits(lab, torch.from_numpy(want.astype(LABELS[dtype or torch.int64])), f"K = 300 {activation} {merge} {dtype}")
        want = [np.argmax(act.apply(activation, v), axis=0) for v in vals]
        assert max(w.max() for w in want) == 299
        for lab, w in zip(back(aa, x, [sizes[g] for g in groups], regions=regions, reduce="argmax", out_dtype=torch.int16, activation=activation), want):
            assert_bits(lab, torch.from_numpy(w.astype(np.int16)), f"K = 300 {activation} items")


@pytest.mark.parametrize("in_dtype", (torch.float16, torch.bfloat16), ids=("fp16", "bf16"))
def test_sixteen_bit_inputs_and_every_out_dtype(aa, in_dtype):
    """The activation sees the fp32 R_i of the 16-bit input; P is rounded ONCE to out_dtype."""
    x = gpu(ref.BASE_CANVAS, in_dtype)
    xl = x.contiguous(memory_format=torch.channels_last)
    vals = r_values(aa, x, ITEM_SIZES, "bicubic", ref.BASE_REGIONS, ref.BASE_FLIPS)
    kw = dict(regions=ref.BASE_REGIONS, flips=ref.BASE_FLIPS)
    for activation in ACTIVATIONS:
        want = [torch.from_numpy(act.apply(activation, v)) for v in vals]
        wants = {m: [torch.from_numpy(w) for w in merged_p(vals, ref.BASE_GROUPS, G, activation, m)] for m in MERGES}
        for out_dtype in (None,) + DTYPES:
            for t in (x, xl):
                outs = back(aa, t, ITEM_SIZES, "bicubic", out_dtype=out_dtype, activation=activation, **kw)
                for i, (o, w) in enumerate(zip(outs, want)):
                    assert_bits(o, w.to(out_dtype or in_dtype), f"{in_dtype} -> {out_dtype} {activation} cl={t is xl} item {i}")
                for merge in MERGES:
                    outs = merged(aa, t, ref.BASE_GROUPS, ref.BASE_SIZES, "bicubic", merge=merge, out_dtype=out_dtype, activation=activation, **kw)
                    for g, (o, w) in enumerate(zip(outs, wants[merge])):
                        assert_bits(o, w.to(out_dtype or in_dtype), f"{in_dtype} -> {out_dtype} {activation} {merge} cl={t is xl} group {g}")


# ---- the reductions -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels_last", (False, True), ids=("planar", "channels_last"))
@pytest.mark.parametrize("activation", ACTIVATIONS)
def test_argmax_and_greater_look_at_the_fp32_probabilities(aa, activation, channels_last):
    x = gpu(ref.BASE_CANVAS, channels_last=channels_last)
    vals = base_r(aa, "cubic")
    kw = dict(regions=ref.BASE_REGIONS, flips=ref.BASE_FLIPS, activation=activation)
    ps = [act.apply(activation, v) for v in vals]
    sums = {m: merged_p(vals, ref.BASE_GROUPS, G, activation, m) for m in MERGES}
    for dtype in (None,) + tuple(LABELS):
        np_dtype = LABELS[dtype or torch.int64]
        labs = back(aa, x, ITEM_SIZES, "bicubic", reduce="argmax", out_dtype=dtype, **kw)
        assert all(lab.grad_fn is None for lab in labs)
        for i, (lab, p) in enumerate(zip(labs, ps)):
            assert_bits(lab, torch.from_numpy(np.argmax(p, axis=0).astype(np_dtype)), f"{activation} argmax {dtype} item {i}")
        for merge in MERGES:
            labs = merged(aa, x, ref.BASE_GROUPS, ref.BASE_SIZES, "bicubic", merge=merge, reduce="argmax", out_dtype=dtype, **kw)
            for g, (lab, s) in enumerate(zip(labs, sums[merge])):
                assert_bits(lab, torch.from_numpy(np.argmax(s, axis=0).astype(np_dtype)), f"{activation} {merge} argmax {dtype} group {g}")
    for dtype in (None, torch.uint8):
        masks = back(aa, x, ITEM_SIZES, "bicubic", reduce="greater", threshold=0.5, out_dtype=dtype, **kw)
        for i, (m, p) in enumerate(zip(masks, ps)):
            assert_bits(m, torch.from_numpy(p > np.float32(0.5)).to(dtype or torch.bool), f"{activation} greater {dtype} item {i}")
        for merge in MERGES:
            masks = merged(aa, x, ref.BASE_GROUPS, ref.BASE_SIZES, "bicubic", merge=merge, reduce="greater", threshold=0.5, out_dtype=dtype, **kw)
            for g, (m, s) in enumerate(zip(masks, sums[merge])):
                assert_bits(m, torch.from_numpy(s > np.float32(0.5)).to(dtype or torch.bool), f"{activation} {merge} greater {dtype} group {g}")
    # the masks are not all one value: the threshold cuts through the case (for a softmax over seven classes through the summed groups)
    assert any((s > np.float32(0.5)).any() and not (s > np.float32(0.5)).all() for m in MERGES for s in sums[m])

# ---- special values -------------------------------------------------------------------------------------------------------------------
def nonfinite_canvas():
    """The base canvas with class 2 masked (-inf) in every member, a +inf in item 0, a NaN in item 2's region, and item 5's one source
    pixel -inf in every class (an all -inf pixel wherever item 5 is read)."""
    c = np.array(ref.BASE_CANVAS)
    c[:, 2] = -np.inf
    c[0, 5, 3, 0] = np.inf
    c[2, 3, 4, 6] = np.nan
    c[5, :, 3, 0] = -np.inf
    return c


@pytest.mark.parametrize("channels_last", (False, True), ids=("planar", "channels_last"))
def test_non_finite_logits(aa, channels_last):
    c = nonfinite_canvas()
    vals = r_values(aa, gpu(c), ITEM_SIZES, "bilinear", ref.BASE_REGIONS, ref.BASE_FLIPS, key=("nonfinite",))
    # the case is what it says: a masked class beside finite ones, a +inf, a NaN, a pixel of nothing but -inf
    assert np.isneginf(vals[6][2]).all() and np.isfinite(vals[6][[0, 1, 3, 4, 5, 6]]).all()
    assert np.isposinf(vals[0][5]).any() and np.isnan(vals[2][3]).any() and np.isneginf(vals[5]).all()
    p = act.softmax(vals[6])
    assert (p[2].view(np.int32) == 0).all() and np.isfinite(p).all(), "the masked class has probability +0"
    assert np.isnan(act.softmax(vals[5])).all() and np.isnan(act.softmax(vals[0])[:, np.isposinf(vals[0][5])]).all()
    x = gpu(c, channels_last=channels_last)
    for activation in ACTIVATIONS:
        check_both_calls(aa, x, vals, ref.BASE_GROUPS, ref.BASE_SIZES, f"non-finite cl={channels_last}", activation, "bilinear", ref.BASE_REGIONS,
                         ref.BASE_FLIPS, nans=True)
        kw = dict(regions=ref.BASE_REGIONS, flips=ref.BASE_FLIPS, activation=activation)
        with np.errstate(invalid="ignore"):
            for i, (lab, m, v) in enumerate(zip(back(aa, x, ITEM_SIZES, reduce="argmax", out_dtype=torch.uint8, **kw),
                                                back(aa, x, ITEM_SIZES, reduce="greater", threshold=0.5, **kw), vals)):
                q = act.apply(activation, v)
                assert_bits(lab, torch.from_numpy(np.argmax(q, axis=0).astype(np.uint8)), f"non-finite {activation} labels {i}")
                assert_bits(m, torch.from_numpy(q > np.float32(0.5)), f"non-finite {activation} masks {i}")
            for merge in MERGES:
                want = merged_p(vals, ref.BASE_GROUPS, G, activation, merge)
                labs = merged(aa, x, ref.BASE_GROUPS, ref.BASE_SIZES, merge=merge, reduce="argmax", out_dtype=torch.uint8, **kw)
                masks = merged(aa, x, ref.BASE_GROUPS, ref.BASE_SIZES, merge=merge, reduce="greater", threshold=0.5, **kw)
                for g, (lab, m, w) in enumerate(zip(labs, masks, want)):
                    assert_bits(lab, torch.from_numpy(np.argmax(w, axis=0).astype(np.uint8)), f"non-finite {activation} {merge} labels {g}")
                    assert_bits(m, torch.from_numpy(w > np.float32(0.5)), f"non-finite {activation} {merge} masks {g}")


@pytest.mark.parametrize("channels_last", (False, True), ids=("planar", "channels_last"))
def test_differences_beyond_the_cutoff_and_subnormal_products(aa, channels_last):
    """K = 8 with the logits scaled by 100: differences pass -86, which gives exact zeros.  Item 1's one source pixel is seven zeros and
    -85.5, so that its last class is aa_exp(-85.5) (7.4e-38, a normal number) times rcp of about 1 / 7: a product below the smallest
    normal number at every pixel of the item, IEEE gradual underflow, as numpy gives it.  A kernel that flushed it would differ there."""
    c = (np.array(ref.k_canvas(8)) * np.float32(100.0)).astype(np.float32)
    assert ref.BASE_REGIONS[1] == (3, 0, 1, 1)
    c[1, :, 3, 0] = [0, 0, 0, 0, 0, 0, 0, -85.5]
    vals = r_values(aa, gpu(c), ITEM_SIZES, "bilinear", ref.BASE_REGIONS, ref.BASE_FLIPS, key=("scaled",))
    tiny = np.finfo(np.float32).tiny
    ps = [act.softmax(v) for v in vals]
    zeros = sum(int((p == 0).sum()) for p in ps)
    subnormal = sum(int(((p > 0) & (p < tiny)).sum()) for p in ps)
    print(f"logits x 100: {zeros} exact zeros and {subnormal} subnormal probabilities of {sum(p.size for p in ps)}")
    assert zeros > 0 and subnormal >= ITEM_SIZES[1][0] * ITEM_SIZES[1][1]
    x = gpu(c, channels_last=channels_last)
    for activation in ACTIVATIONS:
        check_both_calls(aa, x, vals, ref.BASE_GROUPS, ref.BASE_SIZES, f"x 100 cl={channels_last}", activation, "bilinear", ref.BASE_REGIONS,
                         ref.BASE_FLIPS)


# ---- groups ---------------------------------------------------------------------------------------------------------------------------
def test_a_group_of_sixteen_members(aa):
    """The most a softmax group takes: 16 members of seventy_case's sizes (3 x 3 sources, regions of 1 .. 2 pixels a side) to (4, 4),
    beside a group of two, scattered over the item order; 17 are refused, and taken with a sigmoid."""
    c, regions, _, _, flips = ref.seventy_case()
    n = 18
    c, regions, flips = c[:n], regions[:n], flips[:n]
    groups = [0, 1] + [0] * 7 + [1] + [0] * 8
    sizes = [(4, 4), (3, 2)]
    assert groups.count(0) == 16 == act.MAX_SOFTMAX_MEMBERS
    for channels_last in (False, True):
        x = gpu(c, channels_last=channels_last)
        vals = r_values(aa, gpu(c), [sizes[g] for g in groups], "bilinear", regions, flips, key=("sixteen",))
        for activation in ACTIVATIONS:
            check_both_calls(aa, x, vals, groups, sizes, f"sixteen cl={channels_last}", activation, "bilinear", regions, flips)
            for merge in MERGES:
                labs = merged(aa, x, groups, sizes, regions=regions, flips=flips, merge=merge, reduce="argmax", out_dtype=torch.int32, activation=activation)
                for g, (lab, w) in enumerate(zip(labs, merged_p(vals, groups, 2, activation, merge))):
                    assert_bits(lab, torch.from_numpy(np.argmax(w, axis=0).astype(np.int32)), f"sixteen {activation} {merge} labels {g}")
    x = gpu(c)
    seventeen = [0] * 17 + [1]
    with pytest.raises(ValueError, match=r"group 0 \(sizes\[0\]\) has 17 members"):
        aa.resize_many_back_merged(x, seventeen, sizes, regions=regions, activation="softmax")
    vals = r_values(aa, x, [sizes[g] for g in seventeen], "bilinear", regions)
    outs = merged(aa, x, seventeen, sizes, regions=regions, activation="sigmoid")
    for g, (o, w) in enumerate(zip(outs, merged_p(vals, seventeen, 2, "sigmoid", "sum"))):
        assert_bits(o, torch.from_numpy(w), f"seventeen sigmoid group {g}")


@pytest.mark.parametrize("channels_last", (False, True), ids=("planar", "channels_last"))
def test_groups_of_one_member_are_resize_many_back(aa, channels_last):
    x = gpu(ref.BASE_CANVAS, channels_last=channels_last)
    for activation in ACTIVATIONS:
        for reduce, dtype in ((None, None), (None, torch.bfloat16), ("argmax", None), ("argmax", torch.uint8), ("greater", None)):
            kw = dict(regions=ref.BASE_REGIONS, flips=ref.BASE_FLIPS, reduce=reduce, out_dtype=dtype, threshold=0.5, activation=activation)
            want = back(aa, x, ITEM_SIZES, "bicubic", **kw)
            for merge in MERGES:
                got = merged(aa, x, list(range(7)), ITEM_SIZES, "bicubic", merge=merge, **kw)
                assert len(got) == 7
                for i, (g, w) in enumerate(zip(got, want)):
                    assert_bits(g, w, f"{activation} reduce={reduce} {dtype} {merge} item {i}")


def test_activation_none_is_the_call_without_the_argument(aa):
    x = gpu(ref.BASE_CANVAS)
    kw = dict(regions=ref.BASE_REGIONS, flips=ref.BASE_FLIPS)
    for o, w in zip(back(aa, x, ITEM_SIZES, "bicubic", activation=None, **kw), base_r(aa, "cubic")):
        assert_bits(o, torch.from_numpy(np.array(w)), "activation=None")
    for o, w in zip(merged(aa, x, ref.BASE_GROUPS, ref.BASE_SIZES, "bicubic", activation=None, **kw),
                    merged(aa, x, ref.BASE_GROUPS, ref.BASE_SIZES, "bicubic", **kw)):
        assert_bits(o, w, "merged activation=None")
    # no backward through an activation: refused rather than detached; labels and masks never carry a grad_fn
    pred = x.clone().requires_grad_()
    for activation in ACTIVATIONS:
        with pytest.raises(NotImplementedError, match=r"torch\.no_grad\(\).*\.detach\(\)"):
            aa.resize_many_back(pred, ITEM_SIZES, activation=activation, **kw)
        with pytest.raises(NotImplementedError, match=r"torch\.no_grad\(\).*\.detach\(\)"):
            aa.resize_many_back_merged(pred, ref.BASE_GROUPS, ref.BASE_SIZES, activation=activation, **kw)
        with torch.no_grad():
            assert all(o.grad_fn is None for o in back(aa, pred, ITEM_SIZES, activation=activation, **kw))
        assert all(o.grad_fn is None for o in merged(aa, pred, ref.BASE_GROUPS, ref.BASE_SIZES, activation=activation, reduce="argmax", **kw))
    assert all(o.grad_fn is not None for o in back(aa, pred, ITEM_SIZES, **kw))


# ---- launches and memory --------------------------------------------------------------------------------------------------------------
def test_two_launches_for_every_activation(aa):
    x = gpu(ref.BASE_CANVAS)
    kw = dict(regions=ref.BASE_REGIONS, flips=ref.BASE_FLIPS)
    for activation in (None,) + ACTIVATIONS:
        for reduce in (None, "argmax", "greater"):
            def items():
                return aa.resize_many_back(x, ITEM_SIZES, reduce=reduce, activation=activation, **kw)

            def groups():
                return aa.resize_many_back_merged(x, ref.BASE_GROUPS, ref.BASE_SIZES, reduce=reduce, activation=activation, **kw)

            with kit_gpu.gpu_error_ends_the_session("launch count"):
                items(), groups()  # (code objects loaded)
                a, b = kit_gpu.count_launches(items), kit_gpu.count_launches(groups)
            assert len(a) == 2 and len(b) == 2, (activation, reduce, a, b)


def test_softmax_argmax_never_holds_a_float_plane_stack(aa):
    """test_resize_many_back_merged_gpu.py's bound with a softmax before the sum: K = 64, one group of three 12 x 16 members to (96, 128),
    int64 labels.  The label arena, six tables and the descriptor fit under K * oh * ow * 4 bytes; ONE float32 [K, oh, ow] — a member's
    probabilities, or their sum — does not, and neither would a workspace for the members' maxima and denominators that grew with K."""
    k, oh, ow = 64, 96, 128
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((3, k, 12, 16)).astype(np.float32)).cuda()
    flips = [False, True, False]
    args = (x, [0, 0, 0], [(oh, ow)])
    kw = dict(flips=flips, reduce="argmax", out_dtype=torch.int64, activation="softmax")
    vals = r_values(aa, x, [(oh, ow)] * 3, flips=flips)
    want = np.argmax(merged_p(vals, [0, 0, 0], 1, "softmax", "sum")[0], axis=0)
    lab = merged(aa, *args, **kw)  # (code objects loaded, the pinned block cached)
    del lab
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    lab = merged(aa, *args, **kw)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    print(f"peak memory grew by {grown} bytes; K * oh * ow * 4 = {k * oh * ow * 4}")
    assert grown < k * oh * ow * 4
    assert_bits(lab[0], torch.from_numpy(want), "softmax labels")
