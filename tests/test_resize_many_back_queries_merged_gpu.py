"""resize_many_back_queries(groups=...) on the GPU: the merged scores against the float64 sum over the members of
resize_many_back_queries_ref's operands — R_i from the existing resize_many_back at the group's size — under M times the sum of the
members' bounds; labels where that bound decides them; single-member groups against the un-grouped call bit for bit; ties, a NaN, the
launches, the refusals and the guard bands.  The geometry is resize_many_back_merged_ref's base case: 7 members in groups of 3 / 2 / 2,
a 300-column group that crosses the 256-column tile, one-pixel sources, flips; every member has weights of its own."""
import numpy as np
import pytest
import torch

import kit_gpu
import resize_many_back_merged_ref as merged_ref
import resize_many_back_queries_ref as ref
from kit_golden import MODE
from test_resize_many_back_guard_gpu import run_guarded

pytestmark = pytest.mark.gpu

WORST = [0.0]
aa = kit_gpu.aa_fixture(lambda: print(f"\nresize_many_back_queries(groups=): worst error / bound = {WORST[0]:.4f}"))

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
GROUPS, SIZES, REGIONS, FLIPS = merged_ref.BASE_GROUPS, merged_ref.BASE_SIZES, merged_ref.BASE_REGIONS, merged_ref.BASE_FLIPS
N, G, PIXELS = len(GROUPS), len(SIZES), sum(oh * ow for oh, ow in SIZES)
MEMBER_SIZES = [SIZES[g] for g in GROUPS]
ROUND = {F32: 0.0, F16: 2.0 ** -11, BF16: 2.0 ** -8}  # one rounding to nearest of the output type, relative
# Q, C, filter, channels_last, masks' dtype, scores' dtype, labels' dtype, merge.  Q below, at and above the 16 of a matrix step and 256
# once; C below, at and above the 32 of a class block; C = 1, 31, 32 in the resident set of 1 block, 33 and 70 in that of 3, 150 in
# that of 6, and 200 takes two class passes; (16, 32) and (256, 70) channels_last take the vector loads.
CASES = [(1, 1, "linear", False, F32, F32, torch.uint8, "sum"), (15, 31, "cubic", True, F16, F16, torch.int16, "mean"),
         (16, 32, "box", True, F32, F32, torch.int32, "sum"), (17, 33, "linear", False, BF16, BF16, torch.int64, "mean"),
         (37, 70, "cubic", False, F32, F32, torch.uint8, "sum"), (37, 150, "linear", True, F32, F16, torch.uint8, "mean"),
         (40, 200, "box", False, F32, F32, torch.uint8, "sum"), (256, 70, "linear", True, F16, BF16, torch.uint8, "sum")]


def call(aa, x, w, filt="linear", groups=GROUPS, sizes=SIZES, **kw):
    with kit_gpu.gpu_error_ends_the_session("resize_many_back_queries(groups=)"):
        return aa.resize_many_back_queries(x, w, sizes, MODE[filt], regions=REGIONS, flips=FLIPS, groups=groups, **kw)


def resampled(aa, x, filt="linear"):
    """The fp32 R_i of the existing call, every member at its group's size, as numpy arrays."""
    with kit_gpu.gpu_error_ends_the_session("resize_many_back"):
        return [o.cpu().numpy() for o in aa.resize_many_back(x, MEMBER_SIZES, MODE[filt], regions=REGIONS, flips=FLIPS, reduce=None, out_dtype=F32)]


def merged_scores(R, w, merge="sum"):
    """Per group (the float64 sum over its members of ref.scores, M times the sum of their bounds); the mean is both over M plus the one
    fp32 rounding of the quotient."""
    want, bnd = [], []
    for g in range(G):
        idx = merged_ref.members(GROUPS, g)
        s, b = zip(*(ref.scores(R[i], w[i]) for i in idx))
        s, b = sum(s), len(idx) * sum(b)
        if merge == "mean":
            s, b = s / len(idx), b / len(idx) + 2.0 ** -24 * np.abs(s / len(idx))
        want.append(s)
        bnd.append(b)
    return want, bnd


@pytest.mark.parametrize("q,c,filt,channels_last,in_dtype,out_dtype,label_dtype,merge", CASES)
def test_scores_within_the_bound_and_labels_where_decided(aa, q, c, filt, channels_last, in_dtype, out_dtype, label_dtype, merge):
    x = kit_gpu.nchw_gpu(merged_ref.k_canvas(q), channels_last).to(in_dtype)
    w = ref.weights(N, q, c)
    # (the weights of a channels_last case lie transposed in memory, the queries consecutive: read where they lie)
    wg = torch.from_numpy(np.ascontiguousarray(w.transpose(0, 2, 1))).cuda().transpose(1, 2) if channels_last else torch.from_numpy(w).cuda()
    want, bnd = merged_scores(resampled(aa, x, filt), w, merge)
    for dt in dict.fromkeys((F32, out_dtype)):
        got = call(aa, x, wg, filt, reduce=None, out_dtype=dt, merge=merge)
        assert len(got) == G
        for g, (o, s, b) in enumerate(zip(got, want, bnd)):
            assert o.dtype == dt and tuple(o.shape) == s.shape
            err, lim = np.abs(o.float().cpu().numpy().astype(np.float64) - s), b + ROUND[dt] * (np.abs(s) + b)
            if dt == F32:
                WORST[0] = max(WORST[0], float((err / b).max()))
            assert (err <= lim).all(), (g, dt, float((err / lim).max()))
    ok, arg = ref.decided(want, bnd)
    share = sum(int(o.sum()) for o in ok) / PIXELS
    print(f"Q={q} C={c} {merge}: {100 * share:.2f} % of the pixels decided, worst error / bound so far {WORST[0]:.4f}")
    assert share >= 0.9
    for g, (lab, o, a) in enumerate(zip(call(aa, x, wg, filt, out_dtype=label_dtype, merge=merge), ok, arg)):
        assert lab.dtype == label_dtype and tuple(lab.shape) == o.shape
        assert (lab.cpu().numpy()[o] == a[o]).all(), g


@pytest.mark.parametrize("q,c,channels_last", ((37, 70, False), (16, 150, True)), ids=("planar", "channels_last"))
@pytest.mark.parametrize("merge", ("sum", "mean"))
def test_single_member_groups_are_the_ungrouped_call_bit_for_bit(aa, q, c, channels_last, merge):
    x, wg = kit_gpu.nchw_gpu(merged_ref.k_canvas(q), channels_last), torch.from_numpy(ref.weights(N, q, c)).cuda()
    for kw in (dict(reduce=None, out_dtype=F32), dict(out_dtype=torch.int32)):
        with kit_gpu.gpu_error_ends_the_session("resize_many_back_queries"):
            want = aa.resize_many_back_queries(x, wg, MEMBER_SIZES, regions=REGIONS, flips=FLIPS, **kw)
        for i, (o, s) in enumerate(zip(call(aa, x, wg, groups=range(N), sizes=MEMBER_SIZES, merge=merge, **kw), want)):
            kit_gpu.assert_bits(o, s, f"{merge} {kw} member {i}")


@pytest.mark.parametrize("lo,hi", ((3, 4), (3, 20), (5, 37), (5, 197)),
                         ids=("same_lane", "across_half_waves", "across_class_blocks", "across_class_passes"))
def test_ties_go_to_the_lower_class(aa, lo, hi):
    """Two copies of one dominating weight column in every member: their scores are the same bits, and the label is the lower index."""
    x = kit_gpu.nchw_gpu(merged_ref.k_canvas(37))
    w = 0.125 * ref.weights(N, 37, 200)
    w[:, :, lo] = w[:, :, hi] = 1.0
    wg = torch.from_numpy(w).cuda()
    for s in call(aa, x, wg, reduce=None):
        kit_gpu.assert_bits(s[lo], s[hi], "the copies' scores")
        assert (s[lo] > 2 * s[[k for k in range(200) if k not in (lo, hi)]].max(0).values).all()
    for lab in call(aa, x, wg, out_dtype=torch.int32):
        assert (lab == lo).all()


def test_a_nan_logit_of_one_member_is_nan_in_every_class_of_its_pixels_only(aa):
    c = np.array(merged_ref.k_canvas(17))
    c[2, 5, 4, 6] = np.nan  # (member 2 of group 0, inside its region)
    x, w = kit_gpu.nchw_gpu(c), ref.weights(N, 17, 70)
    wg = torch.from_numpy(w).cuda()
    got, labs, R = call(aa, x, wg, reduce=None), call(aa, x, wg, out_dtype=torch.uint8), resampled(aa, x)
    want, bnd = merged_scores([np.nan_to_num(r) for r in R], w)
    for g in range(G):
        nan = np.any([np.isnan(R[i]).any(0) for i in merged_ref.members(GROUPS, g)], axis=0)
        assert nan.any() == (g == 0) and not nan.all()
        s = got[g].cpu().numpy()
        assert np.isnan(s[:, nan]).all() and (labs[g].cpu().numpy()[nan] == 0).all()
        assert (np.abs(s - want[g])[:, ~nan] <= bnd[g][:, ~nan]).all()


def test_two_launches_and_refusals(aa):
    x, wg = kit_gpu.nchw_gpu(merged_ref.k_canvas(17)), torch.from_numpy(ref.weights(N, 17, 33)).cuda()
    call(aa, x, wg)  # (code objects loaded)
    assert len(kit_gpu.count_launches(lambda: call(aa, x, wg))) == 2 and len(kit_gpu.count_launches(lambda: call(aa, x, wg, reduce=None))) == 2
    for bad, words in ((dict(groups=GROUPS[:6]), "one entry per item"), (dict(groups=[0, 1, 0, 1, 1, 0, 1]), "group 2 .* has no member"),
                       (dict(sizes=MEMBER_SIZES), "has no member"), (dict(merge="max"), "merge must be 'sum' or 'mean'"),
                       (dict(groups=None, sizes=MEMBER_SIZES, merge="mean"), "needs groups")):
        with pytest.raises(ValueError, match=words):
            aa.resize_many_back_queries(x, wg, **{"sizes": SIZES, "groups": GROUPS, "regions": REGIONS, **bad})
    with pytest.raises(NotImplementedError, match=r"torch\.no_grad\(\).*\.detach\(\)"):
        aa.resize_many_back_queries(x.clone().requires_grad_(), wg, SIZES, regions=REGIONS, groups=GROUPS, reduce=None)


@pytest.mark.parametrize("reduce,dtype", ((None, BF16), ("argmax", torch.uint8)), ids=("values", "labels"))
def test_the_arena_is_written_completely_and_nothing_beside_it(aa, monkeypatch, reduce, dtype):
    x, wg = kit_gpu.nchw_gpu(merged_ref.k_canvas(17), True), torch.from_numpy(ref.weights(N, 17, 33)).cuda()
    want = call(aa, x, wg, reduce=reduce, out_dtype=dtype, merge="mean")
    for fill in (0xFF, 0x00):
        got, gap_bytes, touched = run_guarded(monkeypatch, 1, fill, lambda: call(aa, x, wg, reduce=reduce, out_dtype=dtype, merge="mean"),
                                              f"merged queries {reduce}")
        for g, (o, s) in enumerate(zip(got, want)):
            kit_gpu.assert_bits(o, s, f"reduce={reduce} fill {fill:#x} group {g}")
        assert gap_bytes > 0 and touched == 0
