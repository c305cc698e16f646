"""resize_many_back_queries on the GPU against resize_many_back_queries_ref: the scores within the reference's bound, the labels equal
to the float64 argmax wherever the bound decides it, exact ties, padding, a NaN, the launches, the refusals and the guard bands.  The
geometry is resize_many_back_ref's base case: a 300-column output that crosses the 256-column tile, one-pixel and one-column sources,
flips and cropped regions."""
import numpy as np
import pytest
import torch

import kit_gpu
import resize_many_back_queries_ref as ref
import resize_many_back_ref as back_ref
from kit_golden import MODE
from test_resize_many_back_guard_gpu import run_guarded

pytestmark = pytest.mark.gpu

WORST = [0.0]
aa = kit_gpu.aa_fixture(lambda: print(f"\nresize_many_back_queries: worst error / bound = {WORST[0]:.4f}"))

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
REGIONS, SIZES, FLIPS, N = back_ref.BASE_REGIONS, back_ref.BASE_SIZES, [True, False, True, True, False], len(back_ref.BASE_SIZES)
ROUND = {F32: 0.0, F16: 2.0 ** -11, BF16: 2.0 ** -8}  # one rounding to nearest of the output type, relative
# Q, C, filter, channels_last, masks' dtype, scores' dtype, labels' dtype, the weights' sign.  Q below, at and above the 16 of a matrix
# step and 256 once; C below, at and above the 32 of a class block; (16, 32) and (256, 70) channels_last take the vector loads.
CASES = [(1, 1, "linear", False, F32, F32, torch.uint8, 1), (15, 31, "cubic", True, F16, F16, torch.int16, 1),
         (16, 32, "box", True, F32, F32, torch.int32, 1), (17, 33, "hamming", False, BF16, BF16, torch.int64, 1),
         (37, 70, "lanczos", False, F32, F32, torch.uint8, 1), (256, 70, "linear", True, F16, BF16, torch.uint8, 1),
         # padded classes never win: every true score is below the zero of classes 33 .. 63
         (17, 33, "linear", True, F32, F16, torch.uint8, -1)]


def masks_gpu(c, dtype=F32, channels_last=False):
    return kit_gpu.nchw_gpu(c, channels_last).to(dtype)


def call(aa, x, w, filt="linear", **kw):
    with kit_gpu.gpu_error_ends_the_session("resize_many_back_queries"):
        return aa.resize_many_back_queries(x, w, SIZES, MODE[filt], regions=REGIONS, flips=FLIPS, **kw)


def resampled(aa, x, filt="linear"):
    """The fp32 R_i of the existing call, as numpy arrays."""
    return [o.cpu().numpy() for o in aa.resize_many_back(x, SIZES, MODE[filt], regions=REGIONS, flips=FLIPS, reduce=None, out_dtype=F32)]


@pytest.mark.parametrize("q,c,filt,channels_last,in_dtype,out_dtype,label_dtype,sign", CASES)
def test_scores_within_the_bound_and_labels_where_decided(aa, q, c, filt, channels_last, in_dtype, out_dtype, label_dtype, sign):
    x = masks_gpu(back_ref.k_canvas(q), in_dtype, channels_last)
    w = ref.weights(N, q, c, sign)
    # (the weights of a channels_last case lie transposed in memory, the queries consecutive: read where they lie)
    wg = torch.from_numpy(np.ascontiguousarray(w.transpose(0, 2, 1))).cuda().transpose(1, 2) if channels_last else torch.from_numpy(w).cuda()
    want, bnd = zip(*(ref.scores(r, w[i]) for i, r in enumerate(resampled(aa, x, filt))))
    for dt in dict.fromkeys((F32, out_dtype)):
        for i, (o, s, b) in enumerate(zip(call(aa, x, wg, filt, reduce=None, out_dtype=dt), want, bnd)):
            assert o.dtype == dt and tuple(o.shape) == s.shape
            err, lim = np.abs(o.float().cpu().numpy().astype(np.float64) - s), b + ROUND[dt] * (np.abs(s) + b)
            if dt == F32:
                WORST[0] = max(WORST[0], float((err / b).max()))
            assert (err <= lim).all(), (i, dt, float((err / lim).max()))
    ok, arg = ref.decided(want, bnd)
    share = sum(int(o.sum()) for o in ok) / back_ref.BASE_PIXELS
    print(f"Q={q} C={c}: {100 * share:.2f} % of the pixels decided, worst error / bound so far {WORST[0]:.4f}")
    assert share >= 0.9
    for i, (lab, o, a) in enumerate(zip(call(aa, x, wg, filt, out_dtype=label_dtype), ok, arg)):
        assert lab.dtype == label_dtype and tuple(lab.shape) == o.shape
        assert (lab.cpu().numpy()[o] == a[o]).all(), i


@pytest.mark.parametrize("lo,hi", ((3, 4), (3, 20), (5, 37)), ids=("same_lane", "across_half_waves", "across_class_blocks"))
def test_ties_go_to_the_lower_class(aa, lo, hi):
    """Two copies of one dominating weight column: their scores are the same bits, and the label is the lower index at every pixel."""
    x = masks_gpu(back_ref.k_canvas(37))
    w = 0.125 * ref.weights(N, 37, 40)
    w[:, :, lo] = w[:, :, hi] = 1.0
    wg = torch.from_numpy(w).cuda()
    for s in call(aa, x, wg, reduce=None):
        kit_gpu.assert_bits(s[lo], s[hi], "the copies' scores")
        assert (s[lo] > 2 * s[[k for k in range(40) if k not in (lo, hi)]].max(0).values).all()
    for lab in call(aa, x, wg, out_dtype=torch.int32):
        assert (lab == lo).all()


def test_a_nan_logit_is_nan_in_every_class_of_its_pixels_only(aa):
    c = np.array(back_ref.k_canvas(17))
    c[0, 5, 4, 6] = np.nan
    x, w = masks_gpu(c), ref.weights(N, 17, 33)
    wg = torch.from_numpy(w).cuda()
    got, labs = call(aa, x, wg, reduce=None), call(aa, x, wg, out_dtype=torch.uint8)
    for i, r in enumerate(resampled(aa, x)):
        nan = np.isnan(r).any(0)
        assert nan.any() == (i == 0) and not nan.all()
        s = got[i].cpu().numpy()
        assert np.isnan(s[:, nan]).all() and (labs[i].cpu().numpy()[nan] == 0).all()
        want, bnd = ref.scores(np.nan_to_num(r), w[i])
        assert (np.abs(s - want)[:, ~nan] <= bnd[:, ~nan]).all()


def test_two_launches_and_refusals(aa):
    x, wg = masks_gpu(back_ref.k_canvas(17)), torch.from_numpy(ref.weights(N, 17, 33)).cuda()
    call(aa, x, wg)  # (code objects loaded)
    assert len(kit_gpu.count_launches(lambda: call(aa, x, wg))) == 2 and len(kit_gpu.count_launches(lambda: call(aa, x, wg, reduce=None))) == 2
    for bad, words in ((dict(x=torch.zeros(N, 257, 12, 16, device="cuda")), "Q must be in 1 .. 256"), (dict(w=wg[:, :16]), "16 queries"),
                       (dict(w=wg[:4]), "one entry per item"), (dict(w=wg.double()), "must be torch.float32"),
                       (dict(w=wg.repeat(1, 1, 8), out_dtype=torch.uint8), "holds labels below 256")):
        kw = {"x": x, "w": wg, **bad}
        with pytest.raises(ValueError, match=words):
            aa.resize_many_back_queries(kw.pop("x"), kw.pop("w"), SIZES, regions=REGIONS, **kw)
    for grad in (dict(x=x.clone().requires_grad_()), dict(w=wg.clone().requires_grad_())):
        kw = {"x": x, "w": wg, **grad}
        with pytest.raises(NotImplementedError, match=r"torch\.no_grad\(\).*\.detach\(\)"):
            aa.resize_many_back_queries(kw["x"], kw["w"], SIZES, regions=REGIONS, reduce=None)
        assert all(o.grad_fn is None for o in aa.resize_many_back_queries(kw["x"], kw["w"], SIZES, regions=REGIONS))


@pytest.mark.parametrize("reduce,dtype", ((None, BF16), ("argmax", torch.uint8)), ids=("values", "labels"))
def test_the_arena_is_written_completely_and_nothing_beside_it(aa, monkeypatch, reduce, dtype):
    x, wg = masks_gpu(back_ref.k_canvas(17), channels_last=True), torch.from_numpy(ref.weights(N, 17, 33)).cuda()
    want = call(aa, x, wg, reduce=reduce, out_dtype=dtype)
    for fill in (0xFF, 0x00):
        got, gap_bytes, touched = run_guarded(monkeypatch, 1, fill, lambda: call(aa, x, wg, reduce=reduce, out_dtype=dtype), f"queries {reduce}")
        for i, (g, w) in enumerate(zip(got, want)):
            kit_gpu.assert_bits(g, w, f"reduce={reduce} fill {fill:#x} item {i}")
        assert gap_bytes > 0 and touched == 0
