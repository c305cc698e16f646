"""resize_many_back_confusion on the GPU: numpy's fast_hist of the CPU restatements' labels (with an activation: of the labels the existing
calls return), exact; every matrix sums to its counted pixels.  Plain and merged, the tie and NaN rules, ignored targets, K = 1, the slot
evictions of K = 300, 70 outputs, targets and predictions read where they lie, two launches, the same bits twice, no label map."""
import numpy as np
import pytest
import torch

import kit_gpu
import resize_many_back_merged_ref as mref
import resize_many_back_ref as ref
from interpolate_antialiasing_amd import _lib
from kit_golden import MODE

pytestmark = pytest.mark.gpu

aa = kit_gpu.aa_fixture()

ROWS = _lib.BACK_CONF_ROWS
TALL = (2 * ROWS + 1, 9)  # one more output, of 2 * ROWS + 1 rows: two full row tiles and a tail
NP = {torch.uint8: np.uint8, torch.int16: np.int16, torch.int32: np.int32, torch.int64: np.int64}
# form -> (canvas by name, regions, groups, sizes, flips): the base cases of the two restatements, item 0 once more at TALL
PLAIN = (dict(base=ref.BASE_CANVAS, tie=ref.tie_canvas(), nonfinite=ref.nonfinite_canvas()), ref.BASE_REGIONS + [(2, 1, 9, 11)], None,
         ref.BASE_SIZES + [TALL], [False, True, False, True, False, True])
MERGED = (dict(base=mref.BASE_CANVAS, tie=mref.tie_canvas(), nonfinite=mref.nonfinite_canvas()), mref.BASE_REGIONS + [(2, 1, 9, 11)],
          mref.BASE_GROUPS + [3], mref.BASE_SIZES + [TALL], mref.BASE_FLIPS + [True])
FORMS = {"plain": PLAIN, "merged": MERGED}


def fast_hist(t, p, k):
    t, p = t.astype(np.int64).ravel(), p.astype(np.int64).ravel()
    keep = (t >= 0) & (t < k)
    return np.bincount(k * t[keep] + p[keep], minlength=k * k).reshape(k, k)


def make_targets(sizes, k, dtype, seed=3, ignore=True):
    """Seeded targets uniform over 0 .. K - 1 with, where the dtype holds them, 255, -1 and K sprinkled in: none of the three is counted."""
    rng, out = np.random.default_rng(seed), []
    lim = np.iinfo(NP[dtype])
    for oh, ow in sizes:
        t = rng.integers(0, k, (oh, ow)).astype(np.int64)
        for v in (255, -1, k) if ignore else ():
            if lim.min <= v <= lim.max and not 0 <= v < k:
                t[rng.random((oh, ow)) < 0.1] = v
        out.append(t.astype(NP[dtype]))
    return out


def run(aa, x, targets, mode="bilinear", **kw):
    with kit_gpu.gpu_error_ends_the_session("resize_many_back_confusion"):
        return aa.resize_many_back_confusion(x, [torch.from_numpy(t).cuda() if isinstance(t, np.ndarray) else t for t in targets], mode, **kw)


def labels(aa, filt, c, regions, groups, sizes, flips, activation=None, merge="sum"):
    """The reference labels: the restatements' on the CPU; with an activation those the existing call returns."""
    if activation is not None:
        kw = dict(regions=regions, flips=flips, reduce="argmax", activation=activation)
        x = kit_gpu.nchw_gpu(c)
        labs = aa.resize_many_back(x, sizes, MODE[filt], **kw) if groups is None else aa.resize_many_back_merged(x, groups, sizes, MODE[filt], merge=merge, **kw)
        return [t.cpu().numpy() for t in labs]
    if groups is None:
        return ref.labels(ref.values(filt, c, regions, sizes, flips))
    return mref.labels(mref.merged_values(filt, c, regions, groups, sizes, flips, merge))


def check(conf, labs, targets, k, what):
    assert conf.dtype == torch.int64 and tuple(conf.shape) == (len(labs), k, k) and conf.grad_fn is None and conf.is_contiguous()
    got = conf.cpu().numpy()
    for i, (lab, t) in enumerate(zip(labs, targets)):
        assert np.array_equal(got[i], fast_hist(t, lab, k)), f"{what}: output {i}"
        assert got[i].sum() == ((t.astype(np.int64) >= 0) & (t.astype(np.int64) < k)).sum(), f"{what}: output {i} counts every kept pixel once"


def case(form, canvas="base"):
    canvases, regions, groups, sizes, flips = FORMS[form]
    c = canvases[canvas]
    return (np.concatenate([c, c[:1]]), regions, groups, sizes, flips)


@pytest.mark.parametrize("dtype", tuple(NP), ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("activation", (None, "softmax"))
@pytest.mark.parametrize("filt", ("linear", "cubic"))
@pytest.mark.parametrize("form", tuple(FORMS))
def test_equals_fast_hist_of_the_labels(aa, form, filt, activation, dtype):
    c, regions, groups, sizes, flips = case(form)
    targets = make_targets(sizes, 7, dtype)
    assert any(((t.astype(np.int64) < 0) | (t.astype(np.int64) >= 7)).any() for t in targets) or dtype == torch.uint8
    labs = labels(aa, filt, c, regions, groups, sizes, flips, activation)
    conf = run(aa, kit_gpu.nchw_gpu(c), targets, MODE[filt], regions=regions, flips=flips, groups=groups, activation=activation)
    check(conf, labs, targets, 7, f"{form} {filt} {activation} {dtype}")
    if form == "merged" and dtype == torch.int64:  # (the mean, and a pred that requires grad, which never raises)
        labs = labels(aa, filt, c, regions, groups, sizes, flips, activation, "mean")
        x = kit_gpu.nchw_gpu(c).requires_grad_()
        check(run(aa, x, targets, MODE[filt], regions=regions, flips=flips, groups=groups, activation=activation, merge="mean"), labs, targets, 7, "mean")


@pytest.mark.parametrize("canvas", ("tie", "nonfinite"))
@pytest.mark.parametrize("form", tuple(FORMS))
def test_lowest_index_wins_and_the_nan_wins(aa, form, canvas):
    c, regions, groups, sizes, flips = case(form, canvas)
    targets = make_targets(sizes, 7, torch.int16)
    labs = labels(aa, "linear", c, regions, groups, sizes, flips)
    for channels_last in (False, True):
        conf = run(aa, kit_gpu.nchw_gpu(c, channels_last), targets, regions=regions, flips=flips, groups=groups)
        check(conf, labs, targets, 7, f"{form} {canvas} cl={channels_last}")
    if canvas == "tie":
        assert not conf[:, :, 4].any() and conf[:, :, 2].any()


@pytest.mark.parametrize("form", tuple(FORMS))
def test_k_of_one_and_k_of_300_with_evictions(aa, form):
    c, regions, groups, sizes, flips = case(form)
    targets = make_targets(sizes, 1, torch.int64)
    conf = run(aa, kit_gpu.nchw_gpu(c[:, :1]), targets, regions=regions, flips=flips, groups=groups)
    check(conf, [np.zeros(s, np.int64) for s in sizes], targets, 1, f"{form} K = 1")
    # K = 300: noise logits, targets uniform over the classes; some wave's tile (64 columns by ROWS rows) holds more keys than it has slots
    c, regions, groups = (ref.k300_case()[0], [(0, 0, 3, 3)], None) if form == "plain" else mref.k300_case()[:3]
    sizes = [(2 * ROWS + 1, 70)]
    targets = make_targets(sizes, 300, torch.int16, ignore=False)
    labs = labels(aa, "linear", c, regions, groups, sizes, None)
    keys = 300 * targets[0].astype(np.int64) + labs[0]
    assert max(len(np.unique(keys[y:y + ROWS, x:x + 64])) for y in range(0, sizes[0][0], ROWS) for x in (0, 64)) >= 65
    check(run(aa, kit_gpu.nchw_gpu(c), targets, regions=regions, groups=groups), labs, targets, 300, f"{form} K = 300")


@pytest.mark.parametrize("form", tuple(FORMS))
def test_seventy_outputs_two_launches_and_the_same_bits_twice(aa, form):
    if form == "plain":
        (c, regions, sizes), groups, flips = ref.seventy_case(), None, None
    else:
        c, regions, groups, sizes, flips = mref.seventy_case()
    targets = make_targets(sizes, 3, torch.uint8)
    x, tg = kit_gpu.nchw_gpu(c), [torch.from_numpy(t).cuda() for t in targets]
    kw = dict(regions=regions, flips=flips, groups=groups)
    conf = run(aa, x, tg, **kw)
    check(conf, labels(aa, "linear", c, regions, groups, sizes, flips), targets, 3, f"{form} seventy")
    assert torch.equal(run(aa, x, tg, **kw), conf)
    one = dict(regions=regions[:1], flips=None, groups=None if groups is None else [0])
    for args in ((x, tg, kw), (x[:1], [torch.zeros((4, 4), dtype=torch.uint8, device="cuda")], one)):
        names = kit_gpu.count_launches(lambda: aa.resize_many_back_confusion(args[0], args[1], **args[2]))
        assert len(names) == 2, names


def test_targets_are_read_where_they_lie(aa):
    c, regions, groups, sizes, flips = case("plain")
    targets = make_targets(sizes, 7, torch.int32)
    x, pitched, strided = kit_gpu.nchw_gpu(c), [], []
    for t in targets:
        big = torch.full((t.shape[0] + 3, t.shape[1] + 5), 3, dtype=torch.int32, device="cuda")  # (a counted class all around)
        big[1:1 + t.shape[0], 3:3 + t.shape[1]] = torch.from_numpy(t).cuda()
        pitched.append(big[1:1 + t.shape[0], 3:3 + t.shape[1]])
        strided.append(torch.from_numpy(np.repeat(t, 2, axis=1)).cuda()[:, ::2])  # (a column stride of 2: copied first)
    labs = labels(aa, "linear", c, regions, groups, sizes, flips)
    for form, tg in (("pitched", pitched), ("strided", strided)):
        check(run(aa, x, tg, regions=regions, flips=flips), labs, targets, 7, form)
    names = kit_gpu.count_launches(lambda: aa.resize_many_back_confusion(x, pitched, regions=regions, flips=flips))
    assert len(names) == 2, names


def test_no_label_map_is_allocated(aa):
    """K = 8, one 12 x 16 item to (96, 128): the 512-byte result, two tables and the descriptor stay under the 98 KB of ONE int64 label map."""
    k, oh, ow = 8, 96, 128
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((1, k, 12, 16)).astype(np.float32)).cuda()
    tg = [torch.from_numpy(make_targets([(oh, ow)], k, torch.uint8)[0]).cuda()]
    want = run(aa, x, tg)  # (code objects loaded, the pinned block cached)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    conf = run(aa, x, tg)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    print(f"peak memory grew by {grown} bytes; one int64 label map is {oh * ow * 8}")
    assert grown < oh * ow * 8 and torch.equal(conf, want)
    lab = aa.resize_many_back(x, [(oh, ow)], reduce="argmax")[0].cpu().numpy()
    check(conf, [lab], [tg[0].cpu().numpy()], k, "against the argmax call")
