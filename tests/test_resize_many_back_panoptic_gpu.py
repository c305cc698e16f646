"""resize_many_back_panoptic on the GPU against resize_many_back_panoptic_ref: maps, counts and survives equal to the reference — every
comparison is equality of integers — ties, the threshold's edge, NaN logits, shared ids and void, the launches, the refusals and the
guard bands.  The geometry is resize_many_back_ref's base case: a 300-column output that crosses the 256-column tile, one-pixel and
one-column sources, flips, cropped regions and a 23- and a 13-row output that are no multiples of the 16-row tile."""
import numpy as np
import pytest
import torch

import kit_gpu
import resize_many_back_panoptic_ref as ref
import resize_many_back_ref as back_ref
from kit_golden import MODE
from test_resize_many_back_guard_gpu import run_guarded

pytestmark = pytest.mark.gpu

aa = kit_gpu.aa_fixture()

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
REGIONS, SIZES, FLIPS, N = back_ref.BASE_REGIONS, back_ref.BASE_SIZES, [True, False, True, True, False], len(back_ref.BASE_SIZES)
# Q, filter, channels_last, masks' dtype, map dtype, kept pattern.  Q below, at and above AA_BACK_UNROLL, 37 (nine steps of four kept
# queries and one more) and 256; channels_last with Q = 4, 8 and 256 takes the vector loads and chunked kept lists, with 3 and 37 not.
CASES = [(1, "linear", False, F32, torch.uint8, "all"), (3, "cubic", True, F16, torch.int16, "all"), (4, "box", True, F32, torch.int32, "edges"),
         (5, "hamming", False, BF16, torch.int64, "edges"), (8, "linear", True, BF16, torch.uint8, "none0"),
         (37, "lanczos", False, F32, torch.uint8, "all"), (37, "linear", False, F16, torch.int16, "none0"), (37, "cubic", True, F32, torch.int32, "one"),
         (256, "linear", True, F16, torch.int16, "edges"), (256, "linear", False, F32, torch.int32, "all")]


def masks_gpu(c, dtype=F32, channels_last=False):
    return kit_gpu.nchw_gpu(c, channels_last).to(dtype)


def call(aa, x, scores, filt="linear", **kw):
    with kit_gpu.gpu_error_ends_the_session("resize_many_back_panoptic"):
        return aa.resize_many_back_panoptic(x, scores, SIZES, MODE[filt], regions=REGIONS, flips=FLIPS, **kw)


def probabilities(aa, x, filt="linear"):
    """p of the existing call, as numpy arrays."""
    return [o.cpu().numpy() for o in aa.resize_many_back(x, SIZES, MODE[filt], regions=REGIONS, flips=FLIPS, activation="sigmoid", reduce=None,
                                                         out_dtype=F32)]


def check(got, p, scores, ids=None, **kw):
    """A call's (maps, counts, survives) against the reference, item by item -> the reference's counts and survives."""
    maps, counts, survives = got
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (N, scores.shape[1], 3) and tuple(survives.shape) == (N, scores.shape[1])
    want = [ref.panoptic(p[i], scores[i], None if ids is None else ids[i], **kw) for i in range(N)]
    for i, (m, c, s) in enumerate(want):
        g = maps[i].cpu().numpy()
        assert g.dtype == m.dtype and g.shape == m.shape and (g == m).all(), (i, np.argwhere(g != m)[:4])
        gc = counts[i].cpu().numpy()
        assert (gc == c).all(), (i, gc[(gc != c).any(1)], c[(gc != c).any(1)])
        assert (survives[i].cpu().numpy().astype(bool) == s).all(), i
    return np.stack([c for _, c, _ in want]), np.stack([s for _, _, s in want])


@pytest.mark.parametrize("q,filt,channels_last,in_dtype,label_dtype,kept", CASES)
def test_maps_counts_and_survives_equal_the_reference(aa, q, filt, channels_last, in_dtype, label_dtype, kept):
    x = masks_gpu(back_ref.k_canvas(q), in_dtype, channels_last)
    scores = ref.pattern(kept, N, q)
    ids = (np.arange(N * q, dtype=np.int32).reshape(N, q) * 7) % 200  # (queries 0 and 1 share an id)
    ids[:, :2] = 201
    void, dtype = (255 if label_dtype == torch.uint8 else -1), np.dtype(str(label_dtype).split(".")[1])
    p = probabilities(aa, x, filt)
    # the threshold: the median area / original of the reference's queries with positive counts, so that some survive and some do not
    c0 = np.stack([ref.panoptic(p[i], scores[i])[1] for i in range(N)]).reshape(-1, 3)
    c0 = c0[(c0 > 0).all(1)]
    thr = float(np.median(c0[:, 0] / c0[:, 1]))
    # (scores and ids transposed in memory for the channels_last cases: read where they lie)
    sg, ig = torch.from_numpy(scores).cuda(), torch.from_numpy(ids).cuda()
    if channels_last:
        sg, ig = sg.t().contiguous().t(), ig.t().contiguous().t()
    got = call(aa, x, sg, filt, ids=ig, void=void, overlap_threshold=thr, out_dtype=label_dtype)
    counts, survives = check(got, p, scores, ids, void=void, overlap_threshold=thr, dtype=dtype)
    print(f"Q={q} {kept}: threshold {thr:.4f}, {int(survives.sum())} of {int((scores > 0).sum())} kept queries survive, "
          f"{int(counts[:, :, 2].sum())} of {back_ref.BASE_PIXELS} pixels inside")
    assert kept == "none0" or survives.any()
    if kept == "none0":
        assert (counts[0] == 0).all() and not survives[0].any() and (got[0][0] == void).all()


def test_ties_go_to_the_lower_query(aa):
    """Two kept queries with copied masks and equal scores: the lower wins every pixel the pair wins, the higher has no area."""
    c = np.array(back_ref.k_canvas(6))
    c[:, 4] = c[:, 2]
    x, scores = masks_gpu(c), ref.pattern("all", N, 6)
    scores[:, 4] = scores[:, 2] = 2.0
    p = probabilities(aa, x)
    got = call(aa, x, torch.from_numpy(scores).cuda(), overlap_threshold=0.0)
    counts, survives = check(got, p, scores, overlap_threshold=0.0)
    assert (counts[:, 4, 0] == 0).all() and not survives[:, 4].any() and (counts[:, 2, 0] > 0).all() and survives[:, 2].all()
    assert (counts[:, 4, 1] == counts[:, 2, 1]).all()  # (original does not depend on the winner)


def test_the_threshold_edge(aa):
    """overlap_threshold at a surviving query's own area / original: it survives; one float64 step above: it does not, and its pixels are void."""
    x, scores = masks_gpu(back_ref.k_canvas(5)), ref.pattern("all", N, 5)
    p, sg = probabilities(aa, x), torch.from_numpy(scores).cuda()
    c = ref.panoptic(p[0], scores[0])[1]
    k = int(np.argmax(c[:, 2] > 0))
    at = int(c[k, 0]) / int(c[k, 1])
    for thr, alive in ((at, True), (float(np.nextafter(at, np.inf)), False)):
        got = call(aa, x, sg, overlap_threshold=thr)
        _, survives = check(got, p, scores, overlap_threshold=thr)
        assert bool(survives[0, k]) == alive and bool((got[0][0] == k).any()) == alive


def test_nan_logits(aa):
    """In a dropped query's mask a NaN changes nothing; in a kept query's it follows the rule, and only at the pixels it reaches."""
    clean, dirty = np.array(back_ref.k_canvas(5)), np.array(back_ref.k_canvas(5))
    dirty[0, 1, 5, 6] = np.nan  # (query 1 is dropped below, query 3 kept)
    scores = ref.pattern("all", N, 5)
    scores[:, 1] = 0.0
    sg = torch.from_numpy(scores).cuda()
    want = call(aa, masks_gpu(clean), sg, overlap_threshold=0.0)
    got = call(aa, masks_gpu(dirty), sg, overlap_threshold=0.0)
    for a, b in zip(got[0] + list(got[1:]), want[0] + list(want[1:])):
        kit_gpu.assert_bits(a, b, "a NaN in a dropped query")
    dirty[0, 3, 5, 6] = np.nan
    x = masks_gpu(dirty)
    p = probabilities(aa, x)
    got = call(aa, x, sg, overlap_threshold=0.0)
    check(got, p, scores, overlap_threshold=0.0)
    nan = np.isnan(p[0][3])
    assert nan.any() and not nan.all() and (got[0][0].cpu().numpy()[nan] == -1).all()  # (the NaN wins and is not inside)
    assert (got[0][0].cpu().numpy()[~nan] == want[0][0].cpu().numpy()[~nan]).all()
    for i in range(1, N):
        kit_gpu.assert_bits(got[0][i], want[0][i], f"item {i} is not reached")


def test_three_launches_and_refusals(aa):
    x, sg = masks_gpu(back_ref.k_canvas(37)), torch.from_numpy(ref.pattern("all", N, 37)).cuda()
    call(aa, x, sg)  # (code objects loaded)
    assert len(kit_gpu.count_launches(lambda: call(aa, x, sg))) == 3
    big = torch.zeros(N, 256, 12, 16, device="cuda")
    for bad, words in ((dict(x=torch.zeros(N, 257, 12, 16, device="cuda")), "Q must be in 1 .. 256"), (dict(s=sg[:, :16]), r"scores must be \[N, Q\]"),
                       (dict(s=sg.double()), "scores must be torch.float32"), (dict(s=sg.cpu()), "scores is on cpu"),
                       (dict(ids=sg.long()), "ids must be torch.int32"), (dict(ids=torch.zeros(N, 3, dtype=torch.int32, device="cuda")), "ids must be"),
                       (dict(void=256, out_dtype=torch.uint8), "void must be an int that torch.uint8 holds"), (dict(void=1.5), "void must be an int"),
                       (dict(x=big, s=torch.ones(N, 256, device="cuda"), void=0, out_dtype=torch.uint8), "got Q = 256")):
        kw = {"x": x, "s": sg, **bad}
        with pytest.raises(ValueError, match=words):
            aa.resize_many_back_panoptic(kw.pop("x"), kw.pop("s"), SIZES, regions=REGIONS, **kw)
    for grad in (dict(x=x.clone().requires_grad_()), dict(s=sg.clone().requires_grad_())):
        kw = {"x": x, "s": sg, **grad}
        with pytest.raises(NotImplementedError, match=r"torch\.no_grad\(\).*\.detach\(\)"):
            aa.resize_many_back_panoptic(kw["x"], kw["s"], SIZES, regions=REGIONS)


@pytest.mark.parametrize("lead,dtype,channels_last", ((0, torch.uint8, True), (1, torch.int64, False)), ids=("aligned_u8", "eight_byte_i64"))
def test_the_arena_is_written_completely_and_nothing_beside_it(aa, monkeypatch, lead, dtype, channels_last):
    """lead 1 puts the maps on 8-byte-only boundaries: the finalise's 16-byte pieces begin and end inside them."""
    x, sg = masks_gpu(back_ref.k_canvas(8), channels_last=channels_last), torch.from_numpy(ref.pattern("all", N, 8)).cuda()
    flat = lambda r: r[0] + [r[1], r[2]]
    want = flat(call(aa, x, sg, overlap_threshold=0.1, out_dtype=dtype, void=7))
    for fill in (0xFF, 0x00):
        got, gap_bytes, touched = run_guarded(monkeypatch, lead, fill, lambda: flat(call(aa, x, sg, overlap_threshold=0.1, out_dtype=dtype, void=7)),
                                              f"panoptic {dtype}")
        for i, (g, w) in enumerate(zip(got, want)):
            kit_gpu.assert_bits(g, w, f"{dtype} fill {fill:#x} output {i}")
        assert gap_bytes > 0 and touched == 0
