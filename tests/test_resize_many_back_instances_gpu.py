"""resize_many_back_instances on the GPU against resize_many_back_instances_ref: masks (bytes or packed bits) and stats equal to the
reference — every comparison is equality of integers or bytes — repeated and empty slots, a query whose mask is empty everywhere, NaN
and +inf logits, the launches, the refusals and the guard bands.  Geometry 1 is resize_many_back_ref's base case: a 300-column output
across the 256-column tile, widths 31, 4, 5 and 7 for the bit tails, 23 and 13 rows that are no multiples of the row tile (8 rows as
built; nor of 16), a one-pixel source.  Geometry 2 is two more items of the same canvas at (18, 300) and (33, 70): varied bits across
the tile seam and the wave seam at column 64, full row tiles and one extra row."""
import numpy as np
import pytest
import torch

import kit_gpu
import resize_many_back_instances_ref as ref
import resize_many_back_ref as back_ref
from kit_golden import MODE
from test_resize_many_back_guard_gpu import run_guarded

pytestmark = pytest.mark.gpu

aa = kit_gpu.aa_fixture()

F32, F16, BF16, I32, I64 = torch.float32, torch.float16, torch.bfloat16, torch.int32, torch.int64
REGIONS = back_ref.BASE_REGIONS + [(0, 0, 12, 16), (2, 1, 9, 13)]
SIZES = back_ref.BASE_SIZES + [(18, 300), (33, 70)]
FLIPS, N = [True, False, True, True, False, False, True], len(SIZES)
# Q, filter, channels_last, masks' dtype, format, queries' dtype, M, pattern.  Q below, at and above AA_BACK_UNROLL, 37 (nine steps of
# four distinct queries and one more) and 256; channels_last with Q = 4, 8 and 256 takes the vector loads and chunked entries, with 3
# and 37 not.  The int64 queries lie transposed in memory.
CASES = [(1, "linear", False, F32, "bool", I32, 1, "once"), (3, "cubic", True, F16, "bits", I64, 5, "repeat"),
         (4, "box", True, F32, "bool", I64, 5, "empties"), (8, "linear", True, BF16, "bits", I32, 256, "repeat"),
         (37, "lanczos", False, F32, "bits", I32, 256, "once"), (37, "linear", False, F16, "bool", I64, 5, "empties"),
         (37, "hamming", True, BF16, "bool", I32, 5, "repeat"), (256, "linear", True, F16, "bits", I32, 256, "once"),
         (256, "linear", False, BF16, "bool", I64, 5, "repeat")]


def masks_gpu(c, dtype=F32, channels_last=False):
    """The canvas [5, Q, 12, 16] -> the call's seven items: the five of the base case, then items 0 and 1 again (views, read where they lie)."""
    x = kit_gpu.nchw_gpu(c, channels_last).to(dtype)
    return [x[i] for i in (0, 1, 2, 3, 4, 0, 1)]


def queries_gpu(queries, dtype=I32):
    t = torch.from_numpy(queries).cuda().to(dtype)
    return t.t().contiguous().t() if dtype == I64 else t


def call(aa, x, queries, filt="linear", **kw):
    with kit_gpu.gpu_error_ends_the_session("resize_many_back_instances"):
        return aa.resize_many_back_instances(x, queries, SIZES, MODE[filt], regions=REGIONS, flips=FLIPS, **kw)


def existing(aa, x, filt="linear", **kw):
    """What an existing resize_many_back call gives the same items, as numpy arrays."""
    return [o.cpu().numpy() for o in aa.resize_many_back(x, SIZES, MODE[filt], regions=REGIONS, flips=FLIPS, **kw)]


def check(aa, got, x, queries, filt="linear", fmt="bool"):
    """A call's (masks, stats) against the reference, item by item -> the reference's stats [N, M, 6]."""
    masks, stats = got
    r, p = existing(aa, x, filt, reduce=None, out_dtype=F32), existing(aa, x, filt, reduce=None, out_dtype=F32, activation="sigmoid")
    assert stats.dtype == I64 and tuple(stats.shape) == (N, queries.shape[1], 6) and len(masks) == N
    want = [ref.instances(r[i], p[i], queries[i]) for i in range(N)]
    for i, (wm, wb, ws) in enumerate(want):
        g, w = masks[i].cpu().numpy(), (wb if fmt == "bits" else wm)
        assert g.dtype == w.dtype and g.shape == w.shape and (g == w).all(), (i, np.argwhere(g != w)[:4])
        gs = stats[i].cpu().numpy()
        assert (gs == ws).all(), (i, gs[(gs != ws).any(1)], ws[(gs != ws).any(1)])
    return np.stack([ws for _, _, ws in want])


@pytest.mark.parametrize("q,filt,channels_last,in_dtype,fmt,q_dtype,m,pattern", CASES)
def test_masks_and_stats_equal_the_reference(aa, q, filt, channels_last, in_dtype, fmt, q_dtype, m, pattern):
    c = np.array(back_ref.k_canvas(q))
    if q > 1:
        c[:, q - 1] -= 10.0  # query Q - 1's mask is empty in every item: the words that are 0
    x, queries = masks_gpu(c, in_dtype, channels_last), ref.pattern(pattern, N, q, m)
    got = call(aa, x, queries_gpu(queries, q_dtype), filt, mask_format=fmt)
    stats = check(aa, got, x, queries, filt, fmt)
    low = queries == q - 1
    print(f"Q={q} M={m} {pattern} {fmt}: {int((stats[:, :, 0] > 0).sum())} of {N * m} slots have pixels, {int(low.sum())} ask for the empty query")
    assert (stats[:, :, 0] > 0).any()
    if q > 1:
        identity = np.array([[0, 0, ow, oh, 0, 0] for oh, ow in SIZES])
        assert low.any() and all((stats[i][low[i]] == identity[i]).all() for i in range(N))
    if fmt == "bool":  # the gathered planes of the existing threshold call, bit for bit
        planes = existing(aa, x, filt, reduce="greater", threshold=0.0)
        for i in range(N):
            asked = (queries[i] >= 0) & (queries[i] < q)
            assert (got[0][i].cpu().numpy()[asked] == planes[i][queries[i][asked]]).all() and not got[0][i].cpu().numpy()[~asked].any(), i
    assert torch.equal(aa.boxmath.instance_scores(got[1]).cpu(), torch.from_numpy(stats[:, :, 1] / 2.0 ** 24 / (stats[:, :, 0] + 1e-6)))


def test_nan_and_inf_logits(aa):
    """In a query nobody asked for they change nothing; in an asked query a NaN is outside the mask, a +inf inside with p = 1."""
    clean, dirty = np.array(back_ref.k_canvas(5)), np.array(back_ref.k_canvas(5))
    dirty[0, 3, 5, 6], dirty[0, 3, 2, 9] = np.nan, np.inf  # (query 3 is not asked below, query 1 is)
    queries = np.tile(np.array([1, 0, 4, 1, 2]), (N, 1))
    qg = queries_gpu(queries)
    want, got = call(aa, masks_gpu(clean), qg), call(aa, masks_gpu(dirty), qg)
    for a, b in zip(got[0] + [got[1]], want[0] + [want[1]]):
        kit_gpu.assert_bits(a, b, "NaN and +inf in a query nobody asked for")
    dirty[0, 1, 5, 6], dirty[0, 1, 2, 9] = np.nan, np.inf
    x = masks_gpu(dirty)
    for fmt in ("bool", "bits"):
        check(aa, call(aa, x, qg, mask_format=fmt), x, queries, fmt=fmt)
    r = existing(aa, x, reduce=None, out_dtype=F32)[0][1]
    assert np.isnan(r).any() and np.isposinf(r).any()


def test_two_launches_and_refusals(aa):
    x, qg = masks_gpu(back_ref.k_canvas(37)), queries_gpu(ref.pattern("repeat", N, 37, 100))
    call(aa, x, qg)  # (code objects loaded)
    assert len(kit_gpu.count_launches(lambda: call(aa, x, qg))) == 2
    for bad, words in ((dict(x=[torch.zeros(257, 12, 16, device="cuda")] * N), "Q must be in 1 .. 256"),
                       (dict(q=torch.zeros(N, 257, dtype=I32, device="cuda")), "M must be in 1 .. 256"),
                       (dict(q=torch.zeros(N, 0, dtype=I32, device="cuda")), "M must be in 1 .. 256"),
                       (dict(q=qg.float()), "queries must be torch.int32 or torch.int64"), (dict(q=qg[:3]), r"queries must be \[N, M\]"),
                       (dict(q=qg[0]), r"queries must be \[N, M\]"), (dict(q=qg.cpu()), "queries is on cpu"),
                       (dict(mask_format="rle"), "mask_format must be 'bool' or 'bits'")):
        kw = {"x": x, "q": qg, **bad}
        with pytest.raises(ValueError, match=words):
            aa.resize_many_back_instances(kw.pop("x"), kw.pop("q"), SIZES, regions=REGIONS, **kw)
    with pytest.raises(NotImplementedError, match=r"torch\.no_grad\(\).*\.detach\(\)"):
        aa.resize_many_back_instances([t.clone().requires_grad_() for t in x], qg, SIZES, regions=REGIONS)


@pytest.mark.parametrize("lead,fmt,channels_last", ((0, "bool", True), (1, "bits", False), (0, "bits", True)),
                         ids=("aligned_bool", "eight_byte_bits", "aligned_bits"))
def test_the_arena_is_written_completely_and_nothing_beside_it(aa, monkeypatch, lead, fmt, channels_last):
    """lead 1 puts the arena on an 8-byte-only boundary.  Every slot's mask — asked, repeated or empty — is written in full."""
    x, qg = masks_gpu(back_ref.k_canvas(8), channels_last=channels_last), queries_gpu(ref.pattern("empties", N, 8, 8))
    # (item 0's masks, M = 8 of them, as the int64 words the arena is allocated as: the guard places an output by its element)
    flat = lambda r: [r[0][0].view(torch.uint8).flatten().view(I64)] + r[0][1:] + [r[1]]
    want = flat(call(aa, x, qg, mask_format=fmt))
    for fill in (0xFF, 0x00):
        got, gap_bytes, touched = run_guarded(monkeypatch, lead, fill, lambda: flat(call(aa, x, qg, mask_format=fmt)), f"instances {fmt}")
        for i, (g, w) in enumerate(zip(got, want)):
            kit_gpu.assert_bits(g, w, f"{fmt} fill {fill:#x} output {i}")
        assert gap_bytes > 0 and touched == 0
