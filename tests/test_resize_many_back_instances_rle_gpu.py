"""resize_many_back_instances_rle on the GPU against resize_many_back_instances_rle_ref fed with the masks of the existing
resize_many_back_instances(mask_format="bool") call on the same inputs — every comparison is equality of integers.  The geometry is the
instance test's: 300 columns cross four 64-column strips and the 256-column tile, widths 4, 5, 7 and 31 leave a partial word, 13, 23
and 33 rows are no multiples of the row tile, one item is a single source pixel."""
import numpy as np
import pytest
import torch

import kit_gpu
import resize_many_back_instances_ref as inst_ref
import resize_many_back_instances_rle_ref as ref
import resize_many_back_ref as back_ref
from kit_golden import MODE
from test_resize_many_back_guard_gpu import run_guarded
from test_resize_many_back_instances_gpu import FLIPS, N, REGIONS, SIZES, masks_gpu, queries_gpu

pytestmark = pytest.mark.gpu

aa = kit_gpu.aa_fixture()

F32, F16, BF16, I32, I64 = torch.float32, torch.float16, torch.bfloat16, torch.int32, torch.int64
LAUNCHES = 3  # tables, resample into bit planes, encode (README)
# Q, filter, channels_last, masks' dtype, queries' dtype, M, pattern.  channels_last with Q = 4 and 256 takes the vector loads and the
# chunked entries; Q <= M indexes a query's plane by the query, M < Q by its first place among the sorted slots.
CASES = [(1, "linear", False, F32, I32, 1, "once"), (4, "box", True, F32, I64, 5, "empties"), (37, "lanczos", False, F16, I32, 256, "once"),
         (37, "linear", False, BF16, I64, 5, "repeat"), (256, "linear", True, F16, I32, 256, "once"), (256, "cubic", False, BF16, I64, 5, "empties")]


def inputs(q, pattern="repeat", m=5, channels_last=False, dtype=F32):
    """The canvas with query Q - 1 lowered by 10 (empty in every item: the row [oh ow]) and query Q // 2 raised by 10 (set everywhere:
    [0, oh ow], a leading zero count and a run carried across every column), the latter asked in slot 0 of items 0, 1 and 3."""
    c, queries = np.array(back_ref.k_canvas(q)), inst_ref.pattern(pattern, N, q, m)
    if q > 1:
        c[:, q - 1] -= 10.0
        c[:, q // 2] += 10.0
        queries[[0, 1, 3], 0] = q // 2
    return masks_gpu(c, dtype, channels_last), queries


def call(aa, x, queries, max_runs, filt="linear"):
    with kit_gpu.gpu_error_ends_the_session("resize_many_back_instances_rle"):
        return aa.resize_many_back_instances_rle(x, queries, SIZES, MODE[filt], regions=REGIONS, flips=FLIPS, max_runs=max_runs)


def check(aa, got, x, qg, max_runs, filt="linear"):
    """A call's (runs, nruns, stats) against the reference rows of the bool call's masks and that call's stats -> nruns."""
    masks, stats = aa.resize_many_back_instances(x, qg, SIZES, MODE[filt], regions=REGIONS, flips=FLIPS)
    runs, nruns = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert runs.dtype == np.int32 and nruns.dtype == np.int32 and runs.shape == (N, qg.shape[1], max_runs) and nruns.shape == runs.shape[:2]
    for i in range(N):
        want_runs, want_nruns = ref.rows(masks[i].cpu().numpy(), max_runs)
        assert (nruns[i] == want_nruns).all(), (i, nruns[i], want_nruns)
        assert (runs[i] == want_runs).all(), (i, np.argwhere(runs[i] != want_runs)[:4])
    kit_gpu.assert_bits(got[2], stats, "stats")
    return nruns


@pytest.mark.parametrize("q,filt,channels_last,in_dtype,q_dtype,m,pattern", CASES)
def test_runs_equal_the_reference(aa, q, filt, channels_last, in_dtype, q_dtype, m, pattern):
    x, queries = inputs(q, pattern, m, channels_last, in_dtype)
    qg = queries_gpu(queries, q_dtype)
    got = call(aa, x, qg, 4096, filt)
    nruns = check(aa, got, x, qg, 4096, filt)
    print(f"Q={q} M={m} {pattern}: nruns up to {nruns.max()}, {int((nruns > 64).sum())} of {nruns.size} slots above 64")
    assert (nruns <= 4096).all() and (nruns > 64).any()
    if q > 1:
        runs, pixels = got[0].cpu().numpy(), np.array([oh * ow for oh, ow in SIZES])[:, None]
        low, full = queries == q - 1, queries == q // 2
        assert low.any() and full.any() and (nruns[low] == 1).all() and (nruns[full] == 2).all()
        assert (runs[:, :, 0][low] == np.broadcast_to(pixels, low.shape)[low]).all()
        assert (runs[:, :, 0][full] == 0).all() and (runs[:, :, 1][full] == np.broadcast_to(pixels, full.shape)[full]).all()


@pytest.mark.parametrize("max_runs", (1, 3))
def test_overflow_keeps_the_first_runs_and_the_true_count(aa, max_runs):
    x, queries = inputs(37, "empties", 8)
    qg = queries_gpu(queries)
    nruns = check(aa, call(aa, x, qg, max_runs), x, qg, max_runs)
    assert (nruns > max_runs).any() and (nruns <= max_runs).any() and torch.equal(call(aa, x, qg, 4096)[1].cpu(), torch.from_numpy(nruns))


def test_nan_and_inf_logits(aa):
    """In a query nobody asked for they change nothing; in an asked query a NaN is outside the mask and a +inf inside."""
    clean, dirty = np.array(back_ref.k_canvas(5)), np.array(back_ref.k_canvas(5))
    dirty[0, 3, 5, 6], dirty[0, 3, 2, 9] = np.nan, np.inf  # (query 3 is not asked below, query 1 is)
    qg = queries_gpu(np.tile(np.array([1, 0, 4, 1, 2]), (N, 1)))
    for a, b in zip(call(aa, masks_gpu(dirty), qg, 512), call(aa, masks_gpu(clean), qg, 512)):
        kit_gpu.assert_bits(a, b, "NaN and +inf in a query nobody asked for")
    dirty[0, 1, 5, 6], dirty[0, 1, 2, 9] = np.nan, np.inf
    x = masks_gpu(dirty)
    check(aa, call(aa, x, qg, 512), x, qg, 512)
    r = aa.resize_many_back(x, SIZES, "bilinear", regions=REGIONS, flips=FLIPS, reduce=None, out_dtype=F32)[0][1]
    assert r.isnan().any() and r.isposinf().any()


def test_launches_refusals_and_a_side_stream(aa):
    x, queries = inputs(37, "repeat", 100)
    qg = queries_gpu(queries)
    want = call(aa, x, qg, 512)  # (code objects loaded)
    assert len(kit_gpu.count_launches(lambda: call(aa, x, qg, 512))) == LAUNCHES <= 4
    assert len(kit_gpu.count_launches(lambda: aa.resize_many_back_instances_rle(x[:1], qg[:1], SIZES[:1], regions=REGIONS[:1], max_runs=512))) == LAUNCHES
    for bad in (0, (1 << 20) + 1, 2.0, None):
        with pytest.raises(ValueError, match="max_runs must be an int in 1 .. 1048576"):
            call(aa, x, qg, bad)
    with pytest.raises(NotImplementedError, match=r"torch\.no_grad\(\).*\.detach\(\)"):
        call(aa, [t.clone().requires_grad_() for t in x], qg, 512)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = call(aa, x, qg, 512)
    side.synchronize()
    for g, w in zip(got, want):
        kit_gpu.assert_bits(g, w, "side stream")


@pytest.mark.parametrize("channels_last,max_runs", ((False, 3), (True, 4096)), ids=("planar_3", "channels_last_4096"))
def test_the_outputs_are_written_completely_and_nothing_beside_them(aa, monkeypatch, channels_last, max_runs):
    """M = 5: runs and nruns end off a 16-byte boundary, so the arena has gaps.  Asked, repeated and empty slots' rows are all written."""
    x, queries = inputs(8, "empties", 5, channels_last)
    qg = queries_gpu(queries)
    want = call(aa, x, qg, max_runs)
    for fill in (0xFF, 0x00):
        got, gap_bytes, touched = run_guarded(monkeypatch, 0, fill, lambda: list(call(aa, x, qg, max_runs)), f"instances rle {max_runs}")
        for i, (g, w) in enumerate(zip(got, want)):
            kit_gpu.assert_bits(g, w, f"fill {fill:#x} output {i}")
        assert gap_bytes > 0 and touched == 0
