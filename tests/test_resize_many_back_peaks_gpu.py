"""resize_many_back_peaks on the GPU against resize_many_back_peaks_ref: peaks equal, values equal by their bits — every comparison is
equality — special values, the launches, the guard bands and boxmath.peak_points.  The geometry is the instance test's: 1o's base case
(a 300-column output across the 256-column tile and the wave seam at 64, 23 and 13 rows that are no multiples of 8, 16 or 32, a
one-pixel source whose (4, 300) output is 1200 exact ties) plus two items at (18, 300) and (33, 70), and a (1, 1) output: all border."""
import numpy as np
import pytest
import torch

import kit_gpu
import resize_many_back_peaks_ref as ref
import resize_many_back_ref as back_ref
from interpolate_antialiasing_amd import _lib
from kit_golden import MODE
from test_resize_many_back_guard_gpu import run_guarded

pytestmark = pytest.mark.gpu

aa = kit_gpu.aa_fixture()

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
REGIONS = back_ref.BASE_REGIONS + [(0, 0, 12, 16), (2, 1, 9, 13), (4, 4, 3, 5)]
SIZES = back_ref.BASE_SIZES + [(18, 300), (33, 70), (1, 1)]
FLIPS, N = [True, False, True, True, False, False, True, False], len(SIZES)
ITEMS = (0, 1, 2, 3, 4, 0, 1, 2)
# K, filter, channels_last, dtype: K below, at and above AA_BACK_UNROLL; channels_last with K = 4 and 8 takes the vector loads
CASES = [(1, "linear", False, F32), (3, "cubic", True, F16), (4, "box", True, F32), (5, "lanczos", False, BF16), (8, "linear", True, BF16),
         (17, "hamming", False, F32), (17, "cubic", True, F16)]


def pred_gpu(c, dtype=F32, channels_last=False):
    """The canvas [5, K, 12, 16] -> the call's eight items (views, read where they lie)."""
    x = kit_gpu.nchw_gpu(c, channels_last).to(dtype)
    return [x[i] for i in ITEMS]


def call(aa, x, filt="linear", sizes=SIZES, regions=REGIONS, flips=FLIPS):
    with kit_gpu.gpu_error_ends_the_session("resize_many_back_peaks"):
        return aa.resize_many_back_peaks(x, sizes, MODE[filt], regions=regions, flips=flips)


def reference(aa, x, filt="linear"):
    """ref.peaks of what the existing call gives the same items -> (xy [N, K, 2], values [N, K, 5]) numpy."""
    rs = aa.resize_many_back(x, SIZES, MODE[filt], regions=REGIONS, flips=FLIPS, reduce=None, out_dtype=F32)
    pairs = [ref.peaks(r.cpu().numpy()) for r in rs]
    return np.stack([p for p, _ in pairs]), np.stack([v for _, v in pairs])


def check(aa, x, filt="linear"):
    peaks, values = call(aa, x, filt)
    want_xy, want_values = reference(aa, x, filt)
    assert peaks.dtype == torch.int32 and (peaks.cpu().numpy() == want_xy).all(), np.argwhere(peaks.cpu().numpy() != want_xy)[:4]
    kit_gpu.assert_bits(values, torch.from_numpy(want_values), f"values {filt}")
    return peaks, values, want_xy, want_values


@pytest.mark.parametrize("k,filt,channels_last,dtype", CASES)
def test_peaks_and_values_equal_the_reference(aa, k, filt, channels_last, dtype):
    peaks, values, xy, want = check(aa, pred_gpu(ref.bump_canvas(k), dtype, channels_last), filt)
    assert (xy[2] == 0).all() and (xy[7] == 0).all()  # 1200 exact ties, flipped: flat index 0; the (1, 1) item
    if (k, channels_last) == (17, False):  # from the reference alone: the cases exercise what they are there for
        x, y = xy[..., 0], xy[..., 1]
        oh, ow = (np.array([s[j] for s in SIZES])[:, None] for j in (0, 1))
        last_tile = y >= (oh - 1) // _lib.BACK_PEAKS_ROWS * _lib.BACK_PEAKS_ROWS
        border = (x == 0) | (y == 0) | (x == ow - 1) | (y == oh - 1)
        assert (x >= 256).any() and ((x >= 64) & (x < 256)).any() and (last_tile & (oh % _lib.BACK_PEAKS_ROWS != 0) & (oh > _lib.BACK_PEAKS_ROWS)).any()
        assert border.any() and (~border).any()
    # boxmath.peak_points of the call's result: the same arithmetic on the reference's arrays
    boxes = [(3.0 * i, 2.0 * i, 3.0 * i + 40.0, 2.0 * i + 25.5) for i in range(N)]
    for kw in (dict(), dict(refine="quarter"), dict(refine="quarter", boxes=boxes)):
        got = aa.boxmath.peak_points(peaks, values, SIZES, **kw)
        assert got.is_cuda and torch.equal(got.cpu(), aa.boxmath.peak_points(torch.from_numpy(xy), torch.from_numpy(want), SIZES, **kw))


SPECIAL = ("zeros", "signed_zeros", "neg_inf", "inf_then_nan", "two_nans")


@pytest.mark.parametrize("what", SPECIAL)
def test_special_values(aa, what):
    """Channel 1 of every batch entry is the special plane, between two ordinary channels."""
    c = np.array(ref.bump_canvas(3))
    plane = c[:, 1]
    plane[:] = {"zeros": 0.0, "neg_inf": -np.inf}.get(what, 0.0)
    if what == "signed_zeros":
        plane[:, :, :8] = -0.0
    elif what == "inf_then_nan":
        plane[:, 2, 3], plane[:, 7, 9] = np.inf, np.nan
    elif what == "two_nans":
        plane[:, 3, 4], plane[:, 8, 11] = np.nan, np.nan
    peaks, values, xy, want = check(aa, pred_gpu(c))
    if what in ("zeros", "signed_zeros"):  # all equal under the key: flat index 0, flipped or not
        assert (xy[:, 1] == 0).all() and (want[:, 1, 0] == 0.0).all()
    if what == "signed_zeros":  # items 0 and 5 see both halves: unflipped the peak is the left half's -0.0, flipped the right half's +0.0
        assert np.signbit(want[5, 1, 0]) and not np.signbit(want[0, 1, 0])
    if what == "neg_inf":  # (a tap of weight 0 makes the resample of -inf a NaN; the one-pixel source has one tap of weight 1: 1200 times -inf)
        assert (xy[2, 1] == 0).all() and (want[2, 1] == -np.inf).all()
    if what in ("inf_then_nan", "two_nans"):
        assert np.isnan(want[[0, 5], 1, 0]).all()


def test_three_launches(aa):
    x = pred_gpu(ref.bump_canvas(17))
    call(aa, x)  # (code objects loaded)
    assert len(kit_gpu.count_launches(lambda: call(aa, x))) == 3
    one = lambda: call(aa, x[:1], sizes=SIZES[:1], regions=REGIONS[:1], flips=FLIPS[:1])
    one()
    assert len(kit_gpu.count_launches(one)) == 3


@pytest.mark.parametrize("lead,channels_last", ((0, True), (1, False)), ids=("aligned", "four_byte"))
def test_the_arena_is_written_completely_and_nothing_beside_it(aa, monkeypatch, lead, channels_last):
    """lead 1 puts the arena on a 4-byte-only boundary.  Seven items of K = 5: 280 bytes of peaks, 8 bytes of gap before the values."""
    x = pred_gpu(ref.bump_canvas(5), channels_last=channels_last)[:7]
    seven = lambda: list(call(aa, x, sizes=SIZES[:7], regions=REGIONS[:7], flips=FLIPS[:7]))
    want = seven()
    for fill in (0xFF, 0x00):
        got, gap_bytes, touched = run_guarded(monkeypatch, lead, fill, seven, "peaks")
        for g, w, what in zip(got, want, ("peaks", "values")):
            kit_gpu.assert_bits(g, w, f"fill {fill:#x} {what}")
        assert gap_bytes > 0 and touched == 0
