"""Image.reduce on the GPU (-m gpu): extension_interpolate.reduce equals Pillow's Image.reduce bit for bit (tests/golden/box_reduce.npz,
made by tests/golden/make_golden_box_reduce.py with Pillow) in both layouts, on partial edge blocks, boxes at odd byte offsets, strips
wider than a tile, many row bands, large blocks, views of larger tensors, and RGBA / LA."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import box_reduce_ref as ref  # noqa: E402
import kit_gpu  # noqa: E402

pytestmark = pytest.mark.gpu
G = ref.gen()
aa = kit_gpu.aa_fixture()
CASES = {cs[0]: cs for cs in G.REDUCE_CASES}


def _nhwc(y):
    return y.permute(0, 2, 3, 1).contiguous().cpu().numpy()


def _layouts(c):
    # the issue's list: C = 3 channels_last and planar, C = 1 (one layout), C = 4 and C = 2 channels_last; planar takes any C, so it runs too
    return (False,) if c == 1 else (True, False)


@pytest.mark.parametrize("name", list(CASES))
def test_reduce_equals_pillow(aa, name):
    _, shape, seed, fill, factor, box, alpha = CASES[name]
    x = ref.batch(shape, seed, fill)
    for cl in _layouts(shape[1]):
        y = aa.reduce(kit_gpu.nchw_gpu(x, cl), factor, box, alpha=alpha)
        assert y.dtype == torch.uint8 and y.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
        ref.assert_matches_fixture(name, x, _nhwc(y))


def test_constant_images_stay_constant(aa):
    for fill in (255, 0):
        y = aa.reduce(kit_gpu.nchw_gpu(ref.batch((1, 3, 37, 53), 0, fill), True), (7, 9))
        assert tuple(y.shape) == (1, 3, 5, 8) and bool((y == fill).all())


@pytest.mark.parametrize("channels_last", [True, False])
def test_views_are_read_where_they_lie(aa, channels_last):
    """A crop and a batch slice of a larger tensor give what their dense copies give (and the crop what the box of the whole gives)."""
    rng = np.random.default_rng(3)
    big = kit_gpu.nchw_gpu(rng.integers(0, 256, (4, 3, 61, 83), dtype=np.uint8), channels_last)
    mf = torch.channels_last if channels_last else torch.contiguous_format
    crop = big[:, :, 7:44, 5:58]  # (odd byte offsets in both layouts)
    assert not crop.is_contiguous(memory_format=mf)
    for factor in ((2, 2), (8, 4), (3, 5)):
        want = aa.reduce(crop.contiguous(memory_format=mf), factor)
        assert torch.equal(aa.reduce(crop, factor), want)
        assert torch.equal(aa.reduce(big, factor, (5, 7, 58, 44)), want)
        sl = big[1:3]
        assert torch.equal(aa.reduce(sl, factor), aa.reduce(sl.clone(memory_format=mf), factor))
        every_other = big[::2]
        assert torch.equal(aa.reduce(every_other, factor), aa.reduce(every_other.contiguous(memory_format=mf), factor))
    # the dense copy itself is checked against the restatement
    got = _nhwc(aa.reduce(crop, (3, 5)))
    want = np.stack([G.reduce_restated(img, (3, 5)) for img in _nhwc(crop)])
    assert np.array_equal(got, want)


def test_factor_one_with_a_full_box_is_a_copy(aa):
    x = ref.batch((2, 3, 37, 53), 13)
    for cl in (True, False):
        t = kit_gpu.nchw_gpu(x, cl)
        y = aa.reduce(t, 1)
        assert torch.equal(y, t) and y.data_ptr() != t.data_ptr()
        assert torch.equal(aa.reduce(t, (1, 1), (5, 7, 50, 36)), t[:, :, 7:36, 5:50])


def test_blocks_wider_than_a_tile(aa):
    """fx * C beyond the 4096 bytes a tile holds per row: the run-time form walks the row in chunks."""
    rng = np.random.default_rng(4)
    x = rng.integers(0, 256, (1, 3, 5, 3001), dtype=np.uint8)
    for cl in (True, False):
        got = _nhwc(aa.reduce(kit_gpu.nchw_gpu(x, cl), (1400, 2)))
        want = np.stack([G.reduce_restated(img, (1400, 2)) for img in x.transpose(0, 2, 3, 1)])
        assert np.array_equal(got, want)


def test_reduce_torch_op(aa):
    x = kit_gpu.nchw_gpu(ref.batch((2, 3, 37, 53), 13), True)
    assert torch.equal(torch.ops.extension_interpolate.reduce(x, [8, 4], [5, 7, 50, 36]), aa.reduce(x, (8, 4), (5, 7, 50, 36)))
