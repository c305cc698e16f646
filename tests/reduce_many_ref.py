"""Shared by the reduce_many tests: the fixture generator (tests/golden/make_golden_reduce_many.py) and the fixture it made with Pillow
(tests/golden/reduce_many.npz), loaded once; item inputs regenerated from their seeds and the expected images computed from the CPU
restatement (which the generator asserted to be Pillow's on every entry), once each, and left unchanged.  Nothing here calls the code
under test.  Not a test module."""
import functools

import numpy as np

import kit_golden
from kit_golden import MODE  # noqa: F401

gen = functools.partial(kit_golden.generator, "reduce_many")
fixture = functools.partial(kit_golden.fixture, "reduce_many")


def case(name):
    return gen().case(name)


def names(plain_only=True):
    """The cases; plain_only: those whose items all go to the case's one output size."""
    return [cs[0] for cs in gen().CASES if not plain_only or cs[8] is None]


def case_filters():
    return [(cs[0], f) for cs in gen().CASES if cs[8] is None for f in cs[5]]


def count(name):
    return len(case(name)[4])


def shapes(name):
    return [it[:2] for it in case(name)[4]]


def boxes(name):
    return [it[2] for it in case(name)[4]]


@functools.lru_cache(maxsize=None)
def item(name, i):
    """[C, H, W] uint8 input of item i of case `name` (read-only: shared between tests)."""
    return kit_golden.readonly(gen().item_input(case(name), i))


@functools.lru_cache(maxsize=None)
def batch(name):
    """The one [N, C, H, W] tensor of a batch case."""
    x = np.stack([item(name, i) for i in range(count(name))])
    x.setflags(write=False)
    return x


def plan(name, f, i):
    """None, or (factor, reduce box, shifted box) as the fixture recorded them from Image.resize's own arithmetic."""
    return gen().recorded_plan(fixture(), f"{name}/{f}/{i}")


@functools.lru_cache(maxsize=None)
def resized(name, f, i):
    """Pillow's Image.resize(..., box=, reducing_gap=) of item i, [oh, ow, C]: the restatement, checked against the fixture's CRC-32 of
    Pillow's own output (read-only: shared between tests)."""
    g = gen()
    out, _ = g.restated(case(name), f, i, item(name, i))
    key = f"{name}/{f}/{i}"
    incrc, outcrc, _ = g.expected(fixture(), key)
    assert g.crc(item(name, i)) == incrc and g.crc(out) == outcrc, f"{key}: the restatement is not the fixture's Pillow output"
    return kit_golden.readonly(out)


def _assert_samples(key, what, got_hwc, outcrc, samples):
    g = gen()
    got = np.ascontiguousarray(got_hwc)
    px = got.reshape(-1, got.shape[-1])
    idx = g.sample_pixels(len(px))
    assert px[idx].shape == samples.shape, f"{key}: {what} shape {got.shape}"
    bad = np.nonzero((px[idx] != samples).any(axis=1))[0]
    assert bad.size == 0, f"{key}: {what}: {bad.size} of {len(idx)} sampled pixels differ, first at flat pixel {idx[bad[0]]}: {px[idx[bad[0]]]} != {samples[bad[0]]}"
    assert g.crc(got) == outcrc, f"{key}: {what}: the sampled pixels match but the whole array's CRC-32 differs from Pillow's"


def assert_resize_matches_fixture(key, x_chw, got_hwc):
    """got_hwc [oh, ow, C] equals Pillow's Image.resize(..., reducing_gap=) of fixture entry `key`."""
    incrc, outcrc, samples = gen().expected(fixture(), key)
    assert gen().crc(x_chw) == incrc, f"{key}: the regenerated input is not the fixture's"
    _assert_samples(key, "the gap resize", got_hwc, outcrc, samples)


def assert_reduce_matches_fixture(key, got_hwc):
    """got_hwc [rh, rw, C] equals Pillow's Image.reduce(factor, reduce box) of fixture entry `key` (a reduced item)."""
    outcrc, samples = gen().expected_reduce(fixture(), key)
    _assert_samples(key, "the reduce", got_hwc, outcrc, samples)


def paste(r_hwc, oh, ow, py, px, fill):
    """The item's [vh, vw, C] resize at (py, px) of a fill-coloured [oh, ow, C] canvas: the placed resize_many's definition."""
    vh, vw, c = r_hwc.shape
    canvas = np.empty((oh, ow, c), np.uint8)
    canvas[:] = np.array(fill, np.uint8)
    y0, y1, x0, x1 = max(0, py), min(oh, py + vh), max(0, px), min(ow, px + vw)
    if y1 > y0 and x1 > x0:
        canvas[y0:y1, x0:x1] = r_hwc[y0 - py:y1 - py, x0 - px:x1 - px]
    return canvas
