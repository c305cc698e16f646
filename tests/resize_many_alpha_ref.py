"""Shared by the resize_many(alpha=True) tests: the fixture generator (tests/golden/make_golden_resize_many_alpha.py) and the fixture it made
with Pillow (tests/golden/resize_many_alpha.npz), loaded once; item inputs regenerated from their seeds, once each, and left unchanged.
Not a test module."""
import functools

import numpy as np

import kit_golden

gen = functools.partial(kit_golden.generator, "resize_many_alpha")
fixture = functools.partial(kit_golden.fixture, "resize_many_alpha")


@functools.lru_cache(maxsize=None)
def _expected_index():
    return {e[0]: i for i, e in enumerate(gen().entries())}


@functools.lru_cache(maxsize=None)
def item(name, i):
    """[C, H, W] uint8 input of item i of case `name` (read-only: shared between tests)."""
    return kit_golden.readonly(gen().item_input(gen().case(name), i))


def boxes(name):
    return [it[2] for it in gen().case(name)[5]]


def sizes(name):
    return [it[3] for it in gen().case(name)[5]]


def offsets(name):
    return [it[4] for it in gen().case(name)[5]]


def fill(name):
    return list(gen().case(name)[3])


def expected(key):
    """-> (input CRC-32, output CRC-32, sampled pixels [n, C]) of one fixture entry."""
    fx = fixture()
    i = _expected_index()[key]
    counts = fx["sample_counts"]
    off = int(counts[:i].sum())
    c = int(fx["channels"][i])
    return int(fx["crcs"][i, 0]), int(fx["crcs"][i, 1]), fx["samples"][off:off + int(counts[i])].reshape(-1, c)


def assert_matches_fixture(key, x_chw, got_hwc):
    """got_hwc [oH, oW, C] equals the expected canvas of fixture entry `key`: the input is the fixture's (CRC-32), the sampled pixels are
    Pillow's (they say where a mismatch lies) and the whole canvas has the fixture's CRC-32."""
    kit_golden.assert_sampled(key, gen(), *expected(key), x_chw, got_hwc)


def placed(name):
    """Whether the case is a placed call (sizes / offsets / fill go into it)."""
    return bool(gen().case(name)[7])


def kwargs(name):
    """boxes, and for a placed case sizes, offsets and fill, as the call takes them."""
    kw = {"boxes": boxes(name)}
    if placed(name):
        kw.update(sizes=sizes(name), offsets=offsets(name), fill=fill(name))
    return kw


@functools.lru_cache(maxsize=None)
def restated(name, f, i, alpha=True):
    """The expected [oH, oW, C] canvas of item i from the numpy restatement (read-only: shared between tests)."""
    y = gen().restated(gen().case(name), f, i, item(name, i), alpha)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def seam_item(c, h, w, seed):
    """[C, H, W] uint8 input of a seam case (make_golden_alpha.make_image), read-only."""
    return kit_golden.readonly(gen().make_image(h, w, c, seed).transpose(2, 0, 1))


# (C, layout class, H, W): one item resized to 2 x 20 bilinear; its hull crosses a staging chunk's seam of the horizontal pass
SEAMS = [(4, "interleaved", 3, 2100), (2, "interleaved", 3, 4200), (4, "planar", 2, 8300)]
SEAM_OUT = (2, 20)


@functools.lru_cache(maxsize=None)
def seam_restated(c, h, w, seed, alpha=True):
    """The expected [oH, oW, C] of a seam item, bilinear."""
    x = seam_item(c, h, w, seed)
    y = gen().resize_alpha_restated("linear", np.ascontiguousarray(x.transpose(1, 2, 0)), SEAM_OUT[0], SEAM_OUT[1], None, alpha)
    y.setflags(write=False)
    return y
