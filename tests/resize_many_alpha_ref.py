"""Shared by the resize_many(alpha=True) tests: the fixture generator (tests/golden/make_golden_resize_many_alpha.py) and the fixture it made
with Pillow (tests/golden/resize_many_alpha.npz), loaded once; item inputs regenerated from their seeds, once each, and left unchanged.
Not a test module."""
import functools
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def gen():
    spec = importlib.util.spec_from_file_location("make_golden_resize_many_alpha",
                                                  os.path.join(ROOT, "tests", "golden", "make_golden_resize_many_alpha.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "resize_many_alpha.npz"), allow_pickle=False))


@functools.lru_cache(maxsize=None)
def _expected_index():
    return {e[0]: i for i, e in enumerate(gen().entries())}


@functools.lru_cache(maxsize=None)
def item(name, i):
    """[C, H, W] uint8 input of item i of case `name` (read-only: shared between tests)."""
    x = np.ascontiguousarray(gen().item_input(gen().case(name), i))
    x.setflags(write=False)
    return x


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
    g = gen()
    incrc, outcrc, samples = expected(key)
    assert g.crc(x_chw) == incrc, f"{key}: the regenerated input is not the fixture's"
    got = np.ascontiguousarray(got_hwc)
    px = got.reshape(-1, got.shape[-1])
    idx = g.sample_pixels(len(px))
    assert px[idx].shape == samples.shape, f"{key}: output shape {got.shape}"
    bad = np.nonzero((px[idx] != samples).any(axis=1))[0]
    assert bad.size == 0, f"{key}: {bad.size} of {len(idx)} sampled pixels differ, first at flat pixel {idx[bad[0]]}: {px[idx[bad[0]]]} != {samples[bad[0]]}"
    assert g.crc(got) == outcrc, f"{key}: the sampled pixels match but the whole canvas's CRC-32 differs from the fixture's"


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
    x = np.ascontiguousarray(gen().make_image(h, w, c, seed).transpose(2, 0, 1))
    x.setflags(write=False)
    return x


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
