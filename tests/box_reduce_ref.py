"""Shared by the box / reduce tests: the numpy restatement (tests/golden/make_golden_box_reduce.py) and the fixture it made with Pillow
(tests/golden/box_reduce.npz), loaded once; inputs regenerated from their seeds, once per shape."""
import functools
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def gen():
    spec = importlib.util.spec_from_file_location("make_golden_box_reduce", os.path.join(ROOT, "tests", "golden", "make_golden_box_reduce.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "box_reduce.npz"), allow_pickle=False))


@functools.lru_cache(maxsize=None)
def batch(shape, seed, fill=None):
    """[N, C, H, W] uint8 input of a fixture case (read-only: shared between tests)."""
    x = np.ascontiguousarray(gen().make_batch(shape, seed, fill))
    x.setflags(write=False)
    return x


def assert_matches_fixture(key, x_nchw, got_nhwc):
    """got_nhwc [N, oH, oW, C] equals Pillow's output of fixture entry `key`: the input is the fixture's (CRC-32), the whole output has
    Pillow's CRC-32, and the sampled pixels are Pillow's (they say where a mismatch lies)."""
    g = gen()
    incrc, outcrc, samples = g.expected(fixture(), key)
    assert g.crc(x_nchw) == incrc, f"{key}: the regenerated input is not the fixture's"
    got = np.ascontiguousarray(got_nhwc)
    px = got.reshape(-1, got.shape[-1])
    idx = g.sample_pixels(len(px))
    assert px[idx].shape == samples.shape, f"{key}: output shape {got.shape}"
    bad = np.nonzero((px[idx] != samples).any(axis=1))[0]
    assert bad.size == 0, f"{key}: {bad.size} of {len(idx)} sampled pixels differ, first at flat pixel {idx[bad[0]]}: {px[idx[bad[0]]]} != {samples[bad[0]]}"
    assert g.crc(got) == outcrc, f"{key}: the sampled pixels match but the whole output's CRC-32 differs from Pillow's"
