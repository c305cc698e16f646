"""Shared by the resize_many_to_patches tests: the fixture generator (tests/golden/make_golden_resize_many_patches.py) and the fixture it
made with Pillow (tests/golden/resize_many_patches.npz), loaded once; item inputs regenerated from their seeds and the expected token
matrices computed from the CPU restatement, once each, and left unchanged.  Nothing here calls the code under test.  Not a test module."""
import functools

import numpy as np

import kit_golden
from kit_golden import MEAN, MODE, STD  # noqa: F401

gen = functools.partial(kit_golden.generator, "resize_many_patches")
fixture = functools.partial(kit_golden.fixture, "resize_many_patches")


def case(name):
    return gen().case(name)


def names():
    return [cs[0] for cs in gen().CASES]


@functools.lru_cache(maxsize=None)
def item(name, i):
    """[C, H, W] uint8 input of item i of case `name` (read-only: shared between tests)."""
    return kit_golden.readonly(gen().item_input(case(name), i))


def inputs(name):
    return [item(name, i) for i in range(len(case(name)[4]))]


def boxes(name):
    return [it[2] for it in case(name)[4]]


def sizes(name):
    return [it[3] for it in case(name)[4]]


def flips(name):
    return [it[4] for it in case(name)[4]]


def token_counts(name):
    ph, pw = case(name)[2]
    return [(vh // ph) * (vw // pw) for vh, vw in sizes(name)]


@functools.lru_cache(maxsize=None)
def tokens(name, f, fmt):
    """The expected uint8 token matrix [sum T_i, D] of a case, filter and format from the CPU restatement and the numpy patchify of the
    generator (read-only: shared between tests)."""
    t = gen().restated(case(name), f, fmt, inputs(name))
    t.setflags(write=False)
    return t


def padded(tok, counts, pad_to):
    """[sum T_i, D] -> [N, pad_to, D]: item i's rows first, zeros after them."""
    out = np.zeros((len(counts), pad_to, tok.shape[1]), tok.dtype)
    at = 0
    for i, t in enumerate(counts):
        out[i, :t] = tok[at:at + t]
        at += t
    return out


def assert_matches_fixture(key, got):
    """got, a uint8 [sum T_i, D] matrix, equals the expected tokens of fixture entry `key`: the regenerated inputs are the fixture's
    (CRC-32), the sampled elements are Pillow's (they say where a mismatch lies) and the whole matrix has the fixture's CRC-32."""
    g = gen()
    name = key.split("/")[0]
    in_crcs, out_crc, samples = g.expected(fixture(), key)
    assert [g.crc(x) for x in inputs(name)] == [int(v) for v in in_crcs], f"{key}: the regenerated inputs are not the fixture's"
    got = np.ascontiguousarray(got)
    assert got.dtype == np.uint8 and got.ndim == 2, (key, got.dtype, got.shape)
    s = g.sample(got).ravel()
    assert s.shape == samples.shape, f"{key}: token matrix shape {got.shape}"
    bad = np.nonzero(s != samples)[0]
    assert bad.size == 0, f"{key}: {bad.size} of {s.size} sampled elements differ, first sample {bad[0]}: {s[bad[0]]} != {samples[bad[0]]}"
    assert g.crc(got) == out_crc, f"{key}: the sampled elements match but the whole matrix's CRC-32 differs from the fixture's"
