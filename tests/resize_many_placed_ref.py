"""Shared by the placed resize_many tests: the fixture generator (tests/golden/make_golden_resize_many_placed.py) and the fixture it made
with Pillow (tests/golden/resize_many_placed.npz), loaded once; item inputs regenerated from their seeds, once each, and left unchanged.
Not a test module."""
import functools

import kit_golden

gen = functools.partial(kit_golden.generator, "resize_many_placed")
fixture = functools.partial(kit_golden.fixture, "resize_many_placed")


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
