"""Shared by the box / reduce tests: the numpy restatement (tests/golden/make_golden_box_reduce.py) and the fixture it made with Pillow
(tests/golden/box_reduce.npz), loaded once; inputs regenerated from their seeds, once per shape."""
import functools

import kit_golden

gen = functools.partial(kit_golden.generator, "box_reduce")
fixture = functools.partial(kit_golden.fixture, "box_reduce")


@functools.lru_cache(maxsize=None)
def batch(shape, seed, fill=None):
    """[N, C, H, W] uint8 input of a fixture case (read-only: shared between tests)."""
    return kit_golden.readonly(gen().make_batch(shape, seed, fill))


def assert_matches_fixture(key, x_nchw, got_nhwc):
    """got_nhwc [N, oH, oW, C] equals Pillow's output of fixture entry `key`: the input is the fixture's (CRC-32), the sampled pixels are
    Pillow's (they say where a mismatch lies) and the whole output has Pillow's CRC-32."""
    kit_golden.assert_sampled(key, gen(), *gen().expected(fixture(), key), x_nchw, got_nhwc)
