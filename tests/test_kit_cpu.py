"""The test kit itself (tests/kit_golden.py, tests/kit_gpu.py): the comparisons refuse what they are there to refuse.  No GPU and no built
library: tensors on the CPU, a made-up fixture entry."""
import numpy as np
import pytest
import torch

import kit_golden
import kit_gpu


# ---- assert_bits -----------------------------------------------------------------------------------------------------------------------
def _from_bits(words, dtype):
    return torch.tensor(words, dtype=torch.int32).view(dtype)


def test_assert_bits_fails_on_a_single_bit():
    a = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    b = a.clone()
    b.view(torch.int32)[1, 2] ^= 1
    with pytest.raises(AssertionError, match=r"1 of 12 elements differ from the reference, first at \[1, 2\]"):
        kit_gpu.assert_bits(a, b, "one bit")
    kit_gpu.assert_bits(a, a.clone(), "equal")


def test_assert_bits_tells_the_zeros_apart():
    assert torch.equal(torch.tensor([0.0]), torch.tensor([-0.0]))  # (what a comparison by value would have accepted)
    with pytest.raises(AssertionError, match="1 of 1 elements differ"):
        kit_gpu.assert_bits(torch.tensor([0.0]), torch.tensor([-0.0]), "zeros")


def test_assert_bits_tells_nan_payloads_apart():
    a, b = _from_bits([0x7FC00000, 0x3F800000], torch.float32), _from_bits([0x7FC00001, 0x3F800000], torch.float32)
    assert bool(torch.isnan(a[0])) and bool(torch.isnan(b[0]))
    with pytest.raises(AssertionError, match=r"1 of 2 elements differ from the reference, first at \[0\]"):
        kit_gpu.assert_bits(a, b, "payloads")
    kit_gpu.assert_bits(a, a.clone(), "the same NaN")


def test_assert_bits_fails_on_dtype_and_on_shape():
    a = torch.zeros(2, 3, dtype=torch.float16)
    with pytest.raises(AssertionError):
        kit_gpu.assert_bits(a, torch.zeros(2, 3, dtype=torch.bfloat16), "dtype")  # (the same bits, another type)
    with pytest.raises(AssertionError):
        kit_gpu.assert_bits(a, torch.zeros(3, 2, dtype=torch.float16), "shape")
    with pytest.raises(AssertionError):
        kit_gpu.assert_bits(a, torch.zeros(2, 3, 1, dtype=torch.float16), "rank")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.uint16, torch.float16, torch.float64, torch.uint8])
def test_assert_bits_passes_on_equal_tensors_of_every_width(dtype):
    words = torch.arange(-300, 300, dtype=torch.int64).reshape(2, 300)
    a = words.to(torch.int16).view(dtype) if dtype in (torch.bfloat16, torch.uint16, torch.float16) else words.to(dtype)
    kit_gpu.assert_bits(a, a.clone(), dtype)
    kit_gpu.assert_bits(a.t(), a.t().contiguous(), (dtype, "a view that is not contiguous"))
    assert kit_gpu.bits(a).dtype == {1: torch.uint8, 2: torch.int16, 8: torch.int64}[a.element_size()]
    b = a.clone()
    b.view(torch.uint8)[-1, -1] ^= 0x80
    with pytest.raises(AssertionError, match="1 of 600 elements differ"):
        kit_gpu.assert_bits(a, b, dtype)


def test_assert_bits_hands_the_first_index_to_explain():
    a = torch.zeros(2, 3, 4, 5)
    b = a.clone()
    b[1, 2, 0, 3] = 1.0
    b[1, 2, 3, 4] = 2.0
    with pytest.raises(AssertionError, match=r"2 of 120 elements differ.*first at \[1, 2, 0, 3\].*; column 3 of item 1"):
        kit_gpu.assert_bits(a, b, "explained", explain=lambda at: f"column {at[3]} of item {at[0]}")


# ---- assert_sampled --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def entry():
    """A made-up fixture entry of a 40 x 50 x 3 output (2000 pixels, 256 of them sampled): (g, in_crc, out_crc, samples, x, out)."""
    g = kit_golden.generator("box_reduce")
    rng = np.random.default_rng(5)
    x = kit_golden.readonly(rng.integers(0, 256, (3, 80, 100), dtype=np.uint8))
    out = kit_golden.readonly(rng.integers(0, 256, (40, 50, 3), dtype=np.uint8))
    idx = g.sample_pixels(2000)
    assert 0 < len(idx) < 2000
    return g, g.crc(x), g.crc(out), out.reshape(-1, 3)[idx].copy(), x, out


def test_assert_sampled_passes_on_the_entry_itself(entry):
    g, in_crc, out_crc, samples, x, out = entry
    kit_golden.assert_sampled("k", g, in_crc, out_crc, samples, x, out)
    kit_golden.assert_sampled("k", g, in_crc, out_crc, samples, x, np.asfortranarray(out))  # (any memory order of the same pixels)


def test_assert_sampled_fails_on_a_wrong_input_crc(entry):
    g, in_crc, out_crc, samples, x, out = entry
    other = x.copy()
    other[2, 79, 99] ^= 1
    with pytest.raises(AssertionError, match="the regenerated input is not the fixture's"):
        kit_golden.assert_sampled("k", g, in_crc, out_crc, samples, other, out)


def test_assert_sampled_fails_on_one_changed_sampled_pixel(entry):
    g, in_crc, out_crc, samples, x, out = entry
    px = int(g.sample_pixels(2000)[100])
    got = out.copy()
    got.reshape(-1, 3)[px, 1] ^= 1
    with pytest.raises(AssertionError, match=f"1 of 256 sampled pixels differ, first at flat pixel {px}:"):
        kit_golden.assert_sampled("k", g, in_crc, out_crc, samples, x, got)


def test_assert_sampled_fails_on_a_change_outside_the_samples(entry):
    g, in_crc, out_crc, samples, x, out = entry
    outside = np.setdiff1d(np.arange(2000), g.sample_pixels(2000))
    got = out.copy()
    got.reshape(-1, 3)[int(outside[700]), 2] ^= 0x40
    with pytest.raises(AssertionError, match="the sampled pixels match but the whole output's CRC-32 differs"):
        kit_golden.assert_sampled("k", g, in_crc, out_crc, samples, x, got)


def test_assert_sampled_fails_on_another_shape(entry):
    g, in_crc, out_crc, samples, x, out = entry
    with pytest.raises(AssertionError, match="output shape"):
        kit_golden.assert_sampled("k", g, in_crc, out_crc, samples, x, out[:, :, :2])


# ---- the loaders and the shared inputs -------------------------------------------------------------------------------------------------
def test_generator_and_fixture_are_loaded_once():
    g = kit_golden.generator("box_reduce")
    assert kit_golden.generator("box_reduce") is g and g.__name__ == "make_golden_box_reduce"
    assert kit_golden.generator("resize_many") is not g
    fx = kit_golden.fixture("box_reduce")
    assert kit_golden.fixture("box_reduce") is fx and isinstance(fx, dict) and all(isinstance(v, np.ndarray) for v in fx.values())


def test_readonly_refuses_a_write():
    x = kit_golden.readonly(np.arange(24).reshape(2, 3, 4).transpose(2, 0, 1))
    assert x.flags.c_contiguous and not x.flags.writeable
    with pytest.raises(ValueError):
        x[0, 0, 0] = 1


# ---- stopping after a GPU error ----------------------------------------------------------------------------------------------------------
def test_only_a_gpu_error_ends_the_session():
    """The three kinds of RuntimeError, raised here in Python: none of them touches a GPU."""
    from interpolate_antialiasing_amd import _lib

    for text in ("HIP error: invalid configuration argument", "an illegal memory access was encountered"):
        with pytest.raises(pytest.exit.Exception) as info:
            with kit_gpu.gpu_error_ends_the_session("a test of the kit"):
                raise RuntimeError(text)
        assert info.value.returncode == 3 and "a test of the kit" in str(info.value) and "nothing more is launched" in str(info.value)
    with pytest.raises(_lib.AAInterpError):  # the package's own refusal, whatever it says
        with kit_gpu.gpu_error_ends_the_session("a test of the kit"):
            raise _lib.AAInterpError("HIP error in the message of a refusal")
    with pytest.raises(RuntimeError, match="something else"):
        with kit_gpu.gpu_error_ends_the_session("a test of the kit"):
            raise RuntimeError("something else")
    with kit_gpu.gpu_error_ends_the_session("a test of the kit"):
        pass
