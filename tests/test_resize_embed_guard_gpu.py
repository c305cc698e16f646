"""resize_embed_to_tokens and its backward under the guarded allocator (guard_ref): the output, the workspace and the descriptor come
from torch.empty in extension_interpolate.py; every element of the output is written, and no byte outside a body is touched.  lead=1
puts the output on an element-only boundary, where the kernels take their per-element path."""
import numpy as np
import pytest
import torch

import guard_ref as G
import kit_gpu
import resize_embed_ref as ref

pytestmark = pytest.mark.gpu

aa = kit_gpu.aa_fixture()

DTYPES = (torch.float32, torch.bfloat16)


def run_guarded(monkeypatch, lead, call, shape, dtype, tag):
    with G.guarded(monkeypatch, lead) as rec:
        try:
            with kit_gpu.gpu_error_ends_the_session(f"{tag}, lead {lead}"):
                y = call()
                rec.check()
        except G.GuardViolation as e:
            raise AssertionError(f"{tag}, lead {lead}: {e}") from None
    r = rec.record_of(y)
    assert r is not None and not r.flat and tuple(r.shape) == tuple(shape) and r.dtype == dtype, f"{tag}: the result is not a guarded output"
    assert y.data_ptr() % 256 == (G.GUARD + lead * y.element_size()) % 256
    flats = [q for q in rec.records if q.flat]
    assert len(flats) == 2, f"{tag}: a descriptor and a workspace, got {rec.records}"
    assert G.unwritten_float(y) == 0, f"{tag}, lead {lead}: {G.unwritten_float(y)} elements of the output were never written"
    return y


@pytest.mark.parametrize("d", (8, 5))
@pytest.mark.parametrize("lead", (0, 1))
def test_forward_writes_its_output_and_nothing_else(aa, monkeypatch, lead, d):
    h0, w0 = ref.BASE_SOURCE
    grids = ref.BASE_GRIDS
    rows = ref.offsets(grids)[-1]
    e = torch.from_numpy(np.array(ref.embed_values(h0, w0, d))).cuda()
    for dtype in DTYPES:
        want = aa.resize_embed_to_tokens(e, grids, out_dtype=dtype)
        got = run_guarded(monkeypatch, lead, lambda: aa.resize_embed_to_tokens(e, grids, out_dtype=dtype), (rows, d), dtype, f"forward D={d} {dtype}")
        kit_gpu.assert_bits(got, want, f"forward D={d} {dtype} lead {lead}")
        wantp = aa.resize_embed_to_tokens(e, grids, pad_to=50, out_dtype=dtype)
        gotp = run_guarded(monkeypatch, lead, lambda: aa.resize_embed_to_tokens(e, grids, pad_to=50, out_dtype=dtype), (len(grids), 50, d), dtype,
                           f"padded forward D={d} {dtype}")
        kit_gpu.assert_bits(gotp, wantp, f"padded forward D={d} {dtype} lead {lead}")


@pytest.mark.parametrize("d", (8, 5))
@pytest.mark.parametrize("lead", (0, 1))
def test_backward_writes_its_output_and_nothing_else(aa, monkeypatch, lead, d):
    h0, w0 = ref.BASE_SOURCE
    grids = ref.BASE_GRIDS
    g = torch.from_numpy(np.array(ref.grad_values(grids, d))).cuda().to(torch.bfloat16)
    for dtype in DTYPES:
        want = aa.resize_embed_to_tokens_backward(g, (h0, w0, d), grids, dtype=dtype)
        got = run_guarded(monkeypatch, lead, lambda: aa.resize_embed_to_tokens_backward(g, (h0, w0, d), grids, dtype=dtype), (h0, w0, d), dtype,
                          f"backward D={d} {dtype}")
        kit_gpu.assert_bits(got, want, f"backward D={d} {dtype} lead {lead}")
