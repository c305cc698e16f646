"""The guarded allocator of tests/guard_ref.py, tested on its own (no GPU): what it returns is what torch.empty returns, a one-element
overrun on either side is reported with its side and offset, an untouched run passes, and a body that was only partly written is seen by
both rules the GPU sweep uses (NaN for floats, two fills for uint8)."""
import itertools

import pytest
import torch

import guard_ref as G

DTYPES = [torch.uint8, torch.float16, torch.bfloat16, torch.float32, torch.float64]
SHAPES = [(2, 3, 5, 7), (1, 3, 4, 6), (2, 1, 5, 3), (1, 1, 1, 1), (3, 4, 1, 9), (2, 5, 6, 1)]
FORMATS = [torch.contiguous_format, torch.channels_last]


def _cpu(lead=0, fill=0xFF):
    return G.Recorder(lead, fill, devices=("cpu",))


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_guarded_empty_is_torch_empty(dtype, lead):
    rec = _cpu(lead)
    for shape, mf in itertools.product(SHAPES, FORMATS):
        want = torch.empty(shape, dtype=dtype, memory_format=mf)
        got = rec.proxy.empty(shape, dtype=dtype, device=torch.device("cpu"), memory_format=mf)
        tag = (shape, mf, dtype, lead)
        assert got.shape == want.shape and got.dtype == want.dtype and got.device == want.device, tag
        assert got.stride() == want.stride(), tag
        for f in FORMATS:
            assert got.is_contiguous(memory_format=f) == want.is_contiguous(memory_format=f), tag
        r = rec.records[-1]
        es = want.element_size()
        assert r.nbytes == want.numel() * es and r.off == G.GUARD + lead * es and r.base.numel() == 2 * G.GUARD + lead * es + r.nbytes, tag
        assert got.data_ptr() == r.base.data_ptr() + r.off, tag
        assert bool((r.base == 0xFF).all()), tag  # the whole base is filled: NaN in every float type
        if dtype != torch.uint8:
            assert bool(torch.isnan(got).all()), tag
    # positional sizes, as the shim writes them
    t = rec.proxy.empty(2, 3, dtype=dtype, device="cpu")
    assert tuple(t.shape) == (2, 3) and t.is_contiguous()
    assert len(rec.check()) == len(rec.records)


def test_flat_uint8_buffers_ignore_the_lead_and_other_allocations_pass_through():
    rec = _cpu(lead=1)
    ws = rec.proxy.empty(100, dtype=torch.uint8, device="cpu")
    assert rec.records[-1].flat and rec.records[-1].off == G.GUARD  # a workspace, descriptor or table: always at the guard's end
    out = rec.proxy.empty((1, 1, 10, 10), dtype=torch.uint8, device="cpu")
    assert not rec.records[-1].flat and rec.records[-1].off == G.GUARD + 1
    assert rec.outputs()[0].data_ptr() == out.data_ptr() and rec.record_of(out) is rec.records[1] and rec.record_of(ws) is rec.records[0]
    n = len(rec.records)
    assert rec.proxy.empty((0, 3, 4, 5), dtype=torch.float32, device="cpu").numel() == 0 and len(rec.records) == n  # empty: nothing to guard
    assert rec.proxy.empty(8, dtype=torch.uint8, device="meta").device.type == "meta" and len(rec.records) == n
    cuda_only = G.Recorder()  # the GPU sweep's recorder leaves CPU (and pinned) allocations alone
    t = cuda_only.proxy.empty(16, dtype=torch.uint8)
    assert t.device.type == "cpu" and t.numel() == 16 and not cuda_only.records
    # every other attribute is torch's own
    assert rec.proxy.float32 is torch.float32 and rec.proxy.Tensor is torch.Tensor and rec.proxy.cuda is torch.cuda


@pytest.mark.parametrize("fill", [0xFF, 0x00])
@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_one_element_before_and_after_the_body_is_reported(dtype, lead, fill):
    """The negative control: the check can fail, and says where."""
    es = torch.empty((), dtype=dtype).element_size()
    rec = _cpu(lead, fill)
    keep = rec.proxy.empty((2, 3, 4, 5), dtype=dtype, device="cpu", memory_format=torch.channels_last)
    body = rec.proxy.empty((1, 3, 4, 5), dtype=dtype, device="cpu")
    body.zero_() if fill else body.fill_(1)
    assert rec.check()[1].data_ptr() == body.data_ptr()  # writing the whole body, and nothing else, passes
    r = rec.records[1]
    elems = r.base[r.off - es:r.off + r.nbytes + es].view(dtype)  # the body with one element on each side, through the base
    poke = 0 if fill else 1

    elems[0] = poke
    with pytest.raises(G.GuardViolation) as e:
        rec.check()
    found = rec.violations()
    assert len(found) == 1 and found[0][0] is r and found[0][1] == "before", found
    assert -es <= found[0][2] <= found[0][3] <= -1, found  # (the bytes of that element that changed)
    assert "allocation #1" in str(e.value) and "before" in str(e.value) and str(list(r.shape)) in str(e.value)
    r.base[r.off - es:r.off] = fill

    elems[-1] = poke
    found = rec.violations()
    assert len(found) == 1 and found[0][0] is r and found[0][1] == "after", found
    assert 0 <= found[0][2] <= found[0][3] <= es - 1, found
    with pytest.raises(G.GuardViolation, match="after"):
        rec.check()
    r.base[r.off + r.nbytes:r.off + r.nbytes + es] = fill

    r.base[0] = poke  # the far ends of both guards are watched too
    r.base[-1] = poke
    found = rec.violations()
    assert [(f[1], f[2], f[3]) for f in found] == [("before", -r.off, -r.off), ("after", G.GUARD - 1, G.GUARD - 1)], found
    r.base[0] = fill
    r.base[-1] = fill
    assert not rec.violations() and keep is rec.records[0].body


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.float64], ids=lambda d: str(d).split(".")[-1])
def test_a_partly_written_float_body_holds_nan(dtype):
    rec = _cpu()
    y = rec.proxy.empty((1, 2, 3, 5), dtype=dtype, device="cpu")
    assert G.unwritten_float(y) == y.numel()
    y[:] = 1.5
    assert G.unwritten_float(y) == 0
    y = rec.proxy.empty((1, 2, 3, 5), dtype=dtype, device="cpu", memory_format=torch.channels_last)
    y[:, :, :, :4] = -2.0  # the last column of every row is never stored
    assert G.unwritten_float(y) == 6
    rec.check()


def test_a_partly_written_uint8_body_differs_between_the_two_fills():
    runs = []
    for fill in (0xFF, 0x00):
        rec = _cpu(lead=1, fill=fill)
        y = rec.proxy.empty((1, 3, 4, 6), dtype=torch.uint8, device="cpu", memory_format=torch.channels_last)
        y[:, :, :, :5] = torch.arange(5, dtype=torch.uint8) * 51  # (0 and 255 among the values written: a value equal to a fill is no miss)
        rec.check()
        runs.append(y)
    assert G.unwritten_u8(*runs) == 12
    runs[0][:, :, :, 5] = 7
    runs[1][:, :, :, 5] = 7
    assert G.unwritten_u8(*runs) == 0
