"""The activation kernels of resize_many_back and resize_many_back_merged under the guarded allocator (guard_ref), as
test_resize_many_back_merged_guard_gpu.py holds the kernels without an activation: every element of every output is written, no byte
outside a body is touched, and neither are the 16-byte alignment gaps between the outputs of the arena.  Both calls, both activations,
all three reductions, on the merged call's base case (for resize_many_back every item at its group's size)."""
import numpy as np
import pytest
import torch

import guard_ref as G
import kit_gpu
import resize_many_back_merged_ref as ref

pytestmark = pytest.mark.gpu

aa = kit_gpu.aa_fixture()

ACTIVATIONS = ("softmax", "sigmoid")
# reduce, out_dtype: the outputs' byte counts are no multiples of 16 for the one- and two-byte elements, so that there are gaps
CASES = [(None, torch.float32), (None, torch.bfloat16), ("argmax", torch.uint8), ("argmax", torch.int16), ("argmax", torch.int64),
         ("greater", torch.bool), ("greater", torch.uint8)]
ITEM_SIZES = [ref.BASE_SIZES[g] for g in ref.BASE_GROUPS]


def run_guarded(monkeypatch, lead, fill, call, tag):
    """-> (the outputs, on the CPU; the gaps' bytes; those that differ from the fill).  Checks the guard bands and the allocations."""
    with G.guarded(monkeypatch, lead, fill) as rec:
        try:
            with kit_gpu.gpu_error_ends_the_session(f"{tag}, lead {lead}"):
                outs = call()
                rec.check()
        except G.GuardViolation as e:
            raise AssertionError(f"{tag}, lead {lead}: {e}") from None
    r = rec.record_of(outs[0])
    assert r is not None, f"{tag}: the arena is not a guarded allocation"
    others = [q for q in rec.records if q is not r]
    assert len(others) == 2 and all(q.flat for q in others), f"{tag}: a descriptor and a workspace besides the arena, got {rec.records}"
    if not r.flat:
        assert outs[0].data_ptr() % 256 == (G.GUARD + lead * outs[0].element_size()) % 256
    # the gaps: bytes of the arena's body that belong to no output
    body = r.base[r.off:r.off + r.nbytes]
    covered = torch.zeros(r.nbytes, dtype=torch.bool, device=body.device)
    start = outs[0].data_ptr()
    for o in outs:
        a = o.data_ptr() - start
        assert a % 16 == 0 and 0 <= a and a + o.numel() * o.element_size() <= r.nbytes
        covered[a:a + o.numel() * o.element_size()] = True
    gaps = body[~covered]
    return [o.cpu() for o in outs], int(gaps.numel()), int((gaps != fill).sum())


def check(monkeypatch, lead, call, tag, n, dtype):
    with kit_gpu.gpu_error_ends_the_session(tag):
        want = call()
    assert len(want) == n
    for fill in (0xFF, 0x00):
        got, gap_bytes, touched = run_guarded(monkeypatch, lead, fill, call, tag)
        # the same bits into 0xFF-filled and into 0x00-filled memory: an element that was never written would show its fill in one
        for g, (a, b) in enumerate(zip(got, want)):
            kit_gpu.assert_bits(a, b, f"{tag} lead {lead} fill {fill:#x} output {g}")
        assert touched == 0, f"{tag}, lead {lead}: {touched} of {gap_bytes} gap bytes between the arena's outputs were written"
    if dtype in (torch.uint8, torch.bool, torch.int16, torch.bfloat16):
        assert gap_bytes > 0, f"{tag}: the case has no gaps to look at"


def canvas(channels_last):
    x = torch.from_numpy(np.array(ref.BASE_CANVAS)).cuda()
    return x.contiguous(memory_format=torch.channels_last) if channels_last else x


@pytest.mark.parametrize("channels_last", (False, True), ids=("planar", "channels_last"))
@pytest.mark.parametrize("lead", (0, 1))
@pytest.mark.parametrize("activation", ACTIVATIONS)
def test_every_item_is_written_and_nothing_else(aa, monkeypatch, activation, lead, channels_last):
    x = canvas(channels_last)
    for reduce, dtype in CASES:
        kw = dict(regions=ref.BASE_REGIONS, flips=ref.BASE_FLIPS, reduce=reduce, out_dtype=dtype, threshold=0.5, activation=activation)
        check(monkeypatch, lead, lambda: aa.resize_many_back(x, ITEM_SIZES, "bicubic", **kw),
              f"resize_many_back {activation} reduce={reduce} {dtype} cl={channels_last}", 7, dtype)


@pytest.mark.parametrize("channels_last", (False, True), ids=("planar", "channels_last"))
@pytest.mark.parametrize("lead", (0, 1))
@pytest.mark.parametrize("activation", ACTIVATIONS)
def test_every_group_is_written_and_nothing_else(aa, monkeypatch, activation, lead, channels_last):
    x = canvas(channels_last)
    for merge in ("sum", "mean"):
        for reduce, dtype in CASES:
            kw = dict(regions=ref.BASE_REGIONS, flips=ref.BASE_FLIPS, merge=merge, reduce=reduce, out_dtype=dtype, threshold=0.5,
                      activation=activation)
            check(monkeypatch, lead, lambda: aa.resize_many_back_merged(x, ref.BASE_GROUPS, ref.BASE_SIZES, "bicubic", **kw),
                  f"resize_many_back_merged {activation} merge={merge} reduce={reduce} {dtype} cl={channels_last}", 3, dtype)
