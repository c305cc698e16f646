"""resize_many_back_backward under the guarded allocator (guard_ref): the output, the workspace and the descriptor come from torch.empty
in extension_interpolate.py.  The one gather kernel writes every element of every item — outside the regions the bits of +0.0, whatever
the memory held — no byte outside a body is touched, and neither are the alignment gaps between the items of an arena.  lead=1 puts the
output on an element-only boundary."""
import pytest
import torch

import guard_ref as G
import kit_gpu
import resize_many_back_bwd_ref as ref

pytestmark = pytest.mark.gpu

aa = kit_gpu.aa_fixture()

# canvases whose byte counts are no multiples of 16 in 16 bits, so that an arena has gaps
CANVASES = [(12, 16), (5, 3), (7, 9), (3, 3), (6, 7)]
REGIONS = [(0, 0, 12, 16), (1, 0, 3, 2), (3, 0, 1, 1), (0, 1, 3, 1), (1, 0, 5, 7)]
K = 3


def run_guarded(monkeypatch, lead, fill, call, tag):
    """-> (the result on the CPU: a tensor or a list; the gaps' byte count; how many of them differ from the fill).  Checks the guard
    bands and the allocations."""
    with G.guarded(monkeypatch, lead, fill) as rec:
        try:
            with kit_gpu.gpu_error_ends_the_session(f"{tag}, lead {lead}"):
                out = call()
                rec.check()
        except G.GuardViolation as e:
            raise AssertionError(f"{tag}, lead {lead}: {e}") from None
    outs = out if isinstance(out, list) else [out]
    r = rec.record_of(outs[0])
    assert r is not None, f"{tag}: the output is not a guarded allocation"
    others = [q for q in rec.records if q is not r]
    assert len(others) == 2 and all(q.flat for q in others), f"{tag}: a descriptor and a workspace besides the output, got {rec.records}"
    assert not r.flat and outs[0].data_ptr() % 256 == (G.GUARD + lead * outs[0].element_size()) % 256
    body = r.base[r.off:r.off + r.nbytes]
    covered = torch.zeros(r.nbytes, dtype=torch.bool, device=body.device)
    start = outs[0].data_ptr()
    for o in outs:
        a = o.data_ptr() - start
        assert (a % 16 == 0 or not isinstance(out, list)) and 0 <= a and a + o.numel() * o.element_size() <= r.nbytes
        covered[a:a + o.numel() * o.element_size()] = True
    gaps = body[~covered]
    cpu = [o.cpu() for o in outs]
    return (cpu if isinstance(out, list) else cpu[0]), int(gaps.numel()), int((gaps != fill).sum())


@pytest.mark.parametrize("out_format", ("nchw", "nhwc"))
@pytest.mark.parametrize("lead", (0, 1))
def test_every_element_is_written_and_nothing_else(aa, monkeypatch, lead, out_format):
    for dtype in (torch.float32, torch.bfloat16):
        gs = [torch.from_numpy(g.copy()).cuda().to(dtype) for g in ref.grads(ref.BASE_SIZES, K, seed=8)]
        gs[3] = None
        flips = ref.BASE_FLIPS
        cases = {"batch": (ref.BASE_HW, ref.BASE_REGIONS), "list": (CANVASES, REGIONS)}
        for name, (canvas, regions) in cases.items():
            kw = dict(regions=regions, flips=flips, out_format=out_format)
            tag = f"{name} {dtype} {out_format}"
            want = aa.resize_many_back_backward(gs, canvas, "bicubic", **kw)
            want = want if isinstance(want, list) else list(want)
            for fill in (0xFF, 0x00):
                got, gap_bytes, touched = run_guarded(monkeypatch, lead, fill, lambda: aa.resize_many_back_backward(gs, canvas, "bicubic", **kw), tag)
                got = got if isinstance(got, list) else list(got)
                # the same bits into 0xFF-filled (NaN) and into 0x00-filled memory: an element never written would show its fill in one
                for i, (g, w) in enumerate(zip(got, want)):
                    kit_gpu.assert_bits(g, w.cpu(), f"{tag} lead {lead} fill {fill:#x} item {i}")
                    assert G.unwritten_float(g) == 0
                assert touched == 0, f"{tag}, lead {lead}: {touched} of {gap_bytes} gap bytes between the arena's items were written"
            # outside the regions, and in the item without a gradient: the bits of +0.0
            cv = ref.canvases_of(canvas, 5)
            for i, (w, (y0, x0, h, ww)) in enumerate(zip(want, regions)):
                outside = torch.ones(cv[i], dtype=torch.bool)
                if gs[i] is not None:
                    outside[y0:y0 + h, x0:x0 + ww] = False
                assert not kit_gpu.bits(w)[:, outside].any(), (tag, i)
            if name == "list" and dtype == torch.bfloat16:
                assert gap_bytes > 0, f"{tag}: the case has no gaps to look at"
