"""resize_many_maps on the GPU, everything by bits (integers with torch.equal, float32 viewed as int32): every fixture case against
Pillow and the numpy restatement, items read where they lie (odd element offsets, pitches that are no multiple of 4 bytes, a
non-contiguous item), the "I;16" overflow rule and the clamp, guard bands around the output and the workspace, a batch tensor against the
list of its items, the torch op, and the launch count."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import guard_ref  # noqa: E402
import kit_gpu  # noqa: E402
import resize_many_maps_ref as ref  # noqa: E402

from interpolate_antialiasing_amd import extension_interpolate as aa  # noqa: E402
from interpolate_antialiasing_amd import tables  # noqa: E402

pytestmark = pytest.mark.gpu

G = ref.gen()
COMBOS = [(case, name, dt) for case, cs in G.CASES.items() for dt in cs["dtypes"] for name in cs["filters"]]
TORCH_DT = {"u16": torch.uint16, "i32": torch.int32, "f32": torch.float32}


def _assert_bits(y, exp_np, what):
    """y [N, 1, oH, oW] on the GPU against a numpy [N, oH, oW] batch."""
    assert y.is_contiguous(), what
    kit_gpu.assert_bits(y, torch.from_numpy(np.ascontiguousarray(exp_np))[:, None], what)


@functools.lru_cache(maxsize=None)
def _maps(case, dt):
    """The case's [1, H, W] maps on the GPU (shared between tests, never written)."""
    return tuple(torch.from_numpy(np.array(x))[None].cuda() for x in ref.inputs(case, dt))


def _call(case, name, dt, **kw):
    return aa.resize_many_maps(list(_maps(case, dt)), list(G.CASES[case]["canvas"]), name, **{**ref.call_args(case, dt), **kw})


# ---- every fixture case: Pillow's bits, and the restatement's ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case,name,dt", COMBOS)
def test_fixture_case(case, name, dt):
    """The ragged list under every filter and dtype (both passes, either one, neither), long Lanczos windows on either axis, outputs of
    65 and 129 columns, canvas rows of 300, placement with overhang on four sides, "center", an item off the canvas, fills, flips, the
    overflow cases and the rows built to show a fused multiply-add."""
    y = _call(case, name, dt)
    _assert_bits(y, ref.expected(case, name, dt), (case, name, dt, "fixture"))
    _assert_bits(y, ref.restate(case, name, dt), (case, name, dt, "restatement"))


# ---- "I;16" overflow ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["over", "over_t"])
def test_u16_overflow_pillow_and_clamp(case):
    pil, clamp = ref.expected(case, "bicubic", "u16"), ref.restate(case, "bicubic", "u16", overflow="clamp")
    assert int((pil != clamp).sum()) >= 20  # (the reference alone: the two rules differ on this image)
    _assert_bits(_call(case, "bicubic", "u16", overflow="pillow"), pil, (case, "pillow"))
    _assert_bits(_call(case, "bicubic", "u16", overflow="clamp"), clamp, (case, "clamp"))


@pytest.mark.parametrize("dt", ["i32", "f32"])
def test_overflow_is_ignored_for_the_other_dtypes(dt):
    _assert_bits(_call("wide65", "bicubic", dt, overflow="clamp"), ref.expected("wide65", "bicubic", dt), dt)


# ---- items read where they lie -------------------------------------------------------------------------------------------------------------
def _views(base_np):
    """(numpy view, torch view of the same elements on the GPU) pairs of one [1, 24, 37] base: rows that start on odd elements, a pitch of
    37 elements (74 bytes for uint16: no multiple of 4), and a column-strided item, which the call copies."""
    t = torch.from_numpy(base_np).cuda()
    return [(base_np[:, 1:, 3:], t[:, 1:, 3:]), (base_np[:, :, 1::1], t[:, :, 1::1]), (base_np[:, 2:20, :30], t[:, 2:20, :30]),
            (base_np[:, :, ::2], t[:, :, ::2]), (base_np[:, 5:6, 7:], t[:, 5:6, 7:])]


@pytest.mark.parametrize("dt", ["u16", "i32", "f32"])
@pytest.mark.parametrize("name", ["bicubic", "lanczos"])
def test_views_at_any_offset_and_pitch(dt, name):
    base = G.as_dtype(np.random.default_rng(77).integers(0, 65536, (1, 24, 37)).astype(np.uint16), dt)
    pairs = _views(base)
    assert not pairs[3][1].is_contiguous() and pairs[1][1].data_ptr() % 4 == (2 if dt == "u16" else 0)
    boxes = [None, (0.5, 1.25, 30.0, 20.5), None, (1, 2, 14, 19), None]
    sizes = [(15, 18), (15, 18), (18, 18), (17, 13), (9, 18)]  # both passes, both under a box, height kept, a copy, one row up-scaled
    offsets = [(0, 0), (-2, 1), (0, 0), (1, 3), (3, -4)]
    flips = [False, True, False, True, True]
    y = aa.resize_many_maps([p[1] for p in pairs], [15, 18], name, boxes=boxes, sizes=sizes, offsets=offsets, flips=flips, fill=9)
    want = ref.many([np.ascontiguousarray(p[0][0]) for p in pairs], (15, 18), name, boxes=boxes, sizes=sizes, offsets=offsets, flips=flips, fill=9)
    _assert_bits(y, want, (dt, name))


@pytest.mark.parametrize("dt,w", [("u16", 5400), ("i32", 2700), ("f32", 2700)])
def test_a_strip_longer_than_the_staging_buffer(dt, w):
    """64 output columns at a scale beyond 40 (uint16: beyond 80) read more of a row than the horizontal pass stages (8 KiB per wave):
    those workgroups read memory directly; the second item, 66 columns at the same scale, has a staged second strip beside it."""
    xs = [G.as_dtype(np.random.default_rng([31, i]).integers(0, 65536, (3, w)).astype(np.uint16), dt) for i in range(2)]
    sizes = [(3, 64), (2, 66)]
    y = aa.resize_many_maps([torch.from_numpy(x)[None].cuda() for x in xs], [3, 66], "bilinear", sizes=sizes, fill=1)
    _assert_bits(y, ref.many(xs, (3, 66), "bilinear", sizes=sizes, fill=1), (dt, w))


def test_a_batch_tensor_is_the_list_of_its_items():
    for dt in ("u16", "f32"):
        x = torch.stack([torch.from_numpy(G.as_dtype(np.random.default_rng([5, i]).integers(0, 65536, (1, 21, 33)).astype(np.uint16), dt)) for i in range(3)]).cuda()
        kw = dict(boxes=[None, (2.5, 1.0, 30.0, 20.0), (3, 1, 20, 13)], flips=[True, False, True])
        a = aa.resize_many_maps(x, [12, 17], "hamming", **kw)
        b = aa.resize_many_maps([x[i] for i in range(3)], [12, 17], "hamming", **kw)
        assert tuple(a.shape) == (3, 1, 12, 17) and torch.equal(kit_gpu.bits(a), kit_gpu.bits(b))
        _assert_bits(a, ref.many([x[i, 0].cpu().numpy() for i in range(3)], (12, 17), "hamming", **kw), dt)


def test_the_torch_op_runs_the_call():
    cs = G.CASES["placed"]
    kw = ref.call_args("placed", "f32")
    flat_boxes = [float(v) for i, b in enumerate(kw["boxes"]) for v in (b or (0, 0, cs["items"][i][1], cs["items"][i][0]))]
    y = torch.ops.extension_interpolate.resize_many_maps(
        list(_maps("placed", "f32")), list(cs["canvas"]), "bicubic", boxes=flat_boxes, flips=kw["flips"], sizes=[v for s in kw["sizes"] for v in s],
        offsets=[v for o in kw["offsets"] for v in o], fill=kw["fill"])
    _assert_bits(y, ref.expected("placed", "bicubic", "f32"), "op")


# ---- guard bands -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,name", [("placed", "bicubic"), ("ragged", "lanczos"), ("vwide", "bilinear")])
@pytest.mark.parametrize("dt", ["u16", "i32", "f32"])
def test_guard_bands(monkeypatch, case, name, dt):
    """The output sits in a larger poisoned buffer and the workspace is poisoned: every output element is written (two poisons give the
    same bits) and nothing outside any buffer is touched, also where the output starts one element off its natural alignment."""
    outs = []
    for lead, fill in ((0, 0xFF), (1, 0x00)):
        with guard_ref.guarded(monkeypatch, lead=lead, fill=fill) as rec:
            y = _call(case, name, dt)
            rec.check()
            assert rec.record_of(y) is not None
        outs.append(y)
        _assert_bits(y, ref.expected(case, name, dt), (case, name, dt, lead))
    assert torch.equal(kit_gpu.bits(outs[0]), kit_gpu.bits(outs[1]))


# ---- the call's promises ---------------------------------------------------------------------------------------------------------------------
def test_three_launches_whatever_n():
    maps = list(_maps("ragged", "u16"))
    kw = ref.call_args("ragged", "u16")
    calls = {1: lambda: aa.resize_many_maps(maps[:1], [20, 23], "bicubic", boxes=kw["boxes"][:1]),
             5: lambda: aa.resize_many_maps(maps, [20, 23], "bicubic", boxes=kw["boxes"])}
    for k, fn in calls.items():
        fn()  # (module load and allocator warm-up stay outside the count)
        names = kit_gpu.count_launches(fn)
        assert len(names) == 3, (k, names)
        assert [sum(1 for nm in names if part in nm) for part in ("maps_tables", "maps_hpass", "maps_vpass")] == [1, 1, 1], (k, names)


def test_no_cache_is_read_or_written_and_a_side_stream_is_served():
    before = (len(tables._cache), len(tables._box_cache), len(aa._plans))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        y = _call("center", "bilinear", "i32")
    s.synchronize()
    assert (len(tables._cache), len(tables._box_cache), len(aa._plans)) == before
    _assert_bits(y, ref.expected("center", "bilinear", "i32"), "side stream")
