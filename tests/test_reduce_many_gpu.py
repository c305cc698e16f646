"""reduce_many and reduce_many_for_resize on the GPU: every fixture case, filter and layout class against Pillow's bytes (tolerance 0) —
Image.reduce per item, and Image.resize(reducing_gap=) through each of the three ragged calls — items read where they lie, equality
with the single-image calls, guard bands, and the calls' promises about launches, streams and devices."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import guard_ref  # noqa: E402
import kit_gpu  # noqa: E402
import reduce_many_ref as ref  # noqa: E402
import resize_many_patches_ref as pref  # noqa: E402
from kit_golden import MODE  # noqa: E402
from kit_gpu import FORWARD  # noqa: E402

from interpolate_antialiasing_amd import _lib, boxmath, tables  # noqa: E402
from interpolate_antialiasing_amd import extension_interpolate as aa  # noqa: E402

pytestmark = pytest.mark.gpu

G = ref.gen()
CLASSES = [(name, cls) for name in ref.names() for cls in (("planar",) if G.case(name)[1] == 1 else ("interleaved", "planar"))]


@functools.lru_cache(maxsize=None)
def _inputs(name, cls):
    """The case's images on the GPU (shared between tests, never written): a list, or one [N, C, H, W] tensor for a batch case."""
    cs = G.case(name)
    if cs[7]:
        x = torch.from_numpy(ref.batch(name)).cuda()
        return x.contiguous(memory_format=torch.channels_last) if cls == "interleaved" else x
    return [kit_gpu.to_gpu(ref.item(name, i), cls) for i in range(ref.count(name))]


def _plans(name, f):
    return [ref.plan(name, f, i) for i in range(ref.count(name))]


def _reduce_args(name, f, imgs):
    """The reduced items of a case and filter -> (their images, factors, reduce boxes, item numbers)."""
    idx = [i for i, p in enumerate(_plans(name, f)) if p is not None]
    return [imgs[i] for i in idx], [ref.plan(name, f, i)[0] for i in idx], [ref.plan(name, f, i)[1] for i in idx], idx


def _check_views(name, cls, c, outs):
    """Every view is dense in the call's class, starts on a 16-byte boundary and shares the one arena."""
    for o in outs:
        _, rh, rw = o.shape
        assert o.dtype == torch.uint8 and o.is_cuda and o.data_ptr() % 16 == 0
        if cls == "interleaved" and c > 1:
            assert o.stride() == (1, rw * c, c) or rw == 1 or rh == 1, (name, o.shape, o.stride())
        else:
            assert o.is_contiguous(), (name, o.shape, o.stride())
    assert len({o.untyped_storage().data_ptr() for o in outs}) == 1


# 1 ---- Image.reduce per item
@pytest.mark.parametrize("name,cls", CLASSES)
def test_reduce_many_equals_pillows_reduce_per_item(name, cls):
    cs = G.case(name)
    for f in cs[5]:
        imgs, factors, rboxes, idx = _reduce_args(name, f, _inputs(name, cls))
        assert idx, name
        outs = aa.reduce_many(imgs, factors, boxes=rboxes)
        assert len(outs) == len(idx)
        _check_views(name, cls, cs[1], outs)
        for o, i, fac, rb in zip(outs, idx, factors, rboxes):
            assert tuple(o.shape) == (cs[1],) + boxmath.reduced_size(rb, fac)[::-1]
            ref.assert_reduce_matches_fixture(f"{name}/{f}/{i}", kit_gpu.hwc(o))


def test_reduce_many_factor_forms_and_whole_images():
    imgs = _inputs("g_c2", "interleaved")
    whole = [np.ascontiguousarray(ref.item("g_c2", i).transpose(1, 2, 0)) for i in range(3)]
    for factors, per_item in ((3, [(3, 3)] * 3), ((2, 5), [(2, 5)] * 3), ([4, (1, 7), (64, 40)], [(4, 4), (1, 7), (64, 40)])):
        outs = aa.reduce_many(imgs, factors)
        for o, x, fac in zip(outs, whole, per_item):
            assert np.array_equal(kit_gpu.hwc(o), G.reduce_restated(x, fac)), (factors, fac)
    outs = aa.reduce_many(imgs, 1, boxes=[(3, 2, 40, 33), None, (0, 0, 1, 1)])  # factor 1 copies the box
    assert np.array_equal(kit_gpu.hwc(outs[0]), whole[0][2:33, 3:40]) and np.array_equal(kit_gpu.hwc(outs[1]), whole[1]) and tuple(outs[2].shape) == (2, 1, 1)
    assert aa.reduce_many([], 2) == [] and aa.reduce_many(_inputs("g_batchbox", "planar")[:0], 2) == []


# 2 ---- reduce_many_for_resize + resize_many
def _gap_resize(name, cls, f, call=aa.resize_many, **kw):
    cs = G.case(name)
    imgs = _inputs(name, cls)
    small, b2 = aa.reduce_many_for_resize(imgs, list(cs[2]), MODE[f], boxes=ref.boxes(name), sizes=cs[8], reducing_gap=cs[3])
    return imgs, small, b2, call(small, list(cs[2]), MODE[f], boxes=b2, **kw)


@pytest.mark.parametrize("name,cls", CLASSES)
def test_reduce_then_resize_many_equals_pillows_reducing_gap(name, cls):
    cs = G.case(name)
    for f in cs[5]:
        imgs, small, b2, y = _gap_resize(name, cls, f)
        assert tuple(y.shape) == (ref.count(name), cs[1]) + tuple(cs[2]) and y.dtype == torch.uint8
        got = y.cpu()
        for i, p in enumerate(_plans(name, f)):
            if p is None:  # not reduced: the very same tensor, its box unchanged
                assert (small[i] is imgs[i]) if isinstance(imgs, list) else torch.equal(small[i], imgs[i]), (name, f, i)
                assert (b2[i] if b2 is not None else None) == ref.boxes(name)[i]
            else:
                assert tuple(b2[i]) == p[2] and tuple(small[i].shape) == (cs[1],) + boxmath.reduced_size(p[1], p[0])[::-1]
            ref.assert_resize_matches_fixture(f"{name}/{f}/{i}", ref.item(name, i), got[i].permute(1, 2, 0).numpy())


def test_a_call_in_which_nothing_reduces_launches_nothing(monkeypatch):
    imgs = [_inputs("g_mixed", "interleaved")[i] for i in (1, 5, 6)]
    assert all(ref.plan("g_mixed", "cubic", i) is None for i in (1, 5, 6))
    calls = []
    L = _lib.load()
    real = L.aa_reduce_many_u8
    monkeypatch.setattr(L, "aa_reduce_many_u8", lambda *a: calls.append(a) or real(*a))
    with guard_ref.guarded(monkeypatch) as rec:
        small, b2 = aa.reduce_many_for_resize(imgs, [30, 45], "bicubic", reducing_gap=2.0)
        assert b2 is None and all(s is t for s, t in zip(small, imgs))
        assert rec.records == [] and calls == []  # no arena, no descriptor, no launch
        small, b2 = aa.reduce_many_for_resize(imgs + [_inputs("g_mixed", "interleaved")[0]], [30, 45], "bicubic", boxes=[None, None, (0, 0, 1, 1), None])
        assert len(calls) == 1 and [r.flat for r in rec.records] == [True, True]  # one launch: a descriptor and an arena
        assert b2[:3] == [None, None, (0, 0, 1, 1)] and tuple(b2[3]) == ref.plan("g_mixed", "cubic", 0)[2]
        rec.check()


def test_no_cache_is_read_or_written_and_nothing_synchronises(monkeypatch):
    before = (len(tables._cache), len(tables._box_cache), len(aa._plans))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: pytest.fail("the call synchronised"))
    small, b2 = aa.reduce_many_for_resize(_inputs("g_mixed", "interleaved"), [30, 45], "bicubic", boxes=ref.boxes("g_mixed"))
    monkeypatch.undo()
    assert (len(tables._cache), len(tables._box_cache), len(aa._plans)) == before
    y = aa.resize_many(small, [30, 45], "bicubic", boxes=b2)
    ref.assert_resize_matches_fixture("g_mixed/cubic/4", ref.item("g_mixed", 4), kit_gpu.hwc(y[4]))


# 3 ---- through resize_many_to_float
@pytest.mark.parametrize("f", ["linear", "lanczos"])
def test_through_resize_many_to_float_bf16_nchw_normalised_flipped(f):
    name = "g_mixed"
    mean, std = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
    flips = [True, True, False, True, False, False, True]  # reduced and unreduced items on both sides
    assert {(flips[i], ref.plan(name, f, i) is None) for i in range(7)} == {(True, True), (True, False), (False, True), (False, False)}
    _, _, _, y = _gap_resize(name, "interleaved", f, aa.resize_many_to_float, flips=flips, out_dtype=torch.bfloat16, out_format="nchw", mean=mean,
                             std=std)
    assert y.dtype == torch.bfloat16 and y.is_contiguous() and tuple(y.shape) == (7, 3, 30, 45)
    u = torch.from_numpy(np.stack([ref.resized(name, f, i) for i in range(7)])).permute(0, 3, 1, 2)  # Pillow's gap bytes, [N, C, oh, ow]
    want = ((u.float() - torch.tensor(mean).view(1, 3, 1, 1)) / torch.tensor(std).view(1, 3, 1, 1)).to(torch.bfloat16)
    for i in range(7):
        if flips[i]:
            want[i] = want[i].flip(-1)
    assert torch.equal(y.cpu().view(torch.int16), want.contiguous().view(torch.int16))


# 4 ---- through the placed resize_many
@pytest.mark.parametrize("cls", ["interleaved", "planar"])
@pytest.mark.parametrize("f", ["linear", "cubic"])
def test_through_the_placed_resize_many(f, cls):
    name = "g_fit"
    cs = G.case(name)
    sizes = boxmath.fit_sizes(ref.shapes(name), shorter=40)
    assert sizes == cs[8] and len({p[0] for p in _plans(name, f) if p is not None}) >= 2
    _, _, _, y = _gap_resize(name, cls, f, sizes=sizes, offsets="center", fill=114)
    got = y.cpu()
    for i, (vh, vw) in enumerate(sizes):
        want = ref.paste(ref.resized(name, f, i), 30, 45, boxmath.center_offset(vh, 30), boxmath.center_offset(vw, 45), [114] * 3)
        assert np.array_equal(got[i].permute(1, 2, 0).numpy(), want), (f, cls, i)


# 5 ---- through resize_many_to_patches
@pytest.mark.parametrize("fmt", ["cpp", "ppc"])
def test_through_resize_many_to_patches_packed_and_padded(fmt):
    name, f = "g_patch", "cubic"
    cs = G.case(name)
    sizes = boxmath.fit_patch_sizes(ref.shapes(name), G.PATCH, max_tokens=48)
    assert sizes == cs[8]
    imgs = _inputs(name, "interleaved")
    small, b2 = aa.reduce_many_for_resize(imgs, list(cs[2]), MODE[f], boxes=ref.boxes(name), sizes=sizes, reducing_gap=cs[3])
    assert sum(1 for s, t in zip(small, imgs) if s is not t) >= 3
    toks = [pref.gen().patchify(ref.resized(name, f, i), G.PATCH, fmt) for i in range(7)]
    counts = [len(t) for t in toks]
    assert max(counts) <= 48
    y = aa.resize_many_to_patches(small, G.PATCH, MODE[f], sizes=sizes, boxes=b2, patch_format=fmt)
    assert np.array_equal(y.cpu().numpy(), np.concatenate(toks).astype(np.float32))
    y = aa.resize_many_to_patches(small, G.PATCH, MODE[f], sizes=sizes, boxes=b2, patch_format=fmt, pad_to=48)
    assert np.array_equal(y.cpu().numpy(), pref.padded(np.concatenate(toks), counts, 48).astype(np.float32))


# 6 ---- the single-image calls
@pytest.mark.parametrize("cls", ["interleaved", "planar"])
@pytest.mark.parametrize("name", ["g_mixed", "g_batchbox", "g_wideblock"])
def test_each_item_equals_the_single_image_call(name, cls):
    cs = G.case(name)
    for f in cs[5]:
        imgs, small, b2, y = _gap_resize(name, cls, f)
        for i, p in enumerate(_plans(name, f)):
            one = FORWARD[f](imgs[i][None], list(cs[2]), box=ref.boxes(name)[i], reducing_gap=cs[3])
            assert torch.equal(y[i], one[0]), (name, f, i)
            if p is not None:
                assert torch.equal(small[i], aa.reduce(imgs[i][None], p[0], p[1])[0]), (name, f, i)


# 7 ---- items read where they lie
@pytest.mark.parametrize("cls", ["interleaved", "planar"])
@pytest.mark.parametrize("name", ["g_mixed", "g_c4", "g_seam"])
def test_crops_at_odd_offsets_and_pitches_are_read_in_place(name, cls, monkeypatch):
    cs = G.case(name)
    f = cs[5][0]
    crops = [kit_gpu.pitched_crop(ref.item(name, i), cls, i) for i in range(ref.count(name))]
    imgs, factors, rboxes, idx = _reduce_args(name, f, crops)
    monkeypatch.setattr(torch.Tensor, "contiguous", lambda *a, **k: pytest.fail("an item in the class was copied"))
    outs = aa.reduce_many(imgs, factors, boxes=rboxes)
    monkeypatch.undo()
    dense = aa.reduce_many(_reduce_args(name, f, _inputs(name, cls))[0], factors, boxes=rboxes)
    for o, d, i in zip(outs, dense, idx):
        assert o.stride() == d.stride() and torch.equal(o, d)
        ref.assert_reduce_matches_fixture(f"{name}/{f}/{i}", kit_gpu.hwc(o))


def test_a_mixed_list_copies_the_minority_and_an_item_in_neither_class():
    name, f = "g_c4", "cubic"
    inter, planar = _inputs(name, "interleaved"), _inputs(name, "planar")
    _, factors, rboxes, idx = _reduce_args(name, f, inter)
    assert idx == [0, 1]
    full = [ref.plan(name, f, i) for i in range(3)]
    factors, rboxes = factors + [(3, 2)], rboxes + [None]  # the third item too, by factors of the test's own
    want = [G.reduce_restated(np.ascontiguousarray(ref.item(name, i).transpose(1, 2, 0)), fac, rb) for i, (fac, rb) in enumerate(zip(factors, rboxes))]
    for items, cls in (([inter[0], planar[1], inter[2]], "interleaved"), ([planar[0], inter[1], planar[2]], "planar")):
        outs = aa.reduce_many(items, factors, boxes=rboxes)
        _check_views(name, cls, 4, outs)
        for o, w in zip(outs, want):
            assert np.array_equal(kit_gpu.hwc(o), w)
    wide = torch.zeros((4, 64, 80), dtype=torch.uint8, device="cuda")
    odd = wide[:, :, ::2]  # columns two bytes apart: neither class
    odd.copy_(planar[2])
    outs = aa.reduce_many([inter[0], inter[1], odd], factors, boxes=rboxes)
    _check_views(name, "interleaved", 4, outs)
    for o, w in zip(outs, want):
        assert np.array_equal(kit_gpu.hwc(o), w)
    assert full[2] is None


# 8 ---- guard bands
@pytest.mark.parametrize("name,cls", [("g_mixed", "interleaved"), ("g_mixed", "planar"), ("g_wideblock", "interleaved"), ("g_seam", "interleaved"),
                                      ("g_tall", "planar"), ("g_tiny37", "planar")])
def test_writes_every_byte_of_every_view_and_nothing_else(name, cls, monkeypatch):
    f = G.case(name)[5][0]
    imgs, factors, rboxes, idx = _reduce_args(name, f, _inputs(name, cls))
    runs = []
    for fill in (0xFF, 0x00):
        with guard_ref.guarded(monkeypatch, fill=fill) as rec:
            outs = aa.reduce_many(imgs, factors, boxes=rboxes)
            rec.check()  # nothing outside the descriptor and the arena
            assert [r.flat for r in rec.records] == [True, True]
            assert all(rec.records[1].body.data_ptr() <= o.data_ptr() < rec.records[1].body.data_ptr() + rec.records[1].nbytes for o in outs)
            runs.append([o.cpu() for o in outs])
    for a, b, i in zip(runs[0], runs[1], idx):
        assert guard_ref.unwritten_u8(a, b) == 0, (name, i)
        ref.assert_reduce_matches_fixture(f"{name}/{f}/{i}", a.permute(1, 2, 0).numpy())


# 9 ---- the torch op
def test_torch_op_equals_the_function():
    name, f = "g_mixed", "hamming"
    imgs, factors, rboxes, idx = _reduce_args(name, f, _inputs(name, "interleaved"))
    outs = torch.ops.extension_interpolate.reduce_many(imgs, [v for fac in factors for v in fac], [v for rb in rboxes for v in rb])
    want = aa.reduce_many(imgs, factors, boxes=rboxes)
    assert len(outs) == len(want) and all(o.stride() == w.stride() and torch.equal(o, w) for o, w in zip(outs, want))
    outs = torch.ops.extension_interpolate.reduce_many(imgs[:2], [3], None)
    want = aa.reduce_many(imgs[:2], 3)
    assert all(torch.equal(o, w) for o, w in zip(outs, want))
    outs = torch.ops.extension_interpolate.reduce_many(imgs[:3], [3, 5])
    assert all(torch.equal(o, w) for o, w in zip(outs, aa.reduce_many(imgs[:3], (3, 5))))


# 10 ---- streams and devices
def test_non_default_stream():
    name, f = "g_seam", "linear"
    imgs = _inputs(name, "interleaved")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        small, b2 = aa.reduce_many_for_resize(imgs, [4, 375], MODE[f], reducing_gap=2.0)
        y = aa.resize_many(small, [4, 375], MODE[f], boxes=b2)
    s.synchronize()
    for i in range(2):
        ref.assert_resize_matches_fixture(f"{name}/{f}/{i}", ref.item(name, i), kit_gpu.hwc(y[i]))


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_non_current_device():
    name, f = "g_seam", "linear"
    imgs = [t.to("cuda:1") for t in _inputs(name, "interleaved")]
    assert torch.cuda.current_device() == 0
    small, b2 = aa.reduce_many_for_resize(imgs, [4, 375], MODE[f], reducing_gap=2.0)
    assert small[0].device == imgs[0].device and small[1] is imgs[1] and torch.cuda.current_device() == 0
    y = aa.resize_many(small, [4, 375], MODE[f], boxes=b2)
    torch.cuda.synchronize(1)
    for i in range(2):
        ref.assert_resize_matches_fixture(f"{name}/{f}/{i}", ref.item(name, i), kit_gpu.hwc(y[i]))
