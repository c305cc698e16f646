"""resize_many_nearest on the GPU: every fixture case in every layout class against Pillow's NEAREST (tolerance 0), the int64 output, the
paired-geometry promise with resize_many_to_float, items read where they lie and up to the last byte of their storage, guard bands around
every buffer, a side stream, and the empty batch."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import guard_ref  # noqa: E402
import kit_gpu  # noqa: E402
import resize_many_nearest_ref as ref  # noqa: E402

from interpolate_antialiasing_amd import extension_interpolate as aa  # noqa: E402
from interpolate_antialiasing_amd import tables  # noqa: E402

pytestmark = pytest.mark.gpu

G = ref.gen()
CLASSES = [(cs[0], cls) for cs in G.CASES for cls in (("planar",) if cs[2] == 1 else ("interleaved", "planar"))]
SINGLE = [cs[0] for cs in G.CASES if cs[2] == 1]


@functools.lru_cache(maxsize=None)
def _inputs(name, cls):
    """The case's images on the GPU (shared between tests, never written): a list, or one [N, C, H, W] tensor for a batch case."""
    cs = G.case(name)
    return kit_gpu.batch_or_list([kit_gpu.to_gpu(x, cls) for x in ref.inputs(name)], cs[9], cls)


@functools.lru_cache(maxsize=None)
def _expected(name):
    """Pillow's batch as [N, C, oH, oW] on the CPU (shared, never written)."""
    return torch.from_numpy(np.ascontiguousarray(ref.expected(name).transpose(0, 3, 1, 2)))


# ---- every fixture case, every class -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cls", CLASSES)
def test_fixture_case(name, cls):
    cs = G.case(name)
    y = aa.resize_many_nearest(_inputs(name, cls), list(cs[3]), **ref.call_args(name))
    kit_gpu.assert_class_format(y, cls, cs[2])
    kit_gpu.assert_bits(y, _expected(name), (name, cls))


@pytest.mark.parametrize("name", SINGLE)
def test_int64_output_is_long_of_the_result(name):
    """Zero-extended from uint8, sign-extended from int16 / int32: exactly y.long()."""
    cs = G.case(name)
    y = aa.resize_many_nearest(_inputs(name, "planar"), list(cs[3]), out_dtype=torch.int64, **ref.call_args(name))
    assert y.is_contiguous()
    exp = _expected(name)
    kit_gpu.assert_bits(y, exp.long(), name)
    if name in ("i16", "i32", "i16_seam", "i32_seam"):
        assert int(exp.min()) < 0 and int(y.min()) == int(exp.min())  # the negative ids and the fill -1 stayed negative
    if cs[1] == "u1":
        assert int(y.min()) >= 0 and int(y.max()) <= 255


def test_the_torch_op_runs_the_call():
    name = "placed_c3"
    cs = G.case(name)
    kw = ref.call_args(name)
    y = torch.ops.extension_interpolate.resize_many_nearest(
        _inputs(name, "interleaved"), list(cs[3]), boxes=[float(v) for i, b in enumerate(kw["boxes"]) for v in (b or (0, 0, cs[5][i][1], cs[5][i][0]))],
        flips=kw["flips"], sizes=[v for s in kw["sizes"] for v in s], offsets=[v for o in kw["offsets"] for v in o], fill=kw["fill"])
    kit_gpu.assert_bits(y, _expected(name), name)


# ---- the paired-geometry promise -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cls", [("placed_c3", "interleaved"), ("center", "planar"), ("plain_flips", "planar")])
def test_same_geometry_arguments_serve_image_and_mask(name, cls):
    """The SAME boxes / sizes / offsets / flips go to resize_many_to_float for the image and to resize_many_nearest for the mask; the
    antialiased call's mode="nearest" stays what it was, the box filter: its result is still its own uint8 call's, converted and flipped."""
    cs = G.case(name)
    imgs = _inputs(name, cls)
    kw = ref.call_args(name)
    mask = aa.resize_many_nearest(imgs, list(cs[3]), **kw)
    kit_gpu.assert_bits(mask, torch.from_numpy(np.ascontiguousarray(ref.restate(cs, ref.inputs(name)).transpose(0, 3, 1, 2))), (name, cls))
    image = aa.resize_many_to_float(imgs, list(cs[3]), "nearest", **kw)
    kw_u8 = {k: v for k, v in kw.items() if k != "flips"}
    u = aa.resize_many(imgs, list(cs[3]), "nearest", **kw_u8).float()
    flips = kw["flips"] or [False] * len(u)
    exp = torch.stack([u[i].flip(-1) if flips[i] else u[i] for i in range(len(u))])
    assert torch.equal(image.cpu(), exp.cpu()), (name, cls)
    box_filter = aa.resize_many(imgs, list(cs[3]), "box", **kw_u8).float()
    assert torch.equal(u, box_filter)  # "nearest" there is an alias of the box filter, not this call


# ---- items read where they lie ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["interleaved", "planar"])
def test_crops_of_larger_tensors_offset_and_pitch(cls):
    name = "plain_c3"
    cs = G.case(name)
    views = []
    for i, x in enumerate(ref.inputs(name)):
        c, h, w = x.shape
        big = np.full((c, h + 5, w + 7 + i), 99, np.uint8)
        big[:, 2:2 + h, 3 + i:3 + i + w] = x
        views.append(kit_gpu.to_gpu(big, cls)[:, 2:2 + h, 3 + i:3 + i + w])
    assert not any(v.is_contiguous() for v in views)
    y = aa.resize_many_nearest(views, list(cs[3]), **ref.call_args(name))
    kit_gpu.assert_class_format(y, cls, 3)
    kit_gpu.assert_bits(y, _expected(name), (name, cls))


def test_minority_class_items_are_copied():
    name = "plain_c3"
    cs = G.case(name)
    xs = ref.inputs(name)
    mixed = [kit_gpu.to_gpu(x, "interleaved" if i < 3 else "planar") for i, x in enumerate(xs)]
    y = aa.resize_many_nearest(mixed, list(cs[3]), **ref.call_args(name))
    kit_gpu.assert_class_format(y, "interleaved", 3)
    kit_gpu.assert_bits(y, _expected(name), name)


def test_instance_mask_stack_goes_in_as_single_plane_views():
    rng = np.random.default_rng(9)
    stack = rng.integers(0, 2, (6, 21, 33)).astype(np.uint8)
    t = torch.from_numpy(stack).cuda()
    box = (2.5, 1.0, 30.0, 20.5)
    y = aa.resize_many_nearest([t[k:k + 1] for k in range(6)], (10, 12), boxes=[box] * 6)
    exp = np.stack([ref.resize_nearest(stack[k:k + 1], (10, 12), box).transpose(2, 0, 1) for k in range(6)])
    kit_gpu.assert_bits(y, torch.from_numpy(exp), "stack")


def test_more_items_than_single_lane_waves():
    """Beyond 1024 items the table kernel packs several (item, axis) lanes into a wave: 1100 views of one small map, mixed geometry."""
    rng = np.random.default_rng(12)
    x = rng.integers(0, 256, (1, 6, 9)).astype(np.uint8)
    t = torch.from_numpy(x).cuda()
    n = 1100
    boxes = [None if i % 3 == 0 else (0.25 * (i % 5), 0.5 * (i % 4), 9.0 - 0.125 * (i % 7), 6.0 - 0.25 * (i % 3)) for i in range(n)]
    sizes = [(2 + i % 4, 3 + i % 6) for i in range(n)]
    offsets = [(i % 3 - 1, 1 - i % 4) for i in range(n)]
    flips = [i % 2 == 1 for i in range(n)]
    y = aa.resize_many_nearest([t] * n, (4, 6), boxes=boxes, sizes=sizes, offsets=offsets, flips=flips, fill=255)
    exp = np.stack([ref.place(ref.resize_nearest(x, sizes[i], boxes[i]), (4, 6), offsets[i], (255,), flips[i]).transpose(2, 0, 1) for i in range(n)])
    kit_gpu.assert_bits(y, torch.from_numpy(np.ascontiguousarray(exp)), "1100 items")


@pytest.mark.parametrize("dtype,c,cls", [(np.uint8, 1, "planar"), (np.uint8, 3, "interleaved"), (np.uint8, 3, "planar"), (np.int16, 1, "planar"),
                                         (np.int32, 1, "planar")])
def test_items_ending_exactly_on_their_allocation(dtype, c, cls):
    """Every item is a view whose last element is the last element of its storage, read with the last row and column in the tables (an
    upscale, whole image and a box that ends at the image's corner): the gather reads whole elements inside the image only."""
    rng = np.random.default_rng(10)
    h, w = 5, 7
    items, exps = [], []
    for i, box in enumerate([None, (2.5, 1.5, 7.0, 5.0)]):
        x = rng.integers(0, 200, (c, h, w)).astype(dtype)
        if cls == "interleaved":
            flat = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 2, 0)).reshape(-1)).cuda()
            t = flat.view(h, w, c).permute(2, 0, 1)
        else:
            flat = torch.from_numpy(x.reshape(-1)).cuda()
            t = flat.view(c, h, w)
        assert t.untyped_storage().nbytes() == flat.numel() * flat.element_size()
        assert t.data_ptr() + (t.numel() * t.element_size()) == flat.data_ptr() + t.untyped_storage().nbytes()
        items.append(t)
        exps.append(ref.resize_nearest(x, (11, 16), box, closed_form=dtype == np.int16).transpose(2, 0, 1))
    y = aa.resize_many_nearest(items, (11, 16), boxes=[None, (2.5, 1.5, 7.0, 5.0)])
    kit_gpu.assert_bits(y, torch.from_numpy(np.stack(exps)), (dtype, c, cls))


# ---- guard bands -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("name,cls", [("placed_c3", "interleaved"), ("placed_c3", "planar"), ("seam1025", "planar"), ("seam1026", "interleaved"),
                                      ("w5_c3", "interleaved"), ("w1_c1", "planar")])
def test_guard_bands_uint8(monkeypatch, name, cls, lead):
    """The descriptor's device copy, the tables and the output: nothing outside them is written, and every byte of the output is (a run
    into 0xFF-filled and a run into 0x00-filled memory agree)."""
    cs = G.case(name)
    imgs = _inputs(name, cls)
    runs = []
    for fill in (0xFF, 0x00):
        with guard_ref.guarded(monkeypatch, lead, fill) as rec:
            y = aa.resize_many_nearest(imgs, list(cs[3]), **ref.call_args(name))
            rec.check()
            assert len(rec.records) == 3 and len(rec.outputs()) == 1  # desc_dev, ws, out
            assert rec.record_of(y) is not None and y.data_ptr() % 2 == lead
            runs.append(y.cpu())
    assert guard_ref.unwritten_u8(runs[0], runs[1]) == 0, (name, cls, lead)
    assert torch.equal(runs[0], _expected(name)), (name, cls, lead)


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("name", ["placed_c1", "seam1025", "i16_seam", "i32_seam", "w5_c1"])
def test_guard_bands_int64(monkeypatch, name, lead):
    cs = G.case(name)
    imgs = _inputs(name, "planar")
    runs = []
    for fill in (0xFF, 0x00):
        with guard_ref.guarded(monkeypatch, lead, fill) as rec:
            y = aa.resize_many_nearest(imgs, list(cs[3]), out_dtype=torch.int64, **ref.call_args(name))
            rec.check()
            assert len(rec.records) == 3 and rec.record_of(y) is not None and y.data_ptr() % 16 == 8 * lead
            runs.append(y.cpu())
    assert guard_ref.unwritten_u8(runs[0].view(torch.uint8), runs[1].view(torch.uint8)) == 0, (name, lead)
    assert torch.equal(runs[0], _expected(name).long()), (name, lead)


@pytest.mark.parametrize("name", ["i16", "i32", "i16_seam"])
def test_guard_bands_wide_elements(monkeypatch, name):
    cs = G.case(name)
    imgs = _inputs(name, "planar")
    runs = []
    for fill in (0xFF, 0x00):
        with guard_ref.guarded(monkeypatch, 1, fill) as rec:
            y = aa.resize_many_nearest(imgs, list(cs[3]), **ref.call_args(name))
            rec.check()
            runs.append(y.cpu())
    assert guard_ref.unwritten_u8(runs[0].view(torch.uint8), runs[1].view(torch.uint8)) == 0, name
    assert torch.equal(runs[0], _expected(name)), name


# ---- streams, caches, the empty batch --------------------------------------------------------------------------------------------------------
def test_side_stream_and_a_second_call_reusing_nothing():
    name = "placed_c3"
    cs = G.case(name)
    imgs = _inputs(name, "interleaved")
    before = (len(tables._cache), len(tables._box_cache))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        y1 = aa.resize_many_nearest(imgs, list(cs[3]), **ref.call_args(name))
        other = "plain_c3"
        y2 = aa.resize_many_nearest(_inputs(other, "interleaved"), list(G.case(other)[3]), **ref.call_args(other))
        y3 = aa.resize_many_nearest(imgs, list(cs[3]), **ref.call_args(name))
    s.synchronize()
    assert (len(tables._cache), len(tables._box_cache)) == before  # the table caches are neither read nor written
    kit_gpu.assert_bits(y1, _expected(name), "first")
    kit_gpu.assert_bits(y2, _expected(other), "second")
    kit_gpu.assert_bits(y3, _expected(name), "third")
    assert y1.data_ptr() != y3.data_ptr()


def test_empty_batch():
    y = aa.resize_many_nearest([], (8, 9), channels=3)
    assert tuple(y.shape) == (0, 3, 8, 9) and y.dtype == torch.uint8 and y.is_cuda
    y = aa.resize_many_nearest(torch.zeros((0, 1, 5, 5), dtype=torch.int32, device="cuda"), (8, 9), out_dtype=torch.int64)
    assert tuple(y.shape) == (0, 1, 8, 9) and y.dtype == torch.int64 and y.is_cuda
