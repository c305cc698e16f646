"""resize_many on the GPU: every fixture case, filter and layout class against Pillow's bytes (tolerance 0), items read where they lie,
equality with the single-image call, and the call's promises about caches, streams and devices."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kit_gpu  # noqa: E402
import resize_many_ref as ref  # noqa: E402
from kit_golden import MODE  # noqa: E402
from kit_gpu import FORWARD  # noqa: E402

from interpolate_antialiasing_amd import extension_interpolate as aa  # noqa: E402
from interpolate_antialiasing_amd import tables  # noqa: E402

pytestmark = pytest.mark.gpu

G = ref.gen()
CASE_NAMES = [cs[0] for cs in G.CASES]
CLASSES = [(name, cls) for name in CASE_NAMES for cls in (("planar",) if G.case(name)[1] == 1 else ("interleaved", "planar"))]


@functools.lru_cache(maxsize=None)
def _inputs(name, cls):
    """The case's images on the GPU (shared between tests, never written): a list, or one [N, C, H, W] tensor for a batch case."""
    cs = G.case(name)
    return kit_gpu.batch_or_list([kit_gpu.to_gpu(ref.item(name, i), cls) for i in range(len(cs[3]))], cs[6], cls)


def _boxes(name):
    return [it[2] for it in G.case(name)[3]]


_check_against_fixture = functools.partial(kit_gpu.check_against_fixture, ref, 3)  # (a case keeps its items at [3])


@pytest.mark.parametrize("name,cls", CLASSES)
def test_every_case_filter_and_layout_class_equals_pillow(name, cls):
    cs = G.case(name)
    for f in cs[4]:
        y = aa.resize_many(_inputs(name, cls), list(cs[2]), MODE[f], boxes=_boxes(name))
        kit_gpu.assert_class_format(y, cls, cs[1])
        _check_against_fixture(name, f, y)


@pytest.mark.parametrize("cls", ["interleaved", "planar"])
@pytest.mark.parametrize("name", ["m_mixed", "m_c4"])
def test_crops_at_odd_offsets_and_pitches_are_read_in_place(name, cls):
    cs = G.case(name)
    crops = [kit_gpu.pitched_crop(ref.item(name, i), cls, i) for i in range(len(cs[3]))]
    for f in cs[4]:
        y = aa.resize_many(crops, list(cs[2]), MODE[f], boxes=_boxes(name))
        dense = aa.resize_many(_inputs(name, cls), list(cs[2]), MODE[f], boxes=_boxes(name))
        assert y.stride() == dense.stride() and torch.equal(y, dense)
        _check_against_fixture(name, f, y)


@pytest.mark.parametrize("cls", ["interleaved", "planar"])
@pytest.mark.parametrize("name", ["m_mixed", "m_batchbox"])
def test_each_item_equals_the_single_image_call(name, cls):
    cs = G.case(name)
    imgs, boxes = _inputs(name, cls), _boxes(name)
    for f in cs[4]:
        y = aa.resize_many(imgs, list(cs[2]), MODE[f], boxes=boxes)
        for i in range(len(cs[3])):
            one = FORWARD[f](imgs[i][None], list(cs[2]), box=boxes[i])
            assert torch.equal(y[i], one[0]), (name, f, i)


def test_no_cache_is_read_or_written():
    before = (len(tables._cache), len(tables._box_cache), len(aa._plans))
    y = aa.resize_many(_inputs("m_mixed", "interleaved"), [30, 45], "bicubic", boxes=_boxes("m_mixed"))
    torch.cuda.synchronize()
    assert (len(tables._cache), len(tables._box_cache), len(aa._plans)) == before
    _check_against_fixture("m_mixed", "cubic", y)


def test_permuting_the_items_permutes_the_output():
    imgs, boxes = _inputs("m_mixed", "interleaved"), _boxes("m_mixed")
    y = aa.resize_many(imgs, [30, 45], "lanczos", boxes=boxes)
    perm = [4, 8, 0, 6, 2, 7, 1, 5, 3]
    yp = aa.resize_many([imgs[p] for p in perm], [30, 45], "lanczos", boxes=[boxes[p] for p in perm])
    assert torch.equal(yp, y[perm])


def test_one_image_and_no_image():
    imgs, boxes = _inputs("m_mixed", "interleaved"), _boxes("m_mixed")
    for i in (1, 6):
        y = aa.resize_many([imgs[i]], [30, 45], "bilinear", boxes=[boxes[i]])
        ref.assert_matches_fixture(f"m_mixed/linear/{i}", ref.item("m_mixed", i), kit_gpu.hwc(y[0]))
    y = aa.resize_many([imgs[0][None]], [30, 45], "bilinear")  # a [1, C, H, W] item, no boxes at all
    ref.assert_matches_fixture("m_mixed/linear/0", ref.item("m_mixed", 0), kit_gpu.hwc(y[0]))
    e = aa.resize_many([], [30, 45], channels=3)
    assert tuple(e.shape) == (0, 3, 30, 45) and e.dtype == torch.uint8 and e.is_cuda
    e = aa.resize_many(_inputs("m_batchbox", "planar")[:0], [30, 45])
    assert tuple(e.shape) == (0, 3, 30, 45) and e.is_cuda


def test_torch_op_takes_flattened_boxes():
    imgs, boxes = _inputs("m_c2", "interleaved"), _boxes("m_c2")
    flat = []
    for t, b in zip(imgs, boxes):
        flat += [float(v) for v in (b if b is not None else (0, 0, t.shape[2], t.shape[1]))]
    y = torch.ops.extension_interpolate.resize_many(imgs, [19, 77], "bicubic", flat)
    _check_against_fixture("m_c2", "cubic", y)


def test_non_default_stream():
    imgs, boxes = _inputs("m_strips", "interleaved"), _boxes("m_strips")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        y = aa.resize_many(imgs, [4, 130], "hamming", boxes=boxes)
    s.synchronize()
    _check_against_fixture("m_strips", "hamming", y)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_non_current_device():
    cs = G.case("m_strips")
    imgs = [t.to("cuda:1") for t in _inputs("m_strips", "interleaved")]
    assert torch.cuda.current_device() == 0
    y = aa.resize_many(imgs, [4, 130], "hamming", boxes=_boxes("m_strips"))
    assert y.device == imgs[0].device and torch.cuda.current_device() == 0
    torch.cuda.synchronize(1)
    _check_against_fixture("m_strips", "hamming", y)
    assert len(cs[3]) == 2


def test_a_mixed_list_copies_the_minority():
    name = "m_c4"
    inter, planar = _inputs(name, "interleaved"), _inputs(name, "planar")
    want = aa.resize_many(inter, [19, 77], "bicubic", boxes=_boxes(name))
    _check_against_fixture(name, "cubic", want)  # (what the mixed lists are compared with is Pillow's)
    y = aa.resize_many([inter[0], planar[1], inter[2]], [19, 77], "bicubic", boxes=_boxes(name))
    assert y.is_contiguous(memory_format=torch.channels_last) and torch.equal(y, want)
    y = aa.resize_many([planar[0], inter[1], planar[2]], [19, 77], "bicubic", boxes=_boxes(name))
    assert y.is_contiguous() and torch.equal(y, want)
    # an item in neither form (columns two bytes apart) is copied into the class of the others
    wide = torch.zeros((4, 64, 80), dtype=torch.uint8, device="cuda")
    odd = wide[:, :, ::2]
    odd.copy_(planar[2])
    y = aa.resize_many([inter[0], inter[1], odd], [19, 77], "bicubic", boxes=_boxes(name))
    assert y.is_contiguous(memory_format=torch.channels_last) and torch.equal(y, want)
