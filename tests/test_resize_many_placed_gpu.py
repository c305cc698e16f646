"""The placed resize_many on the GPU: every fixture case, filter and layout class against Pillow's resize pasted into the fill-coloured
canvas (tolerance 0), equality with the single-image call cropped and pasted by torch, items read where they lie, the converting call
against torch's conversion of the placed bytes, guard bands around every buffer, and the call's promises about caches."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import guard_ref  # noqa: E402
import kit_gpu  # noqa: E402
import resize_many_placed_ref as ref  # noqa: E402
from kit_golden import MEAN, MODE, STD  # noqa: E402
from kit_gpu import FORWARD  # noqa: E402

from interpolate_antialiasing_amd import extension_interpolate as aa  # noqa: E402
from interpolate_antialiasing_amd import tables  # noqa: E402

pytestmark = pytest.mark.gpu

G = ref.gen()
CASE_NAMES = [cs[0] for cs in G.CASES]
CLASSES = [(name, cls) for name in CASE_NAMES for cls in (("planar",) if G.case(name)[1] == 1 else ("interleaved", "planar"))]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]


@functools.lru_cache(maxsize=None)
def _inputs(name, cls):
    """The case's images on the GPU (shared between tests, never written): a list, or one [N, C, H, W] tensor for a batch case."""
    cs = G.case(name)
    return kit_gpu.batch_or_list([kit_gpu.to_gpu(ref.item(name, i), cls) for i in range(len(cs[5]))], cs[7], cls)


def _kw(name):
    return {"boxes": ref.boxes(name), "sizes": ref.sizes(name), "offsets": ref.offsets(name), "fill": ref.fill(name)}


@functools.lru_cache(maxsize=None)
def _bytes(name, f):
    """The expected canvases of one case and filter from the CPU restatement (pinned to Pillow by the CPU tests): [N, C, oH, oW] uint8 on
    the CPU (shared, never written)."""
    cs = G.case(name)
    return torch.from_numpy(np.stack([G.restated(cs, f, i, ref.item(name, i)).transpose(2, 0, 1) for i in range(len(cs[5]))]))


_check_against_fixture = functools.partial(kit_gpu.check_against_fixture, ref, 5)  # (a case keeps its items at [5])


@pytest.mark.parametrize("name,cls", CLASSES)
def test_every_case_filter_and_layout_class_equals_pillow(name, cls):
    cs = G.case(name)
    for f in cs[4]:
        y = aa.resize_many(_inputs(name, cls), list(cs[2]), MODE[f], **_kw(name))
        kit_gpu.assert_class_format(y, cls, cs[1])
        _check_against_fixture(name, f, y)


@pytest.mark.parametrize("cls", ["interleaved", "planar"])
@pytest.mark.parametrize("name", ["p_edges", "p_batch"])
def test_each_item_equals_the_single_image_call_cropped_and_pasted(name, cls):
    cs = G.case(name)
    imgs, kw = _inputs(name, cls), _kw(name)
    oh, ow = cs[2]
    for f in cs[4]:
        y = aa.resize_many(imgs, [oh, ow], MODE[f], **kw)
        for i in range(len(cs[5])):
            (vh, vw), (py, px) = kw["sizes"][i], kw["offsets"][i]
            one = FORWARD[f](imgs[i][None], [vh, vw], box=kw["boxes"][i])[0]
            want = torch.tensor(kw["fill"], dtype=torch.uint8, device="cuda").view(-1, 1, 1).expand(cs[1], oh, ow).clone()
            y0, y1, x0, x1 = max(0, py), min(oh, py + vh), max(0, px), min(ow, px + vw)
            if y1 > y0 and x1 > x0:
                want[:, y0:y1, x0:x1] = one[:, y0 - py:y1 - py, x0 - px:x1 - px]
            assert torch.equal(y[i], want), (name, f, i)
    if name == "p_edges":  # item 0 is today's plain call
        plain = aa.resize_many([imgs[0]], [oh, ow], "bicubic")
        assert torch.equal(aa.resize_many(imgs, [oh, ow], "bicubic", **kw)[0], plain[0])


@pytest.mark.parametrize("cls", ["interleaved", "planar"])
@pytest.mark.parametrize("name", ["p_edges", "p_c4"])
def test_crops_at_odd_offsets_and_pitches_are_read_in_place(name, cls):
    cs = G.case(name)
    crops = [kit_gpu.pitched_crop(ref.item(name, i), cls, i) for i in range(len(cs[5]))]
    for f in cs[4]:
        y = aa.resize_many(crops, list(cs[2]), MODE[f], **_kw(name))
        dense = aa.resize_many(_inputs(name, cls), list(cs[2]), MODE[f], **_kw(name))
        assert y.stride() == dense.stride() and torch.equal(y, dense)
        _check_against_fixture(name, f, y)


# ---- resize_many_to_float ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("cls", ["interleaved", "planar"])
@pytest.mark.parametrize("name", ["p_letterbox", "p_edges"])
def test_to_float_is_the_placed_bytes_converted(name, cls, dtype):
    cs = G.case(name)
    n, c = len(cs[5]), cs[1]
    flips = [i % 2 == 0 for i in range(n)]
    for f in cs[4]:
        u = aa.resize_many(_inputs(name, cls), list(cs[2]), MODE[f], **_kw(name)).cpu()
        assert torch.equal(u, _bytes(name, f)), (name, f)  # (the placed bytes are Pillow's: what is converted below is not the call's own)
        want = kit_gpu.convert(u, dtype, flips=flips)
        for fmt in ("nchw", "nhwc"):
            y = aa.resize_many_to_float(_inputs(name, cls), list(cs[2]), MODE[f], flips=flips, out_dtype=dtype, out_format=fmt, mean=MEAN[:c],
                                        std=STD[:c], **_kw(name))
            assert y.is_contiguous(memory_format=torch.channels_last) == (fmt == "nhwc") and y.is_contiguous() == (fmt == "nchw")
            assert torch.equal(kit_gpu.bits(y), kit_gpu.bits(want)), (name, f, cls, fmt, dtype)
    # the fill area holds (fill[c] - mean[c]) / std[c], rounded once: item 4 of p_edges is all fill, row 0 of p_letterbox's item 2 too
    fillv = ((torch.tensor(ref.fill(name)).float() - torch.tensor(MEAN[:c])) / torch.tensor(STD[:c])).to(dtype)
    area = y[4] if name == "p_edges" else y[2][:, :1, :]
    assert torch.equal(kit_gpu.bits(area), kit_gpu.bits(fillv.view(c, 1, 1).expand_as(area))), (name, dtype)


# ---- guard bands ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("cls", ["interleaved", "planar"])
@pytest.mark.parametrize("name", ["p_edges", "p_letterbox", "p_strips"])
def test_guard_bands_uint8(monkeypatch, name, cls, lead):
    """The descriptor's device copy, the arena of tables and intermediates and the output: nothing outside them is written, and every
    byte of the output is (a run into 0xFF-filled and a run into 0x00-filled memory agree)."""
    cs = G.case(name)
    imgs = _inputs(name, cls)
    for f in cs[4]:
        runs = []
        for fill in (0xFF, 0x00):
            with guard_ref.guarded(monkeypatch, lead, fill) as rec:
                y = aa.resize_many(imgs, list(cs[2]), MODE[f], **_kw(name))
                rec.check()
                assert len(rec.records) == 3 and len(rec.outputs()) == 1  # desc_dev, ws, out
                assert rec.record_of(y) is not None and y.data_ptr() % 2 == lead
                runs.append(y.cpu())
        assert guard_ref.unwritten_u8(runs[0], runs[1]) == 0, (name, f, cls, lead)
        assert torch.equal(runs[0], _bytes(name, f)), (name, f, cls, lead)


@pytest.mark.parametrize("cls", ["interleaved", "planar"])
@pytest.mark.parametrize("name", ["p_edges", "p_letterbox", "p_strips"])
def test_guard_bands_bf16_nchw(monkeypatch, name, cls):
    cs = G.case(name)
    n, c = len(cs[5]), cs[1]
    flips = [i % 2 == 1 for i in range(n)]
    f = cs[4][0]
    with guard_ref.guarded(monkeypatch, 1) as rec:
        y = aa.resize_many_to_float(_inputs(name, cls), list(cs[2]), MODE[f], flips=flips, out_dtype=torch.bfloat16, out_format="nchw",
                                    mean=MEAN[:c], std=STD[:c], **_kw(name))
        rec.check()
        assert len(rec.records) == 3 and rec.record_of(y) is not None
        assert guard_ref.unwritten_float(y) == 0
    kit_gpu.assert_bits(y, kit_gpu.convert(_bytes(name, f), torch.bfloat16, flips=flips), (name, f, cls))


# ---- caches, the torch op ------------------------------------------------------------------------------------------------------------
def test_no_cache_is_read_or_written():
    before = (len(tables._cache), len(tables._box_cache), len(aa._plans))
    y = aa.resize_many(_inputs("p_edges", "interleaved"), [30, 45], "bicubic", **_kw("p_edges"))
    z = aa.resize_many_to_float(_inputs("p_edges", "interleaved"), [30, 45], "bicubic", out_dtype=torch.bfloat16, **_kw("p_edges"))
    torch.cuda.synchronize()
    assert (len(tables._cache), len(tables._box_cache), len(aa._plans)) == before
    _check_against_fixture("p_edges", "cubic", y)
    assert torch.equal(z.float().cpu(), y.float().cpu())  # (bytes are exact in bfloat16)


def test_center_offsets_and_the_torch_op():
    name = "p_eval"
    cs = G.case(name)
    imgs = _inputs(name, "interleaved")
    # the case's offsets are "center" of its sizes on the 28 x 28 canvas
    y = aa.resize_many(imgs, [28, 28], "bicubic", sizes=ref.sizes(name), offsets="center")
    _check_against_fixture(name, "cubic", y)
    flat_s = [v for s in ref.sizes(name) for v in s]
    flat_o = [v for o in ref.offsets(name) for v in o]
    y = torch.ops.extension_interpolate.resize_many(imgs, [28, 28], "bilinear", None, flat_s, flat_o, [0])
    _check_against_fixture(name, "linear", y)
    z = torch.ops.extension_interpolate.resize_many_to_float(imgs, [28, 28], "bilinear", sizes=flat_s, offsets=flat_o, out_format="nchw")
    assert z.dtype == torch.float32 and z.is_contiguous() and torch.equal(z.cpu(), y.float().cpu())
    assert len(cs[5]) == 4
