"""resize_many(alpha=True) and resize_many_to_float(alpha=True) on the GPU, tolerance 0 throughout: every fixture case, filter and layout
class against Pillow's RGBA / LA resize (the fixture) and the numpy restatement the CPU tests pin to it, equality with the single-image
alpha call pasted by torch, items read where they lie, the staging-chunk seams of the horizontal pass, the converting call against torch's
conversion of the alpha bytes, guard bands around every buffer with the inputs left unchanged, and the call's promises."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import guard_ref  # noqa: E402
import kit_golden  # noqa: E402
import kit_gpu  # noqa: E402
import resize_many_alpha_ref as ref  # noqa: E402
from kit_golden import MEAN, STD  # noqa: E402
from kit_gpu import FORWARD  # noqa: E402

from interpolate_antialiasing_amd import extension_interpolate as aa  # noqa: E402
from interpolate_antialiasing_amd import tables  # noqa: E402

pytestmark = pytest.mark.gpu

G = ref.gen()
CASE_NAMES = [cs[0] for cs in G.CASES]
MODE = {**kit_golden.MODE, "box": "nearest"}  # (on purpose: the alias of the box filter's mode)
CLS = ["interleaved", "planar"]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]


@functools.lru_cache(maxsize=None)
def _inputs(name, cls):
    """The case's images on the GPU (shared between tests, never written)."""
    return [kit_gpu.to_gpu(ref.item(name, i), cls) for i in range(len(G.case(name)[5]))]


@functools.lru_cache(maxsize=None)
def _bytes(name, f, alpha=True):
    """The expected canvases of one case and filter from the CPU restatement: [N, C, oH, oW] uint8 on the CPU (shared, never written)."""
    return torch.from_numpy(np.stack([ref.restated(name, f, i, alpha).transpose(2, 0, 1) for i in range(len(G.case(name)[5]))]))


# (a case keeps its items at [5]; the whole result is the restatement's too)
_check_against_fixture = functools.partial(kit_gpu.check_against_fixture, ref, 5, restated=_bytes)


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", CLS)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_every_case_filter_and_layout_class_equals_pillow(name, cls):
    cs = G.case(name)
    for f in cs[4]:
        y = aa.resize_many(_inputs(name, cls), list(cs[2]), MODE[f], alpha=True, **ref.kwargs(name))
        kit_gpu.assert_class_format(y, cls, cs[1])
        _check_against_fixture(name, f, y)


@pytest.mark.parametrize("cls", CLS)
@pytest.mark.parametrize("name", ["a_rgba", "a_la", "a_placed4", "a_placed2"])
def test_each_item_equals_the_single_image_alpha_call_pasted(name, cls):
    cs = G.case(name)
    imgs = _inputs(name, cls)
    oh, ow = cs[2]
    for f in cs[4]:
        y = aa.resize_many(imgs, [oh, ow], MODE[f], alpha=True, **ref.kwargs(name))
        for i, (_, _, box, (vh, vw), (py, px)) in enumerate(cs[5]):
            one = FORWARD[f](imgs[i][None], [vh, vw], box=box, alpha=True)[0]
            want = torch.tensor(cs[3], dtype=torch.uint8, device="cuda").view(-1, 1, 1).expand(cs[1], oh, ow).clone()
            y0, y1, x0, x1 = max(0, py), min(oh, py + vh), max(0, px), min(ow, px + vw)
            if y1 > y0 and x1 > x0:
                want[:, y0:y1, x0:x1] = one[:, y0 - py:y1 - py, x0 - px:x1 - px]
            kit_gpu.assert_bits(y[i], want, (name, f, i))


def test_alpha_false_on_the_same_inputs_is_todays_result():
    """The flag does not leak: without it the same RGBA / LA tensors resize channel by channel, before and after a call with it."""
    for name in ("a_rgba", "a_la", "a_placed4", "a_copy4"):
        cs = G.case(name)
        for cls in CLS:
            for f in cs[4][:2]:
                before = aa.resize_many(_inputs(name, cls), list(cs[2]), MODE[f], **ref.kwargs(name))
                with_alpha = aa.resize_many(_inputs(name, cls), list(cs[2]), MODE[f], alpha=True, **ref.kwargs(name))
                after = aa.resize_many(_inputs(name, cls), list(cs[2]), MODE[f], alpha=False, **ref.kwargs(name))
                kit_gpu.assert_bits(before, _bytes(name, f, False), (name, cls, f))
                kit_gpu.assert_bits(after, _bytes(name, f, False), (name, cls, f))
                assert not torch.equal(with_alpha.cpu(), _bytes(name, f, False))


# ---- items read where they lie -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", CLS)
@pytest.mark.parametrize("name", ["a_rgba", "a_la", "a_placed4", "a_placed2"])
def test_crops_at_odd_offsets_and_pitches_are_read_in_place(name, cls):
    cs = G.case(name)
    crops = [kit_gpu.pitched_crop(ref.item(name, i), cls, i) for i in range(len(cs[5]))]
    for f in cs[4]:
        y = aa.resize_many(crops, list(cs[2]), MODE[f], alpha=True, **ref.kwargs(name))
        kit_gpu.assert_class_format(y, cls, cs[1])
        _check_against_fixture(name, f, y)


@pytest.mark.parametrize("first", [0, 1])
def test_rgba_planes_sliced_out_of_a_five_plane_buffer(first):
    """Four of five planes, plane pitch H * W + 3: the alpha plane's rows lie at another misalignment than the colour planes' rows."""
    name = "a_rgba"
    cs = G.case(name)
    items = []
    for i in range(len(cs[5])):
        x = ref.item(name, i)
        _, h, w = x.shape
        plane = h * w + 3
        buf = torch.full((5 * plane + 16,), 0x5A, dtype=torch.uint8, device="cuda")
        five = buf.as_strided((5, h, w), (plane, w, 1), 0)
        v = five[first:first + 4]
        v.copy_(torch.from_numpy(x).cuda())
        assert v.stride(0) == plane and aa._many_class(v) == (False, True)
        items.append(v)
    for f in ("cubic", "lanczos"):
        y = aa.resize_many(items, list(cs[2]), MODE[f], alpha=True, boxes=ref.boxes(name))
        kit_gpu.assert_class_format(y, "planar", cs[1])
        _check_against_fixture(name, f, y)


@pytest.mark.parametrize("cls", CLS)
def test_one_batch_tensor_in_both_memory_formats(cls):
    n, c, h, w, oh, ow = 3, 4, 21, 34, 9, 13
    xs = [np.ascontiguousarray(G.make_image(h, w, c, 900 + i).transpose(2, 0, 1)) for i in range(n)]
    boxes = [None, (1.5, 2.0, 30.25, 19.0), None]
    x = torch.from_numpy(np.stack(xs)).cuda()
    x = x.contiguous(memory_format=torch.channels_last) if cls == "interleaved" else x.contiguous()
    want = torch.from_numpy(np.stack([G.resize_alpha_restated("cubic", xs[i].transpose(1, 2, 0), oh, ow, boxes[i]).transpose(2, 0, 1) for i in range(n)]))
    y = aa.resize_many(x, [oh, ow], "bicubic", boxes=boxes, alpha=True)
    kit_gpu.assert_class_format(y, cls, c)
    kit_gpu.assert_bits(y, want, cls)
    same = aa.resize_many(x, [h, w], "bicubic", alpha=True)  # every slice is Pillow's copy
    kit_gpu.assert_bits(same, x, cls)


@pytest.mark.parametrize("minority", CLS)
def test_a_list_mixing_the_classes_copies_the_minority(minority):
    name = "a_rgba"
    cs = G.case(name)
    majority = "planar" if minority == "interleaved" else "interleaved"
    imgs = [_inputs(name, minority if i == 2 else majority)[i] for i in range(len(cs[5]))]
    y = aa.resize_many(imgs, list(cs[2]), "bicubic", alpha=True, boxes=ref.boxes(name))
    kit_gpu.assert_class_format(y, majority, cs[1])
    _check_against_fixture(name, "cubic", y)


# ---- the staging chunks' seams -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,cls,h,w", ref.SEAMS)
def test_hulls_across_a_staging_chunk_seam(c, cls, h, w):
    x = ref.seam_item(c, h, w, 7)
    want = torch.from_numpy(ref.seam_restated(c, h, w, 7).transpose(2, 0, 1).copy())[None]
    for img in (kit_gpu.to_gpu(x, cls), kit_gpu.pitched_crop(x, cls, 0)):
        y = aa.resize_many([img], list(ref.SEAM_OUT), "bilinear", alpha=True)
        kit_gpu.assert_class_format(y, cls, c)
        kit_gpu.assert_bits(y, want, (c, cls, h, w))
    assert not np.array_equal(ref.seam_restated(c, h, w, 7), ref.seam_restated(c, h, w, 7, False))


# ---- resize_many_to_float ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("cls", CLS)
@pytest.mark.parametrize("name", ["a_rgba", "a_la", "a_placed4", "a_placed2"])
def test_to_float_is_the_alpha_bytes_converted(name, cls, dtype):
    cs = G.case(name)
    n, c = len(cs[5]), cs[1]
    flips = [i % 2 == 0 for i in range(n)]
    imgs = _inputs(name, cls)
    for f in cs[4][:3]:
        u = aa.resize_many(imgs, list(cs[2]), MODE[f], alpha=True, **ref.kwargs(name)).cpu()
        assert torch.equal(u, _bytes(name, f)), (name, f)  # (the bytes are Pillow's: what is converted below is not the call's own)
        for fmt in ("nchw", "nhwc", None):
            for normalize, fl in ((True, flips), (False, [False] * n), (False, flips)):
                kw = {"mean": MEAN[:c], "std": STD[:c]} if normalize else {}
                y = aa.resize_many_to_float(imgs, list(cs[2]), MODE[f], flips=fl if any(fl) else None, out_dtype=dtype, out_format=fmt, alpha=True,
                                            **kw, **ref.kwargs(name))
                nhwc = fmt == "nhwc" or (fmt is None and cls == "interleaved")
                assert y.is_contiguous(memory_format=torch.channels_last) == nhwc and y.is_contiguous() == (not nhwc)
                assert y.dtype == dtype and torch.equal(kit_gpu.bits(y), kit_gpu.bits(kit_gpu.convert(u, dtype, normalize, fl))), (name, f, cls, fmt, dtype, normalize)


def test_to_float_without_alpha_is_unchanged():
    name, f = "a_rgba", "cubic"
    cs = G.case(name)
    for cls in CLS:
        y = aa.resize_many_to_float(_inputs(name, cls), list(cs[2]), MODE[f], out_dtype=torch.float32, out_format="nchw", boxes=ref.boxes(name))
        assert torch.equal(kit_gpu.bits(y), kit_gpu.bits(_bytes(name, f, False).float()))


# ---- guard bands ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("cls", CLS)
@pytest.mark.parametrize("name", ["a_placed4", "a_placed2"])
def test_guard_bands_uint8(monkeypatch, name, cls, lead):
    """The descriptor's device copy, the arena of tables and intermediates and the output: nothing outside them is written, every byte
    of the output is (a run into 0xFF-filled and a run into 0x00-filled memory agree), and the inputs are unchanged afterwards."""
    cs = G.case(name)
    imgs = [t.clone(memory_format=torch.preserve_format) for t in _inputs(name, cls)]
    before = [t.cpu() for t in imgs]
    for f in cs[4]:
        runs = []
        for fill in (0xFF, 0x00):
            with guard_ref.guarded(monkeypatch, lead, fill) as rec:
                y = aa.resize_many(imgs, list(cs[2]), MODE[f], alpha=True, **ref.kwargs(name))
                rec.check()
                assert len(rec.records) == 3 and len(rec.outputs()) == 1  # desc_dev, ws, out
                assert rec.record_of(y) is not None and y.data_ptr() % 2 == lead
                runs.append(y.cpu())
        assert guard_ref.unwritten_u8(runs[0], runs[1]) == 0, (name, f, cls, lead)
        assert torch.equal(runs[0], _bytes(name, f)), (name, f, cls, lead)
    for t, b in zip(imgs, before):
        assert torch.equal(t.cpu(), b)


@pytest.mark.parametrize("cls", CLS)
@pytest.mark.parametrize("name", ["a_placed4", "a_placed2"])
def test_guard_bands_bf16_nchw(monkeypatch, name, cls):
    cs = G.case(name)
    n, c = len(cs[5]), cs[1]
    flips = [i % 2 == 1 for i in range(n)]
    f = cs[4][1]
    imgs = [t.clone(memory_format=torch.preserve_format) for t in _inputs(name, cls)]
    before = [t.cpu() for t in imgs]
    with guard_ref.guarded(monkeypatch, 1) as rec:
        y = aa.resize_many_to_float(imgs, list(cs[2]), MODE[f], flips=flips, out_dtype=torch.bfloat16, out_format="nchw", mean=MEAN[:c],
                                    std=STD[:c], alpha=True, **ref.kwargs(name))
        rec.check()
        assert len(rec.records) == 3 and rec.record_of(y) is not None
        assert guard_ref.unwritten_float(y) == 0
    assert torch.equal(kit_gpu.bits(y), kit_gpu.bits(kit_gpu.convert(_bytes(name, f), torch.bfloat16, flips=flips)))
    for t, b in zip(imgs, before):
        assert torch.equal(t.cpu(), b)


@pytest.mark.parametrize("c,cls,h,w", ref.SEAMS[::2])
def test_guard_bands_of_a_seam_case(monkeypatch, c, cls, h, w):
    """The input lies in a guarded buffer of its own: the in-place premultiply of a chunk that ends at the row's end touches LDS only."""
    x = ref.seam_item(c, h, w, 7)
    want = torch.from_numpy(ref.seam_restated(c, h, w, 7).transpose(2, 0, 1).copy())[None]
    pad = 4096
    buf = torch.full((pad + x.size + pad,), 0xC3, dtype=torch.uint8, device="cuda")
    body = buf[pad:pad + x.size]
    img = body.view(h, w, c).permute(2, 0, 1) if cls == "interleaved" else body.view(c, h, w)
    img.copy_(torch.from_numpy(x).cuda())
    held = buf.clone()
    runs = []
    for fill in (0xFF, 0x00):
        with guard_ref.guarded(monkeypatch, 1, fill) as rec:
            y = aa.resize_many([img], list(ref.SEAM_OUT), "bilinear", alpha=True)
            rec.check()
            assert len(rec.records) == 3 and rec.record_of(y) is not None
            runs.append(y.cpu())
    assert guard_ref.unwritten_u8(runs[0], runs[1]) == 0 and torch.equal(runs[0], want)
    with guard_ref.guarded(monkeypatch, 1) as rec:
        z = aa.resize_many_to_float([img], list(ref.SEAM_OUT), "bilinear", out_dtype=torch.float16, alpha=True)
        rec.check()
        assert guard_ref.unwritten_float(z) == 0
    assert torch.equal(kit_gpu.bits(z), kit_gpu.bits(want.to(torch.float16)))
    assert torch.equal(buf, held)


# ---- the call's promises -------------------------------------------------------------------------------------------------------------
def test_three_launches_whatever_n():
    name = "a_placed4"
    cs = G.case(name)
    kw = ref.kwargs(name)
    five = _inputs(name, "interleaved") + [_inputs(name, "interleaved")[0]]
    kw5 = {k: (v + [v[0]] if k != "fill" else v) for k, v in kw.items()}
    one = {k: (v[:1] if k != "fill" else v) for k, v in kw.items()}
    calls = {
        1: lambda: aa.resize_many(five[:1], list(cs[2]), "bicubic", alpha=True, **one),
        5: lambda: aa.resize_many(five, list(cs[2]), "bicubic", alpha=True, **kw5),
        "float": lambda: aa.resize_many_to_float(five, list(cs[2]), "bicubic", out_dtype=torch.bfloat16, out_format="nchw", alpha=True, **kw5),
    }
    for k, fn in calls.items():
        fn()  # (module load and allocator warm-up stay outside the count)
        names = kit_gpu.count_launches(fn)
        assert len(names) == 3, (k, names)
        assert [sum(1 for nm in names if part in nm) for part in ("many_tables", "many_hpass", "many_vpass")] == [1, 1, 1], (k, names)


def test_no_cache_is_read_or_written():
    name = "a_placed4"
    before = (len(tables._cache), len(tables._box_cache), len(aa._plans))
    y = aa.resize_many(_inputs(name, "interleaved"), [30, 45], "bicubic", alpha=True, **ref.kwargs(name))
    z = aa.resize_many_to_float(_inputs(name, "planar"), [30, 45], "bicubic", out_dtype=torch.bfloat16, alpha=True, **ref.kwargs(name))
    torch.cuda.synchronize()
    assert (len(tables._cache), len(tables._box_cache), len(aa._plans)) == before
    _check_against_fixture(name, "cubic", y)
    assert torch.equal(z.float().cpu(), y.float().cpu())  # (bytes are exact in bfloat16)
