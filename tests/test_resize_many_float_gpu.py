"""resize_many_to_float on the GPU.  Expected values never come from the package: the bytes are the CPU restatement's (pinned to Pillow by
the CPU tests; the fixture's CRC where the result is bytes again), for an ad-hoc shape too — where a test also compares with resize_many, it
first asserts that resize_many's bytes are the restatement's, because both calls share their horizontal pass and their vertical sums —
and the conversion is torch's on the CPU: ((b.float() - mean) / std).to(dtype), .flip(-1).  Bit patterns are compared: tolerance 0."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kit_gpu  # noqa: E402
import resize_many_ref as ref  # noqa: E402
from kit_golden import MEAN, MODE, STD  # noqa: E402

from interpolate_antialiasing_amd import _lib  # noqa: E402
from interpolate_antialiasing_amd import extension_interpolate as aa  # noqa: E402
from interpolate_antialiasing_amd import tables  # noqa: E402

pytestmark = pytest.mark.gpu

G = ref.gen()
CASE_NAMES = [cs[0] for cs in G.CASES]
CLASSES = [(name, cls) for name in CASE_NAMES for cls in (("planar",) if G.case(name)[1] == 1 else ("interleaved", "planar"))]
NORMALISED = [(name, cls) for name, cls in CLASSES if name in ("m_mixed", "m_c1", "m_c2", "m_c4", "m_strips", "m_tiny37")]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
FORMATS = ["nchw", "nhwc"]


@functools.lru_cache(maxsize=None)
def _inputs(name, cls):
    """The case's images on the GPU (shared between tests, never written): a list, or one [N, C, H, W] tensor for a batch case."""
    cs = G.case(name)
    return kit_gpu.batch_or_list([kit_gpu.to_gpu(ref.item(name, i), cls) for i in range(len(cs[3]))], cs[6], cls)


def _boxes(name):
    return [it[2] for it in G.case(name)[3]]


@functools.lru_cache(maxsize=None)
def _bytes(name, f):
    """Pillow's bytes of one case and filter from the CPU restatement: [N, C, oH, oW] uint8 on the CPU (shared, never written)."""
    cs = G.case(name)
    return torch.from_numpy(np.stack([G.restated(cs, f, i, ref.item(name, i)).transpose(2, 0, 1) for i in range(len(cs[3]))]))


def _assert_format(y, fmt, c):
    if c > 1:
        assert y.is_contiguous(memory_format=torch.channels_last) == (fmt == "nhwc") and y.is_contiguous() == (fmt == "nchw")
    else:
        assert y.is_contiguous()


def _norm(c, norm=True):
    return {"mean": MEAN[:c], "std": STD[:c]} if norm else {}


@pytest.mark.parametrize("name,cls", CLASSES)
def test_identity_every_case_filter_class_and_format_is_pillows_bytes(name, cls):
    cs = G.case(name)
    for f in cs[4]:
        for fmt in FORMATS:
            y = aa.resize_many_to_float(_inputs(name, cls), list(cs[2]), MODE[f], boxes=_boxes(name), out_format=fmt)
            assert y.dtype == torch.float32 and tuple(y.shape) == (len(cs[3]), cs[1]) + tuple(cs[2])
            _assert_format(y, fmt, cs[1])
            got = y.to(torch.uint8).cpu()
            assert torch.equal(got.float(), y.cpu())  # whole bytes, nothing else
            for i in range(len(cs[3])):
                ref.assert_matches_fixture(f"{name}/{f}/{i}", ref.item(name, i), got[i].permute(1, 2, 0).numpy())
        # out_format None follows the class of the items
        y = aa.resize_many_to_float(_inputs(name, cls), list(cs[2]), MODE[cs[4][0]], boxes=_boxes(name))
        _assert_format(y, "nhwc" if cls == "interleaved" else "nchw", cs[1])
        kit_gpu.assert_bits(y, kit_gpu.convert(_bytes(name, cs[4][0]), torch.float32, False), f"{name}/{cls}/default format")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("name,cls", NORMALISED)
def test_normalised_every_dtype_class_and_format(name, cls, dtype):
    cs = G.case(name)
    for f in cs[4]:
        want = kit_gpu.convert(_bytes(name, f), dtype, True)
        for fmt in FORMATS:
            y = aa.resize_many_to_float(_inputs(name, cls), list(cs[2]), MODE[f], boxes=_boxes(name), out_dtype=dtype, out_format=fmt,
                                        **_norm(cs[1]))
            _assert_format(y, fmt, cs[1])
            kit_gpu.assert_bits(y, want, f"{name}/{f}/{cls}/{fmt}/{dtype}")
    # without mean / std the 16-bit types are the byte, converted
    f = cs[4][0]
    y = aa.resize_many_to_float(_inputs(name, cls), list(cs[2]), MODE[f], boxes=_boxes(name), out_dtype=dtype, out_format="nchw")
    kit_gpu.assert_bits(y, kit_gpu.convert(_bytes(name, f), dtype, False), f"{name}/{f}/{cls}/no normalisation/{dtype}")


@pytest.mark.parametrize("cls", ["interleaved", "planar"])
@pytest.mark.parametrize("name,f,flips", [("m_mixed", "cubic", [True, False] * 4 + [True]), ("m_mixed", "linear", [False, True] * 4 + [False]),
                                           ("m_strips", "hamming", [True, False]), ("m_strips", "hamming", [False, True])])
def test_flips_mirror_the_flagged_items_and_leave_the_others(name, f, flips, cls):
    cs = G.case(name)
    for dtype in DTYPES:
        plain = kit_gpu.convert(_bytes(name, f), dtype, True)
        want = kit_gpu.convert(_bytes(name, f), dtype, True, flips)
        for i, fl in enumerate(flips):  # (what the expectation itself says: flagged items mirrored, the others untouched)
            assert torch.equal(kit_gpu.bits(want[i]), kit_gpu.bits(plain[i].flip(-1) if fl else plain[i]))
        for fmt in FORMATS:
            y = aa.resize_many_to_float(_inputs(name, cls), list(cs[2]), MODE[f], boxes=_boxes(name), flips=flips, out_dtype=dtype,
                                        out_format=fmt, **_norm(cs[1]))
            _assert_format(y, fmt, cs[1])
            kit_gpu.assert_bits(y, want, f"{name}/{f}/{cls}/{fmt}/{dtype}/flips")
    # truthy / falsy entries of any kind
    y = aa.resize_many_to_float(_inputs(name, cls), list(cs[2]), MODE[f], boxes=_boxes(name), flips=[int(v) for v in flips],
                                out_dtype=torch.bfloat16, out_format="nchw", **_norm(cs[1]))
    kit_gpu.assert_bits(y, kit_gpu.convert(_bytes(name, f), torch.bfloat16, True, flips), f"{name}/{f}/{cls}/int flips")


def _adhoc(c, sizes, cls, seed):
    rng = np.random.default_rng(seed)
    return [kit_gpu.to_gpu(rng.integers(0, 256, (c, h, w), dtype=np.uint8), cls) for h, w in sizes]


def _adhoc_restated(imgs, size, f, boxes=None):
    """Pillow's bytes of ad-hoc images from the CPU restatement: [N, C, oH, oW] uint8 on the CPU."""
    boxes = boxes if boxes is not None else [None] * len(imgs)
    return torch.from_numpy(np.stack([G._br.resize_box_restated(f, np.ascontiguousarray(t.permute(1, 2, 0).cpu().numpy()), size[0], size[1], b)
                                      .transpose(2, 0, 1) for t, b in zip(imgs, boxes)]))


@pytest.mark.parametrize("ow", [1, 2])
def test_flips_of_outputs_one_and_two_columns_wide(ow):
    imgs = _adhoc(3, [(23, 31), (9, 5), (40, 2)], "interleaved", 100 + ow)
    boxes = [None, (0.5, 1.0, 4.25, 8.0), None]
    flips = [True, False, True]
    u = aa.resize_many(imgs, [7, ow], "bicubic", boxes=boxes).cpu()
    assert torch.equal(u, _adhoc_restated(imgs, (7, ow), "cubic", boxes))  # (what is converted below is Pillow's, not the package's own)
    y = aa.resize_many_to_float(imgs, [7, ow], "bicubic", boxes=boxes, flips=flips, out_dtype=torch.bfloat16, out_format="nchw", **_norm(3))
    assert y.is_contiguous()
    kit_gpu.assert_bits(y, kit_gpu.convert(u, torch.bfloat16, True, flips), f"ow = {ow}")


# Rows longer than one workgroup's piece of the converting pass (1024 / 512 / 256 / 256 pixels for 1 / 2 / 3 / 4 bytes per pixel), the last
# piece ragged, odd widths (rows of 16-bit elements that start 2-byte aligned only), flipped and not.
@pytest.mark.parametrize("c,cls,ow", [(3, "interleaved", 301), (3, "interleaved", 513), (4, "interleaved", 259), (2, "interleaved", 515),
                                      (2, "planar", 1031), (1, "planar", 1027)])
def test_rows_of_several_pieces(c, cls, ow):
    imgs = _adhoc(c, [(5, 400), (4, 37)], cls, 200 + ow)
    flips = [True, False]
    u = aa.resize_many(imgs, [3, ow], "bilinear").cpu()
    assert torch.equal(u, _adhoc_restated(imgs, (3, ow), "linear"))  # (what is converted below is Pillow's, not the package's own)
    for dtype in DTYPES:
        want = kit_gpu.convert(u, dtype, True, flips)
        for fmt in FORMATS:
            y = aa.resize_many_to_float(imgs, [3, ow], "bilinear", flips=flips, out_dtype=dtype, out_format=fmt, **_norm(c))
            _assert_format(y, fmt, c)
            kit_gpu.assert_bits(y, want, f"C = {c}/{cls}/ow = {ow}/{fmt}/{dtype}")


@pytest.mark.parametrize("cls", ["interleaved", "planar"])
@pytest.mark.parametrize("name", ["m_mixed", "m_c4"])
def test_crops_at_odd_offsets_and_pitches_equal_the_dense_call(name, cls):
    cs = G.case(name)
    crops = [kit_gpu.pitched_crop(ref.item(name, i), cls, i) for i in range(len(cs[3]))]
    flips = [i % 3 == 0 for i in range(len(cs[3]))]
    for f in cs[4]:
        kw = dict(boxes=_boxes(name), flips=flips, out_dtype=torch.float16, out_format="nchw", **_norm(cs[1]))
        y = aa.resize_many_to_float(crops, list(cs[2]), MODE[f], **kw)
        dense = aa.resize_many_to_float(_inputs(name, cls), list(cs[2]), MODE[f], **kw)
        assert y.stride() == dense.stride() and torch.equal(kit_gpu.bits(y), kit_gpu.bits(dense))
        kit_gpu.assert_bits(y, kit_gpu.convert(_bytes(name, f), torch.float16, True, flips), f"{name}/{f}/{cls}/crops")


def test_c_abi_output_that_is_only_two_byte_aligned():
    """float16, odd oW, interleaved -> nchw, out_dev = a buffer's address + 2: the same elements as the aligned call, and the elements
    before and after the output region keep their sentinel."""
    name, f = "m_mixed", "cubic"
    cs = G.case(name)
    imgs, boxes = _inputs(name, "interleaved"), _boxes(name)
    n, c, (oh, ow) = len(imgs), cs[1], cs[2]
    assert ow % 2 == 1
    flips = [i % 2 == 1 for i in range(n)]
    aligned = aa.resize_many_to_float(imgs, [oh, ow], MODE[f], boxes=boxes, flips=flips, out_dtype=torch.float16, out_format="nchw", **_norm(c))
    L = _lib.load()
    recs = (_lib.ManyImage * n)()
    for i, t in enumerate(imgs):
        r = recs[i]
        r.data_dev, r.H, r.W = t.data_ptr(), int(t.shape[1]), int(t.shape[2])
        r.stride_ch, r.stride_row, r.stride_px = 1, t.stride(1), c
        if boxes[i] is not None:
            r.has_box = 1
            for q in range(4):
                r.box[q] = boxes[i][q]
        r.flags = _lib.MANY_FLIP_X if flips[i] else 0
    desc_bytes = L.aa_many_desc_bytes(n)
    desc_host = torch.empty(desc_bytes, dtype=torch.uint8)
    ws_bytes = ctypes.c_size_t(0)
    assert L.aa_many_plan(_lib.FILTER_IDS[MODE[f]], _lib.NHWC, n, c, oh, ow, recs, desc_host.data_ptr(), desc_bytes, ctypes.byref(ws_bytes)) == 0
    desc_dev = desc_host.cuda()
    ws = torch.empty(max(ws_bytes.value, 16), dtype=torch.uint8, device="cuda")
    numel = n * c * oh * ow
    sentinel = -1234.0
    buf = torch.full((1 + numel + 7,), sentinel, dtype=torch.float16, device="cuda")
    out_ptr = buf.data_ptr() + 2
    assert out_ptr % 4 == 2
    cv = _lib.Convert()
    cv.out_layout, cv.normalize, cv.flags = _lib.NCHW, 1, _lib.FLAG_OUT_F16
    for i in range(c):
        cv.mean[i], cv.std[i] = MEAN[i], STD[i]
    rc = L.aa_resample_many_u8_to_float(desc_host.data_ptr(), desc_dev.data_ptr(), n, c, oh, ow, _lib.NHWC, out_ptr, ws.data_ptr(), ws.numel(),
                                        ctypes.byref(cv), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    got = buf.cpu()
    assert torch.equal(kit_gpu.bits(got[1:1 + numel].view(n, c, oh, ow)), kit_gpu.bits(aligned))
    assert (got[:1] == sentinel).all() and (got[1 + numel:] == sentinel).all()
    kit_gpu.assert_bits(aligned, kit_gpu.convert(_bytes(name, f), torch.float16, True, flips), "the aligned call")


def _strips_call(imgs, **kw):
    return aa.resize_many_to_float(imgs, [4, 130], "hamming", boxes=_boxes("m_strips"), flips=[True, False], out_dtype=torch.bfloat16,
                                   out_format="nchw", **_norm(3), **kw)


def _strips_want():
    return kit_gpu.convert(_bytes("m_strips", "hamming"), torch.bfloat16, True, [True, False])


def test_non_default_stream():
    imgs = _inputs("m_strips", "interleaved")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        y = _strips_call(imgs)
    s.synchronize()
    kit_gpu.assert_bits(y, _strips_want(), "non-default stream")


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_non_current_device():
    imgs = [t.to("cuda:1") for t in _inputs("m_strips", "interleaved")]
    assert torch.cuda.current_device() == 0
    y = _strips_call(imgs)
    assert y.device == imgs[0].device and torch.cuda.current_device() == 0
    torch.cuda.synchronize(1)
    kit_gpu.assert_bits(y, _strips_want(), "non-current device")


def test_torch_op():
    name = "m_c2"
    imgs, boxes = _inputs(name, "interleaved"), _boxes(name)
    flat = []
    for t, b in zip(imgs, boxes):
        flat += [float(v) for v in (b if b is not None else (0, 0, t.shape[2], t.shape[1]))]
    flips = [False, True, True]
    y = torch.ops.extension_interpolate.resize_many_to_float(imgs, [19, 77], "bicubic", flat, flips, torch.bfloat16, "nchw", MEAN[:2], STD[:2])
    assert y.is_contiguous()
    kit_gpu.assert_bits(y, kit_gpu.convert(_bytes(name, "cubic"), torch.bfloat16, True, flips), "the torch op")
    y = torch.ops.extension_interpolate.resize_many_to_float(imgs, [19, 77], "bicubic", flat)
    assert y.dtype == torch.float32 and y.is_contiguous(memory_format=torch.channels_last)
    kit_gpu.assert_bits(y, kit_gpu.convert(_bytes(name, "cubic"), torch.float32, False), "the torch op, defaults")


def test_a_mixed_list_copies_the_minority():
    name = "m_c4"
    inter, planar = _inputs(name, "interleaved"), _inputs(name, "planar")
    flips = [True, False, True]
    want = kit_gpu.convert(_bytes(name, "cubic"), torch.float16, True, flips)
    kw = dict(boxes=_boxes(name), flips=flips, out_dtype=torch.float16, **_norm(4))
    y = aa.resize_many_to_float([inter[0], planar[1], inter[2]], [19, 77], "bicubic", **kw)
    assert y.is_contiguous(memory_format=torch.channels_last)  # (out_format None: the class of the call)
    kit_gpu.assert_bits(y, want, "two interleaved, one planar")
    y = aa.resize_many_to_float([planar[0], inter[1], planar[2]], [19, 77], "bicubic", **kw)
    assert y.is_contiguous()
    kit_gpu.assert_bits(y, want, "two planar, one interleaved")
    y = aa.resize_many_to_float([planar[0], inter[1], planar[2]], [19, 77], "bicubic", out_format="nhwc", **kw)
    assert y.is_contiguous(memory_format=torch.channels_last)
    kit_gpu.assert_bits(y, want, "two planar, one interleaved, nhwc")


def test_permuting_the_items_permutes_the_output():
    name, f = "m_mixed", "lanczos"
    imgs, boxes = _inputs(name, "interleaved"), _boxes(name)
    perm = [4, 8, 0, 6, 2, 7, 1, 5, 3]
    flips = [i % 2 == 0 for i in range(9)]
    yp = aa.resize_many_to_float([imgs[p] for p in perm], [30, 45], MODE[f], boxes=[boxes[p] for p in perm], flips=[flips[p] for p in perm],
                                 out_dtype=torch.bfloat16, out_format="nchw", **_norm(3))
    kit_gpu.assert_bits(yp, kit_gpu.convert(_bytes(name, f), torch.bfloat16, True, flips)[perm], "permuted items")


def test_empty_batch_and_no_cache_is_read_or_written():
    for dtype in DTYPES:
        e = aa.resize_many_to_float([], [30, 45], channels=3, out_dtype=dtype)
        assert tuple(e.shape) == (0, 3, 30, 45) and e.dtype == dtype and e.is_cuda
        e = aa.resize_many_to_float(_inputs("m_batchbox", "planar")[:0], [30, 45], out_dtype=dtype, flips=[], **_norm(3))
        assert tuple(e.shape) == (0, 3, 30, 45) and e.dtype == dtype and e.is_cuda
    before = (len(tables._cache), len(tables._box_cache), len(aa._plans))
    y = aa.resize_many_to_float(_inputs("m_mixed", "interleaved"), [30, 45], "bicubic", boxes=_boxes("m_mixed"), out_dtype=torch.bfloat16,
                                out_format="nchw", **_norm(3))
    torch.cuda.synchronize()
    assert (len(tables._cache), len(tables._box_cache), len(aa._plans)) == before
    kit_gpu.assert_bits(y, kit_gpu.convert(_bytes("m_mixed", "cubic"), torch.bfloat16, True), "m_mixed/cubic")
