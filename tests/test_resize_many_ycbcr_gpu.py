"""resize_many_ycbcr on the GPU, everything by bits (torch.equal): every fixture case against Pillow's bytes and the numpy restatement, the
float outputs against the uint8 result followed by torch's conversion on the CPU, the composition (resize_many per plane, then the tables
in torch), interleaved chroma against planes, planes read where they lie, guard bands, the torch op and the launch count.  Reads the
fixture only: neither Pillow nor anything outside the repository."""
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
import resize_many_ycbcr_ref as ref  # noqa: E402

from interpolate_antialiasing_amd import boxmath, tables  # noqa: E402
from interpolate_antialiasing_amd import extension_interpolate as aa  # noqa: E402

pytestmark = pytest.mark.gpu

G = ref.gen()
COMBOS = [tuple(k.split("/")) for k in G.keys()]
MEAN, STD = kit_golden.MEAN[:3], kit_golden.STD[:3]


def _nchw(batch_nhwc):
    """A numpy [N, oh, ow, 3] batch -> the [N, 3, oh, ow] uint8 tensor on the CPU."""
    return torch.from_numpy(np.ascontiguousarray(batch_nhwc.transpose(0, 3, 1, 2)))


@functools.lru_cache(maxsize=None)
def _planes(name):
    """The case's (Y, Cb, Cr) tuples on the GPU (shared between tests, never written)."""
    return tuple(tuple(torch.from_numpy(np.array(p)).cuda() for p in ref.planes(name, i)) for i in range(len(G.CASES[name]["items"])))


def _interleaved(items):
    """(Y, Cb, Cr) tuples -> (Y, CbCr) tuples: one [h, w, 2] tensor per item, Cb first."""
    return [(y, torch.stack([cb, cr], dim=-1).contiguous()) for y, cb, cr in items]


def _call(name, f, images=None, **kw):
    return aa.resize_many_ycbcr(list(images if images is not None else _planes(name)), list(G.CASES[name]["canvas"]), f, **{**ref.call_args(name), **kw})


# ---- every fixture case: Pillow's bytes, and the restatement's --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,f", COMBOS)
def test_fixture_case(name, f):
    """1 x 1 and 2 x 2 luma, a fractional box under all five filters, odd sizes to 65 and 129 columns, a canvas one pixel wider and one
    row higher than a workgroup of the vertical pass, long Lanczos windows on either axis (chroma windows half as long), all four
    subsamplings alone and mixed, placement with overhang on four sides, "center", an item off the canvas, an RGB fill, flips, and the
    case that clamps on both sides."""
    y = _call(name, f)
    assert y.is_contiguous()
    kit_gpu.assert_bits(y, _nchw(ref.expected(name, f)), (name, f, "fixture"))
    kit_gpu.assert_bits(y, _nchw(ref.restate(name, f)), (name, f, "restatement"))


@pytest.mark.parametrize("name,f", [("frac", "lanczos"), ("odd129", "cubic"), ("vwide", "linear"), ("long", "lanczos"), ("mixed", "cubic"),
                                    ("placed", "cubic"), ("center", "linear"), ("clamp", "cubic"), ("tiny", "linear")])
@pytest.mark.parametrize("fmt", ["nchw", "nhwc"])
def test_interleaved_chroma_gives_the_planes_values(name, f, fmt):
    """(Y, CbCr) with one [h, w, 2] tensor, the NV12 arrangement, in both output layouts."""
    y = _call(name, f, images=_interleaved(_planes(name)), out_format=fmt)
    assert y.is_contiguous(memory_format=torch.channels_last if fmt == "nhwc" else torch.contiguous_format)
    kit_gpu.assert_bits(y, _nchw(ref.expected(name, f)), (name, f, fmt))


@pytest.mark.parametrize("name,f", [("odd65", "lanczos"), ("vwide", "linear"), ("placed", "cubic"), ("clamp", "cubic"), ("tiny1", "linear")])
def test_uint8_channels_last(name, f):
    y = _call(name, f, out_format="nhwc")
    assert y.is_contiguous(memory_format=torch.channels_last)
    kit_gpu.assert_bits(y, _nchw(ref.expected(name, f)), (name, f))


# ---- the float outputs -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("fmt", ["nchw", "nhwc"])
@pytest.mark.parametrize("norm", [False, True])
def test_float_outputs_are_the_bytes_converted(dtype, fmt, norm):
    kw = {"mean": MEAN, "std": STD} if norm else {}
    for name, f, il in (("placed", "cubic", False), ("vwide", "linear", True), ("clamp", "cubic", False)):
        images = _interleaved(_planes(name)) if il else None
        u = _call(name, f, images=images)
        y = _call(name, f, images=images, out_dtype=dtype, out_format=fmt, **kw)
        assert y.is_contiguous(memory_format=torch.channels_last if fmt == "nhwc" else torch.contiguous_format)
        kit_gpu.assert_bits(u, _nchw(ref.expected(name, f)), (name, "bytes"))
        kit_gpu.assert_bits(y, kit_gpu.convert(u.cpu(), dtype, norm), (name, dtype, fmt, norm))


# ---- the composition: resize_many per plane, then the tables -----------------------------------------------------------------------------------
def _ragged(seed, n=9):
    """n items of random sizes, subsamplings and boxes: (Y, Cb, Cr) on the GPU, subsamplings, boxes."""
    rng = np.random.default_rng(seed)
    items, subs, boxes = [], [], []
    for i in range(n):
        h, w = int(rng.integers(5, 70)), int(rng.integers(5, 90))
        sub = ("420", "422", "440", "444")[int(rng.integers(0, 4))] if i % 3 == 2 else "420"
        ch, cw = boxmath.chroma_shape(h, w, sub)
        items.append(tuple(torch.from_numpy(rng.integers(0, 256, s, dtype=np.uint8)).cuda() for s in ((h, w), (ch, cw), (ch, cw))))
        subs.append(sub)
        if i % 4 == 3:
            boxes.append(None)
        else:
            x0, y0 = float(rng.uniform(0, w / 3)), float(rng.uniform(0, h / 3))
            boxes.append((x0, y0, float(rng.uniform(x0 + w / 3, w)), float(rng.uniform(y0 + h / 3, h))))
    return items, subs, boxes


@pytest.mark.parametrize("f", ["bilinear", "bicubic", "lanczos"])
def test_composition_of_the_existing_calls(f):
    items, subs, boxes = _ragged(2024)
    out = [21, 34]
    got = aa.resize_many_ycbcr(items, out, f, subsampling=subs, boxes=boxes)
    cboxes = [boxmath.chroma_box(boxes[i], tuple(items[i][0].shape), subs[i]) for i in range(len(items))]
    y = aa.resize_many([it[0][None] for it in items], out, f, boxes=boxes)
    cb = aa.resize_many([it[1][None] for it in items], out, f, boxes=cboxes)
    cr = aa.resize_many([it[2][None] for it in items], out, f, boxes=cboxes)
    t = [torch.tensor(x, dtype=torch.int32, device="cuda") for x in boxmath.ycbcr_rgb_tables()]
    yi, cbi, cri = y[:, 0].int(), cb[:, 0].long(), cr[:, 0].long()
    fl = lambda v: torch.div(v, 64, rounding_mode="floor")  # noqa: E731  (the arithmetic shift by 6)
    want = torch.stack([yi + fl(t[0][cri]), yi + fl(t[1][cbi] + t[2][cri]), yi + fl(t[3][cbi])], dim=1).clamp(0, 255).to(torch.uint8)
    kit_gpu.assert_bits(got, want, f)


# ---- planes read where they lie ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interleaved", [False, True])
def test_planes_at_odd_offsets_and_pitches(interleaved):
    """Views into larger buffers: planes that start on odd bytes, pitches that are no multiple of 4, Cb and Cr with different pitches, and
    a column-strided plane, which the call copies."""
    rng = np.random.default_rng(91)
    ybuf = torch.from_numpy(rng.integers(0, 256, (40, 71), dtype=np.uint8)).cuda()
    cbuf = torch.from_numpy(rng.integers(0, 256, (30, 45), dtype=np.uint8)).cuda()
    cbuf2 = torch.from_numpy(rng.integers(0, 256, (30, 39), dtype=np.uint8)).cuda()
    ibuf = torch.from_numpy(rng.integers(0, 256, (30, 37, 2), dtype=np.uint8)).cuda()
    strided = torch.from_numpy(rng.integers(0, 256, (25, 70), dtype=np.uint8)).cuda()
    ys = [ybuf[1:38, 4:57], ybuf[3:26, 1:32], strided[:, ::2]]  # [37, 53] at byte 75, [23, 31] at byte 214, [25, 35] column-strided
    assert ys[0].data_ptr() % 2 == 1 and ys[1].data_ptr() % 4 == 2 and ys[0].stride(0) == 71 and not ys[2].is_contiguous()
    shapes = [(19, 27), (12, 16), (13, 18)]
    if interleaved:
        cs = [ibuf[1:20, 2:29], ibuf[5:17, 1:17], ibuf[0:26:2, 3:21]]  # pitch 74; the last with a doubled row pitch
        assert cs[0].stride(0) == 74 and all(tuple(c.shape[:2]) == s for c, s in zip(cs, shapes))
        images = [(y, c) for y, c in zip(ys, cs)]
        planes3 = [(y, c[..., 0], c[..., 1]) for y, c in zip(ys, cs)]
    else:
        cbs = [cbuf[2:21, 5:32], cbuf[1:13, 3:19], cbuf[4:17, 0:36:2]]   # pitch 45, odd offsets; the last column-strided
        crs = [cbuf2[0:19, 1:28], cbuf2[7:19, 2:18], cbuf2[9:22, 20:38]]  # another buffer with another pitch (39)
        assert cbs[0].data_ptr() % 2 == 1 and cbs[0].stride(0) == 45 and crs[0].stride(0) == 39 and not cbs[2].is_contiguous()
        images = [(y, cb, cr) for y, cb, cr in zip(ys, cbs, crs)]
        planes3 = images
    kw = dict(boxes=[(3.3, 2.2, 52.9, 36.1), None, (0.5, 1.0, 34.0, 24.5)], sizes=[(20, 30), (18, 25), (22, 22)],
              offsets=[(-3, 2), (1, -4), (0, 3)], fill=(7, 8, 9), flips=[False, True, True])
    got = aa.resize_many_ycbcr(images, [18, 27], "bicubic", **kw)
    dense = [tuple(p.contiguous() for p in it) for it in planes3]
    kit_gpu.assert_bits(got, aa.resize_many_ycbcr(dense, [18, 27], "bicubic", **kw), "views against dense copies")
    # and against the restatement
    res = [ref.restate_item("cubic", *(p.cpu().numpy() for p in it), "420", kw["boxes"][i], *kw["sizes"][i]) for i, it in enumerate(dense)]
    want = np.empty((3, 18, 27, 3), np.uint8)
    want[:] = np.array(kw["fill"], np.uint8)
    for i, r in enumerate(res):
        (vh, vw), (py, px) = kw["sizes"][i], kw["offsets"][i]
        y0, y1, x0, x1 = max(0, py), min(18, py + vh), max(0, px), min(27, px + vw)
        want[i, y0:y1, x0:x1] = r[y0 - py:y1 - py, x0 - px:x1 - px]
        if kw["flips"][i]:
            want[i] = want[i, :, ::-1]
    kit_gpu.assert_bits(got, _nchw(want), "restatement")


# ---- guard bands -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,f,il", [("placed", "cubic", False), ("placed", "cubic", True), ("vwide", "linear", False), ("odd65", "lanczos", True)])
@pytest.mark.parametrize("out", [(None, "nchw"), (None, "nhwc"), (torch.bfloat16, "nchw"), (torch.float32, "nhwc")])
def test_guard_bands(monkeypatch, name, f, il, out):
    """The output sits in a larger poisoned buffer and the workspace and the descriptor are poisoned: every output element is written
    (two poisons give the same bits) and nothing outside any buffer is touched, also where the output starts one element off its
    natural alignment."""
    images = _interleaved(_planes(name)) if il else None
    outs = []
    for lead, fill in ((0, 0xFF), (1, 0x00)):
        with guard_ref.guarded(monkeypatch, lead=lead, fill=fill) as rec:
            y = _call(name, f, images=images, out_dtype=out[0], out_format=out[1])
            rec.check()
            assert rec.record_of(y) is not None
        outs.append(y)
    kit_gpu.assert_bits(outs[0], outs[1], (name, out))
    want = _nchw(ref.expected(name, f))
    kit_gpu.assert_bits(outs[0], want if out[0] is None else kit_gpu.convert(want, out[0], False), (name, out, "value"))


# ---- the torch op ------------------------------------------------------------------------------------------------------------------------------
def test_the_torch_op_runs_the_call():
    cs = G.CASES["placed"]
    kw = ref.call_args("placed")
    items = _planes("placed")
    flat_boxes = [float(v) for i, b in enumerate(kw["boxes"]) for v in (b or (0, 0, cs["items"][i][1], cs["items"][i][0]))]
    op = torch.ops.extension_interpolate.resize_many_ycbcr
    args = dict(subsampling=",".join(kw["subsampling"]), boxes=flat_boxes, flips=kw["flips"], sizes=[v for s in kw["sizes"] for v in s],
                offsets=[v for o in kw["offsets"] for v in o], fill=list(kw["fill"]))
    y = op([it[0] for it in items], [p for it in items for p in it[1:]], list(cs["canvas"]), "cubic", **args)
    kit_gpu.assert_bits(y, _nchw(ref.expected("placed", "cubic")), "op, planes")
    y = op([it[0] for it in items], [c for _, c in _interleaved(items)], list(cs["canvas"]), "cubic", out_dtype=torch.float16, out_format="nhwc", **args)
    assert y.is_contiguous(memory_format=torch.channels_last)
    kit_gpu.assert_bits(y, kit_gpu.convert(_nchw(ref.expected("placed", "cubic")), torch.float16, False), "op, interleaved")
    meta = op([it[0].to("meta") for it in items], [p.to("meta") for it in items for p in it[1:]], list(cs["canvas"]), "cubic", **args)
    assert tuple(meta.shape) == tuple(y.shape) and meta.dtype == torch.uint8 and meta.device.type == "meta"


# ---- the call's promises -----------------------------------------------------------------------------------------------------------------------
def test_three_launches_planar_and_five_interleaved_whatever_n():
    """What csrc/aa_many_ycbcr.hip's header documents: tables + horizontal pass over all planes + the converting vertical pass; luma and
    chroma pairs have the first two each when the chroma is interleaved."""
    items = list(_planes("mixed"))
    kw = ref.call_args("mixed")
    sub = lambda k: {**kw, "subsampling": kw["subsampling"][:k], "boxes": kw["boxes"][:k]}  # noqa: E731
    for k in (1, 5):
        for images, want in ((items[:k], [1, 1, 1]), (_interleaved(items[:k]), [2, 2, 1])):
            fn = lambda: aa.resize_many_ycbcr(images, [13, 19], "cubic", out_dtype=torch.bfloat16, mean=MEAN, std=STD, **sub(k))  # noqa: E731
            fn()  # (module load and allocator warm-up stay outside the count)
            names = kit_gpu.count_launches(fn)
            assert len(names) == sum(want), (k, names)
            assert [sum(1 for nm in names if part in nm) for part in ("many_tables", "many_hpass", "ycc_vpass")] == want, (k, names)


def test_no_cache_is_read_or_written_and_a_side_stream_is_served():
    before = (len(tables._cache), len(tables._box_cache), len(aa._plans))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        y = _call("center", "linear")
    s.synchronize()
    assert (len(tables._cache), len(tables._box_cache), len(aa._plans)) == before
    kit_gpu.assert_bits(y, _nchw(ref.expected("center", "linear")), "side stream")
