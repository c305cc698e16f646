"""resize_many_to_patches on the GPU (-m gpu), tolerance 0 everywhere (bit patterns).

Expected values never come from the code under test: the uint8 token matrices are the CPU restatement of every item's own [vh, vw]
resize, cut by the numpy patchify of tests/golden/make_golden_resize_many_patches.py and pinned to Pillow by the fixture (CRC-32 and
samples); normalised values are torch's CPU ``((b.float() - mean) / std).to(dtype)`` of those bytes.  One test compares the call with the
composition through the unchanged resize_many_to_float, and the guard-band test runs it under the guarded allocator of guard_ref.py."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import guard_ref as G  # noqa: E402
import kit_gpu  # noqa: E402
import resize_many_patches_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

CLASSES = ["interleaved", "planar"]
FORMATS = ["cpp", "ppc"]
TAG = {torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32"}
aa = kit_gpu.aa_fixture()


@functools.lru_cache(maxsize=None)
def _images(name, cls):
    """The case's items on the GPU in one layout class: a list, or, for a batch case, one [N, C, H, W] tensor."""
    xs = ref.inputs(name)
    if ref.case(name)[6]:
        t = torch.from_numpy(np.stack(xs)).cuda()
        return t.contiguous(memory_format=torch.channels_last) if cls == "interleaved" else t
    return [kit_gpu.to_gpu(x, cls) for x in xs]


def _call(aa, name, f, cls, **kw):
    cs = ref.case(name)
    return aa.resize_many_to_patches(_images(name, cls), cs[2], ref.MODE[f], sizes=ref.sizes(name), boxes=ref.boxes(name), flips=ref.flips(name), **kw)


def _whole_bytes(y, what):
    """A float32 result of the identity conversion -> its uint8 matrix (every element a whole number in 0..255)."""
    assert y.dtype == torch.float32 and y.is_contiguous(), what
    f = y.cpu()
    b = f.to(torch.uint8)
    assert torch.equal(b.float(), f), (what, "the identity conversion gave values that are not whole bytes")
    return b.numpy()


@functools.lru_cache(maxsize=None)
def _channel_of_column(name, fmt):
    """[D] the channel every column of a token holds: the patchify of an image whose pixel value is its channel index."""
    _, c, (ph, pw), *_ = ref.case(name)
    idx = np.broadcast_to(np.arange(c, dtype=np.uint8), (ph, pw, c))
    return torch.from_numpy(ref.gen().patchify(np.ascontiguousarray(idx), (ph, pw), fmt)[0].astype(np.int64))


def _normalised(name, f, fmt, dtype):
    """torch's CPU conversion of the restated bytes: [sum T_i, D] in `dtype`."""
    c = ref.case(name)[1]
    ch = _channel_of_column(name, fmt)
    mean, std = torch.tensor(ref.MEAN[:c])[ch], torch.tensor(ref.STD[:c])[ch]
    return ((torch.from_numpy(np.array(ref.tokens(name, f, fmt))).float() - mean) / std).to(dtype)


# ---- identity conversion: Pillow's bytes, every case, filter, class and format ------------------------------------------------------------
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("name", ref.names())
def test_identity_conversion_equals_the_fixture(aa, name, cls):
    cs = ref.case(name)
    d = cs[1] * cs[2][0] * cs[2][1]
    for f in cs[3]:
        for fmt in FORMATS:
            y = _call(aa, name, f, cls, patch_format=fmt)
            assert tuple(y.shape) == (sum(ref.token_counts(name)), d), (name, f, fmt, tuple(y.shape))
            ref.assert_matches_fixture(f"{name}/{f}/{fmt}", _whole_bytes(y, (name, f, cls, fmt)))


# ---- normalised, three dtypes, flips, both formats ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=lambda d: TAG[d])
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("name", ["t_vlm", "t_c1", "t_c1_flip", "t_c2", "t_c2_flip", "t_c4", "t_c4_flip"])
def test_normalised_equals_torch_cpu_conversion_of_the_restated_bytes(aa, name, cls, dtype):
    cs = ref.case(name)
    c = cs[1]
    for f in cs[3]:
        for fmt in FORMATS:
            y = _call(aa, name, f, cls, patch_format=fmt, out_dtype=dtype, mean=ref.MEAN[:c], std=ref.STD[:c])
            assert y.is_contiguous()
            kit_gpu.assert_bits(y, _normalised(name, f, fmt, dtype), (name, f, cls, fmt, TAG[dtype]))


# ---- pad_to ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, 3], ids=["L_is_max_T", "L_is_max_T_plus_3"])
@pytest.mark.parametrize("cls", CLASSES)
def test_pad_rows_are_all_zero_bits(aa, cls, extra):
    name = "t_vlm"
    cs = ref.case(name)
    counts = ref.token_counts(name)
    L = max(counts) + extra
    assert (min(L - t for t in counts) == 0) == (extra == 0)  # L = max T: one item has no pad rows
    for f in cs[3]:
        for fmt in FORMATS:
            # identity: the packed rows are the fixture's, the rest zero
            y = _call(aa, name, f, cls, patch_format=fmt, pad_to=L)
            assert tuple(y.shape) == (len(counts), L, 3 * 14 * 14) and y.is_contiguous()
            got = _whole_bytes(y.view(-1, y.shape[-1]), (name, f, cls, fmt, L)).reshape(y.shape)
            ref.assert_matches_fixture(f"{name}/{f}/{fmt}", np.concatenate([got[i, :t] for i, t in enumerate(counts)]))
            # normalised: pad rows are literal zeros (all-zero bits, not (0 - mean) / std and not -0.0)
            for dtype in (torch.float32, torch.bfloat16):
                z = _call(aa, name, f, cls, patch_format=fmt, pad_to=L, out_dtype=dtype, mean=ref.MEAN[:3], std=ref.STD[:3])
                want = torch.zeros((len(counts), L, y.shape[-1]), dtype=dtype)
                packed = _normalised(name, f, fmt, dtype)
                at = 0
                for i, t in enumerate(counts):
                    want[i, :t] = packed[at:at + t]
                    at += t
                kit_gpu.assert_bits(z, want, (name, f, cls, fmt, L, TAG[dtype]))
                for i, t in enumerate(counts):
                    assert int(kit_gpu.bits(z[i, t:]).count_nonzero()) == 0, (name, f, cls, fmt, L, i)


# ---- the call against the composition through the unchanged resize_many_to_float ---------------------------------------------------------------
@pytest.mark.parametrize("cls", CLASSES)
def test_equals_the_composition_through_resize_many_to_float(aa, cls):
    rng = np.random.default_rng(91)
    shapes = [(37, 53), (120, 64), (9, 300), (64, 64), (15, 15)]
    sizes = [(16, 24), (40, 24), (8, 304), (64, 64), (24, 16)]
    boxes = [None, (3.25, 10.5, 60.0, 100.75), None, None, (0, 0, 15, 15)]
    flips = [False, True, True, False, False]
    ph, pw, c = 8, 8, 3
    imgs = [kit_gpu.to_gpu(rng.integers(0, 256, (c, h, w), dtype=np.uint8), cls) for h, w in shapes]
    for mode in ("bicubic", "lanczos"):
        for dtype in (torch.float32, torch.bfloat16):
            rs = [aa.resize_many_to_float([imgs[i]], list(sizes[i]), mode, boxes=[boxes[i]], flips=[flips[i]], out_dtype=dtype, out_format="nchw",
                                          mean=ref.MEAN[:c], std=ref.STD[:c])[0] for i in range(len(imgs))]
            for fmt, perm in (("cpp", (1, 3, 0, 2, 4)), ("ppc", (1, 3, 2, 4, 0))):
                want = torch.cat([r.view(c, vh // ph, ph, vw // pw, pw).permute(*perm).reshape((vh // ph) * (vw // pw), c * ph * pw)
                                  for r, (vh, vw) in zip(rs, sizes)])
                y = aa.resize_many_to_patches(imgs, (ph, pw), mode, sizes=sizes, boxes=boxes, flips=flips, patch_format=fmt, out_dtype=dtype,
                                              mean=ref.MEAN[:c], std=ref.STD[:c])
                kit_gpu.assert_bits(y, want.cpu(), (cls, mode, TAG[dtype], fmt))


# ---- guard band: every output element written, nothing else touched ------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=lambda d: TAG[d])
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("pad", [None, 3], ids=["packed", "padded"])
def test_guard_band(aa, monkeypatch, pad, cls, dtype, lead):
    """t_vlm under the guarded allocator: the output between two 16 KiB guards, at the allocator's alignment (lead 0) and one element
    later (lead 1: a float32 output 4-byte aligned only, a bfloat16 one on an odd element), the workspace and the descriptor's device copy
    guarded too.  No guard byte changes, no output element keeps the fill (NaN), and the values are the expected ones."""
    name = "t_vlm"
    counts = ref.token_counts(name)
    L = None if pad is None else max(counts) + pad
    for f, fmt in (("cubic", "cpp"), ("linear", "ppc")):
        with G.guarded(monkeypatch, lead, 0xFF) as rec:
            y = _call(aa, name, f, cls, patch_format=fmt, pad_to=L, out_dtype=dtype, mean=ref.MEAN[:3], std=ref.STD[:3])
            rec.check()
        assert len(rec.records) == 3 and len(rec.outputs()) == 1  # desc_dev, ws, out
        r = rec.record_of(y)
        assert r is not None and not r.flat and y.data_ptr() % G.ALIGN == (lead * y.element_size()) % G.ALIGN
        assert G.unwritten_float(y) == 0, (name, f, fmt, cls, L, lead, "output elements still hold the fill")
        packed = _normalised(name, f, fmt, dtype)
        want = packed if L is None else torch.from_numpy(ref.padded(kit_gpu.bits(packed).numpy(), counts, L)).view(dtype)
        kit_gpu.assert_bits(y, want, (name, f, fmt, cls, L, lead))


# ---- the torch op ---------------------------------------------------------------------------------------------------------------------------
def test_torch_op_equals_the_python_call(aa):
    name, f = "t_vlm", "cubic"
    imgs = _images(name, "interleaved")
    flat_sizes = [v for s in ref.sizes(name) for v in s]
    flat_boxes = [float(v) for (h, w, bx, *_r) in ref.case(name)[4] for v in (bx if bx is not None else (0, 0, w, h))]
    op = torch.ops.extension_interpolate.resize_many_to_patches
    for fmt, pad, dtype in (("cpp", None, None), ("ppc", max(ref.token_counts(name)) + 1, torch.bfloat16)):
        y = op(imgs, [14, 14], ref.MODE[f], flat_sizes, flat_boxes, ref.flips(name), fmt, pad, dtype, ref.MEAN[:3], ref.STD[:3])
        want = _call(aa, name, f, "interleaved", patch_format=fmt, pad_to=pad, out_dtype=dtype or torch.float32, mean=ref.MEAN[:3], std=ref.STD[:3])
        kit_gpu.assert_bits(y, want.cpu(), (fmt, pad, dtype))
