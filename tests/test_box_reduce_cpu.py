"""Image.reduce, Image.resize(box=...) and Image.resize(reducing_gap=...) without a GPU: the numpy restatement against the fixture and
against Pillow where it imports, the package's host arithmetic (boxmath) against Pillow's own Python, and every argument error."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import box_reduce_ref as ref  # noqa: E402

from interpolate_antialiasing_amd import _lib, boxmath  # noqa: E402
from interpolate_antialiasing_amd import extension_interpolate as aa  # noqa: E402
from interpolate_antialiasing_amd import functional  # noqa: E402

G = ref.gen()
ENTRIES = list(G.entries())


def _pil():
    return pytest.importorskip("PIL.Image")


@pytest.mark.parametrize("kind", ["reduce", "box", "gap"])
def test_restatement_reproduces_the_fixture(kind):
    n = 0
    for key, k, cs, f in ENTRIES:
        if k != kind:
            continue
        x = ref.batch(cs[1], cs[2], cs[3] if k == "reduce" else None)
        ref.assert_matches_fixture(key, x, G.restated(k, cs, f, x))
        n += 1
    assert n > 10


def test_fixture_regenerates_from_pillow():
    _pil()
    results = []
    for key, k, cs, f in ENTRIES:
        x = ref.batch(cs[1], cs[2], cs[3] if k == "reduce" else None)
        results.append((G.crc(x), G.pillow(k, cs, f, x)))
    packed = G.pack(results)
    fx = ref.fixture()
    for name, arr in packed.items():
        assert np.array_equal(arr, fx[name]), name


def test_reduce_mult_and_restatement_equal_pillow_for_every_n():
    """1 x n columns reduced by (1, n), n = 1 .. 4096: one block of n pixels each; channels: noise, all 255, all 0."""
    Image = _pil()
    rng = np.random.default_rng(5)
    for n in range(1, 4097):
        img = np.stack([rng.integers(0, 256, (n, 1), dtype=np.uint8), np.full((n, 1), 255, np.uint8), np.zeros((n, 1), np.uint8)], axis=-1)
        pil = np.asarray(Image.fromarray(img, "RGB").reduce((1, n)))
        mine = G.reduce_restated(img, (1, n))
        assert np.array_equal(mine, pil), n
        assert pil[0, 0, 1] == 255 and pil[0, 0, 2] == 0
        assert G.reduce_mult(n) == int(np.float32(2.0 ** 32) / np.float32(256 * n))


def test_reduce_mult_is_the_identity_for_one_pixel():
    assert G.reduce_mult(1) == 1 << 24
    for n in (1, 2, 3, 7, 63, 150 * 150, 65536):  # 32-bit arithmetic never overflows: (255 n + n / 2) * mult(n) < 2^32
        assert (255 * n + n // 2) * G.reduce_mult(n) < 1 << 32
        assert ((255 * n + n // 2) * G.reduce_mult(n)) >> 24 == 255


def _random_draws(count, seed):
    rng = np.random.default_rng(seed)
    names = ["linear", "cubic", "box", "hamming", "lanczos"]
    for _ in range(count):
        w, h = int(rng.integers(8, 3000)), int(rng.integers(8, 3000))
        ow, oh = int(rng.integers(1, 400)), int(rng.integers(1, 400))
        x0, x1 = sorted(rng.uniform(0, w, 2))
        y0, y1 = sorted(rng.uniform(0, h, 2))
        if rng.random() < 0.3:
            x0, y0, x1, y1 = 0.0, 0.0, float(w), float(h)
        elif rng.random() < 0.3:
            x0, y0, x1, y1 = float(int(x0)), float(int(y0)), float(math.ceil(x1)), float(math.ceil(y1))
        if x1 - x0 < 1 or y1 - y0 < 1:
            continue
        yield w, h, ow, oh, (x0, y0, x1, y1), float(rng.choice([1.0, 1.5, 2.0, 3.0, 4.5])), names[int(rng.integers(0, 5))]


def test_host_arithmetic_matches_pillows_python():
    """boxmath against Image.resize's own reducing_gap code, run on a Pillow image whose reduce and C resize are recorded, not run."""
    Image = _pil()
    flt = {"linear": Image.BILINEAR, "cubic": Image.BICUBIC, "box": Image.BOX, "hamming": Image.HAMMING, "lanczos": Image.LANCZOS}

    class Spy(Image.Image):  # Image.resize's Python with the two calls it makes replaced by recorders
        def load(self):
            return None

        def reduce(self, factor, box=None):
            self.log.append(("reduce", tuple(factor) if not isinstance(factor, int) else (factor, factor), tuple(box)))
            fx, fy = self.log[-1][1]
            out = Spy()
            out.log = self.log
            out._im = _FakeCore(((box[2] - box[0] + fx - 1) // fx, (box[3] - box[1] + fy - 1) // fy), self.log)
            out._mode = "L"
            out._size = out._im.size
            return out

    class _FakeCore:
        def __init__(self, size, log):
            self.size, self.mode, self.log = size, "L", log

        def resize(self, size, resample, box):
            self.log.append(("resize", tuple(size), tuple(box)))
            return _FakeCore(tuple(size), self.log)

    checked = 0
    for w, h, ow, oh, box, gap, name in _random_draws(400, 11):
        log = []
        im = Spy()
        im.log = log
        im._im = _FakeCore((w, h), log)
        im._mode = "L"
        im._size = (w, h)
        im.resize((ow, oh), flt[name], box=box, reducing_gap=gap)  # (a Pillow the recording image no longer fits fails here, loudly)
        if [e[0] for e in log].count("resize") == 2:  # taller than 100 x wide: Pillow swaps its passes there (out of scope)
            continue
        plan = boxmath.reducing_plan(w, h, ow, oh, name, box, gap)
        if plan is None:
            assert [e[0] for e in log] == ["resize"] and log[0][2] == tuple(box)
        else:
            factor, rb, shifted = plan
            assert log[0] == ("reduce", factor, rb), (log, plan)
            assert log[1][0] == "resize" and log[1][2] == shifted, (log, plan)
            assert rb == G.safe_box(w, h, ow, oh, name, box)
        assert boxmath.reducing_factors(box, ow, oh, gap) == G.gap_plan(w, h, ow, oh, name, box, gap)[0]
        checked += 1
    assert checked >= 200


def test_hull_is_the_extent_of_the_restated_windows():
    checked = 0
    for w, h, ow, oh, box, gap, name in _random_draws(300, 12):
        bx = boxmath.box_f32(box)
        for in_size, out, a, b in ((w, ow, bx[0], bx[2]), (h, oh, bx[1], bx[3])):
            if b - a <= 0:
                continue
            _, xmin, xsize, _ = G.box_coeffs(name, in_size, a, b, out)
            assert boxmath.axis_hull(in_size, out, a, b, name) == G.axis_hull_from_coeffs(xmin, xsize) == (int(xmin[0]), int(xmin[-1] + xsize[-1]))
            checked += 1
    assert checked >= 300


def test_box_of_the_whole_axis_is_the_plain_table():
    for name in G.FILTER_NAMES:
        for n_in, n_out in ((131, 40), (97, 97), (50, 120), (2160, 224)):
            k, xmin, xsize, ki = G.box_coeffs(name, n_in, 0.0, float(n_in), n_out)
            if name in ("hamming", "lanczos"):
                k2, xmin2, xsize2, ki2, _ = G._gf.pil_coeffs(name, n_in, n_out)
                assert k == k2 and np.array_equal(xmin, xmin2) and np.array_equal(xsize, xsize2) and np.array_equal(ki, ki2)
            assert boxmath.axis_hull(n_in, n_out, 0.0, float(n_in), name) == (0, n_in)


# ---- argument errors, all before any GPU use (the tensors are on the CPU: reaching the GPU check would raise AAInterpError instead) ------
U8 = torch.zeros((1, 3, 20, 30), dtype=torch.uint8)
FORWARDS = [aa.linear_forward, aa.cubic_forward, aa.nearest_forward, aa.hamming_forward, aa.lanczos_forward]


@pytest.mark.parametrize("fn", FORWARDS)
def test_bad_boxes_have_pillows_wording(fn):
    with pytest.raises(ValueError, match="box offset can't be negative"):
        fn(U8, [10, 10], box=(-1, 0, 20, 20))
    with pytest.raises(ValueError, match="box can't exceed original image size"):
        fn(U8, [10, 10], box=(0, 0, 30.5, 20))
    with pytest.raises(ValueError, match="box can't exceed original image size"):
        fn(U8, [10, 10], box=(0, 0, 30, 21))  # (x first: 30 wide, 20 high)
    with pytest.raises(ValueError, match="box can't be empty"):
        fn(U8, [10, 10], box=(12, 5, 11, 9))
    with pytest.raises(ValueError, match="reducing_gap must be 1.0 or greater"):
        fn(U8, [10, 10], reducing_gap=0.99)
    with pytest.raises(ValueError, match="box can't be empty"):  # not empty in double, empty as the floats Pillow's C takes
        fn(U8, [10, 10], box=(12.0, 5, 12.0 + 1e-9, 9))


@pytest.mark.parametrize("kw", [{"box": (1.5, 2, 20, 18)}, {"reducing_gap": 2.0}])
def test_box_and_gap_are_pillow_uint8_only(kw):
    for fn in FORWARDS:
        with pytest.raises(NotImplementedError):
            fn(torch.zeros((1, 3, 20, 30)), [10, 10], **kw)
        with pytest.raises(NotImplementedError):
            fn(torch.zeros((1, 3, 20, 30), dtype=torch.float16), [10, 10], **kw)
        with pytest.raises(NotImplementedError):
            fn(U8, [10, 10], uint8_mode="harness", **kw)
        with pytest.raises(NotImplementedError):
            fn(U8, [10, 10], out_dtype=torch.float32, **kw)
        with pytest.raises(NotImplementedError):
            fn(U8, [10, 10], out_dtype=torch.float16, uint8_mode="harness", **kw)
    prev = aa.get_uint8_mode()
    aa.set_uint8_mode("harness")
    try:
        with pytest.raises(NotImplementedError):
            aa.linear_forward(U8, [10, 10], **kw)
    finally:
        aa.set_uint8_mode(prev)


def test_gap_with_alpha_is_refused():
    rgba = torch.zeros((1, 4, 20, 30), dtype=torch.uint8)
    with pytest.raises(NotImplementedError, match="reducing_gap"):
        aa.cubic_forward(rgba, [5, 5], alpha=True, reducing_gap=2.0)
    with pytest.raises(NotImplementedError, match="reducing_gap"):
        functional.interpolate_aa(rgba, [5, 5], "bicubic", alpha=True, reducing_gap=2.0)
    with pytest.raises(ValueError, match="box can't be empty"):
        functional.interpolate_aa(rgba, [5, 5], "bicubic", box=(3, 3, 3, 9))


def test_reduce_argument_errors():
    with pytest.raises(ValueError, match="65536"):
        aa.reduce(U8, (257, 256))
    with pytest.raises(ValueError, match="65536"):
        aa.reduce(U8, 257)
    with pytest.raises(ValueError, match="greater than 0"):
        aa.reduce(U8, (0, 2))
    with pytest.raises(ValueError, match="box offset can't be negative"):
        aa.reduce(U8, 2, box=(-1, 0, 10, 10))
    with pytest.raises(ValueError, match="box can't exceed original image size"):
        aa.reduce(U8, 2, box=(0, 0, 31, 20))
    with pytest.raises(ValueError, match="box can't be empty"):
        aa.reduce(U8, 2, box=(5, 5, 5, 10))
    with pytest.raises(ValueError, match="integers"):
        aa.reduce(U8, 2, box=(0.5, 0, 10, 10))
    with pytest.raises(NotImplementedError):
        aa.reduce(torch.zeros((1, 3, 20, 30)), 2)
    with pytest.raises(ValueError, match="alpha=True"):
        aa.reduce(U8, 2, alpha=True)
    with pytest.raises(_lib.AAInterpError, match="ROCm GPU"):  # a valid call reaches the device check, and only then
        aa.reduce(U8, (8, 4), box=(1, 2, 29, 19))


def test_valid_box_call_reaches_the_device_check_only_then():
    with pytest.raises(_lib.AAInterpError, match="ROCm GPU"):
        aa.cubic_forward(U8, [10, 10], box=(1.5, 2, 20, 18))


def test_c_abi_argument_checks_without_a_gpu():
    import ctypes

    L = _lib.load()
    assert L.aa_abi_version() == 3
    for sym in ("aa_reduce_u8", "aa_table_ksize_box", "aa_table_build_bytes_box", "aa_table_build_box", "aa_premultiply_u8", "aa_unpremultiply_u8"):
        assert sym in _lib.EXPORTS and hasattr(L, sym)
    box = (ctypes.c_int64 * 4)(0, 0, 30, 20)
    one = ctypes.c_void_p(16)  # (never dereferenced: the checks come first)
    assert L.aa_reduce_u8(one, one, _lib.NHWC, 1, 3, 20, 30, None, box, 257, 256, None) == -4  # AA_ERR_BAD_SHAPE: fx * fy > 65536
    assert L.aa_reduce_u8(one, one, _lib.NHWC, 1, 5, 20, 30, None, box, 2, 2, None) == -4  # interleaved C > 4
    assert L.aa_reduce_u8(one, one, _lib.NHWC, 1, 3, 20, 30, None, (ctypes.c_int64 * 4)(0, 0, 31, 20), 2, 2, None) == -4
    assert L.aa_reduce_u8(one, one, _lib.NCHW, 0, 3, 20, 30, None, box, 2, 2, None) == 0  # an empty batch launches nothing
    # box tables: Pillow arithmetic only; ksize from the float difference of the box
    assert L.aa_table_ksize_box(_lib.FILTER_CUBIC, _lib.TABLE_F32, 100, 30, 10.0, 100.0) == _lib.ERR_BAD_DTYPE
    assert L.aa_table_ksize_box(_lib.FILTER_CUBIC, _lib.TABLE_PIL, 100, 30, 10.0, 10.0) == -4
    for name, fid in (("linear", _lib.FILTER_LINEAR), ("cubic", _lib.FILTER_CUBIC), ("box", _lib.FILTER_BOX), ("hamming", _lib.FILTER_HAMMING),
                      ("lanczos", _lib.FILTER_LANCZOS)):
        for a, b, out in ((10.3, 120.9, 40), (0.5, 130.5, 131), (10, 70.5, 61), (50.5, 1650.5, 20)):
            a, b = boxmath.f32(a), boxmath.f32(b)
            assert L.aa_table_ksize_box(fid, _lib.TABLE_PIL, 131, out, a, b) == G.box_coeffs(name, 2000, a, b, out)[0]
        assert L.aa_table_ksize_box(fid, _lib.TABLE_PIL, 131, 40, 0.0, 131.0) == L.aa_table_ksize(fid, _lib.TABLE_PIL, 131, 40, 0, 0.0)
        assert L.aa_table_build_bytes_box(fid, _lib.TABLE_PIL, 131, 40, 0.0, 131.0) == L.aa_table_build_bytes(fid, _lib.TABLE_PIL, 131, 40, 0, 0.0)


def test_reduce_op_has_a_meta_implementation():
    x = torch.empty((2, 3, 37, 53), dtype=torch.uint8, device="meta")
    assert tuple(torch.ops.extension_interpolate.reduce(x, [8, 4]).shape) == (2, 3, 10, 7)
    assert tuple(torch.ops.extension_interpolate.reduce(x, [3, 5], [5, 7, 50, 36]).shape) == (2, 3, 6, 15)
    y = torch.ops.extension_interpolate.reduce(x.to(memory_format=torch.channels_last), [2, 2])
    assert y.is_contiguous(memory_format=torch.channels_last) and y.dtype == torch.uint8
