"""Straight-alpha (RGBA / LA) resizing on the GPU (-m gpu): bit-exact parity with PIL.Image.resize on every route (with the variant each
route takes), every (colour, alpha) pair through the fused kernel, fused against the three-step fallback, strided views, a batch, and
alpha=False unchanged.  Expected values come from tests/golden/alpha.npz (made by tests/golden/make_golden_alpha.py with Pillow)."""
import numpy as np
import pytest
import torch

import kit_golden
import kit_gpu

pytestmark = pytest.mark.gpu

FUSED = ("fused_u8_nhwc_pil_alpha_v3", "fused_u8_nhwc_pil_alpha6_v3")
FALLBACK = "alpha_3step"


M = kit_golden.generator("alpha")
aa = kit_gpu.aa_fixture()


@pytest.fixture(scope="module")
def fx():
    return kit_golden.fixture("alpha")


def _op(aa, name):
    return {"nearest": aa.nearest_forward, "linear": aa.linear_forward, "cubic": aa.cubic_forward, "hamming": aa.hamming_forward,
            "lanczos": aa.lanczos_forward}[name]


# routes of channels_last RGBA cases that follow from their window widths and open output rows (the other cases take either)
KNOWN_ROUTES = {("headline_196x320", "linear"): FUSED[0], ("headline_196x320", "nearest"): FUSED[0], ("half_64x80", "linear"): FUSED[0],
                ("six_80x100", "lanczos"): FUSED[1], ("six_80x100", "hamming"): FUSED[0]}
KNOWN_FALLBACK = ("wide_40x48", "split_16x20", "up_90x45")  # 17+ taps, split windows, growing heights


@pytest.mark.parametrize("name", M.FILTERS)
def test_pillow_parity_every_case(aa, fx, name):
    from interpolate_antialiasing_amd import _lib

    routes = {}
    for case, (h, w), (oh, ow), chans, seed in M.CASES:
        for c in chans:
            img = M.make_image(h, w, c, seed)
            in_crc, exp_crc, exp_samples = M.expected(fx, case, c, name)
            assert M.crc(img) == in_crc, ("fixture input generator changed", case, c)
            for channels_last in (True, False):
                _lib.load().aa_set_fused(1)
                y = _op(aa, name)(kit_gpu.image_gpu(img, channels_last), [oh, ow], alpha=True)
                torch.cuda.synchronize()
                variant = _lib.last_variant()
                got = kit_gpu.hwc(y[0])
                tag = (case, c, name, "nhwc" if channels_last else "nchw", variant)
                if M.crc(got) != exp_crc:
                    pix = M.sample_pixels(oh, ow)
                    diff = np.abs(got.reshape(-1, c)[pix].astype(int) - exp_samples.astype(int))
                    pytest.fail(f"{tag}: output differs from Pillow (max abs error over samples {diff.max()})")
                if (h, w) == (oh, ow):
                    continue  # (a copy; no kernel)
                if c == 4 and channels_last:
                    assert variant in FUSED + (FALLBACK,), tag
                    if (case, name) in KNOWN_ROUTES:
                        assert variant == KNOWN_ROUTES[(case, name)], tag
                    if case in KNOWN_FALLBACK:
                        assert variant == FALLBACK, tag
                else:
                    assert variant == FALLBACK, tag
                routes[tag[:4]] = variant
    assert any(v in FUSED for v in routes.values()) and any(v == FALLBACK for v in routes.values())
    print(name, sorted(routes.items()))


def test_every_colour_alpha_pair_through_the_fused_kernel(aa, fx):
    """A 512x512 RGBA image of constant 2x2 blocks, block (i, j) = colour i (three variations), alpha j, box-filtered to 256x256: the box
    filter is exact on constant blocks, so every output pixel is unpremul(premul(c, a), a) — all 65 536 pairs."""
    from interpolate_antialiasing_amd import _lib

    c = np.arange(256, dtype=np.uint8)[:, None] * np.ones((1, 256), np.uint8)
    a = np.ones((256, 1), np.uint8) * np.arange(256, dtype=np.uint8)[None, :]
    small = np.stack([c, 255 - c, c ^ 0x5A, a], axis=-1)
    img = small.repeat(2, axis=0).repeat(2, axis=1)
    y = aa.nearest_forward(kit_gpu.image_gpu(img, True), [256, 256], alpha=True)
    torch.cuda.synchronize()
    assert _lib.last_variant() == FUSED[0]
    got = kit_gpu.hwc(y[0])
    pre, un = fx["premul"].astype(np.int64), fx["unpremul"]
    for ch in range(3):
        exp = un[pre[small[:, :, ch], a], a]
        assert np.array_equal(got[:, :, ch], exp), (ch, np.argwhere(got[:, :, ch] != exp)[:5])
    assert np.array_equal(got[:, :, 3], a)


def _rand_rgba(rng, n, h, w, c=4):
    x = rng.integers(0, 256, (n, h, w, c), dtype=np.uint8)
    a = x[..., -1]
    a[rng.random((n, h, w)) < 0.3] = 0
    a[rng.random((n, h, w)) < 0.3] = 255
    return x


def test_fused_equals_fallback(aa):
    from interpolate_antialiasing_amd import _lib

    rng = np.random.default_rng(11)
    seen = set()
    for i in range(24):
        h, w = int(rng.integers(8, 300)), int(rng.integers(8, 300))
        oh, ow = int(rng.integers(2, h + 1)), int(rng.integers(2, w + 1))
        if (oh, ow) == (h, w):
            continue
        name = M.FILTERS[i % len(M.FILTERS)]
        x = torch.from_numpy(_rand_rgba(rng, 2, h, w)).cuda().permute(0, 3, 1, 2)
        prev = _lib.set_fused(1)
        try:
            y1 = _op(aa, name)(x, [oh, ow], alpha=True)
            v1 = _lib.last_variant()
            _lib.set_fused(0)
            y0 = _op(aa, name)(x, [oh, ow], alpha=True)
            v0 = _lib.last_variant()
        finally:
            _lib.set_fused(prev)
        assert v0 == FALLBACK, (name, h, w, oh, ow, v0)
        assert torch.equal(y1, y0), (name, h, w, oh, ow, v1)
        seen.add(v1)
    assert seen & set(FUSED), seen


def test_strided_crop_views(aa):
    from interpolate_antialiasing_amd import _lib

    rng = np.random.default_rng(12)
    base = torch.from_numpy(_rand_rgba(rng, 3, 300, 400)).cuda().permute(0, 3, 1, 2)  # channels_last
    for name, (y0, y1, x0, x1), (oh, ow), fused in (("linear", (13, 277, 21, 390), (120, 150), True),
                                                      ("lanczos", (5, 125, 7, 167), (80, 100), True),
                                                      ("cubic", (0, 300, 3, 399), (20, 30), False)):
        view = base[:, :, y0:y1, x0:x1]
        assert not view.is_contiguous(memory_format=torch.channels_last)
        y = _op(aa, name)(view, [oh, ow], alpha=True)
        v = _lib.last_variant()
        exp = _op(aa, name)(view.contiguous(memory_format=torch.channels_last), [oh, ow], alpha=True)
        assert torch.equal(y, exp), (name, v)
        assert (v in FUSED) == fused, (name, v)
    planar = base.contiguous()[1:, :, 10:200, 30:300]  # an NCHW crop: the fallback after a dense copy
    y = aa.linear_forward(planar, [64, 90], alpha=True)
    assert _lib.last_variant() == FALLBACK
    assert torch.equal(y, aa.linear_forward(planar.contiguous(), [64, 90], alpha=True))


def test_batch_of_64(aa, fx):
    from interpolate_antialiasing_amd import _lib

    case, (h, w), (oh, ow), _, seed = M.CASES[1]
    img = M.make_image(h, w, 4, seed)
    imgs = np.stack([np.roll(img, 3 * k, axis=1) for k in range(64)])
    x = torch.from_numpy(imgs).cuda().permute(0, 3, 1, 2)
    y = aa.linear_forward(x, [oh, ow], alpha=True)
    assert _lib.last_variant() == FUSED[0]
    assert M.crc(kit_gpu.hwc(y[0])) == M.expected(fx, case, 4, "linear")[1]
    for k in (1, 17, 40, 63):
        assert torch.equal(y[k:k + 1], aa.linear_forward(x[k:k + 1], [oh, ow], alpha=True)), k


def test_alpha_false_is_unchanged(aa, fx):
    import oracle

    for name in M.FILTERS:
        case, (h, w), (oh, ow), _, seed = M.CASES[0]
        img = M.make_image(h, w, 4, seed)
        x = kit_gpu.image_gpu(img, True)
        y = _op(aa, name)(x, [oh, ow]).cpu().numpy()
        if name in oracle.FILTERS:  # (the oracle restates Pillow's bilinear, bicubic and box filters)
            exp = oracle.pil_resize_u8(name, np.ascontiguousarray(img.transpose(2, 0, 1))[None], (oh, ow), nthreads=4)
            assert np.array_equal(y, exp), name
        for ch in range(4):  # channels stay independent: each equals the channel resized on its own
            one = _op(aa, name)(x[:, ch:ch + 1].contiguous(), [oh, ow]).cpu().numpy()
            assert np.array_equal(y[:, ch:ch + 1], one), (name, ch)
        ya = kit_gpu.hwc(_op(aa, name)(x, [oh, ow], alpha=True)[0])
        assert M.crc(ya) == M.expected(fx, case, 4, name)[1], name
        assert not np.array_equal(ya, kit_gpu.hwc(torch.from_numpy(y)[0])), name
    same = kit_gpu.image_gpu(M.make_image(24, 40, 4, 9), True)
    out = aa.linear_forward(same, [24, 40], alpha=True)
    assert torch.equal(out, same) and out.data_ptr() != same.data_ptr()


def test_fused_byte_stores_and_strided_dense_entry(aa):
    """The C-ABI with an output pointer one byte off a dword: the fused kernel's per-lane byte stores un-premultiply too.  And the strided
    entry point on dense strides without a fused route (LA) answers AA_ERR_STRIDES, as it does for pitched views."""
    import ctypes

    from interpolate_antialiasing_amd import _lib, tables

    rng = np.random.default_rng(13)
    n, h, w, oh, ow = 2, 120, 160, 50, 70
    x = torch.from_numpy(_rand_rgba(rng, n, h, w)).cuda().permute(0, 3, 1, 2)
    exp = aa.linear_forward(x, [oh, ow], alpha=True)
    assert _lib.last_variant() == FUSED[0]
    L = _lib.load()
    th, tw = tables.get_table_pair(_lib.FILTER_LINEAR, _lib.TABLE_PIL, h, oh, w, ow, False, 0.0, 0.0, x.device)
    ah, aw = th.axis(), tw.axis()
    buf = torch.zeros(n * oh * ow * 4 + 1, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    rc = L.aa_resample_fwd_ex(x.data_ptr(), buf.data_ptr() + 1, None, 0, _lib.U8, _lib.NHWC, n, 4, h, w, ctypes.byref(ah), ctypes.byref(aw),
                              _lib.FLAG_PREMUL_ALPHA, stream)
    assert rc == 0, rc
    assert _lib.last_variant() == FUSED[0]
    got = buf[1:].view(n, oh, ow, 4).permute(0, 3, 1, 2)
    assert torch.equal(got, exp)
    assert int(buf[0]) == 0

    la = torch.from_numpy(_rand_rgba(rng, 1, h, w, 2)).cuda().permute(0, 3, 1, 2)
    th, tw = tables.get_table_pair(_lib.FILTER_LINEAR, _lib.TABLE_PIL, h, oh, w, ow, False, 0.0, 0.0, la.device)
    ah, aw = th.axis(), tw.axis()
    out = torch.empty(oh * ow * 2, dtype=torch.uint8, device="cuda")
    strides = (ctypes.c_int64 * 4)(*la.stride())
    rc = L.aa_resample_fwd_strided(la.data_ptr(), out.data_ptr(), _lib.U8, _lib.NHWC, 1, 2, h, w, strides, ctypes.byref(ah), ctypes.byref(aw),
                                   _lib.FLAG_PREMUL_ALPHA, stream)
    assert rc == _lib.ERR_STRIDES, rc
