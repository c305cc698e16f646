"""Hamming and Lanczos (Pillow's other two antialiasing filters): host-side checks that need no GPU."""
import functools
import math

import numpy as np
import pytest
import torch

import kit_golden

# tests/golden/make_golden_filters.py: the Python restatement of Pillow's coefficients (imports numpy and math only)
_restatement = functools.partial(kit_golden.generator, "filters")


def _f32_ksize(support, n_in, n_out, align_corners=False):
    interp_size = int(2 * support)
    if align_corners:
        scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0.0)
    else:
        scale = np.float32(n_in) / np.float32(n_out)
    sup = np.float32((interp_size * 0.5) * float(scale)) if scale >= 1.0 else np.float32(interp_size * 0.5)
    return int(math.ceil(sup)) * 2 + 1


def _f64_ksize(support, n_in, n_out):
    interp_size = int(2 * support)
    scale = n_in / n_out
    sup = (interp_size * 0.5) * scale if scale >= 1.0 else interp_size * 0.5
    return int(math.ceil(np.float32(sup))) * 2 + 1


def _pil_ksize(support, n_in, n_out):
    return int(math.ceil(support * max(n_in / n_out, 1.0))) * 2 + 1


SIZES = [(1, 1), (1, 7), (3, 2), (4, 9), (17, 5), (100, 101), (438, 196), (438, 220), (906, 320), (906, 120), (906, 1200),
         (1000, 999), (1080, 720), (2160, 224), (3840, 224), (40000, 20000)]


@pytest.mark.parametrize("fid,support", [(3, 1.0), (4, 3.0)])
def test_ksize_and_build_bytes_for_new_filters(fid, support):
    """aa_table_ksize / aa_table_build_bytes answer ids 3 (Hamming, support 1) and 4 (Lanczos, support 3) with the formulas of every
    table kind: Pillow's ceil(support * max(scale, 1)) * 2 + 1, the reference's float / double promotions with interp_size = 2 x support."""
    from interpolate_antialiasing_amd import _lib

    L = _lib.load()
    for n_in, n_out in SIZES:
        kp = L.aa_table_ksize(fid, _lib.TABLE_PIL, n_in, n_out, 0, 0.0)
        kf = L.aa_table_ksize(fid, _lib.TABLE_F32, n_in, n_out, 0, 0.0)
        kd = L.aa_table_ksize(fid, _lib.TABLE_F64, n_in, n_out, 0, 0.0)
        assert kp == _pil_ksize(support, n_in, n_out), (n_in, n_out)
        assert kf == _f32_ksize(support, n_in, n_out), (n_in, n_out)
        assert kd == _f64_ksize(support, n_in, n_out), (n_in, n_out)
        if n_out > 1:
            assert L.aa_table_ksize(fid, _lib.TABLE_F32, n_in, n_out, 1, 0.0) == _f32_ksize(support, n_in, n_out, True)
        assert L.aa_table_build_bytes(fid, _lib.TABLE_PIL, n_in, n_out, 0, 0.0) == L.aa_table_bytes(_lib.TABLE_PIL, n_out, kp) + 32 * (n_in + 1)
        assert L.aa_table_build_bytes(fid, _lib.TABLE_F32, n_in, n_out, 0, 0.0) == L.aa_table_bytes(_lib.TABLE_F32, n_out, kf) + 32 * (n_in + 1)
        assert L.aa_table_build_bytes(fid, _lib.TABLE_F64, n_in, n_out, 0, 0.0) == L.aa_table_bytes(_lib.TABLE_F64, n_out, kd) + 64 * (n_in + 1)
    # the restatement the fixture is made with agrees
    m = _restatement()
    name = "hamming" if fid == 3 else "lanczos"
    for n_in, n_out in SIZES[:12]:
        assert m.pil_coeffs(name, n_in, n_out)[0] == L.aa_table_ksize(fid, _lib.TABLE_PIL, n_in, n_out, 0, 0.0)
        assert m.f32_table(name, n_in, n_out)[0] == L.aa_table_ksize(fid, _lib.TABLE_F32, n_in, n_out, 0, 0.0)
        assert m.f64_table(name, n_in, n_out)[0] == L.aa_table_ksize(fid, _lib.TABLE_F64, n_in, n_out, 0, 0.0)


def test_unknown_filter_ids_are_rejected():
    from interpolate_antialiasing_amd import _lib

    L = _lib.load()
    for fid in (5, -1, 100):
        for kind in (_lib.TABLE_PIL, _lib.TABLE_F32, _lib.TABLE_F64):
            assert L.aa_table_ksize(fid, kind, 438, 196, 0, 0.0) == -1  # AA_ERR_BAD_FILTER, never a box-filter fall-through
            assert L.aa_table_build_bytes(fid, kind, 438, 196, 0, 0.0) == 0
        assert L.aa_table_transposed_ksize(fid, _lib.TABLE_F32, 438, 196, 0, 0.0) == -1
    assert L.aa_abi_version() == 3  # additive: the version stays


def test_new_python_surface_without_gpu():
    from interpolate_antialiasing_amd import _lib, tables
    from interpolate_antialiasing_amd import extension_interpolate as aa
    from interpolate_antialiasing_amd.functional import interpolate_aa

    assert (_lib.FILTER_HAMMING, _lib.FILTER_LANCZOS) == (3, 4)
    assert tables.FILTER_IDS["hamming"] == 3 and tables.FILTER_IDS["lanczos"] == 4
    names = ["lanczos_forward", "hamming_forward", "lanczos_backward", "hamming_backward", "lanczos_forward_nd", "hamming_forward_nd",
             "lanczos_backward_nd", "hamming_backward_nd"]
    for n in names:
        assert n in aa.__all__ and callable(getattr(aa, n)), n
    x = torch.zeros(1, 3, 8, 8)
    for fwd in (aa.lanczos_forward, aa.hamming_forward):
        with pytest.raises(_lib.AAInterpError, match="no CPU implementation"):
            fwd(x, [4, 4])
        with pytest.raises(RuntimeError, match="Input and output sizes should be greater than 0"):
            fwd(x, [0, 4])
        with pytest.raises(NotImplementedError, match="not implemented for 'Int'"):
            fwd(x.int(), [4, 4])
        # the same keyword set as linear_forward
        with pytest.raises(_lib.AAInterpError, match="no CPU implementation"):
            fwd(x.to(torch.uint8), [4, 4], uint8_mode="harness", scale_factors=None, precision="exact")
    for bwd in (aa.lanczos_backward, aa.hamming_backward):
        with pytest.raises(_lib.AAInterpError, match="no CPU implementation"):
            bwd(torch.zeros(1, 3, 5, 7), [5, 7], [1, 3, 12, 17])
        with pytest.raises(_lib.AAInterpError, match="no CPU implementation"):
            bwd(torch.zeros(1, 3, 5, 7), [5, 7], [1, 3, 12, 17], atomic=True)
    with pytest.raises(NotImplementedError, match="not implemented for 'Byte'"):
        aa.lanczos_forward_nd(torch.zeros(1, 2, 9, dtype=torch.uint8), [4])
    with pytest.raises(_lib.AAInterpError, match="no CPU implementation"):
        aa.hamming_forward_nd(torch.zeros(1, 2, 9), [4])
    # torch.ops registration with shape inference
    for name in ("lanczos_forward", "hamming_forward", "lanczos_backward", "hamming_backward"):
        assert hasattr(torch.ops.extension_interpolate, name)
    y = torch.ops.extension_interpolate.lanczos_forward(torch.zeros(2, 3, 8, 8, device="meta"), [4, 5], False)
    assert tuple(y.shape) == (2, 3, 4, 5)
    g = torch.ops.extension_interpolate.hamming_backward(torch.zeros(2, 3, 4, 5, device="meta"), [4, 5], [2, 3, 8, 8], False)
    assert tuple(g.shape) == (2, 3, 8, 8)
    # interpolate_aa takes the new modes for 3-, 4- and 5-D inputs: the 4-D op has GPU and Meta kernels only (as for the other modes,
    # the dispatcher refuses a CPU tensor); the N-d front-ends refuse it with the package's own error
    for mode in ("lanczos", "hamming"):
        with pytest.raises(NotImplementedError, match="CPU"):
            interpolate_aa(torch.zeros(1, 3, 8, 8), (4, 4), mode=mode)
        with pytest.raises(_lib.AAInterpError, match="no CPU implementation"):
            interpolate_aa(torch.zeros(1, 3, 8), (4,), mode=mode)
        with pytest.raises(_lib.AAInterpError, match="no CPU implementation"):
            interpolate_aa(torch.zeros(1, 3, 4, 8, 8), (2, 4, 4), mode=mode)
        y = interpolate_aa(torch.zeros(1, 3, 8, 8, device="meta"), (4, 6), mode=mode)
        assert tuple(y.shape) == (1, 3, 4, 6)
    with pytest.raises(ValueError):
        interpolate_aa(torch.zeros(1, 3, 8, 8), (4, 4), mode="sinc")


def _pil_fixed_point(name, n_in, n_out):
    """Vectorised restatement of Pillow's 22-bit coefficients (all rows of one table at once) -> int64 k [out, taps]."""
    sup = {"lanczos": 3.0, "hamming": 1.0}[name]
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = sup * fs
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(n_out) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xsize = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), n_in) - xmin
    x = np.arange(ksize)[None, :]
    t = ((x + xmin[:, None]) - center[:, None] + 0.5) * (1.0 / fs)
    with np.errstate(invalid="ignore", divide="ignore"):
        px = t * np.pi
        sinc = np.where(t == 0, 1.0, np.sin(px) / px)
        if name == "lanczos":
            p3 = (t / 3) * np.pi
            w = np.where((t >= -3) & (t < 3), sinc * np.where(t == 0, 1.0, np.sin(p3) / p3), 0.0)
        else:
            a = np.abs(t) * np.pi
            w = np.where(t == 0, 1.0, np.where(np.abs(t) >= 1, 0.0, np.sin(a) / a * (float(np.float32(0.54)) + float(np.float32(0.46)) * np.cos(a))))
    w = np.where(x < xsize[:, None], w, 0.0)
    ww = w.sum(axis=1, keepdims=True)
    w = np.where(ww != 0, w / np.where(ww != 0, ww, 1.0), w)
    return np.where(w < 0, np.trunc(-0.5 + w * (1 << 22)), np.trunc(0.5 + w * (1 << 22))).astype(np.int64)


def test_lanczos_fixed_point_coefficients_fit_the_kernels():
    """The fused uint8 kernels multiply a byte by a 24-bit signed weight operand and accumulate in int32 from 1 << 21 (Pillow's
    arithmetic): every 22-bit fixed-point Lanczos / Hamming coefficient must stay below 2**23 in magnitude, and 255 * sum|k| + 2**21
    below 2**31.  Scan in 1..120 x out 1..260 (wider than the 1..79 x 1..199 range of the issue's figures: max|k| 1.28, sum 1.57)."""
    m = _restatement()
    for name, n_in, n_out in (("lanczos", 7, 19), ("lanczos", 438, 220), ("hamming", 5, 13), ("hamming", 906, 320)):
        # vectorised vs the scalar restatement (numpy's summation order may move a coefficient by one unit)
        d = _pil_fixed_point(name, n_in, n_out) - m.pil_coeffs(name, n_in, n_out)[3]
        assert np.abs(d).max() <= 1, (name, n_in, n_out)
    worst_k, worst_sum = 0, 0
    for name in ("lanczos", "hamming"):
        for n_in in range(1, 121):
            for n_out in range(1, 261):
                a = np.abs(_pil_fixed_point(name, n_in, n_out))
                worst_k, worst_sum = max(worst_k, int(a.max())), max(worst_sum, int(a.sum(axis=1).max()))
    assert worst_k < (1 << 23), worst_k / (1 << 22)
    assert 255 * worst_sum + (1 << 21) < (1 << 31), worst_sum / (1 << 22)
    assert worst_k / (1 << 22) < 1.3 and worst_sum / (1 << 22) < 1.6  # the observed figures, with their margin


def test_fixture_matches_the_restatement():
    """tests/golden/filters.npz read through its packed-layout readers: tables equal the restated ones, every image and float input
    regenerates to the stored CRC-32, and Pillow's sampled output pixels equal the restated Pillow arithmetic."""
    m = _restatement()
    fx = kit_golden.fixture("filters")
    for name in ("hamming", "lanczos"):
        for n_in, n_out in m.TABLE_PAIRS:
            if n_out > 2000:
                continue  # (the scalar restatement of 40000 -> 20000 takes a while; the GPU test covers it)
            for kind, fn in (("pil", m.pil_coeffs), ("f32", m.f32_table), ("f64", m.f64_table)):
                rows, k, xmin, xsize, w = m.table_expected(fx, name, n_in, n_out, kind)
                ref = fn(name, n_in, n_out)
                assert k == ref[0] and np.array_equal(xmin, ref[1][rows]) and np.array_equal(xsize, ref[2][rows]), (name, n_in, n_out, kind)
                assert np.array_equal(w, ref[3][rows]), (name, n_in, n_out, kind)
    for i, (case, name, shape, osz) in enumerate(m.FLOAT_CASES):
        assert m.crc(m.float_case_input(i)) == int(fx[f"flt_{case}_incrc"]), case
    for case, (h, w), (oh, ow), chans, seed in m.U8_CASES:
        if h * w > 600_000:
            continue  # (large images: the restated resample is slow in numpy; the GPU test checks their CRC-32)
        for c in chans:
            img = m.make_image(h, w, c, seed)
            for name in ("hamming", "lanczos"):
                in_crc, out_crc, sample = m.u8_expected(fx, case, c, name)
                assert m.crc(img) == in_crc, (case, c)
                y = m.pil_resize_restated(name, img, oh, ow)
                assert m.crc(y) == out_crc and np.array_equal(y.reshape(-1, c)[m.sample_pixels(oh, ow)], sample), (case, c, name)
