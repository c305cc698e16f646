"""Hamming and Lanczos on the GPU (-m gpu): weight tables, Pillow parity of the uint8 kernels on every route (with the variant each
shape takes), the harness / float32-output modes, float dtypes, the adjoint, the N-d front-ends.  Expected values come from
tests/golden/filters.npz (made by tests/golden/make_golden_filters.py with Pillow)."""
import numpy as np
import pytest
import torch

import kit_golden
import kit_gpu

pytestmark = pytest.mark.gpu

FILTER_NAMES = ("hamming", "lanczos")


M = kit_golden.generator("filters")
aa = kit_gpu.aa_fixture()


@pytest.fixture(scope="module")
def fx():
    return kit_golden.fixture("filters")


def _fwd(aa, name):
    return {"hamming": aa.hamming_forward, "lanczos": aa.lanczos_forward}[name]


def _fid(name):
    from interpolate_antialiasing_amd import _lib

    return {"hamming": _lib.FILTER_HAMMING, "lanczos": _lib.FILTER_LANCZOS}[name]


def _close_ulps(got, exp, ulps):
    """|got - exp| <= ulps units in the last place of the larger magnitude; weights below 1e-12 (the sinc's zeros at integer offsets,
    where two libms may disagree on a residue of ~1e-17) are compared absolutely."""
    got = got.astype(exp.dtype)
    mag = np.maximum(np.abs(got), np.abs(exp))
    tol = np.maximum(ulps * np.spacing(mag), 1e-12)
    return bool(np.all(np.abs(got - exp) <= tol))


def _float_in(fx, i):
    """Input of the float case M.FLOAT_CASES[i], regenerated from its seed and checked against the fixture's CRC-32."""
    x = M.float_case_input(i)
    assert M.crc(x) == int(fx[f"flt_{M.FLOAT_CASES[i][0]}_incrc"]), ("fixture input generator changed", M.FLOAT_CASES[i][0])
    return x


# ------------------------------------------------------------------------------------------------ tables
def _check_table(t, fx, name, n_in, n_out, kind_name, what):
    rows, k, exp_xmin, exp_xsize, exp = M.table_expected(fx, name, n_in, n_out, kind_name)
    xmin, xsize, w = t.unpack()
    tag = (name, n_in, n_out)
    assert t.ksize == k, (what, tag, kind_name)
    assert np.array_equal(xmin[rows], exp_xmin), (what, tag, kind_name)
    assert np.array_equal(xsize[rows], exp_xsize), (what, tag, kind_name)
    if kind_name == "pil":
        assert np.array_equal(w[rows], exp), (what, tag, "pil", np.argwhere(w[rows] != exp)[:5])
    else:
        assert _close_ulps(w[rows], exp, 1 if kind_name == "f32" else 2), (what, tag, kind_name, np.abs(w[rows] - exp).max())


def test_device_tables_match_fixture(aa, fx):
    """Every table kind, every fixture pair, through the single-workgroup build (and the five-launch path for 40000 -> 20000)."""
    from interpolate_antialiasing_amd import _lib, tables

    kinds = {"pil": _lib.TABLE_PIL, "f32": _lib.TABLE_F32, "f64": _lib.TABLE_F64}
    n = 0
    for name in FILTER_NAMES:
        for n_in, n_out in M.TABLE_PAIRS:
            for kname, kind in kinds.items():
                t = tables.build_table(_fid(name), kind, n_in, n_out, False, 0.0, torch.device("cuda"))
                _check_table(t, fx, name, n_in, n_out, kname, "build_table")
                n += 1
    assert n == 2 * len(M.TABLE_PAIRS) * 3


def test_device_tables_pair_launch_matches_fixture(aa, fx):
    """The two tables of a call built as one launch (aa_table_build2): the same tables."""
    from interpolate_antialiasing_amd import _lib, tables

    pairs = [((438, 220), (906, 460)), ((1080, 720), (1920, 1280)), ((2160, 224), (64, 200)), ((4, 9), (17, 40)), ((906, 1200), (1000, 999))]
    for name in FILTER_NAMES:
        for kname, kind in (("pil", _lib.TABLE_PIL), ("f32", _lib.TABLE_F32), ("f64", _lib.TABLE_F64)):
            tables.clear_cache()
            for (ih, oh), (iw, ow) in pairs:
                th, tw = tables.get_table_pair(_fid(name), kind, ih, oh, iw, ow, False, 0.0, 0.0, torch.device("cuda"))
                _check_table(th, fx, name, ih, oh, kname, "pair")
                _check_table(tw, fx, name, iw, ow, kname, "pair")
    tables.clear_cache()


# ------------------------------------------------------------------------------------------------ uint8, Pillow arithmetic
def _expected_variant(case, c, planar):
    up = case.startswith("up_")
    if planar or c == 1:
        return "generic_2pass_u8_pil" if up else "fused_u8_planar_pil_v3"  # (planar growing heights beyond 256 columns: two launches)
    return "fused_u8_nhwc_pil_v3"


def _u8_runs():
    for case, (h, w), (oh, ow), chans, seed in M.U8_CASES:
        for c in chans:
            for planar in ((True,) if c == 1 else (False, True)):
                yield case, (h, w), (oh, ow), c, seed, planar


@pytest.mark.parametrize("name", FILTER_NAMES)
def test_u8_pillow_parity_every_route(aa, fx, name):
    """Bit for bit with PIL.Image.resize (CRC-32 of the whole output; sampled rows for the message), channels_last and planar, with the
    variant expected on each shape; the generic two-launch path (set_fused(0)) gives the same bytes."""
    from interpolate_antialiasing_amd import _lib

    f = _fwd(aa, name)
    for case, (h, w), (oh, ow), c, seed, planar in _u8_runs():
        img = M.make_image(h, w, c, seed)
        in_crc, out_crc, sample = M.u8_expected(fx, case, c, name)
        assert M.crc(img) == in_crc, ("fixture image generator changed", case, c)
        x = kit_gpu.image_gpu(img, not planar)
        y = kit_gpu.hwc(f(x, [oh, ow])[0])
        variant = _lib.last_variant()
        assert np.array_equal(y.reshape(-1, c)[M.sample_pixels(oh, ow)], sample), (name, case, c, planar, variant)
        assert M.crc(y) == out_crc, (name, case, c, planar, variant)
        assert variant == _expected_variant(case, c, planar), (name, case, c, planar, variant)
        prev = _lib.set_fused(0)
        try:
            yg = kit_gpu.hwc(f(x, [oh, ow])[0])
            assert _lib.last_variant().startswith("generic"), _lib.last_variant()
        finally:
            _lib.set_fused(prev)
        assert np.array_equal(yg, y), (name, case, c, planar)


@pytest.mark.parametrize("planar", [False, True])
def test_u8_pillow_parity_on_a_crop_view(aa, fx, planar):
    """1080p -> 720p read in place from a crop of a larger tensor (a pitched view): the narrow six-row route, Pillow's bytes."""
    from interpolate_antialiasing_amd import _lib

    img = M.make_image(1080, 1920, 3, 3)
    big = torch.zeros(1, 1100, 1950, 3, dtype=torch.uint8, device="cuda")
    big[0, 7:1087, 13:1933] = torch.from_numpy(img).cuda()
    x = big.permute(0, 3, 1, 2)[:, :, 7:1087, 13:1933]
    if planar:
        x = big.permute(0, 3, 1, 2).contiguous()[:, :, 7:1087, 13:1933]
    assert not x.is_contiguous() and not x.is_contiguous(memory_format=torch.channels_last)
    for name in FILTER_NAMES:
        y = kit_gpu.hwc(_fwd(aa, name)(x, [720, 1280])[0])
        assert M.crc(y) == M.u8_expected(fx, "hd_720x1280", 3, name)[1], (name, planar, _lib.last_variant())
        assert _lib.last_variant() == ("fused_u8_planar_pil_v3" if planar else "fused_u8_nhwc_pil_v3"), _lib.last_variant()


# ------------------------------------------------------------------------------------------------ uint8, float arithmetic
NARROW = [("headline_narrow_220x460", 3, False), ("headline_narrow_220x460", 1, True), ("headline_narrow_220x460", 4, False),
          ("sq_512_384", 3, True), ("hd_720x1280", 3, False), ("wide_196x320", 3, False)]


def test_u8_harness_and_to_f32_lanczos(aa):
    """Harness mode and uint8 -> float32 (+ mean / std): the fused kernels give the generic path's bytes; harness = clamp and truncation
    of the library's own fp32 result on x.float()."""
    from interpolate_antialiasing_amd import _lib

    cases = {cs[0]: cs for cs in M.U8_CASES}
    for case, c, planar in NARROW:
        _, (h, w), (oh, ow), _, seed = cases[case]
        x = kit_gpu.image_gpu(M.make_image(h, w, c, seed), not planar)
        yh = aa.lanczos_forward(x, [oh, ow], uint8_mode="harness")
        vh = _lib.last_variant()
        assert not vh.startswith("generic"), (case, c, planar, vh)
        yf32 = aa.lanczos_forward(x.float(), [oh, ow])
        ref = yf32.clamp(0, 255).to(torch.uint8)
        assert torch.equal(yh, ref), (case, c, planar, vh)
        mean, std = [0.485 * 255, 0.456 * 255, 0.406 * 255, 0.5 * 255][:c], [0.229 * 255, 0.224 * 255, 0.225 * 255, 0.25 * 255][:c]
        yc = aa.lanczos_forward(x, [oh, ow], out_dtype=torch.float32)
        vc = _lib.last_variant()
        assert not vc.startswith("generic"), (case, c, planar, vc)
        assert torch.equal(yc, yf32), (case, c, planar, vc)
        yn = aa.lanczos_forward(x, [oh, ow], out_dtype=torch.float32, mean=mean, std=std)
        prev = _lib.set_fused(0)
        try:
            assert torch.equal(aa.lanczos_forward(x, [oh, ow], uint8_mode="harness"), yh)
            assert _lib.last_variant().startswith("generic"), _lib.last_variant()
            assert torch.equal(aa.lanczos_forward(x, [oh, ow], out_dtype=torch.float32), yc)
            assert torch.equal(aa.lanczos_forward(x, [oh, ow], out_dtype=torch.float32, mean=mean, std=std), yn)
            assert _lib.last_variant().startswith("generic"), _lib.last_variant()
        finally:
            _lib.set_fused(prev)
        m = torch.tensor(mean, device="cuda").view(1, c, 1, 1)
        s = torch.tensor(std, device="cuda").view(1, c, 1, 1)
        assert torch.allclose(yn, (yf32 - m) / s, rtol=1e-6, atol=1e-5), (case, c, planar)
        # the opt-in tolerance mode takes the exact six-row kernels: same bytes
        assert torch.equal(aa.lanczos_forward(x, [oh, ow], uint8_mode="harness", precision="fast"), yh)


# ------------------------------------------------------------------------------------------------ float dtypes
@pytest.mark.parametrize("name", FILTER_NAMES)
def test_float_dtypes(aa, fx, name):
    from interpolate_antialiasing_amd import _lib

    f = _fwd(aa, name)
    for i, (case, fname, shape, osz) in enumerate(M.FLOAT_CASES):
        if fname != name or len(osz) != 2:
            continue
        x64 = _float_in(fx, i)
        exp = fx[f"flt_{case}_out"]
        for cl in (False, True):
            for dt, tol in ((torch.float64, 1e-9), (torch.float32, 2e-3)):
                x = torch.from_numpy(x64).to("cuda", dt)
                if cl:
                    x = x.contiguous(memory_format=torch.channels_last)
                y = f(x, list(osz))
                assert np.abs(y.double().cpu().numpy() - exp).max() <= tol, (case, dt, cl, _lib.last_variant())
                prev = _lib.set_fused(0)
                try:
                    yg = f(x, list(osz))
                finally:
                    _lib.set_fused(prev)
                assert torch.equal(y, yg), (case, dt, cl)
            x32 = torch.from_numpy(x64).to("cuda", torch.float32)
            for dt in (torch.float16, torch.bfloat16):
                xh = x32.to(dt)
                if cl:
                    xh = xh.contiguous(memory_format=torch.channels_last)
                yh = f(xh, list(osz))
                assert torch.equal(yh, f(xh.float(), list(osz)).to(dt)), (case, dt, cl)
    # a down-scale on the fused float kernel with 6 open rows (Lanczos: support 3) and an up-scale
    rng = np.random.default_rng(11)
    for (h, w), (oh, ow) in (((438, 906), (220, 460)), ((61, 53), (140, 97))):
        x = torch.from_numpy(rng.random((2, 3, h, w)) * 255).cuda()
        for dt in (torch.float32, torch.float64):
            xd = x.to(dt)
            y = f(xd, [oh, ow])
            prev = _lib.set_fused(0)
            try:
                assert torch.equal(y, f(xd, [oh, ow])), (name, dt, (h, w), (oh, ow))
            finally:
                _lib.set_fused(prev)


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("name", FILTER_NAMES)
def test_backward_is_the_adjoint(aa, name):
    """<F x, g> = <x, B^T g> in fp64, gather and atomic forms; gradcheck through torch.ops."""
    from torch.autograd import gradcheck

    fwd = _fwd(aa, name)
    bwd = {"hamming": aa.hamming_backward, "lanczos": aa.lanczos_backward}[name]
    g = torch.Generator(device="cpu").manual_seed(3)
    for (n, c, h, w), (oh, ow), cl in (((2, 3, 61, 53), (17, 23), False), ((1, 2, 19, 23), (41, 37), False),
                                       ((1, 3, 40, 90), (25, 31), True)):
        x = torch.randn(n, c, h, w, generator=g, dtype=torch.float64).cuda()
        gy = torch.randn(n, c, oh, ow, generator=g, dtype=torch.float64).cuda()
        if cl:
            x, gy = x.contiguous(memory_format=torch.channels_last), gy.contiguous(memory_format=torch.channels_last)
        lhs = float((fwd(x, [oh, ow]) * gy).sum())
        for atomic in (False, True):
            gx = bwd(gy, [oh, ow], [n, c, h, w], atomic=atomic)
            rhs = float((x * gx).sum())
            assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs)), (name, atomic, lhs, rhs)
    op = getattr(torch.ops.extension_interpolate, f"{name}_forward")
    for shape, osz in (((1, 2, 12, 17), [5, 7]), ((1, 2, 6, 5), [9, 11])):
        xg = torch.rand(*shape, device="cuda", dtype=torch.float64, requires_grad=True)
        assert gradcheck(lambda t: op(t, osz, False), (xg,), eps=1e-6, atol=1e-6, rtol=1e-6, check_batched_grad=False)


# ------------------------------------------------------------------------------------------------ N-d front-ends
def test_nd_front_ends_match_fixture(aa, fx):
    from interpolate_antialiasing_amd.functional import interpolate_aa

    for i, (case, name, shape, osz) in enumerate(M.FLOAT_CASES):
        if len(osz) == 2:
            continue
        fn = {"hamming": aa.hamming_forward_nd, "lanczos": aa.lanczos_forward_nd}[name]
        x = torch.from_numpy(_float_in(fx, i)).cuda()
        exp = fx[f"flt_{case}_out"]
        y = fn(x, list(osz))
        assert np.abs(y.cpu().numpy() - exp).max() <= 1e-9, case
        assert torch.equal(interpolate_aa(x, osz, mode=name), y), case
        y32 = fn(x.float(), list(osz))
        assert np.abs(y32.double().cpu().numpy() - exp).max() <= 2e-3, case
        # backward: adjoint identity in fp64
        gy = torch.randn(y.shape, dtype=torch.float64, device="cuda")
        bwd = {"hamming": aa.hamming_backward_nd, "lanczos": aa.lanczos_backward_nd}[name]
        gx = bwd(gy, list(osz), list(x.shape))
        assert abs(float((y * gy).sum()) - float((x * gx).sum())) <= 1e-10 * max(1.0, abs(float((y * gy).sum()))), case


def test_interpolate_aa_4d_new_modes(aa, fx):
    from interpolate_antialiasing_amd.functional import interpolate_aa

    i = [c[0] for c in M.FLOAT_CASES].index("f2d_lanczos")
    x = torch.from_numpy(_float_in(fx, i)).cuda().requires_grad_(True)
    y = interpolate_aa(x, (17, 23), mode="lanczos")
    assert np.abs(y.detach().cpu().numpy() - fx["flt_f2d_lanczos_out"]).max() <= 1e-9
    y.sum().backward()
    assert x.grad is not None and x.grad.shape == x.shape


# ------------------------------------------------------------------------------------------------ regression
def test_headline_bilinear_variant_unchanged(aa):
    from interpolate_antialiasing_amd import _lib

    x = torch.randint(0, 256, (2, 438, 906, 3), dtype=torch.uint8, device="cuda").permute(0, 3, 1, 2)
    aa.linear_forward(x, [196, 320], False)
    assert _lib.last_variant() == "fused_u8_nhwc_pil_v3"

