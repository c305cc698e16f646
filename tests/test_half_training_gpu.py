"""The fp16 / bf16 training path on the GPU (-m gpu).

The backward for 16-bit gradients (gather form) is defined as round_to_nearest_even_16(adjoint_fp32(float(g))): a 2-D or 1-D 16-bit
backward equals backward(g.float()).to(g.dtype) of the same build with the same knobs bit for bit, on every route, and lies within

    |got - gi| <= B32 + k u16 (absref + B32) + s,      B32 = (t_h + t_w + 4) 2^-24 absref   (backward_ref.bound, fp32)

of the dense float64 adjoint of tests/backward_ref.py built from the 16-bit gradient widened exactly: the fp32 backward's own bound,
plus k roundings to 16 bits (u16 = 2^-11 for float16, 2^-8 for bfloat16) of a value that is at most absref + B32 in magnitude, plus
half a spacing of the float16 subnormals (s = 2^-25; bfloat16 has fp32's exponent range: s = 0).  k = 1 in 2-D and 1-D (one rounding
at the store) and the number of passes in 3-D (one per axis, each storing the gradient's dtype).

The fused channels_last forward for 16-bit images with 3 / 4 channels (fused_f16_nhwc / fused_bf16_nhwc) is held bit for bit to the
two-launch path and to half(oracle_fp32(float(x)))."""
import ctypes

import numpy as np
import pytest
import torch

import backward_ref as R
import kit_gpu
import oracle

pytestmark = pytest.mark.gpu

HALVES = (torch.float16, torch.bfloat16)
TAG = {torch.float16: "f16", torch.bfloat16: "bf16"}
U16 = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
SUB = {torch.float16: 2.0 ** -25, torch.bfloat16: 0.0}
WORST = {}
_DENSE = {}
aa = kit_gpu.aa_fixture(lambda: print("\n16-bit backward vs dense fp64 reference, worst err / bound:", {k: round(v, 4) for k, v in sorted(WORST.items())}))


FORMS = {"gather_fused": (1, -1), "gather_generic": (0, -1), "gather_store1": (1, 1)}
# forward (N, C, H, W) -> (oH, oW); the backward maps a gradient of the output size back to the input size
SHAPES = [
    ((2, 3, 61, 90), (23, 37)),
    ((1, 2, 19, 23), (41, 60)),       # the backward of an up-scale
    ((2, 3, 100, 905), (33, 300)),    # odd gradient rows, ragged strips
    ((1, 4, 64, 40), (9, 90)),        # mixed
    ((2, 2, 1, 50), (7, 20)),
    ((1, 3, 33, 47), (1, 1)),
]
# (filter, align_corners) per shape: linear and cubic everywhere, Lanczos on a down-scale and an up-scale, align_corners on once
FILTERS = [(("linear", False), ("cubic", False), ("lanczos", False)), (("linear", False), ("cubic", True), ("lanczos", False)),
           (("linear", False), ("cubic", False)), (("linear", False), ("cubic", False)), (("linear", False), ("cubic", False)),
           (("linear", False), ("cubic", False))]


def _bwd(aa, name):
    return {"linear": aa.linear_backward, "cubic": aa.cubic_backward, "lanczos": aa.lanczos_backward}[name]


def _dense(name, n_in, n_out, ac):
    key = (name, n_in, n_out, bool(ac))
    if key not in _DENSE:
        _DENSE[key] = R.dense(name, n_in, n_out, ac, np.float32)
    return _DENSE[key]


def _layout(g, cl):
    return g.contiguous(memory_format=torch.channels_last) if cl else g.contiguous()


def _is_cl(t):
    return t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous()


def _grad(shape, dt, seed, scale=1.0):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=gen) * scale).to(dt).cuda()


def _judge16(got, g16, mats, dt, k, form, tag):
    """got (a 16-bit tensor) against the dense float64 adjoint of the 16-bit gradient g16 within the bound of this file's docstring."""
    gi, ab = R.backward_dense(mats, g16.detach().float().cpu().numpy().astype(np.float64))
    b32 = R.bound(mats, ab, np.float32)
    bnd = b32 + k * U16[dt] * (ab + b32) + SUB[dt]
    gotn = got.detach().float().cpu().numpy().astype(np.float64)
    assert gotn.shape == gi.shape, (tag, gotn.shape, gi.shape)
    assert np.all(gotn[ab == 0] == 0), ("an element no gradient reaches is not exactly 0", tag)
    r = R.worst_ratio(gotn, gi, bnd)
    key = f"{TAG[dt]}/{form}"
    WORST[key] = max(WORST.get(key, 0.0), r)
    assert r <= 1.0, ("16-bit backward outside the derived bound", tag, form, r)
    return r


# ------------------------------------------------------------------------------------------------ the backward
@pytest.mark.parametrize("dt", HALVES)
def test_backward_is_the_cast_fp32_backward_bit_for_bit(aa, dt):
    """Every route: the fused growing-heights kernel, the generic two-launch path, the streaming store form; NCHW and channels_last."""
    from interpolate_antialiasing_amd import _lib

    variants = {}
    for i, ((n, c, h, w), (oh, ow)) in enumerate(SHAPES):
        for name, ac in FILTERS[i]:
            g0 = _grad((n, c, oh, ow), dt, 100 + i, 10.0)
            for cl in (False, True):
                g = _layout(g0, cl)
                for form, (fused, store) in FORMS.items():
                    with kit_gpu.Knobs(fused, store):
                        got = _bwd(aa, name)(g, [oh, ow], [n, c, h, w], ac)
                        v = _lib.last_variant()
                        ref = _bwd(aa, name)(g.float(), [oh, ow], [n, c, h, w], ac).to(dt)
                    tag = (name, (n, c, h, w), (oh, ow), ac, cl, form, v)
                    variants.setdefault((form, cl), set()).add(v)
                    assert got.dtype == dt and tuple(got.shape) == (n, c, h, w), tag
                    assert got.is_contiguous(memory_format=torch.channels_last if _is_cl(g) else torch.contiguous_format), tag
                    assert torch.isfinite(got.float()).all(), tag
                    assert torch.equal(kit_gpu.bits(got), kit_gpu.bits(ref)), (tag, int((kit_gpu.bits(got) != kit_gpu.bits(ref)).sum()))
    print("\nvariants:", {f"{k[0]}/{'nhwc' if k[1] else 'nchw'}": sorted(v) for k, v in variants.items()})
    assert f"fused_{TAG[dt]}_nchw_up" in variants[("gather_fused", False)], variants
    assert f"fused_{TAG[dt]}_nchw_up" in variants[("gather_store1", False)], variants
    assert all(v.startswith("generic") for cl in (False, True) for v in variants[("gather_generic", cl)]), variants


@pytest.mark.parametrize("dt", HALVES)
def test_backward_vs_dense_fp64_adjoint(aa, dt):
    """2-D on every shape and form, against the dense adjoint of the 16-bit gradient widened exactly."""
    for i, ((n, c, h, w), (oh, ow)) in enumerate(SHAPES):
        for name, ac in FILTERS[i]:
            mats = [_dense(name, h, oh, ac), _dense(name, w, ow, ac)]
            g0 = _grad((n, c, oh, ow), dt, 200 + i, (1.0, 10.0)[i % 2])
            for cl in (False, True):
                g = _layout(g0, cl)
                for form, (fused, store) in FORMS.items():
                    with kit_gpu.Knobs(fused, store):
                        got = _bwd(aa, name)(g, [oh, ow], [n, c, h, w], ac)
                    _judge16(got, g0, mats, dt, 1, form, (name, (n, c, h, w), (oh, ow), ac, cl))


@pytest.mark.parametrize("dt", HALVES)
def test_nd_backward_vs_dense_fp64_adjoint(aa, dt):
    """*_backward_nd: 1-D is one pass (k = 1, and bit-equal to the cast fp32 result); 3-D stores the gradient's dtype after each of its
    three passes (k = 3)."""
    fns = {"linear": aa.linear_backward_nd, "cubic": aa.cubic_backward_nd}
    for name in ("linear", "cubic"):
        for lead, sizes, osizes in (((4, 3), (400,), (130,)), ((2, 3), (40,), (300,)), ((1, 2), (19, 23, 29), (7, 40, 29))):
            mats = [_dense(name, a, b, False) for a, b in zip(sizes, osizes)]
            g = _grad(lead + osizes, dt, 300 + len(sizes), 10.0)
            for fused in (1, 0):
                with kit_gpu.Knobs(fused, -1):
                    got = fns[name](g, list(osizes), list(lead + sizes), False)
                    ref = fns[name](g.float(), list(osizes), list(lead + sizes), False).to(dt)
                assert got.dtype == dt and tuple(got.shape) == lead + sizes
                _judge16(got, g, mats, dt, len(sizes), f"nd{len(sizes)}_{'fused' if fused else 'generic'}", (name, sizes, osizes, fused))
                if len(sizes) == 1:
                    assert torch.equal(kit_gpu.bits(got), kit_gpu.bits(ref)), (name, sizes, osizes, fused)


@pytest.mark.parametrize("dt", HALVES)
@pytest.mark.parametrize("cl", [False, True])
def test_autograd_in_sixteen_bits(aa, dt, cl):
    """torch.ops.extension_interpolate.*_forward(x).backward(g) and interpolate_aa(x).float().square().sum().backward(): x.grad has x's
    dtype and memory format, is finite, and is the direct *_backward call's result bit for bit; a stride-0 gradient (.sum().backward())
    and a sliced gradient view are accepted."""
    from interpolate_antialiasing_amd import interpolate_aa

    (n, c, h, w), (oh, ow) = (2, 3, 61, 90), (23, 37)
    mf = torch.channels_last if cl else torch.contiguous_format
    gen = torch.Generator(device="cpu").manual_seed(5)

    def leaf():
        return torch.rand(n, c, h, w, generator=gen).to(dt).cuda().contiguous(memory_format=mf).requires_grad_()

    def check(x, direct, tag):
        assert x.grad is not None and x.grad.dtype == dt and x.grad.stride() == x.stride(), tag
        assert x.grad.is_contiguous(memory_format=mf), tag
        assert torch.isfinite(x.grad.float()).all(), tag
        assert torch.equal(kit_gpu.bits(x.grad), kit_gpu.bits(direct)), tag

    big = _grad((n, c, 2 * oh, ow + 40), dt, 6)
    for name in ("linear", "cubic", "lanczos"):
        op = getattr(torch.ops.extension_interpolate, name + "_forward")
        g = _layout(_grad((n, c, oh, ow), dt, 7), cl)
        x = leaf()
        op(x, [oh, ow], False).backward(g)
        check(x, _bwd(aa, name)(g, [oh, ow], [n, c, h, w], False), (name, "dense"))
        gv = big[:, :, ::2, 3:3 + ow]  # a sliced view
        assert not gv.is_contiguous()
        x = leaf()
        op(x, [oh, ow], False).backward(gv)
        check(x, _bwd(aa, name)(gv, [oh, ow], [n, c, h, w], False), (name, "sliced"))
        x = leaf()
        op(x, [oh, ow], False).sum().backward()  # a stride-0 gradient
        ones = torch.ones((), dtype=dt, device="cuda").expand(n, c, oh, ow)
        direct = _bwd(aa, name)(ones, [oh, ow], [n, c, h, w], False)
        check(x, direct, (name, "sum"))
        _judge16(x.grad, ones, [_dense(name, h, oh, False), _dense(name, w, ow, False)], dt, 1, "autograd", (name, "sum", cl))
    for mode, name in (("bilinear", "linear"), ("bicubic", "cubic")):
        x = leaf()
        y = interpolate_aa(x, [oh, ow], mode)
        assert y.dtype == dt
        y.float().square().sum().backward()
        g = (2.0 * y.detach().float()).to(dt)
        check(x, _bwd(aa, name)(g, [oh, ow], [n, c, h, w], False), (mode, "interpolate_aa"))


@pytest.mark.parametrize("dt", HALVES)
def test_nonfinite_sixteen_bit_gradients_do_not_leak(aa, dt):
    """One inf and one nan in a 16-bit gradient: the NaN / +-inf masks of the result are those of the fp32 backward of the up-cast
    gradient, and every other element is its cast, bit for bit."""
    for name in ("linear", "cubic"):
        for (n, c, h, w), (oh, ow) in (((1, 2, 64, 128), (23, 31)), ((1, 2, 23, 31), (100, 200))):
            g = _grad((n, c, oh, ow), dt, 9)
            g[0, 0, oh // 3, ow // 2] = float("inf")
            g[0, c - 1, (2 * oh) // 3, ow // 4] = float("nan")
            for cl in (False, True):
                gl = _layout(g, cl)
                for form in ("gather_fused", "gather_generic"):
                    fused, store = FORMS[form]
                    with kit_gpu.Knobs(fused, store):
                        got = _bwd(aa, name)(gl, [oh, ow], [n, c, h, w], False)
                        ref = _bwd(aa, name)(gl.float(), [oh, ow], [n, c, h, w], False)
                    tag = (name, (h, w), (oh, ow), cl, form)
                    gf = got.float()
                    assert torch.isnan(ref).any() and torch.isinf(ref).any() and torch.isfinite(ref).sum() > ref.numel() // 2, tag
                    assert torch.equal(torch.isnan(gf), torch.isnan(ref)), ("NaN mask", tag)
                    inf = float("inf")
                    assert torch.equal(gf == inf, ref.to(dt).float() == inf) and torch.equal(gf == -inf, ref.to(dt).float() == -inf), ("inf mask", tag)
                    assert torch.equal(torch.isinf(gf), torch.isinf(ref)), ("inf mask (no finite value overflowed)", tag)
                    ok = torch.isfinite(ref)
                    assert torch.equal(got[ok].view(torch.int16), ref.to(dt)[ok].view(torch.int16)), tag


def test_integration_stub_backward_in_sixteen_bits(aa):
    """The reference-side binding's linear_backward takes half and bfloat16 gradients and gives the shim's result bit for bit."""
    import importlib.util
    import os

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "integration_stub", "build.py")
    spec = importlib.util.spec_from_file_location("aa_stub_build", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    stub = mod.build()
    for dt in HALVES:
        for cl in (False, True):
            g = _layout(_grad((2, 3, 23, 37), dt, 11), cl)
            a = stub.linear_backward(g, [23, 37], [2, 3, 61, 90], False)
            b = aa.linear_backward(g, [23, 37], [2, 3, 61, 90])
            assert a.dtype == dt and a.stride() == b.stride() and torch.equal(kit_gpu.bits(a), kit_gpu.bits(b)), (dt, cl)


# ------------------------------------------------------------------------------------------------ the 16-bit channels_last forward
def _fwd(aa, filt):
    return {"linear": aa.linear_forward, "cubic": aa.cubic_forward}[filt]


def _image(shape, dt, seed):
    """A channels_last 16-bit image batch [N, C, H, W] with values in [-40, 260)."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    n, c, h, w = shape
    return ((torch.rand(n, h, w, c, generator=gen) * 300) - 40).to(dt).cuda().permute(0, 3, 1, 2)


def _check_nhwc(aa, filt, x, size, tag, oracle_too=True):
    """x through the fused kernel: the variant, the two-launch path's bits, the oracle's first image."""
    from interpolate_antialiasing_amd import _lib

    dt = x.dtype
    assert _is_cl(x), tag
    y = _fwd(aa, filt)(x, list(size))
    v = _lib.last_variant()
    with kit_gpu.Knobs(0, -1):
        y0 = _fwd(aa, filt)(x, list(size))
        v0 = _lib.last_variant()
    assert v == f"fused_{TAG[dt]}_nhwc", (tag, v)
    assert v0.startswith("generic_2pass"), (tag, v0)
    assert y.dtype == dt and _is_cl(y) and tuple(y.shape) == tuple(x.shape[:2]) + tuple(size), tag
    assert torch.equal(kit_gpu.bits(y), kit_gpu.bits(y0)), (tag, int((kit_gpu.bits(y) != kit_gpu.bits(y0)).sum()))
    if oracle_too:
        exp = torch.from_numpy(oracle.forward(filt, x[:1].float().cpu().numpy(), tuple(size))).to(dt)
        assert torch.equal(kit_gpu.bits(y[:1].cpu()), kit_gpu.bits(exp)), (tag, "oracle")
    return y


NHWC_CASES = {
    "a": [((2, 37, 61), (13, 23), "linear")],      # C = 3: rows of 183 elements (odd), 69 output elements, right-aligned windows at the row end
    "b": [((1, 40, 9), (20, 4), "linear")],        # the row barely wider than the 8-tap window: lead > 0 on most lanes
    "c": [((2, 64, 200), (40, 71), "cubic")],      # several bands (oH >= 16), scatter_max above 2
    "d": [((1, 64, 906), (16, 120), "linear"), ((1, 64, 906), (16, 120), "cubic"), ((1, 64, 906), (16, 160), "cubic"),  # 17, 33, 25 taps: the
          # AND-mask form beyond 28 positions, two DMAs per row;
          ((1, 32, 1300), (8, 100), "linear")],    # 27 taps whose starts lie 13 pixels apart: a strip of 64 elements spans more than 128
                                                   # staged pieces of 8 halves, so the strip width falls back to 32 elements
    "e": [((2, 300, 31), (10, 40), "cubic")],      # the width grows while the height shrinks
}


@pytest.mark.parametrize("dt", HALVES)
@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("case", sorted(NHWC_CASES))
def test_nhwc16_forward_is_fused_and_exact(aa, dt, c, case):
    for j, ((n, h, w), size, filt) in enumerate(NHWC_CASES[case]):
        x = _image((n, c, h, w), dt, 1000 + 10 * ord(case) + j)
        _check_nhwc(aa, filt, x, size, (case, TAG[dt], c, (n, h, w), size, filt))


@pytest.mark.parametrize("dt", HALVES)
def test_nhwc16_tensor_ending_on_its_allocation(aa, dt):
    """Rows of W * C = 57 / 27 elements (odd): the dword holding the tensor's final element straddles the end of the tensor.  The kernel
    fetches that element on its own and reads nothing beyond the tensor; what is checked here is the VALUE (the last output pixel, which
    depends on it): a tensor of 57 x 512 bytes, and one of 54 MiB that fills its allocator block exactly."""
    from interpolate_antialiasing_amd import _lib

    x = _image((1, 3, 256, 19), dt, 21)
    assert x.numel() * 2 == 57 * 512
    y = _check_nhwc(aa, "linear", x, (100, 7), ("f", TAG[dt]))
    torch.cuda.empty_cache()
    big = torch.empty((1024, 1024, 9, 3), dtype=dt, device="cuda")
    assert big.numel() * 2 == 54 << 20
    big.uniform_(-40.0, 260.0)
    x = big.permute(0, 3, 1, 2)
    y = aa.linear_forward(x, [512, 4])
    v = _lib.last_variant()
    with kit_gpu.Knobs(0, -1):
        y0 = aa.linear_forward(x, [512, 4])
    torch.cuda.synchronize()
    assert v == f"fused_{TAG[dt]}_nhwc", v
    assert torch.equal(kit_gpu.bits(y[-1, :, -1, -1]), kit_gpu.bits(y0[-1, :, -1, -1])), "the last output pixel"
    assert torch.equal(kit_gpu.bits(y), kit_gpu.bits(y0))
    exp = torch.from_numpy(oracle.forward("linear", x[-1:].float().cpu().numpy(), (512, 4))).to(dt)
    assert torch.equal(kit_gpu.bits(y[-1:].cpu()), kit_gpu.bits(exp)), "oracle, last image"
    del big, x, y, y0


def test_nhwc16_fp16_products_are_the_references(aa):
    """The smallest denormal half, a block of tiny normals and denormals, large negatives, signed zeros: the fp16 product (v_fma_mix_f32
    on the low half, addend -0.0) is the separately rounded float(h) * w of the reference in every corner."""
    torch.manual_seed(9)
    x = (torch.rand(2, 64, 120, 3, device="cuda") * 255).half().permute(0, 3, 1, 2)
    x[0, 0, :10] = 0.0
    x[0, 1, :10] = -0.0
    x[0, 2, 10:30, 20:100] = torch.tensor(6.0e-8, dtype=torch.float16, device="cuda")   # the smallest denormal half
    x[1, 0, 30:50] = (torch.rand(20, 120, device="cuda") * 6.0e-5).half()              # denormals and tiny normals
    x[1, 1, 5:60, 50:110] = -(torch.rand(55, 60, device="cuda") * 6.0e4).half()         # large negatives
    x[1, 2, ::3] = 65504.0
    for filt in ("linear", "cubic"):
        _check_nhwc(aa, filt, x, (20, 37), ("h", filt))


@pytest.mark.parametrize("dt", HALVES)
@pytest.mark.parametrize("c", [3, 4])
def test_nhwc16_nonfinite_pixels_do_not_leak(aa, dt, c):
    from interpolate_antialiasing_amd import _lib

    x = _image((2, c, 37, 61), dt, 33).clone(memory_format=torch.channels_last)
    x[0, 0, 11, 30] = float("nan")
    x[1, c - 1, 20, 7] = float("inf")
    for filt in ("linear", "cubic"):
        y = _fwd(aa, filt)(x, [13, 23])
        assert _lib.last_variant() == f"fused_{TAG[dt]}_nhwc"
        with kit_gpu.Knobs(0, -1):
            y0 = _fwd(aa, filt)(x, [13, 23])
        yf, y0f = y.float(), y0.float()
        assert torch.isnan(y0f).any() and torch.isinf(y0f).any() and torch.isfinite(y0f).sum() > y0f.numel() // 2
        assert torch.equal(torch.isnan(yf), torch.isnan(y0f)), (filt, "NaN mask")
        assert torch.equal(yf == float("inf"), y0f == float("inf")) and torch.equal(yf == -float("inf"), y0f == -float("inf")), (filt, "inf mask")
        ok = torch.isfinite(y0f)
        assert torch.equal(y[ok].view(torch.int16), y0[ok].view(torch.int16)), filt


@pytest.mark.parametrize("dt", HALVES)
@pytest.mark.parametrize("c", [3, 4])
def test_nhwc16_views_are_read_in_place(aa, monkeypatch, dt, c):
    """A channels_last crop and a batch slice of a larger 16-bit NHWC tensor go through aa_resample_fwd_strided and are served where they
    lie (its return code is AA_OK, nothing is copied), by the same kernel and with the dense copy's result; so is a tensor whose storage
    starts on an odd element (2-byte aligned only): dispatch does not depend on the pointers."""
    from interpolate_antialiasing_amd import _lib

    L = _lib.load()
    real = L.aa_resample_fwd_strided
    codes, copies = [], []

    def spy(*a):
        codes.append(real(*a))
        return codes[-1]

    monkeypatch.setattr(L, "aa_resample_fwd_strided", spy, raising=False)
    real_mf = aa._memory_format
    monkeypatch.setattr(aa, "_memory_format", lambda t: (copies.append(tuple(t.shape)), real_mf(t))[1])
    want = f"fused_{TAG[dt]}_nhwc"
    h, w, size = 37, 61, [13, 23]
    big = _image((4, c, h + 10, w + 8), dt, 44)
    views = [("crop", big[:, :, 5:5 + h, 3:3 + w]), ("crop at an odd element", big[:, :, 6:6 + h, 4:4 + w][1:]),
             ("batch slice", big[::2]), ("crop of a batch slice", big[1::2, :, 5:5 + h, 2:2 + w])]
    for what, view in views:
        assert not view.is_contiguous() and not view.is_contiguous(memory_format=torch.channels_last), what
        codes.clear()
        copies.clear()
        y = aa.linear_forward(view, size if view.shape[2] == h else [17, 27])
        assert _lib.last_variant() == want, (what, _lib.last_variant())
        assert codes == [_lib.AA_OK] and copies == [], (what, codes, copies)
        ref = aa.linear_forward(view.contiguous(memory_format=torch.channels_last), size if view.shape[2] == h else [17, 27])
        assert _lib.last_variant() == want, what
        assert torch.equal(kit_gpu.bits(y), kit_gpu.bits(ref)) and _is_cl(y), what
    if c == 3:
        assert (views[1][1].storage_offset() & 1) == 1, "the second crop is meant to start on an odd element"
    # a dense tensor that is only 2-byte aligned
    flat = torch.empty(2 * h * w * c + 1, dtype=dt, device="cuda")
    x = _image((2, c, h, w), dt, 45)
    odd = flat[1:].view(2, h, w, c).permute(0, 3, 1, 2)
    odd.copy_(x)
    assert odd.data_ptr() % 4 == 2 and _is_cl(odd)
    y = aa.cubic_forward(odd, size)
    assert _lib.last_variant() == want
    assert torch.equal(kit_gpu.bits(y), kit_gpu.bits(aa.cubic_forward(x, size)))


@pytest.mark.parametrize("dt", HALVES)
def test_nhwc16_workspace_answer_matches_dispatch(aa, dt):
    """aa_workspace_bytes answers 0 exactly where the fused kernel runs, and non-zero for a shape no width holds (45 taps), which runs
    the two-launch path."""
    from interpolate_antialiasing_amd import _lib, tables

    L = _lib.load()
    dev = torch.device("cuda")
    did = _lib.F16 if dt == torch.float16 else _lib.BF16

    def ws(filt, n, c, h, w, oh, ow):
        th, tw = tables.get_table_pair(R.FILTER_ID[filt], _lib.TABLE_F32, h, oh, w, ow, False, 0.0, 0.0, dev)
        ah, aw = th.axis(), tw.axis()
        return L.aa_workspace_bytes(did, _lib.NHWC, n, c, h, w, oh, ow, ctypes.byref(ah), ctypes.byref(aw))

    for case in "acd":
        for (n, h, w), (oh, ow), filt in NHWC_CASES[case]:
            for c in (3, 4):
                assert ws(filt, n, c, h, w, oh, ow) == 0, (case, c, filt)
    assert ws("linear", 1, 3, 32, 2200, 16, 100) > 0
    x = _image((1, 3, 32, 2200), dt, 55)
    y = aa.linear_forward(x, [16, 100])
    assert _lib.last_variant().startswith("generic_2pass"), _lib.last_variant()
    exp = torch.from_numpy(oracle.forward("linear", x.float().cpu().numpy(), (16, 100))).to(dt)
    assert torch.equal(kit_gpu.bits(y.cpu()), kit_gpu.bits(exp))


@pytest.mark.parametrize("dt", HALVES)
@pytest.mark.parametrize("c", [3, 4])
def test_nhwc16_fast_precision_runs_the_exact_kernel(aa, dt, c):
    from interpolate_antialiasing_amd import _lib

    x = _image((2, c, 37, 61), dt, 66)
    y = aa.linear_forward(x, [13, 23])
    yf = aa.linear_forward(x, [13, 23], precision="fast")
    assert _lib.last_variant() == f"fused_{TAG[dt]}_nhwc", _lib.last_variant()
    assert torch.equal(kit_gpu.bits(y), kit_gpu.bits(yf))
