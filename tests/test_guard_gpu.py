"""Guard-band sweep (-m gpu): every kernel writes its whole output and nothing else.

The value tests cannot see where a kernel writes: every output, workspace, descriptor and table comes from torch.empty, which the caching
allocator rounds up to 512 bytes, so a store a few bytes past the end lands in slack, and an element that is never written often shows the
previous, correct result.  Here one public call runs under the guarded allocator of tests/guard_ref.py, once per output placement
(lead 0: the allocator's alignment; lead 1: one element later — a uint8 output on an odd byte, a 16-bit one 2-byte aligned only, a
float32 one 4-byte aligned only, all inside the contract of include/aa_interp.h), and every case asserts

  (a) no byte of the 16 KiB guards around ANY buffer of the call changed (output, workspace, descriptor, tables, N-d intermediates);
  (b) every output element was written: float outputs of finite inputs hold no NaN (the fill), uint8 outputs are bit-identical between
      a run into 0xFF-filled and a run into 0x00-filled memory;
  (c) the output equals the reference of the operation, by the criterion the existing test of that path uses (bit-exact in the default
      precision mode; the derived bounds of the backward tests; the tolerance mode's own tolerances);

and that the kernel family expected for the case really ran (last_variant; for the routes of the fused uint8 kernel, which share one
name, the table figures the route follows from).  Organised by store mechanism and buffer, at the smallest shapes where each exists.
reduce and resize_many* do not report a variant: their cases are pinned by their arguments alone."""
import functools

import numpy as np
import pytest
import torch

import backward_ref as R
import box_reduce_ref as BR
import guard_ref as G
import kit_golden
import kit_gpu
import oracle
import resize_many_ref as MR
from kit_golden import MEAN, MODE, STD

pytestmark = pytest.mark.gpu

LEADS = [0, 1]
HALVES = (torch.float16, torch.bfloat16)
TAG = {torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32", torch.float64: "f64"}
FLOATS = [torch.float32, torch.float16, torch.bfloat16, torch.float64]
SEEN = {}  # group -> variants that ran, printed at the end of the module
BRG = BR.gen()
MG = MR.gen()
AM = kit_golden.generator("alpha")
aa = kit_gpu.aa_fixture(lambda: print("\nguard sweep, variants that ran:", {k: sorted(v) for k, v in sorted(SEEN.items())}))
lib = kit_gpu.lib_fixture()


def _fwd(aa, filt):
    return {"linear": aa.linear_forward, "cubic": aa.cubic_forward, "box": aa.nearest_forward, "nearest": aa.nearest_forward,
            "hamming": aa.hamming_forward, "lanczos": aa.lanczos_forward}[filt]


def _bwd(aa, filt):
    return {"linear": aa.linear_backward, "cubic": aa.cubic_backward, "lanczos": aa.lanczos_backward}[filt]


@functools.lru_cache(maxsize=None)
def _u8(shape, seed):
    x = np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _f32(shape, seed):
    x = (np.random.default_rng(seed).random(shape, dtype=np.float32) * 255).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _pil_ref(filt, shape, seed, size):
    """Pillow's bytes of an NCHW uint8 input, [N, C, oH, oW] on the CPU: the oracle for its three filters, the restatement of the golden
    generators for Hamming and Lanczos.  Computed once, never written."""
    x = _u8(shape, seed)
    if filt in oracle.FILTERS:
        return torch.from_numpy(np.ascontiguousarray(oracle.pil_resize_u8(filt, x, size)))
    return torch.from_numpy(np.stack([BRG.resize_box_restated(filt, np.ascontiguousarray(img.transpose(1, 2, 0)), size[0], size[1]).transpose(2, 0, 1)
                                      for img in x]))


@functools.lru_cache(maxsize=None)
def _float_ref(filt, shape, seed, size, np_dtype=np.float32, from_u8=False):
    """oracle.forward of a float input (or of uint8 bytes as floats), fp32 / fp64, [N, C, oH, oW] numpy.  Once per case, read-only."""
    x = _u8(shape, seed).astype(np.float32) if from_u8 else _f32(shape, seed).astype(np_dtype)
    y = oracle.forward(filt, np.ascontiguousarray(x), size)
    y.setflags(write=False)
    return y


# ---- the guarded call -----------------------------------------------------------------------------------------------------------------
def _placed(rec, y, lead):
    """y is the body of a guarded output allocation at the placement asked for."""
    r = rec.record_of(y)
    assert r is not None and not r.flat, "the result is not an allocation of the guarded allocator"
    assert y.data_ptr() % G.ALIGN == (lead * y.element_size()) % G.ALIGN, (y.data_ptr() % G.ALIGN, lead)


def _guarded(monkeypatch, call, lead, group, variant=None, placed=True, flat_at_least=0, tag=None):
    """One call under the guarded allocator: (a) and (b), the variant and the placement.  uint8 results run twice (two fills).
    variant: None (the call reports none), a name, or a tuple of names.  -> (result, variant that ran, recorder)."""
    from interpolate_antialiasing_amd import _lib

    runs = []
    for fill in (0xFF, 0x00):
        with G.guarded(monkeypatch, lead, fill) as rec:
            try:
                with kit_gpu.gpu_error_ends_the_session(f"{tag}, lead {lead}"):
                    y = call()
                    v = _lib.last_variant()
                    rec.check()  # (a)
            except G.GuardViolation as e:
                raise AssertionError(f"{tag}, lead {lead}, variant {v}: {e}") from None
        if placed:
            _placed(rec, y, lead)
        assert sum(r.flat for r in rec.records) >= flat_at_least, (tag, [repr(r) for r in rec.records])
        runs.append((y, v, rec))
        if y.dtype != torch.uint8:
            break
    y, v, rec = runs[0]
    if variant is not None:
        SEEN.setdefault(group, set()).add(v)
        assert v in ((variant,) if isinstance(variant, str) else variant), (tag, lead, v, variant)
    if y.dtype == torch.uint8:  # (b)
        assert runs[1][1] == v, (tag, v, runs[1][1])
        n = G.unwritten_u8(y, runs[1][0])
        assert n == 0, f"{tag}, lead {lead}, variant {v}: {n} of {y.numel()} output bytes were never written"
    else:
        n = G.unwritten_float(y)
        assert n == 0, f"{tag}, lead {lead}, variant {v}: {n} of {y.numel()} output elements were never written (still the NaN fill)"
    return y, v, rec


def _pil_tables(lib, filt, h, w, oh, ow):
    """The session's (unguarded) Pillow-arithmetic tables of a case: their measured figures decide the fused uint8 kernel's route."""
    from interpolate_antialiasing_amd import tables

    fid = lib.FILTER_IDS[filt]
    dev = torch.device("cuda", torch.cuda.current_device())
    return tables.get_table(fid, lib.TABLE_PIL, h, oh, False, 0.0, dev), tables.get_table(fid, lib.TABLE_PIL, w, ow, False, 0.0, dev)


def _assert_route(lib, route, filt, h, w, oh, ow, tag):
    th, tw = _pil_tables(lib, filt, h, w, oh, ow)
    taps, rows = tw.max_taps, th.scatter_max
    if route == "UP":
        assert h < oh and taps <= 16, (tag, taps)
        return
    assert h >= oh, tag
    if route in ("NARROW", "V1", "ALPHA"):
        assert taps <= 16 and 1 <= rows <= 4, (tag, taps, rows)
    elif route == "WIDE":
        assert 17 <= taps <= 34 and 1 <= rows <= 6, (tag, taps, rows)
    elif route == "SPLIT":
        assert 35 <= taps <= 136 and 1 <= rows <= 6, (tag, taps, rows)
    elif route in ("SIX", "SIX_ALPHA"):
        assert taps <= 16 and 5 <= rows <= 6, (tag, taps, rows)
    else:
        raise AssertionError(route)


# ------------------------------------------------------------------------------------------------ 1. fused uint8, Pillow arithmetic
# (id, C, channels_last, filter, (N, H, W), (oH, oW), route, knobs)
U8_CASES = [
    # channels_last: rows of whole dwords (oW * C and, for C = 3, oW multiples of 4) and rows that are not; C = 4 rows are always dwords
    ("nhwc3_dword_rows", 3, True, "linear", (2, 40, 100), (17, 44), "NARROW", {}),
    ("nhwc3_byte_rows", 3, True, "linear", (2, 40, 100), (17, 45), "NARROW", {}),
    ("nhwc3_ow46_cubic", 3, True, "cubic", (1, 35, 100), (10, 46), "NARROW", {}),
    ("nhwc4_cubic", 4, True, "cubic", (1, 35, 90), (10, 41), "NARROW", {}),
    # 130 columns: three balanced strips of 44, the last one 42 wide; 530 columns: nine strips of 60 in groups of 4, 4 and 1
    ("nhwc3_ragged_last_strip", 3, True, "linear", (1, 30, 300), (13, 130), "NARROW", {}),
    ("nhwc3_nine_strips", 3, True, "linear", (1, 24, 1100), (11, 530), "NARROW", {}),
    ("planar2_nine_strips", 2, False, "linear", (1, 24, 1100), (11, 530), "NARROW", {}),
    # planar: three planes per wave; N * C = 3, 4 (a last group of one) and 5 (a last group of two), and one wave per plane
    ("planar3_byte_rows", 3, False, "linear", (1, 45, 77), (17, 30), "NARROW", {}),
    ("planar3_dword_rows", 3, False, "linear", (1, 45, 77), (17, 32), "NARROW", {}),
    ("planar4_groups", 4, False, "linear", (1, 45, 77), (17, 30), "NARROW", {}),
    ("planar5_groups", 5, False, "linear", (1, 45, 77), (17, 30), "NARROW", {}),
    ("planar4_single_planes", 4, False, "linear", (1, 45, 77), (17, 30), "NARROW", {"groups": 0}),
    ("planar5_single_planes", 5, False, "linear", (1, 45, 77), (17, 30), "NARROW", {"groups": 0}),
    # 17 .. 34 taps, 35 .. 136 taps (a quad's first lane stores), five or six open output rows
    ("nhwc3_wide", 3, True, "cubic", (1, 35, 300), (10, 60), "WIDE", {}),
    ("planar3_wide", 3, False, "cubic", (1, 35, 300), (10, 61), "WIDE", {}),
    ("nhwc3_split", 3, True, "linear", (1, 30, 600), (12, 23), "SPLIT", {}),
    ("nhwc4_split", 4, True, "linear", (1, 30, 600), (12, 23), "SPLIT", {}),
    ("planar3_split", 3, False, "cubic", (1, 35, 600), (10, 23), "SPLIT", {}),
    ("nhwc3_six", 3, True, "lanczos", (1, 48, 80), (32, 50), "SIX", {}),
    ("nhwc4_six", 4, True, "lanczos", (1, 48, 80), (32, 49), "SIX", {}),
    ("planar3_six", 3, False, "lanczos", (1, 48, 80), (32, 50), "SIX", {}),
    # growing heights: channels_last, and planar bytes in 64-byte pieces per strip and row (oW no multiple of 64, at most 256)
    ("nhwc3_up", 3, True, "linear", (1, 12, 70), (100, 45), "UP", {}),
    ("nhwc4_up", 4, True, "cubic", (1, 30, 200), (77, 64), "UP", {}),
    ("planar3_up_200", 3, False, "linear", (1, 21, 64), (64, 200), "UP", {}),
    ("planar3_up_77", 3, False, "cubic", (2, 9, 31), (40, 77), "UP", {}),
    # the first-generation kernel
    ("v1_nhwc3", 3, True, "linear", (2, 40, 100), (17, 44), "V1", {"fused": 2}),
    ("v1_nhwc4", 4, True, "cubic", (1, 35, 90), (10, 41), "V1", {"fused": 2}),
]


@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("case", U8_CASES, ids=lambda c: c[0])
def test_fused_uint8_pillow_arithmetic(aa, lib, monkeypatch, case, lead):
    name, c, cl, filt, (n, h, w), (oh, ow), route, knobs = case
    shape = (n, c, h, w)
    x = kit_gpu.nchw_gpu(_u8(shape, 11), cl)
    want = "fused_u8_nhwc_pil" if route == "V1" else ("fused_u8_nhwc_pil_v3" if cl else "fused_u8_planar_pil_v3")
    _assert_route(lib, route, filt, h, w, oh, ow, name)
    with kit_gpu.Knobs(**knobs):
        y, v, _ = _guarded(monkeypatch, lambda: _fwd(aa, filt)(x, [oh, ow]), lead, "1 fused uint8", want, flat_at_least=2, tag=name)
    assert y.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
    kit_gpu.assert_bits(y, _pil_ref(filt, shape, 11, (oh, ow)), (name, lead, v))


# ------------------------------------------------------------------------------------------------ 2. straight alpha
# (fixture case of tests/golden/alpha.npz, C, channels_last, filter, variant, route)
ALPHA_CASES = [
    ("half_64x80", 4, True, "linear", "fused_u8_nhwc_pil_alpha_v3", "ALPHA"),
    ("six_80x100", 4, True, "lanczos", "fused_u8_nhwc_pil_alpha6_v3", "SIX_ALPHA"),
    ("odd_33x37", 2, True, "linear", "alpha_3step", None),   # LA
    ("odd_33x37", 4, False, "linear", "alpha_3step", None),  # planar RGBA: the premultiplied copy, the plain resize, un-premultiply
]


@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("case", ALPHA_CASES, ids=lambda c: f"{c[0]}_c{c[1]}_{'nhwc' if c[2] else 'nchw'}_{c[3]}")
def test_straight_alpha(aa, lib, monkeypatch, case, lead):
    name, c, cl, filt, want, route = case
    (h, w), (oh, ow), seed = next((cs[1], cs[2], cs[4]) for cs in AM.CASES if cs[0] == name)
    img = AM.make_image(h, w, c, seed)
    fx = kit_golden.fixture("alpha")
    in_crc, exp_crc, exp_samples = AM.expected(fx, name, c, filt)
    assert AM.crc(img) == in_crc
    t = torch.from_numpy(np.ascontiguousarray(img)[None]).cuda().permute(0, 3, 1, 2)
    x = t if cl else t.contiguous()
    if route:
        _assert_route(lib, route, filt, h, w, oh, ow, name)
    y, v, _ = _guarded(monkeypatch, lambda: _fwd(aa, filt)(x, [oh, ow], alpha=True), lead, "2 alpha", want, flat_at_least=2 if route else 3, tag=name)
    got = y[0].permute(1, 2, 0).contiguous().cpu().numpy()
    diff = np.abs(got.reshape(-1, c)[AM.sample_pixels(oh, ow)].astype(int) - exp_samples.astype(int))
    assert diff.max() == 0 and AM.crc(got) == exp_crc, (name, c, cl, filt, v, lead, int(diff.max()))


# ------------------------------------------------------------------------------------------------ 3. uint8 to float in one launch
# (id, C, channels_last input, (H, W), (oH, oW)): even and odd oW (with the placement, what decides pair stores), batch 2
TO_FLOAT = [
    ("c3_even", 3, True, (33, 70), (9, 34)),
    ("c3_odd", 3, True, (33, 70), (9, 33)),
    ("c4_even", 4, True, (40, 140), (12, 66)),
    ("c4_odd", 4, True, (40, 140), (12, 65)),
    ("planar3_even", 3, False, (33, 70), (9, 34)),
    ("planar3_odd", 3, False, (33, 70), (9, 33)),
]


@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=lambda d: TAG[d])
@pytest.mark.parametrize("case", TO_FLOAT, ids=lambda c: c[0])
def test_uint8_to_float(aa, monkeypatch, case, dtype, lead):
    name, c, cl, (h, w), (oh, ow) = case
    shape = (2, c, h, w)
    x = kit_gpu.nchw_gpu(_u8(shape, 12), cl)
    f32 = _float_ref("linear", shape, 12, (oh, ow), from_u8=True)
    m32, s32 = np.asarray(MEAN[:c], np.float32).reshape(1, c, 1, 1), np.asarray(STD[:c], np.float32).reshape(1, c, 1, 1)
    for fmt in ("nchw", "nhwc"):
        for norm in (False, True):
            kw = dict(mean=MEAN[:c], std=STD[:c]) if norm else {}
            want = (f"fused_u8_nhwc_to_{TAG[dtype]}_{fmt}_v3" if cl else
                    f"fused_u8_planar_to_{TAG[dtype]}_v3" if fmt == "nchw" else f"generic_2pass_u8_to_{TAG[dtype]}")  # (a planar wave holds one channel)
            y, v, _ = _guarded(monkeypatch, lambda: aa.linear_forward(x, [oh, ow], out_dtype=dtype, out_format=fmt, **kw), lead, "3 uint8 to float",
                               want, flat_at_least=2 if want.startswith("fused") else 3, tag=(name, fmt, norm))
            assert y.is_contiguous(memory_format=torch.channels_last if fmt == "nhwc" else torch.contiguous_format)
            exp = torch.from_numpy(np.array((f32 - m32) / s32 if norm else f32)).to(dtype)
            kit_gpu.assert_bits(y, exp, (name, TAG[dtype], fmt, norm, lead, v))


@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("cl", [True, False], ids=["nhwc", "planar"])
def test_harness_uint8_output(aa, monkeypatch, cl, lead):
    shape, size = (2, 3, 33, 70), (9, 33)
    x = kit_gpu.nchw_gpu(_u8(shape, 13), cl)
    want = "fused_u8_nhwc_harness_v3" if cl else "fused_u8_planar_harness_v3"
    y, v, _ = _guarded(monkeypatch, lambda: aa.linear_forward(x, list(size), uint8_mode="harness"), lead, "3 harness uint8", want, flat_at_least=2, tag=cl)
    kit_gpu.assert_bits(y, torch.from_numpy(np.ascontiguousarray(oracle.harness_u8("linear", _u8(shape, 13), size))), (cl, lead, v))


# ------------------------------------------------------------------------------------------------ 4. fused floats
def _float_input(shape, seed, dtype, cl=False):
    """A finite float input of `dtype` and the float32 / float64 array the oracle resamples (the input itself, widened exactly)."""
    x = torch.from_numpy(np.array(_f32(shape, seed))).to(dtype)
    wide = x.double().numpy() if dtype == torch.float64 else x.float().numpy()
    xg = x.cuda()
    return (xg.contiguous(memory_format=torch.channels_last) if cl else xg), np.ascontiguousarray(wide)


def _exact_float_case(aa, monkeypatch, group, filt, shape, size, dtype, cl, lead, want, flat_at_least, **kw):
    x, wide = _float_input(shape, 14, dtype, cl)
    y, v, rec = _guarded(monkeypatch, lambda: _fwd(aa, filt)(x, list(size), **kw), lead, group, want, flat_at_least=flat_at_least,
                         tag=(filt, shape, size, TAG[dtype], cl))
    assert y.dtype == dtype and y.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
    exp = torch.from_numpy(oracle.forward(filt, wide, size)).to(dtype)  # (16-bit: the fp32 reference rounded once)
    kit_gpu.assert_bits(y, exp, (filt, shape, size, TAG[dtype], cl, lead, v))
    return v


@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("dtype", FLOATS, ids=lambda d: TAG[d])
@pytest.mark.parametrize("filt,shape,size", [("linear", (2, 3, 61, 53), (17, 23)), ("cubic", (1, 2, 40, 64), (13, 100)), ("linear", (1, 2, 30, 300), (13, 131))],
                         ids=["linear_23", "cubic_100", "three_strips_131"])
def test_fused_float_planes_shrinking(aa, monkeypatch, filt, shape, size, dtype, lead):
    _exact_float_case(aa, monkeypatch, "4 fused float planes", filt, shape, size, dtype, False, lead, f"fused_{TAG[dtype]}_nchw", 2)


@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=lambda d: TAG[d])
@pytest.mark.parametrize("c,size", [(3, (17, 45)), (4, (17, 44)), (3, (13, 130))], ids=["c3_45", "c4_44", "c3_130"])
def test_fused_float_channels_last(aa, monkeypatch, c, size, dtype, lead):
    shape = (2, c, 40, 100) if size[1] < 100 else (1, c, 30, 300)
    _exact_float_case(aa, monkeypatch, "4 fused float channels_last", "linear", shape, size, dtype, True, lead, f"fused_{TAG[dtype]}_nhwc", 2)


# growing heights: 4 / 2 / 1 columns per lane; rows of whole 64-byte sectors, rows that are 8- but not 16-byte aligned, odd widths
UP_SHAPES = [("linear", (1, 2, 20, 128), (44, 512)), ("linear", (1, 2, 30, 90), (41, 258)), ("linear", (1, 2, 20, 100), (33, 301)),
             ("cubic", (2, 3, 9, 31), (40, 50)), ("cubic", (1, 1, 19, 70), (33, 131))]


@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("form", [-1, 0, 1], ids=["store_auto", "store_plain", "store_streaming"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=lambda d: TAG[d])
def test_fused_float_growing_heights_every_store_form(aa, monkeypatch, dtype, form, lead):
    for filt, shape, size in UP_SHAPES:
        with kit_gpu.Knobs(store=form):
            _exact_float_case(aa, monkeypatch, "4 fused float growing", filt, shape, size, dtype, False, lead, f"fused_{TAG[dtype]}_nchw_up", 2)


@pytest.mark.parametrize("lead", LEADS)
def test_tolerance_mode(aa, monkeypatch, lead):
    """precision="fast", one case per unit that has the mode: float planes (fp32, fp16) and the float-arithmetic uint8 kernel (uint8 and
    float32 out).  (a) and (b) as everywhere; (c) with the tolerances of test_fast_precision_mode_is_within_tolerance and of
    test_plane_groups_equal_single_planes."""
    shape, size = (2, 3, 61, 53), (17, 23)
    x, wide = _float_input(shape, 15, torch.float32)
    exp = oracle.forward("linear", wide, size)
    y, _, _ = _guarded(monkeypatch, lambda: aa.linear_forward(x, list(size), precision="fast"), lead, "4 tolerance mode", "fused_f32_nchw_fast",
                       flat_at_least=2, tag="f32")
    np.testing.assert_allclose(y.cpu().numpy(), exp, rtol=1e-4, atol=1e-4 * 255)
    xh = x.half()
    yh, _, _ = _guarded(monkeypatch, lambda: aa.linear_forward(xh, list(size), precision="fast"), lead, "4 tolerance mode", "fused_f16_nchw_fast",
                        flat_at_least=2, tag="f16")
    exact = torch.from_numpy(oracle.forward("linear", xh.float().cpu().numpy(), size)).half()
    np.testing.assert_allclose(yh.float().cpu().numpy(), exact.float().numpy(), rtol=2e-3, atol=0.25)
    u8shape, u8size = (2, 3, 33, 70), (9, 33)
    for cl in (True, False):
        xb = kit_gpu.nchw_gpu(_u8(u8shape, 13), cl)
        want = "fused_u8_nhwc_harness_v3_fast" if cl else "fused_u8_planar_harness_v3_fast"
        yb, _, _ = _guarded(monkeypatch, lambda: aa.linear_forward(xb, list(u8size), uint8_mode="harness", precision="fast"), lead, "4 tolerance mode",
                            want, flat_at_least=2, tag=("harness", cl))
        hb = torch.from_numpy(np.ascontiguousarray(oracle.harness_u8("linear", _u8(u8shape, 13), u8size)))
        assert (yb.cpu().int() - hb.int()).abs().max().item() <= 1
        want = "fused_u8_nhwc_to_f32_nchw_v3_fast" if cl else "fused_u8_planar_to_f32_v3_fast"
        yf, _, _ = _guarded(monkeypatch, lambda: aa.linear_forward(xb, list(u8size), out_dtype=torch.float32, out_format="nchw", precision="fast"), lead,
                            "4 tolerance mode", want, flat_at_least=2, tag=("to_f32", cl))
        np.testing.assert_allclose(yf.cpu().numpy(), _float_ref("linear", u8shape, 13, u8size, from_u8=True), rtol=1e-4, atol=1e-4 * 255)


# ------------------------------------------------------------------------------------------------ 5. the generic two-launch path
@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("size", [(9, 15), (40, 50)], ids=["down", "up"])
@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("kind", ["u8_pil", "u8_harness", "f16", "bf16", "f32", "f64"])
def test_generic_two_launch_path(aa, monkeypatch, kind, cl, size, lead):
    """aa_set_fused(0): the intermediate of the two launches lies in a workspace whose size the shape alone decided."""
    shape = (2, 3, 21, 34)
    with kit_gpu.Knobs(fused=0):
        if kind.startswith("u8"):
            x = kit_gpu.nchw_gpu(_u8(shape, 16), cl)
            mode = kind[3:]
            y, v, _ = _guarded(monkeypatch, lambda: aa.cubic_forward(x, list(size), uint8_mode=mode), lead, "5 generic", f"generic_2pass_{kind}",
                               flat_at_least=3, tag=(kind, cl, size))
            exp = _pil_ref("cubic", shape, 16, size) if mode == "pil" else torch.from_numpy(np.ascontiguousarray(oracle.harness_u8("cubic", _u8(shape, 16), size)))
            kit_gpu.assert_bits(y, exp, (kind, cl, size, lead, v))
        else:
            dtype = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, "f64": torch.float64}[kind]
            _exact_float_case(aa, monkeypatch, "5 generic", "cubic", shape, size, dtype, cl, lead, f"generic_2pass_{kind}", 3)


# ------------------------------------------------------------------------------------------------ 6. backward
U16 = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
SUB = {torch.float16: 2.0 ** -25, torch.bfloat16: 0.0}
# forward (N, C, H, W) -> (oH, oW); the gradient has the output's size.  The first is the backward of a down-scale (the gather grows: the
# fused growing-heights kernel for planes), the second of an up-scale (no fused kernel reads a transposed table in scatter form)
BWD_SHAPES = [((2, 3, 61, 90), (23, 37)), ((1, 2, 19, 23), (41, 60))]


@functools.lru_cache(maxsize=None)
def _dense(name, n_in, n_out):
    return R.dense(name, n_in, n_out, False, np.float32)


@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "generic"])
@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("dt", HALVES, ids=lambda d: TAG[d])
def test_sixteen_bit_backward(aa, monkeypatch, dt, cl, fused, lead):
    """The gather form for 16-bit gradients, judged as tests/test_half_training_gpu.py judges it: within its derived bound of the dense
    float64 adjoint, and bit for bit the float32 backward of the widened gradient, cast back."""
    for i, ((n, c, h, w), (oh, ow)) in enumerate(BWD_SHAPES):
        for name in ("linear", "cubic"):
            gen = torch.Generator(device="cpu").manual_seed(600 + i)
            g0 = (torch.randn(n, c, oh, ow, generator=gen) * 10.0).to(dt).cuda()
            g = g0.contiguous(memory_format=torch.channels_last) if cl else g0
            want = f"fused_{TAG[dt]}_nchw_up" if (fused and not cl and i == 0) else f"generic_2pass_{TAG[dt]}"
            tag = (name, (n, c, h, w), (oh, ow), TAG[dt], cl, fused)
            with kit_gpu.Knobs(fused=fused):
                got, v, _ = _guarded(monkeypatch, lambda: _bwd(aa, name)(g, [oh, ow], [n, c, h, w]), lead, "6 backward 16-bit", want,
                                     flat_at_least=4 if want.startswith("fused") else 5, tag=tag)
                ref = _bwd(aa, name)(g.float(), [oh, ow], [n, c, h, w]).to(dt)
            assert got.dtype == dt and got.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format), tag
            kit_gpu.assert_bits(got, ref.cpu(), (tag, lead, v))
            mats = [_dense(name, h, oh), _dense(name, w, ow)]
            gi, ab = R.backward_dense(mats, g0.float().cpu().numpy().astype(np.float64))
            b32 = R.bound(mats, ab, np.float32)
            bnd = b32 + U16[dt] * (ab + b32) + SUB[dt]
            gotn = got.float().cpu().numpy().astype(np.float64)
            assert np.all(gotn[ab == 0] == 0), ("an element no gradient reaches is not exactly 0", tag)
            r = R.worst_ratio(gotn, gi, bnd)
            assert r <= 1.0, ("16-bit backward outside the derived bound", tag, lead, r)


@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "nhwc"])
def test_float32_atomic_backward_through_python(aa, monkeypatch, cl, lead):
    for i, ((n, c, h, w), (oh, ow)) in enumerate(BWD_SHAPES):
        for name in ("linear", "cubic"):
            g_np = np.random.default_rng(700 + i).standard_normal((n, c, oh, ow)).astype(np.float32)
            g = kit_gpu.nchw_gpu(g_np, cl)
            tag = (name, (n, c, h, w), (oh, ow), cl)
            got, v, _ = _guarded(monkeypatch, lambda: _bwd(aa, name)(g, [oh, ow], [n, c, h, w], atomic=True), lead, "6 backward atomics",
                                 "bwd_scatter_atomics", flat_at_least=2, tag=tag)
            mats = [_dense(name, h, oh), _dense(name, w, ow)]
            gi, ab = R.backward_dense(mats, g_np)
            r = R.worst_ratio(got.cpu().numpy(), gi, R.bound(mats, ab, np.float32))
            assert r <= 1.0, ("backward outside the derived bound", tag, lead, r)


# ------------------------------------------------------------------------------------------------ 7. N-d front-ends
ND_VARIANTS = ("generic_axis", "fused_f32_nchw", "fused_f32_nchw_up")
ND_CASES = [((3, 4), (97,), (31,)), ((3, 4), (97,), (150,)), ((4, 3), (400,), (130,)), ((1, 2), (19, 23, 29), (7, 40, 29)), ((2, 2), (9, 11, 13), (12, 5, 20))]


@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("case", ND_CASES, ids=lambda c: "x".join(str(v) for v in c[1]) + "_to_" + "x".join(str(v) for v in c[2]))
def test_nd_forward_and_backward(aa, monkeypatch, case, lead):
    """1-D and 3-D, float32: one pass per axis, every intermediate an allocation of its own (all of them outputs at the placement)."""
    lead_dims, sizes, osizes = case
    nd = len(sizes)
    for filt, fwd, bwd in (("linear", aa.linear_forward_nd, aa.linear_backward_nd), ("cubic", aa.cubic_forward_nd, aa.cubic_backward_nd)):
        x_np = _f32(lead_dims + sizes, 17)
        x = kit_gpu.nchw_gpu(x_np)
        y, v, rec = _guarded(monkeypatch, lambda: fwd(x, list(osizes)), lead, "7 N-d", ND_VARIANTS, tag=(filt, case))
        assert len(rec.outputs()) == nd
        for t in rec.outputs():
            assert G.unwritten_float(t) == 0, (filt, case, tuple(t.shape))
        exp = x_np
        for axis in range(nd + 1, 1, -1):
            exp = kit_gpu.oracle_axis(filt, exp, axis, osizes[axis - 2])
        kit_gpu.assert_bits(y, torch.from_numpy(np.ascontiguousarray(exp)), (filt, case, lead, v))
        g_np = np.random.default_rng(18).standard_normal(lead_dims + osizes).astype(np.float32)
        g = kit_gpu.nchw_gpu(g_np)
        gi_t, v, rec = _guarded(monkeypatch, lambda: bwd(g, list(osizes), list(lead_dims + sizes)), lead, "7 N-d", ND_VARIANTS, tag=(filt, case, "backward"))
        assert len(rec.outputs()) == nd
        for t in rec.outputs():
            assert G.unwritten_float(t) == 0, (filt, case, tuple(t.shape))
        mats = [_dense(filt, a, b) for a, b in zip(sizes, osizes)]
        gi, ab = R.backward_dense(mats, g_np)
        r = R.worst_ratio(gi_t.cpu().numpy(), gi, R.bound(mats, ab, np.float32))
        assert r <= 1.0, ("N-d backward outside the derived bound", filt, case, lead, r)


# ------------------------------------------------------------------------------------------------ 8. reduce
# (id, (N, C, H, W), (fx, fy), box); every one in both layouts (C = 1: one).  37 x 53 leaves partial right and bottom blocks everywhere.
REDUCE_CASES = [
    ("fx2_c3", (2, 3, 37, 53), (2, 2), None),                 # fx at compile time
    ("fx3_c1", (2, 1, 37, 53), (3, 5), None),
    ("fx4_c2", (2, 2, 37, 53), (4, 3), None),
    ("fx8_c4", (2, 4, 37, 53), (8, 4), None),
    ("fx5_c3", (2, 3, 37, 53), (5, 3), None),                 # fx at run time
    ("fx7_c4", (1, 4, 37, 53), (7, 1), None),
    ("fx1_c2", (1, 2, 37, 53), (1, 7), None),
    ("fx5_c1", (1, 1, 37, 53), (5, 2), None),
    ("odd_box_c3", (2, 3, 37, 53), (3, 3), (5, 7, 50, 36)),   # the box starts on an odd byte in both layouts
    ("odd_box_c4_fx5", (1, 4, 37, 53), (5, 2), (3, 1, 52, 36)),
    ("carry_c3", (1, 3, 5, 3001), (1400, 2), None),           # fx * C > 4096 (channels_last): one output pixel per tile, sums carried
    ("carry_c1", (1, 1, 3, 9001), (4500, 2), None),           # the same for a plane
    ("rows_700_fx2", (1, 3, 700, 10), (2, 300), None),        # more than 256 rows per block: packed sums emptied on the way
    ("rows_700_fx5", (1, 1, 700, 11), (5, 300), None),
    ("one_tile_exactly", (1, 4, 4, 1024), (1, 2), None),       # a row of exactly 4096 bytes
    ("two_tiles", (1, 3, 6, 2051), (2, 4), None),
]


@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("case", REDUCE_CASES, ids=lambda c: c[0])
def test_reduce(aa, monkeypatch, case, lead):
    name, shape, factor, box = case
    x = _u8(shape, 19)
    want = torch.from_numpy(np.stack([BRG.reduce_restated(img, factor, box) for img in x.transpose(0, 2, 3, 1)]).transpose(0, 3, 1, 2))
    for cl in ((False,) if shape[1] == 1 else (True, False)):
        y, _, _ = _guarded(monkeypatch, lambda: aa.reduce(kit_gpu.nchw_gpu(x, cl), factor, box), lead, "8 reduce", None, tag=(name, cl))
        assert y.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
        kit_gpu.assert_bits(y, want, (name, cl, lead))


# ------------------------------------------------------------------------------------------------ 9. box= and reducing_gap=
BOXC = {cs[0]: cs for cs in BRG.BOX_CASES}
GAPC = {cs[0]: cs for cs in BRG.GAP_CASES}
U8_ANY = ("fused_u8_nhwc_pil_v3", "fused_u8_planar_pil_v3", "fused_u8_nhwc_pil", "generic_2pass_u8_pil")


@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("cl", [True, False], ids=["nhwc", "nchw"])
def test_box_and_reducing_gap(aa, monkeypatch, cl, lead):
    """A sub-pixel box (the box tables of _box_table_alloc and a pitched view of the hull), a box that is a plain integer crop, and the
    two-step call (reduce, then the filter with the shifted box): Pillow's bytes from the fixture."""
    fused = "fused_u8_nhwc_pil_v3" if cl else "fused_u8_planar_pil_v3"
    _, shape, seed, (oh, ow), box, _, _ = BOXC["b_down_c3"]
    x_np = BR.batch(shape, seed)
    x = kit_gpu.nchw_gpu(x_np, cl)
    for flt, want in (("linear", fused), ("lanczos", U8_ANY)):  # (bilinear: 7 taps, 3 open rows, a view the fused kernel reads in place)
        y, v, rec = _guarded(monkeypatch, lambda: _fwd(aa, flt)(x, [oh, ow], box=box), lead, "9 box", want, flat_at_least=2, tag=("box", flt, cl))
        assert all(r.nbytes >= 16384 for r in [r for r in rec.records if r.flat][:2])  # (the two box tables come in size classes)
        BR.assert_matches_fixture(f"b_down_c3/{flt}", x_np, y.permute(0, 2, 3, 1).contiguous().cpu().numpy())
    # integer offsets and a box of the output's size: Pillow copies, no kernel, no allocation through torch.empty
    y, _, rec = _guarded(monkeypatch, lambda: aa.lanczos_forward(x, [30, 40], box=(11, 5, 51, 35)), lead, "9 box", None, placed=False, tag=("crop", cl))
    assert torch.equal(y, x[:, :, 5:35, 11:51]) and not rec.records
    for name, flt in (("g_box_2.0", "linear"), ("g_full_3.0", "cubic")):
        _, shape, seed, (oh, ow), box, gap, _ = GAPC[name]
        g_np = BR.batch(shape, seed)
        xg = kit_gpu.nchw_gpu(g_np, cl)
        y, v, rec = _guarded(monkeypatch, lambda: _fwd(aa, flt)(xg, [oh, ow], box=box, reducing_gap=gap), lead, "9 reducing_gap", U8_ANY,
                             flat_at_least=2, tag=(name, flt, cl))
        assert len(rec.outputs()) == 2  # the reduced intermediate and the output, both at the placement
        BR.assert_matches_fixture(f"{name}/{flt}", g_np, y.permute(0, 2, 3, 1).contiguous().cpu().numpy())


# ------------------------------------------------------------------------------------------------ 10. resize_many, resize_many_to_float


@functools.lru_cache(maxsize=None)
def _many_inputs(name, cls):
    return [kit_gpu.to_gpu(MR.item(name, i), cls) for i in range(len(MG.case(name)[3]))]


@functools.lru_cache(maxsize=None)
def _many_bytes(name, f):
    """Pillow's bytes of one fixture case and filter from the CPU restatement, [N, C, oH, oW] (shared, never written)."""
    cs = MG.case(name)
    return torch.from_numpy(np.stack([MG.restated(cs, f, i, MR.item(name, i)).transpose(2, 0, 1) for i in range(len(cs[3]))]))


@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("cls", ["interleaved", "planar"])
@pytest.mark.parametrize("name", ["m_mixed", "m_wide", "m_strips", "m_c2"])
def test_resize_many(aa, monkeypatch, name, cls, lead):
    """The arena of per-item tables and intermediates (ws), the descriptor's device copy and the output."""
    cs = MG.case(name)
    imgs, boxes = _many_inputs(name, cls), [it[2] for it in cs[3]]
    for f in cs[4]:
        y, _, rec = _guarded(monkeypatch, lambda: aa.resize_many(imgs, list(cs[2]), MODE[f], boxes=boxes), lead, "10 resize_many", None,
                             flat_at_least=2, tag=(name, f, cls))
        assert len(rec.records) == 3 and len(rec.outputs()) == 1  # desc_dev, ws, out
        assert y.is_contiguous(memory_format=torch.channels_last if cls == "interleaved" else torch.contiguous_format)
        got = y.cpu()
        for i in range(len(cs[3])):
            MR.assert_matches_fixture(f"{name}/{f}/{i}", MR.item(name, i), got[i].permute(1, 2, 0).numpy())


@pytest.mark.parametrize("lead", LEADS)
def test_resize_many_planar_item_of_two_chunks(aa, monkeypatch, lead):
    """A planar item 9000 columns wide into 9: every window strip covers more than the 8188 columns one staged chunk holds, so the
    horizontal pass walks two chunks (interleaved items reach that at 2730 columns: m_wide).  Expected bytes: the restatement."""
    rng = np.random.default_rng(20)
    sizes = [(5, 9000), (8, 64), (3, 8189)]
    items = [rng.integers(0, 256, (3, h, w), dtype=np.uint8) for h, w in sizes]
    imgs = [kit_gpu.to_gpu(a, "planar") for a in items]
    for f, size in (("linear", (7, 9)), ("cubic", (4, 70))):
        want = torch.from_numpy(np.stack([BRG.resize_box_restated(f, np.ascontiguousarray(a.transpose(1, 2, 0)), size[0], size[1]).transpose(2, 0, 1)
                                          for a in items]))
        y, _, _ = _guarded(monkeypatch, lambda: aa.resize_many(imgs, list(size), MODE[f]), lead, "10 resize_many", None, flat_at_least=2, tag=(f, size))
        assert y.is_contiguous()
        kit_gpu.assert_bits(y, want, (f, size, lead))


@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=lambda d: TAG[d])
@pytest.mark.parametrize("cls", ["interleaved", "planar"])
@pytest.mark.parametrize("name,f", [("m_mixed", "cubic"), ("m_c2", "box")])
def test_resize_many_to_float(aa, monkeypatch, name, f, cls, dtype, lead):
    """Odd output widths (45 and 77), the class's own layout and the other one, flips on and off; expected values as
    tests/test_resize_many_float_gpu.py defines them: torch's conversion of the restatement's bytes, on the CPU."""
    cs = MG.case(name)
    c, n = cs[1], len(cs[3])
    assert cs[2][1] % 2 == 1
    imgs, boxes = _many_inputs(name, cls), [it[2] for it in cs[3]]
    b = _many_bytes(name, f)
    flips_on = [i % 2 == 0 for i in range(n)]
    fl = (b.float() - torch.tensor(MEAN[:c]).view(1, c, 1, 1)) / torch.tensor(STD[:c]).view(1, c, 1, 1)
    for fmt in ("nchw", "nhwc"):
        for flips in (None, flips_on):
            y, _, rec = _guarded(monkeypatch, lambda: aa.resize_many_to_float(imgs, list(cs[2]), MODE[f], boxes=boxes, flips=flips, out_dtype=dtype,
                                                                              out_format=fmt, mean=MEAN[:c], std=STD[:c]),
                                 lead, "10 resize_many_to_float", None, flat_at_least=2, tag=(name, f, cls, fmt, flips is not None))
            assert len(rec.records) == 3
            assert y.is_contiguous(memory_format=torch.channels_last if fmt == "nhwc" else torch.contiguous_format)
            want = fl.to(dtype)
            if flips is not None:
                want = torch.stack([want[i].flip(-1) if flips[i] else want[i] for i in range(n)])
            kit_gpu.assert_bits(y, want, (name, f, cls, fmt, TAG[dtype], flips is not None, lead))


# ------------------------------------------------------------------------------------------------ 11. tables alone
TABLE_SIZES = [(1, 1), (1, 7), (7, 1), (1000, 13), (29, 13), (13, 29), (64, 64)]
FILTER_IDS = {"linear": 0, "cubic": 1, "box": 2, "hamming": 3, "lanczos": 4}


def _three_builds(monkeypatch, build):
    """build() -> [(buffer, bytes that count)]: into 0xFF-filled and 0x00-filled guarded buffers and into plain ones.  The guards are
    intact, and the three are byte-identical: every byte of a table is written, and with the same value wherever it lies."""
    got = []
    for fill in (0xFF, 0x00):
        with G.guarded(monkeypatch, 0, fill) as rec:
            bufs = build()
            rec.check()
            assert rec.records and all(r.flat for r in rec.records)
            for b, _ in bufs:
                assert rec.record_of(b) is not None
        got.append(bufs)
    with monkeypatch.context() as m:  # (fresh caches, the plain allocator)
        from interpolate_antialiasing_amd import tables

        m.setattr(tables, "_cache", {})
        m.setattr(tables, "_box_cache", type(tables._box_cache)())
        got.append(build())
    for (a, na), (b, nb), (p, np_) in zip(*got):
        assert na == nb == np_ and a.numel() >= na
        miss = (a[:na] != b[:na]).nonzero().flatten()
        assert miss.numel() == 0, f"{miss.numel()} of {na} table bytes were never written, offsets {int(miss[0])} .. {int(miss[-1])}"
        diff = (a[:na] != p[:na]).nonzero().flatten()
        assert diff.numel() == 0, (f"the table built into a guarded buffer differs from the same build into a plain one in {diff.numel()} of {na} "
                                   f"bytes, offsets {int(diff[0])} .. {int(diff[-1])}")


@pytest.mark.parametrize("kind", ["pil", "f32", "f64"])
@pytest.mark.parametrize("filt", list(FILTER_IDS))
def test_tables_alone(aa, lib, monkeypatch, filt, kind):
    from interpolate_antialiasing_amd import boxmath, tables

    fid, kid = FILTER_IDS[filt], tables.KIND_IDS[kind]
    dev = torch.device("cuda", torch.cuda.current_device())
    L = lib.load()
    whole = lambda t: (t.buf, t.buf.numel())  # noqa: E731
    for n_in, n_out in TABLE_SIZES:
        for ac in ((False,) if kind == "pil" else (False, True)):  # (Pillow has no align_corners)
            _three_builds(monkeypatch, lambda: [whole(tables.build_table(fid, kid, n_in, n_out, ac, 0.0, dev))])
            if kind != "pil":  # the transposed rows of the backward
                _three_builds(monkeypatch, lambda: [whole(tables.get_transposed_table(tables.get_table(fid, kid, n_in, n_out, ac, 0.0, dev)))])
    for (h, oh), (w, ow) in (((29, 13), (1000, 13)), ((7, 1), (13, 29)), ((1, 7), (64, 63))):  # both tables new: one paired build
        _three_builds(monkeypatch, lambda: [whole(t) for t in tables.get_table_pair(fid, kid, h, oh, w, ow, False, 0.0, 0.0, dev)])
    if kind == "pil":  # box tables: buffers in size classes, the table in their first aa_table_build_bytes_box bytes
        for (h, oh, y0, y1), (w, ow, x0, x1) in (((97, 30, 7.6, 90.2), (131, 40, 10.3, 120.9)), ((64, 20, 2.0, 60.0), (600, 12, 10.5, 590.5)),
                                                 ((9, 9, 0.5, 8.5), (7, 1, 0.25, 6.75))):
            oy, ey = boxmath.axis_hull(h, oh, y0, y1, filt)
            ox, ex = boxmath.axis_hull(w, ow, x0, x1, filt)
            ax_h, ax_w = (oy, ey - oy, oh, y0, y1), (ox, ex - ox, ow, x0, x1)
            nb = [int(L.aa_table_build_bytes_box(fid, kid, a[1], a[2], a[3], a[4])) for a in (ax_h, ax_w)]
            _three_builds(monkeypatch, lambda: [(t.buf, n) for t, n in zip(tables.get_box_table_pair(fid, ax_h, ax_w, dev), nb)])
