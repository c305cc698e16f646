"""The backward on the GPU (-m gpu) against the dense float64 adjoint of tests/backward_ref.py: the transposed weight tables unpacked
and compared with the forward tables entry by entry, then every route a backward can take (gather form through the fused and the
generic kernels and the streaming store forms, atomic form, N-d front-ends, the registered autograd) held element by element to

    |got - A_h^T g A_w| <= (t_h + t_w + 4) u |A_h|^T |g| |A_w|

(backward_ref.py derives it).  Each test prints the largest err / bound it saw per dtype and form (pytest -s shows them)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import backward_ref as R
import kit_gpu

pytestmark = pytest.mark.gpu

NP = {torch.float32: np.float32, torch.float64: np.float64}
WORST = {}     # (dtype name, form) -> largest err / bound seen
_DENSE = {}
aa = kit_gpu.aa_fixture(lambda: print("\nbackward vs dense fp64 reference, worst err / bound:",
                                     {f"{k[0]}/{k[1]}": round(v, 4) for k, v in sorted(WORST.items())}))


def _bwd(aa, name):
    return {"linear": aa.linear_backward, "cubic": aa.cubic_backward, "box": aa.nearest_backward, "hamming": aa.hamming_backward,
            "lanczos": aa.lanczos_backward}[name]


def _dense(name, n_in, n_out, ac, npdt):
    key = (name, n_in, n_out, bool(ac), np.dtype(npdt).name)
    if key not in _DENSE:
        _DENSE[key] = R.dense(name, n_in, n_out, ac, npdt)
    return _DENSE[key]


def _judge(got, gi, bnd, dt, form, tag):
    """got (a tensor) against the reference within the bound, element by element; records the ratio."""
    got = got.detach().cpu().numpy()
    assert got.shape == gi.shape, (tag, got.shape, gi.shape)
    r = R.worst_ratio(got, gi, bnd)
    key = (np.dtype(NP[dt]).name, form)
    WORST[key] = max(WORST.get(key, 0.0), r)
    assert r <= 1.0, ("backward outside the derived bound", tag, form, r)
    return r


def _layout(g, cl):
    return g.contiguous(memory_format=torch.channels_last) if cl else g.contiguous()


FORMS = {"gather_fused": (False, 1, -1), "gather_generic": (False, 0, -1), "gather_store1": (False, 1, 1), "atomic": (True, 1, -1)}


def _run_forms(aa, name, g, in_shape, ac, forms, gi, bnd, variants, tag):
    from interpolate_antialiasing_amd import _lib

    n, c, h, w = in_shape
    oh, ow = g.shape[2:]
    for form in forms:
        atomic, fused, store = FORMS[form]
        with kit_gpu.Knobs(fused, store):
            got = _bwd(aa, name)(g, [oh, ow], [n, c, h, w], ac, atomic=atomic)
            v = _lib.last_variant()
        variants.setdefault(form, set()).add(v)
        assert got.shape == (n, c, h, w) and got.dtype == g.dtype, (tag, form)
        cl = g.is_contiguous(memory_format=torch.channels_last) and not g.is_contiguous()
        assert got.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format), (tag, form)
        _judge(got, gi, bnd, g.dtype, form, tag + (v,))


# ------------------------------------------------------------------------------------------------ 1. the transposed tables
TABLE_PAIRS = [(906, 320), (438, 196), (1024, 224), (196, 438), (20, 900), (2000, 30), (61, 1), (1, 61), (3, 2), (64, 64),
               (3, 4090), (2, 4096)]  # the last two: capacities just under and at the 4096-entry limit


def test_transposed_tables_entry_by_entry(aa):
    """tw[x, k] == w[tmin[x] + k, x - xmin[tmin[x] + k]] for k < tsize[x] and 0 beyond, bit for bit; no tap dropped (the entries of
    the transposed table are those of the forward one); tmin monotone; the header's max_taps is the longest row FOUND (so that a row
    capacity short of it is an error: get_transposed_table raises, which these pairs never see)."""
    from interpolate_antialiasing_amd import _lib, tables

    dev = torch.device("cuda")
    n = 0
    for name in R.FILTERS:
        for kind in (_lib.TABLE_F32, _lib.TABLE_F64):
            for ac in (False, True):
                for n_in, n_out in TABLE_PAIRS:
                    tag = (name, kind, ac, n_in, n_out)
                    fwd = tables.get_table(R.FILTER_ID[name], kind, n_in, n_out, ac, 0.0, dev)
                    tr = tables.get_transposed_table(fwd)
                    xmin, xsize, w = fwd.unpack()
                    tmin, tsize, tw = tr.unpack()
                    assert tr.transposed and (tr.in_size, tr.out_size) == (n_out, n_in) and tw.shape == (n_in, tr.ksize), tag
                    assert w.dtype == tw.dtype == (np.float32 if kind == _lib.TABLE_F32 else np.float64), tag
                    assert tr.ksize == _lib.load().aa_table_transposed_ksize(R.FILTER_ID[name], kind, n_in, n_out, int(ac), 0.0), tag
                    assert tsize.min() >= 0 and tsize.max() <= tr.ksize, tag
                    assert tr.max_taps == max(1, int(tsize.max())), (tag, tr.max_taps, int(tsize.max()))
                    assert int(tsize.sum()) == int(np.maximum(xsize, 1).sum()), ("a tap was dropped", tag, int(tsize.sum()))
                    assert np.all(np.diff(tmin) >= 0) and tmin.min() >= 0 and tmin.max() < n_out, tag
                    k = np.arange(tr.ksize)[None, :]
                    live = k < tsize[:, None]
                    o = np.where(live, tmin[:, None] + k, 0)
                    col = np.where(live, np.arange(n_in)[:, None] - xmin[o], 0)
                    assert np.all(o < n_out) and np.all(col >= 0) and np.all(col[live] < np.maximum(xsize[o], 1)[live]), tag
                    exp = np.where(live, w[o, np.minimum(col, fwd.ksize - 1)], 0)
                    assert np.array_equal(tw.view(np.uint8), exp.astype(tw.dtype).view(np.uint8)), (tag, np.argwhere(tw != exp)[:5])
                    # and the forward table itself is the reference's: what the dense matrices are built from
                    if n_out <= 1000:
                        a = np.zeros((n_out, n_in))
                        rows = np.broadcast_to(np.arange(n_out)[:, None], w.shape)
                        m = np.arange(fwd.ksize)[None, :] < xsize[:, None]
                        a[rows[m], (xmin[:, None] + np.arange(fwd.ksize)[None, :])[m]] = w[m]
                        ref = _dense(name, n_in, n_out, ac, w.dtype)
                        if name in ("hamming", "lanczos"):  # sin / cos of two libms: 1 ulp (f32) / 2 ulps (f64), as test_filters_gpu.py
                            ulps = 1 if kind == _lib.TABLE_F32 else 2
                            tol = np.maximum(ulps * np.spacing(np.maximum(np.abs(a), np.abs(ref)).astype(w.dtype)).astype(np.float64), 1e-12)
                            assert np.all(np.abs(a - ref) <= tol), (tag, np.abs(a - ref).max())
                        else:
                            assert np.array_equal(a, ref), (tag, np.abs(a - ref).max())
                    n += 1
    assert n == 5 * 2 * 2 * len(TABLE_PAIRS)


# ------------------------------------------------------------------------------------------------ 2. every route against the dense reference
# forward (N, C, H, W) -> (oH, oW); the backward maps a gradient of the output size back to the input size
SHAPES = [
    ((2, 3, 438, 906), (196, 320)),     # the headline: gradient rows of 906 columns
    ((1, 2, 1024, 1024), (224, 224)),
    ((2, 3, 196, 320), (438, 906)),     # backward of an up-scale
    ((1, 5, 20, 30), (900, 700)),       # one input feeds ~100 outputs per axis: wide transposed windows
    ((1, 4, 2000, 40), (30, 90)),       # mixed: strong down-scale in H, up-scale in W
    ((2, 1, 64, 300), (64, 100)),       # an identity axis
    ((2, 2, 1, 50), (7, 20)),
    ((2, 2, 50, 1), (20, 7)),
    ((1, 3, 33, 47), (1, 1)),
    ((2, 3, 100, 905), (33, 300)),      # widths that end strips raggedly
    ((2, 3, 65, 1202), (30, 400)),
]


def _matrix_case(aa, rng, name, shape, osz, ac, dtypes, layouts, forms, variants):
    n, c, h, w = shape
    oh, ow = osz
    for dt in dtypes:
        mats = [_dense(name, h, oh, ac, NP[dt]), _dense(name, w, ow, ac, NP[dt])]
        g_np = rng.standard_normal((n, c, oh, ow)).astype(NP[dt])
        gi, ab = R.backward_dense(mats, g_np)
        bnd = R.bound(mats, ab, NP[dt])
        for cl in layouts:
            g = _layout(torch.from_numpy(g_np).cuda(), cl)
            _run_forms(aa, name, g, shape, ac, forms, gi, bnd, variants, (name, shape, osz, ac, str(dt), cl))


def test_backward_every_route_vs_dense_reference(aa):
    """fp32 and fp64, NCHW and channels_last, C in 1..5: the gather form through the fused kernels, the generic two-launch path and the
    streaming store forms, and the atomic form, each against the same dense reference; align_corners off on every shape with linear and
    cubic, on once per shape; box, Hamming and Lanczos on a down-scale and an up-scale."""
    rng = np.random.default_rng(1234)
    variants = {}
    both, all_forms = (torch.float32, torch.float64), tuple(FORMS)
    for shape, osz in SHAPES:
        for name in ("linear", "cubic"):
            _matrix_case(aa, rng, name, shape, osz, False, both, (False, True), all_forms, variants)
    for i, (shape, osz) in enumerate(SHAPES):
        _matrix_case(aa, rng, ("linear", "cubic")[i % 2], shape, osz, True, both, (False, True)[i % 2:][:1], all_forms, variants)
    for name in ("box", "hamming", "lanczos"):
        for shape, osz in (SHAPES[0], SHAPES[2]):
            _matrix_case(aa, rng, name, shape, osz, False, both, (False, True), all_forms, variants)
            _matrix_case(aa, rng, name, shape, osz, True, both, (False,), ("gather_fused", "atomic"), variants)
    print("\nvariants per form:", {k: sorted(v) for k, v in variants.items()})
    assert "fused_f32_nchw_up" in variants["gather_fused"], variants
    assert "fused_f32_nchw_up" in variants["gather_store1"], variants
    assert variants["gather_generic"] and all(v.startswith("generic") for v in variants["gather_generic"]), variants
    assert variants["atomic"] == {"bwd_scatter_atomics"}, variants


# ------------------------------------------------------------------------------------------------ 3. fuzz
def test_backward_fuzz_vs_dense_reference(aa):
    """100 seeded problems: sizes 1..300, factors up to 40x in both directions per axis, any filter, dtype, layout, form, align_corners.
    Forward output sizes stay <= 4096, so no case can pass the transposed table's 4096-entry rows; none is skipped."""
    rng = np.random.default_rng(int(os.environ.get("AA_FUZZ_BWD_SEED", "4711")))   # (a soak: AA_FUZZ_BWD_CASES=2000 AA_FUZZ_BWD_SEED=<n>)
    cases = int(os.environ.get("AA_FUZZ_BWD_CASES", "100"))
    variants, done = {}, 0
    for it in range(cases):
        n, c = int(rng.integers(1, 3)), int(rng.integers(1, 6))
        h, w = int(rng.integers(1, 301)), int(rng.integers(1, 301))
        fh, fw = np.exp(rng.uniform(np.log(1 / 40), np.log(40), 2))
        oh, ow = int(np.clip(round(h * fh), 1, 4096)), int(np.clip(round(w * fw), 1, 4096))
        while oh * ow > 1_500_000:  # (keeps the dense reference modest; deterministic, so still seeded)
            ow = max(1, ow // 2)
        if n * c * oh * ow > 3_000_000:
            n, c = 1, min(c, 2)
        name = R.FILTERS[int(rng.integers(5))]
        dt = (torch.float32, torch.float64)[int(rng.integers(2))]
        cl = bool(rng.integers(2))
        form = ("gather_fused", "gather_generic", "atomic")[int(rng.integers(3))]
        ac = bool(rng.integers(2))
        mats = [R.dense(name, h, oh, ac, NP[dt]), R.dense(name, w, ow, ac, NP[dt])]
        g_np = (rng.standard_normal((n, c, oh, ow)) * 10).astype(NP[dt])
        gi, ab = R.backward_dense(mats, g_np)
        g = _layout(torch.from_numpy(g_np).cuda(), cl)
        _run_forms(aa, name, g, (n, c, h, w), ac, (form,), gi, R.bound(mats, ab, NP[dt]), variants, (it, name, (n, c, h, w), (oh, ow), ac, str(dt), cl))
        done += 1
    assert done == cases
    print("\nfuzz variants per form:", {k: sorted(v) for k, v in variants.items()})


# ------------------------------------------------------------------------------------------------ 4. rows beyond 4096 entries
@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_transposed_rows_beyond_4096_are_an_error_not_numbers(aa, dt):
    """2 -> 20000 along an axis: one input index feeds ~10000 outputs, more than a transposed row holds.  The gather form refuses
    (AA_ERR_KSIZE through the library's error); the atomic form needs no transposed table and matches the reference."""
    from interpolate_antialiasing_amd import _lib

    rng = np.random.default_rng(8)
    for shape, osz in (((1, 2, 2, 5), (20000, 7)), ((1, 2, 6, 2), (4, 20000))):
        n, c, h, w = shape
        g_np = rng.standard_normal((n, c) + osz).astype(NP[dt])
        g = torch.from_numpy(g_np).cuda()
        for name in ("linear", "cubic"):
            with pytest.raises(_lib.AAInterpError, match=r"ksize.*aa_status -7"):
                _bwd(aa, name)(g, list(osz), list(shape), False)
            mats = [_dense(name, h, osz[0], False, NP[dt]), _dense(name, w, osz[1], False, NP[dt])]
            gi, ab = R.backward_dense(mats, g_np)
            got = _bwd(aa, name)(g, list(osz), list(shape), False, atomic=True)
            assert _lib.last_variant() == "bwd_scatter_atomics"
            _judge(got, gi, R.bound(mats, ab, NP[dt]), dt, "atomic", (name, shape, osz))


# ------------------------------------------------------------------------------------------------ 5. gradients that are not dense, autograd
def _nondense_grads(n, c, oh, ow, dt):
    """(what, gradient view on the GPU): a stride-0 expansion of one scalar, a strided slice, a pitched channels_last crop."""
    gen = torch.Generator(device="cpu").manual_seed(17)
    big = torch.randn(n, c, 2 * oh, ow + 40, generator=gen, dtype=dt).cuda()
    nhwc = torch.randn(n, oh + 4, ow + 6, c, generator=gen, dtype=dt).cuda()
    views = [("expanded", torch.ones((), dtype=dt, device="cuda").expand(n, c, oh, ow)),
             ("sliced", big[:, :, ::2, 3:3 + ow]),
             ("channels_last_crop", nhwc.permute(0, 3, 1, 2)[:, :, 2:2 + oh, 3:3 + ow])]
    assert views[0][1].stride() == (0, 0, 0, 0)
    for _, v in views[1:]:
        assert tuple(v.shape) == (n, c, oh, ow) and not v.is_contiguous() and not v.is_contiguous(memory_format=torch.channels_last)
    return views


@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_nondense_gradients_and_autograd_vs_dense_reference(aa, dt):
    """Each gradient view through aa.*_backward (both forms) and through torch.ops.extension_interpolate.*_forward(x).backward(view);
    y.sum().backward() hands the registered autograd the stride-0 gradient: A_h^T 1 A_w."""
    for name, (n, c, h, w), (oh, ow), ac in (("linear", (2, 3, 61, 90), (23, 37), False), ("cubic", (1, 2, 19, 23), (41, 60), True),
                                              ("lanczos", (1, 3, 40, 50), (25, 31), False)):
        mats = [_dense(name, h, oh, ac, NP[dt]), _dense(name, w, ow, ac, NP[dt])]
        op = getattr(torch.ops.extension_interpolate, {"box": "nearest"}.get(name, name) + "_forward")
        for what, gv in _nondense_grads(n, c, oh, ow, dt):
            gi, ab = R.backward_dense(mats, gv.cpu().numpy())
            bnd = R.bound(mats, ab, NP[dt])
            for atomic in (False, True):
                got = _bwd(aa, name)(gv, [oh, ow], [n, c, h, w], ac, atomic=atomic)
                _judge(got, gi, bnd, dt, "atomic" if atomic else "gather_fused", (name, what, atomic))
            x = torch.rand(n, c, h, w, dtype=dt, device="cuda", requires_grad=True)
            op(x, [oh, ow], ac).backward(gv)
            _judge(x.grad, gi, bnd, dt, "autograd", (name, what, "autograd"))
        x = torch.rand(n, c, h, w, dtype=dt, device="cuda", requires_grad=True)
        op(x, [oh, ow], ac).sum().backward()
        gi, ab = R.backward_dense(mats, np.ones((n, c, oh, ow)))
        _judge(x.grad, gi, R.bound(mats, ab, NP[dt]), dt, "autograd", (name, "sum().backward()"))


# ------------------------------------------------------------------------------------------------ 6. every element written, nothing else
@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_every_element_of_grad_input_is_written(aa, dt):
    """Straight through the C-ABI into a buffer pre-filled with NaN (gather form: it is write-once, with no zero fill to lean on) or
    with garbage (atomic form: its own zero fill), 8 guard elements on each side: the result is the reference, no NaN is left, and the
    guards are untouched."""
    from interpolate_antialiasing_amd import _lib, tables

    L = _lib.load()
    dev = torch.device("cuda")
    kind, did = (_lib.TABLE_F32, _lib.F32) if dt == torch.float32 else (_lib.TABLE_F64, _lib.F64)
    es = 4 if dt == torch.float32 else 8
    rng = np.random.default_rng(31)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    seen = set()
    for name, (n, c, h, w), (oh, ow), cl in (("linear", (2, 3, 438, 906), (196, 320), False), ("cubic", (1, 3, 131, 467), (50, 100), False),
                                             ("linear", (2, 3, 61, 53), (17, 23), True), ("cubic", (1, 1, 20, 30), (90, 70), False),
                                             ("linear", (1, 2, 33, 47), (1, 1), False)):
        layout = _lib.NHWC if cl else _lib.NCHW
        mats = [_dense(name, h, oh, False, NP[dt]), _dense(name, w, ow, False, NP[dt])]
        g_np = rng.standard_normal((n, c, oh, ow)).astype(NP[dt])
        gi, ab = R.backward_dense(mats, g_np)
        bnd = R.bound(mats, ab, NP[dt])
        g = _layout(torch.from_numpy(g_np).cuda(), cl)
        th = tables.get_table(R.FILTER_ID[name], kind, h, oh, False, 0.0, dev)
        tw = tables.get_table(R.FILTER_ID[name], kind, w, ow, False, 0.0, dev)
        numel = n * c * h * w

        def view(buf):
            body = buf[8:8 + numel]
            return body.view(n, h, w, c).permute(0, 3, 1, 2) if cl else body.view(n, c, h, w)

        for fused in (1, 0):
            with kit_gpu.Knobs(fused, -1):
                trh, trw = tables.get_transposed_table(th).axis(), tables.get_transposed_table(tw).axis()
                ws_bytes = L.aa_workspace_bytes(did, layout, n, c, oh, ow, h, w, ctypes.byref(trh), ctypes.byref(trw))
                ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
                buf = torch.full((numel + 16,), float("nan"), dtype=dt, device=dev)
                rc = L.aa_resample_bwd(ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(buf.data_ptr() + 8 * es), ctypes.c_void_p(ws.data_ptr()),
                                       ws_bytes, did, layout, n, c, h, w, ctypes.byref(trh), ctypes.byref(trw), stream)
                v = _lib.last_variant()
            assert rc == 0, (name, fused, rc)
            seen.add(v)
            assert fused or v.startswith("generic"), (name, fused, v)
            assert not torch.isnan(buf[8:8 + numel]).any(), ("an element of grad_input was not written", name, fused, v)
            assert torch.isnan(buf[:8]).all() and torch.isnan(buf[8 + numel:]).all(), ("a guard element was written", name, fused, v)
            _judge(view(buf), gi, bnd, dt, "gather_fused" if fused else "gather_generic", (name, "c-abi", v))
        ah, aw = th.axis(), tw.axis()
        ws_bytes = L.aa_workspace_bytes_bwd(did, layout, n, c, h, w, oh, ow)
        ws = torch.full((ws_bytes // es,), 7.0e30, dtype=dt, device=dev)
        buf = torch.full((numel + 16,), -3.0e30, dtype=dt, device=dev)
        rc = L.aa_resample_bwd_atomic(ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(buf.data_ptr() + 8 * es), ctypes.c_void_p(ws.data_ptr()),
                                      ws_bytes, did, layout, n, c, h, w, ctypes.byref(ah), ctypes.byref(aw), stream)
        assert rc == 0 and _lib.last_variant() == "bwd_scatter_atomics", (name, rc)
        assert bool((buf[:8] == -3.0e30).all()) and bool((buf[8 + numel:] == -3.0e30).all()), ("a guard element was written", name, "atomic")
        _judge(view(buf), gi, bnd, dt, "atomic", (name, "c-abi", "atomic"))
    if dt == torch.float32:
        assert "fused_f32_nchw_up" in seen, seen


# ------------------------------------------------------------------------------------------------ 7. inf and nan stay where they belong
@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_nonfinite_gradients_do_not_leak(aa, dt):
    """One inf and one nan in grad_output, gather form through the fused and the generic kernels, a down-scale and an up-scale: the NaN
    and inf masks of grad_input are the reference's (an input index gets them only from outputs whose weight on it is not zero), and
    every finite element is within the bound."""
    rng = np.random.default_rng(77)
    for name in ("linear", "cubic"):
        for (n, c, h, w), (oh, ow) in (((1, 2, 64, 128), (23, 31)), ((1, 2, 23, 31), (100, 200)), ((1, 1, 438, 906), (196, 320))):
            mats = [_dense(name, h, oh, False, NP[dt]), _dense(name, w, ow, False, NP[dt])]
            g_np = rng.standard_normal((n, c, oh, ow)).astype(NP[dt])
            g_np[0, 0, oh // 3, ow // 2] = np.inf
            g_np[0, c - 1, (2 * oh) // 3, ow // 4] = np.nan
            gi, ab = R.backward_dense_nonfinite(mats[0], mats[1], g_np)
            bnd = R.bound(mats, ab, NP[dt])
            ok = np.isfinite(gi)
            assert np.isnan(gi).any() and np.isinf(gi).any() and ok.sum() > ok.size // 2
            g = torch.from_numpy(g_np).cuda()
            for form in ("gather_fused", "gather_generic"):
                _, fused, store = FORMS[form]
                with kit_gpu.Knobs(fused, store):
                    got = _bwd(aa, name)(g, [oh, ow], [n, c, h, w], False).cpu().numpy()
                tag = (name, (h, w), (oh, ow), form)
                assert np.array_equal(np.isnan(got), np.isnan(gi)), ("NaN mask", tag, int(np.isnan(got).sum()), int(np.isnan(gi).sum()))
                assert np.array_equal(got == np.inf, gi == np.inf) and np.array_equal(got == -np.inf, gi == -np.inf), ("inf mask", tag)
                r = R.worst_ratio(got[ok], gi[ok], bnd[ok])
                assert r <= 1.0, ("finite elements", tag, r)


# ------------------------------------------------------------------------------------------------ 8. N-d
@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_nd_backward_vs_dense_reference(aa, dt):
    """*_backward_nd, 1-D and 3-D, against the axis-by-axis reference, align_corners off and on."""
    from interpolate_antialiasing_amd import _lib

    rng = np.random.default_rng(5)
    fns = {"linear": aa.linear_backward_nd, "cubic": aa.cubic_backward_nd, "lanczos": aa.lanczos_backward_nd}
    seen = set()
    for name, lead, sizes, osizes in (("linear", (4, 3), (4000,), (1300,)), ("cubic", (4, 3), (4000,), (1300,)), ("linear", (2, 3), (40,), (900,)),
                                      ("cubic", (2, 3), (40,), (900,)), ("linear", (2, 2), (19, 23, 29), (7, 40, 29)),
                                      ("cubic", (1, 2), (19, 23, 29), (7, 40, 29)), ("lanczos", (1, 2), (19, 23, 29), (7, 40, 29))):
        for ac in (False, True):
            mats = [_dense(name, a, b, ac, NP[dt]) for a, b in zip(sizes, osizes)]
            g_np = rng.standard_normal(lead + osizes).astype(NP[dt])
            gi, ab = R.backward_dense(mats, g_np)
            for fused in (1, 0):
                with kit_gpu.Knobs(fused, -1):
                    got = fns[name](torch.from_numpy(g_np).cuda(), list(osizes), list(lead + sizes), ac)
                    seen.add(_lib.last_variant())
                _judge(got, gi, R.bound(mats, ab, NP[dt]), dt, "nd_fused" if fused else "nd_generic", (name, sizes, osizes, ac))
    print("\nN-d variants:", sorted(seen))
