"""The backward's host-side facts, without a GPU: the row capacity of the transposed (adjoint) weight table against the true number of
outputs an input index feeds, and the dense float64 reference of tests/backward_ref.py against the committed goldens, before that
reference judges any kernel (test_backward_gpu.py)."""
import numpy as np
import pytest

import backward_ref as R
import oracle

KINDS = (("f32", np.float32), ("f64", np.float64))
SLOW = ("hamming", "lanczos")  # their weights come from a scalar restatement; their WINDOWS are vectorised (R.windows) like everyone's


def _pairs():
    """Every (in, out) in 1..39 x 1..39, 1500 seeded random pairs up to 3000, 400 extreme ones (<= 60 against 500..4000, both ways)."""
    rng = np.random.default_rng(20240611)
    grid = [(a, b) for a in range(1, 40) for b in range(1, 40)]
    rnd = [(int(a), int(b)) for a, b in rng.integers(1, 3001, (1500, 2))]
    small, large = rng.integers(1, 61, 400), rng.integers(500, 4001, 400)
    ext = [(int(s), int(b)) if i % 2 else (int(b), int(s)) for i, (s, b) in enumerate(zip(small, large))]
    return grid, rnd, ext


def _lib_kind(L, kname):
    from interpolate_antialiasing_amd import _lib

    return _lib.TABLE_F32 if kname == "f32" else _lib.TABLE_F64


def _check_capacity(L, name, kname, dt, n_in, n_out, ac, scale, xmin, xsize, stats):
    tag = (name, kname, n_in, n_out, ac, scale)
    assert R.monotone(xmin, xsize), tag
    need = max(1, int(R.cover(xmin, xsize, n_in).max()))
    est = R.capacity_estimate(name, n_in, n_out, ac, dt, scale)
    assert est >= need, ("the restated estimate is short", tag, est, need)
    tk = L.aa_table_transposed_ksize(R.FILTER_ID[name], _lib_kind(L, kname), n_in, n_out, int(ac), float(scale))
    fwd_k = L.aa_table_ksize(R.FILTER_ID[name], _lib_kind(L, kname), n_in, n_out, int(ac), float(scale))
    if fwd_k < 0:  # no forward table to transpose (its own rows would pass 4096 taps): the same error
        assert fwd_k == -7 and tk == -7, tag
    elif est > R.MAX_KSIZE:
        assert tk == -7, tag  # AA_ERR_KSIZE
    else:
        assert tk >= need, ("transposed rows too short: gradient taps would be dropped", tag, tk, need)
        assert tk == est, ("aa_table_transposed_ksize is not the documented formula", tag, tk, est)
    stats["n"] += 1
    stats["slack"] = min(stats["slack"], est - need)


def test_windows_restatement_is_the_oracles():
    """R.windows (used for Hamming and Lanczos, vectorised) is the window arithmetic of oracle.weights for the reference's three filters,
    and Hamming's windows are the linear filter's (the same support)."""
    rng = np.random.default_rng(5)
    pairs = [(a, b) for a in range(1, 40, 3) for b in range(1, 40, 2)] + [(int(a), int(b)) for a, b in rng.integers(1, 3001, (150, 2))]
    for name in ("linear", "cubic", "box"):
        for kname, dt in KINDS:
            for ac in (False, True):
                for n_in, n_out in pairs:
                    _, xmin, xsize, _ = oracle.weights(name, n_in, n_out, ac, dt)
                    wx, ws = R.windows(name, n_in, n_out, ac, dt)
                    assert np.array_equal(wx, xmin) and np.array_equal(ws, xsize), (name, kname, ac, n_in, n_out)
            for n_in, n_out in pairs[::5]:
                for s in (0.37, 1.0, 2.5, n_out / n_in):
                    _, xmin, xsize, _ = oracle.weights(name, n_in, n_out, False, dt, s)
                    wx, ws = R.windows(name, n_in, n_out, False, dt, s)
                    assert np.array_equal(wx, xmin) and np.array_equal(ws, xsize), (name, kname, s, n_in, n_out)
    for kname, dt in KINDS:
        for n_in, n_out in pairs:
            h, l = R.windows("hamming", n_in, n_out, False, dt), oracle.weights("linear", n_in, n_out, False, dt)
            assert np.array_equal(h[0], l[1]) and np.array_equal(h[1], l[2])


def test_pillow_filter_tables_are_the_fixtures_restatement():
    """R.axis_table for Hamming / Lanczos at the plain scale equals make_golden_filters.f32_table / f64_table bit for bit (which
    test_filters_cpu.py pins to tests/golden/filters.npz)."""
    for name in SLOW:
        for n_in, n_out in ((1, 1), (3, 7), (7, 3), (17, 40), (64, 200), (438, 196), (250, 31), (33, 5), (100, 101)):
            for dt, fn in ((np.float32, R.M.f32_table), (np.float64, R.M.f64_table)):
                k, xmin, xsize, w = R.axis_table(name, n_in, n_out, False, dt)
                ek, exmin, exsize, ew = fn(name, n_in, n_out)
                assert k == ek and np.array_equal(xmin, exmin) and np.array_equal(xsize, exsize), (name, n_in, n_out, dt)
                assert w.dtype == ew.dtype and np.array_equal(w, ew), (name, n_in, n_out, dt)


def test_transposed_capacity_covers_every_input_index():
    """aa_table_transposed_ksize = ceil((2 support + 1) / scale) + 3, clipped to out_size, is at least the true largest number of outputs
    whose window holds one input index, for all five filters, both float table kinds, align_corners off and on; and the windows are
    monotone (so that those outputs are a contiguous range).  The smallest slack over the sweep is 0: the bound is met exactly, with no
    margin in hand."""
    from interpolate_antialiasing_amd import _lib

    L = _lib.load()
    grid, rnd, ext = _pairs()
    stats = {"n": 0, "slack": 1 << 30}
    for name in R.FILTERS:
        for kname, dt in KINDS:
            for ac in (False, True):
                for n_in, n_out in grid + rnd + ext:
                    if name in SLOW:
                        xmin, xsize = R.windows(name, n_in, n_out, ac, dt)
                    else:
                        _, xmin, xsize, _ = oracle.weights(name, n_in, n_out, ac, dt)
                    _check_capacity(L, name, kname, dt, n_in, n_out, ac, 0.0, xmin, xsize, stats)
    assert stats["n"] == 5 * 2 * 2 * (39 * 39 + 1500 + 400)
    assert stats["slack"] >= 0
    print("capacity sweep:", stats)


def test_transposed_capacity_with_explicit_scale_factors():
    """The same with a user scale factor (the `scale` argument; the windows then follow 1 / scale, not in / out)."""
    from interpolate_antialiasing_amd import _lib

    L = _lib.load()
    rng = np.random.default_rng(99)
    stats = {"n": 0, "slack": 1 << 30}
    pairs = [(a, b) for a in range(1, 40, 4) for b in range(1, 40, 3)] + [(int(a), int(b)) for a, b in rng.integers(1, 1501, (150, 2))]
    for name in R.FILTERS:
        for kname, dt in KINDS:
            for n_in, n_out in pairs:
                exact = n_out / n_in
                for s in (exact, exact * 1.003, exact * 0.91, float(np.exp(rng.uniform(np.log(1 / 40), np.log(40)))), 1.0, 2.0, 0.5):
                    if name in SLOW:
                        xmin, xsize = R.windows(name, n_in, n_out, False, dt, s)
                    else:
                        _, xmin, xsize, _ = oracle.weights(name, n_in, n_out, False, dt, s)
                    _check_capacity(L, name, kname, dt, n_in, n_out, False, s, xmin, xsize, stats)
    assert stats["slack"] >= 0
    print("capacity sweep, explicit scales:", stats)


def test_transposed_capacity_edges():
    """Pillow-kind tables have no adjoint (AA_ERR_BAD_DTYPE); a capacity above 4096 is AA_ERR_KSIZE, 4096 itself is served."""
    from interpolate_antialiasing_amd import _lib

    L = _lib.load()
    for fid in range(5):
        assert L.aa_table_transposed_ksize(fid, _lib.TABLE_PIL, 438, 196, 0, 0.0) == -2
        assert L.aa_table_transposed_ksize(fid, _lib.TABLE_PIL, 20, 900, 0, 0.0) == -2
        for kind in (_lib.TABLE_F32, _lib.TABLE_F64):
            assert L.aa_table_transposed_ksize(fid, kind, 2, 20000, 0, 0.0) == -7
            assert L.aa_table_transposed_ksize(fid, kind, 2, 4097, 0, 0.0) == -7
            assert L.aa_table_transposed_ksize(fid, kind, 2, 4096, 0, 0.0) == 4096
            if fid != 2:  # (box: support 1/2, about 2 / scale = 2730 entries)
                assert L.aa_table_transposed_ksize(fid, kind, 3, 4090, 0, 0.0) == 4090
            assert L.aa_table_transposed_ksize(fid, kind, 2, 20000, 1, 0.0) == -7
    assert L.aa_table_transposed_ksize(0, _lib.TABLE_F32, 0, 5, 0, 0.0) == -4  # sizes are checked first


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_dense_reference_reproduces_the_goldens(golden_backward, case):
    """A_h^T g A_w from the float64 tables is fp64 autograd's gradient of F.interpolate(antialias=True) (backward.npz) to 1e-12, and is
    oracle.backward; with the fp32 tables it is the fp32 oracle within the derived bound."""
    go = golden_backward[f"{case}_go"]
    h, w = (int(v) for v in golden_backward[f"{case}_in_hw"])
    oh, ow = go.shape[2:]
    for filt in ("linear", "cubic"):
        mats = [R.dense(filt, h, oh, False, np.float64), R.dense(filt, w, ow, False, np.float64)]
        gi, ab = R.backward_dense(mats, go)
        assert gi.shape == (go.shape[0], go.shape[1], h, w)
        assert np.abs(gi - golden_backward[f"{case}_{filt}_gi"]).max() < 1e-12, (case, filt)
        assert R.worst_ratio(oracle.backward(filt, go, (h, w)), gi, R.bound(mats, ab, np.float64)) < 1.0, (case, filt)
        go32 = go.astype(np.float32)
        mats32 = [R.dense(filt, h, oh, False, np.float32), R.dense(filt, w, ow, False, np.float32)]
        gi32, ab32 = R.backward_dense(mats32, go32)
        assert R.worst_ratio(oracle.backward(filt, go32, (h, w)), gi32, R.bound(mats32, ab32, np.float32)) < 1.0, (case, filt)
        assert np.abs(gi32 - golden_backward[f"{case}_{filt}_gi"]).max() < 1e-4


def test_dense_reference_properties():
    """Rows of A sum to 1 (each output is a weighted mean); the nonfinite variant equals the plain one on finite gradients and keeps a
    NaN / inf inside the inputs whose weight on it is not zero."""
    rng = np.random.default_rng(3)
    for name in R.FILTERS:
        for n_in, n_out, ac in ((61, 17, False), (20, 90, False), (33, 40, True), (1, 9, False), (9, 1, True)):
            a = R.dense(name, n_in, n_out, ac, np.float64)
            assert np.abs(a.sum(axis=1) - 1.0).max() < 1e-12, (name, n_in, n_out, ac)
    a_h, a_w = R.dense("cubic", 30, 12, False, np.float32), R.dense("cubic", 25, 60, False, np.float32)
    g = rng.standard_normal((1, 2, 12, 60))
    gi, ab = R.backward_dense([a_h, a_w], g)
    gi2, ab2 = R.backward_dense_nonfinite(a_h, a_w, g)
    assert np.array_equal(gi, gi2) and np.array_equal(ab, ab2)
    g[0, 1, 5, 30] = np.inf
    g[0, 0, 2, 7] = np.nan
    gi3, _ = R.backward_dense_nonfinite(a_h, a_w, g)
    assert np.array_equal(np.isnan(gi3[0, 0]), np.outer(a_h[2] != 0, a_w[7] != 0)) and not np.isnan(gi3[0, 1]).any()
    assert np.array_equal(np.isinf(gi3[0, 1]), np.outer(a_h[5] != 0, a_w[30] != 0)) and not np.isinf(gi3[0, 0]).any()
    assert np.array_equal(gi3[0, 1] == -np.inf, np.outer(a_h[5], a_w[30]) < 0)
    ok = np.isfinite(gi3)
    assert np.array_equal(gi3[ok], gi[ok])
