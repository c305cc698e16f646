"""The activations of the return path without a GPU: aa_exp against float64 under the cap the exhaustive sweep gave (tools/exp_sweep.py,
DESIGN.md), softmax and sigmoid against float64 under derived bounds, every special value, the planners with an activation through
ctypes (host arithmetic only), and the argument checks of the two Python calls that come before any device work."""
import ctypes

import numpy as np
import pytest
import torch

import activation_ref as act
import resize_many_back_merged_ref as ref
from interpolate_antialiasing_amd import _lib
from interpolate_antialiasing_amd import extension_interpolate as aa

U = 2.0 ** -24
# tools/exp_sweep.py over all 1 118 568 449 float32 of [-86, 0]: the largest error is 0.991551 ulp, at x = -81.39176177978516
# (bits 0xc2a2c895).  The cap is that figure rounded up to the next quarter ulp.
SWEEP_WORST_X = np.array([0xC2A2C895], np.uint32).view(np.float32)[0]
EXP_CAP_ULP = 1.0
ERR_BAD_DTYPE, ERR_BAD_SHAPE = -2, -4
PTR = 4096  # a dummy device address: the planners never follow it
NONE, SOFTMAX, SIGMOID = 0, 1, 2
INF, NAN = np.float32(np.inf), np.float32(np.nan)


def f32(*v):
    return np.array(v, np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---- aa_exp ---------------------------------------------------------------------------------------------------------------------------
def test_aa_exp_against_float64():
    rng = np.random.default_rng(1)
    x = np.concatenate([-86.0 * rng.random(1 << 20), -2.0 * rng.random(1 << 18), [-86.0, -0.0, 0.0, float(SWEEP_WORST_X)]]).astype(np.float32)
    got = act.aa_exp(x)
    assert got.dtype == np.float32
    err = act.ulp_error(got, np.exp(x.astype(np.float64)))
    worst = int(np.argmax(err))
    at_sweeps = float(err[-1])
    print(f"aa_exp: {x.size} points, largest error {err[worst]:.6f} ulp at x = {float(x[worst])!r}; at the sweep's worst argument {at_sweeps:.6f} ulp")
    assert float(SWEEP_WORST_X) == -81.39176177978516 and abs(at_sweeps - 0.991551) < 1e-6, "the sweep's worst argument reproduces its figure"
    assert err.max() <= EXP_CAP_ULP


def test_aa_exp_edges():
    assert bits(act.aa_exp(f32(0.0, -0.0))).tolist() == bits(f32(1.0, 1.0)).tolist()
    below = np.nextafter(np.float32(-86.0), -INF)
    assert bits(act.aa_exp(f32(below, -87.0, -1e30, -INF))).tolist() == [0, 0, 0, 0], "+0 below -86"
    assert act.aa_exp(f32(-86.0))[0] > 0
    assert np.isnan(act.aa_exp(f32(NAN)))[0]
    # no non-zero subnormal result: the smallest is aa_exp(-86), a normal number; the densest look at the bottom of the domain
    x = np.arange(int(f32(-80.0).view(np.uint32)[0]), int(f32(-86.0).view(np.uint32)[0]) + 1, dtype=np.uint32).view(np.float32)
    got = act.aa_exp(x)
    assert got.min() == act.aa_exp(f32(-86.0))[0] and got.min() >= np.finfo(np.float32).tiny
    print(f"the smallest non-zero result is {got.min():.6e}")


# ---- softmax --------------------------------------------------------------------------------------------------------------------------
def softmax64(v):
    v = v.astype(np.float64)
    e = np.exp(v - v.max(axis=0))
    return e / e.sum(axis=0)


@pytest.mark.parametrize("sigma", (1.0, 8.0))
@pytest.mark.parametrize("k", (1, 2, 19, 150))
def test_softmax_against_float64(k, sigma):
    """|P - softmax64| <= (K + 8) * 2^-24: K sequentially rounded adds of the denominator, one division, one product, a 1-ulp exp (two
    half-ulps) and the rounding of v - m, which costs at most 2^-24 / e absolute because x e^-x <= 1 / e."""
    v = (sigma * np.random.default_rng(100 * k + int(sigma)).standard_normal((k, 4096))).astype(np.float32)
    p = act.softmax(v)
    assert p.dtype == np.float32 and p.shape == v.shape
    err = float(np.abs(p.astype(np.float64) - softmax64(v)).max())
    rows = float(np.abs(p.astype(np.float64).sum(axis=0) - 1.0).max())
    print(f"softmax K = {k} sigma {sigma}: largest error {err:.3e}, rows from 1 by {rows:.3e}, bound {(k + 8) * U:.3e}")
    assert err <= (k + 8) * U
    assert rows <= (k + 8) * U
    if k == 1:
        assert (bits(p) == bits(f32(1.0))[0]).all()


def test_softmax_special_values():
    def col(*v):
        return act.softmax(f32(*v).reshape(-1, 1))[:, 0]

    # a -inf logit (a masked class) gets +0, wherever it stands, and the others are the softmax of the rest
    rest = col(1.0, 2.0, 0.5)
    for at in range(4):
        v = [1.0, 2.0, 0.5]
        v.insert(at, -INF)
        p = col(*v)
        assert bits(p[at:at + 1])[0] == 0
        assert bits(np.delete(p, at)).tolist() == bits(rest).tolist()
    # a NaN anywhere, a +inf anywhere, nothing but -inf: NaN in every class
    for v in ((NAN, 1.0, 2.0), (1.0, NAN, 2.0), (1.0, 2.0, NAN), (INF, 1.0, 2.0), (1.0, INF, 2.0), (1.0, 2.0, INF), (INF, INF, 1.0), (INF, -INF, 0.0),
              (-INF, -INF, -INF), (-INF, NAN, INF)):
        assert np.isnan(col(*v)).all(), v
    # K = 1: 1.0, or NaN for a non-finite logit
    assert bits(col(3.5)).tolist() == bits(f32(1.0)).tolist() and bits(col(-1e30)).tolist() == bits(f32(1.0)).tolist()
    for v in (NAN, INF, -INF):
        assert np.isnan(col(v)).all(), v
    # differences beyond the cutoff are exact zeros, and small products are subnormal numbers, kept
    p = col(0.0, -87.0, -90.0)
    assert p[0] == 1.0 and bits(p[1:]).tolist() == [0, 0]
    p = act.softmax(np.concatenate([np.zeros(8, np.float32), f32(-85.5)]).reshape(-1, 1))[:, 0]
    assert 0 < p[8] < np.finfo(np.float32).tiny, "aa_exp(-85.5) / 8 is a subnormal number"
    # the restatement is the prose's loop, pixel by pixel
    v = (8 * np.random.default_rng(3).standard_normal((19, 64))).astype(np.float32)
    v[3, 5], v[0, 6], v[18, 7] = -INF, -INF, -INF
    p = act.softmax(v)
    for j in range(v.shape[1]):
        m, d = v[0, j], np.float32(1.0)
        for k in range(1, 19):
            if v[k, j] > m:
                d = np.float32(np.float32(d * act.aa_exp(np.float32(m - v[k, j]))) + np.float32(1.0))
                m = v[k, j]
            else:
                d = np.float32(d + act.aa_exp(np.float32(v[k, j] - m)))
        rcp = np.float32(np.float32(1.0) / d)
        want = [np.float32(act.aa_exp(np.float32(v[k, j] - m)) * rcp) for k in range(19)]
        assert bits(p[:, j]).tolist() == bits(np.array(want, np.float32)).tolist(), j


# ---- sigmoid --------------------------------------------------------------------------------------------------------------------------
def test_sigmoid():
    """|P - sigmoid64| <= 4 * 2^-24: a 1-ulp exp (two half-ulps, relative), the rounding of 1 + e and the division, on a value of at
    most 1."""
    v = np.concatenate([8 * np.random.default_rng(4).standard_normal(1 << 18), [0.0, -0.0, 90.0, -90.0, 1e30, -1e30]]).astype(np.float32)
    p = act.sigmoid(v)
    assert p.dtype == np.float32
    with np.errstate(over="ignore"):
        want = 1.0 / (1.0 + np.exp(-v.astype(np.float64)))
    err = float(np.abs(p.astype(np.float64) - want).max())
    print(f"sigmoid: largest error {err:.3e}, bound {4 * U:.3e}")
    assert err <= 4 * U
    assert bits(act.sigmoid(f32(0.0, -0.0))).tolist() == bits(f32(0.5, 0.5)).tolist()
    assert bits(act.sigmoid(f32(INF, -INF, 90.0, -90.0))).tolist() == bits(f32(1.0, 0.0, 1.0, 0.0)).tolist()
    assert np.isnan(act.sigmoid(f32(NAN)))[0]
    # the prose, element by element
    for x in f32(-3.25, 0.75, -86.5, 17.0):
        e = act.aa_exp(np.float32(-abs(x)))
        want = np.float32((np.float32(1.0) if x >= 0 else e) / np.float32(np.float32(1.0) + e))
        assert bits(act.sigmoid(x)).tolist() == bits(want).tolist()
    assert ((p >= 0) & (p <= 1)).all()


def test_merged_probabilities_compose_the_definition():
    """Per member the activation of R_i, then merge_members: a group of one member is the activated item, for both merges, and
    activation=None is merged_values."""
    args = ("cubic", ref.BASE_CANVAS, ref.BASE_REGIONS, ref.BASE_GROUPS, ref.BASE_SIZES, ref.BASE_FLIPS)
    vals = ref.member_values(*args)
    for a in act.ACTIVATIONS:
        for merge in ("sum", "mean"):
            got = act.merged_probabilities(*args, merge=merge, activation=a)
            want = ref.merge_members([act.apply(a, v) for v in vals], ref.BASE_GROUPS, 3, merge)
            assert all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))
            sizes = [ref.BASE_SIZES[g] for g in ref.BASE_GROUPS]
            one = act.merged_probabilities("cubic", ref.BASE_CANVAS, ref.BASE_REGIONS, list(range(7)), sizes, ref.BASE_FLIPS, merge, a)
            assert all(np.array_equal(bits(g), bits(act.apply(a, v))) for g, v in zip(one, vals))
    none = act.merged_probabilities(*args)
    assert all(np.array_equal(bits(g), bits(w)) for g, w in zip(none, ref.merged_values(*args)))
    # the activation shows: the sum of softmax members is not the softmax of the summed members
    s = act.merged_probabilities(*args, activation="softmax")[0]
    assert np.abs(s - act.softmax(ref.merged_values(*args)[0])).max() > 0.1
    assert np.abs(s.sum(axis=0) - 3.0).max() < 1e-5  # (three members' rows of 1)


# ---- the planners ---------------------------------------------------------------------------------------------------------------------
def records(n, oh=3, ow=4, k=7):
    recs = (_lib.BackItemIn * max(n, 1))()
    for i, r in enumerate(recs):
        r.data_dev, r.stride_ch, r.stride_row, r.stride_px, r.h, r.w, r.oh, r.ow, r.flags = PTR + 4 * i, 54, 9, 1, 6, 9, oh, ow, i % 2
    return recs


def plan_many(n, activation, k=7, reduce=_lib.BACK_VALUES, out_dtype=_lib.F32):
    """aa_back_many_plan (activation "old") or aa_back_many_plan_act -> (rc, the block's bytes, its buffer)."""
    L = _lib.load()
    nbytes = L.aa_back_many_desc_bytes(n)
    buf = (ctypes.c_uint8 * nbytes)()
    ws, arena, offs = ctypes.c_size_t(0), ctypes.c_size_t(0), (ctypes.c_int64 * max(n, 1))()
    tail = (out_dtype, ctypes.addressof(buf), nbytes, ctypes.byref(ws), ctypes.byref(arena), offs)
    if activation == "old":
        rc = L.aa_back_many_plan(_lib.FILTER_CUBIC, _lib.NCHW, n, k, records(n, k=k), reduce, *tail)
    else:
        rc = L.aa_back_many_plan_act(_lib.FILTER_CUBIC, _lib.NCHW, n, k, records(n, k=k), reduce, activation, *tail)
    return rc, bytes(buf), buf


def plan_merged(groups, activation, k=7, merge=0, reduce=_lib.BACK_VALUES, out_dtype=_lib.F32):
    L = _lib.load()
    n, g = len(groups), max(groups) + 1
    nbytes = L.aa_back_merged_desc_bytes(n, g)
    buf = (ctypes.c_uint8 * nbytes)()
    ws, arena, offs = ctypes.c_size_t(0), ctypes.c_size_t(0), (ctypes.c_int64 * g)()
    group_of = (ctypes.c_int64 * n)(*groups)
    tail = (out_dtype, ctypes.addressof(buf), nbytes, ctypes.byref(ws), ctypes.byref(arena), offs)
    if activation == "old":
        rc = L.aa_back_merged_plan(_lib.FILTER_CUBIC, _lib.NCHW, n, k, records(n, k=k), g, group_of, merge, reduce, *tail)
    else:
        rc = L.aa_back_merged_plan_act(_lib.FILTER_CUBIC, _lib.NCHW, n, k, records(n, k=k), g, group_of, merge, reduce, activation, *tail)
    return rc, bytes(buf), buf


def test_abi():
    L = _lib.load()
    assert L.aa_abi_version() == 3
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    for sym in ("aa_back_many_plan_act", "aa_back_merged_plan_act"):
        assert sym in _lib.EXPORTS and hasattr(L, sym) and sym + "(" in header
        assert sym in header.split("#define AA_INTERP_ABI_VERSION 3")[1].split("*/")[0]  # (listed in the version's comment)
    assert _lib.BACK_ACT == {None: NONE, "softmax": SOFTMAX, "sigmoid": SIGMOID} and _lib.BACK_ACT_MEMBERS == act.MAX_SOFTMAX_MEMBERS == 16
    assert "AA_BACK_ACT_NONE = 0, AA_BACK_ACT_SOFTMAX = 1, AA_BACK_ACT_SIGMOID = 2" in header


@pytest.mark.parametrize("reduce,out_dtype", [(_lib.BACK_VALUES, _lib.BF16), (_lib.BACK_ARGMAX, _lib.U8), (_lib.BACK_GREATER, _lib.BOOL)])
def test_activation_zero_writes_the_old_planners_bytes(reduce, out_dtype):
    rc0, old, _ = plan_many(5, "old", reduce=reduce, out_dtype=out_dtype)
    rc1, new, _ = plan_many(5, NONE, reduce=reduce, out_dtype=out_dtype)
    assert rc0 == rc1 == 0 and old == new
    groups = [0, 1, 0, 2, 1]
    for merge in (0, 1):
        rc0, old, _ = plan_merged(groups, "old", merge=merge, reduce=reduce, out_dtype=out_dtype)
        rc1, new, _ = plan_merged(groups, NONE, merge=merge, reduce=reduce, out_dtype=out_dtype)
        assert rc0 == rc1 == 0 and old == new


def test_the_headers_hold_the_activation_and_nothing_else_changes():
    _, zero, _ = plan_many(5, NONE)
    _, zero_merged, _ = plan_merged([0, 1, 0, 2, 1], NONE)
    for a in (SOFTMAX, SIGMOID):
        rc, got, buf = plan_many(5, a)
        hd = _lib.back_desc_view(buf, 5)[0]
        assert rc == 0 and hd.reserved0 == a and hd.reserved == 0
        off = _lib.BackHeader.reserved0.offset
        assert got[:off] == zero[:off] and got[off + 4:] == zero[off + 4:]
        rc, got, buf = plan_merged([0, 1, 0, 2, 1], a)
        hd = _lib.back_merged_desc_view(buf, 5, 3)[0]
        assert rc == 0 and hd.reserved == a
        off = _lib.BackMergedHeader.reserved.offset
        assert got[:off] == zero_merged[:off] and got[off + 4:] == zero_merged[off + 4:]


def test_unknown_activations_are_refused():
    for a in (-1, 3, 7, 1 << 20):
        assert plan_many(5, a)[0] == ERR_BAD_SHAPE, a
        assert plan_merged([0, 1, 0], a)[0] == ERR_BAD_SHAPE, a
    # beside the reduce check: before a label type that cannot hold K - 1 is looked at, after the filter and the layout
    L = _lib.load()
    assert L.aa_back_many_plan_act(9, _lib.NCHW, 1, 7, records(1), 0, 5, _lib.F32, None, 0, None, None, None) == -1
    assert L.aa_back_many_plan_act(_lib.FILTER_CUBIC, 9, 1, 7, records(1), 0, 5, _lib.F32, None, 0, None, None, None) == -3
    assert L.aa_back_many_plan_act(_lib.FILTER_CUBIC, _lib.NCHW, 1, 7, records(1), 0, 5, _lib.F32, None, 0, None, None, None) == ERR_BAD_SHAPE
    # a block whose activation was damaged after planning is no plan's block
    # The control: every call below also names an in_dtype that is not built, which is the NEXT check after the header's.  The block as
    # planned gets past the header to it (AA_ERR_BAD_DTYPE); damaged, it does not — so it is the activation check that answers.
    one = ctypes.c_void_p(256)
    rc, _, buf = plan_many(2, SIGMOID)
    assert L.aa_resample_back_many(ctypes.addressof(buf), one, _lib.F64, 0.0, one, 1 << 20, one, 1 << 20, None) == ERR_BAD_DTYPE
    for bad in (3, -1):
        _lib.back_desc_view(buf, 2)[0].reserved0 = bad
        assert L.aa_resample_back_many(ctypes.addressof(buf), one, _lib.F64, 0.0, one, 1 << 20, one, 1 << 20, None) == ERR_BAD_SHAPE
        assert L.aa_resample_back_many(ctypes.addressof(buf), one, _lib.F32, 0.0, one, 1 << 20, one, 1 << 20, None) == ERR_BAD_SHAPE
    rc, _, buf = plan_merged([0, 0], SIGMOID)
    assert L.aa_resample_back_merged(ctypes.addressof(buf), one, _lib.F64, 0.0, one, 1 << 20, one, 1 << 20, None) == ERR_BAD_DTYPE
    for bad in (3, -1):
        _lib.back_merged_desc_view(buf, 2, 1)[0].reserved = bad
        assert L.aa_resample_back_merged(ctypes.addressof(buf), one, _lib.F64, 0.0, one, 1 << 20, one, 1 << 20, None) == ERR_BAD_SHAPE
        assert L.aa_resample_back_merged(ctypes.addressof(buf), one, _lib.F32, 0.0, one, 1 << 20, one, 1 << 20, None) == ERR_BAD_SHAPE


def test_the_softmax_member_limit():
    sixteen, seventeen = [0] * 16 + [1], [1] + [0] * 17
    assert plan_merged(sixteen, SOFTMAX)[0] == 0
    assert plan_merged(seventeen, SOFTMAX)[0] == ERR_BAD_SHAPE
    assert plan_merged(seventeen, SIGMOID)[0] == 0 and plan_merged(seventeen, NONE)[0] == 0 and plan_merged(seventeen, "old")[0] == 0
    # a plan damaged into a 17-member softmax group is refused by the launch as well, before anything is enqueued
    # (the control: with an in_dtype that is not built, the next check, the sigmoid plan of 17 and a softmax plan of 16 get past the
    # header to AA_ERR_BAD_DTYPE; the plan damaged into a softmax of 17 does not, so it is the member check that answers)
    call, one = _lib.load().aa_resample_back_merged, ctypes.c_void_p(256)
    rc, _, buf = plan_merged(seventeen, SIGMOID)
    assert call(ctypes.addressof(buf), one, _lib.F64, 0.0, one, 1 << 30, one, 1 << 30, None) == ERR_BAD_DTYPE
    _lib.back_merged_desc_view(buf, 18, 2)[0].reserved = SOFTMAX
    assert call(ctypes.addressof(buf), one, _lib.F64, 0.0, one, 1 << 30, one, 1 << 30, None) == ERR_BAD_SHAPE
    assert call(ctypes.addressof(buf), one, _lib.F32, 0.0, one, 1 << 30, one, 1 << 30, None) == ERR_BAD_SHAPE
    rc, _, buf = plan_merged(sixteen, SOFTMAX)
    assert call(ctypes.addressof(buf), one, _lib.F64, 0.0, one, 1 << 30, one, 1 << 30, None) == ERR_BAD_DTYPE
    # the Python call names the group
    p = torch.zeros(18, 3, 4, 4)
    with pytest.raises(ValueError, match=r"group 0 \(sizes\[0\]\) has 17 members.*at most 16"):
        aa.resize_many_back_merged(p, seventeen, [(5, 5), (5, 5)], activation="softmax")
    for a in ("sigmoid", None):
        with pytest.raises(_lib.AAInterpError, match="no CPU implementation"):
            aa.resize_many_back_merged(p, seventeen, [(5, 5), (5, 5)], activation=a)
    with pytest.raises(_lib.AAInterpError, match="no CPU implementation"):
        aa.resize_many_back_merged(p[:17], sixteen, [(5, 5), (5, 5)], activation="softmax")


# ---- the Python calls' checks, before any device work ---------------------------------------------------------------------------------
def test_argument_errors():
    p = torch.zeros(4, 7, 12, 16)
    sizes = [(5, 6)] * 4
    for bad in ("Softmax", "log_softmax", "relu", 1, True, ("softmax",)):
        with pytest.raises(ValueError, match="activation must be None, 'softmax' or 'sigmoid'"):
            aa.resize_many_back(p, sizes, activation=bad)
        with pytest.raises(ValueError, match="activation must be None, 'softmax' or 'sigmoid'"):
            aa.resize_many_back_merged(p, [0, 1, 0, 1], sizes[:2], activation=bad)
    with pytest.raises(TypeError):
        aa.resize_many_back(p, sizes, "bilinear", None, None, None, 0.0, None, None, "softmax")  # (keyword-only)
    # not differentiable: refused, naming the two ways out, rather than detached
    for a in act.ACTIVATIONS:
        g = p.clone().requires_grad_()
        for call in (lambda x: aa.resize_many_back(x, sizes, activation=a), lambda x: aa.resize_many_back_merged(x, [0, 1, 0, 1], sizes[:2], activation=a)):
            with pytest.raises(NotImplementedError, match=r"torch\.no_grad\(\).*\.detach\(\)"):
                call(g)
            with pytest.raises(NotImplementedError, match="not differentiable"):
                call([g[0], p[1], p[2], p[3]])
            # under no_grad, detached, or with a reduction that carries no gradient: only the device is missing
            with torch.no_grad(), pytest.raises(_lib.AAInterpError, match="no CPU implementation"):
                call(g)
            with pytest.raises(_lib.AAInterpError, match="no CPU implementation"):
                call(g.detach())
        for reduce in ("argmax", "greater"):
            with pytest.raises(_lib.AAInterpError, match="no CPU implementation"):
                aa.resize_many_back(g, sizes, activation=a, reduce=reduce)
            with pytest.raises(_lib.AAInterpError, match="no CPU implementation"):
                aa.resize_many_back_merged(g, [0, 1, 0, 1], sizes[:2], activation=a, reduce=reduce)
    # N == 0
    assert aa.resize_many_back([], [], channels=3, activation="softmax") == []
    assert aa.resize_many_back_merged([], [], [], channels=3, activation="sigmoid", reduce="argmax") == []
