"""Dense float64 reference of the backward (the adjoint of the antialiased resample), shared by test_backward_cpu.py and
test_backward_gpu.py.  Plain numpy; not a test module.

For one axis (filter, n_in, n_out, align_corners, dtype, scale) `dense()` gives the forward matrix A [n_out, n_in] in float64, holding
the weights of the table kind the kernel under test reads (fp32 weights for fp32 kernels, widened exactly):

  * linear, cubic, box: oracle.weights (the C restatement of the reference, pinned to the reference build's tables);
  * Hamming, Lanczos: the arithmetic of tests/golden/make_golden_filters.py (f32_table / f64_table, which test_filters_cpu.py pins to
    the fixture) with the scale as a parameter, so that align_corners and explicit scale factors are covered as well; for the plain
    scale the two are compared bit for bit in test_backward_cpu.py.  Never the device tables.

The backward of a 2-D forward is then  gi[n, c] = A_h^T . g[n, c] . A_w  (axis by axis for 1-D and 3-D), and

    |got - gi| <= (t_h + t_w + 4) . u . (|A_h|^T . |g| . |A_w|)            element by element,

with t_h, t_w the largest numbers of non-zeros in a column of A_h, A_w (the longest transposed rows) and u = 2^-24 (fp32) or 2^-53
(fp64): the first-order bound for a sum of t_h terms, each a rounded sum of t_w rounded products stored once in the working precision.
It holds in any summation order, so for the atomic form too; the weights are the kernel's own, so no weight-rounding term enters.
Where a whole column of A is zero the bound is 0: the kernel must produce exactly 0.
For fp32 kernels the float64 reference is exact at the bound's scale.  For fp64 kernels it is itself a float64 evaluation, 0.2-0.3 of
the bound away from a long-double one, so an fp64 err / bound is the sum of two roundings (DESIGN.md has the observed figures).
"""
from __future__ import annotations

import math

import numpy as np

import kit_golden
import oracle

FILTERS = ("linear", "cubic", "box", "hamming", "lanczos")
FILTER_ID = {"linear": 0, "cubic": 1, "box": 2, "hamming": 3, "lanczos": 4}
INTERP_SIZE = {"linear": 2, "cubic": 4, "box": 1, "hamming": 2, "lanczos": 6}  # 2 x support
UNIT = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
MAX_KSIZE = 4096  # AA_MAX_KSIZE


M = kit_golden.generator("filters")


# ---- one axis ---------------------------------------------------------------------------------------------------------
def axis_scale(n_in: int, n_out: int, align_corners: bool, dtype, scale: float = 0.0):
    """ATen's area_pixel_compute_scale<scalar_t>: a numpy scalar of `dtype`.  `scale` > 0 is a user scale factor (the ratio becomes
    1 / scale unless align_corners)."""
    t = np.dtype(dtype).type
    if align_corners:
        return t(n_in - 1) / t(n_out - 1) if n_out > 1 else t(0.0)
    if scale and scale > 0.0:
        return t(1.0 / scale)
    return t(n_in) / t(n_out)


def windows(name: str, n_in: int, n_out: int, align_corners: bool = False, dtype=np.float32, scale: float = 0.0):
    """-> (xmin int64[out], xsize int64[out]): the reference's window arithmetic for all outputs at once, every promotion as in
    make_golden_filters.f32_table / f64_table (products in double, narrowed to scalar_t; the window ends truncated from double)."""
    t = np.dtype(dtype).type
    interp = INTERP_SIZE[name]
    s = axis_scale(n_in, n_out, align_corners, dtype, scale)
    support = t((interp * 0.5) * float(s)) if s >= 1.0 else t(interp * 0.5)
    center = (float(s) * (np.arange(n_out, dtype=np.float64) + 0.5)).astype(t)
    xmin = np.maximum(np.trunc((center - support).astype(np.float64) + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc((center + support).astype(np.float64) + 0.5).astype(np.int64), n_in)
    return xmin, xmax - xmin


def _pillow_filter_table(name: str, n_in: int, n_out: int, align_corners: bool, dtype, scale: float):
    """make_golden_filters.f32_table / f64_table with the scale as a parameter."""
    f = M.FILTER_FN[name]
    t = np.dtype(dtype).type
    interp = INTERP_SIZE[name]
    s = axis_scale(n_in, n_out, align_corners, dtype, scale)
    support = t((interp * 0.5) * float(s)) if s >= 1.0 else t(interp * 0.5)
    ksize = int(math.ceil(np.float32(support))) * 2 + 1
    invscale = t(1.0 / float(s)) if s >= 1.0 else t(1.0)
    xmin_a, xsize_a = windows(name, n_in, n_out, align_corners, dtype, scale)
    w = np.zeros((n_out, ksize), t)
    is32 = np.dtype(dtype) == np.float32
    for i in range(n_out):
        center = t(float(s) * (i + 0.5))
        xmin, n = int(xmin_a[i]), min(int(xsize_a[i]), ksize)
        if n <= 0:
            continue
        if is32:
            row = np.empty(n, np.float32)
            for j in range(n):
                d = np.float32(np.float32(j + xmin) - center)
                arg = np.float32((float(d) + 0.5) * float(invscale))
                row[j] = np.float32(f(float(arg)))
            tot = np.float32(0.0)
            for j in range(n):
                tot = np.float32(tot + row[j])
            if tot != 0.0:
                row = (row.astype(np.float64) / float(tot)).astype(np.float32)
        else:
            row = np.array([f(((j + xmin) - float(center) + 0.5) * float(invscale)) for j in range(n)], np.float64)
            tot = 0.0
            for v in row:
                tot += float(v)
            if tot != 0.0:
                row = row / tot
        w[i, :n] = row
    return ksize, xmin_a, xsize_a, w


def axis_table(name: str, n_in: int, n_out: int, align_corners: bool = False, dtype=np.float32, scale: float = 0.0):
    """-> (ksize, xmin, xsize, w[out, ksize]) in `dtype`."""
    if name in ("hamming", "lanczos"):
        return _pillow_filter_table(name, n_in, n_out, align_corners, dtype, scale)
    return oracle.weights(name, n_in, n_out, align_corners, dtype, scale)


def dense(name: str, n_in: int, n_out: int, align_corners: bool = False, dtype=np.float32, scale: float = 0.0) -> np.ndarray:
    """The forward matrix A [n_out, n_in], float64 (the `dtype` weights widened exactly)."""
    k, xmin, xsize, w = axis_table(name, n_in, n_out, align_corners, dtype, scale)
    a = np.zeros((n_out, n_in), np.float64)
    j = np.arange(k)[None, :]
    mask = j < np.minimum(xsize, k)[:, None]
    rows = np.broadcast_to(np.arange(n_out)[:, None], mask.shape)
    cols = np.asarray(xmin)[:, None] + j
    a[rows[mask], cols[mask]] = w[mask].astype(np.float64)
    return a


def cover(xmin, xsize, n_in: int) -> np.ndarray:
    """int64[n_in]: how many outputs' windows [xmin, xmin + max(xsize, 1)) hold each input index (the range the transposed table
    stores for it; a window without taps counts as one entry, as in the device kernel)."""
    lo = np.clip(np.asarray(xmin, np.int64), 0, n_in)
    hi = np.clip(np.asarray(xmin, np.int64) + np.maximum(np.asarray(xsize, np.int64), 1), 0, n_in)
    d = np.bincount(lo, minlength=n_in + 1) - np.bincount(hi, minlength=n_in + 1)
    return np.cumsum(d)[:n_in]


def monotone(xmin, xsize) -> bool:
    """Window starts and ends never move backwards: what makes the outputs holding one input index a contiguous range."""
    xmin = np.asarray(xmin, np.int64)
    end = xmin + np.maximum(np.asarray(xsize, np.int64), 1)
    return bool(np.all(np.diff(xmin) >= 0) and np.all(np.diff(end) >= 0))


def capacity_estimate(name: str, n_in: int, n_out: int, align_corners: bool, dtype, scale: float = 0.0) -> int:
    """aa_table_transposed_ksize restated: ceil((2 support + 1) / scale) + 3 clipped to [1, n_out] (before the 4096 limit)."""
    s = float(axis_scale(n_in, n_out, align_corners, dtype, scale))
    interp = INTERP_SIZE[name]
    support = interp * 0.5 * s if s >= 1.0 else interp * 0.5
    tk = (int(math.ceil((2.0 * support + 1.0) / s)) + 3) if s > 0.0 else n_out
    return max(1, min(tk, n_out))


# ---- the backward -----------------------------------------------------------------------------------------------------
def max_column_count(a: np.ndarray) -> int:
    return max(1, int((a != 0).sum(axis=0).max()))


def backward_dense(mats, g: np.ndarray):
    """mats: one A per resampled axis (the trailing len(mats) axes of g, in order).  -> (gi, absref) in float64:
    gi = g contracted with A along each axis (A_h^T . g . A_w in 2-D), absref the same with |A| and |g|."""
    gi = np.asarray(g, np.float64)
    ab = np.abs(gi)
    nd = len(mats)
    for k, a in enumerate(mats):
        ax = gi.ndim - nd + k
        gi = np.moveaxis(np.tensordot(gi, a, axes=([ax], [0])), -1, ax)
        ab = np.moveaxis(np.tensordot(ab, np.abs(a), axes=([ax], [0])), -1, ax)
    return gi, ab


def bound(mats, absref: np.ndarray, dtype) -> np.ndarray:
    t = sum(max_column_count(a) for a in mats)
    return (t + 4) * UNIT[np.dtype(dtype)] * absref


def worst_ratio(got: np.ndarray, gi: np.ndarray, bnd: np.ndarray) -> float:
    """max err / bound over the elements with a non-zero bound; inf when an element whose bound is 0 is not exactly 0 (or when
    anything is not finite)."""
    err = np.abs(np.asarray(got, np.float64) - gi)
    if not np.all(np.isfinite(err)):
        return float("inf")
    zero = bnd == 0
    if np.any(err[zero] != 0):
        return float("inf")
    if np.all(zero):
        return 0.0
    return float((err[~zero] / bnd[~zero]).max())


def backward_dense_nonfinite(a_h: np.ndarray, a_w: np.ndarray, g: np.ndarray):
    """2-D backward of a gradient holding inf / nan, with the zero entries of A SKIPPED (not multiplied: 0 x inf would put a NaN
    everywhere).  -> (gi with nan / +-inf where they belong, absref of the finite part)."""
    g = np.asarray(g, np.float64)
    fin = np.isfinite(g)
    gi, ab = backward_dense([a_h, a_w], np.where(fin, g, 0.0))
    nz_h, nz_w = (a_h != 0).astype(np.float64), (a_w != 0).astype(np.float64)
    nan = backward_dense([nz_h, nz_w], np.isnan(g).astype(np.float64))[0] > 0
    pos = np.zeros(gi.shape, bool)
    neg = np.zeros(gi.shape, bool)
    for idx in np.argwhere(np.isinf(g)):
        *lead, o, p = (int(v) for v in idx)
        sgn = np.outer(np.sign(a_h[o]), np.sign(a_w[p])) * np.sign(g[tuple(idx)])
        pos[tuple(lead)] |= sgn > 0
        neg[tuple(lead)] |= sgn < 0
    nan |= pos & neg
    gi[pos] = np.inf
    gi[neg] = -np.inf
    gi[nan] = np.nan
    return gi, ab
