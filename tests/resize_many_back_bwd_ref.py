"""The definition of resize_many_back_backward restated on the CPU, shared by test_resize_many_back_bwd_cpu.py,
test_resize_many_back_bwd_gpu.py and test_resize_many_back_bwd_guard_gpu.py.  Plain numpy; not a test module.

Item i has a canvas (H_i, W_i), a region (y0, x0, h, w) of it, a flip and a gradient G_i [K, oh_i, ow_i] or None.  With U_i = G_i,
mirrored left to right where the item flips, its result is [K, H_i, W_i]: the backward B_i of U_i to [K, h, w] inside the region, +0.0
elsewhere, all +0.0 for a None gradient.  Three forms of B_i:

  * backward: oracle.backward (the C restatement's true adjoint, three filters).  It runs the vertical adjoint first and scatters, so
    it is the same sums in ANOTHER order than the package's gather form: equal to it within the bound below, not bit for bit;
  * gather_backward: the gather form itself in float32 from oracle.weights' tables (three filters) — the adjoint rows as
    aa_table_rows.h's table_transpose_one builds them, the horizontal adjoint pass first, a float32 intermediate, tap 0 unconditionally
    and the others in ascending order, product and sum rounded apart.  This is the definition the GPU is held to bit for bit;
  * dense_backward: float64 from backward_ref.dense's matrices (all five filters), with backward_ref.bound element by element,
    (t_h + t_w + 4) . 2^-24 . absref, t the longest column of A_h, A_w; 0 outside the regions: exactly zero is required there.

The cases reuse resize_many_back_ref's geometry: BASE_CANVAS's (12, 16) with BASE_REGIONS and BASE_SIZES, list_case, seventy_case."""
from __future__ import annotations

import numpy as np

import backward_ref
import kit_golden
import oracle
import resize_many_back_ref as fwd_ref

U = 2.0 ** -24
ORACLE_FILTERS = fwd_ref.ORACLE_FILTERS
FILTERS = fwd_ref.FILTERS
BASE_HW = tuple(fwd_ref.BASE_CANVAS.shape[2:])  # (12, 16)
BASE_K = 7
BASE_REGIONS, BASE_SIZES, IDENTITY_ITEM = fwd_ref.BASE_REGIONS, fwd_ref.BASE_SIZES, fwd_ref.IDENTITY_ITEM
BASE_FLIPS = [True, False, True, False, False]
K_VALUES = (1, 3, 4, 5, 7)  # the class loop carries four classes at a time: below it, a multiple of it, and tails


def grads(sizes, k: int, seed: int = 0):
    """[float32 [K, oh_i, ow_i]] of normal values, read-only."""
    rng = np.random.default_rng(4000 + seed)
    return [kit_golden.readonly(rng.standard_normal((k, oh, ow)).astype(np.float32)) for oh, ow in sizes]


def list_case():
    """resize_many_back_ref.list_case as the backward sees it: (canvases, regions, sizes), K = 3."""
    srcs, regions, sizes = fwd_ref.list_case()
    return [tuple(s.shape[1:]) for s in srcs], regions, sizes


def seventy_case():
    """resize_many_back_ref.seventy_case as the backward sees it: (canvas (3, 3), regions, sizes), N = 70, K = 3."""
    c, regions, sizes = fwd_ref.seventy_case()
    return tuple(c.shape[2:]), regions, sizes


def long_rows_case():
    """A [2, 2, 300] region shrunk to (5, 3): adjoint rows along W of one tap or none under forward rows 100 and more floats long, and
    K = 2 below the class loop's step.  -> (canvas, regions, sizes)"""
    return (4, 310), [(1, 7, 2, 300)], [(5, 3)]


def seams_case():
    """A canvas 600 columns wide whose region [3, 598] starts at column 1 and is enlarged two-fold: it crosses every column seam of a
    work unit whatever the unit's width (every multiple of any width below 599), and the rows cross a seam too.  -> (canvas, regions,
    sizes)"""
    return (7, 600), [(2, 1, 3, 598)], [(6, 1196)]


def _rect(region, canvas):
    return (0, 0) + tuple(canvas) if region is None else tuple(region)


def _place(b, canvas, region, k):
    out = np.zeros((k,) + tuple(canvas), b.dtype)
    y0, x0, h, w = _rect(region, canvas)
    out[:, y0:y0 + h, x0:x0 + w] = b
    return out


def _items(gs, canvases, regions, flips):
    """Per item None, or (U, canvas, region): the gradient mirrored where the item flips."""
    out = []
    for i, g in enumerate(gs):
        canvas = canvases[i]
        region = regions[i] if regions is not None else None
        if g is None:
            out.append(None)
            continue
        u = np.asarray(g)
        if flips is not None and flips[i]:
            u = u[:, :, ::-1]
        out.append((np.ascontiguousarray(u), canvas, region))
    return out


def canvases_of(canvas, n):
    return [tuple(canvas)] * n if len(canvas) == 2 and not isinstance(canvas[0], (tuple, list)) else [tuple(c) for c in canvas]


# ---- the true adjoint of the C restatement ------------------------------------------------------------------------------------------------
def backward(filt: str, gs, canvas, regions, flips=None, k=None):
    """-> [float32 [K, H_i, W_i]] with oracle.backward."""
    cv = canvases_of(canvas, len(gs))
    k = k if k is not None else next(g.shape[0] for g in gs if g is not None)
    out = []
    for i, it in enumerate(_items(gs, cv, regions, flips)):
        if it is None:
            out.append(np.zeros((k,) + cv[i], np.float32))
            continue
        u, c, region = it
        _, _, h, w = _rect(region, c)
        out.append(_place(oracle.backward(filt, u.astype(np.float32)[None], (h, w))[0], c, region, k))
    return out


# ---- the gather form, bit for bit -------------------------------------------------------------------------------------------------------
def adjoint_rows(filt: str, n_in: int, n_out: int):
    """The adjoint table of the float32 forward table n_in -> n_out as table_transpose_one builds it and table_row reads it: per input
    index x the first output `start` of its row and the row's float32 weights (at least one: a row without taps is one weight 0)."""
    ks, xmin, xsize, w = oracle.weights(filt, n_in, n_out, False, np.float32)
    xmin, xsize = np.asarray(xmin, np.int64), np.asarray(xsize, np.int64)
    end = xmin + np.maximum(xsize, 1)
    rows = []
    for x in range(n_in):
        first = int(np.searchsorted(end, x, side="right"))  # the first o with xmin[o] + max(xsize[o], 1) > x
        stop = int(np.searchsorted(xmin, x, side="right"))  # the first o with xmin[o] > x
        cnt = max(stop - first, 0)
        if cnt == 0:
            start = first if first < n_out else n_out - 1
            rows.append((min(max(start, 0), n_out - 1), np.zeros(1, np.float32)))
            continue
        ws = np.array([w[o, x - xmin[o]] if x - xmin[o] < ks else 0.0 for o in range(first, first + cnt)], np.float32)
        rows.append((min(first, n_out - cnt), ws))
    return rows


def _gather_axis(u: np.ndarray, rows) -> np.ndarray:
    """u [..., n_out] float32 -> [..., n_in]: per input index the sum over its adjoint row, tap 0 assigned, the others added in order."""
    out = np.empty(u.shape[:-1] + (len(rows),), np.float32)
    for x, (start, ws) in enumerate(rows):
        acc = (u[..., start] * ws[0]).astype(np.float32)
        for t in range(1, len(ws)):
            acc = (acc + (u[..., start + t] * ws[t]).astype(np.float32)).astype(np.float32)
        out[..., x] = acc
    return out


def gather_backward(filt: str, gs, canvas, regions, flips=None, k=None):
    """-> [float32 [K, H_i, W_i]]: the package's gather form in float32, the horizontal adjoint pass first."""
    cv = canvases_of(canvas, len(gs))
    k = k if k is not None else next(g.shape[0] for g in gs if g is not None)
    out = []
    for i, it in enumerate(_items(gs, cv, regions, flips)):
        if it is None:
            out.append(np.zeros((k,) + cv[i], np.float32))
            continue
        u, c, region = it
        _, _, h, w = _rect(region, c)
        oh, ow = u.shape[1:]
        t = _gather_axis(u.astype(np.float32), adjoint_rows(filt, w, ow))                         # [K, oh, w]
        b = _gather_axis(np.ascontiguousarray(t.transpose(0, 2, 1)), adjoint_rows(filt, h, oh))   # [K, w, h]
        out.append(_place(np.ascontiguousarray(b.transpose(0, 2, 1)), c, region, k))
    return out


# ---- the dense float64 form and its bound -----------------------------------------------------------------------------------------------
def dense_backward(filt: str, gs, canvas, regions, flips=None, k=None):
    """-> ([float64 [K, H_i, W_i]], [the bound element by element])."""
    cv = canvases_of(canvas, len(gs))
    k = k if k is not None else next(g.shape[0] for g in gs if g is not None)
    want, bnd = [], []
    for i, it in enumerate(_items(gs, cv, regions, flips)):
        if it is None:
            want.append(np.zeros((k,) + cv[i]))
            bnd.append(np.zeros((k,) + cv[i]))
            continue
        u, c, region = it
        _, _, h, w = _rect(region, c)
        mats = [backward_ref.dense(filt, h, u.shape[1]), backward_ref.dense(filt, w, u.shape[2])]
        gi, ab = backward_ref.backward_dense(mats, u.astype(np.float64))
        want.append(_place(gi, c, region, k))
        bnd.append(_place(backward_ref.bound(mats, ab, np.float32), c, region, k))
    return want, bnd


def worst_ratio(got, want, bnd) -> float:
    return max(backward_ref.worst_ratio(g, w, b) for g, w, b in zip(got, want, bnd))
