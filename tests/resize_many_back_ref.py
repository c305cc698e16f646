"""The definition of resize_many_back restated on the CPU, shared by test_resize_many_back_cpu.py, test_resize_many_back_gpu.py and
test_resize_many_back_guard_gpu.py.  Plain numpy; not a test module.

  * values: per item oracle.forward (the C restatement of the reference's fp32 arithmetic, three filters) of the region's contiguous
    copy as a [1, K, h, w] image at (oh, ow), mirrored left to right where the item flips;
  * labels: numpy.argmax over axis 0 of those fp32 values (the lowest index of the greatest value; the first NaN wins);
  * masks: values > float32(threshold);
  * dense_values: the same in float64 from backward_ref.dense's matrices (all five filters), with resize_embed_ref's forward bound
    element by element, (t_h + t_w + 4) . 2^-24 . absref, t the longest row of A_h, A_w (the taps of one output).
"""
from __future__ import annotations

import numpy as np

import backward_ref
import kit_golden
import oracle

U = 2.0 ** -24
ORACLE_FILTERS = ("linear", "cubic", "box")
FILTERS = ("linear", "cubic", "box", "hamming", "lanczos")

# ---- the cases: (canvas or list of sources, regions, sizes) -------------------------------------------------------------------------------
BASE_CANVAS = kit_golden.readonly(np.random.default_rng(7).standard_normal((5, 7, 12, 16)).astype(np.float32))
# both axes up; both down (antialiased); a one-pixel source to a row wider than a tile; a single column, one axis each way; the identity
BASE_REGIONS = [(0, 0, 12, 16), (1, 2, 6, 9), (3, 0, 1, 1), (0, 5, 12, 1), (2, 3, 5, 7)]
BASE_SIZES = [(23, 31), (3, 4), (4, 300), (13, 5), (5, 7)]
IDENTITY_ITEM = 4
BASE_PIXELS = sum(oh * ow for oh, ow in BASE_SIZES)  # 2025; 6075 over the oracle's three filters


def tie_canvas() -> np.ndarray:
    """The base canvas with plane 4 a copy of plane 2 and plane 6 the constant 0.25: class 4 never wins under the lowest-index rule, and
    a constant plane resamples to exactly 0.25 wherever the weights sum to 1 without rounding."""
    c = np.array(BASE_CANVAS)
    c[:, 4] = c[:, 2]
    c[:, 6] = 0.25
    return kit_golden.readonly(c)


def k_canvas(k: int) -> np.ndarray:
    return kit_golden.readonly(np.random.default_rng(70 + k).standard_normal((5, k, 12, 16)).astype(np.float32))


def k300_case():
    """K = 300 on a 3 x 3 source to (5, 4), plane 299 raised by 10 at one source pixel: labels above 255."""
    c = np.random.default_rng(300).standard_normal((1, 300, 3, 3)).astype(np.float32)
    c[0, 299, 1, 2] += 10.0
    return kit_golden.readonly(c), [(0, 0, 3, 3)], [(5, 4)]


def seventy_case():
    """N = 70 items of at most 3 x 3 to at most 4 x 4 (the item search passes 64), every item a region of its own slice of one batch."""
    c = kit_golden.readonly(np.random.default_rng(70).standard_normal((70, 3, 3, 3)).astype(np.float32))
    regions = [(i % 2, (i // 2) % 2, 1 + (i // 4) % 2 + (1 - i % 2), 1 + (i // 8) % 2 + (1 - (i // 2) % 2)) for i in range(70)]
    sizes = [(1 + i % 4, 1 + (i // 4) % 4) for i in range(70)]
    return c, regions, sizes


def list_case():
    """Separately allocated items of different (H_i, W_i), K = 3."""
    rng = np.random.default_rng(11)
    shapes = [(4, 9), (7, 3), (1, 5), (6, 6)]
    srcs = [kit_golden.readonly(rng.standard_normal((3, h, w)).astype(np.float32)) for h, w in shapes]
    return srcs, [None, (1, 0, 5, 3), None, (2, 1, 3, 4)], [(9, 17), (3, 2), (2, 11), (3, 4)]


def nonfinite_canvas() -> np.ndarray:
    """The base canvas with one NaN (item 0's region, class 3) and one +inf (class 5, also inside item 1's region)."""
    c = np.array(BASE_CANVAS)
    c[0, 3, 5, 6] = np.nan
    c[0, 5, 9, 12] = np.inf
    c[1, 5, 3, 4] = np.inf
    c[1, 1, 4, 7] = np.nan
    return kit_golden.readonly(c)


# ---- the definition with the oracle's fp32 arithmetic -----------------------------------------------------------------------------------
def view(src, region) -> np.ndarray:
    """Item's [K, H, W] source (a slice of a batch or a list entry) and its region -> the contiguous [K, h, w] copy."""
    if region is None:
        return np.ascontiguousarray(src)
    y0, x0, h, w = region
    return np.ascontiguousarray(src[:, y0:y0 + h, x0:x0 + w])


def values(filt: str, srcs, regions, sizes, flips=None):
    """-> [float32 [K, oh_i, ow_i]]: the fp32 values of every item."""
    out = []
    for i, (src, size) in enumerate(zip(srcs, sizes)):
        v = view(src, regions[i] if regions is not None else None).astype(np.float32)
        r = oracle.forward(filt, v[None], size)[0]
        out.append(np.ascontiguousarray(r[:, :, ::-1]) if flips is not None and flips[i] else r)
    return out


def labels(vals, dtype=np.int64):
    return [np.argmax(v, axis=0).astype(dtype) for v in vals]


def masks(vals, threshold: float):
    with np.errstate(invalid="ignore"):
        return [v > np.float32(threshold) for v in vals]


# ---- the dense float64 form and its bound -----------------------------------------------------------------------------------------------
def _max_row_count(a: np.ndarray) -> int:
    return max(1, int((a != 0).sum(axis=1).max()))


def dense_values(filt: str, srcs, regions, sizes, flips=None):
    """-> ([float64 [K, oh_i, ow_i]], [the bound element by element])."""
    want, bnd = [], []
    for i, (src, (oh, ow)) in enumerate(zip(srcs, sizes)):
        v = view(src, regions[i] if regions is not None else None).astype(np.float64)
        a_h, a_w = backward_ref.dense(filt, v.shape[1], oh), backward_ref.dense(filt, v.shape[2], ow)
        r = np.einsum("oy,kyx,px->kop", a_h, v, a_w)
        ab = np.einsum("oy,kyx,px->kop", np.abs(a_h), np.abs(v), np.abs(a_w))
        b = (_max_row_count(a_h) + _max_row_count(a_w) + 4) * U * ab
        if flips is not None and flips[i]:
            r, b = r[:, :, ::-1], b[:, :, ::-1]
        want.append(r)
        bnd.append(b)
    return want, bnd


def worst_ratio(got, want, bnd) -> float:
    return max(backward_ref.worst_ratio(g, w, b) for g, w, b in zip(got, want, bnd))


def decided(want, bnd):
    """Per item the pixels whose float64 top-two margin exceeds twice the bound there (the largest of the K bounds of the pixel): any fp32
    result within the bound has the float64 argmax.  -> ([bool [oh, ow]], [float64 argmax])."""
    ok, arg = [], []
    for w, b in zip(want, bnd):
        arg.append(np.argmax(w, axis=0))
        if w.shape[0] == 1:
            ok.append(np.ones(w.shape[1:], bool))
            continue
        top = np.sort(w, axis=0)
        ok.append(top[-1] - top[-2] > 2.0 * b.max(axis=0))
    return ok, arg


# ---- dtypes -----------------------------------------------------------------------------------------------------------------------------
def to_bf16_bits(a: np.ndarray) -> np.ndarray:
    """float32 -> the uint16 bits of its bfloat16, rounded to nearest even (finite values)."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
