"""The definition of resize_embed_to_tokens and its backward restated on the CPU, shared by test_resize_embed_cpu.py,
test_resize_embed_gpu.py and test_resize_embed_guard_gpu.py.  Plain numpy; not a test module.

  * packed_forward: per item oracle.forward (the C restatement of the reference's fp32 arithmetic) of the grid as a [1, D, H0, W0]
    image, cut into token rows and concatenated (or padded with +0.0 to L rows an item);
  * ordered_backward: acc = b_0, acc = acc + b_i in float32 in ascending order, b_i = oracle.backward of item i's rows;
  * dense_forward / dense_backward: the same two in float64 from backward_ref.dense's matrices, with the element-wise error bounds

        forward   (t_h + t_w + 4) . u . absref                    t: the longest row of A_h, A_w (the taps of one output)
        backward  sum_i (t_h,i + t_w,i + 4) . u . absref_i  +  (N - 1) . u . sum_i absref_i        t: the longest column, as backward_ref

    u = 2^-24: each item's two-pass sum to first order (backward_ref's reasoning), plus one rounding of magnitude at most the partial
    sum's for each of the N - 1 additions across items.  Where a bound is 0 the result must be exactly 0.

oracle has the reference's three filters; the dense forms have all five (backward_ref.axis_table)."""
from __future__ import annotations

import numpy as np

import backward_ref
import kit_golden
import oracle

U = 2.0 ** -24

BASE_SOURCE = (5, 7)
# identity, a single token, one axis up and one down, windows wider than the source, a single row, a single column
BASE_GRIDS = [(5, 7), (1, 1), (3, 11), (12, 4), (2, 9), (7, 7), (1, 13), (10, 1)]
D_VALUES = (1, 5, 8, 520, 523)  # below a vector and odd; a whole number of vectors; more than one wave, without and with a tail
# (source, grids) beyond the base case: a 1 x 1 source, a 16 x 16 one to a tall, an equal and a flat grid, N = 1, repeated grids, and
# N = 70 grids of at most 3 x 3 (the item search passes 64 items)
FURTHER = {
    "source_1x1": ((1, 1), [(1, 1), (4, 3), (1, 9), (6, 1)]),
    "source_16x16": ((16, 16), [(37, 3), (16, 16), (1, 40)]),
    "one_item": ((5, 7), [(3, 11)]),
    "repeated": ((5, 7), [(3, 11), (5, 7), (3, 11), (3, 11), (5, 7)]),
    "seventy": ((4, 3), [(1 + i % 3, 1 + (i // 3) % 3) for i in range(70)]),
}


def offsets(grids):
    out = [0]
    for gh, gw in grids:
        out.append(out[-1] + gh * gw)
    return out


def embed_values(h0: int, w0: int, d: int, seed: int = 0) -> np.ndarray:
    """A [H0, W0, D] float32 grid of normal values, read-only."""
    return kit_golden.readonly(np.random.default_rng(1000 + seed).standard_normal((h0, w0, d)).astype(np.float32))


def grad_values(grids, d: int, seed: int = 0) -> np.ndarray:
    """A packed [sum T_i, D] float32 gradient of normal values, read-only."""
    return kit_golden.readonly(np.random.default_rng(2000 + seed).standard_normal((offsets(grids)[-1], d)).astype(np.float32))


def pad_rows(packed: np.ndarray, grids, pad_to: int, fill=0.0) -> np.ndarray:
    """[sum T_i, D] -> [N, L, D], `fill` beyond T_i."""
    off = offsets(grids)
    out = np.full((len(grids), pad_to, packed.shape[1]), fill, packed.dtype)
    for i in range(len(grids)):
        out[i, :off[i + 1] - off[i]] = packed[off[i]:off[i + 1]]
    return out


# ---- the definition with the oracle's fp32 arithmetic ---------------------------------------------------------------------------------
def item_forward(filt: str, embed: np.ndarray, grid) -> np.ndarray:
    """[H0, W0, D] float32 -> item's [gh * gw, D] float32 token rows."""
    gh, gw = grid
    img = np.ascontiguousarray(embed.transpose(2, 0, 1)[None])
    return np.ascontiguousarray(oracle.forward(filt, img, (gh, gw))[0].transpose(1, 2, 0)).reshape(gh * gw, embed.shape[2])


def packed_forward(filt: str, embed: np.ndarray, grids, pad_to=None) -> np.ndarray:
    d = embed.shape[2]
    packed = np.concatenate([item_forward(filt, embed, g) for g in grids]) if grids else np.zeros((0, d), np.float32)
    return packed if pad_to is None else pad_rows(packed, grids, pad_to)


def ordered_backward(filt: str, grad: np.ndarray, embed_size, grids) -> np.ndarray:
    """grad [sum T_i, D] float32 -> [H0, W0, D] float32: acc = b_0, acc = acc + b_i."""
    h0, w0, d = embed_size
    off = offsets(grids)
    acc = None
    for i, (gh, gw) in enumerate(grids):
        g = np.ascontiguousarray(grad[off[i]:off[i + 1]].reshape(gh, gw, d).transpose(2, 0, 1)[None], dtype=np.float32)
        b = oracle.backward(filt, g, (h0, w0)).astype(np.float32)
        acc = b if acc is None else (acc + b).astype(np.float32)
    if acc is None:
        return np.zeros((h0, w0, d), np.float32)
    return np.ascontiguousarray(acc[0].transpose(1, 2, 0))


# ---- the dense float64 forms and their bounds -----------------------------------------------------------------------------------------
def _mats(filt: str, embed_hw, grid):
    return backward_ref.dense(filt, embed_hw[0], grid[0]), backward_ref.dense(filt, embed_hw[1], grid[1])


def _max_row_count(a: np.ndarray) -> int:
    return max(1, int((a != 0).sum(axis=1).max()))


def dense_forward(filt: str, embed: np.ndarray, grids):
    """-> (packed [sum T_i, D] float64, the bound element by element)."""
    e = np.asarray(embed, np.float64)
    want, bnd = [], []
    for g in grids:
        a_h, a_w = _mats(filt, embed.shape[:2], g)
        want.append(np.einsum("oy,yxd,px->opd", a_h, e, a_w).reshape(g[0] * g[1], -1))
        ab = np.einsum("oy,yxd,px->opd", np.abs(a_h), np.abs(e), np.abs(a_w)).reshape(g[0] * g[1], -1)
        bnd.append((_max_row_count(a_h) + _max_row_count(a_w) + 4) * U * ab)
    return np.concatenate(want), np.concatenate(bnd)


def dense_backward(filt: str, grad: np.ndarray, embed_size, grids):
    """-> (grad_embed [H0, W0, D] float64, the bound element by element)."""
    h0, w0, d = embed_size
    off = offsets(grids)
    want = np.zeros((h0, w0, d))
    bnd = np.zeros((h0, w0, d))
    absum = np.zeros((h0, w0, d))
    for i, (gh, gw) in enumerate(grids):
        a_h, a_w = _mats(filt, (h0, w0), (gh, gw))
        g = np.asarray(grad[off[i]:off[i + 1]], np.float64).reshape(gh, gw, d).transpose(2, 0, 1)
        gi, ab = backward_ref.backward_dense([a_h, a_w], g)
        want += gi.transpose(1, 2, 0)
        bnd += backward_ref.bound([a_h, a_w], ab, np.float32).transpose(1, 2, 0)
        absum += ab.transpose(1, 2, 0)
    return want, bnd + max(len(grids) - 1, 0) * U * absum


def worst_ratio(got, want, bnd) -> float:
    return backward_ref.worst_ratio(got, want, bnd)
