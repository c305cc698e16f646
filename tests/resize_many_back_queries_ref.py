"""The definition of resize_many_back_queries restated in numpy, shared by its CPU and GPU tests.  Not a test module.

With R the fp32 resample of an item's Q masks (what the EXISTING call returns: resize_many_back(..., reduce=None, out_dtype=float32) —
there is no second source of truth for the resample) and w its [Q, C] float32 weights, the operands are defined bit for bit,
P = float16(activation_ref.sigmoid(R)) and Wh = float16(w), and the scores are S[c] = sum_q Wh[q, c] * P[q] with exact products and an
fp32 sum whose order is the kernel's own.  So S is compared with the float64 sum under the bound Q * 2^-23 * sum_q |Wh * P| per
element: twice the first-order bound of a plain fp32 summation, because the matrix unit's internal rounding is undocumented."""
import numpy as np

import activation_ref
import resize_many_back_ref as back_ref

F16_TINY = 2.0 ** -14  # the smallest normal float16: the matrix unit may take anything smaller as zero


def weights(n: int, q: int, c: int, sign: float = 1.0) -> np.ndarray:
    """[N, Q, C] float32 in sign * [0.05, 1): probabilities' range, no two alike."""
    return (sign * np.random.default_rng(1000 * q + c).uniform(0.05, 1.0, (n, q, c))).astype(np.float32)


def operands(R: np.ndarray, w: np.ndarray):
    """-> (P [Q, oh, ow], Wh [Q, C]) as float64 values of float16 numbers; neither holds a float16 subnormal."""
    assert np.abs(R).max() <= 8.0, "logits within +-8: the sigmoid stays a normal float16"
    assert ((w == 0) | (np.abs(w) >= F16_TINY)).all()
    return activation_ref.sigmoid(R).astype(np.float16).astype(np.float64), w.astype(np.float16).astype(np.float64)


def scores(R: np.ndarray, w: np.ndarray):
    """-> (the float64 scores [C, oh, ow], their bound element by element)."""
    p, wh = operands(R, w)
    return np.einsum("qc,qyx->cyx", wh, p), R.shape[0] * 2.0 ** -23 * np.einsum("qc,qyx->cyx", np.abs(wh), np.abs(p))


def decided(want, bnd):
    """resize_many_back_ref.decided with this bound: the pixels at which every result within the bound has the float64 argmax."""
    return back_ref.decided(want, bnd)
