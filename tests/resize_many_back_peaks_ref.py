"""The definition of resize_many_back_peaks restated in numpy, shared by its CPU and GPU tests.  Not a test module.

It starts from R [K, oh, ow] float32 as the EXISTING call returns it — resize_many_back(..., reduce=None, out_dtype=float32): there is
no second source of truth for the resample.  The rest is numpy.argmax per flattened channel and five reads.  Everything is compared for
equality, the values by their bits."""
import numpy as np

import kit_golden
import resize_many_back_ref as back_ref


def peaks(r: np.ndarray):
    """r [K, oh, ow] float32 -> (xy [K, 2] int32, (x, y); values [K, 5] float32: the peak, left, right, up, down, a neighbour outside
    the image the peak itself)."""
    assert r.dtype == np.float32 and r.ndim == 3
    k, oh, ow = r.shape
    xy, values = np.zeros((k, 2), np.int32), np.zeros((k, 5), np.float32)
    for c in range(k):
        y, x = divmod(int(np.argmax(r[c].ravel())), ow)  # (the lowest index of the greatest; the first NaN; -0.0 == +0.0)
        xy[c] = (x, y)
        near = ((y, x), (y, x - 1), (y, x + 1), (y - 1, x), (y + 1, x))
        for j, (yy, xx) in enumerate(near):
            values[c, j] = r[c, yy, xx] if 0 <= yy < oh and 0 <= xx < ow else r[c, y, x]
    return xy, values


def bump_canvas(k: int) -> np.ndarray:
    """back_ref.k_canvas(k) with +10 at source pixel ((7 c) % 12, (5 c) % 16) of channel c in every batch entry: peaks spread over tiles."""
    c = np.array(back_ref.k_canvas(k))
    for ch in range(k):
        c[:, ch, (7 * ch) % 12, (5 * ch) % 16] += 10.0
    return kit_golden.readonly(c)
