"""The definition of resize_many_back_panoptic restated in numpy, shared by its CPU and GPU tests.  Not a test module.

It starts from p [Q, oh, ow] float32 as the EXISTING call returns it — resize_many_back(..., activation="sigmoid", reduce=None,
out_dtype=float32): there is no second source of truth for the resample or the sigmoid.  The rest is a float32 product, the argmax rule
(the lowest kept q of the greatest value, a NaN greater than every number and the first NaN kept), integer counts and one float64
division.  Everything is compared for equality."""
import numpy as np


def panoptic(p: np.ndarray, scores: np.ndarray, ids=None, void: int = -1, overlap_threshold: float = 0.8, dtype=np.int32):
    """p [Q, oh, ow] float32, scores [Q] float32 -> (map [oh, ow] of dtype, counts [Q, 3] int64, survives [Q] bool)."""
    assert p.dtype == np.float32 and scores.dtype == np.float32
    q = p.shape[0]
    with np.errstate(invalid="ignore"):
        kept = np.flatnonzero(scores > 0)
        counts, survives = np.zeros((q, 3), np.int64), np.zeros(q, bool)
        out = np.full(p.shape[1:], void, dtype)
        if kept.size == 0:
            return out, counts, survives
        v = scores[kept, None, None] * p[kept]  # (float32 times float32: one rounded product)
        assert v.dtype == np.float32
        at = np.argmax(v, axis=0)  # (numpy's rule is the call's: the first of the greatest, the first NaN before any number)
        winner = kept[at]
        inside = np.take_along_axis(p[kept], at[None], 0)[0] >= np.float32(0.5)
        for k in kept:
            won = winner == k
            counts[k] = (won.sum(), (p[k] >= np.float32(0.5)).sum(), (won & inside).sum())
    ids = np.arange(q, dtype=np.int32) if ids is None else ids
    for k in kept:
        area, original, inter = (int(c) for c in counts[k])
        survives[k] = area > 0 and original > 0 and inter > 0 and area / original >= float(overlap_threshold)
        if survives[k]:
            out[(winner == k) & inside] = np.asarray(ids[k]).astype(dtype)
    return out, counts, survives


def pattern(name: str, n: int, q: int) -> np.ndarray:
    """[N, Q] float32 scores in [0.3, 1), no two alike, zeroed by the kept pattern: "all"; "none0" (item 0 keeps nothing); "one" (query
    Q // 2 only); "edges" (queries 3 and 4, either side of a chunk edge, and the last; fewer where Q is small)."""
    s = np.random.default_rng(500 + q).uniform(0.3, 1.0, (n, q)).astype(np.float32)
    keep = np.ones((n, q), bool)
    if name == "none0":
        keep[0] = False
        keep[1:, ::3] = False
    elif name == "one":
        keep[:] = False
        keep[:, q // 2] = True
    elif name == "edges":
        keep[:] = False
        keep[:, [k for k in (3, 4, q - 1) if k < q]] = True
    else:
        assert name == "all"
    return np.where(keep, s, np.float32(0.0))
