"""The definition of resize_many_back_instances restated in numpy, shared by its CPU and GPU tests.  Not a test module.

It starts from R [Q, oh, ow] float32 and p = sigmoid(R) as the EXISTING calls return them — resize_many_back(..., reduce=None,
out_dtype=float32) without and with activation="sigmoid": there is no second source of truth for the resample or the sigmoid.  The
rest is a comparison with 0, integer sums and minima and maxima.  Everything is compared for equality."""
import numpy as np

EMPTY = -1


def instances(r: np.ndarray, p: np.ndarray, queries):
    """r, p [Q, oh, ow] float32, queries [M] ints -> (masks [M, oh, ow] bool, their bits [M, oh, ceil(ow / 8)] uint8, stats [M, 6] int64)."""
    assert r.dtype == np.float32 and p.dtype == np.float32 and r.shape == p.shape
    q, oh, ow = r.shape
    masks, stats = np.zeros((len(queries), oh, ow), bool), np.zeros((len(queries), 6), np.int64)
    stats[:, 2], stats[:, 3] = ow, oh  # (the identities of the minima; those of the sums and the maxima are 0)
    for s, k in enumerate(int(v) for v in queries):
        if not 0 <= k < q:
            continue
        with np.errstate(invalid="ignore"):
            on = r[k] > 0  # (a NaN is false)
        masks[s] = on
        if on.any():
            terms = p[k][on].astype(np.float64) * 2.0 ** 24
            assert (terms == np.floor(terms)).all() and (terms >= 2.0 ** 23).all() and (terms <= 2.0 ** 24).all()  # exact integers: p in [0.5, 1]
            ys, xs = np.nonzero(on)
            stats[s] = (on.sum(), terms.astype(np.int64).sum(), xs.min(), ys.min(), xs.max() + 1, ys.max() + 1)
    return masks, np.packbits(masks, axis=-1, bitorder="little"), stats


def pattern(name: str, n: int, q: int, m: int) -> np.ndarray:
    """[N, M] int64 queries.  "once": every query at most once, a permutation cut to M or followed by empty slots; "repeat": random
    queries with query Q // 2 in the non-adjacent slots 0, 2 and M - 1; "empties": random queries with -1 in slot 1, Q in slot 3, and
    item 2's row all empty.  "repeat" (in slot 1) and "empties" (in slot 4; M >= 5) ask for query Q - 1 in every item that has slots."""
    rng = np.random.default_rng(600 + 1000 * q + m)
    if name == "once":
        rows = [np.concatenate([rng.permutation(q), np.full(max(m - q, 0), EMPTY)])[:m] for _ in range(n)]
        return np.stack(rows).astype(np.int64)
    assert m >= 5
    out = rng.integers(0, q, (n, m)).astype(np.int64)
    if name == "repeat":
        out[:, [0, 2, m - 1]], out[:, 1] = q // 2, q - 1
    else:
        assert name == "empties"
        out[:, 1], out[:, 3], out[:, 4] = EMPTY, q, q - 1
        out[2] = EMPTY
    return out
