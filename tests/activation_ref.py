"""The definition of the return path's activations (resize_many_back and resize_many_back_merged, ``activation=``), restated in numpy
float32: every product and every sum is one numpy.float32 operation, rounded on its own.  csrc/aa_activation.h states the same
operations in HIP, and the GPU tests hold the kernels to these bits.  Plain numpy; not a test module.

  * aa_exp: the fp32 exponential for x <= 0 or NaN (Cephes' expf specialised to that domain);
  * sigmoid: per element, one aa_exp and one division;
  * softmax: over axis 0, two passes over the classes in ascending k — an online maximum and denominator, then the probabilities —
    vectorised over the pixels, a loop over k;
  * merged_probabilities: resize_many_back_merged_ref's members, each through the activation, then merged as that module merges.

A NaN result is a NaN: its sign and payload are not part of the definition (they follow the machine's propagation rule).
"""
from __future__ import annotations

import numpy as np

F = np.float32
EXP_CUTOFF = F(-86.0)                 # below it the result is +0: every non-zero result is a normal number (n >= -124)
EXP_LOG2E = F(1.44269504)
EXP_LN2_HI = F(0.693359375)
EXP_LN2_LO = F(-2.12194440e-4)
EXP_POLY = (F(1.9875691500e-4), F(1.3981999507e-3), F(8.3334519073e-3), F(4.1665795894e-2), F(1.6666665459e-1), F(5.0000001201e-1))
ACTIVATIONS = ("softmax", "sigmoid")
MAX_SOFTMAX_MEMBERS = 16              # csrc/aa_many_back.h AA_BACK_ACT_MEMBERS


def aa_exp(x) -> np.ndarray:
    """exp(x) in float32 for x <= 0 or NaN.  NaN -> x + x; x < -86 -> +0; else n = rint(x * log2(e)) (ties to even), r = x - n * ln2 in
    two steps, a degree-5 polynomial in Horner's form, and an exact scaling by the normal power of two 2^n."""
    x = np.asarray(x, dtype=F)
    with np.errstate(all="ignore"):
        nan = x != x
        low = x < EXP_CUTOFF
        xs = np.where(nan | low, F(0), x)
        n = np.rint(xs * EXP_LOG2E)
        r = xs - n * EXP_LN2_HI
        r = r - n * EXP_LN2_LO
        p = np.full(x.shape, EXP_POLY[0], dtype=F)
        for c in EXP_POLY[1:]:
            p = p * r + c
        y = ((p * r) * r + r) + F(1.0)
        scale = ((n.astype(np.int32) + 127) << 23).astype(np.int32).view(F)
        out = y * scale
        out = np.where(low, F(0), out)
        out = np.where(nan, x + x, out)
    assert out.dtype == F
    return out


def sigmoid(v) -> np.ndarray:
    """e = aa_exp(-|v|); q = 1 + e; (v >= 0 ? 1 : e) / q, one correctly rounded division.  NaN -> NaN, +inf -> 1, -inf -> +0."""
    v = np.asarray(v, dtype=F)
    with np.errstate(all="ignore"):
        e = aa_exp(-np.abs(v))
        q = F(1.0) + e
        out = np.where(v >= 0, F(1.0), e) / q
    assert out.dtype == F
    return out


def softmax(v) -> np.ndarray:
    """Softmax over axis 0 of v [K, ...].  Pass one, k ascending: m = v_0, d = 1; a new maximum rescales d, d = d * aa_exp(m - v_k) + 1,
    anything else adds, d = d + aa_exp(v_k - m).  Then rcp = 1 / d (NaN where m is +inf), and pass two: P_k = aa_exp(v_k - m) * rcp."""
    v = np.asarray(v, dtype=F)
    with np.errstate(all="ignore"):
        m = np.array(v[0], dtype=F)
        d = np.ones(m.shape, dtype=F)
        for k in range(1, v.shape[0]):
            gt = v[k] > m
            e = aa_exp(np.where(gt, m - v[k], v[k] - m))
            d = np.where(gt, d * e + F(1.0), d + e)
            m = np.where(gt, v[k], m)
        rcp = np.where(m == F(np.inf), F(np.nan), F(1.0) / d)
        out = np.stack([aa_exp(v[k] - m) * rcp for k in range(v.shape[0])])
    assert out.dtype == F
    return out


def apply(activation, v) -> np.ndarray:
    """P of the definition: v itself for None."""
    if activation is None:
        return np.asarray(v, dtype=F)
    return {"softmax": softmax, "sigmoid": sigmoid}[activation](v)


def merged_probabilities(filt: str, srcs, regions, groups, sizes, flips=None, merge: str = "sum", activation=None):
    """-> [float32 [K, oh_g, ow_g]] per GROUP: the members' R_i (resize_many_back_merged_ref.member_values) each through the activation,
    added in ascending item order, divided by float32(M) for the mean."""
    import resize_many_back_merged_ref as merged_ref

    vals = [apply(activation, r) for r in merged_ref.member_values(filt, srcs, regions, groups, sizes, flips)]
    return merged_ref.merge_members(vals, groups, len(sizes), merge)


def ulp_error(got, exact) -> np.ndarray:
    """|got - exact| in units of the last place of float32 at `exact` (float64, positive and normal as a float32)."""
    exact = np.asarray(exact, dtype=np.float64)
    _, e = np.frexp(exact)  # exact = f * 2^e, f in [0.5, 1): a float32 ulp there is 2^(e - 24)
    return np.ldexp(np.abs(np.asarray(got, dtype=np.float64) - exact), 24 - e)
