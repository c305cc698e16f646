#!/usr/bin/env python3
"""aa_exp over EVERY float32 of its finite domain [-86, 0] against float64 exp: the largest error in float32 ulps and the argument
that gives it.  The restatement under test is tests/activation_ref.py's, the definition the kernels are held to; DESIGN.md records
what this prints, and tests/test_activation_cpu.py takes its cap from it.  numpy on the CPU, in chunks; about 1.1e9 values.

    python tools/exp_sweep.py [--chunk 16777216] [--jobs 4]

(float64 exp is itself within one float64 ulp, 2^-29 of a float32 ulp: it does not show in the figures.)"""
import argparse
import concurrent.futures
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import activation_ref as act  # noqa: E402

FIRST = 0x80000000  # -0.0: the bit patterns of the negative floats ascend as the floats descend
LAST = int(np.array(-86.0, np.float32).view(np.uint32))  # -86.0, the last argument that is not cut off


def sweep(lo: int, hi: int):
    """Bit patterns lo .. hi - 1 -> (count, the largest ulp error, its argument's bits, the largest relative error, the smallest result)."""
    x = np.arange(lo, hi, dtype=np.uint32).view(np.float32)
    got = act.aa_exp(x)
    exact = np.exp(x.astype(np.float64))
    err = act.ulp_error(got, exact)
    i = int(np.argmax(err))
    rel = float((np.abs(got.astype(np.float64) - exact) / exact).max())
    return hi - lo, float(err[i]), int(x[i:i + 1].view(np.uint32)[0]), rel, float(got.min())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--chunk", type=int, default=1 << 24)
    ap.add_argument("--jobs", type=int, default=4)
    a = ap.parse_args()
    bounds = list(range(FIRST, LAST + 1, a.chunk)) + [LAST + 1]
    spans = list(zip(bounds[:-1], bounds[1:]))
    count, worst, at, rel, least = 0, -1.0, 0, 0.0, np.inf
    with concurrent.futures.ProcessPoolExecutor(a.jobs) as pool:
        for j, (c, w, b, r, s) in enumerate(pool.map(sweep, *zip(*spans))):
            count += c
            if w > worst:
                worst, at = w, b
            rel, least = max(rel, r), min(least, s)
            if j % 8 == 7:
                print(f"  {count} values, largest error so far {worst:.6f} ulp", flush=True)
    # +0.0 is in the domain too
    assert act.aa_exp(np.float32(0.0)) == 1.0 and act.aa_exp(np.float32(-0.0)) == 1.0
    x = np.array([at], np.uint32).view(np.float32)[0]
    print(f"aa_exp over all {count} float32 of [-86, -0] (and +0): largest error {worst:.6f} ulp at x = {float(x)!r} (bits {at:#010x}); "
          f"largest relative error {rel:.3e}; smallest result {least:.6e} (the smallest normal number is {np.finfo(np.float32).tiny:.6e})")


if __name__ == "__main__":
    main()
