#!/usr/bin/env python3
"""The fused 16-bit channels_last forward (fused_f16_nhwc / fused_bf16_nhwc) beside what it replaces and its neighbours, in one process on
one GPU: [64,3,438,906] -> [196,320] bilinear and bicubic and -> [96,120] bilinear, fp16 and bf16.  Per workload, ms per call of

    new      the 16-bit channels_last batch, fused kernels on
    generic  the same batch with set_fused(0): the two-launch path with its fp32 intermediate
    f32nhwc  the same values as fp32 channels_last (fused_f32_nhwc)
    nchw16   the same values as 16-bit planes (fused_*_nchw)

Each figure is the median of ROUNDS rounds of REPS calls, the four alternated inside a round; the spread column is (max - min) / median
of `new` and of `generic` over the rounds.  Outputs of new and generic are compared bit for bit first.  GPU only.

    python tools/half_nhwc_bench.py [batch] [--reps 400] [--rounds 7]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from interpolate_antialiasing_amd import _lib, extension_interpolate as aa  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("batch", nargs="?", type=int, default=64)
ap.add_argument("--reps", type=int, default=400)
ap.add_argument("--rounds", type=int, default=7)
args = ap.parse_args()
assert torch.cuda.is_available(), "needs a GPU"


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


torch.manual_seed(0)
base = torch.rand(args.batch, 438, 906, 3, device="cuda") * 255
print(f"# batch {args.batch}, 438x906x3; ms per call, median of {args.rounds} rounds of {args.reps} calls; spread = (max - min) / median", flush=True)
for dt, tag in ((torch.float16, "f16"), (torch.bfloat16, "bf16")):
    x16 = base.to(dt).permute(0, 3, 1, 2)              # channels_last
    x32 = x16.float()                                    # channels_last, the same values
    xpl = x16.contiguous()                               # planes
    for op, fname, size in ((aa.linear_forward, "bilinear", [196, 320]), (aa.cubic_forward, "bicubic", [196, 320]), (aa.linear_forward, "bilinear", [96, 120])):
        runs = {"new": (x16, 1), "generic": (x16, 0), "f32nhwc": (x32, 1), "nchw16": (xpl, 1)}
        variant, out = {}, {}
        for key, (x, mode) in runs.items():  # warm-up, variants, and the outputs to compare
            prev = _lib.set_fused(mode)
            try:
                for _ in range(3):
                    out[key] = op(x, size)
                variant[key] = _lib.last_variant()
            finally:
                _lib.set_fused(prev)
        torch.cuda.synchronize()
        same = torch.equal(out["new"].contiguous().view(torch.int16), out["generic"].contiguous().view(torch.int16))
        ms = {k: [] for k in runs}
        for _ in range(args.rounds):
            for key, (x, mode) in runs.items():
                prev = _lib.set_fused(mode)
                try:
                    ms[key].append(timed(lambda: op(x, size), args.reps))
                finally:
                    _lib.set_fused(prev)
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
        print(f"{tag:4s} {fname:8s} ->{size[0]:4d}x{size[1]:<4d} new {med['new']:7.4f} ({variant['new']}) generic {med['generic']:7.4f} ({variant['generic']}) "
              f"f32nhwc {med['f32nhwc']:7.4f} ({variant['f32nhwc']}) nchw16 {med['nchw16']:7.4f} ({variant['nchw16']}) generic/new x{med['generic'] / med['new']:5.2f} "
              f"spread new {spread['new'] * 100:4.1f}% generic {spread['generic'] * 100:4.1f}% bits_equal {same}", flush=True)
        print("     rounds new     " + " ".join(f"{v:.4f}" for v in ms["new"]), flush=True)
        print("     rounds generic " + " ".join(f"{v:.4f}" for v in ms["generic"]), flush=True)
        del out
    del x16, x32, xpl
    torch.cuda.empty_cache()
