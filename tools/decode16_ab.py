#!/usr/bin/env python3
"""A/B of the decode-adjacent forward's 16-bit output against the two-launch idiom it replaces.

Shape: bench.py's decode-adjacent one, uint8 HWC [N,906,438,3] -> NCHW [N,3,320,196] with mean / std, exact and precision='fast', for
bfloat16 and float16.  Three things are timed with device events after warm-up, ALTERNATING in one process (A B C A B C ...), so that
clock and thermal drift hit all three alike:

  A  out_dtype=float32 followed by .to(dtype)   (the idiom without the feature: two launches, a float32 tensor written and read again)
  B  out_dtype=dtype                            (one launch)
  C  out_dtype=float32 alone                    (what A's first launch costs)

Per variant the table gives the median and the min .. max over the repetitions (each repetition is the mean of --iters calls between one
pair of events).  B must not be slower than A beyond the spread A shows between its own repetitions; B against C is recorded without a
bar.  Writes the table to --out (default profiles/decode16_ab.txt) and prints it."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7, help="alternating repetitions per variant")
    ap.add_argument("--iters", type=int, default=20, help="calls per repetition")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode16_ab.txt"))
    args = ap.parse_args()

    from interpolate_antialiasing_amd import _lib
    from interpolate_antialiasing_amd import extension_interpolate as aa

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    x = torch.randint(0, 256, (args.batch, 906, 438, 3), dtype=torch.uint8, device=dev).permute(0, 3, 1, 2)

    def fwd(dtype, precision):
        return aa.linear_forward(x, [320, 196], out_dtype=dtype, out_format="nchw", mean=MEAN, std=STD, precision=precision)

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.iters):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / args.iters

    lines = [f"decode-adjacent 16-bit output, A/B in one process: uint8 HWC [{args.batch},906,438,3] -> NCHW [{args.batch},3,320,196], mean/std",
             f"{torch.cuda.get_device_name(0)}; {args.reps} alternating repetitions of {args.iters} calls, ms per call: median (min .. max)",
             "A = float32 output then .to(dtype) (two launches), B = out_dtype=dtype (one launch), C = float32 output alone", ""]
    ok = True
    for precision in ("exact", "fast"):
        for dtype in (torch.bfloat16, torch.float16):
            variants = {"A": lambda: fwd(torch.float32, precision).to(dtype), "B": lambda: fwd(dtype, precision),
                        "C": lambda: fwd(torch.float32, precision)}
            names = {}
            for k, fn in variants.items():
                for _ in range(args.warmup):
                    fn()
                names[k] = _lib.last_variant()
            torch.cuda.synchronize()
            assert torch.equal(variants["A"]().view(torch.int16), variants["B"]().view(torch.int16)) or precision == "fast"
            t = {k: [] for k in variants}
            for _ in range(args.reps):
                for k, fn in variants.items():
                    t[k].append(timed(fn))
            med = {k: statistics.median(v) for k, v in t.items()}
            spread_a = max(t["A"]) - min(t["A"])
            verdict = "ok" if med["B"] <= med["A"] + spread_a else "B SLOWER THAN A"
            ok = ok and verdict == "ok"
            lines.append(f"{precision:5s} {str(dtype).replace('torch.', ''):8s}  "
                         + "  ".join(f"{k} {med[k]:.4f} ({min(t[k]):.4f} .. {max(t[k]):.4f})" for k in "ABC")
                         + f"  B/A {med['B'] / med['A']:.3f}  B/C {med['B'] / med['C']:.3f}  [{verdict}]")
            lines.append(f"{'':16s}B ran {names['B']}; A and C ran {names['C']}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
