#!/usr/bin/env python3
"""Throughput map: which kernel ran and at what speed, per filter x shape x dtype / layout / arithmetic, beside the generic two-launch
path (set_fused(0)) timed in the same process, the two alternated.  GPU only; writes one line per case.

    python tools/perf_map.py [batch] [--filters linear,cubic] [--shapes test|filters]

--shapes test (default): test.py's five output sizes of its 438x906 images (test.py:15-21).  --shapes filters: the shapes that reach
every route of the fused uint8 kernel for Pillow's Hamming / Lanczos (tests/golden/make_golden_filters.py's list); the batch is
scaled per shape to move about as many input bytes as `batch` 438x906 images.

--alpha: straight-alpha RGBA / LA (alpha=True) per route instead: the fused alpha kernel against the plain 4-channel kernel on the same
shape (alpha=False) and against the set_fused(0) three-step route (premultiply, generic resample, un-premultiply), at the batch given per
shape (1024 RGBA images at 438x906 -> 196x320 bilinear is the headline)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from interpolate_antialiasing_amd import _lib, extension_interpolate as aa  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("batch", nargs="?", type=int, default=128)
ap.add_argument("--filters", default="linear,cubic", help="comma-separated: linear, cubic, box, hamming, lanczos")
ap.add_argument("--shapes", default="test", choices=("test", "filters"))
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--alpha", action="store_true")
args = ap.parse_args()

B = args.batch
H, W = 438, 906
OPS = {"linear": aa.linear_forward, "cubic": aa.cubic_forward, "box": aa.nearest_forward, "hamming": aa.hamming_forward,
       "lanczos": aa.lanczos_forward}
if args.shapes == "test":
    SHAPES = [("test", (H, W), (oh, ow)) for (ow, oh) in [(320, 196), (460, 220), (120, 96), (1200, 196), (120, 1200), (1200, 1200)]]
else:
    SHAPES = [("narrow", (438, 906), (220, 460)), ("narrow", (438, 906), (196, 1200)), ("narrow", (1080, 1920), (720, 1280)),
              ("narrow", (1000, 1000), (999, 999)), ("narrow", (512, 512), (384, 384)), ("wide", (438, 906), (196, 320)),
              ("split", (438, 906), (96, 120)), ("split", (2160, 3840), (224, 224)), ("up", (438, 906), (1200, 1200)),
              ("up", (196, 320), (438, 906))]


def timed(fn, reps):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def fused_and_generic(fn, reps):
    """-> (fused ms, fused variant, generic ms, generic variant): two alternating rounds each, the faster of each kept."""
    best = {1: (1e30, ""), 0: (1e30, "")}
    for _ in range(2):
        for mode in (1, 0):
            prev = _lib.set_fused(mode)
            try:
                ms = timed(fn, reps)
                variant = _lib.last_variant()
            finally:
                _lib.set_fused(prev)
            if ms < best[mode][0]:
                best[mode] = (ms, variant)
    return best[1][0], best[1][1], best[0][0], best[0][1]



def alpha_map():
    # (filter, in, out, batch, channels): the routes of alpha=True — fused narrow and six-row windows, and the fallback's wide, split,
    # growing and LA cases
    cases = [("linear", (438, 906), (196, 320), 1024, 4), ("box", (438, 906), (196, 320), 1024, 4), ("hamming", (438, 906), (196, 320), 1024, 4),
             ("lanczos", (1080, 1920), (720, 1280), 32, 4), ("cubic", (438, 906), (196, 320), 1024, 4), ("linear", (2160, 3840), (224, 224), 64, 4),
             ("linear", (438, 906), (1200, 1200), 32, 4), ("linear", (438, 906), (196, 320), 1024, 2)]
    print("# ms per call (best of 2 alternating rounds); alpha = alpha=True, set_fused(1): the fused alpha kernel, or where it declines the "
          "default three-step route (its resample is whatever fused kernel applies); plain = alpha=False, set_fused(1); fallback = alpha=True, "
          "set_fused(0): premultiply, GENERIC two-pass resample, un-premultiply", flush=True)
    for fname, (h, w), (oh, ow), b, c in cases:
        x = torch.randint(0, 256, (b, h, w, c), dtype=torch.uint8, device="cuda").permute(0, 3, 1, 2)
        op = OPS[fname]
        best = {}
        for _ in range(2):
            for key, mode, alpha in (("alpha", 1, True), ("plain", 1, False), ("fallback", 0, True)):
                prev = _lib.set_fused(mode)
                try:
                    ms = timed(lambda: op(x, [oh, ow], alpha=alpha), args.reps)
                    v = _lib.last_variant()
                finally:
                    _lib.set_fused(prev)
                if ms < best.get(key, (1e30, ""))[0]:
                    best[key] = (ms, v)
        (am, av), (pm, pv), (fm, fv) = best["alpha"], best["plain"], best["fallback"]
        print(f"{fname:7s} {h:4d}x{w:<4d}->{oh:4d}x{ow:<4d} b{b:<5d} C{c} alpha {am:8.4f} ms {av:28s} plain {pm:8.4f} ms {pv:28s} "
              f"fallback {fm:8.4f} ms  alpha/plain x{am / pm:5.2f}  fallback/alpha x{fm / am:5.2f}", flush=True)
        del x
        torch.cuda.empty_cache()


if args.alpha:
    alpha_map()
    sys.exit(0)

torch.manual_seed(0)
print(f"# batch {B} (per 438x906 image's bytes); ms per call; Mpix/s = output pixels per second; fused vs generic (set_fused(0))", flush=True)
for (tag, (h, w), (oh, ow)) in SHAPES:
    b = max(1, round(B * H * W / (h * w)))
    u8 = torch.randint(0, 256, (b, h, w, 3), dtype=torch.uint8, device="cuda").permute(0, 3, 1, 2)
    cases = [
        ("u8 nhwc pil", u8, dict(uint8_mode="pil"), 1),
        ("u8 nhwc harness", u8, dict(uint8_mode="harness"), 1),
        ("u8 nchw pil", u8.contiguous(), dict(uint8_mode="pil"), 1),
        ("f32 nchw", u8.float().contiguous(), {}, 4),
        ("f32 nhwc", u8.float().contiguous(memory_format=torch.channels_last), {}, 4),
        ("f16 nchw", u8.half().contiguous(), {}, 2),
        ("f16 nhwc", u8.half().contiguous(memory_format=torch.channels_last), {}, 2),
        ("bf16 nhwc", u8.bfloat16().contiguous(memory_format=torch.channels_last), {}, 2),
    ]
    if args.shapes == "filters":
        cases.insert(3, ("u8 nhwc->f32", u8, dict(out_dtype=torch.float32, out_format="nchw"), 1))
    for fname in args.filters.split(","):
        op = OPS[fname]
        for cname, x, kw, es in cases:
            fms, fv, gms, gv = fused_and_generic(lambda: op(x, [oh, ow], **kw), args.reps)
            mpix = b * oh * ow / 1e6
            nbytes = b * 3 * es * (h * w) + b * 3 * (4 if "f32" in cname else es) * (oh * ow)
            print(f"{fname:7s} {tag:6s} {h:4d}x{w:<4d}->{oh:4d}x{ow:<4d} b{b:<4d} {cname:16s} fused {fms:8.4f} ms {mpix / fms * 1e3:8.0f} Mpix/s "
                  f"{nbytes / fms / 1e6:6.0f} GB/s {fv:34s} generic {gms:8.4f} ms {mpix / gms * 1e3:8.0f} Mpix/s {gv:26s} x{gms / fms:5.2f}",
                  flush=True)
    del cases, u8
    torch.cuda.empty_cache()
