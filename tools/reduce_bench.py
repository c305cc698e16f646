#!/usr/bin/env python3
"""Image.reduce and reducing_gap on the GPU, in one process on one GPU; writes profiles/reduce_perf_map.txt (or --out).

(a) reduce (8, 4) of a batch of 4K frames [B,3,2160,3840] uint8, channels_last and planar: ms per call and GB/s of the bytes the
    algorithm needs (input read once + output written), beside aa_probe_copy form 5 (read only) over the SAME tensor, and beside the
    share of that probe the headline uint8 kernel reaches ([B,3,438,906] -> [196,320] bilinear, channels_last, its input + output
    bytes) in the same run.  The expectation: a kernel with about one add per byte should not sit below the headline kernel's share.
(b) cubic_forward(x, [224,224], reducing_gap=2.0) against cubic_forward(x, [224,224]) on the same 4K batch, alternated inside each
    round.  The gate: the two-step call is faster by more than the larger of the two calls' own median-to-min spread.

Every figure: median and min over ROUNDS rounds of REPS calls timed with device events, after a warm-up of every shape.  GPU only.

    python tools/reduce_bench.py [batch] [--reps 20] [--rounds 7] [--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from interpolate_antialiasing_amd import _lib, extension_interpolate as aa  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("batch", nargs="?", type=int, default=32)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reduce_perf_map.txt"))
args = ap.parse_args()
assert torch.cuda.is_available(), "needs a GPU"
assert args.rounds >= 5, "at least 5 rounds"
B = args.batch
L = _lib.load()
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def rounds_of(fns, reps):
    """{name: [ms per call, one per round]}, the functions alternated inside every round, after a warm-up of each."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            ms[k].append(timed(fn, reps))
    return ms


def med_min(v):
    return statistics.median(v), min(v)


say(f"# {torch.cuda.get_device_name(0)}; batch {B}; ms per call: median / min of {args.rounds} rounds of {args.reps} calls (device events)")
torch.manual_seed(0)
frames = torch.randint(0, 256, (B, 2160, 3840, 3), dtype=torch.uint8, device="cuda").permute(0, 3, 1, 2)  # channels_last 4K frames
nbytes = frames.numel()
stream = torch.cuda.current_stream().cuda_stream
sink = torch.empty(max(1 << 20, nbytes // 4096 + 4096), dtype=torch.uint8, device="cuda")  # (form 5 may write one dword per 16 KiB read)

# ---- (a) reduce beside the read-only probe and the headline kernel's share of it
say()
say("# (a) reduce (8, 4) of [B,3,2160,3840]: bytes = input + output; probe = aa_probe_copy form 5 (read only) over the same tensor")
head = torch.randint(0, 256, (B, 438, 906, 3), dtype=torch.uint8, device="cuda").permute(0, 3, 1, 2)
head_bytes = head.numel() + B * 3 * 196 * 320
for tag, x in (("channels_last", frames), ("planar", frames.contiguous())):
    out_bytes = B * 3 * (2160 // 4) * (3840 // 8)
    ms = rounds_of({"reduce": lambda: aa.reduce(x, (8, 4)),
                    "probe": lambda: L.aa_probe_copy(x.data_ptr(), sink.data_ptr(), nbytes, 5, stream),
                    "headline": lambda: aa.linear_forward(head, [196, 320])}, args.reps)
    (r_med, r_min), (p_med, p_min), (h_med, h_min) = med_min(ms["reduce"]), med_min(ms["probe"]), med_min(ms["headline"])
    r_gbs, p_gbs, h_gbs = (nbytes + out_bytes) / r_med / 1e6, nbytes / p_med / 1e6, head_bytes / h_med / 1e6
    say(f"{tag:13s} reduce {r_med:7.4f} / {r_min:7.4f} ms = {r_gbs:7.1f} GB/s | probe {p_med:7.4f} / {p_min:7.4f} ms = {p_gbs:7.1f} GB/s | "
        f"reduce / probe {r_gbs / p_gbs:5.3f} | headline {h_med:7.4f} / {h_min:7.4f} ms = {h_gbs:7.1f} GB/s, headline / probe {h_gbs / p_gbs:5.3f} | "
        f"reduce at or above the headline's share: {r_gbs >= h_gbs}")
    if tag == "planar":
        del x

# ---- (b) the two-step thumbnail against the plain one
say()
say("# (b) cubic_forward([B,3,2160,3840] channels_last, [224,224]): plain, and reducing_gap=2.0 (reduce (8, 4), then 9 taps over 540x480)")
plain_out = aa.cubic_forward(frames, [224, 224])
v_plain = aa.last_variant()
gap_out = aa.cubic_forward(frames, [224, 224], reducing_gap=2.0)
v_gap = aa.last_variant()
diff = (plain_out.int() - gap_out.int()).abs()
ms = rounds_of({"plain": lambda: aa.cubic_forward(frames, [224, 224]), "gap": lambda: aa.cubic_forward(frames, [224, 224], reducing_gap=2.0)},
               args.reps)
(a_med, a_min), (g_med, g_min) = med_min(ms["plain"]), med_min(ms["gap"])
spread = max(a_med - a_min, g_med - g_min)
say(f"plain            {a_med:7.4f} / {a_min:7.4f} ms ({v_plain})")
say(f"reducing_gap=2.0 {g_med:7.4f} / {g_min:7.4f} ms ({v_gap} after the reduce)")
say(f"plain - gap = {a_med - g_med:7.4f} ms (x{a_med / g_med:5.2f}); larger median-to-min spread {spread:7.4f} ms; "
    f"gate (faster by more than the spread): {'PASS' if a_med - g_med > spread else 'FAIL'}")
say(f"(the two results differ by design, as in Pillow: max |plain - gap| = {int(diff.max())} counts, mean {float(diff.float().mean()):.3f})")
say("     rounds plain " + " ".join(f"{v:.4f}" for v in ms["plain"]))
say("     rounds gap   " + " ".join(f"{v:.4f}" for v in ms["gap"]))

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
