#!/usr/bin/env python
"""A loader's batch — N images of N sizes, one RandomResizedCrop box each, all to 224 x 224 — three ways, alternating in one process:

  (a) the per-image loop with boxes never seen before: every call builds two box tables and reads their headers back (one stream
      synchronisation per image) — the case resize_many is for;
  (b) the same loop with fixed boxes and warm caches (the 32-entry box LRU widened so that all N pairs stay in it);
  (c) resize_many: one call per batch, fresh boxes every batch (it has no cache to warm).

and the step after it — the batch as the normalised float tensor a model reads (bicubic, NCHW, mean / std, half the items flipped; bfloat16
and float32) — two ways:

  (d) the composition: resize_many, then .float(), - mean, / std, .to(dtype), .contiguous(), an indexed .flip(-1);
  (e) resize_many_to_float: one call, the same three launches as (c).

(e) must beat (d) by more than the two spreads together; both give the same bits.

--placed, on the same N images, two recipes a loader has besides RandomResizedCrop, each against the loop a user writes without the
placed call: <mode>_forward(img[None], [vh, vw]) per image (tables warm in the cache: the sizes do not change), a slice copy into a
preallocated batch, and for eval the torch conversion of the batch:

  eval       Resize(256) + CenterCrop(224): fit_sizes(shorter=256), canvas 224 x 224, "center", bicubic, bfloat16 NCHW with mean / std;
  letterbox  fit_sizes(longer=640), canvas 640 x 640, "center", bilinear, fill 114, uint8.

Both ways give the same bits; kernel launches per batch are counted with torch's profiler where it works.

--patches, on the same N images: the packed ViT patch tokens of a native-resolution tower (patch 14, fit_patch_sizes(max_tokens=256),
bicubic, bfloat16, mean / std; both token formats, both layout classes of the items), two ways:

  composition  per item resize_many_to_float([img], its own size) and view / permute / reshape, then one cat: the code a user writes
               without the call;
  call         resize_many_to_patches: one call, three launches whatever N.

Both give the same bits.  No bar is set: the numbers are reported as they come.

--gap, on a workload of its own — N camera-sized images (H in [1080, 3000], W in [1440, 4000], about 1.1 GB), bicubic, reducing_gap 2.0 —
Pillow's two-step resize for the list, three ways, for RandomResizedCrop boxes to 224 x 224 and for the eval recipe (fit_sizes(shorter=256),
centred on 224 x 224):

  (a) the per-image loop of cubic_forward(img[None], size, box=, reducing_gap=2.0): the same bytes, the reference for time;
  (b) resize_many without a gap: other bytes (Pillow's one-step resize), today's long-window path;
  (c) reduce_many_for_resize + resize_many: four launches whatever N.

(c) must beat (a) with the min .. max ranges of the rounds apart; (b) against (c) is reported whichever way it falls.  Then the reduce
kernel's own rate: a uniform 64 x 1080 x 1920 x 3 batch at factor (4, 4) through the dense reduce() and through reduce_many, in input GB/s.

--alpha, on the default workload's sizes as RGBA images (C = 4, interleaved pixels and planes), RandomResizedCrop boxes to 224 x 224, bicubic:

  (a) the per-image loop of cubic_forward(img[None], size, box=, alpha=True): the same bytes, the reference for time;
  (b) resize_many(alpha=True): three launches whatever N;
  (c) resize_many without alpha on the same tensors: other bytes, what the fusion of the two conversions costs;
  (d) resize_many_to_float(alpha=True, bfloat16, nchw, mean / std).

(b) is expected to beat (a) with the ranges of the rounds apart; (b) against (c) is reported as it comes.

--nearest, on two workloads of its own — the label maps that travel with the images — Pillow's NEAREST for a list, against the loop a user
writes without the call (per image: index tensors from boxmath.nearest_indices, two index_selects, a flip, a pad, .long()) and against a
plain device copy of the output's bytes, the write floor:

  crops      64 camera-sized single-channel uint8 maps (H in [1080, 3000], W in [1440, 4000]), one RandomResizedCrop box each -> 224 x 224,
             half the items flipped, out_dtype=torch.int64;
  letterbox  16 maps of 1024 x 2048 -> fit_sizes(longer=1024), centred on a 1024 x 1024 canvas, fill 255, uint8.

Both ways give the same elements.  No bar is set; what is required is two kernel launches whatever N, and that the numbers are written down.

--ycbcr: resize_many_ycbcr on 64 camera-sized pictures held as 4:2:0 planes (1.5 B/px), one RandomResizedCrop box each -> 224 x 224
bicubic, normalised bfloat16 NCHW out, planar and interleaved chroma, against (a) resize_many_to_float on the same pictures as interleaved
RGB (3 B/px, no conversion) and (b) what a user does today: repeat_interleave of the chroma, a torch colour conversion to an interleaved
uint8 RGB image per item, then (a).  Times, launch counts and the kernel-level split of (a) and of the new call.

--maps: resize_many_maps (Pillow's "I;16" / "I" / "F" resize: double coefficients, double sums, the mode's store after each pass) on
64 camera-sized uint16 maps, H in [1080, 3000], W in [1440, 4000], one RandomResizedCrop box each -> 224 x 224, bilinear and bicubic,
half the items flipped.  No other GPU code produces these bits, so the contestants are the same call issued once per item (64 x 3
launches) and the one call (3 launches); resize_many_nearest on the same geometry (the maps viewed as int16) is the copy-only floor.
No bar is set; what is required is three launches whatever N, and that the numbers are written down.

--embed: what follows the patch tokens in such a tower — its learned position grid, 16 x 16 x 768 float32, resampled to the token grids
of 64 camera-sized images (patch 16, fit_patch_sizes(max_tokens=256)), bicubic, bfloat16 tokens, forward alone and forward + backward
(bfloat16 gradients, a float32 gradient of the grid) — two ways:

  loop  timm's NaFlexVit method with the existing calls: one cubic_forward per DISTINCT grid, to(bfloat16), cat in the items' order; for
        the backward the gradients of the items of a grid are summed, one cubic_backward per distinct grid, and the results added up;
  call  resize_embed_to_tokens / resize_embed_to_tokens_backward: two launches each, whatever N.

The forward gives the same bits; the loop's backward sums equal grids first, so its last bits differ.  The call must take less time than
the loop by more than the two spreads together; launches are counted with torch's profiler.  With --trace K: K calls of each for a kernel trace.

--logits: the way back — [16, K, 512, 512] logits on a letterbox canvas (fit_sizes(longer=512), "center") to the 16 camera-sized images'
own sizes and their argmax over K, bilinear, K = 19 and 150, float32 and bfloat16 logits — three ways:

  a  the per-item loop of existing calls: linear_forward(crop.float()[None], size), then argmax(1);
  b  resize_many_back(reduce=None), then argmax per item;
  c  resize_many_back(reduce="argmax"): two launches whatever N.

(c) gives (a)'s labels.  Per contestant: kernel launches (torch's profiler), ms per batch, and the growth of
torch.cuda.max_memory_allocated over one call.  No ratio is a bar; the loop (a) is the yardstick, and the numbers are written down.
(b)'s arena at K = 150 is 56 GB: --rounds 5 --batches 5 keeps the run short.

Timing: device events around `--batches` batches that end in a synchronise; every contestant is warmed up first; the median and the
min-to-max spread of `--rounds` rounds.  (c) must beat (a) by more than the two spreads together.  The loops do not assemble their N
results into one tensor; (c) writes the batch.

--tta: the way back for test-time augmentation — --logits' 16 camera-sized images, each answered M = 6 times: [16, K, c, c] logits on
letterbox canvases c = 384, 512 and 640, plain and mirrored; every pass resampled to the image's own size, un-mirrored, summed in pass
order in fp32 and reduced to the argmax over K; bilinear, K = 19 and 150, float32 and bfloat16 logits — three ways:

  a  the per-member loop of existing calls: linear_forward(crop.float()[None], size), flip(-1) where mirrored, added in place; argmax;
  b  resize_many_back(reduce=None, out_dtype=float32) of all 96 members, then torch's adds in order and argmax per image;
  c  resize_many_back_merged(reduce="argmax"): two launches whatever N and M.

The labels of (a) and (b) are compared with (c)'s and the differing ones counted (torch.argmax promises no order among equal sums).
Per contestant: kernel launches, ms per batch, the growth of torch.cuda.max_memory_allocated over one call; a contestant that does not
fit the device's memory — (b) at K = 150 needs 96 float32 [K, oh, ow] tensors, 334 GB — is reported as such and not timed.  No number
is a bar: the output is written down as measured, profiles/resize_many_back_merged.txt (--rounds 5 --batches 3 keeps the run short).

--tta --activation softmax|sigmoid: the same geometry with the activation per pass and the PROBABILITIES summed — (a) the loop a user
writes today, linear_forward, softmax(0) (or sigmoid), flip, add per member, argmax per image; (c) resize_many_back_merged(activation=,
reduce="argmax"); (d) the same call with activation=None, so that (c) against (d) is what the activation costs.  --logits --activation
softmax|sigmoid: probabilities at the images' sizes, reduce=None — (a) linear_forward and softmax per item, (c) resize_many_back(
activation=), (d) the call with activation=None.  Launches, ms per batch with the spread rule and peak memory as above; the share of
labels (the largest difference of the probabilities) by which (a) and (c) differ is reported, never asserted: torch's exp is not this
library's aa_exp.  Nothing is promised to be faster; where the loop wins the line says so.  profiles/resize_many_back_activation.txt.

--logits-backward: the gradient's way — gradients [K, oh_i, ow_i] at the images' own sizes back to the canvas, bilinear, odd items
flipped, float32 and bfloat16, resize_many_back_backward (two launches) against the loop a user writes today: linear_backward per item
(its table cache warm), the gradient flipped where needed, copied into a zeroed canvas.  Two workloads: "small", N = 64, K = 21, image
sides from 240 .. 640 (seed 7), a 128 x 128 letterbox canvas, where the loop is launch-bound and the call MUST be faster by more than
the two spreads together; and "large", --logits' 16 camera-sized images from a 512 x 512 canvas at K = 1, 19 and 150 (a fifth of
`--batches` a round; the K = 150 float32 gradients are 53 GB), whose figures are recorded without a requirement.  The two sides give
the same bits.  The kernel's fetched bytes come from a counter run of its own: tools/pmc_any.sh TAG back_bwd:small:21:f32 back_bwd_gather.

  python tools/resize_many_bench.py                      # the timing table
  python tools/resize_many_bench.py --float-only         # only the (d) / (e) table
  python tools/resize_many_bench.py --placed > out.txt   # only the placed call against the per-image loop (below);
                                                         # profiles/resize_many_placed.txt is this output, after the default table of
                                                         # the parent commit (twice) and of this one from the same session
  python tools/resize_many_bench.py --patches > out.txt  # only the patch tokens against the per-item composition;
                                                         # profiles/resize_many_patches.txt is this output
  python tools/resize_many_bench.py --gap > out.txt      # only the reducing_gap step for a list (above); profiles/resize_many_gap.txt
  python tools/resize_many_bench.py --alpha > out.txt    # only Pillow's RGBA resize for a list (above); profiles/resize_many_alpha.txt
  python tools/resize_many_bench.py --nearest > out.txt  # only Pillow's NEAREST for a list (above); profiles/resize_many_nearest.txt
  python tools/resize_many_bench.py --maps > out.txt     # only Pillow's I;16 resize for a list (below); profiles/resize_many_maps.txt
  python tools/resize_many_bench.py --ycbcr > out.txt    # only 4:2:0 planes to the batch (above); profiles/resize_many_ycbcr.txt
  python tools/resize_many_bench.py --embed > out.txt    # only the position grid to the token grids (above); profiles/resize_embed_many.txt
  python tools/resize_many_bench.py --logits > out.txt   # only the way back: canvas logits to the images' own sizes, argmax (below);
                                                         # profiles/resize_many_back.txt
  python tools/resize_many_bench.py --tta --rounds 5 --batches 3 > out.txt   # only the merged way back: 6 passes per image summed, argmax (above);
                                                         # profiles/resize_many_back_merged.txt is this output
  python tools/resize_many_bench.py --logits-backward > out.txt   # only the gradients' way back to the canvas (above);
                                                         # profiles/resize_many_back_bwd.txt
  python tools/resize_many_bench.py --trace 20           # only resize_many, 20 calls after 3 warm-up calls (run it under a profiler's
                                                         # kernel trace; every input reaches the GPU in ONE host-to-device copy)
  python tools/resize_many_bench.py --trace 20 --trace-float   # the same with resize_many_to_float calls
  python tools/resize_many_bench.py --trace 20 --trace-patches # the same with resize_many_to_patches calls (the --patches workload, cpp)
  python tools/resize_many_bench.py --summarise DIR      # kernels and copies per call, kernel time and bytes / time from that trace
"""
import argparse
import csv
import glob
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, OUT, SEED, WARM_CALLS = 64, (224, 224), 7, 3
MODES = {"bilinear": "linear", "bicubic": "cubic"}


def sizes(rng):
    return [(int(rng.integers(256, 1025)), int(rng.integers(256, 1025))) for _ in range(N)]


def random_resized_crop_box(rng, h, w):
    """torchvision's RandomResizedCrop.get_params (scale 0.08 .. 1, ratio 3/4 .. 4/3) -> Pillow's (x0, y0, x1, y1)."""
    area = h * w
    for _ in range(10):
        target = area * rng.uniform(0.08, 1.0)
        ratio = np.exp(rng.uniform(np.log(3 / 4), np.log(4 / 3)))
        cw, ch = int(round(np.sqrt(target * ratio))), int(round(np.sqrt(target / ratio)))
        if 0 < cw <= w and 0 < ch <= h:
            y0, x0 = int(rng.integers(0, h - ch + 1)), int(rng.integers(0, w - cw + 1))
            return (x0, y0, x0 + cw, y0 + ch)
    return (0, 0, w, h)


def algorithm_bytes(shapes, boxes, filter_name):
    """Bytes the three-launch algorithm moves for one batch: every item's hull in, its intermediate out and in again, the batch out."""
    from interpolate_antialiasing_amd import boxmath

    oh, ow = OUT
    hull = inter = 0
    for (h, w), bx in zip(shapes, boxes):
        b = boxmath.box_f32(bx)
        oy, ey = boxmath.axis_hull(h, oh, b[1], b[3], filter_name)
        ox, ex = boxmath.axis_hull(w, ow, b[0], b[2], filter_name)
        hull += (ey - oy) * (ex - ox) * 3
        inter += (ey - oy) * ow * 3
    return hull, inter, N * oh * ow * 3


def summarise(trace_dir, calls):
    """Kernels and copies per resize_many call, and kernel time per launch, from a profiler's kernel / memory-copy trace CSVs."""
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    ours = {}
    for r in rows:
        name = r.get("Kernel_Name", "")
        for k in ("many_tables", "many_hpass", "many_vpass"):
            if k in name:
                ours.setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    copies = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*memory_copy_trace.csv"), recursive=True):
        with open(path) as f:
            copies += list(csv.DictReader(f))
    h2d = sum(1 for r in copies if "HOST_TO_DEVICE" in (r.get("Direction", "") + r.get("Kind", "")).upper())
    print(f"trace: {len(rows)} kernel launches in all, {sum(len(v) for v in ours.values())} of them resize_many's, over {calls} calls")
    for k in ("many_tables", "many_hpass", "many_vpass"):
        v = ours.get(k, [])
        if v:
            steady = v[WARM_CALLS:] if len(v) > WARM_CALLS else v
            print(f"  {k}: {len(v) / calls:.2f} launches per call, median {statistics.median(steady):.1f} us, min {min(steady):.1f}, max {max(steady):.1f}")
    print(f"  kernels per call: {sum(len(v) for v in ours.values()) / calls:.2f} (expected 3, whatever N)")
    print(f"  host-to-device copies in the trace: {h2d} = 1 (all inputs, at set-up) + {(h2d - 1) / calls:.2f} per call (expected 1: the descriptor)")
    return {k: statistics.median(v[WARM_CALLS:] if len(v) > WARM_CALLS else v) for k, v in ours.items()}


def count_launches(torch, fn):
    """Kernel launches of one fn() from torch's profiler; None where torch has no profiler or it records no device activity.  An error
    of fn() itself, or of a profiler that is there, is an error."""
    try:
        from torch.profiler import ProfilerActivity, profile
    except ImportError:
        return None
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    kernels = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
               and "memset" not in e.name.lower()]
    return len(kernels) or None


def placed(args, torch, aa, images, shapes, timed):
    """The placed call against the per-image loop: eval (Resize + CenterCrop, to normalised bfloat16) and letterbox (uint8)."""
    from interpolate_antialiasing_amd import boxmath

    mean, std = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
    mean_t, std_t = (torch.tensor(v, device="cuda").view(1, 3, 1, 1) for v in (mean, std))
    fwd = {"bilinear": aa.linear_forward, "bicubic": aa.cubic_forward}

    def paste_loop(mode, vs, canvas, batch):
        oh, ow = canvas
        for i, (img, (vh, vw)) in enumerate(zip(images, vs)):
            r = fwd[mode](img[None], [vh, vw])[0]
            py, px = boxmath.center_offset(vh, oh), boxmath.center_offset(vw, ow)
            y0, y1, x0, x1 = max(0, py), min(oh, py + vh), max(0, px), min(ow, px + vw)
            batch[i, :, y0:y1, x0:x1] = r[:, y0 - py:y1 - py, x0 - px:x1 - px]
        return batch

    eval_sizes, eval_canvas = boxmath.fit_sizes(shapes, shorter=256), (224, 224)
    eval_batch = torch.empty((N, 3) + eval_canvas, dtype=torch.uint8, device="cuda", memory_format=torch.channels_last)
    lb_sizes, lb_canvas = boxmath.fit_sizes(shapes, longer=640), (640, 640)
    lb_batch = torch.empty((N, 3) + lb_canvas, dtype=torch.uint8, device="cuda", memory_format=torch.channels_last)

    def eval_loop():
        u = paste_loop("bicubic", eval_sizes, eval_canvas, eval_batch)
        return ((u.float() - mean_t) / std_t).to(torch.bfloat16).contiguous()

    def eval_call():
        return aa.resize_many_to_float(images, list(eval_canvas), "bicubic", sizes=eval_sizes, offsets="center", out_dtype=torch.bfloat16,
                                       out_format="nchw", mean=mean, std=std)

    def lb_loop():
        lb_batch.fill_(114)
        return paste_loop("bilinear", lb_sizes, lb_canvas, lb_batch)

    def lb_call():
        return aa.resize_many(images, list(lb_canvas), "bilinear", sizes=lb_sizes, offsets="center", fill=114)

    print(f"resize_many_bench --placed: N = {N} interleaved uint8 images, H and W in [256, 1024] (seed {SEED}); library: {os.path.basename(_lib_path())}")
    print(f"{args.rounds} rounds of {args.batches} batches per contestant, alternating; ms per batch: median [min .. max]")
    for title, loop_fn, call_fn, sz, canvas in (("eval: fit_sizes(shorter=256) -> 224 x 224 center, bicubic, bfloat16 nchw, mean / std", eval_loop, eval_call,
                                                 eval_sizes, eval_canvas),
                                                ("letterbox: fit_sizes(longer=640) -> 640 x 640 center, bilinear, fill 114, uint8", lb_loop, lb_call,
                                                 lb_sizes, lb_canvas)):
        contestants = {"loop: per-image forward + slice copy": loop_fn, "call: one placed call": call_fn}
        for fn in contestants.values():  # warm-up of every contestant (the loop's tables are cached from here on)
            fn()
            fn()
        torch.cuda.synchronize()
        a, b = loop_fn(), call_fn()
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a,
                                                  b.view(torch.int16) if b.dtype == torch.bfloat16 else b), "the placed call differs from the loop"
        times = {k: [] for k in contestants}
        for _ in range(args.rounds):
            for k, fn in contestants.items():
                times[k].append(timed(fn))
        resampled = sum(vh * vw for vh, vw in sz) / (N * canvas[0] * canvas[1])
        print(f"\n{title}")
        print(f"  pixels the loop resamples per pixel of the batch: {resampled:.2f}")
        stat = {}
        for k, v in times.items():
            stat[k] = (statistics.median(v), min(v), max(v))
            launches = count_launches(torch, contestants[k])
            print(f"  {k:40s} {stat[k][0]:8.3f} [{stat[k][1]:8.3f} .. {stat[k][2]:8.3f}]   kernel launches per batch: "
                  f"{launches if launches is not None else 'not measured'}")
        (ml, ll, hl), (mc, lc, hc) = stat.values()
        print(f"  call against loop: {ml / mc:.2f} x; median gain {ml - mc:.3f} ms, the two spreads together {(hl - ll) + (hc - lc):.3f} ms")


def patches(args, torch, aa, images, shapes, timed):
    """resize_many_to_patches against the per-item composition through resize_many_to_float."""
    from interpolate_antialiasing_amd import boxmath

    mean, std = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
    ph = pw = 14
    vs = boxmath.fit_patch_sizes(shapes, (ph, pw), max_tokens=256)
    offs = boxmath.token_offsets(vs, (ph, pw))
    dtype = torch.bfloat16
    perms = {"cpp": (1, 3, 0, 2, 4), "ppc": (1, 3, 2, 4, 0)}
    by_class = {"interleaved": images, "planar": [img.contiguous() for img in images]}

    def composition(imgs, fmt, n=N):
        toks = []
        for img, (vh, vw) in zip(imgs[:n], vs[:n]):
            r = aa.resize_many_to_float([img], [vh, vw], "bicubic", out_dtype=dtype, out_format="nchw", mean=mean, std=std)[0]
            toks.append(r.view(3, vh // ph, ph, vw // pw, pw).permute(*perms[fmt]).reshape((vh // ph) * (vw // pw), 3 * ph * pw))
        return torch.cat(toks)

    def call(imgs, fmt, n=N):
        return aa.resize_many_to_patches(imgs[:n], (ph, pw), "bicubic", sizes=vs[:n], patch_format=fmt, out_dtype=dtype, mean=mean, std=std)

    print(f"resize_many_bench --patches: N = {N} uint8 images, H and W in [256, 1024] (seed {SEED}); library: {os.path.basename(_lib_path())}")
    print(f"patch {ph} x {pw}, fit_patch_sizes(max_tokens=256): {offs[-1]} tokens of {3 * ph * pw} elements, {min(b - a for a, b in zip(offs, offs[1:]))} .. "
          f"{max(b - a for a, b in zip(offs, offs[1:]))} per item; bicubic, bfloat16, mean / std")
    print(f"{args.rounds} rounds of {args.batches} batches per contestant, alternating; ms per batch: median [min .. max]")
    for cls, imgs in by_class.items():
        for fmt in perms:
            contestants = {"composition: per-item call + view/permute/cat": lambda: composition(imgs, fmt), "call: resize_many_to_patches": lambda: call(imgs, fmt)}
            for fn in contestants.values():
                fn()
                fn()
            torch.cuda.synchronize()
            a, b = composition(imgs, fmt), call(imgs, fmt)
            assert a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16)), "resize_many_to_patches differs from the composition"
            times = {k: [] for k in contestants}
            for _ in range(args.rounds):
                for k, fn in contestants.items():
                    times[k].append(timed(fn))
            print(f"\n{cls} items, token format {fmt}")
            stat = {}
            for k, v in times.items():
                stat[k] = (statistics.median(v), min(v), max(v))
                launches = count_launches(torch, contestants[k])
                print(f"  {k:48s} {stat[k][0]:8.3f} [{stat[k][1]:8.3f} .. {stat[k][2]:8.3f}]   kernel launches per batch: "
                      f"{launches if launches is not None else 'not measured'}")
            (mc, lc, hc), (mo, lo, ho) = stat.values()
            verdict = "the one call is faster" if mo < mc else "THE ONE CALL IS NOT FASTER than the composition"
            print(f"  call against composition: {mc / mo:.2f} x; median gain {mc - mo:.3f} ms, the two spreads together {(hc - lc) + (ho - lo):.3f} ms: {verdict}")
    counts = {n: count_launches(torch, lambda: call(images, "cpp", n)) for n in (1, 8, N)}
    print("\nkernel launches of one resize_many_to_patches call by N (expected 3, whatever N): "
          + ", ".join(f"N = {n}: {v if v is not None else 'not measured'}" for n, v in counts.items()))


def gap(args, torch, aa, timed):
    """Pillow's reducing_gap for a list: the per-image loop, resize_many without a gap, and reduce_many_for_resize + resize_many."""
    from interpolate_antialiasing_amd import boxmath

    g = 2.0
    rng = np.random.default_rng(SEED)
    shapes = [(int(rng.integers(1080, 3001)), int(rng.integers(1440, 4001))) for _ in range(N)]
    flat = rng.integers(0, 256, sum(h * w * 3 for h, w in shapes), dtype=np.uint8)
    dev_flat = torch.from_numpy(flat).cuda()
    images, off = [], 0
    for h, w in shapes:
        images.append(dev_flat[off:off + h * w * 3].view(h, w, 3).permute(2, 0, 1))
        off += h * w * 3
    brng = np.random.default_rng(SEED + 1)
    boxes = [random_resized_crop_box(brng, h, w) for h, w in shapes]
    print(f"resize_many_bench --gap: N = {N} interleaved uint8 images, H in [1080, 3000], W in [1440, 4000], {len(flat) / 1e9:.3f} GB (seed {SEED}); "
          f"bicubic, reducing_gap {g}; library: {os.path.basename(_lib_path())}")
    print(f"{args.rounds} rounds of {args.batches} batches per contestant, alternating; ms per batch: median [min .. max]")

    eval_sizes, canvas = boxmath.fit_sizes(shapes, shorter=256), (224, 224)
    eval_batch = torch.empty((N, 3) + canvas, dtype=torch.uint8, device="cuda", memory_format=torch.channels_last)

    def crop_loop():
        return [aa.cubic_forward(img[None], list(OUT), box=bx, reducing_gap=g) for img, bx in zip(images, boxes)]

    def crop_call():
        small, b2 = aa.reduce_many_for_resize(images, list(OUT), "bicubic", boxes=boxes, reducing_gap=g)
        return aa.resize_many(small, list(OUT), "bicubic", boxes=b2)

    def eval_loop():
        oh, ow = canvas
        for i, (img, (vh, vw)) in enumerate(zip(images, eval_sizes)):
            r = aa.cubic_forward(img[None], [vh, vw], reducing_gap=g)[0]
            py, px = boxmath.center_offset(vh, oh), boxmath.center_offset(vw, ow)
            y0, y1, x0, x1 = max(0, py), min(oh, py + vh), max(0, px), min(ow, px + vw)
            eval_batch[i, :, y0:y1, x0:x1] = r[:, y0 - py:y1 - py, x0 - px:x1 - px]
        return eval_batch

    def eval_call():
        small, b2 = aa.reduce_many_for_resize(images, list(canvas), "bicubic", sizes=eval_sizes, reducing_gap=g)
        return aa.resize_many(small, list(canvas), "bicubic", boxes=b2, sizes=eval_sizes, offsets="center")

    tables = (
        ("one RandomResizedCrop box each -> 224 x 224", boxmath.reducing_plans(shapes, OUT, "bicubic", boxes, None, g),
         {"a: per-image loop, reducing_gap": crop_loop,
          "b: resize_many, no gap (other bytes)": lambda: aa.resize_many(images, list(OUT), "bicubic", boxes=boxes),
          "c: reduce_many_for_resize + resize_many": crop_call}, lambda: torch.cat(crop_loop())),
        ("eval: fit_sizes(shorter=256) -> 224 x 224 center", boxmath.reducing_plans(shapes, canvas, "bicubic", None, eval_sizes, g),
         {"a: per-image loop, reducing_gap + slice copy": eval_loop,
          "b: placed resize_many, no gap (other bytes)": lambda: aa.resize_many(images, list(canvas), "bicubic", sizes=eval_sizes, offsets="center"),
          "c: reduce_many_for_resize + placed resize_many": eval_call}, lambda: eval_loop().clone()),
    )
    for title, plans, contestants, want in tables:
        for fn in contestants.values():  # warm-up of every contestant (the loop's tables are cached from here on)
            fn()
            fn()
        torch.cuda.synchronize()
        names = list(contestants)
        assert torch.equal(contestants[names[2]](), want()), "reduce_many_for_resize + resize_many differs from the per-image loop"
        times = {k: [] for k in contestants}
        for _ in range(args.rounds):
            for k, fn in contestants.items():
                times[k].append(timed(fn))
        facs = sorted({p[0] for p in plans if p is not None})
        print(f"\n{title}")
        print(f"  items reduced: {sum(1 for p in plans if p is not None)} of {N}; factors {facs[0]} .. {facs[-1]}, {len(facs)} different")
        stat = {}
        for k, v in times.items():
            stat[k] = (statistics.median(v), min(v), max(v))
            launches = count_launches(torch, contestants[k])
            print(f"  {k:48s} {stat[k][0]:8.3f} [{stat[k][1]:8.3f} .. {stat[k][2]:8.3f}]   kernel launches per batch: "
                  f"{launches if launches is not None else 'not measured'}")
        (ma, la, ha), (mb, lb, hb), (mc, lc, hc) = stat.values()
        verdict = "PASS: the ranges do not overlap" if hc < la else "FAIL: (c) is not faster than (a) beyond the ranges of the rounds"
        print(f"  (c) against (a): {ma / mc:.2f} x; (c) at most {hc:.3f} ms, (a) at least {la:.3f} ms: {verdict}")
        print(f"  (c) against (b): {mb / mc:.2f} x (no bar: (b) computes other bytes; above 1 the gap path is the faster one)")

    reduce_rate(args, torch, aa, timed)


def alpha(args, torch, aa, shapes, timed):
    """Pillow's RGBA resize for a list: the per-image loop with alpha=True, the one call, the one call without alpha (the cost of the
    fusion) and the converting call, on the default workload's sizes as RGBA, in both layout classes."""
    rng = np.random.default_rng(SEED + 2)
    brng = np.random.default_rng(SEED + 1)
    boxes = [random_resized_crop_box(brng, h, w) for h, w in shapes]
    mean, std = [123.675, 116.28, 103.53, 127.5], [58.395, 57.12, 57.375, 64.0]
    flat = rng.integers(0, 256, sum(h * w * 4 for h, w in shapes), dtype=np.uint8)
    dev_flat = torch.from_numpy(flat).cuda()
    print(f"resize_many_bench --alpha: N = {N} RGBA uint8 images, H and W in [256, 1024] (seed {SEED}), one RandomResizedCrop box each -> {OUT}, "
          f"bicubic; library: {os.path.basename(_lib_path())}")
    print(f"{args.rounds} rounds of {args.batches} batches per contestant, alternating; ms per batch: median [min .. max]")
    for cls in ("interleaved", "planar"):
        images, off = [], 0
        for h, w in shapes:
            v = dev_flat[off:off + h * w * 4]
            images.append(v.view(h, w, 4).permute(2, 0, 1) if cls == "interleaved" else v.view(4, h, w))
            off += h * w * 4
        contestants = {
            "a: per-image loop, alpha=True": lambda: [aa.cubic_forward(img[None], list(OUT), box=bx, alpha=True) for img, bx in zip(images, boxes)],
            "b: resize_many(alpha=True)": lambda: aa.resize_many(images, list(OUT), "bicubic", boxes=boxes, alpha=True),
            "c: resize_many, no alpha (other bytes)": lambda: aa.resize_many(images, list(OUT), "bicubic", boxes=boxes),
            "d: resize_many_to_float(alpha=True, bf16, nchw)": lambda: aa.resize_many_to_float(
                images, list(OUT), "bicubic", boxes=boxes, out_dtype=torch.bfloat16, out_format="nchw", mean=mean, std=std, alpha=True),
        }
        for fn in contestants.values():  # warm-up of every contestant (the loop's tables are cached from here on)
            fn()
            fn()
        torch.cuda.synchronize()
        names = list(contestants)
        assert torch.equal(contestants[names[1]](), torch.cat(contestants[names[0]]())), "resize_many(alpha=True) differs from the per-image loop"
        times = {k: [] for k in contestants}
        for _ in range(args.rounds):
            for k, fn in contestants.items():
                times[k].append(timed(fn))
        print(f"\n{cls}")
        stat = {}
        for k, v in times.items():
            stat[k] = (statistics.median(v), min(v), max(v))
            launches = count_launches(torch, contestants[k])
            print(f"  {k:48s} {stat[k][0]:8.3f} [{stat[k][1]:8.3f} .. {stat[k][2]:8.3f}]   kernel launches per batch: "
                  f"{launches if launches is not None else 'not measured'}")
        (ma, la, ha), (mb, lb, hb), (mc, lc, hc), _ = stat.values()
        verdict = "PASS: the ranges do not overlap" if hb < la else "FAIL: (b) is not faster than (a) beyond the ranges of the rounds"
        print(f"  (b) against (a): {ma / mb:.2f} x; (b) at most {hb:.3f} ms, (a) at least {la:.3f} ms: {verdict}")
        print(f"  (b) against (c): {mb / mc:.3f} x the time (no bar: the cost of premultiplying in the horizontal pass and converting back in the vertical)")
        counts = {n: count_launches(torch, lambda: aa.resize_many(images[:n], list(OUT), "bicubic", boxes=boxes[:n], alpha=True)) for n in (1, 8, N)}
        print("  kernel launches of one resize_many(alpha=True) call by N (expected 3, whatever N): "
              + ", ".join(f"N = {n}: {v if v is not None else 'not measured'}" for n, v in counts.items()))


def nearest(args, torch, aa, timed):
    """resize_many_nearest against the per-image torch loop and the write floor, on the two label-map workloads."""
    from interpolate_antialiasing_amd import boxmath

    rng = np.random.default_rng(SEED)
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    crop_shapes = [(int(rng.integers(1080, 3001)), int(rng.integers(1440, 4001))) for _ in range(N)]
    crop_maps = [torch.randint(0, 21, (1, h, w), dtype=torch.uint8, device="cuda", generator=gen) for h, w in crop_shapes]
    brng = np.random.default_rng(SEED + 1)
    crop_boxes = [random_resized_crop_box(brng, h, w) for h, w in crop_shapes]
    crop_flips = [i % 2 == 1 for i in range(N)]
    lb_shapes = [(1024, 2048)] * 16
    lb_maps = [torch.randint(0, 21, (1, h, w), dtype=torch.uint8, device="cuda", generator=gen) for h, w in lb_shapes]
    lb_sizes, lb_canvas = boxmath.fit_sizes(lb_shapes, longer=1024), (1024, 1024)

    def tables_of(shapes, boxes, vs):
        """The loop's index tensors, built on the host and uploaded: per image (rows, columns)."""
        out = []
        for (h, w), bx, (vh, vw) in zip(shapes, boxes, vs):
            b = boxmath.box_f32(bx) if bx is not None else (None, None, None, None)
            out.append((torch.tensor(boxmath.nearest_indices(h, vh, b[1], b[3]), device="cuda"),
                        torch.tensor(boxmath.nearest_indices(w, vw, b[0], b[2]), device="cuda")))
        return out

    def loop(maps, tabs, vs, canvas, flips, fill, long):
        oh, ow = canvas
        res = []
        for i, (m, (iy, ix), (vh, vw)) in enumerate(zip(maps, tabs, vs)):
            r = m.index_select(1, iy).index_select(2, ix)
            py, px = boxmath.center_offset(vh, oh), boxmath.center_offset(vw, ow)
            if (vh, vw) != (oh, ow):
                r = torch.nn.functional.pad(r, (px, ow - px - vw, py, oh - py - vh), value=fill)
            if flips is not None and flips[i]:
                r = r.flip(-1)
            res.append(r.long() if long else r)
        return torch.stack(res)

    crop_vs = [OUT] * N
    crop_tabs = tables_of(crop_shapes, crop_boxes, crop_vs)
    lb_tabs = tables_of(lb_shapes, [None] * 16, lb_sizes)
    workloads = (
        (f"crops: {N} single-channel uint8 maps, H in [1080, 3000], W in [1440, 4000], one RandomResizedCrop box each -> {OUT}, {sum(crop_flips)} flipped, int64 out",
         {"loop: tables built on the host per batch": lambda: loop(crop_maps, tables_of(crop_shapes, crop_boxes, crop_vs), crop_vs, OUT, crop_flips, 0, True),
          "loop: tables already on the device": lambda: loop(crop_maps, crop_tabs, crop_vs, OUT, crop_flips, 0, True),
          "call: resize_many_nearest": lambda: aa.resize_many_nearest(crop_maps, list(OUT), boxes=crop_boxes, flips=crop_flips, out_dtype=torch.int64)},
         lambda n: aa.resize_many_nearest(crop_maps[:n], list(OUT), boxes=crop_boxes[:n], flips=crop_flips[:n], out_dtype=torch.int64), N),
        (f"letterbox: 16 uint8 maps of 1024 x 2048 -> {lb_sizes[0]}, centred on {lb_canvas}, fill 255, uint8 out",
         {"loop: tables built on the host per batch": lambda: loop(lb_maps, tables_of(lb_shapes, [None] * 16, lb_sizes), lb_sizes, lb_canvas, None, 255, False),
          "loop: tables already on the device": lambda: loop(lb_maps, lb_tabs, lb_sizes, lb_canvas, None, 255, False),
          "call: resize_many_nearest": lambda: aa.resize_many_nearest(lb_maps, list(lb_canvas), sizes=lb_sizes, offsets="center", fill=255)},
         lambda n: aa.resize_many_nearest(lb_maps[:n], list(lb_canvas), sizes=lb_sizes[:n], offsets="center", fill=255), 16),
    )
    print(f"resize_many_bench --nearest: Pillow's NEAREST for label maps (seed {SEED}); library: {os.path.basename(_lib_path())}")
    print(f"{args.rounds} rounds of {args.batches} batches per contestant, alternating; ms per batch: median [min .. max]")
    for title, contestants, call_n, n_all in workloads:
        names = list(contestants)
        for fn in contestants.values():
            fn()
            fn()
        torch.cuda.synchronize()
        want, got = contestants[names[1]](), contestants[names[2]]()
        assert want.dtype == got.dtype and torch.equal(want, got), "resize_many_nearest differs from the per-image loop"
        src = torch.empty_like(got)
        dst = torch.empty_like(got)
        contestants = dict(contestants)
        contestants["floor: device copy of the output's bytes"] = lambda: dst.copy_(src)
        times = {k: [] for k in contestants}
        for _ in range(args.rounds):
            for k, fn in contestants.items():
                times[k].append(timed(fn))
        print(f"\n{title}")
        print(f"  output: {got.numel() * got.element_size() / 1e6:.2f} MB")
        stat = {}
        for k, v in times.items():
            stat[k] = (statistics.median(v), min(v), max(v))
            launches = count_launches(torch, contestants[k])
            print(f"  {k:48s} {stat[k][0]:8.3f} [{stat[k][1]:8.3f} .. {stat[k][2]:8.3f}]   kernel launches per batch: "
                  f"{launches if launches is not None else 'not measured'}")
        (mh, _, _), (md, ld, hd), (mc, lc, hc), (mf, _, _) = stat.values()
        verdict = "the one call is faster" if hc < ld else ("THE ONE CALL IS NOT FASTER than the loop" if mc >= md else "faster by the medians, the ranges overlap")
        print(f"  call against the loop with tables on the device: {md / mc:.2f} x; against the loop that builds them: {mh / mc:.2f} x: {verdict}")
        for part in ("near_tables", "near_gather"):
            kt = kernel_times(torch, contestants[names[2]], part)
            if kt:
                print(f"  {part}: device time median {statistics.median(kt):8.1f} us [{min(kt):8.1f} .. {max(kt):8.1f}] over {len(kt)} launches")
            else:
                print(f"  {part}: device time not measured")
        print(f"  the floor copy: {mf * 1e3:.1f} us per batch by device events")
        counts = {n: count_launches(torch, lambda: call_n(n)) for n in (1, 8, n_all)}
        print("  kernel launches of one resize_many_nearest call by N (expected 2, whatever N): "
              + ", ".join(f"N = {n}: {v if v is not None else 'not measured'}" for n, v in counts.items()))


def maps(args, torch, aa, timed):
    """resize_many_maps against the same call issued once per item, and resize_many_nearest on the same geometry as the copy-only floor."""
    rng = np.random.default_rng(SEED)
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    shapes = [(int(rng.integers(1080, 3001)), int(rng.integers(1440, 4001))) for _ in range(N)]
    # (int16 noise viewed as uint16: the whole range, and the int16 views go to resize_many_nearest as they are)
    signed = [torch.randint(-32768, 32768, (1, h, w), dtype=torch.int16, device="cuda", generator=gen) for h, w in shapes]
    items = [t.view(torch.uint16) for t in signed]
    brng = np.random.default_rng(SEED + 1)
    boxes = [random_resized_crop_box(brng, h, w) for h, w in shapes]
    flips = [i % 2 == 1 for i in range(N)]
    print(f"resize_many_bench --maps: Pillow's I;16 resize for a list (seed {SEED}); library: {os.path.basename(_lib_path())}")
    print(f"{N} single-channel uint16 maps, H in [1080, 3000], W in [1440, 4000], one RandomResizedCrop box each -> {OUT}, {sum(flips)} flipped")
    print(f"{args.rounds} rounds of {args.batches} batches per contestant, alternating; ms per batch: median [min .. max]")
    for mode in MODES:
        def one_call(n=N):
            return aa.resize_many_maps(items[:n], list(OUT), mode, boxes=boxes[:n], flips=flips[:n])

        def per_item():
            return [aa.resize_many_maps(items[i:i + 1], list(OUT), mode, boxes=boxes[i:i + 1], flips=flips[i:i + 1]) for i in range(N)]

        def floor():
            return aa.resize_many_nearest(signed, list(OUT), boxes=boxes, flips=flips)

        contestants = {"loop: resize_many_maps once per item": per_item, "call: resize_many_maps": one_call,
                       "floor: resize_many_nearest, same geometry (copies only)": floor}
        for fn in contestants.values():
            fn()
            fn()
        torch.cuda.synchronize()
        assert torch.equal(torch.cat(per_item()).view(torch.int16), one_call().view(torch.int16)), "the one call differs from the call per item"
        times = {k: [] for k in contestants}
        for _ in range(args.rounds):
            for k, fn in contestants.items():
                times[k].append(timed(fn))
        print(f"\n{mode}")
        stat = {}
        for k, v in times.items():
            stat[k] = (statistics.median(v), min(v), max(v))
            launches = count_launches(torch, contestants[k])
            print(f"  {k:56s} {stat[k][0]:8.3f} [{stat[k][1]:8.3f} .. {stat[k][2]:8.3f}]   kernel launches per batch: "
                  f"{launches if launches is not None else 'not measured'}")
        (ml, ll, hl), (mc, lc, hc), (mf, _, _) = stat.values()
        verdict = "the one call is faster" if hc < ll else ("THE ONE CALL IS NOT FASTER than the call per item" if mc >= ml else "faster by the medians, the ranges overlap")
        print(f"  one call against the call per item: {ml / mc:.2f} x: {verdict}; against the copy-only floor: {mc / mf:.2f} x its time")
        for part in ("maps_tables", "maps_hpass", "maps_vpass"):
            kt = kernel_times(torch, one_call, part)
            if kt:
                print(f"  {part}: device time median {statistics.median(kt):8.1f} us [{min(kt):8.1f} .. {max(kt):8.1f}] over {len(kt)} launches")
            else:
                print(f"  {part}: device time not measured")
        counts = {n: count_launches(torch, lambda: one_call(n)) for n in (1, 8, N)}
        print("  kernel launches of one resize_many_maps call by N (expected 3, whatever N): "
              + ", ".join(f"N = {n}: {v if v is not None else 'not measured'}" for n, v in counts.items()))


def ycbcr(args, torch, aa, timed):
    """resize_many_ycbcr (4:2:0 planes in, planar and interleaved chroma) against two things that exist without it: (a) resize_many_to_float
    on the same pictures as interleaved RGB, which reads twice the bytes and converts nothing, and (b) what a user does today: expand the
    chroma, convert to an interleaved uint8 RGB image per item in torch, then (a)."""
    rng = np.random.default_rng(SEED)
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    shapes = [(int(rng.integers(1080, 3001)), int(rng.integers(1440, 4001))) for _ in range(N)]
    brng = np.random.default_rng(SEED + 1)
    boxes = [random_resized_crop_box(brng, h, w) for h, w in shapes]
    mean, std = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
    kw = dict(boxes=boxes, out_dtype=torch.bfloat16, out_format="nchw", mean=mean, std=std)
    rnd = lambda *s: torch.randint(0, 256, s, dtype=torch.uint8, device="cuda", generator=gen)  # noqa: E731
    planar = [(rnd(h, w), rnd(-(-h // 2), -(-w // 2)), rnd(-(-h // 2), -(-w // 2))) for h, w in shapes]
    inter = [(y, torch.stack([cb, cr], dim=-1).contiguous()) for y, cb, cr in planar]

    def to_rgb(y, cb, cr):
        """What a user writes today: nearest chroma expansion, the JFIF matrix in float, an interleaved uint8 image."""
        h, w = y.shape
        cbf = cb.repeat_interleave(2, 0).repeat_interleave(2, 1)[:h, :w].float() - 128.0
        crf = cr.repeat_interleave(2, 0).repeat_interleave(2, 1)[:h, :w].float() - 128.0
        yf = y.float()
        rgb = torch.stack([yf + 1.402 * crf, yf - 0.34414 * cbf - 0.71414 * crf, yf + 1.772 * cbf], dim=-1)
        return rgb.round().clamp(0, 255).to(torch.uint8).permute(2, 0, 1)

    rgb = [to_rgb(*p) for p in planar]
    contestants = {
        "a: resize_many_to_float on interleaved RGB (3 B/px in)": lambda: aa.resize_many_to_float(rgb, list(OUT), "bicubic", **kw),
        "b: expand + convert in torch per item, then (a)": lambda: aa.resize_many_to_float([to_rgb(*p) for p in planar], list(OUT), "bicubic", **kw),
        "c: resize_many_ycbcr, planes (Y, Cb, Cr)": lambda: aa.resize_many_ycbcr(planar, list(OUT), "bicubic", subsampling="420", **kw),
        "d: resize_many_ycbcr, interleaved (Y, CbCr)": lambda: aa.resize_many_ycbcr(inter, list(OUT), "bicubic", subsampling="420", **kw),
    }
    print(f"resize_many_bench --ycbcr: 4:2:0 planes to a normalised bfloat16 NCHW batch (seed {SEED}); library: {os.path.basename(_lib_path())}")
    print(f"{N} pictures, H in [1080, 3000], W in [1440, 4000], one RandomResizedCrop box each -> {OUT}, bicubic, mean / std")
    print(f"input bytes: planes {sum(y.numel() + cb.numel() + cr.numel() for y, cb, cr in planar) / 1e6:.1f} MB, "
          f"interleaved RGB {sum(t.numel() for t in rgb) / 1e6:.1f} MB")
    print(f"{args.rounds} rounds of {args.batches} batches per contestant, alternating; ms per batch: median [min .. max]")
    for fn in contestants.values():
        fn()
        fn()
    torch.cuda.synchronize()
    c, d = list(contestants.values())[2:]
    if args.trace:  # (under a profiler's kernel trace: the kernel-level split of (a), (c) and (d), the same number of calls each)
        for fn in (list(contestants.values())[0], c, d):
            for _ in range(args.trace):
                fn()
        torch.cuda.synchronize()
        return
    assert torch.equal(c().view(torch.int16), d().view(torch.int16)), "planar and interleaved chroma differ"
    u_new = aa.resize_many_ycbcr(planar, list(OUT), "bicubic", subsampling="420", boxes=boxes).int()
    u_old = aa.resize_many(rgb, list(OUT), "bicubic", boxes=boxes).int()
    print(f"bytes of (c) against bytes of (a) (not promised equal: the roundings fall elsewhere, and (a)'s chroma was expanded by "
          f"repetition): mean |difference| {(u_new - u_old).abs().float().mean().item():.3f}, largest {(u_new - u_old).abs().max().item()}")
    times = {k: [] for k in contestants}
    for _ in range(args.rounds):
        for k, fn in contestants.items():
            times[k].append(timed(fn))
    stat = {}
    for k, v in times.items():
        stat[k] = (statistics.median(v), min(v), max(v))
        launches = count_launches(torch, contestants[k])
        print(f"  {k:56s} {stat[k][0]:8.3f} [{stat[k][1]:8.3f} .. {stat[k][2]:8.3f}]   kernel launches per batch: "
              f"{launches if launches is not None else 'not measured'}")
    (ma, la, ha), (mb, _, _), (mc, lc, hc), (md, ld, hd) = stat.values()
    for label, (m, lo, hi) in (("planes", (mc, lc, hc)), ("interleaved", (md, ld, hd))):
        verdict = "faster than (a)" if hi < la else ("SLOWER THAN (a)" if lo > ha else ("slower than (a) by the medians, the ranges overlap" if m >= ma
                                                                                          else "faster than (a) by the medians, the ranges overlap"))
        print(f"  resize_many_ycbcr, {label}: {ma / m:.2f} x (a), {mb / m:.2f} x (b): {verdict}")
    for name, fn, parts in (("a", list(contestants.values())[0], ("many_tables", "many_hpass", "many_vpass")),
                            ("c", c, ("many_tables", "many_hpass", "ycc_vpass")), ("d", d, ("many_tables", "many_hpass", "ycc_vpass"))):
        for part in parts:
            kt = kernel_times(torch, fn, part, calls=12)
            if kt:  # (interleaved chroma: two launches of the first two kernels per call, so the time is summed per call)
                print(f"  ({name}) {part}: {len(kt) / 12:.0f} launch(es) per call, device time {sum(kt) / 12:8.1f} us per call "
                      f"[single launches {min(kt):8.1f} .. {max(kt):8.1f}] over 12 calls")
            else:
                print(f"  ({name}) {part}: device time not measured")
    for label, images in (("planes", planar), ("interleaved", inter)):
        counts = {n: count_launches(torch, lambda: aa.resize_many_ycbcr(images[:n], list(OUT), "bicubic", subsampling="420",
                                                                         **{**kw, "boxes": boxes[:n]})) for n in (1, 8, N)}
        print(f"  kernel launches of one resize_many_ycbcr call, {label}, by N (expected {3 if label == 'planes' else 5}, whatever N): "
              + ", ".join(f"N = {n}: {v if v is not None else 'not measured'}" for n, v in counts.items()))


def kernel_times(torch, fn, part, calls=12):
    """Device durations in us of the kernels whose name holds `part`, over `calls` runs of fn(), from torch's profiler; [] where it
    records no device activity."""
    try:
        from torch.profiler import ProfilerActivity, profile
    except ImportError:
        return []
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    return [e.time_range.elapsed_us() for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and part in e.name]


def reduce_rate(args, torch, aa, timed):
    """The reduce kernel's own rate: the dense kernel is the yardstick.  A call of reduce_many also plans N records on the host, so the
    kernels' own device times are reported beside the calls' times."""
    x = torch.randint(0, 256, (N, 1080, 1920, 3), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(SEED))
    x = x.permute(0, 3, 1, 2)
    contestants = {"dense reduce(), factor (4, 4)": lambda: aa.reduce(x, (4, 4)), "reduce_many, factor (4, 4)": lambda: aa.reduce_many(x, (4, 4)),
                   "dense reduce(), factor (5, 5)": lambda: aa.reduce(x, (5, 5)), "reduce_many, factor (5, 5)": lambda: aa.reduce_many(x, (5, 5))}
    for fn in contestants.values():
        fn()
        fn()
    torch.cuda.synchronize()
    for f in ((4, 4), (5, 5)):
        assert torch.equal(torch.stack(aa.reduce_many(x, f)), aa.reduce(x, f)), "reduce_many differs from reduce"
    times = {k: [] for k in contestants}
    for _ in range(args.rounds):
        for k, fn in contestants.items():
            times[k].append(timed(fn))
    print(f"\nthe reduce kernel's own rate: uniform {N} x 1080 x 1920 x 3 interleaved, {x.numel() / 1e6:.1f} MB in (library: {os.path.basename(_lib_path())})")
    print("  (5, 5) runs the run-time-fx form in both kernels; ms per call, then the kernel's own device time and its input GB/s: median [min .. max]")
    stat = {}
    for k, v in times.items():
        kt = kernel_times(torch, contestants[k], "reduce")
        stat[k] = (statistics.median(kt), min(kt), max(kt)) if kt else None
        line = f"  {k:32s} call {statistics.median(v):8.4f} [{min(v):8.4f} .. {max(v):8.4f}] ms"
        if kt:
            m, lo, hi = stat[k]
            line += f"   kernel {m:8.1f} [{lo:8.1f} .. {hi:8.1f}] us   {x.numel() / m / 1e3:8.1f} [{x.numel() / hi / 1e3:8.1f} .. {x.numel() / lo / 1e3:8.1f}] GB/s"
        else:
            line += "   kernel time not measured"
        print(line)
    names = list(contestants)
    for d, m in ((names[0], names[1]), (names[2], names[3])):
        if stat[d] and stat[m]:
            apart = stat[m][1] > stat[d][2] or stat[m][2] < stat[d][1]
            print(f"  {m} against {d}: {stat[m][0] / stat[d][0]:.3f} x the kernel time; the ranges {'do not overlap' if apart else 'overlap'}")


def embed(args, torch, aa, timed):
    """resize_embed_to_tokens and its backward against timm's method with the existing calls: one forward (one backward) per distinct grid."""
    from interpolate_antialiasing_amd import boxmath

    rng = np.random.default_rng(SEED)
    shapes = [(int(rng.integers(1080, 3001)), int(rng.integers(1440, 4001))) for _ in range(N)]
    patch, h0, w0, d = (16, 16), 16, 16, 768
    grids = boxmath.patch_grids(boxmath.fit_patch_sizes(shapes, patch, max_tokens=256), patch)
    offs = boxmath.token_offsets(grids, (1, 1))
    distinct = sorted(set(grids))
    members = {g: [i for i, q in enumerate(grids) if q == g] for g in distinct}
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    pos = torch.randn((h0, w0, d), device="cuda", generator=gen)  # the fp32 parameter
    grad = torch.randn((offs[-1], d), device="cuda", generator=gen).to(torch.bfloat16)  # what the AMP model hands back
    if args.trace:  # (under a profiler's kernel trace: the one call, both ways)
        for _ in range(WARM_CALLS + args.trace):
            aa.resize_embed_to_tokens(pos, grids, "bicubic", out_dtype=torch.bfloat16)
            aa.resize_embed_to_tokens_backward(grad, (h0, w0, d), grids, "bicubic")
        torch.cuda.synchronize()
        return
    img = pos.permute(2, 0, 1)[None]  # [1, D, H0, W0] over the same memory (channels_last)

    def loop_forward():
        per = {g: aa.cubic_forward(img, list(g))[0].permute(1, 2, 0).reshape(g[0] * g[1], d).to(torch.bfloat16) for g in distinct}
        return torch.cat([per[g] for g in grids])

    def loop_backward(g_tokens):
        acc = None
        for (gh, gw), idx in members.items():
            gsum = torch.stack([g_tokens[offs[i]:offs[i + 1]] for i in idx]).float().sum(0)
            b = aa.cubic_backward(gsum.view(gh, gw, d).permute(2, 0, 1)[None], [gh, gw], [1, d, h0, w0])
            acc = b if acc is None else acc + b
        return acc[0].permute(1, 2, 0).contiguous()

    def call_forward():
        return aa.resize_embed_to_tokens(pos, grids, "bicubic", out_dtype=torch.bfloat16)

    def call_backward(g_tokens):
        return aa.resize_embed_to_tokens_backward(g_tokens, (h0, w0, d), grids, "bicubic")

    print(f"resize_many_bench --embed: a {h0} x {w0} x {d} float32 position grid to the token grids of N = {N} camera-sized images, H in [1080, 3000], "
          f"W in [1440, 4000] (seed {SEED}); library: {os.path.basename(_lib_path())}")
    print(f"patch {patch[0]} x {patch[1]}, fit_patch_sizes(max_tokens=256): {offs[-1]} tokens, {len(distinct)} distinct grids, "
          f"{min(b - a for a, b in zip(offs, offs[1:]))} .. {max(b - a for a, b in zip(offs, offs[1:]))} tokens per item; bicubic, bfloat16 tokens and gradients")
    print(f"{args.rounds} rounds of {args.batches} batches per contestant, alternating; ms per batch: median [min .. max]")
    a, b = loop_forward(), call_forward()
    assert a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16)), "resize_embed_to_tokens differs from the loop"
    ga, gb = loop_backward(grad), call_backward(grad)
    # (the loop adds the gradients of equal grids first: another order of the same sum, so the last bits differ)
    err = float((ga - gb).abs().max() / ga.abs().max())
    assert err < 1e-5, f"the backward differs from the loop: {err}"
    print(f"forward: the same bits; backward: max |difference| / max |gradient| = {err:.2e} (the loop sums equal grids first)")
    for title, loop_fn, call_fn in (("forward", loop_forward, call_forward),
                                    ("forward + backward", lambda: (loop_forward(), loop_backward(grad)), lambda: (call_forward(), call_backward(grad)))):
        contestants = {"loop: one call per distinct grid, to(bf16), cat": loop_fn, "call: resize_embed_to_tokens": call_fn}
        for fn in contestants.values():
            fn()
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in contestants}
        for _ in range(args.rounds):
            for k, fn in contestants.items():
                times[k].append(timed(fn))
        print(f"\n{title}")
        stat = {}
        for k, v in times.items():
            stat[k] = (statistics.median(v), min(v), max(v))
            launches = count_launches(torch, contestants[k])
            print(f"  {k:50s} {stat[k][0]:8.3f} [{stat[k][1]:8.3f} .. {stat[k][2]:8.3f}]   kernel launches per batch: "
                  f"{launches if launches is not None else 'not measured'}")
        (ml, ll, hl), (mc, lc, hc) = stat.values()
        verdict = "the one call is faster" if ml - mc > (hl - ll) + (hc - lc) else "THE ONE CALL IS NOT FASTER by more than the spreads"
        print(f"  call against loop: {ml / mc:.2f} x; median gain {ml - mc:.3f} ms, the two spreads together {(hl - ll) + (hc - lc):.3f} ms: {verdict}")


def logits(args, torch, aa, timed):
    """resize_many_back against the per-item loop of existing calls: logits on a 512 x 512 letterbox canvas back to 16 camera-sized images,
    argmax over K.  Per contestant: kernel launches, ms per batch, and the growth of torch.cuda.max_memory_allocated over one call."""
    from interpolate_antialiasing_amd import boxmath

    n, canvas = 16, (512, 512)
    rng = np.random.default_rng(SEED)
    shapes = [(int(rng.integers(1080, 3001)), int(rng.integers(1440, 4001))) for _ in range(N)][:n]
    placed_sizes = boxmath.fit_sizes(shapes, longer=canvas[0])
    regions = boxmath.placed_regions(placed_sizes, "center", canvas)
    pixels = sum(h * w for h, w in shapes)
    print(f"resize_many_bench --logits: [N, K, {canvas[0]}, {canvas[1]}] logits on a letterbox canvas (fit_sizes(longer={canvas[0]}), 'center') back to "
          f"N = {n} camera-sized images, H in [1080, 3000], W in [1440, 4000] (seed {SEED}), {pixels / 1e6:.1f} M output pixels; bilinear; "
          f"library: {os.path.basename(_lib_path())}")
    print(f"{args.rounds} rounds of {args.batches} batches per contestant, alternating; ms per batch: median [min .. max]; peak: the growth of "
          "torch.cuda.max_memory_allocated over one call")
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    for k in (19, 150):
        for dtype in (torch.float32, torch.bfloat16):
            x = torch.randn((n, k) + canvas, device="cuda", generator=gen).to(dtype)

            def loop():
                out = []
                for i, (y0, x0, h, w) in enumerate(regions):
                    out.append(aa.linear_forward(x[i, :, y0:y0 + h, x0:x0 + w].float()[None], list(shapes[i])).argmax(1)[0])
                return out

            def values_then_argmax():
                return [v.argmax(0) for v in aa.resize_many_back(x, shapes, regions=regions)]

            def fused():
                return aa.resize_many_back(x, shapes, regions=regions, reduce="argmax")

            contestants = {"a: loop: linear_forward(crop.float()), argmax(1) per item": loop,
                           "b: resize_many_back(reduce=None), argmax per item": values_then_argmax,
                           "c: resize_many_back(reduce='argmax')": fused}
            results = {}
            for key, fn in contestants.items():
                results[key] = fn()
                fn()
            torch.cuda.synchronize()
            # (the 16-bit values of (b) are rounded before its argmax: only the float32 logits must agree everywhere)
            same_a = all(torch.equal(p, q) for p, q in zip(results["a: loop: linear_forward(crop.float()), argmax(1) per item"], results["c: resize_many_back(reduce='argmax')"]))
            assert same_a, "reduce='argmax' differs from the loop"
            del results
            times = {key: [] for key in contestants}
            for _ in range(args.rounds):
                for key, fn in contestants.items():
                    times[key].append(timed(fn))
            print(f"\nK = {k}, {str(dtype).replace('torch.', '')}: (c) gives the loop's labels")
            stat = {}
            for key, v in times.items():
                stat[key] = (statistics.median(v), min(v), max(v))
                launches = count_launches(torch, contestants[key])
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.max_memory_allocated()
                r = contestants[key]()
                torch.cuda.synchronize()
                peak = torch.cuda.max_memory_allocated() - before
                del r
                print(f"  {key:62s} {stat[key][0]:9.3f} [{stat[key][1]:9.3f} .. {stat[key][2]:9.3f}]   launches {launches if launches is not None else 'not measured'}"
                      f"   peak {peak / 1e6:10.1f} MB")
            (ma, la, ha), (mb, lb, hb), (mc, lc, hc) = stat.values()
            verdict = "(c) is faster" if ma - mc > (ha - la) + (hc - lc) else "(c) IS NOT FASTER than the loop by more than the spreads"
            print(f"  (c) against (a): {ma / mc:.2f} x; (c) against (b): {mb / mc:.2f} x; median gain over (a) {ma - mc:.3f} ms, the two spreads together "
                  f"{(ha - la) + (hc - lc):.3f} ms: {verdict}")
            del x


def tta(args, torch, aa, timed):
    """resize_many_back_merged on test-time augmentation: --logits' 16 camera-sized images, each answered M = 6 times (letterbox canvases
    of 384, 512 and 640, plain and mirrored), the passes resampled to the image's size, un-mirrored, summed in order and reduced to the
    argmax.  Three ways; per contestant: kernel launches, ms per batch, and the growth of torch.cuda.max_memory_allocated over one call.
    A contestant that does not fit the device's memory is reported as such and not timed."""
    from interpolate_antialiasing_amd import boxmath

    n, canvases = 16, (384, 512, 640)
    rng = np.random.default_rng(SEED)
    shapes = [(int(rng.integers(1080, 3001)), int(rng.integers(1440, 4001))) for _ in range(N)][:n]
    passes = [(c, flip) for c in canvases for flip in (False, True)]
    regions, flips, groups = [], [], []
    for c, flip in passes:  # (a batch is laid out pass by pass: the groups interleave)
        regions += boxmath.placed_regions(boxmath.fit_sizes(shapes, longer=c), "center", (c, c))
        flips += [flip] * n
        groups += list(range(n))
    pixels = sum(h * w for h, w in shapes)
    print(f"resize_many_bench --tta: N = {n} camera-sized images, H in [1080, 3000], W in [1440, 4000] (seed {SEED}), {pixels / 1e6:.1f} M output "
          f"pixels, each from M = {len(passes)} passes: [N, K, c, c] logits on letterbox canvases c = {', '.join(map(str, canvases))} "
          f"(fit_sizes(longer=c), 'center'), plain and mirrored; bilinear; summed in pass order, argmax over K; library: {os.path.basename(_lib_path())}")
    print(f"{args.rounds} rounds of {args.batches} batches per contestant, alternating; ms per batch: median [min .. max]; peak: the growth of "
          "torch.cuda.max_memory_allocated over one call")
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    for k in (19, 150):
        for dtype in (torch.float32, torch.bfloat16):
            batches = [torch.randn((n, k, c, c), device="cuda", generator=gen).to(dtype) for c, _ in passes]
            items = [b[i] for b in batches for i in range(n)]
            members = [[p * n + i for p in range(len(passes))] for i in range(n)]

            def loop():
                out = []
                for i in range(n):
                    s = None
                    for j in members[i]:
                        y0, x0, h, w = regions[j]
                        r = aa.linear_forward(items[j][:, y0:y0 + h, x0:x0 + w].float()[None], list(shapes[i]))[0]
                        r = r.flip(-1) if flips[j] else r
                        s = r if s is None else s.add_(r)
                    out.append(s.argmax(0))
                return out

            def values_then_sum():
                vals = aa.resize_many_back(items, [shapes[g] for g in groups], regions=regions, flips=flips, out_dtype=torch.float32)
                out = []
                for i in range(n):
                    s = vals[members[i][0]]
                    for j in members[i][1:]:
                        s = s + vals[j]
                    out.append(s.argmax(0))
                return out

            def merged():
                return aa.resize_many_back_merged(items, groups, shapes, regions=regions, flips=flips, reduce="argmax")

            contestants = {"a: loop: linear_forward, flip, add per member; argmax per image": loop,
                           "b: resize_many_back(reduce=None) of all members; add, argmax": values_then_sum,
                           "c: resize_many_back_merged(reduce='argmax')": merged}
            results, fits = {}, {}
            for key, fn in contestants.items():
                try:
                    results[key] = fn()
                    fn()
                    torch.cuda.synchronize()
                    fits[key] = True
                except torch.cuda.OutOfMemoryError:
                    results[key], fits[key] = None, False
                    torch.cuda.empty_cache()
            want = results["c: resize_many_back_merged(reduce='argmax')"]
            agree = []
            for key in list(contestants)[:2]:  # (torch.argmax promises no order among equal sums: the differing labels are counted)
                if fits[key]:
                    agree.append(f"({key[0]}) differs from (c) at {sum(int((p != q).sum()) for p, q in zip(results[key], want))} of {pixels} labels")
                    assert sum(int((p != q).sum()) for p, q in zip(results[key], want)) <= pixels // 10 ** 6, f"({key[0]}) differs from the merged call"
            del results, want
            torch.cuda.empty_cache()
            times = {key: [] for key in contestants if fits[key]}
            for _ in range(args.rounds):
                for key in times:
                    times[key].append(timed(contestants[key]))
            print(f"\nK = {k}, {str(dtype).replace('torch.', '')}: " + "; ".join(agree))
            stat = {}
            for key in contestants:
                if not fits[key]:
                    print(f"  {key:64s} does not fit the device's memory: not timed")
                    continue
                v = times[key]
                stat[key[0]] = (statistics.median(v), min(v), max(v))
                launches = count_launches(torch, contestants[key])
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.max_memory_allocated()
                r = contestants[key]()
                torch.cuda.synchronize()
                peak = torch.cuda.max_memory_allocated() - before
                del r
                m, lo, hi = stat[key[0]]
                print(f"  {key:64s} {m:9.3f} [{lo:9.3f} .. {hi:9.3f}]   launches {launches if launches is not None else 'not measured'}"
                      f"   peak {peak / 1e6:10.1f} MB")
            mc, lc, hc = stat["c"]
            for other in ("a", "b"):
                if other in stat:
                    mo, lo, ho = stat[other]
                    verdict = "(c) is faster" if mo - mc > (ho - lo) + (hc - lc) else f"(c) IS NOT FASTER than ({other}) by more than the spreads"
                    print(f"  (c) against ({other}): {mo / mc:.2f} x; median gain {mo - mc:.3f} ms, the two spreads together {(ho - lo) + (hc - lc):.3f} ms: {verdict}")
            del batches, items
            torch.cuda.empty_cache()


def _run_contestants(args, torch, timed, contestants):
    """A generator of two steps.  First every contestant is warmed (one that does not fit the device's memory is reported and not timed)
    -> {key: the warm-up's result, kept for the first two; None otherwise}.  Then they are timed, alternating, and printed: ms per batch
    as median [min .. max], the kernel launches and the growth of torch.cuda.max_memory_allocated over one call
    -> {a key's first letter: (median, min, max)}."""
    results, fits = {}, {}
    for key, fn in contestants.items():
        try:
            r = fn()
            results[key] = r if len(results) < 2 else None  # (the first two are compared; a third set of outputs need not stay)
            del r
            fn()
            torch.cuda.synchronize()
            fits[key] = True
        except torch.cuda.OutOfMemoryError:
            results[key], fits[key] = None, False
            torch.cuda.empty_cache()
    yield results
    results.clear()
    torch.cuda.empty_cache()
    times = {key: [] for key in contestants if fits[key]}
    for _ in range(args.rounds):
        for key in times:
            times[key].append(timed(contestants[key]))
    stat = {}
    for key in contestants:
        if not fits[key]:
            print(f"  {key:76s} does not fit the device's memory: not timed")
            continue
        v = times[key]
        stat[key[0]] = (statistics.median(v), min(v), max(v))
        launches = count_launches(torch, contestants[key])
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.max_memory_allocated()
        r = contestants[key]()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        del r
        m, lo, hi = stat[key[0]]
        print(f"  {key:76s} {m:9.3f} [{lo:9.3f} .. {hi:9.3f}]   launches {launches if launches is not None else 'not measured'}"
              f"   peak {peak / 1e6:10.1f} MB")
    yield stat


def _against(stat, c, other, what):
    """One line: contestant c against `other`, with the bench's spread rule (a median gain counts when it exceeds the two spreads)."""
    if c not in stat or other not in stat:
        return
    (mc, lc, hc), (mo, lo, ho) = stat[c], stat[other]
    spreads = (ho - lo) + (hc - lc)
    if mo - mc > spreads:
        verdict = f"({c}) is faster"
    elif mc - mo > spreads:
        verdict = f"({other}) WINS: ({c}) is slower by more than the spreads"
    else:
        verdict = f"({c}) and ({other}) are NOT APART by more than the spreads"
    print(f"  ({c}) against ({other}), {what}: {mo / mc:.2f} x; median gain {mo - mc:.3f} ms, the two spreads together {spreads:.3f} ms: {verdict}")


def tta_activation(args, torch, aa, timed):
    """--tta --activation: the standard test-time augmentation — per pass the resized logits through a softmax (or sigmoid), un-mirrored,
    the PROBABILITIES summed, then the argmax — on --tta's geometry.  (a) is the loop a user writes today; (c) is
    resize_many_back_merged(activation=..., reduce='argmax'); (d) is the same call with activation=None, so (c) - (d) is what the
    activation costs.  torch's exp is not this library's, so near-ties may fall the other way: the share of differing labels is
    reported, not asserted."""
    from interpolate_antialiasing_amd import boxmath

    act = args.activation
    n, canvases = 16, (384, 512, 640)
    rng = np.random.default_rng(SEED)
    shapes = [(int(rng.integers(1080, 3001)), int(rng.integers(1440, 4001))) for _ in range(N)][:n]
    passes = [(c, flip) for c in canvases for flip in (False, True)]
    regions, flips, groups = [], [], []
    for c, flip in passes:  # (a batch is laid out pass by pass: the groups interleave)
        regions += boxmath.placed_regions(boxmath.fit_sizes(shapes, longer=c), "center", (c, c))
        flips += [flip] * n
        groups += list(range(n))
    pixels = sum(h * w for h, w in shapes)
    print(f"resize_many_bench --tta --activation {act}: N = {n} camera-sized images, H in [1080, 3000], W in [1440, 4000] (seed {SEED}), "
          f"{pixels / 1e6:.1f} M output pixels, each from M = {len(passes)} passes: [N, K, c, c] logits on letterbox canvases c = "
          f"{', '.join(map(str, canvases))} (fit_sizes(longer=c), 'center'), plain and mirrored; bilinear; {act} per pass, probabilities summed in "
          f"pass order, argmax over K; library: {os.path.basename(_lib_path())}")
    print(f"{args.rounds} rounds of {args.batches} batches per contestant, alternating; ms per batch: median [min .. max]; peak: the growth of "
          "torch.cuda.max_memory_allocated over one call")
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    for k in (19, 150):
        for dtype in (torch.float32, torch.bfloat16):
            batches = [torch.randn((n, k, c, c), device="cuda", generator=gen).to(dtype) for c, _ in passes]
            items = [b[i] for b in batches for i in range(n)]
            members = [[p * n + i for p in range(len(passes))] for i in range(n)]

            def loop():
                out = []
                for i in range(n):
                    s = None
                    for j in members[i]:
                        y0, x0, h, w = regions[j]
                        r = aa.linear_forward(items[j][:, y0:y0 + h, x0:x0 + w].float()[None], list(shapes[i]))[0]
                        r = r.softmax(0) if act == "softmax" else r.sigmoid_()
                        r = r.flip(-1) if flips[j] else r
                        s = r if s is None else s.add_(r)
                    out.append(s.argmax(0))
                return out

            def merged():
                return aa.resize_many_back_merged(items, groups, shapes, regions=regions, flips=flips, reduce="argmax", activation=act)

            def merged_none():
                return aa.resize_many_back_merged(items, groups, shapes, regions=regions, flips=flips, reduce="argmax")

            a_key = f"a: loop: linear_forward, {act}, flip, add per member; argmax per image"
            c_key = f"c: resize_many_back_merged(activation='{act}', reduce='argmax')"
            contestants = {a_key: loop, c_key: merged, "d: resize_many_back_merged(activation=None, reduce='argmax'): summed logits": merged_none}
            run = _run_contestants(args, torch, timed, contestants)
            results = next(run)
            note = "(a) does not fit"
            if results[a_key] is not None:
                differ = sum(int((p != q).sum()) for p, q in zip(results[a_key], results[c_key]))
                note = f"(a) differs from (c) at {differ} of {pixels} labels ({100.0 * differ / pixels:.5f} %)"
            del results
            print(f"\nK = {k}, {str(dtype).replace('torch.', '')}: {note}")
            stat = next(run)
            _against(stat, "c", "a", "the call against the loop")
            _against(stat, "d", "c", "what the activation costs")
            del batches, items
            torch.cuda.empty_cache()


def logits_activation(args, torch, aa, timed):
    """--logits --activation: probabilities at the images' own sizes, reduce=None, on --logits' geometry.  (a) is the loop a user writes
    today, linear_forward and softmax (or sigmoid) per item; (c) is resize_many_back(activation=...); (d) the same call with
    activation=None.  The largest difference between (a) and (c) is reported, not asserted (torch's exp is not this library's)."""
    from interpolate_antialiasing_amd import boxmath

    act = args.activation
    n, canvas = 16, (512, 512)
    rng = np.random.default_rng(SEED)
    shapes = [(int(rng.integers(1080, 3001)), int(rng.integers(1440, 4001))) for _ in range(N)][:n]
    regions = boxmath.placed_regions(boxmath.fit_sizes(shapes, longer=canvas[0]), "center", canvas)
    pixels = sum(h * w for h, w in shapes)
    print(f"resize_many_bench --logits --activation {act}: [N, K, {canvas[0]}, {canvas[1]}] logits on a letterbox canvas (fit_sizes(longer="
          f"{canvas[0]}), 'center') back to N = {n} camera-sized images, H in [1080, 3000], W in [1440, 4000] (seed {SEED}), {pixels / 1e6:.1f} M "
          f"output pixels; bilinear; {act} over K, probabilities in the logits' dtype; library: {os.path.basename(_lib_path())}")
    print(f"{args.rounds} rounds of {args.batches} batches per contestant, alternating; ms per batch: median [min .. max]; peak: the growth of "
          "torch.cuda.max_memory_allocated over one call")
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    for k in (19, 150):
        for dtype in (torch.float32, torch.bfloat16):
            x = torch.randn((n, k) + canvas, device="cuda", generator=gen).to(dtype)

            def loop():
                out = []
                for i, (y0, x0, h, w) in enumerate(regions):
                    r = aa.linear_forward(x[i, :, y0:y0 + h, x0:x0 + w].float()[None], list(shapes[i]))[0]
                    out.append((r.softmax(0) if act == "softmax" else r.sigmoid_()).to(dtype))
                return out

            def call():
                return aa.resize_many_back(x, shapes, regions=regions, activation=act)

            def call_none():
                return aa.resize_many_back(x, shapes, regions=regions)

            a_key = f"a: loop: linear_forward(crop.float()), {act}, .to(dtype) per item"
            c_key = f"c: resize_many_back(activation='{act}', reduce=None)"
            contestants = {a_key: loop, c_key: call, "d: resize_many_back(activation=None, reduce=None): logits": call_none}
            run = _run_contestants(args, torch, timed, contestants)
            results = next(run)
            note = "a contestant does not fit"
            if results[a_key] is not None and results[c_key] is not None:
                worst = max(float((p.float() - q.float()).abs().max()) for p, q in zip(results[a_key], results[c_key]))
                note = f"(a) and (c) differ by at most {worst:.3e}"
            del results
            print(f"\nK = {k}, {str(dtype).replace('torch.', '')}: {note}")
            stat = next(run)
            _against(stat, "c", "a", "the call against the loop")
            _against(stat, "d", "c", "what the activation costs")
            del x
            torch.cuda.empty_cache()


def back_bwd_workload(which, torch, k, dtype):
    """The two geometries of --logits-backward -> (canvas, regions, flips, gradients [K, oh_i, ow_i] on the GPU, their bytes): "large",
    --logits' 16 camera-sized images from a 512 x 512 letterbox canvas; "small", 64 images with sides drawn from 240 .. 640 from a
    128 x 128 letterbox canvas.  Odd items are flipped.  (tools/workload.py back_bwd:... runs the same for the counter passes.)"""
    from interpolate_antialiasing_amd import boxmath

    rng = np.random.default_rng(SEED)
    if which == "large":
        canvas = (512, 512)
        shapes = [(int(rng.integers(1080, 3001)), int(rng.integers(1440, 4001))) for _ in range(N)][:16]
    else:
        canvas = (128, 128)
        shapes = [(int(rng.integers(240, 641)), int(rng.integers(240, 641))) for _ in range(64)]
    regions = boxmath.placed_regions(boxmath.fit_sizes(shapes, longer=canvas[0]), "center", canvas)
    flips = [i % 2 == 1 for i in range(len(shapes))]
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    grads = [torch.randn((k, h, w), device="cuda", generator=gen).to(dtype) for h, w in shapes]
    return canvas, regions, flips, grads, sum(g.numel() * g.element_size() for g in grads)


def logits_backward(args, torch, aa, timed):
    """resize_many_back_backward against the per-item loop a user writes today, on --logits' geometry and on many small items.  Per
    contestant: kernel launches, ms per batch (median and minimum over the rounds), and the growth of torch.cuda.max_memory_allocated."""
    print(f"resize_many_bench --logits-backward: gradients at the images' own sizes back to a letterbox canvas, bilinear, odd items flipped (seed {SEED}); "
          f"library: {os.path.basename(_lib_path())}")
    print(f"{args.rounds} rounds per contestant, alternating, every contestant warmed up first (the loop's table cache is warm); ms per batch: "
          "median, minimum [min .. max]; peak: the growth of torch.cuda.max_memory_allocated over one call")
    for which, ks, batches in (("small", (21,), args.batches), ("large", (1, 19, 150), max(2, args.batches // 5))):
        for k in ks:
            for dtype in (torch.float32, torch.bfloat16):
                canvas, regions, flips, grads, gbytes = back_bwd_workload(which, torch, k, dtype)
                n = len(grads)

                def loop():
                    out = torch.zeros((n, k) + canvas, dtype=dtype, device="cuda")
                    for i, (y0, x0, h, w) in enumerate(regions):
                        g = grads[i].flip(-1) if flips[i] else grads[i]
                        out[i, :, y0:y0 + h, x0:x0 + w] = aa.linear_backward(g[None], list(g.shape[1:]), [1, k, h, w])[0]
                    return out

                def call():
                    return aa.resize_many_back_backward(grads, canvas, regions=regions, flips=flips)

                contestants = {"loop: linear_backward per item, flipped, into a zeroed canvas": loop, "call: resize_many_back_backward": call}
                a, b = loop(), call()
                same = a.dtype == b.dtype and torch.equal(a.view(torch.int32 if dtype == torch.float32 else torch.int16),
                                                           b.view(torch.int32 if dtype == torch.float32 else torch.int16))
                assert same, "resize_many_back_backward differs from the loop"
                del a, b
                for fn in contestants.values():
                    fn()
                torch.cuda.synchronize()
                args_batches, args.batches = args.batches, batches
                times = {key: [] for key in contestants}
                for _ in range(args.rounds):
                    for key, fn in contestants.items():
                        times[key].append(timed(fn))
                args.batches = args_batches
                out_mb = n * k * canvas[0] * canvas[1] * grads[0].element_size() / 1e6
                print(f"\n{which}: N = {n}, K = {k}, canvas {canvas[0]} x {canvas[1]}, {str(dtype).replace('torch.', '')}; gradients {gbytes / 1e6:.1f} MB, "
                      f"result {out_mb:.1f} MB; {batches} batches a round; the same bits")
                stat = {}
                for key, v in times.items():
                    stat[key] = (statistics.median(v), min(v), max(v))
                    launches = count_launches(torch, contestants[key])
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    before = torch.cuda.max_memory_allocated()
                    r = contestants[key]()
                    torch.cuda.synchronize()
                    peak = torch.cuda.max_memory_allocated() - before
                    del r
                    print(f"  {key:66s} median {stat[key][0]:9.3f}  min {stat[key][1]:9.3f} [{stat[key][1]:9.3f} .. {stat[key][2]:9.3f}]   launches "
                          f"{launches if launches is not None else 'not measured'}   peak {peak / 1e6:10.1f} MB")
                (ml, ll, hl), (mc, lc, hc) = stat.values()
                verdict = "the one call is faster" if ml - mc > (hl - ll) + (hc - lc) else "THE ONE CALL IS NOT FASTER by more than the spreads"
                print(f"  call against loop: {ml / mc:.2f} x; median gain {ml - mc:.3f} ms, the two spreads together {(hl - ll) + (hc - lc):.3f} ms: {verdict}"
                      + ("" if which == "small" else "  (recorded, not a requirement)"))
                del grads


def _lib_path():
    from interpolate_antialiasing_amd import _lib

    return _lib.LIB_PATH


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--trace-mode", default="bilinear")
    ap.add_argument("--summarise", default=None)
    ap.add_argument("--float-only", action="store_true")
    ap.add_argument("--placed", action="store_true", help="only the placed call (eval and letterbox) against the per-image loop")
    ap.add_argument("--patches", action="store_true", help="only resize_many_to_patches against the per-item composition")
    ap.add_argument("--gap", action="store_true", help="only Pillow's reducing_gap for a list: the loop, resize_many without a gap, and the new step")
    ap.add_argument("--alpha", action="store_true", help="only Pillow's RGBA resize for a list: the loop with alpha=True against resize_many(alpha=True)")
    ap.add_argument("--nearest", action="store_true", help="only Pillow's NEAREST for label maps: resize_many_nearest against the per-image torch loop")
    ap.add_argument("--maps", action="store_true", help="only Pillow's I;16 resize for measured maps: resize_many_maps against the call per item")
    ap.add_argument("--ycbcr", action="store_true", help="only resize_many_ycbcr (4:2:0 planes in) against resize_many_to_float on interleaved RGB "
                    "and against the torch conversion a user writes today; with --trace K: K calls of the planar form for a kernel trace")
    ap.add_argument("--embed", action="store_true", help="only resize_embed_to_tokens and its backward against one existing call per distinct grid; "
                    "with --trace K: K calls of each for a kernel trace")
    ap.add_argument("--logits", action="store_true", help="only resize_many_back: canvas logits back to the images' sizes and argmax, against the "
                    "per-item loop of existing calls and against reduce=None followed by argmax")
    ap.add_argument("--logits-backward", action="store_true", help="only resize_many_back_backward: gradients at the images' sizes back to the "
                    "canvas, against the per-item loop of linear_backward into a zeroed canvas; --logits' geometry and 64 small items")
    ap.add_argument("--tta", action="store_true", help="only resize_many_back_merged: 6 test-time passes per image summed and reduced to the argmax, "
                    "against resize_many_back(reduce=None) plus torch adds and against the per-member loop of linear_forward")
    ap.add_argument("--activation", choices=("softmax", "sigmoid"), default=None,
                    help="with --tta or --logits: the activation before the sum / the store, against the loop with torch's softmax / sigmoid "
                    "and against the same call with activation=None")
    ap.add_argument("--rate-only", action="store_true", help="with --gap: only the reduce kernels' own rate (dense against ragged)")
    ap.add_argument("--trace-patches", action="store_true", help="with --trace: the calls are resize_many_to_patches (the --patches workload); "
                    "with --summarise: kernel times only")
    ap.add_argument("--trace-float", action="store_true", help="with --trace: the calls are resize_many_to_float (bfloat16, nchw, mean / std, flips)")
    args = ap.parse_args()

    rng = np.random.default_rng(SEED)
    shapes = sizes(rng)
    if args.summarise:
        calls = WARM_CALLS + max(args.trace, 1)
        med = summarise(args.summarise, calls)
        if args.trace_patches:
            return
        brng = np.random.default_rng(SEED + 1)
        boxes = [random_resized_crop_box(brng, h, w) for h, w in shapes]
        hull, inter, out = algorithm_bytes(shapes, boxes, MODES[args.trace_mode])
        print(f"bytes one batch moves ({args.trace_mode}, one draw of boxes): hull in {hull / 1e6:.2f} MB + intermediate {inter / 1e6:.2f} MB twice + out {out / 1e6:.2f} MB")
        for k, b in (("many_hpass", hull + inter), ("many_vpass", inter + out)):
            if k in med:
                print(f"  {k}: {b / 1e6:.2f} MB over {med[k]:.1f} us = {b / med[k] / 1e6:.3f} TB/s")
        return

    import torch

    from interpolate_antialiasing_amd import extension_interpolate as aa
    from interpolate_antialiasing_amd import tables

    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    # every image in one flat buffer, uploaded once; the items are HWC views into it (at whatever alignment their offsets give)
    flat = rng.integers(0, 256, sum(h * w * 3 for h, w in shapes), dtype=np.uint8)
    dev_flat = torch.from_numpy(flat).cuda()
    images, off = [], 0
    for h, w in shapes:
        images.append(dev_flat[off:off + h * w * 3].view(h, w, 3).permute(2, 0, 1))
        off += h * w * 3
    brng = np.random.default_rng(SEED + 1)

    def fresh_boxes():
        return [random_resized_crop_box(brng, h, w) for h, w in shapes]

    if args.trace and args.ycbcr:
        ycbcr(args, torch, aa, None)
        return
    if args.trace and args.embed:
        embed(args, torch, aa, None)
        return
    if args.trace:
        for _ in range(WARM_CALLS + args.trace):
            if args.trace_patches:
                from interpolate_antialiasing_amd import boxmath

                aa.resize_many_to_patches(images, (14, 14), "bicubic", sizes=boxmath.fit_patch_sizes(shapes, (14, 14), max_tokens=256),
                                          out_dtype=torch.bfloat16, mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375])
            elif args.trace_float:
                aa.resize_many_to_float(images, list(OUT), args.trace_mode, boxes=fresh_boxes(), flips=[i % 2 == 1 for i in range(N)],
                                        out_dtype=torch.bfloat16, out_format="nchw", mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375])
            else:
                aa.resize_many(images, list(OUT), args.trace_mode, boxes=fresh_boxes())
        torch.cuda.synchronize()
        return

    fwd = {"bilinear": aa.linear_forward, "bicubic": aa.cubic_forward}
    fixed = fresh_boxes()
    tables.BOX_CACHE_SIZE = max(tables.BOX_CACHE_SIZE, 4 * N)  # (b) only stays warm if the LRU can hold its N pairs

    def loop(mode, boxes):
        f = fwd[mode]
        for img, bx in zip(images, boxes):
            f(img[None], list(OUT), box=bx)

    def timed(fn):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(args.batches):
            fn()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / args.batches

    if args.placed:
        placed(args, torch, aa, images, shapes, timed)
        return
    if args.patches:
        patches(args, torch, aa, images, shapes, timed)
        return
    if args.gap:
        (reduce_rate if args.rate_only else gap)(args, torch, aa, timed)
        return
    if args.alpha:
        alpha(args, torch, aa, shapes, timed)
        return
    if args.nearest:
        nearest(args, torch, aa, timed)
        return
    if args.maps:
        maps(args, torch, aa, timed)
        return
    if args.ycbcr:
        ycbcr(args, torch, aa, timed)
        return
    if args.embed:
        embed(args, torch, aa, timed)
        return
    if args.logits:
        (logits_activation if args.activation else logits)(args, torch, aa, timed)
        return
    if args.logits_backward:
        logits_backward(args, torch, aa, timed)
        return
    if args.tta:
        (tta_activation if args.activation else tta)(args, torch, aa, timed)
        return

    print(f"resize_many_bench: N = {N} interleaved uint8 images, H and W in [256, 1024] (seed {SEED}), one RandomResizedCrop box each -> {OUT}")
    print(f"{args.rounds} rounds of {args.batches} batches per contestant, alternating; ms per batch: median [min .. max]")
    for mode in ([] if args.float_only else MODES):
        contestants = {
            "a: per-image loop, unseen boxes": lambda: loop(mode, fresh_boxes()),
            "b: per-image loop, fixed boxes, warm": lambda: loop(mode, fixed),
            "c: resize_many": lambda: aa.resize_many(images, list(OUT), mode, boxes=fresh_boxes()),
        }
        for fn in contestants.values():  # warm-up of every contestant
            fn()
            fn()
        torch.cuda.synchronize()
        # (c) gives the loop's bytes on the fixed boxes
        want = torch.cat([fwd[mode](img[None], list(OUT), box=bx) for img, bx in zip(images, fixed)])
        assert torch.equal(aa.resize_many(images, list(OUT), mode, boxes=fixed), want), "resize_many differs from the per-image loop"
        times = {k: [] for k in contestants}
        for _ in range(args.rounds):
            for k, fn in contestants.items():
                times[k].append(timed(fn))
        print(f"\n{mode}")
        stat = {}
        for k, v in times.items():
            stat[k] = (statistics.median(v), min(v), max(v))
            print(f"  {k:40s} {stat[k][0]:8.3f} [{stat[k][1]:8.3f} .. {stat[k][2]:8.3f}]")
        (ma, la, ha), (mb, lb, hb), (mc, lc, hc) = stat.values()
        gain, spreads = ma - mc, (ha - la) + (hc - lc)
        verdict = "PASS" if gain > spreads else "FAIL: the design has failed its purpose"
        print(f"  (c) against (a): {ma / mc:.2f} x; median gain {gain:.3f} ms against the two spreads together {spreads:.3f} ms: {verdict}")
        print(f"  (c) against (b): {mb / mc:.2f} x (no bar: what a fused single-launch follow-up would have to beat)")

    # the float batch: the composition against the one call
    mean, std = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
    mean_t, std_t = (torch.tensor(v, device="cuda").view(1, 3, 1, 1) for v in (mean, std))
    flips = [i % 2 == 1 for i in range(N)]
    flip_idx = torch.tensor([i for i in range(N) if flips[i]], device="cuda")
    mode = "bicubic"

    def composition(dtype, boxes):
        y = ((aa.resize_many(images, list(OUT), mode, boxes=boxes).float() - mean_t) / std_t).to(dtype).contiguous()
        y[flip_idx] = y[flip_idx].flip(-1)
        return y

    def one_call(dtype, boxes):
        return aa.resize_many_to_float(images, list(OUT), mode, boxes=boxes, flips=flips, out_dtype=dtype, out_format="nchw", mean=mean, std=std)

    print(f"\nthe float batch ({mode}, nchw, mean / std, {len(flip_idx)} of {N} items flipped; library: {os.path.basename(_lib_path())})")
    for dtype in (torch.bfloat16, torch.float32):
        contestants = {
            "d: resize_many + torch conversion": lambda: composition(dtype, fresh_boxes()),
            "e: resize_many_to_float": lambda: one_call(dtype, fresh_boxes()),
        }
        for fn in contestants.values():
            fn()
            fn()
        torch.cuda.synchronize()
        a, b = composition(dtype, fixed), one_call(dtype, fixed)
        assert a.stride() == b.stride() and torch.equal(a.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                                                        b.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)), \
            "resize_many_to_float differs from the composition"
        times = {k: [] for k in contestants}
        for _ in range(args.rounds):
            for k, fn in contestants.items():
                times[k].append(timed(fn))
        print(f"\n{str(dtype).replace('torch.', '')}")
        stat = {}
        for k, v in times.items():
            stat[k] = (statistics.median(v), min(v), max(v))
            print(f"  {k:40s} {stat[k][0]:8.3f} [{stat[k][1]:8.3f} .. {stat[k][2]:8.3f}]")
        (md, ld, hd), (me, le, he) = stat.values()
        gain, spreads = md - me, (hd - ld) + (he - le)
        verdict = "PASS" if gain > spreads else "FAIL: the gain is within the spread"
        print(f"  (e) against (d): {md / me:.2f} x; median gain {gain:.3f} ms against the two spreads together {spreads:.3f} ms: {verdict}")


if __name__ == "__main__":
    main()
