#!/usr/bin/env python3
"""Do two developer builds of libaa_interp.so (make TUNING=-DAA_V2_TUNING, in separate trees) give every fused launch the same shape?

    python tools/launch_shape_ab.py LIB_A LIB_B [--out DIR]

For each library a fresh child process (the Python package of the library's own tree, AA_INTERP_LIB, with AA_V3_DEBUG, AA_F32_DEBUG and AA_UP_DEBUG set, under its own time limit)
runs the list of small problems below and its debug lines are collected: strips per workgroup, resident workgroups, row bands, groups
and grid of every launch, as the library printed them.  The two logs must be identical, with a launch line for every problem; prints their sha256 and exits 1 if they are not.
A problem that raises, a GPU fault included, ends its child at once, and the tool with it: nothing more is launched.
The first-generation uint8 kernel prints no line: its shapes are covered by tests/test_launch_shape_frozen_cpu.py alone.
Every tensor stays under 64 MB; a child takes well under a minute."""
import argparse
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIXES = ("[aa v3]", "f32:", "up:", "# ")


def tree_of(lib):
    """The checkout a library was built in (TREE/interpolate_antialiasing_amd/csrc/libaa_interp.so), else this one: a library is
    loaded by its own tree's Python package, which declares exactly the symbols that library exports."""
    tree = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(lib))))
    return tree if os.path.isfile(os.path.join(tree, "interpolate_antialiasing_amd", "__init__.py")) else ROOT


def child():
    sys.path.insert(0, tree_of(os.environ["AA_INTERP_LIB"]))
    import torch

    from interpolate_antialiasing_amd import _lib
    from interpolate_antialiasing_amd import extension_interpolate as aa

    dev = torch.device("cuda", 0)

    def u8(n, h, w, planar=False):  # channels_last unless planar
        if planar:
            return torch.randint(0, 256, (n, 3, h, w), dtype=torch.uint8, device=dev)
        return torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device=dev).permute(0, 3, 1, 2)

    def fl(n, h, w, dtype=torch.float32):
        return torch.rand((n, 3, h, w), dtype=dtype, device=dev)

    def run(name, fn):
        sys.stderr.write(f"# {name}\n")
        sys.stderr.flush()
        fn()  # every problem is one both libraries serve: any exception, a GPU fault among them, ends the child, and nothing more is launched
        torch.cuda.synchronize()
        sys.stderr.write(f"# -> {_lib.last_variant()}\n")
        sys.stderr.flush()

    # ---- fused uint8 (v3): 1 strip, 2-8 strips, more than 8; under one round and several rounds; oH below 16; plane groups
    run("u8 1 strip", lambda: aa.linear_forward(u8(2, 100, 120), [40, 48]))
    run("u8 4 strips", lambda: aa.linear_forward(u8(2, 438, 906), [196, 256]))
    run("u8 5 strips", lambda: aa.linear_forward(u8(2, 438, 906), [196, 320]))
    run("u8 5 strips, 32 images", lambda: aa.linear_forward(u8(32, 438, 906), [196, 320]))
    run("u8 11 strips", lambda: aa.linear_forward(u8(2, 300, 1400), [128, 700]))
    run("u8 one image", lambda: aa.linear_forward(u8(1, 72, 40), [32, 20]))
    run("u8 4000 images", lambda: aa.linear_forward(u8(4000, 72, 40), [32, 20]))
    run("u8 oH 12", lambda: aa.linear_forward(u8(4, 100, 200), [12, 100]))
    run("u8 bicubic", lambda: aa.cubic_forward(u8(8, 438, 906), [196, 320]))
    run("u8 growing", lambda: aa.linear_forward(u8(2, 196, 320), [438, 906]))
    run("u8 planar, plane groups", lambda: aa.linear_forward(u8(4, 438, 906, planar=True), [196, 320]))
    _lib.set_plane_groups(0)
    run("u8 planar, single planes", lambda: aa.linear_forward(u8(4, 438, 906, planar=True), [196, 320]))
    _lib.set_plane_groups(1)
    # ---- fused float, shrinking heights: the same strip counts; the saturation model (21-tap fp32 bicubic); the doubling rule (fp16 bilinear)
    run("f32 1 strip", lambda: aa.linear_forward(fl(2, 100, 120), [40, 48]))
    run("f32 4 strips", lambda: aa.linear_forward(fl(2, 438, 906), [196, 256]))
    run("f32 5 strips", lambda: aa.linear_forward(fl(8, 438, 906), [196, 320]))
    run("f32 11 strips", lambda: aa.linear_forward(fl(2, 300, 1400), [128, 700]))
    run("f32 one image", lambda: aa.linear_forward(fl(1, 72, 40), [32, 20]))
    run("f32 1500 images", lambda: aa.linear_forward(fl(1500, 72, 40), [32, 20]))
    run("f32 oH 12", lambda: aa.linear_forward(fl(4, 100, 200), [12, 100]))
    run("f32 bicubic 21 taps", lambda: aa.cubic_forward(fl(4, 1024, 1024), [224, 224]))
    run("f16 bicubic 21 taps", lambda: aa.cubic_forward(fl(4, 1024, 1024, torch.float16), [224, 224]))
    run("f16 bilinear", lambda: aa.linear_forward(fl(8, 1024, 1024, torch.float16), [224, 224]))
    run("bf16 bilinear channels_last", lambda: aa.linear_forward(fl(8, 438, 906, torch.bfloat16).contiguous(memory_format=torch.channels_last),
                                                               [196, 320]))
    # ---- fused float, growing heights and the backward
    run("up 1 strip", lambda: aa.linear_forward(fl(4, 20, 30), [72, 40]))
    run("up forward", lambda: aa.linear_forward(fl(4, 196, 320), [438, 906]))
    run("up forward, 8 images", lambda: aa.linear_forward(fl(8, 196, 320), [438, 906]))
    run("up 10 strips", lambda: aa.linear_forward(fl(2, 40, 700), [100, 2400]))
    run("up oH 20", lambda: aa.linear_forward(fl(2, 10, 30), [20, 100]))
    run("up 1500 images", lambda: aa.linear_forward(fl(1500, 32, 20), [72, 40]))
    run("backward, multi-strip gradient", lambda: aa.linear_backward(fl(4, 196, 320), [196, 320], [4, 3, 438, 906]))
    run("backward, bicubic", lambda: aa.cubic_backward(fl(4, 196, 320), [196, 320], [4, 3, 438, 906]))
    run("backward, 10 strips", lambda: aa.linear_backward(fl(2, 40, 700), [40, 700], [2, 3, 100, 2400]))
    run("backward, one strip", lambda: aa.linear_backward(fl(2, 40, 48), [40, 48], [2, 3, 100, 60]))
    run("backward, f16", lambda: aa.linear_backward(fl(4, 196, 320, torch.float16), [196, 320], [4, 3, 438, 906]))


def collect(lib, limit):
    env = dict(os.environ, AA_INTERP_LIB=os.path.abspath(lib), AA_V3_DEBUG="1", AA_F32_DEBUG="1", AA_UP_DEBUG="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=limit)
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith(PREFIXES)]
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        raise SystemExit(f"the child of {lib} ended with status {r.returncode}")
    return "\n".join(lines) + "\n"


def silent_problems(log):
    """The problems of a log under whose heading no launch line stands."""
    silent, name, seen = [], None, True
    for ln in log.splitlines():
        if ln.startswith("# -> "):
            continue
        if ln.startswith("# "):
            if not seen:
                silent.append(name)
            name, seen = ln[2:], False
        else:
            seen = True
    return silent if seen else silent + [name]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=None, help="directory for the two logs")
    ap.add_argument("--limit", type=int, default=120, help="seconds per child")
    a = ap.parse_args()
    if a.child:
        return child()
    if len(a.libs) != 2:
        ap.error("two libraries")
    logs = [collect(lib, a.limit) for lib in a.libs]
    for name, lib, log in zip(("launch_shapes_a.log", "launch_shapes_b.log"), a.libs, logs):
        shapes = [ln for ln in log.splitlines() if not ln.startswith("# ")]
        print(f"{lib}: {len(shapes)} launch lines, sha256 {hashlib.sha256(log.encode()).hexdigest()}")
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, name), "w") as f:
                f.write(log)
    for lib, log in zip(a.libs, logs):
        if silent_problems(log):  # equal logs prove nothing about a problem that printed no shape
            print(f"{lib}: no launch line for: {', '.join(silent_problems(log))}")
            return 1
    if logs[0] != logs[1]:
        a_, b_ = logs[0].splitlines(), logs[1].splitlines()
        first = next((i for i, (x, y) in enumerate(zip(a_, b_)) if x != y), min(len(a_), len(b_)))
        print(f"DIFFERENT from line {first + 1}:\n  {a_[first] if first < len(a_) else '<end>'}\n  {b_[first] if first < len(b_) else '<end>'}")
        return 1
    print("identical")
    return 0


if __name__ == "__main__":
    sys.exit(main())
