"""Makes tests/golden/launch_shapes.json: the launch shapes (strips per workgroup, row bands, groups, grid) commit 02b5bb4 gave, the last
one whose four fused families each chose them in their own launch code.  tests/test_launch_shape_frozen_cpu.py feeds every row through
aa_probe_launch_shape (csrc/aa_launch_shape.h) and requires the same four numbers.

The sources come from `git archive 02b5bb4` into a temporary directory.  A stand-alone host program (hipcc --cuda-host-only, no GPU)
includes that commit's three impl headers and calls its own pick_ybands, pick_ybands_f and pick_ybands_up.  The few lines around those
functions have no callable form there; the program restates them from that commit's text, each with its line numbers:
  aa_fused_u8_v3_impl.h:938-958       v3: occupancy fallback 16 / s, the drop to single-strip workgroups, grid padding
  aa_fused_float_impl.h:499-526       float down: the 64 KiB limit, fallback from LDS, the drop, what the saturation model is given
  aa_fused_float_up_impl.h:511-536    float up: the same limit, fallback and drop
  aa_fused_u8.hip:318-346             v1: blocks per CU from a formula and the band loop (inline there, so restated whole)
The program also names the branches a row took; this script requires at least 20 rows for every branch.  CU count 256 throughout.

Usage: python tests/golden/make_golden_launch_shapes.py   (from a checkout with the history; writes the JSON next to this file)"""
import collections
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PARENT = "02b5bb4"
CUS = 256
V1, V3, DOWN, UP = 0, 1, 2, 3
COLUMNS = ["family", "nstrips", "spb", "forced", "items", "H", "oH", "taps_h", "taps_w", "lds", "saturation", "threads", "occupancy",
           "out_spb", "out_ybands", "out_groups", "out_grid"]
BRANCHES = [
    "spb_kept", "spb_dropped", "spb_forced", "fallback_v3", "fallback_down_lds", "fallback_down_cap", "fallback_up_lds", "fallback_up_cap",
    "lds_over_64k_down", "lds_over_64k_up", "max_yb_1", "max_yb_1_up", "cap_64", "tie", "sat_on", "sat_off", "double_on", "double_off",
    "double_clamped", "target_on", "target_off", "target_clamp_max", "target_clamp_64", "v1_cap_lds", "v1_cap_waves", "v1_cap_8", "grid_over",
]

HARNESS = r"""
#include <stdio.h>
#include <string>
#include "aa_fused_u8_v3_impl.h"
#include "aa_fused_float_impl.h"
#include "aa_fused_float_up_impl.h"
int aa_device_cu_count() { return 256; }
int g_aa_store_form = -1;
int g_aa_plane_groups = 1;

int main() {
  int fam, nstrips, spb, forced, th, tw, sat, threads, occ[9];
  long long items, H, oH, lds_ll;
  while (scanf("%d %d %d %d %lld %lld %lld %d %d %lld %d %d %d %d %d %d %d %d %d %d", &fam, &nstrips, &spb, &forced, &items, &H, &oH, &th, &tw,
               &lds_ll, &sat, &threads, &occ[1], &occ[2], &occ[3], &occ[4], &occ[5], &occ[6], &occ[7], &occ[8]) == 20) {
    const size_t lds = (size_t)lds_ll;
    std::string tags;
    auto tag = [&](const char *t) { tags += " "; tags += t; };
    const int spb0 = spb;
    int nb = 0, yb = 1, sgroups = 1;
    long long groups = 0, grid = 0;
    if (fam == 1) {  // aa_fused_u8_v3_impl.h:938-958
      auto resident = [&](int s) {
        int nb = occ[s];
        if (nb <= 0) nb = 16 / s;
        return nb < 1 ? 1 : nb;
      };
      if (spb > 1 && !forced && resident(1) > resident(spb) * spb) spb = 1;
      sgroups = (nstrips + spb - 1) / spb;
      nb = resident(spb);
      yb = pick_ybands(items * sgroups, (double)aa_device_cu_count() * resident(spb), th, H, oH);
      groups = items * yb;
      grid = (items * (long long)yb + 7) / 8 * 8 * sgroups;
      if (occ[spb] <= 0) tag("fallback_v3");
    } else if (fam == 2 || fam == 3) {  // aa_fused_float_impl.h:499-526, aa_fused_float_up_impl.h:511-536
      bool used_lds = false, used_cap = false, over = false;
      auto resident = [&](int s) {
        if (lds * s > 64 * 1024) { over = true; return -1; }
        int nb = occ[s];
        if (nb <= 0) {
          nb = (int)((160 * 1024) / (lds * s > 0 ? lds * s : 1));
          used_lds = true;
          if (nb > 32 / s) { nb = 32 / s; used_cap = true; used_lds = false; }
          if (nb < 1) nb = 1;
        }
        return nb;
      };
      if (spb > 1 && (resident(spb) < 0 || resident(1) > resident(spb) * spb)) spb = 1;
      if (over) tag(fam == 2 ? "lds_over_64k_down" : "lds_over_64k_up");
      sgroups = (nstrips + spb - 1) / spb;
      used_lds = used_cap = false;
      nb = resident(spb);
      if (used_lds) tag(fam == 2 ? "fallback_down_lds" : "fallback_up_lds");
      if (used_cap) tag(fam == 2 ? "fallback_down_cap" : "fallback_up_cap");
      const double slots = (double)aa_device_cu_count() * resident(spb);
      if (fam == 2) yb = pick_ybands_f(items * sgroups, slots, th, tw, H, oH, sat ? resident(spb) * spb : 0);
      else yb = pick_ybands_up(items * sgroups, spb, slots, th, H, oH);
      groups = items * (long long)yb;
      grid = (groups + 7) / 8 * 8 * sgroups;
    } else {  // aa_fused_u8.hip:318-346 (items = N * xbands)
      const int cus = aa_device_cu_count();
      const int waves_per_block = threads / 64;
      int blocks_per_cu = (int)((160 * 1024) / (lds > 0 ? lds : 1));
      const char *cap = "v1_cap_lds";
      if (blocks_per_cu > 32 / waves_per_block) { blocks_per_cu = 32 / waves_per_block; cap = "v1_cap_waves"; }
      if (blocks_per_cu > 8) { blocks_per_cu = 8; cap = "v1_cap_8"; }
      if (blocks_per_cu < 1) blocks_per_cu = 1;
      tag(cap);
      const double slots = (double)cus * blocks_per_cu;
      const int64_t max_yb = oH / 8 > 1 ? oH / 8 : 1;
      int64_t ybands = 1;
      double best = 1e30;
      for (int64_t y = 1; y <= max_yb && y <= 64; y++) {
        const double n_items = (double)items * y;
        const double rounds = n_items / slots;
        const double eff = rounds / ceil(rounds);
        const double halo = 1.0 + (double)(y - 1) * th / (double)H;
        const double cost = halo / eff;
        if (cost < best - 1e-9) {
          best = cost;
          ybands = y;
        }
      }
      nb = blocks_per_cu;
      yb = (int)ybands;
      groups = grid = items * ybands;
    }
    if (grid > 0x7FFFFFFF) { grid = 0; tag("grid_over"); }
    // ---- which branches the row took (for this script's census only; the numbers above are the parent's)
    if (fam != 0) tag(forced && spb0 > 1 ? "spb_forced" : spb0 > 1 && spb == 1 ? "spb_dropped" : spb0 > 1 ? "spb_kept" : "spb_one");
    const long long per_band = fam == 3 ? 16 : 8;
    const long long max_yb = oH / per_band > 1 ? oH / per_band : 1;
    const double slots = 256.0 * nb;
    const long long ipb = items * sgroups;
    bool target = false;
    if (fam == 3) {
      const double tw_ = 20.0 * 256, wpb = (double)ipb * spb;
      target = spb == 1 && wpb <= tw_ * 1.25;
      tag(target ? "target_on" : "target_off");
      if (target) {
        const long long y = (long long)(tw_ / (wpb > 0 ? wpb : 1) + 0.5);
        if (y > max_yb && max_yb <= 64) tag("target_clamp_max");
        if (y > 64 && max_yb > 64) tag("target_clamp_64");
      }
    }
    if (max_yb == 1) tag(fam == 3 ? "max_yb_1_up" : "max_yb_1");
    if (!target) {
      if (max_yb > 64) tag("cap_64");
      for (long long y = 1; y <= max_yb && y <= 64; y++) {
        const double r = (double)ipb * y / slots;
        if (r == ceil(r)) { tag("tie"); break; }
      }
    }
    if (fam == 2) {
      const int wpc = sat ? nb * spb : 0;
      tag(tw > 12 && wpc > 12 ? "sat_on" : "sat_off");
      // the band count before the doubling rule: pick_ybands_f's loop once more, for the census alone
      const double sat_ = (tw > 12 && wpc > 12) ? 12.0 / wpc : 1.0;
      long long m = 1;
      double best = 1e30;
      for (long long y = 1; y <= max_yb && y <= 64; y++) {
        const double rounds = (double)ipb * y / slots;
        const double whole = floor(rounds), part = rounds - whole;
        const double units = whole + (part > 1e-9 ? (part > sat_ ? part : sat_) : 0.0);
        const double cost = (1.0 + (double)(y - 1) * th / (double)H) * units / rounds;
        if (cost < best - 1e-9) { best = cost; m = y; }
      }
      const bool on = tw <= 12 && (double)ipb * m / slots < 8.0;
      tag(!on ? "double_off" : 2 * m > max_yb ? "double_clamped" : "double_on");
    }
    printf("%d %d %lld %lld%s\n", spb, yb, groups, grid, tags.c_str());
  }
  return 0;
}
"""


def cases():
    """Rows of inputs; each generator below aims at one branch of the parent's code, the random mix covers their combinations."""
    rng = random.Random(20261019)
    rows = []

    def occupancy(lds, fail=None, base=None):
        # what the runtime answers: the LDS bound, the wave-slot bound and a register bound drawn per row; -1 where the row says so
        regs = base if base is not None else rng.choice([8, 12, 16, 20, 24, 26, 32])
        occ = []
        for s in range(1, 9):
            nb = min(regs // s, (160 * 1024) // max(lds * s, 1), 32 // s)
            occ.append(nb if nb >= 1 else -1)
        if fail == "all":
            occ = [-1] * 8
        elif fail == "some":
            occ = [-1 if rng.random() < 0.5 else o for o in occ]
        return occ

    def row(fam, nstrips=1, spb=None, forced=0, items=1, H=438, oH=196, taps_h=5, taps_w=5, lds=4096, sat=0, threads=64, occ=None,
            fail=None, base=None):
        if spb is None:
            spb = 1 if fam == V1 else (nstrips if nstrips <= 8 else 4)
        rows.append([fam, nstrips, spb, forced, items, H, oH, taps_h, taps_w, lds, sat, threads, occ or occupancy(lds, fail, base)])

    sizes = [(438, 196), (1024, 224), (72, 40), (1080, 360), (61, 17), (2160, 720), (300, 128), (97, 15), (33, 9), (4000, 1100)]
    up_sizes = [(196, 438), (224, 1024), (40, 72), (438, 1200), (17, 61), (10, 31), (12, 20), (360, 2160), (128, 1500)]
    lds_f = [1536, 2048, 3072, 4096, 6144, 8192, 12288, 16384]

    # -- the random mix: every family, strip counts 1 .. 20, batches from one item to many rounds
    for _ in range(110):
        H, oH = rng.choice(sizes)
        row(V3, nstrips=rng.randint(1, 20), items=rng.choice([1, 2, 3, 8, 64, 256, 1000, 4096]), H=H, oH=oH, taps_h=rng.choice([3, 5, 7, 11, 23]),
            lds=rng.choice([2048, 4096, 6656, 8192, 10240]), fail=rng.choice([None, None, "some"]))
    for _ in range(130):
        H, oH = rng.choice(sizes)
        row(DOWN, nstrips=rng.randint(1, 20), items=rng.choice([1, 3, 6, 48, 192, 768, 3000, 12288]), H=H, oH=oH,
            taps_h=rng.choice([3, 5, 9, 21]), taps_w=rng.choice([2, 5, 9, 12, 13, 21]), lds=rng.choice(lds_f), sat=rng.randint(0, 1),
            fail=rng.choice([None, None, "some"]))
    for _ in range(130):
        H, oH = rng.choice(up_sizes + [(b, a) for a, b in sizes])
        row(UP, nstrips=rng.randint(1, 20), items=rng.choice([1, 3, 6, 48, 192, 768, 3000, 12288]), H=H, oH=oH, taps_h=rng.choice([2, 4, 5, 9]),
            lds=rng.choice([1024, 2048, 4096, 8192]), fail=rng.choice([None, None, "some"]))
    for _ in range(60):
        H, oH = rng.choice(sizes)
        row(V1, items=rng.choice([1, 2, 5, 64, 256, 1024, 5000]), H=H, oH=oH, taps_h=rng.choice([3, 5, 7, 11, 23]),
            lds=rng.choice([3000, 9000, 16000, 22000, 40000, 65536]), threads=64 * rng.randint(1, 16))

    # -- strips per workgroup: kept (4 strips fill the CU), dropped (5 strips leave slots empty), forced
    for fam in (V3, DOWN, UP):
        for i in range(24):
            H, oH = rng.choice(sizes if fam != UP else up_sizes)
            row(fam, nstrips=4, items=3 * (i + 1), H=H, oH=oH, base=24, lds=2048)           # 24 vs 6 * 4: kept
            row(fam, nstrips=5, items=3 * (i + 1), H=H, oH=oH, base=24, lds=2048)           # 24 vs 4 * 5: dropped
    for i in range(30):
        H, oH = rng.choice(sizes)
        row(V3, nstrips=rng.choice([3, 5, 6, 7]), forced=1, spb=rng.randint(2, 8), items=1 + 7 * i, H=H, oH=oH, base=24, lds=2048)

    # -- the occupancy query fails: v3's 16 / s, the float families' estimate from LDS (large rings) and its 32 / s cap (small rings)
    for i in range(24):
        H, oH = rng.choice(sizes)
        row(V3, nstrips=rng.randint(1, 12), items=1 + 11 * i, H=H, oH=oH, fail="all")
        for fam in (DOWN, UP):
            h, o = (H, oH) if fam == DOWN else rng.choice(up_sizes)
            row(fam, nstrips=rng.randint(1, 3), items=1 + 11 * i, H=h, oH=o, lds=rng.choice([8192, 12288, 16384]), fail="all")
            row(fam, nstrips=rng.randint(1, 12), items=1 + 11 * i, H=h, oH=o, lds=rng.choice([512, 1024, 1536]), fail="all")

    # -- workgroups whose rings exceed 64 KiB
    for i in range(24):
        for fam in (DOWN, UP):
            H, oH = rng.choice(sizes if fam == DOWN else up_sizes)
            row(fam, nstrips=rng.choice([5, 6, 7, 8, 16]), spb=rng.choice([5, 6, 7, 8]), items=1 + 5 * i, H=H, oH=oH, lds=rng.choice([14336, 16384]))

    # -- one band only (oH < 16; < 32 for up), and more than 64 bands possible
    for i in range(24):
        row(V3, nstrips=rng.randint(1, 6), items=1 + 40 * i, H=rng.randint(20, 400), oH=rng.randint(1, 15))
        row(DOWN, nstrips=rng.randint(1, 6), items=1 + 40 * i, H=rng.randint(20, 400), oH=rng.randint(1, 15), lds=2048)
        row(V1, items=1 + 40 * i, H=rng.randint(20, 400), oH=rng.randint(1, 15), lds=9000, threads=256)
        row(UP, nstrips=rng.randint(1, 6), items=1 + 40 * i, H=rng.randint(4, 30), oH=rng.randint(16, 31), lds=2048)
        row(rng.choice([V3, DOWN, V1]), items=rng.choice([1, 2, 3, 5]), H=rng.randint(2000, 8000), oH=rng.randint(520, 4000), taps_h=rng.choice([3, 5, 9]),
            lds=2048, threads=128)
        row(UP, nstrips=rng.randint(6, 9), items=rng.choice([1, 2, 3]), H=rng.randint(300, 900), oH=rng.randint(1040, 4000), lds=2048, base=24)

    # -- exact-integer round counts: items a multiple or a simple fraction of the slots, so that costs tie
    for i in range(30):
        nb = rng.choice([4, 6, 8, 12, 24])
        fam = rng.choice([V3, DOWN, UP])
        H, oH = rng.choice(sizes if fam != UP else [(360, 2160), (128, 1500)])
        row(fam, nstrips=rng.choice([1, 2, 4]), items=CUS * nb // rng.choice([1, 2, 4, 8]) * rng.choice([1, 2, 3]), H=H, oH=oH, base=nb,
            lds=1024, taps_w=rng.choice([5, 21]), sat=1)

    # -- float down: saturation model on / off, doubling rule on / off / clamped to max_yb
    for i in range(30):
        H, oH = rng.choice(sizes)
        row(DOWN, nstrips=rng.randint(1, 8), items=rng.choice([3, 48, 192, 768]), H=H, oH=oH, taps_h=21, taps_w=21, lds=4096, sat=1, base=24)
        row(DOWN, nstrips=rng.randint(1, 8), items=rng.choice([3, 48, 192, 768]), H=H, oH=oH, taps_h=21, taps_w=21, lds=4096, sat=0, base=24)
        row(DOWN, nstrips=rng.randint(1, 4), items=rng.choice([3, 12, 48, 192]), H=H, oH=oH, taps_h=5, taps_w=5, lds=2048, sat=1)   # doubled
        row(DOWN, nstrips=rng.randint(4, 20), items=rng.choice([12288, 50000]), H=H, oH=oH, taps_h=5, taps_w=5, lds=2048, sat=1)    # >= 8 rounds
        row(DOWN, nstrips=1, items=rng.choice([1, 2, 3]), H=rng.randint(40, 300), oH=rng.choice([17, 24, 25, 33, 40, 41, 56, 57]), taps_h=3, taps_w=5,
            lds=2048, sat=1)                                                                                                      # clamped

    # -- float up: the target-waves rule on, off (several strips per workgroup, or too many waves), clamped to max_yb and to 64
    for i in range(30):
        H, oH = rng.choice(up_sizes)
        row(UP, nstrips=1, items=rng.choice([48, 192, 768, 3000]), H=H, oH=oH, lds=2048)
        row(UP, nstrips=4, items=rng.choice([48, 192, 768]), H=H, oH=oH, lds=2048, base=24)
        row(UP, nstrips=1, items=rng.choice([6500, 12288, 50000]), H=H, oH=oH, lds=2048)
        row(UP, nstrips=1, items=rng.choice([1, 2, 3]), H=rng.randint(20, 200), oH=rng.randint(32, 1000), lds=2048)    # wants > max_yb bands
        row(UP, nstrips=1, items=rng.choice([1, 2, 3]), H=rng.randint(300, 900), oH=rng.randint(1040, 6000), lds=2048)  # wants > 64 bands

    # -- v1: blocks per CU bounded by LDS, by wave slots, by 8
    for i in range(24):
        H, oH = rng.choice(sizes)
        row(V1, items=1 + 9 * i, H=H, oH=oH, lds=rng.choice([30000, 41000, 65536]), threads=rng.choice([64, 128, 256]))
        row(V1, items=1 + 9 * i, H=H, oH=oH, lds=rng.choice([3000, 6000, 9000]), threads=rng.choice([512, 768, 1024]))
        row(V1, items=1 + 9 * i, H=H, oH=oH, lds=rng.choice([3000, 6000, 9000]), threads=rng.choice([64, 128, 192]))

    # -- more workgroups than a grid holds
    for i in range(24):
        fam = rng.choice([V3, DOWN, UP])
        H, oH = rng.choice(sizes if fam != UP else up_sizes)
        row(fam, nstrips=rng.choice([1, 4, 20]), items=(1 << 31) * rng.choice([1, 2, 3]) + i, H=H, oH=oH, lds=2048)
    for fam in (V3, DOWN, UP):  # the edge itself: one band, one strip, so the grid is the items padded to 8
        for items in ((1 << 31) - 9, (1 << 31) - 8, (1 << 31) - 7, (1 << 31) - 1):
            row(fam, nstrips=1, items=items, H=40, oH=9, lds=2048)
    return rows


def main():
    rows = cases()
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run(f"git -C '{ROOT}' archive {PARENT} | tar -x -C '{tmp}'", shell=True, check=True)
        src = os.path.join(tmp, "launch_shapes_parent.hip")
        with open(src, "w") as f:
            f.write(HARNESS)
        exe = os.path.join(tmp, "launch_shapes_parent")
        subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-std=c++17", "-ffp-contract=off", "-I",
                        os.path.join(tmp, "interpolate_antialiasing_amd", "csrc"), "-I", os.path.join(tmp, "include"), src, "-o", exe], check=True)
        text = "".join(" ".join(str(v) for v in r[:12] + r[12]) + "\n" for r in rows)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(rows), (len(out), len(rows))
    census = collections.Counter()
    table = []
    for r, line in zip(rows, out):
        f = line.split()
        table.append(r + [int(v) for v in f[:4]])
        census.update(f[4:])
    for b in BRANCHES:
        print(f"{b:20s} {census[b]}")
    short = [b for b in BRANCHES if census[b] < 20]
    assert not short, f"fewer than 20 rows: {short}"
    path = os.path.join(HERE, "launch_shapes.json")
    with open(path, "w") as f:
        f.write('{"parent": "%s", "cus": %d, "columns": %s,\n "census": %s,\n "rows": [\n' % (
            PARENT, CUS, json.dumps(COLUMNS), json.dumps({b: census[b] for b in BRANCHES})))
        f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in table))
        f.write("\n]}\n")
    print(len(table), "rows,", os.path.getsize(path), "bytes ->", path)


if __name__ == "__main__":
    sys.exit(main())
