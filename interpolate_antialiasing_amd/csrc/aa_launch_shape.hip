// aa_launch_shape.hip — the launch-shape model of the fused families (aa_launch_shape.h).  Costs are compared as doubles: -ffp-contract=off.
#include "aa_launch_shape.h"
#include <math.h>
#include <stdio.h>
#include <atomic>
#include "aa_common.h"  // aa_knob

namespace {

// aa_set_launch_shape (aa_interp.h): spb in the low byte, ybands above it; 0: the model chooses.  One relaxed load per launch.
std::atomic<int> g_forced_shape{0};
int forced_spb() { return g_forced_shape.load(std::memory_order_relaxed) & 0xFF; }
int forced_ybands() { return g_forced_shape.load(std::memory_order_relaxed) >> 8; }

// ---- what differs between the families, besides the band rules of float down and float up below ------------------------------
struct FamilyPolicy {
  int rows_per_band;   // a band has at least this many output rows: max_yb = oH / rows_per_band
  bool halo_over_out;  // halo rows weigh against H + oH, not H: input rows are the cheap side of the write-bound up kernel
  bool by_lds;         // rings over 64 KiB of LDS make no workgroup (resident = -1); a failed query estimates from LDS, not 16 waves
  bool pad8;           // the grid is padded to whole rounds of the 8 XCDs (see the kernels); v1 launches its groups as they are
};
const FamilyPolicy kPolicy[4] = {
    /* AA_LAUNCH_V1       */ {8, false, false, false},
    /* AA_LAUNCH_V3       */ {8, false, false, true},
    /* AA_LAUNCH_F32_DOWN */ {8, false, true, true},
    /* AA_LAUNCH_F32_UP   */ {16, true, true, true},
};

// workgroups a CU holds going by LDS (160 KiB) and wave slots alone, at most cap
int blocks_by_lds(size_t lds, int waves, int cap = 32) {
  const int nb = (int)((160 * 1024) / (lds > 0 ? lds : 1)), slots = 32 / waves < cap ? 32 / waves : cap;
  return nb > slots ? slots : nb;
}

// ---- row bands ------------------------------------------------------------------------------------------------------------
// Float up, the target-waves rule: the band count, or 0 where the round model below decides.
// Single-strip workgroups whose whole problem fits the chip in about one round: this write-bound kernel is fastest with
// about 20 waves per CU in flight, not with every slot filled over several rounds (measured on one box,
// [64,3,438,906] -> 1200x1200: 7.5 waves per CU 0.32 ms, 15 0.304-0.319, 19 0.297-0.313, 24 x 3 rounds 0.327-0.344).  Workgroups
// of several strips (906-wide gradients: 4 strips with the pacing barrier) measured best with the round model.
int64_t up_target_waves_bands(const aa_launch_shape_in &in, int64_t items_per_band, int spb, int64_t max_yb) {
  const double target_waves = 20.0 * in.cus;
  const double waves_per_band = (double)items_per_band * spb;
  if (spb != 1 || waves_per_band > target_waves * 1.25) return 0;
  const int64_t yb = (int64_t)(target_waves / (waves_per_band > 0 ? waves_per_band : 1) + 0.5), cap = max_yb > 64 ? 64 : max_yb;
  return yb < 1 ? 1 : yb > cap ? cap : yb;
}

// Float down, the saturation model.  Wide windows (> 12 taps: rows heavy in arithmetic and staging, 20 halo rows per band): such a kernel
// reaches its rate with about 12 waves on a CU, so a last (or only) round that fills `sat` of the slots costs no more than its work — and
// fewer, taller bands save halo rows.  Measured, config 2 (21-tap bicubic, 24 waves fit a CU), ms by band count: 2: 0.261, 3: 0.229,
// 4: 0.193, 5: 0.204, 6: 0.206, 8 (one full round, the old choice): 0.200, 10: 0.218; tolerance mode 4: 0.180, 8: 0.194.  Narrow windows
// need every wave they can get to hide memory latency (config A fp32, 26 waves fit: 2 bands 0.310, 10 bands 0.268): sat = 1, the plain
// round model.  (Measured for fp32 only: fp16 bicubic thumbnails lose 20 % with it, and their launch passes 0 waves.)
double down_cost(const aa_launch_shape_in &in, int waves_per_cu, double halo, double rounds) {
  const double sat = (in.taps_w > 12 && waves_per_cu > 12) ? 12.0 / waves_per_cu : 1.0;
  const double whole = floor(rounds), part = rounds - whole;
  const double units = whole + (part > 1e-9 ? (part > sat ? part : sat) : 0.0);  // time, in full-occupancy rounds
  return halo * units / rounds;
}

// Float down, the doubling rule.  Narrow windows (bilinear-class shapes, memory-bound): twice the bands of the round model, while the launch
// is fewer than 8 rounds — shorter work items even out the end of the kernel, and their extra halo rows cost little where the vector ALUs
// are half idle.  Measured (ms, model | doubled): [256,3,438,906] fp32 NCHW 0.287 | 0.271, channels_last 0.283 | 0.264, [64,3,1024,1024]
// fp16 bilinear 0.163 | 0.150; the 21-tap bicubic config (vector-ALU bound) loses with more bands (0.20 | 0.22) and keeps the model.
// (Round 3 tried to keep the doubling to launches of 1.5 rounds and more — fp16 bilinear 1024 -> 224 prefers 8 bands, 0.102 ms, to its 18,
// 0.107 — and lost more elsewhere: fp16 [128,3,438,906] -> (196,320) 0.099 -> 0.110, -> (196,1200) 0.228 -> 0.284.  The rule stays.)
int64_t down_doubled_bands(const aa_launch_shape_in &in, int64_t items_per_band, int64_t ybands, double slots, int64_t max_yb) {
  if (in.taps_w > 12 || (double)items_per_band * ybands / slots >= 8.0) return ybands;
  return 2 * ybands < max_yb ? 2 * ybands : max_yb;
}

// Every extra band re-reads and re-filters ~taps_h halo rows, but the grid must fill the chip's resident wave slots a near-integer
// number of times or the last partial round idles most CUs (v1: 2048 workgroups on 1280 slots ran 2 rounds for 1.6 rounds of work).
// Pick the band count minimising (1 + halo fraction) / round efficiency.  items_per_band: workgroups of one band; slots: resident
// workgroups of the chip; waves_per_cu: resident waves per CU where the saturation model applies, else 0.
int pick_ybands(const aa_launch_shape_in &in, int64_t items_per_band, int spb, double slots, int waves_per_cu) {
  const FamilyPolicy &f = kPolicy[in.family];
  const bool down = in.family == AA_LAUNCH_F32_DOWN;
  const int64_t max_yb = in.oH / f.rows_per_band > 1 ? in.oH / f.rows_per_band : 1;
  // the test hook, over the model and the knob alike: a band count the kernels are written for, or it is not looked at
  if (const int fy = forced_ybands(); fy >= 1 && fy <= max_yb && fy <= 64) return fy;
  const char *knob = aa_knob("AA_FUSED_YBANDS");  // experiment knob; not used by tests or bench
  if (in.family == AA_LAUNCH_F32_UP && !knob)
    if (const int64_t yb = up_target_waves_bands(in, items_per_band, spb, max_yb)) return (int)yb;
  int64_t ybands = 1;
  double best = 1e30;
  for (int64_t yb = 1; yb <= max_yb && yb <= 64; yb++) {
    const double rounds = (double)items_per_band * yb / slots;
    const double halo = 1.0 + (double)(yb - 1) * in.taps_h / (double)(f.halo_over_out ? in.H + in.oH : in.H);
    const double cost = down ? down_cost(in, waves_per_cu, halo, rounds) : halo / (rounds / ceil(rounds));
    if (cost < best - 1e-9) best = cost, ybands = yb;
  }
  if (down) ybands = down_doubled_bands(in, items_per_band, ybands, slots, max_yb);
  const int64_t v = knob ? atoll(knob) : 0;
  if (v >= 1 && v <= max_yb) ybands = (in.family == AA_LAUNCH_V1 && v > 64) ? 64 : v;  // (v1's plan bounds the grid for 64 bands)
  return (int)ybands;
}

}  // namespace

void aa_launch_shape(const aa_launch_shape_in &in, AAResidentFn ask, void *ctx, const int *t, aa_launch_shape_out *out) {
  // Resident workgroups of s strips per CU for this kernel and this problem's LDS (-1: their rings do not fit a workgroup's LDS; never
  // for s == 1: a strip's ring is at most 16 KiB).  A failed query only costs the heuristic its input: v3 assumes 16 waves, the float
  // families estimate from LDS and wave slots.  v1 asks nothing: blocks per CU from its LDS and waves, at most 8.
  const FamilyPolicy &f = kPolicy[in.family];
  const auto resident = [&](int s) {
    int nb = -1;
    if (in.family == AA_LAUNCH_V1) {
      nb = blocks_by_lds(in.lds, in.threads / 64, 8);
    } else if (!f.by_lds || in.lds * s <= 64 * 1024) {
      nb = ask ? ask(ctx, s) : s <= 8 ? in.occupancy[s] : -1;
      if (nb <= 0) nb = f.by_lds ? blocks_by_lds(in.lds * s, s) : 16 / s;
    }
    return nb == 0 ? 1 : nb;
  };
  // Strips of a band share a workgroup (neighbouring segments share sectors, their stores meet in L2) unless that leaves
  // wave slots of the CU empty: 5 strips -> 4 workgroups = 20 of 24 waves, and 24 single-strip workgroups are 5 % faster;
  // 4 strips fill the CU either way and stay grouped (measured: grouped 0.396 ms vs 0.425 ms for the 906x438 shape).
  int spb = in.strips_per_block;
  const char *up_spb = in.family == AA_LAUNCH_F32_UP ? aa_knob("AA_UP_SPB") : nullptr;  // experiment knob, before the drop (which may undo it)
  if (const int v = up_spb ? atoi(up_spb) : 0; v >= 1 && v <= 8) spb = v;
  int nb = 0;  // resident(spb), once asked (an answer is never 0): every question costs a cache lookup on the launch path
  if (spb > 1 && !in.spb_forced) {
    nb = resident(spb);
    const int nb1 = nb < 0 ? 0 : resident(1);
    if (nb < 0 || nb1 > nb * spb) spb = 1, nb = nb1;
  }
  const char *f32_spb = in.family == AA_LAUNCH_F32_DOWN ? aa_knob("AA_F32_SPB") : nullptr;  // experiment knob, after the drop
  const int v = f32_spb ? atoi(f32_spb) : 0, r = v >= 1 && v <= 8 ? resident(v) : 0;
  if (r > 0) spb = v, nb = r;
  // the test hook (aa_set_launch_shape), after the knobs and kept like a forced plan's: a grouping the kernels are written for (see
  // aa_interp.h for what was read in them), decided by what the plan knows alone, or it is not looked at
  if (const int fs = forced_spb(); fs >= 1 && fs <= 8 && in.family != AA_LAUNCH_V1 && fs <= in.nstrips && in.lds * fs <= 64 * 1024 && fs != spb)
    spb = fs, nb = 0;
  if (!nb) nb = resident(spb);
  const int sgroups = (in.nstrips + spb - 1) / spb;
  *out = aa_launch_shape_out{spb, pick_ybands(in, in.items * sgroups, spb, (double)in.cus * nb, in.saturation ? nb * spb : 0), nb, 0, 0, 0};
  out->groups = in.items * (int64_t)out->ybands;
  const int64_t grid = (f.pad8 ? (out->groups + 7) / 8 * 8 : out->groups) * sgroups;
  out->grid = grid > 0x7FFFFFFF ? 0 : grid;
  // developer builds: one line per launch, in the text tools/experiments and tools/launch_shape_ab.py read
  const int s = in.nstrips <= 8 ? in.nstrips : 4;
  if (in.family == AA_LAUNCH_V3 && aa_knob("AA_V3_DEBUG"))
    fprintf(stderr, "[aa v3] strips %d spb %d (resident(1) %d, resident(%d) %d) ybands %d lds/strip %zu images %lld\n", in.nstrips, spb,
            resident(1), s, resident(s), out->ybands, (size_t)in.lds, (long long)in.items);
  if (in.family == AA_LAUNCH_F32_DOWN && grid == out->grid && t && aa_knob("AA_F32_DEBUG"))
    fprintf(stderr, "f32: NQ=%d G=%d MAXC=%d DT=%d CS=%d nstrips=%d spb=%d resident=%d ybands=%d planes=%lld grid=%lld lds=%zu\n", t[0], t[1], t[2],
            t[3], t[4], in.nstrips, spb, nb, out->ybands, (long long)in.items, (long long)grid, (size_t)in.lds * spb);
  if (in.family == AA_LAUNCH_F32_UP && grid == out->grid && t && aa_knob("AA_UP_DEBUG"))
    fprintf(stderr, "up: U=%d KR=%d CPL=%d nstrips=%d spb=%d resident=%d ybands=%d groups=%lld grid=%lld lds=%zu nt=%d\n", t[0], t[1], t[2],
            in.nstrips, spb, nb, out->ybands, (long long)out->groups, (long long)grid, (size_t)in.lds * spb, t[3]);
}

int aa_set_launch_shape(int spb, int ybands) {
  // (requests no rule honours are all alike: stored as the nearest value of the range the return value can carry)
  const int s = spb < 0 ? 0 : spb > 255 ? 255 : spb, y = ybands < 0 ? 0 : ybands > 0xFFFF ? 0xFFFF : ybands;
  return g_forced_shape.exchange(s | (y << 8), std::memory_order_relaxed);
}

int aa_probe_launch_shape(const aa_launch_shape_in *in, aa_launch_shape_out *out) {
  if (!in || !out) return AA_ERR_NULL;
  // (sizes a tensor can have: the model's products stay inside 64 bits; strip counts the occupancy array answers)
  if (in->family < AA_LAUNCH_V1 || in->family > AA_LAUNCH_F32_UP || in->nstrips < 1 || in->nstrips > (1 << 20) || in->strips_per_block < 1 ||
      in->strips_per_block > 8 || in->items < 1 || in->items > ((int64_t)1 << 40) || in->H < 1 || in->H > 0x7FFFFFFF || in->oH < 1 ||
      in->oH > 0x7FFFFFFF || in->taps_h < 1 || in->taps_w < 1 || in->cus < 1 || in->lds > ((uint64_t)1 << 32) ||
      (in->family == AA_LAUNCH_V1 && (in->threads < 64 || in->threads % 64 != 0 || in->nstrips != 1 || in->strips_per_block != 1)))
    return AA_ERR_BAD_SHAPE;
  aa_launch_shape(*in, nullptr, nullptr, nullptr, out);
  return AA_OK;
}
