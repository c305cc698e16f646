// aa_fused_float.hip — host-side plan of the fused float kernels: fp32 / fp16 / bf16 / fp64 planes and fp32 / fp16 / bf16 channels_last with
// shrinking heights (aa_fused_float_impl.h), fp32 / fp16 / bf16 planes with growing heights, the gather form of the adjoint among them
// (aa_fused_float_up_impl.h).  aa_f32_plan() makes every decision that does not depend on the pointers: the route, the strip geometry and
// all template arguments of the kernel that will run.  aa_f32_launch() adds the few that do and launches through the unit that compiled
// the kernel.  The compiled set is aa_fused_float_list.h.

#include "aa_fused_float_impl.h"

#define F32_UNIT(name, ...) int aa_f32_launch_##name(const F32Plan &, const AAProblem *);
#include "aa_fused_float_list.h"

namespace {

// the list as data (value lists zero-padded)
template <class... T> constexpr int f32_mask(T... dt) { return ((1 << dt) | ...); }
#define F32_ITEMS(...) __VA_ARGS__
const struct { int unit, dts, cs, width[8]; } kSets[] = {
#define F32_SET(unit, dts, cs, ws) {F32_UNIT_##unit, f32_mask dts, cs, {F32_ITEMS ws}},
#include "aa_fused_float_list.h"
};
const struct { int kernel, vert[8], G[8], NDMA[8]; F32Launch launch; } kUnits[] = {  // indexed by F32UnitId
#define F32_UNIT(name, kernel, fast, vert, g, ndma) {F32_##kernel, {F32_ITEMS vert}, {F32_ITEMS g}, {F32_ITEMS ndma}, aa_f32_launch_##name},
#include "aa_fused_float_list.h"
};

// the widths `unit` lists for element type dt at channel stride (or CPL) cs; nullptr: none
const int *widths_of(int unit, int dt, int64_t cs) {
  for (const auto &s : kSets)
    if (s.unit == unit && dt >= 0 && dt < 31 && (s.dts >> dt & 1) && s.cs == cs) return s.width;
  return nullptr;
}
// index of the smallest value of a zero-padded list of 8 that ok() accepts; -1: none
template <class F> int least(const int *v, F ok) {
  int best = -1;
  for (int i = 0; i < 8 && v[i]; i++)
    if (ok(v[i]) && (best < 0 || v[i] < v[best])) best = i;
  return best;
}
// the rest of the kernel, from the unit's lists: the smallest MAXC / KR that holds `rows`, the smallest staging form that holds the
// segment (64 pieces per DMA); false: the unit has no such kernel
bool finish(int unit, int rows, F32Plan *k) {
  const auto &u = kUnits[unit];
  const int v = least(u.vert, [&](int x) { return rows <= x; });
  const int f = least(u.NDMA, [&](int n) { return k->nseg <= 64 * n; });
  if (v < 0 || f < 0) return false;
  k->kernel = u.kernel; k->vert = u.vert[v]; k->G = u.G[f]; k->NDMA = u.NDMA[f]; k->launch = u.launch;
  return k->launch(*k, nullptr) == 1;
}

// Shrinking heights, the vertical pass in scatter form.  Planes: a lane reads its window with NQ aligned reads of EPQ elements
// (EPQ * NQ - (EPQ - 1) taps).  fp32 / fp16 / bf16 channels_last with 3 or 4 channels: a lane per output element, taps read one by one
// (4 * NQ taps, whatever the element size).
bool down_plan(int unit, int dtype, int layout, int64_t N, int64_t C, int64_t H, int64_t W, const aa_axis &ah, const aa_axis &aw, F32Plan *k) {
  const int64_t cs = (layout == AA_NHWC && C > 1) ? C : 1;
  const int *widths = widths_of(unit, dtype, cs);
  const int want_kind = dtype == AA_F64 ? AA_TABLE_F64 : AA_TABLE_F32;
  if (!widths || (layout != AA_NCHW && layout != AA_NHWC) || ah.kind != want_kind || aw.kind != want_kind) return false;
  if (ah.scatter_off <= 0 || ah.scatter_max <= 0 || ah.scatter_max > 6) return false;
  if (H < ah.out_size || aw.span64p1 <= 0 || (cs != 1 && aw.span4p1 <= 0)) return false;
  const int es = dtype == AA_F64 ? 8 : (dtype == AA_F32 ? 4 : 2);
  const int epq = es == 2 ? 4 : 16 / es;  // elements per aligned window read of a plane (see RB in the kernel)
  const int pe = 16 / es;                 // elements per staged 16-byte piece
  const int taps_w = aw.max_taps > 0 ? aw.max_taps : aw.ksize;
  auto taps_of = [&](int nq) { return cs != 1 ? 4 * nq : epq * nq - (epq - 1); };  // taps a window of NQ reads holds
  const int w = least(widths, [&](int nq) { return taps_w <= taps_of(nq); });
  if (w < 0 || W < taps_of(widths[w])) return false;
  const int nq = k->width = widths[w];
  k->DT = dtype;
  k->cs = (int)cs;
  // strips of 64 output elements (whole 128-byte lines per stored fp32 row piece, one line per 16-bit one); 32, then 16 when the segment
  // does not fit two DMAs
  for (k->strip_w = 64;; k->strip_w /= 2) {
    if (cs != 1) {  // the strip's pixels: ceil((strip_w - 1) / C) + 1; the spread of their window starts, bounded through the measured
                    // spread of 4 neighbours (3 steps) and of 64; + the segment start rounded down to 4 elements; in staged pieces of
                    // pe elements (4 floats, 8 halves)
      const int steps = ((k->strip_w - 1) / (int)cs + 1 + 2) / 3;
      const int spread = steps * (aw.span4p1 - 1) < aw.span64p1 - 1 ? steps * (aw.span4p1 - 1) : aw.span64p1 - 1;
      k->nseg = ((spread + 4 * nq) * (int)cs + 3 + (int)cs + pe - 1) / pe + 1;
    } else {  // the spread of the strip's window starts (+EPQ-1: the first one rounded down to the 16-byte grid) + one window
      const int win = (epq - 1) + epq * nq;
      k->nseg = ((k->strip_w == 64 ? aa_strip_span_px(aw, win) : k->strip_w == 32 ? aa_strip_span_px32(aw, win) : aa_strip_span_px16(aw, win)) +
                 pe - 1) / pe;
    }
    if (k->nseg <= 128 || k->strip_w == 16 || aw.span4p1 <= 0) break;
  }
  k->nstrips = (int)((aw.out_size * cs + k->strip_w - 1) / k->strip_w);
  if ((uint64_t)H * W * 8 * cs > 0xFFFFFFF0ull || (uint64_t)ah.out_size * aw.out_size * 8 * cs > 0xFFFFFFF0ull) return false;
  if (!aa_grid_fits(N * C * k->nstrips)) return false;
  static const char *const kNames[2][5] = {{"", "fused_f32_nchw", "fused_f64_nchw", "fused_f16_nchw", "fused_bf16_nchw"},  // [fast][aa_dtype]
                                           {"", "fused_f32_nchw_fast", "", "fused_f16_nchw_fast", "fused_bf16_nchw_fast"}};
  static const char *const kNhwc[5] = {"", "fused_f32_nhwc", "", "fused_f16_nhwc", "fused_bf16_nhwc"};
  k->variant = cs != 1 ? kNhwc[dtype] : kNames[unit == F32_UNIT_fast][dtype];
  return finish(unit, ah.scatter_max, k);
}

// Growing heights (H <= oH), the vertical pass in gather form.  Columns per lane and union width: the widest CPL with a listed U that holds
// the taps and the spread of CPL neighbouring window starts, and whose strip segment has a staging form.
bool up_plan(int dtype, int layout, int64_t N, int64_t C, int64_t H, int64_t W, const aa_axis &ah, const aa_axis &aw, F32Plan *k) {
  if (layout != AA_NCHW || ah.kind != AA_TABLE_F32 || aw.kind != AA_TABLE_F32 || H > ah.out_size) return false;
  const int taps_h = ah.max_taps > 0 ? ah.max_taps : ah.ksize;
  if (taps_h > 6 || ah.gather_off <= 0) return false;  // (a gather record holds 6 weights)
  const int taps_w = aw.max_taps > 0 ? aw.max_taps : aw.ksize;
  if (taps_w > 8 || aw.span64p1 <= 0 || aw.span4p1 <= 0) return false;
  const int es = dtype == AA_F32 ? 4 : 2;
  k->DT = dtype;
  auto take = [&](int cpl) {
    const int *us = widths_of(F32_UNIT_up, dtype, cpl);
    if (!us || (cpl > 1 && aw.out_size < 64 * cpl)) return false;  // (narrow outputs: keep the lanes busy)
    const int spread = cpl == 1 ? 0 : aw.span4p1 - 1;  // (span4p1 - 1 covers 4 neighbours; 2 spread at most as much)
    const int i = least(us, [&](int u) { return taps_w + spread <= u; });
    if (i < 0 || W < us[i]) return false;
    k->cs = cpl;
    k->width = us[i];
    // floats a strip of 64 * cpl outputs covers: cpl * spread of 64 starts + union (+: the segment start rounded down to a 16-byte piece)
    k->nseg = ((cpl * (aw.span64p1 - 1) + cpl + us[i] + (16 / es - 1)) * es + 15) / 16 + 1;
    return finish(F32_UNIT_up, taps_h, k);
  };
  if (!take(4) && !take(2) && !take(1)) return false;
  k->strip_w = 64 * k->cs;
  k->nstrips = (int)((aw.out_size + k->strip_w - 1) / k->strip_w);
  if ((uint64_t)H * W * 4 > 0xFFFFFFF0ull || (uint64_t)ah.out_size * aw.out_size * 4 > 0xFFFFFFF0ull) return false;
  if (!aa_grid_fits(N * C * k->nstrips)) return false;
  k->variant = dtype == AA_F32 ? "fused_f32_nchw_up" : (dtype == AA_F16 ? "fused_f16_nchw_up" : "fused_bf16_nchw_up");
  return true;
}

// Everything the kernel needs that can be known without the pointers (aa_workspace_bytes asks before they exist): the shrinking route
// first, then growing heights.  The tolerance mode takes the tolerance unit's kernel where it has one (planes of fp32 / fp16 / bf16) and
// the exact kernel otherwise: whatever the tolerance rows list, a problem that has an exact plan (aa_workspace_bytes answers 0) has a
// plan in the tolerance mode too.  false: no kernel.
bool f32_plan(int dtype, int layout, int64_t N, int64_t C, int64_t H, int64_t W, const aa_axis &ah, const aa_axis &aw, bool fast, F32Plan *k) {
  *k = F32Plan{};
  if (fast && down_plan(F32_UNIT_fast, dtype, layout, N, C, H, W, ah, aw, k)) return true;
  *k = F32Plan{};
  if (down_plan(F32_UNIT_down, dtype, layout, N, C, H, W, ah, aw, k)) return true;
  *k = F32Plan{};
  if (down_plan(F32_UNIT_nhwc16, dtype, layout, N, C, H, W, ah, aw, k)) return true;  // (16-bit channels_last: a unit of its own)
  *k = F32Plan{};
  return up_plan(dtype, layout, N, C, H, W, ah, aw, k);
}

}  // namespace

bool aa_f32_plan(const AAProblem &q, bool fast, F32Plan *k) {
  if (!f32_plan(q.dtype, q.layout, q.N, q.C, q.H, q.W, q.ah, q.aw, fast, k)) return false;
  // a pitched view: 32-bit offsets inside a plane (image), whole elements apart; growing heights: dense only
  const int es = q.dtype == AA_F64 ? 8 : (q.dtype == AA_F32 ? 4 : 2);
  return !q.in_row_pitch || !(k->kernel == F32_UP || (uint64_t)q.H * (uint64_t)q.in_row_pitch > 0x7FFFFFF0ull || (q.in_row_pitch & (es - 1)) ||
                              (q.in_img_pitch & (es - 1)));
}

int aa_f32_launch(const F32Plan &pl, const AAProblem &q) {
  F32Plan k = pl;
  const int es = q.dtype == AA_F64 ? 8 : (q.dtype == AA_F32 ? 4 : 2);
  if (k.kernel == F32_UP) {
    // the store form (see the kernel's store): streaming for outputs far larger than the caches, or as aa_set_store_form says (tests of
    // the streaming forms at small sizes)
    const unsigned long long plane_out = (unsigned long long)q.oH * q.oW * es;
    k.store_nt = g_aa_store_form < 0 ? (plane_out * (unsigned long long)(q.N * q.C) > (64ull << 20) ? 1 : 0) : (g_aa_store_form ? 1 : 0);
    // rows or planes that are not whole 64-byte sectors: stream only the whole sectors of each piece
    if (es == 4 && k.store_nt && k.cs == 4 && ((((uintptr_t)q.out) | (uint64_t)q.oW * 4u | plane_out) & 63u) != 0 && !aa_knob("AA_UP_NO_SPLIT"))
      k.store_nt = 2;
    // ... and when the rows are 8-byte but not 16-byte aligned (oW = 906): strips of 240 columns cut at the sector boundaries of each row
    // instead, with a 1088-byte staging area per strip.  Measured, [256,3,196,320] gradients -> 438 x W (ms, split + pacing |
    // sector-aligned pieces): W = 898 0.347 | 0.312, 906 0.321 | 0.301-0.311; rows that are 16-byte aligned are better off with the
    // split: 900 0.257 | 0.303, 904 0.269 | 0.284
    if (k.store_nt == 2 && q.oW % 4 == 2 && ((uintptr_t)q.out & 15) == 0 && !aa_knob("AA_UP_NO_ALN")) {
      k.store_nt = 3;
      k.strip_w = 240;
      k.nstrips = (int)((q.oW + 14 + 239) / 240);
      k.lds_extra = 1088;
    }
  }
  return aa_launch_status(k.launch(k, &q));
}
