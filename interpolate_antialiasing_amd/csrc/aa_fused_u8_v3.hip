// aa_fused_u8_v3.hip — host-side dispatcher of the fused uint8 kernel.  aa_v3_plan() makes every decision that does not depend on the
// pointers: the route and all template arguments of the kernel that will run.  aa_v3_launch() adds the few that do and launches through
// the unit that compiled the kernel.  The kernel and its design notes are in aa_fused_u8_v3_impl.h, the compiled set
// in aa_fused_u8_v3_list.h.

#include "aa_fused_u8_v3_impl.h"

#define V3_UNIT(name, route, C, arith, fast) int aa_v3_launch_##name(const V3Kernel &, const FusedU8V3Params *, const AAProblem *, size_t);
#include "aa_fused_u8_v3_list.h"

static const struct {
  int route, C, arith, fast;
  V3Launch launch;
} kV3Units[] = {
#define V3_UNIT(name, route, C, arith, fast) {V3_##route, C, V3_##arith, fast, aa_v3_launch_##name},
#include "aa_fused_u8_v3_list.h"
};

// the unit that compiled k, if it holds k (nullptr: no such kernel)
static V3Launch v3_unit(const V3Kernel &k) {
  for (const auto &u : kV3Units)
    if (u.route == k.route && u.C == k.C && (u.arith & (k.FLT ? V3_FLT : V3_PIL)) && u.fast == (int)k.fast)
      return u.launch(k, nullptr, nullptr, 0) ? u.launch : nullptr;
  return nullptr;
}

// filters whose shrinking heights may take the narrow-window MAXC-6 instantiations (5-6 open output rows with <= 16 taps)
static bool v3_six_narrow_filter(int filter) { return filter == AA_FILTER_LANCZOS || filter == AA_FILTER_HAMMING; }

// Everything the kernel needs that can be known without the pointers (aa_workspace_bytes asks before they exist).  false: no kernel.
bool aa_v3_plan(const AAProblem &q, bool fast, V3Plan *pl) {
  const int64_t N = q.N, Cin = q.C, H = q.H, W = q.W;
  const aa_axis &ah = q.ah, &aw = q.aw;
  const int layout = q.layout, out_f32 = q.out_f32, out_layout = q.out_layout, alpha = q.alpha;
  if (q.dtype != AA_U8) return false;
  // straight alpha: the ALPHA instantiations cover Pillow arithmetic, 4 interleaved channels, uint8 out, narrow windows of shrinking heights
  if (alpha && (out_f32 || layout != AA_NHWC || Cin != 4 || ah.kind != AA_TABLE_PIL || aw.kind != AA_TABLE_PIL || H < ah.out_size)) return false;
  if (out_f32 && (ah.kind != AA_TABLE_F32 || aw.kind != AA_TABLE_F32)) return false;  // float output = float arithmetic
  const bool flt = ah.kind == AA_TABLE_F32 && aw.kind == AA_TABLE_F32;  // the reference harness's uint8 semantics
  if (!flt && (ah.kind != AA_TABLE_PIL || aw.kind != AA_TABLE_PIL)) return false;
  // channels_last with 3 or 4 interleaved channels, or planar bytes: NCHW is N*C single-channel images
  const bool planar = layout == AA_NCHW || Cin == 1;
  const int C = planar ? 1 : (int)Cin;
  if (C != 1 && C != 3 && C != 4) return false;
  // a planar wave holds one channel: it can write its own float plane, not an interleaved pixel
  if (out_f32 && planar && Cin != 1 && out_layout != AA_NCHW) return false;
  const int64_t oH = ah.out_size, oW = aw.out_size;
  const int out_es = q.out_elem == AA_F32 ? 4 : 2;  // bytes per element of a float output (float16 / bfloat16: 2)
  if (out_f32 && (uint64_t)oH * oW * (planar ? 1 : Cin) * out_es > 0xFFFFFFF0ull) return false;
  const bool up = H < oH;  // growing heights: the vertical pass gathers (template parameter UPK of the kernel)
  const int taps_h = ah.max_taps > 0 ? ah.max_taps : ah.ksize;
  const int taps_w = aw.max_taps > 0 ? aw.max_taps : aw.ksize;
  if (up) {  // needs the H table's gather records (6 weights each)
    if (ah.gather_off <= 0 || taps_h > 6) return false;
    // planar bytes store 64-byte pieces per strip and output row: with many strips the generic two-launch path is faster
    // (measured, [128,3,438,906] -> 1200x1200: fused 1.14 ms, generic 0.64 ms; -> 120 columns: fused 0.123, generic 0.148)
    if (planar && oW > 256) return false;
  } else {  // the in-register scatter pass needs the H table's scatter section and at most 4 open output rows
    if (ah.scatter_off <= 0 || ah.scatter_max <= 0 || ah.scatter_max > 6) return false;
    // 5-6 open rows with windows of <= 16 taps: the MAXC-6 narrow instantiations (routes SIX and SIX_ALPHA), which exist for
    // Hamming and Lanczos only.  Bicubic reaches 5 open rows there too and keeps the two-launch path (a follow-up).
    if (ah.scatter_max > 4 && taps_w <= 16 && !v3_six_narrow_filter(ah.filter)) return false;
  }
  const bool six = !up && ah.scatter_max > 4 && taps_w <= 16;  // the narrow MAXC-6 route
  int tw = round_tw(taps_w);
  if ((flt || six) && tw != 0 && tw < 6) tw = 6;  // float arithmetic and six open rows are instantiated for 6 .. 16 taps
  // windows of 17 .. 34 taps: Pillow arithmetic, shrinking heights.  (With growing heights — test.py's (120, 1200) — the gather form with
  // such windows was built and measured SLOWER than the two-launch path: bicubic channels_last 0.226 vs 0.205 ms per 128 images.)
  if (tw > 16 && up) return false;
  // windows of 35 .. 136 taps (down-scaling by 17 .. 68 bilinear, 9 .. 34 bicubic): SPLIT windows — four lanes share an output pixel, each
  // holds a quarter of its window (tw = taps per lane: 16 / 24 / 34) and the partial sums meet in two DPP additions; Pillow arithmetic
  // (integer sums are associative: bit-exact), shrinking heights, uint8 out; strips of 16 columns
  const bool split = tw == 0 && taps_w <= 136 && !flt && !up && !out_f32;
  if (split) tw = taps_w <= 64 ? 16 : (taps_w <= 96 ? 24 : 34);
  if (tw == 0 || W < (split ? 4 * tw : tw)) return false;
  if ((uint64_t)H * W * C > 0x7FFFFFF0ull || (uint64_t)oH * oW * C > 0xFFFFFFF0ull) return false;
  // segment: bytes covered by the strip's windows in one input row (+ alignment slack)
  int span_px = split ? aa_strip_span_px16(aw, 4 * tw) : aa_strip_span_px(aw, tw);
  if (span_px < 0) return false;
  int nseg = (span_px * C + 3 + 15 + 15) / 16;
  int cap = split ? 16 : 64;  // output columns per strip
  bool v1_first = false;
  if (up && nseg > 64) {
    // the gather form is instantiated with one staging DMA per row (64 pieces): strong down-scaling in W (test.py's 906 -> 120
    // with growing heights) gets strips of 32 columns — half the lanes idle, but such a shape is bound by its input stream
    span_px = aa_strip_span_px32(aw, tw);
    if (span_px < 0) return false;
    nseg = (span_px * C + 3 + 15 + 15) / 16;
    cap = 32;
    if (nseg > 64) return false;
    // ... but the first-generation kernel (Pillow arithmetic, channels_last, uint8 out) runs when it takes the shape: its block-wide
    // tiles handle these wide windows better (measured, [128,3,438,906] -> 1200 x 120: 0.060 ms against 0.095 ms here)
    v1_first = !flt && !planar && !out_f32;
  }
  if (nseg > 128 || (size_t)8 * nseg * 16 > 64 * 1024) return false;  // (8 staged rows per wave: the kernel's G)
  if (six && nseg > 64) return false;  // (the narrow MAXC-6 route has the one-DMA-per-row form only)
  if (alpha && (split || tw > 16 || nseg > 64)) return false;  // (the ALPHA routes: one DMA per row)
  const int64_t nstrips = (oW + cap - 1) / cap + 1;  // (balanced strips can be one more)
  if (!aa_grid_fits((planar ? N * Cin : N) * nstrips)) return false;
  // a pitched view (cropped / batch-sliced tensor): rows q.in_row_pitch bytes apart, images (planes) q.in_img_pitch bytes apart; 32-bit
  // offsets inside an image, and growing heights take dense tensors only
  if (q.in_row_pitch && ((uint64_t)H * (uint64_t)q.in_row_pitch > 0x7FFFFFF0ull || up)) return false;
  pl->row_pitch = q.in_row_pitch ? (unsigned)q.in_row_pitch : (unsigned)(W * C);
  pl->img_in_bytes = q.in_img_pitch ? (unsigned long long)q.in_img_pitch : (unsigned long long)H * W * C;
  pl->img_out_bytes = (unsigned long long)oH * oW * C * (out_f32 ? out_es : 1);

  // the kernel
  const int sm = ah.scatter_max;
  V3Kernel &k = pl->k;
  k = V3Kernel{};
  k.route = alpha ? (six ? V3_SIX_ALPHA : V3_ALPHA) : six ? V3_SIX : split ? V3_SPLIT : up ? V3_UP : tw > 16 ? V3_WIDE : V3_NARROW;
  k.C = C;
  k.TW = tw;
  // accumulator sets for the open output rows (the ALPHA route has sets for 2 and 4); growing heights gather instead
  k.MAXC = up ? 1 : sm <= 2 ? 2 : (sm == 3 && !alpha) ? 3 : sm <= 4 ? 4 : 6;
  k.SP = split ? 4 : 1;
  k.ALPHA = alpha != 0;
  k.FLT = flt;
  // the tolerance mode of the float-arithmetic kernels (AA_FLAG_FAST) exists for narrow windows of shrinking heights; six open rows,
  // wide windows and growing heights run exact in either precision mode
  k.fast = flt && fast && k.route == V3_NARROW;
  // non-negative weights need no clamp of the intermediate; the six-row kernels and float arithmetic have no such form, and growing
  // heights have it with the ring of 2 rows only (triangle / box filters: taps_h <= 2; every other gather keeps a ring of 6)
  k.NONNEG = !flt && !six && aa_filters_nonneg(aw.filter, ah.filter) && (!up || taps_h <= 2);
  k.UPK = !up ? 0 : (taps_h <= 2 && (flt || k.NONNEG)) ? 2 : 6;
  k.TWO_DMA = nseg > 64;  // wide segments (large down-scales): the generic-address form
  if (out_f32 && q.out_elem != AA_F32 && !v3_route_has_out16(k.route)) return false;
  k.launch = v3_unit(k);
  if (!k.launch) return false;

  // Plane groups (template parameter PL of the kernel): planar bytes, either arithmetic, shrinking heights — one wave filters the same strip
  // and band of THREE CONSECUTIVE PLANES of the tensor (the channels of an RGB image; three grayscale images; planes of neighbouring
  // images when C is 2, 4, 5, ...: planes are independent and uniformly spaced), sharing each row's staging DMA and fixed work.  The
  // single-plane form keeps: growing heights; windows beyond 12 taps (8 in float arithmetic: the wider instantiations need 133-147 VGPRs
  // = 3 waves per SIMD; the route's TW lists); segments beyond 16 pieces (down-scaling by 4 and more: the single planes' staging DMAs are
  // full enough as they are, measured +4 % at 1024 -> 224).
  pl->groups = k;
  pl->groups.route = V3_PLANES;
  pl->groups.C = pl->groups.PL = 3;
  // ... when three planes' offsets stay within 32 bits, and aa_set_plane_groups has not turned them off
  const bool groups = planar && N * Cin >= 2 && k.route == V3_NARROW && nseg <= 16 && 3 * pl->img_in_bytes <= 0x7FFFFFF0ull &&
                      3 * pl->img_out_bytes <= 0x7FFFFFF0ull && g_aa_plane_groups != 0;
  pl->groups.launch = groups ? v3_unit(pl->groups) : nullptr;
  // PERIODIC (single planes): the 8 ring slots' row phases repeat when 8 rows span whole 16-byte pieces, in the routes that list that form
  k.PERIODIC = (8ull * pl->row_pitch) % 16 == 0;
  if (!k.launch(k, nullptr, nullptr, 0)) k.PERIODIC = false;

  pl->planar = planar;
  pl->C = C;
  pl->cap = cap;
  pl->nseg = nseg;
  pl->v1_first = v1_first;
#define V3_FAST(s) (k.fast ? s "_fast" : s)
#define V3_TO(a, b) (q.out_elem == AA_F16 ? V3_FAST(a "f16" b) : q.out_elem == AA_BF16 ? V3_FAST(a "bf16" b) : V3_FAST(a "f32" b))
  pl->variant = alpha    ? (six ? "fused_u8_nhwc_pil_alpha6_v3" : "fused_u8_nhwc_pil_alpha_v3")
                : !flt   ? (planar ? "fused_u8_planar_pil_v3" : "fused_u8_nhwc_pil_v3")
                : !out_f32 ? (planar ? V3_FAST("fused_u8_planar_harness_v3") : V3_FAST("fused_u8_nhwc_harness_v3"))
                : planar ? V3_TO("fused_u8_planar_to_", "_v3")
                : out_layout == AA_NCHW ? V3_TO("fused_u8_nhwc_to_", "_nchw_v3") : V3_TO("fused_u8_nhwc_to_", "_nhwc_v3");
#undef V3_TO
#undef V3_FAST
  return true;
}

int aa_v3_launch(const V3Plan &pl, const AAProblem &q) {
  const int C = pl.C;
  const int64_t NI = pl.planar ? q.N * q.C : q.N;  // images the kernel sees

  FusedU8V3Params p;
  p.H = (int)q.H; p.W = (int)q.W; p.oH = (int)q.oH; p.oW = (int)q.oW;
  p.ksize_w = q.aw.ksize; p.ksize_h = q.ah.ksize;
  p.row_pitch = pl.row_pitch;
  p.img_in_bytes = pl.img_in_bytes;
  p.img_out_bytes = pl.img_out_bytes;
  p.outm = q.out_f32 ? (pl.planar || q.out_layout == AA_NCHW ? 1 : 2) : 0;
  p.normalize = q.out_f32 ? q.normalize : 0;
  p.out16 = !q.out_f32 ? 0 : q.out_elem == AA_F16 ? 1 : q.out_elem == AA_BF16 ? 2 : 0;
  p.cin = (int)q.C;
  p.fast = pl.k.fast ? 1 : 0;
  for (int c = 0; c < 4; c++) { p.mean[c] = q.mean[c]; p.std[c] = q.std[c]; }

  // ---- the choices that depend on the pointers
  // byte stores: output rows that are not whole dwords, an output that is not dword aligned, or split windows (a quad's first lane stores
  // its pixel's bytes)
  p.byte_store = (pl.k.route == V3_SPLIT || (!q.out_f32 && ((q.oW * C) % 4 != 0 || (C == 3 && q.oW % 4 != 0) || ((uintptr_t)q.out & 3) != 0))) ? 1 : 0;
  if (q.out_f32 && ((uintptr_t)q.out & (p.out16 ? 1 : 3)) != 0) return AA_ERR_BAD_SHAPE;  // a float tensor that is not element aligned
  // 16-bit floats leave in pairs (dword stores) when the output and every row of it start on dword boundaries: even oW — then every
  // strip is an even number of columns wide too — or interleaved C = 4, whose pixels are 8 bytes
  p.pair_store = (p.out16 && ((uintptr_t)q.out & 3) == 0 && (q.oW % 2 == 0 || (C == 4 && p.outm == 2))) ? 1 : 0;
  p.in_mis = (int)((uintptr_t)q.in & 15);
  // ----

  p.total_in_bytes = q.in_row_pitch ? p.img_in_bytes * (unsigned long long)(NI - 1) + (unsigned long long)(q.H - 1) * p.row_pitch + (unsigned long long)q.W * C + p.in_mis
                                    : p.img_in_bytes * (unsigned long long)NI + (unsigned long long)p.in_mis;
  p.total_out_bytes = p.img_out_bytes * (unsigned long long)NI;
  p.n_images = NI;
  p.sc_off = q.ah.scatter_off;
  p.gather_off = q.ah.gather_off;
  p.nstrips = (int)((q.oW + pl.cap - 1) / pl.cap);
  p.strip_w = (int)(((q.oW + p.nstrips - 1) / p.nstrips + 3) & ~3);  // balanced strips (196 -> 4 x 52, not 3 x 64 + 4)
  p.nstrips = (int)((q.oW + p.strip_w - 1) / p.strip_w);
  // all strips of a band in one workgroup when they fit (<= 8 waves); wider images: groups of 4 strips
  p.strips_per_block = p.nstrips <= 8 ? p.nstrips : 4;
  p.spb_forced = 0;
  if (const char *e = aa_knob("AA_V3_SPB")) {  // experiment knob
    const int v = atoi(e);
    if (v >= 1 && v <= 8) { p.strips_per_block = v; p.spb_forced = 1; }
  }
  p.nseg = pl.nseg;
  p.seg_bytes = p.nseg * 16;
  p.ybands = 1;
  p.plane_in_bytes = p.plane_out_bytes = 0;
  p.pl_planes = 0;

  if (pl.groups.launch) {  // if the plane-group launch declines, the single-plane form runs
    FusedU8V3Params pg = p;
    pg.plane_in_bytes = p.img_in_bytes;  // (the single-plane form's "images" are the planes)
    pg.plane_out_bytes = p.img_out_bytes;
    pg.img_in_bytes = 3 * p.img_in_bytes;
    pg.img_out_bytes = 3 * p.img_out_bytes;
    pg.n_images = (NI + 2) / 3;  // groups of three consecutive planes (the last one may hold one or two)
    pg.pl_planes = NI;
    const int rc = pl.groups.launch(pl.groups, &pg, &q, (size_t)8 * 1024);  // (a 1-KiB stage slot per row: the kernel's fixed layout)
    if (rc != 0) return aa_launch_status(rc);
  }
  return aa_launch_status(pl.k.launch(pl.k, &p, &q, (size_t)8 * p.seg_bytes));
}
