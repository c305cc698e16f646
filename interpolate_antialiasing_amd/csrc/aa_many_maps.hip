// aa_many_maps.hip — Pillow's resize of its three wide single-band modes for a ragged batch: "I;16" (uint16), "I" (int32) and "F"
// (float32) maps, each with its own box, its own size, a place on the canvas and a flip, into one dense batch.  This is neither the
// uint8 fixed-point arithmetic of aa_many.hip nor the reference's fp32 passes: the coefficients stay the doubles precompute_coeffs
// leaves (no normalize_coeffs_8bpc), every output of every pass is one double sum over its window in ascending order,
//   ss = 0.0;  ss = ss + (double)in[xmin + x] * k[x]   for x = 0, 1, ...     (product rounded, then sum rounded: no fused multiply-add)
// and the mode's store rule is applied after EACH pass, so the vertical pass reads what the horizontal one stored.  Three launches
// whatever N:
//   1. maps_tables  one thread per (item, axis, covered output index) of the passes that run: aa_pil_coeffs.h's window, the filter in
//                   double, the normalising division, zero padding to ksize;
//   2. maps_hpass   one workgroup per (item, 16 hull rows, strip of 64 output columns) of the items whose horizontal pass runs, found
//                   from prefix sums; the strip's weights staged in LDS, one output per lane and row into the intermediate, in the
//                   item's own element type;
//   3. maps_vpass   one workgroup per (item, canvas row, 256 canvas columns): every element of the canvas is written — the column sum
//                   of the intermediate (or of the source itself, for an item whose horizontal pass Pillow skips), the element copied
//                   for an item whose vertical pass Pillow skips, the fill where the item is not — mirrored for an item that flips.
// Pillow skips a pass whose axis keeps its size under a box that spans it, and copies when the box is the output's size at an integer
// offset; a skipped pass is never run as an identity filter (Lanczos at scale 1 has non-zero off-centre taps).  The planner decides that
// per item on the host with the table kernel's own window arithmetic, so nothing comes back from the device.
// Built with -ffp-contract=off like every user of aa_pil_coeffs.h; the accumulation must stay a multiply and an add.
// Shared with the other ragged calls: aa_many_dev.h (the item of a work unit, the table view and hull clamp), aa_many_host.h (checks, scale).

#include <math.h>
#include <string.h>

#include "aa_many_dev.h"
#include "aa_many_host.h"
#include "aa_many_maps.h"
#include "aa_pil_coeffs.h"

using namespace aa_coeffs;

namespace {

// ---- 1. tables ---------------------------------------------------------------------------------------------------------------------------
// Every item has oH + oW threads, as in many_tables; an axis uses its m <= o covered indices if its pass runs, the other threads idle.
__global__ void __launch_bounds__(256) maps_tables(const AAMapsItem *items, char *ws, int64_t n, int oH, int oW, int filter) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int per = oH + oW;
  if (t >= n * per) return;
  const AAMapsItem &it = items[t / per];
  const int r = (int)(t % per);
  const bool vert = r < oH;
  const int i = vert ? r : r - oH;
  if (!(it.flags & (vert ? AA_MAPS_ITEM_VPASS : AA_MAPS_ITEM_HPASS))) return;
  const int m = vert ? it.mh : it.mw;
  if (i >= m || it.mh <= 0 || it.mw <= 0) return;
  const int ksize = vert ? it.ksize_h : it.ksize_w;
  const int origin = vert ? it.oy : it.ox;
  char *tab = ws + (vert ? it.tab_h : it.tab_w);
  int32_t *xmin_p = (int32_t *)tab;
  int32_t *xsize_p = xmin_p + m;
  double *kk = (double *)(tab + aa_maps_table_w_off(m)) + (size_t)i * ksize;
  const PilWindow wd = pil_window_at((vert ? it.v0h : it.v0w) + i, filter, vert ? it.scale_h : it.scale_w, vert ? it.in0_h : it.in0_w, 0,
                                     vert ? it.in_h : it.in_w);
  const int xs = wd.xsize < ksize ? (wd.xsize < 0 ? 0 : wd.xsize) : ksize;
  xmin_p[i] = wd.xmin - origin;
  xsize_p[i] = xs;
  // precompute_coeffs: the weights and their sum in one sweep, the division in a second
  double ww = 0.0;
  for (int x = 0; x < xs; x++) {
    const double w = apply_filter<double>(filter, ((double)(x + wd.xmin) - wd.center + 0.5) * wd.ss);
    kk[x] = w;
    ww += w;
  }
  for (int x = 0; x < xs; x++)
    if (ww != 0.0) kk[x] /= ww;
  for (int x = xs; x < ksize; x++) kk[x] = 0.0;
}

// ---- the store rules -----------------------------------------------------------------------------------------------------------------------
__device__ inline int round_up(double f) { return (int)(f >= 0.0 ? f + 0.5 : f - 0.5); }  // Pillow's ROUND_UP
__device__ inline int clip8i(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

template <typename T> __device__ inline T store_rule(double ss, int clamp);
template <> __device__ inline float store_rule<float>(double ss, int) { return (float)ss; }
template <> __device__ inline int32_t store_rule<int32_t>(double ss, int) { return round_up(ss); }
// "I;16": the two bytes are clipped apart, which is no clamp: a negative r gives 0, r > 65535 gives 0xFF00 | (r & 255)
template <> __device__ inline uint16_t store_rule<uint16_t>(double ss, int clamp) {
  const int r = round_up(ss);
  if (clamp) return (uint16_t)(r < 0 ? 0 : (r > 65535 ? 65535 : r));
  return (uint16_t)(clip8i(r % 256) | (clip8i(r >> 8) << 8));
}

// An item's pointer comes out of the descriptor, so the compiler takes it for a generic one and loads through it with flat
// instructions.  The maps and the workspace are global memory: the vertical pass says so, and its loads are global ones.
using gbytes = const __attribute__((address_space(1))) uint8_t *;
__device__ inline gbytes as_global(const void *p) { return (gbytes)p; }
template <typename T> __device__ inline T load_at(const uint8_t *p) { return *(const T *)p; }
template <typename T> __device__ inline T load_at(gbytes p) { return *(const __attribute__((address_space(1))) T *)p; }

// One window's taps added to ss: `taps` elements `pitch` bytes apart from p, by the weights k[0..taps), in ascending order, each one
// multiply and one add.  Four taps at a time, so that their loads and products are in flight together; the adds stay a chain in order.
template <typename T, typename P>
__device__ inline double window_sum(P p, int64_t pitch, const double *k, int taps, double ss = 0.0) {
  int x = 0;
  for (; x + 4 <= taps; x += 4) {
    const double v0 = (double)load_at<T>(p + x * pitch), v1 = (double)load_at<T>(p + (x + 1) * pitch);
    const double v2 = (double)load_at<T>(p + (x + 2) * pitch), v3 = (double)load_at<T>(p + (x + 3) * pitch);
    const double p0 = v0 * k[x], p1 = v1 * k[x + 1], p2 = v2 * k[x + 2], p3 = v3 * k[x + 3];
    ss = ss + p0;
    ss = ss + p1;
    ss = ss + p2;
    ss = ss + p3;
  }
  for (; x < taps; x++) {
    const double prod = (double)load_at<T>(p + x * pitch) * k[x];
    ss = ss + prod;
  }
  return ss;
}

// ---- 2. horizontal pass ------------------------------------------------------------------------------------------------------------------
// A workgroup of four waves owns AA_MAPS_HROWS hull rows of one strip of 64 output columns: lane j of every wave is column x0 + j, wave w
// takes rows w, w + 4, w + 8, w + 12 of the group.  The strip's weights are staged into LDS once per workgroup, kHTaps taps of every
// column at a time (rows of the table are contiguous: consecutive lanes load consecutive doubles; a row of the LDS image is one double
// longer, so that the 64 columns of one tap lie in distinct banks), and every lane walks its window in ascending order through the
// chunks.  The elements come through LDS too: for each of its rows in turn a wave stages what the strip's windows read of that row for
// the chunk's taps — one contiguous piece, loaded once with consecutive lanes on consecutive elements, at the element's own alignment —
// into its kHSegBytes of LDS, and the lanes gather from there; a strip whose piece is longer than the buffer reads memory directly.
// Every sum still sees its own taps in order, one multiply and one add each.  Measured on the --maps workload: lanes a
// scale apart reading the row straight from memory, 497 us bilinear / 936 us bicubic; staged, 464 / 656 us.  The tap loop unrolled by
// four (as window_sum does for the vertical pass, which it helps) measured slower here, 508 / 740 us, and is not used.
constexpr int kHWaves = 4, kHPer = AA_MAPS_HROWS / kHWaves, kHTaps = 32, kHSegBytes = 8192;
static_assert(AA_MAPS_HROWS % kHWaves == 0, "every wave takes the same number of rows");

__device__ inline void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

template <typename T>
__global__ void __launch_bounds__(AA_MANY_STRIP * kHWaves) maps_hpass(const AAMapsItem *items, const int64_t *prefix, char *ws, int n, int clamp) {
  __shared__ double wl[AA_MANY_STRIP][kHTaps + 1];
  __shared__ __attribute__((aligned(16))) uint8_t segs[kHWaves][kHSegBytes];
  constexpr int kSegElems = kHSegBytes / (int)sizeof(T);
  const int64_t unit = blockIdx.x;
  const int lo = aa_unit_item(prefix, n, unit);
  const AAMapsItem &it = items[lo];
  if (!(it.flags & AA_MAPS_ITEM_HPASS)) return;  // (never: such an item has no unit; uniform per workgroup)
  const int64_t u = unit - prefix[lo];
  const int mw = it.mw, hull_h = it.hull_h;
  const int nstrips = (mw + AA_MANY_STRIP - 1) / AA_MANY_STRIP;
  const int x0 = (int)(u % nstrips) * AA_MANY_STRIP;
  const int row0 = (int)(u / nstrips) * AA_MAPS_HROWS;
  const int lane = (int)threadIdx.x & (AA_MANY_STRIP - 1), wave = (int)threadIdx.x / AA_MANY_STRIP;
  T *seg = (T *)segs[wave];
  const int x = x0 + lane;
  const AATab<double> tab = aa_tab<double>(ws + it.tab_w, mw, it.ksize_w);
  const int ksize = tab.ksize;
  int mx = 0, ms = 0;
  if (x < mw) {
    mx = tab.xmin[x];
    ms = tab.taps(x);
    aa_clamp_to_hull(mx, ms, it.hull_w);  // (the second clamp never: the hull is the union of these windows)
  }
  // the strip's first and last window starts (starts do not decrease with the output index): what the strip reads of a row for the taps
  // [c0, c0 + kHTaps) is [first + c0, last + c0 + kHTaps), clipped to the hull
  const int xl = x0 + AA_MANY_STRIP - 1 < mw ? x0 + AA_MANY_STRIP - 1 : mw - 1;
  int mxf = tab.xmin[x0], mxl = tab.xmin[xl];
  if (mxf < 0) mxf = 0;
  if (mxl < 0) mxl = 0;
  double ss[kHPer];
#pragma unroll
  for (int j = 0; j < kHPer; j++) ss[j] = 0.0;
  for (int c0 = 0; c0 < ksize; c0 += kHTaps) {  // (ksize is the item's: uniform per workgroup, so every lane meets every barrier)
    __syncthreads();  // (the previous chunk has been consumed)
    for (int idx = (int)threadIdx.x; idx < AA_MANY_STRIP * kHTaps; idx += AA_MANY_STRIP * kHWaves) {
      const int xx = idx / kHTaps, k = idx % kHTaps;
      wl[xx][k] = (x0 + xx < mw && c0 + k < ksize) ? tab.w[(size_t)(x0 + xx) * ksize + c0 + k] : 0.0;
    }
    __syncthreads();
    const int s0 = mxf + c0;
    const int s1 = mxl + c0 + kHTaps < it.hull_w ? mxl + c0 + kHTaps : it.hull_w;
    const int span = s1 - s0;                 // (<= 0: no window of the strip has a tap in this chunk)
    const bool staged = span <= kSegElems;    // (uniform per workgroup)
    const int k_hi = ms - c0 < kHTaps ? ms - c0 : kHTaps;
#pragma unroll
    for (int j = 0; j < kHPer; j++) {
      const int row = row0 + wave + kHWaves * j;
      const bool rowok = row < hull_h;  // (uniform per wave)
      const uint8_t *rp = it.src + (int64_t)(it.oy + (rowok ? row : 0)) * it.row_stride + (int64_t)it.ox * (int64_t)sizeof(T);
      if (staged) {
        // (the buffer is the wave's own, and a wave's LDS accesses execute in program order: what orders the row before, this row's
        // stores and its gathers is a fence the compiler must not move them across, not a workgroup barrier the other waves wait at)
        wave_lds_fence();
        if (rowok)
          for (int i = lane; i < span; i += AA_MANY_STRIP) seg[i] = *(const T *)(rp + (int64_t)(s0 + i) * (int64_t)sizeof(T));
        wave_lds_fence();
        if (rowok && x < mw) {
          const T *sp = seg + (mx + c0 - s0);  // (mxf <= mx <= mxl, and mx + c0 + k < mx + ms <= hull_w: inside [0, span))
          for (int k = 0; k < k_hi; k++) {
            const double prod = (double)sp[k] * wl[lane][k];
            ss[j] = ss[j] + prod;
          }
        }
      } else if (rowok && x < mw) {  // a strip wider than the staging buffer (a scale beyond about 30): the elements straight from memory
        const uint8_t *ep = rp + (int64_t)(mx + c0) * (int64_t)sizeof(T);
        for (int k = 0; k < k_hi; k++) {
          const double prod = (double)*(const T *)(ep + (int64_t)k * (int64_t)sizeof(T)) * wl[lane][k];
          ss[j] = ss[j] + prod;
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < kHPer; j++) {
    const int row = row0 + wave + kHWaves * j;
    if (row < hull_h && x < mw) ((T *)(ws + it.inter))[(int64_t)row * mw + x] = store_rule<T>(ss[j], clamp);
  }
}

// ---- 3. vertical pass --------------------------------------------------------------------------------------------------------------------
// Lane j owns canvas column X = strip * 256 + j of row y: consecutive lanes store consecutive elements.  An item that flips shows column
// oW - 1 - X there.  The row's window is wave-uniform: its weights come through scalar loads.
template <typename T>
__global__ void __launch_bounds__(AA_MAPS_VCOLS) maps_vpass(const AAMapsItem *items, const char *ws, T *out, int oH, int oW, int nstrips, uint32_t fill,
                                                            int clamp) {
  int64_t u = blockIdx.x;
  const int strip = (int)(u % nstrips);
  u /= nstrips;
  const int y = (int)(u % oH);
  const int64_t item = u / oH;
  const AAMapsItem &it = items[item];
  const int X = strip * AA_MAPS_VCOLS + (int)threadIdx.x;
  if (X >= oW) return;
  T v;
  __builtin_memcpy(&v, &fill, sizeof(T));
  const int ty = y - it.dy;
  const int x = ((it.flags & AA_MAPS_ITEM_FLIP) ? oW - 1 - X : X) - it.dx;
  if (ty >= 0 && ty < it.mh && x >= 0 && x < it.mw) {
    // what this pass reads: the intermediate (row r the result of source row oy + r), or the source from (oy, ox) itself
    const bool hp = (it.flags & AA_MAPS_ITEM_HPASS) != 0;
    const int64_t pitch = hp ? (int64_t)it.mw * (int64_t)sizeof(T) : it.row_stride;
    const gbytes base = hp ? as_global(ws) + it.inter + (int64_t)x * (int64_t)sizeof(T)
                           : as_global(it.src) + (int64_t)it.oy * it.row_stride + (int64_t)(it.ox + x) * (int64_t)sizeof(T);
    if (it.flags & AA_MAPS_ITEM_VPASS) {
      const AATab<double> tab = aa_tab<double>(ws + it.tab_h, it.mh, it.ksize_h);
      int r0 = tab.xmin[ty], nr = tab.taps(ty);
      aa_clamp_to_hull(r0, nr, it.hull_h);  // (the second clamp never: the hull is the union of these windows)
      v = store_rule<T>(window_sum<T>(base + (int64_t)r0 * pitch, pitch, tab.row(ty), nr), clamp);
    } else {  // Pillow's copy of this axis: hull row ty is result row v0h + ty
      v = load_at<T>(base + (int64_t)ty * pitch);
    }
  }
  out[(item * oH + y) * (int64_t)oW + X] = v;
}

}  // namespace

// ---- host: the planner -------------------------------------------------------------------------------------------------------------------
size_t aa_maps_desc_size(int64_t n) { return aa_desc_size(sizeof(AAMapsHeader), sizeof(AAMapsItem), n); }

// One axis of one item.  run: the hull [o, o + hull) of the windows of results [v0, v0 + m) (the first window's start and the last one's
// end, each clipped to the axis: boxmath.axis_hull, with the window the table kernel evaluates) and Pillow's ksize.  Not run: the m
// source indices the results copy.
static int maps_axis(bool run, int filter, int64_t in_size, double in0, double scale, int64_t v0, int64_t m, int32_t *o, int32_t *hull, int32_t *ksize) {
  if (!run) {
    *o = (int32_t)((int64_t)in0 + v0);
    *hull = (int32_t)m;
    *ksize = 0;
    return *o + m <= in_size ? AA_OK : AA_ERR_BAD_SHAPE;
  }
  const PilWindow first = pil_window_at((int)v0, filter, scale, in0, 0, (int)in_size);
  const PilWindow last = pil_window_at((int)(v0 + m - 1), filter, scale, in0, 0, (int)in_size);
  const int64_t e = (int64_t)last.xmin + last.xsize;
  if (e <= first.xmin) return AA_ERR_BAD_SHAPE;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double k = ceil(aa_filter_info(filter).support * filterscale) * 2.0 + 1.0;  // precompute_coeffs: (int)ceil(support) * 2 + 1
  if (k > (double)AA_MAX_KSIZE) return AA_ERR_KSIZE;
  *o = first.xmin;
  *hull = (int32_t)(e - first.xmin);
  *ksize = (int32_t)k;
  return AA_OK;
}

int aa_maps_plan_host(int filter, int elem, int64_t n, int64_t oH, int64_t oW, const aa_many_image *images, const aa_many_place *places,
                      double fill, int overflow, void *desc_host, size_t desc_bytes, size_t *workspace_bytes) {
  if (!aa_filter_valid(filter)) return AA_ERR_BAD_FILTER;
  if (elem != AA_MAPS_U16 && elem != AA_MAPS_I32 && elem != AA_MAPS_F32) return AA_ERR_BAD_DTYPE;
  if (overflow != AA_MAPS_OVERFLOW_PILLOW && overflow != AA_MAPS_OVERFLOW_CLAMP) return AA_ERR_BAD_SHAPE;
  const int rc0 = aa_many_check_canvas(n, kAAManyMax, true, oH, oW, desc_host, workspace_bytes, images, places);
  if (rc0 != AA_OK) return rc0;
  // the fill as the element holds it: an integer of the type's range, or a finite float, written as (float)fill
  uint32_t fill_bits = 0;
  if (elem == AA_MAPS_F32) {
    const float f = (float)fill;
    if (!(fill - fill == 0.0) || !(f - f == 0.0f)) return AA_ERR_BAD_SHAPE;
    memcpy(&fill_bits, &f, 4);
  } else {
    const double lo = elem == AA_MAPS_U16 ? 0.0 : -2147483648.0, hi = elem == AA_MAPS_U16 ? 65535.0 : 2147483647.0;
    if (!(fill >= lo && fill <= hi) || fill != floor(fill)) return AA_ERR_BAD_SHAPE;
    fill_bits = (uint32_t)(int64_t)fill;
  }
  if (desc_bytes < aa_maps_desc_size(n)) return AA_ERR_WORKSPACE;
  const int64_t EB = aa_maps_elem_bytes(elem);
  const int64_t vstrips = (oW + AA_MAPS_VCOLS - 1) / AA_MAPS_VCOLS;
  if (n * oH * vstrips > INT32_MAX || n * (oH + oW) > (int64_t)INT32_MAX * 256) return AA_ERR_BAD_SHAPE;  // (grids of the launches)

  AAMapsHeader *hd = (AAMapsHeader *)desc_host;
  AAMapsItem *items = (AAMapsItem *)(hd + 1);
  int64_t *prefix = (int64_t *)(items + n);
  size_t off = 0;  // the arena first, then the intermediates
  int64_t units = 0;
  const aa_many_place whole = {oH, oW, 0, 0};
  for (int64_t i = 0; i < n; i++) {
    const aa_many_image &im = images[i];
    AAMapsItem it;
    memset(&it, 0, sizeof(it));
    AAManyBox bx;
    int rc = aa_many_check_image_box(im, (im.flags & ~AA_MANY_FLIP_X) == 0, AA_NCHW, 1, EB, EB, &bx);
    if (rc != AA_OK) return rc;
    const AAManyPlace pl = aa_many_cover(places ? places[i] : whole, oH, oW);
    const double W = (double)im.W, H = (double)im.H;
    // Pillow's three ways: a copy (the box is the size asked for, at an integer offset: boxmath.is_plain_crop; no box: the image's own
    // size), else per axis a pass only if the size changes or the box does not span the axis (boxmath.axis_is_full)
    const bool crop = bx.x0 == floor(bx.x0) && bx.y0 == floor(bx.y0) && bx.x1 - bx.x0 == (double)pl.vw && bx.y1 - bx.y0 == (double)pl.vh;
    const bool hrun = !crop && (pl.vw != im.W || bx.x0 != 0.0 || bx.x1 != W);
    const bool vrun = !crop && (pl.vh != im.H || bx.y0 != 0.0 || bx.y1 != H);
    it.src = (const uint8_t *)im.data_dev;
    it.row_stride = im.H > 1 ? im.stride_row : 0;
    it.in_h = (int32_t)im.H; it.in_w = (int32_t)im.W;
    it.in0_h = bx.y0; it.in0_w = bx.x0;
    it.scale_h = aa_pil_scale(bx.on, bx.y0, bx.y1, H, pl.vh);
    it.scale_w = aa_pil_scale(bx.on, bx.x0, bx.x1, W, pl.vw);
    it.vh = pl.vh; it.vw = pl.vw; it.v0h = pl.v0h; it.v0w = pl.v0w;
    it.mh = pl.mh; it.mw = pl.mw; it.dy = pl.dy; it.dx = pl.dx;
    it.flags = im.flags & AA_MAPS_ITEM_FLIP;
    prefix[i] = units;
    if (pl.mh > 0) {  // (off the canvas: no table, no work unit, all fill)
      rc = maps_axis(vrun, filter, im.H, bx.y0, it.scale_h, pl.v0h, pl.mh, &it.oy, &it.hull_h, &it.ksize_h);
      if (rc != AA_OK) return rc;
      rc = maps_axis(hrun, filter, im.W, bx.x0, it.scale_w, pl.v0w, pl.mw, &it.ox, &it.hull_w, &it.ksize_w);
      if (rc != AA_OK) return rc;
      if (vrun) {
        it.flags |= AA_MAPS_ITEM_VPASS;
        it.tab_h = (int64_t)off;
        off += aa_maps_table_bytes(pl.mh, it.ksize_h);
      }
      if (hrun) {
        it.flags |= AA_MAPS_ITEM_HPASS;
        it.tab_w = (int64_t)off;
        off += aa_maps_table_bytes(pl.mw, it.ksize_w);
        units += (((int64_t)it.hull_h + AA_MAPS_HROWS - 1) / AA_MAPS_HROWS) * ((pl.mw + AA_MANY_STRIP - 1) / AA_MANY_STRIP);
        if (units > INT32_MAX) return AA_ERR_BAD_SHAPE;  // (one grid)
      }
    }
    items[i] = it;
  }
  prefix[n] = units;
  for (int64_t i = 0; i < n; i++) {
    if (!(items[i].flags & AA_MAPS_ITEM_HPASS)) continue;
    items[i].inter = (int64_t)off;
    off += aa_align16((size_t)((int64_t)items[i].hull_h * items[i].mw * EB));
  }
  memset(hd, 0, sizeof(*hd));
  hd->magic = AA_MAPS_MAGIC;
  hd->n = (int32_t)n; hd->oH = (int32_t)oH; hd->oW = (int32_t)oW;
  hd->filter = filter; hd->elem = elem; hd->overflow = overflow;
  hd->fill = fill_bits;
  hd->hunits = units;
  hd->ws_bytes = (int64_t)off;
  *workspace_bytes = off;
  return AA_OK;
}

// ---- host: the three launches --------------------------------------------------------------------------------------------------------------
template <typename T>
static void launch_passes(const AAMapsHeader *hd, const AAMapsItem *items, const int64_t *prefix, char *ws, void *out, int vstrips, hipStream_t stream) {
  const int clamp = hd->overflow == AA_MAPS_OVERFLOW_CLAMP ? 1 : 0;
  if (hd->hunits > 0)  // (0: no item's horizontal pass runs on the canvas)
    hipLaunchKernelGGL(maps_hpass<T>, dim3((unsigned)hd->hunits), dim3(AA_MANY_STRIP * kHWaves), 0, stream, items, prefix, ws, (int)hd->n, clamp);
  hipLaunchKernelGGL(maps_vpass<T>, dim3((unsigned)((int64_t)hd->n * hd->oH * vstrips)), dim3(AA_MAPS_VCOLS), 0, stream, items, (const char *)ws,
                     (T *)out, (int)hd->oH, (int)hd->oW, vstrips, hd->fill, clamp);
}

int aa_launch_many_maps(const void *desc_host, const void *desc_dev, void *out_dev, void *workspace_dev, size_t workspace_bytes,
                        hipStream_t stream) {
  const AAMapsHeader *hd = (const AAMapsHeader *)desc_host;
  if (hd->magic != AA_MAPS_MAGIC) return AA_ERR_BAD_SHAPE;
  if (hd->elem != AA_MAPS_U16 && hd->elem != AA_MAPS_I32 && hd->elem != AA_MAPS_F32) return AA_ERR_BAD_SHAPE;
  if (!aa_filter_valid(hd->filter) || hd->n < 0 || hd->oH <= 0 || hd->oW <= 0) return AA_ERR_BAD_SHAPE;
  const int64_t n = hd->n;
  const int rc = aa_many_check_launch(n, desc_dev, out_dev, workspace_dev, workspace_bytes, hd->ws_bytes, (size_t)aa_maps_elem_bytes(hd->elem));
  if (rc != AA_OK || n == 0) return rc;
  const int64_t vstrips = ((int64_t)hd->oW + AA_MAPS_VCOLS - 1) / AA_MAPS_VCOLS;
  if (n * hd->oH * vstrips > INT32_MAX || hd->hunits < 0 || hd->hunits > INT32_MAX) return AA_ERR_BAD_SHAPE;
  const AADescView<AAMapsItem> v = aa_desc_view<AAMapsHeader, AAMapsItem>(desc_dev, n);
  char *ws = (char *)workspace_dev;
  const int64_t tthreads = n * ((int64_t)hd->oH + hd->oW);
  hipLaunchKernelGGL(maps_tables, dim3((unsigned)((tthreads + 255) / 256)), dim3(256), 0, stream, v.items, ws, n, (int)hd->oH, (int)hd->oW, hd->filter);
  switch (hd->elem) {
    case AA_MAPS_U16: launch_passes<uint16_t>(hd, v.items, v.prefix, ws, out_dev, (int)vstrips, stream); break;
    case AA_MAPS_I32: launch_passes<int32_t>(hd, v.items, v.prefix, ws, out_dev, (int)vstrips, stream); break;
    default: launch_passes<float>(hd, v.items, v.prefix, ws, out_dev, (int)vstrips, stream); break;
  }
  AA_HIP_CHECK_LAUNCH();
  return AA_OK;
}
