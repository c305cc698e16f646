// aa_many_ycbcr.hip — subsampled YCbCr planes to an RGB batch (aa_many_ycbcr.h).  The resampling passes are linear and every plane is
// resized at its own resolution, exactly as Pillow resizes an "L" image; the colour conversion runs once per output pixel as the
// vertical pass emits.  Launches whatever n:
//   planar chroma (Y, Cb, Cr)      3: many_tables and many_hpass<1> of aa_many.hip over all 3 n planes, then ycc_vpass
//   interleaved chroma (Y, CbCr)   5: many_tables and many_hpass<1> over the n luma planes, many_tables and many_hpass<2> over the n
//                                     chroma pairs (their rows differ in bytes per pixel, so they cannot share a launch), then ycc_vpass
// The planner composes placed plans of aa_many.hip (nothing of its arithmetic is repeated here) and the table and horizontal kernels
// are aa_many.hip's own.  New here is the converting vertical pass.
// ycc_vpass: a workgroup is AA_YCC_VROWS waves, one canvas row each, 64 lanes x 4 consecutive pixels = AA_YCC_VCOLS columns of one item.
// A lane walks the vertical window three times — the luma dword, then the Cb and the Cr dword, or the two dwords of four interleaved
// Cb Cr pairs — with many_vpass's integer sums and pack4_clip8, converts its four pixels (aa_ycbcr.h: the table entries are computed
// in registers, DESIGN.md says why), mixes in the fill where its pixels straddle the item's edge, mirrors for a flip and stores twelve
// bytes (dword stores where the address allows) or twelve elements.
#include <string.h>

#include <vector>

#include "aa_many_dev.h"
#include "aa_many_host.h"
#include "aa_many_ycbcr.h"
#include "aa_ycbcr.h"

namespace {

// many_vpass_float's conversion of a byte, (T)(((float)byte - mean[c]) / std[c]), with its to_elem (aa_many_dev.h).
struct YccConvert { int normalize; float mean[3], std[3]; };

// The clipped bytes of NDW consecutive dwords from byte `at` of the intermediate's rows, down the window of entry t of an item's vertical
// table (`out` entries): many_vpass's sums (vtap_sums of aa_many.hip, for NDW dwords with a validity mask; one definition for both
// changes the registers of one file's kernels or the other's, profiles/ragged_shared_refactor.txt).  ok[d]: dword d lies inside the
// row; one that does not counts as 0 (of four pairs the first two may lie before the item's first column, the last two beyond its last).
template <int NDW>
__device__ inline void vwalk(const AAManyItem &it, const char *ws, int out, int t, int64_t pitch, int64_t at, const bool (&ok)[NDW],
                             uint32_t (&res)[NDW]) {
  const int32_t *xmin_p = (const int32_t *)(ws + it.tab_h);
  const int32_t *xsize_p = xmin_p + out;
  const int ksize = it.ksize_h;
  const int32_t *wp = xsize_p + out + (size_t)t * ksize;
  int r0 = xmin_p[t], nr = xsize_p[t];
  if (nr > ksize) nr = ksize;
  if (r0 < 0) r0 = 0;
  if (r0 + nr > it.hull_h) nr = it.hull_h - r0;
  const uint8_t *ip = (const uint8_t *)ws + it.inter + (int64_t)r0 * pitch + at;
  int32_t s[4 * NDW];
#pragma unroll
  for (int q = 0; q < 4 * NDW; q++) s[q] = 1 << 21;
  for (int k = 0; k < nr; k++) {
    const int32_t wk = wp[k];
#pragma unroll
    for (int d = 0; d < NDW; d++) {
      const uint32_t v = ok[d] ? *(const uint32_t *)(ip + k * pitch + 4 * d) : 0u;
      s[4 * d] += (int32_t)(v & 255u) * wk;
      s[4 * d + 1] += (int32_t)((v >> 8) & 255u) * wk;
      s[4 * d + 2] += (int32_t)((v >> 16) & 255u) * wk;
      s[4 * d + 3] += (int32_t)(v >> 24) * wk;
    }
  }
#pragma unroll
  for (int d = 0; d < NDW; d++) res[d] = pack4_clip8(s[4 * d], s[4 * d + 1], s[4 * d + 2], s[4 * d + 3]);
}

// T: uint8_t, float, f16_t, bf16_t.  IL: plan B holds interleaved chroma pairs.  NHWC: the output's layout.
template <typename T, bool IL, bool NHWC>
__global__ void __launch_bounds__(64 * AA_YCC_VROWS) ycc_vpass(const AAManyItem *items_a, const AAManyPlace *places_a, const AAManyItem *items_b,
                                                                const char *ws_a, const char *ws_b, T *out, int n, int oH, int oW, int nstrips,
                                                                const YccConvert cv, uint32_t fill) {
  int64_t u = blockIdx.x;
  const int strip = (int)(u % nstrips);
  u /= nstrips;
  const int ygroups = (oH + AA_YCC_VROWS - 1) / AA_YCC_VROWS;
  const int y = (int)(u % ygroups) * AA_YCC_VROWS + (int)threadIdx.y;
  const int64_t i = u / ygroups;
  const int x = strip * AA_YCC_VCOLS + 4 * (int)threadIdx.x;
  if (y >= oH || x >= oW) return;
  const int npx = oW - x < 4 ? oW - x : 4;
  const AAManyItem &ity = items_a[i];
  const AAManyPlace pl = places_a[i];  // (the chroma items of the image have the same place, so the same covered part)

  // R, G, B of the four pixels, one dword per channel: the fill, or the converted sums where the item covers the pixel
  uint32_t ch[3] = {(fill & 255u) * 0x01010101u, ((fill >> 8) & 255u) * 0x01010101u, ((fill >> 16) & 255u) * 0x01010101u};
  const int ty = y - pl.dy;
  if (ty >= 0 && ty < pl.mh && x + 4 > pl.dx && x < pl.dx + pl.mw) {
    // (the rows of an intermediate are led so that a canvas dword is a dword of the row: aa_many.h)
    const int64_t at = x - (pl.dx & ~3);
    const int64_t pitch = aa_many_placed_pitch(pl.dx, pl.mw, 1);
    const bool one[1] = {true};
    uint32_t yw[1], cbw, crw;
    vwalk<1>(ity, ws_a, pl.mh, ty, pitch, at, one, yw);
    if (IL) {  // four Cb Cr pairs: canvas byte 2 x of the pair row
      const int64_t pitch2 = aa_many_placed_pitch(pl.dx, pl.mw, 2), at2 = 2 * (int64_t)x - ((2 * (int64_t)pl.dx) & ~(int64_t)3);
      // (2 dx & ~3 may exceed 2 (dx & ~3): the first dword then lies before the row; the last may lie beyond its pitch)
      const bool two[2] = {at2 >= 0, at2 + 8 <= pitch2};
      uint32_t cw[2];
      vwalk<2>(items_b[i], ws_b, pl.mh, ty, pitch2, at2, two, cw);
      cbw = byte_of(cw[0], 0) | (byte_of(cw[0], 2) << 8) | (byte_of(cw[1], 0) << 16) | (byte_of(cw[1], 2) << 24);
      crw = byte_of(cw[0], 1) | (byte_of(cw[0], 3) << 8) | (byte_of(cw[1], 1) << 16) | (byte_of(cw[1], 3) << 24);
    } else {
      uint32_t w[1];
      vwalk<1>(items_a[n + i], ws_a, pl.mh, ty, pitch, at, one, w);
      cbw = w[0];
      vwalk<1>(items_a[2 * (int64_t)n + i], ws_a, pl.mh, ty, pitch, at, one, w);
      crw = w[0];
    }
    uint32_t r = 0, g = 0, b = 0, mask = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const uint32_t rgb = aa_ycbcr_to_rgb((int)byte_of(yw[0], q), (int)byte_of(cbw, q), (int)byte_of(crw, q));
      r |= (rgb & 255u) << (8 * q);
      g |= ((rgb >> 8) & 255u) << (8 * q);
      b |= ((rgb >> 16) & 255u) << (8 * q);
      if (x + q >= pl.dx && x + q < pl.dx + pl.mw) mask |= 255u << (8 * q);
    }
    ch[0] = (r & mask) | (ch[0] & ~mask);
    ch[1] = (g & mask) | (ch[1] & ~mask);
    ch[2] = (b & mask) | (ch[2] & ~mask);
  }

  // the npx pixels go to columns [xs, xs + npx), in reversed order for an item that flips
  int xs = x;
  if (ity.flags & AA_MANY_ITEM_FLIP) {
    xs = oW - x - npx;
#pragma unroll
    for (int c = 0; c < 3; c++) ch[c] = __builtin_bswap32(ch[c]) >> (8 * (4 - npx));
  }

  if constexpr (sizeof(T) == 1) {
    uint8_t *o = (uint8_t *)out;
    if (NHWC) {
      uint8_t *p = o + ((i * oH + y) * oW + xs) * 3;
      if (npx == 4 && ((uintptr_t)p & 3) == 0) {
        uint32_t *p4 = (uint32_t *)p;
        p4[0] = byte_of(ch[0], 0) | (byte_of(ch[1], 0) << 8) | (byte_of(ch[2], 0) << 16) | (byte_of(ch[0], 1) << 24);
        p4[1] = byte_of(ch[1], 1) | (byte_of(ch[2], 1) << 8) | (byte_of(ch[0], 2) << 16) | (byte_of(ch[1], 2) << 24);
        p4[2] = byte_of(ch[2], 2) | (byte_of(ch[0], 3) << 8) | (byte_of(ch[1], 3) << 16) | (byte_of(ch[2], 3) << 24);
      } else {
#pragma unroll
        for (int q = 0; q < 4; q++) {
          if (q >= npx) break;
#pragma unroll
          for (int c = 0; c < 3; c++) p[3 * q + c] = (uint8_t)byte_of(ch[c], q);
        }
      }
    } else {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        uint8_t *p = o + (((i * 3 + c) * oH + y) * oW + xs);
        if (npx == 4 && ((uintptr_t)p & 3) == 0) {
          *(uint32_t *)p = ch[c];
        } else {
#pragma unroll
          for (int q = 0; q < 4; q++) {
            if (q >= npx) break;
            p[q] = (uint8_t)byte_of(ch[c], q);
          }
        }
      }
    }
  } else {  // (an element store is always aligned: the entry point checks the output's address against its element)
#pragma unroll
    for (int q = 0; q < 4; q++) {
      if (q >= npx) break;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        float v = (float)byte_of(ch[c], q);
        if (cv.normalize) v = (v - cv.mean[c]) / cv.std[c];
        const int64_t at = NHWC ? ((i * oH + y) * oW + xs + q) * 3 + c : ((i * 3 + c) * oH + y) * oW + xs + q;
        out[at] = to_elem<T>(v);
      }
    }
  }
}

struct YccArgs {
  const AAManyItem *items_a;
  const AAManyPlace *places_a;
  const AAManyItem *items_b;
  const char *ws_a, *ws_b;
  void *out;
  int n, oH, oW, nstrips;
  unsigned grid;
  YccConvert cv;
  uint32_t fill;
  hipStream_t stream;
};

template <typename T, bool IL, bool NHWC>
void launch_vpass(const YccArgs &a) {
  hipLaunchKernelGGL((ycc_vpass<T, IL, NHWC>), dim3(a.grid), dim3(64, AA_YCC_VROWS), 0, a.stream, a.items_a, a.places_a, a.items_b, a.ws_a, a.ws_b,
                     (T *)a.out, a.n, a.oH, a.oW, a.nstrips, a.cv, a.fill);
}

template <typename T>
void launch_vpass_t(bool il, bool nhwc, const YccArgs &a) {
  if (il) nhwc ? launch_vpass<T, true, true>(a) : launch_vpass<T, true, false>(a);
  else nhwc ? launch_vpass<T, false, true>(a) : launch_vpass<T, false, false>(a);
}

const AAManyItem *plan_items(const void *plan) { return aa_desc_view<AAManyHeader, AAManyItem>(plan, 0).items; }
// (a placed plan: the placement records follow the prefix sums)
const AAManyPlace *plan_places(const void *plan, int64_t n) { return (const AAManyPlace *)(aa_desc_view<AAManyHeader, AAManyItem>(plan, n).prefix + n + 1); }

}  // namespace

// ---- host: the planner -----------------------------------------------------------------------------------------------------------------------
size_t aa_ycc_desc_size(int64_t n) {
  if (n < 0 || n > kAAManyMax) return 0;
  // (planar: one plan of 3 n items; interleaved: two of n, which is never more)
  const size_t one = aa_many_desc_size_placed(3 * n), two = 2 * aa_many_desc_size_placed(n);
  return sizeof(AAYccHeader) + (one > two ? one : two);
}

int aa_ycc_plan_host(int filter, int64_t n, int64_t oH, int64_t oW, const aa_ycbcr_image *images, const aa_many_place *places,
                     const uint8_t *fill, void *desc_host, size_t desc_bytes, size_t *workspace_bytes) {
  if (!aa_filter_valid(filter)) return AA_ERR_BAD_FILTER;
  // (the places are checked where the composed plans are made, after the images)
  const int rc0 = aa_many_check_canvas(n, kAAManyMax / 3, true, oH, oW, desc_host, workspace_bytes, images, nullptr);
  if (rc0 != AA_OK) return rc0;
  if (desc_bytes < aa_ycc_desc_size(n)) return AA_ERR_WORKSPACE;
  const int64_t ygroups = (oH + AA_YCC_VROWS - 1) / AA_YCC_VROWS, vstrips = (oW + AA_YCC_VCOLS - 1) / AA_YCC_VCOLS;
  if (n * ygroups * vstrips > INT32_MAX) return AA_ERR_BAD_SHAPE;  // (the grid of the vertical pass)
  const bool il = n > 0 && images[0].chroma_stride_px == 2;
  // plan A's records: the luma items, then (planar) the Cb and the Cr items; plan B's: the chroma pairs
  std::vector<aa_many_image> ia((size_t)(il ? n : 3 * n)), ib((size_t)(il ? n : 0));
  std::vector<aa_many_place> pa(ia.size());
  int flips = 0;
  for (int64_t i = 0; i < n; i++) {
    const aa_ycbcr_image &im = images[i];
    if (!im.y_dev || !im.cb_dev || !im.cr_dev) return AA_ERR_NULL;
    if (im.subsampling < AA_YCC_444 || im.subsampling > AA_YCC_440 || (im.flags & ~AA_MANY_FLIP_X)) return AA_ERR_BAD_SHAPE;
    const int sx = (im.subsampling == AA_YCC_422 || im.subsampling == AA_YCC_420) ? 2 : 1;
    const int sy = (im.subsampling == AA_YCC_420 || im.subsampling == AA_YCC_440) ? 2 : 1;
    if (im.H <= 0 || im.W <= 0 || im.H > kAAManyMax || im.W > kAAManyMax) return AA_ERR_BAD_SHAPE;
    if (im.cH != (im.H + sy - 1) / sy || im.cW != (im.W + sx - 1) / sx) return AA_ERR_BAD_SHAPE;
    if (im.chroma_stride_px != (il ? 2 : 1)) return AA_ERR_STRIDES;  // (one arrangement per call)
    if (il && ((const uint8_t *)im.cr_dev != (const uint8_t *)im.cb_dev + 1 || (im.cH > 1 && im.cr_stride_row != im.cb_stride_row))) return AA_ERR_STRIDES;
    aa_many_image y;
    memset(&y, 0, sizeof(y));
    y.data_dev = im.y_dev;
    y.H = im.H; y.W = im.W;
    y.stride_row = im.y_stride_row; y.stride_px = 1;
    y.has_box = im.has_box;
    for (int k = 0; k < 4; k++) y.box[k] = im.box[k];
    y.flags = im.flags;
    flips |= im.flags & AA_MANY_FLIP_X;
    // the chroma box: the luma box (or the whole luma plane) over the subsampling, in float32 — a division by 1 or 2 is exact.  It is a
    // proper box even without one on the luma: for an odd W the last chroma sample reaches half a sample beyond the luma plane
    aa_many_image c = y;
    c.flags = 0;
    c.H = im.cH; c.W = im.cW;
    c.has_box = 1;
    const float lb[4] = {im.has_box ? (float)im.box[0] : 0.f, im.has_box ? (float)im.box[1] : 0.f, im.has_box ? (float)im.box[2] : (float)im.W,
                         im.has_box ? (float)im.box[3] : (float)im.H};
    c.box[0] = (double)(lb[0] / (float)sx); c.box[1] = (double)(lb[1] / (float)sy);
    c.box[2] = (double)(lb[2] / (float)sx); c.box[3] = (double)(lb[3] / (float)sy);
    const aa_many_place whole = {oH, oW, 0, 0};
    const aa_many_place p = places ? places[i] : whole;
    ia[(size_t)i] = y;
    pa[(size_t)i] = p;
    c.data_dev = im.cb_dev;
    c.stride_row = im.cb_stride_row;
    if (il) {
      c.stride_px = 2; c.stride_ch = 1;
      ib[(size_t)i] = c;
    } else {
      ia[(size_t)(n + i)] = c;
      pa[(size_t)(n + i)] = p;
      c.data_dev = im.cr_dev;
      c.stride_row = im.cr_stride_row;
      ia[(size_t)(2 * n + i)] = c;
      pa[(size_t)(2 * n + i)] = p;
    }
  }
  AAYccHeader *hd = (AAYccHeader *)desc_host;
  memset(hd, 0, sizeof(*hd));
  const int64_t na = (int64_t)ia.size();
  hd->off_a = sizeof(AAYccHeader);
  size_t ws_a = 0, ws_b = 0;
  int rc = aa_many_plan_placed_always_host(filter, AA_NCHW, na, 1, oH, oW, ia.data(), pa.data(), (char *)desc_host + hd->off_a,
                                           aa_many_desc_size_placed(na), &ws_a);
  if (rc != AA_OK) return rc;
  ws_a = aa_align16(ws_a);
  if (il) {
    hd->off_b = hd->off_a + (int64_t)aa_many_desc_size_placed(na);
    rc = aa_many_plan_placed_always_host(filter, AA_NHWC, n, 2, oH, oW, ib.data(), pa.data(), (char *)desc_host + hd->off_b,
                                         aa_many_desc_size_placed(n), &ws_b);
    if (rc != AA_OK) return rc;
  }
  hd->magic = AA_YCC_MAGIC;
  hd->n = (int32_t)n; hd->oH = (int32_t)oH; hd->oW = (int32_t)oW;
  hd->filter = filter;
  hd->interleaved = il ? 1 : 0;
  hd->flips = flips;
  for (int c = 0; fill && c < 3; c++) hd->fill |= (uint32_t)fill[c] << (8 * c);
  hd->ws_b = (int64_t)ws_a;
  hd->ws_bytes = (int64_t)(ws_a + ws_b);
  *workspace_bytes = ws_a + ws_b;
  return AA_OK;
}

// ---- host: the launches ----------------------------------------------------------------------------------------------------------------------
int aa_launch_many_ycbcr(const void *desc_host, const void *desc_dev, void *out_dev, void *workspace_dev, size_t workspace_bytes, int out_elem,
                         int out_layout, int normalize, const float *mean, const float *std, hipStream_t stream) {
  const AAYccHeader *hd = (const AAYccHeader *)desc_host;
  if (hd->magic != AA_YCC_MAGIC || hd->n < 0) return AA_ERR_BAD_SHAPE;
  if (out_layout != AA_NCHW && out_layout != AA_NHWC) return AA_ERR_BAD_LAYOUT;
  if (out_elem != AA_U8 && out_elem != AA_F32 && out_elem != AA_F16 && out_elem != AA_BF16) return AA_ERR_BAD_DTYPE;
  const int64_t n = hd->n;
  int rc = aa_many_check_launch(n, desc_dev, out_dev, workspace_dev, workspace_bytes, hd->ws_bytes, out_elem == AA_F32 ? 4 : (out_elem == AA_U8 ? 1 : 2));
  if (rc != AA_OK || n == 0) return rc;
  const bool il = hd->interleaved != 0;
  const char *plan_a = (const char *)desc_host + hd->off_a, *plan_a_dev = (const char *)desc_dev + hd->off_a;
  const char *plan_b = il ? (const char *)desc_host + hd->off_b : nullptr, *plan_b_dev = il ? (const char *)desc_dev + hd->off_b : nullptr;
  char *ws_a = (char *)workspace_dev, *ws_b = ws_a + hd->ws_b;
  const int64_t na = il ? n : 3 * n;
  rc = aa_launch_many_tables_hpass(plan_a, plan_a_dev, ws_a, (size_t)hd->ws_b, stream);
  if (rc != AA_OK) return rc;
  if (il) {
    rc = aa_launch_many_tables_hpass(plan_b, plan_b_dev, ws_b, (size_t)(hd->ws_bytes - hd->ws_b), stream);
    if (rc != AA_OK) return rc;
  }
  YccArgs a;
  a.items_a = plan_items(plan_a_dev);
  a.places_a = plan_places(plan_a_dev, na);
  a.items_b = il ? plan_items(plan_b_dev) : nullptr;
  a.ws_a = ws_a; a.ws_b = ws_b;
  a.out = out_dev;
  a.n = (int)n; a.oH = hd->oH; a.oW = hd->oW;
  a.nstrips = (hd->oW + AA_YCC_VCOLS - 1) / AA_YCC_VCOLS;
  a.grid = (unsigned)(n * ((hd->oH + AA_YCC_VROWS - 1) / AA_YCC_VROWS) * a.nstrips);
  a.cv.normalize = normalize ? 1 : 0;
  for (int c = 0; c < 3; c++) { a.cv.mean[c] = normalize ? mean[c] : 0.f; a.cv.std[c] = normalize ? std[c] : 1.f; }
  a.fill = hd->fill;
  a.stream = stream;
  const bool nhwc = out_layout == AA_NHWC;
  if (out_elem == AA_U8) launch_vpass_t<uint8_t>(il, nhwc, a);
  else if (out_elem == AA_F16) launch_vpass_t<f16_t>(il, nhwc, a);
  else if (out_elem == AA_BF16) launch_vpass_t<bf16_t>(il, nhwc, a);
  else launch_vpass_t<float>(il, nhwc, a);
  AA_HIP_CHECK_LAUNCH();
  return AA_OK;
}
