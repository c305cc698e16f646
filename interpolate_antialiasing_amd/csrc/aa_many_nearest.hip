// aa_many_nearest.hip — Pillow's NEAREST for a ragged batch of label maps: uint8 images of 1..4 channels, or single-channel int16 / int32
// id maps, each with its own box, its own size, a place on the canvas and a flip, copied element by element into one dense batch (or into
// the int64 batch a loss reads).  Two launches whatever N:
//   1. near_tables  one lane per (item, axis).  Pillow picks its source index by ACCUMULATING a double step (xo += a per output index), not
//                   by a closed form, and the two differ (2 -> 7 is the smallest case), so the lane runs the sum in order from index 0 of
//                   the item's own size, whatever part of it lies on the canvas, and stores the covered entries: source rows for the
//                   vertical axis, source byte offsets per canvas unit for the horizontal one, mirrored for an item that flips.
//                   (Only "I;16", the 2-byte element, goes through Pillow's generic transform instead, which IS the closed form.)
//   2. near_gather  one workgroup per (item, plane, canvas row, 1 KiB of the row): the source row is wave-uniform, every lane produces one
//                   output dword from the table entries of its units, or the fill where the item is not.
// The planner (aa_near_plan_host) computes the covered ranges, the two doubles of every axis and the table offsets on the host: nothing
// comes back from the device, nothing is synchronised or allocated.  Indices are clamped to the image by the table kernel, so no load of
// the gather can leave an item's rows whatever the plan says.

#include <string.h>

#include "aa_many_host.h"
#include "aa_many_nearest.h"

namespace {

// ---- 1. tables ---------------------------------------------------------------------------------------------------------------------------
// The covered entries [v0, v0 + m) of one axis, written through p (`step` entries apart: negative for the mirrored horizontal table of an
// item that flips; UP entries per index, the source byte offsets idx * PB + k * EB).  A single lane is bound by instruction issue, so the
// loops are kept to the chain itself: the indices before v0 only add.
// CLOSED (2-byte elements): Pillow resizes an "I;16" image through its generic transform, which evaluates a * (x + 0.5) + b0 afresh for
// every index; the record's xo0 is then b0.  Same lane, same loop, no sum.
template <bool CLOSED, bool ONE>  // ONE: UP == 1, the loop without the inner one (unswitched by hand: the compiler does not)
__device__ inline void near_axis_entries(int32_t *p, int step, int UP, int PB, int EB, int v0, int m, int in_size, double a, double xo) {
  const double top = (double)(in_size - 1);
  if (!CLOSED)
    for (int x = 0; x < v0; x++) xo = xo + a;  // the sum starts at index 0 also where the placement crops the front
  for (int i = 0; i < m; i++) {
    const double xc = CLOSED ? a * ((double)(v0 + i) + 0.5) + xo : xo;
    const int idx = (int)fmax(fmin(xc, top), 0.0);  // Pillow's truncation; the clamp keeps every read inside the image
    if (ONE) {
      *p = idx * PB;
    } else {
      for (int k = 0; k < UP; k++) p[k] = idx * PB + k * EB;
    }
    p += step;
    if (!CLOSED) xo = xo + a;  // one IEEE double add per step, in order: the specification
  }
}

// Block b serves lanes_per_block (item, axis) pairs, one per lane; the other lanes of the wave idle.  The loop is a chain of dependent
// double adds and cannot be split: few lanes per block spread the chains over the compute units.
__global__ void __launch_bounds__(64) near_tables(const AANearItem *items, char *ws, int64_t n, int lanes_per_block, int E, int EB, int closed) {
  if ((int)threadIdx.x >= lanes_per_block) return;
  const int64_t t = (int64_t)blockIdx.x * lanes_per_block + threadIdx.x;
  if (t >= 2 * n) return;
  const AANearItem &it = items[t >> 1];
  const bool vert = (t & 1) == 0;
  const int m = vert ? it.mh : it.mw;
  if (m <= 0 || it.mh <= 0 || it.mw <= 0) return;  // off the canvas: no table
  const int v0 = vert ? it.v0h : it.v0w;
  const int in_size = vert ? it.in_h : it.in_w;
  const double a = vert ? it.a_h : it.a_w;
  const double xo = vert ? it.xo0_h : it.xo0_w;
  int32_t *tab = (int32_t *)(ws + (vert ? it.tab_h : it.tab_w));
  int UP = 1, PB = 1, eb = 1, step = 1;  // the vertical table: one entry per index, the source row itself
  if (!vert) {
    UP = aa_near_units_per_pixel(E, EB);
    PB = UP * EB;  // bytes of a pixel
    eb = EB;
    // the entries beside the covered units, which the gather's vector loads touch and never use
    const int lead = aa_near_lead((int64_t)it.dxo * UP, EB);
    const int64_t used = lead + (int64_t)m * UP, all = (used + 3) & ~(int64_t)3;
    for (int i = 0; i < lead; i++) tab[i] = 0;
    for (int64_t i = used; i < all; i++) tab[i] = 0;
    tab += lead;
    step = UP;
    if (it.flags & AA_MANY_FLIP_X) {  // canvas order: the last covered index first
      tab += (int64_t)(m - 1) * UP;
      step = -UP;
    }
  }
  if (closed) near_axis_entries<true, true>(tab, step, 1, PB, eb, v0, m, in_size, a, xo);  // (2-byte elements have one channel)
  else if (UP == 1) near_axis_entries<false, true>(tab, step, 1, PB, eb, v0, m, in_size, a, xo);
  else near_axis_entries<false, false>(tab, step, UP, PB, eb, v0, m, in_size, a, xo);
}

// ---- 2. gather ---------------------------------------------------------------------------------------------------------------------------
struct NearFill { int32_t f[4]; };
__device__ inline int32_t pick_fill(const NearFill &fl, int c) { return c == 0 ? fl.f[0] : (c == 1 ? fl.f[1] : (c == 2 ? fl.f[2] : fl.f[3])); }

template <typename T> __device__ inline int64_t widen(T v);
template <> __device__ inline int64_t widen<uint8_t>(uint8_t v) { return (int64_t)v; }                // torch.uint8: zero-extended
template <> __device__ inline int64_t widen<uint16_t>(uint16_t v) { return (int64_t)(int16_t)v; }     // torch.int16
template <> __device__ inline int64_t widen<uint32_t>(uint32_t v) { return (int64_t)(int32_t)v; }     // torch.int32

// T: the element (1, 2 or 4 bytes); a unit is one element, a lane owns the 4 / sizeof(T) units of one dword of the canvas row, counted
// from the row's first byte.  O64 (one channel): every element leaves as int64.
template <typename T, bool O64>
__global__ void __launch_bounds__(256) near_gather(const AANearItem *items, const char *ws, void *out, int oH, int oW, int planes, int E,
                                                   int nstrips, const NearFill fl) {
  constexpr int EB = (int)sizeof(T), NE = 4 / EB;
  // the item whose units hold this one: every item has the whole canvas, so the descriptor's prefix sums are i * (planes * oH * nstrips)
  // and a division finds what a search through them would (one dependent load less per step of it, in a kernel that is all latency)
  const unsigned per_item = (unsigned)(planes * oH * nstrips);
  const int lo = (int)(blockIdx.x / per_item);
  const AANearItem &it = items[lo];
  unsigned u = blockIdx.x - (unsigned)lo * per_item;
  const int strip = (int)(u % (unsigned)nstrips);
  u /= (unsigned)nstrips;
  const int y = (int)(u % (unsigned)oH);
  const int plane = (int)(u / (unsigned)oH);
  const int UP = aa_near_units_per_pixel(E, EB);
  const int64_t RU = (int64_t)oW * UP;  // units of a canvas row
  const int64_t e0 = ((int64_t)strip * 256 + threadIdx.x) * NE;
  if (e0 >= RU) return;
  const int nu = RU - e0 < NE ? (int)(RU - e0) : NE;

  T v[NE];
#pragma unroll
  for (int q = 0; q < NE; q++) v[q] = (T)pick_fill(fl, EB > 1 ? 0 : (E == 1 ? plane : (int)((e0 + q) % E)));
  const int ty = y - it.dy;
  const int64_t cu0 = (int64_t)it.dxo * UP, cu1 = cu0 + (int64_t)it.mw * UP;  // the covered units of a canvas row
  if (ty >= 0 && ty < it.mh && e0 + NE > cu0 && e0 < cu1) {
    const int srow = ((const int32_t *)(ws + it.tab_h))[ty];  // (wave-uniform)
    const uint8_t *rowp = it.src + (int64_t)plane * it.plane_stride + (int64_t)srow * it.row_stride;
    // the lane's entries are one aligned vector of the table: entry `lead` is unit cu0, and cu0 - lead is a multiple of NE
    const int32_t *tw = (const int32_t *)(ws + it.tab_w) + (e0 - (cu0 - aa_near_lead(cu0, EB)));
    int32_t off[NE];
    if constexpr (NE == 4) {
      const int4 o = *(const int4 *)tw;
      off[0] = o.x; off[1] = o.y; off[2] = o.z; off[3] = o.w;
    } else if constexpr (NE == 2) {
      const int2 o = *(const int2 *)tw;
      off[0] = o.x; off[1] = o.y;
    } else {
      off[0] = *tw;
    }
#pragma unroll
    for (int q = 0; q < NE; q++)
      if (e0 + q >= cu0 && e0 + q < cu1) v[q] = *(const T *)(rowp + off[q]);
  }

  const int64_t row = ((int64_t)lo * planes + plane) * oH + y;
  if constexpr (O64) {
    int64_t *op = (int64_t *)out + row * RU + e0;
    if (NE == 4 && nu == 4 && ((uintptr_t)op & 15) == 0) {
      longlong2 a, b;
      a.x = widen<T>(v[0]); a.y = widen<T>(v[1]); b.x = widen<T>(v[NE > 2 ? 2 : 0]); b.y = widen<T>(v[NE > 3 ? 3 : 0]);
      ((longlong2 *)op)[0] = a;
      ((longlong2 *)op)[1] = b;
    } else {
#pragma unroll
      for (int q = 0; q < NE; q++)
        if (q < nu) op[q] = widen<T>(v[q]);
    }
  } else {
    T *op = (T *)out + row * RU + e0;
    if (nu == NE && ((uintptr_t)op & 3) == 0) {
      uint32_t w = 0;
#pragma unroll
      for (int q = 0; q < NE; q++) w |= (uint32_t)v[q] << (8 * EB * q);
      *(uint32_t *)op = w;
    } else {  // a row end, or a canvas row that does not start on a dword: element by element
#pragma unroll
      for (int q = 0; q < NE; q++)
        if (q < nu) op[q] = v[q];
    }
  }
}

}  // namespace

// ---- host: the planner -------------------------------------------------------------------------------------------------------------------
size_t aa_near_desc_size(int64_t n) { return aa_desc_size(sizeof(AANearHeader), sizeof(AANearItem), n); }

// Pillow's two doubles of an axis: the step, aa_pil_scale of the box (float32 values already, and NEAREST takes their float difference
// with or without a box); the first centre (closed: b0 itself).
static void near_axis(double b0, double b1, int64_t out_size, bool closed, double *a, double *xo0) {
  const double step = aa_pil_scale(1, b0, b1, 0.0, out_size);
  const double half = step * 0.5;
  *a = step;
  *xo0 = closed ? b0 : b0 + half;
}

int aa_near_plan_host(int layout, int elem_bytes, int64_t n, int64_t C, int64_t oH, int64_t oW, const aa_many_image *images,
                      const aa_many_place *places, const int32_t *fill, void *desc_host, size_t desc_bytes, size_t *workspace_bytes) {
  if (layout != AA_NCHW && layout != AA_NHWC) return AA_ERR_BAD_LAYOUT;
  if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4) return AA_ERR_BAD_DTYPE;
  // (2- and 4-byte elements are single-channel id maps)
  const int rc0 = aa_many_check_canvas(n, kAAManyMax, C >= 1 && C <= 4 && (elem_bytes == 1 || C == 1), oH, oW, desc_host, workspace_bytes, images, places);
  if (rc0 != AA_OK) return rc0;
  for (int c = 0; fill && c < C; c++) {  // what the element holds, signed or unsigned
    const int64_t lo = elem_bytes == 4 ? INT32_MIN : -((int64_t)1 << (8 * elem_bytes - 1)), hi = elem_bytes == 4 ? INT32_MAX : ((int64_t)1 << (8 * elem_bytes)) - 1;
    if (fill[c] < lo || fill[c] > hi) return AA_ERR_BAD_SHAPE;
  }
  if (desc_bytes < aa_near_desc_size(n)) return AA_ERR_WORKSPACE;
  const int E = layout == AA_NHWC ? (int)C : 1;
  const int64_t planes = layout == AA_NHWC ? 1 : C;
  const int UP = aa_near_units_per_pixel(E, elem_bytes);
  const int64_t PB = (int64_t)UP * elem_bytes;
  const int64_t vstrips = (oW * PB + AA_MANY_VBYTES - 1) / AA_MANY_VBYTES;
  const int64_t per_item = planes * oH * vstrips;
  if (n * per_item > INT32_MAX) return AA_ERR_BAD_SHAPE;  // (one grid)

  AANearHeader *hd = (AANearHeader *)desc_host;
  AANearItem *items = (AANearItem *)(hd + 1);
  int64_t *prefix = (int64_t *)(items + n);
  size_t off = 0;
  const aa_many_place whole = {oH, oW, 0, 0};
  for (int64_t i = 0; i < n; i++) {
    const aa_many_image &im = images[i];
    AANearItem it;
    memset(&it, 0, sizeof(it));
    AAManyBox bx;
    const int rc = aa_many_check_image_box(im, (im.flags & ~AA_MANY_FLIP_X) == 0, layout, C, elem_bytes, PB, &bx);
    if (rc != AA_OK) return rc;
    // the item's own size and the part [v0, v0 + m) of it that lies on the canvas, per axis (no places: all of the canvas)
    const AAManyPlace pl = aa_many_cover(places ? places[i] : whole, oH, oW);
    const bool flip = (im.flags & AA_MANY_FLIP_X) != 0;
    it.src = (const uint8_t *)im.data_dev;
    it.row_stride = im.H > 1 ? im.stride_row : 0;
    it.plane_stride = planes > 1 ? im.stride_ch : 0;
    near_axis(bx.y0, bx.y1, pl.vh, elem_bytes == 2, &it.a_h, &it.xo0_h);
    near_axis(bx.x0, bx.x1, pl.vw, elem_bytes == 2, &it.a_w, &it.xo0_w);
    it.in_h = (int32_t)im.H; it.in_w = (int32_t)im.W;
    it.vh = pl.vh; it.vw = pl.vw; it.v0h = pl.v0h; it.v0w = pl.v0w;
    it.mh = pl.mh; it.mw = pl.mw; it.dy = pl.dy; it.dx = pl.dx;
    it.dxo = (int32_t)(pl.mw ? (flip ? oW - pl.dx - pl.mw : pl.dx) : 0);
    it.flags = im.flags & AA_MANY_FLIP_X;
    it.tab_h = (int64_t)off;
    off += aa_near_tab_h_bytes(pl.mh);
    it.tab_w = (int64_t)off;
    off += aa_near_tab_w_bytes((int64_t)it.dxo * UP, (int64_t)pl.mw * UP, elem_bytes);
    prefix[i] = i * per_item;
    items[i] = it;
  }
  prefix[n] = n * per_item;
  memset(hd, 0, sizeof(*hd));
  hd->magic = AA_NEAR_MAGIC;
  hd->n = (int32_t)n; hd->C = (int32_t)C; hd->oH = (int32_t)oH; hd->oW = (int32_t)oW;
  hd->layout = layout; hd->elem_bytes = elem_bytes;
  hd->units = n * per_item;
  hd->ws_bytes = (int64_t)off;
  for (int c = 0; fill && c < C; c++) hd->fill[c] = fill[c];
  *workspace_bytes = off;
  return AA_OK;
}

// ---- host: the two launches --------------------------------------------------------------------------------------------------------------
template <typename T>
static void launch_gather(bool o64, const AANearHeader *hd, const AANearItem *items, const char *ws, void *out, int planes,
                          int E, int nstrips, hipStream_t stream) {
  NearFill fl;
  for (int c = 0; c < 4; c++) fl.f[c] = hd->fill[c];
  const dim3 grid((unsigned)hd->units);
  if (o64)
    hipLaunchKernelGGL((near_gather<T, true>), grid, dim3(256), 0, stream, items, ws, out, hd->oH, hd->oW, planes, E, nstrips, fl);
  else
    hipLaunchKernelGGL((near_gather<T, false>), grid, dim3(256), 0, stream, items, ws, out, hd->oH, hd->oW, planes, E, nstrips, fl);
}

int aa_launch_many_nearest(const void *desc_host, const void *desc_dev, void *out_dev, void *workspace_dev, size_t workspace_bytes,
                           int out_elem_bytes, hipStream_t stream) {
  const AANearHeader *hd = (const AANearHeader *)desc_host;
  if (hd->magic != AA_NEAR_MAGIC) return AA_ERR_BAD_SHAPE;
  const int EB = hd->elem_bytes;
  const int64_t n = hd->n;
  if (EB != 1 && EB != 2 && EB != 4) return AA_ERR_BAD_SHAPE;
  if (out_elem_bytes != EB && out_elem_bytes != 8) return AA_ERR_BAD_DTYPE;
  if (out_elem_bytes == 8 && hd->C != 1) return AA_ERR_BAD_DTYPE;  // (the int64 form is for single-channel maps)
  const int rc = aa_many_check_launch(n, desc_dev, out_dev, workspace_dev, workspace_bytes, hd->ws_bytes, (size_t)out_elem_bytes);
  if (rc != AA_OK || n == 0) return rc;
  const AANearItem *items = aa_desc_view<AANearHeader, AANearItem>(desc_dev, n).items;
  const int E = hd->layout == AA_NHWC ? hd->C : 1;
  const int planes = hd->layout == AA_NHWC ? 1 : hd->C;
  const int64_t PB = (int64_t)aa_near_units_per_pixel(E, EB) * EB;
  const int nstrips = (int)((hd->oW * PB + AA_MANY_VBYTES - 1) / AA_MANY_VBYTES);
  if (hd->units != n * planes * hd->oH * nstrips) return AA_ERR_BAD_SHAPE;
  char *ws = (char *)workspace_dev;
  // up to 2048 single-lane waves, then more lanes per wave
  int64_t lanes = (2 * n + 2047) / 2048;
  if (lanes > 64) lanes = 64;
  hipLaunchKernelGGL(near_tables, dim3((unsigned)((2 * n + lanes - 1) / lanes)), dim3(64), 0, stream, items, ws, n, (int)lanes, E, EB,
                     EB == 2 ? 1 : 0);
  const bool o64 = out_elem_bytes == 8;
  switch (EB) {
    case 1: launch_gather<uint8_t>(o64, hd, items, ws, out_dev, planes, E, nstrips, stream); break;
    case 2: launch_gather<uint16_t>(o64, hd, items, ws, out_dev, planes, E, nstrips, stream); break;
    default: launch_gather<uint32_t>(o64, hd, items, ws, out_dev, planes, E, nstrips, stream); break;
  }
  AA_HIP_CHECK_LAUNCH();
  return AA_OK;
}
