// aa_many.hip — the ragged call: a list of uint8 images of different sizes, each with its own box, resampled into one dense batch with
// Pillow's 8bpc arithmetic.  Three launches whatever N:
//   1. many_tables  every item's two AA_TABLE_PIL coefficient sets into one arena (aa_pil_coeffs.h: the packed tables' own expressions);
//   2. many_hpass   one workgroup per (item, plane, hull row, strip of 64 output columns), found from prefix sums: the grid is the sum of
//                   the items' work, not N x the largest item;
//   3. many_vpass   one workgroup per (item, plane, output row, 1 KiB of the row);
//      or many_vpass_float, the converting form: the same sums, then byte -> float -> (v - mean) / std -> f32 / f16 / bf16, written in the
//      requested layout, mirrored left to right for the items that flip;
//      or many_vpass_patches, the same conversion with ragged work units: every item its own size, its pixels scattered into the rows
//      of a packed (or zero-padded) matrix of ViT patch tokens.
// A PLACED plan (template parameter PL) gives every item its own output size and a place on the canvas: the tables hold the covered
// part of the item's own resize only, the horizontal pass computes the covered columns only, and the vertical pass, still one grid over
// the whole canvas, writes the fill wherever the item is not.  The plain instantiations take none of it.
// An ALPHA plan (template parameter AL: some item asked for AA_MANY_PREMUL_ALPHA and is not Pillow's copy) resizes such items the way
// Pillow resizes RGBA / LA: the horizontal pass premultiplies the colour bytes it stages, the intermediate holds filtered premultiplied
// bytes, and the vertical passes convert every output pixel back with its own resampled alpha.  Same plan, same workspace, same launches.
// The host planner (aa_many_plan_host) computes every hull, ksize and offset with the same double arithmetic the table kernel uses, so
// nothing comes back from the device: no header read-back, no atomicMax, no synchronisation, no allocation.
// Shared with the other ragged calls: aa_many_dev.h (the item of a work unit, the table view, the element types), aa_many_host.h (checks).

#include <math.h>
#include <string.h>

#include "aa_alpha.h"
#include "aa_many_dev.h"
#include "aa_many_host.h"
#include "aa_pil_coeffs.h"

using namespace aa_coeffs;

namespace {

__device__ inline uint8_t clip8(int32_t a) {  // Pillow's clip8(ss >> PRECISION_BITS)
  a >>= 22;
  return (uint8_t)(a < 0 ? 0 : (a > 255 ? 255 : a));
}

// ---- 1. tables -------------------------------------------------------------------------------------------------------------------------
// One thread per (item, axis, output index): every item has oH + oW of them.  PL: an axis has its m <= o covered indices, the threads
// beyond them idle; entry i is the window of index v0 + i of the item's own size v, at the scale of the whole axis (or box) over v.
template <bool PL>
__global__ void __launch_bounds__(256) many_tables(const AAManyItem *items, const AAManyPlace *places, char *ws, int64_t n, int oH, int oW,
                                                   int filter) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int per = oH + oW;
  if (t >= n * per) return;
  const AAManyItem &it = items[t / per];
  const int r = (int)(t % per);
  const bool vert = r < oH;
  const int i = vert ? r : r - oH;
  int out = vert ? oH : oW;
  int v = out, v0 = 0;
  if (PL) {
    const AAManyPlace &pl = places[t / per];
    out = vert ? pl.mh : pl.mw;
    if (i >= out) return;
    v = vert ? pl.vh : pl.vw;
    v0 = vert ? pl.v0h : pl.v0w;
  }
  const int ksize = vert ? it.ksize_h : it.ksize_w;
  const int hull = vert ? it.hull_h : it.hull_w;
  const BoxArgs bx = {vert ? it.in0_h : it.in0_w, vert ? it.in1_h : it.in1_w, vert ? it.oy : it.ox, it.box_on};
  int32_t *xmin_p = (int32_t *)(ws + (vert ? it.tab_h : it.tab_w));
  int32_t *xsize_p = xmin_p + out;
  int32_t *kk = xsize_p + out + (size_t)i * ksize;
  // (no box: the hull is the whole axis, origin 0, and in / out is the scale — aa_table_build's table)
  // (PL, no box: in1 is the whole axis as a double, so in1 / v is the plain call's in / out)
  const PilWindow wd = PL ? pil_window_at(v0 + i, filter, aa_pil_scale(bx.on, bx.in0, bx.in1, bx.in1, v), bx.in0, bx.origin, bx.origin + hull)
                          : pil_window(i, filter, hull, out, bx);
  xmin_p[i] = wd.xmin - bx.origin;
  xsize_p[i] = wd.xsize;
  pil_weights(wd, filter, ksize, kk);
}

// ---- 2. horizontal pass ------------------------------------------------------------------------------------------------------------------
// E = bytes per pixel of a row (C for interleaved pixels, 1 for a plane).  64 * E lanes: lane j computes byte j of the strip's output, i.e.
// column x0 + j / E, channel j % E.  The input bytes the strip's windows cover are staged into LDS in chunks of up to kChunkBytes with
// dword loads from the dword at or below the segment's first byte (bytes outside the segment are never read: the ragged dwords at both
// ends are assembled from byte loads), so rows at any alignment load coalesced; every lane then adds the taps of its window that lie in
// the chunk.  Integer sums: the order of the taps does not matter.
constexpr int kChunkDwords = 2048;
constexpr int kChunkBytes = 4 * kChunkDwords;

// The four bytes at a4 + 4 i of a staged segment [a, a_end): one dword load where all four lie inside (at any alignment: global memory
// serves an unaligned dword), else assembled from byte loads (bytes outside the segment read as 0 and are never looked at).
__device__ inline uint32_t stage_dword(const uint8_t *a4, const uint8_t *a, const uint8_t *a_end, int i) {
  const uint8_t *p = a4 + 4 * (int64_t)i;
  if (p >= a && p + 4 <= a_end) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
  }
  uint32_t v = 0;
  for (int b = 0; b < 4; b++)
    if (p + b >= a && p + b < a_end) v |= (uint32_t)p[b] << (8 * b);
  return v;
}

// Straight -> premultiplied for the pixels of one dword (aa_alpha.h): two LA pixels; four bytes of a colour plane by the four bytes of
// the alpha plane at the same columns.
__device__ inline uint32_t premul_la2(uint32_t v) {
  return (uint32_t)aa_premul8((int)(v & 255u), (int)((v >> 8) & 255u)) | ((uint32_t)aa_premul8((int)((v >> 16) & 255u), (int)(v >> 24)) << 16) |
         (v & 0xff00ff00u);
}
__device__ inline uint32_t premul_planes4(uint32_t v, uint32_t a) {
  return (uint32_t)aa_premul8((int)(v & 255u), (int)(a & 255u)) | ((uint32_t)aa_premul8((int)((v >> 8) & 255u), (int)((a >> 8) & 255u)) << 8) |
         ((uint32_t)aa_premul8((int)((v >> 16) & 255u), (int)((a >> 16) & 255u)) << 16) | ((uint32_t)aa_premul8((int)(v >> 24), (int)(a >> 24)) << 24);
}

// PL: the item's own strip count, its covered columns [0, mw) of the table, and its own row pitch and lead in the intermediate.
// AL (E = 1, 2, 4; the plan's header says some item has AA_MANY_ITEM_ALPHA): a workgroup of such an item stages its chunk PREMULTIPLIED
// (Pillow's RGBA -> RGBa, LA -> La), once per pixel and in LDS only, so the intermediate holds filtered premultiplied bytes.  Where the
// pixels of the row are aligned to the staged dwords (E = 4: shift 0; E = 2: shift even) the staging lane converts its dword in registers
// on the way in; otherwise the chunk is staged as it lies and converted in place, one lane per pixel with byte accesses, behind one more
// barrier.  A colour plane's staging lane loads, beside its dword, the four alpha bytes of the same columns (plane planes - 1, the same
// row: an unaligned dword load where the two rows are misaligned to each other) and multiplies in registers: no second buffer, no
// barrier.  The alpha plane's own workgroups, and items without the bit, run the plain code.
template <int E, bool PL, bool AL>
__global__ void __launch_bounds__(AA_MANY_STRIP * E) many_hpass(const AAManyItem *items, const AAManyPlace *places, const int64_t *prefix, char *ws,
                                                                int n, int oW, int planes) {
  static_assert(!AL || E == 1 || E == 2 || E == 4, "alpha is the last of 2 or 4 channels");
  __shared__ uint32_t seg[kChunkDwords];
  const int64_t unit = blockIdx.x;
  const int lo = aa_unit_item(prefix, n, unit);
  const AAManyItem &it = items[lo];
  int64_t u = unit - prefix[lo];
  int lead = 0;
  int64_t pitch = aa_many_inter_pitch(oW, E);
  if (PL) {
    const AAManyPlace &pl = places[lo];
    oW = pl.mw;
    lead = aa_many_placed_lead(pl.dx, E);
    pitch = aa_many_placed_pitch(pl.dx, pl.mw, E);
  }
  const int nstrips = (oW + AA_MANY_STRIP - 1) / AA_MANY_STRIP;
  const int strip = (int)(u % nstrips);
  u /= nstrips;
  const int hull_h = it.hull_h, hull_w = it.hull_w;
  const int row = (int)(u % hull_h);
  const int plane = (int)(u / hull_h);
  if (plane >= planes) return;  // (never: the grid is prefix[n]; uniform per workgroup)
  const int x0 = strip * AA_MANY_STRIP;
  const int x1 = x0 + AA_MANY_STRIP < oW ? x0 + AA_MANY_STRIP : oW;
  const AATab<int32_t> tab = aa_tab<int32_t>(ws + it.tab_w, oW, it.ksize_w);
  // window starts and ends do not decrease with the output index: the strip's windows cover [first start, last end)
  int seg0 = tab.xmin[x0], seg1 = tab.xmin[x1 - 1] + tab.xsize[x1 - 1];
  if (seg0 < 0) seg0 = 0;
  if (seg1 > hull_w) seg1 = hull_w;
  const uint8_t *rowp = it.src + (int64_t)plane * it.plane_stride + (int64_t)(it.oy + row) * it.row_stride + (int64_t)it.ox * E;
  // AL: this workgroup premultiplies what it stages; aoff, a colour plane's distance to the same byte of the alpha plane
  const bool al = AL && (it.flags & AA_MANY_ITEM_ALPHA) != 0 && (E > 1 || plane < planes - 1);
  const int64_t aoff = AL && E == 1 ? (int64_t)(planes - 1 - plane) * it.plane_stride : 0;

  const int j = threadIdx.x;
  const int x = x0 + j / E, c = j % E;
  const bool active = x < x1;
  int mx = 0, ms = 0;
  const int32_t *wp = tab.w;
  if (active) {
    mx = tab.xmin[x];
    ms = tab.taps(x);
    wp = tab.row(x);
  }
  int32_t ss = 1 << 21;
  constexpr int kChunkCols = (kChunkBytes - 4) / E;
  const uint8_t *lds = (const uint8_t *)seg;
  for (int c0 = seg0; c0 < seg1; c0 += kChunkCols) {
    const int c1 = c0 + kChunkCols < seg1 ? c0 + kChunkCols : seg1;
    const uint8_t *a = rowp + (int64_t)c0 * E, *a_end = rowp + (int64_t)c1 * E;
    const int shift = (int)((uintptr_t)a & 3);
    const uint8_t *a4 = a - shift;
    const int ndw = (shift + (c1 - c0) * E + 3) >> 2;
    __syncthreads();  // (the previous chunk has been consumed)
    if (AL && al) {  // (uniform per workgroup)
      constexpr int NT = AA_MANY_STRIP * E;
      if (E == 1) {  // (the alpha bytes of a staged dword's columns: aoff further on, at whatever alignment that is)
        for (int i = j; i < ndw; i += NT) seg[i] = premul_planes4(stage_dword(a4, a, a_end, i), stage_dword(a4 + aoff, a + aoff, a_end + aoff, i));
      } else if (shift % E == 0) {  // (every pixel lies within one staged dword)
        for (int i = j; i < ndw; i += NT) {
          const uint32_t v = stage_dword(a4, a, a_end, i);
          seg[i] = E == 4 ? aa_premul_px(v) : premul_la2(v);
        }
      } else {
        for (int i = j; i < ndw; i += NT) seg[i] = stage_dword(a4, a, a_end, i);
        __syncthreads();
        uint8_t *ldsw = (uint8_t *)seg;
        for (int p = j; p < c1 - c0; p += NT) {  // (a lane touches the bytes of its own pixel only)
          const int at = shift + p * E;
          const int av = ldsw[at + E - 1];
          for (int ch = 0; ch < E - 1; ch++) ldsw[at + ch] = (uint8_t)aa_premul8(ldsw[at + ch], av);
        }
      }
    } else {  // (stage_dword, written out as it always was: the instantiations without alpha keep the code they had)
      for (int i = j; i < ndw; i += AA_MANY_STRIP * E) {
        const uint8_t *p = a4 + 4 * (int64_t)i;
        uint32_t v;
        if (p >= a && p + 4 <= a_end) {
          v = *(const uint32_t *)p;
        } else {
          v = 0;
          for (int b = 0; b < 4; b++)
            if (p + b >= a && p + b < a_end) v |= (uint32_t)p[b] << (8 * b);
        }
        seg[i] = v;
      }
    }
    __syncthreads();
    if (active) {
      const int k_lo = (mx > c0 ? mx : c0) - mx;
      const int k_hi = (mx + ms < c1 ? mx + ms : c1) - mx;
      const int at = shift + (mx - c0) * E + c;  // (k >= k_lo keeps the index inside the chunk)
      for (int k = k_lo; k < k_hi; k++) ss += (int32_t)lds[at + k * E] * wp[k];
    }
  }
  if (active) {
    uint8_t *inter = (uint8_t *)ws + it.inter + ((int64_t)plane * hull_h + row) * pitch;
    inter[lead + x0 * E + j] = clip8(ss);
  }
}

// ---- 3. vertical pass --------------------------------------------------------------------------------------------------------------------
// Lane j owns bytes [4j, 4j + 4) of the output row, whatever they are (columns of a plane, channels of interleaved pixels): one aligned
// dword load per tap row of the intermediate (its rows start on a dword), four sums, one dword store where the output address is
// dword-aligned and all four bytes exist, byte stores otherwise.
// The four sums of one lane down the window of entry t of an item's vertical table (`out` entries): tap row k is the dword at byte `at` of
// row r0 + k of the plane's intermediate (rows `pitch` bytes apart), its weight w[t][k].  All three vertical passes are this.
struct Sums4 { int32_t s0, s1, s2, s3; };
__device__ inline Sums4 vtap_sums(const AAManyItem &it, const char *ws, int out, int t, int plane, int64_t pitch, int64_t at) {
  const int32_t *xmin_p = (const int32_t *)(ws + it.tab_h);
  const int32_t *xsize_p = xmin_p + out;
  const int ksize = it.ksize_h;
  const int32_t *wp = xsize_p + out + (size_t)t * ksize;
  int r0 = xmin_p[t], nr = xsize_p[t];
  if (nr > ksize) nr = ksize;
  if (r0 < 0) r0 = 0;
  if (r0 + nr > it.hull_h) nr = it.hull_h - r0;
  const uint8_t *ip = (const uint8_t *)ws + it.inter + ((int64_t)plane * it.hull_h + r0) * pitch + at;
  Sums4 s = {1 << 21, 1 << 21, 1 << 21, 1 << 21};
  for (int k = 0; k < nr; k++) {
    const uint32_t v = *(const uint32_t *)(ip + k * pitch);
    const int32_t wk = wp[k];
    s.s0 += (int32_t)(v & 255u) * wk;
    s.s1 += (int32_t)((v >> 8) & 255u) * wk;
    s.s2 += (int32_t)((v >> 16) & 255u) * wk;
    s.s3 += (int32_t)(v >> 24) * wk;
  }
  return s;
}

// AL, an item with AA_MANY_ITEM_ALPHA: the intermediate holds premultiplied bytes, so the four clipped bytes w of a lane are converted
// back (Pillow's RGBa -> RGBA, La -> LA; aa_alpha.h) with the resampled alpha of their own output pixel: in the lane for interleaved
// pixels (one RGBA pixel, or two LA pixels: a row's bytes start on a dword of the canvas and E divides 4), and for a colour plane from a
// second walk down the same window of the alpha plane, plane planes - 1, at the same columns.  The alpha plane's bytes are final.
__device__ inline uint32_t unpremul_px(uint32_t w) {
  const int a = (int)(w >> 24);
  return (uint32_t)aa_unpremul8((int)(w & 255u), a) | ((uint32_t)aa_unpremul8((int)((w >> 8) & 255u), a) << 8) |
         ((uint32_t)aa_unpremul8((int)((w >> 16) & 255u), a) << 16) | (w & 0xff000000u);
}
__device__ inline uint32_t unpremul_la2(uint32_t w) {
  return (uint32_t)aa_unpremul8((int)(w & 255u), (int)((w >> 8) & 255u)) | ((uint32_t)aa_unpremul8((int)((w >> 16) & 255u), (int)(w >> 24)) << 16) |
         (w & 0xff00ff00u);
}
__device__ inline uint32_t unpremul_planes4(uint32_t w, uint32_t a) {
  return (uint32_t)aa_unpremul8((int)(w & 255u), (int)(a & 255u)) | ((uint32_t)aa_unpremul8((int)((w >> 8) & 255u), (int)((a >> 8) & 255u)) << 8) |
         ((uint32_t)aa_unpremul8((int)((w >> 16) & 255u), (int)((a >> 16) & 255u)) << 16) |
         ((uint32_t)aa_unpremul8((int)(w >> 24), (int)(a >> 24)) << 24);
}
__device__ inline uint32_t straight_bytes(const AAManyItem &it, const char *ws, int out, int t, int plane, int planes, int E, int64_t pitch,
                                          int64_t at, uint32_t w) {
  if (E == 4) return unpremul_px(w);
  if (E == 2) return unpremul_la2(w);
  if (plane == planes - 1) return w;
  const Sums4 a = vtap_sums(it, ws, out, t, planes - 1, pitch, at);
  return unpremul_planes4(w, pack4_clip8(a.s0, a.s1, a.s2, a.s3));
}

// PL, the four bytes [b, b + 4) of canvas row y, packed: a row the item does not cover, or four bytes beside its columns, are the fill and
// read nothing; otherwise the four sums (the dword of the intermediate that holds the canvas dword: its rows are led so), each byte then
// the sum or the fill, because a dword may straddle the item's edge.  What the dword holds beyond the covered columns lies inside the
// item's own rows of the intermediate and is not used.  AL: the sums' bytes are converted before the fill is mixed in, so in a dword
// that holds a fill pixel and an item pixel (LA at an odd dx) only the item's is converted; the fill is written as given.
template <bool AL>
__device__ inline uint32_t placed_bytes(const AAManyItem &it, const AAManyPlace &pl, const char *ws, uint32_t fill, int plane, int planes, int E, int y,
                                        int b) {
  uint32_t fw = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) fw |= ((fill >> (8 * (E == 1 ? plane : (b + q) % E))) & 255u) << (8 * q);
  const int ty = y - pl.dy;
  const int cb0 = pl.dx * E, cb1 = cb0 + pl.mw * E;  // the covered bytes of a canvas row
  if (ty < 0 || ty >= pl.mh || b + 4 <= cb0 || b >= cb1) return fw;
  const int64_t pitch = aa_many_placed_pitch(pl.dx, pl.mw, E);
  const Sums4 s = vtap_sums(it, ws, pl.mh, ty, plane, pitch, b - (cb0 & ~3));
  uint32_t sw = pack4_clip8(s.s0, s.s1, s.s2, s.s3);  // (`clip8(a) | clip8(b) << 8 ...` of one word is what hipcc miscompiles: aa_common.h)
  if (AL && (it.flags & AA_MANY_ITEM_ALPHA)) sw = straight_bytes(it, ws, pl.mh, ty, plane, planes, E, pitch, b - (cb0 & ~3), sw);
  uint32_t mask = 0;
#pragma unroll
  for (int q = 0; q < 4; q++)
    if (b + q >= cb0 && b + q < cb1) mask |= 255u << (8 * q);
  return (sw & mask) | (fw & ~mask);
}

template <bool PL, bool AL>
__global__ void __launch_bounds__(256) many_vpass(const AAManyItem *items, const AAManyPlace *places, const char *ws, uint8_t *out, int oH, int oW,
                                                  int planes, int E, int nstrips, uint32_t fill) {
  int64_t u = blockIdx.x;
  const int strip = (int)(u % nstrips);
  u /= nstrips;
  const int y = (int)(u % oH);
  u /= oH;
  const int plane = (int)(u % planes);
  const AAManyItem &it = items[u / planes];
  const int rowbytes = oW * E;
  const int b = (strip * 256 + (int)threadIdx.x) * 4;
  if (b >= rowbytes) return;
  uint32_t r0b, r1b, r2b, r3b;
  if (PL) {
    const uint32_t w = placed_bytes<AL>(it, places[u / planes], ws, fill, plane, planes, E, y, b);
    r0b = w & 255u; r1b = (w >> 8) & 255u; r2b = (w >> 16) & 255u; r3b = w >> 24;
  } else if (AL && (it.flags & AA_MANY_ITEM_ALPHA)) {
    const int64_t pitch = aa_many_inter_pitch(oW, E);
    const Sums4 s = vtap_sums(it, ws, oH, y, plane, pitch, b);
    const uint32_t w = straight_bytes(it, ws, oH, y, plane, planes, E, pitch, b, pack4_clip8(s.s0, s.s1, s.s2, s.s3));
    r0b = w & 255u; r1b = (w >> 8) & 255u; r2b = (w >> 16) & 255u; r3b = w >> 24;
  } else {
    const Sums4 s = vtap_sums(it, ws, oH, y, plane, aa_many_inter_pitch(oW, E), b);
    r0b = clip8(s.s0); r1b = clip8(s.s1); r2b = clip8(s.s2); r3b = clip8(s.s3);  // (this form hipcc does not turn into the packed shift: aa_common.h)
  }
  uint8_t *op = out + (((int64_t)(u / planes) * planes + plane) * oH + y) * rowbytes + b;
  const int nb = rowbytes - b < 4 ? rowbytes - b : 4;
  if (nb == 4 && ((uintptr_t)op & 3) == 0) {
    *(uint32_t *)op = r0b | (r1b << 8) | (r2b << 16) | (r3b << 24);
  } else {
    op[0] = (uint8_t)r0b;
    if (nb > 1) op[1] = (uint8_t)r1b;
    if (nb > 2) op[2] = (uint8_t)r2b;
    if (nb > 3) op[3] = (uint8_t)r3b;
  }
}


// ---- 3b. converting vertical pass --------------------------------------------------------------------------------------------------------
// The bytes of many_vpass (same tables, same intermediate, same integer sums), converted as they leave: element = (T)(((float)byte -
// mean[c]) / std[c]), at column oW - 1 - x of an item that flips, in the class's own layout or the other one (XL).
// A workgroup owns kVPixels<E> pixels of one output row of one plane: lane j the bytes [4j, 4j + 4) of that piece, as in many_vpass.
// Every lane stores its four results where they belong, one element each (an element store is always aligned: the entry point checks the
// output's address against its element), so rows at any element alignment, flips and both output layouts are one code path.  From
// interleaved pixels to planes a store instruction of a wave then covers E planes with short runs; a form that staged the workgroup's
// results in LDS and stored aligned 8- / 16-byte pieces of one plane row per lane measured 5 % slower on that case.
struct ManyConvert { int normalize; float mean[4], std[4]; };  // (the element types and to_elem: aa_many_dev.h)
__device__ inline float pick4(const float (&a)[4], int c) { return c == 0 ? a[0] : (c == 1 ? a[1] : (c == 2 ? a[2] : a[3])); }

template <int E> constexpr int kVLanes = E == 3 ? 192 : 256;   // lanes of a workgroup: 4 bytes each, a whole number of pixels together
template <int E> constexpr int kVPixels = kVLanes<E> * 4 / E;  // 1024, 512, 256, 256

template <typename T, int E, bool XL, bool PL, bool AL>
__global__ void __launch_bounds__(kVLanes<E>) many_vpass_float(const AAManyItem *items, const AAManyPlace *places, const char *ws, T *out, int oH,
                                                               int oW, int planes, int nstrips, const ManyConvert cv, uint32_t fill) {
  constexpr int PX = kVPixels<E>;
  int64_t u = blockIdx.x;
  const int strip = (int)(u % nstrips);
  u /= nstrips;
  const int y = (int)(u % oH);
  u /= oH;
  const int plane = (int)(u % planes);
  const int64_t n = u / planes;
  const AAManyItem &it = items[n];
  const int x0 = strip * PX;
  const int npx = oW - x0 < PX ? oW - x0 : PX;
  const int j = threadIdx.x;
  const int nb = npx * E - 4 * j;  // bytes of the piece from this lane's first (4 or more: all four results exist; <= 0: none)
  if (nb <= 0) return;
  const bool flip = (it.flags & AA_MANY_ITEM_FLIP) != 0;
  const int xr = flip ? oW - x0 - npx : x0;  // the output column the piece's run(s) start at

  float f[4];
  if (PL) {  // (the piece starts on a dword of the canvas row: kVPixels<E> * E is a multiple of 4)
    const uint32_t w = placed_bytes<AL>(it, places[n], ws, fill, plane, planes, E, y, x0 * E + 4 * j);
    f[0] = (float)(w & 255u); f[1] = (float)((w >> 8) & 255u); f[2] = (float)((w >> 16) & 255u); f[3] = (float)(w >> 24);
  } else if (AL && (it.flags & AA_MANY_ITEM_ALPHA)) {
    const int64_t pitch = aa_many_inter_pitch(oW, E), at = (int64_t)x0 * E + 4 * j;
    const Sums4 s = vtap_sums(it, ws, oH, y, plane, pitch, at);
    const uint32_t w = straight_bytes(it, ws, oH, y, plane, planes, E, pitch, at, pack4_clip8(s.s0, s.s1, s.s2, s.s3));
    f[0] = (float)(w & 255u); f[1] = (float)((w >> 8) & 255u); f[2] = (float)((w >> 16) & 255u); f[3] = (float)(w >> 24);
  } else {
    const Sums4 s = vtap_sums(it, ws, oH, y, plane, aa_many_inter_pitch(oW, E), (int64_t)x0 * E + 4 * j);
    f[0] = (float)clip8(s.s0); f[1] = (float)clip8(s.s1); f[2] = (float)clip8(s.s2); f[3] = (float)clip8(s.s3);
  }

#pragma unroll
  for (int i = 0; i < 4; i++) {
    if (i >= nb) break;
    const int q = 4 * j + i, px = q / E, c = q % E;
    float v = f[i];
    if (cv.normalize) v = (v - pick4(cv.mean, plane + c)) / pick4(cv.std, plane + c);  // (one of plane and c is 0)
    const int64_t x = xr + (flip ? npx - 1 - px : px);
    int64_t at;
    if (!XL) at = (((n * planes + plane) * oH + y) * oW + x) * E + c;
    else if (E > 1) at = ((n * E + c) * oH + y) * oW + x;
    else at = ((n * oH + y) * oW + x) * planes + plane;
    out[at] = to_elem<T>(v);
  }
}

// ---- 3c. patch-writing vertical pass -------------------------------------------------------------------------------------------------------
// A patch plan (aa_many.h): item i is the whole of its own [vh, vw] canvas, cut into gh x gw patches of ph x pw pixels; token t = gy * gw +
// gx of the item is row tok0[i] + t of the [rows, D] output, D = C * ph * pw.  The grid is ragged like the horizontal pass's: one
// workgroup per unit, its item found by binary search in vunit_prefix.  An IMAGE unit is many_vpass_float's (plane, row y, strip of
// kVPixels<E> pixels) within the item's own size: the same bytes from placed_bytes, the same conversion, the same mirrored column for an
// item that flips; only the address of the store differs.  Pixel (channel ch, y, x) goes to row tok0 + (y / ph) * gw + x / pw, column
//   (ch * ph + y % ph) * pw + x % pw        token vector [C, ph, pw]  (PPC false)
//   ((y % ph) * pw + x % pw) * C + ch       token vector [ph, pw, C]  (PPC true)
// so a store instruction of a wave writes runs of pw elements (planes, [C, ph, pw]), pw * C elements (interleaved pixels, [ph, pw, C]) or
// single elements C or ph * pw apart (the two crossed combinations), each run in another token row.  A PAD unit (pad_to > 0) zeroes
// AA_MANY_PAD_ELEMS elements of the item's rows [T_i, pad_to), which are contiguous: consecutive lanes, consecutive elements.
template <typename T, int E, bool PPC>
__global__ void __launch_bounds__(kVLanes<E>) many_vpass_patches(const AAManyItem *items, const AAManyPlace *places, const int64_t *vprefix,
                                                                 const int64_t *tok0, const char *ws, T *out, int n, int planes, int ph, int pw,
                                                                 int64_t pad_to, const ManyConvert cv) {
  constexpr int PX = kVPixels<E>;
  static_assert(PX * E == kVLanes<E> * 4 && PX == aa_many_vpixels(E), "a strip is four bytes per lane, and the planner counts the same strips");
  const int64_t unit = blockIdx.x;
  const int lo = aa_unit_item(vprefix, n, unit);
  const AAManyItem &it = items[lo];
  const AAManyPlace &pl = places[lo];
  int64_t u = unit - vprefix[lo];
  const int vh = pl.vh, vw = pl.vw, gw = vw / pw;
  const int C = planes * E;  // (one of the two is 1)
  const int64_t D = (int64_t)C * ph * pw;
  const int nstrips = (vw + PX - 1) / PX;
  const int64_t image_units = (int64_t)planes * vh * nstrips;
  const int j = threadIdx.x;
  if (u >= image_units) {  // (uniform per workgroup)
    const int64_t tokens = (int64_t)(vh / ph) * gw;
    const int64_t e0 = (u - image_units) * AA_MANY_PAD_ELEMS;
    const int64_t left = (pad_to - tokens) * D - e0;
    const int cnt = left < AA_MANY_PAD_ELEMS ? (int)left : AA_MANY_PAD_ELEMS;
    T *p = out + (tok0[lo] + tokens) * D + e0;
    const T zero = T();
    for (int k = j; k < cnt; k += kVLanes<E>) p[k] = zero;
    return;
  }
  const int strip = (int)(u % nstrips);
  u /= nstrips;
  const int y = (int)(u % vh);
  const int plane = (int)(u / vh);
  const int x0 = strip * PX;
  const int npx = vw - x0 < PX ? vw - x0 : PX;
  const int nb = npx * E - 4 * j;  // bytes of the piece from this lane's first (4 or more: all four results exist; <= 0: none)
  if (nb <= 0) return;
  const bool flip = (it.flags & AA_MANY_ITEM_FLIP) != 0;

  const uint32_t w = placed_bytes<false>(it, pl, ws, 0u, plane, planes, E, y, x0 * E + 4 * j);  // (the item covers its canvas: never the fill)
  const float f[4] = {(float)(w & 255u), (float)((w >> 8) & 255u), (float)((w >> 16) & 255u), (float)(w >> 24)};

  const int gy = y / ph, py = y - gy * ph;
  const int64_t row0 = tok0[lo] + (int64_t)gy * gw;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if (i >= nb) break;
    const int q = 4 * j + i, px = q / E, c = q % E;
    float v = f[i];
    if (cv.normalize) v = (v - pick4(cv.mean, plane + c)) / pick4(cv.std, plane + c);  // (one of plane and c is 0)
    const int x = flip ? vw - 1 - (x0 + px) : x0 + px;
    const int gx = x / pw, qx = x - gx * pw;
    const int64_t col = PPC ? (int64_t)(py * pw + qx) * C + (plane + c) : ((int64_t)(plane + c) * ph + py) * pw + qx;
    out[(row0 + gx) * D + col] = to_elem<T>(v);
  }
}

}  // namespace

// ---- host: the planner -------------------------------------------------------------------------------------------------------------------
size_t aa_many_desc_size(int64_t n) { return aa_desc_size(sizeof(AAManyHeader), sizeof(AAManyItem), n); }

size_t aa_many_desc_size_placed(int64_t n) {
  if (n < 0) return 0;
  return aa_many_desc_size(n) + (size_t)n * sizeof(AAManyPlace);
}

size_t aa_many_desc_size_patches(int64_t n) {
  if (n < 0) return 0;
  return aa_many_desc_size_placed(n) + 2 * ((size_t)n + 1) * sizeof(int64_t) + sizeof(AAManyPatchInfo);
}

// The hull [o, e) of the outputs [v0, v1) of an axis resized to out_size: the window start of v0 and the window end of v1 - 1, each
// clipped to the axis (boxmath.axis_hull; the same window the table kernel evaluates).  The scale comes from the whole axis (or the box)
// over the whole out_size, whatever part of the outputs is asked for.
static void axis_hull(int filter, int64_t in_size, int64_t out_size, double in0, double in1, int on, int64_t v0, int64_t v1, int64_t *o, int64_t *e) {
  const BoxArgs bx = {in0, in1, 0, on};
  const PilWindow first = pil_window((int)v0, filter, (int)in_size, (int)out_size, bx);
  const PilWindow last = pil_window((int)v1 - 1, filter, (int)in_size, (int)out_size, bx);
  *o = first.xmin;
  *e = (int64_t)last.xmin + last.xsize;
}

// own_canvas: a patch plan.  Every place is the whole of its item's own canvas, [oH, oW] is only the largest of them: the plan is a
// placed one whatever the places (the patch pass reads the records), and there is no dense vertical grid to bound.
static int many_plan(int filter, int layout, int64_t n, int64_t C, int64_t oH, int64_t oW, const aa_many_image *images, const aa_many_place *places,
                     const uint8_t *fill, bool own_canvas, void *desc_host, size_t desc_bytes, size_t *workspace_bytes) {
  if (!aa_filter_valid(filter)) return AA_ERR_BAD_FILTER;
  if (layout != AA_NCHW && layout != AA_NHWC) return AA_ERR_BAD_LAYOUT;
  const int rc0 = aa_many_check_canvas(n, kAAManyMax, C >= 1 && C <= 4, oH, oW, desc_host, workspace_bytes, images, places);
  if (rc0 != AA_OK) return rc0;
  bool placed = own_canvas;  // every item the whole canvas at offset 0 is the plain plan: nothing of the canvas is left to the fill
  for (int64_t i = 0; places && i < n; i++) placed = placed || places[i].vH != oH || places[i].vW != oW || places[i].oy != 0 || places[i].ox != 0;
  if (desc_bytes < (placed ? aa_many_desc_size_placed(n) : aa_many_desc_size(n))) return AA_ERR_WORKSPACE;
  const int E = layout == AA_NHWC ? (int)C : 1;
  const int64_t planes = layout == AA_NHWC ? 1 : C;
  const int64_t pitch = aa_many_inter_pitch(oW, E);
  const int64_t nstrips = (oW + AA_MANY_STRIP - 1) / AA_MANY_STRIP;
  const int64_t vstrips = (oW * E + AA_MANY_VBYTES - 1) / AA_MANY_VBYTES;
  if ((!own_canvas && n * planes * oH * vstrips > INT32_MAX) || n * (oH + oW) > (int64_t)INT32_MAX * 256) return AA_ERR_BAD_SHAPE;  // (grids of the launches)

  AAManyHeader *hd = (AAManyHeader *)desc_host;
  AAManyItem *items = (AAManyItem *)(hd + 1);
  int64_t *prefix = (int64_t *)(items + n);
  AAManyPlace *pls = (AAManyPlace *)(prefix + n + 1);  // (a placed plan only)
  size_t off = 0;  // the arena first, then the intermediates
  int64_t units = 0;
  int flips = 0, alphas = 0;
  // (straight alpha is the last of 2 or 4 channels, and a patch plan has none)
  const int allowed_flags = AA_MANY_FLIP_X | (!own_canvas && (C == 2 || C == 4) ? AA_MANY_PREMUL_ALPHA : 0);
  const aa_many_place whole = {oH, oW, 0, 0};
  for (int64_t i = 0; i < n; i++) {
    const aa_many_image &im = images[i];
    AAManyItem it;
    memset(&it, 0, sizeof(it));
    AAManyBox bx;
    const int rc = aa_many_check_image_box(im, (im.flags & ~allowed_flags) == 0, layout, C, 1, C, &bx);
    if (rc != AA_OK) return rc;
    // the item's own output size and the part [v0, v0 + m) of it that lies on the canvas, per axis (plain: all of the canvas)
    const AAManyPlace pl = aa_many_cover(placed ? places[i] : whole, oH, oW);
    if (placed) pls[i] = pl;
    const int64_t vH = pl.vh, vW = pl.vw, v0h = pl.v0h, v0w = pl.v0w, mh = pl.mh, mw = pl.mw;  // (off the canvas: no table, no work unit)
    int64_t oy = 0, ey = 0, ox = 0, ex = 0;
    int kh = 0, kw = 0;
    if (mh > 0) {
      axis_hull(filter, im.H, vH, bx.y0, bx.y1, bx.on, v0h, v0h + mh, &oy, &ey);
      axis_hull(filter, im.W, vW, bx.x0, bx.x1, bx.on, v0w, v0w + mw, &ox, &ex);
      if (ey <= oy || ex <= ox) return AA_ERR_BAD_SHAPE;
      kh = bx.on ? aa_table_ksize_box(filter, AA_TABLE_PIL, ey - oy, vH, bx.y0, bx.y1) : aa_table_ksize(filter, AA_TABLE_PIL, im.H, vH, 0, 0.0);
      if (kh < 0) return kh;
      kw = bx.on ? aa_table_ksize_box(filter, AA_TABLE_PIL, ex - ox, vW, bx.x0, bx.x1) : aa_table_ksize(filter, AA_TABLE_PIL, im.W, vW, 0, 0.0);
      if (kw < 0) return kw;
    }
    it.src = (const uint8_t *)im.data_dev;
    it.row_stride = im.stride_row;
    it.plane_stride = layout == AA_NHWC ? 0 : (C > 1 ? im.stride_ch : 0);
    it.in0_h = bx.y0; it.in1_h = bx.y1; it.in0_w = bx.x0; it.in1_w = bx.x1;
    it.oy = (int32_t)oy; it.hull_h = (int32_t)(ey - oy); it.ox = (int32_t)ox; it.hull_w = (int32_t)(ex - ox);
    it.ksize_h = kh; it.ksize_w = kw;
    it.box_on = bx.on;
    it.flags = im.flags & AA_MANY_ITEM_FLIP;
    flips |= it.flags;
    // Image.resize returns self.copy() before it looks at the mode where the size asked for is the image's and the box is the whole
    // image: such an item is never premultiplied (the round trip loses colour at low alpha); its windows are one tap of weight 1
    if ((im.flags & AA_MANY_PREMUL_ALPHA) && !(bx.on == 0 && vH == im.H && vW == im.W)) {
      it.flags |= AA_MANY_ITEM_ALPHA;
      alphas = 1;
    }
    it.tab_h = (int64_t)off;
    off += aa_many_table_bytes(mh, kh);
    it.tab_w = (int64_t)off;
    off += aa_many_table_bytes(mw, kw);
    prefix[i] = units;
    units += planes * (ey - oy) * (placed ? (mw + AA_MANY_STRIP - 1) / AA_MANY_STRIP : nstrips);
    if (units > INT32_MAX) return AA_ERR_BAD_SHAPE;  // (one grid)
    items[i] = it;
  }
  prefix[n] = units;
  for (int64_t i = 0; i < n; i++) {
    items[i].inter = (int64_t)off;
    off += aa_align16((size_t)(planes * items[i].hull_h * (placed ? aa_many_placed_pitch(pls[i].dx, pls[i].mw, E) : pitch)));
  }
  memset(hd, 0, sizeof(*hd));
  hd->magic = AA_MANY_MAGIC;
  hd->n = (int32_t)n; hd->C = (int32_t)C; hd->oH = (int32_t)oH; hd->oW = (int32_t)oW;
  hd->filter = filter; hd->layout = layout;
  hd->flips = flips;
  hd->hunits = units;
  hd->ws_bytes = (int64_t)off;
  if (placed) {
    hd->kind = AA_MANY_PLAN_PLACED;
    for (int c = 0; fill && c < 4; c++) hd->fill |= (int64_t)fill[c] << (8 * c);
  }
  if (alphas) hd->kind |= AA_MANY_PLAN_ALPHA;
  *workspace_bytes = off;
  return AA_OK;
}

int aa_many_plan_host(int filter, int layout, int64_t n, int64_t C, int64_t oH, int64_t oW, const aa_many_image *images,
                      const aa_many_place *places, const uint8_t *fill, void *desc_host, size_t desc_bytes, size_t *workspace_bytes) {
  return many_plan(filter, layout, n, C, oH, oW, images, places, fill, false, desc_host, desc_bytes, workspace_bytes);
}

// The tail of a patch plan's block: vunit_prefix[n + 1], tok0[n + 1], AAManyPatchInfo.
static int64_t *patch_tail(const void *desc, int64_t n) { return (int64_t *)((char *)desc + aa_many_desc_size_placed(n)); }

int aa_many_plan_patches_host(int filter, int layout, int64_t n, int64_t C, int64_t ph, int64_t pw, const aa_many_image *images, const int64_t *sizes,
                              int64_t pad_to, void *desc_host, size_t desc_bytes, size_t *workspace_bytes, int64_t *rows) {
  const int64_t kMax = kAAManyMax;
  if (layout != AA_NCHW && layout != AA_NHWC) return AA_ERR_BAD_LAYOUT;
  if (n < 0 || n > kMax || C < 1 || C > 4 || ph < 1 || pw < 1 || ph > kMax || pw > kMax || pad_to < 0 || pad_to > INT32_MAX) return AA_ERR_BAD_SHAPE;
  if (!desc_host || !workspace_bytes || !rows || (n > 0 && (!images || !sizes))) return AA_ERR_NULL;
  if (desc_bytes < aa_many_desc_size_patches(n)) return AA_ERR_WORKSPACE;
  const int E = layout == AA_NHWC ? (int)C : 1;
  const int64_t planes = layout == AA_NHWC ? 1 : C;
  const int64_t D = C * ph * pw;
  if (D > INT32_MAX) return AA_ERR_BAD_SHAPE;
  int64_t *vprefix = patch_tail(desc_host, n), *tok0 = vprefix + n + 1;
  // (the tail first: the placed plan below does not touch these bytes)
  aa_many_place *places = n ? new aa_many_place[(size_t)n] : nullptr;
  int64_t oH = 1, oW = 1, units = 0, row = 0;
  int rc = AA_OK;
  for (int64_t i = 0; i < n; i++) {
    const int64_t vH = sizes[2 * i], vW = sizes[2 * i + 1];
    if (vH <= 0 || vW <= 0 || vH > kMax || vW > kMax || vH % ph || vW % pw) { rc = AA_ERR_BAD_SHAPE; break; }
    const int64_t tokens = (vH / ph) * (vW / pw);
    if (pad_to && tokens > pad_to) { rc = AA_ERR_BAD_SHAPE; break; }
    const aa_many_place p = {vH, vW, 0, 0};
    places[i] = p;
    oH = vH > oH ? vH : oH;
    oW = vW > oW ? vW : oW;
    vprefix[i] = units;
    tok0[i] = pad_to ? i * pad_to : row;
    row += tokens;
    units += planes * vH * ((vW + aa_many_vpixels(E) - 1) / aa_many_vpixels(E));
    if (pad_to) units += ((pad_to - tokens) * D + AA_MANY_PAD_ELEMS - 1) / AA_MANY_PAD_ELEMS;
    if (units > INT32_MAX) { rc = AA_ERR_BAD_SHAPE; break; }  // (one grid)
  }
  vprefix[n] = units;
  tok0[n] = pad_to ? n * pad_to : row;
  if (rc == AA_OK) rc = many_plan(filter, layout, n, C, oH, oW, images, places, nullptr, true, desc_host, desc_bytes, workspace_bytes);
  delete[] places;
  if (rc != AA_OK) return rc;
  AAManyHeader *hd = (AAManyHeader *)desc_host;
  hd->kind |= AA_MANY_PLAN_PATCHES;
  AAManyPatchInfo *info = (AAManyPatchInfo *)(tok0 + n + 1);
  info->ph = (int32_t)ph; info->pw = (int32_t)pw; info->pad_to = pad_to;
  *rows = tok0[n];
  return AA_OK;
}

// ---- host: the three launches ------------------------------------------------------------------------------------------------------------
// The checks of both entry points against the plan; the tables and the horizontal pass, which both share.
static int many_check(const AAManyHeader *hd, const void *desc_dev, int64_t n, int64_t C, int64_t oH, int64_t oW, int layout,
                      const void *workspace_dev, size_t workspace_bytes) {
  if (hd->magic != AA_MANY_MAGIC || hd->n != n || hd->C != C || hd->oH != oH || hd->oW != oW || hd->layout != layout) return AA_ERR_BAD_SHAPE;
  if (n == 0) return AA_OK;
  if (workspace_bytes < (size_t)hd->ws_bytes) return AA_ERR_WORKSPACE;
  if (((uintptr_t)workspace_dev & 15) || ((uintptr_t)desc_dev & 7)) return AA_ERR_BAD_SHAPE;
  return AA_OK;
}

// Some item of the plan is resampled premultiplied (AA_MANY_ITEM_ALPHA): the AL instantiations.  The planner sets the bit for
// C = 2 or 4 only.
static bool many_alpha(const AAManyHeader *hd) { return (hd->kind & AA_MANY_PLAN_ALPHA) != 0 && (hd->C == 2 || hd->C == 4); }

// What the launches take from a checked plan: the bytes per pixel of a row and the planes of its class, and the device copy's records
// (the placement records follow the prefix sums: a placed plan only, else null).
struct ManyViews {
  int E, planes;
  const AAManyItem *items;
  const int64_t *prefix;
  const AAManyPlace *places;
};
static ManyViews many_views(const AAManyHeader *hd, const void *desc_dev) {
  const AADescView<AAManyItem> v = aa_desc_view<AAManyHeader, AAManyItem>(desc_dev, hd->n);
  const bool nhwc = hd->layout == AA_NHWC;
  return {nhwc ? hd->C : 1, nhwc ? 1 : hd->C, v.items, v.prefix,
          (hd->kind & AA_MANY_PLAN_PLACED) ? (const AAManyPlace *)(v.prefix + hd->n + 1) : nullptr};
}

template <int E, bool PL, bool AL>
static void launch_hpass(const AAManyHeader *hd, const ManyViews &v, char *ws, int64_t oW, hipStream_t stream) {
  if (hd->hunits == 0) return;  // (a placed plan whose items all lie off the canvas)
  hipLaunchKernelGGL((many_hpass<E, PL, AL>), dim3((unsigned)hd->hunits), dim3(AA_MANY_STRIP * E), 0, stream, v.items, v.places, v.prefix, ws, (int)hd->n,
                     (int)oW, v.planes);
}

template <bool PL>
static void launch_many_tables_hpass(const AAManyHeader *hd, const ManyViews &v, char *ws, int64_t oH, int64_t oW, hipStream_t stream) {
  const int64_t n = hd->n, tthreads = n * (oH + oW);
  hipLaunchKernelGGL(many_tables<PL>, dim3((unsigned)((tthreads + 255) / 256)), dim3(256), 0, stream, v.items, v.places, ws, n, (int)oH, (int)oW,
                     hd->filter);
  if (many_alpha(hd)) {  // (C is 2 or 4: E is 1, 2 or 4)
    switch (v.E) {
      case 1: launch_hpass<1, PL, true>(hd, v, ws, oW, stream); break;
      case 2: launch_hpass<2, PL, true>(hd, v, ws, oW, stream); break;
      default: launch_hpass<4, PL, true>(hd, v, ws, oW, stream); break;
    }
    return;
  }
  switch (v.E) {
    case 1: launch_hpass<1, PL, false>(hd, v, ws, oW, stream); break;
    case 2: launch_hpass<2, PL, false>(hd, v, ws, oW, stream); break;
    case 3: launch_hpass<3, PL, false>(hd, v, ws, oW, stream); break;
    default: launch_hpass<4, PL, false>(hd, v, ws, oW, stream); break;
  }
}

int aa_launch_many_u8(const void *desc_host, const void *desc_dev, int64_t n, int64_t C, int64_t oH, int64_t oW, int layout, void *out_dev,
                      void *workspace_dev, size_t workspace_bytes, hipStream_t stream) {
  const AAManyHeader *hd = (const AAManyHeader *)desc_host;
  const int rc = many_check(hd, desc_dev, n, C, oH, oW, layout, workspace_dev, workspace_bytes);
  if (rc != AA_OK) return rc;
  if (hd->flips) return AA_ERR_BAD_SHAPE;  // an item flips: the uint8 pass does not
  if (n == 0) return AA_OK;
  const ManyViews v = many_views(hd, desc_dev);
  const int E = v.E, planes = v.planes;
  char *ws = (char *)workspace_dev;
  const int vstrips = (int)((oW * E + AA_MANY_VBYTES - 1) / AA_MANY_VBYTES);
  const dim3 vgrid((unsigned)(n * planes * oH * vstrips));
  const bool al = many_alpha(hd);
  if (v.places) {
    launch_many_tables_hpass<true>(hd, v, ws, oH, oW, stream);
    hipLaunchKernelGGL((al ? many_vpass<true, true> : many_vpass<true, false>), vgrid, dim3(256), 0, stream, v.items, v.places, (const char *)ws,
                       (uint8_t *)out_dev, (int)oH, (int)oW, planes, E, vstrips, (uint32_t)hd->fill);
  } else {
    launch_many_tables_hpass<false>(hd, v, ws, oH, oW, stream);
    hipLaunchKernelGGL((al ? many_vpass<false, true> : many_vpass<false, false>), vgrid, dim3(256), 0, stream, v.items, v.places, (const char *)ws,
                       (uint8_t *)out_dev, (int)oH, (int)oW, planes, E, vstrips, 0u);
  }
  AA_HIP_CHECK_LAUNCH();
  return AA_OK;
}

// The conversion of both converting passes: no normalisation is mean 0, std 1, never read.
static ManyConvert many_convert(int normalize, const float *mean, const float *std, int64_t C) {
  ManyConvert cv;
  cv.normalize = normalize ? 1 : 0;
  for (int i = 0; i < 4; i++) { cv.mean[i] = normalize && i < C ? mean[i] : 0.f; cv.std[i] = normalize && i < C ? std[i] : 1.f; }
  return cv;
}

// What the converting pass is launched with besides its template arguments.
struct ManyFloatArgs {
  const AAManyItem *items;
  const AAManyPlace *places;  // null: a plain plan
  const char *ws;
  void *out;
  int64_t n, oH, oW;
  int planes;
  ManyConvert cv;
  uint32_t fill;
  bool alpha;  // many_alpha() of the plan
  hipStream_t stream;
};

template <typename T, int E, bool XL, bool AL>
static void launch_vpass_float_al(const ManyFloatArgs &a) {
  const int nstrips = (int)((a.oW + kVPixels<E> - 1) / kVPixels<E>);
  const dim3 grid((unsigned)(a.n * a.planes * a.oH * nstrips));
  if (a.places)
    hipLaunchKernelGGL((many_vpass_float<T, E, XL, true, AL>), grid, dim3(kVLanes<E>), 0, a.stream, a.items, a.places, a.ws, (T *)a.out, (int)a.oH,
                       (int)a.oW, a.planes, nstrips, a.cv, a.fill);
  else
    hipLaunchKernelGGL((many_vpass_float<T, E, XL, false, AL>), grid, dim3(kVLanes<E>), 0, a.stream, a.items, a.places, a.ws, (T *)a.out, (int)a.oH,
                       (int)a.oW, a.planes, nstrips, a.cv, 0u);
}

template <typename T, int E, bool XL>
static void launch_vpass_float(const ManyFloatArgs &a) {
  if constexpr (E != 3) {
    if (a.alpha) return launch_vpass_float_al<T, E, XL, true>(a);
  }
  launch_vpass_float_al<T, E, XL, false>(a);
}

template <typename T>
static void launch_vpass_float_e(int E, bool xl, const ManyFloatArgs &a) {
  switch (E * 2 + (xl ? 1 : 0)) {
    case 2: launch_vpass_float<T, 1, false>(a); break;
    case 3: launch_vpass_float<T, 1, true>(a); break;
    case 4: launch_vpass_float<T, 2, false>(a); break;
    case 5: launch_vpass_float<T, 2, true>(a); break;
    case 6: launch_vpass_float<T, 3, false>(a); break;
    case 7: launch_vpass_float<T, 3, true>(a); break;
    case 8: launch_vpass_float<T, 4, false>(a); break;
    default: launch_vpass_float<T, 4, true>(a); break;
  }
}

int aa_launch_many_float(const void *desc_host, const void *desc_dev, int64_t n, int64_t C, int64_t oH, int64_t oW, int layout, void *out_dev,
                         void *workspace_dev, size_t workspace_bytes, int out_elem, int out_layout, int normalize, const float *mean,
                         const float *std, hipStream_t stream) {
  const AAManyHeader *hd = (const AAManyHeader *)desc_host;
  const int rc = many_check(hd, desc_dev, n, C, oH, oW, layout, workspace_dev, workspace_bytes);
  if (rc != AA_OK) return rc;
  if ((uintptr_t)out_dev & (out_elem == AA_F32 ? 3 : 1)) return AA_ERR_BAD_SHAPE;
  if (n == 0) return AA_OK;
  const ManyViews v = many_views(hd, desc_dev);
  const int E = v.E, planes = v.planes;
  const bool xl = out_layout != layout && C > 1;  // (one channel: the two layouts are the same bytes)
  const int64_t px = E == 1 ? kVPixels<1> : (E == 2 ? kVPixels<2> : kVPixels<4>);
  if (n * planes * oH * ((oW + px - 1) / px) > INT32_MAX) return AA_ERR_BAD_SHAPE;  // (the grid of the converting pass)
  char *ws = (char *)workspace_dev;
  if (v.places) launch_many_tables_hpass<true>(hd, v, ws, oH, oW, stream);
  else launch_many_tables_hpass<false>(hd, v, ws, oH, oW, stream);
  const ManyFloatArgs a = {v.items, v.places, ws, out_dev, n, oH, oW, planes, many_convert(normalize, mean, std, C), (uint32_t)hd->fill,
                           many_alpha(hd), stream};
  if (out_elem == AA_F16) launch_vpass_float_e<f16_t>(E, xl, a);
  else if (out_elem == AA_BF16) launch_vpass_float_e<bf16_t>(E, xl, a);
  else launch_vpass_float_e<float>(E, xl, a);
  AA_HIP_CHECK_LAUNCH();
  return AA_OK;
}

// ---- host: the patch plan's three launches ---------------------------------------------------------------------------------------------------
struct ManyPatchArgs {
  const AAManyItem *items;
  const AAManyPlace *places;
  const int64_t *vprefix, *tok0;
  const char *ws;
  void *out;
  int n, planes, ph, pw;
  int64_t pad_to, vunits;
  ManyConvert cv;
  hipStream_t stream;
};

template <typename T, int E, bool PPC>
static void launch_vpass_patches(const ManyPatchArgs &a) {
  hipLaunchKernelGGL((many_vpass_patches<T, E, PPC>), dim3((unsigned)a.vunits), dim3(kVLanes<E>), 0, a.stream, a.items, a.places, a.vprefix, a.tok0,
                     a.ws, (T *)a.out, a.n, a.planes, a.ph, a.pw, a.pad_to, a.cv);
}

template <typename T>
static void launch_vpass_patches_e(int E, bool ppc, const ManyPatchArgs &a) {
  switch (E * 2 + (ppc ? 1 : 0)) {
    case 2: launch_vpass_patches<T, 1, false>(a); break;
    case 3: launch_vpass_patches<T, 1, true>(a); break;
    case 4: launch_vpass_patches<T, 2, false>(a); break;
    case 5: launch_vpass_patches<T, 2, true>(a); break;
    case 6: launch_vpass_patches<T, 3, false>(a); break;
    case 7: launch_vpass_patches<T, 3, true>(a); break;
    case 8: launch_vpass_patches<T, 4, false>(a); break;
    default: launch_vpass_patches<T, 4, true>(a); break;
  }
}

int aa_launch_many_patches(const void *desc_host, const void *desc_dev, void *out_dev, void *workspace_dev, size_t workspace_bytes, int out_elem,
                           int ppc, int normalize, const float *mean, const float *std, hipStream_t stream) {
  const AAManyHeader *hd = (const AAManyHeader *)desc_host;
  const int64_t patch_plan = AA_MANY_PLAN_PLACED | AA_MANY_PLAN_PATCHES;  // (and no AA_MANY_PLAN_ALPHA)
  if (hd->magic != AA_MANY_MAGIC || (hd->kind & (patch_plan | AA_MANY_PLAN_ALPHA)) != patch_plan || hd->n < 0 || hd->C < 1 || hd->C > 4) return AA_ERR_BAD_SHAPE;
  const int64_t n = hd->n, C = hd->C;
  const int rc = aa_many_check_launch(n, desc_dev, out_dev, workspace_dev, workspace_bytes, hd->ws_bytes, out_elem == AA_F32 ? 4 : 2);
  if (rc != AA_OK || n == 0) return rc;
  const int64_t *tail_host = patch_tail(desc_host, n);
  const AAManyPatchInfo *info = (const AAManyPatchInfo *)(tail_host + 2 * (n + 1));
  const int64_t vunits = tail_host[n];
  if (vunits <= 0 || vunits > INT32_MAX) return AA_ERR_BAD_SHAPE;
  const ManyViews v = many_views(hd, desc_dev);  // (a patch plan is a placed one: v.places is there)
  const int64_t *tail_dev = patch_tail(desc_dev, n);
  char *ws = (char *)workspace_dev;
  launch_many_tables_hpass<true>(hd, v, ws, hd->oH, hd->oW, stream);
  const ManyPatchArgs a = {v.items, v.places, tail_dev, tail_dev + n + 1, ws, out_dev, (int)n, v.planes, info->ph, info->pw, info->pad_to, vunits,
                           many_convert(normalize, mean, std, C), stream};
  if (out_elem == AA_F16) launch_vpass_patches_e<f16_t>(v.E, ppc != 0, a);
  else if (out_elem == AA_BF16) launch_vpass_patches_e<bf16_t>(v.E, ppc != 0, a);
  else launch_vpass_patches_e<float>(v.E, ppc != 0, a);
  AA_HIP_CHECK_LAUNCH();
  return AA_OK;
}

// ---- host: for composing planners (aa_many.h) ------------------------------------------------------------------------------------------------
int aa_many_plan_placed_always_host(int filter, int layout, int64_t n, int64_t C, int64_t oH, int64_t oW, const aa_many_image *images,
                                    const aa_many_place *places, void *desc_host, size_t desc_bytes, size_t *workspace_bytes) {
  return many_plan(filter, layout, n, C, oH, oW, images, places, nullptr, true, desc_host, desc_bytes, workspace_bytes);
}

int aa_launch_many_tables_hpass(const void *desc_host, const void *desc_dev, void *workspace_dev, size_t workspace_bytes, hipStream_t stream) {
  const AAManyHeader *hd = (const AAManyHeader *)desc_host;
  if (hd->magic != AA_MANY_MAGIC || (hd->kind & (AA_MANY_PLAN_PLACED | AA_MANY_PLAN_ALPHA)) != AA_MANY_PLAN_PLACED) return AA_ERR_BAD_SHAPE;
  const int rc = many_check(hd, desc_dev, hd->n, hd->C, hd->oH, hd->oW, hd->layout, workspace_dev, workspace_bytes);
  if (rc != AA_OK || hd->n == 0) return rc;
  launch_many_tables_hpass<true>(hd, many_views(hd, desc_dev), (char *)workspace_dev, hd->oH, hd->oW, stream);
  AA_HIP_CHECK_LAUNCH();
  return AA_OK;
}
