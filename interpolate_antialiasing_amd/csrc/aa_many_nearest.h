// aa_many_nearest.h — Pillow's NEAREST for a ragged batch (include/aa_interp.h, "ragged batches", aa_many_plan_nearest): N label maps of N
// sizes, each with its own box, size, place on the canvas and flip, copied element by element into one dense batch.  The packed descriptor
// block the planner writes on the host and the two kernels read on the device:
//   [ AANearHeader : 64 B ][ AANearItem x n ][ int64 unit_prefix[n + 1] ]
// Everything a kernel needs about an item is in its record: nothing is read back.
#pragma once

#include "aa_common.h"
#include "aa_many.h"

#define AA_NEAR_MAGIC 0x52454E41  // 'ANER'

struct AANearHeader {
  int32_t magic, n, C, oH, oW, layout, elem_bytes, reserved0;
  int64_t units;     // work units of the gather, all items: unit_prefix[n]
  int64_t ws_bytes;  // the index tables
  int32_t fill[4];   // fill[c], channel c's element (the low elem_bytes bytes are written)
};
static_assert(sizeof(AANearHeader) == 64, "descriptor header is 64 bytes");

// One item.  The image is read where it lies, as AAManyItem's: element (row y, column x, channel c) is at src + y * row_stride + x * PB + c
// (interleaved class, PB = C bytes, uint8 only) or src + c * plane_stride + y * row_stride + x * elem_bytes (planar class).
// Per axis the item is resized to its own size v; [v0, v0 + m) of that result lies on the canvas.  a and xo0 are Pillow's two doubles of the
// axis (boxmath.nearest_indices): index x of the result reads source index int(xo0 + a + a + ... (x adds)), and the table kernel runs that
// sum from x = 0 whatever v0 is.  elem_bytes 2 (Pillow's "I;16", which its generic transform serves): no sum, index x reads
// int(a * (x + 0.5) + xo0) with xo0 = b0, the box's first value.
//   tab_h: int32[mh], entry t the source row of result row v0h + t, clamped to [0, in_h).
//   tab_w: int32[lead + mw * UP (rounded up to a multiple of 4)], UP = units per pixel (C for interleaved uint8, else 1; a unit is one
//          element).  Entry lead + p is the source BYTE offset within the row of canvas unit cu0 + p, cu0 = dxo * UP, in canvas order: an
//          item that flips has its pixels mirrored here, and dxo is where the covered part starts on the mirrored canvas row.  lead =
//          cu0 mod (4 / elem_bytes), so that the entries of one output dword are one aligned vector of the table.
struct AANearItem {
  const uint8_t *src;
  int64_t row_stride, plane_stride;
  int64_t tab_h, tab_w;
  double a_h, xo0_h, a_w, xo0_w;
  int32_t in_h, in_w;
  int32_t vh, vw, v0h, v0w, mh, mw, dy, dx;
  int32_t dxo;    // dx, or oW - dx - mw for an item that flips
  int32_t flags;  // AA_MANY_FLIP_X
  int64_t reserved;
};
static_assert(sizeof(AANearItem) == 128, "descriptor item is 128 bytes");

__host__ __device__ inline int aa_near_units_per_pixel(int E, int elem_bytes) { return elem_bytes == 1 ? E : 1; }
__host__ __device__ inline int aa_near_lead(int64_t cu0, int elem_bytes) { return (int)(cu0 & (4 / elem_bytes - 1)); }
inline size_t aa_near_tab_h_bytes(int64_t mh) { return aa_align16(4 * (size_t)mh); }
inline size_t aa_near_tab_w_bytes(int64_t cu0, int64_t units, int elem_bytes) {
  return units ? aa_align16(4 * (size_t)(aa_near_lead(cu0, elem_bytes) + units)) : 0;
}

size_t aa_near_desc_size(int64_t n);
int aa_near_plan_host(int layout, int elem_bytes, int64_t n, int64_t C, int64_t oH, int64_t oW, const aa_many_image *images,
                      const aa_many_place *places, const int32_t *fill, void *desc_host, size_t desc_bytes, size_t *workspace_bytes);
int aa_launch_many_nearest(const void *desc_host, const void *desc_dev, void *out_dev, void *workspace_dev, size_t workspace_bytes,
                           int out_elem_bytes, hipStream_t stream);
