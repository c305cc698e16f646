// aa_many_maps.h — Pillow's "I;16" / "I" / "F" resize for a ragged batch (include/aa_interp.h, "ragged batches", aa_many_plan_maps): N
// single-channel maps of uint16, int32 or float32 elements, each with its own box, size, place on the canvas and flip, filtered with
// double coefficients into a double sum and stored by the mode's own rule after EACH pass.  The packed descriptor block the planner
// writes on the host and the three kernels read on the device:
//   [ AAMapsHeader : 64 B ][ AAMapsItem x n ][ int64 hunit_prefix[n + 1] ]
// Everything a kernel needs about an item is in its record: nothing is read back.
#pragma once

#include "aa_common.h"
#include "aa_many.h"

#define AA_MAPS_MAGIC 0x5350414D  // 'MAPS'
#define AA_MAPS_VCOLS 256         // canvas columns per workgroup of the vertical pass (one per lane)
#define AA_MAPS_HROWS 16          // hull rows per workgroup of the horizontal pass, beside AA_MANY_STRIP output columns
#define AA_MAPS_ITEM_FLIP 1       // AA_MANY_FLIP_X: the vertical pass writes the item's canvas row mirrored left to right
#define AA_MAPS_ITEM_HPASS 2      // Pillow runs the horizontal pass: tab_w and the intermediate exist
#define AA_MAPS_ITEM_VPASS 4      // Pillow runs the vertical pass: tab_h exists
static_assert(AA_MAPS_ITEM_FLIP == AA_MANY_FLIP_X, "an item's flip bit is the caller's");

struct AAMapsHeader {
  int32_t magic, n, oH, oW, filter;
  int32_t elem;      // AA_MAPS_U16 / AA_MAPS_I32 / AA_MAPS_F32
  int32_t overflow;  // AA_MAPS_OVERFLOW_PILLOW / AA_MAPS_OVERFLOW_CLAMP (read for AA_MAPS_U16 only)
  uint32_t fill;     // the fill's element, in the low bytes
  int64_t hunits;    // work units of the horizontal pass, all items: hunit_prefix[n]
  int64_t ws_bytes;  // table arena + intermediates
  int64_t reserved[2];
};
static_assert(sizeof(AAMapsHeader) == 64, "descriptor header is 64 bytes");

// One item.  Element (row y, column x) of the map is at src + y * row_stride + x * EB, EB the bytes of an element; only EB-byte alignment
// is assumed.  Per axis the item is resized to its own size v; [v0, v0 + m) of that result lies on the canvas, from canvas index d on.
// A pass that runs (its flag) has a table
//   [ int32 xmin[m] ][ int32 xsize[m] ][ double w[m * ksize] ]
// at its tab offset of the workspace, entry t the window of result index v0 + t, xmin relative to the hull's origin, the weights
// Pillow's normalised doubles, zero from xsize to ksize.  The hull [o, o + hull) of an axis is what its pass reads: the union of the
// covered windows for a pass that runs; for one that does not, the source indices the covered results copy, int(box origin) + v0 onward
// (m of them).  HPASS: the intermediate, at `inter`, holds hull_h rows of mw elements, row r the horizontal result of source row oy + r,
// and the vertical kernel reads it; without HPASS that kernel reads the source, rows from oy and columns from ox.
struct AAMapsItem {
  const uint8_t *src;
  int64_t row_stride;
  int64_t tab_h, tab_w, inter;
  double in0_h, scale_h, in0_w, scale_w;  // Pillow's centre of result index i is in0 + (i + 0.5) * scale, per axis
  int32_t in_h, in_w;
  int32_t oy, hull_h, ox, hull_w;
  int32_t ksize_h, ksize_w;
  int32_t vh, vw, v0h, v0w, mh, mw, dy, dx;
  int32_t flags;  // AA_MAPS_ITEM_* bits
  int32_t reserved;
};
static_assert(sizeof(AAMapsItem) == 144, "descriptor item is 144 bytes");

__host__ __device__ inline size_t aa_maps_table_w_off(int64_t m) { return 8 * (size_t)m; }  // (xmin and xsize: a multiple of 8 bytes)
inline size_t aa_maps_table_bytes(int64_t m, int ksize) { return aa_align16(aa_maps_table_w_off(m) + 8 * (size_t)m * (size_t)ksize); }
__host__ __device__ inline int aa_maps_elem_bytes(int elem) { return elem == 0 ? 2 : 4; }

size_t aa_maps_desc_size(int64_t n);
int aa_maps_plan_host(int filter, int elem, int64_t n, int64_t oH, int64_t oW, const aa_many_image *images, const aa_many_place *places,
                      double fill, int overflow, void *desc_host, size_t desc_bytes, size_t *workspace_bytes);
int aa_launch_many_maps(const void *desc_host, const void *desc_dev, void *out_dev, void *workspace_dev, size_t workspace_bytes,
                        hipStream_t stream);
