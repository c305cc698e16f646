// aa_many.h — the ragged call (include/aa_interp.h, "ragged batches"): N uint8 images of N sizes, each with its own box, into one dense
// batch.  The packed descriptor block aa_many_plan writes on the host and the three kernels read on the device:
//   [ AAManyHeader : 64 B ][ AAManyItem x n ][ int64 hunit_prefix[n + 1] ]            a plain plan (aa_many_desc_size)
//   [ AAManyHeader : 64 B ][ AAManyItem x n ][ int64 hunit_prefix[n + 1] ][ AAManyPlace x n ]   a placed plan (aa_many_desc_size_placed)
//   [ ... a placed plan ... ][ int64 vunit_prefix[n + 1] ][ int64 tok0[n + 1] ][ AAManyPatchInfo ]   a patch plan (aa_many_desc_size_patches)
// Everything a kernel needs about an item is in its record(s): no table header, nothing read back.
#pragma once

#include <stddef.h>

#include "aa_common.h"

#define AA_MANY_MAGIC 0x594E4D41  // 'AMNY'
#define AA_MANY_STRIP 64          // output columns per workgroup of the horizontal pass
#define AA_MANY_VBYTES 1024       // output-row bytes per workgroup of the vertical pass (256 lanes x 4)

// What a plan is (AAManyHeader.kind) and what an item asks of the kernels (AAManyItem.flags).  Both fields, the header's `flips` and its
// `fill` were called `reserved` while they were unused; the offsets and sizes are what they were.
#define AA_MANY_PLAN_PLACED 1   // AAManyPlace records follow the prefix sums
#define AA_MANY_PLAN_PATCHES 2  // a patch plan: its tail follows them (always with AA_MANY_PLAN_PLACED, never with AA_MANY_PLAN_ALPHA)
#define AA_MANY_PLAN_ALPHA 4    // some item has AA_MANY_ITEM_ALPHA: the launches take the alpha instantiations
#define AA_MANY_ITEM_FLIP 1     // AA_MANY_FLIP_X: the converting vertical pass writes the item mirrored left to right
#define AA_MANY_ITEM_ALPHA 2    // AA_MANY_PREMUL_ALPHA and not Pillow's copy (size asked for == [H, W], no box or the whole image): the
                                // horizontal pass premultiplies what it stages, the vertical passes convert back
static_assert(AA_MANY_ITEM_FLIP == AA_MANY_FLIP_X, "an item's flip bit is the caller's");

struct AAManyHeader {
  int32_t magic, n, C, oH, oW, filter, layout;
  int32_t flips;      // 1 when some item has AA_MANY_ITEM_FLIP (only the converting passes serve it)
  int64_t hunits;     // work units of the horizontal pass, all items: hunit_prefix[n]
  int64_t ws_bytes;   // table arena + intermediates
  int64_t kind;       // AA_MANY_PLAN_* bits; 0: a plain plan
  int64_t fill;       // a placed plan's fill, byte c = channel c's
};
static_assert(sizeof(AAManyHeader) == 64, "descriptor header is 64 bytes");
static_assert(offsetof(AAManyHeader, flips) == 28 && offsetof(AAManyHeader, kind) == 48 && offsetof(AAManyHeader, fill) == 56,
              "the renamed header fields keep their offsets");

// One item.  The image is read where it lies: byte (row y, column x, channel c) is at src + y * row_stride + x * E + c (interleaved class,
// E = C) or src + c * plane_stride + y * row_stride + x (planar class).  tab_h / tab_w / inter are byte offsets into the workspace.
// A table is [ int32 xmin[out] ][ int32 xsize[out] ][ int32 w[out * ksize] ], xmin relative to the hull's origin.
struct AAManyItem {
  const uint8_t *src;
  int64_t row_stride, plane_stride;
  int64_t tab_h, tab_w, inter;
  double in0_h, in1_h, in0_w, in1_w;  // Pillow's source interval per axis, float32 values (box_f32)
  int32_t oy, hull_h, ox, hull_w;     // the hull [o, o + hull) of all windows per axis: nothing outside it is read
  int32_t ksize_h, ksize_w;
  int32_t box_on;                     // 1: the scale is the FLOAT difference of the interval over the output size (a box); 0: in / out
  int32_t flags;                      // AA_MANY_ITEM_* bits
};
static_assert(sizeof(AAManyItem) == 112, "descriptor item is 112 bytes");
static_assert(offsetof(AAManyItem, flags) == 108, "the renamed item field keeps its offset");

// A placed plan's second record of an item: the item is resized to its own size [vh, vw] and that result's corner lies at (py, px) of
// the [oH, oW] canvas.  Per axis the covered part of the result is [v0, v0 + m) and lands at canvas index d = v0 + p; the item's table of
// that axis holds m entries (index 0 is result index v0), its intermediate hull_h rows of mw columns, each row led by (dx * E) & 3 bytes
// so that a canvas dword of the vertical pass is a dword of the intermediate.  An item covered on no axis has m = hull = ksize = 0.
struct AAManyPlace {
  int32_t vh, vw, v0h, v0w, mh, mw, dy, dx;
};
static_assert(sizeof(AAManyPlace) == 32, "placement record is 32 bytes");
__host__ __device__ inline int aa_many_placed_lead(int dx, int E) { return (int)(((int64_t)dx * E) & 3); }
__host__ __device__ inline int64_t aa_many_placed_pitch(int dx, int mw, int E) { return (aa_many_placed_lead(dx, E) + (int64_t)mw * E + 3) & ~(int64_t)3; }

// A patch plan (resize_many_to_patches): a placed plan in which every item is the whole of its own [vh, vw] canvas (place {vh, vw, 0, 0};
// the header's oH, oW are the largest vh and vw, which only size the grid of the table kernel), followed by the work units of the
// patch-writing vertical pass and where each item's token rows start.  Item i has planes * vh_i * ceil(vw_i / kVPixels<E>) image units, then
// ceil((pad_to - T_i) * D / AA_MANY_PAD_ELEMS) pad units (pad_to > 0 only); its first token is row tok0[i] of the output, tok0[n] the
// output's rows.
#define AA_MANY_PAD_ELEMS 4096  // zero elements per pad unit
struct AAManyPatchInfo {
  int32_t ph, pw;
  int64_t pad_to;  // 0: packed rows
};
static_assert(sizeof(AAManyPatchInfo) == 16, "patch tail is 16 bytes");
__host__ __device__ constexpr int aa_many_vpixels(int E) { return E == 1 ? 1024 : (E == 2 ? 512 : 256); }  // kVPixels<E> of aa_many.hip

inline size_t aa_many_table_bytes(int64_t out, int ksize) { return aa_align16(4 * (size_t)out * (2 + (size_t)ksize)); }
__host__ __device__ inline int64_t aa_many_inter_pitch(int64_t oW, int E) { return (oW * E + 3) & ~(int64_t)3; }  // rows of the intermediate start on a dword

size_t aa_many_desc_size(int64_t n);
size_t aa_many_desc_size_placed(int64_t n);
size_t aa_many_desc_size_patches(int64_t n);
// places NULL, or every place the whole canvas at offset 0: the plain plan, whatever the fill.
int aa_many_plan_host(int filter, int layout, int64_t n, int64_t C, int64_t oH, int64_t oW, const aa_many_image *images,
                      const aa_many_place *places, const uint8_t *fill, void *desc_host, size_t desc_bytes, size_t *workspace_bytes);
int aa_launch_many_u8(const void *desc_host, const void *desc_dev, int64_t n, int64_t C, int64_t oH, int64_t oW, int layout, void *out_dev,
                      void *workspace_dev, size_t workspace_bytes, hipStream_t stream);
// The same with the converting vertical pass: out_elem AA_F32 / AA_F16 / AA_BF16, out_layout the layout of the dense output.
int aa_launch_many_float(const void *desc_host, const void *desc_dev, int64_t n, int64_t C, int64_t oH, int64_t oW, int layout, void *out_dev,
                         void *workspace_dev, size_t workspace_bytes, int out_elem, int out_layout, int normalize, const float *mean,
                         const float *std, hipStream_t stream);
// The patch plan and its launches: sizes[2 i], sizes[2 i + 1] = (vH_i, vW_i), multiples of (ph, pw); pad_to 0 = packed rows.  The plan
// reports the output's rows; the launch takes everything else from the plan's header.  ppc: token vectors [ph, pw, C] instead of [C, ph, pw].
int aa_many_plan_patches_host(int filter, int layout, int64_t n, int64_t C, int64_t ph, int64_t pw, const aa_many_image *images, const int64_t *sizes,
                              int64_t pad_to, void *desc_host, size_t desc_bytes, size_t *workspace_bytes, int64_t *rows);
int aa_launch_many_patches(const void *desc_host, const void *desc_dev, void *out_dev, void *workspace_dev, size_t workspace_bytes, int out_elem,
                           int ppc, int normalize, const float *mean, const float *std, hipStream_t stream);
// For a planner that composes placed plans of its own (aa_many_ycbcr.hip): aa_many_plan_host's block with the placement records always
// present (a patch plan's `own_canvas`: no bound on a dense vertical grid, which the composing planner has itself), and the table kernel
// and the horizontal pass of such a block, enqueued on their own (two launches; none for n == 0 or when no item lies on the canvas).
int aa_many_plan_placed_always_host(int filter, int layout, int64_t n, int64_t C, int64_t oH, int64_t oW, const aa_many_image *images,
                                    const aa_many_place *places, void *desc_host, size_t desc_bytes, size_t *workspace_bytes);
int aa_launch_many_tables_hpass(const void *desc_host, const void *desc_dev, void *workspace_dev, size_t workspace_bytes, hipStream_t stream);
