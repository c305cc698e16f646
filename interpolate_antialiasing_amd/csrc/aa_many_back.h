// aa_many_back.h — the return path of the ragged calls (include/aa_interp.h, "ragged predictions back", aa_back_many_plan): N float
// sources [K, h_i, w_i] — the rectangles of a model's canvas output that the images occupied — each resampled to its image's own
// [oh_i, ow_i] in the reference's fp32 arithmetic (AA_TABLE_F32 tables), and stored as values, as the argmax over K, or as value >
// threshold.  The packed descriptor block the planner writes on the host and the kernels read on the device:
//   [ AABackHeader : 64 B ][ AABackItem x n ][ int64 unit0[n + 1] ]
// unit0[i] is the first work unit of item i; a unit is one output row of an item times AA_BACK_TILE consecutive output columns.
// Everything a kernel needs about an item is in its record: nothing is read back.
#pragma once

#include "aa_common.h"

#define AA_BACK_MAGIC 0x4B434142  // 'BACK'
#define AA_BACK_THREADS 256       // lanes of a workgroup of the table kernel
#define AA_BACK_TILE 256          // output columns of a work unit: the lanes of a workgroup of the resample
#define AA_BACK_UNROLL 4          // classes a lane carries through its windows at a time
#define AA_BACK_MAX_ELEMS ((int64_t)1 << 40)  // the bound on K * oh_i * ow_i, and on the elements of the arena

enum { AA_BACK_VALUES = 0, AA_BACK_ARGMAX = 1, AA_BACK_GREATER = 2 };
// The activation an item's (a member's) fp32 value goes through before the reduction (and before the merged call's sum) is one of
// include/aa_interp.h's AA_BACK_ACT_NONE / _SOFTMAX / _SIGMOID; the device code is aa_activation.h.
#define AA_BACK_ACT_MEMBERS 16  // the most members of a group of a merged SOFTMAX plan: a lane keeps (max, 1 / denominator) per member in LDS

struct AABackHeader {
  int32_t magic, n, K, filter, layout;
  int32_t reduce;     // AA_BACK_*
  int32_t out_dtype;  // aa_dtype of an arena element
  int32_t reserved0;  // AA_BACK_ACT_* (0, none: what the field held before there were activations)
  int64_t units;      // unit0[n]: the workgroups of the resample
  int64_t ws_bytes;   // the table arena: per item its H table, then its W table
  int64_t arena_bytes;
  int64_t reserved;
};
static_assert(sizeof(AABackHeader) == 64, "descriptor header is 64 bytes");

// One item.  src is the region's corner; class k, row y, pixel x of the region at src + k * stride_ch + y * stride_row + x * stride_px
// ELEMENTS.  Its two tables are packed tables of include/aa_interp.h's format (header, xmin, xsize, float weights; no gather section) at
// tab_h (h -> oh) and tab_w (w -> ow) of the workspace, rows ksize floats long.  out_off: bytes from the arena's start, a multiple of 16.
struct AABackItem {
  const void *src;
  int64_t stride_ch, stride_row, stride_px;
  int64_t tab_h, tab_w, out_off;
  int32_t h, w, oh, ow;
  int32_t ksize_h, ksize_w;
  float scale_h, scale_w;  // area_pixel_compute_scale<float>: (float)in / (float)out
  int32_t flags;           // AA_MANY_FLIP_X
  int32_t xtiles;          // ceil(ow / AA_BACK_TILE)
};
static_assert(sizeof(AABackItem) == 96, "descriptor item is 96 bytes");

// ---- merged (aa_back_merged_plan): the n items are MEMBERS of G groups, a group one output: its members, each resampled to the group's
// [oh, ow], are summed in fp32 in ascending item order (and divided by their count for the mean) before the reduction over K.  The block:
//   [ AABackMergedHeader : 64 B ][ AABackItem x n ][ AABackGroup x G ][ int32 member[n], padded to 8 B ][ int64 unit0[G + 1] ]
// A member is an ordinary AABackItem whose oh, ow and out_off are its group's, so back_tables builds its tables unchanged.  member[] is
// the item indices grouped by group, ascending within a group; group g's are member[first .. first + count).  unit0[g] is the first work
// unit of group g; a unit is one output row of a GROUP times AA_BACK_TILE consecutive output columns.
#define AA_BACK_MERGED_MAGIC 0x4B43424D  // 'MBCK'
enum { AA_BACK_MERGE_SUM = 0, AA_BACK_MERGE_MEAN = 1 };

struct AABackMergedHeader {
  int32_t magic, n, K, filter, layout;
  int32_t reduce;     // AA_BACK_*
  int32_t out_dtype;  // aa_dtype of an arena element
  int32_t merge;      // AA_BACK_MERGE_*
  int64_t units;      // unit0[G]: the workgroups of the resample
  int64_t ws_bytes;   // the table arena: per member its H table, then its W table (aa_back_many_plan's for the same items)
  int64_t arena_bytes;
  int32_t G;
  int32_t reserved;   // AA_BACK_ACT_* (0, none: what the field held before there were activations)
};
static_assert(sizeof(AABackMergedHeader) == 64, "descriptor header is 64 bytes");

struct AABackGroup {
  int64_t out_off;  // bytes from the arena's start, a multiple of 16
  int32_t first;    // the group's first slot of member[]
  int32_t count;    // its members, at least 1
  int32_t oh, ow;
  int32_t xtiles;   // ceil(ow / AA_BACK_TILE)
  int32_t reserved;
};
static_assert(sizeof(AABackGroup) == 32, "descriptor group is 32 bytes");

size_t aa_back_merged_desc_size(int64_t n, int64_t g);
int aa_back_merged_plan_host(int filter, int layout, int64_t n, int64_t K, const aa_back_item *items, int64_t G, const int64_t *group_of, int merge,
                             int reduce, int activation, int out_dtype, void *desc_host, size_t desc_bytes, size_t *workspace_bytes, size_t *arena_bytes,
                             int64_t *out_offsets);
int aa_launch_back_merged(const void *desc_host, const void *desc_dev, int in_dtype, float threshold, void *arena_dev, size_t arena_bytes,
                          void *workspace_dev, size_t workspace_bytes, hipStream_t stream);

size_t aa_back_desc_size(int64_t n);
int aa_back_plan_host(int filter, int layout, int64_t n, int64_t K, const aa_back_item *items, int reduce, int activation, int out_dtype, void *desc_host,
                      size_t desc_bytes, size_t *workspace_bytes, size_t *arena_bytes, int64_t *out_offsets);
int aa_launch_back_many(const void *desc_host, const void *desc_dev, int in_dtype, float threshold, void *arena_dev, size_t arena_bytes,
                        void *workspace_dev, size_t workspace_bytes, hipStream_t stream);
