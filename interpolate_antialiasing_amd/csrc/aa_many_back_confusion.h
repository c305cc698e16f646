// aa_many_back_confusion.h — per-image confusion matrices of the ragged return path (include/aa_interp.h, aa_back_confusion_plan): the
// label map of aa_back_many_plan's reduce 1 (or aa_back_merged_plan's) is compared with an integer target of the image's size where it
// is computed, and only the K x K counts of every image reach memory.  The packed descriptor block, plain and merged:
//   [ AABackConfHeader : 64 B ][ AABackItem x n ][ int64 unit0[n + 1] ][ AABackConfTarget x n ]
//   [ AABackConfHeader : 64 B ][ AABackItem x n ][ AABackGroup x G ][ int32 member[n], padded to 8 B ][ int64 unit0[G + 1] ][ AABackConfTarget x G ]
// The sections before the targets are aa_many_back.h's, so the table kernel's body and the resamples' class loops read them unchanged.
// unit0[i] is the first work unit of output i (an item, or a group); a unit is AA_BACK_CONF_ROWS consecutive output rows times
// AA_BACK_TILE consecutive output columns, numbered row tile by row tile.
#pragma once

#include "aa_many_back.h"

#define AA_BACK_CONF_MAGIC 0x464E4F43  // 'CONF'
#ifndef AA_BACK_CONF_ROWS
#define AA_BACK_CONF_ROWS 8   // output rows a workgroup walks, its counts kept in LDS between them (profiles/resize_many_back_confusion.txt)
#endif
// (the slots of a wave, AA_BACK_CONF_SLOTS of key << AA_BACK_CONF_COUNT_BITS | count: aa_many_back.h)
static_assert(AA_BACK_CONF_ROWS >= 1 && 64 * AA_BACK_CONF_ROWS < (1 << AA_BACK_CONF_COUNT_BITS), "a slot's count holds a wave's pixels");

struct AABackConfHeader {
  int32_t magic, n, K, filter, layout;
  int32_t activation;    // AA_BACK_ACT_*
  int32_t target_dtype;  // AA_U8, AA_I16, AA_I32 or AA_I64: uniform over the launch
  int32_t merge;         // AA_BACK_MERGE_* (merged)
  int64_t units;         // unit0[outputs]: the workgroups of the resample
  int64_t ws_bytes;      // the table arena, aa_back_many_plan's for the same items
  int64_t conf_elems;    // outputs * K * K
  int32_t G;             // the groups of a merged plan
  int32_t merged;        // 0: the outputs are the n items; 1: the G groups
};
static_assert(sizeof(AABackConfHeader) == 64, "descriptor header is 64 bytes");

// What an output has besides its item's or group's record: row y, column x of its target at tgt + (y * stride_row + x) ELEMENTS, its
// K x K block at element conf_off of the result, and ceil(oh / AA_BACK_CONF_ROWS).
struct AABackConfTarget {
  const void *tgt;
  int64_t stride_row;
  int64_t conf_off;
  int32_t ytiles;
  int32_t reserved;
};
static_assert(sizeof(AABackConfTarget) == 32, "descriptor target is 32 bytes");

size_t aa_back_conf_desc_size(int64_t n, int64_t g, int merged);
int aa_back_conf_plan_host(int filter, int layout, int64_t n, int64_t K, const aa_back_item *items, int merged, int64_t G, const int64_t *group_of,
                           int merge, const aa_back_target *targets, int target_dtype, int activation, void *desc_host, size_t desc_bytes,
                           size_t *workspace_bytes, int64_t *conf_elems);
int aa_launch_back_confusion(const void *desc_host, const void *desc_dev, int in_dtype, void *conf_dev, size_t conf_elems, void *workspace_dev,
                             size_t workspace_bytes, hipStream_t stream);
