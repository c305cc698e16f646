// aa_many_back_instances.h — the ragged return path's instance inference for mask-classification heads (include/aa_interp.h,
// aa_back_instances_plan): item i is Q mask logits [Q, h_i, w_i] and M slots, slot m asking for query queries[i, m]; the asked masks are
// resampled to [oh_i, ow_i] as aa_back_many_plan's items are (K = Q), thresholded at 0 and stored per slot as bytes or packed bits, and
// per slot the area, the exact sum of the sigmoid over the mask and the tight box are counted.  The packed descriptor block:
//   [ AABackInstancesHeader : 80 B ][ AABackItem x n ][ int64 unit0[n + 1] ]
// The sections after the header are aa_many_back.h's, so the table kernel's body and the class loops read them unchanged.  unit0[i] is
// the first work unit of item i, a unit AA_BACK_INSTANCES_ROWS consecutive output rows times AA_BACK_TILE consecutive output columns,
// numbered row tile by row tile.
// The workspace: the items' tables as aa_back_many_plan lays them out (tables_bytes), then from lists_off on one work list per item,
// list_words int32 each:
//   [0]                 E, the entries
//   [1]                 the first empty slot's place in `slots` (the slots before it ask for a query)
//   [2 .. 2 + Q)        query q's range of `slots`: first | count << 16 (count 0: nobody asked)
//   [2 + Q .. 2 + 2 Q)  the entries, ascending: a DISTINCT asked query's index, or — items that take the vector loads — q0 | mask << 16
//                       for the aligned chunk of AA_BACK_UNROLL queries from q0 with at least one asked member, bit c of mask for q0 + c
//   [2 + 2 Q .. + M)    slots: the slot indices sorted by (query, slot), the empty slots (an entry outside 0 .. Q - 1) last
// The arena: the items' masks at out_off (multiples of 16) — [M, oh, ow] bytes 0 / 1, or with `bits` [M, oh, ceil(ow / 8)] bytes, bit
// x & 7 of byte x >> 3 column x — then stats [n, M, 6] int64 (area, psum, x0, y0, x1, y1) at stats_off, a multiple of 16.
#pragma once

#include "aa_many_back.h"

#define AA_BACK_INSTANCES_MAGIC 0x54534E49  // 'INST'
#define AA_BACK_INSTANCES_MAX_Q 256         // the queries of a call: a wave keeps one record per query in LDS
#define AA_BACK_INSTANCES_MAX_M 256         // the slots of an item: a lane of the table kernel's workgroup ranks one
#ifndef AA_BACK_INSTANCES_ROWS
#define AA_BACK_INSTANCES_ROWS 8  // output rows a workgroup walks, its records kept in LDS between them (profiles/resize_many_back_instances.txt)
#endif
#define AA_BACK_INSTANCES_STATS 6  // int64 words of a slot's stats
static_assert(AA_BACK_INSTANCES_ROWS >= 1 && AA_BACK_INSTANCES_ROWS <= 255, "a record holds a tile's first and last row in a byte each");

struct AABackInstancesHeader {
  int32_t magic, n, Q, M, filter, layout;
  int32_t bits;        // 0: a byte per pixel, 1: a bit per pixel
  int32_t list_words;  // int32 words of an item's work list: 2 + 2 Q + M rounded up to 4
  int64_t units;       // unit0[n]: the workgroups of the resample
  int64_t ws_bytes;    // the tables and the work lists
  int64_t arena_bytes;
  int64_t tables_bytes;  // aa_back_many_plan's workspace for the same items
  int64_t lists_off;     // of the workspace, a multiple of 16
  int64_t stats_off;     // of the arena, a multiple of 16
};
static_assert(sizeof(AABackInstancesHeader) == 80, "descriptor header is 80 bytes");

size_t aa_back_instances_desc_size(int64_t n);
int aa_back_instances_plan_host(int filter, int layout, int64_t n, int64_t Q, int64_t M, const aa_back_item *items, int bits, void *desc_host,
                                size_t desc_bytes, size_t *workspace_bytes, size_t *arena_bytes, int64_t *out_offsets, int64_t *stats_offset);
int aa_launch_back_instances(const void *desc_host, const void *desc_dev, int in_dtype, const aa_back_instances_io *io, void *arena_dev, size_t arena_bytes,
                             void *workspace_dev, size_t workspace_bytes, hipStream_t stream);
