// aa_many_back_panoptic.h — the ragged return path's panoptic inference for mask-classification heads (include/aa_interp.h,
// aa_back_panoptic_plan): item i is Q mask logits [Q, h_i, w_i] and Q scores; the masks are resampled to [oh_i, ow_i] as
// aa_back_many_plan's items are (K = Q) and go through the sigmoid; per pixel the kept query of the greatest score * probability wins,
// per query the pixels it won, the pixels of its own mask and the pixels it won inside its mask are counted, and the segment map holds
// the ids of the queries that pass the overlap test.  The packed descriptor block:
//   [ AABackPanopticHeader : 96 B ][ AABackItem x n ][ int64 unit0[n + 1] ][ int64 fin0[n + 1] ]
// The sections before fin0 are aa_many_back.h's, so the table kernel's body and the class loops read them unchanged.  unit0[i] is the
// first work unit of item i in the resample, a unit AA_BACK_PANOPTIC_ROWS consecutive output rows times AA_BACK_TILE consecutive
// output columns, numbered row tile by row tile; fin0[i] its first unit in the finalise, a unit AA_BACK_PANOPTIC_FIN_BYTES of its map.
// The workspace: the items' tables as aa_back_many_plan lays them out (tables_bytes), then from kept_off on one kept list per item,
// kept_words int32 each: [ count ][ entries, ascending ].  An entry is a kept query's index, or — items that take the vector loads —
// q0 | mask << 16 for the aligned chunk of AA_BACK_UNROLL queries from q0 with at least one kept member, bit c of mask for q0 + c.
// The arena: the items' maps at out_off (multiples of 16), then counts [n, Q, 3] int64 at counts_off, then survives [n, Q] uint8 at
// survives_off, both multiples of 16.
#pragma once

#include "aa_many_back.h"

#define AA_BACK_PANOPTIC_MAGIC 0x4F4E4150  // 'PANO'
#define AA_BACK_PANOPTIC_MAX_Q 256         // the queries of a call: a workgroup of the table kernel compacts an item's kept list
#ifndef AA_BACK_PANOPTIC_ROWS
#define AA_BACK_PANOPTIC_ROWS 16  // output rows a workgroup walks, its counts kept in LDS between them (profiles/resize_many_back_panoptic.txt)
#endif
#define AA_BACK_PANOPTIC_FIN_PIECES 4  // 16-byte pieces of the map a lane of the finalise rewrites
#define AA_BACK_PANOPTIC_FIN_BYTES (AA_BACK_PANOPTIC_FIN_PIECES * AA_BACK_THREADS * 16)
static_assert(AA_BACK_PANOPTIC_ROWS >= 1 && 64 * AA_BACK_PANOPTIC_ROWS < (1 << AA_BACK_CONF_COUNT_BITS), "a slot's count holds a wave's pixels");

struct AABackPanopticHeader {
  int32_t magic, n, Q, filter, layout;
  int32_t out_dtype;  // aa_dtype of a map element: AA_U8 (Q <= 255), AA_I16, AA_I32 or AA_I64
  int32_t kept_words; // int32 words of an item's kept list: 1 + Q rounded up to 4
  int32_t reserved0;
  int64_t units;      // unit0[n]: the workgroups of the resample
  int64_t fin_units;  // fin0[n]: the workgroups of the finalise
  int64_t ws_bytes;   // the tables and the kept lists
  int64_t arena_bytes;
  int64_t tables_bytes;  // aa_back_many_plan's workspace for the same items
  int64_t kept_off;      // of the workspace, a multiple of 16
  int64_t counts_off, survives_off;  // of the arena, multiples of 16
};
static_assert(sizeof(AABackPanopticHeader) == 96, "descriptor header is 96 bytes");

size_t aa_back_panoptic_desc_size(int64_t n);
int aa_back_panoptic_plan_host(int filter, int layout, int64_t n, int64_t Q, const aa_back_item *items, int out_dtype, void *desc_host, size_t desc_bytes,
                               size_t *workspace_bytes, size_t *arena_bytes, int64_t *out_offsets, int64_t *counts_offset, int64_t *survives_offset);
int aa_launch_back_panoptic(const void *desc_host, const void *desc_dev, int in_dtype, const aa_back_panoptic_io *io, void *arena_dev, size_t arena_bytes,
                            void *workspace_dev, size_t workspace_bytes, hipStream_t stream);
