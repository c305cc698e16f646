// aa_many_back_peaks.h — the ragged return path's reduction over SPACE, for keypoint and landmark heads (include/aa_interp.h,
// aa_back_peaks_plan): item i is K heatmaps [K, h_i, w_i], resampled to [oh_i, ow_i] as aa_back_many_plan's items are (R_i, bit for
// bit), and per channel only the place of its maximum and five values around it are stored.  The packed descriptor block:
//   [ AABackPeaksHeader : 80 B ][ AABackItem x n ][ int64 unit0[n + 1] ]
// The sections after the header are aa_many_back.h's, so the table kernel's body and the class loops read them unchanged.  unit0[i] is
// the first work unit of item i, a unit AA_BACK_PEAKS_ROWS consecutive output rows times AA_BACK_TILE consecutive output columns,
// numbered row tile by row tile (row_tile).
// The workspace: the items' tables as aa_back_many_plan lays them out (tables_bytes), then at keys_off n * K 64-bit keys, one per
// (item, channel).  The key of a pixel of value v at flat index f = y * ow + x (un-mirrored) is
//   ord(v) << 32 | (0xFFFFFFFF - f)
// with ord the monotone map of float bits to uint32 taken after -0.0 has become +0.0 and every NaN 0xFFFFFFFF: a sign bit set flips
// all bits, a sign bit clear sets it.  ord(-inf) = 0x007FFFFF > 0, so no pixel's key is 0 and 0 is "empty", what the table launch
// writes.  Keys are totally ordered, and their order is numpy.argmax's: a greater value wins, a NaN beats every number, and among
// equal ord — equal numbers, +-0.0, two NaNs — the LOWER flat index has the greater key.  The maximum over a total order is
// associative and commutative, so the winning key does not depend on how the pixels are split over lanes, waves and workgroups, nor
// on the order in which the atomics arrive: the same bits for every launch shape and on every run.  The key's value half only orders
// (it has lost the sign of zero and the NaN's payload): the values stored are resampled again at the decoded place.
// The arena: peaks [n, K, 2] int32 (x, y) at byte 0, then values [n, K, 5] float32 (the peak, its left, right, upper and lower
// neighbour; a neighbour outside the image is the peak's own value) at values_off, a multiple of 16.
// Not built: groups (merged passes), an activation, the top-k peaks of a channel or a non-maximum suppression; the swap of left and
// right channel pairs that a flipped test-time pass needs is the caller's.
#pragma once

#include "aa_many_back.h"

#define AA_BACK_PEAKS_MAGIC 0x4B414550  // 'PEAK'
#ifndef AA_BACK_PEAKS_ROWS
#define AA_BACK_PEAKS_ROWS 16  // output rows a lane walks per class chunk before the keys meet (profiles/resize_many_back_peaks.txt)
#endif
#define AA_BACK_PEAKS_VALUES 5              // the peak, left, right, up, down
#define AA_BACK_PEAKS_MAX_PIXELS INT32_MAX  // oh * ow of an item: a flat index is 32 bits of the key
static_assert(AA_BACK_PEAKS_ROWS >= 1, "a work unit has rows");

struct AABackPeaksHeader {
  int32_t magic, n, K, filter, layout;
  int32_t rows;  // AA_BACK_PEAKS_ROWS of the library that planned
  int32_t reserved0, reserved1;
  int64_t units;         // unit0[n]: the workgroups of the resample
  int64_t ws_bytes;      // the tables and the keys
  int64_t arena_bytes;
  int64_t tables_bytes;  // aa_back_many_plan's workspace for the same items
  int64_t keys_off;      // of the workspace, a multiple of 16
  int64_t values_off;    // of the arena, a multiple of 16
};
static_assert(sizeof(AABackPeaksHeader) == 80, "descriptor header is 80 bytes");

size_t aa_back_peaks_desc_size(int64_t n);
int aa_back_peaks_plan_host(int filter, int layout, int64_t n, int64_t K, const aa_back_item *items, void *desc_host, size_t desc_bytes,
                            size_t *workspace_bytes, size_t *arena_bytes, int64_t *values_offset);
int aa_launch_back_peaks(const void *desc_host, const void *desc_dev, int in_dtype, void *arena_dev, size_t arena_bytes, void *workspace_dev,
                         size_t workspace_bytes, hipStream_t stream);
