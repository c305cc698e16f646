// aa_reduce_many.h — the ragged Image.reduce (include/aa_interp.h, "ragged Image.reduce"): N uint8 images of N sizes, each with its own
// integer box and its own factors, into one arena.  The packed descriptor block aa_reduce_many_plan writes on the host and the kernel
// reads on the device:
//   [ AAReduceManyHeader : 64 B ][ AAReduceManyItem x n ][ int64 unit_prefix[n + 1] ]
// Everything the kernel needs about an item is in its record: nothing is read back.
#pragma once

#include "aa_common.h"

#define AA_REDUCE_MANY_MAGIC 0x4D445241  // 'ARDM'

struct AAReduceManyHeader {
  int32_t magic, n, C, layout;
  int32_t E, planes;     // bytes per pixel and planes per item of the call's class: (C, 1) interleaved, (1, C) planar
  int64_t units;         // work units, all items: unit_prefix[n]
  int64_t arena_bytes;   // every item's result, each at a 16-byte aligned offset
  int64_t reserved[3];
};
static_assert(sizeof(AAReduceManyHeader) == 64, "descriptor header is 64 bytes");

// One item.  Byte (row y, column x, channel c) of the BOX is at src + y * row_pitch + x * E + c (interleaved class) or
// src + c * plane_pitch + y * row_pitch + x (planar class); its result is dense at arena + out_off: [rh, rw, C] or [C, rh, rw].
// A work unit is (plane, output row Y, tile of sx output columns): planes * rh * xtiles of them.
struct AAReduceManyItem {
  const uint8_t *src;
  int64_t row_pitch, plane_pitch, out_off;
  int32_t bw, bh, fx, fy, rw, rh;
  int32_t sx, xtiles;   // output columns per tile (their input bytes per row fit kReduceTile; 1 for a wider block) and tiles per row
  uint32_t mult[4];     // [(partial in x) + 2 * (partial in y)]: aa_reduce.hip's four values, the same float32 division
};
static_assert(sizeof(AAReduceManyItem) == 80, "descriptor item is 80 bytes");

size_t aa_reduce_many_desc_size(int64_t n);
int aa_reduce_many_plan_host(int layout, int64_t n, int64_t C, const aa_reduce_item *items, void *desc_host, size_t desc_bytes, size_t *arena_bytes,
                             int64_t *out_offsets);
int aa_launch_reduce_many_u8(const void *desc_host, const void *desc_dev, void *arena_dev, size_t arena_bytes, hipStream_t stream);
