// aa_reduce.h — the integer box reduction (aa_reduce.hip: Pillow's Image.reduce for 8-bit channels) as aa_api.hip sees it.
#pragma once

#include "aa_common.h"

// One launch.  The input is read where it lies: rows row_pitch bytes apart, images (AA_NHWC) or planes (AA_NCHW: planes = N * C)
// img_pitch bytes apart; `in` points at the box's first byte.  bw x bh: the box in pixels; the output is dense.
struct AAReduceJob {
  const uint8_t *in;
  uint8_t *out;
  int64_t images;     // N for interleaved pixels, N * C for planes
  int C;              // bytes per pixel (1: planes)
  int bw, bh, fx, fy;
  int64_t row_pitch, img_pitch;
  hipStream_t stream;
};
int aa_launch_reduce_u8(const AAReduceJob &job);
