// aa_many_back_bwd.h — the backward of the ragged return path (include/aa_interp.h, "ragged predictions back, backward",
// aa_back_many_bwd_plan): N gradients [K, oh_i, ow_i] of the resampled items back to N canvases [K, H_i, W_i], each the gather-form
// backward of its region (AA_TABLE_F32 adjoint tables) and +0.0 everywhere else.  The packed descriptor block the planner writes on the
// host and the kernels read on the device:
//   [ AABackBwdHeader : 64 B ][ AABackBwdItem x n ][ int64 unit0[n + 1] ]
// unit0[i] is the first work unit of item i; a unit is a tile of AA_BACK_BWD_ROWS canvas rows times AA_BACK_BWD_COLS canvas columns of
// an item's WHOLE canvas (not of its region: the units of an item write every cell of its canvas).  Everything a kernel needs about an
// item is in its record: nothing is read back.
#pragma once

#include "aa_many_back.h"

#define AA_BACK_BWD_MAGIC 0x44574242  // 'BBWD'
#define AA_BACK_BWD_THREADS 256       // lanes of a workgroup of either kernel
#define AA_BACK_BWD_COLS 64           // canvas columns of a work unit: a wave is one canvas row of it
#define AA_BACK_BWD_ROWS 4            // canvas rows of a work unit: the waves of a workgroup
static_assert(AA_BACK_BWD_COLS * AA_BACK_BWD_ROWS == AA_BACK_BWD_THREADS, "a lane per canvas cell of a unit");

struct AABackBwdHeader {
  int32_t magic, n, K, filter;
  int32_t out_layout;  // AA_NCHW: planes [K, H, W]; AA_NHWC: interleaved classes [H, W, K]
  int32_t out_dtype;   // aa_dtype of an output element
  int32_t dense;       // 1: items one after the other (a batch tensor); 0: each on a 16-byte boundary (an arena)
  int32_t reserved0;
  int64_t units;       // unit0[n]: the workgroups of the gather
  int64_t ws_bytes;    // the table arena: per item with a gradient its H table, its W table, then their adjoints
  int64_t out_bytes;
  int64_t reserved;
};
static_assert(sizeof(AABackBwdHeader) == 64, "descriptor header is 64 bytes");

// One item.  grad is class 0, row 0, column 0 of its gradient [K, oh, ow], class k, row r, column c at grad + k * stride_ch +
// r * stride_row + c ELEMENTS; null: the item has no gradient, its canvas is all +0.0, it has no tables and its region is not looked at.
// Its forward tables are packed tables of include/aa_interp.h's format (header, xmin, xsize, float weights; no gather section) at tab_h
// (h -> oh) and tab_w (w -> ow) of the workspace, rows ksize floats long; their adjoints, the same format with h (w) rows of trk floats,
// at tr_h and tr_w.  out_off: bytes from the output's start.
struct AABackBwdItem {
  const void *grad;
  int64_t stride_ch, stride_row;
  int64_t tab_h, tab_w, tr_h, tr_w, out_off;
  int32_t H, W;            // the canvas
  int32_t y0, x0, h, w;    // the region of it the forward read
  int32_t oh, ow;          // the gradient
  int32_t ksize_h, ksize_w, trk_h, trk_w;
  float scale_h, scale_w;  // area_pixel_compute_scale<float>: (float)in / (float)out
  int32_t flags;           // AA_MANY_FLIP_X
  int32_t xtiles;          // ceil(W / AA_BACK_BWD_COLS)
};
static_assert(sizeof(AABackBwdItem) == 128, "descriptor item is 128 bytes");

size_t aa_back_bwd_desc_size(int64_t n);
int aa_back_bwd_plan_host(int filter, int out_layout, int64_t n, int64_t K, const aa_back_bwd_item *items, int out_dtype, int dense, void *desc_host,
                          size_t desc_bytes, size_t *workspace_bytes, size_t *out_bytes, int64_t *out_offsets);
int aa_launch_back_many_bwd(const void *desc_host, const void *desc_dev, int grad_dtype, void *out_dev, size_t out_bytes, void *workspace_dev,
                            size_t workspace_bytes, hipStream_t stream);
