// aa_embed_many.h — one learned position grid resampled to N token grids (include/aa_interp.h, "ragged position grids",
// aa_embed_many_plan): the source is ONE [H0, W0, D] float grid, item i is its resample to [gh_i, gw_i] in the reference's fp32
// arithmetic (AA_TABLE_F32 tables), packed as gh_i * gw_i token rows of D channels; the backward is the ordered fp32 sum of the items'
// gather-form adjoints.  The packed descriptor block the planner writes on the host and the kernels read on the device:
//   [ AAEmbedHeader : 64 B ][ AAEmbedItem x n ][ int64 tok0[n + 1] ]
// tok0[i] is the packed row of item i's first token (T_0 + .. + T_(i-1)); with pad_to = L > 0 item i's rows start at i * L instead.
// Everything a kernel needs about an item is in its record: nothing is read back.
#pragma once

#include "aa_common.h"

#define AA_EMBED_MAGIC 0x44424D45  // 'EMBD'
#define AA_EMBED_THREADS 256       // lanes of a workgroup of the table kernel and of the forward
#define AA_EMBED_VEC 4             // channels per lane where D and every address allow it; 1 otherwise

struct AAEmbedHeader {
  int32_t magic, n, D, H0, W0, filter;
  int32_t pad_to;    // 0: packed rows; L > 0: every item has L rows
  int32_t reserved0;
  int64_t out_rows;  // tok0[n], or n * L
  int64_t ws_bytes;  // the table arena: per item the two forward tables, then the two adjoint tables
  int64_t reserved[2];
};
static_assert(sizeof(AAEmbedHeader) == 64, "descriptor header is 64 bytes");

// One item.  Its four tables are packed tables of include/aa_interp.h's format (header, xmin, xsize, float weights; no gather or
// scatter section) at these offsets of the workspace: tab_h is H0 -> gh, tab_w is W0 -> gw, tr_h and tr_w their adjoints (gh -> H0,
// gw -> W0: what aa_table_transpose builds), rows ksize and trk floats long.  Only the backward builds and reads the adjoints.
struct AAEmbedItem {
  int64_t tab_h, tab_w, tr_h, tr_w;
  int32_t gh, gw;
  int32_t ksize_h, ksize_w, trk_h, trk_w;
  float scale_h, scale_w;  // area_pixel_compute_scale<float>: (float)in / (float)out
};
static_assert(sizeof(AAEmbedItem) == 64, "descriptor item is 64 bytes");

size_t aa_embed_desc_size(int64_t n);
int aa_embed_plan_host(int filter, int64_t n, int64_t D, int64_t H0, int64_t W0, const int64_t *grids, int64_t pad_to, void *desc_host,
                       size_t desc_bytes, size_t *workspace_bytes, int64_t *out_rows);
int aa_launch_embed_many(const void *desc_host, const void *desc_dev, const void *embed_dev, int in_dtype, int64_t stride_row, int64_t stride_px,
                         void *out_dev, int out_dtype, void *workspace_dev, size_t workspace_bytes, hipStream_t stream);
int aa_launch_embed_many_bwd(const void *desc_host, const void *desc_dev, const void *grad_dev, int grad_dtype, void *grad_embed_dev, int out_dtype,
                             void *workspace_dev, size_t workspace_bytes, hipStream_t stream);
