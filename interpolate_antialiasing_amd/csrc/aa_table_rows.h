// aa_table_rows.h — one row of an AA_TABLE_F32 weight table and one row of an adjoint (gather-form) table, as device functions: what
// aa_tables.hip's kernels run per index and what the ragged embedding call's table kernel (aa_embed_many.hip) runs for every item in one
// launch.  Each is written here once, so the tables of the two are the same bits.  Device-only, in the unnamed namespace like the
// kernels that use it; for files built with -ffp-contract=off (a fused multiply-add in `center` or the filter argument moves a window).
#pragma once

#include "aa_common.h"
#include "aa_pil_coeffs.h"

namespace {

__device__ inline int interp_size_of(int filter) { return aa_filter_info(filter).interp_size; }

// Reference arithmetic, scalar_t = float (s2.2:207-209, :242, :253-278).  Every promotion spelled out.
__device__ void table_build_f32_one(int i, int filter, int in_size, int out_size, int ksize, float scale, char *table) {
  using aa_coeffs::apply_filter;
  int32_t *xmin_p = (int32_t *)(table + aa_table_xmin_off());
  int32_t *xsize_p = (int32_t *)(table + aa_table_xsize_off(out_size));
  float *w = (float *)(table + aa_table_w_off(out_size)) + (size_t)i * ksize;
  int32_t *max_taps = &((aa_table_header *)table)->max_taps;

  const int interp_size = interp_size_of(filter);
  const float support = (scale >= 1.0) ? (float)((interp_size * 0.5) * (double)scale) : (float)(interp_size * 0.5);
  const float invscale = (scale >= 1.0) ? (float)(1.0 / (double)scale) : 1.0f;

  const float center = (float)((double)scale * ((double)i + 0.5));
  long long xmin = (long long)((double)(float)(center - support) + 0.5);
  if (xmin < 0) xmin = 0;
  long long xmax = (long long)((double)(float)(center + support) + 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  xmin_p[i] = (int32_t)xmin;
  xsize_p[i] = (int32_t)xmax;

  float total_w = 0.0f;
  int j = 0;
  for (; j < xmax && j < ksize; j++) {
    const float t = (float)((float)(j + xmin) - center);
    const float arg = (float)(((double)t + 0.5) * (double)invscale);
    const float wj = apply_filter<float>(filter, arg);
    w[j] = wj;
    total_w = (float)(total_w + wj);
  }
  if (total_w != 0.0f) {
    for (int q = 0; q < j; q++) w[q] = (float)((double)w[q] / (double)total_w);
  }
  for (; j < ksize; j++) w[j] = 0.0f;
  atomicMax(max_taps, (int32_t)(xmax > 1 ? xmax : 1));
}

// ---- adjoint (gather-form) table -----------------------------------------------------------------------
// For input index x: outputs whose window [xmin, xmin+max(xsize,1)) holds x form a contiguous range because
// xmin[] and xmin[]+xsize[] are non-decreasing.  tmin[x] = first such output, tsize[x] = their count,
// tw[x][k] = w[tmin+k][x - xmin[tmin+k]].
template <typename WT>
__device__ void table_transpose_one(int x, const char *fwd, int32_t *tmin, int32_t *tsize, WT *tw_all, int32_t *max_taps, int out_size, int ksize,
                                    int tr_ksize) {
  const int32_t *xmin = (const int32_t *)(fwd + aa_table_xmin_off());
  const int32_t *xsize = (const int32_t *)(fwd + aa_table_xsize_off(out_size));
  const WT *w = (const WT *)(fwd + aa_table_w_off(out_size));
  WT *tw = tw_all + (size_t)x * tr_ksize;

  // lo = first o with xmin[o] + max(xsize[o],1) > x
  int lo = 0, hi = out_size;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const int xs = xsize[mid] > 1 ? xsize[mid] : 1;
    if (xmin[mid] + xs > x) hi = mid; else lo = mid + 1;
  }
  const int first = lo;
  // end = first o with xmin[o] > x
  lo = first; hi = out_size;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (xmin[mid] > x) hi = mid; else lo = mid + 1;
  }
  int cnt = lo - first;
  if (cnt < 0) cnt = 0;
  // header.max_taps gets the count BEFORE the clamp: a row capacity short of it (tr_ksize not from aa_table_transposed_ksize, or that
  // estimate wrong) would drop gradient taps, so the host compares max_taps with tr_ksize and refuses the table (AA_ERR_KSIZE)
  atomicMax(max_taps, cnt > 1 ? cnt : 1);
  if (cnt > tr_ksize) cnt = tr_ksize;  // (memory safety only: such a table is never handed to a kernel)
  tmin[x] = cnt > 0 ? first : (first < out_size ? first : out_size - 1);  // (kept monotone: the span measurement and the fused kernels' segments rely on it)
  tsize[x] = cnt;
  int k = 0;
  for (; k < cnt; k++) {
    const int o = first + k;
    tw[k] = w[(size_t)o * ksize + (x - xmin[o])];
  }
  for (; k < tr_ksize; k++) tw[k] = (WT)0;
}

}  // namespace
