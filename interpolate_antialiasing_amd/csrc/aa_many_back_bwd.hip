// aa_many_back_bwd.hip — the backward of aa_many_back.hip's values: N gradients [K, oh_i, ow_i] back to N canvases [K, H_i, W_i].
// Inside an item's region the result is the gather-form backward of the single-shape call in fp32 (aa_backward.hip's contract, as
// aa_embed_many.hip's embed_bwd states it): AA_TABLE_F32 adjoint tables, the horizontal adjoint pass first, an fp32 intermediate, tap 0
// unconditionally and taps 1 .. n - 1 in ascending order, product and sum rounded apart (-ffp-contract=off), one
// round-to-nearest-even at the store; outside it, and for an item without a gradient, +0.0.  No atomics.  Two launches whatever N and
// whatever the sizes:
//   1. back_bwd_tables  one workgroup per (item, axis): the rows of the item's forward table (table_build_f32_one), a barrier, the rows
//                       of its adjoint (table_transpose_one) — the body embed_tables runs, with the source size per item
//                       (aa_table_rows.h's device functions, so the tables are the bits aa_table_build and aa_table_transpose give the
//                       shape).  An item without a gradient has no tables: its two workgroups leave at once;
//   2. back_bwd_gather  one workgroup per work unit, AA_BACK_BWD_ROWS x AA_BACK_BWD_COLS cells of an item's CANVAS, a lane per cell, a
//                       wave per canvas row.  The units of an item tile its whole canvas, so this one kernel writes every element of
//                       the output: a cell outside the region stores K zeros, a cell inside it the K sums.  A cell's sums are the
//                       vertical sum, over the adjoint row of its y, of the horizontal sums over the adjoint row of its x, the classes
//                       AA_BACK_UNROLL at a time; the lane recomputes the horizontal sum of each tap row, the same operations in the
//                       same order as the two-pass form, so the same bits, and the fp32 intermediate never reaches memory.
// What a workgroup shares: the lanes of a wave read, tap by tap, addresses ow / w elements apart in one gradient row, so a wave's loads
// of a tap row fall into one segment of that row of about 64 ow / w elements and every line of it is used by the taps that follow; the
// four waves are four neighbouring canvas rows, whose adjoint rows overlap (by half where the item was enlarged).  The caches serve
// most of that, not all: the L2 hit rate is 90 %, and what the L2s fetch is 2.4 to 3.1 times the gradients' bytes.
// Nothing is staged in LDS: adjoint rows have no fixed length (a 1 x 1 region has ONE row of ow taps), so a staged segment needs a
// chunk loop of its own; that form was not built, and the strided scalar loads are what bounds this kernel.
// A flipped item reads gradient column ow - 1 - c for column c.  Every element offset is 64-bit.  Stores are one element a lane, so an
// output on any element boundary is served and the 16-byte gaps between the items of an arena are never written.
// Shared with the other ragged calls: aa_many_dev.h (the item of a unit, the element types), aa_many_host.h (the block, the launch checks);
// with the other float ragged calls: aa_float_many_dev.h (the table kernels' body, table_row, class_sums), aa_float_many_host.h (the
// float types, the tables of an item in a plan).

#include <string.h>

#include "aa_many_back_bwd.h"
#include "aa_float_many_dev.h"
#include "aa_float_many_host.h"

namespace {

// ---- 1. tables ---------------------------------------------------------------------------------------------------------------------------
// Workgroup 2 i builds item i's H axis, 2 i + 1 its W axis: the shared body with adjoints, the source size per item.
__global__ void __launch_bounds__(AA_BACK_BWD_THREADS) back_bwd_tables(const AABackBwdItem *items, char *ws, int filter) {
  const AABackBwdItem &it = items[blockIdx.x >> 1];
  if (!it.grad) return;  // (uniform per workgroup: before every barrier)
  const bool horiz = blockIdx.x & 1;
  const TableAxis ax = {horiz ? it.w : it.h, horiz ? it.ow : it.oh, horiz ? it.ksize_w : it.ksize_h, horiz ? it.trk_w : it.trk_h,
                        horiz ? it.scale_w : it.scale_h, ws + (horiz ? it.tab_w : it.tab_h), ws + (horiz ? it.tr_w : it.tr_h)};
  table_axis_build<AA_BACK_BWD_THREADS>(ax, filter, 1);
}

struct BwdArgs {
  const AABackBwdItem *items;
  const int64_t *unit0;
  const char *ws;
  char *out;
  int n, K;
};

// ---- 2. the gather -------------------------------------------------------------------------------------------------------------------------
template <typename TG, typename TOut, bool NHWC>
__global__ void __launch_bounds__(AA_BACK_BWD_THREADS) back_bwd_gather(BwdArgs a) {
  constexpr int U = AA_BACK_UNROLL;
  const int64_t unit = blockIdx.x;
  const int item = aa_unit_item(a.unit0, a.n, unit);
  const AABackBwdItem &it = a.items[item];
  const int64_t u = unit - a.unit0[item];
  const int ty = (int)(u / it.xtiles), tx = (int)(u - (int64_t)ty * it.xtiles);
  const int Y = ty * AA_BACK_BWD_ROWS + (int)threadIdx.x / AA_BACK_BWD_COLS, X = tx * AA_BACK_BWD_COLS + (int)threadIdx.x % AA_BACK_BWD_COLS;
  if (Y >= it.H || X >= it.W) return;  // (no barrier below)
  // class k of the lane's cell at o[k * kstep]
  const int64_t cell = (int64_t)Y * it.W + X, kstep = NHWC ? 1 : (int64_t)it.H * it.W;
  TOut *o = (TOut *)(a.out + it.out_off) + (NHWC ? cell * a.K : cell);
  const int y = Y - it.y0, x = X - it.x0;
  if (!it.grad || y < 0 || y >= it.h || x < 0 || x >= it.w) {
    const TOut zero = to_elem<TOut>(0.0f);
    for (int k = 0; k < a.K; k++) o[k * kstep] = zero;
    return;
  }
  // the adjoint rows of the cell: the gradient rows [ry.x0, ry.x0 + ry.n) and columns [rx.x0, rx.x0 + rx.n) whose windows hold it
  const Row ry = table_row(a.ws + it.tr_h, it.oh, it.h, it.trk_h, y), rx = table_row(a.ws + it.tr_w, it.ow, it.w, it.trk_w, x);
  const bool flip = it.flags & AA_MANY_FLIP_X;
  const int64_t sch = it.stride_ch, prow = it.stride_row, ppx = flip ? -1 : 1;
  const TG *p = (const TG *)it.grad + ry.x0 * prow + (flip ? it.ow - 1 - rx.x0 : rx.x0);
  int k = 0;
  for (; k + U <= a.K; k += U) {
    float acc[U];
    class_sums<TG, U, false>(p + k * sch, sch, prow, ppx, ry, rx, acc);
#pragma unroll
    for (int c = 0; c < U; c++) o[(k + c) * kstep] = to_elem<TOut>(acc[c]);
  }
  for (; k < a.K; k++) {
    float acc[1];
    class_sums<TG, 1, false>(p + k * sch, sch, prow, ppx, ry, rx, acc);
    o[k * kstep] = to_elem<TOut>(acc[0]);
  }
}

template <typename TG, typename TOut> void launch_as(bool nhwc, const BwdArgs &a, unsigned units, hipStream_t stream) {
  if (nhwc) hipLaunchKernelGGL((back_bwd_gather<TG, TOut, true>), dim3(units), dim3(AA_BACK_BWD_THREADS), 0, stream, a);
  else hipLaunchKernelGGL((back_bwd_gather<TG, TOut, false>), dim3(units), dim3(AA_BACK_BWD_THREADS), 0, stream, a);
}

}  // namespace

// ---- host: the planner -------------------------------------------------------------------------------------------------------------------
size_t aa_back_bwd_desc_size(int64_t n) { return aa_desc_size(sizeof(AABackBwdHeader), sizeof(AABackBwdItem), n); }

int aa_back_bwd_plan_host(int filter, int out_layout, int64_t n, int64_t K, const aa_back_bwd_item *in, int out_dtype, int dense, void *desc_host,
                          size_t desc_bytes, size_t *workspace_bytes, size_t *out_bytes, int64_t *out_offsets) {
  if (!aa_filter_valid(filter)) return AA_ERR_BAD_FILTER;
  if (out_layout != AA_NCHW && out_layout != AA_NHWC) return AA_ERR_BAD_LAYOUT;
  if (n < 0 || n > kAAManyMax || K < 1 || K > kAAManyMax || (dense != 0 && dense != 1)) return AA_ERR_BAD_SHAPE;
  if (!desc_host || !workspace_bytes || !out_bytes || (n > 0 && (!in || !out_offsets))) return AA_ERR_NULL;
  if (desc_bytes < aa_back_bwd_desc_size(n)) return AA_ERR_WORKSPACE;
  const size_t eb = out_dtype == AA_F32 ? 4 : 2;  // (a type that is not stored: refused below, after the items)
  AABackBwdHeader *hd = (AABackBwdHeader *)desc_host;
  AABackBwdItem *items = (AABackBwdItem *)(hd + 1);
  int64_t *unit0 = (int64_t *)(items + n);
  size_t ws = 0, out = 0;
  int64_t units = 0;
  for (int64_t i = 0; i < n; i++) {
    const aa_back_bwd_item &im = in[i];
    if (im.H <= 0 || im.W <= 0 || im.H > kAAManyMax || im.W > kAAManyMax || im.H * im.W > AA_BACK_MAX_ELEMS / K || (im.flags & ~AA_MANY_FLIP_X))
      return AA_ERR_BAD_SHAPE;
    AABackBwdItem it;
    memset(&it, 0, sizeof(it));
    it.H = (int32_t)im.H; it.W = (int32_t)im.W;
    if (im.grad_dev) {  // (an item without a gradient: nothing but its canvas is looked at, and it has no tables)
      if (im.oh <= 0 || im.ow <= 0 || im.oh > kAAManyMax || im.ow > kAAManyMax || im.oh * im.ow > AA_BACK_MAX_ELEMS / K) return AA_ERR_BAD_SHAPE;
      if (im.h <= 0 || im.w <= 0 || im.y0 < 0 || im.x0 < 0 || im.h > im.H || im.w > im.W || im.y0 > im.H - im.h || im.x0 > im.W - im.w)
        return AA_ERR_BAD_SHAPE;
      // (the stride of an axis of one element never matters)
      if ((K > 1 && im.stride_ch < 0) || (im.oh > 1 && im.stride_row < 0)) return AA_ERR_STRIDES;
      it.grad = im.grad_dev;
      it.stride_ch = K > 1 ? im.stride_ch : 0;
      it.stride_row = im.oh > 1 ? im.stride_row : 0;
      it.y0 = (int32_t)im.y0; it.x0 = (int32_t)im.x0; it.h = (int32_t)im.h; it.w = (int32_t)im.w;
      it.oh = (int32_t)im.oh; it.ow = (int32_t)im.ow;
      it.flags = im.flags;
      int rc = plan_forward_tables(filter, im.h, im.w, im.oh, im.ow, it, ws);
      if (rc == AA_OK) rc = plan_adjoint_tables(filter, im.h, im.w, im.oh, im.ow, it, ws);
      if (rc != AA_OK) return rc;
    }
    it.xtiles = (int32_t)((im.W + AA_BACK_BWD_COLS - 1) / AA_BACK_BWD_COLS);
    if (!dense) out = aa_align16(out);
    it.out_off = (int64_t)out;
    out_offsets[i] = (int64_t)out;
    out += (size_t)K * (size_t)im.H * (size_t)im.W * eb;
    if (out > (size_t)AA_BACK_MAX_ELEMS * 8) return AA_ERR_BAD_SHAPE;
    unit0[i] = units;
    units += ((im.H + AA_BACK_BWD_ROWS - 1) / AA_BACK_BWD_ROWS) * (int64_t)it.xtiles;
    if (units > INT32_MAX) return AA_ERR_BAD_SHAPE;  // (one grid)
    items[i] = it;
  }
  unit0[n] = units;
  if (!float_dtype(out_dtype)) return AA_ERR_BAD_DTYPE;
  memset(hd, 0, sizeof(*hd));
  hd->magic = AA_BACK_BWD_MAGIC;
  hd->n = (int32_t)n; hd->K = (int32_t)K; hd->filter = filter;
  hd->out_layout = out_layout; hd->out_dtype = out_dtype; hd->dense = dense;
  hd->units = units;
  hd->ws_bytes = (int64_t)ws;
  hd->out_bytes = (int64_t)out;
  *workspace_bytes = ws;
  *out_bytes = out;
  return AA_OK;
}

// ---- host: the two launches ----------------------------------------------------------------------------------------------------------------
// Every check comes before the first launch.  desc_host is the planned block, so the items' pointers are looked at here, against the
// element of grad_dtype, which the planner did not know.
int aa_launch_back_many_bwd(const void *desc_host, const void *desc_dev, int grad_dtype, void *out_dev, size_t out_bytes, void *workspace_dev,
                            size_t workspace_bytes, hipStream_t stream) {
  const AABackBwdHeader *hd = (const AABackBwdHeader *)desc_host;
  if (hd->magic != AA_BACK_BWD_MAGIC || !aa_filter_valid(hd->filter) || hd->n < 0 || hd->K < 1 || hd->units < 0 || hd->units > INT32_MAX ||
      (hd->out_layout != AA_NCHW && hd->out_layout != AA_NHWC))
    return AA_ERR_BAD_SHAPE;
  if (!float_dtype(grad_dtype) || !float_dtype(hd->out_dtype)) return AA_ERR_BAD_DTYPE;
  const int rc = aa_many_check_launch(hd->n, desc_dev, out_dev, workspace_dev, workspace_bytes, hd->ws_bytes, elem_bytes(hd->out_dtype));
  if (rc != AA_OK || hd->n == 0) return rc;
  if (out_bytes < (size_t)hd->out_bytes) return AA_ERR_WORKSPACE;
  const AABackBwdItem *host_items = (const AABackBwdItem *)(hd + 1);
  const size_t eg = elem_bytes(grad_dtype);
  for (int64_t i = 0; i < hd->n; i++)
    if ((uintptr_t)host_items[i].grad % eg) return AA_ERR_STRIDES;
  const AADescView<AABackBwdItem> v = aa_desc_view<AABackBwdHeader, AABackBwdItem>(desc_dev, hd->n);
  hipLaunchKernelGGL(back_bwd_tables, dim3(2u * (unsigned)hd->n), dim3(AA_BACK_BWD_THREADS), 0, stream, v.items, (char *)workspace_dev, (int)hd->filter);
  AA_HIP_CHECK_LAUNCH();
  BwdArgs a;
  a.items = v.items; a.unit0 = v.prefix; a.ws = (const char *)workspace_dev; a.out = (char *)out_dev;
  a.n = hd->n; a.K = hd->K;
  const bool nhwc = hd->out_layout == AA_NHWC;
  with_float_type(grad_dtype, [&](auto g) {
    with_float_type(hd->out_dtype, [&](auto o) { launch_as<tag_t<decltype(g)>, tag_t<decltype(o)>>(nhwc, a, (unsigned)hd->units, stream); });
  });
  AA_HIP_CHECK_LAUNCH();
  return AA_OK;
}
