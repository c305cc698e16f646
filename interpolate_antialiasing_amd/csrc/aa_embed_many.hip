// aa_embed_many.hip — one learned position grid [H0, W0, D] resampled to N token grids, forward and backward, for native-resolution
// vision transformers: what follows resize_many_to_patches.  The arithmetic is the reference's fp32 passes (aa_generic.hip's contract):
// AA_TABLE_F32 tables, the horizontal pass first, an fp32 intermediate, tap 0 unconditionally and taps 1 .. xsize - 1 in order, product
// and sum rounded apart (-ffp-contract=off), one round-to-nearest-even at the store.  Two launches each way whatever N:
//   1. embed_tables  one workgroup per (item, axis): the rows of the item's forward table (table_build_f32_one), and for the backward,
//                    after a barrier, the rows of its adjoint (table_transpose_one) — aa_table_rows.h's device functions, the ones
//                    aa_tables.hip runs, so item i's tables are the bits aa_table_build and aa_table_transpose give its shape;
//   2. embed_fwd     one lane per (token row of the output, AA_EMBED_VEC channels): the token's two windows, and the vertical sum of
//                    horizontal sums.  No intermediate is staged: a lane recomputes the horizontal sum of each tap row, the same
//                    operations in the same order as the two-pass form, so the same bits; the source grid is small and stays cached.
//      embed_bwd     64 lanes of (source cell, AA_EMBED_VEC channels) per workgroup, eight waves: the waves share out the items, each
//                    computing b_i of its items from the adjoint rows of the cell — the gather form's horizontal pass over the
//                    gradient's token columns, then its vertical pass — and the first wave adds them in ascending order into a
//                    register, acc = b_0, acc = acc + b_i; one store, no atomics, so the result does not depend on the launch shape.
// A lane owns AA_EMBED_VEC consecutive channels when D and every address allow vector accesses, one channel otherwise.
// Shared with the other ragged calls: aa_many_dev.h (the item of a row, the element types), aa_many_host.h (the block, the launch checks);
// with the other float ragged calls: aa_float_many_dev.h (the table kernels' body, table_row, the element helpers), aa_float_many_host.h
// (the float types, the tables of an item in a plan).

#include <string.h>

#include "aa_embed_many.h"
#include "aa_float_many_dev.h"
#include "aa_float_many_host.h"

namespace {

// ---- 1. tables ---------------------------------------------------------------------------------------------------------------------------
// Workgroup 2 i builds item i's H axis, 2 i + 1 its W axis: the shared body, with adjoints for the backward.
__global__ void __launch_bounds__(AA_EMBED_THREADS) embed_tables(const AAEmbedItem *items, char *ws, int H0, int W0, int filter, int adjoints) {
  const AAEmbedItem &it = items[blockIdx.x >> 1];
  const bool horiz = blockIdx.x & 1;
  const TableAxis ax = {horiz ? W0 : H0, horiz ? it.gw : it.gh, horiz ? it.ksize_w : it.ksize_h, horiz ? it.trk_w : it.trk_h,
                        horiz ? it.scale_w : it.scale_h, ws + (horiz ? it.tab_w : it.tab_h), ws + (horiz ? it.tr_w : it.tr_h)};
  table_axis_build<AA_EMBED_THREADS>(ax, filter, adjoints);
}

// ---- the sum both directions share ---------------------------------------------------------------------------------------------------------
// (aa_float_many_dev.h's class_sums<T, V, true> is this sum, but through it the float16-input kernels compile to other code, embed_bwd
// 62 -> 53 VGPRs and embed_fwd 40 -> 33: profiles/float_ragged_shared_refactor.txt.  So this file keeps its own.)
// acc = the vertical sum over ry's window of the horizontal sums over rx's window, for V channels from p = element (row ry.x0, pixel
// rx.x0, the lane's first channel); rows `prow` and pixels `ppx` elements apart.  hs is the fp32 intermediate of the two-pass form.
template <typename T, int V>
__device__ inline void window_sums(const T *p, int64_t prow, int64_t ppx, const Row &ry, const Row &rx, float (&acc)[V]) {
  for (int j = 0; j < ry.n; j++) {
    const T *rp = p + j * prow;
    float hs[V];
    Vec<T, V> e = *(const Vec<T, V> *)rp;
    const float w0 = rx.w[0];
#pragma unroll
    for (int c = 0; c < V; c++) hs[c] = to_f32(e.v[c]) * w0;
    for (int k = 1; k < rx.n; k++) {
      e = *(const Vec<T, V> *)(rp + k * ppx);
      const float wk = rx.w[k];
#pragma unroll
      for (int c = 0; c < V; c++) hs[c] = hs[c] + to_f32(e.v[c]) * wk;
    }
    const float wj = ry.w[j];
#pragma unroll
    for (int c = 0; c < V; c++) acc[c] = j == 0 ? hs[c] * wj : acc[c] + hs[c] * wj;
  }
}

template <typename T, int V> __device__ inline void store_vec(T *p, const float (&a)[V]) {
  Vec<T, V> r;
#pragma unroll
  for (int c = 0; c < V; c++) r.v[c] = to_elem<T>(a[c]);
  *(Vec<T, V> *)p = r;
}

struct EmbedArgs {
  const AAEmbedItem *items;
  const int64_t *tok0;
  const char *ws;
  const void *in;
  void *out;
  int64_t stride_row, stride_px;  // of the forward's source, in elements
  int64_t jobs;                   // lanes with work
  int n, D, DV, H0, W0, pad_to;
};

// ---- 2. forward ----------------------------------------------------------------------------------------------------------------------------
template <typename TIn, typename TOut, int V>
__global__ void __launch_bounds__(AA_EMBED_THREADS) embed_fwd(EmbedArgs a) {
  const int64_t job = (int64_t)blockIdx.x * AA_EMBED_THREADS + threadIdx.x;
  if (job >= a.jobs) return;
  const int64_t row = job / a.DV;
  const int dv = (int)(job - row * a.DV);
  int item;
  int64_t t;
  if (a.pad_to) {
    item = (int)(row / a.pad_to);
    t = row - (int64_t)item * a.pad_to;
  } else {
    item = aa_unit_item(a.tok0, a.n, row);
    t = row - a.tok0[item];
  }
  const AAEmbedItem &it = a.items[item];
  float acc[V];
#pragma unroll
  for (int c = 0; c < V; c++) acc[c] = 0.0f;  // (a pad row: +0.0)
  if (t < (int64_t)it.gh * it.gw) {
    const int ty = (int)(t / it.gw), tx = (int)(t - (int64_t)ty * it.gw);
    const Row ry = table_row(a.ws + it.tab_h, a.H0, it.gh, it.ksize_h, ty), rx = table_row(a.ws + it.tab_w, a.W0, it.gw, it.ksize_w, tx);
    window_sums<TIn, V>((const TIn *)a.in + ry.x0 * a.stride_row + rx.x0 * a.stride_px + dv * V, a.stride_row, a.stride_px, ry, rx, acc);
  }
  store_vec<TOut, V>((TOut *)a.out + row * a.D + dv * V, acc);
}

// ---- 2'. backward --------------------------------------------------------------------------------------------------------------------------
// The items' terms b_i do not depend on each other, only their sum has an order: wave s of a workgroup computes b_i for the items
// i = s, s + kBwdSlots, .. of the workgroup's 64 lanes (cell, channels) and leaves it in LDS, and wave 0 adds each round's terms in
// ascending order.  A walk of all N items by one lane was 0.40 ms on the --embed workload (64 items, three waves a CU); this is the same
// sum with kBwdSlots times the loads in flight.
constexpr int kBwdSlots = 8, kBwdLanes = 64;
template <typename TG, typename TOut, int V>
__global__ void __launch_bounds__(kBwdLanes *kBwdSlots) embed_bwd(EmbedArgs a) {
  __shared__ float part[kBwdSlots][V][kBwdLanes];
  const int lane = (int)threadIdx.x % kBwdLanes, slot = (int)threadIdx.x / kBwdLanes;  // (slot: uniform per wave)
  const int64_t job = (int64_t)blockIdx.x * kBwdLanes + lane;
  const bool live = job < a.jobs;  // (a lane without work computes nothing, but meets every barrier)
  const int64_t cell = live ? job / a.DV : 0;
  const int dv = live ? (int)(job - cell * a.DV) : 0;
  const int y = (int)(cell / a.W0), x = (int)(cell - (int64_t)y * a.W0);
  float acc[V];
#pragma unroll
  for (int c = 0; c < V; c++) acc[c] = -0.0f;  // (-0) + b == b exactly, for every b: the first item is an assignment
  for (int i0 = 0; i0 < a.n; i0 += kBwdSlots) {
    const int i = i0 + slot;
    if (live && i < a.n) {
      const AAEmbedItem &it = a.items[i];
      const int64_t row0 = a.pad_to ? (int64_t)i * a.pad_to : a.tok0[i];
      // the adjoint rows of the cell: the token rows [ry.x0, ry.x0 + ry.n) and columns [rx.x0, rx.x0 + rx.n) whose windows hold it
      const Row ry = table_row(a.ws + it.tr_h, it.gh, a.H0, it.trk_h, y), rx = table_row(a.ws + it.tr_w, it.gw, a.W0, it.trk_w, x);
      float b[V];
      window_sums<TG, V>((const TG *)a.in + (row0 + (int64_t)ry.x0 * it.gw + rx.x0) * a.D + dv * V, (int64_t)it.gw * a.D, a.D, ry, rx, b);
#pragma unroll
      for (int c = 0; c < V; c++) part[slot][c][lane] = b[c];
    }
    __syncthreads();
    if (slot == 0) {
      const int m = a.n - i0 < kBwdSlots ? a.n - i0 : kBwdSlots;
      for (int s = 0; s < m; s++) {
#pragma unroll
        for (int c = 0; c < V; c++) acc[c] = acc[c] + part[s][c][lane];
      }
    }
    __syncthreads();  // (the round's terms have been read)
  }
  if (slot == 0 && live) store_vec<TOut, V>((TOut *)a.out + cell * a.D + dv * V, acc);
}

template <typename TIn, typename TOut, int V> void launch_as(bool bwd, const EmbedArgs &a, hipStream_t stream) {
  if (bwd) hipLaunchKernelGGL((embed_bwd<TIn, TOut, V>), dim3((unsigned)((a.jobs + kBwdLanes - 1) / kBwdLanes)), dim3(kBwdLanes * kBwdSlots), 0, stream, a);
  else hipLaunchKernelGGL((embed_fwd<TIn, TOut, V>), dim3((unsigned)((a.jobs + AA_EMBED_THREADS - 1) / AA_EMBED_THREADS)), dim3(AA_EMBED_THREADS), 0, stream, a);
}
template <int V> void launch_in(int in_dtype, int out_dtype, bool bwd, const EmbedArgs &a, hipStream_t stream) {
  with_float_type(in_dtype, [&](auto in) {
    with_float_type(out_dtype, [&](auto out) { launch_as<tag_t<decltype(in)>, tag_t<decltype(out)>, V>(bwd, a, stream); });
  });
}

}  // namespace

// ---- host: the planner -------------------------------------------------------------------------------------------------------------------
size_t aa_embed_desc_size(int64_t n) { return aa_desc_size(sizeof(AAEmbedHeader), sizeof(AAEmbedItem), n); }

int aa_embed_plan_host(int filter, int64_t n, int64_t D, int64_t H0, int64_t W0, const int64_t *grids, int64_t pad_to, void *desc_host,
                       size_t desc_bytes, size_t *workspace_bytes, int64_t *out_rows) {
  if (!aa_filter_valid(filter)) return AA_ERR_BAD_FILTER;
  if (n < 0 || n > kAAManyMax || D <= 0 || D > kAAManyMax || H0 <= 0 || W0 <= 0 || H0 > kAAManyMax || W0 > kAAManyMax || pad_to < 0 ||
      pad_to > INT32_MAX)
    return AA_ERR_BAD_SHAPE;
  if (!desc_host || !workspace_bytes || !out_rows || (n > 0 && !grids)) return AA_ERR_NULL;
  if (desc_bytes < aa_embed_desc_size(n)) return AA_ERR_WORKSPACE;
  AAEmbedHeader *hd = (AAEmbedHeader *)desc_host;
  AAEmbedItem *items = (AAEmbedItem *)(hd + 1);
  int64_t *tok0 = (int64_t *)(items + n);
  size_t off = 0;
  int64_t rows = 0;
  for (int64_t i = 0; i < n; i++) {
    const int64_t gh = grids[2 * i], gw = grids[2 * i + 1];
    if (gh <= 0 || gw <= 0 || gh > kAAManyMax || gw > kAAManyMax || gh * gw > kAAManyMax) return AA_ERR_BAD_SHAPE;
    if (pad_to > 0 && gh * gw > pad_to) return AA_ERR_BAD_SHAPE;
    AAEmbedItem it;
    memset(&it, 0, sizeof(it));
    it.gh = (int32_t)gh; it.gw = (int32_t)gw;
    int rc = plan_forward_tables(filter, H0, W0, gh, gw, it, off);
    if (rc == AA_OK) rc = plan_adjoint_tables(filter, H0, W0, gh, gw, it, off);
    if (rc != AA_OK) return rc;
    items[i] = it;
    tok0[i] = rows;
    rows += gh * gw;
  }
  tok0[n] = rows;
  if (pad_to > 0) rows = n * pad_to;
  // (one grid each way, a workgroup AA_EMBED_THREADS single-channel lanes of the forward or 64 of the backward; so every element
  // offset fits 63 bits)
  if (rows > (int64_t)INT32_MAX * AA_EMBED_THREADS / D || H0 * W0 > (int64_t)INT32_MAX * 64 / D) return AA_ERR_BAD_SHAPE;
  memset(hd, 0, sizeof(*hd));
  hd->magic = AA_EMBED_MAGIC;
  hd->n = (int32_t)n; hd->D = (int32_t)D; hd->H0 = (int32_t)H0; hd->W0 = (int32_t)W0;
  hd->filter = filter;
  hd->pad_to = (int32_t)pad_to;
  hd->out_rows = rows;
  hd->ws_bytes = (int64_t)off;
  *workspace_bytes = off;
  *out_rows = rows;
  return AA_OK;
}

// ---- host: the two launches of a direction -----------------------------------------------------------------------------------------------
// What both directions check of a planned block, all before any launch, and what they launch first: the table kernel (nothing for n == 0).
static int embed_prologue(const AAEmbedHeader *hd, const void *desc_dev, const void *in_dev, int in_dtype, void *out_dev, int out_dtype,
                          void *workspace_dev, size_t workspace_bytes, int adjoints, hipStream_t stream) {
  if (hd->magic != AA_EMBED_MAGIC || !aa_filter_valid(hd->filter) || hd->n < 0 || hd->D <= 0 || hd->H0 <= 0 || hd->W0 <= 0 || hd->pad_to < 0)
    return AA_ERR_BAD_SHAPE;
  if (!float_dtype(in_dtype) || !float_dtype(out_dtype)) return AA_ERR_BAD_DTYPE;
  const int rc = aa_many_check_launch(hd->n, desc_dev, out_dev, workspace_dev, workspace_bytes, hd->ws_bytes, elem_bytes(out_dtype));
  if (rc != AA_OK || hd->n == 0) return rc;
  if (!in_dev) return AA_ERR_NULL;
  if ((uintptr_t)in_dev % elem_bytes(in_dtype)) return AA_ERR_STRIDES;
  const AADescView<AAEmbedItem> v = aa_desc_view<AAEmbedHeader, AAEmbedItem>(desc_dev, hd->n);
  hipLaunchKernelGGL(embed_tables, dim3(2u * (unsigned)hd->n), dim3(AA_EMBED_THREADS), 0, stream, v.items, (char *)workspace_dev, (int)hd->H0,
                     (int)hd->W0, (int)hd->filter, adjoints);
  return AA_OK;
}

static int embed_launch(const AAEmbedHeader *hd, const void *desc_dev, bool bwd, const void *in_dev, int in_dtype, int64_t stride_row,
                        int64_t stride_px, void *out_dev, int out_dtype, const void *workspace_dev, int64_t cells, hipStream_t stream) {
  const AADescView<AAEmbedItem> v = aa_desc_view<AAEmbedHeader, AAEmbedItem>(desc_dev, hd->n);
  const size_t ei = elem_bytes(in_dtype), eo = elem_bytes(out_dtype);
  const bool vec = hd->D % AA_EMBED_VEC == 0 && (uintptr_t)in_dev % (AA_EMBED_VEC * ei) == 0 && (uintptr_t)out_dev % (AA_EMBED_VEC * eo) == 0 &&
                   stride_row % AA_EMBED_VEC == 0 && stride_px % AA_EMBED_VEC == 0;
  EmbedArgs a;
  a.items = v.items; a.tok0 = v.prefix; a.ws = (const char *)workspace_dev;
  a.in = in_dev; a.out = out_dev;
  a.stride_row = stride_row; a.stride_px = stride_px;
  a.n = hd->n; a.D = hd->D; a.DV = vec ? hd->D / AA_EMBED_VEC : hd->D;
  a.H0 = hd->H0; a.W0 = hd->W0; a.pad_to = hd->pad_to;
  a.jobs = cells * a.DV;
  if (a.jobs > (int64_t)INT32_MAX * (bwd ? kBwdLanes : AA_EMBED_THREADS)) return AA_ERR_BAD_SHAPE;  // (never: the planner's bound)
  if (vec) launch_in<AA_EMBED_VEC>(in_dtype, out_dtype, bwd, a, stream);
  else launch_in<1>(in_dtype, out_dtype, bwd, a, stream);
  AA_HIP_CHECK_LAUNCH();
  return AA_OK;
}

int aa_launch_embed_many(const void *desc_host, const void *desc_dev, const void *embed_dev, int in_dtype, int64_t stride_row, int64_t stride_px,
                         void *out_dev, int out_dtype, void *workspace_dev, size_t workspace_bytes, hipStream_t stream) {
  const AAEmbedHeader *hd = (const AAEmbedHeader *)desc_host;
  if (stride_row < 0 || stride_px < 0) return AA_ERR_STRIDES;
  const int rc = embed_prologue(hd, desc_dev, embed_dev, in_dtype, out_dev, out_dtype, workspace_dev, workspace_bytes, 0, stream);
  if (rc != AA_OK || hd->n == 0) return rc;
  return embed_launch(hd, desc_dev, false, embed_dev, in_dtype, stride_row, stride_px, out_dev, out_dtype, workspace_dev, hd->out_rows, stream);
}

int aa_launch_embed_many_bwd(const void *desc_host, const void *desc_dev, const void *grad_dev, int grad_dtype, void *grad_embed_dev, int out_dtype,
                             void *workspace_dev, size_t workspace_bytes, hipStream_t stream) {
  const AAEmbedHeader *hd = (const AAEmbedHeader *)desc_host;
  const int rc = embed_prologue(hd, desc_dev, grad_dev, grad_dtype, grad_embed_dev, out_dtype, workspace_dev, workspace_bytes, 1, stream);
  if (rc != AA_OK || hd->n == 0) return rc;
  return embed_launch(hd, desc_dev, true, grad_dev, grad_dtype, 0, 0, grad_embed_dev, out_dtype, workspace_dev, (int64_t)hd->H0 * hd->W0, stream);
}
