// aa_many_back_queries.hip — the ragged return path for mask-classification heads (MaskFormer's semantic inference): item i is Q mask
// logits [Q, h_i, w_i] and Q class weights [Q, C].  With R_i the fp32 resample of aa_many_back.hip (K = Q, bit for bit),
//   P[q]       = float16(aa_sigmoid(R_i[q]))         aa_activation.h's sigmoid, then ONE round-to-nearest-even to float16
//   Wh[q, c]   = float16(weights_i[q, c])            round-to-nearest-even; beyond +-65504 it is +-inf
//   S[c, y, x] = sum_q Wh[q, c] * P[q, y, x]         exact products, summed in fp32 by the matrix unit in an order of its own
// and what reaches memory is S rounded once to the output's float type, or its argmax over c by ArgmaxRule's rule (the lowest index of
// the greatest value, a NaN greater than every number and the lowest NaN winning).  Neither the Q probabilities of a pixel nor, for the
// argmax, its C scores are stored.  Two launches whatever n and whatever the sizes:
//   1. queries_tables    one workgroup per (item, axis), back_tables' body (table_axis_build, aa_float_many_dev.h);
//   2. queries_resample  one workgroup per work unit, an output row of an item times AA_BACK_TILE columns; a wave owns 64 of them and
//                        nothing but them, so there is no barrier and a wave wholly beyond ow leaves at once.
//      phase one (VALU)  lane p walks the Q queries of pixel p with each_class — the loop of the per-pixel kernels, a flipped item
//                        mirrored where it is read — and leaves float16(sigmoid) in the wave's LDS tile.  The tile holds
//                        [Qpad / 8][64 pixels][8 queries] halves, Qpad = Q rounded up to 16: the 8 consecutive queries of one pixel
//                        that a lane of phase two feeds the matrix unit are one aligned 16-byte piece, and the pieces of
//                        consecutive pixels are consecutive, so a wave's operand read is two runs of 512 consecutive bytes and has
//                        no bank conflict.  Rows Q .. Qpad - 1 and the lanes beyond ow are ALWAYS written, as +0: what an earlier
//                        workgroup left in LDS may be a NaN, and a NaN times a zero weight is a NaN.
//      phase two (MFMA)  v_mfma_f32_32x32x16_f16, D[32 classes][32 pixels] += A[32 classes][16 queries] . B[16 queries][32 pixels].
//                        Lane l holds of A the class l % 32 and of B the pixel l % 32, both for the queries 8 (l / 32) .. + 7 of the
//                        step; A comes from the item's fp32 weights where they lie (any strides; classes >= C and queries >= Q are
//                        +0, and no address outside the matrix is formed), converted on load, and serves the wave's two pixel blocks.  The class
//                        blocks are the outer loop, so any C takes 2 x 16 accumulator registers.  Of D, register r of lane l is
//                        class 8 (r / 4) + 4 (l / 32) + r % 4 of pixel l % 32: ascending in r, so a lane offers its classes to its
//                        running candidate in ascending order across blocks, classes >= C never; after the last block lane l
//                        exchanges with lane l ^ 32 the candidate of the pixel block the other one stores, merges the two by the
//                        same rule, and stores the label of pixel l.  With reduce 0 the 32 lanes of a half-wave store 32
//                        consecutive pixels of a class plane per register.
// LDS is Qpad * 512 bytes a workgroup (128 KiB at Q = 256), sized per launch and checked against the device's limit.  Every element
// offset is 64-bit.  Plain C++ and vector memory operations only.
// Shared with the other files of the return path: aa_many_back_shared.h.

#include <string.h>

#include "aa_many_back_queries_dev.h"

namespace {

// ---- 1. tables -----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(AA_BACK_THREADS) queries_tables(const AABackItem *items, char *ws, int filter) {
  const AABackItem &it = items[blockIdx.x >> 1];
  const bool horiz = blockIdx.x & 1;
  const TableAxis ax = {horiz ? it.w : it.h, horiz ? it.ow : it.oh, horiz ? it.ksize_w : it.ksize_h, 0, horiz ? it.scale_w : it.scale_h,
                        ws + (horiz ? it.tab_w : it.tab_h), nullptr};
  table_axis_build<AA_BACK_THREADS>(ax, filter, 0);
}

struct QueryArgs {
  const AABackItem *items;
  const int64_t *unit0;
  const AABackQueryWeights *weights;
  const char *ws;
  char *arena;
  int n, Q, C;
};

// ---- the epilogues (Tile, d_class, Scores, Candidate, merged and LabelCandidates: aa_many_back_queries_dev.h) ---------------------------
template <typename TLabel> struct Labels : LabelCandidates {
  TLabel *out;
  __device__ Labels(void *o, const Tile &t_) : LabelCandidates(t_), out((TLabel *)o) {}
  __device__ void done() {
    const int idx = winner();
    const int px = t.x0 + t.lane;
    if (px < t.ow) out[t.row + px] = (TLabel)idx;
  }
};

// ---- 2. the resample -----------------------------------------------------------------------------------------------------------------------
template <typename TIn, bool VEC, typename Epi>
__global__ void __launch_bounds__(AA_BACK_TILE) queries_resample(QueryArgs a) {
  extern __shared__ __attribute__((aligned(16))) _Float16 tiles[];
  const int64_t unit = blockIdx.x;
  const int item = aa_unit_item(a.unit0, a.n, unit);
  const AABackItem &it = a.items[item];
  const int64_t u = unit - a.unit0[item];
  const int y = (int)(u / it.xtiles);
  const int lane = (int)(threadIdx.x & 63);
  const int x = (int)(u - (int64_t)y * it.xtiles) * AA_BACK_TILE + (int)threadIdx.x;
  if (x - lane >= it.ow) return;  // (a wave wholly beyond ow; no barrier below)
  const int qpad = padded_q(a.Q);
  _Float16 *tile = tiles + (size_t)(threadIdx.x >> 6) * qpad * 64;

  // phase one: element (q, pixel p) of the tile at ((q / 8) * 64 + p) * 8 + q % 8
  _Float16 *mine = tile + lane * 8;
  int written = 0;
  if (x < it.ow) {
    const int xr = (it.flags & AA_MANY_FLIP_X) ? it.ow - 1 - x : x;
    const Row ry = table_row(a.ws + it.tab_h, it.h, it.oh, it.ksize_h, y), rx = table_row(a.ws + it.tab_w, it.w, it.ow, it.ksize_w, xr);
    const int64_t sch = it.stride_ch, prow = it.stride_row, ppx = it.stride_px;
    const TIn *p = (const TIn *)it.src + ry.x0 * prow + rx.x0 * ppx;
    each_class<TIn, VEC>(p, sch, prow, ppx, ry, rx, a.Q, [&](int q, float v) { mine[(q >> 3) * 512 + (q & 7)] = (_Float16)aa_sigmoid(v); });
    written = a.Q;
  }
  for (int q = written; q < qpad; q++) mine[(q >> 3) * 512 + (q & 7)] = (_Float16)0.0f;
  // The lanes meet: what lane p wrote, other lanes of the wave read.  A wave's LDS operations complete in the order it issued them;
  // the fence keeps the compiler from moving the reads before the writes.
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

  // phase two
  const int half = lane >> 5, col = lane & 31;
  const AABackQueryWeights &wt = a.weights[item];
  const int64_t sq = wt.stride_q;
  Epi epi(a.arena + it.out_off, Tile{(int64_t)y * it.ow, (int64_t)it.oh * it.ow, x - lane, it.ow, a.C, lane});
  const half8 *bp = (const half8 *)tile + half * 64 + col;  // step ks: pieces ks * 128 (block 0) and ks * 128 + 32 (block 1)
  for (int c0 = 0; c0 < a.C; c0 += kBlock) {
    // (every load is of an element of the matrix — the class and the query clamped into it — and what lies beyond is replaced after
    // the load: eight independent loads a step, no branch)
    const bool c_ok = c0 + col < a.C;
    const float *wp = wt.w + (int64_t)(c_ok ? c0 + col : a.C - 1) * wt.stride_c;
    float16v d0 = {}, d1 = {};
    for (int ks = 0; ks < qpad / kStep; ks++) {
      const int q0 = ks * kStep + 8 * half;
      float af[8];
#pragma unroll
      for (int t = 0; t < 8; t++) af[t] = wp[(q0 + t < a.Q ? q0 + t : a.Q - 1) * sq];
      half8 av;
#pragma unroll
      for (int t = 0; t < 8; t++) av[t] = (_Float16)((c_ok && q0 + t < a.Q) ? af[t] : 0.0f);
      const half8 b0 = bp[ks * 128], b1 = bp[ks * 128 + 32];
      d0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, b0, d0, 0, 0, 0);
      d1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, b1, d1, 0, 0, 0);
    }
    epi.block(c0, d0, d1);
  }
  epi.done();
}

struct QueryLaunch {
  unsigned units, lds;
  hipStream_t stream;
};
template <typename TIn, bool VEC, typename Epi> void launch_as(const QueryArgs &a, const QueryLaunch &l) {
  hipLaunchKernelGGL((queries_resample<TIn, VEC, Epi>), dim3(l.units), dim3(AA_BACK_TILE), l.lds, l.stream, a);
}
template <typename TIn, bool VEC> void launch_epi(int reduce, int out_dtype, const QueryArgs &a, const QueryLaunch &l) {
  if (reduce == AA_BACK_ARGMAX) {
    if (out_dtype == AA_U8) launch_as<TIn, VEC, Labels<uint8_t>>(a, l);
    else if (out_dtype == AA_I16) launch_as<TIn, VEC, Labels<int16_t>>(a, l);
    else if (out_dtype == AA_I32) launch_as<TIn, VEC, Labels<int32_t>>(a, l);
    else launch_as<TIn, VEC, Labels<int64_t>>(a, l);
  } else with_float_type(out_dtype, [&](auto out) { launch_as<TIn, VEC, Scores<tag_t<decltype(out)>>>(a, l); });
}
void launch_resample(bool vec, int in_dtype, int reduce, int out_dtype, const QueryArgs &a, const QueryLaunch &l) {
  with_float_type(in_dtype, [&](auto in) {
    if (vec) launch_epi<tag_t<decltype(in)>, true>(reduce, out_dtype, a, l);
    else launch_epi<tag_t<decltype(in)>, false>(reduce, out_dtype, a, l);
  });
}

}  // namespace

// ---- host: the planner ---------------------------------------------------------------------------------------------------------------------
size_t aa_back_queries_desc_size(int64_t n) {
  return n < 0 ? 0 : aa_desc_size(sizeof(AABackQueriesHeader), sizeof(AABackItem), n) + (size_t)n * sizeof(AABackQueryWeights);
}

// aa_back_plan_host's checks in its order with K = Q: Q beyond AA_BACK_QUERIES_MAX_Q, C outside 1 .. INT32_MAX / 4 and a reduce that is
// neither values nor argmax beside n and K; a label type that cannot hold C - 1; `weights` beside the pointers; after an item's own
// checks its weights — AA_ERR_NULL, AA_ERR_STRIDES for a negative stride or a pointer that is not a float's — and C * oh * ow against
// AA_BACK_MAX_ELEMS with the arena and the work units; last AA_ERR_BAD_DTYPE.
int aa_back_queries_plan_host(int filter, int layout, int64_t n, int64_t Q, int64_t C, const aa_back_item *in, const aa_back_weights *weights,
                              int reduce, int out_dtype, void *desc_host, size_t desc_bytes, size_t *workspace_bytes, size_t *arena_bytes,
                              int64_t *out_offsets) {
  int rc = plan_prologue(filter, layout, n, Q, reduce, AA_BACK_ACT_SIGMOID, out_dtype, shape_ok(Q, C, reduce));
  if (rc != AA_OK) return rc;
  if (!label_holds(reduce, out_dtype, C)) return AA_ERR_BAD_SHAPE;
  if (!desc_host || !workspace_bytes || !arena_bytes || (n > 0 && (!in || !weights || !out_offsets))) return AA_ERR_NULL;
  if (desc_bytes < aa_back_queries_desc_size(n)) return AA_ERR_WORKSPACE;
  const size_t eb = elem_bytes(out_dtype);
  AABackQueriesHeader *hd = (AABackQueriesHeader *)desc_host;
  AABackItem *items = (AABackItem *)(hd + 1);
  int64_t *unit0 = (int64_t *)(items + n);
  AABackQueryWeights *wts = (AABackQueryWeights *)(unit0 + n + 1);
  size_t ws = 0, arena = 0;
  int64_t units = 0;
  for (int64_t i = 0; i < n; i++) {
    AABackItem it;
    if ((rc = plan_item(filter, layout, Q, in[i], it, ws)) != AA_OK) return rc;
    const aa_back_weights &w = weights[i];
    if (!w.data_dev) return AA_ERR_NULL;
    if ((Q > 1 && w.stride_q < 0) || (C > 1 && w.stride_c < 0) || (uintptr_t)w.data_dev % sizeof(float)) return AA_ERR_STRIDES;
    wts[i] = {(const float *)w.data_dev, Q > 1 ? w.stride_q : 0, C > 1 ? w.stride_c : 0, 0};
    if ((int64_t)it.oh * it.ow > AA_BACK_MAX_ELEMS / C) return AA_ERR_BAD_SHAPE;
    arena = aa_align16(arena);
    it.out_off = (int64_t)arena;
    arena += (size_t)(reduce == AA_BACK_ARGMAX ? 1 : C) * (size_t)it.oh * (size_t)it.ow * eb;
    if (arena > (size_t)AA_BACK_MAX_ELEMS * 8) return AA_ERR_BAD_SHAPE;
    unit0[i] = units;
    units += (int64_t)it.oh * it.xtiles;
    if (units > INT32_MAX) return AA_ERR_BAD_SHAPE;  // (one grid)
    out_offsets[i] = it.out_off;
    items[i] = it;
  }
  unit0[n] = units;
  if (!out_dtype_ok(reduce, out_dtype)) return AA_ERR_BAD_DTYPE;
  memset(hd, 0, sizeof(*hd));
  hd->magic = AA_BACK_QUERIES_MAGIC;
  hd->n = (int32_t)n; hd->Q = (int32_t)Q; hd->C = (int32_t)C; hd->filter = filter; hd->layout = layout;
  hd->reduce = reduce; hd->out_dtype = out_dtype;
  hd->units = units;
  hd->ws_bytes = (int64_t)ws;
  hd->arena_bytes = (int64_t)arena;
  *workspace_bytes = ws;
  *arena_bytes = arena;
  return AA_OK;
}

// ---- host: the two launches ----------------------------------------------------------------------------------------------------------------
// aa_launch_back_many's checks in their order, every one before the first launch; last the LDS of a workgroup against the device's limit.
int aa_launch_back_queries(const void *desc_host, const void *desc_dev, int in_dtype, void *arena_dev, size_t arena_bytes, void *workspace_dev,
                           size_t workspace_bytes, hipStream_t stream) {
  const AABackQueriesHeader *hd = (const AABackQueriesHeader *)desc_host;
  if (hd->magic != AA_BACK_QUERIES_MAGIC || !aa_filter_valid(hd->filter) || hd->n < 0 || hd->Q < 1 || !shape_ok(hd->Q, hd->C, hd->reduce) ||
      !label_holds(hd->reduce, hd->out_dtype, hd->C) || hd->units < 0 || hd->units > INT32_MAX || (hd->layout != AA_NCHW && hd->layout != AA_NHWC))
    return AA_ERR_BAD_SHAPE;
  if (!float_dtype(in_dtype) || !out_dtype_ok(hd->reduce, hd->out_dtype)) return AA_ERR_BAD_DTYPE;
  const int rc = aa_many_check_launch(hd->n, desc_dev, arena_dev, workspace_dev, workspace_bytes, hd->ws_bytes, elem_bytes(hd->out_dtype));
  if (rc != AA_OK || hd->n == 0) return rc;
  if (arena_bytes < (size_t)hd->arena_bytes) return AA_ERR_WORKSPACE;
  bool vec;
  const int rs = check_sources((const AABackItem *)(hd + 1), hd->n, in_dtype, hd->layout, hd->Q, &vec);
  if (rs != AA_OK) return rs;
  unsigned lds;
  const int rl = tiles_lds(hd->Q, stream, &lds);
  if (rl != AA_OK) return rl;
  const AADescView<AABackItem> v = aa_desc_view<AABackQueriesHeader, AABackItem>(desc_dev, hd->n);
  hipLaunchKernelGGL(queries_tables, dim3(2u * (unsigned)hd->n), dim3(AA_BACK_THREADS), 0, stream, v.items, (char *)workspace_dev, (int)hd->filter);
  AA_HIP_CHECK_LAUNCH();
  QueryArgs a;
  a.items = v.items; a.unit0 = v.prefix; a.weights = (const AABackQueryWeights *)(v.prefix + hd->n + 1);
  a.ws = (const char *)workspace_dev; a.arena = (char *)arena_dev;
  a.n = hd->n; a.Q = hd->Q; a.C = hd->C;
  launch_resample(vec, in_dtype, hd->reduce, hd->out_dtype, a, QueryLaunch{(unsigned)hd->units, lds, stream});
  AA_HIP_CHECK_LAUNCH();
  return AA_OK;
}
