// aa_many_back_queries_merged.hip — test-time augmentation for mask-classification heads: the n items of aa_many_back_queries.hip are
// MEMBERS of G groups (aa_many_back.h's merged plan), every member with its own Q mask logits and its own [Q, C] weights, and with
// P_i and Wh_i that file's float16 operands of member i at its group's size,
//   S_g[c, y, x] = sum over the members i of g, sum over q, of Wh_i[q, c] * P_i[q, y, x]
// exact products summed in fp32 by the matrix unit: the sum over (member, query) is ONE inner dimension of M * Qpad, so the members
// cost no add of their own and no score of a member ever exists.  merge 1 divides every S_g once by (float)M, correctly rounded,
// before it is stored or offered to the argmax.  Two launches whatever n, G, M and the sizes:
//   1. merged_tables     workgroups 0 .. 2n - 1 are back_tables' body per (member, axis); the workgroups behind them pack every member's
//                        weights ONCE, behind the tables of the workspace, as float16 in the matrix instruction's operand order
//                        [member][class block of 32][query step of 16][64 lanes][8 halves] — the value the un-grouped kernel's lane
//                        converts on load, the same expression (the class and the query clamped into the matrix, what lies beyond
//                        replaced by +0 after the load), so phase two's A operand is one coalesced 16-byte load a lane and step, 1 KiB
//                        a wave, in place of eight strided fp32 loads and eight conversions that would otherwise repeat per member.
//   2. merged_resample   one workgroup per (group, output row, AA_BACK_TILE columns); a wave owns 64 pixels and its own LDS tile
//                        [Qpad / 8][64][8] float16 as in the un-grouped kernel, and there is no barrier.  A SET of NB class blocks has
//                        its 2 x 16 x NB fp32 accumulators resident across the member loop, which is the OUTER one:
//                          for member j of the group:  phase one (each_class over j's own source, tables and flip, float16(sigmoid)
//                                                      into the tile, the padding rows and the lanes beyond ow rewritten as +0),
//                                                      a wavefront fence, phase two (per query step two B pieces from LDS, then per
//                                                      class block of the set one packed A piece and two matrix instructions), and a
//                                                      wavefront fence between these operand reads and the next member's writes.
//                        So LDS does not grow with M and a group may have any number of members.  NB is 1, 3 or 6: C <= 32, 96 and 192
//                        are resampled once; a larger C runs class PASSES of 6 blocks, each walking the members again.  Per
//                        accumulator the matrix instructions are the un-grouped kernel's — query steps ascending, the same operand
//                        values — so a group of one member gives that kernel's bits.  After the last member: the mean's division,
//                        then per class block ascending the un-grouped epilogues (Scores' stores, or the lane's running Candidate,
//                        merged across lane l and l ^ 32 after the last pass); the output's element type is one runtime switch at the
//                        store, not a template parameter.
// LDS is Qpad * 512 bytes a workgroup, checked against the device's limit.  Every element offset is 64-bit.  Plain C++, vector
// memory operations and the MFMA builtin only.

#include <string.h>

#include "aa_many_back_queries_merged.h"
#include "aa_many_back_queries_dev.h"

namespace {

// ---- 1. tables and packed weights ----------------------------------------------------------------------------------------------------------
struct PackArgs {
  const AABackQueryWeights *weights;
  half8 *packed;
  int n, Q, C;
  int blocks;  // workgroups a member: its pieces (64 a class block and query step) over AA_BACK_THREADS, rounded up
};

__global__ void __launch_bounds__(AA_BACK_THREADS) merged_tables(const AABackItem *items, char *ws, int filter, PackArgs p) {
  if (blockIdx.x < 2u * (unsigned)p.n) {  // (uniform)
    const AABackItem &it = items[blockIdx.x >> 1];
    const bool horiz = blockIdx.x & 1;
    const TableAxis ax = {horiz ? it.w : it.h, horiz ? it.ow : it.oh, horiz ? it.ksize_w : it.ksize_h, 0, horiz ? it.scale_w : it.scale_h,
                          ws + (horiz ? it.tab_w : it.tab_h), nullptr};
    table_axis_build<AA_BACK_THREADS>(ax, filter, 0);
    return;
  }
  const int b = (int)(blockIdx.x - 2u * (unsigned)p.n);
  const int m = b / p.blocks;
  const int steps = padded_q(p.Q) / kStep, pieces = (p.C + kBlock - 1) / kBlock * steps * 64;
  const int piece = (b - m * p.blocks) * AA_BACK_THREADS + (int)threadIdx.x;
  if (piece >= pieces) return;
  const int lane = piece & 63, ks = (piece >> 6) % steps, cb = (piece >> 6) / steps;
  const int c = cb * kBlock + (lane & 31), q0 = ks * kStep + 8 * (lane >> 5);
  // (every load is of an element of the matrix — the class and the query clamped into it — and what lies beyond is replaced after the load)
  const AABackQueryWeights &wt = p.weights[m];
  const bool c_ok = c < p.C;
  const float *wp = wt.w + (int64_t)(c_ok ? c : p.C - 1) * wt.stride_c;
  const int64_t sq = wt.stride_q;
  float af[8];
#pragma unroll
  for (int t = 0; t < 8; t++) af[t] = wp[(q0 + t < p.Q ? q0 + t : p.Q - 1) * sq];
  half8 av;
#pragma unroll
  for (int t = 0; t < 8; t++) av[t] = (_Float16)((c_ok && q0 + t < p.Q) ? af[t] : 0.0f);
  p.packed[(int64_t)m * pieces + piece] = av;
}

// ---- 2. the resample -----------------------------------------------------------------------------------------------------------------------
struct MergedQueryArgs {
  const AABackItem *items;
  const AABackGroup *groups;
  const int32_t *member;
  const int64_t *unit0;
  const half8 *packed;
  const char *ws;
  char *arena;
  int G, Q, C, mean;
  int out_dtype;  // of the store: a float type for the scores, an integer type for the labels
};

__device__ inline void store_scores(int dt, void *out, const Tile &t, int c0, const float16v &d0, const float16v &d1) {
  if (dt == AA_F32) Scores<float>(out, t).block(c0, d0, d1);
  else if (dt == AA_F16) Scores<f16_t>(out, t).block(c0, d0, d1);
  else Scores<bf16_t>(out, t).block(c0, d0, d1);
}
__device__ inline void store_label(int dt, void *out, int64_t at, int idx) {
  if (dt == AA_U8) ((uint8_t *)out)[at] = (uint8_t)idx;
  else if (dt == AA_I16) ((int16_t *)out)[at] = (int16_t)idx;
  else if (dt == AA_I32) ((int32_t *)out)[at] = (int32_t)idx;
  else ((int64_t *)out)[at] = (int64_t)idx;
}

template <typename TIn, bool VEC, int NB, bool LABELS>
__global__ void __launch_bounds__(AA_BACK_TILE) merged_resample(MergedQueryArgs a) {
  extern __shared__ __attribute__((aligned(16))) _Float16 tiles[];
  const int64_t unit = blockIdx.x;
  const int g = aa_unit_item(a.unit0, a.G, unit);
  const AABackGroup &gr = a.groups[g];
  const int64_t u = unit - a.unit0[g];
  const int y = (int)(u / gr.xtiles);
  const int lane = (int)(threadIdx.x & 63);
  const int x = (int)(u - (int64_t)y * gr.xtiles) * AA_BACK_TILE + (int)threadIdx.x;
  if (x - lane >= gr.ow) return;  // (a wave wholly beyond ow; no barrier below)
  const int qpad = padded_q(a.Q), steps = qpad / kStep, cblocks = (a.C + kBlock - 1) / kBlock;
  const int64_t pieces = (int64_t)cblocks * steps * 64;  // of one member's packed weights
  _Float16 *tile = tiles + (size_t)(threadIdx.x >> 6) * qpad * 64;
  _Float16 *mine = tile + lane * 8;  // element (q, pixel p) of the tile at ((q / 8) * 64 + p) * 8 + q % 8
  const int half = lane >> 5, col = lane & 31;
  const half8 *bp = (const half8 *)tile + half * 64 + col;  // step ks: pieces ks * 128 (block 0) and ks * 128 + 32 (block 1)
  const int32_t *member = a.member + gr.first;
  void *out = a.arena + gr.out_off;
  LabelCandidates labels(Tile{(int64_t)y * gr.ow, (int64_t)gr.oh * gr.ow, x - lane, gr.ow, a.C, lane});

  for (int cb0 = 0; cb0 < cblocks; cb0 += NB) {  // a class pass: NB blocks' accumulators resident across the members
    float16v d[NB][2];
#pragma unroll
    for (int nb = 0; nb < NB; nb++) d[nb][0] = d[nb][1] = float16v{};
    for (int m = 0; m < gr.count; m++) {
      const int item = member[m];
      const AABackItem &it = a.items[item];
      // phase one: the un-grouped kernel's, over this member (it.oh and it.ow are the group's)
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
      // the fences keep the compiler from moving the reads before these writes, and the next member's writes before the reads.
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

      // phase two: the member's Qpad queries into every accumulator of the set
      const half8 *ap = a.packed + (int64_t)item * pieces + (int64_t)cb0 * steps * 64 + lane;
      for (int ks = 0; ks < steps; ks++) {
        const half8 b0 = bp[ks * 128], b1 = bp[ks * 128 + 32];
#pragma unroll
        for (int nb = 0; nb < NB; nb++) {
          if (cb0 + nb >= cblocks) continue;  // (uniform; no piece beyond the packed matrix is addressed)
          const half8 av = ap[(int64_t)(nb * steps + ks) * 64];
          d[nb][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, b0, d[nb][0], 0, 0, 0);
          d[nb][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, b1, d[nb][1], 0, 0, 0);
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    if (a.mean) {  // (one correctly rounded division; by 1 it is exact)
      const float count = (float)gr.count;
#pragma unroll
      for (int nb = 0; nb < NB; nb++) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
          d[nb][0][r] = d[nb][0][r] / count;
          d[nb][1][r] = d[nb][1][r] / count;
        }
      }
    }
#pragma unroll
    for (int nb = 0; nb < NB; nb++) {
      if (cb0 + nb >= cblocks) continue;
      if constexpr (LABELS) labels.block((cb0 + nb) * kBlock, d[nb][0], d[nb][1]);
      else store_scores(a.out_dtype, out, labels.t, (cb0 + nb) * kBlock, d[nb][0], d[nb][1]);
    }
  }
  if constexpr (LABELS) {
    const int idx = labels.winner();
    if (x < gr.ow) store_label(a.out_dtype, out, labels.t.row + x, idx);
  }
}

struct MergedQueryLaunch {
  unsigned units, lds;
  hipStream_t stream;
};
template <typename TIn, bool VEC, int NB> void launch_as(int reduce, const MergedQueryArgs &a, const MergedQueryLaunch &l) {
  if (reduce == AA_BACK_ARGMAX) hipLaunchKernelGGL((merged_resample<TIn, VEC, NB, true>), dim3(l.units), dim3(AA_BACK_TILE), l.lds, l.stream, a);
  else hipLaunchKernelGGL((merged_resample<TIn, VEC, NB, false>), dim3(l.units), dim3(AA_BACK_TILE), l.lds, l.stream, a);
}
// The resident set: 1, 3 or 6 class blocks, the smallest that holds C; beyond 192 classes 6 blocks a class pass.
template <typename TIn, bool VEC> void launch_set(int reduce, const MergedQueryArgs &a, const MergedQueryLaunch &l) {
  if (a.C <= kBlock) launch_as<TIn, VEC, 1>(reduce, a, l);
  else if (a.C <= 3 * kBlock) launch_as<TIn, VEC, 3>(reduce, a, l);
  else launch_as<TIn, VEC, 6>(reduce, a, l);
}
void launch_resample(bool vec, int in_dtype, int reduce, const MergedQueryArgs &a, const MergedQueryLaunch &l) {
  with_float_type(in_dtype, [&](auto in) {
    if (vec) launch_set<tag_t<decltype(in)>, true>(reduce, a, l);
    else launch_set<tag_t<decltype(in)>, false>(reduce, a, l);
  });
}

// The workgroups of the table launch that pack one member's weights (AA_BACK_THREADS pieces of 16 bytes each), and whether the whole
// launch — two table workgroups and these per member — is one grid; that also keeps a member's pieces within an int.
inline int64_t pack_blocks(int64_t Q, int64_t C) {
  return ((int64_t)(aa_back_queries_packed_bytes(Q, C) / sizeof(half8)) + AA_BACK_THREADS - 1) / AA_BACK_THREADS;
}
inline bool one_grid(int64_t n, int64_t Q, int64_t C) { return Q >= 1 && pack_blocks(Q, C) <= (1 << 22) && n * (2 + pack_blocks(Q, C)) <= INT32_MAX; }

}  // namespace

// ---- host: the planner ---------------------------------------------------------------------------------------------------------------------
size_t aa_back_queries_merged_desc_size(int64_t n, int64_t g) {
  if (n < 0 || g < 0) return 0;
  return sizeof(AABackQueriesMergedHeader) + merged_sections_size(n, g) + (size_t)n * sizeof(AABackQueryWeights);
}

// aa_back_merged_plan_host's checks in its order with K = Q and what aa_back_queries_plan_host adds in its places: Q, C and the reduce
// beside n, G and merge; a label type that cannot hold C - 1; `weights` beside the pointers; the groups' membership after the block's
// size; per member its own checks, its size against its group's, then its weights (AA_ERR_NULL, AA_ERR_STRIDES); per group C * oh * ow
// against AA_BACK_MAX_ELEMS with the arena and the work units; last AA_ERR_BAD_DTYPE.
int aa_back_queries_merged_plan_host(int filter, int layout, int64_t n, int64_t Q, int64_t C, const aa_back_item *in, const aa_back_weights *weights,
                                     int64_t G, const int64_t *group_of, int merge, int reduce, int out_dtype, void *desc_host, size_t desc_bytes,
                                     size_t *workspace_bytes, size_t *arena_bytes, int64_t *out_offsets) {
  const bool own_ok = G >= 0 && G <= n && (G > 0 || n == 0) && (merge == AA_BACK_MERGE_SUM || merge == AA_BACK_MERGE_MEAN) && shape_ok(Q, C, reduce);
  int rc = plan_prologue(filter, layout, n, Q, reduce, AA_BACK_ACT_SIGMOID, out_dtype, own_ok);
  if (rc != AA_OK) return rc;
  if (!label_holds(reduce, out_dtype, C) || !one_grid(n, Q, C)) return AA_ERR_BAD_SHAPE;
  if (!desc_host || !workspace_bytes || !arena_bytes || (n > 0 && (!in || !weights || !group_of || !out_offsets))) return AA_ERR_NULL;
  if (desc_bytes < aa_back_queries_merged_desc_size(n, G)) return AA_ERR_WORKSPACE;
  const size_t eb = elem_bytes(out_dtype);
  AABackQueriesMergedHeader *hd = (AABackQueriesMergedHeader *)desc_host;
  AABackItem *items = (AABackItem *)(hd + 1);
  AABackGroup *groups = (AABackGroup *)(items + n);
  int32_t *member = (int32_t *)(groups + G);
  int64_t *unit0 = (int64_t *)((char *)member + align8((size_t)n * sizeof(int32_t)));
  AABackQueryWeights *wts = (AABackQueryWeights *)(unit0 + G + 1);
  if ((rc = plan_group_slots(n, G, group_of, AA_BACK_ACT_SIGMOID, groups)) != AA_OK) return rc;
  size_t ws = 0, arena = 0;
  int64_t units = 0;
  for (int64_t i = 0; i < n; i++) {
    if ((rc = plan_members(filter, layout, 1, Q, in + i, group_of + i, items + i, groups, member, ws)) != AA_OK) return rc;
    AABackGroup &gr = groups[group_of[i]];
    member[gr.first + gr.count - 1] = (int32_t)i;  // (plan_members saw one item and numbered it 0)
    const aa_back_weights &w = weights[i];
    if (!w.data_dev) return AA_ERR_NULL;
    if ((Q > 1 && w.stride_q < 0) || (C > 1 && w.stride_c < 0) || (uintptr_t)w.data_dev % sizeof(float)) return AA_ERR_STRIDES;
    wts[i] = {(const float *)w.data_dev, Q > 1 ? w.stride_q : 0, C > 1 ? w.stride_c : 0, 0};
  }
  for (int64_t g = 0; g < G; g++) {
    AABackGroup &gr = groups[g];
    if ((int64_t)gr.oh * gr.ow > AA_BACK_MAX_ELEMS / C) return AA_ERR_BAD_SHAPE;
    arena = aa_align16(arena);
    gr.out_off = (int64_t)arena;
    arena += (size_t)(reduce == AA_BACK_ARGMAX ? 1 : C) * (size_t)gr.oh * (size_t)gr.ow * eb;
    if (arena > (size_t)AA_BACK_MAX_ELEMS * 8) return AA_ERR_BAD_SHAPE;
    unit0[g] = units;
    units += (int64_t)gr.oh * gr.xtiles;
    if (units > INT32_MAX) return AA_ERR_BAD_SHAPE;  // (one grid)
    out_offsets[g] = gr.out_off;
  }
  unit0[G] = units;
  for (int64_t i = 0; i < n; i++) items[i].out_off = groups[group_of[i]].out_off;
  if (n % 2) member[n] = 0;  // (the padding)
  if (!out_dtype_ok(reduce, out_dtype)) return AA_ERR_BAD_DTYPE;
  ws = aa_align16(ws) + (size_t)n * aa_back_queries_packed_bytes(Q, C);  // the tables, then every member's packed weights
  memset(hd, 0, sizeof(*hd));
  hd->magic = AA_BACK_QUERIES_MERGED_MAGIC;
  hd->n = (int32_t)n; hd->Q = (int32_t)Q; hd->C = (int32_t)C; hd->filter = filter; hd->layout = layout;
  hd->reduce = reduce; hd->out_dtype = out_dtype;
  hd->units = units;
  hd->ws_bytes = (int64_t)ws;
  hd->arena_bytes = (int64_t)arena;
  hd->G = (int32_t)G; hd->merge = merge;
  *workspace_bytes = ws;
  *arena_bytes = arena;
  return AA_OK;
}

// ---- host: the two launches ----------------------------------------------------------------------------------------------------------------
// aa_launch_back_merged's and aa_launch_back_queries' checks in their order, every one before the first launch; last the LDS of a
// workgroup against the device's limit.
int aa_launch_back_queries_merged(const void *desc_host, const void *desc_dev, int in_dtype, void *arena_dev, size_t arena_bytes, void *workspace_dev,
                                  size_t workspace_bytes, hipStream_t stream) {
  const AABackQueriesMergedHeader *hd = (const AABackQueriesMergedHeader *)desc_host;
  if (hd->magic != AA_BACK_QUERIES_MERGED_MAGIC || !aa_filter_valid(hd->filter) || hd->n < 0 || hd->Q < 1 || !shape_ok(hd->Q, hd->C, hd->reduce) ||
      !label_holds(hd->reduce, hd->out_dtype, hd->C) || hd->units < 0 || hd->units > INT32_MAX || (hd->layout != AA_NCHW && hd->layout != AA_NHWC) ||
      hd->G < 0 || hd->G > hd->n || (hd->G == 0 && hd->n > 0) || (hd->merge != AA_BACK_MERGE_SUM && hd->merge != AA_BACK_MERGE_MEAN) ||
      !one_grid(hd->n, hd->Q, hd->C))
    return AA_ERR_BAD_SHAPE;
  const int64_t packed_bytes = (int64_t)hd->n * (int64_t)aa_back_queries_packed_bytes(hd->Q, hd->C);
  if (hd->ws_bytes < packed_bytes || (hd->ws_bytes - packed_bytes) % 16) return AA_ERR_BAD_SHAPE;
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
  MergedQueryArgs a;
  a.items = (const AABackItem *)((const char *)desc_dev + sizeof(AABackQueriesMergedHeader));
  a.groups = (const AABackGroup *)(a.items + hd->n);
  a.member = (const int32_t *)(a.groups + hd->G);
  a.unit0 = (const int64_t *)((const char *)a.member + align8((size_t)hd->n * sizeof(int32_t)));
  a.packed = (const half8 *)((const char *)workspace_dev + (hd->ws_bytes - packed_bytes));
  a.ws = (const char *)workspace_dev; a.arena = (char *)arena_dev;
  a.G = hd->G; a.Q = hd->Q; a.C = hd->C; a.mean = hd->merge == AA_BACK_MERGE_MEAN;
  a.out_dtype = hd->out_dtype;
  PackArgs p;
  p.weights = (const AABackQueryWeights *)(a.unit0 + hd->G + 1);
  p.packed = (half8 *)((char *)workspace_dev + (hd->ws_bytes - packed_bytes));
  p.n = hd->n; p.Q = hd->Q; p.C = hd->C;
  p.blocks = (int)pack_blocks(hd->Q, hd->C);
  hipLaunchKernelGGL(merged_tables, dim3((unsigned)hd->n * (2u + (unsigned)p.blocks)), dim3(AA_BACK_THREADS), 0, stream, a.items, (char *)workspace_dev, (int)hd->filter, p);
  AA_HIP_CHECK_LAUNCH();
  launch_resample(vec, in_dtype, hd->reduce, a, MergedQueryLaunch{(unsigned)hd->units, lds, stream});
  AA_HIP_CHECK_LAUNCH();
  return AA_OK;
}
