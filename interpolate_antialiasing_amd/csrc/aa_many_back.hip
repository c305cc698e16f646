// aa_many_back.hip — canvas predictions back to each image's own size: N float sources [K, h_i, w_i] resampled to N outputs of N sizes,
// and reduced over the K classes before anything is stored.  The arithmetic is the reference's fp32 passes as aa_embed_many.hip states
// them (aa_generic.hip's contract): AA_TABLE_F32 tables, the horizontal pass first, an fp32 intermediate, tap 0 unconditionally and taps
// 1 .. xsize - 1 in order, product and sum rounded apart (-ffp-contract=off), one round-to-nearest-even at the store.  Two launches
// whatever N and whatever the sizes:
//   1. back_tables    one workgroup per (item, axis): the rows of the item's table (table_build_f32_one, aa_table_rows.h — the device
//                     function aa_tables.hip runs, so item i's tables are the bits aa_table_build gives its shape);
//   2. back_resample  one workgroup per work unit, an output row of an item times AA_BACK_TILE consecutive output columns, a lane per
//                     column: the row's vertical window is the workgroup's, the lane's horizontal window its own, both read once; then
//                     the classes, AA_BACK_UNROLL at a time, each the vertical sum of horizontal sums.  No intermediate is staged: a lane
//                     recomputes the horizontal sum of each tap row, the same operations in the same order as the two-pass form, so the
//                     same bits.  What happens to a class's value is the epilogue, a template parameter: stored to its plane (Values),
//                     compared with the running best (Argmax: the K values of a pixel never leave registers), or compared with the
//                     threshold (Greater).  A flipped item's column x is stored at ow - 1 - x.
// Sources are read where they lie: planes (classes stride_ch apart, pixels consecutive) or interleaved pixels (classes consecutive, pixels
// K apart), the same code with the strides as arguments; interleaved sources whose K and addresses allow it load AA_BACK_UNROLL classes
// as one vector.  Every element offset is 64-bit.  Stores are one element a lane, consecutive along the wave, so an arena on any
// element boundary is served and the 16-byte gaps between items are never written.
// The merged call (aa_back_merged_plan) runs the same two launches with back_resample_merged in place of back_resample: the items are
// members of groups, a work unit is an output row of a GROUP, and a class's value is the members' values added in order before the
// epilogue sees it (at "2'." below).
// An activation (the plan's AA_BACK_ACT_*, aa_activation.h) stands between a value and what follows it, inside the same two launches and
// without a workspace: the kernels with ACT, one instantiation for both activations (which one is uniform over the launch), so that the
// instantiations double rather than triple and the kernels without an activation stay the code they were.  A sigmoid is applied to a
// class's value where it leaves class_sums.  A softmax makes the lane walk the classes twice: once for the pixel's maximum and
// denominator, once more — the resample recomputed, not staged, this kernel's bargain — for the probabilities, which then go where the
// values went.  In the merged kernel a lane needs that pair of every member before the class-outer loop can add probabilities: a first
// phase walks the members and keeps the pairs in LDS, [member][lane], 8 bytes a lane, so consecutive lanes touch consecutive slots
// and a lane reads only what it wrote (no barrier; the early return stays).  That is 2 KiB a member, AA_BACK_ACT_MEMBERS of them at most.
// Shared with the other ragged calls: aa_many_dev.h (the item of a unit, the element types), aa_many_host.h (the block, the launch checks);
// with the other float ragged calls: aa_float_many_dev.h (the table kernels' body, table_row, class_sums), aa_float_many_host.h (the
// float types, the tables of an item in a plan).

#include <string.h>

#include "aa_many_back.h"
#include "aa_activation.h"
#include "aa_float_many_dev.h"
#include "aa_float_many_host.h"

namespace {

// ---- 1. tables ---------------------------------------------------------------------------------------------------------------------------
// Workgroup 2 i builds item i's H axis, 2 i + 1 its W axis: the shared body without adjoints (the record has none).
__global__ void __launch_bounds__(AA_BACK_THREADS) back_tables(const AABackItem *items, char *ws, int filter) {
  const AABackItem &it = items[blockIdx.x >> 1];
  const bool horiz = blockIdx.x & 1;
  const TableAxis ax = {horiz ? it.w : it.h, horiz ? it.ow : it.oh, horiz ? it.ksize_w : it.ksize_h, 0, horiz ? it.scale_w : it.scale_h,
                        ws + (horiz ? it.tab_w : it.tab_h), nullptr};
  table_axis_build<AA_BACK_THREADS>(ax, filter, 0);
}

// ---- the epilogues -------------------------------------------------------------------------------------------------------------------------
// put(k, v): class k's fp32 value of the lane's pixel, k ascending; done(): after the last class.  `at` is the lane's element of plane 0
// of the item's output (the flip already in it), `plane` the elements of a plane.
template <typename TOut> struct Values {
  TOut *at;
  int64_t plane;
  __device__ Values(void *out, int64_t at_, int64_t plane_, float) : at((TOut *)out + at_), plane(plane_) {}
  __device__ void put(int k, float v) { at[k * plane] = to_elem<TOut>(v); }
  __device__ void done() {}
};
// The lowest k of the greatest value, a NaN greater than every number and the first NaN kept: numpy.argmax.
template <typename TLabel> struct Argmax {
  TLabel *at;
  float best;
  int idx;
  __device__ Argmax(void *out, int64_t at_, int64_t, float) : at((TLabel *)out + at_), best(0.0f), idx(0) {}
  __device__ void put(int k, float v) {
    if (k == 0 || (best == best && (v > best || v != v))) {
      best = v;
      idx = k;
    }
  }
  __device__ void done() { *at = (TLabel)idx; }
};
struct Greater {  // (a NaN is not greater: 0)
  uint8_t *at;
  int64_t plane;
  float thr;
  __device__ Greater(void *out, int64_t at_, int64_t plane_, float thr_) : at((uint8_t *)out + at_), plane(plane_), thr(thr_) {}
  __device__ void put(int k, float v) { at[k * plane] = v > thr ? 1 : 0; }
  __device__ void done() {}
};

struct BackArgs {
  const AABackItem *items;
  const int64_t *unit0;
  const char *ws;
  char *arena;
  float threshold;
  int n, K;
  int act;  // AA_BACK_ACT_*: looked at by the kernels with ACT only
};

// The classes of one pixel in ascending k, AA_BACK_UNROLL at a time and then the tail one by one: put(k, class k's fp32 value).
template <typename TIn, bool VEC, typename Put>
__device__ inline void each_class(const TIn *p, int64_t sch, int64_t prow, int64_t ppx, const Row &ry, const Row &rx, int K, Put put) {
  constexpr int U = AA_BACK_UNROLL;
  int k = 0;
  for (; k + U <= K; k += U) {
    float acc[U];
    class_sums<TIn, U, VEC>(p + k * sch, sch, prow, ppx, ry, rx, acc);
#pragma unroll
    for (int c = 0; c < U; c++) put(k + c, acc[c]);
  }
  for (; k < K; k++) {
    float acc[1];
    class_sums<TIn, 1, false>(p + k * sch, sch, prow, ppx, ry, rx, acc);
    put(k, acc[0]);
  }
}

// ---- 2. the resample -----------------------------------------------------------------------------------------------------------------------
// With ACT the value an epilogue sees is the activation's: the sigmoid of the class's value, or — after a first walk over the classes
// for the pixel's maximum and denominator — its softmax term.  Both K loops of each walk are each_class's.
template <typename TIn, bool VEC, bool ACT, typename Epi>
__global__ void __launch_bounds__(AA_BACK_TILE) back_resample(BackArgs a) {
  const int64_t unit = blockIdx.x;
  const int item = aa_unit_item(a.unit0, a.n, unit);
  const AABackItem &it = a.items[item];
  const int64_t u = unit - a.unit0[item];
  const int y = (int)(u / it.xtiles);
  const int x = (int)(u - (int64_t)y * it.xtiles) * AA_BACK_TILE + (int)threadIdx.x;
  if (x >= it.ow) return;  // (no barrier below)
  const Row ry = table_row(a.ws + it.tab_h, it.h, it.oh, it.ksize_h, y), rx = table_row(a.ws + it.tab_w, it.w, it.ow, it.ksize_w, x);
  const int64_t sch = it.stride_ch, prow = it.stride_row, ppx = it.stride_px;
  const TIn *p = (const TIn *)it.src + ry.x0 * prow + rx.x0 * ppx;
  const int xs = (it.flags & AA_MANY_FLIP_X) ? it.ow - 1 - x : x;
  Epi epi(a.arena + it.out_off, (int64_t)y * it.ow + xs, (int64_t)it.oh * it.ow, a.threshold);
  if constexpr (!ACT) {
    each_class<TIn, VEC>(p, sch, prow, ppx, ry, rx, a.K, [&](int k, float v) { epi.put(k, v); });
  } else if (a.act == AA_BACK_ACT_SOFTMAX) {
    SoftmaxPass one;
    each_class<TIn, VEC>(p, sch, prow, ppx, ry, rx, a.K, [&](int k, float v) { one.put(k, v); });
    const float m = one.m, rcp = one.rcp();
    each_class<TIn, VEC>(p, sch, prow, ppx, ry, rx, a.K, [&](int k, float v) { epi.put(k, aa_softmax_term(v, m, rcp)); });
  } else {
    each_class<TIn, VEC>(p, sch, prow, ppx, ry, rx, a.K, [&](int k, float v) { epi.put(k, aa_sigmoid(v)); });
  }
  epi.done();
}

// ---- 2'. the merged resample ---------------------------------------------------------------------------------------------------------------
// A work unit is an output row of a GROUP times AA_BACK_TILE columns.  The class chunk is the outer loop and the group's members the
// inner one, so the epilogue sees a class's complete sum: the first member's value, then one fp32 add per further member, in ascending
// item order (member[] is in that order), then for the mean one correctly rounded division by the count.  A flipped member is mirrored
// where it is READ: lane x walks that member's horizontal window of column ow - 1 - x, and the store is never mirrored.  A member's two
// table rows are looked up again per class chunk (a few cached words; the member index is uniform over the workgroup) rather than
// kept per member, so there is no limit on the members of a group and nothing is indexed dynamically in registers.
struct MergedArgs {
  const AABackItem *items;
  const AABackGroup *groups;
  const int32_t *member;
  const int64_t *unit0;
  const char *ws;
  char *arena;
  float threshold;
  int G, K, mean;
  int act;  // AA_BACK_ACT_*: looked at by the kernels with ACT only
};

// A softmax member's pair for the lane's pixel, in LDS: the maximum and 1 / denominator of its pass one.  Member m's slot of lane t is
// element m * AA_BACK_TILE + t: the lanes of a wave write and read consecutive 8-byte slots.
struct alignas(8) SoftmaxPair { float m, rcp; };

// sum = the merged value of V classes from class k on of the lane's pixel (y, x) of group gr.  With ACT a member's value is first its
// sigmoid, or its softmax term with the pair the lane left at pairs[m * AA_BACK_TILE].
// (A float16 store may follow `sum[c] + acc[c]`, the mean's division or the sigmoid's directly.  Each must reach it as a rounded fp32
// value: today's compiler folds only a PRODUCT into the conversion (aa_softmax_term keeps that apart).  Nothing in the source keeps a
// later compiler from folding an add or a division the same way; the GPU bit tests with float16 outputs are what would show it.)
template <typename TIn, int V, bool VEC, bool ACT>
__device__ inline void member_sums(const MergedArgs &a, const AABackGroup &gr, int y, int x, int k, const SoftmaxPair *pairs, float (&sum)[V]) {
  const int32_t *member = a.member + gr.first;
  for (int m = 0; m < gr.count; m++) {
    const AABackItem &it = a.items[member[m]];
    const int xr = (it.flags & AA_MANY_FLIP_X) ? gr.ow - 1 - x : x;
    const Row ry = table_row(a.ws + it.tab_h, it.h, gr.oh, it.ksize_h, y), rx = table_row(a.ws + it.tab_w, it.w, gr.ow, it.ksize_w, xr);
    const int64_t sch = it.stride_ch, prow = it.stride_row, ppx = it.stride_px;
    float acc[V];
    class_sums<TIn, V, VEC>((const TIn *)it.src + ry.x0 * prow + rx.x0 * ppx + k * sch, sch, prow, ppx, ry, rx, acc);
    if constexpr (ACT) {
      if (a.act == AA_BACK_ACT_SOFTMAX) {
        const SoftmaxPair s = pairs[m * AA_BACK_TILE];
#pragma unroll
        for (int c = 0; c < V; c++) acc[c] = aa_softmax_term(acc[c], s.m, s.rcp);
      } else {
#pragma unroll
        for (int c = 0; c < V; c++) acc[c] = aa_sigmoid(acc[c]);
      }
    }
#pragma unroll
    for (int c = 0; c < V; c++) sum[c] = m == 0 ? acc[c] : sum[c] + acc[c];
  }
  if (a.mean) {
    const float count = (float)gr.count;
#pragma unroll
    for (int c = 0; c < V; c++) sum[c] = sum[c] / count;
  }
}

// With ACT and a softmax, phase one: per member of the group, in order, the lane walks the member's classes once (each_class over the
// member's own windows, mirrored where it is read like phase two) and leaves the pair in its LDS slot.  The launch sizes the dynamic LDS
// for the plan's largest group (AA_BACK_TILE pairs a member; nothing for a sigmoid), and the planner bounds that group.
template <typename TIn, bool VEC, bool ACT, typename Epi>
__global__ void __launch_bounds__(AA_BACK_TILE) back_resample_merged(MergedArgs a) {
  constexpr int U = AA_BACK_UNROLL;
  const int64_t unit = blockIdx.x;
  const int g = aa_unit_item(a.unit0, a.G, unit);
  const AABackGroup &gr = a.groups[g];
  const int64_t u = unit - a.unit0[g];
  const int y = (int)(u / gr.xtiles);
  const int x = (int)(u - (int64_t)y * gr.xtiles) * AA_BACK_TILE + (int)threadIdx.x;
  if (x >= gr.ow) return;  // (no barrier below)
  const SoftmaxPair *pairs = nullptr;
  if constexpr (ACT) {
    extern __shared__ __attribute__((aligned(8))) SoftmaxPair act_pairs[];
    pairs = act_pairs + threadIdx.x;
    if (a.act == AA_BACK_ACT_SOFTMAX) {
      const int32_t *member = a.member + gr.first;
      for (int m = 0; m < gr.count; m++) {
        const AABackItem &it = a.items[member[m]];
        const int xr = (it.flags & AA_MANY_FLIP_X) ? gr.ow - 1 - x : x;
        const Row ry = table_row(a.ws + it.tab_h, it.h, gr.oh, it.ksize_h, y), rx = table_row(a.ws + it.tab_w, it.w, gr.ow, it.ksize_w, xr);
        const int64_t sch = it.stride_ch, prow = it.stride_row, ppx = it.stride_px;
        SoftmaxPass one;
        each_class<TIn, VEC>((const TIn *)it.src + ry.x0 * prow + rx.x0 * ppx, sch, prow, ppx, ry, rx, a.K, [&](int k, float v) { one.put(k, v); });
        act_pairs[m * AA_BACK_TILE + threadIdx.x] = {one.m, one.rcp()};
      }
    }
  }
  Epi epi(a.arena + gr.out_off, (int64_t)y * gr.ow + x, (int64_t)gr.oh * gr.ow, a.threshold);
  int k = 0;
  for (; k + U <= a.K; k += U) {
    float sum[U];
    member_sums<TIn, U, VEC, ACT>(a, gr, y, x, k, pairs, sum);
#pragma unroll
    for (int c = 0; c < U; c++) epi.put(k + c, sum[c]);
  }
  for (; k < a.K; k++) {
    float sum[1];
    member_sums<TIn, 1, false, ACT>(a, gr, y, x, k, pairs, sum);
    epi.put(k, sum[0]);
  }
  epi.done();
}

// The kernel of an argument block: back_resample for the items of aa_back_many_plan, back_resample_merged for the groups of
// aa_back_merged_plan; the same epilogues and element types for both.
// What is launched: the work units, the bytes of dynamic LDS (the merged softmax's pairs; 0 otherwise), the stream.
struct BackLaunch {
  unsigned units, lds;
  hipStream_t stream;
};
template <typename TIn, bool VEC, bool ACT, typename Epi> void launch_as(const BackArgs &a, const BackLaunch &l) {
  hipLaunchKernelGGL((back_resample<TIn, VEC, ACT, Epi>), dim3(l.units), dim3(AA_BACK_TILE), 0, l.stream, a);
}
template <typename TIn, bool VEC, bool ACT, typename Epi> void launch_as(const MergedArgs &a, const BackLaunch &l) {
  hipLaunchKernelGGL((back_resample_merged<TIn, VEC, ACT, Epi>), dim3(l.units), dim3(AA_BACK_TILE), ACT ? l.lds : 0, l.stream, a);
}
template <typename TIn, bool VEC, bool ACT, typename Args> void launch_epi(int reduce, int out_dtype, const Args &a, const BackLaunch &l) {
  if (reduce == AA_BACK_GREATER) launch_as<TIn, VEC, ACT, Greater>(a, l);
  else if (reduce == AA_BACK_ARGMAX) {
    if (out_dtype == AA_U8) launch_as<TIn, VEC, ACT, Argmax<uint8_t>>(a, l);
    else if (out_dtype == AA_I16) launch_as<TIn, VEC, ACT, Argmax<int16_t>>(a, l);
    else if (out_dtype == AA_I32) launch_as<TIn, VEC, ACT, Argmax<int32_t>>(a, l);
    else launch_as<TIn, VEC, ACT, Argmax<int64_t>>(a, l);
  } else with_float_type(out_dtype, [&](auto out) { launch_as<TIn, VEC, ACT, Values<tag_t<decltype(out)>>>(a, l); });
}
template <bool VEC, bool ACT, typename Args> void launch_in(int in_dtype, int reduce, int out_dtype, const Args &a, const BackLaunch &l) {
  with_float_type(in_dtype, [&](auto in) { launch_epi<tag_t<decltype(in)>, VEC, ACT>(reduce, out_dtype, a, l); });
}
// The kernel of (vector loads or not, an activation or not): a.act says which.
template <typename Args> void launch_resample(bool vec, int in_dtype, int reduce, int out_dtype, const Args &a, const BackLaunch &l) {
  if (a.act != AA_BACK_ACT_NONE) {
    if (vec) launch_in<true, true>(in_dtype, reduce, out_dtype, a, l);
    else launch_in<false, true>(in_dtype, reduce, out_dtype, a, l);
  } else if (vec) launch_in<true, false>(in_dtype, reduce, out_dtype, a, l);
  else launch_in<false, false>(in_dtype, reduce, out_dtype, a, l);
}

inline bool act_ok(int activation) { return activation >= AA_BACK_ACT_NONE && activation <= AA_BACK_ACT_SIGMOID; }

// What a reduction stores: values a float, argmax a label, greater a byte of 0 or 1.
inline bool out_dtype_ok(int reduce, int dt) {
  if (reduce == AA_BACK_VALUES) return float_dtype(dt);
  if (reduce == AA_BACK_ARGMAX) return dt == AA_U8 || dt == AA_I16 || dt == AA_I32 || dt == AA_I64;
  return dt == AA_BOOL || dt == AA_U8;
}

// What both planners check first, in this order: the filter; the layout; n, K, reduce and the activation (own_ok: what the caller adds to
// them); a label type that cannot hold K - 1.
inline int plan_prologue(int filter, int layout, int64_t n, int64_t K, int reduce, int activation, int out_dtype, bool own_ok) {
  if (!aa_filter_valid(filter)) return AA_ERR_BAD_FILTER;
  if (layout != AA_NCHW && layout != AA_NHWC) return AA_ERR_BAD_LAYOUT;
  if (n < 0 || n > kAAManyMax || K < 1 || K > kAAManyMax || reduce < AA_BACK_VALUES || reduce > AA_BACK_GREATER || !act_ok(activation) ||
      !own_ok)
    return AA_ERR_BAD_SHAPE;
  if (reduce == AA_BACK_ARGMAX && ((out_dtype == AA_U8 && K > 256) || (out_dtype == AA_I16 && K > 32768))) return AA_ERR_BAD_SHAPE;
  return AA_OK;
}

// One aa_back_item checked and written as its record, its two tables appended to the table arena at ws: everything of an item but its
// place in the arena and among the work units, which are the planner's (an item's own, or its group's).
inline int plan_item(int filter, int layout, int64_t K, const aa_back_item &im, AABackItem &it, size_t &ws) {
  if (!im.data_dev) return AA_ERR_NULL;
  if (im.h <= 0 || im.w <= 0 || im.h > kAAManyMax || im.w > kAAManyMax || im.oh <= 0 || im.ow <= 0 || im.oh > kAAManyMax || im.ow > kAAManyMax ||
      (im.flags & ~AA_MANY_FLIP_X))
    return AA_ERR_BAD_SHAPE;
  if (im.oh * im.ow > AA_BACK_MAX_ELEMS / K) return AA_ERR_BAD_SHAPE;
  // (the stride of an axis of one element never matters)
  if ((K > 1 && im.stride_ch < 0) || (im.h > 1 && im.stride_row < 0) || (im.w > 1 && im.stride_px < 0)) return AA_ERR_STRIDES;
  if (layout == AA_NHWC ? ((K > 1 && im.stride_ch != 1) || (im.w > 1 && im.stride_px != K)) : (im.w > 1 && im.stride_px != 1)) return AA_ERR_STRIDES;
  memset(&it, 0, sizeof(it));
  it.src = im.data_dev;
  it.stride_ch = K > 1 ? im.stride_ch : 0;
  it.stride_row = im.h > 1 ? im.stride_row : 0;
  it.stride_px = im.w > 1 ? im.stride_px : 0;
  it.h = (int32_t)im.h; it.w = (int32_t)im.w; it.oh = (int32_t)im.oh; it.ow = (int32_t)im.ow;
  const int rc = plan_forward_tables(filter, im.h, im.w, im.oh, im.ow, it, ws);
  if (rc != AA_OK) return rc;
  it.flags = im.flags;
  it.xtiles = (int32_t)((im.ow + AA_BACK_TILE - 1) / AA_BACK_TILE);
  return AA_OK;
}

// An output [K or 1, oh, ow] appended to the arena on a 16-byte boundary, its rows of tiles to the work units; -> its offset in *off.
inline int plan_output(int64_t K, int reduce, size_t eb, int64_t oh, int64_t ow, int64_t xtiles, size_t &arena, int64_t &units, int64_t *off) {
  arena = aa_align16(arena);
  *off = (int64_t)arena;
  arena += (size_t)(reduce == AA_BACK_ARGMAX ? 1 : K) * (size_t)oh * (size_t)ow * eb;
  if (arena > (size_t)AA_BACK_MAX_ELEMS * 8) return AA_ERR_BAD_SHAPE;
  units += oh * xtiles;
  if (units > INT32_MAX) return AA_ERR_BAD_SHAPE;  // (one grid)
  return AA_OK;
}

// What both launches check of the planned items' pointers, which the planner could not: against the element of in_dtype, and for
// whether every address of an interleaved list allows the vector loads (*vec).
inline int check_sources(const AABackItem *host_items, int64_t n, int in_dtype, int layout, int K, bool *vec) {
  const size_t ei = elem_bytes(in_dtype);
  *vec = layout == AA_NHWC && K % AA_BACK_UNROLL == 0;
  for (int64_t i = 0; i < n; i++) {
    const AABackItem &it = host_items[i];
    if ((uintptr_t)it.src % ei) return AA_ERR_STRIDES;
    *vec = *vec && (uintptr_t)it.src % (AA_BACK_UNROLL * ei) == 0 && it.stride_row % AA_BACK_UNROLL == 0;  // (stride_px is K or unused)
  }
  return AA_OK;
}

inline size_t align8(size_t v) { return (v + 7) & ~(size_t)7; }

}  // namespace

// ---- host: the planner -------------------------------------------------------------------------------------------------------------------
size_t aa_back_desc_size(int64_t n) { return aa_desc_size(sizeof(AABackHeader), sizeof(AABackItem), n); }

int aa_back_plan_host(int filter, int layout, int64_t n, int64_t K, const aa_back_item *in, int reduce, int activation, int out_dtype,
                      void *desc_host, size_t desc_bytes, size_t *workspace_bytes, size_t *arena_bytes, int64_t *out_offsets) {
  int rc = plan_prologue(filter, layout, n, K, reduce, activation, out_dtype, true);
  if (rc != AA_OK) return rc;
  if (!desc_host || !workspace_bytes || !arena_bytes || (n > 0 && (!in || !out_offsets))) return AA_ERR_NULL;
  if (desc_bytes < aa_back_desc_size(n)) return AA_ERR_WORKSPACE;
  const size_t eb = elem_bytes(out_dtype);
  AABackHeader *hd = (AABackHeader *)desc_host;
  AABackItem *items = (AABackItem *)(hd + 1);
  int64_t *unit0 = (int64_t *)(items + n);
  size_t ws = 0, arena = 0;
  int64_t units = 0;
  for (int64_t i = 0; i < n; i++) {
    AABackItem it;
    if ((rc = plan_item(filter, layout, K, in[i], it, ws)) != AA_OK) return rc;
    unit0[i] = units;
    if ((rc = plan_output(K, reduce, eb, it.oh, it.ow, it.xtiles, arena, units, &it.out_off)) != AA_OK) return rc;
    out_offsets[i] = it.out_off;
    items[i] = it;
  }
  unit0[n] = units;
  if (!out_dtype_ok(reduce, out_dtype)) return AA_ERR_BAD_DTYPE;
  memset(hd, 0, sizeof(*hd));
  hd->magic = AA_BACK_MAGIC;
  hd->n = (int32_t)n; hd->K = (int32_t)K; hd->filter = filter; hd->layout = layout;
  hd->reduce = reduce; hd->out_dtype = out_dtype;
  hd->reserved0 = activation;
  hd->units = units;
  hd->ws_bytes = (int64_t)ws;
  hd->arena_bytes = (int64_t)arena;
  *workspace_bytes = ws;
  *arena_bytes = arena;
  return AA_OK;
}

// ---- host: the two launches ----------------------------------------------------------------------------------------------------------------
// Every check comes before the first launch.  desc_host is the planned block, so the items' pointers are looked at here: against the
// element of in_dtype, which the planner did not know, and for whether every address of an interleaved list allows the vector loads.
int aa_launch_back_many(const void *desc_host, const void *desc_dev, int in_dtype, float threshold, void *arena_dev, size_t arena_bytes,
                        void *workspace_dev, size_t workspace_bytes, hipStream_t stream) {
  const AABackHeader *hd = (const AABackHeader *)desc_host;
  if (hd->magic != AA_BACK_MAGIC || !aa_filter_valid(hd->filter) || hd->n < 0 || hd->K < 1 || hd->units < 0 || hd->units > INT32_MAX ||
      hd->reduce < AA_BACK_VALUES || hd->reduce > AA_BACK_GREATER || (hd->layout != AA_NCHW && hd->layout != AA_NHWC) || !act_ok(hd->reserved0))
    return AA_ERR_BAD_SHAPE;
  if (!float_dtype(in_dtype) || !out_dtype_ok(hd->reduce, hd->out_dtype)) return AA_ERR_BAD_DTYPE;
  if (hd->reduce == AA_BACK_GREATER && !(threshold - threshold == 0.0f)) return AA_ERR_BAD_SHAPE;  // (not finite)
  const int rc = aa_many_check_launch(hd->n, desc_dev, arena_dev, workspace_dev, workspace_bytes, hd->ws_bytes, elem_bytes(hd->out_dtype));
  if (rc != AA_OK || hd->n == 0) return rc;
  if (arena_bytes < (size_t)hd->arena_bytes) return AA_ERR_WORKSPACE;
  bool vec;
  const int rs = check_sources((const AABackItem *)(hd + 1), hd->n, in_dtype, hd->layout, hd->K, &vec);
  if (rs != AA_OK) return rs;
  const AADescView<AABackItem> v = aa_desc_view<AABackHeader, AABackItem>(desc_dev, hd->n);
  hipLaunchKernelGGL(back_tables, dim3(2u * (unsigned)hd->n), dim3(AA_BACK_THREADS), 0, stream, v.items, (char *)workspace_dev, (int)hd->filter);
  AA_HIP_CHECK_LAUNCH();
  BackArgs a;
  a.items = v.items; a.unit0 = v.prefix; a.ws = (const char *)workspace_dev; a.arena = (char *)arena_dev;
  a.threshold = threshold;
  a.n = hd->n; a.K = hd->K;
  a.act = hd->reserved0;
  launch_resample(vec, in_dtype, hd->reduce, hd->out_dtype, a, BackLaunch{(unsigned)hd->units, 0u, stream});
  AA_HIP_CHECK_LAUNCH();
  return AA_OK;
}

// ---- host: the merged planner --------------------------------------------------------------------------------------------------------------
size_t aa_back_merged_desc_size(int64_t n, int64_t g) {
  if (n < 0 || g < 0) return 0;
  return sizeof(AABackMergedHeader) + (size_t)n * sizeof(AABackItem) + (size_t)g * sizeof(AABackGroup) + align8((size_t)n * sizeof(int32_t)) +
         ((size_t)g + 1) * sizeof(int64_t);
}

// aa_back_plan_host's checks in its order, with G and merge beside n, K and reduce; the groups' membership after the block's size and
// before the items; a member's size against its group's after the member's own checks; the arena and the work units per GROUP.
int aa_back_merged_plan_host(int filter, int layout, int64_t n, int64_t K, const aa_back_item *in, int64_t G, const int64_t *group_of, int merge,
                             int reduce, int activation, int out_dtype, void *desc_host, size_t desc_bytes, size_t *workspace_bytes, size_t *arena_bytes,
                             int64_t *out_offsets) {
  const bool own_ok = G >= 0 && G <= n && (G > 0 || n == 0) && (merge == AA_BACK_MERGE_SUM || merge == AA_BACK_MERGE_MEAN);
  int rc = plan_prologue(filter, layout, n, K, reduce, activation, out_dtype, own_ok);
  if (rc != AA_OK) return rc;
  if (!desc_host || !workspace_bytes || !arena_bytes || (n > 0 && (!in || !group_of || !out_offsets))) return AA_ERR_NULL;
  if (desc_bytes < aa_back_merged_desc_size(n, G)) return AA_ERR_WORKSPACE;
  const size_t eb = elem_bytes(out_dtype);
  AABackMergedHeader *hd = (AABackMergedHeader *)desc_host;
  AABackItem *items = (AABackItem *)(hd + 1);
  AABackGroup *groups = (AABackGroup *)(items + n);
  int32_t *member = (int32_t *)(groups + G);
  int64_t *unit0 = (int64_t *)((char *)member + align8((size_t)n * sizeof(int32_t)));
  // the groups' members: counted, then the slots handed out in item order, so a group's members ascend
  memset(groups, 0, (size_t)G * sizeof(AABackGroup));
  for (int64_t i = 0; i < n; i++) {
    if (group_of[i] < 0 || group_of[i] >= G) return AA_ERR_BAD_SHAPE;
    groups[group_of[i]].count++;
  }
  int32_t slot = 0;
  for (int64_t g = 0; g < G; g++) {
    if (groups[g].count == 0) return AA_ERR_BAD_SHAPE;  // (an empty group)
    if (activation == AA_BACK_ACT_SOFTMAX && groups[g].count > AA_BACK_ACT_MEMBERS) return AA_ERR_BAD_SHAPE;  // (the pairs of a lane: LDS)
    groups[g].first = slot;
    slot += groups[g].count;
    groups[g].count = 0;  // (counted up again as the slots are filled)
  }
  size_t ws = 0, arena = 0;
  int64_t units = 0;
  for (int64_t i = 0; i < n; i++) {
    AABackItem &it = items[i];
    if ((rc = plan_item(filter, layout, K, in[i], it, ws)) != AA_OK) return rc;
    AABackGroup &gr = groups[group_of[i]];
    if (gr.count == 0) {
      gr.oh = it.oh; gr.ow = it.ow; gr.xtiles = it.xtiles;
    } else if (gr.oh != it.oh || gr.ow != it.ow) {
      return AA_ERR_BAD_SHAPE;  // (the members of a group have one size)
    }
    member[gr.first + gr.count++] = (int32_t)i;
  }
  for (int64_t g = 0; g < G; g++) {
    AABackGroup &gr = groups[g];
    unit0[g] = units;
    if ((rc = plan_output(K, reduce, eb, gr.oh, gr.ow, gr.xtiles, arena, units, &gr.out_off)) != AA_OK) return rc;
    out_offsets[g] = gr.out_off;
  }
  unit0[G] = units;
  for (int64_t i = 0; i < n; i++) items[i].out_off = groups[group_of[i]].out_off;
  if (n % 2) member[n] = 0;  // (the padding)
  if (!out_dtype_ok(reduce, out_dtype)) return AA_ERR_BAD_DTYPE;
  memset(hd, 0, sizeof(*hd));
  hd->magic = AA_BACK_MERGED_MAGIC;
  hd->n = (int32_t)n; hd->K = (int32_t)K; hd->filter = filter; hd->layout = layout;
  hd->reduce = reduce; hd->out_dtype = out_dtype; hd->merge = merge;
  hd->units = units;
  hd->ws_bytes = (int64_t)ws;
  hd->arena_bytes = (int64_t)arena;
  hd->G = (int32_t)G;
  hd->reserved = activation;
  *workspace_bytes = ws;
  *arena_bytes = arena;
  return AA_OK;
}

// ---- host: the merged call's two launches --------------------------------------------------------------------------------------------------
// aa_launch_back_many's checks, every one before the first launch; the table kernel is its own, over the members.
int aa_launch_back_merged(const void *desc_host, const void *desc_dev, int in_dtype, float threshold, void *arena_dev, size_t arena_bytes,
                          void *workspace_dev, size_t workspace_bytes, hipStream_t stream) {
  const AABackMergedHeader *hd = (const AABackMergedHeader *)desc_host;
  if (hd->magic != AA_BACK_MERGED_MAGIC || !aa_filter_valid(hd->filter) || hd->n < 0 || hd->K < 1 || hd->units < 0 || hd->units > INT32_MAX ||
      hd->reduce < AA_BACK_VALUES || hd->reduce > AA_BACK_GREATER || (hd->layout != AA_NCHW && hd->layout != AA_NHWC) || hd->G < 0 ||
      hd->G > hd->n || (hd->G == 0 && hd->n > 0) || (hd->merge != AA_BACK_MERGE_SUM && hd->merge != AA_BACK_MERGE_MEAN) || !act_ok(hd->reserved))
    return AA_ERR_BAD_SHAPE;
  // a softmax plan's largest group, which the planner bounded: part of what makes the block a plan's, so looked at with the header
  int most = 0;
  if (hd->reserved == AA_BACK_ACT_SOFTMAX) {
    const AABackGroup *host_groups = (const AABackGroup *)((const AABackItem *)(hd + 1) + hd->n);
    for (int32_t g = 0; g < hd->G; g++) most = host_groups[g].count > most ? host_groups[g].count : most;
    if (most > AA_BACK_ACT_MEMBERS) return AA_ERR_BAD_SHAPE;
  }
  if (!float_dtype(in_dtype) || !out_dtype_ok(hd->reduce, hd->out_dtype)) return AA_ERR_BAD_DTYPE;
  if (hd->reduce == AA_BACK_GREATER && !(threshold - threshold == 0.0f)) return AA_ERR_BAD_SHAPE;  // (not finite)
  const int rc = aa_many_check_launch(hd->n, desc_dev, arena_dev, workspace_dev, workspace_bytes, hd->ws_bytes, elem_bytes(hd->out_dtype));
  if (rc != AA_OK || hd->n == 0) return rc;
  if (arena_bytes < (size_t)hd->arena_bytes) return AA_ERR_WORKSPACE;
  bool vec;
  const int rs = check_sources((const AABackItem *)(hd + 1), hd->n, in_dtype, hd->layout, hd->K, &vec);
  if (rs != AA_OK) return rs;
  MergedArgs a;
  a.items = (const AABackItem *)((const char *)desc_dev + sizeof(AABackMergedHeader));
  a.groups = (const AABackGroup *)(a.items + hd->n);
  a.member = (const int32_t *)(a.groups + hd->G);
  a.unit0 = (const int64_t *)((const char *)a.member + align8((size_t)hd->n * sizeof(int32_t)));
  a.ws = (const char *)workspace_dev; a.arena = (char *)arena_dev;
  a.threshold = threshold;
  a.G = hd->G; a.K = hd->K; a.mean = hd->merge == AA_BACK_MERGE_MEAN;
  a.act = hd->reserved;
  // a softmax's pairs: AA_BACK_TILE of them per member of the plan's largest group; the device the launches go to — the stream's, for
  // the null stream the current one — must admit that much LDS a workgroup
  unsigned lds = 0;
  if (a.act == AA_BACK_ACT_SOFTMAX) {
    lds = (unsigned)most * AA_BACK_TILE * (unsigned)sizeof(SoftmaxPair);
    hipDevice_t dev = 0;
    int limit = 0;
    if (hipStreamGetDevice(stream, &dev) != hipSuccess || hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) {
      (void)hipGetLastError();
      return AA_ERR_HIP;
    }
    if ((int64_t)lds > (int64_t)limit) return AA_ERR_BAD_SHAPE;
  }
  hipLaunchKernelGGL(back_tables, dim3(2u * (unsigned)hd->n), dim3(AA_BACK_THREADS), 0, stream, a.items, (char *)workspace_dev, (int)hd->filter);
  AA_HIP_CHECK_LAUNCH();
  launch_resample(vec, in_dtype, hd->reduce, hd->out_dtype, a, BackLaunch{(unsigned)hd->units, lds, stream});
  AA_HIP_CHECK_LAUNCH();
  return AA_OK;
}
