// aa_many_back_shared.h — what the files of the ragged return path share (aa_many_back.hip: values, labels and masks;
// aa_many_back_confusion.hip: confusion matrices; aa_many_back_queries.hip and aa_many_back_panoptic.hip: mask-classification heads):
// the counts of a wave and the geometry of a row tile for the files that count, the argument blocks of the resamples, the classes of one pixel of an item and of a
// group as an epilogue sees them (each_class, the activation's walks, the merged member loop), the argmax rule, and on the host what the
// planners check first, the record of an item, the slots of a merged plan's groups and what a launch checks of the sources.  Each is
// written here once.  In the unnamed namespace like the kernels that use it; only for files built with -ffp-contract=off -fno-fast-math
// (aa_activation.h, aa_table_rows.h).
#pragma once

#include <string.h>

#include "aa_many_back.h"
#include "aa_activation.h"
#include "aa_float_many_dev.h"
#include "aa_float_many_host.h"

namespace {

// ---- the argmax rule -----------------------------------------------------------------------------------------------------------------------
// put(k, v): class k's fp32 value of the lane's pixel, k ascending.  The lowest k of the greatest value, a NaN greater than every number
// and the first NaN kept: numpy.argmax.
struct ArgmaxRule {
  float best;
  int idx;
  __device__ ArgmaxRule() : best(0.0f), idx(0) {}
  __device__ void put(int k, float v) {
    if (k == 0 || (best == best && (v > best || v != v))) {
      best = v;
      idx = k;
    }
  }
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

// epi.put(k, v) for the K classes of pixel (y, x) of item `it`, x the UNFLIPPED column.  With ACT the value an epilogue sees is the
// activation's: the sigmoid of the class's value, or — after a first walk over the classes for the pixel's maximum and denominator —
// its softmax term.  Both K loops of each walk are each_class's.
template <typename TIn, bool VEC, bool ACT, typename Epi>
__device__ inline void item_classes(const BackArgs &a, const AABackItem &it, int y, int x, Epi &epi) {
  const Row ry = table_row(a.ws + it.tab_h, it.h, it.oh, it.ksize_h, y), rx = table_row(a.ws + it.tab_w, it.w, it.ow, it.ksize_w, x);
  const int64_t sch = it.stride_ch, prow = it.stride_row, ppx = it.stride_px;
  const TIn *p = (const TIn *)it.src + ry.x0 * prow + rx.x0 * ppx;
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
}

// ---- merged: the members of a group ----------------------------------------------------------------------------------------------------------
// The class chunk is the outer loop and the group's members the inner one, so the epilogue sees a class's complete sum: the first
// member's value, then one fp32 add per further member, in ascending item order (member[] is in that order), then for the mean one
// correctly rounded division by the count.  A flipped member is mirrored where it is READ: lane x walks that member's horizontal
// window of column ow - 1 - x.  A member's two table rows are looked up again per class chunk (a few cached words; the member index is
// uniform over the workgroup) rather than kept per member, so there is no limit on the members of a group and nothing is indexed
// dynamically in registers.
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
// member's own windows, mirrored where it is read like phase two) and leaves the pair in its LDS slot, act_pairs[m * AA_BACK_TILE +
// lane] (the lane reads only what it wrote: no barrier).  The launch sizes that LDS for the plan's largest group (AA_BACK_TILE pairs a
// member; nothing for a sigmoid), and the planner bounds that group.
template <typename TIn, bool VEC>
__device__ inline void member_pairs(const MergedArgs &a, const AABackGroup &gr, int y, int x, SoftmaxPair *act_pairs) {
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

// epi.put(k, v) for the K merged classes of pixel (y, x) of group gr; pairs: the lane's first pair (ACT and a softmax, after member_pairs).
template <typename TIn, bool VEC, bool ACT, typename Epi>
__device__ inline void group_classes(const MergedArgs &a, const AABackGroup &gr, int y, int x, const SoftmaxPair *pairs, Epi &epi) {
  constexpr int U = AA_BACK_UNROLL;
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
}

// ---- the counts of a wave ------------------------------------------------------------------------------------------------------------------
// (aa_many_back_confusion.hip: key = target * K + label; aa_many_back_panoptic.hip: key = 2 * winner + inside)
constexpr unsigned long long kCountMask = (1ull << AA_BACK_CONF_COUNT_BITS) - 1;

// Where a confusion matrix's (key, count) goes: element `key` of the output's K x K block.
struct ConfSink {
  unsigned long long *conf;
  __device__ void operator()(unsigned long long key, unsigned long long count) const { atomicAdd(conf + key, count); }
};

// slots: the wave's AA_BACK_CONF_SLOTS words of LDS, each key << AA_BACK_CONF_COUNT_BITS | count, 0 an empty slot (a count is never 0
// otherwise).  sink(key, count): what leaves a slot goes to the result, by 64-bit integer atomic adds.  Every method is called by all 64
// lanes of the wave together.  Lane 0 writes what lane
// s reads back: the accesses are relaxed atomics of wavefront scope with a fence of that scope where lanes meet, so that the compiler
// keeps them in program order and in LDS; a wave's LDS operations complete in the order it issued them, so none of this costs a wait.
template <typename Sink> struct WaveCounts {
  unsigned long long *slots;
  Sink sink;
  int lane;

  __device__ static unsigned long long get(const unsigned long long *s) { return __hip_atomic_load(s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
  __device__ static void set(unsigned long long *s, unsigned long long v) { __hip_atomic_store(s, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
  __device__ static void lanes_meet() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }

  __device__ void clear() {
    set(slots + lane, 0);
    lanes_meet();
  }

  // `count` pixels of `key` (both uniform over the wave) into the key's slot; what another key left there goes to the sink first.
  __device__ void add(int64_t key, unsigned count) {
    if (lane != 0) return;
    unsigned long long *s = slots + (key % AA_BACK_CONF_SLOTS);
    unsigned long long held = get(s);
    if (held != 0 && (int64_t)(held >> AA_BACK_CONF_COUNT_BITS) != key) {
      sink(held >> AA_BACK_CONF_COUNT_BITS, held & kCountMask);
      held = 0;
    }
    set(s, (held != 0 ? held : (unsigned long long)key << AA_BACK_CONF_COUNT_BITS) + count);
  }

  // One row: the lanes with `active` hold `key`.  The first live lane's key, the ballot of the lanes that hold it, their count to the
  // table, and they retire; until none is live.
  __device__ void count_row(bool active, int64_t key) {
    unsigned long long live = __ballot(active);
    while (live != 0) {  // (uniform)
      const int first = __builtin_ctzll(live);
      const int64_t k0 = ((int64_t)__builtin_amdgcn_readlane((int)(key >> 32), first) << 32) | (unsigned)__builtin_amdgcn_readlane((int)key, first);
      const unsigned long long same = __ballot(active && key == k0);
      add(k0, (unsigned)__popcll(same));
      live &= ~same;
    }
  }

  // After the last row: lane s hands slot s to the sink.
  __device__ void flush() {
    lanes_meet();
    const unsigned long long held = get(slots + lane);
    if (held != 0) sink(held >> AA_BACK_CONF_COUNT_BITS, held & kCountMask);
  }
};

// The rows [y0, y1) of a unit's tile of ROWS rows and the lane's column; false for a wave wholly beyond ow, which leaves.
struct RowTile { int y0, y1, x; };
template <int ROWS> __device__ inline bool row_tile(int64_t u, int xtiles, int oh, int ow, RowTile &t) {
  const int ty = (int)(u / xtiles);
  t.x = (int)(u - (int64_t)ty * xtiles) * AA_BACK_TILE + (int)threadIdx.x;
  t.y0 = ty * ROWS;
  t.y1 = t.y0 + ROWS < oh ? t.y0 + ROWS : oh;
  return t.x - (int)(threadIdx.x & 63) < ow;
}

// The workgroups of a table launch that zero a result of int64 counts, AA_BACK_CONF_ZERO elements at a time: workgroup b of `blocks`.
__device__ inline void zero_counts(int64_t *counts, int64_t elems, int64_t b, int64_t blocks) {
  const int64_t step = blocks * AA_BACK_CONF_ZERO;
  for (int64_t base = b * AA_BACK_CONF_ZERO; base < elems; base += step) {
    const int64_t end = base + AA_BACK_CONF_ZERO < elems ? base + AA_BACK_CONF_ZERO : elems;
    for (int64_t e = base + threadIdx.x; e < end; e += AA_BACK_THREADS) counts[e] = 0;
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------
// The workgroups that zero: one per AA_BACK_CONF_ZERO elements, 65536 at most (they stride).
inline unsigned zero_blocks(int64_t elems) {
  const int64_t b = (elems + AA_BACK_CONF_ZERO - 1) / AA_BACK_CONF_ZERO;
  return (unsigned)(b < 65536 ? b : 65536);
}

inline bool act_ok(int activation) { return activation >= AA_BACK_ACT_NONE && activation <= AA_BACK_ACT_SIGMOID; }

// What the planners check first, in this order: the filter; the layout; n, K, reduce and the activation (own_ok: what the caller adds to
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

inline size_t align8(size_t v) { return (v + 7) & ~(size_t)7; }

// The sections of a merged plan's block after its 64-byte header:
//   [ AABackItem x n ][ AABackGroup x G ][ int32 member[n], padded to 8 B ][ int64 unit0[G + 1] ]
inline size_t merged_sections_size(int64_t n, int64_t g) {
  return (size_t)n * sizeof(AABackItem) + (size_t)g * sizeof(AABackGroup) + align8((size_t)n * sizeof(int32_t)) + ((size_t)g + 1) * sizeof(int64_t);
}

// The groups' members of a merged plan: counted, then the slots handed out in item order, so a group's members ascend; every count is
// left at 0, to be counted up again as plan_members fills the slots.  AA_ERR_BAD_SHAPE for a group_of entry outside 0 .. G - 1, then
// for an empty group, then for a softmax group of more than AA_BACK_ACT_MEMBERS (the pairs of a lane: LDS).
inline int plan_group_slots(int64_t n, int64_t G, const int64_t *group_of, int activation, AABackGroup *groups) {
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
  return AA_OK;
}

// The members' records, each checked as an item and then against its group's size (the first member's), and the member list.
inline int plan_members(int filter, int layout, int64_t n, int64_t K, const aa_back_item *in, const int64_t *group_of, AABackItem *items,
                        AABackGroup *groups, int32_t *member, size_t &ws) {
  for (int64_t i = 0; i < n; i++) {
    AABackItem &it = items[i];
    const int rc = plan_item(filter, layout, K, in[i], it, ws);
    if (rc != AA_OK) return rc;
    AABackGroup &gr = groups[group_of[i]];
    if (gr.count == 0) {
      gr.oh = it.oh; gr.ow = it.ow; gr.xtiles = it.xtiles;
    } else if (gr.oh != it.oh || gr.ow != it.ow) {
      return AA_ERR_BAD_SHAPE;  // (the members of a group have one size)
    }
    member[gr.first + gr.count++] = (int32_t)i;
  }
  return AA_OK;
}

// What the launches check of the planned items' pointers, which the planner could not: against the element of in_dtype, and for
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

// A softmax plan's largest group against the bound, and the LDS its pairs need against the limit of the device the launches go to —
// the stream's, for the null stream the current one: -> the bytes in *lds (0 without a softmax).
inline int softmax_pairs_lds(int activation, int most, hipStream_t stream, unsigned *lds) {
  *lds = 0;
  if (activation != AA_BACK_ACT_SOFTMAX) return AA_OK;
  *lds = (unsigned)most * AA_BACK_TILE * (unsigned)sizeof(SoftmaxPair);
  hipDevice_t dev = 0;
  int limit = 0;
  if (hipStreamGetDevice(stream, &dev) != hipSuccess || hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) {
    (void)hipGetLastError();
    return AA_ERR_HIP;
  }
  return (int64_t)*lds > (int64_t)limit ? AA_ERR_BAD_SHAPE : AA_OK;
}

}  // namespace
