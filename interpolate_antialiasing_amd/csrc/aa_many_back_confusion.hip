// aa_many_back_confusion.hip — per-image confusion matrices of the ragged return path: conf[i, t, p] = the pixels of output i whose target
// is t and whose label — aa_many_back.hip's argmax, plain or merged, with or without an activation, bit for bit — is p.  A target outside
// 0 .. K - 1 is not counted.  Neither the K values of a pixel nor its label reach memory: K x K int64 counts per output do.  Two launches
// whatever n and whatever the sizes:
//   1. conf_tables    workgroups 0 .. 2 n - 1 build the items' tables as back_tables does (table_axis_build, aa_float_many_dev.h); the
//                     workgroups after them zero the whole result, AA_BACK_CONF_ZERO elements at a time.  No memset, no third launch.
//   2. conf_resample  one workgroup per work unit, AA_BACK_CONF_ROWS consecutive output rows times AA_BACK_TILE columns of one output,
//      (_merged)      a lane per column, walking down the rows.  Per row the lane computes its pixel's label with the class loops of
//                     aa_many_back_shared.h (item_classes; member_pairs and group_classes), loads its target and forms the key
//                     t * K + p.  The wave then aggregates: while a lane is live, the first live lane's key is broadcast, the lanes
//                     holding it are balloted, counted and retired — neighbouring pixels mostly share a key, so one to three rounds a
//                     row — and (key, count) goes to the wave's table in LDS: AA_BACK_CONF_SLOTS slots of key << 16 | count, indexed by
//                     key % slots.  The same key adds to its slot; another key evicts the old pair with one 64-bit integer atomic add
//                     to conf.  After the last row lane s flushes slot s.  A wave's slots are its own, so there is no barrier, a wave
//                     wholly beyond ow leaves at once, and the merged softmax's per-lane pairs stay what they are.
// The only global writes of launch 2 are those atomic adds; integer adds commute, so the bits do not depend on n, on the launch shape
// or on the run.  The target's element type is a field uniform over the launch, not a template parameter: TIn x VEC x ACT kernels per
// form.  Every element offset is 64-bit.  Plain C++ and vector memory operations only.

#include <string.h>

#include "aa_many_back_confusion.h"
#include "aa_many_back_shared.h"

namespace {

// ---- 1. tables, and the result zeroed ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(AA_BACK_THREADS) conf_tables(const AABackItem *items, int n, char *ws, int filter, int64_t *conf, int64_t conf_elems) {
  const int64_t b = (int64_t)blockIdx.x - 2 * (int64_t)n;
  if (b < 0) {  // (uniform over the workgroup: there are barriers in the body)
    const AABackItem &it = items[blockIdx.x >> 1];
    const bool horiz = blockIdx.x & 1;
    const TableAxis ax = {horiz ? it.w : it.h, horiz ? it.ow : it.oh, horiz ? it.ksize_w : it.ksize_h, 0, horiz ? it.scale_w : it.scale_h,
                          ws + (horiz ? it.tab_w : it.tab_h), nullptr};
    table_axis_build<AA_BACK_THREADS>(ax, filter, 0);
    return;
  }
  zero_counts(conf, conf_elems, b, (int64_t)gridDim.x - 2 * (int64_t)n);
}

// ---- what a lane counts (the wave's table, WaveCounts, and the tile's geometry: aa_many_back_shared.h) -------------------------------------
struct ConfArgs {
  const AABackConfTarget *targets;
  int64_t *conf;
  int target_dtype;  // AA_U8 / AA_I16 / AA_I32 / AA_I64
};

// Element e of a target, as an int64: uint8 is unsigned, the others signed.
__device__ inline int64_t load_target(const void *p, int64_t e, int dt) {
  if (dt == AA_U8) return ((const uint8_t *)p)[e];
  if (dt == AA_I16) return ((const int16_t *)p)[e];
  if (dt == AA_I32) return ((const int32_t *)p)[e];
  return ((const int64_t *)p)[e];
}

// The lane's key of target element e with label p, and whether it counts.
__device__ inline bool conf_key(const AABackConfTarget &tg, int64_t e, int dt, int K, int label, int64_t &key) {
  const int64_t t = load_target(tg.tgt, e, dt);
  const bool active = t >= 0 && t < K;
  key = active ? t * K + label : 0;
  return active;
}

// ---- 2. resample, argmax, count ------------------------------------------------------------------------------------------------------------
// A flipped item's column x is the label of column ow - 1 - x of the result: the target is read there.
template <typename TIn, bool VEC, bool ACT>
__global__ void __launch_bounds__(AA_BACK_TILE) conf_resample(BackArgs a, ConfArgs c) {
  __shared__ unsigned long long slots[AA_BACK_TILE / 64 * AA_BACK_CONF_SLOTS];
  const int64_t unit = blockIdx.x;
  const int item = aa_unit_item(a.unit0, a.n, unit);
  const AABackItem &it = a.items[item];
  const AABackConfTarget &tg = c.targets[item];
  RowTile t;
  if (!row_tile<AA_BACK_CONF_ROWS>(unit - a.unit0[item], it.xtiles, it.oh, it.ow, t)) return;  // (no barrier below)
  WaveCounts<ConfSink> wc = {slots + (threadIdx.x >> 6) * AA_BACK_CONF_SLOTS, {(unsigned long long *)c.conf + tg.conf_off}, (int)(threadIdx.x & 63)};
  wc.clear();
  const bool inside = t.x < it.ow;
  const int xs = (it.flags & AA_MANY_FLIP_X) ? it.ow - 1 - t.x : t.x;
  for (int y = t.y0; y < t.y1; y++) {
    bool active = false;
    int64_t key = 0;
    if (inside) {
      ArgmaxRule best;
      item_classes<TIn, VEC, ACT>(a, it, y, t.x, best);
      active = conf_key(tg, (int64_t)y * tg.stride_row + xs, c.target_dtype, a.K, best.idx, key);
    }
    wc.count_row(active, key);
  }
  wc.flush();
}

// 2'. merged: the label of column x of a group is computed at x (a flipped member is mirrored where it is read), so the target is read at x.
template <typename TIn, bool VEC, bool ACT>
__global__ void __launch_bounds__(AA_BACK_TILE) conf_resample_merged(MergedArgs a, ConfArgs c) {
  __shared__ unsigned long long slots[AA_BACK_TILE / 64 * AA_BACK_CONF_SLOTS];
  const int64_t unit = blockIdx.x;
  const int g = aa_unit_item(a.unit0, a.G, unit);
  const AABackGroup &gr = a.groups[g];
  const AABackConfTarget &tg = c.targets[g];
  RowTile t;
  if (!row_tile<AA_BACK_CONF_ROWS>(unit - a.unit0[g], gr.xtiles, gr.oh, gr.ow, t)) return;  // (no barrier below)
  WaveCounts<ConfSink> wc = {slots + (threadIdx.x >> 6) * AA_BACK_CONF_SLOTS, {(unsigned long long *)c.conf + tg.conf_off}, (int)(threadIdx.x & 63)};
  wc.clear();
  const bool inside = t.x < gr.ow;
  const SoftmaxPair *pairs = nullptr;
  SoftmaxPair *all_pairs = nullptr;
  if constexpr (ACT) {
    extern __shared__ __attribute__((aligned(8))) SoftmaxPair act_pairs[];
    all_pairs = act_pairs;
    pairs = act_pairs + threadIdx.x;
  }
  for (int y = t.y0; y < t.y1; y++) {
    bool active = false;
    int64_t key = 0;
    if (inside) {
      if constexpr (ACT) {
        if (a.act == AA_BACK_ACT_SOFTMAX) member_pairs<TIn, VEC>(a, gr, y, t.x, all_pairs);
      }
      ArgmaxRule best;
      group_classes<TIn, VEC, ACT>(a, gr, y, t.x, pairs, best);
      active = conf_key(tg, (int64_t)y * tg.stride_row + t.x, c.target_dtype, a.K, best.idx, key);
    }
    wc.count_row(active, key);
  }
  wc.flush();
}

struct ConfLaunch {
  unsigned units, lds;
  hipStream_t stream;
};
template <typename TIn, bool VEC, bool ACT> void launch_as(const BackArgs &a, const ConfArgs &c, const ConfLaunch &l) {
  hipLaunchKernelGGL((conf_resample<TIn, VEC, ACT>), dim3(l.units), dim3(AA_BACK_TILE), 0, l.stream, a, c);
}
template <typename TIn, bool VEC, bool ACT> void launch_as(const MergedArgs &a, const ConfArgs &c, const ConfLaunch &l) {
  hipLaunchKernelGGL((conf_resample_merged<TIn, VEC, ACT>), dim3(l.units), dim3(AA_BACK_TILE), ACT ? l.lds : 0, l.stream, a, c);
}
template <bool VEC, bool ACT, typename Args> void launch_in(int in_dtype, const Args &a, const ConfArgs &c, const ConfLaunch &l) {
  with_float_type(in_dtype, [&](auto in) { launch_as<tag_t<decltype(in)>, VEC, ACT>(a, c, l); });
}
// The kernel of (vector loads or not, an activation or not): a.act says which.
template <typename Args> void launch_resample(bool vec, int in_dtype, const Args &a, const ConfArgs &c, const ConfLaunch &l) {
  if (a.act != AA_BACK_ACT_NONE) {
    if (vec) launch_in<true, true>(in_dtype, a, c, l);
    else launch_in<false, true>(in_dtype, a, c, l);
  } else if (vec) launch_in<true, false>(in_dtype, a, c, l);
  else launch_in<false, false>(in_dtype, a, c, l);
}

inline bool target_dtype_ok(int dt) { return dt == AA_U8 || dt == AA_I16 || dt == AA_I32 || dt == AA_I64; }

// The sections of a block, of the host's copy or of the device's: groups and member only for a merged plan.
struct ConfSections {
  const AABackItem *items;
  const AABackGroup *groups;
  const int32_t *member;
  const int64_t *unit0;
  const AABackConfTarget *targets;
};
inline ConfSections conf_sections(const void *block, int64_t n, int64_t G, int merged) {
  ConfSections s = {(const AABackItem *)((const char *)block + sizeof(AABackConfHeader)), nullptr, nullptr, nullptr, nullptr};
  if (merged) {
    s.groups = (const AABackGroup *)(s.items + n);
    s.member = (const int32_t *)(s.groups + G);
    s.unit0 = (const int64_t *)((const char *)s.member + align8((size_t)n * sizeof(int32_t)));
  } else {
    s.unit0 = (const int64_t *)(s.items + n);
  }
  s.targets = (const AABackConfTarget *)(s.unit0 + (merged ? G : n) + 1);
  return s;
}

}  // namespace

// ---- host: the planner ---------------------------------------------------------------------------------------------------------------------
size_t aa_back_conf_desc_size(int64_t n, int64_t g, int merged) {
  if (n < 0 || g < 0) return 0;
  const size_t outs = (size_t)(merged ? g : n);
  return (merged ? sizeof(AABackConfHeader) + merged_sections_size(n, g) : aa_desc_size(sizeof(AABackConfHeader), sizeof(AABackItem), n)) +
         outs * sizeof(AABackConfTarget);
}

// aa_back_plan_host's checks in its order (the merged form: aa_back_merged_plan_host's), the reduce an argmax to int64; K * K * outputs
// against AA_BACK_MAX_ELEMS beside n and K; `targets` beside the pointers; after an item's (a group's members') checks the output's
// target: AA_ERR_NULL, AA_ERR_STRIDES for a negative row stride, AA_ERR_BAD_SHAPE for more work units than one grid holds; last
// AA_ERR_BAD_DTYPE for a target type that is no integer of 1, 2, 4 or 8 bytes.
int aa_back_conf_plan_host(int filter, int layout, int64_t n, int64_t K, const aa_back_item *in, int merged, int64_t G, const int64_t *group_of,
                           int merge, const aa_back_target *targets, int target_dtype, int activation, void *desc_host, size_t desc_bytes,
                           size_t *workspace_bytes, int64_t *conf_elems) {
  merged = merged != 0;
  const int64_t outs = merged ? G : n;
  bool own_ok = !merged || (G >= 0 && G <= n && (G > 0 || n == 0) && (merge == AA_BACK_MERGE_SUM || merge == AA_BACK_MERGE_MEAN));
  own_ok = own_ok && (outs <= 0 || K < 1 || K > kAAManyMax || K * K <= AA_BACK_MAX_ELEMS / outs);
  int rc = plan_prologue(filter, layout, n, K, AA_BACK_ARGMAX, activation, AA_I64, own_ok);
  if (rc != AA_OK) return rc;
  if (!desc_host || !workspace_bytes || !conf_elems || (n > 0 && (!in || !targets || (merged && !group_of)))) return AA_ERR_NULL;
  if (desc_bytes < aa_back_conf_desc_size(n, G, merged)) return AA_ERR_WORKSPACE;
  AABackConfHeader *hd = (AABackConfHeader *)desc_host;
  const ConfSections s = conf_sections(desc_host, n, G, merged);
  AABackItem *items = (AABackItem *)s.items;
  AABackGroup *groups = (AABackGroup *)s.groups;
  int32_t *member = (int32_t *)s.member;
  int64_t *unit0 = (int64_t *)s.unit0;
  AABackConfTarget *tgs = (AABackConfTarget *)s.targets;
  size_t ws = 0;
  int64_t units = 0;
  if (merged) {
    if ((rc = plan_group_slots(n, G, group_of, activation, groups)) != AA_OK) return rc;
    if ((rc = plan_members(filter, layout, n, K, in, group_of, items, groups, member, ws)) != AA_OK) return rc;
    if (n % 2) member[n] = 0;  // (the padding)
  }
  for (int64_t i = 0; i < outs; i++) {
    int64_t oh, xtiles;
    if (merged) {
      oh = groups[i].oh; xtiles = groups[i].xtiles;
    } else {
      if ((rc = plan_item(filter, layout, K, in[i], items[i], ws)) != AA_OK) return rc;
      oh = items[i].oh; xtiles = items[i].xtiles;
    }
    if (!targets[i].data_dev) return AA_ERR_NULL;
    if (oh > 1 && targets[i].stride_row < 0) return AA_ERR_STRIDES;
    AABackConfTarget &tg = tgs[i];
    tg.tgt = targets[i].data_dev;
    tg.stride_row = oh > 1 ? targets[i].stride_row : 0;
    tg.conf_off = i * K * K;
    tg.ytiles = (int32_t)((oh + AA_BACK_CONF_ROWS - 1) / AA_BACK_CONF_ROWS);
    tg.reserved = 0;
    unit0[i] = units;
    units += (int64_t)tg.ytiles * xtiles;
    if (units > INT32_MAX) return AA_ERR_BAD_SHAPE;  // (one grid)
  }
  unit0[outs] = units;
  if (!target_dtype_ok(target_dtype)) return AA_ERR_BAD_DTYPE;
  memset(hd, 0, sizeof(*hd));
  hd->magic = AA_BACK_CONF_MAGIC;
  hd->n = (int32_t)n; hd->K = (int32_t)K; hd->filter = filter; hd->layout = layout;
  hd->activation = activation; hd->target_dtype = target_dtype; hd->merge = merged ? merge : 0;
  hd->units = units;
  hd->ws_bytes = (int64_t)ws;
  hd->conf_elems = outs * K * K;
  hd->G = merged ? (int32_t)G : 0;
  hd->merged = merged;
  *workspace_bytes = ws;
  *conf_elems = hd->conf_elems;
  return AA_OK;
}

// ---- host: the two launches ----------------------------------------------------------------------------------------------------------------
// aa_launch_back_many's checks (aa_launch_back_merged's for a merged plan) in their order, every one before the first launch; the
// targets' alignment to their element beside the sources'.
int aa_launch_back_confusion(const void *desc_host, const void *desc_dev, int in_dtype, void *conf_dev, size_t conf_elems, void *workspace_dev,
                             size_t workspace_bytes, hipStream_t stream) {
  const AABackConfHeader *hd = (const AABackConfHeader *)desc_host;
  if (hd->magic != AA_BACK_CONF_MAGIC || !aa_filter_valid(hd->filter) || hd->n < 0 || hd->K < 1 || hd->units < 0 || hd->units > INT32_MAX ||
      (hd->layout != AA_NCHW && hd->layout != AA_NHWC) || !act_ok(hd->activation) || (hd->merged != 0 && hd->merged != 1) || hd->G < 0 ||
      (hd->merged ? (hd->G > hd->n || (hd->G == 0 && hd->n > 0) || (hd->merge != AA_BACK_MERGE_SUM && hd->merge != AA_BACK_MERGE_MEAN)) : hd->G != 0) ||
      hd->conf_elems != (int64_t)(hd->merged ? hd->G : hd->n) * hd->K * hd->K)
    return AA_ERR_BAD_SHAPE;
  const ConfSections host = conf_sections(desc_host, hd->n, hd->G, hd->merged);
  int most = 0;
  if (hd->merged && hd->activation == AA_BACK_ACT_SOFTMAX) {
    for (int32_t g = 0; g < hd->G; g++) most = host.groups[g].count > most ? host.groups[g].count : most;
    if (most > AA_BACK_ACT_MEMBERS) return AA_ERR_BAD_SHAPE;
  }
  if (!float_dtype(in_dtype) || !target_dtype_ok(hd->target_dtype)) return AA_ERR_BAD_DTYPE;
  const int rc = aa_many_check_launch(hd->n, desc_dev, conf_dev, workspace_dev, workspace_bytes, hd->ws_bytes, sizeof(int64_t));
  if (rc != AA_OK || hd->n == 0) return rc;
  if (conf_elems < (size_t)hd->conf_elems) return AA_ERR_WORKSPACE;
  bool vec;
  const int rs = check_sources(host.items, hd->n, in_dtype, hd->layout, hd->K, &vec);
  if (rs != AA_OK) return rs;
  const int64_t outs = hd->merged ? hd->G : hd->n;
  for (int64_t i = 0; i < outs; i++)
    if ((uintptr_t)host.targets[i].tgt % elem_bytes(hd->target_dtype)) return AA_ERR_STRIDES;
  unsigned lds;
  const int rl = softmax_pairs_lds(hd->merged ? hd->activation : AA_BACK_ACT_NONE, most, stream, &lds);
  if (rl != AA_OK) return rl;
  const ConfSections dev = conf_sections(desc_dev, hd->n, hd->G, hd->merged);
  hipLaunchKernelGGL(conf_tables, dim3(2u * (unsigned)hd->n + zero_blocks(hd->conf_elems)), dim3(AA_BACK_THREADS), 0, stream, dev.items, (int)hd->n,
                     (char *)workspace_dev, (int)hd->filter, (int64_t *)conf_dev, (int64_t)hd->conf_elems);
  AA_HIP_CHECK_LAUNCH();
  const ConfArgs c = {dev.targets, (int64_t *)conf_dev, hd->target_dtype};
  const ConfLaunch l = {(unsigned)hd->units, lds, stream};
  if (hd->merged) {
    MergedArgs a;
    a.items = dev.items; a.groups = dev.groups; a.member = dev.member; a.unit0 = dev.unit0;
    a.ws = (const char *)workspace_dev; a.arena = nullptr;
    a.threshold = 0.0f;
    a.G = hd->G; a.K = hd->K; a.mean = hd->merge == AA_BACK_MERGE_MEAN;
    a.act = hd->activation;
    launch_resample(vec, in_dtype, a, c, l);
  } else {
    BackArgs a;
    a.items = dev.items; a.unit0 = dev.unit0; a.ws = (const char *)workspace_dev; a.arena = nullptr;
    a.threshold = 0.0f;
    a.n = hd->n; a.K = hd->K;
    a.act = hd->activation;
    launch_resample(vec, in_dtype, a, c, l);
  }
  AA_HIP_CHECK_LAUNCH();
  return AA_OK;
}
