// aa_many_back_panoptic.hip — panoptic inference of mask-classification heads (MaskFormer, Mask2Former, OneFormer) in the ragged return
// path: item i is Q mask logits [Q, h_i, w_i] and Q float32 scores.  With R_i the fp32 resample of aa_many_back.hip (K = Q, bit for bit),
//   p[q]   = aa_sigmoid(R_i[q])                   aa_activation.h's sigmoid
//   v[q]   = scores[i, q] * p[q]                   ONE rounded fp32 product (the file is built with -ffp-contract=off)
//   winner = ArgmaxRule over the KEPT queries (scores[i, q] > 0) in ascending q; none where no query is kept
//   inside = p[winner] >= 0.5
// counts[i, q] = (area: pixels won by q; original: pixels with p[q] >= 0.5, kept queries only; inter: pixels won and inside), a query
// survives iff area, original and inter are positive and double(area) / double(original) >= overlap_threshold, and a pixel of the map is
// ids[i, winner] where the winner survives and the pixel is inside, `void` everywhere else.  Nothing here has a tolerance.  No matrix
// instruction fits: the work is an argmax and counting, not a product.  Three launches whatever n and whatever the sizes:
//   1. panoptic_tables    workgroups 0 .. 2 n - 1 build the items' tables as back_tables does (table_axis_build); workgroups 2 n ..
//                         3 n - 1 build one item's kept list each from the scores where they lie — lane t holds query t (or the chunk of
//                         AA_BACK_UNROLL queries from 4 t), a ballot per wave, the waves' counts meet in LDS behind the only barrier of
//                         the call, and every kept entry goes to its compacted place; the workgroups after them zero the counts.
//   2. panoptic_resample  one workgroup per work unit, AA_BACK_PANOPTIC_ROWS output rows times AA_BACK_TILE columns, a lane per column
//                         walking down the rows (the confusion kernel's shape).  The lane's horizontal table row is read once.  Per row
//                         it walks the item's kept list — uniform loads, a dropped query is never loaded — four kept queries a step
//                         (class_sums_at: four channel offsets) or, for items that take the vector loads, one aligned chunk a step with
//                         a mask of its kept members; per kept query one ballot of p >= 0.5 and one popcount, lane 0 adding it to the
//                         wave's own [Q] uint32 counters in LDS (original); the running winner is kept with its p in three registers.
//                         Then the provisional map element — the winner's index where inside, else the code Q — is stored in the
//                         arena, and the key 2 * winner + inside is counted by the wave (WaveCounts: area and inter).  After the last
//                         row the lanes flush all counters with 64-bit integer atomic adds.  A wave's LDS is its own: no barrier, and
//                         a wave wholly beyond ow leaves at once.  A lane beyond ow in a wave that stays computes column ow - 1 again
//                         (its column is CLAMPED, so the wave's control flow stays uniform and every address lies inside the item)
//                         and is masked out of every ballot and store.
//   3. panoptic_finalise  one workgroup per AA_BACK_PANOPTIC_FIN_BYTES of an item's map: it forms the item's lookup code -> ids[q] or
//                         void in LDS from the counts (the fp64 test), the item's first workgroup also writes survives, and the map is
//                         rewritten in place with 16-byte loads and stores wherever the absolute address allows.
// Integer adds commute, so counts, survives and map are the same bits on every run.  Every element offset is 64-bit.  Plain C++ and
// vector memory operations only.  Shared with the other files of the return path: aa_many_back_shared.h.

#include <string.h>

#include "aa_many_back_panoptic.h"
#include "aa_many_back_shared.h"

namespace {

constexpr int kRows = AA_BACK_PANOPTIC_ROWS, kMaxQ = AA_BACK_PANOPTIC_MAX_Q, kWaves = AA_BACK_TILE / 64;

// The scores (float32) or ids (int32) of the call: element (i, q) at p + i * stride_n + q * stride_q ELEMENTS.
template <typename T> struct PerQuery {
  const T *p;
  int64_t stride_n, stride_q;
};

struct KeptLists {
  int64_t off;  // of the workspace
  int words;    // int32 words of an item's list: [ count ][ entries ]
  int chunks;   // entries are q0 | mask << 16 (items that take the vector loads) rather than q
};
__device__ inline int32_t *kept_list(char *ws, const KeptLists &k, int item) { return (int32_t *)(ws + k.off) + (int64_t)item * k.words; }

// ---- 1. tables, kept lists, and the counts zeroed ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(AA_BACK_THREADS) panoptic_tables(const AABackItem *items, int n, int Q, char *ws, int filter, PerQuery<float> scores,
                                                                   KeptLists kept, int64_t *counts, int64_t count_elems) {
  __shared__ int wave_kept[AA_BACK_THREADS / 64];
  int64_t b = (int64_t)blockIdx.x - 2 * (int64_t)n;
  if (b < 0) {  // (uniform over the workgroup: there are barriers in the body)
    const AABackItem &it = items[blockIdx.x >> 1];
    const bool horiz = blockIdx.x & 1;
    const TableAxis ax = {horiz ? it.w : it.h, horiz ? it.ow : it.oh, horiz ? it.ksize_w : it.ksize_h, 0, horiz ? it.scale_w : it.scale_h,
                          ws + (horiz ? it.tab_w : it.tab_h), nullptr};
    table_axis_build<AA_BACK_THREADS>(ax, filter, 0);
    return;
  }
  if (b >= n) {
    zero_counts(counts, count_elems, b - n, (int64_t)gridDim.x - 3 * (int64_t)n);
    return;
  }
  // item b's kept list: a score that is NaN or not positive drops its query
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const float *s = scores.p + b * scores.stride_n;
  unsigned entry = 0;
  if (kept.chunks) {
    if (t * AA_BACK_UNROLL < Q) {  // (Q is a multiple of AA_BACK_UNROLL here: check_sources)
      unsigned mask = 0;
#pragma unroll
      for (int c = 0; c < AA_BACK_UNROLL; c++) mask |= (unsigned)(s[(int64_t)(t * AA_BACK_UNROLL + c) * scores.stride_q] > 0.0f) << c;
      entry = mask << 16 | (unsigned)(t * AA_BACK_UNROLL);
    }
  } else if (t < Q) {
    entry = s[(int64_t)t * scores.stride_q] > 0.0f ? 1u << 16 | (unsigned)t : 0;
  }
  const bool keep = entry >> 16 != 0;
  const unsigned long long mine = __ballot(keep);
  if (lane == 0) wave_kept[wave] = __popcll(mine);
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < AA_BACK_THREADS / 64; w++) {
    before += w < wave ? wave_kept[w] : 0;
    all += wave_kept[w];
  }
  int32_t *list = kept_list(ws, kept, (int)b);
  if (keep) list[1 + before + __popcll(mine & ((1ull << lane) - 1))] = (int32_t)(kept.chunks ? entry : entry & 0xFFFF);
  if (t == 0) list[0] = all;
}

// ---- 2. resample, winner, counts -----------------------------------------------------------------------------------------------------------
struct PanopticArgs {
  const AABackItem *items;
  const int64_t *unit0;
  const char *ws;
  char *arena;
  PerQuery<float> scores;
  KeptLists kept;
  int64_t *counts;
  int n, Q;
};

// ArgmaxRule over queries offered in ascending order that need not begin at 0, the winner's probability kept beside its value.
struct Winner {
  float best, p;
  int idx;
  __device__ void offer(int q, float v, float pq) {
    const bool take = (idx < 0) | ((best == best) & ((v > best) | (v != v)));
    best = take ? v : best;
    p = take ? pq : p;
    idx = take ? q : idx;
  }
};

// Where the (key, count) of a wave goes: key = 2 * winner + inside; area of every key, inter of the odd ones.
struct PanopticSink {
  unsigned long long *counts;  // the item's [Q, 3]
  __device__ void operator()(unsigned long long key, unsigned long long count) const {
    unsigned long long *c = counts + 3 * (key >> 1);
    atomicAdd(c, count);
    if (key & 1) atomicAdd(c + 2, count);
  }
};

template <typename TIn, bool VEC, typename TOut>
__global__ void __launch_bounds__(AA_BACK_TILE) panoptic_resample(PanopticArgs a) {
  __shared__ unsigned long long slots[kWaves * AA_BACK_CONF_SLOTS];
  __shared__ unsigned originals[kWaves * kMaxQ];
  const int64_t unit = blockIdx.x;
  const int item = aa_unit_item(a.unit0, a.n, unit);
  const AABackItem &it = a.items[item];
  RowTile t;
  if (!row_tile<kRows>(unit - a.unit0[item], it.xtiles, it.oh, it.ow, t)) return;  // (no barrier below)
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  unsigned long long *counts = (unsigned long long *)a.counts + (int64_t)item * a.Q * 3;
  WaveCounts<PanopticSink> wc = {slots + wave * AA_BACK_CONF_SLOTS, {counts}, lane};
  unsigned *orig = originals + wave * kMaxQ;
  for (int q = lane; q < a.Q; q += 64) __hip_atomic_store(orig + q, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
  wc.clear();  // (with the fence at which the lanes meet)

  const bool in = t.x < it.ow;
  const int xc = in ? t.x : it.ow - 1;  // (clamped: see the head of the file)
  const int xr = (it.flags & AA_MANY_FLIP_X) ? it.ow - 1 - xc : xc;
  const Row rx = table_row(a.ws + it.tab_w, it.w, it.ow, it.ksize_w, xr);
  const int64_t sch = it.stride_ch, prow = it.stride_row, ppx = it.stride_px;
  const int32_t *list = kept_list((char *)a.ws, a.kept, item);
  const int kept = __builtin_amdgcn_readfirstlane(list[0]);  // (the list is the item's: uniform, and said so to the compiler)
  const float *score = a.scores.p + (int64_t)item * a.scores.stride_n;
  const int64_t ssq = a.scores.stride_q;
  TOut *out = (TOut *)(a.arena + it.out_off);

  for (int y = t.y0; y < t.y1; y++) {
    const Row ry = table_row(a.ws + it.tab_h, it.h, it.oh, it.ksize_h, y);
    const TIn *p = (const TIn *)it.src + ry.x0 * prow + rx.x0 * ppx;
    Winner w = {0.0f, 0.0f, -1};
    // kept query q (uniform over the wave) with the lane's resampled logit
    auto offer = [&](int q, float logit) {
      const float pq = aa_sigmoid(logit);
      const float v = score[q * ssq] * pq;
      const unsigned hits = (unsigned)__popcll(__ballot(in && pq >= 0.5f));
      if (lane == 0 && hits != 0) __hip_atomic_fetch_add(orig + q, hits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
      w.offer(q, v, pq);
    };
    if constexpr (VEC) {
      for (int e = 1; e <= kept; e++) {
        const unsigned entry = (unsigned)__builtin_amdgcn_readfirstlane(list[e]);
        const int q0 = (int)(entry & 0xFFFF);
        float acc[AA_BACK_UNROLL];
        class_sums<TIn, AA_BACK_UNROLL, true>(p + q0 * sch, sch, prow, ppx, ry, rx, acc);
#pragma unroll
        for (int c = 0; c < AA_BACK_UNROLL; c++)
          if (entry >> (16 + c) & 1) offer(q0 + c, acc[c]);  // (uniform)
      }
    } else {
      constexpr int U = AA_BACK_UNROLL;
      int e = 1;
      for (; e + U <= kept + 1; e += U) {
        int q[U];
        int64_t off[U];
        float acc[U];
#pragma unroll
        for (int c = 0; c < U; c++) {
          q[c] = __builtin_amdgcn_readfirstlane(list[e + c]);
          off[c] = q[c] * sch;
        }
        class_sums_at<TIn, U>(p, off, prow, ppx, ry, rx, acc);
#pragma unroll
        for (int c = 0; c < U; c++) offer(q[c], acc[c]);
      }
      for (; e <= kept; e++) {
        const int q = __builtin_amdgcn_readfirstlane(list[e]);
        float acc[1];
        class_sums<TIn, 1, false>(p + q * sch, sch, prow, ppx, ry, rx, acc);
        offer(q, acc[0]);
      }
    }
    const bool won = in && w.idx >= 0, inside = won && w.p >= 0.5f;
    if (in) out[(int64_t)y * it.ow + t.x] = (TOut)(inside ? w.idx : a.Q);
    wc.count_row(won, won ? 2 * (int64_t)w.idx + (inside ? 1 : 0) : 0);
  }
  wc.flush();  // (with the fence at which the lanes meet)
  for (int q = lane; q < a.Q; q += 64) {
    const unsigned c = __hip_atomic_load(orig + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    if (c != 0) atomicAdd(counts + 3 * q + 1, (unsigned long long)c);
  }
}

// ---- 3. finalise ---------------------------------------------------------------------------------------------------------------------------
struct FinaliseArgs {
  const AABackItem *items;
  const int64_t *fin0;
  char *arena;
  const int64_t *counts;
  uint8_t *survives;
  PerQuery<int32_t> ids;  // p null: the query's index
  int64_t void_value;
  double threshold;
  int n, Q;
};

template <typename TOut> struct alignas(16) Piece { TOut v[16 / sizeof(TOut)]; };

template <typename TOut>
__global__ void __launch_bounds__(AA_BACK_THREADS) panoptic_finalise(FinaliseArgs f) {
  __shared__ TOut lut[kMaxQ + 1];
  const int64_t unit = blockIdx.x;
  const int item = aa_unit_item(f.fin0, f.n, unit);
  const int64_t u = unit - f.fin0[item];
  for (int q = (int)threadIdx.x; q <= f.Q; q += AA_BACK_THREADS) {
    TOut v = (TOut)f.void_value;  // (code Q: no winner, or not inside)
    if (q < f.Q) {
      // (a dropped query has area 0: it was never offered)
      const int64_t *c = f.counts + ((int64_t)item * f.Q + q) * 3;
      const int64_t area = c[0], original = c[1], inter = c[2];
      const bool alive = area > 0 && original > 0 && inter > 0 && (double)area / (double)original >= f.threshold;
      if (alive) v = (TOut)(f.ids.p ? f.ids.p[item * f.ids.stride_n + q * f.ids.stride_q] : q);
      if (u == 0) f.survives[(int64_t)item * f.Q + q] = alive;
    }
    lut[q] = v;
  }
  __syncthreads();
  const AABackItem &it = f.items[item];
  const uintptr_t first = (uintptr_t)(f.arena + it.out_off), last = first + (uintptr_t)it.oh * it.ow * sizeof(TOut);
  const unsigned top = (unsigned)f.Q;
#pragma unroll
  for (int k = 0; k < AA_BACK_PANOPTIC_FIN_PIECES; k++) {
    const uintptr_t at = (first & ~(uintptr_t)15) + (((uintptr_t)u * AA_BACK_PANOPTIC_FIN_PIECES + k) * AA_BACK_THREADS + threadIdx.x) * 16;
    if (at >= last) break;
    if (at >= first && at + 16 <= last) {
      Piece<TOut> pc = *(const Piece<TOut> *)at;
#pragma unroll
      for (unsigned e = 0; e < 16 / sizeof(TOut); e++) {
        const unsigned code = (unsigned)pc.v[e];
        pc.v[e] = lut[code < top ? code : top];
      }
      *(Piece<TOut> *)at = pc;
    } else {  // (the ends of a map that does not begin or end on a 16-byte boundary)
      const uintptr_t lo = at > first ? at : first, hi = at + 16 < last ? at + 16 : last;
      for (TOut *e = (TOut *)lo; e < (TOut *)hi; e++) {
        const unsigned code = (unsigned)*e;
        *e = lut[code < top ? code : top];
      }
    }
  }
}

// ---- the launches' choice of kernel --------------------------------------------------------------------------------------------------------
struct PanopticLaunch {
  unsigned units, fin_units;
  hipStream_t stream;
};
template <typename F> inline void with_label_type(int dt, F &&f) {
  if (dt == AA_U8) f(TypeTag<uint8_t>{});
  else if (dt == AA_I16) f(TypeTag<int16_t>{});
  else if (dt == AA_I32) f(TypeTag<int32_t>{});
  else f(TypeTag<int64_t>{});
}
void launch_resample(bool vec, int in_dtype, int out_dtype, const PanopticArgs &a, const PanopticLaunch &l) {
  with_float_type(in_dtype, [&](auto in) {
    with_label_type(out_dtype, [&](auto out) {
      using TIn = tag_t<decltype(in)>;
      using TOut = tag_t<decltype(out)>;
      if (vec) hipLaunchKernelGGL((panoptic_resample<TIn, true, TOut>), dim3(l.units), dim3(AA_BACK_TILE), 0, l.stream, a);
      else hipLaunchKernelGGL((panoptic_resample<TIn, false, TOut>), dim3(l.units), dim3(AA_BACK_TILE), 0, l.stream, a);
    });
  });
}
void launch_finalise(int out_dtype, const FinaliseArgs &f, const PanopticLaunch &l) {
  with_label_type(out_dtype, [&](auto out) {
    hipLaunchKernelGGL((panoptic_finalise<tag_t<decltype(out)>>), dim3(l.fin_units), dim3(AA_BACK_THREADS), 0, l.stream, f);
  });
}

inline bool label_dtype(int dt) { return dt == AA_U8 || dt == AA_I16 || dt == AA_I32 || dt == AA_I64; }
// Whether out_dtype holds v, and the code Q beside the query indices.
inline bool label_holds(int dt, int64_t v) {
  switch (dt) {
    case AA_U8: return v >= 0 && v <= 255;
    case AA_I16: return v >= INT16_MIN && v <= INT16_MAX;
    case AA_I32: return v >= INT32_MIN && v <= INT32_MAX;
    default: return true;
  }
}
inline bool shape_ok(int64_t Q) { return Q <= AA_BACK_PANOPTIC_MAX_Q; }
inline int kept_words(int64_t Q) { return (int)((Q + 1 + 3) & ~(int64_t)3); }

struct PanopticSections {
  const AABackItem *items;
  const int64_t *unit0, *fin0;
};
inline PanopticSections sections(const void *block, int64_t n) {
  const AABackItem *items = (const AABackItem *)((const char *)block + sizeof(AABackPanopticHeader));
  const int64_t *unit0 = (const int64_t *)(items + n);
  return {items, unit0, unit0 + n + 1};
}

// The static LDS of the call's largest workgroup against the limit of the device the launches go to (the stream's; for the null stream
// the current one).
inline int lds_fits(hipStream_t stream) {
  const size_t resample = kWaves * (AA_BACK_CONF_SLOTS * sizeof(unsigned long long) + kMaxQ * sizeof(unsigned));
  const size_t finalise = (kMaxQ + 1) * sizeof(int64_t);
  hipDevice_t dev = 0;
  int limit = 0;
  if (hipStreamGetDevice(stream, &dev) != hipSuccess || hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) {
    (void)hipGetLastError();
    return AA_ERR_HIP;
  }
  return (int64_t)(resample > finalise ? resample : finalise) > (int64_t)limit ? AA_ERR_BAD_SHAPE : AA_OK;
}

}  // namespace

// ---- host: the planner ---------------------------------------------------------------------------------------------------------------------
size_t aa_back_panoptic_desc_size(int64_t n) {
  return n < 0 ? 0 : aa_desc_size(sizeof(AABackPanopticHeader), sizeof(AABackItem), n) + ((size_t)n + 1) * sizeof(int64_t);
}

// aa_back_queries_plan_host's checks in its order with K = Q: Q beyond AA_BACK_PANOPTIC_MAX_Q beside n and K; a map type that cannot hold
// the code Q beside the indices (AA_U8 with Q = 256); the pointers; per item its own checks, then the arena and the work units of both
// launches; last AA_ERR_BAD_DTYPE.
int aa_back_panoptic_plan_host(int filter, int layout, int64_t n, int64_t Q, const aa_back_item *in, int out_dtype, void *desc_host, size_t desc_bytes,
                               size_t *workspace_bytes, size_t *arena_bytes, int64_t *out_offsets, int64_t *counts_offset, int64_t *survives_offset) {
  int rc = plan_prologue(filter, layout, n, Q, AA_BACK_ARGMAX, AA_BACK_ACT_SIGMOID, out_dtype, shape_ok(Q));
  if (rc != AA_OK) return rc;
  if (out_dtype == AA_U8 && Q > 255) return AA_ERR_BAD_SHAPE;
  if (!desc_host || !workspace_bytes || !arena_bytes || !counts_offset || !survives_offset || (n > 0 && (!in || !out_offsets))) return AA_ERR_NULL;
  if (desc_bytes < aa_back_panoptic_desc_size(n)) return AA_ERR_WORKSPACE;
  const size_t eb = elem_bytes(out_dtype);
  AABackPanopticHeader *hd = (AABackPanopticHeader *)desc_host;
  const PanopticSections s = sections(desc_host, n);
  AABackItem *items = (AABackItem *)s.items;
  int64_t *unit0 = (int64_t *)s.unit0, *fin0 = (int64_t *)s.fin0;
  size_t ws = 0, arena = 0;
  int64_t units = 0, fin_units = 0;
  for (int64_t i = 0; i < n; i++) {
    AABackItem it;
    if ((rc = plan_item(filter, layout, Q, in[i], it, ws)) != AA_OK) return rc;
    arena = aa_align16(arena);
    it.out_off = (int64_t)arena;
    const size_t map_bytes = (size_t)it.oh * (size_t)it.ow * eb;
    arena += map_bytes;
    if (arena > (size_t)AA_BACK_MAX_ELEMS * 8) return AA_ERR_BAD_SHAPE;
    unit0[i] = units;
    fin0[i] = fin_units;
    units += (int64_t)((it.oh + kRows - 1) / kRows) * it.xtiles;
    // (a map may begin up to 15 bytes after the 16-byte boundary the finalise counts its pieces from)
    fin_units += (int64_t)((map_bytes + 15 + AA_BACK_PANOPTIC_FIN_BYTES - 1) / AA_BACK_PANOPTIC_FIN_BYTES);
    if (units > INT32_MAX || fin_units > INT32_MAX) return AA_ERR_BAD_SHAPE;  // (one grid each)
    out_offsets[i] = it.out_off;
    items[i] = it;
  }
  unit0[n] = units;
  fin0[n] = fin_units;
  if (!label_dtype(out_dtype)) return AA_ERR_BAD_DTYPE;
  memset(hd, 0, sizeof(*hd));
  hd->magic = AA_BACK_PANOPTIC_MAGIC;
  hd->n = (int32_t)n; hd->Q = (int32_t)Q; hd->filter = filter; hd->layout = layout; hd->out_dtype = out_dtype;
  hd->kept_words = kept_words(Q);
  hd->units = units;
  hd->fin_units = fin_units;
  hd->tables_bytes = (int64_t)ws;
  ws = aa_align16(ws);
  hd->kept_off = (int64_t)ws;
  ws += (size_t)n * hd->kept_words * sizeof(int32_t);
  hd->ws_bytes = (int64_t)ws;
  arena = aa_align16(arena);
  hd->counts_off = (int64_t)arena;
  arena += (size_t)n * (size_t)Q * 3 * sizeof(int64_t);
  arena = aa_align16(arena);
  hd->survives_off = (int64_t)arena;
  arena += (size_t)n * (size_t)Q;
  hd->arena_bytes = (int64_t)arena;
  *workspace_bytes = ws;
  *arena_bytes = arena;
  *counts_offset = hd->counts_off;
  *survives_offset = hd->survives_off;
  return AA_OK;
}

// ---- host: the three launches --------------------------------------------------------------------------------------------------------------
// aa_launch_back_queries' checks in their order, every one before the first launch; the arena on an 8-byte boundary (the counts); after
// the sources the scores and ids — AA_ERR_NULL, AA_ERR_STRIDES for a negative stride or a pointer that is not 4-byte aligned — and
// AA_ERR_BAD_SHAPE for a void the map's type does not hold or a threshold that is NaN; last the LDS of a workgroup against the device's limit.
int aa_launch_back_panoptic(const void *desc_host, const void *desc_dev, int in_dtype, const aa_back_panoptic_io *io, void *arena_dev, size_t arena_bytes,
                            void *workspace_dev, size_t workspace_bytes, hipStream_t stream) {
  const AABackPanopticHeader *hd = (const AABackPanopticHeader *)desc_host;
  if (hd->magic != AA_BACK_PANOPTIC_MAGIC || !aa_filter_valid(hd->filter) || hd->n < 0 || hd->Q < 1 || !shape_ok(hd->Q) ||
      (hd->out_dtype == AA_U8 && hd->Q > 255) || hd->units < 0 || hd->units > INT32_MAX || hd->fin_units < 0 || hd->fin_units > INT32_MAX ||
      (hd->layout != AA_NCHW && hd->layout != AA_NHWC) || hd->kept_words != kept_words(hd->Q) || hd->kept_off < hd->tables_bytes || (hd->kept_off & 15) ||
      hd->ws_bytes < hd->kept_off + (int64_t)hd->n * hd->kept_words * 4 || (hd->counts_off & 15) || (hd->survives_off & 15) ||
      hd->survives_off < hd->counts_off + (int64_t)hd->n * hd->Q * 24 || hd->arena_bytes < hd->survives_off + (int64_t)hd->n * hd->Q)
    return AA_ERR_BAD_SHAPE;
  if (!float_dtype(in_dtype) || !label_dtype(hd->out_dtype)) return AA_ERR_BAD_DTYPE;
  const int rc = aa_many_check_launch(hd->n, desc_dev, arena_dev, workspace_dev, workspace_bytes, hd->ws_bytes, sizeof(int64_t));
  if (rc != AA_OK || hd->n == 0) return rc;
  if (arena_bytes < (size_t)hd->arena_bytes) return AA_ERR_WORKSPACE;
  const PanopticSections host = sections(desc_host, hd->n);
  bool vec;
  const int rs = check_sources(host.items, hd->n, in_dtype, hd->layout, hd->Q, &vec);
  if (rs != AA_OK) return rs;
  if (!io || !io->scores_dev) return AA_ERR_NULL;
  if (io->scores_stride_n < 0 || io->scores_stride_q < 0 || (uintptr_t)io->scores_dev % sizeof(float) ||
      (io->ids_dev && (io->ids_stride_n < 0 || io->ids_stride_q < 0 || (uintptr_t)io->ids_dev % sizeof(int32_t))))
    return AA_ERR_STRIDES;
  if (!label_holds(hd->out_dtype, io->void_value) || io->overlap_threshold != io->overlap_threshold) return AA_ERR_BAD_SHAPE;
  const int rl = lds_fits(stream);
  if (rl != AA_OK) return rl;
  const PanopticSections dev = sections(desc_dev, hd->n);
  const PerQuery<float> scores = {(const float *)io->scores_dev, io->scores_stride_n, io->scores_stride_q};
  const KeptLists kept = {hd->kept_off, hd->kept_words, vec ? 1 : 0};
  int64_t *counts = (int64_t *)((char *)arena_dev + hd->counts_off);
  const int64_t count_elems = (int64_t)hd->n * hd->Q * 3;
  hipLaunchKernelGGL(panoptic_tables, dim3(3u * (unsigned)hd->n + zero_blocks(count_elems)), dim3(AA_BACK_THREADS), 0, stream, dev.items, (int)hd->n,
                     (int)hd->Q, (char *)workspace_dev, (int)hd->filter, scores, kept, counts, count_elems);
  AA_HIP_CHECK_LAUNCH();
  PanopticArgs a;
  a.items = dev.items; a.unit0 = dev.unit0; a.ws = (const char *)workspace_dev; a.arena = (char *)arena_dev;
  a.scores = scores; a.kept = kept; a.counts = counts;
  a.n = hd->n; a.Q = hd->Q;
  const PanopticLaunch l = {(unsigned)hd->units, (unsigned)hd->fin_units, stream};
  launch_resample(vec, in_dtype, hd->out_dtype, a, l);
  AA_HIP_CHECK_LAUNCH();
  FinaliseArgs f;
  f.items = dev.items; f.fin0 = dev.fin0; f.arena = (char *)arena_dev; f.counts = counts;
  f.survives = (uint8_t *)arena_dev + hd->survives_off;
  f.ids = {(const int32_t *)io->ids_dev, io->ids_dev ? io->ids_stride_n : 0, io->ids_dev ? io->ids_stride_q : 0};
  f.void_value = io->void_value;
  f.threshold = io->overlap_threshold;
  f.n = hd->n; f.Q = hd->Q;
  launch_finalise(hd->out_dtype, f, l);
  AA_HIP_CHECK_LAUNCH();
  return AA_OK;
}
