// aa_many_back_instances.hip — instance inference of mask-classification heads (MaskFormer, Mask2Former, OneFormer) in the ragged return
// path: item i is Q mask logits [Q, h_i, w_i] and M slots, slot m asking for query queries[i, m] (an entry outside 0 .. Q - 1: an empty
// slot; entries may repeat, as they do after a top-k over Q x C).  With R_i the fp32 resample of aa_many_back.hip (K = Q, bit for bit),
//   mask[m]  = R_i[q] > 0                          a NaN is false; an empty slot's mask is all zeros
//   stats[m] = (area, psum, x0, y0, x1, y1)        area: the mask's pixels; psum: the sum over them of aa_sigmoid(R_i[q]) * 2^24, every
//                                                  term an exact integer (a sigmoid of a positive value lies in [0.5, 1], where float32
//                                                  steps by 2^-24 or more); the tight half-open box, (ow, oh, 0, 0) for an empty mask
// Nothing here has a tolerance.  No matrix instruction fits: the work is a threshold and counting, not a product.  Two launches
// whatever n, M and the sizes:
//   1. instances_tables    workgroups 0 .. 2 n - 1 build the items' tables as back_tables does (table_axis_build); workgroups 2 n ..
//                          3 n - 1 turn one item's queries[i, :] into its work list (aa_many_back_instances.h) — lane t holds slot t's
//                          key in LDS, and behind the only barrier of the call every lane walks the M keys once: as slot t it counts the
//                          slots sorted before it (by query, then slot, the empty ones last), as query t its slots and those before
//                          them, and the asked queries meet in a 256-bit set that the walk keeps in scalar registers, from which an
//                          entry's place among the distinct queries (or chunks) is a popcount; the workgroups after them set every
//                          slot's stats to (0, 0, ow, oh, 0, 0), the identities of the sums, the minima and the maxima.
//   2. instances_resample  one workgroup per work unit, AA_BACK_INSTANCES_ROWS output rows times AA_BACK_TILE columns, a lane per column
//                          walking down the rows (the panoptic kernel's shape, its clamped columns and its waves that leave).  Per row
//                          the wave walks the item's entries — uniform loads, a query nobody asked for is never loaded — four distinct
//                          queries a step (class_sums_at) or one aligned chunk with a mask of its asked members.  Per distinct query ONE
//                          ballot of logit > 0: that word is the output.  Where it is 0 — the common case, instance masks are sparse —
//                          sigmoid and counting are skipped; else the lanes' uint32(p * 2^24) are summed across the wave with DPP
//                          (<= 2^30), and lane 0 updates the wave's record of the query in LDS: area, a 64-bit psum, the first and last
//                          column from ctz / clz of the word, the first and last row.  Then the word is stored for EVERY slot of the
//                          query's range: computed once, stored count-of-duplicates times, a byte per lane or, packed, byte j of the
//                          word by lane j < 8 (a wave's first column is a multiple of 64, so its bytes begin at x / 8; byte stores, the
//                          row pitch ceil(ow / 8) is no multiple of 8).  The empty slots get zeros every row, so the whole output is
//                          written.  After the last row the lanes take a query each and hand its record to every slot of its range:
//                          64-bit integer atomic adds of area and psum, 64-bit atomic min / max of the box.  A wave's LDS is its own:
//                          no barrier.
// Integer adds, minima and maxima commute, so masks and stats are the same bits on every run.  Every element offset is 64-bit.  Plain
// C++ and vector memory operations only.  Shared with the other files of the return path: aa_many_back_shared.h.

#include <string.h>

#include "aa_many_back_instances.h"
#include "aa_many_back_shared.h"

namespace {

constexpr int kRows = AA_BACK_INSTANCES_ROWS, kMaxQ = AA_BACK_INSTANCES_MAX_Q, kMaxM = AA_BACK_INSTANCES_MAX_M, kWaves = AA_BACK_TILE / 64;
constexpr int kStats = AA_BACK_INSTANCES_STATS;
constexpr unsigned kEmptyKey = 0xFFFF;  // the key of an empty slot: after every query
static_assert(kMaxM <= AA_BACK_THREADS && kMaxQ <= AA_BACK_THREADS && kMaxQ == 256, "a lane per slot and per query; the asked set is four 64-bit words");

// The queries of the call: element (i, m) at p + (i * stride_n + m * stride_m) ELEMENTS of `elem` bytes (4: int32, 8: int64).
struct Queries {
  const void *p;
  int64_t stride_n, stride_m;
  int elem;
};

struct WorkLists {
  int64_t off;  // of the workspace
  int words;    // int32 words of an item's list (aa_many_back_instances.h)
  int chunks;   // entries are q0 | mask << 16 (items that take the vector loads) rather than q
  int Q, M;
};
__device__ inline int32_t *work_list(char *ws, const WorkLists &w, int item) { return (int32_t *)(ws + w.off) + (int64_t)item * w.words; }
__device__ inline const int32_t *list_ranges(const int32_t *list) { return list + 2; }
__device__ inline const int32_t *list_entries(const int32_t *list, const WorkLists &w) { return list + 2 + w.Q; }
__device__ inline const int32_t *list_slots(const int32_t *list, const WorkLists &w) { return list + 2 + 2 * w.Q; }

// The set bits of a[0 .. 3] below bit `pos` (pos >= 256: all of them).
__device__ inline int bits_below(const unsigned long long (&a)[4], int pos) {
  int r = 0;
#pragma unroll
  for (int w = 0; w < 4; w++) {
    const unsigned long long part = w < (pos >> 6) ? ~0ull : w == (pos >> 6) ? (1ull << (pos & 63)) - 1 : 0ull;
    r += __popcll(a[w] & part);
  }
  return r;
}

// The workgroups of the table launch that set the stats: workgroup b of `blocks`, AA_BACK_CONF_ZERO elements at a time (zero_counts' stride).
__device__ inline void init_stats(int64_t *stats, const AABackItem *items, int M, int64_t elems, int64_t b, int64_t blocks) {
  const int64_t step = blocks * AA_BACK_CONF_ZERO;
  for (int64_t base = b * AA_BACK_CONF_ZERO; base < elems; base += step) {
    const int64_t end = base + AA_BACK_CONF_ZERO < elems ? base + AA_BACK_CONF_ZERO : elems;
    for (int64_t e = base + threadIdx.x; e < end; e += AA_BACK_THREADS) {
      const int j = (int)(e % kStats);
      const AABackItem &it = items[e / ((int64_t)kStats * M)];
      stats[e] = j == 2 ? it.ow : j == 3 ? it.oh : 0;
    }
  }
}

// ---- 1. tables, work lists, and the stats set ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(AA_BACK_THREADS) instances_tables(const AABackItem *items, int n, char *ws, int filter, Queries queries, WorkLists wl,
                                                                    int64_t *stats, int64_t stat_elems) {
  __shared__ unsigned short keys[kMaxM];
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
    init_stats(stats, items, wl.M, stat_elems, b - n, (int64_t)gridDim.x - 3 * (int64_t)n);
    return;
  }
  // item b's work list.  Slot t's key: its query, or kEmptyKey.
  const int t = (int)threadIdx.x, Q = wl.Q, M = wl.M;
  unsigned key = kEmptyKey;
  if (t < M) {
    const int64_t at = b * queries.stride_n + (int64_t)t * queries.stride_m;
    const int64_t v = queries.elem == 8 ? ((const int64_t *)queries.p)[at] : (int64_t)((const int32_t *)queries.p)[at];
    key = v >= 0 && v < Q ? (unsigned)v : kEmptyKey;
    keys[t] = (unsigned short)key;
  }
  __syncthreads();
  int before = 0;            // as slot t: the slots sorted before it
  int first = 0, count = 0;  // as query t: the slots of lower queries, and its own
  int valid = 0;             // the slots that ask for a query
  unsigned long long asked[4] = {0, 0, 0, 0};  // the set of asked queries (uniform)
  for (int u = 0; u < M; u++) {
    const unsigned k = keys[u];  // (one address for the workgroup: a broadcast)
    before += (int)((k < key) | ((k == key) & (u < t)));
    first += (int)(k < (unsigned)t);
    count += (int)(k == (unsigned)t);
    valid += (int)(k != kEmptyKey);
    const unsigned ku = (unsigned)__builtin_amdgcn_readfirstlane((int)k);
#pragma unroll
    for (int w = 0; w < 4; w++) asked[w] |= (ku >> 6) == (unsigned)w ? 1ull << (ku & 63) : 0ull;
  }
  int32_t *list = work_list(ws, wl, (int)b);
  if (t < M) list[2 + 2 * Q + before] = t;
  if (t < Q) list[2 + t] = first | count << 16;
  // the entries: lane t holds query t, or the chunk of AA_BACK_UNROLL queries from 4 t (Q is a multiple of AA_BACK_UNROLL there:
  // check_sources); `marks` has a bit per entry at the entry's first query
  unsigned long long marks[4];
#pragma unroll
  for (int w = 0; w < 4; w++) {
    const unsigned long long a = asked[w];
    marks[w] = wl.chunks ? (a | a >> 1 | a >> 2 | a >> 3) & 0x1111111111111111ull : a;
  }
  const int pos = wl.chunks ? t * AA_BACK_UNROLL : t;
  if (pos < Q) {
    unsigned long long word = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) word = (pos >> 6) == w ? asked[w] : word;
    const unsigned members = (unsigned)(word >> (pos & 63)) & (wl.chunks ? (1u << AA_BACK_UNROLL) - 1 : 1u);
    if (members != 0) list[2 + Q + bits_below(marks, pos)] = wl.chunks ? (int32_t)((unsigned)pos | members << 16) : pos;
  }
  if (t == 0) {
    list[0] = bits_below(marks, 4 * 64);
    list[1] = valid;
  }
}

// ---- 2. resample, masks, stats -----------------------------------------------------------------------------------------------------------------
struct InstancesArgs {
  const AABackItem *items;
  const int64_t *unit0;
  const char *ws;
  char *arena;
  WorkLists lists;
  int64_t *stats;
  int n;
};

// A wave's record of one query over the rows of its tile, in LDS.  Lane 0 writes it between the rows and lane q reads it back after the
// last: relaxed atomics of wavefront scope with a fence of that scope where lanes meet, as WaveCounts has them.  area 0: nothing
// counted, and nothing else of the record means anything.  box: first column | last column << 8 (of the wave's 64) | first row << 16 |
// last row << 24 (of the tile's).
struct alignas(16) Record {
  unsigned long long psum;
  unsigned area, box;

  template <typename T> __device__ static T get(const T *s) { return __hip_atomic_load(s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
  template <typename T> __device__ static void set(T *s, T v) { __hip_atomic_store(s, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }

  __device__ void clear() { set(&area, 0u); }
  // One row's word (not 0) with the sum of its lanes' terms: rows come in ascending order.
  __device__ void add(unsigned long long word, unsigned sum, unsigned row) {
    const unsigned had = get(&area);
    const unsigned lo = (unsigned)__builtin_ctzll(word), hi = 63u - (unsigned)__builtin_clzll(word);
    unsigned x0 = lo, x1 = hi, y0 = row;
    unsigned long long total = sum;
    if (had != 0) {
      const unsigned b = get(&box);
      x0 = min(lo, b & 0xFF);
      x1 = max(hi, b >> 8 & 0xFF);
      y0 = b >> 16 & 0xFF;
      total += get(&psum);
    }
    set(&psum, total);
    set(&box, x0 | x1 << 8 | y0 << 16 | row << 24);
    set(&area, had + (unsigned)__popcll(word));
  }
};

// The sum of v over the 64 lanes of the wave, all of them active: within quads, halves of eight and rows of sixteen by DPP, then the
// four rows through scalar registers.  (uniform)
__device__ inline unsigned wave_sum(unsigned v) {
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);   // quad_perm [1, 0, 3, 2]
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);   // quad_perm [2, 3, 0, 1]
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true);  // row_half_mirror
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, true);  // row_mirror
  return (unsigned)__builtin_amdgcn_readlane((int)v, 0) + (unsigned)__builtin_amdgcn_readlane((int)v, 16) +
         (unsigned)__builtin_amdgcn_readlane((int)v, 32) + (unsigned)__builtin_amdgcn_readlane((int)v, 48);
}

template <typename TIn, bool VEC, bool BITS>
__global__ void __launch_bounds__(AA_BACK_TILE) instances_resample(InstancesArgs a) {
  __shared__ Record records[kWaves * kMaxQ];
  const int64_t unit = blockIdx.x;
  const int item = aa_unit_item(a.unit0, a.n, unit);
  const AABackItem &it = a.items[item];
  RowTile t;
  if (!row_tile<kRows>(unit - a.unit0[item], it.xtiles, it.oh, it.ow, t)) return;  // (no barrier below)
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const int Q = a.lists.Q, M = a.lists.M;
  Record *rec = records + wave * kMaxQ;
  for (int q = lane; q < Q; q += 64) rec[q].clear();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (the lanes meet)

  const bool in = t.x < it.ow;
  const int xc = in ? t.x : it.ow - 1;  // (clamped: the wave's control flow stays uniform and every address lies inside the item)
  const int xr = (it.flags & AA_MANY_FLIP_X) ? it.ow - 1 - xc : xc;
  const int xw = t.x - lane;  // the wave's first column, a multiple of 64
  const Row rx = table_row(a.ws + it.tab_w, it.w, it.ow, it.ksize_w, xr);
  const int64_t sch = it.stride_ch, prow = it.stride_row, ppx = it.stride_px;
  const int32_t *list = work_list((char *)a.ws, a.lists, item);
  const int32_t *ranges = list_ranges(list), *entries = list_entries(list, a.lists), *slots = list_slots(list, a.lists);
  const int count = __builtin_amdgcn_readfirstlane(list[0]);  // (the list is the item's: uniform, and said so to the compiler)
  const int valid = __builtin_amdgcn_readfirstlane(list[1]);
  const int64_t pitch = BITS ? ((int64_t)it.ow + 7) >> 3 : (int64_t)it.ow;  // bytes of a mask's row
  uint8_t *out = (uint8_t *)(a.arena + it.out_off);

  for (int y = t.y0; y < t.y1; y++) {
    const Row ry = table_row(a.ws + it.tab_h, it.h, it.oh, it.ksize_h, y);
    const TIn *p = (const TIn *)it.src + ry.x0 * prow + rx.x0 * ppx;
    // `word` (bit l: lane l's pixel) into row y of the masks of slots[first .. first + len)   (all uniform)
    auto store = [&](unsigned long long word, int first, int len) {
      for (int s = first; s < first + len; s++) {
        const int slot = __builtin_amdgcn_readfirstlane(slots[s]);
        uint8_t *row = out + ((int64_t)slot * it.oh + y) * pitch;
        if constexpr (BITS) {
          if (lane < 8 && xw + 8 * lane < it.ow) row[(xw >> 3) + lane] = (uint8_t)(word >> (8 * lane));
        } else {
          if (in) row[t.x] = (uint8_t)(word >> lane & 1);
        }
      }
    };
    // asked query q (uniform over the wave) with the lane's resampled logit
    auto take = [&](int q, float logit) {
      const bool on = in && logit > 0.0f;
      const unsigned long long word = __ballot(on);
      if (word != 0) {  // (uniform)
        const float pq = aa_sigmoid(logit);
        const unsigned sum = wave_sum(on ? (unsigned)(pq * 16777216.0f) : 0u);
        if (lane == 0) rec[q].add(word, sum, (unsigned)(y - t.y0));
      }
      const unsigned range = (unsigned)__builtin_amdgcn_readfirstlane(ranges[q]);
      store(word, (int)(range & 0xFFFF), (int)(range >> 16));
    };
    if constexpr (VEC) {
      for (int e = 0; e < count; e++) {
        const unsigned entry = (unsigned)__builtin_amdgcn_readfirstlane(entries[e]);
        const int q0 = (int)(entry & 0xFFFF);
        float acc[AA_BACK_UNROLL];
        class_sums<TIn, AA_BACK_UNROLL, true>(p + q0 * sch, sch, prow, ppx, ry, rx, acc);
#pragma unroll
        for (int c = 0; c < AA_BACK_UNROLL; c++)
          if (entry >> (16 + c) & 1) take(q0 + c, acc[c]);  // (uniform)
      }
    } else {
      constexpr int U = AA_BACK_UNROLL;
      int e = 0;
      for (; e + U <= count; e += U) {
        int q[U];
        int64_t off[U];
        float acc[U];
#pragma unroll
        for (int c = 0; c < U; c++) {
          q[c] = __builtin_amdgcn_readfirstlane(entries[e + c]);
          off[c] = q[c] * sch;
        }
        class_sums_at<TIn, U>(p, off, prow, ppx, ry, rx, acc);
#pragma unroll
        for (int c = 0; c < U; c++) take(q[c], acc[c]);
      }
      for (; e < count; e++) {
        const int q = __builtin_amdgcn_readfirstlane(entries[e]);
        float acc[1];
        class_sums<TIn, 1, false>(p + q * sch, sch, prow, ppx, ry, rx, acc);
        take(q, acc[0]);
      }
    }
    store(0ull, valid, M - valid);  // the empty slots
  }

  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (the lanes meet)
  for (int q = lane; q < Q; q += 64) {
    const unsigned area = Record::get(&rec[q].area);
    if (area == 0) continue;
    const unsigned long long psum = Record::get(&rec[q].psum);
    const unsigned box = Record::get(&rec[q].box);
    const unsigned long long x0 = (unsigned)xw + (box & 0xFF), x1 = (unsigned)xw + (box >> 8 & 0xFF) + 1;
    const unsigned long long y0 = (unsigned)t.y0 + (box >> 16 & 0xFF), y1 = (unsigned)t.y0 + (box >> 24) + 1;
    const unsigned range = (unsigned)ranges[q];
    for (unsigned s = range & 0xFFFF; s < (range & 0xFFFF) + (range >> 16); s++) {
      unsigned long long *st = (unsigned long long *)a.stats + ((int64_t)item * M + slots[s]) * kStats;  // (every value is non-negative)
      atomicAdd(st, (unsigned long long)area);
      atomicAdd(st + 1, psum);
      atomicMin(st + 2, x0);
      atomicMin(st + 3, y0);
      atomicMax(st + 4, x1);
      atomicMax(st + 5, y1);
    }
  }
}

// ---- the launch's choice of kernel ---------------------------------------------------------------------------------------------------------------
template <typename TIn> void launch_resample_of(bool vec, bool bits, const InstancesArgs &a, unsigned units, hipStream_t stream) {
  const dim3 grid(units), block(AA_BACK_TILE);
  if (vec && bits) hipLaunchKernelGGL((instances_resample<TIn, true, true>), grid, block, 0, stream, a);
  else if (vec) hipLaunchKernelGGL((instances_resample<TIn, true, false>), grid, block, 0, stream, a);
  else if (bits) hipLaunchKernelGGL((instances_resample<TIn, false, true>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((instances_resample<TIn, false, false>), grid, block, 0, stream, a);
}
void launch_resample(bool vec, int in_dtype, bool bits, const InstancesArgs &a, unsigned units, hipStream_t stream) {
  with_float_type(in_dtype, [&](auto in) { launch_resample_of<tag_t<decltype(in)>>(vec, bits, a, units, stream); });
}

inline bool shape_ok(int64_t Q, int64_t M, int bits) { return Q <= kMaxQ && M >= 1 && M <= kMaxM && (bits == 0 || bits == 1); }
inline int list_words(int64_t Q, int64_t M) { return (int)((2 + 2 * Q + M + 3) & ~(int64_t)3); }

// The static LDS of the call's largest workgroup against the limit of the device the launches go to (the stream's; for the null stream
// the current one).
inline int lds_fits(hipStream_t stream) {
  const size_t resample = kWaves * kMaxQ * sizeof(Record), tables = kMaxM * sizeof(unsigned short);
  hipDevice_t dev = 0;
  int limit = 0;
  if (hipStreamGetDevice(stream, &dev) != hipSuccess || hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) {
    (void)hipGetLastError();
    return AA_ERR_HIP;
  }
  return (int64_t)(resample > tables ? resample : tables) > (int64_t)limit ? AA_ERR_BAD_SHAPE : AA_OK;
}

}  // namespace

// ---- host: the planner ---------------------------------------------------------------------------------------------------------------------
size_t aa_back_instances_desc_size(int64_t n) { return n < 0 ? 0 : aa_desc_size(sizeof(AABackInstancesHeader), sizeof(AABackItem), n); }

// aa_back_panoptic_plan_host's checks in its order with K = Q: Q beyond AA_BACK_INSTANCES_MAX_Q, M outside 1 .. AA_BACK_INSTANCES_MAX_M
// or a `bits` that is neither 0 nor 1 beside n and K; the pointers; per item its own checks, then M * oh * ow against AA_BACK_MAX_ELEMS,
// the arena and the work units.
int aa_back_instances_plan_host(int filter, int layout, int64_t n, int64_t Q, int64_t M, const aa_back_item *in, int bits, void *desc_host,
                                size_t desc_bytes, size_t *workspace_bytes, size_t *arena_bytes, int64_t *out_offsets, int64_t *stats_offset) {
  int rc = plan_prologue(filter, layout, n, Q, AA_BACK_GREATER, AA_BACK_ACT_NONE, AA_U8, shape_ok(Q, M, bits));
  if (rc != AA_OK) return rc;
  if (!desc_host || !workspace_bytes || !arena_bytes || !stats_offset || (n > 0 && (!in || !out_offsets))) return AA_ERR_NULL;
  if (desc_bytes < aa_back_instances_desc_size(n)) return AA_ERR_WORKSPACE;
  AABackInstancesHeader *hd = (AABackInstancesHeader *)desc_host;
  const AADescView<AABackItem> v = aa_desc_view<AABackInstancesHeader, AABackItem>(desc_host, n);
  AABackItem *items = (AABackItem *)v.items;
  int64_t *unit0 = (int64_t *)v.prefix;
  size_t ws = 0, arena = 0;
  int64_t units = 0;
  for (int64_t i = 0; i < n; i++) {
    AABackItem it;
    if ((rc = plan_item(filter, layout, Q, in[i], it, ws)) != AA_OK) return rc;
    if ((int64_t)it.oh * it.ow > AA_BACK_MAX_ELEMS / M) return AA_ERR_BAD_SHAPE;
    arena = aa_align16(arena);
    it.out_off = (int64_t)arena;
    arena += (size_t)M * (size_t)it.oh * (bits ? ((size_t)it.ow + 7) >> 3 : (size_t)it.ow);
    if (arena > (size_t)AA_BACK_MAX_ELEMS * 8) return AA_ERR_BAD_SHAPE;
    unit0[i] = units;
    units += (int64_t)((it.oh + kRows - 1) / kRows) * it.xtiles;
    if (units > INT32_MAX) return AA_ERR_BAD_SHAPE;  // (one grid)
    out_offsets[i] = it.out_off;
    items[i] = it;
  }
  unit0[n] = units;
  memset(hd, 0, sizeof(*hd));
  hd->magic = AA_BACK_INSTANCES_MAGIC;
  hd->n = (int32_t)n; hd->Q = (int32_t)Q; hd->M = (int32_t)M; hd->filter = filter; hd->layout = layout; hd->bits = bits;
  hd->list_words = list_words(Q, M);
  hd->units = units;
  hd->tables_bytes = (int64_t)ws;
  ws = aa_align16(ws);
  hd->lists_off = (int64_t)ws;
  ws += (size_t)n * hd->list_words * sizeof(int32_t);
  hd->ws_bytes = (int64_t)ws;
  arena = aa_align16(arena);
  hd->stats_off = (int64_t)arena;
  arena += (size_t)n * (size_t)M * kStats * sizeof(int64_t);
  hd->arena_bytes = (int64_t)arena;
  *workspace_bytes = ws;
  *arena_bytes = arena;
  *stats_offset = hd->stats_off;
  return AA_OK;
}

// ---- host: the two launches ------------------------------------------------------------------------------------------------------------------
// aa_launch_back_panoptic's checks in their order, every one before the first launch; the arena on an 8-byte boundary (the stats); after
// the sources the queries — AA_ERR_NULL, AA_ERR_BAD_DTYPE for an element that is neither 4 nor 8 bytes, AA_ERR_STRIDES for a negative
// stride or a pointer that is not aligned to its element; last the LDS of a workgroup against the device's limit.
int aa_launch_back_instances(const void *desc_host, const void *desc_dev, int in_dtype, const aa_back_instances_io *io, void *arena_dev, size_t arena_bytes,
                             void *workspace_dev, size_t workspace_bytes, hipStream_t stream) {
  const AABackInstancesHeader *hd = (const AABackInstancesHeader *)desc_host;
  if (hd->magic != AA_BACK_INSTANCES_MAGIC || !aa_filter_valid(hd->filter) || hd->n < 0 || hd->Q < 1 || !shape_ok(hd->Q, hd->M, hd->bits) || hd->units < 0 ||
      hd->units > INT32_MAX || (hd->layout != AA_NCHW && hd->layout != AA_NHWC) || hd->list_words != list_words(hd->Q, hd->M) ||
      hd->lists_off < hd->tables_bytes || (hd->lists_off & 15) || hd->ws_bytes < hd->lists_off + (int64_t)hd->n * hd->list_words * 4 || (hd->stats_off & 15) ||
      hd->stats_off < 0 || hd->arena_bytes < hd->stats_off + (int64_t)hd->n * hd->M * kStats * 8)
    return AA_ERR_BAD_SHAPE;
  if (!float_dtype(in_dtype)) return AA_ERR_BAD_DTYPE;
  const int rc = aa_many_check_launch(hd->n, desc_dev, arena_dev, workspace_dev, workspace_bytes, hd->ws_bytes, sizeof(int64_t));
  if (rc != AA_OK || hd->n == 0) return rc;
  if (arena_bytes < (size_t)hd->arena_bytes) return AA_ERR_WORKSPACE;
  const AADescView<AABackItem> host = aa_desc_view<AABackInstancesHeader, AABackItem>(desc_host, hd->n);
  bool vec;
  const int rs = check_sources(host.items, hd->n, in_dtype, hd->layout, hd->Q, &vec);
  if (rs != AA_OK) return rs;
  if (!io || !io->queries_dev) return AA_ERR_NULL;
  if (io->queries_elem_bytes != 4 && io->queries_elem_bytes != 8) return AA_ERR_BAD_DTYPE;
  if (io->queries_stride_n < 0 || io->queries_stride_m < 0 || (uintptr_t)io->queries_dev % (uintptr_t)io->queries_elem_bytes) return AA_ERR_STRIDES;
  const int rl = lds_fits(stream);
  if (rl != AA_OK) return rl;
  const AADescView<AABackItem> dev = aa_desc_view<AABackInstancesHeader, AABackItem>(desc_dev, hd->n);
  const Queries queries = {io->queries_dev, io->queries_stride_n, io->queries_stride_m, io->queries_elem_bytes};
  const WorkLists lists = {hd->lists_off, hd->list_words, vec ? 1 : 0, hd->Q, hd->M};
  int64_t *stats = (int64_t *)((char *)arena_dev + hd->stats_off);
  const int64_t stat_elems = (int64_t)hd->n * hd->M * kStats;
  hipLaunchKernelGGL(instances_tables, dim3(3u * (unsigned)hd->n + zero_blocks(stat_elems)), dim3(AA_BACK_THREADS), 0, stream, dev.items, (int)hd->n,
                     (char *)workspace_dev, (int)hd->filter, queries, lists, stats, stat_elems);
  AA_HIP_CHECK_LAUNCH();
  InstancesArgs a;
  a.items = dev.items; a.unit0 = dev.prefix; a.ws = (const char *)workspace_dev; a.arena = (char *)arena_dev;
  a.lists = lists; a.stats = stats; a.n = hd->n;
  launch_resample(vec, in_dtype, hd->bits != 0, a, (unsigned)hd->units, stream);
  AA_HIP_CHECK_LAUNCH();
  return AA_OK;
}
