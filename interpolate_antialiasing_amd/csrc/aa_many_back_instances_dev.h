// aa_many_back_instances_dev.h — what the instance calls of the ragged return path compile alike (aa_many_back_instances.hip: masks as
// bytes or bits per slot; aa_many_back_instances_rle.hip: run lengths per slot): the table kernel with its sort of an item's slots by
// query, the work lists' accessors, a wave's record of a query, and the resample kernel, whose ballot word of (distinct query, row, wave)
// goes to one of three sinks.  Each file that includes this compiles its own copies (an unnamed namespace).
#pragma once

#include "aa_many_back_instances.h"
#include "aa_many_back_shared.h"

namespace {

constexpr int kRows = AA_BACK_INSTANCES_ROWS, kMaxQ = AA_BACK_INSTANCES_MAX_Q, kMaxM = AA_BACK_INSTANCES_MAX_M, kWaves = AA_BACK_TILE / 64;
constexpr int kStats = AA_BACK_INSTANCES_STATS;
constexpr unsigned kEmptyKey = 0xFFFF;  // the key of an empty slot: after every query
static_assert(kMaxM <= AA_BACK_THREADS && kMaxQ <= AA_BACK_THREADS && kMaxQ == 256, "a lane per slot and per query; the asked set is four 64-bit words");

// Where a ballot word goes: a byte per lane into every asking slot's mask; byte j of the word by lane j < 8 into every asking slot's
// packed mask; or ONE 8-byte store into the distinct query's bit plane of the workspace (aa_many_back_instances_rle.h).
constexpr int kSinkBytes = 0, kSinkBits = 1, kSinkPlanes = 2;

// The queries of the call: element (i, m) at p + (i * stride_n + m * stride_m) ELEMENTS of `elem` bytes (4: int32, 8: int64).
struct Queries {
  const void *p;
  int64_t stride_n, stride_m;
  int elem;
};
__device__ inline int64_t query_at(const Queries &queries, int64_t item, int64_t slot) {
  const int64_t at = item * queries.stride_n + slot * queries.stride_m;
  return queries.elem == 8 ? ((const int64_t *)queries.p)[at] : (int64_t)((const int32_t *)queries.p)[at];
}

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

// The bit plane of a distinct asked query among an item's min(Q, M) planes: the query itself where there are no more queries than
// slots, else the place of its first slot among the sorted slots (both are below min(Q, M), and no two distinct queries share one).
__device__ inline int plane_of(const WorkLists &w, int q, int first) { return w.Q <= w.M ? q : first; }

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
  char *arena;  // the items' masks at their out_off; for kSinkPlanes the planes' part of the workspace, an item's planes at its out_off
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

template <typename TIn, bool VEC, int SINK>
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
  // bytes of a mask's row; of a plane's row, whole words
  const int64_t pitch = SINK == kSinkPlanes ? (((int64_t)it.ow + 63) >> 6) * 8 : SINK == kSinkBits ? ((int64_t)it.ow + 7) >> 3 : (int64_t)it.ow;
  uint8_t *out = (uint8_t *)(a.arena + it.out_off);

  for (int y = t.y0; y < t.y1; y++) {
    const Row ry = table_row(a.ws + it.tab_h, it.h, it.oh, it.ksize_h, y);
    const TIn *p = (const TIn *)it.src + ry.x0 * prow + rx.x0 * ppx;
    // `word` (bit l: lane l's pixel) into row y of the masks of slots[first .. first + len)   (all uniform)
    auto store = [&](unsigned long long word, int first, int len) {
      for (int s = first; s < first + len; s++) {
        const int slot = __builtin_amdgcn_readfirstlane(slots[s]);
        uint8_t *row = out + ((int64_t)slot * it.oh + y) * pitch;
        if constexpr (SINK == kSinkBits) {
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
      if constexpr (SINK == kSinkPlanes) {
        // the wave's word of row y of the query's plane, zero or not (the encode reads the plane in full): one aligned 8-byte store
        const int64_t plane = plane_of(a.lists, q, (int)(range & 0xFFFF));
        if (lane == 0) *(unsigned long long *)(out + (plane * it.oh + y) * pitch + (xw >> 6) * 8) = word;
      } else {
        store(word, (int)(range & 0xFFFF), (int)(range >> 16));
      }
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
    if constexpr (SINK != kSinkPlanes) store(0ull, valid, M - valid);  // the empty slots
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

template <typename TIn, int SINK> void launch_resample_sink(bool vec, const InstancesArgs &a, unsigned units, hipStream_t stream) {
  const dim3 grid(units), block(AA_BACK_TILE);
  if (vec) hipLaunchKernelGGL((instances_resample<TIn, true, SINK>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((instances_resample<TIn, false, SINK>), grid, block, 0, stream, a);
}

inline bool shape_ok(int64_t Q, int64_t M, int bits) { return Q <= kMaxQ && M >= 1 && M <= kMaxM && (bits == 0 || bits == 1); }
inline int list_words(int64_t Q, int64_t M) { return (int)((2 + 2 * Q + M + 3) & ~(int64_t)3); }

// The static LDS of the table and resample kernels against the limit of the device the launches go to (the stream's; for the null
// stream the current one), with `more` bytes of dynamic LDS of another kernel of the call.
inline int lds_fits(hipStream_t stream, size_t more = 0) {
  const size_t resample = kWaves * kMaxQ * sizeof(Record), tables = kMaxM * sizeof(unsigned short);
  hipDevice_t dev = 0;
  int limit = 0;
  if (hipStreamGetDevice(stream, &dev) != hipSuccess || hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) {
    (void)hipGetLastError();
    return AA_ERR_HIP;
  }
  const size_t most = resample > tables ? resample : tables;
  return (int64_t)(most > more ? most : more) > (int64_t)limit ? AA_ERR_BAD_SHAPE : AA_OK;
}

}  // namespace
