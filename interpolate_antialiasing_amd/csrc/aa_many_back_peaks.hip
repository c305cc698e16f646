// aa_many_back_peaks.hip — the ragged return path reduced over SPACE: item i is K heatmaps [K, h_i, w_i] (keypoint and landmark heads),
// resampled to [oh_i, ow_i] with aa_many_back.hip's arithmetic (R_i, bit for bit; a flipped item un-mirrored), and per channel
//   peaks[i, k]  = (x, y) of numpy.argmax(R_i[k].ravel()): the lowest flat index y * ow_i + x of the greatest value, a NaN greater
//                  than every number and the first NaN kept, -0.0 and +0.0 equal
//   values[i, k] = R_i[k] at the peak and at its left, right, upper and lower neighbour; one outside the image is the peak's own value
// The K * oh_i * ow_i resampled values never reach memory.  Nothing has a tolerance.  No matrix instruction fits: the work is a
// comparison per value, not a product.  Three launches whatever n, K and the sizes, no memset, nothing read back:
//   1. peaks_tables    workgroups 0 .. 2 n - 1 build the items' tables as back_tables does (table_axis_build); the workgroups after
//                      them set the n * K keys in the workspace to 0, "empty" (aa_many_back_peaks.h states the key and its order).
//   2. peaks_resample  one workgroup per work unit, AA_BACK_PEAKS_ROWS output rows times AA_BACK_TILE columns, a lane per column (the
//                      instance kernel's numbering and its clamped columns, so a wave's control flow is uniform).  The lane's
//                      horizontal window is read once.  The class chunk is the OUTER loop, AA_BACK_UNROLL classes at a time through
//                      class_sums (one vector load for aligned interleaved items); inside it the lane walks down the rows of its tile
//                      and keeps per class of the chunk the greatest key it has seen, 64 bits in registers — an integer maximum, so
//                      the rule is written once, in make_key.  A flipped item is mirrored where it is READ (the window of column
//                      ow - 1 - x); the flat index kept is the un-mirrored one.  After the tile's rows each class's keys meet: across
//                      the 64 lanes by four DPP steps on both halves of the key (quad_perm twice, row_half_mirror, row_mirror) and
//                      four readlanes; across the workgroup's waves through 2 x 4 x AA_BACK_UNROLL words of LDS, double-buffered by
//                      the chunk's parity so that ONE barrier a chunk suffices; then lane c of the workgroup issues one 64-bit
//                      atomicMax for class c of the chunk, skipped where a relaxed load shows a key already as great (the maximum
//                      is idempotent: the result is the same).  Every wave reaches every barrier: a wave wholly beyond ow computes
//                      nothing and holds empty keys.
//   3. peaks_decode    one lane per (item, channel): the key gives (x, y); R is resampled again at the peak and at its neighbours
//                      with table_row and class_sums<TIn, 1, false> — the same operations in the same order as launch 2's, so the
//                      same bits, with the sign of a zero and a NaN as aa_many_back.hip stores them — and peaks and values are
//                      written, every element of both.
// The maximum over a total order is associative and commutative: the bits do not depend on AA_BACK_PEAKS_ROWS, on the split over
// lanes, waves and workgroups, or on the run.  Every element offset is 64-bit.  Plain C++ and vector memory operations only.  Shared
// with the other files of the return path: aa_many_back_shared.h.

#include <string.h>

#include "aa_many_back_peaks.h"
#include "aa_many_back_shared.h"

namespace {

typedef unsigned long long u64;

constexpr int kRows = AA_BACK_PEAKS_ROWS;
constexpr int kWaves = AA_BACK_TILE / 64;
constexpr int kValues = AA_BACK_PEAKS_VALUES;

struct PeaksArgs {
  const AABackItem *items;
  const int64_t *unit0;
  const char *ws;
  u64 *keys;  // [n * K]
  int n, K;
};

// ---- the key ---------------------------------------------------------------------------------------------------------------------------------
// The monotone map of a float to uint32 after -0.0 has become +0.0 and every NaN the greatest word; never 0 (ord(-inf) = 0x007FFFFF).
__device__ inline unsigned ord_of(float v) {
  if (v != v) return 0xFFFFFFFFu;
  const unsigned u = v == 0.0f ? 0u : __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : u | 0x80000000u;
}
__device__ inline u64 make_key(float v, unsigned flat) { return (u64)ord_of(v) << 32 | (0xFFFFFFFFu - flat); }

// The greater of a lane's key and the key of the lane a DPP control names; all 64 lanes active.
template <int CTRL> __device__ inline u64 dpp_max(u64 v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, 0xF, 0xF, true);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, 0xF, 0xF, true);
  const u64 o = (u64)hi << 32 | lo;
  return o > v ? o : v;
}
__device__ inline u64 read_key(u64 v, int lane) {
  return (u64)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane) << 32 | (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane);
}
// The greatest key of the wave's 64 lanes, all of them active: within quads, halves of eight and rows of sixteen by DPP, then the
// four rows through scalar registers.  (uniform)
__device__ inline u64 wave_max(u64 v) {
  v = dpp_max<0xB1>(v);   // quad_perm [1, 0, 3, 2]
  v = dpp_max<0x4E>(v);   // quad_perm [2, 3, 0, 1]
  v = dpp_max<0x141>(v);  // row_half_mirror
  v = dpp_max<0x140>(v);  // row_mirror
  const u64 a = read_key(v, 0), b = read_key(v, 16), c = read_key(v, 32), d = read_key(v, 48);
  const u64 ab = a > b ? a : b, cd = c > d ? c : d;
  return ab > cd ? ab : cd;
}

// ---- 1. tables, and the keys emptied ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(AA_BACK_THREADS) peaks_tables(const AABackItem *items, int n, char *ws, int filter, int64_t *keys, int64_t key_elems) {
  const int64_t b = (int64_t)blockIdx.x - 2 * (int64_t)n;
  if (b < 0) {  // (uniform over the workgroup: there are barriers in the body)
    const AABackItem &it = items[blockIdx.x >> 1];
    const bool horiz = blockIdx.x & 1;
    const TableAxis ax = {horiz ? it.w : it.h, horiz ? it.ow : it.oh, horiz ? it.ksize_w : it.ksize_h, 0, horiz ? it.scale_w : it.scale_h,
                          ws + (horiz ? it.tab_w : it.tab_h), nullptr};
    table_axis_build<AA_BACK_THREADS>(ax, filter, 0);
    return;
  }
  zero_counts(keys, key_elems, b, (int64_t)gridDim.x - 2 * (int64_t)n);
}

// ---- 2. resample and reduce ------------------------------------------------------------------------------------------------------------------
// What a chunk's walk needs of the lane's place: its tile, whether its column and any column of its wave lie inside the item, its
// un-mirrored column (clamped to the item), and its horizontal window.
struct Place {
  RowTile t;
  bool in, wave_in;
  int x;
  Row rx;
};

// V classes from class k on: the lane's greatest key per class over the rows of its tile, the wave's, the workgroup's (part: this
// chunk's kWaves x AA_BACK_UNROLL words of LDS), and one atomicMax per class into keys[k ..].  Every lane of the workgroup comes here.
template <typename TIn, int V, bool VEC>
__device__ inline void chunk_keys(const PeaksArgs &a, const AABackItem &it, const Place &pl, int k, u64 (*part)[AA_BACK_UNROLL], u64 *keys) {
  u64 best[V];
#pragma unroll
  for (int c = 0; c < V; c++) best[c] = 0;
  if (pl.wave_in) {  // (uniform over the wave)
    const int64_t sch = it.stride_ch, prow = it.stride_row, ppx = it.stride_px;
    const TIn *p = (const TIn *)it.src + pl.rx.x0 * ppx + k * sch;
    for (int y = pl.t.y0; y < pl.t.y1; y++) {
      const Row ry = table_row(a.ws + it.tab_h, it.h, it.oh, it.ksize_h, y);
      float acc[V];
      class_sums<TIn, V, VEC>(p + ry.x0 * prow, sch, prow, ppx, ry, pl.rx, acc);
      const unsigned flat = (unsigned)y * (unsigned)it.ow + (unsigned)pl.x;
#pragma unroll
      for (int c = 0; c < V; c++) {
        const u64 key = pl.in ? make_key(acc[c], flat) : 0;
        best[c] = key > best[c] ? key : best[c];
      }
    }
  }
  const int wave = (int)(threadIdx.x >> 6);
#pragma unroll
  for (int c = 0; c < V; c++) {
    const u64 m = wave_max(best[c]);
    if ((threadIdx.x & 63) == 0) part[wave][c] = m;
  }
  __syncthreads();
  if (threadIdx.x < V) {
    u64 m = part[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kWaves; w++) m = part[w][threadIdx.x] > m ? part[w][threadIdx.x] : m;
    u64 *dst = keys + k + threadIdx.x;
    if (m != 0 && __hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < m) atomicMax(dst, m);
  }
}

template <typename TIn, bool VEC>
__global__ void __launch_bounds__(AA_BACK_TILE) peaks_resample(PeaksArgs a) {
  __shared__ u64 part[2][kWaves][AA_BACK_UNROLL];
  constexpr int U = AA_BACK_UNROLL;
  const int64_t unit = blockIdx.x;
  const int item = aa_unit_item(a.unit0, a.n, unit);
  const AABackItem &it = a.items[item];
  Place pl;
  pl.wave_in = row_tile<kRows>(unit - a.unit0[item], it.xtiles, it.oh, it.ow, pl.t);
  pl.in = pl.t.x < it.ow;
  pl.x = pl.in ? pl.t.x : it.ow - 1;  // (clamped: every address lies inside the item)
  const int xr = (it.flags & AA_MANY_FLIP_X) ? it.ow - 1 - pl.x : pl.x;
  pl.rx = table_row(a.ws + it.tab_w, it.w, it.ow, it.ksize_w, xr);
  u64 *keys = a.keys + (int64_t)item * a.K;
  int k = 0, chunk = 0;
  for (; k + U <= a.K; k += U, chunk++) chunk_keys<TIn, U, VEC>(a, it, pl, k, part[chunk & 1], keys);
  for (; k < a.K; k++, chunk++) chunk_keys<TIn, 1, false>(a, it, pl, k, part[chunk & 1], keys);
}

// ---- 3. decode -------------------------------------------------------------------------------------------------------------------------------
// R of channel k of item `it` at (y, x), x the un-mirrored column: launch 2's operations in its order.
template <typename TIn> __device__ inline float value_at(const PeaksArgs &a, const AABackItem &it, int k, int y, int x) {
  const int xr = (it.flags & AA_MANY_FLIP_X) ? it.ow - 1 - x : x;
  const Row ry = table_row(a.ws + it.tab_h, it.h, it.oh, it.ksize_h, y), rx = table_row(a.ws + it.tab_w, it.w, it.ow, it.ksize_w, xr);
  const int64_t sch = it.stride_ch, prow = it.stride_row, ppx = it.stride_px;
  float acc[1];
  class_sums<TIn, 1, false>((const TIn *)it.src + ry.x0 * prow + rx.x0 * ppx + k * sch, sch, prow, ppx, ry, rx, acc);
  return acc[0];
}

template <typename TIn>
__global__ void __launch_bounds__(AA_BACK_THREADS) peaks_decode(PeaksArgs a, int32_t *peaks, float *values) {
  const int64_t e = (int64_t)blockIdx.x * AA_BACK_THREADS + threadIdx.x;
  if (e >= (int64_t)a.n * a.K) return;
  const int item = (int)(e / a.K), k = (int)(e - (int64_t)item * a.K);
  const AABackItem &it = a.items[item];
  const u64 key = a.keys[e];
  // (an item has a pixel, so its keys are not empty and their indices lie inside it; a key that is neither decodes to pixel 0)
  const unsigned flat = key != 0 ? 0xFFFFFFFFu - (unsigned)key : 0u;
  int y = (int)(flat / (unsigned)it.ow), x = (int)(flat - (unsigned)y * (unsigned)it.ow);
  if (y >= it.oh) y = x = 0;
  const float v = value_at<TIn>(a, it, k, y, x);
  peaks[2 * e] = x;
  peaks[2 * e + 1] = y;
  float *o = values + kValues * e;
  o[0] = v;
  o[1] = x > 0 ? value_at<TIn>(a, it, k, y, x - 1) : v;
  o[2] = x + 1 < it.ow ? value_at<TIn>(a, it, k, y, x + 1) : v;
  o[3] = y > 0 ? value_at<TIn>(a, it, k, y - 1, x) : v;
  o[4] = y + 1 < it.oh ? value_at<TIn>(a, it, k, y + 1, x) : v;
}

// ---- the launch's choice of kernel -----------------------------------------------------------------------------------------------------------
void launch_resample(bool vec, int in_dtype, const PeaksArgs &a, unsigned units, hipStream_t stream) {
  with_float_type(in_dtype, [&](auto in) {
    using TIn = tag_t<decltype(in)>;
    if (vec) hipLaunchKernelGGL((peaks_resample<TIn, true>), dim3(units), dim3(AA_BACK_TILE), 0, stream, a);
    else hipLaunchKernelGGL((peaks_resample<TIn, false>), dim3(units), dim3(AA_BACK_TILE), 0, stream, a);
  });
}
void launch_decode(int in_dtype, const PeaksArgs &a, int32_t *peaks, float *values, hipStream_t stream) {
  const unsigned blocks = (unsigned)(((int64_t)a.n * a.K + AA_BACK_THREADS - 1) / AA_BACK_THREADS);
  with_float_type(in_dtype, [&](auto in) {
    hipLaunchKernelGGL((peaks_decode<tag_t<decltype(in)>>), dim3(blocks), dim3(AA_BACK_THREADS), 0, stream, a, peaks, values);
  });
}

// n * K keys, a lane of the decode each: one grid.
inline bool shape_ok(int64_t n, int64_t K) { return n < 0 || K < 1 || n > kAAManyMax || K > kAAManyMax || n * K <= INT32_MAX; }

}  // namespace

// ---- host: the planner -----------------------------------------------------------------------------------------------------------------------
size_t aa_back_peaks_desc_size(int64_t n) { return n < 0 ? 0 : aa_desc_size(sizeof(AABackPeaksHeader), sizeof(AABackItem), n); }

// aa_back_plan_host's checks in its order: n * K beyond one grid beside n and K; the pointers; the block's size; per item its own
// checks, then oh * ow against AA_BACK_PEAKS_MAX_PIXELS (a flat index is 32 bits of the key) and the work units against one grid.
int aa_back_peaks_plan_host(int filter, int layout, int64_t n, int64_t K, const aa_back_item *in, void *desc_host, size_t desc_bytes,
                            size_t *workspace_bytes, size_t *arena_bytes, int64_t *values_offset) {
  int rc = plan_prologue(filter, layout, n, K, AA_BACK_VALUES, AA_BACK_ACT_NONE, AA_F32, shape_ok(n, K));
  if (rc != AA_OK) return rc;
  if (!desc_host || !workspace_bytes || !arena_bytes || !values_offset || (n > 0 && !in)) return AA_ERR_NULL;
  if (desc_bytes < aa_back_peaks_desc_size(n)) return AA_ERR_WORKSPACE;
  AABackPeaksHeader *hd = (AABackPeaksHeader *)desc_host;
  const AADescView<AABackItem> v = aa_desc_view<AABackPeaksHeader, AABackItem>(desc_host, n);
  AABackItem *items = (AABackItem *)v.items;
  int64_t *unit0 = (int64_t *)v.prefix;
  size_t ws = 0;
  int64_t units = 0;
  for (int64_t i = 0; i < n; i++) {
    AABackItem it;
    if ((rc = plan_item(filter, layout, K, in[i], it, ws)) != AA_OK) return rc;
    if ((int64_t)it.oh * it.ow > AA_BACK_PEAKS_MAX_PIXELS) return AA_ERR_BAD_SHAPE;
    it.out_off = i * K * 2 * (int64_t)sizeof(int32_t);  // (its peaks)
    unit0[i] = units;
    units += (int64_t)((it.oh + kRows - 1) / kRows) * it.xtiles;
    if (units > INT32_MAX) return AA_ERR_BAD_SHAPE;  // (one grid)
    items[i] = it;
  }
  unit0[n] = units;
  memset(hd, 0, sizeof(*hd));
  hd->magic = AA_BACK_PEAKS_MAGIC;
  hd->n = (int32_t)n; hd->K = (int32_t)K; hd->filter = filter; hd->layout = layout; hd->rows = kRows;
  hd->units = units;
  hd->tables_bytes = (int64_t)ws;
  ws = aa_align16(ws);
  hd->keys_off = (int64_t)ws;
  ws += (size_t)n * (size_t)K * sizeof(u64);
  hd->ws_bytes = (int64_t)ws;
  size_t arena = aa_align16((size_t)n * (size_t)K * 2 * sizeof(int32_t));
  hd->values_off = (int64_t)arena;
  arena += (size_t)n * (size_t)K * kValues * sizeof(float);
  hd->arena_bytes = (int64_t)arena;
  *workspace_bytes = ws;
  *arena_bytes = arena;
  *values_offset = hd->values_off;
  return AA_OK;
}

// ---- host: the three launches ----------------------------------------------------------------------------------------------------------------
// aa_launch_back_many's checks in their order, every one before the first launch; the arena on a 4-byte boundary.
int aa_launch_back_peaks(const void *desc_host, const void *desc_dev, int in_dtype, void *arena_dev, size_t arena_bytes, void *workspace_dev,
                         size_t workspace_bytes, hipStream_t stream) {
  const AABackPeaksHeader *hd = (const AABackPeaksHeader *)desc_host;
  if (hd->magic != AA_BACK_PEAKS_MAGIC || !aa_filter_valid(hd->filter) || hd->n < 0 || hd->K < 1 || (int64_t)hd->n * hd->K > INT32_MAX ||
      hd->rows != kRows || hd->units < 0 || hd->units > INT32_MAX || (hd->layout != AA_NCHW && hd->layout != AA_NHWC) || (hd->keys_off & 15) ||
      hd->keys_off < hd->tables_bytes || hd->ws_bytes < hd->keys_off + (int64_t)hd->n * hd->K * 8 || (hd->values_off & 15) ||
      hd->values_off < (int64_t)hd->n * hd->K * 8 || hd->arena_bytes < hd->values_off + (int64_t)hd->n * hd->K * kValues * 4)
    return AA_ERR_BAD_SHAPE;
  if (!float_dtype(in_dtype)) return AA_ERR_BAD_DTYPE;
  const int rc = aa_many_check_launch(hd->n, desc_dev, arena_dev, workspace_dev, workspace_bytes, hd->ws_bytes, sizeof(int32_t));
  if (rc != AA_OK || hd->n == 0) return rc;
  if (arena_bytes < (size_t)hd->arena_bytes) return AA_ERR_WORKSPACE;
  const AADescView<AABackItem> host = aa_desc_view<AABackPeaksHeader, AABackItem>(desc_host, hd->n);
  bool vec;
  const int rs = check_sources(host.items, hd->n, in_dtype, hd->layout, hd->K, &vec);
  if (rs != AA_OK) return rs;
  const AADescView<AABackItem> dev = aa_desc_view<AABackPeaksHeader, AABackItem>(desc_dev, hd->n);
  PeaksArgs a;
  a.items = dev.items; a.unit0 = dev.prefix; a.ws = (const char *)workspace_dev;
  a.keys = (u64 *)((char *)workspace_dev + hd->keys_off);
  a.n = hd->n; a.K = hd->K;
  const int64_t key_elems = (int64_t)hd->n * hd->K;
  hipLaunchKernelGGL(peaks_tables, dim3(2u * (unsigned)hd->n + zero_blocks(key_elems)), dim3(AA_BACK_THREADS), 0, stream, dev.items, (int)hd->n,
                     (char *)workspace_dev, (int)hd->filter, (int64_t *)a.keys, key_elems);
  AA_HIP_CHECK_LAUNCH();
  launch_resample(vec, in_dtype, a, (unsigned)hd->units, stream);
  AA_HIP_CHECK_LAUNCH();
  launch_decode(in_dtype, a, (int32_t *)arena_dev, (float *)((char *)arena_dev + hd->values_off), stream);
  AA_HIP_CHECK_LAUNCH();
  return AA_OK;
}
