// aa_many_back_instances_rle.hip — the instance inference of aa_many_back_instances.hip with COCO's uncompressed run-length encoding as
// the mask output (aa_many_back_instances_rle.h): slot m's mask R_i[q] > 0 is read column by column (y fastest: COCO's Fortran order)
// and runs[i, m, :] are the lengths of its runs, zeros first; nruns[i, m] their true count; stats as the instance call has them, bit
// for bit.  No mask exists as bytes anywhere: the ballot words the resample forms are the only form the masks ever take.  Three
// launches whatever n, Q, M and the sizes:
//   1. instances_tables    aa_many_back_instances_dev.h, unchanged: tables, the slots sorted by query, the stats set.
//   2. instances_resample  the same file's kernel with its third sink: the ballot word of (distinct query, row, wave) is stored by lane 0
//                          as ONE aligned 8-byte store into the query's bit plane [oh][ceil(ow / 64)] of the workspace — zero or not,
//                          the plane is read in full — and the stats are added as before.  Nothing is stored per slot.
//   3. instances_encode    one workgroup of four waves per (item, place j among the item's sorted slots).  A place behind the asking
//                          slots is an EMPTY slot: its row is [oh ow, 0, ...], nruns 1.  A place that is not the first of its query's
//                          range leaves.  The first of a range encodes the query's plane for every slot of the range.  A wave owns
//                          every fourth 64-column strip, a lane a column.  walk_strip: 64 rows at a time, lane l loads the strip's
//                          word of row y0 + l and of the row above it (for row 0: the LAST row's word shifted up one column, bit 63
//                          of the strip before carried in: column x - 1's end meets column x's start, column 0 meets 0), their XOR
//                          is the row's vertical transitions, one ballot finds the rows that have any — sparse masks: few — and
//                          each such word is broadcast with two readlanes, lane c taking bit c.
//                            pass A   every lane counts its column's transitions and keeps the last one's y; the wave scans the 64
//                                     columns (shuffles: an exclusive sum of the counts, an exclusive maximum of the last flat position
//                                     x oh + y) into two int32 per column of LDS, and the strip's totals into two per strip.  Behind a
//                                     barrier lane t < strips sums the strips before its own (at most 64), and the last strip's lane
//                                     leaves the mask's transitions T and its last position.
//                            pass B   the same walk again: at a transition the lane knows the run it ends (strip base + column base +
//                                     its own count so far) and the run's length (the position minus the previous transition's, its
//                                     own or the scanned one, 0 before the first) and stores it — a 4-byte vector store — into the
//                                     row of EVERY slot of the range, if the index is below max_runs.  A strip whose base is already
//                                     max_runs or more is skipped.
//                          Lane 0 stores the closing run oh ow - last position at index T and nruns = T + 1; the workgroup zeroes
//                          the rows from T + 1 to max_runs.  Every slot's row is written in pass B (not written once and copied:
//                          the copy was not built and not measured).
// The scan's LDS bounds ow at AA_BACK_INSTANCES_RLE_MAX_OW (no spill to the workspace is built); flat positions are int32, so
// oh ow < 2^31 - 1.  Everything is integers, and every store is by one lane to an address no other lane or workgroup writes: the same
// bits on every run.  Plain C++ and vector memory operations only.

#include <string.h>

#include "aa_many_back_instances_rle.h"
#include "aa_many_back_instances_dev.h"

namespace {

constexpr int kEncodeThreads = AA_BACK_INSTANCES_RLE_THREADS, kEncodeWaves = kEncodeThreads / 64;
constexpr int kMaxStrips = AA_BACK_INSTANCES_RLE_MAX_OW / 64;
static_assert(kMaxStrips <= kEncodeThreads, "a lane per strip sums the strips before it");

inline int strips_of(int64_t ow) { return (int)((ow + 63) >> 6); }
// int32 words of the encode's LDS for `strips` strips: per column the count and position bases, per strip its totals and its bases, T
// and the last position.
inline size_t encode_lds_bytes(int strips) { return ((size_t)strips * (2 * 64 + 4) + 2) * sizeof(int32_t); }

struct EncodeArgs {
  const AABackItem *items;
  const char *ws;
  const char *planes;  // the planes' part of the workspace
  Queries queries;
  WorkLists lists;
  int32_t *runs, *nruns;
  int max_runs;
};

// The vertical transitions of one 64-column strip, rows ascending: at(y) on lane c where column c's pixel of row y differs from the
// pixel above it.  col: the strip's word of row 0 (the next row's W words on); above0: the word above row 0; cols: the strip's columns
// inside the mask.  All 64 lanes call it together.
template <typename F>
__device__ inline void walk_strip(const unsigned long long *col, int W, int oh, unsigned long long above0, unsigned long long cols, int lane, F &&at) {
  for (int y0 = 0; y0 < oh; y0 += 64) {
    const int y = y0 + lane;
    unsigned long long t = 0;
    if (y < oh) {
      const unsigned long long word = col[(int64_t)y * W];
      const unsigned long long above = y > 0 ? col[(int64_t)(y - 1) * W] : above0;
      t = (word ^ above) & cols;
    }
    unsigned long long rows = __ballot(t != 0);
    while (rows != 0) {  // (uniform)
      const int r = __builtin_ctzll(rows);
      rows &= rows - 1;
      const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)t, r), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(t >> 32), r);
      if (((unsigned long long)hi << 32 | lo) >> lane & 1) at(y0 + r);
    }
  }
}

__global__ void __launch_bounds__(kEncodeThreads) instances_encode(EncodeArgs a) {
  extern __shared__ int32_t lds[];
  const int M = a.lists.M, max_runs = a.max_runs;
  const int item = (int)(blockIdx.x / (unsigned)M), j = (int)(blockIdx.x % (unsigned)M);
  const AABackItem &it = a.items[item];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t *list = work_list((char *)a.ws, a.lists, item);
  const int32_t *ranges = list_ranges(list), *slots = list_slots(list, a.lists);
  const int valid = __builtin_amdgcn_readfirstlane(list[1]);
  const int oh = it.oh, ow = it.ow, total = oh * ow;  // (below 2^31 - 1: the planner)
  int32_t *rows = a.runs + (int64_t)item * M * max_runs, *counts = a.nruns + (int64_t)item * M;
  const int slot0 = __builtin_amdgcn_readfirstlane(slots[j]);
  if (j >= valid) {  // an empty slot: one run of zeros   (every branch here is uniform over the workgroup: there are barriers below)
    int32_t *row = rows + (int64_t)slot0 * max_runs;
    for (int r = tid; r < max_runs; r += kEncodeThreads) row[r] = r == 0 ? total : 0;
    if (tid == 0) counts[slot0] = 1;
    return;
  }
  const int q = __builtin_amdgcn_readfirstlane((int)query_at(a.queries, item, slot0));  // (in 0 .. Q - 1: the slot sorted before the empty ones)
  const unsigned range = (unsigned)__builtin_amdgcn_readfirstlane(ranges[q]);
  const int first = (int)(range & 0xFFFF), len = (int)(range >> 16);
  if (first != j) return;  // the range's first place encodes for all of it

  const int W = (ow + 63) >> 6;
  const unsigned long long *plane = (const unsigned long long *)(a.planes + it.out_off) + (int64_t)plane_of(a.lists, q, first) * oh * W;
  int32_t *col_count = lds, *col_pos = lds + 64 * W, *strip_count = lds + 128 * W, *strip_pos = strip_count + W, *strip_base = strip_pos + W,
          *strip_prev = strip_base + W, *whole = strip_prev + W;
  auto strip_cols = [&](int s) { return ow - 64 * s >= 64 ? ~0ull : (1ull << (ow - 64 * s)) - 1; };
  // the word above row 0 of strip s: column x - 1's last pixel for column x
  auto strip_above = [&](int s) {
    const unsigned long long *last = plane + (int64_t)(oh - 1) * W + s;
    return last[0] << 1 | (s > 0 ? last[-1] >> 63 : 0ull);
  };

  // ---- pass A: the columns' counts and last positions, scanned over the strip
  for (int s = wave; s < W; s += kEncodeWaves) {
    const int x = 64 * s + lane;
    int c = 0, last = 0;
    walk_strip(plane + s, W, oh, strip_above(s), strip_cols(s), lane, [&](int y) { c++; last = y; });
    const int p = c != 0 ? x * oh + last : 0;
    int ci = c, pi = p;  // inclusive over the lanes up to this one
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_up(ci, d), u = __shfl_up(pi, d);
      if (lane >= d) {
        ci += v;
        pi = max(pi, u);
      }
    }
    const int before = __shfl_up(pi, 1);
    col_count[x] = ci - c;
    col_pos[x] = lane != 0 ? before : 0;
    if (lane == 63) {
      strip_count[s] = ci;
      strip_pos[s] = pi;
    }
  }
  __syncthreads();
  if (tid < W) {
    int base = 0, prev = 0;
    for (int u = 0; u < tid; u++) {
      base += strip_count[u];
      prev = max(prev, strip_pos[u]);
    }
    strip_base[tid] = base;
    strip_prev[tid] = prev;
    if (tid == W - 1) {
      whole[0] = base + strip_count[tid];
      whole[1] = max(prev, strip_pos[tid]);
    }
  }
  __syncthreads();

  // ---- pass B: every transition ends a run
  for (int s = wave; s < W; s += kEncodeWaves) {
    const int base = __builtin_amdgcn_readfirstlane(strip_base[s]);
    if (base >= max_runs) continue;  // (uniform; the strips after it start later still)
    const int x = 64 * s + lane;
    int index = base + col_count[x], prev = max(strip_prev[s], col_pos[x]);
    walk_strip(plane + s, W, oh, strip_above(s), strip_cols(s), lane, [&](int y) {
      const int p = x * oh + y;
      if (index < max_runs)
        for (int k = first; k < first + len; k++) rows[(int64_t)slots[k] * max_runs + index] = p - prev;
      prev = p;
      index++;
    });
  }

  // ---- the closing run, the count, the zero tail
  const int T = whole[0];
  for (int k = first; k < first + len; k++) {
    const int slot = __builtin_amdgcn_readfirstlane(slots[k]);
    int32_t *row = rows + (int64_t)slot * max_runs;
    if (tid == 0) {
      if (T < max_runs) row[T] = total - whole[1];
      counts[slot] = T + 1;
    }
    for (int64_t r = (int64_t)T + 1 + tid; r < max_runs; r += kEncodeThreads) row[r] = 0;
  }
}

inline bool rle_shape_ok(int64_t Q, int64_t M, int64_t max_runs) { return shape_ok(Q, M, 0) && max_runs >= 1 && max_runs <= AA_BACK_INSTANCES_RLE_MAX_RUNS; }

}  // namespace

// ---- host: the planner ---------------------------------------------------------------------------------------------------------------------
size_t aa_back_instances_rle_desc_size(int64_t n) { return n < 0 ? 0 : aa_desc_size(sizeof(AABackInstancesRleHeader), sizeof(AABackItem), n); }

// aa_back_instances_plan_host's checks in its order, max_runs outside 1 .. AA_BACK_INSTANCES_RLE_MAX_RUNS in the place of `bits`; per
// item after its own checks ow beyond AA_BACK_INSTANCES_RLE_MAX_OW and oh * ow of 2^31 - 1 or more, then the planes, the arena and the
// two grids.
int aa_back_instances_rle_plan_host(int filter, int layout, int64_t n, int64_t Q, int64_t M, const aa_back_item *in, int64_t max_runs, void *desc_host,
                                    size_t desc_bytes, size_t *workspace_bytes, size_t *arena_bytes, int64_t *nruns_offset, int64_t *stats_offset) {
  int rc = plan_prologue(filter, layout, n, Q, AA_BACK_GREATER, AA_BACK_ACT_NONE, AA_U8, rle_shape_ok(Q, M, max_runs));
  if (rc != AA_OK) return rc;
  if (!desc_host || !workspace_bytes || !arena_bytes || !nruns_offset || !stats_offset || (n > 0 && !in)) return AA_ERR_NULL;
  if (desc_bytes < aa_back_instances_rle_desc_size(n)) return AA_ERR_WORKSPACE;
  AABackInstancesRleHeader *hd = (AABackInstancesRleHeader *)desc_host;
  const AADescView<AABackItem> v = aa_desc_view<AABackInstancesRleHeader, AABackItem>(desc_host, n);
  AABackItem *items = (AABackItem *)v.items;
  int64_t *unit0 = (int64_t *)v.prefix;
  const size_t per_item = (size_t)(Q < M ? Q : M);  // planes
  size_t ws = 0, planes = 0;
  int64_t units = 0, max_ow = 0;
  for (int64_t i = 0; i < n; i++) {
    AABackItem it;
    if ((rc = plan_item(filter, layout, Q, in[i], it, ws)) != AA_OK) return rc;
    if (it.ow > AA_BACK_INSTANCES_RLE_MAX_OW || (int64_t)it.oh * it.ow >= INT32_MAX) return AA_ERR_BAD_SHAPE;
    planes = aa_align16(planes);
    it.out_off = (int64_t)planes;
    planes += per_item * (size_t)it.oh * (size_t)strips_of(it.ow) * 8;
    if (planes > (size_t)AA_BACK_MAX_ELEMS * 8) return AA_ERR_BAD_SHAPE;
    unit0[i] = units;
    units += (int64_t)((it.oh + kRows - 1) / kRows) * it.xtiles;
    if (units > INT32_MAX) return AA_ERR_BAD_SHAPE;  // (one grid)
    max_ow = it.ow > max_ow ? it.ow : max_ow;
    items[i] = it;
  }
  if (n * M > INT32_MAX || (size_t)n * (size_t)M * (size_t)max_runs > (size_t)AA_BACK_MAX_ELEMS) return AA_ERR_BAD_SHAPE;  // (the encode's grid; the arena)
  unit0[n] = units;
  memset(hd, 0, sizeof(*hd));
  hd->magic = AA_BACK_INSTANCES_RLE_MAGIC;
  hd->n = (int32_t)n; hd->Q = (int32_t)Q; hd->M = (int32_t)M; hd->filter = filter; hd->layout = layout; hd->max_runs = (int32_t)max_runs;
  hd->list_words = list_words(Q, M);
  hd->units = units;
  hd->max_ow = max_ow;
  hd->tables_bytes = (int64_t)ws;
  ws = aa_align16(ws);
  hd->lists_off = (int64_t)ws;
  ws = aa_align16(ws + (size_t)n * hd->list_words * sizeof(int32_t));
  hd->planes_off = (int64_t)ws;
  ws += planes;
  hd->ws_bytes = (int64_t)ws;
  size_t arena = aa_align16((size_t)n * (size_t)M * (size_t)max_runs * sizeof(int32_t));
  hd->nruns_off = (int64_t)arena;
  arena = aa_align16(arena + (size_t)n * (size_t)M * sizeof(int32_t));
  hd->stats_off = (int64_t)arena;
  arena += (size_t)n * (size_t)M * kStats * sizeof(int64_t);
  hd->arena_bytes = (int64_t)arena;
  *workspace_bytes = ws;
  *arena_bytes = arena;
  *nruns_offset = hd->nruns_off;
  *stats_offset = hd->stats_off;
  return AA_OK;
}

// ---- host: the three launches ------------------------------------------------------------------------------------------------------------------
// aa_launch_back_instances' checks in their order, every one before the first launch; the LDS check counts the encode's scan for the
// plan's widest item.
int aa_back_instances_rle_launch(const void *desc_host, const void *desc_dev, int in_dtype, const aa_back_instances_io *io, void *arena_dev,
                                 size_t arena_bytes, void *workspace_dev, size_t workspace_bytes, hipStream_t stream) {
  const AABackInstancesRleHeader *hd = (const AABackInstancesRleHeader *)desc_host;
  if (hd->magic != AA_BACK_INSTANCES_RLE_MAGIC || !aa_filter_valid(hd->filter) || hd->n < 0 || hd->Q < 1 || !rle_shape_ok(hd->Q, hd->M, hd->max_runs) ||
      hd->units < 0 || hd->units > INT32_MAX || (int64_t)hd->n * hd->M > INT32_MAX || (hd->layout != AA_NCHW && hd->layout != AA_NHWC) ||
      hd->list_words != list_words(hd->Q, hd->M) || hd->lists_off < hd->tables_bytes || (hd->lists_off & 15) ||
      hd->planes_off < hd->lists_off + (int64_t)hd->n * hd->list_words * 4 || (hd->planes_off & 15) || hd->ws_bytes < hd->planes_off || hd->max_ow < 0 ||
      hd->max_ow > AA_BACK_INSTANCES_RLE_MAX_OW || (hd->nruns_off & 15) || hd->nruns_off < (int64_t)hd->n * hd->M * hd->max_runs * 4 || (hd->stats_off & 15) ||
      hd->stats_off < hd->nruns_off + (int64_t)hd->n * hd->M * 4 || hd->arena_bytes < hd->stats_off + (int64_t)hd->n * hd->M * kStats * 8)
    return AA_ERR_BAD_SHAPE;
  if (!float_dtype(in_dtype)) return AA_ERR_BAD_DTYPE;
  const int rc = aa_many_check_launch(hd->n, desc_dev, arena_dev, workspace_dev, workspace_bytes, hd->ws_bytes, sizeof(int64_t));
  if (rc != AA_OK || hd->n == 0) return rc;
  if (arena_bytes < (size_t)hd->arena_bytes) return AA_ERR_WORKSPACE;
  const AADescView<AABackItem> host = aa_desc_view<AABackInstancesRleHeader, AABackItem>(desc_host, hd->n);
  bool vec;
  const int rs = check_sources(host.items, hd->n, in_dtype, hd->layout, hd->Q, &vec);
  if (rs != AA_OK) return rs;
  // (the planes of every item lie inside the workspace, and no item is wider than the LDS was sized for)
  const int64_t per_item = hd->Q < hd->M ? hd->Q : hd->M;
  for (int64_t i = 0; i < hd->n; i++) {
    const AABackItem &it = host.items[i];
    if (it.ow > hd->max_ow || (int64_t)it.oh * it.ow >= INT32_MAX || it.out_off < 0 || (it.out_off & 7) ||
        hd->planes_off + it.out_off + per_item * it.oh * strips_of(it.ow) * 8 > hd->ws_bytes)
      return AA_ERR_BAD_SHAPE;
  }
  if (!io || !io->queries_dev) return AA_ERR_NULL;
  if (io->queries_elem_bytes != 4 && io->queries_elem_bytes != 8) return AA_ERR_BAD_DTYPE;
  if (io->queries_stride_n < 0 || io->queries_stride_m < 0 || (uintptr_t)io->queries_dev % (uintptr_t)io->queries_elem_bytes) return AA_ERR_STRIDES;
  const size_t encode_lds = encode_lds_bytes(strips_of(hd->max_ow));
  const int rl = lds_fits(stream, encode_lds);
  if (rl != AA_OK) return rl;
  const AADescView<AABackItem> dev = aa_desc_view<AABackInstancesRleHeader, AABackItem>(desc_dev, hd->n);
  const Queries queries = {io->queries_dev, io->queries_stride_n, io->queries_stride_m, io->queries_elem_bytes};
  const WorkLists lists = {hd->lists_off, hd->list_words, vec ? 1 : 0, hd->Q, hd->M};
  int64_t *stats = (int64_t *)((char *)arena_dev + hd->stats_off);
  const int64_t stat_elems = (int64_t)hd->n * hd->M * kStats;
  hipLaunchKernelGGL(instances_tables, dim3(3u * (unsigned)hd->n + zero_blocks(stat_elems)), dim3(AA_BACK_THREADS), 0, stream, dev.items, (int)hd->n,
                     (char *)workspace_dev, (int)hd->filter, queries, lists, stats, stat_elems);
  AA_HIP_CHECK_LAUNCH();
  InstancesArgs a;
  a.items = dev.items; a.unit0 = dev.prefix; a.ws = (const char *)workspace_dev; a.arena = (char *)workspace_dev + hd->planes_off;
  a.lists = lists; a.stats = stats; a.n = hd->n;
  with_float_type(in_dtype, [&](auto in) { launch_resample_sink<tag_t<decltype(in)>, kSinkPlanes>(vec, a, (unsigned)hd->units, stream); });
  AA_HIP_CHECK_LAUNCH();
  EncodeArgs e;
  e.items = dev.items; e.ws = (const char *)workspace_dev; e.planes = (const char *)workspace_dev + hd->planes_off;
  e.queries = queries; e.lists = lists;
  e.runs = (int32_t *)arena_dev; e.nruns = (int32_t *)((char *)arena_dev + hd->nruns_off); e.max_runs = hd->max_runs;
  hipLaunchKernelGGL(instances_encode, dim3((unsigned)(hd->n * hd->M)), dim3(kEncodeThreads), encode_lds, stream, e);
  AA_HIP_CHECK_LAUNCH();
  return AA_OK;
}
