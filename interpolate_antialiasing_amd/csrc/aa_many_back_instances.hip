// aa_many_back_instances.hip — instance inference of mask-classification heads (MaskFormer, Mask2Former, OneFormer) in the ragged return
// path: item i is Q mask logits [Q, h_i, w_i] and M slots, slot m asking for query queries[i, m] (an entry outside 0 .. Q - 1: an empty
// slot; entries may repeat, as they do after a top-k over Q x C).  With R_i the fp32 resample of aa_many_back.hip (K = Q, bit for bit),
//   mask[m]  = R_i[q] > 0                          a NaN is false; an empty slot's mask is all zeros
//   stats[m] = (area, psum, x0, y0, x1, y1)        area: the mask's pixels; psum: the sum over them of aa_sigmoid(R_i[q]) * 2^24, every
//                                                  term an exact integer (a sigmoid of a positive value lies in [0.5, 1], where float32
//                                                  steps by 2^-24 or more); the tight half-open box, (ow, oh, 0, 0) for an empty mask
// Nothing here has a tolerance.  No matrix instruction fits: the work is a threshold and counting, not a product.  Two launches
// whatever n, M and the sizes (the kernels: aa_many_back_instances_dev.h, shared with the run-length form):
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

#include "aa_many_back_instances_dev.h"

namespace {

// ---- the launch's choice of kernel ---------------------------------------------------------------------------------------------------------------
void launch_resample(bool vec, int in_dtype, bool bits, const InstancesArgs &a, unsigned units, hipStream_t stream) {
  with_float_type(in_dtype, [&](auto in) {
    if (bits) launch_resample_sink<tag_t<decltype(in)>, kSinkBits>(vec, a, units, stream);
    else launch_resample_sink<tag_t<decltype(in)>, kSinkBytes>(vec, a, units, stream);
  });
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
