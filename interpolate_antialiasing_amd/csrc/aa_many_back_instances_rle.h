// aa_many_back_instances_rle.h — the instance inference of aa_many_back_instances.h with COCO's uncompressed run-length encoding as its
// mask output (include/aa_interp.h, aa_back_instances_rle_plan): slot m's mask [oh_i, ow_i] is read column by column, y fastest, and
// runs[i, m, :] are the lengths of its runs of zeros and ones in turn, the zeros first (0 where the first pixel is set); nruns[i, m] is
// their true count, of which the first max_runs are stored and the rest of the row is 0.  No mask is stored anywhere as bytes.  The
// packed descriptor block:
//   [ AABackInstancesRleHeader : 104 B ][ AABackItem x n ][ int64 unit0[n + 1] ]
// with the sections of aa_many_back_instances.h after the header; an item's out_off is the offset of its planes within the planes.
// The workspace: the tables (tables_bytes), from lists_off on the work lists of aa_many_back_instances.h, and from planes_off on the
// bit planes: per item min(Q, M) planes, one per DISTINCT asked query (the query itself where Q <= M, else the place of its first slot
// among the sorted slots), each [oh_i][ceil(ow_i / 64)] uint64, bit c of word s column 64 s + c, the bits beyond ow_i 0.  Planes
// nobody asked for are neither written nor read.
// The arena: runs [n, M, max_runs] int32 at 0, nruns [n, M] int32 at nruns_off, stats [n, M, 6] int64 at stats_off (multiples of 16).
#pragma once

#include "aa_many_back_instances.h"

#define AA_BACK_INSTANCES_RLE_MAGIC 0x454C5249     // 'IRLE'
#define AA_BACK_INSTANCES_RLE_MAX_RUNS (1 << 20)   // the most runs a slot's row holds
#define AA_BACK_INSTANCES_RLE_MAX_OW 4096          // the encode's scan keeps two int32 per column in LDS: 32 KiB at this width (no spill is built)
#define AA_BACK_INSTANCES_RLE_THREADS 256          // lanes of an encode workgroup: four waves, each owning every fourth 64-column strip

struct AABackInstancesRleHeader {
  int32_t magic, n, Q, M, filter, layout;
  int32_t max_runs;    // int32 words of a slot's row of runs
  int32_t list_words;  // as AABackInstancesHeader's
  int64_t units;       // unit0[n]: the workgroups of the resample
  int64_t ws_bytes;    // the tables, the work lists and the planes
  int64_t arena_bytes;
  int64_t tables_bytes;
  int64_t lists_off;   // of the workspace, a multiple of 16
  int64_t planes_off;  // of the workspace, a multiple of 16
  int64_t nruns_off;   // of the arena, a multiple of 16
  int64_t stats_off;   // of the arena, a multiple of 16
  int64_t max_ow;      // the widest item: sizes the encode's LDS
};
static_assert(sizeof(AABackInstancesRleHeader) == 104, "descriptor header is 104 bytes");

size_t aa_back_instances_rle_desc_size(int64_t n);
int aa_back_instances_rle_plan_host(int filter, int layout, int64_t n, int64_t Q, int64_t M, const aa_back_item *items, int64_t max_runs, void *desc_host,
                                    size_t desc_bytes, size_t *workspace_bytes, size_t *arena_bytes, int64_t *nruns_offset, int64_t *stats_offset);
int aa_back_instances_rle_launch(const void *desc_host, const void *desc_dev, int in_dtype, const aa_back_instances_io *io, void *arena_dev,
                                 size_t arena_bytes, void *workspace_dev, size_t workspace_bytes, hipStream_t stream);
