// aa_many_back_queries.h — the ragged return path for mask-classification heads (include/aa_interp.h, aa_back_queries_plan): item i is
// Q mask logits [Q, h_i, w_i] and a weight matrix [Q, C]; the masks are resampled to [oh_i, ow_i] as aa_back_many_plan's items are
// (K = Q), go through the sigmoid, and the C scores of a pixel — the weights' transpose times the pixel's Q probabilities, float16
// operands, fp32 sums on the matrix unit — are stored or reduced to their argmax.  The packed descriptor block:
//   [ AABackQueriesHeader : 64 B ][ AABackItem x n ][ int64 unit0[n + 1] ][ AABackQueryWeights x n ]
// The sections before the weights are aa_many_back.h's, so the table kernel's body and the class loops read them unchanged.  unit0[i]
// is the first work unit of item i; a unit is one output row of an item times AA_BACK_TILE consecutive output columns.
#pragma once

#include "aa_many_back.h"

#define AA_BACK_QUERIES_MAGIC 0x59525551  // 'QURY'
#define AA_BACK_QUERIES_MAX_Q 256         // the queries of a call: a wave's probabilities, [Qpad][64] float16, stay in LDS (32 KiB a wave)
#define AA_BACK_QUERIES_KSTEP 16          // queries of one matrix instruction; Qpad is Q rounded up to it
#define AA_BACK_QUERIES_MBLOCK 32         // classes of one matrix instruction

struct AABackQueriesHeader {
  int32_t magic, n, Q, filter, layout;
  int32_t reduce;     // AA_BACK_VALUES or AA_BACK_ARGMAX
  int32_t out_dtype;  // aa_dtype of an arena element
  int32_t C;
  int64_t units;      // unit0[n]: the workgroups of the resample
  int64_t ws_bytes;   // the table arena, aa_back_many_plan's for the same items
  int64_t arena_bytes;
  int64_t reserved;
};
static_assert(sizeof(AABackQueriesHeader) == 64, "descriptor header is 64 bytes");

// What an item has besides its record: weight (q, c) at w + q * stride_q + c * stride_c float32 ELEMENTS.
struct AABackQueryWeights {
  const float *w;
  int64_t stride_q, stride_c;
  int64_t reserved;
};
static_assert(sizeof(AABackQueryWeights) == 32, "descriptor weight record is 32 bytes");

size_t aa_back_queries_desc_size(int64_t n);
int aa_back_queries_plan_host(int filter, int layout, int64_t n, int64_t Q, int64_t C, const aa_back_item *items, const aa_back_weights *weights,
                              int reduce, int out_dtype, void *desc_host, size_t desc_bytes, size_t *workspace_bytes, size_t *arena_bytes,
                              int64_t *out_offsets);
int aa_launch_back_queries(const void *desc_host, const void *desc_dev, int in_dtype, void *arena_dev, size_t arena_bytes, void *workspace_dev,
                           size_t workspace_bytes, hipStream_t stream);
