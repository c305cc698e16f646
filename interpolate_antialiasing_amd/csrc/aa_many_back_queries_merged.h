// aa_many_back_queries_merged.h — the merged form of the mask-classification call (include/aa_interp.h, aa_back_queries_merged_plan):
// the n items are MEMBERS of G groups as in aa_many_back.h's merged plan, each with Q mask logits and a [Q, C] weight matrix of its own,
// and a group's scores are the sum over (member, query) of float16 products, taken in fp32 on the matrix unit, one long inner
// dimension.  The packed descriptor block:
//   [ AABackQueriesMergedHeader : 64 B ][ AABackItem x n ][ AABackGroup x G ][ int32 member[n], padded to 8 B ][ int64 unit0[G + 1] ]
//   [ AABackQueryWeights x n ]
// The sections between the header and the weights are aa_many_back.h's merged ones, unchanged.  The workspace is the members' tables
// (aa_back_many_plan's for the same items) and behind them, at ws_bytes - n * aa_back_queries_packed_bytes(Q, C), every member's weights
// as float16 in the operand order of v_mfma_f32_32x32x16_f16:
//   [member][class block of 32][query step of 16][64 lanes][8 halves]
// lane l of (block b, step s) holding class 32 b + l % 32 for the queries 16 s + 8 (l / 32) .. + 7; classes >= C and queries >= Q are +0.
#pragma once

#include "aa_many_back_queries.h"

#define AA_BACK_QUERIES_MERGED_MAGIC 0x5952514D  // 'MQRY'

struct AABackQueriesMergedHeader {
  int32_t magic, n, Q, filter, layout;
  int32_t reduce;     // AA_BACK_VALUES or AA_BACK_ARGMAX
  int32_t out_dtype;  // aa_dtype of an arena element
  int32_t C;
  int64_t units;      // unit0[G]: the workgroups of the resample
  int64_t ws_bytes;   // the table arena, then (on a 16-byte boundary) the packed weights
  int64_t arena_bytes;
  int32_t G;
  int32_t merge;      // AA_BACK_MERGE_*
};
static_assert(sizeof(AABackQueriesMergedHeader) == 64, "descriptor header is 64 bytes");

// The bytes of one member's packed weights: Cpad * Qpad float16, C rounded up to 32 and Q to 16.
inline size_t aa_back_queries_packed_bytes(int64_t Q, int64_t C) {
  const size_t qpad = (size_t)(Q + AA_BACK_QUERIES_KSTEP - 1) / AA_BACK_QUERIES_KSTEP * AA_BACK_QUERIES_KSTEP;
  const size_t cpad = (size_t)(C + AA_BACK_QUERIES_MBLOCK - 1) / AA_BACK_QUERIES_MBLOCK * AA_BACK_QUERIES_MBLOCK;
  return cpad * qpad * 2;
}

size_t aa_back_queries_merged_desc_size(int64_t n, int64_t g);
int aa_back_queries_merged_plan_host(int filter, int layout, int64_t n, int64_t Q, int64_t C, const aa_back_item *items,
                                     const aa_back_weights *weights, int64_t G, const int64_t *group_of, int merge, int reduce, int out_dtype,
                                     void *desc_host, size_t desc_bytes, size_t *workspace_bytes, size_t *arena_bytes, int64_t *out_offsets);
int aa_launch_back_queries_merged(const void *desc_host, const void *desc_dev, int in_dtype, void *arena_dev, size_t arena_bytes,
                                  void *workspace_dev, size_t workspace_bytes, hipStream_t stream);
