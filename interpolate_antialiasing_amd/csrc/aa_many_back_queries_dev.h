// aa_many_back_queries_dev.h — what the two mask-classification kernels share (aa_many_back_queries.hip: one item per output;
// aa_many_back_queries_merged.hip: the members of a group summed in the accumulators): the matrix instruction's vector types and sizes,
// the class a lane holds in an accumulator register, the running argmax candidate and its merge across lanes, and on the host what both
// planners and launches check of Q, C, the reduce and the output type, and a workgroup's LDS against the device's limit.  Each is
// written here once.  In the unnamed namespace like the kernels that use it.
#pragma once

#include "aa_many_back_queries.h"
#include "aa_many_back_shared.h"

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float float16v __attribute__((ext_vector_type(16)));

constexpr int kStep = AA_BACK_QUERIES_KSTEP, kBlock = AA_BACK_QUERIES_MBLOCK;
inline __host__ __device__ int padded_q(int Q) { return (Q + kStep - 1) / kStep * kStep; }

// ---- the epilogues -------------------------------------------------------------------------------------------------------------------------
// block(c0, d0, d1): the scores of classes c0 .. c0 + 31 of the wave's pixel blocks 0 and 1 as the matrix unit leaves them; the class
// of register r is d_class(c0, lane, r).  done(): after the last block.  row: the first element of the item's output row y (of plane 0),
// x0 the wave's first column, ow and plane the elements of a row and of a plane.
struct Tile {
  int64_t row, plane;
  int x0, ow, C, lane;
};
__device__ inline int d_class(int c0, int lane, int r) { return c0 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3); }

// ArgmaxRule over a set of classes that need not begin at 0: idx < 0 until the first offer.
struct Candidate {
  float best;
  int idx;
  __device__ void offer(bool offered, int k, float v) {  // (& and |, not && and ||: selects, not branches — 32 of these follow every class block)
    const bool take = offered & ((idx < 0) | ((best == best) & ((v > best) | (v != v))));
    best = take ? v : best;
    idx = take ? k : idx;
  }
};
// The candidate of the union of two disjoint sets: the greater value, a NaN before any number, and of two equal values or two NaNs
// the lower class — each candidate being the lowest such class of its own set.
__device__ inline Candidate merged(const Candidate &a, const Candidate &b) {
  if (b.idx < 0) return a;
  if (a.idx < 0) return b;
  const bool an = a.best != a.best, bn = b.best != b.best;
  const bool take_b = (an || bn) ? (bn && (!an || b.idx < a.idx)) : (b.best > a.best || (b.best == a.best && b.idx < a.idx));
  return take_b ? b : a;
}

template <typename TOut> struct Scores {
  TOut *out;
  Tile t;
  __device__ Scores(void *o, const Tile &t_) : out((TOut *)o), t(t_) {}
  __device__ void block(int c0, const float16v &d0, const float16v &d1) {
    const int px = t.x0 + (t.lane & 31);
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int c = d_class(c0, t.lane, r);
      if (c >= t.C) continue;
      TOut *at = out + c * t.plane + t.row + px;
      if (px < t.ow) at[0] = to_elem<TOut>(d0[r]);
      if (px + 32 < t.ow) at[32] = to_elem<TOut>(d1[r]);
    }
  }
  __device__ void done() {}
};

// The lane's running candidates over the class blocks it is handed in ascending order, and after the last one the label of pixel
// `lane` of the wave; what stores it is the caller's.
struct LabelCandidates {
  Tile t;
  Candidate b0, b1;  // of the lane's classes, for its pixel of block 0 and of block 1
  __device__ LabelCandidates(const Tile &t_) : t(t_), b0{0.0f, -1}, b1{0.0f, -1} {}
  __device__ void block(int c0, const float16v &d0, const float16v &d1) {
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int c = d_class(c0, t.lane, r);
      b0.offer(c < t.C, c, d0[r]);
      b1.offer(c < t.C, c, d1[r]);
    }
  }
  // Lane l stores pixel l of the wave: its own candidate of block l / 32, merged with what lane l ^ 32 holds of the same pixel.
  __device__ int winner() {
    const bool hi = t.lane >= 32;
    const Candidate keep = hi ? b1 : b0, send = hi ? b0 : b1;
    const Candidate got = {__shfl_xor(send.best, 32), __shfl_xor(send.idx, 32)};
    return merged(keep, got).idx;
  }
};

// ---- host ----------------------------------------------------------------------------------------------------------------------------------
inline bool out_dtype_ok(int reduce, int dt) {
  return reduce == AA_BACK_VALUES ? float_dtype(dt) : (dt == AA_U8 || dt == AA_I16 || dt == AA_I32 || dt == AA_I64);
}
inline bool shape_ok(int64_t Q, int64_t C, int reduce) {
  return Q <= AA_BACK_QUERIES_MAX_Q && C >= 1 && C <= kAAManyMax && (reduce == AA_BACK_VALUES || reduce == AA_BACK_ARGMAX);
}
inline bool label_holds(int reduce, int out_dtype, int64_t C) {
  return reduce != AA_BACK_ARGMAX || !((out_dtype == AA_U8 && C > 256) || (out_dtype == AA_I16 && C > 32768));
}

// The wave tiles of a workgroup against the limit of the device the launches go to (the stream's; for the null stream the current one).
inline int tiles_lds(int Q, hipStream_t stream, unsigned *lds) {
  *lds = (unsigned)padded_q(Q) * 64u * (AA_BACK_TILE / 64) * (unsigned)sizeof(_Float16);
  hipDevice_t dev = 0;
  int limit = 0;
  if (hipStreamGetDevice(stream, &dev) != hipSuccess || hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) {
    (void)hipGetLastError();
    return AA_ERR_HIP;
  }
  return (int64_t)*lds > (int64_t)limit ? AA_ERR_BAD_SHAPE : AA_OK;
}

}  // namespace
