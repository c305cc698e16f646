// aa_float_many_dev.h — the device code the kernels of the float ragged calls share (aa_embed_many.hip, aa_many_back.hip,
// aa_many_back_bwd.hip): the body of their table kernels, the reader of a table row, the element helpers, and the sum of sums over the
// classes of a pixel.  Each is written here once.  Device-only, and in the unnamed namespace like the kernels that use it and like
// aa_many_dev.h, which it builds on; for files built with -ffp-contract=off (aa_table_rows.h).  (What the hosts share: aa_float_many_host.h.)
// (Not here: aa_embed_many.hip's window_sums, the same sums over a vector of channels; why is at window_sums.)
#pragma once

#include "aa_many_dev.h"
#include "aa_table_rows.h"

namespace {

// ---- the table kernels' body ---------------------------------------------------------------------------------------------------------------
// One axis of one item: in_size resampled to out_size, the forward table (rows of ksize weights) at tab and, for a backward, its adjoint
// (rows of trk weights) at tr.
struct TableAxis {
  int in_size, out_size, ksize, trk;
  float scale;
  char *tab, *tr;
};

// What a workgroup of THREADS lanes does for its (item, axis): the rows of the forward table (table_build_f32_one), and with
// `adjoints`, after a barrier, the rows of its adjoint (table_transpose_one) — aa_table_rows.h's device functions, the ones
// aa_tables.hip runs, so the tables are the bits aa_table_build and aa_table_transpose give the shape.  A table's header is zeroed
// first: the row functions keep max_taps there.  Nobody reads that field back; the adjoint rows hold aa_table_transposed_ksize's
// estimate of entries, which the single-shape backward checks against the measured count and has never seen exceeded.  `adjoints` is
// uniform over the workgroup, and every lane of it comes here: there are barriers.  (With adjoints the kernels keep a few scalar
// registers in vector lanes across the two loops; nothing goes to scratch memory.)
template <int THREADS> __device__ inline void table_axis_build(TableAxis ax, int filter, int adjoints) {
  if (threadIdx.x < sizeof(aa_table_header) / 4) {
    ((int32_t *)ax.tab)[threadIdx.x] = 0;
    if (adjoints) ((int32_t *)ax.tr)[threadIdx.x] = 0;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < ax.out_size; i += THREADS) table_build_f32_one(i, filter, ax.in_size, ax.out_size, ax.ksize, ax.scale, ax.tab);
  if (!adjoints) return;
  __threadfence();
  __syncthreads();
  int32_t *tmin = (int32_t *)(ax.tr + aa_table_xmin_off()), *tsize = (int32_t *)(ax.tr + aa_table_xsize_off(ax.in_size));
  float *tw = (float *)(ax.tr + aa_table_w_off(ax.in_size));
  for (int x = threadIdx.x; x < ax.in_size; x += THREADS)
    table_transpose_one<float>(x, ax.tab, tmin, tsize, tw, &((aa_table_header *)ax.tr)->max_taps, ax.out_size, ax.ksize, ax.trk);
}

// ---- elements and table rows ---------------------------------------------------------------------------------------------------------------
__device__ inline float to_f32(float x) { return x; }
__device__ inline float to_f32(f16_t x) { return (float)x.v; }
__device__ inline float to_f32(bf16_t x) { return __uint_as_float((unsigned)x.v << 16); }

template <typename T, int V> struct alignas(sizeof(T) * V) Vec { T v[V]; };

// Row i of a table of out_size rows over an axis of in_size: the window [x0, x0 + n) and its weights.  Three rules, on which the bit
// contract and the bounds of every read rest: n is max(xsize, 1), as in aa_generic.hip (tap 0 is read unconditionally; a row without
// taps has weight 0 there); n is never more than a weight row holds; and the window is kept inside [0, in_size), so nothing outside an
// item's source is read (never moved in a built table: the tables clip their windows to the axis).  For an adjoint table in_size is the
// gradient's side and out_size the source's.
struct Row { int x0, n; const float *w; };
__device__ inline Row table_row(const char *tab, int in_size, int out_size, int ksize, int i) {
  const TableView<float> tv = make_table_view<float>(tab, out_size, ksize);
  int n = tv.xsize[i];
  n = n > 1 ? (n < ksize ? n : ksize) : 1;
  int x0 = tv.xmin[i];
  if (x0 > in_size - n) x0 = in_size - n;
  if (x0 < 0) x0 = 0;
  return {x0, n, tv.w + (size_t)i * ksize};
}

// ---- the sum of sums -----------------------------------------------------------------------------------------------------------------------
// V classes of one pixel from p: one vector (VEC: consecutive classes at an address that allows it) or V loads `sch` elements apart.
template <typename T, int V, bool VEC> __device__ inline void load_classes(const T *p, int64_t sch, float (&e)[V]) {
  if constexpr (VEC) {
    const Vec<T, V> r = *(const Vec<T, V> *)p;
#pragma unroll
    for (int c = 0; c < V; c++) e[c] = to_f32(r.v[c]);
  } else {
#pragma unroll
    for (int c = 0; c < V; c++) e[c] = to_f32(p[c * sch]);
  }
}

// acc = the vertical sum over ry's window of the horizontal sums over rx's window, for V classes from p = element (the lane's first
// class, row ry.x0, the pixel of tap 0 of rx); classes `sch` and rows `prow` elements apart, the pixel of tap k at k * ppx (a backward
// over a flipped item walks with ppx = -1).  hs is the fp32 intermediate of the two-pass form: tap 0 assigned, taps 1 .. n - 1 added in
// order, product and sum rounded apart.  The loops run over the taps: no array is sized by a longest row.  A weight is read once for
// the V classes.
template <typename T, int V, bool VEC>
__device__ inline void class_sums(const T *p, int64_t sch, int64_t prow, int64_t ppx, const Row &ry, const Row &rx, float (&acc)[V]) {
  for (int j = 0; j < ry.n; j++) {
    const T *rp = p + j * prow;
    float hs[V], e[V];
    load_classes<T, V, VEC>(rp, sch, e);
    const float w0 = rx.w[0];
#pragma unroll
    for (int c = 0; c < V; c++) hs[c] = e[c] * w0;
    for (int k = 1; k < rx.n; k++) {
      load_classes<T, V, VEC>(rp + k * ppx, sch, e);
      const float wk = rx.w[k];
#pragma unroll
      for (int c = 0; c < V; c++) hs[c] = hs[c] + e[c] * wk;
    }
    const float wj = ry.w[j];
#pragma unroll
    for (int c = 0; c < V; c++) acc[c] = j == 0 ? hs[c] * wj : acc[c] + hs[c] * wj;
  }
}

}  // namespace
