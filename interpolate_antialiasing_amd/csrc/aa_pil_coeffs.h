// aa_pil_coeffs.h — the filters and Pillow's precompute_coeffs + normalize_coeffs_8bpc for ONE output index, shared by the packed-table
// kernels (aa_tables.hip) and the ragged call's table arena (aa_many.hip), and — the window only — by the host planner of the ragged call
// (aa_many_plan computes every item's hull from it).  One place on purpose: one ulp in `center` or in the scale moves a window.
//
// Built with -ffp-contract=off: a fused multiply-add in `center`, `xmin` or the filter argument moves a window by one pixel (SURVEY §7
// "Weight parity").  Host and device evaluate the window in IEEE double, operation by operation, so they agree to the bit.
#pragma once

#include "aa_common.h"

namespace aa_coeffs {

// ---- filters (reference s2.2:292-300, :410-424, :367-372): argument type scalar_t, evaluated in double ----
template <typename S>
__device__ inline S filt_linear(S x) {
  if (x < 0.0) x = -x;
  if (x < 1.0) return (S)(1.0 - (double)x);
  return (S)0.0;
}
template <typename S>
__device__ inline S filt_cubic(S x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  const double xd = (double)x;
  // first branch: the double literals promote every operation to double
  if (x < 1.0) return (S)(((a + 2.0) * xd - (a + 3.0)) * xd * xd + 1);
  // second branch: `(((x - 5) * x + 8) * x - 4)` has only scalar_t and int operands, so the reference evaluates it
  // in scalar_t (float for float tensors); only the final `* a` is a double product
  if (x < 2.0) return (S)((double)(((x - (S)5) * x + (S)8) * x - (S)4) * a);
  return (S)0.0;
}
template <typename S>
__device__ inline S filt_box(S x) {
  return (x > -0.5 && x <= 0.5) ? (S)1.0 : (S)0.0;
}
// Pillow's Hamming and Lanczos (src/libImaging/Resample.c: sinc_filter, hamming_filter, lanczos_filter), evaluated in double from the
// scalar_t argument and narrowed to scalar_t.  Library sin / cos (not the fast intrinsics): the PIL kind must match Pillow's libm
// coefficients to the bit before they are quantised.
__device__ inline double sinc_d(double x) {
  if (x == 0.0) return 1.0;
  x = x * M_PI;
  return sin(x) / x;
}
template <typename S>
__device__ inline S filt_hamming(S xs) {
  double x = (double)xs;
  if (x < 0.0) x = -x;
  if (x == 0.0) return (S)1.0;
  if (x >= 1.0) return (S)0.0;
  x = x * M_PI;
  // Pillow writes the window constants as FLOAT literals (0.54f, 0.46f), promoted to double in the product
  return (S)(sin(x) / x * ((double)0.54f + (double)0.46f * cos(x)));
}
template <typename S>
__device__ inline S filt_lanczos(S xs) {
  const double x = (double)xs;
  if (-3.0 <= x && x < 3.0) return (S)(sinc_d(x) * sinc_d(x / 3.0));
  return (S)0.0;
}
template <typename S>
__device__ inline S apply_filter(int filter, S x) {
  switch (filter) {
    case AA_FILTER_LINEAR: return filt_linear<S>(x);
    case AA_FILTER_CUBIC: return filt_cubic<S>(x);
    case AA_FILTER_BOX: return filt_box<S>(x);
    case AA_FILTER_HAMMING: return filt_hamming<S>(x);
    case AA_FILTER_LANCZOS: return filt_lanczos<S>(x);
    default: return (S)0.0;  // (unreachable: aa_table_ksize rejects unknown ids before any launch)
  }
}

// Pillow: precompute_coeffs + normalize_coeffs_8bpc (src/libImaging/Resample.c, cited by URL in the reference:
// README.md:18,40; s2.2/aa_interpolation_impl.h:289-291).  double coefficients -> 22-bit fixed point int32.
// BoxArgs (Image.resize(box=...), precompute_coeffs's in0 / in1): the source interval of the axis and the origin of the hull the table
// indexes.  Pillow's C takes the box as FLOATS: in0 and in1 hold float values, and the scale is their float difference over the output
// size.  on == 0 (no box: in0 = 0, origin = 0): every expression below is the one it was before boxes existed (0.0 + x is exact).
struct BoxArgs { double in0, in1; int origin, on; };

// The window of output i: [xmin, xmin + xsize) in UNSHIFTED axis coordinates, clipped to [origin, origin + in_size), and the centre and
// the inverse filter scale its weights are evaluated with.
struct PilWindow { int xmin, xsize; double center, ss; };
// The two inputs of a window apart: the scale (from the whole axis or the box over the whole output size, never from a hull) and the
// interval [lo, hi) the window clips to.  pil_window below is this with both derived from in_size, as they were before they parted.
__host__ __device__ inline PilWindow pil_window_at(int i, int filter, double scale, double in0, int lo, int hi) {
  double filterscale = scale < 1.0 ? 1.0 : scale;
  const double fsupport = aa_filter_info(filter).support;
  const double support = fsupport * filterscale;
  const double center = in0 + ((double)i + 0.5) * scale;
  const double ss = 1.0 / filterscale;
  // windows clip to the hull [lo, hi): the hull is exactly the extreme windows clipped to the image, so this is Pillow's clip
  int xmin = (int)(center - support + 0.5);
  if (xmin < lo) xmin = lo;
  int xmax = (int)(center + support + 0.5);
  if (xmax > hi) xmax = hi;
  xmax -= xmin;
  return PilWindow{xmin, xmax, center, ss};
}
__host__ __device__ inline PilWindow pil_window(int i, int filter, int in_size, int out_size, const BoxArgs &bx) {
  double scale = bx.on ? (double)(float)(bx.in1 - bx.in0) / (double)out_size : (double)in_size / (double)out_size;
  return pil_window_at(i, filter, scale, bx.in0, bx.origin, bx.origin + in_size);
}
// The ksize int32 weights of that output (zero padded from xsize to ksize), computed from the unshifted xmin and centre.
__device__ inline void pil_weights(const PilWindow &wd, int filter, int ksize, int32_t *kk) {
  const int xmin = wd.xmin, xmax = wd.xsize;
  const double center = wd.center, ss = wd.ss;
  // two sweeps (sum, then normalise + quantise) so no per-thread array is needed
  double ww = 0.0;
  for (int x = 0; x < xmax && x < ksize; x++) ww += apply_filter<double>(filter, ((double)(x + xmin) - center + 0.5) * ss);
  int x = 0;
  for (; x < xmax && x < ksize; x++) {
    double k = apply_filter<double>(filter, ((double)(x + xmin) - center + 0.5) * ss);
    if (ww != 0.0) k /= ww;
    kk[x] = (k < 0) ? (int32_t)(-0.5 + k * (double)(1 << 22)) : (int32_t)(0.5 + k * (double)(1 << 22));
  }
  for (; x < ksize; x++) kk[x] = 0;
}

}  // namespace aa_coeffs
