// aa_ycbcr.h — Pillow's "YCbCr" -> "RGB" conversion of one pixel (ConvertYCbCr.c: JFIF full range, 6 fractional bits), shared by the
// converting vertical pass of the ragged YCbCr call (aa_many_ycbcr.hip) and the host function aa_ycbcr_to_rgb_u8 (aa_api.hip), so the
// arithmetic the kernel compiles is checked on a CPU over all 2^24 triples (tests/test_resize_many_ycbcr_cpu.py).
// Pillow keeps four tables of 256 int16 entries; entry v of the table of coefficient c is
//   T_c[v] = (int)(c * 64 * (v - 128) + 0.5)          C's cast: it truncates towards zero, so neither floor nor rint
// with c a double, and  R = clip(Y + (T_1.402[Cr] >> 6)),  G = clip(Y + ((T_-0.34414[Cb] + T_-0.71414[Cr]) >> 6)),
// B = clip(Y + (T_1.772[Cb] >> 6)),  >> arithmetic.  The entries are computed, not looked up: c * 64 is a power-of-two scaling of c,
// the product with |v - 128| <= 128 is rounded once, and no product lies within 1e-4 of a half-integer (the fractions are multiples of
// 0.00032 or 0.008, none of which is 0.5), so neither the order of the two multiplications nor a fused multiply-add changes an entry.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#define AA_YCC_R_CR 1.402
#define AA_YCC_G_CB (-0.34414)
#define AA_YCC_G_CR (-0.71414)
#define AA_YCC_B_CB 1.772

__host__ __device__ inline int aa_ycc_term(double c, int v) { return (int)(c * 64.0 * (double)(v - 128) + 0.5); }
__host__ __device__ inline int aa_ycc_clip(int a) { return a < 0 ? 0 : (a > 255 ? 255 : a); }

// -> R | G << 8 | B << 16
__host__ __device__ inline uint32_t aa_ycbcr_to_rgb(int y, int cb, int cr) {
  const int r = aa_ycc_clip(y + (aa_ycc_term(AA_YCC_R_CR, cr) >> 6));
  const int g = aa_ycc_clip(y + ((aa_ycc_term(AA_YCC_G_CB, cb) + aa_ycc_term(AA_YCC_G_CR, cr)) >> 6));
  const int b = aa_ycc_clip(y + (aa_ycc_term(AA_YCC_B_CB, cb) >> 6));
  return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16);
}
