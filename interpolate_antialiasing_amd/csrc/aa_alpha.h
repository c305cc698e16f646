// aa_alpha.h — Pillow's straight <-> premultiplied alpha conversions (RGBA <-> RGBa, LA <-> La) for one uint8 colour channel, as
// Image.resize applies them around the resampling of an RGBA / LA image.  Shared by the fused uint8 kernel (AA_FLAG_PREMUL_ALPHA
// instantiations) and the three-step fallback (aa_alpha.hip).  tests/test_alpha_cpu.py restates both, exhaustively.
#pragma once
#include <hip/hip_runtime.h>

// RGBA -> RGBa: t = c*a + 128, ((t >> 8) + t) >> 8.  For t < 2^16, ((t >> 8) + t) >> 8 == (t * 257) >> 16 (adding t / 256's fraction
// cannot carry past a multiple of 256), and t * 257 < 2^24: two 24-bit multiply-adds and a shift.
__device__ inline int aa_premul8(int c, int a) { return (int)(((unsigned)(c * a + 128) * 257u) >> 16); }

// RGBa -> RGBA: c where a is 0 or 255, else min(255, 255*c / a) with a truncating division.  c >= a gives 255 at once; otherwise
// n = 255*c < 65 025 and the quotient is < 255.  q = trunc(n * rcp(a)) is within one of the exact quotient for any reciprocal within a
// few ulp of 1/a (v_rcp_f32 is within 1), and one correction step against the remainder makes it exact.
__device__ inline int aa_unpremul8(int c, int a) {
  if (a == 0 || a == 255) return c;
  if (c >= a) return 255;
  const int n = 255 * c;
  int q = (int)((float)n * __builtin_amdgcn_rcpf((float)a));
  const int r = n - q * a;
  q += (r >= a ? 1 : 0) - (r < 0 ? 1 : 0);
  return q;
}

// one RGBA pixel (R in the low byte, straight alpha in the high byte) -> RGBa
__device__ inline unsigned aa_premul_px(unsigned px) {
  const int a = (int)(px >> 24);
  return (unsigned)aa_premul8((int)(px & 0xffu), a) | ((unsigned)aa_premul8((int)((px >> 8) & 0xffu), a) << 8) |
         ((unsigned)aa_premul8((int)((px >> 16) & 0xffu), a) << 16) | (px & 0xff000000u);
}

