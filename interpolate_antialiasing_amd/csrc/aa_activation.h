// aa_activation.h — the activations of the ragged return path (aa_many_back.hip), device code: an fp32 exponential with a bit-exact
// definition, the sigmoid of one value, and the two passes of a softmax over the classes of one pixel.  The definition is the numpy
// restatement tests/activation_ref.py; this file states the same operations in the same order, every product and every sum rounded to
// float32 on its own.  So it may ONLY be included from files built with -ffp-contract=off -fno-fast-math (csrc/Makefile builds every file
// so): a fused multiply-add, a reassociated sum or a reciprocal in place of a division would change the bits.  The divisions are HIP's
// default correctly rounded fp32 division, and fp32 subnormal results are kept (gfx950's default mode), as numpy gives them.
// A NaN result is a NaN; its sign and payload are not part of the definition.  Device-only, in the unnamed namespace like its users.
#pragma once

#include <hip/hip_runtime.h>

namespace {

// exp(x) for x <= 0 or NaN: Cephes' expf specialised to that domain.  Softmax and sigmoid never need a positive argument.
//   NaN -> x + x;  x < -86 -> +0, so that n >= -124 and every non-zero result is a normal number;
//   n = rint(x * log2(e)), ties to even;  r = x - n * ln2 in two steps (hi then lo);  a degree-5 polynomial, Horner's form;
//   the result scaled by 2^n, a normal power of two built from its bits: an exact scaling.
// Over every float32 of [-86, 0] against float64 the largest error is 0.9916 ulp (tools/exp_sweep.py); aa_exp(0) is 1.0f.
__device__ inline float aa_exp(float x) {
  if (x != x) return x + x;
  if (x < -86.0f) return 0.0f;
  const float n = rintf(x * 1.44269504f);
  float r = x - n * 0.693359375f;
  r = r - n * -2.12194440e-4f;
  float p = 1.9875691500e-4f;
  p = p * r + 1.3981999507e-3f;
  p = p * r + 8.3334519073e-3f;
  p = p * r + 4.1665795894e-2f;
  p = p * r + 1.6666665459e-1f;
  p = p * r + 5.0000001201e-1f;
  const float y = ((p * r) * r + r) + 1.0f;
  return y * __int_as_float(((int)n + 127) << 23);
}

// 1 / (1 + exp(-v)) without a positive argument: e = aa_exp(-|v|), then e / (1 + e) below zero and 1 / (1 + e) from zero on, ONE
// correctly rounded division.  NaN -> NaN, +inf -> 1, -inf -> +0.
__device__ inline float aa_sigmoid(float v) {
  const float e = aa_exp(-fabsf(v));
  const float q = 1.0f + e;
  return (v >= 0.0f ? 1.0f : e) / q;
}

// Pass one of a pixel's softmax: the classes' values in ascending k through put(), an online maximum m and denominator d.  A new
// maximum rescales what was summed (d * aa_exp(m - v) + 1), anything else adds its term.  Then rcp(), ONE correctly rounded division
// (NaN where the maximum is +inf), and pass two: P_k = aa_exp(v_k - m) * rcp, the product rounded.  A NaN among the values, a +inf,
// or nothing but -inf makes d NaN or rcp NaN, so every class of the pixel NaN; a -inf beside finite values gets +0.
struct SoftmaxPass {
  float m, d;
  __device__ void put(int k, float v) {
    if (k == 0) {
      m = v;
      d = 1.0f;
      return;
    }
    const bool gt = v > m;
    const float e = aa_exp(gt ? m - v : v - m);
    d = gt ? d * e + 1.0f : d + e;
    m = gt ? v : m;
  }
  __device__ float rcp() const { return m == __builtin_inff() ? __builtin_nanf("") : 1.0f / d; }
};
// The product is an fp32 value of its own before anything rounds it further: where a float16 store follows directly, the compiler would
// otherwise fold product and conversion into one v_fma_mixlo_f16, which rounds the exact product ONCE to 16 bits — not the fp32 product
// rounded again, and a different float16 wherever the fp32 product lands on a tie.  The empty asm keeps the two roundings apart.
__device__ inline float aa_softmax_term(float v, float m, float rcp) {
  float p = aa_exp(v - m) * rcp;
  asm("" : "+v"(p));
  return p;
}

}  // namespace
