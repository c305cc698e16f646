// aa_many_dev.h — the device code the kernels of the ragged calls share (aa_many.hip, aa_many_maps.hip, aa_many_ycbcr.hip,
// aa_reduce_many.hip): the item of a work unit, the view of a window table with the clamp of a window to its hull, and the element
// types of the converting passes.  Each is written here once.  Device-only, and in the unnamed namespace like the kernels that use it:
// the element types are template arguments of kernels, whose names stay what they were per file.
// (Not here: aa_many.hip's vtap_sums and aa_many_ycbcr.hip's vwalk, the same sums; why is at vwalk.)
#pragma once

#include "aa_many.h"

namespace {

// The item whose work units hold `unit`: prefix[item] <= unit < prefix[item + 1].  `prefix[mid] <= unit` moves the lower end, so an item
// with no unit (equal neighbouring entries) is passed over.  Uniform per workgroup.
__device__ inline int aa_unit_item(const int64_t *prefix, int n, int64_t unit) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (prefix[mid] <= unit) lo = mid; else hi = mid;
  }
  return lo;
}

// A window table of `out` entries in the workspace: [ int32 xmin[out] ][ int32 xsize[out] ][ W w[out * ksize] ], xmin relative to the
// hull's origin; W is int32_t for the uint8 calls (aa_many.h) and double for the maps (aa_many_maps.h).
template <typename W> struct AATab {
  const int32_t *xmin, *xsize;
  const W *w;
  int ksize;
  __device__ int taps(int t) const { const int n = xsize[t]; return n > ksize ? ksize : n; }  // never more than a weight row holds
  __device__ const W *row(int t) const { return w + (size_t)t * ksize; }
};
template <typename W> __device__ inline AATab<W> aa_tab(const char *tab, int out, int ksize) {
  const int32_t *xmin = (const int32_t *)tab, *xsize = xmin + out;
  return {xmin, xsize, (const W *)(xsize + out), ksize};
}
// A window [x0, x0 + n) kept inside [0, hull): nothing outside an item's hull is read.
__device__ inline void aa_clamp_to_hull(int &x0, int &n, int hull) {
  if (x0 < 0) x0 = 0;
  if (x0 + n > hull) n = hull - x0;
}

__device__ inline uint32_t byte_of(uint32_t w, int q) { return (w >> (8 * q)) & 255u; }

// The element a converting pass stores: (T)a, rounded to nearest even once.
struct f16_t { _Float16 v; };
struct bf16_t { uint16_t v; };
template <typename T> __device__ inline T to_elem(float a);
template <> __device__ inline float to_elem<float>(float a) { return a; }
template <> __device__ inline f16_t to_elem<f16_t>(float a) { f16_t r; r.v = (_Float16)a; return r; }
template <> __device__ inline bf16_t to_elem<bf16_t>(float a) {
  const unsigned u = __float_as_uint(a);
  bf16_t r;
  if ((u & 0x7fffffffu) > 0x7f800000u) r.v = (uint16_t)((u >> 16) | 0x0040u);
  else r.v = (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
  return r;
}

}  // namespace
