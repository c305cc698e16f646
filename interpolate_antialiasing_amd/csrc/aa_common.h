// aa_common.h — shared host/device definitions for libaa_interp.so (gfx950 only; no CUDA paths).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/aa_interp.h"

#define AA_TABLE_MAGIC 0x42544141
#define AA_MAX_KSIZE 4096  // generic kernels loop over taps, so this only bounds sanity

// ---- filter properties: the one place host and device read them from -------------------------------------------------
// support in Pillow's units (Resample.c's filter structs); interp_size = 2 x support is what the float table kinds size windows by
// (the reference's interp_size for its three filters: 2 / 4 / 1); nonneg: no weight is ever negative, so the fused uint8 kernel's
// horizontal clip may be a plain shift (aa_fused_u8_v3_impl.h, NONNEG).  Hamming is non-negative on its support: sinc > 0 and
// 0.54 + 0.46 cos(pi x) >= 0.08 for |x| < 1; Keys cubic and Lanczos have negative lobes.
struct AAFilterInfo {
  double support;
  int interp_size;
  bool nonneg;
};
__host__ __device__ inline bool aa_filter_valid(int filter) { return filter >= AA_FILTER_LINEAR && filter <= AA_FILTER_LANCZOS; }
__host__ __device__ inline AAFilterInfo aa_filter_info(int filter) {
  switch (filter) {
    case AA_FILTER_LINEAR: return {1.0, 2, true};
    case AA_FILTER_CUBIC: return {2.0, 4, false};
    case AA_FILTER_BOX: return {0.5, 1, true};
    case AA_FILTER_HAMMING: return {1.0, 2, true};
    case AA_FILTER_LANCZOS: return {3.0, 6, false};
    default: return {0.0, -1, false};  // (callers check aa_filter_valid first)
  }
}
// both axes' filters non-negative: the fused uint8 kernel's NONNEG instantiations apply
__host__ __device__ inline bool aa_filters_nonneg(int filter_a, int filter_b) {
  return aa_filter_info(filter_a).nonneg && aa_filter_info(filter_b).nonneg;
}

// ---- four clipped sums in one dword --------------------------------------------------------------------
// Pillow's clip8(ss >> PRECISION_BITS) is ONE gfx950 instruction for two values: v_ashr_pk_u8_i32 D, S0, S1, sh
// writes D[7:0] = sat_u8(S0 >> sh), D[15:8] = sat_u8(S1 >> sh) and PRESERVES the other half of D (op_sel[3]=1
// targets D[31:16] instead) — measured on MI355X (tools/microbench/test_pk.hip).  Written as inline asm on purpose:
// ROCm 7.2's hipcc pattern-matches `clip(a)|clip(b)<<8` to this instruction but then treats the preserved upper
// half as zero when the 16-bit result is widened, which corrupts bytes 2-3 of a packed dword (found by the parity
// tests).  The form `r0 | r1 << 8 | r2 << 16 | r3 << 24` over four separately clipped values (the ragged call's
// plain vertical pass) is not matched and needs no asm.  VALU results are interlocked in hardware, so no manual wait
// states are needed around these.
__device__ inline unsigned pack4_clip8(int a0, int a1, int a2, int a3) {
  unsigned d;
  asm("v_ashr_pk_u8_i32 %0, %1, %2, 22\n\tv_ashr_pk_u8_i32 %0, %3, %4, 22 op_sel:[0,0,0,1]"
      : "=&v"(d)
      : "v"(a0), "v"(a1), "v"(a2), "v"(a3));
  return d;
}

// ---- packed table views --------------------------------------------------------------------------------
__host__ __device__ inline size_t aa_align16(size_t x) { return (x + 15) & ~(size_t)15; }
__host__ __device__ inline size_t aa_weight_elem_bytes(int kind) { return kind == AA_TABLE_F64 ? 8 : 4; }
__host__ __device__ inline size_t aa_table_xmin_off() { return sizeof(aa_table_header); }
__host__ __device__ inline size_t aa_table_xsize_off(int64_t out) { return sizeof(aa_table_header) + 4 * (size_t)out; }
__host__ __device__ inline size_t aa_table_w_off(int64_t out) {
  return aa_align16(sizeof(aa_table_header) + 8 * (size_t)out);
}
// end of the weight rows = start of the gather section
__host__ __device__ inline size_t aa_table_weights_end(int kind, int64_t out, int ksize) {
  return aa_align16(aa_table_w_off(out) + (size_t)out * (size_t)ksize * aa_weight_elem_bytes(kind));
}
// gather section (AA_TABLE_F32 and AA_TABLE_PIL tables; F32 also transposed): one 32-byte record per OUTPUT index
// {xmin, xsize, w[0..5]} — a table row in one scalar load for kernels whose vertical pass gathers (aa_fused_float_up_impl.h, the UPK mode of aa_fused_u8_v3_impl.h)
__host__ __device__ inline size_t aa_table_gather_bytes(int kind, int64_t out) { return (kind == AA_TABLE_F32 || kind == AA_TABLE_PIL) ? 32 * (size_t)out : 0; }
__host__ __device__ inline size_t aa_table_total_bytes(int kind, int64_t out, int ksize) {
  return aa_table_weights_end(kind, out, ksize) + aa_table_gather_bytes(kind, out);
}

template <typename WT>
struct TableView {
  const int32_t *xmin;
  const int32_t *xsize;
  const WT *w;
  int ksize;
};

template <typename WT>
__host__ __device__ inline TableView<WT> make_table_view(const void *table, int out_size, int ksize) {
  const char *p = (const char *)table;
  TableView<WT> v;
  v.xmin = (const int32_t *)(p + aa_table_xmin_off());
  v.xsize = (const int32_t *)(p + aa_table_xsize_off(out_size));
  v.w = (const WT *)(p + aa_table_w_off(out_size));
  v.ksize = ksize;
  return v;
}

// ---- experiment knobs ------------------------------------------------------------------------------------------------
// Environment variables are read by developer builds only (make TUNING=-DAA_V2_TUNING, tools/ab_build.sh): the shipped library
// never calls getenv, so its behaviour cannot depend on the ambient environment and a B = 1 call pays no lookups.
#include <stdlib.h>
#ifdef AA_V2_TUNING
inline const char *aa_knob(const char *name) { return getenv(name); }
#else
inline const char *aa_knob(const char *) { return nullptr; }
#endif
// store form of the up-scaling / backward kernel, set through aa_set_store_form() (tests force the streaming forms at small sizes):
// -1 automatic (by output size), 0 never streaming, 1 always streaming
extern int g_aa_store_form;
// plane groups of the fused uint8 kernel (aa_set_plane_groups): 1 = planar three-channel images run all three planes in one wave
extern int g_aa_plane_groups;

// ---- launch-error plumbing -------------------------------------------------------------------------------
#define AA_HIP_CHECK_LAUNCH()                 \
  do {                                        \
    if (hipGetLastError() != hipSuccess) return AA_ERR_HIP; \
  } while (0)

// entry points implemented in the .hip files and called from aa_api.cpp (the table builds' launcher: aa_box.h)
// bytes of the scatter section appended to AA_TABLE_PIL tables (0 when scatter_ksize == 0)
__host__ __device__ inline size_t aa_table_scatter_pitch(int kind) { return kind == AA_TABLE_F64 ? 64 : 32; }
__host__ __device__ inline size_t aa_table_scatter_bytes(int kind, int64_t in_size, int scatter_ksize) {
  // one record per input index + a sentinel: 8 ints (32-bit weights), or {int32 first, int32 cc, double w[6], pad} = 64 bytes
  return scatter_ksize > 0 ? aa_table_scatter_pitch(kind) * ((size_t)in_size + 1) : 0;
}
int aa_launch_table_transpose(const aa_table_header &h, const void *table_dev, void *tr_dev, int tr_ksize,
                              hipStream_t stream);

struct AAProblem {
  const void *in;
  void *out;
  void *ws;
  size_t ws_bytes;
  int dtype, layout;
  int64_t N, C, H, W, oH, oW;
  aa_axis ah, aw;
  hipStream_t stream;
  // decode-adjacent conversion (aa_resample_fwd_u8_to_f32): uint8 in, float32 out, optional layout change and per-channel
  // (v - mean) / std.  out_f32 == 0: the output has the input's dtype and layout.  out_elem: the float output's element type, AA_F32, or
  // AA_F16 / AA_BF16 (AA_FLAG_OUT_F16 / AA_FLAG_OUT_BF16): the same fp32 result rounded to nearest even once, at the store.
  int out_f32 = 0;
  int out_elem = AA_F32;
  int out_layout = AA_NCHW;
  int normalize = 0;
  float mean[4] = {0.f, 0.f, 0.f, 0.f};
  float std[4] = {1.f, 1.f, 1.f, 1.f};
  // strided input view (aa_resample_fwd_strided): rows are dense, but consecutive rows / images (channels_last) or planes (NCHW; n * C + c,
  // uniformly spaced) lie these many BYTES apart.  0 = the dense tensor.  Only the kernels that say so take pitched problems.
  int64_t in_row_pitch = 0, in_img_pitch = 0;
  int fast = 0;  // AA_FLAG_FAST: the caller accepts results within 1e-4 relative of the reference's (FMA accumulation)
  int alpha = 0;  // AA_FLAG_PREMUL_ALPHA: uint8, Pillow tables, C 2 / 4 with straight alpha last; only the kernels that say so take it
};

// generic two-launch separable path (always available); returns variant name through *variant
int aa_launch_generic_fwd(const AAProblem &p, const char **variant);
int aa_launch_axis_fwd(const void *in, void *out, int dtype, int64_t outer, int64_t in_size, int64_t inner, const aa_axis &ax,
                       hipStream_t stream);
size_t aa_generic_workspace_bytes(int dtype, int kind_w, int64_t N, int64_t C, int64_t H, int64_t oW);
int aa_launch_generic_convert(const AAProblem &p, const char **variant);  // u8 -> f32 (+ layout, normalisation), two launches
// (the fused single-launch families: aa_plan.h)
// the three-step straight-alpha fallback (aa_alpha.hip): premultiply a dense uint8 image of C = 2 / 4 channels (alpha last, either layout)
// into `dst`, and un-premultiply one in place
int aa_launch_premul_u8(const void *src, void *dst, int layout, int64_t N, int64_t C, int64_t H, int64_t W, hipStream_t stream);
int aa_launch_unpremul_u8(void *img, int layout, int64_t N, int64_t C, int64_t H, int64_t W, hipStream_t stream);
// Input pixels the windows (tw taps each) of one strip of <= 64 consecutive outputs cover, from the spread the table
// kernel MEASURED (header.span64p1; explicit scale factors and align_corners make it differ from 63 * in / out).
// -1 = unknown (a caller that did not fill aa_axis.span64p1): the fused kernels decline.
inline int aa_strip_span_px(const aa_axis &aw, int tw) { return aw.span64p1 > 0 ? aw.span64p1 + tw : -1; }
// the same for a strip of 32 outputs: 31 steps are at most 11 runs of 3 steps, each bounded by the measured spread of 4
// neighbouring window starts (span4p1), and never more than the spread of 64
inline int aa_strip_span_px32(const aa_axis &aw, int tw) {
  if (aw.span64p1 <= 0 || aw.span4p1 <= 0) return -1;
  const int by4 = 11 * (aw.span4p1 - 1) + 1;
  return (by4 < aw.span64p1 ? by4 : aw.span64p1) + tw;
}
// ... and for a strip of 16 outputs (split windows: four lanes per pixel): 15 steps are 5 runs of 3
inline int aa_strip_span_px16(const aa_axis &aw, int tw) {
  if (aw.span64p1 <= 0 || aw.span4p1 <= 0) return -1;
  const int by4 = 5 * (aw.span4p1 - 1) + 1;
  return (by4 < aw.span64p1 ? by4 : aw.span64p1) + tw;
}
// (row bands never exceed 64, so a grid of `units * 64` workgroups bounds every launch)
inline bool aa_grid_fits(int64_t units) { return units > 0 && units <= (int64_t)0x7FFFFFFF / 64 - 8; }
// CU count of the current device (cached); 256 on MI355X
int aa_device_cu_count();
// Resident workgroups per CU of `kern` at `threads` threads and `lds` bytes of dynamic LDS, cached per (kernel, device,
// threads, lds) behind a mutex, one cache of 256 entries per `family` (aa_launch_family) — the occupancy query costs microseconds,
// and a B = 1 call is ~10 us end to end.  -1 when the query fails (the launch-shape model, aa_launch_shape.h, falls back to an
// estimate; it only feeds launch-shape heuristics, never results).
int aa_resident_blocks(int family, const void *kern, int threads, size_t lds);
// Launch shape of a fused family's kernel for problem q (aa_launch_shape.h); occupancy from aa_resident_blocks of `kern`, `lds` bytes a strip
aa_launch_shape_out aa_kernel_launch_shape(int family, const void *kern, int nstrips, int spb, int spb_forced, int64_t items, const AAProblem &q,
                                           size_t lds, const int *tag = nullptr, int saturation = 0, int threads = 0);

int aa_launch_probe_copy(const void *src, void *dst, size_t bytes, int form, hipStream_t stream);
// scatter-add adjoint
int aa_launch_bwd_atomic(const AAProblem &p);
