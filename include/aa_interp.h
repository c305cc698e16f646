/*
 * aa_interp.h — C-ABI of libaa_interp.so: MI355X (gfx950) antialiased separable resample.
 *
 * This is the drop-in boundary for the reference's hot path.  The reference binds the path through a
 * pybind11 module (step_two_dot_two/extension_interpolate.cpp:46-51: linear_forward, nearest_forward,
 * cubic_forward, linear_backward; step_three/extension_interpolate.cpp:17-19: forward); a maintainer
 * replaces the bodies of those four wrappers (s2.2/extension_interpolate.cpp:7-42) with calls to the entry
 * points below (INTEGRATION.md shows the stub).  Plain pointers and sizes only: no torch/ATen types.
 *
 * Conventions
 *   - every pointer named *_dev is a DEVICE pointer (HBM); the caller allocates everything (outputs,
 *     tables, workspace); nothing here allocates, frees or synchronises unless its comment says so;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); all work is enqueued on it;
 *   - tensors are 4-D (N,C,H,W) in one of two dense layouts: AA_NCHW (contiguous) or AA_NHWC
 *     (torch.channels_last storage); the output uses the same layout as the input
 *     (s2.2/aa_interpolation_impl.h:752 `suggest_memory_format`);
 *   - return value: 0 on success, a negative aa_status otherwise (aa_strerror() gives the text).
 */
#ifndef AA_INTERP_H
#define AA_INTERP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AA_INTERP_ABI_VERSION 3 /* 3: aa_resample_fwd_ex (flags), aa_resample_fwd_strided, aa_set_store_form, aa_convert.flags; every other
                                   v2 entry point unchanged.  Added since without a version change (additive; a caller looks the
                                   symbol up): aa_back_many_desc_bytes, aa_back_many_plan, aa_resample_back_many, with aa_back_item
                                   and the aa_dtype values AA_I16 .. AA_BOOL that only they take; aa_back_many_bwd_desc_bytes,
                                   aa_back_many_bwd_plan, aa_resample_back_many_bwd, with aa_back_bwd_item; aa_back_merged_desc_bytes,
                                   aa_back_merged_plan, aa_resample_back_merged; aa_back_many_plan_act, aa_back_merged_plan_act
                                   (a softmax or sigmoid before the reduction), with AA_BACK_ACT_* */

typedef void *aa_stream_t; /* hipStream_t */

enum aa_status {
  AA_OK = 0,
  AA_ERR_BAD_FILTER = -1,    /* unknown filter id */
  AA_ERR_BAD_DTYPE = -2,     /* dtype / table-kind combination not implemented ("... not implemented for 'X'") */
  AA_ERR_BAD_LAYOUT = -3,
  AA_ERR_BAD_SHAPE = -4,     /* non-positive sizes (upsample_2d_common_check), table/shape mismatch */
  AA_ERR_NULL = -5,
  AA_ERR_WORKSPACE = -6,     /* workspace smaller than aa_workspace_bytes() */
  AA_ERR_KSIZE = -7,         /* ksize beyond what the kernels support */
  AA_ERR_HIP = -8,           /* a HIP runtime call failed (launch error) */
  AA_ERR_NO_DEVICE = -9,
  AA_ERR_STRIDES = -10       /* aa_resample_fwd_strided: this view needs a dense copy (make one and call aa_resample_fwd) */
};

/* Filters: s2.2/aa_interpolation_impl.h:292-300 (triangle), :410-424 (Keys cubic a=-0.5), :367-372 (box;
 * the reference binds it as "nearest_forward": "it's not nearest but box", extension_interpolate.cpp:48), and Pillow's other two
 * antialiasing filters (src/libImaging/Resample.c): Hamming-windowed sinc (support 1) and Lanczos-3 (support 3, negative lobes).
 * The float table kinds size their windows from interp_size = 2 x support, as the reference does for its three filters.
 * Hamming and Lanczos were added without an ABI version change (the change is additive): a caller detects a library that predates
 * them because aa_table_ksize() returns AA_ERR_BAD_FILTER for ids 3 and 4. */
enum aa_filter { AA_FILTER_LINEAR = 0, AA_FILTER_CUBIC = 1, AA_FILTER_BOX = 2, AA_FILTER_HAMMING = 3, AA_FILTER_LANCZOS = 4 };

/* Element type of the image tensors. */
enum aa_dtype { AA_U8 = 0, AA_F32 = 1, AA_F64 = 2, AA_F16 = 3, AA_BF16 = 4,
                /* what aa_back_many_plan stores besides: labels and masks, never an image's element (AA_ERR_BAD_DTYPE everywhere else) */
                AA_I16 = 5, AA_I32 = 6, AA_I64 = 7, AA_BOOL = 8 };
/* AA_F16 / AA_BF16 (the reference dispatches float and double only): AA_TABLE_F32 tables, fp32
 * arithmetic in the reference's order, fp32 intermediate between the passes, ONE round-to-nearest-even at the store —
 * i.e. exactly  half(reference_fp32(float(x))). */

enum aa_layout { AA_NCHW = 0, AA_NHWC = 1 };

/* Arithmetic a weight table is built in (replaces HelperInterpBase::_compute_indices_weights_aa,
 * s2.2/aa_interpolation_impl.h:195-281):
 *   AA_TABLE_F32   the reference's scalar_t=float promotions, float weights   (f32 images; u8 "harness" mode)
 *   AA_TABLE_F64   scalar_t=double                                            (f64 images)
 *   AA_TABLE_PIL   Pillow's precompute_coeffs + normalize_coeffs_8bpc: double coefficients, int32 weights in
 *                  22-bit fixed point (u8 images, bit-exact with PIL.Image.resize; SURVEY §8 a-U)         */
enum aa_table_kind { AA_TABLE_PIL = 0, AA_TABLE_F32 = 1, AA_TABLE_F64 = 2 };

/* ---- packed weight table (one flat device buffer = one RCCL broadcast payload) -------------------------
 *   [ aa_table_header : 64 B ][ int32 xmin[out] ][ int32 xsize[out] ][ pad to 16 B ][ weight w[out*ksize] ]
 * weight = float (F32), double (F64) or int32 (PIL).  Rows are zero-padded from xsize to ksize (s2.2:276-278). */
typedef struct aa_table_header {
  int32_t magic;         /* 'AATB' 0x42544141 */
  int32_t filter;        /* aa_filter */
  int32_t kind;          /* aa_table_kind */
  int32_t in_size;
  int32_t out_size;
  int32_t ksize;         /* row pitch of w, = (int)ceilf(support)*2+1 (s2.2:210) */
  int32_t align_corners;
  int32_t max_taps;      /* max_i xsize[i], filled by the device kernel */
  int32_t transposed;    /* 1 for an adjoint (backward) table built by aa_table_transpose */
  int32_t scatter_off;   /* byte offset of the scatter section (0 = none), see below */
  int32_t scatter_ksize; /* row pitch of the scatter weights */
  int32_t scatter_max;   /* max outputs fed by one input index, filled by the device kernel */
  int32_t span64p1;      /* 1 + max_i (xmin[min(i+63,out-1)] - xmin[i]): how far the window starts of 64 consecutive outputs
                            spread, measured by the device kernel from the table itself (explicit scale factors and
                            align_corners make it differ from 63*in/out); 0 = not measured */
  int32_t span4p1;       /* the same over 4 consecutive outputs: 1 + max_i (xmin[min(i+3,out-1)] - xmin[i]) (kernels in which
                            a lane computes 4 neighbouring outputs from one shared window) */
  int32_t gather_off;    /* byte offset of the gather section (AA_TABLE_F32 and AA_TABLE_PIL tables; 0 = none): one 32-byte record per OUTPUT index,
                            { int32 xmin, int32 xsize, float w[6] } = a table row in one scalar load (rows wider than 6 taps keep
                            their full weights in w[] above) */
  int32_t reserved[1];
} aa_table_header;
/* Scatter section (every table kind), used by the fused kernels whose vertical pass runs in registers: one record per INPUT
 * index x (in_size + 1 records; the last is an all-zero sentinel a reader may prefetch).  AA_TABLE_PIL / AA_TABLE_F32: 32-byte
 * records { int32 first, int32 count | completes << 16, int32 (PIL) or float (F32) w[6] }; AA_TABLE_F64: 64-byte records
 * { int32 first, int32 count | completes << 16, double w[6], 8 bytes of padding }.  first = the first output whose window ends at or after
 * x; first .. first+count-1 = the outputs whose window holds x, w[k] = weight[first+k][x - xmin[first+k]] (zero
 * padded); completes = how many outputs, starting at `first`, have x as the LAST index of their window (they can be
 * emitted once x has been absorbed).  Present only when count <= 6 everywhere. */

/* Host-side description of one axis handed to the resample calls. */
typedef struct aa_axis {
  const void *table_dev; /* packed table in HBM */
  int32_t in_size;
  int32_t out_size;
  int32_t ksize;
  int32_t max_taps;      /* from aa_table_query(); 0 = unknown (kernels then use ksize) */
  int32_t kind;          /* aa_table_kind */
  int32_t filter;        /* aa_filter */
  int32_t scatter_off;   /* from the table header (aa_table_query); 0 = no scatter section */
  int32_t scatter_ksize;
  int32_t scatter_max;
  int32_t span64p1;      /* from the table header; 0 = unknown: the fused single-launch kernels then decline (they size
                            their staged row segments from it) and the generic two-launch path runs */
  int32_t span4p1;       /* from the table header; 0 = unknown */
  int32_t gather_off;    /* from the table header; 0 = no gather section */
  int32_t reserved[2];   /* reserved[0] = 1 for a table from aa_table_build_box: in_size is the hull's length, and equal sizes in and out
                            do not mean "nothing to do"; 0 otherwise.  reserved[1] = 0 */
} aa_axis;

/* Version / diagnostics. */
int aa_abi_version(void);
const char *aa_strerror(int status);
/* Number of visible HIP devices (0 on a CPU-only host; never throws). */
int aa_device_count(void);

/* ksize for (filter, kind, in, out): host arithmetic with the reference's promotions (s2.2:207-210), or
 * Pillow's for AA_TABLE_PIL.  scale<=0: scale derived from sizes (area_pixel_compute_scale, call site
 * s2.2:314-315).  Returns ksize (>0) or a negative aa_status. */
int aa_table_ksize(int filter, int kind, int64_t in_size, int64_t out_size, int align_corners, double scale);
/* Bytes of the packed table for (kind, out_size, ksize) without a scatter section (transposed tables); AA_TABLE_F32
 * and AA_TABLE_PIL tables include their gather section (32 bytes per output index). */
size_t aa_table_bytes(int kind, int64_t out_size, int ksize);
/* Bytes aa_table_build() needs for this table (AA_TABLE_PIL tables carry a scatter section as well). */
size_t aa_table_build_bytes(int filter, int kind, int64_t in_size, int64_t out_size, int align_corners, double scale);

/* Build a packed table ON DEVICE (one thread per output index).  Asynchronous on `stream`. */
int aa_table_build(int filter, int kind, int64_t in_size, int64_t out_size, int align_corners, double scale,
                   void *table_dev, size_t table_bytes, aa_stream_t stream);

/* Upper bound for the ksize of the adjoint of a table (host arithmetic only). */
int aa_table_transposed_ksize(int filter, int kind, int64_t in_size, int64_t out_size, int align_corners, double scale);
/* Build the adjoint (gather-form) table of `table_dev` on device: for every INPUT index x, the contiguous
 * range of outputs whose window holds x and their weights.  The result is a packed table whose in_size/out_size
 * are swapped, usable with aa_resample_fwd to compute the TRUE adjoint (what test.py:387-398 asks for; the
 * reference's own backward header is non-AA).  F32/F64 kinds only.  Table-build time: reads the forward header before
 * and the new header after the launch (two synchronisations).  header.max_taps of the result is the widest range FOUND; rows of
 * tr_ksize entries that cannot hold it would drop gradient taps, so that is AA_ERR_KSIZE and the table must not be used. */
int aa_table_transpose(const void *table_dev, void *tr_table_dev, size_t tr_table_bytes, int tr_ksize,
                       aa_stream_t stream);

/* Copy a table header back to the host.  SYNCHRONISES `stream` (one-off, at table-build time, never in the
 * per-call path). */
int aa_table_query(const void *table_dev, aa_table_header *host_header, aa_stream_t stream);
/* aa_table_build for the two tables of a call (H and W axis: same filter, kind and align_corners) as ONE launch. */
int aa_table_build2(int filter, int kind, int align_corners, int64_t in_a, int64_t out_a, double scale_a, void *table_a_dev, size_t bytes_a,
                    int64_t in_b, int64_t out_b, double scale_b, void *table_b_dev, size_t bytes_b, aa_stream_t stream);
/* aa_table_query for the two tables of a call (H and W axis) with ONE synchronisation: a shape never seen before costs two table builds, and a
 * data pipeline of random crops meets a new shape on every call. */
int aa_table_query2(const void *table_a_dev, const void *table_b_dev, aa_table_header *host_a, aa_table_header *host_b, aa_stream_t stream);

/* ---- box tables: Pillow's Image.resize(box=...) ------------------------------------------------------------------------------------
 * Pillow's precompute_coeffs(inSize, in0, in1, outSize) resamples the sub-pixel source interval [in0, in1) of an axis: scale =
 * (float)(in1 - in0) / out (Pillow's C takes the box as floats: pass float values in the doubles), centre of output i = in0 + (i + 0.5) * scale, windows clipped to the whole axis [0, inSize).  The windows of all
 * outputs together cover the HULL [origin, origin + hull) = [xmin of output 0, end of the last output's window); the caller computes it
 * (the same double arithmetic) and hands the resample calls the hull as a view of the image (aa_resample_fwd_strided; rows and columns
 * outside the hull are never read).  A box table is an ordinary packed table whose in_size is `hull` and whose xmin[] are relative to
 * `origin`; centres and weights are computed from the UNSHIFTED in0, and clipping to the hull equals clipping to the image because the
 * hull is exactly the extreme windows.  AA_TABLE_PIL only (the reference has no box): other kinds AA_ERR_BAD_DTYPE.  in0 = 0, in1 =
 * inSize, origin = 0, hull = inSize gives aa_table_build's table bit for bit.  Set aa_axis.reserved[0] = 1 for such a table. */
/* ksize of a box table (host arithmetic), or a negative aa_status.  hull: the table's in_size. */
int aa_table_ksize_box(int filter, int kind, int64_t hull, int64_t out_size, double in0, double in1);
/* Bytes aa_table_build_box needs for one such table. */
size_t aa_table_build_bytes_box(int filter, int kind, int64_t hull, int64_t out_size, double in0, double in1);
/* Build the two box tables of a call (a: the H axis, b: the W axis; an axis without a box passes in0 = 0, in1 = inSize, origin = 0)
 * as ONE launch (very large tables — a hull beyond 32768 or an output beyond 16384 — one after the other, as aa_table_build2 does); aa_table_query2 then reads both headers with one synchronisation.  Asynchronous on `stream`. */
int aa_table_build_box(int filter, int kind, int64_t origin_a, int64_t hull_a, int64_t out_a, double in0_a, double in1_a, void *table_a_dev,
                       size_t bytes_a, int64_t origin_b, int64_t hull_b, int64_t out_b, double in0_b, double in1_b, void *table_b_dev,
                       size_t bytes_b, aa_stream_t stream);

/* Workspace (bytes) the forward needs for this problem; 0 when a fused single-launch path applies.  The answer depends on the
 * shape and the tables only, never on the pointers: which kernel runs is decided from the same facts, and a uint8 view that starts
 * on an odd byte is served by the same kernels (byte stores instead of dword stores).  Tensors of 2 / 4 / 8-byte elements must
 * start on an element boundary (AA_ERR_BAD_SHAPE otherwise). */
size_t aa_workspace_bytes(int dtype, int layout, int64_t N, int64_t C, int64_t H, int64_t W, int64_t oH, int64_t oW,
                          const aa_axis *ax_h, const aa_axis *ax_w);
/* The same for aa_resample_fwd_ex with `flags` (AA_FLAG_PREMUL_ALPHA changes the answer; without it this is aa_workspace_bytes). */
size_t aa_workspace_bytes_ex(int dtype, int layout, int64_t N, int64_t C, int64_t H, int64_t W, int64_t oH, int64_t oW,
                             const aa_axis *ax_h, const aa_axis *ax_w, unsigned flags);

/* Forward: replaces ti_upsample_{bilinear,bicubic,nearest}2d_cpu + the separable driver + both passes
 * (s2.2/aa_interpolation_impl.h:731-807, :628-683, :536-625, :131-187, :29-120).
 *   in_dev  [N,C,H,W]  dtype/layout as given          out_dev [N,C,oH,oW] same dtype/layout
 *   ax_w: table for W -> oW (first pass, like the reference and PIL); ax_h: H -> oH (second pass).
 * Table kind selects the arithmetic: F32/F64 tables with f32/f64 images (bit-comparable with the reference's
 * CPU path: separately rounded product and sum, taps in order); u8 images with AA_TABLE_PIL tables give
 * Pillow's integer result; u8 images with AA_TABLE_F32 tables give the reference harness semantics
 * (test.py:52-58,72,75: float(), fp32 op, bicubic clamp, truncating byte()).
 * Empty batch (N==0) is allowed (s2.2:747-750).  Asynchronous on `stream`. */
int aa_resample_fwd(const void *in_dev, void *out_dev, void *workspace_dev, size_t workspace_bytes, int dtype,
                    int layout, int64_t N, int64_t C, int64_t H, int64_t W, const aa_axis *ax_h, const aa_axis *ax_w,
                    aa_stream_t stream);

/* The same with flags.  AA_FLAG_FAST — the opt-in TOLERANCE mode for f32 / f16 / bf16 images: the caller accepts results within
 * 1e-4 relative of the reference's (BASELINE.json's float bar) instead of bit-identical ones, and the fused kernels then accumulate
 * with fused multiply-adds over zero-padded windows (no separately rounded product and sum, no per-position select).  Differences
 * are rounding only (~1e-7 relative); a NaN / Inf input value additionally poisons every output whose 16-byte-aligned window
 * holds it (0 * inf), not only those whose taps do.  u8 images with AA_TABLE_F32 tables (the harness's float arithmetic) have the
 * mode too: FMAs in both passes, so the truncated byte may differ from the exact mode's by one count.  Ignored for Pillow's integer
 * arithmetic, for f64 images and wherever no tolerance kernel applies (the exact kernels run: bit-identical results are always
 * within tolerance).  aa_workspace_bytes() answers for both. */
#define AA_FLAG_FAST 1u
/* AA_FLAG_PREMUL_ALPHA — resize an image with STRAIGHT alpha the way Pillow's Image.resize does for RGBA / LA: the colour channels are
 * premultiplied by alpha (RGBA -> RGBa: t = c*a + 128, c' = ((t >> 8) + t) >> 8), the premultiplied image is resampled, and every
 * output pixel is converted back (c' = c where a is 0 or 255, else min(255, 255*c / a), truncating); alpha itself resamples as an
 * ordinary channel.  Bit-exact with Pillow.  Only for uint8 images with AA_TABLE_PIL tables and C == 2 or 4, the last channel being
 * alpha, in either layout; any other combination returns AA_ERR_BAD_DTYPE.  Output size == input size copies the input unchanged
 * (Pillow returns a copy).  Channels_last RGBA with narrow windows and shrinking heights runs fused in one launch; everything else
 * premultiplies into the workspace, resamples, and un-premultiplies the output in place (aa_workspace_bytes_ex answers for it;
 * aa_resample_fwd_strided has no workspace and returns AA_ERR_STRIDES there).  A library that predates this flag rejects it as an
 * unknown flag bit (AA_ERR_BAD_SHAPE): the ABI version stays 3. */
#define AA_FLAG_PREMUL_ALPHA 2u
int aa_resample_fwd_ex(const void *in_dev, void *out_dev, void *workspace_dev, size_t workspace_bytes, int dtype,
                       int layout, int64_t N, int64_t C, int64_t H, int64_t W, const aa_axis *ax_h, const aa_axis *ax_w,
                       unsigned flags, aa_stream_t stream);

/* Forward over a STRIDED VIEW of a larger tensor, without a copy: the reference walks arbitrary strides through TensorIterator
 * (s2.2/aa_interpolation_impl.h:555-559), and the views a data pipeline produces — a crop x[:, :, y0:y1, x0:x1] (RandomResizedCrop),
 * a batch slice — are read here where they lie.  in_strides = the view's strides in ELEMENTS for (N, C, H, W).  Served: rows of
 * consecutive elements (AA_NCHW: stride_W = 1; AA_NHWC: stride_C = 1, stride_W = C), any row pitch, planes n * C + c uniformly spaced
 * (AA_NCHW: stride_N = C * stride_C; AA_NHWC: any stride_N), and a shape one of the fused single-launch kernels takes (no workspace).
 * Anything else returns AA_ERR_STRIDES: make a dense copy and call aa_resample_fwd.  The output is dense, in `layout`. */
int aa_resample_fwd_strided(const void *in_dev, void *out_dev, int dtype, int layout, int64_t N, int64_t C, int64_t H, int64_t W,
                            const int64_t *in_strides, const aa_axis *ax_h, const aa_axis *ax_w, unsigned flags, aa_stream_t stream);

/* Decode-adjacent forward: uint8 image in, float tensor out (float32; float16 / bfloat16 on request), ONE launch.  Replaces what the reference's harness
 * does around the op on the CPU — np.asarray(pil) -> transpose(2,0,1) -> .float() -> op (test.py:337-339,55; README.md:416
 * prices those conversions at 0.33 of 2.27 ms) — and, optionally, the per-channel normalisation that follows in a data
 * loader.  out = op(float(in)) in the reference's fp32 arithmetic (AA_TABLE_F32 tables; bit-identical to aa_resample_fwd on
 * the converted tensor), written in cv->out_layout, which may differ from the input's; with cv->normalize,
 * out = (out - mean[c]) / std[c] in fp32 (C <= 4).  in_dev [N,C,H,W] uint8 in `layout`; out_dev [N,C,oH,oW] float32.
 *
 * AA_FLAG_OUT_F16 / AA_FLAG_OUT_BF16 (valid in aa_convert.flags ONLY; aa_resample_fwd_ex and aa_resample_fwd_strided reject them as
 * unknown bits): out_dev holds 2-byte elements, float16 or bfloat16, what a model trained in 16-bit precision reads.  The result is
 * round_to_nearest_even_16(f32_result), f32_result being exactly what the call writes without the bit, normalisation included: fp32
 * arithmetic, fp32 normalisation, ONE rounding at the store (the convention of AA_F16 / AA_BF16 images above) — and no float32 tensor
 * written and read again by a cast.  With neither bit the output is float32.  Both bits: AA_ERR_BAD_DTYPE.  out_dev must be aligned to
 * its element (2 bytes; 4 for float32), AA_ERR_BAD_SHAPE otherwise; an output that is only 2-byte aligned, or whose rows are an odd
 * number of elements, is served by the same kernels (2-byte stores instead of paired ones), so aa_workspace_bytes_u8_to_f32 does not
 * depend on the pointer.  A library that predates these bits rejects them as unknown flag bits (AA_ERR_BAD_SHAPE): the ABI version
 * stays 3. */
#define AA_FLAG_OUT_F16 4u
#define AA_FLAG_OUT_BF16 8u
typedef struct aa_convert {
  int32_t out_layout; /* aa_layout of the float output */
  int32_t normalize;  /* 0: raw op result */
  float mean[4];
  float std[4];
  uint32_t flags;     /* 0, or any of: AA_FLAG_FAST, the tolerance mode (fused multiply-adds; results within 1e-4 relative of the exact
                         mode's); AA_FLAG_OUT_F16 or AA_FLAG_OUT_BF16, the output's element type (see above) */
} aa_convert;
size_t aa_workspace_bytes_u8_to_f32(int layout, int64_t N, int64_t C, int64_t H, int64_t W, const aa_axis *ax_h, const aa_axis *ax_w,
                                    const aa_convert *cv);
int aa_resample_fwd_u8_to_f32(const void *in_dev, void *out_dev, void *workspace_dev, size_t workspace_bytes, int layout,
                              int64_t N, int64_t C, int64_t H, int64_t W, const aa_axis *ax_h, const aa_axis *ax_w,
                              const aa_convert *cv, aa_stream_t stream);

/* Backward (true adjoint): grad_in[N,C,H,W] = H^T V^T grad_out[N,C,oH,oW].  Replaces
 * ti_upsample_bilinear2d_backward_cpu (s2.2/aa_interpolation_backward_impl.h:185-219) in API shape.
 * tr_h / tr_w are TRANSPOSED tables from aa_table_transpose (gather form: deterministic, no atomics, no zero fill).
 * dtype: AA_F32 (AA_TABLE_F32 tables), AA_F64 (AA_TABLE_F64), and AA_F16 / AA_BF16 gradients with transposed AA_TABLE_F32 tables, which
 * follow the convention of AA_F16 / AA_BF16 images above: grad_in = round_to_nearest_even_16(adjoint_fp32(float(grad_out))), fp32
 * arithmetic in the fp32 backward's own order, fp32 intermediate between the passes, ONE rounding at the store; bit for bit the fp32
 * call's result cast to 16 bits, on every route.  Any other dtype / table kind: AA_ERR_BAD_DTYPE (the answer of a library older than
 * this addition to 16-bit gradients; the ABI version is unchanged, the change is additive).  Workspace: aa_workspace_bytes(dtype, layout,
 * N, C, oH, oW, H, W, tr_h, tr_w), as for the forward this call is. */
int aa_resample_bwd(const void *grad_out_dev, void *grad_in_dev, void *workspace_dev, size_t workspace_bytes, int dtype,
                    int layout, int64_t N, int64_t C, int64_t H, int64_t W, const aa_axis *tr_h, const aa_axis *tr_w,
                    aa_stream_t stream);
/* Scatter form of the same adjoint with fp32/fp64 atomics straight from the FORWARD tables (BASELINE config 5
 * names it); grad_in is zero-filled first by the call.  Results agree with aa_resample_bwd to rounding only.
 * AA_F32 / AA_F64 only: AA_F16 / AA_BF16 gradients are AA_ERR_BAD_DTYPE here.  Atomic adds that round to 16 bits one by one are a
 * different and worse result than one rounding of the fp32 sum; an fp32 scatter followed by a cast is this call in AA_F32. */
int aa_resample_bwd_atomic(const void *grad_out_dev, void *grad_in_dev, void *workspace_dev, size_t workspace_bytes,
                           int dtype, int layout, int64_t N, int64_t C, int64_t H, int64_t W, const aa_axis *ax_h,
                           const aa_axis *ax_w, aa_stream_t stream);
size_t aa_workspace_bytes_bwd(int dtype, int layout, int64_t N, int64_t C, int64_t H, int64_t W, int64_t oH, int64_t oW);

/* One separable pass along one axis of a dense array viewed as [outer][in_size][inner] -> [outer][out_size][inner]
 * (the body the reference instantiates per dimension, `_ti_separable_upsample_generic_Nd_kernel_impl_single_dim`
 * s2.2/aa_interpolation_impl.h:536-625, "NCHW, NCL or NCKHW" :545).  The N-d front-ends (1-D NCL, 3-D NCDHW) are this
 * call once per resampled axis, last axis first like the reference (:658); no workspace.  dtype/table-kind pairs as
 * for aa_resample_fwd except u8 with AA_TABLE_F32 (the harness mode needs a float intermediate). */
int aa_resample_axis_fwd(const void *in_dev, void *out_dev, int dtype, int64_t outer, int64_t in_size, int64_t inner,
                         const aa_axis *ax, aa_stream_t stream);

/* Pillow's Image.reduce for 8-bit channels (ImagingReduce): every output pixel is the rounded mean of an fx x fy block of input pixels.
 *   in_dev  [N,C,H,W] uint8 in `layout`; in_strides = the view's strides in ELEMENTS for (N, C, H, W) under the rules of
 *           aa_resample_fwd_strided (rows of consecutive elements, any row pitch, planes uniformly spaced), or NULL for a dense tensor;
 *   box     {x0, y0, x1, y1}, an integer rectangle inside the image (Pillow's order: x first); NULL = the whole image;
 *   out_dev [N,C,ceil((y1-y0)/fy),ceil((x1-x0)/fx)] uint8, dense, in `layout`.
 * Output (Y, X) covers the block that starts at (y0 + Y*fy, x0 + X*fx), clipped to the box: the last row and column of blocks, and the
 * corner, may be partial.  With n the pixels in the block and ss their sum: out = ((ss + n/2) * mult(n)) >> 24 in unsigned 32-bit
 * arithmetic, mult(n) = (uint32)(4294967296.0f / (float)(256 * n)), a float32 division made on the host (a launch has at most four n).
 * fx * fy <= 65536, AA_ERR_BAD_SHAPE beyond; C is 1..4 for AA_NHWC, anything for AA_NCHW.  fx = fy = 1 copies the box.  One launch, no
 * workspace, asynchronous on `stream`.  Added without an ABI version change (additive). */
int aa_reduce_u8(const void *in_dev, void *out_dev, int layout, int64_t N, int64_t C, int64_t H, int64_t W, const int64_t *in_strides,
                 const int64_t *box, int fx, int fy, aa_stream_t stream);
/* The two conversions Image.reduce and Image.resize put around an RGBA / LA image (see AA_FLAG_PREMUL_ALPHA), on dense uint8 tensors
 * with C == 2 or 4, alpha last: straight -> premultiplied from src_dev into dst_dev, and premultiplied -> straight in place. */
int aa_premultiply_u8(const void *src_dev, void *dst_dev, int layout, int64_t N, int64_t C, int64_t H, int64_t W, aa_stream_t stream);
int aa_unpremultiply_u8(void *img_dev, int layout, int64_t N, int64_t C, int64_t H, int64_t W, aa_stream_t stream);

/* ---- ragged batches: N uint8 images of N sizes, each with its own box, into one dense batch -----------------------------------------
 * A decoder or a RandomResizedCrop loader produces N images of N different sizes, each with its own box, all going to one
 * [N, C, oH, oW] batch.  Through the calls above that is N table pairs, N header read-backs (aa_table_query2 synchronises) and N launches.
 * The three calls below do it with THREE launches and no synchronisation whatever N, bit-exact with Pillow (AA_TABLE_PIL arithmetic):
 * aa_many_plan is host arithmetic only — per item and axis the float32 box, the hull [o, e) of all windows (the double operations of
 * precompute_coeffs, in its order), ksize (aa_table_ksize_box's arithmetic), the offsets of the item's two tables in one table arena and
 * of its horizontally resampled intermediate [hull_h, oW, C], and prefix sums of work units — written as one packed descriptor block
 * into caller memory; the caller copies the block to the device (one asynchronous copy) and aa_resample_many_u8 enqueues: one kernel
 * that builds every item's two coefficient sets into the arena (xmin, xsize, int32 weights in 22-bit fixed point; no scatter, gather or
 * span section, nothing measured, nothing read back), the horizontal pass over (item, hull row, strip of output columns), and the vertical
 * pass over (item, output row, strip).  Rows and columns outside an item's hull are never read.  Item i of the result equals
 * aa_resample_fwd on that image with the box tables of its box — a full box, an integer box of the output's size (Pillow's plain
 * crop) and equal sizes in and out (a copy) included: their windows are one tap of weight 1.
 * layout: the class ALL items share and the layout of the dense output — AA_NHWC: interleaved pixels (stride_ch = 1, stride_px = C),
 * AA_NCHW: planes of consecutive bytes (stride_px = 1).  Any row pitch, any plane pitch, any byte offset; the stride of an axis of one
 * element is not looked at.  C is 1..4.  Added without an ABI version change (additive).
 * aa_many_image.flags (the field was `reserved`, always 0): AA_MANY_FLIP_X mirrors that item's output left to right (RandomHorizontalFlip);
 * any other bit makes aa_many_plan return AA_ERR_BAD_SHAPE.  Only aa_resample_many_u8_to_float serves a plan in which an item flips:
 * aa_resample_many_u8 returns AA_ERR_BAD_SHAPE for it (its kernel does not flip).  Zero-initialised callers see no change.
 * AA_MANY_PREMUL_ALPHA resizes that item the way Pillow's Image.resize resizes an RGBA / LA image (AA_FLAG_PREMUL_ALPHA above, for a
 * list): C must be 2 or 4 with STRAIGHT alpha in the last channel, AA_ERR_BAD_SHAPE from aa_many_plan / aa_many_plan_placed otherwise.
 * The colour bytes are premultiplied by alpha as the horizontal pass reads them, the intermediate holds horizontally filtered
 * premultiplied bytes, and the vertical pass converts every output pixel back with its own resampled alpha; a placed plan's fill is
 * written as given, never converted.  An item whose size asked for (its own [vH, vW]; [oH, oW] in a plain plan) equals its [H, W] and
 * whose box is absent or the whole image BY VALUE is Pillow's copy: the plan serves it without the conversions, so it comes out
 * unchanged.  The flag changes nothing else of a plan (hulls, ksizes, offsets, workspace), combines with AA_MANY_FLIP_X, and is served
 * by aa_resample_many_u8 and aa_resample_many_u8_to_float, plain and placed, in both layout classes, in the same three launches;
 * aa_many_plan_patches returns AA_ERR_BAD_SHAPE for it, and aa_resample_many_u8_to_patches for a block that carries it. */
#define AA_MANY_FLIP_X 1
#define AA_MANY_PREMUL_ALPHA 2
typedef struct aa_many_image {
  const void *data_dev;  /* byte (row 0, column 0, channel 0) of the image */
  int64_t H, W;
  int64_t stride_row, stride_px, stride_ch; /* in BYTES */
  double box[4];         /* x0, y0, x1, y1 — Pillow's order, x first; rounded to float32 by the plan, as Pillow's C does */
  int32_t has_box;       /* 0: the whole image (box[] is not read) */
  int32_t flags;         /* 0, or any of AA_MANY_FLIP_X, AA_MANY_PREMUL_ALPHA */
} aa_many_image;
/* Bytes of the packed descriptor block for n items. */
size_t aa_many_desc_bytes(int64_t n);
/* Plan a call: fills desc_host (desc_bytes >= aa_many_desc_bytes(n); any host memory, pinned if the copy is to be asynchronous) and
 * reports the workspace the call needs: table arena + intermediates (offsets across items are 64-bit).  No HIP call: works without a
 * device.  Errors: AA_ERR_BAD_SHAPE for an empty box, a box beyond its image, C outside 1..4, a size beyond INT32_MAX / 4 within one
 * image, or more work units than one grid holds; AA_ERR_STRIDES for an item that is not in `layout`'s class; AA_ERR_KSIZE. */
int aa_many_plan(int filter, int layout, int64_t n, int64_t C, int64_t oH, int64_t oW, const aa_many_image *images, void *desc_host,
                 size_t desc_bytes, size_t *workspace_bytes);
/* PLACED plans: item i is resized to ITS OWN size [vH, vW] exactly as Pillow would (box included), and that result's top-left corner
 * is put at (oy, ox) of the dense [oH, oW] output.  A negative offset crops, a positive one pads; what falls outside the output is never
 * computed, and what the item does not cover is fill[c] (Resize + CenterCrop, letterbox, fit-and-pad).  An item that lies wholly
 * outside is legal: all fill, no work.  vH, vW in 1 .. INT32_MAX / 4, |oy|, |ox| <= INT32_MAX / 4, AA_ERR_BAD_SHAPE beyond.
 * The block of a placed plan is larger: desc_bytes >= aa_many_desc_bytes_placed(n), and that many bytes are copied to the device.
 * places NULL, or every place {oH, oW, 0, 0}: exactly aa_many_plan's block (aa_many_desc_bytes(n) suffices), whatever the fill.
 * fill NULL: 0; entries beyond C are not looked at by the kernels.  aa_resample_many_u8 and aa_resample_many_u8_to_float serve a placed
 * plan with their signatures unchanged: the fill byte is converted like any other byte, and a flip mirrors the whole output row.
 * Added without an ABI version change (additive). */
typedef struct aa_many_place { int64_t vH, vW, oy, ox; } aa_many_place;   /* size Pillow resizes to; where its corner lands */
size_t aa_many_desc_bytes_placed(int64_t n);
int aa_many_plan_placed(int filter, int layout, int64_t n, int64_t C, int64_t oH, int64_t oW, const aa_many_image *images,
                        const aa_many_place *places /* NULL: aa_many_plan */, const uint8_t fill[4] /* NULL: 0 */,
                        void *desc_host, size_t desc_bytes, size_t *workspace_bytes);
/* Enqueue the three launches.  desc_dev: the device copy of desc_host (8-byte aligned), in flight or complete on `stream`; desc_host is
 * read only to size the grids and to check the arguments against the plan.  out_dev [n, C, oH, oW] uint8, dense, in `layout`.
 * workspace_dev: 16-byte aligned, at least the plan's size.  Nothing is allocated, nothing is synchronised.  n == 0 launches nothing. */
int aa_resample_many_u8(const void *desc_host, const void *desc_dev, int64_t n, int64_t C, int64_t oH, int64_t oW, int layout, void *out_dev,
                        void *workspace_dev, size_t workspace_bytes, aa_stream_t stream);
/* The same three launches with a CONVERTING vertical pass: what a model reads instead of Pillow's bytes, with no uint8 batch and no
 * float32 intermediate in between.  With u = the bytes aa_resample_many_u8 writes for the plan (Pillow's, bit for bit):
 *   f = (float)u;  with cv->normalize, f = (f - cv->mean[c]) / cv->std[c] in fp32 (one rounded subtraction, one correctly rounded
 *   division; mean / std in 0..255 units);  element = f, or round_to_nearest_even_16(f) with AA_FLAG_OUT_F16 / AA_FLAG_OUT_BF16 in
 *   cv->flags;  written at column oW - 1 - x instead of x for an item planned with AA_MANY_FLIP_X;  in cv->out_layout, which may differ
 *   from `layout`, the class of the items.
 * This is NOT aa_resample_fwd_u8_to_f32's result: that call resamples in fp32 arithmetic throughout and has no box; this one converts
 * Pillow's byte.  out_dev [n, C, oH, oW] elements, dense, in cv->out_layout, aligned to its element (AA_ERR_BAD_SHAPE otherwise); rows
 * at any alignment beyond that are served (every store is one element).  Both output bits:
 * AA_ERR_BAD_DTYPE; AA_FLAG_FAST or an unknown bit: AA_ERR_BAD_SHAPE.  Every other argument and check as aa_resample_many_u8, all before
 * any launch.  n == 0 launches nothing.  Added without an ABI version change (additive). */
int aa_resample_many_u8_to_float(const void *desc_host, const void *desc_dev, int64_t n, int64_t C, int64_t oH, int64_t oW, int layout,
                                 void *out_dev, void *workspace_dev, size_t workspace_bytes, const aa_convert *cv, aa_stream_t stream);

/* PATCH plans: the ragged batch as the token matrix a native-resolution vision transformer reads (NaViT, NaFlex, VLM towers), in the same
 * three launches.  Item i is resized to ITS OWN size [vH_i, vW_i] = sizes[2 i], sizes[2 i + 1], a multiple of the patch [ph, pw] per
 * axis; there is no canvas, no offset and no fill.  With gh = vH / ph, gw = vW / pw, T_i = gh * gw tokens and D = C * ph * pw, and with
 *   R_i = what aa_resample_many_u8_to_float writes for the one item on a [vH_i, vW_i] output in AA_NCHW, flipped if the item flips,
 * token t = gy * gw + gx of item i is, bit for bit,
 *   AA_PATCH_CPP:  tok[c * ph * pw + py * pw + px] = R_i[c][gy * ph + py][gx * pw + px]     (a Conv2d(C, dim, patch, stride = patch) weight's order)
 *   AA_PATCH_PPC:  tok[(py * pw + px) * C + c]     = R_i[c][gy * ph + py][gx * pw + px]     (einops "(p1 p2 c)")
 * and the output is [rows, D] elements, dense: pad_to = 0 packs the items, item i's tokens at rows T_0 + .. + T_(i-1) on, rows = the sum;
 * pad_to = L > 0 gives every item L rows, [n, L, D], rows = n * L, item i's tokens at row i * L on and its rows beyond T_i all-zero bits
 * (+0.0: pad rows are not normalised).
 * aa_many_plan_patches is host arithmetic only, like aa_many_plan (same records, same errors); desc_bytes >= aa_many_desc_bytes_patches(n),
 * and that many bytes are copied to the device.  AA_ERR_BAD_SHAPE also for a patch below 1, a size that is not a positive multiple of the
 * patch, T_i > pad_to, pad_to < 0, and more work units than one grid holds (2^31 - 1).  It reports the workspace and the output's rows.
 * aa_resample_many_u8_to_patches enqueues the table kernel, the horizontal pass and a vertical pass that converts as
 * aa_resample_many_u8_to_float does and stores every element at its place in its token.  n, C, the layout class and the sizes are the
 * plan's.  cv: normalize / mean / std and the AA_FLAG_OUT_* bits as there (both bits AA_ERR_BAD_DTYPE, AA_FLAG_FAST or an unknown bit
 * AA_ERR_BAD_SHAPE); cv->out_layout is not looked at.  patch_format: AA_PATCH_CPP or AA_PATCH_PPC, AA_ERR_BAD_LAYOUT otherwise.  out_dev
 * aligned to its element; desc_dev, workspace_dev as aa_resample_many_u8; a block that is not a patch plan's AA_ERR_BAD_SHAPE.  Every check
 * comes before any launch; nothing is allocated, synchronised or read back.  Added without an ABI version change (additive). */
#define AA_PATCH_CPP 0
#define AA_PATCH_PPC 1
size_t aa_many_desc_bytes_patches(int64_t n);
int aa_many_plan_patches(int filter, int layout, int64_t n, int64_t C, int64_t ph, int64_t pw, const aa_many_image *images,
                         const int64_t *sizes, int64_t pad_to, void *desc_host, size_t desc_bytes, size_t *workspace_bytes, int64_t *rows);
int aa_resample_many_u8_to_patches(const void *desc_host, const void *desc_dev, void *out_dev, void *workspace_dev, size_t workspace_bytes,
                                   const aa_convert *cv, int patch_format, aa_stream_t stream);

/* NEAREST plans: what travels with the image in segmentation, depth and instance-mask training — the label map — through the same box,
 * size, place and flip as its image, but with Pillow's Image.NEAREST (AA_FILTER_BOX, which the reference binds as "nearest", is the box
 * filter; this is not it).  Item i of the result is, element for element,
 *   R_i = PIL.Image.resize((vW_i, vH_i), Image.NEAREST, box=box_i), pasted at (oy_i, ox_i) of an [oH, oW] canvas of fill[c], and the whole
 *   canvas row mirrored left to right for an item planned with AA_MANY_FLIP_X (as aa_resample_many_u8_to_float mirrors it).
 * Pillow picks the source index of an axis by accumulating a double step, not by a closed form (the two differ: 2 -> 7 is the smallest
 * case): with the box as float32 values b0, b1 (no box: 0 and the image's size),
 *   a = (double)(b1 - b0 as a FLOAT difference) / out_size;  xo = (double)b0 + a * 0.5;  idx[x] = (int)xo;  xo = xo + a   for x = 0, 1, ...
 * Pillow resizes "I;16" alone through its generic transform, which evaluates idx[x] = (int)(a * (x + 0.5) + (double)b0) afresh for every
 * x; elem_bytes 2 is that mode and follows it (the plan's second double is then b0).
 * aa_many_plan_nearest is host arithmetic only (no HIP call: works without a device).  It takes aa_many_image records (flags: 0 or
 * AA_MANY_FLIP_X, any other bit AA_ERR_BAD_SHAPE; strides in bytes under the rules of `layout`'s class, with elem_bytes in place of one
 * byte) and aa_many_place records (NULL: every item the whole canvas at offset 0), and writes one packed descriptor block — per item and
 * axis the covered part [v0, v0 + m) of the placed result, the two doubles a and xo computed with exactly the operations above, and the
 * workspace offsets of the item's two index tables — into desc_host, desc_bytes >= aa_many_desc_bytes_nearest(n).  elem_bytes: 1 (uint8,
 * C = 1..4), 2 or 4 (int16 / int32 id maps: C must be 1, AA_ERR_BAD_SHAPE otherwise; data and strides aligned to the element,
 * AA_ERR_STRIDES otherwise); any other value AA_ERR_BAD_DTYPE.  Elements are copied, so signedness does not matter.  fill: C values, each
 * within what the element holds, signed or unsigned (AA_ERR_BAD_SHAPE beyond); NULL: 0.  The other errors are aa_many_plan_placed's:
 * AA_ERR_BAD_SHAPE for an empty box, a box beyond its image, C outside 1..4, a size or offset beyond INT32_MAX / 4, or more work units than
 * one grid holds; AA_ERR_STRIDES for an item that is not in `layout`'s class; AA_ERR_WORKSPACE for a short block; AA_ERR_NULL.
 * aa_resample_many_nearest enqueues TWO launches whatever n: a table kernel (one lane per item and axis runs the sum above in order from
 * index 0 of the item's own size, clamps every index to the image, and stores the covered entries) and a gather over (item, plane, canvas
 * row, 1 KiB of the row) that writes every byte of the output and nothing else.  n, C, the sizes, the class and elem_bytes are the plan's.
 * out_elem_bytes: elem_bytes, or 8 (C = 1 only): every element sign-extended (elem_bytes 2, 4) or zero-extended (elem_bytes 1) to int64,
 * what a loss reads; anything else AA_ERR_BAD_DTYPE.  out_dev [n, C, oH, oW] elements, dense, in the plan's layout, aligned to its element;
 * desc_dev (8-byte aligned) and workspace_dev (16-byte aligned, at least the plan's size) as aa_resample_many_u8.  Every check comes before
 * the first launch; nothing is allocated, synchronised or read back, and no table cache is touched.  n == 0 launches nothing.
 * Added without an ABI version change (additive). */
size_t aa_many_desc_bytes_nearest(int64_t n);
int aa_many_plan_nearest(int layout, int elem_bytes, int64_t n, int64_t C, int64_t oH, int64_t oW, const aa_many_image *images,
                         const aa_many_place *places /* may be NULL */, const int32_t *fill /* C values; NULL: 0 */, void *desc_host,
                         size_t desc_bytes, size_t *workspace_bytes);
int aa_resample_many_nearest(const void *desc_host, const void *desc_dev, void *out_dev, void *workspace_dev, size_t workspace_bytes,
                             int out_elem_bytes /* elem_bytes or 8 */, aa_stream_t stream);

/* MAPS plans: the measured map of a batch — depth and disparity as 16-bit or float32, height maps, 16-bit rasters, int32 counters —
 * through the same box, size, place and flip as its image, FILTERED, with the arithmetic Pillow keeps for its three wide single-band
 * modes (Resample.c: ImagingResampleHorizontal_16bpc / _32bpc and their vertical twins).  elem: AA_MAPS_U16 is "I;16", AA_MAPS_I32 "I",
 * AA_MAPS_F32 "F"; one channel.  Item i of the result is, bit for bit,
 *   R_i = PIL.Image.resize((vW_i, vH_i), FILTER, box=box_i), pasted at (oy_i, ox_i) of an [oH, oW] canvas of `fill`, and the whole canvas
 *   row mirrored left to right for an item planned with AA_MANY_FLIP_X.
 * The arithmetic: windows and coefficients are precompute_coeffs's (the box as floats, the scale their FLOAT difference over the size,
 * windows clipped to the image), and the weights stay its normalised doubles (no normalize_coeffs_8bpc).  Every output of every pass is
 *   ss = 0.0;  ss = ss + (double)in[xmin + x] * k[x]  for x ascending   (product rounded to double, then the sum: no fused multiply-add)
 * stored by the mode's rule after EACH pass, with ROUND_UP(f) = (int)(f >= 0 ? f + 0.5 : f - 0.5):
 *   AA_MAPS_F32: (float)ss.   AA_MAPS_I32: ROUND_UP(ss) (beyond int32: unspecified, as in Pillow's C).
 *   AA_MAPS_U16: r = ROUND_UP(ss); low byte CLIP8(r % 256) (C's remainder), high byte CLIP8(r >> 8).  That is no clamp: a negative r
 *   gives 0, r > 65535 gives 0xFF00 | (r & 255), and the vertical pass reads the wrapped intermediate.  overflow AA_MAPS_OVERFLOW_CLAMP
 *   stores min(max(r, 0), 65535) in both passes instead; the argument is checked and otherwise ignored for the other two elements.
 * Which passes run is Pillow's decision per item: none (the element is copied) when the box has the size asked for at an integer offset
 * (no box: the image's own size); else the horizontal pass only if vW != W or the box does not span the width, the vertical one only if
 * vH != H or the box does not span the height.  A pass that is skipped is not run as an identity filter.
 * aa_many_plan_maps is host arithmetic only (no HIP call: works without a device).  It takes aa_many_image records (flags: 0 or
 * AA_MANY_FLIP_X, any other bit AA_ERR_BAD_SHAPE; strides in bytes under the planar rules with one channel: stride_px is the element's
 * bytes; data and stride_row aligned to the ELEMENT only, so rows of a uint16 view may start on an odd element; AA_ERR_STRIDES
 * otherwise) and aa_many_place records (NULL: every item the whole canvas at offset 0), and writes one packed descriptor block into
 * desc_host, desc_bytes >= aa_many_desc_bytes_maps(n): per item the passes that run, per axis the covered part of the placed result,
 * the hull of its windows, ksize, and the workspace offsets.  The workspace is a table arena — a table is [int32 xmin[m]][int32
 * xsize[m]][double w[m * ksize]], m the covered results of the axis, the doubles 8-byte aligned — plus, for the items whose horizontal
 * pass runs, an intermediate of the element's type that holds only the rows the vertical pass reads.  fill: an integer in 0..65535
 * (AA_MAPS_U16) or within int32 (AA_MAPS_I32), or a finite value whose float is finite (AA_MAPS_F32, written as (float)fill);
 * AA_ERR_BAD_SHAPE otherwise.  Other errors: AA_ERR_BAD_FILTER; AA_ERR_BAD_DTYPE for an unknown elem; AA_ERR_BAD_SHAPE for an unknown
 * overflow, an empty box, a box beyond its image, a size or offset beyond INT32_MAX / 4, or more work units than one grid holds;
 * AA_ERR_KSIZE; AA_ERR_WORKSPACE for a short block; AA_ERR_NULL.
 * aa_resample_many_maps enqueues THREE launches whatever n (two when no item's horizontal pass runs on the canvas): a table kernel
 * (device double arithmetic, aa_pil_coeffs.h's expressions), the horizontal pass over the items that have one, and a vertical pass over
 * (item, canvas row, 256 columns) that writes every element of the output and nothing else.  Everything is the plan's.  out_dev
 * [n, 1, oH, oW] elements, dense, aligned to the element; desc_dev (8-byte aligned) and workspace_dev (16-byte aligned, at least the
 * plan's size) as aa_resample_many_u8.  Every check comes before the first launch; nothing is allocated, synchronised or read back, and
 * no table cache is touched.  n == 0 launches nothing.  Added without an ABI version change (additive). */
#define AA_MAPS_U16 0
#define AA_MAPS_I32 1
#define AA_MAPS_F32 2
#define AA_MAPS_OVERFLOW_PILLOW 0
#define AA_MAPS_OVERFLOW_CLAMP 1
size_t aa_many_desc_bytes_maps(int64_t n);
int aa_many_plan_maps(int filter, int elem, int64_t n, int64_t oH, int64_t oW, const aa_many_image *images,
                      const aa_many_place *places /* may be NULL */, double fill, int overflow, void *desc_host, size_t desc_bytes,
                      size_t *workspace_bytes);
int aa_resample_many_maps(const void *desc_host, const void *desc_dev, void *out_dev, void *workspace_dev, size_t workspace_bytes,
                          aa_stream_t stream);

/* Subsampled YCbCr planes to an RGB batch (resize_many_ycbcr): what a JPEG or video decoder next to the GPU produces, taken to the
 * batch without an RGB image in between.  Item i has a luma plane [H, W] and two chroma planes [ceil(H / sy), ceil(W / sx)], chroma
 * centred (JFIF siting); with b its box (or the whole luma plane) and cb = (b.x0 / sx, b.y0 / sy, b.x1 / sx, b.y1 / sy) in float32,
 *   P = merge("YCbCr", [resize(Y, b), resize(Cb, cb), resize(Cr, cb)]).convert("RGB")       each resize Pillow's "L" resize to (vW, vH)
 * is pasted at its place of the canvas, everything else the fill, which is three RGB bytes written as given; the whole canvas row is
 * mirrored for an item with AA_MANY_FLIP_X.  Bit for bit Pillow's bytes: every plane goes through both 8bpc passes at its own
 * resolution, each rounded to a byte, and Pillow's YCbCr -> RGB integer conversion runs once per output pixel (csrc/aa_ycbcr.h).
 * This is NOT what decoding to RGB with a decoder's chroma upsampling and resizing that gives: the roundings fall elsewhere.
 * aa_ycbcr_image: byte (row y, column x) of the luma plane is at y_dev + y * y_stride_row + x; of a chroma plane at
 * c{b,r}_dev + y * c{b,r}_stride_row + x * chroma_stride_px.  chroma_stride_px 1: two planes, each anywhere with its own pitch;
 * 2: interleaved Cb Cr pairs (NV12), cr_dev == cb_dev + 1 and equal pitches (AA_ERR_STRIDES otherwise).  ONE arrangement per call
 * (AA_ERR_STRIDES for a mixed list).  box, has_box, flags as aa_many_image's, in luma coordinates; flags 0 or AA_MANY_FLIP_X.
 * aa_many_plan_ycbcr is host arithmetic only (no HIP call: works without a device) and does every check: AA_ERR_NULL for a null
 * plane; AA_ERR_BAD_SHAPE for an unknown subsampling, a chroma shape other than [ceil(H / sy), ceil(W / sx)], a box beyond the luma
 * plane, a bad place; the other errors are aa_many_plan_placed's.  desc_bytes >= aa_many_desc_bytes_ycbcr(n), and that many bytes are
 * copied to the device.  n == 0 plans an empty block (AA_OK), which launches nothing.
 * aa_resample_many_ycbcr enqueues THREE launches whatever n when the chroma is planar (one table kernel and one horizontal pass over
 * all 3 n planes, one converting vertical pass) and FIVE when it is interleaved (luma and chroma pairs have a table kernel and a
 * horizontal pass each: their rows differ in bytes per pixel).  cv NULL: out_dev is uint8 [n, 3, oH, oW] in out_layout; otherwise
 * aa_resample_many_u8_to_float's conversion of those bytes (cv->out_layout is not read: out_layout says it), out_dev aligned to its
 * element.  desc_dev (8-byte aligned), workspace_dev (16-byte aligned, at least the plan's size) as aa_resample_many_u8.  Every check
 * comes before the first launch; nothing is allocated, synchronised or read back, no table cache is touched.
 * aa_ycbcr_to_rgb_u8: the conversion alone, on the host, n_px interleaved triples to n_px interleaved triples, with the code the
 * kernel compiles.  Added without an ABI version change (additive). */
#define AA_YCC_444 0  /* sx, sy = 1, 1 */
#define AA_YCC_422 1  /* 2, 1 */
#define AA_YCC_420 2  /* 2, 2 */
#define AA_YCC_440 3  /* 1, 2 */
typedef struct aa_ycbcr_image {
  const void *y_dev, *cb_dev, *cr_dev;
  int64_t H, W;            /* the luma plane */
  int64_t cH, cW;          /* the chroma planes: checked against H, W and the subsampling */
  int64_t y_stride_row, cb_stride_row, cr_stride_row; /* in BYTES */
  int32_t chroma_stride_px; /* 1: planes; 2: interleaved Cb Cr pairs */
  int32_t subsampling;     /* AA_YCC_* */
  double box[4];           /* x0, y0, x1, y1 in luma coordinates */
  int32_t has_box;
  int32_t flags;           /* 0 or AA_MANY_FLIP_X */
} aa_ycbcr_image;
size_t aa_many_desc_bytes_ycbcr(int64_t n);
int aa_many_plan_ycbcr(int filter, int64_t n, int64_t oH, int64_t oW, const aa_ycbcr_image *images,
                       const aa_many_place *places /* may be NULL */, const uint8_t fill_rgb[3] /* NULL: 0 */, void *desc_host,
                       size_t desc_bytes, size_t *workspace_bytes);
int aa_resample_many_ycbcr(const void *desc_host, const void *desc_dev, void *out_dev, void *workspace_dev, size_t workspace_bytes,
                           const aa_convert *cv /* NULL: uint8 */, int out_layout, aa_stream_t stream);
int aa_ycbcr_to_rgb_u8(const uint8_t *ycbcr, uint8_t *rgb, int64_t n_px);

/* ---- ragged position grids: one learned [H0, W0, D] embedding resampled to N token grids, forward and backward ------------------------
 * What follows the patch plans above in a native-resolution vision transformer: its position embedding, a float grid [H0, W0, D], is
 * resampled to every item's own token grid [gh_i, gw_i] and packed in the patch tokens' row order; it is a parameter, so there is a
 * backward.  The arithmetic is aa_resample_fwd's for float images with AA_TABLE_F32 tables: item i is, bit for bit, what that call gives
 * the grid as a [1, D, H0, W0] float32 image at size [gh_i, gw_i] (the horizontal pass first, an fp32 intermediate, taps in order, product
 * and sum rounded apart), token t = ty * gw_i + tx holding the D channels of output pixel (ty, tx), rounded to nearest even ONCE to the
 * output's element.  The output is [rows, D], dense: pad_to = 0 packs the items, item i's tokens at rows T_0 + .. + T_(i-1) on;
 * pad_to = L > 0 gives every item L rows, rows = n * L, item i's tokens at row i * L on and its rows beyond T_i all-zero bits.
 * aa_embed_many_plan is host arithmetic only (no HIP call: works without a device).  grids: n pairs (gh_i, gw_i), height first.  It
 * writes one packed descriptor block — per item the ksize and scale of its two tables (aa_table_ksize's arithmetic), the row capacity of
 * their adjoints (aa_table_transposed_ksize) and the four offsets into one table arena, then the int64 first rows of the items — into
 * desc_host, desc_bytes >= aa_embed_many_desc_bytes(n), and reports the workspace (the arena) and the output's rows.  Errors:
 * AA_ERR_BAD_FILTER; AA_ERR_BAD_SHAPE for n < 0, D, H0 or W0 below 1, any of them or a grid side beyond INT32_MAX / 4, a grid side below
 * 1, T_i beyond INT32_MAX / 4 or beyond pad_to, pad_to < 0, or more lanes than one grid holds; AA_ERR_NULL; AA_ERR_WORKSPACE for a short
 * block; AA_ERR_KSIZE.
 * aa_resample_embed_many enqueues TWO launches whatever n: a table kernel (one workgroup per item and axis, the device functions of
 * aa_table_build) and the resample, one lane per output row and four channels (one where D, a stride or an address is no multiple of
 * four elements).  embed_dev: element (y, x, d) at embed_dev + (y * stride_row + x * stride_px + d) elements, strides in ELEMENTS, any
 * non-negative value, the address aligned to the element (AA_ERR_STRIDES otherwise); in_dtype and out_dtype AA_F32, AA_F16 or AA_BF16,
 * independently (AA_ERR_BAD_DTYPE otherwise).  out_dev [rows, D] elements, aligned to its element.
 * aa_resample_embed_many_bwd enqueues TWO launches whatever n: the table kernel, which also builds every table's adjoint (the rows of
 * aa_table_transpose), and a gather with one lane per source cell and four channels (or one).  With G_i the rows of item i in
 * grad_tokens_dev ([rows, D] of grad_dtype, dense, the plan's rows; pad rows are not read) and b_i = aa_resample_bwd of float(G_i) as a
 * [1, D, gh_i, gw_i] image in AA_F32 (the gather form), grad_embed_dev [H0, W0, D] of out_dtype, dense, is
 *   acc = b_0;  acc = acc + b_i in fp32 for i = 1 .. n - 1 in ascending order;  element = acc rounded to nearest even once.
 * No atomics: the result is deterministic and does not depend on the launch shape.  n == 0 launches nothing (the caller zero-fills).
 * Both: desc_dev (8-byte aligned) and workspace_dev (16-byte aligned, at least the plan's size) as aa_resample_many_u8; n, D, H0, W0,
 * the filter and pad_to are the plan's.  Every check comes before the first launch; nothing is allocated, synchronised or read back, and
 * no table cache is touched.  Added without an ABI version change (additive). */
size_t aa_embed_many_desc_bytes(int64_t n);
int aa_embed_many_plan(int filter, int64_t n, int64_t D, int64_t H0, int64_t W0, const int64_t *grids, int64_t pad_to /* 0: packed */,
                       void *desc_host, size_t desc_bytes, size_t *workspace_bytes, int64_t *out_rows);
int aa_resample_embed_many(const void *desc_host, const void *desc_dev, const void *embed_dev, int in_dtype, int64_t stride_row,
                           int64_t stride_px, void *out_dev, int out_dtype, void *workspace_dev, size_t workspace_bytes, aa_stream_t stream);
int aa_resample_embed_many_bwd(const void *desc_host, const void *desc_dev, const void *grad_tokens_dev, int grad_dtype, void *grad_embed_dev,
                               int out_dtype, void *workspace_dev, size_t workspace_bytes, aa_stream_t stream);

/* ---- ragged predictions back: N float sources [K, h_i, w_i] to N outputs of N sizes, reduced over K before the store -----------------
 * The return path of the ragged calls above.  A segmentation, depth or mask head answers [N, K, H, W] on the canvas; item i is the
 * rectangle of it that image i occupied, and what is wanted is that rectangle at the image's own [oh_i, ow_i], mostly only its argmax
 * over the K classes or its sign.  The arithmetic is aa_resample_fwd's for float images with AA_TABLE_F32 tables: with R_i, bit for
 * bit, what that call gives float(item i) as a [1, K, h_i, w_i] float32 image at size [oh_i, ow_i] (the horizontal pass first, an fp32
 * intermediate, tap 0 unconditionally and the others in order, product and sum rounded apart), item i of the arena is
 *   reduce 0 (values)   [K, oh_i, ow_i] of out_dtype AA_F32 / AA_F16 / AA_BF16: R_i rounded to nearest even ONCE;
 *   reduce 1 (argmax)   [oh_i, ow_i] of out_dtype AA_U8 (K <= 256) / AA_I16 (K <= 32768) / AA_I32 / AA_I64: the lowest k at which R_i is
 *                       greatest, a NaN counting as greater than every number and the first NaN winning (numpy.argmax over axis 0);
 *                       the K values of a pixel are never stored;
 *   reduce 2 (greater)  [K, oh_i, ow_i] bytes, out_dtype AA_BOOL or AA_U8: 1 where R_i > threshold (compared as floats; a NaN gives 0),
 * dense, at byte out_offsets[i] of the arena, a multiple of 16; the bytes between items are not written.  An item with AA_MANY_FLIP_X
 * holds column ow_i - 1 - x of that result at column x.
 * aa_back_item: data_dev is the rectangle's corner, class k, row y, pixel x of it at data_dev + k * stride_ch + y * stride_row +
 * x * stride_px ELEMENTS; non-negative strides in one of two classes, ONE per call (`layout`) — AA_NCHW: planes, stride_px = 1, any
 * stride_ch and stride_row; AA_NHWC: interleaved classes, stride_ch = 1, stride_px = K, any stride_row (AA_ERR_STRIDES otherwise; the
 * stride of an axis of one element is not looked at).  Nothing outside the rectangle is read.
 * aa_back_many_plan is host arithmetic only (no HIP call: works without a device).  It writes one packed descriptor block — per item
 * its pointer and strides, sizes and flags, the ksize and scale of its two tables (aa_table_ksize(filter, AA_TABLE_F32, in, out, 0, 0.0);
 * (float)in / (float)out), their offsets in the workspace (header, xmin, xsize and weight rows each, no gather section, one table after
 * the other) and its arena
 * offset, then the int64 running count of work units (an output row times 256 columns) — into desc_host, desc_bytes >=
 * aa_back_many_desc_bytes(n), and reports the workspace, the arena and the items' offsets.  Errors, in this order: AA_ERR_BAD_FILTER;
 * AA_ERR_BAD_LAYOUT; AA_ERR_BAD_SHAPE for n outside 0 .. INT32_MAX / 4, K outside 1 .. INT32_MAX / 4, an unknown reduce, K beyond what an
 * AA_U8 / AA_I16 label holds; AA_ERR_NULL; AA_ERR_WORKSPACE for a short block; then per item AA_ERR_NULL for a null pointer, AA_ERR_BAD_SHAPE for a
 * size outside 1 .. INT32_MAX / 4, K * oh_i * ow_i beyond 2^40, an unknown flag bit, an arena beyond 2^43 bytes or more work units than
 * one grid holds, AA_ERR_STRIDES, AA_ERR_KSIZE; last AA_ERR_BAD_DTYPE for an out_dtype the reduction does not store.
 * aa_resample_back_many enqueues TWO launches whatever n and whatever the sizes: a table kernel (one workgroup per item and axis, the
 * device function of aa_table_build) and the resample, one workgroup per work unit and a lane per output column, which computes every
 * class's vertical sum of horizontal sums in registers and hands it to the reduction; there is no intermediate in memory.  in_dtype:
 * AA_F32, AA_F16 or AA_BF16 (AA_ERR_BAD_DTYPE otherwise), every data_dev aligned to it (AA_ERR_STRIDES).  threshold: finite
 * (AA_ERR_BAD_SHAPE; looked at for reduce 2 only).  arena_dev: arena_bytes >= the plan's (AA_ERR_WORKSPACE), aligned to out_dtype's
 * element (AA_ERR_BAD_SHAPE); desc_dev (8-byte aligned) and workspace_dev (16-byte aligned, at least the plan's size) as
 * aa_resample_many_u8; a block that is not this planner's AA_ERR_BAD_SHAPE.  Every check comes before the first launch; nothing is
 * allocated, synchronised or read back, and no table cache is touched.  Not built: fractional rectangles, a dense padded output
 * (the backward of reduce 0 is below).  Added without an ABI version change (additive).
 * aa_back_many_plan_act is aa_back_many_plan with an activation between R_i and everything after it: AA_BACK_ACT_NONE (0; the block is
 * aa_back_many_plan's byte for byte), AA_BACK_ACT_SOFTMAX (1, over the K classes of a pixel) or AA_BACK_ACT_SIGMOID (2, per element);
 * anything else is AA_ERR_BAD_SHAPE, beside the unknown reduce.  The block keeps the activation, and aa_resample_back_many reads it
 * there: the same two launches, no workspace beyond the tables.  P replaces R_i in reduce 0, 1 and 2 as they are stated above, computed
 * in fp32 with every product and sum rounded on its own (never fused), bit for bit tests/activation_ref.py's numpy restatement:
 *   aa_exp(x), x <= 0 or NaN:  NaN -> x + x;  x < -86.0f -> +0;  else n = rintf(x * 1.44269504f) (ties to even),
 *       r = x - n * 0.693359375f, r = r - n * -2.12194440e-4f,  p = 1.9875691500e-4f, p = p * r + c for c = 1.3981999507e-3f,
 *       8.3334519073e-3f, 4.1665795894e-2f, 1.6666665459e-1f, 5.0000001201e-1f,  y = ((p * r) * r + r) + 1.0f,  y * 2^n (exact; 2^n is a
 *       normal number).  At most 0.9916 ulp from exp over every float32 of [-86, 0]; aa_exp(0) = 1; no non-zero subnormal result.
 *   sigmoid:  e = aa_exp(-|v|), q = 1.0f + e, P = (v >= 0 ? 1.0f : e) / q, one correctly rounded division.  NaN -> NaN, +inf -> 1, -inf -> +0.
 *   softmax:  pass one over k ascending, m = v_0, d = 1.0f; v_k > m: d = d * aa_exp(m - v_k) + 1.0f, m = v_k; else d = d + aa_exp(v_k - m).
 *       rcp = 1.0f / d, one correctly rounded division, NaN where m is +inf.  Pass two: P_k = aa_exp(v_k - m) * rcp, subnormal products
 *       kept.  A -inf value gets +0; a pixel with a NaN or a +inf value, or with nothing but -inf, is NaN in every class.
 * A NaN's sign and payload are not defined.  The kernel resamples a softmax pixel's classes twice (nothing is staged). */
typedef struct aa_back_item {
  const void *data_dev;                      /* the rectangle's first element of class 0 */
  int64_t stride_ch, stride_row, stride_px;  /* in ELEMENTS */
  int64_t h, w;                              /* the rectangle */
  int64_t oh, ow;                            /* the size it is resampled to */
  int32_t flags;                             /* 0 or AA_MANY_FLIP_X */
  int32_t reserved;
} aa_back_item;
size_t aa_back_many_desc_bytes(int64_t n);
int aa_back_many_plan(int filter, int layout, int64_t n, int64_t K, const aa_back_item *items, int reduce /* 0 values, 1 argmax, 2 greater */,
                      int out_dtype, void *desc_host, size_t desc_bytes, size_t *workspace_bytes, size_t *arena_bytes,
                      int64_t *out_offsets /* n, bytes */);
enum { AA_BACK_ACT_NONE = 0, AA_BACK_ACT_SOFTMAX = 1, AA_BACK_ACT_SIGMOID = 2 };
int aa_back_many_plan_act(int filter, int layout, int64_t n, int64_t K, const aa_back_item *items, int reduce /* 0 values, 1 argmax, 2 greater */,
                          int activation /* AA_BACK_ACT_* */, int out_dtype, void *desc_host, size_t desc_bytes, size_t *workspace_bytes,
                          size_t *arena_bytes, int64_t *out_offsets /* n, bytes */);
int aa_resample_back_many(const void *desc_host, const void *desc_dev, int in_dtype, float threshold, void *arena_dev, size_t arena_bytes,
                          void *workspace_dev, size_t workspace_bytes, aa_stream_t stream);

/* ---- ragged predictions back, merged: the n items are members of G groups, summed per group before the reduction over K --------------
 * Test-time augmentation: a model answers every image several times, at several scales and mirrored, and the passes are resampled to
 * the image's size, un-mirrored and SUMMED before the label is taken.  Here item i is a member of group group_of[i] in 0 .. G - 1 (any
 * order; every group has at least one member, and its members all have the group's oh, ow), and a group is one output.  With R_i the
 * fp32 value aa_back_many_plan's section defines for item i — mirrored left to right for AA_MANY_FLIP_X, before any rounding to
 * out_dtype — and i_0 < i_1 < ... < i_{M-1} the members of group g in ascending item index,
 *   S_g = R_{i_0}, then S_g = S_g + R_{i_j} for j = 1 .. M - 1: one fp32 round-to-nearest add per element, in that order, never fused
 *   and never reassociated; merge 1 (mean) then divides, S_g / (float)M, correctly rounded (merge 0, sum, does not);
 * and group g of the arena is reduce 0, 1 or 2 of S_g exactly as that section states them for R_i, at byte out_offsets[g].  So a NaN in
 * any member is a NaN in the sum, +inf and -inf in two members give NaN, and a group of one member is aa_resample_back_many's item.
 * aa_back_merged_plan is host arithmetic only.  Its block — header, the n item records of aa_back_many_plan (oh, ow and arena offset
 * their group's), G group records (first member slot, member count, oh, ow, column tiles, arena offset), the int32 list of the n item
 * indices grouped by group and ascending within a group, then the int64 running count of work units per GROUP (an output row times 256
 * columns) — goes into desc_host, desc_bytes >= aa_back_merged_desc_bytes(n, G); the workspace is aa_back_many_plan's for the same
 * items.  Errors, in aa_back_many_plan's order with these added: AA_ERR_BAD_SHAPE beside n, K and reduce for G outside 0 .. n, G == 0
 * with n > 0 or an unknown merge; group_of beside the pointers (AA_ERR_NULL, n > 0); after the short block AA_ERR_BAD_SHAPE for a
 * group_of entry outside 0 .. G - 1, then for an empty group; per item, after its own checks, AA_ERR_BAD_SHAPE for an (oh, ow) that is
 * not that of its group's first member; then per group AA_ERR_BAD_SHAPE for an arena beyond 2^43 bytes or more work units than one grid
 * holds; last AA_ERR_BAD_DTYPE.
 * aa_resample_back_merged enqueues TWO launches whatever n, G and the sizes: aa_resample_back_many's table kernel over the members, and
 * a resample with one workgroup per work unit of a group and a lane per output column: for AA_BACK_UNROLL classes at a time the lane
 * walks the group's members in order, each one's vertical sum of horizontal sums added to the group's in registers, and hands the
 * complete sums to the reduction.  A mirrored member is mirrored where it is read.  Neither a member's values nor, for reduce 1, the K
 * sums are ever stored.  Parameters, checks and their order as aa_resample_back_many; every check comes before the first launch;
 * nothing is allocated, synchronised or read back, and no table cache is touched.  n == 0 launches nothing.  Not built: per-member
 * weights, a maximum instead of the sum, members placed at different positions of the output.  Added without an ABI version change
 * (additive).
 * aa_back_merged_plan_act is aa_back_merged_plan with an activation (AA_BACK_ACT_*, defined at aa_back_many_plan_act) applied to every
 * member's R_i BEFORE the sum: S_g adds the members' P in the same order, and the mean and the reductions follow unchanged, so a group
 * of one member is aa_back_many_plan_act's item.  Activation 0 writes aa_back_merged_plan's block byte for byte.  Errors as
 * aa_back_merged_plan, with these added: AA_ERR_BAD_SHAPE beside the unknown reduce for an unknown activation; for AA_BACK_ACT_SOFTMAX,
 * after the empty group, AA_ERR_BAD_SHAPE for a group of more than 16 members (a lane keeps every member's maximum and reciprocal
 * denominator in LDS between its two passes, 2 KiB a member and workgroup; the sigmoid and activation 0 have no limit).  The block
 * keeps the activation and aa_resample_back_merged reads it there: the same two launches, no workspace beyond the tables.  Its checks
 * as before, with a block whose activation is unknown, or whose softmax plan holds a group of more than 16 members, no plan's block
 * (AA_ERR_BAD_SHAPE, with the header, before in_dtype is looked at); then for a softmax, last before the first launch, the limit on a
 * workgroup's LDS of the device the launches go to — the stream's device, for the null stream the current one — against 2 KiB times the
 * plan's largest group (AA_ERR_BAD_SHAPE; AA_ERR_HIP where the device cannot be asked). */
size_t aa_back_merged_desc_bytes(int64_t n, int64_t g);
int aa_back_merged_plan(int filter, int layout, int64_t n, int64_t K, const aa_back_item *items, int64_t G, const int64_t *group_of /* n */,
                        int merge /* 0 sum, 1 mean */, int reduce /* 0 values, 1 argmax, 2 greater */, int out_dtype, void *desc_host,
                        size_t desc_bytes, size_t *workspace_bytes, size_t *arena_bytes, int64_t *out_offsets /* G, bytes */);
int aa_back_merged_plan_act(int filter, int layout, int64_t n, int64_t K, const aa_back_item *items, int64_t G, const int64_t *group_of /* n */,
                            int merge /* 0 sum, 1 mean */, int reduce /* 0 values, 1 argmax, 2 greater */, int activation /* AA_BACK_ACT_* */,
                            int out_dtype, void *desc_host, size_t desc_bytes, size_t *workspace_bytes, size_t *arena_bytes,
                            int64_t *out_offsets /* G, bytes */);
int aa_resample_back_merged(const void *desc_host, const void *desc_dev, int in_dtype, float threshold, void *arena_dev, size_t arena_bytes,
                            void *workspace_dev, size_t workspace_bytes, aa_stream_t stream);

/* ---- ragged predictions back, backward: N gradients [K, oh_i, ow_i] to N canvases [K, H_i, W_i] ---------------------------------------
 * The backward of aa_resample_back_many's reduce 0, for losses taken at every image's own size.  Item i has a canvas [H_i, W_i], the
 * rectangle (y0, x0, h, w) of it that the forward read, and the gradient G_i [K, oh_i, ow_i] of what the forward made of it.  With
 * U_i = G_i, or G_i mirrored left to right for an item with AA_MANY_FLIP_X, and B_i, bit for bit, what aa_resample_bwd (the gather
 * form) gives float(U_i) as a [1, K, oh_i, ow_i] float32 image for the input [1, K, h, w] with AA_TABLE_F32 tables (the horizontal
 * adjoint pass first, an fp32 intermediate, tap 0 unconditionally and the others in ascending order, product and sum rounded apart),
 * item i of the output is [K, H_i, W_i] (out_layout AA_NCHW) or [H_i, W_i, K] (AA_NHWC) of out_dtype AA_F32 / AA_F16 / AA_BF16: B_i
 * rounded to nearest even ONCE inside the rectangle, +0.0 outside it.  An item whose grad_dev is null has no gradient: all +0.0, and
 * nothing but its H and W is looked at.  No atomics: the bits do not depend on n, on the launch shape or on the run.  Item i lies at byte
 * out_offsets[i] of the output: dense = 1 packs the items one after the other (equal canvases: one [n, K, H, W] tensor), dense = 0 puts
 * each on a multiple of 16 and never writes the bytes between them.
 * aa_back_bwd_item: class k, row r, column c of the gradient at grad_dev + k * stride_ch + r * stride_row + c ELEMENTS (columns are
 * consecutive); non-negative strides, the stride of an axis of one element not looked at.  Nothing outside the gradient is read.
 * aa_back_many_bwd_plan is host arithmetic only (no HIP call: works without a device).  It writes one packed descriptor block — a
 * 64-byte header, per item its pointer and strides, sizes and flags, the ksize and scale of its two forward tables (as
 * aa_back_many_plan), the row capacity of their adjoints (aa_table_transposed_ksize) and the four offsets into one table arena (none
 * for an item without a gradient), its output offset, then the int64 running count of work units (4 canvas rows times 64 canvas
 * columns of the WHOLE canvas) — into desc_host, desc_bytes >= aa_back_many_bwd_desc_bytes(n), and reports the workspace, the output's
 * bytes and the items' offsets.  Errors, in this order: AA_ERR_BAD_FILTER; AA_ERR_BAD_LAYOUT; AA_ERR_BAD_SHAPE for n outside
 * 0 .. INT32_MAX / 4, K outside 1 .. INT32_MAX / 4 or dense outside 0 .. 1; AA_ERR_NULL; AA_ERR_WORKSPACE for a short block; then per
 * item AA_ERR_BAD_SHAPE for a canvas side outside 1 .. INT32_MAX / 4, K * H_i * W_i beyond 2^40 or an unknown flag bit, and for an item
 * with a gradient a gradient side outside 1 .. INT32_MAX / 4, K * oh_i * ow_i beyond 2^40 or a rectangle that is empty or not inside the
 * canvas, AA_ERR_STRIDES for a negative stride, AA_ERR_KSIZE, AA_ERR_BAD_SHAPE for an output beyond 2^43 bytes or more work units
 * than one grid holds; last AA_ERR_BAD_DTYPE for an out_dtype that is not AA_F32, AA_F16 or AA_BF16.
 * aa_resample_back_many_bwd enqueues TWO launches whatever n and whatever the sizes: a table kernel (one workgroup per item and axis:
 * the forward table by the device function of aa_table_build, a barrier, its adjoint by that of aa_table_transpose) and the gather, one
 * workgroup per work unit and a lane per canvas cell, which stores every element of the output — the zeros too; there is no memset —
 * and keeps the fp32 intermediate in registers.  grad_dtype: AA_F32, AA_F16 or AA_BF16 (AA_ERR_BAD_DTYPE otherwise), every grad_dev
 * aligned to it (AA_ERR_STRIDES).  out_dev: out_bytes >= the plan's (AA_ERR_WORKSPACE), aligned to out_dtype's element
 * (AA_ERR_BAD_SHAPE); desc_dev (8-byte aligned) and workspace_dev (16-byte aligned, at least the plan's size) as aa_resample_many_u8;
 * a block that is not this planner's AA_ERR_BAD_SHAPE.  Every check comes before the first launch; nothing is allocated, synchronised
 * or read back, and no table cache is touched.  n == 0 launches nothing.  Added without an ABI version change (additive). */
typedef struct aa_back_bwd_item {
  const void *grad_dev;           /* the gradient's first element of class 0; NULL: this item has no gradient */
  int64_t stride_ch, stride_row;  /* in ELEMENTS */
  int64_t H, W;                   /* the item's canvas */
  int64_t y0, x0, h, w;           /* the rectangle of it the forward read */
  int64_t oh, ow;                 /* the gradient's size */
  int32_t flags;                  /* 0 or AA_MANY_FLIP_X */
  int32_t reserved;
} aa_back_bwd_item;
size_t aa_back_many_bwd_desc_bytes(int64_t n);
int aa_back_many_bwd_plan(int filter, int out_layout, int64_t n, int64_t K, const aa_back_bwd_item *items, int out_dtype,
                          int dense /* 0: items on 16-byte boundaries, 1: packed */, void *desc_host, size_t desc_bytes,
                          size_t *workspace_bytes, size_t *out_bytes, int64_t *out_offsets /* n, bytes */);
int aa_resample_back_many_bwd(const void *desc_host, const void *desc_dev, int grad_dtype, void *out_dev, size_t out_bytes,
                              void *workspace_dev, size_t workspace_bytes, aa_stream_t stream);

/* ---- ragged Image.reduce: N uint8 images of N sizes, each with its own integer box and factors, into one arena ------------------------
 * Pillow's first step of Image.resize(reducing_gap=...) for a list: every large item is read ONCE by an integer box mean, and the ragged
 * resize above then runs over the small results, which it reads where they lie (an arena offset is just another pointer of an
 * aa_many_image).  ONE launch whatever n.  Item i of the result equals aa_reduce_u8 on that image with its box and factors, bit for bit
 * (the same device code): dense in the call's class, [rh, rw, C] (AA_NHWC) or [C, rh, rw] (AA_NCHW), rw = ceil((x1 - x0) / fx),
 * rh = ceil((y1 - y0) / fy), at out_offsets[i] of the arena, a multiple of 16.
 * aa_reduce_many_plan is host arithmetic only (no HIP call: works without a device).  It writes one packed descriptor block into caller
 * memory — per item the box's first byte, the pitches, the arena offset, the sizes, the tiling and the four multipliers
 * (uint32)(4294967296.0f / (float)(256 * n)) of aa_reduce_u8, then int64 prefix sums of work units — and reports the arena's size.
 * layout: the class ALL items share, under the rules of aa_many_image; C is 1..4.  Errors: AA_ERR_BAD_SHAPE for C outside 1..4, an
 * empty box or one beyond its image, a factor below 1 or fx * fy > 65536, a size beyond INT32_MAX / 4, or more work units than one grid
 * holds; AA_ERR_STRIDES for an item that is not in `layout`'s class; AA_ERR_NULL; AA_ERR_WORKSPACE for desc_bytes below
 * aa_reduce_many_desc_bytes(n).
 * aa_reduce_many_u8 enqueues the launch.  desc_dev: the device copy of desc_host (8-byte aligned), in flight or complete on `stream`;
 * desc_host is read to size the grid and to check the block's magic, n and arena_bytes against the plan before anything runs.
 * arena_dev: 16-byte aligned, at least the plan's size.  Nothing is allocated, synchronised or read back; n == 0 launches nothing.
 * Added without an ABI version change (additive). */
typedef struct aa_reduce_item {
  const void *data_dev;                      /* byte (row 0, column 0, channel 0) of the IMAGE, not of the box */
  int64_t H, W;
  int64_t stride_row, stride_px, stride_ch;  /* bytes; the rules of aa_many_image for `layout`'s class */
  int64_t box[4];                            /* x0, y0, x1, y1 integers inside the image, Pillow's order */
  int32_t fx, fy;                            /* >= 1, fx * fy <= 65536; 1, 1 copies the box */
} aa_reduce_item;
size_t aa_reduce_many_desc_bytes(int64_t n);
int aa_reduce_many_plan(int layout, int64_t n, int64_t C, const aa_reduce_item *items, void *desc_host, size_t desc_bytes,
                        size_t *arena_bytes, int64_t *out_offsets /* n byte offsets into the arena */);
int aa_reduce_many_u8(const void *desc_host, const void *desc_dev, void *arena_dev, size_t arena_bytes, aa_stream_t stream);

/* Device-to-device copy of `bytes` bytes with 16-byte vector loads/stores, enqueued on `stream`: the probe bench.py times
 * on the box to report the attainable HBM copy ceiling next to the 8 TB/s spec peak.  form 0: one element per
 * thread; 1: grid-stride; 2: four elements per thread, loads in flight before the stores; 3: form 2, streaming (nt) policy;
 * 4: write only (fills dst); 5: read only (sums src). */
int aa_probe_copy(const void *src_dev, void *dst_dev, size_t bytes, int form, aa_stream_t stream);

/* The launch shape a fused family would give a problem: how many strips share a workgroup, how many row bands the image is cut into and
 * how many workgroups are launched (csrc/aa_launch_shape.h; the tests freeze the decisions through this call).  Host arithmetic only:
 * works without a device, the caller states the CU count and what the occupancy query would answer.  AA_ERR_NULL for a null pointer,
 * AA_ERR_BAD_SHAPE for an unknown family or sizes no plan produces (nstrips, items, H, oH, taps, cus < 1; strips_per_block outside 1..8;
 * AA_LAUNCH_V1: threads no positive multiple of 64).  Added without an ABI version change (additive). */
enum aa_launch_family { AA_LAUNCH_V1 = 0, AA_LAUNCH_V3 = 1, AA_LAUNCH_F32_DOWN = 2, AA_LAUNCH_F32_UP = 3 };
typedef struct aa_launch_shape_in {
  int32_t family;           /* aa_launch_family */
  int32_t nstrips;          /* strips of 64 output columns per row band (AA_LAUNCH_V1: 1) */
  int32_t strips_per_block; /* the plan's choice, 1..8 ... */
  int32_t spb_forced;       /* ... and whether the model must keep it */
  int64_t items;            /* images or planes the kernel sees (AA_LAUNCH_V1: N * column bands) */
  int64_t H, oH;
  int32_t taps_h, taps_w;
  uint64_t lds;             /* bytes of LDS per strip (AA_LAUNCH_V1: per workgroup) */
  int32_t saturation;       /* AA_LAUNCH_F32_DOWN: the saturation model applies (fp32 elements) */
  int32_t threads;          /* AA_LAUNCH_V1: threads per workgroup */
  int32_t cus;              /* compute units of the device */
  int32_t occupancy[9];     /* [s], s = 1..8: resident workgroups of s strips per CU as the runtime reports them, -1: the query failed */
} aa_launch_shape_in;
typedef struct aa_launch_shape_out {
  int32_t strips_per_block, ybands;
  int32_t resident;         /* resident workgroups per CU the band count was chosen with */
  int32_t reserved;
  int64_t groups;           /* items x ybands */
  int64_t grid;             /* workgroups; 0: more than 2^31 - 1, the launch fails with AA_ERR_HIP */
} aa_launch_shape_out;
int aa_probe_launch_shape(const aa_launch_shape_in *in, aa_launch_shape_out *out);

/* Launch shape of the fused families, process-wide: a test hook, like aa_set_store_form (the library reads no environment variables).
 * Which shape a launch gets follows from the batch size and the card's occupancy, so a test of ordinary size meets the largest band count
 * and single-strip workgroups only; this makes every shape reachable at any size.  0 means "the model chooses", the default is (0, 0).
 * Applied inside the model, after the knobs of developer builds, so aa_probe_launch_shape answers under it too.  A request is honoured
 * only where it is a shape the kernels are written for; otherwise that component is the model's own answer — nothing is moved to a
 * nearby value and nothing fails.  Whether it is honoured follows from what the plan knows (strips, LDS per strip, oH), never from an
 * occupancy answer:
 *   ybands  honoured when 1 <= ybands <= min(max_yb, 64), max_yb = max(oH / 8, 1) (AA_LAUNCH_F32_UP: oH / 16), the rule of the
 *           developer knob.
 *   spb     honoured when the family is not AA_LAUNCH_V1 (one workgroup form), 1 <= spb <= 8, spb <= nstrips and lds * spb <= 64 KiB
 *           (all three families).  It is then kept as a forced plan's is (no drop to single strips) and the band count is chosen for it,
 *           or forced in turn.
 * Returns the previous setting, spb + 256 * ybands (a request outside 0..255 / 0..65535 is stored as the nearest value of that range:
 * no rule honours it either way).
 * What the kernels presume about the grouping (read before any forced shape ran): all three are compiled with __launch_bounds__(512),
 * eight waves; a wave's stage ring lies at wv * G * seg_bytes (plane groups: wv * G * 1024) of a dynamic LDS block launched as
 * lds * spb bytes, and float up's 1088-byte areas of the 240-column store form lie behind the rings at spb * G * seg_bytes + wv * 1088,
 * inside the same product (their 1088 bytes are part of lds); the kernels read strips_per_block from their parameter block, which the
 * launch fills from this answer together with the block size, so sgroups, the strip of a wave and the surplus exits (strip >= nstrips,
 * group >= items * ybands) agree with the grid; the pacing barriers (v3's unrolled groups, float up's AA_UP_PACE rows) are taken only by
 * workgroups all of whose waves are alive, the waves of a workgroup share one band and so run the same number of groups and rows, and
 * float down has no barrier.  Nothing presumes the plan's own spb.  More than 64 KiB of dynamic LDS needs an attribute no launch sets:
 * hence the LDS rule, stricter than the v3 knob's.  The first-generation kernel has no strips. */
int aa_set_launch_shape(int spb, int ybands);

/* The question and the answer of the last fused launch of aa_resample_fwd* on this thread (thread-local, like aa_last_variant); in the
 * question, occupancy[s] holds what the runtime answered where the model asked it, 0 where it did not.  AA_ERR_BAD_SHAPE when the last
 * such call (or aa_resample_bwd_atomic, aa_resample_axis_fwd) launched no fused kernel; AA_ERR_NULL.  Additive, like the probe. */
int aa_last_launch_shape(aa_launch_shape_in *in, aa_launch_shape_out *out);

/* Kernel selection, process-wide; returns the previous setting.  1 (default): fused single-launch kernels, newest
 * design first; 2: first-generation fused kernels only (A/B measurements); 0: none.
 * With 0 every call takes the generic two-launch path — used by tests to cross-check the fused kernels against an
 * independent implementation at sizes the CPU oracle cannot reach, and by bench.py for A/B numbers. */
int aa_set_fused(int enabled);

/* Store form of the up-scaling / backward kernel, process-wide; returns the previous setting.  -1 (default): chosen from the output
 * size (outputs beyond 64 MiB are stored with the streaming policy, in one of three forms picked from the row pitch); 1: always the
 * streaming forms; 0: never.  A test hook: it lets the parity tests reach the streaming forms at sizes the CPU oracle can check.
 * The library reads NO environment variables (developer builds with -DAA_V2_TUNING do, for experiments). */
int aa_set_store_form(int form);

/* Plane groups of the fused uint8 kernel, process-wide; returns the previous setting.  1 (default): planar (NCHW) uint8 images of
 * three channels run the three planes of an image in one wave (Pillow arithmetic, shrinking heights); 0: one wave per plane, as every
 * other planar shape does.  Same results either way — a test hook and the A/B switch of the measurements in DESIGN.md. */
int aa_set_plane_groups(int enabled);

/* Name of the kernel variant the last aa_resample_fwd on this thread dispatched to (for tests/bench). */
const char *aa_last_variant(void);

#ifdef __cplusplus
}
#endif
#endif /* AA_INTERP_H */
