// aa_api.hip — the C-ABI (include/aa_interp.h): argument checks, host-side ksize arithmetic, dispatch.
// No allocation, no synchronisation (except aa_table_query, documented), no torch types.

#include <math.h>
#include <string.h>

#include <mutex>

#include "aa_box.h"
#include "aa_embed_many.h"
#include "aa_many_back.h"
#include "aa_many_back_bwd.h"
#include "aa_launch_shape.h"
#include "aa_many.h"
#include "aa_many_maps.h"
#include "aa_many_nearest.h"
#include "aa_many_ycbcr.h"
#include "aa_ycbcr.h"
#include "aa_reduce_many.h"
#include "aa_plan.h"
#include "aa_reduce.h"

int g_aa_store_form = -1;  // (aa_common.h; read by aa_fused_float.hip)
int g_aa_plane_groups = 1;  // (aa_common.h; read by aa_fused_u8_v3.hip)

namespace {

thread_local const char *g_last_variant = "none";
// aa_last_launch_shape: the question and the answer of this thread's last fused launch; not valid once a call took another path
thread_local struct { bool valid; aa_launch_shape_in in; aa_launch_shape_out out; } g_last_shape = {};
int g_fused_enabled = 1;

// (s2.2/aa_interpolation_impl.h:287, :377, :333 for the reference's three filters; aa_common.h's table for all of them)
int interp_size_of(int filter) { return aa_filter_valid(filter) ? aa_filter_info(filter).interp_size : -1; }

// ATen area_pixel_compute_scale<scalar_t> (UpSample.h; call site s2.2:314-315). scale<=0: not given.
double scale_for(int kind, int64_t in_size, int64_t out_size, int align_corners, double scale_opt) {
  if (kind == AA_TABLE_F32) {
    if (align_corners) return out_size > 1 ? (double)((float)(in_size - 1) / (float)(out_size - 1)) : 0.0;
    if (scale_opt > 0.) return (double)(float)(1.0 / scale_opt);
    return (double)((float)in_size / (float)out_size);
  }
  if (align_corners) return out_size > 1 ? (double)(in_size - 1) / (double)(out_size - 1) : 0.0;
  if (scale_opt > 0.) return 1.0 / scale_opt;
  return (double)in_size / (double)out_size;
}

int ksize_for(int filter, int kind, double scale) {
  const int interp_size = interp_size_of(filter);
  if (kind == AA_TABLE_PIL) {
    // Pillow precompute_coeffs: support = filter.support * max(scale,1); ksize = (int)ceil(support)*2+1
    const double fs = aa_filter_info(filter).support;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    return (int)ceil(fs * filterscale) * 2 + 1;
  }
  if (kind == AA_TABLE_F32) {
    const float s = (float)scale;
    const float support = (s >= 1.0) ? (float)((interp_size * 0.5) * s) : (float)(interp_size * 0.5);  // s2.2:208-209
    return (int)ceilf(support) * 2 + 1;                                                                  // s2.2:210
  }
  const double support = (scale >= 1.0) ? (interp_size * 0.5) * scale : interp_size * 0.5;
  return (int)ceilf((float)support) * 2 + 1;  // the reference calls ceilf() for double too
}

bool valid_kind(int kind) { return kind == AA_TABLE_PIL || kind == AA_TABLE_F32 || kind == AA_TABLE_F64; }

int check_axis(const aa_axis *a, int64_t in_size) {
  if (!a || !a->table_dev) return AA_ERR_NULL;
  if (a->in_size != in_size || a->out_size <= 0 || a->ksize <= 0) return AA_ERR_BAD_SHAPE;
  if (a->ksize > AA_MAX_KSIZE) return AA_ERR_KSIZE;
  if (!valid_kind(a->kind)) return AA_ERR_BAD_DTYPE;
  return AA_OK;
}

int check_dtype_kind(int dtype, int kh, int kw) {
  if (kh != kw) return AA_ERR_BAD_DTYPE;
  if (dtype == AA_F32 && kh == AA_TABLE_F32) return AA_OK;
  if (dtype == AA_F64 && kh == AA_TABLE_F64) return AA_OK;
  if (dtype == AA_U8 && (kh == AA_TABLE_PIL || kh == AA_TABLE_F32)) return AA_OK;
  if ((dtype == AA_F16 || dtype == AA_BF16) && kh == AA_TABLE_F32) return AA_OK;
  return AA_ERR_BAD_DTYPE;
}

// ---- the forward: one plan, for workspace sizing and launch alike --------------------------------------------------------------------

// AA_FLAG_PREMUL_ALPHA: uint8 images of Pillow's integer arithmetic with 2 or 4 channels, straight alpha last
bool alpha_ok(int dtype, int64_t C, const aa_axis &ah, const aa_axis &aw) {
  return dtype == AA_U8 && (C == 2 || C == 4) && ah.kind == AA_TABLE_PIL && aw.kind == AA_TABLE_PIL;
}

// The problem without its pointers.  oH / oW: the axes' out_size at the entry points, the caller's at aa_workspace_bytes (whose answer
// has always sized the two-pass intermediate from its oW argument).
AAProblem problem(int dtype, int layout, int64_t N, int64_t C, int64_t H, int64_t W, int64_t oH, int64_t oW, const aa_axis &ah,
                  const aa_axis &aw, unsigned flags) {
  AAProblem q{};
  q.dtype = dtype; q.layout = layout;
  q.N = N; q.C = C; q.H = H; q.W = W; q.oH = oH; q.oW = oW;
  q.ah = ah; q.aw = aw;
  q.fast = (flags & AA_FLAG_FAST) ? 1 : 0;
  q.alpha = (flags & AA_FLAG_PREMUL_ALPHA) ? 1 : 0;
  return q;
}

enum FwdRoute { FWD_EMPTY, FWD_ALPHA_COPY, FWD_V3, FWD_V1, FWD_FLOAT, FWD_GENERIC, FWD_CONVERT, FWD_ALPHA_3STEP };

// Which path a forward takes and the workspace it needs, decided once from the problem without its pointers: the aa_workspace_bytes*
// functions answer from it and the forward runs it, so the answer is 0 exactly when the forward needs no workspace.
struct FwdPlan {
  int route;
  int inner;    // FWD_ALPHA_3STEP: the route of its resample of the premultiplied copy
  size_t copy;  // FWD_ALPHA_3STEP: the premultiplied copy, the first part of the workspace
  size_t ws;    // the resample's two-pass intermediate
  V3Plan v3;    // the chosen family's plan
  V1Plan v1;
  F32Plan f32;
  size_t bytes() const { return copy + ws; }
};

FwdPlan plan_fwd(const AAProblem &q) {
  const int mode = g_fused_enabled;  // aa_set_fused: 1 tries v3, v1, float in this order; 2 v1 and float; 0 the two-pass path only
  FwdPlan pl{};
  if (q.N == 0) {  // empty batch is allowed (s2.2:747-750)
    pl.route = FWD_EMPTY;
  } else if (q.alpha) {
    // Pillow's resize returns a copy: no lossy round trip through premultiplied values.  (A box table's in_size is its hull: equal
    // sizes say nothing there, and the caller decides what a full box of the same size is)
    if (q.oH == q.H && q.oW == q.W && !q.ah.reserved[0] && !q.aw.reserved[0]) {
      pl.route = FWD_ALPHA_COPY;
    } else if (mode == 1 && aa_v3_plan(q, false, &pl.v3)) {
      pl.route = FWD_V3;
    } else {  // three steps: premultiplied copy of the input into the workspace, the ordinary resample of it, un-premultiply in place
      AAProblem d = q;
      d.alpha = 0;
      d.in_row_pitch = d.in_img_pitch = 0;
      pl = plan_fwd(d);
      pl.inner = pl.route;
      pl.route = FWD_ALPHA_3STEP;
      pl.copy = aa_align16((size_t)(q.N * q.C * q.H * q.W));
    }
  } else {
    // (Pillow's integer arithmetic and double arithmetic have no tolerance mode; uint8 images with AA_TABLE_F32 tables = the harness's
    // float arithmetic do.  The first-generation kernels of mode 2 have no tolerance mode either)
    const bool fast = q.fast && mode == 1 && q.dtype != AA_F64 && q.aw.kind == AA_TABLE_F32;
    // uint8 -> float32 (out_f32): v3 or the two-pass conversion.  The first-generation kernel takes dense tensors only.
    const bool v3 = mode == 1 && aa_v3_plan(q, fast, &pl.v3);
    if (!q.out_f32 && mode != 0 && !q.in_row_pitch && (!v3 || pl.v3.v1_first) && aa_v1_plan(q, &pl.v1)) pl.route = FWD_V1;
    else if (v3) pl.route = FWD_V3;
    else if (!q.out_f32 && mode != 0 && aa_f32_plan(q, fast, &pl.f32)) pl.route = FWD_FLOAT;
    else {
      pl.route = q.out_f32 ? FWD_CONVERT : FWD_GENERIC;
      pl.ws = aa_generic_workspace_bytes(q.dtype, q.out_f32 ? AA_TABLE_F32 : q.aw.kind, q.N, q.C, q.H, q.oW);
    }
  }
  return pl;
}

int run_fwd(const FwdPlan &pl, int route, const AAProblem &q) {
  const char *variant = "none";
  int rc;
  g_last_shape.valid = false;
  switch (route) {
    case FWD_EMPTY: rc = AA_OK; variant = "empty"; break;
    case FWD_V3: rc = aa_v3_launch(pl.v3, q); variant = pl.v3.variant; break;
    case FWD_V1: rc = aa_v1_launch(pl.v1, q); variant = "fused_u8_nhwc_pil"; break;
    case FWD_FLOAT: rc = aa_f32_launch(pl.f32, q); variant = pl.f32.variant; break;
    case FWD_ALPHA_COPY:
      if (q.in_row_pitch) return AA_ERR_STRIDES;
      if (hipMemcpyAsync(q.out, q.in, (size_t)(q.N * q.C * q.H * q.W), hipMemcpyDeviceToDevice, q.stream) != hipSuccess) return AA_ERR_HIP;
      rc = AA_OK;
      variant = "alpha_copy";
      break;
    case FWD_GENERIC:
    case FWD_CONVERT:
      if (q.in_row_pitch) return AA_ERR_STRIDES;  // no kernel for this view: the caller makes a dense copy (what the two-launch path needs anyway)
      if (!q.ws || q.ws_bytes < pl.ws) return AA_ERR_WORKSPACE;
      rc = route == FWD_GENERIC ? aa_launch_generic_fwd(q, &variant) : aa_launch_generic_convert(q, &variant);
      break;
    default: {  // FWD_ALPHA_3STEP
      if (q.in_row_pitch) return AA_ERR_STRIDES;
      if (!q.ws || q.ws_bytes < pl.bytes()) return AA_ERR_WORKSPACE;
      AAProblem d = q;  // the resample reads the premultiplied copy and has the rest of the workspace
      d.in = q.ws;
      d.ws = (char *)q.ws + pl.copy;
      d.ws_bytes = q.ws_bytes - pl.copy;
      d.alpha = 0;
      rc = aa_launch_premul_u8(q.in, q.ws, q.layout, q.N, q.C, q.H, q.W, q.stream);
      if (rc == AA_OK) rc = run_fwd(pl, pl.inner, d);
      if (rc == AA_OK) rc = aa_launch_unpremul_u8(q.out, q.layout, q.N, q.C, q.oH, q.oW, q.stream);
      variant = "alpha_3step";
    }
  }
  if (rc == AA_OK) g_last_variant = variant;
  return rc;
}

// What every forward does after its own argument checks: plan, check the pointers, run the route
int resample(AAProblem &q, const void *in_dev, void *out_dev, void *workspace_dev, size_t workspace_bytes, aa_stream_t stream) {
  const FwdPlan pl = plan_fwd(q);
  if (pl.route != FWD_EMPTY) {
    if (!in_dev || !out_dev) return AA_ERR_NULL;
    // a tensor of 2 / 4 / 8-byte elements starts on an element boundary; anything else is not a tensor (and the kernels' dispatch must
    // not depend on the pointers: aa_workspace_bytes answers from the shape alone)
    const uintptr_t es = q.dtype == AA_U8 ? 1 : (q.dtype == AA_F64 ? 8 : (q.dtype == AA_F32 ? 4 : 2));
    if ((((uintptr_t)in_dev | (uintptr_t)out_dev) & (es - 1)) != 0) return AA_ERR_BAD_SHAPE;
    // (a float output of uint8 images: its own element size)
    if (q.out_f32 && ((uintptr_t)out_dev & (q.out_elem == AA_F32 ? 3 : 1)) != 0) return AA_ERR_BAD_SHAPE;
  }
  q.in = in_dev; q.out = out_dev; q.ws = workspace_dev; q.ws_bytes = workspace_bytes;
  q.stream = (hipStream_t)stream;
  return run_fwd(pl, pl.route, q);
}

int resample_fwd_impl(const void *in_dev, void *out_dev, void *workspace_dev, size_t workspace_bytes, int dtype, int layout, int64_t N,
                      int64_t C, int64_t H, int64_t W, const aa_axis *ax_h, const aa_axis *ax_w, unsigned flags, int64_t row_pitch,
                      int64_t img_pitch, aa_stream_t stream) {
  if (flags & ~(unsigned)(AA_FLAG_FAST | AA_FLAG_PREMUL_ALPHA)) return AA_ERR_BAD_SHAPE;
  if (dtype < AA_U8 || dtype > AA_BF16) return AA_ERR_BAD_DTYPE;
  if (layout != AA_NCHW && layout != AA_NHWC) return AA_ERR_BAD_LAYOUT;
  if (N < 0 || C <= 0 || H <= 0 || W <= 0) return AA_ERR_BAD_SHAPE;
  int rc = check_axis(ax_h, H);
  if (rc != AA_OK) return rc;
  rc = check_axis(ax_w, W);
  if (rc != AA_OK) return rc;
  rc = check_dtype_kind(dtype, ax_h->kind, ax_w->kind);
  if (rc != AA_OK) return rc;
  if ((flags & AA_FLAG_PREMUL_ALPHA) && !alpha_ok(dtype, C, *ax_h, *ax_w)) return AA_ERR_BAD_DTYPE;
  AAProblem q = problem(dtype, layout, N, C, H, W, ax_h->out_size, ax_w->out_size, *ax_h, *ax_w, flags);
  q.in_row_pitch = row_pitch;
  q.in_img_pitch = img_pitch;
  return resample(q, in_dev, out_dev, workspace_dev, workspace_bytes, stream);
}

// the decode-adjacent conversion's settings; the checks in their order (the fields are filled first: aa_workspace_bytes_u8_to_f32 plans
// with them whatever the checks say)
int fill_convert(AAProblem &q, const aa_convert &cv) {
  q.out_f32 = 1;
  q.out_layout = cv.out_layout;
  q.normalize = cv.normalize ? 1 : 0;
  for (int i = 0; i < 4; i++) { q.mean[i] = cv.mean[i]; q.std[i] = cv.std[i]; }
  q.fast = (cv.flags & AA_FLAG_FAST) ? 1 : 0;
  q.out_elem = (cv.flags & AA_FLAG_OUT_F16) ? AA_F16 : (cv.flags & AA_FLAG_OUT_BF16) ? AA_BF16 : AA_F32;
  if (cv.out_layout != AA_NCHW && cv.out_layout != AA_NHWC) return AA_ERR_BAD_LAYOUT;
  if (cv.normalize && q.C > 4) return AA_ERR_BAD_SHAPE;
  if (cv.flags & ~(uint32_t)(AA_FLAG_FAST | AA_FLAG_OUT_F16 | AA_FLAG_OUT_BF16)) return AA_ERR_BAD_SHAPE;
  if ((cv.flags & AA_FLAG_OUT_F16) && (cv.flags & AA_FLAG_OUT_BF16)) return AA_ERR_BAD_DTYPE;  // one element type
  return AA_OK;
}

}  // namespace

int aa_device_cu_count() {
  static int cached[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (cached[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cached[dev] = n;
  }
  return cached[dev];
}

int aa_resident_blocks(int family, const void *kern, int threads, size_t lds) {
  // (The kernel's address is part of the key.  Until round 3 it was not, and a kernel could be sized with the register budget of whichever
  //  instantiation had asked first with the same threads and LDS bytes — found when the plane-group kernels, whose LDS size is fixed,
  //  ran 40 % slower after a sibling had run)
  struct Entry { const void *kern; int dev, threads; size_t lds; int nb; };
  constexpr int kEntries = 256;
  struct Cache { std::mutex mu; Entry e[kEntries]; int n = 0, next = 0; };
  static Cache caches[4];
  Cache &c = caches[family & 3];
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lock(c.mu);
  for (int i = 0; i < c.n; i++)
    if (c.e[i].kern == kern && c.e[i].dev == dev && c.e[i].threads == threads && c.e[i].lds == lds) return c.e[i].nb;
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, threads, lds) != hipSuccess || nb <= 0) {
    (void)hipGetLastError();
    nb = -1;
  }
  c.e[c.next] = Entry{kern, dev, threads, lds, nb};  // (a full cache forgets its oldest entry)
  c.next = c.next + 1 == kEntries ? 0 : c.next + 1;
  if (c.n < kEntries) c.n++;
  return nb;
}

aa_launch_shape_out aa_kernel_launch_shape(int family, const void *kern, int nstrips, int spb, int spb_forced, int64_t items, const AAProblem &q,
                                           size_t lds, const int *tag, int saturation, int threads) {
  aa_launch_shape_in in{};
  in.family = family; in.nstrips = nstrips; in.strips_per_block = spb; in.spb_forced = spb_forced;
  in.items = items; in.H = q.H; in.oH = q.oH; in.lds = lds; in.saturation = saturation; in.threads = threads;
  in.taps_h = q.ah.max_taps > 0 ? q.ah.max_taps : q.ah.ksize;
  in.taps_w = q.aw.max_taps > 0 ? q.aw.max_taps : q.aw.ksize;
  in.cus = aa_device_cu_count();
  struct Kern { int family; const void *kern; size_t lds; int32_t *asked; } k{family, kern, lds, in.occupancy};
  aa_launch_shape_out out;
  aa_launch_shape(in, [](void *c, int s) {
                    const Kern &k = *(const Kern *)c;
                    const int nb = aa_resident_blocks(k.family, k.kern, 64 * s, k.lds * s);
                    if (s >= 1 && s <= 8) k.asked[s] = nb;  // (for aa_last_launch_shape: the answers this launch was shaped from)
                    return nb;
                  },
                  &k, tag, &out);
  g_last_shape.valid = true; g_last_shape.in = in; g_last_shape.out = out;
  return out;
}

extern "C" {

size_t aa_table_build_bytes(int filter, int kind, int64_t in_size, int64_t out_size, int align_corners, double scale);

int aa_abi_version(void) { return AA_INTERP_ABI_VERSION; }

const char *aa_strerror(int status) {
  switch (status) {
    case AA_OK: return "ok";
    case AA_ERR_BAD_FILTER: return "unknown filter";
    case AA_ERR_BAD_DTYPE: return "dtype / weight-table kind combination not implemented";
    case AA_ERR_BAD_LAYOUT: return "layout must be AA_NCHW or AA_NHWC";
    case AA_ERR_BAD_SHAPE: return "Input and output sizes should be greater than 0 and match the weight tables";
    case AA_ERR_NULL: return "null pointer argument";
    case AA_ERR_WORKSPACE: return "workspace smaller than aa_workspace_bytes()";
    case AA_ERR_KSIZE: return "filter support (ksize) beyond the supported maximum";
    case AA_ERR_HIP: return "HIP kernel launch failed";
    case AA_ERR_STRIDES: return "input view not supported without a copy (rows must be dense, planes uniformly spaced, and a fused kernel must apply)";
    case AA_ERR_NO_DEVICE: return "no HIP device";
    default: return "unknown aa_status";
  }
}

int aa_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

int aa_table_ksize(int filter, int kind, int64_t in_size, int64_t out_size, int align_corners, double scale) {
  if (interp_size_of(filter) < 0) return AA_ERR_BAD_FILTER;
  if (!valid_kind(kind)) return AA_ERR_BAD_DTYPE;
  if (in_size <= 0 || out_size <= 0 || in_size > INT32_MAX / 4 || out_size > INT32_MAX / 4) return AA_ERR_BAD_SHAPE;
  if (kind == AA_TABLE_PIL && (align_corners || scale > 0.)) return AA_ERR_BAD_DTYPE;  // Pillow has neither
  const int k = ksize_for(filter, kind, scale_for(kind, in_size, out_size, align_corners, scale));
  if (k > AA_MAX_KSIZE) return AA_ERR_KSIZE;
  return k;
}

size_t aa_table_bytes(int kind, int64_t out_size, int ksize) {
  if (!valid_kind(kind) || out_size <= 0 || ksize <= 0) return 0;
  return aa_table_total_bytes(kind, out_size, ksize);
}

static int scatter_ksize_for(int filter, int kind, int64_t in_size, int64_t out_size) {
  (void)filter; (void)in_size; (void)out_size;
  // 32-bit weights only (a record holds 6).  Always present: whether an input index really feeds <= 6 outputs is
  // measured by the device kernel (header.scatter_max) and the fused kernels check that before using the section.
  return (kind == AA_TABLE_PIL || kind == AA_TABLE_F32 || kind == AA_TABLE_F64) ? 6 : 0;
}

// What every build call works out per table before it launches: its ksize (negative: the status the call returns), scatter ksize and scale into the
// job spec, and -> the bytes its buffer must hold (0 for a negative ksize).  A box table: in_size is the hull's length, and Pillow's scale comes from the box.
static size_t table_spec(AATableSpec &s, int filter, int kind, int64_t in_size, int64_t out_size, int align_corners, double scale, void *table,
                         int box = 0, int64_t origin = 0, double in0 = 0.0, double in1 = 0.0) {
  const int k = box ? aa_table_ksize_box(filter, kind, in_size, out_size, in0, in1) : aa_table_ksize(filter, kind, in_size, out_size, align_corners, scale);
  s = AATableSpec{in_size, out_size, (box || k < 0) ? 0.0 : scale_for(kind, in_size, out_size, align_corners, scale), k,
                  scatter_ksize_for(filter, kind, in_size, out_size), table, box, origin, in0, in1};
  return k < 0 ? 0 : aa_table_total_bytes(kind, out_size, k) + aa_table_scatter_bytes(kind, in_size, s.scatter_ksize);
}

size_t aa_table_build_bytes(int filter, int kind, int64_t in_size, int64_t out_size, int align_corners, double scale) {
  AATableSpec s;
  return table_spec(s, filter, kind, in_size, out_size, align_corners, scale, nullptr);
}

int aa_table_build(int filter, int kind, int64_t in_size, int64_t out_size, int align_corners, double scale,
                   void *table_dev, size_t table_bytes, aa_stream_t stream) {
  AATableSpec s;
  const size_t need = table_spec(s, filter, kind, in_size, out_size, align_corners, scale, table_dev);
  if (s.ksize < 0) return s.ksize;
  if (!table_dev) return AA_ERR_NULL;
  if (table_bytes < need) return AA_ERR_WORKSPACE;
  return aa_launch_table_jobs(filter, kind, align_corners, &s, 1, (hipStream_t)stream);
}

int aa_table_build2(int filter, int kind, int align_corners, int64_t in_a, int64_t out_a, double scale_a, void *table_a_dev, size_t bytes_a,
                    int64_t in_b, int64_t out_b, double scale_b, void *table_b_dev, size_t bytes_b, aa_stream_t stream) {
  AATableSpec s[2];
  const size_t need_a = table_spec(s[0], filter, kind, in_a, out_a, align_corners, scale_a, table_a_dev);
  if (s[0].ksize < 0) return s[0].ksize;
  const size_t need_b = table_spec(s[1], filter, kind, in_b, out_b, align_corners, scale_b, table_b_dev);
  if (s[1].ksize < 0) return s[1].ksize;
  if (!table_a_dev || !table_b_dev) return AA_ERR_NULL;
  if (bytes_a < need_a || bytes_b < need_b) return AA_ERR_WORKSPACE;
  return aa_launch_table_jobs(filter, kind, align_corners, s, 2, (hipStream_t)stream);
}

int aa_table_transposed_ksize(int filter, int kind, int64_t in_size, int64_t out_size, int align_corners, double scale) {
  const int k = aa_table_ksize(filter, kind, in_size, out_size, align_corners, scale);
  if (k < 0) return k;
  if (kind == AA_TABLE_PIL) return AA_ERR_BAD_DTYPE;
  // an input index x lies in the windows of the outputs whose centre is within +-support of it: about
  // 2*support/scale of them (= interp_size when down-scaling, interp_size/scale when up-scaling); +3 covers the
  // integer rounding of both window ends.
  const double s = scale_for(kind, in_size, out_size, align_corners, scale);
  const int interp_size = interp_size_of(filter);
  const double support = (s >= 1.0) ? interp_size * 0.5 * s : interp_size * 0.5;
  double cover = (s > 0.) ? (2.0 * support + 1.0) / s : (double)out_size;
  int tk = (int)ceil(cover) + 3;
  if (tk > out_size) tk = (int)out_size;
  if (tk < 1) tk = 1;
  if (tk > AA_MAX_KSIZE) return AA_ERR_KSIZE;
  return tk;
}

// Header read-backs land in PINNED host memory (one small buffer per process, behind a mutex) and are copied out from there: an
// asynchronous device-to-host copy into pageable memory — the caller's struct — goes through the runtime's staging path and costs tens of
// microseconds more per copy (a cold call is two of them).
namespace {
std::mutex g_pin_mu;
aa_table_header *g_pin = nullptr;  // two headers
aa_table_header *pinned_headers() {  // (call with g_pin_mu held; nullptr: fall back to the caller's memory)
  if (!g_pin) {
    void *p = nullptr;
    if (hipHostMalloc(&p, 2 * sizeof(aa_table_header), hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      return nullptr;
    }
    g_pin = (aa_table_header *)p;
  }
  return g_pin;
}
}  // namespace

int aa_table_query(const void *table_dev, aa_table_header *host_header, aa_stream_t stream) {
  if (!table_dev || !host_header) return AA_ERR_NULL;
  std::lock_guard<std::mutex> lock(g_pin_mu);
  aa_table_header *pin = pinned_headers();
  aa_table_header *dst = pin ? pin : host_header;
  if (hipMemcpyAsync(dst, table_dev, sizeof(aa_table_header), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess)
    return AA_ERR_HIP;
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return AA_ERR_HIP;
  if (pin) *host_header = *pin;
  if (host_header->magic != AA_TABLE_MAGIC) return AA_ERR_BAD_SHAPE;
  return AA_OK;
}

int aa_table_query2(const void *table_a_dev, const void *table_b_dev, aa_table_header *host_a, aa_table_header *host_b, aa_stream_t stream) {
  if (!table_a_dev || !table_b_dev || !host_a || !host_b) return AA_ERR_NULL;
  std::lock_guard<std::mutex> lock(g_pin_mu);
  aa_table_header *pin = pinned_headers();
  aa_table_header *da = pin ? pin : host_a, *db = pin ? pin + 1 : host_b;
  if (hipMemcpyAsync(da, table_a_dev, sizeof(aa_table_header), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess) return AA_ERR_HIP;
  if (hipMemcpyAsync(db, table_b_dev, sizeof(aa_table_header), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess) return AA_ERR_HIP;
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return AA_ERR_HIP;
  if (pin) { *host_a = pin[0]; *host_b = pin[1]; }
  if (host_a->magic != AA_TABLE_MAGIC || host_b->magic != AA_TABLE_MAGIC) return AA_ERR_BAD_SHAPE;
  return AA_OK;
}

int aa_table_transpose(const void *table_dev, void *tr_table_dev, size_t tr_table_bytes, int tr_ksize,
                       aa_stream_t stream) {
  if (!table_dev || !tr_table_dev) return AA_ERR_NULL;
  aa_table_header h;
  int rc = aa_table_query(table_dev, &h, stream);  // table-build time only
  if (rc != AA_OK) return rc;
  if (h.kind == AA_TABLE_PIL) return AA_ERR_BAD_DTYPE;
  if (tr_ksize <= 0 || tr_ksize > AA_MAX_KSIZE) return AA_ERR_KSIZE;
  if (tr_table_bytes < aa_table_total_bytes(h.kind, h.in_size, tr_ksize)) return AA_ERR_WORKSPACE;
  rc = aa_launch_table_transpose(h, table_dev, tr_table_dev, tr_ksize, (hipStream_t)stream);
  if (rc != AA_OK) return rc;
  // the kernel recorded the widest row it FOUND: rows of tr_ksize entries that cannot hold it would drop gradient taps
  aa_table_header th;
  rc = aa_table_query(tr_table_dev, &th, stream);  // table-build time only
  if (rc != AA_OK) return rc;
  return th.max_taps > tr_ksize ? AA_ERR_KSIZE : AA_OK;
}

// ---- box tables (Image.resize(box=...)) ------------------------------------------------------------------------------------------------
int aa_table_ksize_box(int filter, int kind, int64_t hull, int64_t out_size, double in0, double in1) {
  if (interp_size_of(filter) < 0) return AA_ERR_BAD_FILTER;
  if (!valid_kind(kind)) return AA_ERR_BAD_DTYPE;
  if (kind != AA_TABLE_PIL) return AA_ERR_BAD_DTYPE;  // the reference has no box
  if (hull <= 0 || out_size <= 0 || hull > INT32_MAX / 4 || out_size > INT32_MAX / 4) return AA_ERR_BAD_SHAPE;
  if (!(in0 >= 0.0) || !(in1 > in0) || !(in1 <= (double)(INT32_MAX / 4))) return AA_ERR_BAD_SHAPE;
  const int k = ksize_for(filter, kind, (double)(float)(in1 - in0) / (double)out_size);  // (Pillow's C: a float difference)
  if (k > AA_MAX_KSIZE) return AA_ERR_KSIZE;
  return k;
}

size_t aa_table_build_bytes_box(int filter, int kind, int64_t hull, int64_t out_size, double in0, double in1) {
  AATableSpec s;
  return table_spec(s, filter, kind, hull, out_size, 0, 0.0, nullptr, 1, 0, in0, in1);
}

int aa_table_build_box(int filter, int kind, int64_t origin_a, int64_t hull_a, int64_t out_a, double in0_a, double in1_a, void *table_a_dev,
                       size_t bytes_a, int64_t origin_b, int64_t hull_b, int64_t out_b, double in0_b, double in1_b, void *table_b_dev,
                       size_t bytes_b, aa_stream_t stream) {
  AATableSpec s[2];
  const size_t need_a = table_spec(s[0], filter, kind, hull_a, out_a, 0, 0.0, table_a_dev, 1, origin_a, in0_a, in1_a);
  if (s[0].ksize < 0) return s[0].ksize;
  const size_t need_b = table_spec(s[1], filter, kind, hull_b, out_b, 0, 0.0, table_b_dev, 1, origin_b, in0_b, in1_b);
  if (s[1].ksize < 0) return s[1].ksize;
  if (origin_a < 0 || origin_b < 0 || origin_a > INT32_MAX / 4 || origin_b > INT32_MAX / 4) return AA_ERR_BAD_SHAPE;
  if (!table_a_dev || !table_b_dev) return AA_ERR_NULL;
  if (bytes_a < need_a || bytes_b < need_b) return AA_ERR_WORKSPACE;
  return aa_launch_table_jobs(filter, kind, 0, s, 2, (hipStream_t)stream);
}

// ---- ragged batches ------------------------------------------------------------------------------------------------------------------
size_t aa_many_desc_bytes(int64_t n) { return aa_many_desc_size(n); }

int aa_many_plan(int filter, int layout, int64_t n, int64_t C, int64_t oH, int64_t oW, const aa_many_image *images, void *desc_host,
                 size_t desc_bytes, size_t *workspace_bytes) {
  return aa_many_plan_host(filter, layout, n, C, oH, oW, images, nullptr, nullptr, desc_host, desc_bytes, workspace_bytes);
}

size_t aa_many_desc_bytes_placed(int64_t n) { return aa_many_desc_size_placed(n); }

int aa_many_plan_placed(int filter, int layout, int64_t n, int64_t C, int64_t oH, int64_t oW, const aa_many_image *images,
                        const aa_many_place *places, const uint8_t fill[4], void *desc_host, size_t desc_bytes, size_t *workspace_bytes) {
  return aa_many_plan_host(filter, layout, n, C, oH, oW, images, places, fill, desc_host, desc_bytes, workspace_bytes);
}

int aa_resample_many_u8(const void *desc_host, const void *desc_dev, int64_t n, int64_t C, int64_t oH, int64_t oW, int layout, void *out_dev,
                        void *workspace_dev, size_t workspace_bytes, aa_stream_t stream) {
  if (layout != AA_NCHW && layout != AA_NHWC) return AA_ERR_BAD_LAYOUT;
  if (n < 0 || C < 1 || C > 4 || oH <= 0 || oW <= 0) return AA_ERR_BAD_SHAPE;
  if (!desc_host) return AA_ERR_NULL;
  if (n > 0 && (!desc_dev || !out_dev || !workspace_dev)) return AA_ERR_NULL;
  return aa_launch_many_u8(desc_host, desc_dev, n, C, oH, oW, layout, out_dev, workspace_dev, workspace_bytes, (hipStream_t)stream);
}

int aa_resample_many_u8_to_float(const void *desc_host, const void *desc_dev, int64_t n, int64_t C, int64_t oH, int64_t oW, int layout,
                                 void *out_dev, void *workspace_dev, size_t workspace_bytes, const aa_convert *cv, aa_stream_t stream) {
  if (layout != AA_NCHW && layout != AA_NHWC) return AA_ERR_BAD_LAYOUT;
  if (n < 0 || C < 1 || C > 4 || oH <= 0 || oW <= 0) return AA_ERR_BAD_SHAPE;
  if (!desc_host || !cv) return AA_ERR_NULL;
  if (cv->out_layout != AA_NCHW && cv->out_layout != AA_NHWC) return AA_ERR_BAD_LAYOUT;
  if ((cv->flags & AA_FLAG_OUT_F16) && (cv->flags & AA_FLAG_OUT_BF16)) return AA_ERR_BAD_DTYPE;
  if (cv->flags & ~(AA_FLAG_OUT_F16 | AA_FLAG_OUT_BF16)) return AA_ERR_BAD_SHAPE;  // (AA_FLAG_FAST: the conversion has one arithmetic)
  if (n > 0 && (!desc_dev || !out_dev || !workspace_dev)) return AA_ERR_NULL;
  const int out_elem = (cv->flags & AA_FLAG_OUT_F16) ? AA_F16 : ((cv->flags & AA_FLAG_OUT_BF16) ? AA_BF16 : AA_F32);
  return aa_launch_many_float(desc_host, desc_dev, n, C, oH, oW, layout, out_dev, workspace_dev, workspace_bytes, out_elem, cv->out_layout,
                              cv->normalize, cv->mean, cv->std, (hipStream_t)stream);
}

size_t aa_many_desc_bytes_patches(int64_t n) { return aa_many_desc_size_patches(n); }

int aa_many_plan_patches(int filter, int layout, int64_t n, int64_t C, int64_t ph, int64_t pw, const aa_many_image *images, const int64_t *sizes,
                         int64_t pad_to, void *desc_host, size_t desc_bytes, size_t *workspace_bytes, int64_t *rows) {
  if (!aa_filter_valid(filter)) return AA_ERR_BAD_FILTER;
  return aa_many_plan_patches_host(filter, layout, n, C, ph, pw, images, sizes, pad_to, desc_host, desc_bytes, workspace_bytes, rows);
}

int aa_resample_many_u8_to_patches(const void *desc_host, const void *desc_dev, void *out_dev, void *workspace_dev, size_t workspace_bytes,
                                   const aa_convert *cv, int patch_format, aa_stream_t stream) {
  if (!desc_host || !cv) return AA_ERR_NULL;
  if (patch_format != AA_PATCH_CPP && patch_format != AA_PATCH_PPC) return AA_ERR_BAD_LAYOUT;
  if ((cv->flags & AA_FLAG_OUT_F16) && (cv->flags & AA_FLAG_OUT_BF16)) return AA_ERR_BAD_DTYPE;
  if (cv->flags & ~(AA_FLAG_OUT_F16 | AA_FLAG_OUT_BF16)) return AA_ERR_BAD_SHAPE;  // (AA_FLAG_FAST: the conversion has one arithmetic)
  const int out_elem = (cv->flags & AA_FLAG_OUT_F16) ? AA_F16 : ((cv->flags & AA_FLAG_OUT_BF16) ? AA_BF16 : AA_F32);
  return aa_launch_many_patches(desc_host, desc_dev, out_dev, workspace_dev, workspace_bytes, out_elem, patch_format == AA_PATCH_PPC, cv->normalize,
                                cv->mean, cv->std, (hipStream_t)stream);
}

size_t aa_many_desc_bytes_nearest(int64_t n) { return aa_near_desc_size(n); }

int aa_many_plan_nearest(int layout, int elem_bytes, int64_t n, int64_t C, int64_t oH, int64_t oW, const aa_many_image *images,
                         const aa_many_place *places, const int32_t *fill, void *desc_host, size_t desc_bytes, size_t *workspace_bytes) {
  return aa_near_plan_host(layout, elem_bytes, n, C, oH, oW, images, places, fill, desc_host, desc_bytes, workspace_bytes);
}

int aa_resample_many_nearest(const void *desc_host, const void *desc_dev, void *out_dev, void *workspace_dev, size_t workspace_bytes,
                             int out_elem_bytes, aa_stream_t stream) {
  if (!desc_host) return AA_ERR_NULL;
  return aa_launch_many_nearest(desc_host, desc_dev, out_dev, workspace_dev, workspace_bytes, out_elem_bytes, (hipStream_t)stream);
}

size_t aa_many_desc_bytes_maps(int64_t n) { return aa_maps_desc_size(n); }

int aa_many_plan_maps(int filter, int elem, int64_t n, int64_t oH, int64_t oW, const aa_many_image *images, const aa_many_place *places,
                      double fill, int overflow, void *desc_host, size_t desc_bytes, size_t *workspace_bytes) {
  return aa_maps_plan_host(filter, elem, n, oH, oW, images, places, fill, overflow, desc_host, desc_bytes, workspace_bytes);
}

int aa_resample_many_maps(const void *desc_host, const void *desc_dev, void *out_dev, void *workspace_dev, size_t workspace_bytes,
                          aa_stream_t stream) {
  if (!desc_host) return AA_ERR_NULL;
  return aa_launch_many_maps(desc_host, desc_dev, out_dev, workspace_dev, workspace_bytes, (hipStream_t)stream);
}

// ---- ragged position grids ---------------------------------------------------------------------------------------------------------------
size_t aa_embed_many_desc_bytes(int64_t n) { return aa_embed_desc_size(n); }

int aa_embed_many_plan(int filter, int64_t n, int64_t D, int64_t H0, int64_t W0, const int64_t *grids, int64_t pad_to, void *desc_host,
                       size_t desc_bytes, size_t *workspace_bytes, int64_t *out_rows) {
  return aa_embed_plan_host(filter, n, D, H0, W0, grids, pad_to, desc_host, desc_bytes, workspace_bytes, out_rows);
}

int aa_resample_embed_many(const void *desc_host, const void *desc_dev, const void *embed_dev, int in_dtype, int64_t stride_row, int64_t stride_px,
                           void *out_dev, int out_dtype, void *workspace_dev, size_t workspace_bytes, aa_stream_t stream) {
  if (!desc_host) return AA_ERR_NULL;
  return aa_launch_embed_many(desc_host, desc_dev, embed_dev, in_dtype, stride_row, stride_px, out_dev, out_dtype, workspace_dev, workspace_bytes,
                              (hipStream_t)stream);
}

int aa_resample_embed_many_bwd(const void *desc_host, const void *desc_dev, const void *grad_tokens_dev, int grad_dtype, void *grad_embed_dev,
                               int out_dtype, void *workspace_dev, size_t workspace_bytes, aa_stream_t stream) {
  if (!desc_host) return AA_ERR_NULL;
  return aa_launch_embed_many_bwd(desc_host, desc_dev, grad_tokens_dev, grad_dtype, grad_embed_dev, out_dtype, workspace_dev, workspace_bytes,
                                  (hipStream_t)stream);
}

// ---- ragged predictions back ---------------------------------------------------------------------------------------------------------------
size_t aa_back_many_desc_bytes(int64_t n) { return aa_back_desc_size(n); }

int aa_back_many_plan(int filter, int layout, int64_t n, int64_t K, const aa_back_item *items, int reduce, int out_dtype, void *desc_host,
                      size_t desc_bytes, size_t *workspace_bytes, size_t *arena_bytes, int64_t *out_offsets) {
  return aa_back_plan_host(filter, layout, n, K, items, reduce, AA_BACK_ACT_NONE, out_dtype, desc_host, desc_bytes, workspace_bytes, arena_bytes,
                           out_offsets);
}

int aa_back_many_plan_act(int filter, int layout, int64_t n, int64_t K, const aa_back_item *items, int reduce, int activation, int out_dtype,
                          void *desc_host, size_t desc_bytes, size_t *workspace_bytes, size_t *arena_bytes, int64_t *out_offsets) {
  return aa_back_plan_host(filter, layout, n, K, items, reduce, activation, out_dtype, desc_host, desc_bytes, workspace_bytes, arena_bytes,
                           out_offsets);
}

int aa_resample_back_many(const void *desc_host, const void *desc_dev, int in_dtype, float threshold, void *arena_dev, size_t arena_bytes,
                          void *workspace_dev, size_t workspace_bytes, aa_stream_t stream) {
  if (!desc_host) return AA_ERR_NULL;
  return aa_launch_back_many(desc_host, desc_dev, in_dtype, threshold, arena_dev, arena_bytes, workspace_dev, workspace_bytes, (hipStream_t)stream);
}

// ---- ragged predictions back, merged: the members of a group summed before the reduction ------------------------------------------------
size_t aa_back_merged_desc_bytes(int64_t n, int64_t g) { return aa_back_merged_desc_size(n, g); }

int aa_back_merged_plan(int filter, int layout, int64_t n, int64_t K, const aa_back_item *items, int64_t G, const int64_t *group_of, int merge,
                        int reduce, int out_dtype, void *desc_host, size_t desc_bytes, size_t *workspace_bytes, size_t *arena_bytes,
                        int64_t *out_offsets) {
  return aa_back_merged_plan_host(filter, layout, n, K, items, G, group_of, merge, reduce, AA_BACK_ACT_NONE, out_dtype, desc_host, desc_bytes,
                                  workspace_bytes, arena_bytes, out_offsets);
}

int aa_back_merged_plan_act(int filter, int layout, int64_t n, int64_t K, const aa_back_item *items, int64_t G, const int64_t *group_of, int merge,
                            int reduce, int activation, int out_dtype, void *desc_host, size_t desc_bytes, size_t *workspace_bytes,
                            size_t *arena_bytes, int64_t *out_offsets) {
  return aa_back_merged_plan_host(filter, layout, n, K, items, G, group_of, merge, reduce, activation, out_dtype, desc_host, desc_bytes,
                                  workspace_bytes, arena_bytes, out_offsets);
}

int aa_resample_back_merged(const void *desc_host, const void *desc_dev, int in_dtype, float threshold, void *arena_dev, size_t arena_bytes,
                            void *workspace_dev, size_t workspace_bytes, aa_stream_t stream) {
  if (!desc_host) return AA_ERR_NULL;
  return aa_launch_back_merged(desc_host, desc_dev, in_dtype, threshold, arena_dev, arena_bytes, workspace_dev, workspace_bytes, (hipStream_t)stream);
}

// ---- ragged predictions back, backward -----------------------------------------------------------------------------------------------------
size_t aa_back_many_bwd_desc_bytes(int64_t n) { return aa_back_bwd_desc_size(n); }

int aa_back_many_bwd_plan(int filter, int out_layout, int64_t n, int64_t K, const aa_back_bwd_item *items, int out_dtype, int dense, void *desc_host,
                          size_t desc_bytes, size_t *workspace_bytes, size_t *out_bytes, int64_t *out_offsets) {
  return aa_back_bwd_plan_host(filter, out_layout, n, K, items, out_dtype, dense, desc_host, desc_bytes, workspace_bytes, out_bytes, out_offsets);
}

int aa_resample_back_many_bwd(const void *desc_host, const void *desc_dev, int grad_dtype, void *out_dev, size_t out_bytes, void *workspace_dev,
                              size_t workspace_bytes, aa_stream_t stream) {
  if (!desc_host) return AA_ERR_NULL;
  return aa_launch_back_many_bwd(desc_host, desc_dev, grad_dtype, out_dev, out_bytes, workspace_dev, workspace_bytes, (hipStream_t)stream);
}

size_t aa_many_desc_bytes_ycbcr(int64_t n) { return aa_ycc_desc_size(n); }

int aa_many_plan_ycbcr(int filter, int64_t n, int64_t oH, int64_t oW, const aa_ycbcr_image *images, const aa_many_place *places,
                       const uint8_t fill_rgb[3], void *desc_host, size_t desc_bytes, size_t *workspace_bytes) {
  return aa_ycc_plan_host(filter, n, oH, oW, images, places, fill_rgb, desc_host, desc_bytes, workspace_bytes);
}

int aa_resample_many_ycbcr(const void *desc_host, const void *desc_dev, void *out_dev, void *workspace_dev, size_t workspace_bytes,
                           const aa_convert *cv, int out_layout, aa_stream_t stream) {
  if (!desc_host) return AA_ERR_NULL;
  int out_elem = AA_U8;
  if (cv) {
    if ((cv->flags & AA_FLAG_OUT_F16) && (cv->flags & AA_FLAG_OUT_BF16)) return AA_ERR_BAD_DTYPE;
    if (cv->flags & ~(AA_FLAG_OUT_F16 | AA_FLAG_OUT_BF16)) return AA_ERR_BAD_SHAPE;  // (AA_FLAG_FAST: the conversion has one arithmetic)
    out_elem = (cv->flags & AA_FLAG_OUT_F16) ? AA_F16 : ((cv->flags & AA_FLAG_OUT_BF16) ? AA_BF16 : AA_F32);
  }
  return aa_launch_many_ycbcr(desc_host, desc_dev, out_dev, workspace_dev, workspace_bytes, out_elem, out_layout, cv ? cv->normalize : 0,
                              cv ? cv->mean : nullptr, cv ? cv->std : nullptr, (hipStream_t)stream);
}

int aa_ycbcr_to_rgb_u8(const uint8_t *ycbcr, uint8_t *rgb, int64_t n_px) {
  if (n_px < 0) return AA_ERR_BAD_SHAPE;
  if (n_px > 0 && (!ycbcr || !rgb)) return AA_ERR_NULL;
  for (int64_t i = 0; i < n_px; i++) {
    const uint32_t v = aa_ycbcr_to_rgb(ycbcr[3 * i], ycbcr[3 * i + 1], ycbcr[3 * i + 2]);
    rgb[3 * i] = (uint8_t)v; rgb[3 * i + 1] = (uint8_t)(v >> 8); rgb[3 * i + 2] = (uint8_t)(v >> 16);
  }
  return AA_OK;
}

// ---- Image.reduce ------------------------------------------------------------------------------------------------------------------------
int aa_reduce_u8(const void *in_dev, void *out_dev, int layout, int64_t N, int64_t C, int64_t H, int64_t W, const int64_t *in_strides,
                 const int64_t *box, int fx, int fy, aa_stream_t stream) {
  if (layout != AA_NCHW && layout != AA_NHWC) return AA_ERR_BAD_LAYOUT;
  if (N < 0 || C <= 0 || H <= 0 || W <= 0 || H > INT32_MAX / 4 || W > INT32_MAX / 4) return AA_ERR_BAD_SHAPE;
  if (fx < 1 || fy < 1 || (int64_t)fx * fy > 65536) return AA_ERR_BAD_SHAPE;
  if (layout == AA_NHWC && C > 4) return AA_ERR_BAD_SHAPE;
  const int64_t x0 = box ? box[0] : 0, y0 = box ? box[1] : 0, x1 = box ? box[2] : W, y1 = box ? box[3] : H;
  if (x0 < 0 || y0 < 0 || x1 > W || y1 > H || x1 <= x0 || y1 <= y0) return AA_ERR_BAD_SHAPE;
  if (N == 0) return AA_OK;
  if (!in_dev || !out_dev) return AA_ERR_NULL;
  int64_t sN, sC, sH, sW;
  if (in_strides) {
    sN = in_strides[0]; sC = in_strides[1]; sH = in_strides[2]; sW = in_strides[3];
  } else if (layout == AA_NCHW) {
    sN = C * H * W; sC = H * W; sH = W; sW = 1;
  } else {
    sN = H * W * C; sC = 1; sH = W * C; sW = C;
  }
  AAReduceJob job;
  if (layout == AA_NCHW) {  // (the rules of aa_resample_fwd_strided)
    if (sW != 1 || sH < W || sC < 0 || sN < 0 || (C > 1 && N > 1 && sN != C * sC)) return AA_ERR_STRIDES;
    job.images = N * C;
    job.C = 1;
    job.row_pitch = sH;
    job.img_pitch = C > 1 ? sC : sN;
  } else {
    if (sC != 1 || sW != C || sH < W * C || sN < 0) return AA_ERR_STRIDES;
    job.images = N;
    job.C = (int)C;
    job.row_pitch = sH;
    job.img_pitch = sN;
  }
  if (job.img_pitch == 0 && job.images > 1) return AA_ERR_STRIDES;  // (a broadcast batch: make it dense)
  job.in = (const uint8_t *)in_dev + y0 * job.row_pitch + x0 * job.C;
  job.out = (uint8_t *)out_dev;
  job.bw = (int)(x1 - x0); job.bh = (int)(y1 - y0);
  job.fx = fx; job.fy = fy;
  job.stream = (hipStream_t)stream;
  return aa_launch_reduce_u8(job);
}

// ---- ragged Image.reduce -----------------------------------------------------------------------------------------------------------------
size_t aa_reduce_many_desc_bytes(int64_t n) { return aa_reduce_many_desc_size(n); }

int aa_reduce_many_plan(int layout, int64_t n, int64_t C, const aa_reduce_item *items, void *desc_host, size_t desc_bytes, size_t *arena_bytes,
                        int64_t *out_offsets) {
  return aa_reduce_many_plan_host(layout, n, C, items, desc_host, desc_bytes, arena_bytes, out_offsets);
}

int aa_reduce_many_u8(const void *desc_host, const void *desc_dev, void *arena_dev, size_t arena_bytes, aa_stream_t stream) {
  if (!desc_host) return AA_ERR_NULL;
  return aa_launch_reduce_many_u8(desc_host, desc_dev, arena_dev, arena_bytes, (hipStream_t)stream);
}

int aa_premultiply_u8(const void *src_dev, void *dst_dev, int layout, int64_t N, int64_t C, int64_t H, int64_t W, aa_stream_t stream) {
  if (layout != AA_NCHW && layout != AA_NHWC) return AA_ERR_BAD_LAYOUT;
  if (N < 0 || H <= 0 || W <= 0) return AA_ERR_BAD_SHAPE;
  if (C != 2 && C != 4) return AA_ERR_BAD_DTYPE;
  if (N == 0) return AA_OK;
  if (!src_dev || !dst_dev) return AA_ERR_NULL;
  return aa_launch_premul_u8(src_dev, dst_dev, layout, N, C, H, W, (hipStream_t)stream);
}

int aa_unpremultiply_u8(void *img_dev, int layout, int64_t N, int64_t C, int64_t H, int64_t W, aa_stream_t stream) {
  if (layout != AA_NCHW && layout != AA_NHWC) return AA_ERR_BAD_LAYOUT;
  if (N < 0 || H <= 0 || W <= 0) return AA_ERR_BAD_SHAPE;
  if (C != 2 && C != 4) return AA_ERR_BAD_DTYPE;
  if (N == 0) return AA_OK;
  if (!img_dev) return AA_ERR_NULL;
  return aa_launch_unpremul_u8(img_dev, layout, N, C, H, W, (hipStream_t)stream);
}

size_t aa_workspace_bytes_ex(int dtype, int layout, int64_t N, int64_t C, int64_t H, int64_t W, int64_t oH, int64_t oW,
                             const aa_axis *ax_h, const aa_axis *ax_w, unsigned flags) {
  if (!ax_h || !ax_w || N <= 0) return 0;
  if ((flags & AA_FLAG_PREMUL_ALPHA) && !alpha_ok(dtype, C, *ax_h, *ax_w)) return 0;
  return plan_fwd(problem(dtype, layout, N, C, H, W, oH, oW, *ax_h, *ax_w, flags)).bytes();
}

size_t aa_workspace_bytes(int dtype, int layout, int64_t N, int64_t C, int64_t H, int64_t W, int64_t oH, int64_t oW,
                          const aa_axis *ax_h, const aa_axis *ax_w) {
  return aa_workspace_bytes_ex(dtype, layout, N, C, H, W, oH, oW, ax_h, ax_w, 0u);
}

int aa_resample_fwd(const void *in_dev, void *out_dev, void *workspace_dev, size_t workspace_bytes, int dtype,
                    int layout, int64_t N, int64_t C, int64_t H, int64_t W, const aa_axis *ax_h, const aa_axis *ax_w,
                    aa_stream_t stream) {
  return aa_resample_fwd_ex(in_dev, out_dev, workspace_dev, workspace_bytes, dtype, layout, N, C, H, W, ax_h, ax_w, 0u, stream);
}

int aa_resample_fwd_ex(const void *in_dev, void *out_dev, void *workspace_dev, size_t workspace_bytes, int dtype,
                       int layout, int64_t N, int64_t C, int64_t H, int64_t W, const aa_axis *ax_h, const aa_axis *ax_w,
                       unsigned flags, aa_stream_t stream) {
  return resample_fwd_impl(in_dev, out_dev, workspace_dev, workspace_bytes, dtype, layout, N, C, H, W, ax_h, ax_w, flags, 0, 0, stream);
}

int aa_resample_fwd_strided(const void *in_dev, void *out_dev, int dtype, int layout, int64_t N, int64_t C, int64_t H, int64_t W,
                            const int64_t *in_strides, const aa_axis *ax_h, const aa_axis *ax_w, unsigned flags, aa_stream_t stream) {
  if (!in_strides) return AA_ERR_NULL;
  if (dtype < AA_U8 || dtype > AA_BF16) return AA_ERR_BAD_DTYPE;
  if (N < 0 || C <= 0 || H <= 0 || W <= 0) return AA_ERR_BAD_SHAPE;
  const int64_t es = dtype == AA_U8 ? 1 : (dtype == AA_F64 ? 8 : (dtype == AA_F32 ? 4 : 2));
  const int64_t sN = in_strides[0], sC = in_strides[1], sH = in_strides[2], sW = in_strides[3];
  int64_t row_pitch, img_pitch;
  if (layout == AA_NCHW) {  // rows of W consecutive elements; planes n * C + c uniformly spaced
    if (sW != 1 || sH < W || sC < 0 || sN < 0 || (C > 1 && N > 1 && sN != C * sC)) return AA_ERR_STRIDES;
    row_pitch = sH * es;
    img_pitch = (C > 1 ? sC : sN) * es;
  } else if (layout == AA_NHWC) {  // rows of W pixels of C consecutive channels; images anywhere
    if (sC != 1 || sW != C || sH < W * C || sN < 0) return AA_ERR_STRIDES;
    row_pitch = sH * es;
    img_pitch = sN * es;
  } else {
    return AA_ERR_BAD_LAYOUT;
  }
  const bool dense = row_pitch == W * (layout == AA_NHWC ? C : 1) * es && (N * (layout == AA_NCHW ? C : 1) <= 1 || img_pitch == H * row_pitch);
  if (dense) {
    const int rc = resample_fwd_impl(in_dev, out_dev, nullptr, 0, dtype, layout, N, C, H, W, ax_h, ax_w, flags, 0, 0, stream);
    // (no workspace here: the straight-alpha three-step route is "no kernel for this view", as for a pitched one)
    return (rc == AA_ERR_WORKSPACE && (flags & AA_FLAG_PREMUL_ALPHA)) ? AA_ERR_STRIDES : rc;
  }
  if (img_pitch == 0 && N * (layout == AA_NCHW ? C : 1) > 1) return AA_ERR_STRIDES;  // (a broadcast batch: make it dense)
  return resample_fwd_impl(in_dev, out_dev, nullptr, 0, dtype, layout, N, C, H, W, ax_h, ax_w, flags, row_pitch, img_pitch ? img_pitch : H * row_pitch, stream);
}

size_t aa_workspace_bytes_u8_to_f32(int layout, int64_t N, int64_t C, int64_t H, int64_t W, const aa_axis *ax_h, const aa_axis *ax_w,
                                    const aa_convert *cv) {
  if (!ax_h || !ax_w || !cv || N <= 0) return 0;
  AAProblem q = problem(AA_U8, layout, N, C, H, W, ax_h->out_size, ax_w->out_size, *ax_h, *ax_w, 0u);
  (void)fill_convert(q, *cv);
  return plan_fwd(q).bytes();
}

int aa_resample_fwd_u8_to_f32(const void *in_dev, void *out_dev, void *workspace_dev, size_t workspace_bytes, int layout,
                              int64_t N, int64_t C, int64_t H, int64_t W, const aa_axis *ax_h, const aa_axis *ax_w,
                              const aa_convert *cv, aa_stream_t stream) {
  if (layout != AA_NCHW && layout != AA_NHWC) return AA_ERR_BAD_LAYOUT;
  if (N < 0 || C <= 0 || H <= 0 || W <= 0) return AA_ERR_BAD_SHAPE;
  int rc = check_axis(ax_h, H);
  if (rc != AA_OK) return rc;
  rc = check_axis(ax_w, W);
  if (rc != AA_OK) return rc;
  if (ax_h->kind != AA_TABLE_F32 || ax_w->kind != AA_TABLE_F32) return AA_ERR_BAD_DTYPE;  // float output = float arithmetic
  if (!cv) return AA_ERR_NULL;
  AAProblem q = problem(AA_U8, layout, N, C, H, W, ax_h->out_size, ax_w->out_size, *ax_h, *ax_w, 0u);
  rc = fill_convert(q, *cv);
  if (rc != AA_OK) return rc;
  return resample(q, in_dev, out_dev, workspace_dev, workspace_bytes, stream);
}

size_t aa_workspace_bytes_bwd(int dtype, int layout, int64_t N, int64_t C, int64_t H, int64_t W, int64_t oH, int64_t oW) {
  (void)layout; (void)H; (void)oW;
  if (N <= 0) return 0;
  // gather form: intermediate [N,C,oH,W]; scatter form: intermediate [N,C,H,oW]; size for the larger
  const size_t elem = dtype == AA_F64 ? 8 : 4;
  const size_t a = (size_t)N * C * oH * W, b = (size_t)N * C * H * oW;
  return aa_align16((a > b ? a : b) * elem);
}

int aa_resample_bwd(const void *grad_out_dev, void *grad_in_dev, void *workspace_dev, size_t workspace_bytes, int dtype,
                    int layout, int64_t N, int64_t C, int64_t H, int64_t W, const aa_axis *tr_h, const aa_axis *tr_w,
                    aa_stream_t stream) {
  // 16-bit gradients: storage types, as 16-bit images are in the forward (fp32 arithmetic with AA_TABLE_F32 tables, fp32 intermediate,
  // one rounding at the store); any other table kind is refused by the forward's own check below
  if (dtype != AA_F32 && dtype != AA_F64 && dtype != AA_F16 && dtype != AA_BF16) return AA_ERR_BAD_DTYPE;
  if (!tr_h || !tr_w) return AA_ERR_NULL;
  // The adjoint in gather form IS a forward resample of grad_out [N,C,oH,oW] with the transposed tables
  // (tr_w: oW -> W, tr_h: oH -> H); the two 1-D adjoints act on different axes and commute.
  if (tr_h->out_size != H || tr_w->out_size != W) return AA_ERR_BAD_SHAPE;
  return aa_resample_fwd(grad_out_dev, grad_in_dev, workspace_dev, workspace_bytes, dtype, layout, N, C, tr_h->in_size,
                         tr_w->in_size, tr_h, tr_w, stream);
}

int aa_resample_bwd_atomic(const void *grad_out_dev, void *grad_in_dev, void *workspace_dev, size_t workspace_bytes,
                           int dtype, int layout, int64_t N, int64_t C, int64_t H, int64_t W, const aa_axis *ax_h,
                           const aa_axis *ax_w, aa_stream_t stream) {
  // (16-bit gradients have the gather form only: atomic adds that round to 16 bits one by one are a different and worse result)
  if (dtype != AA_F32 && dtype != AA_F64) return AA_ERR_BAD_DTYPE;
  if (layout != AA_NCHW && layout != AA_NHWC) return AA_ERR_BAD_LAYOUT;
  if (N < 0 || C <= 0 || H <= 0 || W <= 0) return AA_ERR_BAD_SHAPE;
  int rc = check_axis(ax_h, H);
  if (rc != AA_OK) return rc;
  rc = check_axis(ax_w, W);
  if (rc != AA_OK) return rc;
  rc = check_dtype_kind(dtype, ax_h->kind, ax_w->kind);
  if (rc != AA_OK) return rc;
  if (N == 0) {
    g_last_variant = "empty";
    return AA_OK;
  }
  if (!grad_out_dev || !grad_in_dev) return AA_ERR_NULL;
  const size_t need = aa_workspace_bytes_bwd(dtype, layout, N, C, H, W, ax_h->out_size, ax_w->out_size);
  if (!workspace_dev || workspace_bytes < need) return AA_ERR_WORKSPACE;
  AAProblem q = problem(dtype, layout, N, C, H, W, ax_h->out_size, ax_w->out_size, *ax_h, *ax_w, 0u);
  q.in = grad_out_dev; q.out = grad_in_dev; q.ws = workspace_dev; q.ws_bytes = workspace_bytes;
  q.stream = (hipStream_t)stream;
  rc = aa_launch_bwd_atomic(q);
  if (rc == AA_OK) g_last_variant = "bwd_scatter_atomics";
  g_last_shape.valid = false;
  return rc;
}

int aa_resample_axis_fwd(const void *in_dev, void *out_dev, int dtype, int64_t outer, int64_t in_size, int64_t inner,
                         const aa_axis *ax, aa_stream_t stream) {
  if (dtype < AA_U8 || dtype > AA_BF16) return AA_ERR_BAD_DTYPE;
  if (outer < 0 || in_size <= 0 || inner <= 0) return AA_ERR_BAD_SHAPE;
  int rc = check_axis(ax, in_size);
  if (rc != AA_OK) return rc;
  if (dtype == AA_U8 && ax->kind != AA_TABLE_PIL) return AA_ERR_BAD_DTYPE;
  rc = check_dtype_kind(dtype, ax->kind, ax->kind);
  if (rc != AA_OK) return rc;
  if (outer == 0) return AA_OK;
  if (!in_dev || !out_dev) return AA_ERR_NULL;
  g_last_variant = "generic_axis";
  g_last_shape.valid = false;
  return aa_launch_axis_fwd(in_dev, out_dev, dtype, outer, in_size, inner, *ax, (hipStream_t)stream);
}

int aa_probe_copy(const void *src_dev, void *dst_dev, size_t bytes, int form, aa_stream_t stream) {
  if (!src_dev || !dst_dev) return AA_ERR_NULL;
  if ((((uintptr_t)src_dev | (uintptr_t)dst_dev) & 15) != 0 || form < 0 || form > 5) return AA_ERR_BAD_SHAPE;
  return aa_launch_probe_copy(src_dev, dst_dev, bytes, form, (hipStream_t)stream);
}

int aa_set_fused(int enabled) {
  const int prev = g_fused_enabled;
  // 0 generic two-pass, 1 auto (newest fused design first), 2 first-generation fused kernels only
  g_fused_enabled = (enabled < 0 || enabled > 2) ? 1 : enabled;
  return prev;
}

int aa_set_store_form(int form) {
  const int prev = g_aa_store_form;
  g_aa_store_form = (form < -1 || form > 1) ? -1 : form;
  return prev;
}

int aa_set_plane_groups(int enabled) {
  const int prev = g_aa_plane_groups;
  g_aa_plane_groups = enabled ? 1 : 0;
  return prev;
}

const char *aa_last_variant(void) { return g_last_variant; }

int aa_last_launch_shape(aa_launch_shape_in *in, aa_launch_shape_out *out) {
  if (!in || !out) return AA_ERR_NULL;
  if (!g_last_shape.valid) return AA_ERR_BAD_SHAPE;
  *in = g_last_shape.in;
  *out = g_last_shape.out;
  return AA_OK;
}

}  // extern "C"
