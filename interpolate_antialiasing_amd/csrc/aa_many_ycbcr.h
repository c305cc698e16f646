// aa_many_ycbcr.h — subsampled YCbCr planes to an RGB batch for the ragged call (include/aa_interp.h, aa_many_plan_ycbcr).  The plan
// COMPOSES placed plans of aa_many.h: a plane is an ordinary single-channel item and an interleaved chroma pair an ordinary two-channel
// interleaved item, each with its own box, hull and tables, all items of one image with the SAME place.  The packed block:
//   [ AAYccHeader : 64 B ][ plan A : a placed plan of aa_many.h ][ plan B : likewise, interleaved chroma only ]
//   planar chroma       plan A = 3 n single-channel items: item i is Y_i, n + i is Cb_i, 2 n + i is Cr_i; no plan B
//   interleaved chroma  plan A = the n luma items; plan B = the n chroma pairs (C = 2, interleaved pixels), its workspace after A's
// Launches whatever n: plan A's table kernel and horizontal pass, plan B's (interleaved only), and ONE converting vertical pass:
// three when the chroma is planar, five when it is interleaved.
#pragma once

#include "aa_common.h"
#include "aa_many.h"

#define AA_YCC_MAGIC 0x43435941  // 'AYCC'
#define AA_YCC_VROWS 4           // canvas rows per workgroup of the vertical pass: one wave each
#define AA_YCC_VCOLS 256         // canvas columns per workgroup: 64 lanes x 4 pixels

struct AAYccHeader {
  int32_t magic, n, oH, oW, filter;
  int32_t interleaved;  // 1: plan B holds the chroma pairs
  int32_t flips;        // 1 when some item has AA_MANY_FLIP_X
  uint32_t fill;        // R | G << 8 | B << 16
  int64_t off_a, off_b; // byte offsets of the two plans in the block (off_b 0: none)
  int64_t ws_b;         // byte offset of plan B's workspace in the workspace
  int64_t ws_bytes;
};
static_assert(sizeof(AAYccHeader) == 64, "descriptor header is 64 bytes");

size_t aa_ycc_desc_size(int64_t n);
int aa_ycc_plan_host(int filter, int64_t n, int64_t oH, int64_t oW, const aa_ycbcr_image *images, const aa_many_place *places,
                     const uint8_t *fill, void *desc_host, size_t desc_bytes, size_t *workspace_bytes);
// out_elem AA_U8 (Pillow's bytes) or AA_F32 / AA_F16 / AA_BF16 (aa_launch_many_float's conversion of them)
int aa_launch_many_ycbcr(const void *desc_host, const void *desc_dev, void *out_dev, void *workspace_dev, size_t workspace_bytes, int out_elem,
                         int out_layout, int normalize, const float *mean, const float *std, hipStream_t stream);
