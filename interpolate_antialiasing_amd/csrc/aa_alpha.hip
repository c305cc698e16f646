// aa_alpha.hip — the three-step straight-alpha fallback (AA_FLAG_PREMUL_ALPHA wherever no fused ALPHA instantiation applies: LA, planar
// RGBA, wide / split windows, growing heights, aa_set_fused(0)): premultiply the image into the workspace, resample that with the
// ordinary Pillow-arithmetic path, un-premultiply the output in place.  One thread per pixel: channels_last RGBA moves the pixel as one
// dword; otherwise the alpha byte is read once and the colour bytes of the pixel follow it (C - 1 of them; interleaved, or one per plane).

#include "aa_alpha.h"
#include "aa_common.h"

namespace {

// pixel i of image n: colour channel c at base + c * cstep, alpha at base + (C - 1) * cstep  (src == dst when un-premultiplying: no __restrict__)
template <bool PREMUL>
__global__ void __launch_bounds__(256) alpha_convert_kernel(const uint8_t *src, uint8_t *dst, int64_t n_px,
                                                            int64_t hw, int C, int nhwc) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_px; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = i / hw, px = i - n * hw;
    const int64_t base = nhwc ? i * C : n * C * hw + px;
    const int64_t cstep = nhwc ? 1 : hw;
    const int a = src[base + (C - 1) * cstep];
    for (int c = 0; c < C - 1; c++) {
      const int v = src[base + c * cstep];
      dst[base + c * cstep] = (uint8_t)(PREMUL ? aa_premul8(v, a) : aa_unpremul8(v, a));
    }
    if (PREMUL) dst[base + (C - 1) * cstep] = (uint8_t)a;  // (un-premultiplying runs in place: alpha stays where it is)
  }
}

// channels_last RGBA on a 4-byte-aligned tensor: one pixel is one dword
template <bool PREMUL>
__global__ void __launch_bounds__(256) alpha_convert_rgba_kernel(const unsigned *src, unsigned *dst, int64_t n_px) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_px; i += (int64_t)gridDim.x * blockDim.x) {
    const unsigned px = src[i];
    if (PREMUL) {
      dst[i] = aa_premul_px(px);
    } else {
      const int a = (int)(px >> 24);
      dst[i] = (unsigned)aa_unpremul8((int)(px & 0xffu), a) | ((unsigned)aa_unpremul8((int)((px >> 8) & 0xffu), a) << 8) |
               ((unsigned)aa_unpremul8((int)((px >> 16) & 0xffu), a) << 16) | (px & 0xff000000u);
    }
  }
}

template <bool PREMUL>
int launch_convert(const void *src, void *dst, int layout, int64_t N, int64_t C, int64_t H, int64_t W, hipStream_t stream) {
  const int64_t n_px = N * H * W;
  if (n_px <= 0) return AA_OK;
  const int64_t blocks = (n_px + 255) / 256;
  const unsigned grid = (unsigned)(blocks < 65536 ? blocks : 65536);
  if (layout == AA_NHWC && C == 4 && ((((uintptr_t)src | (uintptr_t)dst) & 3) == 0)) {
    hipLaunchKernelGGL(alpha_convert_rgba_kernel<PREMUL>, dim3(grid), dim3(256), 0, stream, (const unsigned *)src, (unsigned *)dst, n_px);
    AA_HIP_CHECK_LAUNCH();
    return AA_OK;
  }
  hipLaunchKernelGGL(alpha_convert_kernel<PREMUL>, dim3(grid), dim3(256), 0, stream, (const uint8_t *)src, (uint8_t *)dst, n_px, H * W,
                     (int)C, layout == AA_NHWC ? 1 : 0);
  AA_HIP_CHECK_LAUNCH();
  return AA_OK;
}

}  // namespace

int aa_launch_premul_u8(const void *src, void *dst, int layout, int64_t N, int64_t C, int64_t H, int64_t W, hipStream_t stream) {
  return launch_convert<true>(src, dst, layout, N, C, H, W, stream);
}

int aa_launch_unpremul_u8(void *img, int layout, int64_t N, int64_t C, int64_t H, int64_t W, hipStream_t stream) {
  return launch_convert<false>(img, img, layout, N, C, H, W, stream);
}
