// aa_reduce.hip — Pillow's Image.reduce for 8-bit channels (ImagingReduce): every output pixel is the rounded mean of an fx x fy block
// of input pixels.  The first step of Image.resize(reducing_gap=...): a large frame is read ONCE by an integer box sum (about one add per
// byte, no weights) before the real filter runs over the small result.
//
// One kernel, bound by its input stream.  A workgroup of 256 lanes owns a TILE: one image (or plane), one output row Y, and a run of
// output columns whose input bytes are at most kReduceTile = 4096 per row.  The kernel only says where its tile lies; the tile's body —
// the vertical sums, the horizontal sums through LDS, the store, the reading rule at the end of the box's row and the chunked form for
// blocks wider than a tile — is reduce_tile (aa_reduce_tile.h), which the ragged kernel (aa_reduce_many.hip) instantiates too.
// FX > 0: fx at compile time (the horizontal sum unrolls); FX == 0: fx at run time.  The set is listed at AA_REDUCE_FX below.

#include "aa_reduce.h"
#include "aa_reduce_tile.h"

namespace {

struct ReduceParams {
  const uint8_t *in;
  uint8_t *out;
  long long row_pitch, img_pitch;  // input, bytes
  int C, bw, bh, fx, fy;
  int ow, oh;
  int sx;       // output columns per tile
  int xtiles;
  unsigned mult[4];  // [(partial in x) + 2 * (partial in y)]
};

template <int FX>
__global__ void __launch_bounds__(kReduceThreads) reduce_u8_kernel(ReduceParams p) {
  __shared__ __attribute__((aligned(16))) uint32_t colsum[kReduceTile];
  const int C = p.C;
  const int fx = FX > 0 ? FX : p.fx;
  const int xt = blockIdx.x % p.xtiles;
  const long long rest = blockIdx.x / p.xtiles;
  const int Y = (int)(rest % p.oh);
  const long long img = rest / p.oh;

  const int X0 = xt * p.sx;
  const int X1 = X0 + p.sx < p.ow ? X0 + p.sx : p.ow;
  const int r0 = Y * p.fy;
  const int r1 = r0 + p.fy < p.bh ? r0 + p.fy : p.bh;
  const int rows = r1 - r0;
  const uint8_t *src = p.in + img * p.img_pitch + (long long)r0 * p.row_pitch + (long long)X0 * fx * C;
  uint8_t *dst = p.out + ((img * p.oh + Y) * (long long)p.ow + X0) * C;
  reduce_tile<FX>(colsum, src, dst, p.row_pitch, C, fx, p.bw, X0, X1, rows, rows != p.fy, p.mult[0], p.mult[1], p.mult[2], p.mult[3]);
}

}  // namespace

// The instantiations: fx at compile time for the factors Image.resize(reducing_gap=2.0 or 3.0) produces most — a thumbnail of a camera or
// video frame is reduced by 2, 3, 4 or 8 — and one run-time form for every other factor (and for blocks wider than a tile).
#define AA_REDUCE_FX(X) X(2) X(3) X(4) X(8)

int aa_launch_reduce_u8(const AAReduceJob &job) {
  ReduceParams p;
  p.in = job.in;
  p.out = job.out;
  p.row_pitch = job.row_pitch;
  p.img_pitch = job.img_pitch;
  p.C = job.C;
  p.bw = job.bw; p.bh = job.bh; p.fx = job.fx; p.fy = job.fy;
  p.ow = (job.bw + job.fx - 1) / job.fx;
  p.oh = (job.bh + job.fy - 1) / job.fy;
  const long long block_bytes = (long long)job.fx * job.C;
  p.sx = reduce_tile_columns(job.fx, job.C);
  p.xtiles = (p.ow + p.sx - 1) / p.sx;
  const unsigned fxr = job.bw % job.fx ? job.bw % job.fx : job.fx, fyb = job.bh % job.fy ? job.bh % job.fy : job.fy;
  p.mult[0] = reduce_mult((unsigned)job.fx * job.fy);
  p.mult[1] = reduce_mult(fxr * job.fy);
  p.mult[2] = reduce_mult((unsigned)job.fx * fyb);
  p.mult[3] = reduce_mult(fxr * fyb);
  const long long blocks = job.images * p.oh * (long long)p.xtiles;
  if (blocks <= 0) return AA_OK;
  if (blocks > 0x7FFFFFFFll) return AA_ERR_BAD_SHAPE;
  switch (block_bytes <= kReduceTile ? job.fx : 0) {
#define X(F) \
    case F: hipLaunchKernelGGL(reduce_u8_kernel<F>, dim3((unsigned)blocks), dim3(kReduceThreads), 0, job.stream, p); break;
    AA_REDUCE_FX(X)
#undef X
    default: hipLaunchKernelGGL(reduce_u8_kernel<0>, dim3((unsigned)blocks), dim3(kReduceThreads), 0, job.stream, p); break;
  }
  AA_HIP_CHECK_LAUNCH();
  return AA_OK;
}
