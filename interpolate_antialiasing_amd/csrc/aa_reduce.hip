// aa_reduce.hip — Pillow's Image.reduce for 8-bit channels (ImagingReduce): every output pixel is the rounded mean of an fx x fy block
// of input pixels.  The first step of Image.resize(reducing_gap=...): a large frame is read ONCE by an integer box sum (about one add per
// byte, no weights) before the real filter runs over the small result.
//
// One kernel, bound by its input stream.  A workgroup of 256 lanes owns a TILE: one image (or plane), one output row Y, and a run of
// output columns whose input bytes are at most kTile = 4096 per row, i.e. ONE 16-byte piece per lane and row.
//   vertical:   every lane reads its piece of each of the block's fy rows with one 16-byte load (the row is read as one contiguous
//               segment: lane i at tile_start + 16 i) and adds the 16 bytes column-wise.  Even and odd bytes of a dword are summed as
//               packed 16-bit pairs (two ANDs, a shift and two adds per four bytes), emptied into 32-bit sums every 256 rows.
//   horizontal: the 16 column sums of every lane go to LDS (slots swizzled so that the 16-byte writes do not meet on a bank: colsum_at),
//               and every output byte adds its fx entries, C apart.
//   store:      out = ((ss + n/2) * mult(n)) >> 24, n = the pixels really in the block; mult comes from the host (four values per launch:
//               full block, right edge, bottom edge, corner).
// The tile starts at the box's own first byte, whatever its alignment (crops at odd byte offsets are read where they lie); only the piece
// that holds the END of the box's row is ever partial: it is loaded whole and masked where the 16 bytes still lie inside the box's row,
// and byte by byte where they would pass its end (the last row of a tensor ends the allocation).
// Blocks wider than a tile (fx * C > 4096: one output pixel per tile) run the same code over several CHUNKS of the row, one thread per
// output byte carrying its sum from chunk to chunk.
// FX > 0: fx at compile time (the horizontal sum unrolls); FX == 0: fx at run time.  The set is listed at AA_REDUCE_FX below.

#include "aa_reduce.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = kThreads * 16;  // bytes of one row a tile (a chunk) holds

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

struct __attribute__((packed, aligned(1))) Piece { uint32_t v[4]; };

// Where column sum i (one dword per input byte of the tile) lives in LDS.  A lane parks 16 consecutive sums = four 16-byte slots, and a
// plain layout puts lanes l, l + 4, l + 8, l + 12 on the same banks (a slot is 4 of the 64 banks; 16 dwords per lane wrap every 4 lanes):
// a 4-way conflict on every ds_write_b128.  So the slot's low two bits are XORed with bits 4-5 of the slot number (= bits 2-3 of the
// lane): the 16 lanes of a write group then cover all 16 slots of a bank row.  A bijection inside each group of 4 slots.
__device__ inline int colsum_at(int i) {
  const int slot = i >> 2;
  return (((slot & ~3) | ((slot ^ (slot >> 4)) & 3)) << 2) | (i & 3);
}

template <int FX>
__global__ void __launch_bounds__(kThreads) reduce_u8_kernel(ReduceParams p) {
  __shared__ __attribute__((aligned(16))) uint32_t colsum[kTile];
  const int tid = threadIdx.x;
  const int C = p.C;
  const int fx = FX > 0 ? FX : p.fx;
  const int xt = blockIdx.x % p.xtiles;
  const long long rest = blockIdx.x / p.xtiles;
  const int Y = (int)(rest % p.oh);
  const long long img = rest / p.oh;

  const int X0 = xt * p.sx;
  const int X1 = X0 + p.sx < p.ow ? X0 + p.sx : p.ow;
  const int nout = (X1 - X0) * C;  // output bytes of the tile
  const long long px0 = (long long)X0 * fx;
  const long long px1 = (long long)X1 * fx < p.bw ? (long long)X1 * fx : p.bw;
  const long long tile_b0 = px0 * C;                   // first byte of the tile in the box's row
  const long long TB = (px1 - px0) * C;                // bytes of the tile per row
  const long long row_left = (long long)p.bw * C - tile_b0;  // bytes from the tile's start to the end of the box's row
  const int r0 = Y * p.fy;
  const int r1 = r0 + p.fy < p.bh ? r0 + p.fy : p.bh;
  const int rows = r1 - r0;
  const uint8_t *src = p.in + img * p.img_pitch + (long long)r0 * p.row_pitch + tile_b0;
  const bool one_chunk = TB <= kTile;

  unsigned carry = 0;  // (several chunks: nout <= 4, thread tid carries output byte tid)
  for (long long cb = 0; cb < TB; cb += kTile) {
    const long long ce = cb + kTile < TB ? cb + kTile : TB;
    // ---- vertical: 16 column sums per lane
    uint32_t s[16];
#pragma unroll
    for (int j = 0; j < 16; j++) s[j] = 0;
    const long long start = cb + 16ll * tid;
    const int nvalid = start >= ce ? 0 : (ce - start >= 16 ? 16 : (int)(ce - start));
    if (nvalid > 0) {
      const bool whole = start + 16 <= row_left;  // the 16 bytes lie inside the box's row: one load, masked below
      const uint8_t *q = src + start;
      for (int rb = 0; rb < rows; rb += 256) {
        const int re = rb + 256 < rows ? rb + 256 : rows;
        uint32_t e[4] = {0, 0, 0, 0}, o[4] = {0, 0, 0, 0};
        if (whole) {
#pragma unroll 4
          for (int r = rb; r < re; r++) {
            Piece pc;
            __builtin_memcpy(&pc, q + (long long)r * p.row_pitch, 16);
#pragma unroll
            for (int d = 0; d < 4; d++) {
              e[d] += pc.v[d] & 0x00FF00FFu;
              o[d] += (pc.v[d] >> 8) & 0x00FF00FFu;
            }
          }
        } else {  // the piece that holds the end of the box's row: its valid bytes one by one
          for (int r = rb; r < re; r++) {
            const uint8_t *qr = q + (long long)r * p.row_pitch;
            for (int j = 0; j < nvalid; j++) {
              const uint32_t b = qr[j];
              const int d = j >> 2, k = j & 3;
              if (k & 1) o[d] += b << (8 * (k - 1));
              else e[d] += b << (8 * k);
            }
          }
        }
#pragma unroll
        for (int d = 0; d < 4; d++) {
          s[4 * d + 0] += e[d] & 0xFFFFu;
          s[4 * d + 1] += o[d] & 0xFFFFu;
          s[4 * d + 2] += e[d] >> 16;
          s[4 * d + 3] += o[d] >> 16;
        }
      }
    }
#pragma unroll
    for (int d = 0; d < 4; d++) {  // (bytes of a whole load beyond the chunk: dropped here)
      uint4 v;
      v.x = 4 * d + 0 < nvalid ? s[4 * d + 0] : 0u;
      v.y = 4 * d + 1 < nvalid ? s[4 * d + 1] : 0u;
      v.z = 4 * d + 2 < nvalid ? s[4 * d + 2] : 0u;
      v.w = 4 * d + 3 < nvalid ? s[4 * d + 3] : 0u;
      *(uint4 *)&colsum[colsum_at(16 * tid + 4 * d)] = v;
    }
    __syncthreads();
    // ---- horizontal: output byte idx = (X - X0) * C + c adds its fx entries, C apart
    for (int idx = tid; idx < nout; idx += kThreads) {
      const int j = idx / C, c = idx - j * C;
      const long long X = (long long)X0 + j;
      const long long left = (long long)p.bw - X * fx;
      const int fxe = left < fx ? (int)left : fx;  // pixels of this block (the last column of blocks may be partial)
      const long long pj = (long long)j * fx * C + c;  // tile byte of the block's first entry
      unsigned ss = 0;
      if (FX > 0 && one_chunk && fxe == FX) {
#pragma unroll
        for (int k = 0; k < (FX > 0 ? FX : 1); k++) ss += colsum[colsum_at((int)pj + k * C)];
      } else {
        const long long k_lo = pj >= cb ? 0 : (cb - pj + C - 1) / C;
        long long k_hi = ce > pj ? (ce - pj + C - 1) / C : 0;
        if (k_hi > fxe) k_hi = fxe;
        for (long long k = k_lo; k < k_hi; k++) ss += colsum[colsum_at((int)(pj + k * C - cb))];
      }
      if (one_chunk) {
        const unsigned n = (unsigned)fxe * (unsigned)rows;
        const unsigned m = rows != p.fy ? (fxe != fx ? p.mult[3] : p.mult[2]) : (fxe != fx ? p.mult[1] : p.mult[0]);
        p.out[((img * p.oh + Y) * (long long)p.ow + X0) * C + idx] = (uint8_t)(((ss + n / 2) * m) >> 24);
      } else {
        carry += ss;
      }
    }
    __syncthreads();
  }
  if (!one_chunk && tid < nout) {
    const int j = tid / C;
    const long long X = (long long)X0 + j;
    const long long left = (long long)p.bw - X * fx;
    const int fxe = left < fx ? (int)left : fx;
    const unsigned n = (unsigned)fxe * (unsigned)rows;
    const unsigned m = rows != p.fy ? (fxe != fx ? p.mult[3] : p.mult[2]) : (fxe != fx ? p.mult[1] : p.mult[0]);
    p.out[((img * p.oh + Y) * (long long)p.ow + X0) * C + tid] = (uint8_t)(((carry + n / 2) * m) >> 24);
  }
}

// Pillow's division_UINT32(n, 8): a float32 division
unsigned reduce_mult(unsigned n) { return (unsigned)(4294967296.0f / (float)(256u * n)); }

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
  p.sx = block_bytes <= kTile ? (int)(kTile / block_bytes) : 1;
  p.xtiles = (p.ow + p.sx - 1) / p.sx;
  const unsigned fxr = job.bw % job.fx ? job.bw % job.fx : job.fx, fyb = job.bh % job.fy ? job.bh % job.fy : job.fy;
  p.mult[0] = reduce_mult((unsigned)job.fx * job.fy);
  p.mult[1] = reduce_mult(fxr * job.fy);
  p.mult[2] = reduce_mult((unsigned)job.fx * fyb);
  p.mult[3] = reduce_mult(fxr * fyb);
  const long long blocks = job.images * p.oh * (long long)p.xtiles;
  if (blocks <= 0) return AA_OK;
  if (blocks > 0x7FFFFFFFll) return AA_ERR_BAD_SHAPE;
  switch (block_bytes <= kTile ? job.fx : 0) {
#define X(F) \
    case F: hipLaunchKernelGGL(reduce_u8_kernel<F>, dim3((unsigned)blocks), dim3(kThreads), 0, job.stream, p); break;
    AA_REDUCE_FX(X)
#undef X
    default: hipLaunchKernelGGL(reduce_u8_kernel<0>, dim3((unsigned)blocks), dim3(kThreads), 0, job.stream, p); break;
  }
  AA_HIP_CHECK_LAUNCH();
  return AA_OK;
}
