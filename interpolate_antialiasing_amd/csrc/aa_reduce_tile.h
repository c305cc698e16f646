// aa_reduce_tile.h — the ONE statement of Image.reduce's 8-bit arithmetic on the device: the body of a tile, which the dense kernel
// (aa_reduce.hip: one box size and one factor per launch) and the ragged kernel (aa_reduce_many.hip: a record per item) both
// instantiate.  A kernel says where its tile lies; everything from the first load to the last store is here.
//
// A workgroup of 256 lanes owns a TILE: one image (or plane), one output row Y, and a run of output columns [X0, X1) whose input bytes
// are at most kReduceTile = 4096 per row, i.e. ONE 16-byte piece per lane and row.
//   vertical:   every lane reads its piece of each of the block's rows with one 16-byte load (the row is read as one contiguous
//               segment: lane i at tile_start + 16 i) and adds the 16 bytes column-wise.  Even and odd bytes of a dword are summed as
//               packed 16-bit pairs (two ANDs, a shift and two adds per four bytes), emptied into 32-bit sums every 256 rows.
//   horizontal: the 16 column sums of every lane go to LDS (slots swizzled so that the 16-byte writes do not meet on a bank:
//               reduce_colsum_at), and every output byte adds its fx entries, C apart.
//   store:      out = ((ss + n/2) * mult(n)) >> 24, n = the pixels really in the block; mult comes from the host (four values per box
//               and factor: full block, right edge, bottom edge, corner).
// The tile starts at the box's own first byte, whatever its alignment (crops at odd byte offsets are read where they lie); only the piece
// that holds the END of the box's row is ever partial: it is loaded whole and masked where the 16 bytes still lie inside the box's row,
// and byte by byte where they would pass its end (the last row of a tensor ends the allocation).
// Blocks wider than a tile (fx * C > 4096: one output pixel per tile) run the same code over several CHUNKS of the row, one thread per
// output byte carrying its sum from chunk to chunk.
#pragma once

#include "aa_common.h"

constexpr int kReduceThreads = 256;
constexpr int kReduceTile = kReduceThreads * 16;  // bytes of one row a tile (a chunk) holds

struct __attribute__((packed, aligned(1))) ReducePiece { uint32_t v[4]; };

// Pillow's division_UINT32(n, 8): a float32 division
inline unsigned reduce_mult(unsigned n) { return (unsigned)(4294967296.0f / (float)(256u * n)); }

// Output columns per tile and tiles per output row, for blocks of fx pixels of C bytes.
inline int reduce_tile_columns(int fx, int C) {
  const long long block_bytes = (long long)fx * C;
  return block_bytes <= kReduceTile ? (int)(kReduceTile / block_bytes) : 1;
}

// Where column sum i (one dword per input byte of the tile) lives in LDS.  A lane parks 16 consecutive sums = four 16-byte slots, and a
// plain layout puts lanes l, l + 4, l + 8, l + 12 on the same banks (a slot is 4 of the 64 banks; 16 dwords per lane wrap every 4 lanes):
// a 4-way conflict on every ds_write_b128.  So the slot's low two bits are XORed with bits 4-5 of the slot number (= bits 2-3 of the
// lane): the 16 lanes of a write group then cover all 16 slots of a bank row.  A bijection inside each group of 4 slots.
__device__ inline int reduce_colsum_at(int i) {
  const int slot = i >> 2;
  return (((slot & ~3) | ((slot ^ (slot >> 4)) & 3)) << 2) | (i & 3);
}

// One tile.  src: the byte (first row of the block, column X0 * fx, channel 0) of the box; dst: the output byte (Y, X0, channel 0);
// bw: the box's width in pixels; rows: the rows really in the block (fy, or fewer in the last row of blocks: rows_partial);
// mult[(partial in x) + 2 * (partial in y)].  FX > 0: fx at compile time (the horizontal sum unrolls); FX == 0: fx at run time.
// colsum: kReduceTile dwords of LDS, 16-byte aligned.  Every lane of the workgroup calls it (it synchronises).
template <int FX>
__device__ __forceinline__ void reduce_tile(uint32_t *colsum, const uint8_t *src, uint8_t *dst, long long row_pitch, int C, int fx_rt, int bw,
                                            int X0, int X1, int rows, bool rows_partial, unsigned m_full, unsigned m_right, unsigned m_bottom,
                                            unsigned m_corner) {
  const int tid = threadIdx.x;
  const int fx = FX > 0 ? FX : fx_rt;
  const int nout = (X1 - X0) * C;  // output bytes of the tile
  const long long px0 = (long long)X0 * fx;
  const long long px1 = (long long)X1 * fx < bw ? (long long)X1 * fx : bw;
  const long long tile_b0 = px0 * C;                       // first byte of the tile in the box's row
  const long long TB = (px1 - px0) * C;                    // bytes of the tile per row
  const long long row_left = (long long)bw * C - tile_b0;  // bytes from the tile's start to the end of the box's row
  const bool one_chunk = TB <= kReduceTile;

  unsigned carry = 0;  // (several chunks: nout <= 4, thread tid carries output byte tid)
  for (long long cb = 0; cb < TB; cb += kReduceTile) {
    const long long ce = cb + kReduceTile < TB ? cb + kReduceTile : TB;
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
            ReducePiece pc;
            __builtin_memcpy(&pc, q + (long long)r * row_pitch, 16);
#pragma unroll
            for (int d = 0; d < 4; d++) {
              e[d] += pc.v[d] & 0x00FF00FFu;
              o[d] += (pc.v[d] >> 8) & 0x00FF00FFu;
            }
          }
        } else {  // the piece that holds the end of the box's row: its valid bytes one by one
          for (int r = rb; r < re; r++) {
            const uint8_t *qr = q + (long long)r * row_pitch;
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
      *(uint4 *)&colsum[reduce_colsum_at(16 * tid + 4 * d)] = v;
    }
    __syncthreads();
    // ---- horizontal: output byte idx = (X - X0) * C + c adds its fx entries, C apart
    for (int idx = tid; idx < nout; idx += kReduceThreads) {
      const int j = idx / C, c = idx - j * C;
      const long long X = (long long)X0 + j;
      const long long left = (long long)bw - X * fx;
      const int fxe = left < fx ? (int)left : fx;  // pixels of this block (the last column of blocks may be partial)
      const long long pj = (long long)j * fx * C + c;  // tile byte of the block's first entry
      unsigned ss = 0;
      if (FX > 0 && one_chunk && fxe == FX) {
#pragma unroll
        for (int k = 0; k < (FX > 0 ? FX : 1); k++) ss += colsum[reduce_colsum_at((int)pj + k * C)];
      } else {
        const long long k_lo = pj >= cb ? 0 : (cb - pj + C - 1) / C;
        long long k_hi = ce > pj ? (ce - pj + C - 1) / C : 0;
        if (k_hi > fxe) k_hi = fxe;
        for (long long k = k_lo; k < k_hi; k++) ss += colsum[reduce_colsum_at((int)(pj + k * C - cb))];
      }
      if (one_chunk) {
        const unsigned n = (unsigned)fxe * (unsigned)rows;
        const unsigned m = rows_partial ? (fxe != fx ? m_corner : m_bottom) : (fxe != fx ? m_right : m_full);
        dst[idx] = (uint8_t)(((ss + n / 2) * m) >> 24);
      } else {
        carry += ss;
      }
    }
    __syncthreads();
  }
  if (!one_chunk && tid < nout) {
    const int j = tid / C;
    const long long X = (long long)X0 + j;
    const long long left = (long long)bw - X * fx;
    const int fxe = left < fx ? (int)left : fx;
    const unsigned n = (unsigned)fxe * (unsigned)rows;
    const unsigned m = rows_partial ? (fxe != fx ? m_corner : m_bottom) : (fxe != fx ? m_right : m_full);
    dst[tid] = (uint8_t)(((carry + n / 2) * m) >> 24);
  }
}
