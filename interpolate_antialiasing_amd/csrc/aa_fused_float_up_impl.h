// aa_fused_float_up_impl.h — fused single-launch resample for fp32 NCHW planes whose height does not shrink (H <= oH):
// the gather form of the true adjoint (aa_resample_bwd = forward resample of grad_out with the transposed tables,
// BASELINE config 5: [.,3,196,320] -> [.,3,438,906]) and forward up-scaling (test.py's 906x438 -> 1200x1200 sizes).
//
// aa_fused_float_impl.h keeps its vertical pass in registers in scatter form, which needs every output row to complete
// once and in order — true when the height shrinks.  When it grows, every input row feeds several output rows and an
// output row needs only the last few input rows, so the vertical pass runs in GATHER form over a small register ring.
// This path is write-bound (4.76 MB out per 0.75 MB in for the backward of config A) and its arithmetic is tiny (2-4 taps
// each way), so what it costs is per-row overhead: round 1's kernel, one output column per lane, spent 48 scalar and 13
// vector instructions per 244-byte row piece (profiles/r02_pmc_bwd_before.json: 261 M SALU vs 69 M VALU per launch).
// Second design (round 2):
//   * a lane computes CPL = 4 (or 2, or 1) NEIGHBOURING output columns, so a wave covers a strip of 256 columns and a
//     finished output row leaves as ONE 1-KiB store instruction (16 bytes per lane): 4x fewer wave-rows, 4x less
//     per-row scalar work per byte;
//   * the 4 windows of a lane overlap (heights and widths grow here), so the lane reads their UNION once per input row
//     (U = taps + spread of 4 neighbouring window starts, measured by the table kernel: header.span4p1) and every output
//     accumulates over the union with its own weights; positions outside an output's own taps are skipped with scalar
//     lane masks exactly as in aa_fused_float_impl.h (never added with a zero weight: no non-finite neighbour leaks in, sums
//     are the reference's bit for bit: tap 0 first, product and sum rounded separately, -ffp-contract=off);
//   * input-row segments are staged into a private G-slot LDS ring by LDS-DMA, the source rounded down to a multiple of
//     four floats OF THE ROW (constant phase of the LDS image, see aa_fused_float_impl.h);
//   * the horizontal-pass results of the KR most recent input rows live in a register ring; an output row is emitted as
//     soon as its last input row has been pushed, so its window is always the ring's LAST ysize entries: the gather is
//     one of KR static unrollings selected by ysize alone; weights come from the table row by scalar loads issued one
//     output row ahead;
//   * output stores and staging DMAs share the in-order vmcnt counter and there are ~2 stores per DMA, so the wave keeps
//     the issue index of every slot's DMA and waits for exactly the operations older than it (a 4-level decision tree).

//
// This header holds the kernel template and launch_k, which launches one instantiation; aa_fused_float_impl.h says where the compiled set,
// the units and the plan live.
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "aa_common.h"

#ifndef AA_UP_DMA_AUX
#define AA_UP_DMA_AUX 0    // cache-policy bits of the staging DMA (developer knob; nt loads are slower: neighbouring strips and bands re-read rows)
#endif
#ifndef AA_UP_PACE
#define AA_UP_PACE 4  // rows between two pacing barriers of a workgroup whose strips share partial sectors (0: none)
#endif
#ifndef AA_UP_ABL
#define AA_UP_ABL 0  // developer ablations (wrong results): 1 no output stores, 2 no input (no DMA, no horizontal pass), 3 stores
                     // of every output row land on row 0 (stay in cache)
#endif

namespace {

typedef __attribute__((address_space(3))) void lds_void;

struct FusedF32UpParams {
  int H, W, oH, oW;
  int ksize_w, ksize_h;
  int ybands, nstrips, strips_per_block, strip_w;
  int nseg, seg_bytes;
  int pace_all;    // experiment: pacing barrier whatever the store mode
  int store_nt;    // output far larger than the caches: wide stores with the streaming (nt) policy.  This path writes 6x what it
                   // reads; with the default policy the written lines push the input rows (re-read by neighbouring strips and
                   // bands) out of L2 / the Infinity Cache and reads queue behind writes: measured -33 % (row pitch a multiple of
                   // 64 B) to -8 % (oW = 906) with nt (profiles/r02_headline_experiments.txt).  2 = rows that are not whole
                   // 64-byte sectors: nt for the whole sectors of a piece only (see the store), a further -5..-25 % for oW = 906
  int gather_off;  // gather section of the H table: one 32-byte record {ymin, ysize, w[6]} per output row
  unsigned long long plane_in_bytes, plane_out_bytes, total_in_bytes, total_out_bytes;
  long long n_groups;  // (plane, band) groups = planes * ybands
};

__device__ inline void wait_vmcnt_up(int n) {  // rounding n DOWN only waits longer; a decision tree, not a chain
  if (n >= 6) {
    if (n >= 16) {
      if (n >= 32) { asm volatile("s_waitcnt vmcnt(32)" ::: "memory"); return; }
      if (n >= 24) { asm volatile("s_waitcnt vmcnt(24)" ::: "memory"); return; }
      asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
      return;
    }
    if (n >= 12) { asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); return; }
    if (n >= 8) { asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); return; }
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    return;
  }
  if (n >= 3) {
    if (n >= 4) { asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); return; }
    asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    return;
  }
  if (n >= 2) { asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); return; }
  if (n >= 1) { asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); return; }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

__device__ inline float select_by_mask_up(float a, float b, unsigned long long mask) {  // mask[lane] ? b : a
  float d;
  asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "s"(mask));
  return d;
}

// 16-bit planes (round 3, template parameter DT): halves are staged and read as halves and converted on the way into the fp32 arithmetic;
// results are rounded once, at the store (= half(reference_fp32(float(x))), like aa_fused_float_impl.h); a lane's CPL results leave as one
// 8-byte store.  The streaming store forms that cut pieces at sector boundaries are fp32-only: 16-bit outputs take the plain forms.
template <int DT> __device__ inline float up_elem_to_f32(unsigned short bits);
template <> __device__ inline float up_elem_to_f32<AA_F16>(unsigned short bits) {
  union { unsigned short u; _Float16 h; } c;
  c.u = bits;
  return (float)c.h;
}
template <> __device__ inline float up_elem_to_f32<AA_BF16>(unsigned short bits) { return __uint_as_float((unsigned)bits << 16); }
template <int DT> __device__ inline unsigned up_f32_to_elem(float a);
template <> __device__ inline unsigned up_f32_to_elem<AA_F16>(float a) {
  union { unsigned short u; _Float16 h; } c;
  c.h = (_Float16)a;
  return c.u;
}
template <> __device__ inline unsigned up_f32_to_elem<AA_BF16>(float a) {  // round to nearest even, NaN stays NaN
  const unsigned u = __float_as_uint(a);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x0040u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// U: floats a lane reads per input row (the union of its CPL windows); G: staged rows; KR: vertical taps kept in registers
// (>= max ysize of the H table); CPL: neighbouring output columns per lane (a strip is 64 * CPL columns).
template <int U, int G, int KR, int CPL, int DT = AA_F32>
__global__ void __launch_bounds__(512)
fused_f32_nchw_up_kernel(const void *__restrict__ in, void *__restrict__ out, const char *__restrict__ tab_w,
                         const char *__restrict__ tab_h, const FusedF32UpParams p) {
  constexpr int ES = DT == AA_F32 ? 4 : 2;  // element bytes
  constexpr int EPP = 16 / ES;              // elements per staged 16-byte piece
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];

  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // XCD-aware index mapping (see aa_fused_u8_v3_impl.h): workgroup id = 8 * k + xcd; within an XCD consecutive k walk
  // the strips of one (plane, band) group first, so neighbouring strips meet in the same L2
  const int sgroups = (p.nstrips + p.strips_per_block - 1) / p.strips_per_block;
  const int xcd = blockIdx.x & 7, k = blockIdx.x >> 3;
  const int strip = (k % sgroups) * p.strips_per_block + wv;
  const long long grp = (long long)(k / sgroups) * 8 + xcd;
  if (grp >= p.n_groups) return;  // the grid is padded to whole rounds of 8 groups
  if (strip >= p.nstrips) return;
  const int yb = (int)(grp % p.ybands);
  const int plane = (int)(grp / p.ybands);  // n * C + c
  // store_nt == 3 (sector-aligned pieces, see the store): strips advance by 240 columns and start 16 columns early, so a wave
  // holds every column its row-dependent 960-byte piece can need; columns outside the row are duplicates and never stored
  const bool aln = p.store_nt == 3;
  const int ox0 = aln ? strip * 240 - 16 : strip * p.strip_w;
  const int bw = aln ? 256 : min(p.strip_w, p.oW - ox0);
  const int oy0 = (int)((long long)yb * p.oH / p.ybands);
  const int oy1 = (int)((long long)(yb + 1) * p.oH / p.ybands);

  const int32_t *__restrict__ xmin_w = (const int32_t *)(tab_w + aa_table_xmin_off());
  const int32_t *__restrict__ xsize_w = (const int32_t *)(tab_w + aa_table_xsize_off(p.oW));
  const float *__restrict__ kw = (const float *)(tab_w + aa_table_w_off(p.oW));
  const int32_t *__restrict__ ymin_h = (const int32_t *)(tab_h + aa_table_xmin_off());
  const int32_t *__restrict__ ysize_h = (const int32_t *)(tab_h + aa_table_xsize_off(p.oH));

  const int r_begin = __builtin_amdgcn_readfirstlane(ymin_h[oy0]);
  const int ylm = __builtin_amdgcn_readfirstlane(ymin_h[oy1 - 1]);
  const int yls = __builtin_amdgcn_readfirstlane(ysize_h[oy1 - 1]);
  const int r_stop = ylm + (yls > 1 ? yls : 1);  // one past the last input row this band reads

  // ---- per-lane horizontal-pass state: CPL outputs sharing one union window of U floats ------------------------------
  const int col0 = lane * CPL;                 // first column of the lane inside the strip
  const bool any_active = col0 < bw;
  int oxb = ox0 + (any_active ? col0 : 0);  // (lanes beyond the strip duplicate lane 0 and never store)
  oxb = oxb < 0 ? 0 : (oxb < p.oW ? oxb : p.oW - 1);
  int ustart;  // row position of the union window's first float
  {
    const int xm0 = xmin_w[oxb];
    int hi = p.W - U;  // right-align a union that would leave the row
    hi = hi > 0 ? hi : 0;
    ustart = xm0 < hi ? xm0 : hi;
  }
  float wreg[CPL][U];
  unsigned long long inwin[CPL][U];  // lane masks (scalar registers): union position q is one of output e's own taps
#pragma unroll
  for (int e = 0; e < CPL; e++) {
    int oxe = ox0 + col0 + e;  // (columns outside the row compute a duplicate, never stored)
    oxe = (!any_active || oxe < 0) ? oxb : (oxe < p.oW ? oxe : p.oW - 1);
    const int xm = xmin_w[oxe];
    int xs = xsize_w[oxe];
    xs = xs > 1 ? xs : 1;  // tap 0 is unconditional in the reference (s2.2:68-73)
    const int t0 = xm - ustart;  // union position of the reference's tap 0 (>= 0: window starts do not decrease)
#pragma unroll
    for (int q = 0; q < U; q++) {
      const int j = q - t0;
      const bool mine = j >= 0 && j < xs;
      wreg[e][q] = (mine && j < p.ksize_w) ? kw[(size_t)oxe * p.ksize_w + j] : 0.0f;
      inwin[e][q] = __ballot(mine);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // from here on vmcnt counts staging DMAs and output stores only
  const int seg0 = __builtin_amdgcn_readfirstlane(ustart) & ~(EPP - 1);  // lane 0 holds the strip's leftmost window
  const unsigned lane_lds = (unsigned)(wv * G * p.seg_bytes + (ustart - seg0) * ES);

  const unsigned long long plane_off = (unsigned long long)plane * p.plane_in_bytes;
  unsigned long long remaining = p.total_in_bytes - plane_off;
  if (remaining > 0xFFFFFFFCull) remaining = 0xFFFFFFFCull;
  const __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc((void *)((const uint8_t *)in + plane_off), 0, (unsigned)remaining, 0x00020000);
  const unsigned row_bytes = (unsigned)p.W * (unsigned)ES;
  const int lds_base = wv * G * p.seg_bytes;
  const bool dma_lane = lane < p.nseg;  // nseg <= 64 (checked on the host)
  const unsigned voff = (unsigned)lane * 16u;

  const unsigned long long out_off = (unsigned long long)plane * p.plane_out_bytes;
  unsigned long long out_rem = p.total_out_bytes - out_off;
  if (out_rem > 0xFFFFFFFFull) out_rem = 0xFFFFFFFFull;
  const __amdgpu_buffer_rsrc_t orsrc =
      __builtin_amdgcn_make_buffer_rsrc((void *)((uint8_t *)out + out_off), 0, (unsigned)out_rem, 0x00020000);
  const unsigned out_row_bytes = (unsigned)p.oW * (unsigned)ES;
  const unsigned store_voff = (unsigned)(ox0 + col0) * (unsigned)ES;
  const bool full_lane = col0 + CPL <= bw;  // all CPL columns of the lane exist: one wide store
  const unsigned phase0 = (unsigned)(((unsigned long long)(uintptr_t)out + out_off + (unsigned long long)ox0 * 4u) & 127u);

  const unsigned a_base = (unsigned)seg0 * (unsigned)ES;  // byte offset (from the plane) of the strip's segment in row 0
  // sector-aligned pieces: this wave's 1088-byte staging area behind the workgroup's stage rings; float phase of the plane in
  // the 64-byte sector grid
  const unsigned aln_lds = (unsigned)(p.strips_per_block * G * p.seg_bytes + wv * 1088);
  const unsigned phase0f = (unsigned)((((unsigned long long)(uintptr_t)out + out_off) >> 2) & 15u);

  // ---- staging ring bookkeeping ------------------------------------------------------------------------------------
  int vm_issued = 0;  // VMEM instructions (DMAs + stores) this wave has issued since the wait above
  int idxv = 0;       // lane s: value of vm_issued right after the DMA that filled slot s
  auto dma = [&](int row, int slot) {
    const int dst = lds_base + slot * p.seg_bytes;
    if (dma_lane)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void *)(lds + dst), 16, voff, a_base + (unsigned)row * row_bytes, 0, AA_UP_DMA_AUX);
    vm_issued++;
    idxv = (lane == slot) ? vm_issued : idxv;
  };
  int dma_next = r_begin;  // next input row to stage
  int slot_next = 0;       // its slot
  for (int i = 0; i < G; i++) {
    if (AA_UP_ABL != 2 && dma_next < r_stop) {
      dma(dma_next, slot_next);
      dma_next++;
      slot_next = slot_next + 1 == G ? 0 : slot_next + 1;
    }
  }

  float ring[KR][CPL];  // horizontal-pass results of input rows top-KR .. top-1
#pragma unroll
  for (int k2 = 0; k2 < KR; k2++)
#pragma unroll
    for (int e = 0; e < CPL; e++) ring[k2][e] = 0.0f;
  int top = r_begin;  // next input row to run the horizontal pass on
  int slot_top = 0;

  // one input row: wait for its DMA, union window from LDS, reference-order accumulation per output, refill, push
  // 16-bit elements, odd W: the dword holding the tensor's final element straddles the end of the tensor and is refused by the range
  // check (see aa_fused_float_impl.h: nothing may be read past a tensor); lane 0 fetches that element on its own into the staged row
  const int fix_row = (ES == 2 && (p.W & 1) && (long long)plane + 1 == p.n_groups / p.ybands) ? p.H - 1 : -1;
  auto hpass_row = [&]() {
    const int my_idx = __builtin_amdgcn_readlane(idxv, slot_top);
    wait_vmcnt_up(vm_issued - my_idx);  // everything issued up to and including that DMA has completed
    if (ES == 2 && top == fix_row) {
      const int pos = p.W - 1 - seg0;  // (even: seg0 is a multiple of 8, W is odd)
      if (pos >= 0 && pos < p.nseg * EPP) {
        if (lane == 0) {
          const unsigned short v = *(const unsigned short *)((const uint8_t *)in + plane_off + (unsigned long long)(p.H - 1) * row_bytes +
                                                             (unsigned long long)(p.W - 1) * 2u);
          *(unsigned *)(lds + lds_base + slot_top * p.seg_bytes + pos * 2) = (unsigned)v;
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      }
    }
    float d[U];
    if constexpr (DT == AA_F32) {
      const __attribute__((address_space(3))) float *src =
          (const __attribute__((address_space(3))) float *)(uintptr_t)(lane_lds + (unsigned)(slot_top * p.seg_bytes));
#pragma unroll
      for (int q = 0; q < U; q++) d[q] = src[q];
    } else {
      const __attribute__((address_space(3))) unsigned short *src =
          (const __attribute__((address_space(3))) unsigned short *)(uintptr_t)(lane_lds + (unsigned)(slot_top * p.seg_bytes));
#pragma unroll
      for (int q = 0; q < U; q++) d[q] = up_elem_to_f32<DT>(src[q]);
    }
    float acc[CPL];
#pragma unroll
    for (int e = 0; e < CPL; e++) {
      acc[e] = -0.0f;  // (-0) + x == x exactly: the first own tap is an assignment
#pragma unroll
      for (int q = 0; q < U; q++) {
        const float prod = d[q] * wreg[e][q];
        const float sum = acc[e] + prod;
        acc[e] = select_by_mask_up(acc[e], sum, inwin[e][q]);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the window is in registers: the slot may be refilled
    if (dma_next < r_stop) {
      dma(dma_next, slot_top);
      dma_next++;
    }
#pragma unroll
    for (int k2 = 0; k2 + 1 < KR; k2++)
#pragma unroll
      for (int e = 0; e < CPL; e++) ring[k2][e] = ring[k2 + 1][e];
#pragma unroll
    for (int e = 0; e < CPL; e++) ring[KR - 1][e] = acc[e];
    top++;
    slot_top = slot_top + 1 == G ? 0 : slot_top + 1;
  };

  // table row of an output: window start, length, weights — ONE scalar load of the row's gather record (wave-uniform,
  // issued one output row ahead)
  struct VRow { int m; int s; float w[KR]; };
  const int32_t *__restrict__ grec = (const int32_t *)(tab_h + p.gather_off);
  auto load_vrow = [&](int oy) -> VRow {
    VRow v;
    const int o = oy < p.oH ? oy : p.oH - 1;
    const int32_t *rec = (const int32_t *)((const char *)grec + (unsigned)o * 32u);
    v.m = __builtin_amdgcn_readfirstlane(rec[0]);
    v.s = __builtin_amdgcn_readfirstlane(rec[1]);
#pragma unroll
    for (int k2 = 0; k2 < KR; k2++) v.w[k2] = __int_as_float(__builtin_amdgcn_readfirstlane(rec[2 + k2]));
    return v;
  };

  VRow cur = load_vrow(oy0);
  // Rows that are not whole sectors: the strips of a row (the waves of this workgroup) are kept within AA_UP_PACE rows of each
  // other, so that the two halves of a shared end sector reach the L2 close together and leave it as one full write
  // (906-wide gradients: 0.345 -> 0.312 ms).  Only workgroups all of whose waves are alive take the barrier.
  const bool pace = AA_UP_PACE != 0 && (p.store_nt == 2 || p.pace_all) && p.strips_per_block > 1 &&
                    ((k % sgroups) + 1) * p.strips_per_block <= p.nstrips;  // every wave of this workgroup is alive
  for (int oy = oy0; oy < oy1; oy++) {
    if (pace && ((oy - oy0) % AA_UP_PACE) == 0) __builtin_amdgcn_s_barrier();
    const VRow nxt = load_vrow(oy + 1);
    int s = cur.s > 1 ? cur.s : 1;
    s = s < KR ? s : KR;
    const int need = cur.m + s;
    if (AA_UP_ABL != 2) { while (top < need) hpass_row(); }
    // Windows end at non-decreasing rows and the ring was advanced exactly to this one's end (top == need), so the
    // window's rows m .. m+s-1 are the ring's LAST s entries: ring[KR-s .. KR-1].
    float res[CPL];
#pragma unroll
    for (int e = 0; e < CPL; e++) res[e] = 0.0f;
#pragma unroll
    for (int ss = 1; ss <= KR; ss++) {
      if (s == ss) {  // wave-uniform: one of the KR static unrollings runs; taps beyond the window are not added at all
#pragma unroll
        for (int e = 0; e < CPL; e++) {
          float acc = ring[KR - ss][e] * cur.w[0];
#pragma unroll
          for (int k2 = 1; k2 < ss; k2++) acc = acc + ring[KR - ss + k2][e] * cur.w[k2];
          res[e] = acc;
        }
      }
    }
    const unsigned soff = AA_UP_ABL == 3 ? 0u : (unsigned)oy * out_row_bytes;
    // vm_issued may only count instructions that are certainly issued (an all-lanes-off store is branched around): every
    // count below is guarded by a wave-uniform condition under which lane 0 or the ragged lane really stores
    if constexpr (DT != AA_F32) {  // 16-bit planes: one store of the lane's CPL halves (plain or streaming), ragged columns one by one
      unsigned hb[CPL];
#pragma unroll
      for (int e = 0; e < CPL; e++) hb[e] = up_f32_to_elem<DT>(res[e]);
      if constexpr (CPL == 4) {
        typedef unsigned u32x2h __attribute__((ext_vector_type(2)));
        const u32x2h t = {hb[0] | (hb[1] << 16), hb[2] | (hb[3] << 16)};
        if (bw >= CPL) {
          if (full_lane) {
            if (p.store_nt != 0) __builtin_amdgcn_raw_buffer_store_b64(t, orsrc, store_voff, soff, 2);
            else __builtin_amdgcn_raw_buffer_store_b64(t, orsrc, store_voff, soff, 0);
          }
          vm_issued++;
        }
      } else if constexpr (CPL == 2) {
        if (bw >= CPL) {
          if (full_lane) __builtin_amdgcn_raw_buffer_store_b32(hb[0] | (hb[1] << 16), orsrc, store_voff, soff, 0);
          vm_issued++;
        }
      } else {
        if (any_active) __builtin_amdgcn_raw_buffer_store_b16((unsigned short)hb[0], orsrc, store_voff, soff, 0);
        vm_issued++;
      }
      if constexpr (CPL > 1) {
        const int ragged = bw % CPL;
#pragma unroll
        for (int e = 0; e < CPL - 1; e++) {
          if (__builtin_expect(ragged != 0, 0) && e < ragged) {
            if (col0 == bw - ragged) __builtin_amdgcn_raw_buffer_store_b16((unsigned short)hb[e], orsrc, store_voff + 2u * e, soff, 0);
            vm_issued++;
          }
        }
      }
      cur = nxt;
      continue;
    }
    if constexpr (CPL == 4) {
      typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
      const u32x4 t = {__float_as_uint(res[0]), __float_as_uint(res[1]), __float_as_uint(res[2]), __float_as_uint(res[3])};
      if (aln) {
        // Rows that are not whole 64-byte sectors, even widths: the piece a strip stores is cut at the sector boundaries of
        // THIS row — columns [240 k - d, 240 k + 240 - d), d = the row's phase in floats (even, 0 .. 14) — so every streamed
        // store covers whole sectors and no sector is shared between strips (only the row's two ends stay partial).  The wave
        // holds columns 240 k - 16 .. 240 k + 239; a pass through LDS moves each lane's four results to the lane that owns
        // their absolute 16-byte slot (8-byte aligned reads: d is even).
        __attribute__((address_space(3))) u32x4 *stw = (__attribute__((address_space(3))) u32x4 *)(uintptr_t)(aln_lds + (unsigned)lane * 16u);
        *stw = t;
        const unsigned d = (phase0f + (unsigned)oy * (unsigned)p.oW) & 15u;
        typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
        const unsigned rd = aln_lds + (16u - d) * 4u + (lane < 60 ? (unsigned)lane * 16u : 0u);
        const __attribute__((address_space(3))) u32x2 *ldp = (const __attribute__((address_space(3))) u32x2 *)(uintptr_t)rd;
        const u32x2 v0 = ldp[0], v1 = ldp[1];
        const int colj = strip * 240 - (int)d + lane * 4;  // first column of this lane's slot
        const bool mine = lane < 60;
        const bool lo_ok = mine && colj >= 0 && colj + 1 < p.oW;
        const bool hi_ok = mine && colj + 2 >= 0 && colj + 3 < p.oW;
        const bool full = lo_ok && hi_ok;
        const unsigned cvoff = (unsigned)(colj * 4);
        if (__ballot(full) != 0ull) {  // (wave-uniform: the store is certainly issued and may be counted)
          const u32x4 tv = {v0.x, v0.y, v1.x, v1.y};
          if (full) __builtin_amdgcn_raw_buffer_store_b128(tv, orsrc, cvoff, soff, 2);
          vm_issued++;
        }
        // the row's first / last slot can hold two columns only (never counted: waiting for more is safe)
        if (lo_ok && !hi_ok) __builtin_amdgcn_raw_buffer_store_b64(v0, orsrc, cvoff, soff, 2);
        if (hi_ok && !lo_ok) __builtin_amdgcn_raw_buffer_store_b64(v1, orsrc, cvoff + 8u, soff, 2);
      } else if (p.store_nt == 2 && bw >= CPL) {
        // Output rows that are not whole 64-byte sectors (oW = 906: 3624 B): the sectors a piece shares with its
        // neighbouring strip are written half by each, and a streamed (nt) half-sector write costs a read-modify-write
        // at the memory.  So only the lanes whose 16 bytes lie in whole sectors of the piece stream; the lanes of its
        // two end sectors store with the default policy and the L2 merges the halves.  Measured on [256,3,438,906]
        // gradients: 0.395-0.44 ms (all nt) -> 0.32-0.376 ms depending on the box / buffer placement; aligned widths
        // keep the single store (the split costs them 3 %).
        const unsigned P = (phase0 + soff) & 63u;
        const unsigned nl_full = (unsigned)bw / CPL;
        const unsigned E = P + 16u * nl_full;
        const unsigned IA = (P + 63u) & ~63u, IB = E & ~63u;
        const unsigned lo = (IA - P + 15u) >> 4;
        const unsigned hi = IB > IA ? (IB - P) >> 4 : lo;
        const bool interior = (unsigned)lane >= lo && (unsigned)lane < hi;
        if (hi > lo) {  // (lane lo is a full, interior lane: the store is issued)
          if (full_lane && interior) __builtin_amdgcn_raw_buffer_store_b128(t, orsrc, store_voff, soff, 2);
          vm_issued++;
        }
        if (lo > 0 || hi < nl_full) {  // (lane 0 or lane hi is a full end lane)
          if (full_lane && !interior) __builtin_amdgcn_raw_buffer_store_b128(t, orsrc, store_voff, soff, 0);
          vm_issued++;
        }
      } else if (bw >= CPL) {
        if (full_lane && (AA_UP_ABL != 1 || t.x == 0x12345678u)) {
          if (p.store_nt != 0) __builtin_amdgcn_raw_buffer_store_b128(t, orsrc, store_voff, soff, 2);
          else __builtin_amdgcn_raw_buffer_store_b128(t, orsrc, store_voff, soff, 0);
        }
        if (AA_UP_ABL != 1) vm_issued++;
      }
    } else if constexpr (CPL == 2) {
      typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
      const u32x2 t = {__float_as_uint(res[0]), __float_as_uint(res[1])};
      if (bw >= CPL) {
        if (full_lane) __builtin_amdgcn_raw_buffer_store_b64(t, orsrc, store_voff, soff, 0);
        vm_issued++;
      }
    } else {
      if (any_active) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(res[0]), orsrc, store_voff, soff, 0);
      vm_issued++;
    }
    if constexpr (CPL > 1) {
      const int ragged = bw % CPL;  // (wave-uniform) columns of the strip's last, partial lane: stored one by one
#pragma unroll
      for (int e = 0; e < CPL - 1; e++) {
        if (__builtin_expect(ragged != 0, 0) && e < ragged) {
          if (col0 == bw - ragged) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(res[e]), orsrc, store_voff + 4u * e, soff, 0);
          vm_issued++;
        }
      }
    }
    cur = nxt;
  }
}

template <int U, int G, int KR, int CPL, int DT>
int launch_k(FusedF32UpParams p, const AAProblem &q, size_t lds) {
  auto kern = fused_f32_nchw_up_kernel<U, G, KR, CPL, DT>;
  const int tag[4] = {U, KR, CPL, p.store_nt};
  // strips per workgroup, row bands and the grid: aa_launch_shape.h, from this instantiation's occupancy at this problem's LDS
  const aa_launch_shape_out s = aa_kernel_launch_shape(AA_LAUNCH_F32_UP, (const void *)kern, p.nstrips, p.strips_per_block, 0, q.N * q.C, q, lds, tag);
  if (s.grid == 0) return 0;
  p.strips_per_block = s.strips_per_block; p.ybands = s.ybands; p.n_groups = s.groups;
  hipLaunchKernelGGL(kern, dim3((unsigned)s.grid), dim3(64 * s.strips_per_block), lds * s.strips_per_block, q.stream, (const void *)q.in,
                     (void *)q.out, (const char *)q.aw.table_dev, (const char *)q.ah.table_dev, p);
  AA_HIP_CHECK_LAUNCH();
  return 1;
}

}  // namespace
