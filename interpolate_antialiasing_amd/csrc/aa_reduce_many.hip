// aa_reduce_many.hip — Pillow's Image.reduce for a RAGGED batch: N uint8 images of N sizes, each with its own integer box and its own
// factors (fx, fy), in ONE launch.  The first step of Image.resize(reducing_gap=...) for a list: every large item is read once by an
// integer box sum, and the ragged resize (aa_many.hip, untouched) then runs over the small results, which it reads where they lie.
//
// The grid is the sum of all items' work units.  A workgroup of 256 lanes takes one unit = (item, plane, output row Y, a tile of output
// columns whose input bytes per row fit 4096), finds its item by the binary search over the prefix sums that many_hpass uses (aa_unit_item, aa_many_dev.h), reads that
// item's record (uniform per workgroup: scalar loads) and runs reduce_tile (aa_reduce_tile.h) — the dense kernel's body, bit for bit.  fx
// differs per item, so it is a run-time value, with a per-workgroup switch to the compile-time forms for 2, 3, 4 and 8.  Row starts have any alignment, and no byte beyond the end of a box's row is read.
// The host planner computes, per item, the box's first byte, the result's size and 16-byte aligned place in one arena, the tiling and
// the four multipliers (the float32 division of aa_reduce.hip): nothing is allocated, synchronised or read back.

#include "aa_many_dev.h"
#include "aa_many_host.h"
#include "aa_reduce_many.h"
#include "aa_reduce_tile.h"

#include <string.h>

namespace {

__global__ void __launch_bounds__(kReduceThreads) reduce_many_u8_kernel(const AAReduceManyItem *items, const int64_t *prefix, uint8_t *arena, int n,
                                                                        int E) {
  __shared__ __attribute__((aligned(16))) uint32_t colsum[kReduceTile];
  const int64_t unit = blockIdx.x;
  const int lo = aa_unit_item(prefix, n, unit);
  const AAReduceManyItem &it = items[lo];
  int64_t u = unit - prefix[lo];
  const int xtiles = it.xtiles, rh = it.rh, rw = it.rw, fx = it.fx, fy = it.fy, bh = it.bh, sx = it.sx;
  const int xt = (int)(u % xtiles);
  u /= xtiles;
  const int Y = (int)(u % rh);
  const int64_t plane = u / rh;
  const int X0 = xt * sx;
  const int X1 = X0 + sx < rw ? X0 + sx : rw;
  const int r0 = Y * fy;
  const int r1 = r0 + fy < bh ? r0 + fy : bh;
  const uint8_t *src = it.src + plane * it.plane_pitch + (long long)r0 * it.row_pitch + (long long)X0 * fx * E;
  uint8_t *dst = arena + it.out_off + ((plane * rh + Y) * (long long)rw + X0) * E;
#define AA_REDUCE_MANY_TILE(F) \
  reduce_tile<F>(colsum, src, dst, it.row_pitch, E, fx, it.bw, X0, X1, r1 - r0, r1 - r0 != fy, it.mult[0], it.mult[1], it.mult[2], it.mult[3])
  // fx is uniform per workgroup, so the dense kernel's compile-time factors (AA_REDUCE_FX of aa_reduce.hip) are one scalar branch away.
  // Measured on a uniform 64 x 1080 x 1920 x 3 batch at (4, 4): 190 us with fx at run time only, 171 us with the switch, the dense
  // kernel 165 us (profiles/resize_many_gap.txt).
  switch (fx) {
    case 2: AA_REDUCE_MANY_TILE(2); break;
    case 3: AA_REDUCE_MANY_TILE(3); break;
    case 4: AA_REDUCE_MANY_TILE(4); break;
    case 8: AA_REDUCE_MANY_TILE(8); break;
    default: AA_REDUCE_MANY_TILE(0); break;
  }
#undef AA_REDUCE_MANY_TILE
}

}  // namespace

// ---- host: the planner -------------------------------------------------------------------------------------------------------------------
size_t aa_reduce_many_desc_size(int64_t n) { return aa_desc_size(sizeof(AAReduceManyHeader), sizeof(AAReduceManyItem), n); }

int aa_reduce_many_plan_host(int layout, int64_t n, int64_t C, const aa_reduce_item *in, void *desc_host, size_t desc_bytes, size_t *arena_bytes,
                             int64_t *out_offsets) {
  if (layout != AA_NCHW && layout != AA_NHWC) return AA_ERR_BAD_LAYOUT;
  const int64_t kMax = kAAManyMax;
  if (n < 0 || n > kMax || C < 1 || C > 4) return AA_ERR_BAD_SHAPE;
  if (!desc_host || !arena_bytes || (n > 0 && (!in || !out_offsets))) return AA_ERR_NULL;
  if (desc_bytes < aa_reduce_many_desc_size(n)) return AA_ERR_WORKSPACE;
  const int E = layout == AA_NHWC ? (int)C : 1;
  const int64_t planes = layout == AA_NHWC ? 1 : C;

  AAReduceManyHeader *hd = (AAReduceManyHeader *)desc_host;
  AAReduceManyItem *items = (AAReduceManyItem *)(hd + 1);
  int64_t *prefix = (int64_t *)(items + n);
  size_t off = 0;
  int64_t units = 0;
  for (int64_t i = 0; i < n; i++) {
    const aa_reduce_item &im = in[i];
    AAReduceManyItem it;
    memset(&it, 0, sizeof(it));
    const int rc = aa_many_check_image(im, im.fx >= 1 && im.fy >= 1 && (int64_t)im.fx * im.fy <= 65536, layout, C, 1, C);
    if (rc != AA_OK) return rc;
    const int64_t x0 = im.box[0], y0 = im.box[1], x1 = im.box[2], y1 = im.box[3];
    if (x0 < 0 || y0 < 0 || x1 > im.W || y1 > im.H || x1 <= x0 || y1 <= y0) return AA_ERR_BAD_SHAPE;
    const int bw = (int)(x1 - x0), bh = (int)(y1 - y0);
    it.src = (const uint8_t *)im.data_dev + y0 * im.stride_row + x0 * E;
    it.row_pitch = im.stride_row;
    it.plane_pitch = layout == AA_NHWC ? 0 : (C > 1 ? im.stride_ch : 0);
    it.bw = bw; it.bh = bh; it.fx = im.fx; it.fy = im.fy;
    it.rw = (bw + im.fx - 1) / im.fx;
    it.rh = (bh + im.fy - 1) / im.fy;
    it.sx = reduce_tile_columns(im.fx, E);
    it.xtiles = (it.rw + it.sx - 1) / it.sx;
    const unsigned fxr = bw % im.fx ? bw % im.fx : im.fx, fyb = bh % im.fy ? bh % im.fy : im.fy;
    it.mult[0] = reduce_mult((unsigned)im.fx * im.fy);
    it.mult[1] = reduce_mult(fxr * im.fy);
    it.mult[2] = reduce_mult((unsigned)im.fx * fyb);
    it.mult[3] = reduce_mult(fxr * fyb);
    it.out_off = (int64_t)off;
    out_offsets[i] = (int64_t)off;
    off += aa_align16((size_t)C * it.rh * it.rw);
    prefix[i] = units;
    units += planes * it.rh * (int64_t)it.xtiles;
    if (units > INT32_MAX) return AA_ERR_BAD_SHAPE;  // (one grid)
    items[i] = it;
  }
  prefix[n] = units;
  memset(hd, 0, sizeof(*hd));
  hd->magic = AA_REDUCE_MANY_MAGIC;
  hd->n = (int32_t)n; hd->C = (int32_t)C; hd->layout = layout;
  hd->E = E; hd->planes = (int32_t)planes;
  hd->units = units;
  hd->arena_bytes = (int64_t)off;
  *arena_bytes = off;
  return AA_OK;
}

// ---- host: the launch --------------------------------------------------------------------------------------------------------------------
int aa_launch_reduce_many_u8(const void *desc_host, const void *desc_dev, void *arena_dev, size_t arena_bytes, hipStream_t stream) {
  const AAReduceManyHeader *hd = (const AAReduceManyHeader *)desc_host;
  if (hd->magic != AA_REDUCE_MANY_MAGIC || hd->n < 0 || hd->units < 0 || hd->units > INT32_MAX) return AA_ERR_BAD_SHAPE;
  const int64_t n = hd->n;
  if (n == 0) return AA_OK;
  if (!desc_dev || !arena_dev) return AA_ERR_NULL;
  if (arena_bytes < (size_t)hd->arena_bytes) return AA_ERR_WORKSPACE;
  if (((uintptr_t)arena_dev & 15) || ((uintptr_t)desc_dev & 7)) return AA_ERR_BAD_SHAPE;
  const AADescView<AAReduceManyItem> v = aa_desc_view<AAReduceManyHeader, AAReduceManyItem>(desc_dev, n);
  hipLaunchKernelGGL(reduce_many_u8_kernel, dim3((unsigned)hd->units), dim3(kReduceThreads), 0, stream, v.items, v.prefix, (uint8_t *)arena_dev, (int)n,
                     hd->E);
  AA_HIP_CHECK_LAUNCH();
  return AA_OK;
}
