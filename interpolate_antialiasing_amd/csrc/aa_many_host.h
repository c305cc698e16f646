// aa_many_host.h — the host side the ragged calls share (aa_many.hip, aa_many_nearest.hip, aa_many_maps.hip, aa_many_ycbcr.hip,
// aa_reduce_many.hip): the [header][items][prefix] block, what a planner checks of its canvas, of a place and of an image, Pillow's
// reading of a box and its scale, the part of a placed item that lies on the canvas, and what a launch checks of a planned block.  Each
// rule is written here once; the planners differ only in what they do with the results.  (What the kernels share: aa_many_dev.h.)
#pragma once

#include "aa_many.h"

constexpr int64_t kAAManyMax = INT32_MAX / 4;  // the bound on a size or an offset of a ragged call

// The block every planner writes: [ header ][ item x n ][ int64 prefix[n + 1] ]; what follows it is the planner's own.
inline size_t aa_desc_size(size_t header_bytes, size_t item_bytes, int64_t n) {
  return n < 0 ? 0 : header_bytes + (size_t)n * item_bytes + ((size_t)n + 1) * sizeof(int64_t);
}
// The records of such a block, as the launches hand the device copy's to the kernels.
template <typename Item> struct AADescView { const Item *items; const int64_t *prefix; };
template <typename Header, typename Item> inline AADescView<Item> aa_desc_view(const void *desc, int64_t n) {
  const Item *items = (const Item *)((const char *)desc + sizeof(Header));
  return {items, (const int64_t *)(items + n)};
}

inline bool aa_many_place_ok(const aa_many_place &p) {
  return p.vH > 0 && p.vW > 0 && p.vH <= kAAManyMax && p.vW <= kAAManyMax && p.oy >= -kAAManyMax && p.oy <= kAAManyMax && p.ox >= -kAAManyMax &&
         p.ox <= kAAManyMax;
}

// The canvas prologue of a planner, in the planners' order of precedence: n (n_max at most), what the caller checks of its own sizes
// (own_ok: C) and the canvas against the bound; the pointers; every place.
inline int aa_many_check_canvas(int64_t n, int64_t n_max, bool own_ok, int64_t oH, int64_t oW, const void *desc_host, const void *workspace_bytes,
                                const void *images, const aa_many_place *places) {
  if (n < 0 || n > n_max || !own_ok || oH <= 0 || oW <= 0 || oH > kAAManyMax || oW > kAAManyMax) return AA_ERR_BAD_SHAPE;
  if (!desc_host || !workspace_bytes || (n > 0 && !images)) return AA_ERR_NULL;
  for (int64_t i = 0; places && i < n; i++)
    if (!aa_many_place_ok(places[i])) return AA_ERR_BAD_SHAPE;
  return AA_OK;
}

// The launch prologue of a planned block of n items whose header has passed the caller's own checks: nothing for n == 0 (the caller
// returns AA_OK); else the pointers, the workspace against the plan's ws_bytes, the alignment of workspace, device block and output.
inline int aa_many_check_launch(int64_t n, const void *desc_dev, const void *out_dev, const void *workspace_dev, size_t workspace_bytes,
                                int64_t ws_bytes, size_t out_elem_bytes) {
  if (n == 0) return AA_OK;
  if (!desc_dev || !out_dev || !workspace_dev) return AA_ERR_NULL;
  if (workspace_bytes < (size_t)ws_bytes) return AA_ERR_WORKSPACE;
  if (((uintptr_t)workspace_dev & 15) || ((uintptr_t)desc_dev & 7) || ((uintptr_t)out_dev % out_elem_bytes)) return AA_ERR_BAD_SHAPE;
  return AA_OK;
}

// One image record (aa_many_image or aa_reduce_item: the same six leading fields), in the planners' order of precedence: the pointer,
// the sizes, what the caller checks of its own fields (own_ok: flags or factors), the stride rule of `layout`'s class, and the
// alignment of data and strides to the element.  el, px: bytes of an element and of a pixel (1 and C for uint8, where the alignment
// check is empty).
template <typename Record>
inline int aa_many_check_image(const Record &im, bool own_ok, int layout, int64_t C, int64_t el, int64_t px) {
  if (!im.data_dev) return AA_ERR_NULL;
  if (im.H <= 0 || im.W <= 0 || im.H > kAAManyMax || im.W > kAAManyMax || !own_ok) return AA_ERR_BAD_SHAPE;
  // (the stride of an axis of one element never matters)
  if (layout == AA_NHWC ? ((C > 1 && im.stride_ch != 1) || (im.W > 1 && im.stride_px != px)) : (im.W > 1 && im.stride_px != el)) return AA_ERR_STRIDES;
  if (((uintptr_t)im.data_dev % el) || (im.H > 1 && im.stride_row % el) || (layout != AA_NHWC && C > 1 && im.stride_ch % el)) return AA_ERR_STRIDES;
  return AA_OK;
}

// The source interval of an image per axis as Pillow's C sees it, and whether the scale comes from it (a box) or from in / out.
struct AAManyBox {
  double x0, y0, x1, y1;
  int on;
};

// aa_many_check_image, then the box: four floats, inside the image, not empty; a full box is no box.
inline int aa_many_check_image_box(const aa_many_image &im, bool own_ok, int layout, int64_t C, int64_t el, int64_t px, AAManyBox *b) {
  const int rc = aa_many_check_image(im, own_ok, layout, C, el, px);
  if (rc != AA_OK) return rc;
  const double W = (double)im.W, H = (double)im.H;
  *b = {0.0, 0.0, W, H, 0};
  if (im.has_box) {  // Pillow's C takes the box as floats
    b->x0 = (double)(float)im.box[0]; b->y0 = (double)(float)im.box[1]; b->x1 = (double)(float)im.box[2]; b->y1 = (double)(float)im.box[3];
    if (!(b->x0 >= 0.0) || !(b->y0 >= 0.0) || !(b->x1 <= W) || !(b->y1 <= H)) return AA_ERR_BAD_SHAPE;  // beyond the image (or NaN)
    if (!(b->x1 - b->x0 > 0.0) || !(b->y1 - b->y0 > 0.0)) return AA_ERR_BAD_SHAPE;                      // empty
    b->on = !(b->x0 == 0.0 && b->y0 == 0.0 && b->x1 == W && b->y1 == H);
  }
  return AA_OK;
}

// Pillow's scale of an axis resized to v: its C takes the box as floats, takes their FLOAT difference, and only then divides in double;
// without a box (on == 0) it is full / v.  The table kernels evaluate the same expression (-ffp-contract=off).
__host__ __device__ inline double aa_pil_scale(int on, double b0, double b1, double full, int64_t v) { return (on ? (double)(float)(b1 - b0) : full) / (double)v; }

// The part [v0, v0 + m) per axis of an item of its own size [vH, vW] at (oy, ox) that lies on the [oH, oW] canvas, and the canvas index
// d = v0 + o it starts at.  Off the canvas on either axis: all fill, everything but the size is 0.
inline AAManyPlace aa_many_cover(const aa_many_place &p, int64_t oH, int64_t oW) {
  const int64_t v0h = p.oy < 0 ? -p.oy : 0, v0w = p.ox < 0 ? -p.ox : 0;
  const int64_t mh = (p.vH < oH - p.oy ? p.vH : oH - p.oy) - v0h, mw = (p.vW < oW - p.ox ? p.vW : oW - p.ox) - v0w;
  if (mh <= 0 || mw <= 0) return {(int32_t)p.vH, (int32_t)p.vW, 0, 0, 0, 0, 0, 0};
  return {(int32_t)p.vH, (int32_t)p.vW, (int32_t)v0h, (int32_t)v0w, (int32_t)mh, (int32_t)mw, (int32_t)(v0h + p.oy), (int32_t)(v0w + p.ox)};
}
