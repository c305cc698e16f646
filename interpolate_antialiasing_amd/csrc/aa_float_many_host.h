// aa_float_many_host.h — the host side the float ragged calls share (aa_embed_many.hip, aa_many_back.hip, aa_many_back_bwd.hip) on top
// of aa_many_host.h: which types are floats and how wide a stored element is, the choice of a kernel's float type, and the tables of
// an item as a planner sizes them and places them in the table arena.  Each is written here once.  In the unnamed namespace: the type
// tags name aa_many_dev.h's element types.  (What the kernels share: aa_float_many_dev.h.)
#pragma once

#include "aa_many_dev.h"
#include "aa_many_host.h"

namespace {

inline bool float_dtype(int dt) { return dt == AA_F32 || dt == AA_F16 || dt == AA_BF16; }
// The bytes of an element of every type a float ragged call stores (aa_many_back.hip's labels and masks among them).
inline size_t elem_bytes(int dt) {
  switch (dt) {
    case AA_U8: case AA_BOOL: return 1;
    case AA_F16: case AA_BF16: case AA_I16: return 2;
    case AA_I64: return 8;
    default: return 4;
  }
}

// f(TypeTag<T>{}) for the element type T of a float dtype (checked by the caller: float_dtype): the kernels' template arguments are
// chosen in one place.  tag_t<decltype(tag)> is T.
template <typename T> struct TypeTag { using type = T; };
template <typename Tag> using tag_t = typename Tag::type;
template <typename F> inline void with_float_type(int dt, F &&f) {
  if (dt == AA_F32) f(TypeTag<float>{});
  else if (dt == AA_F16) f(TypeTag<f16_t>{});
  else f(TypeTag<bf16_t>{});
}

// The two forward tables of an item, [h, w] resampled to [oh, ow], into its record: the rows' lengths (a negative aa_table_ksize is the
// error returned, H before W, and nothing is written), the float scales the table kernels build from, and the tables appended to the
// table arena at ws, H then W.
template <typename Item> inline int plan_forward_tables(int filter, int64_t h, int64_t w, int64_t oh, int64_t ow, Item &it, size_t &ws) {
  const int kh = aa_table_ksize(filter, AA_TABLE_F32, h, oh, 0, 0.0), kw = aa_table_ksize(filter, AA_TABLE_F32, w, ow, 0, 0.0);
  if (kh < 0) return kh;
  if (kw < 0) return kw;
  it.ksize_h = kh; it.ksize_w = kw;
  it.scale_h = (float)h / (float)oh;
  it.scale_w = (float)w / (float)ow;
  it.tab_h = (int64_t)ws; ws += aa_table_weights_end(AA_TABLE_F32, oh, kh);
  it.tab_w = (int64_t)ws; ws += aa_table_weights_end(AA_TABLE_F32, ow, kw);
  return AA_OK;
}
// ... and their two adjoints, for a backward, after them: the arena order of an item is tab_h, tab_w, tr_h, tr_w.
template <typename Item> inline int plan_adjoint_tables(int filter, int64_t h, int64_t w, int64_t oh, int64_t ow, Item &it, size_t &ws) {
  const int th = aa_table_transposed_ksize(filter, AA_TABLE_F32, h, oh, 0, 0.0), tw = aa_table_transposed_ksize(filter, AA_TABLE_F32, w, ow, 0, 0.0);
  if (th < 0) return th;
  if (tw < 0) return tw;
  it.trk_h = th; it.trk_w = tw;
  it.tr_h = (int64_t)ws; ws += aa_table_weights_end(AA_TABLE_F32, h, th);
  it.tr_w = (int64_t)ws; ws += aa_table_weights_end(AA_TABLE_F32, w, tw);
  return AA_OK;
}

}  // namespace
