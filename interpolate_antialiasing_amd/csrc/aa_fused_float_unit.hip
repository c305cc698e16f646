// aa_fused_float_unit.hip — one unit of the fused float kernels' compiled set: the Makefile compiles this source once per F32_UNIT row of
// aa_fused_float_list.h, with -DAA_F32_UNIT=<name>, into aa_fused_float_<name>.o.  The unit instantiates its F32_SET rows, and its entry
// point aa_f32_launch_<name> launches the kernel a plan names.  The kernels' parameter blocks are filled here, from the plan and the
// problem: their types belong to the kernels' anonymous namespace, whose name is part of every kernel's symbol.
#include "aa_fused_float_impl.h"
#include "aa_fused_float_up_impl.h"

namespace {

template <int... V> struct F32Vals {};
#define F32_VALS(...) F32Vals<__VA_ARGS__>
template <int UNIT> struct F32UnitForms;
#define F32_UNIT(name, kernel, fast, vert, g, ndma)                                   \
  template <> struct F32UnitForms<F32_UNIT_##name> {                                \
    static constexpr int KERNEL = F32_##kernel, FAST = fast;                        \
    using VERT = F32_VALS vert; using G = F32_VALS g; using NDMA = F32_VALS ndma;   \
  };
#include "aa_fused_float_list.h"

#define F32_CAT2(a, b) a##b
#define F32_CAT(a, b) F32_CAT2(a, b)
constexpr int kUnit = F32_CAT(F32_UNIT_, AA_F32_UNIT);
static_assert(F32UnitForms<kUnit>::FAST == AA_F32_FAST, "the Makefile passes a unit's fast column as AA_F32_FAST");

// f(std::integral_constant<int, v>) for each v of the list until one returns true; f32_find2 walks two lists in step
template <class F, int... V> bool f32_find(F32Vals<V...>, F f) { return (f(std::integral_constant<int, V>{}) || ...); }
template <class F, int... A, int... B> bool f32_find2(F32Vals<A...>, F32Vals<B...>, F f) {
  return (f(std::integral_constant<int, A>{}, std::integral_constant<int, B>{}) || ...);
}

FusedF32Params down_params(const F32Plan &k, const AAProblem &q) {
  const int es = q.dtype == AA_F64 ? 8 : (q.dtype == AA_F32 ? 4 : 2), cs = k.cs;
  FusedF32Params p;
  p.H = (int)q.H; p.W = (int)q.W * cs; p.oH = (int)q.oH; p.oW = (int)q.oW * cs;
  p.Wp = (int)q.W; p.oWp = (int)q.oW;
  p.ksize_w = q.aw.ksize; p.ksize_h = q.ah.ksize;
  // a pitched view: rows / planes (images) these many bytes apart
  p.plane_in_bytes = q.in_row_pitch ? (unsigned long long)q.in_img_pitch : (unsigned long long)q.H * q.W * es * cs;
  p.row_pitch = q.in_row_pitch ? (unsigned)q.in_row_pitch : (unsigned)(q.W * es * cs);
  p.plane_out_bytes = (unsigned long long)q.oH * q.oW * es * cs;
  const unsigned long long planes = (unsigned long long)(cs == 1 ? q.N * q.C : q.N);
  p.total_in_bytes = q.in_row_pitch ? p.plane_in_bytes * (planes - 1) + (unsigned long long)(q.H - 1) * p.row_pitch + (unsigned long long)q.W * es * cs
                                    : p.plane_in_bytes * planes;
  p.total_out_bytes = p.plane_out_bytes * planes;
  p.sc_off = q.ah.scatter_off;
  p.store_nt = p.total_out_bytes > (64ull << 20) ? 1 : 0;
  p.nstrips = k.nstrips; p.strip_w = k.strip_w; p.strips_per_block = p.nstrips <= 8 ? p.nstrips : 4;
  p.nseg = k.nseg; p.seg_bytes = p.nseg * 16;
  p.ybands = 1; p.n_groups = 0;
  return p;
}

FusedF32UpParams up_params(const F32Plan &k, const AAProblem &q) {
  const int es = q.dtype == AA_F32 ? 4 : 2;
  FusedF32UpParams p;
  p.H = (int)q.H; p.W = (int)q.W; p.oH = (int)q.oH; p.oW = (int)q.oW;
  p.ksize_w = q.aw.ksize; p.ksize_h = q.ah.ksize;
  p.plane_in_bytes = (unsigned long long)q.H * q.W * es;
  p.plane_out_bytes = (unsigned long long)q.oH * q.oW * es;
  p.total_in_bytes = p.plane_in_bytes * (unsigned long long)(q.N * q.C);
  p.total_out_bytes = p.plane_out_bytes * (unsigned long long)(q.N * q.C);
  p.nstrips = k.nstrips;
  p.strip_w = k.strip_w;
  p.strips_per_block = p.nstrips <= 8 ? p.nstrips : 4;
  p.nseg = k.nseg;
  p.seg_bytes = p.nseg * 16;
  p.gather_off = q.ah.gather_off;
  p.store_nt = k.store_nt;
  p.pace_all = aa_knob("AA_UP_PACE_ALL") ? 1 : 0;
  p.ybands = 1;
  p.n_groups = 0;
  return p;
}

// Instantiates the kernels of one F32_SET row (element types DTS, channel stride or CPL CS, widths WS) and launches the one that is k.
// false: the row does not hold k.
template <int CS, class DTS, class WS>
bool f32_launch_set(const F32Plan &k, const AAProblem *q, int *rc) {
  using U = F32UnitForms<kUnit>;
  return f32_find(DTS{}, [&](auto dt) {
    return f32_find(WS{}, [&](auto w) {
      return f32_find(typename U::VERT{}, [&](auto v) {
        return f32_find2(typename U::G{}, typename U::NDMA{}, [&](auto g, auto ndma) {
          constexpr int DT = decltype(dt)::value, W = decltype(w)::value, V = decltype(v)::value;
          constexpr int G = decltype(g)::value, NDMA = decltype(ndma)::value;
          if (k.kernel != U::KERNEL || k.DT != DT || k.cs != CS || k.width != W || k.vert != V || k.G != G || k.NDMA != NDMA) return false;
          if constexpr (U::KERNEL == F32_DOWN) *rc = q ? launch_k<W, G, NDMA, V, DT, CS>(down_params(k, *q), *q) : 1;
          else *rc = q ? launch_k<W, G, V, CS, DT>(up_params(k, *q), *q, (size_t)G * k.nseg * 16 + k.lds_extra) : 1;
          return true;
        });
      });
    });
  });
}

template <int UNIT>
int f32_launch_unit(const F32Plan &k, const AAProblem *q) {
  int rc = 0;
#define F32_SET(unit, dts, cs, ws) \
  if constexpr (F32_UNIT_##unit == UNIT) if (f32_launch_set<cs, F32_VALS dts, F32_VALS ws>(k, q, &rc)) return rc;
#include "aa_fused_float_list.h"
  return 0;
}

}  // namespace

int F32_CAT(aa_f32_launch_, AA_F32_UNIT)(const F32Plan &k, const AAProblem *q) { return f32_launch_unit<kUnit>(k, q); }
