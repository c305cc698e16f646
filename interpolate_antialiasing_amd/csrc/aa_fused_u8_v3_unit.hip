// aa_fused_u8_v3_unit.hip — one unit of the fused uint8 kernel's compiled set: the Makefile compiles this source once per V3_UNIT row of
// aa_fused_u8_v3_list.h, with -DAA_V3_UNIT=<name>, into aa_fused_u8_v3_<name>.o.  The unit instantiates its route's kernels for its
// channel count and arithmetic, and its entry point aa_v3_launch_<name> launches the one a plan names.
#include "aa_fused_u8_v3_impl.h"

namespace {

template <int... V> struct V3Vals {};
struct V3Forms {
  enum : int { T = 1, N = 2, P = 4, U2 = 8, U6 = 16 };  // TWO_DMA, NONNEG, PERIODIC, UPK 2, UPK 6
};
template <int ROUTE> struct V3Set;
#define V3_VALS(...) V3Vals<__VA_ARGS__>
#define V3_ROUTE(route, tw, twf, maxc, forms)                                                                                    \
  template <> struct V3Set<V3_##route> : V3Forms {                                                                               \
    using TW = V3_VALS tw;                                                                                                       \
    using TWF = V3_VALS twf;                                                                                                     \
    using MAXC = V3_VALS maxc;                                                                                                   \
    using FORMS = V3_VALS forms;                                                                                                 \
  };
struct V3Unit {
  int route, C, arith, fast;
};
#define V3_UNIT(name, route, C, arith, fast) constexpr V3Unit v3_unit_##name{V3_##route, C, V3_##arith, fast};
#include "aa_fused_u8_v3_list.h"

#define V3_CAT2(a, b) a##b
#define V3_CAT(a, b) V3_CAT2(a, b)
constexpr V3Unit kUnit = V3_CAT(v3_unit_, AA_V3_UNIT);
static_assert(kUnit.fast == AA_V3_FLT_FAST, "the Makefile passes a unit's fast column as AA_V3_FLT_FAST");

// f(std::integral_constant<int, v>) for each v of the list until one returns true
template <class F, int... V> bool v3_find(V3Vals<V...>, F f) { return (f(std::integral_constant<int, V>{}) || ...); }

// Instantiates every kernel of (route R, channel count C, arithmetic ARITH) and launches the one that matches k
template <int R, int C, int ARITH>
int v3_launch_unit(const V3Kernel &k, const FusedU8V3Params *p, const AAProblem *q, size_t lds) {
  using S = V3Set<R>;
  constexpr int PL = R == V3_PLANES ? 3 : 0, SP = R == V3_SPLIT ? 4 : 1;
  constexpr bool ALPHA = R == V3_ALPHA || R == V3_SIX_ALPHA;
  if (k.route != R || k.C != C || k.fast != (AA_V3_FLT_FAST != 0) || k.PL != PL || k.SP != SP || k.ALPHA != ALPHA) return 0;
  int rc = 0;
  v3_find(V3Vals<0, 1>{}, [&](auto flt) {
    constexpr bool FLT = decltype(flt)::value;
    if constexpr (!(ARITH & (FLT ? V3_FLT : V3_PIL))) {
      return false;
    } else {
      return v3_find(std::conditional_t<FLT, typename S::TWF, typename S::TW>{}, [&](auto tw) {
        return v3_find(typename S::MAXC{}, [&](auto maxc) {
          return v3_find(typename S::FORMS{}, [&](auto form) {
            constexpr int F = FLT ? decltype(form)::value & ~(S::N | S::P) : decltype(form)::value;
            constexpr int TW = decltype(tw)::value, MAXC = decltype(maxc)::value, UPK = F & S::U2 ? 2 : F & S::U6 ? 6 : 0;
            constexpr bool TWO = F & S::T, NONNEG = F & S::N, PERIODIC = F & S::P;
            if (k.FLT != FLT || k.TW != TW || k.MAXC != MAXC || k.UPK != UPK || k.TWO_DMA != TWO || k.NONNEG != NONNEG || k.PERIODIC != PERIODIC)
              return false;
            // float16 / bfloat16 output (p->out16) has instantiations of its own, in the routes v3_route_has_out16 names
            if constexpr (FLT && v3_route_has_out16(R)) {
              if (q && p->out16) {
                rc = launch_k<C, TW, 8, MAXC, TWO, NONNEG, PERIODIC, FLT, UPK, PL, SP, ALPHA, true>(*p, *q, lds);
                return true;
              }
            }
            rc = q ? launch_k<C, TW, 8, MAXC, TWO, NONNEG, PERIODIC, FLT, UPK, PL, SP, ALPHA>(*p, *q, lds) : 1;
            return true;
          });
        });
      });
    }
  });
  return rc;
}

}  // namespace

int V3_CAT(aa_v3_launch_, AA_V3_UNIT)(const V3Kernel &k, const FusedU8V3Params *p, const AAProblem *q, size_t lds) {
  return v3_launch_unit<kUnit.route, kUnit.C, kUnit.arith>(k, p, q, lds);
}
