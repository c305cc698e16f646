// aa_fused_u8_v3_c1l.hip — narrow-window instantiations (<= 16 taps) with 6 open output rows (MAXC = 6) of the fused uint8 kernel
// (aa_fused_u8_v3_impl.h) for 1 channel (planar bytes), Pillow arithmetic: Lanczos down-scaling by 1 .. ~2.7.  The float-arithmetic
// instantiations are in aa_fused_u8_v3_c1lf.hip.
#include "aa_fused_u8_v3_impl.h"

int aa_v3_launch_c1lf(int tw, const FusedU8V3Params &p, const AAProblem &q, size_t lds);

int aa_v3_launch_c1l(int tw, bool flt, const FusedU8V3Params &p, const AAProblem &q, size_t lds) {
  return flt ? aa_v3_launch_c1lf(tw, p, q, lds) : dispatch_tw_six<1, false>(tw, p, q, lds);
}
