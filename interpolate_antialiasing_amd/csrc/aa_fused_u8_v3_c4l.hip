// aa_fused_u8_v3_c4l.hip — narrow-window instantiations (<= 16 taps) with 6 open output rows (MAXC = 6) of the fused uint8 kernel
// (aa_fused_u8_v3_impl.h) for 4 channels per pixel, Pillow arithmetic: Lanczos down-scaling by 1 .. ~2.7.  The float-arithmetic
// instantiations are in aa_fused_u8_v3_c4lf.hip.
#include "aa_fused_u8_v3_impl.h"

int aa_v3_launch_c4lf(int tw, const FusedU8V3Params &p, const AAProblem &q, size_t lds);

int aa_v3_launch_c4l(int tw, bool flt, const FusedU8V3Params &p, const AAProblem &q, size_t lds) {
  return flt ? aa_v3_launch_c4lf(tw, p, q, lds) : dispatch_tw_six<4, false>(tw, p, q, lds);
}
