// aa_fused_u8_v3_c3lf.hip — narrow-window instantiations with 6 open output rows (MAXC = 6) of the fused uint8 kernel
// (aa_fused_u8_v3_impl.h) for 3 channels per pixel in FLOAT arithmetic: the reference harness's uint8 semantics and the uint8 -> float32
// conversion at Lanczos down-scaling by 1 .. ~2.7.
#include "aa_fused_u8_v3_impl.h"

int aa_v3_launch_c3lf(int tw, const FusedU8V3Params &p, const AAProblem &q, size_t lds) {
  return dispatch_tw_six<3, true>(tw, p, q, lds);
}
