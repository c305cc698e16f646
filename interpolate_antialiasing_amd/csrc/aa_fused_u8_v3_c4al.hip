// aa_fused_u8_v3_c4al.hip — straight-alpha instantiations (AA_FLAG_PREMUL_ALPHA) of the fused uint8 kernel (aa_fused_u8_v3_impl.h) for
// 4 interleaved channels, narrow windows (<= 16 taps) with 5-6 open output rows (MAXC = 6): Hamming / Lanczos down-scaling by 1 .. ~2.7.
#include "aa_fused_u8_v3_impl.h"

int aa_v3_launch_c4al(int tw, const FusedU8V3Params &p, const AAProblem &q, size_t lds) {
  return dispatch_tw_six<4, false, true>(tw, p, q, lds);
}
