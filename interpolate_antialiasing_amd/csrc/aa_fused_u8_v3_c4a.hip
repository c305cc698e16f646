// aa_fused_u8_v3_c4a.hip — straight-alpha instantiations (template parameter ALPHA: AA_FLAG_PREMUL_ALPHA, Pillow's RGBA resize) of the
// fused uint8 kernel (aa_fused_u8_v3_impl.h) for 4 interleaved channels, narrow windows (<= 16 taps), <= 4 open output rows.
#include "aa_fused_u8_v3_impl.h"

int aa_v3_launch_c4a(int tw, int maxc, const FusedU8V3Params &p, const AAProblem &q, size_t lds) {
  return dispatch_tw_alpha<4>(tw, maxc, p, q, lds);
}
