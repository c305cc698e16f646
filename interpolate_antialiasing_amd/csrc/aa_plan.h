// aa_plan.h — the fused families as the layer above them (aa_api.hip) sees them: each one's plan, which makes every choice that does not
// depend on the pointers (false: no kernel of the family takes the problem), and its launch, which makes the few that do and does not
// decline.  Plain data and declarations only: the kernels and their parameter blocks stay in the families' own files.
#pragma once

#include "aa_common.h"

// ---- the first-generation uint8 kernel (aa_fused_u8.hip): channels_last, Pillow arithmetic, dense tensors
struct V1Plan {
  int TW, C;
  int xbands, bw;        // column bands, output columns per band (a multiple of 4)
  int ring_rows, pitch;  // LDS ring of the intermediate: depth in rows, bytes per row
  int block;             // threads per workgroup
  size_t lds;
};
bool aa_v1_plan(const AAProblem &q, V1Plan *pl);
int aa_v1_launch(const V1Plan &pl, const AAProblem &q);

// ---- the fused uint8 kernel (aa_fused_u8_v3.hip; the kernel in aa_fused_u8_v3_impl.h, the compiled set in aa_fused_u8_v3_list.h)
struct FusedU8V3Params;
// One kernel of the compiled set, as the plan chose it: its route and every template argument, and the unit that compiled it
struct V3Kernel;
typedef int (*V3Launch)(const V3Kernel &k, const FusedU8V3Params *p, const AAProblem *q, size_t lds);  // (q == nullptr: does the unit
                                                                                                       // hold k?  Launches nothing)
struct V3Kernel {
  int route, C, TW, MAXC, UPK, PL, SP;
  bool ALPHA, FLT, fast, NONNEG, TWO_DMA, PERIODIC;  // fast: AA_V3_FLT_FAST
  V3Launch launch;
};
struct V3Plan {
  V3Kernel k;       // the kernel
  V3Kernel groups;  // plane groups: the same problem, three planes per wave (groups.launch == nullptr: not for this problem)
  bool planar;
  int C;     // bytes per pixel of the data (1: planar)
  int cap;   // output columns per strip
  int nseg;  // 16-byte pieces per staged row segment
  unsigned row_pitch;                              // bytes between input rows
  unsigned long long img_in_bytes, img_out_bytes;  // bytes between the images (planes) the kernel sees
  bool v1_first;  // the first-generation kernel does this shape better: it runs instead whenever aa_v1_plan takes the problem
  const char *variant;
};
bool aa_v3_plan(const AAProblem &q, bool fast, V3Plan *pl);  // (fast: the tolerance mode, AA_FLAG_FAST)
int aa_v3_launch(const V3Plan &pl, const AAProblem &q);

// ---- the fused float kernels (aa_fused_float.hip; the kernels in aa_fused_float_impl.h and aa_fused_float_up_impl.h, the compiled set in
// aa_fused_float_list.h)
// One kernel of the compiled set, as the plan chose it, with its strip geometry and the unit that compiled it
struct F32Plan;
typedef int (*F32Launch)(const F32Plan &k, const AAProblem *q);  // (q == nullptr: does the unit hold k?  Launches nothing)
struct F32Plan {
  // F32_DOWN: fused_f32_nchw_kernel<NQ = width, G, NDMA, MAXC = vert, DT, CS = cs>;
  // F32_UP: fused_f32_nchw_up_kernel<U = width, G, KR = vert, CPL = cs, DT> (NDMA 1)
  int kernel, DT, cs, width, vert, G, NDMA;
  int nstrips, strip_w, nseg;
  int store_nt, lds_extra;  // F32_UP: the store form and the LDS it adds per strip (aa_f32_launch: they depend on the output pointer)
  const char *variant;
  F32Launch launch;
};
bool aa_f32_plan(const AAProblem &q, bool fast, F32Plan *pl);
int aa_f32_launch(const F32Plan &pl, const AAProblem &q);

// A unit's launch result as a status: 1 launched; 0 is launch_k finding a grid beyond 2^31 workgroups, a launch that cannot be made
inline int aa_launch_status(int rc) { return rc == 1 ? AA_OK : rc < 0 ? rc : AA_ERR_HIP; }
