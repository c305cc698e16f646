// aa_box.h — one weight table to build, as aa_api.hip's three build calls hand it to the launcher in aa_tables.hip.
#pragma once

#include "aa_common.h"

// A box table (Pillow's Image.resize(box=...); include/aa_interp.h, "box tables") has box = 1: [in0, in1) is Pillow's source interval of the
// axis, [origin, origin + in_size) the hull of all its windows.  xmin[] are relative to origin; centres and weights come from the unshifted in0.
struct AATableSpec {
  int64_t in_size, out_size;
  double scale;  // (scale_for's answer; Pillow's tables derive theirs from the sizes or the box)
  int ksize, scatter_ksize;
  void *table;
  int box;
  int64_t origin;
  double in0, in1;
};
// The n = 1 or 2 tables of a call.  Each table that fits one workgroup is built by one workgroup, two such tables by the two workgroups of
// one launch; a larger table takes one launch per phase.
int aa_launch_table_jobs(int filter, int kind, int align_corners, const AATableSpec *specs, int n, hipStream_t stream);
