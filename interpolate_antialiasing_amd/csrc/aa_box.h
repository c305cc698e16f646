// aa_box.h — box tables (Pillow's Image.resize(box=...); include/aa_interp.h, "box tables") as aa_api.hip sees them.
#pragma once

#include "aa_common.h"

// One axis of a box call: Pillow's source interval [in0, in1) of the axis and the hull [origin, origin + hull) of all its windows.
// The table has in_size = hull and xmin[] relative to origin; centres and weights come from the unshifted in0.
struct AABoxAxis {
  int64_t origin, hull, out;
  double in0, in1;
  int ksize, scatter_ksize;
  void *table;
};
// the two AA_TABLE_PIL box tables of a call as one launch (tables beyond the one-workgroup form: one after the other, as aa_table_build2)
int aa_launch_table_build_box_pair(int filter, const AABoxAxis &a, const AABoxAxis &b, hipStream_t stream);
