// aa_launch_shape.h — the launch shape of the fused families: strips per workgroup, row bands, workgroups.  Every fused launch chooses
// the three from the problem's sizes and the device (CU count, occupancy of its kernel), never from the pointers: host arithmetic over plain
// data (aa_interp.h: aa_launch_shape_in), written once in aa_launch_shape.hip and frozen by tests/test_launch_shape_frozen_cpu.py through
// aa_probe_launch_shape.  A family's launch_k asks through aa_kernel_launch_shape (aa_common.h), bound to its kernel's address.  No HIP here.
#pragma once
#include "../../include/aa_interp.h"

// Occupancy source: what aa_resident_blocks answers for a workgroup of `strips` strips (64 * strips threads, in.lds * strips bytes), -1 when
// the query failed.  nullptr: in.occupancy[strips] answers.
typedef int (*AAResidentFn)(void *ctx, int strips);
// Fills *out; out->grid == 0 where the grid would exceed 2^31 - 1 workgroups (the launch returns 0: AA_ERR_HIP).
// tag: the kernel's template arguments (and store form) as the family's debug line of developer builds prints them, or nullptr.
void aa_launch_shape(const aa_launch_shape_in &in, AAResidentFn resident, void *ctx, const int *tag, aa_launch_shape_out *out);
