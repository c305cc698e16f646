"""Shared by the launch-shape CPU tests: the frozen rows of tests/golden/launch_shapes.json, the families they name, and one question put
to the launch-shape model (csrc/aa_launch_shape.h) through aa_probe_launch_shape.  Not a test module."""
import ctypes
import json
import os

from interpolate_antialiasing_amd import _lib

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_shapes.json")) as _f:
    FROZEN = json.load(_f)
FAMILIES = {"v1": _lib.LAUNCH_V1, "v3": _lib.LAUNCH_V3, "f32_down": _lib.LAUNCH_F32_DOWN, "f32_up": _lib.LAUNCH_F32_UP}


def question(family, nstrips, spb, forced, items, H, oH, taps_h, taps_w, lds, saturation, threads, occupancy, cus=None):
    q = _lib.LaunchShapeIn()
    q.family, q.nstrips, q.strips_per_block, q.spb_forced = family, nstrips, spb, forced
    q.items, q.H, q.oH, q.taps_h, q.taps_w = items, H, oH, taps_h, taps_w
    q.lds, q.saturation, q.threads, q.cus = lds, saturation, threads, FROZEN["cus"] if cus is None else cus
    q.occupancy[0] = -1
    for s, nb in enumerate(occupancy, 1):
        q.occupancy[s] = nb
    return q


def shape(q):
    out = _lib.LaunchShapeOut()
    rc = _lib.load().aa_probe_launch_shape(ctypes.byref(q), ctypes.byref(out))
    return rc, [out.strips_per_block, out.ybands, out.groups, out.grid]
