"""The launch-shape model (csrc/aa_launch_shape.h) gives every row of tests/golden/launch_shapes.json the strips per workgroup, row
bands, groups and grid recorded there: what the four fused families' own launch code chose at the commit named in the file, before the
model replaced their copies (tests/golden/make_golden_launch_shapes.py made it from that commit's sources and lists the branches the
rows reach).  No GPU: the model is host arithmetic, the CU count and the occupancy answers are part of a row."""
import ctypes

import pytest

from interpolate_antialiasing_amd import _lib
from launch_shape_cases import FAMILIES, FROZEN, question, shape


def test_the_fixture_reaches_every_branch():
    assert FROZEN["cus"] == 256 and FROZEN["columns"][-4:] == ["out_spb", "out_ybands", "out_groups", "out_grid"]
    assert len(FROZEN["census"]) == 27 and min(FROZEN["census"].values()) >= 20, FROZEN["census"]
    assert {r[0] for r in FROZEN["rows"]} == set(FAMILIES.values())


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_every_launch_shape_is_the_frozen_one(family):
    rows = [r for r in FROZEN["rows"] if r[0] == FAMILIES[family]]
    assert len(rows) >= 100
    different = []
    for r in rows:
        rc, got = shape(question(*r[:13]))
        if rc != 0 or got != r[13:]:
            different.append((r[:13], "rc %d" % rc, got, r[13:]))
    assert not different, f"{len(different)} of {len(rows)} shapes differ, the first: {different[0]}"


def test_bad_inputs_are_refused():
    L = _lib.load()
    good = [_lib.LAUNCH_V3, 5, 5, 0, 64, 438, 196, 5, 5, 4096, 0, 0, [24, 12, 8, 6, 4, 4, 3, 3]]
    assert shape(question(*good))[0] == 0
    out = _lib.LaunchShapeOut()
    assert L.aa_probe_launch_shape(None, ctypes.byref(out)) == -5  # AA_ERR_NULL
    assert L.aa_probe_launch_shape(ctypes.byref(question(*good)), None) == -5
    for col, bad in ((0, 4), (0, -1), (1, 0), (2, 0), (2, 9), (4, 0), (5, 0), (6, 0), (7, 0), (8, 0)):
        row = list(good)
        row[col] = bad
        assert shape(question(*row))[0] == -4, (col, bad)  # AA_ERR_BAD_SHAPE
    assert shape(question(*good, cus=0))[0] == -4
    v1 = [_lib.LAUNCH_V1, 1, 1, 0, 64, 438, 196, 5, 5, 9000, 0, 256, [-1] * 8]
    assert shape(question(*v1))[0] == 0
    for threads in (0, 32, 100):
        assert shape(question(*(v1[:11] + [threads] + v1[12:])))[0] == -4
