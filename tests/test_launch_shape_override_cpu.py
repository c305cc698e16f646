"""aa_set_launch_shape, the test hook over the launch-shape model (include/aa_interp.h has its rules), through aa_probe_launch_shape: which
requests are honoured and which are not looked at, per family; what a forced shape means for groups and grid; and that the model is what
tests/golden/launch_shapes.json froze once the hook is back at (0, 0).  No GPU: the hook lives inside the model, host arithmetic.

A request is honoured by what the plan knows alone (strips, LDS per strip, oH) — test_an_occupancy_answer_never_decides holds it to that,
and tests/test_launch_shape_gpu.py relies on it when it requires every shape it asks for to have run."""
import ctypes
import itertools
import threading

import pytest

from interpolate_antialiasing_amd import _lib
from launch_shape_cases import FAMILIES, FROZEN, question, shape

V1, V3, DOWN, UP = _lib.LAUNCH_V1, _lib.LAUNCH_V3, _lib.LAUNCH_F32_DOWN, _lib.LAUNCH_F32_UP
STRIPPED = {"v3": V3, "f32_down": DOWN, "f32_up": UP}
ROWS_PER_BAND = {V1: 8, V3: 8, DOWN: 8, UP: 16}
PADS8 = {V1: False, V3: True, DOWN: True, UP: True}
OCC = [24, 12, 8, 6, 4, 4, 3, 3]  # resident workgroups of 1..8 strips: five strips (4 x 5 = 20 waves) lose to single ones (24), the model drops


@pytest.fixture(autouse=True)
def model_chooses_afterwards():
    _lib.set_launch_shape(0, 0)
    yield
    _lib.set_launch_shape(0, 0)


def _row(family, nstrips=5, spb=None, forced=0, items=6, H=180, oH=83, lds=4096, occupancy=OCC, cus=None, taps_w=5):
    """One question of the model.  The first generation has no strips: one of 256 threads."""
    if family == V1:
        return question(V1, 1, 1, 0, items, H, oH, 5, taps_w, lds, 0, 256, [-1] * 8, cus=cus)
    spb = (nstrips if nstrips <= 8 else 4) if spb is None else spb
    return question(family, nstrips, spb, forced, items, H, oH, 5, taps_w, lds, 1 if family == DOWN else 0, 0, occupancy, cus=cus)


def _ask(q, spb=0, ybands=0):
    """[spb, ybands, groups, grid] of q with the hook at (spb, ybands); the hook is at (0, 0) afterwards."""
    _lib.set_launch_shape(spb, ybands)
    try:
        rc, got = shape(q)
    finally:
        _lib.set_launch_shape(0, 0)
    assert rc == 0
    return got


def _max_yb(family, oH):
    return max(oH // ROWS_PER_BAND[family], 1)


def test_the_setter_returns_the_previous_setting():
    assert _lib.set_launch_shape(0, 0) == (0, 0)
    assert _lib.set_launch_shape(2, 3) == (0, 0)
    assert _lib.set_launch_shape(8, 64) == (2, 3)
    assert _lib.set_launch_shape(0, 5) == (8, 64)
    assert _lib.set_launch_shape(4, 0) == (0, 5)
    assert _lib.set_launch_shape() == (4, 0)
    # requests no rule honours are stored as the nearest value the return carries: none of them changes an answer (below)
    assert _lib.set_launch_shape(-3, -1) == (0, 0)
    assert _lib.set_launch_shape(1000, 1 << 20) == (0, 0)
    assert _lib.set_launch_shape(0, 0) == (255, 0xFFFF)
    # no fused launch on a thread: asked on a thread of its own, since the record is per thread and in a whole-suite run on a GPU the
    # tests before this one (test_launch_shape_gpu.py) have launched fused kernels on pytest's
    seen = []
    asker = threading.Thread(target=lambda: seen.append(_lib.last_launch_shape()))
    asker.start()
    asker.join()
    assert seen == [None]


# oH -> min(max_yb, 64) with 8 rows per band, with the up kernel's 16
TOPS = {7: (1, 1), 41: (5, 2), 83: (10, 5), 800: (64, 50), 1100: (64, 64)}


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("oH", sorted(TOPS))
def test_band_counts_honoured_and_refused(family, oH):
    """1 <= ybands <= min(max_yb, 64) is taken as it is; anything else leaves the model's own count: max_yb + 1, 65, 0, negative."""
    fam = FAMILIES[family]
    q = _row(fam, oH=oH, H=2 * oH + 9)
    own = _ask(q)
    max_yb = _max_yb(fam, oH)
    top = min(max_yb, 64)
    assert top == TOPS[oH][fam == UP]
    for yb in sorted(v for v in {1, 2, 3, top - 1, top} if 1 <= v <= top):
        got = _ask(q, 0, yb)
        assert got[1] == yb and got[0] == own[0], (family, oH, yb, got, own)  # (the grouping does not depend on the bands)
    for yb in (top + 1, max_yb + 1, 65, 66, 1000, 0, -1, -64):
        assert _ask(q, 0, yb) == own, (family, oH, yb)


@pytest.mark.parametrize("family", sorted(STRIPPED))
def test_groupings_honoured_and_refused(family):
    fam = STRIPPED[family]
    q = _row(fam)  # five strips: the plan groups them, the model drops to single strips
    own = _ask(q)
    assert own[0] == 1
    for s in (1, 2, 3, 4, 5):
        got = _ask(q, s, 0)
        assert got[0] == s, (family, s, got)
        # kept as a forced plan's is, and the band count is the model's for that grouping
        assert got == _ask(_row(fam, spb=s, forced=1)), (family, s)
    for s in (6, 7, 8, 9, 255, 0, -1, -5):  # more than the strips there are, more than a workgroup's eight waves, nothing
        assert _ask(q, s, 0) == own, (family, s)
    wide = _row(fam, nstrips=11)  # the plan's groups of 4
    assert _ask(wide)[0] in (1, 4)
    for s in range(1, 9):
        assert _ask(wide, s, 0)[0] == s
    assert _ask(wide, 9, 0) == _ask(wide)
    # a grouping with a short last group (5 = 2 + 2 + 1, 4 + 1; 11 = 8 + 3) is a grouping like any other
    assert _ask(q, 2, 0)[0] == 2 and _ask(q, 4, 0)[0] == 4 and _ask(wide, 8, 0)[0] == 8


@pytest.mark.parametrize("family", sorted(STRIPPED))
def test_a_workgroup_holds_64_kib_of_lds(family):
    """lds * spb <= 64 KiB, for all three families (the fused uint8 kernel's developer knob has no such rule: the hook is stricter)."""
    fam = STRIPPED[family]
    for lds, fits in ((16384, 4), (16385, 3), (16400, 3), (8192, 8), (8193, 7), (13107, 5), (13108, 4), (65536, 1), (32768, 2), (32769, 1)):
        q = _row(fam, nstrips=8, spb=1, lds=lds)
        own = _ask(q)
        assert own[0] == 1
        for s in range(1, 9):
            got = _ask(q, s, 0)
            if s <= fits:
                assert lds * s <= 65536 and got[0] == s, (family, lds, s, got)
            else:
                assert lds * s > 65536 and got == own, (family, lds, s, got)
    q = _row(fam, nstrips=8, spb=1, lds=65537)  # not even one: the request for 1 changes nothing either
    assert _ask(q, 1, 0) == _ask(q)


def test_the_first_generation_has_no_grouping():
    q = _row(V1, oH=83, H=180, lds=9000)
    own = _ask(q)
    assert own[0] == 1
    for s in (1, 2, 4, 8):
        assert _ask(q, s, 0) == own
        got = _ask(q, s, 3)  # ... and the band count beside it is still honoured
        assert got[:2] == [1, 3] and got[2] == got[3] == 6 * 3


@pytest.mark.parametrize("family", sorted(STRIPPED))
def test_both_components_stand_alone(family):
    """A refused component is the model's own, whatever becomes of the other one."""
    fam = STRIPPED[family]
    q = _row(fam)
    assert _ask(q, 2, 3)[:2] == [2, 3]
    assert _ask(q, 9, 3) == _ask(q, 0, 3) and _ask(q, 9, 3)[:2] == [1, 3]
    assert _ask(q, 2, 65) == _ask(q, 2, 0) and _ask(q, 2, 65)[0] == 2
    assert _ask(q, 9, 65) == _ask(q)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_groups_and_grid_under_an_override(family):
    fam = FAMILIES[family]
    for nstrips, items, oH in ((5, 2, 41), (3, 2, 83), (5, 7, 41), (11, 3, 83), (1, 1, 41)):
        q = _row(fam, nstrips=nstrips, items=items, oH=oH, H=2 * oH + 5)
        top = _max_yb(fam, oH)
        own = _ask(q)
        for s, yb in itertools.product((1, 2, 4, 5, 8), sorted({1, 2, 3, top} - set(range(top + 1, 4)))):
            got = _ask(q, s, yb)
            assert got[1] == yb and got[0] == (s if fam != V1 and s <= nstrips else own[0]), (family, nstrips, s, yb, got)
            sgroups = 1 if fam == V1 else -(-nstrips // got[0])
            assert got[2] == items * yb
            assert got[3] == (-(-got[2] // 8) * 8 if PADS8[fam] else got[2]) * sgroups, (family, nstrips, items, s, yb, got)
    # beyond 2^31 - 1 workgroups: no grid
    big = _row(fam, nstrips=5, items=1 << 29, oH=83, H=180)
    got = _ask(big, 1, 1)
    if fam == V1:
        assert got[1:] == [1, 1 << 29, 1 << 29]
        assert _ask(big, 0, 4)[1:] == [4, 1 << 31, 0]
        assert _ask(big, 0, 3)[1:] == [3, 3 << 29, 3 << 29]
    else:
        assert got == [1, 1, 1 << 29, 0]                      # 5 x 2^29 workgroups
        assert _ask(big, 5, 1) == [5, 1, 1 << 29, 1 << 29]   # one workgroup of five strips each
        assert _ask(big, 5, 4) == [5, 4, 1 << 31, 0]
        assert _ask(big, 5, 3) == [5, 3, 3 << 29, 3 << 29]
        assert _ask(big, 4, 2) == [4, 2, 1 << 30, 0]         # 2 x 2^30


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_an_occupancy_answer_never_decides(family):
    """Every request is honoured or not by the rules alone, whatever the runtime would answer and however many CUs there are; a
    component that is not honoured is the model's own for the other one."""
    fam = FAMILIES[family]
    answers = ([-1] * 8, [1] * 8, [32, 16, 10, 8, 6, 5, 4, 4], [2, 1, -1, -1, -1, -1, -1, -1], [16] * 8, OCC)
    top = _max_yb(fam, 41)
    for lds, nstrips in ((4096, 5), (16384, 8), (20000, 3)):
        for occ, cus, items in itertools.product(answers, (1, 64, 256, 304), (1, 2, 4096)):
            q = _row(fam, nstrips=nstrips, lds=lds, occupancy=occ, cus=cus, items=items, oH=41, H=97)
            own = _ask(q)
            for s, yb in itertools.product((1, 2, 3, 4, 5, 8, 9), (1, 2, top, top + 1)):
                got = _ask(q, s, yb)
                s_rule = fam != V1 and 1 <= s <= 8 and s <= nstrips and lds * s <= 65536
                assert got[0] == (s if s_rule else own[0]), (family, lds, nstrips, occ, cus, items, s, yb, got)
                assert got[1] == (yb if yb <= top else _ask(q, s, 0)[1]), (family, lds, nstrips, occ, cus, items, s, yb, got)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_frozen_model_after_setting_and_resetting(family):
    rows = [r for r in FROZEN["rows"] if r[0] == FAMILIES[family]]
    sample = rows[::max(len(rows) // 150, 1)]
    assert len(sample) >= 100
    moved = 0
    for i, r in enumerate(sample):
        want = (1 + i % 8, 1 + i % 5)
        assert _lib.set_launch_shape(*want) == (0, 0)
        rc, forced = shape(question(*r[:13]))
        assert rc == 0
        moved += forced != r[13:]
        assert _lib.set_launch_shape(0, 0) == want
        rc, got = shape(question(*r[:13]))
        assert rc == 0 and got == r[13:], (r[:13], got, r[13:])
    assert moved >= len(sample) // 4, (family, moved)  # (the hook did change answers in between)
