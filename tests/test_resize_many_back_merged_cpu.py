"""resize_many_back_merged without a GPU: that the shared cases can tell a wrong kernel from a right one (the order of the adds, the
division), the argument errors of the Python call, the planner (host arithmetic only) through ctypes with its error codes in their
order, the launch checks that come before anything is enqueued, and the ABI."""
import ctypes

import numpy as np
import pytest
import torch

import resize_many_back_merged_ref as ref
from interpolate_antialiasing_amd import _lib
from interpolate_antialiasing_amd import extension_interpolate as aa

ERR_BAD_FILTER, ERR_BAD_DTYPE, ERR_BAD_LAYOUT, ERR_BAD_SHAPE, ERR_NULL, ERR_WORKSPACE, ERR_STRIDES = -1, -2, -3, -4, -5, -6, -10
MAX = (2 ** 31 - 1) // 4
PTR = 4096  # a dummy device address: the planner never follows it
SUM, MEAN = _lib.BACK_MERGE["sum"], _lib.BACK_MERGE["mean"]  # aa_back_merged_plan's merge


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---- the reference is not vacuous -------------------------------------------------------------------------------------------------------
def test_the_order_of_the_adds_shows_in_the_base_case():
    """Conditions on the INPUTS: with the cubic filter the ascending sum of the base case differs from the descending sum in at least one
    bit, so a kernel that adds the members in another order cannot equal the reference."""
    vals = ref.member_values("cubic", ref.BASE_CANVAS, ref.BASE_REGIONS, ref.BASE_GROUPS, ref.BASE_SIZES, ref.BASE_FLIPS)
    up = ref.merge_members(vals, ref.BASE_GROUPS, 3)
    down = ref.merge_members(vals, ref.BASE_GROUPS, 3, descending=True)
    differ = [int((bits(a) != bits(b)).sum()) for a, b in zip(up, down)]
    print(f"ascending vs descending sums: {differ} elements differ per group")
    assert differ[0] > 0, "group 0 (three members) must be sensitive to the order"
    # two members commute: fp32 addition is commutative, only not associative
    assert differ[1] == 0 and differ[2] == 0


def test_the_division_shows_in_the_base_case():
    """s / float32(3) differs from s * float32(1 / 3) in at least one bit of group 0 (M = 3): a reciprocal multiply cannot pass."""
    s = ref.merged_values("cubic", ref.BASE_CANVAS, ref.BASE_REGIONS, ref.BASE_GROUPS, ref.BASE_SIZES, ref.BASE_FLIPS)[0]
    assert len(ref.members(ref.BASE_GROUPS, 0)) == 3
    mean = ref.merged_values("cubic", ref.BASE_CANVAS, ref.BASE_REGIONS, ref.BASE_GROUPS, ref.BASE_SIZES, ref.BASE_FLIPS, "mean")[0]
    assert np.array_equal(bits(mean), bits(s / np.float32(3)))
    recip = (s * np.float32(1.0 / 3.0)).astype(np.float32)
    n = int((bits(mean) != bits(recip)).sum())
    print(f"s / 3 vs s * (1 / 3): {n} of {s.size} elements differ")
    assert n > 0


def test_the_cases_are_what_they_say():
    assert [len(ref.members(ref.BASE_GROUPS, g)) for g in range(3)] == [3, 2, 2]
    for g in range(3):  # every group mixes flipped and unflipped members
        assert {ref.BASE_FLIPS[i] for i in ref.members(ref.BASE_GROUPS, g)} == {True, False}
    assert ref.BASE_SIZES[1][1] > _lib.BACK_TILE
    assert sum(oh * ow for oh, ow in ref.BASE_SIZES) == 23 * 31 + 4 * 300 + 5 * 7
    # a group of one member is resize_many_back's item, for both merges
    one = ref.member_values("linear", ref.BASE_CANVAS, ref.BASE_REGIONS, list(range(7)), [ref.BASE_SIZES[g] for g in ref.BASE_GROUPS])
    for merge in ("sum", "mean"):
        got = ref.merged_values("linear", ref.BASE_CANVAS, ref.BASE_REGIONS, list(range(7)), [ref.BASE_SIZES[g] for g in ref.BASE_GROUPS],
                                merge=merge)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, one))
    # the tie: the sums of planes 2 and 4 are the same bits, and class 4 never wins
    for filt in ref.ORACLE_FILTERS:
        tie = ref.merged_values(filt, ref.tie_canvas(), ref.BASE_REGIONS, ref.BASE_GROUPS, ref.BASE_SIZES, ref.BASE_FLIPS)
        assert all(np.array_equal(bits(s[2]), bits(s[4])) for s in tie)
        lab = ref.labels(tie)
        assert all(not (x == 4).any() for x in lab) and any((x == 2).any() for x in lab)
    # non-finite members: a NaN in one member is a NaN in the sum; +inf and -inf in two members give NaN, and the NaN wins the argmax
    vals = ref.member_values("linear", ref.nonfinite_canvas(), ref.BASE_REGIONS, ref.BASE_GROUPS, ref.BASE_SIZES, ref.BASE_FLIPS)
    k = ref.INF_AT[0]
    assert np.isposinf(vals[0][k]).any() and np.isneginf(vals[5][k]).all() and not np.isnan(vals[0][k]).all()
    assert np.isnan(vals[2][3]).any() and not np.isnan(vals[0][3]).any() and not np.isnan(vals[5][3]).any()
    s = ref.merged_values("linear", ref.nonfinite_canvas(), ref.BASE_REGIONS, ref.BASE_GROUPS, ref.BASE_SIZES, ref.BASE_FLIPS)[0]
    at = np.isposinf(vals[0][k])
    assert np.isnan(s[k][at]).all(), "+inf + -inf is NaN"
    assert np.array_equal(np.isnan(s[3]), np.isnan(vals[2][3]))
    lab = ref.labels([s])[0]
    only = at & ~np.isnan(s[:k]).any(axis=0)
    assert only.any() and (lab[only] == k).all(), "the NaN's class is the label"
    # the further cases
    c, regions, groups, sizes, flips = ref.seventy_case()
    assert len(sizes) == 70 and sorted(set(groups)) == list(range(70)) and len(groups) == 139
    assert {len(ref.members(groups, g)) for g in range(70)} == {1, 2, 3}
    assert any(groups[i] > groups[i + 1] for i in range(len(groups) - 1)), "scattered over the item order"
    vals = ref.merged_values("linear", c, regions, groups, sizes, flips)
    assert [v.shape for v in vals] == [(3,) + s for s in sizes]
    srcs, regions, groups, sizes, flips = ref.list_case()
    vals = ref.merged_values("box", srcs, regions, groups, sizes, flips, "mean")
    assert [v.shape for v in vals] == [(3, 9, 17), (3, 3, 4)] and len({s.shape for s in srcs}) == len(srcs)
    c, regions, groups, sizes = ref.k300_case()
    lab = ref.labels(ref.merged_values("linear", c, regions, groups, sizes))[0]
    assert lab.shape == (5, 4) and lab.max() == 299


# ---- argument errors of the Python call, before any device work -------------------------------------------------------------------------
def test_argument_errors():
    p = torch.zeros(4, 7, 12, 16)
    groups, sizes = [0, 1, 0, 1], [(5, 6), (7, 8)]
    call = aa.resize_many_back_merged
    assert "resize_many_back_merged" in aa.__all__
    with pytest.raises(_lib.AAInterpError, match="no CPU implementation"):
        call(p, groups, sizes)
    with pytest.raises(ValueError):
        call(p, groups, sizes, mode="area")
    with pytest.raises(ValueError, match="reduce"):
        call(p, groups, sizes, reduce="softmax")
    for merge in ("max", None, 0, "SUM"):
        with pytest.raises(ValueError, match="merge"):
            call(p, groups, sizes, merge=merge)
    # groups: its length, its entries, the empty group
    with pytest.raises(ValueError, match=r"groups must hold one entry per item \(4\), got 3"):
        call(p, groups[:3], sizes)
    with pytest.raises(ValueError, match=r"groups must hold"):
        call(p, groups + [0], sizes)
    with pytest.raises(ValueError, match="groups must be N integers"):
        call(p, 3, sizes)
    for bad in (True, False, 0.5, "0", None, (0,)):
        with pytest.raises(ValueError, match=r"groups\[2\] must be an integer"):
            call(p, [0, 1, bad, 1], sizes)
    for bad in (2, -1, 7):
        with pytest.raises(ValueError, match=rf"groups\[3\] = {bad} is outside 0 \.\. 1"):
            call(p, [0, 1, 0, bad], sizes)
    with pytest.raises(ValueError, match=r"group 1 \(sizes\[1\]\) has no member"):
        call(p, [0, 0, 0, 0], sizes)
    # sizes: one entry per GROUP, so a list of another length names a group that is not there or one without members
    with pytest.raises(ValueError, match=r"groups\[1\] = 1 is outside 0 \.\. 0"):
        call(p, groups, sizes[:1])
    with pytest.raises(ValueError, match=r"group 2 \(sizes\[2\]\) has no member"):
        call(p, groups, sizes + [(3, 3)])
    with pytest.raises(ValueError, match=r"groups\[0\] = 0 is outside"):
        call(p, groups, [])
    with pytest.raises(ValueError, match="sizes must be G pairs"):
        call(p, groups, 5)
    with pytest.raises(ValueError, match=r"sizes\[1\]"):
        call(p, groups, [(5, 6), (0, 8)])
    with pytest.raises(ValueError, match=r"sizes\[0\]"):
        call(p, groups, [(5.5, 6), (7, 8)])
    with pytest.raises(ValueError, match=r"sizes\[1\].*beyond"):
        call(p, groups, [(5, 6), (1 << 20, 1 << 18)])
    # what resize_many_back checks, checked the same
    with pytest.raises(NotImplementedError, match=r"pred\[0\]"):
        call(p.double(), groups, sizes)
    with pytest.raises(ValueError, match=r"same K: pred\[1\]"):
        call([p[0], p[1, :3]], [0, 0], [(5, 6)])
    with pytest.raises(ValueError, match="regions must hold"):
        call(p, groups, sizes, regions=[None])
    with pytest.raises(ValueError, match=r"regions\[0\].*inside"):
        call(p, groups, sizes, regions=[(0, 0, 13, 3), None, None, None])
    with pytest.raises(ValueError, match="flips"):
        call(p, groups, sizes, flips=[True])
    for reduce, dt in ((None, torch.float64), (None, torch.uint8), ("argmax", torch.float32), ("argmax", torch.bool), ("greater", torch.int32)):
        with pytest.raises(NotImplementedError, match="out_dtype"):
            call(p, groups, sizes, reduce=reduce, out_dtype=dt)
    with pytest.raises(ValueError, match="K = 300"):
        call(torch.zeros(2, 300, 1, 1).expand(2, 300, 3, 3), [0, 0], [(2, 2)], reduce="argmax", out_dtype=torch.uint8)
    for thr in (float("nan"), float("inf"), 1e39, "x"):
        with pytest.raises(ValueError, match="threshold"):
            call(p, groups, sizes, reduce="greater", threshold=thr)
    # N == 0: G == 0 gives [], a group without members is an error, and a list states K
    assert call([], [], [], channels=19) == [] and call([], [], [], merge="mean", reduce="argmax", channels=19) == []
    assert call(torch.zeros(0, 7, 4, 4), [], []) == []
    with pytest.raises(ValueError, match="channels="):
        call([], [], [])
    with pytest.raises(ValueError, match=r"group 0 \(sizes\[0\]\) has no member"):
        call([], [], [(4, 4)], channels=19)
    # everything in order: only the device is missing
    with pytest.raises(_lib.AAInterpError, match="no CPU implementation"):
        call(p, [1, 0, 1, 1], sizes, "lanczos", regions=[(1, 1, 2, 2)] * 4, flips=[True] * 4, merge="mean", reduce="argmax", out_dtype=torch.int16)


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------
def test_abi_is_additive():
    L = _lib.load()
    assert L.aa_abi_version() == 3
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    for sym in ("aa_back_merged_desc_bytes", "aa_back_merged_plan", "aa_resample_back_merged"):
        assert sym in _lib.EXPORTS and hasattr(L, sym) and sym + "(" in header
        assert sym in header.split("#define AA_INTERP_ABI_VERSION 3")[1].split("*/")[0]  # (listed in the version's comment)
    assert ctypes.sizeof(_lib.BackMergedHeader) == 64 and ctypes.sizeof(_lib.BackGroup) == 32
    size = L.aa_back_merged_desc_bytes
    assert size(7, 3) == 64 + 7 * 96 + 3 * 32 + 32 + 4 * 8 and size(4, 4) == 64 + 4 * 96 + 4 * 32 + 16 + 5 * 8 and size(0, 0) == 72
    assert size(-1, 0) == 0 and size(1, -1) == 0
    assert (SUM, MEAN) == (0, 1) and set(_lib.BACK_MERGE) == {"sum", "mean"}


# ---- the planner ----------------------------------------------------------------------------------------------------------------------
def item(h=6, w=9, oh=3, ow=4, k=7, layout=_lib.NCHW, ptr=PTR, flags=0, strides=None):
    """One aa_back_item as a tuple (data_dev, stride_ch, stride_row, stride_px, h, w, oh, ow, flags) of a dense source in `layout`."""
    if strides is None:
        strides = (1, w * k, k) if layout == _lib.NHWC else (h * w, w, 1)
    return (ptr,) + tuple(strides) + (h, w, oh, ow, flags)


def records(items):
    recs = (_lib.BackItemIn * max(len(items), 1))()
    for r, it in zip(recs, items):
        r.data_dev, r.stride_ch, r.stride_row, r.stride_px, r.h, r.w, r.oh, r.ow, r.flags = it
    return recs


def plan(items, groups, g=None, k=7, filt=_lib.FILTER_LINEAR, layout=_lib.NCHW, merge=SUM, reduce=_lib.BACK_VALUES, out_dtype=_lib.F32, n=None,
         desc=True, short=0, null=()):
    L = _lib.load()
    n = len(items) if n is None else n
    g = (max(groups) + 1 if groups else 0) if g is None else g
    nbytes = L.aa_back_merged_desc_bytes(max(n, 0), max(g, 0)) - short
    buf = (ctypes.c_uint8 * max(nbytes + short, 4096))()
    ws, arena = ctypes.c_size_t(0), ctypes.c_size_t(0)
    offs = (ctypes.c_int64 * max(g, 1))()
    group_of = (ctypes.c_int64 * max(len(groups), 1))(*groups)
    rc = L.aa_back_merged_plan(filt, layout, n, k, None if "items" in null else records(items), g, None if "groups" in null else group_of, merge,
                               reduce, out_dtype, ctypes.addressof(buf) if desc else None, nbytes, None if "ws" in null else ctypes.byref(ws),
                               None if "arena" in null else ctypes.byref(arena), None if "offs" in null else offs)
    return rc, buf, ws.value, arena.value, list(offs)[:max(g, 0)]


def base_items(k=7):
    return [item(h, w, *ref.BASE_SIZES[g], k, ptr=PTR + 4 * i, flags=int(f), strides=(12 * 16, 16, 1))
            for i, ((_, _, h, w), g, f) in enumerate(zip(ref.BASE_REGIONS, ref.BASE_GROUPS, ref.BASE_FLIPS))]


@pytest.mark.parametrize("reduce,out_dtype,eb", [(_lib.BACK_VALUES, _lib.F32, 4), (_lib.BACK_VALUES, _lib.BF16, 2), (_lib.BACK_ARGMAX, _lib.U8, 1),
                                                 (_lib.BACK_ARGMAX, _lib.I64, 8), (_lib.BACK_GREATER, _lib.BOOL, 1)])
def test_plan_groups_members_offsets_and_units(reduce, out_dtype, eb):
    L = _lib.load()
    k, n, g = 7, 7, 3
    items = base_items(k)
    rc, buf, ws, arena, offs = plan(items, ref.BASE_GROUPS, k=k, filt=_lib.FILTER_CUBIC, merge=MEAN, reduce=reduce, out_dtype=out_dtype)
    assert rc == 0
    hd, recs, groups, member, unit0 = _lib.back_merged_desc_view(buf, n, g)
    assert (hd.n, hd.G, hd.K, hd.filter, hd.layout, hd.merge, hd.reduce, hd.out_dtype, hd.ws_bytes, hd.arena_bytes) == (
        n, g, k, _lib.FILTER_CUBIC, _lib.NCHW, MEAN, reduce, out_dtype, ws, arena)
    # the arena: every GROUP on a 16-byte boundary, dense, in order; the units: an output row of a group times 256 columns
    aend = units = slot = 0
    for j, (gr, (oh, ow)) in enumerate(zip(groups, ref.BASE_SIZES)):
        aend = (aend + 15) & ~15
        assert gr.out_off == offs[j] == aend and offs[j] % 16 == 0
        aend += (1 if reduce == _lib.BACK_ARGMAX else k) * oh * ow * eb
        assert (gr.oh, gr.ow, gr.xtiles) == (oh, ow, -(-ow // _lib.BACK_TILE))
        assert unit0[j] == units
        units += oh * gr.xtiles
        # the member list: grouped, ascending within a group
        want = ref.members(ref.BASE_GROUPS, j)
        assert (gr.first, gr.count) == (slot, len(want)) and list(member[slot:slot + gr.count]) == want
        slot += gr.count
    assert aend == arena and slot == n and unit0[g] == units == hd.units
    assert units == sum(oh * -(-ow // 256) for oh, ow in ref.BASE_SIZES) == 23 + 4 * 2 + 5
    # the members are aa_back_many_plan's records at their group's size and place, and the workspace is that plan's
    nbytes = L.aa_back_many_desc_bytes(n)
    buf1 = (ctypes.c_uint8 * nbytes)()
    ws1, arena1, offs1 = ctypes.c_size_t(0), ctypes.c_size_t(0), (ctypes.c_int64 * n)()
    assert L.aa_back_many_plan(_lib.FILTER_CUBIC, _lib.NCHW, n, k, records(items), reduce, out_dtype, ctypes.addressof(buf1), nbytes, ctypes.byref(ws1),
                               ctypes.byref(arena1), offs1) == 0
    assert ws1.value == ws
    _, recs1, _ = _lib.back_desc_view(buf1, n)
    for i, (a, b) in enumerate(zip(recs, recs1)):
        for name, _ in _lib.BackItem._fields_:
            if name != "out_off":
                assert getattr(a, name) == getattr(b, name), (i, name)
        assert a.out_off == offs[ref.BASE_GROUPS[i]] and (a.oh, a.ow) == ref.BASE_SIZES[ref.BASE_GROUPS[i]] and a.flags == int(ref.BASE_FLIPS[i])


def test_plan_empty_and_one_member_groups():
    rc, buf, ws, arena, _ = plan([], [])
    assert (rc, ws, arena) == (0, 0, 0)
    hd, _, _, _, unit0 = _lib.back_merged_desc_view(buf, 0, 0)
    assert hd.n == 0 and hd.G == 0 and hd.units == 0 and list(unit0) == [0]
    L = _lib.load()
    assert L.aa_resample_back_merged(ctypes.addressof(buf), None, _lib.F32, 0.0, None, 0, None, 0, None) == 0  # (nothing is launched)
    # groups = range(n), in any order: the arena follows the GROUPS
    items = [item(oh=3, ow=4, ptr=PTR), item(oh=5, ow=6, ptr=PTR + 4), item(oh=7, ow=2, ptr=PTR + 8)]
    rc, buf, ws, arena, offs = plan(items, [2, 0, 1])
    assert rc == 0 and offs == [0, 848, 1248] and arena == 1248 + 7 * 3 * 4 * 4  # (840 and 848 + 392 bytes, each rounded up to 16)
    _, recs, groups, member, unit0 = _lib.back_merged_desc_view(buf, 3, 3)
    assert list(member) == [1, 2, 0] and [(gr.oh, gr.ow) for gr in groups] == [(5, 6), (7, 2), (3, 4)] and list(unit0) == [0, 5, 12, 15]
    assert [r.out_off for r in recs] == [offs[2], offs[0], offs[1]]


def test_plan_error_codes_and_their_precedence():
    ok, groups = [item(), item(ptr=PTR + 4)], [0, 0]
    bad_shape = [item(h=0), item()]
    assert plan(ok, groups)[0] == 0 and plan(ok, groups, merge=MEAN)[0] == 0
    # the filter before everything; then the layout; then n, K, reduce, G and merge, and K against a label type
    assert plan(bad_shape, [0, 5], filt=5, layout=7, n=-1, g=-1, merge=2, desc=False)[0] == ERR_BAD_FILTER
    assert plan(bad_shape, [0, 5], layout=7, n=-1, g=-1, merge=2, desc=False)[0] == ERR_BAD_LAYOUT
    assert plan(ok, groups, n=-1, desc=False)[0] == ERR_BAD_SHAPE
    assert plan(ok, groups, k=0, desc=False)[0] == ERR_BAD_SHAPE and plan(ok, groups, k=MAX + 1)[0] == ERR_BAD_SHAPE
    assert plan(ok, groups, reduce=3, desc=False)[0] == ERR_BAD_SHAPE
    for g in (-1, 3, 0):  # G outside 0 .. n; G == 0 with n > 0
        assert plan(ok, groups, g=g, desc=False)[0] == ERR_BAD_SHAPE, g
    for merge in (-1, 2):
        assert plan(ok, groups, merge=merge, desc=False)[0] == ERR_BAD_SHAPE, merge
    assert plan(ok, groups, k=257, reduce=_lib.BACK_ARGMAX, out_dtype=_lib.U8, desc=False)[0] == ERR_BAD_SHAPE
    assert plan(ok, groups, k=256, reduce=_lib.BACK_ARGMAX, out_dtype=_lib.U8)[0] == 0
    # the pointers (group_of among them), then the block's size, then the groups' membership, then the items
    for what in ("items", "groups", "ws", "arena", "offs"):
        assert plan(bad_shape, [0, 5], g=2, null=(what,), short=1)[0] == ERR_NULL, what
    assert plan(bad_shape, [0, 5], g=2, desc=False, short=1)[0] == ERR_NULL
    assert plan(bad_shape, [0, 5], g=2, short=1)[0] == ERR_WORKSPACE
    for bad in ([0, 2], [-1, 0], [0, 1 << 40]):  # an entry outside 0 .. G - 1, before the empty group and the items
        assert plan(bad_shape, bad, g=2)[0] == ERR_BAD_SHAPE, bad
    assert plan([item(ptr=None), item()], [1, 1], g=2)[0] == ERR_BAD_SHAPE      # (an empty group before an item's null pointer)
    assert plan([item(ptr=None), item()], [1, 0], g=2)[0] == ERR_NULL
    for kw in ({"h": 0}, {"ow": 0}, {"h": MAX + 1}, {"flags": 2}):
        assert plan([item(), item(strides=(54, -9, 1), **kw)], groups, out_dtype=_lib.F64)[0] == ERR_BAD_SHAPE, kw   # (before strides and dtype)
    assert plan([item(), item(strides=(54, -9, 1))], groups, out_dtype=_lib.F64)[0] == ERR_STRIDES       # (the strides before the dtype)
    # members of one group with different (oh, ow): after the member's own checks, before the dtype
    for kw in ({"oh": 4}, {"ow": 5}, {"oh": 4, "ow": 3}):
        assert plan([item(), item(**kw)], groups, out_dtype=_lib.F64)[0] == ERR_BAD_SHAPE, kw
        assert plan([item(), item(**kw)], [0, 1], g=2)[0] == 0, kw
        assert plan([item(), item(strides=(54, -9, 1), **kw)], groups)[0] == ERR_STRIDES, kw
    # more work units than one grid holds, per group: two members of one group count once
    big = item(oh=MAX, ow=8)
    assert plan([big] * 4, [0, 0, 0, 0], k=1)[0] == 0
    assert plan([big] * 5, [0, 1, 2, 3, 3], k=1)[0] == 0
    assert plan([big] * 5, [0, 1, 2, 3, 4], k=1)[0] == ERR_BAD_SHAPE
    assert plan([item(oh=1 << 20, ow=1 << 20)], [0], k=2)[0] == ERR_BAD_SHAPE   # (K * oh * ow beyond 2^40)
    # the dtype a reduction stores, last
    for reduce, bad in ((_lib.BACK_VALUES, (_lib.U8, _lib.F64, _lib.BOOL, 9)), (_lib.BACK_ARGMAX, (_lib.F32, _lib.BOOL)), (_lib.BACK_GREATER, (_lib.F32, _lib.I64))):
        for dt in bad:
            assert plan(ok, groups, reduce=reduce, out_dtype=dt)[0] == ERR_BAD_DTYPE, (reduce, dt)


# ---- the launch's checks, all before anything is enqueued (no device is touched) ------------------------------------------------------
def test_launch_checks():
    L = _lib.load()
    one = ctypes.c_void_p(256)
    blank = (ctypes.c_uint8 * 512)()
    call = L.aa_resample_back_merged
    assert call(None, one, _lib.F32, 0.0, one, 1 << 20, one, 1 << 20, None) == ERR_NULL
    assert call(ctypes.addressof(blank), one, _lib.F32, 0.0, one, 1 << 20, one, 1 << 20, None) == ERR_BAD_SHAPE  # no plan's block
    rc, buf, ws, arena, _ = plan([item(ptr=256), item(ptr=512)], [0, 0], reduce=_lib.BACK_GREATER, out_dtype=_lib.BOOL)
    assert rc == 0
    d = ctypes.addressof(buf)
    # the other planner's block is not this call's, and this planner's is not the other call's
    assert L.aa_resample_back_many(d, one, _lib.F32, 0.0, one, arena, one, ws, None) == ERR_BAD_SHAPE
    for dt in (_lib.F64, _lib.U8, _lib.I32, 9):
        assert call(d, one, dt, 0.0, one, arena, one, ws, None) == ERR_BAD_DTYPE
    assert call(d, one, _lib.F32, float("nan"), one, arena, one, ws, None) == ERR_BAD_SHAPE
    assert call(d, None, _lib.F32, 0.0, one, arena, one, ws, None) == ERR_NULL
    assert call(d, one, _lib.F32, 0.0, None, arena, one, ws, None) == ERR_NULL
    assert call(d, one, _lib.F32, 0.0, one, arena, None, ws, None) == ERR_NULL
    assert call(d, one, _lib.F32, 0.0, one, arena, one, ws - 1, None) == ERR_WORKSPACE
    assert call(d, one, _lib.F32, 0.0, one, arena - 1, one, ws, None) == ERR_WORKSPACE
    assert call(d, one, _lib.F32, 0.0, one, arena, ctypes.c_void_p(264), ws, None) == ERR_BAD_SHAPE   # (the workspace: 16 bytes)
    assert call(d, ctypes.c_void_p(260), _lib.F32, 0.0, one, arena, one, ws, None) == ERR_BAD_SHAPE   # (the device block: 8 bytes)
    # the sources against their element: the second member's address
    rc, buf, ws, arena, _ = plan([item(ptr=256), item(ptr=258)], [0, 0])
    d = ctypes.addressof(buf)
    assert call(d, one, _lib.F32, 0.0, one, arena, one, ws, None) == ERR_STRIDES
    # a block whose header was damaged after planning
    hd = _lib.back_merged_desc_view(buf, 2, 1)[0]
    hd.merge = 2
    assert call(d, one, _lib.BF16, 0.0, one, arena, one, ws, None) == ERR_BAD_SHAPE
    hd.merge, hd.G = 0, 3
    assert call(d, one, _lib.BF16, 0.0, one, arena, one, ws, None) == ERR_BAD_SHAPE
