"""The ragged calls' edge fixture without a GPU: the numpy restatement against the fixture (and the fixture against Pillow where it
imports); every case sits on the tile boundary it is named for, worked out from the restatement's coefficients and from the tile sizes as
the source text of csrc/aa_many.h and csrc/aa_many.hip states them; and the host planner, through ctypes, accepts every case and counts
the same work units.  If a tile size changes, the boundary test fails and names the case to move: the GPU tests do not go quietly blind."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import resize_many_edges_ref as ref  # noqa: E402

from interpolate_antialiasing_amd import _lib  # noqa: E402

G = ref.gen()
CASE_NAMES = [cs.name for cs in G.CASES]
FILTER_IDS = {"linear": _lib.FILTER_LINEAR, "cubic": _lib.FILTER_CUBIC, "box": _lib.FILTER_BOX, "hamming": _lib.FILTER_HAMMING,
              "lanczos": _lib.FILTER_LANCZOS}
AA_MAX_KSIZE = 4096


@pytest.mark.parametrize("name", CASE_NAMES)
def test_restatement_reproduces_the_fixture(name):
    cs = G.case(name)
    for f in cs.filters:
        for i in range(len(cs.items)):
            ref.assert_matches_fixture(f"{name}/{f}/{i}", ref.item(name, i), ref.restated(name, f, i))


def test_fixture_regenerates_from_pillow():
    pytest.importorskip("PIL.Image")
    results = [(G.crc(ref.item(cs.name, i)), G.pillow(cs, f, i, ref.item(cs.name, i))) for _, cs, f, i in G.entries()]
    fx = ref.fixture()
    packed = G.pack(results)
    assert set(packed) == set(fx)
    for key, arr in packed.items():
        assert np.array_equal(arr, fx[key]), key


def test_the_constants_are_read_from_the_source_text():
    k = ref.constants()
    assert k["STRIP"] == _lib.MANY_STRIP  # (the one the package mirrors)
    assert all(k["VPIXELS"][e] * e % 4 == 0 for e in (1, 2, 3, 4))  # a piece of the converting pass is whole dwords
    assert [ref.chunk_cols(e) for e in (1, 2, 3, 4)] == [(4 * k["CHUNK_DWORDS"] - 4) // e for e in (1, 2, 3, 4)]


def test_every_case_of_the_issue_is_there():
    by = {cs.name: cs for cs in G.CASES}
    assert set(G.EXPECT) == set(by) and sorted(G.WIDE + G.WIDE_PLACED + G.CHUNKED + G.CHUNKED_PLACED) == sorted(by)
    wide = {(cs.c, cs.out[1]) for cs in G.CASES if cs.name in G.WIDE}
    assert wide == {(1, 1027), (3, 1025), (3, 342), (3, 683), (2, 513), (4, 257), (4, 256), (1, 2048)}
    for cs in G.CASES:
        assert 2 <= len(cs.items) <= 6 and any(it[:2] == (4, 37) for it in cs.items), cs.name  # an ordinary small image in every case
        assert all(2 <= it[0] <= 8 for it in cs.items) and 3 <= cs.out[0] <= 8, cs.name
        assert all(it[0] * it[1] <= 9000 * 8 for it in cs.items), cs.name
        if cs.name in G.WIDE:
            assert [it[:2] for it in cs.items] == [(5, 400), (6, 2100), (4, 37)] and {"linear", "cubic"} <= set(cs.filters)
    assert "box" in by["w_c1_2048"].filters
    assert (by["pw_c3_700"].out, by["pw_c1_1100"].out, by["pw_c3_1100"].out) == ((3, 700), (3, 1100), (3, 1100))
    assert all(v != 0 for n in G.WIDE_PLACED for v in by[n].fill)
    assert by["pw_c3_700"].items[0][3:] == ((3, 120), (0, 300)) and by["pw_c3_700"].items[1][4] == (-1, 341)
    assert {(by[n].c, max(it[1] for it in by[n].items), by[n].out[1]) for n in G.CHUNKED if n.startswith("k_")} == \
        {(4, 2100, 9), (4, 4600, 70), (2, 4200, 9), (2, 9000, 70)}
    assert (5, 4200, None) in by["k_c4_70"].items and by["k_c2_9"].items[2][2] == (7.5, 0.5, 4190.25, 5.5)
    for c in (3, 4):
        assert by[f"l_c{c}_lin2"].items[0][:2] == (5, 4000) and by[f"l_c{c}_lin2"].out[1] == 2 and by[f"l_c{c}_lin2"].filters == ("linear",)
        assert by[f"l_c{c}_box1"].items[0][:2] == (5, 3000) and by[f"l_c{c}_box1"].out[1] == 1 and by[f"l_c{c}_box1"].filters == ("box",)
        pk = by[f"pk_c{c}_2"]
        assert pk.items[0][:2] == (5, 4000) and pk.items[0][3][1] == 4 and pk.c == c


# ---- every case sits on the boundary it is named for -------------------------------------------------------------------------------------
def _claims(name):
    return [(cls, what) for cls, what in G.EXPECT[name].items()]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_every_case_sits_on_the_boundary_it_is_named_for(name):
    cs = G.case(name)
    k = ref.constants()
    move = f"{name} no longer crosses what it is there for: move it (tests/golden/make_golden_resize_many_edges.py)"
    assert G.EXPECT[name], name
    for cls, what in _claims(name):
        e = ref.elem_bytes(cs.c, cls)
        ow = cs.out[1]
        if "vstrips" in what:
            assert ref.vstrips(ow, e) == what["vstrips"], (move, cls, "vertical strips", ref.vstrips(ow, e))
            assert ref.pieces(ow, e) == what["pieces"], (move, cls, "pieces of the converting pass", ref.pieces(ow, e))
        for (f, i), want in what.get("chunks", {}).items():
            got = ref.hstrip_chunks(name, f, i, e)
            assert got == want, (move, cls, f, i, "chunks per horizontal strip", got, "segments", ref.hstrip_segments(name, f, i), "chunk", ref.chunk_cols(e))
        for (f, i) in what.get("window", {}):
            a = ref.axis(name, f, i, 1)
            assert int(a[4].max()) > ref.chunk_cols(e), (move, cls, f, i, "longest window", int(a[4].max()), "chunk", ref.chunk_cols(e))
            assert a[2] <= AA_MAX_KSIZE
        for (f, i), want in what.get("spans", {}).items():
            a = ref.axis(name, f, i, 1)
            got = max(len(ref.window_chunks(name, f, i, e, x)) for x in range(len(a[3])))
            assert got == want, (move, cls, f, i, "chunks the widest-spread window has taps in", got)
        for (f, i) in what.get("origin", {}):
            assert ref.axis(name, f, i, 1)[0] > 0, (move, cls, f, i, "the hull begins at column 0")
        for i, want in what.get("covered", {}).items():
            a = ref.axis(name, cs.filters[0], i, 1)
            if want is None:
                assert a is None, (move, cls, i, "the item lies on the canvas")
                continue
            cb0, cb1 = a[5] * e, (a[5] + len(a[3])) * e
            assert (cb0 // k["VBYTES"], (cb1 - 1) // k["VBYTES"]) == want, (move, cls, i, "covered bytes", cb0, cb1)


def test_the_placed_item_edges_lie_where_the_comments_say():
    """The byte positions the wide placed cases are built around, each against the strip and piece sizes of the source text."""
    k = ref.constants()
    vb = k["VBYTES"]

    def covered(name, i, e):
        a = ref.axis(name, "linear", i, 1)
        return a[5] * e, (a[5] + len(a[3])) * e

    # 3 interleaved bytes per pixel on the [3, 700] canvas
    cb0, cb1 = covered("pw_c3_700", 0, 3)
    assert cb0 % 4 == 0 and cb0 < vb < cb1                      # straddles the seam, starts on a dword
    cb0, cb1 = covered("pw_c3_700", 1, 3)
    assert cb0 == vb - 1                                        # its first byte is the last byte of strip 0: a dword shared with fill
    cb0, cb1 = covered("pw_c3_700", 2, 3)
    assert 2 * vb <= cb0 and cb1 <= 700 * 3                      # wholly in strip 2
    cb0, cb1 = covered("pw_c3_700", 3, 3)
    assert cb0 == 0 and cb1 > vb and ref.axis("pw_c3_700", "linear", 3, 1)[5] == 0 and G.case("pw_c3_700").items[3][4][1] < 0
    piece = k["VPIXELS"][3] * 3
    cb0, cb1 = covered("pw_c3_700", 5, 3)
    assert cb0 % 4 != 0 and cb0 < piece < cb1 and cb0 // 4 == piece // 4 - 1  # its first dword is the last one of piece 0 and holds fill
    assert covered("pw_c3_700", 3, 3)[1] > piece                  # and a cropped item crosses the piece seam too
    # planes on the [3, 1100] canvas
    cb0, cb1 = covered("pw_c1_1100", 0, 1)
    assert cb0 % 4 == 0 and cb0 < vb < cb1
    assert covered("pw_c1_1100", 1, 1)[0] == vb - 1
    assert covered("pw_c1_1100", 2, 1)[0] >= vb
    cb0, cb1 = covered("pw_c1_1100", 3, 1)
    assert cb0 == 0 and cb1 > vb
    # 4 and 2 interleaved bytes per pixel
    for name, e in (("pw_c4_300", 4), ("pw_c2_600", 2)):
        cb0, cb1 = covered(name, 0, e)
        assert cb0 % 4 == 0 and cb0 < vb < cb1, name
        cb0, cb1 = covered(name, 1, e)
        assert cb0 // 4 == vb // 4 - 1 and cb1 > vb, name         # its first dword is the last one of strip 0
    assert covered("pw_c2_600", 1, 2)[0] % 4 == 2                  # ... and half of it is fill


def test_the_second_strip_of_a_chunked_row_begins_mid_row():
    for f in ("linear", "cubic"):
        for name, i in (("k_c4_70", 0), ("k_c4_70", 1), ("k_c4_70", 3), ("k_c2_70", 0)):
            segs = ref.hstrip_segments(name, f, i)
            assert len(segs) == 2 and segs[0][0] == 0 and segs[1][0] > 1000, (name, f, i, segs)


# ---- the planner accepts every case ------------------------------------------------------------------------------------------------------
def _plan(name, f, cls):
    """-> (rc, header, item records, placement records or None) of the case's plan; the data pointers are never dereferenced."""
    cs = G.case(name)
    L = _lib.load()
    layout = _lib.NHWC if cls == "interleaved" else _lib.NCHW
    n, c = len(cs.items), cs.c
    recs = (_lib.ManyImage * n)()
    for i, it in enumerate(cs.items):
        h, w, box = it[:3]
        r = recs[i]
        r.data_dev = 4096 + 16 * i
        r.H, r.W = h, w
        if layout == _lib.NHWC:
            r.stride_row, r.stride_px, r.stride_ch = w * c + 5, c, 1
        else:
            r.stride_row, r.stride_px, r.stride_ch = w + 3, 1, h * (w + 3) + 1
        if box is not None:
            r.has_box = 1
            for q in range(4):
                r.box[q] = box[q]
    precs = fl = None
    if cs.kind == "placed":
        precs = (_lib.ManyPlace * n)()
        for i, it in enumerate(cs.items):
            precs[i].vH, precs[i].vW, precs[i].oy, precs[i].ox = it[3] + it[4]
        fl = (ctypes.c_uint8 * 4)(*(list(cs.fill) + [0] * (4 - len(cs.fill))))
    nbytes = L.aa_many_desc_bytes_placed(n)
    buf = (ctypes.c_uint8 * nbytes)()
    ws = ctypes.c_size_t(0)
    rc = L.aa_many_plan_placed(FILTER_IDS[f], layout, n, c, cs.out[0], cs.out[1], recs, precs, fl, ctypes.addressof(buf), nbytes, ctypes.byref(ws))
    hd, its, _ = _lib.many_desc_view(buf, n)
    return rc, hd, its, (_lib.many_placed_view(buf, n) if cs.kind == "placed" else None), buf


@pytest.mark.parametrize("name,cls", ref.classes(CASE_NAMES))
def test_the_planner_accepts_every_case_and_counts_the_same_units(name, cls):
    cs = G.case(name)
    for f in cs.filters:
        rc, hd, its, pls, _buf = _plan(name, f, cls)
        assert rc == 0, (name, f, cls, _lib.strerror(rc))  # (AA_ERR_KSIZE would refuse a case before the GPU ever saw it)
        assert hd.kind == (_lib.MANY_PLAN_PLACED if cs.kind == "placed" else 0)
        assert hd.hunits == ref.hunits(name, f, cls), (name, f, cls)
        for i in range(len(cs.items)):
            ay, ax = ref.axis(name, f, i, 0), ref.axis(name, f, i, 1)
            if ax is None:
                assert (its[i].hull_w, its[i].ksize_w, pls[i].mw) == (0, 0, 0), (name, f, i)
                continue
            assert (its[i].oy, its[i].hull_h, its[i].ksize_h) == ay[:3], (name, f, i)
            assert (its[i].ox, its[i].hull_w, its[i].ksize_w) == ax[:3], (name, f, i)
            if pls is not None:
                assert (pls[i].mh, pls[i].dy, pls[i].mw, pls[i].dx) == (len(ay[3]), ay[5], len(ax[3]), ax[5]), (name, f, i)
