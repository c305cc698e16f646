"""The float ragged calls' edge cases without a GPU: every case of float_many_edges_ref still has the property it is named for, worked
out from oracle.weights / backward_ref's tables and from the tile sizes as the headers' text states them; the host planner accepts every
resize_many_back case and counts the work units the tile size implies; the oracle's fp32 values lie within the dense float64 bound, so
the GPU test's float64 check cannot fail because of its reference; and the references notice a dropped flip and a column tile computed
with another tile's windows.  If a tile size changes, a test here fails and names the case to resize: the GPU tests never pass for
nothing."""
import ctypes

import numpy as np
import pytest

import backward_ref
import float_many_edges_ref as ref
import resize_many_back_bwd_ref as bwd_ref
import resize_many_back_ref as back_ref
from interpolate_antialiasing_amd import _lib

K = ref.constants()
AA_MAX_KSIZE = 4096
FILTER_IDS = {"linear": _lib.FILTER_LINEAR, "cubic": _lib.FILTER_CUBIC, "box": _lib.FILTER_BOX, "hamming": _lib.FILTER_HAMMING,
              "lanczos": _lib.FILTER_LANCZOS}


def resize(name, what):
    return f"{name} no longer reaches what it is there for ({what}): resize it in tests/float_many_edges_ref.py"


def test_the_constants_are_read_from_the_headers():
    assert set(K) == {"BACK_THREADS", "BACK_TILE", "BACK_UNROLL", "EMBED_THREADS", "EMBED_VEC", "BACK_BWD_THREADS", "BACK_BWD_COLS"}
    assert all(v > 0 for v in K.values()) and K["BACK_BWD_THREADS"] % K["BACK_BWD_COLS"] == 0


def test_every_case_is_there():
    assert ref.BACK_CASES == {
        "wide_out": (5, (3, 150), None, (4, 601)), "tile_256": (3, (2, 64), None, (2, 256)), "tile_257": (3, (2, 64), None, (2, 257)),
        "wide_src_shrink": (2, (4, 610), (1, 7, 2, 600), (5, 3)), "tall_shrink": (4, (300, 5), None, (2, 7)),
        "both_long": (3, (90, 110), None, (2, 3)), "many_rows": (1, (40, 3), None, (700, 2))}
    assert set(ref.BACK_16BIT) | set(ref.BACK_REDUCED) <= set(ref.BACK_NAMES) and len(ref.TOGETHER_FLIPS) == len(ref.BACK_NAMES)
    assert ref.EMBED_CASES == {"shrink_40x48": ((40, 48), [(2, 3), (300, 2), (1, 520), (40, 48)]),
                               "wide_source": ((2, 300), [(1, 7), (3, 900), (2, 300)]), "source_1x1_long": ((1, 1), [(1, 600), (300, 1)])}
    assert [ref.MERGED_SHAPES[i] for i in range(5) if ref.MERGED_GROUPS[i] == 0] == [(3, 150), (2, 75), (1, 1)]
    assert [ref.MERGED_FLIPS[i] for i in range(5) if ref.MERGED_GROUPS[i] == 0] == [True, False, True]
    assert [ref.MERGED_SHAPES[i] for i in range(5) if ref.MERGED_GROUPS[i] == 1] == [(90, 110), (2, 600)]
    assert [ref.MERGED_FLIPS[i] for i in range(5) if ref.MERGED_GROUPS[i] == 1] == [False, True]
    assert ref.MERGED_SIZES == [(4, 601), (2, 3)] and ref.MERGED_GROUPS != sorted(ref.MERGED_GROUPS)  # (the groups interleave)
    # the largest tensor of the GPU file
    assert max(k * oh * ow for k, _, _, (oh, ow) in ref.BACK_CASES.values()) == 5 * 4 * 601
    # the source inputs are what they say: NaN all around a region, none inside
    src = ref.back_source("wide_src_shrink")
    assert np.isnan(src).sum() == src.size - 2 * 2 * 600 and not np.isnan(back_ref.view(src, ref.BACK_CASES["wide_src_shrink"][2])).any()
    assert not src.flags.writeable


# ---- resize_many_back: every case has the property it is named for -----------------------------------------------------------------------
def real_windows_in_every_later_tile(filt, w, ow):
    """Whether every column tile after the first has a lane whose window has more than one tap (the box filter's windows have one tap
    when enlarging, whatever the shape) and does not start at column 0."""
    tile = K["BACK_TILE"]
    _, xmin, xsize = ref.windows(filt, w, ow)
    tiles = -(-ow // tile)
    taps = 1 if filt == "box" else 2
    return tiles, all(((xsize[t * tile:(t + 1) * tile] >= taps) & (xmin[t * tile:(t + 1) * tile] > 0)).any() for t in range(1, tiles))


@pytest.mark.parametrize("filt", ref.FILTERS)
def test_wide_out_has_real_windows_in_every_tile(filt):
    (h, w), (oh, ow) = ref.back_extent("wide_out")
    tiles, real = real_windows_in_every_later_tile(filt, w, ow)
    assert tiles > 2, resize("wide_out", f"more than two column tiles of AA_BACK_TILE = {K['BACK_TILE']}: make (oh, ow) wider")
    assert ow % K["BACK_TILE"] != 0, resize("wide_out", "a partial last tile")
    assert real, resize("wide_out", "a lane with xsize > 1 and xmin > 0 in every tile after the first")
    assert int(ref.windows(filt, w, ow)[1].max()) >= w - 3
    # the merged case's group 0 is the same width, and its flipped first member the same source
    assert ref.MERGED_SIZES[0][1] == ow and ref.MERGED_SHAPES[0] == (h, w) and ref.MERGED_FLIPS[0]
    assert real_windows_in_every_later_tile(filt, ref.MERGED_SHAPES[2][1], ow)[1], resize("the merged group 0", "an unflipped member with real windows")


def test_tile_cases_sit_on_the_tile():
    tile = K["BACK_TILE"]
    assert ref.BACK_CASES["tile_256"][3][1] == tile, resize("tile_256", f"exactly AA_BACK_TILE = {tile} output columns")
    assert ref.BACK_CASES["tile_257"][3][1] == tile + 1, resize("tile_257", f"exactly AA_BACK_TILE + 1 = {tile + 1} output columns")
    assert ref.BACK_CASES["tile_256"][1] == ref.BACK_CASES["tile_257"][1] and ref.BACK_CASES["tile_256"][1][1] > 1


@pytest.mark.parametrize("filt", ref.FILTERS)
def test_long_window_cases_have_long_windows(filt):
    for name, axes in ref.LONG_AXES.items():
        src, out = ref.back_extent(name)
        for ax in (0, 1):
            ksize, _, xsize = ref.windows(filt, src[ax], out[ax])
            assert ksize <= AA_MAX_KSIZE, (name, filt, ax, ksize)
            if ax in axes:
                assert int(xsize.max()) >= ref.LONG_TAPS, resize(name, f"a window of {ref.LONG_TAPS} taps along axis {ax} under {filt}: {int(xsize.max())}")
    # the longest row of all is lanczos on wide_src_shrink, under the limit of a table row
    if filt == "lanczos":
        assert 1000 <= ref.windows(filt, 600, 3)[0] <= AA_MAX_KSIZE
    (h, w), _ = ref.back_extent("wide_src_shrink")
    k, hw, region, _ = ref.BACK_CASES["wide_src_shrink"]
    assert w > K["BACK_TILE"] and hw[1] > w and region[1] > 0, resize("wide_src_shrink", "a pitched source wider than a tile")
    assert k < K["BACK_UNROLL"], resize("wide_src_shrink", f"K below AA_BACK_UNROLL = {K['BACK_UNROLL']}")
    assert ref.BACK_CASES["tall_shrink"][0] == K["BACK_UNROLL"], resize("tall_shrink", f"K = AA_BACK_UNROLL = {K['BACK_UNROLL']}")
    assert all(k % K["BACK_UNROLL"] == 0 for k in (ref.TOGETHER_K[0], ref.MERGED_K[1])) and all(k % K["BACK_UNROLL"] for k in (ref.TOGETHER_K[1], ref.MERGED_K[0]))


def test_both_long_has_long_windows_on_both_axes_of_one_pixel():
    (h, w), (oh, ow) = ref.back_extent("both_long")
    xs_h, xs_w = ref.windows("cubic", h, oh)[2], ref.windows("cubic", w, ow)[2]
    assert (int(xs_h.max()), int(xs_w.max())) == (90, 110), resize("both_long", "cubic windows of 90 x 110 taps")
    for filt in ref.FILTERS:  # (every pixel of an output has its row's H window and its column's W window)
        assert min(int(ref.windows(filt, h, oh)[2].max()), int(ref.windows(filt, w, ow)[2].max())) > 32, (filt, resize("both_long", "long windows on both axes"))
    assert ref.MERGED_SHAPES[1] == (h, w) and ref.MERGED_SIZES[1] == (oh, ow)


def test_many_rows_and_the_embed_grids_exceed_the_table_kernels_lanes():
    (h, w), (oh, ow) = ref.back_extent("many_rows")
    assert oh > 2 * K["BACK_THREADS"] and h > 1, resize("many_rows", f"three rounds of the table loop of AA_BACK_THREADS = {K['BACK_THREADS']} lanes, a real source")
    assert ref.BACK_CASES["wide_out"][3][1] > 2 * K["BACK_THREADS"]
    t = K["EMBED_THREADS"]
    sides = {name: [s for g in grids for s in g] for name, (_, grids) in ref.EMBED_CASES.items()}
    assert 300 in sides["shrink_40x48"] and 300 > t, resize("shrink_40x48", f"more forward rows than AA_EMBED_THREADS = {t}")
    assert 520 in sides["shrink_40x48"] and 520 > 2 * t, resize("shrink_40x48", "three rounds of the forward rows' loop")
    assert 900 in sides["wide_source"] and 900 > 3 * t, resize("wide_source", "four rounds of the forward rows' loop")
    assert ref.EMBED_CASES["wide_source"][0][1] > t, resize("wide_source", f"more source positions than AA_EMBED_THREADS = {t}: the adjoint loop's second round")
    assert max(sides["source_1x1_long"]) > 2 * t
    assert ref.EMBED_D[0] % K["EMBED_VEC"] != 0 and ref.EMBED_D[1] % K["EMBED_VEC"] == 0, "D = 5 takes scalar lanes and D = 8 vector lanes"
    # the identity grids
    for name in ("shrink_40x48", "wide_source"):
        assert ref.EMBED_CASES[name][0] in ref.EMBED_CASES[name][1], name


def test_embed_windows_and_adjoint_rows():
    (h0, w0), grids = ref.EMBED_CASES["shrink_40x48"]
    assert (int(ref.windows("cubic", h0, 2)[2].max()), int(ref.windows("cubic", w0, 3)[2].max())) == (40, 48), resize("shrink_40x48", "forward windows of 40 x 48 taps")
    assert max(ref.adjoint_row_lengths("cubic", h0, 300)) == 30 and max(ref.adjoint_row_lengths("cubic", w0, 520)) == 44, resize("shrink_40x48", "adjoint rows of 30 and 44 taps")
    (h0, w0), grids = ref.EMBED_CASES["wide_source"]
    assert int(ref.windows("cubic", w0, 7)[2].max()) == 172, resize("wide_source", "forward rows of 172 taps")
    assert int(ref.windows("cubic", w0, 7)[2].max()) >= ref.LONG_TAPS
    for filt in ref.ORACLE_FILTERS:
        for (gh, gw) in ref.EMBED_CASES["source_1x1_long"][1]:
            assert ref.adjoint_row_lengths(filt, 1, gh) == [gh] and ref.adjoint_row_lengths(filt, 1, gw) == [gw], resize("source_1x1_long", "one adjoint row as long as the grid side")
    for name, (hw, grids) in ref.EMBED_CASES.items():
        for filt in ref.FILTERS:
            assert all(ref.windows(filt, hw[ax], g[ax])[0] <= AA_MAX_KSIZE for g in grids for ax in (0, 1)), (name, filt)


def test_backward_cases():
    canvas, regions, sizes = ref.tall_adjoint_case()
    assert canvas == (3, 2) and regions == [(1, 1, 1, 1)] and sizes == [(300, 4)]
    for filt in ref.ORACLE_FILTERS:
        assert ref.adjoint_row_lengths(filt, 1, 300) == [300], resize("tall_adjoint_case", "one adjoint row of 300 taps along H")
    assert 300 >= ref.LONG_TAPS and 300 > K["BACK_BWD_THREADS"]
    # the existing cases the new dtypes and layout run on: table loops of several rounds both ways, several column units
    canvas, regions, sizes = bwd_ref.seams_case()
    assert sizes[0][1] > 2 * K["BACK_BWD_THREADS"] and regions[0][3] > 2 * K["BACK_BWD_THREADS"], resize("seams_case", "several rounds of both table loops")
    assert canvas[1] > 2 * K["BACK_BWD_COLS"] and regions[0][1] % K["BACK_BWD_COLS"] != 0, resize("seams_case", "several column units")
    canvas, regions, sizes = bwd_ref.long_rows_case()
    assert int(ref.windows("box", regions[0][3], sizes[0][1])[2].max()) >= 100


# ---- the planner accepts every case and counts the units the tile implies ----------------------------------------------------------------
def _plan(names, k, filt, layout):
    L = _lib.load()
    n = len(names)
    nbytes = L.aa_back_many_desc_bytes(n)
    buf = (ctypes.c_uint8 * nbytes)()
    recs = (_lib.BackItemIn * n)()
    for r, name in zip(recs, names):
        (h, w), (oh, ow) = ref.back_extent(name)
        hh, ww = ref.BACK_CASES[name][1]
        strides = (1, ww * k, k) if layout == _lib.NHWC else (hh * ww, ww, 1)
        r.data_dev, r.stride_ch, r.stride_row, r.stride_px, r.h, r.w, r.oh, r.ow, r.flags = (4096,) + strides + (h, w, oh, ow, 0)
    ws, arena = ctypes.c_size_t(0), ctypes.c_size_t(0)
    offs = (ctypes.c_int64 * n)()
    rc = L.aa_back_many_plan(FILTER_IDS[filt], layout, n, k, recs, _lib.BACK_VALUES, _lib.F32, ctypes.addressof(buf), nbytes, ctypes.byref(ws),
                             ctypes.byref(arena), offs)
    return rc, buf


@pytest.mark.parametrize("filt", ref.FILTERS)
def test_the_planner_accepts_every_case_and_counts_the_units(filt):
    tile = K["BACK_TILE"]
    for layout in (_lib.NCHW, _lib.NHWC):
        rc, buf = _plan(ref.BACK_NAMES, 5, filt, layout)
        assert rc == 0, (filt, _lib.strerror(rc))  # (AA_ERR_KSIZE would refuse a case before the GPU ever saw it)
        hd, recs, prefix = _lib.back_desc_view(buf, len(ref.BACK_NAMES))
        units = [oh * -(-ow // tile) for _, _, _, (oh, ow) in ref.BACK_CASES.values()]
        assert list(prefix) == [sum(units[:i]) for i in range(len(units) + 1)] and hd.units == sum(units), \
            f"the built library's work units are not oh * ceil(ow / {tile}), the AA_BACK_TILE of the header's text: {list(prefix)}"
        for name, r in zip(ref.BACK_NAMES, recs):
            (h, w), (oh, ow) = ref.back_extent(name)
            assert (r.ksize_h, r.ksize_w, r.xtiles) == (ref.windows(filt, h, oh)[0], ref.windows(filt, w, ow)[0], -(-ow // tile)), (name, filt)
    assert units[ref.BACK_NAMES.index("many_rows")] == 700 and units[ref.BACK_NAMES.index("wide_out")] == 12


# ---- the float64 check's reference -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", ref.ORACLE_FILTERS)
def test_the_oracle_lies_within_the_dense_bound(filt):
    worst = {}
    for k in (None,) + ref.TOGETHER_K:
        for names in ([(n,) for n in ref.BACK_NAMES] if k is None else [ref.BACK_NAMES]):
            srcs, regions, sizes = ref.back_list(names, k)
            flips = ref.TOGETHER_FLIPS if k is not None else [True]
            got = back_ref.values(filt, srcs, regions, sizes, flips)
            want, bnd = back_ref.dense_values(filt, srcs, regions, sizes, flips)
            for n, g, w, b in zip(names, got, want, bnd):
                worst[n] = max(worst.get(n, 0.0), backward_ref.worst_ratio(g, w, b))
    print(f"{filt}: the oracle's worst err / bound per case: " + ", ".join(f"{n} {r:.3f}" for n, r in worst.items()))
    assert max(worst.values()) <= 1.0, worst


# ---- the references are sensitive --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", ref.ORACLE_FILTERS)
def test_the_references_notice_a_dropped_flip_and_a_tile_with_another_tiles_windows(filt):
    tile = K["BACK_TILE"]
    srcs, regions, sizes = ref.back_list(("wide_out",))
    assert sizes[0][1] > 2 * tile, resize("wide_out", f"a whole second column tile of AA_BACK_TILE = {tile}")
    flipped = back_ref.values(filt, srcs, regions, sizes, [True])[0]
    plain = back_ref.values(filt, srcs, regions, sizes, [False])[0]
    assert np.array_equal(flipped, plain[:, :, ::-1]) and (flipped.view(np.int32) != plain.view(np.int32)).mean() > 0.9
    # tile 1 computed with tile 0's windows: the columns of tile 1 become those of tile 0
    wrong = np.array(plain)
    wrong[:, :, tile:2 * tile] = plain[:, :, :tile]
    differ = wrong.view(np.int32) != plain.view(np.int32)
    assert differ[:, :, tile:2 * tile].mean() > 0.9 and not differ[:, :, :tile].any() and not differ[:, :, 2 * tile:].any()
    # ... and the float64 check notices both
    want, bnd = back_ref.dense_values(filt, srcs, regions, sizes, [False])
    assert back_ref.worst_ratio([plain], want, bnd) <= 1.0
    assert back_ref.worst_ratio([flipped], want, bnd) > 1.0 and back_ref.worst_ratio([wrong], want, bnd) > 1.0
    # the same with the dense matrix itself: rows of tile 1 replaced by those of tile 0
    (h, w), (oh, ow) = ref.back_extent("wide_out")
    a_h, a_w = backward_ref.dense(filt, h, oh), backward_ref.dense(filt, w, ow)
    a_bad = np.array(a_w)
    a_bad[tile:2 * tile] = a_w[:tile]
    bad = np.einsum("oy,kyx,px->kop", a_h, srcs[0].astype(np.float64), a_bad)
    assert back_ref.worst_ratio([bad], want, bnd) > 1.0
    # the merged sums notice a member read unmirrored beyond the first tile
    k = ref.MERGED_K[0]
    members = ref.merged_ref.member_values(filt, list(ref.merged_sources(k)), None, ref.MERGED_GROUPS, ref.MERGED_SIZES, ref.MERGED_FLIPS)
    unmirrored = [np.array(m) for m in members]
    unmirrored[0][:, :, tile:] = members[0][:, :, ::-1][:, :, tile:]
    good = ref.merged_ref.merge_members(members, ref.MERGED_GROUPS, 2)
    bad = ref.merged_ref.merge_members(unmirrored, ref.MERGED_GROUPS, 2)
    assert np.array_equal(good[0], ref.merged_values(filt, k, "sum")[0])
    assert not np.array_equal(good[0][:, :, tile:], bad[0][:, :, tile:]) and np.array_equal(good[0][:, :, :tile], bad[0][:, :, :tile])
