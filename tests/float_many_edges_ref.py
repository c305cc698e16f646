"""Shared by the float ragged calls' edge tests (test_float_many_edges_cpu.py, test_float_many_edges_gpu.py): the cases that reach the
seams of resize_many_back, resize_many_back_merged, resize_embed_to_tokens (both ways) and resize_many_back_backward — output rows of
several column tiles, windows of hundreds of taps on either axis, tables of more rows than the table kernel has lanes — their inputs,
regenerated from their seeds once and left unchanged, the tile sizes of the kernels read out of their headers' text, and the windows a
case has, from oracle.weights and backward_ref's tables.  The expected values are the existing restatements' (resize_many_back_ref,
resize_many_back_merged_ref, resize_embed_ref); nothing here calls the code under test.  Not a test module."""
import functools
import os
import re

import numpy as np

import backward_ref
import kit_golden
import resize_many_back_bwd_ref as bwd_ref
import resize_many_back_merged_ref as merged_ref
import resize_many_back_ref as back_ref

CSRC = os.path.join(kit_golden.ROOT, "interpolate_antialiasing_amd", "csrc")
ORACLE_FILTERS = back_ref.ORACLE_FILTERS
FILTERS = back_ref.FILTERS
LONG_TAPS = 128  # what "a long window" means here: two waves' lanes; the other float ragged tests' longest row has about 15 taps


# ---- the tile sizes, from the headers' text ----------------------------------------------------------------------------------------------
_DEFINES = {"aa_many_back.h": ("AA_BACK_THREADS", "AA_BACK_TILE", "AA_BACK_UNROLL"), "aa_embed_many.h": ("AA_EMBED_THREADS", "AA_EMBED_VEC"),
            "aa_many_back_bwd.h": ("AA_BACK_BWD_THREADS", "AA_BACK_BWD_COLS")}


@functools.lru_cache(maxsize=None)
def constants():
    """The #defines of _DEFINES by regular expressions on the headers' text -> {name without the AA_ prefix: value}."""
    out = {}
    for header, names in _DEFINES.items():
        with open(os.path.join(CSRC, header)) as f:
            text = f.read()
        for name in names:
            pattern = rf"#define\s+{name}\s+(\d+)\b"
            m = re.search(pattern, text)
            assert m, f"{name} of csrc/{header} is no longer written as this helper reads it: {pattern}"
            out[name[3:]] = int(m.group(1))
    return out


# ---- resize_many_back: one item a case ---------------------------------------------------------------------------------------------------
# name -> (K, the item's (H, W), the region (y0, x0, h, w) or None, (oh, ow)).  An item with a region is NaN outside it.
BACK_CASES = {
    "wide_out": (5, (3, 150), None, (4, 601)),                     # three column tiles, the last of 89 lanes, real windows in each
    "tile_256": (3, (2, 64), None, (2, 256)),                      # exactly one tile
    "tile_257": (3, (2, 64), None, (2, 257)),                      # a second tile of one live lane
    "wide_src_shrink": (2, (4, 610), (1, 7, 2, 600), (5, 3)),      # W windows of hundreds of taps, a pitched source wider than a tile
    "tall_shrink": (4, (300, 5), None, (2, 7)),                    # H windows of hundreds of taps, K = the unroll
    "both_long": (3, (90, 110), None, (2, 3)),                     # long windows on both axes of the same pixel
    "many_rows": (1, (40, 3), None, (700, 2)),                     # 700 table rows and 700 work units
}
BACK_NAMES = tuple(BACK_CASES)
BACK_16BIT = ("wide_out", "wide_src_shrink", "tall_shrink")
BACK_REDUCED = ("wide_out", "both_long")
TOGETHER_K = (4, 5)                                                # one list of all cases needs one K: the unroll, and a tail
TOGETHER_FLIPS = [True, False, True, True, False, True, False]
# the axes (0 = H, 1 = W) on which a case's longest window has LONG_TAPS taps and more under every oracle filter
LONG_AXES = {"wide_src_shrink": (1,), "tall_shrink": (0,)}
THRESHOLD = 0.125


@functools.lru_cache(maxsize=None)
def back_source(name, k=None):
    """The case's [K, H, W] float32 item (read-only): normal values, NaN outside the region."""
    k0, (hh, ww), region, _ = BACK_CASES[name]
    k = k0 if k is None else k
    rng = np.random.default_rng([1, BACK_NAMES.index(name), k])
    if region is None:
        return kit_golden.readonly(rng.standard_normal((k, hh, ww)).astype(np.float32))
    y0, x0, h, w = region
    c = np.full((k, hh, ww), np.nan, np.float32)
    c[:, y0:y0 + h, x0:x0 + w] = rng.standard_normal((k, h, w)).astype(np.float32)
    return kit_golden.readonly(c)


def back_list(names=BACK_NAMES, k=None):
    """-> (sources, regions, sizes) of the named cases as one list; k: None (each case's own K, for a list of one) or the K of all."""
    return [back_source(n, k) for n in names], [BACK_CASES[n][2] for n in names], [BACK_CASES[n][3] for n in names]


def back_extent(name):
    """-> ((h, w) of the region resampled, (oh, ow))."""
    _, hw, region, size = BACK_CASES[name]
    return (tuple(region[2:]) if region is not None else hw), size


def windows(filt, n_in, n_out):
    """-> (ksize, xmin, xsize) of the float32 forward table, for any of the five filters."""
    k, xmin, xsize, _ = backward_ref.axis_table(filt, n_in, n_out, False, np.float32)
    return int(k), np.asarray(xmin, np.int64), np.asarray(xsize, np.int64)


def adjoint_row_lengths(filt, n_in, n_out):
    """The taps of every adjoint row of the table n_in -> n_out, as the table kernels transpose it (the oracle's three filters)."""
    return [len(ws) for _, ws in bwd_ref.adjoint_rows(filt, n_in, n_out)]


def where_back(name_or_ow, flipped=False):
    """explain() of kit_gpu.assert_bits for a [K, oh, ow] or [oh, ow] output: the column tile and lane that stored the element."""
    ow = BACK_CASES[name_or_ow][3][1] if isinstance(name_or_ow, str) else name_or_ow
    tile = constants()["BACK_TILE"]

    def explain(at):
        x = ow - 1 - at[-1] if flipped else at[-1]
        return f"row {at[-2]}, column {at[-1]}: the lane of column {x} = tile {x // tile}, lane {x % tile}"

    return explain


# ---- resize_many_back_merged -------------------------------------------------------------------------------------------------------------
# group 0 (4, 601): mirrored reads across three tiles with real windows, next to an unflipped member and a one-pixel one; group 1
# (2, 3): long windows on both axes next to a flipped 600-column shrink.  The groups interleave in item order.
MERGED_SHAPES = [(3, 150), (90, 110), (2, 75), (2, 600), (1, 1)]
MERGED_GROUPS = [0, 1, 0, 1, 0]
MERGED_FLIPS = [True, False, False, True, True]
MERGED_SIZES = [(4, 601), (2, 3)]
MERGED_K = (5, 8)


@functools.lru_cache(maxsize=None)
def merged_sources(k):
    rng = np.random.default_rng([2, k])
    return tuple(kit_golden.readonly(rng.standard_normal((k, h, w)).astype(np.float32)) for h, w in MERGED_SHAPES)


@functools.lru_cache(maxsize=None)
def merged_values(filt, k, merge):
    """The restated sums of the merged case, per group (read-only)."""
    vals = merged_ref.merged_values(filt, list(merged_sources(k)), None, MERGED_GROUPS, MERGED_SIZES, MERGED_FLIPS, merge)
    return tuple(kit_golden.readonly(v) for v in vals)


# ---- resize_embed_to_tokens --------------------------------------------------------------------------------------------------------------
# name -> ((H0, W0), grids)
EMBED_CASES = {
    "shrink_40x48": ((40, 48), [(2, 3), (300, 2), (1, 520), (40, 48)]),
    "wide_source": ((2, 300), [(1, 7), (3, 900), (2, 300)]),
    "source_1x1_long": ((1, 1), [(1, 600), (300, 1)]),
}
EMBED_D = (5, 8)  # scalar lanes, vector lanes

# ---- resize_many_back_backward -----------------------------------------------------------------------------------------------------------


def tall_adjoint_case():
    """A 1 x 1 region on a (3, 2) canvas under a (300, 4) gradient: one adjoint row of 300 taps along H.  -> (canvas, regions, sizes)"""
    return (3, 2), [(1, 1, 1, 1)], [(300, 4)]
