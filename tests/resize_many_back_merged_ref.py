"""The definition of resize_many_back_merged restated on the CPU, shared by test_resize_many_back_merged_cpu.py,
test_resize_many_back_merged_gpu.py and test_resize_many_back_merged_guard_gpu.py.  Plain numpy; not a test module.

  * merged_values: per member resize_many_back_ref.values (the oracle's fp32 arithmetic, three filters) at its GROUP's size, mirrored
    where the member flips; then per group the members in ascending item index added one by one in numpy.float32 (one round-to-nearest
    add per element and step), and for the mean one numpy.float32 division by float32(M);
  * labels and masks of those sums are resize_many_back_ref's.
"""
from __future__ import annotations

import numpy as np

import kit_golden
import resize_many_back_ref as back_ref

ORACLE_FILTERS = back_ref.ORACLE_FILTERS
FILTERS = back_ref.FILTERS

# ---- the base case ----------------------------------------------------------------------------------------------------------------------
# group 0 mixes a whole, a cropped and a one-pixel source; group 1 crosses the 256-column tile with a one-pixel and a one-column source;
# group 2 mixes the identity with an antialiased shrink; every group mixes flipped and unflipped members; the groups interleave.
BASE_CANVAS = kit_golden.readonly(np.random.default_rng(17).standard_normal((7, 7, 12, 16)).astype(np.float32))
BASE_GROUPS = [0, 1, 0, 2, 1, 0, 2]
BASE_SIZES = [(23, 31), (4, 300), (5, 7)]
BASE_REGIONS = [(0, 0, 12, 16), (3, 0, 1, 1), (1, 2, 6, 9), (2, 3, 5, 7), (0, 5, 12, 1), (3, 0, 1, 1), (0, 0, 12, 16)]
BASE_FLIPS = [True, False, False, True, True, False, False]
INF_AT = (5, 3, 0)  # class, canvas row, canvas column of the +inf (item 0) and the -inf (item 5) of nonfinite_canvas: group 0


def members(groups, g: int):
    """The item indices of group g, ascending."""
    return [i for i, v in enumerate(groups) if v == g]


def tie_canvas() -> np.ndarray:
    """The base canvas with plane 4 a copy of plane 2 in every member: the sums of classes 2 and 4 are the same bits, and class 4 never
    wins under the lowest-index rule."""
    c = np.array(BASE_CANVAS)
    c[:, 4] = c[:, 2]
    return kit_golden.readonly(c)


def nonfinite_canvas() -> np.ndarray:
    """The base canvas with one NaN in a single member (item 2's region, class 3), and +inf in item 0 and -inf in item 5 — two members of
    group 0 — at the same canvas pixel and class: item 5 is that one pixel, so its class 5 is -inf everywhere, and the sum is NaN where
    item 0's is +inf."""
    c = np.array(BASE_CANVAS)
    c[2, 3, 4, 6] = np.nan
    k, y, x = INF_AT
    c[0, k, y, x] = np.inf
    c[5, k, y, x] = -np.inf
    return kit_golden.readonly(c)


CANVASES = {"base": lambda: BASE_CANVAS, "tie": tie_canvas, "nonfinite": nonfinite_canvas}


def k_canvas(k: int) -> np.ndarray:
    return kit_golden.readonly(np.random.default_rng(170 + k).standard_normal((7, k, 12, 16)).astype(np.float32))


def k300_case():
    """K = 300, two members of one group, 3 x 3 sources to (5, 4), plane 299 raised by 10 at one source pixel of each: labels above 255."""
    c = np.random.default_rng(301).standard_normal((2, 300, 3, 3)).astype(np.float32)
    c[:, 299, 1, 2] += 10.0
    return kit_golden.readonly(c), [(0, 0, 3, 3)] * 2, [0, 0], [(5, 4)]


def seventy_case():
    """70 groups of 1 to 3 members (139 items), sources of at most 3 x 3 to at most 4 x 4, the members scattered over the item order: the
    unit search passes 64 groups.  -> (canvas, regions, groups, sizes, flips)"""
    groups = [g for g in range(70) for _ in range(1 + g % 3)]
    groups = [groups[j] for j in np.random.default_rng(71).permutation(len(groups))]
    n = len(groups)
    c = kit_golden.readonly(np.random.default_rng(70).standard_normal((n, 3, 3, 3)).astype(np.float32))
    regions = [(i % 2, (i // 2) % 2, 1 + (i // 4) % 2 + (1 - i % 2), 1 + (i // 8) % 2 + (1 - (i // 2) % 2)) for i in range(n)]
    sizes = [(1 + g % 4, 1 + (g // 4) % 4) for g in range(70)]
    return c, regions, groups, sizes, [i % 3 == 1 for i in range(n)]


def list_case():
    """Separately allocated items of different (H_i, W_i), K = 3, merged into 2 groups: multi-scale passes.
    -> (sources, regions, groups, sizes, flips)"""
    rng = np.random.default_rng(12)
    shapes = [(4, 9), (7, 3), (1, 5), (6, 6), (8, 12)]
    srcs = [kit_golden.readonly(rng.standard_normal((3, h, w)).astype(np.float32)) for h, w in shapes]
    return srcs, [None, (1, 0, 5, 3), None, (2, 1, 3, 4), None], [0, 1, 0, 1, 0], [(9, 17), (3, 4)], [True, False, False, True, False]


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
def member_values(filt: str, srcs, regions, groups, sizes, flips=None):
    """-> [float32 [K, oh_g, ow_g]] per ITEM: R_i, every member at its group's size."""
    return back_ref.values(filt, srcs, regions, [sizes[g] for g in groups], flips)


def merge_members(vals, groups, n_groups: int, merge: str = "sum", descending: bool = False):
    """Per group the members' values added in ascending (or, for the test of the test, descending) item index, float32 at every step; the
    mean divides by float32(M)."""
    assert merge in ("sum", "mean")
    out = []
    with np.errstate(invalid="ignore"):
        for g in range(n_groups):
            idx = members(groups, g)
            if descending:
                idx = idx[::-1]
            s = np.array(vals[idx[0]], dtype=np.float32)
            for i in idx[1:]:
                s = (s + vals[i]).astype(np.float32)
            if merge == "mean":
                s = (s / np.float32(len(idx))).astype(np.float32)
            assert s.dtype == np.float32
            out.append(s)
    return out


def merged_values(filt: str, srcs, regions, groups, sizes, flips=None, merge: str = "sum"):
    """-> [float32 [K, oh_g, ow_g]] per GROUP: S_g of the definition."""
    return merge_members(member_values(filt, srcs, regions, groups, sizes, flips), groups, len(sizes), merge)


labels = back_ref.labels
masks = back_ref.masks
