"""Fixture for the placed resize_many (per-image sizes, cropped or padded into one batch): tests/golden/resize_many_placed.npz.

Run by hand (needs Pillow; no GPU):  python tests/golden/make_golden_resize_many_placed.py

The packing of resize_many.npz, per ITEM: for every case of CASES below, every filter of the case and every item, the CRC-32 of the item's
input, the CRC-32 of the expected [oH, oW, C] canvas and up to 256 sampled pixels of it.  The expected canvas is Pillow's own
``Image.resize((vw, vh), FILTER, box=...)`` pasted by numpy slicing at (py, px) into a canvas of the fill colour.  item_input, crc,
sample_pixels and the numpy restatement of the resize come from make_golden_resize_many.py; main() asserts that the restatement, pasted
the same way, reproduces Pillow bit for bit on every entry, so the tests may use it where Pillow is missing.
"""
from __future__ import annotations

import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "resize_many_placed.npz")

_spec = importlib.util.spec_from_file_location("make_golden_resize_many", os.path.join(HERE, "make_golden_resize_many.py"))
_rm = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_rm)
crc, sample_pixels, pack, FILTER_NAMES = _rm.crc, _rm.sample_pixels, _rm.pack, _rm.FILTER_NAMES

_C124 = [(50, 163, None, (25, 60), (-3, 9)), (25, 90, (3.5, 1.25, 80.0, 22.5), (10, 100), (4, -11)), (64, 40, None, (19, 77), (0, 0))]

# (name, C, canvas (oh, ow), fill per channel, filters, items [(H, W, box (x0, y0, x1, y1) or None, (vh, vw), (py, px))], seed,
#  one [N, C, H, W] tensor?)
CASES = [
    # Resize + CenterCrop: every item larger than the canvas on at least one axis, cropped on both sides
    ("p_eval", 3, (28, 28), (0, 0, 0), ("linear", "cubic"),
     [(97, 131, None, (32, 43), (-2, -8)), (61, 29, None, (67, 32), (-20, -2)), (33, 200, None, (32, 193), (-2, -82)), (40, 40, None, (28, 28), (0, 0))],
     71, False),
    # letterbox: padded on one axis; byte positions px * C that are no multiple of 4; axes of one element at the canvas's edges
    ("p_letterbox", 3, (48, 64), (114, 7, 201), ("linear", "lanczos"),
     [(97, 131, None, (47, 64), (0, 0)), (61, 29, None, (48, 23), (0, 21)), (12, 17, None, (44, 62), (2, 1)), (300, 1, None, (48, 1), (0, 63)),
      (1, 300, None, (1, 64), (47, 0))], 72, False),
    # item 0 is the plain call; crop and pad mixed per axis; a box; item 4 wholly off the canvas; item 5 one pixel in the last corner
    ("p_edges", 3, (30, 45), (9, 250, 77), FILTER_NAMES,
     [(97, 131, None, (30, 45), (0, 0)), (97, 131, None, (40, 60), (-5, -8)), (33, 200, (10.5, 2.25, 180.0, 30.5), (20, 70), (15, -50)),
      (61, 29, None, (25, 20), (-10, 30)), (12, 17, None, (6, 6), (100, 3)), (12, 17, None, (1, 1), (29, 44)), (50, 60, None, (3, 200), (13, -77))],
     73, False),
    # covered ranges that start on no 64-column strip of the canvas, more than one strip per item
    ("p_strips", 3, (4, 200), (0, 0, 0), ("hamming",),
     [(9, 517, None, (4, 130), (0, 37)), (8, 640, None, (4, 300), (0, -70)), (9, 517, None, (4, 65), (0, 135))], 74, False),
    # a hull of a few hundred columns of a 3000-column row; a window that crosses the 8 KiB staging chunk
    ("p_wide", 3, (7, 9), (5, 5, 5), ("linear", "lanczos"),
     [(40, 3000, None, (7, 90), (0, -40)), (40, 3000, None, (7, 12), (0, -2)), (2500, 33, None, (70, 9), (-30, 0))], 75, False),
    ("p_c1", 1, (19, 77), (200,), ("cubic", "box"), _C124, 76, False),
    ("p_c2", 2, (19, 77), (200, 13), ("cubic", "box"), _C124, 77, False),
    ("p_c4", 4, (19, 77), (200, 13, 99, 255), ("cubic", "box"), _C124, 78, False),
    # one [5, 3, 97, 131] tensor
    ("p_batch", 3, (30, 45), (0, 0, 0), ("linear",),
     [(97, 131, None, (30, 45), (0, 0)), (97, 131, None, (60, 90), (-15, -22)), (97, 131, None, (15, 20), (7, 12)),
      (97, 131, None, (97, 131), (-33, -43)), (97, 131, None, (31, 46), (-1, 0))], 79, True),
]


def case(name: str):
    return next(cs for cs in CASES if cs[0] == name)


def _plain_case(cs, i: int):
    """Item i's own resize as a case of make_golden_resize_many.py: the output is the item's (vh, vw)."""
    name, c, _, _, filters, items, seed, batch = cs
    return (name, c, items[i][3], [it[:3] for it in items], filters, seed, batch)


def item_input(cs, i: int) -> np.ndarray:
    """[C, H, W] uint8 input of item i of a case (a batch case: slice i of one [N, C, H, W] batch)."""
    return _rm.item_input(_plain_case(cs, i), i)


def entries():
    """Every (key, case, filter, item index) of the fixture, in the order its arrays are packed."""
    for cs in CASES:
        for f in cs[4]:
            for i in range(len(cs[5])):
                yield f"{cs[0]}/{f}/{i}", cs, f, i


def paste(cs, i: int, r: np.ndarray) -> np.ndarray:
    """The item's [vh, vw, C] resize r at its (py, px) of a fill-coloured [oH, oW, C] canvas."""
    oh, ow = cs[2]
    (vh, vw), (py, px) = cs[5][i][3], cs[5][i][4]
    assert r.shape == (vh, vw, cs[1])
    canvas = np.empty((oh, ow, cs[1]), np.uint8)
    canvas[:] = np.array(cs[3], np.uint8)
    y0, y1, x0, x1 = max(0, py), min(oh, py + vh), max(0, px), min(ow, px + vw)
    if y1 > y0 and x1 > x0:
        canvas[y0:y1, x0:x1] = r[y0 - py:y1 - py, x0 - px:x1 - px]
    return canvas


def restated(cs, f: str, i: int, x: np.ndarray) -> np.ndarray:
    """[C, H, W] -> the expected [oH, oW, C] canvas of one item, from the restatement of the full [vh, vw] resize."""
    return paste(cs, i, _rm.restated(_plain_case(cs, i), f, i, x))


def pillow(cs, f: str, i: int, x: np.ndarray) -> np.ndarray:
    """The same canvas from Pillow itself."""
    return paste(cs, i, _rm.pillow(_plain_case(cs, i), f, i, x))


def expected(fx, key: str):
    """-> (CRC-32 of the item's input, CRC-32 of the expected [oH, oW, C] canvas, its pixels at sample_pixels() [n, C])."""
    i = [e[0] for e in entries()].index(key)
    counts = fx["sample_counts"]
    off = int(counts[:i].sum())
    c = int(fx["channels"][i])
    return int(fx["crcs"][i, 0]), int(fx["crcs"][i, 1]), fx["samples"][off:off + int(counts[i])].reshape(-1, c)


def main() -> None:
    import PIL

    results = []
    for key, cs, f, i in entries():
        x = item_input(cs, i)
        pil = pillow(cs, f, i, x)
        mine = restated(cs, f, i, x)
        assert np.array_equal(mine, pil), f"the restatement differs from Pillow: {key}"
        results.append((crc(x), pil))
    np.savez_compressed(OUT, **pack(results))
    print(OUT, os.path.getsize(OUT), "bytes,", len(results), "entries, Pillow", PIL.__version__)
    fx = np.load(OUT)
    for (key, _, _, _), (incrc, out) in zip(entries(), results):
        e = expected(fx, key)
        assert e[0] == incrc and e[1] == crc(out)


if __name__ == "__main__":
    main()
