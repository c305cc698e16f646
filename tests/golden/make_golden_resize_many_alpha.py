"""Fixture for resize_many(alpha=True) (Pillow's RGBA / LA resize for a list of images): tests/golden/resize_many_alpha.npz.

Run by hand (needs Pillow; no GPU):  python tests/golden/make_golden_resize_many_alpha.py

The packing of resize_many_placed.npz, per ITEM: for every case of CASES below, every filter of the case and every item, the CRC-32 of the
item's input, the CRC-32 of the expected [oH, oW, C] canvas and up to 256 sampled pixels of it.  The expected canvas is Pillow's own
``Image.frombytes("RGBA" | "LA", ...).resize((vw, vh), FILTER, box=...)`` pasted by numpy slicing at (py, px) into a canvas of the fill
colour; the fill is straight values and is never converted.  Inputs are make_golden_alpha.make_image's: large fully transparent and fully
opaque areas, a band of random alpha and hard colour edges, so that resampled premultiplied colour overshoots alpha under bicubic /
Lanczos and meets the ``c >= a -> 255`` clamp.

restated() is numpy only: Image.resize's copy rule, make_golden_alpha's premul_formula, the single-item restatement of the resize with a
box (make_golden_box_reduce.resize_box_restated) and unpremul_formula.  main() asserts that it reproduces Pillow bit for bit on every
entry, so the tests may use it where Pillow is missing.
"""
from __future__ import annotations

import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "resize_many_alpha.npz")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_rm = _load("make_golden_resize_many")
_al = _load("make_golden_alpha")
crc, sample_pixels, pack, FILTER_NAMES = _rm.crc, _rm.sample_pixels, _rm.pack, _rm.FILTER_NAMES
resize_box_restated = _rm.resize_box_restated
premul_formula, unpremul_formula, make_image = _al.premul_formula, _al.unpremul_formula, _al.make_image

# items: (H, W, box (x0, y0, x1, y1) or None, (vh, vw), (py, px))
_PLAIN = [(50, 163, None, (19, 37), (0, 0)), (25, 90, (3.5, 1.25, 80.0, 22.5), (19, 37), (0, 0)), (64, 40, None, (19, 37), (0, 0)),
          (9, 14, (0.5, 1.25, 13.0, 8.5), (19, 37), (0, 0))]  # shrinking, a sub-pixel box, width shrinks / height too, both grow
# Pillow's copy: the canvas's size with no box; with the whole image as a float box; NOT a copy: a real sub-box, another size
_COPY = [(19, 37, None, (19, 37), (0, 0)), (19, 37, (0.0, 0.0, 37.0, 19.0), (19, 37), (0, 0)), (19, 37, (2.5, 1.0, 30.0, 17.5), (19, 37), (0, 0)),
         (40, 50, None, (19, 37), (0, 0))]
# placed copies: sizes[i] == (H_i, W_i), inside the canvas and overhanging it; the same image at another size is none
_COPY_PLACED = [(12, 17, None, (12, 17), (5, 7)), (12, 17, (0.0, 0.0, 17.0, 12.0), (12, 17), (-3, 33)), (12, 17, None, (20, 25), (3, -4)),
                (12, 17, (1.0, 0.0, 17.0, 12.0), (12, 17), (17, 20))]
# overhangs every edge; inside at an odd px (LA: lead 2, one dword holds a fill pixel and an item pixel); wholly off the canvas; the plain
# placement
_PLACED = [(97, 131, None, (40, 60), (-5, -8)), (33, 60, (10.5, 2.25, 50.0, 30.5), (12, 21), (9, 7)), (12, 17, None, (6, 6), (100, 3)),
           (50, 60, None, (30, 45), (0, 0))]

# (name, C, canvas (oh, ow), fill per channel, filters, items, seed, placed call?)
CASES = [
    ("a_rgba", 4, (19, 37), (0, 0, 0, 0), FILTER_NAMES, _PLAIN, 81, False),
    ("a_la", 2, (19, 37), (0, 0), FILTER_NAMES, _PLAIN, 82, False),
    ("a_copy4", 4, (19, 37), (0, 0, 0, 0), ("cubic", "box"), _COPY, 83, False),
    ("a_copy2", 2, (19, 37), (0, 0), ("cubic", "box"), _COPY, 84, False),
    ("a_copyp4", 4, (30, 45), (9, 250, 77, 100), ("cubic", "box"), _COPY_PLACED, 85, True),
    ("a_copyp2", 2, (30, 45), (9, 100), ("cubic", "box"), _COPY_PLACED, 86, True),
    ("a_placed4", 4, (30, 45), (200, 13, 99, 77), ("linear", "cubic", "lanczos"), _PLACED, 87, True),
    ("a_placed2", 2, (30, 45), (200, 77), ("linear", "cubic", "lanczos"), _PLACED, 88, True),
]


def case(name: str):
    return next(cs for cs in CASES if cs[0] == name)


def item_input(cs, i: int) -> np.ndarray:
    """[C, H, W] uint8 input of item i of a case, straight alpha in the last channel."""
    h, w = cs[5][i][:2]
    return np.ascontiguousarray(make_image(h, w, cs[1], 100 * cs[6] + i).transpose(2, 0, 1))


def entries():
    """Every (key, case, filter, item index) of the fixture, in the order its arrays are packed."""
    for cs in CASES:
        for f in cs[4]:
            for i in range(len(cs[5])):
                yield f"{cs[0]}/{f}/{i}", cs, f, i


def is_copy(h: int, w: int, vh: int, vw: int, box) -> bool:
    """Image.resize's first return: the size asked for is the image's and the box is None or the whole image by value."""
    return (vh, vw) == (h, w) and (box is None or tuple(box) == (0, 0, w, h))


def resize_alpha_restated(f: str, img: np.ndarray, vh: int, vw: int, box=None, alpha: bool = True) -> np.ndarray:
    """[H, W, C] straight -> Image.resize((vw, vh), FILTER, box) of the "RGBA" / "LA" image (alpha False: of its plain channels)."""
    h, w = img.shape[:2]
    if is_copy(h, w, vh, vw, box):
        return img.copy()
    if not alpha:
        return resize_box_restated(f, img, vh, vw, box)
    pm = img.copy()
    pm[..., :-1] = premul_formula(img[..., :-1], img[..., -1:])
    r = resize_box_restated(f, pm, vh, vw, box)
    out = r.copy()
    out[..., :-1] = unpremul_formula(r[..., :-1], r[..., -1:])
    return out


def paste(canvas_size, fill, r: np.ndarray, py: int, px: int) -> np.ndarray:
    """The [vh, vw, C] resize r at (py, px) of a fill-coloured [oH, oW, C] canvas."""
    oh, ow = canvas_size
    vh, vw, c = r.shape
    canvas = np.empty((oh, ow, c), np.uint8)
    canvas[:] = np.array(fill, np.uint8)
    y0, y1, x0, x1 = max(0, py), min(oh, py + vh), max(0, px), min(ow, px + vw)
    if y1 > y0 and x1 > x0:
        canvas[y0:y1, x0:x1] = r[y0 - py:y1 - py, x0 - px:x1 - px]
    return canvas


def restated(cs, f: str, i: int, x: np.ndarray, alpha: bool = True) -> np.ndarray:
    """[C, H, W] -> the expected [oH, oW, C] canvas of one item from the restatement (alpha False: the call without alpha)."""
    _, _, box, (vh, vw), (py, px) = cs[5][i]
    return paste(cs[2], cs[3], resize_alpha_restated(f, np.ascontiguousarray(x.transpose(1, 2, 0)), vh, vw, box, alpha), py, px)


def pillow(cs, f: str, i: int, x: np.ndarray) -> np.ndarray:
    """The same canvas from Pillow itself."""
    from PIL import Image

    flt = {"linear": Image.BILINEAR, "cubic": Image.BICUBIC, "box": Image.BOX, "hamming": Image.HAMMING, "lanczos": Image.LANCZOS}
    h, w, box, (vh, vw), (py, px) = cs[5][i]
    c = cs[1]
    img = np.ascontiguousarray(x.transpose(1, 2, 0))
    r = Image.frombytes("RGBA" if c == 4 else "LA", (w, h), img.tobytes()).resize((vw, vh), flt[f], box=box)
    return paste(cs[2], cs[3], np.asarray(r).reshape(vh, vw, c), py, px)


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
        h, w, box, (vh, vw), _ = cs[5][i]
        if is_copy(h, w, vh, vw, box):  # the copy is the untouched input, and the premultiplied round trip would not be
            assert np.array_equal(resize_alpha_restated(f, x.transpose(1, 2, 0), vh, vw, box), x.transpose(1, 2, 0))
            pm = x.transpose(1, 2, 0).copy()
            pm[..., :-1] = unpremul_formula(premul_formula(pm[..., :-1], pm[..., -1:]), pm[..., -1:])
            assert not np.array_equal(pm, x.transpose(1, 2, 0)), f"{key}: the input does not tell a copy from a round trip"
        results.append((crc(x), pil))
    np.savez_compressed(OUT, **pack(results))
    print(OUT, os.path.getsize(OUT), "bytes,", len(results), "entries, Pillow", PIL.__version__)
    fx = np.load(OUT)
    for (key, _, _, _), (incrc, out) in zip(entries(), results):
        e = expected(fx, key)
        assert e[0] == incrc and e[1] == crc(out)


if __name__ == "__main__":
    main()
