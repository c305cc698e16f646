"""Fixture for resize_many_nearest (Pillow's NEAREST for ragged label-map batches): tests/golden/resize_many_nearest.npz.

Run by hand (needs Pillow; no GPU):  python tests/golden/make_golden_resize_many_nearest.py

Pillow only: for every case of CASES below and every item, ``Image.resize((vw, vh), Image.NEAREST, box=...)``, ``paste`` at (px, py) onto
an ``Image.new`` canvas of the fill, and ``transpose(FLIP_LEFT_RIGHT)`` where the item flips.  The cases are a few KB each, so the
fixture holds every expected [N, oH, oW, C] batch whole, beside the CRC-32 of every item's input (inputs are regenerated from seeds).
int16 items are Pillow's "I;16" (the same bytes, read as unsigned there), int32 items its "I".

main() asserts, before it writes anything,
  * that the numpy restatement over boxmath.nearest_indices (tests/resize_many_nearest_ref.py) reproduces Pillow on every case;
  * that no index of the restatement lies outside its image on any case;
  * that on the cases marked as discriminators the OTHER index rule gives another table than Pillow's on every axis named there, and
    another image: a kernel with the wrong rule fails them on values.  (Pillow accumulates a double step for "L", "RGB", "RGBA", "I",
    and evaluates the closed form for "I;16".)
"""
from __future__ import annotations

import importlib.util
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "resize_many_nearest.npz")

DTYPES = {"u1": np.uint8, "i2": np.int16, "i4": np.int32}

_RAGGED = [(7, 9, None), (61, 83, None), (33, 20, (2.5, 1.25, 17.75, 30.5)), (40, 57, (3, 2, 50, 31)), (12, 17, (0.0, 0.0, 17.0, 12.0))]
_PLACED = [
    (20, 31, None, (30, 45), (0, 0)),                      # the plain call among placed ones
    (20, 31, None, (40, 60), (-5, 3)),                     # cropped above, padded on the left: dx * C = 9, no multiple of 4
    (33, 50, (10.5, 2.25, 45.0, 30.5), (20, 70), (15, -50)),  # padded above, cropped on the left and the right
    (12, 17, None, (6, 6), (100, 3)),                      # wholly off the canvas
    (12, 17, None, (1, 1), (29, 44)),                      # one pixel in the last corner
    (9, 14, None, (50, 11), (-13, 34)),                    # runs off the right edge
]

# name, dtype, C, canvas (oh, ow), fill per channel, items [(H, W, box (x0, y0, x1, y1) or None[, (vh, vw) or None, (py, px) or None])],
# flips or None, offsets "center"?, seed, one [N, C, H, W] tensor?, discriminating axes [(in, out, b0, b1)] or None
CASES = [
    # the smallest whole-image sizes at which accumulation and closed form differ, on each axis
    ("acc_whole", "u1", 1, (7, 15), (0,), [(2, 2, None)], None, False, 1, False, [(2, 7, None, None), (2, 15, None, None)]),
    ("acc_whole_t", "u1", 1, (15, 7), (0,), [(2, 2, None)], None, False, 2, False, [(2, 15, None, None), (2, 7, None, None)]),
    ("acc_whole_c3", "u1", 3, (7, 15), (0, 0, 0), [(2, 2, None), (2, 2, None)], [False, True], False, 3, False, [(2, 7, None, None), (2, 15, None, None)]),
    ("acc_box", "u1", 1, (23, 23), (0,), [(3, 3, (0.25, 1.5, 1.75, 2.5))], None, False, 4, False, None),  # 3 -> 23, a float box (main() takes its axes from the box)
    ("acc_i32", "i4", 1, (7, 15), (0,), [(2, 2, None)], None, False, 5, False, [(2, 7, None, None), (2, 15, None, None)]),
    ("closed_i16", "i2", 1, (7, 15), (0,), [(2, 2, None)], None, False, 6, False, [(2, 7, None, None), (2, 15, None, None)]),
    # plain: down- and upscaling, float and integer boxes, ragged sizes in one call
    ("plain_c1", "u1", 1, (13, 17), (0,), _RAGGED, None, False, 11, False, None),
    ("plain_c2", "u1", 2, (13, 17), (0, 0), _RAGGED, None, False, 12, False, None),
    ("plain_c3", "u1", 3, (13, 17), (0, 0, 0), _RAGGED, None, False, 13, False, None),
    ("plain_c4", "u1", 4, (13, 17), (0, 0, 0, 0), _RAGGED, None, False, 14, False, None),
    ("plain_flips", "u1", 3, (13, 18), (0, 0, 0), _RAGGED, [True, False, True, True, False], False, 15, False, None),
    ("batch", "u1", 3, (11, 41), (0, 0, 0), [(20, 30, None), (20, 30, (1.5, 0.5, 29.0, 19.25)), (20, 30, (4, 3, 24, 13))], None, False, 16, True, None),
    ("n1", "u1", 3, (9, 10), (0, 0, 0), [(31, 23, (0.5, 2.0, 22.5, 30.0))], [True], False, 17, False, None),
    # placed: crop and pad mixed per axis, an item off the canvas, a per-channel fill, mirrored fill
    ("placed_c3", "u1", 3, (30, 45), (9, 250, 77), _PLACED, [False, True, True, False, True, True], False, 21, False, None),
    ("placed_c1", "u1", 1, (30, 45), (255,), _PLACED, [True, False, False, True, False, True], False, 22, False, None),
    ("placed_c4", "u1", 4, (30, 45), (200, 13, 99, 255), _PLACED, None, False, 23, False, None),
    ("center", "u1", 1, (28, 28), (255,), [(50, 70, None, (32, 43), None), (40, 20, None, (67, 32), None), (9, 9, None, (20, 15), None),
                                           (30, 30, None, (28, 28), None)], [False, True, False, True], True, 24, False, None),
    # canvas widths 1 and 5; 15 bytes per interleaved row
    ("w1_c1", "u1", 1, (6, 1), (7,), [(9, 4, None, (6, 1), (0, 0)), (9, 4, None, (3, 2), (2, -1)), (5, 5, None, (4, 1), (3, 0))], [False, True, True], False, 31, False, None),
    ("w1_c3", "u1", 3, (6, 1), (7, 8, 9), [(9, 4, None, (6, 1), (0, 0)), (9, 4, None, (3, 2), (2, -1)), (5, 5, None, (4, 1), (3, 0))], None, False, 32, False, None),
    ("w5_c1", "u1", 1, (4, 5), (255,), [(9, 14, None, (4, 5), (0, 0)), (9, 14, None, (3, 3), (1, 1)), (9, 14, None, (6, 9), (-1, -2))], [True, True, False], False, 33, False, None),
    ("w5_c3", "u1", 3, (4, 5), (1, 2, 3), [(9, 14, None, (4, 5), (0, 0)), (9, 14, None, (3, 3), (1, 1)), (9, 14, None, (6, 9), (-1, -2))], [False, True, True], False, 34, False, None),
    # the gather's 1 KiB chunk seam: canvas rows of 1025 and 1026 bytes from tiny sources
    ("seam1025", "u1", 1, (2, 1025), (255,), [(3, 5, None, (2, 1025), (0, 0)), (3, 5, None, (2, 1030), (0, -3)), (2, 7, None, (1, 40), (1, 1004)),
                                              (2, 7, None, (2, 2), (0, 1023))], [False, True, True, False], False, 41, False, None),
    ("seam1026", "u1", 3, (2, 342), (1, 2, 3), [(3, 5, None, (2, 342), (0, 0)), (3, 5, None, (2, 350), (0, -5)), (2, 7, None, (1, 20), (1, 330)),
                                                (2, 7, None, (2, 2), (0, 340))], [True, False, False, True], False, 42, False, None),
    # the other dtypes: negative values, fill -1
    ("i16", "i2", 1, (13, 19), (-1,), [(7, 9, None, None, None), (33, 20, (2.5, 1.25, 17.75, 30.5), (20, 11), (-3, 5)), (12, 17, None, (5, 30), (9, -4))],
     [False, True, True], False, 51, False, None),
    ("i32", "i4", 1, (13, 19), (-1,), [(7, 9, None, None, None), (33, 20, (2.5, 1.25, 17.75, 30.5), (20, 11), (-3, 5)), (12, 17, None, (5, 30), (9, -4))],
     [True, False, True], False, 52, False, None),
    ("i16_seam", "i2", 1, (2, 513), (-1,), [(3, 5, None, (2, 513), (0, 0)), (3, 5, None, (2, 9), (0, 508))], [False, True], False, 53, False, None),
    ("i32_seam", "i4", 1, (2, 257), (-1,), [(3, 5, None, (2, 257), (0, 0)), (3, 5, None, (2, 9), (0, 252))], [True, False], False, 54, False, None),
]


def _boxmath():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from interpolate_antialiasing_amd import boxmath

    return boxmath


def case(name: str):
    return next(cs for cs in CASES if cs[0] == name)


def n_items(cs) -> int:
    return len(cs[5])


def closed_form(cs) -> bool:
    """Pillow's rule for the case's mode: the closed form for "I;16" (int16), the accumulation for every other."""
    return cs[1] == "i2"


def geometry(cs, i: int):
    """Item i -> (H, W, box or None, (vh, vw), (py, px)), sizes and offsets resolved (None: the canvas, (0, 0); a "center" case centred)."""
    it = tuple(cs[5][i]) + (None, None)
    h, w, box, size, off = it[:5]
    oh, ow = cs[3]
    vh, vw = size if size is not None else (oh, ow)
    if cs[7]:
        bm = _boxmath()
        off = (bm.center_offset(vh, oh), bm.center_offset(vw, ow))
    py, px = off if off is not None else (0, 0)
    return h, w, box, (vh, vw), (py, px)


def boxes(cs):
    return [geometry(cs, i)[2] for i in range(n_items(cs))]


def sizes(cs):
    return [geometry(cs, i)[3] for i in range(n_items(cs))]


def offsets(cs):
    return "center" if cs[7] else [geometry(cs, i)[4] for i in range(n_items(cs))]


def item_input(cs, i: int) -> np.ndarray:
    """[C, H, W] input of item i: seeded random class ids (tiny images: distinct values, so that every index shows)."""
    dt = DTYPES[cs[1]]
    c = cs[2]
    h, w = cs[5][i][0], cs[5][i][1]
    rng = np.random.default_rng([cs[8], i])
    lo, hi = {"u1": (0, 256), "i2": (-3000, 30000), "i4": (-100000, 2000000)}[cs[1]]
    if c * h * w <= 64:
        x = rng.permutation(np.arange(lo, hi, max(1, (hi - lo) // 200)))[:c * h * w]
    else:
        x = rng.integers(lo, hi, c * h * w)
    return x.reshape(c, h, w).astype(dt)


def crc(a: np.ndarray) -> int:
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def _to_pil(cs, x: np.ndarray):
    from PIL import Image

    c, h, w = x.shape
    if cs[1] == "i2":
        return Image.frombytes("I;16", (w, h), np.ascontiguousarray(x[0]).view(np.uint16).tobytes())
    if cs[1] == "i4":
        return Image.fromarray(np.ascontiguousarray(x[0]))  # "I"
    return Image.fromarray(x[0] if c == 1 else np.ascontiguousarray(x.transpose(1, 2, 0)))  # "L", "LA", "RGB", "RGBA"


def pillow(cs, xs) -> np.ndarray:
    """The expected [N, oH, oW, C] batch of a case from Pillow itself."""
    from PIL import Image

    oh, ow = cs[3]
    out = np.empty((n_items(cs), oh, ow, cs[2]), DTYPES[cs[1]])
    for i, x in enumerate(xs):
        _, _, box, (vh, vw), (py, px) = geometry(cs, i)
        im = _to_pil(cs, x)
        r = im.resize((vw, vh), Image.NEAREST, box=box)
        fill = tuple(int(v) for v in cs[4])
        if cs[1] == "i2":
            fill = (fill[0] & 0xFFFF,)
        canvas = Image.new(im.mode, (ow, oh), fill[0] if len(fill) == 1 else fill)
        canvas.paste(r, (px, py))
        if cs[6] is not None and cs[6][i]:
            canvas = canvas.transpose(Image.FLIP_LEFT_RIGHT)
        a = np.asarray(canvas)
        if cs[1] == "i2":
            a = a.view(np.int16)
        out[i] = a.reshape(oh, ow, cs[2])
    return out


def _ref():
    spec = importlib.util.spec_from_file_location("resize_many_nearest_ref", os.path.join(ROOT, "tests", "resize_many_nearest_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main() -> None:
    import PIL

    bm = _boxmath()
    ref = _ref()
    arrays = {}
    for cs in CASES:
        name = cs[0]
        xs = [item_input(cs, i) for i in range(n_items(cs))]
        pil = pillow(cs, xs)
        mine = ref.restate(cs, xs)
        assert np.array_equal(mine, pil), f"the restatement differs from Pillow: {name}"
        for i in range(n_items(cs)):  # no index of the restatement leaves its image
            h, w, box, (vh, vw), _ = geometry(cs, i)
            b = box if box is not None else (None, None, None, None)
            iy = bm.nearest_indices(h, vh, b[1], b[3], closed_form=closed_form(cs))
            ix = bm.nearest_indices(w, vw, b[0], b[2], closed_form=closed_form(cs))
            assert 0 <= min(iy) and max(iy) < h and 0 <= min(ix) and max(ix) < w, f"an index outside the image: {name} item {i}"
        if name == "acc_box":  # 3 -> 23 with a float box: both axes must tell the rules apart
            _, _, box, _, _ = geometry(cs, 0)
            disc = [(3, 23, box[1], box[3]), (3, 23, box[0], box[2])]
        else:
            disc = cs[10]
        if disc is not None:
            for in_size, out_size, b0, b1 in disc:
                assert bm.nearest_indices(in_size, out_size, b0, b1, closed_form=False) != bm.nearest_indices(in_size, out_size, b0, b1, closed_form=True), \
                    f"{name}: {in_size} -> {out_size} does not tell accumulation from the closed form"
            wrong = ref.restate(cs, xs, closed_form=not closed_form(cs))
            assert not np.array_equal(wrong, pil), f"{name}: the other index rule gives Pillow's image"
        arrays[name] = pil
        arrays[name + "__incrc"] = np.array([crc(x) for x in xs], np.uint32)
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes,", len(CASES), "cases, Pillow", PIL.__version__)
    assert os.path.getsize(OUT) < 100 * 1024


if __name__ == "__main__":
    main()
