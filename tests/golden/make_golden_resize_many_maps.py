"""Fixture for resize_many_maps (Pillow's "I;16" / "I" / "F" resize for ragged batches): tests/golden/resize_many_maps.npz.

Run by hand (needs Pillow; no GPU):  python tests/golden/make_golden_resize_many_maps.py

Pillow only: for every case of CASES below, every filter and dtype the case names and every item, ``Image.resize((vw, vh), FILTER,
box=...)``, ``paste`` at (px, py) onto an ``Image.new`` canvas of the fill, and ``transpose(FLIP_LEFT_RIGHT)`` where the item flips.
The fixture holds every input ONCE as a uint16 array (``<case>__in<i>``) — the three dtypes derive from it by exact integer and IEEE
operations (as_dtype) — and every expected [N, oH, oW] batch whole (``<case>__<filter>__<dtype>``).

main() asserts, before it writes anything, that the numpy restatement (tests/resize_many_maps_ref.py) reproduces Pillow bit for bit on
every case, that the "I;16" overflow cases differ from a plain clamp, and that the fused-accumulation case tells a fused multiply-add
from Pillow's multiply and add.
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "resize_many_maps.npz")

ALL = ("bilinear", "bicubic", "box", "hamming", "lanczos")
DTS = ("u16", "i32", "f32")
FILLS = {"u16": 40000, "i32": -7, "f32": -1.5}
PIL_FILTER = {"bilinear": "BILINEAR", "bicubic": "BICUBIC", "box": "BOX", "hamming": "HAMMING", "lanczos": "LANCZOS"}

# items: (H, W, box (x0, y0, x1, y1) or None[, (vh, vw) or None, (py, px) or None]); canvas (oh, ow); placed: the case writes the fill
CASES = {
    # every filter x every dtype on a ragged list: down-scaled with a fractional box, up-scaled, width kept (vertical pass only), height
    # kept (horizontal pass only), a plain copy (an integer box of the canvas's size)
    "ragged": dict(canvas=(20, 23), filters=ALL, dtypes=DTS, seed=1,
                   items=[(70, 131, (3.25, 2.5, 120.75, 66.25)), (8, 9, None), (41, 23, None), (20, 35, None), (27, 35, (5, 4, 28, 24))]),
    # long windows: Lanczos 131 -> 5 is a window of about 159 taps, on either axis
    "long_w": dict(canvas=(7, 5), filters=("lanczos",), dtypes=DTS, seed=2, items=[(12, 131, None)]),
    "long_h": dict(canvas=(5, 7), filters=("lanczos",), dtypes=DTS, seed=3, items=[(131, 12, None)]),
    # output rows of one horizontal work unit (64 columns) plus one, and of two plus one
    "wide65": dict(canvas=(5, 65), filters=("bicubic",), dtypes=DTS, seed=4, items=[(6, 40, None), (5, 90, (0.5, 0.0, 88.0, 5.0))]),
    "wide129": dict(canvas=(5, 129), filters=("bicubic",), dtypes=DTS, seed=5, items=[(6, 40, None), (5, 200, (1.0, 0.0, 199.5, 5.0))]),
    # canvas rows wider than one vertical work unit (256 columns), one item mirrored, one placed across the seam
    "vwide": dict(canvas=(3, 300), filters=("bilinear",), dtypes=DTS, seed=6, placed=True, flips=[False, True, True],
                  items=[(4, 50, None), (4, 50, None), (5, 30, None, (3, 40), (0, 240))]),
    # "I;16" overflow: 6 x 12 of {0, 200, 65300, 65535} to 6 x 29 and its transpose; 37 and 28 of 174 pixels differ from a plain clamp
    "over": dict(canvas=(6, 29), filters=("bicubic",), dtypes=("u16",), pattern=True, items=[(6, 12, None)]),
    "over_t": dict(canvas=(29, 6), filters=("bicubic",), dtypes=("u16",), pattern=True, items=[(12, 6, None)]),
    # placement: overhang on all four sides, a float box cropped left and right, an item wholly off the canvas, a placed copy, a placed
    # vertical-only item that runs off the right edge, a placed horizontal-only item; half of them mirrored
    "placed": dict(canvas=(30, 45), filters=("bicubic",), dtypes=DTS, seed=7, placed=True, flips=[False, True, True, False, True, True],
                   items=[(20, 31, None, (40, 60), (-5, -7)), (33, 50, (10.5, 2.25, 45.0, 30.5), (20, 70), (15, -50)), (12, 17, None, (6, 6), (100, 3)),
                          (12, 17, None, (12, 17), (3, 20)), (9, 14, None, (50, 14), (-13, 34)), (25, 30, None, (25, 11), (2, 1))]),
    "placed_lanczos": dict(canvas=(14, 19), filters=("lanczos",), dtypes=DTS, seed=8, placed=True, flips=[True, False],
                           items=[(20, 31, None, (17, 25), (-2, -3)), (9, 14, None, (9, 30), (5, -4))]),
    "center": dict(canvas=(14, 14), filters=("bilinear",), dtypes=DTS, seed=9, placed=True, center=True, flips=[False, True, False],
                   items=[(25, 35, None, (16, 22), None), (20, 10, None, (33, 9), None), (9, 9, None, (10, 7), None)]),
    # same size under a half-pixel box: both passes run at scale 1 (and hamming, whose support then is one pixel)
    "halfpx": dict(canvas=(11, 13), filters=("hamming", "lanczos"), dtypes=DTS, seed=10, items=[(11, 13, (0.5, 0.0, 13.0, 10.5))]),
    # built to tell fused from unfused accumulation (asserted by main() and by the CPU test):
    # rows (v0, v1) chosen so that an exact sum of 2 -> 12 lies on a rounding tie (5 v0 + 7 v1 = 6 mod 12 and its kin): the last bit of
    # the double sum decides the stored integer, and a fused multiply-add rounds it the other way on every row, bilinear on the first six,
    # bicubic on the last two
    "fma": dict(canvas=(8, 12), filters=("bilinear", "bicubic"), dtypes=("u16",), items=[(8, 2, None)],
                values=[(10041, 20739), (2998, 52012), (9259, 58069), (9156, 16170), (38302, 44428), (2024, 24530), (36794, 8864), (62272, 47362)]),
}


def _boxmath():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from interpolate_antialiasing_amd import boxmath

    return boxmath


def geometry(cs, i: int):
    """Item i -> (H, W, box or None, (vh, vw), (py, px)), sizes and offsets resolved (None: the canvas, (0, 0); a "center" case centred)."""
    it = tuple(cs["items"][i]) + (None, None)
    h, w, box, size, off = it[:5]
    oh, ow = cs["canvas"]
    vh, vw = size if size is not None else (oh, ow)
    if cs.get("center"):
        bm = _boxmath()
        off = (bm.center_offset(vh, oh), bm.center_offset(vw, ow))
    py, px = off if off is not None else (0, 0)
    return h, w, box, (vh, vw), (py, px)


def boxes(cs):
    return [geometry(cs, i)[2] for i in range(len(cs["items"]))]


def sizes(cs):
    return [geometry(cs, i)[3] for i in range(len(cs["items"]))] if cs.get("placed") else None


def offsets(cs):
    if not cs.get("placed"):
        return None
    return "center" if cs.get("center") else [geometry(cs, i)[4] for i in range(len(cs["items"]))]


def base_input(cs, i: int) -> np.ndarray:
    """The stored uint16 [H, W] array of item i: the whole range, or the four values of the overflow cases."""
    h, w = cs["items"][i][0], cs["items"][i][1]
    if cs.get("values"):
        return np.array(cs["values"], np.uint16).reshape(h, w)
    if cs.get("pattern"):
        vals = np.array([0, 200, 65300, 65535], np.uint16)
        return vals[np.random.default_rng([99, h, w]).integers(0, 4, (h, w))]
    return np.random.default_rng([cs["seed"], i]).integers(0, 65536, (h, w)).astype(np.uint16)


_DECADES = np.array([1e-3, 1e-2, 1e-1, 1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6])


def as_dtype(u: np.ndarray, dt: str) -> np.ndarray:
    """The stored uint16 array as one of the three dtypes, by exact integer and single IEEE operations:
    u16 the values themselves; i32 up to +-2^29 with busy low bits; f32 24-bit mantissas of mixed sign over 1e-3 .. 1e6."""
    u = u.astype(np.int64)
    if dt == "u16":
        return u.astype(np.uint16)
    if dt == "i32":
        return ((u - 32768) * 16381 + u % 7919).astype(np.int32)
    mant = ((u * 2654435761) % (1 << 24)).astype(np.float64) / float(1 << 24) + 0.5
    sign = np.where(u & 16, 1.0, -1.0)
    return (mant * _DECADES[u % 10] * sign).astype(np.float32)


def _to_pil(x: np.ndarray, dt: str):
    from PIL import Image

    h, w = x.shape
    if dt == "u16":
        return Image.frombytes("I;16", (w, h), np.ascontiguousarray(x).tobytes())
    return Image.fromarray(np.ascontiguousarray(x))  # "I", "F"


def pillow(cs, xs, name: str, dt: str) -> np.ndarray:
    """The expected [N, oH, oW] batch of a case from Pillow itself."""
    from PIL import Image

    oh, ow = cs["canvas"]
    fill = FILLS[dt] if cs.get("placed") else 0
    out = np.empty((len(xs), oh, ow), xs[0].dtype)
    for i, x in enumerate(xs):
        _, _, box, (vh, vw), (py, px) = geometry(cs, i)
        im = _to_pil(x, dt)
        r = im.resize((vw, vh), getattr(Image, PIL_FILTER[name]), box=box)
        canvas = Image.new(im.mode, (ow, oh), fill)
        canvas.paste(r, (px, py))
        if cs.get("flips") is not None and cs["flips"][i]:
            canvas = canvas.transpose(Image.FLIP_LEFT_RIGHT)
        out[i] = np.asarray(canvas).reshape(oh, ow)
    return out


def _ref():
    spec = importlib.util.spec_from_file_location("resize_many_maps_ref", os.path.join(ROOT, "tests", "resize_many_maps_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _bits(a: np.ndarray) -> np.ndarray:
    return a.view(np.int32) if a.dtype == np.float32 else a


def main() -> None:
    import PIL

    ref = _ref()
    arrays = {}
    for case, cs in CASES.items():
        base = [base_input(cs, i) for i in range(len(cs["items"]))]
        for i, u in enumerate(base):
            arrays[f"{case}__in{i}"] = u
        for dt in cs["dtypes"]:
            xs = [as_dtype(u, dt) for u in base]
            kw = dict(boxes=boxes(cs), sizes=sizes(cs), offsets=offsets(cs), flips=cs.get("flips"), fill=FILLS[dt] if cs.get("placed") else 0)
            for name in cs["filters"]:
                pil = pillow(cs, xs, name, dt)
                mine = ref.many(xs, cs["canvas"], name, **kw)
                assert mine.dtype == pil.dtype and np.array_equal(_bits(mine), _bits(pil)), f"the restatement differs from Pillow: {case} {name} {dt}"
                if case in ("over", "over_t"):
                    clamped = ref.many(xs, cs["canvas"], name, overflow="clamp", **kw)
                    differ = int((clamped != pil).sum())
                    assert differ > 0, f"{case}: Pillow's store equals a clamp"
                    print(f"{case}: {differ} of {pil.size} pixels differ from a plain clamp; 65302 present: {bool((pil == 65302).any())}")
                if case == "fma":
                    fused = ref.many(xs, cs["canvas"], name, fused=True, **kw)
                    rows = (fused != pil).any(axis=2)[0]
                    assert rows[:6].all() if name == "bilinear" else rows[6:].all(), f"the fma case does not tell fused from unfused accumulation: {name}"
                arrays[f"{case}__{name}__{dt}"] = pil
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes,", len(CASES), "cases, Pillow", PIL.__version__)
    assert os.path.getsize(OUT) < 600 * 1024


if __name__ == "__main__":
    main()
