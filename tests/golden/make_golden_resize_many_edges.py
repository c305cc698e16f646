"""Fixture for the ragged calls at the edges of their fixed tile sizes: tests/golden/resize_many_edges.npz.

Run by hand (needs Pillow; no GPU):  python tests/golden/make_golden_resize_many_edges.py

The packing of resize_many.npz and resize_many_placed.npz, per ITEM: for every case of CASES below, every filter of the case and every
item, the CRC-32 of the item's input, the CRC-32 of the expected [oH, oW, C] array and up to 256 sampled pixels of it.  A plain case
expects Pillow's own ``Image.resize((ow, oh), FILTER, box=...)``; a placed case expects Pillow's ``Image.resize((vw, vh), FILTER, box=...)``
pasted at (py, px) into a canvas of the fill colour, composed by make_golden_resize_many_placed.py's own paste().  Inputs, CRC, sampling and
the numpy restatement of the resize come from make_golden_resize_many.py; main() asserts that the restatement reproduces Pillow bit for bit
on every entry, so the tests may use it where Pillow is missing.

The shapes are the smallest that cross each tile size of csrc/aa_many.h and csrc/aa_many.hip: 1024 bytes of an output row per workgroup of
the vertical pass (AA_MANY_VBYTES), kVPixels<E> pixels per workgroup of the converting pass, 64 output columns per workgroup of the
horizontal pass (AA_MANY_STRIP) and (8192 - 4) / E staged input columns per chunk of it (kChunkCols).  Which case crosses which boundary,
in which layout class, is written down in EXPECT; tests/test_resize_many_edges_cpu.py recomputes every figure of it from the constants in
the source text, so a changed tile size fails there and names the case to move.  Every axis the kernels do not tile (heights) stays at 2
to 8.
"""
from __future__ import annotations

import collections
import importlib.util
import io
import os
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "resize_many_edges.npz")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_pl = _load("make_golden_resize_many_placed")
_rm = _pl._rm
crc, sample_pixels, pack = _rm.crc, _rm.sample_pixels, _rm.pack

# kind "plain": out is the batch's (oh, ow), an item is (H, W, box (x0, y0, x1, y1) or None).
# kind "placed": out is the canvas, fill one byte per channel, an item is (H, W, box, (vh, vw), (py, px)).
Case = collections.namedtuple("Case", "name kind c out fill filters items seed")

_GROW, _SHRINK, _TINY = (5, 400, None), (6, 2100, None), (4, 37, None)  # width grows, width shrinks, an ordinary small image
_WIDE_ITEMS = [_GROW, _SHRINK, _TINY]
_LC = ("linear", "cubic")


def _wide(name, c, ow, seed, filters=_LC):
    return Case(name, "plain", c, (3, ow), None, filters, _WIDE_ITEMS, seed)


def _place(item, size, offset):
    return item + (size, offset)


# A [3, 700] canvas of 3 interleaved bytes per pixel: 2100 bytes, strips [0, 1024), [1024, 2048), [2048, 2100) of the vertical pass and
# pieces of 256 pixels (768 bytes) of the converting pass.
_P700 = [
    _place(_GROW, (3, 120), (0, 300)),     # bytes [900, 1260): straddles byte 1024, starts on a dword
    _place(_SHRINK, (5, 40), (-1, 341)),   # bytes [1023, 1143): the first one is the last byte of strip 0, in a dword with three of fill
    _place(_TINY, (2, 12), (1, 684)),      # bytes [2052, 2088): wholly in strip 2, row 0 and strips 0 and 1 are fill only
    _place(_SHRINK, (3, 450), (0, -50)),   # cropped on the left, reaches pixel 400 = byte 1200, beyond strip 0 and beyond piece 0
    _place(_TINY, (3, 9), (0, 800)),       # off the canvas
    _place(_GROW, (3, 30), (0, 255)),      # bytes [765, 855): its first dword holds one byte of fill and is the last one of piece 0
]
# A [3, 1100] canvas of planes: strips [0, 1024), [1024, 1100) of both passes, per plane.
_P1100 = [
    _place(_GROW, (3, 120), (0, 960)),     # bytes [960, 1080): straddles byte 1024, starts on a dword
    _place(_SHRINK, (5, 40), (-1, 1023)),  # first byte the last one of strip 0
    _place(_TINY, (2, 50), (1, 1030)),     # wholly in strip 1: strip 0 is fill only
    _place(_SHRINK, (3, 1100), (0, -50)),  # cropped on the left, reaches byte 1050
    _place(_TINY, (3, 9), (4, 0)),         # off the canvas
]
_LONG = (5, 4000, None)

CASES = [
    # ---- wide rows, plain: more than AA_MANY_VBYTES bytes of an output row in at least one class
    _wide("w_c1_1027", 1, 1027, 91),                            # planar: two strips, three bytes in the last, rows at every alignment
    _wide("w_c3_1025", 3, 1025, 92),                            # planar: two strips per plane; interleaved: 3075 bytes, four strips
    _wide("w_c3_342", 3, 342, 93),                              # interleaved: 1026 bytes, two of them in strip 1
    _wide("w_c3_683", 3, 683, 94),                              # interleaved: 2049 bytes, three strips, one byte in the last
    _wide("w_c2_513", 2, 513, 95),                              # interleaved: 1026 bytes
    _wide("w_c4_257", 4, 257, 96),                              # interleaved: 1028 bytes, exactly one dword in strip 1
    _wide("w_c4_256", 4, 256, 97),                              # interleaved: 1024 bytes, one whole strip and no other
    _wide("w_c1_2048", 1, 2048, 98, ("linear", "cubic", "box")),  # planar: two whole strips, no ragged one
    # ---- wide canvases, placed
    Case("pw_c3_700", "placed", 3, (3, 700), (114, 7, 201), _LC, _P700, 101),
    Case("pw_c1_1100", "placed", 1, (3, 1100), (114,), _LC, _P1100, 102),
    Case("pw_c3_1100", "placed", 3, (3, 1100), (114, 7, 201), _LC, _P1100, 103),
    # the straddling item at 4 and at 2 bytes per pixel, and an item whose first dword is the last one of strip 0
    Case("pw_c4_300", "placed", 4, (3, 300), (200, 13, 99, 255), _LC,
         [_place(_GROW, (3, 60), (0, 225)), _place(_SHRINK, (5, 10), (-1, 255)), _place(_TINY, (2, 12), (1, 280))], 104),
    Case("pw_c2_600", "placed", 2, (3, 600), (200, 13), _LC,
         [_place(_GROW, (3, 120), (0, 450)), _place(_SHRINK, (5, 30), (-1, 511)), _place(_TINY, (2, 12), (1, 560))], 105),
    # ---- chunk seams of the horizontal pass, plain: a strip's input segment is longer than kChunkCols
    Case("k_c4_9", "plain", 4, (3, 9), None, _LC, [(5, 2100, None), _TINY, (6, 2100, (300.5, 0.5, 2090.25, 5.5))], 111),
    # 4200 -> 70: two chunks in strip 0, strip 1 begins mid-row; 4600 -> 70: three chunks in strip 0; the box's hull begins after column 0
    Case("k_c4_70", "plain", 4, (4, 70), None, _LC, [(5, 4200, None), (5, 4600, None), _TINY, (5, 4200, (100.5, 0.5, 4190.25, 4.5))], 112),
    # the box's hull begins at column 8 under the box filter (any wider filter reaches back to column 0)
    Case("k_c2_9", "plain", 2, (3, 9), None, ("linear", "cubic", "box"), [(6, 4200, None), _TINY, (6, 4200, (7.5, 0.5, 4190.25, 5.5))], 113),
    Case("k_c2_70", "plain", 2, (3, 70), None, _LC, [(5, 9000, None), _TINY], 114),
    # ---- one window longer than a chunk (3 and 4 bytes per pixel only: AA_MAX_KSIZE bounds ksize by the unclipped support)
    Case("l_c3_lin2", "plain", 3, (3, 2), None, ("linear",), [_LONG, _TINY, (6, 3500, None)], 121),
    Case("l_c4_lin2", "plain", 4, (3, 2), None, ("linear",), [_LONG, _TINY, (6, 3500, None)], 122),
    Case("l_c3_box1", "plain", 3, (3, 1), None, ("box",), [(5, 3000, None), _TINY, (6, 4090, None)], 123),
    Case("l_c4_box1", "plain", 4, (3, 1), None, ("box",), [(5, 3000, None), _TINY, (6, 4090, None)], 124),
    # 6140 -> 3 columns: the middle window, 4094 columns from column 1023, lies in three chunks of 2047
    Case("l_c4_lin3", "plain", 4, (3, 3), None, ("linear",), [(5, 6140, None), _TINY], 125),
    # ---- the 4000-column item resized to 4 columns, two of them on a canvas two columns wide: columns 1 and 2 (a hull of 3000 columns from
    # column 500) and columns 2 and 3 (2500 columns from column 1500)
    Case("pk_c3_2", "placed", 3, (3, 2), (9, 250, 77), ("linear",),
         [_place(_LONG, (3, 4), (0, -1)), _place(_TINY, (2, 4), (1, -1)), _place(_LONG, (3, 4), (0, -2))], 131),
    Case("pk_c4_2", "placed", 4, (3, 2), (9, 250, 77, 31), ("linear",),
         [_place(_LONG, (3, 4), (0, -1)), _place(_TINY, (2, 4), (1, -1)), _place(_LONG, (3, 4), (0, -2))], 132),
]

WIDE = [cs.name for cs in CASES if cs.name.startswith("w_")]
WIDE_PLACED = [cs.name for cs in CASES if cs.name.startswith("pw_")]
CHUNKED = [cs.name for cs in CASES if cs.name[:2] in ("k_", "l_")]
CHUNKED_PLACED = [cs.name for cs in CASES if cs.name.startswith("pk_")]

# What each case is there for, as figures the CPU test recomputes from the constants of the source text.  Per case and layout class
# ("interleaved" / "planar"; absent: the class crosses nothing and is not claimed):
#   "vstrips": work units of the vertical pass per output row (of a plane)
#   "pieces":  work units of the converting pass per output row (of a plane)
#   "chunks":  {(filter, item): chunks of each horizontal strip of that item}, the items that cross a chunk
#   "window":  {(filter, item)}: the longest window of the item is longer than one chunk
#   "spans":   {(filter, item): n}: some window of the item has taps in n chunks
#   "origin":  {(filter, item)}: the item's hull begins after column 0
#   "covered": {item: (strip of the first covered byte, strip of the last covered byte) or None (off the canvas)}, placed cases
def _each(filters, d):
    return {(f, i): v for f in filters for i, v in d.items()}


EXPECT = {
    "w_c1_1027": {"planar": {"vstrips": 2, "pieces": 2}},
    "w_c3_1025": {"planar": {"vstrips": 2, "pieces": 2}, "interleaved": {"vstrips": 4, "pieces": 5}},
    "w_c3_342": {"interleaved": {"vstrips": 2, "pieces": 2}},
    "w_c3_683": {"interleaved": {"vstrips": 3, "pieces": 3}},
    "w_c2_513": {"interleaved": {"vstrips": 2, "pieces": 2}},
    "w_c4_257": {"interleaved": {"vstrips": 2, "pieces": 2}},
    "w_c4_256": {"interleaved": {"vstrips": 1, "pieces": 1}},
    "w_c1_2048": {"planar": {"vstrips": 2, "pieces": 2}},
    "pw_c3_700": {"interleaved": {"vstrips": 3, "pieces": 3, "covered": {0: (0, 1), 1: (0, 1), 2: (2, 2), 3: (0, 1), 4: None, 5: (0, 0)}}},
    "pw_c1_1100": {"planar": {"vstrips": 2, "pieces": 2, "covered": {0: (0, 1), 1: (0, 1), 2: (1, 1), 3: (0, 1), 4: None}}},
    "pw_c3_1100": {"planar": {"vstrips": 2, "pieces": 2, "covered": {0: (0, 1), 1: (0, 1), 2: (1, 1), 3: (0, 1), 4: None}},
                   "interleaved": {"vstrips": 4, "pieces": 5, "covered": {0: (2, 3), 1: (2, 3), 2: (3, 3), 3: (0, 3), 4: None}}},
    "pw_c4_300": {"interleaved": {"vstrips": 2, "pieces": 2, "covered": {0: (0, 1), 1: (0, 1), 2: (1, 1)}}},
    "pw_c2_600": {"interleaved": {"vstrips": 2, "pieces": 2, "covered": {0: (0, 1), 1: (0, 1), 2: (1, 1)}}},
    "k_c4_9": {"interleaved": {"chunks": _each(_LC, {0: [2]}), "origin": _each(_LC, {2: True})}},
    "k_c4_70": {"interleaved": {"chunks": _each(_LC, {0: [2, 1], 1: [3, 1], 3: [2, 1]}), "origin": _each(_LC, {3: True})}},
    "k_c2_9": {"interleaved": {"chunks": _each(("linear", "cubic", "box"), {0: [2], 2: [2]}), "origin": {("box", 2): True}}},
    "k_c2_70": {"interleaved": {"chunks": _each(_LC, {0: [3, 1]})}},
    "l_c3_lin2": {"interleaved": {"chunks": {("linear", 0): [2], ("linear", 2): [2]}, "window": {("linear", 0): True},
                                  "spans": {("linear", 0): 2}}},
    "l_c4_lin2": {"interleaved": {"chunks": {("linear", 0): [2], ("linear", 2): [2]}, "window": {("linear", 0): True, ("linear", 2): True},
                                  "spans": {("linear", 0): 2}}},
    "l_c3_box1": {"interleaved": {"chunks": {("box", 0): [2], ("box", 2): [2]}, "window": {("box", 0): True, ("box", 2): True},
                                  "spans": {("box", 0): 2, ("box", 2): 2}}},
    "l_c4_box1": {"interleaved": {"chunks": {("box", 0): [2], ("box", 2): [2]}, "window": {("box", 0): True, ("box", 2): True},
                                  "spans": {("box", 0): 2, ("box", 2): 2}}},
    "l_c4_lin3": {"interleaved": {"chunks": {("linear", 0): [3]}, "window": {("linear", 0): True}, "spans": {("linear", 0): 3}}},
    "pk_c3_2": {"interleaved": {"chunks": {("linear", 0): [2], ("linear", 2): [1]}, "origin": {("linear", 0): True, ("linear", 2): True}}},
    "pk_c4_2": {"interleaved": {"chunks": {("linear", 0): [2], ("linear", 2): [2]}, "origin": {("linear", 0): True, ("linear", 2): True}}},
}


def case(name: str) -> Case:
    return next(cs for cs in CASES if cs.name == name)


def as_plain(cs: Case):
    """The case in make_golden_resize_many.py's form."""
    assert cs.kind == "plain"
    return (cs.name, cs.c, cs.out, cs.items, cs.filters, cs.seed, False)


def as_placed(cs: Case):
    """The case in make_golden_resize_many_placed.py's form."""
    assert cs.kind == "placed"
    return (cs.name, cs.c, cs.out, cs.fill, cs.filters, cs.items, cs.seed, False)


def item_input(cs: Case, i: int) -> np.ndarray:
    """[C, H, W] uint8 input of item i of a case."""
    return _rm.item_input(as_plain(cs), i) if cs.kind == "plain" else _pl.item_input(as_placed(cs), i)


def entries():
    """Every (key, case, filter, item index) of the fixture, in the order its arrays are packed."""
    for cs in CASES:
        for f in cs.filters:
            for i in range(len(cs.items)):
                yield f"{cs.name}/{f}/{i}", cs, f, i


def restated(cs: Case, f: str, i: int, x: np.ndarray) -> np.ndarray:
    """[C, H, W] -> the expected [oH, oW, C] of one item, from the restatement (a placed item: pasted by the placed maker)."""
    return _rm.restated(as_plain(cs), f, i, x) if cs.kind == "plain" else _pl.restated(as_placed(cs), f, i, x)


def pillow(cs: Case, f: str, i: int, x: np.ndarray) -> np.ndarray:
    """The same item from Pillow itself."""
    return _rm.pillow(as_plain(cs), f, i, x) if cs.kind == "plain" else _pl.pillow(as_placed(cs), f, i, x)


def expected(fx, key: str):
    """-> (CRC-32 of the item's input, CRC-32 of the expected [oH, oW, C] array, its pixels at sample_pixels() [n, C])."""
    i = [e[0] for e in entries()].index(key)
    counts = fx["sample_counts"]
    off = int(counts[:i].sum())
    c = int(fx["channels"][i])
    return int(fx["crcs"][i, 0]), int(fx["crcs"][i, 1]), fx["samples"][off:off + int(counts[i])].reshape(-1, c)


def save(path: str, arrays) -> None:
    """np.savez_compressed with the archive's timestamps fixed: the same arrays give the same file, byte for byte."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main() -> None:
    import PIL

    results = []
    inputs = {}
    for key, cs, f, i in entries():
        if (cs.name, i) not in inputs:
            inputs[cs.name, i] = item_input(cs, i)
        x = inputs[cs.name, i]
        pil = pillow(cs, f, i, x)
        mine = restated(cs, f, i, x)
        assert np.array_equal(mine, pil), f"the restatement differs from Pillow: {key}"
        results.append((crc(x), pil))
    save(OUT, pack(results))
    print(OUT, os.path.getsize(OUT), "bytes,", len(results), "entries, Pillow", PIL.__version__)
    fx = np.load(OUT)
    for (key, _, _, _), (incrc, out) in zip(entries(), results):
        e = expected(fx, key)
        assert e[0] == incrc and e[1] == crc(out)


if __name__ == "__main__":
    main()
