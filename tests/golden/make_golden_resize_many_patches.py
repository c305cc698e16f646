"""Fixture for resize_many_to_patches (a ragged uint8 batch to packed ViT patch tokens): tests/golden/resize_many_patches.npz.

Run by hand (needs Pillow; no GPU):  python tests/golden/make_golden_resize_many_patches.py

The scheme of resize_many_placed.npz, per (case, filter, patch format): the CRC-32 of every item's input, the CRC-32 of the expected uint8
token matrix [sum T_i, C * ph * pw] and a few sampled rows of it (up to 8 rows, up to 32 columns of each: they say where a mismatch lies,
the CRC-32 is the check).  The expected matrix is Pillow's own ``Image.resize((vw, vh), FILTER, box=...)`` of every item, mirrored left to
right where the item flips, cut into patches by the numpy reshape / transpose of patchify() below, and concatenated.  item_input, crc and
the numpy restatement of the resize come from make_golden_resize_many.py; main() asserts that the restatement, cut the same way,
reproduces Pillow bit for bit on every entry, so the tests may use it where Pillow is missing.
"""
from __future__ import annotations

import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "resize_many_patches.npz")

_spec = importlib.util.spec_from_file_location("make_golden_resize_many", os.path.join(HERE, "make_golden_resize_many.py"))
_rm = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_rm)
crc = _rm.crc

FORMATS = ("cpp", "ppc")
_BOX = (10.5, 2.25, 180.0, 30.5)


def _c124(wide: int, flip: bool):
    """Three small items; the last one (two rows of `wide` columns from an 8 x 2000 source) is wider than one strip of the vertical pass."""
    return [(50, 163, None, (4, 9), False), (25, 90, (3.5, 1.25, 80.0, 22.5), (6, 12), False), (8, 2000, None, (2, wide), flip)]


# (name, C, patch (ph, pw), filters, items [(H, W, box (x0, y0, x1, y1) or None, (vh, vw), flip)], seed, one [N, C, H, W] tensor?)
# The smallest shapes at which the patch-writing pass can go wrong:
CASES = [
    # rows of 42 bytes per patch (interleaved): a lane's four bytes straddle pixel, patch and token boundaries.  One token row wider than
    # a 256-pixel strip and flipped; one token; up-scaling; a sub-pixel box
    ("t_vlm", 3, (14, 14), ("linear", "cubic"),
     [(97, 131, None, (42, 56), False), (61, 29, None, (70, 28), False), (33, 200, None, (14, 266), True), (40, 40, None, (14, 14), False),
      (12, 17, None, (28, 42), False), (33, 200, _BOX, (28, 84), False)], 81, False),
    ("t_p16", 3, (16, 16), ("lanczos",), [(97, 131, None, (32, 48), False), (300, 1, None, (16, 16), False), (1, 300, None, (16, 32), False)], 82, False),
    ("t_rect", 3, (2, 3), ("hamming",), [(9, 517, None, (4, 129), False), (8, 640, None, (2, 300), False)], 83, False),
    # every pixel is a token, D = C
    ("t_one", 3, (1, 1), ("box",), [(12, 17, None, (5, 7), False)], 84, False),
    ("t_c1", 1, (2, 3), ("cubic", "box"), _c124(1026, False), 85, False),
    ("t_c1_flip", 1, (2, 3), ("cubic", "box"), _c124(1026, True), 85, False),
    ("t_c2", 2, (2, 3), ("cubic", "box"), _c124(516, False), 86, False),
    ("t_c2_flip", 2, (2, 3), ("cubic", "box"), _c124(516, True), 86, False),
    ("t_c4", 4, (2, 3), ("cubic", "box"), _c124(258, False), 87, False),
    ("t_c4_flip", 4, (2, 3), ("cubic", "box"), _c124(258, True), 87, False),
    # the search of a work unit's item across many items, the first and the last item
    ("t_many", 3, (2, 2), ("linear",), [(12, 17, None, (4, 6), False) if i % 2 == 0 else (9, 11, None, (2, 2), False) for i in range(70)], 88, False),
    # one [5, 3, 97, 131] tensor, five sizes
    ("t_batch", 3, (14, 14), ("linear",),
     [(97, 131, None, (42, 56), False), (97, 131, None, (28, 28), False), (97, 131, None, (14, 70), False), (97, 131, None, (56, 42), False),
      (97, 131, None, (70, 14), False)], 89, True),
]


def case(name: str):
    return next(cs for cs in CASES if cs[0] == name)


def _plain_case(cs, i: int):
    """Item i's own resize as a case of make_golden_resize_many.py: the output is the item's (vh, vw)."""
    name, c, _, filters, items, seed, batch = cs
    return (name, c, items[i][3], [it[:3] for it in items], filters, seed, batch)


def item_input(cs, i: int) -> np.ndarray:
    """[C, H, W] uint8 input of item i of a case (a batch case: slice i of one [N, C, H, W] batch)."""
    return _rm.item_input(_plain_case(cs, i), i)


def entries():
    """Every (key, case, filter, format) of the fixture, in the order its arrays are packed."""
    for cs in CASES:
        for f in cs[3]:
            for fmt in FORMATS:
                yield f"{cs[0]}/{f}/{fmt}", cs, f, fmt


def patchify(r: np.ndarray, patch, fmt: str) -> np.ndarray:
    """[vh, vw, C] -> [gh * gw, C * ph * pw]: token (gy, gx) holds the patch's pixels as [C, ph, pw] ("cpp") or [ph, pw, C] ("ppc")."""
    ph, pw = patch
    vh, vw, c = r.shape
    assert vh % ph == 0 and vw % pw == 0
    p = r.reshape(vh // ph, ph, vw // pw, pw, c)  # gy, py, gx, px, c
    p = p.transpose(0, 2, 4, 1, 3) if fmt == "cpp" else p.transpose(0, 2, 1, 3, 4)
    return np.ascontiguousarray(p).reshape((vh // ph) * (vw // pw), c * ph * pw)


def tokens(cs, fmt: str, resized) -> np.ndarray:
    """The case's token matrix from its items' [vh, vw, C] resizes: each mirrored if it flips, cut, all concatenated."""
    return np.concatenate([patchify(r[:, ::-1] if it[4] else r, cs[2], fmt) for r, it in zip(resized, cs[4])])


def restated(cs, f: str, fmt: str, inputs) -> np.ndarray:
    """inputs [C, H, W] per item -> the expected token matrix, from the restatement of every item's [vh, vw] resize."""
    return tokens(cs, fmt, [_rm.restated(_plain_case(cs, i), f, i, x) for i, x in enumerate(inputs)])


def pillow(cs, f: str, fmt: str, inputs) -> np.ndarray:
    """The same matrix from Pillow itself."""
    return tokens(cs, fmt, [_rm.pillow(_plain_case(cs, i), f, i, x) for i, x in enumerate(inputs)])


def sample(tok: np.ndarray) -> np.ndarray:
    rows = np.unique(np.linspace(0, tok.shape[0] - 1, min(tok.shape[0], 8)).round().astype(np.int64))
    cols = np.unique(np.linspace(0, tok.shape[1] - 1, min(tok.shape[1], 32)).round().astype(np.int64))
    return tok[np.ix_(rows, cols)]


def expected(fx, key: str):
    """-> (CRC-32 of every item's input, CRC-32 of the expected token matrix, its sample() as a flat array)."""
    keys = [e[0] for e in entries()]
    i = keys.index(key)
    n = len(entries_case(key)[4])
    ioff = int(fx["item_counts"][:i].sum())
    soff = int(fx["sample_counts"][:i].sum())
    return fx["input_crcs"][ioff:ioff + n], int(fx["crcs"][i]), fx["samples"][soff:soff + int(fx["sample_counts"][i])]


def entries_case(key: str):
    return case(key.split("/")[0])


def main() -> None:
    import PIL

    crcs, item_counts, input_crcs, sample_counts, samples = [], [], [], [], []
    for key, cs, f, fmt in entries():
        inputs = [item_input(cs, i) for i in range(len(cs[4]))]
        pil = pillow(cs, f, fmt, inputs)
        assert np.array_equal(restated(cs, f, fmt, inputs), pil), f"the restatement differs from Pillow: {key}"
        crcs.append(crc(pil))
        item_counts.append(len(inputs))
        input_crcs += [crc(x) for x in inputs]
        s = sample(pil).ravel()
        sample_counts.append(len(s))
        samples.append(s)
    np.savez_compressed(OUT, crcs=np.array(crcs, np.int64), item_counts=np.array(item_counts, np.int64), input_crcs=np.array(input_crcs, np.int64),
                        sample_counts=np.array(sample_counts, np.int64), samples=np.concatenate(samples))
    print(OUT, os.path.getsize(OUT), "bytes,", len(crcs), "entries, Pillow", PIL.__version__)
    fx = np.load(OUT)
    for (key, _, _, _), c in zip(entries(), crcs):
        assert expected(fx, key)[1] == c


if __name__ == "__main__":
    main()
