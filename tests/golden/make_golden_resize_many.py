"""Fixture for resize_many (a list of different-sized uint8 images into one batch, one box per image): tests/golden/resize_many.npz.

Run by hand (needs Pillow; no GPU):  python tests/golden/make_golden_resize_many.py

The scheme of box_reduce.npz, per ITEM: for every case of CASES below, every filter of the case and every item, Pillow's own
``Image.resize((ow, oh), FILTER, box=...)`` as a CRC-32 of the whole [oH, oW, C] array and up to 256 sampled pixels, and the CRC-32 of the
item's input, which item_input() regenerates from its seed.  Expected outputs only: the file stays small.

The inputs, the CRC, the sampling and the numpy restatement of Pillow's resize with a box come from make_golden_box_reduce.py; main()
asserts that the restatement reproduces Pillow bit for bit on every fixture entry, so the tests may use it where Pillow is missing.
"""
from __future__ import annotations

import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "resize_many.npz")

_spec = importlib.util.spec_from_file_location("make_golden_box_reduce", os.path.join(HERE, "make_golden_box_reduce.py"))
_br = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_br)
make_batch, crc, sample_pixels, resize_box_restated = _br.make_batch, _br.crc, _br.sample_pixels, _br.resize_box_restated

FILTER_NAMES = ("linear", "cubic", "box", "hamming", "lanczos")


def _tiny37():
    rng = np.random.default_rng(37)
    return [(int(rng.integers(3, 21)), int(rng.integers(3, 21)), None) for _ in range(37)]


# (name, C, output (oh, ow), items [(H, W, box (x0, y0, x1, y1) or None)], filters, seed, one [N, C, H, W] tensor?)
# The smallest shapes at which each mechanism can go wrong:
CASES = [
    # shrinking, a sub-pixel box, width grows / height shrinks, both grow, Pillow's plain crop, a copy, and axes of one element
    ("m_mixed", 3, (30, 45), [(97, 131, None), (33, 200, (10.5, 2.25, 180.0, 30.5)), (61, 29, None), (12, 17, None),
                              (97, 131, (11, 5, 56, 35)), (30, 45, None), (1, 1, None), (1, 300, None), (300, 1, None)], FILTER_NAMES, 61, False),
    # windows of hundreds to thousands of taps: the staged segment is walked in chunks
    ("m_wide", 3, (7, 9), [(40, 3000, None), (2500, 33, None)], ("linear", "lanczos"), 62, False),
    ("m_c1", 1, (19, 77), [(50, 163, None), (25, 90, (3.5, 1.25, 80.0, 22.5)), (64, 40, None)], ("cubic", "box"), 63, False),
    ("m_c2", 2, (19, 77), [(50, 163, None), (25, 90, (3.5, 1.25, 80.0, 22.5)), (64, 40, None)], ("cubic", "box"), 64, False),
    ("m_c4", 4, (19, 77), [(50, 163, None), (25, 90, (3.5, 1.25, 80.0, 22.5)), (64, 40, None)], ("cubic", "box"), 65, False),
    # the search of a work unit's item across many items
    ("m_tiny37", 3, (5, 6), _tiny37(), ("linear",), 66, False),
    # three strips of output columns, the last one ragged
    ("m_strips", 3, (4, 130), [(9, 517, None), (8, 64, None)], ("hamming",), 67, False),
    # one [5, 3, 97, 131] tensor, five boxes, one of them None
    ("m_batchbox", 3, (30, 45), [(97, 131, (10.3, 7.6, 120.9, 90.2)), (97, 131, None), (97, 131, (0, 0, 64.5, 97)), (97, 131, (40, 30, 85, 60)),
                                 (97, 131, (3.7, 0.5, 131, 50.5))], ("linear", "cubic"), 68, True),
]


def case(name: str):
    return next(cs for cs in CASES if cs[0] == name)


def item_input(cs, i: int) -> np.ndarray:
    """[C, H, W] uint8 input of item i of a case (a batch case: slice i of one [N, C, H, W] batch)."""
    _, c, _, items, _, seed, batch = cs
    h, w, _ = items[i]
    if batch:
        return make_batch((len(items), c, h, w), seed)[i]
    return make_batch((1, c, h, w), 100 * seed + i)[0]


def entries():
    """Every (key, case, filter, item index) of the fixture, in the order its arrays are packed."""
    for cs in CASES:
        for f in cs[4]:
            for i in range(len(cs[3])):
                yield f"{cs[0]}/{f}/{i}", cs, f, i


def restated(cs, f: str, i: int, x: np.ndarray) -> np.ndarray:
    """[C, H, W] -> the expected [oH, oW, C] of one item, from the restatement."""
    oh, ow = cs[2]
    return resize_box_restated(f, np.ascontiguousarray(x.transpose(1, 2, 0)), oh, ow, cs[3][i][2])


def pillow(cs, f: str, i: int, x: np.ndarray) -> np.ndarray:
    """The same item from Pillow itself."""
    from PIL import Image

    flt = {"linear": Image.BILINEAR, "cubic": Image.BICUBIC, "box": Image.BOX, "hamming": Image.HAMMING, "lanczos": Image.LANCZOS}
    oh, ow = cs[2]
    box = cs[3][i][2]
    img = np.ascontiguousarray(x.transpose(1, 2, 0))
    c = img.shape[2]
    if c == 3:
        return np.asarray(Image.fromarray(img, "RGB").resize((ow, oh), flt[f], box=box))
    # 1, 2 and 4 plain channels: per-channel "L" images (LA / RGBA would premultiply)
    return np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(img[:, :, ch]), "L").resize((ow, oh), flt[f], box=box)) for ch in range(c)], axis=-1)


def expected(fx, key: str):
    """-> (CRC-32 of the item's input, CRC-32 of Pillow's [oH, oW, C] output, its pixels at sample_pixels() [n, C])."""
    i = [e[0] for e in entries()].index(key)
    counts = fx["sample_counts"]
    off = int(counts[:i].sum())
    c = int(fx["channels"][i])
    return int(fx["crcs"][i, 0]), int(fx["crcs"][i, 1]), fx["samples"][off:off + int(counts[i])].reshape(-1, c)


def pack(results):
    """results: [(input crc, output array [oH, oW, C])] in entries() order -> the fixture's arrays."""
    crcs, counts, samples, chans = [], [], [], []
    for incrc, out in results:
        c = out.shape[-1]
        px = out.reshape(-1, c)
        s = px[sample_pixels(len(px))].ravel()
        crcs.append([incrc, crc(out)])
        counts.append(len(s))
        samples.append(s)
        chans.append(c)
    return {"crcs": np.array(crcs, np.int64), "sample_counts": np.array(counts, np.int64), "samples": np.concatenate(samples),
            "channels": np.array(chans, np.int64)}


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
