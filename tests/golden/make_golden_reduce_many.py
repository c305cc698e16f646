"""Fixture for reduce_many / reduce_many_for_resize (Pillow's reducing_gap for a list of different-sized uint8 images):
tests/golden/reduce_many.npz.

Run by hand (needs Pillow; no GPU):  python tests/golden/make_golden_reduce_many.py

The scheme of resize_many.npz, per ITEM: for every case of CASES below, every filter of the case and every item,
  * Pillow's own ``Image.resize((ow, oh), FILTER, box=..., reducing_gap=gap)`` as a CRC-32 of the whole [oh, ow, C] array and up to 64
    sampled pixels, and the CRC-32 of the item's input, which item_input() regenerates from its seed;
  * what Image.resize computes on the way — the factors, the reduce box (Image._get_safe_box) and the shifted box, zeros for an item
    that is not reduced — and, for a reduced item, Pillow's own ``Image.reduce(factor, reduce_box)`` as a CRC-32 and sampled pixels.
Expected outputs only: the file stays small.

The inputs, the CRC and the numpy restatements (reduce_restated, resize_box_restated, gap_plan) come from make_golden_box_reduce.py;
main() asserts that reduce_restated + resize_box_restated with the shifted box reproduce Pillow bit for bit on every entry, that every
reduced item's bytes differ from the resize without a gap (a test fails if the gap is ignored), and that the factors are the ones the
case table names.  The tests may then use the restatement where Pillow is missing.
"""
from __future__ import annotations

import importlib.util
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reduce_many.npz")

_spec = importlib.util.spec_from_file_location("make_golden_box_reduce", os.path.join(HERE, "make_golden_box_reduce.py"))
_br = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_br)
make_batch, crc, resize_box_restated, reduce_restated, gap_plan = _br.make_batch, _br.crc, _br.resize_box_restated, _br.reduce_restated, _br.gap_plan

FILTER_NAMES = ("linear", "cubic", "box", "hamming", "lanczos")
SAMPLES = 64


def sample_pixels(npx: int) -> np.ndarray:
    return np.unique(np.linspace(0, npx - 1, min(npx, SAMPLES)).round().astype(np.int64))


def _tiny37():
    rng = np.random.default_rng(37)
    return [(int(rng.integers(3, 61)), int(rng.integers(3, 61)), None) for _ in range(37)]


def fit_shorter(shapes, s: int):
    """boxmath.fit_sizes(shapes, shorter=s), restated (the CPU tests compare the two)."""
    out = []
    for h, w in shapes:
        short, long = (h, w) if h <= w else (w, h)
        a, b = s, int(s * long / short)
        out.append((a, b) if h <= w else (b, a))
    return out


def fit_patches(shapes, patch, max_tokens: int):
    """boxmath.fit_patch_sizes(shapes, patch, max_tokens=max_tokens), restated (the CPU tests compare the two)."""
    ph, pw = patch
    out = []
    for h, w in shapes:
        vh, vw = max(ph, round(h / ph) * ph), max(pw, round(w / pw) * pw)
        if (vh // ph) * (vw // pw) > max_tokens:
            beta = math.sqrt(h * w / (max_tokens * ph * pw))
            vh, vw = max(ph, math.floor(h / beta / ph) * ph), max(pw, math.floor(w / beta / pw) * pw)
        out.append((vh, vw))
    return out


_MIXED = [(400, 610, None), (97, 131, None), (300, 100, None), (64, 900, (10.5, 2.25, 880.0, 60.5)), (401, 613, (11, 5, 560, 395)), (30, 45, None),
          (1, 1, None)]
_C124 = [(200, 652, None), (100, 360, (3.5, 1.25, 320.0, 90.5)), (64, 40, None)]
PATCH = (4, 4)

# (name, C, output (oh, ow), gap, items [(H, W, box (x0, y0, x1, y1) or None)], filters, seed, one [N, C, H, W] tensor?,
#  per-item sizes [(vh, vw)] or None, the factors the case is there for: {item: (fx, fy) or None}, for every filter of the case)
CASES = [
    # reduced and unreduced items in one list, one-axis factors, a sub-pixel box, partial right / bottom / corner blocks, a copy, 1 x 1
    ("g_mixed", 3, (30, 45), 2.0, _MIXED, FILTER_NAMES, 71, False, None,
     {0: (6, 6), 1: None, 2: (1, 5), 3: (9, 1), 4: (6, 6), 5: None, 6: None}),
    # 4503 bytes per row: two tiles, the last one ragged, an odd width
    ("g_seam", 3, (4, 375), 2.0, [(9, 1501, None), (8, 64, None)], ("linear",), 72, False, None, {0: (2, 1), 1: None}),
    # more than 256 rows per block: the 16-bit sums are emptied
    ("g_tall", 1, (2, 4), 1.0, [(530, 9, None), (5, 9, None)], ("cubic",), 73, False, None, {0: (2, 265), 1: (2, 2)}),
    # 4500-byte blocks: the chunked form next to the tiled form in one launch
    ("g_wideblock", 3, (3, 2), 1.0, [(7, 3001, None), (40, 33, None)], ("linear",), 74, False, None, {0: (1500, 2), 1: (16, 13)}),
    # every pixel width
    ("g_c1", 1, (19, 77), 2.0, _C124, ("cubic", "box"), 75, False, None, {0: (4, 5), 1: (2, 2), 2: None}),
    ("g_c2", 2, (19, 77), 2.0, _C124, ("cubic", "box"), 76, False, None, {0: (4, 5), 1: (2, 2), 2: None}),
    ("g_c4", 4, (19, 77), 2.0, _C124, ("cubic", "box"), 77, False, None, {0: (4, 5), 1: (2, 2), 2: None}),
    # the search of a work unit's item across many items, factors 1..11
    ("g_tiny37", 3, (5, 6), 1.0, _tiny37(), ("linear",), 78, False, None, {}),
    # slices of one [5, 3, 194, 262] tensor, per-item factors
    ("g_batchbox", 3, (30, 45), 2.0, [(194, 262, (10.3, 7.6, 250.9, 190.2)), (194, 262, None), (194, 262, (0, 0, 64.5, 194)),
                                      (194, 262, (40, 30, 85, 60)), (194, 262, (3.7, 0.5, 262, 50.5))], ("linear", "cubic"), 79, True, None,
     {0: (2, 3), 1: (2, 3), 2: (1, 3), 3: None, 4: (2, 1)}),
    # g_mixed's items, each resized to its own size: Resize(40) for a centred (30, 45) canvas; a multiple of the (4, 4) patch
    ("g_fit", 3, (30, 45), 2.0, _MIXED, ("linear", "cubic"), 71, False, fit_shorter([it[:2] for it in _MIXED], 40), {}),
    ("g_patch", 3, (30, 45), 2.0, _MIXED, ("cubic",), 71, False, fit_patches([it[:2] for it in _MIXED], PATCH, 48), {}),
]


def case(name: str):
    return next(cs for cs in CASES if cs[0] == name)


def item_input(cs, i: int) -> np.ndarray:
    """[C, H, W] uint8 input of item i of a case (a batch case: slice i of one [N, C, H, W] batch)."""
    _, c, _, _, items, _, seed, batch = cs[:8]
    h, w, _ = items[i]
    if batch:
        return make_batch((len(items), c, h, w), seed)[i]
    return make_batch((1, c, h, w), 100 * seed + i)[0]


def out_size(cs, i: int):
    """(oh, ow) item i is resized to."""
    return cs[8][i] if cs[8] is not None else cs[2]


def entries():
    """Every (key, case, filter, item index) of the fixture, in the order its arrays are packed."""
    for cs in CASES:
        for f in cs[5]:
            for i in range(len(cs[4])):
                yield f"{cs[0]}/{f}/{i}", cs, f, i


def plan(cs, f: str, i: int):
    """Image.resize's own arithmetic for item i -> (factor (fx, fy), reduce box or None, the box of the resize that follows or None)."""
    h, w, box = cs[4][i]
    oh, ow = out_size(cs, i)
    bx = tuple(float(v) for v in box) if box is not None else (0.0, 0.0, float(w), float(h))
    if (w, h) == (ow, oh) and bx == (0.0, 0.0, float(w), float(h)):
        return (1, 1), None, None  # (a copy: Pillow returns before it looks at reducing_gap)
    factor, rb, sb = gap_plan(w, h, ow, oh, f, bx, cs[3])
    return factor, rb, (sb if rb is not None else box)


def restated(cs, f: str, i: int, x: np.ndarray):
    """[C, H, W] -> (the expected [oh, ow, C] of one item, its reduced image [rh, rw, C] or None), from the restatements composed as the
    package composes them: reduce, then the resize with the shifted box."""
    oh, ow = out_size(cs, i)
    img = np.ascontiguousarray(x.transpose(1, 2, 0))
    factor, rb, sb = plan(cs, f, i)
    if rb is None:
        return resize_box_restated(f, img, oh, ow, cs[4][i][2]), None
    red = reduce_restated(img, factor, rb)
    return resize_box_restated(f, red, oh, ow, sb), red


def _per_channel(img: np.ndarray, run) -> np.ndarray:
    from PIL import Image

    c = img.shape[2]
    if c == 3:
        return np.asarray(run(Image.fromarray(img, "RGB")))
    # 1, 2 and 4 plain channels: per-channel "L" images (LA / RGBA would premultiply, and drop reducing_gap)
    return np.stack([np.asarray(run(Image.fromarray(np.ascontiguousarray(img[:, :, ch]), "L"))) for ch in range(c)], axis=-1)


def pillow(cs, f: str, i: int, x: np.ndarray, gap="case"):
    """The same item from Pillow itself -> (Image.resize(..., reducing_gap=) [oh, ow, C], Image.reduce(factor, reduce box) or None)."""
    from PIL import Image

    flt = {"linear": Image.BILINEAR, "cubic": Image.BICUBIC, "box": Image.BOX, "hamming": Image.HAMMING, "lanczos": Image.LANCZOS}
    oh, ow = out_size(cs, i)
    box = cs[4][i][2]
    img = np.ascontiguousarray(x.transpose(1, 2, 0))
    out = _per_channel(img, lambda im: im.resize((ow, oh), flt[f], box=box, reducing_gap=cs[3] if gap == "case" else gap))
    factor, rb, _ = plan(cs, f, i)
    red = _per_channel(img, lambda im: im.reduce(factor, box=rb)) if rb is not None and gap == "case" else None
    return out, red


def _index(key: str) -> int:
    return [e[0] for e in entries()].index(key)


def _slice(fx, prefix: str, i: int):
    counts = fx[prefix + "sample_counts"]
    off = int(counts[:i].sum())
    c = int(fx["channels"][i])
    return fx[prefix + "samples"][off:off + int(counts[i])].reshape(-1, c)


def expected(fx, key: str):
    """-> (CRC-32 of the item's input, CRC-32 of Pillow's [oh, ow, C] gap resize, its pixels at sample_pixels() [n, C])."""
    i = _index(key)
    return int(fx["crcs"][i, 0]), int(fx["crcs"][i, 1]), _slice(fx, "", i)


def expected_reduce(fx, key: str):
    """-> None for an item that is not reduced, else (CRC-32 of Pillow's Image.reduce [rh, rw, C], its pixels at sample_pixels())."""
    i = _index(key)
    if int(fx["factors"][i, 0]) == 0:
        return None
    return int(fx["crcs"][i, 2]), _slice(fx, "reduce_", i)


def recorded_plan(fx, key: str):
    """-> None, or (factor (fx, fy), reduce box, shifted box) as recorded when the fixture was made."""
    i = _index(key)
    if int(fx["factors"][i, 0]) == 0:
        return None
    return tuple(int(v) for v in fx["factors"][i]), tuple(int(v) for v in fx["reduce_boxes"][i]), tuple(float(v) for v in fx["shifted_boxes"][i])


def pack(results):
    """results: [(input crc, output [oh, ow, C], reduced [rh, rw, C] or None, plan or None)] in entries() order -> the fixture's arrays."""
    crcs, counts, samples, chans, rcounts, rsamples, factors, rboxes, sboxes = [], [], [], [], [], [], [], [], []
    for incrc, out, red, pl in results:
        c = out.shape[-1]
        px = out.reshape(-1, c)
        s = px[sample_pixels(len(px))].ravel()
        counts.append(len(s))
        samples.append(s)
        chans.append(c)
        if red is None:
            rs = np.zeros(0, np.uint8)
            factors.append((0, 0)); rboxes.append((0, 0, 0, 0)); sboxes.append((0.0, 0.0, 0.0, 0.0))
        else:
            rpx = red.reshape(-1, c)
            rs = rpx[sample_pixels(len(rpx))].ravel()
            factors.append(pl[0]); rboxes.append(pl[1]); sboxes.append(pl[2])
        rcounts.append(len(rs))
        rsamples.append(rs)
        crcs.append([incrc, crc(out), crc(red) if red is not None else 0])
    return {"crcs": np.array(crcs, np.int64), "sample_counts": np.array(counts, np.int64), "samples": np.concatenate(samples),
            "channels": np.array(chans, np.int64), "reduce_sample_counts": np.array(rcounts, np.int64),
            "reduce_samples": np.concatenate(rsamples), "factors": np.array(factors, np.int64), "reduce_boxes": np.array(rboxes, np.int64),
            "shifted_boxes": np.array(sboxes, np.float64)}


def main() -> None:
    import PIL

    results = []
    reduced = 0
    for key, cs, f, i in entries():
        x = item_input(cs, i)
        pil, pil_red = pillow(cs, f, i, x)
        mine, mine_red = restated(cs, f, i, x)
        assert np.array_equal(mine, pil), f"reduce + the resize with the shifted box differs from Pillow's reducing_gap: {key}"
        factor, rb, sb = plan(cs, f, i)
        want = cs[9].get(i, "any")
        assert want == "any" or (want is None and rb is None) or (want == factor and rb is not None), f"{key}: factor {factor}, the case names {want}"
        if rb is not None:
            assert np.array_equal(mine_red, pil_red), f"the restated reduce differs from Image.reduce: {key}"
            plain, _ = pillow(cs, f, i, x, gap=None)
            assert not np.array_equal(plain, pil), f"{key}: the gap changes nothing, so a test could not see it ignored"
            reduced += 1
        results.append((crc(x), pil, pil_red, (factor, rb, sb) if rb is not None else None))
    for name in ("g_tiny37", "g_fit", "g_patch"):
        cs = case(name)
        fs = {plan(cs, cs[5][0], i)[0] for i in range(len(cs[4])) if plan(cs, cs[5][0], i)[1] is not None}
        assert len(fs) >= 2, f"{name}: at least two items must get different factors, got {fs}"
    tiny = case("g_tiny37")
    assert {v for i in range(37) for v in plan(tiny, "linear", i)[0]} == set(range(1, 12)), "g_tiny37: factors 1..11"
    np.savez_compressed(OUT, **pack(results))
    print(OUT, os.path.getsize(OUT), "bytes,", len(results), "entries,", reduced, "reduced, Pillow", PIL.__version__)
    fx = np.load(OUT)
    for (key, _, _, _), (incrc, out, red, pl) in zip(entries(), results):
        e = expected(fx, key)
        assert e[0] == incrc and e[1] == crc(out)
        assert (expected_reduce(fx, key) is None) == (red is None) and recorded_plan(fx, key) == pl


if __name__ == "__main__":
    main()
