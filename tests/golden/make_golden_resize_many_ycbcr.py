"""Fixture for resize_many_ycbcr (subsampled YCbCr planes to an RGB batch): tests/golden/resize_many_ycbcr.npz.

Run by hand (needs Pillow; no GPU):  python tests/golden/make_golden_resize_many_ycbcr.py

Per case of CASES and filter, the expected [N, oH, oW, 3] uint8 batch under the key "<case>/<filter>", made with Pillow alone:

    b  = box or (0, 0, W, H)                                   float32 values
    cb = (b[0] / sx, b[1] / sy, b[2] / sx, b[3] / sy)           float32 division
    r  = lambda p, bx: Image.fromarray(p, "L").resize((vw, vh), FILTER, box=bx)
    rgb = Image.merge("YCbCr", [r(Y, b), r(Cb, cb), r(Cr, cb)]).convert("RGB")

pasted by numpy slicing at the item's offset into a canvas of the fill colour and mirrored left to right where the item flips.  The
planes are regenerated from seeds (planes()), never stored.  "ycc_sha256" is the sha256 of Pillow's RGB bytes for all 2^24 YCbCr
triples laid out as a 4096 x 4096 image in C order of [y, cb, cr].  main() asserts that the "clamp" case clamps: from Pillow's resized
planes alone, at least 5 % of its output channels have a pre-clamp value below 0 and at least 5 % one above 255.
"""
from __future__ import annotations

import hashlib
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "resize_many_ycbcr.npz")

_spec = importlib.util.spec_from_file_location("make_golden_box_reduce", os.path.join(HERE, "make_golden_box_reduce.py"))
_br = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_br)
make_batch = _br.make_batch

FILTER_NAMES = ("linear", "cubic", "box", "hamming", "lanczos")
SUBSAMPLING = {"444": (1, 1), "422": (2, 1), "420": (2, 2), "440": (1, 2)}
VROWS, VCOLS = 4, 256  # what a workgroup of the converting vertical pass covers (csrc/aa_many_ycbcr.h)

_P = (23, 31)
# name -> items [(H, W, subsampling, box (x0, y0, x1, y1) or None)], canvas (oh, ow), filters, and where given sizes [(vh, vw)], offsets
# [(py, px)] or "center", fill (R, G, B), flips; kind "clamp": planes of near-black / near-white luma under extreme chroma
CASES = {
    # Y of 1 x 1 and 2 x 2 (chroma 1 x 1), up and to one pixel
    "tiny": dict(items=[(1, 1, "420", None), (2, 2, "420", None)], canvas=(2, 3), filters=("linear", "cubic")),
    "tiny1": dict(items=[(1, 1, "420", None), (2, 2, "420", None)], canvas=(1, 1), filters=("linear", "lanczos")),
    "frac": dict(items=[(7, 9, "420", (1.25, 0.5, 8.5, 6.75))], canvas=(3, 5), filters=FILTER_NAMES),
    # odd sizes, down and up, one column past the horizontal strip of 64 and of 128
    "odd65": dict(items=[(37, 53, "420", None), (37, 53, "420", (3.3, 2.2, 52.9, 36.1))], canvas=(5, 65), filters=("linear", "lanczos")),
    "odd129": dict(items=[(33, 47, "420", None)], canvas=(40, 129), filters=("cubic", "hamming")),
    # one pixel wider, and one row more, than a workgroup of the vertical pass covers; the source is three rows high
    "vwide": dict(items=[(3, 40, "420", None)], canvas=(VROWS + 1, VCOLS + 1), filters=("linear",)),
    # long Lanczos windows: 901 luma and 451 chroma taps down a column; along a row 1547 luma and 775 chroma taps, and the windows of a
    # strip of 64 outputs together beyond the 8 KiB the horizontal pass stages at once, for the luma and for the chroma plane
    "long": dict(items=[(600, 9, "420", None), (5, 17000, "420", None)], canvas=(4, 66), filters=("lanczos",),
                 sizes=[(4, 6), (3, 66)], fill=(1, 2, 3)),
    "s422": dict(items=[_P + ("422", (2.5, 1.25, 30.0, 22.5))], canvas=(11, 17), filters=("linear", "cubic")),
    "s440": dict(items=[_P + ("440", (2.5, 1.25, 30.0, 22.5))], canvas=(11, 17), filters=("linear", "cubic")),
    "s444": dict(items=[_P + ("444", (2.5, 1.25, 30.0, 22.5))], canvas=(11, 17), filters=("linear", "cubic")),
    "mixed": dict(items=[_P + ("444", None), (22, 30, "422", (1.5, 0.0, 29.0, 21.5)), _P + ("420", None), (24, 31, "440", None), (9, 8, "420", None)],
                  canvas=(13, 19), filters=("cubic", "box")),
    # overhang on all four sides, padding, an item wholly off the canvas, one pixel in the last corner, an RGB fill, half the items flipped
    "placed": dict(items=[(37, 53, "420", None), (37, 53, "420", (3.3, 2.2, 52.9, 36.1)), (22, 30, "422", None), (24, 31, "440", None),
                          (9, 8, "420", None), (9, 8, "444", None)], canvas=(30, 45), filters=("cubic", "linear"),
                   sizes=[(40, 60), (20, 70), (25, 20), (12, 50), (6, 6), (1, 1)], offsets=[(-5, -8), (15, -50), (-10, 30), (3, -2), (100, 3), (29, 44)],
                   fill=(9, 250, 77), flips=[True, False, True, False, True, False]),
    "center": dict(items=[(37, 53, "420", None), (22, 30, "422", None), (33, 47, "420", None)], canvas=(28, 28), filters=("linear",),
                   sizes=[(32, 43), (20, 33), (28, 28)], offsets="center", fill=(114, 114, 114), flips=[False, True, True]),
    "clamp": dict(items=[(33, 47, "420", None)], canvas=(40, 129), filters=("cubic",), kind="clamp"),
}
_SEEDS = {name: 300 + k for k, name in enumerate(CASES)}


def keys():
    return [f"{name}/{f}" for name, cs in CASES.items() for f in cs["filters"]]


def chroma_shape(h, w, sub):
    sx, sy = SUBSAMPLING[sub]
    return -(-h // sy), -(-w // sx)


def chroma_box(box, h, w, sub):
    """The recipe's cb: the luma box (or the whole plane) in float32 over the subsampling, in float32."""
    sx, sy = SUBSAMPLING[sub]
    b = [np.float32(v) for v in (box if box is not None else (0, 0, w, h))]
    return tuple(float(v) for v in (b[0] / np.float32(sx), b[1] / np.float32(sy), b[2] / np.float32(sx), b[3] / np.float32(sy)))


def planes(name, i):
    """(Y [H, W], Cb [h, w], Cr [h, w]) uint8 of item i of a case, from seeds."""
    cs = CASES[name]
    h, w, sub, _ = cs["items"][i]
    ch, cw = chroma_shape(h, w, sub)
    seed = 10 * _SEEDS[name] + i
    if cs.get("kind") == "clamp":
        rng = np.random.default_rng(seed)
        # blocks of near-black / near-white luma, chroma at either extreme: most pixels leave 0..255 on some channel
        yb = rng.integers(0, 2, (-(-h // 3), -(-w // 3))).repeat(3, 0).repeat(3, 1)[:h, :w]
        y = np.where(yb == 1, 255 - rng.integers(0, 9, (h, w)), rng.integers(0, 9, (h, w))).astype(np.uint8)
        c = []
        for _ in range(2):
            b = rng.integers(0, 2, (-(-ch // 2), -(-cw // 2))).repeat(2, 0).repeat(2, 1)[:ch, :cw]
            c.append(np.where(b == 1, 255 - rng.integers(0, 16, (ch, cw)), rng.integers(0, 16, (ch, cw))).astype(np.uint8))
        return y, c[0], c[1]
    return (np.ascontiguousarray(make_batch((1, 1, h, w), 3 * seed)[0, 0]), np.ascontiguousarray(make_batch((1, 1, ch, cw), 3 * seed + 1)[0, 0]),
            np.ascontiguousarray(make_batch((1, 1, ch, cw), 3 * seed + 2)[0, 0]))


def center_offset(v, o):
    return -int(round((v - o) / 2.0)) if v >= o else (o - v) // 2


def places(name):
    """[(vh, vw, py, px)] per item."""
    cs = CASES[name]
    oh, ow = cs["canvas"]
    out = []
    for i in range(len(cs["items"])):
        vh, vw = cs["sizes"][i] if cs.get("sizes") else (oh, ow)
        offs = cs.get("offsets")
        py, px = (center_offset(vh, oh), center_offset(vw, ow)) if offs == "center" else (offs[i] if offs else (0, 0))
        out.append((vh, vw, py, px))
    return out


def compose(name, results):
    """The items' [vh, vw, 3] RGB results -> the [N, oh, ow, 3] batch: pasted, filled, mirrored."""
    cs = CASES[name]
    oh, ow = cs["canvas"]
    fill = cs.get("fill") or (0, 0, 0)
    batch = np.empty((len(results), oh, ow, 3), np.uint8)
    batch[:] = np.array(fill, np.uint8)
    for i, (r, (vh, vw, py, px)) in enumerate(zip(results, places(name))):
        assert r.shape == (vh, vw, 3)
        y0, y1, x0, x1 = max(0, py), min(oh, py + vh), max(0, px), min(ow, px + vw)
        if y1 > y0 and x1 > x0:
            batch[i, y0:y1, x0:x1] = r[y0 - py:y1 - py, x0 - px:x1 - px]
        if cs.get("flips") and cs["flips"][i]:
            batch[i] = batch[i, :, ::-1]
    return batch


def pillow_planes(name, f, i):
    """Pillow's three resized planes of one item, [vh, vw] uint8 each."""
    from PIL import Image

    flt = {"linear": Image.BILINEAR, "cubic": Image.BICUBIC, "box": Image.BOX, "hamming": Image.HAMMING, "lanczos": Image.LANCZOS}[f]
    h, w, sub, box = CASES[name]["items"][i]
    vh, vw = places(name)[i][:2]
    y, cb, cr = planes(name, i)
    cbox = chroma_box(box, h, w, sub)
    r = lambda p, bx: Image.fromarray(p, "L").resize((vw, vh), flt, box=bx)  # noqa: E731
    return r(y, box), r(cb, cbox), r(cr, cbox)


def pillow(name, f):
    from PIL import Image

    return compose(name, [np.asarray(Image.merge("YCbCr", list(pillow_planes(name, f, i))).convert("RGB"))
                          for i in range(len(CASES[name]["items"]))])


def all_triples():
    """The 2^24 YCbCr triples as a [4096, 4096, 3] image, C order of [y, cb, cr]."""
    v = np.arange(256, dtype=np.uint8)
    t = np.empty((256, 256, 256, 3), np.uint8)
    t[..., 0], t[..., 1], t[..., 2] = v[:, None, None], v[None, :, None], v[None, None, :]
    return t.reshape(4096, 4096, 3)


def clamp_shares(name="clamp", f="cubic"):
    """(share of output channels below 0 before the clamp, share above 255), from Pillow's resized planes and the matrix in floats."""
    y, cb, cr = (np.asarray(p).astype(np.float64) for p in pillow_planes(name, f, 0))
    pre = np.stack([y + 1.402 * (cr - 128), y - 0.34414 * (cb - 128) - 0.71414 * (cr - 128), y + 1.772 * (cb - 128)])
    return float((pre < -1).mean()), float((pre > 256).mean())  # (a margin of one: beyond any rounding of the integer form)


def main() -> None:
    import PIL
    from PIL import Image

    lo, hi = clamp_shares()
    assert lo >= 0.05 and hi >= 0.05, (lo, hi)
    out = {k: pillow(*k.split("/")) for k in keys()}
    sha = hashlib.sha256(np.asarray(Image.fromarray(all_triples(), "YCbCr").convert("RGB")).tobytes()).hexdigest()
    out["ycc_sha256"] = np.frombuffer(sha.encode(), np.uint8)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes,", len(out) - 1, "entries, Pillow", PIL.__version__, f"clamp case: {lo:.1%} below 0, {hi:.1%} above 255")
    print("sha256 of all triples:", sha)


if __name__ == "__main__":
    main()
