"""Fixture for Image.reduce, Image.resize(box=...) and Image.resize(reducing_gap=...): tests/golden/box_reduce.npz.

Run by hand (needs Pillow; no GPU):  python tests/golden/make_golden_box_reduce.py

Holds, for every case of REDUCE_CASES, BOX_CASES and GAP_CASES below (and every filter of a case), Pillow's own output as a CRC-32 of
the whole [N, oH, oW, C] array and up to 256 sampled pixels, and the CRC-32 of the input, which make_batch() regenerates from its seed.
Expected outputs only: the file stays small.

The functions below restate, in numpy and plain Python, what the package computes on the GPU: ImagingReduce's 8-bit arithmetic,
precompute_coeffs with a box, ImagingResample's two passes, and Image.resize's reducing_gap logic (Image._get_safe_box included).  They
import nothing but numpy, math and the sibling make_golden_filters.py, so the tests load them as well.  main() asserts that the
restatement reproduces Pillow bit for bit on every fixture entry.
"""
from __future__ import annotations

import importlib.util
import math
import os
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "box_reduce.npz")

_spec = importlib.util.spec_from_file_location("make_golden_filters", os.path.join(HERE, "make_golden_filters.py"))
_gf = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_gf)

PRECISION_BITS = 22
FILTER_NAMES = ("linear", "cubic", "box", "hamming", "lanczos")
SUPPORT = {"linear": 1.0, "cubic": 2.0, "box": 0.5, "hamming": 1.0, "lanczos": 3.0}


def _bilinear(x: float) -> float:
    if x < 0.0:
        x = -x
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _box(x: float) -> float:
    return 1.0 if -0.5 < x <= 0.5 else 0.0


FILTER_FN = {"linear": _bilinear, "cubic": _bicubic, "box": _box, "hamming": _gf.hamming, "lanczos": _gf.lanczos}


# ---- Image.reduce ---------------------------------------------------------------------------------------------------
def reduce_mult(n: int) -> int:
    """Pillow's division_UINT32(n, 8): (UINT32)(2^32 as float / (float)(256 * n)), a float32 division."""
    return int(np.float32(4294967296.0) / np.float32(256 * n))


def reduce_restated(img: np.ndarray, factor, box=None) -> np.ndarray:
    """HWC uint8 -> Image.reduce(factor, box): ((ss + n // 2) * mult(n)) >> 24 in unsigned 32-bit arithmetic, n = the pixels really in
    the block (the last row / column of blocks is clipped to the box)."""
    fx, fy = factor
    h, w = img.shape[:2]
    x0, y0, x1, y1 = box if box is not None else (0, 0, w, h)
    a = img[y0:y1, x0:x1].astype(np.uint64)
    bh, bw = a.shape[:2]
    oh, ow = (bh + fy - 1) // fy, (bw + fx - 1) // fx
    ys, xs = np.arange(0, bh, fy), np.arange(0, bw, fx)
    ss = np.add.reduceat(np.add.reduceat(a, ys, axis=0), xs, axis=1)
    ny = np.minimum(fy, bh - ys)[:, None, None]
    nx = np.minimum(fx, bw - xs)[None, :, None]
    n = (ny * nx).astype(np.uint64)
    mult = np.vectorize(reduce_mult, otypes=[np.uint64])(n)
    out = (((ss + n // 2) * mult) & np.uint64(0xFFFFFFFF)) >> np.uint64(24)
    assert out.shape[:2] == (oh, ow)
    return out.astype(np.uint8)


# ---- precompute_coeffs with a box ------------------------------------------------------------------------------------
def box_coeffs(name: str, in_size: int, in0: float, in1: float, out_size: int):
    """Pillow's precompute_coeffs(inSize, in0, in1, outSize) + normalize_coeffs_8bpc -> (ksize, xmin[out], xsize[out], int32 k[out, ksize])."""
    f = FILTER_FN[name]
    scale = float(np.float32(in1 - in0)) / out_size  # (in0, in1 are floats in Pillow's C: a float difference)
    filterscale = max(scale, 1.0)
    support = SUPPORT[name] * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    xmin_a = np.zeros(out_size, np.int32)
    xsize_a = np.zeros(out_size, np.int32)
    kd = np.zeros((out_size, ksize), np.float64)
    ss = 1.0 / filterscale
    for i in range(out_size):
        center = in0 + (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        ww = 0.0
        for x in range(xmax):
            w = f((x + xmin - center + 0.5) * ss)
            kd[i, x] = w
            ww += w
        for x in range(xmax):
            if ww != 0.0:
                kd[i, x] /= ww
        xmin_a[i], xsize_a[i] = xmin, xmax
    ki = np.where(kd < 0, np.trunc(-0.5 + kd * (1 << PRECISION_BITS)), np.trunc(0.5 + kd * (1 << PRECISION_BITS))).astype(np.int32)
    return ksize, xmin_a, xsize_a, ki


def resize_box_restated(name: str, img: np.ndarray, oh: int, ow: int, box=None) -> np.ndarray:
    """HWC uint8 -> Pillow's C resize with a box (x0, y0, x1, y1): a crop when the box has integer offsets and the output's size, else
    ImagingResample: horizontal pass first; a pass runs unless the size stays AND the box spans the whole axis."""
    h, w = img.shape[:2]
    x0, y0, x1, y1 = (float(np.float32(v)) for v in box) if box is not None else (0.0, 0.0, float(w), float(h))  # (the C takes floats)
    if x0 == int(x0) and y0 == int(y0) and x1 - x0 == ow and y1 - y0 == oh:
        return img[int(y0):int(y0) + oh, int(x0):int(x0) + ow].copy()
    out = img
    if ow != w or x0 != 0 or x1 != w:
        _, xmin, xsize, k = box_coeffs(name, w, x0, x1, ow)
        out = _gf._pass_u8(out, 1, xmin, xsize, k)
    if oh != h or y0 != 0 or y1 != h:
        _, xmin, xsize, k = box_coeffs(name, h, y0, y1, oh)
        out = _gf._pass_u8(out, 0, xmin, xsize, k)
    return out


# ---- Image.resize's reducing_gap (its Python, restated) ----------------------------------------------------------------
def safe_box(width: int, height: int, out_w: int, out_h: int, name: str, box):
    """Image._get_safe_box."""
    s = SUPPORT[name] - 0.5
    scale_x = (box[2] - box[0]) / out_w
    scale_y = (box[3] - box[1]) / out_h
    sx, sy = s * scale_x, s * scale_y
    return (max(0, int(box[0] - sx)), max(0, int(box[1] - sy)), min(width, math.ceil(box[2] + sx)), min(height, math.ceil(box[3] + sy)))


def gap_plan(width: int, height: int, out_w: int, out_h: int, name: str, box, gap: float):
    """-> (factor, reduce box or None, box for the resize that follows), as Image.resize computes them."""
    fx = int((box[2] - box[0]) / out_w / gap) or 1
    fy = int((box[3] - box[1]) / out_h / gap) or 1
    if fx > 1 or fy > 1:
        rb = safe_box(width, height, out_w, out_h, name, box)
        return (fx, fy), rb, ((box[0] - rb[0]) / fx, (box[1] - rb[1]) / fy, (box[2] - rb[0]) / fx, (box[3] - rb[1]) / fy)
    return (fx, fy), None, tuple(box)


def resize_restated(name: str, img: np.ndarray, oh: int, ow: int, box=None, gap=None) -> np.ndarray:
    """HWC uint8 -> Image.resize((ow, oh), filter, box, reducing_gap)."""
    h, w = img.shape[:2]
    bx = tuple(float(v) for v in box) if box is not None else (0.0, 0.0, float(w), float(h))
    if (w, h) == (ow, oh) and bx == (0.0, 0.0, float(w), float(h)):
        return img.copy()
    if gap is not None:
        factor, rb, bx = gap_plan(w, h, ow, oh, name, bx, gap)
        if rb is not None:
            img = reduce_restated(img, factor, rb)
    return resize_box_restated(name, img, oh, ow, bx)


def axis_hull_from_coeffs(xmin: np.ndarray, xsize: np.ndarray):
    return int(xmin.min()), int((xmin + xsize).max())


# ---- alpha (Pillow's RGBA <-> RGBa, LA <-> La) -------------------------------------------------------------------------
def premultiply(img: np.ndarray) -> np.ndarray:
    a = img[..., -1:].astype(np.uint32)
    t = img[..., :-1].astype(np.uint32) * a + 128
    out = img.copy()
    out[..., :-1] = (((t >> 8) + t) >> 8).astype(np.uint8)
    return out


def unpremultiply(img: np.ndarray) -> np.ndarray:
    a = img[..., -1:].astype(np.uint32)
    c = img[..., :-1].astype(np.uint32)
    q = np.minimum(255, (255 * c) // np.maximum(a, 1))
    out = img.copy()
    out[..., :-1] = np.where((a == 0) | (a == 255), c, q).astype(np.uint8)
    return out


# ---- fixture inputs ----------------------------------------------------------------------------------------------------
def make_batch(shape, seed: int, fill=None) -> np.ndarray:
    """[N, C, H, W] uint8: make_golden_filters.make_image per batch item (noise with hard 0 / 255 edges), or a constant."""
    n, c, h, w = shape
    if fill is not None:
        return np.full(shape, fill, np.uint8)
    return np.stack([_gf.make_image(h, w, c, 1000 * seed + i).transpose(2, 0, 1) for i in range(n)])


def crc(a: np.ndarray) -> int:
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def sample_pixels(npx: int) -> np.ndarray:
    return np.unique(np.linspace(0, npx - 1, min(npx, 256)).round().astype(np.int64))


# ---- the cases ---------------------------------------------------------------------------------------------------------
REDUCE_FACTORS = [(2, 2), (3, 3), (8, 4), (5, 1), (1, 7), (3, 5)]
# (name, shape, seed, fill, factor, box, alpha)
REDUCE_CASES = []
for _c in (3, 1, 4, 2):
    for _f in REDUCE_FACTORS:
        REDUCE_CASES.append((f"r_c{_c}_{_f[0]}x{_f[1]}", (2, _c, 37, 53), 10 + _c, None, _f, None, False))
for _f in REDUCE_FACTORS:
    REDUCE_CASES.append((f"r_box_{_f[0]}x{_f[1]}", (2, 3, 37, 53), 13, None, _f, (5, 7, 50, 36), False))
REDUCE_CASES += [
    ("r_wide", (1, 3, 16, 2051), 20, None, (2, 4), None, False),
    ("r_tall", (1, 1, 1500, 7), 21, None, (1, 3), None, False),
    ("r_all255", (1, 3, 37, 53), 0, 255, (7, 9), None, False),
    ("r_all0", (1, 3, 37, 53), 0, 0, (7, 9), None, False),
    ("r_n22500", (1, 1, 300, 300), 22, None, (150, 150), None, False),
    ("r_rgba", (2, 4, 37, 53), 23, None, (3, 2), None, True),
    ("r_la", (2, 2, 37, 53), 24, None, (3, 2), None, True),
]

BOX1 = (10.3, 7.6, 120.9, 90.2)
# (name, shape, seed, out (H, W), box, filters, alpha)
BOX_CASES = [
    ("b_down_c3", (2, 3, 97, 131), 31, (30, 40), BOX1, FILTER_NAMES, False),
    ("b_down_c1", (2, 1, 97, 131), 32, (30, 40), BOX1, FILTER_NAMES, False),
    ("b_down_c4", (2, 4, 97, 131), 33, (30, 40), BOX1, FILTER_NAMES, False),
    ("b_same", (2, 3, 97, 131), 31, (97, 131), (0.5, 0.25, 130.5, 96.75), FILTER_NAMES, False),
    ("b_int_up", (2, 3, 97, 131), 31, (64, 64), (30, 20, 62, 52), FILTER_NAMES, False),
    ("b_near1", (2, 3, 97, 131), 31, (61, 61), (10, 10, 70.5, 70.5), FILTER_NAMES, False),
    ("b_border", (2, 3, 97, 131), 31, (29, 33), (3.7, 0, 131, 50.5), FILTER_NAMES, False),
    ("b_xfull", (2, 3, 97, 131), 31, (30, 40), (0, 7.6, 131, 90.2), FILTER_NAMES, False),
    ("b_wide", (1, 3, 64, 1700), 34, (20, 20), (50.5, 2, 1650.5, 60), ("cubic",), False),
    ("b_split", (1, 3, 64, 600), 35, (20, 12), (10.5, 2, 590.5, 60), ("cubic",), False),
    ("b_headline", (2, 3, 438, 906), 36, (196, 320), (20.5, 10.25, 880.0, 420.5), FILTER_NAMES, False),
    ("b_rgba", (2, 4, 97, 131), 33, (30, 40), BOX1, ("linear", "lanczos"), True),
]

# (name, shape, seed, out (H, W), box, gap, filters)
GAP_CASES = []
for _g in (1.0, 2.0, 3.0):
    GAP_CASES.append((f"g_full_{_g}", (2, 3, 300, 411), 41, (30, 40), None, _g, FILTER_NAMES))
    GAP_CASES.append((f"g_box_{_g}", (2, 3, 300, 411), 41, (30, 40), (20.5, 10.25, 400, 290), _g, FILTER_NAMES))
GAP_CASES += [
    ("g_fx15", (1, 3, 64, 900), 42, (32, 30), None, 2.0, FILTER_NAMES),
    ("g_ones", (1, 3, 97, 131), 43, (60, 80), None, 2.0, FILTER_NAMES),
]


def entries():
    """Every (key, kind, case, filter) of the fixture, in the order its arrays are packed."""
    for cs in REDUCE_CASES:
        yield cs[0], "reduce", cs, None
    for cs in BOX_CASES:
        for f in cs[5]:
            yield f"{cs[0]}/{f}", "box", cs, f
    for cs in GAP_CASES:
        for f in cs[6]:
            yield f"{cs[0]}/{f}", "gap", cs, f


def case_input(kind: str, cs) -> np.ndarray:
    return make_batch(cs[1], cs[2], cs[3] if kind == "reduce" else None)


def restated(kind: str, cs, f, x: np.ndarray) -> np.ndarray:
    """[N, C, H, W] -> the expected [N, oH, oW, C] of one entry, from the restatement."""
    outs = []
    for img in x.transpose(0, 2, 3, 1):
        if kind == "reduce":
            if cs[6]:
                outs.append(unpremultiply(reduce_restated(premultiply(img), cs[4], cs[5])))
            else:
                outs.append(reduce_restated(img, cs[4], cs[5]))
        elif kind == "box":
            oh, ow = cs[3]
            if cs[6]:
                outs.append(unpremultiply(resize_box_restated(f, premultiply(img), oh, ow, cs[4])))
            else:
                outs.append(resize_box_restated(f, img, oh, ow, cs[4]))
        else:
            oh, ow = cs[3]
            outs.append(resize_restated(f, img, oh, ow, cs[4], cs[5]))
    return np.stack(outs)


def pillow(kind: str, cs, f, x: np.ndarray) -> np.ndarray:
    """The same entry from Pillow itself."""
    from PIL import Image

    flt = {"linear": Image.BILINEAR, "cubic": Image.BICUBIC, "box": Image.BOX, "hamming": Image.HAMMING, "lanczos": Image.LANCZOS}
    alpha = cs[6] if kind != "gap" else False

    def run(im):
        if kind == "reduce":
            return im.reduce(cs[4], box=cs[5])
        oh, ow = cs[3]
        return im.resize((ow, oh), flt[f], box=cs[4], reducing_gap=cs[5] if kind == "gap" else None)

    outs = []
    for img in x.transpose(0, 2, 3, 1):
        c = img.shape[2]
        mode = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}[c]
        if c == 3 or alpha:
            outs.append(np.asarray(run(Image.fromarray(np.ascontiguousarray(img), mode))))
        else:  # 1, 2 and 4 plain channels: per-channel "L" images (LA / RGBA would premultiply)
            outs.append(np.stack([np.asarray(run(Image.fromarray(np.ascontiguousarray(img[:, :, ch]), "L"))) for ch in range(c)], axis=-1))
    return np.stack(outs)


def expected(fx, key: str):
    """-> (CRC-32 of the input, CRC-32 of Pillow's [N, oH, oW, C] output, its pixels at sample_pixels() [n, C])."""
    keys = [e[0] for e in entries()]
    i = keys.index(key)
    crcs, counts, samples = fx["crcs"], fx["sample_counts"], fx["samples"]
    off = int(counts[:i].sum())
    c = int(fx["channels"][i])
    return int(crcs[i, 0]), int(crcs[i, 1]), samples[off:off + int(counts[i])].reshape(-1, c)


def pack(results):
    """results: [(input crc, output array [N, oH, oW, C])] in entries() order -> the fixture's arrays."""
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
    results = []
    cache = {}
    for key, kind, cs, f in entries():
        ck = (cs[1], cs[2], cs[3] if kind == "reduce" else None)
        if ck not in cache:
            cache[ck] = case_input(kind, cs)
        x = cache[ck]
        pil = pillow(kind, cs, f, x)
        mine = restated(kind, cs, f, x)
        assert np.array_equal(mine, pil), f"the restatement differs from Pillow: {key}"
        results.append((crc(x), pil))
        print(key, pil.shape, flush=True)
    np.savez_compressed(OUT, **pack(results))
    print(OUT, os.path.getsize(OUT), "bytes")
    fx = np.load(OUT)
    for (key, _, _, _), (incrc, out) in zip(entries(), results):
        e = expected(fx, key)
        assert e[0] == incrc and e[1] == crc(out)


if __name__ == "__main__":
    main()
