"""Shared by the ragged calls' edge tests: the fixture generator (tests/golden/make_golden_resize_many_edges.py) and the fixture it made
with Pillow (tests/golden/resize_many_edges.npz), loaded once; item inputs regenerated from their seeds and the restatement's bytes, once
each, and left unchanged; the tile sizes of the kernels read out of their source text, and the work units they imply for a case, worked
out from the restatement's coefficients.  Nothing here calls the code under test.  Not a test module."""
import functools
import os
import re

import numpy as np

import kit_golden
from kit_golden import MODE  # noqa: F401

CSRC = os.path.join(kit_golden.ROOT, "interpolate_antialiasing_amd", "csrc")
gen = functools.partial(kit_golden.generator, "resize_many_edges")
fixture = functools.partial(kit_golden.fixture, "resize_many_edges")


def br():
    """make_golden_box_reduce: box_coeffs, resize_box_restated."""
    return gen()._rm._br


@functools.lru_cache(maxsize=None)
def _expected_index():
    return {e[0]: i for i, e in enumerate(gen().entries())}


def case(name):
    return gen().case(name)


def classes(names):
    """[(case, layout class)]: one channel is planar only."""
    return [(name, cls) for name in names for cls in (("planar",) if case(name).c == 1 else ("interleaved", "planar"))]


@functools.lru_cache(maxsize=None)
def item(name, i):
    """[C, H, W] uint8 input of item i of case `name` (read-only: shared between tests)."""
    return kit_golden.readonly(gen().item_input(case(name), i))


@functools.lru_cache(maxsize=None)
def restated(name, f, i):
    """The expected [oH, oW, C] bytes of one item from the CPU restatement (read-only: shared between tests)."""
    return kit_golden.readonly(gen().restated(case(name), f, i, item(name, i)))


@functools.lru_cache(maxsize=None)
def restated_batch(name, f):
    """The same for the whole case: [N, C, oH, oW] (read-only)."""
    y = np.stack([restated(name, f, i).transpose(2, 0, 1) for i in range(len(case(name).items))])
    y.setflags(write=False)
    return y


def kw(name):
    """The keyword arguments of the call for a case: its boxes, and a placed case's sizes, offsets and fill."""
    cs = case(name)
    d = {"boxes": [it[2] for it in cs.items]}
    if cs.kind == "placed":
        d.update(sizes=[it[3] for it in cs.items], offsets=[it[4] for it in cs.items], fill=list(cs.fill))
    return d


def expected(key):
    """-> (input CRC-32, output CRC-32, sampled pixels [n, C]) of one fixture entry."""
    fx = fixture()
    i = _expected_index()[key]
    counts = fx["sample_counts"]
    off = int(counts[:i].sum())
    c = int(fx["channels"][i])
    return int(fx["crcs"][i, 0]), int(fx["crcs"][i, 1]), fx["samples"][off:off + int(counts[i])].reshape(-1, c)


def assert_matches_fixture(key, x_chw, got_hwc):
    """got_hwc [oH, oW, C] equals the expected array of fixture entry `key`: the input is the fixture's (CRC-32), the sampled pixels are
    Pillow's (they say where a mismatch lies) and the whole array has the fixture's CRC-32."""
    kit_golden.assert_sampled(key, gen(), *expected(key), x_chw, got_hwc)


# ---- the tile sizes, from the source text ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def constants():
    """AA_MANY_STRIP, AA_MANY_VBYTES and aa_many_vpixels of csrc/aa_many.h, kChunkDwords and the kChunkCols expression of
    csrc/aa_many.hip, by regular expressions on the text: -> {"STRIP", "VBYTES", "CHUNK_DWORDS", "VPIXELS": {E: pixels}}."""
    with open(os.path.join(CSRC, "aa_many.h")) as f:
        h = f.read()
    with open(os.path.join(CSRC, "aa_many.hip")) as f:
        hip = f.read()

    def one(pattern, text, what):
        m = re.search(pattern, text)
        assert m, f"{what} is no longer written as this helper reads it: {pattern}"
        return m

    strip = int(one(r"#define\s+AA_MANY_STRIP\s+(\d+)", h, "AA_MANY_STRIP").group(1))
    vbytes = int(one(r"#define\s+AA_MANY_VBYTES\s+(\d+)", h, "AA_MANY_VBYTES").group(1))
    m = one(r"aa_many_vpixels\(int E\)\s*\{\s*return\s+E == 1 \? (\d+) : \(E == 2 \? (\d+) : (\d+)\);", h, "aa_many_vpixels")
    p1, p2, p34 = (int(v) for v in m.groups())
    dwords = int(one(r"constexpr int kChunkDwords = (\d+);", hip, "kChunkDwords").group(1))
    one(r"constexpr int kChunkBytes = 4 \* kChunkDwords;", hip, "kChunkBytes")
    one(r"constexpr int kChunkCols = \(kChunkBytes - 4\) / E;", hip, "kChunkCols")
    return {"STRIP": strip, "VBYTES": vbytes, "CHUNK_DWORDS": dwords, "VPIXELS": {1: p1, 2: p2, 3: p34, 4: p34}}


def chunk_cols(e):
    """kChunkCols of many_hpass<E>: the input columns of one staged chunk."""
    return (4 * constants()["CHUNK_DWORDS"] - 4) // e


def elem_bytes(c, cls):
    """E: the bytes per pixel of a row in the layout class."""
    return c if cls == "interleaved" else 1


def vstrips(ow, e):
    """Work units of many_vpass per output row."""
    vb = constants()["VBYTES"]
    return (ow * e + vb - 1) // vb


def pieces(ow, e):
    """Work units of many_vpass_float per output row."""
    px = constants()["VPIXELS"][e]
    return (ow + px - 1) // px


@functools.lru_cache(maxsize=None)
def axis(name, f, i, ax):
    """One axis (0 vertical, 1 horizontal) of item i as the planner sees it, from the restatement's coefficients: -> None for an item off
    the canvas, else (origin of the hull, hull, ksize, xmin relative to the origin [m], xsize [m], d) where the m table entries are
    the covered outputs [v0, v0 + m) of the item's own size and d is where they land on the output axis."""
    cs = case(name)
    it = cs.items[i]
    h, w, box = it[:3]
    in_size = (h, w)[ax]
    bx = tuple(float(np.float32(v)) for v in box) if box is not None else (0.0, 0.0, float(w), float(h))
    in0, in1 = (bx[1], bx[3]) if ax == 0 else (bx[0], bx[2])
    o = cs.out[ax]
    v, p = (o, 0) if cs.kind == "plain" else (it[3][ax], it[4][ax])
    v0, v1 = max(0, -p), min(v, o - p)
    if cs.kind == "placed":  # off the canvas on either axis: no table at all
        for a in (0, 1):
            if min(it[3][a], cs.out[a] - it[4][a]) <= max(0, -it[4][a]):
                return None
    k, xmin, xsize, _ = br().box_coeffs(f, in_size, in0, in1, v)
    xmin, xsize = xmin[v0:v1].astype(np.int64), xsize[v0:v1].astype(np.int64)
    lo, hi = int(xmin[0]), int(xmin[-1] + xsize[-1])
    assert lo == int(xmin.min()) and hi == int((xmin + xsize).max())
    return lo, hi - lo, k, xmin - lo, xsize, v0 + p


def hstrip_segments(name, f, i):
    """[(seg0, seg1)] per strip of AA_MANY_STRIP covered output columns of item i, relative to the hull's origin, as many_hpass computes
    them: the first window's start and the last window's end, clipped to the hull."""
    a = axis(name, f, i, 1)
    if a is None:
        return []
    _, hull, _, xmin, xsize, _ = a
    s = constants()["STRIP"]
    segs = []
    for x0 in range(0, len(xmin), s):
        x1 = min(x0 + s, len(xmin))
        segs.append((max(int(xmin[x0]), 0), min(int(xmin[x1 - 1] + xsize[x1 - 1]), hull)))
    return segs


def hstrip_chunks(name, f, i, e):
    """Chunks each horizontal strip of item i is staged in."""
    cc = chunk_cols(e)
    return [(s1 - s0 + cc - 1) // cc for s0, s1 in hstrip_segments(name, f, i)]


def window_chunks(name, f, i, e, x):
    """The chunks (indices within its strip) in which table entry x of item i has taps."""
    _, _, _, xmin, xsize, _ = axis(name, f, i, 1)
    s0, s1 = hstrip_segments(name, f, i)[x // constants()["STRIP"]]
    cc = chunk_cols(e)
    lo, hi = max(int(xmin[x]), s0), min(int(xmin[x] + xsize[x]), s1)
    return list(range((lo - s0) // cc, (hi - 1 - s0) // cc + 1))


def hunits(name, f, cls):
    """Work units of the horizontal pass over the whole case: planes x hull rows x strips, per item."""
    cs = case(name)
    planes = 1 if cls == "interleaved" else cs.c
    total = 0
    for i in range(len(cs.items)):
        a = axis(name, f, i, 0)
        if a is not None:
            total += planes * a[1] * len(hstrip_segments(name, f, i))
    return total


def where(name, f, cls, got_nchw, want_nchw):
    """None if the two [N, C, oH, oW] uint8 arrays are equal, else a sentence on the first wrong byte in the output's own memory order:
    its item, plane, row and byte of the row, the work unit of the vertical pass that wrote it, and the work unit and staged chunks of
    the horizontal pass behind it."""
    cs = case(name)
    got, want = np.asarray(got_nchw), np.asarray(want_nchw)
    if got.shape != want.shape:
        return f"{name}/{f}/{cls}: shape {got.shape}, expected {want.shape}"
    if cls == "interleaved":  # memory order [N, oH, oW, C]
        g, w = got.transpose(0, 2, 3, 1), want.transpose(0, 2, 3, 1)
    else:
        g, w = got, want
    bad = np.argwhere(g != w)
    if bad.size == 0:
        return None
    e = elem_bytes(cs.c, cls)
    if cls == "interleaved":
        n, y, x, ch = (int(v) for v in bad[0])
        plane, b = 0, x * e + ch
    else:
        n, plane, y, x = (int(v) for v in bad[0])
        ch, b = plane, x
    vb = constants()["VBYTES"]
    msg = (f"{name}/{f}/{cls}: {len(bad)} of {g.size} bytes differ from Pillow's; the first is item {n}, plane {plane}, row {y}, column {x}, channel {ch}: "
           f"{int(g[tuple(bad[0])])} != {int(w[tuple(bad[0])])}; byte {b} of its row = vertical strip {b // vb}, lane {b % vb // 4}, byte {b % 4} "
           f"of the lane's dword; converting-pass piece {x // constants()['VPIXELS'][e]}")
    a = axis(name, f, n, 1)
    if a is None:
        return msg + "; the item lies off the canvas (all fill)"
    t = x - a[5]  # the table entry behind canvas column x
    if 0 <= t < len(a[3]):
        s = t // constants()["STRIP"]
        s0, s1 = hstrip_segments(name, f, n)[s]
        msg += (f"; table entry {t} = horizontal strip {s} (segment [{s0}, {s1}) of the hull from column {a[0]}, {hstrip_chunks(name, f, n, e)[s]} chunk(s) "
                f"of {chunk_cols(e)} columns), window [{int(a[3][t])}, {int(a[3][t] + a[4][t])}) with taps in chunk(s) {window_chunks(name, f, n, e, t)}")
    else:
        msg += f"; the column lies beside the item's covered columns [{a[5]}, {a[5] + len(a[3])}) (fill)"
    return msg
