"""Shared by the resize_many_ycbcr tests: the fixture generator (tests/golden/make_golden_resize_many_ycbcr.py), the fixture it made with
Pillow (tests/golden/resize_many_ycbcr.npz), and a numpy restatement of the call: every plane through the per-plane restatement of
Pillow's "L" resize that the placed tests use (resize_many_placed_ref.gen()'s resize_box_restated), then the table conversion.
Not a test module."""
import functools

import numpy as np

import kit_golden
import resize_many_placed_ref as placed_ref

gen = functools.partial(kit_golden.generator, "resize_many_ycbcr")
fixture = functools.partial(kit_golden.fixture, "resize_many_ycbcr")


def expected(name, f):
    """The fixture's [N, oh, ow, 3] batch of a case under a filter (read-only)."""
    a = fixture()[f"{name}/{f}"]
    a.setflags(write=False)
    return a


def stored_sha256():
    return fixture()["ycc_sha256"].tobytes().decode()


@functools.lru_cache(maxsize=None)
def planes(name, i):
    """(Y, Cb, Cr) of item i of a case (read-only: shared between tests)."""
    ps = gen().planes(name, i)
    for p in ps:
        p.setflags(write=False)
    return ps


def call_args(name):
    """The keyword arguments of aa.resize_many_ycbcr for a case (everything but images, output_size and mode)."""
    cs = gen().CASES[name]
    kw = dict(subsampling=[it[2] for it in cs["items"]], boxes=[it[3] for it in cs["items"]])
    for k in ("sizes", "offsets", "fill", "flips"):
        if cs.get(k) is not None:
            kw[k] = cs[k] if isinstance(cs[k], str) else list(cs[k])
    return kw


# ---- the restatement --------------------------------------------------------------------------------------------------------------------------
def tables():
    """Pillow's four tables from their definition: C's (int)(c * 64 * (v - 128) + 0.5), which truncates towards zero."""
    return [np.array([int(c * 64 * (v - 128) + 0.5) for v in range(256)], np.int32) for c in (1.402, -0.34414, -0.71414, 1.772)]


def convert(y, cb, cr):
    """uint8 arrays of one shape -> [..., 3] RGB by the tables (>> on negative numpy ints is the arithmetic shift)."""
    r_cr, g_cb, g_cr, b_cb = tables()
    yi = y.astype(np.int32)
    rgb = np.stack([yi + (r_cr[cr] >> 6), yi + ((g_cb[cb] + g_cr[cr]) >> 6), yi + (b_cb[cb] >> 6)], axis=-1)
    return np.clip(rgb, 0, 255).astype(np.uint8)


def restate_item(f, y, cb, cr, sub, box, vh, vw):
    """One item's [vh, vw, 3] RGB: three "L" resizes, then the conversion."""
    g = gen()
    rs = placed_ref.gen()._rm.resize_box_restated
    cbox = g.chroma_box(box, y.shape[0], y.shape[1], sub)
    r = lambda p, bx: rs(f, np.ascontiguousarray(p)[:, :, None], vh, vw, bx)[:, :, 0]  # noqa: E731
    return convert(r(y, box), r(cb, cbox), r(cr, cbox))


def restate(name, f):
    """The [N, oh, ow, 3] batch of a case from the restatement."""
    g = gen()
    cs = g.CASES[name]
    res = []
    for i, (h, w, sub, box) in enumerate(cs["items"]):
        vh, vw = g.places(name)[i][:2]
        res.append(restate_item(f, *planes(name, i), sub, box, vh, vw))
    return g.compose(name, res)
