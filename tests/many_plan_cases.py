"""Shared by the frozen-plan test and its generator (tests/golden/make_golden_many_plans.py): every plan the host planners of the ragged
calls write for the cases of the ragged fixtures, through the C-ABI with fake device pointers (a plan is host arithmetic: the pointers
are never dereferenced), and a handful of literal error inputs per planner.  plans() yields (key, rc, workspace bytes, descriptor
bytes); the block is a zero-initialised buffer and the planners memset their records, so the bytes are deterministic.  Nothing here
says what a plan should hold: tests/golden/many_plans.json records what the planners wrote before they were restructured.  Not a test
module."""
import ctypes
import struct

from kit_golden import generator as gen  # the generator module of one ragged fixture: its CASES are the cases enumerated here

from interpolate_antialiasing_amd import _lib, boxmath

LAYOUTS = (("nhwc", _lib.NHWC), ("nchw", _lib.NCHW))
KMAX = (2 ** 31 - 1) // 4
FLIP, ALPHA = _lib.MANY_FLIP_X, _lib.MANY_PREMUL_ALPHA


def _lie(r, layout, c, h, w, eb=1):
    """Where a record's image lies: in `layout`'s class, with a row pitch beyond the row and a plane pitch beyond the plane."""
    r.H, r.W = h, w
    if layout == _lib.NHWC:
        r.stride_row, r.stride_px, r.stride_ch = (w * c + 5) * eb, c * eb, 1
    else:
        r.stride_row, r.stride_px, r.stride_ch = (w + 3) * eb, eb, (h * (w + 3) + 1) * eb


def images(layout, c, items, flags=None, eb=1):
    """items [(H, W, box or None, ...)] -> aa_many_image records."""
    recs = (_lib.ManyImage * max(len(items), 1))()
    for i, it in enumerate(items):
        r = recs[i]
        r.data_dev = 4096 + 256 * i
        _lie(r, layout, c, it[0], it[1], eb)
        if it[2] is not None:
            r.has_box = 1
            r.box[0], r.box[1], r.box[2], r.box[3] = it[2]
        r.flags = flags[i] if flags is not None else 0
    return recs


def _places(places):
    if places is None:
        return None
    precs = (_lib.ManyPlace * max(len(places), 1))()
    for i, p in enumerate(places):
        precs[i].vH, precs[i].vW, precs[i].oy, precs[i].ox = p
    return precs


def _planned(nbytes, call, tail=lambda: b""):
    """call(block address, block bytes, byref(workspace bytes)) -> (rc, workspace bytes, the block's bytes + what else the plan reports)."""
    buf = (ctypes.c_uint8 * max(nbytes, 1))()
    ws = ctypes.c_size_t(0)
    rc = call(ctypes.addressof(buf), nbytes, ctypes.byref(ws))
    return rc, ws.value, bytes(buf) + tail()


def plan_many(f, layout, c, oh, ow, recs, n, places=None, fill=None, nbytes=None):
    """aa_many_plan (no places, no fill) or aa_many_plan_placed."""
    L = _lib.load()
    fid = _lib.FILTER_IDS[f] if isinstance(f, str) else f
    if places is None and fill is None:
        return _planned(L.aa_many_desc_bytes(n) if nbytes is None else nbytes,
                        lambda b, nb, ws: L.aa_many_plan(fid, layout, n, c, oh, ow, recs, b, nb, ws))
    fl = None if fill is None else (ctypes.c_uint8 * 4)(*(list(fill) + [0] * (4 - len(fill))))
    return _planned(L.aa_many_desc_bytes_placed(n) if nbytes is None else nbytes,
                    lambda b, nb, ws: L.aa_many_plan_placed(fid, layout, n, c, oh, ow, recs, _places(places), fl, b, nb, ws))


def plan_patches(f, layout, c, patch, recs, n, sizes, pad_to=0, nbytes=None):
    """aa_many_plan_patches; the rows it reports follow the block."""
    L = _lib.load()
    flat = (ctypes.c_int64 * max(2 * len(sizes), 1))(*[v for s in sizes for v in s])
    rows = ctypes.c_int64(-1)
    return _planned(L.aa_many_desc_bytes_patches(n) if nbytes is None else nbytes,
                    lambda b, nb, ws: L.aa_many_plan_patches(_lib.FILTER_IDS[f], layout, n, c, patch[0], patch[1], recs, flat, pad_to, b, nb, ws,
                                                             ctypes.byref(rows)),
                    lambda: struct.pack("<q", rows.value))


def plan_nearest(layout, eb, c, oh, ow, recs, n, places=None, fill=None, nbytes=None):
    """aa_many_plan_nearest."""
    L = _lib.load()
    cf = None if fill is None else (ctypes.c_int32 * 4)(*(list(fill) + [0] * (4 - len(fill))))
    return _planned(L.aa_many_desc_bytes_nearest(n) if nbytes is None else nbytes,
                    lambda b, nb, ws: L.aa_many_plan_nearest(layout, eb, n, c, oh, ow, recs, _places(places), cf, b, nb, ws))


def plan_maps(f, elem, oh, ow, recs, n, places=None, fill=0.0, overflow=0, nbytes=None):
    """aa_many_plan_maps."""
    L = _lib.load()
    fid = _lib.FILTER_IDS[f] if isinstance(f, str) else f
    return _planned(L.aa_many_desc_bytes_maps(max(n, 0)) if nbytes is None else nbytes,
                    lambda b, nb, ws: L.aa_many_plan_maps(fid, elem, n, oh, ow, recs, _places(places), fill, overflow, b, nb, ws))


def ycc_images(items, interleaved, flags=None):
    """items [(H, W, subsampling, box or None)] -> aa_ycbcr_image records: every plane's pitch beyond its row; interleaved pairs are one
    plane of 2-byte pixels, Cr one byte after Cb at the same pitch."""
    sub = gen("resize_many_ycbcr").SUBSAMPLING
    recs = (_lib.YccImage * max(len(items), 1))()
    for i, (h, w, ss, box) in enumerate(items):
        r = recs[i]
        sx, sy = sub[ss]
        r.H, r.W, r.cH, r.cW = h, w, -(-h // sy), -(-w // sx)
        r.y_dev, r.cb_dev = (1 << 20) + 65536 * i, (1 << 24) + 65536 * i
        r.y_stride_row = w + 3
        if interleaved:
            r.cr_dev, r.chroma_stride_px = r.cb_dev + 1, 2
            r.cb_stride_row = r.cr_stride_row = 2 * r.cW + 6
        else:
            r.cr_dev, r.chroma_stride_px = (1 << 25) + 65536 * i, 1
            r.cb_stride_row, r.cr_stride_row = r.cW + 3, r.cW + 5
        r.subsampling = _lib.YCC_SUBSAMPLING[ss]
        if box is not None:
            r.has_box = 1
            r.box[0], r.box[1], r.box[2], r.box[3] = box
        r.flags = flags[i] if flags is not None else 0
    return recs


def plan_ycbcr(f, oh, ow, recs, n, places=None, fill=None, nbytes=None):
    """aa_many_plan_ycbcr."""
    L = _lib.load()
    fid = _lib.FILTER_IDS[f] if isinstance(f, str) else f
    fl = None if fill is None else (ctypes.c_uint8 * 3)(*fill)
    return _planned(L.aa_many_desc_bytes_ycbcr(n) if nbytes is None else nbytes,
                    lambda b, nb, ws: L.aa_many_plan_ycbcr(fid, n, oh, ow, recs, _places(places), fl, b, nb, ws))


def reduce_items(layout, c, items):
    """items [(H, W, integer box, (fx, fy))] -> aa_reduce_item records."""
    recs = (_lib.ReduceItem * max(len(items), 1))()
    for i, (h, w, box, (fx, fy)) in enumerate(items):
        r = recs[i]
        r.data_dev = (1 << 20) + 4096 * i
        _lie(r, layout, c, h, w)
        r.box[0], r.box[1], r.box[2], r.box[3] = box
        r.fx, r.fy = fx, fy
    return recs


def plan_reduce(layout, c, recs, n, nbytes=None):
    """aa_reduce_many_plan; the workspace is the arena, and the items' offsets into it follow the block."""
    L = _lib.load()
    offs = (ctypes.c_int64 * max(n, 1))()
    return _planned(L.aa_reduce_many_desc_bytes(n) if nbytes is None else nbytes,
                    lambda b, nb, ws: L.aa_reduce_many_plan(layout, n, c, recs, b, nb, ws, offs), lambda: bytes(offs))


def _case_plans():
    for name, c, (oh, ow), items, filters, _, _ in gen("resize_many").CASES:
        for f in filters:
            for ln, layout in LAYOUTS:
                yield f"many/{name}/{f}/{ln}", plan_many(f, layout, c, oh, ow, images(layout, c, items), len(items))
    for name, c, (oh, ow), fill, filters, items, _, _ in gen("resize_many_placed").CASES:
        for f in filters:
            for ln, layout in LAYOUTS:
                yield f"placed/{name}/{f}/{ln}", plan_many(f, layout, c, oh, ow, images(layout, c, items), len(items),
                                                           [it[3] + it[4] for it in items], fill)
    for name, c, patch, filters, items, _, _ in gen("resize_many_patches").CASES:
        sizes = [it[3] for it in items]
        flags = [FLIP if it[4] else 0 for it in items]
        longest = max((vh // patch[0]) * (vw // patch[1]) for vh, vw in sizes)
        for f in filters:
            for ln, layout in LAYOUTS:
                for pad_to in (0, longest + 3):
                    yield (f"patches/{name}/{f}/{ln}/{'pad' if pad_to else 'packed'}",
                           plan_patches(f, layout, c, patch, images(layout, c, items, flags), len(items), sizes, pad_to))
    for name, c, (oh, ow), fill, filters, items, _, placed in gen("resize_many_alpha").CASES:
        flags = [ALPHA | (FLIP if i % 2 else 0) for i in range(len(items))]
        for f in filters:
            for ln, layout in LAYOUTS:
                yield f"alpha/{name}/{f}/{ln}", plan_many(f, layout, c, oh, ow, images(layout, c, items, flags), len(items),
                                                          [it[3] + it[4] for it in items] if placed else None, fill if placed else None)
    g = gen("resize_many_nearest")
    for cs in g.CASES:
        name, dt, c, (oh, ow), fill, items, flips = cs[:7]
        eb = {"u1": 1, "i2": 2, "i4": 4}[dt]
        geo = [g.geometry(cs, i) for i in range(len(items))]
        flags = [FLIP if flips is not None and flips[i] else 0 for i in range(len(items))]
        # (places only where the case has sizes, offsets or "center": the others plan without them, as the Python call does)
        places = [q[3] + q[4] for q in geo] if cs[7] or any(len(it) > 3 for it in items) else None
        for ln, layout in LAYOUTS:
            yield f"nearest/{name}/{ln}", plan_nearest(layout, eb, c, oh, ow, images(layout, c, geo, flags, eb), len(items), places, fill)
    for name, c, out, gap, items, filters, _, _, sizes, _ in gen("reduce_many").CASES:
        for f in filters:
            plans = boxmath.reducing_plans([it[:2] for it in items], out, f, [it[2] for it in items], sizes, gap)
            reduced = [(items[i][0], items[i][1], p[1], p[0]) for i, p in enumerate(plans) if p is not None]
            for ln, layout in LAYOUTS:
                yield f"reduce/{name}/{f}/{ln}", plan_reduce(layout, c, reduce_items(layout, c, reduced), len(reduced))
    g = gen("resize_many_maps")
    for name, cs in g.CASES.items():
        (oh, ow), n = cs["canvas"], len(cs["items"])
        geo = [g.geometry(cs, i) for i in range(n)]
        flags = [FLIP if cs.get("flips") is not None and cs["flips"][i] else 0 for i in range(n)]
        places = [q[3] + q[4] for q in geo] if cs.get("placed") else None
        for dt in cs["dtypes"]:
            elem, eb = {"u16": (_lib.MAPS_U16, 2), "i32": (_lib.MAPS_I32, 4), "f32": (_lib.MAPS_F32, 4)}[dt]
            fill = float(g.FILLS[dt]) if cs.get("placed") else 0.0
            for f in cs["filters"]:
                for on, over in sorted(_lib.MAPS_OVERFLOW.items()) if dt == "u16" else [("pillow", 0)]:
                    yield (f"maps/{name}/{f}/{dt}" + (f"/{on}" if dt == "u16" else ""),
                           plan_maps(f, elem, oh, ow, images(_lib.NCHW, 1, geo, flags, eb), n, places, fill, over))
    g = gen("resize_many_ycbcr")
    for name, cs in g.CASES.items():
        (oh, ow), n = cs["canvas"], len(cs["items"])
        flags = [FLIP if cs.get("flips") and cs["flips"][i] else 0 for i in range(n)]
        places = g.places(name) if cs.get("sizes") or cs.get("offsets") else None
        for f in cs["filters"]:
            for an, il in (("planar", False), ("interleaved", True)):
                yield f"ycbcr/{name}/{f}/{an}", plan_ycbcr(f, oh, ow, ycc_images(cs["items"], il, flags), n, places, cs.get("fill"))


def _error_plans():
    """Literal bad inputs, a few per planner: what comes back and what the block holds by then."""
    N, ok = _lib.NHWC, [(20, 30, None), (9, 11, (1.5, 2.0, 10.0, 8.5))]

    def strided(recs, **kw):
        for k, v in kw.items():
            setattr(recs[1], k, v)
        return recs

    many = lambda **kw: plan_many(**{**dict(f="linear", layout=N, c=3, oh=10, ow=12, recs=images(N, 3, ok), n=2), **kw})  # noqa: E731
    yield "err/many/ok", many()
    yield "err/many/place_size", many(places=[(7, 9, 0, 0), (0, 9, 0, 0)])
    yield "err/many/place_offset", many(places=[(7, 9, 0, 0), (7, 9, 0, -KMAX - 1)])
    yield "err/many/place_off_canvas", many(places=[(7, 9, KMAX, -KMAX), (7, 9, 1, 2)], fill=(1, 2, 3))
    yield "err/many/box_beyond", many(recs=images(N, 3, [ok[0], (9, 11, (0, 0, 12, 9))]))
    yield "err/many/box_empty", many(recs=images(N, 3, [ok[0], (9, 11, (5, 5, 5, 8))]))
    yield "err/many/box_nan", many(recs=images(N, 3, [ok[0], (9, 11, (0, 0, float("nan"), 9))]))
    yield "err/many/box_full_is_none", many(recs=images(N, 3, [ok[0], (9, 11, (0, 0, 11, 9))]))
    yield "err/many/stride_px", many(recs=strided(images(N, 3, ok), stride_px=4))
    yield "err/many/stride_ch", many(recs=strided(images(N, 3, ok), stride_ch=2))
    yield "err/many/stride_planar", many(layout=_lib.NCHW)
    yield "err/many/short_block", many(nbytes=_lib.load().aa_many_desc_bytes(2) - 1)
    yield "err/many/short_placed_block", many(places=[(7, 9, 0, 0)] * 2, nbytes=_lib.load().aa_many_desc_bytes(2))
    yield "err/many/flag_bit", many(recs=images(N, 3, ok, [0, 4]))
    yield "err/many/flag_alpha_c3", many(recs=images(N, 3, ok, [0, ALPHA]))
    yield "err/many/flag_before_strides", many(recs=strided(images(N, 3, ok, [0, 8]), stride_px=4))
    yield "err/many/null_image", many(recs=strided(images(N, 3, ok), data_dev=None))
    yield "err/many/size", many(recs=images(N, 3, [ok[0], (KMAX + 1, 11, None)]))
    yield "err/many/ksize", plan_many("lanczos", N, 3, 10, 10, images(N, 3, [(20000, 30, None)]), 1, [(1, 10, 0, 0)])
    yield "err/many/filter", many(f=7)

    pt = lambda **kw: plan_patches(**{**dict(f="linear", layout=N, c=3, patch=(2, 3), recs=images(N, 3, ok), n=2,  # noqa: E731
                                             sizes=[(4, 6), (2, 9)]), **kw})
    yield "err/patches/ok", pt()
    yield "err/patches/size_indivisible", pt(sizes=[(4, 6), (2, 10)])
    yield "err/patches/pad_to_short", pt(pad_to=3)
    yield "err/patches/box_beyond", pt(recs=images(N, 3, [ok[0], (9, 11, (0, 0, 12, 9))]))
    yield "err/patches/stride_px", pt(recs=strided(images(N, 3, ok), stride_px=4))
    yield "err/patches/short_block", pt(nbytes=_lib.load().aa_many_desc_bytes_placed(2))
    yield "err/patches/flag_alpha", plan_patches("linear", N, 4, (2, 3), images(N, 4, ok, [0, ALPHA]), 2, [(4, 6), (2, 9)])

    P = _lib.NCHW
    near = lambda **kw: plan_nearest(**{**dict(layout=P, eb=1, c=3, oh=10, ow=12, recs=images(P, 3, ok), n=2), **kw})  # noqa: E731
    yield "err/nearest/ok", near()
    yield "err/nearest/place_size", near(places=[(7, 9, 0, 0), (7, KMAX + 1, 0, 0)])
    yield "err/nearest/place_off_canvas", near(places=[(5, 5, 100, 100), (7, 9, -2, 3)], fill=(255, -128, 0))
    yield "err/nearest/box_beyond", near(recs=images(P, 3, [ok[0], (9, 11, (-1, 0, 11, 9))]))
    yield "err/nearest/box_empty", near(recs=images(P, 3, [ok[0], (9, 11, (5, 5, 5, 8))]))
    yield "err/nearest/stride_px", near(recs=strided(images(P, 3, ok), stride_px=3))
    yield "err/nearest/stride_class", near(layout=N)
    yield "err/nearest/unaligned_data", near(eb=2, c=1, recs=strided(images(P, 1, ok, eb=2), data_dev=4097))
    yield "err/nearest/unaligned_row", near(eb=4, c=1, recs=strided(images(P, 1, ok, eb=4), stride_row=14 * 4 + 2))
    yield "err/nearest/strides_before_box", near(eb=2, c=1, recs=strided(images(P, 1, [ok[0], (9, 11, (5, 5, 5, 8))], eb=2), data_dev=4097))
    yield "err/nearest/short_block", near(nbytes=_lib.load().aa_many_desc_bytes_nearest(2) - 1)
    yield "err/nearest/flag_alpha", near(recs=images(P, 3, ok, [FLIP, ALPHA]))
    yield "err/nearest/fill_range", near(fill=(0, 256, 0))
    yield "err/nearest/elem_bytes", near(eb=3)

    rok = [(20, 30, (0, 0, 30, 20), (2, 2)), (9, 11, (1, 2, 10, 8), (3, 1))]
    red = lambda **kw: plan_reduce(**{**dict(layout=N, c=3, recs=reduce_items(N, 3, rok), n=2), **kw})  # noqa: E731
    yield "err/reduce/ok", red()
    yield "err/reduce/box_beyond", red(recs=reduce_items(N, 3, [rok[0], (9, 11, (0, 0, 12, 9), (2, 2))]))
    yield "err/reduce/box_empty", red(recs=reduce_items(N, 3, [rok[0], (9, 11, (5, 5, 5, 8), (2, 2))]))
    yield "err/reduce/factor", red(recs=reduce_items(N, 3, [rok[0], (9, 11, (0, 0, 11, 9), (0, 2))]))
    yield "err/reduce/factor_before_strides", red(recs=strided(reduce_items(N, 3, [rok[0], (9, 11, (0, 0, 11, 9), (257, 256))]), stride_px=4))
    yield "err/reduce/stride_px", red(recs=strided(reduce_items(N, 3, rok), stride_px=4))
    yield "err/reduce/stride_planar", red(layout=P)
    yield "err/reduce/null_image", red(recs=strided(reduce_items(N, 3, rok), data_dev=None))
    yield "err/reduce/short_block", red(nbytes=_lib.load().aa_reduce_many_desc_bytes(2) - 1)

    U, F = _lib.MAPS_U16, _lib.MAPS_F32
    maps = lambda **kw: plan_maps(**{**dict(f="linear", elem=U, oh=10, ow=12, recs=images(P, 1, ok, eb=2), n=2), **kw})  # noqa: E731
    fmaps = lambda **kw: maps(**{**dict(elem=F, recs=images(P, 1, ok, eb=4)), **kw})  # noqa: E731
    yield "err/maps/ok", maps()
    yield "err/maps/n_negative", maps(n=-1)
    yield "err/maps/null_images", maps(recs=None)
    yield "err/maps/elem", maps(elem=3)
    yield "err/maps/overflow", maps(overflow=2)
    yield "err/maps/fill_nan", fmaps(fill=float("nan"))
    yield "err/maps/fill_inf", fmaps(fill=float("inf"))
    yield "err/maps/fill_beyond_f32", fmaps(fill=1e39)
    yield "err/maps/fill_fraction_u16", maps(fill=1.5)
    yield "err/maps/fill_65536_u16", maps(fill=65536.0)
    yield "err/maps/place_size", maps(places=[(7, 9, 0, 0), (0, 9, 0, 0)])
    yield "err/maps/short_block", maps(nbytes=_lib.load().aa_many_desc_bytes_maps(2) - 1)
    yield "err/maps/box_beyond", maps(recs=images(P, 1, [ok[0], (9, 11, (0, 0, 12, 9))], eb=2))
    yield "err/maps/box_empty", maps(recs=images(P, 1, [ok[0], (9, 11, (5, 5, 5, 8))], eb=2))
    yield "err/maps/unaligned_data", maps(recs=strided(images(P, 1, ok, eb=2), data_dev=4097))
    yield "err/maps/unaligned_row", fmaps(recs=strided(images(P, 1, ok, eb=4), stride_row=14 * 4 + 2))
    yield "err/maps/flag_alpha", maps(recs=images(P, 1, ok, [FLIP, ALPHA], eb=2))
    yield "err/maps/ksize", plan_maps("lanczos", U, 10, 10, images(P, 1, [(20000, 30, None)], eb=2), 1, [(1, 10, 0, 0)])

    yok = [(20, 30, "420", None), (9, 11, "420", (1.5, 2.0, 10.0, 8.5))]
    ycc = lambda il=False, **kw: plan_ycbcr(**{**dict(f="linear", oh=10, ow=12, recs=ycc_images(yok, il), n=2), **kw})  # noqa: E731
    yield "err/ycbcr/ok", ycc()
    yield "err/ycbcr/ok_interleaved", ycc(True)
    yield "err/ycbcr/null_plane", ycc(recs=strided(ycc_images(yok, False), cb_dev=None))
    yield "err/ycbcr/subsampling", ycc(recs=strided(ycc_images(yok, False), subsampling=4))
    yield "err/ycbcr/chroma_height", ycc(recs=strided(ycc_images(yok, False), cH=6))
    yield "err/ycbcr/other_arrangement", ycc(recs=strided(ycc_images(yok, False), chroma_stride_px=2))
    yield "err/ycbcr/cr_not_beside_cb", ycc(recs=strided(ycc_images(yok, True), cr_dev=(1 << 24) + 65536 + 2))
    yield "err/ycbcr/n_beyond", ycc(n=KMAX // 3 + 1, nbytes=_lib.load().aa_many_desc_bytes_ycbcr(2))
    yield "err/ycbcr/short_block", ycc(nbytes=_lib.load().aa_many_desc_bytes_ycbcr(2) - 1)
    yield "err/ycbcr/flag_alpha", ycc(recs=ycc_images(yok, False, [FLIP, ALPHA]))


def plans():
    """-> (key, rc, workspace bytes, descriptor bytes) of every plan."""
    for key, (rc, ws, block) in _case_plans():
        yield key, rc, ws, block
    for key, (rc, ws, block) in _error_plans():
        yield key, rc, ws, block
