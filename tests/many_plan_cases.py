"""Shared by the frozen-plan test and its generator (tests/golden/make_golden_many_plans.py): every plan the host planners of the ragged
calls write for the cases of the ragged fixtures, through the C-ABI with fake device pointers (a plan is host arithmetic: the pointers
are never dereferenced), for the float ragged calls (embed, back, merged, back_bwd) the cases of their CPU restatements
(resize_embed_ref.py, resize_many_back*_ref.py), and literal error inputs per planner.  plans() yields (key, rc, workspace bytes, descriptor
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


# ---- the float ragged calls: one position grid to N token grids, canvas predictions back to N sizes (merged or not), its backward ------
FILTERS5 = ("linear", "cubic", "box", "hamming", "lanczos")
# (reduce, out_dtype) as aa_back_many_plan takes them: values a float, argmax a label, greater a byte
BACK_OUT = ([("values", _lib.BACK_VALUES, n, d) for n, d in (("f32", _lib.F32), ("f16", _lib.F16), ("bf16", _lib.BF16))] +
            [("argmax", _lib.BACK_ARGMAX, n, d) for n, d in (("u8", _lib.U8), ("i16", _lib.I16), ("i32", _lib.I32), ("i64", _lib.I64))] +
            [("greater", _lib.BACK_GREATER, n, d) for n, d in (("bool", _lib.BOOL), ("u8", _lib.U8))])


def _fid(f):
    return _lib.FILTER_IDS[f] if isinstance(f, str) else f


def _or_null(null, **named):
    """The named arguments, None for those listed in `null`."""
    return [None if k in null else v for k, v in named.items()]


def plan_embed(f, d, h0, w0, grids, pad_to=0, n=None, nbytes=None, null=()):
    """aa_embed_many_plan; the rows it reports follow the block."""
    L = _lib.load()
    n = len(grids) if n is None else n
    flat = (ctypes.c_int64 * max(2 * len(grids), 1))(*[v for g in grids for v in g])
    rows = ctypes.c_int64(-1)

    def call(b, nb, ws):
        flat_, b_, ws_, rows_ = _or_null(null, grids=flat, desc=b, ws=ws, rows=ctypes.byref(rows))
        return L.aa_embed_many_plan(_fid(f), n, d, h0, w0, flat_, pad_to, b_, nb, ws_, rows_)
    return _planned(L.aa_embed_many_desc_bytes(max(n, 0)) if nbytes is None else nbytes, call, lambda: struct.pack("<q", rows.value))


def back_items(layout, k, geo, ptr=1 << 20):
    """geo [((H, W) of the source, (y0, x0, h, w) or None, (oh, ow), flip)] -> aa_back_item records of dense [K, H, W] sources in
    `layout`'s class, data_dev at the region's corner."""
    recs = (_lib.BackItemIn * max(len(geo), 1))()
    for i, ((hh, ww), region, (oh, ow), flip) in enumerate(geo):
        y0, x0, h, w = (0, 0, hh, ww) if region is None else region
        r = recs[i]
        r.stride_ch, r.stride_row, r.stride_px = (1, ww * k, k) if layout == _lib.NHWC else (hh * ww, ww, 1)
        r.data_dev = ptr + 65536 * i + 4 * (y0 * r.stride_row + x0 * r.stride_px)
        r.h, r.w, r.oh, r.ow, r.flags = h, w, oh, ow, FLIP if flip else 0
    return recs


def _two_sizes(call, nbytes, n_offs):
    """A planner that reports a second size and n_offs offsets besides the block: both follow the block."""
    second = ctypes.c_size_t(0)
    offs = (ctypes.c_int64 * max(n_offs, 1))()
    return _planned(nbytes, lambda b, nb, ws: call(b, nb, ws, second, offs), lambda: struct.pack("<Q", second.value) + bytes(offs))


def plan_back(f, layout, k, recs, n, reduce=_lib.BACK_VALUES, out_dtype=_lib.F32, nbytes=None, null=()):
    """aa_back_many_plan; the arena's bytes and the items' offsets into it follow the block."""
    L = _lib.load()

    def call(b, nb, ws, arena, offs):
        recs_, b_, ws_, arena_, offs_ = _or_null(null, items=recs, desc=b, ws=ws, arena=ctypes.byref(arena), offs=offs)
        return L.aa_back_many_plan(_fid(f), layout, n, k, recs_, reduce, out_dtype, b_, nb, ws_, arena_, offs_)
    return _two_sizes(call, L.aa_back_many_desc_bytes(max(n, 0)) if nbytes is None else nbytes, n)


def plan_merged(f, layout, k, recs, n, groups, g, merge=0, reduce=_lib.BACK_VALUES, out_dtype=_lib.F32, nbytes=None, null=()):
    """aa_back_merged_plan; the arena's bytes and the groups' offsets into it follow the block."""
    L = _lib.load()
    group_of = (ctypes.c_int64 * max(len(groups), 1))(*groups)

    def call(b, nb, ws, arena, offs):
        recs_, group_, b_, ws_, arena_, offs_ = _or_null(null, items=recs, groups=group_of, desc=b, ws=ws, arena=ctypes.byref(arena), offs=offs)
        return L.aa_back_merged_plan(_fid(f), layout, n, k, recs_, g, group_, merge, reduce, out_dtype, b_, nb, ws_, arena_, offs_)
    return _two_sizes(call, L.aa_back_merged_desc_bytes(max(n, 0), max(g, 0)) if nbytes is None else nbytes, g)


def back_bwd_items(k, geo, ptr=1 << 20):
    """geo [((H, W) of the canvas, (y0, x0, h, w) or None, (oh, ow), flip, has a gradient)] -> aa_back_bwd_item records of dense
    [K, oh, ow] gradients; an item without one has grad_dev None and nothing but its canvas."""
    recs = (_lib.BackBwdItemIn * max(len(geo), 1))()
    for i, ((hh, ww), region, (oh, ow), flip, has) in enumerate(geo):
        r = recs[i]
        r.H, r.W = hh, ww
        if has:
            r.grad_dev = ptr + 65536 * i
            r.stride_ch, r.stride_row = oh * ow, ow
            r.y0, r.x0, r.h, r.w = (0, 0, hh, ww) if region is None else region
            r.oh, r.ow, r.flags = oh, ow, FLIP if flip else 0
    return recs


def plan_back_bwd(f, layout, k, recs, n, out_dtype=_lib.F32, dense=0, nbytes=None, null=()):
    """aa_back_many_bwd_plan; the output's bytes and the items' offsets into it follow the block."""
    L = _lib.load()

    def call(b, nb, ws, out, offs):
        recs_, b_, ws_, out_, offs_ = _or_null(null, items=recs, desc=b, ws=ws, out=ctypes.byref(out), offs=offs)
        return L.aa_back_many_bwd_plan(_fid(f), layout, n, k, recs_, out_dtype, dense, b_, nb, ws_, out_, offs_)
    return _two_sizes(call, L.aa_back_many_bwd_desc_bytes(max(n, 0)) if nbytes is None else nbytes, n)


def _float_case_plans():
    import resize_embed_ref as embed_ref
    import resize_many_back_bwd_ref as bwd_ref
    import resize_many_back_merged_ref as merged_ref
    import resize_many_back_ref as back_ref

    for name, (h0, w0), grids in [("base", embed_ref.BASE_SOURCE, embed_ref.BASE_GRIDS)] + [(k,) + v for k, v in embed_ref.FURTHER.items()]:
        longest = max(gh * gw for gh, gw in grids)
        for f in FILTERS5:
            for pad_to in (0, longest + 3):
                for d in (8, 523):
                    yield f"embed/{name}/{f}/{'pad' if pad_to else 'packed'}/d{d}", plan_embed(f, d, h0, w0, grids, pad_to)

    def batch(canvas, regions, sizes):  # every item a region of its own slice of one [N, K, H, W] batch
        return canvas.shape[1], [(tuple(canvas.shape[2:]), r, s, i % 2 == 1) for i, (r, s) in enumerate(zip(regions, sizes))]

    srcs, regions, sizes = back_ref.list_case()
    back_cases = {"base": batch(back_ref.BASE_CANVAS, back_ref.BASE_REGIONS, back_ref.BASE_SIZES), "k300": batch(*back_ref.k300_case()),
                  "seventy": batch(*back_ref.seventy_case()),
                  "list": (3, [(tuple(s.shape[1:]), r, z, i % 2 == 1) for i, (s, r, z) in enumerate(zip(srcs, regions, sizes))])}
    for name, (k, geo) in back_cases.items():
        for f in FILTERS5:
            for ln, layout in LAYOUTS:
                for rn, reduce, dn, dt in BACK_OUT:
                    if reduce == _lib.BACK_ARGMAX and k > {_lib.U8: 256, _lib.I16: 32768}.get(dt, k):
                        continue  # (a label type that cannot hold K - 1: not a pair the planner accepts)
                    yield f"back/{name}/{f}/{ln}/{rn}/{dn}", plan_back(f, layout, k, back_items(layout, k, geo), len(geo), reduce, dt)

    def members(canvas, regions, groups, sizes, flips):  # every member at its GROUP's size
        shapes = [tuple(s.shape[1:]) for s in canvas] if isinstance(canvas, list) else [tuple(canvas.shape[2:])] * len(groups)
        k = canvas[0].shape[0] if isinstance(canvas, list) else canvas.shape[1]
        return k, [(shapes[i], regions[i], sizes[g], flips[i]) for i, g in enumerate(groups)], groups, len(sizes)

    c, regions, groups, sizes = merged_ref.k300_case()
    merged_cases = {"base": members(merged_ref.BASE_CANVAS, merged_ref.BASE_REGIONS, merged_ref.BASE_GROUPS, merged_ref.BASE_SIZES,
                                    merged_ref.BASE_FLIPS),
                    "k300": members(c, regions, groups, sizes, [False, True]), "seventy": members(*merged_ref.seventy_case()),
                    "list": members(*merged_ref.list_case())}
    for name, (k, geo, groups, g) in merged_cases.items():
        for f in FILTERS5:
            for ln, layout in LAYOUTS:
                for mn, merge in sorted(_lib.BACK_MERGE.items()):
                    for rn, reduce, dt in (("values", _lib.BACK_VALUES, _lib.F32), ("argmax", _lib.BACK_ARGMAX, _lib.I64),
                                           ("greater", _lib.BACK_GREATER, _lib.BOOL)):
                        yield (f"merged/{name}/{f}/{ln}/{mn}/{rn}",
                               plan_merged(f, layout, k, back_items(layout, k, geo), len(geo), groups, g, merge, reduce, dt))

    def canvases(canvas, regions, sizes, flips=None):
        cv = bwd_ref.canvases_of(canvas, len(sizes))
        return [(cv[i], regions[i], sizes[i], flips[i] if flips is not None else i % 2 == 1) for i in range(len(sizes))]

    bwd_cases = {"base": (bwd_ref.BASE_K, canvases(bwd_ref.BASE_HW, bwd_ref.BASE_REGIONS, bwd_ref.BASE_SIZES, bwd_ref.BASE_FLIPS)),
                 "list": (3, canvases(*bwd_ref.list_case())), "seventy": (3, canvases(*bwd_ref.seventy_case())),
                 "long_rows": (2, canvases(*bwd_ref.long_rows_case())), "seams": (5, canvases(*bwd_ref.seams_case()))}
    for name, (k, geo) in bwd_cases.items():
        for nn, none in (("all", ()), ("none3", range(0, len(geo), 3))):  # every item with a gradient; every third without
            recs = back_bwd_items(k, [q + (i not in none,) for i, q in enumerate(geo)])
            for f in FILTERS5:
                for ln, layout in LAYOUTS:
                    for dn, dt in (("f32", _lib.F32), ("f16", _lib.F16), ("bf16", _lib.BF16)):
                        for dense in (0, 1):
                            yield (f"back_bwd/{name}/{nn}/{f}/{ln}/{dn}/{'dense' if dense else 'aligned'}",
                                   plan_back_bwd(f, layout, k, recs, len(geo), dt, dense))


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

    # the float ragged calls: the inputs of their planners' own error tests, and inputs that break two rules at once where the two
    # rules are written in different places, so what comes back says which is looked at first
    L = _lib.load()
    emb = lambda **kw: plan_embed(**{**dict(f="cubic", d=8, h0=5, w0=7, grids=[(2, 3)]), **kw})  # noqa: E731
    yield "err/embed/ok", emb()
    yield "err/embed/n_negative", emb(n=-1)
    yield "err/embed/d_zero", emb(d=0)
    yield "err/embed/h0_zero", emb(h0=0)
    yield "err/embed/w0_beyond", emb(w0=KMAX + 1)
    yield "err/embed/filter", emb(f=5)
    yield "err/embed/filter_before_shape", emb(f=5, d=0)
    yield "err/embed/null_block", emb(null=("desc",))
    yield "err/embed/null_grids", emb(null=("grids",))
    yield "err/embed/null_ws", emb(null=("ws",))
    yield "err/embed/null_rows", emb(null=("rows",))
    yield "err/embed/short_block", emb(nbytes=L.aa_embed_many_desc_bytes(1) - 1)
    yield "err/embed/pad_to_short", emb(pad_to=5)
    yield "err/embed/pad_to_negative", emb(pad_to=-1)
    for i, grids in enumerate([[(0, 3)], [(3, 0)], [(2, 2), (-1, 2)], [(KMAX + 1, 1)], [(1, KMAX + 1)], [(65536, 65536)]]):
        yield f"err/embed/grid_{i}", emb(grids=grids)
    yield "err/embed/ksize_h", emb(f="lanczos", h0=20000, grids=[(2, 3), (1, 3)])
    yield "err/embed/ksize_w", emb(f="lanczos", w0=20000, grids=[(2, 3), (2, 1)])
    yield "err/embed/ksize_h_and_w", emb(f="lanczos", h0=20000, w0=20000, grids=[(2, 3), (1, 1)])
    yield "err/embed/trk_h", emb(h0=1, grids=[(2, 3), (100000, 3)])
    yield "err/embed/ksize_w_and_trk_h", emb(f="lanczos", h0=1, w0=20000, grids=[(100000, 1)])
    yield "err/embed/pad_to_before_ksize", emb(f="lanczos", h0=20000, grids=[(1, 3)], pad_to=2)
    yield "err/embed/rows_beyond_a_grid", emb(d=KMAX, grids=[(1024, 1024)] * 4)

    P = _lib.NCHW
    bgeo = [((12, 16), (1, 2, 6, 9), (3, 4), False), ((12, 16), (0, 0, 12, 16), (5, 7), True)]

    def changed(recs, at=1, **kw):
        for k, v in kw.items():
            setattr(recs[at], k, v)
        return recs

    back = lambda **kw: plan_back(**{**dict(f="linear", layout=P, k=7, recs=back_items(P, 7, bgeo), n=2), **kw})  # noqa: E731
    yield "err/back/ok", back()
    yield "err/back/filter_first", back(f=5, layout=7, n=-1, null=("desc",))
    yield "err/back/layout", back(layout=7, n=-1, null=("desc",))
    yield "err/back/n_negative", back(n=-1, null=("desc",))
    yield "err/back/k_zero", back(k=0, null=("desc",))
    yield "err/back/k_beyond", back(k=KMAX + 1)
    yield "err/back/reduce", back(reduce=3, null=("desc",))
    yield "err/back/reduce_negative", back(reduce=-1)
    yield "err/back/k257_u8", back(k=257, reduce=_lib.BACK_ARGMAX, out_dtype=_lib.U8, null=("desc",))
    yield "err/back/k256_u8", back(k=256, recs=back_items(P, 256, bgeo), reduce=_lib.BACK_ARGMAX, out_dtype=_lib.U8)
    yield "err/back/k32769_i16", back(k=32769, reduce=_lib.BACK_ARGMAX, out_dtype=_lib.I16)
    yield "err/back/k32769_i32", back(k=32769, recs=back_items(P, 32769, bgeo), reduce=_lib.BACK_ARGMAX, out_dtype=_lib.I32)
    for what in ("items", "ws", "arena", "offs", "desc"):
        yield f"err/back/null_{what}", back(recs=changed(back_items(P, 7, bgeo), h=0), null=(what,), nbytes=L.aa_back_many_desc_bytes(2) - 1)
    yield "err/back/short_block", back(recs=changed(back_items(P, 7, bgeo), h=0), nbytes=L.aa_back_many_desc_bytes(2) - 1)
    yield "err/back/null_source", back(recs=changed(back_items(P, 7, bgeo), data_dev=None))
    for name, kw in (("h_zero", {"h": 0}), ("w_negative", {"w": -1}), ("oh_zero", {"oh": 0}), ("ow_zero", {"ow": 0}), ("h_beyond", {"h": KMAX + 1}),
                     ("ow_beyond", {"ow": KMAX + 1}), ("flag_bit", {"flags": 2}), ("flag_bits", {"flags": 3})):
        yield f"err/back/{name}_before_strides_and_dtype", back(recs=changed(back_items(P, 7, bgeo), stride_row=-9, **kw), out_dtype=_lib.F64)
    yield "err/back/elems_beyond", back(k=2, recs=changed(back_items(P, 2, bgeo), oh=1 << 20, ow=1 << 20))
    yield "err/back/elems_beyond_before_strides", back(k=2, recs=changed(back_items(P, 2, bgeo), oh=1 << 20, ow=1 << 20, stride_row=-9))
    yield "err/back/units_beyond", back(k=2, recs=changed(back_items(P, 2, bgeo), oh=1 << 20, ow=1 << 19))
    yield "err/back/units_beyond_sum", plan_back("linear", P, 1, back_items(P, 1, [((6, 9), None, (KMAX, 8), False)] * 5), 5)
    yield "err/back/strides_before_dtype", back(recs=changed(back_items(P, 7, bgeo), stride_row=-9), out_dtype=_lib.F64)
    yield "err/back/stride_class_nchw", back(recs=back_items(N, 7, bgeo))
    yield "err/back/stride_class_nhwc", back(layout=N)
    yield "err/back/stride_px_nhwc", back(layout=N, recs=changed(back_items(N, 7, bgeo), stride_px=8))
    yield "err/back/one_element_axes", back(k=1, recs=changed(changed(back_items(P, 1, [((1, 9), None, (3, 4), False), ((6, 1), None, (3, 4), False)]),
                                                                     0, stride_ch=-3, stride_row=-5), 1, stride_px=77))
    yield "err/back/ksize_h", back(f="lanczos", recs=changed(back_items(P, 7, bgeo), h=20000, oh=1))
    yield "err/back/ksize_w", back(f="lanczos", recs=changed(back_items(P, 7, bgeo), w=20000, ow=1))
    yield "err/back/ksize_h_and_w", back(f="lanczos", recs=changed(back_items(P, 7, bgeo), h=20000, oh=1, w=20000, ow=1))
    yield "err/back/strides_before_ksize", back(f="lanczos", recs=changed(back_items(P, 7, bgeo), h=20000, oh=1, stride_ch=-1))
    yield "err/back/ksize_before_dtype", back(f="lanczos", recs=changed(back_items(P, 7, bgeo), h=20000, oh=1), out_dtype=_lib.F64)
    for rn, reduce, bad in (("values", _lib.BACK_VALUES, (_lib.U8, _lib.F64, _lib.I32, _lib.BOOL, 9, -1)),
                            ("argmax", _lib.BACK_ARGMAX, (_lib.F32, _lib.BOOL, _lib.F64)), ("greater", _lib.BACK_GREATER, (_lib.F32, _lib.I16, _lib.I64))):
        for dt in bad:
            yield f"err/back/dtype_{rn}_{dt}", back(reduce=reduce, out_dtype=dt)

    mgeo = [((12, 16), (1, 2, 6, 9), (3, 4), False), ((12, 16), (0, 0, 12, 16), (3, 4), True)]
    mrg = lambda **kw: plan_merged(**{**dict(f="linear", layout=P, k=7, recs=back_items(P, 7, mgeo), n=2, groups=[0, 0], g=1), **kw})  # noqa: E731
    bad_shape = lambda: changed(back_items(P, 7, mgeo), 0, h=0)  # noqa: E731
    yield "err/merged/ok", mrg()
    yield "err/merged/ok_mean", mrg(merge=1)
    yield "err/merged/filter_first", mrg(f=5, layout=7, n=-1, g=-1, merge=2, groups=[0, 5], null=("desc",))
    yield "err/merged/layout", mrg(layout=7, n=-1, g=-1, merge=2, groups=[0, 5], null=("desc",))
    yield "err/merged/n_negative", mrg(n=-1, null=("desc",))
    yield "err/merged/k_zero", mrg(k=0, null=("desc",))
    yield "err/merged/k_beyond", mrg(k=KMAX + 1)
    yield "err/merged/reduce", mrg(reduce=3, null=("desc",))
    for g in (-1, 3, 0):
        yield f"err/merged/g_{g}", mrg(g=g, null=("desc",))
    for merge in (-1, 2):
        yield f"err/merged/merge_{merge}", mrg(merge=merge, null=("desc",))
    yield "err/merged/k257_u8", mrg(k=257, reduce=_lib.BACK_ARGMAX, out_dtype=_lib.U8, null=("desc",))
    yield "err/merged/k256_u8", mrg(k=256, recs=back_items(P, 256, mgeo), reduce=_lib.BACK_ARGMAX, out_dtype=_lib.U8)
    for what in ("items", "groups", "ws", "arena", "offs", "desc"):
        yield f"err/merged/null_{what}", mrg(recs=bad_shape(), groups=[0, 5], g=2, null=(what,), nbytes=L.aa_back_merged_desc_bytes(2, 2) - 1)
    yield "err/merged/short_block", mrg(recs=bad_shape(), groups=[0, 5], g=2, nbytes=L.aa_back_merged_desc_bytes(2, 2) - 1)
    for i, bad in enumerate([[0, 2], [-1, 0], [0, 1 << 40]]):
        yield f"err/merged/group_of_{i}_before_items", mrg(recs=bad_shape(), groups=bad, g=2)
    yield "err/merged/empty_group_before_null_source", mrg(recs=changed(back_items(P, 7, mgeo), 0, data_dev=None), groups=[1, 1], g=2)
    yield "err/merged/null_source", mrg(recs=changed(back_items(P, 7, mgeo), 0, data_dev=None), groups=[1, 0], g=2)
    for name, kw in (("h_zero", {"h": 0}), ("ow_zero", {"ow": 0}), ("h_beyond", {"h": KMAX + 1}), ("flag_bit", {"flags": 2})):
        yield f"err/merged/{name}_before_strides_and_dtype", mrg(recs=changed(back_items(P, 7, mgeo), stride_row=-9, **kw), out_dtype=_lib.F64)
    yield "err/merged/strides_before_dtype", mrg(recs=changed(back_items(P, 7, mgeo), stride_row=-9), out_dtype=_lib.F64)
    for name, kw in (("oh", {"oh": 4}), ("ow", {"ow": 5}), ("oh_ow", {"oh": 4, "ow": 3})):
        yield f"err/merged/member_size_{name}_before_dtype", mrg(recs=changed(back_items(P, 7, mgeo), **kw), out_dtype=_lib.F64)
        yield f"err/merged/member_size_{name}_two_groups", mrg(recs=changed(back_items(P, 7, mgeo), **kw), groups=[0, 1], g=2)
        yield f"err/merged/strides_before_member_size_{name}", mrg(recs=changed(back_items(P, 7, mgeo), stride_row=-9, **kw))
    big = [((6, 9), None, (KMAX, 8), False)]
    yield "err/merged/units_one_group", plan_merged("linear", P, 1, back_items(P, 1, big * 4), 4, [0, 0, 0, 0], 1)
    yield "err/merged/units_four_groups", plan_merged("linear", P, 1, back_items(P, 1, big * 5), 5, [0, 1, 2, 3, 3], 4)
    yield "err/merged/units_beyond", plan_merged("linear", P, 1, back_items(P, 1, big * 5), 5, [0, 1, 2, 3, 4], 5)
    yield "err/merged/elems_beyond", plan_merged("linear", P, 2, back_items(P, 2, [((6, 9), None, (1 << 20, 1 << 20), False)]), 1, [0], 1)
    yield "err/merged/elems_beyond_before_strides", mrg(k=2, recs=changed(back_items(P, 2, mgeo), oh=1 << 20, ow=1 << 20, stride_row=-9))
    yield "err/merged/ksize_h", mrg(f="lanczos", recs=changed(back_items(P, 7, mgeo), h=20000, oh=1))
    yield "err/merged/ksize_h_and_w", mrg(f="lanczos", recs=changed(back_items(P, 7, mgeo), h=20000, oh=1, w=20000, ow=1))
    yield "err/merged/strides_before_ksize", mrg(f="lanczos", recs=changed(back_items(P, 7, mgeo), h=20000, oh=1, stride_ch=-1))
    yield "err/merged/ksize_before_member_size", mrg(f="lanczos", recs=changed(back_items(P, 7, mgeo), h=20000, oh=1, ow=5))
    for rn, reduce, bad in (("values", _lib.BACK_VALUES, (_lib.U8, _lib.F64, _lib.BOOL, 9)), ("argmax", _lib.BACK_ARGMAX, (_lib.F32, _lib.BOOL)),
                            ("greater", _lib.BACK_GREATER, (_lib.F32, _lib.I64))):
        for dt in bad:
            yield f"err/merged/dtype_{rn}_{dt}", mrg(reduce=reduce, out_dtype=dt)

    wgeo = [((12, 16), (1, 2, 6, 9), (3, 4), False, True), ((12, 16), (2, 3, 5, 7), (5, 7), True, True)]
    bwd = lambda **kw: plan_back_bwd(**{**dict(f="linear", layout=P, k=7, recs=back_bwd_items(7, wgeo), n=2), **kw})  # noqa: E731
    bad_canvas = lambda: changed(back_bwd_items(7, wgeo), H=0)  # noqa: E731
    yield "err/back_bwd/ok", bwd()
    yield "err/back_bwd/filter_first", bwd(f=5, layout=7, n=-1, recs=bad_canvas(), null=("desc",))
    yield "err/back_bwd/layout", bwd(layout=7, n=-1, recs=bad_canvas(), null=("desc",))
    yield "err/back_bwd/n_negative", bwd(n=-1, null=("desc",))
    yield "err/back_bwd/k_zero", bwd(k=0, null=("desc",))
    yield "err/back_bwd/k_beyond", bwd(k=KMAX + 1)
    yield "err/back_bwd/dense_2", bwd(dense=2, null=("desc",))
    yield "err/back_bwd/dense_negative", bwd(dense=-1)
    for what in ("items", "ws", "out", "offs", "desc"):
        yield f"err/back_bwd/null_{what}", bwd(recs=bad_canvas(), null=(what,), nbytes=L.aa_back_many_bwd_desc_bytes(2) - 1)
    yield "err/back_bwd/short_block", bwd(recs=bad_canvas(), nbytes=L.aa_back_many_bwd_desc_bytes(2) - 1)
    for name, kw in (("H_zero", {"H": 0}), ("W_negative", {"W": -1}), ("H_beyond", {"H": KMAX + 1}), ("flag_bit", {"flags": 2}), ("oh_zero", {"oh": 0}),
                     ("ow_beyond", {"ow": KMAX + 1}), ("h_zero", {"h": 0}), ("y0_negative", {"y0": -1}), ("y0_beyond", {"y0": 8}),
                     ("x0_beyond", {"x0": 10}), ("region_beyond", {"y0": 0, "x0": 0, "h": 13, "w": 16})):
        yield f"err/back_bwd/{name}_before_strides_and_dtype", bwd(recs=changed(back_bwd_items(7, wgeo), stride_row=-4, **kw), out_dtype=_lib.F64)
    yield "err/back_bwd/canvas_elems_beyond", bwd(k=2, recs=changed(back_bwd_items(2, wgeo), H=1 << 20, W=1 << 20))
    yield "err/back_bwd/grad_elems_beyond", bwd(k=2, recs=changed(back_bwd_items(2, wgeo), oh=1 << 20, ow=1 << 20))
    yield "err/back_bwd/grad_elems_beyond_before_strides", bwd(k=2, recs=changed(back_bwd_items(2, wgeo), oh=1 << 20, ow=1 << 20, stride_row=-4))
    yield "err/back_bwd/no_gradient_nothing_else_looked_at", bwd(recs=changed(back_bwd_items(7, wgeo), grad_dev=None, y0=-5, x0=99, h=0, w=0, oh=0, ow=-3,
                                                                                stride_ch=-1, stride_row=-1))
    yield "err/back_bwd/no_gradient_bad_canvas", bwd(recs=changed(bad_canvas(), grad_dev=None))
    yield "err/back_bwd/strides_before_dtype", bwd(recs=changed(back_bwd_items(7, wgeo), stride_row=-4), out_dtype=_lib.F64)
    yield "err/back_bwd/stride_ch", bwd(recs=changed(back_bwd_items(7, wgeo), stride_ch=-12))
    yield "err/back_bwd/one_row_stride_unused", bwd(recs=changed(back_bwd_items(7, wgeo), oh=1, stride_row=-4))
    yield "err/back_bwd/one_class_stride_unused", bwd(k=1, recs=changed(back_bwd_items(1, wgeo), stride_ch=-3))
    wide = [((KMAX, 64), (0, 0, 2, 2), (3, 4), False, True)]
    yield "err/back_bwd/units_15", plan_back_bwd("linear", P, 1, back_bwd_items(1, wide * 15), 15)
    yield "err/back_bwd/units_beyond", plan_back_bwd("linear", P, 1, back_bwd_items(1, wide * 16), 16)
    yield "err/back_bwd/ksize_h", bwd(f="lanczos", recs=changed(back_bwd_items(7, [((20000, 16), None, (1, 4), False, True)] * 2), x0=2, w=9))
    yield "err/back_bwd/ksize_w", bwd(f="lanczos", recs=changed(back_bwd_items(7, [((12, 20000), None, (3, 1), False, True)] * 2), y0=1, h=6))
    yield "err/back_bwd/ksize_h_and_w", bwd(f="lanczos", recs=back_bwd_items(7, [((20000, 20000), None, (1, 1), False, True)] * 2))
    yield "err/back_bwd/trk_h", bwd(recs=changed(back_bwd_items(7, wgeo), h=1, oh=100000))
    yield "err/back_bwd/ksize_w_and_trk_h", bwd(f="lanczos", recs=back_bwd_items(7, [((1, 20000), None, (100000, 1), False, True)] * 2))
    yield "err/back_bwd/strides_before_ksize", bwd(f="lanczos", recs=changed(back_bwd_items(7, [((20000, 16), None, (1, 4), False, True)] * 2), 0,
                                                                             stride_ch=-1))
    yield "err/back_bwd/ksize_before_dtype", bwd(f="lanczos", recs=back_bwd_items(7, [((20000, 16), None, (1, 4), False, True)] * 2), out_dtype=_lib.F64)
    for dt in (_lib.U8, _lib.F64, _lib.I32, _lib.BOOL, 9, -1):
        yield f"err/back_bwd/dtype_{dt}", bwd(out_dtype=dt)


def plans():
    """-> (key, rc, workspace bytes, descriptor bytes) of every plan."""
    for key, (rc, ws, block) in _case_plans():
        yield key, rc, ws, block
    for key, (rc, ws, block) in _float_case_plans():
        yield key, rc, ws, block
    for key, (rc, ws, block) in _error_plans():
        yield key, rc, ws, block
