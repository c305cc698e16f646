"""ctypes binding of libaa_interp.so (the C-ABI declared in include/aa_interp.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C interpolate_antialiasing_amd/csrc``.
There is NO fallback: if the shared object is missing, loading fails loudly, and every op in this package
needs it (the CPU oracle under oracle/ is test infrastructure and is never imported from here).
"""
from __future__ import annotations

import collections
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# AA_INTERP_LIB: developer A/B runs of an alternative build of the SAME library (tools/ab_build.sh); never a fallback
LIB_PATH = os.environ.get("AA_INTERP_LIB") or os.path.join(_HERE, "csrc", "libaa_interp.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "aa_interp.h")

# enums (include/aa_interp.h)
AA_OK = 0
FILTER_LINEAR, FILTER_CUBIC, FILTER_BOX, FILTER_HAMMING, FILTER_LANCZOS = 0, 1, 2, 3, 4
# The five filters in one place; every table of filter names, ids, modes and supports in the package is derived from this one.
# support: Pillow's (Resample.c's filter structs, Image._filters_support); op: the stem of its callables' names (<op>_forward, ...).
Filter = collections.namedtuple("Filter", "id name aliases support op")
FILTERS = (Filter(FILTER_LINEAR, "linear", ("bilinear",), 1.0, "linear"), Filter(FILTER_CUBIC, "cubic", ("bicubic",), 2.0, "cubic"),
           Filter(FILTER_BOX, "box", ("nearest",), 0.5, "nearest"), Filter(FILTER_HAMMING, "hamming", (), 1.0, "hamming"),
           Filter(FILTER_LANCZOS, "lanczos", (), 3.0, "lanczos"))
FILTER_NAMES = {f.id: f.name for f in FILTERS}


def by_filter_name(value) -> dict:
    """{name or alias: value(filter)} over the five filters."""
    return {n: value(f) for f in FILTERS for n in (f.name,) + f.aliases}


FILTER_IDS = by_filter_name(lambda f: f.id)
U8, F32, F64, F16, BF16 = 0, 1, 2, 3, 4
I16, I32, I64, BOOL = 5, 6, 7, 8  # aa_dtype: what only aa_back_many_plan stores (labels, masks)
NCHW, NHWC = 0, 1
TABLE_PIL, TABLE_F32, TABLE_F64 = 0, 1, 2
ERR_BAD_DTYPE = -2
ERR_BAD_SHAPE = -4
ERR_STRIDES = -10
FLAG_FAST = 1
FLAG_PREMUL_ALPHA = 2
FLAG_OUT_F16 = 4   # aa_convert.flags only: the decode-adjacent forward writes float16 ...
FLAG_OUT_BF16 = 8  # ... or bfloat16 instead of float32

# every symbol include/aa_interp.h declares (tests check the .so exports exactly these)
EXPORTS = (
    "aa_abi_version", "aa_strerror", "aa_device_count", "aa_table_ksize", "aa_table_bytes", "aa_table_build_bytes", "aa_table_build",
    "aa_table_transposed_ksize", "aa_table_transpose", "aa_table_query", "aa_table_query2", "aa_table_build2", "aa_workspace_bytes", "aa_resample_fwd",
    "aa_resample_bwd", "aa_resample_bwd_atomic", "aa_workspace_bytes_bwd", "aa_resample_axis_fwd", "aa_set_fused",
    "aa_last_variant", "aa_probe_copy", "aa_probe_launch_shape", "aa_workspace_bytes_u8_to_f32", "aa_resample_fwd_u8_to_f32", "aa_set_store_form", "aa_set_plane_groups", "aa_resample_fwd_ex", "aa_resample_fwd_strided",
    "aa_workspace_bytes_ex", "aa_table_ksize_box", "aa_table_build_bytes_box", "aa_table_build_box", "aa_reduce_u8", "aa_premultiply_u8",
    "aa_unpremultiply_u8", "aa_many_desc_bytes", "aa_many_plan", "aa_resample_many_u8", "aa_resample_many_u8_to_float",
    "aa_many_desc_bytes_placed", "aa_many_plan_placed", "aa_many_desc_bytes_patches", "aa_many_plan_patches", "aa_resample_many_u8_to_patches",
    "aa_reduce_many_desc_bytes", "aa_reduce_many_plan", "aa_reduce_many_u8",
    "aa_many_desc_bytes_nearest", "aa_many_plan_nearest", "aa_resample_many_nearest",
    "aa_many_desc_bytes_maps", "aa_many_plan_maps", "aa_resample_many_maps",
    "aa_many_desc_bytes_ycbcr", "aa_many_plan_ycbcr", "aa_resample_many_ycbcr", "aa_ycbcr_to_rgb_u8",
    "aa_set_launch_shape", "aa_last_launch_shape",
    "aa_embed_many_desc_bytes", "aa_embed_many_plan", "aa_resample_embed_many", "aa_resample_embed_many_bwd",
    "aa_back_many_desc_bytes", "aa_back_many_plan", "aa_resample_back_many",
    "aa_back_many_bwd_desc_bytes", "aa_back_many_bwd_plan", "aa_resample_back_many_bwd",
    "aa_back_merged_desc_bytes", "aa_back_merged_plan", "aa_resample_back_merged",
    "aa_back_many_plan_act", "aa_back_merged_plan_act",
)


class TableHeader(ctypes.Structure):
    _fields_ = [
        ("magic", ctypes.c_int32), ("filter", ctypes.c_int32), ("kind", ctypes.c_int32), ("in_size", ctypes.c_int32),
        ("out_size", ctypes.c_int32), ("ksize", ctypes.c_int32), ("align_corners", ctypes.c_int32),
        ("max_taps", ctypes.c_int32), ("transposed", ctypes.c_int32), ("scatter_off", ctypes.c_int32),
        ("scatter_ksize", ctypes.c_int32), ("scatter_max", ctypes.c_int32), ("span64p1", ctypes.c_int32), ("span4p1", ctypes.c_int32), ("gather_off", ctypes.c_int32), ("reserved", ctypes.c_int32 * 1),
    ]


class Axis(ctypes.Structure):
    _fields_ = [
        ("table_dev", ctypes.c_void_p), ("in_size", ctypes.c_int32), ("out_size", ctypes.c_int32),
        ("ksize", ctypes.c_int32), ("max_taps", ctypes.c_int32), ("kind", ctypes.c_int32), ("filter", ctypes.c_int32),
        ("scatter_off", ctypes.c_int32), ("scatter_ksize", ctypes.c_int32), ("scatter_max", ctypes.c_int32),
        ("span64p1", ctypes.c_int32), ("span4p1", ctypes.c_int32), ("gather_off", ctypes.c_int32), ("reserved", ctypes.c_int32 * 2),
    ]


class Convert(ctypes.Structure):
    _fields_ = [("out_layout", ctypes.c_int32), ("normalize", ctypes.c_int32), ("mean", ctypes.c_float * 4),
                ("std", ctypes.c_float * 4), ("flags", ctypes.c_uint32)]


class ManyImage(ctypes.Structure):
    """aa_many_image: one item of the ragged call (strides in bytes; box = x0, y0, x1, y1)."""
    _fields_ = [("data_dev", ctypes.c_void_p), ("H", ctypes.c_int64), ("W", ctypes.c_int64), ("stride_row", ctypes.c_int64),
                ("stride_px", ctypes.c_int64), ("stride_ch", ctypes.c_int64), ("box", ctypes.c_double * 4), ("has_box", ctypes.c_int32),
                ("flags", ctypes.c_int32)]


class ManyHeader(ctypes.Structure):
    """Head of the descriptor block aa_many_plan writes (csrc/aa_many.h AAManyHeader; opaque to C callers, mirrored here for the tests).
    The three live fields are read by the names csrc/aa_many.h gives them, ``flips``, ``kind`` (MANY_PLAN_* bits) and ``fill``; the
    ctypes fields keep the names they had while the words were unused, which earlier code iterates over by name."""
    _fields_ = [("magic", ctypes.c_int32), ("n", ctypes.c_int32), ("C", ctypes.c_int32), ("oH", ctypes.c_int32), ("oW", ctypes.c_int32),
                ("filter", ctypes.c_int32), ("layout", ctypes.c_int32), ("reserved0", ctypes.c_int32), ("hunits", ctypes.c_int64),
                ("ws_bytes", ctypes.c_int64), ("reserved", ctypes.c_int64 * 2)]
    flips = property(lambda self: self.reserved0)
    kind = property(lambda self: self.reserved[0])
    fill = property(lambda self: self.reserved[1])


class ManyItem(ctypes.Structure):
    """One item of that block (csrc/aa_many.h AAManyItem): offsets in bytes into the workspace, hulls [o, o + hull) per axis.  ``flags``
    (MANY_ITEM_* bits) reads the last field by the name csrc/aa_many.h gives it."""
    _fields_ = [("src", ctypes.c_void_p), ("row_stride", ctypes.c_int64), ("plane_stride", ctypes.c_int64), ("tab_h", ctypes.c_int64),
                ("tab_w", ctypes.c_int64), ("inter", ctypes.c_int64), ("in0_h", ctypes.c_double), ("in1_h", ctypes.c_double),
                ("in0_w", ctypes.c_double), ("in1_w", ctypes.c_double), ("oy", ctypes.c_int32), ("hull_h", ctypes.c_int32),
                ("ox", ctypes.c_int32), ("hull_w", ctypes.c_int32), ("ksize_h", ctypes.c_int32), ("ksize_w", ctypes.c_int32),
                ("box_on", ctypes.c_int32), ("reserved", ctypes.c_int32)]
    flags = property(lambda self: self.reserved)


class ManyPlace(ctypes.Structure):
    """aa_many_place: the size [vH, vW] Pillow resizes an item to and where that result's corner lands on the canvas."""
    _fields_ = [("vH", ctypes.c_int64), ("vW", ctypes.c_int64), ("oy", ctypes.c_int64), ("ox", ctypes.c_int64)]


class ManyPlaced(ctypes.Structure):
    """A placed plan's second record of an item (csrc/aa_many.h AAManyPlace): per axis the item's own size v, the covered part
    [v0, v0 + m) of it and the canvas index d that part starts at."""
    _fields_ = [("vh", ctypes.c_int32), ("vw", ctypes.c_int32), ("v0h", ctypes.c_int32), ("v0w", ctypes.c_int32), ("mh", ctypes.c_int32),
                ("mw", ctypes.c_int32), ("dy", ctypes.c_int32), ("dx", ctypes.c_int32)]


class NearHeader(ctypes.Structure):
    """Head of the block aa_many_plan_nearest writes (csrc/aa_many_nearest.h AANearHeader; opaque to C callers, mirrored for the tests)."""
    _fields_ = [("magic", ctypes.c_int32), ("n", ctypes.c_int32), ("C", ctypes.c_int32), ("oH", ctypes.c_int32), ("oW", ctypes.c_int32),
                ("layout", ctypes.c_int32), ("elem_bytes", ctypes.c_int32), ("reserved0", ctypes.c_int32), ("units", ctypes.c_int64),
                ("ws_bytes", ctypes.c_int64), ("fill", ctypes.c_int32 * 4)]


class NearItem(ctypes.Structure):
    """One item of that block (csrc/aa_many_nearest.h AANearItem): per axis Pillow's two doubles (step a, first centre xo0), the item's own
    size v, the covered part [v0, v0 + m) of it and the canvas index d it starts at; dxo is dx on the mirrored row of an item that flips."""
    _fields_ = [("src", ctypes.c_void_p), ("row_stride", ctypes.c_int64), ("plane_stride", ctypes.c_int64), ("tab_h", ctypes.c_int64),
                ("tab_w", ctypes.c_int64), ("a_h", ctypes.c_double), ("xo0_h", ctypes.c_double), ("a_w", ctypes.c_double),
                ("xo0_w", ctypes.c_double), ("in_h", ctypes.c_int32), ("in_w", ctypes.c_int32), ("vh", ctypes.c_int32), ("vw", ctypes.c_int32),
                ("v0h", ctypes.c_int32), ("v0w", ctypes.c_int32), ("mh", ctypes.c_int32), ("mw", ctypes.c_int32), ("dy", ctypes.c_int32),
                ("dx", ctypes.c_int32), ("dxo", ctypes.c_int32), ("flags", ctypes.c_int32), ("reserved", ctypes.c_int64)]


class MapsHeader(ctypes.Structure):
    """Head of the block aa_many_plan_maps writes (csrc/aa_many_maps.h AAMapsHeader; opaque to C callers, mirrored for the tests)."""
    _fields_ = [("magic", ctypes.c_int32), ("n", ctypes.c_int32), ("oH", ctypes.c_int32), ("oW", ctypes.c_int32), ("filter", ctypes.c_int32),
                ("elem", ctypes.c_int32), ("overflow", ctypes.c_int32), ("fill", ctypes.c_uint32), ("hunits", ctypes.c_int64),
                ("ws_bytes", ctypes.c_int64), ("reserved", ctypes.c_int64 * 2)]


class MapsItem(ctypes.Structure):
    """One item of that block (csrc/aa_many_maps.h AAMapsItem): the passes Pillow runs (flags, MAPS_ITEM_*), per axis Pillow's origin and
    scale, the hull [o, o + hull) its pass reads, ksize, the item's own size v, the covered part [v0, v0 + m) and the canvas index d."""
    _fields_ = [("src", ctypes.c_void_p), ("row_stride", ctypes.c_int64), ("tab_h", ctypes.c_int64), ("tab_w", ctypes.c_int64),
                ("inter", ctypes.c_int64), ("in0_h", ctypes.c_double), ("scale_h", ctypes.c_double), ("in0_w", ctypes.c_double),
                ("scale_w", ctypes.c_double), ("in_h", ctypes.c_int32), ("in_w", ctypes.c_int32), ("oy", ctypes.c_int32),
                ("hull_h", ctypes.c_int32), ("ox", ctypes.c_int32), ("hull_w", ctypes.c_int32), ("ksize_h", ctypes.c_int32),
                ("ksize_w", ctypes.c_int32), ("vh", ctypes.c_int32), ("vw", ctypes.c_int32), ("v0h", ctypes.c_int32), ("v0w", ctypes.c_int32),
                ("mh", ctypes.c_int32), ("mw", ctypes.c_int32), ("dy", ctypes.c_int32), ("dx", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class YccImage(ctypes.Structure):
    """aa_ycbcr_image: one item of the ragged YCbCr call (strides in bytes; box = x0, y0, x1, y1 in luma coordinates)."""
    _fields_ = [("y_dev", ctypes.c_void_p), ("cb_dev", ctypes.c_void_p), ("cr_dev", ctypes.c_void_p), ("H", ctypes.c_int64), ("W", ctypes.c_int64),
                ("cH", ctypes.c_int64), ("cW", ctypes.c_int64), ("y_stride_row", ctypes.c_int64), ("cb_stride_row", ctypes.c_int64),
                ("cr_stride_row", ctypes.c_int64), ("chroma_stride_px", ctypes.c_int32), ("subsampling", ctypes.c_int32),
                ("box", ctypes.c_double * 4), ("has_box", ctypes.c_int32), ("flags", ctypes.c_int32)]


class YccHeader(ctypes.Structure):
    """Head of the block aa_many_plan_ycbcr writes (csrc/aa_many_ycbcr.h AAYccHeader; opaque to C callers, mirrored for the tests): plan A
    (a placed ManyHeader block: the luma items, then the Cb and the Cr items when the chroma is planar) at off_a, plan B (the interleaved
    chroma pairs) at off_b or 0."""
    _fields_ = [("magic", ctypes.c_int32), ("n", ctypes.c_int32), ("oH", ctypes.c_int32), ("oW", ctypes.c_int32), ("filter", ctypes.c_int32),
                ("interleaved", ctypes.c_int32), ("flips", ctypes.c_int32), ("fill", ctypes.c_uint32), ("off_a", ctypes.c_int64),
                ("off_b", ctypes.c_int64), ("ws_b", ctypes.c_int64), ("ws_bytes", ctypes.c_int64)]


class ReduceItem(ctypes.Structure):
    """aa_reduce_item: one item of the ragged Image.reduce (strides in bytes; box = x0, y0, x1, y1 integers; factors fx, fy)."""
    _fields_ = [("data_dev", ctypes.c_void_p), ("H", ctypes.c_int64), ("W", ctypes.c_int64), ("stride_row", ctypes.c_int64),
                ("stride_px", ctypes.c_int64), ("stride_ch", ctypes.c_int64), ("box", ctypes.c_int64 * 4), ("fx", ctypes.c_int32),
                ("fy", ctypes.c_int32)]


class ReduceManyHeader(ctypes.Structure):
    """Head of the block aa_reduce_many_plan writes (csrc/aa_reduce_many.h AAReduceManyHeader; opaque to C callers, mirrored for the tests)."""
    _fields_ = [("magic", ctypes.c_int32), ("n", ctypes.c_int32), ("C", ctypes.c_int32), ("layout", ctypes.c_int32), ("E", ctypes.c_int32),
                ("planes", ctypes.c_int32), ("units", ctypes.c_int64), ("arena_bytes", ctypes.c_int64), ("reserved", ctypes.c_int64 * 3)]


class ReduceManyItem(ctypes.Structure):
    """One item of that block (csrc/aa_reduce_many.h AAReduceManyItem): the box's first byte, pitches, arena offset, sizes, tiling, mults."""
    _fields_ = [("src", ctypes.c_void_p), ("row_pitch", ctypes.c_int64), ("plane_pitch", ctypes.c_int64), ("out_off", ctypes.c_int64),
                ("bw", ctypes.c_int32), ("bh", ctypes.c_int32), ("fx", ctypes.c_int32), ("fy", ctypes.c_int32), ("rw", ctypes.c_int32),
                ("rh", ctypes.c_int32), ("sx", ctypes.c_int32), ("xtiles", ctypes.c_int32), ("mult", ctypes.c_uint32 * 4)]


class EmbedHeader(ctypes.Structure):
    """Head of the block aa_embed_many_plan writes (csrc/aa_embed_many.h AAEmbedHeader; opaque to C callers, mirrored for the tests)."""
    _fields_ = [("magic", ctypes.c_int32), ("n", ctypes.c_int32), ("D", ctypes.c_int32), ("H0", ctypes.c_int32), ("W0", ctypes.c_int32),
                ("filter", ctypes.c_int32), ("pad_to", ctypes.c_int32), ("reserved0", ctypes.c_int32), ("out_rows", ctypes.c_int64),
                ("ws_bytes", ctypes.c_int64), ("reserved", ctypes.c_int64 * 2)]


class EmbedItem(ctypes.Structure):
    """One item of that block (csrc/aa_embed_many.h AAEmbedItem): the workspace offsets of its two tables and their adjoints, its token
    grid, the tables' row lengths and the two float scales."""
    _fields_ = [("tab_h", ctypes.c_int64), ("tab_w", ctypes.c_int64), ("tr_h", ctypes.c_int64), ("tr_w", ctypes.c_int64),
                ("gh", ctypes.c_int32), ("gw", ctypes.c_int32), ("ksize_h", ctypes.c_int32), ("ksize_w", ctypes.c_int32),
                ("trk_h", ctypes.c_int32), ("trk_w", ctypes.c_int32), ("scale_h", ctypes.c_float), ("scale_w", ctypes.c_float)]


class BackItemIn(ctypes.Structure):
    """aa_back_item: one item of the ragged return path (strides in ELEMENTS; data_dev at the region's corner)."""
    _fields_ = [("data_dev", ctypes.c_void_p), ("stride_ch", ctypes.c_int64), ("stride_row", ctypes.c_int64), ("stride_px", ctypes.c_int64),
                ("h", ctypes.c_int64), ("w", ctypes.c_int64), ("oh", ctypes.c_int64), ("ow", ctypes.c_int64), ("flags", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class BackHeader(ctypes.Structure):
    """Head of the block aa_back_many_plan writes (csrc/aa_many_back.h AABackHeader; opaque to C callers, mirrored for the tests)."""
    _fields_ = [("magic", ctypes.c_int32), ("n", ctypes.c_int32), ("K", ctypes.c_int32), ("filter", ctypes.c_int32), ("layout", ctypes.c_int32),
                ("reduce", ctypes.c_int32), ("out_dtype", ctypes.c_int32), ("reserved0", ctypes.c_int32), ("units", ctypes.c_int64),
                ("ws_bytes", ctypes.c_int64), ("arena_bytes", ctypes.c_int64), ("reserved", ctypes.c_int64)]


class BackItem(ctypes.Structure):
    """One item of that block (csrc/aa_many_back.h AABackItem): the region's corner and element strides, the workspace offsets of its two
    tables, its arena offset in bytes, sizes, the tables' row lengths, the two float scales, flags and its column tiles."""
    _fields_ = [("src", ctypes.c_void_p), ("stride_ch", ctypes.c_int64), ("stride_row", ctypes.c_int64), ("stride_px", ctypes.c_int64),
                ("tab_h", ctypes.c_int64), ("tab_w", ctypes.c_int64), ("out_off", ctypes.c_int64), ("h", ctypes.c_int32), ("w", ctypes.c_int32),
                ("oh", ctypes.c_int32), ("ow", ctypes.c_int32), ("ksize_h", ctypes.c_int32), ("ksize_w", ctypes.c_int32),
                ("scale_h", ctypes.c_float), ("scale_w", ctypes.c_float), ("flags", ctypes.c_int32), ("xtiles", ctypes.c_int32)]


class BackMergedHeader(ctypes.Structure):
    """Head of the block aa_back_merged_plan writes (csrc/aa_many_back.h AABackMergedHeader; opaque to C callers, mirrored for the tests)."""
    _fields_ = [("magic", ctypes.c_int32), ("n", ctypes.c_int32), ("K", ctypes.c_int32), ("filter", ctypes.c_int32), ("layout", ctypes.c_int32),
                ("reduce", ctypes.c_int32), ("out_dtype", ctypes.c_int32), ("merge", ctypes.c_int32), ("units", ctypes.c_int64),
                ("ws_bytes", ctypes.c_int64), ("arena_bytes", ctypes.c_int64), ("G", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class BackGroup(ctypes.Structure):
    """One group of that block (csrc/aa_many_back.h AABackGroup): its arena offset in bytes, its first slot of the member list, its
    members, its size and its column tiles."""
    _fields_ = [("out_off", ctypes.c_int64), ("first", ctypes.c_int32), ("count", ctypes.c_int32), ("oh", ctypes.c_int32), ("ow", ctypes.c_int32),
                ("xtiles", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class BackBwdItemIn(ctypes.Structure):
    """aa_back_bwd_item: one item of the ragged return path's backward (strides in ELEMENTS; grad_dev None: the item has no gradient)."""
    _fields_ = [("grad_dev", ctypes.c_void_p), ("stride_ch", ctypes.c_int64), ("stride_row", ctypes.c_int64), ("H", ctypes.c_int64),
                ("W", ctypes.c_int64), ("y0", ctypes.c_int64), ("x0", ctypes.c_int64), ("h", ctypes.c_int64), ("w", ctypes.c_int64),
                ("oh", ctypes.c_int64), ("ow", ctypes.c_int64), ("flags", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class BackBwdHeader(ctypes.Structure):
    """Head of the block aa_back_many_bwd_plan writes (csrc/aa_many_back_bwd.h AABackBwdHeader; opaque to C callers, mirrored for the tests)."""
    _fields_ = [("magic", ctypes.c_int32), ("n", ctypes.c_int32), ("K", ctypes.c_int32), ("filter", ctypes.c_int32), ("out_layout", ctypes.c_int32),
                ("out_dtype", ctypes.c_int32), ("dense", ctypes.c_int32), ("reserved0", ctypes.c_int32), ("units", ctypes.c_int64),
                ("ws_bytes", ctypes.c_int64), ("out_bytes", ctypes.c_int64), ("reserved", ctypes.c_int64)]


class BackBwdItem(ctypes.Structure):
    """One item of that block (csrc/aa_many_back_bwd.h AABackBwdItem): the gradient and its element strides, the workspace offsets of its
    two forward tables and their adjoints, its output offset in bytes, the canvas, the region, the gradient's size, the tables' row
    lengths, the two float scales, flags and its column tiles."""
    _fields_ = [("grad", ctypes.c_void_p), ("stride_ch", ctypes.c_int64), ("stride_row", ctypes.c_int64), ("tab_h", ctypes.c_int64),
                ("tab_w", ctypes.c_int64), ("tr_h", ctypes.c_int64), ("tr_w", ctypes.c_int64), ("out_off", ctypes.c_int64),
                ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("y0", ctypes.c_int32), ("x0", ctypes.c_int32), ("h", ctypes.c_int32),
                ("w", ctypes.c_int32), ("oh", ctypes.c_int32), ("ow", ctypes.c_int32), ("ksize_h", ctypes.c_int32), ("ksize_w", ctypes.c_int32),
                ("trk_h", ctypes.c_int32), ("trk_w", ctypes.c_int32), ("scale_h", ctypes.c_float), ("scale_w", ctypes.c_float),
                ("flags", ctypes.c_int32), ("xtiles", ctypes.c_int32)]


class LaunchShapeIn(ctypes.Structure):
    """aa_launch_shape_in: what a fused family's launch shape is chosen from (csrc/aa_launch_shape.h); occupancy[s] for s = 1..8 strips."""
    _fields_ = [("family", ctypes.c_int32), ("nstrips", ctypes.c_int32), ("strips_per_block", ctypes.c_int32), ("spb_forced", ctypes.c_int32),
                ("items", ctypes.c_int64), ("H", ctypes.c_int64), ("oH", ctypes.c_int64), ("taps_h", ctypes.c_int32), ("taps_w", ctypes.c_int32),
                ("lds", ctypes.c_uint64), ("saturation", ctypes.c_int32), ("threads", ctypes.c_int32), ("cus", ctypes.c_int32),
                ("occupancy", ctypes.c_int32 * 9)]


class LaunchShapeOut(ctypes.Structure):
    """aa_launch_shape_out: strips per workgroup, row bands, resident workgroups used, items x bands, workgroups (0: beyond a grid)."""
    _fields_ = [("strips_per_block", ctypes.c_int32), ("ybands", ctypes.c_int32), ("resident", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("groups", ctypes.c_int64), ("grid", ctypes.c_int64)]


LAUNCH_V1, LAUNCH_V3, LAUNCH_F32_DOWN, LAUNCH_F32_UP = 0, 1, 2, 3  # aa_launch_family

MANY_FLIP_X = 1     # aa_many_image.flags: mirror the item's output left to right (aa_resample_many_u8_to_float only)
MANY_PREMUL_ALPHA = 2  # aa_many_image.flags: Pillow's RGBA / LA resize of that item (C 2 or 4, straight alpha last; not for patch plans)
PATCH_CPP, PATCH_PPC = 0, 1  # aa_resample_many_u8_to_patches: token vector [C, ph, pw] or [ph, pw, C]
MANY_PLAN_PLACED, MANY_PLAN_PATCHES, MANY_PLAN_ALPHA = 1, 2, 4  # ManyHeader.kind (csrc/aa_many.h AA_MANY_PLAN_*)
MANY_ITEM_FLIP, MANY_ITEM_ALPHA = 1, 2  # ManyItem.flags (csrc/aa_many.h AA_MANY_ITEM_*)
MAPS_U16, MAPS_I32, MAPS_F32 = 0, 1, 2  # aa_many_plan_maps elem: Pillow's "I;16", "I", "F"
MAPS_OVERFLOW = {"pillow": 0, "clamp": 1}  # aa_many_plan_maps overflow (AA_MAPS_OVERFLOW_*)
MAPS_ITEM_FLIP, MAPS_ITEM_HPASS, MAPS_ITEM_VPASS = 1, 2, 4  # MapsItem.flags (csrc/aa_many_maps.h AA_MAPS_ITEM_*)
MAPS_HROWS = 16     # hull rows per work unit of the maps call's horizontal pass (csrc/aa_many_maps.h AA_MAPS_HROWS)
MAPS_VCOLS = 256    # canvas columns per work unit of the maps call's vertical pass (csrc/aa_many_maps.h AA_MAPS_VCOLS)
YCC_SUBSAMPLING = {"444": 0, "422": 1, "420": 2, "440": 3}  # aa_ycbcr_image.subsampling (AA_YCC_*)
YCC_VROWS, YCC_VCOLS = 4, 256  # canvas rows and columns per work unit of the YCbCr call's vertical pass (csrc/aa_many_ycbcr.h)
BACK_VALUES, BACK_ARGMAX, BACK_GREATER = 0, 1, 2  # aa_back_many_plan reduce (csrc/aa_many_back.h AA_BACK_*)
BACK_MERGE = {"sum": 0, "mean": 1}  # aa_back_merged_plan merge (csrc/aa_many_back.h AA_BACK_MERGE_*)
BACK_ACT = {None: 0, "softmax": 1, "sigmoid": 2}  # aa_back_many_plan_act activation (include/aa_interp.h AA_BACK_ACT_*)
BACK_ACT_MEMBERS = 16  # the most members of a group of a merged softmax plan (csrc/aa_many_back.h AA_BACK_ACT_MEMBERS)
BACK_TILE = 256     # output columns per work unit of the return path's resample (csrc/aa_many_back.h AA_BACK_TILE)
BACK_BWD_ROWS, BACK_BWD_COLS = 4, 64  # canvas rows and columns per work unit of the return path's backward (csrc/aa_many_back_bwd.h)
MANY_STRIP = 64     # output columns per work unit of the ragged call's horizontal pass (csrc/aa_many.h AA_MANY_STRIP)


def desc_view(buf, n: int, Header, Item):
    """(header, items, prefix) of a planner's block held in a ctypes buffer, [Header][n Items][int64 prefix[n + 1]]: the four below."""
    hd = Header.from_buffer(buf, 0)
    items = (Item * n).from_buffer(buf, ctypes.sizeof(Header))
    prefix = (ctypes.c_int64 * (n + 1)).from_buffer(buf, ctypes.sizeof(Header) + n * ctypes.sizeof(Item))
    return hd, items, prefix


def many_desc_view(buf, n: int):  # (any of aa_many_plan's blocks: what follows the prefix sums is many_placed_view's, many_patch_view's)
    return desc_view(buf, n, ManyHeader, ManyItem)


def reduce_many_desc_view(buf, n: int):
    return desc_view(buf, n, ReduceManyHeader, ReduceManyItem)


def near_desc_view(buf, n: int):
    return desc_view(buf, n, NearHeader, NearItem)


def maps_desc_view(buf, n: int):
    return desc_view(buf, n, MapsHeader, MapsItem)


def embed_desc_view(buf, n: int):
    return desc_view(buf, n, EmbedHeader, EmbedItem)


def back_desc_view(buf, n: int):
    return desc_view(buf, n, BackHeader, BackItem)


def back_merged_desc_view(buf, n: int, g: int):
    """(header, items, groups, members, unit0) of aa_back_merged_plan's block held in a ctypes buffer:
    [BackMergedHeader][n BackItems][g BackGroups][int32 member[n], padded to 8 bytes][int64 unit0[g + 1]]."""
    hd = BackMergedHeader.from_buffer(buf, 0)
    at = ctypes.sizeof(BackMergedHeader)
    items = (BackItem * n).from_buffer(buf, at)
    at += n * ctypes.sizeof(BackItem)
    groups = (BackGroup * g).from_buffer(buf, at)
    at += g * ctypes.sizeof(BackGroup)
    members = (ctypes.c_int32 * n).from_buffer(buf, at)
    at += (4 * n + 7) & ~7
    return hd, items, groups, members, (ctypes.c_int64 * (g + 1)).from_buffer(buf, at)


def back_bwd_desc_view(buf, n: int):
    return desc_view(buf, n, BackBwdHeader, BackBwdItem)


def many_placed_view(buf, n: int):
    """The placement records of a placed plan's block (ManyHeader.kind has MANY_PLAN_PLACED): they follow the prefix sums."""
    return (ManyPlaced * n).from_buffer(buf, ctypes.sizeof(ManyHeader) + n * ctypes.sizeof(ManyItem) + 8 * (n + 1))


def many_patch_view(buf, n: int):
    """(vunit_prefix[n + 1], tok0[n + 1]) of a patch plan's block: they follow the placement records."""
    off = ctypes.sizeof(ManyHeader) + n * ctypes.sizeof(ManyItem) + 8 * (n + 1) + n * ctypes.sizeof(ManyPlaced)
    return (ctypes.c_int64 * (n + 1)).from_buffer(buf, off), (ctypes.c_int64 * (n + 1)).from_buffer(buf, off + 8 * (n + 1))


class AAInterpError(RuntimeError):
    pass


_lib = None


def load() -> ctypes.CDLL:
    """Load libaa_interp.so, declaring every prototype.  Raises if the library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AAInterpError(
            f"{LIB_PATH} is missing: the HIP extension has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C interpolate_antialiasing_amd/csrc`). "
            "There is no CPU fallback."
        )
    L = ctypes.CDLL(LIB_PATH)
    i32, i64, dbl, vp, sz = ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t
    ax = ctypes.POINTER(Axis)
    L.aa_abi_version.restype = i32
    L.aa_strerror.argtypes = [i32]
    L.aa_strerror.restype = ctypes.c_char_p
    L.aa_device_count.restype = i32
    L.aa_table_ksize.argtypes = [i32, i32, i64, i64, i32, dbl]
    L.aa_table_ksize.restype = i32
    L.aa_table_bytes.argtypes = [i32, i64, i32]
    L.aa_table_bytes.restype = sz
    L.aa_table_build_bytes.argtypes = [i32, i32, i64, i64, i32, dbl]
    L.aa_table_build_bytes.restype = sz
    L.aa_table_build.argtypes = [i32, i32, i64, i64, i32, dbl, vp, sz, vp]
    L.aa_table_build.restype = i32
    L.aa_table_transposed_ksize.argtypes = [i32, i32, i64, i64, i32, dbl]
    L.aa_table_transposed_ksize.restype = i32
    L.aa_table_transpose.argtypes = [vp, vp, sz, i32, vp]
    L.aa_table_transpose.restype = i32
    L.aa_table_query.argtypes = [vp, ctypes.POINTER(TableHeader), vp]
    L.aa_table_query.restype = i32
    L.aa_table_query2.argtypes = [vp, vp, ctypes.POINTER(TableHeader), ctypes.POINTER(TableHeader), vp]
    L.aa_table_query2.restype = i32
    L.aa_table_build2.argtypes = [i32, i32, i32, i64, i64, ctypes.c_double, vp, sz, i64, i64, ctypes.c_double, vp, sz, vp]
    L.aa_table_build2.restype = i32
    L.aa_workspace_bytes.argtypes = [i32, i32, i64, i64, i64, i64, i64, i64, ax, ax]
    L.aa_workspace_bytes.restype = sz
    L.aa_workspace_bytes_ex.argtypes = [i32, i32, i64, i64, i64, i64, i64, i64, ax, ax, ctypes.c_uint]
    L.aa_workspace_bytes_ex.restype = sz
    L.aa_resample_fwd.argtypes = [vp, vp, vp, sz, i32, i32, i64, i64, i64, i64, ax, ax, vp]
    L.aa_resample_fwd.restype = i32
    L.aa_resample_fwd_ex.argtypes = [vp, vp, vp, sz, i32, i32, i64, i64, i64, i64, ax, ax, ctypes.c_uint, vp]
    L.aa_resample_fwd_ex.restype = i32
    L.aa_resample_fwd_strided.argtypes = [vp, vp, i32, i32, i64, i64, i64, i64, ctypes.POINTER(ctypes.c_int64), ax, ax, ctypes.c_uint, vp]
    L.aa_resample_fwd_strided.restype = i32
    L.aa_resample_bwd.argtypes = [vp, vp, vp, sz, i32, i32, i64, i64, i64, i64, ax, ax, vp]
    L.aa_resample_bwd.restype = i32
    L.aa_resample_bwd_atomic.argtypes = [vp, vp, vp, sz, i32, i32, i64, i64, i64, i64, ax, ax, vp]
    L.aa_resample_bwd_atomic.restype = i32
    L.aa_workspace_bytes_bwd.argtypes = [i32, i32, i64, i64, i64, i64, i64, i64]
    L.aa_workspace_bytes_bwd.restype = sz
    L.aa_resample_axis_fwd.argtypes = [vp, vp, i32, i64, i64, i64, ax, vp]
    L.aa_resample_axis_fwd.restype = i32
    L.aa_last_variant.restype = ctypes.c_char_p
    cvp = ctypes.POINTER(Convert)
    L.aa_workspace_bytes_u8_to_f32.argtypes = [i32, i64, i64, i64, i64, ax, ax, cvp]
    L.aa_workspace_bytes_u8_to_f32.restype = sz
    L.aa_resample_fwd_u8_to_f32.argtypes = [vp, vp, vp, sz, i32, i64, i64, i64, i64, ax, ax, cvp, vp]
    L.aa_resample_fwd_u8_to_f32.restype = i32
    L.aa_probe_copy.argtypes = [vp, vp, sz, i32, vp]
    L.aa_probe_copy.restype = i32
    L.aa_probe_launch_shape.argtypes = [ctypes.POINTER(LaunchShapeIn), ctypes.POINTER(LaunchShapeOut)]
    L.aa_probe_launch_shape.restype = i32
    L.aa_set_launch_shape.argtypes = [i32, i32]
    L.aa_set_launch_shape.restype = i32
    L.aa_last_launch_shape.argtypes = [ctypes.POINTER(LaunchShapeIn), ctypes.POINTER(LaunchShapeOut)]
    L.aa_last_launch_shape.restype = i32
    L.aa_table_ksize_box.argtypes = [i32, i32, i64, i64, dbl, dbl]
    L.aa_table_ksize_box.restype = i32
    L.aa_table_build_bytes_box.argtypes = [i32, i32, i64, i64, dbl, dbl]
    L.aa_table_build_bytes_box.restype = sz
    L.aa_table_build_box.argtypes = [i32, i32, i64, i64, i64, dbl, dbl, vp, sz, i64, i64, i64, dbl, dbl, vp, sz, vp]
    L.aa_table_build_box.restype = i32
    L.aa_reduce_u8.argtypes = [vp, vp, i32, i64, i64, i64, i64, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), i32, i32, vp]
    L.aa_reduce_u8.restype = i32
    L.aa_premultiply_u8.argtypes = [vp, vp, i32, i64, i64, i64, i64, vp]
    L.aa_premultiply_u8.restype = i32
    L.aa_unpremultiply_u8.argtypes = [vp, i32, i64, i64, i64, i64, vp]
    L.aa_unpremultiply_u8.restype = i32
    L.aa_many_desc_bytes.argtypes = [i64]
    L.aa_many_desc_bytes.restype = sz
    L.aa_many_plan.argtypes = [i32, i32, i64, i64, i64, i64, ctypes.POINTER(ManyImage), vp, sz, ctypes.POINTER(sz)]
    L.aa_many_plan.restype = i32
    L.aa_many_desc_bytes_placed.argtypes = [i64]
    L.aa_many_desc_bytes_placed.restype = sz
    L.aa_many_plan_placed.argtypes = [i32, i32, i64, i64, i64, i64, ctypes.POINTER(ManyImage), ctypes.POINTER(ManyPlace),
                                      ctypes.POINTER(ctypes.c_uint8), vp, sz, ctypes.POINTER(sz)]
    L.aa_many_plan_placed.restype = i32
    L.aa_resample_many_u8.argtypes = [vp, vp, i64, i64, i64, i64, i32, vp, vp, sz, vp]
    L.aa_resample_many_u8.restype = i32
    L.aa_resample_many_u8_to_float.argtypes = [vp, vp, i64, i64, i64, i64, i32, vp, vp, sz, cvp, vp]
    L.aa_resample_many_u8_to_float.restype = i32
    L.aa_many_desc_bytes_patches.argtypes = [i64]
    L.aa_many_desc_bytes_patches.restype = sz
    L.aa_many_plan_patches.argtypes = [i32, i32, i64, i64, i64, i64, ctypes.POINTER(ManyImage), ctypes.POINTER(i64), i64, vp, sz,
                                       ctypes.POINTER(sz), ctypes.POINTER(i64)]
    L.aa_many_plan_patches.restype = i32
    L.aa_resample_many_u8_to_patches.argtypes = [vp, vp, vp, vp, sz, cvp, i32, vp]
    L.aa_resample_many_u8_to_patches.restype = i32
    L.aa_reduce_many_desc_bytes.argtypes = [i64]
    L.aa_reduce_many_desc_bytes.restype = sz
    L.aa_reduce_many_plan.argtypes = [i32, i64, i64, ctypes.POINTER(ReduceItem), vp, sz, ctypes.POINTER(sz), ctypes.POINTER(i64)]
    L.aa_reduce_many_plan.restype = i32
    L.aa_reduce_many_u8.argtypes = [vp, vp, vp, sz, vp]
    L.aa_reduce_many_u8.restype = i32
    L.aa_many_desc_bytes_nearest.argtypes = [i64]
    L.aa_many_desc_bytes_nearest.restype = sz
    L.aa_many_plan_nearest.argtypes = [i32, i32, i64, i64, i64, i64, ctypes.POINTER(ManyImage), ctypes.POINTER(ManyPlace),
                                       ctypes.POINTER(ctypes.c_int32), vp, sz, ctypes.POINTER(sz)]
    L.aa_many_plan_nearest.restype = i32
    L.aa_resample_many_nearest.argtypes = [vp, vp, vp, vp, sz, i32, vp]
    L.aa_resample_many_nearest.restype = i32
    L.aa_many_desc_bytes_maps.argtypes = [i64]
    L.aa_many_desc_bytes_maps.restype = sz
    L.aa_many_plan_maps.argtypes = [i32, i32, i64, i64, i64, ctypes.POINTER(ManyImage), ctypes.POINTER(ManyPlace), ctypes.c_double, i32,
                                    vp, sz, ctypes.POINTER(sz)]
    L.aa_many_plan_maps.restype = i32
    L.aa_resample_many_maps.argtypes = [vp, vp, vp, vp, sz, vp]
    L.aa_resample_many_maps.restype = i32
    L.aa_many_desc_bytes_ycbcr.argtypes = [i64]
    L.aa_many_desc_bytes_ycbcr.restype = sz
    L.aa_many_plan_ycbcr.argtypes = [i32, i64, i64, i64, ctypes.POINTER(YccImage), ctypes.POINTER(ManyPlace), ctypes.POINTER(ctypes.c_uint8),
                                     vp, sz, ctypes.POINTER(sz)]
    L.aa_many_plan_ycbcr.restype = i32
    L.aa_resample_many_ycbcr.argtypes = [vp, vp, vp, vp, sz, cvp, i32, vp]
    L.aa_resample_many_ycbcr.restype = i32
    L.aa_ycbcr_to_rgb_u8.argtypes = [vp, vp, i64]
    L.aa_ycbcr_to_rgb_u8.restype = i32
    L.aa_embed_many_desc_bytes.argtypes = [i64]
    L.aa_embed_many_desc_bytes.restype = sz
    L.aa_embed_many_plan.argtypes = [i32, i64, i64, i64, i64, ctypes.POINTER(i64), i64, vp, sz, ctypes.POINTER(sz), ctypes.POINTER(i64)]
    L.aa_embed_many_plan.restype = i32
    L.aa_resample_embed_many.argtypes = [vp, vp, vp, i32, i64, i64, vp, i32, vp, sz, vp]
    L.aa_resample_embed_many.restype = i32
    L.aa_resample_embed_many_bwd.argtypes = [vp, vp, vp, i32, vp, i32, vp, sz, vp]
    L.aa_resample_embed_many_bwd.restype = i32
    L.aa_back_many_desc_bytes.argtypes = [i64]
    L.aa_back_many_desc_bytes.restype = sz
    L.aa_back_many_plan.argtypes = [i32, i32, i64, i64, ctypes.POINTER(BackItemIn), i32, i32, vp, sz, ctypes.POINTER(sz), ctypes.POINTER(sz),
                                    ctypes.POINTER(i64)]
    L.aa_back_many_plan.restype = i32
    L.aa_resample_back_many.argtypes = [vp, vp, i32, ctypes.c_float, vp, sz, vp, sz, vp]
    L.aa_resample_back_many.restype = i32
    L.aa_back_merged_desc_bytes.argtypes = [i64, i64]
    L.aa_back_merged_desc_bytes.restype = sz
    L.aa_back_merged_plan.argtypes = [i32, i32, i64, i64, ctypes.POINTER(BackItemIn), i64, ctypes.POINTER(i64), i32, i32, i32, vp, sz,
                                      ctypes.POINTER(sz), ctypes.POINTER(sz), ctypes.POINTER(i64)]
    L.aa_back_merged_plan.restype = i32
    L.aa_resample_back_merged.argtypes = [vp, vp, i32, ctypes.c_float, vp, sz, vp, sz, vp]
    L.aa_resample_back_merged.restype = i32
    L.aa_back_many_plan_act.argtypes = [i32, i32, i64, i64, ctypes.POINTER(BackItemIn), i32, i32, i32, vp, sz, ctypes.POINTER(sz),
                                        ctypes.POINTER(sz), ctypes.POINTER(i64)]
    L.aa_back_many_plan_act.restype = i32
    L.aa_back_merged_plan_act.argtypes = [i32, i32, i64, i64, ctypes.POINTER(BackItemIn), i64, ctypes.POINTER(i64), i32, i32, i32, i32, vp, sz,
                                          ctypes.POINTER(sz), ctypes.POINTER(sz), ctypes.POINTER(i64)]
    L.aa_back_merged_plan_act.restype = i32
    L.aa_back_many_bwd_desc_bytes.argtypes = [i64]
    L.aa_back_many_bwd_desc_bytes.restype = sz
    L.aa_back_many_bwd_plan.argtypes = [i32, i32, i64, i64, ctypes.POINTER(BackBwdItemIn), i32, i32, vp, sz, ctypes.POINTER(sz), ctypes.POINTER(sz),
                                        ctypes.POINTER(i64)]
    L.aa_back_many_bwd_plan.restype = i32
    L.aa_resample_back_many_bwd.argtypes = [vp, vp, i32, vp, sz, vp, sz, vp]
    L.aa_resample_back_many_bwd.restype = i32
    L.aa_set_fused.argtypes = [i32]
    L.aa_set_fused.restype = i32
    L.aa_set_store_form.argtypes = [i32]
    L.aa_set_store_form.restype = i32
    L.aa_set_plane_groups.argtypes = [i32]
    L.aa_set_plane_groups.restype = i32
    if L.aa_abi_version() != 3:
        raise AAInterpError("libaa_interp.so ABI version mismatch")
    _lib = L
    return L


def strerror(rc: int) -> str:
    return load().aa_strerror(rc).decode()


def check(rc: int, what: str = "") -> None:
    if rc < 0:
        msg = f"{what}: {strerror(rc)} (aa_status {rc})" if what else f"{strerror(rc)} (aa_status {rc})"
        if rc == ERR_BAD_DTYPE:
            raise NotImplementedError(msg)
        raise AAInterpError(msg)


fused_epoch = 0  # bumped by set_fused: host-side plans that cached a workspace size are keyed on it


def set_fused(enabled: int) -> int:
    """Enable/disable the fused kernels (process-wide); returns the previous setting."""
    global fused_epoch
    fused_epoch += 1
    return int(load().aa_set_fused(int(enabled)))


def set_store_form(form: int) -> int:
    """Test hook: -1 automatic, 0 never / 1 always the streaming store forms of the up-scaling / backward kernel; returns the previous setting."""
    return int(load().aa_set_store_form(int(form)))


def set_plane_groups(enabled: int) -> int:
    """Test / A-B hook: 1 (default) planar three-channel uint8 images run all three planes in one wave, 0 one wave per plane; returns the
    previous setting."""
    return int(load().aa_set_plane_groups(int(enabled)))


def last_variant() -> str:
    return load().aa_last_variant().decode()


def set_launch_shape(spb: int = 0, ybands: int = 0):
    """Test hook: strips per workgroup and row bands of the fused launches (process-wide), 0 = the model chooses; a request the kernels are
    not written for is not looked at (include/aa_interp.h has the rules).  Returns the previous setting as (spb, ybands)."""
    prev = int(load().aa_set_launch_shape(int(spb), int(ybands)))
    return prev & 0xFF, prev >> 8


def last_launch_shape():
    """(LaunchShapeIn, LaunchShapeOut) of this thread's last fused launch, or None when the last call launched no fused kernel."""
    q, out = LaunchShapeIn(), LaunchShapeOut()
    rc = load().aa_last_launch_shape(ctypes.byref(q), ctypes.byref(out))
    if rc == ERR_BAD_SHAPE:
        return None
    check(rc, "aa_last_launch_shape")
    return q, out


# sources a kernel variant is compiled from (csrc/): profiles/*.json summaries are stamped with their fingerprint, and bench.py
# flags a committed counter summary as stale when the sources of the kernel it describes have changed since
KERNEL_SOURCES = {
    "fused_u8_nhwc_pil_v3": ("aa_fused_u8_v3_impl.h", "aa_fused_u8_v3.hip", "aa_fused_u8_v3_unit.hip", "aa_fused_u8_v3_list.h", "aa_common.h"),
    "fused_u8_nhwc_pil": ("aa_fused_u8.hip", "aa_common.h"),
    "fused_u8_planar_pil_v3": ("aa_fused_u8_v3_impl.h", "aa_fused_u8_v3.hip", "aa_fused_u8_v3_unit.hip", "aa_fused_u8_v3_list.h", "aa_common.h"),
}


def source_fingerprint(variant: str):
    """sha256[:12] over the source files of `variant` (None for a variant without an entry in KERNEL_SOURCES)."""
    import hashlib

    names = KERNEL_SOURCES.get(variant)
    if not names:
        return None
    h = hashlib.sha256()
    for n in names:
        with open(os.path.join(_HERE, "csrc", n), "rb") as f:
            h.update(n.encode() + b"\0" + f.read())
    return h.hexdigest()[:12]
