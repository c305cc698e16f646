"""Weight tables: device-side precompute, host-side cache, pack/unpack for the one RCCL broadcast.

A table replaces what HelperInterpBase::_compute_indices_weights_aa returns (reference
step_two_dot_two/aa_interpolation_impl.h:195-281: xmin, size, stride, weights, weight-index tensors, recomputed
on every call and every pass).  Here it is ONE packed device buffer per (filter, kind, in, out, align_corners,
scale, device), built once by a HIP kernel and cached.
"""
from __future__ import annotations

import collections
import ctypes
import threading
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch

from . import _lib

FILTER_IDS = _lib.FILTER_IDS
KIND_IDS = {"pil": _lib.TABLE_PIL, "f32": _lib.TABLE_F32, "f64": _lib.TABLE_F64}
HEADER_BYTES = ctypes.sizeof(_lib.TableHeader)  # 64

# fixed-length int64 descriptor broadcast ahead of the payload so receivers can allocate
META_LEN = 16


def _stream_ptr(device: torch.device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


@dataclass
class WeightTable:
    """One packed table.  ``buf`` is a uint8 tensor: on the GPU when used by kernels, possibly on the CPU while
    it is only being transported (tests with the gloo backend)."""
    buf: torch.Tensor
    filter: int
    kind: int
    in_size: int
    out_size: int
    ksize: int
    max_taps: int
    align_corners: bool = False
    transposed: bool = False
    scatter_off: int = 0
    scatter_ksize: int = 0
    scatter_max: int = 0
    span64p1: int = 0  # 1 + the widest spread of 64 consecutive outputs' window starts (measured on device; 0 = unknown)
    span4p1: int = 0   # the same over 4 consecutive outputs
    gather_off: int = 0  # byte offset of the per-output gather records (F32 and Pillow tables)
    box: bool = False  # a box table (get_box_table_pair): in_size is the hull's length, xmin[] are relative to the hull's origin

    def axis(self) -> _lib.Axis:
        if not self.buf.is_cuda:
            raise _lib.AAInterpError("weight table is not on a GPU")
        return _lib.Axis(ctypes.c_void_p(self.buf.data_ptr()), self.in_size, self.out_size, self.ksize, self.max_taps,
                         self.kind, self.filter, self.scatter_off, self.scatter_ksize, self.scatter_max, self.span64p1, self.span4p1, self.gather_off,
                         (ctypes.c_int32 * 2)(1 if self.box else 0, 0))

    # ---- transport -----------------------------------------------------------------------------------
    def meta(self) -> torch.Tensor:
        return torch.tensor([0x42544141, self.filter, self.kind, self.in_size, self.out_size, self.ksize,
                             self.max_taps, int(self.align_corners), int(self.transposed), self.buf.numel(),
                             self.scatter_off, self.scatter_ksize, self.scatter_max, self.span64p1, self.span4p1, self.gather_off],
                            dtype=torch.int64)

    @staticmethod
    def from_meta(meta: torch.Tensor, buf: torch.Tensor) -> "WeightTable":
        m = [int(v) for v in meta.tolist()]
        if m[0] != 0x42544141 or len(m) != META_LEN:
            raise _lib.AAInterpError("bad weight-table descriptor")
        if buf.numel() != m[9]:
            raise _lib.AAInterpError("weight-table payload size mismatch")
        return WeightTable(buf=buf, filter=m[1], kind=m[2], in_size=m[3], out_size=m[4], ksize=m[5], max_taps=m[6],
                           align_corners=bool(m[7]), transposed=bool(m[8]), scatter_off=m[10], scatter_ksize=m[11],
                           scatter_max=m[12], span64p1=m[13], span4p1=m[14], gather_off=m[15])

    # ---- inspection (tests) ----------------------------------------------------------------------------
    def unpack_scatter(self):
        """-> (first int32[in], count int32[in], w [in, 6], completes int32[in]) (CPU numpy).  Record layout by table kind
        (include/aa_interp.h): PIL / F32 tables 32 bytes {int32 first, int32 count | completes << 16, int32 / float w[6]};
        F64 tables 64 bytes {int32 first, int32 count | completes << 16, double w[6], 8 bytes padding}."""
        import numpy as np

        if not self.scatter_off:
            return None
        raw = self.buf.detach().cpu().numpy()
        n, off = self.in_size, self.scatter_off
        if self.kind == _lib.TABLE_F64:
            blk = raw[off:off + 64 * n].reshape(n, 64)
            head = blk[:, :8].copy().view(np.int32).reshape(n, 2)
            w = blk[:, 8:56].copy().view(np.float64).reshape(n, 6)
            return head[:, 0], head[:, 1] & 0xFFFF, w, head[:, 1] >> 16
        rec = raw[off:off + 32 * n].view(np.int32).reshape(n, 8).copy()
        w = rec[:, 2:] if self.kind == _lib.TABLE_PIL else rec[:, 2:].copy().view(np.float32)
        return rec[:, 0], rec[:, 1] & 0xFFFF, w, rec[:, 1] >> 16

    def unpack(self):
        """-> (xmin int32[out], xsize int32[out], w [out,ksize]) as CPU numpy arrays."""
        import numpy as np

        raw = self.buf.detach().cpu().numpy()
        out, k = self.out_size, self.ksize
        xmin = raw[HEADER_BYTES:HEADER_BYTES + 4 * out].view(np.int32).copy()
        xsize = raw[HEADER_BYTES + 4 * out:HEADER_BYTES + 8 * out].view(np.int32).copy()
        woff = (HEADER_BYTES + 8 * out + 15) & ~15
        wdt = {_lib.TABLE_PIL: np.int32, _lib.TABLE_F32: np.float32, _lib.TABLE_F64: np.float64}[self.kind]
        w = raw[woff:woff + out * k * np.dtype(wdt).itemsize].view(wdt).reshape(out, k).copy()
        return xmin, xsize, w


_cache: Dict[Tuple, WeightTable] = {}
_cache_lock = threading.Lock()


def clear_cache() -> None:
    with _cache_lock:
        _cache.clear()
        _box_cache.clear()


def cache_key(filter_id: int, kind: int, in_size: int, out_size: int, align_corners: bool, scale: float,
              device: torch.device, transposed: bool = False) -> Tuple:
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else (torch.cuda.current_device() if dev.type == "cuda" else -1)
    return (int(filter_id), int(kind), int(in_size), int(out_size), bool(align_corners), float(scale or 0.0),
            dev.type, idx, bool(transposed))


def _from_header(buf, filter_id, kind, in_size, out_size, k, align_corners, hdr, transposed=False) -> WeightTable:
    """A table from its arguments and what the device measured into its header (a transposed table's scatter fields are 0 there)."""
    return WeightTable(buf, filter_id, kind, in_size, out_size, k, int(hdr.max_taps), bool(align_corners), transposed,
                       int(hdr.scatter_off), int(hdr.scatter_ksize), int(hdr.scatter_max), int(hdr.span64p1), int(hdr.span4p1), int(hdr.gather_off))


def _read_headers(L, ptrs, s):
    """The headers of one or two tables just built on stream ``s``: one synchronisation either way."""
    hdrs = [_lib.TableHeader() for _ in ptrs]
    if len(ptrs) == 1:
        _lib.check(L.aa_table_query(ptrs[0], ctypes.byref(hdrs[0]), s), "aa_table_query")
    else:
        _lib.check(L.aa_table_query2(ptrs[0], ptrs[1], ctypes.byref(hdrs[0]), ctypes.byref(hdrs[1]), s), "aa_table_query2")
    return hdrs


def _table_alloc(nbytes: int, device: torch.device) -> torch.Tensor:
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _build(filter_id: int, kind: int, axes, align_corners: bool, device: torch.device, alloc=_table_alloc, box: bool = False):
    """Uncached device-side build of the one or two tables of ``axes``: one build call and one header read-back whichever.  A plain axis
    is (in_size, out_size, scale); a box axis (always two) is get_box_table_pair's (origin, hull, out_size, in0, in1)."""
    L = _lib.load()
    ac = int(align_corners)
    if box:
        ksize, nbytes, what = L.aa_table_ksize_box, L.aa_table_build_bytes_box, "aa_table_ksize_box"
        sized = [(n, n_out, (n, n_out, in0, in1)) for _, n, n_out, in0, in1 in axes]
    else:
        ksize, nbytes, what = L.aa_table_ksize, L.aa_table_build_bytes, "aa_table_ksize"
        axes = [(n, n_out, float(scale or 0.0)) for n, n_out, scale in axes]
        sized = [(n, n_out, (n, n_out, ac, scale)) for n, n_out, scale in axes]
    ks = []
    for _, _, args in sized:
        ks.append(ksize(filter_id, kind, *args))
        _lib.check(ks[-1], what)
    nb = [nbytes(filter_id, kind, *args) for _, _, args in sized]
    with torch.cuda.device(device):
        bufs = [alloc(n, device) for n in nb]
        ptrs = [ctypes.c_void_p(b.data_ptr()) for b in bufs]
        s = _stream_ptr(device)
        if box:
            _lib.check(L.aa_table_build_box(filter_id, kind, *axes[0], ptrs[0], nb[0], *axes[1], ptrs[1], nb[1], s), "aa_table_build_box")
        elif len(axes) == 2:
            _lib.check(L.aa_table_build2(filter_id, kind, ac, *axes[0], ptrs[0], nb[0], *axes[1], ptrs[1], nb[1], s), "aa_table_build2")
        else:
            n, n_out, scale = axes[0]
            _lib.check(L.aa_table_build(filter_id, kind, n, n_out, ac, scale, ptrs[0], nb[0], s), "aa_table_build")
        hdrs = _read_headers(L, ptrs, s)
    out = [_from_header(buf, filter_id, kind, n, n_out, k, align_corners, hdr) for buf, (n, n_out, _), k, hdr in zip(bufs, sized, ks, hdrs)]
    for t in out:
        t.box = box
    return out


def build_table(filter_id: int, kind: int, in_size: int, out_size: int, align_corners: bool, scale: float,
                device: torch.device) -> WeightTable:
    """Uncached device-side build (one launch + one 64-byte header read-back)."""
    return _build(filter_id, kind, [(in_size, out_size, scale)], align_corners, device)[0]


def get_table_pair(filter_id: int, kind: int, in_h: int, out_h: int, in_w: int, out_w: int, align_corners: bool, scale_h: float, scale_w: float,
                   device: torch.device):
    """The two tables of a 2-D call.  When BOTH are new (a shape never seen: every call of a random-crop pipeline) they are built
    back to back and their headers read with one synchronisation instead of two."""
    device = torch.device(device)
    kh = cache_key(filter_id, kind, in_h, out_h, align_corners, scale_h, device)
    kw = cache_key(filter_id, kind, in_w, out_w, align_corners, scale_w, device)
    with _cache_lock:
        th, tw = _cache.get(kh), _cache.get(kw)
    if th is None and tw is None and kh != kw:
        th, tw = _build(filter_id, kind, [(in_h, out_h, scale_h), (in_w, out_w, scale_w)], align_corners, device)
        with _cache_lock:
            _cache[kh], _cache[kw] = th, tw
        return th, tw
    if th is None:
        th = get_table(filter_id, kind, in_h, out_h, align_corners, scale_h, device)
    if tw is None:
        tw = get_table(filter_id, kind, in_w, out_w, align_corners, scale_w, device)
    return th, tw


# ---- box tables (Image.resize(box=...)) -----------------------------------------------------------------------------------------
# Random boxes never repeat, so their tables stay out of `_cache` (which never forgets): a small LRU of their own.  An evicted table's
# buffer goes back to the caching allocator only after the launch that used it was enqueued (the caller holds the pair until then),
# and the stream orders every later use of that memory behind it.
# Buffers come in size classes (a power of two, 16 KiB at least), so what the full LRU holds does not drift with the boxes' sizes.
BOX_CACHE_SIZE = 32
BOX_TABLE_MIN_BYTES = 16384


def _box_table_alloc(nbytes: int, device: torch.device) -> torch.Tensor:
    return torch.empty(max(BOX_TABLE_MIN_BYTES, 1 << max(int(nbytes) - 1, 0).bit_length()), dtype=torch.uint8, device=device)

_box_cache: "collections.OrderedDict[Tuple, Tuple[WeightTable, WeightTable]]" = collections.OrderedDict()


def get_box_table_pair(filter_id: int, axis_h: Tuple[int, int, int, float, float], axis_w: Tuple[int, int, int, float, float],
                       device: torch.device):
    """The two AA_TABLE_PIL box tables of a call: ONE launch and ONE header read-back.  axis_* = (origin, hull, out_size, in0, in1):
    Pillow's source interval [in0, in1) of the axis and the hull [origin, origin + hull) of its windows (boxmath.axis_hull); an axis
    without a box is (0, in_size, out_size, 0.0, in_size)."""
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    key = (int(filter_id), tuple(axis_h), tuple(axis_w), idx)
    with _cache_lock:
        pair = _box_cache.get(key)
        if pair is not None:
            _box_cache.move_to_end(key)
            return pair
    th, tw = _build(filter_id, _lib.TABLE_PIL, [tuple(axis_h), tuple(axis_w)], False, device, _box_table_alloc, box=True)
    with _cache_lock:
        _box_cache[key] = (th, tw)
        while len(_box_cache) > BOX_CACHE_SIZE:
            _box_cache.popitem(last=False)
    return th, tw


def get_table(filter_id: int, kind: int, in_size: int, out_size: int, align_corners: bool = False, scale: float = 0.0,
              device: Optional[torch.device] = None) -> WeightTable:
    device = torch.device(device if device is not None else "cuda")
    key = cache_key(filter_id, kind, in_size, out_size, align_corners, scale, device)
    with _cache_lock:
        t = _cache.get(key)
    if t is None:
        t = build_table(filter_id, kind, in_size, out_size, align_corners, scale, device)
        with _cache_lock:
            _cache[key] = t
    return t


def put_table(t: WeightTable, scale: float = 0.0) -> None:
    """Install a table received from another rank into this rank's cache."""
    key = cache_key(t.filter, t.kind, t.in_size, t.out_size, t.align_corners, scale, t.buf.device, t.transposed)
    with _cache_lock:
        _cache[key] = t


def get_transposed_table(fwd: WeightTable, scale: float = 0.0) -> WeightTable:
    """Adjoint (gather-form) table of ``fwd``: in/out swapped, built on device, cached."""
    device = fwd.buf.device
    key = cache_key(fwd.filter, fwd.kind, fwd.in_size, fwd.out_size, fwd.align_corners, scale, device, True)
    with _cache_lock:
        t = _cache.get(key)
    if t is not None:
        return t
    L = _lib.load()
    tk = L.aa_table_transposed_ksize(fwd.filter, fwd.kind, fwd.in_size, fwd.out_size, int(fwd.align_corners), float(scale or 0.0))
    _lib.check(tk, "aa_table_transposed_ksize")
    nbytes = L.aa_table_bytes(fwd.kind, fwd.in_size, tk)
    with torch.cuda.device(device):
        buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        s = _stream_ptr(device)
        _lib.check(L.aa_table_transpose(ctypes.c_void_p(fwd.buf.data_ptr()), ctypes.c_void_p(buf.data_ptr()), nbytes, tk, s),
                   "aa_table_transpose")
        hdr, = _read_headers(L, [ctypes.c_void_p(buf.data_ptr())], s)
    if int(hdr.max_taps) > tk:  # (aa_table_transpose refuses this itself: a table whose rows dropped taps is never cached)
        raise _lib.AAInterpError(f"transposed weight table: an input index feeds {int(hdr.max_taps)} outputs but rows hold {tk} "
                                 f"(filter {fwd.filter}, {fwd.in_size} -> {fwd.out_size})")
    t = _from_header(buf, fwd.filter, fwd.kind, fwd.out_size, fwd.in_size, tk, fwd.align_corners, hdr, transposed=True)
    with _cache_lock:
        _cache[key] = t
    return t
