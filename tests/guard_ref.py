"""A guarded allocator for the Python shim, shared by test_guard_cpu.py and test_guard_gpu.py.  Not a test module.

Every buffer the shim hands to a kernel (outputs, workspaces, the ragged call's descriptor, weight tables, N-d intermediates) comes from
``torch.empty`` in extension_interpolate.py and tables.py, and both modules look ``torch`` up as a module global when they call it.
``guarded()`` puts a proxy there that forwards every attribute to the real torch except ``empty``.  A guarded ``empty``:

  * allocates a flat uint8 base of  GUARD + lead + nbytes + GUARD  bytes and fills all of it with one byte value — 0xFF by default, NaN
    in float16, bfloat16, float32 and float64; 0x00 on request (two runs with different fills show which uint8 bytes were never written);
  * returns a view of the body with the shape, dtype, strides and contiguity torch.empty gives, channels_last included;
  * keeps the base alive until ``check()`` (the shim drops its workspaces as soon as the launch is enqueued, and the caching allocator
    would hand the memory to the next request).

Placement: a flat 1-D uint8 buffer (workspace, descriptor, table) always starts GUARD bytes into the base, on a 256-byte boundary (the
C-ABI asks 16 of a workspace and 8 of a descriptor).  Every other allocation is an output and starts ``lead`` ELEMENTS later: 0 keeps the
alignment the caching allocator gives today, 1 puts a uint8 output on an odd byte, a 16-bit one on a 2-byte-only and a float32 one on a
4-byte-only boundary — all inside the contract of include/aa_interp.h (element-aligned outputs are served).

``check()`` synchronises and asserts that every byte outside every body still holds the fill, naming the allocation (call order, shape,
dtype), the side and the first and last byte touched: before the body as negative offsets from its first byte (-1 is the byte just before
it), after the body as offsets from its end (0 is the byte just after it).
"""
from __future__ import annotations

import collections
import contextlib

import torch as _torch

GUARD = 16384   # bytes on each side: wider than any row tile of the kernels (4 KiB in reduce, 8 KiB chunks in the ragged call)
ALIGN = 256     # a flat uint8 buffer's body starts on this boundary


class GuardViolation(AssertionError):
    pass


class Record:
    __slots__ = ("order", "base", "body", "off", "nbytes", "shape", "dtype", "flat")

    def __init__(self, order, base, body, off, nbytes, shape, dtype, flat):
        self.order, self.base, self.body, self.off, self.nbytes = order, base, body, off, nbytes
        self.shape, self.dtype, self.flat = shape, dtype, flat

    def __repr__(self):
        return f"allocation #{self.order} {list(self.shape)} {self.dtype}"


def _memory_format_strides(shape, memory_format):
    return _torch.empty(shape, dtype=_torch.uint8, device="meta", memory_format=memory_format).stride()


class Recorder:
    """The guarded ``empty`` and its book of allocations.  lead: elements an output's body starts after the guard; fill: 0xFF or 0x00;
    devices: the device types that are guarded (the CPU tests of this helper guard "cpu"), every other one passes through, as do pinned
    and empty allocations."""

    def __init__(self, lead: int = 0, fill: int = 0xFF, devices=("cuda",)):
        if fill not in (0xFF, 0x00):
            raise ValueError("fill is 0xFF or 0x00")
        if lead not in (0, 1):
            raise ValueError("lead is 0 or 1 element")
        self.lead, self.fill, self.devices = lead, fill, tuple(devices)
        self.records = []
        self.proxy = _Proxy(self)

    # ---- torch.empty ---------------------------------------------------------------------------------------------------------------
    def empty(self, *size, dtype=None, device=None, memory_format=_torch.contiguous_format, pin_memory=False, **kw):
        if len(size) == 1 and not isinstance(size[0], int):
            size = tuple(size[0])
        shape = tuple(int(v) for v in size)
        dev = _torch.device(device) if device is not None else _torch.tensor([]).device
        numel = 1
        for v in shape:
            numel *= v
        if dev.type not in self.devices or pin_memory or numel == 0 or kw:
            return _torch.empty(shape, dtype=dtype, device=device, memory_format=memory_format, pin_memory=pin_memory, **kw)
        dtype = dtype if dtype is not None else _torch.get_default_dtype()
        return self.alloc(shape, dtype, dev, memory_format)

    def alloc(self, shape, dtype, device, memory_format=_torch.contiguous_format):
        """One guarded allocation, whatever the device."""
        es = _torch.empty((), dtype=dtype).element_size()
        numel = 1
        for v in shape:
            numel *= v
        nbytes = numel * es
        flat = len(shape) == 1 and dtype == _torch.uint8
        lead = 0 if flat else self.lead * es
        base = _torch.empty(GUARD + lead + nbytes + GUARD, dtype=_torch.uint8, device=device)
        assert not base.is_cuda or base.data_ptr() % ALIGN == 0, "the caching allocator's blocks start on 256-byte boundaries"
        base.fill_(self.fill)
        off = GUARD + lead
        body = base[off:off + nbytes].view(dtype).as_strided(shape, _memory_format_strides(shape, memory_format))
        self.records.append(Record(len(self.records), base, body, off, nbytes, shape, dtype, flat))
        return body

    # ---- the check -----------------------------------------------------------------------------------------------------------------
    def violations(self):
        """[(record, side, first offset, last offset, bytes touched)] over every allocation so far (synchronises first)."""
        if any(r.base.is_cuda for r in self.records):
            _torch.cuda.synchronize()
        found = []
        for r in self.records:
            before = (r.base[:r.off] != self.fill).nonzero().flatten()
            if before.numel():
                found.append((r, "before", int(before[0]) - r.off, int(before[-1]) - r.off, int(before.numel())))
            after = (r.base[r.off + r.nbytes:] != self.fill).nonzero().flatten()
            if after.numel():
                found.append((r, "after", int(after[0]), int(after[-1]), int(after.numel())))
        return found

    def check(self):
        """Assert that no byte outside a body was written; -> the bodies in allocation order."""
        found = self.violations()
        if found:
            raise GuardViolation("; ".join(f"{r!r}: {n} byte(s) written {side} the body, offsets {lo} .. {hi}" for r, side, lo, hi, n in found))
        return [r.body for r in self.records]

    def outputs(self):
        """The bodies that are not flat uint8 buffers (outputs and N-d intermediates), in allocation order."""
        return [r.body for r in self.records if not r.flat]

    def record_of(self, t):
        """The record whose body starts where tensor t starts (None: t did not come from this allocator)."""
        for r in self.records:
            if r.nbytes and r.body.data_ptr() == t.data_ptr():
                return r
        return None


class _Proxy:
    """torch, with a guarded ``empty``."""

    def __init__(self, recorder):
        object.__setattr__(self, "_recorder", recorder)

    def __getattr__(self, name):
        if name == "empty":
            return object.__getattribute__(self, "_recorder").empty
        return getattr(_torch, name)

    def __setattr__(self, name, value):
        raise AttributeError("the proxy is read-only")


# ---- "every element was written" ------------------------------------------------------------------------------------------------------
def unwritten_float(t) -> int:
    """Elements of a float tensor that still hold the 0xFF fill's NaN (inputs were finite, so a NaN is an element no kernel stored)."""
    return int(_torch.isnan(t).sum())


def unwritten_u8(filled_ff, filled_00) -> int:
    """Bytes that differ between the run into 0xFF-filled and the run into 0x00-filled memory: never written (each shows its own fill)."""
    return int((filled_ff != filled_00).sum())


@contextlib.contextmanager
def guarded(monkeypatch, lead: int = 0, fill: int = 0xFF):
    """The shim under the guarded allocator: extension_interpolate and tables see the proxy as ``torch``, and the table caches and the
    plan cache are empty containers of their own types, so that every table of the call is built into a guarded buffer.  Everything is
    put back on the way out."""
    from interpolate_antialiasing_amd import extension_interpolate, tables

    rec = Recorder(lead, fill)
    with monkeypatch.context() as m:
        m.setattr(extension_interpolate, "torch", rec.proxy)
        m.setattr(tables, "torch", rec.proxy)
        m.setattr(tables, "_cache", {})
        m.setattr(tables, "_box_cache", collections.OrderedDict())
        m.setattr(extension_interpolate, "_plans", {})
        yield rec
