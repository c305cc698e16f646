"""Shared by the GPU tests: the `aa` and `lib` fixtures, the knobs' context manager, inputs moved to the GPU in a layout class, comparison
by bit patterns, torch's definition of the converting calls, the launch count, the one-axis oracle, and the rule that nothing more is
launched once the GPU has reported an error.  A new GPU test file starts from here (and from kit_golden.py).  Not a test module, not a
plugin: a test module binds the fixtures it wants at module level, ``aa = kit_gpu.aa_fixture()``."""
import contextlib

import numpy as np
import pytest
import torch

import oracle
from kit_golden import MEAN, STD

from interpolate_antialiasing_amd import extension_interpolate as _aa

FORWARD = {"linear": _aa.linear_forward, "cubic": _aa.cubic_forward, "box": _aa.nearest_forward, "hamming": _aa.hamming_forward,
           "lanczos": _aa.lanczos_forward}


# ---- fixtures --------------------------------------------------------------------------------------------------------------------------
def aa_fixture(report=None):
    """The module-scoped fixture `aa`: skips without a GPU, yields the package's extension_interpolate, then calls report() (a module's
    summary print, or what it has to put back)."""
    @pytest.fixture(scope="module", name="aa")
    def aa():
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        from interpolate_antialiasing_amd import extension_interpolate

        yield extension_interpolate
        if report is not None:
            report()

    return aa


def lib_fixture():
    """The module-scoped fixture `lib`: the package's _lib, behind `aa`'s skip."""
    @pytest.fixture(scope="module", name="lib")
    def lib(aa):
        from interpolate_antialiasing_amd import _lib

        return _lib

    return lib


class Knobs:
    """set_fused / set_store_form / set_plane_groups for one block, restored on the way out."""

    def __init__(self, fused=1, store=-1, groups=1):
        self.want = (fused, store, groups)

    def __enter__(self):
        from interpolate_antialiasing_amd import _lib

        self.prev = (_lib.set_fused(self.want[0]), _lib.set_store_form(self.want[1]), _lib.set_plane_groups(self.want[2]))

    def __exit__(self, *exc):
        from interpolate_antialiasing_amd import _lib

        _lib.set_fused(self.prev[0])
        _lib.set_store_form(self.prev[1])
        _lib.set_plane_groups(self.prev[2])


@contextlib.contextmanager
def gpu_error_ends_the_session(tag):
    """After the GPU reports an error, launch nothing more: a HIP error or an illegal memory access that is not the package's own
    AAInterpError ends the whole pytest session with exit status 3.  Every other exception passes through."""
    from interpolate_antialiasing_amd import _lib

    try:
        yield
    except RuntimeError as e:
        if not isinstance(e, _lib.AAInterpError) and ("HIP error" in str(e) or "illegal memory access" in str(e)):
            pytest.exit(f"the GPU reported an error in {tag}; nothing more is launched: {e}", returncode=3)
        raise


# ---- inputs on the GPU -----------------------------------------------------------------------------------------------------------------
def to_gpu(x_chw, cls):
    """[C, H, W] numpy -> a GPU tensor [C, H, W] lying in memory as the class says (a copy: the shared inputs are read-only)."""
    if cls == "interleaved":
        return torch.from_numpy(np.array(x_chw.transpose(1, 2, 0), order="C")).cuda().permute(2, 0, 1)
    return torch.from_numpy(np.array(x_chw, order="C")).cuda()


def batch_or_list(items, is_batch, cls):
    """A case's [C, H, W] items as the call takes them: the list, or one [N, C, H, W] tensor in the class's memory format for a batch case."""
    if is_batch:
        x = torch.stack(items)
        return x.contiguous(memory_format=torch.channels_last) if cls == "interleaved" else x.contiguous()
    return items


def nchw_gpu(a, channels_last=False):
    """[N, C, H, W] numpy -> the GPU tensor, planar or channels_last (a copy: the cached inputs are read-only)."""
    t = torch.from_numpy(np.array(a, order="C")).cuda()
    return t.contiguous(memory_format=torch.channels_last) if channels_last else t


def image_gpu(img_hwc, channels_last):
    """One [H, W, C] numpy image -> the [1, C, H, W] GPU tensor, in channels_last storage or planar."""
    t = torch.from_numpy(np.ascontiguousarray(img_hwc)[None]).cuda().permute(0, 3, 1, 2)
    return t if channels_last else t.contiguous()


def hwc(t):
    """A [C, H, W] tensor -> the [H, W, C] numpy array."""
    return np.ascontiguousarray(t.permute(1, 2, 0).cpu().numpy())


def pitched_crop(x_chw, cls, k):
    """The image as a crop of a larger padded buffer: an odd byte offset and a row pitch that is no multiple of 4."""
    c, h, w = x_chw.shape
    off = 1 + 2 * (k % 2)
    if cls == "interleaved":
        pitch = w * c + 5
        pitch += 1 if pitch % 4 == 0 else 0
        buf = torch.full((off + h * pitch + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        v = buf.as_strided((c, h, w), (1, pitch, c), off)
    else:
        pitch = w + 6
        pitch += 1 if pitch % 4 == 0 else 0
        plane = h * pitch + 7
        buf = torch.full((off + c * plane + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        v = buf.as_strided((c, h, w), (plane, pitch, 1), off)
    assert pitch % 4 != 0 and v.data_ptr() % 2 == 1
    v.copy_(torch.from_numpy(np.ascontiguousarray(x_chw)).cuda())
    return v


# ---- comparing bits --------------------------------------------------------------------------------------------------------------------
def bits(t):
    """A tensor's bit patterns on the CPU, as the integer dtype of its element size."""
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def assert_bits(got, want, what, explain=None):
    """Same dtype, same shape, same bits.  explain(index of the first differing element) -> more words for the message."""
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (what, got.dtype, tuple(got.shape), want.dtype, tuple(want.shape))
    a, b = bits(got), bits(want)
    if not torch.equal(a, b):
        bad = (a != b).nonzero()
        at = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {a.numel()} elements differ from the reference, first at {list(at)}: "
                             f"{got.cpu()[at].item()!r} != {want.cpu()[at].item()!r}" + (f"; {explain(at)}" if explain is not None else ""))


# ---- other shared checks ---------------------------------------------------------------------------------------------------------------
def assert_class_format(y, cls, c):
    if c > 1:
        assert y.is_contiguous(memory_format=torch.channels_last) == (cls == "interleaved") and y.is_contiguous() == (cls == "planar")
    else:
        assert y.is_contiguous()


def check_against_fixture(ref, items, name, f, y, restated=None):
    """y, a call's whole uint8 result [N, C, oH, oW] of fixture case `name` under filter f: its shape and dtype, then every item against
    ref's fixture; restated(name, f), where given, is the CPU restatement's batch, which y equals too.  items: where the case's record
    keeps its items."""
    cs = ref.gen().case(name)
    assert tuple(y.shape) == (len(cs[items]), cs[1]) + tuple(cs[2]) and y.dtype == torch.uint8
    got = y.cpu()
    for i in range(len(cs[items])):
        ref.assert_matches_fixture(f"{name}/{f}/{i}", ref.item(name, i), got[i].permute(1, 2, 0).numpy())
    if restated is not None:
        assert torch.equal(got, restated(name, f)), (name, f)


def convert(b, dtype, norm=True, flips=None):
    """The converting calls' definition, by torch on the CPU: b [N, C, oH, oW] uint8 -> ((b.float() - mean) / std).to(dtype), the
    flagged items mirrored."""
    c = b.shape[1]
    f = b.float()
    if norm:
        f = (f - torch.tensor(MEAN[:c]).view(1, c, 1, 1)) / torch.tensor(STD[:c]).view(1, c, 1, 1)
    y = f.to(dtype)
    if flips is not None:
        y = torch.stack([y[i].flip(-1) if flips[i] else y[i] for i in range(len(flips))])
    return y


def count_launches(fn):
    """Kernel launches of one fn() from torch's profiler (tools/resize_many_bench.py count_launches)."""
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
            and "memset" not in e.name.lower()]


def oracle_axis(filt, a, axis, n_out, align_corners=False):
    """One separable pass along `axis` with the 2-D oracle: the axis becomes W of an [outer, inner, 1, n] image (the
    H pass is 1 -> 1, a single tap of weight exactly 1)."""
    moved = np.moveaxis(a, axis, -1)
    lead = moved.shape[:-1]
    img = np.ascontiguousarray(moved.reshape(-1, 1, 1, moved.shape[-1]))
    out = oracle.forward(filt, img, (1, n_out), align_corners)
    return np.moveaxis(out.reshape(*lead, n_out), -1, axis)
