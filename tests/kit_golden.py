"""Shared by the CPU tests and the *_ref modules: the fixture generators (tests/golden/make_golden_<stem>.py) and the fixtures they made
(tests/golden/<stem>.npz), each loaded once for the whole session; the read-only form of a shared input; the three assertions that hold
an output to a fixture entry of CRC-32s and sampled pixels; and the constants every call's tests use.  numpy only: no torch, no GPU, no
built library.  A new test file starts from here (and from kit_gpu.py if it runs on the GPU).  Not a test module."""
import functools
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MODE = {"linear": "bilinear", "cubic": "bicubic", "box": "box", "hamming": "hamming", "lanczos": "lanczos"}  # filter -> the calls' mode
MEAN = [123.675, 116.28, 103.53, 127.5]
STD = [58.395, 57.12, 57.375, 64.0]


@functools.lru_cache(maxsize=None)
def generator(stem):
    """tests/golden/make_golden_<stem>.py as a module: one instance for all callers (the generators build constant case lists at import
    and nothing changes them afterwards)."""
    spec = importlib.util.spec_from_file_location(f"make_golden_{stem}", os.path.join(GOLDEN, f"make_golden_{stem}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def fixture(stem):
    """tests/golden/<stem>.npz as a dict of arrays."""
    return dict(np.load(os.path.join(GOLDEN, f"{stem}.npz"), allow_pickle=False))


def readonly(x):
    """x as a C-contiguous array that refuses writes: what the tests share between them."""
    x = np.ascontiguousarray(x)
    x.setflags(write=False)
    return x


def assert_sampled(key, g, in_crc, out_crc, samples, x, got):
    """got [..., C] equals the expected output of fixture entry `key`: the input x is the fixture's (CRC-32), the sampled pixels are the
    fixture's (they say where a mismatch lies) and the whole output has the fixture's CRC-32.  g: the entry's generator (crc,
    sample_pixels)."""
    assert g.crc(x) == in_crc, f"{key}: the regenerated input is not the fixture's"
    got = np.ascontiguousarray(got)
    px = got.reshape(-1, got.shape[-1])
    idx = g.sample_pixels(len(px))
    assert px[idx].shape == samples.shape, f"{key}: output shape {got.shape}"
    bad = np.nonzero((px[idx] != samples).any(axis=1))[0]
    assert bad.size == 0, f"{key}: {bad.size} of {len(idx)} sampled pixels differ, first at flat pixel {idx[bad[0]]}: {px[idx[bad[0]]]} != {samples[bad[0]]}"
    assert g.crc(got) == out_crc, f"{key}: the sampled pixels match but the whole output's CRC-32 differs from the fixture's"


def pack_table_numpy(filt, n_in, n_out):
    """Build the packed F32 table format on the CPU from the oracle (tests only)."""
    import oracle

    k, xmin, xsize, w = oracle.weights(filt, n_in, n_out, False, np.float32)
    woff = (64 + 8 * n_out + 15) & ~15
    buf = np.zeros(woff + 4 * n_out * k, np.uint8)
    hdr = np.zeros(16, np.int32)
    hdr[:9] = [0x42544141, oracle.FILTERS[filt], 1, n_in, n_out, k, 0, int(max(1, xsize.max())), 0]
    buf[:64] = hdr.view(np.uint8)
    buf[64:64 + 4 * n_out] = xmin.astype(np.int32).view(np.uint8)
    buf[64 + 4 * n_out:64 + 8 * n_out] = xsize.astype(np.int32).view(np.uint8)
    buf[woff:] = w.astype(np.float32).reshape(-1).view(np.uint8)
    return buf, k, int(max(1, xsize.max()))
