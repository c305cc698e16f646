"""The ragged calls at the edges of their tile sizes, on the GPU: output rows longer than one work unit of the vertical passes, strips of
the horizontal pass staged in two and three chunks, single windows longer than a chunk, and placed canvases several work units wide.
Every expected byte is Pillow's (tests/golden/resize_many_edges.npz, tolerance 0) or torch's CPU conversion of the CPU restatement's bytes,
which tests/test_resize_many_edges_cpu.py pins to the same fixture; nothing expected comes from the package.  That every case really
crosses the boundary it is named for is asserted there too, without a GPU.  A wrong byte is reported with the work unit that wrote it."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import guard_ref  # noqa: E402
import kit_gpu  # noqa: E402
import resize_many_edges_ref as ref  # noqa: E402
from kit_golden import MEAN, MODE, STD  # noqa: E402
from kit_gpu import FORWARD  # noqa: E402

from interpolate_antialiasing_amd import extension_interpolate as aa  # noqa: E402

pytestmark = pytest.mark.gpu

G = ref.gen()
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
FORMATS = ["nchw", "nhwc"]
ALL = [cs.name for cs in G.CASES]


@functools.lru_cache(maxsize=None)
def _inputs(name, cls):
    """The case's images on the GPU (shared between tests, never written)."""
    return [kit_gpu.to_gpu(ref.item(name, i), cls) for i in range(len(G.case(name).items))]


def _check(name, f, cls, y):
    """y, the call's uint8 result, is Pillow's: against the restatement first (a mismatch names its work units), then the fixture."""
    cs = G.case(name)
    assert tuple(y.shape) == (len(cs.items), cs.c) + tuple(cs.out) and y.dtype == torch.uint8
    kit_gpu.assert_class_format(y, cls, cs.c)
    got = y.cpu()
    wrong = ref.where(name, f, cls, got.numpy(), ref.restated_batch(name, f))
    assert wrong is None, wrong
    for i in range(len(cs.items)):
        ref.assert_matches_fixture(f"{name}/{f}/{i}", ref.item(name, i), got[i].permute(1, 2, 0).numpy())


# ---- resize_many -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cls", ref.classes(ALL))
def test_every_case_filter_and_layout_class_equals_pillow(name, cls):
    cs = G.case(name)
    for f in cs.filters:
        _check(name, f, cls, aa.resize_many(_inputs(name, cls), list(cs.out), MODE[f], **ref.kw(name)))


@pytest.mark.parametrize("name,cls", ref.classes(G.CHUNKED + G.CHUNKED_PLACED))
def test_chunked_rows_of_crops_at_odd_offsets_and_pitches(name, cls):
    """Every chunk of a row starts at another alignment, and no two items share one."""
    cs = G.case(name)
    crops = [kit_gpu.pitched_crop(ref.item(name, i), cls, i) for i in range(len(cs.items))]
    for f in cs.filters:
        y = aa.resize_many(crops, list(cs.out), MODE[f], **ref.kw(name))
        dense = aa.resize_many(_inputs(name, cls), list(cs.out), MODE[f], **ref.kw(name))
        assert y.stride() == dense.stride() and torch.equal(y, dense), (name, f, cls)
        _check(name, f, cls, y)


@pytest.mark.parametrize("name,cls", ref.classes(G.WIDE + G.CHUNKED))
def test_each_item_equals_the_single_image_call(name, cls):
    cs = G.case(name)
    imgs, boxes = _inputs(name, cls), ref.kw(name)["boxes"]
    for f in cs.filters:
        y = aa.resize_many(imgs, list(cs.out), MODE[f], boxes=boxes)
        for i in range(len(cs.items)):
            one = FORWARD[f](imgs[i][None], list(cs.out), box=boxes[i])
            assert torch.equal(y[i], one[0]), (name, f, cls, i)


# ---- resize_many_to_float ----------------------------------------------------------------------------------------------------------------
def _piece(name, cls, flips):
    """For kit_gpu.assert_bits: the column of the unflipped row a wrong element was computed as, and its piece of the converting pass."""
    cs = G.case(name)

    def explain(at):
        n, _, _, x = at
        src = cs.out[1] - 1 - x if flips is not None and flips[n] else x
        return f"computed as column {src} = piece {src // ref.constants()['VPIXELS'][ref.elem_bytes(cs.c, cls)]} of the converting pass"

    return explain


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("name,cls", ref.classes(G.WIDE + G.WIDE_PLACED))
def test_to_float_is_the_restated_bytes_converted(name, cls, dtype):
    cs = G.case(name)
    n, c = len(cs.items), cs.c
    for f in cs.filters:
        b = torch.from_numpy(ref.restated_batch(name, f))
        for flips in (None, [i % 2 == 0 for i in range(n)]):
            want = kit_gpu.convert(b, dtype, flips=flips)
            for fmt in FORMATS:
                y = aa.resize_many_to_float(_inputs(name, cls), list(cs.out), MODE[f], flips=flips, out_dtype=dtype, out_format=fmt, mean=MEAN[:c],
                                            std=STD[:c], **ref.kw(name))
                if c > 1:
                    assert y.is_contiguous(memory_format=torch.channels_last) == (fmt == "nhwc") and y.is_contiguous() == (fmt == "nchw")
                kit_gpu.assert_bits(y, want, f"{name}/{f}/{cls}/{fmt}/{y.dtype}/flips {flips}", _piece(name, cls, flips))


# ---- guard bands -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("name,cls", ref.classes(["w_c3_1025", "w_c3_683", "pw_c3_700", "pw_c3_1100"]))
def test_guard_bands_uint8(monkeypatch, name, cls, lead):
    """The descriptor's device copy, the arena of tables and intermediates and the output: nothing outside them is written, and every
    byte of the output is (a run into 0xFF-filled and a run into 0x00-filled memory agree), at both placements of the output."""
    cs = G.case(name)
    imgs = _inputs(name, cls)
    for f in cs.filters:
        runs = []
        for fill in (0xFF, 0x00):
            with guard_ref.guarded(monkeypatch, lead, fill) as rec:
                y = aa.resize_many(imgs, list(cs.out), MODE[f], **ref.kw(name))
                rec.check()
                assert len(rec.records) == 3 and len(rec.outputs()) == 1  # desc_dev, ws, out
                assert rec.record_of(y) is not None and y.data_ptr() % 2 == lead
                runs.append(y.cpu())
        assert guard_ref.unwritten_u8(runs[0], runs[1]) == 0, (name, f, cls, lead)
        _check(name, f, cls, runs[0])


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("name,cls", ref.classes(["w_c3_1025", "pw_c3_700"]))
def test_guard_bands_bf16(monkeypatch, name, cls, lead):
    cs = G.case(name)
    n, c = len(cs.items), cs.c
    flips = [i % 2 == 1 for i in range(n)]
    f = cs.filters[0]
    want = kit_gpu.convert(torch.from_numpy(ref.restated_batch(name, f)), torch.bfloat16, flips=flips)
    for fmt in FORMATS:
        with guard_ref.guarded(monkeypatch, lead) as rec:
            y = aa.resize_many_to_float(_inputs(name, cls), list(cs.out), MODE[f], flips=flips, out_dtype=torch.bfloat16, out_format=fmt, mean=MEAN[:c],
                                        std=STD[:c], **ref.kw(name))
            rec.check()
            assert len(rec.records) == 3 and rec.record_of(y) is not None and y.data_ptr() % 4 == 2 * lead
            assert guard_ref.unwritten_float(y) == 0, (name, cls, fmt, lead)
        kit_gpu.assert_bits(y, want, f"{name}/{f}/{cls}/{fmt}/{y.dtype}/flips {flips}", _piece(name, cls, flips))
