"""The float ragged calls at the seams of their kernels, on the GPU: output rows of several column tiles with real windows in each,
flipped and mirrored across them; windows of hundreds of taps on either axis; tables of more rows, and adjoints of more source
positions, than the table kernel has lanes.  The cases are float_many_edges_ref's, and test_float_many_edges_cpu.py asserts without a
GPU that each still reaches what it is named for.  Everything is equality of bits — against the CPU restatements (the oracle's three
filters) and against the existing single-shape calls composed as the definitions say (all five) — but for one check: resize_many_back's
values against the dense float64 form with resize_many_back_ref's bound, which the oracle itself meets on these inputs (asserted in
the CPU file)."""
import functools

import numpy as np
import pytest
import torch

import float_many_edges_ref as ref
import kit_gpu
import resize_embed_ref as embed_ref
import resize_many_back_bwd_ref as bwd_ref
import resize_many_back_merged_ref as merged_ref
import resize_many_back_ref as back_ref
from kit_golden import MODE
from kit_gpu import assert_bits
from test_resize_embed_gpu import composed_forward, looped_backward
from test_resize_many_back_bwd_gpu import gpu_grads, looped
from test_resize_many_back_gpu import composed, region_views

pytestmark = pytest.mark.gpu

aa = kit_gpu.aa_fixture()

DTYPES = (torch.float32, torch.float16, torch.bfloat16)
CLASSES = ("planar", "channels_last")
MERGES = ("sum", "mean")


def item_gpu(a, dtype=torch.float32, cls="planar"):
    """[K, H, W] numpy -> the GPU item in dtype, as planes or with interleaved classes (a copy: the shared inputs are read-only)."""
    t = torch.from_numpy(np.array(a)).cuda().to(dtype)
    return t.permute(1, 2, 0).contiguous().permute(2, 0, 1) if cls == "channels_last" else t


def back(aa, *args, **kw):
    with kit_gpu.gpu_error_ends_the_session("resize_many_back"):
        return aa.resize_many_back(*args, **kw)


def merged(aa, *args, **kw):
    with kit_gpu.gpu_error_ends_the_session("resize_many_back_merged"):
        return aa.resize_many_back_merged(*args, **kw)


def embed(aa, *args, **kw):
    with kit_gpu.gpu_error_ends_the_session("resize_embed_to_tokens"):
        return aa.resize_embed_to_tokens(*args, **kw)


def embed_bwd(aa, *args, **kw):
    with kit_gpu.gpu_error_ends_the_session("resize_embed_to_tokens_backward"):
        return aa.resize_embed_to_tokens_backward(*args, **kw)


def back_bwd(aa, *args, **kw):
    with kit_gpu.gpu_error_ends_the_session("resize_many_back_backward"):
        return aa.resize_many_back_backward(*args, **kw)


def rounded(a, dtype):
    """A float32 array as the values its copy in dtype holds."""
    return a if dtype == torch.float32 else torch.from_numpy(np.array(a)).to(dtype).float().numpy()


@functools.lru_cache(maxsize=None)
def restated(filt, names, k, flips, dtype=torch.float32):
    """The oracle's fp32 values of the named cases as one list, on inputs rounded to dtype: computed once and shared."""
    srcs, regions, sizes = ref.back_list(names, k)
    return back_ref.values(filt, [rounded(s, dtype) for s in srcs], regions, sizes, flips)


@functools.lru_cache(maxsize=None)
def dense(filt, names, k, flips):
    srcs, regions, sizes = ref.back_list(names, k)
    return back_ref.dense_values(filt, srcs, regions, sizes, flips)


def check_back(aa, filt, names, k, flips, cls, what):
    """One float32 call over the named cases: bits against the composed existing calls; for the oracle's filters bits against the
    restatement and err / bound <= 1 against the dense float64 form.  -> the call's outputs"""
    srcs, regions, sizes = ref.back_list(names, k)
    items = [item_gpu(s, cls=cls) for s in srcs]
    outs = back(aa, items, sizes, MODE[filt], regions=regions, flips=flips)
    want = composed(filt, region_views(items, regions), sizes, flips)
    tag = f"{what} {filt} {cls} flips {flips}"
    for i, n in enumerate(names):
        explain = ref.where_back(n, flips is not None and flips[i])
        assert_bits(outs[i], want[i], f"{tag} {n} against the composed calls", explain)
        if filt in ref.ORACLE_FILTERS:
            key = None if flips is None else tuple(flips)
            assert_bits(outs[i], torch.from_numpy(restated(filt, names, k, key)[i]), f"{tag} {n} against the restatement", explain)
    if filt in ref.ORACLE_FILTERS:
        d_want, d_bnd = dense(filt, names, k, None if flips is None else tuple(flips))
        ratio = back_ref.worst_ratio([o.cpu().numpy().astype(np.float64) for o in outs], d_want, d_bnd)
        print(f"{tag}: worst err / bound against float64 {ratio:.3f}")
        assert ratio <= 1.0, tag
    return outs


# ---- resize_many_back ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("name", ref.BACK_NAMES)
def test_back_each_case_alone(aa, name, cls):
    for filt in ref.FILTERS:
        for flips in (None, [True]):
            outs = check_back(aa, filt, (name,), None, flips, cls, "alone")
            k, _, _, size = ref.BACK_CASES[name]
            assert tuple(outs[0].shape) == (k,) + size and outs[0].is_contiguous()


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("k", ref.TOGETHER_K)
def test_back_all_cases_in_one_list(aa, k, cls):
    """The item search and the unit prefix cross the wide, the long and the tall items; K = 4 takes the vector loads when interleaved."""
    for filt in ref.FILTERS:
        outs = check_back(aa, filt, ref.BACK_NAMES, k, ref.TOGETHER_FLIPS, cls, f"together K={k}")
        # ... and an item's bits do not depend on its neighbours
        i = ref.BACK_NAMES.index("wide_out")
        srcs, regions, sizes = ref.back_list(("wide_out",), k)
        alone = back(aa, [item_gpu(srcs[0], cls=cls)], sizes, MODE[filt], flips=[ref.TOGETHER_FLIPS[i]])
        assert_bits(outs[i], alone[0], f"together K={k} {filt} {cls}: wide_out alone", ref.where_back("wide_out", ref.TOGETHER_FLIPS[i]))


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("dtype", DTYPES[1:], ids=("fp16", "bf16"))
def test_back_16_bit_inputs(aa, dtype, cls):
    for name in ref.BACK_16BIT:
        srcs, regions, sizes = ref.back_list((name,))
        items = [item_gpu(srcs[0], dtype, cls)]
        for filt in ref.FILTERS:
            for flips in (None, [True]):
                want = composed(filt, region_views(items, regions), sizes, flips)[0]
                tag = f"{name} {filt} {dtype} {cls} flips {flips}"
                explain = ref.where_back(name, flips is not None)
                assert_bits(back(aa, items, sizes, MODE[filt], regions=regions, flips=flips)[0], want.to(dtype), tag, explain)
                got32 = back(aa, items, sizes, MODE[filt], regions=regions, flips=flips, out_dtype=torch.float32)[0]
                assert_bits(got32, want, f"{tag} -> float32", explain)
                if filt in ref.ORACLE_FILTERS:
                    w = restated(filt, (name,), None, None if flips is None else (True,), dtype)[0]
                    assert_bits(got32, torch.from_numpy(w), f"{tag} against the restatement", explain)


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("name", ref.BACK_REDUCED)
def test_back_argmax_and_greater(aa, name, cls):
    srcs, regions, sizes = ref.back_list((name,))
    items = [item_gpu(srcs[0], cls=cls)]
    for filt in ref.FILTERS:
        for flips in (None, [True]):
            if filt in ref.ORACLE_FILTERS:
                vals = restated(filt, (name,), None, None if flips is None else (True,))[0]
            else:
                vals = composed(filt, region_views(items, regions), sizes, flips)[0].cpu().numpy()
            tag = f"{name} {filt} {cls} flips {flips}"
            lab = back(aa, items, sizes, MODE[filt], regions=regions, flips=flips, reduce="argmax", out_dtype=torch.uint8)[0]
            assert_bits(lab, torch.from_numpy(np.argmax(vals, axis=0).astype(np.uint8)), f"{tag} argmax", ref.where_back(name, flips is not None))
            m = back(aa, items, sizes, MODE[filt], regions=regions, flips=flips, reduce="greater", threshold=ref.THRESHOLD)[0]
            assert m.dtype == torch.bool
            assert_bits(m.to(torch.uint8), torch.from_numpy(back_ref.masks([vals], ref.THRESHOLD)[0].astype(np.uint8)), f"{tag} greater",
                        ref.where_back(name, flips is not None))


def misaligned_interleaved(t):
    """[K, h, w] -> the same values as interleaved classes in a larger NaN-filled buffer: the storage begins one element in, and a row
    pitch that is no multiple of 4 elements, so no row but by chance lies where a vector of four classes could be loaded."""
    k, h, w = t.shape
    pitch = w * k + 5 + (1 if (w * k + 5) % 4 == 0 else 0)
    buf = torch.full((1 + h * pitch + 8,), float("nan"), dtype=t.dtype, device="cuda")
    v = buf.as_strided((k, h, w), (1, pitch, k), 1)
    v.copy_(t)
    assert pitch % 4 != 0 and (v.data_ptr() // t.element_size()) % 4 != 0 and v.stride() == (1, pitch, k)
    return v


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "fp16", "bf16"))
def test_back_misaligned_interleaved_storage(aa, dtype):
    """K = 8 would take the vector loads; an item whose addresses do not allow them turns them off for the whole list, and both it and
    an aligned item beside it give the bits of their contiguous copies."""
    rng = np.random.default_rng(8)
    a = torch.from_numpy(rng.standard_normal((8, 5, 11)).astype(np.float32)).cuda().to(dtype)
    b = torch.from_numpy(rng.standard_normal((8, 6, 6)).astype(np.float32)).cuda().to(dtype)
    sizes = [(9, 17), (3, 4)]
    va, vb = misaligned_interleaved(a), item_gpu(b.cpu().float().numpy(), dtype, "channels_last")
    assert vb.stride() == (1, 48, 8) and vb.data_ptr() % 16 == 0
    for filt in ("linear", "cubic", "lanczos"):
        kw = dict(flips=[True, False], out_dtype=torch.float32)
        want = back(aa, [a, b], sizes, MODE[filt], **kw)  # (the contiguous copies: planes)
        assert_bits(back(aa, [va], sizes[:1], MODE[filt], flips=[True], out_dtype=torch.float32)[0], want[0], f"{filt} {dtype} misaligned, alone")
        assert_bits(back(aa, [vb], sizes[1:], MODE[filt], flips=[False], out_dtype=torch.float32)[0], want[1], f"{filt} {dtype} aligned, alone")
        both = back(aa, [va, vb], sizes, MODE[filt], **kw)
        assert_bits(both[0], want[0], f"{filt} {dtype} misaligned, in a list")
        assert_bits(both[1], want[1], f"{filt} {dtype} aligned, beside a misaligned item")
        assert_bits(want[0], composed(filt, [a], sizes[:1], [True])[0], f"{filt} {dtype} the contiguous copy against the composed calls")
    # the view is read where it lies: two launches, no copy
    names = kit_gpu.count_launches(lambda: aa.resize_many_back([va, vb], sizes))
    assert len(names) == 2, names


# ---- resize_many_back_merged -----------------------------------------------------------------------------------------------------------
def composed_merged(filt, items, merge):
    """The definition with the existing calls, as test_resize_many_back_merged_gpu.composed states it for its own case: per member
    FORWARD[filt] at its group's size, flip(-1), torch adds in ascending item order, the mean's division by numpy on the CPU."""
    rs = []
    for i, (t, g) in enumerate(zip(items, ref.MERGED_GROUPS)):
        r = kit_gpu.FORWARD[filt](t.float()[None].contiguous(), list(ref.MERGED_SIZES[g]))[0]
        rs.append(r.flip(-1) if ref.MERGED_FLIPS[i] else r)
    outs = []
    for g in range(len(ref.MERGED_SIZES)):
        idx = merged_ref.members(ref.MERGED_GROUPS, g)
        s = rs[idx[0]]
        for i in idx[1:]:
            s = s + rs[i]
        if merge == "mean":
            s = torch.from_numpy(s.cpu().numpy() / np.float32(len(idx)))
        outs.append(s)
    return outs


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("k", ref.MERGED_K)
def test_merged_mirrored_reads_across_tiles_and_long_windows(aa, k, cls):
    items = [item_gpu(s, cls=cls) for s in ref.merged_sources(k)]
    explain = [ref.where_back(ow) for _, ow in ref.MERGED_SIZES]
    for filt in ref.FILTERS:
        for merge in MERGES:
            tag = f"merged K={k} {cls} {filt} {merge}"
            outs = merged(aa, items, ref.MERGED_GROUPS, ref.MERGED_SIZES, MODE[filt], flips=ref.MERGED_FLIPS, merge=merge)
            labs = merged(aa, items, ref.MERGED_GROUPS, ref.MERGED_SIZES, MODE[filt], flips=ref.MERGED_FLIPS, merge=merge, reduce="argmax",
                          out_dtype=torch.uint8)
            want = composed_merged(filt, items, merge)
            assert [tuple(o.shape) for o in outs] == [(k,) + s for s in ref.MERGED_SIZES] and [tuple(o.shape) for o in labs] == ref.MERGED_SIZES
            for g in range(len(ref.MERGED_SIZES)):
                assert_bits(outs[g], want[g], f"{tag} group {g} against the composed calls", explain[g])
                vals = ref.merged_values(filt, k, merge)[g] if filt in ref.ORACLE_FILTERS else want[g].cpu().numpy()
                if filt in ref.ORACLE_FILTERS:
                    assert_bits(outs[g], torch.from_numpy(np.array(vals)), f"{tag} group {g} against the restatement", explain[g])
                assert_bits(labs[g], torch.from_numpy(np.argmax(vals, axis=0).astype(np.uint8)), f"{tag} group {g} argmax", explain[g])


# ---- resize_embed_to_tokens ------------------------------------------------------------------------------------------------------------
def embed_gpu(hw, d, seed):
    return torch.from_numpy(np.array(embed_ref.embed_values(hw[0], hw[1], d, seed))).cuda()


def tokens_gpu(grids, d, seed, dtype=torch.float32):
    return torch.from_numpy(np.array(embed_ref.grad_values(grids, d, seed))).cuda().to(dtype)


def where_token(grids):
    off = embed_ref.offsets(grids)

    def explain(at):
        i = int(np.searchsorted(off, at[0], side="right")) - 1
        t = at[0] - off[i]
        return f"item {i} of grid {grids[i]}, token row {t // grids[i][1]}, column {t % grids[i][1]}, channel {at[1]}"

    return explain


@pytest.mark.parametrize("d", ref.EMBED_D)
@pytest.mark.parametrize("name", tuple(ref.EMBED_CASES))
def test_embed_forward(aa, name, d):
    hw, grids = ref.EMBED_CASES[name]
    seed = 10 + tuple(ref.EMBED_CASES).index(name)
    e = embed_gpu(hw, d, seed)
    for filt in ref.FILTERS:
        tok = embed(aa, e, grids, MODE[filt])
        assert tuple(tok.shape) == (embed_ref.offsets(grids)[-1], d) and tok.is_contiguous()
        assert_bits(tok, composed_forward(filt, e, grids), f"{name} D={d} {filt} against the composed calls", where_token(grids))
        if filt in ref.ORACLE_FILTERS:
            want = embed_ref.packed_forward(filt, np.array(embed_ref.embed_values(hw[0], hw[1], d, seed)), grids)
            assert_bits(tok, torch.from_numpy(want), f"{name} D={d} {filt} against the restatement", where_token(grids))
    if hw in grids:  # the identity grid is the embedding's bits
        i = grids.index(hw)
        off = embed_ref.offsets(grids)
        assert_bits(tok[off[i]:off[i + 1]], e.reshape(hw[0] * hw[1], d), f"{name} D={d} identity")


@pytest.mark.parametrize("d", ref.EMBED_D)
@pytest.mark.parametrize("name", tuple(ref.EMBED_CASES))
def test_embed_backward(aa, name, d):
    hw, grids = ref.EMBED_CASES[name]
    seed = 10 + tuple(ref.EMBED_CASES).index(name)
    size = hw + (d,)
    g = tokens_gpu(grids, d, seed)
    for filt in ref.FILTERS:
        got = embed_bwd(aa, g, size, grids, MODE[filt])
        assert tuple(got.shape) == size and got.is_contiguous()
        assert_bits(got, looped_backward(aa, filt, g, size, grids), f"{name} D={d} {filt} backward")
    g16 = tokens_gpu(grids, d, seed, torch.bfloat16)
    assert_bits(embed_bwd(aa, g16, size, grids, "bicubic", dtype=torch.float32), looped_backward(aa, "cubic", g16, size, grids),
                f"{name} D={d} bfloat16 gradients")


@pytest.mark.parametrize("d", ref.EMBED_D)
def test_embed_padded_to_the_largest_item(aa, d):
    hw, grids = ref.EMBED_CASES["shrink_40x48"]
    L = max(gh * gw for gh, gw in grids)
    off = embed_ref.offsets(grids)
    e = embed_gpu(hw, d, 10)
    g = tokens_gpu(grids, d, 10)
    for filt in ("cubic", "lanczos"):
        packed = embed(aa, e, grids, MODE[filt])
        padded = embed(aa, e, grids, MODE[filt], pad_to=L)
        assert tuple(padded.shape) == (len(grids), L, d)
        for i in range(len(grids)):
            t = off[i + 1] - off[i]
            assert_bits(padded[i, :t], packed[off[i]:off[i + 1]], f"D={d} {filt} padded item {i}")
            assert not kit_gpu.bits(padded[i, t:]).any(), f"D={d} {filt} item {i}: a pad row is not all-zero bits"
        # pad rows of the gradient are not read: NaNs there change nothing
        gp = torch.from_numpy(embed_ref.pad_rows(g.cpu().numpy(), grids, L, np.nan)).cuda()
        assert_bits(embed_bwd(aa, gp, hw + (d,), grids, MODE[filt], pad_to=L), embed_bwd(aa, g, hw + (d,), grids, MODE[filt]), f"D={d} {filt} padded gradient")


# ---- resize_many_back_backward ---------------------------------------------------------------------------------------------------------
def check_bwd(aa, filt, case, k, gdtype, out_format, seed, what):
    canvas, regions, sizes = case
    gs = gpu_grads(sizes, k, gdtype, seed=seed)
    for flips in (None, [True]):
        for dtype in dict.fromkeys((gdtype, torch.float32)):
            got = back_bwd(aa, gs, canvas, MODE[filt], regions=regions, flips=flips, dtype=dtype, out_format=out_format)
            assert got.dtype == dtype and tuple(got.shape) == (1, k) + tuple(canvas)
            assert got.is_contiguous(memory_format=torch.channels_last if out_format == "nhwc" else torch.contiguous_format)
            assert_bits(got, torch.stack(looped(aa, filt, gs, canvas, regions, flips, dtype)), f"{what} {filt} {gdtype} -> {dtype} {out_format} flips {flips}")


@pytest.mark.parametrize("out_format", ("nchw", "nhwc"))
@pytest.mark.parametrize("filt", ref.FILTERS)
def test_backward_one_adjoint_row_of_300_taps_along_h(aa, filt, out_format):
    for gdtype in DTYPES:
        check_bwd(aa, filt, ref.tall_adjoint_case(), 5, gdtype, out_format, 301, "tall adjoint")


@pytest.mark.parametrize("out_format", ("nchw", "nhwc"))
@pytest.mark.parametrize("gdtype", DTYPES, ids=("fp32", "fp16", "bf16"))
@pytest.mark.parametrize("filt", ("linear", "box", "lanczos"))
def test_backward_long_rows_and_seams_in_every_dtype_and_format(aa, filt, gdtype, out_format):
    for case, k in ((bwd_ref.long_rows_case(), 2), (bwd_ref.seams_case(), 5)):
        check_bwd(aa, filt, case, k, gdtype, out_format, case[2][0][1], f"canvas {case[0]}")
