"""resize_embed_to_tokens on the GPU: the forward against the CPU restatement and against the existing single-shape calls composed as
the definition says, the backward against the ordered loop of the existing gather-form backwards, all bit for bit; views read where
they lie; pad rows; autograd; the adjoint identity; and a launch count that does not depend on N."""
import numpy as np
import pytest
import torch

import kit_gpu
import resize_embed_ref as ref
from kit_gpu import assert_bits

pytestmark = pytest.mark.gpu

aa = kit_gpu.aa_fixture()

FILTERS = ("linear", "cubic", "box", "hamming", "lanczos")
MODE = {"linear": "bilinear", "cubic": "bicubic", "box": "box", "hamming": "hamming", "lanczos": "lanczos"}
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
CASES = [("base", ref.BASE_SOURCE, ref.BASE_GRIDS)] + [(k,) + v for k, v in ref.FURTHER.items()]
CASE_IDS = [c[0] for c in CASES]


def backward_of(aa, filt):
    return {"linear": aa.linear_backward, "cubic": aa.cubic_backward, "box": aa.nearest_backward, "hamming": aa.hamming_backward,
            "lanczos": aa.lanczos_backward}[filt]


def embed_gpu(h0, w0, d, dtype=torch.float32, seed=0):
    return torch.from_numpy(np.array(ref.embed_values(h0, w0, d, seed))).cuda().to(dtype)


def grad_gpu(grids, d, dtype=torch.float32, seed=0):
    return torch.from_numpy(np.array(ref.grad_values(grids, d, seed))).cuda().to(dtype)


def composed_forward(filt, embed, grids):
    """The definition with the existing calls, in fp32: the cat of the items' token rows."""
    d = embed.shape[2]
    img = embed.float().permute(2, 0, 1)[None]
    items = [kit_gpu.FORWARD[filt](img, [gh, gw])[0].permute(1, 2, 0).reshape(gh * gw, d) for gh, gw in grids]
    return torch.cat(items) if items else torch.zeros((0, d), device=embed.device)


def looped_backward(aa, filt, grad, embed_size, grids):
    """The definition with the existing gather-form backward, in fp32: acc = b_0, acc = acc + b_i."""
    h0, w0, d = embed_size
    off = ref.offsets(grids)
    acc = None
    for i, (gh, gw) in enumerate(grids):
        g = grad[off[i]:off[i + 1]].float().reshape(gh, gw, d).permute(2, 0, 1)[None].contiguous()
        b = backward_of(aa, filt)(g, [gh, gw], [1, d, h0, w0])
        assert b.dtype == torch.float32
        acc = b if acc is None else acc + b
    return acc[0].permute(1, 2, 0).contiguous()


# ---- forward --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", ref.D_VALUES)
@pytest.mark.parametrize("filt", ("linear", "cubic", "box"))
def test_forward_equals_the_restatement(aa, filt, d):
    e = ref.embed_values(*ref.BASE_SOURCE, d)
    with kit_gpu.gpu_error_ends_the_session("resize_embed_to_tokens"):
        got = aa.resize_embed_to_tokens(torch.from_numpy(np.array(e)).cuda(), ref.BASE_GRIDS, MODE[filt])
    assert got.is_contiguous()
    assert_bits(got, torch.from_numpy(ref.packed_forward(filt, e, ref.BASE_GRIDS)), f"{filt} D={d}")


@pytest.mark.parametrize("filt", FILTERS)
def test_forward_equals_the_existing_calls_for_every_dtype(aa, filt):
    for d in (5, 8):
        for in_dtype in DTYPES:
            e = embed_gpu(*ref.BASE_SOURCE, d, in_dtype)
            want = composed_forward(filt, e, ref.BASE_GRIDS)
            for out_dtype in (None,) + DTYPES:
                with kit_gpu.gpu_error_ends_the_session("resize_embed_to_tokens"):
                    got = aa.resize_embed_to_tokens(e, ref.BASE_GRIDS, MODE[filt], out_dtype=out_dtype)
                assert_bits(got, want.to(out_dtype or in_dtype), f"{filt} D={d} {in_dtype} -> {out_dtype}")


@pytest.mark.parametrize("case", CASES[1:], ids=CASE_IDS[1:])
def test_further_cases_both_ways(aa, case):
    name, (h0, w0), grids = case
    d = 8
    e = embed_gpu(h0, w0, d)
    g = grad_gpu(grids, d)
    with kit_gpu.gpu_error_ends_the_session("resize_embed_to_tokens"):
        tok = aa.resize_embed_to_tokens(e, grids, "bicubic")
        ge = aa.resize_embed_to_tokens_backward(g, (h0, w0, d), grids, "bicubic")
    assert_bits(tok, composed_forward("cubic", e, grids), f"{name} forward")
    assert_bits(ge, looped_backward(aa, "cubic", g, (h0, w0, d), grids), f"{name} backward")
    assert_bits(tok, torch.from_numpy(ref.packed_forward("cubic", np.array(ref.embed_values(h0, w0, d)), grids)), f"{name} restated")


def test_empty_list(aa):
    e = embed_gpu(5, 7, 8)
    tok = aa.resize_embed_to_tokens(e, [], out_dtype=torch.bfloat16)
    assert tuple(tok.shape) == (0, 8) and tok.dtype == torch.bfloat16 and tok.is_cuda
    assert tuple(aa.resize_embed_to_tokens(e, [], pad_to=9).shape) == (0, 9, 8)
    ge = aa.resize_embed_to_tokens_backward(torch.zeros((0, 8), device="cuda"), (5, 7, 8), [], dtype=torch.float16)
    assert tuple(ge.shape) == (5, 7, 8) and ge.dtype == torch.float16 and not kit_gpu.bits(ge).any()


@pytest.mark.parametrize("filt", FILTERS)
def test_the_identity_item_is_the_embedding(aa, filt):
    for in_dtype in DTYPES:
        e = embed_gpu(5, 7, 8, in_dtype)
        for out_dtype in DTYPES:
            got = aa.resize_embed_to_tokens(e, [(2, 2), (5, 7)], MODE[filt], out_dtype=out_dtype)
            assert_bits(got[4:], e.reshape(35, 8).to(out_dtype), f"{filt} {in_dtype} -> {out_dtype}")


@pytest.mark.parametrize("d", (5, 8))
def test_views_are_read_where_they_lie(aa, d):
    """A view gives the bits of its contiguous copy, from the same launches: a copy made on the way would be one more."""
    h0, w0 = ref.BASE_SOURCE
    # a class token in front: pos_embed [1, 1 + H0 * W0, D]
    pos = torch.from_numpy(np.array(ref.embed_values(1, 1 + h0 * w0, d, 3))).cuda()
    view = pos[0, 1:].view(h0, w0, d)
    assert view.data_ptr() == pos.data_ptr() + 4 * d
    got = aa.resize_embed_to_tokens(view, ref.BASE_GRIDS)
    # rows and pixels with a pitch: a crop of a larger [H0 + 2, W0 + 3, D + 3] buffer (an odd pixel stride: the per-element path)
    big = torch.from_numpy(np.array(ref.embed_values(h0 + 2, w0 + 3, d + 3, 4))).cuda()
    crop = big[1:1 + h0, 2:2 + w0, 1:1 + d]
    assert crop.stride() == ((w0 + 3) * (d + 3), d + 3, 1) and not crop.is_contiguous()
    got2 = aa.resize_embed_to_tokens(crop, ref.BASE_GRIDS)
    # ... and a pitch that keeps every address a multiple of four elements (D = 8: the vector path through a view)
    wide = torch.from_numpy(np.array(ref.embed_values(h0 + 1, w0 + 1, d + 4, 5))).cuda()
    crop4 = wide[1:, 1:, 4:] if d % 4 == 0 else wide[1:, 1:, 3:3 + d]
    got3 = aa.resize_embed_to_tokens(crop4, ref.BASE_GRIDS)
    dense = len(kit_gpu.count_launches(lambda: aa.resize_embed_to_tokens(crop.contiguous(), ref.BASE_GRIDS))) - 1  # (minus the copy)
    for v in (view, crop, crop4):
        assert len(kit_gpu.count_launches(lambda: aa.resize_embed_to_tokens(v, ref.BASE_GRIDS))) == dense
    assert_bits(got, aa.resize_embed_to_tokens(view.clone(), ref.BASE_GRIDS), "class-token view")
    assert_bits(got2, aa.resize_embed_to_tokens(crop.contiguous(), ref.BASE_GRIDS), "pitched view")
    assert_bits(got3, aa.resize_embed_to_tokens(crop4.contiguous(), ref.BASE_GRIDS), "pitched view, aligned")


@pytest.mark.parametrize("out_dtype", DTYPES)
def test_pad_rows_are_plus_zero(aa, out_dtype):
    grids = ref.BASE_GRIDS
    L = 50
    e = embed_gpu(*ref.BASE_SOURCE, 8)
    packed = aa.resize_embed_to_tokens(e, grids, out_dtype=out_dtype)
    padded = aa.resize_embed_to_tokens(e, grids, pad_to=L, out_dtype=out_dtype)
    assert tuple(padded.shape) == (len(grids), L, 8)
    off = ref.offsets(grids)
    for i in range(len(grids)):
        t = off[i + 1] - off[i]
        assert_bits(padded[i, :t], packed[off[i]:off[i + 1]], f"item {i}")
        assert not kit_gpu.bits(padded[i, t:]).any(), f"item {i}: a pad row is not all-zero bits"
    with pytest.raises(ValueError, match="pad_to"):
        aa.resize_embed_to_tokens(e, grids, pad_to=48)


# ---- backward -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", FILTERS)
def test_backward_equals_the_ordered_loop(aa, filt):
    h0, w0 = ref.BASE_SOURCE
    grids = ref.BASE_GRIDS
    for d in (5, 8):
        for gdtype in DTYPES:
            g = grad_gpu(grids, d, gdtype)
            want = looped_backward(aa, filt, g, (h0, w0, d), grids)
            for dtype in DTYPES:
                with kit_gpu.gpu_error_ends_the_session("resize_embed_to_tokens_backward"):
                    got = aa.resize_embed_to_tokens_backward(g, (h0, w0, d), grids, MODE[filt], dtype=dtype)
                assert got.is_contiguous()
                assert_bits(got, want.to(dtype), f"{filt} D={d} {gdtype} -> {dtype}")


@pytest.mark.parametrize("d", (520, 523))
def test_backward_wide_rows_and_padded_gradients(aa, d):
    h0, w0 = ref.BASE_SOURCE
    grids = ref.BASE_GRIDS
    g = grad_gpu(grids, d, torch.bfloat16)
    want = looped_backward(aa, "cubic", g, (h0, w0, d), grids)
    got = aa.resize_embed_to_tokens_backward(g, (h0, w0, d), grids, dtype=torch.float32)
    assert_bits(got, want, f"D={d}")
    assert_bits(aa.resize_embed_to_tokens_backward(g, (h0, w0, d), grids, dtype=torch.float32), got, "a second call")
    # pad rows are not read: NaNs there change nothing
    padded = torch.from_numpy(ref.pad_rows(g.float().cpu().numpy(), grids, 50, np.nan)).cuda().to(torch.bfloat16)
    assert_bits(aa.resize_embed_to_tokens_backward(padded, (h0, w0, d), grids, pad_to=50, dtype=torch.float32), got, "padded gradients")


@pytest.mark.parametrize("dtype", DTYPES)
def test_autograd_is_the_explicit_backward(aa, dtype):
    h0, w0 = ref.BASE_SOURCE
    grids = ref.BASE_GRIDS
    e = embed_gpu(h0, w0, 8, dtype).requires_grad_(True)
    tok = aa.resize_embed_to_tokens(e, grids, out_dtype=torch.bfloat16)
    assert tok.requires_grad and tok.dtype == torch.bfloat16
    assert_bits(tok.detach(), aa.resize_embed_to_tokens(e.detach(), grids, out_dtype=torch.bfloat16), "forward under autograd")
    g = grad_gpu(grids, 8, torch.bfloat16)
    tok.backward(g)
    assert e.grad.dtype == dtype and tuple(e.grad.shape) == (h0, w0, 8)
    assert_bits(e.grad, aa.resize_embed_to_tokens_backward(g, (h0, w0, 8), grids, dtype=dtype), "autograd")
    with torch.no_grad():
        assert not aa.resize_embed_to_tokens(e, grids).requires_grad
    # through the class-token view of a parameter, with pad_to
    pos = embed_gpu(1, 1 + h0 * w0, 8, seed=3).requires_grad_(True)
    tok = aa.resize_embed_to_tokens(pos[0, 1:].view(h0, w0, 8), grids, pad_to=50)
    gp = torch.from_numpy(ref.pad_rows(np.array(ref.grad_values(grids, 8)), grids, 50)).cuda()
    tok.backward(gp)
    assert not kit_gpu.bits(pos.grad[0, 0]).any()
    assert_bits(pos.grad[0, 1:].view(h0, w0, 8), aa.resize_embed_to_tokens_backward(gp, (h0, w0, 8), grids, pad_to=50), "autograd through a view")


@pytest.mark.parametrize("filt", FILTERS)
def test_adjoint_identity_and_dense_bounds(aa, filt):
    """<forward(e), g> = <e, backward(g)> in float64, within what the two dense bounds allow: sum |g| . bound_fwd + sum |e| . bound_bwd;
    and each side within its own dense bound."""
    h0, w0 = ref.BASE_SOURCE
    grids, d = ref.BASE_GRIDS, 6
    e, g = ref.embed_values(h0, w0, d), ref.grad_values(grids, d)
    tok = aa.resize_embed_to_tokens(torch.from_numpy(np.array(e)).cuda(), grids, MODE[filt]).cpu().numpy().astype(np.float64)
    ge = aa.resize_embed_to_tokens_backward(torch.from_numpy(np.array(g)).cuda(), (h0, w0, d), grids, MODE[filt]).cpu().numpy().astype(np.float64)
    fwd, fb = ref.dense_forward(filt, e, grids)
    bwd, bb = ref.dense_backward(filt, g, (h0, w0, d), grids)
    rf, rb = ref.worst_ratio(tok, fwd, fb), ref.worst_ratio(ge, bwd, bb)
    lhs, rhs = float((tok * g).sum()), float((e.astype(np.float64) * ge).sum())
    allowed = float((np.abs(g) * fb).sum() + (np.abs(e) * bb).sum())
    print(f"{filt}: forward err / bound {rf:.3f}, backward {rb:.3f}, adjoint |{lhs:.9g} - {rhs:.9g}| / {allowed:.3g} = {abs(lhs - rhs) / allowed:.3f}")
    assert rf <= 1.0 and rb <= 1.0
    assert abs(lhs - rhs) <= allowed


# ---- launches -------------------------------------------------------------------------------------------------------------------------
def test_launch_count_does_not_depend_on_n(aa):
    h0, w0 = ref.BASE_SOURCE
    e = embed_gpu(h0, w0, 8)
    counts = {}
    for grids in (ref.BASE_GRIDS[:2], ref.BASE_GRIDS + [(4, 4)]):
        g = grad_gpu(grids, 8)
        aa.resize_embed_to_tokens(e, grids), aa.resize_embed_to_tokens_backward(g, (h0, w0, 8), grids)  # (code objects loaded)
        fwd = kit_gpu.count_launches(lambda: aa.resize_embed_to_tokens(e, grids))
        bwd = kit_gpu.count_launches(lambda: aa.resize_embed_to_tokens_backward(g, (h0, w0, 8), grids))
        counts[len(grids)] = (len(fwd), len(bwd))
        assert 1 <= len(fwd) <= 3 and 1 <= len(bwd) <= 3, (fwd, bwd)
    assert counts[2] == counts[9], counts
