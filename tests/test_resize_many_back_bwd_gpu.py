"""resize_many_back_backward and resize_many_back's autograd on the GPU: bit for bit against the loop of the package's own single-shape
backward, as the definition says, and against the CPU restatement of the gather form; the zeros; the launch count; gradients read
where they lie; autograd against the explicit call; and the dense float64 adjoint with its derived bound."""
import numpy as np
import pytest
import torch

import kit_gpu
import resize_many_back_bwd_ref as ref
import resize_many_back_ref as fwd_ref
from kit_golden import MODE
from kit_gpu import assert_bits

pytestmark = pytest.mark.gpu

aa = kit_gpu.aa_fixture()

DTYPES = (torch.float32, torch.float16, torch.bfloat16)
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def gpu_grads(sizes, k, dtype=torch.float32, seed=0):
    """The reference module's gradients on the GPU, rounded to dtype."""
    return [torch.from_numpy(np.array(g)).cuda().to(dtype) for g in ref.grads(sizes, k, seed)]


def call(aa, *args, **kw):
    with kit_gpu.gpu_error_ends_the_session("resize_many_back_backward"):
        return aa.resize_many_back_backward(*args, **kw)


def looped(aa, filt, gs, canvas, regions, flips, dtype, k=None):
    """The definition with the existing single-shape backward, the way a user writes it today: per item <mode>_backward of the (mirrored)
    gradient in fp32, rounded to dtype, copied into a zeroed canvas.  -> [[K, H_i, W_i]]"""
    bwd = {"linear": aa.linear_backward, "cubic": aa.cubic_backward, "box": aa.nearest_backward, "hamming": aa.hamming_backward,
           "lanczos": aa.lanczos_backward}[filt]
    cv = ref.canvases_of(canvas, len(gs))
    k = k if k is not None else next(int(g.shape[0]) for g in gs if g is not None)
    outs = []
    for i, g in enumerate(gs):
        out = torch.zeros((k,) + cv[i], dtype=dtype, device="cuda")
        if g is not None:
            y0, x0, h, w = (0, 0) + cv[i] if regions is None or regions[i] is None else regions[i]
            u = g.flip(-1) if flips is not None and flips[i] else g
            b = bwd(u.float()[None].contiguous(), list(g.shape[1:]), [1, k, h, w])[0]
            out[:, y0:y0 + h, x0:x0 + w] = b.to(dtype)
        outs.append(out)
    return outs


def check_list(outs, canvases, k, dtype, nhwc=False):
    """N tensors [K, H_i, W_i] of dtype, views of one arena, each on a 16-byte boundary of it, each dense in the class."""
    assert isinstance(outs, list) and [tuple(o.shape) for o in outs] == [(k,) + tuple(c) for c in canvases]
    assert all(o.dtype == dtype and o.is_cuda for o in outs)
    base = outs[0].untyped_storage().data_ptr()
    assert all(o.untyped_storage().data_ptr() == base and (o.data_ptr() - outs[0].data_ptr()) % 16 == 0 for o in outs)
    for o in outs:
        assert (o.permute(1, 2, 0) if nhwc else o).is_contiguous()


def assert_items(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert_bits(g, w, f"{what} item {i}")


# ---- the base case ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_format", ("nchw", "nhwc"))
@pytest.mark.parametrize("filt", ref.FILTERS)
def test_base_case_equals_the_loop_for_every_dtype_pair(aa, filt, out_format):
    for gdtype in DTYPES:
        gs = gpu_grads(ref.BASE_SIZES, ref.BASE_K, gdtype)
        for dtype in DTYPES:
            want = looped(aa, filt, gs, ref.BASE_HW, ref.BASE_REGIONS, ref.BASE_FLIPS, dtype)
            got = call(aa, gs, ref.BASE_HW, MODE[filt], regions=ref.BASE_REGIONS, flips=ref.BASE_FLIPS, dtype=dtype, out_format=out_format)
            assert tuple(got.shape) == (5, ref.BASE_K) + ref.BASE_HW and got.dtype == dtype
            assert got.is_contiguous(memory_format=torch.channels_last if out_format == "nhwc" else torch.contiguous_format)
            assert_bits(got, torch.stack(want), f"{filt} {gdtype} -> {dtype} {out_format}")
    # dtype=None is the gradients' dtype
    assert call(aa, gs, ref.BASE_HW, MODE[filt], regions=ref.BASE_REGIONS).dtype == torch.bfloat16


@pytest.mark.parametrize("filt", ref.ORACLE_FILTERS)
def test_base_case_equals_the_restated_gather_form(aa, filt):
    gs = gpu_grads(ref.BASE_SIZES, ref.BASE_K)
    for flips in (None, ref.BASE_FLIPS):
        want = ref.gather_backward(filt, ref.grads(ref.BASE_SIZES, ref.BASE_K), ref.BASE_HW, ref.BASE_REGIONS, flips)
        got = call(aa, gs, ref.BASE_HW, MODE[filt], regions=ref.BASE_REGIONS, flips=flips)
        assert_items(list(got), [torch.from_numpy(w) for w in want], f"{filt} flips {flips is not None}")


def test_identity_item_is_its_gradient_and_zero_outside(aa):
    gs = gpu_grads(ref.BASE_SIZES, ref.BASE_K)
    got = call(aa, gs, ref.BASE_HW, "bicubic", regions=ref.BASE_REGIONS, flips=ref.BASE_FLIPS)[ref.IDENTITY_ITEM]
    y0, x0, h, w = ref.BASE_REGIONS[ref.IDENTITY_ITEM]
    assert_bits(got[:, y0:y0 + h, x0:x0 + w], gs[ref.IDENTITY_ITEM], "identity")
    outside = torch.ones(ref.BASE_HW, dtype=torch.bool)
    outside[y0:y0 + h, x0:x0 + w] = False
    assert not kit_gpu.bits(got)[:, outside].any()


@pytest.mark.parametrize("k", ref.K_VALUES)
def test_class_loop_tails(aa, k):
    gs = gpu_grads(ref.BASE_SIZES, k, seed=k)
    for out_format in ("nchw", "nhwc"):
        got = call(aa, gs, ref.BASE_HW, "bicubic", regions=ref.BASE_REGIONS, flips=ref.BASE_FLIPS, out_format=out_format)
        assert_bits(got, torch.stack(looped(aa, "cubic", gs, ref.BASE_HW, ref.BASE_REGIONS, ref.BASE_FLIPS, torch.float32)), f"K={k} {out_format}")


# ---- lists, many items, long rows, seams ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_format", ("nchw", "nhwc"))
def test_list_canvases(aa, out_format):
    canvases, regions, sizes = ref.list_case()
    flips = [True, False, False, True]
    gs = gpu_grads(sizes, 3, torch.float16, seed=4)
    got = call(aa, gs, canvases, "box", regions=regions, flips=flips, dtype=torch.bfloat16, out_format=out_format)
    check_list(got, canvases, 3, torch.bfloat16, nhwc=out_format == "nhwc")
    assert_items(got, looped(aa, "box", gs, canvases, regions, flips, torch.bfloat16), f"list {out_format}")
    want = ref.gather_backward("box", [g.float().cpu().numpy() for g in gs], canvases, regions, flips)
    assert_items(call(aa, gs, canvases, "box", regions=regions, flips=flips, dtype=torch.float32), [torch.from_numpy(w) for w in want], "list restated")


def test_seventy_items(aa):
    canvas, regions, sizes = ref.seventy_case()
    gs = gpu_grads(sizes, 3, seed=70)
    flips = [i % 3 == 0 for i in range(70)]
    got = call(aa, gs, canvas, regions=regions, flips=flips)
    assert_bits(got, torch.stack(looped(aa, "linear", gs, canvas, regions, flips, torch.float32)), "seventy")
    got = call(aa, gs, [canvas] * 70, regions=regions, flips=flips, out_format="nhwc")
    check_list(got, [canvas] * 70, 3, torch.float32, nhwc=True)
    assert_items(got, looped(aa, "linear", gs, canvas, regions, flips, torch.float32), "seventy as a list")


@pytest.mark.parametrize("filt", ("linear", "box", "lanczos"))
def test_long_adjoint_rows_and_wide_seams(aa, filt):
    for (canvas, regions, sizes), k in ((ref.long_rows_case(), 2), (ref.seams_case(), 5)):
        gs = gpu_grads(sizes, k, seed=sizes[0][1])
        for flips in (None, [True]):
            got = call(aa, gs, canvas, MODE[filt], regions=regions, flips=flips)
            assert_bits(got, torch.stack(looped(aa, filt, gs, canvas, regions, flips, torch.float32)), f"{filt} {canvas} flips {flips}")
    # one adjoint row of 300 taps: the 1 x 1 region that went to (4, 300), alone on a canvas of its own
    gs = gpu_grads([(4, 300)], 3, seed=300)
    got = call(aa, gs, [(2, 3)], MODE[filt], regions=[(1, 1, 1, 1)])
    assert_items(got, looped(aa, filt, gs, [(2, 3)], [(1, 1, 1, 1)], None, torch.float32), f"{filt} 1 x 1")


# ---- None items -----------------------------------------------------------------------------------------------------------------------
def test_none_items(aa):
    gs = gpu_grads(ref.BASE_SIZES, ref.BASE_K, torch.bfloat16)
    some = [gs[0], None, gs[2], None, gs[4]]
    for out_format in ("nchw", "nhwc"):
        got = call(aa, some, ref.BASE_HW, regions=ref.BASE_REGIONS, flips=ref.BASE_FLIPS, out_format=out_format)
        assert_bits(got, torch.stack(looped(aa, "linear", some, ref.BASE_HW, ref.BASE_REGIONS, ref.BASE_FLIPS, torch.bfloat16)), f"None items {out_format}")
        assert not kit_gpu.bits(got[1]).any() and not kit_gpu.bits(got[3]).any()
    # a None entry needs no region
    got = call(aa, some, ref.BASE_HW, regions=[ref.BASE_REGIONS[0], None, ref.BASE_REGIONS[2], None, ref.BASE_REGIONS[4]], flips=ref.BASE_FLIPS)
    assert_bits(got, torch.stack(looped(aa, "linear", some, ref.BASE_HW, ref.BASE_REGIONS, ref.BASE_FLIPS, torch.bfloat16)), "None regions")
    # every item None: K, the dtype and the device are stated
    none = call(aa, [None] * 5, ref.BASE_HW, channels=ref.BASE_K, dtype=torch.float16, device="cuda")
    assert tuple(none.shape) == (5, ref.BASE_K) + ref.BASE_HW and none.dtype == torch.float16 and none.is_cuda and not kit_gpu.bits(none).any()
    outs = call(aa, [None] * 3, [(4, 9), (7, 3), (1, 5)], channels=3, dtype=torch.float32, device=torch.device("cuda", torch.cuda.current_device()))
    check_list(outs, [(4, 9), (7, 3), (1, 5)], 3, torch.float32)
    assert all(not kit_gpu.bits(o).any() for o in outs)


# ---- views, determinism, empty input, launches ------------------------------------------------------------------------------------------
def pitched(g, k):
    """g [K, oh, ow] as a crop of a larger tensor: an odd element offset, a row pitch and a plane pitch that are no multiples of 4."""
    kk, oh, ow = g.shape
    pitch = ow + 5 + (1 if (ow + 5) % 4 == 0 else 0)
    plane = oh * pitch + 3
    plane += 1 if plane % 4 == 0 else 0
    off = 1 + 2 * (k % 2)
    buf = torch.full((off + kk * plane + 8,), float("nan"), dtype=g.dtype, device="cuda")
    v = buf.as_strided((kk, oh, ow), (plane, pitch, 1), off)
    v.copy_(g)
    assert (v.data_ptr() // g.element_size()) % 2 == 1 and not v.is_contiguous()
    return v


@pytest.mark.parametrize("gdtype", (torch.float32, torch.bfloat16))
def test_pitched_gradients_are_read_in_place(aa, gdtype):
    gs = gpu_grads(ref.BASE_SIZES, ref.BASE_K, gdtype)
    views = [pitched(g, i) for i, g in enumerate(gs)]
    kw = dict(regions=ref.BASE_REGIONS, flips=ref.BASE_FLIPS)
    want = call(aa, gs, ref.BASE_HW, "bicubic", **kw)
    assert_bits(call(aa, views, ref.BASE_HW, "bicubic", **kw), want, f"pitched {gdtype}")
    a = kit_gpu.count_launches(lambda: aa.resize_many_back_backward(gs, ref.BASE_HW, "bicubic", **kw))
    b = kit_gpu.count_launches(lambda: aa.resize_many_back_backward(views, ref.BASE_HW, "bicubic", **kw))
    assert len(a) == len(b) == 2, (a, b)
    # columns that are not consecutive are copied first: the same bits
    t = [g.permute(0, 2, 1).contiguous().permute(0, 2, 1) for g in gs]
    assert t[0].stride(2) != 1
    assert_bits(call(aa, t, ref.BASE_HW, "bicubic", **kw), want, "transposed")


def test_a_second_call_gives_the_same_bits(aa):
    gs = gpu_grads(ref.BASE_SIZES, ref.BASE_K, torch.float16)
    kw = dict(regions=ref.BASE_REGIONS, flips=ref.BASE_FLIPS, dtype=torch.float32)
    assert_bits(call(aa, gs, ref.BASE_HW, "lanczos", **kw), call(aa, gs, ref.BASE_HW, "lanczos", **kw), "a second call")
    # nor do they depend on N: item 2 alone
    alone = call(aa, gs[2:3], ref.BASE_HW, "lanczos", regions=ref.BASE_REGIONS[2:3], flips=ref.BASE_FLIPS[2:3], dtype=torch.float32)
    assert_bits(alone[0], call(aa, gs, ref.BASE_HW, "lanczos", **kw)[2], "alone")


def test_empty_input(aa):
    y = call(aa, [], (12, 16), channels=7, dtype=torch.bfloat16, device="cuda", out_format="nhwc")
    assert tuple(y.shape) == (0, 7, 12, 16) and y.dtype == torch.bfloat16 and y.is_cuda
    assert call(aa, [], [], channels=7, dtype=torch.float32) == []


def test_two_launches_whatever_n(aa):
    canvas, regions, sizes = ref.seventy_case()
    gs = gpu_grads(sizes, 3, seed=70)
    call(aa, gs, canvas, regions=regions)  # (code objects loaded)
    one = kit_gpu.count_launches(lambda: aa.resize_many_back_backward(gs[:1], canvas, regions=regions[:1]))
    seventy = kit_gpu.count_launches(lambda: aa.resize_many_back_backward(gs, canvas, regions=regions))
    assert len(one) == 2 and len(seventy) == 2, (one, seventy)


# ---- autograd -------------------------------------------------------------------------------------------------------------------------
def canvas_gpu(dtype=torch.float32, channels_last=False):
    t = torch.from_numpy(np.array(fwd_ref.BASE_CANVAS)).cuda().to(dtype)
    return t.contiguous(memory_format=torch.channels_last) if channels_last else t


def loss_of(outs, gs, use=None):
    return sum((o.float() * g.float()).sum() for i, (o, g) in enumerate(zip(outs, gs)) if use is None or i in use)


@pytest.mark.parametrize("channels_last", (False, True), ids=("planar", "channels_last"))
@pytest.mark.parametrize("pred_dtype,out_dtype", [(torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16)])
def test_autograd_of_a_batch_is_the_explicit_call(aa, pred_dtype, out_dtype, channels_last):
    pred = canvas_gpu(pred_dtype, channels_last).requires_grad_(True)
    kw = dict(regions=ref.BASE_REGIONS, flips=ref.BASE_FLIPS)
    with kit_gpu.gpu_error_ends_the_session("resize_many_back under autograd"):
        outs = aa.resize_many_back(pred, ref.BASE_SIZES, "bicubic", out_dtype=out_dtype, **kw)
    assert all(o.requires_grad and o.dtype == out_dtype for o in outs)
    # the forward's values and arena are what they are without autograd
    plain = aa.resize_many_back(pred.detach(), ref.BASE_SIZES, "bicubic", out_dtype=out_dtype, **kw)
    assert_items([o.detach() for o in outs], plain, "forward under autograd")
    assert [o.data_ptr() - outs[0].data_ptr() for o in outs] == [o.data_ptr() - plain[0].data_ptr() for o in plain]
    gs = gpu_grads(ref.BASE_SIZES, ref.BASE_K, out_dtype, seed=9)
    with kit_gpu.gpu_error_ends_the_session("resize_many_back's backward"):
        got, = torch.autograd.grad(loss_of(outs, gs), pred)
    fmt = "nhwc" if channels_last else "nchw"
    want = call(aa, gs, ref.BASE_HW, "bicubic", dtype=pred_dtype, out_format=fmt, **kw)
    assert got.dtype == pred_dtype and tuple(got.shape) == tuple(pred.shape)
    assert_bits(got, want, f"autograd {pred_dtype} -> {out_dtype} {fmt}")
    # a loss that uses items 0 and 2 only leaves the other canvases +0.0
    outs = aa.resize_many_back(pred, ref.BASE_SIZES, "bicubic", out_dtype=out_dtype, **kw)
    got, = torch.autograd.grad(loss_of(outs, gs, use=(0, 2)), pred)
    want = call(aa, [gs[0], None, gs[2], None, None], ref.BASE_HW, "bicubic", dtype=pred_dtype, out_format=fmt, **kw)
    assert_bits(got, want, "two items used")
    assert not kit_gpu.bits(got[1]).any() and not kit_gpu.bits(got[3]).any() and not kit_gpu.bits(got[4]).any()


def test_autograd_of_a_list_and_through_views(aa):
    srcs, regions, sizes = fwd_ref.list_case()
    canvases = [tuple(s.shape[1:]) for s in srcs]
    items = [torch.from_numpy(np.array(s)).cuda().requires_grad_(i != 1) for i, s in enumerate(srcs)]
    gs = gpu_grads(sizes, 3, seed=5)
    outs = aa.resize_many_back(items, sizes, "bilinear", regions=regions)
    got = torch.autograd.grad(loss_of(outs, gs), [items[0], items[2], items[3]])
    want = call(aa, gs, canvases, "bilinear", regions=regions)
    assert_items(list(got), [want[0], want[2], want[3]], "list")
    assert all(g.shape == t.shape for g, t in zip(got, (items[0], items[2], items[3])))
    # pred[:, :, 1:, 2:]: the gradient reaches the base through the view
    base = canvas_gpu().requires_grad_(True)
    view = base[:, :, 1:, 2:]
    regions = [(0, 0, 11, 14), (1, 2, 6, 9), (3, 0, 1, 1), (0, 5, 11, 1), (2, 3, 5, 7)]
    outs = aa.resize_many_back(view, ref.BASE_SIZES, "bicubic", regions=regions, flips=ref.BASE_FLIPS)
    gs = gpu_grads(ref.BASE_SIZES, ref.BASE_K, seed=6)
    got, = torch.autograd.grad(loss_of(outs, gs), base)
    want = call(aa, gs, (11, 14), "bicubic", regions=regions, flips=ref.BASE_FLIPS)
    assert_bits(got[:, :, 1:, 2:], want, "through a view")
    assert not kit_gpu.bits(got[:, :, :1]).any() and not kit_gpu.bits(got[:, :, :, :2]).any()


def test_nothing_requires_grad_without_autograd_or_with_a_reduction(aa):
    pred = canvas_gpu().requires_grad_(True)
    with torch.no_grad():
        assert not any(o.requires_grad for o in aa.resize_many_back(pred, ref.BASE_SIZES, regions=ref.BASE_REGIONS))
    for reduce in ("argmax", "greater"):
        outs = aa.resize_many_back(pred, ref.BASE_SIZES, regions=ref.BASE_REGIONS, reduce=reduce)
        assert all(o.grad_fn is None and not o.requires_grad for o in outs)
    assert all(o.grad_fn is None for o in aa.resize_many_back(pred.detach(), ref.BASE_SIZES, regions=ref.BASE_REGIONS))


# ---- the dense check ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", ref.FILTERS)
def test_dense_bound_and_adjoint_identity(aa, filt):
    """worst err / bound <= 1 against the float64 adjoint, and <R(x), G> == <x, B(G)> with the GPU forward, within the two bounds."""
    x = fwd_ref.BASE_CANVAS
    g_np = ref.grads(ref.BASE_SIZES, ref.BASE_K)
    gs = gpu_grads(ref.BASE_SIZES, ref.BASE_K)
    kw = dict(regions=ref.BASE_REGIONS, flips=ref.BASE_FLIPS)
    got = call(aa, gs, ref.BASE_HW, MODE[filt], **kw).cpu().numpy().astype(np.float64)
    want, bb = cached(("dense", filt), lambda: ref.dense_backward(filt, g_np, ref.BASE_HW, ref.BASE_REGIONS, ref.BASE_FLIPS))
    r = ref.worst_ratio(list(got), want, bb)
    vals = [v.cpu().numpy().astype(np.float64) for v in aa.resize_many_back(canvas_gpu(), ref.BASE_SIZES, MODE[filt], **kw)]
    _, fb = fwd_ref.dense_values(filt, x, ref.BASE_REGIONS, ref.BASE_SIZES, ref.BASE_FLIPS)
    lhs = sum(float((v * g).sum()) for v, g in zip(vals, g_np))
    rhs = float((x.astype(np.float64) * got).sum())
    allowed = sum(float((np.abs(g) * b).sum()) for g, b in zip(g_np, fb)) + sum(float((np.abs(x[i].astype(np.float64)) * b).sum()) for i, b in enumerate(bb))
    print(f"{filt}: backward err / bound {r:.3f}, adjoint |{lhs:.9g} - {rhs:.9g}| / {allowed:.3g} = {abs(lhs - rhs) / allowed:.3f}")
    assert r <= 1.0
    assert abs(lhs - rhs) <= allowed
