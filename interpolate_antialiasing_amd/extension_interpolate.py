"""Drop-in operator surface of the reference's pybind11 module, running on MI355X.

Mirrors step_two_dot_two/extension_interpolate.cpp:46-51 (same names, argument meaning, error behaviour):

    linear_forward(input, output_size, align_corners=False)   -> Tensor      (:7-14)
    nearest_forward(input, output_size, align_corners=False)  -> Tensor      (:26-33; "it's not nearest but box")
    cubic_forward(input, output_size, align_corners=False)    -> Tensor      (:35-42)
    linear_backward(grad_output, output_size, input_size, align_corners=False) -> Tensor   (:16-24)
    forward(...)                                               legacy name of linear_forward used by every other
                                                               step (step_three/extension_interpolate.cpp:17-19)
plus cubic_backward / nearest_backward (the commented-out intent at test.py:111-116), and Pillow's two other antialiasing filters
with the same signatures: lanczos_forward / hamming_forward, lanczos_backward / hamming_backward (PIL.Image.LANCZOS / HAMMING).

``output_size`` is (H, W); ``input_size`` is the full NCHW size (test.py:140-143).  antialias=True and
scale_factors={} are hard-wired exactly as in the reference wrappers.  The callee allocates and returns a fresh
tensor whose memory format follows the input (aa_interpolation_impl.h:739,752).

Differences, all additive:
  * tensors must live on a ROCm GPU — this package is the HIP path only and has no CPU implementation;
  * uint8 input is accepted for linear/cubic/box (the reference dispatches floating types only, :609-614): the
    default ``uint8_mode="pil"`` is bit-exact with PIL.Image.resize (integer arithmetic, uint8 intermediate);
    ``uint8_mode="harness"`` reproduces test.py:52-58,72,75 (float(), fp32 op, clamp for bicubic, truncating byte());
  * the backward is the TRUE adjoint of the antialiased forward (the reference header's is the non-AA one);
  * float16 / bfloat16 are differentiable too: the backward (gather form) takes 16-bit gradients and gives
    ``backward(g.float()).to(g.dtype)`` bit for bit in 2-D and 1-D: fp32 arithmetic in the fp32 backward's own order, one rounding to
    nearest even at the store (a 3-D backward rounds once per axis).  The registered autograd and interpolate_aa go through it;
    ``atomic=True`` stays float32 / float64 (adds rounded to 16 bits one by one are a different and worse result);
  * ``precision="fast"`` (f32 / f16 / bf16): the opt-in tolerance mode — FMA accumulation, results within 1e-4 relative of the
    reference's (BASELINE.json's float bar) instead of bit-identical; the default ``"exact"`` rounds product and sum separately in
    the reference's tap order.  In fast mode a NaN / Inf pixel also reaches outputs whose 16-byte-aligned window holds it;
  * ``alpha=True`` (uint8, ``uint8_mode="pil"``, 2 or 4 channels with straight alpha last): Pillow's RGBA / LA resize — colour is
    premultiplied by alpha, resampled, and converted back, bit-exact with PIL.Image.resize on an "RGBA" / "LA" image; the same
    size in and out returns a copy;
  * ``box=(x0, y0, x1, y1)`` on the five forwards (uint8, ``uint8_mode="pil"``): Pillow's ``Image.resize(size, resample, box=...)``, the
    sub-pixel source rectangle to resample from, bit-exact with Pillow.  PILLOW'S ORDER, X FIRST — unlike ``output_size``, which is
    (H, W).  Not a crop view: windows clip at the image's edge, so the neighbours outside the box contribute;
  * ``reducing_gap=g`` on the same forwards: Pillow's two-step resize (``Image.reduce`` by integer factors, then the filter), what
    ``Image.thumbnail`` does with 2.0.  The result is Pillow's ``reducing_gap`` result, not the plain one.  Two launches plus the table
    build, through a temporary uint8 tensor in the input's layout;
  * ``reduce(input, factor, box=None, alpha=False)``: Pillow's ``Image.reduce`` (integer box means), bit-exact;
  * ``resize_many_to_float(images, output_size, mode, boxes=None, flips=None, out_dtype=, out_format=, mean=, std=, alpha=False)``: ``resize_many``
    and the float conversion, normalisation, layout change and horizontal flips a model needs after it, in the same three launches.
  * ``resize_many_to_patches(images, patch, mode, sizes=, patch_format=, pad_to=, ...)``: the same list, every item resized to its own
    multiple of the patch, converted and cut into ViT patch tokens: one packed [sum T_i, C * ph * pw] matrix (or a zero-padded
    [N, L, C * ph * pw] one) from the same three launches;
  * ``resize_embed_to_tokens(embed, grids, mode, pad_to=, out_dtype=)``: the model's learned position grid [H0, W0, D] resampled to every
    item's token grid in the reference's fp32 arithmetic and packed in those tokens' row order, two launches whatever N; differentiable,
    and ``resize_embed_to_tokens_backward`` is its deterministic backward, the ordered fp32 sum of the items' gather-form adjoints;
  * ``resize_many_back(pred, sizes, mode, regions=, flips=, reduce=, threshold=, out_dtype=)``: the way back — a model's [N, K, H, W] float
    answer on the canvas resampled to every image's own size in the reference's fp32 arithmetic, as values, as the argmax over K or as
    ``> threshold``, two launches whatever N; with ``reduce="argmax"`` the K values of a pixel are never stored; ``activation="softmax"``
    or ``"sigmoid"`` puts bit-exactly defined probabilities in the values' place, here and in ``resize_many_back_merged``, which sums
    several test-time passes per image before the reduction;
  * ``resize_many(images, output_size, mode, boxes=None, alpha=False)``: a LIST of uint8 images of different sizes, each with its own box, into one
    dense [N, C, oH, oW] batch, bit-exact with the single-image call per item: three launches and one small host-to-device copy
    whatever N, no table cache traffic, no synchronisation.  ``sizes=``, ``offsets=``, ``fill=`` on both calls give every item its own
    output size and a place on the [oH, oW] canvas (Resize + CenterCrop, letterbox): cropped or padded, only the covered part computed;
  * ``reduce_many(images, factors, boxes=None)``: ``Image.reduce`` for such a list, every item with its own integer box and factors,
    in one launch; ``reduce_many_for_resize(images, output_size, mode, boxes=, sizes=, reducing_gap=)``: Pillow's first step of
    ``resize(..., reducing_gap=)`` for the list — the reduced images and shifted boxes that go into the three ragged calls above;
  * the same callables are registered as ``torch.ops.extension_interpolate.*``.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Sequence

import torch

from . import _lib, boxmath, tables

__all__ = ["reduce", "reduce_many", "reduce_many_for_resize", "resize_many", "resize_many_to_float", "resize_many_to_patches",
           "resize_embed_to_tokens", "resize_embed_to_tokens_backward", "resize_many_back", "resize_many_back_backward", "resize_many_back_merged", "linear_forward", "nearest_forward", "cubic_forward", "linear_backward", "cubic_backward",
           "nearest_backward", "forward", "linear_forward_nd", "cubic_forward_nd", "nearest_forward_nd", "linear_backward_nd",
           "cubic_backward_nd", "lanczos_forward", "hamming_forward", "lanczos_backward", "hamming_backward", "lanczos_forward_nd",
           "hamming_forward_nd", "lanczos_backward_nd", "hamming_backward_nd", "set_uint8_mode",
           "get_uint8_mode", "last_variant"]

_uint8_mode = "pil"
_plans = {}  # per call shape: (axis descriptors, workspace bytes); see _forward

_DTYPE_IDS = {torch.uint8: _lib.U8, torch.float32: _lib.F32, torch.float64: _lib.F64, torch.float16: _lib.F16,
              torch.bfloat16: _lib.BF16}
_GRAD_DTYPES = (torch.float32, torch.float64, torch.float16, torch.bfloat16)  # what the backward takes
_DTYPE_NAMES = {torch.float16: "Half", torch.bfloat16: "BFloat16", torch.int8: "Char", torch.int16: "Short",
                torch.int32: "Int", torch.int64: "Long", torch.bool: "Bool", torch.uint8: "Byte"}


def set_uint8_mode(mode: str) -> None:
    global _uint8_mode
    if mode not in ("pil", "harness"):
        raise ValueError("uint8_mode must be 'pil' or 'harness'")
    _uint8_mode = mode


def get_uint8_mode() -> str:
    return _uint8_mode


def last_variant() -> str:
    """Kernel variant the last forward on this thread dispatched to."""
    return _lib.last_variant()


# ---- argument checks with the reference's wording (ATen upsample_2d_common_check; s2.2:744-750) -------------
def _check_sizes(input_size: Sequence[int], output_size: Sequence[int]):
    if len(output_size) != 2:
        raise RuntimeError(f"It is expected output_size equals to 2, but got size {len(output_size)}")
    if len(input_size) != 4:
        raise RuntimeError(f"It is expected input_size equals to 4, but got size {len(input_size)}")
    n, c, h, w = (int(v) for v in input_size)
    oh, ow = int(output_size[0]), int(output_size[1])
    if not (h > 0 and w > 0 and oh > 0 and ow > 0):
        raise RuntimeError("Input and output sizes should be greater than 0, but got "
                           f"input (H: {h}, W: {w}) output (H: {oh}, W: {ow})")
    return n, c, h, w, oh, ow


def _memory_format(x: torch.Tensor, layout: int = _lib.NCHW) -> torch.Tensor:
    """The one dense copy of the 2-D resample paths (the reference walks arbitrary strides through TensorIterator): whatever no kernel
    reads where it lies comes through here, as the part of the image that will be read.  Tests count copies by wrapping this function."""
    return x.contiguous(memory_format=torch.channels_last if layout == _lib.NHWC else torch.contiguous_format)


def _layout_of(x: torch.Tensor, pitched: bool = True):
    """-> (tensor, layout, strides or None): the tensor as the kernels can read it — dense in one of the two layouts, a pitched view
    (strides given), or, failing both, a contiguous copy.  Callers pass the part of the image they will read (the hull, the box), so a
    copy is of that part only.  pitched=False: the caller's entry point has no strided form.
    A pitched view (aa_resample_fwd_strided) has rows of consecutive elements, any row pitch, and planes uniformly spaced — what a crop
    x[:, :, y0:y1, x0:x1] or (channels_last) a batch slice of a dense tensor is."""
    if x.is_contiguous():
        return x, _lib.NCHW, None
    if x.is_contiguous(memory_format=torch.channels_last):
        return x, _lib.NHWC, None
    n, c, h, w = x.shape
    sn, sc, sh, sw = strides = x.stride()
    if pitched and min(strides) >= 0 and x.numel() != 0:
        if sw == 1 and sh >= w and (c == 1 or n == 1 or sn == c * sc) and (c == 1 or sc >= 1):
            return x, _lib.NCHW, strides
        if sc == 1 and sw == c and sh >= w * c and c > 1:
            return x, _lib.NHWC, strides
    return _memory_format(x), _lib.NCHW, None


def _table_kind(dtype: torch.dtype, uint8_mode: Optional[str]) -> int:
    if dtype in (torch.float32, torch.float16, torch.bfloat16):  # 16-bit floats compute in fp32
        return _lib.TABLE_F32
    if dtype == torch.float64:
        return _lib.TABLE_F64
    mode = uint8_mode or _uint8_mode
    if mode not in ("pil", "harness"):
        raise ValueError("uint8_mode must be 'pil' or 'harness'")
    return _lib.TABLE_PIL if mode == "pil" else _lib.TABLE_F32


def _require_gpu(x: torch.Tensor, what: str):
    if not x.is_cuda:
        raise _lib.AAInterpError(
            f"{what}: expected a tensor on a ROCm GPU, got device '{x.device}'. interpolate_antialiasing_amd is the "
            "MI355X HIP path only and has no CPU implementation.")


def _user_scales(scale_factors, n: int):
    """ATen's optional per-axis scale factors (`scale_h`, `scale_w` of upsample_*2d; the reference hard-wires none,
    s2.2:11-13).  A given factor s replaces in/out by 1/s in area_pixel_compute_scale unless align_corners."""
    if scale_factors is None:
        return [0.0] * n
    sf = [float(v) if v is not None else 0.0 for v in scale_factors]
    if len(sf) != n or any(v < 0 for v in sf):
        raise RuntimeError(f"scale_factors must hold {n} positive values, got {list(scale_factors)}")
    return sf


def _plan_launch(L, th, tw, dt: int, layout: int, n: int, c: int, h: int, w: int, oh: int, ow: int, flags: int, cv=None):
    """The host-side plan of one launch, made under the device's guard: the two tables' axis descriptors, the workspace size, and the
    byref objects _launch hands over.  (th, tw ride along to keep the device buffers alive.)  cv: the uint8-to-float entry point's aa_convert."""
    ah, aw = th.axis(), tw.axis()
    pah, paw = ctypes.byref(ah), ctypes.byref(aw)
    if cv is None:
        ws_bytes = L.aa_workspace_bytes_ex(dt, layout, n, c, h, w, oh, ow, pah, paw, flags)
    else:
        ws_bytes = L.aa_workspace_bytes_u8_to_f32(layout, n, c, h, w, pah, paw, ctypes.byref(cv))
    return (ah, aw, ws_bytes, pah, paw, th, tw)


def _launch(L, name: str, x: torch.Tensor, out: torch.Tensor, plan, dt: int, layout: int, n: int, c: int, h: int, w: int, flags: int,
            strides=None, cv=None) -> bool:
    """Enqueue the resample of x [n, c, h, w] into out with a plan of _plan_launch: allocates the workspace, launches, checks.  x is dense
    in `layout`, or the pitched view `strides` describes; then -> False means that no kernel reads this view where it lies and nothing was
    launched: the caller makes the dense copy of its choice and calls again.  No device guard when x's device is the current one."""
    dev = x.device
    if dev.index != torch.cuda.current_device():
        with torch.cuda.device(dev):
            return _launch(L, name, x, out, plan, dt, layout, n, c, h, w, flags, strides, cv)
    ws_bytes, pah, paw = plan[2:5]
    stream = torch.cuda.current_stream(dev).cuda_stream
    if strides is not None:
        rc = L.aa_resample_fwd_strided(x.data_ptr(), out.data_ptr(), dt, layout, n, c, h, w, (ctypes.c_int64 * 4)(*strides), pah, paw, flags, stream)
        if rc == _lib.ERR_STRIDES:
            return False
    else:
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None  # (held until the launch is enqueued)
        pws = ws.data_ptr() if ws is not None else None
        if cv is None:
            rc = L.aa_resample_fwd_ex(x.data_ptr(), out.data_ptr(), pws, ws_bytes, dt, layout, n, c, h, w, pah, paw, flags, stream)
        else:
            rc = L.aa_resample_fwd_u8_to_f32(x.data_ptr(), out.data_ptr(), pws, ws_bytes, layout, n, c, h, w, pah, paw, ctypes.byref(cv), stream)
    _lib.check(rc, name)
    return True


def _forward(filter_id: int, name: str, input: torch.Tensor, output_size: Sequence[int], align_corners: bool,
             uint8_mode: Optional[str] = None, scale_factors: Optional[Sequence[float]] = None, out_dtype=None,
             out_format: Optional[str] = None, mean=None, std=None, precision: Optional[str] = None, alpha: bool = False,
             box: Optional[Sequence[float]] = None, reducing_gap: Optional[float] = None) -> torch.Tensor:
    if not isinstance(input, torch.Tensor):
        raise TypeError(f"{name}(): argument 'input' must be Tensor")
    if precision not in (None, "exact", "fast"):
        raise ValueError("precision must be 'exact' (default: the reference's results bit for bit) or 'fast' (within 1e-4 relative)")
    if box is not None or reducing_gap is not None:
        return _forward_boxed(filter_id, name, input, output_size, align_corners, uint8_mode, scale_factors, out_dtype, out_format, mean, std,
                              alpha, box, reducing_gap)
    flags = _lib.FLAG_FAST if precision == "fast" else 0
    if alpha:
        _check_alpha(name, input, uint8_mode, out_dtype, out_format, mean, std)
        flags |= _lib.FLAG_PREMUL_ALPHA
        if tuple(input.shape[2:]) == tuple(int(v) for v in output_size):
            _require_gpu(input, name)
            return input.clone()  # Pillow returns a copy: no lossy round trip through premultiplied values
    if out_dtype is not None or out_format is not None or mean is not None or std is not None:
        if input.dtype != torch.uint8 or out_dtype not in (None, torch.float32, torch.float16, torch.bfloat16):
            raise NotImplementedError("out_dtype / out_format / mean / std: the fused conversion takes uint8 input and gives float32")
        if uint8_mode == "pil":
            raise NotImplementedError("float32 output is the reference's fp32 arithmetic (uint8_mode='harness'), not Pillow's integers")
        return _forward_to_float(filter_id, name, input, output_size, align_corners, scale_factors, out_format, mean, std, flags,
                                 out_dtype or torch.float32)
    n, c, h, w, oh, ow = _check_sizes(input.shape, output_size)
    if input.numel() == 0 and (c == 0):  # empty batch allowed, nothing else (s2.2:747-750)
        raise RuntimeError(f"Non-empty 4D data tensor expected but got a tensor with sizes {list(input.shape)}")
    if input.dtype not in _DTYPE_IDS:
        raise NotImplementedError(f'"upsample_generic_Nd" not implemented for \'{_DTYPE_NAMES.get(input.dtype, str(input.dtype))}\'')
    _require_gpu(input, name)
    L = _lib.load()
    x, layout, strides = _layout_of(input)  # a crop / batch slice is read in place when a fused kernel takes it (no .contiguous() round trip)
    kind = _table_kind(x.dtype, uint8_mode)
    if kind == _lib.TABLE_PIL and align_corners:
        raise NotImplementedError("uint8_mode='pil' has no align_corners (Pillow has none); use uint8_mode='harness'")
    sh, sw = _user_scales(scale_factors, 2)
    if kind == _lib.TABLE_PIL and (sh or sw):
        raise NotImplementedError("uint8_mode='pil' has no scale factors (Pillow derives the scale from the sizes)")
    dev = x.device
    mf = torch.channels_last if layout == _lib.NHWC else torch.contiguous_format
    out = torch.empty((n, c, oh, ow), dtype=x.dtype, device=dev, memory_format=mf)
    if n == 0:
        return out
    dt = _DTYPE_IDS[x.dtype]
    # host-side plan: the two cached tables' axis descriptors and the workspace size for this exact call shape
    key = (filter_id, dt, layout, n, c, h, w, oh, ow, bool(align_corners), kind, sh, sw, dev.index, _lib.fused_epoch, bool(alpha))
    plan = _plans.get(key)
    if plan is None:
        with torch.cuda.device(dev):
            th, tw = tables.get_table_pair(filter_id, kind, h, oh, w, ow, align_corners, sh, sw, dev)
            plan = _plan_launch(L, th, tw, dt, layout, n, c, h, w, oh, ow, flags)
        if len(_plans) > 4096:
            _plans.clear()
        _plans[key] = plan
    if not _launch(L, name, x, out, plan, dt, layout, n, c, h, w, flags, strides):
        x = _memory_format(input)  # no kernel for this view: the dense copy after all, NCHW whatever the view's layout
        if layout != _lib.NCHW:  # (the plan was made for the view's layout)
            return _forward(filter_id, name, x, output_size, align_corners, uint8_mode, scale_factors, None, None, None, None, precision, alpha)
        _launch(L, name, x, out, plan, dt, layout, n, c, h, w, flags)
    return out


def _forward_boxed(filter_id: int, name: str, input: torch.Tensor, output_size: Sequence[int], align_corners: bool, uint8_mode, scale_factors,
                   out_dtype, out_format, mean, std, alpha: bool, box, reducing_gap) -> torch.Tensor:
    """Image.resize(size, resample, box, reducing_gap) as Pillow's Python and C order it: checks, the optional reduce with its shifted
    box, then a full box (today's path, same tables, same variant), a plain crop, or the box tables.  Every check comes before any GPU use."""
    what = "box" if box is not None else "reducing_gap"
    gap = boxmath.check_reducing_gap(reducing_gap)
    if input.dtype != torch.uint8:
        raise NotImplementedError(f"{name}(): {what} is Pillow's uint8 resize; {input.dtype} images have none (the reference has no box)")
    if (uint8_mode or _uint8_mode) != "pil":
        raise NotImplementedError(f"{name}(): {what} is Pillow's arithmetic; uint8_mode='harness' has none (the reference has no box)")
    if out_dtype is not None or out_format is not None or mean is not None or std is not None:
        raise NotImplementedError(f"{name}(): {what} gives uint8 in the input's layout; out_dtype / out_format / mean / std do not apply")
    if align_corners or scale_factors is not None:
        raise NotImplementedError("uint8_mode='pil' has no align_corners and no scale factors (Pillow has neither)")
    if alpha:
        _check_alpha(name, input, uint8_mode, out_dtype, out_format, mean, std)
        if gap is not None:
            raise NotImplementedError(f"{name}(): alpha=True with reducing_gap: Pillow drops reducing_gap for RGBA / LA images; reduce(alpha=True) "
                                      "and a resize with the shifted box are the two steps, if that is what is wanted")
    n, c, h, w, oh, ow = _check_sizes(input.shape, output_size)
    bx = boxmath.check_box(box, w, h) if box is not None else (0.0, 0.0, float(w), float(h))

    def plain(x):  # today's call, unchanged
        return _forward(filter_id, name, x, output_size, False, "pil", None, None, None, None, None, None, alpha)

    x = input
    full = boxmath.axis_is_full(w, bx[0], bx[2]) and boxmath.axis_is_full(h, bx[1], bx[3])
    if gap is not None and not (full and (h, w) == (oh, ow)):
        plan = boxmath.reducing_plan(w, h, ow, oh, _lib.FILTER_NAMES[filter_id], bx, gap)
        if plan is not None:
            factor, rb, bx = plan
            boxmath.check_factor(factor)
            x = reduce(x, factor, rb)
            h, w = int(x.shape[2]), int(x.shape[3])
            full = boxmath.axis_is_full(w, bx[0], bx[2]) and boxmath.axis_is_full(h, bx[1], bx[3])
    if full:
        return plain(x)
    bx = boxmath.box_f32(bx)  # Pillow's C resize takes the box as floats
    if boxmath.axis_is_full(w, bx[0], bx[2]) and boxmath.axis_is_full(h, bx[1], bx[3]):
        return plain(x)
    _require_gpu(x, name)
    if boxmath.is_plain_crop(bx, ow, oh):  # Pillow's C: integer offsets and a box of the output's size is a crop, no filter
        x0, y0 = int(bx[0]), int(bx[1])
        crop = x[:, :, y0:y0 + oh, x0:x0 + ow]
        t, lay, _ = _layout_of(crop)  # (the layout follows the input's; a view no kernel reads was copied here already)
        mf = torch.channels_last if lay == _lib.NHWC else torch.contiguous_format
        out = t if t is not crop else crop.clone(memory_format=mf)
        if alpha and n:  # (Pillow converts to premultiplied and back around the crop as around any resize)
            L = _lib.load()
            lay = _lib.NHWC if mf == torch.channels_last else _lib.NCHW
            with torch.cuda.device(out.device):
                s = torch.cuda.current_stream(out.device).cuda_stream
                _lib.check(L.aa_premultiply_u8(out.data_ptr(), out.data_ptr(), lay, n, c, oh, ow, s), name)
                _lib.check(L.aa_unpremultiply_u8(out.data_ptr(), lay, n, c, oh, ow, s), name)
        return out
    return _forward_box(filter_id, name, x, oh, ow, bx, alpha)


def _forward_box(filter_id: int, name: str, input: torch.Tensor, oh: int, ow: int, bx, alpha: bool) -> torch.Tensor:
    """The resampling kernels, untouched, on the HULL of the box: per axis the hull [o, e) of all filter windows (boxmath.axis_hull) is
    handed to them as a pitched view of the input, with a table whose in_size is e - o (tables.get_box_table_pair).  Rows and columns
    outside the hull are neither read nor copied: where no fused kernel takes the view, the dense fallback copies the hull."""
    L = _lib.load()
    n, c, h, w = (int(v) for v in input.shape)
    fname = _lib.FILTER_NAMES[filter_id]
    oy, ey = boxmath.axis_hull(h, oh, bx[1], bx[3], fname)
    ox, ex = boxmath.axis_hull(w, ow, bx[0], bx[2], fname)
    if ey <= oy or ex <= ox:
        raise ValueError("box can't be empty")
    hull, layout, strides = _layout_of(input[:, :, oy:ey, ox:ex])  # (a view no kernel reads: a copy of the hull, never of the image)
    dev = hull.device
    mf = torch.channels_last if layout == _lib.NHWC else torch.contiguous_format
    out = torch.empty((n, c, oh, ow), dtype=torch.uint8, device=dev, memory_format=mf)
    if n == 0:
        return out
    flags = _lib.FLAG_PREMUL_ALPHA if alpha else 0
    hh, hw = ey - oy, ex - ox
    with torch.cuda.device(dev):
        # (th, tw are held until the launch is enqueued: the LRU may drop them at any later call)
        th, tw = tables.get_box_table_pair(filter_id, (oy, hh, oh, bx[1], bx[3]), (ox, hw, ow, bx[0], bx[2]), dev)
        plan = _plan_launch(L, th, tw, _lib.U8, layout, n, c, hh, hw, oh, ow, flags)
        if not _launch(L, name, hull, out, plan, _lib.U8, layout, n, c, hh, hw, flags, strides):
            hull = _memory_format(hull, layout)  # no kernel for this view: the dense copy of the hull (not of the image), in the hull's layout
            _launch(L, name, hull, out, plan, _lib.U8, layout, n, c, hh, hw, flags)
    return out


def reduce(input: torch.Tensor, factor, box: Optional[Sequence[int]] = None, *, alpha: bool = False) -> torch.Tensor:
    """Pillow's ``Image.reduce(factor, box)`` for uint8 images [N, C, H, W], bit-exact: every output pixel is the rounded mean of an
    fx x fy block of input pixels; the blocks of the last row and column (and the corner) may be partial.

    ORDER OF COORDINATES — PILLOW'S, X FIRST: ``factor`` is an int or **(fx, fy)** and ``box`` is **(x0, y0, x1, y1)**, an integer
    rectangle inside the image (default: all of it).  ``output_size`` elsewhere in this module is (H, W); these two are not.

    The result is [N, C, ceil((y1 - y0) / fy), ceil((x1 - x0) / fx)], uint8, in the input's layout.  One launch, no workspace; a crop or a
    batch slice of a larger tensor is read where it lies.  fx * fy <= 65536.  ``alpha=True`` ([N, 2 or 4, H, W], straight alpha last):
    premultiply, reduce, convert back, as Image.reduce does for RGBA / LA."""
    if not isinstance(input, torch.Tensor):
        raise TypeError("reduce(): argument 'input' must be Tensor")
    fx, fy = boxmath.check_factor(factor)
    if input.dim() != 4:
        raise RuntimeError(f"It is expected input_size equals to 4, but got size {input.dim()}")
    if input.dtype != torch.uint8:
        raise NotImplementedError(f"reduce(): Image.reduce's 8-bit arithmetic takes uint8 images, got {input.dtype}")
    n, c, h, w = (int(v) for v in input.shape)
    if not (h > 0 and w > 0 and c > 0):
        raise RuntimeError(f"Non-empty 4D data tensor expected but got a tensor with sizes {list(input.shape)}")
    x0, y0, x1, y1 = boxmath.check_int_box(box, w, h)
    if alpha and c not in (2, 4):
        raise ValueError(f"reduce(): alpha=True needs [N, 2 or 4, H, W] with straight alpha in the last channel, got {list(input.shape)}")
    _require_gpu(input, "reduce")
    L = _lib.load()
    x, layout, strides = _layout_of(input[:, :, y0:y1, x0:x1])  # (the box only: a view no kernel reads is copied, the rest of the image is not)
    h, w = y1 - y0, x1 - x0
    x0, y0, x1, y1 = 0, 0, w, h
    channels_last = layout == _lib.NHWC
    if channels_last and c > 4:  # interleaved pixels of up to 4 bytes; anything wider goes through planes
        x, layout, strides = x.contiguous(), _lib.NCHW, None
    mf = torch.channels_last if layout == _lib.NHWC else torch.contiguous_format
    dev = x.device
    ow, oh = boxmath.reduced_size((x0, y0, x1, y1), (fx, fy))
    out = torch.empty((n, c, oh, ow), dtype=torch.uint8, device=dev, memory_format=mf)
    if n == 0:
        return out
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        if alpha:  # a premultiplied copy of the box
            x = x.clone(memory_format=mf)
            strides = None
            _lib.check(L.aa_premultiply_u8(x.data_ptr(), x.data_ptr(), layout, n, c, h, w, stream), "reduce")
        cs = (ctypes.c_int64 * 4)(*strides) if strides is not None else None
        cb = (ctypes.c_int64 * 4)(x0, y0, x1, y1)
        _lib.check(L.aa_reduce_u8(x.data_ptr(), out.data_ptr(), layout, n, c, h, w, cs, cb, fx, fy, stream), "reduce")
        if alpha:
            _lib.check(L.aa_unpremultiply_u8(out.data_ptr(), layout, n, c, oh, ow, stream), "reduce")
    if channels_last and layout == _lib.NCHW:
        out = out.contiguous(memory_format=torch.channels_last)
    return out


def _many_class(t: torch.Tensor):
    """Layout class of one [C, H, W] item as it lies in memory: -> (interleaved pixels?, planar?).  The stride of an axis of one element
    never matters, so a single-channel image is both."""
    c, h, w = t.shape
    sc, sh, sw = t.stride()
    if min(sc, sh, sw) < 0:
        return False, False
    inter = (c == 1 or sc == 1) and (w == 1 or sw == c)
    planar = w == 1 or sw == 1
    return inter, planar


def resize_many(images, output_size: Sequence[int], mode: str = "bilinear", *, boxes=None, channels: Optional[int] = None,
                sizes=None, offsets=None, fill=0, alpha: bool = False, reducing_gap: Optional[float] = None, uint8_mode: Optional[str] = None, out_dtype=None,
                out_format: Optional[str] = None, mean=None, std=None, align_corners: bool = False,
                scale_factors: Optional[Sequence[float]] = None) -> torch.Tensor:
    """Resize a list of uint8 images of different sizes into one batch: ``y[i]`` is ``<mode>_forward(images[i][None], output_size,
    box=boxes[i])[0]`` bit for bit, i.e. ``PIL.Image.resize((ow, oh), FILTER, box=boxes[i])``.

    ``images``: a sequence of N uint8 GPU tensors [C, H_i, W_i] (or [1, C, H_i, W_i]), or one [N, C, H, W] tensor whose slices are the
    items.  Same C (1..4) and device for all.  Items are read where they lie, at any row pitch, plane pitch and byte offset (crops,
    slices), in one of two layout classes: interleaved pixels (``hwc.permute(2, 0, 1)``: the result is channels_last) or planes (rows of
    consecutive bytes: the result is contiguous).  An item in neither form is copied into the class of the others; of two classes in
    one list the minority is copied (a tie: the planar items).
    ``boxes``: None, or N entries, each None or (x0, y0, x1, y1) — PILLOW'S ORDER, X FIRST, unlike ``output_size`` = (H, W).
    ``mode``: bilinear | bicubic | nearest (the box filter) | lanczos | hamming.  Pillow's arithmetic only.
    N == 0 gives an empty [0, C, oh, ow] tensor; a list then says its C with ``channels=``.

    Placement (all keyword-only, all defaulting to the above): item i is resized to ITS OWN size and pasted onto the [oh, ow] canvas,

        R_i = PIL.Image.resize((vw_i, vh_i), FILTER, box=boxes[i]);  y[i, c, y, x] = R_i[y - py_i, x - px_i, c] where that exists, else fill[c]

    bit for bit.  Only the part of R_i that lies on the canvas is computed; an item wholly off the canvas is legal and all fill.
    ``sizes``: None, or N entries, each None (``output_size``) or (vh, vw), height first like ``output_size``.
    ``offsets``: None, "center", or N entries, each None (= (0, 0)) or integers (py, px); negative crops, positive pads.  "center", per
    axis: ``-int(round((v - o) / 2.0))`` for v >= o (torchvision's center_crop), ``(o - v) // 2`` for v < o.
    ``fill``: one int or C ints in 0..255 (default 0); without ``sizes`` / ``offsets`` it has no effect.
    ``Resize(256)`` + ``CenterCrop(224)`` is ``sizes=boxmath.fit_sizes(shapes, shorter=256), offsets="center"`` on a 224 x 224 canvas; a
    letterbox is ``sizes=boxmath.fit_sizes(shapes, longer=640), offsets="center", fill=114`` on a 640 x 640 one.

    ``alpha=True`` (2 or 4 channels, STRAIGHT alpha last): every item is resized the way Pillow resizes an "LA" / "RGBA" image — colour
    premultiplied by alpha, resampled, converted back with the resampled alpha — so ``y[i]`` is ``<mode>_forward(images[i][None], ...,
    box=boxes[i], alpha=True)[0]``, and with placement ``R_i`` above is the RGBA / LA resize.  ``fill`` is written as given (straight
    values, never converted).  An item whose own size equals its image's and whose box is None or the whole image is Pillow's copy and
    comes out unchanged.  Same three launches, same workspace: the horizontal pass premultiplies as it reads, the vertical pass converts back.

    Three launches and one non-blocking copy of a packed descriptor whatever N; every hull, ksize and offset is host arithmetic
    (aa_many_plan), so nothing is read back, and the table caches are neither read nor written.  Not built here: reducing_gap,
    uint8_mode="harness", float images or outputs, align_corners, scale factors (each raises NotImplementedError); float, normalised,
    flipped output in either layout is ``resize_many_to_float``, packed ViT patch tokens are ``resize_many_to_patches``.  Pillow's
    ``reducing_gap`` is a step of its own, ``reduce_many_for_resize``, whose images and boxes go into any of the three calls."""
    name = "resize_many"
    for opt, given in (("reducing_gap", reducing_gap is not None), ("out_dtype", out_dtype is not None),
                       ("out_format", out_format is not None), ("mean", mean is not None), ("std", std is not None),
                       ("align_corners", bool(align_corners)), ("scale_factors", scale_factors is not None)):
        if given:
            hint = "; reduce_many_for_resize() is that step for a list, its results go into this call" if opt == "reducing_gap" else ""
            raise NotImplementedError(f"{name}(): {opt} is not built for a list of images; the single-image forwards have it{hint}")
    if (uint8_mode or _uint8_mode) != "pil":
        if (uint8_mode or _uint8_mode) != "harness":
            raise ValueError("uint8_mode must be 'pil' or 'harness'")
        raise NotImplementedError(f"{name}(): uint8_mode='harness' is not built for a list of images (Pillow's arithmetic only)")
    return _resize_many(name, images, output_size, mode, boxes, channels, None, (sizes, offsets, fill), bool(alpha))


def resize_many_to_float(images, output_size: Sequence[int], mode: str = "bilinear", *, boxes=None, flips=None,
                         channels: Optional[int] = None, sizes=None, offsets=None, fill=0, out_dtype=torch.float32, out_format: Optional[str] = None, mean=None,
                         std=None, alpha: bool = False) -> torch.Tensor:
    """``resize_many`` and the conversion a model needs after it, in the same three launches: with ``u = resize_many(images, output_size,
    mode, boxes=boxes)`` (Pillow's bytes), the result is, bit for bit,

        f = u.float();  f = (f - mean[c]) / std[c]  (fp32, when given);  y = f.to(out_dtype);  y[i] = y[i].flip(-1) where flips[i]

    written in ``out_format``: ``PIL.Image.resize(..., box=)``, ``transpose(FLIP_LEFT_RIGHT)``, a ToTensor-style conversion and Normalize
    folded into 0..255 units, without the uint8 batch, a float32 intermediate or a second pass.

    ``images``, ``output_size``, ``mode``, ``boxes``, ``channels``, ``sizes``, ``offsets``, ``fill``: exactly ``resize_many``'s; ``u`` above is
    then the placed ``resize_many(..., sizes=, offsets=, fill=)``: the fill byte is converted like any other byte, and a flip mirrors the
    whole canvas row.
    ``out_dtype``: torch.float32 | torch.float16 | torch.bfloat16 (rounded to nearest even once, at the store).
    ``out_format``: "nchw" | "nhwc" | None (the class of the items, as ``resize_many``'s output).
    ``mean`` / ``std``: None, or C floats each in 0..255 units (the convention of the single-image forwards), given together.
    ``flips``: None, or N truthy / falsy entries; a truthy entry mirrors that item's output left to right (RandomHorizontalFlip).
    ``alpha``: ``resize_many``'s; ``u`` above is then ``resize_many(..., alpha=True)``, and the alpha channel is converted with
    ``mean[C - 1]`` / ``std[C - 1]`` like any other.

    This is NOT the single-image forwards' ``out_dtype`` result: those resample in fp32 arithmetic throughout (uint8_mode="harness") and
    take no box; this call converts Pillow's byte, what torchvision's PIL pipeline produces."""
    name = "resize_many_to_float"
    if out_dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise NotImplementedError(f"{name}(): out_dtype {out_dtype} is not built; torch.float32, torch.float16 or torch.bfloat16")
    if out_format not in (None, "nchw", "nhwc"):
        raise ValueError("out_format must be 'nchw', 'nhwc' or None (same as the input)")
    if (mean is None) != (std is None):
        raise ValueError("mean and std must be given together")
    if _uint8_mode != "pil":
        raise NotImplementedError(f"{name}(): uint8_mode='harness' is not built for a list of images (Pillow's arithmetic only)")
    return _resize_many(name, images, output_size, mode, boxes, channels,
                        {"out_dtype": out_dtype, "out_format": out_format, "mean": mean, "std": std, "flips": flips}, (sizes, offsets, fill),
                        bool(alpha))


_MANY_MAX = (2 ** 31 - 1) // 4  # the library's bound on a size or an offset of the ragged call


def _many_int_pair(name: str, arg: str, i: int, v):
    """One (a, b) entry of sizes / offsets as two ints; anything that is not two integers raises, naming the argument and the item."""
    try:
        a, b = v
        if isinstance(a, bool) or isinstance(b, bool) or int(a) != a or int(b) != b:
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError(f"{name}(): {arg}[{i}] must be two integers, got {v!r}") from None
    return int(a), int(b)


def _many_fill(name: str, fill, c: int, lo: int = 0, hi: int = 255, note: str = ""):
    """fill of a canvas call, checked -> C ints in lo..hi.  note: what the range message adds (the dtype of a NEAREST call)."""
    try:
        fills = [fill] if not isinstance(fill, (tuple, list)) else list(fill)
        if any(isinstance(v, bool) or int(v) != v for v in fills):
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError(f"{name}(): fill must be one int or {c} ints in {lo}..{hi}, got {fill!r}") from None
    if len(fills) == 1 and not isinstance(fill, (tuple, list)):
        fills = fills * c
    if len(fills) != c:
        raise ValueError(f"{name}(): fill must be one int or one per channel ({c}), got {len(fills)}")
    for k, v in enumerate(fills):
        if not (lo <= v <= hi):
            raise ValueError(f"{name}(): fill[{k}] = {v} is outside {lo}..{hi}{note}")
    return [int(v) for v in fills]


def _many_places(name: str, sizes, offsets, n: int, oh: int, ow: int):
    """sizes / offsets, checked -> None or [(vh, vw, py, px)] per item."""
    if sizes is None and offsets is None:
        return None
    if sizes is not None and len(sizes) != n:
        raise ValueError(f"{name}(): sizes must hold one entry per image ({n}), got {len(sizes)}")
    center = isinstance(offsets, str)
    if center and offsets != "center":
        raise ValueError(f"{name}(): offsets must be None, 'center' or one entry per image, got {offsets!r}")
    if offsets is not None and not center and len(offsets) != n:
        raise ValueError(f"{name}(): offsets must hold one entry per image ({n}), got {len(offsets)}")
    places = []
    for i in range(n):
        vh, vw = oh, ow
        if sizes is not None and sizes[i] is not None:
            vh, vw = _many_int_pair(name, "sizes", i, sizes[i])
            if vh <= 0 or vw <= 0:
                raise ValueError(f"{name}(): sizes[{i}] = ({vh}, {vw}) must be positive")
            if vh > _MANY_MAX or vw > _MANY_MAX:
                raise ValueError(f"{name}(): sizes[{i}] = ({vh}, {vw}) is beyond the supported {_MANY_MAX}")
        py, px = 0, 0
        if center:
            py, px = boxmath.center_offset(vh, oh), boxmath.center_offset(vw, ow)
        elif offsets is not None and offsets[i] is not None:
            py, px = _many_int_pair(name, "offsets", i, offsets[i])
            if abs(py) > _MANY_MAX or abs(px) > _MANY_MAX:
                raise ValueError(f"{name}(): offsets[{i}] = ({py}, {px}) is beyond the supported {_MANY_MAX}")
        places.append((vh, vw, py, px))
    return places


def _many_pack_places(places):
    """None or [(vh, vw, py, px)] -> None or the aa_many_place records."""
    if places is None:
        return None
    precs = (_lib.ManyPlace * len(places))()
    for i, p in enumerate(places):
        precs[i].vH, precs[i].vW, precs[i].oy, precs[i].ox = p
    return precs


def _many_flips(name: str, flips, n: int):
    """flips of a ragged call, checked -> None or N bools."""
    if flips is None:
        return None
    flips = [bool(v) for v in flips]
    if len(flips) != n:
        raise ValueError(f"{name}(): flips must hold one entry per image ({n}), got {len(flips)}")
    return flips


def _many_output_size(name: str, output_size: Sequence[int], images_checked: bool = True):
    """output_size of a call with a canvas -> (oh, ow).  The calls look at its length before the images and at its values after them:
    images_checked False is the first look alone."""
    if len(output_size) != 2:
        raise RuntimeError(f"It is expected output_size equals to 2, but got size {len(output_size)}")
    oh, ow = int(output_size[0]), int(output_size[1])
    if images_checked and not (oh > 0 and ow > 0):
        raise RuntimeError(f"Input and output sizes should be greater than 0, but got output (H: {oh}, W: {ow})")
    return oh, ow


def _many_canvas(name: str, images, output_size: Sequence[int], channels: Optional[int], empty: str = "[0, C, oh, ow]", alpha: bool = False):
    """output_size and the images of a call with a canvas, checked in the calls' order -> (oh, ow, items, device of a batch tensor or
    None, N, C).  alpha: the call resizes the way Pillow resizes LA / RGBA."""
    _many_output_size(name, output_size, images_checked=False)
    items, dev0, n, c = _many_items(name, images, channels, empty)
    if alpha and c not in (2, 4):
        raise NotImplementedError(f"{name}(): alpha=True is built for 2- or 4-channel images with straight alpha last (Pillow's LA / RGBA "
                                  f"resize), got C = {c}")
    oh, ow = _many_output_size(name, output_size)
    return oh, ow, items, dev0, n, c


def _many_empty_device(dev0):
    """Where the empty result of N == 0 lives: the batch tensor's device, else the current GPU, else the CPU."""
    if dev0 is not None:
        return dev0
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")


def _many_convert(name: str, conv: dict, n: int, c: int):
    """The conversion options of resize_many_to_float, checked -> (aa_convert without its layout, flips or None, out_dtype)."""
    out_dtype = conv["out_dtype"]
    cv = _lib.Convert()
    cv.normalize = 0
    cv.flags = {torch.float16: _lib.FLAG_OUT_F16, torch.bfloat16: _lib.FLAG_OUT_BF16}.get(out_dtype, 0)
    mean, std = conv["mean"], conv["std"]
    if mean is not None:
        mean, std = [float(v) for v in mean], [float(v) for v in std]
        if len(mean) != c or len(std) != c or c > 4:
            raise RuntimeError(f"mean/std must hold one value per channel (C = {c} <= 4)")
        for i in range(c):
            if not math.isfinite(mean[i]):
                raise ValueError(f"{name}(): mean[{i}] = {mean[i]} is not finite")
            if not math.isfinite(std[i]) or std[i] == 0.0:
                raise ValueError(f"{name}(): std[{i}] = {std[i]} must be finite and not zero")
            cv.mean[i], cv.std[i] = mean[i], std[i]
        cv.normalize = 1
    return cv, _many_flips(name, conv["flips"], n), out_dtype


def _many_items(name: str, images, channels: Optional[int], empty: str):
    """The images of a ragged call -> ([C, H, W] items, the device of a batch tensor or None, N, C).  empty: the shape of the N == 0 result,
    for the message that asks for channels=."""
    if isinstance(images, torch.Tensor):
        if images.dim() != 4:
            raise RuntimeError(f"{name}(): one tensor must be [N, C, H, W], got {list(images.shape)}")
        if channels is None:
            channels = int(images.shape[1])
        items = list(images.unbind(0))
        dev0 = images.device
    else:
        items, dev0 = [], None
        for i, t in enumerate(images):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{name}(): images[{i}] must be Tensor")
            if t.dim() == 4 and t.shape[0] == 1:
                t = t[0]
            if t.dim() != 3:
                raise RuntimeError(f"{name}(): images[{i}] must be [C, H, W] or [1, C, H, W], got {list(t.shape)}")
            items.append(t)
    n = len(items)
    if n == 0 and channels is None:
        raise ValueError(f"{name}(): an empty list needs channels= (the C of the {empty} result)")
    c = int(channels) if channels is not None else int(items[0].shape[0])
    if not (1 <= c <= 4):
        raise ValueError(f"{name}(): images of 1 to 4 channels, got C = {c}")
    return items, dev0, n, c


def _many_box(bx, w: int, h: int):
    """One entry of boxes for a [h, w] image -> None, or the box as Pillow's C sees it: Pillow's checks and wording, then floats."""
    return None if bx is None else boxmath.box_f32(boxmath.check_box(bx, w, h))


def _many_check_items(name: str, items, c: int, boxes, out_size, dtypes=None):
    """Dtype, C, sizes, device and box of every item -> the boxes as Pillow's C sees them (None: the whole image).  out_size(i): the
    (H, W) item i is resized to, for the wording of the size check.  dtypes: None (uint8 only), or the dtypes the call copies (one per
    call, the first item's; more than one byte per element only with one channel)."""
    n = len(items)
    if boxes is not None and len(boxes) != n:
        raise ValueError(f"{name}(): boxes must hold one entry per image ({n}), got {len(boxes)}")
    checked = []
    for i, t in enumerate(items):
        if dtypes is not None:
            if t.dtype not in dtypes:
                raise NotImplementedError(f"{name}(): images[{i}] is {t.dtype}; built for {', '.join(str(d) for d in dtypes)}")
            if t.dtype != items[0].dtype:
                raise ValueError(f"{name}(): every image must have the same dtype: images[{i}] is {t.dtype}, images[0] {items[0].dtype}")
            if t.element_size() > 1 and c != 1:
                raise NotImplementedError(f"{name}(): images[{i}] is {t.dtype} with C = {c}; {t.dtype} maps have one channel (Pillow's "
                                          f"\"I;16\" and \"I\"), only torch.uint8 has up to 4")
        elif t.dtype != torch.uint8:
            raise NotImplementedError(f"{name}(): images[{i}] is {t.dtype}; a list of images is Pillow's uint8 resize only")
        if int(t.shape[0]) != c:
            raise ValueError(f"{name}(): every image must have the same C: images[{i}] has {int(t.shape[0])}, expected {c}")
        h, w = int(t.shape[1]), int(t.shape[2])
        if not (h > 0 and w > 0):
            oh, ow = out_size(i)
            raise RuntimeError(f"Input and output sizes should be greater than 0, but got input (H: {h}, W: {w}) output (H: {oh}, W: {ow})")
        if t.device != items[0].device:
            raise ValueError(f"{name}(): every image must be on the same device: images[{i}] is on {t.device}, images[0] on {items[0].device}")
        checked.append(_many_box(boxes[i] if boxes is not None else None, w, h))
    return checked


def _many_layout(items, c: int):
    """One layout class for the call: the majority's; whoever is not in it is copied.  -> (per-item classes, interleaved pixels?)"""
    classes = [_many_class(t) for t in items]
    n_inter = sum(1 for a, b in classes if a and not b)
    n_planar = sum(1 for a, b in classes if b and not a)
    return classes, c > 1 and n_inter > 0 and n_inter >= n_planar


def _many_fill_records(recs, items, classes, interleaved: bool, c: int, keep: list, eb: int = 1):
    """Where every item lies, in the call's class, into the leading fields that aa_many_image and aa_reduce_item share: data_dev, H, W
    and the three strides in bytes (eb per element).  Yields (i, record i) as each is written, so that the caller adds its own fields
    in the same pass.  An item outside the class is copied into it, and the copy appended to ``keep``: it must outlive the launches
    (the stream orders its release after them)."""
    for i, t in enumerate(items):
        if not classes[i][0 if interleaved else 1]:
            t = t.permute(1, 2, 0).contiguous().permute(2, 0, 1) if interleaved else t.contiguous()
            keep.append(t)
        r = recs[i]
        r.data_dev = t.data_ptr()
        r.H, r.W = int(t.shape[1]), int(t.shape[2])
        # (the stride of an axis of one element is arbitrary: hand over the class's own)
        r.stride_ch = (1 if interleaved else (t.stride(0) if c > 1 else 0)) * eb
        r.stride_row = (t.stride(1) if r.H > 1 else 0) * eb
        r.stride_px = (c if interleaved else 1) * eb
        yield i, r


def _many_records(items, classes, interleaved: bool, c: int, checked, flips, alpha: bool = False, eb: int = 1):
    """The aa_many_image records of the items in the call's class -> (records, the copies that must outlive the launches).  alpha: every
    record asks for Pillow's RGBA / LA resize; which items are Pillow's copies instead is the planner's decision."""
    recs, keep = (_lib.ManyImage * len(items))(), []
    for i, r in _many_fill_records(recs, items, classes, interleaved, c, keep, eb):
        bx = checked[i]
        if bx is not None:
            r.has_box = 1
            r.box[:] = bx
        if flips is not None and flips[i]:
            r.flags = _lib.MANY_FLIP_X
        if alpha:
            r.flags |= _lib.MANY_PREMUL_ALPHA
    return recs, keep


def _many_run(name: str, dev, desc_bytes: int, plan, alloc_out, launch):
    """What every ragged call ends with, on `dev`: a pinned block, ``plan(desc_host, desc_bytes, byref(workspace bytes))``, the
    non-blocking copy of the block, the workspace, the output of ``alloc_out()`` and ``launch(desc_host, desc_dev, out, workspace,
    stream)`` on the current stream -> (out, workspace).  Whatever the launch reads besides (copies of items) the caller keeps alive
    until this returns."""
    with torch.cuda.device(dev):
        desc_host = torch.empty(desc_bytes, dtype=torch.uint8, pin_memory=True)  # (the caching host allocator)
        ws_bytes = ctypes.c_size_t(0)
        _lib.check(plan(desc_host.data_ptr(), desc_bytes, ctypes.byref(ws_bytes)), name)
        desc_dev = torch.empty(desc_bytes, dtype=torch.uint8, device=dev)
        desc_dev.copy_(desc_host, non_blocking=True)  # (the host allocator holds the block until the copy has run)
        ws = torch.empty(max(ws_bytes.value, 16), dtype=torch.uint8, device=dev)
        out = alloc_out()
        rc = launch(desc_host.data_ptr(), desc_dev.data_ptr(), out, ws, torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, name)
    return out, ws


def _resize_many(name: str, images, output_size: Sequence[int], mode: str, boxes, channels: Optional[int], conv: Optional[dict],
                 place=(None, None, 0), alpha: bool = False) -> torch.Tensor:
    """resize_many (conv None) and resize_many_to_float (conv: its options): the checks, the layout class, the plan and the launches.
    place: (sizes, offsets, fill).  alpha: Pillow's RGBA / LA resize of every item."""
    if mode not in _lib.FILTER_IDS:
        raise ValueError(mode)
    filter_id = _lib.FILTER_IDS[mode]
    oh, ow, items, dev0, n, c = _many_canvas(name, images, output_size, channels, alpha=alpha)
    checked = _many_check_items(name, items, c, boxes, lambda i: (oh, ow))
    cv, flips, out_dtype = None, None, torch.uint8
    if conv is not None:
        cv, flips, out_dtype = _many_convert(name, conv, n, c)
    sizes, offsets, fill = place
    fills = _many_fill(name, fill, c)
    places = _many_places(name, sizes, offsets, n, oh, ow)
    if n == 0:
        return torch.empty((0, c, oh, ow), dtype=out_dtype, device=_many_empty_device(dev0))
    for t in items:
        _require_gpu(t, name)
    dev = items[0].device
    classes, interleaved = _many_layout(items, c)
    layout = _lib.NHWC if interleaved else _lib.NCHW
    out_nhwc = interleaved
    if cv is not None:
        if conv["out_format"] is not None:
            out_nhwc = conv["out_format"] == "nhwc"
        cv.out_layout = _lib.NHWC if out_nhwc else _lib.NCHW
    L = _lib.load()
    recs, keep = _many_records(items, classes, interleaved, c, checked, flips, alpha)
    precs = _many_pack_places(places)
    # (places that are all the whole canvas at offset 0 plan to the plain block: the tail of the larger one is then copied as it is
    # and never read)
    desc_bytes = L.aa_many_desc_bytes(n) if precs is None else L.aa_many_desc_bytes_placed(n)

    def plan(desc, nbytes, ws_bytes):
        if precs is None:
            return L.aa_many_plan(filter_id, layout, n, c, oh, ow, recs, desc, nbytes, ws_bytes)
        return L.aa_many_plan_placed(filter_id, layout, n, c, oh, ow, recs, precs, (ctypes.c_uint8 * 4)(*fills), desc, nbytes, ws_bytes)

    def launch(desc_host, desc_dev, out, ws, stream):
        if cv is None:
            return L.aa_resample_many_u8(desc_host, desc_dev, n, c, oh, ow, layout, out.data_ptr(), ws.data_ptr(), ws.numel(), stream)
        return L.aa_resample_many_u8_to_float(desc_host, desc_dev, n, c, oh, ow, layout, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                              ctypes.byref(cv), stream)

    mf = torch.channels_last if out_nhwc else torch.contiguous_format
    return _many_run(name, dev, desc_bytes, plan, lambda: torch.empty((n, c, oh, ow), dtype=out_dtype, device=dev, memory_format=mf), launch)[0]


_NEAREST_RANGE = {torch.uint8: (0, 255), torch.int16: (-32768, 32767), torch.int32: (-2 ** 31, 2 ** 31 - 1)}  # the dtypes the call copies


def resize_many_nearest(images, output_size: Sequence[int], *, boxes=None, flips=None, channels: Optional[int] = None, sizes=None,
                        offsets=None, fill=0, out_dtype=None) -> torch.Tensor:
    """The label maps of a ragged batch, with Pillow's ``Image.NEAREST``: what goes through the same crop, size, placement and flip as its
    image in segmentation, depth, instance-mask and panoptic training, where a filtered class id is a wrong class id.  Per item i, bit
    for bit,

        R_i = PIL.Image.resize((vw_i, vh_i), Image.NEAREST, box=boxes[i])    # vh_i, vw_i = sizes[i], or output_size
        y[i, c, Y, X] = R_i[Y - py_i, X - px_i, c] where that exists, else fill[c]
        y[i] = y[i].flip(-1) where flips[i]                                  # the whole canvas row, as resize_many_to_float does

    ``images``, ``boxes`` (Pillow's order, x first), ``channels``, ``sizes``, ``offsets`` (``"center"`` included) and ``flips`` are exactly
    ``resize_many`` / ``resize_many_to_float``'s arguments, with the same checks, the same two layout classes and the same reading of
    every item where it lies: pass the SAME ``boxes, sizes, offsets, flips`` to ``resize_many_to_float`` for the images and to this call
    for the masks.
    Items are ``torch.uint8`` with 1..4 channels (Pillow's "L", "LA", "RGB", "RGBA"; NEAREST treats every channel alike, so there is no
    ``alpha=``), or ``torch.int16`` / ``torch.int32`` with one channel ("I;16", "I"); one dtype per call.  Elements are copied, never
    computed with.
    ``fill``: one int or C ints within the dtype's range (255 as the ignore index of a uint8 map, -1 of an int32 one).
    ``out_dtype``: None (the items' dtype) or ``torch.int64``, for one channel only: exactly ``y.long()`` (zero-extended from uint8,
    sign-extended from int16 / int32), what ``cross_entropy`` takes, without the second pass.
    The result is contiguous for planar items and channels_last for interleaved ones; N == 0 gives an empty [0, C, oh, ow] tensor.

    Three things that are easy to get wrong:
    * This is NOT ``mode="nearest"`` of the other calls: that one is the box filter (the reference's naming), which averages.
    * It is Pillow's ``resize(box=)``, which for an integer box is NOT promised equal to ``crop(box).resize()``: the source index of
      output x is ``int(xo)`` after x additions of the step to ``xo = x0 + step / 2`` (``boxmath.nearest_indices``), and that sum starts
      from the box's x0, not from 0, so its rounding differs.  (Pillow serves "I;16" alone through its generic transform, which
      evaluates ``step * (x + 0.5) + x0`` afresh for every x; int16 items follow Pillow there, ``nearest_indices(closed_form=True)``,
      so an int16 map and a uint8 map of one geometry can differ by one source pixel where the two forms fall on either side of an
      integer, exactly as the two Pillow images do.)
    * A [K, H, W] stack of instance masks with K > 4 goes in as K single-plane items (``stack[k:k + 1]`` views) with the same box
      repeated, not as one K-channel item.

    Two launches and one non-blocking copy of a packed descriptor whatever N: a table kernel that runs Pillow's accumulation per item and
    axis, and a gather that writes every byte of the output.  Nothing is read back; the table caches are neither read nor written."""
    name = "resize_many_nearest"
    if out_dtype not in (None, torch.int64):
        raise NotImplementedError(f"{name}(): out_dtype {out_dtype} is not built; None (the items' dtype) or torch.int64")
    oh, ow, items, dev0, n, c = _many_canvas(name, images, output_size, channels)
    checked = _many_check_items(name, items, c, boxes, lambda i: (oh, ow), tuple(_NEAREST_RANGE))
    dtype = items[0].dtype if n else (images.dtype if isinstance(images, torch.Tensor) and images.dtype in _NEAREST_RANGE else torch.uint8)
    if out_dtype is torch.int64 and c != 1:
        raise NotImplementedError(f"{name}(): out_dtype torch.int64 is built for one channel (a class-id map), got C = {c}")
    flips = _many_flips(name, flips, n)
    places = _many_places(name, sizes, offsets, n, oh, ow)
    fills = _many_fill(name, fill, c, *_NEAREST_RANGE[dtype], note=f" ({dtype})")
    res_dtype = dtype if out_dtype is None else out_dtype
    if n == 0:
        return torch.empty((0, c, oh, ow), dtype=res_dtype, device=_many_empty_device(dev0))
    for t in items:
        _require_gpu(t, name)
    dev = items[0].device
    classes, interleaved = _many_layout(items, c)
    layout = _lib.NHWC if interleaved else _lib.NCHW
    eb = items[0].element_size()
    L = _lib.load()
    recs, keep = _many_records(items, classes, interleaved, c, checked, flips, eb=eb)  # (the library takes strides in bytes)
    precs = _many_pack_places(places)
    cfill = (ctypes.c_int32 * 4)(*(fills + [0] * (4 - c)))
    mf = torch.channels_last if interleaved else torch.contiguous_format
    return _many_run(
        name, dev, L.aa_many_desc_bytes_nearest(n),
        lambda desc, nbytes, ws_bytes: L.aa_many_plan_nearest(layout, eb, n, c, oh, ow, recs, precs, cfill, desc, nbytes, ws_bytes),
        lambda: torch.empty((n, c, oh, ow), dtype=res_dtype, device=dev, memory_format=mf),
        lambda desc_host, desc_dev, out, ws, stream: L.aa_resample_many_nearest(desc_host, desc_dev, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                                                out.element_size(), stream))[0]


# the dtypes resize_many_maps filters: Pillow's mode, the library's element id, the fill's range (None: a finite float)
_MAPS_MODES = {torch.uint16: ("I;16", _lib.MAPS_U16, (0, 65535)), torch.int32: ("I", _lib.MAPS_I32, (-2 ** 31, 2 ** 31 - 1)),
               torch.float32: ("F", _lib.MAPS_F32, None)}
_MAPS_NOT_BUILT = {"alpha": "Pillow's LA / RGBA resize is resize_many(alpha=True), uint8 only",
                   "reducing_gap": "Pillow's Image.reduce refuses \"I;16\"; reduce_many_for_resize is the uint8 step",
                   "out_dtype": "the result has the items' dtype", "mean": "the result has the items' dtype, not normalised",
                   "std": "the result has the items' dtype, not normalised", "out_format": "one channel has one layout",
                   "patch": "packed patch tokens are resize_many_to_patches, uint8 only"}


def resize_many_maps(maps, output_size: Sequence[int], mode: str = "bilinear", *, boxes=None, flips=None, channels: Optional[int] = None,
                     sizes=None, offsets=None, fill=0, overflow: str = "pillow", **not_built) -> torch.Tensor:
    """The measured maps of a ragged batch — depth and disparity stored as 16-bit PNG or float32, height maps, 16-bit medical and
    satellite rasters, int32 counters — FILTERED through the same crop, size, placement and flip as their image, with the arithmetic
    Pillow keeps for its three wide single-band modes.  Per item i, bit for bit,

        R_i = PIL.Image.resize((vw_i, vh_i), FILTER, box=boxes[i])          # vh_i, vw_i = sizes[i], or output_size
        y[i, 0, Y, X] = R_i[Y - py_i, X - px_i] where that exists, else fill
        y[i] = y[i].flip(-1) where flips[i]                                  # the whole canvas row

    ``maps``, ``boxes`` (Pillow's order, x first), ``channels``, ``sizes``, ``offsets`` (``"center"`` included) and ``flips`` are exactly
    ``resize_many_nearest``'s arguments, with the same checks and the same reading of every item where it lies (any row pitch; rows of a
    uint16 view may start on an odd element): pass the SAME ``boxes, sizes, offsets, flips`` as the images get.
    Items are ``torch.uint16`` (Pillow's "I;16"), ``torch.int32`` ("I") or ``torch.float32`` ("F"), one channel, one dtype per call; a
    [N, 1, H, W] tensor is the list of its items.  ``t.view(torch.uint16)`` of an int16 tensor is free — but this is NOT the bits
    ``resize_many_nearest`` gives for int16: NEAREST copies elements, this call computes with the UNSIGNED value.
    ``mode``: bilinear | bicubic | nearest (the box filter) | lanczos | hamming.
    ``fill``: an int in 0..65535 for uint16, within int32 for int32; a finite float for float32, written as ``float32(fill)``.
    ``overflow`` (uint16 only; accepted and ignored for the other two): ``"pillow"`` stores what Pillow stores, which is no clamp — with
    ``r`` the rounded sum, the low byte is ``CLIP8(r % 256)`` and the high byte ``CLIP8(r >> 8)``, so a negative ``r`` gives 0 but
    ``r > 65535`` gives ``0xFF00 | (r & 255)`` (bicubic or Lanczos overshoot beside a 65535 wraps, e.g. to 65302), after the horizontal
    pass too, and the vertical pass reads the wrapped value.  ``"clamp"`` stores ``min(max(r, 0), 65535)`` in both passes instead.
    The result is [N, 1, oh, ow] in the items' dtype, contiguous; N == 0 gives the empty tensor.

    The arithmetic (Resample.c, the 16bpc / 32bpc passes) is neither the uint8 fixed-point path of ``resize_many`` nor the fp32 path of
    the single-image forwards: coefficients are precompute_coeffs's normalised DOUBLES, every output of every pass is one double sum over
    its window in ascending order (product rounded, then the sum: no fused multiply-add), and the store rule — ``float32(ss)``; for the
    integer modes ``int(ss + 0.5)`` or ``int(ss - 0.5)`` by the sign — is applied after EACH pass.  Pillow runs the horizontal pass only
    if the width changes or the box does not span it, the vertical one likewise, and copies when the box has the size asked for at an
    integer offset; a skipped pass is not run as an identity filter.  int32 results beyond int32 are undefined in Pillow's C and
    unspecified here.

    Three launches and one non-blocking copy of a packed descriptor whatever N (two when no item's horizontal pass runs): a table kernel
    that evaluates the double coefficients on the device, the horizontal pass into an intermediate of the items' dtype that holds only
    the rows the vertical pass reads, and a vertical pass that writes every element of the output.  Nothing is read back; the table
    caches are neither read nor written.  Not built: more than one channel, alpha, reducing_gap, out_dtype / mean / std, patches."""
    name = "resize_many_maps"
    for opt in not_built:
        if opt not in _MAPS_NOT_BUILT:
            raise TypeError(f"{name}() got an unexpected keyword argument '{opt}'")
        raise NotImplementedError(f"{name}(): {opt} is not built for maps ({_MAPS_NOT_BUILT[opt]})")
    if mode not in _lib.FILTER_IDS:
        raise ValueError(mode)
    if overflow not in _lib.MAPS_OVERFLOW:
        raise ValueError(f"{name}(): overflow must be 'pillow' or 'clamp', got {overflow!r}")
    oh, ow, items, dev0, n, c = _many_canvas(name, maps, output_size, channels, "[0, 1, oh, ow]")
    checked = _many_check_items(name, items, c, boxes, lambda i: (oh, ow), tuple(_MAPS_MODES))
    dtype = items[0].dtype if n else (maps.dtype if isinstance(maps, torch.Tensor) and maps.dtype in _MAPS_MODES else torch.float32)
    if c != 1:  # (an empty batch that names its C)
        raise NotImplementedError(f"{name}(): {dtype} maps have one channel (Pillow's \"I;16\", \"I\" and \"F\"), got C = {c}")
    flips = _many_flips(name, flips, n)
    places = _many_places(name, sizes, offsets, n, oh, ow)
    _, elem, fill_range = _MAPS_MODES[dtype]
    if fill_range is not None:
        fill = _many_fill(name, fill, 1, *fill_range, note=f" ({dtype})")[0]
    else:
        try:
            if isinstance(fill, bool):
                raise TypeError
            fill = float(fill)
        except (TypeError, ValueError):
            raise ValueError(f"{name}(): fill must be one finite float for {dtype}, got {fill!r}") from None
        try:
            finite = math.isfinite(fill) and math.isfinite(boxmath.f32(fill))
        except OverflowError:  # (beyond float32)
            finite = False
        if not finite:
            raise ValueError(f"{name}(): fill = {fill} is not finite as {dtype}")
    if n == 0:
        return torch.empty((0, 1, oh, ow), dtype=dtype, device=_many_empty_device(dev0))
    for t in items:
        _require_gpu(t, name)
    dev = items[0].device
    classes = [_many_class(t) for t in items]
    L = _lib.load()
    recs, keep = _many_records(items, classes, False, 1, checked, flips, eb=items[0].element_size())  # (the library takes strides in bytes)
    precs = _many_pack_places(places)
    filter_id, over = _lib.FILTER_IDS[mode], _lib.MAPS_OVERFLOW[overflow]
    return _many_run(
        name, dev, L.aa_many_desc_bytes_maps(n),
        lambda desc, nbytes, ws_bytes: L.aa_many_plan_maps(filter_id, elem, n, oh, ow, recs, precs, float(fill), over, desc, nbytes, ws_bytes),
        lambda: torch.empty((n, 1, oh, ow), dtype=dtype, device=dev),
        lambda desc_host, desc_dev, out, ws, stream: L.aa_resample_many_maps(desc_host, desc_dev, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                                             stream))[0]


def _ycbcr_plane(name: str, i: int, what: str, t, dims: int):
    """One plane of item i, checked -> a uint8 tensor of `dims` dimensions ([H, W], or [h, w, 2] for interleaved chroma)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}(): images[{i}] {what} must be Tensor")
    if t.dtype != torch.uint8:
        raise TypeError(f"{name}(): images[{i}] {what} is {t.dtype}; the planes of a decoder are torch.uint8")
    if dims == 2 and t.dim() == 3 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != dims or (dims == 3 and t.shape[2] != 2):
        shape = "[H, W] or [1, H, W]" if dims == 2 else "[h, w, 2]"
        raise ValueError(f"{name}(): images[{i}] {what} must be {shape}, got {list(t.shape)}")
    if min(t.shape) <= 0:
        raise ValueError(f"{name}(): images[{i}] {what} is empty: {list(t.shape)}")
    return t


def _ycbcr_in_place(t: torch.Tensor, px: int) -> torch.Tensor:
    """A plane as the library reads it: unit pixel stride (px elements per pixel: 2 for interleaved pairs), any row pitch, any offset;
    anything else is copied."""
    ok = t.stride(0) >= 0 and (t.shape[1] == 1 or t.stride(1) == px) and (px == 1 or t.stride(2) == 1)
    return t if ok else t.contiguous()


def resize_many_ycbcr(images, output_size: Sequence[int], mode: str = "bilinear", *, subsampling="420", boxes=None, flips=None, sizes=None,
                      offsets=None, fill=None, out_dtype=None, out_format: str = "nchw", mean=None, std=None) -> torch.Tensor:
    """What a JPEG or video decoder next to the GPU produces — a luma plane and subsampled chroma planes — taken straight to the RGB batch
    a model reads, without expanding the chroma, a colour-conversion pass or an RGB image in between.  Per item i, bit for bit,

        b  = boxes[i] or (0, 0, W, H)                                   # float32 values, luma coordinates
        cb = boxmath.chroma_box(boxes[i], (H, W), subsampling)          # b over (sx, sy), float32
        r  = lambda p, bx: Image.fromarray(p, "L").resize((vw, vh), FILTER, box=bx)
        R_i = Image.merge("YCbCr", [r(Y, b), r(Cb, cb), r(Cr, cb)]).convert("RGB")

    so every plane is resized exactly as Pillow resizes an "L" image, at its own resolution (both 8bpc passes, each rounded to a byte),
    and the three bytes of a pixel then go through Pillow's YCbCr -> RGB conversion.  After that the call is ``resize_many_to_float``:
    ``R_i`` is pasted at ``offsets[i]`` of the [oh, ow] canvas, the rest is ``fill``, the canvas row is mirrored where ``flips[i]``, and a
    float ``out_dtype`` gives ``(float(byte) - mean[c]) / std[c]`` in fp32, rounded once.
    This is NOT what decoding to RGB with the decoder's chroma upsampling and resizing that image gives: the roundings fall elsewhere.

    ``images``: N tuples ``(Y, Cb, Cr)`` or ``(Y, CbCr)`` of uint8 GPU tensors.  ``Y`` is [H, W] (or [1, H, W]); ``Cb`` and ``Cr`` are
    [h, w] each, anywhere, each with its own pitch; ``CbCr`` is one [h, w, 2] tensor of interleaved pairs, Cb first (NV12).  One
    arrangement per call.  Planes are read where they lie: unit pixel stride, any row pitch, any offset; anything else is copied.
    ``subsampling``: "444" | "422" | "420" | "440", one string or one per item; [h, w] must be ``boxmath.chroma_shape(H, W, subsampling)``
    = [ceil(H / sy), ceil(W / sx)] (ValueError otherwise).  Chroma is centred (JFIF siting).
    ``boxes``, ``flips``, ``sizes``, ``offsets``: exactly ``resize_many_to_float``'s, in luma coordinates.
    ``fill``: None (black) or three RGB values, written as given, never converted.
    ``out_dtype``: None / torch.uint8 (Pillow's RGB bytes) | torch.float32 | torch.float16 | torch.bfloat16; ``mean`` / ``std`` (three
    values each, 0..255 units, given together) with a float ``out_dtype`` only.
    ``out_format``: "nchw" (contiguous [N, 3, oh, ow]) | "nhwc" (the same shape, channels_last).  N == 0 gives the empty tensor.

    Three launches whatever N when the chroma is planar (one table kernel and one horizontal pass over all 3 N planes, one converting
    vertical pass), five when it is interleaved (luma and chroma pairs each have the first two), one non-blocking copy of a packed
    descriptor, nothing read back, no table cache touched.  Not built: video-range or BT.709 matrices, left-sited chroma, NV21, alpha,
    patches, reducing_gap."""
    name = "resize_many_ycbcr"
    if mode not in _lib.FILTER_IDS:
        raise ValueError(mode)
    if out_dtype not in (None, torch.uint8, torch.float32, torch.float16, torch.bfloat16):
        raise NotImplementedError(f"{name}(): out_dtype {out_dtype} is not built; None / torch.uint8, torch.float32, torch.float16 or torch.bfloat16")
    if out_format not in ("nchw", "nhwc"):
        raise ValueError("out_format must be 'nchw' or 'nhwc'")
    if (mean is None) != (std is None):
        raise ValueError("mean and std must be given together")
    as_bytes = out_dtype in (None, torch.uint8)
    if as_bytes and mean is not None:
        raise ValueError(f"{name}(): mean / std need a float out_dtype")
    oh, ow = _many_output_size(name, output_size)
    images = list(images)
    n = len(images)
    subs = [subsampling] * n if isinstance(subsampling, str) else list(subsampling)
    if len(subs) != n:
        raise ValueError(f"{name}(): subsampling must be one string or one per image ({n}), got {len(subs)}")
    if boxes is not None and len(boxes) != n:
        raise ValueError(f"{name}(): boxes must hold one entry per image ({n}), got {len(boxes)}")
    planes, arrangement = [], None
    for i, item in enumerate(images):
        if not isinstance(item, (tuple, list)) or len(item) not in (2, 3):
            raise TypeError(f"{name}(): images[{i}] must be a (Y, Cb, Cr) or (Y, CbCr) tuple of tensors")
        boxmath.check_subsampling(subs[i])
        y = _ycbcr_plane(name, i, "Y", item[0], 2)
        if len(item) == 3:
            chroma = [_ycbcr_plane(name, i, "Cb", item[1], 2), _ycbcr_plane(name, i, "Cr", item[2], 2)]
        else:
            chroma = [_ycbcr_plane(name, i, "CbCr", item[1], 3)]
        if arrangement is None:
            arrangement = len(item)
        elif arrangement != len(item):
            raise ValueError(f"{name}(): one chroma arrangement per call: images[{i}] has {len(item) - 1} chroma tensor(s), images[0] "
                             f"{arrangement - 1} (planar (Y, Cb, Cr) or interleaved (Y, CbCr))")
        h, w = int(y.shape[0]), int(y.shape[1])
        want = boxmath.chroma_shape(h, w, subs[i])
        for t in chroma:
            if tuple(t.shape[:2]) != want:
                raise ValueError(f"{name}(): images[{i}] is [{h}, {w}] with subsampling {subs[i]!r}: its chroma must be {list(want)}, got "
                                 f"{list(t.shape[:2])}")
            if t.device != y.device:
                raise ValueError(f"{name}(): images[{i}]: every plane must be on the same device")
        if planes and y.device != planes[0][0].device:
            raise ValueError(f"{name}(): every image must be on the same device: images[{i}] is on {y.device}, images[0] on {planes[0][0].device}")
        planes.append((y, chroma))
    checked = [_many_box(boxes[i] if boxes is not None else None, int(y.shape[1]), int(y.shape[0])) for i, (y, _) in enumerate(planes)]
    cv, res_dtype = None, torch.uint8
    if as_bytes:
        flips = _many_flips(name, flips, n)
    else:
        cv, flips, res_dtype = _many_convert(name, {"out_dtype": out_dtype, "mean": mean, "std": std, "flips": flips}, n, 3)
    fills = _many_fill(name, 0 if fill is None else fill, 3)
    places = _many_places(name, sizes, offsets, n, oh, ow)
    if n == 0:
        return torch.empty((0, 3, oh, ow), dtype=res_dtype, device=_many_empty_device(None))
    for y, chroma in planes:
        for t in [y] + chroma:
            _require_gpu(t, name)
    dev = planes[0][0].device
    nhwc = out_format == "nhwc"
    if cv is not None:
        cv.out_layout = _lib.NHWC if nhwc else _lib.NCHW
    L = _lib.load()
    recs, keep = (_lib.YccImage * n)(), []
    for i, (y, chroma) in enumerate(planes):
        y = _ycbcr_in_place(y, 1)
        chroma = [_ycbcr_in_place(t, 1 if arrangement == 3 else 2) for t in chroma]
        keep += [y] + chroma  # (copies must outlive the launches; the stream orders their release after them)
        r = recs[i]
        r.y_dev, r.cb_dev = y.data_ptr(), chroma[0].data_ptr()
        r.cr_dev = chroma[1].data_ptr() if arrangement == 3 else chroma[0].data_ptr() + 1
        r.H, r.W = int(y.shape[0]), int(y.shape[1])
        r.cH, r.cW = int(chroma[0].shape[0]), int(chroma[0].shape[1])
        # (the pitch of a plane of one row is arbitrary)
        r.y_stride_row = y.stride(0) if r.H > 1 else 0
        r.cb_stride_row = chroma[0].stride(0) if r.cH > 1 else 0
        r.cr_stride_row = chroma[-1].stride(0) if r.cH > 1 else 0
        r.chroma_stride_px = 1 if arrangement == 3 else 2
        r.subsampling = _lib.YCC_SUBSAMPLING[subs[i]]
        if checked[i] is not None:
            r.has_box = 1
            r.box[:] = checked[i]
        if flips is not None and flips[i]:
            r.flags = _lib.MANY_FLIP_X
    precs = _many_pack_places(places)
    cfill = (ctypes.c_uint8 * 3)(*fills)
    layout = _lib.NHWC if nhwc else _lib.NCHW
    mf = torch.channels_last if nhwc else torch.contiguous_format
    return _many_run(
        name, dev, L.aa_many_desc_bytes_ycbcr(n),
        lambda desc, nbytes, ws_bytes: L.aa_many_plan_ycbcr(_lib.FILTER_IDS[mode], n, oh, ow, recs, precs, cfill, desc, nbytes, ws_bytes),
        lambda: torch.empty((n, 3, oh, ow), dtype=res_dtype, device=dev, memory_format=mf),
        lambda desc_host, desc_dev, out, ws, stream: L.aa_resample_many_ycbcr(desc_host, desc_dev, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                                              ctypes.byref(cv) if cv is not None else None, layout, stream))[0]


def _patch_sizes(name: str, sizes, patch, n: int, pad_to):
    """patch, sizes and pad_to of resize_many_to_patches, checked -> ((ph, pw), [(vh, vw)] per item, L or None)."""
    try:
        ph, pw = boxmath.check_patch(patch)
    except ValueError as e:
        raise ValueError(f"{name}(): {e}") from None
    if ph > _MANY_MAX or pw > _MANY_MAX:
        raise ValueError(f"{name}(): patch = ({ph}, {pw}) is beyond the supported {_MANY_MAX}")
    if sizes is None:
        raise ValueError(f"{name}(): sizes is required: N entries (vh, vw), or one pair for all items")
    try:
        one = len(sizes) == 2 and not isinstance(sizes[0], (tuple, list)) and int(sizes[0]) == sizes[0]
    except (TypeError, ValueError):
        one = False
    if one:
        sizes = [tuple(sizes)] * n
    if len(sizes) != n:
        raise ValueError(f"{name}(): sizes must hold one entry per image ({n}), got {len(sizes)}")
    out = []
    for i in range(n):
        vh, vw = _many_int_pair(name, "sizes", i, sizes[i])
        if vh <= 0 or vw <= 0:
            raise ValueError(f"{name}(): sizes[{i}] = ({vh}, {vw}) must be positive")
        if vh > _MANY_MAX or vw > _MANY_MAX:
            raise ValueError(f"{name}(): sizes[{i}] = ({vh}, {vw}) is beyond the supported {_MANY_MAX}")
        out.append((vh, vw))
    try:
        grids = boxmath.patch_grids(out, (ph, pw))  # (the divisibility check, naming the item)
    except ValueError as e:
        raise ValueError(f"{name}(): {e}") from None
    if pad_to is not None:
        if isinstance(pad_to, bool) or int(pad_to) != pad_to or pad_to < 1 or pad_to > 2 ** 31 - 1:
            raise ValueError(f"{name}(): pad_to must be None or a positive integer, got {pad_to!r}")
        pad_to = int(pad_to)
        for i, (gh, gw) in enumerate(grids):
            if gh * gw > pad_to:
                raise ValueError(f"{name}(): sizes[{i}] = {out[i]} is {gh * gw} tokens, more than pad_to = {pad_to}")
    return (ph, pw), out, pad_to


def resize_many_to_patches(images, patch: Sequence[int], mode: str = "bicubic", *, sizes=None, boxes=None, flips=None,
                           channels: Optional[int] = None, patch_format: str = "cpp", pad_to: Optional[int] = None, out_dtype=torch.float32,
                           mean=None, std=None) -> torch.Tensor:
    """The ragged batch as the packed patch tokens a native-resolution vision transformer reads (NaViT, NaFlex, VLM towers): item i is
    resized to ITS OWN size ``sizes[i] = (vh_i, vw_i)``, a multiple of ``patch = (ph, pw)``, converted like ``resize_many_to_float`` and
    cut into ``ph x pw`` patches, all in the same three launches.  With ``gh = vh // ph``, ``gw = vw // pw``, ``T = gh * gw``, ``D = C * ph * pw``
    and

        R_i = resize_many_to_float([images[i]], (vh_i, vw_i), mode, boxes=[boxes[i]], flips=[flips[i]], out_dtype=out_dtype,
                                   out_format="nchw", mean=mean, std=std)[0]
        P_i = R_i.view(C, gh, ph, gw, pw)
        P_i = P_i.permute(1, 3, 0, 2, 4).reshape(T, D)    patch_format="cpp": a token is [C, ph, pw], a Conv2d(C, dim, patch, stride=patch) weight flattened
        P_i = P_i.permute(1, 3, 2, 4, 0).reshape(T, D)    patch_format="ppc": a token is [ph, pw, C], einops '(p1 p2 c)'

    the result is, bit for bit, ``torch.cat(P_0 .. P_{N-1})``, [sum T_i, D], item i at rows ``boxmath.token_offsets(sizes, patch)[i]`` on
    (``pad_to=None``); or [N, L, D] with ``tok[i, :T_i] = P_i`` and literal zeros (+0.0, not normalised) beyond (``pad_to=L``; an item of
    more than L tokens raises ValueError).  A flip mirrors the item's own resized image before it is cut.

    ``images``, ``mode``, ``boxes``, ``flips``, ``channels``, ``out_dtype``, ``mean``, ``std``: ``resize_many_to_float``'s.  ``sizes``: N entries
    (vh, vw), height first, or one pair for all items; ``boxmath.fit_patch_sizes`` makes them from the images' shapes.  There is no canvas:
    no ``output_size``, ``offsets`` or ``fill``.  N == 0 gives [0, D] or [0, L, D]; a list then says its C with ``channels=``.

    One contiguous tensor from three launches and one non-blocking descriptor copy whatever N and whatever the sizes; nothing is read
    back, no table cache is touched, the call does not synchronise."""
    name = "resize_many_to_patches"
    if out_dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise NotImplementedError(f"{name}(): out_dtype {out_dtype} is not built; torch.float32, torch.float16 or torch.bfloat16")
    if patch_format not in ("cpp", "ppc"):
        raise ValueError("patch_format must be 'cpp' (token = [C, ph, pw]) or 'ppc' (token = [ph, pw, C])")
    if (mean is None) != (std is None):
        raise ValueError("mean and std must be given together")
    if _uint8_mode != "pil":
        raise NotImplementedError(f"{name}(): uint8_mode='harness' is not built for a list of images (Pillow's arithmetic only)")
    if mode not in _lib.FILTER_IDS:
        raise ValueError(mode)
    filter_id = _lib.FILTER_IDS[mode]
    items, dev0, n, c = _many_items(name, images, channels, "[0, C * ph * pw]")
    (ph, pw), sizes, pad_to = _patch_sizes(name, sizes, patch, n, pad_to)
    checked = _many_check_items(name, items, c, boxes, lambda i: sizes[i])
    cv, flips, out_dtype = _many_convert(name, {"out_dtype": out_dtype, "mean": mean, "std": std, "flips": flips}, n, c)
    d = c * ph * pw
    rows = boxmath.token_offsets(sizes, (ph, pw))[-1]
    shape = (rows, d) if pad_to is None else (n, pad_to, d)
    if n == 0:
        return torch.empty(shape, dtype=out_dtype, device=_many_empty_device(dev0))
    for t in items:
        _require_gpu(t, name)
    dev = items[0].device
    classes, interleaved = _many_layout(items, c)
    layout = _lib.NHWC if interleaved else _lib.NCHW
    cv.out_layout = _lib.NCHW  # (not looked at: the token layout is patch_format)
    L = _lib.load()
    recs, keep = _many_records(items, classes, interleaved, c, checked, flips)
    flat = (ctypes.c_int64 * (2 * n))(*[v for s in sizes for v in s])
    out_rows = ctypes.c_int64(0)

    def plan(desc, nbytes, ws_bytes):
        rc = L.aa_many_plan_patches(filter_id, layout, n, c, ph, pw, recs, flat, pad_to or 0, desc, nbytes, ws_bytes, ctypes.byref(out_rows))
        assert rc < 0 or out_rows.value == (rows if pad_to is None else n * pad_to), (out_rows.value, rows, pad_to)
        return rc

    fmt = _lib.PATCH_PPC if patch_format == "ppc" else _lib.PATCH_CPP
    return _many_run(
        name, dev, L.aa_many_desc_bytes_patches(n), plan, lambda: torch.empty(shape, dtype=out_dtype, device=dev),
        lambda desc_host, desc_dev, out, ws, stream: L.aa_resample_many_u8_to_patches(desc_host, desc_dev, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                                                      ctypes.byref(cv), fmt, stream))[0]


_EMBED_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _embed_grids(name: str, grids, pad_to):
    """grids and pad_to of the position-grid calls, checked -> ([(gh, gw)], the int64 pairs for the planner, L or None)."""
    try:
        grids = list(grids)
    except TypeError:
        raise ValueError(f"{name}(): grids must be N pairs (gh, gw), got {grids!r}") from None
    out = []
    for i, g in enumerate(grids):
        gh, gw = _many_int_pair(name, "grids", i, g)
        if gh < 1 or gw < 1:
            raise ValueError(f"{name}(): grids[{i}] = ({gh}, {gw}) must be positive")
        if gh > _MANY_MAX or gw > _MANY_MAX or gh * gw > _MANY_MAX:
            raise ValueError(f"{name}(): grids[{i}] = ({gh}, {gw}) is beyond the supported {_MANY_MAX}")
        out.append((gh, gw))
    if pad_to is not None:
        if isinstance(pad_to, bool) or int(pad_to) != pad_to or pad_to < 1 or pad_to > 2 ** 31 - 1:
            raise ValueError(f"{name}(): pad_to must be None or a positive integer, got {pad_to!r}")
        pad_to = int(pad_to)
        for i, (gh, gw) in enumerate(out):
            if gh * gw > pad_to:
                raise ValueError(f"{name}(): grids[{i}] = ({gh}, {gw}) is {gh * gw} tokens, more than pad_to = {pad_to}")
    return out, (ctypes.c_int64 * max(2 * len(out), 1))(*[v for g in out for v in g]), pad_to


def _embed_run(name: str, mode: str, dev, d: int, h0: int, w0: int, grids, flat, pad_to, alloc_out, launch):
    """The plan of the position-grid calls and _many_run: ``launch(L, desc_host, desc_dev, out, ws, stream)``."""
    L = _lib.load()
    n = len(grids)
    out_rows = ctypes.c_int64(0)
    rows = boxmath.token_offsets(grids, (1, 1))[-1] if pad_to is None else n * pad_to

    def plan(desc, nbytes, ws_bytes):
        rc = L.aa_embed_many_plan(_lib.FILTER_IDS[mode], n, d, h0, w0, flat, pad_to or 0, desc, nbytes, ws_bytes, ctypes.byref(out_rows))
        assert rc < 0 or out_rows.value == rows, (out_rows.value, rows, pad_to)
        return rc

    return _many_run(name, dev, L.aa_embed_many_desc_bytes(n), plan, alloc_out,
                     lambda desc_host, desc_dev, out, ws, stream: launch(L, desc_host, desc_dev, out, ws, stream))[0]


def _resize_embed_forward(embed: torch.Tensor, grids, flat, pad_to, mode: str, out_dtype) -> torch.Tensor:
    name = "resize_embed_to_tokens"
    h0, w0, d = embed.shape
    n = len(grids)
    rows = boxmath.token_offsets(grids, (1, 1))[-1]
    shape = (rows, d) if pad_to is None else (n, pad_to, d)
    if n == 0:
        return torch.empty(shape, dtype=out_dtype, device=embed.device)
    return _embed_run(name, mode, embed.device, d, h0, w0, grids, flat, pad_to, lambda: torch.empty(shape, dtype=out_dtype, device=embed.device),
                      lambda L, desc_host, desc_dev, out, ws, stream: L.aa_resample_embed_many(
                          desc_host, desc_dev, embed.data_ptr(), _DTYPE_IDS[embed.dtype], embed.stride(0), embed.stride(1), out.data_ptr(),
                          _DTYPE_IDS[out_dtype], ws.data_ptr(), ws.numel(), stream))


class _ResizeEmbedToTokens(torch.autograd.Function):
    """resize_embed_to_tokens for an embedding that requires grad: the backward plans again from the saved grids."""

    @staticmethod
    def forward(ctx, embed, grids, flat, pad_to, mode, out_dtype):
        ctx.embed_size, ctx.embed_dtype = tuple(embed.shape), embed.dtype
        ctx.grids, ctx.pad_to, ctx.mode = grids, pad_to, mode
        return _resize_embed_forward(embed, grids, flat, pad_to, mode, out_dtype)

    @staticmethod
    def backward(ctx, grad_tokens):
        ge = resize_embed_to_tokens_backward(grad_tokens, ctx.embed_size, ctx.grids, ctx.mode, pad_to=ctx.pad_to, dtype=ctx.embed_dtype)
        return ge, None, None, None, None, None


def resize_embed_to_tokens(embed: torch.Tensor, grids, mode: str = "bicubic", *, pad_to: Optional[int] = None, out_dtype=None) -> torch.Tensor:
    """A learned position grid resampled to every item's own token grid and packed in ``resize_many_to_patches``'s row order: what a
    native-resolution vision transformer (NaViT, NaFlex, VLM towers) adds to those tokens.  ``embed`` is [H0, W0, D], float32, float16 or
    bfloat16 on the GPU, read where it lies: ``stride(2) == 1``, any row and pixel stride, any element-aligned address — a view such as
    ``pos_embed[0, 1:].view(H0, W0, D)``, which skips a class token, is not copied.  ``grids``: N pairs (gh_i, gw_i), height first, each
    at least 1 — what ``boxmath.patch_grids(sizes, patch)`` returns.  With ``F`` the ``<mode>_forward`` of this module, item i is, bit
    for bit,

        F(embed.float().permute(2, 0, 1)[None], [gh_i, gw_i])[0].permute(1, 2, 0).reshape(gh_i * gw_i, D).to(out_dtype)

    the reference's fp32 arithmetic (the horizontal pass first, an fp32 intermediate, product and sum rounded apart, antialiased where an
    axis shrinks) with ONE rounding to nearest even at the store, and the result is the ``torch.cat`` of the items, [sum T_i, D], item i at
    rows ``boxmath.token_offsets(grids, (1, 1))[i]`` on; or [N, L, D] with literal zeros (+0.0) beyond T_i (``pad_to=L``; an item of more
    than L tokens raises ValueError).  ``mode``: any of the five filters' names; ``align_corners`` is always False.  ``out_dtype``: None
    (``embed.dtype``), float32, float16 or bfloat16.  N == 0 gives [0, D] or [0, L, D].

    Differentiable: when ``embed`` requires grad the result carries a backward, ``resize_embed_to_tokens_backward`` with
    ``dtype=embed.dtype``.  Two launches and one non-blocking descriptor copy whatever N and whatever the grids; nothing is read back, no
    table cache is touched, the call does not synchronise."""
    name = "resize_embed_to_tokens"
    if not isinstance(embed, torch.Tensor) or embed.dim() != 3:
        raise ValueError(f"{name}(): embed must be a tensor [H0, W0, D]")
    if embed.dtype not in _EMBED_DTYPES:
        raise NotImplementedError(f"{name}(): embed of {embed.dtype} is not built; torch.float32, torch.float16 or torch.bfloat16")
    out_dtype = embed.dtype if out_dtype is None else out_dtype
    if out_dtype not in _EMBED_DTYPES:
        raise NotImplementedError(f"{name}(): out_dtype {out_dtype} is not built; torch.float32, torch.float16 or torch.bfloat16")
    if mode not in _lib.FILTER_IDS:
        raise ValueError(mode)
    h0, w0, d = embed.shape
    if h0 < 1 or w0 < 1 or d < 1 or max(h0, w0, d) > _MANY_MAX:
        raise ValueError(f"{name}(): embed of shape {tuple(embed.shape)}: every size must be in 1 .. {_MANY_MAX}")
    if d > 1 and embed.stride(2) != 1:
        raise ValueError(f"{name}(): embed must have stride(2) == 1 (channels last), got strides {embed.stride()}")
    grids, flat, pad_to = _embed_grids(name, grids, pad_to)
    _require_gpu(embed, name)
    if embed.requires_grad and torch.is_grad_enabled():
        return _ResizeEmbedToTokens.apply(embed, grids, flat, pad_to, mode, out_dtype)
    return _resize_embed_forward(embed.detach(), grids, flat, pad_to, mode, out_dtype)


def resize_embed_to_tokens_backward(grad_tokens: torch.Tensor, embed_size: Sequence[int], grids, mode: str = "bicubic", *,
                                    pad_to: Optional[int] = None, dtype=torch.float32) -> torch.Tensor:
    """The backward of ``resize_embed_to_tokens``: the gradient of the [H0, W0, D] position grid from the tokens' gradient,
    [sum T_i, D] or [N, L, D] (``pad_to=L``; rows beyond T_i are not read), float32, float16 or bfloat16.  With ``b_i`` the existing
    gather-form backward of item i's rows in fp32, ``<mode>_backward(G_i.float() as [1, D, gh_i, gw_i], [gh_i, gw_i], [1, D, H0, W0])``,
    the result is, bit for bit, ``acc = b_0``, then ``acc = acc + b_i`` in fp32 for i = 1 .. N - 1 in ascending order, then
    ``acc.to(dtype)`` as [H0, W0, D], contiguous.  No atomics: deterministic, whatever the launch shape.  N == 0 gives zeros.
    Two launches whatever N; nothing is read back, the call does not synchronise."""
    name = "resize_embed_to_tokens_backward"
    if not isinstance(grad_tokens, torch.Tensor):
        raise ValueError(f"{name}(): grad_tokens must be a tensor")
    if grad_tokens.dtype not in _EMBED_DTYPES:
        raise NotImplementedError(f"{name}(): grad_tokens of {grad_tokens.dtype} is not built; torch.float32, torch.float16 or torch.bfloat16")
    if dtype not in _EMBED_DTYPES:
        raise NotImplementedError(f"{name}(): dtype {dtype} is not built; torch.float32, torch.float16 or torch.bfloat16")
    if mode not in _lib.FILTER_IDS:
        raise ValueError(mode)
    try:
        h0, w0, d = (int(v) for v in embed_size)
    except (TypeError, ValueError):
        raise ValueError(f"{name}(): embed_size must be (H0, W0, D), got {embed_size!r}") from None
    if h0 < 1 or w0 < 1 or d < 1 or max(h0, w0, d) > _MANY_MAX:
        raise ValueError(f"{name}(): embed_size = ({h0}, {w0}, {d}): every size must be in 1 .. {_MANY_MAX}")
    grids, flat, pad_to = _embed_grids(name, grids, pad_to)
    n = len(grids)
    rows = boxmath.token_offsets(grids, (1, 1))[-1]
    shape = (rows, d) if pad_to is None else (n, pad_to, d)
    if tuple(grad_tokens.shape) != shape:
        raise ValueError(f"{name}(): grad_tokens of shape {tuple(grad_tokens.shape)}, expected {shape}")
    _require_gpu(grad_tokens, name)
    dev = grad_tokens.device
    if n == 0:
        return torch.zeros((h0, w0, d), dtype=dtype, device=dev)
    g = grad_tokens.detach().contiguous()
    return _embed_run(name, mode, dev, d, h0, w0, grids, flat, pad_to, lambda: torch.empty((h0, w0, d), dtype=dtype, device=dev),
                      lambda L, desc_host, desc_dev, out, ws, stream: L.aa_resample_embed_many_bwd(
                          desc_host, desc_dev, g.data_ptr(), _DTYPE_IDS[g.dtype], out.data_ptr(), _DTYPE_IDS[dtype], ws.data_ptr(), ws.numel(),
                          stream))


_BACK_MAX_ELEMS = 2 ** 40  # the library's bound on K * oh_i * ow_i (csrc/aa_many_back.h AA_BACK_MAX_ELEMS)
# reduce -> (the planner's id, the default out_dtype, {out_dtype: (aa_dtype, the most classes it holds or None)})
_BACK_REDUCE = {
    None: (_lib.BACK_VALUES, None, {torch.float32: (_lib.F32, None), torch.float16: (_lib.F16, None), torch.bfloat16: (_lib.BF16, None)}),
    "argmax": (_lib.BACK_ARGMAX, torch.int64, {torch.int64: (_lib.I64, None), torch.int32: (_lib.I32, None), torch.int16: (_lib.I16, 32768),
                                               torch.uint8: (_lib.U8, 256)}),
    "greater": (_lib.BACK_GREATER, torch.bool, {torch.bool: (_lib.BOOL, None), torch.uint8: (_lib.U8, None)}),
}


def _back_items(name: str, pred, channels: Optional[int]):
    """pred of resize_many_back -> ([K, H_i, W_i] items, the device of a batch tensor or None, N, K), dtype, K, sizes and devices checked."""
    if isinstance(pred, torch.Tensor):
        if pred.dim() != 4:
            raise ValueError(f"{name}(): one tensor must be [N, K, H, W], got {list(pred.shape)}")
        if channels is None:
            channels = int(pred.shape[1])
        items, dev0 = list(pred.unbind(0)), pred.device
    else:
        items, dev0 = [], None
        for i, t in enumerate(pred):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{name}(): pred[{i}] must be Tensor")
            if t.dim() == 4 and t.shape[0] == 1:
                t = t[0]
            if t.dim() != 3:
                raise ValueError(f"{name}(): pred[{i}] must be [K, H, W] or [1, K, H, W], got {list(t.shape)}")
            items.append(t)
    n = len(items)
    if n == 0 and channels is None:
        raise ValueError(f"{name}(): an empty list needs channels= (the K of the items)")
    k = int(channels) if channels is not None else int(items[0].shape[0])
    if not (1 <= k <= _MANY_MAX):
        raise ValueError(f"{name}(): K must be in 1 .. {_MANY_MAX}, got K = {k}")
    for i, t in enumerate(items):
        if t.dtype not in _EMBED_DTYPES:
            raise NotImplementedError(f"{name}(): pred[{i}] of {t.dtype} is not built; torch.float32, torch.float16 or torch.bfloat16")
        if t.dtype != items[0].dtype:
            raise ValueError(f"{name}(): every item must have the same dtype: pred[{i}] is {t.dtype}, pred[0] {items[0].dtype}")
        if int(t.shape[0]) != k:
            raise ValueError(f"{name}(): every item must have the same K: pred[{i}] has {int(t.shape[0])}, expected {k}")
        if not (int(t.shape[1]) > 0 and int(t.shape[2]) > 0):
            raise ValueError(f"{name}(): pred[{i}] is empty: {list(t.shape)}")
        if t.device != items[0].device:
            raise ValueError(f"{name}(): every item must be on the same device: pred[{i}] is on {t.device}, pred[0] on {items[0].device}")
    return items, dev0, n, k


def _back_sizes(name: str, sizes, n: int, k: int):
    try:
        sizes = list(sizes)
    except TypeError:
        raise ValueError(f"{name}(): sizes must be N pairs (oh, ow), got {sizes!r}") from None
    if len(sizes) != n:
        raise ValueError(f"{name}(): sizes must hold one entry per item ({n}), got {len(sizes)}")
    out = []
    for i, s in enumerate(sizes):
        oh, ow = _many_int_pair(name, "sizes", i, s)
        if oh < 1 or ow < 1:
            raise ValueError(f"{name}(): sizes[{i}] = ({oh}, {ow}) must be positive")
        if oh > _MANY_MAX or ow > _MANY_MAX or oh * ow * k > _BACK_MAX_ELEMS:
            raise ValueError(f"{name}(): sizes[{i}] = ({oh}, {ow}) with K = {k} is beyond the supported {_MANY_MAX} a side and "
                             f"{_BACK_MAX_ELEMS} elements")
        out.append((oh, ow))
    return out


def _back_regions(name: str, regions, items):
    """regions of resize_many_back, checked -> [(y0, x0, h, w)], the whole item for None."""
    n = len(items)
    if regions is not None and len(regions) != n:
        raise ValueError(f"{name}(): regions must hold one entry per item ({n}), got {len(regions)}")
    out = []
    for i, t in enumerate(items):
        hh, ww = int(t.shape[1]), int(t.shape[2])
        r = regions[i] if regions is not None else None
        if r is None:
            out.append((0, 0, hh, ww))
            continue
        try:
            y0, x0, h, w = r
            if any(isinstance(v, bool) or int(v) != v for v in (y0, x0, h, w)):
                raise TypeError
        except (TypeError, ValueError):
            raise ValueError(f"{name}(): regions[{i}] must be None or four integers (y0, x0, h, w), got {r!r}") from None
        y0, x0, h, w = int(y0), int(x0), int(h), int(w)
        if h < 1 or w < 1:
            raise ValueError(f"{name}(): regions[{i}] = ({y0}, {x0}, {h}, {w}) is empty")
        if y0 < 0 or x0 < 0 or y0 + h > hh or x0 + w > ww:
            raise ValueError(f"{name}(): regions[{i}] = ({y0}, {x0}, {h}, {w}) does not lie inside its item of size ({hh}, {ww})")
        out.append((y0, x0, h, w))
    return out


def _back_out(name: str, reduce, out_dtype, threshold, items, k: int):
    """out_dtype and threshold of resize_many_back and its kin, checked for ``reduce`` (a key of _BACK_REDUCE) ->
    (the planner's reduce id, out_dtype, its aa_dtype, threshold as a float)."""
    reduce_id, default_dtype, out_dtypes = _BACK_REDUCE[reduce]
    if out_dtype is None:
        out_dtype = default_dtype if default_dtype is not None else (items[0].dtype if items else torch.float32)
    if out_dtype not in out_dtypes:
        raise NotImplementedError(f"{name}(): out_dtype {out_dtype} is not built for reduce={reduce!r}; {', '.join(str(d) for d in out_dtypes)}")
    out_id, most = out_dtypes[out_dtype]
    if most is not None and k > most:
        raise ValueError(f"{name}(): out_dtype {out_dtype} holds labels below {most}, got K = {k}")
    try:
        threshold = float(threshold)
    except (TypeError, ValueError):
        raise ValueError(f"{name}(): threshold must be a finite float, got {threshold!r}") from None
    if not math.isfinite(threshold) or not math.isfinite(ctypes.c_float(threshold).value):
        raise ValueError(f"{name}(): threshold must be a finite float (as float32), got {threshold!r}")
    return reduce_id, out_dtype, out_id, threshold


def _back_activation_name(name: str, activation):
    """activation of resize_many_back and its kin: None, "softmax" or "sigmoid"."""
    if not (activation is None or isinstance(activation, str)) or activation not in _lib.BACK_ACT:
        raise ValueError(f"{name}(): activation must be None, 'softmax' or 'sigmoid', got {activation!r}")


def _back_activation(name: str, activation, reduce, pred, items) -> int:
    """-> the planner's id of a checked activation name.  The activations have no backward: values that would carry a grad_fn are refused
    rather than handed out detached."""
    if activation is not None and reduce is None and torch.is_grad_enabled():
        if pred.requires_grad if isinstance(pred, torch.Tensor) else any(t.requires_grad for t in items):
            raise NotImplementedError(f"{name}(): activation={activation!r} is not differentiable: with reduce=None and a pred that requires "
                                      f"grad, call it under torch.no_grad() or pass pred.detach()")
    return _lib.BACK_ACT[activation]


def resize_many_back(pred, sizes, mode: str = "bilinear", *, regions=None, flips=None, reduce: Optional[str] = None, threshold: float = 0.0,
                     out_dtype=None, channels: Optional[int] = None, activation: Optional[str] = None):
    """A model's answer on the canvas, back at every image's own size: the return path of ``resize_many`` and its kin, for segmentation,
    depth and mask heads.  ``pred``: one float32 / float16 / bfloat16 GPU tensor [N, K, H, W], or a sequence of N tensors [K, H_i, W_i]
    (or [1, K, H_i, W_i]); the same K (1 .. 2^29 - 1), dtype and device for all.  Items are read where they lie, in one of two classes:
    planes (``stride(2) == 1``, any plane and row stride) or interleaved classes (``stride(0) == 1``, ``stride(2) == K``: a channels_last
    batch).  One class per call, the majority's; an item in neither, or in the other, is copied into it first.
    ``regions``: None, or N entries, each None (the whole item) or integers (y0, x0, h, w) — HEIGHT FIRST, like ``output_size`` — the
    rectangle of the item that image i occupied; exactly the view ``pred_i[:, y0:y0 + h, x0:x0 + w]``, and nothing outside it is read.
    ``boxmath.placed_regions(sizes, offsets, output_size)`` gives the rectangles ``resize_many(..., sizes=, offsets=)`` placed the images
    at.  ``sizes``: N pairs (oh_i, ow_i), the images' own sizes.  ``flips``: None or N booleans; a flipped item's column x holds column
    ``ow_i - 1 - x`` of the unflipped result (the undo of a flipped test-time pass).  ``mode``: any of the five filters' names;
    ``align_corners`` is always False.

    With ``F`` the ``<mode>_forward`` of this module and ``R_i = F(view_i.float()[None], [oh_i, ow_i])[0]`` — the reference's fp32
    arithmetic: the horizontal pass first, an fp32 intermediate, product and sum rounded apart, antialiased where an axis shrinks — the
    result is a list of N tensors, bit for bit:

      * ``reduce=None``: ``R_i.to(out_dtype)`` [K, oh_i, ow_i], ONE rounding to nearest even; ``out_dtype`` None (``pred``'s), float32,
        float16 or bfloat16;
      * ``reduce="argmax"``: [oh_i, ow_i], the lowest k at which ``R_i`` is greatest, taken on the fp32 value before any rounding to 16
        bits; a NaN counts as greater than every number and the first NaN wins (``numpy.argmax`` over axis 0).  ``out_dtype`` None
        (int64, what ``torch.argmax`` gives), uint8 (K <= 256), int16 (K <= 32768) or int32.  The K values of a pixel are never stored;
      * ``reduce="greater"``: ``R_i > threshold`` [K, oh_i, ow_i] on the fp32 value; ``threshold`` a finite float, compared as float32; a
        NaN gives False.  ``out_dtype`` None (bool) or uint8.

    The tensors are contiguous views of ONE arena, each starting on a 16-byte boundary of it, as ``reduce_many`` returns its images.
    N == 0 gives [] (a list then states K with ``channels=``).  Two launches whatever N and whatever the sizes — one builds every item's two
    fp32 weight tables, one resamples and reduces — and one non-blocking copy of a packed descriptor; nothing is read back, no table cache
    is touched, the call does not synchronise.

    Differentiable for ``reduce=None``: when gradients are enabled and ``pred`` (or any item of a list) requires grad, the results carry
    a backward, ``resize_many_back_backward`` with ``dtype=pred``'s dtype and the layout class ``pred`` was read in: one gradient for a
    batch tensor, one per list item, +0.0 outside the regions and for items the loss did not use (two launches for the whole list,
    whatever the loss uses).  The values, the arena and the launch count are the same with and without it.  The results are views of
    one arena and outputs of one autograd node: under autograd they must not be modified in place.  ``reduce="argmax"`` and
    ``"greater"`` are not differentiable and never carry a ``grad_fn``.

    ``activation``: None (everything above as it stands), ``"softmax"`` (over the K classes of a pixel) or ``"sigmoid"`` (per element),
    applied in fp32 to ``R_i`` — before any rounding to 16 bits — inside the same two launches; the probabilities ``P_i`` then stand where
    ``R_i`` stood: ``reduce=None`` rounds ``P_i`` once to ``out_dtype``, ``"argmax"`` and ``"greater"`` look at the fp32 ``P_i``.  ``P_i`` is
    defined bit for bit (``tests/activation_ref.py`` restates it in numpy; ``include/aa_interp.h`` spells it out): ``aa_exp``, an fp32
    exponential for arguments <= 0, at most 0.9916 ulp from ``exp`` over all of [-86, 0] and +0 below -86, every product and sum rounded
    on its own; the sigmoid ``(v >= 0 ? 1 : e) / (1 + e)`` with ``e = aa_exp(-|v|)``, one correctly rounded division; the softmax in two
    passes over ascending k — an online maximum ``m`` and denominator ``d``, then ``aa_exp(v_k - m) * (1 / d)`` — so a ``-inf`` (masked)
    class gets +0, and a pixel with a NaN, a ``+inf`` or nothing but ``-inf`` is NaN in every class (which class the argmax then names
    is ``numpy.argmax``'s answer: 0).  A softmax pixel's classes are resampled twice; nothing more is stored than without it.  The
    activation is NOT differentiable: with ``reduce=None``, gradients enabled and a ``pred`` that requires grad the call raises
    ``NotImplementedError`` rather than hand out detached probabilities — call it under ``torch.no_grad()`` or pass ``pred.detach()``.

    Not built: fractional regions, a dense padded output, a backward through the activation, ``log_softmax`` (several passes per image
    summed before the reduction: ``resize_many_back_merged``)."""
    name = "resize_many_back"
    if mode not in _lib.FILTER_IDS:
        raise ValueError(mode)
    if reduce not in _BACK_REDUCE:
        raise ValueError(f"{name}(): reduce must be None, 'argmax' or 'greater', got {reduce!r}")
    _back_activation_name(name, activation)
    items, dev0, n, k = _back_items(name, pred, channels)
    sizes = _back_sizes(name, sizes, n, k)
    rects = _back_regions(name, regions, items)
    flips = _many_flips(name, flips, n)
    reduce_id, out_dtype, out_id, threshold = _back_out(name, reduce, out_dtype, threshold, items, k)
    act_id = _back_activation(name, activation, reduce, pred, items)
    if n == 0:
        return []
    for t in items:
        _require_gpu(t, name)
    plan = (name, mode, n, k, sizes, rects, flips, reduce, reduce_id, out_dtype, out_id, threshold, act_id)
    if reduce is None and torch.is_grad_enabled():
        if isinstance(pred, torch.Tensor):
            if pred.requires_grad:
                return list(_ResizeManyBack.apply(plan, True, pred))
        elif any(t.requires_grad for t in items):
            return list(_ResizeManyBack.apply(plan, False, *items))
    return _resize_many_back_run(plan, [t.detach() for t in items])[0]


def _back_records(items, rects, sizes, flips, k: int):
    """The aa_back_item records of checked GPU items: each one's region, read where it lies in the call's layout class and resampled to
    sizes[i] -> (records, the copies of items outside the class, which must stay alive until the launches are enqueued; whether the
    class is interleaved)."""
    n = len(items)
    views = [t[:, y0:y0 + h, x0:x0 + w] for t, (y0, x0, h, w) in zip(items, rects)]
    classes, interleaved = _many_layout(views, k)
    recs, keep = (_lib.BackItemIn * n)(), []
    for i, t in enumerate(views):
        if not classes[i][0 if interleaved else 1]:
            t = t.permute(1, 2, 0).contiguous().permute(2, 0, 1) if interleaved else t.contiguous()
            keep.append(t)
        r = recs[i]
        r.data_dev = t.data_ptr()
        r.h, r.w = int(t.shape[1]), int(t.shape[2])
        r.oh, r.ow = sizes[i]
        # (the stride of an axis of one element is arbitrary: hand over the class's own)
        r.stride_ch = 1 if interleaved else (t.stride(0) if k > 1 else 0)
        r.stride_row = t.stride(1) if r.h > 1 else 0
        r.stride_px = k if interleaved else 1
        r.flags = _lib.MANY_FLIP_X if flips is not None and flips[i] else 0
    return recs, keep, interleaved


def _back_views(arena, offs, sizes, reduce, k: int):
    """The outputs of a return-path call as views of its arena: [oh, ow] at byte offs[i] for argmax, else [K, oh, ow]."""
    es, outs = arena.element_size(), []
    for i, (oh, ow) in enumerate(sizes):
        shape = (oh, ow) if reduce == "argmax" else (k, oh, ow)
        outs.append(arena[offs[i] // es:offs[i] // es + math.prod(shape)].view(shape))
    return outs


def _resize_many_back_run(plan, items, merged=None):
    """The layout class, the plan and the two launches of resize_many_back on checked GPU items -> (N views of one arena, whether the
    items were read as interleaved classes).  merged: None, or (groups, the G groups' sizes, merge) of resize_many_back_merged, whose
    plan's sizes are the members' (each its group's): the merged planner and launch, and G views."""
    name, mode, n, k, sizes, rects, flips, reduce, reduce_id, out_dtype, out_id, threshold, act_id = plan
    dev = items[0].device
    recs, keep, interleaved = _back_records(items, rects, sizes, flips, k)  # (keep: alive until the launches are enqueued)
    layout = _lib.NHWC if interleaved else _lib.NCHW
    L = _lib.load()
    arena_bytes = ctypes.c_size_t(0)
    es = torch.empty((), dtype=out_dtype).element_size()
    if merged is None:
        out_sizes, offs = sizes, (ctypes.c_int64 * n)()
        desc_bytes, resample = L.aa_back_many_desc_bytes(n), L.aa_resample_back_many

        def planner(desc, nbytes, ws_bytes):
            return L.aa_back_many_plan_act(_lib.FILTER_IDS[mode], layout, n, k, recs, reduce_id, act_id, out_id, desc, nbytes, ws_bytes,
                                           ctypes.byref(arena_bytes), offs)
    else:
        groups, out_sizes, merge = merged
        g = len(out_sizes)
        offs, group_of = (ctypes.c_int64 * g)(), (ctypes.c_int64 * n)(*groups)
        desc_bytes, resample = L.aa_back_merged_desc_bytes(n, g), L.aa_resample_back_merged

        def planner(desc, nbytes, ws_bytes):
            return L.aa_back_merged_plan_act(_lib.FILTER_IDS[mode], layout, n, k, recs, g, group_of, _lib.BACK_MERGE[merge], reduce_id, act_id, out_id,
                                             desc, nbytes, ws_bytes, ctypes.byref(arena_bytes), offs)
    arena = _many_run(
        name, dev, desc_bytes, planner, lambda: torch.empty((arena_bytes.value // es,), dtype=out_dtype, device=dev),
        lambda desc_host, desc_dev, out, ws, stream: resample(desc_host, desc_dev, _DTYPE_IDS[items[0].dtype], threshold, out.data_ptr(),
                                                              out.numel() * es, ws.data_ptr(), ws.numel(), stream))[0]
    return _back_views(arena, offs, out_sizes, reduce, k), interleaved


def _back_input_grads(ctx, grads, first: int = 2):
    """What the backward of a return-path autograd node returns for its inputs from number ``first`` on, the batch tensor or the list's
    items: resize_many_back_backward of the N items' gradients (None: not used) on the geometry ctx saved."""
    _, mode, n, k, _, rects, flips, *_ = ctx.plan
    kw = dict(regions=rects, flips=flips, channels=k, dtype=ctx.in_dtype, out_format="nhwc" if ctx.interleaved else "nchw", device=ctx.dev)
    if ctx.is_batch:
        return (resize_many_back_backward(grads, ctx.shapes[0][2:], mode, **kw),)
    gs = resize_many_back_backward(grads, [s[-2:] for s in ctx.shapes], mode, **kw)
    return tuple(g.view(s) if ctx.needs_input_grad[first + i] else None for i, (g, s) in enumerate(zip(gs, ctx.shapes)))


class _ResizeManyBack(torch.autograd.Function):
    """resize_many_back(reduce=None) for predictions that require grad: the backward is resize_many_back_backward on the saved geometry,
    in pred's dtype and in the layout class the forward read pred in.  One input (a batch tensor) or N (a list's items); N outputs,
    views of one arena.  Outputs the loss did not use arrive as None and stay None items."""

    @staticmethod
    def forward(ctx, plan, is_batch, *inputs):
        items = list(inputs[0].unbind(0)) if is_batch else [t[0] if t.dim() == 4 else t for t in inputs]
        outs, interleaved = _resize_many_back_run(plan, items)
        ctx.plan, ctx.is_batch, ctx.interleaved = plan, is_batch, interleaved
        ctx.shapes, ctx.in_dtype, ctx.dev = [tuple(t.shape) for t in inputs], inputs[0].dtype, inputs[0].device
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        return (None, None) + _back_input_grads(ctx, grads)


def _back_groups(name: str, groups, n: int, g: int):
    """groups of resize_many_back_merged, checked -> (N ints in 0 .. G - 1, the members of every group, each at least 1)."""
    try:
        groups = list(groups)
    except TypeError:
        raise ValueError(f"{name}(): groups must be N integers, got {groups!r}") from None
    if len(groups) != n:
        raise ValueError(f"{name}(): groups must hold one entry per item ({n}), got {len(groups)}")
    counts = [0] * g
    for i, v in enumerate(groups):
        try:
            if isinstance(v, bool) or int(v) != v:
                raise TypeError
        except (TypeError, ValueError):
            raise ValueError(f"{name}(): groups[{i}] must be an integer, got {v!r}") from None
        if not (0 <= int(v) < g):
            raise ValueError(f"{name}(): groups[{i}] = {int(v)} is outside 0 .. {g - 1}, the groups that sizes states ({g})")
        groups[i] = int(v)
        counts[groups[i]] += 1
    for j, c in enumerate(counts):
        if c == 0:
            raise ValueError(f"{name}(): group {j} (sizes[{j}]) has no member: every group needs at least one entry of groups")
    return groups, counts


def resize_many_back_merged(pred, groups, sizes, mode: str = "bilinear", *, regions=None, flips=None, merge: str = "sum",
                            reduce: Optional[str] = None, threshold: float = 0.0, out_dtype=None, channels: Optional[int] = None,
                            activation: Optional[str] = None):
    """Test-time augmentation's merge: several passes per image — scales, mirrored or not — each brought back to the image's own size as
    ``resize_many_back`` does, un-mirrored, SUMMED per image, and only then reduced to a label, a mask or values.  ``pred``, ``regions``,
    ``flips``, ``mode``, ``reduce``, ``threshold``, ``out_dtype`` and ``channels`` are ``resize_many_back``'s, with its checks: N items, one
    batch tensor [N, K, H, W] or a list of [K, H_i, W_i], float32 / float16 / bfloat16, read where they lie in one layout class.
    ``groups``: N integers, ``groups[i]`` in 0 .. G - 1 the output that item i contributes to, in any order (a batch laid out pass by pass
    interleaves them); every group has at least one member.  ``sizes``: G pairs (oh_g, ow_g), one per GROUP: every member of group g is
    resampled to that size.  ``merge``: "sum" or "mean".

    With ``R_i`` the fp32 value ``resize_many_back`` defines for item i at size ``sizes[groups[i]]`` — mirrored left to right where
    ``flips[i]``, BEFORE any rounding to ``out_dtype`` — and ``i_0 < i_1 < ... < i_{M-1}`` the members of group g in ascending item index,
    ``S_g = R_{i_0}``, then ``S_g = S_g + R_{i_j}`` for j = 1 .. M - 1: one fp32 round-to-nearest add per element, in that order, no fused
    multiply-add, no reassociation.  ``merge="mean"`` then divides once, ``S_g / float32(M)``, correctly rounded (not a multiplication by a
    reciprocal).  The result is a list of G tensors, bit for bit ``resize_many_back``'s reductions of ``S_g``: ``reduce=None`` gives
    ``S_g.to(out_dtype)`` [K, oh_g, ow_g], ONE rounding; ``"argmax"`` gives ``numpy.argmax`` of the fp32 ``S_g`` over K [oh_g, ow_g];
    ``"greater"`` gives ``S_g > float32(threshold)``.  So a NaN in any member makes the sum NaN; +inf in one member and -inf in another
    at the same pixel and class give NaN, which wins the argmax; and a group of one member is exactly ``resize_many_back``'s item, for
    both merges.

    The tensors are contiguous views of ONE arena, each on a 16-byte boundary of it; G == 0 with N == 0 gives [].  Two launches
    whatever N, G and the sizes — the members' tables, then one resample that walks a group's members per chunk of four classes and adds
    them in registers — and one non-blocking copy of a packed descriptor; nothing is read back, no table cache is touched, the call does
    not synchronise.  With ``"argmax"`` neither the K sums nor any member's values are ever stored.

    Differentiable for ``reduce=None`` like ``resize_many_back``: when gradients are enabled and ``pred`` (or any item of a list) requires
    grad, the results carry a backward, ONE ``resize_many_back_backward`` over all members with member i's gradient that of its group's
    output — for "sum" the same tensor for every member, read where it lies; for "mean" ``G_g.float() / M_g``, one division per used
    group; None for the members of a group the loss did not use.  ``"argmax"`` and ``"greater"`` never carry a ``grad_fn``.

    ``activation``: None, ``"softmax"`` or ``"sigmoid"``, ``resize_many_back``'s, applied to every member's ``R_i`` BEFORE the sum: with
    ``P_i`` as that call defines it, ``S_g`` adds the members' ``P_i`` in the same order, and the mean and the reductions follow
    unchanged — the standard test-time augmentation, softmax per pass, probabilities summed, then the argmax; or sigmoid, ``merge="mean"``
    and ``reduce="greater", threshold=0.5`` for mask heads.  A group of one member is ``resize_many_back``'s item with the same
    activation, bit for bit.  Still two launches and no workspace beyond the tables: for a softmax a lane first walks every member's
    classes once for its maximum and denominator, keeps the pairs in LDS, and then adds probabilities class by class; that bounds a
    softmax group to 16 members (``ValueError`` naming the group; the sigmoid and None have no limit).  Not differentiable: with
    ``reduce=None``, gradients enabled and a ``pred`` that requires grad the call raises ``NotImplementedError`` — call it under
    ``torch.no_grad()`` or pass ``pred.detach()``.

    Not built: per-member weights, a maximum instead of the sum, a backward through the activation, ``log_softmax``,
    sliding-window overlap-add (members placed at different positions of the output), a dense padded output."""
    name = "resize_many_back_merged"
    if mode not in _lib.FILTER_IDS:
        raise ValueError(mode)
    if reduce not in _BACK_REDUCE:
        raise ValueError(f"{name}(): reduce must be None, 'argmax' or 'greater', got {reduce!r}")
    if merge not in _lib.BACK_MERGE:
        raise ValueError(f"{name}(): merge must be 'sum' or 'mean', got {merge!r}")
    _back_activation_name(name, activation)
    items, dev0, n, k = _back_items(name, pred, channels)
    try:
        sizes = list(sizes)
    except TypeError:
        raise ValueError(f"{name}(): sizes must be G pairs (oh, ow), got {sizes!r}") from None
    sizes = _back_sizes(name, sizes, len(sizes), k)
    groups, counts = _back_groups(name, groups, n, len(sizes))
    if activation == "softmax":
        for j, c in enumerate(counts):
            if c > _lib.BACK_ACT_MEMBERS:
                raise ValueError(f"{name}(): group {j} (sizes[{j}]) has {c} members: activation='softmax' takes at most "
                                 f"{_lib.BACK_ACT_MEMBERS} per group")
    rects = _back_regions(name, regions, items)
    flips = _many_flips(name, flips, n)
    reduce_id, out_dtype, out_id, threshold = _back_out(name, reduce, out_dtype, threshold, items, k)
    act_id = _back_activation(name, activation, reduce, pred, items)
    if n == 0:
        return []
    for t in items:
        _require_gpu(t, name)
    plan = (name, mode, n, k, [sizes[g] for g in groups], rects, flips, reduce, reduce_id, out_dtype, out_id, threshold, act_id)
    merged = (groups, sizes, merge)
    if reduce is None and torch.is_grad_enabled():
        if isinstance(pred, torch.Tensor):
            if pred.requires_grad:
                return list(_ResizeManyBackMerged.apply(plan, True, merged, counts, pred))
        elif any(t.requires_grad for t in items):
            return list(_ResizeManyBackMerged.apply(plan, False, merged, counts, *items))
    return _resize_many_back_run(plan, [t.detach() for t in items], merged)[0]


class _ResizeManyBackMerged(torch.autograd.Function):
    """resize_many_back_merged(reduce=None) for predictions that require grad.  A member's gradient is its group's: the backward is
    _ResizeManyBack's, resize_many_back_backward once over the N members, given per member the group's gradient (sum) or the group's
    gradient in float32 divided by the members' count (mean), None where the loss did not use the group."""

    @staticmethod
    def forward(ctx, plan, is_batch, merged, counts, *inputs):
        items = list(inputs[0].unbind(0)) if is_batch else [t[0] if t.dim() == 4 else t for t in inputs]
        outs, interleaved = _resize_many_back_run(plan, items, merged)
        ctx.plan, ctx.is_batch, ctx.interleaved, ctx.merged, ctx.counts = plan, is_batch, interleaved, merged, counts
        ctx.shapes, ctx.in_dtype, ctx.dev = [tuple(t.shape) for t in inputs], inputs[0].dtype, inputs[0].device
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        groups, _, merge = ctx.merged
        if merge == "mean":
            grads = [None if g is None else g.float() / m for g, m in zip(grads, ctx.counts)]
        return (None,) * 4 + _back_input_grads(ctx, [grads[g] for g in groups], first=4)


def _back_canvas(name: str, canvas, n: int, k: int):
    """canvas of resize_many_back_backward -> (whether it is ONE (H, W), [(H_i, W_i)] per item), checked."""
    try:
        canvas = list(canvas)
    except TypeError:
        raise ValueError(f"{name}(): canvas must be (H, W) or N pairs (H_i, W_i), got {canvas!r}") from None
    one = len(canvas) == 2 and not any(isinstance(v, (tuple, list, torch.Size)) for v in canvas)
    pairs = [canvas] if one else canvas
    if not one and len(pairs) != n:
        raise ValueError(f"{name}(): canvas must be (H, W) or hold one pair per item ({n}), got {len(pairs)}")
    out = []
    for i, c in enumerate(pairs):
        hh, ww = _many_int_pair(name, "canvas", i, c)
        if hh < 1 or ww < 1:
            raise ValueError(f"{name}(): canvas[{i}] = ({hh}, {ww}) must be positive")
        if hh > _MANY_MAX or ww > _MANY_MAX or hh * ww * k > _BACK_MAX_ELEMS:
            raise ValueError(f"{name}(): canvas[{i}] = ({hh}, {ww}) with K = {k} is beyond the supported {_MANY_MAX} a side and "
                             f"{_BACK_MAX_ELEMS} elements")
        out.append((hh, ww))
    return one, out * max(n, 1) if one else out


class _CanvasShape:
    """What _back_regions looks at of an item: its shape."""

    def __init__(self, k, hh, ww):
        self.shape = (k, hh, ww)


def resize_many_back_backward(grads, canvas, mode: str = "bilinear", *, regions=None, flips=None, channels: Optional[int] = None, dtype=None,
                              out_format: str = "nchw", device=None):
    """The backward of ``resize_many_back(..., reduce=None)``: the gradients of the resampled items, each at its image's own size, back
    to the canvas — for depth, mask and distillation losses taken at full resolution.  ``grads``: a sequence of N entries, each None
    (autograd's "this output was not used") or a float32 / float16 / bfloat16 GPU tensor [K, oh_i, ow_i]; one dtype, one device and one
    K for all tensors; the items' sizes are the tensors'.  A gradient with ``stride(2) == 1`` is read where it lies, at any plane
    stride, row stride and element-aligned address (a crop of a larger tensor is not copied); any other is copied first.
    ``canvas``: (H, W), the size of the batch the forward read — the result is ONE tensor [N, K, H, W], contiguous
    (``out_format="nchw"``) or channels_last (``"nhwc"``), [0, K, H, W] for N == 0; or a list of N pairs (H_i, W_i), the sizes of a
    list's items — the result is a list of N tensors [K, H_i, W_i], views of one arena, each starting on a 16-byte boundary of it, each
    contiguous (``"nchw"``) or with interleaved classes, strides (1, W_i * K, K) (``"nhwc"``); [] for N == 0.
    ``regions``, ``flips``, ``mode``: exactly what the forward was given (a region lies inside its item's canvas).  ``dtype``: None (the
    gradients' dtype), float32, float16 or bfloat16.  If every entry of ``grads`` is None there is no tensor to take K, the dtype and the
    device from: state them, ``channels=K, dtype=..., device=...`` (otherwise ``channels`` and ``device``, where given, must agree with
    the tensors).

    With ``U_i = G_i``, or ``G_i.flip(-1)`` for a flipped item, and ``B`` the ``<mode>_backward`` of this module in its gather form,
    ``B_i = B(U_i.float()[None], [oh_i, ow_i], [1, K, h, w])[0]``, item i of the result is, bit for bit, ``B_i.to(dtype)`` at
    ``[:, y0:y0 + h, x0:x0 + w]`` — fp32 arithmetic, the horizontal adjoint pass first, an fp32 intermediate, taps in ascending order,
    product and sum rounded apart, ONE rounding to nearest even at the store — and literal +0.0 everywhere else; an item whose gradient is
    None is all +0.0.  No atomics: the bits do not depend on N, on the launch shape or on the run.

    Two launches whatever N and whatever the sizes — one builds every item's two fp32 weight tables and their adjoints, one gathers and
    writes the WHOLE result, the zeros too (there is no memset) — and one non-blocking copy of a packed descriptor; nothing is read back,
    no table cache is touched, the call does not synchronise.  Not built: fractional regions, an atomics form."""
    name = "resize_many_back_backward"
    if mode not in _lib.FILTER_IDS:
        raise ValueError(mode)
    if out_format not in ("nchw", "nhwc"):
        raise ValueError(f"{name}(): out_format must be 'nchw' or 'nhwc', got {out_format!r}")
    if isinstance(grads, torch.Tensor):
        raise ValueError(f"{name}(): grads must be a sequence of N entries, each None or a tensor [K, oh, ow]")
    try:
        grads = list(grads)
    except TypeError:
        raise ValueError(f"{name}(): grads must be a sequence of N entries, each None or a tensor [K, oh, ow]") from None
    n = len(grads)
    live = [i for i, g in enumerate(grads) if g is not None]
    for i in live:
        g = grads[i]
        if not isinstance(g, torch.Tensor):
            raise TypeError(f"{name}(): grads[{i}] must be None or Tensor")
        if g.dim() != 3:
            raise ValueError(f"{name}(): grads[{i}] must be [K, oh, ow], got {list(g.shape)}")
        if g.dtype not in _EMBED_DTYPES:
            raise NotImplementedError(f"{name}(): grads[{i}] of {g.dtype} is not built; torch.float32, torch.float16 or torch.bfloat16")
    first = grads[live[0]] if live else None
    if first is None and (channels is None or dtype is None or (device is None and n > 0)):
        raise ValueError(f"{name}(): no entry of grads is a tensor: state channels=, dtype= and device= (an empty list: channels= and dtype=)")
    k = int(channels) if channels is not None else int(first.shape[0])
    if not (1 <= k <= _MANY_MAX):
        raise ValueError(f"{name}(): K must be in 1 .. {_MANY_MAX}, got K = {k}")
    dev = torch.device(device) if device is not None else (first.device if first is not None else _many_empty_device(None))
    for i in live:
        g = grads[i]
        if g.dtype != first.dtype:
            raise ValueError(f"{name}(): every gradient must have the same dtype: grads[{i}] is {g.dtype}, grads[{live[0]}] {first.dtype}")
        if int(g.shape[0]) != k:
            raise ValueError(f"{name}(): every gradient must have the same K: grads[{i}] has {int(g.shape[0])}, expected {k}")
        if not (int(g.shape[1]) > 0 and int(g.shape[2]) > 0):
            raise ValueError(f"{name}(): grads[{i}] is empty: {list(g.shape)}")
        if g.device != dev:
            raise ValueError(f"{name}(): every gradient must be on the same device: grads[{i}] is on {g.device}, expected {dev}")
    dtype = first.dtype if dtype is None else dtype
    if dtype not in _EMBED_DTYPES:
        raise NotImplementedError(f"{name}(): dtype {dtype} is not built; torch.float32, torch.float16 or torch.bfloat16")
    one, canvases = _back_canvas(name, canvas, n, k)
    # (an item without a gradient has no size: any will do for the check, and the planner does not look at it)
    sizes = _back_sizes(name, [(1, 1) if g is None else (int(g.shape[1]), int(g.shape[2])) for g in grads], n, k)
    rects = _back_regions(name, regions, [_CanvasShape(k, hh, ww) for hh, ww in canvases[:n]])
    flips = _many_flips(name, flips, n)
    nhwc = out_format == "nhwc"
    if n == 0:
        if not one:
            return []
        hh, ww = canvases[0]
        return torch.empty((0, k, hh, ww), dtype=dtype, device=dev, memory_format=torch.channels_last if nhwc else torch.contiguous_format)
    if first is None and dev.type != "cuda":
        raise _lib.AAInterpError(f"{name}: expected device= a ROCm GPU, got '{dev}'. interpolate_antialiasing_amd is the MI355X HIP path "
                                 "only and has no CPU implementation.")
    for i in live:
        _require_gpu(grads[i], name)
    L = _lib.load()
    recs, keep = (_lib.BackBwdItemIn * n)(), []  # (keep: the copies of gradients whose columns are not consecutive, alive until the launches are enqueued)
    for i, g in enumerate(grads):
        r = recs[i]
        r.H, r.W = canvases[i]
        if g is None:
            continue
        g = g.detach()
        if g.shape[2] > 1 and g.stride(2) != 1:
            g = g.contiguous()
            keep.append(g)
        r.grad_dev = g.data_ptr()
        r.stride_ch = g.stride(0) if k > 1 else 0
        r.stride_row = g.stride(1) if g.shape[1] > 1 else 0
        r.y0, r.x0, r.h, r.w = rects[i]
        r.oh, r.ow = sizes[i]
        r.flags = _lib.MANY_FLIP_X if flips is not None and flips[i] else 0
    offs = (ctypes.c_int64 * n)()
    out_bytes = ctypes.c_size_t(0)
    es = torch.empty((), dtype=dtype).element_size()
    grad_id = _DTYPE_IDS[first.dtype if first is not None else dtype]

    def alloc_out():
        if one:
            return torch.empty((n, k) + canvases[0], dtype=dtype, device=dev, memory_format=torch.channels_last if nhwc else torch.contiguous_format)
        return torch.empty((out_bytes.value // es,), dtype=dtype, device=dev)

    out = _many_run(
        name, dev, L.aa_back_many_bwd_desc_bytes(n),
        lambda desc, nbytes, ws_bytes: L.aa_back_many_bwd_plan(_lib.FILTER_IDS[mode], _lib.NHWC if nhwc else _lib.NCHW, n, k, recs, _DTYPE_IDS[dtype],
                                                               1 if one else 0, desc, nbytes, ws_bytes, ctypes.byref(out_bytes), offs),
        alloc_out,
        lambda desc_host, desc_dev, o, ws, stream: L.aa_resample_back_many_bwd(desc_host, desc_dev, grad_id, o.data_ptr(), o.numel() * es,
                                                                               ws.data_ptr(), ws.numel(), stream))[0]
    if one:
        return out
    outs = []
    for i, (hh, ww) in enumerate(canvases):
        flat = out[offs[i] // es:offs[i] // es + k * hh * ww]
        outs.append(flat.view(hh, ww, k).permute(2, 0, 1) if nhwc else flat.view(k, hh, ww))
    return outs


def _reduce_many_factors(name: str, factors, n: int):
    """factors of reduce_many -> [(fx, fy)] per item: one int, one (fx, fy) — a pair of plain integers, as ``reduce`` takes it — or N
    entries, each an int or a pair."""
    def one(what, f):
        try:
            return boxmath.check_factor(f)
        except (ValueError, TypeError) as e:
            raise ValueError(f"{name}(): {what}: {e}") from None

    if not isinstance(factors, (tuple, list)) or (len(factors) == 2 and not any(isinstance(v, (tuple, list)) for v in factors)):
        return [one("factors", factors)] * n
    if len(factors) != n:
        raise ValueError(f"{name}(): factors must be one int, one (fx, fy) or one entry per image ({n}), got {len(factors)}")
    return [one(f"factors[{i}]", f) for i, f in enumerate(factors)]


def _reduce_many_channels(images, channels: Optional[int]):
    """The result of a ragged reduce is a list, so an empty list of images needs no C: any will do."""
    if channels is None and not isinstance(images, torch.Tensor) and len(images) == 0:
        return 1
    return channels


def _reduce_many_check_items(name: str, items, c: int):
    """Dtype, C, sizes and device of every item of a ragged reduce."""
    for i, t in enumerate(items):
        if t.dtype != torch.uint8:
            raise NotImplementedError(f"{name}(): images[{i}] is {t.dtype}; a list of images is Pillow's uint8 arithmetic only")
        if int(t.shape[0]) != c:
            raise ValueError(f"{name}(): every image must have the same C: images[{i}] has {int(t.shape[0])}, expected {c}")
        if not (int(t.shape[1]) > 0 and int(t.shape[2]) > 0):
            raise RuntimeError(f"{name}(): images[{i}] is empty: {list(t.shape)}")
        if t.device != items[0].device:
            raise ValueError(f"{name}(): every image must be on the same device: images[{i}] is on {t.device}, images[0] on {items[0].device}")


def _reduce_many_launch(name: str, items, c: int, factors, rboxes):
    """The plan, the descriptor copy and the one launch of a ragged reduce -> N views [C, rh_i, rw_i] of one arena.  items: checked
    [C, H, W] uint8 GPU tensors (at least one); factors [(fx, fy)], rboxes [(x0, y0, x1, y1)] integer boxes inside their images."""
    n = len(items)
    dev = items[0].device
    classes, interleaved = _many_layout(items, c)
    layout = _lib.NHWC if interleaved else _lib.NCHW
    L = _lib.load()
    recs, keep = (_lib.ReduceItem * n)(), []  # (keep: the copies of items outside the class, alive until the launch is enqueued)
    for i, r in _many_fill_records(recs, items, classes, interleaved, c, keep):
        r.box[:] = rboxes[i]
        r.fx, r.fy = factors[i]
    offs = (ctypes.c_int64 * n)()
    # (the call's workspace is its result: the arena)
    arena = _many_run(name, dev, L.aa_reduce_many_desc_bytes(n),
                      lambda desc, nbytes, arena_bytes: L.aa_reduce_many_plan(layout, n, c, recs, desc, nbytes, arena_bytes, offs), lambda: None,
                      lambda desc_host, desc_dev, _, ws, stream: L.aa_reduce_many_u8(desc_host, desc_dev, ws.data_ptr(), ws.numel(), stream))[1]
    views = []
    for i in range(n):
        rw, rh = boxmath.reduced_size(rboxes[i], factors[i])
        flat = arena[offs[i]:offs[i] + c * rh * rw]
        views.append(flat.view(rh, rw, c).permute(2, 0, 1) if interleaved else flat.view(c, rh, rw))
    return views


def reduce_many(images, factors, *, boxes=None, channels: Optional[int] = None):
    """Pillow's ``Image.reduce(factors[i], boxes[i])`` for a list of uint8 images of different sizes, bit-exact, in ONE launch whatever
    N: ``y[i]`` is ``reduce(images[i][None], factors[i], boxes[i])[0]`` bit for bit.

    ``images``: what ``resize_many`` takes — a sequence of N uint8 GPU tensors [C, H_i, W_i] (or [1, C, H_i, W_i]), or one [N, C, H, W]
    tensor whose slices are the items; same C (1..4) and device for all.  Items are read where they lie, at any row pitch, plane pitch
    and byte offset; the call's layout class is chosen as in ``resize_many``, and an item outside it is copied into it first.
    ``factors`` — PILLOW'S ORDER, X FIRST: one int, one (fx, fy), or N entries, each an int or (fx, fy); fx * fy <= 65536.  (A plain pair of
    integers is always ONE (fx, fy): two per-item ints are written [(a, a), (b, b)].)
    ``boxes``: None, or N entries, each None or an INTEGER box (x0, y0, x1, y1) inside its image.

    The result is a list of N views [C, ceil((y1 - y0) / fy_i), ceil((x1 - x0) / fx_i)] of ONE arena tensor, each dense in the call's
    class (interleaved items: strides (1, rw * C, C)), each starting on a 16-byte boundary: they go straight into ``resize_many``,
    ``resize_many_to_float`` or ``resize_many_to_patches``.  One launch, one non-blocking copy of a packed descriptor from pinned memory,
    no synchronisation, no table cache traffic.  N == 0 gives [].  There is no ``alpha``: Pillow drops ``reducing_gap`` for RGBA / LA
    images (``resize_many(alpha=True)`` takes them as they are), and ``reduce(alpha=True)`` serves a single one."""
    name = "reduce_many"
    if _uint8_mode != "pil":
        raise NotImplementedError(f"{name}(): uint8_mode='harness' is not built for a list of images (Pillow's arithmetic only)")
    items, dev0, n, c = _many_items(name, images, _reduce_many_channels(images, channels), "[]")
    facs = _reduce_many_factors(name, factors, n)
    if boxes is not None and len(boxes) != n:
        raise ValueError(f"{name}(): boxes must hold one entry per image ({n}), got {len(boxes)}")
    _reduce_many_check_items(name, items, c)
    rboxes = []
    for i, t in enumerate(items):
        try:
            rboxes.append(boxmath.check_int_box(boxes[i] if boxes is not None else None, int(t.shape[2]), int(t.shape[1])))
        except (ValueError, TypeError) as e:
            raise ValueError(f"{name}(): boxes[{i}]: {e}") from None
    if n == 0:
        return []
    for t in items:
        _require_gpu(t, name)
    return _reduce_many_launch(name, items, c, facs, rboxes)


def reduce_many_for_resize(images, output_size: Sequence[int], mode: str = "bilinear", *, boxes=None, sizes=None, reducing_gap: float = 2.0,
                           channels: Optional[int] = None):
    """Pillow's first step of ``Image.resize(size, FILTER, box=boxes[i], reducing_gap=g)`` for a whole list -> ``(images2, boxes2)``, the
    arguments of the resize that follows:

        small, b2 = reduce_many_for_resize(decoded, [224, 224], "bicubic", boxes=crops, reducing_gap=2.0)    # one launch
        y = resize_many(small, [224, 224], "bicubic", boxes=b2)                                                 # three

    gives, item for item, the bytes of ``PIL.Image.resize((224, 224), BICUBIC, box=crops[i], reducing_gap=2.0)``; the same holds for
    ``resize_many_to_float`` and ``resize_many_to_patches`` and every option they take (flips, placement, conversion), since a reduced item
    is just another image in device memory.  Per item the factors, the reduce box (Image._get_safe_box) and the shifted box are
    ``boxmath.reducing_plans``: Pillow's arithmetic, from the box and the size the item is resized to (``sizes[i]``, height first, else
    ``output_size``) — never from a place on a canvas, so offsets do not enter.

    Items that Pillow would not reduce (both factors 1, or a full box at the item's own size) come back as the VERY SAME tensor objects
    with their box unchanged: not copied, not launched on.  The others come back as views of one arena (``reduce_many``) with the shifted
    box as four doubles (the resize rounds them to float32, as Pillow's C does).  If no item reduces there is no arena and no launch.
    ``boxes2`` is None only when every entry is None.  There is no ``alpha``: Pillow drops ``reducing_gap`` for RGBA / LA images."""
    name = "reduce_many_for_resize"
    if _uint8_mode != "pil":
        raise NotImplementedError(f"{name}(): uint8_mode='harness' is not built for a list of images (Pillow's arithmetic only)")
    if mode not in _lib.FILTER_IDS:
        raise ValueError(mode)
    oh, ow, items, dev0, n, c = _many_canvas(name, images, output_size, _reduce_many_channels(images, channels), "[]")
    same = items if isinstance(images, torch.Tensor) else list(images)  # (what comes back for an item that is not reduced)
    if sizes is not None:
        if len(sizes) != n:
            raise ValueError(f"{name}(): sizes must hold one entry per image ({n}), got {len(sizes)}")
        sizes = [None if s is None else _many_int_pair(name, "sizes", i, s) for i, s in enumerate(sizes)]
        for i, s in enumerate(sizes):
            if s is not None and (s[0] <= 0 or s[1] <= 0):
                raise ValueError(f"{name}(): sizes[{i}] = ({s[0]}, {s[1]}) must be positive")
    _reduce_many_check_items(name, items, c)
    try:
        plans = boxmath.reducing_plans([(int(t.shape[1]), int(t.shape[2])) for t in items], (oh, ow), mode, boxes, sizes, reducing_gap)
    except (ValueError, TypeError) as e:
        raise ValueError(f"{name}(): {e}") from None
    images2 = list(same)
    boxes2 = list(boxes) if boxes is not None else [None] * n
    for t in items:
        _require_gpu(t, name)
    idx = [i for i, p in enumerate(plans) if p is not None]
    if idx:
        views = _reduce_many_launch(name, [items[i] for i in idx], c, [plans[i][0] for i in idx], [plans[i][1] for i in idx])
        for k, i in enumerate(idx):
            images2[i] = views[k]
            boxes2[i] = plans[i][2]
    return images2, (None if all(b is None for b in boxes2) else boxes2)


def _check_alpha(name: str, input: torch.Tensor, uint8_mode, out_dtype, out_format, mean, std) -> None:
    """alpha=True (Pillow's RGBA / LA resize) is defined for uint8 images in Pillow's arithmetic with 2 or 4 channels, alpha last."""
    if input.dtype != torch.uint8:
        raise ValueError(f"{name}(): alpha=True takes uint8 images (Pillow's RGBA / LA resize), got {input.dtype}")
    if (uint8_mode or _uint8_mode) != "pil":
        raise ValueError(f"{name}(): alpha=True is Pillow's arithmetic; uint8_mode='harness' has no premultiplied alpha")
    if out_dtype is not None or out_format is not None or mean is not None or std is not None:
        raise ValueError(f"{name}(): alpha=True gives uint8 in the input's layout; out_dtype / out_format / mean / std do not apply")
    if input.dim() != 4 or input.shape[1] not in (2, 4):
        raise ValueError(f"{name}(): alpha=True needs [N, 2 or 4, H, W] with straight alpha in the last channel, got {list(input.shape)}")


def _forward_to_float(filter_id: int, name: str, input: torch.Tensor, output_size: Sequence[int], align_corners: bool,
                      scale_factors, out_format: Optional[str], mean, std, flags: int = 0, out_dtype=torch.float32) -> torch.Tensor:
    """Decode-adjacent forward: uint8 in, float32 out, one launch.  The reference's harness spends 0.33 of its
    2.27 ms per image on np.asarray(pil) -> transpose -> .float() before the op (test.py:337-339,55; README.md:416); here the
    uint8 bytes (HWC = channels_last, or CHW) are read directly, the op runs in the reference's fp32 arithmetic and the
    float32 result is written in the requested layout ("nchw" / "nhwc"; default: the input's), optionally normalised
    per channel as (v - mean[c]) / std[c].  Equals ``op(input.float())`` bit for bit.  out_dtype torch.float16 / torch.bfloat16:
    that float32 result, normalisation included, rounded to nearest even once as it is stored, i.e. what ``.to(out_dtype)`` of it
    gives, without the float32 tensor and the second pass."""
    n, c, h, w, oh, ow = _check_sizes(input.shape, output_size)
    if input.numel() == 0 and c == 0:
        raise RuntimeError(f"Non-empty 4D data tensor expected but got a tensor with sizes {list(input.shape)}")
    _require_gpu(input, name)
    L = _lib.load()
    x, layout, _ = _layout_of(input, pitched=False)  # (the uint8-to-float entry point has no strided form)
    if out_format not in (None, "nchw", "nhwc"):
        raise ValueError("out_format must be 'nchw', 'nhwc' or None (same as the input)")
    out_layout = layout if out_format is None else (_lib.NHWC if out_format == "nhwc" else _lib.NCHW)
    cv = _lib.Convert()
    cv.out_layout = out_layout
    cv.normalize = 0
    cv.flags = flags | {torch.float16: _lib.FLAG_OUT_F16, torch.bfloat16: _lib.FLAG_OUT_BF16}.get(out_dtype, 0)
    if (mean is None) != (std is None):
        raise ValueError("mean and std must be given together")
    if mean is not None:
        mean, std = [float(v) for v in mean], [float(v) for v in std]
        if len(mean) != c or len(std) != c or c > 4:
            raise RuntimeError(f"mean/std must hold one value per channel (C = {c} <= 4)")
        cv.normalize = 1
        for i in range(c):
            cv.mean[i], cv.std[i] = mean[i], std[i]
    sh, sw = _user_scales(scale_factors, 2)
    dev = x.device
    mf = torch.channels_last if out_layout == _lib.NHWC else torch.contiguous_format
    out = torch.empty((n, c, oh, ow), dtype=out_dtype, device=dev, memory_format=mf)
    if n == 0:
        return out
    with torch.cuda.device(dev):
        th, tw = tables.get_table_pair(filter_id, _lib.TABLE_F32, h, oh, w, ow, align_corners, sh, sw, dev)
        plan = _plan_launch(L, th, tw, _lib.U8, layout, n, c, h, w, oh, ow, 0, cv)
        _launch(L, name, x, out, plan, _lib.U8, layout, n, c, h, w, 0, None, cv)
    return out


def _backward(filter_id: int, name: str, grad_output: torch.Tensor, output_size: Sequence[int],
              input_size: Sequence[int], align_corners: bool, atomic: bool = False) -> torch.Tensor:
    n, c, h, w, oh, ow = _check_sizes(input_size, output_size)
    # ti_upsample_bilinear2d_backward_cpu checks (s2.2/aa_interpolation_backward_impl.h:202-212)
    if grad_output.dim() != 4:
        raise RuntimeError(f"Expected grad_output to be a tensor of dimension 4 but got: dimension {grad_output.dim()}")
    full = (n, c, oh, ow)
    for i in range(4):
        if grad_output.size(i) != full[i]:
            raise RuntimeError("Expected grad_output to have the same shape as output; "
                               f"output.size({i}) = {full[i]} but got grad_output.size({i}) = {grad_output.size(i)}")
    if grad_output.dtype not in _GRAD_DTYPES:
        raise NotImplementedError(f'"ti_upsample_bilinear2d_backward_cpu" not implemented for '
                                  f'\'{_DTYPE_NAMES.get(grad_output.dtype, str(grad_output.dtype))}\'')
    if atomic and grad_output.dtype in (torch.float16, torch.bfloat16):
        # adds that round to 16 bits one by one are a different and worse result than one rounding of the fp32 sum
        raise NotImplementedError(f"{name}(): atomic=True takes float32 / float64 gradients only; a {grad_output.dtype} gradient has "
                                  "the gather form (atomic=False), or cast it to float32 for the scatter")
    _require_gpu(grad_output, name)
    L = _lib.load()
    go, layout, _ = _layout_of(grad_output, pitched=False)  # (the backward has no strided form)
    dev = go.device
    mf = torch.channels_last if layout == _lib.NHWC else torch.contiguous_format
    gi = torch.empty((n, c, h, w), dtype=go.dtype, device=dev, memory_format=mf)
    if n == 0:
        return gi
    kind = _table_kind(go.dtype, None)  # 16-bit gradients: fp32 arithmetic, one rounding at the store
    dt = _DTYPE_IDS[go.dtype]
    with torch.cuda.device(dev):
        th = tables.get_table(filter_id, kind, h, oh, align_corners, 0.0, dev)
        tw = tables.get_table(filter_id, kind, w, ow, align_corners, 0.0, dev)
        if atomic:
            ah, aw = th.axis(), tw.axis()
            ws_bytes = L.aa_workspace_bytes_bwd(dt, layout, n, c, h, w, oh, ow)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            rc = L.aa_resample_bwd_atomic(ctypes.c_void_p(go.data_ptr()), ctypes.c_void_p(gi.data_ptr()),
                                          ctypes.c_void_p(ws.data_ptr()), ws_bytes, dt, layout, n, c, h, w,
                                          ctypes.byref(ah), ctypes.byref(aw), tables._stream_ptr(dev))
            _lib.check(rc, name)
        else:
            # the gather-form adjoint is a forward resample of grad_out with the transposed tables (what aa_resample_bwd does)
            plan = _plan_launch(L, tables.get_transposed_table(th), tables.get_transposed_table(tw), dt, layout, n, c, oh, ow, h, w, 0)
            _launch(L, name, go, gi, plan, dt, layout, n, c, oh, ow, 0)
    return gi


def _axis_pass_2d(L, x, y, dt, kind, outer, n_in, n_out, inner, table, dev) -> bool:
    """One separable pass of an N-d resample through the FUSED 2-D kernels: the dense array [outer][n][inner] is a stack of 2-D
    images in which only one axis changes — [1,1,outer,n] -> [1,1,outer,n_out] when inner == 1 (the pass runs along rows),
    [outer,1,n,inner] -> [outer,1,n_out,inner] otherwise (along columns) — and the other axis gets the IDENTITY table (box filter,
    same size: one tap of weight exactly 1.0, so x * 1.0 = x bit for bit and no neighbour is ever touched).  Same bytes moved as
    the generic single-axis kernel, but through the streaming kernels.  Returns False (caller runs the single-axis kernel
    aa_resample_axis_fwd, one launch, no workspace) whenever that would NOT be one fused launch: sizes the 2-D entry point cannot
    index, a problem no fused kernel takes (aa_workspace_bytes answers non-zero: the two-launch path would add an identity pass and
    a full-size intermediate, twice the traffic of the single-axis kernel), the fused kernels switched off, and rows so short that
    the identity table (one record per row of the stack) would outweigh them."""
    es = x.element_size()
    if inner == 1:
        if n_in * es < 4 * 84 or outer > (1 << 22):  # identity table: ~84 bytes per row of the stack, cached per distinct `outer`
            return False
        n2, h2, w2, oh2, ow2 = 1, outer, n_in, outer, n_out
        th = tables.get_table(_lib.FILTER_BOX, kind, outer, outer, False, 0.0, dev)
        tw = table
    else:
        n2, h2, w2, oh2, ow2 = outer, n_in, inner, n_out, inner
        th = table
        tw = tables.get_table(_lib.FILTER_BOX, kind, inner, inner, False, 0.0, dev)
    if max(h2, w2, oh2, ow2) >= (1 << 24):
        return False
    plan = _plan_launch(L, th, tw, dt, _lib.NCHW, n2, 1, h2, w2, oh2, ow2, 0)
    if plan[2] != 0:
        return False  # no fused kernel for this pass (or they are disabled): the single-axis kernel is the cheaper form
    _launch(L, "aa_resample_fwd (axis pass)", x, y, plan, dt, _lib.NCHW, n2, 1, h2, w2, 0)
    return True


def _forward_nd(filter_id: int, name: str, input: torch.Tensor, output_size: Sequence[int], align_corners: bool) -> torch.Tensor:
    """1-D (NCL) and 3-D (NCDHW) front-ends: the reference's separable driver is N-d generic
    (s2.2/aa_interpolation_impl.h:536-683, "NCHW, NCL or NCKHW" :545) although only the 2-D callables are bound.
    One aa_resample_axis_fwd per resampled axis, LAST axis first like the reference (:658), contiguous intermediates."""
    if not isinstance(input, torch.Tensor):
        raise TypeError(f"{name}(): argument 'input' must be Tensor")
    nd = input.dim() - 2
    if nd not in (1, 2, 3):
        raise RuntimeError(f"It is expected input_size equals to 3, 4 or 5, but got size {input.dim()}")
    if len(output_size) != nd:
        raise RuntimeError(f"It is expected output_size equals to {nd}, but got size {len(output_size)}")
    if nd == 2:
        return _forward(filter_id, name, input, output_size, align_corners)
    sizes = [int(v) for v in input.shape[2:]]
    osizes = [int(v) for v in output_size]
    if not all(v > 0 for v in sizes + osizes):
        raise RuntimeError(f"Input and output sizes should be greater than 0, but got input {sizes} output {osizes}")
    if input.dtype not in _DTYPE_IDS or input.dtype == torch.uint8:  # Pillow has no 1-D/3-D resize to be exact against
        raise NotImplementedError(f'"upsample_generic_Nd" not implemented for \'{_DTYPE_NAMES.get(input.dtype, str(input.dtype))}\'')
    _require_gpu(input, name)
    L = _lib.load()
    x = input.contiguous()
    dev = x.device
    kind = _table_kind(x.dtype, None)
    dt = _DTYPE_IDS[x.dtype]
    if x.numel() == 0:
        if x.shape[1] == 0:
            raise RuntimeError(f"Non-empty {nd + 2}D data tensor expected but got a tensor with sizes {list(input.shape)}")
        return torch.empty(list(x.shape[:2]) + osizes, dtype=x.dtype, device=dev)
    with torch.cuda.device(dev):
        s = tables._stream_ptr(dev)
        for k in range(nd - 1, -1, -1):
            shape = list(x.shape)
            n_in, n_out = shape[2 + k], osizes[k]
            outer = 1
            for v in shape[:2 + k]:
                outer *= v
            inner = 1
            for v in shape[3 + k:]:
                inner *= v
            t = tables.get_table(filter_id, kind, n_in, n_out, align_corners, 0.0, dev)
            shape[2 + k] = n_out
            y = torch.empty(shape, dtype=x.dtype, device=dev)
            if not _axis_pass_2d(L, x, y, dt, kind, outer, n_in, n_out, inner, t, dev):
                ax = t.axis()
                rc = L.aa_resample_axis_fwd(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()), dt, outer, n_in, inner,
                                            ctypes.byref(ax), s)
                _lib.check(rc, name)
            x = y
    return x


def _backward_nd(filter_id: int, name: str, grad_output: torch.Tensor, output_size: Sequence[int], input_size: Sequence[int],
                 align_corners: bool) -> torch.Tensor:
    """True adjoint of `_forward_nd`: one pass per axis with the transposed table of that axis (the 1-D adjoints act on
    different axes and commute).  The reference's backward header carries 1-D/3-D loops as well
    (aa_interpolation_backward_impl.h:58-78,110-150), non-antialiased like its 2-D one.
    float16 / bfloat16 gradients: fp32 arithmetic in every pass, intermediates in the gradient's dtype, so a 3-D backward rounds
    once per resampled axis, as the 16-bit N-d forward does; a 1-D backward is one pass and equals the fp32 backward of the
    up-cast gradient, cast back, bit for bit."""
    nd = len(input_size) - 2
    if nd not in (1, 2, 3) or len(output_size) != nd:
        raise RuntimeError(f"It is expected input_size equals to 3, 4 or 5 and output_size to match, but got {list(input_size)} "
                           f"and {list(output_size)}")
    if nd == 2:
        return _backward(filter_id, name, grad_output, output_size, input_size, align_corners)
    full = [int(v) for v in input_size[:2]] + [int(v) for v in output_size]
    if list(grad_output.shape) != full:
        raise RuntimeError(f"Expected grad_output to have the same shape as output; output.shape = {full} but got "
                           f"grad_output.shape = {list(grad_output.shape)}")
    if grad_output.dtype not in _GRAD_DTYPES:
        raise NotImplementedError(f'"ti_upsample_bilinear2d_backward_cpu" not implemented for '
                                  f'\'{_DTYPE_NAMES.get(grad_output.dtype, str(grad_output.dtype))}\'')
    _require_gpu(grad_output, name)
    L = _lib.load()
    g = grad_output.contiguous()
    dev = g.device
    kind = _table_kind(g.dtype, None)
    dt = _DTYPE_IDS[g.dtype]
    if g.numel() == 0:
        return torch.zeros([int(v) for v in input_size], dtype=g.dtype, device=dev)
    with torch.cuda.device(dev):
        s = tables._stream_ptr(dev)
        for k in range(nd):
            shape = list(g.shape)
            n_out_fwd, n_in_fwd = shape[2 + k], int(input_size[2 + k])
            outer = 1
            for v in shape[:2 + k]:
                outer *= v
            inner = 1
            for v in shape[3 + k:]:
                inner *= v
            fwd = tables.get_table(filter_id, kind, n_in_fwd, n_out_fwd, align_corners, 0.0, dev)
            tr = tables.get_transposed_table(fwd)  # maps n_out_fwd -> n_in_fwd
            shape[2 + k] = n_in_fwd
            y = torch.empty(shape, dtype=g.dtype, device=dev)
            if not _axis_pass_2d(L, g, y, dt, kind, outer, n_out_fwd, n_in_fwd, inner, tr, dev):
                ax = tr.axis()
                rc = L.aa_resample_axis_fwd(ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(y.data_ptr()), dt, outer, n_out_fwd, inner,
                                            ctypes.byref(ax), s)
                _lib.check(rc, name)
            g = y
    return g


def linear_backward_nd(grad_output: torch.Tensor, output_size: Sequence[int], input_size: Sequence[int],
                       align_corners: bool = False) -> torch.Tensor:
    return _backward_nd(_lib.FILTER_LINEAR, "linear_backward_nd", grad_output, output_size, input_size, align_corners)


def cubic_backward_nd(grad_output: torch.Tensor, output_size: Sequence[int], input_size: Sequence[int],
                      align_corners: bool = False) -> torch.Tensor:
    return _backward_nd(_lib.FILTER_CUBIC, "cubic_backward_nd", grad_output, output_size, input_size, align_corners)


def linear_forward_nd(input: torch.Tensor, output_size: Sequence[int], align_corners: bool = False) -> torch.Tensor:
    """Antialiased linear / bilinear / trilinear resize of an NCL, NCHW or NCDHW tensor."""
    return _forward_nd(_lib.FILTER_LINEAR, "linear_forward_nd", input, output_size, align_corners)


def cubic_forward_nd(input: torch.Tensor, output_size: Sequence[int], align_corners: bool = False) -> torch.Tensor:
    return _forward_nd(_lib.FILTER_CUBIC, "cubic_forward_nd", input, output_size, align_corners)


def nearest_forward_nd(input: torch.Tensor, output_size: Sequence[int], align_corners: bool = False) -> torch.Tensor:
    return _forward_nd(_lib.FILTER_BOX, "nearest_forward_nd", input, output_size, align_corners)


# ---- the reference's callables ---------------------------------------------------------------------------
def linear_forward(input: torch.Tensor, output_size: Sequence[int], align_corners: bool = False, *,
                    uint8_mode: Optional[str] = None, scale_factors: Optional[Sequence[float]] = None, out_dtype=None,
                    out_format: Optional[str] = None, mean=None, std=None, precision: Optional[str] = None,
                    alpha: bool = False, box: Optional[Sequence[float]] = None, reducing_gap: Optional[float] = None) -> torch.Tensor:
    """Anti-Aliased Linear Interpolation forward (s2.2/extension_interpolate.cpp:7-14,47)."""
    return _forward(_lib.FILTER_LINEAR, "linear_forward", input, output_size, align_corners, uint8_mode, scale_factors, out_dtype, out_format,
                    mean, std, precision, alpha, box, reducing_gap)


def nearest_forward(input: torch.Tensor, output_size: Sequence[int], align_corners: bool = False, *,
                    uint8_mode: Optional[str] = None, scale_factors: Optional[Sequence[float]] = None, out_dtype=None,
                    out_format: Optional[str] = None, mean=None, std=None, precision: Optional[str] = None,
                    alpha: bool = False, box: Optional[Sequence[float]] = None, reducing_gap: Optional[float] = None) -> torch.Tensor:
    """Anti-Aliased "Nearest" (really: box filter) forward (s2.2/extension_interpolate.cpp:26-33,48)."""
    return _forward(_lib.FILTER_BOX, "nearest_forward", input, output_size, align_corners, uint8_mode, scale_factors, out_dtype, out_format,
                    mean, std, precision, alpha, box, reducing_gap)


def cubic_forward(input: torch.Tensor, output_size: Sequence[int], align_corners: bool = False, *,
                    uint8_mode: Optional[str] = None, scale_factors: Optional[Sequence[float]] = None, out_dtype=None,
                    out_format: Optional[str] = None, mean=None, std=None, precision: Optional[str] = None,
                    alpha: bool = False, box: Optional[Sequence[float]] = None, reducing_gap: Optional[float] = None) -> torch.Tensor:
    """Anti-Aliased Cubic Interpolation forward (s2.2/extension_interpolate.cpp:35-42,49)."""
    return _forward(_lib.FILTER_CUBIC, "cubic_forward", input, output_size, align_corners, uint8_mode, scale_factors, out_dtype, out_format,
                    mean, std, precision, alpha, box, reducing_gap)


def linear_backward(grad_output: torch.Tensor, output_size: Sequence[int], input_size: Sequence[int],
                    align_corners: bool = False, *, atomic: bool = False) -> torch.Tensor:
    """Backward of linear_forward (s2.2/extension_interpolate.cpp:16-24,50) — the true AA adjoint.  float32 / float64 gradients, and
    float16 / bfloat16 ones in the gather form (atomic=False): backward(g.float()).to(g.dtype) bit for bit."""
    return _backward(_lib.FILTER_LINEAR, "linear_backward", grad_output, output_size, input_size, align_corners, atomic)


def cubic_backward(grad_output: torch.Tensor, output_size: Sequence[int], input_size: Sequence[int],
                   align_corners: bool = False, *, atomic: bool = False) -> torch.Tensor:
    """Backward of cubic_forward (intent at test.py:111-116)."""
    return _backward(_lib.FILTER_CUBIC, "cubic_backward", grad_output, output_size, input_size, align_corners, atomic)


def nearest_backward(grad_output: torch.Tensor, output_size: Sequence[int], input_size: Sequence[int],
                     align_corners: bool = False, *, atomic: bool = False) -> torch.Tensor:
    return _backward(_lib.FILTER_BOX, "nearest_backward", grad_output, output_size, input_size, align_corners, atomic)


def lanczos_forward(input: torch.Tensor, output_size: Sequence[int], align_corners: bool = False, *,
                    uint8_mode: Optional[str] = None, scale_factors: Optional[Sequence[float]] = None, out_dtype=None,
                    out_format: Optional[str] = None, mean=None, std=None, precision: Optional[str] = None,
                    alpha: bool = False, box: Optional[Sequence[float]] = None, reducing_gap: Optional[float] = None) -> torch.Tensor:
    """Antialiased Lanczos-3 forward (Pillow's Image.LANCZOS; uint8 in the default mode equals PIL.Image.resize bit for bit)."""
    return _forward(_lib.FILTER_LANCZOS, "lanczos_forward", input, output_size, align_corners, uint8_mode, scale_factors, out_dtype, out_format,
                    mean, std, precision, alpha, box, reducing_gap)


def hamming_forward(input: torch.Tensor, output_size: Sequence[int], align_corners: bool = False, *,
                    uint8_mode: Optional[str] = None, scale_factors: Optional[Sequence[float]] = None, out_dtype=None,
                    out_format: Optional[str] = None, mean=None, std=None, precision: Optional[str] = None,
                    alpha: bool = False, box: Optional[Sequence[float]] = None, reducing_gap: Optional[float] = None) -> torch.Tensor:
    """Antialiased Hamming-windowed forward (Pillow's Image.HAMMING; uint8 in the default mode equals PIL.Image.resize bit for bit)."""
    return _forward(_lib.FILTER_HAMMING, "hamming_forward", input, output_size, align_corners, uint8_mode, scale_factors, out_dtype, out_format,
                    mean, std, precision, alpha, box, reducing_gap)


def lanczos_backward(grad_output: torch.Tensor, output_size: Sequence[int], input_size: Sequence[int],
                     align_corners: bool = False, *, atomic: bool = False) -> torch.Tensor:
    """Backward of lanczos_forward — the true adjoint."""
    return _backward(_lib.FILTER_LANCZOS, "lanczos_backward", grad_output, output_size, input_size, align_corners, atomic)


def hamming_backward(grad_output: torch.Tensor, output_size: Sequence[int], input_size: Sequence[int],
                     align_corners: bool = False, *, atomic: bool = False) -> torch.Tensor:
    """Backward of hamming_forward — the true adjoint."""
    return _backward(_lib.FILTER_HAMMING, "hamming_backward", grad_output, output_size, input_size, align_corners, atomic)


def lanczos_forward_nd(input: torch.Tensor, output_size: Sequence[int], align_corners: bool = False) -> torch.Tensor:
    return _forward_nd(_lib.FILTER_LANCZOS, "lanczos_forward_nd", input, output_size, align_corners)


def hamming_forward_nd(input: torch.Tensor, output_size: Sequence[int], align_corners: bool = False) -> torch.Tensor:
    return _forward_nd(_lib.FILTER_HAMMING, "hamming_forward_nd", input, output_size, align_corners)


def lanczos_backward_nd(grad_output: torch.Tensor, output_size: Sequence[int], input_size: Sequence[int],
                        align_corners: bool = False) -> torch.Tensor:
    return _backward_nd(_lib.FILTER_LANCZOS, "lanczos_backward_nd", grad_output, output_size, input_size, align_corners)


def hamming_backward_nd(grad_output: torch.Tensor, output_size: Sequence[int], input_size: Sequence[int],
                        align_corners: bool = False) -> torch.Tensor:
    return _backward_nd(_lib.FILTER_HAMMING, "hamming_backward_nd", grad_output, output_size, input_size, align_corners)


# legacy export of every step but step_two_dot_two (step_three/extension_interpolate.cpp:17-19)
forward = linear_forward


# ---- torch.ops.extension_interpolate.* ---------------------------------------------------------------------
def _register_torch_ops() -> None:
    lib = torch.library.Library("extension_interpolate", "DEF")
    fwd_schema = "(Tensor input, int[] output_size, bool align_corners=False) -> Tensor"
    bwd_schema = "(Tensor grad_output, int[] output_size, int[] input_size, bool align_corners=False) -> Tensor"
    fwds = {"linear_forward": linear_forward, "nearest_forward": nearest_forward, "cubic_forward": cubic_forward,
            "forward": linear_forward, "lanczos_forward": lanczos_forward, "hamming_forward": hamming_forward}
    bwds = {"linear_backward": linear_backward, "cubic_backward": cubic_backward, "nearest_backward": nearest_backward,
            "lanczos_backward": lanczos_backward, "hamming_backward": hamming_backward}
    for name in fwds:
        lib.define(name + fwd_schema)
    for name in bwds:
        lib.define(name + bwd_schema)

    lib.define("reduce(Tensor input, int[] factor, int[]? box=None, bool alpha=False) -> Tensor")

    def _mf(x):
        return torch.channels_last if (x.dim() == 4 and not x.is_contiguous()
                                       and x.is_contiguous(memory_format=torch.channels_last)) else torch.contiguous_format

    for name, fn in fwds.items():
        lib.impl(name, (lambda f: lambda input, output_size, align_corners=False: f(input, output_size, align_corners))(fn), "CUDA")
        lib.impl(name, lambda input, output_size, align_corners=False: torch.empty(
            (input.shape[0], input.shape[1], output_size[0], output_size[1]), dtype=input.dtype, device=input.device,
            memory_format=_mf(input)), "Meta")
    def _reduce_meta(input, factor, box=None, alpha=False):
        fx, fy = boxmath.check_factor(tuple(factor) if len(factor) != 1 else factor[0])
        bx = boxmath.check_int_box(box, input.shape[3], input.shape[2])
        ow, oh = boxmath.reduced_size(bx, (fx, fy))
        return torch.empty((input.shape[0], input.shape[1], oh, ow), dtype=input.dtype, device=input.device, memory_format=_mf(input))

    lib.impl("reduce", lambda input, factor, box=None, alpha=False: reduce(
        input, tuple(factor) if len(factor) != 1 else factor[0], box, alpha=alpha), "CUDA")
    lib.impl("reduce", _reduce_meta, "Meta")

    # a list of images into one batch; boxes flattened to 4 N values, a full-image box standing for None
    # sizes and offsets flattened to 2 N ints (height first), fill to 1 or C ints
    lib.define('resize_many(Tensor[] images, int[] output_size, str mode="bilinear", float[]? boxes=None, int[]? sizes=None, '
               'int[]? offsets=None, int[]? fill=None, bool alpha=False) -> Tensor')

    def _many_boxes(images, boxes):
        if boxes is None:
            return None
        if len(boxes) != 4 * len(images):
            raise ValueError(f"resize_many(): boxes must hold 4 values per image ({4 * len(images)}), got {len(boxes)}")
        return [tuple(boxes[4 * i:4 * i + 4]) for i in range(len(images))]

    def _many_pairs(images, flat, what):
        if flat is None:
            return None
        if len(flat) != 2 * len(images):
            raise ValueError(f"resize_many(): {what} must hold 2 values per image ({2 * len(images)}), got {len(flat)}")
        return [tuple(flat[2 * i:2 * i + 2]) for i in range(len(images))]

    def _many_fill(fill):
        return 0 if fill is None else (fill[0] if len(fill) == 1 else list(fill))

    def _many_meta(images, output_size, mode="bilinear", boxes=None, sizes=None, offsets=None, fill=None, alpha=False):
        if not images:
            raise ValueError("resize_many(): the op needs at least one image (an empty list has no C)")
        items = [t[0] if t.dim() == 4 else t for t in images]
        classes = [_many_class(t) for t in items]
        n_inter = sum(1 for a, b in classes if a and not b)
        n_planar = sum(1 for a, b in classes if b and not a)
        c = int(items[0].shape[0])
        mf = torch.channels_last if (c > 1 and n_inter > 0 and n_inter >= n_planar) else torch.contiguous_format
        return torch.empty((len(items), c, output_size[0], output_size[1]), dtype=items[0].dtype, device=items[0].device, memory_format=mf)

    lib.impl("resize_many", lambda images, output_size, mode="bilinear", boxes=None, sizes=None, offsets=None, fill=None, alpha=False: resize_many(
        list(images), output_size, mode, boxes=_many_boxes(images, boxes), sizes=_many_pairs(images, sizes, "sizes"),
        offsets=_many_pairs(images, offsets, "offsets"), fill=_many_fill(fill), alpha=alpha), "CUDA")
    lib.impl("resize_many", _many_meta, "Meta")
    lib.define('resize_many_to_float(Tensor[] images, int[] output_size, str mode="bilinear", float[]? boxes=None, bool[]? flips=None, '
               'ScalarType? out_dtype=None, str? out_format=None, float[]? mean=None, float[]? std=None, int[]? sizes=None, '
               'int[]? offsets=None, int[]? fill=None, bool alpha=False) -> Tensor')

    def _many_float_meta(images, output_size, mode="bilinear", boxes=None, flips=None, out_dtype=None, out_format=None, mean=None, std=None,
                         sizes=None, offsets=None, fill=None, alpha=False):
        u = _many_meta(images, output_size, mode, boxes)
        out_dtype = torch.float32 if out_dtype is None else out_dtype
        nhwc = u.is_contiguous(memory_format=torch.channels_last) and not u.is_contiguous() if out_format is None else out_format == "nhwc"
        return torch.empty(u.shape, dtype=out_dtype, device="meta", memory_format=torch.channels_last if nhwc else torch.contiguous_format)

    lib.impl("resize_many_to_float", lambda images, output_size, mode="bilinear", boxes=None, flips=None, out_dtype=None,
             out_format=None, mean=None, std=None, sizes=None, offsets=None, fill=None, alpha=False: resize_many_to_float(
                 list(images), output_size, mode, boxes=_many_boxes(images, boxes), flips=flips,
                 out_dtype=torch.float32 if out_dtype is None else out_dtype, out_format=out_format,
                 mean=mean, std=std, sizes=_many_pairs(images, sizes, "sizes"), offsets=_many_pairs(images, offsets, "offsets"),
                 fill=_many_fill(fill), alpha=alpha), "CUDA")
    lib.impl("resize_many_to_float", _many_float_meta, "Meta")

    # per-item sizes flattened to 2 N ints (height first), or one pair for all; the Meta shape follows from them alone
    lib.define('resize_many_to_patches(Tensor[] images, int[] patch, str mode, int[] sizes, float[]? boxes, bool[]? flips, str patch_format, '
               'int? pad_to, ScalarType? out_dtype, float[]? mean, float[]? std) -> Tensor')

    def _patch_pairs(images, sizes):
        if len(sizes) == 2:
            return [tuple(sizes)] * len(images)
        if len(sizes) != 2 * len(images):
            raise ValueError(f"resize_many_to_patches(): sizes must hold 2 values per image ({2 * len(images)}) or one pair, got {len(sizes)}")
        return [tuple(sizes[2 * i:2 * i + 2]) for i in range(len(images))]

    def _many_patches_meta(images, patch, mode, sizes, boxes, flips, patch_format, pad_to, out_dtype, mean, std):
        if not images:
            raise ValueError("resize_many_to_patches(): the op needs at least one image (an empty list has no C)")
        t = images[0]
        c = int(t.shape[1] if t.dim() == 4 else t.shape[0])
        (ph, pw), pairs, pad_to = _patch_sizes("resize_many_to_patches", _patch_pairs(images, sizes), tuple(patch), len(images), pad_to)
        rows = boxmath.token_offsets(pairs, (ph, pw))[-1]
        shape = (rows, c * ph * pw) if pad_to is None else (len(images), pad_to, c * ph * pw)
        return torch.empty(shape, dtype=torch.float32 if out_dtype is None else out_dtype, device="meta")

    lib.impl("resize_many_to_patches", lambda images, patch, mode, sizes, boxes, flips, patch_format, pad_to, out_dtype, mean, std:
             resize_many_to_patches(list(images), tuple(patch), mode, sizes=_patch_pairs(images, sizes), boxes=_many_boxes(images, boxes), flips=flips,
                                    patch_format=patch_format, pad_to=pad_to, out_dtype=torch.float32 if out_dtype is None else out_dtype,
                                    mean=mean, std=std), "CUDA")
    lib.impl("resize_many_to_patches", _many_patches_meta, "Meta")

    # Pillow's NEAREST for the label maps: the same flattened boxes / sizes / offsets / fill as resize_many, flips as resize_many_to_float
    lib.define('resize_many_nearest(Tensor[] images, int[] output_size, float[]? boxes=None, bool[]? flips=None, int[]? sizes=None, '
               'int[]? offsets=None, int[]? fill=None, ScalarType? out_dtype=None) -> Tensor')

    def _many_nearest_meta(images, output_size, boxes=None, flips=None, sizes=None, offsets=None, fill=None, out_dtype=None):
        u = _many_meta(images, output_size)
        nhwc = u.is_contiguous(memory_format=torch.channels_last) and not u.is_contiguous()
        return torch.empty(u.shape, dtype=u.dtype if out_dtype is None else out_dtype, device="meta",
                           memory_format=torch.channels_last if nhwc else torch.contiguous_format)

    lib.impl("resize_many_nearest", lambda images, output_size, boxes=None, flips=None, sizes=None, offsets=None, fill=None, out_dtype=None:
             resize_many_nearest(list(images), output_size, boxes=_many_boxes(images, boxes), flips=flips,
                                 sizes=_many_pairs(images, sizes, "sizes"), offsets=_many_pairs(images, offsets, "offsets"),
                                 fill=_many_fill(fill), out_dtype=out_dtype), "CUDA")
    lib.impl("resize_many_nearest", _many_nearest_meta, "Meta")

    # Pillow's I;16 / I / F resize for the measured maps: the same flattened boxes / sizes / offsets and flips; one fill, a float
    lib.define('resize_many_maps(Tensor[] maps, int[] output_size, str mode="bilinear", float[]? boxes=None, bool[]? flips=None, '
               'int[]? sizes=None, int[]? offsets=None, float? fill=None, str overflow="pillow") -> Tensor')

    def _many_maps_meta(maps, output_size, mode="bilinear", boxes=None, flips=None, sizes=None, offsets=None, fill=None, overflow="pillow"):
        if not maps:
            raise ValueError("resize_many_maps(): the op needs at least one map (an empty list has no dtype)")
        return torch.empty((len(maps), 1, output_size[0], output_size[1]), dtype=maps[0].dtype, device="meta")

    def _many_maps_fill(maps, fill):
        if fill is None:
            return 0
        return fill if maps and maps[0].dtype == torch.float32 else (int(fill) if int(fill) == fill else fill)

    lib.impl("resize_many_maps", lambda maps, output_size, mode="bilinear", boxes=None, flips=None, sizes=None, offsets=None, fill=None,
             overflow="pillow": resize_many_maps(list(maps), output_size, mode, boxes=_many_boxes(maps, boxes), flips=flips,
                                                 sizes=_many_pairs(maps, sizes, "sizes"), offsets=_many_pairs(maps, offsets, "offsets"),
                                                 fill=_many_maps_fill(maps, fill), overflow=overflow), "CUDA")
    lib.impl("resize_many_maps", _many_maps_meta, "Meta")

    # subsampled YCbCr planes to an RGB batch: N luma planes; N interleaved [h, w, 2] chroma tensors, or 2 N planes (Cb_0, Cr_0, Cb_1, ...);
    # subsampling one string or N joined by commas; the same flattened boxes / sizes / offsets / fill as resize_many
    lib.define('resize_many_ycbcr(Tensor[] luma, Tensor[] chroma, int[] output_size, str mode="bilinear", str subsampling="420", '
               'float[]? boxes=None, bool[]? flips=None, int[]? sizes=None, int[]? offsets=None, int[]? fill=None, ScalarType? out_dtype=None, '
               'str out_format="nchw", float[]? mean=None, float[]? std=None) -> Tensor')

    def _ycbcr_tuples(luma, chroma):
        n = len(luma)
        if len(chroma) == n:
            return [(luma[i], chroma[i]) for i in range(n)]
        if len(chroma) == 2 * n:
            return [(luma[i], chroma[2 * i], chroma[2 * i + 1]) for i in range(n)]
        raise ValueError(f"resize_many_ycbcr(): chroma must hold one [h, w, 2] tensor or two planes per luma plane ({n}), got {len(chroma)}")

    def _ycbcr_meta(luma, chroma, output_size, mode="bilinear", subsampling="420", boxes=None, flips=None, sizes=None, offsets=None, fill=None,
                    out_dtype=None, out_format="nchw", mean=None, std=None):
        _ycbcr_tuples(luma, chroma)
        mf = torch.channels_last if out_format == "nhwc" else torch.contiguous_format
        return torch.empty((len(luma), 3, output_size[0], output_size[1]), dtype=torch.uint8 if out_dtype is None else out_dtype, device="meta",
                           memory_format=mf)

    def _ycbcr_cuda(luma, chroma, output_size, mode="bilinear", subsampling="420", boxes=None, flips=None, sizes=None, offsets=None, fill=None,
                    out_dtype=None, out_format="nchw", mean=None, std=None):
        subs = subsampling.split(",") if "," in subsampling else subsampling
        return resize_many_ycbcr(_ycbcr_tuples(luma, chroma), output_size, mode, subsampling=subs, boxes=_many_boxes(luma, boxes), flips=flips,
                                 sizes=_many_pairs(luma, sizes, "sizes"), offsets=_many_pairs(luma, offsets, "offsets"),
                                 fill=None if fill is None else list(fill), out_dtype=out_dtype, out_format=out_format, mean=mean, std=std)

    lib.impl("resize_many_ycbcr", _ycbcr_cuda, "CUDA")
    lib.impl("resize_many_ycbcr", _ycbcr_meta, "Meta")

    # the ragged Image.reduce: factors one int, one (fx, fy) or 2 N ints (x first); boxes 4 N ints, a full-image box standing for None
    lib.define("reduce_many(Tensor[] images, int[] factors, int[]? boxes=None) -> Tensor[]")

    def _reduce_many_args(images, factors, boxes):
        n = len(images)
        if len(factors) == 1:
            facs = int(factors[0])
        elif len(factors) == 2:
            facs = (int(factors[0]), int(factors[1]))
        elif len(factors) == 2 * n:
            facs = [(int(factors[2 * i]), int(factors[2 * i + 1])) for i in range(n)]
        else:
            raise ValueError(f"reduce_many(): factors must hold 1 value, one (fx, fy) or 2 values per image ({2 * n}), got {len(factors)}")
        if boxes is not None and len(boxes) != 4 * n:
            raise ValueError(f"reduce_many(): boxes must hold 4 values per image ({4 * n}), got {len(boxes)}")
        return facs, (None if boxes is None else [tuple(int(v) for v in boxes[4 * i:4 * i + 4]) for i in range(n)])

    def _reduce_many_meta(images, factors, boxes=None):
        facs, bxs = _reduce_many_args(images, factors, boxes)
        items = [t[0] if t.dim() == 4 else t for t in images]
        if not items:
            return []
        c = int(items[0].shape[0])
        facs = _reduce_many_factors("reduce_many", facs, len(items))
        _, interleaved = _many_layout(items, c)
        outs = []
        for i, t in enumerate(items):
            bx = boxmath.check_int_box(bxs[i] if bxs is not None else None, int(t.shape[2]), int(t.shape[1]))
            rw, rh = boxmath.reduced_size(bx, facs[i])
            outs.append(torch.empty_strided((c, rh, rw), (1, rw * c, c) if interleaved else (rh * rw, rw, 1), dtype=t.dtype, device=t.device))
        return outs

    def _reduce_many_cuda(images, factors, boxes=None):
        facs, bxs = _reduce_many_args(images, factors, boxes)
        return reduce_many(list(images), facs, boxes=bxs)

    lib.impl("reduce_many", _reduce_many_cuda, "CUDA")
    lib.impl("reduce_many", _reduce_many_meta, "Meta")

    for name, fn in bwds.items():
        lib.impl(name, (lambda f: lambda grad_output, output_size, input_size, align_corners=False:
                        f(grad_output, output_size, input_size, align_corners))(fn), "CUDA")
        lib.impl(name, lambda grad_output, output_size, input_size, align_corners=False: torch.empty(
            tuple(input_size), dtype=grad_output.dtype, device=grad_output.device, memory_format=_mf(grad_output)), "Meta")

    # autograd: d(forward)/d(input) is the matching backward op (true adjoint); differentiable for float32 / float64 and for
    # float16 / bfloat16 (the gradient arrives in the input's dtype and the backward ops take it as it is)
    def _make_autograd(fwd_name, bwd_name):
        def setup_context(ctx, inputs, output):
            input, output_size, align_corners = inputs
            ctx.in_shape = tuple(input.shape)
            ctx.out_size = tuple(output_size)
            ctx.align_corners = align_corners

        def backward(ctx, grad):
            op = getattr(torch.ops.extension_interpolate, bwd_name)
            return op(grad, list(ctx.out_size), list(ctx.in_shape), ctx.align_corners), None, None

        torch.library.register_autograd(f"extension_interpolate::{fwd_name}", backward, setup_context=setup_context, lib=lib)

    _make_autograd("linear_forward", "linear_backward")
    _make_autograd("forward", "linear_backward")
    _make_autograd("cubic_forward", "cubic_backward")
    _make_autograd("nearest_forward", "nearest_backward")
    _make_autograd("lanczos_forward", "lanczos_backward")
    _make_autograd("hamming_forward", "hamming_backward")
    globals()["_torch_library"] = lib  # keep alive


try:
    _register_torch_ops()
except Exception as _e:  # pragma: no cover - registration problems must not hide the direct callables
    import warnings

    warnings.warn(f"torch.ops.extension_interpolate registration failed: {_e}")
