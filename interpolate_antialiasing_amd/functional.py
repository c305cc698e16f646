"""Differentiable convenience wrapper (the counterpart of test.py:122-158's autograd.Function + Module)."""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from ._lib import by_filter_name

# mode -> name of the 2-D callable / of the N-d front-end
_MODES = by_filter_name(lambda f: f.op + "_forward")
_MODES_ND = {**{n: v + "_nd" for n, v in _MODES.items()}, "trilinear": "linear_forward_nd"}


def interpolate_aa(input: torch.Tensor, size: Sequence[int], mode: str = "bilinear", align_corners: bool = False, *,
                   alpha: bool = False, box: Optional[Sequence[float]] = None, reducing_gap: Optional[float] = None) -> torch.Tensor:
    """Antialiased resize of a 4-D GPU tensor to ``size`` = (H, W); differentiable for float32 / float64 and for float16 / bfloat16
    (the gradient has the input's dtype and memory format: fp32 arithmetic, one rounding to nearest even at the store).
    ``mode``: bilinear | bicubic | nearest (= box filter, as in the reference) | lanczos | hamming (Pillow's filters of those names).
    3-D (NCL) and 5-D (NCDHW) inputs take the N-d front-ends (forward only): ``mode`` linear/bilinear/trilinear | bicubic | nearest |
    lanczos | hamming.
    ``alpha=True``: a uint8 [N, 2 or 4, H, W] image with straight alpha last, resized as Pillow resizes "LA" / "RGBA" (premultiplied).
    ``box=(x0, y0, x1, y1)`` — Pillow's order, x first, unlike ``size`` — and ``reducing_gap``: the arguments of those names of
    ``PIL.Image.resize``, for 4-D uint8 images in Pillow's arithmetic (forward only; see extension_interpolate)."""
    if alpha or box is not None or reducing_gap is not None:
        from . import extension_interpolate as ext

        if mode not in _MODES:
            raise ValueError(mode)
        if input.dim() != 4:
            raise ValueError(f"alpha=True, box and reducing_gap need a 4-D uint8 tensor ([N, 2 or 4, H, W] with alpha), got {input.dim()}-D")
        return getattr(ext, _MODES[mode])(input, [int(size[0]), int(size[1])], bool(align_corners), alpha=bool(alpha), box=box,
                                          reducing_gap=reducing_gap)
    if input.dim() in (3, 5):
        from . import extension_interpolate as ext

        if mode not in _MODES_ND:
            raise ValueError(mode)
        return getattr(ext, _MODES_ND[mode])(input, [int(v) for v in size], bool(align_corners))
    if mode not in _MODES:
        raise ValueError(mode)  # test.py:78-79
    op = getattr(torch.ops.extension_interpolate, _MODES[mode])
    return op(input, [int(size[0]), int(size[1])], bool(align_corners))
