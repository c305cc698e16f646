"""Host arithmetic of Pillow's ``Image.resize(size, resample, box=..., reducing_gap=...)`` and ``Image.reduce``: plain Python doubles and
ints, no torch, no GPU.  Everything here restates Pillow's own Python (Image.resize, Image._get_safe_box) or the double arithmetic of
its C (precompute_coeffs), so that the device code only ever sees integers and the two doubles in0 / in1.

ORDER OF COORDINATES: ``box`` and ``factor`` are Pillow's — x first: box = (x0, y0, x1, y1), factor = (fx, fy) — while ``output_size``
everywhere in this package is (H, W).
"""
from __future__ import annotations

import math
import struct
from typing import Optional, Sequence, Tuple

from ._lib import by_filter_name  # (ctypes only: nothing is loaded)

SUPPORT = by_filter_name(lambda f: f.support)  # Pillow's filter supports by the package's filter names
MAX_REDUCE_BLOCK = 65536  # fx * fy the reduce kernel's 32-bit sums hold


def f32(v: float) -> float:
    """v rounded to float32: Pillow's C takes the resize box as four floats."""
    return struct.unpack("f", struct.pack("f", v))[0]


def box_f32(box: Sequence[float]) -> Tuple[float, float, float, float]:
    """The box as Pillow's C resize sees it.  (The Python above it — the reducing_gap logic — works on the doubles.)  A box narrower
    than the floats can tell apart is empty there, and is refused here with Pillow's words."""
    x0, y0, x1, y1 = (f32(v) for v in box)
    if x1 - x0 <= 0 or y1 - y0 <= 0:
        raise ValueError("box can't be empty")
    return x0, y0, x1, y1


def check_box(box: Sequence[float], width: int, height: int) -> Tuple[float, float, float, float]:
    """Pillow's checks of a resize / reduce box (x0, y0, x1, y1), with its wording."""
    if len(box) != 4:
        raise ValueError("box must be (x0, y0, x1, y1)")
    x0, y0, x1, y1 = (float(v) for v in box)
    if not all(math.isfinite(v) for v in (x0, y0, x1, y1)):
        raise ValueError("box must hold finite numbers")
    if x0 < 0 or y0 < 0:
        raise ValueError("box offset can't be negative")
    if x1 > width or y1 > height:
        raise ValueError("box can't exceed original image size")
    if x1 - x0 <= 0 or y1 - y0 <= 0:
        raise ValueError("box can't be empty")
    return x0, y0, x1, y1


def check_int_box(box: Optional[Sequence[int]], width: int, height: int) -> Tuple[int, int, int, int]:
    """The integer box of Image.reduce; None = the whole image."""
    if box is None:
        return 0, 0, int(width), int(height)
    if len(box) != 4 or any(int(v) != v for v in box):
        raise ValueError("reduce box must be four integers (x0, y0, x1, y1)")
    x0, y0, x1, y1 = check_box(box, width, height)
    return int(x0), int(y0), int(x1), int(y1)


def check_factor(factor) -> Tuple[int, int]:
    """Image.reduce's factor: an int or (fx, fy), each at least 1; fx * fy within what the kernel's sums hold."""
    if isinstance(factor, (tuple, list)):
        if len(factor) != 2:
            raise ValueError("factor must be an int or (fx, fy)")
        fx, fy = factor
    else:
        fx = fy = factor
    if int(fx) != fx or int(fy) != fy or fx < 1 or fy < 1:
        raise ValueError("the factor must be greater than 0")
    fx, fy = int(fx), int(fy)
    if fx * fy > MAX_REDUCE_BLOCK:
        raise ValueError(f"reduce: fx * fy = {fx * fy} is beyond the supported {MAX_REDUCE_BLOCK}")
    return fx, fy


def reduced_size(box: Sequence[int], factor: Tuple[int, int]) -> Tuple[int, int]:
    """(width, height) of Image.reduce's result."""
    x0, y0, x1, y1 = box
    return (x1 - x0 + factor[0] - 1) // factor[0], (y1 - y0 + factor[1] - 1) // factor[1]


def check_reducing_gap(reducing_gap) -> Optional[float]:
    if reducing_gap is None:
        return None
    if reducing_gap < 1.0:
        raise ValueError("reducing_gap must be 1.0 or greater")
    return float(reducing_gap)


def reducing_factors(box: Sequence[float], out_w: int, out_h: int, reducing_gap: float) -> Tuple[int, int]:
    """Image.resize: the integer factors (fx, fy) of the reduce that goes first."""
    fx = int((box[2] - box[0]) / out_w / reducing_gap) or 1
    fy = int((box[3] - box[1]) / out_h / reducing_gap) or 1
    return fx, fy


def safe_box(width: int, height: int, out_w: int, out_h: int, filter_name: str, box: Sequence[float]) -> Tuple[int, int, int, int]:
    """Image._get_safe_box: the integer box the reduce must cover so that the filter that follows still sees every pixel it needs."""
    s = SUPPORT[filter_name] - 0.5
    sx = s * ((box[2] - box[0]) / out_w)
    sy = s * ((box[3] - box[1]) / out_h)
    return (max(0, int(box[0] - sx)), max(0, int(box[1] - sy)), min(width, math.ceil(box[2] + sx)), min(height, math.ceil(box[3] + sy)))


def shifted_box(box: Sequence[float], rb: Sequence[int], factor: Tuple[int, int]) -> Tuple[float, float, float, float]:
    """Image.resize: the box in the coordinates of the reduced image."""
    fx, fy = factor
    return (box[0] - rb[0]) / fx, (box[1] - rb[1]) / fy, (box[2] - rb[0]) / fx, (box[3] - rb[1]) / fy


def reducing_plan(width: int, height: int, out_w: int, out_h: int, filter_name: str, box: Sequence[float], reducing_gap: float):
    """-> None when both factors are 1 (the plain resize), else (factor, reduce box, the box for the resize of the reduced image)."""
    factor = reducing_factors(box, out_w, out_h, reducing_gap)
    if factor[0] <= 1 and factor[1] <= 1:
        return None
    rb = safe_box(width, height, out_w, out_h, filter_name, box)
    return factor, rb, shifted_box(box, rb, factor)


def reducing_plans(shapes, output_size, mode: str, boxes=None, sizes=None, reducing_gap=2.0):
    """``reducing_plan`` for a list: shapes [(H_i, W_i)], the (H, W) every item is resized to (``sizes[i]`` where given, height first, else
    ``output_size``) and one box per item (None: the whole image) -> N entries, each None (both factors are 1: the plain resize) or
    (factor (fx, fy), reduce box (x0, y0, x1, y1) ints, the box for the resize of the reduced image, four doubles).  Pillow computes the
    factors from the box and the size it resizes to, never from a place on a canvas.  An item whose box is full and whose size is its
    own is None whatever the gap: Pillow returns a copy before it looks at reducing_gap.  Errors name the item."""
    if mode not in SUPPORT:
        raise ValueError(mode)
    gap = check_reducing_gap(reducing_gap)
    if gap is None:
        raise ValueError("reducing_gap must be 1.0 or greater")
    n = len(shapes)
    if boxes is not None and len(boxes) != n:
        raise ValueError(f"boxes must hold one entry per image ({n}), got {len(boxes)}")
    if sizes is not None and len(sizes) != n:
        raise ValueError(f"sizes must hold one entry per image ({n}), got {len(sizes)}")
    if len(output_size) != 2:
        raise ValueError(f"output_size must be (H, W), got {output_size!r}")
    plans = []
    for i, (h, w) in enumerate(shapes):
        h, w = int(h), int(w)
        oh, ow = output_size if sizes is None or sizes[i] is None else sizes[i]
        oh, ow = int(oh), int(ow)
        if h <= 0 or w <= 0 or oh <= 0 or ow <= 0:
            raise ValueError(f"images[{i}]: sizes must be positive, got input (H: {h}, W: {w}) output (H: {oh}, W: {ow})")
        bx = (0.0, 0.0, float(w), float(h))
        if boxes is not None and boxes[i] is not None:
            try:
                bx = check_box(boxes[i], w, h)
            except (ValueError, TypeError) as e:
                raise ValueError(f"boxes[{i}]: {e}") from None
        if axis_is_full(w, bx[0], bx[2]) and axis_is_full(h, bx[1], bx[3]) and (h, w) == (oh, ow):
            plans.append(None)
            continue
        plan = reducing_plan(w, h, ow, oh, mode, bx, gap)
        if plan is not None and plan[0][0] * plan[0][1] > MAX_REDUCE_BLOCK:
            raise ValueError(f"images[{i}]: fx * fy = {plan[0][0] * plan[0][1]} beyond {MAX_REDUCE_BLOCK}")
        plans.append(plan)
    return plans


def axis_hull(in_size: int, out_size: int, in0: float, in1: float, filter_name: str) -> Tuple[int, int]:
    """[o, e): what the windows of precompute_coeffs(in_size, in0, in1, out_size) cover together — the first output's xmin and the end of
    the last output's window, both clipped to the axis (window starts and ends are non-decreasing in the output index).  The same
    double operations, in the same order, as the C; in0 and in1 hold float32 values (box_f32), and the scale is their FLOAT difference
    over the output size."""
    scale = f32(in1 - in0) / out_size
    filterscale = 1.0 if scale < 1.0 else scale
    support = SUPPORT[filter_name] * filterscale
    first = in0 + (0 + 0.5) * scale
    last = in0 + ((out_size - 1) + 0.5) * scale
    o = int(first - support + 0.5)
    if o < 0:
        o = 0
    e = int(last + support + 0.5)
    if e > in_size:
        e = in_size
    return o, e


def nearest_axis(in_size: int, out_size: int, b0: Optional[float] = None, b1: Optional[float] = None, closed_form: bool = False) -> Tuple[float, float]:
    """(a, xo0) of one axis of Pillow's ``Image.resize(size, NEAREST, box=)``: the step and the first centre, both doubles.  b0, b1: the
    box's two values on this axis (None: the whole axis).  Pillow's C takes the box as floats, takes their FLOAT difference, and only then
    divides in double.  closed_form: the second value is float32(b0) itself (see nearest_indices)."""
    f0 = f32(0.0 if b0 is None else b0)
    f1 = f32(float(in_size) if b1 is None else b1)
    a = f32(f1 - f0) / out_size
    return a, (f0 if closed_form else f0 + a * 0.5)


def nearest_indices(in_size: int, out_size: int, b0: Optional[float] = None, b1: Optional[float] = None, clamp: bool = False,
                    closed_form: bool = False):
    """The source index of every output index of one axis of ``Image.resize(size, NEAREST, box=)``, as Pillow's affine scaling picks it:

        a = float64(float32(b1) - float32(b0)) / out_size;  xo = float64(float32(b0)) + a * 0.5
        for x in 0 .. out_size - 1:  idx[x] = int(xo);  xo = xo + a

    The ACCUMULATION is the specification: one double add per step, in order.  The closed form ``a * (x + 0.5) + b0`` gives another table
    (2 -> 7 is the smallest case: it reaches exactly 1.0 where the accumulated sum is just below it).  For a box check_box accepts, xo is
    never negative, so int() is the C's truncation.
    closed_form=True is that other table, and it is what Pillow computes for ONE mode: "I;16" is a "special" image type there, served by
    the generic transform, which evaluates ``a * (x + 0.5) + b0`` afresh for every x.  resize_many_nearest follows Pillow in both: int16
    items take closed_form=True, uint8 and int32 items the accumulation.
    clamp: what the device table kernel stores, indices above in_size - 1 pulled back (none occurs for a box inside the image; the
    tests assert that on their cases)."""
    a, xo = nearest_axis(in_size, out_size, b0, b1, closed_form)
    idx = []
    for x in range(int(out_size)):
        i = int(a * (x + 0.5) + xo) if closed_form else int(xo)
        if clamp:
            i = min(max(i, 0), int(in_size) - 1)
        idx.append(i)
        if not closed_form:
            xo = xo + a
    return idx


def fit_sizes(shapes, shorter: Optional[int] = None, longer: Optional[int] = None):
    """[(H_i, W_i)] -> [(vh_i, vw_i)], aspect ratio kept.  shorter=s: the short side becomes s and the long one int(s * long / short),
    torchvision's Resize(int).  longer=s: the long side becomes s and the short one max(1, int(s * short / long)), the letterbox fit.
    Exactly one of the two."""
    if (shorter is None) == (longer is None):
        raise ValueError("fit_sizes: give exactly one of shorter= and longer=")
    s = int(shorter if shorter is not None else longer)
    if s <= 0:
        raise ValueError("fit_sizes: the side must be positive")
    out = []
    for h, w in shapes:
        h, w = int(h), int(w)
        if h <= 0 or w <= 0:
            raise ValueError("fit_sizes: shapes must be positive")
        short, long = (h, w) if h <= w else (w, h)
        if shorter is not None:
            a, b = s, int(s * long / short)  # (short side, long side)
        else:
            a, b = max(1, int(s * short / long)), s
        out.append((a, b) if h <= w else (b, a))
    return out


def check_patch(patch) -> Tuple[int, int]:
    try:
        ph, pw = patch
        if isinstance(ph, bool) or isinstance(pw, bool) or int(ph) != ph or int(pw) != pw:
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError(f"patch must be two integers (ph, pw), got {patch!r}") from None
    if ph < 1 or pw < 1:
        raise ValueError(f"patch = ({ph}, {pw}) must be positive")
    return int(ph), int(pw)


def patch_grids(sizes, patch):
    """[(vh_i, vw_i)] -> [(gh_i, gw_i)]: how many (ph, pw) patches each size holds per axis.  A size that is not a positive multiple of the
    patch on both axes raises ValueError naming the item."""
    ph, pw = check_patch(patch)
    out = []
    for i, (vh, vw) in enumerate(sizes):
        if vh <= 0 or vw <= 0:
            raise ValueError(f"sizes[{i}] = ({vh}, {vw}) must be positive")
        if vh % ph != 0 or vw % pw != 0:
            raise ValueError(f"sizes[{i}] = ({vh}, {vw}) is not a multiple of the patch ({ph}, {pw})")
        out.append((int(vh) // ph, int(vw) // pw))
    return out


def token_offsets(sizes, patch):
    """N + 1 prefix sums of the token counts gh_i * gw_i: item i's tokens are rows [offsets[i], offsets[i + 1]) of the packed matrix.  The
    cu_seqlens of a variable-length attention (the caller puts them on the device)."""
    out = [0]
    for gh, gw in patch_grids(sizes, patch):
        out.append(out[-1] + gh * gw)
    return out


def fit_patch_sizes(shapes, patch, min_tokens: int = 1, max_tokens: Optional[int] = None):
    """[(H_i, W_i)] -> [(vh_i, vw_i)], multiples of the patch (ph, pw) with the aspect ratio kept as well as they allow: the usual rule of
    native-resolution vision towers.  Per axis the nearest multiple (Python's round, at least one patch); if that gives more than
    max_tokens patches, both axes are divided by beta = sqrt(h * w / (max_tokens * ph * pw)) and rounded DOWN to a multiple (at least one
    patch); else if it gives fewer than min_tokens, both are multiplied by beta = sqrt(min_tokens * ph * pw / (h * w)) and rounded UP."""
    ph, pw = check_patch(patch)
    min_tokens = int(min_tokens)
    if min_tokens < 1 or (max_tokens is not None and int(max_tokens) < min_tokens):
        raise ValueError("fit_patch_sizes: 1 <= min_tokens <= max_tokens")
    out = []
    for h, w in shapes:
        h, w = int(h), int(w)
        if h <= 0 or w <= 0:
            raise ValueError("fit_patch_sizes: shapes must be positive")
        vh, vw = max(ph, round(h / ph) * ph), max(pw, round(w / pw) * pw)
        tokens = (vh // ph) * (vw // pw)
        if max_tokens is not None and tokens > max_tokens:
            beta = math.sqrt(h * w / (int(max_tokens) * ph * pw))
            vh, vw = max(ph, math.floor(h / beta / ph) * ph), max(pw, math.floor(w / beta / pw) * pw)
        elif tokens < min_tokens:
            beta = math.sqrt(min_tokens * ph * pw / (h * w))
            vh, vw = math.ceil(h * beta / ph) * ph, math.ceil(w * beta / pw) * pw
        out.append((vh, vw))
    return out


def center_offset(v: int, o: int) -> int:
    """Where the corner of an axis of v pixels lands on a canvas axis of o so that it is centred: a crop (v >= o) with the arithmetic of
    torchvision's center_crop (Python's round, half to even), a pad (v < o) with the smaller half first."""
    return -int(round((v - o) / 2.0)) if v >= o else (o - v) // 2


def placed_regions(sizes, offsets, output_size):
    """[(y0, x0, h, w)]: the rectangle of the [oh, ow] canvas that ``resize_many(..., sizes=, offsets=)`` gave each item — height first,
    like ``output_size``; what ``resize_many_back(regions=)`` takes to bring a prediction on that canvas back to the images.  ``sizes``:
    N pairs (vh_i, vw_i), or None per entry for the whole canvas; ``offsets``: None (every corner at (0, 0)), "center"
    (``center_offset`` per axis) or N pairs (py_i, px_i), None per entry for (0, 0).  An item that does not lie wholly on the canvas
    raises ValueError naming it: a cropped item has no way back to its whole image."""
    oh, ow = (int(v) for v in output_size)
    center = isinstance(offsets, str)
    if center and offsets != "center":
        raise ValueError(f"placed_regions: offsets must be None, 'center' or one entry per item, got {offsets!r}")
    if offsets is not None and not center and len(offsets) != len(sizes):
        raise ValueError(f"placed_regions: offsets must hold one entry per item ({len(sizes)}), got {len(offsets)}")
    out = []
    for i, s in enumerate(sizes):
        vh, vw = (oh, ow) if s is None else (int(s[0]), int(s[1]))
        if vh <= 0 or vw <= 0:
            raise ValueError(f"placed_regions: sizes[{i}] = ({vh}, {vw}) must be positive")
        if center:
            py, px = center_offset(vh, oh), center_offset(vw, ow)
        elif offsets is None or offsets[i] is None:
            py, px = 0, 0
        else:
            py, px = int(offsets[i][0]), int(offsets[i][1])
        if py < 0 or px < 0 or py + vh > oh or px + vw > ow:
            raise ValueError(f"placed_regions: item {i} of size ({vh}, {vw}) at ({py}, {px}) does not lie wholly on the ({oh}, {ow}) canvas: "
                             "a cropped item has no way back to its whole image")
        out.append((py, px, vh, vw))
    return out


def axis_is_full(in_size: int, in0: float, in1: float) -> bool:
    return in0 == 0 and in1 == in_size


def is_plain_crop(box: Sequence[float], out_w: int, out_h: int) -> bool:
    """Pillow's C resize: integer offsets and a box of exactly the output's size is a crop, not a filter."""
    return box[0] == int(box[0]) and box[1] == int(box[1]) and box[2] - box[0] == out_w and box[3] - box[1] == out_h


# ---- subsampled YCbCr planes (resize_many_ycbcr) ----------------------------------------------------------------------------------------------
SUBSAMPLING = {"444": (1, 1), "422": (2, 1), "420": (2, 2), "440": (1, 2)}  # name -> (sx, sy), the luma samples per chroma sample


def check_subsampling(subsampling: str) -> Tuple[int, int]:
    if subsampling not in SUBSAMPLING:
        raise ValueError(f"subsampling must be one of {', '.join(repr(k) for k in SUBSAMPLING)}, got {subsampling!r}")
    return SUBSAMPLING[subsampling]


def chroma_shape(h: int, w: int, subsampling: str) -> Tuple[int, int]:
    """(h, w) of the chroma planes of an [h, w] luma plane: ceil(h / sy), ceil(w / sx), what a JPEG or video decoder produces."""
    sx, sy = check_subsampling(subsampling)
    return -(-int(h) // sy), -(-int(w) // sx)


def chroma_box(box: Optional[Sequence[float]], shape: Sequence[int], subsampling: str) -> Tuple[float, float, float, float]:
    """The box of the chroma planes for a luma box (x0, y0, x1, y1), or for the whole [H, W] = ``shape`` luma plane when None: the luma
    box as Pillow's C sees it (float32 values) over the subsampling, in float32 — a division by 1 or 2, which is exact.  Chroma is
    centred (JFIF siting), so chroma sample j covers the luma interval [j * s, (j + 1) * s) and the coordinates simply scale.  It is a
    proper box even for None: for an odd W, W / sx is half a sample less than the chroma plane's width."""
    sx, sy = check_subsampling(subsampling)
    b = box_f32(box) if box is not None else (0.0, 0.0, f32(float(shape[1])), f32(float(shape[0])))
    return f32(b[0] / sx), f32(b[1] / sy), f32(b[2] / sx), f32(b[3] / sy)


_YCC_COEFFS = (1.402, -0.34414, -0.71414, 1.772)  # R from Cr, G from Cb, G from Cr, B from Cb (Pillow's ConvertYCbCr.c)


def ycbcr_rgb_tables():
    """Pillow's four YCbCr -> RGB tables (R_Cr, G_Cb, G_Cr, B_Cb), 256 ints each: ``int(c * 64 * (v - 128) + 0.5)`` with C's cast, which
    truncates towards zero (Python's int() does too).  R = clip(Y + (R_Cr[Cr] >> 6)), G = clip(Y + ((G_Cb[Cb] + G_Cr[Cr]) >> 6)),
    B = clip(Y + (B_Cb[Cb] >> 6)), >> arithmetic.  The library computes the same entries in registers (csrc/aa_ycbcr.h)."""
    return tuple([int(c * 64 * (v - 128) + 0.5) for v in range(256)] for c in _YCC_COEFFS)
