"""The numerical functions of the reference's ``preprocess.py`` (tf2.5/scripts/preprocess.py, P:), the step between a resampled scan
and ``predict`` / ``predict_mc``:

  * ``whitening(image, percentile=None)`` (P:29-39): clip to the percentiles {100 - p, p} when given, then (x - mean) / std over the
    whole array (population std), zeros when std is not positive;
  * ``center_crop(img, cropz, cropx, cropy, center_2d_coords=None, multi_channel=False)`` (P:42-49);
  * ``resize_image_with_crop_or_pad(image, img_size, **kwargs)`` (P:74-98): per axis, pad (target - size) // 2 in front and the rest
    behind, or crop from floor((size - target) / 2); ``kwargs`` are np.pad's ``mode`` and a scalar ``constant_values``;
  * ``resample_img`` (P:52-71) takes an ITK image and still raises; its numerical content is ``resample(image, spacing, out_spacing,
    is_label)`` on a plain array: the grid of P:52-71 keeps origin and direction and uses the identity transform, so it is axis-aligned,
    output index j of an axis reads the continuous source index j * out_spacing / spacing, and the output size per axis is
    round(size * spacing / out_spacing).  Images use a cubic B-spline, labels nearest neighbour.  Spacings are in array-axis order
    (z, x, y), like the shapes, not in ITK's reversed order.

A numpy array is processed on the host with numpy only (``whitening`` by the reference's own numpy calls; ``whitening_host`` /
``crop_pad_host`` are the restatement the tests measure the kernels against, pinned against a direct numpy computation, not against
the reference file, whose imports need SimpleITK, cv2, nibabel and dipy).  A device tensor goes through the kernels of
csrc/preprocess.hip and returns a device tensor; there the results are fp32 (every int16 is exact in fp32).

``prepare_input`` is what the kernels were fused for: raw (B,d,h,w,C) fp32 / int16 on the device -> the whitened, cropped / padded
(B,*img_size,C) network input in the model's storage type, every (sample, channel) on its own, with no host synchronisation and no
cropped intermediate volume: the statistics and the element pass read the source through the crop / pad index map.

``resample_host`` is the restatement of the resampler: Unser's recursive prefilter (pole sqrt(3) - 2, gain 6, mirror boundary of period
2(n - 1), the causal start as the exact mirror sum) and the 4-tap cubic B-spline sum, axis after axis in the order RESAMPLE_AXIS_ORDER =
(2, 1, 0), which is also the order of the kernels in csrc/resample.hip.  It is pinned against scipy.ndimage (``spline_filter(order=3,
mode='mirror')`` + ``map_coordinates(order=3, mode='mirror', prefilter=False)``), which implements the same algorithm ITK's
BSplineDecompositionImageFilter / BSplineInterpolateImageFunction descend from.  Parity with ITK itself is NOT pinned: SimpleITK is not
installed where this is built.  One known difference: ITK truncates the causal start's sum at a horizon of 1e-10, the restatement (like
scipy) sums it exactly, the kernels truncate it at 24 terms (2.6e-14): at most 1e-10 relative.  ``prepare_scan`` chains the resampler
and ``prepare_input`` on the device and resamples only the part of the grid the crop keeps.

``restore`` is the way back: a map on the network's grid (a softmax, an entropy, a candidate or label map) put on the scan's own grid, the
exact inverse of prepare_scan's geometry (``restore_geometry``, from the same ``scan_window`` / ``crop_or_pad_starts`` / spacings):
linear interpolation for probabilities, nearest neighbour for label-like maps, voxels the network never saw get a default, and a pad
voxel of the network grid is never read.  The reference ships no such step (it has no inference script); ``restore_host`` is the
restatement the kernel of csrc/restore.hip is measured against, pinned against scipy.ndimage.map_coordinates(order=1, mode='nearest').

Differences from the reference's resample_img, on purpose: the default pixel value is a parameter that defaults to 0 (P:66 passes
GetPixelIDValue(), the pixel-TYPE enum, by accident); image results are fp32 (ITK casts back to the input pixel type); direction and
origin do not enter, because P:63-64 keep both.

Differences from the reference, on purpose: a ``center_crop`` window that leaves the volume raises ValueError (Python's negative-slice
wrap at P:48-49 is an accident); pad modes other than constant / edge / reflect / symmetric raise NotImplementedError; non-finite
input is outside the contract (P:38's ``image * 0.`` keeps NaNs by accident).
"""
from __future__ import annotations

import collections
import math
from typing import Sequence, Tuple

import numpy as np
import torch

from .hip import ops

PAD_MODES = ("constant", "edge", "reflect", "symmetric")


# ---- host arithmetic shared by both paths ----------------------------------------------------------------------------------
def percentile_rank(q: float, n: int) -> Tuple[int, float]:
    """(k, gamma) of np.percentile's default (linear) rule on n values, in fp64: virtual = q / 100 * (n - 1), k = floor, gamma = the
    fraction.  The percentile is a[k] + (a[min(k + 1, n - 1)] - a[k]) * gamma on the sorted values."""
    if not 0.0 <= float(q) <= 100.0:
        raise ValueError(f"percentiles must be in the range [0, 100], got {q}")
    virtual = float(np.true_divide(np.float64(q), 100.0) * np.float64(int(n) - 1))
    k = int(math.floor(virtual))
    return min(k, int(n) - 1), virtual - k


def reflect_index(i: int, n: int) -> int:
    """Source index of np.pad(mode='reflect') for any i: period 2(n - 1), the edge not repeated; 0 when n == 1."""
    if n == 1:
        return 0
    r = i % (2 * (n - 1))
    return r if r < n else 2 * (n - 1) - r


def symmetric_index(i: int, n: int) -> int:
    """Source index of np.pad(mode='symmetric') for any i: period 2n, the edge repeated."""
    r = i % (2 * n)
    return r if r < n else 2 * n - 1 - r


def _axis_table(size: int, out: int, start: int, mode: str) -> np.ndarray:
    """Source index per output voxel of one axis (-1 where mode 'constant' supplies the value)."""
    idx = np.arange(out) + start
    inside = (idx >= 0) & (idx < size)
    if mode == "constant":
        return np.where(inside, idx, -1)
    if mode == "edge":
        return np.clip(idx, 0, size - 1)
    f = reflect_index if mode == "reflect" else symmetric_index
    return np.array([i if ok else f(int(i), size) for i, ok in zip(idx, inside)], dtype=np.int64)


def crop_pad_host(image: np.ndarray, dst: Sequence[int], start: Sequence[int], mode: str = "constant", cval=0) -> np.ndarray:
    """The index map of m1_crop_pad_t on the host: the leading len(dst) axes of ``image`` are gathered, output voxel o of an axis
    reading source index o + start through ``mode``; trailing axes are kept."""
    if mode not in PAD_MODES:
        raise NotImplementedError(f"pad mode {mode!r} is not built: {', '.join(PAD_MODES)} are")
    out = image
    hole = np.zeros((), dtype=bool)
    for ax, (o, s) in enumerate(zip(dst, start)):
        tab = _axis_table(image.shape[ax], int(o), int(s), mode)
        out = np.take(out, np.maximum(tab, 0), axis=ax)
        shape = [1] * image.ndim
        shape[ax] = int(o)
        hole = hole | (tab < 0).reshape(shape)
    if mode == "constant":
        out = np.where(hole, np.asarray(cval).astype(image.dtype), out)
    return np.ascontiguousarray(out)


def crop_or_pad_starts(shape: Sequence[int], img_size: Sequence[int]):
    """``start`` per axis of resize_image_with_crop_or_pad: -((target - size) // 2) where the axis is padded, floor((size - target)
    / 2) where it is cropped."""
    return [-((int(t) - int(s)) // 2) if int(s) < int(t) else (int(s) - int(t)) // 2 for s, t in zip(shape, img_size)]


def _center_starts(shape, crop, center_2d_coords):
    z, x, y = (int(v) for v in shape[:3])
    cz, cx, cy = (int(v) for v in crop)
    px, py = (int(center_2d_coords[0]), int(center_2d_coords[1])) if center_2d_coords else (x // 2, y // 2)
    start = [z // 2 - cz // 2, px - cx // 2, py - cy // 2]
    for s, c, n, name in zip(start, (cz, cx, cy), (z, x, y), "zxy"):
        if c < 1 or s < 0 or s + c > n:
            raise ValueError(f"center_crop: the {name} window [{s}, {s + c}) leaves the volume's extent {n}")
    return start


def _pad_kwargs(kwargs):
    kw = dict(kwargs)
    mode = kw.pop("mode", "constant")
    cval = kw.pop("constant_values", 0)
    if not isinstance(mode, str) or mode not in PAD_MODES:
        raise NotImplementedError(f"resize_image_with_crop_or_pad: np.pad mode {mode!r} is not built; {', '.join(PAD_MODES)} are")
    if kw:
        raise NotImplementedError(f"resize_image_with_crop_or_pad: np.pad arguments {sorted(kw)} are not built (mode, constant_values are)")
    if np.ndim(cval) != 0:
        raise NotImplementedError("resize_image_with_crop_or_pad: only a scalar constant_values is built")
    if mode != "constant":
        cval = 0
    return mode, cval


def percentile_host(values: np.ndarray, q: float, dtype=np.float64):
    """np.percentile's default rule written out: the two order statistics around ``percentile_rank`` (fp64) and numpy's two-sided
    interpolation, a + (b - a) * gamma below gamma = 0.5 and b - (b - a) * (1 - gamma) from there on, in ``dtype`` values."""
    s = np.sort(np.asarray(values, dtype=dtype), axis=None)
    k, g = percentile_rank(q, s.size)
    a, b, g = s[k], s[min(k + 1, s.size - 1)], dtype(g)
    return b - (b - a) * (dtype(1) - g) if g >= 0.5 else a + (b - a) * g


def whitening_host(image: np.ndarray, percentile=None, dtype=np.float64) -> np.ndarray:
    """The restatement of P:29-39 the tests measure against, in ``dtype`` values (the input is rounded to fp32 first, as P:30 does):
    clip = min(max(x, lo), hi) with the thresholds of ``percentile_host``, mean and population std, (x - mean) / std or zeros.
    float64: the yardstick, equal to np.percentile / np.clip / np.mean / np.std on the fp64 array bit for bit.  float32: the same
    operations on fp32 values with the rank and weight still taken in fp64, which is what the kernels do; np.percentile on an fp32
    array additionally rounds the quantile itself, which moves its threshold by several fp32 ulps (see whitening)."""
    image = np.asarray(image).astype(np.float32).astype(dtype)
    if percentile is not None:
        lo, hi = percentile_host(image, 100 - percentile, dtype), percentile_host(image, percentile, dtype)
        image = np.minimum(np.maximum(image, lo), hi)
    mean, std = np.mean(image, dtype=dtype), np.std(image, dtype=dtype)
    return (image - mean) / std if std > 0 else np.zeros_like(image)


# ---- the reference's functions -----------------------------------------------------------------------------------------------
def _five(t: torch.Tensor, channels: bool) -> torch.Tensor:
    """A (z,x,y[,c]) device volume as the kernels' (1,d,h,w,C)."""
    if t.dtype not in (torch.float32, torch.int16):
        t = t.to(torch.float32)
    t = t.contiguous()
    return t.reshape(1, *t.shape) if channels else t.reshape(1, *t.shape, 1)


def whitening(image, percentile=None):
    """P:29-39 over the whole array, any shape.  numpy in -> fp32 numpy out by the reference's own numpy calls (np.percentile on the
    fp32 array, whose threshold lies up to ~8 fp32 ulps from the percentile of the same values in fp64 on the tests' data); device
    tensor in -> fp32 device tensor out (exact order statistics, fp64 interpolation and statistics, one rounding each)."""
    if not isinstance(image, torch.Tensor):
        image = np.asarray(image).astype(np.float32)
        if percentile is not None:
            image = np.clip(image, np.percentile(image, 100 - percentile), np.percentile(image, percentile))
        mean, std = np.mean(image), np.std(image)
        return (image - mean) / std if std > 0 else np.zeros_like(image)
    n = image.numel()
    if n == 0:
        raise ValueError("whitening: empty image")
    src = _five(image.reshape(1, 1, n), False)
    out, _ = _whiten_device(src, (1, 1, n), (0, 0, 0), "constant", 0.0, percentile, torch.float32)
    return out.reshape(image.shape)


def center_crop(img, cropz, cropx, cropy, center_2d_coords=None, multi_channel=False):
    """P:42-49: the (cropz, cropx, cropy) window around the volume's centre, or around ``center_2d_coords`` in the (x, y) plane; a
    trailing channel axis with ``multi_channel``.  A window that leaves the volume raises ValueError."""
    rank = 4 if multi_channel else 3
    if img.ndim != rank:
        raise ValueError(f"center_crop: a rank-{rank} volume expected (multi_channel={multi_channel}), got shape {tuple(img.shape)}")
    start = _center_starts(img.shape, (cropz, cropx, cropy), center_2d_coords)
    if not isinstance(img, torch.Tensor):
        sl = tuple(slice(s, s + int(c)) for s, c in zip(start, (cropz, cropx, cropy)))
        return img[sl]
    out = ops.crop_pad(_five(img, bool(multi_channel)), (cropz, cropx, cropy), start)
    return out[0] if multi_channel else out[0, ..., 0]


def resize_image_with_crop_or_pad(image, img_size=(64, 64, 64), **kwargs):
    """P:74-98 for rank 3, or rank 4 with a trailing channel axis (which is neither cropped nor padded)."""
    if len(img_size) != 3 or image.ndim not in (3, 4):
        raise ValueError(f"resize_image_with_crop_or_pad: a (z,x,y[,c]) image and three target sizes expected, got {tuple(image.shape)}, "
                         f"{tuple(img_size)}")
    mode, cval = _pad_kwargs(kwargs)
    start = crop_or_pad_starts(image.shape[:3], img_size)
    if not isinstance(image, torch.Tensor):
        return crop_pad_host(image, img_size, start, mode, cval)
    out = ops.crop_pad(_five(image, image.ndim == 4), img_size, start, mode, float(cval))
    return out[0] if image.ndim == 4 else out[0, ..., 0]


def resample_img(itk_image, out_spacing=(2.0, 2.0, 2.0), is_label=False):
    raise NotImplementedError("resample_img (P:52-71) takes a SimpleITK image, and SimpleITK is not a dependency of this package: hand "
                              "the array and its spacing, both in (z, x, y) order, to resample(image, spacing, out_spacing, is_label), "
                              "or the raw batch to prepare_scan")


# ---- resampling to a target spacing (P:52-71) ----------------------------------------------------------------------------------
BSPLINE_POLE = math.sqrt(3.0) - 2.0
RESAMPLE_AXIS_ORDER = (2, 1, 0)


def resample_size(shape, spacing, out_spacing) -> Tuple[int, ...]:
    """P:56-58 per axis: int(np.round(n * (spacing / out_spacing))), np.round's half-to-even included."""
    if not (len(shape) == len(spacing) == len(out_spacing)):
        raise ValueError(f"resample_size: one spacing and one target spacing per axis expected, got {tuple(shape)}, {tuple(spacing)}, "
                         f"{tuple(out_spacing)}")
    size = tuple(int(np.round(int(n) * (float(s) / float(o)))) for n, s, o in zip(shape, spacing, out_spacing))
    if any(v < 1 for v in size):
        raise ValueError(f"resample_size: {tuple(shape)} at spacing {tuple(spacing)} has no voxel at spacing {tuple(out_spacing)}: {size}")
    return size


def resample_steps(spacing, out_spacing) -> Tuple[float, ...]:
    """The continuous source index per output index of every axis, out_spacing / spacing in fp64."""
    steps = tuple(float(o) / float(s) if float(s) > 0.0 else math.nan for s, o in zip(spacing, out_spacing))
    if len(steps) != 3 or not all(math.isfinite(v) and v > 0.0 for v in steps):
        raise ValueError(f"resample: three positive spacings and target spacings expected, got {tuple(spacing)}, {tuple(out_spacing)}")
    return steps


def _resample_window(shape, spacing, out_spacing, window):
    size = resample_size(shape, spacing, out_spacing)
    if window is None:
        return size, tuple((0, n) for n in size)
    window = tuple((int(f), int(c)) for f, c in window)
    if len(window) != 3 or any(f < 0 or c < 1 or f + c > n for (f, c), n in zip(window, size)):
        raise ValueError(f"resample: the window {window} leaves the resampled extent {size}")
    return size, window


def mirror_index(i, n: int):
    """Source index of the mirror boundary (period 2(n - 1), the edge not repeated) for any integer array i; 0 when n == 1."""
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    r = np.mod(i, 2 * (n - 1))
    return np.where(r < n, r, 2 * (n - 1) - r)


def bspline_prefilter_host(c: np.ndarray, axis: int, dtype=np.float64) -> np.ndarray:
    """The cubic B-spline coefficients of the lines of ``c`` along ``axis`` in ``dtype`` values: gain (1 - z)(1 - 1/z), causal start
    = the exact mirror sum (c[0] + z^(n-1) c[n-1] + sum_i z^i (c[i] + z^(n-1) c[n-1-i])) / (1 - z^(2n-2)), c+[k] = gain * s[k] + z *
    c+[k-1], anticausal start z / (z^2 - 1) * (z * c+[n-2] + c+[n-1]), c[k] = z * (c[k+1] - c+[k]).  A line of one voxel is kept."""
    c = np.moveaxis(np.asarray(c, dtype=dtype), axis, 0).copy()
    n = c.shape[0]
    if n < 2:
        return np.moveaxis(c, 0, axis)
    z = dtype(BSPLINE_POLE)
    gain = (dtype(1) - z) * (dtype(1) - dtype(1) / z)
    zn = z
    for _ in range(2, n):
        zn = zn * z
    acc = c[0] + zn * c[n - 1]
    zi = z
    for i in range(1, n - 1):
        acc = acc + zi * (c[i] + zn * c[n - 1 - i])
        zi = zi * z
    acc = acc / (dtype(1) - zn * zn)
    acc = acc * gain
    c[0] = acc
    for k in range(1, n):
        acc = gain * c[k] + z * acc
        c[k] = acc
    acc = (z * c[n - 2] + acc) * (z / (z * z - dtype(1)))
    c[n - 1] = acc
    for k in range(n - 2, -1, -1):
        acc = z * (acc - c[k])
        c[k] = acc
    return np.moveaxis(c, 0, axis)


def resample_coords(n: int, step: float, first: int, count: int):
    """(x, inside) of the outputs first .. first + count - 1 of an axis of n voxels: x = j * step in fp64, inside = -0.5 <= x < n - 0.5
    (ITK's IsInsideBuffer)."""
    x = np.arange(first, first + count, dtype=np.float64) * np.float64(step)
    return x, (x >= -0.5) & (x < n - 0.5)


def _bspline_axis_host(c: np.ndarray, axis: int, x: np.ndarray, dtype) -> np.ndarray:
    """The 4-tap cubic B-spline sum of the coefficient lines along ``axis`` at the coordinates x (fp64; floor and fraction in fp64,
    weights and sums in ``dtype``)."""
    n = c.shape[axis]
    fl = np.floor(x)
    y = (x - fl).astype(dtype)
    zc = dtype(1) - y
    w = (zc * zc * zc / dtype(6), (y * y * (y - dtype(2)) * dtype(3) + dtype(4)) / dtype(6),
         (zc * zc * (zc - dtype(2)) * dtype(3) + dtype(4)) / dtype(6), y * y * y / dtype(6))
    shape = [1] * c.ndim
    shape[axis] = x.size
    i = fl.astype(np.int64)
    t = [np.take(c, mirror_index(i - 1 + k, n), axis=axis) * w[k].reshape(shape) for k in range(4)]
    return ((t[0] + t[1]) + t[2]) + t[3]


def resample_host(image: np.ndarray, spacing, out_spacing=(2.0, 2.0, 2.0), is_label=False, default_value=0, dtype=np.float64,
                  window=None) -> np.ndarray:
    """The restatement of P:52-71 the tests measure against, on a (z,x,y[,c]) array, in ``dtype`` values (the input is rounded to fp32
    first).  Cubic path: for the axes 2, 1, 0 in turn, prefilter the lines of the axis and take the 4-tap sums at x_j = j * (out_spacing
    / spacing); voxels outside on any axis are ``default_value``.  Nearest path (``is_label``): a gather at floor(x + 0.5), dtype kept.
    ``window`` = ((first, count),) * 3 returns those output indices only."""
    image = np.asarray(image)
    if image.ndim not in (3, 4):
        raise ValueError(f"resample: a (z,x,y[,c]) array expected, got shape {tuple(image.shape)}")
    steps = resample_steps(spacing, out_spacing)
    _, window = _resample_window(image.shape[:3], spacing, out_spacing, window)
    coords = [resample_coords(image.shape[a], steps[a], *window[a]) for a in range(3)]
    inside = np.ones((), dtype=bool)
    for a, (_, ok) in enumerate(coords):
        shape = [1] * image.ndim
        shape[a] = ok.size
        inside = inside & ok.reshape(shape)
    if is_label:
        out = image
        for a, (x, ok) in enumerate(coords):
            idx = np.clip(np.floor(np.where(ok, x, 0.0) + 0.5).astype(np.int64), 0, image.shape[a] - 1)
            out = np.take(out, idx, axis=a)
        return np.ascontiguousarray(np.where(inside, out, np.asarray(default_value).astype(image.dtype)).astype(image.dtype))
    out = image.astype(np.float32).astype(dtype)
    for a in RESAMPLE_AXIS_ORDER:
        x, ok = coords[a]
        out = _bspline_axis_host(bspline_prefilter_host(out, a, dtype), a, np.where(ok, x, 0.0), dtype)
    return np.ascontiguousarray(np.where(inside, out, dtype(default_value)))


def _resample_device(src: torch.Tensor, spacing, out_spacing, is_label, default_value, window=None) -> torch.Tensor:
    steps = resample_steps(spacing, out_spacing)
    _, window = _resample_window(src.shape[1:4], spacing, out_spacing, window)
    return ops.resample(src, steps, [c for _, c in window], [f for f, _ in window], 0 if is_label else 3, float(default_value))


def resample(image, spacing, out_spacing=(2.0, 2.0, 2.0), is_label=False, default_value=0):
    """P:52-71 on a (z,x,y[,c]) array: numpy in -> the host path (fp64 compute, fp32 result for images, dtype kept for labels); device
    tensor in -> the kernels of csrc/resample.hip (fp32 out for images, the input's dtype for labels)."""
    if image.ndim not in (3, 4):
        raise ValueError(f"resample: a (z,x,y[,c]) array expected, got shape {tuple(image.shape)}")
    if not isinstance(image, torch.Tensor):
        out = resample_host(image, spacing, out_spacing, is_label, default_value, np.float64)
        return out if is_label else out.astype(np.float32)
    src = image
    if is_label and image.dtype not in (torch.float32, torch.int16):
        src = image.to(torch.int16)                       # (uint8 and the other label types: every class index is exact in int16)
    out = _resample_device(_five(src, image.ndim == 4), spacing, out_spacing, is_label, default_value)
    out = out[0] if image.ndim == 4 else out[0, ..., 0]
    return out.to(image.dtype) if is_label else out


# ---- the fused call ----------------------------------------------------------------------------------------------------------
def _whiten_device(src, dst, start, mode, cval, percentile, dtype):
    bounds = None
    if percentile is not None:
        n = int(dst[0]) * int(dst[1]) * int(dst[2])
        (k0, w0), (k1, w1) = percentile_rank(100 - percentile, n), percentile_rank(percentile, n)
        bounds = ops.order_stats(src, dst, start, (k0, k1), (w0, w1), mode, cval)[1]
    return ops.whiten(src, dst, start, mode, cval, bounds, dtype)


def prepare_input(raw: torch.Tensor, img_size, percentile=None, pad_mode="constant", constant_values=0, center_2d_coords=None,
                  dtype=torch.float32):
    """raw (B,d,h,w,C) fp32 / int16 on the device -> (network input (B,*img_size,C) in ``dtype``, (B,C,2) fp64 {mean, std}).

    Geometry: resize_image_with_crop_or_pad's rule per axis (``pad_mode`` / ``constant_values`` as np.pad's); with
    ``center_2d_coords`` the (h, w) window is center_crop's around that point instead (ValueError when it leaves the volume) and the
    depth axis keeps the crop-or-pad rule.  Every (sample, channel) is then whitened on its own over the cropped / padded volume,
    pad values included (``percentile``: whitening's clip).  3 launches without a percentile, 11 with; nothing synchronises, so the
    call can be captured."""
    if not isinstance(raw, torch.Tensor) or raw.dim() != 5:
        raise ValueError("prepare_input: a device tensor (B,d,h,w,C) expected")
    if len(img_size) != 3:
        raise ValueError(f"prepare_input: three target sizes expected, got {tuple(img_size)}")
    mode, cval = _pad_kwargs({"mode": pad_mode, "constant_values": constant_values})
    start = crop_or_pad_starts(raw.shape[1:4], img_size)
    if center_2d_coords:
        h, w = int(raw.shape[2]), int(raw.shape[3])
        start[1:] = _center_starts((1, h, w), (1, img_size[1], img_size[2]), center_2d_coords)[1:]
    if raw.dtype not in (torch.float32, torch.int16):
        raw = raw.to(torch.float32)
    return _whiten_device(raw.contiguous(), tuple(int(v) for v in img_size), start, mode, float(cval), percentile, dtype)


def scan_window(shape, spacing, out_spacing, img_size):
    """((first, count),) * 3 of the resampled grid that resize_image_with_crop_or_pad to ``img_size`` keeps: the crop window where the
    resampled size exceeds the target, the whole axis otherwise."""
    size = resample_size(shape, spacing, out_spacing)
    return tuple(((n - int(t)) // 2, int(t)) if n > int(t) else (0, n) for n, t in zip(size, img_size))


def prepare_scan(raw: torch.Tensor, spacing, out_spacing, img_size, percentile=None, pad_mode="constant", constant_values=0,
                 dtype=torch.float32, default_value=0):
    """raw (B,d,h,w,C) fp32 / int16 on the device at ``spacing`` -> what prepare_input(resample(raw), img_size, ...) returns, bit for
    bit: the cubic B-spline resampling to ``out_spacing`` of only the part of the grid the crop keeps (``scan_window``; an output does
    not depend on the window it is computed in), then prepare_input on it, which pads the axes that are still short.  3 launches more
    than prepare_input; nothing synchronises, so the call can be captured."""
    if not isinstance(raw, torch.Tensor) or raw.dim() != 5:
        raise ValueError("prepare_scan: a device tensor (B,d,h,w,C) expected")
    if len(img_size) != 3:
        raise ValueError(f"prepare_scan: three target sizes expected, got {tuple(img_size)}")
    if raw.dtype not in (torch.float32, torch.int16):
        raw = raw.to(torch.float32)
    window = scan_window(raw.shape[1:4], spacing, out_spacing, img_size)
    vol = _resample_device(raw.contiguous(), spacing, out_spacing, False, default_value, window)
    return prepare_input(vol, img_size, percentile=percentile, pad_mode=pad_mode, constant_values=constant_values, dtype=dtype)


# ---- back onto the scan's own grid ---------------------------------------------------------------------------------------------
RestoreAxis = collections.namedtuple("RestoreAxis", "n ratio first count lo size")     # one axis of restore_geometry


def restore_geometry(scan_shape, spacing, out_spacing, img_size):
    """What prepare_scan did to a scan of ``scan_shape`` at ``spacing``, per axis, as a RestoreAxis: n = the scan's length; ratio =
    spacing / out_spacing in fp64 (the reciprocal of resample_steps' step); (first, count) = scan_window's part of the resampled grid
    that the crop kept; lo = the pad voxels in front on the network grid, so that its real voxels are [lo, lo + count); size = the
    network's length.  Scan voxel i sits at the window coordinate u = i * ratio - first."""
    if not (len(scan_shape) == len(img_size) == 3) or any(int(v) < 1 for v in tuple(scan_shape) + tuple(img_size)):
        raise ValueError(f"restore: three positive scan extents and three positive network extents expected, got {tuple(scan_shape)}, "
                         f"{tuple(img_size)}")
    resample_steps(spacing, out_spacing)                   # (ValueError unless both are three positive spacings)
    window = scan_window(scan_shape, spacing, out_spacing, img_size)
    axes = []
    for a in range(3):
        first, count = window[a]
        lo = -crop_or_pad_starts((count,), (img_size[a],))[0]
        assert lo >= 0 and lo + count <= int(img_size[a])
        axes.append(RestoreAxis(int(scan_shape[a]), float(spacing[a]) / float(out_spacing[a]), first, count, lo, int(img_size[a])))
    return tuple(axes)


def restore_coords(axis: RestoreAxis):
    """(u, inside) of the scan voxels of an axis: u = i * ratio - first in fp64, inside = -0.5 <= u < count - 0.5 (resample_coords'
    rule on the kept window)."""
    u = np.arange(axis.n, dtype=np.float64) * np.float64(axis.ratio) - np.float64(axis.first)
    return u, (u >= -0.5) & (u < axis.count - 0.5)


def restore_inside(geom) -> np.ndarray:
    """The (d,h,w) mask of the scan voxels that lie inside on every axis."""
    inside = np.ones((), dtype=bool)
    for a, ax in enumerate(geom):
        shape = [1, 1, 1]
        shape[a] = ax.n
        inside = inside & restore_coords(ax)[1].reshape(shape)
    return inside


def restore_host(pred: np.ndarray, scan_shape, spacing, out_spacing, order=1, default_value=0, dtype=np.float64) -> np.ndarray:
    """The restatement the kernel of csrc/restore.hip is measured against, on a (D,H,W[,C]) array whose spatial shape is the network's
    size.  Order 1: the input is rounded to fp32 first; per axis, in the order 0, 1, 2, the taps floor(u) and floor(u) + 1, each
    clamped to [0, count - 1] and then offset by lo, weight y = dtype(u - floor(u)) (coordinate, floor and fraction in fp64), and
    a * (1 - y) + b * y in ``dtype`` values.  Order 0: a gather at floor(u + 0.5), clamped the same way, dtype kept.  Voxels outside on
    any axis are ``default_value``; a pad voxel of the network grid is never read."""
    pred = np.asarray(pred)
    if pred.ndim not in (3, 4):
        raise ValueError(f"restore: a (D,H,W[,C]) array expected, got shape {tuple(pred.shape)}")
    if order not in (0, 1):
        raise NotImplementedError(f"restore: order {order!r} is not built; 0 (nearest) and 1 (linear) are")
    geom = restore_geometry(scan_shape, spacing, out_spacing, pred.shape[:3])
    inside = restore_inside(geom)
    if pred.ndim == 4:
        inside = inside[..., None]
    coords = [restore_coords(ax) for ax in geom]
    if order == 0:
        out = pred
        for a, (ax, (u, ok)) in enumerate(zip(geom, coords)):
            idx = np.clip(np.floor(np.where(ok, u, 0.0) + 0.5).astype(np.int64), 0, ax.count - 1) + ax.lo
            out = np.take(out, idx, axis=a)
        return np.ascontiguousarray(np.where(inside, out, np.asarray(default_value).astype(pred.dtype)).astype(pred.dtype))
    out = pred.astype(np.float32).astype(dtype)
    for a, (ax, (u, ok)) in enumerate(zip(geom, coords)):
        u = np.where(ok, u, 0.0)
        fl = np.floor(u)
        shape = [1] * pred.ndim
        shape[a] = ax.n
        y = (u - fl).astype(dtype).reshape(shape)
        i = fl.astype(np.int64)
        lo_tap = np.take(out, np.clip(i, 0, ax.count - 1) + ax.lo, axis=a)
        hi_tap = np.take(out, np.clip(i + 1, 0, ax.count - 1) + ax.lo, axis=a)
        out = lo_tap * (dtype(1) - y) + hi_tap * y
    return np.ascontiguousarray(np.where(inside, out, dtype(default_value)))


def _channel_range(channels, Cn: int) -> Tuple[int, int]:
    """(c0, nsel) of ``channels``: None = all, an int = that channel alone, a (start, stop) pair / range / slice of step 1."""
    if channels is None:
        return 0, Cn
    if isinstance(channels, (int, np.integer)):
        c0, c1 = int(channels), int(channels) + 1
    elif isinstance(channels, slice):
        c0, c1, step = channels.indices(Cn)
        if step != 1:
            raise ValueError(f"restore: a contiguous channel range expected, got {channels!r}")
    elif isinstance(channels, range):
        if channels.step != 1:
            raise ValueError(f"restore: a contiguous channel range expected, got {channels!r}")
        c0, c1 = channels.start, channels.stop
    else:
        c0, c1 = (int(v) for v in channels)
    if not 0 <= c0 < c1 <= Cn:
        raise ValueError(f"restore: the channel range [{c0}, {c1}) leaves the map's {Cn} channel(s)")
    return c0, c1 - c0


def _restore_device_dtype(dtype, order: int, default_value):
    """The type the kernel runs a device map of ``dtype`` in.  Order 1 computes in fp32 (float64 is rounded to it, as the numpy path
    rounds its input).  Order 0 moves values unchanged, so only exact routes are taken: fp32, int16 and int32 as they are, float16 /
    bfloat16 through fp32, bool / uint8 / int8 through int16 (the result is cast back); float64 and int64 have no exact route and
    raise, as does an int32 default beyond 2^24 (the C ABI carries the default as a float)."""
    if order == 1:
        return torch.float32
    if dtype in (torch.float32, torch.int16, torch.int32):
        if dtype == torch.int32 and abs(int(default_value)) > 2 ** 24:
            raise ValueError(f"restore: an int32 default_value beyond 2^24 in magnitude is not exact on the device path, got {default_value}")
        return dtype
    if dtype in (torch.float16, torch.bfloat16):
        return torch.float32
    if dtype in (torch.bool, torch.uint8, torch.int8):
        return torch.int16
    raise ValueError(f"restore: order 0 keeps every value exactly, and a device map of {dtype} has no exact route through the kernel (fp32, "
                     "int16, int32 run as they are, float16 / bfloat16 through fp32, bool / uint8 / int8 through int16): cast it first, or "
                     "hand a numpy array to the host path")


def restore(pred, scan_shape, spacing, out_spacing, order=1, channels=None, labels=False, default_value=0, default_label=0):
    """A map on the network's grid back on the grid of the scan that prepare_scan(raw of ``scan_shape`` at ``spacing``, spacing,
    out_spacing, img_size = pred's own spatial shape) was given.  ``pred``: (D,H,W), (D,H,W,C) or (B,D,H,W,C).  order 1 (probabilities,
    entropy): linear, fp32 out; order 0 (candidate and label maps): nearest, dtype kept.  ``channels``: None, an int or a (start, stop)
    range of the channels to return (for a lesion model, 1 never writes the background at scan resolution).  ``labels``: also return
    the uint8 argmax over ALL channels of the restored map, ``default_label`` outside -- the probabilities are interpolated and the
    argmax is taken on the scan's grid; labels are never interpolated.  Returns the map, or (map, labels).
    numpy in -> restore_host (fp64 compute, fp32 result; dtype kept for order 0); device tensor in -> the kernel of csrc/restore.hip,
    one launch; for order 0 it keeps dtype and values exactly as the host path does, or raises ValueError for a dtype it has no exact
    route for (float64, int64: ``_restore_device_dtype``)."""
    if pred.ndim not in (3, 4, 5):
        raise ValueError(f"restore: a (D,H,W), (D,H,W,C) or (B,D,H,W,C) map expected, got shape {tuple(pred.shape)}")
    if order not in (0, 1):
        raise NotImplementedError(f"restore: order {order!r} is not built; 0 (nearest) and 1 (linear) are")
    if not 0 <= int(default_label) <= 255:
        raise ValueError(f"restore: a default label in [0, 255] expected, got {default_label}")
    spatial = tuple(int(v) for v in (pred.shape[1:4] if pred.ndim == 5 else pred.shape[:3]))
    Cn = int(pred.shape[-1]) if pred.ndim >= 4 else 1
    geom = restore_geometry(scan_shape, spacing, out_spacing, spatial)
    c0, nsel = _channel_range(channels, Cn)
    if labels and Cn > 255:
        raise ValueError(f"restore: uint8 labels hold at most 255 channels, got {Cn}")
    if not isinstance(pred, torch.Tensor):
        vols = pred if pred.ndim == 5 else pred[None]
        full = np.stack([restore_host(v, scan_shape, spacing, out_spacing, order, default_value, np.float64) for v in vols])
        if order == 1:
            full = full.astype(np.float32)
        full = full if pred.ndim >= 4 else full[..., None]
        out = np.ascontiguousarray(full[..., c0:c0 + nsel])
        lab = np.where(restore_inside(geom), np.argmax(full, axis=-1), int(default_label)).astype(np.uint8) if labels else None
        if pred.ndim < 5:
            out, lab = out[0], (lab[0] if labels else None)
        if pred.ndim == 3:
            out = out[..., 0]
        return (out, lab) if labels else out
    src = pred.to(_restore_device_dtype(pred.dtype, order, default_value))
    src = src.contiguous().reshape(-1 if pred.ndim == 5 else 1, *spatial, Cn)
    g = ops.restore_geom(spatial, [ax.n for ax in geom], [ax.ratio for ax in geom], [ax.first for ax in geom],
                         [ax.count for ax in geom], [ax.lo for ax in geom], order, float(default_value), int(default_label))
    res = ops.restore(src, g, c0, nsel, True, bool(labels))
    out, lab = res if labels else (res, None)
    if order == 0 and out.dtype != pred.dtype:
        out = out.to(pred.dtype)
    if pred.ndim < 5:
        out, lab = out[0], (lab[0] if labels else None)
    if pred.ndim == 3:
        out = out[..., 0]
    return (out, lab) if labels else out
