"""The numerical functions of the reference's ``preprocess.py`` (tf2.5/scripts/preprocess.py, P:), the step between a resampled scan
and ``predict`` / ``predict_mc``:

  * ``whitening(image, percentile=None)`` (P:29-39): clip to the percentiles {100 - p, p} when given, then (x - mean) / std over the
    whole array (population std), zeros when std is not positive;
  * ``center_crop(img, cropz, cropx, cropy, center_2d_coords=None, multi_channel=False)`` (P:42-49);
  * ``resize_image_with_crop_or_pad(image, img_size, **kwargs)`` (P:74-98): per axis, pad (target - size) // 2 in front and the rest
    behind, or crop from floor((size - target) / 2); ``kwargs`` are np.pad's ``mode`` and a scalar ``constant_values``;
  * ``resample_img`` (P:52-71) is SimpleITK's B-spline resampler and is not built.

A numpy array is processed on the host with numpy only (``whitening`` by the reference's own numpy calls; ``whitening_host`` /
``crop_pad_host`` are the restatement the tests measure the kernels against, pinned against a direct numpy computation, not against
the reference file, whose imports need SimpleITK, cv2, nibabel and dipy).  A device tensor goes through the kernels of
csrc/preprocess.hip and returns a device tensor; there the results are fp32 (every int16 is exact in fp32).

``prepare_input`` is what the kernels were fused for: raw (B,d,h,w,C) fp32 / int16 on the device -> the whitened, cropped / padded
(B,*img_size,C) network input in the model's storage type, every (sample, channel) on its own, with no host synchronisation and no
cropped intermediate volume: the statistics and the element pass read the source through the crop / pad index map.

Differences from the reference, on purpose: a ``center_crop`` window that leaves the volume raises ValueError (Python's negative-slice
wrap at P:48-49 is an accident); pad modes other than constant / edge / reflect / symmetric raise NotImplementedError; non-finite
input is outside the contract (P:38's ``image * 0.`` keeps NaNs by accident).
"""
from __future__ import annotations

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
    raise NotImplementedError("resample_img (P:52-71) is SimpleITK's ResampleImageFilter (B-spline / nearest neighbour on an ITK image): "
                              "it is not built here; resample with SimpleITK and hand the array to prepare_input")


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
