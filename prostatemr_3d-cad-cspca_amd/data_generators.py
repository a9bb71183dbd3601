"""The reference's data generator (tf2.5/scripts/data_generators.py, "D:" below) with the label preparation on the GPU.

What the reference does to an annotation before it is a training label (D:51-72, 92-97), and what this module restates:

  1. binarisation: lesion grades ``<= 1 -> 0``, ``>= 2 -> 1`` (csPCa is GGG >= 2); zones TZ (``== 1``) and PZ (``== 2``) each on its own;
  2. ``contour_smoothening``: ``cv2.GaussianBlur(slice.astype(uint8), (7, 7), cv2.BORDER_DEFAULT)`` on every axial slice.  The third
     positional argument of GaussianBlur is ``sigmaX`` and ``cv2.BORDER_DEFAULT == 4``: the reference blurs with sigma = 4 over 7 taps,
     in OpenCV's 8-bit fixed-point path, and rounds back to uint8 -- on a 0/1 mask a weighted 7x7 majority filter;
  3. one-hot in the annotation's integer type (zonal background ``1 - tz - pz`` in uint8), the posterior's label channels appended
     to the image in training (zeros in 'valid' / 'test'), a zero ``KL`` target.

The smoothing is written here as an INTEGER rule (``smooth_slices``; DESIGN.md "label feed") restated from OpenCV's bit-exact 8-bit
Gaussian.  It is NOT pinned against cv2 (cv2 is not a dependency of this build): the taps come from ``gaussian_taps_u8`` and are
handed to the kernel as data, so a later pin changes one table.

Two feeds produce the same batches, bit for bit:
  * ``batches(custom_data_generator(sheet, ...), ...)``: the reference's generator on the host (numpy), batched as the trainer does;
  * ``device_batches(sheet, ...)``: the raw image and a uint8 annotation go to the device and ONE launch (ops.prepare_labels,
    csrc/labels.hip) writes the network input, the ``detection`` target and the ``KL`` target there.
"""
from __future__ import annotations

import math
import os
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ddp
from .hip import ops

SIGMA = 4.0                       # cv2.BORDER_DEFAULT, read as sigmaX by the reference's call (D:95-96)
COLUMNS = ("image_path", "label_path", "zones_path")


# ---- the smoothing rule ---------------------------------------------------------------------------------------
def gaussian_taps_u8(n: int, sigma: float) -> List[int]:
    """The ``n`` taps (odd) of a Gaussian of ``sigma``, normalised and scaled by 256, as integers that sum to exactly 256: the outer
    pairs are rounded from the outside in with the rounding error carried to the next tap, the centre takes the remainder.
    ``gaussian_taps_u8(7, 4.0) == [31, 36, 40, 42, 40, 36, 31]`` (unrounded 31.10, 36.36, 39.94, 41.20)."""
    n = int(n)
    if n < 1 or n % 2 == 0 or not sigma > 0:
        raise ValueError(f"gaussian_taps_u8: an odd number of taps and sigma > 0 expected, got n={n}, sigma={sigma}")
    r = n // 2
    g = [math.exp(-((i - r) ** 2) / (2.0 * float(sigma) ** 2)) for i in range(n)]
    total = sum(g)
    taps, err = [0] * n, 0.0
    for i in range(r):
        want = 256.0 * g[i] / total + err
        taps[i] = taps[n - 1 - i] = int(math.floor(want + 0.5))
        err = want - taps[i]
    taps[r] = 256 - 2 * sum(taps[:r])
    return taps


def reflect101(idx: np.ndarray, n: int) -> np.ndarray:
    """cv2.BORDER_REFLECT_101 (``-1 -> 1``, ``n -> n - 2``), repeated until the index is in range; 0 when ``n == 1``."""
    idx = np.asarray(idx, dtype=np.int64)
    if n == 1:
        return np.zeros_like(idx)
    p = 2 * (n - 1)
    idx = np.mod(idx, p)
    return np.where(idx < n, idx, p - idx)


def smooth_slices(mask: np.ndarray, kernel_2d: Sequence[int] = (7, 7), sigma: float = SIGMA) -> np.ndarray:
    """One smoothing pass over every (H, W) slice of a uint8 array (..., H, W), integers throughout:
    ``S(y,x) = sum_dy sum_dx wy[dy] wx[dx] m(r(y+dy,H), r(x+dx,W))``, out = ``(S + 32768) >> 16``.  ``kernel_2d`` = (width, height)
    as cv2 takes it."""
    m = np.asarray(mask)
    if m.dtype != np.uint8 or m.ndim < 2:
        raise ValueError(f"smooth_slices: a uint8 array (..., H, W) expected, got {m.dtype} {m.shape}")
    wx, wy = gaussian_taps_u8(kernel_2d[0], sigma), gaussian_taps_u8(kernel_2d[1], sigma)
    H, W = m.shape[-2:]
    m = m.astype(np.int64)
    ix = reflect101(np.arange(-(len(wx) // 2), W + len(wx) // 2), W)
    iy = reflect101(np.arange(-(len(wy) // 2), H + len(wy) // 2), H)
    rows = sum(w * m[..., ix[d:d + W]] for d, w in enumerate(wx))                     # (..., H, W)
    S = sum(w * rows[..., iy[d:d + H], :] for d, w in enumerate(wy))
    return ((S + 32768) >> 16).astype(np.uint8)


def contour_smoothening(label, kernel_2d=(7, 7), iterations=1):
    """D:92-97.  A numpy array (D, H, W) goes through ``smooth_slices`` (every slice is taken ``astype(uint8)`` and written back in
    the array's own type, in place, as the reference does); a device tensor goes through the kernel (ops.contour_smooth), where only
    the reference's (7, 7) is built."""
    if isinstance(label, torch.Tensor):
        if tuple(int(k) for k in kernel_2d) != (7, 7):
            raise NotImplementedError(f"contour_smoothening on the device: only kernel_2d=(7, 7) is built, got {tuple(kernel_2d)}")
        if int(iterations) > 0:
            m = label if label.dtype == torch.uint8 else label.to(torch.uint8)
            label.copy_(ops.contour_smooth(m.contiguous(), int(iterations), gaussian_taps_u8(7, SIGMA)))
        return label
    for _ in range(int(iterations)):
        label[...] = smooth_slices(label.astype(np.uint8), kernel_2d)
    return label


# ---- the sheet ------------------------------------------------------------------------------------------------
def read_sheet(data_xlsx: str) -> Dict[str, List[str]]:
    """The I/O sheet (D:40): columns ``image_path`` and ``label_path`` / ``zones_path``.  ``.xlsx`` through pandas.read_excel (needs
    openpyxl: its ImportError says so), ``.csv`` with the same columns through pandas.read_csv."""
    import pandas as pd
    if str(data_xlsx).lower().endswith(".csv"):
        data = pd.read_csv(data_xlsx)
    else:
        data = pd.read_excel(data_xlsx)
    if "image_path" not in data:
        raise KeyError(f"{data_xlsx}: no 'image_path' column (columns: {list(data.columns)})")
    return {c: [str(v) for v in data[c]] for c in COLUMNS if c in data}


def fold_sheet(prefix: str, f: int) -> str:
    """``prefix + str(f + 1) + '.xlsx'`` (train_model.py:143), or the ``.csv`` beside it when the ``.xlsx`` does not exist."""
    xlsx = prefix + str(f + 1) + ".xlsx"
    csv = prefix + str(f + 1) + ".csv"
    return csv if (not os.path.exists(xlsx) and os.path.exists(csv)) else xlsx


def _annotation(path: str) -> np.ndarray:
    """An annotation file as an integer array; integer-valued floats are accepted, anything else is a ValueError (what the reference
    does to a float between 1 and 2 is an accident of its two assignments and is not reproduced)."""
    a = np.load(path)
    if a.dtype == np.bool_:
        return a.astype(np.uint8)
    if np.issubdtype(a.dtype, np.integer):
        return a
    if np.issubdtype(a.dtype, np.floating) and np.all(np.isfinite(a)) and np.array_equal(a, np.rint(a)):
        return a.astype(np.int64)
    raise ValueError(f"{path}: annotations must be integer-valued (dtype {a.dtype})")


def _raw_sample(sheet, i: int, train_obj: str, mode: str) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """(image fp32 (D,H,W,C) as stored, raw annotation as uint8 (D,H,W) or None in 'test') of row ``i``.  Lesion grades saturate
    into uint8 (they are compared with 1 and 2 only); zones are taken ``astype(uint8)`` as the reference takes them (D:54)."""
    if train_obj not in ("zonal", "lesion"):
        raise ValueError(f"train_obj must be 'zonal' or 'lesion', got {train_obj!r}")
    image = np.load(sheet["image_path"][i]).astype(np.float32, copy=False)
    if mode == "test":
        return image, None
    a = _annotation(sheet["zones_path" if train_obj == "zonal" else "label_path"][i])
    a = a.astype(np.uint8) if train_obj == "zonal" else np.clip(a, 0, 255).astype(np.uint8)
    if a.shape != image.shape[:3]:
        raise ValueError(f"row {i}: annotation {a.shape} does not cover the image {image.shape[:3]}")
    return image, a


# ---- host generator -------------------------------------------------------------------------------------------
def custom_data_generator(data_xlsx, train_obj='zonal', probabilistic=False, mode='train') -> Iterator:
    """D:30-88 on the host: cycles over the sheet for ever and yields ``({"image": x}, {"detection": y[, "KL": 0]})``.  ``x`` is fp32
    (the posterior's label channels are appended in the image's type), ``y`` uint8 (the type the masks are smoothed in), ``KL`` fp32."""
    sheet = read_sheet(data_xlsx)
    n = len(sheet["image_path"])
    i = 0
    while True:
        if (i + 1) > n:
            i = 0
        image, a = _raw_sample(sheet, i, train_obj, mode)
        i += 1
        if a is None:
            a = np.zeros(image.shape[:3], dtype=np.uint8)
        if train_obj == 'zonal':
            image = image[:, :, :, :1]
            tz, pz = (a == 1).astype(np.uint8), (a == 2).astype(np.uint8)             # binarised independently (D:57-59)
            tz, pz = contour_smoothening(tz), contour_smoothening(pz)
            label = np.stack([np.ones_like(a) - tz - pz, tz, pz], axis=-1)            # uint8 arithmetic, as D:61
        else:
            lesions = contour_smoothening((a >= 2).astype(np.uint8))                  # D:69-71
            label = np.stack([np.ones_like(lesions) - lesions, lesions], axis=-1)
        postq_lbl = np.zeros_like(label)[:, :, :, 1:] if mode in ('test', 'valid') else label.copy()[:, :, :, 1:]
        if probabilistic:
            yield {"image": np.concatenate((image.copy(), postq_lbl.astype(image.dtype)), axis=-1)}, {
                "detection": label.copy(), "KL": np.zeros(shape=label.shape, dtype=np.float32)}
        else:
            yield {"image": image.copy()}, {"detection": label.copy()}


def batches(gen: Iterator, batch_size: int, device, rank: int = 0, world: int = 1) -> Iterator:
    """``train_model.batches``: ``dataset.batch(BATCH_SIZE)`` with this rank's shard, as dicts of device tensors."""
    from . import train_model
    return train_model.batches(gen, batch_size, device, rank, world)


# ---- device feed ----------------------------------------------------------------------------------------------
def device_batches(data_xlsx, train_obj='zonal', probabilistic=False, mode='train', batch_size: int = 1, device="cuda",
                   rank: int = 0, world: int = 1) -> Iterator:
    """The GPU feed: per batch, this rank's shard of raw images and uint8 annotations is uploaded and ops.prepare_labels writes the
    network input and the targets on the device.  Yields what ``batches(custom_data_generator(...), ...)`` yields, bit for bit."""
    sheet = read_sheet(data_xlsx)
    n = len(sheet["image_path"])
    mine = ddp.shard_batch(batch_size, rank, world)
    taps = gaussian_taps_u8(7, SIGMA)
    i = 0
    while True:
        rows = []
        for _ in range(batch_size):
            if (i + 1) > n:
                i = 0
            rows.append(i)
            i += 1
        raw = [_raw_sample(sheet, r, train_obj, mode) for r in rows[mine.start:mine.stop]]
        image = torch.from_numpy(np.stack([im for im, _ in raw])).to(device)
        ann = None if mode == "test" else torch.from_numpy(np.stack([a for _, a in raw])).to(device)
        x, det, kl = ops.prepare_labels(ann, image, train_obj, mode, bool(probabilistic), taps)
        yield {"image": x}, ({"detection": det, "KL": kl} if probabilistic else {"detection": det})
