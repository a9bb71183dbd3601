"""Surface-distance metrics of segmentations, in millimetres: Hausdorff distance (HD), percentile Hausdorff distance (HD95), average
symmetric surface distance (ASSD) and normalised surface Dice (NSD), next to a hard Dice per class -- what a zonal (or any lesion)
segmentation is judged on.  The reference's ``train_model.py`` imports an ``AnatomySegmentationValidation`` callback that was never
published, so nothing here restates reference code; the definitions below are this module's contract and are PINNED against
``scipy.ndimage`` (``binary_erosion``, ``distance_transform_edt`` with ``sampling``) and ``np.percentile`` in
tests/test_surface_distance_host.py.  Parity with medpy, MONAI and DeepMind's ``surface_distance`` is NOT pinned: none of them is a
dependency here.

Inputs: ``pred`` and ``truth`` are integer label maps (B,D,H,W) or (D,H,W), uint8 or int32; ``labels`` is a tuple of K class ids,
1 <= K <= 8; ``spacing`` is three positive numbers in ARRAY-AXIS order (D,H,W), in mm.  A binary mask is the case ``labels=(1,)``;
the argmax or the threshold of a softmax stays with the caller.  Every (b, k) pair is independent.  For one pair let
A = (pred == labels[k]) and B = (truth == labels[k]).

  border(M)   the voxels of M with at least one of their six face neighbours outside M, where outside the volume counts as
              background (mask voxels on a volume face are border voxels):
              ``M & ~binary_erosion(M, generate_binary_structure(3, 1), border_value=0)``.
  dist_M(x)   the distance of voxel x to the nearest border voxel of M, the exact minimum of sqrt(sum_i (spacing_i * delta_i)^2):
              ``distance_transform_edt(~border(M), sampling=spacing)[x]``, formed in fp64 and stored as fp32.
  d_AB        the multiset {dist_B(a) : a in border(A)}; d_BA the same with the roles swapped.

Per (b, k), as a dict of (B,K) results ((K,) for a (D,H,W) input; ``nsd`` has a last axis of T tolerances):

  n_pred, n_truth              |border(A)|, |border(B)|, int64
  vol_pred, vol_truth, vol_both  |A|, |B|, |A and B|, int64; dice = 2 vol_both / (vol_pred + vol_truth), NaN when both are empty
  hd_ab, hd_ba, hd             max d_AB, max d_BA and the larger of the two
  mean_ab, mean_ba, assd       the directed means (fp64 sums) and (mean_ab + mean_ba) / 2 -- medpy's definition of ASSD
  hdq_ab, hdq_ba, hdq          the ``percentile``-th percentile of d_AB, of d_BA, and of the POOLED multiset d_AB + d_BA (medpy's hd95
                               at 95; max(hdq_ab, hdq_ba) is the other definition in use).  numpy's linear rule: with the n values
                               sorted, h = (n - 1) * q / 100 in fp64, lo = floor(h), a[lo] + (h - lo) * (a[min(lo + 1, n - 1)] - a[lo])
                               in fp64, rounded once to fp32
  nsd[t]                       (#{d_AB <= tau_t} + #{d_BA <= tau_t}) / (n_pred + n_truth) for up to four tolerances tau_t per call
                               (compared as fp32) -- the voxel-count form of the surface Dice

Empty sets: when A or B is empty every distance result of that (b, k) is NaN (a distance transform without a feature voxel means
nothing) and so is nsd, except that nsd is 1 when BOTH are empty; the counts stay exact.  Nothing raises, and the host reads nothing.

numpy arrays go through the ``*_host`` restatements below (numpy alone); device tensors go through csrc/surface.hip
(ops.sd_border / sd_distance / sd_metrics) and come back as device tensors: nothing is read back.  The kernels hold a line of at most
256 voxels: a device volume with a longer axis raises.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from .hip import ops

COUNT_KEYS = ops.SD_COUNT_KEYS
FLOAT_KEYS = ("dice", "hd", "hd_ab", "hd_ba", "assd", "mean_ab", "mean_ba", "hdq", "hdq_ab", "hdq_ba")
MAX_CLASSES, MAX_TOLERANCES = 8, 4


# ---- host restatements -------------------------------------------------------------------------------------------------------
def _spacing(spacing) -> tuple:
    s = tuple(float(v) for v in spacing)
    if len(s) != 3 or not all(np.isfinite(v) and v > 0 for v in s):
        raise ValueError(f"spacing must be three positive numbers in (D,H,W) order, got {spacing!r}")
    return s


def _labels(labels) -> tuple:
    labels = tuple(int(v) for v in labels)
    if not 1 <= len(labels) <= MAX_CLASSES:
        raise ValueError(f"1..{MAX_CLASSES} class ids expected, got {len(labels)}")
    return labels


def _tolerances(tolerances) -> tuple:
    tolerances = tuple(float(v) for v in tolerances)
    if len(tolerances) > MAX_TOLERANCES or any(np.isnan(v) for v in tolerances):
        raise ValueError(f"at most {MAX_TOLERANCES} tolerances per call, none of them NaN, got {tolerances!r}")
    return tolerances


def _percentile_arg(q) -> float:
    q = float(q)
    if not 0.0 <= q <= 100.0:
        raise ValueError(f"a percentile in [0, 100] expected, got {q!r}")
    return q


def _border_of(m: np.ndarray) -> np.ndarray:
    """border(M) of a boolean array over its last three axes."""
    interior = m.copy()
    for ax in (-3, -2, -1):
        a = np.moveaxis(m, ax, -1)
        both = np.zeros_like(a)
        both[..., 1:-1] = a[..., :-2] & a[..., 2:]          # both neighbours along the axis inside the volume and in the mask
        interior &= np.moveaxis(both, -1, ax)
    return m & ~interior


def mask_border_host(mask: np.ndarray) -> np.ndarray:
    """border(mask == 1) of a (D,H,W) or (B,D,H,W) array, boolean."""
    m = np.asarray(mask)
    if m.ndim not in (3, 4):
        raise ValueError(f"a (D,H,W) or (B,D,H,W) mask expected, got {m.shape}")
    return _border_of(m == 1)


def _min_pass(f: np.ndarray, axis: int, s: float) -> np.ndarray:
    """f_out(x) = min_y ((s * (x - y))^2 + f(y)) along ``axis`` in fp64, +inf meaning no feature on the line."""
    f = np.moveaxis(f, axis, 0)
    n = f.shape[0]
    x = np.arange(n, dtype=np.float64).reshape((n,) + (1,) * (f.ndim - 1))
    out = np.full(f.shape, np.inf)
    for y in range(n):
        if np.isfinite(f[y]).any():
            t = s * (x - float(y))
            np.minimum(out, t * t + f[y][None], out=out)
    return np.moveaxis(out, 0, axis)


def edt_host(feature: np.ndarray, spacing=(1.0, 1.0, 1.0)) -> np.ndarray:
    """The exact Euclidean distance (fp64, stored as fp32) of every voxel to the nearest True voxel of ``feature`` over its last three
    axes, by the three separable passes of csrc/surface.hip (W, then H, then D); +inf in a volume without a True voxel."""
    s = _spacing(spacing)
    f = np.asarray(feature) != 0
    w = f.shape[-1]
    idx = np.arange(w)
    left = np.maximum.accumulate(np.where(f, idx, -1), axis=-1)                              # the nearest feature at or below x
    right = np.minimum.accumulate(np.where(f, idx, 2 * w)[..., ::-1], axis=-1)[..., ::-1]     # ... at or above x
    d = np.minimum(np.where(left >= 0, idx - left, 2 * w), np.where(right < 2 * w, right - idx, 2 * w))
    t = s[2] * d.astype(np.float64)
    g = np.where(d < 2 * w, t * t, np.inf)
    g = _min_pass(g, -2, s[1])
    g = _min_pass(g, -3, s[0])
    return np.sqrt(g).astype(np.float32)


def distance_to_border_host(mask: np.ndarray, spacing=(1.0, 1.0, 1.0)) -> np.ndarray:
    """dist_M of M = (mask == 1) for a (D,H,W) or (B,D,H,W) array, fp32."""
    return edt_host(mask_border_host(mask), spacing)


def percentile_host(values: np.ndarray, q: float) -> np.float32:
    """The module's percentile rule on a 1-D fp32 array (NaN when it is empty)."""
    a = np.sort(np.asarray(values, np.float32)).astype(np.float64)
    n = a.size
    if n == 0:
        return np.float32(np.nan)
    h = (float(n - 1) * float(q)) / 100.0
    lo = min(max(int(np.floor(h)), 0), n - 1)
    with np.errstate(invalid="ignore"):
        return np.float32(a[lo] + (h - lo) * (a[min(lo + 1, n - 1)] - a[lo]))


def surface_metrics_host(pred: np.ndarray, truth: np.ndarray, labels: Sequence[int] = (1,), spacing=(1.0, 1.0, 1.0),
                         percentile: float = 95.0, tolerances: Sequence[float] = ()) -> dict:
    """``surface_metrics`` for numpy arrays, with numpy alone (the module docstring has the definitions)."""
    pred, truth = np.asarray(pred), np.asarray(truth)
    if pred.shape != truth.shape or pred.ndim not in (3, 4):
        raise ValueError(f"two (D,H,W) or (B,D,H,W) label maps of one shape expected, got {pred.shape} and {truth.shape}")
    labels, spacing, tol, q = _labels(labels), _spacing(spacing), _tolerances(tolerances), _percentile_arg(percentile)
    squeeze = pred.ndim == 3
    if squeeze:
        pred, truth = pred[None], truth[None]
    B, K, T = pred.shape[0], len(labels), len(tol)
    out = {k: np.zeros((B, K), np.int64) for k in COUNT_KEYS}
    out.update({k: np.full((B, K), np.nan, np.float32) for k in FLOAT_KEYS})
    out["nsd"] = np.full((B, K, T), np.nan, np.float32)
    a = np.stack([pred == l for l in labels], axis=1)                   # (B,K,D,H,W)
    b = np.stack([truth == l for l in labels], axis=1)
    ba, bb = _border_of(a), _border_of(b)
    da, db = edt_host(ba, spacing), edt_host(bb, spacing)
    for i in range(B):
        for k in range(K):
            d_ab, d_ba = db[i, k][ba[i, k]], da[i, k][bb[i, k]]
            n0, n1 = d_ab.size, d_ba.size
            vp, vt, vb = int(a[i, k].sum()), int(b[i, k].sum()), int((a[i, k] & b[i, k]).sum())
            for key, v in zip(COUNT_KEYS, (n0, n1, vp, vt, vb)):
                out[key][i, k] = v
            if vp + vt > 0:
                out["dice"][i, k] = np.float32(2.0 * vb / (vp + vt))
            if n0 == 0 and n1 == 0:
                out["nsd"][i, k] = 1.0
            if n0 == 0 or n1 == 0:
                continue
            m0, m1 = d_ab.astype(np.float64).sum() / n0, d_ba.astype(np.float64).sum() / n1
            out["hd_ab"][i, k], out["hd_ba"][i, k] = d_ab.max(), d_ba.max()
            out["hd"][i, k] = max(d_ab.max(), d_ba.max())
            out["mean_ab"][i, k], out["mean_ba"][i, k], out["assd"][i, k] = m0, m1, (m0 + m1) / 2.0
            out["hdq_ab"][i, k], out["hdq_ba"][i, k] = percentile_host(d_ab, q), percentile_host(d_ba, q)
            out["hdq"][i, k] = percentile_host(np.concatenate([d_ab, d_ba]), q)
            for t, tau in enumerate(tol):
                le = int((d_ab <= np.float32(tau)).sum()) + int((d_ba <= np.float32(tau)).sum())
                out["nsd"][i, k, t] = np.float32(le / (n0 + n1))
    return {k: v[0] for k, v in out.items()} if squeeze else out


# ---- public surface ----------------------------------------------------------------------------------------------------------
def _is_host(x) -> bool:
    return not isinstance(x, torch.Tensor)


def _device_maps(pred: torch.Tensor, truth: torch.Tensor):
    if not isinstance(truth, torch.Tensor) or pred.shape != truth.shape or pred.dim() not in (3, 4):
        raise ValueError("two device label maps (D,H,W) or (B,D,H,W) of one shape expected")
    squeeze = pred.dim() == 3
    if pred.dtype == torch.bool:
        pred = pred.view(torch.uint8)
    if truth.dtype == torch.bool:
        truth = truth.view(torch.uint8)
    return (pred[None], truth[None], True) if squeeze else (pred, truth, False)


def mask_border(mask):
    """border(mask == 1) of a (D,H,W) or (B,D,H,W) mask: a boolean numpy array for a numpy array, a uint8 device tensor of 0 / 1 for a
    device tensor (bool, uint8 or int32)."""
    if _is_host(mask):
        return mask_border_host(mask)
    m, _, squeeze = _device_maps(mask, mask)
    borders, _ = ops.sd_border(m, m, (1,))
    return borders[0, 0, 0] if squeeze else borders[0, :, 0]


def distance_to_border(mask, spacing=(1.0, 1.0, 1.0)):
    """dist_M of M = (mask == 1): the distance in mm of every voxel to the nearest border voxel of the mask, fp32, ``spacing`` in
    (D,H,W) order; +inf where the mask is empty."""
    if _is_host(mask):
        return distance_to_border_host(mask, spacing)
    b = mask_border(mask)
    d = ops.sd_distance(b if b.dim() == 4 else b[None], _spacing(spacing))
    return d if b.dim() == 4 else d[0]


def surface_metrics(pred, truth, labels: Sequence[int] = (1,), spacing=(1.0, 1.0, 1.0), percentile: float = 95.0,
                    tolerances: Sequence[float] = ()) -> dict:
    """Every metric of the module docstring for K classes at once -> dict of (B,K) results (``nsd``: (B,K,T)); numpy in, numpy out;
    device tensors in, device tensors out (three stages of kernels, nothing read back)."""
    if _is_host(pred):
        return surface_metrics_host(pred, truth, labels, spacing, percentile, tolerances)
    pred, truth, squeeze = _device_maps(pred, truth)
    labels, spacing, tol, q = _labels(labels), _spacing(spacing), _tolerances(tolerances), _percentile_arg(percentile)
    borders, counts = ops.sd_border(pred, truth, labels)
    dist = ops.sd_distance(borders.view(-1, *borders.shape[3:]), spacing).view(borders.shape)
    m = ops.sd_metrics(borders, dist, counts, q, tol)
    out = {key: counts[..., j] for j, key in enumerate(COUNT_KEYS)}
    out.update({key: m[key] for key in FLOAT_KEYS + ("nsd",)})
    return {k: v[0] for k, v in out.items()} if squeeze else out


def hausdorff(pred, truth, labels: Sequence[int] = (1,), spacing=(1.0, 1.0, 1.0)):
    """The symmetric Hausdorff distance per (b, k)."""
    return surface_metrics(pred, truth, labels, spacing)["hd"]


def hausdorff_percentile(pred, truth, labels: Sequence[int] = (1,), spacing=(1.0, 1.0, 1.0), percentile: float = 95.0):
    """The ``percentile``-th percentile of the pooled surface distances per (b, k) (medpy's hd95 at 95)."""
    return surface_metrics(pred, truth, labels, spacing, percentile)["hdq"]


def assd(pred, truth, labels: Sequence[int] = (1,), spacing=(1.0, 1.0, 1.0)):
    """The average symmetric surface distance per (b, k)."""
    return surface_metrics(pred, truth, labels, spacing)["assd"]


def nsd(pred, truth, tolerance: float, labels: Sequence[int] = (1,), spacing=(1.0, 1.0, 1.0)):
    """The normalised surface Dice at one tolerance (mm) per (b, k)."""
    return surface_metrics(pred, truth, labels, spacing, tolerances=(tolerance,))["nsd"][..., 0]


def dice_per_class(pred, truth, labels: Sequence[int] = (1,)):
    """The hard Dice 2 |A and B| / (|A| + |B|) per (b, k), NaN where both are empty.  On the device the voxels are counted by the
    border kernel; the division of the (B,K) table is a tensor expression (0 / 0 is the NaN)."""
    if _is_host(pred):
        return _dice_host(pred, truth, labels)
    pred, truth, squeeze = _device_maps(pred, truth)
    _, counts = ops.sd_border(pred, truth, _labels(labels))
    dice = (2.0 * counts[..., 4].double() / (counts[..., 2] + counts[..., 3]).double()).float()
    return dice[0] if squeeze else dice


def _dice_host(pred, truth, labels) -> np.ndarray:
    pred, truth = np.asarray(pred), np.asarray(truth)
    ax = (-3, -2, -1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.stack([(2.0 * ((pred == l) & (truth == l)).sum(ax) / ((pred == l).sum(ax) + (truth == l).sum(ax))) for l in _labels(labels)],
                        axis=-1).astype(np.float32)
