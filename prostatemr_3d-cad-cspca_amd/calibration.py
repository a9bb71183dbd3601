"""Calibration of the predicted probabilities and of the uncertainty maps: does a voxel predicted at 0.8 turn out right eight times in
ten, and are the voxels with a high entropy / mutual information the voxels that are wrong?  No reference counterpart.

As ``detection`` and ``surface_distance``: numpy arrays run on the host (``reliability_host``), device tensors go through one kernel
(``ops.cal_score``, csrc/calibrate.hip) that leaves a small integer record per case.  Everything reported is plain host arithmetic on
that record, and the record of a data set is the slot-wise sum of its cases' records (``merge``).

The record (include/m1hip.h has the slot layout; here a dict).  With am = argmax of p (the lowest index among equals), conf = p[am],
y = label, M bins, ``fx(v) = floor(max(v, 0) as fp64 * 2^32)`` and ``bin(v) = min(M - 1, int(clip(fp32(v) * fp32(M), 0, M)))``:
  n_valid, n_invalid, n_ignored   voxels scored / with a NaN probability or a NaN uncertainty / with a label >= K (an ignore label);
                                  a voxel whose mask is 0 is counted nowhere; invalid is decided before ignored
  top_count, top_conf_sum, top_correct (M,)    at bin(conf): 1, fx(conf), am == y                       -> ECE, MCE
  cls_count, cls_p_sum, cls_pos (K, M)         at bin(p[c]): 1, fx(p[c]), y == c                        -> one-vs-rest reliability
  brier (K,)                                   fx((p[c] - (y == c))^2), the difference in fp64
  nll                                          fx(-log(max(p[y], 1e-7))), fp64 log of p as given (no renormalisation)
  unc_count, unc_u_sum, unc_errors (M,)        at min(M - 1, int(clip(u * fp32(M / u_max), 0, M))): 1, fx(max(u, 0)), am != y
All of it integers (Python ints and uint64 arrays): the sums do not depend on the order of the additions, so the kernel and
``reliability_host`` agree bit for bit -- except ``nll``, where the device's fp64 log may differ from numpy's in the last place (at
most one fixed-point unit per voxel).  ``u_max`` defaults to ln K, the largest entropy of K classes.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np

from .hip import lib as L

K_EPSILON = 1e-7
FX_ONE = float(2 ** 32)
INT_KEYS = ("n_valid", "n_invalid", "n_ignored", "nll")
ARRAY_KEYS = ("brier", "top_count", "top_conf_sum", "top_correct", "cls_count", "cls_p_sum", "cls_pos", "unc_count", "unc_u_sum",
              "unc_errors")
MIN_K, MAX_K, MAX_BINS, MAX_VOXELS = L.M1_CAL_MIN_K, L.M1_CAL_MAX_K, L.M1_CAL_MAX_BINS, L.M1_CAL_MAX_VOXELS     # the kernel's limits


def _is_tensor(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


def _check_km(K: int, M: int) -> None:
    if not (MIN_K <= K <= MAX_K) or not (1 <= M <= MAX_BINS):
        raise ValueError(f"K must be in {MIN_K}..{MAX_K} and bins in 1..{MAX_BINS}, got K = {K}, bins = {M}")


def u_scale(bins: int, u_max: float) -> np.float32:
    """float32(bins / u_max): the factor the uncertainty is multiplied with, in fp32, to find its bin -- the one definition, which
    ``ops.cal_score`` hands to the kernel.  ValueError unless ``u_max`` is positive and finite."""
    u = float(u_max)
    if not (u > 0.0 and math.isfinite(u)):
        raise ValueError(f"u_max must be positive and finite, got {u_max!r}")
    return np.float32(int(bins) / u)


def _fx(x) -> np.ndarray:
    return np.floor(np.maximum(np.asarray(x).astype(np.float64), 0.0) * FX_ONE).astype(np.uint64)


def _bins(v32: np.ndarray, factor: np.float32, M: int) -> np.ndarray:
    prod = v32.astype(np.float32) * np.float32(factor)                     # one fp32 multiply
    return np.minimum(M - 1, np.clip(prod, np.float32(0), np.float32(M)).astype(np.int64))


def _hist(bins: np.ndarray, M: int, sums: np.ndarray, hits: np.ndarray):
    count = np.bincount(bins, minlength=M).astype(np.uint64)
    hit = np.bincount(bins[hits], minlength=M).astype(np.uint64)
    s = np.zeros(M, np.uint64)
    np.add.at(s, bins, sums)
    return count, s, hit


def empty_record(K: int, M: int) -> dict:
    _check_km(K, M)
    z = lambda *s: np.zeros(s, np.uint64)                                  # noqa: E731
    return {"K": K, "M": M, "n_valid": 0, "n_invalid": 0, "n_ignored": 0, "nll": 0, "brier": z(K), "top_count": z(M),
            "top_conf_sum": z(M), "top_correct": z(M), "cls_count": z(K, M), "cls_p_sum": z(K, M), "cls_pos": z(K, M),
            "unc_count": z(M), "unc_u_sum": z(M), "unc_errors": z(M)}


# ---- the record ----------------------------------------------------------------------------------------------------------------
def reliability_host(prob, label, bins: int = 15, mask=None, uncertainty=None, u_max: Optional[float] = None) -> List[dict]:
    """The records of ``ops.cal_score`` in numpy with the same integer arithmetic: ``prob`` (B,...,K) taken as fp32, ``label`` (B,...)
    class indices in 0..255, ``mask`` (B,...) or None (0 skips the voxel), ``uncertainty`` (B,...) or None -> one dict per case."""
    p = np.asarray(prob, np.float32)
    B, K, M = int(p.shape[0]), int(p.shape[-1]), int(bins)
    _check_km(K, M)
    p = p.reshape(B, -1, K)
    V = p.shape[1]
    if not (1 <= V < MAX_VOXELS):
        raise ValueError(f"1 <= voxels per case < 2^27 expected, got {V}")
    y = np.asarray(label).reshape(B, -1).astype(np.int64)
    m = None if mask is None else np.asarray(mask).reshape(B, -1) != 0
    u = None if uncertainty is None else np.asarray(uncertainty, np.float32).reshape(B, -1)
    if y.shape[1] != V or (m is not None and m.shape[1] != V) or (u is not None and u.shape[1] != V):
        raise ValueError("label, mask and uncertainty must have the shape of prob without its last axis")
    us = None if u is None else u_scale(M, math.log(K) if u_max is None else u_max)
    out = []
    for b in range(B):
        keep = np.ones(V, bool) if m is None else m[b]
        nan = np.isnan(p[b]).any(axis=-1)
        if u is not None:
            nan |= np.isnan(u[b])
        ign = (y[b] >= K) | (y[b] < 0)
        valid = keep & ~nan & ~ign
        r = empty_record(K, M)
        r["n_invalid"], r["n_ignored"], r["n_valid"] = int((keep & nan).sum()), int((keep & ~nan & ign).sum()), int(valid.sum())
        pv, yv = p[b][valid], y[b][valid]
        am = np.argmax(pv, axis=-1) if len(pv) else np.zeros(0, np.int64)
        rows = np.arange(len(pv))
        conf = pv[rows, am]
        r["top_count"], r["top_conf_sum"], r["top_correct"] = _hist(_bins(conf, np.float32(M), M), M, _fx(conf), am == yv)
        for c in range(K):
            r["cls_count"][c], r["cls_p_sum"][c], r["cls_pos"][c] = _hist(_bins(pv[:, c], np.float32(M), M), M, _fx(pv[:, c]), yv == c)
            d = pv[:, c].astype(np.float64) - (yv == c)
            r["brier"][c] = _fx(d * d).sum(dtype=np.uint64)
        py = np.maximum(pv[rows, yv], np.float32(K_EPSILON)).astype(np.float64)
        r["nll"] = int(_fx(-np.log(py)).sum(dtype=np.uint64))
        if u is not None:
            uv = u[b][valid]
            r["unc_count"], r["unc_u_sum"], r["unc_errors"] = _hist(_bins(uv, us, M), M, _fx(np.maximum(uv, np.float32(0))), am != yv)
        out.append(r)
    return out


def reliability(prob, label, bins: int = 15, mask=None, uncertainty=None, u_max: Optional[float] = None) -> List[dict]:
    """Per-case calibration records.  Device tensors (``prob`` (B,...,K) fp32 or bf16, ``label`` / ``mask`` uint8, ``uncertainty``
    fp32) go through ``ops.cal_score`` and one host read; numpy arrays through ``reliability_host``.  ``u_max``: the upper end of
    the last uncertainty bin, ln K by default.  K outside 2..4, bins outside 1..64 and a ``u_max`` that is not positive and finite
    raise ValueError on both paths; what only the device path checks (dtypes, shapes, device) raises RuntimeError as every op does."""
    _check_km(int(prob.shape[-1]), int(bins))
    if not _is_tensor(prob):
        return reliability_host(prob, label, bins, mask, uncertainty, u_max)
    import torch
    from .hip import ops
    K = int(prob.shape[-1])
    with torch.no_grad():
        um = None if uncertainty is None else (math.log(K) if u_max is None else u_max)
        rec = ops.cal_score(prob.contiguous(), label.contiguous(), bins, None if mask is None else mask.contiguous(),
                            None if uncertainty is None else uncertainty.contiguous(), um)
    return ops.read_cal_records(rec, K, bins)


def merge(records: Sequence[dict]) -> dict:
    """The slot-wise integer sum: the record of the voxels of all ``records`` together."""
    records = list(records)
    if not records:
        raise ValueError("merge: no records")
    K, M = records[0]["K"], records[0]["M"]
    out = empty_record(K, M)
    for r in records:
        if (r["K"], r["M"]) != (K, M):
            raise ValueError("merge: records of different K or bins")
        for k in INT_KEYS:
            out[k] += int(r[k])
        for k in ARRAY_KEYS:
            out[k] = out[k] + np.asarray(r[k], np.uint64)
    return out


# ---- derived numbers -----------------------------------------------------------------------------------------------------------------
def _f(a) -> np.ndarray:
    return np.asarray(a, np.uint64).astype(np.float64)


def _curve(count, sums, hits):
    """(mean value, observed frequency, count) per bin; NaN in empty bins."""
    n, s, h = _f(count), _f(sums) / FX_ONE, _f(hits)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n > 0, s / n, np.nan), np.where(n > 0, h / n, np.nan), np.asarray(count, np.uint64).astype(np.int64)


def _gaps(count, sums, hits):
    """(weights n_b / N, |observed frequency - mean value|) over the non-empty bins."""
    mean, freq, n = _curve(count, sums, hits)
    ok = n > 0
    N = n.sum()
    return n[ok] / N if N else np.zeros(0), np.abs(freq[ok] - mean[ok])


def ece(rec: dict) -> float:
    """Expected calibration error of the arg-max label: sum_b n_b / N * |correct_b / n_b - conf_b / n_b| over the non-empty bins."""
    w, g = _gaps(rec["top_count"], rec["top_conf_sum"], rec["top_correct"])
    return float((w * g).sum()) if w.size else float("nan")


def mce(rec: dict) -> float:
    """Maximum calibration error: the largest gap of a non-empty bin."""
    _, g = _gaps(rec["top_count"], rec["top_conf_sum"], rec["top_correct"])
    return float(g.max()) if g.size else float("nan")


def classwise_ece(rec: dict, classes=None) -> float:
    """The mean over ``classes`` (all by default) of the ECE expression on the one-vs-rest histogram of each class."""
    cs = range(rec["K"]) if classes is None else list(classes)
    vals = []
    for c in cs:
        w, g = _gaps(rec["cls_count"][c], rec["cls_p_sum"][c], rec["cls_pos"][c])
        vals.append(float((w * g).sum()) if w.size else float("nan"))
    return float(np.mean(vals)) if vals else float("nan")


def brier(rec: dict) -> dict:
    """{"per_class": mean squared error of p[c] against (y == c) per class, "total": their sum} over the valid voxels."""
    N = rec["n_valid"]
    per = _f(rec["brier"]) / FX_ONE / N if N else np.full(rec["K"], np.nan)
    return {"per_class": [float(v) for v in per], "total": float(per.sum())}


def nll(rec: dict) -> float:
    """Mean negative log-likelihood of the true class (nats), p clipped at 1e-7 from below."""
    return int(rec["nll"]) / FX_ONE / rec["n_valid"] if rec["n_valid"] else float("nan")


def reliability_curve(rec: dict, cls: Optional[int] = None):
    """(mean confidence, observed frequency, count) per bin: of the arg-max label, or one-vs-rest of class ``cls``."""
    if cls is None:
        return _curve(rec["top_count"], rec["top_conf_sum"], rec["top_correct"])
    return _curve(rec["cls_count"][cls], rec["cls_p_sum"][cls], rec["cls_pos"][cls])


def uncertainty_error_curve(rec: dict):
    """(mean uncertainty, error rate, count) per uncertainty bin."""
    return _curve(rec["unc_count"], rec["unc_u_sum"], rec["unc_errors"])


def uncertainty_auroc(rec: dict) -> float:
    """The Mann-Whitney statistic of the uncertainty bin index as a detector of am != y: the chance that a wrong voxel sits in a
    higher bin than a right one, ties inside a bin counting 1/2.  NaN without errors or without correct voxels."""
    n = [int(v) for v in rec["unc_count"]]
    e = [int(v) for v in rec["unc_errors"]]
    E, C = sum(e), sum(n) - sum(e)
    if E == 0 or C == 0:
        return float("nan")
    twice, below = 0, 0                                                    # 2 U in whole numbers; correct voxels in lower bins
    for nb, eb in zip(n, e):
        twice += eb * (2 * below + (nb - eb))
        below += nb - eb
    return twice / (2 * E * C)


def referral_curve(rec: dict) -> dict:
    """Referring the most uncertain voxels first, bin by bin: entry j (0..M) refers the j highest bins.  "retained": fraction of the
    voxels kept, "error_rate": errors among the kept (NaN when none is kept), "errors_removed": fraction of all errors referred (NaN
    without errors)."""
    n = np.asarray(rec["unc_count"], np.uint64).astype(np.int64)
    e = np.asarray(rec["unc_errors"], np.uint64).astype(np.int64)
    N, E = int(n.sum()), int(e.sum())
    kept_n = np.concatenate([np.cumsum(n)[::-1], [0]]).astype(np.float64)
    kept_e = np.concatenate([np.cumsum(e)[::-1], [0]]).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return {"retained": kept_n / N if N else np.full(len(kept_n), np.nan),
                "error_rate": np.where(kept_n > 0, kept_e / kept_n, np.nan),
                "errors_removed": (E - kept_e) / E if E else np.full(len(kept_e), np.nan)}


def error_at_referral(curve: dict, fraction: float) -> float:
    """The error rate among the kept voxels at the first cut of ``referral_curve`` that refers at least ``fraction`` of the voxels
    -- the largest retained fraction not beyond 1 - fraction, the rule of ``validation.sens_at``; NaN when there is no such cut with
    a voxel kept (or no uncertainty histogram)."""
    kept = np.asarray(curve["retained"], np.float64)
    ok = np.nonzero(kept <= 1.0 - float(fraction))[0]
    return float(curve["error_rate"][ok[0]]) if ok.size else float("nan")
