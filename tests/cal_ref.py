"""An independent restatement of the calibration record (include/m1hip.h: m1_cal_score) for the tests: one Python loop over the voxels
that builds the record from the definitions, with Python's unbounded integers as accumulators.  It shares no code with
``calibration.reliability_host`` (vectorised numpy) and is used on the small shapes only (V <= 257)."""
import math

import numpy as np

F32 = np.float32
EPS = F32(1e-7)


def fx(v: float) -> int:
    """floor(max(v, 0) * 2^32) of a double."""
    v = float(v)
    return int(math.floor(v * 4294967296.0)) if v > 0.0 else 0


def bin_of(v, factor, M: int) -> int:
    """min(M - 1, (int)clip(v * factor, 0, M)): one fp32 multiply, then truncation."""
    prod = F32(F32(v) * F32(factor))
    prod = min(max(float(prod), 0.0), float(M))
    return min(M - 1, int(prod))


def record(prob, label, bins, mask=None, unc=None, u_max=None):
    """One record (a dict of Python ints and nested lists) per case of prob (B,...,K) fp32, label (B,...)."""
    p = np.asarray(prob, F32)
    B, K, M = p.shape[0], p.shape[-1], int(bins)
    p = p.reshape(B, -1, K)
    y = np.asarray(label).reshape(B, -1)
    m = None if mask is None else np.asarray(mask).reshape(B, -1)
    u = None if unc is None else np.asarray(unc, F32).reshape(B, -1)
    us = None if unc is None else F32(M / float(math.log(K) if u_max is None else u_max))
    out = []
    for b in range(B):
        z = lambda: [0] * M                                                # noqa: E731
        r = {"K": K, "M": M, "n_valid": 0, "n_invalid": 0, "n_ignored": 0, "nll": 0, "brier": [0] * K,
             "top_count": z(), "top_conf_sum": z(), "top_correct": z(),
             "cls_count": [z() for _ in range(K)], "cls_p_sum": [z() for _ in range(K)], "cls_pos": [z() for _ in range(K)],
             "unc_count": z(), "unc_u_sum": z(), "unc_errors": z()}
        for v in range(p.shape[1]):
            if m is not None and int(m[b, v]) == 0:
                continue
            pv = [F32(x) for x in p[b, v]]
            if any(math.isnan(float(x)) for x in pv) or (u is not None and math.isnan(float(u[b, v]))):
                r["n_invalid"] += 1
                continue
            yv = int(y[b, v])
            if yv >= K:
                r["n_ignored"] += 1
                continue
            r["n_valid"] += 1
            am = 0
            for c in range(1, K):
                if pv[c] > pv[am]:
                    am = c
            conf = pv[am]
            t = bin_of(conf, F32(M), M)
            r["top_count"][t] += 1
            r["top_conf_sum"][t] += fx(conf)
            r["top_correct"][t] += int(am == yv)
            for c in range(K):
                t = bin_of(pv[c], F32(M), M)
                r["cls_count"][c][t] += 1
                r["cls_p_sum"][c][t] += fx(pv[c])
                r["cls_pos"][c][t] += int(yv == c)
                d = float(pv[c]) - (1.0 if yv == c else 0.0)
                r["brier"][c] += fx(d * d)
            r["nll"] += fx(-np.log(np.float64(max(pv[yv], EPS))))
            if u is not None:
                uv = F32(u[b, v])
                t = bin_of(uv, us, M)
                r["unc_count"][t] += 1
                r["unc_u_sum"][t] += fx(max(float(uv), 0.0))
                r["unc_errors"][t] += int(am != yv)
        out.append(r)
    return out


def same(a: dict, b: dict, skip=()) -> list:
    """The keys in which two records (of this module, of reliability_host or of ops.read_cal_records) differ."""
    bad = []
    for k in a:
        if k in skip:
            continue
        if not np.array_equal(np.asarray(a[k]).astype(object), np.asarray(b[k]).astype(object)):
            bad.append(k)
    return bad


# ---- the small cases both test files score -----------------------------------------------------------------------------------------------
def as_bf16(a: np.ndarray) -> np.ndarray:
    """fp32 values rounded to bf16 (round to nearest even; NaN kept), still stored as fp32."""
    u = np.asarray(a, F32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    out = r.astype(np.uint32).view(F32).copy()
    out[np.isnan(a)] = np.nan
    return out


def case(B: int, V: int, K: int, content: str = "random", mask: bool = False, unc: bool = False, bf16: bool = False, seed: int = 0):
    """{"p" (B,V,K) fp32, "label" (B,V) uint8, "mask" (B,V) uint8 or None, "unc" (B,V) fp32 or None, "u_max"}.
    random     softmax of wide logits; p exactly 1.0, an exact tie, a few ignore labels (255); NaN at the first voxel, at the last
               voxel and at voxel 4 (the first of the second vector of four) of case 0; the mask random; unc = the entropy with the
               values 0, exactly u_max, above u_max, a negative one and a NaN put in
    onebin     every voxel p = (1, 0, ...), label 0: every lane of every wave in one bin
    alternate  p alternates voxel by voxel between two bins
    masked     random, case 0 entirely masked out (a mask is always given)
    ignored    random, the last case entirely labelled 255"""
    g = np.random.default_rng(1000 * V + 10 * K + B + seed)
    p = g.standard_normal((B, V, K)) * 2.5
    p = np.exp(p - p.max(-1, keepdims=True))
    p = (p / p.sum(-1, keepdims=True)).astype(F32)
    label = g.integers(0, K, (B, V)).astype(np.uint8)
    u_max = math.log(K)
    if content == "onebin":
        p[:] = 0
        p[..., 0] = 1
        label[:] = 0
        label[:, V // 2] = 1
    elif content == "alternate":
        lo, hi = F32(0.1 / (K - 1)), F32(0.9)
        p[:, 0::2] = [hi] + [lo] * (K - 1)
        p[:, 1::2] = [lo] * (K - 1) + [hi]
    else:
        p[0, 1] = [1.0] + [0.0] * (K - 1)
        p[0, 2] = [0.5, 0.5] + [0.0] * (K - 2)                              # a tie: the lowest class wins
        label[0, 2] = 1
        label[:, 7::31] = 255
        p[0, 0, K - 1] = p[0, V - 1, 0] = p[0, 4, 0] = np.nan
        if content == "ignored":
            label[B - 1] = 255
    if bf16:
        p = as_bf16(p)
    m = None
    if mask or content == "masked":
        m = (g.random((B, V)) < 0.8).astype(np.uint8) * g.integers(1, 256, (B, V)).astype(np.uint8)
        if content == "masked":
            m[0] = 0
    u = None
    if unc:
        with np.errstate(divide="ignore", invalid="ignore"):
            u = -(np.where(p > 0, p * np.log(p), 0)).sum(-1).astype(F32)
        u[np.isnan(u)] = 0.25
        u[:, 3], u[:, 5], u[:, 6], u[:, 8] = 0.0, F32(u_max), F32(3.0 * u_max), -0.5
        u[B - 1, 9] = np.nan
    return {"p": p, "label": label, "mask": m, "unc": u, "u_max": u_max if unc else None}
