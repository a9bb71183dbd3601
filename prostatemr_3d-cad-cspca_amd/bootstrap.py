"""Case-level bootstrap confidence intervals for what ``validation.validate`` reports: AUROC, lesion-level AP, the FROC sensitivities
and the per-case means (Dice, HD95, ASSD).  The csPCa literature reports a 95 % interval from 1000 or more case-level replicates;
nothing in the reference computes one, so nothing here restates reference code.

The scores never change between replicates, only the case multiplicities do.  ``pack`` therefore sorts once, on the host, and a
replicate is one draw, two weighted prefix scans and a few integer comparisons: ``ops.bootstrap_metrics`` (csrc/bootstrap.hip, one
workgroup per replicate, the multiplicities in LDS) computes all replicates in one launch; ``replicates_host`` is its numpy
restatement -- slow and exact: the same integers, the same fp64 expressions term by term, so AUROC and the sensitivities agree bit
for bit and AP and the means up to the order of one fp64 sum.  tests/bootstrap_ref.py resamples the case list explicitly and calls
``detection.auroc`` / ``froc`` / ``average_precision``, ``validation.sens_at`` and ``np.nanmean`` on it: the definition both are held to.

A replicate defines (``columns``):
  auroc        ``detection.auroc`` of the resampled cases; NaN without both classes of cases
  ap           ``detection.average_precision`` of the resampled cases; NaN without lesions
  sens@<x>fp   ``validation.sens_at(detection.froc(resampled), x)``; NaN without lesions (``sens_at`` itself reports 0 there: an
               interval over replicates must not mix 'no lesion drawn' into the sensitivities)
  <value>      the mean of a per-case scalar over the resampled cases that have one (NaN = none); NaN when no drawn case has one

The draw (restated from tests/philox_ref.py in tests/bootstrap_ref.py): Philox4x32-10 under the key
``seed + STREAM_ID * 0x9E3779B97F4A7C15 mod 2^64``; draw j of replicate b reads word ``j & 3`` of counter ``(b << 12) + (j >> 2)`` and
picks case ``(word * N) >> 32`` of the caller's list; stratified, draws j < P pick among the P positive cases (in the list's order),
``(word * P) >> 32``, the others among the negative ones, ``(word * (N - P)) >> 32``.  A replicate is a pure function of (seed, b):
the first 100 of 1000 replicates are the 100 of a shorter call, and two models scored on the same cases in the same order get the same
resamples (``paired_difference``)."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from .hip import lib as L
from .hip import ops

STREAM_ID = L.M1_STREAM_BOOTSTRAP
FP_RATES = (0.5, 1.0, 2.0)
MAX_CASES, MAX_BOOT, MAX_RATES, MAX_VALUES, MAX_WEIGHT = (L.M1_BOOTSTRAP_MAX_CASES, L.M1_BOOTSTRAP_MAX_BOOT, L.M1_BOOTSTRAP_MAX_RATES,
                                                          L.M1_BOOTSTRAP_MAX_VALUES, 65535)
_GOLDEN, _M64, _M32 = 0x9E3779B97F4A7C15, (1 << 64) - 1, 0xFFFFFFFF


# ---- the table ---------------------------------------------------------------------------------------------------------------------
def _group_end(sorted_keys: np.ndarray) -> np.ndarray:
    end = np.ones(sorted_keys.shape, np.uint8)
    if sorted_keys.size > 1:
        end[:-1] = sorted_keys[1:] != sorted_keys[:-1]
    return end


def pack(cases: Sequence[dict], train_obj: str = "lesion", fp_rates: Sequence[float] = FP_RATES, values=None,
         value_names: Optional[Sequence[str]] = None) -> dict:
    """The per-case list of ``validation.validate`` as plain numpy arrays, sorted once.

    'lesion': a case gives ``lesion_results`` and ``confidence`` (``detection.evaluate_case``) and its label ``record["n_true"][1] > 0``
    (or ``"label"`` where there is no record).  'zonal': ``dice`` / ``hd95`` / ``assd`` per class become the ``values`` columns; there
    are no scores, so auroc / ap / the sensitivities of such a table are NaN.  ``values`` (N, V) fp64 with V <= 16, NaN allowed:
    per-case scalars to average instead (``value_names`` names their columns).

    Case arrays, in ASCENDING score order (equal scores in their original order): ``case_label`` u8, ``case_group_end`` u8 (1 on the last
    case of a run of equal scores), ``case_perm`` (the original index), ``case_lesions`` i32 (lesions of the case, missed ones
    included: the recall denominator), ``values`` (N, V) in that order.  A draw's index names a case in the ORIGINAL order -- two models
    scored on the same cases get the same resamples -- and goes through ``case_rank`` i32 (the packed position of original case i), or,
    stratified, through ``strat_perm`` i32 (packed positions, the ``P`` positive cases first, each class in original order).  Event
    arrays -- unmatched candidates and matched lesions with confidence > 0 -- in DESCENDING confidence order: ``ev_case`` i32 (index
    into the case order), ``ev_tp`` u8, ``ev_group_end`` u8."""
    if train_obj not in ("lesion", "zonal"):
        raise ValueError(f"train_obj must be 'zonal' or 'lesion', got {train_obj!r}")
    cases = list(cases)
    N = len(cases)
    rates = tuple(float(x) for x in fp_rates)
    if len(rates) > MAX_RATES:
        raise ValueError(f"at most {MAX_RATES} false-positive rates, got {len(rates)}")
    if train_obj == "lesion":
        score = np.array([float(c["confidence"]) for c in cases], np.float64)
        label = np.array([bool(c["record"]["n_true"][1] > 0) if "record" in c else bool(c["label"]) for c in cases], bool)
        results = [list(c["lesion_results"]) for c in cases]
    else:
        score, label, results = np.zeros(N, np.float64), np.zeros(N, bool), [[] for _ in cases]
        if values is None and N:
            K1 = len(cases[0]["dice"])
            values = np.array([[c[k][j] for j in range(K1) for k in ("dice", "hd95", "assd")] for c in cases], np.float64)
            value_names = [f"{k}_c{j + 1}" for j in range(K1) for k in ("dice", "hd95", "assd")]
    if np.isnan(score).any():
        raise ValueError("a case confidence is NaN: the cases cannot be ranked")
    perm = np.argsort(score, kind="stable")
    rank = np.empty(N, np.int64)
    rank[perm] = np.arange(N)
    ev = [(float(c), rank[i], 1 if is_l else 0) for i, res in enumerate(results) for is_l, c, ov in res
          if float(c) > 0 and (not is_l or ov > 0)]
    conf = np.array([e[0] for e in ev], np.float64)
    order = np.argsort(-conf, kind="stable")
    if values is None:
        vals = np.zeros((N, 0), np.float64)
    else:
        vals = np.asarray(values, np.float64).reshape(N, -1)[perm]
    if vals.shape[1] > MAX_VALUES:
        raise ValueError(f"at most {MAX_VALUES} value columns, got {vals.shape[1]}")
    names = [f"value{v}" for v in range(vals.shape[1])] if value_names is None else [str(s) for s in value_names]
    if len(names) != vals.shape[1]:
        raise ValueError(f"{vals.shape[1]} value names expected, got {len(names)}")
    lab = label[perm]
    return {"N": N, "M": int(conf.size), "V": int(vals.shape[1]), "P": int(lab.sum()), "train_obj": train_obj, "fp_rates": rates,
            "case_label": lab.astype(np.uint8), "case_group_end": _group_end(score[perm]), "case_perm": perm.astype(np.int64),
            "case_lesions": np.array([sum(1 for is_l, _, _ in results[i] if is_l) for i in perm], np.int32).reshape(N),
            "ev_case": np.array([ev[k][1] for k in order], np.int32).reshape(-1),
            "ev_tp": np.array([ev[k][2] for k in order], np.uint8).reshape(-1), "ev_group_end": _group_end(conf[order]),
            "values": np.ascontiguousarray(vals), "value_names": names,
            "case_rank": rank.astype(np.int32),
            "strat_perm": rank[np.concatenate([np.flatnonzero(label), np.flatnonzero(~label)])].astype(np.int32)}


def columns(table: dict) -> list:
    """The names of the columns of ``replicates``."""
    return ["auroc", "ap"] + ["sens@%gfp" % x for x in table["fp_rates"]] + list(table["value_names"])


def to_device(table: dict, device) -> dict:
    """``table`` with its arrays resident on ``device`` under "dev" (``values`` transposed to (V, N): one row per scalar), for several
    ``replicates`` calls on one table."""
    dev = {k: torch.from_numpy(np.ascontiguousarray(table[k])).to(device)
           for k in ("case_label", "case_group_end", "case_lesions", "ev_case", "ev_tp", "ev_group_end", "case_rank", "strat_perm")}
    dev["values"] = torch.from_numpy(np.ascontiguousarray(table["values"].T)).to(device) if table["V"] else None
    dev["P"] = int(table["P"])
    return dict(table, dev=dev)


# ---- the draw ----------------------------------------------------------------------------------------------------------------------
def _philox_words(key: int, counter: np.ndarray) -> np.ndarray:
    """(n, 4) uint32: Philox4x32-10 of the 64-bit counters under the 64-bit key (csrc/common.h: philox4x32_10; words 2 and 3 of the
    counter are the fixed 0x243F6A88, 0x85A308D3)."""
    ctr = np.asarray(counter, np.uint64).reshape(-1)
    m32 = np.uint64(_M32)
    c = [ctr & m32, ctr >> np.uint64(32), np.full(ctr.shape, 0x243F6A88, np.uint64), np.full(ctr.shape, 0x85A308D3, np.uint64)]
    k0, k1 = key & _M32, (key >> 32) & _M32
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(0xD2511F53), c[2] * np.uint64(0xCD9E8D57)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return np.stack(c, axis=-1).astype(np.uint32)


def draw_indices(N: int, b: int, seed: int = 0, P: Optional[int] = None) -> np.ndarray:
    """The N indices replicate ``b`` draws (module docstring); ``P``: the stratified draw over P positives placed first."""
    N, b = int(N), int(b)
    if not 1 <= N <= MAX_CASES or not 0 <= b < MAX_BOOT:
        raise ValueError(f"1 <= N <= {MAX_CASES} and 0 <= b < {MAX_BOOT} expected, got N = {N}, b = {b}")
    key = (int(seed) + STREAM_ID * _GOLDEN) & _M64
    word = _philox_words(key, (b << 12) + np.arange((N + 3) // 4, dtype=np.uint64)).reshape(-1)[:N].astype(np.uint64)
    if P is None:
        return ((word * np.uint64(N)) >> np.uint64(32)).astype(np.int64)
    P = int(P)
    j = np.arange(N)
    return np.where(j < P, (word * np.uint64(P)) >> np.uint64(32), np.uint64(P) + ((word * np.uint64(N - P)) >> np.uint64(32))).astype(np.int64)


def draw_weights(table: dict, b: int, seed: int = 0, stratified: bool = False) -> np.ndarray:
    """How often replicate ``b`` draws every case, in the packed case order: int64 (N,)."""
    N = table["N"]
    if stratified:
        idx = table["strat_perm"][draw_indices(N, b, seed, table["P"])]
    else:
        idx = table["case_rank"][draw_indices(N, b, seed)]
    return np.bincount(idx, minlength=N).astype(np.int64)


def _check_weights(table: dict, n_boot: int, weights) -> np.ndarray:
    w = np.asarray(weights)
    if w.shape != (n_boot, table["N"]) or not np.issubdtype(w.dtype, np.integer):
        raise ValueError(f"weights must be integers of shape {(n_boot, table['N'])}, got {w.dtype} {w.shape}")
    if w.size and (w.min() < 0 or w.max() > MAX_WEIGHT):
        raise ValueError(f"weights must lie in [0, {MAX_WEIGHT}]")
    return np.ascontiguousarray(w[:, table["case_perm"]].astype(np.int32))     # (given per original case; the kernels read the packed order)


# ---- the replicates ----------------------------------------------------------------------------------------------------------------
def metrics_of_weights(table: dict, w: np.ndarray) -> np.ndarray:
    """One row of ``replicates`` from the multiplicities ``w`` (packed case order): the weighted formulation the kernel evaluates."""
    nan = float("nan")
    R, V = len(table["fp_rates"]), table["V"]
    out = np.full(2 + R + V, nan, np.float64)
    w = np.asarray(w, np.int64)
    lab = table["case_label"] != 0
    cp, cn = np.cumsum(np.where(lab, w, 0)), np.cumsum(np.where(lab, 0, w))
    Pw, Nw = (int(cp[-1]), int(cn[-1])) if w.size else (0, 0)
    if Pw and Nw:
        ge = np.flatnonzero(table["case_group_end"])
        pe, ne = cp[ge], cn[ge]
        two_u = int(((pe - np.r_[0, pe[:-1]]) * (np.r_[0, ne[:-1]] + ne)).sum())
        out[0] = float(two_u) / float(2 * Pw * Nw)
    Lw, Sw = int((w * table["case_lesions"].astype(np.int64)).sum()), Pw + Nw
    if Lw:
        we = w[table["ev_case"]]
        tp_ev = table["ev_tp"] != 0
        ge = np.flatnonzero(table["ev_group_end"])
        te, fe = np.cumsum(np.where(tp_ev, we, 0))[ge], np.cumsum(np.where(tp_ev, 0, we))[ge]
        prev = np.r_[0, te[:-1]].astype(np.int64)
        up = te > prev
        t64, f64 = te[up].astype(np.float64), fe[up].astype(np.float64)
        out[1] = float(np.sum((t64 / float(Lw) - prev[up].astype(np.float64) / float(Lw)) * (t64 / (t64 + f64))))
        fpc = fe.astype(np.float64) / float(Sw)
        for r, x in enumerate(table["fp_rates"]):
            ok = fpc <= float(x)
            out[2 + r] = float(te[ok].max()) / float(Lw) if ok.any() else 0.0
    for v in range(V):
        x = table["values"][:, v]
        ok = (w > 0) & ~np.isnan(x)
        c = int(w[ok].sum())
        if c:
            out[2 + R + v] = float(np.sum(w[ok].astype(np.float64) * x[ok])) / float(c)
    return out


def replicates_host(table: dict, n_boot: int, seed: int = 0, stratified: bool = False, weights=None) -> np.ndarray:
    """``replicates`` in numpy: one ``metrics_of_weights`` per replicate."""
    n_boot = _check_n_boot(table, n_boot)
    wp = None if weights is None else _check_weights(table, n_boot, weights)
    return np.stack([metrics_of_weights(table, draw_weights(table, b, seed, stratified) if wp is None else wp[b]) for b in range(n_boot)])


def _check_n_boot(table: dict, n_boot: int) -> int:
    n_boot = int(n_boot)
    if not 1 <= n_boot <= MAX_BOOT:
        raise ValueError(f"1 <= n_boot <= {MAX_BOOT} expected, got {n_boot}")
    if not 1 <= table["N"] <= MAX_CASES:
        raise ValueError(f"the bootstrap takes 1 .. {MAX_CASES} cases, got {table['N']}")
    return n_boot


def replicates(table: dict, n_boot: int, seed: int = 0, stratified: bool = False, weights=None, device=None) -> np.ndarray:
    """(n_boot, S) fp64 replicates of ``columns(table)``; NaN marks a statistic a replicate cannot define (module docstring).

    With a ``device`` (or a table from ``to_device``) this is ONE call of ``ops.bootstrap_metrics`` and one read of the result
    (1000 x 10 doubles are 80 kB); without, ``replicates_host``.  ``weights`` (n_boot, N) integers in [0, 65535], one column per case in
    the ORIGINAL case order, replace the draw with the caller's multiplicities: a jackknife (ones with one zero), a patient-clustered
    bootstrap, adversarial cases."""
    if device is None and "dev" not in table:
        return replicates_host(table, n_boot, seed, stratified, weights)
    n_boot = _check_n_boot(table, n_boot)
    t = table if "dev" in table else to_device(table, device)
    dev = t["dev"]
    wd = None if weights is None else torch.from_numpy(_check_weights(table, n_boot, weights)).to(dev["case_label"].device)
    with torch.no_grad():
        out = ops.bootstrap_metrics(dev, n_boot, seed, stratified, table["fp_rates"], wd)
    return out.cpu().numpy()


# ---- intervals ---------------------------------------------------------------------------------------------------------------------
def _percentiles(col: np.ndarray, level: float):
    ok = col[np.isfinite(col)]
    if not ok.size:
        return float("nan"), float("nan"), 0
    lo, hi = np.percentile(ok, [50.0 * (1.0 - level), 50.0 * (1.0 + level)])
    return float(lo), float(hi), int(ok.size)


def interval(reps, level: float = 0.95):
    """The percentile interval of every column over its finite replicates -> (lo, hi, n_valid), arrays of S entries (lo = hi = NaN
    and n_valid = 0 for a column without one)."""
    if not 0.0 < float(level) < 1.0:
        raise ValueError(f"0 < level < 1 expected, got {level}")
    reps = np.asarray(reps, np.float64)
    if reps.ndim != 2:
        raise ValueError(f"(n_boot, S) replicates expected, got {reps.shape}")
    rows = [_percentiles(reps[:, j], float(level)) for j in range(reps.shape[1])]
    return (np.array([r[0] for r in rows], np.float64), np.array([r[1] for r in rows], np.float64), np.array([r[2] for r in rows], np.int64))


def paired_difference(reps_a, reps_b, level: float = 0.95, tables=None) -> dict:
    """Two models scored on the SAME cases IN THE SAME ORDER with the same seed and n_boot get the same resamples, so their replicates
    are paired: per column the percentile interval of a - b over the replicates where both are finite (``lo``, ``hi``, ``n_valid``)
    and ``share_a_le_b``, the share of those replicates with a <= b (NaN without one).  ``tables`` = (table_a, table_b): checks that
    both hold the same number of cases with the same case labels in the original order -- the order itself cannot be checked."""
    a, b = np.asarray(reps_a, np.float64), np.asarray(reps_b, np.float64)
    if a.shape != b.shape or a.ndim != 2:
        raise ValueError(f"two (n_boot, S) arrays of one shape expected, got {a.shape} and {b.shape}")
    if tables is not None:
        ta, tb = tables
        if ta["N"] != tb["N"]:
            raise ValueError(f"paired replicates need the same cases: N = {ta['N']} and {tb['N']}")
        la, lb = np.empty(ta["N"], np.uint8), np.empty(tb["N"], np.uint8)
        la[ta["case_perm"]], lb[tb["case_perm"]] = ta["case_label"], tb["case_label"]
        if ta["train_obj"] == "lesion" and tb["train_obj"] == "lesion" and not np.array_equal(la, lb):
            raise ValueError("paired replicates need the same cases in the same order: the case labels differ")
    both = np.isfinite(a) & np.isfinite(b)
    d = np.where(both, a - b, np.nan)
    lo, hi, n = interval(d, level)
    with np.errstate(invalid="ignore", divide="ignore"):
        share = np.where(n > 0, ((a <= b) & both).sum(axis=0) / np.maximum(n, 1), np.nan)
    return {"lo": lo, "hi": hi, "n_valid": n, "share_a_le_b": share}
