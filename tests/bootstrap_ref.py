"""The bootstrap by explicit resampling (a helper, not a test module): the draw restated from tests/philox_ref.py, the resampled
case list built entry by entry, and the public host functions called on it -- ``detection.auroc``, ``detection.froc``,
``validation.sens_at``, ``detection.average_precision`` and ``np.nanmean``.  It shares no code with the packed, weighted formulation of
``bootstrap.replicates_host`` and csrc/bootstrap.hip; it is what both are held to.

The draw: key = seed + STREAM_ID * 0x9E3779B97F4A7C15 mod 2^64 (philox_ref.key); draw j of replicate b reads word
j & 3 of counter (b << 12) + (j >> 2); index = (word * N) >> 32 into the caller's case list.  Stratified over the positive cases pos
and the negative cases neg (both in the list's order): j < P draws pos[(word * P) >> 32], j >= P draws neg[(word * (N - P)) >> 32]."""
import warnings

import numpy as np

import philox_ref
from util import PKG

D, V = PKG.detection, PKG.validation
STREAM_ID = 0x424F4F54


def draw(N, b, seed, labels=None):
    """The N case indices (into the caller's list) replicate b draws.  ``labels`` makes the draw stratified."""
    ctr = (int(b) << 12) + np.arange((N + 3) // 4, dtype=np.uint64)
    word = [int(v) for v in philox_ref.words(seed, STREAM_ID, ctr).reshape(-1)[:N]]
    if labels is None:
        return [(w * N) >> 32 for w in word]
    pos, neg = [i for i in range(N) if labels[i]], [i for i in range(N) if not labels[i]]
    P = len(pos)
    return [pos[(w * P) >> 32] if j < P else neg[(w * (N - P)) >> 32] for j, w in enumerate(word)]


def metrics(labels, scores, results, values, fp_rates, picked):
    """One row [auroc, ap, sens@x..., nanmean of every value column] of the cases ``picked`` (a list of original indices, repeats
    allowed), from the public functions on the explicitly resampled list."""
    nan = float("nan")
    lab, sc, res = [labels[i] for i in picked], [scores[i] for i in picked], [results[i] for i in picked]
    try:
        auroc = D.auroc(lab, sc) if picked else nan
    except ValueError:
        auroc = nan
    curve = D.froc(res)
    row = [auroc, D.average_precision(res)]
    row += [V.sens_at(curve, x) if curve["num_lesions"] else nan for x in fp_rates]
    if values is not None:
        sel = np.asarray(values, np.float64)[picked]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)                # (a column of NaN only: nanmean warns and returns NaN)
            row += [float(np.nanmean(sel[:, v])) if len(picked) else nan for v in range(sel.shape[1])]
    return np.array(row, np.float64)


def replicates(cases, n_boot, seed=0, stratified=False, weights=None, fp_rates=(0.5, 1.0, 2.0), values=None):
    """(n_boot, S): the oracle.  ``cases``: dicts with "label", "confidence", "lesion_results"; ``weights`` (n_boot, N) replace the draw."""
    N = len(cases)
    labels, scores = [bool(c["label"]) for c in cases], [float(c["confidence"]) for c in cases]
    results = [c["lesion_results"] for c in cases]
    rows = []
    for b in range(n_boot):
        if weights is not None:
            picked = [i for i in range(N) for _ in range(int(weights[b][i]))]
        else:
            picked = draw(N, b, seed, labels if stratified else None)
        rows.append(metrics(labels, scores, results, values, fp_rates, picked))
    return np.stack(rows)


def synthetic_cases(N, seed, p_pos=0.5, max_fp=3, quant=8, mode="mixed"):
    """N cases in the form ``validation.validate`` gathers: about ``p_pos`` positive cases with 1 - 2 lesions each (one in five missed),
    0 .. ``max_fp`` false positives per case, every confidence a multiple of 1 / ``quant`` (heavy ties).  ``mode``: 'mixed'; 'all_tp'
    (no false positive, no miss), 'all_fp' (no lesion anywhere), 'missed' (lesions, all missed, no candidates), 'one_class' (every case
    positive)."""
    g = np.random.default_rng(seed)
    cases = []
    for _ in range(N):
        pos = bool(g.random() < p_pos) or mode == "one_class"
        if mode == "all_fp":
            pos = False
        res = []
        if pos:
            for _ in range(int(g.integers(1, 3))):
                missed = mode == "missed" or (mode != "all_tp" and g.random() < 0.2)
                c = 0.0 if missed else float(g.integers(quant // 2, quant + 1)) / quant
                res.append((1, c, 0.0 if missed else 0.5))
        if mode not in ("all_tp", "missed"):
            for _ in range(int(g.integers(0, max_fp + 1))):
                res.append((0, float(g.integers(1, quant)) / quant, 0.0))
        cases.append({"label": pos, "lesion_results": res, "confidence": max([r[1] for r in res], default=0.0)})
    return cases


def cases_with(N, M, seed, quant=8):
    """N cases, about half of them positive with one or two lesions each (N = 1: one positive case), holding exactly M events: event k
    falls on a random case and is a matched lesion (confidence 4/8 .. 8/8) while that case has an unmatched lesion left and a coin
    agrees, else a false positive (1/8 .. 7/8); the lesions left over are missed.  Confidences are multiples of 1 / ``quant``, so the
    tie groups of M >> quant events are hundreds of events long and straddle every thread, wave and chunk border."""
    g = np.random.default_rng([seed, N, M])
    pos = g.random(N) < 0.5
    pos[0] = True
    if N > 1:
        pos[1] = False
    left = np.where(pos, g.integers(1, 3, N), 0)
    res = [[] for _ in range(N)]
    where, coin = g.integers(0, N, M), g.random(M) < 0.6
    c_tp, c_fp = g.integers(quant // 2, quant + 1, M) / quant, g.integers(1, quant, M) / quant
    for k in range(M):
        i = int(where[k])
        if left[i] and coin[k]:
            left[i] -= 1
            res[i].append((1, float(c_tp[k]), 0.5))
        else:
            res[i].append((0, float(c_fp[k]), 0.0))
    for i in range(N):
        res[i] += [(1, 0.0, 0.0)] * int(left[i])
    return [{"label": bool(pos[i]), "lesion_results": res[i], "confidence": max([r[1] for r in res[i]], default=0.0)} for i in range(N)]


def value_columns(N, V, seed):
    """(N, V) per-case scalars in [0, 4): column 0 complete, every third column NaN in a fifth of the cases, the last of 16 all NaN."""
    g = np.random.default_rng([seed, N, V])
    vals = g.random((N, V)) * 4.0
    for v in range(1, V, 3):
        vals[g.random(N) < 0.2, v] = np.nan
    if V == 16:
        vals[:, 15] = np.nan
    return vals


def assert_rows(got, ref, table, W, what):
    """``got`` against ``ref`` ((n, S) replicates of ``table`` under the multiplicities ``W`` (n, N), packed case order): NaN in the same
    places; AUROC and the sensitivities bit-equal; AP and the means within 4 * n * 2^-53 of the sum of their |terms| -- the bound of any
    order of one fp64 sum of n terms (each order is within (n - 1) * 2^-53 of the exact sum, Higham, Accuracy and Stability, 4.2; the
    means' terms carry one more rounding each).  n and the sum of |terms| are computed here per replicate: for AP the event groups
    that add a matched lesion (every other group adds exactly 0) and AP itself (the terms are non-negative); for a mean the drawn cases
    with a value and the mean of |x| over them."""
    got, ref, W = np.asarray(got), np.asarray(ref), np.asarray(W, np.int64)
    Rn = len(table["fp_rates"])
    assert got.shape == ref.shape == (W.shape[0], 2 + Rn + table["V"]), (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, np.argwhere(np.isnan(got) != np.isnan(ref))[:5])
    for j in [0] + list(range(2, 2 + Rn)):
        assert np.array_equal(got[:, j], ref[:, j], equal_nan=True), (what, j, got[:, j], ref[:, j])
    ends, tp = np.flatnonzero(table["ev_group_end"]), table["ev_tp"] != 0
    worst = {}
    for b in range(W.shape[0]):
        if not np.isnan(ref[b, 1]):
            te = np.cumsum(np.where(tp, W[b][table["ev_case"]], 0))[ends]
            n = int((np.diff(np.r_[0, te]) > 0).sum())
            d, bound = abs(got[b, 1] - ref[b, 1]), 4.0 * n * 2.0 ** -53 * abs(ref[b, 1])
            worst["ap"] = max(worst.get("ap", 0.0), d)
            assert d <= bound, (what, "ap", b, got[b, 1], ref[b, 1], bound)
        for v in range(table["V"]):
            col, x = 2 + Rn + v, table["values"][:, v]
            if np.isnan(ref[b, col]):
                continue
            ok = ~np.isnan(x) & (W[b] > 0)
            n = int(W[b][ok].sum())
            mag = float((W[b][ok] * np.abs(x[ok])).sum()) / n
            d, bound = abs(got[b, col] - ref[b, col]), 4.0 * n * 2.0 ** -53 * mag
            worst[v] = max(worst.get(v, 0.0), d)
            assert d <= bound, (what, "mean", v, b, got[b, col], ref[b, col], bound)
    print(what, "largest |difference|", worst)
