"""Lesion candidates, their matching to annotated lesions, FROC and case-level AUROC: what a csPCa detection model is judged on.

The reference's ``train_model.py`` imports ``regionprops`` and its ``callbacks.py`` imports ``compute_FROC`` from a ``deploy_FROC``
module that was never published, so nothing here restates reference code except ``dice_3d`` (callbacks.py:36-40).  The compute
underneath is 3D connected-component labelling:

  * ``label_components`` / ``component_stats`` / ``component_overlap``: numpy arrays go through the ``*_host`` restatements below
    (numpy only), device tensors through csrc/components.hip (ops.label_components & co.).  The numbering of the components --
    1..K in raster order of each component's first voxel -- and the table columns are PINNED against ``scipy.ndimage.label``,
    ``find_objects``, ``maximum``, ``maximum_position`` and ``sum`` in tests/test_detection_host.py; the kernels are compared with
    the restatements exactly.  Everything is an integer or an exact maximum: no tolerance exists anywhere.
  * ``auroc`` is pinned against ``sklearn.metrics.roc_auc_score`` where sklearn is installed.

NOT pinned, and this project's own definitions (as ``data_generators.py`` says of its unpinned cv2 rule): the dynamic extraction rule,
the candidate / lesion matching and the FROC curve.  They follow what the field's evaluation tools (picai_eval,
report_guided_annotation) describe, neither of which is a dependency here, and are stated in full in the functions' docstrings so
that a later pin changes one function.

Batches: every volume function takes (D,H,W) or (B,D,H,W); batch entries are independent and each numbers its components from 1.
A device tensor in means device tensors out, and no function reads device memory back to the host inside a loop:
``extract_lesion_candidates(threshold='dynamic')`` is ``num_lesions_to_extract`` rounds of peak -> label -> select -> take on the whole
batch with its state in device memory.  The fixed-threshold path and ``evaluate_case`` read the component counts once, to size
their tables.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .hip import ops

STAT_KEYS = ("count", "max", "argmax", "lo", "hi", "sum")


# ---- host restatements -------------------------------------------------------------------------------------------------------
def _backward_offsets(connectivity: int):
    """The half of the 6- / 18- / 26-neighbourhood that precedes a voxel in raster order (13 offsets at connectivity 3)."""
    if connectivity not in (1, 2, 3):
        raise ValueError(f"connectivity must be 1, 2 or 3, got {connectivity!r}")
    return [(dz, dy, dx) for dz in (-1, 0) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if (dz, dy, dx) < (0, 0, 0) and (dz != 0) + (dy != 0) + (dx != 0) <= connectivity]


def _label_one(mask: np.ndarray, connectivity: int) -> Tuple[np.ndarray, int]:
    D, H, W = mask.shape
    idx = np.arange(mask.size, dtype=np.int64).reshape(mask.shape)
    us, vs = [], []
    for dz, dy, dx in _backward_offsets(connectivity):
        # voxel (z, y, x) with its neighbour (z + dz, y + dy, x + dx): both inside the volume, hence nothing wraps around a row end
        a = (slice(-dz, D), slice(max(-dy, 0), H - max(dy, 0)), slice(max(-dx, 0), W - max(dx, 0)))
        b = (slice(0, D + dz), slice(max(dy, 0), H + min(dy, 0)), slice(max(dx, 0), W + min(dx, 0)))
        both = mask[a] & mask[b]
        us.append(idx[a][both])
        vs.append(idx[b][both])
    u, v = np.concatenate(us), np.concatenate(vs)
    parent = np.arange(mask.size, dtype=np.int64)
    while u.size:
        pu, pv = parent[u], parent[v]
        low = np.minimum(pu, pv)
        before = parent.copy()
        np.minimum.at(parent, pu, low)                      # hook the larger root under the smaller
        np.minimum.at(parent, pv, low)
        while True:                                         # pointer jumping until every voxel points at a root
            jumped = parent[parent]
            if np.array_equal(jumped, parent):
                break
            parent = jumped
        if np.array_equal(parent, before):
            break
    flat = mask.reshape(-1)
    # parent <= own index always, so a component's root is its smallest linear index; its rank among the roots is its number
    roots = np.flatnonzero(flat & (parent == np.arange(mask.size)))
    labels = np.zeros(mask.size, np.int32)
    labels[flat] = (np.searchsorted(roots, parent[flat]) + 1).astype(np.int32)
    return labels.reshape(mask.shape), int(roots.size)


def label_components_host(mask: np.ndarray, connectivity: int = 3):
    """The connected components of the non-zero voxels of ``mask`` ((D,H,W) -> (labels int32, K); (B,D,H,W) -> (labels, counts (B,)
    int32)), numbered 1..K per batch entry in raster order of each component's first voxel: ``scipy.ndimage.label`` with
    ``generate_binary_structure(3, connectivity)``, by vectorised union-find (hook to the smaller root, pointer jumping)."""
    m = np.asarray(mask) != 0
    if m.ndim == 3:
        return _label_one(m, connectivity)
    if m.ndim != 4:
        raise ValueError(f"a (D,H,W) or (B,D,H,W) mask expected, got {m.shape}")
    out = [_label_one(mb, connectivity) for mb in m]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32)


def _stats_one(labels: np.ndarray, values: Optional[np.ndarray], K: int) -> dict:
    D, H, W = labels.shape
    flat = labels.reshape(-1)
    vox = np.flatnonzero((flat > 0) & (flat <= K))
    row = flat[vox].astype(np.int64) - 1
    val = np.zeros(vox.size, np.float32) if values is None else np.asarray(values, np.float32).reshape(-1)[vox] + np.float32(0)
    coords = np.stack(np.unravel_index(vox, (D, H, W)), axis=1).astype(np.int64) if vox.size else np.zeros((0, 3), np.int64)
    out = {"count": np.bincount(row, minlength=K).astype(np.int32), "max": np.zeros(K, np.float32), "argmax": np.zeros(K, np.int64),
           "lo": np.zeros((K, 3), np.int32), "hi": np.zeros((K, 3), np.int32), "sum": np.zeros((K, 3), np.int64)}
    if vox.size:
        order = np.lexsort((vox, -val.astype(np.float64), row))             # per row: the largest value first, then the smallest index
        first = order[np.r_[True, row[order][1:] != row[order][:-1]]]
        out["max"][row[first]] = val[first]
        out["argmax"][row[first]] = vox[first]
        lo = np.full((K, 3), np.iinfo(np.int64).max, np.int64)
        hi = np.zeros((K, 3), np.int64)
        np.minimum.at(lo, row, coords)
        np.maximum.at(hi, row, coords + 1)
        np.add.at(out["sum"], row, coords)
        present = out["count"] > 0
        out["lo"][present] = lo[present]
        out["hi"][present] = hi[present]
    return out


def component_stats_host(labels: np.ndarray, values: Optional[np.ndarray] = None, max_components: int = 64) -> dict:
    """The per-component table of a label volume, K = ``max_components`` rows per batch entry (row l - 1 for label l; larger labels
    have no row, rows of absent labels are zero): ``count``; ``max`` (fp32) and ``argmax`` (linear index inside the batch entry, ties
    to the smallest) of ``values``, 0 and the component's first voxel without values; ``lo`` / ``hi`` the bounding box per axis, hi
    exclusive as ``scipy.ndimage.find_objects``; ``sum`` the int64 coordinate sums (centroid = sum / count)."""
    lab = np.asarray(labels)
    K = int(max_components)
    if K < 1:
        raise ValueError("max_components must be positive")
    if lab.ndim == 3:
        return _stats_one(lab, values, K)
    if lab.ndim != 4:
        raise ValueError(f"a (D,H,W) or (B,D,H,W) label volume expected, got {lab.shape}")
    per = [_stats_one(lab[b], None if values is None else np.asarray(values)[b], K) for b in range(lab.shape[0])]
    return {k: np.stack([p[k] for p in per]) for k in STAT_KEYS}


def overlap_host(a: np.ndarray, b: np.ndarray, max_a: int, max_b: int) -> np.ndarray:
    """The contingency table of two label volumes: ((B,) max_a + 1, max_b + 1) int32 counts of the voxels labelled (i, j); row and
    column 0 are background; a voxel whose label is negative or above its cap is counted nowhere."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.ndim not in (3, 4):
        raise ValueError(f"two label volumes of one shape expected, got {a.shape} and {b.shape}")
    if a.ndim == 4:
        return np.stack([overlap_host(x, y, max_a, max_b) for x, y in zip(a, b)])
    fa, fb = a.reshape(-1).astype(np.int64), b.reshape(-1).astype(np.int64)
    ok = (fa >= 0) & (fa <= max_a) & (fb >= 0) & (fb <= max_b)
    cells = np.bincount(fa[ok] * (max_b + 1) + fb[ok], minlength=(max_a + 1) * (max_b + 1))
    return cells.reshape(max_a + 1, max_b + 1).astype(np.int32)


# ---- both paths --------------------------------------------------------------------------------------------------------------
def _batched(t):
    """(the (B,D,H,W) view, whether a batch axis was added)"""
    if t.ndim == 3:
        return t[None], True
    if t.ndim != 4:
        raise ValueError(f"a (D,H,W) or (B,D,H,W) volume expected, got {tuple(t.shape)}")
    return t, False


def label_components(x, threshold: float = 0.0, connectivity: int = 3):
    """The components of ``x > threshold`` -> (labels int32, counts): host restatement for arrays, kernels for device tensors."""
    if not isinstance(x, torch.Tensor):
        return label_components_host(np.asarray(x) > threshold, connectivity)
    xb, single = _batched(x)
    if xb.dtype not in (torch.float32, torch.uint8):
        xb = xb.to(torch.float32)
    labels, counts = ops.label_components(xb.contiguous(), threshold, connectivity)
    return (labels[0], counts[0]) if single else (labels, counts)


def component_stats(labels, values=None, max_components: int = 64) -> dict:
    if not isinstance(labels, torch.Tensor):
        return component_stats_host(labels, values, max_components)
    lb, single = _batched(labels)
    st = ops.component_stats(lb.contiguous(), None if values is None else _batched(values)[0].contiguous(), max_components)
    return {k: (st[k][0] if single else st[k]) for k in STAT_KEYS}


def component_overlap(a, b, max_a: int, max_b: int):
    if not isinstance(a, torch.Tensor):
        return overlap_host(a, b, max_a, max_b)
    ab, single = _batched(a)
    t = ops.component_overlap(ab.contiguous(), _batched(b)[0].contiguous(), max_a, max_b)
    return t[0] if single else t


def _extract_host(softmax: np.ndarray, threshold, n_max: int, min_voxels: int, factor: float, min_confidence: float, connectivity: int):
    B = softmax.shape[0]
    det = np.zeros(softmax.shape, np.float32)
    cand = np.zeros(softmax.shape, np.int32)
    if threshold != "dynamic":
        labels, counts = label_components_host(softmax > np.float32(threshold), connectivity)
        K = max(int(counts.max()), 1)
        st = component_stats_host(labels, softmax, K)
        conf = np.zeros((B, K), np.float32)
        for b in range(B):
            k = 0
            for l in range(int(counts[b])):
                if st["count"][b, l] >= min_voxels:
                    sel = labels[b] == l + 1
                    conf[b, k] = st["max"][b, l]
                    k += 1
                    det[b][sel], cand[b][sel] = st["max"][b, l], k
        return det, conf, cand
    conf = np.zeros((B, n_max), np.float32)
    for b in range(B):
        w = softmax[b].copy()
        k = 0
        for _ in range(n_max):
            i = int(np.argmax(w))                                          # (the first of equal maxima)
            peak = w.reshape(-1)[i]
            if not peak > np.float32(min_confidence):
                break
            labels, _ = _label_one(w > peak / np.float32(factor), connectivity)
            sel = labels.reshape(-1)[i]
            if sel == 0:                                                   # the peak is not above its own threshold (peak <= 0)
                break
            comp = labels == sel
            if int(comp.sum()) >= min_voxels:
                conf[b, k] = peak
                k += 1
                det[b][comp], cand[b][comp] = peak, k
            w[comp] = 0
    return det, conf, cand


def _extract_device(softmax: torch.Tensor, threshold, n_max: int, min_voxels: int, factor: float, min_confidence: float,
                    connectivity: int):
    B = softmax.shape[0]
    ws = ops.cc_workspace(softmax.shape, softmax.device)
    if threshold != "dynamic":
        labels, counts = ops.label_components(softmax, float(np.float32(threshold)), connectivity, ws=ws)
        K = max(int(counts.max()), 1)                                      # the one host read: it sizes the table
        det, cand, conf, _ = ops.cc_relabel(labels, ops.component_stats(labels, softmax, K), min_voxels)
        return det, conf, cand
    w = torch.empty_like(softmax)                                          # (the first round reads softmax and writes w: no copy)
    state = ops.cc_state(B, softmax.device)
    det = torch.empty(softmax.shape, dtype=torch.float32, device=softmax.device)
    cand = torch.empty(softmax.shape, dtype=torch.int32, device=softmax.device)
    conf = torch.empty((B, n_max), dtype=torch.float32, device=softmax.device)
    for it in range(n_max):
        src = softmax if it == 0 else w
        ops.cc_peak(src, state, factor, min_confidence, reset=it == 0, ws=ws)
        labels, _ = ops.label_components(src, state[ops.L.M1_CC_ST_THRESHOLD].view(torch.float32), connectivity, ws=ws)
        ops.cc_select(labels, state)
        ops.cc_take(labels, state, w, det, cand, conf, min_voxels, reset=it == 0, w_src=src if it == 0 else None)
    return det, conf, cand


def extract_lesion_candidates(softmax, threshold="dynamic", num_lesions_to_extract: int = 5, min_voxels_detection: int = 10,
                              dynamic_threshold_factor: float = 2.5, min_confidence: float = 0.1, connectivity: int = 3):
    """Lesion candidates of a (D,H,W) or (B,D,H,W) fp32 probability map -> (detection_map fp32, confidences fp32 ((B,) n), candidate_labels
    int32): candidate k of a batch entry has confidence ``confidences[..., k - 1]`` (0 beyond the last candidate), carries the number k
    in ``candidate_labels`` and its confidence on its voxels in ``detection_map``; everything else is 0.

    A number as ``threshold``: the components of ``softmax > fp32(threshold)`` with at least ``min_voxels_detection`` voxels, in label
    order, confidence = the component's maximum; n = the largest component count of the batch.

    ``'dynamic'`` (this project's statement of the rule; n = ``num_lesions_to_extract``): start from w = a copy of softmax and repeat n
    times: peak, i = the maximum of w and the first index where it is reached; stop unless peak > ``min_confidence``; label
    w > fp32(peak) / fp32(``dynamic_threshold_factor``); sel = the component that holds i; if it has ``min_voxels_detection`` voxels or
    more it becomes the next candidate with confidence peak; in every case w = 0 on sel.  (sel is background only when peak <= 0,
    which also stops.)"""
    n_max = int(num_lesions_to_extract)
    if n_max < 1:
        raise ValueError("num_lesions_to_extract must be positive")
    if isinstance(threshold, str) and threshold != "dynamic":
        raise NotImplementedError(f"threshold {threshold!r}: a number or 'dynamic' ('dynamic-fast' and the like are not built)")
    if not float(dynamic_threshold_factor) > 0:
        raise ValueError("dynamic_threshold_factor must be positive")
    args = (threshold, n_max, int(min_voxels_detection), float(dynamic_threshold_factor), float(min_confidence), int(connectivity))
    if isinstance(softmax, torch.Tensor):
        sb, single = _batched(softmax)
        out = _extract_device(sb.to(torch.float32).contiguous(), *args)
    else:
        sb, single = _batched(np.asarray(softmax, np.float32))
        out = _extract_host(sb, *args)
    return tuple(o[0] for o in out) if single else out


# ---- matching and the curves (host: the tables are a few numbers) ----------------------------------------------------------------
def _best_assignment(score: np.ndarray, allowed: np.ndarray) -> List[int]:
    """match[j] = the row matched to column j or -1: the one-to-one assignment over the allowed pairs with the largest total score,
    by exhaustive search (the first found among equals: rows are tried in ascending order, 'no match' last)."""
    nrow, ncol = score.shape
    best = {"total": -1.0, "match": [-1] * ncol}

    def rec(j: int, used: int, total: float, match: List[int]) -> None:
        if j == ncol:
            if total > best["total"]:
                best["total"], best["match"] = total, list(match)
            return
        for i in range(nrow):
            if allowed[i, j] and not used >> i & 1:
                match[j] = i
                rec(j + 1, used | 1 << i, total + float(score[i, j]), match)
        match[j] = -1
        rec(j + 1, used, total, match)

    rec(0, 0, 0.0, [-1] * ncol)
    return best["match"]


def match_table(table: np.ndarray, confidences: Sequence[float], min_overlap: float = 0.10, overlap: str = "iou"):
    """``evaluate_case`` from the (Kc + 1, Kl + 1) contingency table of candidates x lesions and the candidates' confidences."""
    if overlap not in ("iou", "dice"):
        raise NotImplementedError(f"overlap {overlap!r}: 'iou' and 'dice' are built")
    t = np.asarray(table, np.int64)
    inter = t[1:, 1:].astype(np.float64)
    size_c, size_l = t[1:, :].sum(axis=1, dtype=np.float64)[:, None], t[:, 1:].sum(axis=0, dtype=np.float64)[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        score = inter / (size_c + size_l - inter) if overlap == "iou" else 2.0 * inter / (size_c + size_l)
    score = np.nan_to_num(score)
    allowed = (score >= float(min_overlap)) & (inter > 0)
    # only candidates and lesions with an allowed pair take part in the search
    rows, cols = np.flatnonzero(allowed.any(axis=1)), np.flatnonzero(allowed.any(axis=0))
    sub = _best_assignment(score[np.ix_(rows, cols)], allowed[np.ix_(rows, cols)]) if rows.size and cols.size else []
    match = {int(cols[j]): int(rows[i]) for j, i in enumerate(sub) if i >= 0}
    results = []
    for j in range(inter.shape[1]):
        if j in match:
            results.append((1, float(confidences[match[j]]), float(score[match[j], j])))
        else:
            results.append((1, 0.0, 0.0))
    taken = set(match.values())
    results += [(0, float(confidences[i]), 0.0) for i in range(inter.shape[0]) if i not in taken]
    return results, max([float(c) for c in confidences], default=0.0)


def evaluate_case(detection_map, y_true, min_overlap: float = 0.10, overlap: str = "iou"):
    """One case -> (lesion_results, case_confidence).  Candidates are the components (connectivity 3) of ``detection_map > 0``, each
    with its maximum as confidence; lesions those of ``y_true >= 1``.  One contingency table gives every pair's IoU (or Dice); pairs
    below ``min_overlap`` may not match; among the rest the one-to-one assignment with the largest total overlap is taken.
    ``lesion_results``: (1, confidence, overlap) per matched lesion, (1, 0, 0) per missed lesion, (0, confidence, 0) per unmatched
    candidate; ``case_confidence``: the largest confidence or 0.  This is this project's own definition (module docstring)."""
    if isinstance(detection_map, torch.Tensor) != isinstance(y_true, torch.Tensor):
        raise TypeError("evaluate_case: the detection map and the annotation must both be arrays or both be device tensors")
    if tuple(detection_map.shape) != tuple(y_true.shape) or len(detection_map.shape) != 3:
        raise ValueError(f"two (D,H,W) volumes expected, got {tuple(detection_map.shape)} and {tuple(y_true.shape)}")
    below_one = float(np.nextafter(np.float32(1), np.float32(0)))          # x > below_one  <=>  x >= 1 in fp32
    if isinstance(detection_map, torch.Tensor):
        det = detection_map.to(torch.float32).contiguous()[None]
        gt = y_true.contiguous()[None]
        gt = gt if gt.dtype in (torch.float32, torch.uint8) else gt.to(torch.float32)
        ws = ops.cc_workspace(det.shape, det.device)
        lc, nc = ops.label_components(det, 0.0, 3, ws=ws)
        ll, nl = ops.label_components(gt, below_one, 3, ws=ws)
        kc, kl = int(nc[0]), int(nl[0])                                    # the one host read: it sizes the tables
        conf = ops.component_stats(lc, det, max(kc, 1))["max"][0, :kc].cpu().numpy()
        table = ops.component_overlap(lc, ll, kc, kl)[0].cpu().numpy()
    else:
        det = np.asarray(detection_map, np.float32)
        lc, kc = label_components_host(det > 0, 3)
        ll, kl = label_components_host(np.asarray(y_true).astype(np.float32) > np.float32(below_one), 3)
        conf = component_stats_host(lc, det, max(kc, 1))["max"][:kc]
        table = overlap_host(lc, ll, kc, kl)
    return match_table(table, conf, min_overlap, overlap)


def froc(per_case_lesion_results, thresholds=None) -> dict:
    """Free-response ROC from the ``lesion_results`` of every case (a sequence of sequences of (is_lesion, confidence, overlap)):
    at each threshold t, ``sensitivity`` = matched lesions with confidence >= t / all lesions (nan without lesions) and
    ``fp_per_case`` = unmatched candidates with confidence >= t / cases.  ``thresholds``: every distinct positive confidence, from the
    largest down, unless given.  A missed lesion (overlap 0) is detected at no threshold."""
    cases = [list(c) for c in per_case_lesion_results]
    tp = np.array([c for case in cases for is_l, c, ov in case if is_l and ov > 0], np.float64)
    fp = np.array([c for case in cases for is_l, c, ov in case if not is_l], np.float64)
    n_lesions = sum(1 for case in cases for is_l, _, _ in case if is_l)
    if thresholds is None:
        every = np.concatenate([tp, fp])
        thresholds = np.unique(every[every > 0])[::-1]
    thr = np.asarray(thresholds, np.float64).reshape(-1)
    hit = (tp[None, :] >= thr[:, None]).sum(axis=1).astype(np.float64)
    false = (fp[None, :] >= thr[:, None]).sum(axis=1).astype(np.float64)
    return {"thresholds": thr, "sensitivity": hit / n_lesions if n_lesions else np.full(thr.shape, np.nan),
            "fp_per_case": false / len(cases) if cases else np.full(thr.shape, np.nan), "num_lesions": n_lesions,
            "num_cases": len(cases)}


def average_precision(per_case_lesion_results) -> float:
    """Lesion-level average precision over the thresholds of ``froc`` (every distinct positive confidence, from the largest down):
    AP = sum_k (R_k - R_{k-1}) * P_k with R_0 = 0, R_k = ``froc``'s ``sensitivity`` at threshold k -- missed lesions count in its
    denominator and are detected at no threshold -- and P_k = TP_k / (TP_k + FP_k), TP_k the matched lesions and FP_k the unmatched
    candidates with confidence >= the threshold.  NaN without lesions, 0 with lesions and no positive confidence.

    This is this project's own definition, like ``froc`` (module docstring).  Pinned in tests/test_bootstrap_host.py: without missed
    lesions it equals ``sklearn.metrics.average_precision_score(is_lesion, confidence)``; with m missed of L lesions it is (L - m) / L
    times sklearn's value on the list without the missed ones."""
    cases = [list(c) for c in per_case_lesion_results]
    curve = froc(cases)
    if not curve["num_lesions"]:
        return float("nan")
    thr = curve["thresholds"]
    tp = np.array([c for case in cases for is_l, c, ov in case if is_l and ov > 0], np.float64)
    fp = np.array([c for case in cases for is_l, c, ov in case if not is_l], np.float64)
    hit = (tp[None, :] >= thr[:, None]).sum(axis=1).astype(np.float64)
    false = (fp[None, :] >= thr[:, None]).sum(axis=1).astype(np.float64)
    recall = np.concatenate([[0.0], curve["sensitivity"]])
    return float(np.sum((recall[1:] - recall[:-1]) * (hit / (hit + false))))


def auroc(case_labels, case_scores) -> float:
    """Area under the ROC curve by ranks (Mann-Whitney U / (positives * negatives)), tied scores counting half; fp64."""
    y = np.asarray(case_labels).reshape(-1) != 0
    s = np.asarray(case_scores, np.float64).reshape(-1)
    if y.shape != s.shape:
        raise ValueError("one score per label expected")
    n_pos, n_neg = int(y.sum()), int((~y).sum())
    if n_pos == 0 or n_neg == 0:
        raise ValueError("AUROC needs at least one positive and one negative case")
    _, inverse, counts = np.unique(s, return_inverse=True, return_counts=True)
    ends = np.cumsum(counts).astype(np.float64)
    rank = (ends - (counts - 1) / 2.0)[inverse.reshape(-1)]                # the mean 1-based rank of each group of equal scores
    return float((rank[y].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * float(n_neg)))


def dice_3d(predictions, labels):
    """callbacks.py:36-40: (2 * sum of the predictions where labels == 1 + 1e-7) / (sum of predictions + sum of labels + 1e-7), fp32;
    numpy for arrays, torch ops for tensors (a 0-d tensor on the inputs' device)."""
    eps = 1e-7
    if isinstance(predictions, torch.Tensor):
        p, l = predictions.to(torch.float64), labels.to(torch.float64)
        return ((2.0 * (p * (l == 1)).sum() + eps) / (p.sum() + l.sum() + eps)).to(torch.float32)
    p, l = np.asarray(predictions), np.asarray(labels)
    return np.float32((2.0 * np.sum(p[l == 1]) + eps) / (np.sum(p) + np.sum(l) + eps))
