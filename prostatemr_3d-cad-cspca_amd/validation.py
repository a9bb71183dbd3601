"""Validation during training: what the reference's trainer leaves open (train_model.py:240-245, ``# TBA - CALLBACKS FOR TRAIN-TIME
VALIDATION OF PERFORMANCE``) and its ``callbacks.py`` imports ``compute_FROC``, ``roc_auc_score`` and ``dice_3d`` for.  Nothing here
restates reference code: the callbacks themselves were never published.  ``validate`` connects pieces that exist and are tested on
their own -- ``get_detect_model().predict_mc`` (n-draw inference, --UNET_PROBA_ITER), ``detection`` (lesion candidates, matching, FROC,
AUROC), ``surface_distance`` (HD95, ASSD) -- and one kernel of its own, ``ops.val_score`` (csrc/validate.hip): one launch per batch
that leaves a 40-double record per case on the device (the focal term, the sums behind the soft and the hard Dice, the entropy sums).
The records of all batches are read once, after the last batch.

The validation loss ``val_focal`` is the DETECTION term alone, on the mean of the n draws: ``Focal.FL`` of each case, averaged over the
cases.  It holds no KL term and no L2 term; Keras' ``val_loss`` would include both.  (At inference the posterior is not run, so there
is no KL to report, and the L2 term does not depend on the data.)

Per-case definitions, all from the record (``score_host`` is their fp64 numpy restatement):
  soft Dice of class c    (2 sum_py + 1e-7) / (sum_p + sum_y + 1e-7), the reference's ``dice_3d`` (callbacks.py:36-40)
  hard Dice of class c    2 n_both / (n_pred + n_true) on the argmax labels, NaN when both are empty
  entropy, entropy_fg     entropy_sum / n_voxels, entropy_fg_sum / n_fg (NaN without foreground); NaN with n_draws == 1, where
                          ``predict`` returns no entropy
"""
from __future__ import annotations

import math
from typing import Iterable, List, Optional, Sequence

import numpy as np
import torch

from . import bootstrap as _boot             # (validate() has a parameter named bootstrap)
from . import calibration as _cal            # (validate() has a parameter named calibration)
from . import detection, surface_distance
from .hip import ops
from .unets.networks import tta_views

K_EPSILON = 1e-7
DEFAULT_SPACING = (3.0, 0.5, 0.5)            # mm in (D,H,W) order: the grid of the README's model
FP_RATES = (0.5, 1.0, 2.0)
REFERRALS = (0.10, 0.20)                     # val_err@refer10 / val_err@refer20: the error rate kept after referring that share
CALIBRATION_MAPS = ("entropy", "mutual_info", "expected_entropy")


# ---- the record on the host ---------------------------------------------------------------------------------------------------
def score_host(p, y, entropy=None, alpha: Sequence[float] = (0.25, 0.75), gamma: float = 2.0) -> List[dict]:
    """The records of ``ops.val_score`` in fp64 numpy, in the layout of ``ops.read_val_records``: one dict per case of ``p``
    (B,...,K) with the one-hot ``y`` of the same shape and ``entropy`` (B,...) or None.  The clip bounds are the fp32 numbers the
    kernel (and TensorFlow) clip with."""
    p32 = np.asarray(p, np.float32)
    B, K = int(p32.shape[0]), int(p32.shape[-1])
    pf = p32.reshape(B, -1, K).astype(np.float64)
    yf = np.asarray(y).reshape(B, -1, K).astype(np.float64)
    ef = None if entropy is None else np.asarray(entropy, np.float32).reshape(B, -1).astype(np.float64)
    al = np.asarray([float(np.float32(a)) for a in alpha], np.float64)
    if al.shape != (K,):
        raise ValueError(f"{K} class weights expected, got {len(alpha)}")
    lo, hi = float(np.float32(K_EPSILON)), float(np.float32(1) - np.float32(K_EPSILON))
    out = []
    for b in range(B):
        q = np.clip(pf[b] / pf[b].sum(axis=-1, keepdims=True), lo, hi)
        focal = float((al * ((yf[b] * (1.0 - q) ** float(gamma)) * (yf[b] * -np.log(q)))).sum())
        pred, true = np.argmax(pf[b], axis=-1), np.argmax(yf[b], axis=-1)
        fg = true >= 1
        d = {"focal": focal, "entropy_sum": 0.0 if ef is None else float(ef[b].sum()),
             "entropy_fg_sum": 0.0 if ef is None else float(ef[b][fg].sum()), "n_voxels": int(pf.shape[1]), "n_fg": int(fg.sum()),
             "sum_p": [float(pf[b, :, c].sum()) for c in range(K)], "sum_y": [float(yf[b, :, c].sum()) for c in range(K)],
             "sum_py": [float((pf[b, :, c] * yf[b, :, c]).sum()) for c in range(K)],
             "n_pred": [int((pred == c).sum()) for c in range(K)], "n_true": [int((true == c).sum()) for c in range(K)],
             "n_both": [int(((pred == c) & (true == c)).sum()) for c in range(K)],
             "p_max": [max(float(pf[b, :, c].max()), 0.0) for c in range(K)]}
        out.append(d)
    return out


def soft_dice(rec: dict, c: int) -> float:
    return (2.0 * rec["sum_py"][c] + K_EPSILON) / (rec["sum_p"][c] + rec["sum_y"][c] + K_EPSILON)


def hard_dice(rec: dict, c: int) -> float:
    den = rec["n_pred"][c] + rec["n_true"][c]
    return 2.0 * rec["n_both"][c] / den if den else float("nan")


def _nanmean(values) -> float:
    v = np.asarray(list(values), np.float64)
    v = v[~np.isnan(v)]
    return float(v.mean()) if v.size else float("nan")


def sens_at(froc: dict, x: float) -> float:
    """The largest sensitivity among the thresholds of ``detection.froc`` whose ``fp_per_case <= x``; 0 when there is none (or no
    lesion: the curve's sensitivities are NaN then)."""
    ok = np.asarray(froc["fp_per_case"], np.float64) <= float(x)
    s = np.asarray(froc["sensitivity"], np.float64)[ok]
    s = s[~np.isnan(s)]
    return float(s.max()) if s.size else 0.0


# ---- from the per-case lists to the reported numbers ------------------------------------------------------------------------------
def merge_case_records(shards: Iterable[Sequence[dict]]) -> List[dict]:
    """The per-case lists of every rank as the one list an unsharded run produces: every case carries ``index`` = (batch, position in
    the global batch), and rank r holds positions [r * b, (r + 1) * b) of every batch (ddp.shard_batch)."""
    return sorted((c for shard in shards for c in shard), key=lambda c: tuple(c["index"]))


def summarise(cases: Sequence[dict], train_obj: str, with_entropy: bool = True) -> dict:
    """The reported dict from the per-case list (pure host arithmetic on a few numbers per case)."""
    recs = [c["record"] for c in cases]
    out = {"val_focal": _nanmean(r["focal"] for r in recs)}
    if train_obj == "lesion":
        out["val_dice"] = _nanmean(soft_dice(r, 1) for r in recs)
        out["val_hard_dice"] = _nanmean(hard_dice(r, 1) for r in recs)
        try:
            out["val_auroc"] = detection.auroc([r["n_true"][1] > 0 for r in recs], [c["confidence"] for c in cases])
        except ValueError:                                                 # one class of cases is absent
            out["val_auroc"] = float("nan")
        curve = detection.froc([c["lesion_results"] for c in cases])
        for x in FP_RATES:
            out["val_sens@%gfp" % x] = sens_at(curve, x)
        nan = float("nan")
        out["val_entropy"] = _nanmean(r["entropy_sum"] / r["n_voxels"] for r in recs) if with_entropy else nan
        out["val_entropy_fg"] = _nanmean(r["entropy_fg_sum"] / r["n_fg"] if r["n_fg"] else nan for r in recs) if with_entropy else nan
    else:
        K = len(recs[0]["sum_p"]) if recs else 0
        for k in range(1, K):
            out[f"val_dice_c{k}"] = _nanmean(c["dice"][k - 1] for c in cases)
            out[f"val_hd95_c{k}"] = _nanmean(c["hd95"][k - 1] for c in cases)
            out[f"val_assd_c{k}"] = _nanmean(c["assd"][k - 1] for c in cases)
    out["val_cases"] = len(cases)
    if cases and all("calibration" in c for c in cases):
        out.update(summarise_calibration([c["calibration"] for c in cases], train_obj))
    return out


def summarise_calibration(records: Sequence[dict], train_obj: str) -> dict:
    """The calibration keys of ``summarise``, all from the POOLED record (``calibration.merge``: the voxels of every case together):
    ECE and MCE of the arg-max label, the Brier score (summed over the classes) and the NLL per voxel, the one-vs-rest ECE of class 1
    ('lesion') or the class-wise ECE ('zonal'), the AUROC of the uncertainty bin as a detector of wrong voxels and the error rate
    kept after referring the most uncertain 10 % / 20 % of the voxels (NaN without an uncertainty map: one draw)."""
    rec = _cal.merge(records)
    out = {"val_ece": _cal.ece(rec), "val_mce": _cal.mce(rec), "val_brier": _cal.brier(rec)["total"],
           "val_nll": _cal.nll(rec)}
    if train_obj == "lesion":
        out["val_ece_c1"] = _cal.classwise_ece(rec, (1,))
    else:
        out["val_cw_ece"] = _cal.classwise_ece(rec)
    out["val_unc_auroc"] = _cal.uncertainty_auroc(rec)
    curve = _cal.referral_curve(rec)
    for x in REFERRALS:
        out["val_err@refer%d" % round(100 * x)] = _cal.error_at_referral(curve, x)
    return out


def check_bootstrap(n_boot, level: float = 0.95) -> int:
    """The replicate count of ``validate(bootstrap=...)`` as an int: 0 (off) .. 2^20, with 0 < level < 1; ValueError otherwise."""
    n = int(n_boot)
    if n != n_boot or not 0 <= n <= _boot.MAX_BOOT:
        raise ValueError(f"bootstrap must be a whole number in 0..{_boot.MAX_BOOT} (0 = off), got {n_boot!r}")
    if not 0.0 < float(level) < 1.0:
        raise ValueError(f"bootstrap_level must lie strictly between 0 and 1, got {level!r}")
    return n


def summarise_bootstrap(cases: Sequence[dict], train_obj: str, n_boot: int, seed: int = 0, level: float = 0.95,
                        stratified: bool = False, device=None) -> dict:
    """The bootstrap keys of ``validate``: one ``bootstrap.pack`` of the per-case list, ONE call of ``bootstrap.replicates`` (the
    kernel with a ``device``) and the percentile interval of every column.  'lesion': ``val_ap`` (the point estimate,
    ``detection.average_precision``), then ``<key>_lo`` / ``<key>_hi`` for val_auroc, val_ap and every val_sens@<x>fp; 'zonal': the
    same pair for every val_dice_c<k>, val_hd95_c<k> and val_assd_c<k>.  Bounds of a column without a finite replicate are NaN."""
    out = {}
    if train_obj == "lesion":
        out["val_ap"] = detection.average_precision([c["lesion_results"] for c in cases])
    table = _boot.pack(cases, train_obj, FP_RATES)
    if train_obj == "lesion":
        keys = ["val_auroc", "val_ap"] + ["val_sens@%gfp" % x for x in FP_RATES]
    else:
        keys = ["val_" + name for name in table["value_names"]]
    if table["N"]:
        lo, hi, _ = _boot.interval(_boot.replicates(table, n_boot, seed, stratified, device=device), level)
    else:
        lo = hi = np.full(len(_boot.columns(table)), np.nan)
    first = 0 if train_obj == "lesion" else 2 + len(FP_RATES)
    for j, k in enumerate(keys):
        out[k + "_lo"], out[k + "_hi"] = float(lo[first + j]), float(hi[first + j])
    return out


# ---- the pass ----------------------------------------------------------------------------------------------------------------------
def validate(model, batches, steps: int, train_obj: str, n_draws: int = 1, draws_per_pass: int = 1,
             alpha: Sequence[float] = (0.25, 0.75), gamma: float = 2.0, spacing=None, rank: int = 0, world: int = 1,
             tta=None, calibration: bool = False, bins: int = 15, calibration_uncertainty: str = "entropy", bootstrap: int = 0,
             bootstrap_seed: int = 0, bootstrap_level: float = 0.95, bootstrap_stratified: bool = False) -> dict:
    """``steps`` batches of ``batches`` (an iterator of ``({"image": x}, {"detection": y, ...})`` as the feeds yield them, y one-hot)
    through ``model.get_detect_model()`` -> the dict of ``summarise``.

    Per batch: ``predict_mc(x, n_draws, draws_per_pass)`` (``predict`` with n_draws == 1), then ``ops.val_score`` on the mean, the
    labels and the entropy; the records stay on the device until the last batch.  'lesion': the candidates of ``mean[..., 1]``
    (``detection.extract_lesion_candidates``, 'dynamic') are matched per case with ``detection.evaluate_case``; FROC, AUROC (case label:
    n_true[1] > 0, score: the case's largest confidence) and the sensitivities at 0.5 / 1 / 2 false positives per case follow at the
    end.  'zonal': the argmax labels go to ``surface_distance.surface_metrics`` with ``spacing`` (mm, (D,H,W) order; default
    (3.0, 0.5, 0.5)); Dice, HD95 and ASSD per class are NaN-aware means over the cases.

    ``tta`` (``unets.networks.tta_views``: mirrored views, e.g. ``("", "w")``): a batch goes through ``predict_mc(x, n_draws,
    draws_per_pass, tta=views)``, views * n_draws draws in all, and the entropy is scored whenever that is more than one draw.

    The loss reported as ``val_focal`` is the detection term on the MC mean alone: no KL, no L2 (module docstring).

    ``calibration`` (off by default: the calls and the keys are then exactly those above): one more launch pair per batch,
    ``ops.cal_score`` on the mean and the arg-max labels with ``bins`` bins, and -- with more than one draw behind the mean -- on the
    map ``calibration_uncertainty`` names ('entropy'; 'mutual_info' / 'expected_entropy' make the batch go through
    ``predict_mc(..., uncertainty=True)``), binned up to ln K.  The records stay on the device and are read with the scoring records;
    every case carries its own under "calibration", and ``summarise`` appends the keys of ``summarise_calibration``.

    ``bootstrap`` = n > 0 (off by default: the calls and the keys are then exactly those above): after the last batch rank 0 packs the
    gathered case list and makes ONE more call, ``ops.bootstrap_metrics`` with n case-level replicates under ``bootstrap_seed``
    (``bootstrap_stratified``: positive and negative cases resampled apart), and appends the keys of ``summarise_bootstrap`` behind all
    others: ``val_ap`` and the ``bootstrap_level`` percentile bounds ``<key>_lo`` / ``<key>_hi``.  The other ranks do nothing more.

    Validation leaves no trace on training: the model's ``rng_state`` ({seed, step}) and its ``training`` flag are put back
    afterwards, whatever happens, so a run with validation gives the weights of the run without it bit for bit.

    Data parallel (world > 1): every rank scores its own shard and the per-case lists go to rank 0 (``gather_object``: a
    collective, every rank calls ``validate`` at the same point); rank 0 computes the curves, the other ranks return ``{}``."""
    if train_obj not in ("lesion", "zonal"):
        raise ValueError(f"train_obj must be 'zonal' or 'lesion', got {train_obj!r}")
    if model.references.cascaded != False:  # noqa: E712
        raise NotImplementedError("validate: a cascaded model returns two predictions per case; only the standalone model is scored")
    if calibration_uncertainty not in CALIBRATION_MAPS:
        raise ValueError(f"calibration_uncertainty must be one of {CALIBRATION_MAPS}, got {calibration_uncertainty!r}")
    n_boot = check_bootstrap(bootstrap, bootstrap_level)
    n, steps = int(n_draws), int(steps)
    views = tta_views(tta)
    N = n * (len(views) if views else 1)                                   # draws behind one mean
    cal_on, cal_recs, cal_map = bool(calibration), [], None
    ukw = {"uncertainty": True} if cal_on and N > 1 and calibration_uncertainty != "entropy" else {}
    spacing = DEFAULT_SPACING if spacing is None else tuple(float(s) for s in spacing)
    saved_rng, was_training = model.rng_state.clone(), model.training
    detect = model.get_detect_model()
    it = iter(batches)
    recs, cases, surf, ws, K = [], [], [], None, 0
    try:
        model.eval()
        with torch.no_grad():
            for step in range(steps):
                bx, by = next(it)
                y = by["detection"] if isinstance(by, dict) else by
                y = y.contiguous()
                if views is not None:
                    o = detect.predict_mc(bx, n, draws_per_pass, tta=views, **ukw)
                    mean, ent = o["mean"], (o["entropy"] if N > 1 else None)
                elif n == 1:
                    mean, ent = detect.predict(bx), None
                else:
                    o = detect.predict_mc(bx, n, draws_per_pass, **ukw)
                    mean, ent = o["mean"], o["entropy"]
                mean = mean.contiguous()
                B, K = int(mean.shape[0]), int(mean.shape[-1])
                if train_obj == "lesion" and K != 2:
                    raise ValueError(f"validate: 'lesion' scores class 1 of 2, the model has {K} classes")
                need = ops.val_score_ws(B, mean.numel() // (B * K), K)
                if ws is None or ws.numel() < need:                        # one workspace for every batch of the pass
                    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=mean.device)
                recs.append(ops.val_score(mean, y, ent, alpha, gamma, ws))
                if cal_on:
                    cal_map = None if N == 1 else o[calibration_uncertainty].contiguous()
                    cal_recs.append(ops.cal_score(mean, y.argmax(dim=-1).to(torch.uint8), bins, None, cal_map, math.log(K)))
                batch = [{"index": (step, rank * B + i)} for i in range(B)]
                if train_obj == "lesion":
                    det_map = detection.extract_lesion_candidates(mean[..., 1].contiguous(), "dynamic")[0]
                    truth = y[..., 1].contiguous()
                    for i, c in enumerate(batch):
                        c["lesion_results"], c["confidence"] = detection.evaluate_case(det_map[i], truth[i])
                else:
                    pred, truth = mean.argmax(dim=-1).to(torch.uint8), y.argmax(dim=-1).to(torch.uint8)
                    m = surface_distance.surface_metrics(pred, truth, tuple(range(1, K)), spacing, 95.0)
                    surf.append((len(cases), m))                           # (device tensors: read with the records, at the end)
                cases.extend(batch)
            rows = ops.read_val_records(torch.cat(recs), K) if recs else []                # the one host read of the records
            for c, r in zip(cases, rows):
                c["record"] = r
            if cal_recs:
                for c, r in zip(cases, ops.read_cal_records(torch.cat(cal_recs), K, bins)):
                    c["calibration"] = r
            for first, m in surf:
                t = {k: m[k].double().cpu().numpy() for k in ("dice", "hdq", "assd")}
                for i in range(len(t["dice"])):
                    c = cases[first + i]
                    c["dice"], c["hd95"], c["assd"] = ([float(v) for v in t[k][i]] for k in ("dice", "hdq", "assd"))
    finally:
        with torch.no_grad():
            model.rng_state.copy_(saved_rng)
        model.train(was_training)
    if world > 1:
        import torch.distributed as dist
        gathered = [None] * world if rank == 0 else None
        dist.gather_object(cases, gathered, dst=0)
        if rank != 0:
            return {}
        cases = merge_case_records(gathered)
    out = summarise(cases, train_obj, with_entropy=N > 1)
    if n_boot:
        out.update(summarise_bootstrap(cases, train_obj, n_boot, bootstrap_seed, bootstrap_level, bootstrap_stratified,
                                       device=next(model.parameters()).device))
    return out
