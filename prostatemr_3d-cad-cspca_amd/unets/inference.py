"""Inference driving, host composition only: ``_Predictor`` defines ``predict`` / ``predict_mc`` / ``predict_tiled`` / ``predict_scan``
once, on one primitive, ``_accumulate`` (passes of draws folded into the MC accumulators of ops.mc_*).  ``Detector``
(``M1.get_detect_model()``) runs one model's passes; ``Ensemble`` walks its members' detectors over one set of accumulators.
``networks`` imports this module at its end (``networks.Ensemble``, ``networks.tta_views``), so nothing here imports ``networks`` at
module level."""
import glob
import os

import numpy as np
import torch
import torch.nn as nn

from ..hip import ops


def _mc_counts(n_draws, draws_per_pass, views=None):
    n, R = int(n_draws), int(draws_per_pass)
    N = n * (len(views) if views else 1)
    if n < 1 or R < 1 or N % R:
        what = "it" if views is None else f"views * n_draws = {N}"
        raise ValueError(f"predict_mc: n_draws >= 1 and draws_per_pass dividing {what} expected, got {n_draws} / {draws_per_pass}")
    if views is not None and R > 16:
        raise ValueError(f"predict_mc: at most 16 draws per pass with tta (one mirror mask each), got {R}")
    return n, R


_TTA_BITS = {"w": 1, "h": 2, "d": 4}


def tta_views(spec):
    """The mirror masks of a test-time augmentation: ``None`` (no TTA) or a non-empty sequence of views, each a string over the letters
    ``d``, ``h``, ``w`` naming the axes it mirrors (``""`` or ``"id"``: the identity), e.g. ``("", "w")`` or ``("", "w", "h", "hw")``
    -> the tuple of 3-bit masks (w = 1, h = 2, d = 4) that ops.tta_views / ops.mc_accum_v take.  The identity is a view like any
    other: it is in only if listed.  ValueError for an unknown or repeated letter, a view listed twice, or no view at all."""
    if spec is None:
        return None
    if isinstance(spec, str):
        raise ValueError(f"tta: a sequence of views expected, e.g. ('', 'w'), got the string {spec!r}")
    masks = []
    for v in spec:
        if isinstance(v, str):
            letters = "" if v == "id" else v.lower()
            if any(c not in _TTA_BITS for c in letters) or len(set(letters)) != len(letters):
                raise ValueError(f"tta: a view is made of the letters d, h, w, each at most once ('' or 'id': identity), got {v!r}")
            m = sum(_TTA_BITS[c] for c in letters)
        elif isinstance(v, (int, np.integer)) and not isinstance(v, bool) and 0 <= int(v) <= 7:
            m = int(v)
        else:
            raise ValueError(f"tta: a view is a string over d, h, w (or its mask 0..7), got {v!r}")
        if m in masks:
            raise ValueError(f"tta: view {v!r} is listed twice")
        masks.append(m)
    if not masks:
        raise ValueError("tta: at least one view expected (None switches it off)")
    return tuple(masks)


class _Predictor:
    """The four entry points of anything that runs MC passes on a network's grid.  A subclass gives
    ``dims``      the network's grid (D, H, W),
    ``members``   the number of models whose draws share the accumulators (1 for the detect model),
    ``cascaded``  whether there are two stages: every result is then the list [stage 1, stage 2],
    ``_accumulate(x, n, R, uncertainty=False, *, total=0, advance=True, views=None[, eps_p=None]) -> (sums, draws)``, one entry per
                  stage: every member's ``n`` draws (per view of ``views``) of ``x`` in passes of ``R``, see ``Detector._accumulate``,
    and, where they differ from what stands here, ``_predict_one``, ``_injectable`` and ``_scans``."""
    _predict_one = None            # ``predict`` without ``tta``, where that is not one draw per member into the accumulators
    _injectable = frozenset()      # the keywords of injected draws that ``predict`` / ``predict_mc`` pass on

    def _check_inject(self, who, inject):
        extra = sorted(inject.keys() - self._injectable)
        if extra:
            raise TypeError(f"{who}() got an unexpected keyword argument {extra[0]!r}")

    def _scans(self, x):                         # (the per-stage parts of an input or of ``predict_scan``'s ``raw``)
        return [x]

    def _mc_results(self, sums, draws, n, views, uncertainty, mean_only=False):
        """The accumulators of ``_accumulate`` after ``n`` draws per member and view -> the result dict (``mean_only``: its "mean"), per
        stage when cascaded."""
        res = []
        with torch.no_grad():
            for j, s in enumerate(sums):
                d = ops.mc_finalize(s, self.members * n * (len(views) if views else 1), uncertainty)
                if draws is not None:
                    d["samples"] = draws[j]
                res.append(d["mean"] if mean_only else d)
        return res if self.cascaded else res[0]

    def predict(self, x, tta=None, **inject):
        """One prediction at the current {seed, step} state, which does not move.  The detect model: ``forward(x, **inject)``.  An
        ensemble: (B,D,H,W,nc) fp32, the mean of the members' ``predict(x)``, one draw each at the member's current state.
        With ``tta`` (see ``tta_views``) the mean over the mirrored views, each un-mirrored: what
        ``predict_mc(x, 1, draws_per_pass=len(views), tta=views)`` returns as "mean" from the current state, one stacked pass (an
        ensemble: the mean of the members' ``predict(x, tta=tta)``, one stacked pass per member).
        ``inject``: the detect model's ``eps_q`` / ``eps_p``; an ensemble takes none (TypeError)."""
        self._check_inject("predict", inject)
        views = tta_views(tta)
        if views is None and self._predict_one is not None:
            return self._predict_one(x, **inject)
        if inject.pop("eps_q", None) is not None:
            raise ValueError("predict: eps_q has no part in a prediction with tta")
        sums, _ = self._accumulate(x, 1, len(views) if views else 1, advance=False, views=views, **inject)
        return self._mc_results(sums, None, 1, views, False, mean_only=True)

    def predict_mc(self, x, n_draws, draws_per_pass=1, *, return_samples=False, uncertainty=False, tta=None, **inject):
        """Monte-Carlo inference (the reference's --UNET_PROBA_ITER, train_model.py:72): ``n_draws`` hypotheses of ``predict`` --
        fresh dropout masks and, for the probabilistic model, fresh z ~ P at every level -- folded into
        {"mean": (B,D,H,W,nc) fp32, "entropy": (B,D,H,W) fp32 in nats (scipy.stats.entropy of the mean)
         [, "samples": (n_draws,B,D,H,W,nc) fp32 with ``return_samples``]}; a cascaded model returns [stage 1, stage 2] of these.
        A pass runs ``draws_per_pass`` replicas of the input stacked along the batch axis, replica-major (sample r*B + b is
        replica r of sample b): the in-kernel draws are keyed by the element index over the whole batch, so every replica
        draws for itself.  The head's raw logits go to ops.mc_accum, which keeps only the running sum of the probabilities;
        ops.mc_finish divides and takes the entropy.  The {seed, step} state advances once per pass: the first draw is what
        ``predict(x)`` returns at the current state, and the call leaves the state at step + n_draws / draws_per_pass.
        ``inject``: the detect model's ``eps_p`` (injected draws, as in ``forward``), only with n_draws == 1: every draw would be
        the same; an ensemble takes none (TypeError).
        ``uncertainty``: the passes go through ops.mc_accum_u / ops.mc_finish_u and the result gains, per voxel and in nats,
        "expected_entropy" (B,D,H,W) = the mean of the draws' own entropies (what every draw agrees is ambiguous),
        "mutual_info" (B,D,H,W) = entropy - expected_entropy >= 0 (what the draws disagree on) and "variance" (B,D,H,W,nc),
        the population variance of the draws per class.  mean, entropy, samples and the state after the call are those of
        the call without it; one draw gives mutual_info = variance = +0.
        ``tta`` (see ``tta_views``): test-time augmentation by mirroring.  Every view takes ``n_draws`` draws, N = views *
        n_draws in all, view-major (view v owns draws [v * n_draws, (v + 1) * n_draws)), cut into passes of ``draws_per_pass``
        consecutive draws, which must divide N; a pass may mix views.  The input of a pass is ops.tta_views, its logits go
        to ops.mc_accum_v, which reads them at the mirrored coordinates: the sums, the maps and the samples (N,B,D,H,W,nc)
        are on the caller's grid, and no un-mirrored tensor exists in between.  ``tta=None`` is the call without it;
        ``tta=("",)`` gives its bits and its final state.
        An ensemble: N = members * n_draws draws, ``n_draws`` per member; "samples" (N,B,D,H,W,nc) are member-major (member i's draws
        at [i * n_draws, (i + 1) * n_draws)).  With ``tta``: N = members * views * n_draws, member-major, then view-major, every
        member's passes cut as in its own ``predict_mc(..., tta=tta)``."""
        self._check_inject("predict_mc", inject)
        views = tta_views(tta)
        n, R = _mc_counts(n_draws, draws_per_pass, views)
        per = n * (len(views) if views else 1)                        # (draws per member)
        if inject.get("eps_p") is not None and per > 1:
            raise ValueError("predict_mc: injected eps_p with n_draws > 1 would repeat one draw n_draws times")
        sums, draws = self._accumulate(x, n, R, uncertainty, total=self.members * per if return_samples else 0, views=views, **inject)
        return self._mc_results(sums, draws, n, views, uncertainty)

    def predict_tiled(self, x, n_draws=1, draws_per_pass=1, tiles_per_pass=1, *, overlap=0.5, weighting='gaussian', uncertainty=False,
                      tta=None):
        """``predict`` / ``predict_mc`` of an ``x`` (B,D,H,W,C) whose every extent is at least the network's ``dims`` (ValueError
        otherwise): sliding-window inference.  Returns what ``predict`` (n_draws == 1 without ``uncertainty``: the mean tensor) or
        ``predict_mc`` (the dict) returns, on x's grid.  A cascaded model raises NotImplementedError: its second stage reads the first
        stage's softmax tile by tile, and blending that is not built.
        ``x`` is cut by ops.tile_gather into the T overlapping tiles of ``tiling.tile_geometry(x's grid, dims, overlap)``; groups of
        ``tiles_per_pass`` consecutive tiles (it must divide T), stacked along the batch axis as the gather left them, go through
        ``_accumulate`` -> the group's accumulators (sum_p, or the triple with ``uncertainty``) after all its draws: the detect
        model's passes, or for an ``Ensemble`` its members one after the other into one set of accumulators, each member drawing from
        its own state as in its own call, N = members * n_draws draws per tile.  The MC accumulators are linear in the draws, so it
        is THEY that are blended: each group's accumulators are copied into their rows of one buffer per accumulator, allocated once
        for all T * B tiles (no ``cat``), ops.tile_blend turns each buffer into the accumulator on x's grid -- a mean over the
        covering tiles with the separable weight ``tiling.tile_weights(dims, weighting)``, 'gaussian' or 'constant' -- and one
        ops.mc_finalize finishes them.  What the tiles of a voxel disagree on therefore lands in mutual_info and variance, as the
        disagreement between folds does in ``Ensemble``.
        Draws and state: n_draws == 1 without ``uncertainty`` is ``predict`` -- one draw (with ``tta`` one stacked pass of the views)
        per group at the current {seed, step} state, which does not move, and the mean tensor is returned.  Anything else is
        ``predict_mc``: every group takes its own n_draws (times views) draws in passes of ``draws_per_pass`` and the state advances
        once per pass, group after group in ascending tile order, (T / tiles_per_pass) * passes steps in all; the dict is returned.
        The in-kernel draws are keyed by the element index over the stacked batch, so the tiles of a group draw for themselves.  With
        T == 1 the one group is x itself: the result and the state after the call are those of ``predict`` / ``predict_mc``, bit for
        bit."""
        from .. import tiling
        if self.cascaded:
            raise NotImplementedError("predict_tiled: cascaded models are not supported; only single-stage models are")
        if not isinstance(x, torch.Tensor) or x.dim() != 5:
            raise ValueError("predict_tiled: a tensor (B,D,H,W,C) expected (cascaded inputs are not supported)")
        dims = self.dims
        vol = tuple(int(v) for v in x.shape[1:4])
        if any(v < d for v, d in zip(vol, dims)):
            raise ValueError(f"predict_tiled: every extent of x must be at least the model's {tuple(dims)}, got {vol}")
        views = tta_views(tta)
        single = int(n_draws) == 1 and not uncertainty
        n, R = (1, len(views) if views else 1) if single else _mc_counts(n_draws, draws_per_pass, views)
        geom = tiling.tile_geometry(vol, dims, overlap)
        weights = tiling.tile_weights(dims, weighting)
        T, G, B = geom["T"], int(tiles_per_pass), int(x.shape[0])
        if G < 1 or T % G:
            raise ValueError(f"predict_tiled: tiles_per_pass must divide the {T} tiles of {vol} cut into {tuple(dims)}, got {tiles_per_pass}")
        with torch.no_grad():
            profile = ops.tile_profile(weights, x.device)
            tiles = ops.tile_gather(x.contiguous(), geom)
            bufs = None
            for k in range(T // G):
                rows = slice(k * G * B, (k + 1) * G * B)
                sums = self._accumulate(tiles[rows], n, R, uncertainty, advance=not single, views=views)[0][0]
                parts = tuple(sums) if uncertainty else (sums,)
                if bufs is None:
                    bufs = [torch.empty((T * B, *p.shape[1:]), dtype=torch.float32, device=p.device) for p in parts]
                for buf, p in zip(bufs, parts):
                    buf[rows].copy_(p)
            # (sum_h has no channel axis: it is blended as C = 1)
            acc = [ops.tile_blend(b if b.dim() == 5 else b.unsqueeze(-1), geom, profile) for b in bufs]
            acc = [a if b.dim() == 5 else a.squeeze(-1) for a, b in zip(acc, bufs)]
        return self._mc_results([tuple(acc) if uncertainty else acc[0]], None, n, views, uncertainty, mean_only=single)

    def predict_scan(self, raw, spacing, out_spacing, n_draws=1, draws_per_pass=1, *, percentile=None, channels=None, labels=False,
                     uncertainty=False, tta=None, region=None, tiles_per_pass=1, overlap=0.5, weighting='gaussian', **prepare_kw):
        """From a raw scan to a prediction on the scan's own grid: preprocess.prepare_scan to the network's grid ``dims``, ``predict``
        (n_draws == 1) or ``predict_mc``, then preprocess.restore of every map.  ``raw``: (B,d,h,w,C) fp32 / int16 on the
        device at ``spacing`` (cascaded: the pair or dict of the two stages' scans, both on one grid); ``prepare_kw`` goes to
        prepare_scan (pad_mode, constant_values, dtype, default_value).  Returns {"mean": (B,d,h,w,nsel) fp32, the channels
        ``channels`` of the restored softmax [, "entropy": (B,d,h,w) with n_draws > 1] [, "labels": (B,d,h,w) uint8, the argmax
        of the restored softmax, with ``labels``], "network": what predict / predict_mc returned on the network's grid}; a
        cascaded model returns [stage 1, stage 2] of these.  ``uncertainty``: the call goes through ``predict_mc(...,
        uncertainty=True)`` even with one draw, and the result gains "expected_entropy" and "mutual_info" (B,d,h,w), restored
        as the entropy is, and "variance" (B,d,h,w,nsel), restored with the channel selection of the mean.  ``tta`` goes to
        ``predict`` / ``predict_mc``.  ``region`` = (D,H,W) voxels at ``out_spacing``: the scan is prepared to max(region,
        the model's size) per axis instead of the model's size, ``predict_tiled`` (with ``tiles_per_pass``, ``overlap``,
        ``weighting``) stands in the middle, and "network" is on that larger grid (restore reads the grid off the map it is given);
        ``region=None`` is the call without it.  An ensemble: its own ``predict`` / ``predict_mc`` / ``predict_tiled`` in the middle.
        Host composition only."""
        from .. import preprocess as PP
        dims = self.dims
        if region is not None:
            if self.cascaded:
                raise NotImplementedError("predict_scan: region needs predict_tiled, which cascaded models do not have")
            if len(tuple(region)) != 3 or any(int(v) < 1 for v in region):
                raise ValueError(f"predict_scan: region must be three positive extents (D, H, W), got {region}")
            dims = tuple(max(int(r), int(d)) for r, d in zip(region, dims))
        raws = self._scans(raw)
        shape = tuple(int(v) for v in raws[0].shape[1:4])
        if any(tuple(int(v) for v in r.shape[1:4]) != shape for r in raws):
            raise ValueError(f"predict_scan: both stages' scans must share one grid, got {[tuple(r.shape) for r in raws]}")
        xs = [PP.prepare_scan(r, spacing, out_spacing, dims, percentile=percentile, **prepare_kw)[0] for r in raws]
        x = xs if self.cascaded else xs[0]
        if region is not None:
            net = self.predict_tiled(x, n_draws, draws_per_pass, tiles_per_pass, overlap=overlap, weighting=weighting,
                                     uncertainty=uncertainty, tta=tta)
        elif uncertainty or int(n_draws) != 1:
            net = self.predict_mc(x, n_draws, draws_per_pass, uncertainty=uncertainty, tta=tta)
        else:
            net = self.predict(x, tta=tta)
        res = []
        for o in (net if self.cascaded else [net]):
            mean = o["mean"] if isinstance(o, dict) else o
            r = PP.restore(mean.contiguous(), shape, spacing, out_spacing, order=1, channels=channels, labels=labels)
            d = {"mean": r[0] if labels else r}
            if isinstance(o, dict):
                for k in ("entropy", "expected_entropy", "mutual_info"):
                    if k in o:
                        d[k] = PP.restore(o[k].unsqueeze(-1), shape, spacing, out_spacing, order=1)[..., 0]
                if "variance" in o:
                    d["variance"] = PP.restore(o["variance"].contiguous(), shape, spacing, out_spacing, order=1, channels=channels)
            if labels:
                d["labels"] = r[1]
            d["network"] = o
            res.append(d)
        return res if self.cascaded else res[0]


class Detector(_Predictor, nn.Module):
    """``M1.get_detect_model()``: the model reconfigured to predict segment probabilities only (networks.py:196-206); see there for
    what ``forward`` returns.  It has no parameters, buffers or children of its own: the model is held, not registered, so ``to()``,
    ``state_dict()`` and ``parameters()`` are empty."""
    members = 1
    _injectable = frozenset(("eps_q", "eps_p"))

    def __init__(self, model):
        super().__init__()
        object.__setattr__(self, "model", model)          # (nn.Module.__setattr__ would register it as a child)
        self.dims = model.input_spatial_dims
        self.cascaded = model.references.cascaded != False  # noqa: E712

    def _stages(self, xs, eps_q=None, eps_p=None):
        """One pass over the stages' inputs ``xs`` -> the stages' output dicts; a probabilistic model runs the prior net with z ~ P
        ('prob_infer_conv'), on its own when there is one stage.  (A deterministic net has no use for the draws.)"""
        m, prob = self.model, self.model.references.probabilistic
        if self.cascaded:
            return m._cascade_stages(xs, eps_q=eps_q, eps_p=eps_p, with_infer=prob)
        return (m.m1_model(xs[0], train_outputs=False, eps_p=eps_p) if prob else m.m1_model(xs[0]),)

    def forward(self, x, eps_q=None, eps_p=None):
        m = self.model
        nc, prob = m.references.num_classes, m.references.probabilistic
        with torch.no_grad():
            outs = self._stages(x if self.cascaded else (m._prep(x),), eps_q, eps_p)
            res = [ops.softmax_heads([o['prob_infer_conv']], [(1, 1, 1)]) if prob else o['y_softmax'][..., :nc] for o in outs]
        return res if self.cascaded else res[0]

    _predict_one = forward

    def _scans(self, x):
        return list(self.model._cascade_inputs(x)) if self.cascaded else [x]

    def _accumulate(self, x, n, R, uncertainty=False, *, eps_p=None, total=0, advance=True, views=None, carry=None, first=0):
        """``n // R`` passes of ``R`` replicas each, folded into the accumulators ``carry`` = (sums, draws) of an earlier call
        (another model's, see ``Ensemble._accumulate``) or into fresh ones; returns (sums, draws), one entry per stage.  sums[j] is
        ops.mc_accumulate's sum_p, or its triple with ``uncertainty``.  ``total`` > 0 asks for the per-draw
        probabilities: draws[j] is (total, B, D, H, W, nc), and this call fills [first, first + n).  The {seed, step} state
        advances once per pass unless ``advance`` is False.
        ``views`` (mirror masks, ``tta_views``): len(views) * n draws, view-major, in (len(views) * n) // R passes of R
        consecutive draws; a pass's input is ops.tta_views of its draws' masks (both stages of a cascaded model alike) and
        its logits go to ops.mc_accumulate with these masks, which un-mirrors them; the call fills
        [first, first + len(views) * n)."""
        m, prob = self.model, self.model.references.probabilistic
        # (with views the stacks come from ops.tta_views, pass by pass)
        rep = (lambda t: t.repeat(R, 1, 1, 1, 1)) if R > 1 and views is None else (lambda t: t)
        sums, draws = carry if carry is not None else (None, None)
        with torch.no_grad():
            base, mirrored = tuple(rep(m._prep(t, channels=m.input_channels)) for t in self._scans(x)), {}
            for k in range((n if views is None else len(views) * n) // R):
                masks = None if views is None else tuple(views[j // n] for j in range(k * R, (k + 1) * R))
                if masks is not None and masks not in mirrored:
                    mirrored[masks] = tuple(ops.tta_views(t, masks) for t in base)
                xin = mirrored.get(masks, base)
                logits = [o['prob_infer_conv'] if prob else o['logits'] for o in self._stages(xin, eps_p=eps_p)]
                if sums is None:
                    sums = [None] * len(logits)
                if total and draws is None:
                    draws = [torch.empty((total, int(l.shape[0]) // R, *l.shape[1:]), dtype=torch.float32, device=l.device)
                             for l in logits]
                for j, l in enumerate(logits):
                    lo = first + k * R
                    r = ops.mc_accumulate(l, R, sums[j], draws[j][lo:lo + R] if total else False, uncertainty, masks)
                    sums[j] = r[0] if total else r
                if advance:
                    m.advance_rng()
        return sums, draws


class Ensemble(_Predictor):
    """Several non-cascaded ``M1`` models -- the trainer's one model per fold (--FOLDS 0 1 2 3 4) -- as one predictor.  An ensemble is
    more draws into the same accumulators: every member's passes are folded by ops.mc_accum[_u] into the sums the previous member
    left, in list order, and finished once with N = members * n_draws.  With ``uncertainty`` the between-draw term (mutual_info,
    variance) therefore also carries the disagreement between the folds.
    Each member draws from its own {seed, step} state, which advances exactly as that member's own ``predict_mc`` call would;
    ``seed`` gives member i ``seed_dropout(seed + i)``.
    ``Ensemble([m])`` equals ``m.get_detect_model()`` bit for bit from the same state.  The order of the members is the order of the
    summation: ensembles of the same members in another order agree to rounding (the tests' bound), not to the bit."""
    cascaded = False

    def __init__(self, models, seed=None):
        from .networks import M1
        models = list(models)
        if not models:
            raise ValueError("Ensemble: at least one model expected")
        for i, m in enumerate(models):
            if not isinstance(m, M1):
                raise ValueError(f"Ensemble: member {i} is a {type(m).__name__}, not an M1")
            if m.references.cascaded != False:  # noqa: E712
                raise NotImplementedError(f"Ensemble: member {i} is a cascaded model ('{m.references.cascaded}'); only single-stage "
                                          "members are supported")
        for what in ("num_classes", "input_spatial_dims", "input_channels"):
            vals = [getattr(m, what) for m in models]
            if any(v != vals[0] for v in vals):
                raise ValueError(f"Ensemble: members disagree in {what}: {vals}")
        self.models = models
        self.detectors = [m.get_detect_model() for m in models]
        self.members = len(models)
        self.num_classes, self.input_channels = models[0].num_classes, models[0].input_channels
        self.dims = self.input_spatial_dims = models[0].input_spatial_dims
        if seed is not None:
            for i, m in enumerate(models):
                m.seed_dropout(int(seed) + i)

    @classmethod
    def load(cls, paths, device, compute_dtype=None, seed=None):
        """One member per entry of ``paths`` through ``M1.load``: a checkpoint file (model_weights_NNN.npz), or a fold directory, of
        which the checkpoint with the highest number is taken.  Members are moved to ``device`` and put in eval mode."""
        from .networks import M1
        models = []
        for p in paths:
            if os.path.isdir(p):
                found = sorted(glob.glob(os.path.join(p, "model_weights_*.npz")))
                if not found:
                    raise FileNotFoundError(f"Ensemble.load: no model_weights_*.npz in {p}")
                p = found[-1]
            m = M1.load(p).to(device)
            if compute_dtype is not None:
                m.set_compute_dtype(compute_dtype)
            m.eval()
            models.append(m)
        return cls(models, seed=seed)

    def _accumulate(self, x, n, R, uncertainty=False, *, total=0, advance=True, views=None):
        """Every member's ``Detector._accumulate`` in list order, each into the accumulators the previous one left; with ``total``
        member i fills the draws [i * per, (i + 1) * per), per = views * n."""
        per = n * (len(views) if views else 1)                        # (draws per member)
        carry = None
        for i, dm in enumerate(self.detectors):
            carry = dm._accumulate(x, n, R, uncertainty, carry=carry, total=total, first=i * per, advance=advance, views=views)
        return carry
