"""Seeded fuzz of the whole BACKWARD pass: every parameter gradient and the input gradient of one train step of sixteen random
model configurations against the fp64 oracle, on the autograd path and on the path training runs (flat-buffer sinks, queued
weight-gradient folds, batched SE-gate backwards, stacked passes).  The host-side machinery only the backward pass exercises
chooses its paths from shapes and constructor arguments -- gradient-slot fan-out, the InstanceNorm-backward hand-over, the
conv-pair path, the shared stem of the stacked passes, tail slices, the deferred fold queue, side-stream joins -- so a gradient
that is wrong for SOME configuration needs configurations nobody picked by hand.

Axes (``_train_fuzz_cases``): those of test_hip_model._model_fuzz_cases -- four filter sets, three stride sets, three kernel-size
sets, three SE reductions, four latent layouts, two or three classes, dense skip, deep supervision, probabilistic / deterministic,
input channels -- plus the batch size 1, 2 or 3 (3: the stacked passes get an odd half) and dropout off or 0.5 monte-carlo.  Volumes
are the smallest that reach every level: D = (product of the D strides) x {1, 2}, H, W in {32, 48}, B*D*H*W <= 18432 (a draw above
that is rejected and redrawn from the same stream: both oracle evaluations of the largest case then take a few seconds).

* fp32, per case: logits, softmax, KL and loss to the 1e-3 rules of test_hip_model; every parameter gradient through
  test_hip_model._check_grads (relative L2 <= max(1e-3, 3 e32) PER PARAMETER, e32 = the fp32 oracle's own error on that parameter);
  d(loss)/d(input) by the same rule; then the compiled training path on the same model and the same draw: its forward output is
  bit-equal to the first run (which licenses reusing the activation pattern and the oracle result) and its flat-buffer gradients
  pass the same check.
* bf16, per case, no oracle (model-level bf16 gradients sit 23-36 % from fp64 by the nature of the network): the autograd path and
  the training path agree per parameter to max|d| / max|ref| < 1e-5, a second run of each is bit-identical, nothing is NaN / Inf.

Conditions that keep the mechanism from hiding a failure, all asserted below:
* the LeakyReLU branches forced on the oracle differ from its own in at most max(3, MAX_FLIP_FRACTION * elements) elements
  (test_hip_model.MAX_FLIP_FRACTION = 5e-6, unchanged);
* no case is skipped, expected to fail or left out: sixteen cases, sixteen ids, no mark but ``gpu`` and the parametrisation;
* at most 5 % of a case's parameters have a tolerance relaxed above 1e-3 (MAX_RELAXED_SHARE);
* no relaxed tolerance exceeds 1e-2 (MAX_RELAXED_TOL).
The seed is one for which the ORACLE ALONE meets the last two (test_oracle_alone_meets_the_relaxation_caps: the fp64 evaluation's
own pattern, recorded by O.recorded_activation_pattern, forced on the fp32 evaluation), checked on the CPU.

Sensitivity (CPU, oracle only, test_rule_rejects_*): the per-parameter rule rejects a gradient that lacks one sample's share, one
that lacks its L2 term and a posterior gradient without the KL term -- and the whole-vector norm alone does NOT reject the first for
small parameters, which is why the rule is per parameter."""
import contextlib
import functools
import random
import time

import numpy as np
import pytest
import torch

from oracle import m1_oracle as O
from test_hip_model import MAX_FLIP_FRACTION, _check_grads, _oracle_loss_and_grads
from util import PKG, FlatGradView, activation_pattern, build_m1, load_params_into, rnd

N_CASES, SEED = 16, 0
MAX_VOXELS = 18432                  # B*D*H*W
MAX_RELAXED_SHARE = 0.05            # share of a case's parameters whose tolerance may lie above 1e-3
MAX_RELAXED_TOL = 1e-2              # and none above this
ALPHA = {2: (0.75, 0.25), 3: (0.6, 0.25, 0.15)}          # (three classes: the alpha of test_hip_model.test_c1_three_classes)

FILTER_SETS = [(8, 16, 32, 64, 128), (8, 16, 24, 32, 48), (16, 32, 48, 64, 96), (8, 16, 32, 48, 64)]
STRIDE_SETS = [((1, 1, 1), (1, 2, 2), (1, 2, 2), (2, 2, 2), (2, 2, 2)), ((1, 1, 1), (1, 2, 2), (1, 2, 2), (2, 2, 2), (1, 2, 2)),
               ((1, 1, 1), (2, 2, 2), (1, 2, 2), (1, 2, 2), (2, 2, 2))]
KERNEL_SETS = [((1, 3, 3), (1, 3, 3), (3, 3, 3), (3, 3, 3), (3, 3, 3)), ((3, 3, 3),) * 5, ((1, 3, 3),) * 5]
REDUCTIONS = [(8, 8, 8, 8, 8), (4, 4, 4, 4, 4), (2, 4, 8, 8, 16)]
LATENTS = [(3, 2, 1, 0), (1, 1, 1, 1), (2, 2, 0, 0), (4, 0, 0, 0)]


def _train_fuzz_cases(n, seed):
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        prob = rng.random() < 0.5
        filters = rng.choice(FILTER_SETS)
        strides = rng.choice(STRIDE_SETS)
        dmul = 1
        for s_ in strides:
            dmul *= s_[0]
        dims = (dmul * rng.choice([1, 2]), 16 * rng.choice([2, 3]), 16 * rng.choice([2, 3]))
        ks = rng.choice(KERNEL_SETS)
        red = rng.choice(REDUCTIONS)
        lat = rng.choice(LATENTS)
        nc = rng.choice([2, 2, 3])
        cin = (nc - 1) + rng.choice([1, 2, 3]) if prob else rng.choice([1, 2, 3, 4])
        dense, deep = rng.random() < 0.6, rng.random() < 0.5
        B = rng.choice([1, 2, 3])
        drop = rng.choice([0.0, 0.5])
        if B * dims[0] * dims[1] * dims[2] > MAX_VOXELS:
            continue                                     # too slow in the fp64 oracle: redraw from the same stream
        out.append(dict(i=len(out), prob=prob, filters=filters, strides=strides, dims=dims, ks=ks, red=red, lat=lat, nc=nc, cin=cin,
                        dense=dense, deep=deep, B=B, drop=drop))
    return out


CASES = _train_fuzz_cases(N_CASES, SEED)
_ids = lambda c: f"m{c['i']}"


def _config(c):
    return O.M1Config(input_spatial_dims=c["dims"], input_channels=c["cin"], num_classes=c["nc"], filters=c["filters"],
                      strides=c["strides"], kernel_sizes=c["ks"], se_reduction=c["red"], dense_skip=c["dense"],
                      deep_supervision=c["deep"], probabilistic=c["prob"], prob_latent_dims=c["lat"],
                      dropout_rate=c["drop"], dropout_mode="monte-carlo" if c["drop"] else "standard")


def _target(shape, nc, seed):
    """One-hot (B,D,H,W,nc): background and one ball per foreground class (a lower class wins where they overlap), centred anywhere
    along D (the volumes here are 2 to 8 slices deep)."""
    B, D, H, W = shape
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    t = np.zeros((B, D, H, W, nc), dtype=np.float32)
    for b in range(B):
        lab = np.zeros((D, H, W), dtype=np.int64)
        for cls in range(nc - 1, 0, -1):
            ctr = [rng.integers(0, D), rng.integers(5, H - 5), rng.integers(5, W - 5)]
            lab[((zz - ctr[0]) ** 2 + (yy - ctr[1]) ** 2 + (xx - ctr[2]) ** 2) <= 30] = cls
        for k in range(nc):
            t[b, ..., k] = lab == k
    return torch.from_numpy(t)


def _inputs(c, cfg):
    """(P, x, target, eps): fixture weights, a normal input whose last nc-1 channels carry the label in a probabilistic model
    (data_generators.py:82), the injected latent draws."""
    i, B, nc = c["i"], c["B"], c["nc"]
    P = O.fixture_params(cfg, seed=900 + i)
    x = rnd((B, *c["dims"], c["cin"]), 1000 + i)
    tgt = _target((B, *c["dims"]), nc, 1100 + i)
    if c["prob"]:
        x[..., c["cin"] - (nc - 1):] = tgt[..., 1:]
    eps = [rnd((B, *s), 1200 + 10 * i + j) for j, s in enumerate(O.latent_shapes(cfg))] if c["prob"] else None
    return P, x, tgt, eps


# ---- oracle only (CPU) ---------------------------------------------------------------------------------------------------------
def _level_dims(c, level):
    d = list(c["dims"])
    for s_ in c["strides"][:level + 1]:
        d = [-(-a // b) for a, b in zip(d, s_)]
    return tuple(d)


def _cpu_drop_masks(c):
    """Keep-masks for an oracle-only evaluation (on the GPU they are the product's own draw): every dropout layer behind a block of
    level L sees (B, dims of L, filters[L]); each pass through a core draws its own mask, like tf.nn.dropout does per call."""
    if not c["drop"]:
        return None
    g = torch.Generator().manual_seed(1300 + c["i"])
    dm = {}
    for core in (("posterior", "prior") if c["prob"] else ("core",)):
        for name, level in [(f"drope{l}", l) for l in (1, 2, 3, 4)] + [(f"dropd{l}", l) for l in (3, 2, 1, 0)] + \
                           ([(f"dropp{l}", l) for l in (3, 2, 1, 0)] if c["prob"] else []):
            shape = (c["B"], *_level_dims(c, level), c["filters"][level])
            rate = c["drop"] / 2 if name == "dropd0" else c["drop"]
            dm[f"{core}.{name}"] = {k: (torch.rand(shape, generator=g) >= rate).double() for k in (0, 1)}
    return dm


def _oracle_eval(cfg, c, P, x, tgt, eps, dm, dt, masks=None, record=False, **kw):
    """One oracle evaluation of the train loss in ``dt``: (parameter gradients, input gradient, recorded pattern or None), fp64 tensors."""
    Pd = {k: v.detach().to(dt, copy=True).requires_grad_(True) for k, v in P.items()}
    xd = x.detach().to(dt, copy=True).requires_grad_(True)
    dmd = None if dm is None else {k: {q: m.to(dt) for q, m in v.items()} for k, v in dm.items()}
    with (O.recorded_activation_pattern() if record else contextlib.nullcontext()) as rec, \
            (O.forced_activation_pattern(masks) if masks is not None else contextlib.nullcontext()):
        loss, _, _ = O.train_loss(Pd, cfg, xd, tgt.to(dt), eps_q=[e.to(dt) for e in eps] if eps else None, drop_masks=dmd,
                                  focal_alpha=ALPHA[c["nc"]], **kw)
    loss.backward()
    return {k: (v.grad.double() if v.grad is not None else None) for k, v in Pd.items()}, xd.grad.double(), (rec.masks if record else None)


@functools.lru_cache(maxsize=None)
def _oracle_alone(i):
    """fp64 evaluation on its own activation pattern, fp32 evaluation FORCED onto that pattern: what the fp32 format costs on one
    piecewise-linear branch, free of the fp32 run's own kink flips.  Computed once per case and shared (read-only) by the CPU tests."""
    c = CASES[i]
    cfg = _config(c)
    P, x, tgt, eps = _inputs(c, cfg)
    dm = _cpu_drop_masks(c)
    g64, gx64, masks = _oracle_eval(cfg, c, P, x, tgt, eps, dm, torch.float64, record=True)
    g32, gx32, _ = _oracle_eval(cfg, c, P, x, tgt, eps, dm, torch.float32, masks=masks)
    return dict(cfg=cfg, P=P, x=x, tgt=tgt, eps=eps, dm=dm, masks=masks, g64=g64, g32=g32, gx64=gx64, gx32=gx32)


class _DictView:
    """A gradient dict behind the interface _check_grads reads."""

    def __init__(self, P, grads):
        self.P, self.grads = P, grads

    def named_parameters(self):
        for k, v in self.P.items():
            q = torch.nn.Parameter(v.detach().double(), requires_grad=False)
            q.grad = None if self.grads[k] is None else self.grads[k].clone()
            yield k, q


def _input_rule(gx, gx64, gx32):
    """(error, tolerance) of an input gradient: relative L2 against fp64, max(1e-3, 3 e32) -- the rule of _check_grads."""
    n = float(gx64.norm())
    return float((gx.detach().double().cpu() - gx64).norm()) / n, max(1e-3, 3.0 * float((gx32 - gx64).norm()) / n)


def test_generator_covers_every_axis():
    assert len(CASES) == N_CASES and [c["i"] for c in CASES] == list(range(N_CASES))
    assert CASES == _train_fuzz_cases(N_CASES, SEED)                     # seeded: the same cases in every process
    for c in CASES:
        assert c["B"] * c["dims"][0] * c["dims"][1] * c["dims"][2] <= MAX_VOXELS
        cfg = _config(c)
        shapes = O.m1_param_shapes(cfg)                                  # the case builds in the oracle
        assert set(O.fixture_params(cfg, seed=0, shapes=shapes)) == set(shapes)
    count = lambda f: sum(1 for c in CASES if f(c))
    for B in (1, 2, 3):
        assert count(lambda c: c["B"] == B) >= 3, B
    assert count(lambda c: c["drop"] > 0) >= 5
    assert count(lambda c: c["prob"]) >= 5 and count(lambda c: not c["prob"]) >= 5
    assert count(lambda c: c["nc"] == 3) >= 3
    assert {c["filters"] for c in CASES} == set(FILTER_SETS)
    assert {c["strides"] for c in CASES} == set(STRIDE_SETS)


def test_no_case_is_skipped_or_expected_to_fail():
    assert MAX_FLIP_FRACTION == 5e-6
    for fn in (test_train_step_fp32_against_oracle, test_train_step_bf16_paths_agree_and_repeat):
        marks = fn.pytestmark
        assert sorted(m.name for m in marks) == ["gpu", "parametrize"], marks
        (par,) = [m for m in marks if m.name == "parametrize"]
        assert par.args[1] is CASES and len(par.args[1]) == N_CASES
        assert not any(hasattr(v, "marks") for v in par.args[1])         # no pytest.param(..., marks=skip / xfail)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_oracle_alone_meets_the_relaxation_caps(case):
    """What decides the seed: on the fp64 pattern the fp32 oracle itself relaxes at most 5 % of the parameters, none above 1e-2,
    and the input gradient's tolerance stays below 1e-2 as well."""
    t0 = time.time()
    r = _oracle_alone(case["i"])
    rep = {}
    relaxed = _check_grads(_DictView(r["P"], r["g64"]), r["g64"], r["g32"], strip=(), max_relaxed_tol=MAX_RELAXED_TOL, report=rep)
    _, tolx = _input_rule(r["gx64"], r["gx64"], r["gx32"])
    print(f"oracle alone m{case['i']}: {relaxed} of {rep['params']} parameters relaxed, largest tolerance {rep['max_tol']:.2e}, "
          f"input-gradient tolerance {tolx:.2e}, {time.time() - t0:.1f} s")
    assert relaxed <= MAX_RELAXED_SHARE * rep["params"], (relaxed, rep["params"])
    assert tolx <= MAX_RELAXED_TOL, tolx


# ---- sensitivity (CPU, oracle only) ----------------------------------------------------------------------------------------------
def _vector_rule_rejects(gh, g64, g32):
    """The whole-gradient-vector check of _check_grads, alone."""
    gmax = max(float(g.norm()) for g in g64.values() if g is not None)
    num = den = num32 = 0.0
    for k, go in g64.items():
        if go is None or float(go.norm()) < 1e-6 * gmax:
            continue
        num += float((gh[k] - go).norm()) ** 2; den += float(go.norm()) ** 2; num32 += float((g32[k] - go).norm()) ** 2
    return not ((num / den) ** 0.5 < max(1e-3, 2.0 * (num32 / den) ** 0.5))


def _rule_rejects(r, name, g):
    """Does _check_grads reject the oracle's own fp64 gradients with ``name`` replaced by ``g`` -- and by its PER-PARAMETER rule?"""
    gh = dict(r["g64"]); gh[name] = g
    try:
        _check_grads(_DictView(r["P"], gh), r["g64"], r["g32"], strip=())
    except AssertionError as e:
        return f"'{name}'" in str(e)
    return False


SENSITIVITY_CASE = 4


def _sensitivity_case():
    """One probabilistic B = 3 case for (a), (b) and (c), so that they share one set of oracle gradients.  Latents (2, 2, 0, 0): the
    posterior's decoder past its last latent head reaches no loss term, so the whole gradient of those kernels is their L2 term --
    the only place where 2*lambda*w (1e-3 in norm) is visible beside data gradients of norm 1e2..1e4."""
    c = CASES[SENSITIVITY_CASE]
    assert c["B"] == 3 and c["prob"] and c["lat"] == (2, 2, 0, 0), c
    return c


def test_rule_rejects_a_gradient_that_lacks_one_samples_share():
    """(a) a fan-out / batch-tail bug drops the last sample's contribution to a shared gradient slot.  Samples are independent
    (InstanceNorm), so the gradient is mean_b(g_b) + L2: the oracle on the first two samples gives (g_0 + g_1) / 2 + L2.  The
    per-parameter rule rejects it for a deep conv kernel, an InstanceNorm beta and an SE conv7.bias; beta and bias carry 3e-4 of the
    whole gradient's norm each, and the whole-vector check alone lets them through."""
    c = _sensitivity_case()
    r = _oracle_alone(c["i"])
    sub = lambda m: {k: {q: t[:2] for q, t in v.items()} for k, v in m.items()}
    g2, _, _ = _oracle_eval(r["cfg"], c, r["P"], r["x"][:2], r["tgt"][:2], [e[:2] for e in r["eps"]],
                            None if r["dm"] is None else sub(r["dm"]), torch.float64, masks=sub(r["masks"]))
    small = ("prior.sersd1.norm1.beta", "prior.sersd1.conv7.bias")
    for name in ("prior.serse4.conv2.kernel",) + small:
        l2 = 2.0 * r["cfg"].l2_kernel * r["P"][name].double() if name.endswith(".kernel") else 0.0
        g = (g2[name] - l2) * (2.0 / 3.0) + l2
        gh = dict(r["g64"]); gh[name] = g
        e = float((g - r["g64"][name]).norm() / r["g64"][name].norm())
        print(f"(a) {name}: relative error {e:.3f}, whole-vector rule rejects: {_vector_rule_rejects(gh, r['g64'], r['g32'])}")
        assert _rule_rejects(r, name, g), name
        if name in small:
            assert not _vector_rule_rejects(gh, r["g64"], r["g32"]), name          # a vector norm would let it through


def test_rule_rejects_a_gradient_without_its_l2_term():
    """(b) the regulariser's share 2*lambda*w missing from one kernel's gradient: a kernel of the posterior's pruned decoder, which
    owns no other gradient (see _sensitivity_case).  Its norm is 1.3e-6 of the largest parameter gradient's, above the 1e-6 under
    which _check_grads treats a gradient as numerically zero."""
    c = _sensitivity_case()
    r = _oracle_alone(c["i"])
    name = "posterior.dec_hi2.kernel"
    g = r["g64"][name] - 2.0 * r["cfg"].l2_kernel * r["P"][name].double()
    gmax = max(float(v.norm()) for v in r["g64"].values() if v is not None)
    print(f"(b) {name}: relative error {float((g - r['g64'][name]).norm() / r['g64'][name].norm()):.4f}, "
          f"norm / largest norm {float(r['g64'][name].norm()) / gmax:.2e}")
    assert _rule_rejects(r, name, g)


def test_rule_rejects_a_posterior_gradient_without_the_kl_term():
    """(c) the KL term's path into the posterior cut (a latent head whose gradient slot the KL backward never reached)."""
    c = _sensitivity_case()
    r = _oracle_alone(c["i"])
    g0, _, _ = _oracle_eval(r["cfg"], c, r["P"], r["x"], r["tgt"], r["eps"], r["dm"], torch.float64, masks=r["masks"], kl_weight=0.0)
    name = "posterior.mu_logsig2.kernel"
    print(f"(c) {name}: relative error {float((g0[name] - r['g64'][name]).norm() / r['g64'][name].norm()):.3f}")
    assert _rule_rejects(r, name, g0[name])


# ---- the product (GPU) -----------------------------------------------------------------------------------------------------------
def _loss(m, c, focal, tgt, out):
    if c["prob"]:
        det, kl = out
        return focal(tgt, det) + 10.0 * PKG.losses.EvidenceLowerBound().loss(None, kl) + m.regularization_loss()
    return focal(tgt, out) + m.regularization_loss()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_train_step_fp32_against_oracle(dev, case):
    c, t0 = case, time.time()
    cfg = _config(c)
    P, x, tgt, eps = _inputs(c, cfg)
    m = build_m1(cfg, dev)
    names = {k.replace("m1_model.", "") for k, _ in m.named_parameters()}
    assert names == set(P), (sorted(names - set(P))[:5], sorted(set(P) - names)[:5])
    load_params_into(m, P)
    m.seed_dropout(4000 + c["i"])
    focal = PKG.losses.Focal(alpha=list(ALPHA[c["nc"]]), gamma=2.0).loss
    xs, ts = x.to(dev).requires_grad_(True), tgt.to(dev)
    kw = {"eps_q": [e.to(dev) for e in eps]} if c["prob"] else {}

    # -- the autograd path
    with activation_pattern(m) as ap:
        out = m(xs, **kw)
    assert bool(ap.drop) == (c["drop"] > 0)
    loss = _loss(m, c, focal, ts, out)
    loss.backward()
    torch.cuda.synchronize()
    t_gpu = time.time() - t0
    orc = _oracle_loss_and_grads(cfg, P, x, tgt, eps, masks=ap.masks, drop_masks=ap.oracle_drop_masks(), flip_skip=(".out",),
                                 input_grad=True, focal_alpha=ALPHA[c["nc"]])
    loss_o, o, g64 = orc[torch.float64]
    g32 = orc[torch.float32][2]
    gx64, gx32 = orc["input_grad"][torch.float64], orc["input_grad"][torch.float32]
    nc = c["nc"]
    if c["prob"]:
        assert m.m1_model.stack_passes                                  # the four passes run stacked into two, as in training
        det, kl = out
        tc = m.references.m1_model['prob_train_conv']
        assert float((tc.double().cpu() - o["prob_train_conv"]).abs().max()) < 1e-3
        assert abs(float(kl) - float(o["prob_kl"])) < 1e-3 * max(1.0, abs(float(o["prob_kl"])))
        assert float((det.double().cpu() - o["prob_softmax"]).abs().max()) < 1e-3
    else:
        det = out
        lg = m.references.m1_model['logits']
        assert float((lg.double().cpu() - o["logits"]).abs().max()) < 1e-3
        assert det.shape[-1] == (4 * nc if c["deep"] else nc)
        assert float((det.double().cpu() - o["y_softmax"]).abs().max()) < 1e-3
    assert abs(float(loss.detach()) - float(loss_o)) < 1e-3 * abs(float(loss_o)), (float(loss.detach()), float(loss_o))

    rep = {}
    relaxed = _check_grads(m, g64, g32, max_relaxed_tol=MAX_RELAXED_TOL, report=rep)
    assert relaxed <= MAX_RELAXED_SHARE * rep["params"], (relaxed, rep["params"])
    ex, tolx = _input_rule(xs.grad, gx64, gx32)
    assert tolx <= MAX_RELAXED_TOL and ex <= tolx, ("input gradient", ex, tolx)

    # -- the training path: the same model, the same dropout draw (the stream has not moved)
    first = [t.detach().clone() for t in (out if c["prob"] else [out])]
    for p in m.parameters():
        p.grad = None
    xs.grad = None
    opt = PKG.optim.Adam(learning_rate=1e-3, amsgrad=True)
    m.compile(optimizer=opt, loss=[focal], loss_weights=[1.0])          # binds the parameters to the flat buffers
    opt.zero_grad()
    out2 = m(xs, **kw)
    _loss(m, c, focal, ts, out2).backward()
    opt.flatp.gather_grads()
    torch.cuda.synchronize()
    for a, b in zip(first, out2 if c["prob"] else [out2]):
        assert torch.equal(a, b.detach())                               # the same forward: the pattern and the oracle result hold
    rep2 = {}
    relaxed2 = _check_grads(FlatGradView(m, opt.flatp), g64, g32, max_relaxed_tol=MAX_RELAXED_TOL, report=rep2)
    assert relaxed2 == relaxed
    ex2, _ = _input_rule(xs.grad, gx64, gx32)
    assert ex2 <= tolx, ("input gradient, training path", ex2, tolx)
    nflip, ntot = orc["flips"]
    w1, w2 = rep["worst"], rep2["worst"]
    print(f"train fuzz m{c['i']} {'prob' if c['prob'] else 'det'} B={c['B']} {c['dims']} f={c['filters']} drop={c['drop']}: "
          f"autograd worst {w1[0]} {w1[1]:.2e} / {w1[2]:.2e}, flat worst {w2[0]} {w2[1]:.2e} / {w2[2]:.2e}, "
          f"input {ex:.2e} / {ex2:.2e} / {tolx:.2e}, relaxed {relaxed} of {rep['params']}, flips {nflip} of {ntot}, "
          f"{time.time() - t0:.1f} s ({t_gpu:.1f} s before the oracle)")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_train_step_bf16_paths_agree_and_repeat(dev, case):
    c = case
    cfg = _config(c)
    P, x, tgt, eps = _inputs(c, cfg)
    m = build_m1(cfg, dev, dtype=torch.bfloat16)
    load_params_into(m, P)
    m.seed_dropout(4000 + c["i"])
    focal = PKG.losses.Focal(alpha=list(ALPHA[c["nc"]]), gamma=2.0).loss
    xs, ts = x.to(dev), tgt.to(dev)
    kw = {"eps_q": [e.to(dev) for e in eps]} if c["prob"] else {}

    def run(grads):
        out = m(xs, **kw)
        _loss(m, c, focal, ts, out).backward()
        g = grads()
        torch.cuda.synchronize()
        outs = [t.detach().clone() for t in (out if c["prob"] else [out])]
        for t in outs + [v for v in g.values() if v is not None]:
            assert bool(torch.isfinite(t).all())
        return outs, g

    def same(a, b, what):
        for u, v in zip(a[0], b[0]):
            assert torch.equal(u, v), what
        assert a[1].keys() == b[1].keys()
        for n in a[1]:
            assert (a[1][n] is None) == (b[1][n] is None) and (a[1][n] is None or torch.equal(a[1][n], b[1][n])), (what, n)

    def autograd_grads():
        g = {n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in m.named_parameters()}
        for p in m.parameters():
            p.grad = None
        return g
    ref = run(autograd_grads)
    same(ref, run(autograd_grads), "autograd path, second run")

    opt = PKG.optim.Adam(learning_rate=1e-3, amsgrad=True)
    m.compile(optimizer=opt, loss=[focal], loss_weights=[1.0])
    byid = {id(p): gv for p, gv in zip(opt.flatp.params, opt.flatp.gviews)}

    def flat_grads():
        opt.flatp.gather_grads()
        g = {n: byid[id(p)].reshape(p.shape).clone() for n, p in m.named_parameters()}
        opt.zero_grad()
        return g
    opt.zero_grad()
    flat = run(flat_grads)
    same(flat, run(flat_grads), "training path, second run")
    for u, v in zip(ref[0], flat[0]):
        assert torch.equal(u, v)
    for n, g in flat[1].items():
        if ref[1][n] is None:
            assert float(g.abs().max()) == 0.0, n
            continue
        e = float((g - ref[1][n]).abs().max()) / (float(ref[1][n].abs().max()) + 1e-30)
        assert e < 1e-5, (n, e)
