"""Training state over several steps: every step of a short run against the fp64 oracle, and a trained model against a fresh twin.

Everything else in the suite that runs for more than one step compares the product with itself (bf16 with fp32, replay with eager):
a defect both sides share passes.  What only a second step exercises is state -- the cached weight panels behind a raw-pointer
update, the in-kernel draws of a new {seed, step}, Adam's bias correction at t >= 2, a learning rate that follows a schedule.  A
free-running comparison with an oracle trajectory is no tool for it (test_bench_parity.test_loss_curve_bf16_tracks_fp32_over_20_steps
records that a re-association in one kernel moves the curve by 1.4 %); two tools are immune:

* TEACHER FORCING (part 1, fp32, eager, C1 filters, batch 2, stacked passes, K = 3 steps, Adam(CosineDecayRestarts(1e-3, 2)), a new
  batch every step, the step written as bench.py writes it).  At every step the restatement of tests/step_ref.py starts from the
  product's own state S_t:
    1. gradients -- the oracle at the parameters S_t.flat, the restated latent draws of (seed, step t - 1, posterior.latent_stream_id
       + level), the product's activation pattern and dropout masks: train logits and KL within 1e-3, loss within 1e-3 relative, every
       parameter gradient under test_hip_model._check_grads (max(1e-3, 3 e32) per parameter), the caps of test_train_step_fuzz.py
       (flips <= max(3, 5e-6 of the elements), at most 5 % of the parameters relaxed, none above 1e-2).  The flat buffer holds the data
       gradient; the oracle differentiates data + L2, so 2*lambda*w (restated, fp64) is added before the comparison -- the product's
       own L2 term lives in the Adam kernel and is judged by 3.
    2. draws -- (dropout configuration) the masks of step t equal philox_ref.keep_mask(seed, t - 1, layer id, ...) and differ from
       those of step t - 1.
    3. update -- S_{t+1} against step_ref.adam_update(S_t, G_t): m, v, vhat, p - p_t element-wise under the bounds of
       test_ops_at_scale.test_adam_amsgrad_c3_parameter_count_against_fp64, per step (beta_1 / beta_2 as the fp32 numbers the kernel
       receives, see step_ref.py); the step counter, the {seed, step} pair, the device learning rate; the gradient of every parameter
       outside flatp.live_ranges() is exactly zero (it moves by L2 alone).
  Configurations: (a) the full probabilistic model (dense skip, deep supervision, latents (3,2,1,0), dropout 0, draws made in the
  kernels -- no eps_q), (b) the deterministic model with dropout 0.5 monte-carlo.  Two sensitivity runs patch Python only:
  ops.repack_all as a no-op must fail assertion 1 at step 2, a step without ops.step_advance must fail assertion 2 at step 2.

* A FRESH TWIN (part 2, README filters, probabilistic, dropout 0.5 monte-carlo, bits).  A model that has trained K steps runs one more
  step on a fixed batch and an evaluation at batch 1; a NEW model and optimiser, loaded with its parameters, m, v, vhat, step counter,
  {seed, step} and iterations (and built under the same dropout-layer / latent-stream ids: they are per-process counters and part of
  what the draws are a function of), runs the same step eagerly and the same evaluation.  Loss, flat gradient, new state and
  evaluation output must be torch.equal as integers.  This composes three documented claims: run-to-run determinism, the same bits
  from a packed and an unpacked first call, the same bits from eager and replay.  Cases: fp32 and bf16 eager with an evaluation at
  batch 1 between steps 2 and 3 (new panels registered in the middle of training); bf16 with the old model's steps as replays of a
  graph captured in bench.py's order, the evaluation once BEFORE the capture; the same with the first evaluation AFTER the capture
  (a geometry the captured re-pack does not cover: hip/panels.py packs it per call -- before that fix the second evaluation read
  panels of the weights before the replayed update; test_convs_at_scale.test_panel_first_met_after_a_captured_repack_is_not_served_
  stale is the op-level form); the guarded optimiser (global_clipnorm low enough to clip, skip_nonfinite), step_ctl included.

CPU (part 0): the restatement iterated alone lowers the loss; along that trajectory the fp32 oracle on the fp64 pattern meets the
relaxation caps at every step (the condition for asserting them on the GPU); three wrong restatements (no L2 term, t frozen at 1, the
learning rate of the step before) break the bounds of assertion 3, and the right one rounded to fp32 meets them.

What this file cannot see: the oracle part is fp32 and eager only; bf16 and replay are covered by bits alone (against the eager twin
of the same precision); nothing runs beyond K + 1 steps.  Measured figures: DESIGN.md section 4, "Training state over several steps"."""
import contextlib
import functools

import pytest
import torch

import step_ref as SR
from oracle import m1_oracle as O
from test_bench_parity import DIMS, README_FILTERS, _cfg
from test_hip_model import MAX_FLIP_FRACTION, _ball_target, _check_grads, _oracle_loss_and_grads
from test_train_step_fuzz import MAX_RELAXED_SHARE, MAX_RELAXED_TOL
from util import C1_FILTERS, PKG, activation_pattern, build_m1, load_params_into, ops, rnd

K = 3                                # steps of part 1 and of the old model of part 2
B = 2
SEED = 0x51A7E
LATENT_ID0 = 0x4C415400              # the oracle-only trajectory (CPU): the first core's streams; on the GPU the ids are read from the model
PARAM_SEED = {"prob": 211, "det": 212, "twin": 213}
FIXED, EVAL = 9, 10                  # batch numbers of the twin's step K + 1 and of its batch-1 evaluation
assert MAX_FLIP_FRACTION == 5e-6 and MAX_RELAXED_SHARE == 0.05 and MAX_RELAXED_TOL == 1e-2


@pytest.fixture(autouse=True)
def _ids_from_copies_of_the_counters(monkeypatch):
    """The dropout-layer and latent-stream ids are counted per process.  Every test of this file counts from the start (the ids of
    the first model of a process), so its draws -- and every figure it prints -- are the same alone and inside the whole suite, and
    the models of the tests that run after it draw what they drew before it existed."""
    NB, NW = PKG.unets.network_blocks, PKG.unets.networks
    monkeypatch.setattr(NB._DropoutBase, "_next_id", [1])
    monkeypatch.setattr(NW.M1Core, "_next_latent_id", [0])


def _schedule():
    return PKG.optim.CosineDecayRestarts(1e-3, first_decay_steps=2)      # 1e-3, 5e-4, then the restart: 1e-3 again at step 3


def _config(kind):
    if kind == "prob":
        return _cfg(True, filters=C1_FILTERS)
    if kind == "det":
        return _cfg(False, filters=C1_FILTERS, dropout_rate=0.5, dropout_mode="monte-carlo")
    return _cfg(True, filters=README_FILTERS, dropout_rate=0.5, dropout_mode="monte-carlo")


@functools.lru_cache(maxsize=None)
def _fixture(kind):
    """The fixture weights of a configuration, computed once and shared (read-only)."""
    return O.fixture_params(_config(kind), seed=PARAM_SEED[kind])


def _batch(cfg, t, n=B):
    """Batch number ``t``: a different input and target for every t."""
    x = rnd((n, *DIMS, 3), 300 + 10 * t)
    tgt = _ball_target((n, *DIMS), 301 + 10 * t)
    if cfg.probabilistic:
        x[..., 2] = tgt[..., 1]                                # label channel, like data_generators.py:82
    return x, tgt


# =====================================================================================================================================
# part 0 (CPU): the restatement alone
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def _oracle_trajectory(kind):
    """K steps of the restatement from O.fixture_params, computed once and shared (read-only) by the CPU tests."""
    cfg = _config(kind)
    P = _fixture(kind)
    lay = SR.layout_from_oracle(P)
    S, sched, steps = SR.new_state(lay, P), _schedule(), []

    def draws(t):
        if cfg.probabilistic:
            return SR.latent_draws(cfg, B, SEED, t - 1, LATENT_ID0), None
        return None, SR.det_drop_masks(cfg, B, SEED, t - 1)
    for t in range(1, K + 1):
        Pt = SR.unflatten(lay, S["p"])
        x, tgt = _batch(cfg, t)
        eps, dm = draws(t)
        loss, parts, g64, g32 = SR.oracle_pair(cfg, Pt, x, tgt, eps, dm)
        g_data = SR.split_l2(lay, cfg, S["p"], SR.flatten(lay, g64), -1)
        lr = SR.lr_of(sched, t - 1)
        S1 = SR.adam_update(lay, cfg, S, g_data, lr)
        steps.append(dict(S=S, S1=S1, g_data=g_data, lr=lr, loss=loss, P=Pt, g64=g64, g32=g32))
        S = S1
    # the loss of the first batch under the first step's draws, at the parameters after K steps
    x, tgt = _batch(cfg, 1)
    eps, dm = draws(1)
    final, _, _, _ = SR._eval(cfg, SR.unflatten(lay, S["p"]), x, tgt, eps, dm, torch.float64)
    return dict(cfg=cfg, lay=lay, steps=steps, final=final, sched=sched)


@pytest.mark.parametrize("kind", ["prob", "det"])
def test_restatement_alone_lowers_the_loss(kind):
    tr = _oracle_trajectory(kind)
    first = tr["steps"][0]["loss"]
    print(f"restatement alone ({kind}): losses of the steps' own batches {[round(s['loss'], 3) for s in tr['steps']]}, "
          f"first batch before {first:.4f} and after {K} steps {tr['final']:.4f}; lr {[s['lr'] for s in tr['steps']]}")
    assert tr["final"] < first
    assert [s["S1"]["t"] for s in tr["steps"]] == [2, 3, 4]
    lrs = [s["lr"] for s in tr["steps"]]
    assert lrs[0] == lrs[2] == SR.lr_of(1e-3, 0) and lrs[1] == SR.lr_of(5e-4, 0)        # the schedule restarts inside the run


@pytest.mark.parametrize("kind", ["prob", "det"])
def test_oracle_alone_meets_the_relaxation_caps_along_the_trajectory(kind):
    """At every step: at most 5 % of the parameters relaxed above 1e-3, none above 1e-2 (test_train_step_fuzz.py's caps)."""
    tr = _oracle_trajectory(kind)
    for t, s in enumerate(tr["steps"], 1):
        rep = {}
        relaxed = _check_grads(SR.GradDictView(s["P"], s["g64"]), s["g64"], s["g32"], strip=(), max_relaxed_tol=MAX_RELAXED_TOL, report=rep)
        print(f"oracle alone ({kind}) step {t}: {relaxed} of {rep['params']} parameters relaxed, largest tolerance {rep['max_tol']:.2e}")
        assert relaxed <= MAX_RELAXED_SHARE * rep["params"], (t, relaxed, rep["params"])


def _as_fp32(S):
    return {k: (v.float().double() if torch.is_tensor(v) else v) for k, v in S.items()}


def test_plain_fp32_recurrence_meets_the_moment_bounds_along_the_trajectory():
    """The condition for asserting the bounds of m, v and vhat on the GPU: the recurrence written in plain fp32 tensor arithmetic
    (no fused multiply-add, the fp32 betas, the state and the gradient rounded to fp32 as the device holds them) stays inside them
    at every step of the oracle-only trajectory -- the steps at which a gradient that changed sign leaves m a small difference."""
    tr = _oracle_trajectory("prob")
    lay, cfg = tr["lay"], tr["cfg"]
    b1, b2, one = torch.tensor(SR.BETA_1).float(), torch.tensor(SR.BETA_2).float(), torch.tensor(1.0)
    for t, s in enumerate(tr["steps"], 1):
        S = _as_fp32(s["S"])
        g = s["g_data"].float()
        ref = SR.adam_update(lay, cfg, S, g, s["lr"])
        gr = g + 2.0 * SR.l2_vector(lay, cfg, torch.float32) * S["p"].float()
        m = b1 * S["m"].float() + (one - b1) * gr
        v = b2 * S["v"].float() + (one - b2) * gr * gr
        got = {"m": m, "v": v, "vhat": torch.maximum(S["vhat"].float(), v), "p": ref["p"].float(), "t": ref["t"]}
        rep = {}
        SR.check_state(got, ref, S, what=f"plain fp32, step {t}", report=rep)
        print(f"plain fp32 recurrence step {t}: |error| / bound m {rep['m']:.3f} v {rep['v']:.3f} vhat {rep['vhat']:.3f}")


@pytest.mark.parametrize("case,step", [("no_l2", 1), ("t_frozen", 2), ("stale_lr", 2)])
def test_state_bounds_reject_a_wrong_update(case, step):
    """The bounds of assertion 3 (step_ref.check_state) pass the restated update rounded to fp32 and reject: the L2 term dropped from
    the update; t frozen at 1 (the bias correction of step 2 with t = 1); the learning rate of step t - 1 used at step t."""
    tr = _oracle_trajectory("prob")
    lay, cfg, s = tr["lay"], tr["cfg"], tr["steps"][step - 1]
    rep = {}
    SR.check_state(_as_fp32(s["S1"]), s["S1"], s["S"], what="restatement rounded to fp32", report=rep)
    assert max(rep.values()) <= 1.0
    wrong = SR.adam_update(lay, cfg, s["S"], s["g_data"],
                           lr=SR.lr_of(tr["sched"], step - 2) if case == "stale_lr" else s["lr"],
                           t=1 if case == "t_frozen" else None, l2=case != "no_l2")
    if case == "stale_lr":
        assert SR.lr_of(tr["sched"], step - 2) != s["lr"]
    rep = {}
    with pytest.raises(AssertionError) as e:
        SR.check_state(_as_fp32(wrong), s["S1"], s["S"], what=case, report=rep)
    print(f"{case} at step {step}: worst |error| / bound {({k: round(v, 2) for k, v in rep.items()})}; {str(e.value)[:160]}")


# =====================================================================================================================================
# the product (GPU)
# =====================================================================================================================================
class StepMismatch(AssertionError):
    """An assertion of part 1 that failed, by name ('gradients', 'draws', 'update') and step."""

    def __init__(self, which, step, msg):
        super().__init__(f"step {step}, assertion '{which}': {msg}")
        self.which, self.step = which, step


@contextlib.contextmanager
def _named(which, step):
    try:
        yield
    except StepMismatch:
        raise
    except AssertionError as e:
        raise StepMismatch(which, step, str(e)) from e


def _make(dev, kind, dtype=torch.float32, **opt_kw):
    cfg = _config(kind)
    P = _fixture(kind)
    # (every weight is loaded below: a zero initializer spares the QR of the orthogonal one)
    m = build_m1(cfg, dev, dtype=dtype, kernel_initializer=PKG.initializers.Zeros())
    names = {k.replace("m1_model.", "") for k, _ in m.named_parameters()}
    assert names == set(P), (sorted(names - set(P))[:5], sorted(set(P) - names)[:5])
    load_params_into(m, P)
    m.seed_dropout(SEED)
    opt = PKG.optim.Adam(learning_rate=_schedule(), amsgrad=True, **opt_kw)
    focal = PKG.losses.Focal(alpha=[0.75, 0.25], gamma=2.0).loss
    if cfg.probabilistic:
        m.compile(optimizer=opt, loss=[focal, PKG.losses.EvidenceLowerBound().loss], loss_weights=[1.0, 10.0])
    else:
        m.compile(optimizer=opt, loss=[focal], loss_weights=[1.0])
    m.train()
    return cfg, m, opt


def _state(m, opt):
    """flatp.flat, m, v, vhat, step_dev, rng_state as test_bench_parity.test_graph_replay_equals_eager_steps lists them (guarded: and
    the control record)."""
    return [opt.flatp.flat, opt.m, opt.v, opt.vhat, opt.step_dev, m.rng_state] + ([opt.step_ctl] if opt.guarded else [])


STATE_NAMES = ["parameters", "adam m", "adam v", "adam vhat", "step counter", "rng state", "step_ctl"]


def _snap(m, opt):
    torch.cuda.synchronize()
    return [t.detach().clone() for t in _state(m, opt)]


def _host_state(snap, n):
    return {"p": snap[0][:n].cpu(), "m": snap[1][:n].cpu(), "v": snap[2][:n].cpu(), "vhat": snap[3][:n].cpu(), "t": int(snap[4])}


# ---- part 1: teacher-forced steps ---------------------------------------------------------------------------------------------------
def _teacher_forced_steps(dev, kind, checks=("gradients", "draws", "update"), advance=True, steps=K):
    """``steps`` steps of configuration ``kind``, each followed by the assertions named in ``checks``; returns one report per step."""
    NB = PKG.unets.network_blocks
    cfg, m, opt = _make(dev, kind)
    lay = SR.layout_from_flatp(m, opt.flatp)
    n, sched, prob = lay.n, opt.learning_rate, cfg.probabilistic
    layers = {name.replace("m1_model.", ""): (mod.layer_id, mod.rate) for name, mod in m.named_modules() if isinstance(mod, NB._DropoutBase)}
    assert m.m1_model.stack_passes or not prob
    prev_masks, reports = None, []
    for t in range(1, steps + 1):
        x, tgt = _batch(cfg, t)
        xs, ts = x.to(dev), tgt.to(dev)
        S0 = _snap(m, opt)
        # -- the step, as bench.py writes it (eager; the learning rate follows the schedule, the host counts the iterations)
        opt.zero_grad()
        with activation_pattern(m) as ap:
            outs = m(xs)
        total, _ = m.compute_loss(outs, {"detection": ts})
        reg = m.regularization_loss()
        total.backward()
        opt.flatp.gather_grads()
        opt.exchange()
        torch.cuda.synchronize()
        G = opt.flatp.grad[:n].detach().cpu().clone()
        head = m.references.m1_model["prob_train_conv" if prob else "logits"].detach().double().cpu()
        kl = float(outs[1]) if prob else None
        loss = float(total.detach()) + float(reg.detach())
        opt.set_lr_device()
        opt.apply_flat()
        if advance:
            ops.step_advance(None, m.rng_state)
        opt.iterations += 1
        S1 = _snap(m, opt)
        lr_dev = float(opt.lr_dev)
        before, got = _host_state(S0, n), _host_state(S1, n)
        rep = {"step": t}

        if "gradients" in checks:
            with _named("gradients", t):
                Pt = SR.unflatten(lay, S0[0][:n])
                eps = SR.latent_draws(cfg, B, SEED, t - 1, m.m1_model.posterior.latent_stream_id) if prob else None
                assert bool(ap.drop) == (cfg.dropout_rate > 0)
                dm = ap.oracle_drop_masks() if ap.drop else None
                orc = _oracle_loss_and_grads(cfg, Pt, x, tgt, eps, masks=ap.masks, drop_masks=dm, flip_skip=(".out",) if dm else ())
                loss_o, o, g64 = orc[torch.float64]
                rep["head"] = float((head - o["prob_train_conv" if prob else "logits"]).abs().max())
                assert rep["head"] < 1e-3, ("train logits", rep["head"])
                if prob:
                    rep["kl"] = abs(kl - float(o["prob_kl"])) / max(1.0, abs(float(o["prob_kl"])))
                    assert rep["kl"] < 1e-3, ("KL", kl, float(o["prob_kl"]))
                rep["loss"] = abs(loss - float(loss_o)) / abs(float(loss_o))
                assert rep["loss"] < 1e-3, ("loss", loss, float(loss_o))
                # the regularised gradient: the flat buffer's data term + the restated 2 lambda w (module docstring, 1.)
                gh = SR.unflatten(lay, SR.split_l2(lay, cfg, before["p"], G, +1))
                r = {}
                relaxed = _check_grads(SR.GradDictView(Pt, gh), g64, orc[torch.float32][2], strip=(), max_relaxed_tol=MAX_RELAXED_TOL, report=r)
                assert relaxed <= MAX_RELAXED_SHARE * r["params"], (relaxed, r["params"])
                rep.update(worst=r["worst"], relaxed=relaxed, params=r["params"], flips=orc["flips"])

        if "draws" in checks and not prob:
            with _named("draws", t):
                cur = {tag: per[0] for tag, per in ap.drop.items()}
                assert set(cur) == set(layers) and len(cur) == 8, (sorted(cur), sorted(layers))
                assert layers["core.dropd0"][1] == cfg.dropout_rate / 2                 # p / 2 behind sersd0 (networks.py:523)
                for tag, (lid, rate) in layers.items():
                    keep = SR.keep_decisions(SEED, t - 1, lid, cur[tag].shape, rate)
                    assert torch.equal(cur[tag], keep), (tag, lid, int((cur[tag] != keep).sum()), keep.numel())
                    assert prev_masks is None or not torch.equal(cur[tag], prev_masks[tag]), (tag, "the masks of the step before")
                prev_masks = cur

        if "update" in checks:
            with _named("update", t):
                lr = SR.lr_of(sched, t - 1)
                assert lr_dev == lr, (lr_dev, lr)
                assert before["t"] == t and got["t"] == t + 1, (before["t"], got["t"])
                ref = SR.adam_update(lay, cfg, before, G, lr)
                rep.update(SR.check_state(got, ref, before, what=f"{kind} step {t}"))
                r0, r1 = S0[5].cpu().tolist(), S1[5].cpu().tolist()
                assert r0 == [SEED, t - 1] and r1 == [SEED, t], (r0, r1)
                live = torch.zeros(n, dtype=torch.bool)
                for a, b in opt.flatp.live_ranges():
                    live[a:min(b, n)] = True
                assert not bool(G[~live].any()), "a parameter outside flatp.live_ranges() received a gradient"
                rep["dead"] = int((~live).sum())
                assert (rep["dead"] > 0) == prob                 # the layers behind sersd0 / logits of the probabilistic cores
        reports.append(rep)
        w = rep.get("worst", ("-", 0.0, 1e-3))
        print(f"teacher-forced {kind} step {t}: logits {rep.get('head', -1):.2e} loss {rep.get('loss', -1):.2e} KL {rep.get('kl', -1):.2e}; "
              f"worst parameter {w[0]} {w[1]:.2e} / {w[2]:.2e}, relaxed {rep.get('relaxed', -1)} of {rep.get('params', -1)}, "
              f"flips {rep.get('flips', -1)}; |error| / bound: m {rep.get('m', -1):.3f} v {rep.get('v', -1):.3f} "
              f"vhat {rep.get('vhat', -1):.3f} p {rep.get('p', -1):.3f}; lr {lr_dev:.3e}, dead elements {rep.get('dead', -1)}")
    return reports


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["prob", "det"])
def test_teacher_forced_steps_against_the_oracle(dev, kind):
    try:
        reports = _teacher_forced_steps(dev, kind)
    finally:
        ops.drop_deferred(); ops.invalidate_panels()
    assert [r["step"] for r in reports] == [1, 2, 3]


@pytest.mark.gpu
def test_teacher_forcing_notices_a_step_without_repack(dev, monkeypatch):
    """Python only: with ops.repack_all a no-op the second forward pass reads the panels packed from the initial weights."""
    monkeypatch.setattr(ops, "repack_all", lambda: None)
    try:
        with pytest.raises(StepMismatch) as e:
            _teacher_forced_steps(dev, "det", checks=("gradients",), steps=2)
    finally:
        monkeypatch.undo()
        ops.drop_deferred(); ops.invalidate_panels()
    print(str(e.value)[:300])
    assert (e.value.which, e.value.step) == ("gradients", 2)


@pytest.mark.gpu
def test_teacher_forcing_notices_a_step_without_step_advance(dev):
    """Python only: the {seed, step} pair stays where it was, the second step draws the first step's masks again."""
    try:
        with pytest.raises(StepMismatch) as e:
            _teacher_forced_steps(dev, "det", checks=("gradients", "draws"), advance=False, steps=2)
    finally:
        ops.drop_deferred(); ops.invalidate_panels()
    print(str(e.value)[:300])
    assert (e.value.which, e.value.step) == ("draws", 2)


# ---- part 2: the fresh twin ----------------------------------------------------------------------------------------------------------
def _bits(t):
    t = t.detach().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class _Run:
    """A model, its optimiser and static input buffers; ``body`` is bench.py's step()."""

    def __init__(self, dev, dtype, **opt_kw):
        self.dev, self.dtype = dev, dtype
        self.cfg, self.m, self.opt = _make(dev, "twin", dtype, **opt_kw)
        x, tgt = _batch(self.cfg, 1)
        self.xs, self.ts = ops.cast(x.to(dev).contiguous(), dtype), tgt.to(dev)
        self.x1 = _batch(self.cfg, EVAL, n=1)[0].to(dev)
        self.loss = torch.zeros(1, device=dev)
        self.detect = self.m.get_detect_model()
        self.graph = None

    def feed(self, t):
        x, tgt = _batch(self.cfg, t)
        self.xs.copy_(ops.cast(x.to(self.dev).contiguous(), self.dtype))
        self.ts.copy_(tgt.to(self.dev))
        self.opt.set_lr_device()                                # outside the captured step: the schedule moves the device value

    def body(self):
        m, opt = self.m, self.opt
        opt.zero_grad()
        outs = m(self.xs)
        total, _ = m.compute_loss(outs, {"detection": self.ts})
        total.backward()
        opt.flatp.gather_grads()
        self.loss.copy_(total.detach().reshape(1))
        opt.exchange()
        opt.apply_flat()
        ops.step_advance(None, m.rng_state)

    def eager(self, t):
        self.feed(t)
        self.body()
        self.opt.iterations += 1

    def capture(self, t):
        """bench.py's capture(): one eager step on a side stream (it counts as a step), then the capture."""
        self.feed(t)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self.body()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self.opt.iterations += 1
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.body()
        torch.cuda.synchronize()

    def replay(self, t):
        self.feed(t)
        self.graph.replay()
        self.opt.iterations += 1

    def evaluate(self):
        with torch.no_grad():
            out = self.detect.predict(self.x1)
        torch.cuda.synchronize()
        return out.detach().clone()

    def result(self):
        torch.cuda.synchronize()
        return [self.loss.clone(), self.opt.flatp.grad.clone()] + _snap(self.m, self.opt)


TWIN_CASES = [("fp32-eager", torch.float32, "eager", {}), ("bf16-eager", torch.bfloat16, "eager", {}),
              ("bf16-replay-eval-before-capture", torch.bfloat16, "replay", {}),
              ("bf16-replay-eval-after-capture", torch.bfloat16, "replay_eval_after", {}),
              ("bf16-eager-guarded", torch.bfloat16, "eager", dict(global_clipnorm=1.0, skip_nonfinite=True))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,dtype,mode,opt_kw", TWIN_CASES, ids=[c[0] for c in TWIN_CASES])
def test_trained_model_equals_a_fresh_twin_built_from_its_state(dev, monkeypatch, name, dtype, mode, opt_kw):
    NB, NW = PKG.unets.network_blocks, PKG.unets.networks
    ids0 = list(NB._DropoutBase._next_id), list(NW.M1Core._next_latent_id)
    try:
        old = _Run(dev, dtype, **opt_kw)
        start = _snap(old.m, old.opt)
        if mode == "eager":
            old.eager(1); old.eager(2); old.evaluate(); old.eager(3)           # new panels registered in the middle of training
            final = old.eager
        elif mode == "replay":
            old.eager(1); old.eager(2); old.evaluate(); old.capture(3); old.replay(4)
            final = old.replay
        else:
            old.eager(1); old.eager(2); old.capture(3); old.replay(4)
            try:
                old.evaluate()                                                   # a geometry first met AFTER the capture
            except RuntimeError as e:                                            # (a clear refusal would be acceptable; a stale panel is not)
                assert "panel" in str(e), e
                return
            final = old.replay
        saved, iterations = _snap(old.m, old.opt), old.opt.iterations
        assert not any(torch.equal(a, b) for a, b in zip(saved, start))        # the steps moved every part of the state
        final(FIXED)
        want = old.result() + [old.evaluate()]
        if opt_kw:
            ctl = ops.read_step_ctl(old.opt.step_ctl)
            print(f"{name}: gradient norm {ctl['norm']:.3e}, clip coefficient {ctl['coef']:.3e}, skipped {ctl['skipped']}")
            assert ctl["apply"] == 1 and 0.0 < ctl["coef"] < 1.0, ctl       # the clip did trigger
        assert bool(torch.isfinite(want[0]).all()) and bool(torch.isfinite(want[-1]).all())

        ops.drop_deferred(); ops.invalidate_panels()
        # the twin: a new model and optimiser under the ids the old model was built under, loaded with the saved state
        monkeypatch.setattr(NB._DropoutBase, "_next_id", list(ids0[0]))
        monkeypatch.setattr(NW.M1Core, "_next_latent_id", list(ids0[1]))
        new = _Run(dev, dtype, **opt_kw)
        assert new.m.m1_model.posterior.latent_stream_id == old.m.m1_model.posterior.latent_stream_id
        with torch.no_grad():
            for dst, src in zip(_state(new.m, new.opt), saved):
                dst.copy_(src)
        new.opt.iterations = iterations
        new.eager(FIXED)
        got = new.result() + [new.evaluate()]
        names = ["loss", "flat gradient"] + STATE_NAMES[:len(saved)] + ["evaluation at batch 1"]
        assert len(names) == len(want) == len(got)
        for n_, a, b in zip(names, want, got):
            assert a.shape == b.shape and a.dtype == b.dtype, n_
            diff = int((_bits(a) != _bits(b)).sum())
            assert diff == 0, f"{name}: {n_}: {diff} of {a.numel()} elements differ between the trained model and its fresh twin"
    finally:
        monkeypatch.undo()
        ops.drop_deferred(); ops.invalidate_panels()
