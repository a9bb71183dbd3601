"""The guarded optimiser step: tf.keras' ``clipvalue`` / ``global_clipnorm`` and the non-finite skip of optim.Adam
(csrc/optim.hip: grad_norm_kernel, grad_control_kernel, adam_amsgrad_kernel<true>, step_inc_ctl_kernel).

* CPU: the fp64 restatement (tests/clip_ref.py) equals util.ref_adam_amsgrad_step exactly when nothing triggers, and does what the
  Keras formulas say on hand cases (parity with TensorFlow itself is NOT pinned: TensorFlow is not installed); constructor validation;
  trainer flags; the entry points reject bad arguments before any launch.
* GPU, op level: the kernels against the restatement -- never against the record the kernels wrote themselves.
* GPU, model level: a poisoned gradient buffer, a bad input batch end to end, the captured step, a reducer stub with grad_scale 0.5.

Bounds (none fitted to observed errors):
* norm: 5e-7 relative to the fp64 value = 4 fp32 ulps: one for each of the two fp32 roundings in gr (2*lambda*p, then the fused
  multiply-add), one for the final cast of the fp64 root, one spare.  The squares and their sum are fp64 in the kernel.  The norm of a
  later step is compared with the fp64 norm of what the kernel READ (the device's own weights before that step).
* p: rel_err < 1e-5, the bound of test_hip_ops.py::test_adam_amsgrad_matches_keras_formula.
* m, v, vhat: per element A_32 * |ref| + B_32 * rms(ref) of test_ops_at_scale.py.  beta_1 / beta_2 are handed to the kernel AND to the
  reference as the fp32 numbers the C ABI carries (float(np.float32(0.999))): 1 - fl(0.999) differs from 1e-3 by 1.3e-5 relative,
  which is a property of the argument type and not of the kernels under test.
* every clip is placed so that norm / clip is 2 or 0.5 (outside [0.9, 1.1]): rounding cannot flip the branch.
"""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import clip_ref
import util
from util import C1_STRIDES, PKG, ops, rel_err, rnd, assert_close_ew

T = importlib.import_module("prostatemr_3d-cad-cspca_amd.train_model")
L = PKG.hip.lib
A_32, B_32 = 1e-5, 4e-6                                   # test_ops_at_scale.py
NORM_REL = 5e-7
LK, LB, GS, LR, EPS = 1e-2, 3e-2, 0.5, 1e-2, 1e-7
B1, B2 = float(np.float32(0.9)), float(np.float32(0.999))


# =================================================================================================================================
# CPU
# =================================================================================================================================
def test_restatement_equals_the_plain_reference_when_nothing_triggers():
    n, nk, nb = 1003, 400, 200
    g = rnd((n,), 2).double()
    a = [rnd((n,), 1).double()] + [torch.zeros(n, dtype=torch.float64) for _ in range(3)]
    b = [t.clone() for t in a]
    t = 1
    for step in range(1, 4):
        a = list(util.ref_adam_amsgrad_step(a[0], g, *a[1:], step, nk, nb, LK, LB, GS, LR, B1, B2, EPS))
        *b, t, info = clip_ref.guarded_step(b[0], g, *b[1:], t, nk, nb, LK, LB, GS, LR, B1, B2, EPS, clipvalue=0.0, global_clipnorm=1e6,
                                            skip_nonfinite=True)
        assert info["coef"] == 1.0 and info["apply"] and t == step + 1
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_restatement_follows_the_keras_formulas_on_hand_cases():
    z = lambda *v: torch.tensor(v, dtype=torch.float64)
    g, p0, zero = z(3, 4, 0, 0), z(1, 1, 1, 1), z(0, 0, 0, 0)
    step = lambda **kw: clip_ref.guarded_step(p0, kw.pop("g", g), zero, zero, zero, 1, 0, 0, 0.0, 0.0, 1.0, LR, B1, B2, EPS, **kw)
    assert step(global_clipnorm=5.0)[5] == {"norm": 5.0, "coef": 1.0, "apply": True}           # norm == clip: not clipped
    assert step(global_clipnorm=2.5)[5] == {"norm": 5.0, "coef": 0.5, "apply": True}
    _, m, *_ = step(global_clipnorm=2.5)
    assert torch.allclose(m, (1 - B1) * 0.5 * g, rtol=1e-15, atol=0)
    info = step(clipvalue=3.5, global_clipnorm=1.0)[5]                                         # clamp first: (3, 3.5) has norm sqrt(21.25)
    assert info["norm"] == pytest.approx(21.25 ** 0.5, rel=1e-15) and info["coef"] == pytest.approx(21.25 ** -0.5, rel=1e-15)
    _, m, *_ = step(clipvalue=3.5)
    assert torch.allclose(m, (1 - B1) * z(3, 3.5, 0, 0), rtol=1e-15, atol=0)
    assert step(g=zero, global_clipnorm=1.0)[5] == {"norm": 0.0, "coef": 1.0, "apply": True}   # no 0/0
    for bad in (float("nan"), float("inf"), float("-inf")):
        gb = z(3, bad, 0, 0)
        p, m, v, h, t, info = step(g=gb, skip_nonfinite=True)
        assert not info["apply"] and t == 1 and p is p0 and m is zero
        info = step(g=gb, global_clipnorm=1.0)[5]
        assert info["apply"] and info["coef"] != info["coef"]                                   # tf.clip_by_global_norm: NaN
        assert step(g=gb)[5]["coef"] == 1.0
    assert step(g=z(3, float("inf"), 0, 0), clipvalue=4.0, skip_nonfinite=True)[5] == {"norm": 5.0, "coef": 1.0, "apply": True}
    assert step(g=z(1e200, 0, 0, 0), skip_nonfinite=True)[5]["apply"] is False                  # (fp64 overflows too: only fp32-range inputs are finite)


def test_constructor_validation():
    A = PKG.optim.Adam
    o = A()
    assert (o.clipvalue, o.global_clipnorm, o.skip_nonfinite, o.guarded, o.step_ctl) == (None, None, False, False, None)
    o = A(clipvalue=0.5, global_clipnorm=2, skip_nonfinite=True)
    assert (o.clipvalue, o.global_clipnorm, o.skip_nonfinite, o.guarded) == (0.5, 2.0, True, True)
    assert A(skip_nonfinite=True).guarded and A(clipvalue=1.0).guarded and A(global_clipnorm=1.0).guarded
    with pytest.raises(NotImplementedError, match="global_clipnorm"):
        A(clipnorm=1.0)
    for kw in ({"clipvalue": 0.0}, {"clipvalue": -1.0}, {"global_clipnorm": 0}, {"global_clipnorm": -2.0},
               {"global_clipnorm": float("nan")}, {"clipvalue": float("inf")}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            A(**kw)
    with pytest.raises(RuntimeError, match="skip_nonfinite"):
        A().grad_norm
    with pytest.raises(RuntimeError, match="bind"):
        A(skip_nonfinite=True).skipped_steps


def test_trainer_flags_and_defaults():
    a = T.build_parser().parse_args([])
    assert (a.GRAD_CLIP_NORM, a.GRAD_CLIP_VALUE, a.SKIP_NONFINITE) == (0.0, 0.0, 0)
    assert T.optimizer_kwargs(a) == dict(global_clipnorm=None, clipvalue=None, skip_nonfinite=False)
    assert not PKG.optim.Adam(**T.optimizer_kwargs(a)).guarded                                  # the defaults change nothing
    b = T.build_parser().parse_args("--GRAD_CLIP_NORM 2.5 --GRAD_CLIP_VALUE 0.25 --SKIP_NONFINITE 1".split())
    assert T.optimizer_kwargs(b) == dict(global_clipnorm=2.5, clipvalue=0.25, skip_nonfinite=True)
    with pytest.raises(ValueError, match="GRAD_CLIP_NORM"):
        T.optimizer_kwargs(T.build_parser().parse_args(["--GRAD_CLIP_NORM", "-1"]))
    for flag in ("--GRAD_CLIP_NORM", "--GRAD_CLIP_VALUE", "--SKIP_NONFINITE"):
        assert flag in T.__doc__


def test_bad_arguments_are_rejected_before_any_launch():
    """Null, n <= 0, misaligned buffers, a short workspace, clips that are negative / NaN / Inf: M1_ERR_BAD_ARG.  The addresses are
    made up -- a rejected call dereferences nothing and launches nothing (this test runs without a GPU)."""
    lib = L.load()
    ok, odd = 0x10000, 0x10004
    assert lib.m1_grad_norm_ws(0) == 0 and lib.m1_grad_norm_ws(-5) == 0
    assert lib.m1_grad_norm_ws(1) == 8 and lib.m1_grad_norm_ws(1015) == 8 and lib.m1_grad_norm_ws(1016) == 16
    assert lib.m1_grad_norm_ws(2_100_003) == 8 * 2048 == lib.m1_grad_norm_ws(67_254_246)        # the cap

    def norm(g=ok, p=ok, n=100, cv=0.0, cn=0.0, ws=ok, wsb=8, ctl=ok):
        return lib.m1_grad_norm(g, p, n, 10, 10, 0.0, 0.0, 1.0, cv, cn, 1, ws, wsb, ctl, None)
    for kw in (dict(g=None), dict(p=None), dict(ws=None), dict(ctl=None), dict(n=0), dict(n=-4), dict(g=odd), dict(p=odd), dict(ctl=odd),
               dict(ws=odd), dict(wsb=7), dict(n=1022, wsb=8), dict(cv=-1.0), dict(cn=-1.0), dict(cv=float("nan")), dict(cn=float("inf"))):
        assert norm(**kw) == -1, kw

    def adam(p=ok, g=ok, m=ok, v=ok, h=ok, n=100, lr=ok, step=ok, cv=0.0, ctl=ok):
        return lib.m1_adam_amsgrad_ctl(p, g, m, v, h, n, 10, 10, 0.0, 0.0, 1.0, lr, 0.9, 0.999, 1e-7, step, cv, ctl, None)
    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(h=None), dict(lr=None), dict(step=None), dict(ctl=None),
               dict(n=0), dict(p=odd), dict(g=odd), dict(m=odd), dict(v=odd), dict(h=odd), dict(ctl=odd), dict(cv=-0.5), dict(cv=float("nan"))):
        assert adam(**kw) == -1, kw
    assert lib.m1_step_advance_ctl(None, ok, None) == -1 and lib.m1_step_advance_ctl(ok, None, None) == -1


# =================================================================================================================================
# GPU, op level
# =================================================================================================================================
class State:
    """p, m, v, vhat, step counter, workspace and control record on the device: buffers of exactly n floats (the float4 body and the
    scalar tail of n % 4 elements both run)."""

    def __init__(self, dev, p0, g, nk, nb, lk=LK, lb=LB, gs=GS):
        self.n, self.nk, self.nb, self.lk, self.lb, self.gs = p0.numel(), nk, nb, lk, lb, gs
        self.p, self.g = p0.to(dev).clone(), g.to(dev).clone()
        self.m, self.v, self.h = (torch.zeros_like(self.p) for _ in range(3))
        self.lr = torch.tensor([LR], device=dev)
        self.step = torch.ones(1, dtype=torch.int32, device=dev)
        self.ws = torch.empty(ops.grad_norm_ws(self.n), dtype=torch.uint8, device=dev)
        self.ctl = ops.new_step_ctl(dev)

    def plain(self):
        ops.adam_amsgrad_(self.p, self.g, self.m, self.v, self.h, self.nk, self.nb, self.lk, self.lb, self.gs, self.lr, B1, B2, EPS, self.step)
        ops.step_advance(self.step, None)

    def guarded(self, cv=0.0, cn=0.0, guard=False):
        ops.grad_norm_(self.g, self.p, self.nk, self.nb, self.lk, self.lb, self.gs, cv, cn, guard, self.ws, self.ctl)
        ops.adam_amsgrad_ctl_(self.p, self.g, self.m, self.v, self.h, self.nk, self.nb, self.lk, self.lb, self.gs, self.lr, B1, B2, EPS,
                              self.step, cv, self.ctl)
        ops.step_advance_ctl(self.step, self.ctl)
        return ops.read_step_ctl(self.ctl)

    def bits(self):
        return [t.clone().view(torch.int32) for t in (self.p, self.m, self.v, self.h, self.step)]

    def ref_norm(self, cv=0.0):
        """fp64 norm of the clamped regularised gradient of the device's CURRENT weights"""
        gr = clip_ref.regularised_grad(self.p.double(), self.g.double(), self.nk, self.nb, self.lk, self.lb, self.gs)
        return float((clip_ref.clamp_value(gr, cv) ** 2).sum().sqrt())


def _same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _inputs(n, seed=1):
    return rnd((n,), seed), rnd((n,), seed + 1)


# (n, n_kernel, n_bias, M1_EW_BLOCKS or None)
SIZES = [(1, 1, 0, None), (3, 1, 1, None), (4, 2, 1, None), (1003, 400, 200, None), (10_007, 5_003, 1_206, 2),
         (2_100_003, 1_000_001, 1_206, None)]
# (clipvalue, global_clipnorm as a multiple of the first step's fp64 norm)
MODES = {"norm": (0.0, 0.5), "value": (0.7, 0.0), "value+norm": (0.7, 0.5), "norm-above": (0.0, 2.0)}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n,nk,nb,cap", SIZES)
def test_guarded_step_matches_the_restatement(dev, n, nk, nb, cap, mode):
    """Three steps.  n = 10,007 runs with the norm pass capped at 2 blocks (several grid-stride trips per thread, both range edges inside a
    float4); n = 2,100,003 fills all 2048 blocks: the control pass folds more than 256 partials."""
    cv, ratio = MODES[mode]
    assert n != 10_007 or (nk % 4 and (nk + nb) % 4)
    p0, g = _inputs(n)
    s = State(dev, p0, g, nk, nb)
    cn = ratio * s.ref_norm(cv)
    r = [p0.to(dev).double()] + [torch.zeros(n, dtype=torch.float64, device=dev) for _ in range(3)]
    t, gd64 = 1, g.to(dev).double()
    with ops.config(**({"M1_EW_BLOCKS": cap} if cap else {})):
        for step in range(3):
            want_norm = s.ref_norm(cv)
            assert not (0.9 <= want_norm / cn <= 1.1) if cn else True
            rec = s.guarded(cv, cn, guard=True)
            *r, t, info = clip_ref.guarded_step(r[0], gd64, *r[1:], t, nk, nb, LK, LB, GS, LR, B1, B2, EPS, cv, cn, True)
            print(f"n={n} {mode} step {step + 1}: norm {rec['norm']:.9g} (fp64 {want_norm:.12g}, rel {abs(rec['norm'] - want_norm) / want_norm:.2e}) "
                  f"coef {rec['coef']:.9g} (ref {info['coef']:.9g})")
            assert abs(rec["norm"] - want_norm) <= NORM_REL * want_norm
            assert rec["apply"] == 1 and rec["skipped"] == 0
            if ratio == 0.0 or ratio > 1:
                assert rec["coef"] == 1.0 and info["coef"] == 1.0
            else:
                assert info["coef"] < 1 and abs(rec["coef"] - info["coef"]) <= NORM_REL * info["coef"]
    assert int(s.step) == 4 and t == 4
    assert rel_err(s.p, r[0]) < 1e-5
    for name, got, ref in (("m", s.m, r[1]), ("v", s.v, r[2]), ("vhat", s.h, r[3])):
        assert_close_ew(got, ref, A_32, B_32, what=f"n={n} {mode} {name}")
    assert torch.equal(s.g.cpu(), g)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 4, 1003])
def test_exact_norm_and_coefficient(dev, n):
    """g = (3, 4, 0, ...), no regulariser: the norm is 5.0f exactly; clip 5 leaves coef at 1.0f (norm > clip is false), clip 2.5 gives
    exactly 0.5, and the first moment is then (1 - beta_1) * 0.5 * g in fp32."""
    g = torch.zeros(n); g[0], g[1] = 3.0, 4.0
    for clip, coef in ((5.0, 1.0), (2.5, 0.5)):
        s = State(dev, rnd((n,), 3), g, n // 2, 1, lk=0.0, lb=0.0, gs=1.0)
        rec = s.guarded(0.0, clip, True)
        assert rec == {"norm": 5.0, "coef": coef, "apply": 1, "skipped": 0}
        want = (torch.tensor(1.0) - torch.tensor(B1, dtype=torch.float32)) * (g * coef)
        assert torch.equal(s.m.cpu(), want) and int(s.step) == 2


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 1003])
def test_zero_gradient(dev, n):
    """norm = 0, coef = 1 (no 0 / 0), the step is applied and moves nothing."""
    p0 = rnd((n,), 4)
    s = State(dev, p0, torch.zeros(n), n // 2, 1, lk=0.0, lb=0.0)
    rec = s.guarded(0.3, 1.0, True)
    assert rec == {"norm": 0.0, "coef": 1.0, "apply": 1, "skipped": 0}
    assert torch.equal(s.p.cpu(), p0) and not s.m.any() and not s.v.any() and not s.h.any() and int(s.step) == 2


@pytest.mark.gpu
@pytest.mark.parametrize("n,nk,nb,cap", SIZES[3:5])
def test_bit_equal_to_the_plain_update_when_nothing_triggers(dev, n, nk, nb, cap):
    """Guard on, a clip far above the norm, no clamp: coef is 1.0f and clamp(gr, +Inf) is gr, so the controlled kernel computes what
    m1_adam_amsgrad computes -- the same device function -- bit for bit, over three steps."""
    p0, g = _inputs(n, 5)
    a, b = State(dev, p0, g, nk, nb), State(dev, p0, g, nk, nb)
    with ops.config(**({"M1_EW_BLOCKS": cap} if cap else {})):
        for _ in range(3):
            a.plain()
            rec = b.guarded(0.0, 1e6, True)
            assert rec["coef"] == 1.0 and rec["apply"] == 1
            assert _same_bits(a.bits(), b.bits())
    assert int(b.step) == 4


POISON = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}
# (n, index): element 0; the tail past the last float4; the last element of a buffer without a tail
PLACES = [(1003, 0), (1003, 1002), (1000, 999), (4, 3), (1, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(POISON))
@pytest.mark.parametrize("n,at", PLACES)
def test_nonfinite_gradient_is_skipped_and_leaves_no_trace(dev, n, at, kind):
    p0, g = _inputs(n, 6)
    bad = g.clone(); bad[at] = POISON[kind]
    nk, nb = n * 2 // 5, n // 5
    s, twin = State(dev, p0, g, nk, nb), State(dev, p0, g, nk, nb)
    s.guarded(0.0, 0.0, True); twin.guarded(0.0, 0.0, True)            # one clean step first: non-zero moments
    before = s.bits()
    s.g.copy_(bad)
    rec = s.guarded(0.0, 0.0, True)
    assert rec["apply"] == 0 and rec["skipped"] == 1 and not np.isfinite(rec["norm"])
    assert _same_bits(before, s.bits()) and int(s.step) == 2           # p, m, v, vhat and Adam's t keep their bits
    rec = s.guarded(0.0, 0.5 * twin.ref_norm(), True)                  # skipped again, with the norm clip on as well
    assert rec["apply"] == 0 and rec["skipped"] == 2 and _same_bits(before, s.bits())
    s.g.copy_(g)
    rec, rec_t = s.guarded(0.0, 0.0, True), twin.guarded(0.0, 0.0, True)
    assert rec["apply"] == 1 and rec["skipped"] == 2 and rec["norm"] == rec_t["norm"]
    assert _same_bits(s.bits(), twin.bits()) and int(s.step) == 3      # as if the bad steps had never happened


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(POISON))
def test_guard_off_poisons_like_the_plain_update_and_like_tensorflow(dev, kind):
    n, nk, nb = 1003, 400, 200
    p0, g = _inputs(n, 7)
    g[1002] = POISON[kind]
    a, b = State(dev, p0, g, nk, nb), State(dev, p0, g, nk, nb)
    a.plain()
    rec = b.guarded(0.0, 0.0, False)                                   # no clip, no guard: the plain update on the same buffer
    assert rec["apply"] == 1 and rec["coef"] == 1.0 and rec["skipped"] == 0 and _same_bits(a.bits(), b.bits())
    assert not bool(torch.isfinite(b.p[1002])) and bool(torch.isfinite(b.p[:1002]).all())
    c = State(dev, p0, g, nk, nb)
    rec = c.guarded(0.0, 1.0, False)                                   # tf.clip_by_global_norm: a non-finite norm poisons everything
    assert rec["apply"] == 1 and np.isnan(rec["coef"]) and bool(torch.isnan(c.p).all()) and int(c.step) == 2


@pytest.mark.gpu
def test_a_large_finite_gradient_is_not_mistaken_for_inf(dev):
    """1e20 squared overflows fp32 but not the fp64 accumulation: the norm is finite and the step is applied (and clipped)."""
    n, nk, nb = 1003, 400, 200
    p0, g = _inputs(n, 8)
    g[5], g[1002] = 1e20, -3e19
    s = State(dev, p0, g, nk, nb, gs=1.0)
    want = s.ref_norm()
    rec = s.guarded(0.0, 1.0, True)
    assert rec["apply"] == 1 and rec["skipped"] == 0 and np.isfinite(rec["norm"]) and abs(rec["norm"] - want) <= NORM_REL * want
    assert abs(rec["coef"] - 1.0 / want) <= NORM_REL / want and bool(torch.isfinite(s.p).all()) and int(s.step) == 2


@pytest.mark.gpu
@pytest.mark.parametrize("n,nk,nb,cap", SIZES[4:])
def test_two_runs_give_identical_bits(dev, n, nk, nb, cap):
    """No atomics and a grid that depends on n and M1_EW_BLOCKS only: the partial sums, the record and the update repeat exactly."""
    p0, g = _inputs(n, 9)
    runs = []
    with ops.config(**({"M1_EW_BLOCKS": cap} if cap else {})):
        for _ in range(2):
            s = State(dev, p0, g, nk, nb)
            if not runs:
                cn = 0.5 * s.ref_norm(0.9)
            s.guarded(0.9, cn, True)
            runs.append(s.bits() + [s.ctl.clone()])
    assert _same_bits(runs[0], runs[1])


@pytest.mark.gpu
def test_norm_at_the_c3_parameter_count(dev):
    """67,254,246 elements (n % 4 == 2, both range edges inside a float4), regulariser on: the norm against
    (gr.double() ** 2).sum().sqrt() computed by torch on the device."""
    n, nk, nb = 67_254_246, 33_626_946 + 1, 1_206
    gen = torch.Generator(device=dev).manual_seed(11)
    p = torch.randn(n, generator=gen, device=dev)
    g = torch.randn(n, generator=gen, device=dev) * 0.01
    ws, ctl = torch.empty(ops.grad_norm_ws(n), dtype=torch.uint8, device=dev), ops.new_step_ctl(dev)
    lam = torch.zeros(n, dtype=torch.float64, device=dev); lam[:nk] = 0.3; lam[nk:nk + nb] = 0.7
    gr = lam.mul_(2.0).mul_(p.double()).add_(g.double(), alpha=0.5)
    want = float((gr ** 2).sum().sqrt())
    del gr, lam
    ops.grad_norm_(g, p, nk, nb, 0.3, 0.7, 0.5, 0.0, 0.5 * want, True, ws, ctl)
    rec = ops.read_step_ctl(ctl)
    print(f"C3 norm {rec['norm']:.9g} fp64 {want:.12g} rel {abs(rec['norm'] - want) / want:.2e}")
    assert abs(rec["norm"] - want) <= NORM_REL * want and rec["apply"] == 1
    assert abs(rec["coef"] - 0.5) <= NORM_REL * 0.5
    del p, g
    torch.cuda.empty_cache()


# =================================================================================================================================
# GPU, model level: the small probabilistic model of test_trainer.py (filters 8 ... 128, (4, 32, 32), batch 2)
# =================================================================================================================================
DIMS = (4, 32, 32)


def _model(dev, dtype, seed=0, **opt_kw):
    rng = np.random.default_rng(seed)
    cases = [T.synthetic_case(rng, DIMS, 3, 2) for _ in range(2)]
    x, y = next(T.batches(T.custom_data_generator(cases, probabilistic=True, mode='train'), 2, dev))
    PKG.unets.network_blocks.set_init_seed(seed)
    m = PKG.unets.networks.M1(input_spatial_dims=DIMS, input_channels=4, num_classes=2, dropout_rate=0.0, filters=(8, 16, 32, 64, 128),
                              strides=C1_STRIDES, dense_skip=True, probabilistic=True, prob_latent_dims=(3, 2, 1, 0), summary=False).to(dev)
    m.set_compute_dtype(dtype)
    opt = PKG.optim.Adam(learning_rate=1e-3, amsgrad=True, **opt_kw)
    m.compile(optimizer=opt, loss=[PKG.losses.Focal(alpha=[0.75, 0.25], gamma=2.0).loss, PKG.losses.EvidenceLowerBound().loss],
              loss_weights=[1.0, 10.0])
    return m, opt, x, y


def _opt_bits(opt):
    return [t.clone().view(torch.int32) for t in (opt.flatp.flat, opt.m, opt.v, opt.vhat, opt.step_dev)]


def _fwd_bwd(m, opt, x, y):
    opt.set_lr_device()
    m.train()
    opt.zero_grad()
    total, _ = m.compute_loss(m(x), y)
    total.backward()
    opt.flatp.gather_grads()
    return total


@pytest.mark.gpu
def test_model_poisoned_gradient_buffer_is_skipped(dev):
    m, opt, x, y = _model(dev, torch.float32, skip_nonfinite=True)
    logs = m.train_step(x, y)                                                  # a clean step: moments are non-zero afterwards
    assert logs["skipped"] == 0 and np.isfinite(logs["grad_norm"]) and logs["grad_norm"] > 0 and int(opt.step_dev) == 2
    before = _opt_bits(opt)
    _fwd_bwd(m, opt, x, y)
    live = int(opt.flatp.grad.abs().argmax())
    opt.flatp.grad[live] = float("inf")
    opt.exchange()
    opt.apply_flat()
    assert opt.skipped_steps == 1 and opt.grad_norm == float("inf")
    assert _same_bits(before, _opt_bits(opt))


@pytest.mark.gpu
def test_model_bad_input_batch_end_to_end(dev):
    """One +Inf voxel in the input: with the guard the parameters stay finite and unchanged and the next clean step trains on; without
    it the same batch leaves NaN weights."""
    m, opt, x, y = _model(dev, torch.float32, skip_nonfinite=True)
    xb = {k: v.clone() for k, v in x.items()}
    xb["image"][0, 1, 7, 9, 0] = float("inf")
    before = _opt_bits(opt)
    logs = m.train_step(xb, y)
    assert logs["skipped"] == 1 and not np.isfinite(logs["grad_norm"])
    assert _same_bits(before, _opt_bits(opt)) and bool(torch.isfinite(opt.flatp.flat).all())
    assert opt.iterations == 1 and int(opt.step_dev) == 1                       # the schedule moves on, Adam's t does not
    logs = m.train_step(x, y)
    assert np.isfinite(logs["loss"]) and logs["skipped"] == 1 and np.isfinite(logs["grad_norm"]) and int(opt.step_dev) == 2
    assert not torch.equal(before[0], _opt_bits(opt)[0])

    m2, opt2, _, _ = _model(dev, torch.float32)                                 # the control run: today's optimiser
    logs2 = m2.train_step(xb, y)
    assert set(logs2) == {"loss", "detection_loss", "KL_loss"}
    assert bool(torch.isnan(opt2.flatp.flat).any())


@pytest.mark.gpu
def test_model_captured_guarded_step_replays_like_eager(dev):
    """bf16, captured as test_bench_parity.py::test_graph_replay_equals_eager_steps captures the step, with global_clipnorm at half the
    measured norm of the first of the three compared steps (taken from the restored start state, after the two warm-up steps: a fresh
    model's norm falls several-fold within its first steps, so the norm of the very first step would clip nothing here).  That step's
    coef is 0.5; three replays leave the bits of three eager steps, control record included; the graph holds no memset node."""
    m, opt, x, y = _model(dev, torch.bfloat16, skip_nonfinite=True)
    opt.set_lr_device()
    m.train()

    def step():
        opt.zero_grad()
        total, _ = m.compute_loss(m(x), y)
        total.backward()
        opt.flatp.gather_grads()
        opt.exchange()
        opt.apply_flat()
        ops.step_advance(None, m.rng_state)

    state = lambda: [opt.flatp.flat, opt.m, opt.v, opt.vhat, opt.step_dev, m.rng_state, opt.step_ctl]
    step(); norm_fresh = opt.grad_norm; step()
    torch.cuda.synchronize()
    start = [t.clone() for t in state()]
    gen0 = torch.cuda.get_rng_state(dev)

    def restore():
        with torch.no_grad():
            for t, s0 in zip(state(), start):
                t.copy_(s0)
        torch.cuda.set_rng_state(gen0, dev)
        ops.repack_all()
        torch.cuda.synchronize()

    step()                                        # the first compared step, unclipped: its norm places the clip
    norm1 = opt.grad_norm
    assert np.isfinite(norm1) and norm1 > 0
    opt.global_clipnorm = 0.5 * norm1
    restore()
    recs = []
    for _ in range(3):
        step(); recs.append(ops.read_step_ctl(opt.step_ctl))
    torch.cuda.synchronize()
    eager = [t.clone() for t in state()]
    print("captured-step test: norm of the fresh model's first step", norm_fresh, "of the first compared step", norm1, "records of the eager steps", recs)
    assert recs[0]["norm"] == norm1 and abs(recs[0]["coef"] - 0.5) <= 1e-6       # (0.5 * float(norm) / fp64 norm: within 2^-24 of 0.5)
    assert all(0 < r["coef"] <= 1 and r["apply"] == 1 for r in recs), recs
    assert not torch.equal(eager[0], start[0]) and int(opt.step_dev) == int(start[4]) + 3

    restore()
    s_ = torch.cuda.Stream()
    s_.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s_):
        step()
    torch.cuda.current_stream().wait_stream(s_)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(gr):
        step()
    torch.cuda.synchronize()
    hist = PKG.hip.graphs.assert_no_memset_nodes(gr)
    assert hist.get("memset", 0) == 0 and hist.get("kernel", 0) > 0, hist
    restore()
    for _ in range(3):
        gr.replay()
    torch.cuda.synchronize()
    for name, a, b in zip(["parameters", "adam m", "adam v", "adam vhat", "step counter", "rng state", "control record"], eager, state()):
        assert torch.equal(a, b), f"{name}: {int((a != b).sum())} of {a.numel()} elements differ between 3 eager steps and 3 replays"
    del gr


class _StubReducer:
    """What optim.Adam reads of a ddp.GradReducer: 1 / world_size = 0.5 and an exchange that does nothing."""
    grad_scale = 0.5
    active = False

    def begin_step(self):
        pass

    def finish(self):
        pass


@pytest.mark.gpu
def test_model_norm_is_taken_after_the_exchange_with_grad_scale_inside(dev):
    m, opt, x, y = _model(dev, torch.float32, skip_nonfinite=True)
    opt.reducer, opt.grad_scale = _StubReducer(), _StubReducer.grad_scale
    _fwd_bwd(m, opt, x, y)
    opt.exchange()
    f = opt.flatp
    args = (f.flat.double(), f.grad.double(), f.n_kernel, f.n_bias, opt.l2_kernel, opt.l2_bias)
    halved = float((clip_ref.regularised_grad(*args, 0.5) ** 2).sum().sqrt())
    full = float((clip_ref.regularised_grad(*args, 1.0) ** 2).sum().sqrt())
    assert full > 1.5 * halved                                                   # the two are told apart by far more than the bound
    opt.apply_flat()
    assert abs(opt.grad_norm - halved) <= NORM_REL * halved and opt.skipped_steps == 0
