"""The in-kernel random streams, draw for draw, against a host restatement of Philox4x32-10 (tests/philox_ref.py).

Every stochastic part of the training step -- dropout (stand-alone and fused into se_combine / se_combine_dup), the latent draws,
the augmentation table and the augmentation noise -- is a pure function of (seed, step, layer or stream id, element index).  The
parity tests elsewhere inject the draw or reuse the kernel's own mask; here the draws themselves are pinned:

  * CPU: the restatement against the three published Random123 vectors; the id layout of real models cannot put two consumers on
    one (key, counter) pair; masks and latent draws of different steps / layers / ranks are uncorrelated; the keep frequency.
  * GPU: every kernel's draws against the restatement -- masks element for element, normals within a tolerance that comes from
    the restatement's own float32 / float64 difference.

Measured on the MI355X (printed by the tests; the bound is 4 x max|float32 restatement - float64 restatement| over the test's own
draws, the factor covering the few ulp by which the device's logf / cosf / sinf may differ from the host's):

    latent draws   (5.3e5 draws per case)   bound 3.76e-06 .. 4.25e-06    device max error 9.0e-07 .. 1.15e-06  (d(logsigma) <= 1.0e-06)
    noise          (7.8e3 voxels x 4)       bound 2.80e-06 .. 2.93e-06 (one rounding of the sum included)    device max error 7.4e-07
    table          cos / sin within 0.73 ulp, the two offsets within 0.75 ulp(w1) of float64 (bound: 4)
"""
import math

import numpy as np
import pytest
import torch

import philox_ref as R
from util import PKG, ops

A = PKG.augmentations
gpu = pytest.mark.gpu
SEED = 0x5EED1234
README_CASCADE_LAST_ID = 48          # dropout layers of a cascaded probabilistic model: 2 stages x (prior + posterior) x 12
LATENT_ID0 = 0x4C415400


def _rng(seed, step, dev):
    # (the device pair is int64: a step of 2^28 - 1 and a 31-bit seed fit)
    return torch.tensor([seed, step], dtype=torch.int64, device=dev)


def _keep_scale(rate):
    """float32(1 / (1 - rate)) of the float32 rate that crosses the C ABI (one rounding of the quotient; at the rates used here the
    kernel's float32 division gives the same value, asserted by test_keep_scale_formulas_agree)."""
    return np.float32(1.0 / (1.0 - float(np.float32(rate))))


# =====================================================================================================================================
# CPU: the restatement itself
# =====================================================================================================================================
KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_restatement_matches_the_random123_known_answers(ctr, key, want):
    got = R.philox4x32_10(*ctr, *key)
    assert " ".join("%08x" % int(v[0]) for v in got) == want


def test_restatement_is_vectorised_over_counters():
    one = R.philox4x32_10(0, 0, 0, 0, 0, 0)
    many = R.philox4x32_10(np.array([0, 7, 0], dtype=np.uint64), 0, 0, 0, 0, 0)
    assert all(m.shape == (3,) and int(m[0]) == int(o[0]) == int(m[2]) for m, o in zip(many, one))
    assert all(int(m[1]) != int(m[0]) for m in many)


def test_keep_mask_takes_word_e_and_3_of_block_e_shift_2():
    """keep_uniform against ``words`` evaluated one element at a time, across a block boundary, at a step and an offset."""
    seed, step, lid, first, n = SEED, 4, 2, 1261, 11
    u = R.keep_uniform(seed, step, lid, n, first)
    for i in range(n):
        e = (step << 36) + first + i
        w = int(R.words(seed, lid, e >> 2)[0, e & 3])
        assert u[i] == np.float32(w >> 8) * np.float32(2.0 ** -24)
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()


def _edge_element(seed, step, lid):
    """(index, u) of the first element of the stream whose uniform lies well inside (0, 1): the rate of the >= edge tests."""
    u = R.keep_uniform(seed, step, lid, 64)
    j = int(np.nonzero((u > 0.2) & (u < 0.8))[0][0])
    return j, u[j]


def test_edge_rate_is_the_uniform_of_the_chosen_element():
    seed, step, lid = SEED, 1, 2
    j, u = _edge_element(seed, step, lid)
    e = (step << 36) + j
    w = int(R.words(seed, lid, e >> 2)[0, e & 3])
    assert u == np.float32(w >> 8) * np.float32(2.0 ** -24)
    rate = float(u)
    assert np.float32(rate) == u and 0.2 < rate < 0.8              # exactly representable: the float the C ABI carries is u itself
    assert bool(R.keep_mask(seed, step, lid, 64, rate)[j])          # u >= u keeps
    assert not (R.keep_uniform(seed, step, lid, 64)[j] > np.float32(rate))          # ... and `>` would drop it


def test_keep_scale_formulas_agree():
    for rate in (0.1, 0.25, 0.5, 0.9):
        r = np.float32(rate)
        assert np.float32(1.0) / (np.float32(1.0) - r) == _keep_scale(rate)          # the kernel's float32 division


@pytest.mark.parametrize("rate", [0.1, 0.25, 0.5, 0.9])
def test_keep_frequency_within_four_binomial_sigmas(rate):
    n = 1 << 18
    keep = R.keep_mask(SEED, 3, 5, n, rate)
    p = 1.0 - float(np.float32(rate))
    sig = abs(keep.mean() - p) / math.sqrt(p * (1 - p) / n)
    print(f"rate {rate}: keep frequency {keep.mean():.6f}, {sig:.2f} sigma")
    assert sig < 4.0


# ---- independence ---------------------------------------------------------------------------------------------------------------
def _corr(a, b):
    n = min(a.size, b.size)
    a, b = a[:n].astype(np.float64), b[:n].astype(np.float64)
    a, b = a - a.mean(), b - b.mean()
    return abs(float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))) * math.sqrt(n)


def test_streams_of_different_steps_layers_levels_and_ranks_are_uncorrelated():
    masks = {(s, l): R.keep_mask(SEED, s, l, 65536, 0.5) for s in (0, 1, 4) for l in (1, 2, 3, 40)}
    lats = {(s, v): R.normal(SEED, s, LATENT_ID0 + v, 48000) for s in (0, 1) for v in range(4)}
    mk, lk = list(masks), list(lats)
    mm = [_corr(masks[a], masks[b]) for i, a in enumerate(mk) for b in mk[i + 1:]]
    ll = [_corr(lats[a], lats[b]) for i, a in enumerate(lk) for b in lk[i + 1:]]
    ml = [_corr(masks[a], lats[b]) for a in mk for b in lk]
    assert (len(mm), len(ll), len(ml)) == (66, 28, 96)
    m0 = masks[(0, 1)]
    auto = [_corr(m0[:-lag], m0[lag:]) for lag in (1, 2, 3, 4, 8, 16, 64)]
    ranks = [R.keep_mask(SEED + 2 + r, 0, 1, 65536, 0.5) for r in range(8)]
    rr = [_corr(a, b) for i, a in enumerate(ranks) for b in ranks[i + 1:]]
    print(f"max |corr| * sqrt(n): masks {max(mm):.2f} latents {max(ll):.2f} mask-latent {max(ml):.2f} "
          f"autocorrelation {max(auto):.2f} ranks {max(rr):.2f}")
    assert max(mm + ll + ml + auto + rr) < 4.5


# ---- the id layout -------------------------------------------------------------------------------------------------------------
BENCH_VOX = 20 * 160 * 160
STEPS = [0, 1, 2, 3, 4, 5, 8, (1 << 28) - 2, (1 << 28) - 1]


def _readme_model(**kw):
    # (the ids do not depend on the weights: a zero initializer spares the QR of the orthogonal one)
    return PKG.unets.networks.M1(input_spatial_dims=(20, 160, 160), input_channels=3, num_classes=2, summary=False,
                                 kernel_initializer=PKG.initializers.Zeros(), **kw)


def _model_consumers(tag, m, seeds):
    NB, NW = PKG.unets.network_blocks, PKG.unets.networks
    out = []
    for name, mod in m.named_modules():
        for r, seed in enumerate(seeds):
            if isinstance(mod, NB._DropoutBase):
                # the largest tensor a dropout layer of the bench step sees: 2 volumes x 2 stacked passes x 32 channels (bounded here by 512)
                out.append((f"{tag}.{name}@{r}", "dropout", seed, mod.layer_id, 4 * BENCH_VOX * 512))
            elif isinstance(mod, NW.M1Core):
                out += [(f"{tag}.{name}.z{lvl}@{r}", "latent", seed, mod.latent_stream_id + lvl, 4 * BENCH_VOX * 3) for lvl in range(4)]
    return out


def test_no_two_consumers_of_real_models_share_a_key_and_a_counter():
    """The README deterministic, probabilistic and cascaded models (and a second probabilistic one: two models of one process),
    under the trainer's seeds of ranks 0..7 (``SEED + 2 + rank``) and the model's built-in default; the augmentation streams of
    ranks 0..7 under the trainer's seed of folds 0..4 (``SEED + 7919 + 1000 * fold``) and under the module's default pair."""
    prob = dict(probabilistic=True, dense_skip=True, deep_supervision=True)
    casc = _readme_model(cascaded='noisy-or', **prob)
    NB = PKG.unets.network_blocks
    assert sum(isinstance(x, NB._DropoutBase) for x in casc.modules()) == README_CASCADE_LAST_ID
    models = {"det": _readme_model(), "prob": _readme_model(**prob), "casc": casc, "prob2": _readme_model(**prob)}
    for base_seed in (0, 1234):
        seeds = [base_seed + 2 + r for r in range(8)] + [0x1234ABCD]
        cons = [c for tag, m in models.items() for c in _model_consumers(tag, m, seeds)]
        ids = [c[3] for c in cons if c[2] == seeds[0]]
        assert len(set(ids)) == len(ids)                              # the allocation itself: no id handed out twice
        for aseed in [base_seed + 7919 + 1000 * f for f in range(5)] + [0]:
            for r in range(8):
                cons.append((f"aug.table@{aseed}/{r}", "table", aseed, A.STREAM_DRAW + 2 * r, 2))
                cons.append((f"aug.noise@{aseed}/{r}", "noise", aseed, A.STREAM_NOISE + 2 * r, 2 * BENCH_VOX))
        keys = [R.key(c[2], c[3]) for c in cons]
        assert len(set(keys)) == len(keys), "two consumers share a Philox key"
        assert R.collisions(cons, STEPS) == []


def test_the_audit_sees_the_hazards_the_layout_avoids():
    # one key for a dropout layer and a latent head: dropout divides the counter by four, so step 4t meets the latent's step t
    bad = R.collisions([("d", "dropout", 9, 7, 4096), ("z", "latent", 9, 7, 4096)], STEPS)
    assert ("d", 4, "z", 1) in bad and ("d", 0, "z", 0) in bad
    # the two limits: step < 2^28 (step << 36 wraps) and fewer than 2^36 elements per consumer
    assert R.counter_range("latent", 1 << 28, 1)[0] == R.counter_range("latent", 0, 1)[0]
    assert R.collisions([("z", "latent", 9, 7, (1 << 36) + 1)], [0, 1]) == [("z", 0, "z", 1)]
    assert R.collisions([("d", "dropout", 9, 7, (1 << 36) + 1)], [0, 1]) == [("d", 0, "d", 1)]
    assert R.collisions([("z", "latent", 9, 7, 1 << 36), ("d", "dropout", 9, 8, 1 << 36), ("t", "table", 9, 9, 1 << 30)], STEPS) == []


# =====================================================================================================================================
# GPU: the kernels against the restatement
# =====================================================================================================================================
BIG = (1 << 20) + 4099            # above the 4096 x 256 threads of the launch (the grid-stride loop runs twice), not a multiple of 4


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rate", [0.1, 0.25, 0.5, 0.9])
def test_dropout_mask_equals_the_restatement_element_for_element(dev, dtype, rate):
    sc = torch.tensor(float(_keep_scale(rate))).to(dtype)            # float32(1 / (1 - rate)), rounded to the storage type
    for n in (BIG, 5):
        x = torch.ones(n, dtype=dtype, device=dev)
        for step in (0, 1, 4, (1 << 28) - 1):
            for lid in (1, 2, README_CASCADE_LAST_ID):
                y = ops.dropout(x, rate, _rng(SEED, step, dev), lid).cpu()
                keep = torch.from_numpy(R.keep_mask(SEED, step, lid, n, rate))
                assert torch.equal(y != 0, keep), (n, step, lid, int(((y != 0) != keep).sum()))
                assert torch.equal(y[keep], sc.expand(int(keep.sum())))
    # the backward of a non-constant dy uses the same mask
    n, step, lid = BIG, 4, 2
    x = torch.ones(n, dtype=dtype, device=dev, requires_grad=True)
    dy = (((torch.arange(n) % 251) + 1).float() / 256).to(dtype)     # 8 significant bits: exact in bf16
    ops.dropout(x, rate, _rng(SEED, step, dev), lid).backward(dy.to(dev))
    keep = torch.from_numpy(R.keep_mask(SEED, step, lid, n, rate))
    want = torch.where(keep, (dy.float() * float(_keep_scale(rate))).to(dtype), torch.zeros((), dtype=dtype))
    assert torch.equal(x.grad.cpu(), want)


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_dropout_keeps_the_element_whose_uniform_equals_the_rate(dev, dtype):
    seed, step, lid = SEED, 1, 2
    j, u = _edge_element(seed, step, lid)
    y = ops.dropout(torch.ones(64, dtype=dtype, device=dev), float(u), _rng(seed, step, dev), lid).cpu()
    assert bool(y[j] != 0)                                          # u >= rate with u == rate
    assert torch.equal(y != 0, torch.from_numpy(R.keep_mask(seed, step, lid, 64, float(u))))


# ---- dropout fused into se_combine ----------------------------------------------------------------------------------------------
def _se_inputs(N, sp, F_, dtype, dev, ident=False):
    """Inputs under which the undropped output is far from zero everywhere: IN3 / IN4 outputs sit in 3 +- 0.5 * 1.8 (uniform inputs:
    |xhat| < 1.8), the identity residual in [0.5, 1.5), the gate is sigmoid(b7) (W7 = 0: the gate takes no gradient from W6's side)."""
    g = np.random.default_rng(77)
    shp = (N, *sp, F_)
    y3 = torch.from_numpy(g.random(shp)).to(dtype)
    y4 = torch.from_numpy(g.random(shp) + 0.5).to(dtype)
    ch = torch.arange(F_, dtype=torch.float32)
    g3, b3 = 0.5 + 0.01 * ch, 3.0 - 0.02 * ch
    g4, b4 = (None, None) if ident else (0.5 + 0.02 * ch, 3.0 + 0.01 * ch)
    W6, b6 = torch.from_numpy(g.standard_normal((1, 1, 1, F_, 2))).float() * 0.5, torch.tensor([0.1, -0.1])
    W7, b7 = torch.zeros(1, 1, 1, 2, F_), 0.05 * ch
    dout = torch.from_numpy(0.5 + g.integers(0, 128, (2 * N, *sp, F_)) / 128.0).to(dtype)       # [0.5, 1.5), exact in bf16
    mv = lambda t: None if t is None else t.to(dev)
    return [mv(t) for t in (y3, y4, g3, b3, g4, b4, W6, b6, W7, b7)], dout.to(dev)


def _leaves(ins, dtype=None):
    out = []
    for i, t in enumerate(ins):
        if t is None:
            out.append(None)
        else:
            t = t.detach().clone()
            out.append((t.to(dtype) if (dtype is not None and i < 2) else t).requires_grad_(True))
    return out


def _se_backward_tolerance(dtype, ref):
    """The reference is the same fp32 arithmetic on the same inputs; what differs is the storage rounding of the gradients (bf16: 8
    significant bits, half an ulp = 2^-9 of the value, and the reduced sums see bf16-rounded d(out) products) and the order of the
    fp32 sums.  A keep decision that differs at one element moves d(y3) there by d(out) * scale * g * rho * gamma3 * rstd3 > 0.5,
    a hundred times these tolerances."""
    return (2.0 ** -7 if dtype == torch.bfloat16 else 1e-5) * float(ref.abs().max())


SE_CASES = [("bf16-F16-stored-bits", torch.bfloat16, 16, False, 0.5),       # VEC = 8, ALIGNED; the backward reads the stored keep bits
            ("bf16-F12-regenerates", torch.bfloat16, 12, False, 0.25),      # 12 % 8: VEC = 1, the element path, fwd and bwd
            ("fp32-F12-regenerates", torch.float32, 12, False, 0.25),       # VEC = 4, ALIGNED (V * F % 4 == 0), fwd and bwd regenerate
            ("fp32-F5-element-path", torch.float32, 5, False, 0.5),         # VEC = 1, odd sample offset V * F: every word index is reached
            ("fp32-F8-identity", torch.float32, 8, True, 0.25),
            ("bf16-F8-identity", torch.bfloat16, 8, True, 0.5),
            ("fp32-F12-edge-rate", torch.float32, 12, False, None)]         # rate = the uniform of one element: the vector path's own >=


@gpu
@pytest.mark.parametrize("name,dtype,F_,ident,rate", SE_CASES, ids=[c[0] for c in SE_CASES])
def test_se_combine_fused_dropout_draws_the_restatement_mask(dev, name, dtype, F_, ident, rate):
    N, sp, step, lid = 2, (3, 15, 17), 4, 21                         # 765 voxels per sample (odd), several blocks per sample
    ins, dout = _se_inputs(N, sp, F_, dtype, dev, ident)
    dout = dout[:N]
    n = N * 765 * F_
    edge = None
    if rate is None:
        u = R.keep_uniform(SEED, step, lid, n)
        edge = int(np.nonzero((u > 0.2) & (u < 0.8))[0][5])
        rate = float(u[edge])
    rng = _rng(SEED, step, dev)
    keep = torch.from_numpy(R.keep_mask(SEED, step, lid, n, rate)).reshape(N, *sp, F_)
    assert edge is None or bool(keep.reshape(-1)[edge])
    a = _leaves(ins, dtype)
    out = ops.se_combine(*a, rate, rng, lid)
    out.backward(dout)
    out0 = ops.se_combine(*_leaves(ins, dtype)).detach()
    assert bool((out0 != 0).all())                                  # nothing hides a dropped element
    assert torch.equal(out.detach().cpu() != 0, keep)
    sc = float(_keep_scale(rate))
    if dtype == torch.float32 and edge is None:                    # (at these rates the kernel's float32 quotient is _keep_scale)
        assert torch.equal(out.detach().cpu(), torch.where(keep, out0.cpu() * sc, torch.zeros(())))
    # the backward: the unfused composition in fp32 -- se_combine without dropout, times the RESTATEMENT's mask
    r = _leaves(ins, torch.float32)
    o = ops.se_combine(*r) * (keep.to(dev).float() * sc)
    o.backward(dout.float())
    for i in (0, 1):
        got, ref = a[i].grad.float(), r[i].grad
        tol = _se_backward_tolerance(dtype, ref)
        err = float((got - ref).abs().max())
        print(f"{name}: d(y{3 + i}) max error {err:.3e} (tolerance {tol:.3e}, max |ref| {float(ref.abs().max()):.3e})")
        assert err <= tol
    if ident:                                                       # no norm4: d(y4) is d(rho) itself, zero exactly where the mask drops
        assert torch.equal(a[1].grad.cpu() != 0, keep)


SE_DUP_CASES = [("fp32-F4", torch.float32, 1, 4, 0.25),       # second half at offset 765 * 4: a multiple of 4, not of 8
                ("fp32-F12-N2", torch.float32, 2, 12, 0.5),
                ("bf16-F8-N2", torch.bfloat16, 2, 8, 0.5)]     # the stored keep bits: byte (offset >> 3) of the second half


@gpu
@pytest.mark.parametrize("name,dtype,N,F_,rate", SE_DUP_CASES, ids=[c[0] for c in SE_DUP_CASES])
def test_se_combine_dup_second_half_has_its_own_draws(dev, name, dtype, N, F_, rate):
    """Output half 1 reads stream positions [0, N V F), half 2 [N V F, 2 N V F).  se.hip instantiates philox_keep_vec with
    ALIGNED = (VEC % 4 == 0), and the duplicating form only exists for whole 16-byte channel vectors (VEC = 4 / 8, F % VEC == 0):
    N V F is then always a multiple of 4 and BOTH halves take the aligned vector path -- an odd offset cannot occur (the last
    assertion: the odd F is refused); the element path of the fused draws is covered by the F = 5 and bf16 F = 12 cases above."""
    sp, step, lid = (3, 15, 17), 1, README_CASCADE_LAST_ID
    ins, dout = _se_inputs(N, sp, F_, dtype, dev)
    half = N * 765 * F_
    k1 = torch.from_numpy(R.keep_mask(SEED, step, lid, half, rate)).reshape(N, *sp, F_)
    k2 = torch.from_numpy(R.keep_mask(SEED, step, lid, half, rate, first=half)).reshape(N, *sp, F_)
    assert not torch.equal(k1, k2)
    keep = torch.cat([k1, k2])
    a = _leaves(ins, dtype)
    out = ops.se_combine(*a, rate, _rng(SEED, step, dev), lid, dup=True)
    out.backward(dout)
    out0 = ops.se_combine(*_leaves(ins, dtype)).detach()
    assert bool((out0 != 0).all())
    got = out.detach().cpu() != 0
    assert torch.equal(got[:N], k1) and torch.equal(got[N:], k2)
    sc = float(_keep_scale(rate))
    r = _leaves(ins, torch.float32)
    o0 = ops.se_combine(*r)
    o = torch.cat([o0, o0]) * (keep.to(dev).float() * sc)
    o.backward(dout.float())
    # ... and the reference would differ, by far more than the tolerance, had the second half drawn the first half's mask again
    w = _leaves(ins, torch.float32)
    o0w = ops.se_combine(*w)
    (torch.cat([o0w, o0w]) * (torch.cat([k1, k1]).to(dev).float() * sc)).backward(dout.float())
    for i in (0, 1):
        g, ref = a[i].grad.float(), r[i].grad
        tol = _se_backward_tolerance(dtype, ref)
        err = float((g - ref).abs().max())
        print(f"dup {name}: d(y{3 + i}) max error {err:.3e} (tolerance {tol:.3e}); same-mask reference is off by "
              f"{float((w[i].grad - ref).abs().max()):.3e}")
        assert err <= tol
        assert float((w[i].grad - ref).abs().max()) > 10 * tol
    with pytest.raises(RuntimeError):
        ops.se_combine(*_leaves(_se_inputs(1, (1, 3, 3), 5, dtype, dev)[0], dtype), rate, _rng(SEED, step, dev), lid, dup=True)


# ---- latent draws --------------------------------------------------------------------------------------------------------------
LAT_N = (1 << 19) + 777          # N * V * L: above the 2048 x 256 threads of the launch
# 2^19 + 777 = 5 * 19 * 5527 has no factor 3 (and no factor 2): the L = 3 and the stacked (even N) cases hold one element more
LAT_SHAPES = {(1, False): (1, 5, 19, 5527), (3, False): (1, 2, 1, 87511), (1, True): (2, 1, 1, 262533), (3, True): (2, 1, 1, 87511)}


def _latent_reference(step, sid, n):
    z64 = R.normal(SEED, step, sid, n)
    bound = 4.0 * float(np.abs(R.normal(SEED, step, sid, n, np.float32).astype(np.float64) - z64).max())
    return z64, bound


@gpu
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("step", [0, 5])
@pytest.mark.parametrize("sid", [LATENT_ID0, LATENT_ID0 + 8 + 2], ids=["core0-level0", "core1-level2"])
def test_latent_draws_equal_the_restatement(dev, L, step, sid):
    """ml = 0: mu = 0, sigma = 1, z is the draw.  Bound and measured error: see the module docstring."""
    shp = LAT_SHAPES[(L, False)]
    n = int(np.prod(shp)) * L
    assert n in (LAT_N, LAT_N + 1) and n > 2048 * 256
    z64, bound = _latent_reference(step, sid, n)
    rng = _rng(SEED, step, dev)
    ml = torch.zeros((*shp, 2 * L), device=dev, requires_grad=True)
    z = ops.latent_sample(ml, None, False, rng=rng, stream_id=sid)
    err = float(np.abs(z.detach().cpu().double().numpy().reshape(-1) - z64).max())
    print(f"latent L={L} step={step} id={sid:#x}: bound {bound:.3e}, device max error {err:.3e}")
    assert 0 < bound < 1e-4 and err <= bound
    # the backward regenerates the draw: d(mu) = dz, d(logsigma) = dz * eps  (|dz| <= 1: the same bound)
    dz = (((torch.arange(n) % 255) - 127).float() / 128).reshape(*shp, L)
    z.backward(dz.to(dev))
    g = ml.grad.cpu()
    assert torch.equal(g[..., :L], dz)
    gerr = float(np.abs(g[..., L:].double().numpy().reshape(-1) - dz.double().numpy().reshape(-1) * z64).max())
    print(f"   d(logsigma) max error {gerr:.3e}")
    assert gerr <= bound + 0.5 * float(np.spacing(np.float32(np.abs(z64).max())))          # (the product is rounded once to fp32)
    # bf16 storage: the fp32 result rounded once
    zb = ops.latent_sample(torch.zeros((*shp, 2 * L), device=dev, dtype=torch.bfloat16), None, False, rng=rng, stream_id=sid)
    assert zb.dtype == torch.bfloat16 and torch.equal(zb, z.detach().to(torch.bfloat16))


@gpu
@pytest.mark.parametrize("L", [1, 3])
def test_stacked_latent_draws_cover_the_first_half_only(dev, L):
    shp, step, sid = LAT_SHAPES[(L, True)], 5, LATENT_ID0 + 1
    n = int(np.prod(shp)) * L
    z64, bound = _latent_reference(step, sid, n // 2)
    ml = torch.zeros((*shp, 2 * L), device=dev, requires_grad=True)
    z = ops.latent_sample(ml, None, False, stacked=True, rng=_rng(SEED, step, dev), stream_id=sid)
    zc = z.detach().cpu().double().numpy().reshape(-1)
    err = float(np.abs(zc[:n // 2] - z64).max())
    print(f"stacked latent L={L}: bound {bound:.3e}, device max error {err:.3e}")
    assert err <= bound and not zc[n // 2:].any()                   # the mean pass: z = mu = 0, no draw
    z.backward(torch.ones_like(z))
    gl = ml.grad[..., L:].cpu().double().numpy().reshape(-1)
    assert float(np.abs(gl[:n // 2] - z64).max()) <= bound and not gl[n // 2:].any()


# ---- augmentation noise and table -----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("nimg", [1, 3])
def test_augmentation_noise_equals_the_four_normals_of_the_restatement(dev, nimg):
    """Only the noise stage fired, noise_std = 1: out - in is the draw.  The sum in + z is rounded once to fp32, which adds half an
    ulp of the largest |out| to the bound of the draws."""
    N, D, H, C, step, sid = 2, 3, 36, nimg + 1, 3, A.STREAM_NOISE + 2 * 5
    g = np.random.default_rng(5)
    x = torch.from_numpy(g.standard_normal((N, D, H, H, C))).float()
    table = A.draw_params(None, N, H, H, explicit=[{"fired": R.MASTER | R.NOISE, "noise_std": 1.0}] * N, device=dev)
    out, _ = ops.aug_apply(x.to(dev), None, table, R.MASTER | R.NOISE, nimg, _rng(SEED, step, dev), sid)
    out = out.cpu()
    nv = N * D * H * H
    z64 = R.noise4(SEED, step, sid, nv)
    z32 = R.noise4(SEED, step, sid, nv, np.float32).astype(np.float64)
    bound = 4.0 * float(np.abs(z32 - z64)[:, :nimg].max()) + 0.5 * float(np.spacing(np.float32(out.abs().max())))
    diff = (out.double() - x.double()).numpy().reshape(nv, C)
    err = float(np.abs(diff[:, :nimg] - z64[:, :nimg]).max())
    print(f"noise nimg={nimg}: bound {bound:.3e}, device max error {err:.3e}")
    assert err <= bound < 1e-4
    assert torch.equal(out[..., nimg:], x[..., nimg:])              # the label channel receives none


def _ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


DEFAULT_HYPER = [1.00, 0.25, 0.15, 10.0, True, 1.20, 0.10, 0.025, True, 0.50, 1.50]       # train_model.py --AUGM_PARAMS
BUSY_HYPER = [0.70, 0.50, 0.20, 25.0, True, 1.50, 0.30, 0.10, True, 0.70, 1.80]          # every stage on, every coin near even


@gpu
@pytest.mark.parametrize("hyper", [DEFAULT_HYPER, BUSY_HYPER], ids=["default", "busy"])
def test_augmentation_table_equals_the_restatement(dev, hyper):
    """N = 70: two 64-thread blocks.  Integer and flag fields, gamma, noise_std and angle_deg are exact.  cos / sin (rot[0, 1, 3, 4])
    are within 4 ulp of the float64 value; the two offsets rot[2], rot[5] = (w1 - (c w1 - s h1)) / 2 are EXACTLY the float32
    expression of the kernel's own c and s, and within 4 ulp -- at the magnitude of w1, the largest term: an error of k ulp in c
    is k ulp(w1) in c * w1, whatever is left after the cancellation -- of the float64 value."""
    N, H, nimg = 70, 32, 3
    f = np.float32
    for step in (0, 3):
        for sid in (A.STREAM_DRAW, A.STREAM_DRAW + 2 * 7):
            t = A.table_to_numpy(ops.aug_draw(N, _rng(SEED, step, dev), sid, hyper, H, H, nimg, True))
            ref, rot64, used = R.aug_table(SEED, step, sid, N, hyper, H, H, nimg, True)
            assert used.max() < R.AUG_STRIDE, used.max()
            for name in ("fired", "scale", "tr", "cs", "cs_channel", "gamma_ch", "poor_ch", "rot_pad", "_pad"):
                assert np.array_equal(t[name], ref[name]), (name, step, sid)
            for name in ("gamma", "noise_std", "angle_deg"):
                assert t[name].tobytes() == ref[name].tobytes(), (name, step, sid)
            rot = t["rot"].astype(np.float64)
            trig = [0, 1, 3, 4]
            e_trig = float((np.abs(rot[:, trig] - rot64[:, trig]) / _ulp32(rot64[:, trig])).max())
            w1 = float(H + 2 * R.rotation_pad(H, H) - 1)
            e_off = float((np.abs(rot[:, [2, 5]] - rot64[:, [2, 5]]) / _ulp32(w1)).max())
            print(f"table step={step} id={sid:#x}: fired {int((t['fired'] & 1).sum())}/{N}, max words {used.max()}, "
                  f"cos/sin {e_trig:.2f} ulp, offsets {e_off:.2f} ulp(w1)")
            assert e_trig <= 4.0 and e_off <= 4.0
            c, s, w, h = t["rot"][:, 0], t["rot"][:, 3], f(w1), f(w1)
            on = (ref["fired"] & R.MASTER) != 0
            assert np.array_equal(t["rot"][:, 1], -s) and np.array_equal(t["rot"][:, 4], c)
            assert np.array_equal(t["rot"][on, 2], ((w - (c * w - s * h)) / f(2.0))[on])
            assert np.array_equal(t["rot"][on, 5], ((h - (s * w + c * h)) / f(2.0))[on])
            assert (ref["fired"] & R.MASTER).sum() > N // 2 and len(np.unique(ref["fired"])) > 8

