"""Monte-Carlo inference: the n-draw mean / entropy kernels (csrc/mc.hip: m1_mc_accum, m1_mc_finish), their ops and
``get_detect_model().predict_mc`` (the reference's --UNET_PROBA_ITER, train_model.py:72, with scipy.stats.entropy).

Kernel level: against the fp64 numpy restatement below (``r_accum`` / ``r_finish``), per element, with the bound

    |got - ref64| <= max(k * 2^-24 * scale, 4 * e32)

where e32 is the largest error of the SAME restatement run with fp32 values (computed per case, never taken from the kernel) and k
counts the fp32 roundings behind one output, each at most 2^-24 relative to a quantity that ``scale`` bounds (a library function,
expf / logf, is documented to 1 ulp = two half-ulp roundings):

  one probability p = e_c * (1 / s) <= 1:    x - max (1: |p ln p| <= 1/e), expf (2), the same two through s (3), the nc - 1 additions
                                             of s, the division, the product                                  K_P  = nc + 7
  sum_p of n = R * passes draws, scale n:    every p above, plus n - 1 additions of partial sums <= n          k    = K_P + n - 1
  mean = sum_p / n, scale 1:                 plus the division                                                 k    = K_P + n
  entropy, scale 1 + ln(nc):                 d(m ln m) = (ln m + 1) dm and sum_c |m_c (ln m_c + 1)| <= 1 + H; logf (2), the
                                             product, nc - 1 subtractions of partial sums <= H <= ln(nc)       k    = K_P + n + nc + 2

``test_fp32_restatement_stays_inside_the_bound`` checks on the CPU that the fp32 restatement alone meets the first term in every
case.  Worst errors measured on the MI355X are recorded in DESIGN.md section 7.

Model level: fp32 compute, filters (8,16,32,64,128) on a (4,32,32) volume, batch 2."""
import ctypes
import itertools
import math

import numpy as np
import pytest
import torch

from oracle import m1_oracle as O
from guarded import guarded
from util import C1_FILTERS, C1_STRIDES, PKG, build_m1, load_params_into, ops, rnd

L = PKG.hip.lib
U = 2.0 ** -24
DIMS = (4, 32, 32)
BS, RS, NCS, VS = (1, 2), (1, 3), (2, 3), (1, 7, 64 * 5 + 3, 4 * 32 * 32)
DTYPES = (torch.float32, torch.bfloat16)
PASSES = 3


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement (numpy; ``vt`` = np.float64 for the reference, np.float32 for e32) and the bound
# ---------------------------------------------------------------------------------------------------------------------------------
def r_softmax(x, vt):
    """Max-subtracted softmax over the last axis in m1_softmax_heads_fwd's operation order: exp(x - max), sum in class order,
    1 / sum, product."""
    x = x.astype(vt)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    s = e[..., 0]
    for c in range(1, x.shape[-1]):
        s = s + e[..., c]
    return e * (vt(1) / s)[..., None]


def r_accum(passes, R, vt):
    """passes: list of (R*B, V, nc) logits, replica-major -> (sum_p (B, V, nc) after each pass, per-draw probabilities per pass)."""
    sums, draws, total = [], [], None
    for lg in passes:
        p = r_softmax(lg.reshape(R, lg.shape[0] // R, *lg.shape[1:]), vt)
        acc = p[0]
        for r in range(1, R):
            acc = acc + p[r]
        total = acc if total is None else total + acc
        sums.append(total)
        draws.append(p)
    return sums, draws


def r_finish(sum_p, n, vt):
    """mean = sum_p / n; entropy = -sum_c mean_c ln(mean_c) in nats, 0 ln 0 = 0 (scipy.stats.entropy's default)."""
    mean = sum_p.astype(vt) / vt(n)
    pos = mean > 0
    t = np.where(pos, mean * np.log(np.where(pos, mean, vt(1))), vt(0))
    h = np.zeros(mean.shape[:-1], vt)
    for c in range(mean.shape[-1]):
        h = h - t[..., c]
    return mean, h


def k_p(nc):
    return nc + 7


def bound_sum(nc, n, e32):
    return max((k_p(nc) + n - 1) * U * n, 4 * e32)


def bound_mean(nc, n, e32):
    return max((k_p(nc) + n) * U, 4 * e32)


def bound_entropy(nc, n, e32):
    return max((k_p(nc) + n + nc + 2) * U * (1 + math.log(nc)), 4 * e32)


def make_logits(B, R, V, nc, dtype, seed):
    """PASSES tensors (R*B, V, nc): seeded normal clipped to |x| <= 6; from V = 7 on voxel 0 holds a +-80 spread (softmax exactly 0 / 1
    in fp32, class 0 winning in every draw) and voxel 1 equal logits (entropy ln nc).  Values are exact in ``dtype``."""
    g = np.random.default_rng(seed)
    out = []
    for _ in range(PASSES):
        x = np.clip(g.standard_normal((R * B, V, nc)) * 2.5, -6, 6).astype(np.float32)
        if V >= 7:
            x[:, 0, :] = -80.0
            x[:, 0, 0] = 80.0
            x[:, 1, :] = 0.75
        t = torch.from_numpy(x).to(dtype)
        out.append(t)
    return out


def as_np(t):
    return t.detach().float().cpu().numpy()


def case_refs(passes_t, R):
    """fp64 reference and the fp32 restatement's own error (e32) of the running sums, and of mean / entropy after the last pass."""
    lg = [as_np(t) for t in passes_t]
    s64, d64 = r_accum(lg, R, np.float64)
    s32, _ = r_accum(lg, R, np.float32)
    n = R * len(lg)
    m64, h64 = r_finish(s64[-1], n, np.float64)
    m32, h32 = r_finish(s32[-1], n, np.float32)
    e32 = {"sum": [float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(s32, s64)],
           "mean": float(np.abs(m32.astype(np.float64) - m64).max()), "entropy": float(np.abs(h32.astype(np.float64) - h64).max())}
    return s64, d64, m64, h64, e32


ALL_CASES = list(itertools.product(DTYPES, NCS, VS, BS, RS))


# ---------------------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound():
    lib = L.load()
    for name in ("m1_mc_accum", "m1_mc_finish"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert lib.m1_abi_version() == 1


def test_bad_arguments_are_rejected_without_a_gpu():
    lib = L.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    assert lib.m1_mc_accum(None, 1, 1, 1, 2, 0, p, 0, None, None) == -1               # NULL logits
    assert lib.m1_mc_accum(p, 1, 1, 1, 2, 0, None, 0, None, None) == -1               # NULL accumulator
    assert lib.m1_mc_accum(p, 0, 1, 1, 2, 0, p, 0, None, None) == -1                  # R = 0
    assert lib.m1_mc_accum(p, 1, 0, 1, 2, 0, p, 0, None, None) == -1 and lib.m1_mc_accum(p, 1, 1, 0, 2, 0, p, 0, None, None) == -1
    assert lib.m1_mc_accum(p, 1, 1, 1, 2, 7, p, 0, None, None) == -1                  # unknown dtype
    assert lib.m1_mc_accum(p, 1, 1, 1, 5, 0, p, 0, None, None) == -2                  # nc = 5
    assert lib.m1_mc_accum(p, 1, 1, 1, 1, 0, p, 0, None, None) == -2
    assert lib.m1_mc_accum(p + 2, 1, 1, 1, 2, 0, p, 0, None, None) == -1              # fp32 logits off their element alignment
    assert lib.m1_mc_accum(p + 1, 1, 1, 1, 2, 1, p, 0, None, None) == -1              # bf16 logits at an odd address
    assert lib.m1_mc_accum(p, 1, 1, 1, 2, 0, p + 2, 0, None, None) == -1 and lib.m1_mc_accum(p, 1, 1, 1, 2, 0, p, 0, p + 2, None) == -1
    assert lib.m1_mc_finish(None, 1, 1, 1, 2, p, p, None) == -1 and lib.m1_mc_finish(p, 1, 1, 1, 2, None, p, None) == -1
    assert lib.m1_mc_finish(p, 1, 1, 1, 2, p, None, None) == -1
    assert lib.m1_mc_finish(p, 0, 1, 1, 2, p, p, None) == -1                          # n_draws = 0
    assert lib.m1_mc_finish(p, 1, 1, 1, 5, p, p, None) == -2
    assert lib.m1_mc_finish(p + 2, 1, 1, 1, 2, p, p, None) == -1


def test_ops_refuse_to_run_under_autograd():
    t = torch.zeros(1, 1, 1, 1, 2)
    with pytest.raises(RuntimeError, match="no_grad"):
        ops.mc_accum(t, 1)
    with pytest.raises(RuntimeError, match="no_grad"):
        ops.mc_finish(t, 1)


def test_fp32_restatement_stays_inside_the_bound():
    """The first term of the bound, k * 2^-24 * scale, holds for the fp32-valued restatement in every case of the GPU tests: the
    count k is not short of what fp32 arithmetic in this operation order does."""
    worst = {"sum": 0.0, "mean": 0.0, "entropy": 0.0}
    with np.errstate(all="ignore"):
        for i, (dtype, nc, V, B, R) in enumerate(ALL_CASES):
            _, _, _, _, e32 = case_refs(make_logits(B, R, V, nc, dtype, 100 + i), R)
            for k, es in enumerate(e32["sum"]):
                n = R * (k + 1)
                assert es <= (k_p(nc) + n - 1) * U * n, (dtype, nc, V, B, R, n, es)
                worst["sum"] = max(worst["sum"], es / n)
            n = R * PASSES
            assert e32["mean"] <= (k_p(nc) + n) * U, (dtype, nc, V, B, R, e32)
            assert e32["entropy"] <= (k_p(nc) + n + nc + 2) * U * (1 + math.log(nc)), (dtype, nc, V, B, R, e32)
            worst["mean"], worst["entropy"] = max(worst["mean"], e32["mean"]), max(worst["entropy"], e32["entropy"])
    print("fp32 restatement, worst error over all cases (sum per draw, mean, entropy):", worst)


# ---------------------------------------------------------------------------------------------------------------------------------
# kernels on the GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def _five(t, dev):
    """(N, V, nc) host tensor -> contiguous (N, 1, 1, V, nc) on the device."""
    return t.reshape(t.shape[0], 1, 1, t.shape[1], t.shape[2]).contiguous().to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,nc,V", list(itertools.product(DTYPES, NCS, VS)), ids=lambda v: str(v).replace("torch.", ""))
def test_accumulate_and_finish_match_the_fp64_restatement(dev, dtype, nc, V):
    """accumulate = 0, 1, 1 over three passes: the running sum after every pass (one, two and three successive calls), the per-draw
    probabilities, and mean / entropy after the last one.  The first call writes into a NaN-filled buffer (no zero fill needed)."""
    worst = {"sum": 0.0, "mean": 0.0, "entropy": 0.0}
    with torch.no_grad(), np.errstate(all="ignore"):
        for B, R in itertools.product(BS, RS):
            i = ALL_CASES.index((dtype, nc, V, B, R))
            passes = make_logits(B, R, V, nc, dtype, 100 + i)
            s64, d64, m64, h64, e32 = case_refs(passes, R)
            sum_p = torch.full((B, 1, 1, V, nc), float("nan"), device=dev)
            for k, lg in enumerate(passes):
                x, draws = _five(lg, dev), None
                if k == 0:
                    rc = L.load().m1_mc_accum(x.data_ptr(), R, B, V, nc, ops._dt(x), sum_p.data_ptr(), 0, None,
                                              torch.cuda.current_stream().cuda_stream)
                    assert rc == 0
                    assert torch.equal(ops.mc_accum(x, R), sum_p)                     # the op's allocating form: the same write
                elif k == 1:
                    _, draws = ops.mc_accum(x, R, sum_p, samples=True)
                else:
                    ops.mc_accum(x, R, sum_p)
                n = R * (k + 1)
                got = as_np(sum_p).reshape(B, V, nc).astype(np.float64)
                assert np.isfinite(got).all(), "NaN left in the accumulator"
                err = float(np.abs(got - s64[k]).max())
                worst["sum"] = max(worst["sum"], err / n)
                assert err <= bound_sum(nc, n, e32["sum"][k]), (B, R, n, err, e32["sum"][k])
                if draws is not None:
                    assert tuple(draws.shape) == (R, B, 1, 1, V, nc)
                    derr = float(np.abs(as_np(draws).reshape(R, B, V, nc) - d64[k]).max())
                    assert derr <= k_p(nc) * U, (B, R, derr)
            n = R * PASSES
            mean, ent = ops.mc_finish(sum_p, n)
            assert mean.data_ptr() == sum_p.data_ptr() and tuple(ent.shape) == (B, 1, 1, V)
            em = float(np.abs(as_np(mean).reshape(B, V, nc) - m64).max())
            eh = float(np.abs(as_np(ent).reshape(B, V) - h64).max())
            worst["mean"], worst["entropy"] = max(worst["mean"], em), max(worst["entropy"], eh)
            assert em <= bound_mean(nc, n, e32["mean"]), (B, R, em, e32)
            assert eh <= bound_entropy(nc, n, e32["entropy"]), (B, R, eh, e32)
            if V >= 7:
                # the +-80 voxel: probabilities exactly 1 / 0 in every draw, so sum = n, mean = 1 / 0 and entropy 0.0 exactly
                mv, hv = as_np(mean).reshape(B, V, nc)[:, 0], as_np(ent).reshape(B, V)[:, 0]
                assert (mv[:, 0] == 1.0).all() and (mv[:, 1:] == 0.0).all() and (hv == 0.0).all()
                hu = as_np(ent).reshape(B, V)[:, 1]
                assert float(np.abs(hu - math.log(nc)).max()) <= bound_entropy(nc, n, e32["entropy"])
    print(f"mc kernels {dtype} nc={nc} V={V}: worst |err| sum/draw {worst['sum']:.3g} mean {worst['mean']:.3g} entropy {worst['entropy']:.3g}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda v: str(v).replace("torch.", ""))
@pytest.mark.parametrize("nc", NCS)
def test_exact_zero_probabilities_give_exact_mean_and_zero_entropy(dev, dtype, nc):
    """Logits with a +-80 spread: exp(-160) is 0 in fp32, the softmax is exactly {1, 0, ..}.  Draws that disagree on the winning class
    give exact dyadic means (1/2, 1/4), whose entropy has no 0 * -inf term; all-agreeing draws give entropy 0.0 exactly."""
    R, B, V = 4, 1, 9
    x = np.full((R * B, V, nc), -80.0, np.float32)
    x[:, :, 0] = 80.0                                  # every draw: class 0
    x[2:, 3, 0], x[2:, 3, 1] = -80.0, 80.0             # voxel 3: two draws for class 0, two for class 1
    x[3, 5, 0], x[3, 5, 1] = -80.0, 80.0               # voxel 5: three to one
    with torch.no_grad():
        s = ops.mc_accum(_five(torch.from_numpy(x).to(dtype), dev), R)
        mean, ent = ops.mc_finish(s, R)
    m, h = as_np(mean).reshape(V, nc), as_np(ent).reshape(V)
    assert np.isfinite(m).all() and np.isfinite(h).all()
    want = np.zeros((V, nc), np.float32)
    want[:, 0] = 1.0
    want[3, :2] = 0.5
    want[5, :2] = (0.75, 0.25)
    assert np.array_equal(m, want)
    rest = [v for v in range(V) if v not in (3, 5)]
    assert (h[rest] == 0.0).all() and not np.signbit(h[rest]).any()
    _, h64 = r_finish(want.astype(np.float64), 1, np.float64)
    assert float(np.abs(h - h64).max()) <= (nc + 2) * U * (1 + math.log(nc))
    # one voxel, equal logits: ln(nc)
    with torch.no_grad():
        s = ops.mc_accum(torch.full((1, 1, 1, 1, nc), 1.5, dtype=dtype, device=dev), 1)
        _, e1 = ops.mc_finish(s, 1)
    assert abs(float(e1) - math.log(nc)) <= (k_p(nc) + 1 + nc + 2) * U * (1 + math.log(nc))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,nc,V", list(itertools.product(DTYPES, NCS, VS)), ids=lambda v: str(v).replace("torch.", ""))
def test_single_draw_equals_softmax_heads_bit_for_bit(dev, dtype, nc, V):
    """R = 1, accumulate = 0, n = 1: ``mean`` and the per-draw output ARE m1_softmax_heads_fwd's probabilities."""
    lg = _five(make_logits(2, 1, V, nc, dtype, 7)[0], dev)
    with torch.no_grad():
        want = ops.softmax_heads([lg], [(1, 1, 1)])
        s, draws = ops.mc_accum(lg, 1, samples=True)
        assert torch.equal(draws[0].view(torch.int32), want.view(torch.int32))
        mean, _ = ops.mc_finish(s, 1)
    assert torch.equal(mean.view(torch.int32), want.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda v: str(v).replace("torch.", ""))
def test_unaligned_buffers_take_the_element_path_with_the_same_bits(dev, dtype):
    """Buffers one element off a 16-byte boundary cannot use vector accesses: the element path must give the bits of the vector path
    (B * V * nc = 1304 elements per replica: a multiple of 16 bytes in both types, so the aligned call does take 16-byte accesses;
    652 voxels leave a tail behind the groups of 8)."""
    B, R, V, nc = 2, 3, 326, 2
    lg = _five(make_logits(B, R, V, nc, dtype, 11)[0], dev)
    with torch.no_grad():
        s0, d0 = ops.mc_accum(lg, R, samples=True)
        m0, h0 = ops.mc_finish(s0.clone(), R)
        off = lambda t: torch.cat([t.reshape(-1)[:1], t.reshape(-1)])[1:].view(t.shape)      # the same values, one element further
        lg1, s1, d1 = off(lg), off(torch.empty_like(s0)), off(torch.empty_like(d0))
        assert lg1.data_ptr() % 16 and s1.data_ptr() % 16 and d1.data_ptr() % 16
        assert torch.equal(ops.mc_accum(lg1, R), s0)                                         # (aligned accumulator, unaligned logits)
        rc = L.load().m1_mc_accum(lg1.data_ptr(), R, B, V, nc, ops._dt(lg1), s1.data_ptr(), 0, d1.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        assert torch.equal(s1, s0) and torch.equal(d1, d0)
        h1 = off(torch.empty_like(h0))
        rc = L.load().m1_mc_finish(s1.data_ptr(), R, B, V, nc, s1.data_ptr(), h1.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0 and torch.equal(s1, m0) and torch.equal(h1, h0)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda v: str(v).replace("torch.", ""))
def test_guard_bands_stay_untouched(dev, dtype, monkeypatch):
    """Every tensor of both ops between guard bands (tests/guarded.py): the single voxel and the tail shape, with and without
    replicas, accumulating and not, with and without the per-draw output."""
    with guarded(monkeypatch) as g, torch.no_grad():
        for V, nc, (B, R) in itertools.product((1, 64 * 5 + 3), NCS, ((1, 1), (2, 3))):
            passes = make_logits(B, R, V, nc, dtype, 5)
            sum_p = g.empty((B, 1, 1, V, nc), dtype=torch.float32, device=dev)
            draws = g.empty((R, B, 1, 1, V, nc), dtype=torch.float32, device=dev)
            lib = L.load()
            st = torch.cuda.current_stream().cuda_stream
            for k, lg in enumerate(passes[:2]):
                x = g.put(lg.reshape(R * B, 1, 1, V, nc), dtype=dtype)
                assert lib.m1_mc_accum(x.data_ptr(), R, B, V, nc, ops._dt(x), sum_p.data_ptr(), k, draws.data_ptr() if k else None, st) == 0
            fresh = ops.mc_accum(g.put(passes[2].reshape(R * B, 1, 1, V, nc), dtype=dtype), R, samples=True)      # the op's own allocations
            mean, ent = ops.mc_finish(sum_p, 2 * R)
            ops.mc_finish(fresh[0], R)
            assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(ent).all()) and bool(torch.isfinite(draws).all())
            assert g.check() >= 6


# ---------------------------------------------------------------------------------------------------------------------------------
# predict_mc
# ---------------------------------------------------------------------------------------------------------------------------------
def _cfg(prob, **kw):
    return O.M1Config(input_spatial_dims=DIMS, filters=C1_FILTERS, strides=C1_STRIDES, dense_skip=prob, probabilistic=prob,
                      prob_latent_dims=(3, 2, 1, 0), **kw)


@pytest.fixture(scope="module")
def prob_model(dev):
    cfg = _cfg(True, dropout_rate=0.5, dropout_mode="monte-carlo")
    m = build_m1(cfg, dev)
    load_params_into(m, O.fixture_params(cfg, seed=61))
    m.eval()
    return m, m.get_detect_model(), rnd((2, *DIMS, 3), 62).to(dev)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _entropy64(mean):
    return r_finish(as_np(mean).astype(np.float64), 1, np.float64)[1]


def _manual_draws(m, dm, x, n):
    out = []
    for _ in range(n):
        out.append(dm.predict(x).clone())
        m.advance_rng()
    return out


@pytest.mark.gpu
def test_one_draw_is_predict_and_the_stream_advances(prob_model):
    m, dm, x = prob_model
    m.seed_dropout(41)
    want = dm.predict(x).clone()
    assert int(m.rng_state[1]) == 0
    r = dm.predict_mc(x, 1)
    assert set(r) == {"mean", "entropy"} and r["mean"].dtype == torch.float32 and r["entropy"].dtype == torch.float32
    assert tuple(r["mean"].shape) == (2, *DIMS, 2) and tuple(r["entropy"].shape) == (2, *DIMS)
    assert _bits_equal(r["mean"], want)
    assert int(m.rng_state[0]) == 41 and int(m.rng_state[1]) == 1


@pytest.mark.gpu
def test_four_draws_are_four_predicts_with_an_advance_between(prob_model):
    m, dm, x = prob_model
    m.seed_dropout(42)
    manual = _manual_draws(m, dm, x, 4)
    m.seed_dropout(42)
    r = dm.predict_mc(x, 4, return_samples=True)
    assert tuple(r["samples"].shape) == (4, 2, *DIMS, 2) and int(m.rng_state[1]) == 4
    for k in range(4):
        assert _bits_equal(r["samples"][k], manual[k]), k
    mean64 = torch.stack(manual).double().mean(dim=0)
    err = float((r["mean"].double() - mean64).abs().max())
    print("predict_mc n=4: max |mean - fp64 mean of four predicts|", err)
    assert err <= 4 * U


@pytest.mark.gpu
def test_consecutive_calls_differ_and_a_seed_reproduces_them(prob_model):
    m, dm, x = prob_model
    m.seed_dropout(43)
    a = dm.predict_mc(x, 2)
    b = dm.predict_mc(x, 2)
    assert int(m.rng_state[1]) == 4
    assert not torch.equal(a["mean"], b["mean"]) and not torch.equal(a["entropy"], b["entropy"])
    m.seed_dropout(43)
    c = dm.predict_mc(x, 2)
    assert _bits_equal(c["mean"], a["mean"]) and _bits_equal(c["entropy"], a["entropy"])
    # what a loop over predict() gives instead: the stream state does not move, every call is the same sample
    m.seed_dropout(43)
    assert _bits_equal(dm.predict(x), dm.predict(x)) and int(m.rng_state[1]) == 0


@pytest.mark.gpu
def test_replicated_passes_draw_independently(prob_model):
    m, dm, x = prob_model
    m.seed_dropout(44)
    r = dm.predict_mc(x, 4, draws_per_pass=2, return_samples=True)
    assert int(m.rng_state[1]) == 2
    s = r["samples"]
    for i, j in itertools.combinations(range(4), 2):
        assert not torch.equal(s[i], s[j]), (i, j)
    err = float((r["mean"].double() - s.double().mean(dim=0)).abs().max())
    assert err <= 4 * U, err
    nc = 2
    with np.errstate(all="ignore"):
        h64 = _entropy64(r["mean"])
        h32 = r_finish(as_np(r["mean"]), 1, np.float32)[1]
    e32 = float(np.abs(h32.astype(np.float64) - h64).max())
    eh = float(np.abs(as_np(r["entropy"]) - h64).max())
    print("predict_mc n=4 R=2: max |mean - fp64 mean of samples|", err, "max |entropy - restatement(mean)|", eh)
    assert eh <= max((nc + 2) * U * (1 + math.log(nc)), 4 * e32)             # from the given mean: logf (2), product, nc - 1 subtractions


@pytest.mark.gpu
def test_deterministic_model_without_dropout_returns_its_softmax(dev):
    cfg = _cfg(False, deep_supervision=True, dropout_rate=0.0)
    m = build_m1(cfg, dev)
    load_params_into(m, O.fixture_params(cfg, seed=63))
    m.eval()
    dm, x = m.get_detect_model(), rnd((2, *DIMS, 3), 64).to(dev)
    want = dm.predict(x).contiguous()
    r1 = dm.predict_mc(x, 1)
    assert _bits_equal(r1["mean"], want)
    r3 = dm.predict_mc(x, 3, return_samples=True)
    assert all(_bits_equal(r3["samples"][k], want) for k in range(3))
    assert float((r3["mean"].double() - want.double()).abs().max()) <= 3 * U
    nc = 2
    with np.errstate(all="ignore"):
        h64 = _entropy64(want)
    for r, n in ((r1, 1), (r3, 3)):
        # entropy of the single softmax: the mean is off by at most n * 2^-24 (0 for n = 1), then logf (2), product, nc - 1 subtractions
        assert float(np.abs(as_np(r["entropy"]) - h64).max()) <= (n + nc + 2) * U * (1 + math.log(nc)), n


@pytest.mark.gpu
def test_cascaded_probabilistic_model_returns_both_stages(dev):
    cfg = _cfg(True, dropout_rate=0.5, dropout_mode="monte-carlo")
    m = build_m1(cfg, dev, cascaded="noisy-or")
    P = O.fixture_params(cfg, seed=65, shapes=O.cascade_param_shapes(cfg))
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if k != "rng_state":
                v.copy_(P[k.replace("m1_stage", "stage")].to(v.device, v.dtype))
    m.eval()
    dm = m.get_detect_model()
    x = [rnd((2, *DIMS, 3), 66).to(dev), rnd((2, *DIMS, 3), 67).to(dev)]
    m.seed_dropout(45)
    want = [t.clone() for t in dm(x)]
    r = dm.predict_mc(x, 1)
    assert isinstance(r, list) and len(r) == 2 and int(m.rng_state[1]) == 1
    for got, w in zip(r, want):
        assert set(got) == {"mean", "entropy"} and _bits_equal(got["mean"], w)
    m.seed_dropout(45)
    r2 = dm.predict_mc({"image_1": x[0], "image_2": x[1]}, 2, draws_per_pass=2, return_samples=True)
    assert tuple(r2[1]["samples"].shape) == (2, 2, *DIMS, 2) and int(m.rng_state[1]) == 1
    assert not torch.equal(r2[1]["samples"][0], r2[1]["samples"][1])


def test_argument_errors():
    cfg = _cfg(True)
    init = PKG.initializers
    m = PKG.unets.networks.M1(input_spatial_dims=DIMS, input_channels=3, num_classes=2, dropout_rate=0.0, filters=C1_FILTERS,
                              strides=C1_STRIDES, dense_skip=True, probabilistic=True, prob_latent_dims=cfg.prob_latent_dims,
                              kernel_regularizer=init.l2(0.0), bias_regularizer=init.l2(0.0), summary=False)
    dm = m.get_detect_model()
    x = torch.zeros(1, *DIMS, 3)
    with pytest.raises(ValueError):
        dm.predict_mc(x, 0)
    with pytest.raises(ValueError):
        dm.predict_mc(x, 4, draws_per_pass=3)
    with pytest.raises(ValueError):
        dm.predict_mc(x, 2, eps_p=[torch.zeros(1)])
    with pytest.raises(RuntimeError, match="GPU"):                     # a valid call reaches _prep, which refuses host tensors
        dm.predict_mc(x, 2)


@pytest.mark.gpu
def test_wrong_input_shape_fails_through_prep(prob_model):
    _, dm, x = prob_model
    with pytest.raises(ValueError, match="expected input of shape"):
        dm.predict_mc(x[:, :, :16], 2)


@pytest.mark.gpu
def test_captured_call_replays_the_eager_result(prob_model):
    """predict_mc(x, 2) captured on a side stream after one warm-up call: no memset node, and a replay from a restored {seed, step}
    equals the eager call from that state bit for bit (the state advance is part of the graph)."""
    m, dm, x = prob_model
    m.seed_dropout(46)
    state = m.rng_state.clone()
    eager = dm.predict_mc(x, 2)
    eager = {k: v.clone() for k, v in eager.items()}
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        dm.predict_mc(x, 2)
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(gr):
        out = dm.predict_mc(x, 2)
    hist = PKG.hip.graphs.assert_no_memset_nodes(gr)
    assert hist.get("kernel", 0) > 50, hist                            # (two passes of the prior network + accumulate, advance, finish)
    gr.instantiate()
    with torch.no_grad():
        m.rng_state.copy_(state)
    gr.replay()
    torch.cuda.synchronize()
    assert _bits_equal(out["mean"], eager["mean"]) and _bits_equal(out["entropy"], eager["entropy"])
    assert int(m.rng_state[1]) == int(state[1]) + 2
    gr.replay()                                                        # the next two draws: another result
    torch.cuda.synchronize()
    assert not torch.equal(out["mean"], eager["mean"]) and int(m.rng_state[1]) == int(state[1]) + 4
