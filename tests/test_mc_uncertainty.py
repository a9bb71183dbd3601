"""Uncertainty maps of the Monte-Carlo draws (csrc/mc.hip: m1_mc_accum_u, m1_mc_finish_u; ops.mc_accum_u / ops.mc_finish_u;
``predict_mc(..., uncertainty=True)``, ``predict_scan(..., uncertainty=True)``, ``unets.networks.Ensemble``).

Kernel level: per element against the fp64 restatement of tests/mc_uncertainty_ref.py under |got - ref64| <= max(k * 2^-24 * scale,
4 * e32); the counts k are derived in that module's docstring.  ``test_fp32_restatement_stays_inside_the_first_term`` checks on the CPU
that the fp32 restatement alone meets the first term in every kernel-level case, which is the condition for asserting it on the GPU;
``test_wrong_restatements_break_the_bound`` that the bound is tight enough to tell the definitions from four near misses.
Model level: test_mc_inference.py's configuration, fp32 and bf16 compute, the probabilistic and the deterministic model; the maps are
restated from the returned samples (exact fp32 inputs: the counts with K_P = 0).  Worst errors measured on the MI355X: DESIGN.md
section 7."""
import ctypes
import functools
import itertools
import math

import numpy as np
import pytest
import torch

from oracle import m1_oracle as O
from util import C1_FILTERS, C1_STRIDES, PKG, build_m1, load_params_into, ops, rnd
from test_mc_inference import DIMS, DTYPES, PASSES, as_np, make_logits
import mc_uncertainty_ref as Rf

L = PKG.hip.lib
NW = PKG.unets.networks
P = PKG.preprocess
BS, RS, NCS, VS = (1, 2), (1, 3), (2, 3, 4), (1, 7, 64 * 5 + 3, 4 * 32 * 32)
ALL_CASES = list(itertools.product(DTYPES, NCS, VS, BS, RS))
MAPS = ("mean", "entropy", "expected_entropy", "mutual_info", "variance")
_ID = lambda v: str(v).replace("torch.", "")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _case(dtype, nc, V, B, R):
    """The logits of one kernel-level case (exact in ``dtype``) and its references, computed once and shared by every test."""
    passes = make_logits(B, R, V, nc, dtype, 300 + ALL_CASES.index((dtype, nc, V, B, R)))
    with np.errstate(all="ignore"):
        return passes, Rf.case_refs_u([as_np(t) for t in passes], R)


@functools.lru_cache(maxsize=None)
def _near_case(dtype):
    """Nearly equal draws: base logits + 1e-3 * noise per draw (fp32 logits keep the noise; in bf16 most of it rounds away, which is
    the other way to get draws that agree, and the few that do not differ by a whole bf16 step).  mutual_info is about 1e-7 and nowhere
    above 1e-4: the subtraction cancels and the clamp acts."""
    B, R, V, nc = 2, 3, 64 * 5 + 3, 2
    g = np.random.default_rng(77)
    base = np.clip(g.standard_normal((1, B, V, nc)) * 2.5, -6, 6)
    passes = [torch.from_numpy((base + 1e-3 * g.standard_normal((R, B, V, nc))).reshape(R * B, V, nc).astype(np.float32)).to(dtype)
              for _ in range(PASSES)]
    with np.errstate(all="ignore"):
        refs = Rf.case_refs_u([as_np(t) for t in passes], R)
    assert refs[2]["mutual_info"].max() < 1e-4 and np.median(refs[2]["mutual_info"]) < 1e-6
    return passes, refs, (B, R, V, nc)


# ---------------------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound():
    lib = L.load()
    for name in ("m1_mc_accum_u", "m1_mc_finish_u"):
        assert name in L.SIGNATURES and hasattr(lib, name)


def test_bad_arguments_are_rejected_without_a_gpu():
    lib = L.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    acc = lambda *a: lib.m1_mc_accum_u(*a)
    assert acc(None, 1, 1, 1, 2, 0, p, p, p, 0, None, None) == -1                    # NULL logits
    assert acc(p, 1, 1, 1, 2, 0, None, p, p, 0, None, None) == -1                    # NULL accumulators, one by one
    assert acc(p, 1, 1, 1, 2, 0, p, None, p, 0, None, None) == -1
    assert acc(p, 1, 1, 1, 2, 0, p, p, None, 0, None, None) == -1
    assert acc(p, 0, 1, 1, 2, 0, p, p, p, 0, None, None) == -1                       # R = 0
    assert acc(p, 1, 0, 1, 2, 0, p, p, p, 0, None, None) == -1 and acc(p, 1, 1, 0, 2, 0, p, p, p, 0, None, None) == -1
    assert acc(p, 1, 1, 1, 2, 7, p, p, p, 0, None, None) == -1                       # unknown dtype
    assert acc(p, 1, 1, 1, 5, 0, p, p, p, 0, None, None) == -2 and acc(p, 1, 1, 1, 1, 0, p, p, p, 0, None, None) == -2
    assert acc(p + 2, 1, 1, 1, 2, 0, p, p, p, 0, None, None) == -1                   # fp32 logits off their element alignment
    assert acc(p + 1, 1, 1, 1, 2, 1, p, p, p, 0, None, None) == -1                   # bf16 logits at an odd address
    for k in range(3):                                                               # each accumulator, and the samples, misaligned
        ptrs = [p, p, p]
        ptrs[k] = p + 2
        assert acc(p, 1, 1, 1, 2, 0, *ptrs, 0, None, None) == -1
    assert acc(p, 1, 1, 1, 2, 0, p, p, p, 0, p + 2, None) == -1
    assert acc(p, 2, 1 << 20, 1 << 20, 2, 0, p, p, p, 0, None, None) == -1           # M above 2^40 / R
    fin = lambda *a: lib.m1_mc_finish_u(*a)
    good = [p, p, p, 1, 1, 1, 2, p, p, p, p, p, None]
    for k in (0, 1, 2, 7, 8, 9, 10, 11):                                             # every pointer: NULL, then misaligned
        a = list(good)
        a[k] = None
        assert fin(*a) == -1, k
        a[k] = p + 2
        assert fin(*a) == -1, k
    assert fin(p, p, p, 0, 1, 1, 2, p, p, p, p, p, None) == -1                       # n_draws = 0
    assert fin(p, p, p, 1, 0, 1, 2, p, p, p, p, p, None) == -1 and fin(p, p, p, 1, 1, 0, 2, p, p, p, p, p, None) == -1
    assert fin(p, p, p, 1, 1, 1, 5, p, p, p, p, p, None) == -2 and fin(p, p, p, 1, 1, 1, 1, p, p, p, p, p, None) == -2
    assert fin(p, p, p, 1, 1 << 21, 1 << 20, 2, p, p, p, p, p, None) == -1           # M above 2^40


def test_ops_refuse_to_run_under_autograd_and_check_their_arguments():
    t = torch.zeros(1, 1, 1, 1, 2)
    with pytest.raises(RuntimeError, match="no_grad"):
        ops.mc_accum_u(t, 1)
    with pytest.raises(RuntimeError, match="no_grad"):
        ops.mc_finish_u((t, t[..., 0], t), 1)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="GPU"):
            ops.mc_accum_u(t, 1)
        with pytest.raises(RuntimeError, match="sum_p, sum_h, sum_pp"):
            ops.mc_finish_u((t, t), 1)


def test_hand_cases():
    """Two one-hot draws of different classes: all of the entropy is disagreement (mutual_info = ln 2, expected_entropy = 0, variance
    1/4); two equal 50 / 50 draws: all of it is ambiguity every draw agrees on (the reverse, variance 0)."""
    for nc in NCS:
        onehot = np.zeros((2, 1, 1, nc))
        onehot[0, 0, 0, 0] = onehot[1, 0, 0, 1] = 1.0
        half = np.zeros((2, 1, 1, nc))
        half[:, 0, 0, :2] = 0.5
        for vt in (np.float64, np.float32):
            with np.errstate(all="ignore"):
                (h, q), = Rf.r_fold_u([onehot], vt)
                a = Rf.r_finish_u(onehot.sum(0).astype(vt), h, q, 2, vt)
                (h, q), = Rf.r_fold_u([half], vt)
                b = Rf.r_finish_u(half.sum(0).astype(vt), h, q, 2, vt)
            tol = 4 * float(np.finfo(vt).eps)
            assert abs(float(a["mutual_info"][0, 0]) - math.log(2)) <= tol and float(a["expected_entropy"][0, 0]) == 0.0
            assert np.array_equal(a["variance"][0, 0, :2], [0.25, 0.25]) and abs(float(a["entropy"][0, 0]) - math.log(2)) <= tol
            assert float(b["mutual_info"][0, 0]) == 0.0 and abs(float(b["expected_entropy"][0, 0]) - math.log(2)) <= tol
            assert (b["variance"] == 0).all()


def test_fp32_restatement_stays_inside_the_first_term():
    """k * 2^-24 * scale holds for the fp32-valued restatement of every output in every kernel-level case of the GPU tests, after
    every pass for the sums; and with one draw the fp32 restatement gives mutual_info and variance exactly 0."""
    worst = {}
    cases = [(*_case(*c), c[1], c[4]) for c in ALL_CASES]
    for dtype in DTYPES:
        passes, refs, (_, R, _, nc) = _near_case(dtype)
        cases.append((passes, refs, nc, R))
    for passes, (s64, d64, m64, e32), nc, R in cases:
        for k in range(len(passes)):
            n = R * (k + 1)
            for what in ("sum_p", "sum_h", "sum_pp"):
                assert e32[what][k] <= Rf.first_term(nc, n, what), (what, nc, R, n, e32[what][k])
                worst[what] = max(worst.get(what, 0.0), e32[what][k] / Rf.first_term(nc, n, what))
        n = R * len(passes)
        for what in MAPS:
            assert e32[what] <= Rf.first_term(nc, n, what), (what, nc, R, e32[what])
            worst[what] = max(worst.get(what, 0.0), e32[what] / Rf.first_term(nc, n, what))
    print("fp32 restatement, worst error as a share of the first term:", {k: round(v, 3) for k, v in worst.items()})
    for dtype, nc in itertools.product(DTYPES, NCS):
        lg = [as_np(make_logits(2, 1, 64 * 5 + 3, nc, dtype, 9)[0])]
        with np.errstate(all="ignore"):
            (sp, sh, sq), = Rf.r_accum_u(lg, 1, np.float32)[0]
            m = Rf.r_finish_u(sp, sh, sq, 1, np.float32)
        assert (m["mutual_info"] == 0).all() and (m["variance"] == 0).all() and np.array_equal(m["entropy"], m["expected_entropy"])


@pytest.mark.parametrize("wrong,what", [(dict(var_div="n-1"), "variance"), (dict(log_base=2.0), "expected_entropy"),
                                        (dict(log_base=2.0), "entropy"), (dict(mi_from_mean=True), "mutual_info"),
                                        (dict(ee_div=False), "expected_entropy")], ids=lambda v: str(v))
def test_wrong_restatements_break_the_bound(wrong, what):
    """Variance over n - 1, entropy in bits, mutual_info as entropy - H(mean) and an expected entropy that is not divided by n, each in
    fp64: the output it changes leaves the bound in every multi-draw case it is tried on."""
    for dtype, nc in itertools.product(DTYPES, NCS):
        B, R, V = 2, 3, 64 * 5 + 3
        passes, (s64, d64, m64, e32) = _case(dtype, nc, V, B, R)
        n = R * len(passes)
        kw = {k: (n - 1 if v == "n-1" else v) for k, v in wrong.items()}
        with np.errstate(all="ignore"):
            bad = Rf.r_finish_u(*s64[-1], n, np.float64, **kw)
        err = float(np.abs(bad[what] - m64[what]).max())
        assert err > Rf.bound(nc, n, what, e32[what]), (dtype, nc, what, err)


def _m1(cascaded=False, classes=2, dims=DIMS, channels=3):
    init = PKG.initializers
    return NW.M1(input_spatial_dims=dims, input_channels=channels, num_classes=classes, dropout_rate=0.0, filters=C1_FILTERS,
                 strides=C1_STRIDES, dense_skip=True, probabilistic=True, prob_latent_dims=(3, 2, 1, 0), cascaded=cascaded,
                 kernel_regularizer=init.l2(0.0), bias_regularizer=init.l2(0.0), summary=False)


def test_ensemble_constructor_errors():
    a = _m1()
    with pytest.raises(ValueError, match="at least one"):
        NW.Ensemble([])
    with pytest.raises(ValueError, match="num_classes"):
        NW.Ensemble([a, _m1(classes=3)])
    with pytest.raises(ValueError, match="input_spatial_dims"):
        NW.Ensemble([a, _m1(dims=(4, 32, 64))])
    with pytest.raises(ValueError, match="input_channels"):
        NW.Ensemble([a, _m1(channels=2)])
    with pytest.raises(ValueError, match="not an M1"):
        NW.Ensemble([a, torch.nn.Linear(1, 1)])
    with pytest.raises(NotImplementedError, match="cascaded"):
        NW.Ensemble([a, _m1(cascaded="noisy-or")])
    e = NW.Ensemble([a, _m1()], seed=7)
    assert [int(m.rng_state[0]) for m in e.models] == [7, 8] and all(int(m.rng_state[1]) == 0 for m in e.models)
    with pytest.raises(ValueError):
        e.predict_mc(torch.zeros(1, *DIMS, 3), 4, draws_per_pass=3)
    with pytest.raises(RuntimeError, match="GPU"):
        e.predict_mc(torch.zeros(1, *DIMS, 3), 2, uncertainty=True)


def test_ensemble_load_reads_checkpoints_and_fold_directories(tmp_path):
    PKG.unets.network_blocks.set_init_seed(3)
    a = _m1()
    (tmp_path / "F0").mkdir()
    a.save_weights(str(tmp_path / "F0" / "model_weights_001.npz"))
    a.save_weights(str(tmp_path / "model_weights_007.npz"))
    e = NW.Ensemble.load([str(tmp_path / "F0"), str(tmp_path / "model_weights_007.npz")], "cpu", compute_dtype=torch.bfloat16, seed=11)
    assert len(e.models) == 2 and all(m.compute_dtype == torch.bfloat16 and not m.training for m in e.models)
    assert [int(m.rng_state[0]) for m in e.models] == [11, 12]
    for m in e.models:
        for (k, v), (_, w) in zip(m.state_dict().items(), a.state_dict().items()):
            assert k == "rng_state" or torch.equal(v, w), k
    (tmp_path / "empty").mkdir()
    with pytest.raises(FileNotFoundError):
        NW.Ensemble.load([str(tmp_path / "empty")], "cpu")


# ---------------------------------------------------------------------------------------------------------------------------------
# kernels on the GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def _five(t, dev):
    """(N, V, nc) host tensor -> contiguous (N, 1, 1, V, nc) on the device."""
    return t.reshape(t.shape[0], 1, 1, t.shape[1], t.shape[2]).contiguous().to(dev)


def _check_maps(maps, m64, e32, nc, n, shape_bv, worst, tag):
    B, V = shape_bv
    got = {k: as_np(v).reshape(B, V, nc) if k in ("mean", "variance") else as_np(v).reshape(B, V) for k, v in maps.items() if k in MAPS}
    assert set(got) == set(MAPS)
    for what in MAPS:
        assert np.isfinite(got[what]).all(), (tag, what)
        err = float(np.abs(got[what].astype(np.float64) - m64[what]).max())
        worst[what] = max(worst.get(what, 0.0), err)
        assert err <= Rf.bound(nc, n, what, e32[what]), (tag, what, err, e32[what])
    assert (got["mutual_info"] >= 0).all() and (got["variance"] >= 0).all() and (got["expected_entropy"] >= 0).all()
    assert not np.signbit(got["mutual_info"]).any() and not np.signbit(got["variance"]).any()
    assert (got["mutual_info"] <= got["entropy"] + Rf.bound(nc, n, "mutual_info", e32["mutual_info"])).all(), tag
    assert (got["variance"] <= 0.25 + Rf.bound(nc, n, "variance", e32["variance"])).all(), tag
    return got


def _run_case(dev, passes, refs, B, R, V, nc, worst, tag):
    """accumulate = 0, 1, 1 over the passes into NaN-filled accumulators: the three sums after every pass, sum_p / samples against
    ops.mc_accum bit for bit, then the five maps, mean / entropy against ops.mc_finish bit for bit."""
    s64, d64, m64, e32 = refs
    acc = tuple(torch.full(s, float("nan"), device=dev) for s in ((B, 1, 1, V, nc), (B, 1, 1, V), (B, 1, 1, V, nc)))
    old = None
    for k, lg in enumerate(passes):
        x = _five(lg, dev)
        if k == 0:
            rc = L.load().m1_mc_accum_u(x.data_ptr(), R, B, V, nc, ops._dt(x), acc[0].data_ptr(), acc[1].data_ptr(), acc[2].data_ptr(), 0,
                                        None, torch.cuda.current_stream().cuda_stream)
            assert rc == 0
            fresh = ops.mc_accum_u(x, R)                                         # the op's allocating form: the same write
            assert all(_bits_equal(a, b) for a, b in zip(fresh, acc))
            old = ops.mc_accum(x, R)
        else:
            r, draws = ops.mc_accum_u(x, R, acc, samples=True)
            assert all(a.data_ptr() == b.data_ptr() for a, b in zip(r, acc))
            old, odraws = ops.mc_accum(x, R, old, samples=True)
            assert _bits_equal(draws, odraws), (tag, k)
        assert _bits_equal(acc[0], old), (tag, k)
        n = R * (k + 1)
        for i, what in enumerate(("sum_p", "sum_h", "sum_pp")):
            got = as_np(acc[i]).reshape(s64[k][i].shape).astype(np.float64)
            assert np.isfinite(got).all(), (tag, what, "NaN left in the accumulator")
            err = float(np.abs(got - s64[k][i]).max())
            worst[what] = max(worst.get(what, 0.0), err / n)
            assert err <= Rf.bound(nc, n, what, e32[what][k]), (tag, what, n, err, e32[what][k])
    n = R * len(passes)
    maps = ops.mc_finish_u(acc, n)
    assert maps["mean"].data_ptr() == acc[0].data_ptr() and maps["expected_entropy"].data_ptr() == acc[1].data_ptr()
    assert maps["variance"].data_ptr() == acc[2].data_ptr() and tuple(maps["mutual_info"].shape) == (B, 1, 1, V)
    mean, ent = ops.mc_finish(old, n)
    assert _bits_equal(maps["mean"], mean) and _bits_equal(maps["entropy"], ent), tag
    return _check_maps(maps, m64, e32, nc, n, (B, V), worst, tag)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,nc,V", list(itertools.product(DTYPES, NCS, VS)), ids=_ID)
def test_accumulators_and_maps_match_the_fp64_restatement(dev, dtype, nc, V):
    worst = {}
    with torch.no_grad(), np.errstate(all="ignore"):
        for B, R in itertools.product(BS, RS):
            passes, refs = _case(dtype, nc, V, B, R)
            got = _run_case(dev, passes, refs, B, R, V, nc, worst, (B, R))
            if V >= 7:
                # the +-80 voxel: every draw exactly one-hot on class 0 -> all five maps exact; the equal-logit voxel: every draw
                # uniform -> entropy = expected_entropy = ln nc to the bound, no disagreement beyond it
                assert (got["expected_entropy"][:, 0] == 0).all() and (got["mutual_info"][:, 0] == 0).all() and (got["variance"][:, 0] == 0).all()
                n = R * PASSES
                assert float(np.abs(got["expected_entropy"][:, 1] - math.log(nc)).max()) <= Rf.bound(nc, n, "expected_entropy", refs[3]["expected_entropy"])
    print(f"mc_u kernels {dtype} nc={nc} V={V}: worst |err| " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_nearly_equal_draws_cancel_inside_the_bound(dev, dtype):
    passes, refs, (B, R, V, nc) = _near_case(dtype)
    worst = {}
    with torch.no_grad(), np.errstate(all="ignore"):
        got = _run_case(dev, passes, refs, B, R, V, nc, worst, "near")
    print(f"nearly equal draws {dtype}: largest mutual_info {got['mutual_info'].max():.3g} (ref {refs[2]['mutual_info'].max():.3g}), "
          f"zeros after the clamp {int((got['mutual_info'] == 0).sum())} of {got['mutual_info'].size}; worst |err| {worst}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,nc,V", list(itertools.product(DTYPES, NCS, VS)), ids=_ID)
def test_one_draw_has_no_disagreement_bit_for_bit(dev, dtype, nc, V):
    """One pass of R = 1, n = 1: expected_entropy IS entropy, and mutual_info = variance = +0 (p*p - p*p with rounded products)."""
    lg = _five(make_logits(2, 1, V, nc, dtype, 7)[0], dev)
    with torch.no_grad():
        m = ops.mc_finish_u(ops.mc_accum_u(lg, 1), 1)
        want = ops.softmax_heads([lg], [(1, 1, 1)])
    assert _bits_equal(m["mean"], want) and _bits_equal(m["expected_entropy"], m["entropy"])
    zero = torch.zeros_like(m["mutual_info"])
    assert _bits_equal(m["mutual_info"], zero) and _bits_equal(m["variance"], torch.zeros_like(m["variance"]))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_unaligned_buffers_take_the_element_path_with_the_same_bits(dev, dtype):
    """Views one element off a 16-byte boundary take G = 1 everywhere: the bits of the aligned call (B * V * nc = 1304 elements per
    replica, a multiple of 16 bytes in both types; 652 voxels leave a tail behind the groups of 8).  Two aligned runs: equal bits."""
    B, R, V, nc = 2, 3, 326, 2
    lgs = [_five(t, dev) for t in make_logits(B, R, V, nc, dtype, 11)[:2]]
    st = torch.cuda.current_stream().cuda_stream
    lib = L.load()
    off = lambda t: torch.cat([t.reshape(-1)[:1], t.reshape(-1)])[1:].view(t.shape)          # the same values, one element further
    with torch.no_grad():
        def aligned():
            a = ops.mc_accum_u(lgs[0], R)
            a, d = ops.mc_accum_u(lgs[1], R, a, samples=True)
            sums = [t.clone() for t in a]
            return sums, d, ops.mc_finish_u(a, 2 * R)
        s0, d0, m0 = aligned()
        s1, d1, m1 = aligned()
        assert all(_bits_equal(a, b) for a, b in zip(s0, s1)) and _bits_equal(d0, d1) and all(_bits_equal(m0[k], m1[k]) for k in MAPS)
        acc = [off(torch.empty_like(t)) for t in s0]
        d = off(torch.empty_like(d0))
        assert all(t.data_ptr() % 16 for t in (*acc, d))
        for k, lg in enumerate(lgs):
            x = off(lg)
            assert x.data_ptr() % 16
            rc = lib.m1_mc_accum_u(x.data_ptr(), R, B, V, nc, ops._dt(x), acc[0].data_ptr(), acc[1].data_ptr(), acc[2].data_ptr(), k,
                                   d.data_ptr() if k else None, st)
            assert rc == 0
        assert all(_bits_equal(a, b) for a, b in zip(acc, s0)) and _bits_equal(d, d0)
        # one unaligned pointer is enough: aligned accumulators, unaligned logits
        a2 = ops.mc_accum_u(off(lgs[0]), R)
        a2 = ops.mc_accum_u(off(lgs[1]), R, a2)
        assert all(_bits_equal(a, b) for a, b in zip(a2, s0))
        ent, mi = off(torch.empty_like(m0["entropy"])), off(torch.empty_like(m0["entropy"]))
        rc = lib.m1_mc_finish_u(acc[0].data_ptr(), acc[1].data_ptr(), acc[2].data_ptr(), 2 * R, B, V, nc, acc[0].data_ptr(), ent.data_ptr(),
                                acc[1].data_ptr(), mi.data_ptr(), acc[2].data_ptr(), st)
        assert rc == 0
        for got, k in zip((acc[0], ent, acc[1], mi, acc[2]), MAPS):
            assert _bits_equal(got, m0[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
@pytest.mark.parametrize("nc", NCS)
def test_a_nan_logit_marks_its_voxel_and_no_other(dev, dtype, nc):
    """One NaN logit in one draw of a voxel inside a group of G (the vector path) and of one in the tail behind the groups (the
    element path): all five maps of those voxels are NaN, every other voxel has the bits of the run without the NaN."""
    V = 64 * 5 + 3
    passes = make_logits(1, 1, V, nc, dtype, 13)                       # three passes of one draw: R = 1 keeps the groups of G
    hit = (21, V - 1)
    bad = [t.clone() for t in passes]
    bad[1][0, hit[0], nc - 1] = float("nan")
    bad[2][0, hit[1], 0] = float("nan")

    def run(ps):
        acc = None
        for t in ps:
            acc = ops.mc_accum_u(_five(t, dev), 1, acc)
        return ops.mc_finish_u(acc, len(ps))
    with torch.no_grad():
        clean, got = run(passes), run(bad)
    others = [v for v in range(V) if v not in hit]
    for k in MAPS:
        g, c = got[k].reshape(V, -1), clean[k].reshape(V, -1)
        assert bool(torch.isnan(g[list(hit)]).all()), k
        assert _bits_equal(g[others], c[others]) and bool(torch.isfinite(g[others]).all()), k


# ---------------------------------------------------------------------------------------------------------------------------------
# predict_mc, Ensemble, predict_scan
# ---------------------------------------------------------------------------------------------------------------------------------
def _cfg(prob, **kw):
    return O.M1Config(input_spatial_dims=DIMS, filters=C1_FILTERS, strides=C1_STRIDES, dense_skip=prob, probabilistic=prob,
                      prob_latent_dims=(3, 2, 1, 0), dropout_rate=0.5, dropout_mode="monte-carlo", **kw)


@pytest.fixture(scope="module", params=list(itertools.product(DTYPES, (True, False))), ids=lambda p: f"{_ID(p[0])}-{'prob' if p[1] else 'det'}")
def model(dev, request):
    dtype, prob = request.param
    cfg = _cfg(prob) if prob else _cfg(False, deep_supervision=True)
    m = build_m1(cfg, dev, dtype)
    load_params_into(m, O.fixture_params(cfg, seed=61))
    m.eval()
    return m, m.get_detect_model(), rnd((2, *DIMS, 3), 62).to(dev)


def _check_against_samples(r, n, R, nc=2):
    """The three new maps (and mean / entropy) against the restatement of the returned samples, taken as exact fp32 inputs in passes
    of R draws; returns the worst errors."""
    s = as_np(r["samples"])
    draws = [s[k * R:(k + 1) * R].reshape(R, s.shape[1], -1, nc) for k in range(n // R)]
    with np.errstate(all="ignore"):
        m64, e32 = Rf.refs_from_draws(draws, n)
    worst = {}
    for what in MAPS:
        got = as_np(r[what]).reshape(m64[what].shape).astype(np.float64)
        worst[what] = float(np.abs(got - m64[what]).max())
        assert worst[what] <= Rf.bound(nc, n, what, e32[what], from_samples=True), (what, worst[what], e32[what])
    return worst


@pytest.mark.gpu
def test_predict_mc_with_uncertainty_keeps_mean_entropy_samples_and_state(model):
    m, dm, x = model
    m.seed_dropout(71)
    a = dm.predict_mc(x, 6, 3, return_samples=True)
    sa = m.rng_state.clone()
    m.seed_dropout(71)
    b = dm.predict_mc(x, 6, 3, return_samples=True, uncertainty=True)
    assert set(b) == set(MAPS) | {"samples"} and torch.equal(m.rng_state, sa) and int(sa[1]) == 2
    assert torch.equal(a["mean"], b["mean"]) and torch.equal(a["entropy"], b["entropy"]) and torch.equal(a["samples"], b["samples"])
    assert tuple(b["expected_entropy"].shape) == (2, *DIMS) == tuple(b["mutual_info"].shape) and tuple(b["variance"].shape) == (2, *DIMS, 2)
    assert all(b[k].dtype == torch.float32 for k in MAPS)
    worst = _check_against_samples(b, 6, 3)
    print("predict_mc(6, 3, uncertainty): worst |err| against the restated samples", worst, "largest mutual_info", float(b["mutual_info"].max()))
    m.seed_dropout(71)
    c = dm.predict_mc(x, 6, 3, uncertainty=True)                       # without the samples: the same maps
    assert set(c) == set(MAPS) and all(torch.equal(b[k], c[k]) for k in MAPS)


@pytest.mark.gpu
def test_one_draw_has_exactly_zero_mutual_info_and_variance(model):
    m, dm, x = model
    m.seed_dropout(72)
    want = dm.predict(x).clone()
    r = dm.predict_mc(x, 1, uncertainty=True)
    assert torch.equal(r["mean"], want) and int(m.rng_state[1]) == 1
    assert _bits_equal(r["mutual_info"], torch.zeros_like(r["mutual_info"])) and _bits_equal(r["variance"], torch.zeros_like(r["variance"]))
    assert _bits_equal(r["expected_entropy"], r["entropy"])


@pytest.mark.gpu
def test_cascaded_model_returns_both_stages_with_the_new_maps(dev):
    cfg = _cfg(True)
    m = build_m1(cfg, dev, cascaded="noisy-or")
    params = O.fixture_params(cfg, seed=65, shapes=O.cascade_param_shapes(cfg))
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if k != "rng_state":
                v.copy_(params[k.replace("m1_stage", "stage")].to(v.device, v.dtype))
    m.eval()
    dm = m.get_detect_model()
    x = [rnd((2, *DIMS, 3), 66).to(dev), rnd((2, *DIMS, 3), 67).to(dev)]
    m.seed_dropout(73)
    a = dm.predict_mc(x, 2, 2)
    m.seed_dropout(73)
    b = dm.predict_mc(x, 2, 2, uncertainty=True, return_samples=True)
    assert isinstance(b, list) and len(b) == 2 and int(m.rng_state[1]) == 1
    for sa, sb in zip(a, b):
        assert set(sb) == set(MAPS) | {"samples"} and torch.equal(sa["mean"], sb["mean"]) and torch.equal(sa["entropy"], sb["entropy"])
        _check_against_samples(sb, 2, 2)


@pytest.fixture(scope="module")
def two_models(dev):
    """Two probabilistic models of the same configuration from different initial-weight seeds (two 'folds')."""
    ms = []
    for seed in (5, 6):
        PKG.unets.network_blocks.set_init_seed(seed)
        m = build_m1(_cfg(True), dev)
        m.eval()
        ms.append(m)
    return ms, rnd((2, *DIMS, 3), 68).to(dev)


@pytest.mark.gpu
def test_ensemble_folds_its_members_draws_member_major(two_models):
    ms, x = two_models
    e = NW.Ensemble(ms, seed=81)
    r = e.predict_mc(x, 4, 2, uncertainty=True, return_samples=True)
    assert tuple(r["samples"].shape) == (8, 2, *DIMS, 2) and set(r) == set(MAPS) | {"samples"}
    assert [int(m.rng_state[0]) for m in ms] == [81, 82] and all(int(m.rng_state[1]) == 2 for m in ms)     # n_draws / draws_per_pass
    worst = _check_against_samples(r, 8, 2)
    for i, m in enumerate(ms):                                         # member i's own call from the same state gives its slice
        m.seed_dropout(81 + i)
        own = m.get_detect_model().predict_mc(x, 4, 2, return_samples=True)
        assert torch.equal(own["samples"], r["samples"][4 * i:4 * i + 4]), i
    print("Ensemble of two, 2 x 4 draws: worst |err| against the restated samples", worst, "largest mutual_info", float(r["mutual_info"].max()))
    # the members in the other order: another summation order, the same maps to the bound
    for i, m in enumerate(ms):
        m.seed_dropout(81 + i)
    s = NW.Ensemble(ms[::-1]).predict_mc(x, 4, 2, uncertainty=True, return_samples=True)
    assert torch.equal(s["samples"][:4], r["samples"][4:]) and torch.equal(s["samples"][4:], r["samples"][:4])
    _check_against_samples(s, 8, 2)


@pytest.mark.gpu
def test_single_member_ensemble_is_the_model_bit_for_bit(two_models):
    ms, x = two_models
    m = ms[0]
    for kw in (dict(uncertainty=True, return_samples=True), dict()):
        m.seed_dropout(82)
        own = m.get_detect_model().predict_mc(x, 4, 2, **kw)
        st = m.rng_state.clone()
        m.seed_dropout(82)
        got = NW.Ensemble([m]).predict_mc(x, 4, 2, **kw)
        assert set(got) == set(own) and all(_bits_equal(got[k], own[k]) for k in own) and torch.equal(m.rng_state, st)
    # every entry point is one body for both: the same call on the detect model and on the ensemble of it, from the same seed
    calls = (lambda p: p.predict(x), lambda p: p.predict(x, tta=("", "w")),
             lambda p: p.predict_mc(x, 2, 2, tta=("", "hw"), uncertainty=True, return_samples=True))
    for i, call in enumerate(calls):
        m.seed_dropout(84 + i)
        own = call(m.get_detect_model())
        own = {k: v.clone() for k, v in own.items()} if isinstance(own, dict) else {"mean": own.clone()}
        st = m.rng_state.clone()
        m.seed_dropout(84 + i)
        got = call(NW.Ensemble([m]))
        got = got if isinstance(got, dict) else {"mean": got}
        assert set(got) == set(own) and all(_bits_equal(got[k], own[k]) for k in own) and torch.equal(m.rng_state, st), i


@pytest.mark.gpu
def test_ensemble_predict_is_the_mean_of_the_members_predict(two_models):
    ms, x = two_models
    e = NW.Ensemble(ms, seed=83)
    want = torch.stack([m.get_detect_model().predict(x).double() for m in ms]).mean(dim=0)
    got = e.predict(x)
    assert tuple(got.shape) == (2, *DIMS, 2) and got.dtype == torch.float32 and all(int(m.rng_state[1]) == 0 for m in ms)
    err = float((got.double() - want).abs().max())
    assert err <= Rf.first_term(2, 2, "mean", from_samples=True), err   # (from the members' fp32 softmaxes: one addition, one division)


SCAN, SCAN_SP, NET_SP = (5, 40, 40), (3.6, .4, .4), (3.0, .5, .5)


@pytest.mark.gpu
def test_predict_scan_restores_every_new_map(two_models, dev):
    ms, _ = two_models
    g = np.random.default_rng(91)
    raw = torch.from_numpy((g.standard_normal((2, *SCAN, 3)) * 200 + 400).astype(np.float32)).to(dev)
    x, _ = P.prepare_scan(raw, SCAN_SP, NET_SP, DIMS, percentile=99.5)
    for who, seed in ((ms[0].get_detect_model(), lambda: ms[0].seed_dropout(91)), (NW.Ensemble(ms), lambda: [m.seed_dropout(91) for m in ms])):
        for n in (1, 2):
            seed()
            net = who.predict_mc(x, n, uncertainty=True)
            seed()
            r = who.predict_scan(raw, SCAN_SP, NET_SP, n_draws=n, percentile=99.5, channels=1, uncertainty=True)
            assert set(r) == set(MAPS) | {"network"} and all(torch.equal(net[k], r["network"][k]) for k in MAPS)
            assert torch.equal(r["mean"], P.restore(net["mean"], SCAN, SCAN_SP, NET_SP, channels=1))
            for k in ("entropy", "expected_entropy", "mutual_info"):
                assert tuple(r[k].shape) == (2, *SCAN)
                assert torch.equal(r[k], P.restore(net[k].unsqueeze(-1), SCAN, SCAN_SP, NET_SP, order=1)[..., 0]), k
            assert tuple(r["variance"].shape) == (2, *SCAN, 1)
            assert torch.equal(r["variance"], P.restore(net["variance"], SCAN, SCAN_SP, NET_SP, order=1, channels=1))
        seed()
        plain = who.predict_scan(raw, SCAN_SP, NET_SP, percentile=99.5)             # the default call: no new key, a tensor from predict
        assert set(plain) == {"mean", "network"} and isinstance(plain["network"], torch.Tensor)
