"""The bootstrap kernel (csrc/bootstrap.hip, ops.bootstrap_metrics) against ``bootstrap.replicates_host``, which
tests/test_bootstrap_host.py holds to the explicit-resample oracle: AUROC and the sensitivities bit-equal, AP and the means within the
bound of one fp64 sum in another order (bootstrap_ref.assert_rows computes n and the sum of |terms| per replicate), NaN in the same
places; at most 32 replicates per call.

Shapes.  N in {1, 2, 3, 255, 256, 257, 1000, 16384}: one case, fewer cases than a thread's four, one chunk of 1024 minus / exactly /
plus a thread's worth around 256, several chunks, the LDS cap.  M in {0, 1, chunk - 1, chunk, chunk + 1, 3 * chunk + 5} with
chunk = M1_BOOTSTRAP_CHUNK = 1024, the events of one block-wide scan.  Confidences are multiples of 1 / 8: tie groups of hundreds of
events straddle thread, wave and chunk borders.  V in {0, 1, 16} with NaN entries and one column of NaN only.

Validity: where a comparison says 'equal where finite' the fixture must define the statistic: at most 5 % NaN per column is asserted
wherever both classes of cases can be drawn reliably (N >= 255, or the stratified draw from N >= 2).  The unstratified draw from 2 or
3 cases loses a class in 1/2 or 1/4 of the replicates by construction; there the finite share is asserted to be at least a third.
N = 1, the one-class / no-lesion tables and the all-NaN value column are the deliberately degenerate ones: NaN everywhere, asserted."""
import functools
import importlib
import math
import os

import numpy as np
import pytest
import torch

import bootstrap_ref as R
from oracle import m1_oracle as O
from util import C1_FILTERS, C1_STRIDES, PKG, build_m1, load_params_into, ops, rnd

pytestmark = pytest.mark.gpu
B, V, L = PKG.bootstrap, PKG.validation, PKG.hip.lib
T = importlib.import_module("prostatemr_3d-cad-cspca_amd.train_model")
CHUNK = L.M1_BOOTSTRAP_CHUNK
NB, SEED = 32, 1234
EVENTS = {1: 1, 2: 3, 3: 5, 255: CHUNK - 1, 256: CHUNK, 257: CHUNK + 1, 1000: 3 * CHUNK + 5, 16384: 40 * CHUNK + 7}
VALUES = {1: 1, 2: 0, 3: 1, 255: 1, 256: 0, 257: 16, 1000: 1, 16384: 16}


@functools.lru_cache(maxsize=None)
def _fixture(N, M, Vn):
    """(cases, table, host replicates unstratified / stratified, their multiplicities), computed once per shape."""
    cases = R.cases_with(N, M, SEED)
    t = B.pack(cases, values=R.value_columns(N, Vn, SEED) if Vn else None)
    assert (t["N"], t["M"], t["V"]) == (N, M, Vn)
    host = {s: B.replicates_host(t, NB, SEED, s) for s in (False, True)}
    W = {s: np.stack([B.draw_weights(t, b, SEED, s) for b in range(NB)]) for s in (False, True)}
    return cases, t, host, W


def _assert_valid(got, t, stratified, what):
    """The validity condition of the module docstring."""
    share = np.isnan(got).mean(axis=0)
    dead = [2 + len(t["fp_rates"]) + 15] if t["V"] == 16 else []            # the all-NaN value column
    live = [j for j in range(got.shape[1]) if j not in dead]
    assert (share[dead] == 1.0).all(), what
    if t["N"] == 1:
        assert share[0] == 1.0 and (share[1:5] == 0.0).all(), (what, share)
    elif t["N"] >= 255 or stratified:
        assert share[live].max() <= 0.05, (what, share)
    else:
        assert share[live].max() <= 2.0 / 3.0, (what, share)


@pytest.mark.parametrize("stratified", [False, True])
@pytest.mark.parametrize("N", sorted(EVENTS))
def test_kernel_equals_replicates_host(dev, N, stratified):
    cases, t, host, W = _fixture(N, EVENTS[N], VALUES[N])
    got = B.replicates(t, NB, SEED, stratified, device=dev)
    R.assert_rows(got, host[stratified], t, W[stratified], (N, stratified))
    _assert_valid(got, t, stratified, (N, stratified))


@pytest.mark.parametrize("M", [0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5])
def test_event_counts_around_the_chunk(dev, M):
    cases, t, host, W = _fixture(300, M, 0)
    got = B.replicates(t, NB, SEED, device=dev)
    R.assert_rows(got, host[False], t, W[False], ("M", M))
    _assert_valid(got, t, False, ("M", M))
    if M == 0:
        assert not got[:, 1:].any()                                         # lesions, all missed: AP and the sensitivities are 0


@pytest.mark.parametrize("mode,nan_cols", [("all_tp", []), ("all_fp", [0, 1, 2, 3, 4]), ("missed", []), ("one_class", [0])])
def test_degenerate_tables(dev, mode, nan_cols):
    cases = R.synthetic_cases(300, 7, mode=mode)
    t = B.pack(cases)
    host = B.replicates_host(t, NB, SEED)
    got = B.replicates(t, NB, SEED, device=dev)
    R.assert_rows(got, host, t, np.stack([B.draw_weights(t, b, SEED) for b in range(NB)]), mode)
    fine = [j for j in range(5) if j not in nan_cols]
    assert np.isnan(got[:, nan_cols]).all() and not np.isnan(got[:, fine]).any(), mode
    if mode == "all_tp":
        assert (got[:, 2:] == 1.0).all()
    if mode == "missed":
        assert t["M"] == 0 and not got[:, 1:].any() and (got[:, 0] == 0.5).all()


def test_weights_replace_the_draw(dev):
    cases, t, host, _ = _fixture(257, CHUNK + 1, 16)
    N = 257
    jack = np.ones((8, N), np.int32)
    jack[np.arange(8), [0, 1, 63, 64, 128, 255, 256, 100]] = 0
    one = np.zeros((2, N), np.int32)
    one[0, 5], one[1, 200] = 3, 65535
    for w in (jack, one):
        ref = B.replicates_host(t, len(w), weights=w)
        got = B.replicates(t, len(w), weights=w, device=dev)
        R.assert_rows(got, ref, t, w[:, t["case_perm"]], "weights")
    assert np.isnan(B.replicates(t, 2, weights=one, device=dev)[:, 0]).all()
    with pytest.raises(ValueError):
        B.replicates(t, 2, weights=np.full((2, N), 65536), device=dev)


def test_weights_at_the_cap_do_not_overflow(dev):
    """Every event on one case at weight 65535, and every one of 16384 cases at 65535: 2 * P_w * N_w is near 2^59 (past the 53 bits a
    double holds exactly: both sides round the same integers once), the TP / FP counts above 2^24 and 2^31 -- inside the 64 bits the
    kernel computes in."""
    g = np.random.default_rng(3)
    N, M = 257, CHUNK + 1
    res = [(1, float(g.integers(4, 9)) / 8, 0.5) if k % 3 == 0 else (0, float(g.integers(1, 8)) / 8, 0.0) for k in range(M)]
    cases = [{"label": i % 2 == 0, "lesion_results": res if i == 100 else [], "confidence": float(g.integers(0, 9)) / 8} for i in range(N)]
    t = B.pack(cases)
    w = np.ones((2, N), np.int32)
    w[0, 100], w[1, :] = 65535, 65535
    ref, got = B.replicates_host(t, 2, weights=w), B.replicates(t, 2, weights=w, device=dev)
    R.assert_rows(got, ref, t, w[:, t["case_perm"]], "cap")
    assert not np.isnan(got).any() and 65535 * (M // 3) > 2 ** 24
    cases, t, _, _ = _fixture(16384, EVENTS[16384], 16)
    w = np.full((1, 16384), 65535, np.int32)
    ref, got = B.replicates_host(t, 1, weights=w), B.replicates(t, 1, weights=w, device=dev)
    R.assert_rows(got, ref, t, w, "cap 16384")
    assert 2 * int(t["P"]) * 65535 * (16384 - int(t["P"])) * 65535 > 2 ** 58
    # all weights equal: the point estimate of the unweighted list, up to the one rounding of each integer above 2^53
    assert np.allclose(got[0, [0, 2, 3, 4]], B.metrics_of_weights(t, np.ones(16384, np.int64))[[0, 2, 3, 4]], rtol=2.0 ** -50, atol=0.0)


def _offset(t: torch.Tensor) -> torch.Tensor:
    """A copy of ``t`` that starts one element behind an allocation's start."""
    return torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)[1:].view(t.shape).copy_(t)


@pytest.mark.parametrize("N", [257, 16384])
def test_rows_repeat_bit_for_bit(dev, N):
    """Two runs, buffers that start one element off, a longer call (the prefix property) and a call with an ``out`` of its own."""
    cases, t, host, _ = _fixture(N, EVENTS[N], VALUES[N])
    td = B.to_device(t, dev)["dev"]
    off = {k: (_offset(v) if isinstance(v, torch.Tensor) else v) for k, v in td.items()}
    assert off["case_label"].data_ptr() % 2 == 1 and off["ev_case"].data_ptr() % 8 == 4 and off["values"].data_ptr() % 16 == 8
    with torch.no_grad():
        for strat in (False, True):
            a = ops.bootstrap_metrics(td, NB, SEED, strat)
            b = ops.bootstrap_metrics(td, NB, SEED, strat)
            c = ops.bootstrap_metrics(off, NB, SEED, strat)
            d = ops.bootstrap_metrics(td, 3 * NB + 1, SEED, strat)
            e = ops.bootstrap_metrics(td, NB, SEED, strat, out=torch.full((NB, a.shape[1]), 7.0, dtype=torch.float64, device=dev))
            bits = a.view(torch.int64)
            for other in (b, c, d[:NB], e):
                assert torch.equal(bits, other.view(torch.int64))
            assert not torch.equal(bits, ops.bootstrap_metrics(td, NB, SEED + 1, strat).view(torch.int64))
    assert tuple(a.shape) == (NB, len(B.columns(t))) and a.dtype == torch.float64


def test_capture_and_three_replays(dev):
    cases, t, host, _ = _fixture(1000, EVENTS[1000], 1)
    td = B.to_device(t, dev)["dev"]
    out = torch.empty((NB, len(B.columns(t))), dtype=torch.float64, device=dev)
    with torch.no_grad():
        eager = [ops.bootstrap_metrics(td, NB, SEED).clone() for _ in range(3)]
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            ops.bootstrap_metrics(td, NB, SEED, out=out)
        torch.cuda.current_stream().wait_stream(st)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(gr):
            ops.bootstrap_metrics(td, NB, SEED, out=out)
        hist = PKG.hip.graphs.assert_no_memset_nodes(gr)
        assert hist.get("kernel", 0) == 1 and not hist.get("memcpy", 0), hist
        gr.instantiate()
        for k in range(3):
            out.fill_(7.0)
            gr.replay()
            torch.cuda.synchronize()
            assert torch.equal(out.view(torch.int64), eager[k].view(torch.int64))


def test_ops_refuses_what_the_kernel_does_not_take(dev):
    cases, t, host, _ = _fixture(257, CHUNK + 1, 16)
    td = B.to_device(t, dev)["dev"]
    with pytest.raises(RuntimeError, match="no_grad"):
        ops.bootstrap_metrics(td, 4)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="M1_ERR_BAD_ARG"):
            ops.bootstrap_metrics(td, 0)
        with pytest.raises(RuntimeError, match="M1_ERR_BAD_ARG"):
            ops.bootstrap_metrics(td, 4, fp_rates=[0.5] * 9)
        with pytest.raises(RuntimeError, match="M1_ERR_UNSUPPORTED"):
            ops.bootstrap_metrics(B.to_device(_fixture(256, CHUNK, 0)[1], dev)["dev"], (1 << 20) + 1, fp_rates=())    # (16 MiB of out)
        with pytest.raises(RuntimeError, match="weights"):
            ops.bootstrap_metrics(td, 4, weights=torch.ones((4, 257), dtype=torch.int64, device=dev))
        with pytest.raises(RuntimeError, match="ev_tp"):
            ops.bootstrap_metrics(dict(td, ev_tp=td["ev_tp"][:-1]), 4)
    big = B.pack([{"label": i % 2, "lesion_results": [], "confidence": 0.0} for i in range(16385)])
    with pytest.raises(ValueError, match="16384"):
        B.replicates(big, 4, device=dev)


# ---- validate(bootstrap=...) on the tiny model of tests/test_validation.py ---------------------------------------------------------------
DIMS = (4, 32, 32)


def _model(dev, num_classes):
    cfg = O.M1Config(input_spatial_dims=DIMS, filters=C1_FILTERS, strides=C1_STRIDES, dense_skip=True, probabilistic=True,
                     prob_latent_dims=(3, 2, 1, 0), dropout_rate=0.5, dropout_mode="monte-carlo", num_classes=num_classes,
                     input_channels=3)
    m = build_m1(cfg, dev)
    load_params_into(m, O.fixture_params(cfg, seed=71))
    return m


def _lesion_batches(dev):
    rng = np.random.default_rng(72)
    out = []
    for s in range(2):
        xs, ys = zip(*[T.synthetic_case(rng, DIMS, 3, 2) for _ in range(2)])
        x, y = np.stack(xs), np.stack(ys)
        if s == 1:
            y[1, ..., 0], y[1, ..., 1] = 1.0, 0.0
        out.append(({"image": torch.from_numpy(x).to(dev)}, {"detection": torch.from_numpy(y).to(dev)}))
    return out


def _zonal_batches(dev):
    lab = np.zeros((2, 2, *DIMS), np.int64)
    lab[:, :, :, 8:20, 8:20] = 1
    lab[:, :, :, 20:28, 10:24] = 2
    lab[1, 1, :, 8:20, 8:20] = 0
    return [({"image": rnd((2, *DIMS, 3), 73 + s).to(dev)},
             {"detection": torch.from_numpy(np.stack([lab[s] == k for k in range(3)], axis=-1).astype(np.uint8)).to(dev)}) for s in range(2)]


def _same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


@pytest.mark.parametrize("train_obj", ["lesion", "zonal"])
def test_validate_appends_the_bootstrap_keys(dev, train_obj, monkeypatch):
    m = _model(dev, 2 if train_obj == "lesion" else 3)
    batches = _lesion_batches(dev) if train_obj == "lesion" else _zonal_batches(dev)
    alpha = (0.25, 0.75) if train_obj == "lesion" else (0.75, 0.25, 0.5)
    calls = []
    real = ops.bootstrap_metrics
    monkeypatch.setattr(ops, "bootstrap_metrics", lambda *a, **k: calls.append(a[1]) or real(*a, **k))
    m.eval()
    m.seed_dropout(81)
    base = V.validate(m, batches, 2, train_obj, n_draws=2, alpha=alpha)
    assert calls == []                                                       # off: not one call more than before
    m.seed_dropout(81)
    state = m.rng_state.clone()
    got = V.validate(m, batches, 2, train_obj, n_draws=2, alpha=alpha, bootstrap=32, bootstrap_seed=5, bootstrap_stratified=True)
    assert calls == [32] and torch.equal(m.rng_state, state)                 # one call; no trace
    assert list(got)[:len(base)] == list(base) and all(_same(got[k], base[k]) for k in base)
    if train_obj == "lesion":
        keys = ["val_auroc", "val_ap", "val_sens@0.5fp", "val_sens@1fp", "val_sens@2fp"]
        assert list(got)[len(base):] == ["val_ap"] + [k + s for k in keys for s in ("_lo", "_hi")]
    else:
        keys = [f"val_{n}_c{k}" for k in (1, 2) for n in ("dice", "hd95", "assd")]
        assert list(got)[len(base):] == [k + s for k in keys for s in ("_lo", "_hi")]
    n_finite = 0
    for k in keys:
        lo, p, hi = got[k + "_lo"], got[k], got[k + "_hi"]
        print(k, lo, p, hi)
        if all(map(math.isfinite, (lo, p, hi))):
            n_finite += 1
            assert lo <= p <= hi, (k, lo, p, hi)
    assert n_finite >= 2
    with pytest.raises(ValueError, match="bootstrap"):
        V.validate(m, batches, 2, train_obj, bootstrap=-1)


# ---- the trainer: the flag off is today's run, the flag on leaves no trace on training -------------------------------------------------
def test_trainer_flag_adds_columns_and_nothing_else(dev, tmp_path):
    counters = (PKG.unets.network_blocks._DropoutBase._next_id, PKG.unets.networks.M1Core._next_latent_id)
    before, out = [c[0] for c in counters], {}
    for name, extra in (("off", []), ("on", ["--VALIDATE_BOOTSTRAP", "16", "--VALIDATE_BOOTSTRAP_SEED", "3"])):
        counters[0][0], counters[1][0] = 1, 0                                # (process-wide construction counters key the streams)
        wd = str(tmp_path / name) + "/"
        args = ["--WEIGHTS_DIR", wd, "--METRICS_DIR", wd, "--NAME", "run", "--FOLDS", "0", "--UNET_FEATURE_CHANNELS", "8", "16", "32",
                "64", "128", "--UNET_PROBABILISTIC", "1", "--UNET_DENSE_SKIP", "1", "--SYNTHETIC_SAMPLES", "4", "--IMAGE_SPATIAL_DIMS",
                "4", "32", "32", "--BATCH_SIZE", "2", "--COMPUTE_DTYPE", "fp32", "--NUM_EPOCHS", "2", "--FOCAL_LOSS_ALPHA", "0.25", "0.75",
                "--VALIDATE", "1", "--VALIDATE_PER_N_EPOCHS", "1", "--VALIDATE_MIN_EPOCH", "1", "--UNET_PROBA_ITER", "2",
                "--SYNTHETIC_VALID_SAMPLES", "3"]
        (model, hist, _), = T.main(args + extra)
        out[name] = (model, open(os.path.join(wd + "run", "F1", "validation.csv")).read().splitlines())
    for c, b in zip(counters, before):
        c[0] = max(c[0], b)
    (m0, rows0), (m1, rows1) = out["off"], out["on"]
    o0, o1 = m0._compiled["optimizer"], m1._compiled["optimizer"]
    for name in ("m", "v", "vhat", "step_dev"):
        assert torch.equal(getattr(o0, name), getattr(o1, name)), name
    assert torch.equal(o0.flatp.flat, o1.flatp.flat) and torch.equal(m0.rng_state, m1.rng_state)
    head0, head1 = rows0[0].split(","), rows1[0].split(",")
    assert head0 == ["epoch", "val_focal", "val_dice", "val_hard_dice", "val_auroc", "val_sens@0.5fp", "val_sens@1fp", "val_sens@2fp",
                     "val_entropy", "val_entropy_fg", "val_cases"]            # today's columns
    assert head1[:len(head0)] == head0 and head1[len(head0)] == "val_ap" and len(head1) == len(head0) + 11
    assert [r.split(",")[:len(head0)] for r in rows1[1:]] == [r.split(",") for r in rows0[1:]] and len(rows1) == 3
