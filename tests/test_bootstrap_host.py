"""The bootstrap on the host (no GPU): ``detection.average_precision`` against sklearn and by hand; ``bootstrap.replicates_host`` -- the
packed, weighted formulation the kernel evaluates -- against the explicit-resample oracle of tests/bootstrap_ref.py and against
sklearn's ``sample_weight`` forms; the draw against tests/philox_ref.py; the prefix property; stratified draws; intervals; paired
differences; the argument checks of the C entry, which all precede any launch.

Bounds.  AUROC and the sensitivities are one fp64 division of two integers below 2^53 on both sides: bit-equal.  AP: both sides add
the SAME fp64 terms (R_k - R_{k-1}) * P_k -- a zero-weight group or a group without a new TP adds exactly 0 -- in different orders, so
they differ by at most 4 * n * 2^-53 of the sum of the n terms, all non-negative (bootstrap_ref.assert_rows).  Means: the oracle adds
x_i w_i times, the restatement adds (double)w_i * x_i (one more rounding per case, 2^-53 relative): the same bound over n = N terms
relative to the sum of |terms|.  sklearn evaluates other expressions of the same quantities (weighted trapezoids and step sums over its own thresholds): 1e-12."""
import ctypes
import importlib
import math

import numpy as np
import pytest

import bootstrap_ref as R
import philox_ref
from util import PKG

B, D, V, L = PKG.bootstrap, PKG.detection, PKG.validation, PKG.hip.lib
T = importlib.import_module("prostatemr_3d-cad-cspca_amd.train_model")
try:
    import sklearn.metrics as skm
except ImportError:                                                         # (auroc's pin in test_detection_host.py is optional likewise)
    skm = None
needs_sklearn = pytest.mark.skipif(skm is None, reason="sklearn is not installed")
N, SEED, NB = 200, 1234, 60


def _flat(cases, drop_missed=False):
    rows = [(is_l, c) for case in cases for is_l, c, ov in case["lesion_results"] if not (drop_missed and is_l and ov == 0)]
    return np.array([r[0] for r in rows]), np.array([r[1] for r in rows], np.float64)


# ---- average_precision ------------------------------------------------------------------------------------------------------------------
@needs_sklearn
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_average_precision_equals_sklearn_without_missed_lesions(seed):
    cases = R.synthetic_cases(80, seed)
    for c in cases:                                                         # no missed lesion: every lesion is matched
        c["lesion_results"] = [r for r in c["lesion_results"] if not (r[0] and r[2] == 0)]
    y, s = _flat(cases)
    assert y.sum() > 20 and (1 - y).sum() > 20
    got, want = D.average_precision([c["lesion_results"] for c in cases]), skm.average_precision_score(y, s)
    print(got, want)
    assert abs(got - want) <= 1e-12


@needs_sklearn
@pytest.mark.parametrize("seed", [3, 4])
def test_average_precision_with_missed_lesions_scales_sklearn(seed):
    cases = R.synthetic_cases(80, seed)
    y_all, _ = _flat(cases)
    y, s = _flat(cases, drop_missed=True)
    n_l, m = int(y_all.sum()), int(y_all.sum() - y.sum())
    assert m > 3
    got, want = D.average_precision([c["lesion_results"] for c in cases]), (n_l - m) / n_l * skm.average_precision_score(y, s)
    print(got, want, n_l, m)
    assert abs(got - want) <= 1e-12


def test_average_precision_by_hand():
    assert math.isnan(D.average_precision([]))
    assert math.isnan(D.average_precision([[], [(0, 0.5, 0.0)]]))            # candidates, no lesion
    assert D.average_precision([[(1, 0.0, 0.0)], []]) == 0.0                  # no candidates: lesions, all missed
    assert D.average_precision([[(1, 0.0, 0.0), (1, 0.0, 0.0)], [(0, 0.25, 0.0)]]) == 0.0
    # one tie group holding a TP and an FP: one threshold, R = 1, P = 1 / 2
    assert D.average_precision([[(1, 0.5, 0.3), (0, 0.5, 0.0)]]) == 0.5
    # thresholds 0.9 (TP), 0.5 (FP), 0.25 (TP), one lesion missed: R = 1/3, 1/3, 2/3; P = 1, 1/2, 2/3
    got = D.average_precision([[(1, 0.9, 0.4), (0, 0.5, 0.0)], [(1, 0.25, 0.2), (1, 0.0, 0.0)]])
    assert abs(got - (1 / 3 * 1.0 + 0.0 * 0.5 + 1 / 3 * 2 / 3)) <= 2 ** -52


# ---- the shared fixture ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    cases = R.synthetic_cases(N, SEED)
    g = np.random.default_rng(SEED)
    vals = g.random((N, 3)) * 4.0
    vals[g.random((N, 3)) < 0.2] = np.nan
    out = {"cases": cases, "values": vals, "table": B.pack(cases, values=vals)}
    for strat in (False, True):
        out["host", strat] = B.replicates_host(out["table"], NB, SEED, strat)
        out["oracle", strat] = R.replicates(cases, NB, SEED, strat, values=vals)
    return out


def _drawn(table, n, seed, strat=False):
    return np.stack([B.draw_weights(table, b, seed, strat) for b in range(n)])


def test_replicates_host_equals_the_explicit_resample(fx):
    for strat in (False, True):
        R.assert_rows(fx["host", strat], fx["oracle", strat], fx["table"], _drawn(fx["table"], NB, SEED, strat), ("stratified", strat))
        assert np.isnan(fx["host", strat]).mean(axis=0).max() <= 0.05       # the validity condition: the fixture defines what is compared
    assert not np.array_equal(fx["host", False], fx["host", True])


@needs_sklearn
def test_replicates_host_equals_sklearn_sample_weight(fx):
    t, cases = fx["table"], fx["cases"]
    labels, scores = np.array([c["label"] for c in cases]), np.array([c["confidence"] for c in cases])
    for b in range(20):
        w = np.empty(N, np.int64)
        w[t["case_perm"]] = B.draw_weights(t, b, SEED)                        # multiplicities in the original order
        assert abs(fx["host", False][b, 0] - skm.roc_auc_score(labels, scores, sample_weight=w)) <= 1e-12
        rows = [(is_l, c, w[i]) for i, case in enumerate(cases) for is_l, c, ov in case["lesion_results"] if not (is_l and ov == 0)]
        y, s, sw = (np.array(v) for v in zip(*rows))
        lw = sum(w[i] * sum(1 for r in case["lesion_results"] if r[0]) for i, case in enumerate(cases))
        want = float(sw[y == 1].sum()) / lw * skm.average_precision_score(y, s, sample_weight=sw)
        assert abs(fx["host", False][b, 1] - want) <= 1e-12, (b, fx["host", False][b, 1], want)


def test_weights_replace_the_draw(fx):
    t, cases, vals = fx["table"], fx["cases"], fx["values"]
    jack = np.ones((5, N), np.int32)
    jack[np.arange(5), [0, 17, 60, 133, N - 1]] = 0
    one = np.zeros((2, N), np.int32)
    one[0, 3], one[1, 5] = 4, 1
    for w in (jack, one):
        got, ref = B.replicates_host(t, len(w), weights=w), R.replicates(cases, len(w), weights=w, values=vals)
        R.assert_rows(got, ref, t, w[:, t["case_perm"]], "weights")
    assert np.isnan(B.replicates_host(t, 2, weights=one)[:, 0]).all()         # one case: one class
    # the multiplicities of replicate b as weights give replicate b
    w = np.empty((3, N), np.int64)
    for b in range(3):
        w[b, t["case_perm"]] = B.draw_weights(t, b, SEED)
    assert np.array_equal(B.replicates_host(t, 3, weights=w), fx["host", False][:3], equal_nan=True)
    for bad in (np.ones((2, N + 1), np.int32), np.full((2, N), -1), np.full((2, N), 65536), np.ones((2, N))):
        with pytest.raises(ValueError):
            B.replicates_host(t, 2, weights=bad)


def test_degenerate_tables_are_nan_where_the_host_functions_are(fx):
    for mode, nan_cols, zero_cols in (("all_fp", [0, 1, 2, 3, 4], []), ("missed", [], [1, 2, 3, 4]), ("one_class", [0], []),
                                      ("all_tp", [], [])):
        cases = R.synthetic_cases(40, 7, mode=mode)
        t = B.pack(cases)
        got, ref = B.replicates_host(t, 12, 1), R.replicates(cases, 12, 1)
        R.assert_rows(got, ref, t, _drawn(t, 12, 1), mode)
        assert np.isnan(got[:, nan_cols]).all() and not got[:, zero_cols].any(), mode
        if mode == "all_tp":
            assert (np.abs(got[:, 1] - 1.0) <= 2.0 ** -50).all() and (got[:, 2:] == 1.0).all()
        if mode == "missed":
            assert t["M"] == 0 and (got[:, 0] == 0.5).all()                     # no event at all; every score ties


# ---- the draw ----------------------------------------------------------------------------------------------------------------------------
def test_the_draw_is_the_documented_philox_stream():
    assert B.STREAM_ID == R.STREAM_ID == L.M1_STREAM_BOOTSTRAP
    header = open(L.HEADER).read()
    assert "#define M1_STREAM_BOOTSTRAP 0x%Xull" % B.STREAM_ID in header
    for n, b, seed in ((1, 0, 0), (5, 3, 9), (257, 1000, 2 ** 63 + 5), (1000, (1 << 20) - 1, SEED)):
        assert B.draw_indices(n, b, seed).tolist() == R.draw(n, b, seed)
        w = philox_ref.words(seed, B.STREAM_ID, (b << 12) + np.arange((n + 3) // 4, dtype=np.uint64)).reshape(-1)[:n]
        assert B.draw_indices(n, b, seed).tolist() == [(int(x) * n) >> 32 for x in w]
    labels = [i % 3 == 0 for i in range(50)]
    pos = [i for i in range(50) if labels[i]]
    neg = [i for i in range(50) if not labels[i]]
    order = np.array(pos + neg)
    assert order[B.draw_indices(50, 4, 11, P=len(pos))].tolist() == R.draw(50, 4, 11, labels)


def test_prefix_property_and_seed(fx):
    t = fx["table"]
    assert np.array_equal(B.replicates_host(t, 10, SEED), fx["host", False][:10], equal_nan=True)
    assert not np.array_equal(B.replicates_host(t, 10, SEED + 1), fx["host", False][:10])


def test_stratified_draws_keep_the_class_counts(fx):
    t = fx["table"]
    lab = t["case_label"] != 0
    for b in range(NB):
        w = B.draw_weights(t, b, SEED, stratified=True)
        assert int(w[lab].sum()) == t["P"] and int(w[~lab].sum()) == N - t["P"]
    assert any(int(B.draw_weights(t, b, SEED)[lab].sum()) != t["P"] for b in range(NB))
    assert not np.isnan(fx["host", True][:, 0]).any()


def test_the_draw_names_cases_in_the_original_order(fx):
    """Two models on the same cases: other scores, another packed order, the same resampled cases."""
    cases = fx["cases"]
    other = [dict(c, confidence=1.0 - c["confidence"]) for c in cases]
    ta, tb = fx["table"], B.pack(other, values=fx["values"])
    assert not np.array_equal(ta["case_perm"], tb["case_perm"])
    for strat in (False, True):
        wa, wb = np.empty(N, np.int64), np.empty(N, np.int64)
        wa[ta["case_perm"]], wb[tb["case_perm"]] = B.draw_weights(ta, 3, SEED, strat), B.draw_weights(tb, 3, SEED, strat)
        assert np.array_equal(wa, wb)
    ra, rb = fx["host", False], B.replicates_host(tb, NB, SEED)
    assert np.allclose(ra[:, 5:], rb[:, 5:], rtol=1e-13, atol=0.0)           # the value means do not depend on the scores
    assert np.allclose(ra[:, 0], 1.0 - rb[:, 0], rtol=0.0, atol=2.0 ** -50)  # a reversed ranking: 1 - AUROC, on the same resamples


# ---- intervals ------------------------------------------------------------------------------------------------------------------------------
def test_interval_ignores_nan_replicates():
    reps = np.array([[1.0, np.nan], [2.0, np.nan], [np.nan, np.nan], [4.0, np.nan], [3.0, np.inf]])
    lo, hi, n = B.interval(reps, 0.5)
    assert n.tolist() == [4, 0] and math.isnan(lo[1]) and math.isnan(hi[1])
    assert (lo[0], hi[0]) == tuple(np.percentile([1.0, 2.0, 4.0, 3.0], [25.0, 75.0]))
    with pytest.raises(ValueError):
        B.interval(reps, 1.0)


def test_interval_brackets_the_point_estimate(fx):
    cases = fx["cases"]
    point = R.metrics([c["label"] for c in cases], [c["confidence"] for c in cases], [c["lesion_results"] for c in cases],
                      fx["values"], B.FP_RATES, list(range(N)))
    assert np.array_equal(B.metrics_of_weights(fx["table"], np.ones(N, np.int64))[[0, 2, 3, 4]], point[[0, 2, 3, 4]])
    lo, hi, n = B.interval(fx["host", False], 0.95)
    assert (n == NB).all() and (lo <= point).all() and (point <= hi).all(), (lo, point, hi)
    assert B.columns(fx["table"]) == ["auroc", "ap", "sens@0.5fp", "sens@1fp", "sens@2fp", "value0", "value1", "value2"]


def test_paired_difference(fx):
    a = fx["host", False]
    d = B.paired_difference(a, a.copy(), 0.95, tables=(fx["table"], fx["table"]))
    assert not d["lo"].any() and not d["hi"].any() and (d["n_valid"] == NB).all() and (d["share_a_le_b"] == 1.0).all()
    b = a.copy()
    b[:, 0] += 0.125
    b[0, 1] = np.nan
    d = B.paired_difference(a, b)
    assert d["lo"][0] == d["hi"][0] == -0.125 and d["share_a_le_b"][0] == 1.0 and d["n_valid"][1] == NB - 1
    with pytest.raises(ValueError):
        B.paired_difference(a, a[:-1])
    with pytest.raises(ValueError, match="same cases"):
        B.paired_difference(a, a, tables=(fx["table"], B.pack(fx["cases"][:-1])))


def test_pack_layout(fx):
    t, cases = fx["table"], fx["cases"]
    score = np.array([c["confidence"] for c in cases])[t["case_perm"]]
    assert (np.diff(score) >= 0).all() and t["case_group_end"][-1] == 1
    assert np.array_equal(t["case_group_end"][:-1] != 0, np.diff(score) != 0)
    assert t["case_label"].dtype == t["ev_tp"].dtype == t["ev_group_end"].dtype == np.uint8
    assert t["ev_case"].dtype == t["case_lesions"].dtype == t["strat_perm"].dtype == np.int32
    assert int(t["case_lesions"].sum()) == sum(1 for c in cases for r in c["lesion_results"] if r[0])
    assert t["M"] == sum(1 for c in cases for is_l, cf, ov in c["lesion_results"] if cf > 0 and (not is_l or ov > 0))
    assert sorted(t["strat_perm"].tolist()) == list(range(N)) and (t["case_label"][t["strat_perm"][:t["P"]]] == 1).all()
    z = B.pack([{"dice": [0.5, 0.25], "hd95": [1.0, float("nan")], "assd": [0.5, 2.0]}] * 3, "zonal")
    assert z["V"] == 6 and z["M"] == 0 and B.columns(z)[5:] == ["dice_c1", "hd95_c1", "assd_c1", "dice_c2", "hd95_c2", "assd_c2"]
    got = B.replicates_host(z, 4)
    assert np.isnan(got[:, :5]).all() and np.isnan(got[:, 9]).all() and (got[:, 5] == 0.5).all()
    with pytest.raises(ValueError):
        B.pack(cases, values=np.zeros((N, 17)))


# ---- the C entry and the flags ------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_rejected_without_a_gpu():
    lib = L.load()
    rates = (ctypes.c_double * 9)(*([0.5] * 9))
    buf = (ctypes.c_double * 64)()                                              # host memory: nothing is launched, nothing dereferenced
    p = ctypes.addressof(buf)

    def table(**kw):
        t = L.m1_bootstrap_table_t()
        for n in ("case_label", "case_group_end", "case_lesions", "ev_case", "ev_tp", "ev_group_end", "values"):
            setattr(t, n, p)
        t.N, t.M, t.V, t.P = 4, 4, 1, -1
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    def call(t, n_boot=4, n_rates=3, out=p):
        return lib.m1_bootstrap_metrics(None if t is None else ctypes.byref(t), n_boot, 0, None, rates, n_rates, out, None)
    bad, unsupported = -1, -2
    assert call(None) == bad
    assert call(table(N=0)) == bad and call(table(N=-1)) == bad
    assert call(table(), n_boot=0) == bad
    assert call(table(), n_rates=9) == bad and call(table(V=17)) == bad
    assert call(table(case_label=None)) == bad and call(table(ev_case=None)) == bad and call(table(values=None)) == bad
    assert call(table(), out=None) == bad and call(table(), out=p + 4) == bad and call(table(case_lesions=p + 2)) == bad
    assert call(table(P=5, draw_perm=p)) == bad
    assert call(table(), n_boot=(1 << 20) + 1) == unsupported
    assert call(table(N=16385)) == unsupported
    assert L.status_name(call(table(N=16385))) == "M1_ERR_UNSUPPORTED"
    assert (L.M1_BOOTSTRAP_MAX_CASES, L.M1_BOOTSTRAP_MAX_BOOT, L.M1_BOOTSTRAP_MAX_RATES, L.M1_BOOTSTRAP_MAX_VALUES) == (16384, 1 << 20, 8, 16)


def test_trainer_flags_and_validate_arguments():
    a = T.build_parser().parse_args([])
    assert (a.VALIDATE_BOOTSTRAP, a.VALIDATE_BOOTSTRAP_SEED, a.VALIDATE_BOOTSTRAP_STRATIFIED) == (0, 0, 0)
    assert T.validate_bootstrap(a) == {}
    b = T.build_parser().parse_args("--VALIDATE_BOOTSTRAP 1000 --VALIDATE_BOOTSTRAP_SEED 7 --VALIDATE_BOOTSTRAP_STRATIFIED 1".split())
    assert T.validate_bootstrap(b) == {"bootstrap": 1000, "bootstrap_seed": 7, "bootstrap_stratified": True}
    for n in ("-1", str((1 << 20) + 1)):
        with pytest.raises(ValueError, match="bootstrap"):
            T.validate_bootstrap(T.build_parser().parse_args(["--VALIDATE_BOOTSTRAP", n]))
    with pytest.raises(ValueError, match="bootstrap_level"):
        V.check_bootstrap(10, 1.5)


def test_summarise_bootstrap_keys_on_the_host(fx):
    got = V.summarise_bootstrap(fx["cases"], "lesion", 40, seed=SEED)
    keys = ["val_auroc", "val_ap", "val_sens@0.5fp", "val_sens@1fp", "val_sens@2fp"]
    assert list(got) == ["val_ap"] + [k + s for k in keys for s in ("_lo", "_hi")]
    assert got["val_ap"] == D.average_precision([c["lesion_results"] for c in fx["cases"]])
    assert got["val_ap_lo"] <= got["val_ap"] <= got["val_ap_hi"]
    zon = [{"dice": [0.5 + 0.01 * i], "hd95": [2.0 + i], "assd": [1.0]} for i in range(8)]
    gz = V.summarise_bootstrap(zon, "zonal", 40)
    assert list(gz) == [f"val_{k}_c1{s}" for k in ("dice", "hd95", "assd") for s in ("_lo", "_hi")]
    assert gz["val_assd_c1_lo"] == gz["val_assd_c1_hi"] == 1.0 and gz["val_dice_c1_lo"] < gz["val_dice_c1_hi"]
