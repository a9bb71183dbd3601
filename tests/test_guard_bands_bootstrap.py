"""Guard bands (tests/guarded.py) around every buffer of the bootstrap kernel (csrc/bootstrap.hip: m1_bootstrap_metrics) at N = 257
cases and M = chunk + 1 events: one case and one event behind a full thread / chunk, so the last thread of a pass reads exactly one
item and every other lane's bounds test decides.  The case arrays of exactly N bytes / N int32, the event arrays of exactly M, the
values of exactly V * N doubles, the draw's permutation, the weights of exactly n_boot * N int32 and the output of exactly
n_boot * S doubles.  No byte outside a buffer is written; a load from a guard would show in the results -- 0xFF bytes are a positive
label, a group end, case index -1 (dropped), weight -1 (clamped to 0), a NaN value -- which are compared with
``bootstrap.replicates_host`` as tests/test_bootstrap.py compares them."""
import numpy as np
import pytest
import torch

import bootstrap_ref as R
from guarded import guarded
from util import PKG, ops

pytestmark = pytest.mark.gpu
B, L = PKG.bootstrap, PKG.hip.lib
N, M, NB, SEED = 257, L.M1_BOOTSTRAP_CHUNK + 1, 16, 99


@pytest.fixture
def g(dev, monkeypatch):
    with guarded(monkeypatch, dev) as g_:
        yield g_


@pytest.mark.parametrize("stratified", [False, True])
@pytest.mark.parametrize("with_weights", [False, True])
@pytest.mark.parametrize("Vn", [0, 3])
def test_bootstrap_metrics_under_guards(g, Vn, with_weights, stratified):
    cases = R.cases_with(N, M, SEED)
    t = B.pack(cases, values=R.value_columns(N, Vn, SEED) if Vn else None)
    assert (t["N"], t["M"], t["V"]) == (N, M, Vn)
    w = None
    if with_weights:
        w = np.random.default_rng(SEED).integers(0, 4, (NB, N)).astype(np.int32)
        w[0], w[1, :-1], w[1, -1] = 1, 0, 2                                  # the list itself; the last case alone
    ref = B.replicates_host(t, NB, SEED, stratified, weights=w)
    W = w[:, t["case_perm"]] if with_weights else np.stack([B.draw_weights(t, b, SEED, stratified) for b in range(NB)])
    names = ["case_label", "case_group_end", "case_lesions", "ev_case", "ev_tp", "ev_group_end", "case_rank", "strat_perm"]
    td = {k: g.put(torch.from_numpy(t[k])) for k in names}
    td["values"] = g.put(torch.from_numpy(np.ascontiguousarray(t["values"].T))) if Vn else None
    td["P"] = t["P"]
    wd = g.put(torch.from_numpy(np.ascontiguousarray(W.astype(np.int32)))) if with_weights else None
    with torch.no_grad():
        out = ops.bootstrap_metrics(td, NB, SEED, stratified, t["fp_rates"], wd)
    S = 5 + Vn
    assert g.count == 1 and out.numel() * out.element_size() == 8 * NB * S
    got = out.cpu().numpy()
    assert g.check() == len(names) + int(Vn > 0) + int(with_weights) + 1
    R.assert_rows(got, ref, t, W, (Vn, with_weights, stratified))
