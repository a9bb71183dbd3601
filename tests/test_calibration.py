"""The calibration kernel (csrc/calibrate.hip, ops.cal_score) against the per-voxel loop of tests/cal_ref.py on the small shapes and
against ``calibration.reliability_host`` (which tests/test_calibration_host.py pins to that loop) on the large one; never against
anything the kernel wrote itself.

Bounds.  Every slot of the record is an integer and must be EQUAL, with one exception: ``nll`` adds floor(-log(p) * 2^32) with the
device's fp64 log, which may differ from numpy's in the last place; such a difference moves a floor by at most one unit, so
|nll - reference| <= n_valid units of 2^-32 (derived, not fitted; the observed difference is printed).

Shapes.  V = 105 (odd: the scalar tail runs, and the cases after the first start off the grid of the wide loads), 256 and 257 (one
and one-plus-a-tail vector bodies), 20 * 160 * 160 once (250 blocks per case, and 2 under M1_EW_BLOCKS = 2: long grid-stride walks)."""
import functools
import importlib
import math

import numpy as np
import pytest
import torch

import cal_ref
from oracle import m1_oracle as O
from util import C1_FILTERS, C1_STRIDES, PKG, build_m1, load_params_into, ops

pytestmark = pytest.mark.gpu
CAL, VAL = PKG.calibration, PKG.validation
T = importlib.import_module("prostatemr_3d-cad-cspca_amd.train_model")
BINS = (1, 8, 15, 64)
FXU = 2.0 ** -32


@functools.lru_cache(maxsize=None)
def _case(B, V, K, content, mask, unc, bf16):
    return cal_ref.case(B, V, K, content, mask=mask, unc=unc, bf16=bf16)


@functools.lru_cache(maxsize=None)
def _loop(B, V, K, content, mask, unc, bf16, M):
    c = _case(B, V, K, content, mask, unc, bf16)
    return cal_ref.record(c["p"], c["label"], M, c["mask"], c["unc"], c["u_max"])


def _run(dev, c, M, bf16=False, out=None):
    p = torch.from_numpy(c["p"]).to(dev)
    if bf16:
        assert torch.equal(torch.nan_to_num(p.bfloat16().float()), torch.nan_to_num(p))       # the case holds bf16 values already
        p = p.bfloat16()
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)        # noqa: E731
    with torch.no_grad():
        return ops.cal_score(p, t(c["label"]), M, t(c["mask"]), t(c["unc"]), c["u_max"], out=out)


def _assert_records(got, ref, what):
    assert len(got) == len(ref)
    for b, (g, r) in enumerate(zip(got, ref)):
        assert cal_ref.same(r, g, skip=("nll",)) == [], (what, b)
        d = int(g["nll"]) - int(r["nll"])
        print(what, "case", b, "nll units: kernel - reference =", d, "of n_valid", r["n_valid"])
        assert abs(d) <= r["n_valid"], (what, b, d)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("B,V", [(1, 105), (3, 105), (1, 256), (3, 256), (1, 257), (3, 257)])
def test_kernel_equals_the_per_voxel_loop(dev, B, V, K, bf16):
    for mask, unc in ((False, False), (True, True)):
        c = _case(B, V, K, "random", mask, unc, bf16)
        for M in BINS:
            rec = _run(dev, c, M, bf16)
            assert tuple(rec.shape) == (B, 8 + 3 * M * (K + 2)) and rec.dtype == torch.int64 and rec.is_cuda
            got = ops.read_cal_records(rec, K, M)
            _assert_records(got, _loop(B, V, K, "random", mask, unc, bf16, M), (B, V, K, bf16, mask, unc, M))
            assert got[0]["n_invalid"] >= 1                                 # the NaN voxels of case 0
            if not unc:
                assert not any(g["unc_count"].any() or g["unc_u_sum"].any() or g["unc_errors"].any() for g in got)


@pytest.mark.parametrize("mask,unc", [(True, False), (False, True)])
def test_mask_alone_and_uncertainty_alone(dev, mask, unc):
    for K, V in ((2, 257), (3, 105)):
        c = _case(3, V, K, "random", mask, unc, False)
        got = ops.read_cal_records(_run(dev, c, 15), K, 15)
        _assert_records(got, _loop(3, V, K, "random", mask, unc, False, 15), (K, V, mask, unc))


def test_uncertainty_clamps(dev):
    """u = 0 and a negative u in bin 0 (the negative one adds 0 to the sum), exactly u_max and 3 u_max in the top bin, 0.3 in bin
    int(0.3 * 15 / ln 2) = 6: the expected slots are written out by hand."""
    um = math.log(2)
    u = np.array([[0.0, -0.5, um, 3 * um, 0.3, 0.3, 0.3, 0.3, 0.3]], np.float32)
    c = {"p": np.tile(np.array([0.875, 0.125], np.float32), (1, 9, 1)), "label": np.zeros((1, 9), np.uint8), "mask": None, "unc": u,
         "u_max": um}
    got, = ops.read_cal_records(_run(dev, c, 15), 2, 15)
    want = [0] * 15
    want[0], want[6], want[14] = 2, 5, 2
    assert got["unc_count"].tolist() == want and not got["unc_errors"].any() and got["n_valid"] == 9
    f = lambda v: int(math.floor(float(np.float32(v)) * 2 ** 32))           # noqa: E731
    assert int(got["unc_u_sum"][0]) == 0 and int(got["unc_u_sum"][14]) == f(um) + f(3 * um) and int(got["unc_u_sum"][6]) == 5 * f(0.3)


@pytest.mark.parametrize("content", ["onebin", "alternate", "masked", "ignored"])
@pytest.mark.parametrize("K", [2, 3])
def test_adversarial_contents(dev, content, K):
    """Every voxel in one bin (every lane of a wave on one LDS word: the run-length path), bins alternating voxel by voxel (a flush
    per voxel), a case that is masked out entirely, a case that is ignored entirely."""
    B, V = 3, 257
    for M in (15, 64):
        c = _case(B, V, K, content, content == "masked", True, False)
        got = ops.read_cal_records(_run(dev, c, M), K, M)
        _assert_records(got, _loop(B, V, K, content, content == "masked", True, False, M), (content, K, M))
        if content == "onebin":
            # (one voxel of every case carries the other label; the NaN uncertainty takes one voxel of the last case out)
            assert all(g["top_count"][M - 1] == g["n_valid"] >= V - 1 and g["top_correct"][M - 1] == g["n_valid"] - 1 for g in got)
        if content == "alternate":
            assert all(np.count_nonzero(g["cls_count"][0]) == 2 for g in got)
        if content == "masked":
            assert got[0]["n_valid"] == got[0]["n_invalid"] == got[0]["n_ignored"] == 0 and not got[0]["cls_count"].any()
        if content == "ignored":
            assert got[B - 1]["n_valid"] == 0 and got[B - 1]["n_ignored"] > 0 and not got[B - 1]["top_count"].any()


@functools.lru_cache(maxsize=None)
def _large():
    """(2, 20*160*160) voxels, K = 2: case 0 a detection map (background at conf ~ 1 with a few blobs of graded confidence), case 1
    every voxel p = (1, 0); a mask, an entropy map, NaN at the first and the last voxel; and its record by reliability_host."""
    V = 20 * 160 * 160
    g = np.random.default_rng(5)
    p1 = np.full((2, V), 1e-4, np.float32)
    p1[0] += (g.random(V) < 0.004) * g.random(V).astype(np.float32) * np.float32(0.98)
    p1[1] = 0
    p = np.stack([np.float32(1) - p1, p1], axis=-1)
    label = (g.random((2, V)) < 0.003).astype(np.uint8)
    label[0, ::4099] = 255
    mask = (g.random((2, V)) < 0.95).astype(np.uint8)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = -np.where(p > 0, p * np.log(p), 0).sum(-1).astype(np.float32)
    p[0, 0, 0] = p[0, V - 1, 1] = np.nan
    c = {"p": p, "label": label, "mask": mask, "unc": u, "u_max": math.log(2)}
    return c, CAL.reliability_host(p, label, 15, mask, u, c["u_max"])


def test_many_blocks_per_case_and_long_grid_stride_walks(dev):
    c, ref = _large()
    a = _run(dev, c, 15)
    with ops.config(M1_EW_BLOCKS=2):
        b = _run(dev, c, 15)
    assert torch.equal(a, b)                                               # integers: the grid does not show in the record
    got = ops.read_cal_records(a, 2, 15)
    _assert_records(got, ref, "20x160x160")
    assert got[0]["n_invalid"] >= 1 and got[0]["n_ignored"] > 0 and got[1]["top_count"][14] == got[1]["n_valid"] > 400_000


def test_records_repeat_bit_for_bit(dev):
    """Two calls; a call on buffers that start 4 bytes (p, unc) and 1 byte (label, mask) off the grid of the wide loads."""
    for K, V in ((2, 256), (3, 257), (4, 105)):
        c = _case(3, V, K, "random", True, True, False)
        a, b = _run(dev, c, 15), _run(dev, c, 15)
        ts = [torch.from_numpy(c[k]).to(dev) for k in ("p", "label", "mask", "unc")]
        off = [torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)[1:].view(t.shape).copy_(t) for t in ts]
        assert off[0].data_ptr() % 16 == 4 and off[1].data_ptr() % 4 == 1 and off[3].data_ptr() % 16 == 4
        with torch.no_grad():
            d = ops.cal_score(off[0], off[1], 15, off[2], off[3], c["u_max"])
            e = ops.cal_score(off[0].bfloat16().float(), off[1], 15, off[2], off[3], c["u_max"])
            f = ops.cal_score(off[0].bfloat16(), off[1], 15, off[2], off[3], c["u_max"])
        assert torch.equal(a, b) and torch.equal(a, d) and torch.equal(e, f)


def test_captured_call_replays_like_eager_without_a_memset_node(dev):
    """Captured once on static buffers (after a warm-up on a side stream); three replays on three different inputs leave the bits of
    three eager calls -- the zero fill is part of the graph, so nothing accumulates from replay to replay -- and the graph holds no
    memset node."""
    B, V, K, M = 3, 257, 3, 15
    cs = [cal_ref.case(B, V, K, "random", mask=True, unc=True, seed=s) for s in (1, 2, 3)]
    dv = lambda c: [torch.from_numpy(c[k]).to(dev) for k in ("p", "label", "mask", "unc")]       # noqa: E731
    eager = [_run(dev, c, M).clone() for c in cs]
    assert not torch.equal(eager[0], eager[1])
    st = dv(cs[0])
    out = torch.empty((B, ops.cal_record_slots(K, M)), dtype=torch.int64, device=dev)
    call = lambda: ops.cal_score(st[0], st[1], M, st[2], st[3], cs[0]["u_max"], out=out)          # noqa: E731
    with torch.no_grad():
        s_ = torch.cuda.Stream()
        s_.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s_):
            call()
        torch.cuda.current_stream().wait_stream(s_)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(gr):
            call()
        torch.cuda.synchronize()
        hist = PKG.hip.graphs.assert_no_memset_nodes(gr)
        assert hist.get("memset", 0) == 0 and hist.get("kernel", 0) >= 2, hist
        for c, want in zip(cs, eager):
            for dst, src in zip(st, dv(c)):
                dst.copy_(src)
            gr.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want)
    del gr


def test_bad_arguments_are_rejected(dev):
    p = torch.full((2, 3, 5, 7, 2), 0.5, device=dev)
    y = torch.zeros((2, 3, 5, 7), dtype=torch.uint8, device=dev)
    u = torch.zeros((2, 3, 5, 7), device=dev)
    slots = ops.cal_record_slots(2, 15)
    with pytest.raises(RuntimeError, match="no_grad"):
        ops.cal_score(p, y, 15)
    with torch.no_grad():
        for kw, msg in ((dict(bins=0), "bins"), (dict(bins=65), "bins"), (dict(p=p.double()), "fp32 or bf16"),
                        (dict(p=torch.full((2, 3, 5, 7, 5), 0.2, device=dev)), "K must be"), (dict(label=y.int()), "label must be uint8"),
                        (dict(label=y[:1].contiguous()), "label must be uint8"), (dict(mask=y.float()), "mask must be uint8"),
                        (dict(unc=u.double(), u_max=1.0), "unc must be fp32"), (dict(unc=u[:, :2].contiguous(), u_max=1.0), "unc must be"),
                        (dict(unc=u), "u_max"),
                        (dict(out=torch.empty((2, slots + 1), dtype=torch.int64, device=dev)), "out must be"),
                        (dict(out=torch.empty((2, slots), dtype=torch.float64, device=dev)), "out must be"),
                        (dict(p=p.cpu()), "GPU")):
            args = dict(p=p, label=y, bins=15, mask=None, unc=None, u_max=None, out=None)
            args.update(kw)
            with pytest.raises(RuntimeError, match=msg):
                ops.cal_score(**args)
        for bad in (0.0, -1.0, float("inf"), float("nan")):                 # calibration.u_scale, the one definition: ValueError
            with pytest.raises(ValueError, match="u_max"):
                ops.cal_score(p, y, 15, None, u, bad)
            with pytest.raises(ValueError, match="u_max"):
                CAL.reliability(p, y, 15, None, u, bad)
        with pytest.raises(ValueError, match="bins"):                       # reliability(): the exception of the host path on both
            CAL.reliability(p, y, 65)
        odd = torch.empty(4 * slots + 1, dtype=torch.int32, device=dev)[1:]
        assert odd.data_ptr() % 8 == 4
        lib = PKG.hip.lib.load()                                           # a record off its 8-byte grid: refused by the entry point
        assert lib.m1_cal_score(p.data_ptr(), 0, y.data_ptr(), None, None, 0.0, 2, 105, 2, 15, odd.data_ptr(), None) == -1
        torch.cuda.synchronize()


# ---- validate(..., calibration=True) against the pieces composed by hand ----------------------------------------------------------------
DIMS = (4, 32, 32)
ALPHA = (0.25, 0.75)


def _model(dev):
    cfg = O.M1Config(input_spatial_dims=DIMS, filters=C1_FILTERS, strides=C1_STRIDES, dense_skip=True, probabilistic=True,
                     prob_latent_dims=(3, 2, 1, 0), dropout_rate=0.5, dropout_mode="monte-carlo", num_classes=2, input_channels=3)
    m = build_m1(cfg, dev)
    load_params_into(m, O.fixture_params(cfg, seed=71))
    return m


def _batches(dev):
    rng = np.random.default_rng(72)
    out = []
    for s in range(2):
        xs, ys = zip(*[T.synthetic_case(rng, DIMS, 3, 2) for _ in range(2)])
        out.append(({"image": torch.from_numpy(np.stack(xs)).to(dev)}, {"detection": torch.from_numpy(np.stack(ys)).to(dev)}))
    return out


def _same(a, b):
    return (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b)) or a == b


@pytest.mark.parametrize("n_draws", [1, 4])
def test_validate_with_calibration_equals_the_pieces_composed_by_hand(dev, n_draws):
    m, batches = _model(dev), _batches(dev)
    today = ["val_focal", "val_dice", "val_hard_dice", "val_auroc", "val_sens@0.5fp", "val_sens@1fp", "val_sens@2fp", "val_entropy",
             "val_entropy_fg", "val_cases"]
    extra = ["val_ece", "val_mce", "val_brier", "val_nll", "val_ece_c1", "val_unc_auroc", "val_err@refer10", "val_err@refer20"]
    m.train(True)
    m.seed_dropout(91)
    ops.step_advance(None, m.rng_state)
    state = m.rng_state.clone()
    off = VAL.validate(m, batches, 2, "lesion", n_draws=n_draws, alpha=ALPHA)
    assert torch.equal(m.rng_state, state) and m.training is True
    on = VAL.validate(m, batches, 2, "lesion", n_draws=n_draws, alpha=ALPHA, calibration=True, bins=15)
    assert torch.equal(m.rng_state, state) and m.training is True           # no trace
    assert list(off) == today and list(on) == today + extra
    for k in today:
        assert _same(on[k], off[k]), (k, on[k], off[k])
    dm = m.get_detect_model()
    m.eval()
    recs = []
    with torch.no_grad():
        for bx, by in batches:
            if n_draws == 1:
                mean, ent = dm.predict(bx), None
            else:
                o = dm.predict_mc(bx, n_draws)
                mean, ent = o["mean"], o["entropy"].cpu().numpy()
            label = by["detection"].argmax(dim=-1).to(torch.uint8).cpu().numpy()
            recs += CAL.reliability_host(mean.float().cpu().numpy(), label, 15, uncertainty=ent, u_max=math.log(2))
    m.train(True)
    rec = CAL.merge(recs)
    assert rec["n_valid"] == 4 * DIMS[0] * DIMS[1] * DIMS[2] and rec["n_invalid"] == rec["n_ignored"] == 0
    print("n_draws", n_draws, {k: on[k] for k in extra})
    assert on["val_ece"] == CAL.ece(rec) and on["val_mce"] == CAL.mce(rec) and on["val_brier"] == CAL.brier(rec)["total"]
    assert on["val_ece_c1"] == CAL.classwise_ece(rec, (1,))
    print("val_nll", on["val_nll"], CAL.nll(rec), abs(on["val_nll"] - CAL.nll(rec)))
    assert abs(on["val_nll"] - CAL.nll(rec)) <= FXU                          # at most one unit per voxel, divided by the voxels
    cur = CAL.referral_curve(rec)
    if n_draws == 1:
        assert all(math.isnan(on[k]) for k in ("val_unc_auroc", "val_err@refer10", "val_err@refer20"))
    else:
        assert _same(on["val_unc_auroc"], CAL.uncertainty_auroc(rec))
        assert _same(on["val_err@refer10"], CAL.error_at_referral(cur, 0.1)) and _same(on["val_err@refer20"], CAL.error_at_referral(cur, 0.2))
    for name in ("mutual_info", "expected_entropy"):
        if n_draws > 1:
            before = m.rng_state.clone()                                    # (the draws composed by hand above have moved the stream)
            other = VAL.validate(m, batches, 2, "lesion", n_draws=n_draws, alpha=ALPHA, calibration=True, calibration_uncertainty=name)
            assert torch.equal(m.rng_state, before) and m.training is True and list(other) == today + extra
            assert 0.0 <= other["val_ece"] <= 1.0 and (math.isnan(other["val_unc_auroc"]) or 0.0 <= other["val_unc_auroc"] <= 1.0)
    with pytest.raises(ValueError, match="calibration_uncertainty"):
        VAL.validate(m, batches, 2, "lesion", calibration=True, calibration_uncertainty="variance")


def test_reliability_takes_device_tensors_through_the_kernel(dev):
    c = _case(3, 257, 3, "random", True, True, False)
    t = lambda a: torch.from_numpy(a).to(dev)                               # noqa: E731
    got = CAL.reliability(t(c["p"]).view(3, 257, 1, 1, 3), t(c["label"]).view(3, 257, 1, 1), 15, t(c["mask"]).view(3, 257, 1, 1),
                          t(c["unc"]).view(3, 257, 1, 1))                   # u_max: ln 3 by default
    _assert_records(got, _loop(3, 257, 3, "random", True, True, False, 15), "reliability")
    host = CAL.reliability(c["p"], c["label"], 15, c["mask"], c["unc"])
    assert all(cal_ref.same(a, b) == [] for a, b in zip(host, _loop(3, 257, 3, "random", True, True, False, 15)))
