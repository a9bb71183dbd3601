"""No kernel reads or writes outside its buffers: the operations of the C ABI once more, at the small shapes where their edge logic
is live, with every tensor they touch between two 64 KiB guard bands (tests/guarded.py).  Every case asserts

  * parity with the fp64 reference under the bound the existing test of that operation uses (a NaN loaded from a guard fails it),
  * that no guard byte changed (``g.check()``),
  * that the helper saw the call's allocations (``g.count > 0``: a route it does not intercept must fail, not pass vacuously),
  * where the existing test pins the kernel, the same kernel (a guarded allocation must not move a case to the fallback).

Parameter gradients are taken twice: into fresh tensors, and accumulated into a guarded flat sink laid out like the optimiser's flat
gradient buffer -- [sink | neighbour | sink | neighbour ...], every neighbour standing for the next parameter's gradient, which must
come back bit-identical."""
import numpy as np
import pytest
import torch

import util
from guarded import guarded
from util import PKG, ops, rel_err, rnd, assert_conv_close, ref_conv_with_mag, ref_member_amag
from test_hip_ops import (TOL, T3F_CASES, T3S2_CASES, CT3_CASES, CT3_LOW, HALO_CLS_CASES, THIN_FWD_CASES, _TF_PARAMS,
                          _TF_EXPECT, _T3F_EXPECT, _T3, _FUZZ_LIFT, _fuzz_cases, _wgrad_kernels)
from test_ops_at_scale import lib_nchunks, red_nchunks

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture
def g(dev, monkeypatch):
    ops.invalidate_panels()
    with guarded(monkeypatch, dev) as gd:
        yield gd
    ops.invalidate_panels()


def _done(g):
    """The two assertions every case ends a launch sequence with: the helper saw allocations, and no guard byte changed."""
    assert g.count > 0, "no allocation of this call went through the guarded allocator"
    return g.check()


def _q(t, dtype):
    """``t`` as the kernels will read it in ``dtype`` (values exact in that type), fp32 on the host."""
    return t.to(dtype).float()


def _ref_grads(fn, inputs, dys):
    """fp64 outputs (a tuple) and autograd gradients of ``fn`` for the upstream gradients ``dys``."""
    ins = [t.detach().double().requires_grad_(True) for t in inputs]
    ys = fn(*ins)
    ys = ys if isinstance(ys, (tuple, list)) else (ys,)
    torch.autograd.backward(list(ys), [d.double() for d in dys])
    return [y.detach() for y in ys], [t.grad for t in ins]


class Sinks:
    """One guarded flat fp32 buffer of known values laid out [sink(p0) | gap | sink(p1) | gap | ...]; ``p._m1_gsink`` of every
    parameter is its view, as optim.FlatParams binds them (no alignment between parameters: the gap is 37 floats)."""
    GAP = 37

    def __init__(self, g, params, seed=77):
        params = [p for p in params if p is not None]
        self.spans, off = [], 0
        for p in params:
            self.spans.append((off, p.numel(), tuple(p.shape)))
            off += p.numel() + self.GAP
        self.init = rnd((off,), seed)
        self.flat = g.put(self.init)
        for p, (o, n, shp) in zip(params, self.spans):
            p._m1_gsink = self.flat[o:o + n].view(shp)

    def start(self, i):
        o, n, shp = self.spans[i]
        return self.init[o:o + n].view(shp).double()

    def got(self, i):
        o, n, shp = self.spans[i]
        return self.flat[o:o + n].view(shp).detach().cpu()

    def assert_neighbours_untouched(self, what=""):
        flat = self.flat.detach().cpu()
        for o, n, _ in self.spans:
            a, b = flat[o + n:o + n + self.GAP], self.init[o + n:o + n + self.GAP]
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (what, "the sink behind offset", o + n, "changed")


# =================================================================================================================================
# 1. the helper itself (torch only; every access stays inside the helper's own base buffer)
# =================================================================================================================================
def _elem_at(t, k):
    """The one-element view ``k`` elements from the start of ``t`` (may lie outside ``t``, inside its base buffer)."""
    return t.as_strided((1,), (1,), t.storage_offset() + k)


def test_helper_sees_one_element_past_the_end(g, dev):
    t = torch.empty((3, 5), dtype=torch.float32, device=dev)
    assert g.count == 1 and t.data_ptr() % 512 == 0
    _elem_at(t, t.numel()).fill_(1.0)
    with pytest.raises(AssertionError, match=r"offset \+0 from its end") as e:
        g.check()
    assert "(3, 5)" in str(e.value) and "torch.float32" in str(e.value) and "test_guard_bands.py" in str(e.value)
    assert g.count == 0 and g.check() == 0                       # reported once, then dropped


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.uint8])
def test_helper_sees_one_element_before_the_start(g, dev, dtype):
    t = torch.zeros(7, dtype=dtype, device=dev)
    _elem_at(t, -1).fill_(1)
    with pytest.raises(AssertionError, match=rf"offset -{t.element_size()} from its start"):
        g.check()


def test_helper_read_past_the_end_is_nan(g, dev):
    for make in (torch.empty, torch.zeros):
        t = make(11, dtype=torch.bfloat16, device=dev)
        t.fill_(1.0)
        assert float(t.sum()) == 11.0
        assert torch.isnan(t.as_strided((12,), (1,), t.storage_offset()).float().sum())
        assert torch.isnan(t.as_strided((12,), (1,), t.storage_offset() - 1).float().sum())
    assert g.check() == 2


def test_helper_interior_patterns_untouched_allocations_and_host_tensors(g, dev):
    e = torch.empty((2, 3), dtype=torch.float32, device=dev)
    z = torch.zeros_like(e)
    el = torch.empty_like(e, dtype=torch.bfloat16)
    i = torch.empty(5, dtype=torch.int32, device="cuda")
    p = g.put(rnd((4, 3), 1), torch.bfloat16)
    assert torch.isnan(e).all() and torch.isnan(el).all() and el.dtype == torch.bfloat16 and bool((z == 0).all()) and bool((i == -1).all())
    assert torch.equal(p.cpu(), rnd((4, 3), 1).bfloat16())
    assert g.count == 4                                          # (what put() places is checked, not counted)
    h = [torch.empty(4), torch.zeros((2, 2)), torch.empty_like(torch.ones(3)), torch.zeros_like(torch.ones(3)), torch.empty(3, device="cpu")]
    assert g.count == 4 and not any(t.is_cuda for t in h)        # CPU allocations are not intercepted
    for t in (e, z, el, i, p):                                   # the last byte abuts the back guard; the start is 512-byte aligned
        assert t.data_ptr() % 512 == 0 and t.is_contiguous()
    assert g.check() == 5 and g.count == 0


# =================================================================================================================================
# 2. convolutions
# =================================================================================================================================
EW = "assert_conv_close"


def _close(got, ref, mag, dtype, what, bound, key, acc=False, amag=None):
    if bound == EW:
        assert_conv_close(got.cpu(), ref, mag, dtype, what, acc=acc, amag=amag)
    else:
        e = rel_err(got, ref)
        print(f"{what}: rel_err {e:.3g} (limit {bound[key]:.3g})")
        assert e < bound[key] and bool(torch.isfinite(got).all()), (what, e, bound[key])


def _conv_case(g, transposed, k, s, cins, cout, dims, dtype, cfgs, bound, stats, seed, tag):
    """One conv configuration under the guards: forward, the data gradient of every concat member, weight and bias gradients, once
    into fresh tensors and once accumulated into a flat sink, for every (switches, expectation on the kernel log) of ``cfgs``.
    Returns the kernel base names seen."""
    bf = dtype == BF16
    xs = [_q(rnd((*dims, c), seed + j), dtype) for j, c in enumerate(cins)]
    cin = sum(cins)
    sc = 1.0 / (cin * k[0] * k[1] * k[2]) ** 0.5
    w = rnd((*k, cout, cin) if transposed else (*k, cin, cout), seed + 50, sc); b = rnd((cout,), seed + 51)
    w = _q(w, dtype)                                          # (the kernels read the weights in the activation type)
    xcat = torch.cat(xs, -1)
    osz = [n * st if transposed else -(-n // st) for n, st in zip(dims[1:], s)]
    dy = _q(rnd((dims[0], *osz, cout), seed + 52), dtype)
    ref, mg = ref_conv_with_mag(xcat, w, b, s, dy, transposed)
    am = ref_member_amag(xs, w, b, s, transposed) if bf and len(xs) > 1 else None
    seen = set()
    for cfg, expect in cfgs:
        for sink in (False, True):
            what = f"{tag} cfg={cfg} sink={sink}"
            ops.invalidate_panels()
            xd = [g.put(x, dtype).requires_grad_(True) for x in xs]
            wd, bd = g.put(w).requires_grad_(True), g.put(b).requires_grad_(True)
            sk = Sinks(g, [wd, bd]) if sink else None
            with ops.config(**cfg), ops.kernel_log() as kl:
                if transposed:
                    y, st = ops.conv3d_transpose_same(xd, wd, bd, k, s), None
                elif stats:
                    y, st = ops.conv3d_same(xd, wd, bd, k, s, stats=True)
                else:
                    y, st = ops.conv3d_same(xd, wd, bd, k, s), None
                y.backward(g.put(dy, dtype))
                ops.flush_deferred()                          # (sink mode: the queued weight gradient and its folds)
                torch.cuda.synchronize()
            _done(g)
            seen.update(n.split(":")[0] for n in kl.names)
            what += f" kernels={sorted(set(kl.names))}"
            convs = [n for n in kl.names if not (n.startswith("wgrad_") or n == "conv_wgrad_direct")]
            if expect is not None:
                expect(kl, sink)
            if sink:                                          # forward and data gradient: the kernels of the fresh run
                assert convs == fresh_convs, (what, fresh_convs)
            fresh_convs = convs
            assert tuple(y.shape) == tuple(ref["y"].shape), what
            _close(y, ref["y"], mg["y"], dtype, what + " y", bound, "y", amag=am)
            off = 0
            for x in xd:
                c = x.shape[-1]
                _close(x.grad, ref["dx"][..., off:off + c], mg["dx"][..., off:off + c], dtype, what + f" dx[{off}]", bound, "dx")
                off += c
            if sink:
                assert wd.grad is None and bd.grad is None, what
                _close(sk.got(0), sk.start(0) + ref["dw"], mg["dw"] + sk.start(0).abs(), F32, what + " dW (sink)", bound, "dw", acc=True)
                _close(sk.got(1), sk.start(1) + ref["db"], mg["db"] + sk.start(1).abs(), F32, what + " db (sink)", bound, "db", acc=True)
                sk.assert_neighbours_untouched(what)
            else:
                _close(wd.grad, ref["dw"], mg["dw"], F32, what + " dW", bound, "dw")
                _close(bd.grad, ref["db"], mg["db"], F32, what + " db", bound, "db")
            if st is not None:
                yf = y.detach().float()
                mean = yf.mean(dim=(1, 2, 3)); var = yf.var(dim=(1, 2, 3), unbiased=False)
                assert float((st[..., 0] - mean).abs().max()) < 1e-4 * (1.0 + float(mean.abs().max())), (what, "mean")
                assert rel_err(st[..., 1], 1.0 / torch.sqrt(var + 1e-3)) < 1e-3, (what, "rstd")
    ops.invalidate_panels()
    return seen


@pytest.mark.parametrize("chunk", range(10))
def test_conv_fuzz_under_guards(g, chunk):
    """The 300 configurations of test_conv_fuzz_against_oracle, each with the size floors of the special kernels lifted AND not."""
    seen = set()
    for (i, transposed, k, s, cins, cout, dims, dtype, _lifted) in _fuzz_cases(300, seed=20251003)[chunk * 30:(chunk + 1) * 30]:
        tag = f"case {i}: T={transposed} k={k} s={s} cins={cins} cout={cout} dims={dims} {dtype}"
        seen |= _conv_case(g, transposed, k, s, cins, cout, dims, dtype, [(_FUZZ_LIFT, None), ({}, None)], EW, True, 1000 + 7 * i, tag)
    assert seen, "no kernel was logged"


_TF_TOL = dict(y=TOL[BF16], dx=TOL[BF16], dw=1e-4, db=1e-4)       # the limits of test_tap_fused_wgrad


@pytest.mark.parametrize("idx", range(len(_TF_PARAMS)))
def test_tap_fused_wgrad_under_guards(g, idx):
    _tf_case(g, idx)


def _tf_case(g, idx, tag=""):
    ((dims, cins, cout, k, s, transposed), t3_floor), expect = _TF_PARAMS[idx], _TF_EXPECT[idx]

    def same_kernels(kl, sink):
        if sink:          # (queued, fold deferred: the weight-gradient kernel is pinned on the fresh run; _conv_case pins forward and dgrad)
            return
        assert _wgrad_kernels(kl) == expect, (kl.names, expect)
        if expect == _T3 and s[1] == 2:
            assert any(n.startswith("wgrad_t3:s2:") for n in kl.names), kl.names
    _conv_case(g, transposed, k, s, cins, cout, dims, BF16, [(dict(M1_T3_MIN_BLOCKS=t3_floor), same_kernels)], _TF_TOL, not transposed, 40,
               f"TF[{idx}]{tag}")


_T3F_TOL = dict(y=TOL[F32], dx=TOL[F32], dw=1e-4, db=1e-4)        # the limits of test_t3_fp32_wgrad / test_t3s_fp32_strided_wgrad


@pytest.mark.parametrize("idx", range(len(T3F_CASES)))
def test_t3_fp32_wgrad_under_guards(g, idx):
    _t3f_case(g, idx)


def _t3f_case(g, idx, tag=""):
    dims, cins, cout, k = T3F_CASES[idx]

    def same_kernels(kl, sink):
        if sink:          # (queued, fold deferred: the weight-gradient kernel is pinned on the fresh run; _conv_case pins forward and dgrad)
            return
        assert _wgrad_kernels(kl) == {_T3F_EXPECT[idx]}, (kl.names, _T3F_EXPECT[idx])
    _conv_case(g, False, k, (1, 1, 1), cins, cout, dims, F32, [({}, same_kernels)], _T3F_TOL, False, 50, f"T3F[{idx}]{tag}")


@pytest.mark.parametrize("idx", range(len(T3S2_CASES)))
def test_t3s_fp32_strided_wgrad_under_guards(g, idx):
    dims, cins, cout, k, s, transposed = T3S2_CASES[idx]

    def same_kernels(kl, sink):
        if sink:          # (queued, fold deferred: the weight-gradient kernel is pinned on the fresh run; _conv_case pins forward and dgrad)
            return
        assert _wgrad_kernels(kl) == {"wgrad_t3s" if idx < 4 else "wgrad_mfma"}, kl.names
    _conv_case(g, transposed, k, s, cins, cout, dims, F32, [({}, same_kernels)], _T3F_TOL, False, 60, f"T3S2[{idx}]")


@pytest.mark.parametrize("idx", range(len(CT3_CASES)))
def test_conv_t3_staged_run_kernel_under_guards(g, idx):
    _ct3_case(g, idx)


def _ct3_case(g, idx, tag=""):
    dims, cins, cout, k, extra = CT3_CASES[idx]

    def same_kernels(kl, sink):
        t3 = [n for n in kl.names if n.startswith("conv_t3:")]
        assert len(t3) == (1 if idx in (5, 8) else 2), kl.names
        if "M1_CT3_BN" in extra:
            assert all(f":bn{extra['M1_CT3_BN']}:" in n for n in t3), kl.names
        if "M1_CT3_KSPLIT" in extra:
            assert all(n.endswith(f":ks{extra['M1_CT3_KSPLIT']}") for n in t3), kl.names
    _conv_case(g, False, k, (1, 1, 1), cins, cout, dims, BF16, [(dict(CT3_LOW, **extra), same_kernels)], EW, True, 70, f"CT3[{idx}]{tag}")


_HALO_TOL = dict(y=1e-2, dx=1e-2, dw=2e-4, db=2e-4)               # y, dx: test_conv_halo_parity_classes; dW, db: the fuzz's limit


@pytest.mark.parametrize("idx", range(len(HALO_CLS_CASES)))
def test_conv_halo_parity_classes_under_guards(g, idx):
    (N, D, H, W), clo, chi, transposed = HALO_CLS_CASES[idx]
    k, s = (1, 3, 3), (1, 2, 2)

    def same_kernels(kl, sink):
        assert kl.ran("conv_halo_cls"), kl.names
    cfg = dict(M1_HALO=2, M1_HALO_CLASSES=1)
    if transposed:
        _conv_case(g, True, k, s, [clo], chi, (N, D, H, W), BF16, [(cfg, same_kernels)], _HALO_TOL, False, 95, f"HALO[{idx}]")
    else:
        _conv_case(g, False, k, s, [chi], clo, (N, D, 2 * H, 2 * W), BF16, [(cfg, same_kernels)], _HALO_TOL, False, 95, f"HALO[{idx}]")


def test_conv_halo_parity_classes_accumulate_under_guards(g):
    """conv1 || conv4 of a strided SE block: the second data gradient adds into the first one's (guarded) buffer."""
    k, s = (1, 3, 3), (1, 2, 2)
    x = _q(rnd((2, 2, 24, 32, 32), 96), BF16)
    w1, w4 = _q(rnd((*k, 32, 16), 6, 1.0 / (32 * 9) ** 0.5), BF16), _q(rnd((*k, 32, 64), 7, 1.0 / (32 * 9) ** 0.5), BF16)
    b1, b4 = rnd((16,), 8), rnd((64,), 9)
    f = lambda x_, a, b, c, d: (util.ref_conv3d_same(x_, a, b, s), util.ref_conv3d_same(x_, c, d, s))      # noqa: E731
    y1o, y4o = f(x, w1, b1, w4, b4)
    dy1, dy4 = _q(rnd(tuple(y1o.shape), 10), BF16), _q(rnd(tuple(y4o.shape), 11), BF16)
    _, grads = _ref_grads(f, [x, w1, b1, w4, b4], (dy1, dy4))
    with ops.config(M1_HALO=2), ops.kernel_log() as kl:
        xd = g.put(x, BF16).requires_grad_(True)
        pd = [g.put(t).requires_grad_(True) for t in (w1, b1, w4, b4)]
        za, zb = ops.fanout(xd * 1.0, 2)
        y1 = ops.conv3d_same([za], pd[0], pd[1], k, s); y4 = ops.conv3d_same([zb], pd[2], pd[3], k, s)
        torch.autograd.backward([y1, y4], [g.put(dy1, BF16), g.put(dy4, BF16)])
        torch.cuda.synchronize()
    _done(g)
    assert sum(n.startswith("conv_halo_cls:") for n in kl.names) == 2, kl.names
    assert rel_err(y1, y1o) < 1e-2 and rel_err(y4, y4o) < 1e-2
    assert rel_err(xd.grad, grads[0]) < 1.5e-2
    for p, r in zip(pd, grads[1:]):
        assert rel_err(p.grad, r) < 2e-4


_THIN_TOL = dict(y=1e-2, dx=1e-2, dw=1e-4, db=2e-4)               # test_conv_thin_forward_kernel / _pointwise_dgrad_kernel (db: the fuzz's limit)
THIN_PW_CASES = [((2, 3, 8, 10), 128, 2), ((1, 2, 5, 7), 32, 2), ((2, 2, 6, 6), 256, 4), ((1, 3, 4, 8), 512, 6)]


@pytest.mark.parametrize("idx", range(len(THIN_FWD_CASES)))
def test_conv_thin_forward_kernel_under_guards(g, idx):
    _thin_case(g, idx)


def _thin_case(g, idx, tag=""):
    dims, cin, cout, k = THIN_FWD_CASES[idx]

    def same_kernels(kl, sink):
        assert kl.ran("thin_fwd"), kl.names
    _conv_case(g, False, k, (1, 1, 1), [cin], cout, dims, BF16, [(dict(M1_THIN=2), same_kernels)], _THIN_TOL, True, 90, f"THIN[{idx}]{tag}")


@pytest.mark.parametrize("idx", range(len(THIN_PW_CASES)))
def test_conv_thin_pointwise_dgrad_kernel_under_guards(g, idx):
    dims, cin, cout = THIN_PW_CASES[idx]

    def same_kernels(kl, sink):
        assert kl.ran("thin_pw_dgrad"), kl.names
    _conv_case(g, False, (1, 1, 1), (1, 1, 1), [cin], cout, dims, BF16, [(dict(M1_THIN=2), same_kernels)], _THIN_TOL, False, 91, f"THINPW[{idx}]")


# ---- the binding rounds every conv workspace up to 256 bytes (panels._conv_ws); the header promises m1_conv_ws_bytes ------------
WS_EXACT_CASES = [("TF", 0), ("TF", 5), ("TF", 11), ("TF", 19), ("TF", 24), ("T3F", 0), ("T3F", 5), ("T3F", 10), ("CT3", 3), ("THIN", 1)]


@pytest.mark.parametrize("table,idx", WS_EXACT_CASES)
def test_conv_workspace_of_exactly_the_queried_size(g, monkeypatch, table, idx):
    """The forward, data-gradient and weight-gradient entry points with workspaces of exactly m1_conv_ws_bytes(d, transposed, role)
    bytes (one byte where the query answers 0: an empty tensor has no address), not the binding's max(n, 256)."""
    import ctypes as C
    asked = []

    def exact_ws(d, transposed, role, device, zero=False):
        n = int(PKG.hip.lib.load().m1_conv_ws_bytes(C.byref(d), 1 if transposed else 0, role))
        asked.append((role, n))
        return (torch.zeros if zero else torch.empty)(max(n, 1), dtype=torch.uint8, device=device)
    monkeypatch.setattr(PKG.hip.panels, "_conv_ws", exact_ws)
    monkeypatch.setattr(ops, "_conv_ws", exact_ws)
    # (the same cases, switches and kernel expectations as the table tests above: M1_T3_MIN_BLOCKS = 1 for the first len(TF_CASES))
    {"TF": _tf_case, "T3F": _t3f_case, "CT3": _ct3_case, "THIN": _thin_case}[table](g, idx, " exact ws")
    assert {r for r, _ in asked} == {0, 1, 2} and max(n for _, n in asked) > 1, asked


# ---- conv1 || conv4 pair ---------------------------------------------------------------------------------------------------------
PAIR_CASES = [([128, 128], 32, 128, (3, 3, 3), (1, 1, 1), (2, 4, 8, 8)), ([64], 64, 256, (3, 3, 3), (2, 2, 2), (2, 4, 8, 8)),
              ([64, 32, 32], 32, 128, (1, 3, 3), (1, 2, 2), (1, 3, 8, 16)), ([256, 256, 256], 64, 256, (3, 3, 3), (1, 1, 1), (1, 2, 4, 4))]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("case", PAIR_CASES)
@pytest.mark.parametrize("fused_fwd", ["0", "1"])
def test_conv_pair_under_guards(g, monkeypatch, dtype, case, fused_fwd):
    """test_conv_pair_matches_two_convs under the guards, fresh gradients and sinks (conv4's weight gradient hangs on a tap of y4 on
    the side stream; in sink mode all of them are queued and folded by flush_deferred)."""
    cins, c1, c4, k, s, dims = case
    monkeypatch.setenv("M1_CONV_PAIR_FWD", fused_fwd)
    xs = [_q(rnd((*dims, c), 30 + i), dtype) for i, c in enumerate(cins)]
    cin = sum(cins)
    sc = 1.0 / (cin * k[0] * k[1] * k[2]) ** 0.5
    ps = [rnd((*k, cin, c1), 3, sc), rnd((c1,), 4, 0.1), rnd((*k, cin, c4), 5, sc), rnd((c4,), 6, 0.1)]
    f = lambda x, a, b, c, d: (util.ref_conv3d_same(x, a, b, s), util.ref_conv3d_same(x, c, d, s))      # noqa: E731
    y1o, y4o = f(torch.cat(xs, -1), *ps)
    dy1, dy4 = _q(rnd(tuple(y1o.shape), 7), dtype), _q(rnd(tuple(y4o.shape), 8), dtype)
    (y1o, y4o), grads = _ref_grads(f, [torch.cat(xs, -1), *ps], (dy1, dy4))
    tol = TOL[dtype]
    for sink in (False, True):
        ops.invalidate_panels()
        xd = [g.put(x, dtype).requires_grad_(True) for x in xs]
        pd = [g.put(t).requires_grad_(True) for t in ps]
        sk = Sinks(g, pd) if sink else None
        assert ops.conv_pair_supported(xd, pd[0], pd[2], s)
        y1, s1, y4, s4, br = ops.conv_pair_same(xd, *pd, k, s)
        br.join(y4, s4)
        torch.autograd.backward([y1, y4], [g.put(dy1, dtype), g.put(dy4, dtype)])
        ops.flush_deferred()
        torch.cuda.synchronize()
        _done(g)
        assert rel_err(y1, y1o) < tol and rel_err(y4, y4o) < tol
        for y, st in ((y1, s1), (y4, s4)):
            yf = y.detach().double()
            assert rel_err(st[..., 0], yf.mean(dim=(1, 2, 3)).float()) < 1e-3 + tol
            assert rel_err(st[..., 1], (1 / torch.sqrt(yf.var(dim=(1, 2, 3), unbiased=False) + 1e-3)).float()) < 1e-3
        for i, (p, want, nm) in enumerate(zip(pd, grads[1:], "w1 b1 w4 b4".split())):
            if sink:
                assert p.grad is None and rel_err(sk.got(i), sk.start(i) + want) < tol * 2, (nm, "sink")
            else:
                assert rel_err(p.grad, want) < tol * 2, nm
        if sink:
            sk.assert_neighbours_untouched("pair")
        off = 0
        for x in xd:
            c = x.shape[-1]
            assert rel_err(x.grad, grads[0][..., off:off + c]) < tol * 2
            off += c


# ---- InstanceNorm-backward sums from the data gradient's epilogue; `partial` is allocated at exactly the header's size -----------
INBWD_CASES = [((2, 4, 16, 16), 32, 32, (3, 3, 3)), ((2, 4, 16, 16), 64, 256, (1, 1, 1)), ((4, 2, 4, 8), 64, 64, (3, 3, 3)),
               ((1, 3, 9, 10), 24, 16, (3, 3, 3)), ((2, 8, 32, 32), 8, 8, (3, 3, 3)), ((1, 6, 24, 40), 16, 16, (3, 3, 3)),
               ((2, 4, 16, 16), 16, 64, (1, 1, 1)), ((2, 8, 32, 32), 8, 32, (1, 1, 1))]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("case", INBWD_CASES)
def test_dgrad_inbwd_epilogue_under_guards(g, dtype, case):
    """y = conv(lrelu(IN(x))): m1_conv3d_dgrad_inbwd writes its partial sums into N*rows*C*2 + N*C*2 + 64 floats (ops allocates exactly
    that), m1_instnorm_bwd_partials folds them; fresh gradients and sinks."""
    dims, c, cout, k = case
    x = _q(rnd((*dims, c), 1), dtype); gm = 1.0 + 0.2 * rnd((c,), 2); bt = 0.1 * rnd((c,), 3)
    w = rnd((*k, c, cout), 4, 1.0 / (c * k[0] * k[1] * k[2]) ** 0.5); b = rnd((cout,), 5)
    dy = _q(rnd((*dims, cout), 6), dtype)
    _, gro = _ref_grads(lambda x_, g_, b_, w_, bb_: util.ref_conv3d_same(util.ref_instnorm_act(x_, g_, b_, 0.1), w_, bb_, (1, 1, 1)),
                        [x, gm, bt, w, b], (dy,))
    halo_case = c <= 16 and dtype == BF16
    tol = 2e-4 if dtype == F32 else 4e-2
    assert ops._INBWD["on"]
    with ops.config(**({"M1_HALO": 2} if halo_case else {})):
        for sink in (False, True):
            ops.invalidate_panels()
            f0 = dict(ops._INBWD)
            xd = g.put(x, dtype).requires_grad_(True)
            ps = [g.put(t).requires_grad_(True) for t in (gm, bt, w, b)]
            sk = Sinks(g, ps) if sink else None
            a = ops.instnorm_act(xd, ps[0], ps[1], 0.1, ops.instnorm_stats(xd))
            y = ops.conv3d_same([a], ps[2], ps[3], k, (1, 1, 1))
            y.backward(g.put(dy, dtype))
            ops.flush_deferred()
            torch.cuda.synchronize()
            _done(g)
            fused = ops._INBWD["fused"] - f0["fused"], ops._INBWD["plain"] - f0["plain"]
            assert sum(fused) == 1, fused
            if c >= 24 or halo_case:
                assert fused == (1, 0), fused
            assert rel_err(xd.grad, gro[0]) < tol
            for i, (p, want) in enumerate(zip(ps, gro[1:])):
                if sink:
                    assert p.grad is None and rel_err(sk.got(i), sk.start(i) + want) < tol, (i, "sink")
                else:
                    assert rel_err(p.grad, want) < tol, i
            if sink:
                sk.assert_neighbours_untouched("inbwd")


@pytest.mark.parametrize("transposed", [False, True])
def test_repack_all_under_guards(g, transposed):
    """test_repack_all_refreshes_cached_panels with the panels' workspaces, the weights and every activation guarded."""
    k, s = (3, 3, 3), ((1, 2, 2) if transposed else (1, 1, 1))
    cins, cout = [16, 3, 32], 24
    xs = [g.put(rnd((2, 4, 8, 6, c), 20 + i), BF16).requires_grad_(True) for i, c in enumerate(cins)]
    w = g.put(rnd((*k, cout, sum(cins)) if transposed else (*k, sum(cins), cout), 7, 0.2)).requires_grad_(True)
    b = g.put(rnd((cout,), 8)).requires_grad_(True)
    f = ops.conv3d_transpose_same if transposed else ops.conv3d_same

    def run():
        for x in xs:
            x.grad = None
        y = f(xs, w, b, k, s)
        y.backward(torch.ones_like(y))
        return y.detach().float().clone(), [x.grad.float().clone() for x in xs]

    ops.invalidate_panels()
    run()
    alias = torch.from_dlpack(torch.utils.dlpack.to_dlpack(w.detach()))
    v0 = w._version
    alias.mul_(-1.5)
    assert w._version == v0
    ops.repack_all()
    y1, g1 = run()
    ops.invalidate_panels()
    y2, g2 = run()
    torch.cuda.synchronize()
    _done(g)
    assert torch.equal(y1, y2) and bool(torch.isfinite(y1).all())
    for a, c in zip(g1, g2):
        assert torch.equal(a, c) and bool(torch.isfinite(a).all())
    yo = (util.ref_conv3d_transpose_same if transposed else util.ref_conv3d_same)(
        torch.cat([x.detach().float().cpu() for x in xs], -1), _q(w.detach().cpu(), BF16), b.detach().cpu(), s)
    assert rel_err(y1, yo) < TOL[BF16]


# =================================================================================================================================
# 3. everything else
# =================================================================================================================================
def _two_chunks_plus_one(C, N):
    """(D, H, W) whose voxel count makes the reductions of a C-channel tensor take >= 2 whole chunks plus one voxel."""
    per_block = max(16, 256 * 16 // C)                     # (test_ops_at_scale.red_nchunks: the chunk of a small volume)
    V = 2 * per_block + 1
    assert red_nchunks(V, C, N) == 3 and lib_nchunks(N, V, C, 2) == 3 and V % 256
    return (1, 1, V)


# (C, N, dims): odd extents, and per channel count one volume of two reduction chunks plus one voxel
NORM_CASES = [(1, 2, (3, 5, 7)), (3, 1, (2, 5, 9)), (5, 3, (1, 7, 11)), (8, 2, None), (24, 1, None), (40, 3, None), (64, 2, None), (2, 2, None)]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("C,N,dims", NORM_CASES)
def test_instnorm_under_guards(g, dtype, C, N, dims):
    dims = _two_chunks_plus_one(C, N) if dims is None else dims
    shape = (N, *dims, C)
    x = _q(rnd(shape, 1) * 2.0 + 0.5, dtype)
    gm, bt = 1 + 0.2 * rnd((C,), 2), 0.3 * rnd((C,), 3)
    dy = _q(rnd(shape, 4), dtype)
    (yo,), (gx, gg, gb) = _ref_grads(lambda x_, g_, b_: util.ref_instnorm_act(x_, g_, b_, 0.1), [x, gm, bt], (dy,))
    sto = util.ref_in_stats(x)
    tol = TOL[dtype]
    for sink in (False, True):
        xd = g.put(x, dtype).requires_grad_(True)
        gd, bd = g.put(gm).requires_grad_(True), g.put(bt).requires_grad_(True)
        sk = Sinks(g, [gd, bd]) if sink else None
        st = ops.instnorm_stats(xd.detach())
        y = ops.instnorm_act(xd, gd, bd, 0.1, st if sink else None)
        y.backward(g.put(dy, dtype))
        torch.cuda.synchronize()
        _done(g)
        assert float((st[..., 0].cpu().double() - sto[..., 0]).abs().max()) < 1e-4 * (1.0 + float(sto[..., 0].abs().max()))
        assert rel_err(st[..., 1], sto[..., 1]) < 1e-3
        assert rel_err(y, yo) < tol and rel_err(xd.grad, gx) < tol * 2
        if sink:
            assert rel_err(sk.got(0), sk.start(0) + gg) < tol * 2 and rel_err(sk.got(1), sk.start(1) + gb) < tol * 2
            sk.assert_neighbours_untouched("instnorm")
        else:
            assert rel_err(gd.grad, gg) < tol * 2 and rel_err(bd.grad, gb) < tol * 2


def test_se_gate_batch_under_guards(g):
    cfgs = [(8, 8), (24, 4), (40, 8), (64, 8), (5, 5), (3, 1)]
    host = [(0.5 * rnd((F_,), 10 * k + 1), rnd((1, 1, 1, F_, F_ // red), 10 * k + 2, 0.5), 0.1 * rnd((F_ // red,), 10 * k + 3),
             rnd((1, 1, 1, F_ // red, F_), 10 * k + 4, 0.5), 0.1 * rnd((F_,), 10 * k + 5)) for k, (F_, red) in enumerate(cfgs)]
    pairs = ops.se_gate_batch([tuple(g.put(t) for t in ps) for ps in host])
    torch.cuda.synchronize()
    _done(g)
    for (b3, W6, b6, W7, b7), (hidden, gate) in zip(host, pairs):
        h_pre = b3.double() @ W6.double().reshape(W6.shape[-2], -1) + b6.double()
        g_ref = torch.sigmoid(torch.nn.functional.leaky_relu(h_pre, 0.1) @ W7.double().reshape(W7.shape[-2], -1) + b7.double())
        assert rel_err(gate, g_ref) < 1e-5 and rel_err(hidden, h_pre) < 1e-5


# F, reduction, N, dims (None: two reduction chunks plus one voxel)
SE_CASES = [(8, 8, 2, None), (24, 4, 1, None), (40, 8, 3, (1, 5, 41)), (64, 8, 2, None), (5, 5, 1, (3, 5, 7)), (3, 1, 2, (2, 3, 5))]


# (the duplicating form needs whole 16-byte channel vectors: se_combine raises otherwise)
_SE_PARAMS = [(dt, dr, md, *c) for c in SE_CASES for md in ("plain", "ident", "dup") for dr in (0.0, 0.4) for dt in (F32, BF16)
              if not (md == "dup" and c[0] % (8 if dt == BF16 else 4))]


@pytest.mark.parametrize("dtype,drop,mode,F_,red,N,dims", _SE_PARAMS)
def test_se_combine_under_guards(g, dev, dtype, drop, mode, F_, red, N, dims):
    """se_combine plain, with the identity residual and duplicating, with and without the fused dropout (bf16, F % 8 == 0: the stored
    keep mask), fresh gradients and sinks (the SE gate backward queued, run by flush_deferred as one m1_se_gate_bwd_batch)."""
    dims = _two_chunks_plus_one(F_, N) if dims is None else dims
    shp = (N, *dims, F_)
    oshp = (2 * N, *dims, F_) if mode == "dup" else shp
    Fr = F_ // red
    y3, y4 = _q(rnd(shp, 1), dtype), _q(rnd(shp, 2) * 1.5 + 0.2, dtype)
    ps = [1 + 0.2 * rnd((F_,), 3), 0.5 * rnd((F_,), 4), 1 + 0.2 * rnd((F_,), 5), 0.5 * rnd((F_,), 6), rnd((1, 1, 1, F_, Fr), 7, 0.5),
          0.1 * rnd((Fr,), 8), rnd((1, 1, 1, Fr, F_), 9, 0.5), 0.1 * rnd((F_,), 10)]
    if mode == "ident":
        ps = ps[:2] + ps[4:]
    dout = _q(rnd(oshp, 11), dtype)
    rng = g.put(torch.tensor([12345, 3], dtype=torch.int64)) if drop > 0 else None
    keep = None
    if drop > 0:                                           # the draw is a pure function of (seed, step, layer id, output element index)
        keep = (ops.dropout(g.put(torch.ones(oshp), dtype), drop, rng, 7) != 0).double().cpu()

    def fn(y3_, y4_, *p):
        p = list(p)
        if mode == "ident":
            p = p[:2] + [None, None] + p[2:]
        return util.ref_se_combine(y3_, y4_, *p, rate=drop, keep=keep, dup=mode == "dup")
    (yo,), grads = _ref_grads(fn, [y3, y4, *ps], (dout,))
    tol = TOL[dtype]
    for sink in (False, True):
        a, b = g.put(y3, dtype).requires_grad_(True), g.put(y4, dtype).requires_grad_(True)
        pd = [g.put(t).requires_grad_(True) for t in ps]
        sk = Sinks(g, pd) if sink else None
        full = pd if mode != "ident" else pd[:2] + [None, None] + pd[2:]
        out = ops.se_combine(a, b, *full, drop, rng, 7, None, None, None, dup=mode == "dup")
        out.backward(g.put(dout, dtype))
        if sink:
            assert len(ops._SE_DEFER) == 1
        ops.flush_deferred()
        torch.cuda.synchronize()
        _done(g)
        assert tuple(out.shape) == oshp and rel_err(out, yo) < tol
        assert rel_err(a.grad, grads[0]) < tol * 3 and rel_err(b.grad, grads[1]) < tol * 3
        for i, (p, want) in enumerate(zip(pd, grads[2:])):
            if sink:
                assert p.grad is None and rel_err(sk.got(i), sk.start(i) + want) < tol * 3, (i, "sink")
            else:
                assert rel_err(p.grad, want) < tol * 3, i
        if sink:
            sk.assert_neighbours_untouched("se_combine")


# C, N, fine (theta / x) extents, up-sampling of phi; odd fine extents where the factor is 1
GATE_CASES = [(8, 2, (3, 6, 10), (1, 2, 2)), (24, 1, (4, 8, 4), (2, 2, 1)), (40, 3, (3, 4, 8), (1, 4, 4)), (64, 1, (2, 6, 5), (2, 2, 1)),
              (3, 2, (5, 4, 6), (1, 2, 2)), (1, 1, (3, 7, 4), (1, 1, 2))]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("C,N,fine,up", GATE_CASES)
def test_gate_sigma_under_guards(g, dtype, C, N, fine, up):
    coarse = tuple(f // u for f, u in zip(fine, up))
    theta, phi = _q(rnd((N, *fine, C), 1), dtype), _q(rnd((N, *coarse, C), 2), dtype)
    w, b = rnd((1, 1, 1, C, 1), 3, 0.3), rnd((1,), 4)
    ds = _q(rnd((N, *fine), 5), dtype)
    (so,), (gt, gp, gw, gb) = _ref_grads(util.ref_gate_sigma, [theta, phi, w, b], (ds,))
    tol = TOL[dtype]
    for sink in (False, True):
        td, pd = g.put(theta, dtype).requires_grad_(True), g.put(phi, dtype).requires_grad_(True)
        wd, bd = g.put(w).requires_grad_(True), g.put(b).requires_grad_(True)
        sk = Sinks(g, [wd, bd]) if sink else None
        sg = ops.gate_sigma(td, pd, wd, bd)
        sg.backward(g.put(ds, dtype))
        torch.cuda.synchronize()
        _done(g)
        assert rel_err(sg, so) < tol and rel_err(td.grad, gt) < tol * 2 and rel_err(pd.grad, gp) < tol * 2
        if sink:
            assert rel_err(sk.got(0), sk.start(0) + gw) < tol * 2 and rel_err(sk.got(1), sk.start(1) + gb) < tol * 2
            sk.assert_neighbours_untouched("gate_sigma")
        else:
            assert rel_err(wd.grad, gw) < tol * 2 and rel_err(bd.grad, gb) < tol * 2


# C, N, dims of x, sub-sampling of sigma against x
MUL_CASES = [(8, 2, (3, 6, 10), (1, 2, 2)), (3, 1, (4, 4, 6), (2, 2, 2)), (5, 3, (3, 5, 7), (1, 1, 1)), (24, 1, (2, 6, 10), (2, 2, 2)),
             (40, 2, (3, 4, 6), (1, 2, 2)), (64, 1, (5, 2, 6), (1, 2, 2)), (1, 2, (3, 6, 2), (1, 2, 2)), (2, 1, (2, 2, 14), (2, 2, 2))]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("C,N,dims,ss", MUL_CASES)
def test_mul_sigma_under_guards(g, dtype, C, N, dims, ss):
    x, dy = _q(rnd((N, *dims, C), 1), dtype), _q(rnd((N, *dims, C), 3), dtype)
    sig = _q(torch.sigmoid(rnd((N, *[d // s_ for d, s_ in zip(dims, ss)]), 2)), dtype)
    (yo,), (gx, gs) = _ref_grads(lambda x_, s_: util.ref_upsample(s_.unsqueeze(-1), ss) * x_, [x, sig], (dy,))
    xd, sd = g.put(x, dtype).requires_grad_(True), g.put(sig, dtype).requires_grad_(True)
    y = ops.mul_sigma(xd, sd, ss)
    y.backward(g.put(dy, dtype))
    torch.cuda.synchronize()
    _done(g)
    tol = TOL[dtype]
    assert rel_err(y, yo) < tol and rel_err(xd.grad, gx) < tol and rel_err(sd.grad, gs) < tol * 2


# Ci, Cx, N, dims of x, sub-sampling of sigma against x, up-sampling of phi against theta (whole 16-byte channel vectors: one launch)
GSM_CASES = [(8, 24, 2, (3, 6, 10), (1, 2, 2), (1, 1, 1)), (40, 8, 1, (4, 8, 4), (2, 2, 2), (1, 2, 1)), (64, 64, 1, (3, 4, 12), (1, 2, 2), (1, 2, 2)),
             (24, 40, 3, (2, 6, 6), (2, 2, 2), (1, 1, 3))]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("Ci,Cx,N,dims,ss,coarse", GSM_CASES)
def test_gate_sigma_mul_under_guards(g, dtype, Ci, Cx, N, dims, ss, coarse):
    tdims = tuple(d // s_ for d, s_ in zip(dims, ss))
    pdims = tuple(t // c for t, c in zip(tdims, coarse))
    theta, phi, x, dy = (_q(t, dtype) for t in (rnd((N, *tdims, Ci), 1), rnd((N, *pdims, Ci), 2), rnd((N, *dims, Cx), 3), rnd((N, *dims, Cx), 6)))
    w, b = rnd((1, 1, 1, Ci, 1), 4, 0.3), rnd((1,), 5)
    (yo, so), (gt, gp, gw, gb, gx) = _ref_grads(
        lambda t_, p_, w_, b_, x_: util.ref_gate_sigma_mul(t_, p_, w_, b_, x_, ss, None if dtype == F32 else dtype),
        [theta, phi, w, b, x], (dy, torch.zeros((N, *tdims))))
    td, pd, xd = (g.put(t, dtype).requires_grad_(True) for t in (theta, phi, x))
    wd, bd = g.put(w).requires_grad_(True), g.put(b).requires_grad_(True)
    y, sg = ops._GateSigmaMul.apply(td, pd, wd, bd, xd, ss)
    y.backward(g.put(dy, dtype))
    torch.cuda.synchronize()
    _done(g)
    tol = TOL[dtype]
    assert rel_err(y, yo) < tol and rel_err(sg, so) < tol
    for got, want, name in zip((td, pd, wd, bd, xd), (gt, gp, gw, gb, gx), ("dtheta", "dphi", "dw", "db", "dx")):
        assert rel_err(got.grad, want) < tol * 2, name


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("L_", [1, 2, 3])
@pytest.mark.parametrize("N,V", [(2, (3, 5, 7)), (4, (1, 3, 43))])
def test_latent_sample_under_guards(g, dtype, L_, N, V):
    """Injected draws in modes 0 (sample), 1 (mean) and 2 (stacked: draws for the first half only) and the draws made in the kernel."""
    ml = _q(rnd((N, *V, 2 * L_), 1) * 0.2, dtype)                 # log-sigma straddles the +-0.1 clip
    eps, dz = _q(rnd((N, *V, L_), 3), dtype), _q(rnd((N, *V, L_), 4), dtype)
    tol = 1e-5 if dtype == F32 else TOL[BF16]
    (zo,), (gml,) = _ref_grads(lambda m_: util.ref_latent_sample(m_, eps.double()), [ml], (dz,))
    h = N // 2

    def stacked(m_):
        return torch.cat([util.ref_latent_sample(m_[:h], eps[:h].double()), m_[h:, ..., :L_]], 0)
    (z2o,), (g2,) = _ref_grads(stacked, [ml], (dz,))
    mld = g.put(ml, dtype).requires_grad_(True)
    z = ops.latent_sample(mld, g.put(eps, dtype), False)
    z.backward(g.put(dz, dtype))
    zm = ops.latent_sample(g.put(ml, dtype), None, True)
    ml2 = g.put(ml, dtype).requires_grad_(True)
    z2 = ops.latent_sample(ml2, g.put(eps[:h], dtype), False, stacked=True)
    z2.backward(g.put(dz, dtype))
    rng = g.put(torch.tensor([1234, 7], dtype=torch.int64))
    mlr = g.put(ml, dtype).requires_grad_(True)
    zr = ops.latent_sample(mlr, None, False, rng=rng, stream_id=5)
    zr.backward(g.put(dz, dtype))
    zr2 = ops.latent_sample(g.put(ml, dtype), None, False, stacked=True, rng=rng, stream_id=5)
    torch.cuda.synchronize()
    _done(g)
    assert rel_err(z, zo) < tol and rel_err(mld.grad, gml) < tol
    assert rel_err(zm, ml[..., :L_]) < 1e-7
    assert rel_err(z2, z2o) < tol and rel_err(ml2.grad, g2) < tol
    # draws made in the kernel: finite, |eps| < 6, the stacked mode draws for its first half what the plain mode draws for a batch of
    # that size, and the backward regenerates the forward's draw: d z / d logsigma = z - mu inside the clip band
    sig = torch.exp(torch.clamp(ml[..., L_:], -0.1, 0.1))
    er = (zr.detach().cpu().float() - ml[..., :L_]) / sig
    assert bool(torch.isfinite(er).all()) and float(er.abs().max()) < 6.0 + (0.5 if dtype == BF16 else 0.0)
    assert torch.equal(zr2[h:].cpu().float(), ml[h:, ..., :L_]) and bool(torch.isfinite(zr2.float()).all())
    if dtype == F32:
        inside = (ml[..., L_:].abs() <= 0.1).float()
        assert rel_err(mlr.grad[..., :L_], dz) < 1e-7
        assert rel_err(mlr.grad[..., L_:], dz * (zr.detach().cpu() - ml[..., :L_]) * inside) < 1e-5
    else:
        assert bool(torch.isfinite(mlr.grad.float()).all())


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("L_,N,first,V", [(1, 1, None, (3, 5, 7)), (2, 2, None, (1, 3, 43)), (3, 3, None, (2, 5, 9)), (1, 2, 1, (3, 5, 7)),
                                          (2, 3, 1, (1, 3, 43)), (3, 3, 2, (2, 5, 9)), (2, 2, 2, (1, 1, 129))])
def test_kl_under_guards(g, dtype, L_, N, first, V):
    mq, mp = _q(rnd((N, *V, 2 * L_), 1) * 0.2, dtype), _q(rnd((N, *V, 2 * L_), 2) * 0.2, dtype)
    (ko,), (gq, gp) = _ref_grads(lambda q_, p_: util.ref_kl(q_, p_, first), [mq, mp], (torch.tensor([2.5]),))
    qd, pd = g.put(mq, dtype).requires_grad_(True), g.put(mp, dtype).requires_grad_(True)
    kl = ops.kl_mvn_diag(qd, pd, first)
    kl.backward(g.put(torch.tensor([2.5])))
    torch.cuda.synchronize()
    _done(g)
    tol = 1e-5 if dtype == F32 else TOL[BF16]
    assert rel_err(kl, ko) < 1e-5 and rel_err(qd.grad, gq) < tol and rel_err(pd.grad, gp) < tol
    if first is not None and first < N:                    # the samples beyond `first`: zeros, exact to the last element
        for t in (qd.grad, pd.grad):
            assert tuple(t.shape) == tuple(mq.shape) and int(torch.count_nonzero(t[first:].float())) == 0
            assert not bool(torch.isnan(t.float()).any())


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("nc,N,dims", [(2, 2, (2, 8, 24)), (3, 1, (4, 8, 8)), (2, 3, (2, 16, 8))])
def test_softmax_heads_under_guards(g, dtype, nc, N, dims):
    D, H, W = dims
    ups = [(1, 1, 1), (1, 2, 2), (1, 4, 4), (2, 8, 8)]
    ls = [_q(rnd((N, D // u[0], H // u[1], W // u[2], nc), 10 + i), dtype) for i, u in enumerate(ups)]
    dp = rnd((N, D, H, W, nc * len(ups)), 20)
    (po,), grads = _ref_grads(lambda *ts: util.ref_softmax_heads(ts, ups), ls, (dp,))
    ld = [g.put(t, dtype).requires_grad_(True) for t in ls]
    p = ops.softmax_heads(ld, ups)
    p.backward(g.put(dp))
    torch.cuda.synchronize()
    _done(g)
    assert p.dtype == F32 and rel_err(p, po) < 1e-5
    for a, b in zip(ld, grads):
        assert rel_err(a.grad, b) < TOL[dtype]


@pytest.mark.parametrize("nheads,nc,gamma,ydt,N,dims", [(1, 2, 2.0, F32, 2, (3, 9, 7)), (4, 2, 2.0, BF16, 1, (3, 9, 7)), (2, 3, 1.5, F32, 3, (1, 5, 53)),
                                                       (1, 2, 0.0, F32, 2, (2, 3, 5)), (3, 2, 1.0, BF16, 2, (1, 1, 1027))])
def test_focal_loss_under_guards(g, nheads, nc, gamma, ydt, N, dims):
    gen = torch.Generator().manual_seed(5)
    p = torch.softmax(3.0 * torch.randn((N, *dims, nheads, nc), generator=gen), dim=-1)
    p[0, 0, 0, 0, 0] = torch.tensor([1.0] + [0.0] * (nc - 1))            # saturated: outside the clip range
    p[-1, -1, -1, -1, -1] = torch.tensor([0.0] * (nc - 1) + [1.0])
    p = p.reshape(N, *dims, nheads * nc)
    y = torch.nn.functional.one_hot(torch.randint(0, nc, (N, *dims), generator=gen), nc).float()
    alpha = [0.75, 0.25, 0.5][:nc]
    po = p.double().requires_grad_(True)
    lo = util.ref_focal(y.double(), po, alpha, gamma)
    (3.0 * lo).backward()
    pd = g.put(p).requires_grad_(True)
    ld = ops.focal_loss(g.put(y, ydt), pd, alpha, gamma)
    (3.0 * ld).backward()
    torch.cuda.synchronize()
    _done(g)
    assert abs(float(ld.detach()) - float(lo.detach())) < 1e-5 * max(1.0, abs(float(lo.detach())))
    assert rel_err(pd.grad, po.grad) < 1e-5


def test_dist_map_and_dice_boundary_under_guards(g, dev):
    import test_dice_boundary as DB
    for name in ("every_face", "empty_class", "nc3", "d1", "w1", "h1", "single_voxel"):
        for dtype in (F32, BF16):
            got = ops.dist_map(g.put(torch.from_numpy(DB.CASES[name]), dtype))
            torch.cuda.synchronize()
            _done(g)
            DB._check_phi(got, DB.phi_ref(DB.CASES[name]))
    for nheads, nc, ydt, shape in ((1, 2, F32, (2, 3, 7, 9)), (3, 3, BF16, (1, 5, 6, 11)), (2, 2, F32, (3, 2, 9, 15))):
        y, p = DB._problem(shape, nc, nheads, 100 + 10 * nheads + nc)
        w = [0.5, 1.5]
        pr = torch.from_numpy(p).double().requires_grad_(True)
        lr = DB.loss_ref(torch.from_numpy(y), pr, torch.from_numpy(DB.phi_ref(y, edt=DB.edt_auto)), w)
        lr.backward()
        pg = g.put(torch.from_numpy(p)).requires_grad_(True)
        l = ops.dice_boundary_loss(g.put(torch.from_numpy(y), ydt), pg, w, 1e-7)
        l.backward()
        torch.cuda.synchronize()
        _done(g)
        assert abs(float(l.detach()) - float(lr.detach())) <= 1e-5 * abs(float(lr.detach()))
        assert float((pg.grad.double().cpu() - pr.grad).abs().max()) <= 1e-5 * float(pr.grad.abs().max())


def test_augmentations_under_guards(g, dev):
    """Every stage bit alone and the whole chain, both objectives, on injected tables (test_stage_and_chain_match_the_fp64_restatement
    at its small size), and the table drawn on the device."""
    import test_augmentations as TA
    A = TA.A
    for stage, bits in TA.STAGES.items():
        for obj in ("lesion", "zonal"):
            img, lab, nimg = TA._problem(obj, "small", 1)
            N, D, H = img.shape[:3]
            hyper = [1.0, 0.25, 0.15 if bits & A.TRANSLATE else 0, 10.0 if bits & A.ROTATE else 0, bool(bits & A.FLIP),
                     1.2 if bits & A.ZOOM else 0, 0.1 if bits & A.NOISE else 0, 0.025 if bits & A.CSHIFT else 0, bool(bits & A.POOR),
                     [0.5, 1.5] if bits & A.GAMMA else [0, 0]]
            stages = A.enabled_stages(A.parse_augm_params(hyper), obj)
            rec_d = TA._records(N, H, 1, bits, obj)
            rec_d[1]["fired"] = bits                             # master coin not fired: the sample is copied
            table = g.put(A.draw_params(None, N, H, H, explicit=rec_d, device=dev).cpu())
            recs = A.table_to_numpy(table)
            rng = g.put(A.new_rng(12, dev).cpu())
            z = TA._noise_draws(dev, img.shape, nimg, rng) if bits & A.NOISE else None
            g.check()
            gx, gy = ops.aug_apply(g.put(torch.from_numpy(img)), g.put(torch.from_numpy(lab)), table, stages, nimg, rng, A.STREAM_NOISE)
            torch.cuda.synchronize()
            _done(g)
            TA._compare(gx.cpu().numpy(), gy.cpu().numpy(), img, lab, recs, stages, nimg, z, stage in TA.EXACT, f"{stage}/{obj}/guarded")
    # the table drawn on the device: every record inside the ranges test_drawn_table_statistics_ranges_and_chain asserts (a record
    # pulled in from a guard is 0xFF bytes: every bit of `fired` set, NaN floats)
    import math
    f32 = np.float32
    hyper, H = [0.80, 0.25, 0.15, 10.0, True, 1.20, 0.10, 0.10, True, 0.50, 1.50], 32
    rng = g.put(torch.tensor([7, 3], dtype=torch.int64))
    for N, lesion in ((1, True), (3, False), (64, True), (129, False)):
        t1 = ops.aug_draw(N, rng, 2, hyper, H, H, 3 if lesion else 1, lesion)
        t2 = ops.aug_draw(N, rng, 2, hyper, H, H, 3 if lesion else 1, lesion)
        torch.cuda.synchronize()
        _done(g)
        assert tuple(t1.shape) == (N, ops.AUG_RECORD_BYTES) and torch.equal(t1, t2)
        t = A.table_to_numpy(t1)
        master = (t["fired"] & A.MASTER) != 0
        assert not t["fired"][~master].any() and not (t["fired"] >> 9).any()
        tm = t[master]
        if not lesion:                                          # ('zonal': one sequence, no channel shift)
            assert not (tm["fired"] & A.CSHIFT).any() and not (tm["gamma_ch"] >> 1).any()
            continue
        for field, bit in (("gamma_ch", A.GAMMA), ("poor_ch", A.POOR)):
            assert not (tm[field] >> 3).any() and not tm[(tm["fired"] & bit) == 0][field].any()
        if len(tm):
            assert tm["scale"].min() >= H and tm["scale"].max() <= math.ceil(f32(H * 1.20)) - 1
            for field, hi in (("tr", math.ceil(f32(H * 0.15))), ("cs", math.ceil(f32(H * 0.10)))):
                assert tm[field].min() >= 0 and tm[field].max() <= hi - 1, field
            assert set(tm[(tm["fired"] & A.CSHIFT) != 0]["cs_channel"].tolist()) <= {0, 1, 2}
            assert tm["angle_deg"].min() >= -10.0 and tm["angle_deg"].max() < 10.0
            assert tm["gamma"].min() >= 0.5 and tm["gamma"].max() < 1.5
            assert tm["noise_std"].min() >= 0.0 and tm["noise_std"].max() < f32(0.10)
            assert (tm["rot_pad"] == A.rotation_pad(H, H)).all()
            for r in tm[:16]:
                assert np.abs(r["rot"] - A.rotation_coefficients(r["angle_deg"], H, H)).max() < 1e-4


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("n", [1, 7, 13, 250, 1001, 1027])
def test_dropout_and_cast_under_guards(g, dtype, n):
    """Element counts that are no multiple of 8: the draw is a pure function of the element index, so the first n elements of a longer
    tensor's mask are the mask of the n-element tensor; the cast is torch's round-to-nearest-even."""
    rng = g.put(torch.tensor([1234, 0], dtype=torch.int64))
    x = _q(rnd((n,), 1), dtype)
    xd = g.put(x, dtype).requires_grad_(True)
    y = ops.dropout(xd, 0.25, rng, 7)
    y.backward(g.put(torch.ones(n), dtype))
    big = ops.dropout(g.put(torch.ones(n + 9), dtype), 0.25, rng, 7)
    c = ops.cast(g.put(rnd((n,), 2)), BF16) if dtype == F32 else ops.cast(g.put(x, BF16), F32)
    torch.cuda.synchronize()
    _done(g)
    keep = (big[:n] != 0).cpu()
    want = torch.where(keep, x.double() / 0.75, torch.zeros(n, dtype=torch.float64))
    assert rel_err(y, want) < TOL[dtype] and torch.equal((y != 0).cpu() | (x == 0), keep | (x == 0))
    assert torch.equal(xd.grad.cpu().float() != 0, keep) and bool(torch.isfinite(xd.grad.float()).all())
    assert torch.equal(c.cpu(), rnd((n,), 2).bfloat16() if dtype == F32 else x)


@pytest.mark.parametrize("n", [1000, 1001, 1002, 1003, 5, 3])
def test_adam_under_guards(g, n):
    """Buffers of exactly n floats (n % 4 in {0, 1, 2, 3}: the float4 body and the scalar tail), the kernel / bias / rest boundaries
    inside a float4."""
    nk, nb = (n * 2 // 5) | 1, n // 5 + 1
    lk, lb, lr, b1, b2, eps = 1e-2, 3e-2, 1e-2, 0.9, 0.999, 1e-7
    p0, gr = rnd((n,), 1), rnd((n,), 2)
    pd, gd = g.put(p0), g.put(gr)
    m, v, vh = (g.put(torch.zeros(n)) for _ in range(3))
    lr_dev, step = g.put(torch.tensor([lr])), g.put(torch.ones(1, dtype=torch.int32))
    p, mm, vv, hh = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for t in range(1, 4):
        ops.adam_amsgrad_(pd, gd, m, v, vh, nk, nb, lk, lb, 0.5, lr_dev, b1, b2, eps, step)
        ops.step_advance(step, None)
        p, mm, vv, hh = util.ref_adam_amsgrad_step(p, gr.double(), mm, vv, hh, t, nk, nb, lk, lb, 0.5, lr, b1, b2, eps)
    torch.cuda.synchronize()
    assert g.count == 0 and g.check() == 7                   # (in place: the entry point allocates nothing; seven placed buffers)
    assert int(step) == 4 and torch.equal(gd.cpu(), gr)
    errs = {k: rel_err(a, b) for k, a, b in (("p", pd, p), ("m", m, mm), ("v", v, vv), ("vhat", vh, hh))}
    print(f"adam n={n}: " + ", ".join(f"{k} {e:.3g}" for k, e in errs.items()))
    # p: the limit of test_adam_amsgrad_matches_keras_formula.  The moments (not asserted there): the kernel receives beta as a float,
    # |fl(beta) - beta| <= 2^-25 for beta in [0.5, 1), so its factor (1 - beta) is off by up to 2^-25 / (1 - beta) relative -- 3.0e-7
    # for m (beta1 = 0.9), 3.0e-5 for v and vhat (beta2 = 0.999) -- plus a few fp32 roundings of the three updates (8 * 2^-24).
    lim = {"p": 1e-5, "m": 2.0 ** -25 / (1 - b1) + 8 * 2.0 ** -24, "v": 2.0 ** -25 / (1 - b2) + 8 * 2.0 ** -24}
    lim["vhat"] = lim["v"]
    assert all(errs[k] < lim[k] for k in errs), (errs, lim)
