"""The 32x32x16 body of the tap-fused weight gradient (csrc/wgrad_tf.hip, M1_TF_MFMA32; 32 channels on both sides of the tile, waves
split by tap) against fp64, per element, at the smallest shapes at which its own logic can go wrong:

* K-tile columns 8 / 16 / 32 (W = 8, 24 / 16 / 32): every way a 16-voxel k-step splits into rows and columns;
* H = 10: the last row block of K-tiles is ragged; D = 3 with the (3,3,3) kernel: both depth halos are cut; N = 2;
* two a-tiles (C_in = 64: blockIdx.x), two concat members in one launch (blockIdx.z), stride (1,2,2);
* with and without bias sums; into fresh tensors and accumulated into pre-filled sinks with the folds queued;
* blocks with unequal K-tile counts and padding stages (M1_TF_SPLIT forces a split that does not divide the tile count).

Inputs are test_convs_at_scale._conv_inputs, the bound is util.assert_conv_close under util.CONV_A / util.CONV_R -- this file has no
tolerance of its own.  Every case asserts that the launch was wgrad_tf, and part 0 (no GPU) that tests/wgrad_plan_mirror.py sends
every shape to the tap-fused kernel with kparts == 1, the instantiations the switch selects.

The stride-(1,2,2) case is a (1,3,3) kernel: a (3,3,3) kernel with that stride never reaches wgrad_tf with 32-channel tiles -- its
three-slice input tile of 867 rows or more needs 14 LDS-DMA pieces per thread where tf_plan allows 10, the ladder sends it to
wgrad_mfma (asserted in part 0).
"""
import functools

import pytest
import torch

from util import ops, assert_conv_close, ref_conv_with_mag
from test_ops_at_scale import _gen, _randn
from test_convs_at_scale import _conv_inputs
from test_guard_bands import g, _conv_case, EW          # noqa: F401  (g: the guard-band fixture)
from wgrad_plan_mirror import wg_plan_of

BF16 = torch.bfloat16
K133, K333, ONE = (1, 3, 3), (3, 3, 3), (1, 1, 1)

# id -> (N, (D, H, W), cins, cout, k, s, switches)
CASES = {f"{kn}-w{W}": (2, (3, 10, W), (32,), 32, k, ONE, {}) for kn, k in (("k133", K133), ("k333", K333)) for W in (8, 16, 24, 32)}
CASES.update({
    "k333-cin64": (2, (3, 10, 16), (64,), 32, K333, ONE, {}),
    "k133-cin64": (2, (3, 10, 16), (64,), 32, K133, ONE, {}),
    "k133-two-members": (2, (3, 10, 16), (32, 32), 32, K133, ONE, {}),
    "k333-two-members": (2, (3, 10, 16), (32, 32), 32, K333, ONE, {}),
    "k133-s122": (2, (4, 16, 32), (64,), 32, K133, (1, 2, 2), {}),
    "k133-s122-w64": (2, (3, 20, 64), (64,), 32, K133, (1, 2, 2), {}),
    "k333-split7": (2, (3, 10, 16), (32,), 32, K333, ONE, {"M1_TF_SPLIT": 7}),      # 18 K-tiles over 7 blocks
    "k133-split5": (2, (3, 10, 16), (32,), 32, K133, ONE, {"M1_TF_SPLIT": 5}),      # 12 over 5
    "k333-split4-w32": (2, (3, 10, 32), (32,), 32, K333, ONE, {"M1_TF_SPLIT": 4}),  # 30 over 4: 8 / 8 / 7 / 7 tiles through 3 stages
})
UNEQUAL = ("k333-split7", "k133-split5", "k333-split4-w32")


# =================================================================================================================================
# part 0 (no GPU): the shapes reach the kernel under test
# =================================================================================================================================
@pytest.mark.parametrize("cid", sorted(CASES))
def test_case_lands_on_the_tap_fused_kernel_with_32_channel_tiles(cid):
    N, dims, cins, cout, k, s, sw = CASES[cid]
    entries, launches = wg_plan_of("m1_conv3d_wgrad", N, *dims, cins, cout, k, s, "bf16", switches=sw)
    assert [(r, n) for r, n, _ in launches] == [("tf-multi" if len(cins) > 1 else "tf", "wgrad_tf")], launches
    p = launches[0][2]
    assert p.kparts == 1 and p.nks == (4 if k == K133 else 2)
    wg = [e for e in entries if e["kind"] == "wg"][0]
    assert wg["grid"] == (sum(cins) // len(cins) // 32, wg["splits"], len(cins))
    if cid in UNEQUAL:
        assert p.ntiles % wg["splits"] != 0 and p.tpb > 1, (p.ntiles, wg["splits"])
    if sw == {} and s == ONE and len(cins) == 1 and cins[0] == 32:
        assert p.KWs == {8: 8, 16: 16, 24: 8, 32: 32}[dims[2]]


def test_strided_333_layers_do_not_reach_the_tap_fused_kernel():
    for W in (16, 32, 64):
        _, launches = wg_plan_of("m1_conv3d_wgrad", 2, 4, 16, W, (64,), 32, K333, (1, 2, 2), "bf16")
        assert [n for _, n, _ in launches] == ["wgrad_mfma"], launches


# =================================================================================================================================
# part 1: against fp64
# =================================================================================================================================
@functools.lru_cache(maxsize=None)
def _data(dev, cid):
    """Inputs, sink contents and the fp64 reference of a case: computed once, shared by the tests below, never modified."""
    N, dims, cins, cout, k, s, _ = CASES[cid]
    gen = _gen(dev, 4001 + sorted(CASES).index(cid))
    xs, w, b, dy = _conv_inputs(dev, BF16, N, dims, cins, cout, k, s, False, gen)
    pre = 2.0 + _randn(tuple(w.shape), gen, dev), -1.0 + _randn((cout,), gen, dev)
    ref, mag = ref_conv_with_mag(torch.cat(xs, -1), w, b, s, dy, False)
    return [x.to(BF16) for x in xs], w, b, dy.to(BF16), pre, ref, mag


def _wgrad(dev, cid, mfma32, sink, bias=True):
    """dW, db of the case through ops.conv3d_same with the 32x32x16 body on or off; sink: added into pre-filled sinks, folds queued."""
    _, _, _, _, k, s, sw = CASES[cid]
    xd, w, b, dy, pre, _, _ = _data(dev, cid)
    try:
        with ops.config(M1_TF_MFMA32=mfma32, **sw):
            wd, bd = w.clone().requires_grad_(True), (b.clone().requires_grad_(True) if bias else None)
            if sink:
                wd._m1_gsink = pre[0].clone()
                if bias:
                    bd._m1_gsink = pre[1].clone()
            y = ops.conv3d_same(xd, wd, bd, k, s)
            with ops.kernel_log() as kl:
                y.backward(dy)
                ops.fold_pending()
                torch.cuda.synchronize()
            assert [n for n in kl.names if n.startswith("wgrad")] == ["wgrad_tf"], kl.names      # (never a fallback)
            if sink:
                assert wd.grad is None
                return wd._m1_gsink, bd._m1_gsink if bias else None
            return wd.grad, bd.grad if bias else None
    finally:
        ops.drop_deferred()
        ops.invalidate_panels()


def _assert_fp64(dev, cid, got, sink, what):
    *_, pre, ref, mag = _data(dev, cid)
    for name, t, p in (("dw", got[0], pre[0]), ("db", got[1], pre[1])):
        if t is None:
            continue
        if sink:
            assert_conv_close(t, p.double() + ref[name], mag[name] + p.double().abs(), torch.float32, f"{name} (into sinks) of {what}", acc=True)
        else:
            assert_conv_close(t, ref[name], mag[name], torch.float32, f"{name} of {what}")


@pytest.mark.gpu
@pytest.mark.parametrize("cid", sorted(CASES))
def test_mfma32_body_against_fp64(dev, cid):
    for sink in (False, True):
        _assert_fp64(dev, cid, _wgrad(dev, cid, 1, sink), sink, f"{cid} M1_TF_MFMA32=1")


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["k133-w16", "k333-w24"])
def test_mfma32_body_without_bias(dev, cid):
    dw, db = _wgrad(dev, cid, 1, False, bias=False)
    assert db is None
    _assert_fp64(dev, cid, (dw, None), False, f"{cid} without bias")
    dw, _ = _wgrad(dev, cid, 1, True, bias=False)
    _assert_fp64(dev, cid, (dw, None), True, f"{cid} without bias")


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["k133-w32", "k333-w8", "k133-split5", "k333-split7", "k133-s122", "k333-two-members"])
def test_old_and_new_body_both_meet_the_bound(dev, cid):
    for on in (0, 1):
        _assert_fp64(dev, cid, _wgrad(dev, cid, on, False), False, f"{cid} M1_TF_MFMA32={on}")


@pytest.mark.gpu
@pytest.mark.parametrize("cid", sorted(CASES))
def test_new_body_equals_the_old_body_bit_for_bit(dev, cid):
    """The MFMA adds the k values of one instruction in order, and both bodies walk the voxels of a block in the same order: two
    K = 16 steps of the 32x32x16 body leave the bits of one K = 32 step of the 16x16x32 body, in dW and (ones operand) in db.  A
    training run therefore computes with the switch on what it computed with it off."""
    for sink in (False, True):
        a, b = _wgrad(dev, cid, 0, sink), _wgrad(dev, cid, 1, sink)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (cid, sink)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["k133-split5", "k333-split4-w32", "k133-two-members", "k333-cin64"])
def test_mfma32_body_twice_is_bit_equal(dev, cid):
    for sink in (False, True):
        a, b = (_wgrad(dev, cid, 1, sink) for _ in range(2))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (cid, sink)


# =================================================================================================================================
# part 2: between guard bands (the helpers of test_guard_bands.py)
# =================================================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["k133-w24", "k333-w16"])
def test_mfma32_body_under_guards(g, cid):
    N, dims, cins, cout, k, s, sw = CASES[cid]

    def tap_fused(kl, sink):
        if sink:          # (queued: the kernel is pinned on the fresh run, as in test_guard_bands._tf_case)
            return
        assert [n for n in kl.names if n.startswith("wgrad")] == ["wgrad_tf"], kl.names

    seen = _conv_case(g, False, k, s, cins, cout, (N, *dims), BF16, [(dict(M1_TF_MFMA32=1, **sw), tap_fused)], EW, False, 61, f"mfma32 {cid}")
    assert "wgrad_tf" in seen
