"""Every convolution call of the C3 bench step (forward, data gradient, weight / bias gradient, the conv1 || conv4 pair, the fused
InstanceNorm-backward epilogue) against a plain fp64 reference on the same device: per element, on the whole volume.

* part 0 (no GPU): util.ref_conv3d_same / ref_conv3d_transpose_same and their autograd gradients equal oracle/m1_oracle.py; the
  magnitude helper equals a brute-force loop; the bound rejects a weight tensor that lost one 8-channel chunk of one tap at K = 13,824.
* part 1: the table of conv calls of one forward + backward of the C3 bench configuration (C3_CONV_KEYS), kept current by a recorder
  that wraps the library's nine conv entry points, plus EXTRA_CONV_KEYS for routes only other workloads reach.
* part 2: one test per key through the ops entry points at the production switches, asserting first that the kernels launched are
  the kernels the key names.

The bound (util.assert_conv_close): per element |got - ref| <= a*|ref| + r*mag, mag = the sum of |terms| behind the element (the
reference evaluated on |x|, |w|, |b|, |dy|; plus |slot| where a kernel adds into a gradient slot that holds a value).  No element is
left out: mag > 0 everywhere for these inputs.  Neither constant is fitted to what the kernels produce:

* a -- the rounding of the STORED result.  bf16 (8 significant bits): one round-to-nearest moves a value by at most half the spacing of
  its binade, 2^-8 of the value (1 + 2^-8 lies midway between its neighbours 1 and 1 + 2^-7; test_bf16_round_to_nearest_needs_2_pow_minus_8
  shows that the fp64 reference itself, rounded once, violates 2^-9 and meets 2^-8).  Twice that where the kernel adds into a bf16 slot
  that already holds a value: the kernels round their own gradient to bf16 and then the sum, so the two roundings are bounded by
  a * (|dx| + |slot + dx|), both from the reference (a * 2|ref| would miss sums that cancel; the slot's value is a term of mag).  A
  forward that the dispatch splits into several launches over groups of concat members (conv_halo: up to five for five members; a
  transposed conv with a thin latent member: two) does the same per launch with its bf16 output as the slot:
  a * (|ref| + sum of the members' |contributions| + sum of |member-prefix sums|), all from the reference.  (Found by this module: the
  output of such a layer carries two roundings per launch, not one.)  fp32 results (fp32 activations, every
  weight and bias gradient): 4 * 2^-24 -- the final conversion, the bias add and the fold of partial copies.
* r = 1e-5 -- fp32 accumulation of exact products (bf16 x bf16 products are exact in fp32; operands are rounded to the storage type
  before both sides see them).  The project's figure for fp32 reductions (test_ops_at_scale.RED).  A sum of K terms accumulated in
  fp32 in blocks (MFMA accumulators over 16- or 32-deep chunks, K groups added through LDS, split-K slabs and per-split partial copies
  folded in fp32) carries an error of about sqrt(K) * 2^-24 * rms-partial-sum in the random-walk model and at most depth * 2^-24 * mag
  along the longest chain of dependent additions; that chain is K / 16 MFMA steps (864 at K = 13,824: 5e-5 * mag worst case, never
  approached because the partial sums stay far below mag), and the blocked paths only shorten it.  The weight gradients sum up to 10^6
  voxels, but in tiles of voxels per block and per split, folded pairwise: the same argument with K = voxels per split.  So 1e-5 holds
  for every path of the table and no path gets a wider figure; the worst case K * 2^-24 (8e-4 at K = 13,824) is not used anywhere.

Sensitivity: with unit-variance operands a term has E|t| = 2/pi = 0.64, mag is about 0.64 * K * sigma_term and the output's rms is
sqrt(K) * sigma_term, so r*mag = 0.64 * sqrt(K) * r of rms: 7.5e-4 at K = 13,824, 1.1e-4 at K = 288.  A lost chunk of c channels of one
tap moves an output by sqrt(c / K) of rms (2.4 % at c = 8, K = 13,824): with a*|ref| = 0.4 % of |ref| that exceeds the bound on most
elements for every c >= 8 at every layer of the model (test_bound_rejects_a_lost_chunk_of_8_channels_at_the_largest_k).

Inputs: x and dy carry a mean and the slow D / H ramp of test_ops_at_scale._ramp, so that the weight- and bias-gradient sums do not
cancel: the median of mag / |ref| over dW is asserted below DW_CANCEL (chosen on the reference alone, on the CPU, at a scaled-down
shape: E|x||dy| / (E x E dy + the ramps' correlation) is about 4 for these means; 8 leaves room for the noise of a few thousand voxels).
"""
import re
import zlib

import numpy as np
import pytest
import torch

from oracle import m1_oracle as O
import util
from util import PKG, ops, assert_conv_close, ref_conv_with_mag
from test_ops_at_scale import _as, _gen, _ramp, _randn, _assert_stats, _same, _inbwd_case

L = PKG.hip.lib
DW_CANCEL = 8.0
_DT = {"bf16": torch.bfloat16, "fp32": torch.float32}


# =================================================================================================================================
# part 0: the references against the CPU oracle (no GPU)
# =================================================================================================================================
REF_KS = [(k, s) for k in ((1, 1, 1), (1, 3, 3), (3, 3, 3)) for s in ((1, 1, 1), (1, 2, 2), (2, 2, 2))]
REF_DIMS = [(3, 5, 7), (4, 6, 8), (1, 6, 5)]            # odd extents, even extents, extent 1 along D


def _grads(fn, ins, dy):
    ins = [t.clone().double().requires_grad_(True) for t in ins]
    y = fn(*ins)
    y.backward(dy.double())
    return y.detach(), [t.grad for t in ins]


@pytest.mark.parametrize("dims", REF_DIMS)
@pytest.mark.parametrize("k,s", REF_KS)
def test_reference_conv_matches_oracle(k, s, dims):
    N, cin, cout = 2, 5, 4
    x, w, b = util.rnd((N, *dims, cin), 1), util.rnd((*k, cin, cout), 2), util.rnd((cout,), 3)
    yo = O.conv3d_same(x.double(), w.double(), b.double(), s)
    dy = util.rnd(tuple(yo.shape), 4)
    yo, go = _grads(lambda *a: O.conv3d_same(*a, s), [x, w, b], dy)
    yr, gr = _grads(lambda *a: util.ref_conv3d_same(*a, s), [x, w, b], dy)
    _same(yr, yo)
    for a_, b_ in zip(gr, go):
        _same(a_, b_)


@pytest.mark.parametrize("dims", REF_DIMS)
@pytest.mark.parametrize("k,s", REF_KS)
def test_reference_conv_transpose_matches_oracle(k, s, dims):
    N, cin, cout = 2, 5, 4
    x, w, b = util.rnd((N, *dims, cin), 1), util.rnd((*k, cout, cin), 2), util.rnd((cout,), 3)
    yo = O.conv3d_transpose_same(x.double(), w.double(), b.double(), s)
    dy = util.rnd(tuple(yo.shape), 4)
    yo, go = _grads(lambda *a: O.conv3d_transpose_same(*a, s), [x, w, b], dy)
    yr, gr = _grads(lambda *a: util.ref_conv3d_transpose_same(*a, s), [x, w, b], dy)
    _same(yr, yo)
    for a_, b_ in zip(gr, go):
        _same(a_, b_)


@pytest.mark.parametrize("transposed", [False, True])
def test_magnitude_helper_matches_brute_force(transposed):
    """Sum of |terms| behind y, dx, dw and db at one tiny shape, by a loop over every (output voxel, tap, ci, co)."""
    N, dims, cin, cout, k, s = 2, (2, 3, 4), 3, 2, (1, 3, 3), (1, 2, 2)
    x = util.rnd((N, *dims, cin), 1).double()
    w = util.rnd((*k, cout, cin) if transposed else (*k, cin, cout), 2).double()
    b = util.rnd((cout,), 3).double()
    odims = [n * st for n, st in zip(dims, s)] if transposed else [-(-n // st) for n, st in zip(dims, s)]
    dy = util.rnd((N, *odims, cout), 4).double()
    ref, mag = ref_conv_with_mag(x, w, b, s, dy, transposed)
    my, mx, mw = torch.zeros_like(ref["y"]), torch.zeros_like(x), torch.zeros_like(w)
    big, small = (odims, dims) if transposed else (dims, odims)        # the strided side is `small`
    pads = [max(kk - st, 0) // 2 for kk, st in zip(k, s)] if transposed else [util.same_pads(n, kk, st)[1] for n, kk, st in zip(dims, k, s)]
    for n in range(N):
        for i in np.ndindex(*small):
            for t in np.ndindex(*k):
                j = tuple(ii * st + tt - p for ii, st, tt, p in zip(i, s, t, pads))
                if any(v < 0 or v >= m for v, m in zip(j, big)):
                    continue
                xi, yi = ((n, *i), (n, *j)) if transposed else ((n, *j), (n, *i))
                for ci in range(cin):
                    for co in range(cout):
                        wv = w[(*t, co, ci)] if transposed else w[(*t, ci, co)]
                        wi = (*t, co, ci) if transposed else (*t, ci, co)
                        my[(*yi, co)] += (x[(*xi, ci)] * wv).abs()
                        mx[(*xi, ci)] += (dy[(*yi, co)] * wv).abs()
                        mw[wi] += (x[(*xi, ci)] * dy[(*yi, co)]).abs()
    _same(mag["y"], my + b.abs())
    _same(mag["dx"], mx)
    _same(mag["dw"], mw)
    _same(mag["db"], dy.abs().sum(dim=(0, 1, 2, 3)))
    for key in ("y", "dx", "dw", "db"):
        assert bool((mag[key] >= ref[key].abs() - 1e-12).all())


def test_bf16_round_to_nearest_needs_2_pow_minus_8():
    """The constant a for bf16 results comes from the number format: a reference rounded ONCE to bf16 (the best any kernel can store)
    stays inside 2^-8 |ref| everywhere and leaves 2^-9 |ref| on a large share of the elements."""
    ref = util.rnd((4096,), 5).double()
    d = (ref.to(torch.bfloat16).double() - ref).abs()
    assert bool((d <= 2.0 ** -8 * ref.abs()).all())
    assert float((d > 2.0 ** -9 * ref.abs()).double().mean()) > 0.2
    assert util.CONV_A[torch.bfloat16] == 2.0 ** -8 and util.CONV_R == 1e-5


def _conv_inputs(dev, dtype, N, dims, cins, cout, k, s, transposed, g):
    """x members, w, b, dy as the kernels read them (rounded to the storage type; w is read in the activation type), with means and the
    D / H ramp on x and dy."""
    cin = sum(cins)
    xs = [_as(_randn((N, *dims, c), g, dev) + 0.5 + _ramp((N, *dims, c), dev), dtype) for c in cins]
    K = cin * k[0] * k[1] * k[2]
    w = _as(_randn((*k, cout, cin) if transposed else (*k, cin, cout), g, dev, 1.0 / K ** 0.5), dtype)
    b = 0.1 * _randn((cout,), g, dev)
    odims = [n * st for n, st in zip(dims, s)] if transposed else [-(-n // st) for n, st in zip(dims, s)]
    dy = _as(_randn((N, *odims, cout), g, dev) + 0.3 + _ramp((N, *odims, cout), dev), dtype)
    return xs, w, b, dy


def test_bound_rejects_a_lost_chunk_of_8_channels_at_the_largest_k():
    """The sensitivity the bound buys, on the reference alone: K = 27 * 512 = 13,824 (res4, scaled down in voxels, not in K), one
    8-channel chunk of one tap removed from w.  The damaged result, stored as well as bf16 allows, is rejected on most elements; the
    undamaged one passes; the weight-gradient sums of these inputs do not cancel."""
    cpu = torch.device("cpu")
    N, dims, cins, cout, k, s = 1, (3, 4, 4), [512], 16, (3, 3, 3), (1, 1, 1)
    xs, w, b, dy = _conv_inputs(cpu, torch.bfloat16, N, dims, cins, cout, k, s, False, _gen(cpu, 3))
    ref, mag = ref_conv_with_mag(xs[0], w, b, s, dy)
    assert_conv_close(ref["y"].to(torch.bfloat16), ref["y"], mag["y"], torch.bfloat16, "undamaged y")
    wb = w.clone()
    wb[1, 1, 1, 256:264, :] = 0
    bad = util.ref_conv3d_same(xs[0], wb, b, s)
    with pytest.raises(AssertionError, match="elements outside"):
        assert_conv_close(bad.to(torch.bfloat16), ref["y"], mag["y"], torch.bfloat16, "lost chunk y")
    out = (bad - ref["y"]).abs() > util.CONV_A[torch.bfloat16] * ref["y"].abs() + util.CONV_R * mag["y"]
    interior = out[:, 1:-1, 1:-1, 1:-1]                       # (every interior output reads the damaged tap)
    assert float(interior.double().mean()) > 0.5, float(interior.double().mean())
    # r * mag against the output's rms: 0.64 * sqrt(K) * r, within the spread the non-zero means add
    ratio = float((util.CONV_R * mag["y"]).mean() / ref["y"].std())
    assert 0.5 * 7.5e-4 < ratio < 3 * 7.5e-4, ratio
    assert float((mag["dw"] / ref["dw"].abs()).median()) < DW_CANCEL


# =================================================================================================================================
# part 1: the table of the bench step's conv calls
# =================================================================================================================================
ENTRY_POINTS = ("m1_conv3d_fwd", "m1_convT3d_fwd", "m1_conv3d_dgrad", "m1_conv3d_dgrad_inbwd", "m1_convT3d_dgrad", "m1_conv3d_pair_fwd",
                "m1_conv3d_pair_dgrad", "m1_conv3d_wgrad", "m1_convT3d_wgrad")


def _flags(ptrs, accs, n):
    need = tuple(1 if ptrs[i] else 0 for i in range(n))
    return f"need={need},acc={tuple(int(accs[i]) if need[i] else 0 for i in range(n))}"


def conv_key(name, args, kernels, defer, nparts=None):
    """(entry point, N, D, H, W, members' channels, Cout or (c1, c4), k, s, dtype, flags, kernels) of one call of a conv entry point
    of the library: everything its dispatch decides on, and the kernels it launched."""
    d = args[0]._obj                                        # (ctypes.byref(desc))
    cins = tuple(int(d.src[i].C) for i in range(d.nsrc))
    cout = int(d.Cout)
    if name == "m1_conv3d_fwd":
        fl = f"stats={int(bool(args[4]))}"
    elif name == "m1_convT3d_fwd":
        fl = ""
    elif name in ("m1_conv3d_dgrad", "m1_convT3d_dgrad"):
        fl = _flags(args[3], args[4], d.nsrc)
    elif name == "m1_conv3d_dgrad_inbwd":
        fl = f"fused={int(nparts > 0)}"
    elif name == "m1_conv3d_pair_fwd":
        cout = (int(args[5]), cout - int(args[5])); fl = "stats=1"
    elif name == "m1_conv3d_pair_dgrad":
        cout = (int(args[3]), cout - int(args[3])); fl = _flags(args[6], args[7], d.nsrc)
    else:
        fl = f"acc={int(args[5])},bias={int(bool(args[3]))},defer={int(defer)}"
    return (name, int(d.N), int(d.D), int(d.H), int(d.W), cins, cout, (int(d.kd), int(d.kh), int(d.kw)), (int(d.sd), int(d.sh), int(d.sw)),
            "bf16" if d.dtype == L.M1_BF16 else "fp32", fl, "+".join(kernels))


class conv_recorder:
    """``with conv_recorder(monkeypatch) as rec: ...; rec.keys`` -- the conv_key of every call of the nine conv entry points inside the
    block (the attributes of the loaded library object are wrapped; weight gradients queued by ops reach the wrappers when
    ops._run_deferred_wgrads launches them).  ``rec.calls`` counts the calls."""

    def __init__(self, monkeypatch):
        self.cm = monkeypatch.context()
        self.keys, self.calls, self.defer = set(), 0, 0

    def __enter__(self):
        self.mp = self.cm.__enter__()                       # (a context of its own: leaving it undoes the recorder's patches only)
        lib = L.load()
        defer0 = lib.m1_wgrad_defer

        def defer(on, _fn=defer0):
            self.defer = int(on)
            return _fn(on)
        self.mp.setattr(lib, "m1_wgrad_defer", defer)
        for name in ENTRY_POINTS:
            fn = getattr(lib, name)

            def wrap(*args, _fn=fn, _name=name):
                lib.m1_debug_kernels(1)
                try:
                    rc = _fn(*args)
                finally:
                    raw = lib.m1_debug_kernels(0)
                kernels = [n for n in (raw.decode() if raw else "").split(",") if n]
                nparts = int(args[11]._obj.value) if _name == "m1_conv3d_dgrad_inbwd" else None
                self.keys.add(conv_key(_name, args, kernels, self.defer, nparts))
                self.calls += 1
                return rc
            self.mp.setattr(lib, name, wrap)
        return self

    def __exit__(self, *exc):
        return self.cm.__exit__(*exc)


def record_c3_bench_conv_keys(dev, monkeypatch):
    """One forward + backward of the C3 bench configuration, as test_ops_at_scale.record_c3_bench_keys drives it."""
    from test_ops_at_scale import record_c3_bench_keys
    with conv_recorder(monkeypatch) as rec:
        record_c3_bench_keys(dev, monkeypatch)
        ops.fold_pending()
        torch.cuda.synchronize()
    return rec.keys, rec.calls


# (entry point, N, D, H, W, members' channels, Cout or (c1, c4), k, s, dtype, flags, kernels launched) of every call of the library's conv
# entry points in one forward + backward of the C3 bench configuration (bf16, batch 2, stacked to 4 where the passes are stacked); D, H, W
# are those of the conv's INPUT (the low-resolution side of a transposed conv).  Flags: stats = fused InstanceNorm statistics asked for;
# need / acc = per-member need mask and accumulate flags of a data gradient; fused = the IN-backward epilogue emitted its sums; acc, bias,
# defer = accumulate flag of a weight gradient, bias gradient asked for, m1_wgrad_defer on.  test_c3_bench_conv_keys_are_in_the_table
# keeps it current.
C3_CONV_KEYS = [
    ('m1_conv3d_dgrad', 2, 20, 160, 160, (32, 32, 32, 32, 32, 32), 32, (1, 3, 3), (1, 1, 1), 'bf16', 'need=(1, 1, 1, 1, 1, 1),acc=(1, 1, 1, 1, 1, 1)', 'conv_halo:bn32+conv_halo:bn32+conv_halo:bn32+conv_halo:bn32+conv_halo:bn32+conv_halo:bn32'),
    ('m1_conv3d_dgrad', 2, 20, 160, 160, (32, 32, 32, 32, 32, 32), 8, (1, 3, 3), (1, 1, 1), 'bf16', 'need=(1, 1, 1, 1, 1, 1),acc=(0, 0, 0, 0, 0, 0)', 'conv_halo:bn32+conv_halo:bn32+conv_halo:bn32+conv_halo:bn32+conv_halo:bn32+conv_halo:bn32'),
    ('m1_conv3d_dgrad', 2, 20, 160, 160, (32,), 16, (1, 3, 3), (1, 2, 2), 'bf16', 'need=(1,),acc=(0,)', 'conv_halo_cls:bn32'),
    ('m1_conv3d_dgrad', 2, 20, 160, 160, (32,), 16, (1, 3, 3), (1, 2, 2), 'bf16', 'need=(1,),acc=(1,)', 'conv_halo_cls:bn32'),
    ('m1_conv3d_dgrad', 2, 20, 160, 160, (32,), 2, (1, 1, 1), (1, 1, 1), 'bf16', 'need=(1,),acc=(0,)', 'thin_pw_dgrad'),
    ('m1_conv3d_dgrad', 2, 20, 160, 160, (32,), 32, (1, 1, 1), (1, 1, 1), 'bf16', 'need=(1,),acc=(0,)', 'conv_pw:bn32'),
    ('m1_conv3d_dgrad', 2, 20, 160, 160, (32,), 32, (1, 1, 1), (1, 1, 1), 'bf16', 'need=(1,),acc=(1,)', 'conv_pw:bn32'),
    ('m1_conv3d_dgrad', 2, 20, 160, 160, (32,), 64, (1, 3, 3), (1, 2, 2), 'bf16', 'need=(1,),acc=(1,)', 'conv_halo_cls:bn32'),
    ('m1_conv3d_dgrad', 2, 20, 80, 80, (64, 64, 64, 64), 16, (1, 3, 3), (1, 1, 1), 'bf16', 'need=(1, 1, 1, 1),acc=(1, 1, 1, 1)', 'conv_halo:bn32+conv_halo:bn32+conv_halo:bn32+conv_halo:bn32'),
    ('m1_conv3d_dgrad', 2, 20, 80, 80, (64, 64, 64, 64), 64, (1, 3, 3), (1, 1, 1), 'bf16', 'need=(1, 1, 1, 1),acc=(1, 1, 1, 1)', 'conv_halo:bn32+conv_halo:bn32+conv_halo:bn32+conv_halo:bn32'),
    ('m1_conv3d_dgrad', 2, 20, 80, 80, (64, 64, 64, 64, 64), 16, (1, 3, 3), (1, 1, 1), 'bf16', 'need=(1, 1, 1, 1, 1),acc=(0, 0, 0, 0, 0)', 'conv_halo:bn32+conv_halo:bn32+conv_halo:bn32+conv_halo:bn32+conv_halo:bn32'),
    ('m1_conv3d_dgrad', 2, 20, 80, 80, (64, 64, 64, 64, 64), 64, (1, 3, 3), (1, 1, 1), 'bf16', 'need=(1, 1, 1, 1, 1),acc=(1, 1, 1, 1, 1)', 'conv_halo:bn32+conv_halo:bn32+conv_halo:bn32+conv_halo:bn32+conv_halo:bn32'),
    ('m1_conv3d_dgrad', 2, 20, 80, 80, (64,), 64, (1, 1, 1), (1, 1, 1), 'bf16', 'need=(1,),acc=(0,)', 'conv_pw:bn32'),
    ('m1_conv3d_dgrad', 2, 20, 80, 80, (64,), 64, (1, 1, 1), (1, 1, 1), 'bf16', 'need=(1,),acc=(1,)', 'conv_pw:bn32'),
    ('m1_conv3d_dgrad', 2, 5, 10, 10, (512,), 32, (1, 1, 1), (1, 1, 1), 'bf16', 'need=(1,),acc=(1,)', 'conv_mfma:64x128:w4:ks1'),
    ('m1_conv3d_dgrad', 2, 5, 10, 10, (512,), 64, (1, 1, 1), (1, 1, 1), 'bf16', 'need=(1,),acc=(1,)', 'conv_mfma:64x128:w4:ks1'),
    ('m1_conv3d_dgrad', 4, 10, 20, 20, (256,), 256, (1, 1, 1), (1, 1, 1), 'bf16', 'need=(1,),acc=(0,)', 'conv_mfma:128x128:w8:ks1'),
    ('m1_conv3d_dgrad', 4, 10, 20, 20, (256,), 256, (1, 1, 1), (1, 1, 1), 'bf16', 'need=(1,),acc=(1,)', 'conv_mfma:128x128:w8:ks1'),
    ('m1_conv3d_dgrad', 4, 10, 20, 20, (256,), 4, (1, 1, 1), (1, 1, 1), 'bf16', 'need=(1,),acc=(1,)', 'thin_pw_dgrad'),
    ('m1_conv3d_dgrad', 4, 20, 40, 40, (128,), 128, (1, 1, 1), (1, 1, 1), 'bf16', 'need=(1,),acc=(0,)', 'conv_mfma:128x128:w8:ks1'),
    ('m1_conv3d_dgrad', 4, 20, 40, 40, (128,), 128, (1, 1, 1), (1, 1, 1), 'bf16', 'need=(1,),acc=(1,)', 'conv_mfma:128x128:w8:ks1'),
    ('m1_conv3d_dgrad', 4, 20, 40, 40, (128,), 2, (1, 1, 1), (1, 1, 1), 'bf16', 'need=(1,),acc=(0,)', 'thin_pw_dgrad'),
    ('m1_conv3d_dgrad', 4, 20, 40, 40, (128,), 2, (1, 1, 1), (1, 1, 1), 'bf16', 'need=(1,),acc=(1,)', 'thin_pw_dgrad'),
    ('m1_conv3d_dgrad', 4, 5, 10, 10, (512,), 128, (1, 1, 1), (1, 1, 1), 'bf16', 'need=(1,),acc=(1,)', 'conv_mfma:64x128:w4:ks1'),
    ('m1_conv3d_dgrad', 4, 5, 10, 10, (512,), 256, (1, 1, 1), (1, 1, 1), 'bf16', 'need=(1,),acc=(1,)', 'conv_mfma:64x128:w4:ks1'),
    ('m1_conv3d_dgrad', 4, 5, 10, 10, (512,), 6, (1, 1, 1), (1, 1, 1), 'bf16', 'need=(1,),acc=(1,)', 'thin_pw_dgrad'),
    ('m1_conv3d_dgrad_inbwd', 2, 20, 160, 160, (8,), 32, (1, 1, 1), (1, 1, 1), 'bf16', 'fused=1', 'conv_pw:bn16'),
    ('m1_conv3d_dgrad_inbwd', 2, 20, 160, 160, (8,), 8, (3, 3, 3), (1, 1, 1), 'bf16', 'fused=1', 'conv_halo:bn16'),
    ('m1_conv3d_dgrad_inbwd', 2, 20, 40, 40, (32,), 128, (1, 1, 1), (1, 1, 1), 'bf16', 'fused=1', 'conv_mfma:128x32:w8:ks1'),
    ('m1_conv3d_dgrad_inbwd', 2, 20, 40, 40, (32,), 32, (3, 3, 3), (1, 1, 1), 'bf16', 'fused=1', 'conv_mfma:128x32:w8:ks1'),
    ('m1_conv3d_dgrad_inbwd', 2, 20, 80, 80, (16,), 16, (3, 3, 3), (1, 1, 1), 'bf16', 'fused=1', 'conv_halo:bn16'),
    ('m1_conv3d_dgrad_inbwd', 2, 20, 80, 80, (16,), 64, (1, 1, 1), (1, 1, 1), 'bf16', 'fused=1', 'conv_pw:bn16'),
    ('m1_conv3d_dgrad_inbwd', 4, 10, 20, 20, (64,), 256, (1, 1, 1), (1, 1, 1), 'bf16', 'fused=1', 'conv_mfma:64x64:w4:ks1'),
    ('m1_conv3d_dgrad_inbwd', 4, 10, 20, 20, (64,), 64, (3, 3, 3), (1, 1, 1), 'bf16', 'fused=1', 'conv_mfma:64x64:w4:ks1:kg3'),
    ('m1_conv3d_dgrad_inbwd', 4, 20, 40, 40, (32,), 128, (1, 1, 1), (1, 1, 1), 'bf16', 'fused=1', 'conv_mfma:128x32:w8:ks1'),
    ('m1_conv3d_dgrad_inbwd', 4, 20, 40, 40, (32,), 32, (3, 3, 3), (1, 1, 1), 'bf16', 'fused=1', 'conv_mfma:128x32:w8:ks1'),
    ('m1_conv3d_dgrad_inbwd', 4, 5, 10, 10, (128,), 128, (3, 3, 3), (1, 1, 1), 'bf16', 'fused=1', 'conv_mfma:64x128:w4:ks13'),
    ('m1_conv3d_dgrad_inbwd', 4, 5, 10, 10, (128,), 512, (1, 1, 1), (1, 1, 1), 'bf16', 'fused=1', 'conv_mfma:64x128:w4:ks2'),
    ('m1_conv3d_fwd', 2, 20, 160, 160, (2,), 32, (1, 3, 3), (1, 1, 1), 'bf16', 'stats=1', 'thin_fwd'),
    ('m1_conv3d_fwd', 2, 20, 160, 160, (3,), 32, (1, 3, 3), (1, 1, 1), 'bf16', 'stats=1', 'thin_fwd'),
    ('m1_conv3d_fwd', 2, 20, 160, 160, (32, 32, 32, 32, 32, 32), 32, (1, 3, 3), (1, 1, 1), 'bf16', 'stats=1', 'conv_halo:bn32+conv_halo:bn32+conv_halo:bn32'),
    ('m1_conv3d_fwd', 2, 20, 160, 160, (32, 32, 32, 32, 32, 32), 8, (1, 3, 3), (1, 1, 1), 'bf16', 'stats=1', 'conv_halo:bn16+conv_halo:bn16+conv_halo:bn16'),
    ('m1_conv3d_fwd', 2, 20, 160, 160, (32,), 16, (1, 3, 3), (1, 2, 2), 'bf16', 'stats=1', 'conv_halo:bn16'),
    ('m1_conv3d_fwd', 2, 20, 160, 160, (32,), 2, (1, 1, 1), (1, 1, 1), 'bf16', 'stats=0', 'conv_pw:bn16'),
    ('m1_conv3d_fwd', 2, 20, 160, 160, (32,), 32, (1, 1, 1), (1, 1, 1), 'bf16', 'stats=0', 'conv_pw:bn32'),
    ('m1_conv3d_fwd', 2, 20, 160, 160, (32,), 32, (1, 1, 1), (1, 1, 1), 'bf16', 'stats=1', 'conv_pw:bn32'),
    ('m1_conv3d_fwd', 2, 20, 160, 160, (32,), 64, (1, 3, 3), (1, 2, 2), 'bf16', 'stats=1', 'conv_halo:bn32'),
    ('m1_conv3d_fwd', 2, 20, 160, 160, (8,), 32, (1, 1, 1), (1, 1, 1), 'bf16', 'stats=1', 'conv_pw:bn32'),
    ('m1_conv3d_fwd', 2, 20, 160, 160, (8,), 8, (3, 3, 3), (1, 1, 1), 'bf16', 'stats=1', 'conv_halo:bn16'),
    ('m1_conv3d_fwd', 2, 20, 40, 40, (32,), 128, (1, 1, 1), (1, 1, 1), 'bf16', 'stats=1', 'conv_pw:bn32'),
    ('m1_conv3d_fwd', 2, 20, 40, 40, (32,), 32, (3, 3, 3), (1, 1, 1), 'bf16', 'stats=1', 'conv_mfma:128x32:w8:ks1'),
    ('m1_conv3d_fwd', 2, 20, 80, 80, (16,), 16, (3, 3, 3), (1, 1, 1), 'bf16', 'stats=1', 'conv_halo:bn16'),
    ('m1_conv3d_fwd', 2, 20, 80, 80, (16,), 64, (1, 1, 1), (1, 1, 1), 'bf16', 'stats=1', 'conv_pw:bn32'),
    ('m1_conv3d_fwd', 2, 20, 80, 80, (64, 64, 64, 64), 16, (1, 3, 3), (1, 1, 1), 'bf16', 'stats=1', 'conv_halo:bn16+conv_halo:bn16+conv_halo:bn16+conv_halo:bn16'),
    ('m1_conv3d_fwd', 2, 20, 80, 80, (64, 64, 64, 64), 64, (1, 3, 3), (1, 1, 1), 'bf16', 'stats=1', 'conv_halo:bn32+conv_halo:bn32+conv_halo:bn32+conv_halo:bn32'),
    ('m1_conv3d_fwd', 2, 20, 80, 80, (64, 64, 64, 64, 64), 16, (1, 3, 3), (1, 1, 1), 'bf16', 'stats=1', 'conv_halo:bn16+conv_halo:bn16+conv_halo:bn16+conv_halo:bn16+conv_halo:bn16'),
    ('m1_conv3d_fwd', 2, 20, 80, 80, (64, 64, 64, 64, 64), 64, (1, 3, 3), (1, 1, 1), 'bf16', 'stats=1', 'conv_halo:bn32+conv_halo:bn32+conv_halo:bn32+conv_halo:bn32+conv_halo:bn32'),
    ('m1_conv3d_fwd', 2, 20, 80, 80, (64,), 64, (1, 1, 1), (1, 1, 1), 'bf16', 'stats=0', 'conv_pw:bn32'),
    ('m1_conv3d_fwd', 2, 20, 80, 80, (64,), 64, (1, 1, 1), (1, 1, 1), 'bf16', 'stats=1', 'conv_pw:bn32'),
    ('m1_conv3d_fwd', 2, 5, 10, 10, (512,), 32, (1, 1, 1), (1, 1, 1), 'bf16', 'stats=0', 'conv_mfma:64x32:w4:ks2'),
    ('m1_conv3d_fwd', 2, 5, 10, 10, (512,), 64, (1, 1, 1), (1, 1, 1), 'bf16', 'stats=0', 'conv_mfma:64x64:w4:ks2'),
    ('m1_conv3d_fwd', 4, 10, 20, 20, (256,), 256, (1, 1, 1), (1, 1, 1), 'bf16', 'stats=0', 'conv_mfma:128x128:w8:ks1'),
    ('m1_conv3d_fwd', 4, 10, 20, 20, (256,), 256, (1, 1, 1), (1, 1, 1), 'bf16', 'stats=1', 'conv_mfma:128x128:w8:ks1'),
    ('m1_conv3d_fwd', 4, 10, 20, 20, (256,), 4, (1, 1, 1), (1, 1, 1), 'bf16', 'stats=0', 'conv_mfma:64x16:w4:ks1'),
    ('m1_conv3d_fwd', 4, 10, 20, 20, (64,), 256, (1, 1, 1), (1, 1, 1), 'bf16', 'stats=1', 'conv_pw:bn32'),
    ('m1_conv3d_fwd', 4, 10, 20, 20, (64,), 64, (3, 3, 3), (1, 1, 1), 'bf16', 'stats=1', 'conv_mfma:64x64:w4:ks1:kg3'),
    ('m1_conv3d_fwd', 4, 20, 40, 40, (128,), 128, (1, 1, 1), (1, 1, 1), 'bf16', 'stats=0', 'conv_mfma:128x128:w8:ks1'),
    ('m1_conv3d_fwd', 4, 20, 40, 40, (128,), 128, (1, 1, 1), (1, 1, 1), 'bf16', 'stats=1', 'conv_mfma:128x128:w8:ks1'),
    ('m1_conv3d_fwd', 4, 20, 40, 40, (128,), 2, (1, 1, 1), (1, 1, 1), 'bf16', 'stats=0', 'conv_mfma:128x16:w4:ks1'),
    ('m1_conv3d_fwd', 4, 20, 40, 40, (32,), 128, (1, 1, 1), (1, 1, 1), 'bf16', 'stats=1', 'conv_pw:bn32'),
    ('m1_conv3d_fwd', 4, 20, 40, 40, (32,), 32, (3, 3, 3), (1, 1, 1), 'bf16', 'stats=1', 'conv_mfma:128x32:w8:ks1'),
    ('m1_conv3d_fwd', 4, 5, 10, 10, (128,), 128, (3, 3, 3), (1, 1, 1), 'bf16', 'stats=1', 'conv_mfma:64x128:w4:ks13'),
    ('m1_conv3d_fwd', 4, 5, 10, 10, (128,), 512, (1, 1, 1), (1, 1, 1), 'bf16', 'stats=1', 'conv_mfma:64x128:w4:ks1'),
    ('m1_conv3d_fwd', 4, 5, 10, 10, (512,), 128, (1, 1, 1), (1, 1, 1), 'bf16', 'stats=0', 'conv_mfma:64x128:w4:ks2'),
    ('m1_conv3d_fwd', 4, 5, 10, 10, (512,), 256, (1, 1, 1), (1, 1, 1), 'bf16', 'stats=0', 'conv_mfma:64x128:w4:ks2'),
    ('m1_conv3d_fwd', 4, 5, 10, 10, (512,), 6, (1, 1, 1), (1, 1, 1), 'bf16', 'stats=0', 'conv_mfma:64x16:w4:ks2'),
    ('m1_conv3d_pair_dgrad', 2, 20, 40, 40, (128, 128, 128), (32, 128), (3, 3, 3), (1, 1, 1), 'bf16', 'need=(1, 1, 1),acc=(1, 1, 1)', 'conv_t3:bn192:ks1'),
    ('m1_conv3d_pair_dgrad', 4, 10, 20, 20, (256, 256), (64, 256), (3, 3, 3), (1, 1, 1), 'bf16', 'need=(1, 1),acc=(1, 1)', 'conv_t3:bn128:ks1'),
    ('m1_conv3d_pair_dgrad', 4, 10, 20, 20, (256, 256, 256), (64, 256), (3, 3, 3), (1, 1, 1), 'bf16', 'need=(1, 1, 1),acc=(0, 0, 0)', 'conv_t3:bn192:ks1'),
    ('m1_conv3d_pair_dgrad', 4, 10, 20, 20, (256,), (128, 512), (3, 3, 3), (2, 2, 2), 'bf16', 'need=(1,),acc=(1,)', 'conv_mfma:128x128:w8:ks1'),
    ('m1_conv3d_pair_dgrad', 4, 20, 40, 40, (128, 128, 128, 128), (32, 128), (3, 3, 3), (1, 1, 1), 'bf16', 'need=(1, 1, 1, 1),acc=(0, 0, 0, 0)', 'conv_t3:bn256:ks1'),
    ('m1_conv3d_pair_dgrad', 4, 20, 40, 40, (128,), (64, 256), (3, 3, 3), (2, 2, 2), 'bf16', 'need=(1,),acc=(1,)', 'conv_mfma:128x128:w8:ks1'),
    ('m1_conv3d_pair_dgrad', 4, 20, 80, 80, (64,), (32, 128), (3, 3, 3), (1, 2, 2), 'bf16', 'need=(1,),acc=(0,)', 'conv_mfma:128x64:w8:ks1'),
    ('m1_conv3d_pair_dgrad', 4, 20, 80, 80, (64,), (32, 128), (3, 3, 3), (1, 2, 2), 'bf16', 'need=(1,),acc=(1,)', 'conv_mfma:128x64:w8:ks1'),
    ('m1_conv3d_pair_fwd', 2, 20, 40, 40, (128, 128, 128), (32, 128), (3, 3, 3), (1, 1, 1), 'bf16', 'stats=1', 'conv_t3:bn160:ks1'),
    ('m1_conv3d_pair_fwd', 4, 10, 20, 20, (256, 256), (64, 256), (3, 3, 3), (1, 1, 1), 'bf16', 'stats=1', 'conv_t3:bn160:ks2'),
    ('m1_conv3d_pair_fwd', 4, 10, 20, 20, (256, 256, 256), (64, 256), (3, 3, 3), (1, 1, 1), 'bf16', 'stats=1', 'conv_t3:bn160:ks2'),
    ('m1_conv3d_pair_fwd', 4, 10, 20, 20, (256,), (128, 512), (3, 3, 3), (2, 2, 2), 'bf16', 'stats=1', 'conv_mfma:64x128:w4:ks4'),
    ('m1_conv3d_pair_fwd', 4, 20, 40, 40, (128, 128, 128, 128), (32, 128), (3, 3, 3), (1, 1, 1), 'bf16', 'stats=1', 'conv_t3:bn160:ks1'),
    ('m1_conv3d_pair_fwd', 4, 20, 40, 40, (128,), (64, 256), (3, 3, 3), (2, 2, 2), 'bf16', 'stats=1', 'conv_mfma:128x160:w4:ks3'),
    ('m1_conv3d_pair_fwd', 4, 20, 80, 80, (64,), (32, 128), (3, 3, 3), (1, 2, 2), 'bf16', 'stats=1', 'conv_mfma:128x160:w4:ks1'),
    ('m1_conv3d_wgrad', 2, 20, 160, 160, (2,), 32, (1, 3, 3), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tf'),
    ('m1_conv3d_wgrad', 2, 20, 160, 160, (3,), 32, (1, 3, 3), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tf'),
    ('m1_conv3d_wgrad', 2, 20, 160, 160, (32, 32, 32, 32, 32, 32), 32, (1, 3, 3), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tf'),
    ('m1_conv3d_wgrad', 2, 20, 160, 160, (32, 32, 32, 32, 32, 32), 8, (1, 3, 3), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tf'),
    ('m1_conv3d_wgrad', 2, 20, 160, 160, (32,), 16, (1, 3, 3), (1, 2, 2), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tf'),
    ('m1_conv3d_wgrad', 2, 20, 160, 160, (32,), 2, (1, 1, 1), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_mfma'),
    ('m1_conv3d_wgrad', 2, 20, 160, 160, (32,), 32, (1, 1, 1), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_mfma'),
    ('m1_conv3d_wgrad', 2, 20, 160, 160, (32,), 64, (1, 3, 3), (1, 2, 2), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tf'),
    ('m1_conv3d_wgrad', 2, 20, 160, 160, (8,), 32, (1, 1, 1), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_mfma'),
    ('m1_conv3d_wgrad', 2, 20, 160, 160, (8,), 8, (3, 3, 3), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tf'),
    ('m1_conv3d_wgrad', 2, 20, 40, 40, (128, 128, 128), 128, (3, 3, 3), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_t3:kws8:big1'),
    ('m1_conv3d_wgrad', 2, 20, 40, 40, (128, 128, 128), 32, (3, 3, 3), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tf'),
    ('m1_conv3d_wgrad', 2, 20, 40, 40, (32,), 128, (1, 1, 1), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_mfma'),
    ('m1_conv3d_wgrad', 2, 20, 40, 40, (32,), 32, (3, 3, 3), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tf'),
    ('m1_conv3d_wgrad', 2, 20, 80, 80, (16,), 16, (3, 3, 3), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tf'),
    ('m1_conv3d_wgrad', 2, 20, 80, 80, (16,), 64, (1, 1, 1), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_mfma'),
    ('m1_conv3d_wgrad', 2, 20, 80, 80, (64, 64, 64, 64), 16, (1, 3, 3), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tf'),
    ('m1_conv3d_wgrad', 2, 20, 80, 80, (64, 64, 64, 64), 64, (1, 3, 3), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_t3:kws16:big0'),
    ('m1_conv3d_wgrad', 2, 20, 80, 80, (64, 64, 64, 64, 64), 16, (1, 3, 3), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tf'),
    ('m1_conv3d_wgrad', 2, 20, 80, 80, (64, 64, 64, 64, 64), 64, (1, 3, 3), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_t3:kws16:big0'),
    ('m1_conv3d_wgrad', 2, 20, 80, 80, (64,), 64, (1, 1, 1), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tap'),
    ('m1_conv3d_wgrad', 2, 5, 10, 10, (512,), 32, (1, 1, 1), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_mfma'),
    ('m1_conv3d_wgrad', 2, 5, 10, 10, (512,), 64, (1, 1, 1), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tap'),
    ('m1_conv3d_wgrad', 4, 10, 20, 20, (256, 256), 256, (3, 3, 3), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_t3:kws20:big1'),
    ('m1_conv3d_wgrad', 4, 10, 20, 20, (256, 256), 64, (3, 3, 3), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_t3:kws20:big0'),
    ('m1_conv3d_wgrad', 4, 10, 20, 20, (256, 256, 256), 256, (3, 3, 3), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_t3:kws20:big1'),
    ('m1_conv3d_wgrad', 4, 10, 20, 20, (256, 256, 256), 64, (3, 3, 3), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_t3:kws20:big0'),
    ('m1_conv3d_wgrad', 4, 10, 20, 20, (256,), 128, (3, 3, 3), (2, 2, 2), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tap'),
    ('m1_conv3d_wgrad', 4, 10, 20, 20, (256,), 256, (1, 1, 1), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tap'),
    ('m1_conv3d_wgrad', 4, 10, 20, 20, (256,), 4, (1, 1, 1), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_mfma'),
    ('m1_conv3d_wgrad', 4, 10, 20, 20, (256,), 512, (3, 3, 3), (2, 2, 2), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tap'),
    ('m1_conv3d_wgrad', 4, 10, 20, 20, (64,), 256, (1, 1, 1), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tap'),
    ('m1_conv3d_wgrad', 4, 10, 20, 20, (64,), 64, (3, 3, 3), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tap'),
    ('m1_conv3d_wgrad', 4, 20, 40, 40, (128, 128, 128, 128), 128, (3, 3, 3), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_t3:kws8:big1'),
    ('m1_conv3d_wgrad', 4, 20, 40, 40, (128, 128, 128, 128), 32, (3, 3, 3), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tf'),
    ('m1_conv3d_wgrad', 4, 20, 40, 40, (128,), 128, (1, 1, 1), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tap'),
    ('m1_conv3d_wgrad', 4, 20, 40, 40, (128,), 2, (1, 1, 1), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_mfma'),
    ('m1_conv3d_wgrad', 4, 20, 40, 40, (128,), 256, (3, 3, 3), (2, 2, 2), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_t3:s2:kws20:big1'),
    ('m1_conv3d_wgrad', 4, 20, 40, 40, (128,), 64, (3, 3, 3), (2, 2, 2), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tap'),
    ('m1_conv3d_wgrad', 4, 20, 40, 40, (32,), 128, (1, 1, 1), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_mfma'),
    ('m1_conv3d_wgrad', 4, 20, 40, 40, (32,), 32, (3, 3, 3), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tf'),
    ('m1_conv3d_wgrad', 4, 20, 80, 80, (64,), 128, (3, 3, 3), (1, 2, 2), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_t3:s2:kws8:big1'),
    ('m1_conv3d_wgrad', 4, 20, 80, 80, (64,), 32, (3, 3, 3), (1, 2, 2), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_mfma'),
    ('m1_conv3d_wgrad', 4, 5, 10, 10, (128,), 128, (3, 3, 3), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tap'),
    ('m1_conv3d_wgrad', 4, 5, 10, 10, (128,), 512, (1, 1, 1), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tap'),
    ('m1_conv3d_wgrad', 4, 5, 10, 10, (512,), 128, (1, 1, 1), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tap'),
    ('m1_conv3d_wgrad', 4, 5, 10, 10, (512,), 256, (1, 1, 1), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tap'),
    ('m1_conv3d_wgrad', 4, 5, 10, 10, (512,), 6, (1, 1, 1), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_mfma'),
    ('m1_convT3d_dgrad', 2, 20, 40, 40, (1, 128), 64, (3, 3, 3), (1, 2, 2), 'bf16', 'need=(1, 1),acc=(0, 0)', 'conv_mfma:128x16:w4:ks1+conv_mfma:128x128:w8:ks1'),
    ('m1_convT3d_dgrad', 2, 20, 40, 40, (128,), 64, (3, 3, 3), (1, 2, 2), 'bf16', 'need=(1,),acc=(0,)', 'conv_mfma:128x128:w8:ks1'),
    ('m1_convT3d_dgrad', 2, 20, 40, 40, (128,), 64, (3, 3, 3), (1, 2, 2), 'bf16', 'need=(1,),acc=(1,)', 'conv_mfma:128x128:w8:ks1'),
    ('m1_convT3d_dgrad', 2, 20, 80, 80, (64,), 32, (1, 3, 3), (1, 2, 2), 'bf16', 'need=(1,),acc=(0,)', 'conv_halo:bn32'),
    ('m1_convT3d_dgrad', 2, 20, 80, 80, (64,), 32, (1, 3, 3), (1, 2, 2), 'bf16', 'need=(1,),acc=(1,)', 'conv_halo:bn32'),
    ('m1_convT3d_dgrad', 4, 10, 20, 20, (2, 256), 128, (3, 3, 3), (2, 2, 2), 'bf16', 'need=(1, 1),acc=(0, 0)', 'conv_mfma:64x16:w4:ks3+conv_mfma:128x128:w8:ks1'),
    ('m1_convT3d_dgrad', 4, 10, 20, 20, (256,), 128, (3, 3, 3), (2, 2, 2), 'bf16', 'need=(1,),acc=(0,)', 'conv_mfma:128x128:w8:ks1'),
    ('m1_convT3d_dgrad', 4, 10, 20, 20, (256,), 128, (3, 3, 3), (2, 2, 2), 'bf16', 'need=(1,),acc=(1,)', 'conv_mfma:128x128:w8:ks1'),
    ('m1_convT3d_dgrad', 4, 5, 10, 10, (3, 512), 256, (3, 3, 3), (2, 2, 2), 'bf16', 'need=(1, 1),acc=(0, 0)', 'conv_mfma:64x16:w4:ks16+conv_mfma:64x128:w4:ks4'),
    ('m1_convT3d_dgrad', 4, 5, 10, 10, (512,), 256, (3, 3, 3), (2, 2, 2), 'bf16', 'need=(1,),acc=(1,)', 'conv_mfma:64x128:w4:ks4'),
    ('m1_convT3d_fwd', 2, 20, 40, 40, (1, 128), 64, (3, 3, 3), (1, 2, 2), 'bf16', '', 'conv_mfma:128x64:w8:ks1+conv_mfma:128x64:w8:ks1'),
    ('m1_convT3d_fwd', 2, 20, 40, 40, (128,), 64, (3, 3, 3), (1, 2, 2), 'bf16', '', 'conv_mfma:128x64:w8:ks1'),
    ('m1_convT3d_fwd', 2, 20, 80, 80, (64,), 32, (1, 3, 3), (1, 2, 2), 'bf16', '', 'conv_halo_cls:bn32'),
    ('m1_convT3d_fwd', 4, 10, 20, 20, (2, 256), 128, (3, 3, 3), (2, 2, 2), 'bf16', '', 'conv_mfma:128x128:w8:ks1+conv_mfma:128x128:w8:ks1'),
    ('m1_convT3d_fwd', 4, 10, 20, 20, (256,), 128, (3, 3, 3), (2, 2, 2), 'bf16', '', 'conv_mfma:128x128:w8:ks1'),
    ('m1_convT3d_fwd', 4, 5, 10, 10, (3, 512), 256, (3, 3, 3), (2, 2, 2), 'bf16', '', 'conv_mfma:128x128:w8:ks1+conv_mfma:128x128:w8:ks1'),
    ('m1_convT3d_fwd', 4, 5, 10, 10, (512,), 256, (3, 3, 3), (2, 2, 2), 'bf16', '', 'conv_mfma:128x128:w8:ks1'),
    ('m1_convT3d_wgrad', 2, 20, 40, 40, (1, 128), 64, (3, 3, 3), (1, 2, 2), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_mfma+wgrad_t3:s2:kws8:big1'),
    ('m1_convT3d_wgrad', 2, 20, 40, 40, (128,), 64, (3, 3, 3), (1, 2, 2), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_t3:s2:kws8:big1'),
    ('m1_convT3d_wgrad', 2, 20, 80, 80, (64,), 32, (1, 3, 3), (1, 2, 2), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tf'),
    ('m1_convT3d_wgrad', 4, 10, 20, 20, (2, 256), 128, (3, 3, 3), (2, 2, 2), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_mfma+wgrad_t3:s2:kws20:big1'),
    ('m1_convT3d_wgrad', 4, 10, 20, 20, (256,), 128, (3, 3, 3), (2, 2, 2), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_t3:s2:kws20:big1'),
    ('m1_convT3d_wgrad', 4, 5, 10, 10, (3, 512), 256, (3, 3, 3), (2, 2, 2), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_mfma+wgrad_tap'),
    ('m1_convT3d_wgrad', 4, 5, 10, 10, (512,), 256, (3, 3, 3), (2, 2, 2), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tap'),
]

# what the C3 recording does not show but other workloads reach
EXTRA_CONV_KEYS = [
    # the stem at C5's size in fp32 (Cin = 3: zero-padded to a matrix-core tile; strided tap-fused fp32 weight gradient)
    ('m1_conv3d_dgrad', 1, 32, 256, 256, (3,), 32, (1, 3, 3), (1, 1, 1), 'fp32', 'need=(1,),acc=(0,)', 'conv_mfma:128x16:w4:ks1'),
    ('m1_conv3d_fwd', 1, 32, 256, 256, (3,), 32, (1, 3, 3), (1, 1, 1), 'fp32', 'stats=1', 'conv_mfma:128x32:w8:ks1'),
    ('m1_conv3d_wgrad', 1, 32, 256, 256, (3,), 32, (1, 3, 3), (1, 1, 1), 'fp32', 'acc=1,bias=1,defer=1', 'wgrad_t3s'),
    # C5 fp32 res0 (1, 32, 256, 256): fp32 matrix-core forward / data gradient where bf16 takes conv_halo / conv_pw, wgrad_t3s / wgrad_pwf
    ('m1_conv3d_dgrad', 1, 32, 256, 256, (32, 32), 32, (1, 3, 3), (1, 1, 1), 'fp32', 'need=(1, 1),acc=(0, 0)', 'conv_mfma:128x64:w8:ks1'),
    ('m1_conv3d_fwd', 1, 32, 256, 256, (32, 32), 32, (1, 3, 3), (1, 1, 1), 'fp32', 'stats=1', 'conv_mfma:128x32:w8:ks1'),
    ('m1_conv3d_wgrad', 1, 32, 256, 256, (32, 32), 32, (1, 3, 3), (1, 1, 1), 'fp32', 'acc=1,bias=1,defer=1', 'wgrad_t3s+wgrad_t3s'),
    ('m1_conv3d_dgrad', 1, 32, 256, 256, (32,), 32, (1, 1, 1), (1, 1, 1), 'fp32', 'need=(1,),acc=(0,)', 'conv_mfma:128x32:w8:ks1'),
    ('m1_conv3d_fwd', 1, 32, 256, 256, (32,), 32, (1, 1, 1), (1, 1, 1), 'fp32', 'stats=1', 'conv_mfma:128x32:w8:ks1'),
    ('m1_conv3d_wgrad', 1, 32, 256, 256, (32,), 32, (1, 1, 1), (1, 1, 1), 'fp32', 'acc=1,bias=1,defer=1', 'wgrad_pwf'),
    ('m1_conv3d_dgrad', 1, 32, 256, 256, (32,), 64, (1, 3, 3), (1, 2, 2), 'fp32', 'need=(1,),acc=(0,)', 'conv_mfma:128x32:w8:ks1'),
    ('m1_conv3d_fwd', 1, 32, 256, 256, (32,), 64, (1, 3, 3), (1, 2, 2), 'fp32', 'stats=1', 'conv_mfma:128x64:w8:ks1'),
    ('m1_conv3d_wgrad', 1, 32, 256, 256, (32,), 64, (1, 3, 3), (1, 2, 2), 'fp32', 'acc=1,bias=1,defer=1', 'wgrad_t3s'),
    # C5 fp32 deeper levels: wgrad_t3f (64x64 tiles), strided and transposed wgrad_t3s
    ('m1_conv3d_dgrad', 1, 32, 64, 64, (128, 128), 128, (3, 3, 3), (1, 1, 1), 'fp32', 'need=(1, 1),acc=(0, 0)', 'conv_mfma:128x128:w8:ks1'),
    ('m1_conv3d_fwd', 1, 32, 64, 64, (128, 128), 128, (3, 3, 3), (1, 1, 1), 'fp32', 'stats=1', 'conv_mfma:128x128:w8:ks1'),
    ('m1_conv3d_wgrad', 1, 32, 64, 64, (128, 128), 128, (3, 3, 3), (1, 1, 1), 'fp32', 'acc=1,bias=1,defer=1', 'wgrad_t3f:kws32:big1'),
    ('m1_conv3d_dgrad', 1, 32, 128, 128, (64,), 128, (3, 3, 3), (1, 2, 2), 'fp32', 'need=(1,),acc=(0,)', 'conv_mfma:128x64:w8:ks1'),
    ('m1_conv3d_fwd', 1, 32, 128, 128, (64,), 128, (3, 3, 3), (1, 2, 2), 'fp32', 'stats=1', 'conv_mfma:128x128:w8:ks1'),
    ('m1_conv3d_wgrad', 1, 32, 128, 128, (64,), 128, (3, 3, 3), (1, 2, 2), 'fp32', 'acc=1,bias=1,defer=1', 'wgrad_t3s'),
    ('m1_convT3d_dgrad', 1, 32, 128, 128, (64,), 32, (1, 3, 3), (1, 2, 2), 'fp32', 'need=(1,),acc=(0,)', 'conv_mfma:128x64:w8:ks1'),
    ('m1_convT3d_fwd', 1, 32, 128, 128, (64,), 32, (1, 3, 3), (1, 2, 2), 'fp32', '', 'conv_mfma:128x32:w8:ks1'),
    ('m1_convT3d_wgrad', 1, 32, 128, 128, (64,), 32, (1, 3, 3), (1, 2, 2), 'fp32', 'acc=1,bias=1,defer=1', 'wgrad_t3s'),
    # batch 4 of layers the C3 step runs at batch 2 only (grids over N * tiles: conv_halo, thin_fwd, wgrad_tf, wgrad_t3)
    ('m1_conv3d_dgrad', 4, 20, 80, 80, (64, 64, 64, 64), 64, (1, 3, 3), (1, 1, 1), 'bf16', 'need=(1, 1, 1, 1),acc=(0, 0, 0, 0)', 'conv_halo:bn32+conv_halo:bn32+conv_halo:bn32+conv_halo:bn32'),
    ('m1_conv3d_fwd', 4, 20, 80, 80, (64, 64, 64, 64), 64, (1, 3, 3), (1, 1, 1), 'bf16', 'stats=1', 'conv_halo:bn32+conv_halo:bn32+conv_halo:bn32+conv_halo:bn32'),
    ('m1_conv3d_wgrad', 4, 20, 80, 80, (64, 64, 64, 64), 64, (1, 3, 3), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_t3:kws16:big0'),
    ('m1_conv3d_dgrad', 4, 20, 160, 160, (32, 32), 32, (1, 3, 3), (1, 1, 1), 'bf16', 'need=(1, 1),acc=(0, 0)', 'conv_halo:bn32+conv_halo:bn32'),
    ('m1_conv3d_fwd', 4, 20, 160, 160, (32, 32), 32, (1, 3, 3), (1, 1, 1), 'bf16', 'stats=1', 'conv_halo:bn32'),
    ('m1_conv3d_wgrad', 4, 20, 160, 160, (32, 32), 32, (1, 3, 3), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tf'),
    ('m1_conv3d_dgrad', 4, 20, 160, 160, (3,), 32, (1, 3, 3), (1, 1, 1), 'bf16', 'need=(1,),acc=(0,)', 'conv_halo:bn16'),
    ('m1_conv3d_fwd', 4, 20, 160, 160, (3,), 32, (1, 3, 3), (1, 1, 1), 'bf16', 'stats=1', 'thin_fwd'),
    ('m1_conv3d_wgrad', 4, 20, 160, 160, (3,), 32, (1, 3, 3), (1, 1, 1), 'bf16', 'acc=1,bias=1,defer=1', 'wgrad_tf'),
    # InstanceNorm-backward sums from conv_t3's LDS-tile epilogue (no layer of the C3 step: its 3x3x3 layers with a norm in front are
    # narrower or smaller than the staged-run kernel takes): the smallest launch m1_ct3_plan accepts -- 96 channels on both sides,
    # N V = 4,200 >= 4,096 voxels -- on a ragged volume (2,100 voxels per sample = 8 tiles of 256 + 52)
    ('m1_conv3d_dgrad_inbwd', 2, 7, 15, 20, (96,), 96, (3, 3, 3), (1, 1, 1), 'bf16', 'fused=1', 'conv_t3:bn128:ks1'),
]


# =================================================================================================================================
# part 2: every key against fp64 on the whole volume
# =================================================================================================================================
def _split(t, cins):
    return torch.split(t, list(cins), dim=-1)


def _no_wgrad(names):
    return [n for n in names if not n.startswith("wgrad")]


def _parse(fl, field):
    return tuple(int(v) for v in re.search(field + r"=\(([^)]*)\)", fl).group(1).replace(" ", "").split(",") if v)


def _fwd_key(dev, key):
    name, N, D, H, W, cins, cout, k, s, dts, fl, kern = key
    dtype, transposed, pair = _DT[dts], "convT" in name, "pair" in name
    ctot = sum(cout) if pair else cout
    xs, w, b, _ = _conv_inputs(dev, dtype, N, (D, H, W), cins, ctot, k, s, transposed, _gen(dev, zlib.crc32(repr(key).encode()) % 10007))
    xd = [x.to(dtype) for x in xs]
    with torch.no_grad(), ops.kernel_log() as kl:
        if pair:
            c1 = cout[0]
            assert ops.conv_pair_supported(xd, w[..., :c1], w[..., c1:], s)
            y1, s1, y4, s4, br = ops.conv_pair_same(xd, w[..., :c1].contiguous(), b[:c1].contiguous(), w[..., c1:].contiguous(),
                                                    b[c1:].contiguous(), k, s)
            br.join(y4, s4)
            outs = [(y1, s1, slice(0, c1)), (y4, s4, slice(c1, ctot))]
        elif transposed:
            outs = [(ops.conv3d_transpose_same(xd, w, b, k, s), None, slice(0, ctot))]
        else:
            st = "stats=1" in fl
            r = ops.conv3d_same(xd, w, b, k, s, stats=st)
            outs = [(r[0], r[1], slice(0, ctot))] if st else [(r, None, slice(0, ctot))]
        torch.cuda.synchronize()
    assert _no_wgrad(kl.names) == kern.split("+"), (kl.names, kern)
    ref, mag = ref_conv_with_mag(torch.cat(xs, -1), w, b, s, None, transposed)
    amag = None
    if len(kern.split("+")) > 1 and dtype == torch.bfloat16:
        # several launches (groups of concat members) add into the bf16 output: every launch rounds its own contribution and the new
        # running sum (util.ref_member_amag)
        amag = util.ref_member_amag(xs, w, b, s, transposed)
    for y, st, sl in outs:
        assert_conv_close(y, ref["y"][..., sl], mag["y"][..., sl], dtype, f"y[{sl.start}:{sl.stop}] of {key}",
                          amag=None if amag is None else amag[..., sl])
        if st is not None:
            _assert_stats(st, y.float(), f"fused statistics of {key}")
    # the second call with an unchanged weight finds its panel packed: bit for bit the first result
    if not pair:
        wl = w.clone().requires_grad_(True)                   # (a leaf: its panels are cached on it)
        with torch.no_grad():
            if transposed:
                ya, yb = (ops.conv3d_transpose_same(xd, wl, b, k, s) for _ in range(2))
            else:
                ya, yb = (ops.conv3d_same(xd, wl, b, k, s, stats="stats=1" in fl) for _ in range(2))
                if "stats=1" in fl:
                    assert torch.equal(ya[1], yb[1])
                    ya, yb = ya[0], yb[0]
        assert torch.equal(ya, yb) and torch.equal(ya, outs[0][0])


def _dgrad_key(dev, key):
    name, N, D, H, W, cins, cout, k, s, dts, fl, kern = key
    dtype, transposed, pair = _DT[dts], "convT" in name, "pair" in name
    ctot = sum(cout) if pair else cout
    need, acc = _parse(fl, "need"), _parse(fl, "acc")
    g = _gen(dev, zlib.crc32(repr(key).encode()) % 10007)
    xs, w, b, dy = _conv_inputs(dev, dtype, N, (D, H, W), cins, ctot, k, s, transposed, g)
    xd, pre = [], []
    for x, nd, ac in zip(xs, need, acc):
        t = x.to(dtype).requires_grad_(bool(nd))
        pre.append(None)
        if ac:                                              # a fan-out slot that already holds another consumer's gradient
            slot = ops._GradSlot()
            pre[-1] = _as(_randn(tuple(x.shape), g, dev) - 0.4, dtype).to(dtype)
            slot.buf, slot.tail_init = pre[-1].clone(), True
            t._m1_gslot = slot
        xd.append(t)
    if pair:
        c1 = cout[0]
        y1, s1, y4, s4, br = ops.conv_pair_same(xd, w[..., :c1].contiguous(), b[:c1].contiguous(), w[..., c1:].contiguous(),
                                                b[c1:].contiguous(), k, s)
        br.join(y4, s4)
        ys, dys = [y1, y4], [dy[..., :c1].to(dtype).contiguous(), dy[..., c1:].to(dtype).contiguous()]
    else:
        ys = [(ops.conv3d_transpose_same if transposed else ops.conv3d_same)(xd, w, b, k, s)]
        dys = [dy.to(dtype)]
    with ops.kernel_log() as kl:
        torch.autograd.backward(ys, dys)
        ops.join_side_streams()
        torch.cuda.synchronize()
    assert _no_wgrad(kl.names) == kern.split("+"), (kl.names, kern)
    ref, mag = ref_conv_with_mag(torch.cat(xs, -1), w, None, s, dy, transposed)
    for i, (t, r_, m_) in enumerate(zip(xd, _split(ref["dx"], cins), _split(mag["dx"], cins))):
        if not need[i]:
            assert t.grad is None
            continue
        if acc[i]:
            got = t._m1_gslot.buf
            assert got.data_ptr() != pre[i].data_ptr()
            # the kernel rounds its own gradient to the storage type, adds it to the slot and rounds the sum: a * (|dx| + |sum|)
            assert_conv_close(got, pre[i].double() + r_, m_ + pre[i].double().abs(), dtype, f"dx[{i}] (accumulated) of {key}",
                              amag=r_.abs() if dtype == torch.bfloat16 else None, acc=dtype != torch.bfloat16)
        else:
            assert_conv_close(t.grad, r_, m_, dtype, f"dx[{i}] of {key}")


def _wgrad_key(dev, key):
    name, N, D, H, W, cins, cout, k, s, dts, fl, kern = key
    dtype, transposed = _DT[dts], "convT" in name
    assert fl == "acc=1,bias=1,defer=1", fl                 # what the step does: gradients into the optimiser's flat buffer, folds queued
    g = _gen(dev, zlib.crc32(repr(key).encode()) % 10007)
    xs, w, b, dy = _conv_inputs(dev, dtype, N, (D, H, W), cins, cout, k, s, transposed, g)
    xd = [x.to(dtype) for x in xs]
    fn = ops.conv3d_transpose_same if transposed else ops.conv3d_same
    ref, mag = ref_conv_with_mag(torch.cat(xs, -1), w, b, s, dy, transposed)
    assert float((mag["dw"] / ref["dw"].abs()).median()) < DW_CANCEL
    pre_w, pre_b = 2.0 + _randn(tuple(w.shape), g, dev), -1.0 + _randn((cout,), g, dev)
    res = {}
    for mode in ("sink", "plain"):
        wd, bd = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        if mode == "sink":
            wd._m1_gsink, bd._m1_gsink = pre_w.clone(), pre_b.clone()
        y = fn(xd, wd, bd, k, s)
        with ops.kernel_log() as kl:
            y.backward(dy.to(dtype))
            ops.fold_pending()
            torch.cuda.synchronize()
        if mode == "sink":                                  # (the recorded call; accumulate 0 may legitimately take another route)
            assert [n for n in kl.names if n.startswith("wgrad")] == kern.split("+"), (kl.names, kern)
        if mode == "sink":
            assert wd.grad is None and bd.grad is None
            assert_conv_close(wd._m1_gsink, pre_w.double() + ref["dw"], mag["dw"] + pre_w.double().abs(), torch.float32,
                              f"dW (accumulate 1, folds queued) of {key}", acc=True)
            assert_conv_close(bd._m1_gsink, pre_b.double() + ref["db"], mag["db"] + pre_b.double().abs(), torch.float32,
                              f"db (accumulate 1, folds queued) of {key}", acc=True)
        else:
            assert_conv_close(wd.grad, ref["dw"], mag["dw"], torch.float32, f"dW (accumulate 0) of {key}")
            assert_conv_close(bd.grad, ref["db"], mag["db"], torch.float32, f"db (accumulate 0) of {key}")


def _inbwd_key(dev, key):
    name, N, D, H, W, cins, cout, k, s, dts, fl, kern = key
    assert s == (1, 1, 1) and len(cins) == 1
    _inbwd_case(dev, _DT[dts], (N, D, H, W), cins[0], cout, seed=zlib.crc32(repr(key).encode()) % 10007, expect_fused=fl == "fused=1",
                k=k, kernels=kern.split("+"))


def _run_conv_key(dev, key):
    name = key[0]
    with ops.config(M1_T3_MIN_BLOCKS=128):                  # (the suite's conftest lifts this one floor; the bench runs at 128)
        if name.endswith("_fwd"):
            _fwd_key(dev, key)
        elif name == "m1_conv3d_dgrad_inbwd":
            _inbwd_key(dev, key)
        elif name.endswith("_dgrad"):
            _dgrad_key(dev, key)
        else:
            _wgrad_key(dev, key)
    ops.drop_deferred()
    ops.invalidate_panels()
    torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("key", C3_CONV_KEYS + EXTRA_CONV_KEYS, ids=lambda k: "-".join(str(v) for v in k).replace(" ", ""))
def test_bench_conv_against_fp64(dev, key):
    _run_conv_key(dev, key)


@pytest.mark.gpu
def test_c3_bench_conv_keys_are_in_the_table(dev, monkeypatch):
    with ops.config(M1_T3_MIN_BLOCKS=128):
        seen, calls = record_c3_bench_conv_keys(dev, monkeypatch)
    assert calls >= 300, calls
    missing = sorted(seen - set(C3_CONV_KEYS), key=str)
    assert not missing, f"conv calls of the C3 bench step not in C3_CONV_KEYS: {missing}"


# ---- weight gradients through the queue: two different layers queued (ops._WGP), launched and folded together by fold_pending ----
def _key(name, N, D, H, W, cins, cout, k, s=(1, 1, 1)):
    hit = [q for q in C3_CONV_KEYS if q[:9] == (name, N, D, H, W, tuple(cins), cout, k, s)]
    assert hit, (name, N, D, H, W, cins, cout, k, s)
    return hit[0]


QUEUE_PAIRS = [  # a transposed conv (its bias gradient is the column sum deferred to the fold) next to a tap-fused stride-1 layer ...
    (("m1_convT3d_wgrad", 2, 20, 40, 40, (128,), 64, (3, 3, 3), (1, 2, 2)), ("m1_conv3d_wgrad", 4, 10, 20, 20, (256, 256), 64, (3, 3, 3), (1, 1, 1))),
    # ... and the small-channel tap-fused kernel next to the per-tap kernel and a transposed halo layer
    (("m1_conv3d_wgrad", 2, 20, 40, 40, (32,), 32, (3, 3, 3), (1, 1, 1)), ("m1_convT3d_wgrad", 2, 20, 80, 80, (64,), 32, (1, 3, 3), (1, 2, 2))),
    (("m1_conv3d_wgrad", 4, 5, 10, 10, (128,), 128, (3, 3, 3), (1, 1, 1)), ("m1_conv3d_wgrad", 2, 20, 80, 80, (64,), 64, (1, 1, 1), (1, 1, 1))),
]


@pytest.mark.gpu
@pytest.mark.parametrize("pair", QUEUE_PAIRS, ids=lambda p: "+".join(f"{q[0][3:]}-{q[1]}x{q[2]}x{q[3]}x{q[4]}-{sum(q[5])}-{q[6]}" for q in p))
def test_queued_weight_gradients_equal_direct_and_fp64(dev, pair, monkeypatch):
    """m1_wgrad_defer with two different layers in the queue: both are launched by ops._run_deferred_wgrads and folded by one
    fold_pending.  M1_WG_DET (default 1) promises run-to-run identical weight gradients: the queued results equal the results of the
    same layers launched in place one at a time, bit for bit, and both meet the fp64 bound (a wrong workspace slot, a wrong fold target
    or a second entry's bias column sum left out would not)."""
    keys = [_key(*q) for q in pair]
    layers = []
    for key in keys:
        name, N, D, H, W, cins, cout, k, s, dts, fl, kern = key
        dtype, tr = _DT[dts], "convT" in name
        g = _gen(dev, zlib.crc32(repr(key).encode()) % 10007)
        xs, w, b, dy = _conv_inputs(dev, dtype, N, (D, H, W), cins, cout, k, s, tr, g)
        pre = (2.0 + _randn(tuple(w.shape), g, dev), -1.0 + _randn((cout,), g, dev))
        layers.append((key, dtype, tr, xs, w, b, dy, pre))

    def run(queued):
        out = []
        with ops.config(M1_T3_MIN_BLOCKS=128), ops.kernel_log() as kl:
            for (key, dtype, tr, xs, w, b, dy, pre) in layers:
                wd, bd = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
                wd._m1_gsink, bd._m1_gsink = pre[0].clone(), pre[1].clone()
                y = (ops.conv3d_transpose_same if tr else ops.conv3d_same)([x.to(dtype) for x in xs], wd, bd, key[7], key[8])
                y.backward(dy.to(dtype))
                out.append((wd._m1_gsink, bd._m1_gsink))
                if not queued:
                    ops.fold_pending()
            if queued:
                assert len(ops._WGP["jobs"]) == 2 and not [n for n in kl.names if n.startswith("wgrad")], (len(ops._WGP["jobs"]), kl.names)
                ops.fold_pending()
            torch.cuda.synchronize()
        assert not ops._WGP["jobs"] and not ops._FOLD["keep"]
        assert [n for n in kl.names if n.startswith("wgrad")] == [n for key in keys for n in key[-1].split("+")], kl.names
        return out
    monkeypatch.setitem(ops._BRANCH, "origin", torch.cuda.current_stream())
    monkeypatch.setitem(ops._FOLD, "async", 0)                # (no fold trigger of its own inside the two backward passes)
    queued = run(True)
    monkeypatch.setitem(ops._WGP, "maxvox", 0)                # launched where autograd calls them, folds still queued
    direct = run(False)
    for (key, dtype, tr, xs, w, b, dy, pre), (qw, qb), (dw, db) in zip(layers, queued, direct):
        assert torch.equal(qw, dw) and torch.equal(qb, db), key
        ref, mag = ref_conv_with_mag(torch.cat(xs, -1), w, b, key[8], dy, tr)
        assert_conv_close(qw, pre[0].double() + ref["dw"], mag["dw"] + pre[0].double().abs(), torch.float32, f"queued dW of {key}", acc=True)
        assert_conv_close(qb, pre[1].double() + ref["db"], mag["db"] + pre[1].double().abs(), torch.float32, f"queued db of {key}", acc=True)
    ops.drop_deferred(); ops.invalidate_panels(); torch.cuda.empty_cache()


# ---- the queue's duplicate rules: the same weight / the same db twice before one fold_pending ----
QUEUE_TWICE = [("m1_conv3d_wgrad", 4, 5, 10, 10, (128,), 128, (3, 3, 3), (1, 1, 1)),       # the smallest keys of C3_CONV_KEYS
               ("m1_convT3d_wgrad", 2, 20, 40, 40, (128,), 64, (3, 3, 3), (1, 2, 2))]


@pytest.mark.gpu
@pytest.mark.parametrize("q", QUEUE_TWICE, ids=lambda q: f"{q[0][3:]}-{q[1]}x{q[2]}x{q[3]}x{q[4]}-{sum(q[5])}-{q[6]}")
def test_same_parameter_twice_in_the_queue(dev, q, monkeypatch):
    """Two backward passes of ONE layer accumulate into the same ``_m1_gsink`` pair before one fold_pending (a parameter used by two
    passes of a step).  Two read-modify-writes of the same block must not share a batched launch:
    * fold: the second fold into a queued (R, a_off, b_off) runs at once on its call's stream, the queued one stays (m1_wg_rx_finish);
    * column sum (transposed conv, db): a second sum into a queued ``out`` is declined and the caller reduces in place (m1_colsum_defer).
    The plan log (ops.plan_log) says of every fold whether it was queued or ran at once: with the weight gradients launched in place
    the first call's folds are all "queued", the second call's all "now", and fold_pending launches one batch that holds the first call's.
    The column sums have no log entry, so for them (and once more for the folds) what was queued is read off the sinks between the
    calls: a queued fold / sum leaves its sink untouched, one that ran at once has added one gradient; after fold_pending both hold two.  The same through the deferred launches (both calls inside one m1_wgrad_defer window), twice: equal
    bits run to run.  Not compared bit for bit ACROSS the two orders: which call folds first may change the last bit."""
    key = _key(*q)
    name, N, D, H, W, cins, cout, k, s, dts, fl, kern = key
    dtype, tr = _DT[dts], "convT" in name
    g = _gen(dev, zlib.crc32(repr(key).encode()) % 10007)
    xs, w, b, dy = _conv_inputs(dev, dtype, N, (D, H, W), cins, cout, k, s, tr, g)
    pre_w, pre_b = 2.0 + _randn(tuple(w.shape), g, dev), -1.0 + _randn((cout,), g, dev)
    ref, mag = ref_conv_with_mag(torch.cat(xs, -1), w, b, s, dy, tr)
    once = {}

    def run(in_place):
        wd, bd = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        wd._m1_gsink, bd._m1_gsink = pre_w.clone(), pre_b.clone()
        folds = []                                            # per backward pass: its "fold:" entries of the plan log
        with ops.config(M1_T3_MIN_BLOCKS=128), ops.kernel_log() as kl:
            for i in range(2):
                y = (ops.conv3d_transpose_same if tr else ops.conv3d_same)([x.to(dtype) for x in xs], wd, bd, k, s)
                with ops.plan_log() as pl:
                    y.backward(dy.to(dtype))
                folds.append(pl.of("fold:"))
                if in_place:
                    # the first call's folds are queued; the second finds its (R, a_off, b_off) in the queue and folds at once
                    assert folds[i] and all(f.endswith(" now" if i else " queued") for f in folds[i]), (i, folds[i])
                    assert not pl.of("foldbatch:"), pl.entries
                    torch.cuda.synchronize()
                    if i == 0:                                # queued: nothing has touched the sinks
                        assert torch.equal(wd._m1_gsink, pre_w) and torch.equal(bd._m1_gsink, pre_b), key
                    else:                                     # the duplicates ran at once: ONE gradient in each sink
                        once["w"], once["b"] = wd._m1_gsink.clone(), bd._m1_gsink.clone()
            if not in_place:
                assert len(ops._WGP["jobs"]) == 2 and not [n for n in kl.names if n.startswith("wgrad")], (len(ops._WGP["jobs"]), kl.names)
                assert folds == [[], []], folds               # (nothing launched, nothing folded or queued yet)
            with ops.plan_log() as pl:
                ops.fold_pending()
                torch.cuda.synchronize()
            late, batch = pl.of("fold:"), pl.of("foldbatch:")
            if in_place:                                      # one batch: exactly the folds the first call queued
                assert not late and batch == [f"foldbatch:n={len(folds[0])} blocks={batch[0].split('blocks=')[1]}"], (late, batch)
            else:                                             # both calls launched here, in order: the first queues, the second folds at once
                assert len(late) % 2 == 0 and late[:len(late) // 2] == [f.replace(" now", " queued") for f in late[len(late) // 2:]], late
                assert all(f.endswith(" queued") for f in late[:len(late) // 2]) and len(batch) == 1, (late, batch)
                assert batch[0].startswith(f"foldbatch:n={len(late) // 2} "), (late, batch)
        assert not ops._WGP["jobs"] and not ops._FOLD["keep"]
        assert [n for n in kl.names if n.startswith("wgrad")] == 2 * kern.split("+"), kl.names      # (partial-copy kernels, both times)
        return wd._m1_gsink, bd._m1_gsink
    monkeypatch.setitem(ops._BRANCH, "origin", torch.cuda.current_stream())
    monkeypatch.setitem(ops._FOLD, "async", 0)                # (no fold trigger of its own inside the two backward passes)
    qa, qb = run(False), run(False)
    assert torch.equal(qa[0], qb[0]) and torch.equal(qa[1], qb[1]), key
    monkeypatch.setitem(ops._WGP, "maxvox", 0)                # launched where autograd calls them, folds and column sums still queued
    da, db_ = run(True), run(True)
    assert torch.equal(da[0], db_[0]) and torch.equal(da[1], db_[1]), key
    assert_conv_close(once["w"], pre_w.double() + ref["dw"], mag["dw"] + pre_w.double().abs(), torch.float32, f"dW after the duplicate of {key}", acc=True)
    assert_conv_close(once["b"], pre_b.double() + ref["db"], mag["db"] + pre_b.double().abs(), torch.float32, f"db after the duplicate of {key}", acc=True)
    for what, (gw, gb) in (("deferred launches", qa), ("in place", da)):
        assert_conv_close(gw, pre_w.double() + 2 * ref["dw"], 2 * mag["dw"] + pre_w.double().abs(), torch.float32, f"dW twice ({what}) of {key}", acc=True)
        assert_conv_close(gb, pre_b.double() + 2 * ref["db"], 2 * mag["db"] + pre_b.double().abs(), torch.float32, f"db twice ({what}) of {key}", acc=True)
    ops.drop_deferred(); ops.invalidate_panels(); torch.cuda.empty_cache()


# ---- packed panels: second call with packed = 1, bit for bit; weights changed behind autograd's back + repack_all against fp64 ----
PANEL_KEYS = [  # one forward key per kernel family that reads a packed panel (its data gradient runs as well)
    ("m1_conv3d_fwd", 4, 10, 20, 20, (64,), 64, (3, 3, 3), (1, 1, 1)),                     # conv_mfma (K groups)
    ("m1_conv3d_pair_fwd", 4, 10, 20, 20, (256, 256), (64, 256), (3, 3, 3), (1, 1, 1)),   # conv_t3, the pair's panel
    ("m1_conv3d_fwd", 2, 20, 80, 80, (64, 64, 64, 64), 64, (1, 3, 3), (1, 1, 1)),         # conv_halo, one launch per member
    ("m1_conv3d_fwd", 2, 20, 80, 80, (64,), 64, (1, 1, 1), (1, 1, 1)),                    # conv_pw
    ("m1_conv3d_fwd", 2, 20, 160, 160, (3,), 32, (1, 3, 3), (1, 1, 1)),                   # thin_fwd (stem)
    ("m1_convT3d_fwd", 2, 20, 80, 80, (64,), 32, (1, 3, 3), (1, 2, 2)),                   # conv_halo_cls (transposed)
    ("m1_convT3d_fwd", 4, 5, 10, 10, (512,), 256, (3, 3, 3), (2, 2, 2)),                  # conv_mfma parity classes
]


@pytest.mark.gpu
@pytest.mark.parametrize("pk", PANEL_KEYS, ids=lambda q: f"{q[0][3:]}-{q[1]}x{q[2]}x{q[3]}x{q[4]}-{sum(q[5])}-{q[6]}")
def test_packed_panels_second_call_and_repack_after_weight_update(dev, pk, monkeypatch):
    key = _key(*pk)
    name, N, D, H, W, cins, cout, k, s, dts, fl, kern = key
    dtype, tr, pair = _DT[dts], "convT" in name, "pair" in name
    ctot = sum(cout) if pair else cout
    g = _gen(dev, zlib.crc32(repr(key).encode()) % 10007)
    xs, w, b, dy = _conv_inputs(dev, dtype, N, (D, H, W), cins, ctot, k, s, tr, g)
    w2 = _as(0.7 * w + _randn(tuple(w.shape), g, dev, 0.7 / (sum(cins) * k[0] * k[1] * k[2]) ** 0.5), dtype)
    lib, flags = L.load(), []
    where = {"m1_conv3d_fwd": 6, "m1_convT3d_fwd": 5, "m1_conv3d_dgrad": 6, "m1_convT3d_dgrad": 6, "m1_conv3d_pair_fwd": 11,
             "m1_conv3d_pair_dgrad": 9}
    for fname, pos in where.items():
        def wrap(*args, _fn=getattr(lib, fname), _n=fname, _p=pos):
            flags.append((_n.split("_")[-1], int(args[_p])))
            return _fn(*args)
        monkeypatch.setattr(lib, fname, wrap)
    c1 = cout[0] if pair else None
    ws = [w[..., :c1].clone(), w[..., c1:].clone()] if pair else [w.clone()]
    ws = [t.requires_grad_(True) for t in ws]                 # leaves: the panels are cached on them and registered for repack_all

    def run():
        del flags[:]
        xd = [x.to(dtype).requires_grad_(True) for x in xs]
        if pair:
            y1, s1, y4, s4, br = ops.conv_pair_same(xd, ws[0], b[:c1].contiguous(), ws[1], b[c1:].contiguous(), k, s)
            br.join(y4, s4)
            torch.autograd.backward([y1, y4], [dy[..., :c1].to(dtype).contiguous(), dy[..., c1:].to(dtype).contiguous()])
            y = torch.cat([y1, y4], -1)
        else:
            y = (ops.conv3d_transpose_same if tr else ops.conv3d_same)(xd, ws[0], b, k, s)
            y.backward(dy.to(dtype))
        ops.join_side_streams()
        torch.cuda.synchronize()
        return y.detach(), [x.grad for x in xd], sorted(set(flags))
    with ops.config(M1_T3_MIN_BLOCKS=128):
        ops.invalidate_panels()
        y0, dx0, f0 = run()
        y1_, dx1, f1 = run()
        assert f0 == [("dgrad", 0), ("fwd", 0)] and f1 == [("dgrad", 1), ("fwd", 1)], (f0, f1)
        assert torch.equal(y0, y1_) and all(torch.equal(a_, b_) for a_, b_ in zip(dx0, dx1))
        # the optimiser's way: the values change through the raw buffer (no version bump), then one repack_all
        with torch.no_grad():
            for t, src in zip(ws, [w2[..., :c1], w2[..., c1:]] if pair else [w2]):
                t.data.copy_(src)
        ops.repack_all()
        y2, dx2, f2 = run()
        assert f2 == [("dgrad", 1), ("fwd", 1)], f2
    ref, mag = ref_conv_with_mag(torch.cat(xs, -1), w2, b, s, dy, tr)
    amag = util.ref_member_amag(xs, w2, b, s, tr) if len(kern.split("+")) > 1 else None
    assert_conv_close(y2, ref["y"], mag["y"], dtype, f"y after repack_all of {key}", amag=amag)
    for i, (g_, r_, m_) in enumerate(zip(dx2, _split(ref["dx"], cins), _split(mag["dx"], cins))):
        assert_conv_close(g_, r_, m_, dtype, f"dx[{i}] after repack_all of {key}")
    ops.drop_deferred(); ops.invalidate_panels(); torch.cuda.empty_cache()


@pytest.mark.gpu
def test_panel_first_met_after_a_captured_repack_is_not_served_stale(dev, monkeypatch):
    """A repack_all() recorded into a graph re-packs, at every replay, the panels registered when it was captured.  A geometry the
    weight first meets AFTER the capture (an evaluation at another batch size between replayed training steps) is not among them: its
    panel must not be cached across a replayed update.  Geometry A (N = 4) is registered before the capture, geometry B (N = 2) is
    first met after it; the weights then change through the raw buffer and ONE replay re-packs; both geometries must give the
    convolution of the new weights against fp64 -- A from its re-packed panel (packed = 1), B packed at the call (packed = 0)."""
    key = _key("m1_conv3d_fwd", 4, 10, 20, 20, (64,), 64, (3, 3, 3), (1, 1, 1))
    name, N, D, H, W, cins, cout, k, s, dts, fl, kern = key
    dtype = _DT[dts]
    g = _gen(dev, 4242)
    xs, w, b, dy = _conv_inputs(dev, dtype, N, (D, H, W), cins, cout, k, s, False, g)
    w2 = _as(0.7 * w + _randn(tuple(w.shape), g, dev, 0.7 / (sum(cins) * k[0] * k[1] * k[2]) ** 0.5), dtype)
    lib, flags = L.load(), []

    def wrap(*args, _fn=lib.m1_conv3d_fwd):
        flags.append(int(args[6]))
        return _fn(*args)
    monkeypatch.setattr(lib, "m1_conv3d_fwd", wrap)
    ws = w.clone().requires_grad_(True)                        # a leaf: its panels are cached on it and registered for repack_all
    xa, xb = xs[0], xs[0][:2].contiguous()

    def fwd(x):
        del flags[:]
        with torch.no_grad():
            y = ops.conv3d_same([x.to(dtype)], ws, b, k, s)
        torch.cuda.synchronize()
        return y, sorted(set(flags))
    panels = PKG.hip.panels
    try:
        with ops.config(M1_T3_MIN_BLOCKS=128):
            ops.invalidate_panels()
            assert fwd(xa)[1] == [0] and fwd(xa)[1] == [1]
            ops.repack_all()                                   # eager first: the table the capture records exists
            table = panels._PACK_TABLE[0]                      # (held here as well: the replay reads it through raw addresses)
            assert table is not None
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                ops.repack_all()
            torch.cuda.synchronize()
            yb0, fb0 = fwd(xb)                                 # first met after the capture
            assert fb0 == [0]
            with torch.no_grad():
                ws.data.copy_(w2)                              # the optimiser's way: no version bump
            gr.replay()
            torch.cuda.synchronize()
            ya, fa = fwd(xa)
            yb, fb = fwd(xb)
            still = panels._PACK_TABLE[0] is table             # (read here: leaving ops.config drops every panel)
        for what, x, y in (("A (registered before the capture)", xa, ya), ("B (first met after the capture)", xb, yb)):
            ref, mag = ref_conv_with_mag(x, w2, b, s, None, False)
            assert_conv_close(y, ref["y"], mag["y"], dtype, f"y of geometry {what} after a replayed repack_all")
        assert fa == [1] and fb == [0], (fa, fb)
        assert still                                           # the late geometry did not disturb the table the graph reads
    finally:
        ops.drop_deferred(); ops.invalidate_panels(); torch.cuda.empty_cache()
