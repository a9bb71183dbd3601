"""The non-conv kernels of the training step (InstanceNorm, SE combine, attention gate, softmax heads, focal loss, latent sample / KL,
dropout / cast, Adam-amsgrad) on the paths only large inputs reach, against plain fp64 references (util.ref_*):

* part 0 (no GPU): each fp64 reference equals the CPU oracle (oracle/m1_oracle.py) at two small shapes;
* part 1: the production paths forced at small sizes through the library's switches -- grid-stride loops that run many times
  (M1_EW_BLOCKS), many reduction chunks and the wide finalize kernel (M1_RED_BLOCKS, M1_FINP_WIDE), partial groups of samples,
  accumulation into pre-filled gradients, and a fused gate backward whose blocks loop over coarse voxels;
* part 2: the shapes the C3 bench step (and C5, where it differs) calls these ops at, against fp64 on the same device.

Tolerances (never fitted to observed errors):
* element-wise results: |got - ref| <= a*|ref| + b*rms(ref) per element.
  bf16 storage: a = 6 * 2^-9 -- one round-to-nearest of the stored result (unit roundoff 2^-8), plus one bf16 operand the kernel
  reads back in its rounded form (the gate's sigma and d(sigma)) that may sit one ulp (<= 2^-7) from the rounded fp64 value, plus fp32
  arithmetic (< 2^-16);
  b = 1e-3 covers results that cancel (IN backward, LeakyReLU near 0) where fp32 residue of the O(rms) terms stays below 2^-10.
  fp32: a = 1e-5 -- chains of ~20 fp32 roundings (2^-24 each, 1.2e-6) with a margin of ~8; b = 4e-6 -- the per-(n, c) sums an
  element consumes carry ~1e-6 relative error (fp32 partial sums of <= 2^10 terms) on terms of up to a few rms(ref).
* reductions (statistics, parameter gradients, the losses): |got - ref| <= 1e-5 * sum|term| of that sum; the inputs give every sum
  a bias (non-zero means, dy correlated with the normalised input, a slow ramp along D and H) so that sum|term| is within a small
  factor of |sum|, and one dropped, doubled or misplaced chunk among n moves the sum by ~1/n -- far above the tolerance.
"""
import ctypes
import math
import zlib

import numpy as np
import pytest
import torch

from oracle import m1_oracle as O
import util
from util import PKG, ops, assert_close_ew, assert_conv_close

A_BF, B_BF = 6 * 2.0 ** -9, 1e-3
A_32, B_32 = 1e-5, 4e-6
RED = 1e-5


def _ab(dtype):
    return (A_BF, B_BF) if dtype == torch.bfloat16 else (A_32, B_32)


def _assert_sum(got, ref, mag, what, rel=RED):
    """|got - ref| <= rel * mag per element of a vector of sums (mag = sum of |terms| of each)."""
    got, ref, mag = got.detach().double().reshape(-1), ref.detach().double().reshape(-1), mag.detach().double().reshape(-1)
    d = (got - ref).abs() - rel * mag
    k = int(torch.argmax(d))
    assert float(d[k]) <= 0.0 and bool(torch.isfinite(got).all()), \
        f"{what}: {int((d > 0).sum())} of {got.numel()} sums off; worst [{k}] got {float(got[k]):.9g} ref {float(ref[k]):.9g} " \
        f"sum|term| {float(mag[k]):.3g}"


# ---------------------------------------------------------------------------------------------------------------------------------
# host mirrors of the launch formulas (common.h m1_grid_for, reduce.h m1_red_chunkV): what a forcing setting makes the kernels do
# ---------------------------------------------------------------------------------------------------------------------------------
def grid_for(per, cg, cap):
    g = max(1, min(-(-per // 256), max(cap, 1)))
    need = cg // math.gcd(cg, 256)
    return -(-g // need) * need


def red_nchunks(V, C, N, red_blocks=512):
    per_block = max(16, 256 * 16 // (C if C < 256 else 256) if C >= 1 else 256 * 16)
    maxc = max(32, max(red_blocks, 1) // max(N, 1))
    chunk = min(max(per_block, -(-V // maxc)), V)
    return -(-V // chunk)


def lib_nchunks(N, V, C, nsums):
    """Chunk count the library sizes its reduction workspace for (m1_reduce_ws_floats = N*nchunks*C*nsums + N*C*nsums + 64)."""
    n = int(PKG.hip.lib.load().m1_reduce_ws_floats(N, V, C, nsums))
    return (n - 64 - N * C * nsums) // (N * C * nsums)


def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _randn(shape, g, dev, scale=1.0):
    return torch.randn(shape, generator=g, device=dev, dtype=torch.float32) * scale


def _ramp(shape, dev, amp=0.3):
    """A slow ramp along D and H of an NDHWC shape (broadcasts over N, W, C)."""
    D, H = shape[1], shape[2]
    d = torch.linspace(-1, 1, D, device=dev).view(1, D, 1, 1, 1)
    h = torch.linspace(-1, 1, H, device=dev).view(1, 1, H, 1, 1)
    return amp * (d + 0.5 * h)


def _as(t, dtype):
    """The value the kernel reads: rounded to the storage type, held in fp32."""
    return t.to(dtype).float()


# =================================================================================================================================
# part 0: the fp64 references against the CPU oracle (no GPU)
# =================================================================================================================================
SMALL = [(2, 3, 4, 5, 8), (1, 2, 6, 3, 5)]


def _o_grads(fn, ins, dy):
    ins = [t.clone().double().requires_grad_(True) for t in ins]
    y = fn(*ins)
    y.backward(dy.double())
    return y.detach(), [t.grad for t in ins]


def _same(a, b, tol=1e-12):
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).detach().double()
    assert a.shape == b.shape and float((a - b).abs().max()) <= tol * (1.0 + float(b.abs().max())), float((a - b).abs().max())


@pytest.mark.parametrize("shape", SMALL)
def test_reference_instnorm_matches_oracle(shape):
    x = util.rnd(shape, 1) * 2 + 0.5
    g, b = 1 + 0.2 * util.rnd(shape[-1:], 2), 0.3 * util.rnd(shape[-1:], 3)
    dy = util.rnd(shape, 4)
    for slope in (0.1, 1.0):
        yo, go = _o_grads(lambda x_, g_, b_: (lambda t: torch.where(t >= 0, t, slope * t))(O.instance_norm(x_, g_, b_)), [x, g, b], dy)
        yr, gr = _o_grads(lambda x_, g_, b_: util.ref_instnorm_act(x_, g_, b_, slope), [x, g, b], dy)
        _same(yr, yo)
        for a_, b_ in zip(gr, go):
            _same(a_, b_)
    xd = x.double()
    st = util.ref_in_stats(xd)
    _same(st[..., 0], xd.mean(dim=(1, 2, 3)))
    _same(st[..., 1], torch.rsqrt(xd.var(dim=(1, 2, 3), unbiased=False) + O.IN_EPS))


@pytest.mark.parametrize("shape", SMALL)
@pytest.mark.parametrize("variant", ["member", "ident", "dup"])
def test_reference_se_combine_matches_oracle(shape, variant):
    F_ = shape[-1]
    Fr = max(F_ // 4, 1)
    y3, y4 = util.rnd(shape, 1), util.rnd(shape, 2) * 1.5 + 0.2
    ps = [1 + 0.2 * util.rnd((F_,), 3), 0.5 * util.rnd((F_,), 4), 1 + 0.2 * util.rnd((F_,), 5), 0.5 * util.rnd((F_,), 6),
          util.rnd((1, 1, 1, F_, Fr), 7, 0.5), 0.1 * util.rnd((Fr,), 8), util.rnd((1, 1, 1, Fr, F_), 9, 0.5), 0.1 * util.rnd((F_,), 10)]
    rate = 0.5
    nout = 2 * shape[0] if variant == "dup" else shape[0]
    keep = (torch.from_numpy(np.random.default_rng(11).random((nout, *shape[1:]))) >= rate).double()
    dout = util.rnd((nout, *shape[1:]), 12)
    ident = variant == "ident"

    def oracle(y3_, y4_, g3, b3, g4, b4, W6, b6, W7, b7):
        x_ = O.instance_norm(y3_, g3, b3)
        rho = y4_ if ident else O.instance_norm(y4_, g4, b4)
        gp = x_.mean(dim=(1, 2, 3), keepdim=True)
        gp = torch.sigmoid(O.conv3d_same(O.lrelu(O.conv3d_same(gp, W6, b6, (1, 1, 1))), W7, b7, (1, 1, 1)))
        out = O.lrelu(x_ * gp * rho)
        if variant == "dup":
            out = torch.cat([out, out], 0)
        return O.dropout_with_mask(out, rate, keep)

    def ref(y3_, y4_, g3, b3, g4, b4, W6, b6, W7, b7):
        return util.ref_se_combine(y3_, y4_, g3, b3, None if ident else g4, None if ident else b4, W6, b6, W7, b7, rate, keep,
                                   dup=variant == "dup")
    yo, go = _o_grads(oracle, [y3, y4] + ps, dout)
    yr, gr = _o_grads(ref, [y3, y4] + ps, dout)
    _same(yr, yo)
    for k, (a_, b_) in enumerate(zip(gr, go)):
        if ident and k in (4, 5):
            continue                                      # (g4, b4 unused)
        _same(a_, b_)


@pytest.mark.parametrize("fine,coarse,ss", [((4, 6, 4), (2, 3, 2), (1, 1, 1)), ((2, 4, 4), (1, 1, 2), (1, 2, 2))])
def test_reference_gate_matches_oracle(fine, coarse, ss):
    N, C = 2, 8
    theta, phi = util.rnd((N, *fine, C), 1), util.rnd((N, *coarse, C), 2)
    w, b = util.rnd((1, 1, 1, C, 1), 3, 0.3), util.rnd((1,), 4)
    x = util.rnd((N, *[f * s for f, s in zip(fine, ss)], 5), 5)
    dy = util.rnd(tuple(x.shape), 6)
    up = [f // c for f, c in zip(fine, coarse)]

    def oracle(t_, p_, w_, b_, x_):
        sg = torch.sigmoid(O.conv3d_same(O.lrelu(t_ + O.upsample_nearest(p_, up)), w_, b_, (1, 1, 1)))
        return O.upsample_nearest(sg, ss) * x_
    yo, go = _o_grads(oracle, [theta, phi, w, b, x], dy)
    yr, gr = _o_grads(lambda *a: util.ref_gate_sigma_mul(*a, ss)[0], [theta, phi, w, b, x], dy)
    _same(yr, yo)
    for a_, b_ in zip(gr, go):
        _same(a_, b_)


@pytest.mark.parametrize("nc,N", [(2, 2), (3, 1)])
def test_reference_softmax_focal_latent_kl_match_oracle(nc, N):
    D, H, W = 2, 4, 4
    ups = [(1, 1, 1), (1, 2, 2), (2, 4, 4)]
    ls = [util.rnd((N, D // u[0], H // u[1], W // u[2], nc), 10 + i) for i, u in enumerate(ups)]
    dp = util.rnd((N, D, H, W, nc * len(ups)), 20)
    po, go = _o_grads(lambda *ts: torch.cat([torch.softmax(O.upsample_nearest(t, u), -1) for t, u in zip(ts, ups)], -1), ls, dp)
    pr, gr = _o_grads(lambda *ts: util.ref_softmax_heads(ts, ups), ls, dp)
    _same(pr, po)
    for a_, b_ in zip(gr, go):
        _same(a_, b_)
    # focal (incl. saturated probabilities)
    p = po.clone()
    p[0, 0, 0, 0, :nc] = torch.tensor([1.0] + [0.0] * (nc - 1), dtype=p.dtype)
    y = torch.nn.functional.one_hot(torch.randint(0, nc, (N, D, H, W), generator=torch.Generator().manual_seed(3)), nc).double()
    alpha = [0.75, 0.25, 0.5][:nc]
    for gamma in (2.0, 1.5):
        pa, pb = p.clone().requires_grad_(True), p.clone().requires_grad_(True)
        lo = O.focal_loss(y, pa, alpha, gamma); lo.backward()
        lr_ = util.ref_focal(y, pb, alpha, gamma); lr_.backward()
        _same(lr_, lo); _same(pb.grad, pa.grad)
    # latent sample / KL (log-sigma straddles the clip)
    L_ = 2
    mq, mp = util.rnd((N, D, H, W, 2 * L_), 1) * 0.2, util.rnd((N, D, H, W, 2 * L_), 2) * 0.2
    eps = util.rnd((N, D, H, W, L_), 3).double()
    dz = util.rnd((N, D, H, W, L_), 4)
    zo, go = _o_grads(lambda m_: m_[..., :L_] + torch.exp(torch.clamp(m_[..., L_:], -0.1, 0.1)) * eps, [mq], dz)
    zr, gr = _o_grads(lambda m_: util.ref_latent_sample(m_, eps), [mq], dz)
    _same(zr, zo); _same(gr[0], go[0])

    def kl_o(q_, p_):
        return O.kl_mvn_diag(q_[..., :L_], torch.clamp(q_[..., L_:], -0.1, 0.1), p_[..., :L_],
                             torch.clamp(p_[..., L_:], -0.1, 0.1)).sum(dim=(1, 2, 3)).mean().reshape(1)
    ko, go = _o_grads(kl_o, [mq, mp], torch.tensor([2.5]))
    kr, gr = _o_grads(util.ref_kl, [mq, mp], torch.tensor([2.5]))
    _same(kr, ko)
    for a_, b_ in zip(gr, go):
        _same(a_, b_)


@pytest.mark.parametrize("n,nk,nb", [(1003, 400, 200), (37, 13, 7)])
def test_reference_adam_matches_torch_amsgrad(n, nk, nb):
    """Keras Adam(amsgrad) == torch.optim.Adam(amsgrad) with eps_torch = eps / sqrt(1 - b2^t) (torch adds eps after the bias
    correction of sqrt(vhat)), the L2 gradient 2*lambda*w added to the gradient by hand."""
    p0, g = util.rnd((n,), 1).double(), util.rnd((n,), 2).double()
    lk, lb, gs, lr, b1, b2, eps = 1e-2, 3e-2, 0.5, 1e-2, 0.9, 0.999, 1e-7
    lam = torch.zeros(n, dtype=torch.float64); lam[:nk] = lk; lam[nk:nk + nb] = lb
    pt = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=lr, betas=(b1, b2), eps=eps, amsgrad=True)
    p, m, v, vh = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for t in range(1, 4):
        p, m, v, vh = util.ref_adam_amsgrad_step(p, g, m, v, vh, t, nk, nb, lk, lb, gs, lr, b1, b2, eps)
        pt.grad = gs * g + 2 * lam * pt.detach()
        opt.param_groups[0]["eps"] = eps / math.sqrt(1 - b2 ** t)
        opt.step()
        _same(p, pt.detach(), 1e-11)


def test_host_mirrors_of_the_launch_formulas():
    """The host mirrors behind part 1's forcing checks: grids are multiples of the channel-group count's share of 256 lanes, and the
    chunk count is what m1_reduce_ws_floats sizes (checked against the library by the GPU tests, lib_nchunks)."""
    for cg in (1, 2, 4, 5, 8, 12, 20, 48, 160, 384):
        for cap in (1, 3, 7, 2048):
            g = grid_for(10 ** 6, cg, cap)
            assert (g * 256) % cg == 0 and g >= min(cap, 10 ** 6 // 256)
    assert red_nchunks(20 * 160 * 160, 32, 4) == 128 and red_nchunks(5 * 10 * 10, 512, 4) == 32 and red_nchunks(4000, 8, 2) == 8


# =================================================================================================================================
# part 1: production paths forced at small sizes
# =================================================================================================================================
def _conv_input(dev, dtype, shape, g, mean, scale):
    """(x, stats) as the bench step hands them to the norms: x written by a 1x1x1 convolution, its (N, C, 2) {mean, rstd} from that
    convolution's epilogue.  x has a mean, a ramp along D and H and ~``scale`` spread."""
    C = shape[-1]
    h = _as(_randn(shape, g, dev) + 0.5 + _ramp(shape, dev), dtype)
    w = _randn((1, 1, 1, C, C), g, dev, scale / C ** 0.5)
    b = mean + 0.2 * _randn((C,), g, dev) - 0.5 * w.reshape(C, C).sum(0)
    with torch.no_grad():
        x, st = ops.conv3d_same([h.to(dtype)], w, b, (1, 1, 1), (1, 1, 1), stats=True)
    return x.float(), st


def _assert_stats(stats, x, what):
    """{mean, rstd} of x against fp64: bounds relative to the sums of |x| and x^2 behind them."""
    st = util.ref_in_stats(x.double())
    _assert_sum(stats[..., 0], st[..., 0], x.double().abs().mean(dim=(1, 2, 3)), what + " mean")
    var = 1.0 / st[..., 1] ** 2 - 1e-3
    _assert_sum(stats[..., 1], st[..., 1], st[..., 1] * x.double().square().mean(dim=(1, 2, 3)) / var, what + " rstd")


def _in_case(dev, dtype, shape, slope, seed, acc=False, step_stats=False):
    """HIP instnorm_act fwd + bwd vs fp64, inputs with a bias; returns nothing (asserts).  ``step_stats``: x and its statistics come
    from a convolution's epilogue, as in the bench step (network_blocks.py: the conv that writes x hands its stats to the norm)."""
    N, C = shape[0], shape[-1]
    g = _gen(dev, seed)
    st_in = None
    if step_stats:
        x, st_in = _conv_input(dev, dtype, shape, g, 0.8, 1.7)
        _assert_stats(st_in, x, f"conv-epilogue stats {shape}")
    else:
        x = _as(_randn(shape, g, dev, 1.7) + 0.8 + _ramp(shape, dev) + 0.2 * _randn((1, 1, 1, 1, C), g, dev), dtype)
    gam = 1 + 0.2 * _randn((C,), g, dev)
    bet = 0.3 + 0.2 * _randn((C,), g, dev)
    xr = x.double().requires_grad_(True)
    gr, br = gam.double().requires_grad_(True), bet.double().requires_grad_(True)
    yr = util.ref_instnorm_act(xr, gr, br, slope)
    dy = _as(yr.detach().float() + 0.5 + 0.7 * _randn(shape, g, dev), dtype)       # dy ~ the output: dgamma ~ sum xhat^2, dbeta ~ 0.5 V
    yr.backward(dy.double())
    xd = x.to(dtype).requires_grad_(True)
    gd, bd = gam.clone().requires_grad_(True), bet.clone().requires_grad_(True)
    pre_g, pre_b = None, None
    if acc:                                             # accumulate = 1: the gradient sinks of an optimiser's flat buffer
        pre_g, pre_b = 3.0 + _randn((C,), g, dev), -2.0 + _randn((C,), g, dev)
        gd._m1_gsink, bd._m1_gsink = pre_g.clone(), pre_b.clone()
    y = ops.instnorm_act(xd, gd, bd, slope, st_in)
    y.backward(dy.to(dtype))
    a, b = _ab(dtype)
    assert_close_ew(y, yr, a, b, what=f"IN y {shape} {dtype}")
    assert_close_ew(xd.grad, xr.grad, a, b, what=f"IN dx {shape} {dtype}")
    with torch.no_grad():
        st = util.ref_in_stats(x.double())
        xhat = (x.double() - st[:, None, None, None, :, 0]) * st[:, None, None, None, :, 1]
        z = xhat * gam.double() + bet.double()
        dz = dy.double() * torch.where(z >= 0, 1.0, slope)
        mg, mb = (dz * xhat).abs().sum(dim=(0, 1, 2, 3)), dz.abs().sum(dim=(0, 1, 2, 3))
    if acc:
        assert gd.grad is None and bd.grad is None
        _assert_sum(gd._m1_gsink, pre_g.double() + gr.grad, mg + pre_g.double().abs(), f"IN dgamma (acc) {shape}")
        _assert_sum(bd._m1_gsink, pre_b.double() + br.grad, mb + pre_b.double().abs(), f"IN dbeta (acc) {shape}")
    else:
        _assert_sum(gd.grad, gr.grad, mg, f"IN dgamma {shape} {dtype}")
        _assert_sum(bd.grad, br.grad, mb, f"IN dbeta {shape} {dtype}")
    _assert_stats(ops.instnorm_stats(x.to(dtype)), x, "IN")


# channel counts: every branch of the grid rounding -- need = cg / gcd(cg, 256) is 1 (8, 16, 32), 5 (C = 40 fp32 -> cg 10; 160 bf16
# -> cg 20), 3 (384 bf16 -> cg 48), and the scalar paths (5, 12: C % VEC != 0; cg = C)
EW_CHANNELS = [8, 16, 32, 40, 160, 384, 5, 12]


def _ew_shape(C, vec, cap):
    """A volume whose V*C/VEC vector items take >= 3 passes of the grid and are no multiple of it."""
    cgc = C // vec if C % vec == 0 else C
    gx = grid_for(1 << 40, cgc, cap)
    V = (3 * gx * 256) // cgc + 37
    return (2, 3, 7, -(-V // 21), C)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", EW_CHANNELS)
@pytest.mark.parametrize("cap", [1, 3, 7])
def test_instnorm_many_grid_stride_iterations(dev, dtype, C, cap):
    vec = 8 if dtype == torch.bfloat16 else 4
    shape = _ew_shape(C, vec, cap)
    cg = C // vec if C % vec == 0 else C
    per = shape[1] * shape[2] * shape[3] * (C // vec if C % vec == 0 else C)
    gx = grid_for(per, cg, cap)
    assert (gx * 256) % cg == 0 and per > 2 * gx * 256 and per % (gx * 256) != 0, (per, gx)
    with ops.config(M1_EW_BLOCKS=cap):
        assert ops.config_get("M1_EW_BLOCKS") == cap
        _in_case(dev, dtype, shape, 0.1, seed=C * 10 + cap)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 2, 4, 5])
@pytest.mark.parametrize("C,dtype", [(8, torch.bfloat16), (32, torch.float32), (160, torch.bfloat16), (12, torch.float32)])
@pytest.mark.parametrize("acc", [False, True])
def test_instnorm_many_chunks_wide_finalize(dev, N, C, dtype, acc):
    """Many small chunks (M1_RED_BLOCKS large: one chunk per ~16 elements per lane) folded by the wide finalize kernel (M1_FINP_WIDE=0),
    N = 5 leaves a partial group of NB = 4 samples; accumulate = 1 adds into pre-filled gradient sinks."""
    shape = (N, 4, 12, 100 + (C % 7), C)
    V = shape[1] * shape[2] * shape[3]
    with ops.config(M1_RED_BLOCKS=1 << 20, M1_FINP_WIDE=0, M1_EW_BLOCKS=3):
        nch = lib_nchunks(N, V, C, 2)
        assert nch == red_nchunks(V, C, N, 1 << 20) and nch >= 4, nch        # many chunks; > 0 = M1_FINP_WIDE -> the wide kernel
        _in_case(dev, dtype, shape, 0.1, seed=N * 100 + C, acc=acc)


def _se_case(dev, dtype, N, V3, F_, variant, rate, seed, layer_id=5, acc=False, step_inputs=False):
    """se_combine fwd + bwd vs fp64.  ``acc``: every parameter bound to a pre-filled gradient sink (the optimiser's flat buffer:
    accumulate = 1, the gate backward queued and run by ops.flush_deferred).  ``step_inputs``: y3 / y4 and their statistics from a
    convolution's epilogue and the gate precomputed by ops.se_gate_batch, as the bench step calls the op."""
    Fr = max(F_ // 8, 1)
    g = _gen(dev, seed)
    shp = (N, *V3, F_)
    ident, dup = variant == "ident", variant == "dup"
    s3 = s4 = None
    if step_inputs:
        y3, s3 = _conv_input(dev, dtype, shp, g, 0.4, 1.3)
        y4, s4 = _conv_input(dev, dtype, shp, g, -0.3, 1.1)
        _assert_stats(s3, y3, "conv-epilogue stats3"); _assert_stats(s4, y4, "conv-epilogue stats4")
    else:
        y3 = _as(_randn(shp, g, dev, 1.3) + 0.4 + _ramp(shp, dev), dtype)
        y4 = _as(_randn(shp, g, dev, 1.1) - 0.3 + _ramp(shp, dev), dtype)
    if ident:
        y4, s4 = _as(_randn(shp, g, dev, 0.8) + 1.0, dtype), None        # the block input: positive mean (sums stay dominated)
    # gate weights at fan-in scale (as the model initialises them): the gate stays off saturation, where fp32's sigmoid carries
    # 1 - g, and with it every gate gradient, to a relative precision of only 2^-24 / (1 - g)
    ps = [1 + 0.2 * _randn((F_,), g, dev), 0.5 + 0.2 * _randn((F_,), g, dev), 1 + 0.2 * _randn((F_,), g, dev),
          0.6 + 0.2 * _randn((F_,), g, dev), _randn((1, 1, 1, F_, Fr), g, dev, 1.0 / F_ ** 0.5), 0.1 * _randn((Fr,), g, dev),
          _randn((1, 1, 1, Fr, F_), g, dev, 1.0 / Fr ** 0.5), 0.1 * _randn((F_,), g, dev)]
    nout = 2 * N if dup else N
    rng = torch.tensor([4321, 9], dtype=torch.int64, device=dev)
    keep = None
    if rate > 0:
        keep = ops.dropout(torch.ones((nout, *V3, F_), device=dev, dtype=dtype), rate, rng, layer_id) != 0
    ins = [y3.double(), y4.double()] + [p.double() for p in ps]
    ins = [t.requires_grad_(True) for t in ins]
    args = ins[:4] + ([None, None] if ident else ins[4:6]) + ins[6:]
    inter = {}
    yr = util.ref_se_combine(*args, rate=rate, keep=keep, dup=dup, inter=inter)
    dout = _as(yr.detach().float() + 0.2 + 0.5 * _randn(tuple(yr.shape), g, dev), dtype)
    yr.backward(dout.double())
    d = [y3.to(dtype).requires_grad_(True), y4.to(dtype).requires_grad_(True)] + [p.clone().requires_grad_(True) for p in ps]
    used = [k for k in range(2, 10) if not (ident and k in (4, 5))]
    pre = {}
    if acc:
        for k in used:
            pre[k] = 2.0 + _randn(tuple(d[k].shape), g, dev)
            d[k]._m1_gsink = pre[k].clone()
    gate = ops.se_gate_batch([(d[3], d[6], d[7], d[8], d[9])])[0] if step_inputs else None
    out = ops.se_combine(d[0], d[1], d[2], d[3], None if ident else d[4], None if ident else d[5], d[6], d[7], d[8], d[9],
                         rate, rng if rate > 0 else None, layer_id, s3, s4, gate=gate, dup=dup)
    out.backward(dout.to(dtype))
    if acc:
        assert len(ops._SE_DEFER) == 1
        ops.flush_deferred()
    a, b = _ab(dtype)
    tag = f"SE {variant} {shp} {dtype} drop={rate}{' acc' if acc else ''}{' step-inputs' if step_inputs else ''}"
    assert_close_ew(out, yr, a, b, what=tag + " out")
    # the LeakyReLU's branch is decided on the fp32 product: where that product is within fp32 error of 0 the two branches are both
    # right and the data gradients may differ by the slope (0.9 of the term); those elements are left out of dy3 / dy4
    with torch.no_grad():
        prod = inter["prod"].detach()
        tie = prod.abs() <= 1e-5 * prod.square().mean().sqrt()
    for k, nm in ((0, "dy3"), (1, "dy4")):
        assert_close_ew(torch.where(tie, 0.0, d[k].grad.double()), torch.where(tie, 0.0, ins[k].grad), a, b, what=tag + " " + nm)
    # parameter gradients against sum|term|: g3 / b3 = sums over (n, v) of G3 * xhat3 / G3 (G3 = dL/dx_, the IN3 output, gate path
    # included); g4 / b4 the same with G4 = dL/drho; the gate's parameters from the terms of dL/dgate = sum_v Gp * x_ * rho (Gp =
    # dL/dprod) carried through the gate's small contractions with absolute values
    with torch.no_grad():
        dims = (0, 1, 2, 3)
        x_, G3, Gp = inter["x_"].detach(), inter["x_"].grad, inter["prod"].grad
        xh3 = (x_ - ins[3].detach()) / ins[2].detach()
        # the kernels expand x_ = g3 xhat3 + b3 and rho = g4 xhat4 + b4 inside their per-channel sums: the terms are bounded by
        # A3 = |g3 xhat3| + |b3| and A4 = |g4 xhat4| + |b4| (|rho| for the identity residual) in place of |x_| and |rho|
        rho = inter["rho"].detach()
        Gg = (Gp * inter["gate"].detach()).abs()
        A3 = (ins[2].detach() * xh3).abs() + ins[3].detach().abs()
        if ident:
            A4 = rho.abs()
        else:
            xh4 = (rho - ins[5].detach()) / ins[4].detach()
            A4 = (ins[4].detach() * xh4).abs() + ins[5].detach().abs()
        mag = {2: (Gg * xh3.abs() * A4).abs().sum(dims), 3: (Gg * A4).sum(dims)}
        if not ident:
            mag[4], mag[5] = (Gg * A3 * xh4.abs()).sum(dims), (Gg * A3).sum(dims)
        W6, b6, W7 = (t.detach().reshape(t.shape[-2], t.shape[-1]) if t.dim() > 1 else t.detach() for t in ins[6:9])
        gp = x_.mean(dim=(1, 2, 3))
        z6 = gp @ W6 + b6
        hdn = util.ref_lrelu(z6)
        sg = inter["gate"].detach()[:, 0, 0, 0, :]
        tg = (Gp.abs() * A3 * A4).sum(dim=(1, 2, 3))                   # (prod is taken once for both halves of the dup form)
        m7 = tg * sg * (1 - sg)                                         # |terms| of dL/dz7 per (n, f)
        m6 = (m7 @ W7.abs().T) * torch.where(z6 >= 0, 1.0, 0.1)        # ... of dL/dz6 per (n, r)
        mag[6], mag[7] = (gp.abs().T @ m6).reshape(ins[6].shape), m6.sum(0)
        # (the hidden unit h = lrelu(b3 . W6 + b6) is an fp32 dot product over F terms: its error is bounded by F 2^-24 of the sum of
        # its |terms| (gamma_F), which matters where h cancels to near 0; dW7 = sum_n h dz7 carries that error)
        Hm = (gp.abs() @ W6.abs() + b6.abs()) * (F_ * 2.0 ** -24 / RED)
        mag[8], mag[9] = ((hdn.abs() + Hm).T @ m7).reshape(ins[8].shape), m7.sum(0)
        mag[3] = mag[3] + (m6 @ W6.abs().T).sum(0)                     # beta3 also feeds the gate (GAP of the IN3 output)
    names = "y3 y4 g3 b3 g4 b4 W6 b6 W7 b7".split()
    for k in used:
        ref = ins[k].grad
        if acc:
            assert d[k].grad is None
            _assert_sum(d[k]._m1_gsink, pre[k].double() + ref, mag[k] + pre[k].double().abs(), f"{tag} d{names[k]} (acc)")
        else:
            _assert_sum(d[k].grad, ref, mag[k], f"{tag} d{names[k]}")


SE_CHANNELS = [8, 16, 32, 40, 160, 384, 12]


# (the duplicating form needs whole 16-byte channel vectors: ops.se_combine raises on bf16 F = 12)
SE_CASES = [(dt, F_, v, r) for dt in (torch.float32, torch.bfloat16) for F_ in SE_CHANNELS
            for v, r in (("member", 0.0), ("ident", 0.5), ("dup", 0.5)) if not (v == "dup" and F_ % (8 if dt == torch.bfloat16 else 4))]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,F_,variant,rate", SE_CASES)
def test_se_combine_many_iterations_many_chunks(dev, dtype, F_, variant, rate):
    vec = 8 if dtype == torch.bfloat16 else 4
    V3 = (3, 9, max(2400 // F_, 4) + 1)
    N = 5 if variant == "member" else 2
    V = V3[0] * V3[1] * V3[2]
    cg = F_ // vec if F_ % vec == 0 else F_
    per = V * cg
    with ops.config(M1_EW_BLOCKS=3, M1_RED_BLOCKS=1 << 20, M1_FINP_WIDE=0):
        gx = grid_for(per, cg, 3)
        assert per > 2 * gx * 256 and (gx * 256) % cg == 0, (per, gx)
        assert lib_nchunks(N, V, F_, 5) >= 4
        _se_case(dev, dtype, N, V3, F_, variant, rate, seed=F_ + len(variant))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("variant,N", [("member", 5), ("ident", 2), ("dup", 2)])
def test_se_combine_accumulates_into_gradient_sinks(dev, dtype, variant, N):
    """accumulate = 1 for every SE parameter gradient (g3 b3 g4 b4 through the wide finalize, W6 b6 W7 b7 through the queued gate
    backward) into pre-filled sinks, under many chunks and looping grids."""
    V3 = (3, 9, 41)
    with ops.config(M1_EW_BLOCKS=3, M1_RED_BLOCKS=1 << 20, M1_FINP_WIDE=0):
        assert lib_nchunks(N, V3[0] * V3[1] * V3[2], 32, 5) >= 4
        _se_case(dev, dtype, N, V3, 32, variant, 0.5 if variant != "member" else 0.0, seed=N + len(variant), acc=True)


def _gate_case(dev, dtype, N, tdims, pdims, Ci, Cx, ss, seed, acc=False):
    """gate_sigma_mul fwd + bwd (fused when the shapes allow) vs fp64; returns the number of coarse voxels.  ``acc``: w_psi and b_psi
    bound to pre-filled gradient sinks (accumulate = 1 in the fold of the partial rows)."""
    g = _gen(dev, seed)
    xdims = tuple(t * s for t, s in zip(tdims, ss))
    theta = _as(_randn((N, *tdims, Ci), g, dev) + 0.3 + _ramp((N, *tdims, Ci), dev), dtype)
    phi = _as(_randn((N, *pdims, Ci), g, dev) + 0.2, dtype)
    x = _as(_randn((N, *xdims, Cx), g, dev) + 0.5, dtype)
    w, b = _randn((1, 1, 1, Ci, 1), g, dev, 0.3) + 0.05, _randn((1,), g, dev)
    ins = [t.double().requires_grad_(True) for t in (theta, phi, w, b, x)]
    yr, sr = util.ref_gate_sigma_mul(*ins[:4], ins[4], ss, sigma_dtype=dtype)
    dy = _as(yr.detach().float() + 0.3 + 0.5 * _randn(tuple(yr.shape), g, dev), dtype)
    yr.backward(dy.double())
    d = [t.to(dtype).requires_grad_(True) for t in (theta, phi)] + [w.clone().requires_grad_(True), b.clone().requires_grad_(True)] + \
        [x.to(dtype).requires_grad_(True)]
    pre = []
    if acc:
        pre = [1.0 + _randn(tuple(d[k].shape), g, dev) for k in (2, 3)]
        d[2]._m1_gsink, d[3]._m1_gsink = pre[0].clone(), pre[1].clone()
    y, sg = ops.gate_sigma_mul(d[0], d[1], d[2], d[3], d[4], ss)
    y.backward(dy.to(dtype))
    a, bb = _ab(dtype)
    tag = f"gate {N}x{tdims}/{pdims} Ci={Ci} Cx={Cx} ss={ss} {dtype}"
    assert_close_ew(sg, sr, a, bb, what=tag + " sigma")
    assert_close_ew(y, yr, a, bb, what=tag + " y")
    assert_close_ew(d[4].grad, ins[4].grad, a, bb, what=tag + " dx")
    with torch.no_grad():
        up = [t // p for t, p in zip(tdims, pdims)]
        sgd = util.ref_gate_sigma(*[t.detach() for t in ins[:4]])
        if dtype == torch.bfloat16:
            sgd = sgd.to(dtype).double()
        dsig = (dy.double() * ins[4].detach()).reshape(N, tdims[0], ss[0], tdims[1], ss[1], tdims[2], ss[2], Cx).sum(dim=(2, 4, 6, 7))
        dpsi = dsig * sgd * (1 - sgd)
        f = util.ref_lrelu(ins[0].detach() + util.ref_upsample(ins[1].detach(), up))
        # a stored sigma one bf16 ulp (2^-8) off the rounded fp64 value moves s (1 - s) by |1 - 2 s| 2^-8: d(theta) = D s (1 - s),
        # D = d(sigma) w lrelu'(f), is bounded with |D (1 - 2 s)| added to its magnitude (a >= 2^-8)
        mag_t = ins[0].grad.abs()
        if dtype == torch.bfloat16:
            mag_t = mag_t + (dsig * (1 - 2 * sgd)).abs().unsqueeze(-1) * (ins[2].detach().reshape(-1) * torch.where(f >= 0, 1.0, 0.1)).abs()
        # d(phi) = window sum of d(theta): bounded by the window sum of those magnitudes
        mag = mag_t.reshape(N, pdims[0], up[0], pdims[1], up[1], pdims[2], up[2], Ci).sum(dim=(2, 4, 6))
        # d(psi) per theta voxel and f: the terms of d(w_psi) and d(b_psi)
        mw, mb = (dpsi.unsqueeze(-1) * f).abs().sum(dim=(0, 1, 2, 3)), dpsi.abs().sum().reshape(1)
    assert_close_ew(d[0].grad, ins[0].grad, a, bb, mag=mag_t, what=tag + " dtheta")
    assert_close_ew(d[1].grad, ins[1].grad, a, bb, mag=mag, what=tag + " dphi")
    # the reference reads the stored (rounded) sigma and d(sigma) as the kernels do: what remains is fp32 accumulation, and the rare
    # voxel whose fp32 d(sigma) rounds to the other bf16 neighbour (2^-8 of one term) -- the fp32 bound holds for both types
    if acc:
        assert d[2].grad is None and d[3].grad is None
        _assert_sum(d[2]._m1_gsink.reshape(-1), pre[0].double().reshape(-1) + ins[2].grad.reshape(-1), mw + pre[0].double().abs().reshape(-1),
                    tag + " dw_psi (acc)")
        _assert_sum(d[3]._m1_gsink, pre[1].double() + ins[3].grad, mb + pre[1].double().abs(), tag + " db_psi (acc)")
    else:
        _assert_sum(d[2].grad.reshape(-1), ins[2].grad.reshape(-1), mw, tag + " dw_psi")
        _assert_sum(d[3].grad, ins[3].grad, mb, tag + " db_psi")
    return int(np.prod(pdims)) * N


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N,tdims,pdims,Ci,Cx,ss,acc", [(2, (4, 32, 32), (2, 32, 32), 8, 16, (1, 1, 1), False),
                                                        (3, (2, 40, 40), (2, 20, 20), 16, 8, (1, 2, 2), True),
                                                        (1, (4, 64, 40), (4, 32, 40), 8, 8, (1, 1, 1), False)])
def test_gate_fused_backward_blocks_loop(dev, dtype, N, tdims, pdims, Ci, Cx, ss, acc):
    """The fused gate backward launches min(4096, workspace rows, coarse voxels) blocks; M1_RED_BLOCKS=1 shrinks the workspace
    (32 chunks per sample) so that every block strides over many coarse voxels, and M1_EW_BLOCKS=2 makes the element-wise product
    passes loop as well."""
    Vt = int(np.prod(tdims))
    with ops.config(M1_RED_BLOCKS=1, M1_EW_BLOCKS=2, M1_GATE_FWD_FUSED=1, M1_GATE_MUL_BWD_FUSED=1, M1_GATE_BWD_FUSED=1):
        rows = min(4096, int(PKG.hip.lib.load().m1_reduce_ws_floats(N, Vt, Ci, 2)) // (Ci * 2))
        nvox = int(np.prod(pdims)) * N
        assert nvox >= 4 * rows, (nvox, rows)               # every block covers >= 4 coarse voxels
        _gate_case(dev, dtype, N, tdims, pdims, Ci, Cx, ss, seed=Ci + N, acc=acc)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gate_fused_backward_default_switches_many_voxels_per_block(dev, dtype):
    """More than 4096 * N coarse voxels at the default switches: the block count is the reduction workspace's row count (about
    M1_RED_BLOCKS + N rows: the 4096-block cap of the launch cannot bind at the default of 512), every block strides over many coarse
    voxels."""
    N, tdims, pdims = 2, (4, 64, 80), (4, 64, 80)
    Vt = int(np.prod(tdims))
    rows = int(PKG.hip.lib.load().m1_reduce_ws_floats(N, Vt, 8, 2)) // 16
    nvox = int(np.prod(pdims)) * N
    assert rows < 4096 and nvox > 4096 * N and nvox >= 100 * rows, (rows, nvox)
    _gate_case(dev, dtype, N, tdims, pdims, 8, 8, (1, 1, 1), seed=77)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,dims,ss", [(8, (4, 16, 16), (1, 1, 1)), (40, (2, 12, 12), (1, 2, 2)), (5, (4, 8, 8), (2, 2, 2))])
def test_mul_sigma_many_grid_stride_iterations(dev, dtype, C, dims, ss):
    N = 2
    g = _gen(dev, C)
    x = _as(_randn((N, *dims, C), g, dev) + 0.4, dtype)
    sig = _as(torch.sigmoid(_randn((N, *[d // s for d, s in zip(dims, ss)]), g, dev)), dtype)
    dy = _as(_randn((N, *dims, C), g, dev) + 0.3, dtype)
    xr, sr = x.double().requires_grad_(True), sig.double().requires_grad_(True)
    yr = util.ref_upsample(sr.unsqueeze(-1), ss) * xr
    yr.backward(dy.double())
    with ops.config(M1_EW_BLOCKS=1):
        xd, sd = x.to(dtype).requires_grad_(True), sig.to(dtype).requires_grad_(True)
        y = ops.mul_sigma(xd, sd, ss)
        y.backward(dy.to(dtype))
    a, b = _ab(dtype)
    assert_close_ew(y, yr, a, b, what="mul_sigma y")
    assert_close_ew(xd.grad, xr.grad, a, b, what="mul_sigma dx")
    mag = (dy.double() * x.double()).abs().reshape(N, dims[0] // ss[0], ss[0], dims[1] // ss[1], ss[1], dims[2] // ss[2], ss[2], C).sum(dim=(2, 4, 6, 7))
    assert_close_ew(sd.grad, sr.grad, a, b, mag=mag, what="mul_sigma dsigma")


# =================================================================================================================================
# part 2: the bench step's own shapes against fp64 on the GPU
# =================================================================================================================================
def _dt(t):
    return "bf16" if t.dtype == torch.bfloat16 else "fp32"


def _key_of(name, args, kwargs):
    """(op, N, D, H, W, C, dtype, variant) of one call of an ops entry point the model makes."""
    a = list(args)
    if name == "instnorm_act":
        x = a[0]; slope = a[3] if len(a) > 3 else kwargs.get("slope", 1.0)
        st = (a[4] if len(a) > 4 else kwargs.get("stats")) is not None
        return ("instnorm_act", *x.shape, _dt(x), f"slope={float(slope):g},stats={int(st)}")
    if name == "se_combine":
        y3 = a[0]; rate = a[10] if len(a) > 10 else kwargs.get("drop_rate", 0.0)
        var = ("ident" if a[4] is None else ("dup" if kwargs.get("dup") else "member"))
        st = (a[13] if len(a) > 13 else kwargs.get("stats3")) is not None
        gt = (a[15] if len(a) > 15 else kwargs.get("gate")) is not None
        return ("se_combine", *y3.shape, _dt(y3), f"{var},Fr={int(a[6].shape[-1])},drop={float(rate):g},stats={int(st)},gate={int(gt)}")
    if name == "gate_sigma_mul":
        th, ph, x = a[0], a[1], a[4]; ss = tuple(a[5]) if len(a) > 5 else tuple(kwargs.get("ss", (1, 1, 1)))
        return ("gate_sigma_mul", *x.shape, _dt(x), f"theta={tuple(th.shape[1:])},phi={tuple(ph.shape[1:4])},ss={ss}")
    if name == "softmax_heads":
        ls, ups = a[0], a[1]
        return ("softmax_heads", *ls[0].shape, _dt(ls[0]), f"ups={tuple(tuple(int(v) for v in u) for u in ups)}")
    if name == "focal_loss":
        y, p = a[0], a[1]
        return ("focal_loss", *p.shape, _dt(y), f"nc={int(y.shape[-1])}")
    if name == "latent_sample":
        ml = a[0]; mean = a[2]; stacked = a[3] if len(a) > 3 else kwargs.get("stacked", False)
        mode = "mean" if mean else ("rng" if a[1] is None else "eps") + (",stacked" if stacked else "")
        return ("latent_sample", *ml.shape, _dt(ml), mode)
    if name == "kl_mvn_diag":
        q = a[0]; first = a[2] if len(a) > 2 else kwargs.get("first")
        return ("kl_mvn_diag", *q.shape, _dt(q), f"first={first}")
    if name in ("dropout", "cast"):
        x = a[0]
        return (name, int(x.numel()), 1, 1, 1, 1, _dt(x), f"rate={float(a[1]):g}" if name == "dropout" else f"to={a[1]}")
    raise KeyError(name)


RECORDED = ("instnorm_act", "se_combine", "gate_sigma_mul", "softmax_heads", "focal_loss", "latent_sample", "kl_mvn_diag", "dropout", "cast")


def record_c3_bench_keys(dev, monkeypatch):
    """One forward + backward of the C3 bench configuration (test_full_size.c3_bench_model, batch 2, drawn latents), every call of
    the recorded ops entry points noted by its key."""
    from test_full_size import c3_bench_model, _box_target
    seen = set()
    for name in RECORDED:
        fn = getattr(ops, name)

        def wrap(*args, _fn=fn, _name=name, **kwargs):
            seen.add(_key_of(_name, args, kwargs))
            return _fn(*args, **kwargs)
        monkeypatch.setattr(ops, name, wrap)
    dims = (20, 160, 160)
    m = c3_bench_model(dev)
    tgt = torch.cat([_box_target(dims), _box_target(dims).roll(17, dims=2)], dim=0).to(dev)
    x = util.rnd((2, *dims, 3), 11)
    x[..., 2] = tgt[..., 1].cpu()
    x = ops.cast(x.to(dev).contiguous(), torch.bfloat16)
    opt = PKG.optim.Adam(learning_rate=1e-3, amsgrad=True)
    focal = PKG.losses.Focal(alpha=[0.75, 0.25], gamma=2.0).loss
    m.compile(optimizer=opt, loss=[focal, PKG.losses.EvidenceLowerBound().loss], loss_weights=[1.0, 10.0])
    m.train()
    opt.zero_grad()
    det, kl = m(x)
    (focal(tgt, det) + 10.0 * kl.sum()).backward()
    opt.flatp.gather_grads()
    torch.cuda.synchronize()
    return seen, sum(p.numel() for p in m.parameters())


# (op, N, D, H, W, C, dtype, variant) of every call of the recorded ops entry points in one forward + backward of the C3 bench
# configuration (bf16, batch 2 stacked to 4 where the passes are stacked, dropout 0.5 fused into the SE blocks, drawn latents);
# test_c3_bench_keys_are_in_the_table keeps it current.  cast / dropout: (op, numel, 1, 1, 1, 1, dtype, variant).
C3_KEYS = [
    ('cast', 3072000, 1, 1, 1, 1, 'fp32', 'to=torch.bfloat16'),
    ('focal_loss', 2, 20, 160, 160, 2, 'fp32', 'nc=2'),
    ('gate_sigma_mul', 2, 20, 160, 160, 32, 'bf16', 'theta=(20, 160, 160, 32),phi=(5, 10, 10),ss=(1, 1, 1)'),
    ('gate_sigma_mul', 2, 20, 80, 80, 64, 'bf16', 'theta=(20, 80, 80, 64),phi=(5, 10, 10),ss=(1, 1, 1)'),
    ('gate_sigma_mul', 4, 10, 20, 20, 256, 'bf16', 'theta=(10, 20, 20, 256),phi=(5, 10, 10),ss=(1, 1, 1)'),
    ('gate_sigma_mul', 4, 20, 40, 40, 128, 'bf16', 'theta=(20, 40, 40, 128),phi=(5, 10, 10),ss=(1, 1, 1)'),
    ('instnorm_act', 2, 20, 160, 160, 32, 'bf16', 'slope=0.1,stats=1'),
    ('instnorm_act', 2, 20, 160, 160, 32, 'bf16', 'slope=1,stats=1'),
    ('instnorm_act', 2, 20, 160, 160, 8, 'bf16', 'slope=0.1,stats=1'),
    ('instnorm_act', 2, 20, 40, 40, 32, 'bf16', 'slope=0.1,stats=1'),
    ('instnorm_act', 2, 20, 80, 80, 16, 'bf16', 'slope=0.1,stats=1'),
    ('instnorm_act', 2, 20, 80, 80, 64, 'bf16', 'slope=1,stats=1'),
    ('instnorm_act', 4, 10, 20, 20, 256, 'bf16', 'slope=1,stats=1'),
    ('instnorm_act', 4, 10, 20, 20, 64, 'bf16', 'slope=0.1,stats=1'),
    ('instnorm_act', 4, 20, 40, 40, 128, 'bf16', 'slope=1,stats=1'),
    ('instnorm_act', 4, 20, 40, 40, 32, 'bf16', 'slope=0.1,stats=1'),
    ('instnorm_act', 4, 5, 10, 10, 128, 'bf16', 'slope=0.1,stats=1'),
    ('kl_mvn_diag', 4, 10, 20, 20, 4, 'bf16', 'first=2'),
    ('kl_mvn_diag', 4, 20, 40, 40, 2, 'bf16', 'first=2'),
    ('kl_mvn_diag', 4, 5, 10, 10, 6, 'bf16', 'first=2'),
    ('latent_sample', 4, 10, 20, 20, 4, 'bf16', 'rng,stacked'),
    ('latent_sample', 4, 20, 40, 40, 2, 'bf16', 'rng,stacked'),
    ('latent_sample', 4, 5, 10, 10, 6, 'bf16', 'rng,stacked'),
    ('se_combine', 2, 20, 160, 160, 32, 'bf16', 'member,Fr=4,drop=0.5,stats=1,gate=1'),
    ('se_combine', 2, 20, 40, 40, 128, 'bf16', 'member,Fr=16,drop=0.5,stats=1,gate=1'),
    ('se_combine', 2, 20, 80, 80, 64, 'bf16', 'dup,Fr=8,drop=0.5,stats=1,gate=1'),
    ('se_combine', 2, 20, 80, 80, 64, 'bf16', 'member,Fr=8,drop=0.5,stats=1,gate=1'),
    ('se_combine', 4, 10, 20, 20, 256, 'bf16', 'member,Fr=32,drop=0.5,stats=1,gate=1'),
    ('se_combine', 4, 20, 40, 40, 128, 'bf16', 'member,Fr=16,drop=0.5,stats=1,gate=1'),
    ('se_combine', 4, 5, 10, 10, 512, 'bf16', 'member,Fr=64,drop=0.5,stats=1,gate=1'),
    ('softmax_heads', 2, 20, 160, 160, 2, 'bf16', 'ups=((1, 1, 1),)'),
]
# cases the bench step reaches that its recorded calls do not show: 4 softmax heads and the stacked batch of 4 (the 4096-block grid
# loops only from N = 4 on), focal loss over 4 heads at batch 2 and 4, an fp32 (C5) normalisation and SE block at full size
EXTRA_KEYS = [
    ("softmax_heads", 4, 20, 160, 160, 2, "bf16", "ups=((1, 1, 1), (1, 2, 2), (1, 4, 4), (2, 8, 8))"),
    ("softmax_heads", 1, 32, 256, 256, 2, "fp32", "ups=((1, 1, 1),)"),
    ("focal_loss", 2, 20, 160, 160, 8, "fp32", "nc=2"),
    ("focal_loss", 4, 20, 160, 160, 8, "bf16", "nc=2"),
    ("instnorm_act", 1, 32, 256, 256, 32, "fp32", "slope=0.1,stats=1"),
    ("se_combine", 1, 32, 256, 256, 32, "fp32", "member,Fr=4,drop=0,stats=1,gate=1"),
    ("kl_mvn_diag", 4, 20, 40, 40, 2, "fp32", "first=2"),
]
_DT = {"bf16": torch.bfloat16, "fp32": torch.float32}


def _softmax_case(dev, dtype, N, D, H, W, nc, ups, seed):
    g = _gen(dev, seed)
    ls = [_as(_randn((N, D // u[0], H // u[1], W // u[2], nc), g, dev, 2.0), dtype) for u in ups]
    lr_ = [t.double().requires_grad_(True) for t in ls]
    pr = util.ref_softmax_heads(lr_, ups)
    dp = _randn(tuple(pr.shape), g, dev) + pr.detach().float()
    pr.backward(dp.double())
    ld = [t.to(dtype).requires_grad_(True) for t in ls]
    p = ops.softmax_heads(ld, ups)
    p.backward(dp)
    assert_close_ew(p, pr, A_32, B_32, what="softmax probs")            # (fp32 output of bf16 / fp32 logits)
    a, b = _ab(dtype)
    for k, (x_, r_) in enumerate(zip(ld, lr_)):
        # the gradient of a coarse head sums its upsampling window: bounded by the window's sum of |terms|
        u = ups[k]
        pk = pr.detach()[..., k * nc:(k + 1) * nc]
        t = (dp.double()[..., k * nc:(k + 1) * nc] * pk).abs() + pk * (dp.double()[..., k * nc:(k + 1) * nc] * pk).sum(-1, keepdim=True).abs()
        mag = t.reshape(N, D // u[0], u[0], H // u[1], u[1], W // u[2], u[2], nc).sum(dim=(2, 4, 6))
        assert_close_ew(x_.grad, r_.grad, a, b, mag=mag, what=f"softmax dlogits head {k}")


def _focal_case(dev, ydt, N, D, H, W, nheads, nc, seed, alpha=(0.75, 0.25), gamma=2.0):
    g = _gen(dev, seed)
    p = torch.softmax(3.0 * _randn((N, D, H, W, nheads, nc), g, dev), dim=-1)
    p[0, 0, 0, 0, 0] = torch.tensor([1.0] + [0.0] * (nc - 1), device=dev)          # saturated: outside the clip range
    p[-1, 1, 2, 3, -1] = torch.tensor([0.0] * (nc - 1) + [1.0], device=dev)
    p = p.reshape(N, D, H, W, nheads * nc)
    cls = (torch.rand((N, D, H, W), generator=g, device=dev) < 0.3).long()
    y = torch.nn.functional.one_hot(cls, nc).float()
    pr = p.double().requires_grad_(True)
    terms = util.ref_focal_terms(y.double(), pr, alpha, gamma)
    lr_ = terms.sum(dim=(1, 2, 3)).mean()
    (3.0 * lr_).backward()
    pd = p.clone().requires_grad_(True)
    ld = ops.focal_loss(y.to(ydt), pd, alpha, gamma)
    (3.0 * ld).backward()
    _assert_sum(ld.reshape(1), lr_.reshape(1), terms.detach().abs().sum(dim=(1, 2, 3)).mean().reshape(1), f"focal loss {N}x{nheads}")
    assert_close_ew(pd.grad, pr.grad, A_32, B_32, what="focal dprobs")


def _kl_case(dev, dtype, N, D, H, W, C, first, seed):
    g = _gen(dev, seed)
    L_ = C // 2
    mq = _as(torch.cat([_randn((N, D, H, W, L_), g, dev) + 0.3, 0.08 * _randn((N, D, H, W, L_), g, dev)], -1), dtype)
    mp = _as(torch.cat([_randn((N, D, H, W, L_), g, dev) - 0.2, 0.08 * _randn((N, D, H, W, L_), g, dev)], -1), dtype)
    qr, pr = mq.double().requires_grad_(True), mp.double().requires_grad_(True)
    terms = util.ref_kl_terms(qr, pr, first)
    kr = terms.sum(dim=(1, 2, 3)).mean().reshape(1)
    kr.backward(torch.full((1,), 2.5, dtype=torch.float64, device=dev))
    qd, pd = mq.to(dtype).requires_grad_(True), mp.to(dtype).requires_grad_(True)
    k = ops.kl_mvn_diag(qd, pd, first=first)
    k.backward(torch.full((1,), 2.5, device=dev))
    _assert_sum(k, kr, terms.detach().abs().sum(dim=(1, 2, 3)).mean().reshape(1), "KL")
    a, b = _ab(dtype)
    assert_close_ew(qd.grad, qr.grad, a, b, what="KL dq")
    assert_close_ew(pd.grad, pr.grad, a, b, what="KL dp")


def _latent_rng_case(dev, dtype, N, D, H, W, C, seed):
    """Stacked in-kernel draws: the prob_mean half is mu exactly; the sampling half is mu + sigma * eps with eps the draw implied by z,
    and the backward is the fp64 derivative at that draw: d mu = dz, d logsigma = dz * sigma * eps inside the clip band."""
    g = _gen(dev, seed)
    L_ = C // 2
    ml = _as(torch.cat([_randn((N, D, H, W, L_), g, dev), 0.08 * _randn((N, D, H, W, L_), g, dev)], -1), dtype)
    rng = torch.tensor([1234, 7], dtype=torch.int64, device=dev)
    mld = ml.to(dtype).requires_grad_(True)
    z = ops.latent_sample(mld, None, False, stacked=True, rng=rng, stream_id=3)
    h = N // 2
    assert torch.equal(z[h:], ml.to(dtype)[h:, ..., :L_])
    sig = torch.exp(torch.clamp(ml.double()[..., L_:], -0.1, 0.1))
    eps = (z.detach().double() - ml.double()[..., :L_]) / sig
    assert float(eps[:h].abs().max()) < 7.0
    dz = _as(_randn(tuple(z.shape), g, dev), dtype)
    z.backward(dz.to(dtype))
    mr = ml.double().requires_grad_(True)
    zr = torch.cat([util.ref_latent_sample(mr[:h], eps[:h]), mr[h:, ..., :L_]], 0)
    zr.backward(dz.double())
    a, b = _ab(dtype)
    # the implied draw carries the rounding of the stored z (<= 2^-8 |z|): d logsigma = dz * (z - mu) is bounded by |dz| (|z| + |mu|)
    mag = mr.grad.detach().abs().clone()
    mag[:h, ..., L_:] += dz[:h].double().abs() * (z.detach()[:h].double().abs() + ml[:h, ..., :L_].double().abs())
    assert_close_ew(mld.grad, mr.grad, a, b, mag=mag, what="latent dml")


def _run_key(dev, key, seed):
    op, N, D, H, W, C, dts, var = key
    dtype = _DT[dts]
    kv = dict(f.split("=", 1) for f in var.split(",") if "=" in f and not f.startswith(("theta", "phi", "ss", "ups")))
    if op == "instnorm_act":
        _in_case(dev, dtype, (N, D, H, W, C), float(kv["slope"]), seed, step_stats=kv.get("stats") == "1")
    elif op == "se_combine":
        # (stats and gate are supplied together by the step: one flag drives both)
        _se_case(dev, dtype, N, (D, H, W), C, var.split(",")[0], float(kv["drop"]), seed,
                 step_inputs=kv.get("stats") == "1" and kv.get("gate") == "1")
    elif op == "gate_sigma_mul":
        th = eval(var.split("theta=")[1].split("),")[0] + ")")
        ph = eval(var.split("phi=")[1].split("),")[0] + ")")
        ss = eval(var.split("ss=")[1])
        _gate_case(dev, dtype, N, th[:3], ph, th[3], C, ss, seed)
    elif op == "softmax_heads":
        _softmax_case(dev, dtype, N, D, H, W, C, eval(var.split("=")[1]), seed)
    elif op == "focal_loss":
        nc = int(var.split("=")[1])
        _focal_case(dev, dtype, N, D, H, W, C // nc, nc, seed)
    elif op == "kl_mvn_diag":
        _kl_case(dev, dtype, N, D, H, W, C, int(var.split("=")[1]), seed)
    elif op == "latent_sample":
        assert var == "rng,stacked", var
        _latent_rng_case(dev, dtype, N, D, H, W, C, seed)
    elif op == "cast":
        x = _randn((N,), _gen(dev, seed), dev, 3.0)
        assert torch.equal(ops.cast(x, torch.bfloat16), x.to(torch.bfloat16))            # round to nearest even, bit for bit
    else:
        raise KeyError(op)


def _inbwd_case(dev, dtype, dims, c, cout, seed, expect_fused, k=(1, 1, 1), kernels=None):
    """y = conv(lrelu(IN(x))), by default 1x1x1 (the pointwise conv3 of an SE block reading the norm2 output; ``k``: another stride-1
    kernel, e.g. conv2 reading norm1 -- test_convs_at_scale.py runs the bench step's own layers): the IN backward from the sums the
    conv's data-gradient epilogue emits (ops._INBWD, one partial row per epilogue tile -- thousands at res0) and from the stand-alone
    reduction, both against fp64.  The reference stores the data gradient of the norm's output in the activation type, as the conv
    does; the weights are given in that type (the conv reads them so).  The activation gradient d(a) the conv hands to the norm is
    compared per element as well (util.assert_conv_close); ``kernels``: the kernel-log entries the fused data gradient must show."""
    g = _gen(dev, seed)
    shape = (*dims, c)
    K = c * k[0] * k[1] * k[2]
    x = _as(_randn(shape, g, dev, 1.7) + 0.8 + _ramp(shape, dev) + 0.2 * _randn((1, 1, 1, 1, c), g, dev), dtype)
    gam, bet = 1 + 0.2 * _randn((c,), g, dev), 0.3 + 0.2 * _randn((c,), g, dev)
    w = _as(_randn((*k, c, cout), g, dev, 1.0 / K ** 0.5), dtype)
    bc = 0.1 * _randn((cout,), g, dev)
    xr, gr, br = (t.double().requires_grad_(True) for t in (x, gam, bet))
    a_ = util.round_grad(util.ref_instnorm_act(xr, gr, br, 0.1), dtype)
    pw = tuple(k) == (1, 1, 1)
    yr = util.ref_pointwise_conv(a_, w.double(), bc.double()) if pw else util.ref_conv3d_same(a_, w.double(), bc.double(), (1, 1, 1))
    dy = _as(yr.detach().float() + 0.5 * _randn(tuple(yr.shape), g, dev), dtype)   # dy ~ y: da ~ a (W W^T) -- dgamma stays biased
    yr.backward(dy.double())
    with torch.no_grad():
        st = util.ref_in_stats(x.double())
        xhat = (x.double() - st[:, None, None, None, :, 0]) * st[:, None, None, None, :, 1]
        z = xhat * gam.double() + bet.double()
        if pw:
            da64 = torch.einsum("ndhwo,co->ndhwc", dy.double(), w.double().reshape(c, cout))
            mda = torch.einsum("ndhwo,co->ndhwc", dy.double().abs(), w.double().abs().reshape(c, cout))
    if not pw:
        # (the input of the conv rounded to the storage type, as the kernel reads it: da does not depend on it, the shapes do)
        rf, mg_ = util.ref_conv_with_mag(torch.zeros_like(x), w, None, (1, 1, 1), dy)
        da64, mda = rf["dx"], mg_["dx"]
        del rf, mg_
    with torch.no_grad():
        da = da64.to(dtype).double()
        dz = da * torch.where(z >= 0, 1.0, 0.1)
        mg, mb = (dz * xhat).abs().sum(dim=(0, 1, 2, 3)), dz.abs().sum(dim=(0, 1, 2, 3))
        # the LeakyReLU's branch at z within fp32 error of 0 is a tie (both branches right): left out of dx.  The conv stores the
        # data gradient da in the activation type; where its fp32 value lands next to a rounding boundary the two sides may differ by
        # an ulp (2^-7 relative): |rstd * gamma * dz| joins the magnitude of dx
        tie = z.abs() <= 1e-5 * z.square().mean().sqrt()
        mdx = xr.grad.abs() + (dz * st[:, None, None, None, :, 1] * gam.double()).abs() if dtype == torch.bfloat16 else None

    def run(on):
        was = ops._INBWD["on"]; ops._INBWD["on"] = on
        try:
            xd = x.to(dtype).clone().requires_grad_(True)                 # (a fresh leaf per run: x.to(fp32) would be x itself)
            ps = [t.clone().requires_grad_(True) for t in (gam, bet, w, bc)]
            a = ops.instnorm_act(xd, ps[0], ps[1], 0.1, ops.instnorm_stats(xd))
            y = ops.conv3d_same([a], ps[2], ps[3], k, (1, 1, 1))
            seen = []
            a.register_hook(lambda g_: seen.append(g_.detach().clone()))
            with ops.kernel_log() as kl:
                y.backward(dy.to(dtype))
                torch.cuda.synchronize()
            assert len(seen) == 1
            assert_conv_close(seen[0], da64, mda, dtype, f"d(a) of the conv, fused={on} {(*dims, c)}->{cout} k={k}")
            if on and kernels is not None:
                assert [n for n in kl.names if not n.startswith("wgrad")] == list(kernels), (kl.names, kernels)
            return xd.grad, ps[0].grad, ps[1].grad
        finally:
            ops._INBWD["on"] = was
    f0 = dict(ops._INBWD)
    got = run(True)
    fused = ops._INBWD["fused"] - f0["fused"], ops._INBWD["plain"] - f0["plain"]
    assert sum(fused) == 1, fused
    if expect_fused:
        assert fused == (1, 0), fused                                   # the epilogue did emit the sums
    base = run(False)
    a, b = _ab(dtype)
    for tag, (dx, dgm, dbt) in (("fused", got), ("plain", base)):
        what = f"IN bwd ({tag}) {shape}->{cout} {dtype}"
        assert_close_ew(torch.where(tie, 0.0, dx.double()), torch.where(tie, 0.0, xr.grad), a, b,
                        mag=None if mdx is None else torch.where(tie, 0.0, mdx), what=what + " dx")
        _assert_sum(dgm, gr.grad, mg, what + " dgamma")
        _assert_sum(dbt, br.grad, mb, what + " dbeta")


@pytest.mark.gpu
@pytest.mark.parametrize("rows_small", [0, 1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("dims,c,cout", [((2, 2, 16, 16), 32, 32), ((2, 2, 16, 16), 8, 32), ((5, 2, 12, 16), 32, 32)])
def test_instnorm_backward_epilogue_sums_stats_rows_small(dev, rows_small, dtype, dims, c, cout):
    """M1_STATS_ROWS_SMALL 0 / 1 with the fused IN backward (conv epilogue partial rows, then the finalize kernel).  The switch sets the
    row capacity of the statistics workspace (m1_stats_rows_cap: one row per 64 voxels, or per 16 on small volumes); its effect is
    observed through m1_conv3d_dgrad_inbwd_rows, which sizes the epilogue's partial rows from that capacity (m1_stats_ws_floats itself
    is not exported).  The whole forward + backward runs inside one setting; N = 5 leaves a partial group of 4 samples."""
    lib = PKG.hip.lib.load()
    probe = torch.empty((*dims, c), device=dev)
    rows = {}
    for v in (0, 1):
        with ops.config(M1_STATS_ROWS_SMALL=v):
            rows[v] = int(lib.m1_conv3d_dgrad_inbwd_rows(ctypes.byref(ops._desc([probe], cout, (1, 1, 1), (1, 1, 1)))))
    V = dims[1] * dims[2] * dims[3]
    assert rows[0] == max(-(-V // 64), red_nchunks(V, c, dims[0])) and rows[1] > rows[0], rows
    with ops.config(M1_STATS_ROWS_SMALL=rows_small):
        assert ops.config_get("M1_STATS_ROWS_SMALL") == rows_small
        _inbwd_case(dev, dtype, dims, c, cout, seed=c + rows_small, expect_fused=c >= 24)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("c,cout", [(32, 32), (8, 32)])
def test_instnorm_backward_epilogue_sums_at_res0(dev, dtype, c, cout):
    """The dgrad-epilogue IN sums at res0 full size (2, 20, 160, 160): ~4,000 partial rows per sample, folded by the wide finalize
    kernel (reduce.h) -- against fp64, next to the stand-alone reduction."""
    dims = (2, 20, 160, 160)
    probe = torch.empty((*dims, c), device=dev)
    rows = int(PKG.hip.lib.load().m1_conv3d_dgrad_inbwd_rows(ctypes.byref(ops._desc([probe], cout, (1, 1, 1), (1, 1, 1)))))
    assert rows >= 4000, rows
    _inbwd_case(dev, dtype, dims, c, cout, seed=c, expect_fused=c >= 24 or dtype == torch.bfloat16)
    torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("key", C3_KEYS + EXTRA_KEYS, ids=lambda k: "-".join(str(v) for v in k))
def test_bench_shapes_against_fp64(dev, key):
    _run_key(dev, key, seed=zlib.crc32(repr(key).encode()) % 10007)
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_c3_bench_keys_are_in_the_table(dev, monkeypatch):
    seen, npar = record_c3_bench_keys(dev, monkeypatch)
    assert npar == 67_254_246
    missing = sorted(seen - set(C3_KEYS), key=str)
    assert not missing, f"calls of the C3 bench step not in C3_KEYS: {missing}"


@pytest.mark.gpu
def test_adam_amsgrad_c3_parameter_count_against_fp64(dev):
    """The flat buffer of the C3 model (67,254,246 floats: n % 4 != 0) with kernel / bias boundaries inside a float4 (nk, nk + nb not
    multiples of 4), three steps against the fp64 recurrence: the moments element-wise at the fp32 tolerance, p as p0 + (update)."""
    n, nk, nb = 67_254_246, 33_626_946 + 1, 1_206
    assert n % 4 and nk % 4 and (nk + nb) % 4
    g_ = _gen(dev, 5)
    npad = (n + 3) // 4 * 4
    p0 = torch.zeros(npad, device=dev); p0[:n] = _randn((n,), g_, dev)
    gr = torch.zeros(npad, device=dev); gr[:n] = _randn((n,), g_, dev) * 0.01
    pd, m, v, vh = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0), torch.zeros_like(p0)
    lr, b1, b2, eps, lk, lb, gs = 1e-2, 0.9, 0.999, 1e-7, 0.3, 0.7, 0.5
    lr_dev = torch.tensor([lr], device=dev); step = torch.ones(1, dtype=torch.int32, device=dev)
    p, mm, vv, hh = p0[:n].double(), torch.zeros(n, dtype=torch.float64, device=dev), None, None
    vv, hh = torch.zeros_like(mm), torch.zeros_like(mm)
    mag = 4e-4 * p0[:n].double().abs()                  # (x 5e-4: three roundings of the fp32 weight, 3 * 2^-24 |p0| < 2e-7 |p0|)
    for t in range(1, 4):
        ops.adam_amsgrad_(pd, gr, m, v, vh, nk, nb, lk, lb, gs, lr_dev, b1, b2, eps, step)
        ops.step_advance(step, None)
        pn, mm, vv, hh = util.ref_adam_amsgrad_step(p, gr[:n].double(), mm, vv, hh, t, nk, nb, lk, lb, gs, lr, b1, b2, eps)
        mag += (pn - p).abs()
        p = pn
    assert int(step) == 4
    assert_close_ew(m[:n], mm, A_32, B_32, what="adam m")
    # p - p0 is the sum of three steps that may cancel.  Each step's size lr * sqrt(1 - b2^t) / (1 - b1^t) is evaluated in fp32 (as
    # Keras does): 1 - b2^t cancels, one ulp of powf(b2, t) is 2^-24 b2^t / (1 - b2^t) = 3e-5 relative at t = 2, a few ulps of powf
    # and the fp32 constants give ~2e-4: bounded by 5e-4 of the sum of |step| (plus the weight's own rounding, in mag)
    du, dr = pd[:n].double() - p0[:n].double(), p - p0[:n].double()
    assert_close_ew(du, dr, 5e-4, 1e-5, mag=mag, what="adam p - p0")
    # (1 - b2 in fp32 is 1e-3 * (1 - 1.29e-5): every v and vhat carries that factor, a = 3e-5; b: the weights' own step-size error
    # (5e-4 of a step, below) enters the gradient through 2 lambda p, which matters where the fp32 gradient cancels)
    assert_close_ew(vh[:n], hh, 3e-5, 1e-6, what="adam vhat")
