"""Shared helpers for the parity tests (HIP path vs. the CPU oracle)."""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PKG = importlib.import_module("prostatemr_3d-cad-cspca_amd")
ops = PKG.hip.ops

C1_STRIDES = ((1, 1, 1), (1, 2, 2), (1, 2, 2), (2, 2, 2), (2, 2, 2))
C1_FILTERS = (8, 16, 32, 64, 128)


def rel_err(a: torch.Tensor, b: torch.Tensor) -> float:
    """max|a-b| / (max|b| + tiny), both brought to fp64 on the CPU."""
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def rnd(shape, seed, scale=1.0, dtype=torch.float32):
    g = np.random.default_rng(seed)
    return torch.from_numpy(g.standard_normal(shape) * scale).to(dtype)


def load_params_into(model, P):
    """Copy an oracle parameter dict (App. E names) into the product model."""
    sd = model.state_dict()
    with torch.no_grad():
        for k, v in sd.items():
            name = k.replace("m1_model.", "")
            v.copy_(P[name].to(v.device, v.dtype))


def build_m1(cfg, device, dtype=torch.float32, **extra):
    """Product model with the same constructor arguments as an oracle M1Config."""
    init = PKG.initializers
    m = PKG.unets.networks.M1(
        input_spatial_dims=cfg.input_spatial_dims, input_channels=cfg.input_channels, num_classes=cfg.num_classes,
        dropout_rate=cfg.dropout_rate, dropout_mode=cfg.dropout_mode, filters=cfg.filters, strides=cfg.strides,
        kernel_sizes=cfg.kernel_sizes, se_reduction=cfg.se_reduction, att_sub_samp=cfg.att_sub_samp,
        kernel_regularizer=init.l2(cfg.l2_kernel), bias_regularizer=init.l2(cfg.l2_bias),
        dense_skip=cfg.dense_skip, deep_supervision=cfg.deep_supervision, probabilistic=cfg.probabilistic,
        prob_latent_dims=cfg.prob_latent_dims, summary=False, **extra)
    m = m.to(device)
    m.set_compute_dtype(dtype)
    return m


class FlatGradView:
    """What test_hip_model._check_grads reads (``.named_parameters()`` / ``.grad``) over the optimiser's FLAT gradient buffer:
    every parameter of ``model`` paired with its slice of ``flatp`` (optim.FlatParams, after ``gather_grads()``)."""

    def __init__(self, model, flatp):
        self.model = model
        self.byid = {id(p): gv for p, gv in zip(flatp.params, flatp.gviews)}

    def named_parameters(self):
        for n, p in self.model.named_parameters():
            q = torch.nn.Parameter(p.detach(), requires_grad=False)
            q.grad = self.byid[id(p)].reshape(p.shape).clone()
            yield n, q


class activation_pattern:
    """``with activation_pattern(model) as ap: model(x)`` records, through forward hooks only, which branch every LeakyReLU
    of the HIP path took: ``ap.masks[tag][k]`` = boolean CPU tensor of the k-th pass through the core that owns the layer,
    tags as in oracle.m1_oracle.lrelu (``{core}.{layer}.norm1|norm2|out``, ``{core}.norme0``, ``{core}.att{i}.f``).  Fed to
    ``O.forced_activation_pattern`` the oracle evaluates the gradient of the same piecewise-linear branch."""

    def __init__(self, model):
        self.model, self.masks, self.handles, self.passes = model, {}, [], {}
        self.drop = {}          # keep-masks of the dropout draws: drop[oracle layer name][pass] (see oracle_drop_masks)

    def _tag(self, name):
        for a, b in (("m1_model.", ""), ("m1_stage1.", "stage1."), ("m1_stage2.", "stage2.")):
            if name.startswith(a):
                return b + name[len(a):]
        return name

    def __enter__(self):
        NB, NW = PKG.unets.network_blocks, PKG.unets.networks
        cores = {}

        stacked = set()          # cores whose two reference passes run stacked along the batch axis (M1Net.stack_passes)
        for name, mod in self.model.named_modules():
            if isinstance(mod, NW.M1Net) and mod.probabilistic and mod.stack_passes and not mod.show_summary:
                stacked |= {self._tag(name + ".prior"), self._tag(name + ".posterior")}
        batch, dupped = {}, {}

        shared = (".norme0", ".serse1.norm1", ".serse1.norm2")      # layers in front of the first dropout draw (M1Core.forward dup_first)

        def add(tag, m, store=None):
            store = self.masks if store is None else store
            core = next(c for c in sorted(cores, key=len, reverse=True) if tag.startswith(c + "."))
            m = m.cpu()
            if core in stacked and self.passes[core] == 0:
                # one stacked pass = the oracle's passes 0 and 1: [0:B] / [B:2B]; a tensor of the tail slice belongs to pass 1;
                # a layer the two passes SHARE (dup_first: run once on B samples) has the same pattern in both
                B2 = batch[core]
                if m.shape[0] == B2:
                    store.setdefault(tag, {})[0] = m[:B2 // 2]
                    store[tag][1] = m[B2 // 2:]
                elif dupped.get(core) and any(tag == core + sfx for sfx in shared):
                    store.setdefault(tag, {})[0] = m
                    store[tag][1] = m
                else:
                    store.setdefault(tag, {})[1] = m
                return
            k = self.passes[core] + (1 if core in stacked else 0)      # (a later separate pass, e.g. the inference sample, is pass 2)
            store.setdefault(tag, {})[k] = m
        drop_name = {id(mod): self._tag(name) for name, mod in self.model.named_modules() if isinstance(mod, NB._DropoutBase)}
        for name, mod in self.model.named_modules():
            tag = self._tag(name)
            if isinstance(mod, NW.M1Core):
                cores[tag] = mod
                self.passes[tag] = -1
                def pre(m_, i_, kw_, tag=tag):
                    self.passes[tag] += 1
                    t0 = i_[0][0] if isinstance(i_[0], (list, tuple)) else i_[0]
                    dupped[tag] = bool(kw_.get("dup_first"))
                    batch[tag] = int(t0.shape[0]) * (2 if dupped[tag] else 1)
                self.handles.append(mod.register_forward_pre_hook(pre, with_kwargs=True))
            elif isinstance(mod, NB.InstanceNormalization):
                def h(mod, inp, out, tag=tag):
                    if len(inp) > 1 and float(inp[1]) == 0.1:           # (x, slope, stats): LeakyReLU(0.1) follows
                        add(tag, out.detach() >= 0)
                self.handles.append(mod.register_forward_hook(h))
            elif isinstance(mod, NB.SEResNetBottleNeck):
                def hse(mod, args, kwargs, out, tag=tag):
                    add(tag + ".out", out.detach() >= 0)
                    dr = kwargs.get("dropout")
                    rate = dr.effective_rate() if dr is not None else 0.0
                    if rate > 0.0:
                        # the keep decision is a pure function of (seed, step, layer id, element index): the stand-alone dropout
                        # kernel on a tensor of ones reproduces the draw the fused kernel made, independently of its output
                        keep = ops.dropout(torch.ones_like(out), rate, dr.rng, dr.layer_id) != 0
                        add(drop_name[id(dr)], keep, self.drop)
                self.handles.append(mod.register_forward_hook(hse, with_kwargs=True))
            elif isinstance(mod, NB.GridAttentionBlock3D):
                st = {}
                self.handles.append(mod.theta.register_forward_hook(lambda m_, i_, o_, st=st: st.__setitem__("theta", o_.detach())))
                self.handles.append(mod.phi.register_forward_hook(lambda m_, i_, o_, st=st: st.__setitem__("phi", o_.detach())))

                def hg(mod, inp, out, tag=tag, st=st):
                    th, ph = st["theta"].float(), st["phi"].float()
                    for ax in range(3):
                        ph = ph.repeat_interleave(th.shape[1 + ax] // ph.shape[1 + ax], dim=1 + ax)
                    add(tag + ".f", (th + ph) >= 0)                     # the same fp32 add the gate kernel makes
                self.handles.append(mod.register_forward_hook(hg))
        return self

    def __exit__(self, *exc):
        for h in self.handles:
            h.remove()
        return False

    def oracle_drop_masks(self, dtype=torch.float64):
        """``drop_masks`` argument of the oracle: the keep-masks of this run, per layer and pass; layers / passes the product
        pruned (no output reads them) keep everything."""
        dm = {tag: {k: m.to(dtype) for k, m in per.items()} for tag, per in self.drop.items()}
        dm["__keep_all_where_missing__"] = True
        return dm


# ---------------------------------------------------------------------------------------------------------------------------------
# fp64 references of the non-conv ops, device-agnostic (they run where their inputs live: on the GPU at the bench step's own sizes,
# where the CPU oracle would take minutes), written with plain tensor algebra only -- the 1x1x1 SE-gate and psi convolutions are
# einsum / matmul, not conv3d.  Backward passes come from autograd.  tests/test_ops_at_scale.py pins each one to oracle/m1_oracle.py.
# ---------------------------------------------------------------------------------------------------------------------------------
IN_EPS64 = 1e-3
LRELU64 = 0.1


def ref_in_stats(x: torch.Tensor) -> torch.Tensor:
    """(N, C, 2) {mean, rstd} of an NDHWC tensor over D, H, W (biased variance, eps 1e-3), fp64."""
    x = x.double()
    mu = x.mean(dim=(1, 2, 3))
    var = ((x - mu[:, None, None, None]) ** 2).mean(dim=(1, 2, 3))
    return torch.stack([mu, torch.rsqrt(var + IN_EPS64)], dim=-1)


def ref_instnorm(x, gamma, beta):
    mu = x.mean(dim=(1, 2, 3), keepdim=True)
    var = ((x - mu) ** 2).mean(dim=(1, 2, 3), keepdim=True)
    return (x - mu) * torch.rsqrt(var + IN_EPS64) * gamma + beta


def ref_lrelu(x, slope=LRELU64):
    return torch.where(x >= 0, x, slope * x)


def ref_instnorm_act(x, gamma, beta, slope):
    return ref_lrelu(ref_instnorm(x, gamma, beta), slope)


def ref_se_gate(x_, W6, b6, W7, b7):
    """sigmoid(W7 . lrelu(W6 . GAP(x_) + b6) + b7) per sample: (N, 1, 1, 1, F); W6 (1,1,1,F,Fr), W7 (1,1,1,Fr,F)."""
    gp = x_.mean(dim=(1, 2, 3))
    h = ref_lrelu(gp @ W6.reshape(W6.shape[-2], W6.shape[-1]) + b6)
    return torch.sigmoid(h @ W7.reshape(W7.shape[-2], W7.shape[-1]) + b7)[:, None, None, None, :]


def ref_se_combine(y3, y4, g3, b3, g4, b4, W6, b6, W7, b7, rate=0.0, keep=None, dup=False, inter=None):
    """dropout(lrelu(IN3(y3) * gate * R)), R = IN4(y4) (member residual) or y4 itself (identity residual: g4 = b4 = None).
    ``dup``: two output samples per input sample, n and n + N, each behind its own slice of ``keep`` (shape of the output).
    ``inter`` (a dict): receives the intermediate tensors x_ (IN3 output), rho, gate and prod (= x_ * gate * rho), their gradients
    retained (the terms of the parameter gradients' sums)."""
    x_ = ref_instnorm(y3, g3, b3)
    rho = y4 if g4 is None else ref_instnorm(y4, g4, b4)
    gate = ref_se_gate(x_, W6, b6, W7, b7)
    prod = x_ * gate * rho
    if inter is not None:
        for k, t in (("x_", x_), ("rho", rho), ("gate", gate), ("prod", prod)):
            if t.requires_grad:
                t.retain_grad()
            inter[k] = t
    out = ref_lrelu(prod)
    if dup:
        out = torch.cat([out, out], dim=0)
    if rate > 0.0:
        out = out * keep.to(out.dtype) / (1.0 - rate)
    return out


def ref_upsample(x, size):
    for ax, r in enumerate(size):
        if int(r) != 1:
            x = x.repeat_interleave(int(r), dim=1 + ax)
    return x


def ref_gate_sigma(theta, phi, wpsi, bpsi):
    """sigmoid(psi(lrelu(theta + up(phi)))): (N, Dt, Ht, Wt); psi as a contraction over the channels."""
    up = [t // p for t, p in zip(theta.shape[1:4], phi.shape[1:4])]
    f = ref_lrelu(theta + ref_upsample(phi, up))
    return torch.sigmoid(torch.einsum("ndhwc,c->ndhw", f, wpsi.reshape(-1)) + bpsi.reshape(()))


def ref_gate_sigma_mul(theta, phi, wpsi, bpsi, x, ss, sigma_dtype=None):
    """(y, sigma), y = up(sigma, ss) * x.  ``sigma_dtype``: the product reads sigma as stored in that type (the value rounded, the
    gradient passed straight through), as the kernels do."""
    if sigma_dtype is None or sigma_dtype == torch.float64:
        sg = ref_gate_sigma(theta, phi, wpsi, bpsi)
    else:
        # the backward kernels read the STORED sigma and d(sigma): d(psi) = round(d sigma) * s_r * (1 - s_r), s_r = round(sigma)
        up = [t // p for t, p in zip(theta.shape[1:4], phi.shape[1:4])]
        psi = torch.einsum("ndhwc,c->ndhw", ref_lrelu(theta + ref_upsample(phi, up)), wpsi.reshape(-1)) + bpsi.reshape(())
        s_r = torch.sigmoid(psi.detach()).to(sigma_dtype).double()
        sg = _RoundGrad.apply(s_r + (psi - psi.detach()) * s_r * (1 - s_r), sigma_dtype)
    return ref_upsample(sg.unsqueeze(-1), ss) * x, sg


def ref_pointwise_conv(x, w, b):
    """1x1x1 convolution NDHWC (Cin) -> (Cout) as a contraction; w (1, 1, 1, Cin, Cout)."""
    return torch.einsum("ndhwc,co->ndhwo", x, w.reshape(w.shape[-2], w.shape[-1])) + b


def round_grad(x, dtype):
    """Identity whose backward rounds the gradient to ``dtype``: a data gradient a kernel stores in that type."""
    return x if dtype in (None, torch.float64, torch.float32) else _RoundGrad.apply(x, dtype)


class _RoundGrad(torch.autograd.Function):
    """Identity whose backward rounds the incoming gradient to ``dtype`` (a gradient the kernels store in that type)."""
    @staticmethod
    def forward(ctx, x, dtype):
        ctx.dtype = dtype
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.dtype).to(g.dtype), None


def ref_softmax_heads(logits, ups):
    return torch.cat([torch.softmax(ref_upsample(t, u), dim=-1) for t, u in zip(logits, ups)], dim=-1)


def ref_focal_terms(y_true, y_pred, alpha, gamma):
    """Per (voxel, head) focal terms (N, D, H, W, nheads) of losses.py Focal.FL: the loss is their sum over voxels, mean over samples
    and heads."""
    nc = y_true.shape[-1]
    nh = y_pred.shape[-1] // nc
    p = y_pred.reshape(*y_pred.shape[:-1], nh, nc)
    p = torch.clamp(p / p.sum(dim=-1, keepdim=True), 1e-7, 1 - 1e-7)
    y = y_true.unsqueeze(-2).to(p.dtype)
    cw = torch.tensor(alpha, dtype=p.dtype, device=p.device)
    return (cw * ((y * torch.pow(1.0 - p, gamma)) * (y * -torch.log(p)))).sum(dim=-1)


def ref_focal(y_true, y_pred, alpha, gamma):
    t = ref_focal_terms(y_true, y_pred, alpha, gamma)
    return t.sum(dim=(1, 2, 3)).mean()


def ref_latent_sample(ml, eps):
    L_ = ml.shape[-1] // 2
    return ml[..., :L_] + torch.exp(torch.clamp(ml[..., L_:], -0.1, 0.1)) * eps


def ref_kl_terms(mq, mp, first=None):
    """Per-voxel KL(q || p) of the first ``first`` samples (N', D, H, W); log-sigma clipped to +-0.1."""
    n = mq.shape[0] if first is None else int(first)
    mq, mp = mq[:n], mp[:n]
    L_ = mq.shape[-1] // 2
    lq, lp = torch.clamp(mq[..., L_:], -0.1, 0.1), torch.clamp(mp[..., L_:], -0.1, 0.1)
    t = torch.exp(2 * (lq - lp)) + ((mq[..., :L_] - mp[..., :L_]) / torch.exp(lp)) ** 2 - 1.0 + 2.0 * (lp - lq)
    return 0.5 * t.sum(dim=-1)


def ref_kl(mq, mp, first=None):
    return ref_kl_terms(mq, mp, first).sum(dim=(1, 2, 3)).mean().reshape(1)


def ref_adam_amsgrad_step(p, g, m, v, vhat, t, n_kernel, n_bias, l2k, l2b, grad_scale, lr, b1, b2, eps):
    """One Keras Adam(amsgrad) step with the L2 gradient 2*lambda*w on the [kernels | biases | rest] ranges; returns (p, m, v, vhat)."""
    lam = torch.zeros_like(p)
    lam[:n_kernel] = l2k
    lam[n_kernel:n_kernel + n_bias] = l2b
    gr = grad_scale * g + 2.0 * lam * p
    m = b1 * m + (1 - b1) * gr
    v = b2 * v + (1 - b2) * gr * gr
    vhat = torch.maximum(vhat, v)
    lr_t = lr * (1 - b2 ** t) ** 0.5 / (1 - b1 ** t)
    return p - lr_t * m / (vhat.sqrt() + eps), m, v, vhat


def assert_close_ew(got: torch.Tensor, ref: torch.Tensor, a: float, b: float, mag=None, what: str = ""):
    """Per element |got - ref| <= a*mag + b*rms(ref), mag = |ref| unless given (e.g. the sum of |terms| behind each element);
    evaluated where the tensors live.  Reports the worst element (by excess over its bound) and its index."""
    got = got.detach(); ref = ref.detach()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    r = ref.double()
    d = (got.double() - r).abs()
    rms = float(r.square().mean().sqrt()) if r.numel() else 0.0
    bound = a * (r.abs() if mag is None else mag.double()) + b * rms
    excess = d - bound
    k = int(torch.argmax(excess))
    if not (float(excess.reshape(-1)[k]) <= 0.0 and bool(torch.isfinite(got).all())):
        idx = tuple(int(i) for i in np.unravel_index(k, tuple(got.shape)))
        nbad = int((excess > 0).sum()) + int((~torch.isfinite(got)).sum())
        raise AssertionError(f"{what}: {nbad} of {got.numel()} elements outside |d| <= {a:.3g}*|ref| + {b:.3g}*rms; worst at {idx}: "
                             f"got {float(got.reshape(-1)[k]):.9g} ref {float(r.reshape(-1)[k]):.9g} bound {float(bound.reshape(-1)[k]):.3g} "
                             f"(rms(ref) {rms:.3g})")


# ---------------------------------------------------------------------------------------------------------------------------------
# fp64 references of the convolutions, device-agnostic and readable: a loop over the kernel's taps, each tap a shifted (and strided)
# slice of the input times a (Cin, Cout) matrix.  No library convolution.  Gradients come from autograd.  Called with |x|, |w|, |b|
# (and |dy| as the upstream gradient) the same code yields the sum of |terms| behind every output, data-gradient and weight-gradient
# element (ref_conv_with_mag).  tests/test_convs_at_scale.py pins both to oracle/m1_oracle.py.
# ---------------------------------------------------------------------------------------------------------------------------------
def same_pads(n: int, k: int, s: int):
    """(out, before, after) of TensorFlow's SAME padding: total = max((ceil(n/s) - 1)*s + k - n, 0), the smaller half in front."""
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return out, total // 2, total - total // 2


def ref_conv3d_same(x, w, b, s):
    """Conv3D(padding='same') on NDHWC in fp64; w (kd, kh, kw, Cin, Cout), b (Cout,) or None, s = (sd, sh, sw)."""
    x, w = x.double(), w.double()
    kd, kh, kw, cin, cout = w.shape
    assert x.shape[-1] == cin, (tuple(x.shape), tuple(w.shape))
    (od, db, da), (oh, hb, ha), (ow, wb, wa) = (same_pads(int(n), int(k), int(st)) for n, k, st in zip(x.shape[1:4], (kd, kh, kw), s))
    xp = torch.nn.functional.pad(x, (0, 0, wb, wa, hb, ha, db, da))
    y = None
    for a in range(kd):
        for b_ in range(kh):
            for c in range(kw):
                xs = xp[:, a:a + (od - 1) * s[0] + 1:s[0], b_:b_ + (oh - 1) * s[1] + 1:s[1], c:c + (ow - 1) * s[2] + 1:s[2]]
                t = torch.matmul(xs, w[a, b_, c])
                y = t if y is None else y + t
    return y if b is None else y + b.double()


def ref_conv3d_transpose_same(x, w, b, s):
    """Conv3DTranspose(padding='same') on NDHWC in fp64; w (kd, kh, kw, Cout, Cin); out = in * s per axis:
    out[j, co] = sum over (i, tap) with j = i*s + tap - pb of x[i, :] . w[tap, co, :] + b[co], pb = max(k - s, 0) // 2."""
    x, w = x.double(), w.double()
    kd, kh, kw, cout, cin = w.shape
    assert x.shape[-1] == cin, (tuple(x.shape), tuple(w.shape))
    n = [int(v) for v in x.shape[1:4]]
    pb = [max(k - st, 0) // 2 for k, st in zip((kd, kh, kw), s)]
    full = [max((m - 1) * st + k, p + m * st) for m, st, k, p in zip(n, s, (kd, kh, kw), pb)]
    y = x.new_zeros((x.shape[0], *full, cout))
    for a in range(kd):
        for b_ in range(kh):
            for c in range(kw):
                t = torch.matmul(x, w[a, b_, c].transpose(0, 1))
                y[:, a:a + (n[0] - 1) * s[0] + 1:s[0], b_:b_ + (n[1] - 1) * s[1] + 1:s[1], c:c + (n[2] - 1) * s[2] + 1:s[2]] += t
    y = y[:, pb[0]:pb[0] + n[0] * s[0], pb[1]:pb[1] + n[1] * s[1], pb[2]:pb[2] + n[2] * s[2]]
    return y if b is None else y + b.double()


def ref_conv_with_mag(x, w, b, s, dy=None, transposed=False):
    """(ref, mag): dicts with 'y' and, when ``dy`` is given, 'dx', 'dw', 'db' (None without a bias).  ``ref`` is the fp64 convolution and
    its autograd gradients; ``mag`` is the same computation on |x|, |w|, |b| with |dy| upstream: the sum of |terms| behind every
    element (for y the bias is one term; every db element sums the |dy| of its channel)."""
    fn = ref_conv3d_transpose_same if transposed else ref_conv3d_same
    out = []
    for f in ((lambda t: t), torch.abs):
        ins = [f(x.detach().double()).requires_grad_(dy is not None), f(w.detach().double()).requires_grad_(dy is not None),
               None if b is None else f(b.detach().double()).requires_grad_(dy is not None)]
        y = fn(ins[0], ins[1], ins[2], s)
        r = {"y": y.detach()}
        if dy is not None:
            y.backward(f(dy.detach().double()))
            r.update(dx=ins[0].grad, dw=ins[1].grad, db=None if b is None else ins[2].grad)
        del y
        out.append(r)
    return out[0], out[1]


def ref_member_amag(xs, w, b, s, transposed=False):
    """Magnitudes of the values a forward stores in its output when it runs as several launches over groups of concat members, each
    launch rounding its own contribution and the new running sum to the storage type: sum_m |C_m| + sum_{j < last} |P_j| + 2|b|, with C_m
    the contribution of member m, P_j the member-prefix sums (every running sum of launches over runs of whole members is one of them)
    and the bias counted as part of a contribution and of a running sum, whichever launch adds it."""
    fn = ref_conv3d_transpose_same if transposed else ref_conv3d_same
    amag, run, off = None, None, 0
    for j, x_ in enumerate(xs):
        c = int(x_.shape[-1])
        cm = fn(x_, w[..., off:off + c] if transposed else w[..., off:off + c, :], None, s)
        off += c
        run = cm + (0.0 if b is None else b.double()) if run is None else run + cm
        amag = cm.abs() if amag is None else amag + cm.abs()
        if j < len(xs) - 1:
            amag = amag + run.abs()
    return amag if b is None else amag + 2 * b.double().abs()


# rounding of a stored conv result (a) and fp32 accumulation of exact products, relative to the sum of |terms| (r): derived in the
# docstring of tests/test_convs_at_scale.py
CONV_A = {torch.bfloat16: 2.0 ** -8, torch.float32: 4 * 2.0 ** -24}
CONV_R = 1e-5


def assert_conv_close(got, ref, mag, dtype, what, acc=False, r=CONV_R, amag=None):
    """Per element |got - ref| <= a*|ref| + r*mag, no element left out.  ``dtype``: the type the result is STORED in (fp32 for weight
    and bias gradients); ``acc``: the kernel added into a slot of that type that already held a value (two roundings); ``mag``: the
    sum of |terms| behind each element (ref_conv_with_mag, plus |slot| where the kernel accumulates).  ``amag``: the magnitudes of further
    values that were stored in ``dtype`` on the way (the running sum a multi-launch forward keeps in its output): a*(|ref| + amag)."""
    got, ref, mag = got.detach(), ref.detach().double(), mag.detach().double()
    assert got.shape == ref.shape == mag.shape, (what, tuple(got.shape), tuple(ref.shape), tuple(mag.shape))
    a = CONV_A[dtype] * (2 if acc else 1)
    bound = a * (ref.abs() if amag is None else ref.abs() + amag.detach().double()) + r * mag
    excess = (got.double() - ref).abs() - bound
    k = int(torch.argmax(torch.nan_to_num(excess, nan=float("inf"))))
    if not (float(excess.reshape(-1)[k]) <= 0.0 and bool(torch.isfinite(got).all())):
        idx = tuple(int(i) for i in np.unravel_index(k, tuple(got.shape)))
        nbad = int((excess > 0).sum()) + int((~torch.isfinite(got)).sum())
        raise AssertionError(f"{what}: {nbad} of {got.numel()} elements outside |d| <= {a:.3g}*|ref| + {r:.3g}*sum|terms|; worst at {idx}: "
                             f"got {float(got.reshape(-1)[k]):.9g} ref {float(ref.reshape(-1)[k]):.9g} "
                             f"sum|terms| {float(mag.reshape(-1)[k]):.6g} bound {float(bound.reshape(-1)[k]):.3g}")
