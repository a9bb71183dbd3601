"""fp64 restatement of ONE guarded optimiser step (optim.Adam with clipvalue / global_clipnorm / skip_nonfinite; csrc/optim.hip), in
plain tensor algebra, device-agnostic (it runs where its inputs live).

The order is tf.keras': the optimiser receives the gradient with the regulariser's part in it (gr = grad_scale*g + 2*lambda*w, lambda
by range as in util.ref_adam_amsgrad_step), ``clipvalue`` clamps every element first (tf.clip_by_value: NaN stays NaN, an Inf is
clamped), ``global_clipnorm`` then scales ALL elements by clip / norm when the L2 norm over all of them exceeds clip
(tf.clip_by_global_norm: a non-finite norm makes every gradient NaN), and Adam(amsgrad) follows.  ``skip_nonfinite`` is this
project's own: a step whose squared norm is not finite changes nothing, Adam's t included.

What is pinned: with no clamp and coef == 1 the step equals util.ref_adam_amsgrad_step EXACTLY (test_grad_clip.py).  What is not:
parity with TensorFlow itself -- TensorFlow is not installed where these tests run; the formulas above are its documented ones."""
import math

import torch


def regularised_grad(p, g, n_kernel, n_bias, l2k, l2b, grad_scale):
    lam = torch.zeros_like(p)
    lam[:n_kernel] = l2k
    lam[n_kernel:n_kernel + n_bias] = l2b
    return grad_scale * g + 2.0 * lam * p


def clamp_value(gr, clipvalue):
    """tf.clip_by_value(gr, -c, c) = min(max(gr, -c), c); 0 / None = off."""
    if not clipvalue:
        return gr
    c = float(clipvalue)
    return torch.where(gr < -c, torch.full_like(gr, -c), torch.where(gr > c, torch.full_like(gr, c), gr))


def control(gr, global_clipnorm=0.0, skip_nonfinite=False):
    """(norm, coef, apply) of the clamped gradient ``gr``: python floats / bool."""
    s = float((gr * gr).sum())
    finite = math.isfinite(s)
    norm = math.sqrt(s) if s == s else float("nan")
    if not finite and skip_nonfinite:
        return norm, 1.0, False
    coef = 1.0
    if global_clipnorm:
        if not finite:
            coef = float("nan")
        elif norm > float(global_clipnorm):
            coef = float(global_clipnorm) / norm
    return norm, coef, True


def guarded_step(p, g, m, v, vhat, t, n_kernel, n_bias, l2k, l2b, grad_scale, lr, b1, b2, eps, clipvalue=0.0, global_clipnorm=0.0,
                 skip_nonfinite=False):
    """One step on fp64 tensors.  Returns (p, m, v, vhat, t, info) with info = {norm, coef, apply}; a skipped step returns its inputs."""
    gr = clamp_value(regularised_grad(p, g, n_kernel, n_bias, l2k, l2b, grad_scale), clipvalue)
    norm, coef, apply = control(gr, global_clipnorm, skip_nonfinite)
    info = {"norm": norm, "coef": coef, "apply": apply}
    if not apply:
        return p, m, v, vhat, t, info
    if coef != 1.0:
        gr = gr * coef
    m = b1 * m + (1 - b1) * gr
    v = b2 * v + (1 - b2) * gr * gr
    vhat = torch.maximum(vhat, v)
    lr_t = lr * (1 - b2 ** t) ** 0.5 / (1 - b1 ** t)
    return p - lr_t * m / (vhat.sqrt() + eps), m, v, vhat, t + 1, info
