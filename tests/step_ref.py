"""Host restatement of ONE training step of the compiled model (a helper, not a test module).  It composes yardsticks the suite
already has and adds none:

    gradients   oracle.m1_oracle.train_loss in fp64 and fp32 (test_hip_model._oracle_loss_and_grads on the GPU side, ``oracle_pair``
                below for an oracle-only trajectory: the fp64 evaluation's own LeakyReLU pattern forced on the fp32 evaluation, as
                test_train_step_fuzz._oracle_alone does)
    update      util.ref_adam_amsgrad_step (clip_ref.guarded_step for the guarded optimiser) on a flat vector laid out
                [regularised kernels | regularised biases | everything else] like optim.FlatParams, so that the L2 coefficient goes by
                range; the learning rate is optim.CosineDecayRestarts(iteration) rounded to float32 as ``lr_dev`` holds it; ``t`` is
                Adam's own step counter
    draws       philox_ref.normal(seed, step, core.latent_stream_id + level, n) for the latent draws of a stacked pass (the first half
                of the batch draws, the second half is the mean pass: test_random_streams.test_stacked_latent_draws_cover_the_first_
                half_only), philox_ref.keep_mask(seed, step, layer id, n, rate) for the dropout decisions

The flat gradient the product's step leaves holds the DATA term only (the compiled loss has no L2 part: the Adam kernel adds
2*lambda*w itself, optim.Adam.handles_l2); the oracle's gradient holds both.  ``split_l2`` moves between the two.

``check_state`` holds the bounds of one update, each taken from test_ops_at_scale.test_adam_amsgrad_c3_parameter_count_against_fp64
and applied PER STEP: m (and v, vhat) element-wise, p as p_t + (step)."""
import collections
import contextlib

import numpy as np
import torch

import clip_ref
import philox_ref as R
import util
from oracle import m1_oracle as O

A_32, B_32 = 1e-5, 4e-6                     # test_ops_at_scale.py: m
A_VHAT, B_VHAT = 3e-5, 1e-6                 # test_adam_amsgrad_c3_parameter_count_against_fp64: v and vhat carry fp32(1 - beta_2)
A_STEP, B_STEP = 5e-4, 1e-5                 # the same test: p - p0 against the sum of |step| ...
W_ROUND = 4e-4 / 3.0                        # ... plus 4e-4 |p0| in ``mag`` for THREE roundings of the fp32 weight: one third per step
# optim.Adam's defaults (tf.keras'), beta_1 / beta_2 as the fp32 numbers the C ABI carries, as in test_grad_clip.py: the kernel forms
# 1 - fl(0.9) = 0.1 * (1 + 2.4e-7), and where m is the small difference of 0.9 m and 0.1 g (a gradient that changed sign between two
# batches; single gradient elements reach 700 x rms(m) on these models) that factor alone put a plain numpy fp32 evaluation of the
# recurrence at 2.4 x the bound of m at step 2 of the oracle-only trajectory (0.73 x with the fp32 betas), and the kernel with it.
# A property of the argument type, not of the kernel under test.
BETA_1, BETA_2, EPSILON = float(np.float32(0.9)), float(np.float32(0.999)), 1e-7

Layout = collections.namedtuple("Layout", "names shapes n_kernel n_bias n")


def _regularised(name):
    """'kernel' / 'bias' / None: the L2 class of an oracle parameter name (oracle.m1_oracle.l2_regularisation)."""
    if ".conv6." in name or ".conv7." in name:
        return None
    return "kernel" if name.endswith(".kernel") else "bias" if name.endswith(".bias") else None


def layout_from_oracle(P):
    """[kernels | biases | rest] over an oracle parameter dict, in the dict's order inside each range."""
    ks = [k for k in P if _regularised(k) == "kernel"]
    bs = [k for k in P if _regularised(k) == "bias"]
    rest = [k for k in P if _regularised(k) is None]
    names = ks + bs + rest
    return Layout(names, [tuple(P[k].shape) for k in names], sum(P[k].numel() for k in ks), sum(P[k].numel() for k in bs),
                  sum(P[k].numel() for k in names))


def layout_from_flatp(model, flatp, strip=("m1_model.",)):
    """The layout of the product's flat buffers, under the oracle's parameter names."""
    byid = {}
    for n, p in model.named_parameters():
        for pre in strip:
            n = n.replace(pre, "")
        byid[id(p)] = n
    names = [byid[id(p)] for p in flatp.params]
    assert len(set(names)) == len(names)
    return Layout(names, [tuple(p.shape) for p in flatp.params], int(flatp.n_kernel), int(flatp.n_bias), int(flatp.n))


def flatten(lay, d, dtype=torch.float64):
    return torch.cat([(torch.zeros(s, dtype=dtype) if d[k] is None else d[k].detach().cpu().to(dtype)).reshape(-1)
                      for k, s in zip(lay.names, lay.shapes)])


def unflatten(lay, flat, dtype=None):
    out, off = {}, 0
    flat = flat.detach().cpu()
    for k, s in zip(lay.names, lay.shapes):
        n = int(np.prod(s)) if len(s) else 1
        t = flat[off:off + n].reshape(s).clone()
        out[k] = t if dtype is None else t.to(dtype)
        off += n
    assert off == lay.n
    return out


def l2_vector(lay, cfg, dtype=torch.float64):
    lam = torch.zeros(lay.n, dtype=dtype)
    lam[:lay.n_kernel] = cfg.l2_kernel
    lam[lay.n_kernel:lay.n_kernel + lay.n_bias] = cfg.l2_bias
    return lam


def split_l2(lay, cfg, p_flat, g_flat, sign):
    """``sign`` = -1: the oracle's gradient without its L2 part (what the backward pass leaves in the flat buffer); +1: a flat data
    gradient with the L2 part the Adam kernel adds (what the oracle differentiates)."""
    return g_flat.double() + sign * 2.0 * l2_vector(lay, cfg) * p_flat.double()


def lr_of(schedule, iteration):
    """The learning rate of the step that starts with ``iterations == iteration``, as float32 holds it (optim.Adam.set_lr_device)."""
    v = schedule(iteration) if callable(schedule) else schedule
    return float(np.float32(v))


# ---- draws ------------------------------------------------------------------------------------------------------------------------
def latent_draws(cfg, B, seed, step, stream_id0):
    """eps_q of the oracle: one (B, D, H, W, L) fp64 tensor per level with a latent; level ``lvl`` of the core whose
    ``latent_stream_id`` is ``stream_id0`` reads stream ``stream_id0 + lvl``, element i = index into the first B samples."""
    out, lvl_of = [], [lvl for lvl, Ld in enumerate(cfg.prob_latent_dims) if Ld != 0]
    for lvl, shp in zip(lvl_of, O.latent_shapes(cfg)):
        n = B * int(np.prod(shp))
        out.append(torch.from_numpy(R.normal(seed, step, stream_id0 + lvl, n)).reshape(B, *shp))
    return out


def keep_decisions(seed, step, layer_id, shape, rate):
    """The keep mask of a dropout layer's output of ``shape`` (element i = index into the output, test_random_streams.py)."""
    n = int(np.prod(shape))
    return torch.from_numpy(R.keep_mask(seed, step, layer_id, n, rate)).reshape(tuple(shape))


def level_dims(cfg, level):
    d = list(cfg.input_spatial_dims)
    for s_ in cfg.strides[:level + 1]:
        d = [-(-a // b) for a, b in zip(d, s_)]
    return tuple(d)


def det_dropout_layers(cfg):
    """(oracle name, level, rate) of the eight dropout layers of a deterministic core, in construction order (p / 2 behind sersd0)."""
    p = cfg.dropout_rate
    return [(f"core.drope{l}", l, p) for l in (1, 2, 3, 4)] + [(f"core.dropd{l}", l, p / 2 if l == 0 else p) for l in (3, 2, 1, 0)]


def det_drop_masks(cfg, B, seed, step, first_id=1):
    """drop_masks of the oracle for a deterministic model whose dropout layers own the ids first_id, first_id + 1, ..."""
    if not cfg.dropout_rate:
        return None
    return {name: {0: keep_decisions(seed, step, first_id + i, (B, *level_dims(cfg, lvl), cfg.filters[lvl]), rate).double()}
            for i, (name, lvl, rate) in enumerate(det_dropout_layers(cfg))}


# ---- gradients ----------------------------------------------------------------------------------------------------------------------
def _eval(cfg, P, x, tgt, eps, dm, dt, masks=None, record=False):
    Pd = {k: v.detach().to(dt, copy=True).requires_grad_(True) for k, v in P.items()}
    dmd = None if dm is None else {k: {q: m.to(dt) for q, m in v.items()} for k, v in dm.items()}
    with (O.recorded_activation_pattern() if record else contextlib.nullcontext()) as rec, \
            (O.forced_activation_pattern(masks) if masks is not None else contextlib.nullcontext()):
        loss, parts, _ = O.train_loss(Pd, cfg, x.to(dt), tgt.to(dt), eps_q=[e.to(dt) for e in eps] if eps else None, drop_masks=dmd)
    loss.backward()
    g = {k: (v.grad.double() if v.grad is not None else None) for k, v in Pd.items()}
    return float(loss.detach()), {k: float(v.detach()) for k, v in parts.items()}, g, (rec.masks if record else None)


def oracle_pair(cfg, P, x, tgt, eps=None, drop_masks=None):
    """Oracle alone: (loss, parts, g64, g32) -- fp64 on its own activation pattern, fp32 forced onto that pattern."""
    loss, parts, g64, masks = _eval(cfg, P, x, tgt, eps, drop_masks, torch.float64, record=True)
    _, _, g32, _ = _eval(cfg, P, x, tgt, eps, drop_masks, torch.float32, masks=masks)
    return loss, parts, g64, g32


class GradDictView:
    """A gradient dict behind the interface test_hip_model._check_grads reads."""

    def __init__(self, P, grads):
        self.P, self.grads = P, grads

    def named_parameters(self):
        for k, v in self.P.items():
            q = torch.nn.Parameter(v.detach().double(), requires_grad=False)
            q.grad = None if self.grads[k] is None else self.grads[k].detach().double().clone()
            yield k, q


# ---- update -------------------------------------------------------------------------------------------------------------------------
def new_state(lay, P):
    """The optimiser state in front of the first step: fp64 {p, m, v, vhat}, t = 1 (optim.Adam.bind: step_dev starts at 1)."""
    p = flatten(lay, P)
    return {"p": p, "m": torch.zeros_like(p), "v": torch.zeros_like(p), "vhat": torch.zeros_like(p), "t": 1}


def adam_update(lay, cfg, S, g_data, lr, t=None, l2=True, guard=None, grad_scale=1.0):
    """S_{t+1} from (S_t, the flat DATA gradient): util.ref_adam_amsgrad_step with the L2 ranges of the layout.  ``t`` / ``l2``
    override the step number and drop the L2 term (the sensitivity cases); ``guard`` = dict(clipvalue, global_clipnorm,
    skip_nonfinite) routes through clip_ref.guarded_step, and the returned state then carries ``info``."""
    t_ = S["t"] if t is None else t
    lk, lb = (cfg.l2_kernel, cfg.l2_bias) if l2 else (0.0, 0.0)
    args = (S["p"].double(), g_data.double(), S["m"].double(), S["v"].double(), S["vhat"].double(), t_, lay.n_kernel, lay.n_bias,
            lk, lb, grad_scale, lr, BETA_1, BETA_2, EPSILON)
    if guard is None:
        p, m, v, vhat = util.ref_adam_amsgrad_step(*args)
        return {"p": p, "m": m, "v": v, "vhat": vhat, "t": S["t"] + 1}
    p, m, v, vhat, tn, info = clip_ref.guarded_step(*args, **guard)
    return {"p": p, "m": m, "v": v, "vhat": vhat, "t": S["t"] + (tn - t_), "info": info}


def _ratio(got, ref, a, b, mag=None):
    """max over the elements of |got - ref| / (a*mag + b*rms(ref)): the quantity util.assert_close_ew bounds by 1."""
    r = ref.double()
    rms = float(r.square().mean().sqrt())
    bound = a * (r.abs() if mag is None else mag.double()) + b * rms
    return float(((got.double() - r).abs() / bound.clamp_min(1e-300)).max())


def check_state(got, ref, before, what="", report=None):
    """One update: ``got`` (the state under test after the step) against ``ref`` (the restatement applied to ``before``), all flat
    CPU tensors of the layout's n elements.  Bounds: see the module docstring.  ``report`` receives the worst |error| / bound of
    each of m, v, vhat, p (1.0 = at the bound)."""
    p0 = before["p"].double()
    du, dr = got["p"].double() - p0, ref["p"].double() - p0
    mag = dr.abs() + W_ROUND * p0.abs()
    rep = {"m": _ratio(got["m"], ref["m"], A_32, B_32), "v": _ratio(got["v"], ref["v"], A_VHAT, B_VHAT),
           "vhat": _ratio(got["vhat"], ref["vhat"], A_VHAT, B_VHAT), "p": _ratio(du, dr, A_STEP, B_STEP, mag)}
    if report is not None:
        report.update(rep)
    util.assert_close_ew(got["m"], ref["m"], A_32, B_32, what=f"{what} adam m")
    util.assert_close_ew(got["v"], ref["v"], A_VHAT, B_VHAT, what=f"{what} adam v")
    util.assert_close_ew(got["vhat"], ref["vhat"], A_VHAT, B_VHAT, what=f"{what} adam vhat")
    util.assert_close_ew(du, dr, A_STEP, B_STEP, mag=mag, what=f"{what} adam p - p_t")
    assert int(got["t"]) == int(ref["t"]), (what, "step counter", int(got["t"]), int(ref["t"]))
    return rep
