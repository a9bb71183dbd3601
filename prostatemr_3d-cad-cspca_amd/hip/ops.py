"""torch.autograd.Function shims over the C ABI (include/m1hip.h): PyTorch supplies device memory, the
current HIP stream and the autograd tape; every FLOP of the M1 hot path runs in libm1hip.so.

All activations are NDHWC, contiguous, float32 or bfloat16, on a CUDA(HIP) device.  There is no CPU
path: ops raise RuntimeError on non-GPU tensors.
"""
from __future__ import annotations

import ctypes as C
import os as _os
from typing import Optional, Sequence, Tuple

import torch

from .debug import trace_reset, trace_snapshot          # noqa: F401 -- first: installs the M1_DEBUG_* patches (torch.empty, lib.check)
from . import lib as L
from .streams import (_BRANCH, _FOLD, _WGP, _p, _req, _run_deferred_wgrads, _stream, branch, exchange_streams,  # noqa: F401
                      finish_queued_for_exchange, fold_async_default, fold_drop, fold_pending, join_side_streams,
                      on_origin_stream, submit_wgrad)
from .gradslot import _GradSlot, _slot_of, _slot_target, _slot_written, batch_tail, fanout          # noqa: F401
from .panels import _PANEL_EPOCH, _conv_ws, _pair_panel_ws, _panel_ws, invalidate_panels, repack_all     # noqa: F401

IN_EPS = 1e-3


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return L.M1_F32
    if t.dtype == torch.bfloat16:
        return L.M1_BF16
    raise RuntimeError(f"unsupported activation dtype {t.dtype} (float32 / bfloat16 only)")


def _ws(N: int, V: int, Cn: int, nsums: int, device) -> torch.Tensor:
    n = L.load().m1_reduce_ws_floats(int(N), int(V), int(Cn), int(nsums))
    return torch.empty(int(n), dtype=torch.float32, device=device)


def _desc(srcs: Sequence[torch.Tensor], cout: int, k, s) -> L.m1_conv_desc_t:
    d = L.m1_conv_desc_t()
    x0 = srcs[0]
    d.N, d.D, d.H, d.W = int(x0.shape[0]), int(x0.shape[1]), int(x0.shape[2]), int(x0.shape[3])
    d.Cin = int(sum(int(t.shape[4]) for t in srcs))
    d.Cout = int(cout)
    d.kd, d.kh, d.kw = (int(v) for v in k)
    d.sd, d.sh, d.sw = (int(v) for v in s)
    d.dtype = _dt(x0)
    d.nsrc = len(srcs)
    if len(srcs) > L.M1_MAX_SRC:
        raise RuntimeError("too many concat members")
    for i, t in enumerate(srcs):
        if t.shape[:4] != x0.shape[:4] or t.dtype != x0.dtype:
            raise RuntimeError("concat members must agree in N,D,H,W and dtype")
        d.src[i].ptr = t.data_ptr()
        d.src[i].C = int(t.shape[4])
    return d


def _nvc(x: torch.Tensor, k: int = 1) -> Tuple[int, int, int]:
    """(N, V, C) of an NDHWC tensor whose last axis holds ``k`` groups of C channels (k = 2: the {mu, logsigma} of a latent head)."""
    N, Cn = int(x.shape[0]), int(x.shape[-1]) // k
    return N, x.numel() // (N * k * Cn), Cn


def _sink(param: torch.Tensor):
    """(buffer, accumulate, autograd_return) for a parameter gradient.  A parameter bound to an optimiser's flat
    gradient buffer (optim.FlatParams sets ``_m1_gsink``) gets its gradient ACCUMULATED there by the kernel and
    autograd receives None (no per-parameter tensors, no AccumulateGrad adds, no gather pass)."""
    g = getattr(param, "_m1_gsink", None)
    if g is not None:
        param._m1_live = True            # (a backward kernel writes this parameter's gradient: optim.FlatParams.live_ranges)
        return g, 1, None
    t = torch.empty_like(param, dtype=torch.float32)
    return t, 0, t


def _sinks(*params):
    """(buffers, accumulate, autograd_returns) for the parameter gradients one backward kernel writes with ONE accumulate flag: all
    of them live in the flat buffer or none does (_sink); otherwise every parameter falls back to an fp32 temporary that autograd
    receives (vectors -- a conv bias, psi's bias -- 1-D).  ``None`` parameters (a conv without bias) get (None, None)."""
    bound = {getattr(p, "_m1_gsink", None) is not None for p in params if p is not None}
    if len(bound) == 1:
        out = [(None, 0, None) if p is None else _sink(p) for p in params]
        return [o[0] for o in out], int(True in bound), [o[2] for o in out]
    tmp = [None if p is None else torch.empty(p.shape if p.dim() > 1 else (p.numel(),), dtype=torch.float32, device=p.device)
           for p in params]
    return tmp, 0, list(tmp)


def same_out(size: int, s: int) -> int:
    return -(-size // s)


# ---------------------------------------------------------------------------------------------------------
# Conv3D / Conv3DTranspose (padding='same') over a virtual channel concat
# ---------------------------------------------------------------------------------------------------------
# InstanceNorm-backward sums from the epilogue of the data gradient that produces d(a) (m1_conv3d_dgrad_inbwd): "fused" counts the
# data gradients that emitted them, "plain" those whose kernel has no such epilogue (the norm then runs its own reduction)
_INBWD = {"on": _os.environ.get("M1_INBWD_FUSE", "1") != "0", "fused": 0, "plain": 0}


def _dgrad_targets(ctx, srcs, first: int):
    """(dsrc, ptrs, accs) of a conv's data gradient: per concat member the gradient tensor (its slot's buffer or a fresh one; None
    when input ``first + i`` needs no gradient), its address and its accumulate flag."""
    dsrc = []
    ptrs = (C.c_void_p * len(srcs))()
    accs = (C.c_int * len(srcs))()
    for i, t in enumerate(srcs):
        g = None
        if ctx.needs_input_grad[first + i]:
            g, accs[i] = _slot_target(ctx.gslots[i], t)
        dsrc.append(g)
        ptrs[i] = _p(g)
    return dsrc, ptrs, accs


def _dgrad_written(ctx, dsrc) -> None:
    """After the launch that wrote ``dsrc``: see _slot_written."""
    for slot, g in zip(ctx.gslots, dsrc):
        if g is not None:
            _slot_written(slot)


class _Conv3d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w, b, k, s, transposed, want_stats, *srcs):
        _req(w, b, *srcs)
        lib = L.load()
        x0 = srcs[0]
        cout = int(w.shape[3] if transposed else w.shape[4])
        cin = int(w.shape[4] if transposed else w.shape[3])
        d = _desc(srcs, cout, k, s)
        if d.Cin != cin or tuple(w.shape[:3]) != tuple(k):
            raise RuntimeError(f"kernel {tuple(w.shape)} does not match inputs (Cin={d.Cin}, k={k})")
        if transposed:
            osz = (d.N, d.D * d.sd, d.H * d.sh, d.W * d.sw, cout)
        else:
            osz = (d.N, same_out(d.D, d.sd), same_out(d.H, d.sh), same_out(d.W, d.sw), cout)
        y = torch.empty(osz, dtype=x0.dtype, device=x0.device)
        ws, packed = _panel_ws(w, d, transposed, 0)
        stats = None
        if transposed:
            L.check(lib.m1_convT3d_fwd(C.byref(d), _p(w), _p(b), _p(y), _p(ws), packed, _stream()), "m1_convT3d_fwd")
        else:
            if want_stats:
                stats = torch.empty((d.N, cout, 2), dtype=torch.float32, device=x0.device)
            L.check(lib.m1_conv3d_fwd(C.byref(d), _p(w), _p(b), _p(y), _p(stats), _p(ws), packed, _stream()), "m1_conv3d_fwd")
        ctx.save_for_backward(w, *srcs)
        ctx.w_param, ctx.b_param = w, b
        ctx.gslots = [_slot_of(t) for t in srcs]
        ctx.k, ctx.s, ctx.transposed, ctx.has_bias, ctx.cout = tuple(k), tuple(s), transposed, b is not None, cout
        # the input is a = lrelu(IN(x)) with this conv as its only reader (conv2 / conv3 of an SE block): the data gradient can
        # emit the InstanceNorm-backward sums from its own epilogue (instnorm_act tags its output, see _InstNormAct.backward)
        ctx.in_src = None
        for t in srcs:                    # every conv reading a tagged tensor counts (two readers: the norm keeps its own reduction)
            tk = getattr(t, "_m1_in_src", None)
            if tk is not None:
                tk.readers += 1
        tok = getattr(srcs[0], "_m1_in_src", None)
        if _INBWD["on"] and len(srcs) == 1 and not transposed and ctx.gslots[0] is None and tok is not None and tok.src is not None:
            ctx.in_src = tok
        if want_stats:
            ctx.mark_non_differentiable(stats)
            ctx.set_materialize_grads(False)      # no zero-filled "gradient" for the statistics output
            return y, stats
        return y

    @staticmethod
    def backward(ctx, dy, *_unused):
        lib = L.load()
        w, *srcs = ctx.saved_tensors
        if dy is None:
            return (None,) * (6 + len(srcs))
        dy = dy.contiguous()
        _req(dy)
        d = _desc(srcs, ctx.cout, ctx.k, ctx.s)
        st = _stream()
        name = "convT3d" if ctx.transposed else "conv3d"
        dw = db = None
        if ctx.needs_input_grad[0] or (ctx.has_bias and ctx.needs_input_grad[1]):
            dw, db = _wgrad_into_sinks(lib, d, dy, ctx.w_param, ctx.b_param if ctx.has_bias else None, ctx.transposed, st, srcs)
        dsrc, ptrs, accs = _dgrad_targets(ctx, srcs, 6)
        any_d = any(g is not None for g in dsrc)
        if any_d and ctx.in_src is not None and accs[0] == 0:
            tok = ctx.in_src
            xs, stats, gamma, beta, slope = tok.src
            da = dsrc[0]
            N, _, Cn = _nvc(xs)
            # partial rows: the library states how many the kernel may write (its epilogue tiles or the split-K finish chunks)
            nmax = int(lib.m1_conv3d_dgrad_inbwd_rows(C.byref(d)))
            part = torch.empty(N * nmax * Cn * 2 + N * Cn * 2 + 64, dtype=torch.float32, device=da.device)
            nparts = C.c_int(0)
            ws, packed = _panel_ws(ctx.w_param, d, False, 1, (True,))
            L.check(lib.m1_conv3d_dgrad_inbwd(C.byref(d), _p(w), _p(dy), _p(da), _p(xs), _p(stats), _p(gamma), _p(beta), float(slope),
                                              _p(part), nmax, C.byref(nparts), _p(ws), packed, st), "m1_conv3d_dgrad_inbwd")
            if nparts.value > 0:
                # hand-over to the norm's backward: valid for exactly this gradient tensor in exactly this state (an in-place
                # accumulation of a second consumer's gradient bumps the version, a summed copy has another address)
                tok.partials = (part, int(nparts.value), da.data_ptr(), da._version, tuple(da.shape))
                _INBWD["fused"] += 1
            else:
                _INBWD["plain"] += 1
        elif any_d:
            fn = lib.m1_convT3d_dgrad if ctx.transposed else lib.m1_conv3d_dgrad
            ws, packed = _panel_ws(ctx.w_param, d, ctx.transposed, 1, tuple(bool(g is not None) for g in dsrc))
            L.check(fn(C.byref(d), _p(w), _p(dy), ptrs, accs, _p(ws), packed, st), f"m1_{name}_dgrad")
            _dgrad_written(ctx, dsrc)
        return (dw, db, None, None, None, None, *dsrc)


def _wgrad_into_sinks(lib, d, dy, w_param, b_param, transposed: bool, st, srcs=()):
    """Weight (+ bias) gradient of a conv into the parameters' sinks (or fresh tensors): returns (dw, db) for autograd.  Where and
    when the kernel runs is streams.submit_wgrad's business."""
    (wbuf, bbuf), acc_w, (dw, db) = _sinks(w_param, b_param)
    fn = lib.m1_convT3d_wgrad if transposed else lib.m1_conv3d_wgrad
    ws = _conv_ws(d, transposed, 2, w_param.device)
    submit_wgrad(fn, d, dy, wbuf, bbuf, ws, acc_w, transposed, srcs, st, flat=dw is None and db is None)
    return dw, db


class _ConvPair(torch.autograd.Function):
    """conv1 || conv4 of an SE block as one launch (m1_conv3d_pair_fwd / _dgrad).  Its backward produces conv1's weight gradient
    and the fused data gradient; conv4's weight gradient hangs on a _WgradTap of y4 so that it starts as soon as dy4 exists."""

    @staticmethod
    def forward(ctx, w1, b1, w4, b4, k, s, *srcs):
        _req(w1, b1, w4, b4, *srcs)
        lib = L.load()
        x0 = srcs[0]
        c1, c4 = int(w1.shape[4]), int(w4.shape[4])
        d = _desc(srcs, c1 + c4, k, s)
        osz = (d.N, same_out(d.D, d.sd), same_out(d.H, d.sh), same_out(d.W, d.sw))
        y1 = torch.empty((*osz, c1), dtype=x0.dtype, device=x0.device)
        y4 = torch.empty((*osz, c4), dtype=x0.dtype, device=x0.device)
        s1 = torch.empty((d.N, c1, 2), dtype=torch.float32, device=x0.device)
        s4 = torch.empty((d.N, c4, 2), dtype=torch.float32, device=x0.device)
        ws, packed = _pair_panel_ws(w1, w4, d, 0)
        L.check(lib.m1_conv3d_pair_fwd(C.byref(d), _p(w1), _p(b1), _p(w4), _p(b4), c1, _p(y1), _p(y4), _p(s1), _p(s4), _p(ws), packed,
                                       _stream()), "m1_conv3d_pair_fwd")
        ctx.save_for_backward(w1, w4, *srcs)
        ctx.w1_param, ctx.b1_param, ctx.w4_param = w1, b1, w4
        ctx.gslots = [_slot_of(t) for t in srcs]
        ctx.k, ctx.s, ctx.c1, ctx.c4 = tuple(k), tuple(s), c1, c4
        ctx.mark_non_differentiable(s1, s4)
        ctx.set_materialize_grads(False)
        return y1, s1, y4, s4

    @staticmethod
    def backward(ctx, dy1, _s1, dy4, _s4):
        lib = L.load()
        w1, w4, *srcs = ctx.saved_tensors
        n_in = 6 + len(srcs)
        if dy1 is None and dy4 is None:
            return (None,) * n_in
        osz = (srcs[0].shape[0], *[same_out(int(v), st_) for v, st_ in zip(srcs[0].shape[1:4], ctx.s)])
        if dy1 is None:
            dy1 = torch.zeros((*osz, ctx.c1), dtype=srcs[0].dtype, device=srcs[0].device)
        if dy4 is None:
            dy4 = torch.zeros((*osz, ctx.c4), dtype=srcs[0].dtype, device=srcs[0].device)
        dy1, dy4 = dy1.contiguous(), dy4.contiguous()
        st = _stream()
        dw1 = db1 = None
        iw, isrc = getattr(ctx, "idx_w1", 0), getattr(ctx, "idx_src", 6)       # positions of w1 / the first member among the inputs
        if ctx.needs_input_grad[iw] or ctx.needs_input_grad[iw + 1]:
            dw1, db1 = _wgrad_into_sinks(lib, _desc(srcs, ctx.c1, ctx.k, ctx.s), dy1, ctx.w1_param, ctx.b1_param, False, st, srcs)
        d = _desc(srcs, ctx.c1 + ctx.c4, ctx.k, ctx.s)
        dsrc, ptrs, accs = _dgrad_targets(ctx, srcs, isrc)
        if any(g is not None for g in dsrc):
            ws, packed = _pair_panel_ws(ctx.w1_param, ctx.w4_param, d, 1, tuple(bool(g is not None) for g in dsrc))
            L.check(lib.m1_conv3d_pair_dgrad(C.byref(d), _p(w1), _p(w4), ctx.c1, _p(dy1), _p(dy4), ptrs, accs, _p(ws), packed, st),
                    "m1_conv3d_pair_dgrad")
            _dgrad_written(ctx, dsrc)
        return (dw1, db1, None, None, None, None, *dsrc)


class _WgradTap(torch.autograd.Function):
    """Identity on ``y`` whose backward computes the weight / bias gradient of the conv that produced it (``y`` = conv(srcs; w, b))
    and passes dy on: the gradient starts as soon as dy exists, on the stream the tap was created on (ops.branch)."""

    @staticmethod
    def forward(ctx, y, w, b, k, s, *srcs):
        ctx.save_for_backward(*srcs)
        ctx.w_param, ctx.b_param, ctx.k, ctx.s = w, b, tuple(k), tuple(s)
        return y.view_as(y)

    @staticmethod
    def backward(ctx, dy):
        srcs = ctx.saved_tensors
        if dy is None:
            return (None,) * (5 + len(srcs))
        dyc = dy.contiguous()
        dw, db = _wgrad_into_sinks(L.load(), _desc(srcs, int(ctx.w_param.shape[4]), ctx.k, ctx.s), dyc, ctx.w_param, ctx.b_param, False,
                                   _stream(), srcs)
        return (dy, dw, db, None, None, *([None] * len(srcs)))


class _PairGraft(torch.autograd.Function):
    """Joins the outputs of conv1 and conv4 (computed by two ordinary forward launches, conv4 on a side stream) into ONE autograd
    node whose backward is conv1's weight gradient + the fused data gradient over [dy1 | dy4] (m1_conv3d_pair_dgrad)."""

    @staticmethod
    def forward(ctx, y1, y4, w1, b1, w4, k, s, *srcs):
        ctx.save_for_backward(w1, w4, *srcs)
        ctx.w1_param, ctx.b1_param, ctx.w4_param = w1, b1, w4
        ctx.gslots = [_slot_of(t) for t in srcs]
        ctx.k, ctx.s, ctx.c1, ctx.c4 = tuple(k), tuple(s), int(w1.shape[4]), int(w4.shape[4])
        ctx.idx_w1, ctx.idx_src = 2, 7
        ctx.set_materialize_grads(False)
        return y1.view_as(y1), y4.view_as(y4)

    @staticmethod
    def backward(ctx, dy1, dy4):
        g = _ConvPair.backward(ctx, dy1, None, dy4, None)       # (dw1, db1, None, None, None, None, *dsrc)
        return (None, None, g[0], g[1], None, None, None, *g[6:])


_FORCE_DIRECT = [False]


def conv_pair_supported(srcs, w1, w4, s) -> bool:
    """conv1 || conv4 with one data gradient pays on the matrix-core (not halo-tile) layers: >= 32 + 128 output channels."""
    if _os.environ.get("M1_CONV_PAIR", "1") == "0" or _FORCE_DIRECT[0] or not srcs[0].is_cuda:
        return False
    seg = 8 if srcs[0].dtype == torch.bfloat16 else 4
    c1, c4 = int(w1.shape[4]), int(w4.shape[4])
    if not (c4 >= 128 and c1 % seg == 0 and all(int(t.shape[4]) % seg == 0 for t in srcs)):
        return False
    # the library's own gates for the pair's forward AND data gradient (a refusal inside the backward pass would have no fallback)
    d = _desc(srcs, c1 + c4, tuple(int(v) for v in w1.shape[:3]), s)
    return bool(L.load().m1_conv3d_pair_supported(C.byref(d), c1))


def conv_pair_same(srcs, w1, b1, w4, b4, k, s):
    """(y1, stats1, y4, stats4, branch) of Conv3D(w1) and Conv3D(w4) applied to the same virtual concat (network_blocks.py:53,64).
    Forward: ONE launch over the 32 + 128 (64 + 256) output columns on 160-column tiles (conv_mfma.hip want_bn160): conv1 rides on
    the rows conv4 gathers anyway (-1.7 % per C3 step against two launches on two streams; with 128-column tiles, the last one 75 %
    empty, it lost: 2.31 vs 1.21 + 0.97 ms on the 512-channel res2 layer).  M1_CONV_PAIR_FWD=0: two launches.  Backward: ONE
    contraction over [dy1 | dy4] for the data gradient (1.60 vs 1.32 + 0.61 ms there), conv4's weight gradient on a tap of y4 on
    the side stream.  The caller joins ``branch`` before it reads y4 / stats4."""
    dev = srcs[0].device
    if _os.environ.get("M1_CONV_PAIR_FWD", "1") == "1":
        y1, s1, y4raw, s4 = _ConvPair.apply(w1, b1, w4, b4, tuple(k), tuple(s), *srcs)
    else:
        with torch.no_grad():
            det = [t.detach() for t in srcs]
            with branch(dev, 0) as br0:
                y4n, s4 = _Conv3d.apply(w4, b4, tuple(k), tuple(s), False, True, *det)
            y1n, s1 = _Conv3d.apply(w1, b1, tuple(k), tuple(s), False, True, *det)
            br0.join()
        y1, y4raw = _PairGraft.apply(y1n, y4n, w1, b1, w4, tuple(k), tuple(s), *srcs)
    with branch(dev, 0) as br:                              # conv4's weight gradient: next to the conv3 -> conv2 backward chain
        y4 = _WgradTap.apply(y4raw, w4, b4, tuple(k), tuple(s), *[t.detach() for t in srcs])
    return y1, s1, y4, s4, br


def conv3d_same(srcs, w, b, k, s, stats: bool = False):
    """tf.keras.layers.Conv3D(padding='same') on the channel-concat of ``srcs`` (never materialised).
    ``stats=True`` also returns the (N,Cout,2) {mean, rstd} of the output (for the InstanceNorm that follows),
    accumulated in the conv's epilogue."""
    if isinstance(srcs, torch.Tensor):
        srcs = [srcs]
    return _Conv3d.apply(w, b, tuple(k), tuple(s), False, bool(stats), *srcs)


def conv3d_transpose_same(srcs, w, b, k, s):
    """tf.keras.layers.Conv3DTranspose(padding='same') on the channel-concat of ``srcs``."""
    if isinstance(srcs, torch.Tensor):
        srcs = [srcs]
    return _Conv3d.apply(w, b, tuple(k), tuple(s), True, False, *srcs)


# ---------------------------------------------------------------------------------------------------------
# InstanceNormalization (+ LeakyReLU)
# ---------------------------------------------------------------------------------------------------------
def instnorm_stats(x: torch.Tensor) -> torch.Tensor:
    _req(x)
    N, V, Cn = _nvc(x)
    stats = torch.empty((N, Cn, 2), dtype=torch.float32, device=x.device)
    ws = _ws(N, V, Cn, 2, x.device)
    L.check(L.load().m1_instnorm_stats(_p(x), N, V, Cn, _dt(x), IN_EPS, _p(stats), _p(ws), _stream()), "m1_instnorm_stats")
    return stats


class _InTok:
    """Hand-over of the fused InstanceNorm-backward sums: created by instnorm_act's forward, found by the ONE conv that reads its
    output (``_m1_in_src`` on the output tensor), filled by that conv's data gradient (``partials``), checked by the norm's backward
    against the gradient tensor it actually receives."""
    __slots__ = ("src", "partials", "readers")

    def __init__(self):
        self.src, self.partials, self.readers = None, None, 0


class _InstNormAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, slope, stats, tok=None):
        _req(x, gamma, beta)
        N, V, Cn = _nvc(x)
        if stats is None:
            stats = instnorm_stats(x)
        y = torch.empty_like(x)
        L.check(L.load().m1_instnorm_apply(_p(x), _p(stats), _p(gamma), _p(beta), float(slope), _p(y), N, V, Cn, _dt(x),
                                           _stream()), "m1_instnorm_apply")
        ctx.save_for_backward(x, stats, gamma, beta)
        ctx.g_param, ctx.b_param = gamma, beta
        ctx.slope = float(slope)
        ctx.tok = tok
        return y

    @staticmethod
    def backward(ctx, dy):
        x, stats, gamma, beta = ctx.saved_tensors
        dy = dy.contiguous()
        N, V, Cn = _nvc(x)
        dx = torch.empty_like(x)
        (gbuf, bbuf), acc, (dg, db) = _sinks(ctx.g_param, ctx.b_param)
        tok = ctx.tok
        pp = tok.partials if tok is not None else None
        if tok is not None:
            tok.partials = None
        # the data gradient that produced dy already emitted {sum dy, sum dy*xh} per tile -- accepted only for the very tensor
        # (address, shape, version) that kernel wrote, from the single reader the forward saw
        if (pp is not None and tok.readers == 1 and pp[2] == dy.data_ptr() and pp[3] == dy._version and pp[4] == tuple(dy.shape)):
            part, nparts = pp[0], pp[1]
            sums = part[part.numel() - N * Cn * 2 - 64:]
            L.check(L.load().m1_instnorm_bwd_partials(_p(x), _p(stats), _p(gamma), _p(beta), ctx.slope, _p(dy), _p(dx), _p(gbuf), _p(bbuf),
                                                      N, V, Cn, _dt(x), _p(part), nparts, _p(sums), acc, _stream()),
                    "m1_instnorm_bwd_partials")
            return dx, dg, db, None, None, None
        ws = _ws(N, V, Cn, 2, x.device)
        L.check(L.load().m1_instnorm_bwd(_p(x), _p(stats), _p(gamma), _p(beta), ctx.slope, _p(dy), _p(dx), _p(gbuf), _p(bbuf),
                                         N, V, Cn, _dt(x), _p(ws), acc, _stream()), "m1_instnorm_bwd")
        return dx, dg, db, None, None, None


def instnorm_act(x, gamma, beta, slope: float = 1.0, stats=None):
    """tfa InstanceNormalization (eps 1e-3) followed by LeakyReLU(slope) (slope=1 -> no activation).
    ``stats``: the (N,C,2) {mean, rstd} already produced by the conv that wrote ``x`` (else computed here)."""
    if _INBWD["on"] and stats is not None and torch.is_grad_enabled():
        tok = _InTok()
        y = _InstNormAct.apply(x, gamma, beta, slope, stats, tok)
        tok.src = (x, stats, gamma, beta, float(slope))
        y._m1_in_src = tok                                         # (found by the conv that consumes y, see _Conv3d.forward)
        return y
    return _InstNormAct.apply(x, gamma, beta, slope, stats)


# ---------------------------------------------------------------------------------------------------------
# SE gate + multiplicative combine (+ fused dropout)
# ---------------------------------------------------------------------------------------------------------
_SE_DEFER: list = []      # (m1_se_gate_job_t, tensors kept alive) queued by _SECombine.backward in gradient-sink mode


def flush_deferred() -> None:
    """Run the queued SE gate backwards (m1_se_gate_bwd_batch).  optim.FlatParams.gather_grads calls this before anything
    reads the flat gradient buffer; the tensors the jobs point at are held until the launch is enqueued."""
    join_side_streams()
    if not _SE_DEFER:
        return
    jobs = (L.SeGateJob * len(_SE_DEFER))(*[j for j, _ in _SE_DEFER])
    try:
        L.check(L.load().m1_se_gate_bwd_batch(jobs, len(_SE_DEFER), _stream()), "m1_se_gate_bwd_batch")
    finally:
        _SE_DEFER.clear()


def drop_deferred() -> None:
    """Forget queued jobs of a backward pass whose gradients are being discarded (optimiser zero_grad)."""
    fold_drop()
    join_side_streams()
    _SE_DEFER.clear()


class _SECombine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y3, y4, g3, b3, g4, b4, W6, b6, W7, b7, drop_rate, rng, layer_id, s3, s4, gate, dup=False):
        _req(y3, y4, g3, b3, g4, b4, W6, b6, W7, b7)
        lib = L.load()
        N, V, Fn = _nvc(y3)
        Fr = int(W6.shape[-1])
        st = _stream()
        ident = g4 is None and b4 is None            # network_blocks.py:63 false branch: y4 is the block input, no norm4
        if (g4 is None) != (b4 is None) or tuple(y4.shape) != tuple(y3.shape):
            raise RuntimeError("se_combine: gamma4 / beta4 both or neither; y4 must have y3's shape")
        s3 = instnorm_stats(y3) if s3 is None else s3
        s4 = None if ident else (instnorm_stats(y4) if s4 is None else s4)
        if gate is not None:                      # evaluated up front with the other gates of the pass (se_gate_batch)
            hidden, g = gate
            if hidden.numel() != Fr or g.numel() != Fn:
                raise RuntimeError("se_combine: precomputed gate does not match this block")
        else:
            hidden = torch.empty(Fr, dtype=torch.float32, device=y3.device)
            g = torch.empty(Fn, dtype=torch.float32, device=y3.device)
            L.check(lib.m1_se_gate_fwd(_p(b3), _p(W6), _p(b6), _p(W7), _p(b7), Fn, Fr, _p(hidden), _p(g), st), "m1_se_gate_fwd")
        dup = bool(dup)
        if dup and (ident or Fn % (8 if y3.dtype == torch.bfloat16 else 4)):
            raise RuntimeError("se_combine: the duplicating form needs a norm4 residual and whole 16-byte channel vectors")
        # dup: the two stacked passes of a core share (y3, y4); the output holds both, each behind its own dropout draw
        out = torch.empty((2 * N, *y3.shape[1:]), dtype=y3.dtype, device=y3.device) if dup else torch.empty_like(y3)
        # keep bits of the fused dropout, stored for the backward (bf16, F % 8 == 0: one byte per 16-byte vector)
        mask = None
        if drop_rate > 0.0 and y3.dtype == torch.bfloat16 and Fn % 8 == 0 and any(ctx.needs_input_grad):
            mask = torch.empty(out.numel() // 8, dtype=torch.uint8, device=y3.device)
        fwd = lib.m1_se_combine_dup_fwd if dup else lib.m1_se_combine_fwd
        L.check(fwd(_p(y3), _p(y4), _p(s3), _p(s4), _p(g3), _p(b3), _p(g4), _p(b4), _p(g), _p(out), N, V, Fn,
                    _dt(y3), float(drop_rate), _p(rng), int(layer_id), _p(mask), st), "m1_se_combine_fwd")
        ctx.ident, ctx.dup = ident, dup
        if ident:
            ctx.save_for_backward(y3, y4, s3, g3, b3, W6, W7, hidden, g)
        else:
            ctx.save_for_backward(y3, y4, s3, s4, g3, b3, g4, b4, W6, W7, hidden, g)
        ctx.params = (g3, b3, g4, b4, W6, b6, W7, b7)             # (g4 = b4 = None on the identity residual)
        ctx.mask = mask
        ctx.rng, ctx.drop_rate, ctx.layer_id = rng, float(drop_rate), int(layer_id)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = L.load()
        if ctx.ident:
            y3, y4, s3, g3, b3, W6, W7, hidden, g = ctx.saved_tensors
            s4 = g4 = b4 = None
        else:
            y3, y4, s3, s4, g3, b3, g4, b4, W6, W7, hidden, g = ctx.saved_tensors
        dout = dout.contiguous()
        N, V, Fn = _nvc(y3)
        Fr = int(W6.shape[-1])
        st = _stream()
        dev = y3.device
        dy3, dy4 = torch.empty_like(y3), torch.empty_like(y4)
        (bg3, bb3, bg4, bb4, bW6, bb6, bW7, bb7), acc, rets = _sinks(*ctx.params)
        dg = torch.empty(Fn + Fr, dtype=torch.float32, device=dev)
        ws = _ws(N, V, Fn, 5, dev)
        bwd = lib.m1_se_combine_dup_bwd if ctx.dup else lib.m1_se_combine_bwd
        L.check(bwd(_p(y3), _p(y4), _p(s3), _p(s4), _p(g3), _p(b3), _p(g4), _p(b4), _p(g), _p(dout),
                    _p(dy3), _p(dy4), _p(bg3), _p(bb3), _p(bg4), _p(bb4), _p(dg), N, V, Fn, _dt(y3),
                    ctx.drop_rate, _p(ctx.rng), ctx.layer_id, _p(ctx.mask), _p(ws), acc, st), "m1_se_combine_bwd")
        if acc == 1:
            # parameter gradients only, accumulated into the optimiser's flat buffer: nothing downstream in this backward
            # reads them, so the job is queued and all SE blocks' gate backwards run as one batch (flush_deferred)
            job = L.SeGateJob(_p(b3), _p(W6), _p(W7), _p(hidden), _p(g), _p(dg), _p(bb3), _p(bW6), _p(bb6), _p(bW7), _p(bb7),
                              Fn, Fr, 1, 0)
            _SE_DEFER.append((job, (b3, W6, W7, hidden, g, dg)))
        else:
            L.check(lib.m1_se_gate_bwd(_p(b3), _p(W6), _p(W7), _p(hidden), _p(g), _p(dg), Fn, Fr, _p(bb3), _p(bW6), _p(bb6),
                                       _p(bW7), _p(bb7), acc, st), "m1_se_gate_bwd")
        return (dy3, dy4, *rets, None, None, None, None, None, None, None)


def se_combine(y3, y4, g3, b3, g4, b4, W6, b6, W7, b7, drop_rate=0.0, rng=None, layer_id=0, stats3=None, stats4=None,
               gate=None, dup=False):
    """dropout(lrelu(IN3(y3) * sigmoid(W7.lrelu(W6.beta3+b6)+b7) * IN4(y4)))  (network_blocks.py:60-78).
    ``gate``: the (hidden, g) pair se_gate_batch computed for this block from the same parameters, else evaluated here.
    ``g4 = b4 = None``: the identity residual of network_blocks.py:63 (C_in == filters) -- ``y4`` is the block's input tensor.
    ``dup``: the output holds TWO samples per input sample (n and n + N), each behind its own dropout draw: the two stacked passes of
    a core share everything in front of their first draw (M1Core.forward ``dup_first``); the backward sums the halves' gradients."""
    return _SECombine.apply(y3, y4, g3, b3, g4, b4, W6, b6, W7, b7, drop_rate, rng, layer_id, stats3, stats4, gate, bool(dup))


def se_gate_batch(params):
    """[(hidden, g)] for a list of SE blocks' (beta3, W6, b6, W7, b7): the gates depend on parameters only (GAP of an
    InstanceNorm output is its beta), so one launch evaluates all gates of a core pass (m1_se_gate_fwd_batch)."""
    if not params:
        return []
    _req(*[t for ps in params for t in ps])
    dev = params[0][0].device
    sizes = [(int(W6.shape[-1]), int(W6.shape[-2])) for _, W6, _, _, _ in params]          # (Fr, F)
    buf = torch.empty(sum(a + b for a, b in sizes), dtype=torch.float32, device=dev)
    jobs = (L.SeGateFwdJob * len(params))()
    out, off = [], 0
    for j, ((b3, W6, b6, W7, b7), (Fr, Fn)) in enumerate(zip(params, sizes)):
        hidden, g = buf[off:off + Fr], buf[off + Fr:off + Fr + Fn]
        off += Fr + Fn
        jobs[j] = L.SeGateFwdJob(_p(b3), _p(W6), _p(b6), _p(W7), _p(b7), hidden.data_ptr(), g.data_ptr(), Fn, Fr)
        out.append((hidden, g))
    L.check(L.load().m1_se_gate_fwd_batch(jobs, len(params), _stream()), "m1_se_gate_fwd_batch")
    return out


# ---------------------------------------------------------------------------------------------------------
# attention-gate pieces
# ---------------------------------------------------------------------------------------------------------
def _gate_sigma_bwd(ctx, theta, phi, wpsi, sigma, dsigma):
    """(dtheta, dphi, dw, db) of sigma = gate_sigma(theta, phi, psi) for a contiguous ``dsigma`` (m1_gate_sigma_bwd)."""
    N, Dt, Ht, Wt, Cn = (int(v) for v in theta.shape)
    Dp, Hp, Wp = (int(v) for v in phi.shape[1:4])
    dtheta, dphi = torch.empty_like(theta), torch.empty_like(phi)
    (wbuf, bbuf), acc, (dw, db) = _sinks(ctx.w_param, ctx.b_param)
    ws = _ws(N, Dt * Ht * Wt, Cn, 2, theta.device)
    L.check(L.load().m1_gate_sigma_bwd(_p(theta), _p(phi), _p(wpsi), _p(sigma), _p(dsigma), _p(dtheta), _p(dphi), _p(wbuf),
                                       _p(bbuf), N, Dt, Ht, Wt, Dp, Hp, Wp, Cn, _dt(theta), _p(ws), acc, _stream()),
            "m1_gate_sigma_bwd")
    return dtheta, dphi, dw, db


def _mul_sigma_bwd(ctx, x, sigma, dy):
    """(dx, dsigma) of y = mul_sigma(x, sigma) for a contiguous ``dy``; dx goes to x's gradient slot (m1_mul_sigma_bwd)."""
    N, D, H, W, Cn = (int(v) for v in x.shape)
    dsig = torch.empty_like(sigma)
    dx, acc = _slot_target(ctx.gslot, x)
    L.check(L.load().m1_mul_sigma_bwd(_p(x), _p(sigma), _p(dy), _p(dx), _p(dsig), N, D, H, W, Cn, *ctx.ss, _dt(x), acc,
                                      _stream()), "m1_mul_sigma_bwd")
    _slot_written(ctx.gslot)
    return dx, dsig


class _GateSigma(torch.autograd.Function):
    @staticmethod
    def forward(ctx, theta, phi, wpsi, bpsi):
        _req(theta, phi, wpsi, bpsi)
        N, Dt, Ht, Wt, Cn = (int(v) for v in theta.shape)
        Dp, Hp, Wp = (int(v) for v in phi.shape[1:4])
        sigma = torch.empty((N, Dt, Ht, Wt), dtype=theta.dtype, device=theta.device)
        L.check(L.load().m1_gate_sigma_fwd(_p(theta), _p(phi), _p(wpsi), _p(bpsi), _p(sigma), N, Dt, Ht, Wt, Dp, Hp, Wp, Cn,
                                           _dt(theta), _stream()), "m1_gate_sigma_fwd")
        ctx.save_for_backward(theta, phi, wpsi, sigma)
        ctx.w_param, ctx.b_param = wpsi, bpsi
        return sigma

    @staticmethod
    def backward(ctx, dsigma):
        return _gate_sigma_bwd(ctx, *ctx.saved_tensors, dsigma.contiguous())


def gate_sigma(theta, phi, wpsi, bpsi):
    return _GateSigma.apply(theta, phi, wpsi, bpsi)


class _MulSigma(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, sigma, ss):
        _req(x, sigma)
        N, D, H, W, Cn = (int(v) for v in x.shape)
        y = torch.empty_like(x)
        L.check(L.load().m1_mul_sigma_fwd(_p(x), _p(sigma), _p(y), N, D, H, W, Cn, int(ss[0]), int(ss[1]), int(ss[2]), _dt(x),
                                          _stream()), "m1_mul_sigma_fwd")
        ctx.save_for_backward(x, sigma)
        ctx.ss = tuple(int(v) for v in ss)
        ctx.gslot = _slot_of(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        return (*_mul_sigma_bwd(ctx, *ctx.saved_tensors, dy.contiguous()), None)


def mul_sigma(x, sigma, ss=(1, 1, 1)):
    return _MulSigma.apply(x, sigma, tuple(ss))


class _GateSigmaMul(torch.autograd.Function):
    """sigma = gate_sigma(theta, phi, psi) and y = mul_sigma(x, sigma) as ONE forward launch (m1_gate_sigma_mul_fwd, B:113-124); the
    backward runs the two backward entry points in order (the product first: it produces d(sigma))."""

    @staticmethod
    def forward(ctx, theta, phi, wpsi, bpsi, x, ss):
        _req(theta, phi, x)
        N, Dt, Ht, Wt, Ci = (int(v) for v in theta.shape)
        Dp, Hp, Wp = (int(v) for v in phi.shape[1:4])
        _, D, H, W, Cx = (int(v) for v in x.shape)
        sigma = torch.empty((N, Dt, Ht, Wt), dtype=theta.dtype, device=theta.device)
        y = torch.empty_like(x)
        L.check(L.load().m1_gate_sigma_mul_fwd(_p(theta), _p(phi), _p(wpsi), _p(bpsi), _p(sigma), _p(x), _p(y), N, Dt, Ht, Wt, Dp, Hp, Wp,
                                               Ci, D, H, W, Cx, int(ss[0]), int(ss[1]), int(ss[2]), _dt(x), _stream()),
                "m1_gate_sigma_mul_fwd")
        ctx.save_for_backward(theta, phi, wpsi, sigma, x)
        ctx.w_param, ctx.b_param = wpsi, bpsi
        ctx.ss = tuple(int(v) for v in ss)
        ctx.gslot = _slot_of(x)
        ctx.set_materialize_grads(False)                     # (an unused output's gradient arrives as None, not as a zero tensor)
        return y, sigma

    @staticmethod
    def backward(ctx, dy, dsigma_out):
        theta, phi, wpsi, sigma, x = ctx.saved_tensors
        if dy is None:                                       # (only sigma was used downstream)
            dy = torch.zeros_like(x)
        dx, dsig = _mul_sigma_bwd(ctx, x, sigma, dy.contiguous())
        if dsigma_out is not None:                           # sigma is an output of the block too (B:130): its own gradient, if any
            dsig = dsig + dsigma_out.to(dsig.dtype)
        return (*_gate_sigma_bwd(ctx, theta, phi, wpsi, sigma, dsig), dx, None)


_GATE_FUSED = {"on": _os.environ.get("M1_GATE_FWD_FUSED", "1") != "0"}


def gate_sigma_mul(theta, phi, wpsi, bpsi, x, ss=(1, 1, 1)):
    """(y, sigma) of a grid attention gate's non-GEMM part: one launch where the shapes allow it, else gate_sigma + mul_sigma."""
    vec = 8 if theta.dtype == torch.bfloat16 else 4
    ok = (_GATE_FUSED["on"] and theta.shape[-1] % vec == 0 and x.shape[-1] % vec == 0 and
          all(int(x.shape[1 + i]) == int(theta.shape[1 + i]) * int(ss[i]) for i in range(3)))
    if ok:
        return _GateSigmaMul.apply(theta, phi, wpsi, bpsi, x, tuple(ss))
    sigma = gate_sigma(theta, phi, wpsi, bpsi)
    return mul_sigma(x, sigma, ss), sigma


# ---------------------------------------------------------------------------------------------------------
# latent sample / KL
# ---------------------------------------------------------------------------------------------------------
class _LatentSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ml, eps, mode):
        _req(ml, eps)
        if eps is not None and eps.dtype != ml.dtype:
            raise RuntimeError(f"latent_sample: eps is {eps.dtype}, the head output {ml.dtype} (the kernel reads both as one type)")
        N, V, Lc = _nvc(ml, 2)
        # the kernel reads eps for every sample (modes 0 / 1 -- mode 1 ignores the values) or for the first half of the batch only
        # (mode 2, stacked passes): a draw tensor of another size would be read out of bounds
        need = ml.numel() // 4 if int(mode) == 2 else ml.numel() // 2
        if int(mode) == 2 and N % 2:
            raise RuntimeError("latent_sample: stacked mode needs an even batch")
        if eps is not None and (int(mode) != 1) and eps.numel() != need:
            raise RuntimeError(f"latent_sample: eps holds {eps.numel()} draws, mode {int(mode)} of a {tuple(ml.shape)} head needs {need}")
        z = torch.empty((*ml.shape[:-1], Lc), dtype=ml.dtype, device=ml.device)
        L.check(L.load().m1_latent_sample_fwd(_p(ml), _p(eps), _p(z), N, V, Lc, int(mode), _dt(ml), _stream()),
                "m1_latent_sample_fwd")
        ctx.save_for_backward(ml, eps if eps is not None else ml.new_empty(0))
        ctx.mode = int(mode)
        return z

    @staticmethod
    def backward(ctx, dz):
        ml, eps = ctx.saved_tensors
        dz = dz.contiguous()
        N, V, Lc = _nvc(ml, 2)
        dml = torch.empty_like(ml)
        L.check(L.load().m1_latent_sample_bwd(_p(ml), _p(eps) if eps.numel() else None, _p(dz), _p(dml), N, V, Lc, ctx.mode,
                                              _dt(ml), _stream()), "m1_latent_sample_bwd")
        return dml, None, None


class _LatentSampleRng(torch.autograd.Function):
    """latent_sample with the draws made in the kernel from the device-resident {seed, step} state (m1_latent_sample_rng_*)."""

    @staticmethod
    def forward(ctx, ml, rng, stream_id, mode):
        _req(ml, rng)
        N, V, Lc = _nvc(ml, 2)
        if int(mode) == 2 and N % 2:
            raise RuntimeError("latent_sample: stacked mode needs an even batch")
        z = torch.empty((*ml.shape[:-1], Lc), dtype=ml.dtype, device=ml.device)
        L.check(L.load().m1_latent_sample_rng_fwd(_p(ml), _p(rng), int(stream_id), _p(z), N, V, Lc, int(mode), _dt(ml), _stream()),
                "m1_latent_sample_rng_fwd")
        ctx.save_for_backward(ml)
        ctx.rng, ctx.stream_id, ctx.mode = rng, int(stream_id), int(mode)
        return z

    @staticmethod
    def backward(ctx, dz):
        (ml,) = ctx.saved_tensors
        dz = dz.contiguous()
        N, V, Lc = _nvc(ml, 2)
        dml = torch.empty_like(ml)
        L.check(L.load().m1_latent_sample_rng_bwd(_p(ml), _p(ctx.rng), ctx.stream_id, _p(dz), _p(dml), N, V, Lc, ctx.mode, _dt(ml),
                                                  _stream()), "m1_latent_sample_rng_bwd")
        return dml, None, None, None


def latent_sample(ml, eps, mean: bool, stacked: bool = False, rng=None, stream_id: int = 0):
    """z = mu + exp(clip(logsigma,+-0.1))*eps, or mu when ``mean`` (networks.py:640-647).  ``stacked``: the batch holds the
    sampling pass and the prob_mean pass of the reference one after the other; ``eps`` covers the first half only.
    ``eps=None`` with ``rng`` (device int64[2] = {seed, step}): the draws are made inside the kernel, a pure function of
    (seed, step, stream_id, element index) that the backward regenerates."""
    if eps is None and not mean and rng is not None:
        return _LatentSampleRng.apply(ml, rng, int(stream_id), 2 if stacked else 0)
    return _LatentSample.apply(ml, eps, 2 if stacked else (1 if mean else 0))


class _KL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mq, mp, first):
        _req(mq, mp)
        Nall, V, Lc = _nvc(mq, 2)
        N = Nall if first is None else int(first)
        if not (0 < N <= Nall) or mq.shape != mp.shape:
            raise RuntimeError("kl_mvn_diag: both heads must have one shape, `first` within the batch")
        kl = torch.empty(1, dtype=torch.float32, device=mq.device)
        L.check(L.load().m1_kl_fwd(_p(mq), _p(mp), _p(kl), N, V, Lc, _dt(mq), _stream()), "m1_kl_fwd")
        ctx.save_for_backward(mq, mp)
        ctx.first = N
        return kl

    @staticmethod
    def backward(ctx, dkl):
        mq, mp = ctx.saved_tensors
        dkl = dkl.contiguous().float()
        Nall, V, Lc = _nvc(mq, 2)
        dq, dp = torch.empty_like(mq), torch.empty_like(mp)
        L.check(L.load().m1_kl_bwd_first(_p(mq), _p(mp), _p(dkl), _p(dq), _p(dp), ctx.first, V, Lc, Nall, _dt(mq), _stream()), "m1_kl_bwd")
        return dq, dp, None


def kl_mvn_diag(ml_q, ml_p, first: Optional[int] = None):
    """mean_b sum_voxels KL(q||p) of one level (networks.py:375-377) -> tensor of shape (1,).  ``first``: only the first ``first``
    samples of the two (contiguous) heads enter the term (the sampling half of two stacked passes); their gradient comes back at full
    size with zeros behind -- no slice, so no zero-fill + copy of autograd's slice backward."""
    return _KL.apply(ml_q, ml_p, first)


# ---------------------------------------------------------------------------------------------------------
# softmax heads
# ---------------------------------------------------------------------------------------------------------
class _SoftmaxHeads(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ups, *logits):
        _req(*logits)
        l0 = logits[0]
        N, D, H, W, nc = (int(v) for v in l0.shape)
        heads = (L.m1_head_t * len(logits))()
        for i, (t, u) in enumerate(zip(logits, ups)):
            heads[i].logits = t.data_ptr(); heads[i].dlogits = None
            heads[i].u0, heads[i].u1, heads[i].u2 = (int(v) for v in u)
        probs = torch.empty((N, D, H, W, nc * len(logits)), dtype=torch.float32, device=l0.device)
        L.check(L.load().m1_softmax_heads_fwd(heads, len(logits), _p(probs), N, D, H, W, nc, _dt(l0), _stream()),
                "m1_softmax_heads_fwd")
        ctx.save_for_backward(probs, *logits)
        ctx.ups = ups
        return probs

    @staticmethod
    def backward(ctx, dprobs):
        probs, *logits = ctx.saved_tensors
        dprobs = dprobs.contiguous().float()
        l0 = logits[0]
        N, D, H, W, nc = (int(v) for v in l0.shape)
        heads = (L.m1_head_t * len(logits))()
        grads = []
        for i, (t, u) in enumerate(zip(logits, ctx.ups)):
            g = torch.empty_like(t)
            grads.append(g)
            heads[i].logits = t.data_ptr(); heads[i].dlogits = g.data_ptr()
            heads[i].u0, heads[i].u1, heads[i].u2 = (int(v) for v in u)
        L.check(L.load().m1_softmax_heads_bwd(heads, len(logits), _p(probs), _p(dprobs), N, D, H, W, nc, _dt(l0), _stream()),
                "m1_softmax_heads_bwd")
        return (None, *grads)


def softmax_heads(logits: Sequence[torch.Tensor], ups: Sequence[Tuple[int, int, int]]):
    """concat_h softmax(upsample_nearest(logits_h, ups_h)) -> fp32 (N,D,H,W,nheads*nc) (networks.py:751-754)."""
    return _SoftmaxHeads.apply(tuple(tuple(int(v) for v in u) for u in ups), *logits)


# ---------------------------------------------------------------------------------------------------------
# Monte-Carlo inference: n-draw mean and entropy of the detection head (mc.hip; M1.get_detect_model().predict_mc)
# ---------------------------------------------------------------------------------------------------------
def _no_grad_only(what: str) -> None:
    if torch.is_grad_enabled():
        raise RuntimeError(f"{what} is an inference op without a backward: call it under torch.no_grad()")


def _mc_accum(what: str, logits: torch.Tensor, R: int, acc, samples, uncertainty: bool, views):
    """The one body of ``mc_accum`` / ``mc_accum_u`` / ``mc_accum_v`` / ``mc_accumulate``, which document it; ``what`` names the caller
    in the error messages.  ``acc``: the sum_p tensor, or the triple with ``uncertainty``."""
    _no_grad_only(what)
    R, ls = int(R), logits.shape
    if views is None:
        if len(ls) < 3 or R < 1 or ls[0] % R:
            raise RuntimeError(f"{what}: logits {tuple(ls)} do not hold {R} replicas of a batch")
    else:
        if len(ls) != 5 or R < 1 or ls[0] % R:
            raise RuntimeError(f"{what}: logits {tuple(ls)} are not (R*B, D, H, W, nc) with R = {R}")
        R, flips = _flips(what, views, R)
    B, nc = ls[0] // R, ls[-1]
    shape = (B, *ls[1:])
    shapes = (shape, shape[:-1], shape) if uncertainty else (shape,)
    if acc is None:
        add, sums = 0, ()
    else:
        add, sums = 1, (tuple(acc) if uncertainty else (acc,))
        if len(sums) != len(shapes):
            raise RuntimeError(f"{what}: acc must be (sum_p, sum_h, sum_pp), got {len(sums)} tensors")
        for t, s, n in zip(sums, shapes, ("sum_p", "sum_h", "sum_pp")):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.shape != s:
                raise RuntimeError(f"{what}: {n} must be fp32 {s}, got {getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    draws = samples if isinstance(samples, torch.Tensor) else None     # (the caller's own slice of an (n_draws, B, ...) tensor)
    if draws is not None and (draws.dtype != torch.float32 or draws.shape != (R, *shape)):
        raise RuntimeError(f"{what}: samples must be fp32 {(R, *shape)}, got {draws.dtype} {tuple(draws.shape)}")
    _req(logits, draws, *sums)
    if not add:
        sums = tuple([torch.empty(s, dtype=torch.float32, device=logits.device) for s in shapes])
    if draws is None and samples:
        draws = torch.empty((R, *shape), dtype=torch.float32, device=logits.device)
    lib, lp, dt, dp, st = L.load(), logits.data_ptr(), _dt(logits), _p(draws), _stream()
    sp, sh, sq = (t.data_ptr() for t in sums) if uncertainty else (sums[0].data_ptr(), None, None)
    V = logits.numel() // (R * B * nc)
    if views is not None:
        L.check(lib.m1_mc_accum_v(lp, R, *shape, dt, flips, sp, sh, sq, add, dp, st), "m1_mc_accum_v")
    elif uncertainty:
        L.check(lib.m1_mc_accum_u(lp, R, B, V, nc, dt, sp, sh, sq, add, dp, st), "m1_mc_accum_u")
    else:
        L.check(lib.m1_mc_accum(lp, R, B, V, nc, dt, sp, add, dp, st), "m1_mc_accum")
    res = sums if uncertainty else sums[0]
    return res if draws is None else (res, draws)


def _mc_finish(what: str, acc, n: int, uncertainty: bool):
    """The one body of ``mc_finish`` / ``mc_finish_u`` / ``mc_finalize``: the dict of maps, each written over its accumulator."""
    _no_grad_only(what)
    sums = tuple(acc) if uncertainty else (acc,)
    if uncertainty and len(sums) != 3:
        raise RuntimeError(f"{what}: acc must be (sum_p, sum_h, sum_pp), got {len(sums)} tensors")
    _req(*sums)
    sum_p, ps = sums[0], sums[0].shape
    if ([t for t in sums if t.dtype != torch.float32] or len(ps) < 2 or int(n) < 1
            or (uncertainty and (sums[2].shape != ps or sums[1].shape != ps[:-1]))):
        raise RuntimeError(f"{what}: acc must hold the fp32 accumulators of mc_accum{'_u' if uncertainty else ''} and n >= 1")
    B, nc = ps[0], ps[-1]
    V = sum_p.numel() // (B * nc)
    ent = torch.empty(ps[:-1], dtype=torch.float32, device=sum_p.device)
    if not uncertainty:
        L.check(L.load().m1_mc_finish(_p(sum_p), int(n), B, V, nc, _p(sum_p), _p(ent), _stream()), "m1_mc_finish")
        return {"mean": sum_p, "entropy": ent}
    _, sum_h, sum_pp = sums
    mi = torch.empty_like(ent)
    L.check(L.load().m1_mc_finish_u(_p(sum_p), _p(sum_h), _p(sum_pp), int(n), B, V, nc, _p(sum_p), _p(ent), _p(sum_h), _p(mi), _p(sum_pp),
                                    _stream()), "m1_mc_finish_u")
    return {"mean": sum_p, "entropy": ent, "expected_entropy": sum_h, "mutual_info": mi, "variance": sum_pp}


def mc_accum(logits: torch.Tensor, R: int, sum_p: Optional[torch.Tensor] = None, samples: bool = False):
    """One pass of an n-draw inference (m1_mc_accum): ``logits`` (R*B, D, H, W, nc) is the head's raw output over ``R`` replicas of
    the caller's B samples, replica-major.  ``sum_p=None`` starts an accumulator (B, D, H, W, nc) fp32 = sum_r softmax(logits_r) --
    written, not added to, so it needs no zero fill; a given ``sum_p`` is added to in place.  Returns ``sum_p``, or
    ``(sum_p, per-draw probabilities (R, B, D, H, W, nc) fp32)`` with ``samples=True`` or with ``samples`` = the fp32 tensor of that
    shape to write them into."""
    return _mc_accum("mc_accum", logits, R, sum_p, samples, False, None)


def mc_finish(sum_p: torch.Tensor, n: int):
    """(mean, entropy) of ``n`` accumulated draws (m1_mc_finish): mean = sum_p / n, written over ``sum_p``; entropy (B, D, H, W) fp32 =
    -sum_c mean_c ln(mean_c) in nats (scipy.stats.entropy's default), 0 ln 0 = 0."""
    d = _mc_finish("mc_finish", sum_p, n, False)
    return d["mean"], d["entropy"]


def mc_accum_u(logits: torch.Tensor, R: int, acc=None, samples: bool = False):
    """``mc_accum`` with the accumulators of the uncertainty maps (m1_mc_accum_u): ``acc`` = (sum_p (B, D, H, W, nc), sum_h (B, D, H, W),
    sum_pp (B, D, H, W, nc)), all fp32; sum_h (+)= sum_r H(softmax(logits_r)), sum_pp (+)= sum_r softmax(logits_r)^2.  ``acc=None`` starts
    the triple -- written, not added to, so no zero fill; a given triple is added to in place.  Returns the triple, or ``(triple,
    per-draw probabilities)`` with ``samples`` as in ``mc_accum``.  sum_p and the samples are ``mc_accum``'s, bit for bit."""
    return _mc_accum("mc_accum_u", logits, R, acc, samples, True, None)


def mc_finish_u(acc, n: int):
    """The five maps of ``n`` accumulated draws (m1_mc_finish_u) from ``acc`` = mc_accum_u's triple: {"mean" (over sum_p), "entropy",
    "expected_entropy" = sum_h / n (over sum_h), "mutual_info" = max(entropy - expected_entropy, 0), "variance" = max(sum_pp / n -
    mean^2, 0) (over sum_pp)}, nats, fp32.  mean and entropy are ``mc_finish``'s, bit for bit, unless a draw held a NaN: then every map
    of that voxel is NaN here, where ``mc_finish``'s entropy reads 0."""
    return _mc_finish("mc_finish_u", acc, n, True)


def _flips(what: str, views, R: Optional[int] = None) -> Tuple[int, int]:
    """(R, the packed masks of m1_mc_accum_v / m1_tta_views) of ``views``, a sequence of 3-bit mirror masks (bit 0: W, 1: H, 2: D)."""
    views = [int(v) for v in views]
    if not 1 <= len(views) <= 16 or (R is not None and len(views) != int(R)):
        raise RuntimeError(f"{what}: one mask per replica expected (1..16), got {len(views)} masks" + ("" if R is None else f" for R = {R}"))
    if any(v < 0 or v > 7 for v in views):
        raise RuntimeError(f"{what}: a view is a mask 0..7 (bit 0 mirrors W, bit 1 H, bit 2 D), got {views}")
    return len(views), sum(v << (3 * r) for r, v in enumerate(views))


def mc_accum_v(logits: torch.Tensor, R: int, views, acc=None, samples: bool = False, uncertainty: bool = False):
    """``mc_accum`` (``uncertainty=False``: ``acc`` and the result are its sum_p) or ``mc_accum_u`` (``uncertainty=True``: its triple)
    of a pass whose replica r was computed on the input mirrored by ``views[r]``, a mask 0..7 (bit 0: W, bit 1: H, bit 2: D): the
    logits (R*B, D, H, W, nc) are read at the mirrored coordinates, so the accumulators and the samples (R, B, D, H, W, nc) are on the
    caller's own grid (m1_mc_accum_v).  Equal, bit for bit, to the plain op on logits that were flipped back beforehand."""
    return _mc_accum("mc_accum_v", logits, R, acc, samples, uncertainty, tuple(views))


def mc_accumulate(logits: torch.Tensor, R: int, acc=None, samples: bool = False, uncertainty: bool = False, views=None):
    """The three ops above in one spelling: ``mc_accum_v`` with ``views``, else ``mc_accum_u`` with ``uncertainty``, else ``mc_accum``
    (``acc`` is then its sum_p) -- the same launch and the same bits as the op it stands for."""
    return _mc_accum("mc_accumulate", logits, R, acc, samples, uncertainty, views)


def mc_finalize(acc, n: int, uncertainty: bool = False):
    """The finish of ``mc_accumulate``'s result, always a dict: ``mc_finish_u`` of the triple with ``uncertainty``, else ``mc_finish``
    of the sum_p tensor as {"mean", "entropy"}."""
    return _mc_finish("mc_finalize", acc, n, uncertainty)


def tta_views(x: torch.Tensor, views) -> torch.Tensor:
    """(len(views)*B, D, H, W, C), replica-major: replica r is ``x`` (B, D, H, W, C) fp32 / bf16 mirrored by the mask ``views[r]``
    (m1_tta_views) -- ``x.repeat`` and the per-view flips in one launch."""
    _no_grad_only("tta_views")
    if x.dim() != 5:
        raise RuntimeError(f"tta_views: x must be (B, D, H, W, C), got {tuple(x.shape)}")
    R, flips = _flips("tta_views", views)
    _req(x)
    B, D, H, W, Cn = (int(v) for v in x.shape)
    out = torch.empty((R * B, D, H, W, Cn), dtype=x.dtype, device=x.device)
    L.check(L.load().m1_tta_views(_p(x), B, D, H, W, Cn, _dt(x), R, flips, _p(out), _stream()), "m1_tta_views")
    return out


# ---------------------------------------------------------------------------------------------------------
# Sliding-window inference: tiles of the network's size out of a larger volume and back (tile.hip; unets.networks.predict_tiled)
# ---------------------------------------------------------------------------------------------------------
def tile_struct(geom) -> L.m1_tile_t:
    """m1_tile_t from ``tiling.tile_geometry``'s dict (an m1_tile_t passes through).  The C entry points check what it holds."""
    if isinstance(geom, L.m1_tile_t):
        return geom
    g = L.m1_tile_t()
    for a in range(3):
        o = [int(v) for v in geom["origin"][a]]
        if len(o) != int(geom["n"][a]) or not 1 <= len(o) <= L.M1_TILE_MAX_AXIS:
            raise RuntimeError(f"tile geometry: axis {a} lists {len(o)} origins for n = {geom['n'][a]} (1..{L.M1_TILE_MAX_AXIS})")
        g.vol[a], g.tile[a], g.n[a] = int(geom["vol"][a]), int(geom["tile"][a]), len(o)
        for k, v in enumerate(o):
            g.origin[a][k] = v
    return g


def tile_gather(x: torch.Tensor, geom) -> torch.Tensor:
    """(T*B, d, h, w, C), tile-major (sample t * B + b is tile t of batch entry b): the tiles of ``geom`` (``tiling.tile_geometry``) cut
    out of ``x`` (B, D, H, W, C) fp32 / bf16 (m1_tile_gather) -- the slices and their ``cat`` in one launch."""
    _no_grad_only("tile_gather")
    g = tile_struct(geom)
    if x.dim() != 5 or tuple(int(v) for v in x.shape[1:4]) != tuple(g.vol):
        raise RuntimeError(f"tile_gather: x must be (B, {', '.join(str(v) for v in g.vol)}, C), got {tuple(x.shape)}")
    _req(x)
    B, Cn = int(x.shape[0]), int(x.shape[4])
    T = g.n[0] * g.n[1] * g.n[2]
    out = torch.empty((T * B, *g.tile, Cn), dtype=x.dtype, device=x.device)
    L.check(L.load().m1_tile_gather(_p(x), B, Cn, _dt(x), C.byref(g), _p(out), _stream()), "m1_tile_gather")
    return out


def tile_profile(weights, device) -> torch.Tensor:
    """The three weight rows of a blend (``tiling.tile_weights``: host arrays) as the one fp32 device tensor m1_tile_blend reads, w0,
    w1, w2 one after the other.  ValueError for an entry that is not finite and positive: the kernel divides by their sum."""
    rows = [torch.as_tensor(r, dtype=torch.float32, device="cpu").reshape(-1) for r in weights]
    if len(rows) != 3 or any(r.numel() < 1 for r in rows):
        raise ValueError(f"tile_profile: three non-empty weight rows expected, got {[r.numel() for r in rows]}")
    flat = torch.cat(rows)
    if not bool((torch.isfinite(flat) & (flat > 0)).all()):
        raise ValueError("tile_profile: every weight must be finite and > 0")
    return flat.to(device)


def tile_blend(tiles: torch.Tensor, geom, profile) -> torch.Tensor:
    """(B, D, H, W, C) fp32: the weighted mean, voxel by voxel, of the tiles that cover it (m1_tile_blend).  ``tiles`` (T*B, d, h, w,
    C) fp32 in ``tile_gather``'s order; ``profile``: the three host rows of ``tiling.tile_weights`` (checked and uploaded here), or the
    device tensor ``tile_profile`` made of them (for a call that is captured or repeated)."""
    _no_grad_only("tile_blend")
    g = tile_struct(geom)
    T = g.n[0] * g.n[1] * g.n[2]
    if tiles.dim() != 5 or tiles.dtype != torch.float32 or tiles.shape[0] % T or tuple(int(v) for v in tiles.shape[1:4]) != tuple(g.tile):
        raise RuntimeError(f"tile_blend: tiles must be fp32 ({T} * B, {', '.join(str(v) for v in g.tile)}, C), got {tiles.dtype} "
                           f"{tuple(tiles.shape)}")
    if not isinstance(profile, torch.Tensor):
        profile = tile_profile(profile, tiles.device)
    if profile.dtype != torch.float32 or profile.dim() != 1 or profile.numel() != sum(g.tile):
        raise RuntimeError(f"tile_blend: profile must be fp32 ({sum(g.tile)},) = w0, w1, w2 of the tile {tuple(g.tile)}, got "
                           f"{profile.dtype} {tuple(profile.shape)}")
    _req(tiles, profile)
    B, Cn = int(tiles.shape[0]) // T, int(tiles.shape[4])
    out = torch.empty((B, *g.vol, Cn), dtype=torch.float32, device=tiles.device)
    L.check(L.load().m1_tile_blend(_p(tiles), B, Cn, C.byref(g), _p(profile), _p(out), _stream()), "m1_tile_blend")
    return out


# ---------------------------------------------------------------------------------------------------------
# Per-case scoring of a validation batch (validate.hip; validation.validate)
# ---------------------------------------------------------------------------------------------------------
def val_score_ws(B: int, voxels: int, K: int) -> int:
    """Bytes of the workspace ``val_score`` needs for B cases of ``voxels`` voxels and K classes (host only)."""
    return int(L.load().m1_val_score_ws(int(B), int(voxels), int(K)))


def val_score(p: torch.Tensor, y: torch.Tensor, entropy: Optional[torch.Tensor] = None, alpha: Sequence[float] = (0.25, 0.75),
              gamma: float = 2.0, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One record of 40 doubles per case (m1_val_record_t, include/m1hip.h) from ``p`` (B,D,H,W,K) fp32, the one-hot ``y`` of the same
    shape (uint8 or fp32; anything else is converted to fp32) and ``entropy`` (B,D,H,W) fp32 or None -> (B, 40) fp64 on the device.
    Nothing is read back: ``read_val_records`` is the host read.  ``ws``: at least val_score_ws(B, D*H*W, K) bytes, 8-byte aligned."""
    _no_grad_only("val_score")
    if y.dtype not in (torch.float32, torch.uint8):
        y = y.to(torch.float32)
    _req(p, y, entropy, ws)
    if p.dtype != torch.float32 or p.dim() < 3 or tuple(p.shape) != tuple(y.shape):
        raise RuntimeError(f"val_score: p must be fp32 (B,...,K) and y of the same shape, got {p.dtype} {tuple(p.shape)} / {tuple(y.shape)}")
    B, K = int(p.shape[0]), int(p.shape[-1])
    V = p.numel() // max(B * K, 1)
    if entropy is not None and (entropy.dtype != torch.float32 or tuple(entropy.shape) != tuple(p.shape[:-1])):
        raise RuntimeError(f"val_score: entropy must be fp32 {tuple(p.shape[:-1])}, got {entropy.dtype} {tuple(entropy.shape)}")
    if len(alpha) != K:
        raise RuntimeError(f"val_score: {K} class weights expected, got {len(alpha)}")
    lib = L.load()
    if ws is None:
        ws = torch.empty(max(val_score_ws(B, V, K), 8), dtype=torch.uint8, device=p.device)
    rec = torch.empty((B, L.M1_VAL_SLOTS), dtype=torch.float64, device=p.device)
    al = (C.c_float * K)(*[float(a) for a in alpha])
    L.check(lib.m1_val_score(_p(p), _p(y), L.M1_VAL_Y_U8 if y.dtype == torch.uint8 else L.M1_VAL_Y_F32, _p(entropy), al, float(gamma),
                             B, V, K, _p(rec), _p(ws), ws.numel() * ws.element_size(), _stream()), "m1_val_score")
    return rec


def read_val_records(records: torch.Tensor, K: int = L.M1_VAL_MAX_K) -> list:
    """The records of ``val_score`` ((N, 40) fp64; several batches concatenated) on the host, one dict per case (synchronises): the
    header's keys as floats, ints for the counts, and each class key as a list over the first ``K`` classes."""
    w = records.detach().reshape(-1, L.M1_VAL_SLOTS).cpu().numpy()
    out = []
    for r in w:
        d = {k: float(r[i]) for i, k in enumerate(L.VAL_HEAD_KEYS)}
        d["n_voxels"], d["n_fg"] = int(d["n_voxels"]), int(d["n_fg"])
        for j, k in enumerate(L.VAL_CLASS_KEYS):
            col = [r[8 + 8 * c + j] for c in range(int(K))]
            d[k] = [int(v) for v in col] if k.startswith("n_") else [float(v) for v in col]
        out.append(d)
    return out


# ---------------------------------------------------------------------------------------------------------
# Calibration record of a validation batch (calibrate.hip; calibration.reliability)
# ---------------------------------------------------------------------------------------------------------
def cal_record_slots(K: int, bins: int) -> int:
    """Unsigned 64-bit slots of one case's calibration record, 8 + 3 * bins * (K + 2) (host only); raises when K is outside 2..4 or
    bins outside 1..64."""
    n = int(L.load().m1_cal_record_slots(int(K), int(bins)))
    if n == 0:
        raise RuntimeError(f"cal_score: K must be in {L.M1_CAL_MIN_K}..{L.M1_CAL_MAX_K} and bins in 1..{L.M1_CAL_MAX_BINS}, got K = {K}, "
                           f"bins = {bins}")
    return n


def cal_score(p: torch.Tensor, label: torch.Tensor, bins: int, mask: Optional[torch.Tensor] = None, unc: Optional[torch.Tensor] = None,
              u_max: Optional[float] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One calibration record per case (m1_cal_score, include/m1hip.h) from ``p`` (B,...,K) fp32 or bf16, ``label`` (B,...) uint8 class
    indices, ``mask`` (B,...) uint8 or None (0 skips the voxel) and ``unc`` (B,...) fp32 or None with its upper end ``u_max`` (required
    with ``unc``) -> (B, cal_record_slots(K, bins)) int64 on the device, holding the unsigned 64-bit slots.  ``out``: a contiguous
    int64 tensor of that shape to write into.  Nothing is read back: ``read_cal_records`` is the host read.  Every argument is
    checked before anything is launched (RuntimeError; a ``u_max`` that is not positive and finite: calibration.u_scale's ValueError)."""
    _no_grad_only("cal_score")
    _req(p, label, mask, unc, out)
    if p.dtype not in (torch.float32, torch.bfloat16) or p.dim() < 2:
        raise RuntimeError(f"cal_score: p must be fp32 or bf16 (B,...,K), got {p.dtype} {tuple(p.shape)}")
    B, K, M = int(p.shape[0]), int(p.shape[-1]), int(bins)
    slots = cal_record_slots(K, M)
    V = p.numel() // max(B * K, 1)
    if B < 1 or V < 1 or V >= L.M1_CAL_MAX_VOXELS:
        raise RuntimeError(f"cal_score: 1 <= voxels per case < 2^27 and B >= 1 expected, got p {tuple(p.shape)}")
    for name, t in (("label", label), ("mask", mask)):
        if t is not None and (t.dtype != torch.uint8 or tuple(t.shape) != tuple(p.shape[:-1])):
            raise RuntimeError(f"cal_score: {name} must be uint8 {tuple(p.shape[:-1])}, got {t.dtype} {tuple(t.shape)}")
    u_scale = 0.0
    if unc is not None:
        if unc.dtype != torch.float32 or tuple(unc.shape) != tuple(p.shape[:-1]):
            raise RuntimeError(f"cal_score: unc must be fp32 {tuple(p.shape[:-1])}, got {unc.dtype} {tuple(unc.shape)}")
        if u_max is None:
            raise RuntimeError("cal_score: unc needs u_max, the value at the upper end of its last bin")
        from ..calibration import u_scale as cal_u_scale                   # (the one definition; ValueError for a bad u_max)
        u_scale = float(cal_u_scale(M, u_max))
    if out is None:
        out = torch.empty((B, slots), dtype=torch.int64, device=p.device)
    elif out.dtype != torch.int64 or tuple(out.shape) != (B, slots) or out.data_ptr() % 8:
        raise RuntimeError(f"cal_score: out must be int64 {(B, slots)}, 8-byte aligned, got {out.dtype} {tuple(out.shape)}")
    L.check(L.load().m1_cal_score(_p(p), _dt(p), _p(label), _p(mask), _p(unc), u_scale, B, V, K, M, _p(out), _stream()), "m1_cal_score")
    return out


def read_cal_records(records: torch.Tensor, K: int, bins: int) -> list:
    """The records of ``cal_score`` ((N, slots); several batches concatenated) on the host, one dict per case (synchronises): "K",
    "M", the ints n_valid / n_invalid / n_ignored / nll, and uint64 arrays brier (K,), top_count / top_conf_sum / top_correct (M,),
    cls_count / cls_p_sum / cls_pos (K, M), unc_count / unc_u_sum / unc_errors (M,) -- the layout calibration.reliability_host
    returns."""
    K, M = int(K), int(bins)
    slots = cal_record_slots(K, M)
    w = records.detach().reshape(-1, slots).cpu().numpy().view("uint64")
    out = []
    for r in w:
        d = {"K": K, "M": M}
        d.update({k: int(r[i]) for i, k in enumerate(L.CAL_HEAD_KEYS)})
        d["brier"] = r[4:4 + K].copy()
        h = r[L.M1_CAL_HEAD:].reshape(K + 2, 3, M)
        for j, k in enumerate(L.CAL_HIST_KEYS["top"]):
            d["top_" + k] = h[0, j].copy()
        for j, k in enumerate(L.CAL_HIST_KEYS["cls"]):
            d["cls_" + k] = h[1:K + 1, j].copy()
        for j, k in enumerate(L.CAL_HIST_KEYS["unc"]):
            d["unc_" + k] = h[K + 1, j].copy()
        out.append(d)
    return out


# ---------------------------------------------------------------------------------------------------------
# Case-level bootstrap replicates (bootstrap.hip; bootstrap.replicates)
# ---------------------------------------------------------------------------------------------------------
_BS_ARRAYS = (("case_label", torch.uint8, "N"), ("case_group_end", torch.uint8, "N"), ("case_lesions", torch.int32, "N"),
              ("ev_case", torch.int32, "M"), ("ev_tp", torch.uint8, "M"), ("ev_group_end", torch.uint8, "M"))


def bootstrap_metrics(table: dict, n_boot: int, seed: int = 0, stratified: bool = False, fp_rates: Sequence[float] = (0.5, 1.0, 2.0),
                      weights: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``n_boot`` bootstrap replicates of [auroc, ap, sens@fp_rates..., mean of every value row] in one launch (m1_bootstrap_metrics,
    include/m1hip.h) -> (n_boot, 2 + len(fp_rates) + V) fp64 on the device.  ``table``: device tensors in the packed order of
    ``bootstrap.pack`` (``bootstrap.to_device`` makes them): case_label / case_group_end uint8 (N,), case_lesions int32 (N,), ev_case
    int32 (M,), ev_tp / ev_group_end uint8 (M,), optionally values fp64 (V, N) -- one ROW per scalar --, case_rank int32 (N,) (the packed
    position of every original case: what a draw's index goes through; absent = identity) and, for ``stratified``, strat_perm int32 (N,)
    with the int ``P`` in its place.  ``weights``: int32 (n_boot, N) in the packed case order, replacing the draw.  Nothing
    is read back and every argument is checked before the launch."""
    _no_grad_only("bootstrap_metrics")
    ts = {}
    for name, dt, dim in _BS_ARRAYS:
        t = table.get(name)
        if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != 1:
            raise RuntimeError(f"bootstrap_metrics: table[{name!r}] must be a 1-d {dt} device tensor")
        ts[name] = t
    N, M = int(ts["case_label"].numel()), int(ts["ev_case"].numel())
    for name, _, dim in _BS_ARRAYS:
        if ts[name].numel() != (N if dim == "N" else M):
            raise RuntimeError(f"bootstrap_metrics: table[{name!r}] holds {ts[name].numel()} entries, {dim} = {N if dim == 'N' else M} expected")
    values, V = table.get("values"), 0
    if values is not None and values.numel():
        if values.dtype != torch.float64 or values.dim() != 2 or int(values.shape[1]) != N:
            raise RuntimeError(f"bootstrap_metrics: table['values'] must be fp64 (V, {N}), got {values.dtype} {tuple(values.shape)}")
        V = int(values.shape[0])
    else:
        values = None
    perm, P = table.get("case_rank"), -1                                   # (None: the draw indexes the packed order itself)
    if stratified:
        perm, P = table.get("strat_perm"), int(table.get("P", -1))
        if perm is None or not 0 <= P <= N:
            raise RuntimeError("bootstrap_metrics: a stratified draw needs table['strat_perm'] and 0 <= table['P'] <= N")
    if perm is not None and (not isinstance(perm, torch.Tensor) or perm.dtype != torch.int32 or tuple(perm.shape) != (N,)):
        raise RuntimeError(f"bootstrap_metrics: the draw's permutation must be int32 ({N},)")
    n_boot, rates = int(n_boot), [float(x) for x in fp_rates]
    if weights is not None and (weights.dtype != torch.int32 or tuple(weights.shape) != (n_boot, N)):
        raise RuntimeError(f"bootstrap_metrics: weights must be int32 {(n_boot, N)}, got {weights.dtype} {tuple(weights.shape)}")
    _req(*ts.values(), values, perm, weights, out)
    S = 2 + len(rates) + V
    if out is None:
        out = torch.empty((max(n_boot, 0), S), dtype=torch.float64, device=ts["case_label"].device)
    elif out.dtype != torch.float64 or tuple(out.shape) != (n_boot, S):
        raise RuntimeError(f"bootstrap_metrics: out must be fp64 {(n_boot, S)}, got {out.dtype} {tuple(out.shape)}")
    tb = L.m1_bootstrap_table_t()
    for name in ts:
        setattr(tb, name, ts[name].data_ptr() or None)
    tb.values, tb.draw_perm = _p(values), _p(perm)
    tb.N, tb.M, tb.V, tb.P = N, M, V, P
    L.check(L.load().m1_bootstrap_metrics(C.byref(tb), n_boot, int(seed) & (2 ** 64 - 1), _p(weights), (C.c_double * max(len(rates), 1))(*rates),
                                          len(rates), _p(out), _stream()), "m1_bootstrap_metrics")
    return out


# ---------------------------------------------------------------------------------------------------------
# Focal loss on the softmax heads (losses.py:32-49)
# ---------------------------------------------------------------------------------------------------------
class _Focal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y_true, y_pred, alpha, gamma):
        _req(y_true, y_pred)
        if y_pred.dtype != torch.float32:
            raise RuntimeError("focal_loss: y_pred must be the fp32 probabilities of softmax_heads")
        nc = int(y_true.shape[-1])
        nheads = int(y_pred.shape[-1]) // nc
        if nheads * nc != int(y_pred.shape[-1]) or len(alpha) != nc or y_true.shape[:-1] != y_pred.shape[:-1]:
            raise RuntimeError("focal_loss: y_pred must hold nheads*nc channels over the voxels of y_true, alpha nc weights")
        if y_true.dtype not in (torch.float32, torch.bfloat16):
            y_true = y_true.to(torch.float32)
        N = int(y_pred.shape[0])
        V = y_true.numel() // (N * nc)
        lib = L.load()
        al = (C.c_float * nc)(*[float(a) for a in alpha])
        ws = torch.empty(max(int(lib.m1_focal_ws_floats(N, V, nheads)), 1), dtype=torch.float32, device=y_pred.device)
        loss = torch.empty((), dtype=torch.float32, device=y_pred.device)
        L.check(lib.m1_focal_fwd(_p(y_pred), _p(y_true), _dt(y_true), al, float(gamma), N, V, nheads, nc, _p(ws), _p(loss),
                                 _stream()), "m1_focal_fwd")
        ctx.save_for_backward(y_true, y_pred)
        ctx.cfg = (al, float(gamma), N, V, nheads, nc)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        y_true, y_pred = ctx.saved_tensors
        al, gamma, N, V, nheads, nc = ctx.cfg
        dloss = dloss.contiguous().float()
        dp = torch.empty_like(y_pred)
        L.check(L.load().m1_focal_bwd(_p(y_pred), _p(y_true), _dt(y_true), al, gamma, N, V, nheads, nc, _p(dloss), _p(dp),
                                      _stream()), "m1_focal_bwd")
        return None, dp, None, None


def focal_loss(y_true: torch.Tensor, y_pred: torch.Tensor, alpha: Sequence[float], gamma: float) -> torch.Tensor:
    """Focal.loss (losses.py:43-49) over all heads of ``y_pred`` in one pass; gradient w.r.t. ``y_pred`` only."""
    return _Focal.apply(y_true.contiguous(), y_pred.contiguous(), tuple(float(a) for a in alpha), float(gamma))


def _label_dtype(y_true: torch.Tensor) -> torch.Tensor:
    return y_true if y_true.dtype in (torch.float32, torch.bfloat16) else y_true.to(torch.float32)


def dist_map(y_true: torch.Tensor) -> torch.Tensor:
    """SoftDicePlusBoundarySurface.calc_dist_map_batch (losses.py:83-97) of the foreground classes: y_true (N,D,H,W,nc) one-hot
    -> signed Euclidean distance map phi (N,D,H,W,nc-1) fp32 (m1_dist_map; dice_boundary.hip).  No autograd: phi is a label."""
    _req(y_true)
    if y_true.dim() != 5 or int(y_true.shape[-1]) < 2:
        raise RuntimeError("dist_map: y_true must be (N,D,H,W,nc) with nc >= 2 (class 0 is the background)")
    y_true = _label_dtype(y_true).contiguous()
    N, D, H, W, nc = (int(v) for v in y_true.shape)
    lib = L.load()
    ws = torch.empty(max(int(lib.m1_dist_map_ws_bytes(N, D, H, W, nc)), 1), dtype=torch.uint8, device=y_true.device)
    out = torch.empty((N, D, H, W, nc - 1), dtype=torch.float32, device=y_true.device)
    L.check(lib.m1_dist_map(_p(y_true), _dt(y_true), N, D, H, W, nc, _p(ws), _p(out), _stream()), "m1_dist_map")
    return out


class _DiceBoundary(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y_true, y_pred, w0, w1, smooth):
        _req(y_true, y_pred)
        if y_pred.dtype != torch.float32:
            raise RuntimeError("dice_boundary_loss: y_pred must be the fp32 probabilities of softmax_heads")
        nc = int(y_true.shape[-1])
        nheads = int(y_pred.shape[-1]) // nc
        if nheads * nc != int(y_pred.shape[-1]) or y_true.shape[:-1] != y_pred.shape[:-1] or y_true.dim() != 5:
            raise RuntimeError("dice_boundary_loss: y_pred must hold nheads*nc channels over the (N,D,H,W) voxels of y_true")
        y_true = _label_dtype(y_true)
        phi = dist_map(y_true)
        NV = y_true.numel() // nc
        lib = L.load()
        ws = torch.empty(max(int(lib.m1_dice_bd_ws_floats(NV, nheads)), 2), dtype=torch.float32, device=y_pred.device)
        loss = torch.empty((), dtype=torch.float32, device=y_pred.device)
        L.check(lib.m1_dice_bd_fwd(_p(y_pred), _p(y_true), _dt(y_true), _p(phi), NV, nheads, nc, w0, w1, smooth, _p(ws), _p(loss),
                                   _stream()), "m1_dice_bd_fwd")
        ctx.save_for_backward(y_true, y_pred, phi, ws)
        ctx.cfg = (NV, nheads, nc, w0, w1, smooth)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        y_true, y_pred, phi, ws = ctx.saved_tensors
        NV, nheads, nc, w0, w1, smooth = ctx.cfg
        dloss = dloss.contiguous().float()
        dp = torch.empty_like(y_pred)
        L.check(L.load().m1_dice_bd_bwd(_p(y_pred), _p(y_true), _dt(y_true), _p(phi), NV, nheads, nc, w0, w1, smooth, _p(ws),
                                        _p(dloss), _p(dp), _stream()), "m1_dice_bd_bwd")
        return None, dp, None, None, None


def dice_boundary_loss(y_true: torch.Tensor, y_pred: torch.Tensor, weights: Sequence[float], smooth: float) -> torch.Tensor:
    """SoftDicePlusBoundarySurface.loss (losses.py:66-130) over all heads of ``y_pred``: the distance map of ``y_true`` once per
    call, then one fused forward pass (m1_dice_bd_fwd / m1_dice_bd_bwd); gradient w.r.t. ``y_pred`` only."""
    if len(weights) != 2:
        raise RuntimeError("dice_boundary_loss: weights must be [dice weight, boundary weight]")
    return _DiceBoundary.apply(y_true.contiguous(), y_pred.contiguous(), float(weights[0]), float(weights[1]), float(smooth))


# ---------------------------------------------------------------------------------------------------------
# train-time augmentations (augment.hip; augmentations.py is the public surface)
# ---------------------------------------------------------------------------------------------------------
AUG_RECORD_BYTES = C.sizeof(L.m1_aug_params_t)


def _aug_table(table: torch.Tensor, N: int) -> torch.Tensor:
    _req(table)
    if table.dtype != torch.uint8 or table.numel() != N * AUG_RECORD_BYTES:
        raise RuntimeError(f"augmentation table: expected {N} records of {AUG_RECORD_BYTES} bytes (uint8), got {tuple(table.shape)} {table.dtype}")
    return table


def aug_draw(N: int, rng: torch.Tensor, stream_id: int, hyper: Sequence, H: int, W: int, nimg: int, lesion: bool) -> torch.Tensor:
    """m1_aug_draw: the (N, record bytes) uint8 table of one batch, drawn on the device from the {seed, step} pair ``rng``.
    ``hyper``: prob, tx_prob, translate_factor, rotation_degree, axial_hflip, zoom_factor, gauss_noise_stddev, chan_shift_factor,
    sim_poor_scan, gamma_lo, gamma_hi (A:39-48)."""
    _req(rng)
    p, tx, tr, rot, flip, zoom, noise, cs, poor, g0, g1 = hyper
    table = torch.empty((int(N), AUG_RECORD_BYTES), dtype=torch.uint8, device=rng.device)
    flip = int(flip == True)                                     # noqa: E712 -- `axial_hflip==True` (A:65), the rule of augmentations.enabled_stages
    L.check(L.load().m1_aug_draw(_p(table), int(N), _p(rng), int(stream_id), float(p), float(tx), float(tr), float(rot), flip,
                                 float(zoom), float(noise), float(cs), int(bool(poor)), float(g0), float(g1), int(H), int(W), int(nimg),
                                 int(bool(lesion)), _stream()), "m1_aug_draw")
    return table


def aug_apply(x: torch.Tensor, y: Optional[torch.Tensor], table: torch.Tensor, stages: int, nimg: int,
              rng: Optional[torch.Tensor] = None, stream_id: int = 0):
    """The whole chain of A:36-132 on a batch: m1_aug_geom (+ m1_aug_gamma_stats + m1_aug_intensity when an intensity stage is
    enabled in ``stages``).  x (N,D,H,W,C) fp32, y (N,D,H,W,nc) fp32 or None; returns (image, label)."""
    _req(x, y, rng)
    if x.dim() != 5 or (y is not None and (y.dim() != 5 or y.shape[:4] != x.shape[:4])):
        raise RuntimeError("augmentations: image (N,D,H,W,C) and label (N,D,H,W,nc) over the same voxels expected")
    if x.dtype != torch.float32 or (y is not None and y.dtype != torch.float32):
        raise RuntimeError("augmentations: fp32 image and label expected (what the generator yields)")
    N, D, H, W, Cn = (int(v) for v in x.shape)
    nc = int(y.shape[-1]) if y is not None else 0
    _aug_table(table, N)
    lib, st = L.load(), _stream()
    ws = torch.empty(max(int(lib.m1_aug_ws_bytes(N, D, H, W, int(nimg))), 8) // 8, dtype=torch.float64, device=x.device)
    gx = torch.empty_like(x)
    gy = torch.empty_like(y) if y is not None else None
    dims = (N, D, H, W, Cn, int(nimg))
    L.check(lib.m1_aug_geom(_p(x), _p(y), _p(table), _p(gx), _p(gy), *dims, nc, int(stages), L.M1_F32, _p(ws), st), "m1_aug_geom")
    if not stages & (L.M1_AUG_GAMMA | L.M1_AUG_POOR | L.M1_AUG_NOISE):
        return gx, gy
    if stages & L.M1_AUG_NOISE and rng is None:
        raise RuntimeError("augmentations: the noise stage needs a device {seed, step} pair (rng=)")
    if stages & L.M1_AUG_GAMMA:
        L.check(lib.m1_aug_gamma_stats(_p(gx), _p(table), *dims, int(stages), L.M1_F32, _p(ws), st), "m1_aug_gamma_stats")
    out = torch.empty_like(x)
    L.check(lib.m1_aug_intensity(_p(gx), _p(table), _p(rng), int(stream_id), _p(out), *dims, int(stages), L.M1_F32, _p(ws), st),
            "m1_aug_intensity")
    return out, gy


# ---------------------------------------------------------------------------------------------------------
# label preparation of the data generator (labels.hip; data_generators.py is the public surface)
# ---------------------------------------------------------------------------------------------------------
LABEL_TILE = 32                     # tile edge of the label kernels (labels.hip LT): the sizes around it are what the tests probe
LABEL_TAPS = (31, 36, 40, 42, 40, 36, 31)          # data_generators.gaussian_taps_u8(7, 4.0), the default of both wrappers
_OBJECTIVES = {"lesion": L.M1_LABEL_LESION, "zonal": L.M1_LABEL_ZONAL}
_FEED_MODES = {"train": L.M1_FEED_TRAIN, "valid": L.M1_FEED_VALID, "test": L.M1_FEED_TEST}


def _taps(taps) -> "C.Array":
    taps = LABEL_TAPS if taps is None else tuple(int(v) for v in taps)
    if len(taps) != 7:
        raise NotImplementedError(f"label kernels: only 7 taps (the reference's (7,7) kernel) are built, got {len(taps)}")
    return (C.c_int * 7)(*taps)


def contour_smooth(mask: torch.Tensor, iterations: int = 1, taps=None) -> torch.Tensor:
    """contour_smoothening (data_generators.py:92-97) of a uint8 mask (..., H, W), every H x W slice on its own, as the integer rule
    of m1_contour_smooth_u8; returns a new tensor."""
    _req(mask)
    if mask.dtype != torch.uint8 or mask.dim() < 2:
        raise RuntimeError(f"contour_smooth: a uint8 mask (..., H, W) expected, got {mask.dtype} {tuple(mask.shape)}")
    H, W = int(mask.shape[-2]), int(mask.shape[-1])
    out = torch.empty_like(mask)
    scratch = torch.empty_like(mask) if int(iterations) > 1 else None
    L.check(L.load().m1_contour_smooth_u8(_p(mask), _p(out), _p(scratch), mask.numel() // max(H * W, 1), H, W, _taps(taps),
                                          int(iterations), _stream()), "m1_contour_smooth_u8")
    return out


def prepare_labels(ann: Optional[torch.Tensor], image: torch.Tensor, train_obj: str = "lesion", mode: str = "train",
                   probabilistic: bool = False, taps=None):
    """The generator's batch from the raw arrays in one launch (m1_label_prepare): ``ann`` (B,D,H,W) uint8 grades / zones (None for
    ``mode='test'``), ``image`` (B,D,H,W,C) fp32 -> (network input, detection, KL or None), all fp32 on the device."""
    _req(ann, image)
    if train_obj not in _OBJECTIVES or mode not in _FEED_MODES:
        raise RuntimeError(f"prepare_labels: train_obj 'lesion' / 'zonal' and mode 'train' / 'valid' / 'test', got {train_obj!r}, {mode!r}")
    if image.dim() != 5 or image.dtype != torch.float32:
        raise RuntimeError(f"prepare_labels: an fp32 image (B,D,H,W,C) expected, got {image.dtype} {tuple(image.shape)}")
    if ann is not None and (ann.dtype != torch.uint8 or tuple(ann.shape) != tuple(image.shape[:4])):
        raise RuntimeError(f"prepare_labels: a uint8 annotation {tuple(image.shape[:4])} expected, got {ann.dtype} {tuple(ann.shape)}")
    B, D, H, W, Cn = (int(v) for v in image.shape)
    nc = 2 if train_obj == "lesion" else 3
    keep = Cn if train_obj == "lesion" else 1
    prob = bool(probabilistic)
    x = torch.empty((B, D, H, W, keep + (nc - 1 if prob else 0)), dtype=torch.float32, device=image.device)
    det = torch.empty((B, D, H, W, nc), dtype=torch.float32, device=image.device)
    kl = torch.empty_like(det) if prob else None
    L.check(L.load().m1_label_prepare(_p(ann), _p(image), _p(x), _p(det), _p(kl), B, D, H, W, Cn, _OBJECTIVES[train_obj],
                                      _FEED_MODES[mode], int(prob), _taps(taps), _stream()), "m1_label_prepare")
    return x, det, kl


# ---------------------------------------------------------------------------------------------------------
# scan preprocessing (preprocess.hip, resample.hip; preprocess.py is the public surface)
# ---------------------------------------------------------------------------------------------------------
PAD_MODES = {"constant": L.M1_PAD_CONSTANT, "edge": L.M1_PAD_EDGE, "reflect": L.M1_PAD_REFLECT, "symmetric": L.M1_PAD_SYMMETRIC}
_RAW_DTYPES = {torch.float32: L.M1_RAW_F32, torch.int16: L.M1_RAW_I16}


def _raw(src: torch.Tensor, what: str):
    _req(src)
    if src.dim() != 5 or src.dtype not in _RAW_DTYPES:
        raise RuntimeError(f"{what}: a raw fp32 / int16 source (B,d,h,w,C) expected, got {src.dtype} {tuple(src.shape)}")
    return int(src.shape[0]), int(src.shape[4]), _RAW_DTYPES[src.dtype]


def crop_pad_geom(src_dims, dst, start, mode: str = "constant", cval: float = 0.0) -> L.m1_crop_pad_t:
    """The m1_crop_pad_t of a (d,h,w) source: output voxel o of an axis reads source index o + start."""
    if mode not in PAD_MODES:
        raise NotImplementedError(f"pad mode {mode!r}: built are {sorted(PAD_MODES)}")
    if len(dst) != 3 or len(start) != 3 or any(int(v) < 1 for v in dst):
        raise RuntimeError(f"crop / pad geometry: three positive output extents and three starts expected, got {tuple(dst)}, {tuple(start)}")
    g = L.m1_crop_pad_t()
    g.src[:], g.dst[:], g.start[:] = [int(v) for v in src_dims], [int(v) for v in dst], [int(v) for v in start]
    g.mode, g.cval = PAD_MODES[mode], float(cval)
    return g


def _out_dtype(dtype) -> int:
    if dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"preprocessing output: float32 / bfloat16 only, got {dtype}")
    return L.M1_F32 if dtype == torch.float32 else L.M1_BF16


def _pp_ws(g, B: int, Cn: int, nq: int, device) -> torch.Tensor:
    n = int(L.load().m1_preprocess_ws_bytes(C.byref(g), B, Cn, nq))
    return torch.empty(max(n, 8) // 8, dtype=torch.float64, device=device)


def crop_pad(src: torch.Tensor, dst, start, mode: str = "constant", cval: float = 0.0, dtype=torch.float32) -> torch.Tensor:
    """m1_crop_pad: the crop / pad gather of a raw (B,d,h,w,C) fp32 / int16 source -> (B,*dst,C) in ``dtype``."""
    B, Cn, raw = _raw(src, "crop_pad")
    g = crop_pad_geom(src.shape[1:4], dst, start, mode, cval)
    out = torch.empty((B, *[int(v) for v in dst], Cn), dtype=dtype, device=src.device)
    L.check(L.load().m1_crop_pad(_p(src), raw, C.byref(g), B, Cn, _p(out), _out_dtype(dtype), _stream()), "m1_crop_pad")
    return out


def order_stats(src: torch.Tensor, dst, start, ranks, weights, mode: str = "constant", cval: float = 0.0):
    """m1_order_stats over the output domain of every (b, c) slice: (pairs (B,C,nq,2) fp32 = the exact {a[rank], a[min(rank+1,n-1)]},
    values (B,C,nq) fp32 = their fp64 interpolation by ``weights`` rounded once).  ``ranks`` / ``weights``: host sequences
    (preprocess.percentile_rank)."""
    B, Cn, raw = _raw(src, "order_stats")
    g = crop_pad_geom(src.shape[1:4], dst, start, mode, cval)
    nq = len(ranks)
    if nq < 1 or len(weights) != nq:
        raise RuntimeError("order_stats: one weight per rank and at least one rank expected")
    pairs = torch.empty((B, Cn, nq, 2), dtype=torch.float32, device=src.device)
    values = torch.empty((B, Cn, nq), dtype=torch.float32, device=src.device)
    ws = _pp_ws(g, B, Cn, min(nq, 4), src.device)
    L.check(L.load().m1_order_stats(_p(src), raw, C.byref(g), B, Cn, (C.c_int * nq)(*[int(k) for k in ranks]),
                                    (C.c_double * nq)(*[float(w) for w in weights]), nq, _p(pairs), _p(values), _p(ws), _stream()),
            "m1_order_stats")
    return pairs, values


def whiten(src: torch.Tensor, dst, start, mode: str = "constant", cval: float = 0.0, bounds: Optional[torch.Tensor] = None,
           dtype=torch.float32):
    """m1_whiten: every (b, c) slice of the cropped / padded source clipped to ``bounds`` ((B,C,2) fp32 {lo, hi} on the device, or
    None) and standardised -> (out (B,*dst,C) in ``dtype``, stats (B,C,2) fp64 {mean, std})."""
    B, Cn, raw = _raw(src, "whiten")
    _req(bounds)
    g = crop_pad_geom(src.shape[1:4], dst, start, mode, cval)
    if bounds is not None and (bounds.dtype != torch.float32 or tuple(bounds.shape) != (B, Cn, 2)):
        raise RuntimeError(f"whiten: bounds must be fp32 {(B, Cn, 2)}, got {bounds.dtype} {tuple(bounds.shape)}")
    out = torch.empty((B, *[int(v) for v in dst], Cn), dtype=dtype, device=src.device)
    stats = torch.empty((B, Cn, 2), dtype=torch.float64, device=src.device)
    ws = _pp_ws(g, B, Cn, 0, src.device)
    L.check(L.load().m1_whiten(_p(src), raw, C.byref(g), B, Cn, _p(bounds), _p(out), _out_dtype(dtype), _p(stats), _p(ws), _stream()),
            "m1_whiten")
    return out, stats


def resample_geom(src_dims, step, dst, first=(0, 0, 0), order: int = 3, default_value: float = 0.0) -> L.m1_resample_t:
    """The m1_resample_t of a (d,h,w) source: output o of an axis reads the continuous source index (first + o) * step."""
    if len(step) != 3 or len(dst) != 3 or len(first) != 3 or any(int(v) < 1 for v in dst):
        raise RuntimeError(f"resampling geometry: three steps, three positive output extents and three firsts expected, got "
                           f"{tuple(step)}, {tuple(dst)}, {tuple(first)}")
    if order not in (0, 3):
        raise NotImplementedError(f"resample: order {order!r} is not built; 0 (nearest) and 3 (cubic B-spline) are")
    g = L.m1_resample_t()
    g.src[:], g.dst[:], g.first[:] = [int(v) for v in src_dims], [int(v) for v in dst], [int(v) for v in first]
    g.step[:] = [float(v) for v in step]
    g.order, g.defval = int(order), float(default_value)
    return g


def resample(src: torch.Tensor, step, dst=None, first=(0, 0, 0), order: int = 3, default_value: float = 0.0) -> torch.Tensor:
    """m1_resample: a raw (B,d,h,w,C) fp32 / int16 source on the grid whose output o of an axis reads the continuous source index
    (first + o) * step -> (B,*dst,C), fp32 for order 3 (cubic B-spline), the source's dtype for order 0 (nearest neighbour).  ``step``
    is three numbers (out_spacing / spacing per axis) with ``dst`` / ``first``, or a ready m1_resample_t."""
    B, Cn, raw = _raw(src, "resample")
    g = step if isinstance(step, L.m1_resample_t) else resample_geom(src.shape[1:4], step, dst, first, order, default_value)
    if tuple(g.src) != tuple(int(v) for v in src.shape[1:4]):
        raise RuntimeError(f"resample: the geometry is for a source {tuple(g.src)}, got {tuple(src.shape[1:4])}")
    lib = L.load()
    cubic = g.order == 3
    out = torch.empty((B, *[int(v) for v in g.dst], Cn), dtype=torch.float32 if cubic else src.dtype, device=src.device)
    ws, odt = None, raw                                 # (order 0 keeps the type and needs no workspace)
    if cubic:
        odt = _out_dtype(out.dtype)                     # (M1_F32 and M1_RAW_F32 are the same value)
        ws = torch.empty(max(int(lib.m1_resample_ws_bytes(C.byref(g), B, Cn)), 16) // 4, dtype=torch.float32, device=src.device)
    L.check(lib.m1_resample(_p(src), raw, C.byref(g), B, Cn, _p(out), odt, _p(ws), _stream()), "m1_resample")
    return out


_RESTORE_DTYPES = {**_RAW_DTYPES, torch.int32: L.M1_RAW_I32}


def restore_geom(src_dims, dst, ratio, first, count, lo, order: int = 1, default_value: float = 0.0,
                 default_label: int = 0) -> L.m1_restore_t:
    """The m1_restore_t of a (D,H,W) map on the network's grid: scan voxel i of an axis of ``dst`` voxels sits at the window coordinate
    i * ratio - first and reads the real voxels [lo, lo + count) of the network axis (preprocess.restore_geometry computes the five)."""
    if any(len(v) != 3 for v in (src_dims, dst, ratio, first, count, lo)):
        raise RuntimeError(f"back-projection geometry: three values per field expected, got {tuple(src_dims)}, {tuple(dst)}, {tuple(ratio)}, "
                           f"{tuple(first)}, {tuple(count)}, {tuple(lo)}")
    if order not in (0, 1):
        raise NotImplementedError(f"restore: order {order!r} is not built; 0 (nearest) and 1 (linear) are")
    g = L.m1_restore_t()
    g.src[:], g.dst[:] = [int(v) for v in src_dims], [int(v) for v in dst]
    g.first[:], g.count[:], g.lo[:] = [int(v) for v in first], [int(v) for v in count], [int(v) for v in lo]
    g.ratio[:] = [float(v) for v in ratio]
    g.order, g.defval, g.deflabel = int(order), float(default_value), int(default_label)
    return g


def restore(src: torch.Tensor, geom: L.m1_restore_t, c0: int = 0, nsel: Optional[int] = None, prob: bool = True, label: bool = False):
    """m1_restore: a (B,D,H,W,C) fp32 map on the network's grid (int16 / int32 as well for order 0) -> on the scan's grid ``geom.dst``, in one
    launch: ``prob`` (B,*dst,nsel) = the channels [c0, c0 + nsel) in the source's dtype (nsel None: all from c0 on) and / or ``label``
    (B,*dst) uint8 = the argmax over all C restored channels.  Returns the one asked for, or (prob, label)."""
    _req(src)
    if src.dim() != 5 or src.dtype not in _RESTORE_DTYPES:
        raise RuntimeError(f"restore: an fp32 / int16 / int32 map (B,D,H,W,C) expected, got {src.dtype} {tuple(src.shape)}")
    B, Cn, raw = int(src.shape[0]), int(src.shape[4]), _RESTORE_DTYPES[src.dtype]
    if tuple(geom.src) != tuple(int(v) for v in src.shape[1:4]):
        raise RuntimeError(f"restore: the geometry is for a source {tuple(geom.src)}, got {tuple(src.shape[1:4])}")
    if not (prob or label):
        raise RuntimeError("restore: at least one of prob / label expected")
    c0 = int(c0)
    nsel = Cn - c0 if nsel is None else int(nsel)
    dst = [int(v) for v in geom.dst]
    out = torch.empty((B, *dst, nsel), dtype=src.dtype, device=src.device) if prob else None
    lab = torch.empty((B, *dst), dtype=torch.uint8, device=src.device) if label else None
    L.check(L.load().m1_restore(_p(src), raw, C.byref(geom), B, Cn, c0, nsel, _p(out), _p(lab), _stream()), "m1_restore")
    return (out, lab) if prob and label else out if prob else lab


# ---------------------------------------------------------------------------------------------------------
# connected components, lesion candidates and matching (components.hip; detection.py is the public surface)
# ---------------------------------------------------------------------------------------------------------
_CC_DTYPES = {torch.float32: L.M1_CC_F32, torch.uint8: L.M1_CC_U8}
CC_STATE_WORDS = 8


def _cc_vol(t: torch.Tensor, what: str, dtypes) -> Tuple[int, int, int, int]:
    _req(t)
    if t.dim() != 4 or t.dtype not in dtypes:
        raise RuntimeError(f"{what}: a (B,D,H,W) volume of {' / '.join(str(d) for d in dtypes)} expected, got {t.dtype} {tuple(t.shape)}")
    return tuple(int(v) for v in t.shape)


def _cc_same(a: torch.Tensor, b: Optional[torch.Tensor], what: str, dtype) -> None:
    _req(b)
    if b is not None and (b.dtype != dtype or b.shape != a.shape):
        raise RuntimeError(f"{what}: {dtype} of shape {tuple(a.shape)} expected, got {b.dtype} {tuple(b.shape)}")


def cc_workspace(shape, device) -> torch.Tensor:
    """The workspace of label_components / cc_peak for (B,D,H,W) volumes (m1_cc_ws_bytes), from torch's allocator."""
    B, D, H, W = (int(v) for v in shape)
    return torch.empty(max(int(L.load().m1_cc_ws_bytes(B, D, H, W)), 16) // 4, dtype=torch.int32, device=device)


def _cc_ws(ws: Optional[torch.Tensor], shape, device) -> torch.Tensor:
    if ws is None:
        return cc_workspace(shape, device)
    _req(ws)
    need = int(L.load().m1_cc_ws_bytes(*[int(v) for v in shape]))
    if ws.numel() * ws.element_size() < need:
        raise RuntimeError(f"components workspace: {need} bytes needed for {tuple(shape)}, got {ws.numel() * ws.element_size()}")
    return ws


def label_components(x: torch.Tensor, threshold=0.0, connectivity: int = 3, ws: Optional[torch.Tensor] = None):
    """m1_cc_label: the connected components of ``x > threshold`` for a (B,D,H,W) fp32 / uint8 volume -> (labels (B,D,H,W) int32 numbered
    as scipy.ndimage.label numbers them, per batch entry; counts (B,) int32).  ``threshold``: a number, or a (B,) fp32 device tensor
    (one threshold per batch entry, no host read).  ``ws``: cc_workspace(x.shape), or None to allocate it."""
    B, D, H, W = _cc_vol(x, "label_components", tuple(_CC_DTYPES))
    thr_dev = None
    if isinstance(threshold, torch.Tensor):
        _req(threshold)
        if threshold.dtype != torch.float32 or threshold.numel() != B:
            raise RuntimeError(f"label_components: a per-sample threshold is {B} fp32 values, got {threshold.dtype} {tuple(threshold.shape)}")
        thr_dev, threshold = threshold, 0.0
    ws = _cc_ws(ws, x.shape, x.device)
    labels = torch.empty(x.shape, dtype=torch.int32, device=x.device)
    counts = torch.empty(B, dtype=torch.int32, device=x.device)
    L.check(L.load().m1_cc_label(_p(x), _CC_DTYPES[x.dtype], float(threshold), _p(thr_dev), int(connectivity), B, D, H, W, _p(labels),
                                 _p(counts), _p(ws), _stream()), "m1_cc_label")
    return labels, counts


def _cc_rows_dict(rows: torch.Tensor) -> dict:
    """The fields of a (B,K,16) int32 tensor of m1_cc_row_t as views."""
    r64 = rows.view(torch.int64)
    return {"count": rows[..., 0], "max": rows.view(torch.float32)[..., 1], "argmax": r64[..., 1], "lo": rows[..., 4:7],
            "hi": rows[..., 7:10], "sum": r64[..., 5:8], "rows": rows}


def component_stats(labels: torch.Tensor, values: Optional[torch.Tensor] = None, max_components: int = 64) -> dict:
    """m1_cc_stats: the per-component table of (B,D,H,W) int32 ``labels`` -> dict of (B,K,...) tensors: count, max and argmax of
    ``values`` (linear index inside the batch entry, ties to the smallest), lo / hi (bounding box, hi exclusive), sum (int64
    coordinate sums), and ``rows``, the raw (B,K,16) int32 table they are views of."""
    B, D, H, W = _cc_vol(labels, "component_stats", (torch.int32,))
    _cc_same(labels, values, "component_stats values", torch.float32)
    K = int(max_components)
    rows = torch.empty((B, max(K, 1), C.sizeof(L.m1_cc_row_t) // 4), dtype=torch.int32, device=labels.device)
    L.check(L.load().m1_cc_stats(_p(labels), _p(values), B, D, H, W, K, _p(rows), _stream()), "m1_cc_stats")
    return _cc_rows_dict(rows)


def component_overlap(a: torch.Tensor, b: torch.Tensor, max_a: int, max_b: int) -> torch.Tensor:
    """m1_cc_overlap: (B, max_a + 1, max_b + 1) int32 counts of the voxels with labels (a, b); row / column 0 are background."""
    B = _cc_vol(a, "component_overlap", (torch.int32,))[0]
    _cc_same(a, b, "component_overlap", torch.int32)
    table = torch.empty((B, max(int(max_a), 0) + 1, max(int(max_b), 0) + 1), dtype=torch.int32, device=a.device)
    L.check(L.load().m1_cc_overlap(_p(a), _p(b), B, a.numel() // B, int(max_a), int(max_b), _p(table), _stream()), "m1_cc_overlap")
    return table


def cc_state(B: int, device) -> torch.Tensor:
    """The (8, B) int32 device state of the dynamic extraction (enum m1_cc_state); cc_peak(reset=True) initialises it."""
    return torch.empty((CC_STATE_WORDS, int(B)), dtype=torch.int32, device=device)


def _cc_state(state: torch.Tensor, B: int) -> None:
    _req(state)
    if state.dtype != torch.int32 or tuple(state.shape) != (CC_STATE_WORDS, B):
        raise RuntimeError(f"components state: int32 {(CC_STATE_WORDS, B)} expected, got {state.dtype} {tuple(state.shape)}")


def cc_peak(w: torch.Tensor, state: torch.Tensor, factor: float = 1.0, min_confidence: float = float("-inf"), reset: bool = False,
            ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """m1_cc_peak: per sample of the (B,D,H,W) fp32 ``w`` the maximum and its index (ties to the smallest) into ``state``, with
    THRESHOLD = PEAK / factor and DONE set where not PEAK > min_confidence."""
    B = _cc_vol(w, "cc_peak", (torch.float32,))[0]
    _cc_state(state, B)
    ws = _cc_ws(ws, w.shape, w.device)
    L.check(L.load().m1_cc_peak(_p(w), B, w.numel() // B, float(factor), float(min_confidence), int(bool(reset)), _p(state), _p(ws),
                                _stream()), "m1_cc_peak")
    return state


def cc_select(labels: torch.Tensor, state: torch.Tensor) -> torch.Tensor:
    """m1_cc_select: SEL = the label at each sample's ARGMAX and COUNT = its voxels."""
    B = _cc_vol(labels, "cc_select", (torch.int32,))[0]
    _cc_state(state, B)
    L.check(L.load().m1_cc_select(_p(labels), B, labels.numel() // B, _p(state), _stream()), "m1_cc_select")
    return state


def cc_take(labels: torch.Tensor, state: torch.Tensor, w: torch.Tensor, detection_map: torch.Tensor, candidates: torch.Tensor,
            confidences: torch.Tensor, min_voxels: int, reset: bool = False, w_src: Optional[torch.Tensor] = None) -> None:
    """m1_cc_take: the selected component leaves ``w`` and, when it has ``min_voxels``, becomes the next candidate of its sample in
    ``detection_map`` / ``candidates`` / ``confidences`` (B, n_max); ``reset`` initialises those three, and ``w`` from ``w_src`` when given (the round then ran on ``w_src``)."""
    B = _cc_vol(labels, "cc_take", (torch.int32,))[0]
    _cc_state(state, B)
    _cc_same(labels, w, "cc_take w", torch.float32)
    _cc_same(labels, w_src, "cc_take w_src", torch.float32)
    _cc_same(labels, detection_map, "cc_take detection_map", torch.float32)
    _cc_same(labels, candidates, "cc_take candidates", torch.int32)
    _req(confidences)
    if confidences.dtype != torch.float32 or confidences.dim() != 2 or confidences.shape[0] != B:
        raise RuntimeError(f"cc_take: confidences are fp32 (B, n), got {confidences.dtype} {tuple(confidences.shape)}")
    L.check(L.load().m1_cc_take(_p(labels), _p(state), _p(w_src if reset else None), _p(w), _p(detection_map), _p(candidates), _p(confidences), B, labels.numel() // B,
                                int(confidences.shape[1]), int(min_voxels), int(bool(reset)), _stream()), "m1_cc_take")


def cc_relabel(labels: torch.Tensor, stats: dict, min_voxels: int):
    """m1_cc_relabel: the components of ``labels`` with at least ``min_voxels`` voxels, renumbered in order, from the table of
    component_stats -> (detection_map fp32, candidates int32, confidences (B,K) fp32, ncand (B,) int32)."""
    B = _cc_vol(labels, "cc_relabel", (torch.int32,))[0]
    rows = stats["rows"]
    _req(rows)
    K = int(rows.shape[1])
    dev = labels.device
    cmap = torch.empty((B, K), dtype=torch.int32, device=dev)
    det = torch.empty(labels.shape, dtype=torch.float32, device=dev)
    cand = torch.empty(labels.shape, dtype=torch.int32, device=dev)
    conf = torch.empty((B, K), dtype=torch.float32, device=dev)
    ncand = torch.empty(B, dtype=torch.int32, device=dev)
    L.check(L.load().m1_cc_relabel(_p(labels), _p(rows), B, labels.numel() // B, K, int(min_voxels), _p(cmap), _p(det), _p(cand), _p(conf),
                                   _p(ncand), _stream()), "m1_cc_relabel")
    return det, cand, conf, ncand


# ---------------------------------------------------------------------------------------------------------
# surface-distance metrics (surface.hip; surface_distance.py is the public surface)
# ---------------------------------------------------------------------------------------------------------
_SD_DTYPES = {torch.uint8: L.M1_SD_U8, torch.int32: L.M1_SD_I32}
SD_ROW_WORDS = C.sizeof(L.m1_sd_row_t) // 4
SD_COUNT_KEYS = ("n_pred", "n_truth", "vol_pred", "vol_truth", "vol_both")


def sd_workspace(stage: int, B: int, K: int, shape, device) -> torch.Tensor:
    """The workspace of one surface-distance stage (L.M1_SD_STAGE_*) for (D,H,W) volumes (m1_sd_ws_bytes), from torch's allocator.
    For the distance stage ``B`` is the number of stacked volumes and ``K`` is not used."""
    D, H, W = (int(v) for v in shape)
    return torch.empty(max(int(L.load().m1_sd_ws_bytes(int(stage), int(B), int(K), D, H, W)), 16) // 4, dtype=torch.int32, device=device)


def _sd_ws(ws: Optional[torch.Tensor], stage: int, B: int, K: int, shape, device) -> torch.Tensor:
    if ws is None:
        return sd_workspace(stage, B, K, shape, device)
    _req(ws)
    need = int(L.load().m1_sd_ws_bytes(int(stage), int(B), int(K), *[int(v) for v in shape]))
    if ws.numel() * ws.element_size() < need:
        raise RuntimeError(f"surface-distance workspace: {need} bytes needed for {tuple(shape)}, got {ws.numel() * ws.element_size()}")
    return ws


def _sd_labels(labels) -> Tuple[int, ...]:
    labels = tuple(int(v) for v in labels)
    if not 1 <= len(labels) <= L.M1_SD_MAX_CLASSES:
        raise RuntimeError(f"surface distance: 1..{L.M1_SD_MAX_CLASSES} class ids expected, got {len(labels)}")
    return labels


def sd_border(pred: torch.Tensor, truth: torch.Tensor, labels=(1,), ws: Optional[torch.Tensor] = None):
    """m1_sd_border: for (B,D,H,W) uint8 / int32 label maps and K class ids -> (borders (2,B,K,D,H,W) uint8: the 6-neighbourhood
    border voxels of ``pred == labels[k]`` then of ``truth == labels[k]``, outside the volume counting as background; counts (B,K,5)
    int64: SD_COUNT_KEYS)."""
    B, D, H, W = _cc_vol(pred, "sd_border", tuple(_SD_DTYPES))
    _cc_same(pred, truth, "sd_border truth", pred.dtype)
    labels = _sd_labels(labels)
    K = len(labels)
    ws = _sd_ws(ws, L.M1_SD_STAGE_BORDER, B, K, (D, H, W), pred.device)
    borders = torch.empty((2, B, K, D, H, W), dtype=torch.uint8, device=pred.device)
    counts = torch.empty((B, K, 5), dtype=torch.int64, device=pred.device)
    L.check(L.load().m1_sd_border(_p(pred), _p(truth), _SD_DTYPES[pred.dtype], (C.c_int * K)(*labels), K, B, D, H, W, _p(borders),
                                  _p(counts), _p(ws), _stream()), "m1_sd_border")
    return borders, counts


def sd_distance(mask: torch.Tensor, spacing=(1.0, 1.0, 1.0), ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """m1_sd_distance: the exact Euclidean distance of every voxel of an (N,D,H,W) uint8 stack to the nearest non-zero voxel of its own
    volume, ``spacing`` in array-axis order (D,H,W); fp64 inside, fp32 out; +inf in a volume without a non-zero voxel."""
    N, D, H, W = _cc_vol(mask, "sd_distance", (torch.uint8,))
    spacing = tuple(float(v) for v in spacing)
    if len(spacing) != 3:
        raise RuntimeError(f"sd_distance: three spacings (D,H,W) expected, got {spacing}")
    ws = _sd_ws(ws, L.M1_SD_STAGE_DISTANCE, N, 1, (D, H, W), mask.device)      # (an unsupported shape asks for nothing and is refused below)
    dist = torch.empty(mask.shape, dtype=torch.float32, device=mask.device)
    L.check(L.load().m1_sd_distance(_p(mask), N, D, H, W, (C.c_double * 3)(*spacing), _p(dist), _p(ws), _stream()), "m1_sd_distance")
    return dist


def _sd_rows_dict(rows: torch.Tensor, T: int) -> dict:
    """The fields of a (B,K,40) int32 tensor of m1_sd_row_t as views."""
    r64, rf, rd = rows.view(torch.int64), rows.view(torch.float32), rows.view(torch.float64)
    out = {"n_ab": r64[..., 0], "n_ba": r64[..., 1], "le_ab": r64[..., 2:2 + T], "le_ba": r64[..., 6:6 + T], "sum_ab": rd[..., 10],
           "sum_ba": rd[..., 11], "rows": rows}
    for j, key in enumerate(("hd", "hd_ab", "hd_ba", "assd", "mean_ab", "mean_ba", "hdq", "hdq_ab", "hdq_ba", "dice")):
        out[key] = rf[..., 24 + j]
    out["nsd"] = rf[..., 34:34 + T]
    return out


def sd_metrics(borders: torch.Tensor, dist: torch.Tensor, counts: Optional[torch.Tensor] = None, percentile: float = 95.0,
               tolerances=(), ws: Optional[torch.Tensor] = None) -> dict:
    """m1_sd_metrics: from the (2,B,K,D,H,W) border masks of sd_border and the distances of those volumes to their own borders
    (sd_distance of the 2*B*K stack) -> dict of (B,K) device tensors (views of ``rows``, the raw (B,K,40) int32 table): the directed
    counts, fp64 sums and maxima, hd, assd, the ``percentile``-th percentiles hdq_ab / hdq_ba / hdq (pooled), nsd (B,K,T) and, when
    the ``counts`` of sd_border are given, dice."""
    _req(borders, dist, counts)
    if borders.dim() != 6 or borders.shape[0] != 2 or borders.dtype != torch.uint8:
        raise RuntimeError(f"sd_metrics: (2,B,K,D,H,W) uint8 border masks expected, got {borders.dtype} {tuple(borders.shape)}")
    if dist.shape != borders.shape or dist.dtype != torch.float32:
        raise RuntimeError(f"sd_metrics: fp32 distances of shape {tuple(borders.shape)} expected, got {dist.dtype} {tuple(dist.shape)}")
    _, B, K, D, H, W = (int(v) for v in borders.shape)
    if counts is not None and (counts.dtype != torch.int64 or tuple(counts.shape) != (B, K, 5)):
        raise RuntimeError(f"sd_metrics: counts are int64 {(B, K, 5)}, got {counts.dtype} {tuple(counts.shape)}")
    tolerances = tuple(float(v) for v in tolerances)
    T = len(tolerances)
    if T > L.M1_SD_MAX_TOLERANCES:
        raise RuntimeError(f"sd_metrics: at most {L.M1_SD_MAX_TOLERANCES} tolerances per call, got {T}")
    ws = _sd_ws(ws, L.M1_SD_STAGE_METRICS, B, K, (D, H, W), borders.device)
    rows = torch.empty((B, K, SD_ROW_WORDS), dtype=torch.int32, device=borders.device)
    L.check(L.load().m1_sd_metrics(_p(borders), _p(dist), _p(counts), B, K, D, H, W, float(percentile), (C.c_float * max(T, 1))(*tolerances),
                                   T, _p(rows), _p(ws), _stream()), "m1_sd_metrics")
    return _sd_rows_dict(rows, T)


# ---------------------------------------------------------------------------------------------------------
# dropout (standalone), cast
# ---------------------------------------------------------------------------------------------------------
class _Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rate, rng, layer_id):
        _req(x, rng)
        y = torch.empty_like(x)
        L.check(L.load().m1_dropout(_p(x), _p(y), x.numel(), float(rate), _p(rng), int(layer_id), _dt(x), _stream()), "m1_dropout")
        ctx.rate, ctx.rng, ctx.layer_id = float(rate), rng, int(layer_id)
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        L.check(L.load().m1_dropout(_p(dy), _p(dx), dy.numel(), ctx.rate, _p(ctx.rng), ctx.layer_id, _dt(dy), _stream()),
                "m1_dropout")
        return dx, None, None, None


def dropout(x, rate, rng, layer_id):
    if rate == 0.0:
        return x
    return _Dropout.apply(x, rate, rng, layer_id)


def cast(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """fp32 <-> bf16 activation cast (no autograd: used on network inputs only)."""
    _req(x)
    if x.dtype == dtype:
        return x
    y = torch.empty(x.shape, dtype=dtype, device=x.device)
    L.check(L.load().m1_cast(_p(x), _dt(x), _p(y), _dt(y), x.numel(), _stream()), "m1_cast")
    return y


# ---------------------------------------------------------------------------------------------------------
# optimizer / profiler
# ---------------------------------------------------------------------------------------------------------
def adam_amsgrad_(p, g, m, v, vhat, n_kernel, n_bias, l2_kernel, l2_bias, grad_scale, lr_dev, beta1, beta2, eps, step_dev):
    _req(p, g, m, v, vhat, lr_dev, step_dev)
    L.check(L.load().m1_adam_amsgrad(_p(p), _p(g), _p(m), _p(v), _p(vhat), p.numel(), int(n_kernel), int(n_bias),
                                     float(l2_kernel), float(l2_bias), float(grad_scale), _p(lr_dev), float(beta1), float(beta2),
                                     float(eps), _p(step_dev), _stream()), "m1_adam_amsgrad")


def step_advance(step_dev, rng_dev):
    L.check(L.load().m1_step_advance(_p(step_dev), _p(rng_dev), _stream()), "m1_step_advance")


# ---- guarded optimiser step (csrc/optim.hip): clipvalue / global_clipnorm / non-finite skip through a 16-byte device record ----
def grad_norm_ws(n: int) -> int:
    """Bytes of the workspace ``grad_norm_`` needs for n elements (host only)."""
    return int(L.load().m1_grad_norm_ws(int(n)))


def new_step_ctl(device) -> torch.Tensor:
    """A zeroed control record m1_step_ctl_t {float norm; float coef; int apply; int skipped} as four int32 words."""
    return torch.zeros(4, dtype=torch.int32, device=device)


def read_step_ctl(ctl: torch.Tensor) -> dict:
    """The record on the host (synchronises)."""
    w = ctl.cpu()
    f = w.view(torch.float32)
    return {"norm": float(f[0]), "coef": float(f[1]), "apply": int(w[2]), "skipped": int(w[3])}


def grad_norm_(g, p, n_kernel, n_bias, l2_kernel, l2_bias, grad_scale, clipvalue, global_clipnorm, skip_nonfinite, ws, ctl):
    """Norm pass + control pass: ``ctl`` receives the global norm of the (clamped) regularised gradient, the clip coefficient and the
    apply / skip decision.  0 switches clipvalue / global_clipnorm off.  ``ws``: at least grad_norm_ws(g.numel()) bytes."""
    _req(g, p, ws, ctl)
    L.check(L.load().m1_grad_norm(_p(g), _p(p), g.numel(), int(n_kernel), int(n_bias), float(l2_kernel), float(l2_bias),
                                  float(grad_scale), float(clipvalue), float(global_clipnorm), int(bool(skip_nonfinite)), _p(ws),
                                  ws.numel() * ws.element_size(), _p(ctl), _stream()), "m1_grad_norm")


def adam_amsgrad_ctl_(p, g, m, v, vhat, n_kernel, n_bias, l2_kernel, l2_bias, grad_scale, lr_dev, beta1, beta2, eps, step_dev,
                      clipvalue, ctl):
    """adam_amsgrad_ on clamp(gr, clipvalue) * ctl.coef; a no-op when ctl.apply == 0."""
    _req(p, g, m, v, vhat, lr_dev, step_dev, ctl)
    L.check(L.load().m1_adam_amsgrad_ctl(_p(p), _p(g), _p(m), _p(v), _p(vhat), p.numel(), int(n_kernel), int(n_bias),
                                         float(l2_kernel), float(l2_bias), float(grad_scale), _p(lr_dev), float(beta1), float(beta2),
                                         float(eps), _p(step_dev), float(clipvalue), _p(ctl), _stream()), "m1_adam_amsgrad_ctl")


def step_advance_ctl(step_dev, ctl):
    """step_dev += ctl.apply."""
    _req(step_dev, ctl)
    L.check(L.load().m1_step_advance_ctl(_p(step_dev), _p(ctl), _stream()), "m1_step_advance_ctl")


def set_force_direct(on: bool):
    """Test hook: route every conv through the generic direct kernels instead of the matrix-core kernels."""
    _FORCE_DIRECT[0] = bool(on)
    L.load().m1_set_force_direct(int(on) if not isinstance(on, bool) else (1 if on else 0))


_CFG_OVERRIDES = {}          # switches set through config_set (name -> value): what ``config`` restores on exit


def config_set(name: str, value: int) -> None:
    """Set a tuning switch of libm1hip.so (m1_config_set): effective from the next launch that consults it.  Switches such as
    M1_CONV_T3 / M1_CT3_BN / M1_CT3_KSPLIT / M1_HALO / M1_KORDER change the K order, padding and split-K slab size of the packed weight
    panels and the size of their workspaces, which are cached by layer geometry: every change drops the cached panels (they are
    re-packed, and their workspaces re-sized under the new plan, at the next use)."""
    L.check(L.load().m1_config_set(name.encode(), int(value)), "m1_config_set")
    _CFG_OVERRIDES[name] = int(value)
    invalidate_panels()


def config_unset(name: str) -> None:
    L.check(L.load().m1_config_unset(name.encode()), "m1_config_unset")
    _CFG_OVERRIDES.pop(name, None)
    invalidate_panels()


def config_get(name: str):
    """Current value of a switch, or None when nothing has consulted or set it yet."""
    v = C.c_int(0)
    return int(v.value) if L.load().m1_config_get(name.encode(), C.byref(v)) == 0 else None


class config:
    """``with ops.config(M1_T3_MIN_BLOCKS=1): ...`` -- switches set for the block; on exit each one returns to what it was before the
    block: the override an enclosing ``config`` / ``config_set`` had put there, or no override at all."""

    def __init__(self, **kv):
        self.kv = kv
        self.prev = {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.prev[k] = _CFG_OVERRIDES.get(k)          # None = there was no override
            config_set(k, v)
        return self

    def __exit__(self, *exc):
        for k in self.kv:
            if self.prev.get(k) is None:
                config_unset(k)
            else:
                config_set(k, self.prev[k])
        return False


class kernel_log:
    """``with ops.kernel_log() as kl: ...; kl.names`` -- the kernels the library's dispatch launched for the conv-like entry points
    inside the block (m1_debug_kernels), e.g. ['conv_t3:bn160:ks2', 'wgrad_t3:kws16:big1'].  ``kl.ran('conv_t3')`` is true when a
    name starts with that prefix."""

    def __enter__(self):
        L.load().m1_debug_kernels(1)
        self.names = []
        return self

    def __exit__(self, *exc):
        raw = L.load().m1_debug_kernels(0)
        self.names = [n for n in (raw.decode() if raw else "").split(",") if n]
        return False

    def ran(self, prefix: str) -> bool:
        return any(n == prefix or n.startswith(prefix + ":") for n in self.names)


class plan_log:
    """``with ops.plan_log() as pl: ...; pl.entries`` -- what the weight-gradient launchers, the fold and the ladder decided inside the
    block (m1_debug_plans), e.g. ['wg:wgrad_tf tiles=150 want=64 splits=64 fit=512 rx=1 stages=8 grid=4,64,1',
    'fold:generic copies=64 n=9248 nb=32 el=32 queued', 'foldbatch:n=1 blocks=289'].  ``pl.of('fold:')``: the entries with that prefix."""

    def __enter__(self):
        L.load().m1_debug_plans(1)
        self.entries = []
        return self

    def __exit__(self, *exc):
        raw = L.load().m1_debug_plans(0)
        self.entries = [n for n in (raw.decode() if raw else "").split(";") if n]
        return False

    def of(self, prefix: str):
        return [n for n in self.entries if n.startswith(prefix)]


def prof_enable(on: bool):
    L.load().m1_prof_enable(1 if on else 0)


def prof_reset():
    L.load().m1_prof_reset()


def prof_read():
    arr = (L.m1_prof_rec_t * 512)()
    n = L.load().m1_prof_read(arr, 512)
    return [dict(name=arr[i].name.decode(), total_ms=arr[i].total_ms, flops=arr[i].flops, bytes=arr[i].bytes,
                 launches=arr[i].launches) for i in range(n)]
