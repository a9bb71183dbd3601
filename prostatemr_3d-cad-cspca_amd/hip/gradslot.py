"""Data gradients of tensors with several consumers: one shared gradient buffer per tensor (``fanout``) and per batch tail of such
a tensor (``batch_tail``), written and accumulated by the consumers' backward kernels."""
import os as _os

import torch

from .streams import _BRANCH


class _GradSlot:
    """The one gradient buffer of a tensor that feeds several layers (an SE block's input feeds conv1 and conv4,
    network_blocks.py:53,64; an encoder output also feeds its attention gate, networks.py:584-590).  The first backward
    kernel to produce a gradient for the tensor allocates the buffer, the following ones ACCUMULATE into it in their own
    epilogue (m1_conv3d_dgrad / m1_convT3d_dgrad ``accumulate``, m1_mul_sigma_bwd ``accumulate_dx``): the per-consumer
    gradient tensors and autograd's add passes over them disappear."""
    __slots__ = ("buf", "event", "stream", "tail_init")

    def __init__(self):
        self.buf = None
        self.event = None      # recorded after the last kernel that wrote ``buf`` (only when branches run on side streams)
        self.stream = None
        self.tail_init = False # the region of ``buf`` behind a batch_tail() holds gradient sums already


class _TailRef:
    """Gradient slot of ``x[start:]`` for an ``x`` that has a slot (batch_tail): the reader's backward kernel writes the tail
    region of x's own gradient buffer."""
    __slots__ = ("slot", "start", "full_shape")

    def __init__(self, slot, start, full_shape):
        self.slot, self.start, self.full_shape = slot, int(start), tuple(full_shape)


def _slot_of(t: torch.Tensor):
    ref = getattr(t, "_m1_gslot_tail", None)
    return ref if ref is not None else getattr(t, "_m1_gslot", None)


def _wait_last_writer(slot, buf) -> None:
    """The current stream waits for the last kernel that wrote ``buf`` of ``slot`` when that ran on another stream (a gate branch,
    the posterior lane) and takes a share in the buffer, which belongs to the stream of its first writer (see streams._req)."""
    if slot.event is not None and slot.stream != torch.cuda.current_stream():
        torch.cuda.current_stream().wait_event(slot.event)
        buf.record_stream(torch.cuda.current_stream())


def _slot_target(slot, like: torch.Tensor):
    """(gradient tensor, accumulate flag) for a data gradient shaped like ``like``."""
    if slot is None:
        return torch.empty_like(like), 0
    if isinstance(slot, _TailRef):
        ref, slot = slot, slot.slot
        b = slot.buf
        if b is None or tuple(b.shape) != ref.full_shape or b.dtype != like.dtype:
            if b is not None:
                return torch.empty_like(like), 0          # (a buffer of another shape owns the slot: plain gradient tensor)
            b = torch.empty(ref.full_shape, dtype=like.dtype, device=like.device)
            b[:ref.start].zero_()                         # nobody has written the head of the batch yet
            slot.buf, slot.tail_init = b, False
        else:
            _wait_last_writer(slot, b)
        view = b[ref.start:]
        if tuple(view.shape) != tuple(like.shape) or not view.is_contiguous():
            return torch.empty_like(like), 0
        acc = 1 if slot.tail_init else 0
        slot.tail_init = True
        return view, acc
    b = slot.buf
    if b is not None and b.shape == like.shape and b.dtype == like.dtype and b.is_contiguous():
        _wait_last_writer(slot, b)
        return b, 1
    g = torch.empty_like(like)
    if b is None:
        slot.buf, slot.tail_init = g, True               # (written whole by this kernel)
    return g, 0


def _slot_written(slot) -> None:
    """Call after enqueueing the kernel that wrote / accumulated into ``slot.buf`` (orders readers on other streams)."""
    if isinstance(slot, _TailRef):
        slot = slot.slot
    if slot is not None and _BRANCH["on"]:
        ev = torch.cuda.Event()
        ev.record()
        slot.event, slot.stream = ev, torch.cuda.current_stream()


def _sum_shares(buf, gs):
    """The summed gradient of a fanned-out tensor: ``buf`` (the slot buffer, or None) plus the shares that are not ``buf`` itself."""
    rest = None
    for g in gs:
        if g is None or (buf is not None and g.data_ptr() == buf.data_ptr() and g.shape == buf.shape):
            continue                      # nothing, or the slot buffer itself (already holds that consumer's share)
        if buf is not None:
            buf.add_(g)                   # a consumer that does not accumulate in its kernel: fold it into the slot
        else:
            rest = g if rest is None else rest + g
    return buf if buf is not None else rest


class _Fanout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k, slot, owner):
        ctx.slot, ctx.owner = slot, owner
        ctx.set_materialize_grads(False)
        return tuple(x.view_as(x) for _ in range(k))

    @staticmethod
    def backward(ctx, *gs):
        slot = ctx.slot
        if isinstance(slot, _TailRef):
            # aliases of a batch_tail() output: the consumers wrote (and summed) their shares straight into the tail of the parent
            # tensor's gradient buffer; hand that view on -- _BatchTail.backward recognises it and no slice backward runs
            ref, slot = slot, slot.slot
            full = slot.buf
            buf = None
            if full is not None and tuple(full.shape) == ref.full_shape and slot.tail_init:
                _wait_last_writer(slot, full)
                buf = full[ref.start:]
        else:
            buf = slot.buf
            if buf is not None:
                # the last share may have been added on another stream than this node's: the readers of the summed gradient are
                # ordered behind THIS node by autograd, so it must wait for that write itself
                _wait_last_writer(slot, buf)
            if ctx.owner:
                slot.buf, slot.tail_init = None, False
        return _sum_shares(buf, gs), None, None, None


def fanout(x: torch.Tensor, k: int):
    """``k`` aliases of ``x``, one per consumer.  Their backward kernels sum the gradient of ``x`` in one shared buffer (see
    _GradSlot); consumers without an accumulating kernel still work (their gradient is added here).  Each alias must be
    used by exactly one consumer.  Nested use (a module forks an alias it was handed) shares the outer buffer."""
    if k <= 1 or not torch.is_grad_enabled() or not x.requires_grad:
        return (x,) * k
    tref = getattr(x, "_m1_gslot_tail", None)
    if tref is not None:
        # x is the batch slice of a tensor with a shared gradient buffer (batch_tail): its consumers accumulate into the TAIL of that
        # buffer (a gate forks the slice for its theta conv and the sigma product -- without this the fork opened a buffer of its own
        # and autograd's slice backward added a zero-filled full-size tensor: a fill, a copy and an add over a res1 skip tensor)
        outs = _Fanout.apply(x, k, tref, False)
        for o in outs:
            o._m1_gslot_tail = tref
        return outs
    slot = getattr(x, "_m1_gslot", None)
    owner = slot is None
    if owner:
        slot = _GradSlot()
    outs = _Fanout.apply(x, k, slot, owner)
    for o in outs:
        o._m1_gslot = slot
    return outs


class _BatchTail(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, start, slot):
        ctx.slot, ctx.start, ctx.full_shape = slot, int(start), tuple(x.shape)
        ctx.set_materialize_grads(False)
        return x[int(start):]

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None
        buf = ctx.slot.buf
        if buf is not None and tuple(buf.shape) == ctx.full_shape and g.dtype == buf.dtype:
            tail = buf[ctx.start:]
            if g.data_ptr() == tail.data_ptr() and tuple(g.shape) == tuple(tail.shape):
                return buf, None, None                # the reader wrote straight into x's gradient buffer (_TailRef)
        full = g.new_zeros(ctx.full_shape)
        full[ctx.start:] = g
        return full, None, None


def batch_tail(x: torch.Tensor, start: int) -> torch.Tensor:
    """``x[start:]`` along the batch axis for a reader that runs on the second of two stacked passes (M1Core.forward
    ``tail_from``).  When ``x`` is a fanout alias the reader's backward kernel writes the tail of x's own gradient buffer:
    autograd's slice backward (a zero-filled full-size tensor, a copy into it and an add into the buffer -- 4.5 passes over the
    res0 / res1 skip tensors) disappears."""
    slot = getattr(x, "_m1_gslot", None)
    if slot is None or not torch.is_grad_enabled() or not x.requires_grad or _os.environ.get("M1_TAIL_SLOT", "1") == "0":
        return x[int(start):]
    y = _BatchTail.apply(x, int(start), slot)
    y._m1_gslot_tail = _TailRef(slot, start, x.shape)
    return y
