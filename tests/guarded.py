"""Guard bands around device allocations: a kernel that stores or loads a few elements outside one of its buffers lands, in an ordinary
run, in the caching allocator's slack (every block is rounded to 512 B) or in an unrelated tensor, and no parity test sees it.  Inside
``with guarded(monkeypatch) as g:`` every CUDA tensor from torch.empty / empty_like / zeros / zeros_like (the same interception
hip/debug.py uses for M1_DEBUG_POISON) is a view into a larger uint8 buffer

    [ front guard | tensor | back guard ]

with both guards filled with 0xFF bytes (NaN in fp32 and bf16, -1 in the integer types).  The front guard is a multiple of 512 B, so
the tensor keeps the 512-byte alignment of a block of its own; its last byte abuts the back guard (no rounding), so an overrun of one
element is already in the guard.  ``g.check()`` asserts that every guard byte is still 0xFF; a load from a guard shows as NaN in the
results, which the parity assertions of the caller catch.

What this cannot see: a load outside the tensor whose value is masked before use; a store of 0xFF bytes; a store further than one
guard away (it lands in another allocation or faults, and is not attributed)."""
import contextlib
import os
import sys

import torch

# Bytes per guard.  A choice, not a measurement: larger than one row of the widest tile at the shapes of the suite (160 channels x
# 40 voxels x 4 B = 25 KiB), small enough that a few thousand live allocations of a test stay far below a GiB.
GUARD = 64 * 1024
assert GUARD % 512 == 0
_HERE = os.path.abspath(__file__)
_NAMES = ("empty", "empty_like", "zeros", "zeros_like")


def _site(depth=3):
    """A short stack of the caller outside this module: 'file:line fn < file:line fn < ...'."""
    out, f = [], sys._getframe(1)
    while f is not None and len(out) < depth:
        if os.path.abspath(f.f_code.co_filename) != _HERE:
            out.append(f"{os.path.basename(f.f_code.co_filename)}:{f.f_lineno} {f.f_code.co_name}")
        f = f.f_back
    return " < ".join(out)


def _is_cuda(device) -> bool:
    return device is not None and torch.device(device).type == "cuda"


class Guarded:
    def __init__(self, device=None):
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.real = {n: getattr(torch, n) for n in _NAMES}
        self.records = []            # (base, nbytes, shape, dtype, call site) of every allocation since the last check
        self.count = 0               # allocations INTERCEPTED since the last check (torch.empty & co.; what put() places is not counted)

    # ---- allocation -----------------------------------------------------------------------------------------------------------
    def alloc(self, shape, dtype, device, zero: bool, requires_grad: bool = False, intercepted: bool = True) -> torch.Tensor:
        shape = tuple(int(v) for v in shape)
        dtype = torch.get_default_dtype() if dtype is None else dtype
        numel = 1
        for v in shape:
            numel *= v
        nbytes = numel * dtype.itemsize
        if nbytes == 0:                                  # (an empty tensor has no address: nothing to guard)
            return self.real["empty"](shape, dtype=dtype, device=device)
        base = self.real["empty"](GUARD + nbytes + GUARD, dtype=torch.uint8, device=device)
        assert base.data_ptr() % 512 == 0, "the allocator's blocks are 512-byte aligned"
        base.fill_(0xFF)
        inner = base[GUARD:GUARD + nbytes]
        if zero:
            inner.zero_()
        t = inner.view(dtype).view(shape)
        assert t.data_ptr() == base.data_ptr() + GUARD and t.data_ptr() + nbytes == base.data_ptr() + GUARD + nbytes
        self.records.append((base, nbytes, shape, dtype, _site()))
        if intercepted:
            self.count += 1
        return t.requires_grad_(True) if requires_grad else t

    def _new(self, zero, *size, dtype=None, device=None, requires_grad=False, **kw):
        name = "zeros" if zero else "empty"
        if not _is_cuda(device) or kw.get("out") is not None or kw.get("layout", torch.strided) != torch.strided:
            return self.real[name](*size, dtype=dtype, device=device, requires_grad=requires_grad, **kw)
        if len(size) == 1 and not isinstance(size[0], int):
            size = tuple(size[0])
        return self.alloc(size, dtype, device, zero, requires_grad)

    def _like(self, zero, t, dtype=None, device=None, requires_grad=False, **kw):
        name = "zeros_like" if zero else "empty_like"
        device = t.device if device is None else device
        if not _is_cuda(device) or kw.get("layout", torch.strided) != torch.strided:
            return self.real[name](t, dtype=dtype, device=device, requires_grad=requires_grad, **kw)
        return self.alloc(t.shape, t.dtype if dtype is None else dtype, device, zero, requires_grad)

    def empty(self, *size, **kw):
        return self._new(False, *size, **kw)

    def zeros(self, *size, **kw):
        return self._new(True, *size, **kw)

    def empty_like(self, t, **kw):
        return self._like(False, t, **kw)

    def zeros_like(self, t, **kw):
        return self._like(True, t, **kw)

    def put(self, host: torch.Tensor, dtype=None) -> torch.Tensor:
        """A guarded device copy of ``host`` in ``dtype``: inputs, incoming gradients, parameters, statistics, flat gradient sinks.
        Checked like every allocation, but not counted: ``count`` says what the code under test allocated."""
        t = self.alloc(host.shape, host.dtype if dtype is None else dtype, self.device, False, intercepted=False)
        t.copy_(host.detach())
        return t

    # ---- verification ---------------------------------------------------------------------------------------------------------
    def check(self) -> int:
        """Assert that every guard byte of every allocation since the last check is still 0xFF; returns how many were checked.  The
        buffers are kept alive until here (a freed block could be handed out again and overwritten legitimately) and dropped after."""
        torch.cuda.synchronize()
        recs, self.records, self.count = self.records, [], 0
        if not recs:
            return 0
        flags = torch.stack([(b[:GUARD] != 0xFF).any() | (b[GUARD + nb:] != 0xFF).any() for b, nb, _, _, _ in recs]).cpu()
        for bad, (base, nbytes, shape, dtype, site) in zip(flags.tolist(), recs):
            if not bad:
                continue
            esz = dtype.itemsize
            what = []
            front = torch.nonzero(base[:GUARD] != 0xFF).flatten()
            back = torch.nonzero(base[GUARD + nbytes:] != 0xFF).flatten()
            if front.numel():
                what.append(f"{front.numel()} byte(s) changed in FRONT of the tensor, the first at offset {int(front[0]) - GUARD} "
                            f"from its start ({(int(front[0]) - GUARD) / esz:g} elements)")
            if back.numel():
                what.append(f"{back.numel()} byte(s) changed BEHIND the tensor, the first at offset +{int(back[0])} from its end "
                            f"({int(back[0]) / esz:g} elements)")
            nbad = int(flags.sum())
            raise AssertionError(f"guard band of a {shape} {dtype} tensor ({nbytes} bytes) allocated at [{site}] was written: "
                                 + "; ".join(what) + f" ({nbad} of {len(recs)} allocations affected)")
        return len(recs)


@contextlib.contextmanager
def guarded(monkeypatch, device=None):
    """``with guarded(monkeypatch) as g:`` -- torch.empty / empty_like / zeros / zeros_like hand out guarded CUDA tensors inside the
    block; the originals come back through ``monkeypatch`` on exit."""
    g = Guarded(device)
    with monkeypatch.context() as m:
        for n in _NAMES:
            m.setattr(torch, n, getattr(g, n))
        yield g
