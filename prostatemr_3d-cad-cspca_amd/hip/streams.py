"""Scheduling of a step on the host: independent branches on side streams, their joins, the queues of deferred weight gradients and
of their folds, and what a gradient exchange (ddp.GradReducer) needs to know about all of them."""
import ctypes as C
import os as _os
from typing import Optional

import torch

from . import lib as L
from .debug import _POISON

# ---------------------------------------------------------------------------------------------------------
# independent branches on side streams
# ---------------------------------------------------------------------------------------------------------
_BRANCH = {"on": _os.environ.get("M1_STREAMS", "1") != "0", "streams": {}, "used": set(), "depth": 0}


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream():
    s = torch.cuda.current_stream().cuda_stream
    if _POISON >= 2:
        L.load().m1_debug_scribble(0, 8, s)
    return s


def _side_stream():
    """The current stream when it is a branch stream of the running step, else False."""
    if not _BRANCH["on"]:
        return False
    origin = _BRANCH.get("origin")
    if origin is None:
        return False
    cur = torch.cuda.current_stream()
    return cur if cur != origin else False


def _req(*ts):
    side = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("M1 HIP ops need tensors on a GPU (cuda/HIP) device: the HIP extension is the only "
                               "compute path of this package; there is no CPU fallback")
        if not t.is_contiguous():
            raise RuntimeError("M1 HIP ops need contiguous NDHWC tensors")
        # An op running on a branch stream (ops.branch: SE shortcut, attention gates, the posterior lane) reads tensors that were
        # allocated on the stream the step started on.  The caching allocator hands a freed block back to its OWN stream at once: the
        # moment autograd drops such a tensor (its last backward node has been enqueued, not executed) a later allocation of the main
        # stream could overwrite it under the branch's kernel.  Eager launches rarely lose that race; a replayed hipGraph, whose
        # branches run with no host pacing, did (round 4: gradients of the deep levels off by 10-40 % in 2 of 5 runs of the captured
        # probabilistic step).  record_stream ties the block to the branch stream as well (no-op for blocks of that stream).
        if side is None:
            side = _side_stream()
        if side:
            t.record_stream(side)


class branch:
    """``with ops.branch(device, k) as br: y = f(x)`` then ``br.join(y)``: runs an independent part of the step (the conv4
    shortcut of an SE block next to its conv1-conv2-conv3 chain; the attention gates next to the decoder) on side stream
    ``k``; autograd runs the backward of these ops on the same stream, so both directions overlap, inside a captured graph
    as well (fork/join become graph dependencies).  Most kernels of the deep levels fill a fraction of the 256 CUs: measured
    -8 % per C2 train step (SE shortcuts + gates), -4 % on the full probabilistic model.  M1_STREAMS=0 runs everything in order.
    Tensors handed to the branch must stay referenced until ``join`` (they are read on the side stream)."""

    def __init__(self, device, k: int = 0):
        # a branch opened INSIDE another branch runs in line on its parent's stream: forks of forks segfault the HIP graph
        # capture of this ROCm release (and every fork then starts from the capture's origin stream)
        self.on = _BRANCH["on"] and device.type == "cuda" and _BRANCH["depth"] == 0
        if self.on:
            _BRANCH["origin"] = torch.cuda.current_stream(device)          # (depth 0: the stream the step runs on)
            key = (device, k)
            if key not in _BRANCH["streams"]:
                _BRANCH["streams"][key] = torch.cuda.Stream(device=device)
            self.side = _BRANCH["streams"][key]
            self.cur = torch.cuda.current_stream(device)
            self.ctx = torch.cuda.stream(self.side)

    def __enter__(self):
        if self.on:
            self.side.wait_stream(self.cur)
            _BRANCH["used"].add(self.side)
            self.ctx.__enter__()
            _BRANCH["depth"] += 1
        return self

    def __exit__(self, *exc):
        if self.on:
            _BRANCH["depth"] -= 1
            self.ctx.__exit__(*exc)
        return False

    def join(self, *tensors):
        """Make the current stream wait for the branch; ``tensors``: its results that the current stream will read."""
        if self.on:
            self.cur.wait_stream(self.side)
            for t in tensors:
                if t is not None:
                    t.record_stream(self.cur)


# ---------------------------------------------------------------------------------------------------------
# weight gradients: the fold queue and the deferred launches
# ---------------------------------------------------------------------------------------------------------
# Deferred folds of the weight-gradient partial copies (m1_wgrad_defer): with gradients going to the flat buffer nothing reads a
# weight gradient before join_side_streams, so the ~130 fold launches of a step (5-10 us each, a few dozen blocks, alone on
# their stream) become a handful of batched ones there.  The workspaces holding the copies are kept until then.
_FOLD = {"on": _os.environ.get("M1_WG_FOLD_BATCH", "1") != "0", "keep": [],
         # M1_FOLD_ASYNC = n > 0 (default 24, one batched launch): every n queued weight gradients the folds queued so far run on
         # a stream of their own NEXT TO the backward pass (bandwidth-bound folds beside MFMA-bound convolutions) instead of
         # all at its end, where they ran alone on the GPU (0.8 ms of the C3 step)
         "async": int(_os.environ.get("M1_FOLD_ASYNC", "-1")), "stream": None,
         "async_mb": int(_os.environ.get("M1_FOLD_ASYNC_MB", "0")), "bytes": 0}


# Deferred weight gradients of the deep levels (round 6).  A weight gradient feeds nothing before the optimiser, and the skip test of
# round 6 showed that the replayed step is the SUM of its kernels -- except for what runs on the fold stream, which rides for free next
# to the data-gradient chain.  Weight gradients are therefore not launched where autograd calls them: they are queued (operands kept
# alive) and launched, in call order, on the fold stream with the next batch of folds -- no fork / join per op (weight gradients on
# streams of their own WITH a fork and a join each were measured slower in rounds 2, 3 and 6).  M1_WG_DEFER_VOX limits this to layers
# with at most that many input voxels per launch (0 = launch in place, round 5).  Same box, C3: in place 22.76 ms, <= 16,000 voxels
# 22.6, <= 520,000 22.29, all 22.00 ms (90.9 volumes/s) at a batch interval of 11-13 (M1_FOLD_ASYNC; 8: 23.6, 16: 22.8, 24: 22.8);
# profiles/r06_ab_deferred_weight_gradients.txt.
_WGP = {"maxvox": int(_os.environ.get("M1_WG_DEFER_VOX", str(1 << 40)) or 0), "jobs": [], "extra": []}


def submit_wgrad(fn, d, dy, wbuf, bbuf, ws, acc_w, transposed: bool, srcs, st, flat: bool) -> None:
    """The weight (+ bias) gradient ``fn`` of one conv, on the caller's stream ``st`` or through the queues.  ``flat``: both gradients
    go to the optimiser's flat buffer, so the folds of the per-split partial copies are queued (m1_wgrad_defer) and run in batches."""
    if not (flat and _FOLD["on"]):
        L.check(fn(C.byref(d), _p(dy), _p(wbuf), _p(bbuf), _p(ws), acc_w, st), "m1_conv3d_wgrad")
        return
    lib = L.load()
    cur_ = torch.cuda.current_stream(ws.device)
    if (_WGP["maxvox"] > 0 and _BRANCH["on"] and _BRANCH.get("origin") is not None and
            int(d.N) * int(d.D) * int(d.H) * int(d.W) <= _WGP["maxvox"]):
        # queued: launched on the fold stream with the next batch (operands referenced until then, see _run_deferred_wgrads)
        _WGP["jobs"].append((fn, d, dy, wbuf, bbuf, ws, acc_w, tuple(srcs)))
        _WGP["extra"].extend((t, cur_) for t in (dy, *srcs))
    else:
        lib.m1_wgrad_defer(1)
        try:
            L.check(fn(C.byref(d), _p(dy), _p(wbuf), _p(bbuf), _p(ws), acc_w, st), "m1_conv3d_wgrad")
        finally:
            lib.m1_wgrad_defer(0)
    _FOLD["keep"].append((ws, cur_))
    if transposed and bbuf is not None:
        # the bias gradient of a transposed conv is queued with the folds (norm.hip: m1_colsum_defer): d(out) is read at the fold
        _FOLD["keep"].append((dy, cur_))
    _FOLD["bytes"] += ws.numel() * ws.element_size()
    if _BRANCH["on"] and ((_FOLD["async"] > 0 and len(_FOLD["keep"]) >= _FOLD["async"]) or
                          (_FOLD["async_mb"] > 0 and _FOLD["bytes"] >= _FOLD["async_mb"] << 20)):
        _fold_async()


def _run_deferred_wgrads(stream_handle, stream) -> None:
    """Launch the queued weight gradients (in call order) on ``stream``; the caller has ordered it behind their operands."""
    jobs, _WGP["jobs"] = _WGP["jobs"], []
    if not jobs:
        return
    lib = L.load()
    lib.m1_wgrad_defer(1)
    try:
        for fn, d, dy, wbuf, bbuf, ws, acc_w, _srcs in jobs:
            L.check(fn(C.byref(d), _p(dy), _p(wbuf), _p(bbuf), _p(ws), acc_w, stream_handle), "m1_conv3d_wgrad (deferred)")
    finally:
        lib.m1_wgrad_defer(0)
    for t, made_on in _WGP["extra"]:
        if made_on != stream:
            t.record_stream(stream)
    _WGP["extra"] = []


def fold_async_default(n: int) -> None:
    """Model-level default of the M1_FOLD_ASYNC interval (the environment variable wins).  Measured optimum, same box: 10-12 for
    the hierarchical probabilistic model (~130 weight gradients per step: 26.7 ms against 27.3 at 24, 27.7 without, 27.6-27.9
    at <= 8), 24 for the deterministic one (~60 per step: 7.87 ms against 8.01 at 12, 7.94 without)."""
    if "M1_FOLD_ASYNC" not in _os.environ:
        _FOLD["async"] = int(n)


def _fold_here() -> None:
    """The queued weight gradients, then the queued folds, on the current stream; the kept workspaces are released to it."""
    cur = torch.cuda.current_stream()
    try:
        _run_deferred_wgrads(_stream(), cur)
        L.check(L.load().m1_wgrad_fold_pending(_stream()), "m1_wgrad_fold_pending")
        for ws, made_on in _FOLD["keep"]:
            if made_on != cur:
                ws.record_stream(cur)                 # read here, allocated on another (a branch) stream
    finally:
        _FOLD["keep"].clear(); _FOLD["bytes"] = 0


def _fold_async() -> None:
    """Run the queued folds on the fold stream, ordered behind everything enqueued so far.  Only from the stream the step started
    on (a fork of a fork breaks graph capture, see ``branch``): weight gradients of branch streams wait for the next trigger."""
    origin = _BRANCH.get("origin")
    cur = torch.cuda.current_stream()
    if origin is None or cur != origin or not _FOLD["keep"]:
        return
    fs = _FOLD["stream"]
    if fs is None:
        fs = _FOLD["stream"] = torch.cuda.Stream(device=cur.device)
    fs.wait_stream(cur)                                   # (first: the fold stream joins a capture through its origin)
    for s in _BRANCH["used"]:
        if s != cur and s != fs:
            fs.wait_stream(s)
    _BRANCH["used"].add(fs)
    with torch.cuda.stream(fs):
        _fold_here()


def fold_pending() -> None:
    """Run the queued weight-gradient folds on the current stream (which must be ordered behind the weight-gradient kernels)."""
    if _FOLD["keep"]:
        _fold_here()


def fold_drop() -> None:
    _WGP["jobs"], _WGP["extra"] = [], []
    if _FOLD["keep"]:
        L.load().m1_wgrad_fold_drop()
        _FOLD["keep"].clear(); _FOLD["bytes"] = 0


# ---------------------------------------------------------------------------------------------------------
# joins, and what a gradient exchange during backward needs
# ---------------------------------------------------------------------------------------------------------
def join_side_streams() -> None:
    """The current stream waits for every side stream used since the last call.  Backward kernels that only add into
    parameter-gradient sinks return nothing to autograd, so the engine never orders them before the caller: gather_grads /
    zero_grad do it here (inside a capture this is also what rejoins the forked streams)."""
    if _BRANCH["used"]:
        cur = torch.cuda.current_stream()
        for s in _BRANCH["used"]:
            if s != cur:
                cur.wait_stream(s)
        _BRANCH["used"].clear()
    fold_pending()


def finish_queued_for_exchange() -> None:
    """Before a gradient group is exchanged during backward (ddp.GradReducer): the current stream waits for the branch streams
    (without retiring them) and runs the weight-gradient folds queued so far."""
    if _FOLD["keep"]:
        cur = torch.cuda.current_stream()
        # a hook that fires on a lane (the posterior pass runs its backward on a side stream, networks.py M1_PQ_LANES) must also
        # wait for the ORIGIN stream: the queue holds the prior's partial copies too, whose weight-gradient kernels are in flight
        # there (``used`` only lists side streams)
        origin = _BRANCH.get("origin")
        if origin is not None and origin != cur:
            cur.wait_stream(origin)
        for s in _BRANCH["used"]:
            if s != cur:
                cur.wait_stream(s)
        fold_pending()


def on_origin_stream() -> bool:
    """True unless the current stream is a branch stream of the running step (autograd runs a branch's backward nodes on it)."""
    origin = _BRANCH.get("origin")
    return origin is None or not torch.cuda.is_available() or torch.cuda.current_stream() == origin


def exchange_streams():
    """Streams that may hold backward kernels of the running step, the origin stream FIRST (a communication stream must join a
    graph capture through the stream the capture started on before it takes edges from forked streams), for ddp.GradReducer."""
    origin = _BRANCH.get("origin")
    out = [origin] if origin is not None else []
    return out + [s for s in _BRANCH["used"] if s is not origin]
