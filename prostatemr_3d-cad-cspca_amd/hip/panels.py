"""Conv workspaces and the cache of packed weight panels: kept on the weight tensor while it is unchanged, registered so that one
launch re-packs all of them after an optimiser step."""
import ctypes as C
import weakref

import torch

from . import lib as L
from .streams import _p, _stream


def _conv_ws(d, transposed: bool, role: int, device, zero: bool = False) -> torch.Tensor:
    n = L.load().m1_conv_ws_bytes(C.byref(d), 1 if transposed else 0, role)
    return (torch.zeros if zero else torch.empty)(max(int(n), 256), dtype=torch.uint8, device=device)


# Packed weight panels are kept ON the weight tensor object, per (version, role, geometry), while the weights are
# unchanged, so that the second pass of a core within one train step (prior and posterior each run twice,
# networks.py:348-352) skips the pack.  Living on the tensor object they die with it (no address-reuse aliasing).
_PANEL_EPOCH = [0]


# Every cached panel is also REGISTERED: (id(weight), key) -> (weakref(weight), data_ptr, workspace, [device addresses of
# its pack-job records]).  repack_all() refreshes all of them with one m1_pack_batch launch after an optimiser step.
_PACK_REG: dict = {}
_PACK_TABLE = [None]      # device int64 tensor of job-record addresses (rebuilt when the registry changes)

# A repack_all() recorded into a graph reads ITS table through raw addresses at every replay, and re-packs the panels that table
# lists, no others.  The table therefore stays alive for the life of the process (a few kB per capture), and the weights it covers
# are frozen (``_m1_frozen`` = the panel epoch of the capture): a geometry such a weight first meets AFTER the capture -- an
# evaluation at another batch size between replays -- is packed at every call and neither cached nor registered, because no replay
# would refresh it and the next call would be served a panel of the weights before the update.
_CAPTURED_TABLES: list = []


def _frozen(holder: torch.Tensor) -> bool:
    return getattr(holder, "_m1_frozen", None) == _PANEL_EPOCH[0]


def invalidate_panels() -> None:
    """Call after anything that changes weights through raw pointers without re-packing (e.g. load_weights)."""
    _PANEL_EPOCH[0] += 1
    _PACK_REG.clear()
    _PACK_TABLE[0] = None


def repack_all() -> None:
    """Re-pack every registered weight panel from the current weight values (one kernel launch).  The fused optimiser
    calls this after its update, so the next step's convolutions find their panels already packed."""
    dead = [k for k, (r, ptr, _, _) in _PACK_REG.items() if r() is None or r().data_ptr() != ptr]
    for k in dead:
        del _PACK_REG[k]
        _PACK_TABLE[0] = None
    if not _PACK_REG:
        return
    if _PACK_TABLE[0] is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("weight-panel registry changed during graph capture: run one eager step first")
        ws0 = next(iter(_PACK_REG.values()))[2]
        ptrs, blocks = [], [0]
        for (r, _, _, jobs) in _PACK_REG.values():
            per = max(1, int(r().numel()) // max(1, len(jobs)))          # weights per job (a dgrad panel per concat member)
            for j in jobs:
                ptrs.append(j)
                blocks.append(blocks[-1] + min(512, max(1, -(-per // 16384))))   # ~8 segments of 8 weights per thread
        _PACK_TABLE[0] = (torch.tensor(ptrs, dtype=torch.int64).to(ws0.device),
                          torch.tensor(blocks, dtype=torch.int32).to(ws0.device), blocks[-1])
    t, pref, total = _PACK_TABLE[0]
    if torch.cuda.is_current_stream_capturing() and not any(c is _PACK_TABLE[0] for c in _CAPTURED_TABLES):
        _CAPTURED_TABLES.append(_PACK_TABLE[0])
        for (r, _, _, _) in _PACK_REG.values():
            r()._m1_frozen = _PANEL_EPOCH[0]
    L.check(L.load().m1_pack_batch(_p(t), _p(pref), int(t.numel()), int(total), _stream()), "m1_pack_batch")


def _lookup(holder: torch.Tensor, attr: str, weights, prefix, d, transposed: bool, role: int, need_mask):
    """(workspace, packed) of the panel built from ``weights``, cached in attribute ``attr`` of ``holder`` while no (_version,
    data_ptr) of ``weights`` changes; ``prefix`` opens the key."""
    if not all(w.is_leaf for w in weights):   # a derived weight (e.g. the zero-padded stem kernel): packed per call, never registered
        return _conv_ws(d, transposed, role, holder.device, zero=True), 0
    store = getattr(holder, attr, None)
    stamp = (_PANEL_EPOCH[0], *(v for w in weights for v in (w._version, w.data_ptr())))
    if store is None or store[0] != stamp:
        store = (stamp, {})
        try:
            setattr(holder, attr, store)
        except Exception:  # noqa: BLE001 -- an object that cannot carry attributes: no caching
            return _conv_ws(d, transposed, role, holder.device), 0
    key = (*prefix, role, transposed, d.N, d.D, d.H, d.W, d.kd, d.kh, d.kw, d.sd, d.sh, d.sw, d.dtype,
           tuple(d.src[i].C for i in range(d.nsrc)), need_mask)
    hit = store[1].get(key)
    if hit is not None:
        return hit, 1
    if _frozen(holder):                       # a captured repack_all covers this weight, but not this geometry: packed per call
        return _conv_ws(d, transposed, role, holder.device, zero=True), 0
    ws = _conv_ws(d, transposed, role, holder.device, zero=True)     # zero: unfilled job records must read as empty
    store[1][key] = ws
    out = (C.c_void_p * L.M1_MAX_SRC)()
    n = L.load().m1_conv_pack_jobs(C.byref(d), 1 if transposed else 0, role, _p(ws), out)
    if n > 0:
        _PACK_REG[(id(holder), key)] = (weakref.ref(holder), holder.data_ptr(), ws, [int(out[i]) for i in range(n)])
        _PACK_TABLE[0] = None
    return ws, 0


def _panel_ws(w: torch.Tensor, d, transposed: bool, role: int, need_mask=None):
    return _lookup(w, "_m1_panels", (w,), (), d, transposed, role, need_mask)


def _pair_panel_ws(w1: torch.Tensor, w4: torch.Tensor, d, role: int, need_mask=None):
    """Packed panel of the conv1 || conv4 pair (built from BOTH weight tensors), cached on w4 while neither changes."""
    return _lookup(w4, "_m1_pair_panels", (w1, w4), ("pair", int(w1.shape[-1])), d, False, role, need_mask)
