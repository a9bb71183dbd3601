"""Guard bands (tests/guarded.py) around every buffer of the guarded optimiser step (csrc/optim.hip: m1_grad_norm, m1_adam_amsgrad_ctl,
m1_step_advance_ctl): buffers of exactly n floats with n % 4 in {0, 1, 2, 3} (the float4 body next to the scalar tail), a workspace of
exactly m1_grad_norm_ws(n) bytes, a control record of exactly 16 bytes.  No byte outside a buffer is written, the entry points allocate
nothing, and nothing outside a buffer reaches a result (a guard reads as 0xFF bytes: NaN in fp32 -- it would make the norm NaN and,
with the guard on, skip the step)."""
import numpy as np
import pytest
import torch

import clip_ref
from guarded import guarded
from util import ops, rel_err, rnd

pytestmark = pytest.mark.gpu
LK, LB, GS, LR, EPS = 1e-2, 3e-2, 0.5, 1e-2, 1e-7
B1, B2 = float(np.float32(0.9)), float(np.float32(0.999))


@pytest.fixture
def g(dev, monkeypatch):
    with guarded(monkeypatch, dev) as g_:
        yield g_


def _buffers(g, n, seed):
    p0, gr = rnd((n,), seed), rnd((n,), seed + 1)
    pd, gd = g.put(p0), g.put(gr)
    m, v, vh = (g.put(torch.zeros(n)) for _ in range(3))
    lr_dev, step = g.put(torch.tensor([LR])), g.put(torch.ones(1, dtype=torch.int32))
    nws = ops.grad_norm_ws(n)
    ws = g.put(torch.zeros(nws, dtype=torch.uint8))
    ctl = g.put(torch.zeros(4, dtype=torch.int32))
    assert ws.numel() == nws and ctl.numel() * ctl.element_size() == 16
    return p0, gr, pd, gd, m, v, vh, lr_dev, step, ws, ctl


# 1016 floats is the first size with two blocks (two partials in a 16-byte workspace); 262,147 has 257 of them: the control pass's
# threads 0 and 1 read a second partial, the last one at the workspace's end
@pytest.mark.parametrize("l2", [True, False])
@pytest.mark.parametrize("n", [1, 3, 5, 1000, 1001, 1002, 1003, 1016, 1019, 262_147])
def test_guarded_step_under_guards(g, n, l2):
    nk, nb = (n * 2 // 5) | 1, n // 5 + 1
    lk, lb = (LK, LB) if l2 else (0.0, 0.0)
    p0, gr, pd, gd, m, v, vh, lr_dev, step, ws, ctl = _buffers(g, n, 1)
    r = [p0.double()] + [torch.zeros(n, dtype=torch.float64) for _ in range(3)]
    cv = 0.7
    cn = 0.5 * float((clip_ref.clamp_value(clip_ref.regularised_grad(r[0], gr.double(), nk, nb, lk, lb, GS), cv) ** 2).sum().sqrt())
    t = 1
    for _ in range(3):
        ops.grad_norm_(gd, pd, nk, nb, lk, lb, GS, cv, cn, True, ws, ctl)
        ops.adam_amsgrad_ctl_(pd, gd, m, v, vh, nk, nb, lk, lb, GS, lr_dev, B1, B2, EPS, step, cv, ctl)
        ops.step_advance_ctl(step, ctl)
        *r, t, info = clip_ref.guarded_step(r[0], gr.double(), *r[1:], t, nk, nb, lk, lb, GS, LR, B1, B2, EPS, cv, cn, True)
    torch.cuda.synchronize()
    assert g.count == 0 and g.check() == 9                   # (in place: the entry points allocate nothing; nine placed buffers)
    rec = ops.read_step_ctl(ctl)
    assert rec["apply"] == 1 and rec["skipped"] == 0 and int(step) == 4 and torch.equal(gd.cpu(), gr)
    assert abs(rec["norm"] - info["norm"]) <= 1e-5 * info["norm"]          # (third step, weights of two earlier steps: p's own bound)
    assert rec["coef"] < 1 and rel_err(pd, r[0]) < 1e-5


@pytest.mark.parametrize("n", [3, 1001, 1016])
def test_skipped_step_under_guards(g, n):
    """A NaN in the last element (the scalar tail, or the last lane of the last float4): the record says skip, nothing else is written."""
    nk, nb = (n * 2 // 5) | 1, n // 5 + 1
    p0, gr, pd, gd, m, v, vh, lr_dev, step, ws, ctl = _buffers(g, n, 3)
    gd[n - 1] = float("nan")
    ops.grad_norm_(gd, pd, nk, nb, LK, LB, GS, 0.0, 1.0, True, ws, ctl)
    ops.adam_amsgrad_ctl_(pd, gd, m, v, vh, nk, nb, LK, LB, GS, lr_dev, B1, B2, EPS, step, 0.0, ctl)
    ops.step_advance_ctl(step, ctl)
    torch.cuda.synchronize()
    assert g.count == 0 and g.check() == 9
    rec = ops.read_step_ctl(ctl)
    assert rec["apply"] == 0 and rec["skipped"] == 1 and np.isnan(rec["norm"]) and int(step) == 1
    assert torch.equal(pd.cpu(), p0) and not m.any() and not v.any() and not vh.any()
