"""Guard bands (tests/guarded.py) around every buffer of the mirror kernels (csrc/mc.hip: m1_tta_views, m1_mc_accum_v): the input and
the stacked views of the copy; the logits, the three accumulators and the per-draw output of the accumulate, each of exactly its element
count.  (2,3,5,7,nc) is odd in every extent: the element path, a mirrored coordinate next to every face of the volume, and samples that
start off the 16-byte grid; (1,4,32,32,3) reads whole groups, with a W mirror from the far end of a row (W - G - w).  A mirrored
index that left the volume would read a guard -- 0xFF bytes, NaN in fp32 and bf16 -- which the NaN-keeping maps would show, or write
one, which ``check`` shows; the maps are compared with the fp64 restatement of the logits flipped back on the host."""
import numpy as np
import pytest
import torch

from guarded import guarded
from util import ops
from test_mc_inference import as_np
import mc_uncertainty_ref as Rf

pytestmark = pytest.mark.gpu


@pytest.fixture
def g(dev, monkeypatch):
    with guarded(monkeypatch, dev) as g_:
        yield g_


def _flip(t, mask):
    dims = [ax for bit, ax in ((1, 3), (2, 2), (4, 1)) if mask & bit]
    return torch.flip(t, dims) if dims else t


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=lambda v: str(v).replace("torch.", ""))
@pytest.mark.parametrize("shape", [(2, 3, 5, 7, 2), (2, 3, 5, 7, 3), (2, 3, 5, 7, 4), (1, 4, 32, 32, 3)], ids=str)
def test_both_ops_under_guards(g, shape, dtype):
    B, nc = shape[0], shape[-1]
    V = int(np.prod(shape[1:-1]))
    gen = np.random.default_rng(23)
    for R, views in ((1, (7,)), (3, (5, 0, 3)), (3, (6, 7, 1))):
        # pass 1: R * B logits of their own; pass 2: one batch of logits stacked into its R views by tta_views
        first = torch.from_numpy(np.clip(gen.standard_normal((R * B, *shape[1:])) * 2.5, -6, 6).astype(np.float32)).to(dtype)
        base = torch.from_numpy(np.clip(gen.standard_normal(shape) * 2.5, -6, 6).astype(np.float32)).to(dtype)
        flat = [torch.cat([_flip(first[r * B:(r + 1) * B], views[r]) for r in range(R)]), base.repeat(R, 1, 1, 1, 1)]
        with np.errstate(all="ignore"):
            _, _, m64, e32 = Rf.case_refs_u([as_np(t).reshape(R * B, V, nc) for t in flat], R)
        with torch.no_grad():
            acc = ops.mc_accum_v(g.put(first), R, views, uncertainty=True)          # the op's own three allocations
            assert g.count == 3 and [t.numel() for t in acc] == [B * V * nc, B * V, B * V * nc]
            stacked = ops.tta_views(g.put(base), views)
            assert g.count == 4 and stacked.numel() == R * B * V * nc and stacked.dtype == dtype
            acc, draws = ops.mc_accum_v(stacked, R, views, acc, samples=True, uncertainty=True)
            assert g.count == 5 and draws.numel() == R * B * V * nc
            plain = ops.mc_accum_v(stacked, R, views)                                # without the uncertainty sums: one
            assert g.count == 6 and plain.numel() == B * V * nc
            maps = ops.mc_finish_u(acc, 2 * R)
            assert g.count == 8
        assert g.check() == 10
        assert bool(torch.isfinite(draws).all()) and bool(torch.isfinite(plain).all())
        for k, v in maps.items():
            got = as_np(v).reshape(m64[k].shape).astype(np.float64)
            assert np.isfinite(got).all(), k
            assert float(np.abs(got - m64[k]).max()) <= Rf.bound(nc, 2 * R, k, e32[k]), k
