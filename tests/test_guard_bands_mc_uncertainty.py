"""Guard bands (tests/guarded.py) around every buffer of the uncertainty kernels (csrc/mc.hip: m1_mc_accum_u, m1_mc_finish_u): logits,
the three accumulators, the per-draw output and the two maps the finish allocates, each of exactly its element count.  (2,3,5,7,nc) has
105 voxels per sample -- odd, so a sample starts off the 16-byte grid of the bf16 logits, the groups of G leave a tail and with replicas
the loads are narrow; (1,4,32,32,3) walks three floats per voxel in whole groups.  No byte outside a buffer is written, and nothing
outside a buffer reaches a map: a guard reads as 0xFF bytes, NaN in fp32 and bf16, which the NaN-keeping maps would show; they are
compared with the fp64 restatement."""
import itertools

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


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=lambda v: str(v).replace("torch.", ""))
@pytest.mark.parametrize("shape", [(2, 3, 5, 7, 2), (2, 3, 5, 7, 3), (2, 3, 5, 7, 4), (1, 4, 32, 32, 3)], ids=str)
def test_both_ops_under_guards(g, shape, dtype):
    B, nc = shape[0], shape[-1]
    V = int(np.prod(shape[1:-1]))
    gen = np.random.default_rng(17)
    for R in (1, 3):
        passes = [torch.from_numpy(np.clip(gen.standard_normal((R * B, *shape[1:])) * 2.5, -6, 6).astype(np.float32)).to(dtype) for _ in range(2)]
        with np.errstate(all="ignore"):
            _, _, m64, e32 = Rf.case_refs_u([as_np(t).reshape(R * B, V, nc) for t in passes], R)
        with torch.no_grad():
            acc = ops.mc_accum_u(g.put(passes[0]), R)                            # the op's own three allocations
            assert g.count == 3 and [t.numel() for t in acc] == [B * V * nc, B * V, B * V * nc]
            acc, draws = ops.mc_accum_u(g.put(passes[1]), R, acc, samples=True)
            assert g.count == 4 and draws.numel() == R * B * V * nc
            maps = ops.mc_finish_u(acc, 2 * R)
            assert g.count == 6                                                  # entropy and mutual_info; the rest over the sums
        assert g.check() == 8
        assert bool(torch.isfinite(draws).all())
        for k, v in maps.items():
            got = as_np(v).reshape(m64[k].shape).astype(np.float64)
            assert np.isfinite(got).all(), k
            assert float(np.abs(got - m64[k]).max()) <= Rf.bound(nc, 2 * R, k, e32[k]), k
