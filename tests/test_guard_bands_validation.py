"""Guard bands (tests/guarded.py) around every buffer of the validation scoring kernel (csrc/validate.hip: m1_val_score): p, y and the
entropy of exactly B * voxels (* K) elements, a workspace of exactly m1_val_score_ws bytes and the records of exactly B * 320 bytes.
(2,3,5,7,2) has 105 voxels per case -- odd, so a case starts off the 16-byte grid and the loads are narrow; (1,4,32,32,3) walks three
floats per voxel.  No byte outside a buffer is written, and nothing outside a buffer reaches a record (a guard reads as 0xFF bytes: NaN
in fp32, 255 in uint8 -- either would show in the sums, which are compared with the fp64 restatement)."""
import pytest
import torch

from guarded import guarded
from util import PKG, ops

pytestmark = pytest.mark.gpu
V = PKG.validation
ALPHA = {2: (0.25, 0.75), 3: (0.75, 0.25, 0.5)}


@pytest.fixture
def g(dev, monkeypatch):
    with guarded(monkeypatch, dev) as g_:
        yield g_


@pytest.mark.parametrize("ydt", [torch.uint8, torch.float32])
@pytest.mark.parametrize("shape", [(2, 3, 5, 7, 2), (1, 4, 32, 32, 3), (2, 2, 4, 8, 2)])
def test_val_score_under_guards(g, shape, ydt):
    B, K = shape[0], shape[-1]
    gen = torch.Generator().manual_seed(7)
    p = torch.softmax(2.0 * torch.randn(shape, generator=gen), dim=-1)
    y = torch.nn.functional.one_hot(torch.randint(0, K, shape[:-1], generator=gen), K).to(ydt)
    ent = -(p * torch.log(p)).sum(dim=-1)
    ref = V.score_host(p.numpy(), y.numpy(), ent.numpy(), ALPHA[K], 2.0)
    pd, yd, ed = g.put(p), g.put(y), g.put(ent)
    nws = ops.val_score_ws(B, p.numel() // (B * K), K)
    ws = g.put(torch.zeros(nws, dtype=torch.uint8))
    assert ws.numel() == nws == 8 * 40 * B * (4 if K == 3 else 1)              # (4,32,32) voxels of three floats: four blocks
    with torch.no_grad():
        rec = ops.val_score(pd, yd, ed, ALPHA[K], 2.0, ws=ws)
    assert g.count == 1 and rec.numel() * rec.element_size() == 320 * B         # the records are the one allocation of the call
    got = ops.read_val_records(rec, K)
    assert g.check() == 5
    n = ref[0]["n_voxels"]
    for a, b in zip(got, ref):
        for k in ("n_voxels", "n_fg", "n_pred", "n_true", "n_both", "p_max"):
            assert a[k] == b[k], k
        for k in ("sum_p", "sum_y", "sum_py"):
            assert all(abs(u - v) <= n * 2.0 ** -53 * abs(v) for u, v in zip(a[k], b[k])), k
        for k in ("entropy_sum", "entropy_fg_sum"):
            assert abs(a[k] - b[k]) <= n * 2.0 ** -53 * abs(b[k]), k
        assert abs(a["focal"] - b["focal"]) < 1e-5 * max(1.0, abs(b["focal"]))
