"""Guard bands (tests/guarded.py) around every buffer of the calibration kernel (csrc/calibrate.hip: m1_cal_score): p of exactly
B * voxels * K elements, label / mask of B * voxels bytes, the uncertainty of B * voxels floats and the records of exactly
B * (8 + 3 * bins * (K + 2)) * 8 bytes.  105 voxels per case is odd -- the cases after the first start off the 16-byte grid, the loads
are narrow and a scalar tail runs; 257 with one case takes the wide loads and a tail of one.  No byte outside a buffer is written, and
nothing outside a buffer reaches a record: a guard reads as 0xFF bytes -- NaN in fp32 and bf16, label 255, mask 255 -- and any of them
would show in n_invalid / n_ignored / the counts, which are compared with the per-voxel loop of tests/cal_ref.py."""
import pytest
import torch

import cal_ref
from guarded import guarded
from util import ops

pytestmark = pytest.mark.gpu
M = 15


@pytest.fixture
def g(dev, monkeypatch):
    with guarded(monkeypatch, dev) as g_:
        yield g_


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("mask,unc", [(False, False), (True, True)])
@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("B,V", [(2, 105), (1, 257), (2, 257)])
def test_cal_score_under_guards(g, B, V, K, mask, unc, bf16):
    c = cal_ref.case(B, V, K, "random", mask=mask, unc=unc, bf16=bf16)
    ref = cal_ref.record(c["p"], c["label"], M, c["mask"], c["unc"], c["u_max"])
    put = lambda a, dt=None: None if a is None else g.put(torch.from_numpy(a), dt)        # noqa: E731
    pd, yd, md, ud = put(c["p"], torch.bfloat16 if bf16 else None), put(c["label"]), put(c["mask"]), put(c["unc"])
    with torch.no_grad():
        rec = ops.cal_score(pd, yd, M, md, ud, c["u_max"])
    slots = 8 + 3 * M * (K + 2)
    assert g.count == 1 and rec.numel() * rec.element_size() == 8 * slots * B == 8 * B * ops.cal_record_slots(K, M)
    got = ops.read_cal_records(rec, K, M)
    assert g.check() == 3 + int(mask) + int(unc)
    for b in range(B):
        assert cal_ref.same(ref[b], got[b], skip=("nll",)) == [], b
        assert abs(int(got[b]["nll"]) - int(ref[b]["nll"])) <= ref[b]["n_valid"]            # (the device's fp64 log: one unit per voxel)
        kept = V if c["mask"] is None else int((c["mask"][b] != 0).sum())
        assert got[b]["n_valid"] + got[b]["n_invalid"] + got[b]["n_ignored"] == kept
