"""Guard bands (tests/guarded.py) around every buffer of the resampling kernels (csrc/resample.hip) at the odd geometries: the staged
LDS tile's vector loads next to the element ones, short and full last tiles, lines on both sides of the closed-form / truncated causal
start and of the LDS / workspace switch, the two intermediate volumes in the workspace, windows -- no byte outside a buffer is written,
and nothing outside one reaches a result (a guard reads as 0xFF bytes: NaN in fp32, -1 in int16; through the recursion a NaN read as
data would spread over its whole line)."""
import numpy as np
import pytest
import torch

from guarded import guarded
from util import PKG, ops
from test_preprocess import scan_like
from test_resample import GEOMS, KERNEL, SMALL, steps_of

P = PKG.preprocess
pytestmark = pytest.mark.gpu
# (B, geometry).  B = 1 with 63 and 65 rows: one below and one above RS_ROWS = 64, the rows of an LDS tile (w = 9: the pitch allows 64)
CASES = [(2, g) for g in GEOMS + SMALL + KERNEL[:10]] + [(1, ((7, 9, 9), (3, .5, .5), (3, .4, .7))), (1, ((5, 13, 9), (3, .5, .5), (2.5, .6, .4))),
                                                          (1, KERNEL[10]), (1, KERNEL[11])]


@pytest.mark.parametrize("in_dtype", (np.float32, np.int16))
@pytest.mark.parametrize("Cn", (1, 3, 4))
def test_cubic_resampling_stays_inside_its_buffers(dev, monkeypatch, Cn, in_dtype):
    with guarded(monkeypatch, dev) as g:
        for B, (shape, sp, osp) in CASES:
            raw = scan_like((B, *shape, Cn), 17 + Cn, in_dtype)
            ref = np.stack([P.resample_host(raw[b], sp, osp, default_value=5.0, dtype=np.float64) for b in range(B)])
            e32 = float(np.abs(np.stack([P.resample_host(raw[b], sp, osp, default_value=5.0, dtype=np.float32) for b in range(B)]) - ref).max())
            size = P.resample_size(shape, sp, osp)
            rd = g.put(torch.from_numpy(raw))
            got = ops.resample(rd, steps_of(sp, osp), size, default_value=5.0)
            assert g.count == 2                                                        # the output and the workspace
            got = got.cpu().numpy().astype(np.float64)
            assert np.isfinite(got).all() and (np.abs(got - ref) <= 4 * e32).all(), (B, shape, sp, osp)
            g.check()
            # a window: the last outputs of every axis
            first = [n // 2 for n in size]
            count = [n - f for n, f in zip(size, first)]
            win = ops.resample(rd, steps_of(sp, osp), count, first, default_value=5.0)
            assert g.count == 2
            sl = (slice(None),) + tuple(slice(f, None) for f in first)
            assert (np.abs(win.cpu().numpy().astype(np.float64) - ref[sl]) <= 4 * e32).all(), (B, shape, sp, osp)
            g.check()


@pytest.mark.parametrize("in_dtype", (np.float32, np.int16))
@pytest.mark.parametrize("Cn", (1, 3, 4))
def test_nearest_resampling_stays_inside_its_buffers(dev, monkeypatch, Cn, in_dtype):
    with guarded(monkeypatch, dev) as g:
        for B, (shape, sp, osp) in CASES:
            lab = scan_like((B, *shape, Cn), 19 + Cn, in_dtype)
            want = np.stack([P.resample_host(lab[b], sp, osp, is_label=True, default_value=5) for b in range(B)])
            got = ops.resample(g.put(torch.from_numpy(lab)), steps_of(sp, osp), P.resample_size(shape, sp, osp), order=0, default_value=5)
            assert g.count == 1                                                        # the output: no workspace
            assert np.array_equal(got.cpu().numpy(), want), (B, shape, sp, osp)
            g.check()
