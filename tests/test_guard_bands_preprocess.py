"""Guard bands (tests/guarded.py) around every buffer of the preprocessing kernels (csrc/preprocess.hip) at the odd geometries: the
vector loads and stores next to the element ones, pads wider than the axis, windows that read the first and the last source element,
the per-block histograms and partials in the workspace -- no byte outside a buffer is written, and nothing outside one reaches a
result (a guard reads as 0xFF bytes: NaN in fp32, -1 in int16, which would show in the gathered values and in the statistics)."""
import numpy as np
import pytest
import torch

from guarded import guarded
from util import PKG, ops
from test_preprocess import GEOMS, MODES, K_CLIP, K_PLAIN, U, as_bits, scan_like

P = PKG.preprocess
pytestmark = pytest.mark.gpu
# the geometries of the gather test, one whose window is the whole source, and slices of more than one block (n > 2048)
CASES = GEOMS + [((2, 3, 8), (2, 3, 8), (0, 0, 0)), ((3, 33, 33), (3, 33, 36), (0, 0, -2)), ((2, 40, 33), (3, 33, 33), (-1, 7, 0))]


@pytest.mark.parametrize("in_dtype", (np.float32, np.int16))
@pytest.mark.parametrize("Cn", (1, 3, 4))
def test_crop_pad_stays_inside_its_buffers(dev, monkeypatch, Cn, in_dtype):
    with guarded(monkeypatch, dev) as g:
        for src, dst, start in CASES:
            raw = scan_like((2, *src, Cn), 7 + Cn, in_dtype)
            for mode in MODES:
                want = torch.from_numpy(np.stack([P.crop_pad_host(raw[b], dst, start, mode, 3.0) for b in range(2)]).astype(np.float32))
                for dtype in (torch.float32, torch.bfloat16):
                    got = ops.crop_pad(g.put(torch.from_numpy(raw)), dst, start, mode, 3.0, dtype)
                    assert g.count == 1                                                # the output came from the guarded allocator
                    assert torch.equal(as_bits(got.cpu()), as_bits(want.to(dtype))), (src, dst, start, mode, dtype)
                    g.check()


@pytest.mark.parametrize("in_dtype", (np.float32, np.int16))
def test_order_stats_stay_inside_their_buffers(dev, monkeypatch, in_dtype):
    with guarded(monkeypatch, dev) as g:
        for src, dst, start in CASES:
            n = dst[0] * dst[1] * dst[2]
            for Cn, mode in ((1, "constant"), (3, "symmetric"), (4, "reflect")):
                raw = scan_like((2, *src, Cn), 9 + Cn, in_dtype)
                sl = np.stack([[np.sort(P.crop_pad_host(raw[b, ..., c], dst, start, mode, -2.0).astype(np.float32), axis=None)
                                for c in range(Cn)] for b in range(2)])
                ranks = (0, n - 1, n // 2, P.percentile_rank(99.5, n)[0])
                pairs, values = ops.order_stats(g.put(torch.from_numpy(raw)), dst, start, ranks, (0.0, 0.0, 0.5, 0.25), mode, -2.0)
                assert g.count == 3                                                    # pairs, values, workspace
                for j, k in enumerate(ranks):
                    want = sl[:, :, [k, min(k + 1, n - 1)]]
                    assert np.array_equal(pairs[:, :, j].cpu().numpy().view(np.uint32), want.view(np.uint32)), (src, dst, start, mode, j)
                assert bool(torch.isfinite(values).all())
                g.check()


@pytest.mark.parametrize("in_dtype", (np.float32, np.int16))
def test_whiten_stays_inside_its_buffers(dev, monkeypatch, in_dtype):
    with guarded(monkeypatch, dev) as g:
        for src, dst, start in CASES:
            n = dst[0] * dst[1] * dst[2]
            for Cn, mode in ((1, "edge"), (3, "constant"), (4, "symmetric")):
                raw = scan_like((2, *src, Cn), 13 + Cn, in_dtype)
                vols = [[P.crop_pad_host(raw[b, ..., c], dst, start, mode, 5.0) for c in range(Cn)] for b in range(2)]
                for p in (None, 99.0):
                    ref = np.stack([np.stack([P.whitening_host(v, p, np.float64) for v in row], axis=-1) for row in vols])
                    e32 = max(float(np.abs(P.whitening_host(v, p, np.float32) - ref[b, ..., c]).max())
                              for b, row in enumerate(vols) for c, v in enumerate(row))
                    rd, bounds = g.put(torch.from_numpy(raw)), None
                    if p is not None:
                        (k0, w0), (k1, w1) = P.percentile_rank(100 - p, n), P.percentile_rank(p, n)
                        bounds = ops.order_stats(rd, dst, start, (k0, k1), (w0, w1), mode, 5.0)[1]
                        assert g.count == 3
                        g.check()                                                      # (bounds stays alive: it is read below)
                    out, stats = ops.whiten(rd, dst, start, mode, 5.0, bounds, torch.float32)
                    assert g.count == 3                                                # out, stats, workspace
                    got = out.cpu().numpy().astype(np.float64)
                    bound = max((K_PLAIN if p is None else K_CLIP) * U * float(np.abs(ref).max()), 4 * e32)
                    assert np.isfinite(got).all() and float(np.abs(got - ref).max()) <= bound, (src, dst, start, mode, p)
                    assert bool(torch.isfinite(stats).all())
                    g.check()
