"""Guard bands (tests/guarded.py) around every buffer of the back-projection kernel (csrc/restore.hip) over the geometries of
test_restore.py: whole and short runs of 4 voxels, the 16-byte stores next to the element ones (rows that start off a 16-byte boundary),
blocks that straddle rows, the 4-byte label stores, taps clamped at both ends of the real window -- no byte outside a buffer is
written, exactly the output buffers are allocated, and nothing outside a buffer reaches a result (a guard reads as 0xFF bytes: NaN in
fp32, -1 in int16)."""
import numpy as np
import pytest
import torch

from guarded import guarded
from util import PKG, ops
from test_restore import CHANNELS, DEFAULT, DEFLABEL, GPU_GEOMS, RANGES, case, check_linear, device_geom, host, lab_like

P = PKG.preprocess
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("Cn", CHANNELS)
def test_linear_restore_stays_inside_its_buffers(dev, monkeypatch, Cn):
    with guarded(monkeypatch, dev) as g:
        for gi, geo in enumerate(GPU_GEOMS):
            pred, ref, e32, inside = case(gi, Cn)
            pd, geom = g.put(torch.from_numpy(pred)), device_geom(geo)
            for c0, nsel in RANGES[Cn]:
                got = ops.restore(pd, geom, c0, nsel)
                assert g.count == 1                                                    # the output: no workspace
                check_linear(got, ref[..., c0:c0 + nsel], e32, inside, (geo, Cn, c0, nsel))
                g.check()
            prob, lab = ops.restore(pd, geom, 0, Cn, True, True)
            assert g.count == 2                                                        # both outputs
            check_linear(prob, ref, e32, inside, (geo, Cn, "both"))
            assert np.array_equal(lab.cpu().numpy(), np.where(inside, np.argmax(prob.cpu().numpy(), axis=-1), DEFLABEL)), (geo, Cn)
            g.check()
            only = ops.restore(pd, geom, prob=False, label=True)
            assert g.count == 1 and torch.equal(only, lab)
            g.check()
            # the public entry point: the same single allocation per output
            shape, sp, osp, _ = geo
            pub, plab = P.restore(pd, shape, sp, osp, channels=Cn - 1, labels=True, default_value=DEFAULT, default_label=DEFLABEL)
            assert g.count == 2 and torch.equal(plab, lab)
            check_linear(pub, ref[..., Cn - 1:], e32, inside, (geo, Cn, "public"))
            g.check()


@pytest.mark.parametrize("in_dtype", (np.float32, np.int16, np.int32))
@pytest.mark.parametrize("Cn", CHANNELS)
def test_nearest_restore_stays_inside_its_buffers(dev, monkeypatch, Cn, in_dtype):
    with guarded(monkeypatch, dev) as g:
        for gi, geo in enumerate(GPU_GEOMS):
            lab = lab_like((2, *geo[3], Cn), 23 + gi + Cn, in_dtype)
            want = host(lab, geo, order=0, default_value=5)
            ld, geom = g.put(torch.from_numpy(lab)), device_geom(geo, 0, 5)
            for c0, nsel in RANGES[Cn]:
                got = ops.restore(ld, geom, c0, nsel)
                assert g.count == 1
                assert np.array_equal(got.cpu().numpy(), want[..., c0:c0 + nsel]), (geo, Cn, c0, nsel)
                g.check()
            got, lb = ops.restore(ld, geom, 0, Cn, True, True)
            assert g.count == 2 and np.array_equal(got.cpu().numpy(), want)
            inside = P.restore_inside(P.restore_geometry(*geo))
            assert np.array_equal(lb.cpu().numpy(), np.where(inside, np.argmax(want, axis=-1), DEFLABEL)), (geo, Cn)
            g.check()
