"""Guard bands (tests/guarded.py) around every tensor and workspace of the surface-distance kernels (csrc/surface.hip) at the small
shapes: volumes of a few voxels, degenerate axes, rows of 65 and of 256 voxels, chunks that end inside a row.  No byte outside a
buffer is written, and nothing outside one reaches a result: a guard reads as 0xFF bytes, which is the label 255 / -1, a set border
voxel and the distance NaN -- a neighbour fetched across a volume's end would change a border mask, a NaN would become a maximum."""
import numpy as np
import pytest
import torch

from guarded import guarded
from util import PKG, ops
from test_surface_distance import check_stages, host_reference, to_host
from test_surface_distance_host import CASES, LABELS, PERCENTILE, SPACINGS, TOLERANCES, assert_metrics_close, label_maps

SD = PKG.surface_distance
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("in_dtype", (torch.uint8, torch.int32))
def test_every_stage_stays_inside_its_buffers(dev, monkeypatch, in_dtype):
    spacing = SPACINGS[1]
    with guarded(monkeypatch, dev) as g:
        for shape, name in CASES:
            pred, truth = label_maps(shape, name)
            pred_d, truth_d = g.put(torch.tensor(pred), in_dtype), g.put(torch.tensor(truth), in_dtype)
            borders, counts = ops.sd_border(pred_d, truth_d, LABELS)
            assert g.count == 3                                                # the workspace, the masks and the counts
            dist = ops.sd_distance(borders.view(-1, *shape), spacing)
            assert g.count == 5                                                # the workspace and the distances
            ops.sd_metrics(borders, dist.view(borders.shape), counts, PERCENTILE, TOLERANCES)
            assert g.count == 7                                                # the workspace and the rows
            check_stages(pred_d, truth_d, shape, name, spacing, (shape, name, str(in_dtype)))
            g.check()


def test_guard_labels_are_not_counted(dev, monkeypatch):
    """255 is what a guard byte reads as in a uint8 map, -1 in an int32 one: asked for as a class, it stays empty."""
    with guarded(monkeypatch, dev) as g:
        for shape in ((3, 5, 7), (1, 1, 9), (4, 1, 1), (2, 3, 65)):
            pred, truth = label_maps(shape, "random0.35")
            for dtype, ghost in ((torch.uint8, 255), (torch.int32, -1)):
                got = SD.surface_metrics(g.put(torch.tensor(pred), dtype), g.put(torch.tensor(truth), dtype), LABELS + (ghost,),
                                         SPACINGS[2], PERCENTILE, TOLERANCES)
                got = to_host(got)
                want = host_reference(shape, "random0.35", SPACINGS[2])[2]
                assert_metrics_close({k: v[:, :2] for k, v in got.items()}, want, (shape, str(dtype)))
                assert all(np.all(got[k][:, 2] == 0) for k in ("n_pred", "n_truth", "vol_pred", "vol_truth", "vol_both"))
                assert np.isnan(got["hd"][:, 2]).all() and np.all(got["nsd"][:, 2] == 1.0)
                g.check()
