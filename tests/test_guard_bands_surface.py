"""Guard bands (tests/guarded.py) around every tensor and workspace of the surface-distance kernels (csrc/surface.hip) at the small
shapes: volumes of a few voxels, degenerate axes, rows of 65 and of 256 voxels, chunks that end inside a row.  No byte outside a
buffer is written, and nothing outside one reaches a result: a guard reads as 0xFF bytes, which is the label 255 / -1, a set border
voxel and the distance NaN -- a neighbour fetched across a volume's end would change a border mask, a NaN would become a maximum.
With the inputs of tests/test_surface_distance_edges.py also where a buffer is sized by a kernel constant: lines of up to 256 voxels
along H and D, 40 slices (a second block of the per-slice kernels) and 18 metric blocks with a ragged last chunk."""
import numpy as np
import pytest
import torch

import test_surface_distance_edges as E
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


@pytest.mark.parametrize("shape", E.LONG_SHAPES)
def test_long_lines_stay_inside_their_buffers(dev, monkeypatch, shape):
    """Lines of up to SD_MAX_LINE = 256 voxels staged in LDS along H and D, several SD_CH = 64 chunks per line, a last column tile
    with fewer than SD_TC = 16 columns: the uint16 and fp64 intermediates and the distances, against the brute force."""
    with guarded(monkeypatch, dev) as g:
        mask = g.put(torch.tensor(E.distance_stack("long", shape)))
        for spacing in E.DT_SPACINGS:
            dist = ops.sd_distance(mask, spacing)
            assert g.count == 2                                                # the workspace and the distances
            E.assert_distances(dist.cpu().numpy(), "long", shape, spacing)
            g.check()


def test_forty_slices_stay_inside_their_buffers(dev, monkeypatch):
    """S = 40: the second 64-thread block of the per-slice kernels (80 and 40 threads in use) writes rows 32..39 and no further."""
    with guarded(monkeypatch, dev) as g:
        pred, truth = (g.put(torch.tensor(v)) for v in E.s40_maps())
        got = SD.surface_metrics(pred, truth, E.S40_LABELS, E.S40_SPACING, E.S40_Q, E.S40_TOLERANCES)
        assert g.count == 7
        E.assert_s40(to_host(got))
        g.check()


@pytest.mark.parametrize("family", ("any_normal", "descending"))
def test_a_ragged_last_chunk_stays_inside_its_buffers(dev, monkeypatch, family):
    """n = 34817: 18 blocks of 1935 voxels, the last with 1922; a guard reads as a set border voxel with the distance NaN."""
    case = E.metrics_case((1, 1, 34817), family)
    with guarded(monkeypatch, dev) as g:
        borders, dist = g.put(torch.tensor(case.borders)), g.put(torch.tensor(case.dist))
        for q, tol in ((37.5, case.tolerances), (100.0, ())):
            m = ops.sd_metrics(borders, dist, None, q, tol)
            assert g.count == 2                                                # the workspace and the rows
            host = ops._sd_rows_dict(m["rows"].cpu(), len(tol))
            E.check_metrics({k: v.numpy().reshape((E.MT_S,) + tuple(v.shape[2:])) for k, v in host.items() if k != "rows"}, case, q, tol,
                            (family, q))
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
