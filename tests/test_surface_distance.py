"""The surface-distance kernels (csrc/surface.hip) against the numpy restatements of surface_distance.py, which
tests/test_surface_distance_host.py pins against scipy: the shapes, spacings and label patterns are that module's.

Bounds, derived there and not measured here: border masks and every integer count are identical; a distance map is within 1 fp32 ulp
(the kernels form the same fp64 expression as the restatement: in practice the bits agree); means, percentiles and the hard Dice are
within rtol 2^-22; NaNs sit in the same places; nsd is exact because no distance lies within 4 fp32 ulp of a tolerance -- which also
means that `d <= tolerance` and `d < tolerance` count alike here: that the comparison is inclusive is tested in
tests/test_surface_distance_edges.py (tolerances that are distances of the set), as are the other label sets, percentiles, numbers of
tolerances, line lengths and block counts than the one point (K = 2, q = 95, T = 4, B = 2, D <= 20) of this module."""
import functools
import inspect

import numpy as np
import pytest
import torch

from util import PKG, ops
from test_surface_distance_host import (B, CASES, COUNT_KEYS, FLOAT_KEYS, LABELS, PERCENTILE, SPACINGS, TOLERANCES, assert_clear,
                                        assert_metrics_close, directed_sets, label_maps, ulp_distance)

SD = PKG.surface_distance
L = PKG.hip.lib
pytestmark = pytest.mark.gpu
FULL_SHAPE, FULL_SPACING = (20, 160, 160), (3.0, 0.5, 0.5)


@functools.lru_cache(maxsize=None)
def host_reference(shape, name, spacing):
    """(borders (2,B,K,D,H,W) bool, dist (2,B,K,D,H,W) fp32, metrics) by the numpy restatements; computed once and shared."""
    pred, truth = label_maps(shape, name)
    borders = np.stack([np.stack([SD.mask_border_host(v == l) for l in LABELS], axis=1) for v in (pred, truth)])
    dist = SD.edt_host(borders, spacing)
    for a in (borders, dist):
        a.setflags(write=False)
    return borders, dist, SD.surface_metrics_host(pred, truth, LABELS, spacing, PERCENTILE, TOLERANCES)


def to_host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def check_stages(pred_d, truth_d, shape, name, spacing, what):
    """Each op on its own against the restatement; returns the three device results."""
    want_b, want_d, want_m = host_reference(shape, name, spacing)
    borders, counts = ops.sd_border(pred_d, truth_d, LABELS)
    assert borders.dtype == torch.uint8 and counts.dtype == torch.int64 and borders.is_cuda and counts.is_cuda
    assert np.array_equal(borders.cpu().numpy(), want_b.astype(np.uint8)), what
    for j, key in enumerate(COUNT_KEYS):
        assert np.array_equal(counts[..., j].cpu().numpy(), want_m[key]), (what, key)
    dist = ops.sd_distance(borders.view(-1, *shape), spacing).view(borders.shape)
    assert dist.dtype == torch.float32 and dist.is_cuda
    assert ulp_distance(dist.cpu().numpy(), want_d) <= 1, what
    m = ops.sd_metrics(borders, dist, counts, PERCENTILE, TOLERANCES)
    assert all(v.is_cuda for v in m.values())
    got = to_host(m)
    assert np.array_equal(got["n_ab"], want_m["n_pred"]) and np.array_equal(got["n_ba"], want_m["n_truth"]), what
    got.update({key: want_m[key] for key in COUNT_KEYS})               # (compared above: assert_metrics_close wants the keys)
    assert_metrics_close(got, want_m, what)
    return borders, counts, dist, m


@pytest.mark.parametrize("shape,name", CASES)
def test_every_stage_matches_the_host(dev, shape, name):
    pred, truth = label_maps(shape, name)
    pred_d, truth_d = torch.tensor(pred, device=dev), torch.tensor(truth, device=dev)
    for spacing in SPACINGS:
        check_stages(pred_d, truth_d, shape, name, spacing, (shape, name, spacing))
        got = SD.surface_metrics(pred_d, truth_d, LABELS, spacing, PERCENTILE, TOLERANCES)
        assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in got.values())
        assert got["nsd"].shape == (B, len(LABELS), len(TOLERANCES)) and got["hd"].shape == (B, len(LABELS))
        assert_metrics_close(to_host(got), host_reference(shape, name, spacing)[2], (shape, name, spacing, "surface_metrics"))


@pytest.mark.parametrize("shape,name", [((5, 9, 33), "ellipsoids"), ((2, 3, 65), "random0.35"), ((8, 40, 40), "pred_only")])
def test_dtypes_batch_axis_and_conveniences(dev, shape, name):
    pred, truth = label_maps(shape, name)
    sp = SPACINGS[1]
    p8, t8 = torch.tensor(pred, device=dev), torch.tensor(truth, device=dev)
    p32, t32 = p8.to(torch.int32), t8.to(torch.int32)
    a, b = SD.surface_metrics(p8, t8, LABELS, sp, PERCENTILE, TOLERANCES), SD.surface_metrics(p32, t32, LABELS, sp, PERCENTILE, TOLERANCES)
    for key in a:
        assert torch.equal(a[key].view(torch.int32) if a[key].dtype == torch.float32 else a[key],
                           b[key].view(torch.int32) if b[key].dtype == torch.float32 else b[key]), (key, "uint8 vs int32")
    for i in range(B):
        one = SD.surface_metrics(p8[i], t8[i], LABELS, sp, PERCENTILE, TOLERANCES)
        for key in a:
            assert one[key].shape == a[key].shape[1:]
            assert np.array_equal(one[key].cpu().numpy(), a[key][i].cpu().numpy(), equal_nan=True), (key, i, "(D,H,W) vs (B,D,H,W)")
    want = host_reference(shape, name, sp)[2]
    thin = {"hd": SD.hausdorff(p8, t8, LABELS, sp), "hdq": SD.hausdorff_percentile(p8, t8, LABELS, sp, PERCENTILE),
            "assd": SD.assd(p8, t8, LABELS, sp), "dice": SD.dice_per_class(p8, t8, LABELS)}
    for key, v in thin.items():
        assert np.array_equal(v.cpu().numpy(), a[key].cpu().numpy(), equal_nan=True), key
    assert np.array_equal(SD.nsd(p8, t8, TOLERANCES[1], LABELS, sp).cpu().numpy(), want["nsd"][..., 1], equal_nan=True)
    # a binary mask is the case labels = (1,): its border and its distance map, bool and uint8 alike
    mask = pred == 1
    wb, wd = SD.mask_border_host(mask), SD.distance_to_border_host(mask, sp)
    for m in (torch.tensor(mask, device=dev), torch.tensor(mask.astype(np.uint8), device=dev)):
        assert np.array_equal(SD.mask_border(m).cpu().numpy(), wb.astype(np.uint8))
        assert np.array_equal(SD.mask_border(m[0]).cpu().numpy(), wb[0].astype(np.uint8))
        assert ulp_distance(SD.distance_to_border(m, sp).cpu().numpy(), wd) <= 1
        assert ulp_distance(SD.distance_to_border(m[1], sp).cpu().numpy(), wd[1]) <= 1


def test_two_calls_give_identical_bits(dev):
    """The fixed-order sums: every output of every stage, twice, on the dense random labelling (the most border voxels per block)."""
    for shape in ((8, 40, 40), (2, 3, 256)):
        pred, truth = label_maps(shape, "random0.35")
        pred_d, truth_d = torch.tensor(pred, device=dev), torch.tensor(truth, device=dev)
        runs = []
        for _ in range(2):
            borders, counts = ops.sd_border(pred_d, truth_d, LABELS)
            dist = ops.sd_distance(borders.view(-1, *shape), SPACINGS[2]).view(borders.shape)
            rows = ops.sd_metrics(borders, dist, counts, PERCENTILE, TOLERANCES)["rows"]
            runs.append((borders, counts, dist.view(torch.int32), rows))
        for x, y in zip(*runs):
            assert torch.equal(x, y), shape


def test_nothing_is_read_back():
    """Device tensors in, device tensors out (asserted where the results are made above), and no op of the path reads one."""
    for fn in (ops.sd_workspace, ops.sd_border, ops.sd_distance, ops.sd_metrics, ops._sd_rows_dict, ops._sd_ws, SD.surface_metrics,
               SD._device_maps):
        src = inspect.getsource(fn)
        for word in (".item(", ".cpu(", ".tolist(", ".numpy(", "synchronize"):
            assert word not in src, (fn.__name__, word)


def test_refusals(dev):
    lib = L.load()
    x = torch.zeros((1, 2, 3, 257), dtype=torch.uint8, device=dev)
    for shape in ((1, 257, 3, 2), (1, 2, 257, 3), (1, 2, 3, 257)):
        m = x.view(shape)
        with pytest.raises(RuntimeError, match="M1_ERR_UNSUPPORTED"):
            ops.sd_distance(m)
        with pytest.raises(RuntimeError, match="M1_ERR_UNSUPPORTED"):
            SD.surface_metrics(m, m)
    m = torch.zeros((1, 3, 5, 7), dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="M1_ERR_BAD_ARG"):
        ops.sd_distance(m, (1.0, 0.0, 1.0))
    with pytest.raises(RuntimeError):
        ops.sd_border(m, m, ())
    with pytest.raises(RuntimeError):
        ops.sd_border(m, m, tuple(range(9)))
    with pytest.raises(RuntimeError):
        ops.sd_border(m, m.to(torch.int32))
    with pytest.raises(RuntimeError):
        ops.sd_border(m.float(), m.float())
    borders, counts = ops.sd_border(m, m)
    dist = ops.sd_distance(borders.view(-1, 3, 5, 7)).view(borders.shape)
    with pytest.raises(RuntimeError):
        ops.sd_metrics(borders, dist, counts, tolerances=(1.0,) * 5)
    with pytest.raises(RuntimeError, match="M1_ERR_BAD_ARG"):
        ops.sd_metrics(borders, dist, counts, percentile=-1.0)
    with pytest.raises(RuntimeError, match="M1_ERR_BAD_ARG"):
        ops.sd_metrics(borders, dist, counts, tolerances=(float("nan"),))
    ws = torch.empty(4, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="workspace"):
        ops.sd_metrics(borders, dist, counts, ws=ws)
    assert lib.m1_sd_metrics(borders.data_ptr(), dist.data_ptr(), None, 1, 1, 3, 5, 7, 95.0, None, 0, None, ws.data_ptr(), None) == -1


def test_full_size_ellipsoids(dev):
    """The one full-size case: (2,20,160,160), K = 2, spacing (3.0, 0.5, 0.5), against the host restatement."""
    pred, truth = label_maps(FULL_SHAPE, "ellipsoids")
    for b in range(B):
        for l in LABELS:
            for d in directed_sets(pred[b], truth[b], l, FULL_SPACING)[:2]:
                assert_clear(d, TOLERANCES, ("full size", b, l))
    pred_d, truth_d = torch.tensor(pred, device=dev), torch.tensor(truth, device=dev)
    check_stages(pred_d, truth_d, FULL_SHAPE, "ellipsoids", FULL_SPACING, "full size")
