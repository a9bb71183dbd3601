"""surface_distance.py's numpy restatements against the scipy pipeline the module docstring names: borders by
``scipy.ndimage.binary_erosion`` (6-neighbourhood, border_value=0), distances by ``distance_transform_edt(~border, sampling=spacing)``,
percentiles by ``np.percentile`` (linear).  Borders and counts are exact.  Distances and metrics are held to rtol 2^-22, derived, not
measured: the fp64 separable minimum of (s * delta)^2 sums differs from scipy's fp64 value by a few fp64 ulp (each is a handful of
correctly rounded fp64 operations on the same integers and spacings), hence by at most 1 fp32 ulp (2^-23 relative) after the one
rounding to fp32; a mean or a percentile interpolation of such values adds one more fp32 rounding: 2 * 2^-23.

The shapes, spacings and label patterns here are shared with the device tests (tests/test_surface_distance.py and
tests/test_guard_bands_surface.py), which compare the kernels with the restatements.  Runs anywhere: no GPU."""
import ctypes
import functools

import numpy as np
import pytest
from scipy import ndimage

from util import PKG

SD = PKG.surface_distance
L = PKG.hip.lib

B = 2
LABELS = (1, 2)
SHAPES = ((3, 5, 7), (5, 9, 33), (2, 3, 65), (8, 40, 40), (1, 1, 9), (4, 1, 1), (2, 3, 256))
SPACINGS = ((1.0, 1.0, 1.0), (3.0, 0.5, 0.5), (3.6, 0.3, 0.3))
PATTERNS = ("ellipsoids", "random0.35", "full", "single", "pred_only", "absent")
RTOL = 2.0 ** -22
PERCENTILE = 95.0
TOLERANCES = (0.4, 1.1, 2.3, 5.9)            # mm; test_tolerances_are_clear_of_every_distance holds them away from every distance
FLOAT_KEYS = SD.FLOAT_KEYS
COUNT_KEYS = SD.COUNT_KEYS


# ---- label patterns -----------------------------------------------------------------------------------------------------------
def _ellipsoid(shape, centre, radii):
    g = np.ogrid[tuple(slice(0, n) for n in shape)]
    return sum(((a - c) / max(r, 0.6)) ** 2 for a, c, r in zip(g, centre, radii)) <= 1.0


def _ellipsoid_pair(shape, b):
    """Two shifted ellipsoids per class: class 1 with a hole in ``pred``, class 2 touching the last z face of the volume."""
    D, H, W = shape
    out = []
    for shift in ((0, 0, 0), (0, 1, 2 + b)):
        lab = np.zeros(shape, np.uint8)
        c2 = (D - 1 - shift[0], 0.7 * H - shift[1], 0.72 * W - shift[2] + b)
        lab[_ellipsoid(shape, c2, (0.3 * D, 0.2 * H, 0.2 * W))] = 2
        c1 = (0.35 * D + shift[0], 0.4 * H + shift[1] + b, 0.35 * W + shift[2])
        lab[_ellipsoid(shape, c1, (0.3 * D, 0.3 * H, 0.25 * W))] = 1
        out.append(lab)
    hole = _ellipsoid(shape, (0.35 * D, 0.4 * H + b, 0.35 * W), (0.1 * D, 0.1 * H, 0.08 * W))
    out[0][hole & (out[0] == 1)] = 0
    return out


@functools.lru_cache(maxsize=None)
def label_maps(shape, name):
    """(pred, truth): uint8 (B,D,H,W) label maps in {0, 1, 2}, read-only, different content per batch entry."""
    rng = np.random.default_rng(sum(shape) * 131 + len(name))
    pred, truth = np.zeros((B,) + shape, np.uint8), np.zeros((B,) + shape, np.uint8)
    n = int(np.prod(shape))
    for b in range(B):
        if name == "ellipsoids":
            pred[b], truth[b] = _ellipsoid_pair(shape, b)
        elif name == "random0.35":
            pred[b] = rng.choice(3, size=shape, p=(0.3, 0.35, 0.35))
            truth[b] = rng.choice(3, size=shape, p=(0.3, 0.35, 0.35))
        elif name == "full":                              # the whole volume one class; the other class is in neither map
            pred[b] = truth[b] = 1 + b
        elif name == "single":                            # one voxel each, at different places; n = 1 in both directed sets
            pred[b].reshape(-1)[(3 + 5 * b) % n] = 1
            truth[b].reshape(-1)[(n - 1 - b) % n] = 1
        elif name == "pred_only":                         # class 1 (entry 1: class 2) in pred only; the other class in both
            pred[b], truth[b] = _ellipsoid_pair(shape, b)
            truth[b][truth[b] == 1 + b] = 0
        elif name != "absent":
            raise KeyError(name)
    pred.setflags(write=False)
    truth.setflags(write=False)
    return pred, truth


# ---- the oracle ---------------------------------------------------------------------------------------------------------------
STRUCT = ndimage.generate_binary_structure(3, 1)


def scipy_border(m):
    return m & ~ndimage.binary_erosion(m, STRUCT, border_value=0)


def scipy_dist(border, spacing):
    return ndimage.distance_transform_edt(~border, sampling=spacing).astype(np.float32)


def directed_sets(pred, truth, label, spacing):
    """(d_AB, d_BA, counts) of one volume and class by scipy; the sets are None when A or B is empty."""
    a, b = pred == label, truth == label
    ba, bb = scipy_border(a), scipy_border(b)
    counts = (int(ba.sum()), int(bb.sum()), int(a.sum()), int(b.sum()), int((a & b).sum()))
    if not a.any() or not b.any():
        return None, None, counts
    return scipy_dist(bb, spacing)[ba], scipy_dist(ba, spacing)[bb], counts


@functools.lru_cache(maxsize=None)
def oracle(shape, name, spacing, q=PERCENTILE, tol=TOLERANCES):
    pred, truth = label_maps(shape, name)
    K, T = len(LABELS), len(tol)
    out = {k: np.zeros((B, K), np.int64) for k in COUNT_KEYS}
    out.update({k: np.full((B, K), np.nan, np.float64) for k in FLOAT_KEYS})
    out["nsd"] = np.full((B, K, T), np.nan, np.float64)
    for b in range(B):
        for k, l in enumerate(LABELS):
            d_ab, d_ba, counts = directed_sets(pred[b], truth[b], l, spacing)
            for key, v in zip(COUNT_KEYS, counts):
                out[key][b, k] = v
            if counts[2] + counts[3] > 0:
                out["dice"][b, k] = 2.0 * counts[4] / (counts[2] + counts[3])
            if counts[2] == 0 and counts[3] == 0:
                out["nsd"][b, k] = 1.0
            if d_ab is None:
                continue
            d_ab, d_ba = d_ab.astype(np.float64), d_ba.astype(np.float64)
            pooled = np.concatenate([d_ab, d_ba])
            out["hd_ab"][b, k], out["hd_ba"][b, k], out["hd"][b, k] = d_ab.max(), d_ba.max(), pooled.max()
            out["mean_ab"][b, k], out["mean_ba"][b, k] = d_ab.mean(), d_ba.mean()
            out["assd"][b, k] = (d_ab.mean() + d_ba.mean()) / 2
            out["hdq_ab"][b, k], out["hdq_ba"][b, k] = np.percentile(d_ab, q), np.percentile(d_ba, q)
            out["hdq"][b, k] = np.percentile(pooled, q)
            for t, tau in enumerate(tol):
                out["nsd"][b, k, t] = (pooled.astype(np.float32) <= np.float32(tau)).sum() / pooled.size
    return out


def ulp_distance(a, b):
    """Largest distance in fp32 ulps between two arrays of non-negative fp32 values (+inf allowed; equal infinities are 0 apart)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape and not np.isnan(a).any() and not np.isnan(b).any()
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max()) if a.size else 0


def assert_metrics_close(got, want, what, exact_nsd=True, rtol=RTOL):
    """Counts identical, NaNs in the same places, floats within ``rtol``, nsd exact (tolerances clear of every distance)."""
    for key in COUNT_KEYS:
        assert np.array_equal(np.asarray(got[key]), want[key]), (what, key, got[key], want[key])
    for key in FLOAT_KEYS + ("nsd",):
        g, w = np.asarray(got[key], np.float64), np.asarray(want[key], np.float64)
        assert g.shape == w.shape, (what, key, g.shape, w.shape)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, key, g, w)
        ok = ~np.isnan(w)
        if key == "nsd" and exact_nsd:
            assert np.array_equal(g[ok].astype(np.float32), w[ok].astype(np.float32)), (what, key, g, w)
        else:
            assert np.all(np.abs(g[ok] - w[ok]) <= rtol * np.abs(w[ok])), (what, key, g, w)


CASES = [(s, p) for s in SHAPES for p in PATTERNS]


# ---- tests --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,name", CASES)
def test_borders_and_counts_equal_scipy(shape, name):
    pred, truth = label_maps(shape, name)
    for vol in (pred, truth):
        for l in LABELS:
            want = np.stack([scipy_border(v == l) for v in vol])
            assert np.array_equal(SD.mask_border_host((vol == l).astype(np.uint8)), want), (shape, name, l)
            assert np.array_equal(SD.mask_border_host(vol[0] == l), want[0])
    got = SD.surface_metrics_host(pred, truth, LABELS)
    want = oracle(shape, name, SPACINGS[0])
    for key in COUNT_KEYS:
        assert got[key].dtype == np.int64 and np.array_equal(got[key], want[key]), (shape, name, key)


@pytest.mark.parametrize("shape,name", CASES)
def test_distances_within_one_ulp_of_scipy(shape, name):
    pred, _ = label_maps(shape, name)
    for spacing in SPACINGS:
        for l in LABELS:
            got = SD.distance_to_border_host((pred == l).astype(np.uint8), spacing)
            assert got.dtype == np.float32 and got.shape == pred.shape
            for b in range(B):
                border = scipy_border(pred[b] == l)
                if not border.any():
                    assert np.all(np.isposinf(got[b])), (shape, name, spacing, l)
                    continue
                want = ndimage.distance_transform_edt(~border, sampling=spacing)
                assert np.all(np.abs(got[b].astype(np.float64) - want) <= RTOL * want), (shape, name, spacing, l)
                assert ulp_distance(got[b], want.astype(np.float32)) <= 1, (shape, name, spacing, l)


def test_tolerances_are_clear_of_every_distance():
    """No oracle distance lies within 4 fp32 ulp of a tolerance, so that `d <= tau` cannot depend on the last bit of d."""
    for shape, name in CASES:                               # (the full-size case is checked where it is used: tests/test_surface_distance.py)
        pred, truth = label_maps(shape, name)
        for spacing in SPACINGS:
            for b in range(B):
                for l in LABELS:
                    for d in directed_sets(pred[b], truth[b], l, spacing)[:2]:
                        assert_clear(d, TOLERANCES, (shape, name, spacing))


def assert_clear(d, tolerances, what):
    if d is None or d.size == 0:
        return
    for tau in tolerances:
        tau = np.float32(tau)
        gap = np.abs(d.astype(np.float64) - float(tau)).min()
        assert gap > 4 * float(np.spacing(tau)), (what, tau, gap)


@pytest.mark.parametrize("shape,name", CASES)
def test_metrics_match_the_scipy_pipeline(shape, name):
    pred, truth = label_maps(shape, name)
    for spacing in SPACINGS:
        got = SD.surface_metrics(pred, truth, LABELS, spacing, PERCENTILE, TOLERANCES)
        assert all(isinstance(v, np.ndarray) for v in got.values())
        assert all(got[k].dtype == np.float32 for k in FLOAT_KEYS + ("nsd",)) and got["nsd"].shape == (B, len(LABELS), len(TOLERANCES))
        assert_metrics_close(got, oracle(shape, name, spacing), (shape, name, spacing))


def test_empty_sets_give_nan_and_exact_counts():
    shape = (5, 9, 33)
    pred, truth = label_maps(shape, "pred_only")
    m = SD.surface_metrics(pred, truth, LABELS, (3.0, 0.5, 0.5), tolerances=(1.1,))
    # entry 0: class 1 in pred only; entry 1: class 2 in pred only
    for b, k in ((0, 0), (1, 1)):
        assert m["vol_pred"][b, k] > 0 and m["vol_truth"][b, k] == 0 and m["n_pred"][b, k] > 0 and m["n_truth"][b, k] == 0
        assert all(np.isnan(m[key][b, k]) for key in FLOAT_KEYS if key != "dice") and np.isnan(m["nsd"][b, k, 0])
        assert m["dice"][b, k] == 0.0
    for b, k in ((0, 1), (1, 0)):
        assert all(np.isfinite(m[key][b, k]) for key in FLOAT_KEYS) and np.isfinite(m["nsd"][b, k, 0])
    pred, truth = label_maps(shape, "absent")
    m = SD.surface_metrics(pred, truth, LABELS, tolerances=(1.1,))
    assert all(np.isnan(m[key]).all() for key in FLOAT_KEYS) and np.all(m["nsd"] == 1.0)
    assert all(np.all(m[key] == 0) for key in COUNT_KEYS)


def test_percentile_ends_and_single_element():
    pred, truth = label_maps((8, 40, 40), "ellipsoids")
    sp = (3.6, 0.3, 0.3)
    lo, hi = SD.surface_metrics(pred, truth, LABELS, sp, 0.0), SD.surface_metrics(pred, truth, LABELS, sp, 100.0)
    for b in range(B):
        for k, l in enumerate(LABELS):
            d_ab, d_ba, _ = directed_sets(pred[b], truth[b], l, sp)
            assert hi["hdq_ab"][b, k] == hi["hd_ab"][b, k] and hi["hdq_ba"][b, k] == hi["hd_ba"][b, k] and hi["hdq"][b, k] == hi["hd"][b, k]
            assert abs(float(lo["hdq_ab"][b, k]) - float(d_ab.min())) <= RTOL * float(d_ab.min())
            assert abs(float(lo["hdq"][b, k]) - float(min(d_ab.min(), d_ba.min()))) <= RTOL * float(min(d_ab.min(), d_ba.min()))
    # n = 1 in both directions: every percentile is the one distance between the two voxels
    pred, truth = label_maps((3, 5, 7), "single")
    for q in (0.0, 37.5, 95.0, 100.0):
        m = SD.surface_metrics(pred, truth, (1,), sp, q)
        for b in range(B):
            pa, pt = np.argwhere(pred[b] == 1)[0], np.argwhere(truth[b] == 1)[0]
            want = np.sqrt((((pa - pt) * np.array(sp)) ** 2).sum())
            assert m["n_pred"][b, 0] == 1 and m["n_truth"][b, 0] == 1
            for key in ("hd", "hd_ab", "hd_ba", "assd", "hdq", "hdq_ab", "hdq_ba"):
                assert abs(float(m[key][b, 0]) - want) <= RTOL * want, (q, key)


def test_swapping_pred_and_truth_swaps_the_directed_results():
    for name in ("ellipsoids", "random0.35", "pred_only"):
        pred, truth = label_maps((5, 9, 33), name)
        a = SD.surface_metrics(pred, truth, LABELS, (3.0, 0.5, 0.5), PERCENTILE, TOLERANCES)
        b = SD.surface_metrics(truth, pred, LABELS, (3.0, 0.5, 0.5), PERCENTILE, TOLERANCES)
        for x, y in (("hd_ab", "hd_ba"), ("mean_ab", "mean_ba"), ("hdq_ab", "hdq_ba"), ("n_pred", "n_truth"), ("vol_pred", "vol_truth")):
            assert np.array_equal(a[x], b[y], equal_nan=True) and np.array_equal(a[y], b[x], equal_nan=True), (name, x)
        for x in ("hd", "assd", "hdq", "nsd", "dice", "vol_both"):
            assert np.array_equal(a[x], b[x], equal_nan=True), (name, x)


def test_shifted_cube_has_hausdorff_distance_of_the_shift():
    shape = (12, 14, 16)
    for spacing in SPACINGS:
        for axis in range(3):
            for k in (1, 2, 3):
                truth = np.zeros(shape, np.uint8)
                truth[2:7, 3:8, 4:9] = 1
                pred = np.roll(truth, k, axis=axis)
                m = SD.surface_metrics(pred, truth, (1,), spacing)
                assert m["hd"].shape == (1,) and m["hd"][0] == np.float32(k * spacing[axis]), (spacing, axis, k)
                assert SD.hausdorff(pred, truth, (1,), spacing)[0] == m["hd"][0]


def test_conveniences_and_batch_axis():
    pred, truth = label_maps((5, 9, 33), "ellipsoids")
    sp = (3.0, 0.5, 0.5)
    m = SD.surface_metrics(pred, truth, LABELS, sp, 95.0, (1.1,))
    m0 = SD.surface_metrics(pred[0], truth[0], LABELS, sp, 95.0, (1.1,))
    for key in m:
        assert np.array_equal(m0[key], m[key][0], equal_nan=True), key
    assert np.array_equal(SD.hausdorff_percentile(pred, truth, LABELS, sp), m["hdq"])
    assert np.array_equal(SD.assd(pred, truth, LABELS, sp), m["assd"])
    assert np.array_equal(SD.nsd(pred, truth, 1.1, LABELS, sp), m["nsd"][..., 0])
    assert np.array_equal(SD.dice_per_class(pred, truth, LABELS), m["dice"])
    assert np.array_equal(SD.dice_per_class(pred[0], truth[0], LABELS), m["dice"][0])
    import model
    assert model.surface_distance is SD


def test_bad_arguments_raise_on_the_host():
    pred, truth = label_maps((3, 5, 7), "ellipsoids")
    for kw in (dict(spacing=(1.0, 0.0, 1.0)), dict(spacing=(1.0, 1.0)), dict(labels=()), dict(labels=tuple(range(1, 10))),
               dict(tolerances=(1.0,) * 5), dict(percentile=101.0)):
        with pytest.raises(ValueError):
            SD.surface_metrics(pred, truth, **kw)


def test_abi_rejects_bad_arguments_before_any_launch():
    """Every refusal comes before the first launch, so the pointers only have to be non-NULL and aligned: nothing dereferences them."""
    lib = L.load()
    p = 1 << 20
    lab, sp, tol = (ctypes.c_int * 8)(1, 2, 3, 4, 5, 6, 7, 8), (ctypes.c_double * 3)(3.0, 0.5, 0.5), (ctypes.c_float * 4)(1, 2, 3, 4)
    assert ctypes.sizeof(L.m1_sd_row_t) == 160
    assert lib.m1_sd_border(None, p, L.M1_SD_U8, lab, 2, 1, 3, 5, 7, p, p, p, None) == -1
    assert lib.m1_sd_border(p, p, L.M1_SD_U8, None, 2, 1, 3, 5, 7, p, p, p, None) == -1
    for K in (0, 9):
        assert lib.m1_sd_border(p, p, L.M1_SD_U8, lab, K, 1, 3, 5, 7, p, p, p, None) == -1
        assert lib.m1_sd_metrics(p, p, p, 1, K, 3, 5, 7, 95.0, tol, 1, p, p, None) == -1
        assert lib.m1_sd_ws_bytes(L.M1_SD_STAGE_BORDER, 1, K, 3, 5, 7) == 0
    assert lib.m1_sd_border(p, p, 7, lab, 2, 1, 3, 5, 7, p, p, p, None) == -2
    assert lib.m1_sd_distance(None, 1, 3, 5, 7, sp, p, p, None) == -1
    assert lib.m1_sd_distance(p, 1, 3, 5, 7, None, p, p, None) == -1
    for bad in ((0.0, 1.0, 1.0), (1.0, -0.5, 1.0), (1.0, 1.0, float("nan")), (float("inf"), 1.0, 1.0)):
        assert lib.m1_sd_distance(p, 1, 3, 5, 7, (ctypes.c_double * 3)(*bad), p, p, None) == -1
    for shape in ((257, 5, 7), (3, 257, 7), (3, 5, 257)):
        assert lib.m1_sd_distance(p, 1, *shape, sp, p, p, None) == -2
        assert lib.m1_sd_ws_bytes(L.M1_SD_STAGE_DISTANCE, 1, 1, *shape) == 0
    assert lib.m1_sd_metrics(p, p, None, 1, 2, 3, 5, 7, 95.0, tol, 5, p, p, None) == -1
    assert lib.m1_sd_metrics(p, p, None, 1, 2, 3, 5, 7, 95.0, None, 1, p, p, None) == -1
    assert lib.m1_sd_metrics(p, p, None, 1, 2, 3, 5, 7, 100.5, tol, 1, p, p, None) == -1
    assert lib.m1_sd_metrics(p, None, None, 1, 2, 3, 5, 7, 95.0, tol, 1, p, p, None) == -1
    # the workspace query is a pure host function
    assert lib.m1_sd_ws_bytes(L.M1_SD_STAGE_BORDER, 2, 2, 20, 160, 160) == 2 * 2 * 500 * 5 * 4
    assert lib.m1_sd_ws_bytes(L.M1_SD_STAGE_DISTANCE, 8, 1, 20, 160, 160) == 8 * 512000 * (2 + 8)
    assert lib.m1_sd_ws_bytes(L.M1_SD_STAGE_METRICS, 2, 2, 20, 160, 160) >= 4 * 2 * 6 * 256 * 4             # a histogram per rank, slice and direction at least
