"""The component kernels (csrc/components.hip) against the host restatements of detection.py, which tests/test_detection_host.py pins
against scipy: labelling with its numbering, the per-component table, the contingency table, the steps of the dynamic extraction and the
whole extraction / matching path.  Every comparison is exact (array_equal): the kernels compute integers and exact maxima.  Shapes and
patterns are the smallest that reach every path: inside one tile, one voxel past a tile edge on every axis, several tiles, W = 64 + 1,
long union chains across tile borders, contacts across tile corners, neighbours in memory that are not neighbours in the volume."""
import functools

import numpy as np
import pytest
import torch

from util import PKG, ops
from test_detection_host import (ALL_SHAPES, B, CASES, CONNECTIVITIES, SERPENTINE_SHAPE, blob_map, ndimage, needs_scipy, patterns)

Dt = PKG.detection
L = PKG.hip.lib
pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def reference(shape, name, connectivity):
    """(labels, counts) of the host restatement, computed once and shared (never modified) by the tests of this file and of
    test_guard_bands_components.py."""
    labels, counts = Dt.label_components_host(patterns(shape)[name], connectivity)
    labels.setflags(write=False)
    return labels, counts


def to_dev(a: np.ndarray, dev, dtype=None) -> torch.Tensor:
    return torch.from_numpy(np.array(a, dtype=dtype)).to(dev)                          # (a copy: the shared references are read-only)


def values_for(shape, seed=11) -> np.ndarray:
    """(B, *shape) fp32 with many equal values (quarters in [-0.5, 1]): every component's maximum is reached more than once."""
    return (np.random.default_rng(seed).integers(-2, 5, (B, *shape)) / 4).astype(np.float32)


def assert_stats_equal(got: dict, want: dict, what) -> None:
    for key in Dt.STAT_KEYS:
        g = got[key].cpu().numpy()
        assert g.dtype == want[key].dtype and np.array_equal(g, want[key]), (what, key)


# ---- labelling -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dtype", (np.float32, np.uint8))
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_labelling_equals_the_host_restatement(dev, shape, in_dtype):
    ws = ops.cc_workspace((B, *shape), dev)                                           # one workspace for every call of the shape
    for name, masks in patterns(shape).items():
        x = to_dev(masks, dev, in_dtype)
        for c in CONNECTIVITIES:
            want, counts = reference(shape, name, c)
            labels, k = ops.label_components(x, 0.0, c, ws=ws)
            assert labels.dtype == torch.int32 and k.dtype == torch.int32
            assert np.array_equal(k.cpu().numpy(), counts), (shape, name, c, k.tolist(), counts.tolist())
            assert np.array_equal(labels.cpu().numpy(), want), (shape, name, c)


def test_labelling_has_no_component_cap_and_restarts_per_batch_entry(dev):
    shape = (9, 40, 40)
    want, counts = reference(shape, "random0.2", 1)
    assert counts.min() > 1000
    labels, k = ops.label_components(to_dev(patterns(shape)["random0.2"], dev, np.float32), 0.0, 1)
    got = labels.cpu().numpy()
    assert [int(got[b].max()) for b in range(B)] == counts.tolist() == k.tolist()
    assert all(got[b][got[b] > 0].min() == 1 for b in range(B))
    # serpentine: ONE component through every tile border; the checkerboard: every voxel its own component, or one
    assert ops.label_components(to_dev(patterns(SERPENTINE_SHAPE)["serpentine"], dev, np.uint8), 0, 1)[1].tolist() == [1, 1]
    ck = to_dev(patterns(shape)["checkerboard"], dev, np.uint8)
    assert ops.label_components(ck, 0, 1)[1].tolist() == [int(m.sum()) for m in patterns(shape)["checkerboard"]]
    assert ops.label_components(ck, 0, 3)[1].tolist() == [1, 1]
    ends = to_dev(patterns(shape)["row_ends"], dev, np.uint8)
    assert [int(ops.label_components(ends, 0, c)[1].sum()) for c in CONNECTIVITIES] == [6, 6, 6]      # nothing merges across an end
    assert [ops.label_components(to_dev(patterns(shape)["corners"], dev, np.uint8), 0, c)[1][0].item() for c in CONNECTIVITIES] == [4, 3, 2]


def test_thresholds_strict_per_sample_and_nan(dev):
    shape = (5, 9, 33)
    rng = np.random.default_rng(2)
    x = (rng.integers(0, 11, (B, *shape)) / 10).astype(np.float32)                    # tenths: many values equal to a threshold
    x[0, 1, 2, 3] = np.nan                                                            # NaN > t is false: background
    xd = to_dev(x, dev)
    thr = np.array([0.3, 0.7], np.float32)
    per, kper = ops.label_components(xd, to_dev(thr, dev), 2)
    for b in range(B):
        with np.errstate(invalid="ignore"):
            want, k = Dt.label_components_host(x[b] > thr[b], 2)
        one, kone = ops.label_components(xd, float(thr[b]), 2)                         # the scalar form, the whole batch at thr[b]
        assert np.array_equal(per[b].cpu().numpy(), want) and kper[b].item() == k
        assert torch.equal(one[b], per[b]) and kone[b] == kper[b]
    tenths = np.rint(np.nan_to_num(x) * 10).astype(np.uint8)
    got, _ = ops.label_components(to_dev(tenths, dev), 3, 1)                           # strict: 3 is background at threshold 3
    assert np.array_equal(got.cpu().numpy(), Dt.label_components_host(tenths > 3, 1)[0])
    with pytest.raises(RuntimeError):
        ops.label_components(xd, 0.5, 4)
    with pytest.raises(RuntimeError):
        ops.label_components(xd.to(torch.float64), 0.5, 3)


@needs_scipy
def test_dense_volume_equals_scipy(dev):
    shape = (20, 160, 160)
    masks = np.random.default_rng(9).random((B, *shape)) < 0.35
    labels, k = ops.label_components(to_dev(masks, dev, np.uint8), 0, 3)
    got = labels.cpu().numpy()
    for b in range(B):
        want, n = ndimage.label(masks[b], np.ones((3, 3, 3)))
        assert k[b].item() == n and np.array_equal(got[b], want)


# ---- the tables ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,name,c", (((3, 5, 7), "random0.35", 1), ((5, 9, 33), "random0.2", 2), ((9, 40, 40), "random0.05", 3),
                                           ((2, 3, 65), "random0.5", 1), ((1, 1, 1), "full", 3), ((4, 33, 33), "serpentine", 1)))
def test_component_stats_equal_the_host_restatement(dev, shape, name, c):
    labels, counts = reference(shape, name, c)
    values = values_for(shape)
    ld, vd = to_dev(labels, dev), to_dev(values, dev)
    kb = int(counts.max())
    for K in sorted({max(kb - 2, 1), max(kb, 1), kb + 3}):                             # below, equal to and above K_b
        got = ops.component_stats(ld, vd, K)
        assert_stats_equal(got, Dt.component_stats_host(labels, values, K), (shape, name, K))
        assert tuple(got["count"].shape) == (B, K) and not got["rows"][:, kb:].any()   # rows beyond K_b are zero
    assert_stats_equal(ops.component_stats(ld, None, kb + 1), Dt.component_stats_host(labels, None, kb + 1), (shape, name, "no values"))


def test_argmax_tie_goes_to_the_smallest_index(dev):
    labels = np.ones((1, 2, 3, 70), np.int32)
    values = np.zeros(labels.shape, np.float32)
    values[0, 1, 2, 69] = values[0, 0, 1, 5] = values[0, 1, 0, 0] = 0.75
    values[0, 0, 0, 0] = -0.0
    got = ops.component_stats(to_dev(labels, dev), to_dev(values, dev), 2)
    assert got["argmax"].tolist() == [[70 + 5, 0]] and got["max"].tolist() == [[0.75, 0.0]] and got["count"].tolist() == [[420, 0]]
    allzero = ops.component_stats(to_dev(labels, dev), to_dev(values * 0 - 0.0, dev), 1)       # -0.0 everywhere: the first voxel
    assert allzero["argmax"].tolist() == [[0]] and allzero["max"].tolist() == [[0.0]]


@pytest.mark.parametrize("shape", ((3, 5, 7), (5, 9, 33), (9, 40, 40), (2, 3, 65)))
def test_component_overlap_equals_the_host_restatement(dev, shape):
    a, ka = reference(shape, "random0.2", 1)
    b, kb = reference(shape, "random0.35", 3)
    ad, bd = to_dev(a, dev), to_dev(b, dev)
    for ma, mb in ((int(ka.max()), int(kb.max())), (3, 1), (0, 0), (int(ka.max()) + 2, 2)):      # exact caps, caps below, caps above
        got = ops.component_overlap(ad, bd, ma, mb)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), Dt.overlap_host(a, b, ma, mb)), (shape, ma, mb)
    full = ops.component_overlap(ad, bd, int(ka.max()), int(kb.max()))
    assert full.sum(dim=(1, 2)).tolist() == [int(np.prod(shape))] * B


# ---- the steps and the extraction ---------------------------------------------------------------------------------------------
def test_peak_select_take_by_hand(dev):
    w = np.zeros((2, 1, 2, 70), np.float32)
    w[0, 0, 0, 10:14] = (0.5, 0.9, 0.9, 0.5)                                           # the first of two equal maxima
    w[0, 0, 1, 60:] = 0.3
    w[1] = 0.05
    wd = to_dev(w, dev)
    st = ops.cc_state(2, dev)
    ops.cc_peak(wd, st, factor=2.0, min_confidence=0.1, reset=True)
    s = st.cpu().numpy()
    assert s[L.M1_CC_ST_ARGMAX].tolist() == [11, 0] and s[L.M1_CC_ST_DONE].tolist() == [0, 1] and s[L.M1_CC_ST_NCAND].tolist() == [0, 0]
    assert s[L.M1_CC_ST_PEAK].view(np.float32).tolist() == [np.float32(0.9), np.float32(0.05)]
    assert s[L.M1_CC_ST_THRESHOLD].view(np.float32).tolist() == [np.float32(0.9) / np.float32(2.0), np.float32(0.05) / np.float32(2.0)]
    labels, _ = ops.label_components(wd, st[L.M1_CC_ST_THRESHOLD].view(torch.float32), 1)
    ops.cc_select(labels, st)
    s = st.cpu().numpy()
    assert s[L.M1_CC_ST_SEL].tolist() == [1, 0] and s[L.M1_CC_ST_COUNT].tolist() == [4, 0]
    out = torch.empty_like(wd)
    det, cand, conf = torch.empty_like(wd), torch.empty(wd.shape, dtype=torch.int32, device=dev), torch.empty((2, 3), device=dev)
    ops.cc_take(labels, st, out, det, cand, conf, min_voxels=3, reset=True, w_src=wd)
    want = w.copy()
    want[0, 0, 0, 10:14] = 0
    assert np.array_equal(out.cpu().numpy(), want) and conf.tolist() == [[np.float32(0.9), 0, 0], [0, 0, 0]]
    assert np.array_equal(det.cpu().numpy(), np.where(w >= 0.5, np.float32(0.9), np.float32(0)))
    assert np.array_equal(cand.cpu().numpy(), (w >= 0.5).astype(np.int32)) and st[L.M1_CC_ST_NCAND].tolist() == [1, 0]
    # second round on the working volume: the run of 0.3 has ten voxels, min_voxels = 11 drops it but still clears it
    ops.cc_peak(out, st, factor=2.0, min_confidence=0.1)
    labels, _ = ops.label_components(out, st[L.M1_CC_ST_THRESHOLD].view(torch.float32), 1)
    ops.cc_select(labels, st)
    ops.cc_take(labels, st, out, det, cand, conf, min_voxels=11)
    assert st[L.M1_CC_ST_COUNT].tolist() == [10, 0] and st[L.M1_CC_ST_NCAND].tolist() == [1, 0] and st[L.M1_CC_ST_DONE].tolist() == [0, 1]
    assert not out[0].any() and torch.equal(out[1], wd[1]) and conf.tolist() == [[np.float32(0.9), 0, 0], [0, 0, 0]]
    assert np.array_equal(cand.cpu().numpy(), (w >= 0.5).astype(np.int32))


@functools.lru_cache(maxsize=None)
def extraction_reference(threshold):
    maps = blob_map()
    out = Dt.extract_lesion_candidates(maps, threshold=threshold)
    for a in out:
        a.setflags(write=False)
    return maps, out


@pytest.mark.parametrize("threshold", ("dynamic", 0.25, 0.5))
def test_extraction_on_device_equals_the_host_path(dev, threshold):
    maps, (det, conf, cand) = extraction_reference(threshold)
    if threshold == "dynamic":
        # the cases the issue names: samples that stop after different numbers of rounds (the last one before the first: its peak is
        # below min_confidence), and a blob below min_voxels_detection that is cleared without becoming a candidate
        assert (conf > 0).sum(axis=1).tolist() == [4, 2, 0] and det[0][2, 10, 30] == 0 and maps[0][2, 10, 30] > 0.4
    gd, gc, gl = Dt.extract_lesion_candidates(to_dev(maps, dev), threshold=threshold)
    assert gd.dtype == torch.float32 and gl.dtype == torch.int32 and gc.dtype == torch.float32
    assert np.array_equal(gc.cpu().numpy(), conf) and np.array_equal(gl.cpu().numpy(), cand) and np.array_equal(gd.cpu().numpy(), det)
    one = Dt.extract_lesion_candidates(to_dev(maps[1], dev), threshold=threshold)       # (D,H,W) in, (D,H,W) out
    assert np.array_equal(one[0].cpu().numpy(), det[1]) and np.array_equal(one[2].cpu().numpy(), cand[1])
    k = int(cand[1].max())
    assert np.array_equal(one[1].cpu().numpy()[:k], conf[1][:k]) and not one[1][k:].any()


def test_extraction_other_parameters(dev):
    maps = blob_map(seed=4)
    for kw in (dict(num_lesions_to_extract=2), dict(min_voxels_detection=1, connectivity=1), dict(dynamic_threshold_factor=1.5, min_confidence=0.4)):
        want = Dt.extract_lesion_candidates(maps, **kw)
        got = Dt.extract_lesion_candidates(to_dev(maps, dev), **kw)
        for g, w in zip(got, want):
            assert np.array_equal(g.cpu().numpy(), w), kw


@pytest.mark.parametrize("case", CASES)
def test_evaluate_case_from_device_tensors(dev, case):
    det, gt, want, conf = case()
    got, c = Dt.evaluate_case(to_dev(det, dev), to_dev(gt, dev))
    assert got == want == Dt.evaluate_case(det, gt)[0] and c == conf
    maps, (dmap, _, _) = extraction_reference("dynamic")
    truth = (maps[0] > 0.45).astype(np.float32)
    assert Dt.evaluate_case(to_dev(dmap[0], dev), to_dev(truth, dev), overlap="dice") == Dt.evaluate_case(dmap[0], truth, overlap="dice")


# ---- determinism and capture ----------------------------------------------------------------------------------------------------
def test_every_op_is_bitwise_reproducible(dev):
    shape = (9, 40, 40)
    x = to_dev(patterns(shape)["random0.35"], dev, np.float32)
    vals = to_dev(values_for(shape), dev)
    maps = to_dev(blob_map(), dev)
    other = ops.label_components(to_dev(patterns(shape)["random0.2"], dev, np.uint8), 0, 1)[0]

    def run():
        labels, counts = ops.label_components(x, 0.0, 3)
        k = int(counts.max())
        rows = ops.component_stats(labels, vals, k)["rows"]
        table = ops.component_overlap(labels, other, k, 50)
        return (labels, counts, rows, table) + tuple(Dt.extract_lesion_candidates(maps)) + tuple(Dt.extract_lesion_candidates(maps, 0.25))

    first, second = run(), run()
    for a, b in zip(first, second):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_dynamic_extraction_is_capturable(dev):
    maps = to_dev(blob_map(), dev)
    call = lambda: Dt.extract_lesion_candidates(maps)
    eager = call()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        call()
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(gr):
        out = call()
    hist = PKG.hip.graphs.assert_no_memset_nodes(gr)                                   # the query behind bench.py's config.graph_nodes
    # five rounds of peak (2) + label (6) + select (2) + take (2) launches, nothing else: no copy of the map, no fill
    assert hist.get("kernel", 0) == 5 * 12 and not hist.get("memcpy", 0), hist
    gr.instantiate()
    for _ in range(3):
        for t in out:
            t.fill_(7)
        gr.replay()
        torch.cuda.synchronize()
        for t, e in zip(out, eager):
            assert torch.equal(t.view(torch.int32), e.view(torch.int32))
