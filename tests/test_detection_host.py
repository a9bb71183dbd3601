"""detection.py on the host: the numpy restatements the component kernels are compared with (tests/test_components.py) are pinned here
against scipy.ndimage -- labelling with its numbering, find_objects, maximum, maximum_position, sum -- and ``auroc`` against sklearn.
The matching, FROC and the dynamic extraction are this project's own definitions: hand-built cases with known answers, and the dynamic
rule against a scipy transcription kept in this file.  No GPU: the C entry points are only asked to reject bad arguments."""
import ctypes
import functools

import numpy as np
import pytest

from util import PKG

Dt = PKG.detection
L = PKG.hip.lib

try:
    from scipy import ndimage
except ImportError:                                    # pragma: no cover
    ndimage = None
needs_scipy = pytest.mark.skipif(ndimage is None, reason="scipy is not installed")

TILE = L.M1_CC_TILE                                    # (4, 8, 32): the labelling kernel's tile
# (1,1,1); strictly inside a tile; one voxel past a tile edge on every axis; several tiles on every axis; W = 64 + 1
SHAPES = ((1, 1, 1), (3, 5, 7), (TILE[0] + 1, TILE[1] + 1, TILE[2] + 1), (9, 40, 40), (2, 3, 65))
SERPENTINE_SHAPE = (4, 33, 33)
DENSITIES = (0.05, 0.2, 0.35, 0.5, 0.8)
CONNECTIVITIES = (1, 2, 3)
B = 2


def serpentine(shape=SERPENTINE_SHAPE) -> np.ndarray:
    """Even rows full, odd rows one voxel at alternating ends, the same in every slice: one component that crosses every tile border
    many times (2308 voxels on (4, 33, 33))."""
    m = np.zeros(shape, bool)
    m[:, ::2, :] = True
    m[:, 1::4, -1] = True
    m[:, 3::4, 0] = True
    return m


def corner_blobs(shape) -> np.ndarray:
    """Two 2x2x2 blobs that touch only corner-to-corner across the corner of the first tile, two that touch only edge-to-edge across a
    tile edge: the pairs merge at connectivity 3, respectively 2 and 3."""
    tz, ty, tx = TILE
    m = np.zeros(shape, bool)
    m[tz - 2:tz, ty - 2:ty, tx - 2:tx] = True
    m[tz:tz + 2, ty:ty + 2, tx:tx + 2] = True
    m[0:2, 2 * ty - 2:2 * ty, tx - 2:tx] = True
    m[0:2, 2 * ty:2 * ty + 2, tx:tx + 2] = True
    return m


def row_ends(shape) -> np.ndarray:
    """(B, D, H, W): runs that end at x = W - 1 next to runs that start at x = 0 of the next row, the same across a slice end and across
    the two batch entries.  Neighbours in memory, not in the volume."""
    D, H, W = shape
    m = np.zeros((B, D, H, W), bool)
    m[0, 0, 2, W - 3:] = True
    m[0, 0, 3, :3] = True
    m[0, 0, H - 1, W - 2:] = True
    m[0, 1, 0, :2] = True
    m[0, D - 1, H - 1, W - 2:] = True
    m[1, 0, 0, :2] = True
    return m


@functools.lru_cache(maxsize=None)
def patterns(shape):
    """name -> (B, D, H, W) bool mask; the two batch entries differ wherever the pattern is random."""
    rng = np.random.default_rng(sum(shape) * 7 + 1)
    out = {"empty": np.zeros((B, *shape), bool), "full": np.ones((B, *shape), bool)}
    for p in DENSITIES:
        out[f"random{p}"] = rng.random((B, *shape)) < p
    z, y, x = np.indices(shape)
    checker = (z + y + x) % 2 == 0
    out["checkerboard"] = np.stack([checker, ~checker])
    if shape == SERPENTINE_SHAPE:
        out["serpentine"] = np.stack([serpentine(), serpentine()[:, ::-1].copy()])
    if shape[0] >= TILE[0] + 2 and shape[1] >= 2 * TILE[1] + 2 and shape[2] >= TILE[2] + 2:
        out["corners"] = np.stack([corner_blobs(shape), rng.random(shape) < 0.1])
    if shape[0] >= 2 and shape[1] >= 5 and shape[2] >= 7:
        out["row_ends"] = row_ends(shape)
    return out


ALL_SHAPES = SHAPES + (SERPENTINE_SHAPE,)


def blob_map(shape=(8, 40, 40), seed=0) -> np.ndarray:
    """(3, *shape) fp32 in [0, 1): sample 0 has blobs with peaks 0.9 / 0.7 / 0.5 / 0.3, the 0.5 one a single voxel wide (below ten voxels
    at its threshold), sample 1 one blob of 0.6, sample 2 nothing above 0.05; uniform noise of 0.02 everywhere."""
    rng = np.random.default_rng(seed)
    z, y, x = np.indices(shape).astype(np.float64)
    def blob(c, peak, sigma):
        return peak * np.exp(-((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2) / (2 * sigma ** 2))
    s0 = blob((3, 8, 8), 0.9, 2.0) + blob((4, 30, 10), 0.7, 2.0) + blob((2, 10, 30), 0.5, 0.6) + blob((5, 30, 30), 0.3, 2.5)
    s1 = blob((4, 20, 20), 0.6, 2.0)
    s2 = np.full(shape, 0.03)
    noise = rng.random((3, *shape)) * 0.02
    return (np.stack([s0, s1, s2]) * (1 - 0.02) + noise).astype(np.float32)


def structure(c):
    return ndimage.generate_binary_structure(3, c)


# ---- labelling -----------------------------------------------------------------------------------------------------------------
@needs_scipy
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_label_components_host_equals_scipy_numbering_included(shape):
    for name, masks in patterns(shape).items():
        for c in CONNECTIVITIES:
            labels, counts = Dt.label_components_host(masks, c)
            assert labels.dtype == np.int32 and labels.shape == masks.shape
            for b in range(B):
                want, k = ndimage.label(masks[b], structure(c))
                assert counts[b] == k and np.array_equal(labels[b], want), (shape, name, c, b)


@needs_scipy
def test_the_patterns_are_what_they_claim():
    s = serpentine()
    assert s.sum() == 2308 and [ndimage.label(s, structure(c))[1] for c in CONNECTIVITIES] == [1, 1, 1]
    assert [ndimage.label(corner_blobs((9, 40, 40)), structure(c))[1] for c in CONNECTIVITIES] == [4, 3, 2]
    checker = patterns((3, 5, 7))["checkerboard"][0]
    assert ndimage.label(checker, structure(1))[1] == checker.sum() and ndimage.label(checker, structure(3))[1] == 1
    ends = row_ends((9, 40, 40))
    assert [int(Dt.label_components_host(ends, c)[1].sum()) for c in CONNECTIVITIES] == [6, 6, 6]
    assert Dt.label_components_host(patterns((9, 40, 40))["random0.2"][0], 1)[1] > 1000            # no cap on the component count


def test_label_components_threshold_is_strict_and_per_batch():
    x = np.zeros((2, 1, 1, 4), np.float32)
    x[0, 0, 0] = (0.5, 0.5, 0.2, 0.6)
    x[1, 0, 0] = (0.0, 1.0, 0.0, 1.0)
    labels, counts = Dt.label_components(x, 0.5, 1)
    assert labels.tolist() == [[[[0, 0, 0, 1]]], [[[0, 1, 0, 2]]]] and counts.tolist() == [1, 2]
    assert Dt.label_components(x.astype(np.uint8), 0, 1)[1].tolist() == [0, 2]


# ---- the table -----------------------------------------------------------------------------------------------------------------
@needs_scipy
@pytest.mark.parametrize("shape", ((3, 5, 7), (9, 40, 40)))
def test_component_stats_host_equals_scipy(shape):
    rng = np.random.default_rng(5)
    for name in ("random0.2", "random0.5", "checkerboard"):
        mask = patterns(shape)[name][0]
        labels, k = ndimage.label(mask, structure(3 if name != "checkerboard" else 1))
        values = (rng.integers(0, 7, shape) / 4).astype(np.float32)                  # many ties
        for K in (max(k - 2, 1), k, k + 3):
            st = Dt.component_stats_host(labels.astype(np.int32), values, K)
            n = min(k, K)
            index = np.arange(1, n + 1)
            assert np.array_equal(st["count"][:n], ndimage.sum(np.ones(shape), labels, index).astype(np.int32))
            assert np.array_equal(st["max"][:n], ndimage.maximum(values, labels, index).astype(np.float32))
            # scipy's maximum_position does not promise the first of equal maxima: compare the value there, and the rule by hand
            flat_l, flat_v = labels.reshape(-1), values.reshape(-1)
            for l in range(1, n + 1):
                assert st["argmax"][l - 1] == np.flatnonzero((flat_l == l) & (flat_v == st["max"][l - 1]))[0]
                pos = ndimage.maximum_position(values, labels, l)
                assert values[pos] == st["max"][l - 1]
            for l, sl in enumerate(ndimage.find_objects(labels)[:n]):
                assert st["lo"][l].tolist() == [s.start for s in sl] and st["hi"][l].tolist() == [s.stop for s in sl]
            com = np.array(ndimage.center_of_mass(np.ones(shape), labels, index)).reshape(n, 3)
            assert np.allclose(st["sum"][:n] / st["count"][:n, None], com, rtol=1e-12, atol=0)
            for key in Dt.STAT_KEYS:
                assert st[key].shape[0] == K and not st[key][n:].any()                   # rows beyond the last component are zero
    none = Dt.component_stats_host(labels.astype(np.int32), None, 4)
    assert not none["max"].any() and none["argmax"].tolist() == [int(np.flatnonzero(labels.reshape(-1) == l)[0]) for l in (1, 2, 3, 4)]


def test_overlap_host_by_hand():
    a = np.array([[[0, 1, 1, 2, 3]]])
    b = np.array([[[1, 1, 0, 2, 2]]])
    assert Dt.overlap_host(a, b, 3, 2).tolist() == [[0, 1, 0], [1, 1, 0], [0, 0, 1], [0, 0, 1]]
    assert Dt.overlap_host(a, b, 2, 1).tolist() == [[0, 1], [1, 1], [0, 0]]        # labels above a cap are counted nowhere
    assert Dt.overlap_host(np.stack([a, a]), np.stack([b, a]), 3, 3).shape == (2, 4, 4)


# ---- matching, FROC, AUROC, Dice ---------------------------------------------------------------------------------------------------
def f32(v):
    return float(np.float32(v))


def case_one_hit_one_miss():
    """Two lesions, three candidates: one hit (IoU 24 / 40), one candidate overlapping the second lesion at IoU 1 / 20 = 0.05 < 0.10
    (so the lesion is missed and the candidate is a false positive), one candidate on nothing."""
    det, gt = np.zeros((8, 32, 32), np.float32), np.zeros((8, 32, 32), np.uint8)
    gt[2:4, 2:6, 2:6] = 1
    gt[3, 20, 10:21] = 1
    det[2:4, 2:6, 3:7] = 0.9
    det[3, 20, 20:30] = 0.7
    det[6:8, 10:14, 10:14] = 0.5
    return det, gt, [(1, f32(0.9), 24 / 40), (1, 0.0, 0.0), (0, f32(0.7), 0.0), (0, f32(0.5), 0.0)], f32(0.9)


def case_two_on_one():
    """Two candidates on one lesion: the larger overlap is the true positive, the other a false positive."""
    det, gt = np.zeros((8, 32, 32), np.float32), np.zeros((8, 32, 32), np.uint8)
    gt[2:4, 2:10, 2:10] = 2                                                            # (any grade >= 1 is a lesion)
    det[2:4, 2:6, 2:10] = 0.8
    det[2:4, 7:10, 2:10] = 0.6
    return det, gt, [(1, f32(0.8), 64 / 128), (0, f32(0.6), 0.0)], f32(0.8)


def case_empty_truth():
    det, gt = np.zeros((8, 32, 32), np.float32), np.zeros((8, 32, 32), np.uint8)
    det[1:3, 1:4, 1:4] = 0.4
    return det, gt, [(0, f32(0.4), 0.0)], f32(0.4)


def case_empty_map():
    det, gt = np.zeros((8, 32, 32), np.float32), np.zeros((8, 32, 32), np.uint8)
    gt[1:3, 1:4, 1:4] = 1
    return det, gt, [(1, 0.0, 0.0)], 0.0


CASES = (case_one_hit_one_miss, case_two_on_one, case_empty_truth, case_empty_map)


@pytest.mark.parametrize("case", CASES)
def test_evaluate_case_by_hand(case):
    det, gt, want, conf = case()
    got, c = Dt.evaluate_case(det, gt)
    assert got == want and c == conf


def test_evaluate_case_dice_and_min_overlap():
    det, gt, _, _ = case_one_hit_one_miss()
    got, _ = Dt.evaluate_case(det, gt, overlap="dice")
    assert got[0] == (1, f32(0.9), 48 / 64) and got[1] == (1, 0.0, 0.0)             # Dice 2 / 21 of the second pair is below 0.10
    got, _ = Dt.evaluate_case(det, gt, min_overlap=0.04)
    assert got == [(1, f32(0.9), 24 / 40), (1, f32(0.7), 1 / 20), (0, f32(0.5), 0.0)]
    with pytest.raises(NotImplementedError):
        Dt.evaluate_case(det, gt, overlap="jaccard")


def test_assignment_takes_the_largest_total_overlap():
    # candidate 1 overlaps both lesions, candidate 2 only the first: greedy by lesion would give lesion 1 its best candidate (1) and
    # leave lesion 2 without one
    table = np.array([[0, 10, 10], [10, 30, 20], [10, 25, 0]])
    got, _ = Dt.match_table(table, [0.9, 0.8])
    assert [r[:2] for r in got] == [(1, 0.8), (1, 0.9)]


def test_froc_by_hand():
    results = [case()[2] for case in CASES[:2]]
    curve = Dt.froc(results)
    assert curve["thresholds"].tolist() == [f32(v) for v in (0.9, 0.8, 0.7, 0.6, 0.5)]
    assert curve["sensitivity"].tolist() == [1 / 3, 2 / 3, 2 / 3, 2 / 3, 2 / 3]
    assert curve["fp_per_case"].tolist() == [0, 0, 0.5, 1.0, 1.5]
    assert (curve["num_lesions"], curve["num_cases"]) == (3, 2)
    at = Dt.froc(results + [CASES[2]()[2], CASES[3]()[2]], thresholds=[0.45, 0.0])
    assert at["sensitivity"].tolist() == [0.5, 0.5] and at["fp_per_case"].tolist() == [3 / 4, 1.0]   # a missed lesion is never detected
    assert np.isnan(Dt.froc([CASES[2]()[2]])["sensitivity"]).all()


def test_auroc_equals_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(3)
    for n in (2, 7, 50, 301):
        y = rng.integers(0, 2, n)
        y[:2] = (0, 1)
        scores = rng.integers(0, 6, n) / 5                                             # ties within and across the classes
        assert abs(Dt.auroc(y, scores) - metrics.roc_auc_score(y, scores)) <= 1e-12
        s = rng.random(n)
        assert abs(Dt.auroc(y, s) - metrics.roc_auc_score(y, s)) <= 1e-12


def test_auroc_by_hand():
    assert Dt.auroc([0, 0, 1, 1], [0.1, 0.4, 0.35, 0.8]) == 0.75
    assert Dt.auroc([0, 1], [0.5, 0.5]) == 0.5
    with pytest.raises(ValueError):
        Dt.auroc([1, 1], [0.2, 0.3])


def test_dice_3d_by_hand():
    pred = np.array([[0.5, 0.5], [0.0, 1.0]])
    lab = np.array([[1, 0], [0, 1]])
    got = Dt.dice_3d(pred, lab)
    assert got.dtype == np.float32 and got == np.float32((3 + 1e-7) / (4 + 1e-7))
    assert Dt.dice_3d(np.zeros((2, 2)), np.zeros((2, 2))) == np.float32(1)


# ---- extraction ----------------------------------------------------------------------------------------------------------------
def dynamic_by_scipy(softmax, n, min_voxels, factor, min_confidence, connectivity):
    """The rule of detection.extract_lesion_candidates('dynamic'), transcribed with scipy for one volume."""
    w = softmax.copy()
    det, cand, conf = np.zeros_like(softmax), np.zeros(softmax.shape, np.int32), []
    for _ in range(n):
        peak = w.max()
        i = np.unravel_index(np.argmax(w), w.shape)
        if not peak > min_confidence:
            break
        labels, _ = ndimage.label(w > np.float32(peak) / np.float32(factor), structure(connectivity))
        comp = labels == labels[i]
        if comp.sum() >= min_voxels:
            conf.append(peak)
            det[comp], cand[comp] = peak, len(conf)
        w[comp] = 0
    return det, conf, cand


@needs_scipy
def test_dynamic_extraction_equals_the_scipy_transcription():
    maps = blob_map()
    det, conf, cand = Dt.extract_lesion_candidates(maps)
    assert det.dtype == np.float32 and cand.dtype == np.int32 and conf.shape == (3, 5)
    counts = []
    for b in range(3):
        d, c, l = dynamic_by_scipy(maps[b], 5, 10, 2.5, 0.1, 3)
        assert np.array_equal(det[b], d) and np.array_equal(cand[b], l)
        assert conf[b, :len(c)].tolist() == [float(v) for v in c] and not conf[b, len(c):].any()
        counts.append(len(c))
        one = Dt.extract_lesion_candidates(maps[b])                                    # a single volume: no batch axis in the results
        assert np.array_equal(one[0], d) and np.array_equal(one[2], l) and np.array_equal(one[1], conf[b])
    # sample 0: the 0.9 and 0.7 blobs, the one-voxel blob (cleared, not kept), then the skirt the 0.9 blob left below 0.9 / 2.5 and the
    # 0.3 blob: five rounds, four candidates; sample 1: its blob and the blob's skirt (0.24), whose own skirt is below 0.1: two rounds
    assert counts == [4, 2, 0]
    assert (det[0][2, 10, 30], maps[0][2, 10, 30] > 0.4) == (0, True)


@needs_scipy
def test_static_extraction_by_scipy():
    maps = blob_map()
    det, conf, cand = Dt.extract_lesion_candidates(maps, threshold=0.25)
    for b in range(3):
        labels, k = ndimage.label(maps[b] > np.float32(0.25), structure(3))
        kept = [l for l in range(1, k + 1) if (labels == l).sum() >= 10]
        assert cand[b].max() == len(kept)
        for n, l in enumerate(kept):
            assert np.array_equal(cand[b] == n + 1, labels == l) and conf[b, n] == maps[b][labels == l].max()
            assert (det[b][labels == l] == conf[b, n]).all()
        assert not det[b][cand[b] == 0].any() and not conf[b, len(kept):].any()
    with pytest.raises(NotImplementedError):
        Dt.extract_lesion_candidates(maps, threshold="dynamic-fast")


def test_module_is_reachable_as_model_detection():
    import model.detection as alias
    assert alias is Dt
    src = open(Dt.__file__).read()
    assert "import scipy" not in src and "from scipy" not in src                     # the package stays numpy-only on the host


# ---- the C entry points reject bad arguments before any launch -------------------------------------------------------------------
def test_bad_arguments_are_rejected_without_a_gpu():
    lib = L.load()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 255) & ~255                                           # a 256-byte aligned host address: never dereferenced
    BAD = -1
    assert ctypes.sizeof(L.m1_cc_row_t) == 64
    assert lib.m1_cc_ws_bytes(0, 4, 4, 4) == 0 and lib.m1_cc_ws_bytes(2, 4, -1, 4) == 0
    n = 2 * 9 * 40 * 40
    assert lib.m1_cc_ws_bytes(2, 9, 40, 40) >= 2 * 4 * n and lib.m1_cc_ws_bytes(2, 9, 40, 40) % 16 == 0
    label = lambda src=p, conn=3, dims=(2, 3, 5, 7), labels=p, counts=p, ws=p, thr=None: \
        lib.m1_cc_label(src, L.M1_CC_F32, 0.0, thr, conn, *dims, labels, counts, ws, None)
    assert label(src=None) == BAD and label(labels=None) == BAD and label(counts=None) == BAD and label(ws=None) == BAD
    assert label(conn=0) == BAD and label(conn=4) == BAD
    for dims in ((0, 3, 5, 7), (2, 0, 5, 7), (2, 3, -5, 7), (2, 3, 5, 0)):
        assert label(dims=dims) == BAD
    assert label(ws=p + 4) == BAD and label(labels=p + 2) == BAD and label(thr=p + 1) == BAD
    assert lib.m1_cc_label(p, 7, 0.0, None, 3, 2, 3, 5, 7, p, p, p, None) == -2          # a dtype outside the enum
    assert lib.m1_cc_label(p, 0, 0.0, None, 3, 2, 1024, 1024, 1024, p, p, p, None) == -2  # B * n does not fit an int label
    assert lib.m1_cc_stats(None, None, 2, 3, 5, 7, 4, p, None) == BAD and lib.m1_cc_stats(p, None, 2, 3, 5, 7, 0, p, None) == BAD
    assert lib.m1_cc_stats(p, None, 2, 3, 5, 7, 4, p + 4, None) == BAD and lib.m1_cc_stats(p, None, 2, 3, 0, 7, 4, p, None) == BAD
    assert lib.m1_cc_overlap(p, None, 2, 105, 3, 3, p, None) == BAD and lib.m1_cc_overlap(p, p, 2, 0, 3, 3, p, None) == BAD
    assert lib.m1_cc_overlap(p, p, 2, 105, -1, 3, p, None) == BAD
    assert lib.m1_cc_peak(None, 2, 105, 2.5, 0.1, 1, p, p, None) == BAD and lib.m1_cc_peak(p, 2, 105, 0.0, 0.1, 1, p, p, None) == BAD
    assert lib.m1_cc_peak(p, 2, 105, 2.5, 0.1, 1, p, p + 8, None) == BAD and lib.m1_cc_peak(p, 0, 105, 2.5, 0.1, 1, p, p, None) == BAD
    assert lib.m1_cc_select(p, 2, 105, None, None) == BAD and lib.m1_cc_select(p, 2, -3, p, None) == BAD
    assert lib.m1_cc_take(p, p, None, None, p, p, p, 2, 105, 5, 10, 1, None) == BAD
    assert lib.m1_cc_take(p, p, None, p, p, p, p, 2, 105, 0, 10, 1, None) == BAD
    assert lib.m1_cc_relabel(p, None, 2, 105, 4, 10, p, p, p, p, p, None) == BAD
    assert lib.m1_cc_relabel(p, p, 2, 105, 0, 10, p, p, p, p, p, None) == BAD
