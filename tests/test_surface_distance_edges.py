"""The surface-distance kernels (csrc/surface.hip) at the edges of their own constants, each stage driven on its own with inputs built
for the edge and compared with a plain reference that shares nothing with the kernel's algorithm (DESIGN.md lists which constant every
shape targets).  tests/test_surface_distance.py runs one parameter point (K = 2, q = 95, T = 4, B = 2, D <= 20); here:

  distance  `ops.sd_distance` on sparse masks against a brute-force fp64 minimum over the feature voxels (no separable passes): rows
            of 63..256 voxels with the only feature at a ballot-word edge (SD_MAX_LINE = 4 x 64), lines of up to 256 voxels along H
            and D (SD_CH = 64 per block, SD_TC = 16 columns per tile), three spacings.  Bound: 1 fp32 ulp -- both sides form
            sum_a (s_a delta_a)^2 of the nearest feature in fp64 with a few correctly rounded operations (a few fp64 ulp apart, in
            another order) and round once to fp32; +inf in the same places.
  border    `ops.sd_border` for K = 1 and K = 8 (SD_MAX_K), unordered, repeated, absent and out-of-byte-range ids and the label 0
            (what a neighbour outside the volume reads as), uint8 and int32, B in {1, 3}: masks and counts exact.
  metrics   `ops.sd_metrics` on synthetic border masks and synthetic distances: nblk in {1, 14, 17, 18, 19} (the scan's unrolled fold
            and its ragged tail), q in {0, 37.5, 50, 95, 99.9, 100}, directed sets of 0, 1 and 2 elements, T in {0, 1, 4}, tolerances
            that ARE values of the set (so that `<=` and `<` count differently), 0 and +inf.  Counts and maxima exact; fp64 sums within
            2^-40 of math.fsum (a term passes through at most 8 thread-sequential + 6 shuffle + 3 wave + 19 block additions of
            non-negative fp64 values, each 2^-53 relative); means within RTOL = 2^-22; a percentile bit-exact where the interpolation
            weight is 0 or the two order statistics are equal, else within RTOL and between the two order statistics.
  slices    B = 5, K = 8: S = 40, a second block of the 64-thread per-slice kernels.
  nsd       tolerances 0, 1, 2, 3 at unit spacing, where distances 0, 1, 2, 3 occur and are exact: the inclusive comparison, end to end.
  capture   the whole call captured into one graph: 16 kernel nodes, no memset / memcpy node, replayed on new inputs.

The CPU tests (unmarked) pin every reference used here: the brute force against `edt_host`, scipy's erosion against `mask_border_host`
for the label 0, `np.percentile` against `percentile_host`, and the gap between the distances and the integer tolerances."""
import functools
import math

import numpy as np
import pytest
import torch

from util import PKG, ops
from test_surface_distance import to_host
from test_surface_distance_host import (COUNT_KEYS, FLOAT_KEYS, LABELS, PERCENTILE, RTOL, TOLERANCES, assert_metrics_close, directed_sets,
                                        label_maps, scipy_border, ulp_distance)

SD = PKG.surface_distance
L = PKG.hip.lib
gpu = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. distance transform ----------------------------------------------------------------------------------------------------
DT_SPACINGS = ((1.0, 1.0, 1.0), (3.6, 0.3, 0.3), (0.1, 10.0, 1.0))   # the last: the nearest feature along W is not the nearest overall
WORD_WIDTHS = (63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)
LONG_SHAPES = ((256, 3, 17), (130, 2, 5), (2, 256, 5), (3, 129, 18), (65, 1, 1))
DT_CASES = [("word", W) for W in WORD_WIDTHS] + [("long", s) for s in LONG_SHAPES]


def word_edge_stack(W):
    """(N,2,2,W) uint8: per volume ONE row with a feature layout (the three other rows have none, so every distance of the volume is a
    function of that row's pass along W alone), an empty volume between them, and a last volume with another layout in every row."""
    # first / last voxel; the last lane of word 0; the first lane of words 1, 2, 3 (the only feature that lane 63 of the word can see
    # through its own mask); both ends; either side of the first word border
    layouts = [(0,), (W - 1,), (63,), (64,), (0, W - 1), (62, 65), (128,), (192,)]
    vols = []
    for i, xs in enumerate(l for l in layouts if max(l) < W):
        v = np.zeros((2, 2, W), np.uint8)
        v[i % 2, (i // 2) % 2, list(xs)] = 1
        vols.append(v)
        if i == 1:
            vols.append(np.zeros((2, 2, W), np.uint8))              # all +inf, between two volumes that have a feature
    v = np.zeros((2, 2, W), np.uint8)
    v[0, 0, 0] = v[0, 1, W - 1] = v[1, 0, min(63, W - 2)] = 1       # row (1, 1) has no feature
    vols.append(v)
    return np.stack(vols)


def long_line_stack(shape):
    """(5,D,H,W) uint8 with features at the first and the last position of the longest axis only: first; none; last; both in different
    columns; both in one column.  5 volumes: the number of rows is odd wherever D * H is."""
    ax = int(np.argmax(shape))
    rest = [n for a, n in enumerate(shape) if a != ax]

    def at(t, j):
        p = [(7 * j + 1) % rest[0], (5 * j + 2) % rest[1]]
        p.insert(ax, t)
        return tuple(p)
    last = shape[ax] - 1
    vols = [np.zeros(shape, np.uint8) for _ in range(5)]
    vols[0][at(0, 0)] = 1
    vols[2][at(last, 1)] = 1
    vols[3][at(0, 2)] = vols[3][at(last, 3)] = 1
    vols[4][at(0, 4)] = vols[4][at(last, 4)] = 1
    return np.stack(vols)


@functools.lru_cache(maxsize=None)
def distance_stack(kind, key):
    m = word_edge_stack(key) if kind == "word" else long_line_stack(key)
    assert m.shape[0] >= 3 and int(np.prod(m.shape[1:])) <= 40000 and max(int(v.sum()) for v in m) <= 8
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def brute_force_edt(kind, key, spacing):
    """sqrt(min over the feature voxels of sum_a (spacing_a * delta_a)^2) in fp64, rounded to fp32; +inf in a volume without one."""
    stack = distance_stack(kind, key)
    s = np.asarray(spacing, np.float64)
    grid = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in stack.shape[1:]], indexing="ij"), axis=-1)
    out = np.full(stack.shape, np.inf, np.float32)
    for i, vol in enumerate(stack):
        best = np.full(vol.shape, np.inf)
        for p in np.argwhere(vol != 0).astype(np.float64):
            best = np.minimum(best, (((grid - p) * s) ** 2).sum(axis=-1))
        out[i] = np.sqrt(best).astype(np.float32)
    out.setflags(write=False)
    return out


def assert_distances(got, kind, key, spacing):
    want = brute_force_edt(kind, key, spacing)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(np.isposinf(got), np.isposinf(want)), (kind, key, spacing)
    assert ulp_distance(got, want) <= 1, (kind, key, spacing, ulp_distance(got, want))


@pytest.mark.parametrize("kind,key", DT_CASES)
def test_edt_host_equals_the_brute_force(kind, key):
    stack = distance_stack(kind, key)
    assert np.isposinf(brute_force_edt(kind, key, DT_SPACINGS[0])).all(axis=(1, 2, 3)).tolist() == [not v.any() for v in stack]
    for spacing in DT_SPACINGS:
        assert_distances(SD.edt_host(stack, spacing), kind, key, spacing)


@gpu
@pytest.mark.parametrize("kind,key", DT_CASES)
def test_distance_equals_the_brute_force(dev, kind, key):
    mask = torch.tensor(distance_stack(kind, key), device=dev)
    for spacing in DT_SPACINGS:
        assert_distances(ops.sd_distance(mask, spacing).cpu().numpy(), kind, key, spacing)


# ---- 2. border masks and counts over label sets ---------------------------------------------------------------------------------
BORDER_SHAPES = ((3, 5, 7), (8, 40, 40))           # 105 voxels: one chunk of SD_CHUNK = 1024; 12800: chunks that end inside a row
K8 = (5, 2, 7, 1, 8, 3, 6, 4)
LABEL_SETS = ((3,), K8, (2, 4, 2), (1, 200), (0, 1), (0,), (-5, 70000, 1), (257, 1, -255))


@functools.lru_cache(maxsize=None)
def id_maps(shape, B):
    """(pred, truth) int64 (B,D,H,W): blocks of 3 voxels of the ids 0..8 (so that interiors exist) with single voxels changed, some of
    them to -5 and to 70000, which a uint8 copy holds as 251 and 112."""
    rng = np.random.default_rng(sum(shape) * 17 + B)
    out = []
    for _ in range(2):
        coarse = rng.integers(0, 9, size=(B,) + tuple(-(-n // 3) for n in shape))
        v = coarse.repeat(3, 1).repeat(3, 2).repeat(3, 3)[:, :shape[0], :shape[1], :shape[2]].copy()
        flip = rng.random(v.shape) < 0.08
        v[flip] = rng.choice(np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, -5, 70000]), size=int(flip.sum()))
        v.setflags(write=False)
        out.append(v)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pocket_maps(shape, B):
    """(pred, truth) uint8 (B,D,H,W): a box of class 1 around the centre with a pocket of background inside it; the background
    touches every face of the volume (where a neighbour outside the volume reads as 0, the background's own id)."""
    D, H, W = shape
    out = []
    for shift in (0, 1):
        v = np.zeros((B,) + shape, np.uint8)
        for b in range(B):
            v[b, 1:D - 1, H // 6 + 1:H - H // 6 - 1 - shift, W // 6 + 1:W - W // 6 - 1] = 1
            x0 = W // 2 + (b if W >= 20 else 0)                                # (the pocket moves with the batch entry where there is room)
            v[b, D // 2 - D // 8:D // 2 + D // 8 + 1, H // 2 - H // 8:H // 2 + H // 8 + 1, x0 - W // 8:x0 + W // 8 + 1] = 0
            assert v[b, D // 2, H // 2, x0] == 0 and v[b, D // 2, H // 2, x0 - W // 8 - 1] == 1 and v[b, D // 2, H // 2, x0 + W // 8 + 1] == 1
        assert all(np.all(f == 0) for f in (v[:, 0], v[:, -1], v[:, :, 0], v[:, :, -1], v[..., 0], v[..., -1]))
        v.setflags(write=False)
        out.append(v)
    return tuple(out)


def border_reference(pred, truth, labels):
    """(borders (2,B,K,D,H,W) uint8, counts (B,K,5) int64) by the host restatement and numpy sums."""
    a = np.stack([pred.astype(np.int64) == l for l in labels], axis=1)
    b = np.stack([truth.astype(np.int64) == l for l in labels], axis=1)
    borders = np.stack([np.stack([SD.mask_border_host(m[:, k]) for k in range(len(labels))], axis=1) for m in (a, b)])
    ax = (-3, -2, -1)
    counts = np.stack([borders[0].sum(ax), borders[1].sum(ax), a.sum(ax), b.sum(ax), (a & b).sum(ax)], axis=-1).astype(np.int64)
    return borders.astype(np.uint8), counts


def test_mask_border_host_of_the_background_equals_scipy():
    for shape in BORDER_SHAPES:
        for maps in (pocket_maps(shape, 3), tuple(v.astype(np.uint8) for v in id_maps(shape, 3))):
            for v in maps:
                want = np.stack([scipy_border(x == 0) for x in v])
                assert want.any() and (shape == (3, 5, 7) or not np.array_equal(want, v == 0))   # (the larger volume has interior background)
                assert np.array_equal(SD.mask_border_host(v == 0), want), shape
                # every background voxel on a volume face is a border voxel
                face = np.zeros(v.shape, bool)
                face[:, [0, -1]] = face[:, :, [0, -1]] = face[..., [0, -1]] = True
                assert np.array_equal(want & face, (v == 0) & face)


@gpu
@pytest.mark.parametrize("dtype", (torch.uint8, torch.int32), ids=("uint8", "int32"))
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("shape", BORDER_SHAPES)
def test_borders_and_counts_over_label_sets(dev, shape, B, dtype):
    np_dtype = np.uint8 if dtype == torch.uint8 else np.int32
    for maps in (id_maps(shape, B), pocket_maps(shape, B)):
        pred, truth = (v.astype(np_dtype) for v in maps)                       # (uint8 wraps -5 and 70000: the reference sees what the kernel sees)
        pred_d, truth_d = torch.tensor(pred, device=dev), torch.tensor(truth, device=dev)
        for labels in LABEL_SETS:
            want_b, want_c = border_reference(pred, truth, labels)
            borders, counts = ops.sd_border(pred_d, truth_d, labels)
            assert borders.shape == (2, B, len(labels)) + shape and counts.shape == (B, len(labels), 5)
            got_b, got_c = borders.cpu().numpy(), counts.cpu().numpy()
            assert np.array_equal(got_b, want_b), (shape, B, labels)
            assert np.array_equal(got_c, want_c), (shape, B, labels, got_c, want_c)
            if labels == (2, 4, 2):
                assert np.array_equal(got_b[:, :, 0], got_b[:, :, 2]) and np.array_equal(got_c[:, 0], got_c[:, 2])
            if labels == (1, 200):
                assert not got_b[:, :, 1].any() and not got_c[:, 1].any()
            big_ids = shape == (8, 40, 40) and maps is id_maps(shape, B)
            if labels == (-5, 70000, 1) and dtype == torch.int32 and big_ids:
                assert got_c[:, :2, 2:4].all(), "the maps hold -5 and 70000"
            if labels[0] == 0 and (big_ids or maps is pocket_maps(shape, B)):
                assert got_c[:, 0, :4].all(), "the background is a populated class"


# ---- 3. metrics stage on constructed distances ----------------------------------------------------------------------------------
MT_SHAPES = ((4, 70, 100), (17, 8, 256), (1, 1, 34817), (19, 20, 100), (3, 5, 7))
MT_NBLK = {28000: (14, 2000), 34816: (17, 2048), 34817: (18, 1935), 38000: (19, 2000), 105: (1, 105)}
MT_B, MT_K = 2, 4
MT_S = MT_B * MT_K
QS = (0.0, 37.5, 50.0, 95.0, 99.9, 100.0)
FAMILIES = ("last_byte", "two_values", "zeros", "any_normal", "ascending", "descending")
SUM_RTOL = 2.0 ** -40


class MetricsCase:
    """Synthetic inputs of `ops.sd_metrics` and what a reference needs of them, for one shape and one family of distances.
    Slices: 0 dense / dense; 1 empty / dense; 2 dense / empty; 3 empty / empty; 4 one / two voxels; 5 one / one; 6 dense / sparse;
    7 two voxels / dense.  Direction 0 of slice s: the voxels of borders[0, s] with the values of dist[1, s]; direction 1: the reverse."""

    def __init__(self, shape, family):
        n = int(np.prod(shape))
        rng = np.random.default_rng(n * 7 + FAMILIES.index(family))
        m = np.zeros((2, MT_S, n), np.uint8)
        for s, dens in {0: (0.3, 0.3), 1: (0.0, 0.3), 2: (0.3, 0.0), 6: (0.3, 0.05), 7: (0.0, 0.3)}.items():
            for d in range(2):
                m[d, s] = rng.random(n) < dens[d]
        for s, cnt in {4: (1, 2), 5: (1, 1), 7: (2, 0)}.items():
            for d in range(2):
                m[d, s, rng.choice(n, cnt[d], replace=False)] = 1
        if family == "last_byte":                       # every rank splits from its neighbour only in the last 8-bit pass
            v = (0x3f800000 + rng.integers(0, 256, size=m.shape)).astype(np.uint32).view(np.float32)
        elif family == "two_values":
            v = np.where(rng.random(m.shape) < 0.5, np.float32(0.5), np.float32(0.75)).astype(np.float32)
            # direction 0 of slice 0: ranks lo and lo + 1 of q = 37.5 lie on either side of the change (at q = 50 both lie above it)
            at = rng.permutation(np.flatnonzero(m[0, 0]))
            c = int(math.floor((at.size - 1) * 0.375)) + 1
            v[1, 0, at[:c]], v[1, 0, at[c:]] = 0.5, 0.75
        elif family == "zeros":
            v = np.zeros(m.shape, np.float32)
        elif family == "any_normal":                    # any normal fp32 bit pattern, and exact zeros: no denormals, which are no distances
            v = rng.integers(0x00800000, 0x7f7fffff, size=m.shape, endpoint=True).astype(np.uint32).view(np.float32).copy()
            v[rng.random(m.shape) < 0.1] = 0.0
        else:                                           # all values of a volume distinct, in memory order or against it
            line = (0x3f000000 + 1021 * np.arange(n, dtype=np.int64)).astype(np.uint32).view(np.float32)
            v = np.broadcast_to(line if family == "ascending" else line[::-1], m.shape).copy()
        assert np.all((bits(v) == 0) | ((bits(v) >= 0x00800000) & (bits(v) <= 0x7f7fffff)))
        self.shape, self.family, self.n = shape, family, n
        self.borders = m.reshape((2, MT_B, MT_K) + shape)
        self.dist = v.reshape((2, MT_B, MT_K) + shape)
        self.sets = [(np.sort(v[1, s][m[0, s] != 0]), np.sort(v[0, s][m[1, s] != 0])) for s in range(MT_S)]      # sorted
        self.pooled = [np.sort(np.concatenate(p)) for p in self.sets]
        self.sums = [tuple(math.fsum(d.astype(np.float64).tolist()) for d in p) for p in self.sets]
        # tolerances that are values of the sets, next to 0 and +inf
        d0, d6 = self.sets[0][0], self.sets[6][1] if self.sets[6][1].size else self.sets[0][1]
        self.tolerances = (0.0, float(d0[d0.size // 3]), float(d6[d6.size // 2]), float("inf"))


@functools.lru_cache(maxsize=2)
def metrics_case(shape, family):
    return MetricsCase(shape, family)


def rank_parts(a, q):
    """(a[lo], a[up], weight) of the module's percentile rule on a sorted non-empty fp32 array."""
    h = (float(a.size - 1) * float(q)) / 100.0
    lo = min(max(int(math.floor(h)), 0), a.size - 1)
    return a[lo], a[min(lo + 1, a.size - 1)], h - lo


def check_metrics(got, case, q, tol, what):
    """``got``: the host copy of sd_metrics' dict with the (B, K) axes flattened to S, against plain numpy on the masked values."""
    T = len(tol)
    assert got["nsd"].shape == (MT_S, T) and got["le_ab"].shape == (MT_S, T) and got["le_ba"].shape == (MT_S, T), what
    assert np.isnan(got["dice"]).all(), what                                   # counts=None
    for s in range(MT_S):
        d, pooled, sums, w = case.sets[s], case.pooled[s], case.sums[s], (what, "slice", s)
        n0, n1 = d[0].size, d[1].size
        assert (got["n_ab"][s], got["n_ba"][s]) == (n0, n1), w
        le = [[int((x <= np.float32(t)).sum()) for t in tol] for x in d]
        assert got["le_ab"][s].tolist() == le[0] and got["le_ba"][s].tolist() == le[1], (w, got["le_ab"][s], got["le_ba"][s], le)
        for key, want in zip(("sum_ab", "sum_ba"), sums):
            assert abs(float(got[key][s]) - want) <= SUM_RTOL * want, (w, key, got[key][s], want)
        if n0 == 0 or n1 == 0:
            assert all(np.isnan(got[key][s]) for key in FLOAT_KEYS), w
            assert np.isnan(got["nsd"][s]).all() if n0 + n1 else np.all(got["nsd"][s] == 1.0), (w, got["nsd"][s])
            continue
        for key, want in (("hd_ab", d[0][-1]), ("hd_ba", d[1][-1]), ("hd", pooled[-1])):
            assert bits(got[key][s]) == bits(want), (w, key, got[key][s], want)
        m0, m1 = sums[0] / n0, sums[1] / n1
        for key, want in (("mean_ab", m0), ("mean_ba", m1), ("assd", (m0 + m1) / 2.0)):
            assert abs(float(got[key][s]) - want) <= RTOL * want, (w, key, got[key][s], want)
        for key, a, top in (("hdq_ab", d[0], "hd_ab"), ("hdq_ba", d[1], "hd_ba"), ("hdq", pooled, "hd")):
            g, want = got[key][s], SD.percentile_host(a, q)
            lo, up, wt = rank_parts(a, q)
            if wt == 0.0 or lo == up:
                assert bits(g) == bits(want), (w, key, q, g, want)
            else:
                assert abs(float(g) - float(want)) <= RTOL * float(want) and lo <= g <= up, (w, key, q, g, want, lo, up)
            if q == 100.0:
                assert bits(g) == bits(got[top][s]), (w, key, g, got[top][s])
        want = [np.float32((le[0][t] + le[1][t]) / (n0 + n1)) for t in range(T)]
        assert bits(got["nsd"][s]).tolist() == bits(want).tolist(), (w, got["nsd"][s], want)
        assert all(got["nsd"][s][t] == 1.0 for t in range(T) if tol[t] == float("inf")), w


def metrics_ws_bytes(nblk, S):
    """m1_sd_ws_bytes of the metrics stage: 56-byte partials and 6 x 256 histogram bins per block, slice and direction, 72 bytes of
    selection state per slice, twice."""
    up16 = lambda v: (v + 15) & ~15
    return up16(S * 2 * nblk * 56) + up16(2 * S * 72) + S * 2 * nblk * 6 * 256 * 4


@pytest.mark.parametrize("shape", MT_SHAPES)
def test_metric_shapes_give_the_block_counts_they_are_meant_to(shape):
    n = int(np.prod(shape))
    nblk, chunk = MT_NBLK[n]
    nb = min(-(-n // 2048), 64)
    assert (-(-n // nb), -(-n // -(-n // nb))) == (chunk, nblk)
    assert L.load().m1_sd_ws_bytes(L.M1_SD_STAGE_METRICS, MT_B, MT_K, *shape) == metrics_ws_bytes(nblk, MT_S)
    # the scan's unrolled fold runs from 14 blocks on; with 17..19 blocks some of its four parts have a tail after the unrolled part
    assert nblk == 1 or nblk >= 14


@pytest.mark.parametrize("shape", MT_SHAPES)
def test_percentile_host_equals_numpy_on_the_metric_inputs(shape):
    straddles = 0
    for family in FAMILIES:
        case = metrics_case(shape, family)
        assert [tuple(x.size for x in p) for p in case.sets][3:6] == [(0, 0), (1, 2), (1, 1)] and case.sets[7][0].size == 2
        assert case.sets[1][0].size == 0 and case.sets[2][1].size == 0 and min(case.sets[0][0].size, case.sets[0][1].size) > 2
        # `<=` and `<` count differently at the tolerances taken from the sets
        for t in case.tolerances[1:3]:
            assert sum(int((x <= np.float32(t)).sum()) - int((x < np.float32(t)).sum()) for p in case.sets for x in p) > 0, (family, t)
        for s in range(MT_S):
            for a in case.sets[s] + (case.pooled[s],):
                for q in QS:
                    got = SD.percentile_host(a, q)
                    if a.size == 0:
                        assert np.isnan(got)
                        continue
                    want = float(np.percentile(a.astype(np.float64), q, method="linear"))
                    assert abs(float(got) - want) <= RTOL * want, (shape, family, s, q, got, want)
                    lo, up, wt = rank_parts(a, q)
                    straddles += family == "two_values" and lo != up and wt != 0.0
    if int(np.prod(shape)) > 105:
        assert straddles > 0, "no percentile of the two-valued family interpolates across the change"


def numpy_metrics(case, q, tol, le=np.less_equal):
    """The dict check_metrics takes, evaluated with numpy in the order of the rules in surface_distance.py's docstring."""
    T, nan = len(tol), np.float32(np.nan)
    out = {k: np.zeros(MT_S, np.int64) for k in ("n_ab", "n_ba")}
    out.update({k: np.zeros((MT_S, T), np.int64) for k in ("le_ab", "le_ba")})
    out.update({k: np.zeros(MT_S, np.float64) for k in ("sum_ab", "sum_ba")})
    out.update({k: np.full(MT_S, nan) for k in FLOAT_KEYS})
    out["nsd"] = np.full((MT_S, T), nan)
    for s, (d0, d1) in enumerate(case.sets):
        out["n_ab"][s], out["n_ba"][s] = d0.size, d1.size
        out["sum_ab"][s], out["sum_ba"][s] = d0.astype(np.float64).sum(), d1.astype(np.float64).sum()
        for t, tau in enumerate(tol):
            out["le_ab"][s, t], out["le_ba"][s, t] = le(d0, np.float32(tau)).sum(), le(d1, np.float32(tau)).sum()
        if d0.size == 0 and d1.size == 0:
            out["nsd"][s] = 1.0
        if d0.size == 0 or d1.size == 0:
            continue
        m0, m1 = out["sum_ab"][s] / d0.size, out["sum_ba"][s] / d1.size
        out["hd_ab"][s], out["hd_ba"][s], out["hd"][s] = d0.max(), d1.max(), max(d0.max(), d1.max())
        out["mean_ab"][s], out["mean_ba"][s], out["assd"][s] = m0, m1, (m0 + m1) / 2.0
        for key, a in (("hdq_ab", d0), ("hdq_ba", d1), ("hdq", case.pooled[s])):
            out[key][s] = SD.percentile_host(a, q)
        out["nsd"][s] = ((out["le_ab"][s] + out["le_ba"][s]) / (d0.size + d1.size)).astype(np.float32)
    return out


@pytest.mark.parametrize("shape", ((3, 5, 7), (1, 1, 34817)))
def test_the_metric_checks_take_numpy_and_refuse_a_strict_comparison(shape):
    """check_metrics is what the device test asserts with: a plain numpy evaluation passes it, and the same evaluation with `d < tol`
    in place of `d <= tol` does not, in any family."""
    for family in FAMILIES:
        case = metrics_case(shape, family)
        for q, t in [(q, case.tolerances) for q in QS] + [(37.5, ()), (37.5, case.tolerances[1:2])]:
            check_metrics(numpy_metrics(case, q, t), case, q, t, (shape, family, q))
        with pytest.raises(AssertionError):
            check_metrics(numpy_metrics(case, 50.0, case.tolerances, np.less), case, 50.0, case.tolerances, (shape, family))


@gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", MT_SHAPES)
def test_metrics_stage_on_constructed_distances(dev, shape, family):
    case = metrics_case(shape, family)
    borders, dist = torch.tensor(case.borders, device=dev), torch.tensor(case.dist, device=dev)
    tol = case.tolerances
    runs = [(q, tol) for q in QS] + [(37.5, ()), (37.5, tol[1:2]), (99.9, tol[::-1])]
    for q, t in runs:
        m = ops.sd_metrics(borders, dist, None, q, t)
        assert m["nsd"].shape == (MT_B, MT_K, len(t)) and m["hd"].shape == (MT_B, MT_K)
        host = ops._sd_rows_dict(m["rows"].cpu(), len(t))                      # (one copy: the fields are views of the rows)
        got = {k: v.numpy().reshape((MT_S,) + tuple(v.shape[2:])) for k, v in host.items() if k != "rows"}
        check_metrics(got, case, q, t, (shape, family, q, t))


# ---- 4. more than one block of the per-slice kernels ----------------------------------------------------------------------------
S40_SHAPE, S40_B, S40_LABELS, S40_SPACING, S40_Q = (3, 5, 7), 5, (1, 2, 3, 4, 5, 6, 7, 8), (3.0, 0.5, 0.5), 62.5
# at spacing (3.0, 0.5, 0.5) a squared distance is m / 4 with an integer m: a distance equals 0.5 or 1.5 exactly (m = 1, 9) or is at
# least 0.5 * (sqrt(10) - 3) = 0.08 away, so the inclusive counts cannot hinge on a last bit
S40_TOLERANCES = (0.5, 1.5)


@functools.lru_cache(maxsize=None)
def s40_maps():
    """(pred, truth) uint8 (5,3,5,7) over the ids 0..8; entry b has no id b + 1 in pred and no id b + 3 in truth."""
    rng = np.random.default_rng(40)
    pred, truth = (rng.integers(0, 9, size=(S40_B,) + S40_SHAPE).astype(np.uint8) for _ in range(2))
    for b in range(S40_B):
        pred[b][pred[b] == b + 1] = 0
        truth[b][truth[b] == b + 3] = 0
    pred.setflags(write=False)
    truth.setflags(write=False)
    return pred, truth


@functools.lru_cache(maxsize=None)
def s40_reference():
    return SD.surface_metrics_host(*s40_maps(), S40_LABELS, S40_SPACING, S40_Q, S40_TOLERANCES)


def assert_s40(got):
    want = s40_reference()
    assert_metrics_close(got, want, "S = 40")
    # every class is populated in some entries and absent from others; the last eight slices (the second block of sd_rows_kernel, the
    # threads 0..15 of the second block of sd_stats_fold_kernel) differ from one another and from the first eight
    assert all((want[k] > 0).any(axis=0).all() and (want[k] == 0).any(axis=0).any() for k in ("n_pred", "n_truth"))
    rows = [tuple(np.asarray(got[k], np.float64).reshape(S40_B * 8, -1)[s].tolist() for k in COUNT_KEYS + FLOAT_KEYS + ("nsd",))
            for s in range(S40_B * 8)]
    assert len({repr(r) for r in rows[32:]}) == 8 and not {repr(r) for r in rows[32:]} & {repr(r) for r in rows[:8]}


def test_s40_host_reference_has_distinct_slices():
    assert_s40(s40_reference())


@gpu
def test_forty_slices_take_a_second_block(dev):
    pred, truth = (torch.tensor(v, device=dev) for v in s40_maps())
    got = SD.surface_metrics(pred, truth, S40_LABELS, S40_SPACING, S40_Q, S40_TOLERANCES)
    assert got["hd"].shape == (S40_B, 8) and got["nsd"].shape == (S40_B, 8, 2)
    assert_s40(to_host(got))


# ---- 5. inclusive tolerances end to end -------------------------------------------------------------------------------------------
INT_SHAPES, INT_TOLERANCES, UNIT = ((8, 40, 40), (5, 9, 33)), (0.0, 1.0, 2.0, 3.0), (1.0, 1.0, 1.0)


@pytest.mark.parametrize("shape", INT_SHAPES)
def test_integer_tolerances_are_met_exactly_and_missed_clearly(shape):
    pred, truth = label_maps(shape, "ellipsoids")
    d = np.concatenate([x for b in range(pred.shape[0]) for l in LABELS for x in directed_sets(pred[b], truth[b], l, UNIT)[:2]]).astype(np.float64)
    off = np.abs(d - np.rint(d))
    assert np.all((off == 0.0) | (off >= 0.16)), off[(off > 0) & (off < 0.16)]
    for t in INT_TOLERANCES:
        assert int((d <= t).sum()) > int((d < t).sum()), t


@gpu
@pytest.mark.parametrize("shape", INT_SHAPES)
def test_inclusive_tolerances_end_to_end(dev, shape):
    pred, truth = label_maps(shape, "ellipsoids")
    got = SD.surface_metrics(torch.tensor(pred, device=dev), torch.tensor(truth, device=dev), LABELS, UNIT, PERCENTILE, INT_TOLERANCES)
    assert_metrics_close(to_host(got), SD.surface_metrics_host(pred, truth, LABELS, UNIT, PERCENTILE, INT_TOLERANCES), shape)


# ---- 6. capture and replay --------------------------------------------------------------------------------------------------------
@gpu
def test_surface_metrics_is_capturable(dev):
    shape, sp = (5, 9, 33), (3.0, 0.5, 0.5)
    first, second = label_maps(shape, "ellipsoids"), label_maps(shape, "random0.35")
    pred, truth = torch.tensor(first[0], device=dev), torch.tensor(first[1], device=dev)
    call = lambda p, t: SD.surface_metrics(p, t, LABELS, sp, PERCENTILE, TOLERANCES)
    eager = {k: v.clone() for k, v in call(torch.tensor(second[0], device=dev), torch.tensor(second[1], device=dev)).items()}
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        call(pred, truth)
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(gr):
        out = call(pred, truth)
    hist = PKG.hip.graphs.assert_no_memset_nodes(gr)
    # border (2) + distance (3) + metrics (stats 2, four rounds of histogram and scan 8, rows 1): nothing else, no copy, no fill
    assert hist.get("kernel", 0) == 16 and not hist.get("memcpy", 0), hist
    gr.instantiate()
    pred.copy_(torch.tensor(second[0]))                                          # the captured call reads its inputs where they were
    truth.copy_(torch.tensor(second[1]))
    for _ in range(3):
        for t in out.values():
            t.fill_(7)
        gr.replay()
        torch.cuda.synchronize()
        for key, e in eager.items():
            t = out[key]
            assert t.dtype == e.dtype and t.shape == e.shape
            same = torch.equal(t.view(torch.int32), e.view(torch.int32)) if t.dtype == torch.float32 else torch.equal(t, e)
            assert same, key
    assert not np.array_equal(first[0], second[0])
