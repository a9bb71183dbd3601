"""Sliding-window inference on the GPU: the tile kernels (csrc/tile.hip: m1_tile_gather, m1_tile_blend; ops.tile_gather /
ops.tile_blend) and ``predict_tiled`` / ``predict_scan(region=)`` of the detect model and of ``Ensemble``.

Kernel level.  Shapes with a tile count of their own on every axis: vol (5, 11, 13) in tiles of (4, 8, 8) -> 2 x 2 x 3 tiles, odd in
every extent (the element path), and vol (4, 32, 40) in tiles of (4, 32, 32) -> 1 x 1 x 2 tiles at W origins 0 and 8 (whole 16-byte
groups for every C), also from pointers one element off the 16-byte grid (the element path on the same values).  The gather is a
copy and is compared bit for bit with torch slices.  The blend is compared with ``tiling.blend_host`` (fp64) under the bound derived
in tests/tiling_ref.py,

    |got - ref| <= (k + 3) * 2^-24 * sum_i (w_i / W) |v_i|,    k = the voxel's cover count,

which is never taken from the kernel: k comes from the geometry and the sum from blend_host of |tiles|.

Model level: fp32 compute, the (4, 32, 32) model of tests/test_mc_inference.py, B = 1, x (5, 44, 52) -> 2 x 2 x 3 = 12 tiles in
groups of 4."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from oracle import m1_oracle as O
from util import C1_FILTERS, C1_STRIDES, PKG, build_m1, ops, rnd
from test_mc_inference import DIMS, as_np
import mc_uncertainty_ref as Mu
import tiling_ref as Rf

pytestmark = pytest.mark.gpu

NW = PKG.unets.networks
P = PKG.preprocess
T = PKG.tiling
U = 2.0 ** -24
MAPS = ("mean", "entropy", "expected_entropy", "mutual_info", "variance")
SMALL, WHOLE = ((5, 11, 13), (4, 8, 8)), ((4, 32, 40), (4, 32, 32))
_ID = lambda v: str(v).replace("torch.", "")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _off(t):
    """The same values one element further: a tensor that starts off the 16-byte grid."""
    return torch.cat([t.reshape(-1)[:1], t.reshape(-1)])[1:].view(t.shape)


def _slices(x, geom):
    """torch slices and a cat: what the gather replaces."""
    o, tl = geom["origin"], geom["tile"]
    return torch.cat([x[:, a:a + tl[0], b:b + tl[1], c:c + tl[2]] for a, b, c in itertools.product(*o)])


# ---------------------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ID)
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_gather_is_torch_slicing_bit_for_bit(dev, dtype, C):
    with torch.no_grad():
        for (vol, tile), B in ((SMALL, 2), (WHOLE, 2)):
            geom = T.tile_geometry(vol, tile)
            x = rnd((B, *vol, C), 11 + C).to(dtype).to(dev)
            want = _slices(x, geom)
            got = ops.tile_gather(x, geom)
            assert got.dtype == dtype and _bits_equal(got, want), (vol, C)
            xo = _off(x)
            assert xo.data_ptr() % 16 and _bits_equal(ops.tile_gather(xo, geom), want), (vol, C)
            if C == 3:                                   # tile-major: sample t * B + b is tile t of batch entry b
                t = (0 * geom["n"][1] + 0) * geom["n"][2] + 1
                o2 = geom["origin"][2][1]
                assert torch.equal(got[t * B + 1], x[1, :tile[0], :tile[1], o2:o2 + tile[2]])


def _blend_case(vol, tile, B, C, mode, seed):
    geom = T.tile_geometry(vol, tile)
    w = T.tile_weights(tile, mode)
    tiles = np.random.default_rng(seed).standard_normal((geom["T"] * B, *tile, C)).astype(np.float32)
    tiles[0, 0, 0, 0, :] = -0.0                          # voxel (0, 0, 0) has one cover: the sign of a zero is kept too
    ref = T.blend_host(tiles, geom, w)
    mag = T.blend_host(np.abs(tiles), geom, w)
    k = Rf.cover_count(geom)
    return geom, w, tiles, ref, mag, k


def _check_blend(got, geom, tiles, ref, mag, k, B, what):
    g = as_np(got).astype(np.float64)
    assert np.isfinite(g).all(), what
    bound = (k[None, ..., None] + 3) * U * mag
    err = np.abs(g - ref)
    assert (err <= bound).all(), (what, float((err / np.maximum(bound, 1e-300)).max()))
    # one cover: the tile's own bits
    o, tl = geom["origin"], geom["tile"]
    g32, seen = as_np(got), 0
    for z, y, x in np.argwhere(k == 1):
        (t, d), = Rf.covering(geom, (z, y, x))
        a, b = g32[:, z, y, x], tiles[t * B:(t + 1) * B, d[0], d[1], d[2]]
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), (what, z, y, x)
        seen += 1
    assert seen > 0
    # a weighted mean stays between the least and the largest covering value, up to the bound
    lo, hi = np.full(ref.shape, np.inf), np.full(ref.shape, -np.inf)
    for t, (a, b, c) in enumerate(itertools.product(*o)):
        s = (slice(None), slice(a, a + tl[0]), slice(b, b + tl[1]), slice(c, c + tl[2]))
        v = tiles[t * B:(t + 1) * B].astype(np.float64)
        lo[s], hi[s] = np.minimum(lo[s], v), np.maximum(hi[s], v)
    assert (g >= lo - bound).all() and (g <= hi + bound).all(), what
    return float((err / np.maximum(bound, 1e-300)).max())


@pytest.mark.parametrize("mode", T.WEIGHTINGS)
@pytest.mark.parametrize("C", [1, 2, 3, 4, 5])
def test_blend_matches_the_fp64_restatement(dev, C, mode):
    B = 2
    geom, w, tiles, ref, mag, k = _blend_case(*SMALL, B, C, mode, 20 + C)
    with torch.no_grad():
        td = torch.from_numpy(tiles).to(dev)
        got = ops.tile_blend(td, geom, w)
        assert tuple(got.shape) == (B, *SMALL[0], C) and got.dtype == torch.float32
        worst = _check_blend(got, geom, tiles, ref, mag, k, B, (C, mode))
        assert _bits_equal(ops.tile_blend(td, geom, w), got)                                  # run to run
        prof = ops.tile_profile(w, dev)
        for blocks in (1, 3):                                                                 # grid to grid
            with ops.config(M1_EW_BLOCKS=blocks):
                assert _bits_equal(ops.tile_blend(td, geom, prof), got), blocks
    print(f"tile_blend C={C} {mode}: worst |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("mode", T.WEIGHTINGS)
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_whole_group_path_and_its_unaligned_twin(dev, C, mode):
    """vol (4, 32, 40): W extents and origins (0, 8) are multiples of every group, so aligned tensors take 16-byte accesses; one
    element off they cannot, and the element path must give the same bits."""
    B = 2
    geom, w, tiles, ref, mag, k = _blend_case(*WHOLE, B, C, mode, 40 + C)
    assert geom["origin"][2] == [0, 8]
    with torch.no_grad():
        td = torch.from_numpy(tiles).to(dev)
        got = ops.tile_blend(td, geom, w)
        worst = _check_blend(got, geom, tiles, ref, mag, k, B, (C, mode))
        to = _off(td)
        assert td.data_ptr() % 16 == 0 and to.data_ptr() % 16
        assert _bits_equal(ops.tile_blend(to, geom, w), got)
        out = _off(torch.empty_like(got))
        g = ops.tile_struct(geom)
        rc = PKG.hip.lib.load().m1_tile_blend(td.data_ptr(), B, C, ctypes.byref(g), ops.tile_profile(w, dev).data_ptr(), out.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream)
        assert rc == 0 and out.data_ptr() % 16 and _bits_equal(out, got)
        with ops.config(M1_EW_BLOCKS=2):
            assert _bits_equal(ops.tile_blend(td, geom, w), got)
    print(f"tile_blend whole groups C={C} {mode}: worst |err| / bound = {worst:.3f}")


def test_gather_then_blend_of_consistent_tiles_is_the_volume(dev):
    """Tiles cut from one volume agree wherever they overlap: the blend gives the volume back within the bound (|v_i| = |x|)."""
    with torch.no_grad():
        for (vol, tile), C in ((SMALL, 3), (WHOLE, 3), (SMALL, 1)):
            geom = T.tile_geometry(vol, tile)
            x = rnd((2, *vol, C), 51).to(dev)
            back = ops.tile_blend(ops.tile_gather(x, geom), geom, T.tile_weights(tile))
            k = torch.from_numpy(Rf.cover_count(geom)).to(dev)[None, ..., None]
            assert bool(((back - x).abs().double() <= (k + 3) * U * x.abs().double()).all()), (vol, C)
            assert torch.equal(back[:, 0, 0, 0], x[:, 0, 0, 0])


def test_captured_graph_replays_on_new_inputs(dev):
    """gather -> blend captured once (geometry by value, the profile on the device): three replays on three inputs equal three eager
    calls, and the graph holds no memset node."""
    vol, tile = WHOLE
    geom = T.tile_geometry(vol, tile)
    xs = [rnd((2, *vol, 3), 60 + i).to(dev) for i in range(3)]
    with torch.no_grad():
        prof = ops.tile_profile(T.tile_weights(tile), dev)
        eager = [ops.tile_blend(ops.tile_gather(x, geom), geom, prof).clone() for x in xs]
        buf = xs[0].clone()
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            ops.tile_blend(ops.tile_gather(buf, geom), geom, prof)
        torch.cuda.current_stream().wait_stream(st)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(gr):
            tiles = ops.tile_gather(buf, geom)
            out = ops.tile_blend(tiles, geom, prof)
        hist = PKG.hip.graphs.assert_no_memset_nodes(gr)
        assert hist.get("kernel", 0) == 2 and not hist.get("memcpy", 0), hist
        gr.instantiate()
        for x, want in zip(xs, eager):
            buf.copy_(x)
            gr.replay()
            torch.cuda.synchronize()
            assert _bits_equal(out, want) and _bits_equal(tiles, _slices(x, geom))


# ---------------------------------------------------------------------------------------------------------------------------------
# predict_tiled
# ---------------------------------------------------------------------------------------------------------------------------------
VOL, GROUP = (5, 44, 52), 4


def _cfg():
    return O.M1Config(input_spatial_dims=DIMS, filters=C1_FILTERS, strides=C1_STRIDES, dense_skip=True, probabilistic=True,
                      prob_latent_dims=(3, 2, 1, 0), dropout_rate=0.5, dropout_mode="monte-carlo")


@pytest.fixture(scope="module")
def models(dev):
    """Two probabilistic models of one configuration from different initial-weight seeds (two 'folds'), and the large input."""
    ms = []
    for seed in (5, 6):
        PKG.unets.network_blocks.set_init_seed(seed)
        m = build_m1(_cfg(), dev)
        m.eval()
        ms.append(m)
    return ms, rnd((1, *VOL, 3), 70).to(dev)


@pytest.mark.parametrize("mode", T.WEIGHTINGS)
def test_one_tile_is_the_untiled_call_bit_for_bit(models, dev, mode):
    ms, _ = models
    m, dm = ms[0], ms[0].get_detect_model()
    x = rnd((2, *DIMS, 3), 71).to(dev)
    calls = [(lambda: dm.predict(x), lambda: dm.predict_tiled(x, weighting=mode), 0),
             (lambda: dm.predict_mc(x, 4, 2, uncertainty=True), lambda: dm.predict_tiled(x, 4, 2, weighting=mode, uncertainty=True), 2),
             (lambda: dm.predict_mc(x, 2), lambda: dm.predict_tiled(x, 2, weighting=mode), 2),
             (lambda: dm.predict(x, tta=("", "w")), lambda: dm.predict_tiled(x, weighting=mode, tta=("", "w")), 0),
             (lambda: dm.predict_mc(x, 2, 2, uncertainty=True, tta=("", "hw")),
              lambda: dm.predict_tiled(x, 2, 2, weighting=mode, uncertainty=True, tta=("", "hw")), 2)]
    for i, (plain, tiled, steps) in enumerate(calls):
        m.seed_dropout(100 + i)
        want = plain()
        want = {k: v.clone() for k, v in want.items()} if isinstance(want, dict) else want.clone()
        state = m.rng_state.clone()
        assert int(state[1]) == steps, i
        m.seed_dropout(100 + i)
        got = tiled()
        assert torch.equal(m.rng_state, state), i
        if isinstance(want, dict):
            assert set(got) == set(want) and all(_bits_equal(got[k], want[k]) for k in want), i
        else:
            assert isinstance(got, torch.Tensor) and _bits_equal(got, want), i
    e = NW.Ensemble(ms)
    for m_ in ms:
        m_.seed_dropout(110)
    want = {k: v.clone() for k, v in e.predict_mc(x, 2, uncertainty=True).items()}
    for m_ in ms:
        m_.seed_dropout(110)
    got = e.predict_tiled(x, 2, weighting=mode, uncertainty=True)
    assert all(_bits_equal(got[k], want[k]) for k in want) and all(int(m_.rng_state[1]) == 2 for m_ in ms)
    # a single-member ensemble against its detect model: the tiled and the scan call are one body for both
    xv = models[1]
    g = np.random.default_rng(92)
    raw = torch.from_numpy((g.standard_normal((1, *SCAN, 3)) * 200 + 400).astype(np.float32)).to(dev)
    calls = (lambda p: p.predict_tiled(xv, tiles_per_pass=GROUP, weighting=mode, uncertainty=True, tta=("", "w")),
             lambda p: p.predict_scan(raw, SCAN_SP, NET_SP, n_draws=2, percentile=99.5, channels=1, uncertainty=True, region=(5, 44, 20),
                                      tiles_per_pass=GROUP, weighting=mode))
    for i, call in enumerate(calls):
        m.seed_dropout(115 + i)
        want = {k: ({j: t.clone() for j, t in v.items()} if k == "network" else v.clone()) for k, v in call(dm).items()}
        state = m.rng_state.clone()
        m.seed_dropout(115 + i)
        got = call(NW.Ensemble([m]))
        assert torch.equal(m.rng_state, state) and int(state[1]) > 0 and set(got) == set(want), i
        for k in want:
            pairs = [(got[k][j], want[k][j]) for j in MAPS] if k == "network" else [(got[k], want[k])]
            assert all(_bits_equal(a, b) for a, b in pairs), (i, k)


def _restated(dms, seeders, x, geom, weights, n, R):
    """fp64 maps of a tiled call restated from the public API: the same stacked groups (torch slices, same order) go through every
    member's ``predict_mc(return_samples=True)`` from the same states; the samples, exact fp32 inputs, are summed in fp64 into
    the accumulators of every tile, ``blend_host`` blends them and ``r_finish_u`` finishes them.  Also returns the per-tile fp32 means
    of a single member (the kernel's own sum_p / n per tile) and the fp32 restatement's error of every map."""
    Tn, B = geom["T"], int(x.shape[0])
    tiles = _slices(x, geom)
    for s in seeders:
        s()
    acc = {vt: [np.zeros((Tn * B, *DIMS, 2), vt), np.zeros((Tn * B, *DIMS), vt), np.zeros((Tn * B, *DIMS, 2), vt)] for vt in (np.float64, np.float32)}
    means = np.zeros((Tn * B, *DIMS, 2), np.float32)
    for k in range(Tn // GROUP):
        rows = slice(k * GROUP * B, (k + 1) * GROUP * B)
        for dm in dms:
            r = dm.predict_mc(tiles[rows], n, R, return_samples=True, uncertainty=True)
            s = as_np(r["samples"])
            means[rows] = as_np(r["mean"])
            for vt in acc:
                for p in s.astype(vt):
                    acc[vt][0][rows] += p
                    acc[vt][1][rows] += Mu.r_entropy(p, vt)
                    acc[vt][2][rows] += p * p
    N = n * len(dms)
    out = {}
    with np.errstate(all="ignore"):
        for vt in acc:
            sp, sh, sq = (T.blend_host(a if a.ndim == 5 else a[..., None], geom, weights) for a in acc[vt])
            if vt is np.float32:
                sp, sh, sq = (a.astype(np.float32) for a in (sp, sh, sq))
            out[vt] = Mu.r_finish_u(sp, sh[..., 0], sq, N, vt)
    e32 = {k: float(np.abs(out[np.float32][k].astype(np.float64) - out[np.float64][k]).max()) for k in MAPS}
    return out[np.float64], e32, means


def _map_bound(what, nc, N, kmax, e32):
    """mc_uncertainty_ref's bound from given samples, plus the blend's own roundings: every blended accumulator carries (kmax + 3)
    more roundings relative to its scale (tests/tiling_ref.py); mutual_info reads two accumulators, variance sum_pp and the mean twice."""
    k, scale = Mu.k_counts(nc, N, from_samples=True)[what]
    extra = {"mean": 1, "entropy": 1, "expected_entropy": 1, "mutual_info": 2, "variance": 3}[what] * (kmax + 3)
    return max((k + extra) * U * scale, 4 * e32)


def _check_maps(got, ref, e32, N, kmax, tag):
    worst = {}
    for what in MAPS:
        g = as_np(got[what]).astype(np.float64)
        assert g.shape == ref[what].shape and np.isfinite(g).all(), (tag, what)
        worst[what] = float(np.abs(g - ref[what]).max())
        assert worst[what] <= _map_bound(what, 2, N, kmax, e32[what]), (tag, what, worst[what], e32[what])
    return worst


def test_predict_tiled_is_the_blend_of_the_tiles_accumulators(models):
    ms, x = models
    m, dm = ms[0], ms[0].get_detect_model()
    geom, w = T.tile_geometry(VOL, DIMS), T.tile_weights(DIMS)
    assert geom["T"] == 12 and geom["n"] == (2, 2, 3)
    n, R = 2, 1
    ref, e32, means = _restated([dm], [lambda: m.seed_dropout(120)], x, geom, w, n, R)
    steps = int(m.rng_state[1])
    m.seed_dropout(120)
    got = dm.predict_tiled(x, n, R, tiles_per_pass=GROUP, uncertainty=True)
    # the state: one step per pass, (T / tiles_per_pass) * (n / R) passes, as the restated groups moved it
    assert int(m.rng_state[1]) == steps == (12 // GROUP) * (n // R) and int(m.rng_state[0]) == 120
    assert set(got) == set(MAPS) and tuple(got["mean"].shape) == (1, *VOL, 2) and tuple(got["entropy"].shape) == (1, *VOL)
    # n = 2: sum_p / n is exact and commutes with the blend, so the mean is the blend of the per-tile means under the derived bound
    k = Rf.cover_count(geom)
    mref, mmag = T.blend_host(means, geom, w), T.blend_host(np.abs(means), geom, w)
    err = np.abs(as_np(got["mean"]).astype(np.float64) - mref)
    assert (err <= (k[None, ..., None] + 3) * U * mmag).all(), float(err.max())
    worst = _check_maps(got, ref, e32, n, int(k.max()), "predict_tiled")
    print("predict_tiled 12 tiles, 2 draws: worst |err| against the restated samples", worst)
    # the mean tensor of one draw: `predict` per group at the current state, which does not move
    m.seed_dropout(121)
    one = dm.predict_tiled(x, tiles_per_pass=GROUP)
    assert isinstance(one, torch.Tensor) and tuple(one.shape) == (1, *VOL, 2) and int(m.rng_state[1]) == 0
    tiles = _slices(x, geom)
    per = np.concatenate([as_np(dm.predict(tiles[i:i + GROUP])) for i in range(0, 12, GROUP)])
    err = np.abs(as_np(one).astype(np.float64) - T.blend_host(per, geom, w))
    assert (err <= (k[None, ..., None] + 3) * U * T.blend_host(np.abs(per), geom, w)).all()
    # other groupings: other draws (the stream is keyed by the element index over the stacked batch), the same kind of result
    m.seed_dropout(121)
    other = dm.predict_tiled(x, tiles_per_pass=12)
    assert tuple(other.shape) == tuple(one.shape) and bool(torch.isfinite(other).all())


def test_ensemble_is_one_tiled_call_on_the_concatenated_draws(models):
    ms, x = models
    geom, w = T.tile_geometry(VOL, DIMS), T.tile_weights(DIMS, "constant")
    dms = [m.get_detect_model() for m in ms]
    n, R = 2, 2
    ref, e32, _ = _restated(dms, [lambda m=m, i=i: m.seed_dropout(130 + i) for i, m in enumerate(ms)], x, geom, w, n, R)
    e = NW.Ensemble(ms, seed=130)
    got = e.predict_tiled(x, n, R, tiles_per_pass=GROUP, weighting="constant", uncertainty=True)
    assert all(int(m.rng_state[1]) == (12 // GROUP) * (n // R) for m in ms)
    worst = _check_maps(got, ref, e32, n * len(ms), int(Rf.cover_count(geom).max()), "Ensemble.predict_tiled")
    print("Ensemble.predict_tiled 12 tiles, 2 x 2 draws: worst |err| against the restated samples", worst)


SCAN, SCAN_SP, NET_SP = (6, 60, 70), (3.6, .4, .4), (3.0, .5, .5)


def test_predict_scan_with_a_region(models, dev):
    ms, _ = models
    m, dm = ms[0], ms[0].get_detect_model()
    g = np.random.default_rng(91)
    raw = torch.from_numpy((g.standard_normal((1, *SCAN, 3)) * 200 + 400).astype(np.float32)).to(dev)
    kw = dict(tiles_per_pass=GROUP, overlap=0.5, weighting="gaussian")
    img = (5, 44, 32)                                    # max(region, the model's size) per axis: 2 x 2 x 1 tiles
    for unc, n in ((True, 2), (False, 1)):
        x, _ = P.prepare_scan(raw, SCAN_SP, NET_SP, img, percentile=99.5)
        assert tuple(x.shape) == (1, *img, 3)
        m.seed_dropout(140)
        net = dm.predict_tiled(x, n, 1, uncertainty=unc, **kw)
        m.seed_dropout(140)
        r = dm.predict_scan(raw, SCAN_SP, NET_SP, n_draws=n, percentile=99.5, channels=1, uncertainty=unc, region=(5, 44, 20), **kw)
        mean = net["mean"] if unc else net
        assert _bits_equal(r["mean"], P.restore(mean.contiguous(), SCAN, SCAN_SP, NET_SP, channels=1))
        assert tuple(r["mean"].shape) == (1, *SCAN, 1)
        if unc:
            assert all(_bits_equal(net[k], r["network"][k]) for k in MAPS)
            for k in ("entropy", "expected_entropy", "mutual_info"):
                assert _bits_equal(r[k], P.restore(net[k].unsqueeze(-1), SCAN, SCAN_SP, NET_SP, order=1)[..., 0]), k
            assert _bits_equal(r["variance"], P.restore(net["variance"].contiguous(), SCAN, SCAN_SP, NET_SP, order=1, channels=1))
        else:
            assert _bits_equal(r["network"], net)
    # region=None: the call as it was -- prepare_scan to the model's grid, predict, restore
    x, _ = P.prepare_scan(raw, SCAN_SP, NET_SP, DIMS, percentile=99.5)
    m.seed_dropout(141)
    want = P.restore(dm.predict(x).contiguous(), SCAN, SCAN_SP, NET_SP, channels=1)
    m.seed_dropout(141)
    r = dm.predict_scan(raw, SCAN_SP, NET_SP, percentile=99.5, channels=1)
    assert _bits_equal(r["mean"], want) and tuple(r["network"].shape) == (1, *DIMS, 2)
    e = NW.Ensemble(ms, seed=142)
    r = e.predict_scan(raw, SCAN_SP, NET_SP, n_draws=2, percentile=99.5, uncertainty=True, region=VOL, tiles_per_pass=12)
    assert tuple(r["network"]["mean"].shape) == (1, *VOL, 2) and tuple(r["variance"].shape) == (1, *SCAN, 2)


def test_errors_on_the_device(models, dev):
    ms, x = models
    dm = ms[0].get_detect_model()
    with pytest.raises(ValueError, match="at least the model's"):
        dm.predict_tiled(x[:, :, :31])
    with pytest.raises(ValueError, match="tiles_per_pass"):
        dm.predict_tiled(x, tiles_per_pass=5)
    with pytest.raises(ValueError, match="tiles_per_pass"):
        NW.Ensemble(ms).predict_tiled(x, tiles_per_pass=0)
