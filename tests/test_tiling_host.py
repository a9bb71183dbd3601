"""Sliding-window inference without a GPU: ``tiling.tile_origins`` / ``tile_geometry`` / ``tile_weights``, the fp64 restatements
``gather_host`` / ``blend_host`` against the per-voxel loop of tests/tiling_ref.py, and the argument checks of m1_tile_gather /
m1_tile_blend (csrc/tile.hip), which answer before anything is launched."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import tiling_ref as Rf
from util import PKG, ops

L = PKG.hip.lib
T = PKG.tiling


@pytest.mark.parametrize("L_,t,want", [(5, 4, [0, 1]), (11, 8, [0, 3]), (13, 8, [0, 2, 5]), (44, 32, [0, 12]), (52, 32, [0, 10, 20]),
                                       (8, 8, [0]), (32, 32, [0])])
def test_origins_of_the_hand_listed_cases(L_, t, want):
    assert T.tile_origins(L_, t) == want


def test_origin_errors():
    with pytest.raises(ValueError, match="does not hold"):
        T.tile_origins(7, 8)
    for ov in (-0.01, 0.76, float("nan")):
        with pytest.raises(ValueError, match="overlap"):
            T.tile_origins(16, 8, ov)
    with pytest.raises(ValueError, match="at most 16"):
        T.tile_origins(8 + 4 * 16, 8)                      # 17 tiles at overlap 0.5
    assert len(T.tile_origins(8 + 4 * 15, 8)) == 16
    with pytest.raises(ValueError, match="less than one voxel"):
        T.tile_origins(4, 3, 0.75)                         # a step of 0.75 voxels: two tiles would share an origin


def test_cover_is_complete_over_a_sweep():
    n = 0
    for t, ov in itertools.product((4, 5, 8, 20, 32, 160), (0.0, 0.25, 0.5, 0.6, 0.75)):
        for L_ in list(range(t, 3 * t + 2)) + [7 * t + 3]:
            try:
                o = T.tile_origins(L_, t, ov)
            except ValueError as e:
                assert "at most 16" in str(e), (L_, t, ov, e)
                continue
            n += 1
            assert o[0] == 0 and o[-1] + t == L_, (L_, t, ov, o)
            assert all(a < b <= a + t for a, b in zip(o, o[1:])), (L_, t, ov, o)         # strictly ascending, no gap
            seen = np.zeros(L_, bool)
            for a in o:
                seen[a:a + t] = True
            assert seen.all()
            if L_ > t:                                                                     # neighbours overlap by overlap * t, to rounding
                assert max(b - a for a, b in zip(o, o[1:])) <= int(np.ceil(t * (1 - ov))), (L_, t, ov, o)
    assert n > 500


def test_geometry_fields():
    g = T.tile_geometry((5, 44, 52), (4, 32, 32))
    assert g == {"vol": (5, 44, 52), "tile": (4, 32, 32), "n": (2, 2, 3), "origin": [[0, 1], [0, 12], [0, 10, 20]], "T": 12}
    assert T.tile_geometry((24, 256, 256), (20, 160, 160))["T"] == 18
    assert T.tile_geometry((4, 32, 40), (4, 32, 32), (0.5, 0.5, 0.0))["origin"] == [[0], [0], [0, 8]]
    s = ops.tile_struct(g)
    assert tuple(s.vol) == (5, 44, 52) and tuple(s.n) == (2, 2, 3) and list(s.origin[2])[:4] == [0, 10, 20, 0]
    with pytest.raises(ValueError):
        T.tile_geometry((5, 44), (4, 32, 32))
    with pytest.raises(ValueError):
        T.tile_geometry((3, 44, 52), (4, 32, 32))


def test_weights():
    w = T.tile_weights((4, 8, 160), "gaussian")
    assert [r.shape for r in w] == [(4,), (8,), (160,)] and all(r.dtype == np.float32 for r in w)
    for r in w:
        t = r.size
        i = np.arange(t, dtype=np.float64)
        want = np.exp(-0.5 * ((i - (t - 1) / 2) / (t / 8)) ** 2)
        assert np.array_equal(r, want.astype(np.float32)) and (r > 0).all() and np.array_equal(r, r[::-1])
    assert all(np.array_equal(r, np.ones(t, np.float32)) for r, t in zip(T.tile_weights((4, 8, 160), "constant"), (4, 8, 160)))
    with pytest.raises(ValueError, match="weighting"):
        T.tile_weights((4, 8, 8), "linear")


@pytest.mark.parametrize("mode", T.WEIGHTINGS)
def test_blend_host_equals_the_voxel_loop(mode):
    geom, B, C = T.tile_geometry((5, 11, 13), (4, 8, 8)), 2, 3
    assert geom["n"] == (2, 2, 3)
    tiles = np.random.default_rng(3).standard_normal((geom["T"] * B, 4, 8, 8, C)).astype(np.float32)
    w = T.tile_weights(geom["tile"], mode)
    want, k, mag = Rf.blend_loop(tiles, geom, w)
    got = T.blend_host(tiles, geom, w)
    assert got.dtype == np.float64 and got.shape == (B, 5, 11, 13, C)
    assert float(np.abs(got - want).max()) <= 4 * 2.0 ** -53 * float(mag.max())
    assert np.array_equal(k, Rf.cover_count(geom)) and k.min() == 1 and k.max() == 2 * 2 * 3
    ones = np.argwhere(k == 1)                                  # a voxel one tile covers takes that tile's value exactly
    assert len(ones) >= 8
    for z, y, x in ones:
        (t, d), = Rf.covering(geom, (z, y, x))
        assert np.array_equal(got[:, z, y, x], tiles[t * B:(t + 1) * B, d[0], d[1], d[2]].astype(np.float64))


@pytest.mark.parametrize("mode", T.WEIGHTINGS)
def test_gather_then_blend_returns_the_volume(mode):
    """Tiles cut from one volume agree wherever they overlap, so their blend is the volume again.  The bound is 4 * 2^-53 relative,
    whatever the cover count k; the geometry is the GPU tests' (k up to 2 * 2 * 3 = 12).  blend_host computed in plain fp64 missed it
    with gaussian weights (worst over three seeds 6.01 * 2^-53 at k = 12, 5.87 at k = 6; constant weights 3.96): W carries k + 1
    roundings, every term two more and the sum k - 1.  It now accumulates in np.longdouble and rounds once."""
    geom = T.tile_geometry((5, 11, 13), (4, 8, 8))
    x = np.random.default_rng(4).standard_normal((2, 5, 11, 13, 3))
    tiles = T.gather_host(x, geom)
    assert tiles.shape == (24, 4, 8, 8, 3) and np.array_equal(tiles[2 * 5 + 1], x[1, 0:4, 3:11, 5:13])       # tile (0, 1, 2) of entry 1
    back = T.blend_host(tiles, geom, T.tile_weights(geom["tile"], mode))
    rel = float((np.abs(back - x) / np.abs(x)).max())
    print(f"gather_host -> blend_host ({mode}): max relative error {rel / 2.0 ** -53:.2f} * 2^-53")
    assert rel <= 4 * 2.0 ** -53


def _geom(vol=(5, 11, 13), tile=(4, 8, 8)):
    return ops.tile_struct(T.tile_geometry(vol, tile))


def test_bad_arguments_are_rejected_without_a_gpu():
    lib = L.load()
    for name in ("m1_tile_gather", "m1_tile_blend"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    ok = _geom()
    gather = lambda g, x=p, o=p, B=2, C=3, dt=0: lib.m1_tile_gather(x, B, C, dt, None if g is None else ctypes.byref(g), o, None)
    blend = lambda g, x=p, w=p, o=p, B=2, C=3: lib.m1_tile_blend(x, B, C, None if g is None else ctypes.byref(g), w, o, None)
    for f in (gather, blend):
        assert f(None) == -1                                                        # no geometry
        assert f(ok, x=None) == -1 and f(ok, o=None) == -1                          # NULL tensors
        assert f(ok, B=0) == -1 and f(ok, C=0) == -1
        assert f(ok, x=p + 2) == -1 and f(ok, o=p + 2) == -1                        # off the fp32 element
        for a in range(3):
            g = _geom(); g.vol[a] = 0
            assert f(g) == -1
            g = _geom(); g.tile[a] = 0
            assert f(g) == -1
            for n in (0, 17):
                g = _geom(); g.n[a] = n
                assert f(g) == -1, (a, n)
        g = _geom(); g.origin[2][1], g.origin[2][2] = 5, 2                          # not ascending
        assert f(g) == -1
        g = _geom(); g.origin[2][1] = 0                                             # twice the same origin
        assert f(g) == -1
        g = _geom(); g.origin[2][2] = 6                                             # the last tile leaves the volume
        assert f(g) == -1
        g = _geom(); g.origin[0][0] = -1
        assert f(g) == -1
        g = _geom(); g.origin[1][0] = 1                                             # voxel 0 of axis 1 uncovered
        assert f(g) == -1
        g = _geom(); g.n[2] = 2                                                     # [0, 8) and [2, 10): the end uncovered
        assert f(g) == -1
        g = _geom((5, 11, 30), (4, 8, 8)); g.origin[2][1] = 9                       # a gap between two tiles
        assert f(g) == -1
        big = ops.tile_struct({"vol": (1024, 1024, 1024), "tile": (1024, 1024, 1024), "n": (1, 1, 1), "origin": [[0], [0], [0]]})
        assert f(big, B=1, C=2) == -2 and f(big, B=2, C=1) == -2                    # 2^31 elements
    assert blend(ok, w=None) == -1 and blend(ok, w=p + 2) == -1
    assert gather(ok, dt=7) == -2                                                   # a dtype outside the enum
    assert gather(ok, x=p + 1, dt=1) == -1                                          # bf16 at an odd address


def test_wrappers_refuse_before_any_launch():
    geom = T.tile_geometry((5, 11, 13), (4, 8, 8))
    x = torch.zeros(2, 5, 11, 13, 3)
    with pytest.raises(RuntimeError, match="no_grad"):
        ops.tile_gather(x, geom)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="GPU"):
            ops.tile_gather(x, geom)
        with pytest.raises(RuntimeError, match="must be"):
            ops.tile_gather(x[:, :4], geom)
        tiles = torch.zeros(24, 4, 8, 8, 3)
        with pytest.raises(RuntimeError, match="must be fp32"):
            ops.tile_blend(tiles[:23], geom, T.tile_weights((4, 8, 8)))
        with pytest.raises(RuntimeError, match="profile"):
            ops.tile_blend(tiles, geom, torch.ones(19))
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            w = T.tile_weights((4, 8, 8))
            w[1][3] = bad
            with pytest.raises(ValueError, match="finite and > 0"):
                ops.tile_blend(tiles, geom, w)
        with pytest.raises(ValueError, match="three"):
            ops.tile_profile(T.tile_weights((4, 8, 8))[:2], "cpu")


def test_predict_tiled_argument_errors():
    NW = PKG.unets.networks
    m = NW.M1(input_spatial_dims=(4, 32, 32), input_channels=3, num_classes=2, dropout_rate=0.0, filters=(8, 16, 32, 64, 128),
              strides=((1, 1, 1), (1, 2, 2), (1, 2, 2), (2, 2, 2), (2, 2, 2)), summary=False)
    dm = m.get_detect_model()
    with pytest.raises(ValueError, match="at least the model's"):
        dm.predict_tiled(torch.zeros(1, 5, 44, 31, 3))
    with pytest.raises(ValueError, match="tiles_per_pass"):
        dm.predict_tiled(torch.zeros(1, 5, 44, 52, 3), tiles_per_pass=5)
    with pytest.raises(ValueError, match="weighting"):
        dm.predict_tiled(torch.zeros(1, 5, 44, 52, 3), weighting="linear")
    with pytest.raises(ValueError, match="overlap"):
        dm.predict_tiled(torch.zeros(1, 5, 44, 52, 3), overlap=0.9)
    with pytest.raises(ValueError):
        dm.predict_tiled(torch.zeros(1, 5, 44, 52, 3), n_draws=4, draws_per_pass=3)
    with pytest.raises(ValueError, match="at least the model's"):
        NW.Ensemble([m]).predict_tiled(torch.zeros(1, 4, 32, 31, 3))
    casc = NW.M1(input_spatial_dims=(4, 32, 32), input_channels=3, num_classes=2, dropout_rate=0.0, filters=(8, 16, 32, 64, 128),
                 strides=((1, 1, 1), (1, 2, 2), (1, 2, 2), (2, 2, 2), (2, 2, 2)), cascaded="noisy-or", summary=False)
    x2 = [torch.zeros(1, 5, 44, 52, 3)] * 2
    with pytest.raises(NotImplementedError, match="cascaded"):
        casc.get_detect_model().predict_tiled(x2)
    with pytest.raises(NotImplementedError, match="cascaded"):
        casc.get_detect_model().predict_scan(x2, (3.0, .5, .5), (3.0, .5, .5), region=(5, 44, 52))
