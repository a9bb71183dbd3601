"""Guard bands (tests/guarded.py) around every buffer of the tile kernels (csrc/tile.hip: m1_tile_gather, m1_tile_blend): the volume
and the stacked tiles of the copy; the tiles, the weight rows and the blended volume of the blend, each of exactly its element count.
(2, 5, 11, 13, C) is odd in every extent: the element path, tiles that end on the last voxel of every axis.  (1, 4, 32, 40, 3) moves
whole 16-byte groups, the last one ending on the last byte of its tensor.  Inputs are finite: an index that left a tensor would read a
guard -- 0xFF bytes, NaN in fp32 and bf16 -- which the compared results would show, or write one, which ``check`` shows."""
import numpy as np
import pytest
import torch

from guarded import guarded
from util import PKG, ops
from test_mc_inference import as_np
import tiling_ref as Rf

pytestmark = pytest.mark.gpu
T = PKG.tiling
U = 2.0 ** -24
CASES = [((2, 5, 11, 13, C), (4, 8, 8)) for C in (1, 2, 3, 4, 5)] + [((1, 4, 32, 40, 3), (4, 32, 32))]


@pytest.fixture
def g(dev, monkeypatch):
    with guarded(monkeypatch, dev) as g_:
        yield g_


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=lambda v: str(v).replace("torch.", ""))
@pytest.mark.parametrize("shape,tile", CASES, ids=str)
def test_both_ops_under_guards(g, shape, tile, dtype):
    B, vol, C = shape[0], shape[1:4], shape[4]
    geom = T.tile_geometry(vol, tile)
    n_tiles = geom["T"] * B * int(np.prod(tile)) * C
    x = torch.from_numpy(np.random.default_rng(31).standard_normal(shape).astype(np.float32)).to(dtype)
    w = T.tile_weights(tile)
    with torch.no_grad():
        tiles = ops.tile_gather(g.put(x), geom)                                       # the op's one allocation
        assert g.count == 1 and tiles.numel() == n_tiles and tiles.dtype == dtype
        want = T.gather_host(as_np(x), geom)
        assert np.array_equal(as_np(tiles), want)
        prof = g.put(torch.from_numpy(np.concatenate(w)))
        assert prof.numel() == sum(tile)
        acc = g.put(torch.from_numpy(want))                                           # fp32 tiles of exactly their element count
        out = ops.tile_blend(acc, geom, prof)
        assert g.count == 2 and out.numel() == int(np.prod(shape))
    assert g.check() == 5
    got = as_np(out).astype(np.float64)
    assert np.isfinite(got).all()
    k = Rf.cover_count(geom)[None, ..., None]
    assert (np.abs(got - T.blend_host(want, geom, w)) <= (k + 3) * U * T.blend_host(np.abs(want), geom, w)).all()
