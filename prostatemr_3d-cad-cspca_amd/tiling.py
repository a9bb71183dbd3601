"""Sliding-window inference, host side: where the tiles of a fixed-size network go on a larger volume, the separable weight they are
blended with, and fp64 restatements of the two kernels of csrc/tile.hip (m1_tile_gather / m1_tile_blend, ``ops.tile_gather`` /
``ops.tile_blend``).  ``predict_tiled`` of the detect model and of ``Ensemble`` (``unets.inference``) is the public surface; nothing here touches the GPU.

Tiles never leave the volume: an axis of length L takes n tiles of length t at evenly spread origins from 0 to L - t, so the last tile
ends at L and nothing is padded.  Tile t = (i0 * n[1] + i1) * n[2] + i2, and a stack of tiles is tile-major: sample t * B + b is tile t
of batch entry b."""
from __future__ import annotations

import math

import numpy as np

MAX_AXIS = 16                       # M1_TILE_MAX_AXIS (include/m1hip.h): the origins of an axis travel by value
WEIGHTINGS = ("gaussian", "constant")


def tile_origins(L, t, overlap=0.5):
    """The ascending origins of the tiles of length ``t`` on an axis of length ``L``: n = ceil((L - t) / (t * (1 - overlap))) + 1 tiles
    at round(i * (L - t) / (n - 1)) (numpy's round: halves to even), ``[0]`` when L == t.  Neighbours overlap by at least ``overlap`` *
    t before rounding.  ValueError: L < t, an overlap outside [0, 0.75], more than 16 tiles (the C ABI's limit), or a step below one
    voxel (t * (1 - overlap) < 1: two tiles would share an origin)."""
    L, t, overlap = int(L), int(t), float(overlap)
    if t < 1 or L < t:
        raise ValueError(f"tile_origins: an axis of {L} voxels does not hold a tile of {t}")
    if not 0.0 <= overlap <= 0.75:
        raise ValueError(f"tile_origins: overlap must be in [0, 0.75], got {overlap}")
    if L == t:
        return [0]
    step = t * (1.0 - overlap)
    if step < 1.0:
        raise ValueError(f"tile_origins: tiles of {t} voxels at overlap {overlap} advance by less than one voxel")
    n = int(math.ceil((L - t) / step)) + 1
    if n > MAX_AXIS:
        raise ValueError(f"tile_origins: {n} tiles of {t} on an axis of {L} at overlap {overlap}; at most {MAX_AXIS} per axis")
    return [int(np.round(i * (L - t) / (n - 1))) for i in range(n)]


def tile_geometry(vol, tile, overlap=0.5):
    """The fields of m1_tile_t for a volume ``vol`` = (D, H, W) cut into tiles ``tile`` = (d, h, w), plus T:
    {"vol", "tile", "n" (tiles per axis), "origin" (three ascending lists), "T" = n[0] * n[1] * n[2]}.  ``overlap``: one fraction or
    one per axis.  ValueError as ``tile_origins``."""
    vol, tile = tuple(int(v) for v in vol), tuple(int(v) for v in tile)
    if len(vol) != 3 or len(tile) != 3:
        raise ValueError(f"tile_geometry: vol and tile must be (D, H, W), got {vol} / {tile}")
    ov = tuple(overlap) if isinstance(overlap, (tuple, list)) else (overlap,) * 3
    if len(ov) != 3:
        raise ValueError(f"tile_geometry: one overlap or one per axis expected, got {overlap}")
    origin = [tile_origins(L, t, o) for L, t, o in zip(vol, tile, ov)]
    n = tuple(len(o) for o in origin)
    return {"vol": vol, "tile": tile, "n": n, "origin": origin, "T": n[0] * n[1] * n[2]}


def tile_weights(tile, mode="gaussian"):
    """Three fp32 rows w0[d], w1[h], w2[w]; the weight of a voxel inside its tile is their product.  'gaussian':
    exp(-0.5 * ((i - (t - 1) / 2) / (t / 8))^2) -- the centre counts most, an edge voxel still about 3e-4 of it -- computed in fp64 and
    rounded once; 'constant': ones (a plain average of the covering tiles)."""
    if mode not in WEIGHTINGS:
        raise ValueError(f"tile_weights: weighting must be one of {WEIGHTINGS}, got {mode!r}")
    rows = []
    for t in (int(v) for v in tile):
        if t < 1:
            raise ValueError(f"tile_weights: a tile extent of {t}")
        i = np.arange(t, dtype=np.float64)
        rows.append((np.exp(-0.5 * ((i - (t - 1) / 2.0) / (t / 8.0)) ** 2) if mode == "gaussian" else np.ones(t)).astype(np.float32))
    return rows


def _tile_slices(geom):
    """(t, (slice0, slice1, slice2)) of every tile in ascending t."""
    o, tl, n = geom["origin"], geom["tile"], geom["n"]
    for i0 in range(n[0]):
        for i1 in range(n[1]):
            for i2 in range(n[2]):
                yield (i0 * n[1] + i1) * n[2] + i2, tuple(slice(o[a][i], o[a][i] + tl[a]) for a, i in enumerate((i0, i1, i2)))


def gather_host(x, geom):
    """numpy restatement of m1_tile_gather: x (B, D, H, W, C) -> (T * B, d, h, w, C), tile-major; the values as they are."""
    x = np.asarray(x)
    B = x.shape[0]
    if tuple(x.shape[1:4]) != tuple(geom["vol"]):
        raise ValueError(f"gather_host: x {x.shape} is not on the volume {geom['vol']}")
    out = np.empty((geom["T"] * B, *geom["tile"], x.shape[4]), x.dtype)
    for t, (s0, s1, s2) in _tile_slices(geom):
        out[t * B:(t + 1) * B] = x[:, s0, s1, s2]
    return out


def blend_host(tiles, geom, weights):
    """fp64 restatement of m1_tile_blend: tiles (T * B, d, h, w, C), tile-major, and the three weight rows -> (B, D, H, W, C) fp64.
    Per voxel over its covering tiles in ascending t: w_i = (w0 * w1) * w2 at the voxel's place in tile i, W = sum w_i,
    out = sum (w_i / W) * v_i.
    A reference should not carry the roundings it is there to measure: with k covering tiles, plain fp64 arithmetic in this order is
    off by up to about 2k + 2 half-ulps (6 * 2^-53 relative was seen at k = 12), so the products, both sums and the division run in
    numpy's widest float (``np.longdouble``: a 64-bit mantissa on x86-64) and the result is rounded to fp64 once.  Where longdouble is
    no wider than double this is the plain fp64 computation."""
    wide = np.longdouble
    tiles = np.asarray(tiles, dtype=np.float64)
    T = geom["T"]
    if tiles.ndim != 5 or tiles.shape[0] % T or tuple(tiles.shape[1:4]) != tuple(geom["tile"]):
        raise ValueError(f"blend_host: tiles {tiles.shape} are not T * B = {T} * B tiles of {geom['tile']}")
    B = tiles.shape[0] // T
    w0, w1, w2 = (np.asarray(r, dtype=np.float64).astype(wide) for r in weights)
    w = (w0[:, None, None] * w1[None, :, None]) * w2[None, None, :]
    W = np.zeros(tuple(geom["vol"]), wide)
    for _, sl in _tile_slices(geom):
        W[sl] += w
    out = np.zeros((B, *geom["vol"], tiles.shape[4]), wide)
    for t, (s0, s1, s2) in _tile_slices(geom):
        out[:, s0, s1, s2] += (w / W[s0, s1, s2])[None, ..., None] * tiles[t * B:(t + 1) * B].astype(wide)
    return out.astype(np.float64)
