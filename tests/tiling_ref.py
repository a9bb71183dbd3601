"""A third statement of the tile blend (csrc/tile.hip: m1_tile_blend; tiling.blend_host is the vectorised second): one Python loop per
output voxel, written from the header's sentences.  For every voxel the covering tiles are found by testing every tile, visited in
ascending t = (i0 * n[1] + i1) * n[2] + i2; w_i = (w0 * w1) * w2 at the voxel's position inside tile i; W = sum w_i; out_c = sum
(w_i / W) * v_i,c.  fp64 throughout.  Also the two side results the derived bound of tests/test_tiling.py needs: the cover count k of
every voxel and sum_i (w_i / W) |v_i,c|.

    |kernel - fp64| <= (k + 3) * 2^-24 * sum_i (w_i / W) |v_i|

The count: w_i carries 2 roundings (two fp32 products), W those plus its k - 1 additions, w_i / W one more, the product with v_i one,
and the k - 1 additions of the terms -- relative to quantities that sum_i (w_i / W) |v_i| bounds term by term, the first-order
total is below (k + 3) half-ulps of fp32 per unit of that sum (2 + 1 + 1 per term, and each partial sum's rounding k - 1 times)."""
import itertools

import numpy as np

U = 2.0 ** -24


def covering(geom, pos):
    """[(t, (d0, d1, d2))] of the tiles that hold voxel ``pos`` = (z, y, x), ascending in t; d = the voxel's place inside the tile."""
    o, tl, n = geom["origin"], geom["tile"], geom["n"]
    out = []
    for i0, i1, i2 in itertools.product(range(n[0]), range(n[1]), range(n[2])):
        d = tuple(pos[a] - o[a][i] for a, i in enumerate((i0, i1, i2)))
        if all(0 <= d[a] < tl[a] for a in range(3)):
            out.append(((i0 * n[1] + i1) * n[2] + i2, d))
    return out


def blend_loop(tiles, geom, weights):
    """tiles (T * B, d, h, w, C), tile-major -> (out (B, D, H, W, C) fp64, k (D, H, W) cover counts, mag (B, D, H, W, C) = sum_i
    (w_i / W) |v_i|)."""
    tiles = np.asarray(tiles, dtype=np.float64)
    T, vol = geom["T"], geom["vol"]
    B, C = tiles.shape[0] // T, tiles.shape[4]
    w0, w1, w2 = (np.asarray(r, dtype=np.float64) for r in weights)
    out = np.zeros((B, *vol, C))
    mag = np.zeros((B, *vol, C))
    k = np.zeros(vol, np.int64)
    for z, y, x in itertools.product(range(vol[0]), range(vol[1]), range(vol[2])):
        cov = covering(geom, (z, y, x))
        ws = [(w0[d[0]] * w1[d[1]]) * w2[d[2]] for _, d in cov]
        W = 0.0
        for w in ws:
            W = W + w
        k[z, y, x] = len(cov)
        for (t, d), w in zip(cov, ws):
            v = tiles[t * B:(t + 1) * B, d[0], d[1], d[2], :]
            out[:, z, y, x, :] += (w / W) * v
            mag[:, z, y, x, :] += (w / W) * np.abs(v)
    return out, k, mag


def cover_count(geom):
    """(D, H, W) int: how many tiles cover each voxel (vectorised; equals blend_loop's k)."""
    k = np.ones(geom["vol"], np.int64)
    for a in range(3):
        c = np.zeros(geom["vol"][a], np.int64)
        for o in geom["origin"][a]:
            c[o:o + geom["tile"][a]] += 1
        k = k * c.reshape([-1 if b == a else 1 for b in range(3)])
    return k
