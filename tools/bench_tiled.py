"""Measurements of the sliding-window kernels and of predict_tiled (profiles/tiled.txt):

    python tools/bench_tiled.py --out profiles/tiled.txt

The README model's tile (20, 160, 160) inside a (24, 256, 256) region: 2 x 3 x 3 = 18 tiles at overlap 0.5, B = 1 and 2, resident
data, hipEvents around each call, 20 warm-up + 200 timed runs, twice per side, the sides alternating in one process:

  (a) ops.tile_gather, fp32 and bf16, C = 3, against torch slices + cat, and against a flat copy (Tensor.copy_) of as many bytes as
      the gather writes -- it reads and writes that many;
  (b) ops.tile_blend, C = 2, 3 and 1, gaussian weights, against the torch composition it replaces (T weighted += on slices of a
      zeroed volume, the same for a weight volume, a divide), and against a flat copy of (tiles + volume) / 2 bytes, which reads
      and writes as many bytes as the blend must read and write;
  (c) predict_tiled(x, tiles_per_pass=2) at one draw on the README model (C3 of bench.py, bf16), x (1, 24, 256, 256, 3), against the
      Python loop it replaces: slice, predict, weighted += , divide (2 warm-up + 6 timed runs, twice per side, alternating).
"""
import argparse
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from util import PKG, ops  # noqa: E402

T = PKG.tiling
VOL, TILE = (24, 256, 256), (20, 160, 160)


def timeit(fn, warm=20, runs=200):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return np.array(ts)


def alternate(sides, rounds=2, **kw):
    ts = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            ts[k].append(timeit(fn, **kw))
    return {k: np.concatenate(v) for k, v in ts.items()}


med = lambda t: float(np.median(t))                                                  # noqa: E731
us = lambda t: f"median {med(t) * 1e3:8.1f} us  min {t.min() * 1e3:8.1f} us  p90 {np.percentile(t, 90) * 1e3:8.1f} us"   # noqa: E731
name = lambda dt: str(dt).replace("torch.", "")                                      # noqa: E731


def origins(geom):
    return list(itertools.product(*geom["origin"]))


def slices_cat(x, geom):
    d, h, w = geom["tile"]
    return torch.cat([x[:, a:a + d, b:b + h, c:c + w] for a, b, c in origins(geom)])


def torch_blend(tiles, geom, w3, B):
    """The composition a caller writes: weighted += of every tile into a zeroed volume, the weights into another, a divide."""
    d, h, w = geom["tile"]
    out = torch.zeros((B, *geom["vol"], tiles.shape[-1]), dtype=torch.float32, device=tiles.device)
    wsum = torch.zeros((1, *geom["vol"], 1), dtype=torch.float32, device=tiles.device)
    for t, (a, b, c) in enumerate(origins(geom)):
        out[:, a:a + d, b:b + h, c:c + w] += w3 * tiles[t * B:(t + 1) * B]
        wsum[:, a:a + d, b:b + h, c:c + w] += w3
    return out / wsum


def flat_copy(nbytes, dev):
    src = torch.empty(nbytes // 4, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    return lambda: dst.copy_(src)


def part_a(say, dev):
    say("(a) tile_gather against torch slices + cat and against a flat copy of the bytes it writes; bytes = tiles read + tiles written")
    geom = T.tile_geometry(VOL, TILE)
    g = torch.Generator().manual_seed(0)
    for dtype, B in itertools.product((torch.float32, torch.bfloat16), (1, 2)):
        x = torch.randn((B, *VOL, 3), generator=g).to(dtype).to(dev)
        same = bool(torch.equal(ops.tile_gather(x, geom), slices_cat(x, geom)))
        nout = geom["T"] * B * int(np.prod(TILE)) * 3 * x.element_size()
        t = alternate({"kernel": lambda: ops.tile_gather(x, geom), "torch": lambda: slices_cat(x, geom), "copy": flat_copy(nout, dev)})
        say(f"  {name(dtype):8s} B={B} C=3  {2 * nout / 1e6:6.1f} MB  equal to slices + cat: {same}")
        say(f"      tile_gather  {us(t['kernel'])}  {2 * nout / med(t['kernel']) / 1e9:6.3f} TB/s at the median")
        say(f"      slices + cat {us(t['torch'])}")
        say(f"      flat copy    {us(t['copy'])}  {2 * nout / med(t['copy']) / 1e9:6.3f} TB/s at the median")
        say(f"      tile_gather / (slices + cat) = {med(t['kernel']) / med(t['torch']):.3f}   tile_gather / copy = "
            f"{med(t['kernel']) / med(t['copy']):.3f}  (medians)")


def part_b(say, dev):
    say("(b) tile_blend (gaussian) against the torch composition (T weighted += on slices of a zeroed volume, a weight volume, a divide)")
    say("    and against a flat copy that reads and writes as many bytes; bytes = tiles read + volume written")
    geom = T.tile_geometry(VOL, TILE)
    w = T.tile_weights(TILE)
    prof = ops.tile_profile(w, dev)
    w3 = (torch.from_numpy(w[0])[:, None, None] * torch.from_numpy(w[1])[None, :, None] * torch.from_numpy(w[2])[None, None, :])
    w3 = w3[None, ..., None].to(dev)
    g = torch.Generator().manual_seed(1)
    for C, B in itertools.product((2, 3, 1), (1, 2)):
        tiles = torch.rand((geom["T"] * B, *TILE, C), generator=g).to(dev)
        got, ref = ops.tile_blend(tiles, geom, prof), torch_blend(tiles, geom, w3, B)
        err = float((got - ref).abs().max())
        nbytes = (tiles.numel() + got.numel()) * 4
        t = alternate({"kernel": lambda: ops.tile_blend(tiles, geom, prof), "torch": lambda: torch_blend(tiles, geom, w3, B),
                       "copy": flat_copy(nbytes // 2, dev)})
        say(f"  fp32 B={B} C={C}  {nbytes / 1e6:6.1f} MB  max |kernel - torch| = {err:.2e}")
        say(f"      tile_blend  {us(t['kernel'])}  {nbytes / med(t['kernel']) / 1e9:6.3f} TB/s at the median")
        say(f"      torch       {us(t['torch'])}")
        say(f"      flat copy   {us(t['copy'])}  {nbytes / med(t['copy']) / 1e9:6.3f} TB/s at the median")
        say(f"      tile_blend / torch = {med(t['kernel']) / med(t['torch']):.3f}   tile_blend / copy = "
            f"{med(t['kernel']) / med(t['copy']):.3f}  (medians)")


def part_c(say, dev):
    PKG.unets.network_blocks.set_init_seed(0)
    init = PKG.initializers
    model = PKG.unets.networks.M1(
        input_spatial_dims=TILE, input_channels=3, num_classes=2, filters=(32, 64, 128, 256, 512),
        strides=((1, 1, 1), (1, 2, 2), (1, 2, 2), (2, 2, 2), (2, 2, 2)),
        kernel_sizes=((1, 3, 3), (1, 3, 3), (3, 3, 3), (3, 3, 3), (3, 3, 3)), prob_latent_dims=(3, 2, 1, 0), dropout_rate=0.5,
        dropout_mode="monte-carlo", se_reduction=(8, 8, 8, 8, 8), att_sub_samp=((1, 1, 1),) * 4,
        kernel_initializer=init.Orthogonal(gain=1.0), bias_initializer=init.TruncatedNormal(mean=0.0, stddev=1e-3),
        kernel_regularizer=init.l2(1e-4), bias_regularizer=init.l2(1e-4), cascaded=False, dense_skip=True, probabilistic=True,
        deep_supervision=True, summary=False).to(dev)
    model.set_compute_dtype(torch.bfloat16)
    model.seed_dropout(2)
    model.eval()
    dm = model.get_detect_model()
    x = torch.randn((1, *VOL, 3), generator=torch.Generator().manual_seed(3)).to(dev)
    geom = T.tile_geometry(VOL, TILE)
    w = T.tile_weights(TILE)
    w3 = (torch.from_numpy(w[0])[:, None, None] * torch.from_numpy(w[1])[None, :, None] * torch.from_numpy(w[2])[None, None, :])
    w3 = w3[None, ..., None].to(dev)
    d, h, ww = TILE

    def tiled():
        return dm.predict_tiled(x, tiles_per_pass=2)

    def by_hand():
        out = torch.zeros((1, *VOL, 2), dtype=torch.float32, device=dev)
        wsum = torch.zeros((1, *VOL, 1), dtype=torch.float32, device=dev)
        o = origins(geom)
        for i in range(0, len(o), 2):
            xin = torch.cat([x[:, a:a + d, b:b + h, c:c + ww] for a, b, c in o[i:i + 2]])
            p = dm.predict(xin)
            for j, (a, b, c) in enumerate(o[i:i + 2]):
                out[:, a:a + d, b:b + h, c:c + ww] += w3 * p[j:j + 1]
                wsum[:, a:a + d, b:b + h, c:c + ww] += w3
        return out / wsum
    err = float((tiled() - by_hand()).abs().max())
    t = alternate({"tiled": tiled, "by hand": by_hand}, warm=2, runs=6)
    say("(c) one draw over a (1, 24, 256, 256, 3) region with the README model (C3: probabilistic, dense skip, deep supervision, filters")
    say("    32..512, tile (20, 160, 160), bf16, untrained weights), 18 tiles, two per pass; hipEvents around the whole call, 2 warm-up + 6")
    say("    timed runs, twice, alternating")
    say(f"      predict_tiled(x, tiles_per_pass=2):                               {us(t['tiled'])}")
    say(f"      Python loop (slices + cat, predict, weighted +=, divide):         {us(t['by hand'])}")
    say(f"      predict_tiled / loop = {med(t['tiled']) / med(t['by hand']):.3f}  (medians)   max |tiled - loop| = {err:.2e} (same draws: the state does not move)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parts", default="abc")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tiled.py measures on a GPU; none is visible")
    out = open(a.out, "w") if a.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()
    dev = torch.device("cuda:0")
    say("Sliding-window inference: tiles of (20, 160, 160) in a (24, 256, 256) region, 18 tiles, one MI355X (gfx950); hipEvents around each")
    say("call, 20 warm-up + 200 timed runs, twice per side, alternating (tools/bench_tiled.py).  Event pairs around single launches")
    say("include the launch itself.")
    with torch.no_grad():
        for part, fn in (("a", part_a), ("b", part_b), ("c", part_c)):
            if part in a.parts:
                fn(say, dev)
    if out:
        out.close()


if __name__ == "__main__":
    main()
