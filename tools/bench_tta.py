"""Measurements of the test-time-augmentation kernels (profiles/tta.txt):

    python tools/bench_tta.py --out profiles/tta.txt

On resident (2, 20, 160, 160, nc) data, fp32 and bf16, nc 2 and 3, hipEvents around each call, 20 warm-up + 200 timed runs, twice per
side, the sides alternating in one process on the same tensors:

  (a) ops.mc_accum_v with R = 2, masks (0, 1), and R = 8, all eight masks, accumulating into existing sums, with and without the
      uncertainty sums, against
        plain: ops.mc_accum[_u] on the same logits -- the same bytes, so the ratio is what the mirrored addressing costs;
        flips: what a caller writes without it -- torch.flip per replica, torch.cat, then ops.mc_accum[_u];
      and the sums of the fused call compared with those of the flips bit for bit;
  (b) ops.tta_views against torch.cat of torch.flip's of the input, (2, 20, 160, 160, 3);
  (c) predict_mc(x, 1, draws_per_pass=2, tta=("", "w")) on the README model (C3 of bench.py, bf16) against two predict calls with
      torch flips and a torch average (3 warm-up + 10 timed runs, twice per side, alternating).
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

B, DIMS = 2, (20, 160, 160)


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


def flip(t, mask):
    dims = [ax for bit, ax in ((1, 3), (2, 2), (4, 1)) if mask & bit]
    return torch.flip(t, dims) if dims else t


def unmirror(lg, views):
    return torch.cat([flip(lg[r * B:(r + 1) * B], m) for r, m in enumerate(views)])


med = lambda t: float(np.median(t))                                                  # noqa: E731
us = lambda t: f"median {med(t) * 1e3:7.1f} us  min {t.min() * 1e3:7.1f} us  p90 {np.percentile(t, 90) * 1e3:7.1f} us"   # noqa: E731


def part_a(say, dev):
    say("(a) mc_accum_v (accumulating call) against plain mc_accum[_u] on the same logits and against torch.flip per replica + cat +")
    say("    mc_accum[_u]; bytes = logits read + sums read and written (the count of the kernels' profiler scope)")
    g = torch.Generator().manual_seed(0)
    vox = B * int(np.prod(DIMS))
    for dtype, nc, (R, views), unc in itertools.product((torch.float32, torch.bfloat16), (2, 3), ((2, (0, 1)), (8, tuple(range(8)))),
                                                        (False, True)):
        lg = (torch.randn((R * B, *DIMS, nc), generator=g) * 2.5).to(dtype).to(dev)
        plain = ops.mc_accum_u if unc else ops.mc_accum
        accs = {k: plain(lg, R) for k in ("fused", "plain", "flips")}
        want = plain(unmirror(lg, views), R)
        got = ops.mc_accum_v(lg, R, views, uncertainty=unc)
        tup = lambda a: a if isinstance(a, tuple) else (a,)                          # noqa: E731
        same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(tup(got), tup(want)))
        t = alternate({"fused": lambda: ops.mc_accum_v(lg, R, views, accs["fused"], uncertainty=unc),
                       "plain": lambda: plain(lg, R, accs["plain"]),
                       "flips": lambda: plain(unmirror(lg, views), R, accs["flips"])})
        el = vox * nc
        nbytes = el * R * lg.element_size() + ((2 * el + vox) if unc else el) * 4 * 2
        name = f"{str(dtype).replace('torch.', ''):8s} nc={nc} R={R} {'mc_accum_u' if unc else 'mc_accum  '}"
        say(f"  {name} {nbytes / 1e6:6.1f} MB  bits equal to flips + plain: {same}")
        say(f"      fused  {us(t['fused'])}  {nbytes / med(t['fused']) / 1e9:6.3f} TB/s at the median")
        say(f"      plain  {us(t['plain'])}  {nbytes / med(t['plain']) / 1e9:6.3f} TB/s at the median")
        say(f"      flips  {us(t['flips'])}")
        say(f"      fused / plain = {med(t['fused']) / med(t['plain']):.3f}   fused / flips = {med(t['fused']) / med(t['flips']):.3f}  (medians)")


def part_b(say, dev):
    say("(b) tta_views against torch.cat of torch.flip's, x (2, 20, 160, 160, 3); bytes = x read once + R views written")
    g = torch.Generator().manual_seed(1)
    for dtype, views in itertools.product((torch.float32, torch.bfloat16), ((0, 1), tuple(range(8)))):
        x = torch.randn((B, *DIMS, 3), generator=g).to(dtype).to(dev)
        same = bool(torch.equal(ops.tta_views(x, views), torch.cat([flip(x, m) for m in views])))
        t = alternate({"kernel": lambda: ops.tta_views(x, views), "torch": lambda: torch.cat([flip(x, m) for m in views])})
        nbytes = x.numel() * x.element_size() * (1 + len(views))
        say(f"  {str(dtype).replace('torch.', ''):8s} R={len(views)} {nbytes / 1e6:6.1f} MB  equal: {same}")
        say(f"      tta_views  {us(t['kernel'])}  {nbytes / med(t['kernel']) / 1e9:6.3f} TB/s at the median")
        say(f"      cat(flips) {us(t['torch'])}")
        say(f"      tta_views / cat(flips) = {med(t['kernel']) / med(t['torch']):.3f}  (medians)")


def part_c(say, dev):
    PKG.unets.network_blocks.set_init_seed(0)
    init = PKG.initializers
    model = PKG.unets.networks.M1(
        input_spatial_dims=DIMS, input_channels=3, num_classes=2, filters=(32, 64, 128, 256, 512),
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
    x = torch.randn((B, *DIMS, 3), generator=torch.Generator().manual_seed(3)).to(dev)

    def fused():
        return dm.predict_mc(x, 1, draws_per_pass=2, tta=("", "w"))["mean"]

    def by_hand():
        p = dm.predict(x)
        model.advance_rng()
        q = torch.flip(dm.predict(torch.flip(x, [3])), [3])
        model.advance_rng()
        return (p + q) / 2
    t = alternate({"fused": fused, "by hand": by_hand}, warm=3, runs=10)
    say("(c) one prediction with tta=('', 'w') on the README model (C3: probabilistic, dense skip, deep supervision, filters 32..512,")
    say("    (2, 20, 160, 160, 3), bf16, untrained weights), hipEvents around the whole call, 3 warm-up + 10 timed runs, twice, alternating")
    say(f"      predict_mc(x, 1, draws_per_pass=2, tta=('', 'w')): one pass of 4 samples      {us(t['fused'])}")
    say(f"      two predict calls (2 samples each), torch.flip in and out, torch average:   {us(t['by hand'])}")
    say(f"      fused / by hand = {med(t['fused']) / med(t['by hand']):.3f}  (medians; the by-hand side has no entropy)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parts", default="abc")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tta.py measures on a GPU; none is visible")
    out = open(a.out, "w") if a.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()
    dev = torch.device("cuda:0")
    say("Test-time augmentation by mirroring at B = 2, 20x160x160, one MI355X (gfx950); hipEvents around each call, 20 warm-up + 200 timed")
    say("runs, twice per side, alternating (tools/bench_tta.py).  Event pairs around single launches include the launch itself.")
    with torch.no_grad():
        for part, fn in (("a", part_a), ("b", part_b), ("c", part_c)):
            if part in a.parts:
                fn(say, dev)
    if out:
        out.close()


if __name__ == "__main__":
    main()
