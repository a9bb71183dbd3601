"""Measurements of the uncertainty kernels of the Monte-Carlo inference (profiles/mc_uncertainty.txt):

    python tools/bench_mc_uncertainty.py --out profiles/mc_uncertainty.txt

At the shape of tools/bench_mc.py (B = 2, 20x160x160, nc = 2, bf16 logits), n = 4 draws, one draw per pass, hipEvents around each call,
20 warm-up + 200 timed runs, twice per side, the sides alternating in one process on the same logits:

  (a) ops.mc_accum_u per pass + ops.mc_finish_u: the five maps (csrc/mc.hip);
  (b) ops.mc_accum per pass + ops.mc_finish: mean and entropy only -- the code that was there before, on the same box;
  (c) what a caller has to write without (a): ops.softmax_heads per pass into an (n, B, D, H, W, nc) tensor, as ``return_samples``
      gives it, and the five maps from it in torch element-wise ops;

and the results of (a) and (c) compared.  Also each new kernel alone against its own traffic count.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from util import ops  # noqa: E402

B, DIMS, NC, N_DRAWS = 2, (20, 160, 160), 2, 4
MAPS = ("mean", "entropy", "expected_entropy", "mutual_info", "variance")


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


def fused_u(logits):
    acc = None
    for lg in logits:
        acc = ops.mc_accum_u(lg, 1, acc)
    return ops.mc_finish_u(acc, len(logits))


def fused(logits):
    s = None
    for lg in logits:
        s = ops.mc_accum(lg, 1, s)
    return ops.mc_finish(s, len(logits))


def composed(logits):
    p = torch.stack([ops.softmax_heads([lg], [(1, 1, 1)]) for lg in logits])
    mean = p.mean(dim=0)
    ent = -torch.xlogy(mean, mean).sum(dim=-1)
    ee = -torch.xlogy(p, p).sum(dim=-1).mean(dim=0)
    return {"mean": mean, "entropy": ent, "expected_entropy": ee, "mutual_info": (ent - ee).clamp_min_(0),
            "variance": ((p * p).mean(dim=0) - mean * mean).clamp_min_(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mc_uncertainty.py measures on a GPU; none is visible")
    out = open(a.out, "w") if a.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    logits = [(torch.randn((B, *DIMS, NC), generator=g) * 2.5).to(torch.bfloat16).to(dev) for _ in range(N_DRAWS)]
    vox = B * int(np.prod(DIMS))
    with torch.no_grad():
        mu, mc = fused_u(logits), composed(logits)
        diff = {k: float((mu[k] - mc[k]).abs().max()) for k in MAPS}
        mo, ho = fused(logits)
        same = bool(torch.equal(mu["mean"], mo)) and bool(torch.equal(mu["entropy"], ho))
        ta, tb, tc = [], [], []
        for _ in range(2):                                  # alternating: (a), (b), (c), (a), (b), (c)
            ta.append(timeit(lambda: fused_u(logits)))
            tb.append(timeit(lambda: fused(logits)))
            tc.append(timeit(lambda: composed(logits)))
        ta, tb, tc = np.concatenate(ta), np.concatenate(tb), np.concatenate(tc)
        acc = ops.mc_accum_u(logits[0], 1)
        t1 = timeit(lambda: ops.mc_accum_u(logits[1], 1, acc))
        t0 = timeit(lambda: ops.mc_accum_u(logits[0], 1))
        ent, mi = torch.empty_like(acc[1]), torch.empty_like(acc[1])
        lib, st = ops.L.load(), torch.cuda.current_stream().cuda_stream

        def finish_alone():                                 # (the C entry point on fixed buffers: no allocation inside the window)
            ops.L.check(lib.m1_mc_finish_u(acc[0].data_ptr(), acc[1].data_ptr(), acc[2].data_ptr(), N_DRAWS, B, vox // B, NC,
                                           acc[0].data_ptr(), ent.data_ptr(), acc[1].data_ptr(), mi.data_ptr(), acc[2].data_ptr(), st),
                        "m1_mc_finish_u")
        tfin = timeit(finish_alone)
    med = lambda t: float(np.median(t))
    us = lambda t: f"median {med(t) * 1e3:.1f} us   min {t.min() * 1e3:.1f} us   p90 {np.percentile(t, 90) * 1e3:.1f} us"
    say(f"Uncertainty maps of the Monte-Carlo inference at B = {B}, {DIMS[0]}x{DIMS[1]}x{DIMS[2]}, nc = {NC}, bf16 logits, n = {N_DRAWS} draws, one draw per pass,")
    say("one MI355X (gfx950); hipEvents around the call, 20 warm-up + 200 timed runs, twice per side, alternating (tools/bench_mc_uncertainty.py).")
    say(f"1) (a) {N_DRAWS} x mc_accum_u + mc_finish_u, five maps, {N_DRAWS + 1} launches:            {us(ta)}")
    say(f"   (b) {N_DRAWS} x mc_accum + mc_finish, mean and entropy, {N_DRAWS + 1} launches:         {us(tb)}")
    say(f"   (c) {N_DRAWS} x softmax_heads, stack, five maps in torch element-wise ops:   {us(tc)}")
    el = vox * NC
    b_first, b_acc = el * 2 + (2 * el + vox) * 4, el * 2 + (2 * el + vox) * 4 * 2
    b_fin = (2 * el + vox) * 4 + (2 * el + 3 * vox) * 4
    o_first, o_acc, o_fin = el * (2 + 4), el * (2 + 4 + 4), vox * (2 * NC + 1) * 4
    bytes_a, bytes_b = b_first + (N_DRAWS - 1) * b_acc + b_fin, o_first + (N_DRAWS - 1) * o_acc + o_fin
    say(f"   (a) / (b) = {med(ta) / med(tb):.3f} (medians) for {bytes_a / 1e6:.1f} MB / {bytes_b / 1e6:.1f} MB = {bytes_a / bytes_b:.3f} of the bytes; "
        f"(a) - (b) = {(med(ta) - med(tb)) * 1e3:.1f} us, p90 - median of (b) = {(np.percentile(tb, 90) - med(tb)) * 1e3:.1f} us")
    say(f"   (a) / (c) = {med(ta) / med(tc):.3f} (medians); mean and entropy of (a) equal (b)'s bit for bit: {same}")
    say("   largest difference (a) - (c): " + ", ".join(f"{k} {v:.3g}" for k, v in diff.items()))
    say("2) each new kernel alone, its own traffic (logits read, accumulators written [+ read]; sums read, five maps written):")
    say(f"   mc_accum_u first pass (write):      {b_first / 1e6:.2f} MB   {us(t0)}   {b_first / med(t0) / 1e6:.0f} GB/s at the median (includes the allocation of the accumulators)")
    say(f"   mc_accum_u later pass (accumulate): {b_acc / 1e6:.2f} MB   {us(t1)}   {b_acc / med(t1) / 1e6:.0f} GB/s at the median")
    say(f"   mc_finish_u:                        {b_fin / 1e6:.2f} MB   {us(tfin)}   {b_fin / med(tfin) / 1e6:.0f} GB/s at the median")
    say("   (event pairs around single launches of a few microseconds include the launch itself; no kernel trace was collected)")
    if out:
        out.close()


if __name__ == "__main__":
    main()
