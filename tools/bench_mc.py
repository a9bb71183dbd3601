"""Measurements of the Monte-Carlo inference kernels (profiles/mc_inference.txt):

    python tools/bench_mc.py --out profiles/mc_inference.txt

At the bench shape (B = 2, 20x160x160, nc = 2, bf16 logits), n = 4 draws, one draw per pass, hipEvents around each call, median of 200:

  * fused: ops.mc_accum per pass + ops.mc_finish (csrc/mc.hip);
  * composed: what a caller has to write without them -- ops.softmax_heads per pass, torch add_ into an accumulator, a division,
    the entropy in torch element-wise ops (clamp-free 0 ln 0 = 0 through torch.xlogy);

both in this process on the same logits, alternating, and the two results compared.  Also the accumulate kernel alone against its own
traffic count (logits read, accumulator read + written).
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


def fused(logits):
    s = None
    for lg in logits:
        s = ops.mc_accum(lg, 1, s)
    return ops.mc_finish(s, len(logits))


def composed(logits):
    s = None
    for lg in logits:
        p = ops.softmax_heads([lg], [(1, 1, 1)])
        s = p if s is None else s.add_(p)
    mean = s.div_(float(len(logits)))
    return mean, -torch.xlogy(mean, mean).sum(dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mc.py measures on a GPU; none is visible")
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
        mf, hf = fused(logits)
        mc, hc = composed(logits)
        dm, dh = float((mf - mc).abs().max()), float((hf - hc).abs().max())
        tf, tc = [], []
        for _ in range(2):                                  # alternating: fused, composed, fused, composed
            tf.append(timeit(lambda: fused(logits)))
            tc.append(timeit(lambda: composed(logits)))
        tf, tc = np.concatenate(tf), np.concatenate(tc)
        acc = torch.empty((B, *DIMS, NC), dtype=torch.float32, device=dev)
        ops.mc_accum(logits[0], 1, acc)
        t1 = timeit(lambda: ops.mc_accum(logits[1], 1, acc))
        t0 = timeit(lambda: ops.mc_accum(logits[0], 1))
        tfin = timeit(lambda: ops.mc_finish(acc, N_DRAWS))
    us = lambda t: f"median {np.median(t) * 1e3:.1f} us   min {t.min() * 1e3:.1f} us   p90 {np.percentile(t, 90) * 1e3:.1f} us"
    say(f"Monte-Carlo inference kernels at B = {B}, {DIMS[0]}x{DIMS[1]}x{DIMS[2]}, nc = {NC}, bf16 logits, n = {N_DRAWS} draws, one draw per pass, one MI355X")
    say("(gfx950); hipEvents around the call, 20 warm-up + 200 timed runs, twice per side, alternating (tools/bench_mc.py).")
    say(f"1) fused    ({N_DRAWS} x mc_accum + mc_finish, {N_DRAWS + 1} launches):                                  {us(tf)}")
    say(f"   composed ({N_DRAWS} x softmax_heads, {N_DRAWS - 1} x add_, div_, xlogy, sum, neg: {2 * N_DRAWS + 3} launches):  {us(tc)}")
    say(f"   fused / composed = {np.median(tf) / np.median(tc):.3f} (medians); largest difference of the results: mean {dm:.3g}, entropy {dh:.3g}")
    b_first = vox * NC * (2 + 4)
    b_acc = vox * NC * (2 + 4 + 4)
    b_fin = vox * (2 * NC + 1) * 4
    say(f"2) mc_accum alone, its own traffic (logits read + accumulator written [+ read]):")
    say(f"   first pass (write):      {b_first / 1e6:.2f} MB   {us(t0)}   {b_first / np.median(t0) / 1e6:.0f} GB/s at the median (includes the allocation of the accumulator)")
    say(f"   later pass (accumulate): {b_acc / 1e6:.2f} MB   {us(t1)}   {b_acc / np.median(t1) / 1e6:.0f} GB/s at the median")
    say(f"   mc_finish:               {b_fin / 1e6:.2f} MB   {us(tfin)}   {b_fin / np.median(tfin) / 1e6:.0f} GB/s at the median")
    say("   (event pairs around single launches of a few microseconds include the launch itself; no kernel trace was collected)")
    if out:
        out.close()


if __name__ == "__main__":
    main()
