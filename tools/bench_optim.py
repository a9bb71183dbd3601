"""Measurements of the guarded optimiser step's kernels (profiles/grad_clip.txt):

    python tools/bench_optim.py --out profiles/grad_clip.txt

On the flat fp32 buffer of the C3 model (67,254,246 parameters padded to 67,254,248 floats; kernel / bias ranges of that model), hipEvents
around each call, medians of 2 x 100 runs after 20 warm-up runs, the three sides alternating in this one process:

  * plain:    ops.adam_amsgrad_ (csrc/optim.hip adam_amsgrad_kernel<false>), what the default step launches;
  * norm:     ops.grad_norm_ = the norm pass + the control pass (two launches), with the regulariser on (g and p are read: 8 B per
              element) and off (g only: 4 B per element);
  * guarded:  ops.adam_amsgrad_ctl_ (adam_amsgrad_kernel<true>) with a clamp and a coefficient below 1.

Bytes are counted from the shapes (Adam reads p, g, m, v, vhat and writes p, m, v, vhat: 36 B per element); the rates are those bytes
over the median time, against the HBM figures of the MI355X: 8.0 TB/s (data sheet), 6.29 TB/s (a float4 copy).
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

N, NK, NB = 67_254_248, 33_626_947, 1_206
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12
LK = LB = 1e-5
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-7


def timeit(fn, warm=20, runs=100):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=N, help="elements (a multiple of 4)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim.py measures on a GPU; none is visible")
    out = open(a.out, "w") if a.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()
    dev = torch.device("cuda:0")
    n = a.n
    nk, nb = (NK, NB) if n == N else (n // 2 + 1, min(NB, n // 4))
    gen = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(n, generator=gen, device=dev)
    g = torch.randn(n, generator=gen, device=dev) * 0.01
    m, v, vh = (torch.zeros_like(p) for _ in range(3))
    lr_dev = torch.tensor([LR], device=dev)
    step = torch.ones(1, dtype=torch.int32, device=dev)
    ws = torch.empty(ops.grad_norm_ws(n), dtype=torch.uint8, device=dev)
    ctl = ops.new_step_ctl(dev)

    ops.grad_norm_(g, p, nk, nb, LK, LB, 1.0, 0.0, 0.0, True, ws, ctl)
    norm = ops.read_step_ctl(ctl)["norm"]
    want = float((g.double() + 2.0 * LK * torch.where(torch.arange(n, device=dev) < nk + nb, p, torch.zeros_like(p)).double()).square().sum().sqrt())
    cv, cn = 0.03, 0.5 * norm

    plain = lambda: ops.adam_amsgrad_(p, g, m, v, vh, nk, nb, LK, LB, 1.0, lr_dev, B1, B2, EPS, step)
    norm_l2 = lambda: ops.grad_norm_(g, p, nk, nb, LK, LB, 1.0, cv, cn, True, ws, ctl)
    norm_g = lambda: ops.grad_norm_(g, p, nk, nb, 0.0, 0.0, 1.0, cv, cn, True, ws, ctl)
    guarded = lambda: ops.adam_amsgrad_ctl_(p, g, m, v, vh, nk, nb, LK, LB, 1.0, lr_dev, B1, B2, EPS, step, cv, ctl)
    sides = {"plain": plain, "norm_l2": norm_l2, "norm_g": norm_g, "guarded": guarded}
    ts = {k: [] for k in sides}
    for _ in range(2):                                      # alternating: plain, norm (L2 on), norm (L2 off), guarded, and again
        for k, fn in sides.items():
            if k == "guarded":
                norm_l2()                                   # (the record the guarded update reads: apply = 1, coef < 1)
            ts[k].append(timeit(fn))
    ts = {k: np.concatenate(t) for k, t in ts.items()}
    rec = ops.read_step_ctl(ctl)
    med = {k: float(np.median(t)) * 1e-3 for k, t in ts.items()}         # seconds
    us = lambda t: f"median {np.median(t) * 1e3:8.1f} us   min {t.min() * 1e3:8.1f} us   p90 {np.percentile(t, 90) * 1e3:8.1f} us"
    rate = lambda b, k: f"{b / med[k] / 1e12:.2f} TB/s = {100 * b / med[k] / HBM_SPEC:.0f} % of 8.0 TB/s (data sheet), {100 * b / med[k] / HBM_COPY:.0f} % of 6.29 TB/s (float4 copy)"
    say(f"Guarded optimiser step, kernels alone, on a flat fp32 buffer of {n:,} floats (n_kernel {nk:,}, n_bias {nb:,}), one MI355X (gfx950);")
    say("hipEvents around each call, 20 warm-up + 100 timed runs, twice per side, alternating (tools/bench_optim.py).")
    say(f"norm of the regularised gradient: kernel {norm:.9g}, torch fp64 {want:.12g} (relative difference {abs(norm - want) / want:.1e}); "
        f"last record: coef {rec['coef']:.6g}, apply {rec['apply']}, skipped {rec['skipped']}")
    say(f"1) plain Adam-amsgrad (1 launch, 36 B/element = {36 * n / 1e9:.3f} GB):        {us(ts['plain'])}   {rate(36 * n, 'plain')}")
    say(f"2) guarded Adam-amsgrad (1 launch, 36 B/element, clamp + coef):       {us(ts['guarded'])}   {rate(36 * n, 'guarded')}")
    say(f"   guarded / plain = {med['guarded'] / med['plain']:.3f} (medians)")
    say(f"3) norm + control (2 launches), regulariser on, 8 B/element = {8 * n / 1e9:.3f} GB: {us(ts['norm_l2'])}   {rate(8 * n, 'norm_l2')}")
    say(f"   norm + control (2 launches), regulariser off, 4 B/element = {4 * n / 1e9:.3f} GB: {us(ts['norm_g'])}   {rate(4 * n, 'norm_g')}")
    say(f"   (norm + control) / plain Adam = {med['norm_l2'] / med['plain']:.3f} with the regulariser, {med['norm_g'] / med['plain']:.3f} without "
        f"(by bytes: {8 / 36:.3f} and {4 / 36:.3f})")
    say(f"4) the guarded step's optimiser part (norm + control + guarded Adam) / the plain one = "
        f"{(med['norm_l2'] + med['guarded']) / med['plain']:.3f} (sum of medians; the two step-counter launches are equal on both sides)")
    say("   (event pairs include the launches themselves: two for the norm side; no kernel trace was collected)")
    if out:
        out.close()


if __name__ == "__main__":
    main()
