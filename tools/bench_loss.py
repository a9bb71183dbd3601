"""Focal.loss vs SoftDicePlusBoundarySurface.loss, forward + backward, at the bench shape (2,20,160,160), nc = 2, with 1 and 4
heads: hipEvent time per call, the two losses alternating call by call after a warm-up.

    python tools/bench_loss.py [--iters 200] [--warmup 20] [--out FILE.json]

Run it once more under `rocprofv3 --kernel-trace --stats` (fewer iterations) for the per-kernel split."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from util import PKG

LS = PKG.losses


def problem(nheads, dev, shape=(2, 20, 160, 160), nc=2, seed=0):
    """Softmax heads of random logits and the one-hot label of a radius-6 ball per sample (the trainer's synthetic lesion)."""
    g = np.random.default_rng(seed)
    zz, yy, xx = np.meshgrid(*(np.arange(s) for s in shape[1:]), indexing="ij")
    lbl = np.zeros(shape, np.int64)
    for n in range(shape[0]):
        c = [g.integers(1, shape[1] - 1), g.integers(6, shape[2] - 6), g.integers(6, shape[3] - 6)]
        lbl[n][((zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2) <= 36] = 1
    y = torch.from_numpy(np.stack([(lbl == k) for k in range(nc)], -1).astype(np.float32)).to(dev)
    logits = torch.from_numpy(g.standard_normal(shape + (nheads, nc)).astype(np.float32)).to(dev)
    p = torch.softmax(logits, -1).reshape(shape + (nheads * nc,)).contiguous()
    return y, p.requires_grad_(True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss needs a GPU")
    dev = torch.device("cuda:0")
    fns = {"focal": LS.Focal(alpha=[1.0, 1.0], gamma=2.0).loss,
           "dice_boundary": LS.SoftDicePlusBoundarySurface(loss_weights=[0.5, 0.5]).loss}
    rows = []
    for nheads in (1, 4):
        y, p = problem(nheads, dev)

        def call(fn):
            p.grad = None
            fn(y, p).backward()
        for _ in range(a.warmup):
            for fn in fns.values():
                call(fn)
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(a.iters):
            for k, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); call(fn); e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1))
        for k, t in times.items():
            t = np.array(t) * 1e3
            r = {"loss": k, "shape": [2, 20, 160, 160], "nc": 2, "nheads": nheads, "iters": a.iters,
                 "fwd_bwd_us_median": round(float(np.median(t)), 1), "p10_us": round(float(np.percentile(t, 10)), 1),
                 "p90_us": round(float(np.percentile(t, 90)), 1)}
            rows.append(r)
            print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
