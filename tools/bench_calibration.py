"""Measurements of the calibration record (profiles/calibration.txt):

    python tools/bench_calibration.py --out profiles/calibration.txt

(a) the kernel.  ops.cal_score (csrc/calibrate.hip, two launches: zero fill + scoring) on resident (2,20,160,160,K) probabilities,
    K = 2 and 3, fp32 and bf16, 15 bins, uint8 labels, with and without an uncertainty map, on two contents:
      detection  a detection map: > 99 % of the voxels at conf > 0.93 (nearly every lane of a wave in the top bin)
      uniform    uniform random probabilities (the bins change from voxel to voxel)
    against a torch composition that leaves the SAME integer record on the device without a host read: isnan / argmax / floor for
    the bins, one int64 scatter_add per histogram column, squared error, fp64 log.  It exists only here (the project never had one);
    the two sides are compared slot by slot before they are timed (nll within one unit per voxel).  hipEvents around each call, 20
    warm-up + 100 timed runs, twice per side, alternating, in this one process.  Bytes are counted from the shapes (every input is
    read once) over the median time, next to a float4 copy of the same number of bytes measured here (read + written bytes / time)
    and the 6.29 TB/s tools/bench_optim.py reports for large buffers.  Launches per side: torch.profiler device events.
(b) the added cost in validation.validate(): one batch of two cases on the README model (as tools/bench_validation.py part b),
    n_draws 1 and 8, calibration off and on; wall clock around a device synchronisation, medians of 5 runs after 2.
"""
import argparse
import importlib
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from util import PKG, ops  # noqa: E402

T = importlib.import_module("prostatemr_3d-cad-cspca_amd.train_model")
V = PKG.validation
HBM_COPY = 6.29e12
DIMS = (20, 160, 160)
BINS = 15
FX = float(2 ** 32)


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


def wall(fn, warm=2, runs=5):
    ts = []
    for i in range(warm + runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return str(n) if n else "n/a"
    except Exception as exc:  # noqa: BLE001 -- the count is a side note of the measurement
        return f"n/a ({type(exc).__name__})"


def composition(p, label, unc, M, u_scale):
    """The record of ops.cal_score from torch calls, left on the device as (B, slots) int64 (no host read, no boolean indexing)."""
    B, K = p.shape[0], p.shape[-1]
    slots = ops.cal_record_slots(K, M)

    def fx(v):
        return (v.double().clamp_min(0) * FX).floor().long()

    def bins(v, factor):
        return (v * factor).clamp(0, M).long().clamp_max(M - 1)

    def hist(row, h, b, ok, sums, hits):
        base = 8 + 3 * M * h
        row[base:base + M].scatter_add_(0, b, ok)
        row[base + M:base + 2 * M].scatter_add_(0, b, sums * ok)
        row[base + 2 * M:base + 3 * M].scatter_add_(0, b, hits.long() * ok)

    def run():
        out = torch.zeros((B, slots), dtype=torch.int64, device=p.device)
        pf = p.float().flatten(1, -2)
        y = label.flatten(1).long()
        for b in range(B):
            pb, yb = pf[b], y[b]
            nan = torch.isnan(pb).any(-1)
            ub = None
            if unc is not None:
                ub = unc[b].flatten()
                nan = nan | torch.isnan(ub)
            ign = yb >= K
            valid = ~nan & ~ign
            ok = valid.long()
            row = out[b]
            row[0], row[1], row[2] = ok.sum(), nan.sum(), (~nan & ign).sum()
            pz = torch.where(valid[:, None], pb, torch.zeros_like(pb))
            yz = torch.where(valid, yb, torch.zeros_like(yb))
            conf, am = pz.max(-1)
            hist(row, 0, bins(conf, float(M)), ok, fx(conf), am == yz)
            for c in range(K):
                hist(row, 1 + c, bins(pz[:, c], float(M)), ok, fx(pz[:, c]), yz == c)
                d = pz[:, c].double() - (yz == c).double()
                row[4 + c] = (fx(d * d) * ok).sum()
            py = pz.gather(1, yz[:, None])[:, 0].clamp_min(1e-7).double()
            row[3] = (fx(-torch.log(py)) * ok).sum()
            if ub is not None:
                uz = torch.where(valid, ub, torch.zeros_like(ub))
                hist(row, K + 1, bins(uz, u_scale), ok, fx(uz), am != yz)
        return out
    return run


def contents(K, kind, gen):
    shape = (2, *DIMS, K)
    if kind == "uniform":
        p = torch.rand(shape, generator=gen) + 1e-3
        p = p / p.sum(-1, keepdim=True)
    else:
        fg = torch.rand(shape[:-1], generator=gen) < 0.005                  # blobs of graded confidence on a background at ~ 1
        rest = torch.where(fg, torch.rand(shape[:-1], generator=gen), torch.full(shape[:-1], 1e-3) * torch.rand(shape[:-1], generator=gen))
        p = torch.empty(shape)
        p[..., 0] = 1 - rest
        for c in range(1, K):
            p[..., c] = rest / (K - 1)
    label = (torch.rand(shape[:-1], generator=gen) < (0.5 if kind == "uniform" else 0.004)).to(torch.uint8)
    unc = -(p * torch.log(p.clamp_min(1e-30))).sum(-1)
    return p, label, unc


def copy_rate(nbytes, dev):
    n = max(nbytes // 16 * 4, 4)
    src, dst = torch.rand(n, device=dev), torch.empty(n, device=dev)
    t = float(np.median(timeit(lambda: dst.copy_(src)))) * 1e-3
    return 2 * 4 * n / t, t


def part_a(say, dev):
    say(f"(a) ops.cal_score vs a torch composition of the same record; B = 2 cases of {DIMS}, {BINS} bins, uint8 labels, no mask")
    us = lambda t: f"median {np.median(t) * 1e3:8.1f} us   min {t.min() * 1e3:8.1f} us   p90 {np.percentile(t, 90) * 1e3:8.1f} us"   # noqa: E731
    med_of = {}
    for K in (2, 3):
        for dt in (torch.float32, torch.bfloat16):
            for with_unc in (True, False):
                for kind in ("detection", "uniform"):
                    gen = torch.Generator().manual_seed(10 * K + (kind == "uniform"))
                    p, label, unc = contents(K, kind, gen)
                    p, label = p.to(dev).to(dt), label.to(dev)
                    unc = unc.to(dev) if with_unc else None
                    u_max = math.log(K)
                    nvox = label.numel() // 2
                    out = torch.empty((2, ops.cal_record_slots(K, BINS)), dtype=torch.int64, device=dev)
                    kernel = lambda: ops.cal_score(p, label, BINS, None, unc, u_max if with_unc else None, out=out)      # noqa: E731
                    comp = composition(p, label, unc, BINS, float(PKG.calibration.u_scale(BINS, u_max)))
                    a, b = kernel().clone(), comp()
                    diff = (a != b)
                    diff[:, 3] = (a[:, 3] - b[:, 3]).abs() > a[:, 0]        # nll: the two fp64 logs, one unit per voxel
                    agree = "records agree" if not bool(diff.any()) else f"RECORDS DIFFER in {int(diff.sum())} slots"
                    conf = p.float().amax(-1)
                    share = float((conf > 0.93).float().mean())
                    sides = {"kernel": kernel, "composition": comp}
                    ts = {k: [] for k in sides}
                    for _ in range(2):
                        for k, fn in sides.items():
                            ts[k].append(timeit(fn))
                    ts = {k: np.concatenate(t) for k, t in ts.items()}
                    nb = 2 * nvox * (K * p.element_size() + 1 + (4 if with_unc else 0))
                    med = {k: float(np.median(t)) * 1e-3 for k, t in ts.items()}
                    rate, tcopy = copy_rate(nb, dev)
                    name = "fp32" if dt == torch.float32 else "bf16"
                    med_of[(K, name, with_unc, kind)] = med["kernel"]
                    say(f"  K = {K} {name} {'with' if with_unc else 'no  '} unc, {kind:9s}: {nb / 1e6:6.2f} MB read once; "
                        f"{100 * share:5.1f} % of the voxels at conf > 0.93; {agree}")
                    say(f"    ops.cal_score   launches {launches(kernel):>4}   {us(ts['kernel'])}   {nb / med['kernel'] / 1e12:.3f} TB/s = "
                        f"{100 * nb / med['kernel'] / HBM_COPY:.1f} % of 6.29 TB/s; a float4 copy of {nb / 2e6:.2f} MB in + out here: "
                        f"{tcopy * 1e6:.1f} us = {rate / 1e12:.3f} TB/s")
                    say(f"    composition     launches {launches(comp):>4}   {us(ts['composition'])}")
                    say(f"    composition / kernel = {med['composition'] / med['kernel']:.2f} (medians; event pairs include the launches themselves)")
    say("  detection / uniform, medians of ops.cal_score (the contention case against the flush-per-voxel case):")
    for (K, name, with_unc, kind), t in med_of.items():
        if kind == "detection":
            say(f"    K = {K} {name} {'with' if with_unc else 'no  '} unc: {t / med_of[(K, name, with_unc, 'uniform')]:.2f}")


def part_b(say, dev):
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
    rng = np.random.default_rng(3)
    xs, ys = zip(*[T.synthetic_case(rng, DIMS, 3, 2) for _ in range(2)])
    bx = {"image": torch.from_numpy(np.stack(xs)).to(dev)}
    y = torch.from_numpy(np.stack(ys)).to(torch.uint8).to(dev)
    batch = [(bx, {"detection": y})]
    say("(b) validation.validate() of one batch of two cases on the README model (C3, (20,160,160), bf16, untrained weights), wall clock")
    say("    per CASE in ms (medians of 5 runs after 2), calibration off / on:")
    for n in (1, 8):
        t_off = wall(lambda: V.validate(model, batch, 1, "lesion", n_draws=n)) / 2
        t_on = wall(lambda: V.validate(model, batch, 1, "lesion", n_draws=n, calibration=True, bins=BINS)) / 2
        say(f"    n_draws {n}: validate {t_off:8.2f}   with calibration {t_on:8.2f}   added {t_on - t_off:+7.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-model", action="store_true", help="part (a) only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_calibration.py measures on a GPU; none is visible")
    out = open(a.out, "w") if a.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()
    dev = torch.device("cuda:0")
    say("Calibration record on one MI355X (gfx950), tools/bench_calibration.py.")
    with torch.no_grad():
        part_a(say, dev)
    if not a.skip_model:
        part_b(say, dev)
    if out:
        out.close()


if __name__ == "__main__":
    main()
