"""Measurements of the bootstrap replicates (profiles/bootstrap.txt):

    python tools/bench_bootstrap.py --out profiles/bootstrap.txt

(a) the kernel.  ops.bootstrap_metrics (csrc/bootstrap.hip, one launch, one workgroup per replicate) on resident tables: N = 1000
    cases with about 3 events per case and three value columns, n_boot = 1000 and 10000, plain and stratified; N = 16384 (the LDS cap)
    at n_boot = 1000.  hipEvents around each call, 20 warm-up + 100 timed runs (10 + 30 at n_boot = 10000).  Reported: the median kernel
    time by event pairs (they include the launch itself), replicates per second, the bytes a replicate reads (from the shapes: every
    table array once) and the LDS-implied residency: blocks per CU = min(8, floor(160 KiB / (4 N + static bytes))) against the 4 the
    kernel's 114 VGPRs allow at 256 threads (waves per SIMD = blocks per CU).
(b) the same table on the host: ``bootstrap.replicates_host`` (numpy, the weighted formulation) and the explicit-resample oracle loop of
    tests/bootstrap_ref.py (``detection.auroc`` / ``froc`` / ``average_precision`` / ``sens_at`` per replicate), wall clock of 200 and 50
    replicates, scaled per replicate; the ratios against the kernel's time per replicate at n_boot = 1000.
(c) the added cost in validation.validate(): one batch of two cases on the README model (as tools/bench_validation.py part b), one
    draw, bootstrap off and 1000; wall clock around a device synchronisation, medians of 5 runs after 2.
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bootstrap_ref as R  # noqa: E402
from util import PKG, ops  # noqa: E402

T = importlib.import_module("prostatemr_3d-cad-cspca_amd.train_model")
B, V = PKG.bootstrap, PKG.validation
DIMS = (20, 160, 160)
STATIC_LDS, LDS_PER_CU, VGPR_BLOCKS = 1472, 160 * 1024, 4


def timeit(fn, warm, runs):
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


def table_of(N, seed=1):
    cases = R.cases_with(N, 3 * N, seed)
    return cases, B.pack(cases, values=R.value_columns(N, 3, seed))


def part_a(say, dev):
    say("(a) ops.bootstrap_metrics on resident tables, about 3 events per case, 3 value columns, 3 false-positive rates")
    per_rep = {}
    for N, boots in ((1000, (1000, 10000)), (16384, (1000,))):
        cases, t = table_of(N)
        td = B.to_device(t, dev)["dev"]
        nbytes = 6 * t["N"] + 6 * t["M"] + 8 * t["N"] * t["V"] + 4 * t["N"]
        lds = 4 * N + STATIC_LDS
        blocks = min(8, LDS_PER_CU // lds)
        say(f"  N = {N}, M = {t['M']}, V = {t['V']}: {nbytes} bytes read per replicate (L2 resident); LDS {lds} bytes per block -> "
            f"{blocks} blocks per CU by LDS, {min(blocks, VGPR_BLOCKS)} with the VGPR limit of {VGPR_BLOCKS} = "
            f"{min(blocks, VGPR_BLOCKS)} of 8 waves per SIMD")
        for nb in boots:
            for strat in (False, True):
                out = torch.empty((nb, len(B.columns(t))), dtype=torch.float64, device=dev)
                fn = lambda: ops.bootstrap_metrics(td, nb, 7, strat, t["fp_rates"], out=out)      # noqa: E731
                ts = timeit(fn, 20 if nb <= 1000 else 10, 100 if nb <= 1000 else 30)
                med = float(np.median(ts)) * 1e-3
                per_rep[(N, nb, strat)] = med / nb
                say(f"    n_boot {nb:6d} {'stratified' if strat else 'plain     '}: median {med * 1e6:9.1f} us   min {ts.min() * 1e3:9.1f} us   "
                    f"p90 {np.percentile(ts, 90) * 1e3:9.1f} us   {nb / med:12.0f} replicates/s   {nbytes * nb / med / 1e9:8.1f} GB/s of table reads")
    return per_rep


def part_b(say, per_rep):
    cases, t = table_of(1000)
    vals = R.value_columns(1000, 3, 1)
    say("(b) the same N = 1000 table on the host, wall clock per replicate:")
    t0 = time.perf_counter()
    B.replicates_host(t, 200, 7)
    host = (time.perf_counter() - t0) / 200
    t0 = time.perf_counter()
    R.replicates(cases, 50, 7, values=vals)
    oracle = (time.perf_counter() - t0) / 50
    k = per_rep[(1000, 1000, False)]
    say(f"    kernel (n_boot 1000)      {k * 1e6:10.3f} us per replicate")
    say(f"    bootstrap.replicates_host {host * 1e6:10.1f} us per replicate = {host / k:8.0f} times the kernel")
    say(f"    explicit-resample oracle  {oracle * 1e6:10.1f} us per replicate = {oracle / k:8.0f} times the kernel")


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
    rng = np.random.default_rng(3)
    xs, ys = zip(*[T.synthetic_case(rng, DIMS, 3, 2) for _ in range(2)])
    batch = [({"image": torch.from_numpy(np.stack(xs)).to(dev)}, {"detection": torch.from_numpy(np.stack(ys)).to(torch.uint8).to(dev)})]
    say("(c) validation.validate() of one batch of two cases on the README model (C3, (20,160,160), bf16, untrained weights), one draw,")
    say("    wall clock per VALIDATION in ms (medians of 5 runs after 2): pack + one launch + one read of 1000 x 5 doubles + percentiles")
    t_off = wall(lambda: V.validate(model, batch, 1, "lesion", n_draws=1))
    t_on = wall(lambda: V.validate(model, batch, 1, "lesion", n_draws=1, bootstrap=1000))
    say(f"    validate {t_off:8.2f}   with bootstrap=1000 {t_on:8.2f}   added {t_on - t_off:+7.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-model", action="store_true", help="parts (a) and (b) only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bootstrap.py measures on a GPU; none is visible")
    out = open(a.out, "w") if a.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()
    dev = torch.device("cuda:0")
    say("Bootstrap replicates on one MI355X (gfx950), tools/bench_bootstrap.py.")
    with torch.no_grad():
        per_rep = part_a(say, dev)
    part_b(say, per_rep)
    if not a.skip_model:
        part_c(say, dev)
    if out:
        out.close()


if __name__ == "__main__":
    main()
