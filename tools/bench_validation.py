"""Measurements of train-time validation (profiles/validation.txt):

    python tools/bench_validation.py --out profiles/validation.txt

(a) the scoring kernel.  ops.val_score (csrc/validate.hip, two launches) on (2,20,160,160,2) and (2,20,160,160,3) fp32 probabilities
    with uint8 labels and an entropy map, against the composition of existing calls that yields the same per-case numbers on the
    device: losses.Focal.FL per case, detection.dice_3d per case and class, two argmax passes and the masked sums / maxima as torch
    expressions.  hipEvents around each call, 20 warm-up + 100 timed runs, twice per side, alternating, in this one process.  Bytes
    are counted from the shapes (p, y and the entropy are read once) over the median time, next to the float4-copy figure
    tools/bench_optim.py uses (6.29 TB/s).  Launches per side: counted once with torch.profiler (device kernel events), 'n/a' when the
    profiler is not usable.
(b) a whole validation.validate() pass of one batch of two cases on the README model (C3 of bench.py: hierarchical probabilistic,
    dense skip, deep supervision, filters 32..512, (20,160,160), bf16), n_draws 1 and 8, and its three parts on the same data:
    inference (predict / predict_mc), scoring (ops.val_score), candidates + matching (detection.extract_lesion_candidates +
    evaluate_case per case).  Wall clock around a device synchronisation (the parts read the device back, as validate does); medians
    of 5 runs after 2 warm-up runs.
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
from util import PKG, ops  # noqa: E402

T = importlib.import_module("prostatemr_3d-cad-cspca_amd.train_model")
V, D = PKG.validation, PKG.detection
HBM_COPY = 6.29e12
DIMS = (20, 160, 160)
ALPHA = {2: (0.25, 0.75), 3: (0.75, 0.25, 0.5)}
GAMMA = 2.0


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


def composition(p, y, ent, K):
    """The per-case numbers of the record from existing calls, left on the device (no host read on either side)."""
    focal = PKG.losses.Focal(alpha=list(ALPHA[K]), gamma=GAMMA)
    B = p.shape[0]

    def run():
        yf = y.float()
        out = []
        for b in range(B):
            out.append(focal.FL(yf[b:b + 1], p[b:b + 1]))
            for c in range(K):
                out.append(D.dice_3d(p[b, ..., c], y[b, ..., c]))
        pred, true = p.argmax(dim=-1), y.argmax(dim=-1)
        fg = true >= 1
        out += [ent.flatten(1).sum(1), (ent * fg).flatten(1).sum(1), fg.flatten(1).sum(1)]
        for c in range(K):
            pc, tc = pred == c, true == c
            out += [pc.flatten(1).sum(1), tc.flatten(1).sum(1), (pc & tc).flatten(1).sum(1), p[..., c].flatten(1).amax(1)]
        return out
    return run


def part_a(say, dev):
    say("(a) scoring kernel vs the composition of existing calls; B = 2 cases of (20,160,160), uint8 labels, entropy map given")
    for K in (2, 3):
        shape = (2, *DIMS, K)
        g = torch.Generator().manual_seed(K)
        p = torch.softmax(3.0 * torch.randn(shape, generator=g), dim=-1)
        y = torch.nn.functional.one_hot(torch.randint(0, K, shape[:-1], generator=g), K).to(torch.uint8)
        ent = -(p * torch.log(p)).sum(dim=-1)
        p, y, ent = p.to(dev), y.to(dev), ent.to(dev)
        nvox = p.numel() // (2 * K)
        ws = torch.empty(ops.val_score_ws(2, nvox, K), dtype=torch.uint8, device=dev)
        kernel = lambda: ops.val_score(p, y, ent, ALPHA[K], GAMMA, ws=ws)                  # noqa: E731
        comp = composition(p, y, ent, K)
        # the two sides agree before they are timed
        rec = ops.read_val_records(kernel(), K)
        c = [float(v.double().sum()) for v in comp()]
        fl = (c[0] + c[1 + K]) / 2
        mean_focal = sum(r["focal"] for r in rec) / 2
        sides = {"kernel": kernel, "composition": comp}
        ts = {k: [] for k in sides}
        for _ in range(2):
            for k, fn in sides.items():
                ts[k].append(timeit(fn))
        ts = {k: np.concatenate(t) for k, t in ts.items()}
        nb = 2 * nvox * (4 * K + K + 4)
        med = {k: float(np.median(t)) * 1e-3 for k, t in ts.items()}
        us = lambda t: f"median {np.median(t) * 1e3:8.1f} us   min {t.min() * 1e3:8.1f} us   p90 {np.percentile(t, 90) * 1e3:8.1f} us"   # noqa: E731
        say(f"  K = {K}: p {tuple(shape)} fp32, {nb / 1e6:.2f} MB read once per call; mean focal: kernel {mean_focal:.9g}, Focal.FL per case {fl:.9g}")
        say(f"    ops.val_score   launches {launches(kernel):>4}   {us(ts['kernel'])}   {nb / med['kernel'] / 1e12:.3f} TB/s = "
            f"{100 * nb / med['kernel'] / HBM_COPY:.1f} % of 6.29 TB/s (float4 copy)")
        say(f"    composition     launches {launches(comp):>4}   {us(ts['composition'])}")
        say(f"    composition / kernel = {med['composition'] / med['kernel']:.2f} (medians; event pairs include the launches themselves)")


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
    dm = model.get_detect_model()
    a = ALPHA[2]
    say("(b) validation.validate() of one batch of two cases on the README model (C3: probabilistic, dense skip, deep supervision,")
    say("    filters 32..512, (20,160,160), bf16, untrained weights), wall clock per CASE in ms (medians of 5 runs after 2):")
    for n in (1, 8):
        infer = (lambda: dm.predict(bx)) if n == 1 else (lambda: dm.predict_mc(bx, n))
        with torch.no_grad():
            o = infer()
            mean, ent = (o, None) if n == 1 else (o["mean"], o["entropy"])
            mean = mean.contiguous()

            def score():
                return ops.read_val_records(ops.val_score(mean, y, ent, a, GAMMA), 2)

            def cand():
                det = D.extract_lesion_candidates(mean[..., 1].contiguous(), "dynamic")[0]
                truth = y[..., 1].contiguous()
                return [D.evaluate_case(det[i], truth[i]) for i in range(2)]
            whole = wall(lambda: V.validate(model, batch, 1, "lesion", n_draws=n, alpha=a, gamma=GAMMA)) / 2
            t_inf, t_score, t_cand = wall(infer) / 2, wall(score) / 2, wall(cand) / 2
        say(f"    n_draws {n}: validate {whole:8.2f}   inference {t_inf:8.2f}   scoring (kernel + the host read) {t_score:7.3f}   "
            f"candidates + matching {t_cand:8.2f}   (sum of parts {t_inf + t_score + t_cand:8.2f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-model", action="store_true", help="part (a) only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_validation.py measures on a GPU; none is visible")
    out = open(a.out, "w") if a.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()
    dev = torch.device("cuda:0")
    say("Train-time validation on one MI355X (gfx950), tools/bench_validation.py.")
    with torch.no_grad():
        part_a(say, dev)
    if not a.skip_model:
        part_b(say, dev)
    if out:
        out.close()


if __name__ == "__main__":
    main()
