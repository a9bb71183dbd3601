"""Measurements of the train-time augmentation chain (profiles/augment_gpu.txt):

    python tools/bench_augment.py --out profiles/augment_gpu.txt

  * hipEvent time of the whole chain per batch at (2,20,160,160), lesion, probabilistic input, all stages fired, and the bytes it
    moves against the algorithmic minimum;
  * the numpy restatement of tests/test_augmentations.py on one volume (what the CPU would have to do per sample);
  * the trainer's step-to-step time with --AUGMENT 1 against --AUGMENT 0, C3 filters (eager ``fit``).
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_augmentations as TA  # noqa: E402

PKG, A, ops, T = TA.PKG, TA.A, TA.ops, TA.T


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-trainer", action="store_true")
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()
    dev = torch.device("cuda:0")
    img, lab, nimg = TA._problem("lesion", "big", 0)
    N, D, H = img.shape[:3]
    table = A.draw_params(None, N, H, H, explicit=TA._records(N, H, 0, 0x1FE, "lesion"), device=dev)
    x, y = torch.from_numpy(img).to(dev), torch.from_numpy(lab).to(dev)
    rng = A.new_rng(1, dev)
    ts = timeit(lambda: A.augment_tensors({"image": x}, {"detection": y}, TA.DEFAULT, rng=rng, params=table))
    say("Augmentation chain at (2,20,160,160), lesion, probabilistic input (C = 4, nc = 2), one MI355X (gfx950); hipEvents around the call,")
    say("20 warm-up + 200 timed runs (tools/bench_augment.py).")
    say("1) all stages fired in both samples (injected table), eager launches (geom + fold, gamma stats + fold, intensity):")
    say(f"   median {np.median(ts) * 1e3:.1f} us   min {ts.min() * 1e3:.1f} us   p90 {np.percentile(ts, 90) * 1e3:.1f} us")
    ts2 = timeit(lambda: A.augment_tensors({"image": x}, {"detection": y}, TA.DEFAULT, rng=rng))
    say(f"   with m1_aug_draw in front (default AUGM_PARAMS: every stage fires with probability 0.75): median {np.median(ts2) * 1e3:.1f} us")
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        A.augment_tensors({"image": x}, {"detection": y}, TA.DEFAULT, rng=rng)
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        A.augment_tensors({"image": x}, {"detection": y}, TA.DEFAULT, rng=rng)
        ops.step_advance(None, rng)
    tg = timeit(gr.replay, warm=10)
    say(f"   draw + chain + step advance captured in one graph, fresh draws per replay: median {np.median(tg) * 1e3:.1f} us   min {tg.min() * 1e3:.1f} us")
    vox = N * D * H * H
    src, im = vox * (4 + 2) * 4, vox * 4 * 4
    mn = 2 * src + 3 * im
    say(f"2) bytes: source image + label {src / 1e6:.2f} MB.  Algorithmic minimum with the gamma stage on: the geometric pass reads the source")
    say(f"   once and writes G + label ({src / 1e6:.2f} + {src / 1e6:.2f}), the statistics of the powered values read G ({im / 1e6:.2f}), the intensity pass")
    say(f"   reads G and writes the image ({im / 1e6:.2f} + {im / 1e6:.2f}): {mn / 1e6:.2f} MB.  On top of that the kernels REQUEST the gather's re-reads")
    say("   (up to 16 taps per element, 32 for the shifted channel; neighbouring voxels share them through the caches) and the")
    say("   poor-scan taps; no counters were collected, so what reaches HBM is not known.")
    say(f"   {mn / 1e6:.2f} MB in the median time of 1) = {mn / np.median(ts) / 1e6:.0f} GB/s of algorithmic traffic")
    rn = A.table_to_numpy(table)
    for vt in (np.float64, np.float32):
        z = np.zeros_like(img[0])
        t0 = time.time()
        TA.r_chain(img[0], lab[0], rn[0], 0x1FF, nimg, vt, z)
        t1 = time.time()
        say(f"3) numpy restatement on the host, one (20,160,160) volume, all stages fired, values in {vt.__name__}: {t1 - t0:.2f} s "
            f"= {1 / (t1 - t0):.2f} volumes/s on one thread (the noise draws not included)")
    if not a.no_trainer:
        M1 = PKG.unets.networks.M1
        real, stamps = M1.train_step, []

        def timed(self, bx, by):
            r = real(self, bx, by)
            torch.cuda.synchronize()
            stamps.append(time.time())
            return r
        M1.train_step = timed
        say("4) trainer, eager fit (NOT the captured bench step), C3 filters (32,64,128,256,512), dense skip + deep supervision, probabilistic,")
        say("   bf16, batch 2, 8 synthetic samples; step-to-step wall time incl. host batch assembly and upload, steps 9-32, alternating:")
        for aug in (0, 1, 0, 1):
            del stamps[:]
            T.main(["--WEIGHTS_DIR", tempfile.mkdtemp() + "/", "--NAME", "m", "--FOLDS", "0", "--UNET_FEATURE_CHANNELS", "32", "64", "128",
                    "256", "512", "--UNET_PROBABILISTIC", "1", "--UNET_DENSE_SKIP", "1", "--UNET_DEEP_SUPERVISION", "1",
                    "--SYNTHETIC_SAMPLES", "8", "--NUM_EPOCHS", "8", "--WEIGHTS_MIN_EPOCH", "99", "--AUGMENT", str(aug)])
            d = np.diff(np.array(stamps))[8:]
            say(f"   --AUGMENT {aug}: median {np.median(d) * 1e3:.2f} ms/step   min {d.min() * 1e3:.2f}   ({len(d)} steps)")
        M1.train_step = real
    if out:
        out.close()


if __name__ == "__main__":
    main()
