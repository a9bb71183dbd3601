"""Measurements of the label feed (profiles/label_prep.txt):

    python tools/bench_labels.py --out profiles/label_prep.txt
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_labels.py --kernels-only          (kernel times, a run of its own)
    python tools/bench_labels.py --out profiles/label_prep.txt --append --stats DIR                 (adds the kernel rates)

One batch of the workload's own size: B = 2, (20,160,160), lesion, probabilistic, training; seeded cases written to a temporary
directory first.  Two sides in this process, alternating, host clock around work that ends in a device synchronise, 20 warm-up + 200
timed batches, twice per side:

  (a) the path without the generator, for the same arrays: train_model.batches(train_model.custom_data_generator(cases, ...)) over
      train_model.load_npy_cases -- no smoothing, the one-hot, posterior and KL planes built in fp32 on the host and copied;
  (b) data_generators.device_batches over a sheet of the same files: binarise + smooth + one-hot + the three outputs in ONE launch
      from the raw image and a uint8 annotation.

(a) holds its cases in memory (load_npy_cases reads every file once, before the timed window); (b) is the generator's own path and
reads its batch's .npy files inside the window, as the reference's generator does (they were written a moment ago: page cache).
Bytes are computed from shapes.
"""
import argparse
import glob
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from util import PKG, ops  # noqa: E402

import importlib  # noqa: E402
T = importlib.import_module("prostatemr_3d-cad-cspca_amd.train_model")
G = PKG.data_generators

B, DIMS, C, NC, NCASES = 2, (20, 160, 160), 3, 2, 4
VOX = B * int(np.prod(DIMS))


def write_cases(root):
    """Seeded cases: whitened noise, grades 0..5 in a ball of radius 12 per case (0 elsewhere).  image_*.npy / label_*.npy as
    --TRAIN_NPY_DIR takes them, and the sheet over the same files."""
    rng = np.random.default_rng(0)
    zz, yy, xx = np.meshgrid(*[np.arange(n) for n in DIMS], indexing="ij")
    rows = []
    for i in range(NCASES):
        img = rng.standard_normal((*DIMS, C)).astype(np.float32)
        c = [rng.integers(4, DIMS[0] - 4), rng.integers(20, DIMS[1] - 20), rng.integers(20, DIMS[2] - 20)]
        ball = ((zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2) <= 144
        lab = np.where(ball, rng.integers(0, 6, DIMS), 0).astype(np.uint8)
        p = [os.path.join(root, f"image_{i:03d}.npy"), os.path.join(root, f"label_{i:03d}.npy")]
        np.save(p[0], img)
        np.save(p[1], lab)
        rows.append(p)
    sheet = os.path.join(root, "train-fold-1.csv")
    with open(sheet, "w") as fh:
        fh.write("image_path,label_path\n" + "".join(",".join(r) + "\n" for r in rows))
    return sheet, rows


def time_batches(gen, warm=20, runs=200):
    for _ in range(warm):
        next(gen)
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        next(gen)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return np.array(ts)


def kernel_rows(stats_dir):
    """(name, calls, average ns) of the label kernels from rocprofv3's kernel_stats.csv under ``stats_dir``."""
    import csv
    rows = []
    for f in sorted(glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True)):
        for r in csv.DictReader(open(f)):
            if "label_prepare" in r["Name"] or "contour_smooth" in r["Name"]:
                rows.append((r["Name"], int(r["Calls"]), float(r["AverageNs"])))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--kernels-only", action="store_true", help="launch the two kernels 50 times each and exit (the rocprofv3 run)")
    ap.add_argument("--stats", default=None, help="directory of a rocprofv3 --kernel-trace --stats run of --kernels-only: report rates and exit")
    a = ap.parse_args()
    out = open(a.out, "a" if a.append else "w") if a.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()
    b_prep = VOX * (1 + 4 * C + 4 * (C + NC - 1) + 4 * NC + 4 * NC)          # annotation + image read; input, detection, KL written
    b_smooth = VOX * 2
    if a.stats:
        rows = kernel_rows(a.stats)
        if not rows:
            raise SystemExit(f"no label kernel in the kernel_stats.csv under {a.stats}")
        say("3) kernel times from a separate rocprofv3 --kernel-trace --stats run (tools/bench_labels.py --kernels-only), bytes from shapes:")
        for name, calls, avg in rows:
            nb = b_prep if "label_prepare" in name else b_smooth
            say(f"   {name.split('(')[0][:60]}: {calls} calls, average {avg / 1e3:.1f} us, {nb / 1e6:.2f} MB -> {nb / avg:.0f} GB/s")
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_labels.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as root:
        sheet, rows = write_cases(root)
        if a.kernels_only:
            img = torch.from_numpy(np.stack([np.load(r[0]) for r in rows[:B]])).to(dev)
            ann = torch.from_numpy(np.stack([np.load(r[1]) for r in rows[:B]])).to(dev)
            mask = (ann >= 2).to(torch.uint8)
            for _ in range(50):
                ops.prepare_labels(ann, img, "lesion", "train", True)
                ops.contour_smooth(mask)
            torch.cuda.synchronize()
            return
        measure(a, say, sheet, T.load_npy_cases(root, NC), dev)
    if out:
        out.close()


def measure(a, say, sheet, cases, dev):
    side_a = lambda: T.batches(T.custom_data_generator(cases, probabilistic=True, mode='train'), B, dev)
    side_b = lambda: G.device_batches(sheet, train_obj='lesion', probabilistic=True, mode='train', batch_size=B, device=dev)
    (ax, ay), (bx, by) = next(side_a()), next(side_b())
    same_img = torch.equal(ax["image"][..., :C], bx["image"][..., :C])
    fg_a, fg_b = int(ay["detection"][..., 1].sum()), int(by["detection"][..., 1].sum())
    ta, tb = [], []
    for _ in range(2):                                          # alternating: a, b, a, b
        ta.append(time_batches(side_a()))
        tb.append(time_batches(side_b()))
    ta, tb = np.concatenate(ta), np.concatenate(tb)
    ms = lambda t: f"median {np.median(t):.3f} ms   min {t.min():.3f} ms   p90 {np.percentile(t, 90):.3f} ms"
    up_a, up_b = VOX * 4 * (C + NC - 1 + NC + NC), VOX * (4 * C + 1)
    lab_a, lab_b = VOX * 4 * (NC - 1 + NC + NC), VOX
    spread = np.percentile(ta, 90) - np.median(ta)
    say(f"Label feed at B = {B}, {DIMS[0]}x{DIMS[1]}x{DIMS[2]}, lesion, probabilistic, training, {NCASES} seeded cases, one MI355X (gfx950);")
    say("host clock around one batch ending in a device synchronise, 20 warm-up + 200 timed batches, twice per side, alternating")
    say("(tools/bench_labels.py).  (a) holds its cases in memory; (b) reads its batch's .npy files (page cache) inside the window.")
    say(f"1) (a) host planes, no smoothing (train_model.batches over load_npy_cases):   {ms(ta)}")
    say(f"   (b) device_batches (raw image + uint8 annotation, one m1_label_prepare):  {ms(tb)}")
    say(f"   (b) - (a) at the median: {np.median(tb) - np.median(ta):+.3f} ms; (a)'s own p90 - median spread: {spread:.3f} ms -> "
        f"{'within' if np.median(tb) - np.median(ta) <= spread else 'OUTSIDE'} the expectation (b) <= (a) + spread")
    say(f"   same image channels on both sides: {same_img}; foreground voxels of the batch: (a) {fg_a} unsmoothed (label == 1 only), (b) {fg_b} (grades >= 2, smoothed)")
    say(f"2) bytes per batch, from shapes: uploaded (a) {up_a / 1e6:.2f} MB, (b) {up_b / 1e6:.2f} MB; of which label planes (a) {lab_a / 1e6:.2f} MB "
        f"(posterior + detection + KL in fp32), (b) {lab_b / 1e6:.2f} MB (uint8) = 1/{lab_a // lab_b};")
    say(f"   m1_label_prepare reads {VOX * (1 + 4 * C) / 1e6:.2f} MB and writes {VOX * 4 * (C + NC - 1 + 2 * NC) / 1e6:.2f} MB on the device.")


if __name__ == "__main__":
    main()
