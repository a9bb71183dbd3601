"""Measurements of the scan preprocessing (profiles/preprocess.txt):

    python tools/bench_preprocess.py --out profiles/preprocess.txt
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_preprocess.py --kernels-only      (kernel times, a run of its own)
    python tools/bench_preprocess.py --out profiles/preprocess.txt --append --stats DIR             (adds the kernel times)

One batch: raw (2,24,192,192,3), int16 and fp32, -> (20,160,160), percentile None and 99.5 (an example: the reference fixes none).

  (a) the host path for the same arrays: preprocess.resize_image_with_crop_or_pad + preprocess.whitening (the reference's numpy calls)
      per sequence, stacked and uploaded; host clock around one batch ending in a device synchronise;
  (b) preprocess.prepare_input on device-resident raw data, and again including the upload of the raw array; hipEvents.

(a) and (b, with upload) alternate, 2 x 100 batches each per setting = 200; 10 warm-up batches first.  Bytes are computed from shapes.
"""
import argparse
import glob
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from util import PKG, ops  # noqa: E402

P = PKG.preprocess
B, RAW, DIMS, C = 2, (24, 192, 192), (20, 160, 160), 3
N = int(np.prod(DIMS))
KERNELS = ("pp_rows_kernel", "os_hist_kernel", "os_scan_kernel", "wh_stats_kernel", "wh_fold_kernel")


def raw_batch(dtype):
    x = np.random.default_rng(0).normal(300.0, 200.0, (B, *RAW, C))
    return np.rint(x).astype(np.int16) if dtype == np.int16 else x.astype(np.float32)


def host_batch(raw, percentile, dev):
    seqs = [[P.whitening(P.resize_image_with_crop_or_pad(raw[b, ..., c], DIMS), percentile) for c in range(C)] for b in range(B)]
    return torch.from_numpy(np.stack([np.stack(s, axis=-1) for s in seqs])).to(dev)


def host_clock(fn, runs):
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def event_clock(fn, runs):
    ts = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def kernel_rows(stats_dir):
    import csv
    rows = []
    for f in sorted(glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True)):
        for r in csv.DictReader(open(f)):
            if any(k in r["Name"] for k in KERNELS):
                rows.append((r["Name"], int(r["Calls"]), float(r["AverageNs"])))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--kernels-only", action="store_true", help="50 prepare_input calls per setting and exit (the rocprofv3 run)")
    ap.add_argument("--stats", default=None, help="directory of a rocprofv3 --kernel-trace --stats run of --kernels-only: report and exit")
    a = ap.parse_args()
    out = open(a.out, "a" if a.append else "w") if a.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()
    if a.stats:
        rows = kernel_rows(a.stats)
        if not rows:
            raise SystemExit(f"no preprocessing kernel in the kernel_stats.csv under {a.stats}")
        say("3) kernel times from a separate rocprofv3 --kernel-trace --stats run (tools/bench_preprocess.py --kernels-only: 50 calls per")
        say("   setting, int16 and fp32, percentile None and 99.5; a selection pass is 4 launches of each of its two kernels):")
        for name, calls, avg in rows:
            say(f"   {name.split('(')[0][:70]}: {calls} calls, average {avg / 1e3:.1f} us")
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_preprocess.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    if a.kernels_only:
        for dtype in (np.int16, np.float32):
            rd = torch.from_numpy(raw_batch(dtype)).to(dev)
            for p in (None, 99.5):
                for _ in range(50):
                    P.prepare_input(rd, DIMS, percentile=p)
        torch.cuda.synchronize()
        return
    ms = lambda t: f"median {np.median(t):.3f} ms   min {np.min(t):.3f} ms   p90 {np.percentile(t, 90):.3f} ms"
    say(f"Scan preprocessing at B = {B}, raw {RAW} x {C} channels -> {DIMS}, one MI355X (gfx950); tools/bench_preprocess.py.")
    say("(a) host: resize_image_with_crop_or_pad + whitening per sequence (numpy, one thread), stacked, uploaded; host clock around one")
    say("    batch ending in a device synchronise.  (b) prepare_input on the device: hipEvents; 'resident' = the raw batch is on the")
    say("    device already, 'with upload' = the timed window includes the copy of the raw array.  10 warm-up, then 2 x 100 batches per")
    say("    side, (a) and (b with upload) alternating.")
    for dtype in (np.int16, np.float32):
        raw = raw_batch(dtype)
        host_t = torch.from_numpy(raw)
        rd = host_t.to(dev)
        esz = raw.dtype.itemsize
        for p in (None, 99.5):
            side_a = lambda: host_batch(raw, p, dev)
            side_b = lambda: P.prepare_input(rd, DIMS, percentile=p)
            side_bu = lambda: P.prepare_input(host_t.to(dev), DIMS, percentile=p)
            host_clock(side_a, 2)
            event_clock(side_b, 10)
            event_clock(side_bu, 10)
            ta, tbu = [], []
            for _ in range(2):
                ta += host_clock(side_a, 100)
                tbu += event_clock(side_bu, 100)
            tb = event_clock(side_b, 200)
            diff = float((side_a().double() - side_b()[0].double()).abs().max())
            launches = 3 if p is None else 11
            passes = 3 if p is None else 7                    # sweeps of the output domain: 2 statistics + 1 element (+ 4 selection)
            moved = B * C * N * (passes * esz + 4)
            say(f"{raw.dtype.name} raw, percentile {p}:")
            say(f"   (a) host path + upload of the fp32 result:      {ms(ta)}")
            say(f"   (b) prepare_input, raw resident:                {ms(tb)}")
            say(f"   (b) prepare_input, with upload of the raw:      {ms(tbu)}")
            say(f"   (b with upload) <= (a): {np.median(tbu) <= np.median(ta)}; max |(a) - (b)| over the batch: {diff:.3g}")
            say(f"   launches per call: {launches}; uploaded (a) {B * C * N * 4 / 1e6:.2f} MB fp32, (b) {raw.nbytes / 1e6:.2f} MB raw; "
                f"device reads of the output domain: {passes} sweeps x {B * C * N * esz / 1e6:.2f} MB + one write of {B * C * N * 4 / 1e6:.2f} MB "
                f"= {moved / 1e6:.2f} MB (the algorithmic minimum for this pass structure: each sweep reads the domain once; "
                f"a single-sweep minimum would be {B * C * N * (esz + 4) / 1e6:.2f} MB)")
    if out:
        out.close()


if __name__ == "__main__":
    main()
