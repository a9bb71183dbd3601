"""Measurements of the resampling to a target spacing (profiles/resample.txt):

    python tools/bench_resample.py --out profiles/resample.txt
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_resample.py --kernels-only      (kernel times, a run of its own)
    python tools/bench_resample.py --out profiles/resample.txt --append --stats DIR               (adds the kernel times)

One batch: a T2-like int16 raw (2,24,384,384,1) at spacing (3.6, 0.3, 0.3) -> spacing (3.0, 0.5, 0.5), i.e. a grid of (29,230,230), and
prepare_scan to (20,160,160) (an example: the reference fixes none).

  (a) the host pair for the same arrays: scipy.ndimage.spline_filter + map_coordinates (order 3, mode 'mirror') per sequence on the whole
      grid (SimpleITK, the reference's resampler, is not installed), host clock;
  (b) ops.resample of the whole grid on device-resident raw data; hipEvents;
  (c) preprocess.prepare_scan (the window the crop keeps, then prepare_input) on device-resident raw data; hipEvents.

(a) and (b) alternate, 2 x HOST_RUNS / 2 x 100 batches; 10 warm-up batches of the device side first.  Bytes are computed from shapes.
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
B, RAW, C, DIMS = 2, (24, 384, 384), 1, (20, 160, 160)
SPACING, OUT_SPACING = (3.6, 0.3, 0.3), (3.0, 0.5, 0.5)
HOST_RUNS = 5
KERNELS = ("rs_rows_kernel", "rs_cols_kernel", "rs_nearest_kernel")


def raw_batch():
    x = np.random.default_rng(0).normal(300.0, 200.0, (B, *RAW, C))
    return np.rint(x).astype(np.int16)


def host_batch(raw):
    from scipy import ndimage
    size = P.resample_size(RAW, SPACING, OUT_SPACING)
    steps = P.resample_steps(SPACING, OUT_SPACING)
    coords = np.stack(np.meshgrid(*[np.arange(n) * s for n, s in zip(size, steps)], indexing="ij"))
    out = np.empty((B, *size, C), np.float32)
    for b in range(B):
        for c in range(C):
            coef = ndimage.spline_filter(raw[b, ..., c].astype(np.float32), order=3, mode="mirror", output=np.float64)
            out[b, ..., c] = ndimage.map_coordinates(coef, coords, order=3, mode="mirror", prefilter=False)
    return out


def host_clock(fn, runs):
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
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


def pass_bytes(src, dst, esz):
    """Bytes per pass of the order 2, 1, 0 from shapes: each pass reads its input once and writes its output once."""
    v0 = B * C * src[0] * src[1] * src[2]
    v1 = B * C * src[0] * src[1] * dst[2]
    v2 = B * C * src[0] * dst[1] * dst[2]
    v3 = B * C * dst[0] * dst[1] * dst[2]
    return (v0 * esz + v1 * 4, v1 * 4 + v2 * 4, v2 * 4 + v3 * 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--kernels-only", action="store_true", help="50 calls of each device side and exit (the rocprofv3 run)")
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
            raise SystemExit(f"no resampling kernel in the kernel_stats.csv under {a.stats}")
        say("3) kernel times from a separate rocprofv3 --kernel-trace --stats run (tools/bench_resample.py --kernels-only: 50 calls of the")
        say("   whole grid and 50 of prepare_scan's window; every row averages both):")
        for name, calls, avg in rows:
            say(f"   {name.split('(')[0][:90]}: {calls} calls, average {avg / 1e3:.1f} us")
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    raw = raw_batch()
    rd = torch.from_numpy(raw).to(dev)
    size = P.resample_size(RAW, SPACING, OUT_SPACING)
    steps = P.resample_steps(SPACING, OUT_SPACING)
    side_b = lambda: ops.resample(rd, steps, size)
    side_c = lambda: P.prepare_scan(rd, SPACING, OUT_SPACING, DIMS, percentile=99.5)
    if a.kernels_only:
        for _ in range(50):
            side_b()
            side_c()
        torch.cuda.synchronize()
        return
    ms = lambda t: f"median {np.median(t):.3f} ms   min {np.min(t):.3f} ms   p90 {np.percentile(t, 90):.3f} ms"
    window = P.scan_window(RAW, SPACING, OUT_SPACING, DIMS)
    say(f"Resampling at B = {B}, int16 raw {RAW} x {C} channel, spacing {SPACING} -> {OUT_SPACING}: grid {size}; prepare_scan to {DIMS}")
    say(f"(window {window}); one MI355X (gfx950); tools/bench_resample.py.")
    say("(a) host: scipy.ndimage.spline_filter + map_coordinates (order 3, mirror) per sequence on the whole grid, one thread, host clock,")
    say("    no upload.  SimpleITK is not installed: the reference's own resampler is NOT measured.  (b) ops.resample of the whole grid,")
    say("    (c) preprocess.prepare_scan with percentile 99.5 (3 resampling launches on the window + 11 of prepare_input); raw resident,")
    say(f"    hipEvents.  10 warm-up, then (a) {2 * HOST_RUNS} and (b) 200 batches, alternating in two rounds; (c) 200 batches.")
    event_clock(side_b, 10)
    event_clock(side_c, 10)
    ta, tb = [], []
    for _ in range(2):
        ta += host_clock(lambda: host_batch(raw), HOST_RUNS)
        tb += event_clock(side_b, 100)
    tc = event_clock(side_c, 200)
    ref = host_batch(raw)
    got = side_b().cpu().numpy()
    diff = float(np.abs(got.astype(np.float64) - ref).max()) / float(np.abs(ref).max())
    say(f"   (a) scipy pair on the host, whole grid:          {ms(ta)}")
    say(f"   (b) ops.resample, whole grid, raw resident:      {ms(tb)}")
    say(f"   (c) prepare_scan (window + prepare_input):       {ms(tc)}")
    say(f"   (b) <= (a): {np.median(tb) <= np.median(ta)}; max |(a) - (b)| / max|(a)| over the batch: {diff:.3g}")
    for name, dst, t in (("(b) whole grid", size, tb), ("(c) window", tuple(c for _, c in window), None)):
        pb = pass_bytes(RAW, dst, raw.dtype.itemsize)
        line = (f"   bytes from shapes, {name}: pass over axis 2 {pb[0] / 1e6:.2f} MB, axis 1 {pb[1] / 1e6:.2f} MB, axis 0 {pb[2] / 1e6:.2f} MB "
                f"= {sum(pb) / 1e6:.2f} MB (each pass reads its input once and writes its output once")
        if t is not None:
            line += f"; at the median of (b) that is {sum(pb) / np.median(t) / 1e6:.1f} GB/s"
        say(line + ")")
    say("   The pass over axis 1 filters its 384-voxel lines in place in the workspace: it reads its input twice more and writes it twice")
    say("   (the two recursions), which the model above does not count.")
    say("Not measured: SimpleITK / ITK (not installed), the upload of the raw batch, the label (nearest) path, fp32 raw input, C > 1.")
    if out:
        out.close()


if __name__ == "__main__":
    main()
