"""Measurements of the back-projection onto the scan's grid (profiles/restore.txt):

    python tools/bench_restore.py --out profiles/restore.txt
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_restore.py --kernels-only      (kernel times, a run of its own)
    python tools/bench_restore.py --out profiles/restore.txt --append --stats DIR                 (adds the kernel times)

One batch: a softmax (2,20,160,160,2) fp32 on the network's grid at spacing (3.0, 0.5, 0.5) -> the scan's grid (24,384,384) at (3.6, 0.3,
0.3), the inverse of bench_resample.py's prepare_scan.  Three variants of the one launch: (i) channel 1 only, (ii) both channels,
(iii) channel 1 and the uint8 labels.

  (a) the host pipeline for the same arrays: the un-pad / window of the network grid, then scipy.ndimage.map_coordinates (order 1, mode
      'nearest') per channel and the inside rule, host clock;
  (b) a device fill_ of a tensor of the size of the variant's output, in the same process: the price of the stores alone; hipEvents;
  (c) ops.restore on device-resident data; hipEvents.

(a) runs HOST_RUNS times per round, (b) and (c) alternate, 2 x 100 batches each; 10 warm-up batches of the device side first.  Bytes are
computed from shapes.  The hipEvent figures of (c) include the host side of the call (torch.empty of one or two outputs, the ctypes
launch) where it is not hidden behind the kernel; the kernel against the fill kernel, both without any host share, is what the
rocprofv3 run gives: --kernels-only runs (i), (ii), (iii) and then the three fills, 50 times, and --stats reads the per-dispatch
kernel trace, so that (i) and (iii), which share a template instantiation, are told apart by their position in that order.
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
B, SCAN, C, DIMS = 2, (24, 384, 384), 2, (20, 160, 160)
SPACING, OUT_SPACING = (3.6, 0.3, 0.3), (3.0, 0.5, 0.5)
HOST_RUNS = 3
KERNELS = ("rst_kernel",)
# name, (c0, nsel), labels
VARIANTS = (("(i)   channel 1", (1, 1), False), ("(ii)  both channels", (0, 2), False), ("(iii) channel 1 + labels", (1, 1), True))


def softmax_batch():
    x = np.random.default_rng(0).normal(0.0, 2.0, (B, *DIMS, C))
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)


def host_batch(pred, geom, c0, nsel, labels):
    """The host pipeline: the real window of the network grid, map_coordinates (order 1, 'nearest') per channel, the inside rule."""
    from scipy import ndimage
    us = [P.restore_coords(ax)[0] for ax in geom]
    coords = np.stack(np.meshgrid(*us, indexing="ij"))
    inside = P.restore_inside(geom)
    real = tuple(slice(ax.lo, ax.lo + ax.count) for ax in geom)
    chans = range(C) if labels else range(c0, c0 + nsel)
    out = np.empty((B, *SCAN, len(chans)), np.float32)
    for b in range(B):
        for k, c in enumerate(chans):
            got = ndimage.map_coordinates(pred[b][real + (c,)], coords, order=1, mode="nearest", output=np.float32)
            out[b, ..., k] = np.where(inside, got, 0.0)
    if labels:
        return out[..., c0:c0 + nsel], np.where(inside, np.argmax(out, axis=-1), 0).astype(np.uint8)
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
    """Per variant (restore kernel times, fill kernel times) in ns from the per-dispatch kernel trace: --kernels-only dispatches the
    three variants and then the three fills in a fixed order, so the k-th dispatch of either kind belongs to variant k % 3."""
    import csv
    disp = []
    for f in sorted(glob.glob(os.path.join(stats_dir, "**", "*kernel_trace.csv"), recursive=True)):
        for r in csv.DictReader(open(f)):
            disp.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"]))
    disp.sort()
    mine = [d for _, d, n in disp if any(k in n for k in KERNELS)]
    fills = [d for _, d, n in disp if "FillFunctor" in n]
    if not mine or len(mine) % 3 or len(fills) != len(mine):
        raise SystemExit(f"{len(mine)} back-projection and {len(fills)} fill dispatches in the kernel trace under {stats_dir}: three variants "
                         "and three fills per round expected")
    return [(mine[v::3], fills[v::3]) for v in range(3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--kernels-only", action="store_true", help="50 calls of each variant and exit (the rocprofv3 run)")
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
        say("Kernel times from a separate rocprofv3 --kernel-trace --stats run (tools/bench_restore.py --kernels-only: 50 rounds of the three")
        say("variants and then a fill_ of each variant's output bytes; per-dispatch times from the kernel trace, no host share):")
        for (name, _, _), (mine, fills) in zip(VARIANTS, rows):
            km, kf = np.median(mine) / 1e3, np.median(fills) / 1e3
            say(f" {name}: rst_kernel median {km:.1f} us (min {np.min(mine) / 1e3:.1f}, {len(mine)} dispatches); fill kernel median {kf:.1f} us "
                f"(min {np.min(fills) / 1e3:.1f}); kernel / fill = {km / kf:.2f}")
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_restore.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    pred = softmax_batch()
    pd = torch.from_numpy(pred).to(dev)
    geom = P.restore_geometry(SCAN, SPACING, OUT_SPACING, DIMS)
    g = ops.restore_geom(DIMS, [ax.n for ax in geom], [ax.ratio for ax in geom], [ax.first for ax in geom], [ax.count for ax in geom],
                         [ax.lo for ax in geom])
    sides = [(lambda c0=c0, nsel=nsel, lab=lab: ops.restore(pd, g, c0, nsel, True, lab)) for _, (c0, nsel), lab in VARIANTS]
    nvox = B * int(np.prod(SCAN))
    fill_ts = [torch.empty(nvox * (4 * nsel + (1 if lab else 0)), dtype=torch.uint8, device=dev) for _, (_, nsel), lab in VARIANTS]
    if a.kernels_only:
        for _ in range(50):
            for side in sides:
                side()
            for t in fill_ts:
                t.fill_(1)
        torch.cuda.synchronize()
        return
    ms = lambda t: f"median {np.median(t):.3f} ms   min {np.min(t):.3f} ms   p90 {np.percentile(t, 90):.3f} ms"
    inside = P.restore_inside(geom)
    say(f"Back-projection at B = {B}: softmax {DIMS} x {C} channels fp32 at spacing {OUT_SPACING} -> the scan's grid {SCAN} at {SPACING}")
    say(f"(window {[(ax.first, ax.count) for ax in geom]}, pads in front {[ax.lo for ax in geom]}; {int(inside.sum())} of {inside.size} scan voxels")
    say("inside); one MI355X (gfx950); tools/bench_restore.py.")
    say("(a) host: the real window of the network grid, scipy.ndimage.map_coordinates (order 1, 'nearest') per channel, the inside rule (and")
    say("    np.argmax over both channels for the labels); one thread, host clock, no upload or download.  (b) a device fill_ of a tensor of")
    say("    the size of the variant's output in the same process: the price of the stores alone.  (c) ops.restore, ONE launch, data resident;")
    say(f"    hipEvents.  10 warm-up, then (a) {2 * HOST_RUNS} batches, (b) and (c) 200 batches each, alternating in two rounds.")
    say("    The event figures of (c) include the host side of the call (torch.empty of the outputs, the ctypes launch) where the kernel does")
    say("    not hide it; kernel against fill kernel without it: the rocprofv3 section below.")
    for (name, (c0, nsel), lab), side, fill_t in zip(VARIANTS, sides, fill_ts):
        fill = lambda: fill_t.fill_(1)
        event_clock(side, 10)
        event_clock(fill, 10)
        ta, tb, tc = [], [], []
        for _ in range(2):
            ta += host_clock(lambda: host_batch(pred, geom, c0, nsel, lab), HOST_RUNS)
            tb += event_clock(fill, 100)
            tc += event_clock(side, 100)
        ref = host_batch(pred, geom, c0, nsel, lab)
        got = side()
        diff = float(np.abs((got[0] if lab else got).cpu().numpy().astype(np.float64) - (ref[0] if lab else ref)).max())
        wbytes = nvox * (4 * nsel + (1 if lab else 0))
        rbytes = pred.nbytes
        say(f" {name}: output {wbytes / 1e6:.2f} MB, source {rbytes / 1e6:.2f} MB")
        say(f"   (a) host pipeline:                   {ms(ta)}")
        say(f"   (b) fill_ of the output's bytes:     {ms(tb)}   ({wbytes / np.median(tb) / 1e6:.0f} GB/s)")
        say(f"   (c) ops.restore:                     {ms(tc)}   ({wbytes / np.median(tc) / 1e6:.0f} GB/s of stores)")
        line = f"   (c) / (b) = {np.median(tc) / np.median(tb):.2f}; (a) / (c) = {np.median(ta) / np.median(tc):.0f}; max |(a) - (c)| over the batch: {diff:.3g}"
        if lab:
            line += f"; labels that differ from (a): {int((got[1].cpu().numpy() != ref[1]).sum())} of {nvox}"
        say(line)
    say("Not measured: the upload of the network's output or the download of the result, int16 / order 0, C > 2.")
    if out:
        out.close()


if __name__ == "__main__":
    main()
