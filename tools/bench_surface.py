"""Measurements of the surface-distance metrics (profiles/surface_metrics.txt):

    python tools/bench_surface.py --out profiles/surface_metrics.txt

One batch of (2, 20, 160, 160) uint8 label maps with K = 2 classes and spacing (3.0, 0.5, 0.5) mm, resident on the device, once as two
overlapping ellipsoids per class (tests/test_surface_distance_host.py's pattern: thin borders, a few per cent of the voxels) and once
as a dense random labelling at p = 0.35 (nearly every class voxel is a border voxel).  Timed: the three stages on their own
(ops.sd_border, ops.sd_distance of the 2 * B * K border masks, ops.sd_metrics) with preallocated workspaces, and the whole
surface_distance.surface_metrics call, which allocates its own; against the scipy pipeline of the same definitions on the host
(binary_erosion, distance_transform_edt with sampling, np.percentile).

Device sides: hipEvents, 10 warm-up and 200 batches; host side: host clock, HOST_RUNS batches, no upload or download counted.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from util import PKG, ops  # noqa: E402
import test_surface_distance_host as H  # noqa: E402

SD = PKG.surface_distance
L = PKG.hip.lib
B, DIMS, LABELS, SPACING = H.B, (20, 160, 160), H.LABELS, (3.0, 0.5, 0.5)
Q, TOL = 95.0, (1.1, 2.3)
HOST_RUNS = 3


def scipy_pipeline(pred, truth):
    out = []
    for b in range(B):
        for l in LABELS:
            d_ab, d_ba, counts = H.directed_sets(pred[b], truth[b], l, SPACING)
            if d_ab is None:
                out.append(counts)
                continue
            pooled = np.concatenate([d_ab, d_ba])
            out.append((counts, pooled.max(), (d_ab.mean() + d_ba.mean()) / 2, np.percentile(pooled, Q), np.percentile(d_ab, Q),
                        np.percentile(d_ba, Q), [(pooled <= np.float32(t)).mean() for t in TOL]))
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()
    if not torch.cuda.is_available():
        raise SystemExit("bench_surface.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    K, S = len(LABELS), B * len(LABELS)
    ms = lambda t: f"median {np.median(t):9.3f} ms   min {np.min(t):9.3f} ms   p90 {np.percentile(t, 90):9.3f} ms"
    say(f"Surface-distance metrics at B = {B}, volume {DIMS}, K = {K}, spacing {SPACING} mm, percentile {Q}, tolerances {TOL}; one MI355X")
    say("(gfx950); tools/bench_surface.py.  Device: data resident, hipEvents, 10 warm-up and 200 batches.  Host: scipy.ndimage")
    say(f"binary_erosion + distance_transform_edt + np.percentile on the same arrays, one thread, host clock, {HOST_RUNS} batches, no transfer counted.")
    ws = [ops.sd_workspace(L.M1_SD_STAGE_BORDER, B, K, DIMS, dev), ops.sd_workspace(L.M1_SD_STAGE_DISTANCE, 2 * S, 1, DIMS, dev),
          ops.sd_workspace(L.M1_SD_STAGE_METRICS, B, K, DIMS, dev)]
    for title, name in (("two overlapping ellipsoids per class", "ellipsoids"), ("dense random labelling, p = 0.35", "random0.35")):
        pred, truth = H.label_maps(DIMS, name)
        pd, td = torch.tensor(pred, device=dev), torch.tensor(truth, device=dev)
        borders, counts = ops.sd_border(pd, td, LABELS, ws=ws[0])
        stack = borders.view(-1, *DIMS)
        dist = ops.sd_distance(stack, SPACING, ws=ws[1]).view(borders.shape)
        sides = (("sd_border   (2 launches)", lambda: ops.sd_border(pd, td, LABELS, ws=ws[0])),
                 (f"sd_distance ({2 * S} volumes, 3 launches)", lambda: ops.sd_distance(stack, SPACING, ws=ws[1])),
                 ("sd_metrics  (11 launches)", lambda: ops.sd_metrics(borders, dist, counts, Q, TOL, ws=ws[2])),
                 ("surface_metrics, the whole call", lambda: SD.surface_metrics(pd, td, LABELS, SPACING, Q, TOL)))
        say(f"   {title}: border voxels per (b, k) {counts[..., 0].flatten().tolist()} (pred) {counts[..., 1].flatten().tolist()} (truth)")
        for what, fn in sides:
            event_clock(fn, 10)
            say(f"       device {what:42s} {ms(event_clock(fn, 200))}")
        say(f"       host   {'scipy pipeline':42s} {ms(host_clock(lambda: scipy_pipeline(pred, truth), HOST_RUNS))}")
        # what was measured computes the same thing
        got = {k: v.cpu().numpy() for k, v in SD.surface_metrics(pd, td, LABELS, SPACING, Q, TOL).items()}
        want = H.oracle(DIMS, name, SPACING, Q, TOL)
        H.assert_metrics_close(got, want, name, exact_nsd=False)
        say(f"       hd {got['hd'].flatten().tolist()}  hd95 {got['hdq'].flatten().tolist()}: counts equal scipy's, metrics within rtol 2^-22")
    n = B * int(np.prod(DIMS))
    say(f"   Per call: {n} voxels read as uint8 twice, {2 * S} border masks and fp32 distance maps of {n // B} voxels; the distance stage keeps")
    say(f"   {sum(w.numel() * 4 for w in ws[1:2]) / 1e6:.1f} MB of uint16 / fp64 intermediates in its workspace.")
    say("Not measured: uploads and downloads, int32 label maps, other K, kernel times on their own.")
    if out:
        out.close()


if __name__ == "__main__":
    main()
