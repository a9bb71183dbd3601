"""Measurements of the connected-component labelling and the lesion extraction (profiles/components.txt):

    python tools/bench_components.py --out profiles/components.txt

One batch of (2, 20, 160, 160), resident on the device:

  (a) ops.label_components (connectivity 3) of a softmax-like map -- a handful of Gaussian blobs plus noise -- at threshold 0.25,
      against scipy.ndimage.label of the same masks on the host;
  (b) detection.extract_lesion_candidates('dynamic') of that map (5 rounds of peak, label, select, take: 60 launches), against the
      numpy / scipy transcription of the rule on the host;
  (c) ops.label_components of a dense random mask (p = 0.35, connectivity 3: long chains of unions across the tile borders), against
      scipy.ndimage.label.

Device sides: hipEvents, 10 warm-up and 200 batches; host sides: host clock, HOST_RUNS batches, no upload or download counted.
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

Dt = PKG.detection
B, DIMS = 2, (20, 160, 160)
HOST_RUNS = 5
STATIC = 0.25


def softmax_like(seed=0):
    """(B, *DIMS) fp32: per sample five blobs (peaks 0.95 .. 0.35, sigma 1.5 .. 4 voxels in-plane) on uniform noise of 0.02."""
    rng = np.random.default_rng(seed)
    z, y, x = np.indices(DIMS).astype(np.float32)
    out = rng.random((B, *DIMS)).astype(np.float32) * np.float32(0.02)
    for b in range(B):
        for peak in (0.95, 0.8, 0.65, 0.5, 0.35):
            c = [rng.uniform(3, n - 3) for n in DIMS]
            s = rng.uniform(1.5, 4.0)
            out[b] += np.float32(peak) * np.exp(-(((z - c[0]) / (s / 2)) ** 2 + ((y - c[1]) / s) ** 2 + ((x - c[2]) / s) ** 2) / 2)
    return np.minimum(out, np.float32(0.999))


def dynamic_host(maps, n=5, min_voxels=10, factor=2.5, min_confidence=0.1):
    from scipy import ndimage
    structure = np.ones((3, 3, 3))
    dets = []
    for w in maps.copy():
        det, k = np.zeros_like(w), 0
        for _ in range(n):
            i = np.unravel_index(np.argmax(w), w.shape)
            peak = w[i]
            if not peak > min_confidence:
                break
            labels, _ = ndimage.label(w > peak / np.float32(factor), structure)
            comp = labels == labels[i]
            if comp.sum() >= min_voxels:
                k += 1
                det[comp] = peak
            w[comp] = 0
        dets.append(det)
    return np.stack(dets)


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
        raise SystemExit("bench_components.py measures on a GPU; none is visible")
    from scipy import ndimage
    dev = torch.device("cuda:0")
    structure = np.ones((3, 3, 3))
    maps = softmax_like()
    dense = np.random.default_rng(1).random((B, *DIMS)) < 0.35
    md, dd = torch.from_numpy(maps).to(dev), torch.from_numpy(dense.astype(np.uint8)).to(dev)
    ws = ops.cc_workspace(md.shape, dev)
    sides = (("(a) labelling, softmax-like map > 0.25", lambda: ops.label_components(md, STATIC, 3, ws=ws),
              lambda: [ndimage.label(m > np.float32(STATIC), structure) for m in maps]),
             ("(b) extract_lesion_candidates('dynamic')", lambda: Dt.extract_lesion_candidates(md), lambda: dynamic_host(maps)),
             ("(c) labelling, dense random mask p = 0.35", lambda: ops.label_components(dd, 0, 3, ws=ws),
              lambda: [ndimage.label(m, structure) for m in dense]))
    ms = lambda t: f"median {np.median(t):9.3f} ms   min {np.min(t):9.3f} ms   p90 {np.percentile(t, 90):9.3f} ms"
    say(f"Connected components and lesion extraction at B = {B}, volume {DIMS}, connectivity 3; one MI355X (gfx950); tools/bench_components.py.")
    say(f"Device: data resident, hipEvents, 10 warm-up and 200 batches.  Host: scipy.ndimage.label / the numpy + scipy transcription of the")
    say(f"dynamic rule on the same arrays, one thread, host clock, {HOST_RUNS} batches, no transfer counted.")
    for name, device_side, host_side in sides:
        event_clock(device_side, 10)
        td, th = event_clock(device_side, 200), host_clock(host_side, HOST_RUNS)
        say(f"   {name}")
        say(f"       device: {ms(td)}")
        say(f"       host:   {ms(th)}")
    # what was measured computes the same thing
    for m, x, thr in ((maps > np.float32(STATIC), md, STATIC), (dense, dd, 0)):
        labels, counts = ops.label_components(x, thr, 3, ws=ws)
        for b in range(B):
            want, k = ndimage.label(m[b], structure)
            assert counts[b].item() == k and np.array_equal(labels[b].cpu().numpy(), want)
    assert np.array_equal(Dt.extract_lesion_candidates(md)[0].cpu().numpy(), dynamic_host(maps))
    kc = [int(ndimage.label(m, structure)[1]) for m in dense]
    say(f"   components: (a) {[int(ndimage.label(m > np.float32(STATIC), structure)[1]) for m in maps]}, (c) {kc} per sample; device results equal the host's exactly.")
    n = B * int(np.prod(DIMS))
    say(f"   The labelling is 6 launches over {n} voxels ({n * 4 / 1e6:.2f} MB per int32 pass); a round of the extraction is 12 launches.")
    say("Not measured: uploads and downloads, connectivity 1 and 2, the fixed-threshold extraction, evaluate_case, kernel times on their own.")
    if out:
        out.close()


if __name__ == "__main__":
    main()
