"""Guard bands (tests/guarded.py) around every buffer of the label kernels (csrc/labels.hip) at the odd shapes: the staged halo, the
partial tiles, the 32-bit and float4 stores next to the byte and element ones -- no byte outside a buffer is written, and nothing
outside one reaches a result (a guard reads as 0xFF / NaN)."""
import itertools

import numpy as np
import pytest
import torch

from guarded import guarded
from util import PKG, ops

G = PKG.data_generators
T = ops.LABEL_TILE
EDGES = (1, 2, 3, 6, 7, T - 1, T, T + 1, 2 * T + 3)
pytestmark = pytest.mark.gpu


def _host_labels(ann, img, train_obj, mode, prob):
    """The host generator's arithmetic on in-memory arrays: (x, detection) of one batch."""
    if mode == "test":
        ann = np.zeros_like(ann)
    masks = [(ann >= 2)] if train_obj == "lesion" else [(ann == 1), (ann == 2)]
    masks = [G.smooth_slices(m.astype(np.uint8)) for m in masks]
    bg = np.ones_like(ann)
    for m in masks:
        bg = bg - m
    det = np.stack([bg] + masks, axis=-1)
    x = img if train_obj == "lesion" else img[..., :1]
    if prob:
        post = det[..., 1:] if mode == "train" else np.zeros_like(det[..., 1:])
        x = np.concatenate((x, post.astype(np.float32)), axis=-1)
    return x, det.astype(np.float32)


@pytest.mark.parametrize("planes,iterations", [(1, 1), (3, 2)])
def test_contour_smooth_stays_inside_its_buffers(dev, monkeypatch, planes, iterations):
    rng = np.random.default_rng(planes)
    with guarded(monkeypatch, dev) as g:
        for H, W in itertools.product(EDGES, EDGES):
            m = (rng.random((planes, H, W)) < 0.5).astype(np.uint8)
            got = ops.contour_smooth(g.put(torch.from_numpy(m)), iterations)
            assert g.count == (2 if iterations > 1 else 1)                      # the output (+ the scratch) came from the guarded allocator
            want = m
            for _ in range(iterations):
                want = G.smooth_slices(want)
            assert np.array_equal(got.cpu().numpy(), want), (H, W)
            g.check()


@pytest.mark.parametrize("train_obj,prob,mode", [("lesion", True, "train"), ("lesion", False, "valid"), ("zonal", True, "train"),
                                                 ("zonal", True, "test"), ("zonal", False, "train")])
def test_label_prepare_stays_inside_its_buffers(dev, monkeypatch, train_obj, prob, mode):
    rng = np.random.default_rng(17)
    with guarded(monkeypatch, dev) as g:
        for H, W in ((1, 1), (2, 3), (3, 7), (6, T - 1), (7, T + 1), (T, T), (T + 1, 2 * T + 3), (2 * T + 3, 6), (9, 36)):
            ann = rng.integers(0, 4, (2, 2, H, W)).astype(np.uint8)
            img = rng.standard_normal((2, 2, H, W, 3)).astype(np.float32)
            x, det, kl = ops.prepare_labels(None if mode == "test" else g.put(torch.from_numpy(ann)), g.put(torch.from_numpy(img)),
                                            train_obj, mode, prob)
            assert g.count == (3 if prob else 2)
            wx, wdet = _host_labels(ann, img, train_obj, mode, prob)
            assert np.array_equal(x.cpu().numpy(), wx) and np.array_equal(det.cpu().numpy(), wdet), (H, W)
            assert (kl is None) == (not prob) and (kl is None or not kl.any())
            g.check()
