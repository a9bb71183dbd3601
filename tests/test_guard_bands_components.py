"""Guard bands (tests/guarded.py) around every tensor and workspace of the component kernels (csrc/components.hip) at the odd shapes:
a volume smaller than a tile, one voxel past a tile edge on every axis, W = 64 + 1, chunks of 1024 voxels that end inside a row.  No
byte outside a buffer is written, and nothing outside one reaches a result: a guard reads as 0xFF bytes, which is the label -1 and the
value NaN -- a neighbour fetched across a volume's end would join components, a NaN would become a maximum."""
import numpy as np
import pytest
import torch

from guarded import guarded
from util import PKG, ops
from test_components import assert_stats_equal, reference, values_for
from test_detection_host import B, CONNECTIVITIES, SERPENTINE_SHAPE, SHAPES, blob_map, patterns

Dt = PKG.detection
pytestmark = pytest.mark.gpu
NAMES = ("full", "random0.35", "random0.8", "checkerboard")


@pytest.mark.parametrize("in_dtype", (np.float32, np.uint8))
def test_labelling_and_tables_stay_inside_their_buffers(dev, monkeypatch, in_dtype):
    with guarded(monkeypatch, dev) as g:
        for shape in SHAPES + (SERPENTINE_SHAPE,):
            for name in NAMES + (("serpentine",) if shape == SERPENTINE_SHAPE else ()):
                x = g.put(torch.from_numpy(patterns(shape)[name].astype(in_dtype)))
                vals = g.put(torch.from_numpy(values_for(shape)))
                for c in CONNECTIVITIES:
                    want, counts = reference(shape, name, c)
                    labels, k = ops.label_components(x, 0.0, c)
                    assert g.count == 3                                                # labels, counts and the workspace
                    assert np.array_equal(labels.cpu().numpy(), want) and np.array_equal(k.cpu().numpy(), counts), (shape, name, c)
                    K = int(counts.max()) + 1
                    stats = ops.component_stats(labels, vals, K)
                    assert_stats_equal(stats, Dt.component_stats_host(want, values_for(shape), K), (shape, name, c))
                    other = g.put(torch.from_numpy(np.ascontiguousarray(want[::-1])))    # the batch entries swapped
                    table = ops.component_overlap(labels, other, K, 2)
                    assert np.array_equal(table.cpu().numpy(), Dt.overlap_host(want, want[::-1], K, 2)), (shape, name, c)
                    g.check()


def test_extraction_stays_inside_its_buffers(dev, monkeypatch):
    with guarded(monkeypatch, dev) as g:
        for shape in ((3, 5, 7), (5, 9, 33), (2, 3, 65), (8, 40, 40)):
            maps = blob_map(shape)
            md = g.put(torch.from_numpy(maps))
            for kw in (dict(), dict(min_voxels_detection=2, connectivity=1), dict(threshold=0.25)):
                want = Dt.extract_lesion_candidates(maps, **kw)
                got = Dt.extract_lesion_candidates(md, **kw)
                for a, w in zip(got, want):
                    assert np.array_equal(a.cpu().numpy(), w), (shape, kw)
                g.check()
        # the steps on their own, the per-sample peak of a volume whose length is no multiple of anything
        w = g.put(torch.from_numpy(blob_map((3, 5, 7))))
        st = ops.cc_state(3, dev)
        ops.cc_peak(w, st, reset=True)
        got = st.cpu().numpy()
        flat = blob_map((3, 5, 7)).reshape(3, -1)
        assert got[0].view(np.float32).tolist() == flat.max(axis=1).tolist() and got[1].tolist() == flat.argmax(axis=1).tolist()
        g.check()
