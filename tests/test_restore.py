"""Back-projection of a map on the network's grid onto the scan's own grid (csrc/restore.hip: m1_restore; ops.restore;
preprocess.restore_geometry / restore_host / restore; get_detect_model().predict_scan), the inverse of prepare_scan's geometry.

Yardsticks.  The reference ships no such step, so the pin is scipy: the fp64 host restatement (preprocess.restore_host) against
scipy.ndimage.map_coordinates(order=1, mode='nearest') on the real window of the network grid to 1e-13 of max|ref| (the bound of
test_resample.py's pin), order 0 against a direct np.take at floor(u + 0.5).  The order-1 kernel per element against that restatement
under

    |got - ref64| <= 4 * e32

where e32 is the error of the SAME restatement in fp32 values on the same input (coordinate, floor and fraction stay fp64, as in the
kernel) and 4 is test_resample.py's factor; e32 itself is capped (E32_CAP) so that the yardstick cannot grow unnoticed.  Order 0, the
label output against the prob output, one launch against two, NaN pads and predict_scan against the hand-written chain are bit-exact
statements.  The label output against fp64: equal to the argmax of ref64 wherever its top-two margin exceeds 8 * e32 (each of the two
values is within 4 * e32); the voxels that rule leaves out may be at most 0.1 % of the inside voxels, and on the committed seeds the
reference leaves out none (checked on the CPU).  Measured values: DESIGN.md section 7.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import m1_oracle as O
from util import C1_FILTERS, C1_STRIDES, PKG, build_m1, load_params_into, ops
from test_preprocess import U, as_bits, scan_like

P = PKG.preprocess
L = PKG.hip.lib

# (scan_shape, spacing, out_spacing, img_size) of the base geometries; OUTSIDE: (scan voxels, of which outside), computed by hand from
# scan_window / crop_or_pad_starts for G1-G5
G1 = ((7, 30, 41), (3.6, .3, .3), (3, .5, .5), (8, 16, 32))          # crop on axis 1, pad on axis 2 (lo = 3)
G2 = ((5, 9, 11), (3, .5, .5), (3.6, .3, .75), (4, 16, 8))
G3 = ((2, 3, 70), (1, 1, .5), (.5, .3, .77), (4, 10, 40))            # crop with first = 2
G4 = ((1, 7, 2), (3, .5, .5), (3, .4, .7), (2, 8, 4))                # axes of one real voxel
G5 = ((6, 33, 33), (3, .5, .5), (3, .5, .5), (6, 33, 33))            # identity
G6 = ((9, 37, 53), (3.6, .3, .3), (3, .5, .5), (8, 24, 32))
GEOMS = [G1, G2, G3, G4, G5, G6]
OUTSIDE = {0: (8610, 861), 1: (495, 45), 2: (420, 54), 3: (14, 8), 4: (6534, 0)}
# the lengths the kernel itself makes critical (csrc/restore.hip), B = 2 in the GPU tests:
#   RST_RUN = 4 voxels of the contiguous axis per lane: scan widths 1, 2, 3, 4, 5 (a short run alone, a whole run, a whole run and a short
#       one); with 1 to 2 runs per row a block of RST_NT = 256 threads holds 128 to 256 rows in its LDS row table;
#   RST_NT * RST_RUN = 1024 voxels, the stretch of a row one block covers: widths 1023, 1024 (256 runs: one block per row) and 1025 (257
#       runs: every block straddles two rows);
#   more than RST_NT rows at one run per row (a row table filled to its last entry, several blocks): 2 * 9 * 40 = 720 rows of width 3;
#   a row start that is not 16-byte aligned: odd w * nsel (G1: 41, G6: 53, the widths 1, 3, 5, 1023, 1025) with B = 2;
#   every (c0, nsel) of C = 1..4 runs on every geometry (nsel 1..4 are the kernel's four register-held store widths, M1_RESTORE_MAX_SEL =
#       4); C = 6 with nsel 5 and 6 takes the element-store path of wider selections, nsel 1 and 4 of C = 6 the label loops on both sides
#       of the selection.
WIDTHS = [((3, 5, w), (3, .5, .5), (3, .4, .7), (4, 6, 4)) for w in (1, 2, 3, 4, 5)]
TILE = [((1, 2, w), (3, .5, .25), (3, .5, .5), (3, 2, 500)) for w in (1023, 1024, 1025)]
ROWS = [((9, 40, 3), (3.6, .3, .3), (3, .5, .5), (12, 20, 4))]
GPU_GEOMS = GEOMS + WIDTHS + TILE + ROWS
LABEL_GEOMS = (0, 1, 2, 5)                                            # G1, G2, G3, G6
DEFAULT, DEFLABEL = -7.0, 9
CHANNELS = (1, 2, 3, 4, 6)
# e32 in units of 2^-24 max|ref64| on the committed inputs: the largest value measured on the CPU is 1.91; the cap
# is twice that
E32_MEASURED = 1.91
E32_CAP = 2 * E32_MEASURED


def prob_like(shape, seed):
    """Softmax over the last axis of seeded N(0, 2^2) logits (a sigmoid for one channel), fp32."""
    x = np.random.default_rng(seed).normal(0.0, 2.0, shape)
    if shape[-1] == 1:
        return (1.0 / (1.0 + np.exp(-x))).astype(np.float32)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)


def lab_like(shape, seed, dtype):
    """A label-like map for order 0: scan_like for fp32 / int16; int32 values far beyond the int16 range."""
    if dtype == np.int32:
        return scan_like(shape, seed, np.int16).astype(np.int32) * 1000
    return scan_like(shape, seed, dtype)


def host(pred, geo, **kw):
    """restore_host over a batch."""
    shape, sp, osp, _ = geo
    return np.stack([P.restore_host(v, shape, sp, osp, **kw) for v in pred])


def pad_mask(geo):
    """The (D,H,W) mask of the pad voxels of the network grid: outside [lo, lo + count) on any axis."""
    real = np.ones((), dtype=bool)
    for a, ax in enumerate(P.restore_geometry(*geo)):
        sh = [1, 1, 1]
        sh[a] = ax.size
        i = np.arange(ax.size)
        real = real & ((i >= ax.lo) & (i < ax.lo + ax.count)).reshape(sh)
    return ~np.broadcast_to(real, geo[3])


@functools.lru_cache(maxsize=None)
def case(gi, Cn):
    """(pred (2,*img_size,C) fp32, ref64 (2,*scan_shape,C), e32, inside) of GPU_GEOMS[gi]: computed once, shared by the CPU yardstick test
    and the GPU tests, never changed."""
    geo = GPU_GEOMS[gi]
    pred = prob_like((2, *geo[3], Cn), 3000 + 11 * gi + Cn)
    ref = host(pred, geo, default_value=DEFAULT, dtype=np.float64)
    r32 = host(pred, geo, default_value=DEFAULT, dtype=np.float32)
    assert r32.dtype == np.float32 and ref.dtype == np.float64
    inside = P.restore_inside(P.restore_geometry(*geo))
    for a in (pred, ref, inside):
        a.setflags(write=False)
    return pred, ref, float(np.abs(r32.astype(np.float64) - ref).max()), inside


def margin_rule(ref, inside, e32):
    """(argmax of ref64, the voxels where its top-two margin exceeds 8 * e32) over the inside voxels of a (B,d,h,w,C) reference."""
    top = np.sort(ref, axis=-1)
    sure = ((top[..., -1] - top[..., -2]) > 8 * e32) & inside
    return np.argmax(ref, axis=-1), sure


def device_geom(geo, order=1, default_value=DEFAULT, default_label=DEFLABEL):
    g = P.restore_geometry(*geo)
    return ops.restore_geom(geo[3], [a.n for a in g], [a.ratio for a in g], [a.first for a in g], [a.count for a in g], [a.lo for a in g],
                            order, default_value, default_label)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_geometry_is_built_from_the_forward_functions():
    for gi, geo in enumerate(GPU_GEOMS):
        shape, sp, osp, img = geo
        g = P.restore_geometry(*geo)
        window = P.scan_window(shape, sp, osp, img)
        steps = P.resample_steps(sp, osp)
        for a, ax in enumerate(g):
            assert (ax.n, ax.size) == (shape[a], img[a]) and (ax.first, ax.count) == window[a]
            assert ax.ratio == sp[a] / osp[a] and abs(ax.ratio * steps[a] - 1) <= 2 ** -52
            assert ax.lo == -P.crop_or_pad_starts((ax.count,), (img[a],))[0] and 0 <= ax.lo and ax.lo + ax.count <= img[a]
        inside = P.restore_inside(g)
        assert inside.shape == shape
        if gi in OUTSIDE:
            assert (inside.size, int((~inside).sum())) == OUTSIDE[gi], (geo, inside.size, (~inside).sum())
    g1, g3 = P.restore_geometry(*G1), P.restore_geometry(*G3)
    assert [a.lo for a in g1] == [0, 0, 3] and g1[1].first == 1 and g3[2].first == 2
    assert [a.count for a in P.restore_geometry(*G4)] == [1, 8, 1]


@pytest.mark.parametrize("gi", range(5))
def test_restatement_equals_scipy_on_the_real_window(gi):
    from scipy import ndimage
    geo = GEOMS[gi]
    shape, sp, osp, img = geo
    g = P.restore_geometry(*geo)
    pred = prob_like((*img, 2), 40 + gi)
    inside = P.restore_inside(g)
    us = [P.restore_coords(ax)[0] for ax in g]
    real = tuple(slice(ax.lo, ax.lo + ax.count) for ax in g)
    got = P.restore_host(pred, shape, sp, osp, default_value=DEFAULT)
    assert got.shape == (*shape, 2) and got.dtype == np.float64
    coords = np.stack(np.meshgrid(*us, indexing="ij"))
    for c in range(2):
        ref = ndimage.map_coordinates(pred[real + (c,)].astype(np.float64), coords, order=1, mode="nearest")
        ref = np.where(inside, ref, DEFAULT)
        err = float(np.abs(got[..., c] - ref).max()) / float(np.abs(ref).max())
        print(geo, c, f"max |restatement - scipy| = {err:.2e} max|ref|")
        assert err <= 1e-13
        # a volume without a channel axis is the channel on its own
        assert np.array_equal(P.restore_host(pred[..., c], shape, sp, osp, default_value=DEFAULT), got[..., c])
    assert np.array_equal(got[~inside], np.full(got[~inside].shape, DEFAULT))
    # order 0: a direct np.take at floor(u + 0.5), the dtype kept
    for dtype in (np.int16, np.float32):
        lab = scan_like((*img, 2), 50 + gi, dtype)
        want = lab
        for a, (ax, u) in enumerate(zip(g, us)):
            want = np.take(want, np.clip(np.floor(u + 0.5).astype(np.int64), 0, ax.count - 1) + ax.lo, axis=a)
        want = np.where(inside[..., None], want, dtype(-3))
        got0 = P.restore_host(lab, shape, sp, osp, order=0, default_value=-3)
        assert got0.dtype == dtype and np.array_equal(got0, want)
        assert np.array_equal(got0[~inside], np.full(got0[~inside].shape, dtype(-3)))


def test_properties_of_the_restatement():
    # identity geometry returns the input bit for bit, in both value types
    shape, sp, osp, img = G5
    pred = prob_like((*img, 3), 60)
    for dt in (np.float64, np.float32):
        ident = P.restore_host(pred, shape, sp, osp, dtype=dt)
        assert ident.dtype == dt and np.array_equal(ident.astype(np.float32).view(np.uint32), pred.view(np.uint32))
    assert np.array_equal(P.restore_host(scan_like(img, 61, np.int16), shape, sp, osp, order=0), scan_like(img, 61, np.int16))
    for geo in GEOMS:
        shape, sp, osp, img = geo
        inside = P.restore_inside(P.restore_geometry(*geo))
        # a constant stays that constant at every inside voxel and the default value outside, exactly.  In fp64 values a * (1 - y) +
        # a * y is a convex combination with three roundings per axis and may sit an ulp of fp64 from a (hence 1e-13 there); the
        # public result, rounded to fp32, is the constant itself
        got = P.restore_host(np.full(img, 123.25, np.float32), shape, sp, osp, default_value=DEFAULT)
        assert np.abs(got[inside] - 123.25).max() <= 1e-13 * 123.25 and (got[~inside] == DEFAULT).all()
        pub = P.restore(np.full(img, 123.25, np.float32), shape, sp, osp, default_value=DEFAULT)
        assert pub.dtype == np.float32 and np.array_equal(pub, np.where(inside, np.float32(123.25), np.float32(DEFAULT)))
        assert (P.restore_host(np.full(img, 5, np.int16), shape, sp, osp, order=0, default_value=2)[inside] == 5).all()
        # what the network predicted on padding cannot leak: NaN in every pad voxel changes no output bit
        pred = prob_like((*img, 2), 62)
        poisoned = pred.copy()
        poisoned[pad_mask(geo)] = np.nan
        if geo in (G1, G4, G6):
            assert pad_mask(geo).any()
        for order in (1, 0):
            a = P.restore_host(pred, shape, sp, osp, order=order, default_value=DEFAULT)
            b = P.restore_host(poisoned, shape, sp, osp, order=order, default_value=DEFAULT)
            assert np.isfinite(b).all() and np.array_equal(a.view(np.uint64 if order else np.uint32), b.view(np.uint64 if order else np.uint32))
    # an integer ratio: the network grid twice as coarse on axis 2 and nothing cropped -> the even scan indices are the network samples
    pred = prob_like((4, 6, 5), 63)
    got = P.restore_host(pred, (4, 6, 10), (3, .5, .5), (3, .5, 1.0))
    assert np.array_equal(got[:, :, 0:9:2], pred[:, :, :5].astype(np.float64)) and (got[:, :, 9] == 0).all()      # u = 4.5 is outside


@pytest.mark.parametrize("gi", range(len(GPU_GEOMS)))
def test_fp32_restatement_stays_below_the_cap_of_the_yardstick(gi):
    """e32 of exactly the inputs of the GPU accuracy test, in units of 2^-24 max|ref64|: the cap keeps the GPU test's bound 4 * e32 from
    growing unnoticed."""
    for Cn in CHANNELS:
        pred, ref, e32, inside = case(gi, Cn)
        unit = U * float(np.abs(ref).max())
        print(GPU_GEOMS[gi], Cn, f"e32 = {e32 / unit:.2f} x 2^-24 max|ref|")
        assert e32 / unit <= E32_CAP


@pytest.mark.parametrize("gi", LABEL_GEOMS)
def test_margin_rule_leaves_out_no_voxel_on_the_committed_seeds(gi):
    pred, ref, e32, inside = case(gi, 3)
    top = np.sort(ref[:, inside], axis=-1)
    margin = float((top[..., -1] - top[..., -2]).min())
    print(GPU_GEOMS[gi], f"smallest top-two margin {margin:.3e}, threshold 8 * e32 = {8 * e32:.3e}")
    _, sure = margin_rule(ref, inside, e32)
    assert int(sure.sum()) == 2 * int(inside.sum())


def test_public_restore_on_arrays():
    shape, sp, osp, img = G1
    pred = prob_like((2, *img, 3), 70)
    full = host(pred, G1, default_value=2.0)
    inside = P.restore_inside(P.restore_geometry(*G1))
    got = P.restore(pred, shape, sp, osp, default_value=2.0)
    assert got.dtype == np.float32 and np.array_equal(got, full.astype(np.float32))
    one, lab = P.restore(pred, shape, sp, osp, channels=1, labels=True, default_value=2.0, default_label=DEFLABEL)
    assert one.shape == (2, *shape, 1) and np.array_equal(one[..., 0], got[..., 1])
    assert lab.dtype == np.uint8 and np.array_equal(lab, np.where(inside, np.argmax(got, axis=-1), DEFLABEL))
    assert np.array_equal(P.restore(pred, shape, sp, osp, channels=(1, 3), default_value=2.0), got[..., 1:3])
    assert np.array_equal(P.restore(pred[0], shape, sp, osp, default_value=2.0), got[0])
    assert np.array_equal(P.restore(pred[0, ..., 2], shape, sp, osp, default_value=2.0), got[0, ..., 2])
    lab16 = scan_like((*img, 2), 71, np.int16)
    g0 = P.restore(lab16, shape, sp, osp, order=0, default_value=-3)
    assert g0.dtype == np.int16 and np.array_equal(g0, P.restore_host(lab16, shape, sp, osp, order=0, default_value=-3))
    import model.preprocess as alias
    assert alias is P and alias.restore is P.restore


def test_argument_errors():
    shape, sp, osp, img = G1
    pred = np.zeros(img, np.float32)
    for bad in (np.zeros((8, 16), np.float32), np.zeros((1, 1, 8, 16, 32, 2), np.float32)):                       # wrong ranks
        with pytest.raises(ValueError):
            P.restore(bad, shape, sp, osp)
    with pytest.raises(ValueError):
        P.restore_host(np.zeros((2, *img, 2), np.float32), shape, sp, osp)
    for bad_img in ((8, 16), (8, 0, 32), (8, 16, 32, 2)):                  # sizes prepare_scan could not have produced for any scan
        with pytest.raises(ValueError):
            P.restore_geometry(shape, sp, osp, bad_img)
    with pytest.raises(ValueError):
        P.restore_geometry((7, 30), sp, osp, img)
    with pytest.raises(ValueError):
        P.restore_geometry((1, 30, 41), (1, 1, 1), (4, 1, 1), img)         # the scan has no voxel at that spacing: prepare_scan raises too
    for bad_sp, bad_osp in (((3.6, 0, .3), osp), ((3.6, -.3, .3), osp), (sp, (3, .5, 0)), (sp, (3, .5)), (sp, (3, float("nan"), .5))):
        with pytest.raises(ValueError):
            P.restore(pred, shape, bad_sp, bad_osp)
    with pytest.raises(NotImplementedError):
        P.restore(pred, shape, sp, osp, order=3)
    for bad_ch in (2, (1, 1), (0, 3), -1, slice(0, 2, 2)):
        with pytest.raises(ValueError):
            P.restore(np.zeros((*img, 2), np.float32), shape, sp, osp, channels=bad_ch)
    with pytest.raises(ValueError):
        P.restore(pred, shape, sp, osp, labels=True, default_label=256)
    with pytest.raises(RuntimeError, match="GPU"):
        P.restore(torch.zeros(*img, 2), shape, sp, osp)


def _rgeom(src=(8, 16, 32), dst=(7, 30, 41), ratio=(1.2, .6, .6), first=(0, 1, 0), count=(8, 16, 25), lo=(0, 0, 3), order=1, deflabel=0):
    g = L.m1_restore_t()
    g.src[:], g.dst[:], g.ratio[:], g.first[:], g.count[:], g.lo[:], g.order, g.deflabel = src, dst, ratio, first, count, lo, order, deflabel
    return g


def test_c_entry_point_rejects_bad_arguments_without_a_gpu():
    lib = L.load()
    BAD, UNSUP = -1, -2
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    assert C.sizeof(L.m1_restore_t) == 96 and L.m1_restore_t.ratio.offset == 64

    def rs(src=p, sdt=0, geom=_rgeom(), B=1, Cn=2, c0=0, nsel=2, prob=p, label=p):
        return lib.m1_restore(src, sdt, C.byref(geom) if geom is not None else None, B, Cn, c0, nsel, prob, label, None)

    assert rs(src=None) == BAD and rs(geom=None) == BAD and rs(prob=None, label=None) == BAD
    assert rs(geom=L.m1_restore_t()) == BAD                                                # a zeroed geometry
    assert rs(B=0) == BAD and rs(Cn=0) == BAD and rs(Cn=-1) == BAD
    assert rs(c0=-1) == BAD and rs(c0=1, nsel=2) == BAD and rs(nsel=0) == BAD and rs(c0=2, nsel=1) == BAD
    assert rs(Cn=256, label=p) == BAD and rs(geom=_rgeom(deflabel=256)) == BAD and rs(geom=_rgeom(deflabel=-1)) == BAD
    assert rs(geom=_rgeom(lo=(0, 1, 3))) == BAD and rs(geom=_rgeom(lo=(0, 0, 8))) == BAD     # lo + count exceeds src
    assert rs(geom=_rgeom(lo=(0, -1, 3))) == BAD and rs(geom=_rgeom(count=(8, 0, 25))) == BAD and rs(geom=_rgeom(first=(0, -1, 0))) == BAD
    assert rs(geom=_rgeom(src=(8, 0, 32))) == BAD and rs(geom=_rgeom(dst=(7, 30, -1))) == BAD
    for order in (3, 2, -1):
        assert rs(geom=_rgeom(order=order)) == BAD
    assert rs(sdt=1) == BAD and rs(sdt=2) == BAD                                            # int16 / int32 with order 1
    for bad_ratio in (0.0, -1.0, float("nan"), float("inf")):
        assert rs(geom=_rgeom(ratio=(1.2, bad_ratio, .6))) == BAD
    assert rs(src=p + 2) == BAD and rs(prob=p + 2) == BAD and rs(src=p + 1, sdt=1, geom=_rgeom(order=0)) == BAD
    assert rs(sdt=3) == UNSUP and rs(sdt=-1) == UNSUP and (L.M1_RAW_F32, L.M1_RAW_I16, L.M1_RAW_I32) == (0, 1, 2)
    assert L.M1_RESTORE_MAX_SEL == 4
    assert rs(geom=_rgeom(dst=(2048, 1024, 1024))) == UNSUP                                 # 2^31 output voxels
    assert rs(geom=_rgeom(src=(1024, 1024, 1024), count=(8, 16, 25)), Cn=2) == UNSUP        # 2^31 source elements
    assert "m1_restore" in L.SIGNATURES


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
RANGES = {Cn: [(c0, n) for c0 in range(Cn) for n in range(1, Cn - c0 + 1)] for Cn in (1, 2, 3, 4)}
RANGES[6] = [(0, 6), (0, 5), (1, 5), (2, 1), (1, 4)]


def check_linear(got, ref, e32, inside, what):
    got = got.cpu().numpy().astype(np.float64)
    assert (got[:, ~inside] == DEFAULT).all(), what
    assert np.isfinite(got).all() and (np.abs(got - ref) <= 4 * e32).all(), (what, float(np.abs(got - ref).max()), e32)
    return float(np.abs(got - ref).max())


@pytest.mark.gpu
@pytest.mark.parametrize("Cn", CHANNELS)
def test_linear_restore_against_the_fp64_restatement(dev, Cn):
    worst = 0.0
    for gi, geo in enumerate(GPU_GEOMS):
        pred, ref, e32, inside = case(gi, Cn)
        pd, g = torch.from_numpy(pred).to(dev), device_geom(geo)
        for c0, nsel in RANGES[Cn]:
            got = ops.restore(pd, g, c0, nsel)
            assert got.dtype == torch.float32 and tuple(got.shape) == (2, *geo[0], nsel)
            err = check_linear(got, ref[..., c0:c0 + nsel], e32, inside, (geo, Cn, c0, nsel))
            worst = max(worst, err / e32 if e32 > 0 else 0.0)
        print(geo, f"C={Cn}: e32 = {e32 / (U * np.abs(ref).max()):.2f} x 2^-24 max|ref|")
    print(f"C={Cn}: largest max|got - ref64| / e32 = {worst:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", (np.int16, np.float32, np.int32))
def test_nearest_restore_is_the_host_gather_bit_for_bit(dev, dtype):
    bits = np.uint16 if dtype == np.int16 else np.uint32
    for gi, geo in enumerate(GPU_GEOMS):
        for Cn in CHANNELS:
            lab = lab_like((2, *geo[3], Cn), 80 + gi + Cn, dtype)
            want = host(lab, geo, order=0, default_value=-3)
            ld, g = torch.from_numpy(lab).to(dev), device_geom(geo, 0, -3)
            for c0, nsel in RANGES[Cn]:
                got = ops.restore(ld, g, c0, nsel)
                assert got.dtype == ld.dtype
                assert np.array_equal(got.cpu().numpy().view(bits), np.ascontiguousarray(want[..., c0:c0 + nsel]).view(bits)), (geo, Cn, c0, nsel)
            # the label output of a nearest launch is the argmax of what it stores
            got, lb = ops.restore(ld, g, 0, Cn, True, True)
            inside = P.restore_inside(P.restore_geometry(*geo))
            assert np.array_equal(lb.cpu().numpy(), np.where(inside, np.argmax(got.cpu().numpy(), axis=-1), DEFLABEL)), (geo, Cn)


@pytest.mark.gpu
@pytest.mark.parametrize("Cn", CHANNELS)
def test_labels_are_the_argmax_of_the_prob_output_and_one_launch_equals_two(dev, Cn):
    for gi, geo in enumerate(GPU_GEOMS):
        pred, ref, e32, inside = case(gi, Cn)
        pd, g = torch.from_numpy(pred).to(dev), device_geom(geo)
        prob, lab = ops.restore(pd, g, 0, Cn, True, True)
        assert lab.dtype == torch.uint8 and tuple(lab.shape) == (2, *geo[0])
        pn, ln = prob.cpu().numpy(), lab.cpu().numpy()
        assert (ln[:, ~inside] == DEFLABEL).all()
        assert np.array_equal(ln, np.where(inside, np.argmax(pn, axis=-1), DEFLABEL)), geo          # np.argmax: the first maximum
        # one launch with both outputs equals the two single-output launches, for every channel range
        only = ops.restore(pd, g, prob=False, label=True)
        assert torch.equal(only, lab)
        for c0, nsel in RANGES[Cn]:
            single = ops.restore(pd, g, c0, nsel)
            both, lb = ops.restore(pd, g, c0, nsel, True, True)
            assert torch.equal(as_bits(single), as_bits(both)) and torch.equal(lb, lab), (geo, c0, nsel)
            assert torch.equal(as_bits(single), as_bits(prob[..., c0:c0 + nsel])), (geo, c0, nsel)


@pytest.mark.gpu
@pytest.mark.parametrize("gi", LABEL_GEOMS)
def test_labels_against_the_fp64_argmax(dev, gi):
    geo = GPU_GEOMS[gi]
    pred, ref, e32, inside = case(gi, 3)
    want, sure = margin_rule(ref, inside, e32)
    lab = ops.restore(torch.from_numpy(pred).to(dev), device_geom(geo), prob=False, label=True).cpu().numpy()
    left_out = 2 * int(inside.sum()) - int(sure.sum())
    print(geo, f"{left_out} of {2 * int(inside.sum())} inside voxels left out by the margin rule")
    assert left_out <= 1e-3 * 2 * int(inside.sum())
    assert np.array_equal(lab[sure], want[sure]) and (lab[:, ~inside] == DEFLABEL).all()


@pytest.mark.gpu
def test_label_ties_go_to_the_lower_index(dev):
    for gi in (0, 3, 5, 7):
        geo = GPU_GEOMS[gi]
        pred = case(gi, 2)[0]
        inside = case(gi, 2)[3]
        g = device_geom(geo)
        twin = np.ascontiguousarray(pred[..., [0, 0]])                                   # two identical channels: 0 everywhere
        lab = ops.restore(torch.from_numpy(twin).to(dev), g, prob=False, label=True).cpu().numpy()
        assert (lab[:, inside] == 0).all() and (lab[:, ~inside] == DEFLABEL).all()
        trio = np.ascontiguousarray(pred[..., [0, 1, 1]])                                # the last two identical: never 2
        prob, lab = ops.restore(torch.from_numpy(trio).to(dev), g, 0, 3, True, True)
        pn, ln = prob.cpu().numpy(), lab.cpu().numpy()
        assert np.array_equal(pn[..., 1], pn[..., 2]) and (ln[:, inside] < 2).all() and (ln[:, inside] == 1).any()
        assert np.array_equal(ln[:, inside], (pn[..., 1] > pn[..., 0])[:, inside])


@pytest.mark.gpu
def test_nan_in_every_pad_voxel_changes_no_output_bit(dev):
    for gi, geo in enumerate(GPU_GEOMS):
        pads = pad_mask(geo)
        if not pads.any():
            continue
        pred = case(gi, 3)[0]
        poisoned = pred.copy()
        poisoned[:, pads] = np.nan
        for order in (1, 0):
            g = device_geom(geo, order)
            a, la = ops.restore(torch.from_numpy(pred).to(dev), g, 0, 3, True, True)
            b, lb = ops.restore(torch.from_numpy(poisoned).to(dev), g, 0, 3, True, True)
            assert bool(torch.isfinite(b).all()) and torch.equal(as_bits(a), as_bits(b)) and torch.equal(la, lb), (geo, order)


@pytest.mark.gpu
def test_public_restore_on_device_tensors(dev):
    shape, sp, osp, img = G6
    pred, ref, e32, inside = case(5, 3)
    pd = torch.from_numpy(pred).to(dev)
    got = P.restore(pd, shape, sp, osp, default_value=DEFAULT)
    check_linear(got, ref, e32, inside, "public")
    one, lab = P.restore(pd, shape, sp, osp, channels=1, labels=True, default_value=DEFAULT, default_label=DEFLABEL)
    assert tuple(one.shape) == (2, *shape, 1) and torch.equal(as_bits(one[..., 0]), as_bits(got[..., 1]))
    assert torch.equal(lab.cpu(), torch.from_numpy(np.where(inside, np.argmax(got.cpu().numpy(), axis=-1), DEFLABEL).astype(np.uint8)))
    assert torch.equal(as_bits(P.restore(pd[0], shape, sp, osp, default_value=DEFAULT)), as_bits(got[0]))
    assert torch.equal(as_bits(P.restore(pd[0, ..., 2], shape, sp, osp, default_value=DEFAULT)), as_bits(got[0, ..., 2]))
    for lab_in in (scan_like((*img, 2), 90, np.int16), (np.abs(scan_like(img, 91, np.int16)) % 3).astype(np.uint8)):   # uint8 goes through int16
        gl = P.restore(torch.from_numpy(lab_in).to(dev), shape, sp, osp, order=0, default_value=2)
        assert gl.dtype == torch.from_numpy(lab_in).dtype
        assert np.array_equal(gl.cpu().numpy(), P.restore(lab_in, shape, sp, osp, order=0, default_value=2))
    with pytest.raises(RuntimeError):
        ops.restore(pd, device_geom(G1))                                                  # a geometry for another source
    # channels=None of a map with more channels than the kernel's register-held selections
    p6, r6, e6, _ = case(5, 6)
    check_linear(P.restore(torch.from_numpy(p6).to(dev), shape, sp, osp, default_value=DEFAULT), r6, e6, inside, "public C = 6")


@pytest.mark.gpu
def test_public_nearest_restore_keeps_dtype_and_values_like_the_host_path(dev):
    """Order 0 moves values unchanged: every dtype the device path accepts gives what the numpy path gives, and a dtype without an exact
    route raises instead of truncating or wrapping."""
    shape, sp, osp, img = G1
    base = scan_like((*img, 2), 92, np.int16)
    big = base.astype(np.int32) * 1000                                                    # far beyond the int16 range
    assert big.max() > 32767 and big.min() < -32768
    conf = (base.astype(np.float32) / 1024).astype(np.float16)                            # fractions: 0.7 must not become 0
    assert (conf.astype(np.float32) % 1 != 0).any()
    for arr, dv in ((big, -70000), (big.astype(np.int32)[..., 0], 3), (conf, 0.5), (base.astype(np.int8), -3), (base % 7 == 0, 1),
                    (np.abs(base % 251).astype(np.uint8), 2), (base, -3), (base.astype(np.float32) / 3, 0.25)):
        want = P.restore(arr, shape, sp, osp, order=0, default_value=dv)
        got = P.restore(torch.from_numpy(arr).to(dev), shape, sp, osp, order=0, default_value=dv)
        assert got.dtype == torch.from_numpy(arr).dtype and tuple(got.shape) == want.shape
        assert np.array_equal(got.cpu().numpy(), want), arr.dtype
    bf = torch.from_numpy(conf.astype(np.float32)).to(torch.bfloat16)                     # numpy has no bfloat16: against its fp32 values
    got = P.restore(bf.to(dev), shape, sp, osp, order=0, default_value=0.5)
    want = P.restore(bf.float().numpy(), shape, sp, osp, order=0, default_value=0.5)
    assert got.dtype == torch.bfloat16 and np.array_equal(got.float().cpu().numpy(), want)
    for bad in (torch.float64, torch.int64):
        with pytest.raises(ValueError, match="exact"):
            P.restore(torch.from_numpy(base).to(dev).to(bad), shape, sp, osp, order=0)
    with pytest.raises(ValueError, match="2\\^24"):
        P.restore(torch.from_numpy(big).to(dev), shape, sp, osp, order=0, default_value=2 ** 25)
    # order 1 of any type computes in fp32 from the fp32-rounded input, as the numpy path does
    d64 = torch.from_numpy(conf.astype(np.float64) / 3)
    got = P.restore(d64.to(dev), shape, sp, osp)
    ref, r32 = (P.restore_host(d64.numpy(), shape, sp, osp, dtype=t) for t in (np.float64, np.float32))
    assert got.dtype == torch.float32 and (np.abs(got.cpu().numpy() - ref) <= 4 * np.abs(r32 - ref).max()).all()


# ---- predict_scan: the smallest model of test_mc_inference.py, a scan of (5,44,50) at (3.6,.4,.4) -> (6,35,40) at (3,.5,.5) -> (4,32,32)
DIMS = (4, 32, 32)
SCAN, SCAN_SP, NET_SP = (5, 44, 50), (3.6, .4, .4), (3, .5, .5)


def _cfg():
    return O.M1Config(input_spatial_dims=DIMS, filters=C1_FILTERS, strides=C1_STRIDES, dense_skip=True, probabilistic=True,
                      prob_latent_dims=(3, 2, 1, 0), dropout_rate=0.5, dropout_mode="monte-carlo")


def _equal_dict(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], dict):
            _equal_dict(a[k], b[k])
        else:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(as_bits(a[k].float()), as_bits(b[k].float())), k


@pytest.mark.gpu
def test_predict_scan_equals_the_hand_written_chain(dev):
    cfg = _cfg()
    m = build_m1(cfg, dev)
    load_params_into(m, O.fixture_params(cfg, seed=61))
    m.eval()
    dm = m.get_detect_model()
    raw = torch.from_numpy(scan_like((2, *SCAN, 3), 95, np.int16)).to(dev)
    assert P.resample_size(SCAN, SCAN_SP, NET_SP) == (6, 35, 40)
    x, _ = P.prepare_scan(raw, SCAN_SP, NET_SP, DIMS, percentile=99.5)
    # one draw: predict
    m.seed_dropout(51)
    net = dm.predict(x)
    mean, lab = P.restore(net, SCAN, SCAN_SP, NET_SP, channels=1, labels=True)
    m.seed_dropout(51)
    r = dm.predict_scan(raw, SCAN_SP, NET_SP, percentile=99.5, channels=1, labels=True)
    assert tuple(r["mean"].shape) == (2, *SCAN, 1) and tuple(r["labels"].shape) == (2, *SCAN) and "entropy" not in r
    _equal_dict(r, {"mean": mean, "labels": lab, "network": net})
    # four draws: predict_mc, with the entropy
    m.seed_dropout(52)
    net = dm.predict_mc(x, 4, 2)
    want = {"mean": P.restore(net["mean"], SCAN, SCAN_SP, NET_SP), "entropy": P.restore(net["entropy"].unsqueeze(-1), SCAN, SCAN_SP, NET_SP)[..., 0],
            "network": net}
    m.seed_dropout(52)
    r = dm.predict_scan(raw, SCAN_SP, NET_SP, n_draws=4, draws_per_pass=2, percentile=99.5)
    assert tuple(r["mean"].shape) == (2, *SCAN, 2) and tuple(r["entropy"].shape) == (2, *SCAN) and int(m.rng_state[1]) == 2
    _equal_dict(r, want)
    inside = P.restore_inside(P.restore_geometry(SCAN, SCAN_SP, NET_SP, DIMS))
    assert not inside.all() and (r["mean"].cpu().numpy()[:, ~inside] == 0).all()


@pytest.mark.gpu
def test_predict_scan_of_a_cascaded_model_returns_both_stages(dev):
    cfg = _cfg()
    m = build_m1(cfg, dev, cascaded="noisy-or")
    params = O.fixture_params(cfg, seed=65, shapes=O.cascade_param_shapes(cfg))
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if k != "rng_state":
                v.copy_(params[k.replace("m1_stage", "stage")].to(v.device, v.dtype))
    m.eval()
    dm = m.get_detect_model()
    raws = [torch.from_numpy(scan_like((2, *SCAN, 3), 96 + k, np.int16)).to(dev) for k in range(2)]
    xs = [P.prepare_scan(r, SCAN_SP, NET_SP, DIMS)[0] for r in raws]
    m.seed_dropout(53)
    nets = dm.predict_mc(xs, 2)
    want = [{"mean": P.restore(n["mean"], SCAN, SCAN_SP, NET_SP, channels=1), "entropy": P.restore(n["entropy"].unsqueeze(-1), SCAN, SCAN_SP, NET_SP)[..., 0],
             "network": n} for n in nets]
    m.seed_dropout(53)
    r = dm.predict_scan({"image_1": raws[0], "image_2": raws[1]}, SCAN_SP, NET_SP, n_draws=2, channels=1)
    assert isinstance(r, list) and len(r) == 2
    for got, w in zip(r, want):
        _equal_dict(got, w)
