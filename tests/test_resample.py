"""Resampling to a target spacing (csrc/resample.hip: m1_resample; ops.resample; preprocess.resample_size / resample_host / resample /
prepare_scan), the reference's resample_img (P:52-71) on a plain array.

Yardsticks.  SimpleITK is not installed, so parity with ITK itself is NOT pinned.  Pinned instead: the fp64 host restatement
(preprocess.resample_host) against scipy.ndimage's spline_filter + map_coordinates (mode 'mirror', the same Unser / Thevenaz algorithm)
to 1e-13 of max|ref|; the cubic kernels per element against that restatement under

    |got - ref64| <= 4 * e32

where e32 is the error of the SAME restatement in fp32 values on the same input (coordinate, floor and fraction stay fp64, as in the
kernels) and 4 is the factor of test_preprocess.py for a different but equally long order of fp32 operations; e32 itself is capped
(E32_CAP) so that the yardstick cannot grow unnoticed.  The nearest path, windows and the fused prepare_scan are bit-exact statements.
The kernel's truncated causal start (24 terms, 2.6e-14 of max|src|) is far inside the bound.  Measured values: DESIGN.md section 7.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from util import PKG, ops
from test_preprocess import K_CLIP, K_PLAIN, U, as_bits, scan_like

P = PKG.preprocess
L = PKG.hip.lib

# (shape, spacing, out_spacing) of the restatement's pin: down- and up-sampling mixed, an axis of length 1, up-sampling that puts
# default voxels into the output (585 of 1800 in the fourth), identity spacing
GEOMS = [((5, 9, 11), (3, .5, .5), (3.6, .3, .75)), ((1, 7, 2), (3, .5, .5), (3, .4, .7)), ((19, 40, 37), (3.6, .3, .3), (3, .5, .5)),
         ((2, 3, 70), (1, 1, .5), (.5, .3, .77)), ((6, 33, 33), (3, .5, .5), (3, .5, .5))]
# lengths 1, 2 and 3 on every axis in turn
SMALL = [(tuple(n if a == ax else v for a, v in enumerate((4, 5, 6))), (3, .5, .5), (2.4, .7, .4)) for n in (1, 2, 3) for ax in range(3)]
# the lengths the kernels themselves make critical (csrc/resample.hip), B = 2 in the GPU tests:
#   RS_ROWS = 64 rows per LDS tile of the contiguous-axis kernel (pitch 33..36 at w = 9): 62, 64 and 66 rows -- a short last tile, none,
#       a last tile of two rows (the guard-band tests add 63 and 65 rows with B = 1);
#   RS_LDS_FLOATS = 12288: at w = 1024 (M1_RESAMPLE_MAX_LINE, a line at the limit) the tile holds 11, 3 and 2 rows for C = 1, 3, 4;
#   RS_HORIZON = 24, the closed-form / truncated causal start: 23, 24, 25 on every axis;
#   RS_SHORT = 32, the LDS / workspace switch of the strided passes: 31, 32, 33 on axes 0 and 1; a strided line at the limit
KERNEL = [((1, 31, 9), (3, .5, .5), (3, .4, .7)), ((4, 8, 9), (3, .5, .5), (2.5, .6, .4)), ((3, 11, 9), (3, .5, .5), (3.5, .4, .6)),
          ((2, 3, 1024), (3, .5, .3), (3, .5, 1.2)), ((23, 24, 25), (3, .5, .5), (3.6, .4, .6)), ((25, 23, 24), (3, .5, .5), (2.5, .6, .4)),
          ((24, 25, 23), (3, .5, .5), (3.3, .45, .55)), ((31, 32, 33), (3, .5, .5), (3.6, .7, .4)), ((33, 31, 32), (3, .5, .5), (2.5, .6, .9)),
          ((32, 33, 31), (3, .5, .5), (4, .4, .6)), ((1024, 2, 3), (.3, 1, 1), (1.1, 1, .8)), ((2, 1024, 3), (1, .3, 1), (.8, 1.3, 1))]
GPU_GEOMS = GEOMS + SMALL + KERNEL
DEFAULT = -7.0
# e32 in units of 2^-24 max|ref64| on the committed inputs: the largest value measured on the CPU is 11.2; the cap
# is twice that
E32_MEASURED = 11.2
E32_CAP = 2 * E32_MEASURED


def scipy_pair(vol, spacing, out_spacing, default):
    """scipy.ndimage's spline_filter + map_coordinates on a (z,x,y) volume, the inside rule applied to its result."""
    from scipy import ndimage
    steps = [o / s for s, o in zip(spacing, out_spacing)]
    size = P.resample_size(vol.shape, spacing, out_spacing)
    xs = [np.arange(n, dtype=np.float64) * st for n, st in zip(size, steps)]
    inside = np.ones(size, dtype=bool)
    for a, (x, n) in enumerate(zip(xs, vol.shape)):
        shape = [1, 1, 1]
        shape[a] = x.size
        inside &= ((x >= -0.5) & (x < n - 0.5)).reshape(shape)
    coef = ndimage.spline_filter(vol.astype(np.float32).astype(np.float64), order=3, mode="mirror")
    got = ndimage.map_coordinates(coef, np.stack(np.meshgrid(*xs, indexing="ij")), order=3, mode="mirror", prefilter=False)
    return np.where(inside, got, default), inside


@functools.lru_cache(maxsize=None)
def case(gi, dtype_name, Cn):
    """(raw (2,d,h,w,C), ref64, e32) of GPU_GEOMS[gi]: computed once, shared by the CPU yardstick test and the GPU tests, never changed."""
    shape, sp, osp = GPU_GEOMS[gi]
    raw = scan_like((2, *shape, Cn), 1000 + 7 * gi + Cn, np.dtype(dtype_name).type)
    ref = np.stack([P.resample_host(raw[b], sp, osp, default_value=DEFAULT, dtype=np.float64) for b in range(2)])
    r32 = np.stack([P.resample_host(raw[b], sp, osp, default_value=DEFAULT, dtype=np.float32) for b in range(2)])
    assert r32.dtype == np.float32
    for a in (raw, ref):
        a.setflags(write=False)
    return raw, ref, float(np.abs(r32.astype(np.float64) - ref).max())


def inside_mask(shape, sp, osp):
    size = P.resample_size(shape, sp, osp)
    m = np.ones(size, dtype=bool)
    for a in range(3):
        x = np.arange(size[a]) * (osp[a] / sp[a])
        sh = [1, 1, 1]
        sh[a] = size[a]
        m &= ((x >= -0.5) & (x < shape[a] - 0.5)).reshape(sh)
    return m


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gi", range(len(GEOMS) + len(SMALL)))
def test_restatement_equals_the_scipy_pair(gi):
    shape, sp, osp = (GEOMS + SMALL)[gi]
    vol = scan_like(shape, 50 + gi)
    default = 41.5 if shape == (2, 3, 70) else 0
    ref, inside = scipy_pair(vol, sp, osp, default)
    got = P.resample_host(vol, sp, osp, default_value=default, dtype=np.float64)
    assert got.shape == ref.shape == P.resample_size(shape, sp, osp) and got.dtype == np.float64
    assert np.array_equal(inside, inside_mask(shape, sp, osp))
    assert np.array_equal(got[~inside], np.full((~inside).sum(), float(default)))
    if shape == (2, 3, 70):
        assert got.size == 1800 and (~inside).sum() == 585
    err = float(np.abs(got - ref).max()) / float(np.abs(ref).max())
    print(shape, sp, osp, f"max |restatement - scipy| = {err:.2e} max|ref|")
    assert err <= 1e-13
    # a channel axis is carried along
    v4 = np.stack([vol, vol[::-1, ::-1, ::-1]], axis=-1)
    g4 = P.resample_host(v4, sp, osp, default_value=default)
    assert np.array_equal(g4[..., 0], got) and np.array_equal(g4[..., 1], P.resample_host(v4[..., 1], sp, osp, default_value=default))


def test_properties_of_the_restatement():
    shape, sp = (5, 9, 11), (3, .5, .5)
    vol = scan_like(shape, 60)
    # a constant stays that constant; identity spacing returns the samples
    for osp in ((3.6, .3, .75), (2, .7, .4)):
        got = P.resample_host(np.full(shape, 123.25, np.float32), sp, osp)
        assert np.abs(got - 123.25)[inside_mask(shape, sp, osp)].max() <= 1e-13 * 123.25 and not got[~inside_mask(shape, sp, osp)].any()
    ident = P.resample_host(vol, sp, sp)
    assert ident.shape == shape and np.abs(ident - vol).max() <= 1e-13 * np.abs(vol).max()
    # where j * step is an integer the output is the sample there: step 2 on axis 2, 0.5 on axis 1 (every second output), 1 on axis 0
    got = P.resample_host(vol, sp, (3, .25, 1.0))
    assert got.shape == (5, 18, 6)                                   # round(5.5) = 6, half to even
    want = vol[:, :, ::2]
    assert np.abs(got[:, ::2, :] - want).max() <= 1e-13 * np.abs(vol).max()
    # a window is the slice of the full result, exactly
    osp = (2.5, .3, .75)
    full = P.resample_host(vol, sp, osp, default_value=3)
    assert full.shape == (6, 15, 7)
    for win in (((0, 6), (0, 15), (0, 7)), ((1, 4), (3, 9), (2, 5)), ((5, 1), (14, 1), (0, 1))):
        sl = tuple(slice(f, f + c) for f, c in win)
        for dt in (np.float64, np.float32):
            assert np.array_equal(P.resample_host(vol, sp, osp, default_value=3, dtype=dt, window=win),
                                  P.resample_host(vol, sp, osp, default_value=3, dtype=dt)[sl])
        assert np.array_equal(P.resample_host(vol, sp, osp, is_label=True, default_value=3, window=win),
                              P.resample_host(vol, sp, osp, is_label=True, default_value=3)[sl])
    for bad in (((0, 7), (0, 15), (0, 7)), ((-1, 2), (0, 15), (0, 7)), ((0, 6), (15, 1), (0, 7)), ((0, 6), (0, 15))):
        with pytest.raises(ValueError):
            P.resample_host(vol, sp, osp, window=bad)
    # the public numpy path: fp64 compute, fp32 out
    pub = P.resample(vol, sp, osp, default_value=3)
    assert pub.dtype == np.float32 and np.array_equal(pub, full.astype(np.float32))


def test_resample_size_is_the_reference_expression():
    for shape, sp, osp in GPU_GEOMS + [((5, 5, 3), (1, 1, 1), (2, 2, 2))]:
        want = tuple(int(np.round(n * (s / o))) for n, s, o in zip(shape, sp, osp))
        assert P.resample_size(shape, sp, osp) == want
    assert P.resample_size((5, 7, 3), (1, 1, 1), (2, 2, 2)) == (2, 4, 2)            # 2.5 -> 2, 3.5 -> 4, 1.5 -> 2: half to even
    with pytest.raises(ValueError):
        P.resample_size((1, 5, 5), (1, 1, 1), (2, 1, 1))                              # round(0.5) = 0
    with pytest.raises(ValueError):
        P.resample_size((5, 5), (1, 1, 1), (2, 2, 2))


@pytest.mark.parametrize("dtype", (np.int16, np.float32))
def test_nearest_path_is_np_take_at_round_half_up(dtype):
    # step 0.5 on axes 0 and 2 puts every second coordinate exactly on k + 0.5: floor(x + 0.5) = k + 1; axis 1 shrinks
    for shape, sp, osp in GEOMS + [((4, 7, 5), (1, 1, 1), (.5, 1.3, .5))]:
        lab = scan_like(shape + (2,), 70, dtype)
        got = P.resample_host(lab, sp, osp, is_label=True, default_value=-3)
        assert got.dtype == dtype
        want = lab
        size = P.resample_size(shape, sp, osp)
        for a in range(3):
            x = np.arange(size[a]) * (osp[a] / sp[a])
            want = np.take(want, np.minimum(np.floor(x + 0.5).astype(np.int64), shape[a] - 1), axis=a)
        want = np.where(inside_mask(shape, sp, osp)[..., None], want, dtype(-3))
        assert np.array_equal(got.view(np.uint16 if dtype == np.int16 else np.uint32), want.view(np.uint16 if dtype == np.int16 else np.uint32))
        assert np.array_equal(P.resample(lab, sp, osp, is_label=True, default_value=-3), got)
    x = np.arange(8) * 0.5
    assert (x[1::2] % 1 == 0.5).all()                                                  # the half-way coordinates are in the data above


@pytest.mark.parametrize("gi", range(len(GPU_GEOMS)))
def test_fp32_restatement_stays_below_the_cap_of_the_yardstick(gi):
    """e32 of exactly the inputs of the GPU accuracy test, in units of 2^-24 max|ref64|: the cap keeps the GPU test's bound 4 * e32 from
    growing unnoticed."""
    worst = 0.0
    for dtype in ("int16", "float32"):
        for Cn in (1, 3, 4):
            raw, ref, e32 = case(gi, dtype, Cn)
            unit = U * float(np.abs(ref).max())
            worst = max(worst, e32 / unit)
            print(GPU_GEOMS[gi], dtype, Cn, f"e32 = {e32 / unit:.2f} x 2^-24 max|ref|")
            assert e32 / unit <= E32_CAP
    print("largest:", worst)


def _rgeom(src=(5, 9, 11), dst=(4, 15, 7), first=(0, 0, 0), step=(1.2, 0.6, 1.5), order=3, defval=0.0):
    g = L.m1_resample_t()
    g.src[:], g.dst[:], g.first[:], g.step[:], g.order, g.defval = src, dst, first, step, order, defval
    return g


def test_c_entry_points_reject_bad_arguments_without_a_gpu():
    lib = L.load()
    BAD, UNSUP = -1, -2
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    g = _rgeom()

    def rs(src=p, sdt=0, geom=g, B=1, Cn=1, out=p, odt=0, ws=p):
        return lib.m1_resample(src, sdt, C.byref(geom) if geom is not None else None, B, Cn, out, odt, ws, None)

    assert rs(src=None) == BAD and rs(out=None) == BAD and rs(ws=None) == BAD and rs(geom=None) == BAD
    assert rs(B=0) == BAD and rs(Cn=0) == BAD and rs(Cn=-2) == BAD
    assert rs(geom=_rgeom(src=(0, 9, 11))) == BAD and rs(geom=_rgeom(dst=(4, -1, 7))) == BAD and rs(geom=_rgeom(first=(0, -1, 0))) == BAD
    for bad_step in (0.0, -1.0, float("nan"), float("inf")):
        assert rs(geom=_rgeom(step=(1.2, bad_step, 1.5))) == BAD
    assert rs(src=p + 2) == BAD and rs(src=p + 1, sdt=1) == BAD and rs(out=p + 2) == BAD and rs(ws=p + 8) == BAD
    assert rs(sdt=2) == UNSUP and rs(sdt=-1) == UNSUP and rs(odt=1) == UNSUP and rs(odt=5) == UNSUP
    assert rs(geom=_rgeom(order=1)) == UNSUP and rs(geom=_rgeom(order=-3)) == UNSUP
    assert rs(Cn=9) == UNSUP
    assert rs(geom=_rgeom(dst=(2048, 1024, 1024))) == UNSUP                            # 2^31 outputs
    assert rs(geom=_rgeom(src=(1024, 1024, 1024), dst=(1, 1, 2048))) == UNSUP          # 2^31 elements after the pass over axis 2
    assert L.M1_RESAMPLE_MAX_LINE >= 1024
    for ax in range(3):
        src = [5, 9, 11]
        src[ax] = L.M1_RESAMPLE_MAX_LINE + 1
        assert rs(geom=_rgeom(src=tuple(src))) == UNSUP                                # an axis beyond the line limit
    # order 0 keeps the type and needs no workspace: a mismatching output type is refused
    assert rs(geom=_rgeom(order=0), sdt=1, odt=0, ws=None) == UNSUP and rs(geom=_rgeom(order=0), sdt=0, odt=1, ws=None) == UNSUP
    # the workspace query is pure host: 4 * (roundup4(B*C*src0*src1*dst2) + B*C*src0*dst1*dst2) bytes
    q = lambda geom, B, Cn: int(lib.m1_resample_ws_bytes(C.byref(geom), B, Cn))
    assert q(g, 2, 3) == 4 * ((2 * 3 * 5 * 9 * 7 + 3) // 4 * 4 + 2 * 3 * 5 * 15 * 7) == 20168
    big = _rgeom(src=(24, 384, 384), dst=(20, 160, 160), first=(4, 35, 35), step=(5 / 6, 5 / 3, 5 / 3))
    assert q(big, 2, 1) == 4 * (2 * 24 * 384 * 160 + 2 * 24 * 160 * 160) == 16711680
    assert q(g, 0, 1) == 0 and q(g, 1, 9) == 0 and q(_rgeom(order=2), 1, 1) == 0 and q(_rgeom(order=0), 1, 1) == 0
    assert q(_rgeom(step=(1.2, 0.0, 1.5)), 1, 1) == 0 and int(lib.m1_resample_ws_bytes(None, 1, 1)) == 0


def test_public_surface():
    with pytest.raises(NotImplementedError, match="SimpleITK"):
        P.resample_img(None)
    with pytest.raises(NotImplementedError, match="resample"):
        P.resample_img(None)
    import model.preprocess as alias
    assert alias is P and alias.resample is P.resample
    with pytest.raises(RuntimeError, match="GPU"):
        P.prepare_scan(torch.zeros(1, 3, 3, 3, 1), (3, .5, .5), (3, .5, .5), (4, 4, 4))
    with pytest.raises(ValueError):
        P.prepare_scan(np.zeros((1, 3, 3, 3, 1), np.float32), (3, .5, .5), (3, .5, .5), (4, 4, 4))
    with pytest.raises(ValueError):
        P.resample(np.zeros((3, 3)), (1, 1), (1, 1))
    with pytest.raises(ValueError):
        P.resample(np.zeros((3, 3, 3)), (1, 1, 0), (1, 1, 1))
    assert P.scan_window((24, 384, 384), (3.6, .3, .3), (3, .5, .5), (20, 160, 160)) == ((4, 20), (35, 160), (35, 160))   # of (29, 230, 230)
    assert P.scan_window((5, 9, 11), (3, .5, .5), (3, .5, .5), (8, 9, 4)) == ((0, 5), (0, 9), (3, 4))


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def steps_of(sp, osp):
    return [o / s for s, o in zip(sp, osp)]


@pytest.mark.gpu
@pytest.mark.parametrize("Cn", (1, 3, 4))
@pytest.mark.parametrize("dtype", ("int16", "float32"))
def test_cubic_resampling_against_the_fp64_restatement(dev, dtype, Cn):
    worst = 0.0
    for gi, (shape, sp, osp) in enumerate(GPU_GEOMS):
        raw, ref, e32 = case(gi, dtype, Cn)
        size = P.resample_size(shape, sp, osp)
        got = ops.resample(torch.from_numpy(raw).to(dev), steps_of(sp, osp), size, default_value=DEFAULT)
        assert got.dtype == torch.float32 and tuple(got.shape) == (2, *size, Cn)
        got = got.cpu().numpy().astype(np.float64)
        outside = ~inside_mask(shape, sp, osp)
        assert (got[:, outside] == DEFAULT).all(), (shape, sp, osp)
        err = float(np.abs(got - ref).max())
        ratio = err / e32 if e32 > 0 else 0.0
        worst = max(worst, ratio)
        print(shape, sp, osp, f"max |got - ref64| = {err / (U * np.abs(ref).max()):.2f} x 2^-24 max|ref|, {ratio:.2f} e32")
        assert np.isfinite(got).all() and (np.abs(got - ref) <= 4 * e32).all(), (shape, sp, osp, err, e32)
    print(f"{dtype} C={Cn}: largest max|got - ref64| / e32 = {worst:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", (np.int16, np.float32))
def test_nearest_resampling_is_the_host_gather_bit_for_bit(dev, dtype):
    for shape, sp, osp in GEOMS + SMALL + KERNEL[:4] + [((4, 7, 5), (1, 1, 1), (.5, 1.3, .5))]:       # the last: coordinates on k + 0.5
        for Cn in (1, 3):
            lab = scan_like((2, *shape, Cn), 80 + Cn, dtype)
            want = np.stack([P.resample_host(lab[b], sp, osp, is_label=True, default_value=-3) for b in range(2)])
            got = ops.resample(torch.from_numpy(lab).to(dev), steps_of(sp, osp), P.resample_size(shape, sp, osp), order=0, default_value=-3)
            assert got.dtype == torch.from_numpy(lab).dtype
            bits = np.uint16 if dtype == np.int16 else np.uint32
            assert np.array_equal(got.cpu().numpy().view(bits), want.view(bits)), (shape, sp, osp, Cn)


@pytest.mark.gpu
def test_a_window_is_the_slice_of_the_full_result_and_calls_repeat(dev):
    for gi in (0, 2, 3, len(GEOMS) + len(SMALL) + 7):
        shape, sp, osp = GPU_GEOMS[gi]
        for dtype, Cn in (("int16", 1), ("float32", 3)):
            rd = torch.from_numpy(case(gi, dtype, Cn)[0]).to(dev)
            size = P.resample_size(shape, sp, osp)
            full = ops.resample(rd, steps_of(sp, osp), size, default_value=DEFAULT)
            assert torch.equal(as_bits(full), as_bits(ops.resample(rd, steps_of(sp, osp), size, default_value=DEFAULT)))
            first = [n // 3 for n in size]
            count = [max(1, n - f - n // 4) for n, f in zip(size, first)]
            sl = (slice(None),) + tuple(slice(f, f + c) for f, c in zip(first, count))
            for order in (3, 0):
                f = full if order == 3 else ops.resample(rd, steps_of(sp, osp), size, order=0, default_value=DEFAULT)
                win = ops.resample(rd, steps_of(sp, osp), count, first, order=order, default_value=DEFAULT)
                assert torch.equal(win, f[sl].contiguous()) and torch.equal(as_bits(win.float()), as_bits(f[sl].contiguous().float()))
            g = ops.resample_geom(shape, steps_of(sp, osp), count, first, 3, DEFAULT)                 # the ready geometry
            assert torch.equal(as_bits(ops.resample(rd, g)), as_bits(full[sl].contiguous()))


# raw (d,h,w), spacing, out_spacing -> resampled (6,17,18); img_size: every axis cropped, every axis padded, mixed
SCAN = ((6, 20, 22), (3, .5, .5), (3, .6, .6))
SCAN_SIZES = ((4, 12, 12), (8, 20, 20), (4, 20, 12))


def chain_host(raw, sp, osp, img, p, vt):
    B, Cn = raw.shape[0], raw.shape[-1]
    out = np.zeros((B, *img, Cn), vt)
    for b in range(B):
        for c in range(Cn):
            vol = P.resample_host(raw[b, ..., c], sp, osp, dtype=vt)
            vol = P.crop_pad_host(vol, img, P.crop_or_pad_starts(vol.shape, img), "constant", 0)
            out[b, ..., c] = P.whitening_host(vol, p, vt)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ("int16", "float32"))
def test_prepare_scan_equals_resample_then_prepare_input(dev, dtype):
    shape, sp, osp = SCAN
    assert P.resample_size(shape, sp, osp) == (6, 17, 18)
    raw = scan_like((2, *shape, 2), 90, np.dtype(dtype).type)
    rd = torch.from_numpy(raw).to(dev)
    full = ops.resample(rd, steps_of(sp, osp), (6, 17, 18))
    for img in SCAN_SIZES:
        for p in (None, 99.5):
            want, wstats = P.prepare_input(full, img, percentile=p)
            out, stats = P.prepare_scan(rd, sp, osp, img, percentile=p)
            assert out.dtype == torch.float32 and tuple(out.shape) == (2, *img, 2)
            assert torch.equal(as_bits(out), as_bits(want)) and torch.equal(stats, wstats), (img, p)
            ob, sb = P.prepare_scan(rd, sp, osp, img, percentile=p, dtype=torch.bfloat16)
            wb, _ = P.prepare_input(full, img, percentile=p, dtype=torch.bfloat16)
            assert ob.dtype == torch.bfloat16 and torch.equal(as_bits(ob), as_bits(wb)) and torch.equal(sb, wstats)
            # against the fp64 chain, under the whitening bound of test_preprocess.py with e32 from the same chain in fp32
            ref = chain_host(raw, sp, osp, img, p, np.float64)
            e32 = float(np.abs(chain_host(raw, sp, osp, img, p, np.float32).astype(np.float64) - ref).max())
            unit = U * float(np.abs(ref).max())
            err, bound = float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max()), max((K_PLAIN if p is None else K_CLIP) * unit, 4 * e32)
            print(f"{img} {dtype} p={p}: max |out - ref64| = {err / unit:.2f} x 2^-24 max|out|, e32 = {e32 / unit:.2f}")
            assert err <= bound, (img, p, err, bound)


@pytest.mark.gpu
def test_prepare_scan_is_capturable(dev):
    shape, sp, osp = SCAN
    rd = torch.from_numpy(scan_like((2, *shape, 2), 91, np.int16)).to(dev)
    call = lambda: P.prepare_scan(rd, sp, osp, (4, 20, 12), percentile=99.5, dtype=torch.bfloat16)
    e0, s0 = call()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        call()
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(gr):
        out, stats = call()
    hist = PKG.hip.graphs.assert_no_memset_nodes(gr)
    assert hist.get("kernel", 0) == 14 and not hist.get("memcpy", 0), hist           # 3 of the resampling + 11 of prepare_input
    gr.instantiate()
    for _ in range(2):
        out.zero_(); stats.zero_()
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(as_bits(out), as_bits(e0)) and torch.equal(stats, s0)


@pytest.mark.gpu
def test_public_resample_on_device_tensors(dev):
    shape, sp, osp = GEOMS[0]
    for ch in (None, 3):
        x = scan_like(shape + ((ch,) if ch else ()), 95, np.int16)
        ref = P.resample_host(x, sp, osp, default_value=2)
        e32 = float(np.abs(P.resample_host(x, sp, osp, default_value=2, dtype=np.float32) - ref).max())
        got = P.resample(torch.from_numpy(x).to(dev), sp, osp, default_value=2)
        assert got.dtype == torch.float32 and tuple(got.shape) == ref.shape
        assert (np.abs(got.cpu().numpy() - ref) <= 4 * e32).all()
        for lab in (x, (np.abs(x) % 3).astype(np.uint8), x.astype(np.float32)):      # a uint8 label goes through int16
            gl = P.resample(torch.from_numpy(lab).to(dev), sp, osp, is_label=True, default_value=2)
            assert gl.dtype == torch.from_numpy(lab).dtype
            assert np.array_equal(gl.cpu().numpy(), P.resample(lab, sp, osp, is_label=True, default_value=2))
    with pytest.raises(ValueError):
        P.resample(torch.zeros(3, 3, device=dev), (1, 1), (1, 1))
