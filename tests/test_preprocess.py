"""Scan preprocessing (csrc/preprocess.hip: m1_crop_pad, m1_order_stats, m1_whiten; ops.crop_pad / order_stats / whiten; the public
module preprocess.py with the reference's whitening, center_crop, resize_image_with_crop_or_pad and the fused prepare_input).

Yardsticks: the selection and the gather are exact (bit-equal to np.sort / to the numpy index map); the interpolated percentile is
within 1 fp32 ulp of np.percentile on the fp64 slice; the whitened elements are compared per element with the fp64 restatement
(preprocess.whitening_host(..., np.float64)) under

    |got - ref64| <= max(k * 2^-24 * max|ref64|, 4 * e32)

where e32 is the error of the SAME restatement in fp32 values on the same input (rank and weight of a percentile stay fp64, as in the
kernels; np.percentile on an fp32 array also rounds the quantile, which costs it more than the whole bound: the CPU test prints it) and k counts
the fp32 roundings behind one output in the kernel's operation order, each at most 2^-24 relative to a quantity max|out| bounds after
the division: the rounding of the mean, the subtraction, the rounding of std, the division -> K_PLAIN = 4; with a clip the threshold's
rounding to fp32 passes through a clipped element -> K_CLIP = 5.  mean / std are fp64 sums of exact fp32 values: 8 * 2^-53 relative
for the operations of one partial, times sqrt(n) headroom for the folds.  Measured values: see DESIGN.md section 7.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from util import C1_FILTERS, C1_STRIDES, PKG, build_m1, load_params_into, ops

P = PKG.preprocess
L = PKG.hip.lib
U = 2.0 ** -24
K_PLAIN, K_CLIP = 4, 5
QS = (0, 0.5, 1, 50, 99, 99.5, 100)
NS = (1, 2, 3, 255, 256, 257, 4099)
MODES = ("constant", "edge", "reflect", "symmetric")
WH_SHAPES = ((3, 9, 11), (5, 33, 36), (4, 32, 32))
PERCENTILES = (None, 99.5, 99, 30)


def k_of(percentile):
    return K_PLAIN if percentile is None else K_CLIP


def scan_like(shape, seed, dtype=np.float32):
    """N(300, 200^2), the intensities of a T2 sequence in scanner units (int16: rounded)."""
    x = np.random.default_rng(seed).normal(300.0, 200.0, shape)
    return np.rint(x).astype(np.int16) if dtype == np.int16 else x.astype(np.float32)


def wh_source(dst, seed, dtype=np.float32, B=2, Cn=3):
    """A raw batch around target ``dst``: the depth axis is cropped, the height axis padded, the width axis cropped by an odd amount."""
    return scan_like((B, dst[0] + 2, max(dst[1] - 3, 1), dst[2] + 5, Cn), seed, dtype)


def slices64(raw, dst, start, mode, cval, percentile, vt):
    """The restatement per (b, c) slice: (whitened (B,*dst,C), the clipped-but-not-whitened volumes (B,*dst,C)) in ``vt`` values."""
    B, Cn = raw.shape[0], raw.shape[-1]
    out = np.zeros((B, *dst, Cn), vt)
    for b in range(B):
        for c in range(Cn):
            vol = P.crop_pad_host(raw[b, ..., c], dst, start, mode, cval)
            out[b, ..., c] = P.whitening_host(vol, percentile, vt)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_percentile_rank_reconstructs_numpy_percentile():
    for n in NS:
        a = np.arange(n, dtype=np.float64)
        for q in QS:
            k, g = P.percentile_rank(q, n)
            assert 0 <= k < n and 0.0 <= g < 1.0
            lo, hi = a[k], a[min(k + 1, n - 1)]
            assert lo + (hi - lo) * g == np.percentile(a, q), (n, q, k, g)
    with pytest.raises(ValueError):
        P.percentile_rank(100.5, 4)


def test_periodic_maps_equal_np_pad_for_pads_wider_than_the_axis():
    for n in (1, 2, 3, 5):
        a = np.arange(n)
        for pad in range(14):
            for mode, f in (("reflect", P.reflect_index), ("symmetric", P.symmetric_index)):
                want = np.pad(a, (pad, pad), mode=mode)
                got = np.array([f(i, n) for i in range(-pad, n + pad)])
                assert np.array_equal(got, want), (mode, n, pad)


def _direct_resize(x, target, **kw):
    sl, pad = [], []
    for s, t in zip(x.shape, target):
        if s < t:
            sl.append(slice(None)); pad.append(((t - s) // 2, t - s - (t - s) // 2))
        else:
            f = int(np.floor((s - t) / 2.0))
            sl.append(slice(f, f + t)); pad.append((0, 0))
    pad += [(0, 0)] * (x.ndim - len(target))
    return np.pad(x[tuple(sl)], pad, **kw)


RESIZE_CASES = [((5, 4, 7), (2, 9, 7)), ((1, 3, 2), (4, 1, 9)), ((3, 3, 3), (16, 3, 1)), ((8, 9, 33), (7, 33, 8)), ((2, 1, 6), (5, 4, 3)),
                ((7, 8, 9), (1, 1, 1)), ((1, 1, 1), (3, 8, 2))]


def test_resize_with_crop_or_pad_equals_slicing_and_np_pad():
    rng = np.random.default_rng(3)
    for src, dst in RESIZE_CASES:
        for ch in (None, 2):
            x = rng.integers(-99, 99, src + ((ch,) if ch else ())).astype(np.int16)
            for mode in MODES:
                kw = {"mode": mode, **({"constant_values": -3} if mode == "constant" else {})}
                got = P.resize_image_with_crop_or_pad(x, dst, **kw)
                assert got.dtype == x.dtype and np.array_equal(got, _direct_resize(x, dst, **kw)), (src, dst, ch, mode)
    x = rng.standard_normal((4, 5, 6)).astype(np.float32)
    assert np.array_equal(P.resize_image_with_crop_or_pad(x, (6, 5, 2)), _direct_resize(x, (6, 5, 2)))           # the default: zeros


def test_center_crop_equals_slicing():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((7, 9, 8)).astype(np.float32)
    assert np.array_equal(P.center_crop(x, 3, 4, 5), x[2:5, 2:6, 2:7])                 # 7//2 - 3//2 = 2, 9//2 - 4//2 = 2, 8//2 - 5//2 = 2
    assert np.array_equal(P.center_crop(x, 7, 9, 8), x)
    assert np.array_equal(P.center_crop(x, 2, 3, 3, center_2d_coords=(7.9, 1)), x[2:4, 6:9, 0:3])      # int(7.9) - 1 = 6, 1 - 1 = 0
    xc = rng.standard_normal((4, 6, 6, 3)).astype(np.float32)
    assert np.array_equal(P.center_crop(xc, 1, 2, 6, multi_channel=True), xc[2:3, 2:4, 0:6, :])
    for bad in (dict(cropz=8), dict(cropx=10), dict(center_2d_coords=(0, 4)), dict(center_2d_coords=(4, 7))):
        kw = dict(cropz=3, cropx=4, cropy=5)
        kw.update(bad)
        with pytest.raises(ValueError):
            P.center_crop(x, **kw)
    with pytest.raises(ValueError):
        P.center_crop(xc, 1, 2, 2)                                                     # rank 4 without multi_channel


def test_whitening_equals_the_direct_numpy_computation():
    for seed, shape in enumerate(((4, 5, 6), (37,), (3, 2, 2, 2))):
        for dtype in (np.float32, np.int16, np.float64):
            x = scan_like(shape, seed, np.int16 if dtype == np.int16 else np.float32).astype(dtype)
            for p in PERCENTILES:
                im = x.astype(np.float32)
                if p is not None:
                    im = np.clip(im, np.percentile(im, 100 - p), np.percentile(im, p))
                mean, std = np.mean(im), np.std(im)
                want = (im - mean) / std if std > 0 else im * 0.0
                got = P.whitening(x, p)
                assert got.dtype == np.float32 and np.array_equal(got, want), (shape, dtype, p)
                im64 = x.astype(np.float32).astype(np.float64)
                if p is not None:
                    im64 = np.clip(im64, np.percentile(im64, 100 - p), np.percentile(im64, p))
                want64 = (im64 - im64.mean()) / im64.std() if im64.std() > 0 else im64 * 0.0
                assert np.array_equal(P.whitening_host(x, p, np.float64), want64)
    assert not P.whitening(np.full((3, 4), 7.0)).any()                                 # std == 0: zeros
    x = scan_like((50,), 9)                                                            # lo > hi: the operation order np.clip has, hi everywhere
    assert np.array_equal(np.minimum(np.maximum(x, 400.0), 200.0), np.clip(x, 400.0, 200.0)) and (np.clip(x, 400.0, 200.0) == 200.0).all()


def test_unbuilt_parts_say_so():
    x = np.zeros((3, 3, 3), np.float32)
    for kw in (dict(mode="wrap"), dict(mode="linear_ramp"), dict(mode="constant", constant_values=(1, 2)), dict(mode="reflect", reflect_type="odd"),
               dict(mode=lambda *a: None)):
        with pytest.raises(NotImplementedError, match="constant"):
            P.resize_image_with_crop_or_pad(x, (4, 4, 4), **kw)
    with pytest.raises(NotImplementedError, match="SimpleITK"):
        P.resample_img(None)
    with pytest.raises(ValueError):
        P.resize_image_with_crop_or_pad(x, (4, 4))
    with pytest.raises(ValueError):
        P.prepare_input(x, (4, 4, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        P.prepare_input(torch.zeros(1, 3, 3, 3, 1), (4, 4, 4))
    import model.preprocess as alias
    assert alias is P


def _geom(src=(3, 4, 5), dst=(2, 6, 5), start=(0, -1, 0), mode=0, cval=0.0):
    g = L.m1_crop_pad_t()
    g.src[:], g.dst[:], g.start[:], g.mode, g.cval = src, dst, start, mode, cval
    return g


def test_c_entry_points_reject_bad_arguments_without_a_gpu():
    lib = L.load()
    BAD, UNSUP = -1, -2
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    ranks, w = (C.c_int * 4)(0, 1, 2, 3), (C.c_double * 4)(0.0, 0.5, 0.25, 1.0)
    g = _geom()
    n = 2 * 6 * 5

    def cp(src=p, sdt=0, geom=g, B=1, Cn=1, out=p, odt=0):
        return lib.m1_crop_pad(src, sdt, C.byref(geom) if geom is not None else None, B, Cn, out, odt, None)

    def osx(src=p, sdt=0, geom=g, B=1, Cn=1, r=ranks, wt=w, nq=2, pairs=p, values=p, ws=p):
        return lib.m1_order_stats(src, sdt, C.byref(geom) if geom is not None else None, B, Cn, r, wt, nq, pairs, values, ws, None)

    def wh(src=p, sdt=0, geom=g, B=1, Cn=1, bounds=None, out=p, odt=0, stats=p, ws=p):
        return lib.m1_whiten(src, sdt, C.byref(geom) if geom is not None else None, B, Cn, bounds, out, odt, stats, ws, None)

    for f in (cp, osx, wh):
        assert f(src=None) == BAD and f(geom=None) == BAD and f(B=0) == BAD and f(Cn=0) == BAD and f(Cn=-2) == BAD
        assert f(geom=_geom(src=(0, 4, 5))) == BAD and f(geom=_geom(dst=(2, -6, 5))) == BAD
        assert f(src=p + 2) == BAD and f(src=p + 1, sdt=1) == BAD                      # off the element alignment
        assert f(sdt=2) == UNSUP and f(sdt=-1) == UNSUP and f(geom=_geom(mode=4)) == UNSUP and f(geom=_geom(mode=-1)) == UNSUP
        assert f(Cn=9) == UNSUP
        assert f(geom=_geom(dst=(2048, 1024, 1024))) == UNSUP                          # n = 2^31
    assert cp(out=None) == BAD and cp(out=p + 2) == BAD and cp(out=p + 1, odt=1) == BAD and cp(odt=2) == UNSUP
    assert wh(out=None) == BAD and wh(stats=None) == BAD and wh(ws=None) == BAD and wh(stats=p + 4) == BAD and wh(ws=p + 4) == BAD
    assert wh(bounds=p + 2) == BAD and wh(odt=-1) == UNSUP
    assert osx(r=None) == BAD and osx(wt=None) == BAD and osx(pairs=None) == BAD and osx(values=None) == BAD and osx(ws=None) == BAD
    assert osx(nq=0) == BAD and osx(nq=5) == UNSUP and osx(ws=p + 4) == BAD and osx(values=p + 2) == BAD
    assert osx(r=(C.c_int * 2)(0, n)) == BAD and osx(r=(C.c_int * 2)(-1, 0)) == BAD
    assert osx(wt=(C.c_double * 2)(0.0, 1.5)) == BAD
    # the workspace query is pure host: state + per-block histograms of the 2 nq ranks, or the whitening partials
    q = lambda geom, B, Cn, nq: int(lib.m1_preprocess_ws_bytes(C.byref(geom), B, Cn, nq))
    big = _geom(dst=(20, 160, 160))
    assert q(big, 2, 3, 0) == 6 * 64 * 3 * 8 and q(big, 2, 3, 2) == 6 * 160 + 6 * 64 * 4 * 256 * 4
    assert q(g, 1, 1, 0) == 24 and q(g, 1, 1, 5) == 0 and q(g, 0, 1, 0) == 0 and q(_geom(mode=7), 1, 1, 0) == 0


@pytest.mark.parametrize("shape", WH_SHAPES)
def test_fp32_numpy_stays_inside_the_rounding_term_of_the_bound(shape):
    """The first term of the elements' bound, k * 2^-24 * max|out|, is meant to cover an fp32 evaluation in the kernel's operation
    order: the restatement run in fp32 values must fit it on the inputs the GPU test uses, or the term would say nothing about them.
    Printed next to it, not asserted: the reference's own numpy calls on the fp32 array (preprocess.whitening), whose np.percentile
    rounds the quantile to fp32 and lands at 1.0 - 48 x 2^-24 max|out| here, above k = 5 wherever a wide gap between neighbouring
    order statistics (small n, a run of equal pad values) meets a clip."""
    for dtype in (np.float32, np.int16):
        raw = wh_source(shape, 11, dtype)
        start = P.crop_or_pad_starts(raw.shape[1:4], shape)
        for mode, cval in (("constant", 41), ("symmetric", 0), ("constant", 0)):
            for p in PERCENTILES[:3]:
                ref = slices64(raw, shape, start, mode, cval, p, np.float64)
                unit = U * np.abs(ref).max()
                e32 = np.abs(slices64(raw, shape, start, mode, cval, p, np.float32).astype(np.float64) - ref).max()
                enp = max(np.abs(P.whitening(P.crop_pad_host(raw[b, ..., c], shape, start, mode, cval), p) - ref[b, ..., c]).max()
                          for b in range(2) for c in range(3))
                print(shape, dtype.__name__, mode, cval, p, f"e32 = {e32 / unit:.2f}, numpy's own fp32 calls {enp / unit:.2f} x 2^-24 max|out|")
                assert e32 <= k_of(p) * unit, (shape, dtype, mode, p)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: selection
# ---------------------------------------------------------------------------------------------------------------------------------
# n -> (source extent, output extent, start): the pads (n >= 3) put pad values into the output domain
SEL_GEOM = {1: ((1, 1, 1), (1, 1, 1), (0, 0, 0)), 2: ((1, 2, 2), (1, 1, 2), (0, 1, 0)), 3: ((1, 2, 1), (1, 3, 1), (0, -1, 0)),
            255: ((2, 5, 15), (3, 5, 17), (0, 0, -1)), 256: ((5, 8, 7), (4, 8, 8), (1, 0, -1)), 257: ((1, 1, 250), (1, 1, 257), (0, 0, -3)),
            4099: ((1, 2, 4000), (1, 1, 4099), (0, 1, -50))}
SEL_DATA = ("normal", "equal", "two", "zeros", "extremes", "int16")
FMAX = float(np.finfo(np.float32).max)


def sel_data(kind, shape, seed):
    rng = np.random.default_rng(seed)
    if kind == "normal":
        return (rng.standard_normal(shape) * 200 + 300).astype(np.float32)
    if kind == "equal":
        return np.full(shape, 7.25, np.float32)
    if kind == "two":                                       # about half of each: the run of ties straddles the middle rank
        return np.where(rng.random(shape) < 0.5, np.float32(-2.5), np.float32(1.0e3)).astype(np.float32)
    if kind == "zeros":
        x = (rng.standard_normal(shape) * 3).astype(np.float32)
        r = rng.random(shape)
        x[r < 0.3] = 0.0
        x[r < 0.15] = -0.0
        return x
    if kind == "extremes":
        x = (rng.standard_normal(shape)).astype(np.float32)
        r = rng.random(shape)
        den = (rng.integers(-5000, 5000, shape) * np.float64(1.4e-45)).astype(np.float32)      # denormals of both signs
        x = np.where(r < 0.4, den, x)
        x = np.where(r > 0.9, np.float32(FMAX), x)
        return np.where(r > 0.95, np.float32(-FMAX), x).astype(np.float32)
    return rng.integers(-32768, 32767, shape, endpoint=True).astype(np.int16)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", SEL_DATA)
def test_order_stats_are_the_sorted_values_bit_for_bit(dev, kind):
    for n, (src, dst, start) in SEL_GEOM.items():
        for (B, Cn), mode in (((1, 1), "constant"), ((2, 3), "reflect")):
            raw = sel_data(kind, (B, *src, Cn), 100 * n + B)
            cval = -7.0 if kind == "int16" else 1.5
            sl = np.stack([[np.sort(P.crop_pad_host(raw[b, ..., c], dst, start, mode, cval).astype(np.float32), axis=None)
                            for c in range(Cn)] for b in range(B)])                    # (B, C, n) sorted
            assert sl.shape == (B, Cn, n)
            rd = torch.from_numpy(raw).to(dev)
            pct = [P.percentile_rank(q, n) for q in (0.5, 99.5)]
            for ranks, weights, qs in (((0, n - 1, n // 2), (0.0, 1.0, 0.5), None), (tuple(k for k, _ in pct), tuple(g for _, g in pct), (0.5, 99.5))):
                pairs, values = ops.order_stats(rd, dst, start, ranks, weights, mode, cval)
                pairs, values = pairs.cpu().numpy(), values.cpu().numpy()
                assert pairs.shape == (B, Cn, len(ranks), 2) and values.shape == (B, Cn, len(ranks))
                for j, k in enumerate(ranks):
                    want = sl[:, :, [k, min(k + 1, n - 1)]]
                    if kind == "zeros":                     # np.sort leaves -0.0 and +0.0 in any order: they compare equal
                        assert np.array_equal(pairs[:, :, j], want), (n, B, j)
                    else:
                        assert np.array_equal(pairs[:, :, j].view(np.uint32), want.view(np.uint32)), (n, B, j, pairs[:, :, j], want)
                    if qs is not None:                      # the interpolation: 1 fp32 ulp around numpy's fp64 percentile
                        ref = np.percentile(sl.astype(np.float64), qs[j], axis=-1)
                        with np.errstate(over="ignore"):                                # (spacing(FLT_MAX) overflows in fp32: it is 2^104)
                            ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
                        ulp = np.where(np.isinf(ulp), 2.0 ** 104, ulp)
                        assert (np.abs(values[:, :, j].astype(np.float64) - ref) <= ulp).all(), (n, B, qs[j], values[:, :, j], ref)
                    else:
                        a, b = want[..., 0].astype(np.float64), want[..., 1].astype(np.float64)
                        assert np.array_equal(values[:, :, j], (a + (b - a) * weights[j]).astype(np.float32)), (n, j)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: geometry
# ---------------------------------------------------------------------------------------------------------------------------------
# (source, output, start): edges from {1, 2, 3, 7, 8, 9, 33}, crop and pad mixed per axis, pads wider than the axis, the first and
# the last source element read
GEOMS = [((1, 1, 1), (1, 1, 1), (0, 0, 0)), ((2, 3, 7), (7, 3, 2), (-2, 0, 3)), ((3, 8, 9), (2, 9, 8), (1, -1, 0)),
         ((7, 2, 33), (3, 7, 33), (2, -2, 0)), ((9, 33, 1), (1, 8, 9), (4, 12, -4)), ((1, 7, 8), (8, 1, 33), (-3, 6, -12)),
         ((33, 1, 3), (9, 2, 7), (24, -1, -2)), ((8, 9, 2), (8, 9, 2), (0, 0, 0)), ((3, 3, 8), (2, 33, 8), (0, -15, 0)),
         ((2, 2, 2), (3, 3, 9), (-1, 0, -7))]


def as_bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("Cn", (1, 3, 4))
def test_crop_pad_equals_the_index_map_bit_for_bit(dev, Cn):
    for src, dst, start in GEOMS:
        for in_dtype in (np.float32, np.int16):
            raw = scan_like((2, *src, Cn), sum(src) + Cn, in_dtype)
            rd = torch.from_numpy(raw).to(dev)
            for mode in MODES:
                cval = 3.0 if mode == "constant" else 0.0
                want = np.stack([P.crop_pad_host(raw[b], dst, start, mode, cval) for b in range(2)]).astype(np.float32)
                wt = torch.from_numpy(want)
                got = ops.crop_pad(rd, dst, start, mode, cval)
                assert got.dtype == torch.float32 and torch.equal(as_bits(got.cpu()), as_bits(wt)), (src, dst, start, mode, in_dtype)
                gb = ops.crop_pad(rd, dst, start, mode, cval, torch.bfloat16)
                assert torch.equal(as_bits(gb), as_bits(ops.cast(got, torch.bfloat16))) and torch.equal(as_bits(gb.cpu()), as_bits(wt.to(torch.bfloat16)))
                # a view whose first element is off the 16-byte grid: the element paths, the same values
                flat = torch.empty(rd.numel() + 1, dtype=rd.dtype, device=dev)
                flat[1:].copy_(rd.reshape(-1))
                assert torch.equal(ops.crop_pad(flat[1:].view(rd.shape), dst, start, mode, cval), got)


@pytest.mark.gpu
def test_public_crop_functions_on_device_tensors(dev):
    for src, dst in RESIZE_CASES:
        for ch in (None, 3):
            for dtype in (np.float32, np.int16):
                x = scan_like(src + ((ch,) if ch else ()), 5, dtype)
                for mode in MODES:
                    kw = {"mode": mode, **({"constant_values": -3} if mode == "constant" else {})}
                    got = P.resize_image_with_crop_or_pad(torch.from_numpy(x).to(dev), dst, **kw)
                    want = P.resize_image_with_crop_or_pad(x, dst, **kw).astype(np.float32)
                    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), want), (src, dst, ch, dtype, mode)
    x = scan_like((7, 9, 8, 3), 6, np.int16)
    xd = torch.from_numpy(x).to(dev)
    for kw in (dict(cropz=3, cropx=4, cropy=5), dict(cropz=7, cropx=9, cropy=8), dict(cropz=2, cropx=3, cropy=3, center_2d_coords=(7.9, 1))):
        assert np.array_equal(P.center_crop(xd, multi_channel=True, **kw).cpu().numpy(), P.center_crop(x, multi_channel=True, **kw).astype(np.float32))
        assert np.array_equal(P.center_crop(xd[..., 1], **kw).cpu().numpy(), P.center_crop(x[..., 1], **kw).astype(np.float32))
    with pytest.raises(ValueError):
        P.center_crop(xd, 8, 2, 2, multi_channel=True)
    with pytest.raises(NotImplementedError):
        P.resize_image_with_crop_or_pad(xd, (4, 4, 4), mode="wrap")


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: whitening and prepare_input
# ---------------------------------------------------------------------------------------------------------------------------------
def _ref_stats(raw, dst, start, mode, cval, percentile):
    """fp64 {mean, std} (B, C, 2) of every slice clipped at the fp32 thresholds a + (b - a) * gamma (fp64, rounded once), computed
    from the sorted slice: the y of m1_whiten."""
    B, Cn = raw.shape[0], raw.shape[-1]
    out = np.zeros((B, Cn, 2))
    for b in range(B):
        for c in range(Cn):
            v = P.crop_pad_host(raw[b, ..., c], dst, start, mode, cval).astype(np.float32).astype(np.float64)
            if percentile is not None:
                s = np.sort(v, axis=None)
                th = []
                for q in (100 - percentile, percentile):
                    k, g = P.percentile_rank(q, s.size)
                    th.append(np.float64(np.float32(s[k] + (s[min(k + 1, s.size - 1)] - s[k]) * g)))
                v = np.minimum(np.maximum(v, th[0]), th[1])
            out[b, c] = v.mean(), v.std()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("in_dtype", (np.float32, np.int16))
@pytest.mark.parametrize("shape", WH_SHAPES)
def test_prepare_input_against_the_fp64_restatement(dev, shape, in_dtype):
    raw = wh_source(shape, 11, in_dtype)
    raw[1, ..., 2] = 41                                      # a constant slice: zeros
    rd = torch.from_numpy(raw).to(dev)
    n = shape[0] * shape[1] * shape[2]
    for mode, cval in (("constant", 41), ("symmetric", 0)):           # (pads of 41 keep the constant slice constant)
        start = P.crop_or_pad_starts(raw.shape[1:4], shape)
        for p in PERCENTILES:
            out, stats = P.prepare_input(rd, shape, percentile=p, pad_mode=mode, constant_values=cval)
            assert out.dtype == torch.float32 and tuple(out.shape) == (2, *shape, 3) and tuple(stats.shape) == (2, 3, 2) and stats.dtype == torch.float64
            got = out.cpu().numpy().astype(np.float64)
            assert np.isfinite(got).all() and not got[1, ..., 2].any()
            if p == 30:
                # lo > hi: y = hi everywhere, so the output is all zeros -- asserted as such.  The restatement is no yardstick here: the mean
                # of n copies of an fp64 threshold is not that threshold to the last bit, and it then divides rounding noise by rounding noise
                assert not got.any()
            else:
                ref = slices64(raw, shape, start, mode, cval, p, np.float64)
                e32 = float(np.abs(slices64(raw, shape, start, mode, cval, p, np.float32).astype(np.float64) - ref).max())
                unit = U * float(np.abs(ref).max())
                err, bound = float(np.abs(got - ref).max()), max(k_of(p) * unit, 4 * e32)
                print(f"{shape} {in_dtype.__name__} {mode} p={p}: max |out - ref64| = {err / unit:.2f} x 2^-24 max|out|, e32 = {e32 / unit:.2f}")
                assert err <= bound, (shape, mode, p, err, bound)
            want = _ref_stats(raw, shape, start, mode, cval, p)
            st = stats.cpu().numpy()
            tol = 8 * 2.0 ** -53 * math.sqrt(n)
            rel = np.abs(st - want) / np.maximum(np.abs(want), 1e-300)
            print("   mean / std: largest relative error", float(rel[want != 0].max()) if (want != 0).any() else 0.0, "tolerance", tol)
            assert (np.abs(st - want) <= tol * np.abs(want)).all(), (shape, mode, p, st, want)
            ob, sb = P.prepare_input(rd, shape, percentile=p, pad_mode=mode, constant_values=cval, dtype=torch.bfloat16)
            assert ob.dtype == torch.bfloat16 and torch.equal(as_bits(ob), as_bits(ops.cast(out, torch.bfloat16))) and torch.equal(sb, stats)
    # per-slice independence: slice (b, c) of the batched call equals the single-slice call bit for bit
    for p in (None, 99.5):
        out, stats = P.prepare_input(rd, shape, percentile=p)
        for b, c in ((0, 0), (1, 1), (0, 2)):
            o1, s1 = P.prepare_input(rd[b:b + 1, ..., c:c + 1].contiguous(), shape, percentile=p)
            assert torch.equal(as_bits(o1[0, ..., 0]), as_bits(out[b, ..., c])) and torch.equal(s1[0, 0], stats[b, c])


@pytest.mark.gpu
def test_whitening_of_a_whole_device_array_and_the_explicit_centre(dev):
    x = scan_like((5, 33, 36), 21)
    xd = torch.from_numpy(x).to(dev)
    assert not P.whitening(xd, 30).any()                                               # lo > hi: zeros (see the test above)
    for p in (None, 99.5):
        ref = P.whitening_host(x, p, np.float64)
        e32 = float(np.abs(P.whitening_host(x, p, np.float32).astype(np.float64) - ref).max())
        got = P.whitening(xd, p)
        assert got.dtype == torch.float32 and got.shape == xd.shape
        assert float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max()) <= max(k_of(p) * U * float(np.abs(ref).max()), 4 * e32)
    xi = scan_like((37,), 22, np.int16)
    ref = P.whitening_host(xi, 99, np.float64)
    e32 = float(np.abs(P.whitening_host(xi, 99, np.float32).astype(np.float64) - ref).max())
    assert float(np.abs(P.whitening(torch.from_numpy(xi).to(dev), 99).cpu().numpy() - ref).max()) <= max(K_CLIP * U * float(np.abs(ref).max()), 4 * e32)
    assert not P.whitening(torch.full((3, 4), 7.0, device=dev)).any()
    # prepare_input around an explicit centre: the (h, w) window of center_crop, the depth axis padded
    raw = scan_like((1, 3, 9, 8, 2), 23)
    out, _ = P.prepare_input(torch.from_numpy(raw).to(dev), (4, 3, 3), center_2d_coords=(7.9, 1), pad_mode="edge")
    ref = slices64(raw, (4, 3, 3), (0, 6, 0), "edge", 0, None, np.float64)
    e32 = float(np.abs(slices64(raw, (4, 3, 3), (0, 6, 0), "edge", 0, None, np.float32) - ref).max())
    assert float(np.abs(out.cpu().numpy() - ref).max()) <= max(K_PLAIN * U * float(np.abs(ref).max()), 4 * e32)
    with pytest.raises(ValueError):
        P.prepare_input(torch.from_numpy(raw).to(dev), (4, 3, 3), center_2d_coords=(8, 1))


@pytest.mark.gpu
def test_prepare_input_is_deterministic_and_capturable(dev):
    shape = (5, 33, 36)
    rd = torch.from_numpy(wh_source(shape, 31, np.int16)).to(dev)
    call = lambda: P.prepare_input(rd, shape, percentile=99.5, pad_mode="reflect", dtype=torch.bfloat16)
    e0, s0 = call()
    e1, s1 = call()
    assert torch.equal(as_bits(e0), as_bits(e1)) and torch.equal(s0, s1)
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
    assert hist.get("kernel", 0) == 11 and not hist.get("memcpy", 0), hist          # 8 launches of the selection + 3 of the whitening
    gr.instantiate()
    for _ in range(2):
        out.zero_(); stats.zero_()
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(as_bits(out), as_bits(e0)) and torch.equal(stats, s0)


@pytest.mark.gpu
def test_prepared_input_feeds_predict(dev):
    """Shape, dtype and layout join: predict of the device-prepared input equals predict of the host-preprocessed, uploaded one to the
    forward tolerance of the model tests (tests/test_hip_model.py: 1e-3 on the output), the inputs differing by the whitening bound."""
    from oracle import m1_oracle as O
    dims = (4, 32, 32)
    cfg = O.M1Config(input_spatial_dims=dims, filters=C1_FILTERS, strides=C1_STRIDES, dense_skip=False, probabilistic=False,
                     prob_latent_dims=(3, 2, 1, 0), dropout_rate=0.0)
    m = build_m1(cfg, dev)
    load_params_into(m, O.fixture_params(cfg, seed=71))
    m.eval()
    dm = m.get_detect_model()
    raw = wh_source(dims, 72, np.int16)
    start = P.crop_or_pad_starts(raw.shape[1:4], dims)
    host = slices64(raw, dims, start, "constant", 0, 99.5, np.float32)
    x, _ = P.prepare_input(torch.from_numpy(raw).to(dev), dims, percentile=99.5)
    got, want = dm.predict(x), dm.predict(torch.from_numpy(host).to(dev))
    assert got.shape == want.shape and got.dtype == want.dtype
    assert float((got.double() - want.double()).abs().max()) < 1e-3
