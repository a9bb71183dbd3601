"""Train-time augmentations on the GPU (augmentations.py, csrc/augment.hip) against a numpy restatement of the reference's
``tf2.5/scripts/model/augmentations.py`` (cited as ``A:``).

TensorFlow is not installable here, so the yardstick is a restatement of the documented semantics of the TF ops the reference
calls, stage by stage, materialising every stage (``np.pad`` for the SYMMETRIC pads, whole resized / rotated slices).  Sampling
coordinates are computed in ``np.float32`` in TF's operation order; VALUES are interpolated in ``vt`` = float64 (the yardstick) or
float32 (a second run, whose largest element error against the float64 run on the same inputs is ``e32``).

Tolerance of the interpolating / intensity stages: ``max(floor, 4 * e32)``; the factor 4 covers a different but equally valid fp32
operation order and ``powf`` rounding.  ``floor = k * 2**-24 * max|x|`` with k the fp32 roundings on the longest path through the
kernels for the stages that are enabled (K_ROUNDINGS, summed per case by ``_k_roundings``), counted from csrc/augment.hip:
  zoom      aug_zf:   top = a + (b - a) * t (3), out = top + (bot - top) * t (3)                                   6
  rotate    aug_zfr:  lo = w0 * a + w1 * b (2), out = w0 * lo + w1 * hi (2)                                         4
  gamma     aug_gam:  7 fp32 constants (lo, rnge, den, mn, sd, m2, den2); aug_pow: sub, div, powf (2), mul, add (6);
            aug_gamma: sub, div, mul, add (4)                                                                      17
  poor scan two nested lerps                                                                                        6
  noise     std * z, add                                                                                            2
                                                                                                             total 35
Index-only stages (flip, translate, channel shift, un-fired samples, label channels of the image in the intensity stages) are
compared for bit equality.

The measured e32 and product errors are printed per case and summarised in DESIGN.md section 7 ("Train-time augmentations").
"""
import importlib
import inspect
import math

import numpy as np
import pytest
import torch

from util import PKG

A = PKG.augmentations
L = PKG.hip.lib
ops = PKG.hip.ops
T = importlib.import_module("prostatemr_3d-cad-cspca_amd.train_model")

f32 = np.float32
K_ROUNDINGS = {"zoom": 6, "rotate": 4, "gamma": 17, "poor": 6, "noise": 2}     # the table of the module docstring
DEFAULT = [1.00, 0.25, 0.15, 10.0, True, 1.20, 0.10, 0.025, True, [0.50, 1.50]]


# ---- the restatement --------------------------------------------------------------------------------------------------------
def r_pad_crop(x, top, bottom, right, left):
    """translate_4D_tensor (A:167-181): pad_to_bounding_box SYMMETRIC (A:331-368: top / left offsets, the rest after), then
    crop_to_bounding_box at (pad_bottom, pad_right).  x (D,H,W,C)."""
    H, W = x.shape[1:3]
    p = np.pad(x, ((0, 0), (top, bottom), (left, right), (0, 0)), mode="symmetric")
    return p[:, bottom:bottom + H, right:right + W]


def r_resize_taps(n_in, n_out):
    """tf.image.resize bilinear, TF2 (half_pixel_centers, no antialias): in = (i + 0.5) * scale - 0.5 in fp32,
    lower = max(floor(in), 0), upper = min(ceil(in), n_in - 1), lerp = in - floor(in)."""
    scale = f32(f32(n_in) / f32(n_out))
    i = np.arange(n_out, dtype=f32)
    src = (i + f32(0.5)) * scale - f32(0.5)
    assert src.dtype == f32
    fl = np.floor(src)
    lo = np.maximum(fl.astype(np.int64), 0)
    hi = np.minimum(np.ceil(src).astype(np.int64), n_in - 1)
    return lo, hi, (src - fl).astype(f32), src


def r_resize_bilinear(x, oh, ow, vt):
    ylo, yhi, yt, _ = r_resize_taps(x.shape[1], oh)
    xlo, xhi, xt, _ = r_resize_taps(x.shape[2], ow)
    x = x.astype(vt)
    xt = xt.astype(vt)[None, None, :, None]
    yt = yt.astype(vt)[None, :, None, None]
    top = x[:, ylo][:, :, xlo] + (x[:, ylo][:, :, xhi] - x[:, ylo][:, :, xlo]) * xt
    bot = x[:, yhi][:, :, xlo] + (x[:, yhi][:, :, xhi] - x[:, yhi][:, :, xlo]) * xt
    return top + (bot - top) * yt


def r_nearest_index(n_in, n_out):
    """tf.image.resize nearest, TF2: min(floor((i + 0.5) * scale), n_in - 1), fp32."""
    scale = f32(f32(n_in) / f32(n_out))
    i = np.arange(n_out, dtype=f32)
    return np.minimum(np.floor((i + f32(0.5)) * scale).astype(np.int64), n_in - 1)


def r_zoom(x, scale, vt):
    """zoom_4D_tensor (A:139-152)."""
    H, W = x.shape[1:3]
    z = r_resize_bilinear(x, scale, scale, vt)
    return z[:, scale - H:scale - H + H, scale - W:scale - W + W]


def r_flip(x):
    """axial_4D_hflip (A:156-163): tf.image.flip_left_right."""
    return x[:, :, ::-1]


def r_rotate(x, rot, vt):
    """rotate_4D_tensor (A:219-236) with the six projective coefficients tfa.image.rotate derives from the angle:
    bilinear, output -> input map, constant fill 0, then central_crop."""
    H, W = x.shape[1:3]
    pad = A.rotation_pad(H, W)
    p = np.pad(x.astype(vt), ((0, 0), (pad, pad), (pad, pad), (0, 0)), mode="symmetric")
    Hp, Wp = p.shape[1:3]
    t = [f32(v) for v in rot]
    X, Y = np.meshgrid(np.arange(Wp, dtype=f32), np.arange(Hp, dtype=f32))
    ix = (t[0] * X + t[1] * Y) + t[2]
    iy = (t[3] * X + t[4] * Y) + t[5]
    assert ix.dtype == f32
    xf, yf = np.floor(ix), np.floor(iy)
    xc, yc = xf + f32(1), yf + f32(1)

    def read(yy, xx):
        ok = (yy >= 0) & (yy < Hp) & (xx >= 0) & (xx < Wp)
        yi, xi = np.clip(yy, 0, Hp - 1).astype(np.int64), np.clip(xx, 0, Wp - 1).astype(np.int64)
        return np.where(ok[None, :, :, None], p[:, yi, xi], vt(0))
    wx0, wx1 = (xc - ix).astype(vt)[None, :, :, None], (ix - xf).astype(vt)[None, :, :, None]
    wy0, wy1 = (yc - iy).astype(vt)[None, :, :, None], (iy - yf).astype(vt)[None, :, :, None]
    lo = wx0 * read(yf, xf) + wx1 * read(yf, xc)
    hi = wx0 * read(yc, xf) + wx1 * read(yc, xc)
    r = wy0 * lo + wy1 * hi
    frac = H / Hp                                                 # A:233
    sh, sw = A.central_crop_start(Hp, frac), A.central_crop_start(Wp, frac)
    out = r[:, sh:Hp - sh, sw:Wp - sw]
    assert out.shape[1:3] == (H, W)
    return out


def r_channel_shift(x, cs, ch):
    """channel_shift_4D_tensor (A:185-215)."""
    out = x.copy()
    out[..., ch:ch + 1] = r_pad_crop(x[..., ch:ch + 1], *cs)
    return out


def r_gamma_channel(x, gamma, vt):
    """gamma_shift_3D_tensor (A:298-310), fired."""
    x = x.astype(vt)
    g, eps = vt(gamma), vt(1e-8)
    mn, sd = x.mean(dtype=vt), x.std(dtype=vt)
    lo, hi = x.min(), x.max()
    x_ = np.power((x - lo) / (hi - lo + eps), g) * (hi - lo) + lo
    x_ = x_ - x_.mean(dtype=vt)
    x_ = x_ / (x_.std(dtype=vt) + eps) * sd
    return x_ + mn


def r_poor_channel(x, vt):
    """sim_poor_scan_3D_tensor (A:264-271), fired."""
    H = x.shape[1]
    h2 = int(H * 0.75)
    d = r_resize_bilinear(x, h2, h2, vt)
    idx = r_nearest_index(h2, H)
    return d[:, idx][:, :, idx]


def r_chain(img, lab, rec, stages, nimg, vt, z=None):
    """augment_tensors (A:36-132) for ONE sample with every draw given by the record ``rec``; ``stages``: the enabled stages."""
    fired = int(rec["fired"])
    if not fired & A.MASTER:
        return img, lab
    fired &= stages

    def geo(x, image):
        if fired & A.ZOOM: x = r_zoom(x, int(rec["scale"]), vt)
        if fired & A.FLIP: x = r_flip(x)
        if fired & A.ROTATE: x = r_rotate(x, rec["rot"], vt)
        if fired & A.TRANSLATE: x = r_pad_crop(x, *[int(v) for v in rec["tr"]])
        if image and fired & A.CSHIFT: x = r_channel_shift(x, [int(v) for v in rec["cs"]], int(rec["cs_channel"]))
        return x
    x = np.array(geo(img, True))
    if fired & (A.ZOOM | A.ROTATE):
        x = x.astype(vt)                                          # (each stage hands an fp32 tensor on in TF; the vt run keeps vt)
    if fired & A.GAMMA:
        x = x.astype(vt) if x.dtype != vt else x.copy()
        for c in range(nimg):
            if (int(rec["gamma_ch"]) >> c) & 1:
                x[..., c] = r_gamma_channel(x[..., c], rec["gamma"], vt)
    if fired & A.POOR:
        x = x.astype(vt) if x.dtype != vt else x.copy()
        for c in range(nimg):
            if (int(rec["poor_ch"]) >> c) & 1:
                x[..., c:c + 1] = r_poor_channel(x[..., c:c + 1], vt)
    if fired & A.NOISE:
        x = x.astype(vt) if x.dtype != vt else x.copy()
        x[..., :nimg] = x[..., :nimg] + (f32(rec["noise_std"]) * z[..., :nimg].astype(f32)).astype(vt)
    return x, np.array(geo(lab, False))


# ---- CPU 1: the restatement pins itself ------------------------------------------------------------------------------------------
def test_restatement_symmetric_pad_and_crop_known_answer():
    x = np.arange(16, dtype=f32).reshape(1, 4, 4, 1)
    out = r_pad_crop(x, 1, 0, 0, 2)[0, :, :, 0]                   # down by one row, right by two columns, mirrored at the edges
    want = np.array([[1, 0, 0, 1], [1, 0, 0, 1], [5, 4, 4, 5], [9, 8, 8, 9]], dtype=f32)
    assert np.array_equal(out, want)
    out = r_pad_crop(x, 0, 2, 1, 0)[0, :, :, 0]                   # up by two rows, left by one column
    want = np.array([[9, 10, 11, 11], [13, 14, 15, 15], [13, 14, 15, 15], [9, 10, 11, 11]], dtype=f32)
    assert np.array_equal(out, want)
    assert np.array_equal(r_pad_crop(x, 2, 2, 3, 3), x)           # equal pads cancel


def test_restatement_rotation_known_answers():
    g = np.random.default_rng(0)
    x = g.standard_normal((2, 8, 8, 2)).astype(f32)
    assert np.array_equal(r_rotate(x, A.rotation_coefficients(0.0, 8, 8), np.float64), x.astype(np.float64))
    r90 = r_rotate(x, A.rotation_coefficients(90.0, 8, 8), np.float64)
    want = np.rot90(x, k=1, axes=(1, 2)).astype(np.float64)       # tfa: positive angle = counter-clockwise
    assert np.abs(r90 - want).max() < 64 * 2.0 ** -24 * np.abs(x).max()      # cos(f32(pi/2)) = -4.4e-8, offsets rounded in fp32
    co = A.rotation_coefficients(10.0, 160, 160)
    assert co[0] == f32(np.cos(f32(f32(f32(10.0) * f32(math.pi)) / f32(180)))) and co[1] == -co[3] and co[0] == co[4]


def test_restatement_zoom_known_answers():
    g = np.random.default_rng(1)
    x = g.standard_normal((1, 6, 6, 1)).astype(f32)
    assert np.array_equal(r_zoom(x, 6, np.float64), x.astype(np.float64))           # scale == H: identity
    z = r_zoom(x, 8, np.float64)                                                    # scale == H + 2: rows / columns 2..7 of the 8x8 resize
    full = r_resize_bilinear(x, 8, 8, np.float64)
    assert np.array_equal(z, full[:, 2:8, 2:8])
    # the last output row sits at source coordinate (7.5 * 0.75 - 0.5) = 5.125 -> clamped to row 5; the one before at 4.375
    assert np.allclose(z[0, -1, -1, 0], x[0, 5, 5, 0])
    lo, hi, t, src = r_resize_taps(6, 8)
    assert list(lo) == [0, 0, 1, 2, 2, 3, 4, 5] and list(hi) == [0, 1, 2, 3, 3, 4, 5, 5]
    assert src[6] == f32(4.375) and t[6] == f32(0.375)


def test_restatement_nearest_up_indices():
    for H in (160, 32):
        h2 = int(H * 0.75)
        idx = r_nearest_index(h2, H)
        assert h2 == {160: 120, 32: 24}[H] and idx[0] == 0 and idx[-1] == h2 - 1 and len(idx) == H
        # floor((i + 0.5) * 0.75): every group of four outputs takes source cells 3k, 3k+1, 3k+1, 3k+2
        assert list(idx[:8]) == [0, 1, 1, 2, 3, 4, 4, 5]
        assert np.array_equal(idx, np.floor((np.arange(H) + 0.5) * 0.75).astype(np.int64))


def test_restatement_gamma_one_is_identity_and_central_crop_start():
    g = np.random.default_rng(2)
    x = g.standard_normal((3, 8, 8)).astype(f32)
    assert np.abs(r_gamma_channel(x, 1.0, np.float64) - x).max() < 1e-6            # the +1e-8 terms of A:303,307
    for H, pad in ((160, 34), (32, 7)):
        assert A.rotation_pad(H, H) == pad
        assert A.central_crop_start(H + 2 * pad, H / (H + 2 * pad)) == pad
        A.check_geometry(A.ROTATE, H, H)
    with pytest.raises(ValueError, match="233-234"):
        A.check_geometry(A.ROTATE, 32, 48)


# ---- CPU 2: ABI ---------------------------------------------------------------------------------------------------------------------
def test_abi_rejects_bad_arguments_without_a_gpu():
    lib = L.load()
    BAD, UNS = -1, -2
    p = 4096                                                      # any non-null address: nothing is launched or dereferenced
    hyper = (1.0, 0.25, 0.15, 10.0, 1, 1.2, 0.1, 0.025, 1, 0.5, 1.5)
    assert lib.m1_aug_draw(None, 2, p, 0, *hyper, 32, 32, 3, 1, None) == BAD
    assert lib.m1_aug_draw(p, 2, None, 0, *hyper, 32, 32, 3, 1, None) == BAD
    assert lib.m1_aug_draw(p, 0, p, 0, *hyper, 32, 32, 3, 1, None) == BAD
    assert lib.m1_aug_draw(p, 2, p, 0, *hyper, 32, 0, 3, 1, None) == BAD
    assert lib.m1_aug_draw(p, 2, p, 0, *hyper, 32, 48, 3, 1, None) == UNS           # zoom / rotation / poor scan on a non-square slice
    assert lib.m1_aug_draw(p, 2, p, 0, 1.0, 0.25, 0.15, 10.0, 1, 1.0, 0.1, 0.025, 1, 0.5, 1.5, 32, 32, 3, 1, None) == BAD   # [H, H) empty
    assert lib.m1_aug_ws_bytes(0, 4, 32, 32, 3) == 0 and lib.m1_aug_ws_bytes(2, 4, 32, 32, 3) >= 2 * 3 * 6 * 8
    geom = lambda x=p, y=p, t=p, gx=2 * p, gy=3 * p, N=2, D=4, H=32, W=32, C=4, nimg=3, nc=2, st=A.MASTER | A.FLIP, dt=0, ws=p: \
        lib.m1_aug_geom(x, y, t, gx, gy, N, D, H, W, C, nimg, nc, st, dt, ws, None)
    assert geom(x=None) == BAD and geom(t=None) == BAD and geom(gx=None) == BAD and geom(gy=None) == BAD
    assert geom(N=0) == BAD and geom(D=0) == BAD and geom(C=0) == BAD and geom(nimg=5, C=4) == BAD
    assert geom(dt=7) == BAD and geom(dt=L.M1_BF16) == UNS
    assert geom(W=48, st=A.MASTER | A.ZOOM) == UNS and geom(W=48, st=A.MASTER | A.POOR) == UNS
    assert geom(st=A.MASTER | A.GAMMA, ws=None) == BAD
    gst = lambda gx=p, t=p, N=2, H=32, W=32, st=A.MASTER | A.GAMMA, dt=0, ws=p: \
        lib.m1_aug_gamma_stats(gx, t, N, 4, H, W, 4, 3, st, dt, ws, None)
    assert gst(gx=None) == BAD and gst(t=None) == BAD and gst(ws=None) == BAD and gst(N=0) == BAD
    assert gst(dt=9) == BAD and gst(dt=L.M1_BF16) == UNS and gst(W=48, st=A.MASTER | A.GAMMA | A.POOR) == UNS
    inten = lambda gx=p, t=p, rng=p, out=2 * p, N=2, H=32, W=32, st=A.MASTER | A.NOISE, dt=0, ws=p: \
        lib.m1_aug_intensity(gx, t, rng, 0, out, N, 4, H, W, 4, 3, st, dt, ws, None)
    assert inten(gx=None) == BAD and inten(t=None) == BAD and inten(out=None) == BAD and inten(rng=None) == BAD
    assert inten(N=0) == BAD and inten(H=0) == BAD and inten(dt=5) == BAD and inten(dt=L.M1_BF16) == UNS
    assert inten(W=48, st=A.MASTER | A.POOR) == UNS and inten(W=48, st=A.MASTER | A.ZOOM) == UNS


# ---- CPU 3: surface -----------------------------------------------------------------------------------------------------------------
def test_surface_has_the_reference_signatures():
    want = {"augment_tensors": ["features", "targets", "augmentation_params", "train_obj", "debug_on"],
            "zoom_4D_tensor": ["input_tensor", "scale"], "axial_4D_hflip": ["input_tensor"],
            "translate_4D_tensor": ["input_tensor", "pad_mode", "pad_top", "pad_bottom", "pad_right", "pad_left"],
            "channel_shift_4D_tensor": ["input_tensor", "pad_mode", "pad_top", "pad_bottom", "pad_right", "pad_left"],
            "rotate_4D_tensor": ["input_tensor", "pad_mode", "angle"], "sim_poor_scan_4D_tensor": ["input_tensor", "train_obj"],
            "gamma_shift_4D_tensor": ["input_tensor", "gamma", "train_obj"],
            "gaussian_noise_4D_tensor": ["input_tensor", "stddev", "train_obj"]}
    for name, params in want.items():
        sig = inspect.signature(getattr(A, name))
        pos = [k for k, v in sig.parameters.items() if v.kind == v.POSITIONAL_OR_KEYWORD]
        assert pos == params, name
    s = inspect.signature(A.augment_tensors).parameters
    assert s["train_obj"].default == 'lesion' and s["debug_on"].default is False
    assert s["rng"].kind == s["rng"].KEYWORD_ONLY and s["params"].kind == s["params"].KEYWORD_ONLY
    import model.augmentations as MA                             # the reference's import path (train_model.py:22)
    assert MA is A


def test_host_tensors_raise():
    x = torch.zeros(1, 2, 8, 8, 4)
    y = torch.zeros(1, 2, 8, 8, 2)
    with pytest.raises(RuntimeError, match="HIP extension"):
        A.augment_tensors({"image": x}, {"detection": y}, DEFAULT)
    for fn in (A.zoom_4D_tensor, A.axial_4D_hflip, A.translate_4D_tensor, A.channel_shift_4D_tensor, A.rotate_4D_tensor,
               A.sim_poor_scan_4D_tensor, A.gamma_shift_4D_tensor, A.gaussian_noise_4D_tensor):
        with pytest.raises(RuntimeError, match="HIP extension"):
            fn(x[0])


def test_parser_and_hyper_parameter_forms():
    a = T.build_parser().parse_args([])
    assert a.AUGMENT == 0 and a.AUGM_PARAMS == DEFAULT
    want = [1.0, 0.25, 0.15, 10.0, 1.0, 1.2, 0.1, 0.025, 1.0, 0.5, 1.5]
    assert A.parse_augm_params(a.AUGM_PARAMS) == want
    flat = "--AUGMENT 1 --AUGM_PARAMS 1.0 0.25 0.15 10 1 1.2 0.1 0.025 1 0.5 1.5".split()
    b = T.build_parser().parse_args(flat)
    assert b.AUGMENT == 1 and A.parse_augm_params(b.AUGM_PARAMS) == want
    with pytest.raises(SystemExit):
        T.build_parser().parse_args("--AUGM_PARAMS 1.0 0.25 0.15 10 1 1.2 0.1 0.025 1 0.5".split())
    with pytest.raises(ValueError, match="AUGM_PARAMS"):
        A.parse_augm_params([1.0, 0.25, 0.15])
    with pytest.raises(ValueError, match="AUGM_PARAMS"):         # ten scalars: the gamma range is missing
        A.parse_augm_params([1.0, 0.25, 0.15, 10.0, True, 1.2, 0.1, 0.025, True, 0])
    assert not A.enabled_stages([1.0, 0.25, 0.15, 10.0, 2.0, 1.2, 0.1, 0.025, 1.0, 0.5, 1.5]) & A.FLIP     # `axial_hflip==True` (A:65)
    assert A.enabled_stages(want, 'lesion') == 0x1FF and A.enabled_stages(want, 'zonal') == 0x1FF & ~A.CSHIFT
    assert A.enabled_stages(A.parse_augm_params([1, 0.25, 0, 0, False, 0, 0, 0, False, [0, 0]])) == A.MASTER
    with pytest.raises(ValueError, match="143-148"):
        A.check_geometry(A.ZOOM, 32, 48)
    with pytest.raises(ValueError, match="267-268"):
        A.check_geometry(A.POOR, 32, 48)
    assert "out of scope" not in T.__doc__ and "--AUGMENT" in T.__doc__


# ---- GPU helpers --------------------------------------------------------------------------------------------------------------------
def _problem(obj, size, seed):
    """lesion: 3 sequences + 1 label channel, 2 classes; zonal: 1 sequence + 2 label channels, 3 classes."""
    N, D, H = (2, 4, 32) if size == "small" else (2, 20, 160)
    nimg, nc = (3, 2) if obj == "lesion" else (1, 3)
    g = np.random.default_rng(1000 + seed)
    lab_idx = g.integers(0, nc, size=(N, D, H // 8, H // 8)).repeat(8, axis=2).repeat(8, axis=3)
    lab = np.stack([(lab_idx == k) for k in range(nc)], axis=-1).astype(f32)
    img = np.concatenate([g.standard_normal((N, D, H, H, nimg)).astype(f32), lab[..., 1:]], axis=-1)
    return img, lab, nimg


def _records(N, H, seed, fired, obj):
    g = np.random.default_rng(77 + seed)
    out = []
    for n in range(N):
        out.append(dict(fired=A.MASTER | fired, scale=int(g.integers(H, math.ceil(H * 1.2))), angle_deg=float(g.uniform(-10, 10)),
                        tr=[int(v) for v in g.integers(0, math.ceil(H * 0.15), 4)], cs=[int(v) for v in g.integers(0, max(2, math.ceil(H * 0.025)) + 1, 4)],
                        cs_channel=int(g.integers(0, 3)), gamma=float(g.uniform(0.5, 1.5)), noise_std=float(g.uniform(0.02, 0.1)),
                        gamma_ch=int(g.integers(1, 8)) if obj == "lesion" else 1, poor_ch=int(g.integers(1, 8)) if obj == "lesion" else 1))
    return out


def _noise_draws(dev, shape, nimg, rng):
    """The N(0,1) draws of the noise stage: the stage on a zero image with stddev 1 returns them."""
    z = A.gaussian_noise_4D_tensor(torch.zeros(shape, device=dev), stddev=1.0, train_obj='lesion' if nimg == 3 else 'zonal', rng=rng)
    return z.cpu().numpy()


def _k_roundings(stages):
    bits = {"zoom": A.ZOOM, "rotate": A.ROTATE, "gamma": A.GAMMA, "poor": A.POOR, "noise": A.NOISE}
    return sum(K_ROUNDINGS[k] for k, b in bits.items() if stages & b)


def _compare(got_x, got_y, img, lab, recs, stages, nimg, z, exact, label):
    """Every element of image and label of every sample against the fp64 restatement: bit-exact, or within max(floor, 4 e32)."""
    worst = dict(e32=0.0, err=0.0, tol=0.0)
    for n in range(img.shape[0]):
        zn = None if z is None else z[n]
        x64, y64 = r_chain(img[n], lab[n], recs[n], stages, nimg, np.float64, zn)
        if exact:
            assert np.array_equal(got_x[n], x64.astype(f32)) and np.array_equal(got_y[n], y64.astype(f32)), (label, n)
            continue
        x32, y32 = r_chain(img[n], lab[n], recs[n], stages, nimg, np.float32, zn)
        for got, r64, r32, what in ((got_x[n], x64, x32, "image"), (got_y[n], y64, y32, "label")):
            e32 = float(np.abs(r32.astype(np.float64) - r64).max())
            if what == "label" and not (int(recs[n]["fired"]) & stages & (A.ZOOM | A.ROTATE)):
                assert np.array_equal(got, r64.astype(f32)), (label, n, what)      # no interpolating stage touched it: a copy / index map
                continue
            k = _k_roundings(stages if what == "image" else stages & (A.ZOOM | A.ROTATE))
            floor = k * 2.0 ** -24 * float(np.abs(r64).max())
            tol = max(floor, 4 * e32)
            err = float(np.abs(got.astype(np.float64) - r64).max())
            print(f"{label} sample {n} {what}: k {k} e32 {e32:.3e} floor {floor:.3e} product error {err:.3e}")
            if err / tol > worst["err"] / max(worst["tol"], 1e-300):
                worst = dict(e32=e32, err=err, tol=tol)
            assert err <= tol, (label, n, what, err, tol, e32)
        if not (int(recs[n]["fired"]) & A.MASTER):
            assert np.array_equal(got_x[n], img[n]) and np.array_equal(got_y[n], lab[n])
        # the label channels of the image take no intensity stage: geometry only
        if not (int(recs[n]["fired"]) & stages & (A.ZOOM | A.ROTATE)):
            assert np.array_equal(got_x[n][..., nimg:], x64[..., nimg:].astype(f32)), (label, n)
    return worst


STAGES = {"zoom": A.ZOOM, "flip": A.FLIP, "rotate": A.ROTATE, "translate": A.TRANSLATE, "cshift": A.CSHIFT, "gamma": A.GAMMA,
          "poor": A.POOR, "noise": A.NOISE, "chain": 0x1FE}
EXACT = {"flip", "translate", "cshift"}


# ---- GPU 4: every stage alone and the whole chain, injected tables ---------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("size", ["small", "big"])
@pytest.mark.parametrize("obj", ["lesion", "zonal"])
@pytest.mark.parametrize("stage", list(STAGES))
def test_stage_and_chain_match_the_fp64_restatement(dev, stage, obj, size):
    bits = STAGES[stage]                                         # (cshift on 'zonal': A:85 never enables it -- the sample passes unchanged)
    for seed in ((0, 1, 2) if size == "small" else (0,)):
        img, lab, nimg = _problem(obj, size, seed)
        N, D, H = img.shape[:3]
        train_obj = obj
        hyper = [1.0, 0.25, 0.15 if bits & A.TRANSLATE else 0, 10.0 if bits & A.ROTATE else 0, bool(bits & A.FLIP),
                 1.2 if bits & A.ZOOM else 0, 0.1 if bits & A.NOISE else 0, 0.025 if bits & A.CSHIFT else 0, bool(bits & A.POOR),
                 [0.5, 1.5] if bits & A.GAMMA else [0, 0]]
        stages = A.enabled_stages(A.parse_augm_params(hyper), train_obj)
        rec_d = _records(N, H, seed, bits, obj)
        if seed == 1:
            rec_d[1]["fired"] = bits                             # master coin not fired: the sample is copied
        table = A.draw_params(None, N, H, H, explicit=rec_d, device=dev)
        recs = A.table_to_numpy(table)
        rng = A.new_rng(11 + seed, dev)
        z = _noise_draws(dev, img.shape, nimg, rng) if bits & A.NOISE else None
        f, t = A.augment_tensors({"image": torch.from_numpy(img).to(dev)}, {"detection": torch.from_numpy(lab).to(dev), "KL": None},
                                 hyper, train_obj=train_obj, rng=rng, params=table)
        assert t["KL"] is None
        got_x, got_y = f["image"].cpu().numpy(), t["detection"].cpu().numpy()
        exact = stage in EXACT
        _compare(got_x, got_y, img, lab, recs, stages, nimg, z, exact, f"{stage}/{obj}/{size}/seed{seed}")


# ---- GPU 5: cell choices ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("H", [32, 160])
def test_cell_choices_equal_the_restatements(dev, H):
    """Input that encodes its own position (channel 0 = column index, channel 1 = row index, channel 2 = row * W + column), one
    stage at a time.  With the same fp32 coordinates the kernel and the fp32-valued restatement perform the same IEEE operations
    on the same cells, so the outputs are EQUAL; one coordinate off by a last bit (an fma contraction) moves a floor or a weight
    and shows.  For zoom and poor scan the column channel decodes directly: a bilinear tap of a ramp returns lo + t = the fp32
    source coordinate itself, clamped at the edges."""
    D = 2
    yy, xx = np.meshgrid(np.arange(H, dtype=f32), np.arange(H, dtype=f32), indexing="ij")
    img = np.broadcast_to(np.stack([xx, yy, yy * H + xx], axis=-1), (1, D, H, H, 3)).copy()
    x = torch.from_numpy(img).to(dev)
    for scale in sorted({H, H + 1, H + 7, math.ceil(H * 1.2) - 1}):
        got = A.zoom_4D_tensor(x[0], scale=scale).cpu().numpy()
        assert np.array_equal(got, r_zoom(img[0], scale, np.float32)), scale
        _, _, _, src = r_resize_taps(H, scale)
        want_col = np.clip(src[scale - H:], 0, H - 1)             # the source coordinate of every output column
        assert np.array_equal(got[0, 0, :, 0], want_col), scale
    for angle in (-10.0, -3.3, 0.7, 9.99, 45.0):
        got = A.rotate_4D_tensor(x[0], angle=angle).cpu().numpy()
        assert np.array_equal(got, r_rotate(img[0], A.rotation_coefficients(angle, H, H), np.float32)), angle
    got = A.sim_poor_scan_4D_tensor(x[0], channel_coins=[True, True, True]).cpu().numpy()
    want = np.concatenate([r_poor_channel(img[0][..., c:c + 1], np.float32) for c in range(3)], axis=-1)
    assert np.array_equal(got, want)
    h2 = int(H * 0.75)
    _, _, _, src = r_resize_taps(H, h2)
    assert np.array_equal(got[0, 0, :, 0], np.clip(src, 0, H - 1)[r_nearest_index(h2, H)])    # nearest picks of bilinear taps


# ---- GPU 6: noise -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_noise_draws_are_standard_normal_keyed_by_seed_and_step(dev):
    shape = (2, 20, 160, 160, 4)
    rng = A.new_rng(5, dev)
    z = A.gaussian_noise_4D_tensor(torch.zeros(shape, device=dev), stddev=1.0, rng=rng)
    z2 = A.gaussian_noise_4D_tensor(torch.zeros(shape, device=dev), stddev=1.0, rng=rng)
    assert torch.equal(z, z2)                                     # same {seed, step}: bit-identical
    assert not z[..., 3].any()                                    # the label channel receives none
    v = z[..., :3].double().cpu().numpy().ravel()
    n = v.size
    assert n == 2 * 20 * 160 * 160 * 3
    se_mean, se_var = 1.0 / math.sqrt(n), math.sqrt(2.0 / n)      # standard errors of the mean and of the variance of N(0,1) samples
    print(f"noise: n {n} mean {v.mean():.3e} (5 se {5 * se_mean:.3e}) var-1 {v.var() - 1:.3e} (5 se {5 * se_var:.3e})")
    assert abs(v.mean()) < 5 * se_mean and abs(v.var() - 1.0) < 5 * se_var
    ops.step_advance(None, rng)
    z3 = A.gaussian_noise_4D_tensor(torch.zeros(shape, device=dev), stddev=1.0, rng=rng)
    assert not torch.equal(z, z3)
    zz = A.gaussian_noise_4D_tensor(torch.zeros((1, 2, 32, 32, 3), device=dev), stddev=1.0, train_obj='zonal', rng=rng)
    assert zz[..., 0].any() and not zz[..., 1:].any()


# ---- GPU 7: the drawn table -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_drawn_table_statistics_ranges_and_chain(dev):
    n, H = 4096, 32
    hyper = [0.80, 0.25, 0.15, 10.0, True, 1.20, 0.10, 0.10, True, [0.50, 1.50]]
    rng = A.new_rng(3, dev)
    t = A.table_to_numpy(A.draw_params(hyper, n, H, H, rng=rng))
    t_again = A.table_to_numpy(A.draw_params(hyper, n, H, H, rng=rng))
    assert t.tobytes() == t_again.tobytes()
    assert A.table_to_numpy(A.draw_params(hyper, n, H, H, rng=rng, stream_id=A.STREAM_DRAW + 2)).tobytes() != t.tobytes()

    def check(count, total, p, what):
        bound = 5 * math.sqrt(p * (1 - p) / total)                # five binomial standard deviations
        print(f"{what}: {count}/{total} = {count / total:.4f}, expected {p} +- {bound:.4f}")
        assert abs(count / total - p) < bound, what
    master = (t["fired"] & A.MASTER) != 0
    m = int(master.sum())
    assert 5 * math.sqrt(0.75 * 0.25 / m) < 0.25                  # the bound separates 0.75 from 0.25 (and from 0.5)
    check(m, n, 0.80, "master")
    assert not t["fired"][~master].any()
    tm = t[master]
    for bit, name in ((A.ZOOM, "zoom"), (A.ROTATE, "rotate"), (A.TRANSLATE, "translate"), (A.CSHIFT, "cshift"), (A.GAMMA, "gamma"),
                      (A.POOR, "poor"), (A.NOISE, "noise")):
        check(int(((tm["fired"] & bit) != 0).sum()), m, 0.75, name)
    check(int(((tm["fired"] & A.FLIP) != 0).sum()), m, 0.5, "flip")
    for field, bit in (("gamma_ch", A.GAMMA), ("poor_ch", A.POOR)):
        on = tm[(tm["fired"] & bit) != 0]
        for c in range(3):
            check(int(((on[field] >> c) & 1).sum()), len(on), 0.5, f"{field}[{c}]")
        assert not (on[field] >> 3).any() and not tm[(tm["fired"] & bit) == 0][field].any()
    assert tm["scale"].min() == H and tm["scale"].max() == math.ceil(f32(H * 1.20)) - 1
    for field, hi in (("tr", math.ceil(f32(H * 0.15))), ("cs", math.ceil(f32(H * 0.10)))):
        for k in range(4):
            assert tm[field][:, k].min() == 0 and tm[field][:, k].max() == hi - 1, (field, k)
    ch = tm[(tm["fired"] & A.CSHIFT) != 0]["cs_channel"]
    assert sorted(set(ch.tolist())) == [0, 1, 2]
    assert tm["angle_deg"].min() >= -10.0 and tm["angle_deg"].max() < 10.0 and tm["angle_deg"].min() < -9.9 and tm["angle_deg"].max() > 9.9
    assert tm["gamma"].min() >= 0.5 and tm["gamma"].max() < 1.5
    assert tm["noise_std"].min() >= 0.0 and tm["noise_std"].max() < f32(0.10)
    assert (tm["rot_pad"] == A.rotation_pad(H, H)).all()
    for r in tm[:64]:                                             # the coefficients are tfa's for the drawn angle, to fp32 cos / sin rounding
        assert np.abs(r["rot"] - A.rotation_coefficients(r["angle_deg"], H, H)).max() < 1e-4
    ops.step_advance(None, rng)
    assert A.table_to_numpy(A.draw_params(hyper, n, H, H, rng=rng)).tobytes() != t.tobytes()
    # a stage whose hyper-parameter is zero never fires (and draws nothing)
    off = A.table_to_numpy(A.draw_params([1.0, 0.25, 0, 0, False, 0, 0, 0, False, [0, 0]], n, H, H, rng=rng))
    assert (off["fired"] == A.MASTER).all()
    zon = A.table_to_numpy(A.draw_params(DEFAULT, n, H, H, 'zonal', rng=rng))
    assert not (zon["fired"] & A.CSHIFT).any() and not (zon["gamma_ch"] >> 1).any()
    # one drawn table, read back, drives the restatement for a whole-chain comparison
    for obj in ("lesion", "zonal"):
        img, lab, nimg = _problem(obj, "small", 9)
        rng2 = A.new_rng(21, dev)
        recs = A.table_to_numpy(A.draw_params(DEFAULT, img.shape[0], H, H, obj, rng=rng2))
        z = _noise_draws(dev, img.shape, nimg, rng2)
        f, tg = A.augment_tensors({"image": torch.from_numpy(img).to(dev)}, {"detection": torch.from_numpy(lab).to(dev)}, DEFAULT,
                                  train_obj=obj, rng=rng2)
        stages = A.enabled_stages(A.parse_augm_params(DEFAULT), obj)
        _compare(f["image"].cpu().numpy(), tg["detection"].cpu().numpy(), img, lab, recs, stages, nimg, z, False, f"drawn/{obj}")


# ---- GPU 8: determinism and capture ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_chain_is_deterministic_and_replays_bit_exact_from_a_graph(dev):
    img, lab, _ = _problem("lesion", "small", 4)
    x_s, y_s = torch.from_numpy(img).to(dev), torch.from_numpy(lab).to(dev)
    seed = 17

    def eager(step):
        rng = torch.tensor([seed, step], dtype=torch.int64, device=dev)
        f, t = A.augment_tensors({"image": x_s}, {"detection": y_s}, DEFAULT, rng=rng)
        return f["image"].clone(), t["detection"].clone()
    a, b = eager(0), eager(0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0], x_s)
    rng = A.new_rng(seed, dev)

    def step():
        f, t = A.augment_tensors({"image": x_s}, {"detection": y_s}, DEFAULT, rng=rng)
        ops.step_advance(None, rng)
        return f["image"], t["detection"]
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        step()
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    rng.copy_(torch.tensor([seed, 0], dtype=torch.int64))
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(gr):
        gx, gy = step()
    hist = PKG.hip.graphs.assert_no_memset_nodes(gr)
    assert hist.get("memcpy", 0) == 0 and hist.get("kernel", 0) >= 6, hist     # draw, geom + fold, gamma stats + fold, intensity, advance
    gr.instantiate()
    for k in range(3):
        gr.replay()
        torch.cuda.synchronize()
        ex, ey = eager(k)
        assert torch.equal(gx, ex) and torch.equal(gy, ey), k
    assert int(rng[1]) == 3
    del gr


# ---- GPU 9: trainer ----------------------------------------------------------------------------------------------------------------
def _trainer_args(tmp_path, name):
    return ["--WEIGHTS_DIR", str(tmp_path) + "/", "--NAME", name, "--FOLDS", "0", "--UNET_FEATURE_CHANNELS", "8", "16", "32", "64", "128",
            "--UNET_PROBABILISTIC", "1", "--UNET_DENSE_SKIP", "1", "--SYNTHETIC_SAMPLES", "4", "--IMAGE_SPATIAL_DIMS", "4", "32", "32",
            "--BATCH_SIZE", "2", "--UNET_DROPOUT_RATE", "0", "--WEIGHTS_MIN_EPOCH", "2", "--STORE_WEIGHTS_PER_N_EPOCHS", "2",
            "--COMPUTE_DTYPE", "fp32"]


@pytest.mark.gpu
def test_trainer_with_augmentation_trains(dev, tmp_path):
    (model, hist, _), = T.main(_trainer_args(tmp_path, "aug") + ["--NUM_EPOCHS", "4", "--AUGMENT", "1"])
    assert len(hist.history["loss"]) == 4 and all(np.isfinite(hist.history["loss"]))
    assert set(hist.history) == {"loss", "detection_loss", "KL_loss"}
    assert model.optimizer.iterations == 8


@pytest.mark.gpu
def test_trainer_off_is_the_old_path_and_probability_zero_passes_batches_through(dev, tmp_path, monkeypatch):
    calls = []
    real = A.augment_tensors

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(T.augmentations, "augment_tensors", counting)
    seen = []
    M1 = PKG.unets.networks.M1
    real_step = M1.train_step

    def recording(self, x, y):
        seen.append(({k: v.clone() for k, v in x.items()}, {k: v.clone() for k, v in y.items()}))
        return real_step(self, x, y)
    monkeypatch.setattr(M1, "train_step", recording)
    T.main(_trainer_args(tmp_path, "off") + ["--NUM_EPOCHS", "1", "--AUGMENT", "0"])
    assert calls == [] and len(seen) == 2                         # off: augment_tensors is never called
    del seen[:]
    T.main(_trainer_args(tmp_path, "p0") + ["--NUM_EPOCHS", "1", "--AUGMENT", "1", "--AUGM_PARAMS", "0", "0.25", "0.15", "10", "1", "1.2",
                                            "0.1", "0.025", "1", "0.5", "1.5"])
    assert len(calls) == 2 and len(seen) == 2
    g = np.random.default_rng(0)
    cases = [T.synthetic_case(g, (4, 32, 32), 3, 2) for _ in range(4)]
    gen = T.batches(T.custom_data_generator(cases, probabilistic=True, mode='train'), 2, dev)
    for bx, by in seen:
        wx, wy = next(gen)
        assert set(bx) == set(wx) and set(by) == set(wy)
        for k in wx:
            assert torch.equal(bx[k], wx[k]), k
        for k in wy:
            assert torch.equal(by[k], wy[k]), k
