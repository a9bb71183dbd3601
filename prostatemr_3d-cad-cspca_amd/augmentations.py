"""Train-time augmentations on the GPU: the counterpart of the reference's ``model/augmentations.py``
(tf2.5/scripts/model/augmentations.py, cited as ``A:``), on BATCHED device tensors.

``augment_tensors`` keeps the reference's signature and return value (A:36-132).  The reference maps it over single samples
before ``dataset.batch``; here ``features["image"]`` is (N,D,H,W,C) and ``targets["detection"]`` (N,D,H,W,nc), and every sample
of the batch has its own draws.  All arithmetic runs in csrc/augment.hip behind the C ABI (include/m1hip.h, m1_aug_*): there is
no CPU path, host tensors raise.

Everything random reaches the kernels through one plain-data table, one ``m1_aug_params_t`` record per sample: drawn on the
device (``draw_params(..., rng=)``: Philox keyed by a device-resident {seed, step} pair, no host synchronisation, fresh draws on
every replay of a captured graph) or built from explicit values (``draw_params(..., explicit=[...])``).  The helper functions of
A:139-326 exist with the reference's arguments and run their single stage through the same kernels (a table with one stage
fired); their own random choices (A:189 channel, A:265 / A:299 per-channel coins) come from keyword-only arguments or Python's
``random``.
"""
from __future__ import annotations

import math
import random
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .hip import lib as L
from .hip import ops

MASTER, ZOOM, FLIP, ROTATE, TRANSLATE = L.M1_AUG_MASTER, L.M1_AUG_ZOOM, L.M1_AUG_FLIP, L.M1_AUG_ROTATE, L.M1_AUG_TRANSLATE
CSHIFT, GAMMA, POOR, NOISE = L.M1_AUG_CSHIFT, L.M1_AUG_GAMMA, L.M1_AUG_POOR, L.M1_AUG_NOISE

# numpy view of m1_aug_params_t (include/m1hip.h)
AUG_DTYPE = np.dtype([("fired", "<u4"), ("gamma_ch", "<u4"), ("poor_ch", "<u4"), ("scale", "<i4"), ("rot_pad", "<i4"),
                      ("rot", "<f4", (6,)), ("tr", "<i4", (4,)), ("cs", "<i4", (4,)), ("cs_channel", "<i4"), ("gamma", "<f4"),
                      ("noise_std", "<f4"), ("angle_deg", "<f4"), ("_pad", "<i4")])
assert AUG_DTYPE.itemsize == ops.AUG_RECORD_BYTES

STREAM_DRAW, STREAM_NOISE = 0xA06D, 0xA06E          # Philox stream ids of the table draws and of the noise (+ 2 * rank in the trainer)
_DEFAULT_RNG: Dict[torch.device, torch.Tensor] = {}


def parse_augm_params(augmentation_params: Sequence) -> List[float]:
    """The ten entries of ``AUGM_PARAMS`` (A:39-48) as eleven numbers, the gamma range last.  Accepts the reference's nested
    default ``[..., [0.50, 1.50]]`` and the flat list of eleven floats a command line yields; any other shape is an error."""
    p = list(augmentation_params)
    if len(p) == 10 and isinstance(p[9], (list, tuple, np.ndarray)) and len(p[9]) == 2:
        p = p[:9] + [p[9][0], p[9][1]]
    elif len(p) != 11 or any(isinstance(v, (list, tuple, np.ndarray)) for v in p):
        raise ValueError(f"AUGM_PARAMS: expected the ten entries of augmentations.py:39-48 with a [lo, hi] gamma range last, or eleven "
                         f"numbers (the range flattened), got {len(p)} entries")
    return [float(v) for v in p]


def enabled_stages(hyper: Sequence[float], train_obj: str = 'lesion') -> int:
    """The stages the ``if``s of A:58-108 enable for these hyper-parameters."""
    _, _, tr, rot, flip, zoom, noise, cs, poor, g0, g1 = hyper
    s = MASTER
    s |= ZOOM if zoom != 0.0 else 0
    s |= FLIP if flip == True else 0                             # noqa: E712 -- `axial_hflip==True` (A:65)
    s |= ROTATE if rot != 0 else 0
    s |= TRANSLATE if tr != 0.0 else 0
    s |= CSHIFT if (train_obj == 'lesion' and cs != 0) else 0
    s |= GAMMA if (g0 + g1) != 0 else 0
    s |= POOR if poor != False else 0                            # noqa: E712 -- `sim_poor_scan!=False` (A:103)
    s |= NOISE if noise != 0 else 0
    return s


def _image_channels(train_obj: str) -> int:
    if train_obj == 'lesion':
        return 3
    if train_obj == 'zonal':
        return 1
    raise ValueError(f"train_obj {train_obj!r}: 'lesion' or 'zonal' (augmentations.py:85,244,254)")


def rotation_pad(H: int, W: int) -> int:
    """A:222-223."""
    return int(np.ceil(((H ** 2 + W ** 2) ** 0.5 - min(H, W)) / 2))


def central_crop_start(Hp: int, fraction: float) -> int:
    """tf.image.central_crop: ``int((Hp - Hp * fraction) / 2)`` in double arithmetic."""
    return int((float(Hp) - float(Hp) * fraction) / 2)


def check_geometry(stages: int, H: int, W: int) -> None:
    """What the reference's pipeline would break on: zoom / poor scan use shape[1] for both axes (A:60-61,143-148; A:267-268), and
    the rotation's central crop (A:233-234) must give back (H, W)."""
    if stages & (ZOOM | POOR) and H != W:
        raise ValueError(f"zoom / poor-scan augmentation on a non-square slice ({H}x{W}): augmentations.py:60-61,143-148 and 267-268 "
                         "use shape[1] for both axes")
    if stages & ROTATE:
        pad = rotation_pad(H, W)
        Hp, Wp = H + 2 * pad, W + 2 * pad
        frac = H / Hp
        sh, sw = central_crop_start(Hp, frac), central_crop_start(Wp, frac)
        if Hp - 2 * sh != H or Wp - 2 * sw != W:
            raise ValueError(f"rotation augmentation: central_crop(fraction {H}/{Hp}) of the padded {Hp}x{Wp} slice gives "
                             f"{Hp - 2 * sh}x{Wp - 2 * sw}, not {H}x{W} (augmentations.py:233-234)")


def rotation_coefficients(angle_deg, H: int, W: int) -> np.ndarray:
    """The six fp32 coefficients tfa.image.rotate hands to the projective transform for ``angle*math.pi/180`` (A:232) on the
    padded slice: [cos, -sin, x_off, sin, cos, y_off], all in fp32 as tfa's angles_to_projective_transforms computes them."""
    f = np.float32
    pad = rotation_pad(H, W)
    rad = f(f(f(angle_deg) * f(math.pi)) / f(180.0))
    c, s = f(np.cos(rad)), f(np.sin(rad))
    w1, h1 = f(W + 2 * pad - 1), f(H + 2 * pad - 1)
    x_off = f(f(w1 - f(f(c * w1) - f(s * h1))) / f(2.0))
    y_off = f(f(h1 - f(f(s * w1) + f(c * h1))) / f(2.0))
    return np.array([c, -s, x_off, s, c, y_off], dtype=np.float32)


def _record(H: int, W: int, e: Optional[dict] = None) -> np.ndarray:
    r = np.zeros((), dtype=AUG_DTYPE)
    r["scale"], r["rot_pad"], r["gamma"] = H, rotation_pad(H, W), 1.0
    r["rot"] = (1, 0, 0, 0, 1, 0)
    for k, v in (e or {}).items():
        if k == "angle_deg":
            r["angle_deg"] = v
            r["rot"] = rotation_coefficients(v, H, W)
        elif k not in AUG_DTYPE.names:
            raise ValueError(f"unknown augmentation table field {k!r}")
        else:
            r[k] = v
    return r


def table_to_numpy(table: torch.Tensor) -> np.ndarray:
    """A device table as a numpy structured array (AUG_DTYPE), one record per sample.  Synchronises."""
    return table.detach().cpu().numpy().reshape(-1).view(AUG_DTYPE).copy()


def table_from_numpy(records: np.ndarray, device) -> torch.Tensor:
    raw = np.ascontiguousarray(records.astype(AUG_DTYPE, copy=False)).view(np.uint8).reshape(len(records), AUG_DTYPE.itemsize)
    return torch.from_numpy(raw.copy()).to(device)


def draw_params(augmentation_params: Optional[Sequence], N: int, H: int, W: int, train_obj: str = 'lesion', *, rng: Optional[torch.Tensor] = None,
                stream_id: int = STREAM_DRAW, explicit: Optional[Sequence[dict]] = None, device=None) -> torch.Tensor:
    """The table of one batch, (N, record bytes) uint8 on the device.

    ``rng=`` (device int64 {seed, step}): drawn by m1_aug_draw in the draw order of A:51-111 for the given hyper-parameters.
    ``explicit=`` (N dicts of m1_aug_params_t fields; ``angle_deg`` also fills ``rot``; missing fields are the identity): built on
    the host and copied."""
    if explicit is not None:
        if len(explicit) != N:
            raise ValueError(f"explicit table: {len(explicit)} records for {N} samples")
        recs = np.stack([_record(H, W, e) for e in explicit])
        return table_from_numpy(recs, device if device is not None else (rng.device if rng is not None else torch.device("cuda")))
    if rng is None:
        raise ValueError("draw_params needs rng= (a device {seed, step} pair) or explicit= values")
    hyper = parse_augm_params(augmentation_params)
    check_geometry(enabled_stages(hyper, train_obj), H, W)
    return ops.aug_draw(N, rng, stream_id, hyper, H, W, _image_channels(train_obj), train_obj == 'lesion')


def new_rng(seed: int, device) -> torch.Tensor:
    """A device-resident {seed, step} pair (``ops.step_advance(None, rng)`` moves it to the next step)."""
    return torch.tensor([int(seed), 0], dtype=torch.int64, device=device)


def _default_rng(device) -> torch.Tensor:
    if device not in _DEFAULT_RNG:
        _DEFAULT_RNG[device] = new_rng(0, device)
    return _DEFAULT_RNG[device]


def augment_tensors(features, targets, augmentation_params, train_obj='lesion', debug_on=False, *, rng=None, params=None,
                    stream_id=0):
    """A:36-132 on a batch.  ``rng=``: the device {seed, step} pair the draws and the noise are keyed by (the caller advances it;
    without it a module-level pair is used and advanced after every call).  ``params=``: an injected table (``draw_params``)
    instead of fresh draws.  ``stream_id`` separates callers that share a pair (ranks).  Returns ``(features, targets)`` with
    ``features["image"]`` and ``targets["detection"]`` replaced; other entries (``"KL"``) are passed through untouched."""
    x, y = features["image"], targets["detection"]
    ops._req(x, y)
    hyper = parse_augm_params(augmentation_params)
    nimg = _image_channels(train_obj)
    stages = enabled_stages(hyper, train_obj)
    if x.dim() != 5 or nimg > int(x.shape[-1]):
        raise ValueError(f"features['image'] must be (N,D,H,W,C) with C >= {nimg} for train_obj {train_obj!r}, got {tuple(x.shape)}")
    N, _, H, W, _ = (int(v) for v in x.shape)
    check_geometry(stages, H, W)
    own = rng is None
    if own:
        rng = _default_rng(x.device)
    if params is None:
        params = ops.aug_draw(N, rng, STREAM_DRAW + 2 * int(stream_id), hyper, H, W, nimg, train_obj == 'lesion')
    gx, gy = ops.aug_apply(x.contiguous(), y.contiguous(), params, stages, nimg, rng, STREAM_NOISE + 2 * int(stream_id))
    if debug_on:                                                 # A:123-127: label-swap sanity check (synchronises)
        a, b = math.ceil(float(y.max())), math.ceil(float(gy.max()))
        if a != b:
            print(a)
            print(b)
    if own:
        ops.step_advance(None, rng)
    features, targets = dict(features), dict(targets)
    features["image"], targets["detection"] = gx, gy
    return features, targets


# ---- the helpers of A:139-326: one stage through the same kernels ---------------------------------------------------------------
def _one_stage(input_tensor: torch.Tensor, stage: int, nimg: int, rng=None, **fields) -> torch.Tensor:
    ops._req(input_tensor)
    x = input_tensor if input_tensor.dim() == 5 else input_tensor.unsqueeze(0)
    if x.dim() != 5:
        raise ValueError(f"expected a (D,H,W,C) tensor (or a batch of them), got {tuple(input_tensor.shape)}")
    N, _, H, W, Cn = (int(v) for v in x.shape)
    check_geometry(stage, H, W)
    fields["fired"] = MASTER | stage
    table = draw_params(None, N, H, W, explicit=[fields] * N, device=x.device)
    out, _ = ops.aug_apply(x.contiguous().float(), None, table, MASTER | stage, min(nimg, Cn), rng, STREAM_NOISE)
    return out if input_tensor.dim() == 5 else out[0]


def _coins(n: int, coins) -> int:
    bits = [random.random() > 0.5 for _ in range(n)] if coins is None else list(coins)
    return sum(1 << c for c, b in enumerate(bits) if b)


def zoom_4D_tensor(input_tensor, scale=1.00):
    """A:139-152."""
    return _one_stage(input_tensor, ZOOM, 1, scale=int(scale))


def axial_4D_hflip(input_tensor):
    """A:156-163."""
    return _one_stage(input_tensor, FLIP, 1)


def translate_4D_tensor(input_tensor, pad_mode='SYMMETRIC', pad_top=0, pad_bottom=0, pad_right=0, pad_left=0):
    """A:167-181."""
    if pad_mode != 'SYMMETRIC':
        raise NotImplementedError("only pad_mode='SYMMETRIC' (the one augment_tensors uses) runs on the HIP kernels")
    return _one_stage(input_tensor, TRANSLATE, 1, tr=(int(pad_top), int(pad_bottom), int(pad_right), int(pad_left)))


def channel_shift_4D_tensor(input_tensor, pad_mode='SYMMETRIC', pad_top=0, pad_bottom=0, pad_right=0, pad_left=0, *, select_channel=None):
    """A:185-215; ``select_channel`` (A:189) is drawn from Python's ``random`` when not given."""
    if pad_mode != 'SYMMETRIC':
        raise NotImplementedError("only pad_mode='SYMMETRIC' (the one augment_tensors uses) runs on the HIP kernels")
    ch = random.randrange(3) if select_channel is None else int(select_channel)
    return _one_stage(input_tensor, CSHIFT, 1, cs=(int(pad_top), int(pad_bottom), int(pad_right), int(pad_left)), cs_channel=ch)


def rotate_4D_tensor(input_tensor, pad_mode='SYMMETRIC', angle=0):
    """A:219-236; ``angle`` in degrees."""
    if pad_mode != 'SYMMETRIC':
        raise NotImplementedError("only pad_mode='SYMMETRIC' (the one augment_tensors uses) runs on the HIP kernels")
    return _one_stage(input_tensor, ROTATE, 1, angle_deg=float(angle))


def sim_poor_scan_4D_tensor(input_tensor, train_obj='lesion', *, channel_coins=None):
    """A:240-271; ``channel_coins``: the per-channel coins of A:265 (drawn from Python's ``random`` when not given)."""
    n = _image_channels(train_obj)
    return _one_stage(input_tensor, POOR, n, poor_ch=_coins(n, channel_coins))


def gamma_shift_4D_tensor(input_tensor, gamma=1, train_obj='lesion', *, channel_coins=None):
    """A:275-310; ``channel_coins``: the per-channel coins of A:299."""
    n = _image_channels(train_obj)
    return _one_stage(input_tensor, GAMMA, n, gamma=float(gamma), gamma_ch=_coins(n, channel_coins))


def gaussian_noise_4D_tensor(input_tensor, stddev=1.0, train_obj='lesion', *, rng=None):
    """A:314-326; ``rng``: the device {seed, step} pair of the draws (a module-level pair, advanced per call, when not given)."""
    own = rng is None
    if own:
        ops._req(input_tensor)
        rng = _default_rng(input_tensor.device)
    out = _one_stage(input_tensor, NOISE, _image_channels(train_obj), rng=rng, noise_std=float(stddev))
    if own:
        ops.step_advance(None, rng)
    return out
