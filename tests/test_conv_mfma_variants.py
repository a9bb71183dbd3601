"""The large-tile variants of the implicit-GEMM convolution (csrc/conv_mfma.hip) on ragged volumes, against fp64, per element.

conv_mfma is a family of template instantiations chosen by make_plan / run_mfma from COUNTS OF TILES: 128-row tiles from 256 tiles on,
the 8-wave 128x128 tile from 160 blocks on, slab split-K on 128x128 tiles for 100..767 tiles and >= 200 K chunks, K groups inside the
block from 200 64-row tiles on.  No switch lowers those thresholds, so the op tests (about 1,000 voxels) only reach the 64-row forms and
test_convs_at_scale.py meets the large ones at the bench step's own volumes, whose voxel counts per sample are multiples of 128.  Here
they run at 13,000 to 35,000 voxels chosen so that

* (a) N = 1 and M % 128 != 0: a ragged last row tile;
* (b) N >= 2, V % 128 != 0, statistics (or the InstanceNorm-backward sums) asked for: the per-sample tiling (MfmaP::tps);
* (c) the same shape without statistics: one tile holds the last rows of a sample and the first rows of the next.

* part 0 (no GPU): plan_of, a restatement of make_plan + run_mfma + launch_cfg; it reproduces every single-launch conv_mfma name of
  test_convs_at_scale.C3_CONV_KEYS / EXTRA_CONV_KEYS and the names and KC / aligned / per_sample fields of the table below; the bounds
  reject a result (statistics) whose straddling tile took its rows from (credited its rows to) the wrong sample.
* part 1: ROWS, one test per row, at the production dispatch floor (M1_T3_MIN_BLOCKS=128), on shapes the specialised kernels decline
  by themselves: W % 8 != 0 or fewer than 32,768 voxels (conv_halo), fewer than 96 channels or W > 44 or fewer than 4,096 voxels
  (conv_t3), V % 32 != 0 or more than one tap (conv_pw), more than 4 input channels (thin_fwd).  No taker is switched off.
* part 2: SWITCH_ROWS, the switches of run_mfma that nothing else sets, on shapes of part 1, the kernel names asserted to change (or
  not) as plan_of says.
* closing: the names part 1 logged, and the names its table expects, contain REQUIRED.

Comparison: util.ref_conv_with_mag + util.assert_conv_close with util.CONV_A / CONV_R, inputs from test_convs_at_scale._conv_inputs,
statistics by test_ops_at_scale._assert_stats, the InstanceNorm-backward sums by the bounds of test_ops_at_scale._inbwd_case (_inbwd_row
below says where it differs), accumulated slots pre-filled -- the runners of test_convs_at_scale.py; no tolerance of this module's own.

What the table cannot have, and why:
* 128x160:w4 (the conv1 || conv4 pair forward) always asks for statistics: it has edges (a) and (b) only.
* 128x128:w4:ksN: split-K launches never tile per sample (run_mfma: per_sample needs ksplit == 1); their statistics and
  InstanceNorm-backward sums come from the finish pass, so edge (b) is "N >= 2, ragged V, statistics from the finish pass" and
  plan_of says per_sample = False.
"""
import math
import re
import zlib

import pytest
import torch

import util
from util import ops, assert_close_ew, assert_conv_close, ref_conv_with_mag
from test_ops_at_scale import _ab, _as, _gen, _ramp, _randn, _assert_stats, _assert_sum
from test_convs_at_scale import (C3_CONV_KEYS, EXTRA_CONV_KEYS, _DT, _conv_inputs, _fwd_key, _no_wgrad, _parse, _split)


# =================================================================================================================================
# part 0: the mirror of the plan
# =================================================================================================================================
SWITCH_DEFAULTS = {"M1_PLAN128": 768, "M1_CONV8": 1, "M1_F32_W8": 3, "M1_MFMA_TPS": 1, "M1_MFMA_KG": 1, "M1_BN160": 1}


def _cdiv(a, b):
    return -(-a // b)


def _min_class_chunks(members, k, classes, seg):
    """Smallest K-chunk count over the parity classes (min_class_chunks / build_classes): a class of parity p keeps, per axis, the taps a
    with (p + pad - a) % stride == 0; the padding only shifts which parity gets which count."""
    taps = 1
    for kk, st in zip(k, classes):
        taps *= min(len([a for a in range(kk) if (p - a) % st == 0]) for p in range(st))
    return _cdiv(taps * sum(_cdiv(c, seg) for c in members), 4)


def plan_of(N, odims, members, cout, k, classes, dtype, switches=None, fused=False, pair=False):
    """(BM, BN, waves, ksplit, kgroups, KC, aligned, per_sample) of one conv_mfma launch, from conv_mfma.hip make_plan, run_mfma and
    launch_cfg.  ``odims``: the launch's output dims; ``members``: channels of the contraction's concat members; ``cout``: its output
    columns; ``classes``: the strides whose parities make the classes of a strided data gradient / transposed forward ((1, 1, 1): one
    class, rows = N * V; else rows = N * prod(ceil(odims / classes)) per class); ``fused``: statistics or InstanceNorm-backward sums
    are asked of the epilogue; ``pair``: the conv1 || conv4 forward.  BM is the tile the launch runs (128 on the 8-wave form)."""
    sw = dict(SWITCH_DEFAULTS)
    sw.update(switches or {})
    bf16 = dtype in ("bf16", torch.bfloat16)
    seg = 8 if bf16 else 4
    ncls = classes[0] * classes[1] * classes[2]
    V = odims[0] * odims[1] * odims[2]
    maxM = N * V if ncls == 1 else N * math.prod(_cdiv(o, s) for o, s in zip(odims, classes))
    nch = _min_class_chunks(members, k, classes, seg)
    bn160 = bool(pair and bf16 and sw["M1_BN160"] and cout % 160 == 0 and cout <= 320)
    BN = 160 if bn160 else (128 if cout > 64 else 64 if cout > 32 else 32 if cout > 16 else 16)
    ntile = _cdiv(cout, BN)
    b128 = _cdiv(maxM, 128) * ncls * ntile
    BM = 128 if (bn160 or b128 >= 256) else 64
    blocks = _cdiv(maxM, BM) * ncls * ntile
    ks, t128 = 1, sw["M1_PLAN128"]
    if t128 > 0 and BN == 128 and 100 <= b128 < t128 and nch >= 200:
        BM, ks = 128, max(1, min(_cdiv(t128, b128), nch // 64))
    elif blocks < 256 and nch >= 16:
        ks = min(max(1, min(_cdiv(512, blocks), nch // 8)), 32)
    aligned = all(c % (4 * seg) == 0 for c in members)
    kg = 1
    if bf16 and BM == 64 and BN in (64, 128) and ks >= 2 and sw["M1_MFMA_KG"]:
        kmax = min((150 * 1024) // (2 * 2 * (64 + BN) * 64), 1024 // 256, 4)
        if aligned and kmax >= 2 and ks <= 4 and _cdiv(maxM, 64) * ncls * ntile >= 200:
            kg, ks = min(ks, kmax), 1
    c8 = sw["M1_CONV8"]
    use8 = bool(kg == 1 and c8 and BN == 128 and (ks == 1 or (c8 >= 2 and BM == 128)) and _cdiv(maxM, 128) * ncls * ntile * ks >= 160)
    if BN == 128:
        bm_eff, waves = (128, 8) if use8 else (BM, 4)
    elif BN in (64, 32):
        bm_eff, waves = BM, 8 if (BM == 128 and sw["M1_F32_W8"] & (2 if bf16 else 1)) else 4
    else:
        bm_eff, waves = BM, 4
    per_sample = bool(N > 1 and V % bm_eff != 0 and ncls == 1 and ks == 1 and sw["M1_MFMA_TPS"] and fused)
    KC = 2 if (kg > 1 or nch // ks >= 6) else 1
    return bm_eff, BN, waves, ks, kg, KC, aligned, per_sample


def plan_name(p):
    return f"conv_mfma:{p[0]}x{p[1]}:w{p[2]}:ks{p[3]}" + (f":kg{p[4]}" if p[4] > 1 else "")


def launch_of(key):
    """plan_of's arguments for the single conv_mfma launch behind a conv key (test_convs_at_scale.conv_key): what dispatch.hip's
    fwd_spec / dgrad_spec / dgrad_fused_spec / pair_*_spec hand to run_mfma."""
    name, N, D, H, W, cins, cout, k, s, dts, fl = key[:11]
    dims, one = (D, H, W), (1, 1, 1)
    down = tuple(_cdiv(n, st) for n, st in zip(dims, s))
    if name == "m1_conv3d_fwd":
        return dict(N=N, odims=down, members=cins, cout=cout, k=k, classes=one, dtype=dts, fused="stats=1" in fl)
    if name == "m1_conv3d_pair_fwd":
        return dict(N=N, odims=down, members=cins, cout=sum(cout), k=k, classes=one, dtype=dts, fused=True, pair=True)
    if name == "m1_convT3d_fwd":
        return dict(N=N, odims=tuple(n * st for n, st in zip(dims, s)), members=cins, cout=cout, k=k, classes=s, dtype=dts)
    if name in ("m1_conv3d_dgrad", "m1_conv3d_dgrad_inbwd"):            # (one launch: one member, or all of them as one problem)
        return dict(N=N, odims=dims, members=(cout,), cout=sum(cins), k=k, classes=s, dtype=dts, fused=name.endswith("inbwd"))
    if name == "m1_conv3d_pair_dgrad":
        return dict(N=N, odims=dims, members=tuple(cout), cout=sum(cins), k=k, classes=s, dtype=dts)
    assert name == "m1_convT3d_dgrad", name                             # a strided forward conv of dy on the low-resolution grid
    return dict(N=N, odims=dims, members=(cout,), cout=sum(cins), k=k, classes=one, dtype=dts)


def _single_mfma_keys():
    return [q for q in C3_CONV_KEYS + EXTRA_CONV_KEYS if q[-1].startswith("conv_mfma:") and "+" not in q[-1]]


def test_plan_mirror_reproduces_the_pinned_bench_names():
    """Every single-launch conv_mfma key of the two bench tables, parity-class keys included (the class count is the product of the
    key's strides): none is left out."""
    keys = _single_mfma_keys()
    assert len(keys) >= 50, len(keys)
    wrong = [(q, plan_name(plan_of(**launch_of(q)))) for q in keys if plan_name(plan_of(**launch_of(q))) != q[-1]]
    assert not wrong, wrong
    for want in ("64x128:w4:ks13", "64x64:w4:ks1:kg3", "128x160:w4:ks3", "128x16:w4:ks1", "128x64:w8:ks1"):
        assert any(q[-1] == "conv_mfma:" + want for q in keys), want


# =================================================================================================================================
# the table
# =================================================================================================================================
def _fwd(N, dims, cins, cout, k, dt, stats, kern, plan, edge, s=(1, 1, 1), sw=None):
    return (("m1_conv3d_fwd", N, *dims, tuple(cins), cout, k, s, dt, f"stats={int(stats)}", "conv_mfma:" + kern), sw or {}, plan, edge)


def _dg(N, dims, cins, cout, k, dt, acc, kern, plan, edge, s=(1, 1, 1), sw=None):
    fl = f"need={tuple(1 for _ in cins)},acc={tuple(acc)}"
    return (("m1_conv3d_dgrad", N, *dims, tuple(cins), cout, k, s, dt, fl, "conv_mfma:" + kern), sw or {}, plan, edge)


def _ib(N, dims, c, cout, k, dt, kern, plan, edge, sw=None):
    return (("m1_conv3d_dgrad_inbwd", N, *dims, (c,), cout, k, (1, 1, 1), dt, "fused=1", "conv_mfma:" + kern), sw or {}, plan, edge)


def _tf(N, dims, cins, cout, k, s, dt, kern, plan, edge, sw=None):
    return (("m1_convT3d_fwd", N, *dims, tuple(cins), cout, k, s, dt, "", "conv_mfma:" + kern), sw or {}, plan, edge)


def _pf(N, dims, cins, c1, c4, k, kern, plan, edge, s=(1, 1, 1), sw=None):
    return (("m1_conv3d_pair_fwd", N, *dims, tuple(cins), (c1, c4), k, s, "bf16", "stats=1", "conv_mfma:" + kern), sw or {}, plan, edge)


K333, K133, K111 = (3, 3, 3), (1, 3, 3), (1, 1, 1)
# volumes (input dims of the conv).  V = D*H*W per sample, M = N*V rows:
A1, A2 = (1, (6, 52, 53)), (2, (3, 52, 53))        # M = 16,536: 130 row tiles (x 2 column tiles = 260); M % 128 = 24, V % 128 = 76
B1, B2 = (1, (6, 75, 77)), (2, (3, 75, 77))        # M = 34,650: 271 row tiles; M % 128 = 90, V % 128 = 45
D1, D3 = (1, (6, 75, 75)), (3, (2, 75, 75))        # M = 33,750: 264 row tiles; M % 128 = 86, V % 128 = 114
E1, E2 = (1, (4, 58, 57)), (2, (2, 58, 57))        # M = 13,224: 104 row tiles (the split-K window 100..767); M % 128 = 40, V % 128 = 84
G2 = (2, (4, 37, 45))                              # M = 13,320: 209 64-row tiles; V % 64 = 4
H2 = (2, (3, 19, 21))                              # M = 2,394: 38 64-row tiles; V % 64 = 45


def _rows_for(dt):
    """Part 1 for one type.  plan = (KC, aligned, per_sample) as plan_of states them (the kernel log cannot)."""
    bf = dt == "bf16"
    ksE = 3 if bf else 6                            # [256] x 27 taps: 216 bf16 / 432 fp32 chunks; split = min(ceil(768 / 104), chunks / 64)
    ksH = 13 if bf else 14                          # [128] x 27 taps: 108 / 216 chunks; split = min(ceil(512 / 38), chunks / 8)
    al16 = not bf                                   # a 16-channel member is whole 64-byte chunks in fp32 only
    r = [
        # ---- 128x128 on 8 waves: [32] -> 256, 27 taps
        _fwd(*A1, [32], 256, K333, dt, 0, "128x128:w8:ks1", (2, True, False), "a"),
        _fwd(*A2, [32], 256, K333, dt, 1, "128x128:w8:ks1", (2, True, True), "b"),
        _fwd(*A2, [32], 256, K333, dt, 0, "128x128:w8:ks1", (2, True, False), "c"),
        _fwd(*A2, [20], 136, K133, dt, 1, "128x128:w8:ks1", (2, False, True), "b, unaligned member, Cout % column tile != 0"),
        # ---- 128x64 on 8 waves: [16] -> 64, 27 taps
        _fwd(*B1, [16], 64, K333, dt, 0, "128x64:w8:ks1", (2, al16, False), "a"),
        _fwd(*B2, [16], 64, K333, dt, 1, "128x64:w8:ks1", (2, al16, True), "b"),
        _fwd(*B2, [16], 64, K333, dt, 0, "128x64:w8:ks1", (2, al16, False), "c"),
        # ---- 128x32 on 8 waves: [24] -> 32 and the aligned concat [32, 32] -> 24, 9 taps
        _fwd(*B1, [24], 32, K133, dt, 0, "128x32:w8:ks1", (2, False, False), "a, unaligned member"),
        _fwd(*B2, [24], 32, K133, dt, 1, "128x32:w8:ks1", (2, False, True), "b, unaligned member"),
        _fwd(*B2, [24], 32, K133, dt, 0, "128x32:w8:ks1", (2, False, False), "c, unaligned member"),
        _fwd(*B2, [32, 32], 24, K133, dt, 1, "128x32:w8:ks1", (2, True, True), "b, aligned concat, Cout % column tile != 0"),
        # ---- 128x16: [40] -> 6, one tap (V % 32 != 0 keeps conv_pw away): KC = 1, Cout * element size % 16 != 0
        _fwd(*D1, [40], 6, K111, dt, 0, "128x16:w4:ks1", (1, False, False), "a, KC 1, Cout not 16 bytes"),
        _fwd(*D3, [40], 6, K111, dt, 1, "128x16:w4:ks1", (1, False, True), "b, KC 1, Cout not 16 bytes"),
        _fwd(*D3, [40], 6, K111, dt, 0, "128x16:w4:ks1", (1, False, False), "c, KC 1, Cout not 16 bytes"),
        # ---- slab split-K on 128x128 tiles (M1_PLAN128): [256] -> 128, 27 taps (W = 57 keeps conv_t3 away)
        _fwd(*E1, [256], 128, K333, dt, 0, f"128x128:w4:ks{ksE}", (2, True, False), "a, split-K"),
        _fwd(*E2, [256], 128, K333, dt, 1, f"128x128:w4:ks{ksE}", (2, True, False), "b, split-K, finish pass with statistics"),
        _fwd(*E2, [256], 128, K333, dt, 0, f"128x128:w4:ks{ksE}", (2, True, False), "c, split-K, plain finish pass"),
        _ib(*E2, 128, 256, K333, dt, f"128x128:w4:ks{ksE}", (2, True, False), "b, split-K, finish pass with the IN-backward sums"),
        # ---- roles on 128-row tiles.  Data gradients also check dW and db of the same backward call.
        _dg(*A2, [256], 32, K333, dt, (0,), "128x128:w8:ks1", (2, True, False), "c, stride-1 data gradient"),
        _dg(*A2, [256], 32, K333, dt, (1,), "128x128:w8:ks1", (2, True, False), "c, stride-1 data gradient, accumulate"),
        _dg(*A2, [128, 128], 32, K333, dt, (1, 0), "128x128:w8:ks1", (2, True, False), "c, data gradient of two members in one launch"),
        _dg(*B2, [64], 32, K333, dt, (0,), "128x64:w8:ks1", (1 if bf else 2, True, False), "4 parity classes, rows % 128 = 60", s=(1, 2, 2)),
        _dg(*B2, [64], 32, K333, dt, (1,), "128x64:w8:ks1", (1 if bf else 2, True, False), "4 parity classes, rows % 128 = 60, accumulate",
            s=(1, 2, 2)),
        _dg(2, (6, 52, 53), [128], 32, K333, dt, (0,), "128x128:w8:ks1", (1, True, False), "8 parity classes, rows % 128 = 116", s=(2, 2, 2)),
        _tf(2, (3, 38, 39), [64], 32, K333, (1, 2, 2), dt, "128x32:w8:ks1", (2, True, False), "transposed forward, 4 classes, rows % 128 = 60"),
        _ib(*A2, 256, 32, K333, dt, "128x128:w8:ks1", (2, True, True), "b, IN-backward sums from the epilogue"),
        _ib(*B2, 32, 32, K333, dt, "128x32:w8:ks1", (2, True, True), "b, IN-backward sums from the epilogue"),
        # ---- 64-row split-K at a ragged V: statistics / IN-backward sums from the finish pass
        _fwd(*H2, [128], 128, K333, dt, 1, f"64x128:w4:ks{ksH}", (2, True, False), "64-row split-K, finish pass with statistics"),
        _ib(*H2, 128, 128, K333, dt, f"64x128:w4:ks{ksH}", (2, True, False), "64-row split-K, finish pass with the IN-backward sums"),
    ]
    if bf:
        r += [
            # ---- 128x160: the conv1 || conv4 pair forward, [64] -> 32 + 128 (statistics always)
            _pf(*B1, [64], 32, 128, K333, "128x160:w4:ks1", (2, True, False), "a"),
            _pf(*B2, [64], 32, 128, K333, "128x160:w4:ks1", (2, True, True), "b"),
            _pf(*E2, [64], 32, 128, K333, "128x160:w4:ks5", (2, True, False), "split-K, finish pass with two statistics"),
            # ---- K groups inside the block, 64-row tiles, V % 64 = 4
            _fwd(*G2, [64], 64, K333, dt, 1, "64x64:w4:ks1:kg3", (2, True, True), "K groups, ragged V, per-sample tiling"),
            _fwd(*G2, [64], 128, K333, dt, 1, "64x128:w4:ks1:kg3", (2, True, True), "K groups, ragged V, per-sample tiling"),
            _fwd(*G2, [64], 128, K333, dt, 0, "64x128:w4:ks1:kg3", (2, True, False), "K groups, tiles straddle the samples"),
        ]
    return r


ROWS = _rows_for("bf16") + _rows_for("fp32")


def _with(row, sw, kern, plan=None, edge=None):
    key, _, pl, ed = row
    return ((*key[:-1], "conv_mfma:" + kern), dict(sw), plan or pl, edge or ed)


def _find(dt, name, vol, cins, cout, fl):
    hit = [r for r in ROWS if r[0][0] == name and r[0][1:5] == (vol[0], *vol[1]) and r[0][5] == tuple(cins) and r[0][6] == cout and
           r[0][9] == dt and r[0][10] == fl and r[0][8] == (1, 1, 1)]
    assert len(hit) == 1, (dt, name, vol, cins, cout, fl, len(hit))
    return hit[0]


def _switch_rows():
    F = "m1_conv3d_fwd"
    a2 = {dt: _find(dt, F, A2, [32], 256, "stats=1") for dt in _DT}
    a1 = {dt: _find(dt, F, A1, [32], 256, "stats=0") for dt in _DT}
    b2 = {dt: _find(dt, F, B2, [16], 64, "stats=1") for dt in _DT}
    c2 = {dt: _find(dt, F, B2, [24], 32, "stats=1") for dt in _DT}
    cc = {dt: _find(dt, F, B2, [32, 32], 24, "stats=1") for dt in _DT}
    e1 = {dt: _find(dt, F, E1, [256], 128, "stats=0") for dt in _DT}
    e2 = {dt: _find(dt, F, E2, [256], 128, "stats=1") for dt in _DT}
    h2 = {dt: _find(dt, F, H2, [128], 128, "stats=1") for dt in _DT}
    return [
        # M1_CONV8=0: the 4-wave 128x128 tile where the 8-wave one ran; =2: 8 waves on the split-K shape as well
        _with(a2["bf16"], {"M1_CONV8": 0}, "128x128:w4:ks1"),
        _with(a1["fp32"], {"M1_CONV8": 0}, "128x128:w4:ks1"),
        _with(e2["bf16"], {"M1_CONV8": 2}, "128x128:w8:ks3"),
        _with(e1["fp32"], {"M1_CONV8": 2}, "128x128:w8:ks6"),
        # M1_F32_W8=0: 4 waves on the 64- and 32-column tiles
        _with(b2["bf16"], {"M1_F32_W8": 0}, "128x64:w4:ks1"),
        _with(b2["fp32"], {"M1_F32_W8": 0}, "128x64:w4:ks1"),
        _with(c2["bf16"], {"M1_F32_W8": 0}, "128x32:w4:ks1"),
        _with(c2["fp32"], {"M1_F32_W8": 0}, "128x32:w4:ks1"),
        # M1_PLAN128=0 on the split-K shape: 64-row tiles (207 of them), split 3 -- as K groups in bf16, as slabs in fp32
        _with(e2["bf16"], {"M1_PLAN128": 0}, "64x128:w4:ks1:kg3", plan=(2, True, True)),
        _with(e2["fp32"], {"M1_PLAN128": 0}, "64x128:w4:ks3"),
        # M1_MFMA_TPS=0 on edge (b): tiles straddle the samples, statistics from the stand-alone pass
        _with(a2["bf16"], {"M1_MFMA_TPS": 0}, "128x128:w8:ks1", plan=(2, True, False)),
        _with(c2["fp32"], {"M1_MFMA_TPS": 0}, "128x32:w8:ks1", plan=(2, False, False)),
        # M1_KORDER=0 / 1 on aligned multi-tap shapes: [tap][channel] panels / single chunks instead of pairs
        _with(e2["bf16"], {"M1_KORDER": 0}, "128x128:w4:ks3"),
        _with(e2["bf16"], {"M1_KORDER": 1}, "128x128:w4:ks3"),
        _with(cc["fp32"], {"M1_KORDER": 0}, "128x32:w8:ks1"),
        _with(cc["fp32"], {"M1_KORDER": 1}, "128x32:w8:ks1"),
        # M1_FINISH_STATS=0 on split-K rows with statistics: splitk_finish_kernel, then the stand-alone statistics
        _with(e2["bf16"], {"M1_FINISH_STATS": 0}, "128x128:w4:ks3"),
        _with(e2["fp32"], {"M1_FINISH_STATS": 0}, "128x128:w4:ks6"),
        _with(h2["bf16"], {"M1_FINISH_STATS": 0}, "64x128:w4:ks13"),
    ]


SWITCH_ROWS = _switch_rows()

# the variants part 1 must reach, per type (regular expressions over "conv_mfma:" names)
REQUIRED = {
    "bf16": [r"128x16:w4:ks1$", r"128x32:w8:ks1$", r"128x64:w8:ks1$", r"128x128:w8:ks1$", r"128x128:w4:ks([2-9]|\d\d)$", r"128x160:w4:ks\d+$",
             r"64x64:w4:ks1:kg[234]$", r"64x128:w4:ks1:kg[234]$"],
    "fp32": [r"128x16:w4:ks1$", r"128x32:w8:ks1$", r"128x64:w8:ks1$", r"128x128:w8:ks1$", r"128x128:w4:ks([2-9]|\d\d)$"],
}
# the 128-row variants that need edges (a), (b) and (c) each (the pair forward: (a) and (b), see the module docstring)
EDGED = {"bf16": ["128x16:w4", "128x32:w8", "128x64:w8", "128x128:w8", "128x128:w4", "128x160:w4"],
         "fp32": ["128x16:w4", "128x32:w8", "128x64:w8", "128x128:w8", "128x128:w4"]}


def _missing(names_by_type):
    return [(dt, pat) for dt, pats in REQUIRED.items() for pat in pats
            if not any(re.search("^conv_mfma:" + pat, n) for n in names_by_type.get(dt, ()))]


def _edge(row):
    e = row[3].split(",")[0]
    return e if e in ("a", "b", "c") else None


def _row_id(row):
    key, sw = row[0], row[1]
    return "-".join(str(v) for v in key).replace(" ", "") + "".join(f"-{k}={v}" for k, v in sw.items())


def test_table_names_and_fields_are_what_the_mirror_says():
    """Every row's expected kernel and its (KC, aligned, per_sample) equal plan_of under the row's switches; the table stays small."""
    assert len(ROWS) + len(SWITCH_ROWS) <= 90, (len(ROWS), len(SWITCH_ROWS))
    assert len({_row_id(r) for r in ROWS + SWITCH_ROWS}) == len(ROWS) + len(SWITCH_ROWS)
    for key, sw, plan, edge in ROWS + SWITCH_ROWS:
        p = plan_of(switches={k: v for k, v in sw.items() if k in SWITCH_DEFAULTS}, **launch_of(key))
        assert plan_name(p) == key[-1], (key, sw, p)
        assert (p[5], p[6], p[7]) == plan, (key, sw, p, plan)
        V = key[2] * key[3] * key[4]
        assert key[1] * V <= 36000                                     # "a few tens of thousands of voxels"


def test_table_covers_the_required_variants_edges_and_roles():
    names = {dt: {r[0][-1] for r in ROWS if r[0][9] == dt} for dt in _DT}
    assert not _missing(names), _missing(names)
    for dt, variants in EDGED.items():
        for v in variants:
            rows = [r for r in ROWS if r[0][9] == dt and r[0][-1].startswith("conv_mfma:" + v + ":") and r[0][8] == (1, 1, 1)]
            edges = {_edge(r) for r in rows} - {None}
            assert edges >= ({"a", "b"} if v == "128x160:w4" else {"a", "b", "c"}), (dt, v, edges)
            for key, sw, plan, edge in rows:
                N, V, e = key[1], key[2] * key[3] * key[4], _edge((key, sw, plan, edge))
                if e == "a":
                    assert N == 1 and V % 128 != 0, key
                elif e in ("b", "c"):
                    fused = key[10] in ("stats=1", "fused=1")
                    assert N >= 2 and V % 128 != 0 and fused == (e == "b"), key
                    if e == "b" and ":ks1" in key[-1]:
                        assert plan[2], key                            # plan_of: per-sample tiling
        big = [r for r in ROWS if r[0][9] == dt and r[0][-1].startswith("conv_mfma:128x")]
        esz = 2 if dt == "bf16" else 4
        chunk = 64 // esz
        assert {r[2][0] for r in big} == {1, 2}, dt                                       # KC 1 and KC 2
        assert any(r[0][6] * esz % 16 for r in big if r[0][0] == "m1_conv3d_fwd"), dt     # Cout not 16 bytes' worth
        assert any(r[0][6] % int(r[0][-1].split(":")[1].split("x")[1]) for r in big if r[0][0] == "m1_conv3d_fwd"), dt
        assert any(not r[2][1] for r in big) and any(r[2][1] and len(r[0][5]) > 1 and r[0][0] == "m1_conv3d_fwd" and
                                                     all(c % chunk == 0 for c in r[0][5]) for r in big), dt
        roles = {(r[0][0], r[0][8], r[0][10].split("acc=")[-1]) for r in big}
        for want in (("m1_conv3d_dgrad", (1, 1, 1), "(0,)"), ("m1_conv3d_dgrad", (1, 1, 1), "(1,)"), ("m1_conv3d_dgrad", (1, 2, 2), "(0,)"),
                     ("m1_conv3d_dgrad", (2, 2, 2), "(0,)"), ("m1_convT3d_fwd", (1, 2, 2), ""), ("m1_conv3d_dgrad_inbwd", (1, 1, 1), "fused=1")):
            assert want in roles, (dt, want)
        assert any(r[0][0] == "m1_conv3d_dgrad_inbwd" and r[0][1] >= 2 and ":ks1" not in r[0][-1] for r in ROWS if r[0][9] == dt), dt
    sw = {k for r in SWITCH_ROWS for k in r[1].items()}
    for want in (("M1_CONV8", 0), ("M1_CONV8", 2), ("M1_F32_W8", 0), ("M1_PLAN128", 0), ("M1_MFMA_TPS", 0), ("M1_KORDER", 0), ("M1_KORDER", 1),
                 ("M1_FINISH_STATS", 0)):
        assert want in sw, want


# ---- sensitivity of the two bounds to the faults these shapes exist for, on the reference alone ----
@pytest.fixture(scope="module")
def straddling_reference():
    """The fp64 result of the 128x32 row of edge (c), N = 2, V = 17,325 = 135 * 128 + 45, computed once on the CPU."""
    cpu = torch.device("cpu")
    N, dims, cins, cout, k, s = 2, (3, 75, 77), [24], 32, K133, (1, 1, 1)
    xs, w, b, _ = _conv_inputs(cpu, torch.bfloat16, N, dims, cins, cout, k, s, False, _gen(cpu, 11))
    ref, mag = ref_conv_with_mag(xs[0], w, b, s)
    return ref["y"], mag["y"]


def _straddle(V):
    """Rows of the tile that holds the sample border: (its rows in sample 0, its rows in sample 1)."""
    t0 = V // 128 * 128
    assert 0 < V - t0 < 128
    return V - t0, t0 + 128 - V


def test_bound_rejects_a_straddling_tile_read_from_the_wrong_sample(straddling_reference):
    y, mag = straddling_reference
    N, D, H, W, C = y.shape
    V = D * H * W
    n0, n1 = _straddle(V)
    assert (n0, n1) == (45, 83)
    assert_conv_close(y.to(torch.bfloat16), y, mag, torch.bfloat16, "undamaged y")
    assert_conv_close(y.float(), y, mag, torch.float32, "undamaged y, fp32")
    bad = y.clone().reshape(N, V, C)
    bad[1, :n1] = y.reshape(N, V, C)[0, :n1]                 # the tile took its sample index from its first row
    bad = bad.reshape(y.shape)
    for dt in (torch.bfloat16, torch.float32):
        with pytest.raises(AssertionError, match="elements outside"):
            assert_conv_close(bad.to(dt), y, mag, dt, "straddling tile from sample 0")
    out = (bad.to(torch.bfloat16).double() - y).abs() > util.CONV_A[torch.bfloat16] * y.abs() + util.CONV_R * mag
    assert float(out.reshape(N, V, C)[1, :n1].double().mean()) > 0.9          # nearly every element of the damaged rows


def test_statistics_bound_rejects_a_straddling_tile_credited_to_the_other_sample(straddling_reference):
    y = straddling_reference[0].to(torch.bfloat16).float()   # what a kernel stores
    N, D, H, W, C = y.shape
    V = D * H * W
    n0, n1 = _straddle(V)
    good = util.ref_in_stats(y.double())
    _assert_stats(good.float(), y, "undamaged statistics")
    flat = y.double().reshape(N, V, C)
    s1, s2 = flat.sum(1), flat.square().sum(1)
    t1, t2 = flat[1, :n1].sum(0), flat[1, :n1].square().sum(0)
    s1[0] += t1; s2[0] += t2; s1[1] -= t1; s2[1] -= t2       # the 83 rows of sample 1 in the shared tile counted for sample 0
    mean = s1 / V
    var = (s2 / V - mean * mean).clamp_min(0)
    bad = torch.stack([mean, 1.0 / torch.sqrt(var + 1e-3)], -1)
    assert bad.shape == good.shape
    with pytest.raises(AssertionError, match="sums off"):
        _assert_stats(bad.float(), y, "credited to sample 0")


# =================================================================================================================================
# parts 1 and 2: the rows on the GPU
# =================================================================================================================================
_SEEN = {"bf16": set(), "fp32": set()}       # conv_mfma names part 1 logged, per type
_RAN = set()


def _dgrad_row(dev, key):
    """test_convs_at_scale._dgrad_key with the weight and bias gradients of the same backward call checked as well."""
    name, N, D, H, W, cins, cout, k, s, dts, fl, kern = key
    dtype = _DT[dts]
    need, acc = _parse(fl, "need"), _parse(fl, "acc")
    g = _gen(dev, zlib.crc32(repr(key).encode()) % 10007)
    xs, w, b, dy = _conv_inputs(dev, dtype, N, (D, H, W), cins, cout, k, s, False, g)
    xd, pre = [], []
    for x, nd, ac in zip(xs, need, acc):
        t = x.to(dtype).requires_grad_(bool(nd))
        pre.append(None)
        if ac:                                              # a fan-out slot that already holds another consumer's gradient
            slot = ops._GradSlot()
            pre[-1] = _as(_randn(tuple(x.shape), g, dev) - 0.4, dtype).to(dtype)
            slot.buf, slot.tail_init = pre[-1].clone(), True
            t._m1_gslot = slot
        xd.append(t)
    wd, bd = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = ops.conv3d_same(xd, wd, bd, k, s)
    with ops.kernel_log() as kl:
        y.backward(dy.to(dtype))
        ops.fold_pending()
        ops.join_side_streams()
        torch.cuda.synchronize()
    assert _no_wgrad(kl.names) == kern.split("+"), (kl.names, kern)
    ref, mag = ref_conv_with_mag(torch.cat(xs, -1), w, b, s, dy)
    for i, (t, r_, m_) in enumerate(zip(xd, _split(ref["dx"], cins), _split(mag["dx"], cins))):
        if acc[i]:
            got = t._m1_gslot.buf
            assert got.data_ptr() != pre[i].data_ptr()
            assert_conv_close(got, pre[i].double() + r_, m_ + pre[i].double().abs(), dtype, f"dx[{i}] (accumulated) of {key}",
                              amag=r_.abs() if dtype == torch.bfloat16 else None, acc=dtype != torch.bfloat16)
        else:
            assert_conv_close(t.grad, r_, m_, dtype, f"dx[{i}] of {key}")
    assert_conv_close(wd.grad, ref["dw"], mag["dw"], torch.float32, f"dW of {key}")
    assert_conv_close(bd.grad, ref["db"], mag["db"], torch.float32, f"db of {key}")
    return kl.names


def _inbwd_row(dev, key):
    """y = conv(lrelu(IN(x))), the data gradient through m1_conv3d_dgrad_inbwd: test_ops_at_scale._inbwd_case with its references and
    bounds for d(a) (util.assert_conv_close against fp64) and for the sums dgamma / dbeta (_assert_sum against fp64), fused and
    stand-alone.  One difference, in the check of the norm's dx: _inbwd_case derives it from the fp64 d(a) rounded once to the
    activation type, which for fp32 leaves no room for the conv's own accumulation error (its fp32 cases are 1x1x1 convs over <= 32
    channels; here K is up to 6,912, and sqrt(K) * 2^-24 of d(a) reaches dx through rstd * gamma, past 4e-6 of rms on a handful of
    elements in a million).  d(a) has its own per-element check, so dx is compared with the fp64 InstanceNorm backward OF THE d(a) THE
    CONV STORED (the hook's tensor) under _inbwd_case's unchanged constants: what is left is the error of the norm's backward and of the
    sums it reads -- the sums are what a tile credited to the wrong sample would spoil.  The closed form is checked against autograd."""
    name, N, D, H, W, cins, cout, k, s, dts, fl, kern = key
    dtype, dims, c = _DT[dts], (N, D, H, W), cins[0]
    g = _gen(dev, zlib.crc32(repr(key).encode()) % 10007)
    shape = (*dims, c)
    K = c * k[0] * k[1] * k[2]
    x = _as(_randn(shape, g, dev, 1.7) + 0.8 + _ramp(shape, dev) + 0.2 * _randn((1, 1, 1, 1, c), g, dev), dtype)
    gam, bet = 1 + 0.2 * _randn((c,), g, dev), 0.3 + 0.2 * _randn((c,), g, dev)
    w = _as(_randn((*k, c, cout), g, dev, 1.0 / K ** 0.5), dtype)
    bc = 0.1 * _randn((cout,), g, dev)
    xr, gr, br = (t.double().requires_grad_(True) for t in (x, gam, bet))
    a_ = util.round_grad(util.ref_instnorm_act(xr, gr, br, 0.1), dtype)
    yr = util.ref_conv3d_same(a_, w.double(), bc.double(), (1, 1, 1))
    dy = _as(yr.detach().float() + 0.5 * _randn(tuple(yr.shape), g, dev), dtype)
    yr.backward(dy.double())
    rf, mg_ = ref_conv_with_mag(torch.zeros_like(x), w, None, (1, 1, 1), dy)
    da64, mda = rf["dx"], mg_["dx"]
    del rf, mg_
    with torch.no_grad():
        st = util.ref_in_stats(x.double())
        rstd = st[:, None, None, None, :, 1]
        xhat = (x.double() - st[:, None, None, None, :, 0]) * rstd
        z = xhat * gam.double() + bet.double()
        slope = torch.where(z >= 0, 1.0, 0.1)
        tie = z.abs() <= 1e-5 * z.square().mean().sqrt()       # (the LeakyReLU's branch within fp32 error of 0: both branches right)

        def in_backward(da):
            dzh = da * slope * gam.double()
            m1, m2 = dzh.mean(dim=(1, 2, 3), keepdim=True), (dzh * xhat).mean(dim=(1, 2, 3), keepdim=True)
            return rstd * (dzh - m1 - xhat * m2)
        da = da64.to(dtype).double()
        dz = da * slope
        mg, mb = (dz * xhat).abs().sum(dim=(0, 1, 2, 3)), dz.abs().sum(dim=(0, 1, 2, 3))
    x2 = x.double().requires_grad_(True)                       # the closed form against autograd, on the same upstream gradient
    util.ref_instnorm_act(x2, gam.double(), bet.double(), 0.1).backward(da)
    assert float((in_backward(da) - x2.grad).abs().max()) <= 1e-7 * float(x2.grad.abs().max())     # (a wrong formula is off by O(1))
    del x2

    def run(on):
        was = ops._INBWD["on"]; ops._INBWD["on"] = on
        try:
            xd = x.to(dtype).clone().requires_grad_(True)
            ps = [t.clone().requires_grad_(True) for t in (gam, bet, w, bc)]
            a = ops.instnorm_act(xd, ps[0], ps[1], 0.1, ops.instnorm_stats(xd))
            y = ops.conv3d_same([a], ps[2], ps[3], k, (1, 1, 1))
            seen = []
            a.register_hook(lambda g_: seen.append(g_.detach().clone()))
            with ops.kernel_log() as kl:
                y.backward(dy.to(dtype))
                torch.cuda.synchronize()
            assert len(seen) == 1
            if on:
                assert _no_wgrad(kl.names) == kern.split("+"), (kl.names, kern)
            assert_conv_close(seen[0], da64, mda, dtype, f"d(a) of the conv, fused={on}, of {key}")
            return xd.grad, ps[0].grad, ps[1].grad, seen[0]
        finally:
            ops._INBWD["on"] = was
    f0 = dict(ops._INBWD)
    got = run(True)
    fused = ops._INBWD["fused"] - f0["fused"], ops._INBWD["plain"] - f0["plain"]
    assert fused == (1, 0), fused                               # the epilogue (or the finish pass) did emit the sums
    base = run(False)
    a, b = _ab(dtype)
    for tag, (dx, dgm, dbt, da_k) in (("fused", got), ("plain", base)):
        what = f"IN bwd ({tag}) of {key}"
        with torch.no_grad():
            ref_dx = in_backward(da_k.double())
            mdx = ref_dx.abs() + (da_k.double() * slope * rstd * gam.double()).abs() if dtype == torch.bfloat16 else None
        assert_close_ew(torch.where(tie, 0.0, dx.double()), torch.where(tie, 0.0, ref_dx), a, b,
                        mag=None if mdx is None else torch.where(tie, 0.0, mdx), what=what + " dx")
        _assert_sum(dgm, gr.grad, mg, what + " dgamma")
        _assert_sum(dbt, br.grad, mb, what + " dbeta")


def _run_row(dev, row):
    key, sw = row[0], row[1]
    try:
        with ops.config(M1_T3_MIN_BLOCKS=128, **sw):          # (the production floor; nothing else unless the row says so)
            if key[0] == "m1_conv3d_dgrad":
                _dgrad_row(dev, key)
            elif key[0] == "m1_conv3d_dgrad_inbwd":
                _inbwd_row(dev, key)
            else:
                _fwd_key(dev, key)
    finally:
        ops.drop_deferred()
        ops.invalidate_panels()
        torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_large_tile_variant_against_fp64(dev, row):
    """The runners assert the kernel names of the row first (ops.kernel_log), then y / dx / dW / db per element, the fused statistics
    and the InstanceNorm-backward sums against fp64."""
    _run_row(dev, row)
    _SEEN[row[0][9]].add(row[0][-1])                          # (asserted equal to the log by the runner)
    _RAN.add(_row_id(row))


@pytest.mark.gpu
@pytest.mark.parametrize("row", SWITCH_ROWS, ids=_row_id)
def test_unset_switches_against_fp64(dev, row):
    _run_row(dev, row)


@pytest.mark.gpu
def test_part_one_reached_every_required_variant(dev):
    """The union of the kernel names part 1 launched (each asserted against the kernel log by its runner) holds both required lists."""
    not_run = [_row_id(r) for r in ROWS if _row_id(r) not in _RAN]
    assert not _missing(_SEEN), (_missing(_SEEN), f"{len(not_run)} rows of part 1 did not pass in this session", not_run[:5])
