"""The weight-gradient launchers' split, copy and fold plans on ragged volumes, against fp64, per element.

The seven launchers (wgrad_t3 / t3f, t3s, pwf, tf / tf-multi, tap, mfma, direct) deal K-tiles of TH x KWs voxels to ``nsplit`` blocks, every
split writes a partial copy into a capped scratch region (m1_wg_copies), and one of three fold kernels adds the copies up
(m1_wg_rx_finish), at once or from the batched queue.  test_convs_at_scale.py checks them per element at the bench step's round volumes
and default switches; test_hip_ops.py has ragged shapes of a few hundred voxels, one to three splits and only the generic fold.  Here
they run at 10,000 to 40,000 voxels (the larger side of a strided / transposed conv) on shapes chosen so that tile rows are ragged AND
the splits uneven, blocks walk many tiles, grids carry ghost blocks, the region clamps the copies, and every fold kernel meets awkward
bias widths -- and the planners' switches, which nothing else sets and checks, move the plans.

* part 0 (no GPU): wg_plan_of (tests/wgrad_plan_mirror.py), a restatement of the ladder, the K-tile geometry, the copy planner with every
  launcher's rule and the fold choice.  It reproduces the weight-gradient kernel names of every m1_conv3d_wgrad / m1_convT3d_wgrad key of
  C3_CONV_KEYS + EXTRA_CONV_KEYS and test_hip_ops._TF_EXPECT / _T3F_EXPECT / the T3S2 expectation; every row's kernel names and edge
  predicate hold on the mirror; DW_CANCEL holds for every row's inputs (on a 4 x 4 channel sample of dW: the channels are i.i.d.); the
  bound rejects a dW that lost one 64-voxel K-tile and one that lost a whole partial copy, at the largest row (40,000 voxels).
* part 1: ROWS, one test per row through ops.conv3d_same / conv3d_transpose_same at the production floor (M1_T3_MIN_BLOCKS=128) unless the
  row names a switch, accumulate 1 into pre-filled sinks with the folds queued, and accumulate 0, as test_convs_at_scale._wgrad_key.
  Each row asserts the kernel-log names, that the plan log (ops.plan_log) equals wg_plan_of entry for entry -- tiles, want, splits, fit,
  rx, stages, grid, fold kernel, copies, n, nb, EL, queued / now, declined rungs, the stem -- and dW / db per element.  The edge
  predicate was asserted on the mirror in part 0, so a row cannot pass on a fallback.
* the queue: 27 distinct small layers queued under m1_wgrad_defer and folded by one fold_pending: two batched launches, the three fold
  kernels mixed in the first; every layer meets the bound and equals, bit for bit, the same layer folded alone.
* part 2: every row with M1_WG_DET=1 twice, bit-equal.
* closing: the names, fold kernels and entry kinds part 1 logged contain REQUIRED.

Comparison: util.ref_conv_with_mag + util.assert_conv_close with util.CONV_A / CONV_R, inputs from test_convs_at_scale._conv_inputs; no
tolerance of this module's own.

Sensitivity (test_bound_rejects_a_lost_tile_and_a_lost_copy): with these inputs (x mean 0.5 + ramp, dy mean 0.3 + ramp) an element of dW
is a sum over V voxels of terms that do not cancel, so a 64-voxel tile carries about 64 / V of it: 1.6e-3 |ref| at V = 40,000, against a
bound of 4 * 2^-24 |ref| + 1e-5 mag <= about 8e-5 |ref| (DW_CANCEL).  Measured on the fp64 reference at the 40,000-voxel row: the lost
tile moves the MEDIAN element by 27 x its bound and 98 % of the elements leave it; a lost copy (3 tiles, 1 of 256) by 49 x.

Copies: which branches of m1_wg_copies a caller with a workspace can reach.  wgrad_rx_bytes sizes the region for the widest member and
never below two of ITS copies, and a member's own stride is no larger, so fit >= 2 always (test_the_region_always_holds_two_copies):
``fit < 1`` (M1_ERR_WORKSPACE) and the fallback launchers' ``fit < 2`` (one split, or atomics) need a null workspace, and with fit >= 1
``n < 1`` needs want < 1 or a byte ceiling below one copy -- tf's 96 MB against blocks of at most 128 x 128 x 27 floats: unreachable too.
What M1_WG_RX_MB=1 does reach is ``n > fit`` with 2 <= fit < want, and fit == 2 from the floor; the rx1-* rows are those.  The workspace
always comes from m1_conv_ws_bytes under the row's switches (ops allocates it per call).
"""
import zlib

import pytest
import torch

import util
from util import ops, assert_conv_close, ref_conv_with_mag
from test_ops_at_scale import _gen, _randn
from test_convs_at_scale import C3_CONV_KEYS, EXTRA_CONV_KEYS, DW_CANCEL, _DT, _conv_inputs
import test_hip_ops as H
from wgrad_plan_mirror import SWITCHES, wg_plan_of, kernel_names, parse_plan_entry, rx_bytes, t3_plan, tap_plan, _cdiv

K333, K133, K111 = (3, 3, 3), (1, 3, 3), (1, 1, 1)
ONE = (1, 1, 1)


# =================================================================================================================================
# the table
# =================================================================================================================================
def _wgs(e):
    return [x for x in e if x["kind"] == "wg"]


def _folds(e):
    return [x for x in e if x["kind"] == "fold"]


def _ragged(l, i=-1):
    p = l[i][2]
    return p.g.BH % p.TH != 0


def _uneven(e, i=-1):
    w = _wgs(e)[i]
    return w["tiles"] % w["splits"] != 0


def _ru(e, l, i=-1):
    return _ragged(l, i) and _uneven(e, i)


def _fold(e, mode, nb):
    f = _folds(e)[0]
    return f["mode"] == mode and f["nb"] == nb


# the edge a row exists for, as a predicate over wg_plan_of's (entries, launches); asserted in part 0, and part 1 asserts that the plan
# log of the real call EQUALS those entries
EDGES = {
    "ragged rows, uneven splits": _ru,
    "ghost unit": lambda e, l: _ru(e, l) and l[0][1].endswith(":big0") and (l[0][2].g.CA // 64 * len(_folds(e))) % 2 == 1,
    "whole-row tiles": lambda e, l: _ru(e, l) and l[-1][2].tiles_w == 1 and l[-1][2].KWs == l[-1][2].g.BW,
    "divisor search": lambda e, l: _ru(e, l) and l[0][2].g.BW == 36 and l[0][2].KWs == 12,
    "declined by t3 and tap": lambda e, l: _uneven(e) and l[0][0] == "mfma" and l[0][2].g.BW == 44 and t3_plan(l[0][2].g) is None and
    tap_plan(l[0][2].g) is None,
    "stride 2": lambda e, l: _ru(e, l) and l[-1][2].s2,
    "ph = 1: t3 must decline": lambda e, l: l[-1][2].g.ph == 1 and l[-1][2].g.pw == 1,
    "few splits, many tiles per block": lambda e, l: _ragged(l) and _wgs(e)[0]["splits"] == 2 and l[0][2].tpb >= 60,
    "two stages": lambda e, l: _ru(e, l) and _wgs(e)[0]["stages"] == 2,
    "three stages": lambda e, l: _ru(e, l) and _wgs(e)[0]["stages"] == 3 and l[0][2].tpb >= 2 * 3,
    "kws 32 needs CB % 128": lambda e, l: _ru(e, l) and l[0][2].g.BW % 32 == 0 and l[0][2].g.CB % 128 != 0 and l[0][2].KWs == 16,
    "TLh 16": lambda e, l: _ru(e, l) and l[0][2].TLh == 16,
    "TLh 32, partial units": lambda e, l: _ru(e, l) and l[0][2].TLh == 32 and l[0][2].g.CA % 32 and l[0][2].g.CB % 32,
    "TLh 32, stride 2": lambda e, l: _ru(e, l) and l[0][2].TLh == 32 and l[0][2].s2,
    "TLh 16, stride 2": lambda e, l: _ru(e, l) and l[0][2].TLh == 16 and l[0][2].s2,
    "V % PW_KT, uneven": lambda e, l: l[0][2].V % 128 != 0 and _uneven(e),
    "V % PW_KT, uneven, units": lambda e, l: l[0][2].V % 128 != 0 and _uneven(e) and l[0][2].nau * l[0][2].nbu > 1 and
    l[0][2].g.CA % 64 and l[0][2].g.CB % 64,
    "nks 4": lambda e, l: _ru(e, l) and l[0][2].nks == 4,
    "nks 2": lambda e, l: _ru(e, l) and l[0][2].nks == 2,
    "tf-multi then tf": lambda e, l: [x[0] for x in l] == ["tf-multi", "tf"] and _wgs(e)[0]["grid"][2] == 3 and _ru(e, l, 0),
    "four tf launches": lambda e, l: [x[0] for x in l] == ["tf"] * 4 and _ru(e, l, 0),
    "one tile per split": lambda e, l: _ragged(l) and _wgs(e)[0]["splits"] == _wgs(e)[0]["tiles"] < _wgs(e)[0]["want"],
    "one copy through the fold": lambda e, l: _ragged(l) and _wgs(e)[0]["splits"] == 1 and _folds(e)[0]["copies"] == 1,
    "stem": lambda e, l: _ru(e, l) and e[-1]["kind"] == "stem" and l[0][0] == "stem",
    "partial channel tiles": lambda e, l: _ru(e, l) and (l[0][2].g.CA % l[0][2].TA or l[0][2].g.CB % l[0][2].TB),
    "ghost blocks": lambda e, l: _ru(e, l) and (l[-1][2].ctiles * _wgs(e)[-1]["splits"] * l[-1][2].taps) % 8 != 0,
    "rounded up": lambda e, l: _ru(e, l) and _wgs(e)[0]["want"] * l[0][2].ctiles * l[0][2].taps > 512,
    "TV % KS, >= 3 splits": lambda e, l: l[0][2].TV % l[0][2].KS != 0 and _wgs(e)[0]["splits"] >= 3,
    "small rule": lambda e, l: l[0][2].small and _wgs(e)[0]["rx"] == 1 and _wgs(e)[0]["splits"] >= 24,
    "atomics": lambda e, l: _wgs(e)[0]["rx"] == 0 and _wgs(e)[0]["splits"] >= 3 and not _folds(e),
    "2 <= fit < want": lambda e, l: 2 <= _wgs(e)[-1]["fit"] == _wgs(e)[-1]["splits"] < _wgs(e)[-1]["want"],
    "fit == 2": lambda e, l: _wgs(e)[-1]["fit"] == 2 == _wgs(e)[-1]["splits"],
    "generic nb 8": lambda e, l: _fold(e, "generic", 8), "wide nb 8": lambda e, l: _fold(e, "wide", 8),
    "vec nb 8": lambda e, l: _fold(e, "vec", 8),
    "generic nb 96": lambda e, l: _fold(e, "generic", 96), "wide nb 96": lambda e, l: _fold(e, "wide", 96),
    "vec nb 96": lambda e, l: _fold(e, "vec", 96),
    "generic nb 160": lambda e, l: _fold(e, "generic", 160), "wide nb 160": lambda e, l: _fold(e, "wide", 160),
    "vec nb 160": lambda e, l: _fold(e, "vec", 160),
    "generic nb 320": lambda e, l: _fold(e, "generic", 320), "wide nb 320": lambda e, l: _fold(e, "wide", 320),
    "vec nb 320": lambda e, l: _fold(e, "vec", 320),
    "CB % 4 stays generic": lambda e, l: _fold(e, "generic", 6) and _folds(e)[0]["n"] >= 65536,
    "EL 4": lambda e, l: _folds(e)[0]["mode"] == "generic" and _folds(e)[0]["el"] == 4,
    "EL 16": lambda e, l: _folds(e)[0]["mode"] == "generic" and _folds(e)[0]["el"] == 16,
    "40,000 voxels": lambda e, l: _ru(e, l) and l[0][2].g.N * l[0][2].g.BD * l[0][2].g.BH * l[0][2].g.BW == 40000,
}


def R(rid, kind, N, dims, cins, cout, k, s, dt, sw, kern, edge):
    name = "m1_convT3d_wgrad" if kind == "t" else "m1_conv3d_wgrad"
    return (rid, (name, N, *dims, tuple(cins), cout, k, s, dt), sw, kern, edge)


RX1 = {"M1_WG_RX_MB": 1}
RX1_T3 = {"M1_WG_RX_MB": 1, "M1_T3_MIN_BLOCKS": 1}      # (two to seven splits are below the production floor of wgrad_t3)
ROWS = [
    # ---- wgrad_t3 (bf16)
    R("t3-kws8", "c", 1, (6, 42, 40), [128], 128, K333, ONE, "bf16", {}, "wgrad_t3:kws8:big1", "ragged rows, uneven splits"),
    R("t3-kws16-big0-2mem", "c", 1, (9, 49, 48), [64, 64], 64, K333, ONE, "bf16", {}, "wgrad_t3:kws16:big0", "ragged rows, uneven splits"),
    R("t3-kws16-big0-3mem", "c", 1, (10, 21, 48), [64, 64, 64], 64, K333, ONE, "bf16", {}, "wgrad_t3:kws16:big0", "ghost unit"),
    R("t3-kws32", "c", 2, (10, 17, 32), [128], 128, K333, ONE, "bf16", {}, "wgrad_t3:kws32:big1", "ragged rows, uneven splits"),
    R("t3-row12", "c", 2, (10, 42, 12), [128], 128, K333, ONE, "bf16", {}, "wgrad_t3:kws12:big1", "whole-row tiles"),
    R("t3-row20", "c", 1, (5, 100, 20), [128, 128], 128, K333, ONE, "bf16", {}, "wgrad_t3:kws20:big1", "whole-row tiles"),
    R("t3-row28", "c", 1, (11, 33, 28), [128], 128, K333, ONE, "bf16", {}, "wgrad_t3:kws28:big1", "whole-row tiles"),
    R("t3-w36", "c", 1, (9, 31, 36), [128], 128, K333, ONE, "bf16", {}, "wgrad_t3:kws12:big1", "divisor search"),
    R("w44", "c", 1, (2, 114, 44), [128], 128, K333, ONE, "bf16", {}, "wgrad_mfma", "declined by t3 and tap"),
    R("t3-s2-122", "c", 1, (9, 18, 80), [128], 256, K333, (1, 2, 2), "bf16", {}, "wgrad_t3:s2:kws8:big1", "stride 2"),
    R("t3-s2-222", "c", 1, (9, 18, 80), [256], 256, K333, (2, 2, 2), "bf16", {}, "wgrad_t3:s2:kws8:big1", "stride 2"),
    R("t3-s2-T122", "t", 1, (9, 9, 40), [256], 128, K333, (1, 2, 2), "bf16", {}, "wgrad_t3:s2:kws8:big1", "stride 2"),
    R("t3-s2-T222", "t", 1, (5, 9, 40), [256], 256, K333, (2, 2, 2), "bf16", {}, "wgrad_t3:s2:kws8:big1", "stride 2"),
    R("t3-s2-T-thin", "t", 1, (9, 9, 40), [2, 256], 128, K333, (1, 2, 2), "bf16", {}, "wgrad_mfma+wgrad_t3:s2:kws8:big1", "stride 2"),
    R("s2-oddHW-w65", "c", 1, (2, 77, 65), [64], 128, K333, (1, 2, 2), "bf16", {}, "wgrad_mfma", "ph = 1: t3 must decline"),
    R("s2-oddHW-w41", "c", 1, (4, 61, 41), [64], 128, K333, (1, 2, 2), "bf16", {}, "wgrad_tap", "ph = 1: t3 must decline"),
    R("t3-blocks-small", "c", 1, (10, 25, 40), [128], 128, K333, ONE, "bf16", {"M1_T3_BLOCKS": 12, "M1_T3_MIN_BLOCKS": 1},
      "wgrad_t3:kws8:big1", "few splits, many tiles per block"),
    R("t3-stages2", "c", 1, (6, 42, 40), [128], 128, K333, ONE, "bf16", {"M1_T3_STAGES": 2}, "wgrad_t3:kws8:big1", "two stages"),
    # ---- wgrad_t3f / t3s / pwf (fp32)
    R("t3f-kws8", "c", 2, (7, 33, 40), [64, 64], 64, K333, ONE, "fp32", {}, "wgrad_t3f:kws8:big0", "ragged rows, uneven splits"),
    R("t3f-kws16", "c", 1, (10, 21, 48), [128], 128, K333, ONE, "fp32", {}, "wgrad_t3f:kws16:big1", "ragged rows, uneven splits"),
    R("t3f-kws32", "c", 1, (9, 113, 32), [128], 128, K133, ONE, "fp32", {}, "wgrad_t3f:kws32:big1", "ragged rows, uneven splits"),
    R("t3f-w32-cb64", "c", 1, (6, 113, 32), [64, 64], 64, K333, ONE, "fp32", {}, "wgrad_t3f:kws16:big0", "kws 32 needs CB % 128"),
    R("t3f-3mem", "c", 2, (11, 19, 24), [64, 64, 64], 64, K333, ONE, "fp32", {}, "wgrad_t3f:kws8:big0", "ghost unit"),
    R("t3s-tl16", "c", 1, (11, 38, 24), [16], 24, K333, ONE, "fp32", {}, "wgrad_t3s", "TLh 16"),
    R("t3s-tl32", "c", 1, (11, 19, 48), [40], 72, K133, ONE, "fp32", {}, "wgrad_t3s", "TLh 32, partial units"),
    R("t3s-s2-122", "c", 1, (3, 70, 48), [32], 64, K133, (1, 2, 2), "fp32", {}, "wgrad_t3s", "TLh 32, stride 2"),
    R("t3s-s2-222", "c", 1, (3, 70, 48), [16], 8, K333, (2, 2, 2), "fp32", {}, "wgrad_t3s", "TLh 16, stride 2"),
    R("t3s-T122", "t", 1, (3, 35, 24), [64], 32, K133, (1, 2, 2), "fp32", {}, "wgrad_t3s", "TLh 32, stride 2"),
    R("t3s-blocks-small", "c", 1, (9, 33, 40), [16], 24, K333, ONE, "fp32", {"M1_T3S_BLOCKS": 12}, "wgrad_t3s",
      "few splits, many tiles per block"),
    R("pwf-ragged", "c", 1, (4, 100, 25), [20], 12, K111, ONE, "fp32", {}, "wgrad_pwf", "V % PW_KT, uneven"),
    R("pwf-units", "c", 1, (4, 100, 25), [72], 200, K111, ONE, "fp32", {}, "wgrad_pwf", "V % PW_KT, uneven, units"),
    R("pwf-blocks-small", "c", 1, (4, 100, 25), [72], 200, K111, ONE, "fp32", {"M1_PWF_BLOCKS": 24}, "wgrad_pwf", "V % PW_KT, uneven, units"),
    # ---- wgrad_tf / tf-multi (bf16)
    R("tf-nks4-w24-c8", "c", 2, (11, 49, 24), [8], 8, K133, ONE, "bf16", {}, "wgrad_tf", "nks 4"),
    R("tf-nks4-w48-c16-32", "c", 2, (11, 25, 48), [16], 32, K133, ONE, "bf16", {}, "wgrad_tf", "nks 4"),
    R("tf-nks4-w96-c32-96", "c", 1, (5, 21, 96), [32], 96, K133, ONE, "bf16", {}, "wgrad_tf", "nks 4"),
    R("tf-nks4-k333-c16-8", "c", 2, (11, 49, 24), [16], 8, K333, ONE, "bf16", {}, "wgrad_tf", "nks 4"),
    R("tf-nks2-w24-c32", "c", 2, (11, 25, 24), [32], 32, K333, ONE, "bf16", {}, "wgrad_tf", "nks 2"),
    R("tf-nks2-w48-c96-16", "c", 1, (11, 19, 48), [96], 16, K333, ONE, "bf16", {}, "wgrad_tf", "nks 2"),
    R("tf-nks2-w96-c8-32", "c", 2, (9, 9, 96), [8], 32, K333, ONE, "bf16", {}, "wgrad_tf", "nks 2"),
    R("tf-multi-then-tf", "c", 2, (11, 49, 24), [32, 32, 32, 16], 32, K133, ONE, "bf16", {}, "wgrad_tf+wgrad_tf", "tf-multi then tf"),
    R("tf-multi-off", "c", 2, (11, 49, 24), [32, 32, 32, 16], 32, K133, ONE, "bf16", {"M1_TF_MULTI": 0},
      "wgrad_tf+wgrad_tf+wgrad_tf+wgrad_tf", "four tf launches"),
    R("tf-split512", "c", 1, (5, 50, 40), [16], 16, K333, ONE, "bf16", {"M1_TF_SPLIT": 512}, "wgrad_tf", "one tile per split"),
    R("tf-split1", "c", 1, (5, 50, 40), [16], 16, K333, ONE, "bf16", {"M1_TF_SPLIT": 1}, "wgrad_tf", "one copy through the fold"),
    R("tf-nks4-off", "c", 2, (9, 17, 40), [16], 16, K133, ONE, "bf16", {"M1_TF_NKS4": 0}, "wgrad_tf", "nks 2"),
    R("tf-maxc512", "c", 1, (5, 50, 40), [256], 32, K333, ONE, "bf16", {"M1_TF_MAXC": 512}, "wgrad_tf", "ragged rows, uneven splits"),
    R("tf-stages3", "c", 2, (11, 49, 24), [8], 8, K133, ONE, "bf16", {"M1_TF_STAGES": 3, "M1_TF_SPLIT": 32}, "wgrad_tf", "three stages"),
    R("tf-40000", "c", 2, (10, 50, 40), [32], 32, K333, ONE, "bf16", {}, "wgrad_tf", "40,000 voxels"),
] + [R(f"stem-bf16-c{c}", "c", 2, (9, 33, 40), [c], 32, K133, ONE, "bf16", {}, "wgrad_tf", "stem") for c in range(1, 8)] + [
    R(f"stem-fp32-c{c}", "c", 1, (11, 38, 24), [c], 32, K133, ONE, "fp32", {}, "wgrad_t3s", "stem") for c in range(1, 4)] + [
    # ---- wgrad_tap
    R("tap-64-64-row20", "c", 1, (5, 100, 20), [64], 64, K333, ONE, "bf16", {}, "wgrad_tap", "whole-row tiles"),
    R("tap-64-64-row12", "c", 1, (9, 93, 12), [64], 64, K111, ONE, "bf16", {}, "wgrad_tap", "whole-row tiles"),
    R("tap-64-128", "c", 1, (5, 50, 40), [64], 200, K133, ONE, "bf16", {}, "wgrad_tap", "partial channel tiles"),
    R("tap-128-64", "c", 1, (5, 50, 40), [72], 64, K133, ONE, "bf16", {}, "wgrad_tap", "ghost blocks"),
    R("tap-128-64-xcd0", "c", 1, (5, 50, 40), [72], 64, K133, ONE, "bf16", {"M1_WG_XCD": 0}, "wgrad_tap", "ghost blocks"),
    R("tap-128-128", "c", 1, (5, 50, 40), [72], 200, K333, ONE, "bf16", {}, "wgrad_tap", "partial channel tiles"),
    R("tap-128-128-row20", "c", 1, (5, 100, 20), [72], 200, K133, ONE, "bf16", {}, "wgrad_tap", "whole-row tiles"),
    R("tap-floor0", "c", 1, (5, 50, 40), [72], 200, K133, ONE, "bf16", {"M1_WG_FLOOR": 0}, "wgrad_tap", "rounded up"),
    R("tap-stages2", "c", 1, (5, 50, 40), [64], 200, K133, ONE, "bf16", {"M1_WG_TAP_STAGES": 2}, "wgrad_tap", "two stages"),
    R("tap-blocks-small", "c", 1, (5, 50, 40), [72], 200, K133, ONE, "bf16", {"M1_WG_TAP_BLOCKS": 36}, "wgrad_tap",
      "few splits, many tiles per block"),
    # ---- wgrad_mfma
    R("mfma-w9", "c", 1, (12, 93, 9), [32], 32, K111, ONE, "bf16", {}, "wgrad_mfma", "TV % KS, >= 3 splits"),
    R("mfma-c20", "c", 1, (9, 53, 21), [20], 20, K133, ONE, "bf16", {}, "wgrad_mfma", "TV % KS, >= 3 splits"),
    R("mfma-c12-fp32", "c", 1, (9, 53, 21), [64], 12, K333, ONE, "fp32", {}, "wgrad_mfma", "TV % KS, >= 3 splits"),
    R("mfma-c3", "c", 1, (9, 53, 21), [32], 3, K333, ONE, "bf16", {}, "wgrad_mfma", "TV % KS, >= 3 splits"),
    R("mfma-blocks-small", "c", 1, (9, 53, 21), [32], 32, K111, ONE, "bf16", {"M1_WG_BLOCKS": 3}, "wgrad_mfma", "TV % KS, >= 3 splits"),
    R("mfma-blocks-large", "c", 1, (2, 114, 44), [128], 128, K333, ONE, "bf16", {"M1_WG_BLOCKS": 4096}, "wgrad_mfma", "TV % KS, >= 3 splits"),
    R("mfma-small-rule", "c", 1, (11, 102, 21), [32], 32, K133, ONE, "bf16", {"M1_WG_DET": 0}, "wgrad_mfma", "small rule"),
    R("mfma-det0", "c", 1, (2, 114, 44), [128], 128, K333, ONE, "bf16", {"M1_WG_DET": 0}, "wgrad_mfma", "atomics"),
    # ---- copies clamped by the region
    R("rx1-t3-clamped", "c", 1, (5, 50, 40), [64, 64], 64, K133, ONE, "bf16", RX1_T3, "wgrad_t3:kws8:big0", "2 <= fit < want"),
    R("rx1-t3-fit2", "c", 1, (5, 50, 40), [128], 128, K333, ONE, "bf16", RX1_T3, "wgrad_t3:kws8:big1", "fit == 2"),
    R("rx1-tf-clamped", "c", 1, (5, 50, 40), [32], 32, K333, ONE, "bf16", RX1, "wgrad_tf", "2 <= fit < want"),
    R("rx1-tf-fit2", "c", 1, (5, 50, 40), [128], 32, K333, ONE, "bf16", RX1, "wgrad_tf", "fit == 2"),
    R("rx1-tap-clamped", "c", 1, (5, 100, 20), [64], 64, K133, ONE, "bf16", RX1, "wgrad_tap", "2 <= fit < want"),
    R("rx1-tap-fit2", "c", 1, (5, 100, 20), [128], 128, K333, ONE, "bf16", RX1, "wgrad_tap", "fit == 2"),
    R("rx1-mfma-clamped", "c", 1, (9, 53, 21), [32], 64, K333, ONE, "bf16", RX1, "wgrad_mfma", "2 <= fit < want"),
    R("rx1-mfma-fit2", "c", 1, (2, 114, 44), [128], 128, K333, ONE, "bf16", RX1, "wgrad_mfma", "fit == 2"),
    # ---- the three fold kernels at awkward bias widths
    R("fold-generic-nb8", "c", 1, (5, 50, 40), [32], 8, K133, ONE, "bf16", {}, "wgrad_tf", "generic nb 8"),
    R("fold-wide-nb8", "c", 1, (5, 50, 40), [160], 8, K333, ONE, "bf16", {}, "wgrad_mfma", "wide nb 8"),
    R("fold-vec-nb8", "c", 1, (5, 50, 40), [320], 8, K333, ONE, "bf16", {}, "wgrad_mfma", "vec nb 8"),
    R("fold-generic-nb96", "c", 1, (5, 50, 40), [8], 96, K133, ONE, "bf16", {}, "wgrad_tf", "generic nb 96"),
    R("fold-wide-nb96", "c", 1, (5, 50, 40), [32], 96, K333, ONE, "bf16", {}, "wgrad_tf", "wide nb 96"),
    R("fold-vec-nb96", "c", 1, (5, 50, 40), [32], 96, K333, ONE, "bf16", {"M1_TF_SPLIT": 16}, "wgrad_tf", "vec nb 96"),
    R("fold-generic-nb160", "c", 1, (5, 50, 40), [8], 160, K133, ONE, "bf16", {}, "wgrad_mfma", "generic nb 160"),
    R("fold-wide-nb160", "c", 1, (5, 50, 40), [32], 160, K333, ONE, "bf16", {"M1_WG_BLOCKS": 2048}, "wgrad_mfma", "wide nb 160"),
    R("fold-vec-nb160", "c", 1, (5, 50, 40), [32], 160, K333, ONE, "bf16", {}, "wgrad_mfma", "vec nb 160"),
    R("fold-generic-nb320", "c", 1, (5, 50, 40), [8], 320, K133, ONE, "bf16", {}, "wgrad_mfma", "generic nb 320"),
    R("fold-wide-nb320", "c", 1, (5, 50, 40), [32], 320, K133, ONE, "bf16", {}, "wgrad_mfma", "wide nb 320"),
    R("fold-vec-nb320", "c", 1, (5, 50, 40), [32], 320, K333, ONE, "bf16", {}, "wgrad_mfma", "vec nb 320"),
    R("fold-generic-cb6", "c", 1, (5, 50, 40), [512], 6, K333, ONE, "bf16", {}, "wgrad_mfma", "CB % 4 stays generic"),
    R("fold-generic-el4", "c", 1, (5, 50, 40), [8], 8, K133, ONE, "bf16", {}, "wgrad_tf", "EL 4"),
    R("fold-generic-el16", "c", 1, (5, 50, 40), [16], 16, K133, ONE, "bf16", {}, "wgrad_tf", "EL 16"),
]
_ROW_IDS = [r[0] for r in ROWS]

# what part 1 must have logged: kernel names (prefixes), fold kernels, entry kinds
REQUIRED = {"wgrad_t3:kws", "wgrad_t3:s2:", "wgrad_t3f:", "wgrad_t3s", "wgrad_pwf", "wgrad_tf", "wgrad_tap", "wgrad_mfma",
            "fold:generic", "fold:vec", "fold:wide", "stem:", "decline:", "foldbatch:"}
# (wgrad_direct is the ladder's last resort behind m1_set_force_direct / a shape wgrad_mfma cannot index -- more than 2^31 voxels; it
# makes no plan and notes nothing in the plan log: test_hip_ops.py runs it under force_direct)


def _plan(row, queued=True):
    rid, key, sw, kern, edge = row
    return wg_plan_of(*key, switches=sw, queued=queued)


def _big_voxels(key):
    name, N, D, H, W, cins, cout, k, s, dt = key
    V = N * D * H * W
    return V * s[0] * s[1] * s[2] if "convT" in name else V


# =================================================================================================================================
# part 0: the mirror against the pinned tables; the table against the mirror; the inputs; the bound
# =================================================================================================================================
def test_mirror_reproduces_the_pinned_bench_names():
    keys = [q for q in C3_CONV_KEYS + EXTRA_CONV_KEYS if q[0] in ("m1_conv3d_wgrad", "m1_convT3d_wgrad")]
    assert len(keys) >= 60, len(keys)
    wrong = [(q, kernel_names(wg_plan_of(*q[:10])[0])) for q in keys if "+".join(kernel_names(wg_plan_of(*q[:10])[0])) != q[-1]]
    assert not wrong, wrong
    assert SWITCHES["M1_T3_MIN_BLOCKS"] == 128


def _base(names):
    return {n.split(":")[0] for n in names}


def test_mirror_reproduces_the_op_tests_expectations():
    """test_hip_ops._TF_EXPECT (at both floors of wgrad_t3), _T3F_EXPECT and the T3S2 expectation (at the suite's floor, 1)."""
    for ((dims, cins, cout, k, s, T), floor), expect in zip(H._TF_PARAMS, H._TF_EXPECT):
        e, _ = wg_plan_of("m1_convT3d_wgrad" if T else "m1_conv3d_wgrad", *dims, tuple(cins), cout, k, s, "bf16", {"M1_T3_MIN_BLOCKS": floor})
        assert _base(kernel_names(e)) == expect, (dims, cins, cout, k, s, T, floor, kernel_names(e))
        if expect == H._T3 and s[1] == 2:
            assert any(n.startswith("wgrad_t3:s2:") for n in kernel_names(e))
    for (dims, cins, cout, k), expect in zip(H.T3F_CASES, H._T3F_EXPECT):
        e, _ = wg_plan_of("m1_conv3d_wgrad", *dims, tuple(cins), cout, k, ONE, "fp32", {"M1_T3_MIN_BLOCKS": 1})
        assert _base(kernel_names(e)) == {expect}, (dims, cins, cout, k, kernel_names(e))
    for idx, (dims, cins, cout, k, s, T) in enumerate(H.T3S2_CASES):
        e, _ = wg_plan_of("m1_convT3d_wgrad" if T else "m1_conv3d_wgrad", *dims, tuple(cins), cout, k, s, "fp32", {"M1_T3_MIN_BLOCKS": 1})
        assert _base(kernel_names(e)) == {"wgrad_t3s" if idx < 4 else "wgrad_mfma"}, (idx, kernel_names(e))


def test_table_names_edges_and_sizes_are_what_the_mirror_says():
    assert len(set(_ROW_IDS)) == len(ROWS) <= 100
    for row in ROWS:
        rid, key, sw, kern, edge = row
        assert set(sw) <= set(SWITCHES), rid
        e, l = _plan(row)
        assert "+".join(kernel_names(e)) == kern, (rid, kernel_names(e))
        assert EDGES[edge](e, l), (rid, edge, e)
        assert 10000 <= _big_voxels(key) <= 40000, (rid, _big_voxels(key))
    # the edges the launchers have, each by at least one row
    plans = {r[0]: _plan(r) for r in ROWS}
    for kws in (8, 16, 32):
        assert any(r[3] == f"wgrad_t3:kws{kws}:big{b}" and r[4] == "ragged rows, uneven splits" for r in ROWS for b in (0, 1)), kws
        assert any(r[3].startswith(f"wgrad_t3f:kws{kws}:") for r in ROWS), kws
    assert {l[0][2].g.BW for rid, (e, l) in plans.items() if rid.startswith("t3-row")} == {12, 20, 28}
    assert {(l[0][2].TA, l[0][2].TB) for rid, (e, l) in plans.items() if rid.startswith("tap-")} == {(64, 64), (64, 128), (128, 64), (128, 128)}
    assert {l[0][2].kparts for rid, (e, l) in plans.items() if rid.startswith("tf-nks")} == {1, 2, 4}
    assert {(l[0][2].nks, l[0][2].g.BW) for rid, (e, l) in plans.items() if rid.startswith("tf-nks") and "off" not in rid} >= {
        (4, 24), (4, 48), (4, 96), (2, 24), (2, 48), (2, 96)}
    assert any(x["kind"] == "decline" for e, l in plans.values() for x in e)
    modes = {(f["mode"], f["nb"]) for e, l in plans.values() for f in _folds(e)}
    assert modes >= {(m, nb) for m in ("generic", "vec", "wide") for nb in (8, 96, 160, 320)}


def test_the_region_always_holds_two_copies():
    """wgrad_rx_bytes against every member's own stride, at the smallest cap: fit >= 2 for every member of every row and of every pinned
    bench key -- the ``fit < 1`` and ``fit < 2`` branches of m1_wg_copies need a null workspace."""
    keys = [r[1] for r in ROWS] + [q[:10] for q in C3_CONV_KEYS + EXTRA_CONV_KEYS if "wgrad" in q[0]]
    for name, N, D, H, W, cins, cout, k, s, dt in keys:
        for mb in (1, 64):
            floats = rx_bytes(cins, cout, k, {"M1_WG_RX_MB": mb}) // 4
            for c in tuple(cins) + (8,):
                stride = k[0] * k[1] * k[2] * c * cout + (c if "convT" in name else cout)
                assert floats // stride >= 2, (name, cins, cout, k, mb)
    for row in ROWS:
        assert all(w["fit"] >= 2 for w in _wgs(_plan(row)[0])), row[0]


def _cpu_sample(key, seed):
    """fp64 dW (and its sum of |terms|) of the row's geometry with at most 4 channels a side: the channels of _conv_inputs are i.i.d., so
    the median of mag / |ref| over this block is the layer's."""
    name, N, D, H, W, cins, cout, k, s, dt = key
    cpu = torch.device("cpu")
    T = "convT" in name
    xs, w, b, dy = _conv_inputs(cpu, _DT[dt], N, (D, H, W), [min(4, sum(cins))], min(4, cout), k, s, T, _gen(cpu, seed))
    return ref_conv_with_mag(xs[0], w, b, s, dy, T)


def test_weight_gradient_sums_of_every_rows_inputs_do_not_cancel():
    seen = {}
    for rid, key, sw, kern, edge in ROWS:
        geo = (key[0], *key[1:5], key[7], key[8], key[9])
        if geo in seen:
            continue
        ref, mag = _cpu_sample(key, 7)
        seen[geo] = float((mag["dw"] / ref["dw"].abs()).median())
        assert seen[geo] < DW_CANCEL, (rid, seen[geo])
    assert len(seen) >= 20


def test_bound_rejects_a_lost_tile_and_a_lost_copy():
    """On the reference alone, at the largest row: dW summed over all voxels but one 64-voxel K-tile (TH x KWs = 8 x 8 voxels of one
    (n, d) slice of dY), and over all but the K-tiles of one split (one partial copy left out of the fold)."""
    row = max(ROWS, key=lambda r: _big_voxels(r[1]))
    rid, key, sw, kern, edge = row
    assert _big_voxels(key) == 40000 and rid == "tf-40000"
    name, N, D, H, W, cins, cout, k, s, dt = key
    e, l = _plan(row)
    p, wg = l[0][2], _wgs(e)[0]
    assert (p.TH, p.KWs) == (8, 8) and wg["splits"] == 256 and wg["tiles"] == 700 and p.tpb == 3
    cpu = torch.device("cpu")
    xs, w, b, dy = _conv_inputs(cpu, _DT[dt], N, (D, H, W), list(cins), cout, k, s, False, _gen(cpu, 5))
    ref, mag = ref_conv_with_mag(xs[0], w, b, s, dy)
    assert_conv_close(ref["dw"].float(), ref["dw"], mag["dw"], torch.float32, "undamaged dW")
    bound = util.CONV_A[torch.float32] * ref["dw"].abs() + util.CONV_R * mag["dw"]

    def without(mask):
        lost, _ = ref_conv_with_mag(xs[0], w, b, s, dy * mask)
        return ref["dw"] - lost["dw"], lost["dw"].abs()
    tile = torch.zeros_like(dy)
    tile[1, 4, 16:24, 8:16] = 1                               # one K-tile of the last-but-ragged rows
    bad, moved = without(tile)
    with pytest.raises(AssertionError, match="elements outside"):
        assert_conv_close(bad.float(), ref["dw"], mag["dw"], torch.float32, "dW without one K-tile")
    assert float((moved > bound).double().mean()) > 0.9
    margin = float((moved / bound).median())
    assert margin > 10, margin                                # (measured 27: the docstring's figure)
    # one split's K-tiles: ceil(700 / 256) = 3 tiles of one tile row of an interior slice
    copy = torch.zeros_like(dy)
    copy[0, 4, 8:16, 0:24] = 1
    bad, moved = without(copy)
    with pytest.raises(AssertionError, match="elements outside"):
        assert_conv_close(bad.float(), ref["dw"], mag["dw"], torch.float32, "dW without one partial copy")
    print(f"lost tile: median |lost| / bound = {margin:.1f}; lost copy: {float((moved / bound).median()):.1f}")
    assert float((moved > bound).double().mean()) > 0.9 and float((moved / bound).median()) > margin


# =================================================================================================================================
# part 1: the rows on the GPU
# =================================================================================================================================
_SEEN = set()          # kernel names, "fold:<mode>", "stem:", "decline:", "foldbatch:" part 1 logged
_RAN = set()
REPORT = {}            # row id -> (kernels, tiles, splits, fit, fold kernels, worst |d| / bound over dW)


def _fold_blocks(f):
    if f["mode"] == "vec":
        return min(_cdiv(f["n"] // 4, 256), 4096)
    if f["mode"] == "wide":
        return _cdiv(f["n"] - f["nb"], 256)
    return _cdiv(f["n"], f["el"])


def _expect_log(row, queued):
    """The plan log of one backward pass + fold_pending: wg_plan_of's entries, then one foldbatch per 24 queued folds."""
    e, _ = _plan(row, queued)
    q = [f for f in e if f["kind"] == "fold" and f["when"] == "queued"]
    return e + [dict(kind="foldbatch", n=len(q[i:i + 24]), blocks=sum(_fold_blocks(f) for f in q[i:i + 24])) for i in range(0, len(q), 24)]


def _share(got, ref, mag, acc):
    bound = util.CONV_A[torch.float32] * (2 if acc else 1) * ref.abs() + util.CONV_R * mag
    return float(((got.double() - ref).abs() / bound).max())


def _inputs(dev, row):
    rid, key, sw, kern, edge = row
    name, N, D, H, W, cins, cout, k, s, dts = key
    dtype, T = _DT[dts], "convT" in name
    g = _gen(dev, zlib.crc32(rid.encode()) % 10007)
    xs, w, b, dy = _conv_inputs(dev, dtype, N, (D, H, W), list(cins), cout, k, s, T, g)
    pre = (2.0 + _randn(tuple(w.shape), g, dev), -1.0 + _randn((cout,), g, dev))
    return dtype, T, xs, w, b, dy, pre


def _backward(dtype, T, xs, w, b, dy, pre, k, s, sink, fold=True):
    """One forward + backward of the layer; sink: accumulate 1 into pre-filled sinks, folds queued until fold_pending."""
    wd, bd = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    if sink:
        wd._m1_gsink, bd._m1_gsink = pre[0].clone(), pre[1].clone()
    y = (ops.conv3d_transpose_same if T else ops.conv3d_same)([x.to(dtype) for x in xs], wd, bd, k, s)
    with ops.kernel_log() as kl, ops.plan_log() as pl:
        y.backward(dy.to(dtype))
        if fold:
            ops.fold_pending()
            torch.cuda.synchronize()
    if sink:
        assert wd.grad is None and bd.grad is None
        return wd._m1_gsink, bd._m1_gsink, kl.names, pl.entries
    return wd.grad, bd.grad, kl.names, pl.entries


def _run_row(dev, row):
    rid, key, sw, kern, edge = row
    k, s = key[7], key[8]
    dtype, T, xs, w, b, dy, pre = _inputs(dev, row)
    ref, mag = ref_conv_with_mag(torch.cat(xs, -1), w, b, s, dy, T)
    assert float((mag["dw"] / ref["dw"].abs()).median()) < DW_CANCEL
    shares = []
    for sink in (True, False):
        gw, gb, names, entries = _backward(dtype, T, xs, w, b, dy, pre, k, s, sink)
        assert [n for n in names if n.startswith("wgrad")] == kern.split("+"), (rid, names, kern)
        got = [parse_plan_entry(x) for x in entries]
        want = _expect_log(row, queued=sink)
        assert got == want, (rid, sink, got, want)
        if sink:
            _SEEN.update(names)
            _SEEN.update(x.split(" ")[0] if x.startswith("fold:") else x.split("=")[0].split(":")[0] + ":" for x in entries if not x.startswith("wg:"))
            rw, rb = pre[0].double() + ref["dw"], pre[1].double() + ref["db"]
            mw, mb = mag["dw"] + pre[0].double().abs(), mag["db"] + pre[1].double().abs()
            what = "(accumulate 1, folds queued)"
        else:
            rw, rb, mw, mb, what = ref["dw"], ref["db"], mag["dw"], mag["db"], "(accumulate 0)"
        shares.append(_share(gw, rw, mw, sink))
        assert_conv_close(gw, rw, mw, torch.float32, f"dW {what} of {rid}", acc=sink)
        assert_conv_close(gb, rb, mb, torch.float32, f"db {what} of {rid}", acc=sink)
    wg = [x for x in want if x["kind"] == "wg"]
    REPORT[rid] = (kern, [x["tiles"] for x in wg], [x["splits"] for x in wg], [x["fit"] for x in wg],
                   [f["mode"] for f in want if f["kind"] == "fold"], max(shares))
    print(f"PLANROW {rid}: {kern} tiles={REPORT[rid][1]} splits={REPORT[rid][2]} fit={REPORT[rid][3]} fold={REPORT[rid][4]} "
          f"worst share of bound={max(shares):.3f}")


def _cleanup():
    ops.drop_deferred()
    ops.invalidate_panels()
    torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=_ROW_IDS)
def test_plan_row_against_fp64(dev, row):
    try:
        with ops.config(M1_T3_MIN_BLOCKS=128), ops.config(**row[2]):       # (the production floor; nothing else unless the row says so)
            _run_row(dev, row)
    finally:
        _cleanup()
    _RAN.add(row[0])


# ---- the queue: more folds than one batched launch holds, the three fold kernels in one batch ----
def _queue_layers():
    """27 distinct layers on one ragged volume of 1,248 voxels: (cins, cout, k), all Conv3D, bf16."""
    tf = [([ci], co, k) for k in (K133, K333) for ci in (8, 16, 32) for co in (8, 16, 32)]
    big = [([32], 160, K333), ([160], 8, K333), ([32], 64, K333), ([32], 96, K333), ([320], 8, K333), ([32], 320, K333), ([32], 320, K133),
           ([64], 64, K333), ([512], 6, K333)]
    return (big[:5] + tf + big[5:])[:27]


QUEUE_VOL = (1, (4, 13, 24))


def _queue_rows():
    N, dims = QUEUE_VOL
    return [R(f"queue-{i}", "c", N, dims, ci, co, k, ONE, "bf16", {}, None, None) for i, (ci, co, k) in enumerate(_queue_layers())]


def test_queue_layers_mix_the_fold_kernels_in_the_first_batch():
    rows = _queue_rows()
    assert len(rows) == 27 and len({r[1] for r in rows}) == 27
    folds = [f for r in rows for f in _folds(_plan(r)[0])]
    assert len(folds) >= 26 and all(f["when"] == "queued" for f in folds)
    assert {f["mode"] for f in folds[:24]} == {"generic", "vec", "wide"}, [f["mode"] for f in folds]


@pytest.mark.gpu
def test_more_folds_than_one_batched_launch_holds(dev, monkeypatch):
    monkeypatch.setitem(ops._WGP, "maxvox", 0)                # launched where autograd calls them, folds queued ...
    monkeypatch.setitem(ops._FOLD, "async", 0)                # ... until the one fold_pending below: no fold trigger of ops' own
    monkeypatch.setitem(ops._FOLD, "async_mb", 0)
    rows = _queue_rows()
    data = [_inputs(dev, r) for r in rows]
    try:
        with ops.config(M1_T3_MIN_BLOCKS=128):
            assert ops.config_get("M1_WG_DET") in (None, 1)
            queued, logged = [], []
            for r, d in zip(rows, data):
                gw, gb, names, entries = _backward(*d, r[1][7], r[1][8], sink=True, fold=False)
                queued.append((gw, gb))
                logged += entries
            with ops.plan_log() as pl:
                ops.fold_pending()
                torch.cuda.synchronize()
            want = [x for r in rows for x in _plan(r)[0]]
            assert [parse_plan_entry(x) for x in logged] == want, (logged, want)
            nq = len([x for x in want if x["kind"] == "fold"])
            batches = [parse_plan_entry(x) for x in pl.entries]
            assert [x["kind"] for x in batches] == ["foldbatch", "foldbatch"] and [x["n"] for x in batches] == [24, nq - 24], pl.entries
            _SEEN.update(("foldbatch:",))
            for r, d, (qw, qb) in zip(rows, data, queued):
                dtype, T, xs, w, b, dy, pre = d
                aw, ab, _, entries = _backward(*d, r[1][7], r[1][8], sink=True)           # the same layer, folded alone
                assert torch.equal(qw, aw) and torch.equal(qb, ab), r[0]
                ref, mag = ref_conv_with_mag(torch.cat(xs, -1), w, b, ONE, dy)
                assert_conv_close(qw, pre[0].double() + ref["dw"], mag["dw"] + pre[0].double().abs(), torch.float32, f"dW of {r[0]}", acc=True)
                assert_conv_close(qb, pre[1].double() + ref["db"], mag["db"] + pre[1].double().abs(), torch.float32, f"db of {r[0]}", acc=True)
    finally:
        _cleanup()


# =================================================================================================================================
# part 2: determinism
# =================================================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("row", [r for r in ROWS if r[2].get("M1_WG_DET", 1) == 1], ids=[r[0] for r in ROWS if r[2].get("M1_WG_DET", 1) == 1])
def test_plan_row_twice_is_bit_equal(dev, row):
    rid, key, sw, kern, edge = row
    try:
        with ops.config(M1_T3_MIN_BLOCKS=128), ops.config(**sw):
            d = _inputs(dev, row)
            a, b = (_backward(*d, key[7], key[8], sink=True) for _ in range(2))
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), rid
            c, e = (_backward(*d, key[7], key[8], sink=False) for _ in range(2))
            assert torch.equal(c[0], e[0]) and torch.equal(c[1], e[1]), rid
    finally:
        _cleanup()


@pytest.mark.gpu
def test_part_one_reached_every_required_plan(dev):
    not_run = [r for r in _ROW_IDS if r not in _RAN]
    assert not not_run, f"part 1 did not run (or failed) for: {not_run}"
    missing = [q for q in REQUIRED if not any(n.startswith(q) for n in _SEEN)]
    assert not missing, (missing, sorted(_SEEN))
