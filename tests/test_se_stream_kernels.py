"""The streaming kernels behind se_combine and the InstanceNorm backward -- se_combine_fwd_kernel, the SeBwdF / InBwdF reductions
(reduce.h) and se_combine_bwd_apply_kernel -- at the smallest shapes that reach every path of their loops:

* V = 3*5*8 = 120 voxels, N = 2: no multiple of a thread's stride, so the unrolled loops (two voxels / vectors in flight) end in their
  one-at-a-time tails;
* F = 8 (one channel group, cpad < 64), F = 24 in fp32 (F % 4 == 0: six groups of four), F = 12 in bf16 (F % 8 != 0: the VEC = 1
  kernels and the scalar reduction), F = 520 (65 channel groups > 64: the reduction folds its voxel rows through LDS);
* V = 3*9*19 = 513 at F = 8: the smallest volume m1_red_chunkV cuts into two chunks (per_block = 256 * 16 / 8 = 512 voxels);
* each with drop rate 0 and 0.5, the norm4 / identity-residual / duplicating entry points, the keep mask given and absent.

References, tolerances and input construction are those of test_ops_at_scale.py (its fp64 references are pinned to the CPU oracle in
its part 0; its docstring derives the tolerances): nothing is chosen here.  The masked and the Philox form of the backward, two runs of
one backward, and the forward's keep decisions against its mask bytes are compared bit for bit."""
import pytest
import torch

import test_ops_at_scale as S
from util import ops

BF, F32 = torch.bfloat16, torch.float32
V120, V513 = (3, 5, 8), (3, 9, 19)
# (dtype, F, spatial)
SHAPES = [(BF, 8, V120), (F32, 8, V120), (F32, 24, V120), (BF, 12, V120), (BF, 520, V120), (BF, 8, V513)]
IDS = ["bf16-F8", "fp32-F8", "fp32-F24", "bf16-F12", "bf16-F520", "bf16-F8-V513"]


def _vec(dtype):
    return 8 if dtype == BF else 4


def test_shapes_reach_the_paths_they_are_named_for():
    """Host mirrors of the launch formulas (no GPU): chunk counts and channel groups of the shapes above."""
    assert S.red_nchunks(120, 8, 2) == 1 and S.red_nchunks(512, 8, 2) == 1 and S.red_nchunks(513, 8, 2) == 2
    assert S.red_nchunks(120, 520, 2) > 1 and 520 // 8 == 65 and 12 % 8 != 0 and 24 % 4 == 0
    # 120 voxels over the 256 / cpad voxel sub-lanes of a block: an odd count of voxels per lane somewhere (the tail of the unroll by 2)
    for cg in (1, 2, 6):
        cpad = 1
        while cpad < cg:
            cpad <<= 1
        nvs = 256 // cpad
        assert any(len(range(vs, 120, nvs)) % 2 for vs in range(nvs))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["member", "ident", "dup"])
@pytest.mark.parametrize("rate", [0.0, 0.5])
@pytest.mark.parametrize("dtype,F_,V3", SHAPES, ids=IDS)
def test_se_combine_small_shapes_against_fp64(dev, dtype, F_, V3, rate, variant):
    if variant == "dup" and F_ % _vec(dtype):
        with pytest.raises(RuntimeError):           # (the duplicating form needs whole 16-byte channel vectors)
            S._se_case(dev, dtype, 2, V3, F_, variant, rate, seed=F_)
        return
    S._se_case(dev, dtype, 2, V3, F_, variant, rate, seed=F_ + len(variant))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,F_,V3", SHAPES, ids=IDS)
def test_instnorm_backward_small_shapes_against_fp64(dev, dtype, F_, V3):
    S._in_case(dev, dtype, (2, *V3, F_), 0.1, seed=F_)


def _se_inputs(dev, dtype, F_, V3, variant, seed):
    g = S._gen(dev, seed)
    shp = (2, *V3, F_)
    Fr = max(F_ // 8, 1)
    y3 = (S._randn(shp, g, dev, 1.3) + 0.4).to(dtype).requires_grad_(True)
    y4 = (S._randn(shp, g, dev, 1.1) - 0.3).to(dtype).requires_grad_(True)
    ps = [1 + 0.2 * S._randn((F_,), g, dev), 0.5 + 0.2 * S._randn((F_,), g, dev), 1 + 0.2 * S._randn((F_,), g, dev),
          0.6 + 0.2 * S._randn((F_,), g, dev), S._randn((1, 1, 1, F_, Fr), g, dev, 1.0 / F_ ** 0.5), 0.1 * S._randn((Fr,), g, dev),
          S._randn((1, 1, 1, Fr, F_), g, dev, 1.0 / Fr ** 0.5), 0.1 * S._randn((F_,), g, dev)]
    ps = [p.requires_grad_(True) for p in ps]
    if variant == "ident":
        ps[2] = ps[3] = None
    nout = 4 if variant == "dup" else 2
    dout = (0.2 + S._randn((nout, *V3, F_), g, dev)).to(dtype)
    return y3, y4, ps, dout


def _fwd(y3, y4, ps, rate, rng, variant):
    return ops.se_combine(y3, y4, *ps, rate, rng if rate > 0 else None, 7, dup=variant == "dup")


def _bwd(out, dout, leaves):
    """One backward of `out`; returns clones of the leaves' gradients and clears them."""
    out.backward(dout, retain_graph=True)
    got = [t.grad.clone() for t in leaves]
    for t in leaves:
        t.grad = None
    return got


MASKED = [(F_, V3, v) for F_, V3 in ((8, V120), (520, V120), (8, V513)) for v in ("member", "ident", "dup")]


@pytest.mark.gpu
@pytest.mark.parametrize("F_,V3,variant", MASKED)
def test_masked_and_philox_backward_agree_bit_for_bit(dev, F_, V3, variant):
    """bf16, F % 8 == 0, rate 0.5: the forward writes one keep byte per 16-byte vector.  (a) the bytes are the forward's own keep
    decisions; (b) the backward that reads them and the backward that re-runs Philox (mask absent) give the same dy3 / dy4, bit for
    bit -- and the same parameter gradients, their reductions being the same arithmetic in the same order; (c) a second run of either
    backward repeats the first (fixed summation order)."""
    y3, y4, ps, dout = _se_inputs(dev, BF, F_, V3, variant, seed=F_ + 3)
    rng = torch.tensor([977, 4], dtype=torch.int64, device=dev)
    leaves = [y3, y4] + [p for p in ps if p is not None]
    out = _fwd(y3, y4, ps, 0.5, rng, variant)
    mask = out.grad_fn.mask
    assert mask is not None and mask.numel() == out.numel() // 8
    # (a) bit (idx & 7) of byte (idx >> 3) against out != 0, wherever the output without dropout is not 0 itself
    with torch.no_grad():
        out0 = _fwd(y3.detach(), y4.detach(), [None if p is None else p.detach() for p in ps], 0.0, None, variant)
    bits = ((mask.to(torch.int32).unsqueeze(1) >> torch.arange(8, device=dev, dtype=torch.int32)) & 1).bool().reshape(out.shape)
    live = out0 != 0
    assert int(live.sum()) > 0.99 * out.numel()
    assert torch.equal((out != 0)[live], bits[live])
    assert 0.4 < float(bits.float().mean()) < 0.6
    assert torch.equal(out[live & bits].float(), (out0[live & bits].float() * 2.0).to(BF).float())
    # (b), (c)
    m1 = _bwd(out, dout, leaves)
    m2 = _bwd(out, dout, leaves)
    out.grad_fn.mask = None                          # mask absent: the backward draws the keep decisions from the stream again
    p1 = _bwd(out, dout, leaves)
    p2 = _bwd(out, dout, leaves)
    for a, b, c, d in zip(m1, m2, p1, p2):
        assert torch.equal(a, b) and torch.equal(c, d)
    assert torch.equal(m1[0], p1[0]) and torch.equal(m1[1], p1[1])
    for a, c in zip(m1[2:], p1[2:]):
        assert torch.equal(a, c)
    ops.flush_deferred()


# (the duplicating form needs whole 16-byte channel vectors: no bf16 F = 12)
DET = [(dt, F_, V3, v) for dt, F_, V3 in SHAPES for v in ("member", "ident", "dup") if not (v == "dup" and F_ % _vec(dt))]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,F_,V3,variant", DET)
def test_backward_is_deterministic(dev, dtype, F_, V3, variant):
    """The same backward twice (SE combine at rate 0.5, InstanceNorm): every gradient repeats bit for bit."""
    y3, y4, ps, dout = _se_inputs(dev, dtype, F_, V3, variant, seed=F_ + 11)
    rng = torch.tensor([31, 2], dtype=torch.int64, device=dev)
    leaves = [y3, y4] + [p for p in ps if p is not None]
    out = _fwd(y3, y4, ps, 0.5, rng, variant)
    for a, b in zip(_bwd(out, dout, leaves), _bwd(out, dout, leaves)):
        assert torch.equal(a, b)
    if variant == "member":
        y = ops.instnorm_act(y3, ps[0], ps[1], 0.1)
        dy = dout[:2]
        for a, b in zip(_bwd(y, dy, [y3, ps[0], ps[1]]), _bwd(y, dy, [y3, ps[0], ps[1]])):
            assert torch.equal(a, b)
    ops.flush_deferred()
