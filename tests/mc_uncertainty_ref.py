"""The numpy restatement of csrc/mc.hip's uncertainty accumulators and maps (m1_mc_accum_u, m1_mc_finish_u) and their error bound.
It extends ``r_softmax`` / ``r_accum`` / ``r_finish`` of tests/test_mc_inference.py in the kernels' operation order; ``vt`` = np.float64
gives the reference, np.float32 the restatement's own error e32.

Per voxel, nats, N draws p_1..p_N:
    expected_entropy = (1/N) sum_r H(p_r),  H(p) = -sum_c p_c ln p_c (0 ln 0 = 0)
    mutual_info      = max(entropy - expected_entropy, 0)
    variance_c       = max((1/N) sum_r p_r,c^2 - mean_c^2, 0)

The bound is the project's form, |got - ref64| <= max(k * 2^-24 * scale, 4 * e32), e32 from this restatement in fp32 values and never
from the kernel.  k counts fp32 roundings, each at most 2^-24 relative to a quantity that ``scale`` bounds, the way test_mc_inference.py
counts them (K_P = nc + 7 behind one probability, S = 1 + ln nc; expf / logf are 1 ulp = two roundings):

  per-draw H, scale S:          d(p ln p) = (ln p + 1) dp and sum_c |p_c (ln p_c + 1)| <= 1 + H <= S carry the K_P of the
                                probabilities; then logf (2), the product, and nc - 1 subtractions of partial sums <= ln nc
                                                                                                        k = K_P + nc + 2
  sum_h of n draws, scale n*S:  every H above plus n - 1 additions of partial sums <= n ln nc              k = K_P + nc + 2 + n - 1
  expected_entropy, scale S:    plus the division                                                         k = K_P + nc + 2 + n
  mutual_info, scale S:         the two entropies' errors add (k(entropy) = K_P + n + nc + 2 from test_mc_inference.py), plus the
                                subtraction of two values <= ln nc; the clamp moves a value towards the reference, which is >= 0
                                                                                                        k = 2 (K_P + n + nc + 2) + 1
  sum_pp of n draws, scale n:   p^2 carries twice the K_P of p, plus the product: 2 K_P + 1 per term <= 1; n - 1 additions of
                                partial sums <= n                                                         k = 2 K_P + n
  variance, scale 1:            sum_pp / n (k(sum_pp) + 1, a value <= 1), mean^2 (twice k(mean) = K_P + n, plus the product, a value
                                <= 1), the subtraction of the two                                         k = (2 K_P + n + 1) + (2 (K_P + n) + 1) + 1

``from_samples=True`` is the count for maps computed from GIVEN fp32 probabilities (the model-level tests restate the returned
samples, which are then exact inputs): the same formulas with K_P = 0."""
import math

import numpy as np

from test_mc_inference import k_p, r_accum, r_finish

U = 2.0 ** -24
OUTPUTS = ("expected_entropy", "mutual_info", "variance")


def r_entropy(p, vt):
    """H of every draw in mc_finish_item's order: r_finish with n = 1 (the division by 1 is exact)."""
    return r_finish(p, 1, vt)[1]


def r_fold_u(draws, vt):
    """draws: list, one (R, B, V, nc) array of probabilities per pass -> the running (sum_h (B, V), sum_pp (B, V, nc)) after each pass:
    the replicas of a pass added in replica order, then old + acc, exactly as sum_p in ``r_accum``."""
    out, th, tq = [], None, None
    for p in draws:
        p = p.astype(vt)
        h, q = r_entropy(p, vt), p * p
        ah, aq = h[0], q[0]
        for r in range(1, p.shape[0]):
            ah, aq = ah + h[r], aq + q[r]
        th, tq = (ah, aq) if th is None else (th + ah, tq + aq)
        out.append((th, tq))
    return out


def r_accum_u(passes, R, vt):
    """passes: list of (R*B, V, nc) logits -> ([(sum_p, sum_h, sum_pp) after each pass], per-draw probabilities per pass)."""
    sums, draws = r_accum(passes, R, vt)
    return [(s, h, q) for s, (h, q) in zip(sums, r_fold_u(draws, vt))], draws


def r_finish_u(sum_p, sum_h, sum_pp, n, vt, *, var_div=None, log_base=None, mi_from_mean=False, ee_div=True):
    """The five maps.  The keyword switches build the WRONG restatements the CPU tests must see break the bound."""
    mean, ent = r_finish(sum_p, n, vt)
    ee = sum_h.astype(vt) / vt(n) if ee_div else sum_h.astype(vt)
    if log_base is not None:
        ent, ee = ent / vt(math.log(log_base)), ee / vt(math.log(log_base))
    mi = ent - (r_entropy(mean, vt) if mi_from_mean else ee)
    mi = np.where(mi < 0, vt(0), mi)                                       # (a NaN stays a NaN, as x < 0 ? 0 : x)
    var = sum_pp.astype(vt) / vt(n if var_div is None else var_div) - mean * mean
    var = np.where(var < 0, vt(0), var)
    return {"mean": mean, "entropy": ent, "expected_entropy": ee, "mutual_info": mi, "variance": var}


def k_counts(nc, n, from_samples=False):
    kp = 0 if from_samples else k_p(nc)
    S = 1 + math.log(nc)
    k_ent = kp + n + nc + 2
    return {"draw_h": (kp + nc + 2, S), "sum_h": (kp + nc + 2 + n - 1, n * S), "expected_entropy": (kp + nc + 2 + n, S),
            "mutual_info": (2 * k_ent + 1, S), "sum_pp": (2 * kp + n, n), "variance": ((2 * kp + n + 1) + (2 * (kp + n) + 1) + 1, 1.0),
            "sum_p": (kp + n - 1, n), "mean": (kp + n, 1.0), "entropy": (k_ent, S)}


def first_term(nc, n, what, from_samples=False):
    k, scale = k_counts(nc, n, from_samples)[what]
    return k * U * scale


def bound(nc, n, what, e32, from_samples=False):
    return max(first_term(nc, n, what, from_samples), 4 * e32)


def _err(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max())


def refs_from_draws(draws, n):
    """fp64 maps and the fp32 restatement's error of each, from given per-pass probabilities (list of (R, B, V, nc))."""
    out = {}
    for vt in (np.float64, np.float32):
        sums = None
        for p in draws:                                                     # sum_p in r_accum's association
            p = p.astype(vt)
            a = p[0]
            for r in range(1, p.shape[0]):
                a = a + p[r]
            sums = a if sums is None else sums + a
        h, q = r_fold_u(draws, vt)[-1]
        out[vt] = r_finish_u(sums, h, q, n, vt)
    return out[np.float64], {k: _err(out[np.float32][k], out[np.float64][k]) for k in out[np.float64]}


def case_refs_u(logits, R):
    """logits: list of (R*B, V, nc) float32 arrays.  -> (s64: [(sum_p, sum_h, sum_pp)] per pass, d64: draws per pass, maps64: the five
    maps after the last pass, e32: {"sum_p" / "sum_h" / "sum_pp": [per pass], map name: float})."""
    s64, d64 = r_accum_u(logits, R, np.float64)
    s32, _ = r_accum_u(logits, R, np.float32)
    n = R * len(logits)
    m64, m32 = r_finish_u(*s64[-1], n, np.float64), r_finish_u(*s32[-1], n, np.float32)
    e32 = {name: [_err(a[i], b[i]) for a, b in zip(s32, s64)] for i, name in enumerate(("sum_p", "sum_h", "sum_pp"))}
    e32.update({k: _err(m32[k], m64[k]) for k in m64})
    return s64, d64, m64, e32
