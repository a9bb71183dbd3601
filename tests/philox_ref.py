"""Host restatement of the in-kernel random streams (numpy only; a helper, not a test module).

``philox4x32_10`` is Philox-4x32 with ten rounds as Salmon, Moraes, Dror and Shaw define it ("Parallel random numbers: as easy as
1, 2, 3", SC'11, section 3.3 / the Random123 library): one round maps the counter (c0, c1, c2, c3) under the key (k0, k1) to

    (hi(M1 * c2) ^ c1 ^ k0,  lo(M1 * c2),  hi(M0 * c0) ^ c3 ^ k1,  lo(M0 * c0)),    M0 = 0xD2511F53, M1 = 0xCD9E8D57

and the key is bumped by the Weyl constants (0x9E3779B9, 0xBB67AE85) between rounds.  tests/test_random_streams.py checks it
against the three published Random123 known-answer vectors.

On top of it, the project's derivations as the kernels document them (csrc/common.h, latent.hip, augment.hip, include/m1hip.h):

    key      = (seed + id * 0x9E3779B97F4A7C15) mod 2^64            -> (k0, k1) = (low, high) word
    counter  = a 64-bit position -> (c0, c1) = (low, high) word;  c2, c3 = 0x243F6A88, 0x85A308D3 (fixed)
    dropout  : element e = (step << 36) + first + i  reads word  e & 3  of counter  e >> 2;  u = float32(w >> 8) * 2^-24;  keep = u >= rate
    latent   : element i reads counter (step << 36) + i;  u1 = (float32(x >> 8) + 0.5) * 2^-24,  u2 = float32(y >> 8) * 2^-24;
               eps = sqrt(-2 ln u1) * cos(2 pi u2)
    noise    : voxel v reads counter (step << 36) + v;  (x, y) give cos / sin, (z, w) give cos / sin: four normals
    table    : draw k of sample n reads word .x of counter (step << 36) + 64 n + k
"""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
C2, C3 = 0x243F6A88, 0x85A308D3          # the counter words the project fixes
GOLDEN = 0x9E3779B97F4A7C15
MASK32, MASK64 = 0xFFFFFFFF, (1 << 64) - 1
TWO_PI_F32 = np.float32(6.28318530718)
F32 = np.float32
INV24, INV23 = F32(2.0 ** -24), F32(2.0 ** -23)

# m1_aug_params_t (include/m1hip.h) and its stage bits
AUG_DTYPE = np.dtype([("fired", "<u4"), ("gamma_ch", "<u4"), ("poor_ch", "<u4"), ("scale", "<i4"), ("rot_pad", "<i4"),
                      ("rot", "<f4", (6,)), ("tr", "<i4", (4,)), ("cs", "<i4", (4,)), ("cs_channel", "<i4"), ("gamma", "<f4"),
                      ("noise_std", "<f4"), ("angle_deg", "<f4"), ("_pad", "<i4")])
MASTER, ZOOM, FLIP, ROTATE, TRANSLATE, CSHIFT, GAMMA, POOR, NOISE = 1, 2, 4, 8, 16, 32, 64, 128, 256
AUG_STRIDE = 64                           # counter positions reserved per sample of the table


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds over arrays (or scalars) of 32-bit words; returns four uint32 arrays."""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & np.uint64(MASK32) for v in (c0, c1, c2, c3)]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(k0) & MASK32, int(k1) & MASK32
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)                    # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK32)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK32)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return tuple(v.astype(np.uint32) for v in c)


def key(seed, ident):
    """The 64-bit Philox key of consumer ``ident`` under ``seed`` (both taken mod 2^64, as the device's uint64 arithmetic does)."""
    return (int(seed) + int(ident) * GOLDEN) & MASK64


def words(seed, ident, counter):
    """(n, 4) uint32: the four output words of every 64-bit ``counter`` under ``key(seed, ident)``."""
    k = key(seed, ident)
    ctr = np.atleast_1d(np.asarray(counter, dtype=np.uint64))
    out = philox4x32_10(ctr & np.uint64(MASK32), ctr >> np.uint64(32), C2, C3, k & MASK32, k >> 32)
    return np.stack(out, axis=-1)


def _positions(step, first, n):
    base = ((int(step) << 36) + int(first)) & MASK64
    assert base + n <= MASK64, "the restatement does not wrap inside one tensor"
    return base


def keep_uniform(seed, step, layer_id, n, first=0):
    """float32 uniforms in [0, 1) of elements first .. first + n - 1 of a dropout stream."""
    e0 = _positions(step, first, n)
    b0, b1 = e0 >> 2, (e0 + n - 1) >> 2
    w = words(seed, layer_id, np.arange(b0, b1 + 1, dtype=np.uint64)).reshape(-1)
    w = w[e0 - 4 * b0: e0 - 4 * b0 + n]
    return (w >> np.uint32(8)).astype(np.float32) * INV24


def keep_mask(seed, step, layer_id, n, rate, first=0):
    """bool[n]: element i is kept iff its uniform is >= rate, compared in float32."""
    return keep_uniform(seed, step, layer_id, n, first) >= F32(rate)


def _box_muller(a, b, dtype):
    """(r cos t, r sin t) from the words ``a`` (radius) and ``b`` (angle): float32 uniforms, then ``dtype`` arithmetic."""
    u1 = ((a >> np.uint32(8)).astype(np.float32) + F32(0.5)) * INV24
    u2 = (b >> np.uint32(8)).astype(np.float32) * INV24
    two_pi = TWO_PI_F32.astype(dtype)
    r = np.sqrt(dtype(-2.0) * np.log(u1.astype(dtype)))
    t = two_pi * u2.astype(dtype)
    return r * np.cos(t), r * np.sin(t)


def normal(seed, step, stream_id, n, dtype=np.float64):
    """The N(0, 1) draw of elements 0 .. n - 1 of a latent stream (``dtype=np.float32``: the same formula in single precision)."""
    w = words(seed, stream_id, np.uint64(_positions(step, 0, n)) + np.arange(n, dtype=np.uint64))
    return _box_muller(w[:, 0], w[:, 1], dtype)[0]


def noise4(seed, step, stream_id, n_voxels, dtype=np.float64):
    """(n_voxels, 4): the four normals of every voxel of the augmentation noise (image channel c receives column c)."""
    w = words(seed, stream_id, np.uint64(_positions(step, 0, n_voxels)) + np.arange(n_voxels, dtype=np.uint64))
    z0, z1 = _box_muller(w[:, 0], w[:, 1], dtype)
    z2, z3 = _box_muller(w[:, 2], w[:, 3], dtype)
    return np.stack([z0, z1, z2, z3], axis=-1)


def rotation_pad(H, W):
    return int(math.ceil((math.sqrt(H * H + W * W) - min(H, W)) / 2.0))


def _ceil_f32(v):
    return int(math.ceil(float(F32(v))))


def aug_table(seed, step, stream_id, N, hyper, H, W, nimg, lesion):
    """The table m1_aug_draw fills for ``hyper`` = (prob, tx_prob, translate, rotation, hflip, zoom, noise, chan_shift, poor_scan,
    gamma_lo, gamma_hi), in the draw order of aug_draw_kernel.  Returns (records[N] of AUG_DTYPE, rot64[N, 6], used[N]):
    ``rot`` of the records and ``rot64`` hold the six rotation coefficients evaluated in float64 from the float32 angle (the
    kernel's go through cosf / sinf), ``used`` the number of words each sample consumed."""
    prob, tx, tr, rot, flip, zoom, noise, cs, poor, g0, g1 = (float(v) for v in hyper)
    f = F32
    gamma_on = (g0 + g1) != 0.0
    prob, tx, rot_deg, noise_hi, g0, g1 = f(prob), f(tx), f(rot), f(noise), f(g0), f(g1)
    zoom_on, zoom_hi = zoom != 0.0, _ceil_f32(H * zoom)
    flip_on, rot_on, tr_on = flip == 1.0, rot != 0.0, tr != 0.0
    tr_hi_h, tr_hi_w = _ceil_f32(H * tr), _ceil_f32(W * tr)
    cs_on, cs_hi_h, cs_hi_w = bool(lesion) and cs != 0.0, _ceil_f32(H * cs), _ceil_f32(W * cs)
    poor_on, noise_on = poor != 0.0, noise != 0.0
    pad = rotation_pad(H, W)
    base = _positions(step, 0, AUG_STRIDE * N)
    ctr = np.uint64(base) + np.arange(AUG_STRIDE * N, dtype=np.uint64)
    wx = words(seed, stream_id, ctr)[:, 0].reshape(N, AUG_STRIDE)
    recs = np.zeros(N, dtype=AUG_DTYPE)
    rot64 = np.zeros((N, 6), dtype=np.float64)
    used = np.zeros(N, dtype=np.int64)
    for n in range(N):
        k = [0]

        def word():
            w = int(wx[n, k[0]]) if k[0] < AUG_STRIDE else None          # (past the stride: the caller's assertion on `used` fails)
            k[0] += 1
            return 0 if w is None else w

        def uni():
            return f(word() >> 9) * INV23

        def between(lo, hi):
            return lo + word() % (hi - lo)

        def ufl(lo, hi):
            return f(f(uni() * f(hi - lo)) + lo)
        r = recs[n]
        r["scale"], r["rot_pad"], r["gamma"] = H, pad, 1.0
        r64 = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0])
        fired = 0
        if uni() > f(f(1.0) - prob):
            fired |= MASTER
            if zoom_on:
                if uni() > tx:
                    fired |= ZOOM
                r["scale"] = between(H, zoom_hi)
            if flip_on and uni() > f(0.5):
                fired |= FLIP
            if rot_on:
                if uni() > tx:
                    fired |= ROTATE
                ang = ufl(-rot_deg, rot_deg)
                r["angle_deg"] = ang
                rad = float(f(f(ang * f(math.pi)) / f(180.0)))
                c, s = math.cos(rad), math.sin(rad)
                w1, h1 = float(W + 2 * pad - 1), float(H + 2 * pad - 1)
                r64 = np.array([c, -s, (w1 - (c * w1 - s * h1)) / 2.0, s, c, (h1 - (s * w1 + c * h1)) / 2.0])
            if tr_on:
                if uni() > tx:
                    fired |= TRANSLATE
                r["tr"] = [between(0, tr_hi_h), between(0, tr_hi_h), between(0, tr_hi_w), between(0, tr_hi_w)]
            if cs_on:
                on = uni() > tx
                r["cs"] = [between(0, cs_hi_h), between(0, cs_hi_h), between(0, cs_hi_w), between(0, cs_hi_w)]
                if on:
                    fired |= CSHIFT
                    r["cs_channel"] = between(0, 3)
            if gamma_on:
                on = uni() > tx
                r["gamma"] = ufl(g0, g1)
                if on:
                    fired |= GAMMA
                    for ch in range(nimg):
                        if uni() > f(0.5):
                            r["gamma_ch"] |= 1 << ch
            if poor_on and uni() > tx:
                fired |= POOR
                for ch in range(nimg):
                    if uni() > f(0.5):
                        r["poor_ch"] |= 1 << ch
            if noise_on:
                if uni() > tx:
                    fired |= NOISE
                r["noise_std"] = ufl(f(0.0), noise_hi)
        r["fired"] = fired
        r["rot"] = r64.astype(np.float32)
        rot64[n] = r64
        used[n] = k[0]
    return recs, rot64, used


# ---- the layout of the streams (the id audit of test_random_streams.py) ----------------------------------------------------------
def counter_range(kind, step, numel):
    """[lo, hi) of the Philox counters a consumer touches at ``step``: ``kind`` 'dropout' (four elements per counter), 'latent' /
    'noise' (one per element) or 'table' (``numel`` = samples, 64 counters each)."""
    base = (int(step) << 36) & MASK64
    if kind == "dropout":
        return base >> 2, (base >> 2) + (int(numel) + 3) // 4
    if kind == "table":
        return base, base + AUG_STRIDE * int(numel)
    return base, base + int(numel)


def collisions(consumers, steps):
    """``consumers``: (name, kind, seed, id, numel).  Returns every (a, step, b, step) that shares a key AND a counter, over all
    pairs of consumers and of ``steps`` (a consumer against itself at two different steps included) -- what the layout must never
    produce.  Two different consumers under one key always collide at step 0 (both ranges start at counter 0), so for them this is
    the demand that the keys differ; for a consumer against itself it is the demand that one step's range ends before the next
    step's begins."""
    by_key = {}
    for c in consumers:
        by_key.setdefault(key(c[2], c[3]), []).append(c)
    bad = []
    for group in by_key.values():
        for i, a in enumerate(group):
            for b in group[i:]:
                for s in steps:
                    for t in steps:
                        if a is b and s >= t:
                            continue
                        x, y = counter_range(a[1], s, a[4]), counter_range(b[1], t, b[4])
                        if x[0] < y[1] and y[0] < x[1]:
                            bad.append((a[0], s, b[0], t))
    return bad
