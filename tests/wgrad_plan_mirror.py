"""wg_plan_of: a Python restatement of how the library plans a weight gradient (no GPU, no library call).

It restates, from the sources named in brackets, for one call of m1_conv3d_wgrad / m1_convT3d_wgrad:
* the ladder and its gates [csrc/dispatch.hip: wgrad_common, WG_LADDER, tf_wanted, equal_run, stem_wanted, wgrad_spec, wgrad_rx_bytes;
  t3_plan, ts_plan, m1_pwf_wgrad_supported, tf_plan, tap_plan, m1_mfma_wgrad_supported in csrc/wgrad_*.hip];
* the K-tile geometry and the copy planner with each launcher's rule [csrc/wgrad_fold.h: m1_wg_kws, m1_wg_ktiles, m1_wg_copies];
* each launcher's splits, stages and grid [m1_t3_wgrad, m1_t3s_wgrad, m1_pwf_wgrad, tf_wgrad_launch, m1_tap_wgrad, launch_wg];
* the fold-kernel choice [csrc/wgrad_fold.hip: m1_wg_rx_finish].

The result is the list of plan-log entries (include/m1hip.h: m1_debug_plans) the call must leave, parsed: tests/test_wgrad_plans.py
compares it with the log of the real call, and with the kernel-name tables the suite already pins."""
import re
from types import SimpleNamespace as NS

ERR_UNSUPPORTED, ERR_WORKSPACE = -2, -4
MAX_COPIES = 512
SWITCHES = {"M1_T3_BLOCKS": 256, "M1_T3_MIN_BLOCKS": 128, "M1_T3_STAGES": 0, "M1_T3S_BLOCKS": 256, "M1_PWF_BLOCKS": 256,
            "M1_TF_SPLIT": 0, "M1_TF_NKS4": 2, "M1_TF_MULTI": 1, "M1_TF_MAXC": 128, "M1_TF_STAGES": 0, "M1_WG_BLOCKS": 512,
            "M1_WG_TAP_BLOCKS": 512, "M1_WG_TAP_STAGES": 0, "M1_WG_RX_MB": 64, "M1_WG_XCD": 1, "M1_WG_FLOOR": 1, "M1_WG_DET": 1}


def _cdiv(a, b):
    return -(-a // b)


def _align256(b):
    return _cdiv(b, 256) * 256


def same_pad(n, k, s):
    o = _cdiv(n, s)
    return o, max((o - 1) * s + k - n, 0) // 2


def rx_bytes(members, cout, k, sw):
    """wgrad_rx_bytes: the partial-copy region of ONE member.  Never fewer than two copies of the widest member's block."""
    taps = k[0] * k[1] * k[2]
    cmax = max(8, *members)
    stride = taps * cmax * cout + max(cmax, cout)
    b = min(MAX_COPIES * stride * 4, sw["M1_WG_RX_MB"] << 20)
    return _align256(max(b, 2 * stride * 4))


def member_spec(N, dims, members, cout, k, s, f32, T, i, rx_floats, bias):
    """wgrad_spec for member i.  A: the operand read at the shifted (strided) positions, B: the one whose voxels are the K-tiles."""
    if not T:
        o = [same_pad(n, kk, st) for n, kk, st in zip(dims, k, s)]
        A, B, CA, CB = dims, tuple(v[0] for v in o), members[i], cout
        pads = tuple(v[1] for v in o)
    else:
        A, B, CA, CB = tuple(n * st for n, st in zip(dims, s)), dims, cout, members[i]
        pads = tuple(max(kk - st, 0) // 2 for kk, st in zip(k, s))
    return NS(N=N, CA=CA, CB=CB, AD=A[0], AH=A[1], AW=A[2], BD=B[0], BH=B[1], BW=B[2], kd=k[0], kh=k[1], kw=k[2], sd=s[0], sh=s[1], sw=s[2],
              pd=pads[0], ph=pads[1], pw=pads[2], f32=f32, rx_floats=rx_floats, bsum=bool(bias and not T and i == 0))


# ---- wgrad_fold.h ----------------------------------------------------------------------------------------------------------------
def wg_kws(BW, other):
    return 32 if BW % 32 == 0 else 16 if BW % 16 == 0 else 8 if BW % 8 == 0 else other


def wg_ktiles(g, kt, kws, min_tiles):
    TH = kt // kws
    tw, th = g.BW // kws, _cdiv(g.BH, TH)
    nt = g.N * g.BD * th * tw
    return NS(KWs=kws, TH=TH, tiles_w=tw, tiles_h=th, ntiles=nt) if (1 << 30) > nt >= min_tiles else None


def wg_vox32(g):
    lim = (1 << 31) - (1 << 20)
    return g.N * g.AD * g.AH * g.AW < lim and g.N * g.BD * g.BH * g.BW < lim


def wg_copies(g, taps, want, ntiles, rule, use_rx=True):
    """m1_wg_copies.  rule = (min_ktiles, max_copies, max_bytes, short) with short in ('error', 'fallback')."""
    min_kt, max_copies, max_bytes, short = rule
    stride = taps * g.CA * g.CB + g.CB
    n = want
    if min_kt and n > ntiles // min_kt:
        n = ntiles // min_kt
    if max_copies and n > max_copies:
        n = max_copies
    if max_bytes and n * stride * 4 > max_bytes:
        n = max_bytes // (stride * 4)
    fit = g.rx_floats // stride
    c = NS(stride=stride, nsplit=0, Rx=False, rc=0, fit=fit)
    if short == "error":
        if fit < 1:
            c.rc = ERR_WORKSPACE
            return c
        n = min(n, fit)
        if n < 1:
            if max_bytes:
                c.rc = ERR_UNSUPPORTED
                return c
            n = 1
        c.Rx = True
    else:
        n = max(n, 1)
        if use_rx and n >= 2 and fit >= 2:
            n = min(n, fit)
            c.Rx = True
    c.nsplit = n
    return c


def fold_of(ncopies, g, queued):
    """m1_wg_rx_finish: (mode, n, nb, EL) of the fold of ``ncopies`` copies of this member's block."""
    nb = g.CB if g.bsum else 0
    n = g.kd * g.kh * g.kw * g.CA * g.CB + nb
    EL = 32
    if ncopies <= 16 and g.CB % 4 == 0 and n >= (1 << 16):
        mode = "vec"
    elif g.CB % 4 == 0 and n - nb >= (1 << 15):
        mode = "wide"
    else:
        mode = "generic"
        while EL > 4 and n // EL < 128:
            EL >>= 1
    return dict(kind="fold", mode=mode, copies=ncopies, n=n, nb=nb, el=EL, when="queued" if queued else "now")


def _wg(name, tiles, want, splits, c, rx, stages, grid):
    return dict(kind="wg", name=name, tiles=tiles, want=want, splits=splits, fit=c.fit, rx=int(rx), stages=stages, grid=tuple(grid))


# ---- wgrad_t3.hip ----------------------------------------------------------------------------------------------------------------
def t3_plan(g):
    if g.CA < 64 or g.CB < 64 or g.CA % 64 or g.CB % 64:
        return None
    if not (g.kh == 3 and g.kw == 3 and g.kd in (1, 3)):
        return None
    s1 = (g.sd, g.sh, g.sw) == (1, 1, 1)
    s2 = g.sh == 2 and g.sw == 2 and g.sd in (1, 2) and g.ph == 0 and g.pw == 0
    if not s1 and not s2:
        return None
    if g.f32 and (not s1 or g.BW % 8):
        return None
    if s2 and g.CB % 128:
        return None
    if g.BW % 4 or g.BW < 8:
        return None
    esz = 4 if g.f32 else 2
    if (g.AH + 4) * g.AW * g.CA * esz >= (1 << 31) - 4096 or (g.BH + 4) * g.BW * g.CB * esz >= (1 << 31) - 4096:
        return None
    kws = 0
    for c in (32, 16, 8):
        if g.f32 and c == 32 and g.CB % 128:
            continue
        if g.BW % c == 0:
            kws = c
            break
    if not kws:
        if g.BW <= 32:
            kws = g.BW
        else:
            for c in range(28, 7, -4):
                if g.BW % c == 0:
                    kws = c
                    break
    if not kws:
        return None
    p = wg_ktiles(g, 64, kws, 8)
    if p is None or p.TH + 2 > 255 or p.KWs + 2 > 255:
        return None
    nA = _cdiv((p.TH + 2) * (p.KWs + 2), 8) if s1 else _cdiv(4 * (p.TH + 1) * (p.KWs + 2), 8)
    if not g.f32 and nA > (18 if s1 else 60):
        return None
    if g.f32 and kws not in (8, 16, 32):
        return None
    if not (2 * p.TH + 1 <= 255 and 2 * p.KWs + 3 <= 255):
        return None
    p.s2 = s2
    return p


def t3_run(g, sw, nmem):
    p = t3_plan(g)
    if p is None or nmem < 1 or nmem > 6:
        return ERR_UNSUPPORTED
    nunits = g.CA // 64 * nmem
    bigb = g.CB % 128 == 0
    if not bigb and nunits < 2:
        return ERR_UNSUPPORTED
    gx, gzu = (g.CB // 128, nunits) if bigb else (g.CB // 64, (nunits + 1) // 2)
    per_split = gx * gzu * g.kd
    want = sw["M1_T3_BLOCKS"] // per_split
    c = wg_copies(g, g.kd * 9, want, p.ntiles, (8, 0, 0, "error"))
    if c.rc:
        return c.rc
    if c.nsplit * per_split < sw["M1_T3_MIN_BLOCKS"]:
        return ERR_UNSUPPORTED
    if g.f32:
        nA = _cdiv((p.TH + 2) * (p.KWs + 2), 4)
        stage = ((nA + 32) if bigb else (2 * nA + 16)) * 1024
    else:
        nA = _cdiv((p.TH + 2) * (p.KWs + 2), 8) if not p.s2 else _cdiv(4 * (p.TH + 1) * (p.KWs + 2), 8)
        stage = ((nA + 16) if bigb else (2 * nA + 8)) * 1024
    tpb = _cdiv(p.ntiles, c.nsplit)
    S = 3 if g.f32 else 4
    if 2 <= sw["M1_T3_STAGES"] <= 5:
        S = sw["M1_T3_STAGES"]
    if g.f32 and S > 3:
        S = 3
    while S >= 2 and S * stage + 1024 + (tpb + S) * 32 > 160 * 1024:
        S -= 1
    if S < 2:
        return ERR_UNSUPPORTED
    name = ("wgrad_t3f:kws%d:big%d" if g.f32 else "wgrad_t3:s2:kws%d:big%d" if p.s2 else "wgrad_t3:kws%d:big%d") % (p.KWs, bigb)
    out = [_wg(name, p.ntiles, want, c.nsplit, c, True, S, (gx, c.nsplit, gzu * g.kd))]
    for m in range(nmem):
        gm = NS(**vars(g))
        gm.bsum = g.bsum and m == 0
        out.append(("fold", c.nsplit, gm))
    p.tpb = tpb
    return out, p


# ---- wgrad_t3s.hip ---------------------------------------------------------------------------------------------------------------
def ts_plan(g):
    if not g.f32 or g.CA % 4 or g.CB % 4 or g.CA < 4 or g.CB < 4:
        return None
    if not (g.kh == 3 and g.kw == 3 and g.kd in (1, 3)):
        return None
    s1 = (g.sd, g.sh, g.sw) == (1, 1, 1)
    s2 = g.sh == 2 and g.sw == 2 and g.sd in (1, 2) and g.ph == 0 and g.pw == 0
    if (not s1 and not s2) or g.BW % 8:
        return None
    TLh = 16 if (g.CA <= 16 or g.CB <= 16) else 32
    nau, nbu = _cdiv(g.CA, TLh), _cdiv(g.CB, TLh)
    if nau * nbu > (128 if s2 else 32):
        return None
    if (g.AH + 4) * g.AW * g.CA * 4 >= (1 << 31) - 4096 or (g.BH + 20) * g.BW * g.CB * 4 >= (1 << 31) - 4096:
        return None
    p = wg_ktiles(g, 64 if s2 else 128, wg_kws(g.BW, 8), 4)
    if p is None:
        return None
    p.s2, p.TLh, p.nau, p.nbu = s2, TLh, nau, nbu
    return p


def ts_run(g, sw):
    p = ts_plan(g)
    if p is None:
        return ERR_UNSUPPORTED
    per_split = p.nbu * p.nau * g.kd
    want = sw["M1_T3S_BLOCKS"] // per_split
    c = wg_copies(g, g.kd * 9, want, p.ntiles, (4, MAX_COPIES, 0, "error"))
    if c.rc:
        return c.rc
    KT, kws = (64 if p.s2 else 128), p.KWs
    TH = KT // kws
    arows = (2 * TH + 1) * (2 * kws + 2) if p.s2 else (TH + 2) * (kws + 2)
    stage = (_cdiv(arows, 8) + KT // 8) * 1024
    tpb = _cdiv(p.ntiles, c.nsplit)
    red = 9 * 3 * (16 if p.TLh == 32 else 4) * 64 * 4
    S = 3
    while S >= 2 and max(S * stage + 1024, red) + (tpb + S) * 32 + 1024 > 160 * 1024:
        S -= 1
    if S < 2:
        return ERR_UNSUPPORTED
    p.tpb = tpb
    return [_wg("wgrad_t3s", p.ntiles, want, c.nsplit, c, True, S, (p.nbu, c.nsplit, p.nau * g.kd)), ("fold", c.nsplit, g)], p


def pwf_ok(g):
    if not g.f32 or (g.kd, g.kh, g.kw, g.sd, g.sh, g.sw) != (1,) * 6:
        return False
    if (g.AD, g.AH, g.AW) != (g.BD, g.BH, g.BW) or g.CA % 4 or g.CB % 4 or g.CA < 4 or g.CB < 4:
        return False
    if g.N * g.BD * g.BH * g.BW < 4 * 128:
        return False
    return _cdiv(g.CA, 64) * _cdiv(g.CB, 64) <= 64


def pwf_run(g, sw):
    if not pwf_ok(g):
        return ERR_UNSUPPORTED
    V = g.N * g.BD * g.BH * g.BW
    ntiles = _cdiv(V, 128)
    nau, nbu = _cdiv(g.CA, 64), _cdiv(g.CB, 64)
    want = sw["M1_PWF_BLOCKS"] // (nau * nbu)
    c = wg_copies(g, 1, want, ntiles, (2, MAX_COPIES, 0, "error"))
    if c.rc:
        return c.rc
    p = NS(ntiles=ntiles, V=V, nau=nau, nbu=nbu, tpb=_cdiv(ntiles, c.nsplit))
    return [_wg("wgrad_pwf", ntiles, want, c.nsplit, c, True, 0, (nbu, c.nsplit, nau)), ("fold", c.nsplit, g)], p


# ---- wgrad_tf.hip ----------------------------------------------------------------------------------------------------------------
def _tf_chan_ok(c):
    return c in (8, 16) or (c >= 32 and c % 32 == 0)


def tf_plan(g, sw):
    if g.f32 or (g.kd, g.kh, g.kw) not in ((1, 3, 3), (3, 3, 3)):
        return None
    if not _tf_chan_ok(g.CA) or not _tf_chan_ok(g.CB) or g.BW % 8 or not wg_vox32(g):
        return None
    n4 = sw["M1_TF_NKS4"]
    nks = 4 if ((n4 and g.CA <= 16 and g.CB <= 16) or (n4 == 2 and g.kd == 1)) else 2
    p = wg_ktiles(g, nks * 32, wg_kws(g.BW, 8), 0)
    if p is None:
        return None
    AHt, AWt = (p.TH - 1) * g.sh + g.kh, (p.KWs - 1) * g.sw + g.kw
    spra, sprb = min(g.CA, 32) // 8, min(g.CB, 32) // 8
    a_slots = _cdiv(g.kd * AHt * AWt * spra, 256) * 256
    b_slots = nks * 32 * sprb
    if a_slots > 10 * 256 or AHt > 255 or AWt > 255:
        return None
    sb = a_slots * 16 + _cdiv(b_slots, 256) * 256 * 16 + 64
    npiece = a_slots // 256 + _cdiv(b_slots, 256)
    S = min(max((76 * 1024) // sb, 3), 8)
    while S > 3 and npiece * (S - 2) > 48:
        S -= 1
    if sw["M1_TF_STAGES"] >= 3:
        S = sw["M1_TF_STAGES"]
    if not (npiece * (S - 2) <= 48 and S * sb <= 160 * 1024):
        return None
    p.nks, p.stages = nks, S
    return p


def tf_wanted(g, sw):
    if g.CA > 64 and g.CB > 32:
        return False
    return g.CA <= sw["M1_TF_MAXC"] and g.CB <= sw["M1_TF_MAXC"] and tf_plan(g, sw) is not None


def tf_run(g, sw, nmem=1):
    p = tf_plan(g, sw)
    if p is None:
        return ERR_UNSUPPORTED
    ctiles = _cdiv(g.CA, 32) * _cdiv(g.CB, 32)
    tgt = sw["M1_TF_SPLIT"] if sw["M1_TF_SPLIT"] > 0 else (512 if p.ntiles >= 24576 else 256)
    want = _cdiv(tgt, ctiles)
    c = wg_copies(g, g.kd * 9, want, p.ntiles, (1, 0, 96 << 20, "error"))
    if c.rc:
        return c.rc
    if nmem > 6:
        return ERR_UNSUPPORTED
    kparts = 4 // ((2 if g.CA > 16 else 1) * (2 if g.CB > 16 else 1))
    if p.nks == 4 and not (kparts == 4 or g.kd == 1):
        return ERR_UNSUPPORTED
    p.kparts, p.tpb = kparts, _cdiv(p.ntiles, c.nsplit)
    out = [_wg("wgrad_tf", p.ntiles, want, c.nsplit, c, True, p.stages, (ctiles, c.nsplit, max(nmem, 1)))]
    for m in range(max(nmem, 1)):
        gm = NS(**vars(g))
        gm.bsum = g.bsum and m == 0
        out.append(("fold", c.nsplit, gm))
    return out, p


# ---- wgrad_tap.hip / wgrad_mfma.hip ------------------------------------------------------------------------------------------------
def tap_plan(g):
    if g.f32 or g.CA < 64 or g.CB < 64 or g.CA % 8 or g.CB % 8:
        return None
    if (g.BW % 8 and g.BW > 32) or not wg_vox32(g):
        return None
    p = wg_ktiles(g, 64, wg_kws(g.BW, g.BW), 8)
    if p is None or (p.TH - 1) * g.sh > 255 or (p.KWs - 1) * g.sw > 255:
        return None
    return p


def tap_run(g, sw):
    p = tap_plan(g)
    TA, TB = (128 if g.CA > 64 else 64), (128 if g.CB > 64 else 64)
    taps = g.kd * g.kh * g.kw
    ctiles = _cdiv(g.CA, TA) * _cdiv(g.CB, TB)
    tgt = sw["M1_WG_TAP_BLOCKS"]
    want = tgt // (ctiles * taps) if sw["M1_WG_FLOOR"] else _cdiv(tgt, ctiles * taps)
    det = sw["M1_WG_DET"]
    c = wg_copies(g, taps, want, p.ntiles, (4, 0, 0, "fallback"), det != 0)
    nsplit = 1 if det and not c.Rx else c.nsplit
    S = min(max((76 * 1024) // (64 * (TA + TB) * 2), 2), 4)
    if sw["M1_WG_TAP_STAGES"] >= 2:
        S = sw["M1_WG_TAP_STAGES"]
    if sw["M1_WG_XCD"] and taps > 1:
        grid = (_cdiv(ctiles * nsplit * taps, 8) * 8, 1, 1)
    else:
        grid = (ctiles, nsplit, taps)
    p.TA, p.TB, p.ctiles, p.taps, p.tpb = TA, TB, ctiles, taps, _cdiv(p.ntiles, nsplit)
    out = [_wg("wgrad_tap", p.ntiles, want, nsplit, c, c.Rx, S, grid)]
    if c.Rx:
        out.append(("fold", nsplit, g))
    return out, p


def _pick_t(c):
    return 128 if c > 64 else 64 if c > 32 else 32


def mfma_run(g, sw):
    TA, TB = _pick_t(g.CA), _pick_t(g.CB)
    KB = 8 if TA + TB <= 64 else 4 if TA + TB <= 128 else 2
    KS = 4 * (4 if g.f32 else 8) * KB
    ct = _cdiv(g.CA, TA) * _cdiv(g.CB, TB)
    taps = g.kd * g.kh * g.kw
    TV = g.N * g.BD * g.BH * g.BW
    tgt = sw["M1_WG_BLOCKS"]
    splits = tgt // (ct * taps) if sw["M1_WG_FLOOR"] else _cdiv(tgt, ct * taps)
    splits = max(min(splits, _cdiv(TV, 4 * KS)), 1)

    def resplit(n):
        vps = _cdiv(_cdiv(TV, n), KS) * KS
        return _cdiv(TV, vps), vps
    splits, vps = resplit(splits)
    det = sw["M1_WG_DET"]
    small = taps * g.CA * g.CB <= 32768 and splits >= 24
    want = splits
    c = wg_copies(g, taps, splits, 0, (0, 0, 0, "fallback"), bool(det or small))
    rx = False
    if c.Rx:
        if c.nsplit < splits:
            splits, vps = resplit(c.nsplit)
        rx = splits >= 2
    elif det and splits >= 2:
        splits, vps = 1, _cdiv(TV, KS) * KS
    if sw["M1_WG_XCD"] and ct * taps > 1 and splits > 1:
        grid = (_cdiv(ct * taps * splits, 8) * 8, 1, 1)
    else:
        grid = (ct, taps, splits)
    p = NS(TV=TV, KS=KS, vps=vps, TA=TA, TB=TB, ct=ct, taps=taps, small=small, ntiles=TV)
    out = [_wg("wgrad_mfma", TV, want, splits, c, rx, 0, grid)]
    if rx:
        out.append(("fold", splits, g))
    return out, p


# ---- dispatch.hip: the ladder ------------------------------------------------------------------------------------------------------
def wg_plan_of(name, N, D, H, W, cins, cout, k, s, dtype, switches=None, bias=True, queued=True):
    """The plan-log entries of one m1_conv3d_wgrad / m1_convT3d_wgrad call, as dicts (parse_plan_entry's form), in log order, plus for
    every launch the launcher's geometry: returns (entries, launches) with launches = [(rung, kernel name, geometry)]; geometry.g is
    the member's spec.
    ``queued``: the folds are deferred (m1_wgrad_defer); a stem's fold never is."""
    sw = dict(SWITCHES)
    sw.update(switches or {})
    T, f32 = "convT" in name, dtype in ("fp32", "float32")
    dims, members = (D, H, W), tuple(cins)
    rxf = rx_bytes(members, cout, k, sw) // 4
    entries, launches = [], []

    def emit(res, rung, g, q=queued):
        out, p = res
        p.g = g
        for e in out:
            entries.append(fold_of(e[1], e[2], q) if isinstance(e, tuple) else e)
        launches.append((rung, out[0]["name"], p))

    if (not T) and len(members) == 1 and members[0] < (4 if f32 else 8):                   # stem_wanted
        CP = 4 if f32 else 8
        g = member_spec(N, dims, (CP,), cout, k, s, f32, False, 0, rxf, bias)
        if (ts_plan(g) if f32 else tf_plan(g, sw)) is not None:
            res = ts_run(g, sw) if f32 else tf_run(g, sw)
            if not isinstance(res, int):
                emit(res, "stem", g, False)
                entries.append(dict(kind="stem", cp=CP))
                return entries, launches
    i = 0
    while i < len(members):
        run = 1
        if not T:
            while i + run < len(members) and members[i + run] == members[i]:
                run += 1
        g = member_spec(N, dims, members, cout, k, s, f32, T, i, rxf, bias)
        ladder = [
            ("t3", True, lambda: t3_plan(g) is not None, lambda: t3_run(g, sw, run)),
            ("pwf", False, lambda: f32 and not T and pwf_ok(g), lambda: pwf_run(g, sw)),
            ("t3s", False, lambda: f32 and ts_plan(g) is not None, lambda: ts_run(g, sw)),
            ("tf-multi", True, lambda: sw["M1_TF_MULTI"] and not T and tf_wanted(g, sw) and run > 1, lambda: tf_run(g, sw, run)),
            ("tf", False, lambda: tf_wanted(g, sw), lambda: tf_run(g, sw)),
        ]
        used = None
        for rung, whole, gate, go in ladder:
            if not gate():
                continue
            res = go()
            if isinstance(res, int):
                entries.append(dict(kind="decline", rung=rung, rc=res))
                continue
            emit(res, rung, g)
            used = run if whole else 1
            break
        if used is None:
            if tap_plan(g) is not None:
                emit(tap_run(g, sw), "tap", g)
            else:                                                   # (m1_mfma_wgrad_supported: 32-bit voxel counts, far beyond these volumes)
                assert g.N * g.BD * g.BH * g.BW < (1 << 31) - 4096
                emit(mfma_run(g, sw), "mfma", g)
            used = 1
        i += used
    return entries, launches


def kernel_names(entries):
    return [e["name"] for e in entries if e["kind"] == "wg"]


_WG = re.compile(r"wg:(\S+) tiles=(\d+) want=(\d+) splits=(\d+) fit=(\d+) rx=([01]) stages=(\d+) grid=(\d+),(\d+),(\d+)$")
_FOLD = re.compile(r"fold:(generic|vec|wide) copies=(\d+) n=(\d+) nb=(\d+) el=(\d+) (queued|now)$")
_BATCH = re.compile(r"foldbatch:n=(\d+) blocks=(\d+)$")
_DECL = re.compile(r"decline:(\S+) rc=(-?\d+)$")
_STEM = re.compile(r"stem:cp=(\d)$")


def parse_plan_entry(e):
    """One entry of the plan log as a dict; an entry of no known form is an error."""
    m = _WG.match(e)
    if m:
        v = [int(x) for x in m.groups()[1:]]
        return dict(kind="wg", name=m.group(1), tiles=v[0], want=v[1], splits=v[2], fit=v[3], rx=v[4], stages=v[5], grid=tuple(v[6:9]))
    m = _FOLD.match(e)
    if m:
        return dict(kind="fold", mode=m.group(1), copies=int(m.group(2)), n=int(m.group(3)), nb=int(m.group(4)), el=int(m.group(5)),
                    when=m.group(6))
    m = _BATCH.match(e)
    if m:
        return dict(kind="foldbatch", n=int(m.group(1)), blocks=int(m.group(2)))
    m = _DECL.match(e)
    if m:
        return dict(kind="decline", rung=m.group(1), rc=int(m.group(2)))
    m = _STEM.match(e)
    assert m, f"plan-log entry of no known form: {e!r}"
    return dict(kind="stem", cp=int(m.group(1)))
