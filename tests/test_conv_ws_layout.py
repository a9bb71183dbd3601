"""The workspace layout of the conv dispatch is pinned byte for byte (pure host code: no GPU).

For a table of descriptors with at least one on each side of every branch of the dispatch's planner (grouped forward, odd split, fused
data gradient, per member, single; the stem region and the partial-copy scratch of the weight gradient), under the default switches and
under each switch that moves a branch: m1_conv_ws_bytes for roles 0, 1, 2, transposed and not, and the pack-job addresses of roles 0
and 1 relative to a fake workspace base that is never dereferenced.  The expected values, tests/golden/conv_ws_layout.json, were written
by `python tests/test_conv_ws_layout.py --write` with a library built from commit 2812fb1 (the parent of the dispatch restructuring)
and are not to be regenerated from later code: a layout change is a deliberate act that edits them by hand, with its reason."""
import ctypes as C
import json
import os
import sys

import pytest

from util import PKG, ROOT

L = PKG.hip.lib
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_ws_layout.json")
WS_BASE = 0x7F0000000000          # fake device address of `ws`
BF16, F32 = L.M1_BF16, L.M1_F32


def D(name, dims, members, cout, k=(3, 3, 3), s=(1, 1, 1), dtype=BF16, n=1):
    return dict(name=name, N=n, dims=dims, members=list(members), Cout=cout, k=k, s=s, dtype=dtype)


BIG, MID = (20, 160, 160), (20, 80, 80)
TABLE = [
    # layer shapes
    D("k333_s1_bf16", (8, 32, 32), [32], 32), D("k333_s1_f32", (8, 32, 32), [32], 32, dtype=F32),
    D("k333_s122", (8, 32, 32), [32], 64, s=(1, 2, 2)), D("k333_s222", (8, 32, 32), [32], 64, s=(2, 2, 2)),
    D("pointwise", (8, 32, 32), [64], 16, k=(1, 1, 1)), D("pointwise_f32", (8, 32, 32), [64], 16, k=(1, 1, 1), dtype=F32),
    D("up_k122", (4, 16, 16), [64], 32, k=(1, 2, 2), s=(1, 2, 2)), D("up_k222", (4, 16, 16), [64], 32, k=(2, 2, 2), s=(2, 2, 2)),
    D("up_k222_f32", (4, 16, 16), [64], 32, k=(2, 2, 2), s=(2, 2, 2), dtype=F32),
    D("deep_512_256", (4, 8, 8), [512], 256, n=2), D("wide_cout320", (8, 16, 16), [128], 320),
    # shapes the matrix-core kernels do not take (more than 27 taps; more than 8 stride classes)
    D("k335", (4, 16, 16), [32], 32, k=(3, 3, 5)), D("k335_concat", (4, 16, 16), [32, 32], 32, k=(3, 3, 5)),
    D("s224", (4, 16, 16), [32], 32, k=(2, 2, 4), s=(2, 2, 4)),
    # stem
    D("stem3_bf16", (8, 64, 64), [3], 32, n=2), D("stem2_bf16", (8, 64, 64), [2], 32, n=2),
    D("stem3_f32", (8, 64, 64), [3], 32, n=2, dtype=F32), D("stem2_f32", (8, 64, 64), [2], 32, n=2, dtype=F32),
    D("stem_two_members", (8, 64, 64), [2, 1], 32, n=2), D("stem_two_members_f32", (8, 64, 64), [2, 1], 32, n=2, dtype=F32),
    D("stem7_bf16", (8, 64, 64), [7], 32), D("nostem8_bf16", (8, 64, 64), [8], 32), D("nostem4_f32", (8, 64, 64), [4], 32, dtype=F32),
    # forward in member groups
    D("skip_32x5", BIG, [32] * 5, 32), D("skip_64x4", MID, [64] * 4, 64),
    D("skip_32x5_f32", BIG, [32] * 5, 32, dtype=F32), D("skip_64x4_f32", MID, [64] * 4, 64, dtype=F32),
    D("skip_ow_not_8", (20, 160, 156), [32] * 5, 32), D("skip_vox_32768", (8, 64, 64), [32] * 5, 32),
    D("skip_vox_below", (1, 4095, 8), [32] * 5, 32),         # 32760 voxels: the most below 32768 with OW % 8 == 0
    D("skip_member_24", BIG, [32, 24, 32], 32), D("skip_cin_64", BIG, [32, 32], 32),
    D("skip_pointwise", BIG, [32] * 5, 32, k=(1, 1, 1)), D("skip_merge", MID, [16, 16, 32, 64], 64),
    D("skip_s122", BIG, [32] * 5, 64, s=(1, 2, 2)),
    # odd split
    D("odd_3_512", (4, 8, 8), [3, 512], 256), D("odd_512_2", (4, 8, 8), [512, 2], 256), D("odd_3_512_2", (4, 8, 8), [3, 512, 2], 256),
    D("odd_3_512_up", (4, 8, 8), [3, 512], 256, k=(2, 2, 2), s=(2, 2, 2)),
    D("odd_512_2_up", (4, 8, 8), [512, 2], 256, k=(2, 2, 2), s=(2, 2, 2)),
    D("odd_3_512_f32", (4, 8, 8), [3, 512], 256, dtype=F32),
    D("odd_3_32", (4, 8, 8), [3, 32], 256), D("odd_3_256_3_256", (4, 8, 8), [3, 256, 3, 256], 256), D("odd_12_256", (4, 8, 8), [12, 256], 256),
    # fused data gradient
    D("dg_two_aligned", (4, 16, 16), [64, 64], 128), D("dg_two_aligned_f32", (4, 16, 16), [64, 64], 128, dtype=F32),
    D("dg_one_unaligned", (4, 16, 16), [32, 12], 128), D("dg_two_aligned_up", (4, 16, 16), [64, 64], 32, k=(2, 2, 2), s=(2, 2, 2)),
    D("dg_halo_32768", (8, 64, 64), [32, 32], 32), D("dg_halo_below", (7, 31, 151), [32, 32], 32),      # 32767 voxels
    D("dg_halo_cout64", (8, 64, 64), [32, 32], 64), D("dg_halo_cout72", (8, 64, 64), [32, 32], 72),
    D("dg_halo_s122", (8, 64, 64), [32, 32], 32, s=(1, 2, 2)), D("dg_halo_pointwise", (8, 64, 64), [32, 32], 32, k=(1, 1, 1)),
    D("dg_halo_f32", (8, 64, 64), [32, 32], 32, dtype=F32),
    # member count
    D("six_members", (8, 32, 32), [32] * L.M1_MAX_SRC, 64), D("six_mixed", (8, 64, 64), [16, 32, 64, 16, 32, 64], 32),
    D("six_members_f32", (8, 32, 32), [16] * L.M1_MAX_SRC, 64, dtype=F32),
]
assert len({t["name"] for t in TABLE}) == len(TABLE)

# (name, value) of m1_config_set; "force_direct" = m1_set_force_direct(1)
SETTINGS = [None, ("M1_ODD_SPLIT", 0), ("M1_HALO_GROUPS", 0), ("M1_DGRAD_FUSED", 0), ("M1_DGRAD_FUSED_HALO", 1), ("M1_STEM_TF", 0),
            ("M1_WG_RX_MB", 1), ("force_direct", 1)]


def _sid(s):
    return "default" if s is None else f"{s[0]}={s[1]}"


def _desc(t):
    d = L.m1_conv_desc_t()
    d.N = t["N"]; d.D, d.H, d.W = t["dims"]
    d.Cin = sum(t["members"]); d.Cout = t["Cout"]
    d.kd, d.kh, d.kw = t["k"]; d.sd, d.sh, d.sw = t["s"]
    d.dtype = t["dtype"]; d.nsrc = len(t["members"])
    for i, c in enumerate(t["members"]):
        d.src[i].ptr = 0x1000 * (i + 1)          # non-null, never dereferenced
        d.src[i].C = c
    return d


def layout(setting):
    """{descriptor name: {"ws": [[role 0, 1, 2] not transposed, [...] transposed], "jobs": the same shape for roles 0, 1, offsets from ws}}"""
    lib = L.load()
    if setting is not None:
        name, v = setting
        rc = lib.m1_set_force_direct(v) if name == "force_direct" else lib.m1_config_set(name.encode(), v)
        assert rc == 0
    try:
        out = {}
        for t in TABLE:
            d = _desc(t)
            ws, jobs = [], []
            for T in (0, 1):
                ws.append([int(lib.m1_conv_ws_bytes(C.byref(d), T, role)) for role in (0, 1, 2)])
                per = []
                for role in (0, 1):
                    buf = (C.c_void_p * L.M1_MAX_SRC)()
                    n = lib.m1_conv_pack_jobs(C.byref(d), T, role, C.c_void_p(WS_BASE), buf)
                    assert 0 <= n <= L.M1_MAX_SRC
                    per.append([int(buf[i]) - WS_BASE for i in range(n)])
                jobs.append(per)
            out[t["name"]] = {"ws": ws, "jobs": jobs}
        return out
    finally:
        if setting is not None:
            if setting[0] == "force_direct":
                lib.m1_set_force_direct(0)
            else:
                lib.m1_config_unset(setting[0].encode())


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_covers_the_table(golden):
    assert sorted(golden) == sorted(_sid(s) for s in SETTINGS)
    for sid, per in golden.items():
        assert sorted(per) == sorted(t["name"] for t in TABLE), sid


@pytest.mark.parametrize("setting", SETTINGS, ids=_sid)
def test_layout_matches_golden(setting, golden):
    got, want = layout(setting), golden[_sid(setting)]
    bad = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not bad, f"{len(bad)} of {len(want)} descriptors moved (got, golden): {bad}"


def test_table_reaches_both_sides_of_the_planner(golden):
    """The golden itself shows that the table is on both sides of each branch: jobs per role and the sizes that a switch moves."""
    g = golden["default"]
    njobs = lambda name, T, role: len(g[name]["jobs"][T][role])
    assert njobs("skip_32x5", 0, 0) == 3 and njobs("skip_64x4", 0, 0) == 4 and njobs("skip_merge", 0, 0) == 2       # grouped
    for name in ("skip_32x5_f32", "skip_64x4_f32", "skip_ow_not_8", "skip_vox_below", "skip_member_24", "skip_cin_64", "skip_pointwise"):
        assert njobs(name, 0, 0) == 1, name
    assert njobs("skip_vox_32768", 0, 0) == 3 and njobs("skip_32x5", 1, 0) == 1
    for name in ("odd_3_512", "odd_512_2", "odd_3_512_up", "odd_512_2_up", "odd_3_512_f32"):                             # odd split
        assert njobs(name, 0, 0) == 2 and njobs(name, 1, 0) == 2, name
    assert njobs("odd_3_512_2", 0, 0) == 3
    for name in ("odd_3_32", "odd_3_256_3_256", "odd_12_256"):
        assert njobs(name, 0, 0) == 1 and njobs(name, 1, 0) == 1, name
    for name in ("dg_two_aligned", "dg_two_aligned_f32", "dg_two_aligned_up", "dg_halo_below", "dg_halo_cout72", "dg_halo_s122",   # fused
                 "dg_halo_pointwise", "dg_halo_f32", "six_members"):
        assert njobs(name, 0, 1) == 1, name
    for name in ("dg_one_unaligned", "dg_halo_32768", "dg_halo_cout64"):                                                  # per member
        assert njobs(name, 0, 1) == 2, name
    assert njobs("six_mixed", 0, 1) == 6
    for name in ("k335", "k335_concat"):                                                                                  # no panel at all
        assert njobs(name, 0, 0) == 0 and njobs(name, 1, 1) == 0, name
    assert njobs("s224", 0, 0) == 1 and njobs("s224", 0, 1) == 0 and njobs("s224", 1, 0) == 0 and njobs("s224", 1, 1) == 1
    role2 = lambda sid, name: golden[sid][name]["ws"][0][2]
    for name in ("stem3_bf16", "stem2_bf16", "stem3_f32", "stem2_f32", "stem7_bf16"):                                     # stem region
        assert role2("default", name) > role2("M1_STEM_TF=0", name), name
    for name in ("stem_two_members", "stem_two_members_f32", "nostem8_bf16", "nostem4_f32"):
        assert role2("default", name) == role2("M1_STEM_TF=0", name), name
    assert role2("default", "deep_512_256") > role2("M1_WG_RX_MB=1", "deep_512_256")
    assert len(golden["M1_ODD_SPLIT=0"]["odd_3_512"]["jobs"][0][0]) == 1 and len(golden["M1_HALO_GROUPS=0"]["skip_32x5"]["jobs"][0][0]) == 1
    assert len(golden["M1_DGRAD_FUSED=0"]["dg_two_aligned"]["jobs"][0][1]) == 2
    assert len(golden["M1_DGRAD_FUSED_HALO=1"]["dg_halo_32768"]["jobs"][0][1]) == 1
    assert all(not j for v in golden["force_direct=1"].values() for T in v["jobs"] for j in T)


def test_invalid_descriptor_returns_zero():
    lib = L.load()
    d = L.m1_conv_desc_t()          # all zeros
    buf = (C.c_void_p * L.M1_MAX_SRC)()
    for T in (0, 1):
        for role in (0, 1, 2):
            for desc in (C.byref(d), None):          # (None: a null descriptor)
                assert lib.m1_conv_ws_bytes(desc, T, role) == 0
                assert lib.m1_conv_pack_jobs(desc, T, role, C.c_void_p(WS_BASE), buf) == 0
    assert lib.m1_conv3d_pair_supported(C.byref(d), 8) == 0 and lib.m1_conv3d_pair_supported(None, 8) == 0


if __name__ == "__main__":
    if sys.argv[1:] == ["--write"]:
        dump = lambda v: json.dumps(v, separators=(",", ":"))
        with open(GOLDEN, "w") as f:          # one descriptor per line
            f.write("{\n" + ",\n".join(
                dump(_sid(s)) + ":{\n" + ",\n".join(f"{dump(k)}:{dump(v)}" for k, v in layout(s).items()) + "\n}" for s in SETTINGS) + "\n}\n")
        print("wrote", GOLDEN)
