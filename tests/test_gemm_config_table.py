"""cl_gemm's table of tile configurations (ctrlora_amd/csrc/gemm.hip: kCfgs), read through the probe hook
cl_debug_gemm_config, against literals written down from the 46-way switch, the bn_of lambda and the GEGLU chain that the table
replaced.  Nothing here is read back from the table: the dicts below are the independent record of what every id launched
before it existed.  No kernel is launched (no GPU needed)."""
import ast
import ctypes
import os

import pytest

from tests.util import ROOT

GEN, FL, XS, W4 = 0, 1, 2, 3
PERSIST, PAIR, PAIR_BF16, K_LINES, LINEAR, WHOLE_N = 1, 2, 4, 8, 16, 32

# id -> (BM, BN, WGM, WGN, KSUB, R): the launch_cfg<T, ...> cases of the old switch (gemm_kernel)
OLD_GENERIC = {
    0: (64, 64, 2, 2, 1, 4), 1: (128, 128, 2, 2, 2, 4), 2: (128, 160, 2, 2, 2, 4), 3: (128, 160, 2, 2, 1, 4),
    4: (128, 160, 2, 2, 2, 6), 5: (256, 160, 4, 2, 2, 4), 6: (128, 128, 2, 2, 1, 2), 7: (256, 128, 4, 2, 2, 4),
    22: (64, 128, 2, 2, 1, 4), 23: (64, 160, 2, 2, 1, 4), 24: (128, 64, 2, 2, 1, 4),
    42: (64, 64, 2, 2, 1, 8), 43: (64, 128, 2, 2, 1, 8), 44: (64, 160, 2, 2, 1, 8), 45: (128, 64, 2, 2, 1, 8),
    46: (128, 128, 2, 2, 2, 8),
}
# id -> (BM, BN, WGM, WGN, R, PRIO, persistent): the launch_fl<T, ...> cases (gemm_fl_kernel / gemm_fl_persist_kernel)
OLD_FULL_LINE = {
    8: (256, 160, 4, 2, 3, 0, 0), 9: (256, 128, 4, 2, 3, 0, 0), 10: (128, 160, 2, 2, 2, 0, 0), 11: (128, 128, 2, 2, 2, 0, 0),
    12: (256, 160, 4, 2, 3, 1, 0), 13: (256, 128, 4, 2, 3, 1, 0), 14: (256, 160, 4, 2, 3, 2, 0), 15: (256, 128, 4, 2, 3, 2, 0),
    16: (256, 160, 4, 2, 3, 3, 0), 17: (256, 128, 4, 2, 3, 3, 0), 18: (256, 160, 4, 2, 3, 4, 0), 19: (256, 128, 4, 2, 3, 4, 0),
    20: (128, 160, 4, 2, 3, 3, 0), 21: (128, 128, 4, 2, 3, 3, 0),
    25: (256, 160, 4, 2, 3, 3, 1), 26: (256, 128, 4, 2, 3, 3, 1), 27: (128, 160, 4, 2, 3, 3, 1), 28: (128, 128, 4, 2, 3, 3, 1),
    29: (128, 160, 2, 2, 2, 0, 1), 30: (128, 128, 2, 2, 2, 0, 1),
    31: (128, 80, 4, 1, 2, 0, 0), 32: (128, 80, 4, 1, 3, 0, 0), 33: (128, 320, 2, 4, 2, 0, 0),
    35: (64, 80, 4, 1, 3, 0, 0), 36: (64, 80, 4, 1, 2, 0, 0),
}
# the other translation units: id -> (family, BN handed to / used by the launcher, persistent)
OLD_FOREIGN = {34: (XS, 32, 0), 40: (W4, 160, 0), 41: (W4, 128, 0), 47: (W4, 160, 1), 48: (W4, 128, 1)}
# the pasted `kps` blocks: which ids ran the generic 128 x 128 tile (id 1) instead, and when
OLD_FALLBACK = {
    **{i: K_LINES for i in (8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21)},      # K1 % kps || K2 % kps || (mode != LINEAR && K2)
    **{i: K_LINES | LINEAR for i in (25, 26, 27, 28, 29, 30)},                           # ... || mode != LINEAR
    **{i: K_LINES | LINEAR | WHOLE_N for i in (31, 32, 33)},                             # ... || mode != LINEAR || N % 80 (33: N % 320)
    **{i: K_LINES | WHOLE_N for i in (35, 36)},                                          # ... || (mode != LINEAR && K2) || N % 80
}
# the chain on the first line of the old launch_t_cfg (+ 40 / 47 where sizeof(T) == 2)
OLD_GEGLU = {2, 8, 10, 12, 14, 16, 18, 20, 23, 25, 27, 29, 44}
OLD_GEGLU_BF16 = {40, 47}
# the old bn_of lambda for K in whole 128-byte lines (and N a multiple of 80 / 320 where it asked)
OLD_BN = {
    **{i: 64 for i in (0, 24, 42, 45)}, 43: 128, 44: 160, 46: 128, **{i: 128 for i in (1, 6, 7, 22)},
    **{i: 160 for i in (2, 3, 4, 5, 23)}, 40: 160, 47: 160, 41: 128, 48: 128, **{i: 80 for i in (31, 32, 35, 36)}, 33: 320, 34: 32,
    **{i: 160 for i in (8, 12, 14, 16, 18, 20, 10, 25, 27, 29)},
    **{i: 128 for i in (9, 11, 13, 15, 17, 19, 21, 26, 28, 30)},                          # its default branch
}
ALL_IDS = list(range(0, 37)) + list(range(40, 49))


@pytest.fixture(scope="module")
def rows():
    from ctrlora_amd import build
    L = ctypes.CDLL(build.build(verbose=False))
    L.cl_debug_gemm_config.argtypes = [ctypes.c_int, ctypes.c_void_p]
    out = {}
    for cfg in range(-3, 80):
        buf = (ctypes.c_int * 10)(*([-7] * 10))
        rc = L.cl_debug_gemm_config(cfg, ctypes.cast(buf, ctypes.c_void_p))
        if rc == 0:
            out[cfg] = dict(zip(("id", "fam", "bm", "bn", "wgm", "wgn", "ksub", "r", "prio", "flags"), buf))
        else:
            assert rc == 1 and list(buf) == [-7] * 10, (cfg, rc, list(buf))       # CL_EINVAL, nothing written
    assert L.cl_debug_gemm_config(1, None) == 1
    return out


def test_the_hook_knows_exactly_the_46_ids(rows):
    assert sorted(rows) == ALL_IDS and len(ALL_IDS) == 46
    assert all(r["id"] == cfg for cfg, r in rows.items())
    assert sorted([*OLD_GENERIC, *OLD_FULL_LINE, *OLD_FOREIGN]) == ALL_IDS == sorted(OLD_BN)


def test_every_row_is_what_the_old_switch_launched(rows):
    for cfg, want in OLD_GENERIC.items():
        r = rows[cfg]
        assert (r["fam"], r["bm"], r["bn"], r["wgm"], r["wgn"], r["ksub"], r["r"]) == (GEN, *want), (cfg, r)
        assert r["prio"] == 0 and not r["flags"] & ~PAIR, (cfg, r)       # never persistent, never falls back
    for cfg, want in OLD_FULL_LINE.items():
        r = rows[cfg]
        got = (r["fam"], r["bm"], r["bn"], r["wgm"], r["wgn"], r["r"], r["prio"], r["flags"] & PERSIST)
        assert got == (FL, *want), (cfg, r)
    for cfg, (fam, bn, persist) in OLD_FOREIGN.items():
        r = rows[cfg]
        assert (r["fam"], r["bn"], r["flags"] & PERSIST) == (fam, bn, persist), (cfg, r)
        assert fam == XS or r["bm"] == 256, (cfg, r)                     # gemm_w4.hip: W4_BM


def test_fall_back_conditions_are_the_old_kps_blocks(rows):
    for cfg in OLD_GENERIC:
        assert rows[cfg]["flags"] & (K_LINES | LINEAR | WHOLE_N) == 0, cfg
    for cfg in OLD_FULL_LINE:
        assert rows[cfg]["flags"] & (K_LINES | LINEAR | WHOLE_N) == OLD_FALLBACK[cfg], (cfg, rows[cfg])
    assert set(OLD_FALLBACK) == set(OLD_FULL_LINE)
    # the fall-back tile itself is the old `launch_cfg<T, 128, 128, 2, 2, 2, 4>`
    assert OLD_GENERIC[1] == (128, 128, 2, 2, 2, 4)


def test_geglu_capable_ids_are_the_old_chain(rows):
    assert {c for c, r in rows.items() if r["flags"] & PAIR} == OLD_GEGLU
    assert {c for c, r in rows.items() if r["flags"] & PAIR_BF16} == OLD_GEGLU_BF16
    assert all(rows[c]["bn"] == 160 for c in OLD_GEGLU | OLD_GEGLU_BF16)


def test_tile_width_is_the_old_bn_of(rows):
    assert {c: r["bn"] for c, r in rows.items()} == OLD_BN
    # for K not in whole lines the lambda answered 128 for exactly the ids below; they are the rows flagged K_LINES
    old_128_without_lines = set(OLD_FULL_LINE) | {40, 47, 41, 48}
    assert {c for c, r in rows.items() if r["flags"] & K_LINES} == old_128_without_lines


def _tuner_pools():
    tree = ast.parse(open(os.path.join(ROOT, "tools", "gemm_autotune.py")).read())
    pools = {}
    for node in tree.body:
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name):
            name = node.targets[0].id
            if name in ("FL", "W80", "W320", "PERSIST", "W160", "W128", "GEGLU_OK", "DEEP", "W4"):
                pools[name] = set(ast.literal_eval(node.value))
    assert len(pools) == 9, sorted(pools)
    return pools


def test_tuner_pools_offer_only_what_the_table_says_they_are(rows):
    """tools/gemm_autotune.py keeps its candidate pools literal (they are choices: FL leaves out 8 / 9, ...); each must lie
    inside the set of ids the table gives that property."""
    pools = _tuner_pools()

    def ids(pred):
        return {c for c, r in rows.items() if pred(r)}

    assert pools["FL"] <= ids(lambda r: r["fam"] == FL)
    for name, bn in (("W160", 160), ("W128", 128), ("W80", 80), ("W320", 320)):
        assert pools[name] <= ids(lambda r: r["bn"] == bn), name
    assert pools["PERSIST"] | {47, 48} <= ids(lambda r: r["flags"] & PERSIST)
    assert pools["GEGLU_OK"] <= ids(lambda r: r["flags"] & (PAIR | PAIR_BF16))
    assert pools["DEEP"] <= ids(lambda r: r["fam"] == GEN and r["r"] == 8)
    assert pools["W4"] <= ids(lambda r: r["fam"] == W4)
    assert all(p and p <= set(ALL_IDS) for p in pools.values())
