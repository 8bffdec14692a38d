"""Kernel-level conformance of cl_gemm (ctypes -> C ABI, like every GPU test): every launch the shipped tables or the rules of
csrc/gemm.hip:launch_t_cfg can choose, element-wise against the fp64 contract of include/ctrlora_hip.h:cl_gemm_params.

  A. every row of the three launch tables (gemm_tuned_gfx950{,_xs,_r06}.json, read at collection time) as exactly that product,
     once through the table and once with its (cfg, splitk) forced: bit-identical, same grid;
  B. the same signatures at the per-GPU batch sizes nobody tuned (M b / 8 for b = 1, 3, 4; b = 4 is the reference's pre-training
     batch, train_ctrlora_pretrain.py:35), which have no row and go by rule -- bf16, and b = 3 in fp32 (no fp32 product has a row);
  C. every configuration id launch_t_cfg accepts, forced, across the epilogue contract at small shapes that sit on tile edges,
     in both dtypes, linear and the five 3x3 modes (CONV_S2A, AutoencoderKL's Downsample, on an even and an odd grid; once more at
     a size the full-line and the loader / consumer kernels take themselves: test_s2a_on_the_whole_line_kernels), and the
     residual epilogues a second time IN PLACE (C == residual: "part of the contract for every configuration"), bit for bit the
     out-of-place result, forced split-K included.  "A stale or foreign table costs speed, never correctness": a forced
     configuration that cannot take a case runs it through its fall-back and passes the same checks; only what the CONTRACT
     excludes (a predicate on the case, never on the configuration) may be refused.

Every launch gets the four checks of tests/gemm_ref.py: rel-L2 (the project's gates), the element-wise bound
u_out |ref| + 2 K 2^-24 mag with zero violations, the canary around the output (ldc = N + 8, 64 guard rows, padded and mutually
different leading dimensions of A1 / A2 / residual / rowbias), and exactly one launch of the signature in the tag table.
Measured figures are written through _record (test_zz_conformance_summary: per-layer maxima and the wall time).
"""
import json
import os
import time

import pytest
import torch

from tests import gemm_ref as G
from tests.gemm_ref import _tags
from tests.test_gpu_bench_shapes import _need_gpu, _record

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
_STATS = {}
_T0 = [None]


def _note(layer, c, res):
    if _T0[0] is None:
        _T0[0] = time.time()
    s = _STATS.setdefault(layer, dict(launches=0, err_over_bound=0.0, rel_bf16=0.0, rel_f32=0.0, violations=0, canary=0))
    s["launches"] += 1
    s["err_over_bound"] = max(s["err_over_bound"], res["err_over_bound"])
    k = "rel_bf16" if c["out_dtype"] == BF else "rel_f32"
    s[k] = max(s[k], res["rel"])
    s["violations"] += res["violations"]
    s["canary"] += res["guard_rows"] + res["pad_elems"] + res["nan_left"]


# ------------------------------------------------------------------------------------------------ tables

def _tables():
    """[(file tag, row)] in the order the host loads them, and signature -> (cfg, splitk) as the overlays leave it."""
    from ctrlora_amd import hip
    entries, eff = [], {}
    for tag, path in (("main", hip.GEMM_TABLE_PATH), ("xs", hip.GEMM_XS_TABLE_PATH), ("r06", hip.GEMM_R06_TABLE_PATH)):
        with open(path) as f:
            for row in json.load(f)["entries"]:
                row = tuple(int(v) for v in row[:9])
                entries.append((tag, row))
                eff[row[:7]] = row[7:9]
    return entries, eff


_ENTRIES, _EFFECTIVE = _tables()


def _reload_tables():
    from ctrlora_amd import hip
    hip.load_gemm_table(hip.GEMM_TABLE_PATH)
    hip.load_gemm_table(hip.GEMM_XS_TABLE_PATH, clear=False)
    hip.load_gemm_table(hip.GEMM_R06_TABLE_PATH, clear=False)


def _assert_tables_loaded_as_the_engine_loads_them():
    from ctrlora_amd import hip
    assert os.environ.get("CTRLORA_GEMM_TUNED", "1") != "0" and "CTRLORA_GEMM_TABLE" not in os.environ
    assert hip.XS_ENABLED and hip.R06_ENABLED, "the _xs and _r06 overlays are part of the default"
    assert hip.lib().cl_gemm_tune_size() == len(_EFFECTIVE), (hip.lib().cl_gemm_tune_size(), len(_EFFECTIVE))


# ------------------------------------------------------------------------------------------------ cases and launches

def _rand(seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return lambda *s, sc=1.0, dtype=F32: (torch.randn(*s, generator=g, device="cuda") * sc).to(dtype)


def _geometry(M, mode, b=8):
    """conv = (B, Hin, Win, Hout, Wout) with B Hout Wout = M.  At the tuned batch (b = 8): the largest power-of-two B <= 16 for
    which M / B is a square (tools/gemm_autotune.py records the products of the training / DDIM / VAE steps and names no
    geometry).  At another per-GPU batch b: the same images, B b / 8 of them."""
    M8 = M * 8 // b
    for B in (16, 8, 4, 2, 1):
        if M8 % B == 0:
            h = int(round((M8 // B) ** 0.5))
            if h * h == M8 // B:
                hin = h // 2 if mode in (G.CONV_UP2, G.CONV_T2) else h
                assert mode not in (G.CONV_UP2, G.CONV_T2) or h % 2 == 0
                assert (B * b) % 8 == 0 and B * b // 8 * h * h == M, (M, b, B, h)
                return (B * b // 8, hin, hin, h, h)
    raise AssertionError(f"no square geometry for M = {M}")


def _signature_case(dtype, mode, M, N, K1, K2, geglu, b=8):
    """The product of one table signature: operands at unit scale, both K segments at the magnitude of the whole, bias always."""
    r = _rand(M + N + K1 + K2 + mode)
    bias = r(N, sc=0.1)
    if mode == G.LINEAR:
        kw = dict(a2=r(M, K2, dtype=dtype), w2=r(N, K2, sc=K2 ** -0.5, dtype=dtype)) if K2 else {}
        return G.make_case(r(M, K1, dtype=dtype), r(N, K1, sc=K1 ** -0.5, dtype=dtype), bias=bias,
                           act=G.ACT_GEGLU if geglu else G.ACT_NONE, **kw)
    # 3x3 products through the engine's own packing (packing.Conv3W), called as blocks.conv3_fwd (S1 / UP2: Wp, the conv's own
    # bias) and blocks.conv3_bwd_data (T2: the tap-flipped Wd, K1 = the conv's output channels) call them
    from ctrlora_amd.engine.packing import Conv3W
    assert K2 == 0 and not geglu
    conv = _geometry(M, mode, b)
    B, Hin, Win = conv[:3]
    if mode == G.CONV_T2:
        cw = Conv3W(r(K1, N, 3, 3, sc=1.0 / (3 * K1 ** 0.5)).cpu(), r(K1).cpu(), dtype, "cuda", True)
        w1 = cw.Wd
    else:
        cw = Conv3W(r(N, K1, 3, 3, sc=1.0 / (3 * K1 ** 0.5)).cpu(), bias.cpu(), dtype, "cuda", False)
        w1, bias = cw.Wp, cw.bias
    assert tuple(w1.shape) == (N, 9 * K1), (tuple(w1.shape), N, K1)
    return G.make_case(r(B * Hin * Win, K1, dtype=dtype), w1, bias=bias, mode=mode, conv=conv)


def _launch(c, inplace=False):
    """cl_gemm on the case: the output a view into a guarded buffer, every strided operand a padded copy.  inplace: the view holds
    the residual's values and IS the residual (residual = C, ldr = ldc)."""
    from ctrlora_amd import hip
    guard = G.Guarded(c["M"], c["out_cols"], c["out_dtype"], "cuda", fill=c["c0"] if c["atomic"] else float("nan"))
    if inplace:
        assert _inplace_possible(c), "in place: a residual of the output's own type and shape"
        guard.view.copy_(c["residual"])
        residual = guard.view
    else:
        residual = G.padded(c["residual"], G.PAD_RES)
    hip.gemm(G.padded(c["a1"], G.PAD_A1), c["w1"], guard.view, a2=G.padded(c["a2"], G.PAD_A2), w2=c["w2"], bias=c["bias"],
             rowbias=G.padded(c["rowbias"], G.PAD_RB), rows_per_batch=c["rows_per_batch"], residual=residual,
             alpha=c["alpha"], beta=c["beta"], act=c["act"], mode=c["mode"], conv=c["conv"], k1=c["K1"], out_f32=c["out_f32"],
             atomic=c["atomic"], splitk=c["splitk"], N=c["N"], a1_group_n=c["a1_group_n"], a2_group_n=c["a2_group_n"],
             alpha_n=c["alpha_n"])
    return guard


def _sig(c):
    from ctrlora_amd import hip
    return dict(dtype=hip.dt_of(c["dtype"]), mode=c["mode"], M=c["M"], N=c["N"], K1=c["K1"], K2=c["K2"], act=c["act"],
                residual=int(c["residual"] is not None))


def _inplace_possible(c):
    """Can C be the residual?  The residual is read in `dtype`, so only where C is stored in `dtype` too (a bf16 product with an
    fp32 output has no element that is both), and never with atomic accumulation.  A predicate on the case alone."""
    return c["residual"] is not None and c["out_dtype"] == c["dtype"] and not c["atomic"] and c["out_cols"] == c["N"]


def _launch_tagged(c, inplace=False):
    """(guard, launches of the case's signature, (workgroups, wg_size))."""
    from ctrlora_amd import hip
    with _tags() as tags:
        guard = _launch(c, inplace)
        torch.cuda.synchronize()
        n, _ = tags.launches(**_sig(c))
        grid = [(t["workgroups"], t["wg_size"]) for t in hip.gemm_tags() if all(t[k] == v for k, v in _sig(c).items())]
    return guard, n, (grid[0] if grid else None)


def _forced(cfg, sk):
    class _F:
        def __enter__(self):
            from ctrlora_amd import hip
            L = hip.lib()
            L.cl_gemm_force_config(cfg)
            L.cl_gemm_force_splitk(sk)

        def __exit__(self, *exc):
            from ctrlora_amd import hip
            L = hip.lib()
            L.cl_gemm_force_config(-1)
            L.cl_gemm_force_splitk(0)
            return False
    return _F()


def _bits(guard):
    return guard.buf.view(torch.int16 if guard.buf.dtype == BF else torch.int32)


# ------------------------------------------------------------------------------------------------ A: every row of every table

def test_layer_a_has_one_case_per_table_entry():
    from ctrlora_amd import hip
    n = 0
    for path in (hip.GEMM_TABLE_PATH, hip.GEMM_XS_TABLE_PATH, hip.GEMM_R06_TABLE_PATH):
        with open(path) as f:
            n += len(json.load(f)["entries"])
    assert len(_ENTRIES) == n and n >= 230, (len(_ENTRIES), n)
    _record("gemm_conformance_layer_a_cases", entries=n, signatures=len(_EFFECTIVE))


@pytest.mark.parametrize("tag,row", _ENTRIES, ids=[t + "-" + "-".join(str(v) for v in r) for t, r in _ENTRIES])
def test_tabled_row_elementwise_vs_fp64(tag, row):
    """One table entry [dtype, mode, M, N, K1, K2, geglu, cfg, splitk] as exactly that product.  (1) through the table, as
    the overlays leave the signature; (2) with that (cfg, splitk) forced: bit-identical, guard region included, and the same
    (workgroups, wg_size) -- the row is in effect; (3) under the rules alone (table cleared, then reloaded): recorded, so that a
    row indistinguishable from the rules (the rules choose the same form, or the form refused the product and fell back) is on
    record; (4) an entry that an overlay replaces is also launched with its OWN (cfg, splitk) forced: what ships with
    CTRLORA_GEMM_XS=0 / CTRLORA_GEMM_R06=0.  Every launch: the four checks."""
    _need_gpu()
    from ctrlora_amd import hip
    _assert_tables_loaded_as_the_engine_loads_them()
    dtype_id, mode, M, N, K1, K2, geglu, cfg_own, sk_own = row
    cfg, sk = _EFFECTIVE[row[:7]]
    c = _signature_case({hip.BF16: BF, hip.F32: F32}[dtype_id], mode, M, N, K1, K2, geglu)
    assert (c["M"], c["N"], c["K1"], c["K2"]) == (M, N, K1, K2)
    tabled, n, grid = _launch_tagged(c)
    assert n == 1, (n, hip.gemm_tags())
    res = G.run_checks(c, tabled.view, tabled)
    with _forced(cfg, sk):
        forced, n_f, grid_f = _launch_tagged(c)
    L = hip.lib()
    try:
        L.cl_gemm_tune_clear()
        ruled, n_r, grid_r = _launch_tagged(c)
    finally:
        _reload_tables()
    identical = bool(torch.equal(_bits(tabled), _bits(forced)))
    as_rules = bool(grid == grid_r and torch.equal(_bits(tabled), _bits(ruled)))
    res_r = G.run_checks(c, ruled.view, ruled)
    rec = dict(file=tag, row=list(row), effective=[cfg, sk], grid=grid, grid_forced=grid_f, grid_rules=grid_r,
               identical_to_forced=identical, indistinguishable_from_rules=as_rules, rel=res["rel"], gate=res["gate"],
               err_over_bound=res["err_over_bound"], violations=res["violations"], first_violation=res["first_violation"],
               canary=[res["guard_rows"], res["pad_elems"], res["nan_left"]], rules_err_over_bound=res_r["err_over_bound"],
               rules_failures=G.failures(res_r))
    _note("A", c, res)
    _note("A_rules", c, res_r)
    own = None
    if (cfg_own, sk_own) != (cfg, sk):
        with _forced(cfg_own, sk_own):
            g_own, n_o, grid_o = _launch_tagged(c)
        own = G.run_checks(c, g_own.view, g_own)
        _note("A_replaced", c, own)
        rec.update(own=[cfg_own, sk_own], own_grid=grid_o, own_err_over_bound=own["err_over_bound"], own_failures=G.failures(own))
    _record("gemm_conformance_tabled_row", **rec)
    assert n_f == 1 and n_r == 1, (n_f, n_r)
    assert identical and grid == grid_f, ("the forced launch differs from the tabled one", grid, grid_f, identical)
    assert G.failures(res) == [], res
    assert G.failures(res_r) == [], ("under the rules alone", res_r)
    assert own is None or G.failures(own) == [], ("the entry an overlay replaces", own)


# ------------------------------------------------------------------------------------------------ B: untuned batch sizes, by rule

def _untuned():
    seen, out = set(), []
    for b in (1, 3, 4):
        for sig in _EFFECTIVE:
            dtype_id, mode, M, N, K1, K2, geglu = sig
            if (M * b) % 8:
                continue
            s = (dtype_id, mode, M * b // 8, N, K1, K2, geglu)
            if s in _EFFECTIVE or s in seen:
                continue
            seen.add(s)
            out.append((b, s, BF))
    # fp32 "parity mode": no fp32 signature has a row; the b = 3 set (ragged M) again in fp32
    out += [(b, (1,) + s[1:], F32) for b, s, _ in out if b == 3]
    return out


_UNTUNED = _untuned()


def test_layer_b_case_count():
    n_bf = sum(1 for _, _, d in _UNTUNED if d == BF)
    assert n_bf >= len(_EFFECTIVE) and len(_UNTUNED) > n_bf, (n_bf, len(_UNTUNED))
    assert len({(s, d) for _, s, d in _UNTUNED}) == len(_UNTUNED)           # distinct after scaling
    assert all(s not in _EFFECTIVE for _, s, _ in _UNTUNED)                 # none has a row: these launches go by rule
    print("layer B cases:", len(_UNTUNED), "bf16:", n_bf)
    _record("gemm_conformance_layer_b_cases", cases=len(_UNTUNED), bf16=n_bf, fp32=len(_UNTUNED) - n_bf)


@pytest.mark.parametrize("b,sig,dtype", _UNTUNED,
                         ids=[f"b{b}-{'f32' if d == F32 else 'bf16'}-" + "-".join(str(v) for v in s[1:]) for b, s, d in _UNTUNED])
def test_rule_dispatched_signature_elementwise_vs_fp64(b, sig, dtype):
    """A table signature at per-GPU batch b instead of 8 (M b / 8): no row, so launch_t_cfg's rules choose the form."""
    _need_gpu()
    from ctrlora_amd import hip
    _assert_tables_loaded_as_the_engine_loads_them()
    assert sig not in _EFFECTIVE and sig[0] == hip.dt_of(dtype)
    _, mode, M, N, K1, K2, geglu = sig
    c = _signature_case(dtype, mode, M, N, K1, K2, geglu, b)
    guard, n, grid = _launch_tagged(c)
    res = G.run_checks(c, guard.view, guard)
    _note("B", c, res)
    _record("gemm_conformance_rule_row", b=b, sig=list(sig), grid=grid, rel=res["rel"], gate=res["gate"], torch_f32=res["torch_f32"],
            err_over_bound=res["err_over_bound"], violations=res["violations"], first_violation=res["first_violation"],
            canary=[res["guard_rows"], res["pad_elems"], res["nan_left"]])
    assert n == 1, (n, hip.gemm_tags())
    assert G.failures(res) == [], res


# ------------------------------------------------------------------------------------------------ C: every configuration

# the ids csrc/gemm.hip launches (kept literal here: the rows of its table kCfgs are what this file tests)
CONFIGS = tuple(range(0, 37)) + tuple(range(40, 49))
NOT_CONFIGS = (37, 38, 39, 49)
# (M, N, K1, K2): M in {1, 63, 129, 257, 1000}, N in {8, 72, 160, 328, 640}, K1 in {32, 96, 320, 1344} (96 and 1344 are not whole
# 128-byte lines in bf16: the fall-back inside the full-line cases), K2 in {0, 32, 128}; every value at least twice
SHAPES = [(1, 8, 32, 0), (1, 328, 1344, 32), (1, 160, 320, 128), (63, 72, 96, 128), (63, 640, 320, 0), (63, 160, 1344, 32),
          (129, 160, 32, 128), (129, 8, 320, 32), (129, 328, 96, 0), (257, 328, 320, 128), (257, 72, 1344, 0), (257, 640, 32, 32),
          (1000, 640, 96, 128), (1000, 160, 320, 0), (1000, 72, 32, 32), (1000, 8, 1344, 128)]
ALWAYS = ("bias", "rowbias", "residual", "alpha_n", "silu", "out_f32", "k2")       # every configuration takes these


def _contract_excludes(c):
    """Is the case outside the contract of cl_gemm_params (include/ctrlora_hip.h)?  A predicate on the case alone."""
    kq = 32 if c["dtype"] == BF else 16
    if c["N"] % 8 or c["K1"] % kq or c["K2"] % kq:
        return True
    if c["splitk"] > 1 and (not c["atomic"] or c["act"] != G.ACT_NONE):
        return True
    if c["act"] == G.ACT_GEGLU and (c["N"] % 160 or c["rowbias"] is not None or c["residual"] is not None or c["atomic"]
                                   or c["alpha"] != 1.0 or c["alpha_n"]):
        return True
    if c["mode"] != G.LINEAR and (c["K2"] or c["a1_group_n"] or c["a2_group_n"]):
        return True
    for gn in (c["a1_group_n"], c["a2_group_n"]):
        if gn and (c["N"] % gn or not any(gn % bn == 0 for bn in (64, 128, 160))):
            return True
    return False


def _linear_cases(dtype):
    """[(name, shape, case, forced split-K)]: the literal list of Layer C for one dtype."""
    out = []
    for i, (M, N, K1, K2) in enumerate(SHAPES):
        r = _rand(1000 * i + (7 if dtype == F32 else 0))
        o = dict(a1=r(M, K1, dtype=dtype), w1=r(N, K1, sc=K1 ** -0.5, dtype=dtype), bias=r(N, sc=0.1))
        if K2:
            o.update(a2=r(M, K2, dtype=dtype), w2=r(N, K2, sc=K2 ** -0.5, dtype=dtype))
        add = lambda name, sk=0, **kw: out.append((name, (M, N, K1, K2), G.make_case(**{**o, **kw}), sk))
        add("k2" if K2 else "bias")
        nb = (M + 76) // 77
        # every other epilogue on a rotating third of the shapes; GEGLU wherever N % 160 == 0
        if i % 3 == 0:
            add("rowbias", rowbias=r(nb, N, dtype=dtype), rows_per_batch=77)
            add("silu", act=G.ACT_SILU)
            add("atomic", atomic=True, splitk=3, c0=1.0)
            add("splitk5", sk=5)
        if i % 3 == 1:
            add("residual", residual=r(M, N, dtype=dtype), alpha=0.7, beta=-0.5)
            add("out_f32", out_f32=True)
            add("splitk2", sk=2)
        if i % 3 == 2:
            add("alpha_n", alpha=0.125, alpha_n=max(8, N // 16 * 8))
            add("rowbias+residual+silu", rowbias=r(nb, N, dtype=dtype), rows_per_batch=77, residual=r(M, N, dtype=dtype), beta=1.0,
                act=G.ACT_SILU)
            add("splitk2+residual", sk=2, residual=r(M, N, dtype=dtype), alpha=0.7, beta=-0.5)
        if N % 160 == 0:
            add("geglu", act=G.ACT_GEGLU)
            add("geglu+out_f32", act=G.ACT_GEGLU, out_f32=True)
    # grouped K segments, as test_grouped_lora_products_vs_fp64 builds them: x | W_g | t = [t_g] | B_g, and u = [dy_g B_g]
    for j, (M, K, Ng, rk, Gn) in enumerate([(63, 96, 64, 32, 3), (257, 320, 160, 128, 2), (1000, 64, 64, 32, 2), (129, 320, 128, 64, 3)]):
        r = _rand(5000 + j)
        x, W = r(M, K, dtype=dtype), r(Gn * Ng, K, sc=K ** -0.5, dtype=dtype)
        t, Bm = r(M, Gn * rk, dtype=dtype), r(Gn * Ng, rk, sc=rk ** -0.5, dtype=dtype)
        out.append(("grouped_a2", (M, Gn * Ng, K, rk), G.make_case(x, W, a2=t, w2=Bm, a2_group_n=Ng, bias=r(Gn * Ng, sc=0.1)), 0))
        dy, Bt = r(M, Gn * K, dtype=dtype), r(Gn * 64, K, sc=K ** -0.5, dtype=dtype)
        out.append(("grouped_a1", (M, Gn * 64, K, 0), G.make_case(dy, Bt, a1_group_n=64), 0))
    # what the contract excludes (must be refused by every configuration alike)
    r = _rand(9000)
    M, N, K = 129, 160, 96
    o = dict(a1=r(M, K, dtype=dtype), w1=r(N, K, sc=K ** -0.5, dtype=dtype), bias=r(N, sc=0.1))
    out.append(("x:splitk_without_atomic", (M, N, K, 0), G.make_case(**o, splitk=2), 0))
    out.append(("x:atomic_splitk+silu", (M, N, K, 0), G.make_case(**o, atomic=True, splitk=3, c0=1.0, act=G.ACT_SILU), 0))
    out.append(("atomic+rowbias+residual", (M, N, K, 0), G.make_case(**o, atomic=True, splitk=3, c0=1.0, rowbias=r(2, N, dtype=dtype),
                                                                      rows_per_batch=77, residual=r(M, N, dtype=dtype), beta=-0.5), 0))
    out.append(("x:geglu+residual", (M, N, K, 0), G.make_case(**o, act=G.ACT_GEGLU, residual=r(M, N, dtype=dtype), beta=1.0), 0))
    out.append(("x:geglu+alpha", (M, N, K, 0), G.make_case(**o, act=G.ACT_GEGLU, alpha=0.5), 0))
    out.append(("x:group_width_24", (M, 72, K, 32), G.make_case(r(M, K, dtype=dtype), r(72, K, dtype=dtype), a2=r(M, 96, dtype=dtype),
                                                                 w2=r(72, 32, dtype=dtype), a2_group_n=24), 0))
    out.append(("x:k_48" if dtype == BF else "k_48", (M, N, 48, 0), G.make_case(r(M, 48, dtype=dtype), r(N, 48, dtype=dtype), bias=r(N)), 0))
    out.append(("x:n_12", (M, 12, K, 0), G.make_case(r(M, K, dtype=dtype), r(12, K, dtype=dtype)), 0))
    return out


def _conv_cases(dtype):
    out = []
    i = 0
    for B, H, W in ((3, 5, 7), (2, 9, 6)):
        for mode, (Ho, Wo) in ((G.CONV_S1, (H, W)), (G.CONV_S2, ((H - 1) // 2 + 1, (W - 1) // 2 + 1)), (G.CONV_UP2, (2 * H, 2 * W)),
                               (G.CONV_T2, (2 * H, 2 * W))):
            K1, N = ((32, 160), (96, 72))[i % 2]
            i += 1
            r = _rand(7000 + i)
            M = B * Ho * Wo
            o = dict(a1=r(B * H * W, K1, dtype=dtype), w1=r(N, 9 * K1, sc=1.0 / (3 * K1 ** 0.5), dtype=dtype), bias=r(N, sc=0.1),
                     mode=mode, conv=(B, H, W, Ho, Wo))
            out.append((f"conv{mode}", (M, N, K1, 0), G.make_case(**o), 0))
            out.append((f"conv{mode}+rowbias+residual", (M, N, K1, 0),
                        G.make_case(**o, rowbias=r(B, N, dtype=dtype), rows_per_batch=Ho * Wo, residual=r(M, N, dtype=dtype), beta=1.0), 0))
    # AutoencoderKL's Downsample (pad (0, 1, 0, 1), stride 2): an even grid, a second one, and an odd grid, where the kernel never
    # reaches the pad row / column (2 Hout + 1 <= Hin) and the last input row / column is read by the last tap only
    for conv in ((3, 6, 10, 3, 5), (2, 8, 6, 4, 3), (2, 9, 7, 4, 3)):
        B, H, W, Ho, Wo = conv
        K1, N = ((32, 160), (96, 72))[i % 2]
        i += 1
        r = _rand(7000 + i)
        M = B * Ho * Wo
        o = dict(a1=r(B * H * W, K1, dtype=dtype), w1=r(N, 9 * K1, sc=1.0 / (3 * K1 ** 0.5), dtype=dtype), bias=r(N, sc=0.1),
                 mode=G.CONV_S2A, conv=conv)
        out.append((f"conv{G.CONV_S2A}", (M, N, K1, 0), G.make_case(**o), 0))
        out.append((f"conv{G.CONV_S2A}+rowbias+residual", (M, N, K1, 0),
                    G.make_case(**o, rowbias=r(B, N, dtype=dtype), rows_per_batch=Ho * Wo, residual=r(M, N, dtype=dtype), beta=1.0), 0))
    r = _rand(7100)
    out.append(("x:conv_k2", (105, 72, 32, 32), G.make_case(r(105, 32, dtype=dtype), r(72, 288, dtype=dtype), a2=r(105, 32, dtype=dtype),
                                                             w2=r(72, 32, dtype=dtype), mode=G.CONV_S1, conv=(3, 5, 7, 5, 7)), 0))
    return out


def _s2a_big(dtype, epilogue):
    """CONV_S2A at a size the whole-line kernels take themselves: K1 = 128 (whole 128-byte lines in both dtypes, K1 % 64 for the
    loader / consumer kernel), M = 2 x 16 x 8 = 256 > 128 output pixels in ONE 256-row tile that spans both images, N = 160."""
    conv = (2, 32, 16, 16, 8)
    B, H, W, Ho, Wo = conv
    K1, N, M = 128, 160, B * Ho * Wo
    r = _rand(7200 + (7 if dtype == F32 else 0))
    o = dict(a1=r(B * H * W, K1, dtype=dtype), w1=r(N, 9 * K1, sc=1.0 / (3 * K1 ** 0.5), dtype=dtype), bias=r(N, sc=0.1),
             mode=G.CONV_S2A, conv=conv)
    if epilogue:
        o.update(rowbias=r(B, N, dtype=dtype), rows_per_batch=Ho * Wo, residual=r(M, N, dtype=dtype), beta=1.0)
    return G.make_case(**o)


# SHAPES rows whose K1 (and K2) are whole 128-byte lines in bf16 too, so that the full-line, persistent and loader / consumer forms
# run them themselves in both dtypes: one from each third of the list, and one with a second K segment
_INPLACE_ROWS = (4, 10, 13)          # (63, 640, 320, 0), (257, 72, 1344, 0), (1000, 160, 320, 0)
_INPLACE_K2_ROW = 9                  # (257, 328, 320, 128)


def _inplace_cases(dtype):
    """[(name, shape, case, forced split-K)]: products with a residual, each launched out of place and in place."""
    out = []

    def lin(i, seed):
        M, N, K1, K2 = SHAPES[i]
        r = _rand(11000 + 10 * seed + (7 if dtype == F32 else 0))
        o = dict(a1=r(M, K1, dtype=dtype), w1=r(N, K1, sc=K1 ** -0.5, dtype=dtype), bias=r(N, sc=0.1), residual=r(M, N, dtype=dtype))
        if K2:
            o.update(a2=r(M, K2, dtype=dtype), w2=r(N, K2, sc=K2 ** -0.5, dtype=dtype))
        return (M, N, K1, K2), o, r

    for n, i in enumerate(_INPLACE_ROWS):
        shape, o, r = lin(i, n)
        out.append(("residual", shape, G.make_case(**o, alpha=0.7, beta=-0.5), 0))
    shape, o, r = lin(_INPLACE_K2_ROW, 3)
    out.append(("k2+residual", shape, G.make_case(**o, beta=1.0), 0))
    shape, o, r = lin(13, 4)
    nb = (shape[0] + 76) // 77
    out.append(("rowbias+residual+silu", shape, G.make_case(**o, rowbias=r(nb, shape[1], dtype=dtype), rows_per_batch=77, beta=1.0,
                                                            act=G.ACT_SILU), 0))
    shape, o, r = lin(4, 5)
    out.append(("residual+out_f32", shape, G.make_case(**o, alpha=0.7, beta=-0.5, out_f32=True), 0))
    # forced split-K: the slabs go through the workspace, the reduce launch reads the residual and writes C (K = 1344: 21 / 42 steps)
    shape, o, r = lin(10, 6)
    out.append(("splitk2+residual", shape, G.make_case(**o, alpha=0.7, beta=-0.5), 2))
    shape, o, r = lin(13, 7)
    out.append(("splitk5+residual", shape, G.make_case(**o, beta=1.0), 5))
    # 3x3: stride 1 (the ResnetBlock's conv2 onto the nin_shortcut output) and the Downsample mode, odd grid and whole-line size
    r = _rand(11900 + (7 if dtype == F32 else 0))
    for mode, conv, K1, N in ((G.CONV_S1, (3, 5, 7, 5, 7), 32, 160), (G.CONV_S1, (2, 16, 8, 16, 8), 128, 160),
                              (G.CONV_S2A, (2, 9, 7, 4, 3), 96, 72)):
        B, H, W, Ho, Wo = conv
        M = B * Ho * Wo
        out.append((f"conv{mode}+rowbias+residual", (M, N, K1, 0),
                    G.make_case(r(B * H * W, K1, dtype=dtype), r(N, 9 * K1, sc=1.0 / (3 * K1 ** 0.5), dtype=dtype), bias=r(N, sc=0.1),
                                mode=mode, conv=conv, rowbias=r(B, N, dtype=dtype), rows_per_batch=Ho * Wo,
                                residual=r(M, N, dtype=dtype), beta=1.0), 0))
    c = _s2a_big(dtype, True)
    out.append((f"conv{G.CONV_S2A}+rowbias+residual", (c["M"], c["N"], c["K1"], 0), c, 0))
    return out


def _twin_launch(c, cfg, sk):
    """The case out of place and in place under one forced configuration: (failures, figures of both, grids).  Every launch gets
    the four checks; the two guarded buffers -- guard rows and pad columns included -- must hold the same bits."""
    f, figs, grids = [], [], []
    guards = []
    for inplace in (False, True):
        if inplace and not _inplace_possible(c):
            break
        with _forced(cfg, sk):
            guard, n, grid = _launch_tagged(c, inplace)
        res = G.run_checks(c, guard.view, guard)
        _note("C_inplace" if inplace else "C", c, res)
        tag = "in place: " if inplace else ""
        f += [tag + x for x in G.failures(res)] + ([] if n == 1 else [f"{tag}launches={n}"])
        figs.append(res)
        grids.append(grid)
        guards.append(guard)
    if len(guards) == 2:
        if grids[0] != grids[1]:
            f.append(f"in place: another launch form {grids}")
        if not torch.equal(_bits(guards[0]), _bits(guards[1])):
            f.append("in place differs from out of place in %d elements" % int((_bits(guards[0]) != _bits(guards[1])).sum()))
    return f, figs, grids


def test_contract_excludes_is_a_predicate_on_the_case_alone():
    for fn in (_contract_excludes, _inplace_possible):
        code = fn.__code__
        assert code.co_argcount == 1 and code.co_varnames[0] == "c"
        assert not any("cfg" in n or "config" in n.lower() for n in code.co_names + code.co_varnames)


def test_inplace_cases_cover_what_they_name():
    """The literal list: residual rows from each third of SHAPES on whole 128-byte lines, a second K segment, rowbias + residual +
    SiLU, an fp32 output (in place in fp32 only: a bf16 residual and an fp32 C share no element), both forced split-K factors, conv
    S1 and conv S2A -- and nothing the contract excludes."""
    assert [i * 3 // len(SHAPES) for i in _INPLACE_ROWS] == [0, 1, 2] and SHAPES[_INPLACE_K2_ROW][3] > 0
    for i in _INPLACE_ROWS + (_INPLACE_K2_ROW,):
        assert SHAPES[i][2] % 64 == 0 and SHAPES[i][3] % 64 == 0, SHAPES[i]
    _need_gpu()
    for dtype in (BF, F32):
        cases = _inplace_cases(dtype)
        names = [n for n, _, _, _ in cases]
        assert {"residual", "k2+residual", "rowbias+residual+silu", "residual+out_f32", "splitk2+residual", "splitk5+residual",
                f"conv{G.CONV_S1}+rowbias+residual", f"conv{G.CONV_S2A}+rowbias+residual"} == set(names)
        for name, _, c, sk in cases:
            assert not _contract_excludes(c) and c["residual"] is not None
            assert _inplace_possible(c) == (not (name == "residual+out_f32" and dtype == BF)), name


def test_ids_outside_the_switch_are_refused():
    _need_gpu()
    from ctrlora_amd import hip
    r = _rand(3)
    c = G.make_case(r(129, 96, dtype=BF), r(160, 96, dtype=BF), bias=r(160))
    for cfg in NOT_CONFIGS:
        with _forced(cfg, 0):
            with pytest.raises(hip.HipError, match="code 1"):
                _launch(c)
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("cfg", CONFIGS)
def test_forced_configuration_across_the_contract(cfg, dtype):
    """Configuration `cfg` forced (cl_gemm_force_config) over the literal case list: every case inside the contract passes the four
    checks -- through the configuration's own kernel or through its fall-back -- and every case outside it is refused."""
    _need_gpu()
    from ctrlora_amd import hip
    bad, accepted, launches, worst = [], set(), 0, 0.0
    for name, shape, c, sk in _linear_cases(dtype) + _conv_cases(dtype):
        excluded = _contract_excludes(c)
        assert excluded == name.startswith("x:"), (name, excluded)
        try:
            with _forced(cfg, sk):
                guard, n, grid = _launch_tagged(c)
        except hip.HipError as e:
            if not excluded:
                bad.append((name, shape, "refused: " + str(e)))
            continue
        if excluded:
            bad.append((name, shape, "accepted a case the contract excludes"))
            continue
        res = G.run_checks(c, guard.view, guard)
        _note("C", c, res)
        launches += 1
        worst = max(worst, res["err_over_bound"])
        accepted.add(name)
        f = G.failures(res) + ([] if n == 1 else [f"launches={n}"])
        if f:
            bad.append((name, shape, f, {k: res[k] for k in ("rel", "gate", "violations", "err_over_bound", "first_violation",
                                                             "guard_rows", "pad_elems", "nan_left")}, grid))
    # the residual epilogues again, each out of place and IN PLACE (C == residual): the same four checks, the same launch form,
    # the same bits.  A configuration that refuses one of them contradicts "for every configuration" in the header.
    twins = 0
    for name, shape, c, sk in _inplace_cases(dtype):
        try:
            f, figs, grids = _twin_launch(c, cfg, sk)
        except hip.HipError as e:
            bad.append(("inplace:" + name, shape, "refused: " + str(e)))
            continue
        launches += len(figs)
        twins += len(figs) == 2
        worst = max([worst] + [r["err_over_bound"] for r in figs])
        if f:
            bad.append(("inplace:" + name, shape, f, [{k: r[k] for k in ("rel", "gate", "violations", "err_over_bound", "first_violation",
                                                                         "guard_rows", "pad_elems", "nan_left")} for r in figs], grids))
    _record("gemm_conformance_forced_config", cfg=cfg, dtype=str(dtype), launches=launches, err_over_bound=worst, inplace_twins=twins,
            failures=[str(b) for b in bad])
    assert set(ALWAYS) <= accepted, (cfg, sorted(set(ALWAYS) - accepted))
    assert twins == 12 - (dtype == BF), twins          # (every case but the bf16 product with an fp32 output)
    assert not bad, (cfg, bad)


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("cfg", [16, 17, 40, 41])
def test_s2a_on_the_whole_line_kernels(cfg, dtype):
    """CONV_S2A where the full-line ping-pong rows (16 / 17) and the loader / consumer rows (40 / 41) run it THEMSELVES instead of
    handing it to the generic tile: each has its own copy of the mode's address line.  Plain, and + rowbias + residual out of
    place and in place.  That the forced kernel ran is read off the tag table: both kernels launch 512 work items per workgroup
    on a grid of 256-row tiles; every tile this product could fall back to (the generic 128-row tiles, ids 1 / 2) launches 256.
    The loader / consumer kernel exists in bf16 only: in fp32 its rows hand the product to the rules, which is asserted too."""
    _need_gpu()
    from ctrlora_amd import hip
    bn = 160 if cfg in (16, 40) else 128
    own = dtype == BF or cfg in (16, 17)
    for epilogue in (False, True):
        c = _s2a_big(dtype, epilogue)
        assert not _contract_excludes(c) and c["M"] > 128 and c["N"] >= 96 and c["K1"] % 64 == 0
        f, figs, grids = _twin_launch(c, cfg, 0)
        tiles = ((c["M"] + 255) // 256) * ((c["N"] + bn - 1) // bn)
        _record("gemm_conformance_s2a_whole_line", cfg=cfg, dtype=str(dtype), epilogue=epilogue, grids=grids, own_kernel=own,
                err_over_bound=[r["err_over_bound"] for r in figs], rel=[r["rel"] for r in figs], failures=f)
        assert len(figs) == (2 if epilogue else 1)
        assert not f, (cfg, epilogue, f, figs)
        for wgs, wg_size in grids:
            if own:
                assert wg_size == 512 and wgs % tiles == 0, ("the forced kernel did not run", cfg, grids, tiles)
            else:
                assert wg_size == 256, ("fp32 has no loader / consumer kernel: the rules' generic tile", cfg, grids)


def test_zz_conformance_summary():
    """Per-layer maxima and the wall time of this file, for DESIGN.md."""
    _need_gpu()
    wall = None if _T0[0] is None else time.time() - _T0[0]
    print("gemm conformance:", json.dumps(_STATS), "wall_s:", wall)
    _record("gemm_conformance_summary", layers=_STATS, wall_s=wall, layer_a_entries=len(_ENTRIES), layer_b_cases=len(_UNTUNED),
            layer_c_configs=len(CONFIGS), inplace_twin_launches=_STATS.get("C_inplace", {}).get("launches", 0),
            # measured once on one MI355X, both files in the same run: this file before the CONV_S2A and in-place cases, and with them
            wall_s_before_s2a_and_inplace=14.8, wall_s_with_them=17.7)
    for layer, s in _STATS.items():
        assert s["violations"] == 0 and s["canary"] == 0 and s["err_over_bound"] <= 1.0, (layer, s)
