"""CPU side of the x-stationary conformance suite (no GPU): the fp64 contract of the two forms only
csrc/gemm_xs.hip has (tests/gemm_ref.py: act = ACT_GEGLU_SPLIT, the LayerNorm prologue) against plain torch, the rounding model
of the kernel (tests/xs_ref.py) through the checks at every row of the GPU table, one negative control per mistake this
kernel can make, the transcription of its launcher -- what the table reaches is asserted from it -- and the refusals, which the
library decides on the host before any launch."""
import ctypes
import math

import pytest
import torch

from tests import gemm_ref as G
from tests import xs_ref as X

BF, F32 = torch.bfloat16, torch.float32
_ROWS = {r["name"]: r for r in X.CASES}


def _gen(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc


# ------------------------------------------------------------------------------------------------ the contract against plain torch

def test_reference_layernorm_prologue_vs_plain_torch():
    F = torch.nn.functional
    r = _gen(1)
    M, N, K = 37, 64, 320
    x, w = (r(M, K, sc=1.7) + 0.6).to(BF), r(N, K, sc=K ** -0.5).to(BF)
    gamma, beta, bias = 1 + r(K, sc=0.3), r(K, sc=0.3), r(N)
    for eps in (1e-5, 1e-6):
        xn = F.layer_norm(x.double(), (K,), gamma.double(), beta.double(), eps).to(BF).double()
        want = (xn @ w.double().t() + bias.double()) * 0.31
        c = G.make_case(x, w, bias=bias, alpha=0.31, ln=(gamma, beta, eps))
        got = G.gemm_ref64(c)
        assert float((got - want).abs().max()) < 1e-12
        P = G.ln_parts(c)
        assert torch.equal(P["xn"], xn)
        assert float((P["mean"] - x.double().mean(1)).abs().max()) < 1e-14
        assert float((P["rstd"] - (x.double().var(1, unbiased=False) + eps).rsqrt()).abs().max()) < 1e-11
        # the magnitude of check 2 is the same product on |xn|, |w|, |bias|
        mag = G.gemm_ref64(c, absolute=True)
        assert float((mag - (xn.abs() @ w.double().abs().t() + bias.double().abs()) * 0.31).abs().max()) < 1e-12
        assert G.k_total(c) == K + 2


def test_reference_geglu_split_vs_plain_torch():
    F = torch.nn.functional
    r = _gen(2)
    M, N, K, K2 = 29, 192, 320, 128
    x, w, t, b = r(M, K).to(BF), r(N, K, sc=K ** -0.5).to(BF), r(M, K2).to(BF), r(N, K2, sc=K2 ** -0.5).to(BF)
    bias = r(N)
    h = x.double() @ w.double().t() + t.double() @ b.double().t() + bias.double()
    want = h[:, :N // 2] * F.gelu(h[:, N // 2:])
    c = G.make_case(x, w, a2=t, w2=b, bias=bias, act=G.ACT_GEGLU_SPLIT)
    assert c["out_cols"] == N // 2 and G.k_total(c) == K + K2 + 7
    assert float((G.gemm_ref64(c) - want).abs().max()) < 1e-12
    # ... which is the tile-interleaved layout of act 2 at one 160-row tile and no longer at two
    w320 = r(320, K, sc=K ** -0.5).to(BF)
    both = lambda n: [G.gemm_ref64(G.make_case(x, w320[:n], act=a)) for a in (G.ACT_GEGLU, G.ACT_GEGLU_SPLIT)]
    assert torch.equal(*both(160)) and not torch.allclose(*both(320))
    # prologue and split GEGLU together
    gamma, beta = 1 + r(K, sc=0.3), r(K, sc=0.3)
    xn = F.layer_norm(x.double(), (K,), gamma.double(), beta.double(), 1e-5).to(BF).double()
    h = xn @ w.double().t() + bias.double()
    c4 = G.make_case(x, w, bias=bias, act=G.ACT_GEGLU_SPLIT, ln=(gamma, beta, 1e-5))
    assert float((G.gemm_ref64(c4) - h[:, :N // 2] * F.gelu(h[:, N // 2:])).abs().max()) < 1e-12


def test_derived_gelu_bound_covers_the_fp32_model_of_the_code():
    """dgelu_as is derived from the code's operations (tests/gemm_ref.py); the fp32 transcription of those operations must lie
    inside it at every gate value, and the bound must stay far below the bf16 rounding it sits beside."""
    g = torch.cat([torch.linspace(-14, 14, 200001), torch.randn(100000, generator=torch.Generator().manual_seed(3)) * 2]).to(F32)
    exact = 0.5 * g.double() * (1.0 + torch.erf(g.double() * 0.5 ** 0.5))
    err = (X._gelu_as32(g).double() - exact).abs()
    bound = G.dgelu_as(g.double())
    ratio = float((err / bound).max())
    print("gelu_as model: worst err / derived bound", ratio, "largest bound", float(bound.max()))
    assert ratio <= 1.0, ratio
    assert float(bound.max()) < 2e-5                      # |g| 1.5e-7 / 2 dominates: 1e-6 at |g| = 14


def test_ambiguity_marks_exactly_the_elements_near_a_tie():
    r = _gen(4)
    K = 320
    x = (r(64, K, sc=1.7) + 0.6).to(BF)
    gamma, beta = torch.ones(K), torch.zeros(K)
    c = G.make_case(x, r(32, K).to(BF), ln=(gamma, beta, 1e-5))
    P = G.ln_parts(c)
    # bf16 neighbours 1.0 and 1.0078125: ulp 2^-7; 3.0 -> 2^-6; 0.75 -> 2^-8
    v = torch.tensor([1.0, 1.5, 3.0, 0.75, -0.75, 0.0], dtype=torch.float64)
    assert G.ulp_bf16(v).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -8, 0.0]
    # every flagged element carries one ulp of xn, and only a small share of elements is flagged at all
    amb = P["amb_ulp"] != 0
    assert torch.equal(P["amb_ulp"][amb], G.ulp_bf16(P["xn"])[amb])
    assert 0 < int(amb.sum()) < 0.002 * amb.numel(), int(amb.sum())


# ------------------------------------------------------------------------------------------------ the model through the checks

_CPU_STATS = {}


@pytest.mark.parametrize("family", X.FAMILIES)
def test_rounding_model_passes_the_checks_at_every_row_of_the_gpu_table(family):
    """xs_model (the kernel's order of operations, fp32) through checks 1 - 3 and the statistics gate at every row; the
    ambiguous-row cap is a condition on the inputs and is asserted here from the reference alone."""
    worst = dict(err_over_bound=0.0, rel=0.0, amb_rows=0.0, stat=0.0, rows=0)
    for row in X.CASES:
        if row["family"] != family:
            continue
        c = X.build_case(row)
        out, stats = X.xs_model(c)
        guard = G.Guarded(c["M"], c["out_cols"], c["out_dtype"], "cpu")
        guard.view.copy_(out)
        res = G.run_checks(c, guard.view, guard)
        assert G.failures(res) == [], (row["name"], res)
        worst["err_over_bound"] = max(worst["err_over_bound"], res["err_over_bound"])
        worst["rel"] = max(worst["rel"], res["rel"])
        worst["rows"] += 1
        if c["ln"] is not None:
            assert res["amb_rows"] <= X.AMB_ROW_CAP, (row["name"], res["amb_rows"])
            sg = X.stats_gate(c, stats)
            assert sg["violations"] == 0, (row["name"], sg)
            worst["amb_rows"] = max(worst["amb_rows"], res["amb_rows"])
            worst["stat"] = max(worst["stat"], sg["err_over_bound"])
    assert worst["rows"] >= 15
    _CPU_STATS[family] = worst
    print("xs model", family, worst)


def test_measured_constant_is_what_the_model_needs():
    """MEASURED is the model's own need (python -m tests.xs_ref prints it); nothing was fitted to a kernel's output."""
    w = X.measure_constants()
    need = max(v for v, _ in w.values())
    print("xs statistics constant:", w)
    # (5 % either way: the host's own rsqrt may differ in the last bit from the one the figure was taken with)
    assert 0.95 * X.MEASURED["stat"] <= need <= 1.05 * X.MEASURED["stat"], (w, X.MEASURED)
    assert abs(w["mean"][0] - X.MEASURED["mean"]) <= 0.05 * X.MEASURED["stat"] and abs(w["rstd"][0] - X.MEASURED["rstd"]) <= 0.05 * X.MEASURED["stat"]
    assert X.C_STAT_XS == X.MARGIN * X.MEASURED["stat"]


# ------------------------------------------------------------------------------------------------ negative controls

def _control(name, fault):
    c = X.build_case(_ROWS[name])
    out, stats = X.xs_model(c, fault=fault)
    res = G.run_checks(c, out)
    sg = X.stats_gate(c, stats) if stats is not None else None
    print("control %-22s on %-40s rel_l2 %.3e (gate %.1e)  violations %d  rows hit %s  stats violations %s" % (
        fault, name, res["rel"], res["gate"], res["violations"], (res["first_violation"] or {}).get("rows_hit"),
        None if sg is None else sg["violations"]))
    return c, res, sg


@pytest.mark.parametrize("fault,name", [("half_mean", "ln320-plain-M129-b3-s1-nostats"), ("half_var", "ln640-geglu-M129-b3-s1"),
                                        ("affine_shift", "ln320-plain-M129-b3-s1-nostats"), ("affine_shift", "ln640-geglu-M129-b3-s1")])
def test_a_wrong_prologue_is_flagged_by_the_elementwise_check(fault, name):
    """The partner half-row lost from the mean or from the variance; gamma | beta read one 8-element half k-step off."""
    c, res, sg = _control(name, fault)
    assert "elementwise" in G.failures(res), res
    assert res["first_violation"]["rows_hit"] == c["M"]
    if fault != "affine_shift":
        assert sg["violations"] >= c["M"], sg                      # and by the statistics gate on every row


@pytest.mark.parametrize("fault,name", [("swap_halves", "k320+0-geglu-M300-b2-s1"), ("gate_bias_from_value", "k320+128-geglu-M300-b3-s1"),
                                        ("gate_bias_from_value", "ln320-geglu-M129-b1-s1")])
def test_a_wrong_geglu_half_is_flagged_by_the_elementwise_check(fault, name):
    c, res, _ = _control(name, fault)
    assert "elementwise" in G.failures(res), res
    assert res["first_violation"]["rows_hit"] == c["M"]


def test_a_block_stored_with_its_neighbours_residual_is_flagged():
    c, res, _ = _control("k320+0-res-M300-b2-s1-beta-0.5", "prev_residual")
    assert "elementwise" in G.failures(res) and res["first_violation"]["col"] >= 32, res
    assert res["violations"] > 0.9 * 32 * c["M"]


@pytest.mark.parametrize("name", ["k320+0-res-M129-b3-s1-inplace-beta-0.5", "k640+128-res-M300-b4-s1-inplace"])
def test_the_residual_applied_twice_on_one_row_is_flagged(name):
    """What the in-place race of the duplicate rows would store: acc + beta (acc + beta r) on ONE row: every element of that row
    and no other.  (The whole-matrix rel-L2 printed beside it sees one row of 129 or 300; of the 4100 rows of the older test's
    in-place case it is 1 / 64 of that, below its gate.)"""
    c, res, _ = _control(name, "double_residual")
    assert "elementwise" in G.failures(res), res
    assert res["first_violation"]["row"] == c["M"] // 2 and res["first_violation"]["rows_hit"] == 1
    assert res["violations"] > 0.9 * c["N"]


def test_the_last_k_step_of_the_second_segment_dropped_in_one_block_is_flagged():
    c, res, _ = _control("k320+128-plain-M129-b3-s1", "drop_k2_tail")
    assert "elementwise" in G.failures(res), res
    assert 32 <= res["first_violation"]["col"] < 64 and res["violations"] > 0.5 * 32 * c["M"]


def test_alpha_on_the_block_that_starts_at_alpha_n_is_flagged():
    c, res, _ = _control("k640+0-plain-M300-b5-s1-alpha_mid", "alpha_block")
    assert "elementwise" in G.failures(res), res
    assert 96 <= res["first_violation"]["col"] < 128 and res["violations"] > 0.9 * 32 * c["M"]


def test_a_row_of_statistics_left_unwritten_is_flagged_by_the_statistics_gate():
    c, res, sg = _control("ln320-plain-M129-b4-s4", "stats_unwritten")
    assert G.failures(res) == []                                  # the product itself is right
    assert sg["violations"] == 2 and sg["first"][1]["index"] == c["M"] // 2, sg


# ------------------------------------------------------------------------------------------------ what the table reaches

def test_table_reaches_every_instance_ring_phase_and_accumulator_residue():
    cov = X.coverage()
    assert {t[1] for t in cov if t[0] == "instance"} == set(X.INSTANCES) and len(X.INSTANCES) == 16
    # nch below, at and above D = RING - 1 for both ring depths (nch < D needs D = 2, i.e. the 3-slot ring: nch = 1; the
    # 2-slot ring has D = 1 and nch >= 1, so "below" does not exist there)
    assert {(3, "nch<D"), (3, "nch=D"), (3, "nch>D"), (2, "nch=D"), (2, "nch>D")} <= {(t[1], t[2]) for t in cov if t[0] == "ring"}
    # every residue of nch mod NACC: plain / residual NACC = 2 over chunks = blocks; GEGLU NACC = 4 over chunks = 2 blocks -> 0, 2
    assert {(2, 0), (2, 1), (4, 0), (4, 2)} == {(t[1], t[2]) for t in cov if t[0] == "nacc"}
    # a run longer than the bias image, re-split by the launcher, for every epilogue and for the prologue
    assert {("plain", False), ("res", False), ("geglu", False), ("plain", True), ("geglu", True)} <= {t[1:] for t in cov if t[0] == "resplit"}
    for inst in X.INSTANCES:
        assert {t[2] for t in cov if t[0] == "M" and t[1] == inst} == set(X.MS), inst
        assert ("runs>1", inst) in cov and ("forced_count_clamped", inst) in cov, inst
        if inst[2] != X.XS_GEGLU:
            assert ("alpha_n_mid_run", inst) in cov, inst
            if inst[1]:
                assert {t[2] for t in cov if t[0] == "grouped" and t[1] == inst} == {1, 2}, inst
    # in place at one full block, with three copy waves (129) and with one (300 = 2 x 128 + 44): every residual instance
    for inst in X.INSTANCES:
        if inst[2] == X.XS_RES:
            assert {t[2] for t in cov if t[0] == "inplace" and t[1] == inst} == {128, 129, 300}, inst


def test_run_rule_transcription_on_the_forms_the_engine_launches():
    """The tabled / production shapes the old test names, by hand from launch_xs."""
    base = dict(act=G.ACT_NONE, mode=G.LINEAR, bf16=True, alpha=1.0, alpha_n=0, a1_group_n=0, a2_group_n=0, residual=False, rowbias=False,
                atomic=False, out_f32=False, splitk=1, ln=False, ln_beta=True, inplace=False)
    call = lambda M, N, K1, K2, **kw: dict(dict(base, M=M, N=N, K1=K1, K2=K2, lda1=K1, ldw1=K1, ldc=N, lda2=K2, ldw2=K2, ldr=N), **kw)
    f = X.xs_form(call(256, 3200, 320, 0), 1)                      # 100 blocks: the bias image holds 80 -> 2 runs of 50
    assert (f["nsplit"], f["cpw"], f["resplit"], f["workgroups"]) == (2, 50, True, 4)
    f = X.xs_form(call(32768, 2560, 320, 0), 0)                    # 256 row blocks: 512 wanted, 80 -> 2 x 40
    assert (f["nsplit"], f["cpw"]) == (2, 40)
    f = X.xs_form(call(8192, 5120, 640, 128), 0)                   # 64 row blocks, one workgroup per CU: 256 wanted -> 4 x 40
    assert (f["nsplit"], f["cpw"], f["RING"], f["NACC"]) == (4, 40, 3, 2)
    f = X.xs_form(call(1000, 960, 320, 128, a2_group_n=320, alpha=0.31, alpha_n=320), 0)
    assert (f["groups"], f["bpg"], f["nsplit"], f["cpw"], f["RING"], f["workgroups"]) == (3, 10, 2, 5, 2, 8 * 3 * 2)
    f = X.xs_form(call(4096, 2560, 320, 0, act=G.ACT_GEGLU_SPLIT, ldc=1280), 0)     # 40 GEGLU blocks = 80 chunks
    assert (f["nsplit"], f["cpw"], f["nch"], f["NACC"]) == (8, 5, 10, 4)
    f = X.xs_form(call(128, 2624, 320, 0, act=G.ACT_GEGLU_SPLIT, ldc=1312), 1)       # 41 blocks, prime: one block per workgroup
    assert (f["nsplit"], f["cpw"], f["resplit"]) == (41, 1, True)
    assert f["smem"] <= 3 * 32 * 20 * 32 + 2560 * 4


# ------------------------------------------------------------------------------------------------ refusals, decided on the host

def _params(hip, p, fake):
    """cl_gemm_params of a transcription call; every pointer the call needs points at the same scrap of host memory (never read:
    the rows of this table are refused before any launch)."""
    q = hip.GemmParams()
    q.A1 = fake; q.lda1 = p["lda1"]; q.K1 = p["K1"]; q.W1 = fake; q.ldw1 = p["ldw1"]
    if p["K2"]:
        q.A2 = fake; q.lda2 = p["lda2"]; q.K2 = p["K2"]; q.W2 = fake; q.ldw2 = p["ldw2"]
    q.M = p["M"]; q.N = p["N"]; q.mode = p["mode"]
    if p["mode"] != G.LINEAR:
        q.B, q.Hin, q.Win, q.Hout, q.Wout = 1, 16, 16, 16, 16
        q.zero_page = fake
    q.bias = fake
    if p["rowbias"]:
        q.rowbias = fake; q.ldrb = p["N"]; q.rows_per_batch = 64
    if p["residual"]:
        q.residual = fake; q.ldr = p["ldr"]
    q.alpha = p["alpha"]; q.beta = 1.0 if p["residual"] else 0.0; q.act = p["act"]
    q.C = fake; q.ldc = p["ldc"]; q.out_f32 = int(p["out_f32"]); q.atomic = int(p["atomic"]); q.splitk = p["splitk"]
    q.a1_group_n = p["a1_group_n"]; q.a2_group_n = p["a2_group_n"]; q.alpha_n = p["alpha_n"]
    if p["ln"]:
        q.ln_gamma = fake; q.ln_beta = fake if p["ln_beta"] else None; q.ln_eps = 1e-5; q.ln_stats = fake
    return q


def _refusal_rows():
    base = dict(M=256, N=128, K1=320, K2=0, act=G.ACT_NONE, mode=G.LINEAR, bf16=True, alpha=1.0, alpha_n=0, a1_group_n=0, a2_group_n=0,
                residual=False, rowbias=False, atomic=False, out_f32=False, splitk=1, ln=False, ln_beta=True, inplace=False)

    def call(kind, **kw):
        p = dict(base, **({"act": G.ACT_GEGLU_SPLIT} if kind == "act3" else {"ln": True} if kind == "ln" else
                          {"act": G.ACT_GEGLU_SPLIT, "ln": True}))
        p.update(kw)
        out_cols = p["N"] // 2 if p["act"] == G.ACT_GEGLU_SPLIT else p["N"]
        groups = p["N"] // p["a2_group_n"] if p["a2_group_n"] > 0 else 1
        for k, v in (("lda1", p["K1"]), ("ldw1", p["K1"]), ("ldc", out_cols), ("lda2", groups * p["K2"]), ("ldw2", p["K2"]), ("ldr", p["N"])):
            p.setdefault(k, v)
        return p

    rows = []
    for kind in ("act3", "ln", "ln+act3"):
        rows += [(kind + ": M < 128", call(kind, M=127)), (kind + ": fp32", call(kind, bf16=False)),
                 (kind + ": K1 = 448", call(kind, K1=448)), (kind + ": lda1 % 8", call(kind, lda1=324)),
                 (kind + ": ldw1 % 8", call(kind, ldw1=324)), (kind + ": ldc % 8", call(kind, ldc=132)),
                 (kind + ": alpha_n < 0", call(kind, alpha=0.5, alpha_n=-32)), (kind + ": alpha_n > N", call(kind, alpha=0.5, alpha_n=160)),
                 (kind + ": rowbias", call(kind, rowbias=True)), (kind + ": conv mode", call(kind, mode=G.CONV_S1)),
                 (kind + ": out_f32", call(kind, out_f32=True)), (kind + ": a1_group_n", call(kind, a1_group_n=64)),
                 (kind + ": residual", call(kind, residual=True))]
    rows += [("ln: N % 32", call("ln", N=48)), ("ln: N % 32 (N = 80)", call("ln", N=80)), ("act3: N % 64", call("act3", N=96)),
             ("ln+act3: N % 64", call("ln+act3", N=96)),
             ("ln: alpha_n % 32", call("ln", alpha=0.5, alpha_n=8)), ("ln: alpha_n % 32 (alpha_n = 48)", call("ln", alpha=0.5, alpha_n=48)),
             ("act3: alpha != 1", call("act3", alpha=0.5)), ("act3: alpha_n", call("act3", alpha_n=32)),
             ("act3: a2_group_n", call("act3", K2=128, a2_group_n=64)), ("act3: K2 = 64", call("act3", K2=64)),
             ("act3: lda2 % 8", call("act3", K2=128, lda2=132)), ("act3: ldw2 % 8", call("act3", K2=128, ldw2=132)),
             ("ln: K2", call("ln", K2=128)), ("ln+act3: K2", call("ln+act3", K2=128)),
             ("ln: no ln_beta", call("ln", ln_beta=False)), ("ln+act3: no ln_beta", call("ln+act3", ln_beta=False))]
    return rows


def test_refusals_of_the_x_stationary_only_forms_are_decided_on_the_host():
    """Every restriction include/ctrlora_hip.h lists for act 3 and the LayerNorm prologue returns CL_EINVAL before anything
    touches a GPU, and the transcription agrees row by row."""
    from ctrlora_amd import hip
    L = hip.lib()
    buf = ctypes.create_string_buffer(64)
    fake = ctypes.addressof(buf)
    rows = _refusal_rows()
    assert len(rows) == 55 and len({n for n, _ in rows}) == 55
    got = []
    for name, p in rows:
        assert X.accepts(p) == "refused", ("the transcription would launch this row: it is not sent to the library", name)
        rc = L.cl_gemm(ctypes.byref(_params(hip, p, fake)), hip.BF16 if p["bf16"] else hip.F32, None)
        got.append((name, rc))
    assert [n for n, rc in got if rc != 1] == [], got
    assert L.cl_gemm(None, hip.BF16, None) == 1


def test_host_predicates_never_promise_what_the_launcher_refuses():
    """hip.xs_ln_ok / hip.xs_geglu_ok decide in the engine whether a block takes the one-launch forms: true only where the
    launcher (its transcription) takes the call with the engine's contiguous operands."""
    from ctrlora_amd import hip
    base = dict(mode=G.LINEAR, bf16=True, alpha=1.0, alpha_n=0, a1_group_n=0, a2_group_n=0, residual=False, rowbias=False, atomic=False,
                out_f32=False, splitk=1, ln_beta=True, inplace=False)
    yes = 0
    for M in (1, 64, 127, 128, 129, 300, 4096, 8192):
        for K in (64, 320, 448, 640, 1280):
            for N in (8, 32, 48, 64, 96, 320, 2560, 2592, 5120):
                for act in (G.ACT_NONE, G.ACT_SILU, G.ACT_GEGLU_SPLIT):
                    oc = N // 2 if act == G.ACT_GEGLU_SPLIT else N
                    p = dict(base, M=M, N=N, K1=K, K2=0, act=act, ln=True, lda1=K, ldw1=K, ldc=oc, lda2=0, ldw2=0, ldr=N)
                    if hip.xs_ln_ok(M, N, K, act):
                        yes += 1
                        assert oc % 8 == 0 and X.accepts(p) == "xs", (M, N, K, act)
            for r in (0, 64, 128, 256):
                if hip.xs_geglu_ok(M, K, r):
                    yes += 1
                    for N in (64, 640, 2560, 5120):           # (inner = 4 dim: N = 8 dim is a multiple of 64 at every level)
                        p = dict(base, M=M, N=N, K1=K, K2=r, act=G.ACT_GEGLU_SPLIT, ln=False, lda1=K, ldw1=K, ldc=N // 2, lda2=r, ldw2=r, ldr=N)
                        assert X.accepts(p) == "xs", (M, N, K, r)
    assert yes > 50, yes


def test_zz_cpu_model_summary():
    if len(_CPU_STATS) == len(X.FAMILIES):
        print("xs model, all families: worst err / bound %.3f, worst rel-L2 %.2e, worst ambiguous-row share %.4f, worst statistics err / bound %.3f"
              % (max(s["err_over_bound"] for s in _CPU_STATS.values()), max(s["rel"] for s in _CPU_STATS.values()),
                 max(s["amb_rows"] for s in _CPU_STATS.values()), max(s["stat"] for s in _CPU_STATS.values())))
        assert max(s["err_over_bound"] for s in _CPU_STATS.values()) <= 1.0
