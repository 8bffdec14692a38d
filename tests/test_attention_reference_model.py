"""CPU side of the attention conformance suite (tests/attn_ref.py): the fp64 reference is right (closed-form gradients vs
autograd), the rounding model passes the gate it calibrates on every row of the case table, the gate bites, and the table
names every launch form the GPU suite (tests/test_gpu_attention_conformance.py) must reach."""
import pytest
import torch

from tests import attn_ref as A


def _small_case(prescaled, dtype=torch.float64):
    g = torch.Generator().manual_seed(5)
    B, H, N, Nkv, dh = 2, 3, 9, 7, 8
    scale = dh ** -0.5
    mk = lambda n: torch.randn(B * n, H * dh, generator=g, dtype=torch.float64)
    q, k, v, do = mk(N), mk(Nkv), mk(Nkv), mk(N)
    return dict(B=B, H=H, N=N, Nkv=Nkv, dh=dh, scale=scale, prescaled=prescaled, dtype=dtype,
                q=q * (scale * A.LOG2E) if prescaled else q, k=k, v=v, do=do), q


@pytest.mark.parametrize("prescaled", [False, True])
def test_closed_form_gradients_match_fp64_autograd(prescaled):
    case, q_true = _small_case(prescaled)
    B, H, N, Nkv, dh = (case[x] for x in ("B", "H", "N", "Nkv", "dh"))
    ref = A.attn_ref64(case)
    leaf = lambda x, n: A._split(x, B, n, H, dh).clone().requires_grad_(True)
    qr, kr, vr = leaf(q_true, N), leaf(case["k"], Nkv), leaf(case["v"], Nkv)
    s = torch.einsum("bhid,bhjd->bhij", qr, kr) * case["scale"]
    o = s.softmax(-1) @ vr
    o.backward(A._split(case["do"], B, N, H, dh))
    for name, want in (("o", o.detach()), ("dq", qr.grad), ("dk", kr.grad), ("dv", vr.grad)):
        assert torch.allclose(ref[name], A._back(want), rtol=1e-11, atol=1e-13), name
    assert torch.allclose(ref["lse"], torch.logsumexp(s.detach(), -1) * A.LOG2E, rtol=1e-12, atol=1e-12)
    # every magnitude dominates its output: each is the same last contraction over absolute terms
    for name in ("o", "dq", "dk", "dv"):
        assert bool((ref["mag_" + name] >= ref[name].abs() * (1 - 1e-12)).all()), name


@pytest.mark.parametrize("group", A.GROUPS)
def test_rounding_model_passes_the_gate_on_every_row(group):
    """Every row, none skipped: the model's excess stays at or under the value the constants were measured as (so the written
    constants ARE 3 x the table's maximum), which is the gate with a factor 3 to spare."""
    rows = [r for r in A.CASES if A.group_of(r) == group]
    assert rows
    bad = []
    for row in rows:
        m, case, ref, mod = A.measure_row(row)
        dt = row["dtype"]
        for k, v in m.items():
            if not v <= A.MEASURED[dt][k] * 1.0005:
                bad.append((row["name"], k, v, A.MEASURED[dt][k]))
        res = A.check_outputs(case, ref, mod, dt)
        if A.failures(res):
            bad.append((row["name"], A.failures(res)))
    assert not bad, bad


def test_constants_are_three_times_what_was_measured_and_none_hides_a_weak_magnitude():
    for dt in (A.BF, A.F32):
        for k, v in A.MEASURED[dt].items():
            if k == "lse":
                assert A.LSE_BOUND[dt] == 3.0 * v
            else:
                assert A.C[dt][k] == 3.0 * v and 0 < v <= 4.0, (dt, k, v)
    assert A.LSE_BOUND[A.BF] < 3 * 2.82e-3 and A.LSE_BOUND[A.F32] < 2e-6


def test_the_gate_bites():
    """What the issue names: a mask one key off, V walked with another stride, one wrong element."""
    row = next(r for r in A.CASES if r["name"] == "tr1-dh16-70x77-plain")
    case = A.make_case(row)
    ref = A.attn_ref64(case)
    good = A.attn_model(case, A.BF)
    assert not A.failures(A.check_outputs(case, ref, good, A.BF))
    short = dict(case, Nkv=76, k=case["k"].reshape(2, 77, -1)[:, :76].reshape(2 * 76, -1), v=case["v"].reshape(2, 77, -1)[:, :76].reshape(2 * 76, -1))
    off = A.attn_model(short, A.BF, backward=False)
    assert A.check_outputs(case, ref, dict(o=off["o"]), A.BF)["o"]["violations"] > 0
    shifted = dict(case, v=torch.roll(case["v"], 1, 0))
    assert A.check_outputs(case, ref, dict(o=A.attn_model(shifted, A.BF, backward=False)["o"]), A.BF)["o"]["violations"] > 0
    one = good["dq"].clone()
    one[3, 5] += 40 * A.U[A.BF] * ref["mag_dq"][3, 5]
    assert A.check_outputs(case, ref, dict(dq=one), A.BF)["dq"]["violations"] == 1
    nan = good["dv"].clone()
    nan[0, 0] = float("nan")
    assert A.check_outputs(case, ref, dict(dv=nan), A.BF)["dv"]["violations"] == 1


@pytest.mark.parametrize("dh", [8, 160])
def test_the_fp32_gate_bites_and_how_loose_its_score_term_is(dh):
    """fp32 carries the worst-case score term (linear in d_head): a key mask one off and V one row off must still fail at both
    ends of the d_head range, and the smallest single-element error the gate catches is recorded in units of u |mag|."""
    row = next(r for r in A.CASES if r["name"] == f"t-f32-dh{dh}-70x77")
    case = A.make_case(row)
    ref = A.attn_ref64(case)
    good = A.attn_model(case, A.F32)
    assert not A.failures(A.check_outputs(case, ref, good, A.F32))
    short = dict(case, Nkv=76, k=case["k"].reshape(2, 77, -1)[:, :76].reshape(2 * 76, -1), v=case["v"].reshape(2, 77, -1)[:, :76].reshape(2 * 76, -1))
    res = A.check_outputs(case, ref, dict(o=A.attn_model(short, A.F32, backward=False)["o"]), A.F32)["o"]
    assert res["violations"] > 0.9 * ref["o"].numel() and res["err_over_bound"] > 50, res      # nearly every element, by far
    shifted = dict(case, v=torch.roll(case["v"], 1, 0))
    assert A.check_outputs(case, ref, dict(o=A.attn_model(shifted, A.F32, backward=False)["o"]), A.F32)["o"]["violations"] > 0
    # the looseness, quantified: bound / (u mag) over the outputs -- what multiple of one fp32 ulp of the terms a single wrong
    # element must exceed to be caught.  Median, measured: d_head 8: o 41, dv 48, dq 98, dk 105; d_head 160: o 2624, dv 2634,
    # dq 10601, dk 10553 (6e-4 of the terms: there rel-L2 at 5e-4 is the tighter gate).  The ceilings keep the term from growing.
    u = A.U[A.F32]
    slack = {}
    for k in ("o", "dq", "dk", "dv"):
        bound = u * ref[k].abs() + A.C[A.F32][k] * u * ref["mag_" + k] + ref["score_" + k]
        slack[k] = float((bound / (u * ref["mag_" + k])).median())
        one = good[k].clone()
        one[3, 5] += 2.0 * bound[3, 5]
        assert A.check_outputs(case, ref, {k: one}, A.F32)[k]["violations"] == 1
    print(f"fp32 gate slack at d_head {dh} (bound / u mag, median):", slack)
    lim = 150 if dh == 8 else 15000
    assert all(A.C[A.F32][k] <= v < lim for k, v in slack.items()), slack
    # in every case orders of magnitude under bf16's u: an fp32 kernel that rounded anything to bf16 fails
    assert A.failures(A.check_outputs(case, ref, dict(o=ref["o"].bfloat16()), A.F32))


def test_case_table_has_no_duplicates_and_names_every_form():
    names = [r["name"] for r in A.CASES]
    assert len(set(names)) == len(names)
    key = lambda r: (r["entry"], r["dtype"], r["dh"], r["B"], r["H"], r["N"], r["Nkv"], r["prescaled"], r["variant"], r["row_ws"],
                     r["q_std"], r["spike"])
    keys = [key(r) for r in A.CASES]
    assert len(set(keys)) == len(keys), [k for k in keys if keys.count(k) > 1]
    named = {f for r in A.CASES for f in r["forms"]}
    assert named == set(A.FORMS), named ^ set(A.FORMS)
    assert {A.group_of(r) for r in A.CASES} == set(A.GROUPS)
    # the issue's shape list: every d_head x the tail set in both bf16 contracts and in fp32
    for dh in A.ALL_DH:
        for N, Nkv in A.TAILSET:
            assert any(r["entry"] == "t" and r["dtype"] == A.F32 and (r["dh"], r["N"], r["Nkv"]) == (dh, N, Nkv) for r in A.CASES)
            for pre in (False, True):
                assert any(r["entry"] == "v2" and (r["dh"], r["N"], r["Nkv"], r["prescaled"]) == (dh, N, Nkv, pre) for r in A.CASES)
    # all four TQ x TK forms of the backward at every d_head: transpose-free in both q contracts, and fp32 transposed
    for dh in A.ALL_DH:
        for tq in (False, True):
            for tk in (False, True):
                hit = lambda r: (r["dh"], r["N"] % 64 != 0, r["Nkv"] % 64 != 0) == (dh, tq, tk)
                bits = (A.BIT_TQ if tq else 0) | (A.BIT_TK if tk else 0)
                for pre in (False, True):
                    assert any(hit(r) and r["entry"] == "v2" and r["prescaled"] == pre and r["bwd"]["dq_frags"] == 1
                               and r["bwd"]["bits"] == bits for r in A.CASES), (dh, tq, tk, pre)
                assert any(hit(r) and r["entry"] == "t" and r["dtype"] == A.F32 and r["bwd"]["bits"] == bits for r in A.CASES), (dh, tq, tk)
    for N, Nkv in A.TAILSET:
        assert any(r["entry"] == "t" and r["dtype"] == A.BF and (r["N"], r["Nkv"]) == (N, Nkv) for r in A.CASES)
    for r in A.CASES:
        assert r["B"] >= 2 and r["fwd"]["kind"] == 1 and r["bwd"]["kind"] == 2, r["name"]


def test_rel_l2_of_an_identically_zero_gradient_is_taken_against_its_terms():
    """Nkv = 1: dq = dk = 0 by the contract; the fp64 reference is cancellation noise and no relative error exists against it."""
    row = next(r for r in A.CASES if r["name"] == "tr1-dh32-1x1-plain")
    case = A.make_case(row)
    ref = A.attn_ref64(case)
    assert float(ref["dq"].abs().max()) < 1e-12 and float(ref["dk"].abs().max()) < 1e-12
    noise = dict(dq=1e-6 * A.U[A.BF] * ref["mag_dq"], dk=1e-6 * A.U[A.BF] * ref["mag_dk"], dv=ref["dv"].bfloat16())
    res = A.check_outputs(case, ref, noise, A.BF)
    assert res["dq"]["degenerate"] and res["dk"]["degenerate"] and not res["dv"]["degenerate"] and not A.failures(res)
    wrong = dict(dq=0.05 * ref["mag_dq"])
    assert {f[1] for f in A.failures(A.check_outputs(case, ref, wrong, A.BF))} == {"elementwise", "rel_l2"}
    other = A.attn_ref64(A.make_case(next(r for r in A.CASES if r["name"] == "tr1-dh32-129x3-plain")))
    assert not A.gate(other["dq"], other["dq"], other["mag_dq"], A.U[A.BF], 1.0)["degenerate"]
