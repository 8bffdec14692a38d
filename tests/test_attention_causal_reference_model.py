"""The causal attention reference, rounding model and gate of tests/attn_causal_ref.py, checked on the CPU: the fp64 reference
against torch's own causal attention, the rounding model against the gate on every row, the written constants against
measure_constants(), and the gate against three wrong masks."""
import pytest
import torch

from tests import attn_causal_ref as R

_ROWS = {}


def _row(row):
    """(excess of the rounding model, case, fp64 reference) of a row: computed once, shared."""
    if row["name"] not in _ROWS:
        _ROWS[row["name"]] = R.measure_row(row)
    return _ROWS[row["name"]]


def _by_name(name):
    return next(r for r in R.CASES if r["name"] == name)


def test_case_table_covers_the_sizes_at_which_the_kernel_changes_path():
    assert len(R.CASES) == 2 * (2 * 9 + 1) and len({r["name"] for r in R.CASES}) == len(R.CASES)
    for dt in (R.BF, R.F32):
        rows = [r for r in R.CASES if r["dtype"] == dt]
        assert {(r["B"], r["H"]) for r in rows} == {(2, 2), (1, 12)}
        assert {r["N"] for r in rows} == {1, 16, 17, 63, 64, 65, 77, 127, 128}
        assert sum(r["q_std"] == 4.0 for r in rows) == 1


@pytest.mark.parametrize("name", ["f32-b2h2-n1", "f32-b2h2-n17", "f32-b1h12-n77", "f32-b2h2-n128", "bf16-b2h2-n77-q4"])
def test_reference_equals_torch_causal_attention_in_fp64(name):
    _, case, ref = _row(_by_name(name))
    B, H, N = case["B"], case["H"], case["N"]
    hd = lambda x: x.double().reshape(B, N, H, R.DH).permute(0, 2, 1, 3)
    want = torch.nn.functional.scaled_dot_product_attention(hd(case["q"]), hd(case["k"]), hd(case["v"]), is_causal=True)
    want = want.permute(0, 2, 1, 3).reshape(B * N, H * R.DH)
    assert float((ref["o"] - want).abs().max()) < 1e-12
    assert bool((ref["mag_o"] >= ref["o"].abs() - 1e-12).all()) and bool((ref["score_o"] >= 0).all())
    # row 0 of every head sees one key: the output is v[0]
    assert torch.equal(ref["o"].reshape(B, N, -1)[:, 0], case["v"].double().reshape(B, N, -1)[:, 0])


@pytest.mark.parametrize("row", R.CASES, ids=[r["name"] for r in R.CASES])
def test_rounding_model_passes_the_gate(row):
    _, case, ref = _row(row)
    res = R.check(R.causal_model(case, row["dtype"]), ref, row["dtype"])
    assert R.passes(res), res


def test_measured_constants_are_the_written_ones():
    worst = {R.BF: 0.0, R.F32: 0.0}
    for row in R.CASES:
        worst[row["dtype"]] = max(worst[row["dtype"]], _row(row)[0])
    for dt in (R.BF, R.F32):
        assert abs(worst[dt] - R.MEASURED[dt]) <= 2e-3 * R.MEASURED[dt] + 5e-4, (dt, worst[dt], R.MEASURED[dt])
        assert R.C_O[dt] == R.MARGIN * R.MEASURED[dt] and R.MARGIN == 3.0


@pytest.mark.parametrize("wrong", ["shifted", "nomask", "lastkey"])
@pytest.mark.parametrize("name", ["bf16-b2h2-n17", "bf16-b2h2-n65", "f32-b2h2-n17", "f32-b2h2-n65"])
def test_gate_rejects_a_wrong_mask(name, wrong):
    """An exact (fp64) output under the mask j <= i + 1, under no mask, and with each row's last key (the diagonal) dropped."""
    row = _by_name(name)
    _, case, ref = _row(row)
    N = case["N"]
    i, j = torch.arange(N)[:, None], torch.arange(N)[None, :]
    keep = {"shifted": j <= i + 1, "nomask": torch.ones(N, N, dtype=torch.bool), "lastkey": (j < i) | ((i == 0) & (j == 0))}[wrong]
    res = R.check(R.causal_ref64(case, keep)["o"], ref, row["dtype"])
    assert res["violations"] > 0 and res["err_over_bound"] > 2.0 and not R.passes(res), res
