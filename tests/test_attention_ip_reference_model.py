"""The image-prompt attention reference, rounding model and gate of tests/attn_ip_ref.py, checked on the CPU: the fp64 reference
against the fp64 torch arithmetic of the reference's IPCrossAttention (tests/test_gpu_style_ip.py:_ref), the rounding model against
the gate on every row, the written constants against measure_constants(), and the gate against eight planted defects, each evaluated
in the rounding model on named rows."""
import pytest
import torch

from tests import attn_ip_ref as R
from tests.test_gpu_style_ip import _ref as torch_ip_ref

_ROWS = {}


def _row(row):
    """(excess of the rounding model, case, fp64 reference) of a row: computed once, shared, never modified."""
    if row["name"] not in _ROWS:
        _ROWS[row["name"]] = R.measure_row(row)
    return _ROWS[row["name"]]


def test_case_table_is_the_one_the_suite_was_written_for():
    names = [r["name"] for r in R.CASES]
    assert len(names) == len(set(names)) == 6 * 9 * 3 + 2 + 5 * 3 + 1 + 2 * 3 * 2
    tail = [r for r in R.CASES if r["B"] == 2 and r["q_std"] == 1.0 and "t32" not in r["name"]]
    for dt, pre in ((R.BF, False), (R.BF, True), (R.F32, False)):
        rows = [r for r in tail if r["dtype"] == dt and r["prescaled"] == pre]
        assert {(r["dh"], r["N"], r["Nkv"], r["Nip"]) for r in rows} == {(dh,) + t for dh in R.ALL_DH for t in R.TAILSET}
        assert all(r["H"] == 2 and r["fwd_frags"] == 1 for r in rows)
        for dh in R.ALL_DH:                                          # every d_head of every variant sees every ip_scale
            assert {r["ip_scale"] for r in rows if r["dh"] == dh} == set(R.IP_SCALES)
    for t in R.TAILSET:                                              # ... and so does every shape
        assert {r["ip_scale"] for r in tail if (r["N"], r["Nkv"], r["Nip"]) == t and r["dtype"] == R.BF} == set(R.IP_SCALES)
    assert {(r["Nkv"] + 63) // 64 for r in tail} == {1, 2, 3}        # the image-prompt tile in either LDS buffer
    assert sorted(r["name"] for r in R.CASES if r["q_std"] == 4.0) == ["bf16-dh40-65x77x16-std4", "f32-dh40-65x77x16-std4"]
    two = [r for r in R.CASES if r["B"] > 2]
    assert all(r["dtype"] == R.BF and r["H"] == 8 for r in two)
    for r in two:                                                    # the table NAMES the form; this is the documented rule beside it
        assert r["fwd_frags"] == (2 if r["dh"] <= 80 and (r["N"] + 127) // 128 * r["H"] * r["B"] >= 512 else 1), r["name"]
    assert {(r["dh"], r["B"], r["N"], r["Nkv"], r["Nip"], r["fwd_frags"]) for r in two} == (
        {(dh, 32, 130, 77, 4, 2) for dh in (8, 16, 32, 40, 80)} | {(dh, 32, 255, 77, 64, 2) for dh in (8, 16, 32, 40, 80)}
        | {(dh, 31, 130, 77, 4, 1) for dh in (8, 16, 32, 40, 80)} | {(160, 32, 130, 77, 4, 1)})
    edges = [r for r in R.CASES if "t32" in r["name"]]
    assert {(r["dh"], r["N"], r["Nkv"], r["Nip"], r["vt_pads"]) for r in edges} == {
        (dh, 65, nkv, nip, (R.rup(nkv) + e, ld2)) for dh in (80, 160) for nkv, nip in ((32, 32), (33, 33), (77, 64))
        for e, ld2 in ((0, 64), (64, 128))}
    assert all(r["tile"] == (32 if r["dh"] >= 80 else 64) for r in R.CASES if r["dtype"] == R.F32)


@pytest.mark.parametrize("name", ["f32-dh8-1x1x1", "f32-dh40-65x77x4", "bf16-dh40-65x77x4-pre", "bf16-dh80-64x129x63-plain",
                                  "f32-t32-dh160-65x33x33-p0", "bf16-dh40-65x77x16-std4", "bf16-dh16-130x154x4-plain"])
def test_reference_equals_the_torch_arithmetic_of_ip_cross_attention_in_fp64(name):
    _, case, ref = _row(R.by_name(name))
    B, H, N, Nkv, Nip, dh = (case[k] for k in ("B", "H", "N", "Nkv", "Nip", "dh"))
    q = case["q"].double() / (case["scale"] * R.LOG2E) if case["prescaled"] else case["q"]
    want = torch_ip_ref(q, case["k"], case["v"], case["k_ip"], case["v_ip"], B, H, N, Nkv, Nip, dh, case["scale"], case["ip_scale"])
    assert float((ref["o"] - want).abs().max()) < 1e-12
    assert bool((ref["mag_o"] >= ref["o"].abs() - 1e-12).all()) and bool((ref["score_o"] >= 0).all())
    if Nkv == 1 and Nip == 1:                                        # both softmaxes are 1
        want1 = case["v"].double().repeat_interleave(N, 0) + case["ip_scale"] * case["v_ip"].double().repeat_interleave(N, 0)
        assert float((ref["o"] - want1).abs().max()) < 1e-15


@pytest.mark.parametrize("row", R.CASES, ids=[r["name"] for r in R.CASES])
def test_rounding_model_passes_the_gate(row):
    _, case, ref = _row(row)
    res = R.check(R.ip_model(case, row["dtype"]), ref, row["dtype"])
    assert R.passes(res) and res["err_over_bound"] <= 1.0, res


def test_measured_constants_are_the_written_ones():
    worst = {R.BF: 0.0, R.F32: 0.0}
    for row in R.CASES:
        worst[row["dtype"]] = max(worst[row["dtype"]], _row(row)[0])
    for dt in (R.BF, R.F32):
        assert abs(worst[dt] - R.MEASURED[dt]) < 5e-4, (dt, worst[dt], R.MEASURED[dt])          # to the printed digits
        assert R.C_O[dt] == R.MARGIN * R.MEASURED[dt] and R.MARGIN == 3.0
    named = R.measure_constants([R.by_name("bf16-dh40-65x77x16-std4"), R.by_name("f32-dh40-65x77x16-std4")])
    assert abs(named[R.BF][0] - R.MEASURED[R.BF]) < 5e-4 and abs(named[R.F32][0] - R.MEASURED[R.F32]) < 5e-4   # the worst rows named there


# The rows each planted defect must fail on.  ip_scale: -pre 65x77x4 0.6, -plain 65x77x4 0; 70x77x16 -plain 0.6, -pre 1.0, f32 0;
# f32 65x77x4 1.0; dh80 64x129x63 -plain 1.0, f32 0.6; dh40 64x64x64 -plain 0.6; dh40 130x154x4 -plain 1.0.
_BOTH = ["bf16-dh40-65x77x4-pre", "bf16-dh40-70x77x16-plain", "f32-dh40-65x77x4", "f32-dh80-64x129x63"]
_NAMED = {
    "joint": _BOTH + ["bf16-dh40-65x77x4-plain", "f32-dh40-70x77x16"],            # ... at ip_scale 0 too: the text part is rescaled
    "nip_minus": _BOTH + ["bf16-dh80-64x129x63-plain"],
    "nip_plus": _BOTH + ["bf16-dh80-64x129x63-plain"],
    "scale_both": ["bf16-dh40-65x77x4-pre", "bf16-dh40-70x77x16-plain", "bf16-dh40-65x77x4-plain", "f32-dh80-64x129x63", "f32-dh40-70x77x16"],
    "scale_dropped": ["bf16-dh40-65x77x4-pre", "bf16-dh40-70x77x16-plain", "bf16-dh40-65x77x4-plain", "f32-dh80-64x129x63", "f32-dh40-70x77x16"],
    "wrong_buffer": _BOTH + ["bf16-dh40-64x64x64-plain", "bf16-dh40-130x154x4-plain"],   # one, two and three text tiles
    "sample_stride": _BOTH,
    "double_c": ["bf16-dh40-65x77x4-pre", "bf16-dh40-70x77x16-pre"],
}


@pytest.mark.parametrize("defect,name", [(d, n) for d in R.DEFECTS for n in _NAMED[d]])
def test_gate_rejects_a_planted_defect(defect, name):
    row = R.by_name(name)
    _, case, ref = _row(row)
    res = R.check(R.ip_model(case, row["dtype"], defect), ref, row["dtype"])
    assert res["violations"] > 0 and res["err_over_bound"] > 2.0 and not R.passes(res), res


def _visible(defect, row):
    """Where the CONTRACT lets a defect show: an image-side defect needs ip_scale != 0 and more than one image-prompt key (over one
    key the softmax is 1 whatever the score, and a repeated key changes nothing); a misplaced ip_scale needs ip_scale != 1; the
    sample stride b Nkv lands on sample b's own rows when Nkv = Nip (mod B Nip) (two samples: 64x64x64, 32x32x32, 33x33x33)."""
    image_side = row["ip_scale"] != 0.0 and row["Nip"] >= 2
    if defect == "joint":
        return True
    if defect in ("scale_both", "scale_dropped"):
        return row["ip_scale"] != 1.0
    if defect == "sample_stride":
        return image_side and row["Nkv"] % (row["B"] * row["Nip"]) != row["Nip"]
    return image_side


def test_a_defect_escapes_only_where_the_contract_hides_it():
    """Every planted defect on every two-sample row it applies to: violations exactly where _visible says it can show."""
    wrong = []
    for row in R.CASES:
        if row["B"] != 2:
            continue
        _, case, ref = _row(row)
        for d in R.DEFECTS:
            if (d == "nip_minus" and row["Nip"] < 2) or (d == "nip_plus" and row["Nip"] == 64) or (d == "double_c" and not row["prescaled"]):
                continue
            caught = R.check(R.ip_model(case, row["dtype"], d), ref, row["dtype"])["violations"] > 0
            if caught != _visible(d, row):
                wrong.append((row["name"], d, caught))
    assert not wrong, wrong


def test_gate_counts_a_nan_and_one_element_out_of_bound():
    row = R.by_name("bf16-dh40-65x77x4-pre")
    _, case, ref = _row(row)
    got = R.ip_model(case, R.BF).clone()
    got[3, 5] = float("nan")
    got[7, 9] = ref["o"][7, 9] + 40 * R.U[R.BF] * ref["mag_o"][7, 9]
    res = R.check(got, ref, R.BF)
    assert res["violations"] == 2 and res["first"]["row"] == 3 and res["first"]["col"] == 5
