"""The gates of tests/grad_clip_ref.py bite: each mistake a gradient-norm / clip kernel could make is flagged by at least one row of
the case table, and the unmutated fp64 model by none.  CPU only; the GPU suite applies the same gates to the kernels
(tests/test_gpu_grad_clip.py)."""
import functools

import numpy as np
import pytest

from tests import grad_clip_ref as G


@functools.lru_cache(maxsize=None)
def _views(name):
    return [v for _, v in G.make_bufs(G.ROW[name])]


def _norm_rows_flagged(mutant):
    bad = []
    for row in G.CASES:
        n32, c32 = G.model(row, _views(row["name"]), mutant)
        if G.judge(row, _views(row["name"]), n32, c32):
            bad.append(row["name"])
    return bad


def _adamw_rows_flagged(mutant):
    bad = []
    for n in G.ADAMW_N:
        ops = G.adamw_ops(n)
        state = (ops["p"], ops["m"], ops["v"])
        for scale, coef in ((1.0 / 128, 1.0), (1.0 / 128, 0.37), (1.0, 0.37)):
            got = G.adamw_model(state, ops["g"], 2, scale, coef, mutant)
            if G.adamw_flags(got, G.adamw_specs(state, ops["g"], 2, scale, coef)):
                bad.append((n, scale, coef))
    return bad


def test_the_model_itself_passes_every_row():
    assert _norm_rows_flagged(None) == []
    assert _adamw_rows_flagged(None) == []


def test_the_table_covers_what_it_claims():
    rows = G.CASES
    assert {len(r["counts"]) for r in rows} >= {1, 3, 16}
    assert {n for r in rows for n in r["counts"]} >= set(G.COUNTS)
    assert {r["scale"] for r in rows} == {1.0, 1.0 / 8}
    assert {r["shift"] for r in rows} == {0, 1, 2, 3}
    assert any(r["span"] for r in rows) and {r["plant"][0] for r in rows if r["plant"]} == {"nan", "inf"}
    assert any(r["max_norm"] is None for r in rows) and any(r["max_norm"] == 0.0 for r in rows)
    # clipping acts in some rows and not in others
    coefs = [float(G.model(r, _views(r["name"]))[1]) for r in rows if r["max_norm"] and not r["plant"]]
    assert any(c < 1.0 for c in coefs) and any(c == 1.0 for c in coefs)
    # a view one float past a 16-byte boundary is what it says
    back, view = G.make_bufs(G.ROW["shift1"])[0]
    assert back.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4
    assert all(G.guards_intact(b, v) for r in rows[:8] for b, v in G.make_bufs(r))


def test_the_span_row_needs_fp64_squares():
    """1e-25 .. 1e+25 in one buffer: the true norm is finite in fp32, a sum of fp32 squares is not."""
    v = _views("span-1e25")[0]
    n32, _ = G.model(G.ROW["span-1e25"], [v])
    assert np.isfinite(n32) and 1e24 < float(n32) < 3e38
    assert not bool((v * v).sum().isfinite()) and int(((v * v) == 0).sum()) > 0


def test_nan_and_inf_rows():
    n32, c32 = G.model(G.ROW["nan"], _views("nan"))
    assert n32 != n32 and c32 != c32
    n32, c32 = G.model(G.ROW["inf"], _views("inf"))
    assert np.isinf(n32) and float(c32) == 0.0


@pytest.mark.parametrize("mutant", ["drop_last_buffer", "drop_tail", "no_grad_scale", "fminf"])
def test_norm_mutants_are_flagged(mutant):
    bad = _norm_rows_flagged(mutant)
    assert bad, f"no row of the table notices '{mutant}'"
    if mutant == "fminf":
        assert bad == ["nan"]
    if mutant == "no_grad_scale":
        assert set(bad) == {r["name"] for r in G.CASES if r["scale"] != 1.0 and any(r["counts"])}


def test_coef_on_m_only_is_flagged():
    bad = _adamw_rows_flagged("coef_on_m_only")
    assert bad and all(coef != 1.0 for _, _, coef in bad)
    assert {(n, s) for n, s, c in bad} == {(n, s) for n in G.ADAMW_N for s in (1.0 / 128, 1.0)}


def test_mutant_list_is_the_one_checked_here():
    assert set(G.MUTANTS) == {"drop_last_buffer", "drop_tail", "no_grad_scale", "fminf", "coef_on_m_only"}
