"""CPU checks of tests/block_ref.py: the fp64 block reference against the oracle, the reproducibility of the same-storage
comparator's error (the floor the GPU gate is a multiple of), that the gate separates a wrong block from a rounded one, and
that the pure-Python launch-form predicates evaluate as each case declares."""
import functools

import pytest
import torch

from oracle import ref_model as R
from tests import block_ref as BR

SEEDS = (1, 2, 3)
GATE = 2.0        # the bf16 gate of tests/test_gpu_block_conformance.py: engine error <= GATE x comparator error


def _forms():
    """Distinct (case, storage mode, form) of the bf16 runs: what the comparator is evaluated as."""
    seen = {}
    for r in BR.RUNS:
        if r.dtype == "bf16":
            seen.setdefault((r.case, r.mode, r.case == "rb-frozen", r.ip, r.backward, r.variant == "deslot"), r)
    return list(seen.values())


@functools.lru_cache(maxsize=None)
def _floor(run_id, seed):
    """{output: rel-L2(comparator, fp64)} of one run's form at one seed."""
    run = BR.RUN_BY_ID[run_id]
    case = BR.CASES[run.case]
    e_pre, ips = run.case == "rb-frozen", (0.6 if run.ip else None)
    ref = BR.reference(run.case, seed, e_pre, ips, run.backward)
    sd = BR.make_sd(case, seed, ips)
    cmp_ = BR.evaluate(case, sd, BR.make_inputs(case, seed), run.mode, e_pre=e_pre, ip=run.ip, backward=run.backward)
    return {k: BR.rel(cmp_[k], ref[k]) for k in BR.gated(run, sd)}


# ------------------------------------------------------------------------------------------- reference against the oracle

@pytest.mark.parametrize("name", ["rb-ft-skip", "rb-pre", "st-ft-ragged"])
def test_reference_matches_the_fp32_oracle(name):
    """block_ref's fp64 functions against oracle/ref_model.py's (fp32, pinned to the unmodified reference by
    test_oracle_golden.py) on the same state: rel-L2 < 1e-5 on the output and every gradient."""
    case = BR.CASES[name]
    sd, inp = BR.make_sd(case, 1), BR.make_inputs(case, 1)
    g = torch.Generator().manual_seed(7)
    emb = torch.randn(case.B, BR.CFG.time_embed_dim, generator=g)

    def run(dt, res_fn, st_fn):
        s = {k: v.to(dt).requires_grad_(True) for k, v in sd.items()}
        x = inp["x"].to(dt).requires_grad_(True)
        out = res_fn(s, BR.P, x, emb.to(dt)) if case.kind == "res" else st_fn(s, BR.P, x, inp["c"].to(dt), BR.HEADS)
        names = list(s)
        grads = torch.autograd.grad((out * inp["dout"].to(dt)).sum(), [x] + [s[k] for k in names])
        return dict(zip(["out", "dx"] + names, (out.detach(),) + grads))

    got = run(torch.float64, BR.resblock, BR.spatial_transformer)
    want = run(torch.float32, R.resblock, R.spatial_transformer)
    worst = max((BR.rel(want[k], got[k]), k) for k in want)
    assert worst[0] < 1e-5, worst


def test_ip_branch_is_the_documented_contract():
    """ip_scale = 0 leaves the plain cross-attention; a non-zero scale adds exactly ip_scale * softmax(ip) V_ip."""
    case = BR.CASES["st-ip"]
    inp = BR.make_inputs(case, 1)
    outs = {}
    for s in (0.0, 0.6, 1.2):
        sd = {k: v.double() for k, v in BR.make_sd(case, 1, s).items()}
        outs[s] = BR.spatial_transformer(sd, BR.P, inp["x"].double(), inp["c"].double(), BR.HEADS, ip=inp["c_ip"].double())
    plain = BR.spatial_transformer({k: v.double() for k, v in BR.make_sd(case, 1).items()}, BR.P, inp["x"].double(),
                                   inp["c"].double(), BR.HEADS)
    assert torch.equal(outs[0.0], plain)
    assert BR.rel(outs[0.6], plain) > 1e-3


# ------------------------------------------------------------------------------------------- the floor is reproducible

@pytest.mark.parametrize("run", _forms(), ids=lambda r: r.id)
def test_comparator_floor_is_stable_across_seeds(run):
    """For every gated output the comparator's error over seeds 1, 2, 3 has max / min <= 1.5: the floor a run is gated
    against is a property of the case, not of the draw."""
    floors = [_floor(run.id, s) for s in SEEDS]
    bad = {}
    for k in floors[0]:
        v = [f[k] for f in floors]
        if max(v) == 0.0:
            # the storage model rounds nothing on the way to this output (the bias gradient of the block's last layer is a
            # column sum of the bf16 upstream gradient): no floor to scale -- the GPU test gates it as an fp32 accumulation
            assert k.endswith(".bias"), k
            continue
        assert min(v) > 0, (k, v)
        if max(v) / min(v) > 1.5:
            bad[k] = v
    assert not bad, bad


# ------------------------------------------------------------------------------------------- the gate catches a wrong block

_DEFECT_RUNS = [("st-ft-r64-bf16", d) for d in ("scale", "lora", "residual", "accum", "geglu_swap")] + \
               [("rb-ft-bf16", d) for d in ("lora", "residual", "accum", "rowbias")]


@pytest.mark.parametrize("run_id,defect", _DEFECT_RUNS)
def test_gate_catches_defect(run_id, defect):
    """Each defect, applied to the comparator, puts at least one gated output beyond GATE x the comparator's own error.
    Measured (seed 1; the worst output's error / its floor, and how many of the gated outputs exceed the gate):
      st-ft-r64   attention scale x 1.02                    4.1x   15 of 30
                  LoRA term of attn1.to_v dropped           160x   25 of 30
                  attn1's residual dropped                  483x   30 of 30
                  accum ignored in norm2's backward         210x   13 of 30
                  GEGLU halves swapped in backward only     200x   27 of 30
      rb-ft       LoRA term of emb_layers dropped           215x    5 of 5
                  the block's residual dropped              511x    2 of 5
                  accum (dskip) ignored in GroupNorm bwd    511x    1 of 5
                  emb row-bias dropped                      215x    5 of 5"""
    import dataclasses
    run = BR.RUN_BY_ID[run_id]
    case = BR.CASES[run.case]
    floor = _floor(run_id, 1)
    sd = BR.make_sd(case, 1)
    bad = BR.evaluate(case, sd, BR.make_inputs(case, 1), dataclasses.replace(run.mode, defect=defect))
    ref = BR.reference(run.case, 1, False, None, True)
    # (a tensor the defective block never touches has no gradient at all: the engine would leave its slice zero)
    ratios = {k: BR.rel(bad.get(k, torch.zeros_like(ref[k])), ref[k]) / floor[k] for k in floor}
    beyond = [k for k, v in ratios.items() if v > GATE]
    print(f"{run_id} {defect}: worst {max(ratios.values()):.1f}x, {len(beyond)} of {len(ratios)} beyond the gate")
    assert beyond, ratios


# ------------------------------------------------------------------------------------------- case predicates

@pytest.mark.parametrize("run", BR.RUNS, ids=lambda r: r.id)
def test_pure_predicates_evaluate_as_declared(run, monkeypatch):
    from ctrlora_amd import hip
    if run.variant == "ln-off":
        monkeypatch.setattr(hip, "LN_PROLOGUE", False)
    got = BR.pure_predicates(run)
    want = dict(run.expect)
    both = sorted(set(got) & set(want))
    assert both or not want
    assert {k: got[k] for k in both} == {k: want[k] for k in both}


def test_run_table_covers_every_case():
    assert {r.case for r in BR.RUNS} == set(BR.CASES)
    assert len(BR.RUN_BY_ID) == len(BR.RUNS)
