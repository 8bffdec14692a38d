"""The grouped-step restatement (tests/optim_groups_ref.py) against torch.optim.AdamW with real parameter groups and a real
LambdaLR over the same tensors, at the gate the one-group restatement is held to (tests/test_ew_reference_model.py: rel-L2 1e-7 for
p and m, 1e-6 for v) -- and proof that the restatement bites: three plausible mistakes each miss that gate by orders of magnitude."""
import math

import pytest
import torch

from tests import optim_groups_ref as G

SIZES = (64, 100, 128, 5, 192, 64, 70)
GROUPS = (0, 1, 2, 1, 0, 2, 1)
ROWS = [G.row(1e-3, 0.9, 0.999, 1e-8, 1e-2, 1 / 128), G.row(4e-3, 0.8, 0.99, 1e-6, 0.0, 1 / 128),
        G.row(2.5e-4, 0.95, 0.9, 1e-7, 0.1, 1 / 128)]
LAMBDAS = [lambda n: (n + 1) / 3 if n < 3 else 0.5 * (1 + math.cos(math.pi * min(1.0, (n - 3) / 4))),
           lambda n: 1.0 / (1 + n), lambda n: 0.9 ** n]
STEPS, T = 6, 5          # the table ends one row before the run does: the last row holds
GATE = dict(p=1e-7, m=1e-7, v=1e-6)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _problem():
    gen = torch.Generator().manual_seed(11)
    offs, total = G.layout(SIZES)
    p0 = torch.zeros(total)
    grads = [torch.zeros(total) for _ in range(STEPS)]
    for s, o in zip(SIZES, offs):
        p0[o:o + s] = torch.randn(s, generator=gen)
        for g in grads:
            g[o:o + s] = torch.randn(s, generator=gen) * 64
    return offs, total, p0, grads


def _starts():
    """The state as stored (fp32) before every step: the restatement's own trajectory, carried in fp32 as the device carries it."""
    offs, total, p0, grads = _problem()
    cg = G.chunk_map(SIZES, GROUPS)
    state, out = (p0.clone(), torch.zeros(total), torch.zeros(total)), []
    for step in range(1, STEPS + 1):
        out.append(state)
        sp = G.eval_grouped_step(state, grads[step - 1], step, ROWS, cg, lr_table=_lr_table())
        state = tuple(sp[k]["model"] for k in ("p", "m", "v"))
    return out


def _lr_table():
    return torch.tensor([[G.f32(r["lr"]) * lam(n) for r, lam in zip(ROWS, LAMBDAS)] for n in range(STEPS)], dtype=torch.float64).float()


def _torch_run():
    """torch.optim.AdamW in fp64 on the hyper-parameters as stored (fp32), groups as real param_groups, a real LambdaLR stepped
    once per optimizer step; every step starts from the stored fp32 state (as tests/test_ew_reference_model.py holds the one-group
    restatement: a step's arithmetic, not six steps of carried rounding).  Returns per step the flat (p, m, v) and the lr every
    group used."""
    offs, total, p0, grads = _problem()
    starts = _starts()
    f = G.f32
    params = [torch.nn.Parameter(p0[o:o + s].double().clone()) for s, o in zip(SIZES, offs)]
    groups = [dict(params=[p for p, k in zip(params, GROUPS) if k == gi], lr=f(r["lr"]), betas=(f(r["beta1"]), f(r["beta2"])), eps=f(r["eps"]),
                   weight_decay=f(r["wd"])) for gi, r in enumerate(ROWS)]
    opt = torch.optim.AdamW(groups)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=LAMBDAS)
    out, lrs = [], []
    for step in range(STEPS):
        lrs.append([g["lr"] for g in opt.param_groups])
        for p, s, o in zip(params, SIZES, offs):
            p.grad = grads[step][o:o + s].double() * f(ROWS[0]["gscale"])
            p.data.copy_(starts[step][0][o:o + s])
            if step:
                opt.state[p]["exp_avg"].copy_(starts[step][1][o:o + s])
                opt.state[p]["exp_avg_sq"].copy_(starts[step][2][o:o + s])
        opt.step()
        sched.step()
        flat = {k: torch.zeros(total, dtype=torch.float64) for k in "pmv"}
        for p, s, o in zip(params, SIZES, offs):
            flat["p"][o:o + s] = p.detach()
            flat["m"][o:o + s] = opt.state[p]["exp_avg"]
            flat["v"][o:o + s] = opt.state[p]["exp_avg_sq"]
        out.append(flat)
    return out, lrs


def _restated(rows=ROWS, shift=0, row_of=None, table_rows=T):
    """The restatement's trajectory from the same start; the knobs plant the mistakes."""
    offs, total, p0, grads = _problem()
    cg = G.chunk_map(SIZES, GROUPS)
    if shift:
        cg = torch.roll(cg, shift)
    lr_table, starts = _lr_table(), _starts()
    out = []
    for step in range(1, STEPS + 1):
        s_for_lr = step if row_of is None else row_of(step)
        rws = G.scheduled_rows(rows, lr_table[:table_rows], s_for_lr)
        sp = G.eval_grouped_step(starts[step - 1], grads[step - 1], step, rws, cg)
        out.append({k: sp[k]["ref"] for k in ("p", "m", "v")})
    return out, lr_table


@pytest.fixture(scope="module")
def want():
    return _torch_run()


def _worst(got, want_steps, steps):
    return {k: max(_rel(got[s][k], want_steps[s][k]) for s in range(steps)) for k in ("p", "m", "v")}


def test_restatement_is_torch_adamw_with_param_groups_and_lambda_lr(want):
    steps, lrs = want
    got, lr_table = _restated(table_rows=STEPS)
    # the compiled curve is the fp32 of what the host scheduler put into param_groups, entry for entry
    for s in range(STEPS):
        assert [float(torch.tensor(x, dtype=torch.float32)) for x in lrs[s]] == lr_table[s].tolist()
    w = _worst(got, steps, STEPS)
    print("[optim groups ref] worst rel-L2 against torch.optim.AdamW over", STEPS, "steps:", w)
    assert all(w[k] < GATE[k] for k in w), w
    # the padding between the tensors stays zero
    offs, total, _, _ = _problem()
    pad = torch.ones(total, dtype=torch.bool)
    for s, o in zip(SIZES, offs):
        pad[o:o + s] = False
    assert pad.any() and all(float(got[-1][k][pad].abs().max()) == 0.0 for k in ("p", "m", "v"))


def test_past_the_end_the_last_row_holds(want):
    steps, _ = want
    assert [G.lr_row(s, T) for s in (0, 1, 2, T, T + 1, 10 ** 6)] == [0, 0, 1, T - 1, T - 1, T - 1]
    got, _ = _restated(table_rows=T)
    assert all(v < GATE[k] for k, v in _worst(got, steps, T).items()), "within the table nothing changes"
    held, _ = _restated(table_rows=STEPS, row_of=lambda s: min(s, T))
    assert all(torch.equal(got[STEPS - 1][k], held[STEPS - 1][k]) for k in ("p", "m", "v")), "step T + 1 runs on row T - 1"
    assert _rel(got[STEPS - 1]["p"], steps[STEPS - 1]["p"]) > 100 * GATE["p"], "torch's curve moved on, the table did not"


@pytest.mark.parametrize("mistake", ["rows_swapped", "map_shifted", "row_s_not_s_minus_1"])
def test_the_restatement_bites(want, mistake):
    steps, _ = want
    if mistake == "rows_swapped":
        got, _ = _restated(rows=[ROWS[1], ROWS[0], ROWS[2]], table_rows=STEPS)
    elif mistake == "map_shifted":
        got, _ = _restated(shift=1, table_rows=STEPS)
    else:
        got, _ = _restated(table_rows=STEPS, row_of=lambda s: s + 1)
    w = _worst(got, steps, STEPS)
    print(f"[optim groups ref] {mistake}: worst rel-L2 {w}")
    assert w["p"] > 100 * GATE["p"], (mistake, w)
