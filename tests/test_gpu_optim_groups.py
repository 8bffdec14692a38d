"""Parameter groups and the device learning-rate schedule on an MI355X: cl_adamw_dev_groups / cl_lr_schedule through the C ABI, the
optimizer step on the tiny fine-tune model (eager and replayed), resume, and the script end to end.

Kernel: p, m, v of cl_adamw_dev_groups are held BIT FOR BIT to the existing cl_adamw_dev / cl_adamw_dev_clip launched once per
contiguous run of chunks with that group's row of the table as its 6-float `hyper`, from the same starting state -- the same
expression, so the same bits; tests/test_gpu_ew_conformance.py already ties those kernels to fp64.

Optimizer: two runs from one seed do not end on the same bits on this engine (profiles/ema/run_to_run_bits.json), so only what ONE
run determines is asserted bit for bit (the learning rates the device used; a step from a saved state and a saved gradient); across
runs the parameters are held to the same-trajectory gate of tests/test_gpu_trainer_graph.py, rel-L2 < 1e-4.
"""
import ctypes
import math
import os
import sys

import pytest
import torch

from tests import ew_ref as R
from tests import optim_groups_ref as G
from tests.util import ROOT

pytestmark = pytest.mark.gpu

GUARD = 1e30
SIZES = [64, 128, 192, 320, 64 * 257, (1 << 20) + 64]
GROUPS = [1, 2, 4, 8]
MAPS = ["one", "alternating", "every_chunk", "one_group_empty", "last_chunk_alone"]
STEPS = [1, 2, 1000]
COEFS = [None, 1.0, 0.37]
EW_ADAMW_DEV_GROUPS, EW_LR_SCHEDULE = 42, 43          # csrc/elementwise.h: appended after EW_SWAP (41)


def _hip():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ctrlora_amd import hip
    hip.lib()
    return hip


def _probe(hip):
    out = (ctypes.c_int * 8)()
    assert hip.lib().cl_debug_ew_last_launch(out) == 0
    return dict(zip(R.PROBE_FIELDS, list(out)))


@pytest.fixture(autouse=True)
def _workdir(tmp_path, monkeypatch):
    _hip()
    monkeypatch.chdir(tmp_path)          # configure_optimizers writes ./tmp, the trainer ./run


@pytest.fixture
def collect_after():
    """As tests/test_gpu_ema.py: a step object and its graphs go between tests, not inside another test's capture."""
    import gc
    yield
    torch.cuda.synchronize()
    gc.collect()


def _rows(ngroups):
    """Rows that differ in every one of lr / betas / eps / weight decay (grad_scale is common to all groups)."""
    return [G.row(1e-3 * (1 + 0.7 * k), 0.9 - 0.05 * k, 0.999 - 0.01 * k, 1e-8 * 10 ** k if k < 4 else 3e-6 * k, 1e-2 * k, 1.0 / 128)
            for k in range(ngroups)]


def _map(kind, chunks, ngroups):
    c = torch.arange(chunks)
    if kind == "one" or ngroups == 1:
        return torch.zeros(chunks, dtype=torch.uint8)
    if kind == "alternating":
        return (c % 2).to(torch.uint8) * (ngroups - 1)
    if kind == "every_chunk":
        return (c % ngroups).to(torch.uint8)
    if kind == "one_group_empty":                       # runs of three chunks over every group but one
        ids = torch.tensor([k for k in range(ngroups) if k != ngroups // 2])
        return ids[(c // 3) % len(ids)].to(torch.uint8)
    if kind == "last_chunk_alone":
        m = (c % max(1, ngroups - 1)).to(torch.uint8)
        m[-1] = ngroups - 1
        return m
    raise AssertionError(kind)


class _Floats:
    """n floats between 64 guard floats of 1e30 (`tail` of them after)."""

    def __init__(self, values, tail=64):
        n = values.numel()
        self.buf = torch.full((64 + n + tail,), GUARD, device="cuda")
        self.view = self.buf[64:64 + n]
        self.view.copy_(values.reshape(-1))
        self.n = n

    def ptr(self, off=0):
        return self.view.data_ptr() + 4 * off

    def intact(self):
        return bool((self.buf[:64] == GUARD).all()) and bool((self.buf[64 + self.n:] == GUARD).all())


class _Bytes:
    def __init__(self, values):
        n = values.numel()
        self.buf = torch.full((64 + n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        self.view = self.buf[64:64 + n]
        self.view.copy_(values)
        self.n, self.want = n, values.clone()

    def intact(self):
        return bool((self.buf[:64] == 0xA5).all()) and bool((self.buf[64 + self.n:] == 0xA5).all()) and torch.equal(self.view.cpu(), self.want)


def _state(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g), torch.randn(n, generator=g) * 64, torch.randn(n, generator=g) * 0.1,
            torch.rand(n, generator=g) * 0.01)             # p, g, m, v (v >= 0)


def _launch_pair(hip, state, cg, rows, step, coef):
    """(what cl_adamw_dev_groups left, what the one-group kernel left run by run, the probe record, the guarded buffers)."""
    L, st = hip.lib(), hip.stream()
    p0, g0, m0, v0 = state
    n, ng = p0.numel(), len(rows)
    # 2048 guard floats behind the table: even row 255 of a map entry nobody clamped would stay inside this allocation
    tab = _Floats(G.table(rows), tail=2048)
    stepd = torch.tensor([step], dtype=torch.int32, device="cuda")
    clip = None if coef is None else torch.tensor([3.25, coef], dtype=torch.float32, device="cuda")
    want = [_Floats(x) for x in (p0, g0, m0, v0)]
    for lo, hi, k in G.runs(cg, ng):
        args = (want[0].ptr(lo), want[1].ptr(lo), want[2].ptr(lo), want[3].ptr(lo), hi - lo, tab.ptr(6 * k), stepd.data_ptr())
        rc = L.cl_adamw_dev(*args, st) if clip is None else L.cl_adamw_dev_clip(*args, clip.data_ptr(), st)
        assert rc == 0
    got = [_Floats(x) for x in (p0, g0, m0, v0)]
    cgd = _Bytes(cg)
    rc = L.cl_adamw_dev_groups(got[0].ptr(), got[1].ptr(), got[2].ptr(), got[3].ptr(), n, tab.ptr(), ng, cgd.view.data_ptr(),
                               stepd.data_ptr(), None if clip is None else clip.data_ptr(), st)
    assert rc == 0
    rec = _probe(hip)
    torch.cuda.synchronize()
    assert int(stepd) == step and (clip is None or clip.tolist() == [3.25, float(torch.tensor(coef, dtype=torch.float32))])
    return got, want, rec, (tab, cgd)


def _assert_case(hip, what, state, cg, rows, step, coef):
    got, want, rec, (tab, cgd) = _launch_pair(hip, state, cg, rows, step, coef)
    n = state[0].numel()
    assert rec == dict(id=EW_ADAMW_DEV_GROUPS, dtype=-1, gx=R.ew_grid(n), gy=1, gz=1, threads=256, form=0 if coef is None else 1,
                       aux=len(rows)), (what, rec)
    for name, a, b in zip("pgmv", got, want):
        diff = int((R.bits(a.view) != R.bits(b.view)).sum())
        assert diff == 0, f"{what}: {name} differs from the one-group kernel in {diff} of {n} elements"
        assert a.intact() and b.intact(), f"{what}: a guard around {name} was written"
    assert R.same_bits(got[1].view.cpu(), state[1]), f"{what}: g was written"
    assert tab.intact() and cgd.intact(), f"{what}: the table or the map was written"
    assert not R.same_bits(got[0].view.cpu(), state[0]), f"{what}: nothing moved"
    return got


@pytest.mark.parametrize("n", SIZES)
def test_grouped_launch_has_the_bits_of_the_one_group_kernel_run_by_run(n):
    hip = _hip()
    chunks = n // 64
    state = _state(n, seed=n % 9973)
    seen = set()
    for i, (ng, kind) in enumerate((a, b) for a in GROUPS for b in MAPS):
        step, coef = STEPS[i % 3], COEFS[(i // 3) % 3]
        seen.add((step, coef))
        _assert_case(hip, f"n={n} G={ng} map={kind} step={step} coef={coef}", state, _map(kind, chunks, ng), _rows(ng), step, coef)
    assert len(seen) == 9
    # every step with every clip form, on the map that changes group at every chunk (the largest size: at every third, to keep
    # the number of one-group launches of the oracle down)
    kind = "every_chunk" if chunks <= 1024 else "one_group_empty"
    for step in STEPS:
        outs = {}
        for coef in COEFS:
            got = _assert_case(hip, f"n={n} G=4 {kind} step={step} coef={coef}", state, _map(kind, chunks, 4), _rows(4), step, coef)
            outs[coef] = [x.view.cpu().clone() for x in got]
        assert all(R.same_bits(a, b) for a, b in zip(outs[None], outs[1.0])), "a coefficient of 1.0 gives the bits of no clipping"
        assert not R.same_bits(outs[None][0], outs[0.37][0])
    # rows that differ really give different results: a map of group 0 only is not the grouped result
    if chunks > 1:
        a = _launch_pair(hip, state, _map("every_chunk", chunks, 4), _rows(4), 2, None)[0]
        b = _launch_pair(hip, state, _map("one", chunks, 4), _rows(4), 2, None)[0]
        assert R.same_bits(a[0].view[:64].cpu(), b[0].view[:64].cpu()) and not R.same_bits(a[0].view[64:128].cpu(), b[0].view[64:128].cpu())


def test_grouped_launch_against_the_fp64_restatement_and_twice_from_one_state():
    hip = _hip()
    n, ng = 64 * 257, 4
    state = _state(n, seed=5)
    cg, rows = _map("one_group_empty", n // 64, ng), _rows(ng)
    for step, coef in ((1, None), (2, 0.37), (1000, 1.0)):
        got, _, _, _ = _launch_pair(hip, state, cg, rows, step, coef)
        again, _, _, _ = _launch_pair(hip, state, cg, rows, step, coef)
        assert all(R.same_bits(a.view, b.view) for a, b in zip(got, again)), "two launches from one state"
        sp = G.eval_grouped_step((state[0], state[2], state[3]), state[1], step, rows, cg, coef=coef)
        res = R.check(sp, dict(p=got[0].view.cpu(), m=got[2].view.cpu(), v=got[3].view.cpu()))
        assert not R.failures(res), (step, coef, R.failures(res))


def test_nan_and_inf_land_where_planted_and_nowhere_else():
    hip = _hip()
    n, ng = 320, 4
    p, g, m, v = _state(n, seed=3)
    g[5], g[64 + 7], p[130], m[200], v[319] = float("nan"), float("inf"), float("-inf"), float("nan"), float("inf")
    planted = {"p": {5, 71, 130, 200}, "m": {5, 71, 200}, "v": {5, 71, 319}}      # a non-finite g reaches p, m and v of its element
    got = _assert_case(hip, "planted", (p, g, m, v), _map("every_chunk", n // 64, ng), _rows(ng), 2, None)
    for name, buf in (("p", got[0]), ("m", got[2]), ("v", got[3])):
        bad = set(torch.nonzero(~torch.isfinite(buf.view.cpu())).flatten().tolist())
        assert bad == planted[name], (name, sorted(bad))


def test_out_of_range_map_entries_are_clamped_to_the_last_group():
    hip = _hip()
    n, ng = 320, 3
    state = _state(n, seed=8)
    cg = torch.tensor([0, 3, 255, 1, 8], dtype=torch.uint8)
    got = _assert_case(hip, "clamped", state, cg, _rows(ng), 2, 0.37)          # the oracle runs chunks 1, 2 and 4 on row ng - 1
    clean = _launch_pair(hip, state, torch.tensor([0, 2, 2, 1, 2], dtype=torch.uint8), _rows(ng), 2, 0.37)[0]
    assert all(R.same_bits(a.view, b.view) for a, b in zip(got, clean))
    assert all(bool(torch.isfinite(x.view).all()) for x in got), "nothing of the 1e30 behind the table was read"


@pytest.mark.parametrize("ngroups", [1, 4])
@pytest.mark.parametrize("T", [1, 2, 5])
def test_lr_schedule_rows_and_the_rest_of_the_table(T, ngroups):
    hip = _hip()
    L, st = hip.lib(), hip.stream()
    gen = torch.Generator().manual_seed(T * 10 + ngroups)
    lr_table = torch.rand(T, ngroups, generator=gen) * 1e-3
    table0 = torch.rand(ngroups, 6, generator=gen) + 2.0
    for counter in (1, 2, T, T + 1, 10 ** 6, 0, -5):
        tab, lrs = _Floats(table0), _Floats(lr_table)
        stepd = torch.tensor([counter], dtype=torch.int32, device="cuda")
        assert L.cl_lr_schedule(tab.ptr(), ngroups, lrs.ptr(), T, stepd.data_ptr(), st) == 0
        assert _probe(hip) == dict(id=EW_LR_SCHEDULE, dtype=-1, gx=1, gy=1, gz=1, threads=64, form=0, aux=ngroups)
        torch.cuda.synchronize()
        got = tab.view.cpu().reshape(ngroups, 6)
        row = G.lr_row(counter, T)
        assert row == min(max(counter - 1, 0), T - 1)
        assert R.same_bits(got[:, 0].contiguous(), lr_table[row].contiguous()), (T, ngroups, counter)
        assert R.same_bits(got[:, 1:].contiguous(), table0[:, 1:].contiguous()), "columns 1..5 are not the schedule's"
        assert tab.intact() and lrs.intact() and R.same_bits(lrs.view.cpu(), lr_table.reshape(-1)) and int(stepd) == counter


# ------------------------------------------------------------------------------------------------ the optimizer step, tiny model

LORA_PLUS = {"name": "lora_up", "match": ["lora_layer.up."], "lr_scale": 4.0}
NO_DECAY = {"name": "no_decay", "match": ["norm", ".bias"], "weight_decay": 0.0}
SCHED = {"target": "ctrlora_amd.lr_schedule.WarmupDecay", "params": dict(kind="cosine", warmup_steps=2, total_steps=6, min_ratio=0.1)}
LR = 1e-3


def _model(groups=None, sched=False, ema=False):
    import bench

    def mutate(p):
        if groups is not None:
            p.update(optim_groups=list(groups))
        if sched:
            p.update(scheduler_config=SCHED)
        if ema:
            p.update(use_ema=True, ema_decay=0.9)
    m = bench.build_model("ctrlora_finetune_sd15_rank128.yaml", 0, tiny=True, mutate=mutate)
    m.learning_rate = LR
    m.get_input = lambda batch, k, *a, **kw: (batch["z"], {"c_crossattn": [batch["ctx"]], "c_concat": [batch["hint_z"]]})
    return m


def _want_table(steps, scales=(1.0, 4.0, 1.0)):
    """The compiled curve, from the closed form: fl32(base_lr_k * lambda(n))."""
    from ctrlora_amd.lr_schedule import WarmupDecay
    lam = WarmupDecay(**SCHED["params"]).schedule
    return torch.tensor([[LR * s * lam(n) for s in scales] for n in range(steps)], dtype=torch.float64).to(torch.float32)


def _on_gpu(m):
    m = m.cuda().train()
    m.set_engine_dtype(torch.float32)
    return m


def _fill_state(opt, seed=21):
    """A saved state and a saved gradient: random masters' gradient and moments (v >= 0), the counter at 3."""
    (ex,), (st,) = opt.executors, opt._states
    g = torch.Generator().manual_seed(seed)
    n = ex.tr.numel
    ex.tr.flat_grad.copy_(torch.randn(n, generator=g) * 0.05)
    st.m.copy_(torch.randn(n, generator=g) * 0.01)
    st.v.copy_(torch.rand(n, generator=g) * 1e-4)
    opt._step_dev.fill_(3)
    torch.cuda.synchronize()
    return [x.clone() for x in (ex.tr.flat, ex.tr.flat_grad, st.m, st.v)]


def test_grouped_step_from_one_state_and_one_gradient():
    """From one saved state and one gradient: the grouped step is, tensor by tensor, the one-group kernel with that tensor's group's
    row (bit for bit) and the fp64 restatement (at the conformance gate); and with a lora_up ratio of 4 only the lora_layer.up
    tensors move differently from the one-group step -- every other tensor keeps its bits."""
    hip = _hip()
    m = _on_gpu(_model(groups=[LORA_PLUS, NO_DECAY]))
    opt = m.configure_optimizers()
    assert opt.group_names == ["default", "lora_up", "no_decay"] and opt._chunk_group is not None
    (ex,), (st,) = opt.executors, opt._states
    p0, g0, m0, v0 = _fill_state(opt)
    opt.step()
    torch.cuda.synchronize()
    assert int(opt._step) == 4
    got = [x.clone() for x in (ex.tr.flat, st.m, st.v)]
    assert R.same_bits(ex.tr.flat_grad, g0)
    # (a) the one-group kernel per tensor, with the row of the tensor's group
    group_of = {id(p): k for k, grp in enumerate(opt.param_groups) for p in grp["params"]}
    bound = dict(zip([t.name for t in ex.tr.items], m.control_model.__dict__["_bound"]))
    want = [x.clone() for x in (p0, m0, v0)]
    stepd = torch.tensor([4], dtype=torch.int32, device="cuda")
    rows = {}
    for t in ex.tr.items:
        k = group_of[id(bound[t.name])]
        rows.setdefault(k, []).append(t.name)
        lo, nn = t.offset, (t.master.numel() + 63) // 64 * 64
        hip.adamw_dev(want[0][lo:lo + nn], g0[lo:lo + nn], want[1][lo:lo + nn], want[2][lo:lo + nn], opt._hyper_table[k], stepd)
    torch.cuda.synchronize()
    assert all(R.same_bits(a, b) for a, b in zip(got, want)), "the grouped step is not the one-group kernel per tensor"
    assert all("lora_layer.up." in n for n in rows[1]) and len(rows[1]) == 82 and all("norm" in n or ".bias" in n for n in rows[2])
    # (b) the host restatement, at the gate the one-group kernel is held to
    table = [dict(zip(G.KEYS, r)) for r in opt._hyper_table.cpu().tolist()]
    assert [round(r["lr"] / LR) for r in table] == [1, 4, 1] and [r["wd"] for r in table] == [table[0]["wd"], table[0]["wd"], 0.0]
    sp = G.eval_grouped_step((p0.cpu(), m0.cpu(), v0.cpu()), g0.cpu(), 4, table, opt._chunk_group[0].cpu())
    res = R.check(sp, dict(p=got[0].cpu(), m=got[1].cpu(), v=got[2].cpu()))
    assert not R.failures(res), R.failures(res)
    # (c) LoRA+ alone against one group, from the same state and gradient: only the up matrices move differently
    del opt, m
    plus = _on_gpu(_model(groups=[LORA_PLUS]))
    one = _on_gpu(_model())
    outs = []
    for mod in (plus, one):
        o = mod.configure_optimizers()
        (e,), (s,) = o.executors, o._states
        e.tr.flat.copy_(p0); e.tr.flat_grad.copy_(g0); s.m.copy_(m0); s.v.copy_(v0)
        o._step_dev.fill_(3)
        o.step()
        torch.cuda.synchronize()
        outs.append((o, e.tr.flat.clone(), s.m.clone(), s.v.clone()))
    (o_plus, p_plus, m_plus, v_plus), (o_one, p_one, m_one, v_one) = outs
    assert o_one._chunk_group is None and o_plus.group_names == ["default", "lora_up"]
    assert R.same_bits(m_plus, m_one) and R.same_bits(v_plus, v_one), "the moments do not depend on the learning rate"
    moved = same = 0
    for t in o_one.executors[0].tr.items:
        sl = slice(t.offset, t.offset + t.master.numel())
        if "lora_layer.up." in t.name:
            assert not R.same_bits(p_plus[sl], p_one[sl]), f"{t.name}: the ratio of 4 changed nothing (it does nothing on the parent commit)"
            step_plus, step_one = (p_plus[sl] - p0[sl]).double(), (p_one[sl] - p0[sl]).double()
            # lr enters the decay and the update linearly and 4 lr is exact in fp32, so the step is 4 x the one-group step up to
            # rounding: each p' carries half an ulp of p and each update (a product, two quotients) under three ulps of itself;
            # 1 + 4 of the former and 3 + 4 x 3 / 4 of the latter stay under 16 units of 2^-24 (|p| + |step|)
            assert float((step_plus - 4 * step_one).abs().max()) <= 16 * float(p0[sl].abs().max() + step_plus.abs().max()) * 2.0 ** -24
            moved += 1
        else:
            assert R.same_bits(p_plus[sl], p_one[sl]), f"{t.name} is in the default group and must keep the one-group step's bits"
            same += 1
    assert moved == 82 and same == 82 + 56 + 26


class _LrRecorder:
    """Trainer callback: after every optimizer step the device's lr column (a clone, no host wait) and the flat masters."""

    def __init__(self, start=0):
        self.lrs, self.flat, self.seen = [], None, start

    def on_batch_end(self, trainer, model):
        if trainer.global_step > self.seen:
            self.seen = trainer.global_step
            self.lrs.append(trainer.optimizer.last_lr().clone())
            self.flat = trainer.optimizer.executors[0].tr.flat


_RUNS = {}


def _fit(graph_step, steps=6, acc=1, clip=None, ema=False, ckpt_path=None, start=0, rng_state=None, callbacks=()):
    from ctrlora_amd.trainer import Trainer
    from tests.test_gpu_trainer_graph import SEED, _batches
    key = (repr(graph_step), steps, acc, clip, ema)
    if key in _RUNS and ckpt_path is None and not callbacks:
        return _RUNS[key]
    rec = _LrRecorder(start)
    tr = Trainer(max_steps=steps, accumulate_grad_batches=acc, precision=32, default_root_dir="run", log_every_n_steps=1,
                 graph_step=graph_step, gradient_clip_val=clip, callbacks=[rec, *callbacks])
    m = _model(groups=[LORA_PLUS, NO_DECAY], sched=True, ema=ema)
    torch.manual_seed(SEED)
    if rng_state is not None:
        torch.cuda.set_rng_state(rng_state)
    tr.fit(m, _batches(6 * acc)[start * acc:], ckpt_path=ckpt_path)
    torch.cuda.synchronize()
    out = (tr, rec, rec.flat.cpu().clone())
    if ckpt_path is None and not callbacks:
        _RUNS[key] = out
    return out


def _assert_lrs(what, tr, rec, first_step, last_step):
    """After optimizer step s the device's lr column is row s - 1 of the compiled table, bit for bit, and the fp32 of the host
    mirror `param_groups[k]["lr"]` that step was logged with."""
    table = _want_table(tr.max_steps)
    assert tr._lr_on_device and R.same_bits(tr.optimizer._lr_table.cpu(), table), f"{what}: the table on the device"
    assert len(rec.lrs) == last_step - first_step + 1, (what, len(rec.lrs))
    for s, lr in zip(range(first_step, last_step + 1), rec.lrs):
        assert R.same_bits(lr.cpu().contiguous(), table[s - 1].contiguous()), f"{what}: step {s} ran on {lr.tolist()}, row {s - 1} is {table[s - 1].tolist()}"
    assert [s for s, _ in tr.logged_lr] == list(range(first_step, last_step + 1))
    for s, logs in tr.logged_lr:
        assert list(logs) == ["train/lr/default", "train/lr/lora_up", "train/lr/no_decay"]
        mirror = torch.tensor(list(logs.values()), dtype=torch.float64).to(torch.float32)
        assert R.same_bits(mirror, table[s - 1].contiguous()), f"{what}: the host mirror at step {s}"
    assert int(tr.optimizer._step) == last_step == tr.global_step and tr.lr_scheduler.last_epoch == last_step


def _close(what, got, want):
    from tests.test_gpu_trainer_graph import GATE
    from tests.util import rel_l2
    r = rel_l2(got, want)
    print(f"[optim groups] {what}: rel-L2 {r:.3e} (gate {GATE:.1e})")
    assert r < GATE, (what, r)


def test_eager_trainer_follows_the_table():
    tr, rec, flat = _fit(False)
    assert tr.graph_mode == "off" and tr.optimizer.group_names == ["default", "lora_up", "no_decay"]
    _assert_lrs("eager", tr, rec, 1, 6)
    table = _want_table(6)
    # half the rate, the rate twice (the end of the warm-up, q = 0), then three steps down the cosine
    assert len({float(x) for x in table[:, 0]}) == 5 and float(table[1, 0]) == float(table[2, 0]) == float(torch.tensor(LR)) == 2 * float(table[0, 0])
    assert "train/lr/lora_up" in tr.model.last_logged


@pytest.mark.parametrize("form", ["one", "gradacc2", "clip+ema"])
def test_replayed_trainer_follows_the_table(form, collect_after):
    acc = 2 if form == "gradacc2" else 1
    clip, ema = (1e-3, True) if form == "clip+ema" else (None, False)
    steps = 4 if acc == 2 else 6
    tr, rec, flat = _fit(True, steps=steps, acc=acc, clip=clip, ema=ema)
    assert tr.graph_mode == "one" and tr.graph_replays > 0 and tr.graph_replays == steps - tr.graph_eager_steps
    _assert_lrs(f"replayed ({form})", tr, rec, 1, steps)
    assert tr.optimizer._captured
    if clip:
        assert float(tr.optimizer.last_grad_norm()[1]) < 1.0 and int(tr.model.model_ema.num_updates) == steps
    tr_e, rec_e, flat_e = _fit(False, steps=steps, acc=acc, clip=clip, ema=ema)
    _assert_lrs(f"eager ({form})", tr_e, rec_e, 1, steps)
    _close(f"{form}: parameters, scheduled replayed against scheduled eager", flat, flat_e)
    if form == "one":
        # the schedule and the groups act: a run without them ends somewhere else
        from tests.test_gpu_trainer_graph import _eager_ref
        from tests.util import rel_l2
        plain = _eager_ref(32, 1)[1]
        names = [t.name for t in tr.optimizer.executors[0].tr.items if "lora_layer.up." in t.name][:4]
        got = dict(tr.model.control_model.named_parameters())
        assert all(rel_l2(got[n].detach().float().cpu(), plain[n]) > 1e-3 for n in names)


def test_graphed_train_step_follows_the_table_and_takes_new_values_after_capture(collect_after):
    from ctrlora_amd.lr_schedule import compile_lambda_lr
    from ctrlora_amd.train import GraphedTrainStep
    from tests.test_gpu_ema import _step_batches
    table = _want_table(6)
    results = []
    for graphed in (False, True):
        m = _on_gpu(_model(groups=[LORA_PLUS, NO_DECAY], sched=True))
        (opt,), (entry,) = m.configure_optimizers()
        sched = entry["scheduler"]
        assert entry["interval"] == "step" and entry["frequency"] == 1 and type(sched).__name__ == "LambdaLR"
        opt.set_lr_schedule(compile_lambda_lr(sched, 6))
        assert R.same_bits(opt._lr_table.cpu(), table)
        batches = _step_batches(6)
        gs = GraphedTrainStep(m, opt, *batches[0], warmup=0, capture=False)
        for k, batch in enumerate(batches):
            if graphed and k == 2:
                gs.capture()
            mirror = torch.tensor([g["lr"] for g in opt.param_groups], dtype=torch.float64).to(torch.float32)
            (gs if gs.captured else gs.eager)(*batch)
            sched.step()
            assert R.same_bits(opt.last_lr().cpu().contiguous(), table[k].contiguous()), (graphed, k)
            assert R.same_bits(mirror, table[k].contiguous()), "the host mirror of the step"
        torch.cuda.synchronize()
        results.append(opt.executors[0].tr.flat.cpu().clone())
        if graphed:
            assert opt._captured
            # a same-shape copy is followed by the next replay ...
            opt._step_dev.fill_(1)
            opt.set_lr_schedule(table * 0.5)
            gs(*batches[0])
            assert R.same_bits(opt.last_lr().cpu().contiguous(), (table * 0.5)[1].contiguous()), "the replay read the new values"
            # ... switching off or to another shape is refused, and so is switching on after a capture
            for bad in (None, table[:3]):
                with pytest.raises(RuntimeError, match="after a capture"):
                    opt.set_lr_schedule(bad)
        del gs
    _close("GraphedTrainStep: parameters, scheduled replayed against scheduled eager", results[1], results[0])
    m = _on_gpu(_model(groups=[LORA_PLUS]))
    opt = m.configure_optimizers()
    batches = _step_batches(2)
    gs = GraphedTrainStep(m, opt, *batches[0], warmup=1, capture=True)
    with pytest.raises(RuntimeError, match="after a capture.*does not launch cl_lr_schedule"):
        opt.set_lr_schedule(torch.ones(4, 2))
    gs(*batches[1])
    torch.cuda.synchronize()
    del gs


def test_resume_at_step_three_is_back_on_the_curve(tmp_path):
    class _Rng:
        state = None

        def on_batch_end(self, trainer, model):
            if trainer.global_step == 3 and self.state is None:
                self.state = torch.cuda.get_rng_state()
    rng = _Rng()
    a, rec_a, _ = _fit(True, steps=3, callbacks=[rng])
    # the first leg's table has max_steps = 3 rows, a prefix of the curve: WarmupDecay's total_steps is the config's, not the leg's
    assert R.same_bits(a.optimizer._lr_table.cpu(), _want_table(3)) and len(rec_a.lrs) == 3
    ck = str(tmp_path / "three.ckpt")
    a.save_checkpoint(ck)
    saved = torch.load(ck, map_location="cpu", weights_only=False)
    assert saved["lr_schedulers"][0]["last_epoch"] == 3 and saved["optimizer_states"][0]["step"] == 3
    assert [g["name"] for g in saved["optimizer_states"][0]["param_groups"]] == ["default", "lora_up", "no_decay"]
    table = _want_table(6)
    assert [float(torch.tensor(g["lr"], dtype=torch.float32)) for g in saved["optimizer_states"][0]["param_groups"]] == table[3].tolist(), \
        "the mirror in the checkpoint is the next step's rate"
    del a
    for graph_step in (True, False):
        b, rec_b, flat_b = _fit(graph_step, steps=6, ckpt_path=ck, start=3, rng_state=rng.state)
        _assert_lrs(f"resumed (graph_step={graph_step})", b, rec_b, 4, 6)
        _, _, flat_whole = _fit(graph_step)
        _close(f"resumed against uninterrupted (graph_step={graph_step})", flat_b, flat_whole)
    # a checkpoint of other groups is refused before anything is copied
    from ctrlora_amd.trainer import Trainer
    m = _model(groups=[LORA_PLUS], sched=True)
    with pytest.raises(ValueError, match=r"\['default', 'lora_up', 'no_decay'\].*\['default', 'lora_up'\]"):
        Trainer(max_steps=6, precision=32, default_root_dir="run").fit(m, [], ckpt_path=ck)


def test_a_host_scheduler_on_the_engine_optimizer_is_refused_under_graph_step():
    from ctrlora_amd.trainer import Trainer
    from tests.test_gpu_trainer_graph import SEED, _batches
    m = _model(groups=[LORA_PLUS])
    conf = m.configure_optimizers
    m.configure_optimizers = lambda: (lambda o: ([o], [torch.optim.lr_scheduler.StepLR(o, 2, 0.5)]))(conf())
    with pytest.raises(ValueError, match="graph_step refused: a StepLR moves the learning rate on the host"):
        Trainer(max_steps=2, precision=32, default_root_dir="run", graph_step=True).fit(m, _batches(2))
    assert not torch.cuda.is_current_stream_capturing()
    # without graph_step it takes the host path: scheduler.step() + sync_hyper()
    torch.manual_seed(SEED)
    rec = _LrRecorder()
    tr = Trainer(max_steps=4, precision=32, default_root_dir="run", log_every_n_steps=1, callbacks=[rec])
    m2 = _model(groups=[LORA_PLUS])
    conf2 = m2.configure_optimizers
    m2.configure_optimizers = lambda: (lambda o: ([o], [torch.optim.lr_scheduler.StepLR(o, 2, 0.5)]))(conf2())
    tr.fit(m2, _batches(4))
    torch.cuda.synchronize()
    f = lambda x: float(torch.tensor(x, dtype=torch.float32))
    assert not tr._lr_on_device and tr.optimizer._lr_table is None
    assert [lr.tolist() for lr in rec.lrs] == [[f(LR * s), f(4 * LR * s)] for s in (1.0, 0.5, 0.5, 0.25)], "pushed after scheduler.step()"


# ------------------------------------------------------------------------------------------------ the script, end to end

def test_finetune_script_with_schedule_and_groups_under_graph(tmp_path_factory, monkeypatch, collect_after):
    """scripts/train_ctrlora_finetune.py --graph --lr_schedule cosine --lr_warmup_steps 2 --lora_plus_ratio 4 --no_decay_norm_bias for
    four steps: train/lr/<group> in the log, the compiled rates on the device, the group names in last.ckpt."""
    from tests.test_gpu_trainer_graph import _load
    import ctrlora_amd.trainer as trainer_mod
    out = str(tmp_path_factory.mktemp("synth_optim_groups"))
    mod = _load(os.path.join(ROOT, "tests", "tools", "make_synthetic_assets.py"), "make_synthetic_assets")
    argv, sys.argv = sys.argv, ["make_synthetic_assets.py", "--out", out, "--n", "4"]
    try:
        mod.main()
    finally:
        sys.argv = argv
    monkeypatch.setenv("CTRLORA_SYNTHETIC_TOKENIZER", "1")
    real = trainer_mod.Trainer
    monkeypatch.setattr(trainer_mod, "Trainer", lambda **kw: real(**{**kw, "log_every_n_steps": 1}))      # the script logs every 50 steps
    train = _load(os.path.join(ROOT, "scripts", "train_ctrlora_finetune.py"), "train_ctrlora_finetune")
    tr = train.main(["--dataroot", os.path.join(out, "custom"), "--config", os.path.join(out, "finetune_narrow.yaml"),
                     "--sd_ckpt", os.path.join(out, "sd_synth.ckpt"), "--cn_ckpt", os.path.join(out, "basecn_synth.ckpt"), "--graph", "--bs", "2",
                     "--max_steps", "4", "--precision", "16", "--num_workers", "0", "--img_logger_freq", "1000", "--ckpt_logger_freq", "1000",
                     "--lr", "1e-4", "-n", "groups", "--lr_schedule", "cosine", "--lr_warmup_steps", "2", "--lora_plus_ratio", "4",
                     "--no_decay_norm_bias"])
    torch.cuda.synchronize()
    assert tr.global_step == 4 and int(tr.optimizer._step) == 4 and tr.graph_mode == "one" and tr.graph_replays > 0
    assert tr.optimizer.group_names == ["default", "lora_up", "no_decay"] and tr._lr_on_device
    from ctrlora_amd.lr_schedule import WarmupDecay
    lam = WarmupDecay("cosine", 2, 4, 0.0).schedule
    want = torch.tensor([[1e-4 * s * lam(n) for s in (1.0, 4.0, 1.0)] for n in range(4)], dtype=torch.float64).to(torch.float32)
    assert R.same_bits(tr.optimizer._lr_table.cpu(), want) and R.same_bits(tr.optimizer.last_lr().cpu().contiguous(), want[3].contiguous())
    assert [s for s, _ in tr.logged_lr] == [1, 2, 3, 4]
    for s, logs in tr.logged_lr:
        assert list(logs) == ["train/lr/default", "train/lr/lora_up", "train/lr/no_decay"]
        assert torch.tensor(list(logs.values()), dtype=torch.float64).to(torch.float32).tolist() == want[s - 1].tolist()
    assert {"train/lr/default", "train/lr/lora_up", "train/lr/no_decay", "train/loss"} <= set(tr.model.last_logged)
    assert tr.optimizer._hyper_table[:, 4].tolist() == [float(torch.tensor(1e-2)), float(torch.tensor(1e-2)), 0.0]
    last = os.path.join(tr.checkpoint_callback.dirpath, tr.checkpoint_callback.filename)
    tr.save_checkpoint(last)
    saved = torch.load(last, map_location="cpu", weights_only=False)
    assert os.path.basename(last) == "last.ckpt" and saved["global_step"] == 4 and saved["lr_schedulers"][0]["last_epoch"] == 4
    assert [g["name"] for g in saved["optimizer_states"][0]["param_groups"]] == ["default", "lora_up", "no_decay"]
    up = [v for k, v in tr.model.state_dict().items() if k.endswith("lora_layer.up.weight")]
    assert up and all(torch.isfinite(v).all() for v in up) and any(float(v.abs().sum()) > 0 for v in up)
