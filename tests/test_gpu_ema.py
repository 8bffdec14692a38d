"""EMA of the fine-tuned weights on an MI355X: cl_ema_update / cl_swap, the optimizer step (eager and replayed), resume,
ema_scope, log_images and the scripts.

Kernels: bit-equal to tests/ema_ref.py (which tests/test_ema_reference_model.py ties to the reference's LitEma) over the sizes,
the 4 x 4 pointer offsets from a 16-byte boundary, the counters and the decays below; guards of 1e30 around both buffers; p
untouched; two launches the same bits; NaN / inf land where they were planted; the launch record; refusals launch nothing.

Optimizer step, on the tiny fine-tune model of tests/test_gpu_trainer_graph.py in fp32.  Two runs of this model from one seed
do not end on the same bits, with or without the EMA: the weight-gradient sums are accumulated in arrival order, and two eager
runs of the parent's own loop, EMA off, differed in all 246 trained tensors after six steps (largest difference 4e-7, the last
loss in its last bit; eager against replayed and replayed against replayed the same: profiles/ema/run_to_run_bits.json).  A bit comparison ACROSS runs can therefore
not tell the EMA from the engine, and what is asserted bit for bit here is what one run determines: the optimizer step from one
state and one gradient with the EMA attached and detached (it does not touch training); the shadows against the host restatement
of the run's own recorded parameter trajectory (eager, GraphedTrainStep, Trainer(graph_step=...), gradient accumulation, clipping,
after a resume from the restored bits, after an ema_scope); num_updates == optimizer steps; the bits a checkpoint restores; the
masters, shadows and eps before and after an ema_scope, and eps inside it against a model loaded from the extracted --ema file.
Across runs (EMA on / off, replayed / eager, resumed / uninterrupted, with / without a scope) parameters and shadows are held to
the same-trajectory gate of tests/test_gpu_trainer_graph.py, rel-L2 < 1e-4."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import ema_ref as E
from tests import ew_ref as R
from tests.util import ROOT

pytestmark = pytest.mark.gpu

GUARD = 1e30
SIZES = [0, 1, 3, 4, 5, 63, 64, 65, 257, 4099, (1 << 20) + 5]
COUNTERS = [-1, 1, 9, 10, 89989, 89990, 89991]
DECAYS = [0.0, 0.9, 0.9999, 1.0]
OFFSETS = [(a, b) for a in range(4) for b in range(4)]
EMA_DECAY = 0.9


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


def _ew_id(name):
    from tests.test_gpu_ddim_edit import _ew_id as f
    return f(name)


@pytest.fixture(autouse=True)
def _workdir(tmp_path, monkeypatch):
    _hip()
    monkeypatch.chdir(tmp_path)          # configure_optimizers writes ./tmp, the trainer ./run


@pytest.fixture
def collect_after():
    """A GraphedTrainStep is reachable from its own reduce_fn closure, so it and its captured graphs go only when the cycle
    collector runs: collect here, between tests, and not whenever it fires next -- possibly inside another test's capture."""
    import gc
    yield
    torch.cuda.synchronize()
    gc.collect()


class _Guarded:
    """n floats starting `off` floats past a 16-byte boundary, 64 guard floats of 1e30 on either side."""

    def __init__(self, values: torch.Tensor, off: int):
        n = values.numel()
        self.buf = torch.full((n + 136,), GUARD, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.lo = 64 + off
        self.view = self.buf[self.lo:self.lo + n]
        self.view.copy_(values)
        assert n == 0 or self.view.data_ptr() % 16 == 4 * off

    def intact(self):
        n = self.view.numel()
        return bool((self.buf[:self.lo] == GUARD).all()) and bool((self.buf[self.lo + n:] == GUARD).all())


def _values(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g), torch.randn(n, generator=g)


def _want_record(name, n, off_a, off_b):
    if off_a == off_b:
        head = min((4 - off_a) % 4, n)
        nvec = (n - head) // 4
        return dict(id=_ew_id(name), dtype=-1, gx=R.ew_grid(nvec), gy=1, gz=1, threads=256, form=1, aux=nvec)
    return dict(id=_ew_id(name), dtype=-1, gx=R.ew_grid(n), gy=1, gz=1, threads=256, form=0, aux=0)


def _scalars(decay, u):
    return torch.tensor(decay, dtype=torch.float32).cuda(), torch.tensor(u, dtype=torch.int32).cuda()


# ------------------------------------------------------------------------------------------------ cl_ema_update

@pytest.mark.parametrize("n", SIZES)
def test_ema_update_sizes_and_offsets(n):
    """Every size at all 16 offset pairs (decay 0.9999, u = 9: the warm-up term rules): the reference's bits, guards, p untouched,
    two launches from one state the same bits, the launch record."""
    hip = _hip()
    s0, p0 = _values(n, 100 + n % 97)
    want = torch.from_numpy(E.update(s0.numpy(), p0.numpy(), 0.9999, 9)) if n else s0
    d, u = _scalars(0.9999, 9)
    for off_s, off_p in OFFSETS:
        results = []
        for _ in range(2):
            s, p = _Guarded(s0, off_s), _Guarded(p0, off_p)
            hip.ema_update(s.view, p.view, d, u)
            torch.cuda.synchronize()
            rec = _probe(hip)
            assert rec == (_want_record("EW_EMA_UPDATE", n, off_s, off_p) if n else dict.fromkeys(R.PROBE_FIELDS, 0)), (rec, off_s, off_p)
            assert s.intact() and p.intact() and E.same_bits(p.view, p0), (n, off_s, off_p)
            results.append(s.view.cpu())
        assert E.same_bits(results[0], want), (n, off_s, off_p, int((E.bits(results[0]) != E.bits(want)).sum()))
        assert E.same_bits(results[0], results[1])
    assert int(u) == 9 and float(d) == float(np.float32(0.9999))


@pytest.mark.parametrize("u", COUNTERS)
@pytest.mark.parametrize("decay", DECAYS)
def test_ema_update_counters_and_decays(u, decay):
    """Both forms (offsets equal / different) at a size with a head, vectors that wrap the grid-stride loop once, and a tail."""
    hip = _hip()
    n = 4099
    s0, p0 = _values(n, 7)
    want = torch.from_numpy(E.update(s0.numpy(), p0.numpy(), decay, u))
    d, cnt = _scalars(decay, u)
    for off_s, off_p in ((0, 0), (3, 3), (1, 2)):
        s, p = _Guarded(s0, off_s), _Guarded(p0, off_p)
        hip.ema_update(s.view, p.view, d, cnt)
        torch.cuda.synchronize()
        assert s.intact() and p.intact() and E.same_bits(p.view, p0)
        assert E.same_bits(s.view, want), (u, decay, off_s, off_p)
    if decay == 1.0 and u < 0:
        assert E.same_bits(want, s0), "decay 1 without the warm-up keeps the shadow"
    if decay == 0.0:
        assert torch.allclose(want, p0, atol=1e-6), "decay 0 follows the parameter"


def test_ema_update_large_wraps_the_grid():
    """2^20 + 5 elements from different offsets: the scalar form's grid-stride loop iterates (1 M threads at most)."""
    hip = _hip()
    n = (1 << 20) + 5
    assert R.wraps(n)
    s0, p0 = _values(n, 3)
    s, p = _Guarded(s0, 2), _Guarded(p0, 1)
    d, u = _scalars(0.9, -1)
    hip.ema_update(s.view, p.view, d, u)
    torch.cuda.synchronize()
    assert s.intact() and p.intact()
    assert E.same_bits(s.view, torch.from_numpy(E.update(s0.numpy(), p0.numpy(), 0.9, -1)))


@pytest.mark.parametrize("offs", [(0, 0), (1, 3)], ids=["vector", "scalar"])
def test_ema_update_nan_and_inf_land_where_planted(offs):
    hip = _hip()
    n = 257
    s0, p0 = _values(n, 21)
    p0[0], p0[5], p0[130], p0[256] = float("nan"), float("inf"), float("-inf"), float("nan")
    s, p = _Guarded(s0, offs[0]), _Guarded(p0, offs[1])
    d, u = _scalars(0.9, 50)
    hip.ema_update(s.view, p.view, d, u)
    torch.cuda.synchronize()
    got = s.view.cpu()
    assert torch.isnan(got).nonzero().flatten().tolist() == [0, 256]
    assert torch.isinf(got).nonzero().flatten().tolist() == [5, 130] and got[5] > 0 and got[130] < 0
    want = torch.from_numpy(E.update(s0.numpy(), p0.numpy(), 0.9, 50))
    finite = torch.isfinite(want)
    assert E.same_bits(got[finite], want[finite]) and s.intact() and p.intact()


def test_ema_update_padding_stays_zero():
    hip = _hip()
    s = torch.zeros(192, device="cuda")
    p = torch.zeros(192, device="cuda")
    s[:50], p[:50] = 1.5, -2.0
    d, u = _scalars(0.9999, 3)
    hip.ema_update(s, p, d, u)
    torch.cuda.synchronize()
    assert E.bits(s[50:]).tolist() == [0] * 142 and E.bits(p[50:]).tolist() == [0] * 142


def test_ema_update_refusals_leave_the_shadow_untouched():
    hip = _hip()
    L, st = hip.lib(), hip.stream()
    s0, p0 = _values(64, 1)
    s, p = _Guarded(s0, 0), _Guarded(p0, 0)
    d, u = _scalars(0.9, 1)
    sp, pp, dp, up = s.view.data_ptr(), p.view.data_ptr(), d.data_ptr(), u.data_ptr()
    calls = {
        "null shadow": L.cl_ema_update(None, pp, 64, dp, up, st), "null p": L.cl_ema_update(sp, None, 64, dp, up, st),
        "null decay": L.cl_ema_update(sp, pp, 64, None, up, st), "null num_updates": L.cl_ema_update(sp, pp, 64, dp, None, st),
        "null decay, n = 0": L.cl_ema_update(sp, pp, 0, None, up, st), "n < 0": L.cl_ema_update(sp, pp, -1, dp, up, st),
        "misaligned": L.cl_ema_update(sp + 2, pp, 8, dp, up, st), "overlap": L.cl_ema_update(sp, sp + 16, 32, dp, up, st),
    }
    torch.cuda.synchronize()
    assert {k: v for k, v in calls.items() if v != 1} == {}
    assert _probe(hip)["id"] == 0
    assert E.same_bits(s.view, s0) and E.same_bits(p.view, p0) and s.intact() and p.intact()
    assert L.cl_ema_update(None, None, 0, dp, up, st) == 0 and _probe(hip)["id"] == 0        # n == 0: fine, nothing launched


# ------------------------------------------------------------------------------------------------ cl_swap

@pytest.mark.parametrize("n", SIZES)
def test_swap_sizes_and_offsets(n):
    hip = _hip()
    a0, b0 = _values(n, 300 + n % 89)
    for off_a, off_b in OFFSETS:
        a, b = _Guarded(a0, off_a), _Guarded(b0, off_b)
        hip.swap_(a.view, b.view)
        torch.cuda.synchronize()
        rec = _probe(hip)
        assert rec == (_want_record("EW_SWAP", n, off_a, off_b) if n else dict.fromkeys(R.PROBE_FIELDS, 0)), (rec, off_a, off_b)
        assert E.same_bits(a.view, b0) and E.same_bits(b.view, a0) and a.intact() and b.intact(), (n, off_a, off_b)
        hip.swap_(a.view, b.view)
        torch.cuda.synchronize()
        assert E.same_bits(a.view, a0) and E.same_bits(b.view, b0) and a.intact() and b.intact(), "twice is the identity"


def test_swap_with_itself_and_refusals():
    hip = _hip()
    L, st = hip.lib(), hip.stream()
    a0, b0 = _values(64, 2)
    a0[3] = float("nan")
    a, b = _Guarded(a0, 1), _Guarded(b0, 0)
    ap, bp = a.view.data_ptr(), b.view.data_ptr()
    assert L.cl_swap(ap, ap, 64, st) == 0 and _probe(hip)["id"] == 0, "a == b: fine, nothing to do"
    calls = {"overlap": L.cl_swap(ap, ap + 16, 32, st), "n < 0": L.cl_swap(ap, bp, -1, st), "null a": L.cl_swap(None, bp, 4, st),
             "null b": L.cl_swap(ap, None, 4, st), "misaligned": L.cl_swap(ap + 1, bp, 4, st)}
    torch.cuda.synchronize()
    assert {k: v for k, v in calls.items() if v != 1} == {}
    assert _probe(hip)["id"] == 0 and E.same_bits(a.view, a0) and E.same_bits(b.view, b0) and a.intact() and b.intact()
    assert L.cl_swap(None, None, 0, st) == 0
    hip.swap_(a.view, b.view)
    torch.cuda.synchronize()
    assert E.same_bits(a.view, b0) and E.same_bits(b.view, a0), "the bits travel, a NaN's payload included"


# ------------------------------------------------------------------------------------------------ the optimizer step

def _model(ema=True, decay=EMA_DECAY, **cn):
    import bench

    def mutate(p):
        if ema:
            p.update(use_ema=True, ema_decay=decay)
        p["control_stage_config"]["params"].update(cn)
    m = bench.build_model("ctrlora_finetune_sd15_rank128.yaml", 0, tiny=True, mutate=mutate)
    m.learning_rate = 1e-3
    m.get_input = lambda batch, k, *a, **kw: (batch["z"], {"c_crossattn": [batch["ctx"]], "c_concat": [batch["hint_z"]]})
    return m


class _Recorder:
    """Trainer callback: the flat masters after every optimizer step (a device clone, no host wait)."""

    def __init__(self):
        self.flats, self.seen = [], 0

    def on_batch_end(self, trainer, model):
        if trainer.global_step > self.seen:
            self.seen = trainer.global_step
            self.flats.append(trainer.optimizer.executors[0].tr.flat.clone())


_RUNS = {}


def _fit(ema=True, graph_step=False, steps=6, acc=1, clip=None, ckpt_path=None, start=0, rng_state=None, key=None):
    """One Trainer run from the common seed; (trainer, recorder, flat masters, flat shadows or None, num_updates or None)."""
    from ctrlora_amd.trainer import Trainer
    from tests.test_gpu_trainer_graph import SEED, _batches
    key = key or (ema, repr(graph_step), steps, acc, clip)
    if key in _RUNS and ckpt_path is None:
        return _RUNS[key]
    rec = _Recorder()
    rec.seen = start
    tr = Trainer(max_steps=steps, accumulate_grad_batches=acc, precision=32, default_root_dir="run", log_every_n_steps=1,
                 graph_step=graph_step, gradient_clip_val=clip, callbacks=[rec])
    m = _model(ema)                      # seeds the generators itself: the run's seed comes after
    torch.manual_seed(SEED)
    if rng_state is not None:
        torch.cuda.set_rng_state(rng_state)       # a resumed leg continues the uninterrupted leg's stream of t and noise
    batches = _batches(6 * acc)[start * acc:]
    tr.fit(m, batches, ckpt_path=ckpt_path)
    torch.cuda.synchronize()
    ex = tr.optimizer.executors[0]
    out = (tr, rec, ex.tr.flat.cpu().clone(), m.model_ema.flat.cpu().clone() if ema else None,
           int(m.model_ema.num_updates) if ema else None)
    if ckpt_path is None:
        _RUNS[key] = out
    return out


def _seed_flat():
    """The flat masters before the first step: what the shadows are seeded with (the model is a function of the seed)."""
    if "seed" not in _RUNS:
        m = _model(True).cuda().train()
        m.set_engine_dtype(torch.float32)
        _RUNS["seed"] = m.control_model.executor().tr.flat.cpu().clone()
    return _RUNS["seed"]


def _host_shadows(rec, u0=0, start=None):
    start = _seed_flat() if start is None else start
    return E.trajectory(start, [f.cpu() for f in rec.flats], EMA_DECAY, u0)


def _close(what, got, want, gate=None):
    """rel-L2 under the same-trajectory gate of tests/test_gpu_trainer_graph.py (1e-4 in fp32): two runs of one seed."""
    from tests.test_gpu_trainer_graph import GATE
    from tests.util import rel_l2
    r = rel_l2(got, want)
    print(f"[ema] {what}: rel-L2 {r:.3e} (gate {gate or GATE:.1e}), {int((E.bits(got) != E.bits(want)).sum())} of {got.numel()} elements differ in bits")
    assert r < (gate or GATE), (what, r)


def _tiny():
    m = _model(True).cuda().train()
    m.set_engine_dtype(torch.float32)
    return m


def _step_batches(n):
    """n micro-batches (z, ctx, hint, t, noise), the same in every leg."""
    from tests.test_gpu_trainer_graph import B, H, _batches
    g = torch.Generator().manual_seed(11)
    out = []
    for b in _batches(n, seed=9):
        t = torch.randint(0, 1000, (B,), generator=g).cuda()
        out.append((b["z"], b["ctx"], b["hint_z"], t, torch.randn(B, 4, H, H, generator=g).cuda()))
    return out


@pytest.mark.parametrize("clip", [None, 1e-3], ids=["plain", "grad_clip"])
def test_the_step_with_the_ema_is_the_step_without_it_bit_for_bit(clip):
    """Six steps; at each, from the same state and the same gradient: opt.step() with the EMA detached and attached -- the same
    masters, moments and step count, bit for bit (the feature does not touch training), and the shadows move by the restatement."""
    m = _tiny()
    opt = m.configure_optimizers()
    opt.max_grad_norm = clip
    ema, flats = opt.ema, opt._ema_flats
    assert ema is m.model_ema and flats[0] is ema.flat and E.same_bits(ema.flat, opt.executors[0].tr.flat), "seeded from the masters"
    (ex,), (st,) = opt.executors, opt._states
    live = [ex.tr.flat, st.m, st.v, opt._step_dev]
    for k, (z, ctx, hint, t, noise) in enumerate(_step_batches(6)):
        opt.zero_grad()
        loss, _ = m.p_losses(z, {"c_crossattn": [ctx], "c_concat": [hint]}, t, noise=noise)
        loss.backward()
        before = [x.clone() for x in live]
        shadow_before = ema.flat.cpu().clone()
        opt.ema, opt._ema_flats = None, None
        opt.step()
        torch.cuda.synchronize()
        off = [x.clone() for x in live]
        assert int(ema.num_updates) == k and E.same_bits(ema.flat, shadow_before), "detached: nothing of the EMA moves"
        for x, y in zip(live, before):
            x.copy_(y)
        opt.ema, opt._ema_flats = ema, flats
        opt.step()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(live, off)), f"step {k + 1}: the EMA changed the optimizer step"
        assert not torch.equal(off[0], before[0]), "the step moved nothing"
        assert int(ema.num_updates) == k + 1 == int(opt._step)
        want = E.update(shadow_before.numpy(), ex.tr.flat.cpu().numpy(), EMA_DECAY, k + 1)
        assert E.same_bits(ema.flat, want), f"step {k + 1}"
        if clip:
            assert float(opt.last_grad_norm()[1]) < 1.0, "clipping must act"


@pytest.mark.parametrize("acc,clip", [(1, None), (2, None), (1, 1e-3)], ids=["plain", "gradacc2", "grad_clip"])
def test_eager_trainer_shadows_follow_the_restatement(acc, clip):
    """The Trainer's eager loop: the shadows are the host restatement of the run's own recorded parameter trajectory, bit for bit,
    and num_updates counts optimizer steps.  EMA on against EMA off is compared under the same-trajectory gate: two runs of one
    seed do not give the same bits on this engine with or without the EMA (see the module docstring)."""
    steps = 6 if acc == 1 else 3
    tr_off, _, flat_off, _, _ = _fit(False, False, steps, acc, clip)
    tr, rec, flat, shadow, count = _fit(True, False, steps, acc, clip)
    assert tr.optimizer.ema is tr.model.model_ema and tr_off.optimizer.ema is None
    assert not hasattr(tr_off.model, "model_ema")
    _close(f"parameters, EMA on against off (acc {acc}, clip {clip})", flat, flat_off)
    assert count == steps == len(rec.flats) == int(tr.optimizer._step), "num_updates counts optimizer steps"
    assert E.same_bits(rec.flats[-1].cpu(), flat) and not E.same_bits(flat, _seed_flat()), "the run moved nothing"
    want = _host_shadows(rec)
    assert E.same_bits(shadow, want), int((E.bits(shadow) != E.bits(want)).sum())
    assert not E.same_bits(shadow, flat), "the shadows are not the weights"
    if clip:
        assert float(tr.optimizer.last_grad_norm()[1]) < 1.0, "clipping must act"
    # and the shadows a state_dict carries are views of that flat buffer, under LitEma's key rule
    sd = tr.model.state_dict()
    ex = tr.optimizer.executors[0]
    for t in ex.tr.items[:5] + ex.tr.items[-5:]:
        key = "model_ema." + ("control_model." + t.name).replace(".", "")
        want = t.param_view(tr.model.model_ema.flat[t.offset:t.offset + t.master.numel()].view(t.shape))
        assert sd[key].shape == dict(tr.model.control_model.named_parameters())[t.name].shape and torch.equal(sd[key], want)


@pytest.mark.parametrize("form", ["trainer-one", "trainer-acc2", "trainer-segmented", "trainer-one-clip", "graphed-train-step"])
def test_replayed_steps_follow_the_restatement_and_the_eager_run(form, collect_after):
    """The update inside a captured step: bit for bit the restatement of the replayed run's own trajectory (a stale address, a
    count baked into the graph or a second tick would all show), num_updates == optimizer steps, and the eager run's shadows and
    parameters under the same-trajectory gate."""
    if form == "graphed-train-step":
        from ctrlora_amd.train import GraphedTrainStep
        results = []
        for graphed in (False, True):
            m = _tiny()
            opt = m.configure_optimizers()
            ex = opt.executors[0]
            batches = _step_batches(6)
            seed = ex.tr.flat.cpu().clone()
            gs = GraphedTrainStep(m, opt, *batches[0], warmup=0, capture=False)
            flats = []
            for k, batch in enumerate(batches):
                if graphed and k == 2:
                    gs.capture()
                (gs if gs.captured else gs.eager)(*batch)
                flats.append(ex.tr.flat.clone())
            torch.cuda.synchronize()
            shadow = m.model_ema.flat.cpu().clone()
            assert int(m.model_ema.num_updates) == 6 == int(opt._step)
            assert E.same_bits(shadow, E.trajectory(seed, [f.cpu() for f in flats], EMA_DECAY)), f"graphed={graphed}"
            results.append((ex.tr.flat.cpu().clone(), shadow))
            # the step object is no reference cycle: it goes, with its graphs, when the last reference does
            import gc
            import weakref
            alive = weakref.ref(gs)
            gc.disable()
            try:
                del gs
                assert alive() is None, "GraphedTrainStep is kept alive by a reference cycle"
            finally:
                gc.enable()
        (p_e, s_e), (p_g, s_g) = results
        _close("GraphedTrainStep parameters, replayed against eager", p_g, p_e)
        _close("GraphedTrainStep shadows, replayed against eager", s_g, s_e)
        assert not E.same_bits(s_e, p_e)
        return
    acc = 2 if form == "trainer-acc2" else 1
    clip = 1e-3 if form.endswith("clip") else None
    steps = 3 if acc == 2 else 6
    graph_step = dict(split_graphs="segmented", bucket_bytes=256 << 10, reduce_fn=lambda buf: None) if form == "trainer-segmented" else True
    _, _, flat_e, shadow_e, count_e = _fit(True, False, steps, acc, clip)
    tr, rec, flat, shadow, count = _fit(True, graph_step, steps, acc, clip)
    assert tr.graph_replays > 0 and tr.graph_replays == steps - tr.graph_eager_steps
    assert tr.graph_mode == ("segmented" if form == "trainer-segmented" else "one")
    assert count == count_e == steps == int(tr.optimizer._step) == len(rec.flats)
    assert E.same_bits(shadow, _host_shadows(rec)), "the replayed update is not the restatement of its own trajectory"
    _close(f"{form}: parameters, replayed against eager", flat, flat_e)
    _close(f"{form}: shadows, replayed against eager", shadow, shadow_e)
    if clip:
        assert float(tr.optimizer.last_grad_norm()[1]) < 1.0, "clipping must act"


def test_resume_restores_the_shadows_and_continues(tmp_path):
    """3 steps, save_checkpoint, a fresh model, fit(ckpt_path=), 3 more: the resumed run starts from the saved bits (masters,
    shadows, num_updates), its shadows are the restatement continued from them with the count at 3, bit for bit, and it ends on
    the uninterrupted run's parameters and shadows under the same-trajectory gate."""
    from ctrlora_amd.trainer import Trainer
    from tests.test_gpu_trainer_graph import SEED, _batches
    _, _, flat6, shadow6, count6 = _fit(True, False, 6, 1)

    class _Rng:
        state = None

        def on_batch_end(self, trainer, model):
            if trainer.global_step == 3 and self.state is None:
                self.state = torch.cuda.get_rng_state()
    rng = _Rng()
    tr = Trainer(max_steps=3, precision=32, default_root_dir="run", log_every_n_steps=1, callbacks=[rng])
    m3 = _model(True)
    torch.manual_seed(SEED)
    tr.fit(m3, _batches(6)[:3])
    torch.cuda.synchronize()
    path = str(tmp_path / "three.ckpt")
    tr.save_checkpoint(path)
    flat3, shadow3 = tr.optimizer.executors[0].tr.flat.cpu().clone(), m3.model_ema.flat.cpu().clone()
    saved = torch.load(path, map_location="cpu", weights_only=False)["state_dict"]
    assert int(saved["model_ema.num_updates"]) == 3 and float(saved["model_ema.decay"]) == float(np.float32(EMA_DECAY))
    del tr, m3

    start = {}
    orig = Trainer._restore_optimizer

    def spy(self, ck):
        orig(self, ck)
        start.update(flat=self.optimizer.executors[0].tr.flat.cpu().clone(), shadow=self.model.model_ema.flat.cpu().clone(),
                     count=int(self.model.model_ema.num_updates), attached=self.optimizer.ema is self.model.model_ema)
    Trainer._restore_optimizer = spy
    try:
        tr2, rec, flat, shadow, count = _fit(True, False, 6, 1, ckpt_path=path, start=3, rng_state=rng.state)
    finally:
        Trainer._restore_optimizer = orig
    assert start["attached"] and start["count"] == 3
    assert E.same_bits(start["flat"], flat3) and E.same_bits(start["shadow"], shadow3), "the checkpoint's bits, not a re-seed"
    assert tr2.global_step == 6 and count == count6 == 6 and len(rec.flats) == 3
    assert E.same_bits(shadow, _host_shadows(rec, u0=3, start=shadow3)), "resumed shadows"
    _close("resumed parameters against six uninterrupted steps", flat, flat6)
    _close("resumed shadows against six uninterrupted steps", shadow, shadow6)


# ------------------------------------------------------------------------------------------------ ema_scope

def _eps(m, seed=3):
    from tests.test_gpu_trainer_graph import B, CTX_DIM, H
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g).cuda()
    x, ctx, hint = mk(B, 4, H, H), mk(B, 77, CTX_DIM), mk(B, 4, H, H)
    t = torch.tensor([17, 801][:B]).cuda()
    with torch.no_grad():
        was = m.training
        m.eval()
        out = m.apply_model(x, t, {"c_crossattn": [ctx], "c_concat": [hint]}).float().cpu().clone()
        m.train(was)
    return out


def test_ema_scope_swaps_in_place_and_a_captured_step_survives_it(tmp_path, collect_after):
    from ctrlora_amd.train import GraphedTrainStep
    from tests.test_gpu_trainer_graph import _load
    X = _load(os.path.join(ROOT, "scripts", "tool_extract_weights.py"), "tool_extract_weights")

    legs = []
    for scoped in (False, True):
        m = _tiny()
        opt = m.configure_optimizers()
        bs = _step_batches(5)
        gs = GraphedTrainStep(m, opt, *bs[0], warmup=0, capture=False)
        gs.eager(*bs[0])
        gs.eager(*bs[1])
        gs.capture()
        gs(*bs[2])
        torch.cuda.synchronize()
        ex = opt.executors[0]
        if scoped:
            flat_ptr, shadow_ptr = ex.tr.flat.data_ptr(), m.model_ema.flat.data_ptr()
            before = (ex.tr.flat.cpu().clone(), m.model_ema.flat.cpu().clone(), _eps(m))
            assert not E.same_bits(before[0], before[1])
            ckpt = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
            with m.ema_scope():
                torch.cuda.synchronize()
                assert E.same_bits(ex.tr.flat.cpu(), before[1]) and E.same_bits(m.model_ema.flat.cpu(), before[0])
                inside = _eps(m)
                with pytest.raises(RuntimeError, match="ema_scope"):
                    opt.step()
                for launch in (gs, gs.eager):          # a replay does not pass through opt.step(): refused all the same
                    with pytest.raises(RuntimeError, match="ema_scope"):
                        launch(*bs[3])
                torch.cuda.synchronize()
                assert int(m.model_ema.num_updates) == 3 == int(opt._step), "a refused step launched nothing"
            torch.cuda.synchronize()
            assert (ex.tr.flat.data_ptr(), m.model_ema.flat.data_ptr()) == (flat_ptr, shadow_ptr), "no tensor moves"
            assert E.same_bits(ex.tr.flat.cpu(), before[0]) and E.same_bits(m.model_ema.flat.cpu(), before[1])
            assert E.same_bits(_eps(m), before[2]) and not E.same_bits(inside, before[2])
            # a second model, EMA off, whose trained weights come from the extracted --ema file
            lora = X.with_ema_values(X.extract_lora(ckpt), ckpt)
            assert len(lora) == len(m.trainable_names())
            m2 = _model(False).cuda().train()
            m2.set_engine_dtype(torch.float32)
            m2.load_state_dict({k: v for k, v in ckpt.items() if not k.startswith("model_ema.")}, strict=True)
            m2.load_state_dict(lora, strict=False)
            assert E.same_bits(_eps(m2), inside), "inside the scope the engine runs the extracted EMA weights"
            del m2
        traj = []
        seed_shadow, u0 = m.model_ema.flat.cpu().clone(), int(m.model_ema.num_updates)
        for batch in bs[3:]:
            gs(*batch)
            traj.append(ex.tr.flat.clone())
        torch.cuda.synchronize()
        assert u0 == 3 and int(m.model_ema.num_updates) == 5 == int(opt._step)
        assert not E.same_bits(traj[0].cpu(), traj[1].cpu()), "the replays after the scope move the masters"
        assert E.same_bits(m.model_ema.flat, E.trajectory(seed_shadow, [f.cpu() for f in traj], EMA_DECAY, u0)), f"scoped={scoped}"
        legs.append((ex.tr.flat.cpu().clone(), m.model_ema.flat.cpu().clone()))
        del gs, opt, m
    (p0, s0), (p1, s1) = legs
    # the step captured before the scope, replayed after it, continues the run that never opened one
    _close("parameters after the scope against the leg without it", p1, p0)
    _close("shadows after the scope against the leg without it", s1, s0)


def test_log_images_samples_from_the_shadows():
    from tests.test_gpu_trainer_graph import _batches
    tr, _, _, _, _ = _fit(True, False, 6, 1)
    m = tr.model
    m.cond_stage_key = "txt"
    batch = dict(_batches(1)[0], txt=["a", "b"])
    m.get_unconditional_conditioning = lambda N: torch.zeros_like(batch["ctx"][:N])
    m.decode_first_stage = lambda z, *a, **k: z
    logs = {}
    for scope in (False, True):
        torch.manual_seed(5)
        logs[scope] = m.log_images(batch, N=2, ddim_steps=2, unconditional_guidance_scale=3.0, use_ema_scope=scope)
    torch.cuda.synchronize()
    assert set(logs[True]) == set(logs[False])
    key = "samples_cfg_scale_3.00"
    assert torch.isfinite(logs[True][key]).all() and not torch.equal(logs[True][key], logs[False][key])
    assert torch.equal(logs[True]["reconstruction"], logs[False]["reconstruction"])
    assert not m.model_ema.in_scope


# ------------------------------------------------------------------------------------------------ the scripts, end to end

def test_scripts_train_extract_and_sample_with_ema(tmp_path_factory, monkeypatch, collect_after):
    """train_ctrlora_finetune.py --ema_decay 0.999 --graph on the synthetic tiny set, then tool_extract_weights.py --ema and
    sample.py --use_ema, each in a fresh child process (tests/test_gpu_scripts.py)."""
    import yaml
    from tests.test_gpu_trainer_graph import _load
    out = str(tmp_path_factory.mktemp("synth_ema"))
    mod = _load(os.path.join(ROOT, "tests", "tools", "make_synthetic_assets.py"), "make_synthetic_assets")
    monkeypatch.setattr(sys, "argv", ["make_synthetic_assets.py", "--out", out, "--n", "4"])
    mod.main()
    monkeypatch.setenv("CTRLORA_SYNTHETIC_TOKENIZER", "1")
    cfg = os.path.join(out, "finetune_narrow.yaml")
    train = _load(os.path.join(ROOT, "scripts", "train_ctrlora_finetune.py"), "train_ctrlora_finetune")
    tr = train.main(["--dataroot", os.path.join(out, "custom"), "--config", cfg, "--sd_ckpt", os.path.join(out, "sd_synth.ckpt"),
                     "--cn_ckpt", os.path.join(out, "basecn_synth.ckpt"), "--graph", "--ema_decay", "0.999", "--bs", "2",
                     "--max_steps", "6", "--precision", "16", "--num_workers", "0", "--img_logger_freq", "1000",
                     "--ckpt_logger_freq", "2", "--lr", "1e-4", "-n", "ema"])
    torch.cuda.synchronize()
    assert tr.global_step == 6 and tr.graph_replays == 6 - tr.graph_eager_steps and tr.graph_replays > 0
    assert tr.optimizer.ema is tr.model.model_ema and int(tr.model.model_ema.num_updates) == 6
    import glob
    ckpt = max(glob.glob(os.path.join("runs", "ema", "**", "*.ckpt"), recursive=True), key=os.path.getmtime)
    ckpt = os.path.abspath(ckpt)
    blob = torch.load(ckpt, map_location="cpu", weights_only=False)
    sd = blob["state_dict"]
    assert int(sd["model_ema.num_updates"]) == int(blob["global_step"]) >= 3
    assert float(sd["model_ema.decay"]) == float(np.float32(0.999))
    del tr
    run = lambda *argv: subprocess.run([sys.executable, *argv], cwd=out, env=dict(os.environ), capture_output=True, text=True,
                                       timeout=600)
    lora_path = os.path.join(out, "ema_lora.ckpt")
    r = run(os.path.join(ROOT, "scripts", "tool_extract_weights.py"), "-t", "lora", "--ckpt", ckpt, "--save_path", lora_path, "--ema")
    assert r.returncode == 0, r.stderr[-3000:]
    lora = torch.load(lora_path, map_location="cpu", weights_only=False)
    assert lora and not any(k.startswith("model_ema.") for k in lora)
    moved = 0
    for k, v in lora.items():
        assert torch.equal(v, sd["model_ema." + k.replace(".", "")])
        moved += int(not torch.equal(v, sd[k]))
    assert moved > 0, "after these steps the average is not the weights"
    with open(cfg) as f:
        tree = yaml.safe_load(f)
    tree["model"]["params"].update(use_ema=True, ema_decay=0.999)
    cfg_ema = os.path.join(out, "finetune_narrow_ema.yaml")
    with open(cfg_ema, "w") as f:
        yaml.safe_dump(tree, f)
    save = os.path.join(out, "samples_ema")
    r = run(os.path.join(ROOT, "scripts", "sample.py"), "--dataroot", os.path.join(out, "custom"), "--config", cfg_ema, "--ckpt", ckpt,
            "--n_samples", "1", "--save_dir", save, "--ddim_steps", "2", "--use_ema")
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert "Switched to EMA weights" in r.stdout and os.path.exists(os.path.join(save, "sample", "0.png"))
    r = run(os.path.join(ROOT, "scripts", "sample.py"), "--dataroot", os.path.join(out, "custom"), "--config", cfg, "--ckpt", ckpt,
            "--n_samples", "1", "--save_dir", save, "--ddim_steps", "2", "--use_ema")
    assert r.returncode != 0 and "use_ema: true" in r.stderr
