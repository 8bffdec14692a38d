"""Global gradient norm and clipping on the device (cl_grad_norm, cl_adamw_dev_clip; ctrlora_amd.train._FlatAdamW;
Trainer(gradient_clip_val=, track_grad_norm=)) on an MI355X.

Kernels: every row of tests/grad_clip_ref.py under its gates (norm within 2 fp32 ulp of fp64, coef bit-equal to the fp32 formula on
the kernel's own norm, two launches the same bits, guards of 1e30 around every buffer, NaN / inf rows, refusals that leave `out`
untouched); cl_adamw_dev_clip against cl_adamw_dev (coef 1: the same bits) and against tests/ew_ref.py's adamw bound (coef 0.37).

Optimizer step, on the tiny fine-tune model of tests/test_gpu_trainer_graph.py: off and far above the norms -- the bits of today's
step from the same state; acting -- against clip_grad_norm_ + torch.optim.AdamW on the engine's own gradient, gated at twice the
error the same comparison shows with clipping off (measured here, appended to profiles/grad_clip/parity_measured.jsonl) plus one
fp32 ulp of the parameter; replayed through Trainer(graph_step=...) and GraphedTrainStep; pre-training with per-task graphs."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import ew_ref as R
from tests import grad_clip_ref as G
from tests.util import ROOT, rel_l2

pytestmark = pytest.mark.gpu

PATTERN = -7.25
HYPER = (1e-3, 0.9, 0.999, 1e-8, 1e-2)


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


# ------------------------------------------------------------------------------------------------ cl_grad_norm

def _launch_norm(hip, row):
    """Two launches of a row on fresh `out` slots: ([(norm, coef) as numpy float32] x 2, the buffers, the launch record)."""
    bufs = G.make_bufs(row, "cuda")
    views = [v for _, v in bufs]
    hyper = torch.tensor(HYPER + (row["scale"],), dtype=torch.float32).cuda()
    mx = None if row["max_norm"] is None else torch.tensor([row["max_norm"]], dtype=torch.float32).cuda()
    scratch = torch.full((hip.grad_norm_scratch_floats(len(views)) + 16,), float("nan"), device="cuda")
    got = []
    for _ in range(2):
        out = torch.full((18,), PATTERN, device="cuda")
        hip.grad_norm(views, hyper, mx, out[8:10], scratch[:-16])
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert (o[:8] == PATTERN).all() and (o[10:] == PATTERN).all(), "wrote outside out[0..1]"
        got.append((o[8], o[9]))
    assert bool(torch.isnan(scratch[-16:]).all()), "wrote past the scratch slab"
    return got, bufs, _probe(hip)


@pytest.mark.parametrize("name", [r["name"] for r in G.CASES])
def test_grad_norm_rows(name):
    hip = _hip()
    row = G.ROW[name]
    got, bufs, rec = _launch_norm(hip, row)
    total = sum(row["counts"])
    groups = min(512, max(1, -(-total // 1024)))
    assert rec == dict(id=_ew_id("EW_GRAD_NORM"), dtype=-1, gx=groups, gy=1, gz=1, threads=256, form=0, aux=len(row["counts"])), rec
    assert all(G.guards_intact(b, v) for b, v in bufs), "the kernel is read-only"
    cpu_views = [v for _, v in G.make_bufs(row)]
    (n0, c0), (n1, c1) = got
    ref = G.norm64(cpu_views, row["scale"])
    print(f"[grad norm] {name}: norm {float(n0)!r} (fp64 {ref!r}), coef {float(c0)!r}, {groups} workgroups")
    flags = G.judge(row, cpu_views, n0, c0)
    assert flags == [], flags
    assert np.array([n0, c0]).view(np.uint32).tolist() == np.array([n1, c1]).view(np.uint32).tolist(), "two launches, two results"
    if row["plant"] is not None:
        if row["plant"][0] == "nan":
            assert n0 != n0 and c0 != c0
        else:
            assert np.isinf(n0) and n0 > 0 and float(c0) == 0.0
    if row["max_norm"] is None or row["max_norm"] <= 0:
        assert float(c0) == 1.0


def test_grad_norm_refusals_leave_out_untouched():
    hip = _hip()
    L = hip.lib()
    st = hip.stream()
    g = torch.randn(64, device="cuda")
    hyper = torch.tensor(HYPER + (1.0,), dtype=torch.float32).cuda()
    mx = torch.ones(1, device="cuda")
    out = torch.full((2,), PATTERN, device="cuda")
    scratch = torch.zeros(hip.grad_norm_scratch_floats(1), device="cuda")
    p, h, m, o, s = g.data_ptr(), hyper.data_ptr(), mx.data_ptr(), out.data_ptr(), scratch.data_ptr()
    bufs = lambda *a: (ctypes.c_void_p * 17)(*a)
    cnt = lambda *a: (ctypes.c_long * 17)(*a)
    calls = {
        "nbuf=0": L.cl_grad_norm(bufs(p), cnt(4), 0, h, m, o, s, st), "nbuf=17": L.cl_grad_norm(bufs(*[p] * 17), cnt(*[1] * 17), 17, h, m, o, s, st),
        "count<0": L.cl_grad_norm(bufs(p, p), cnt(4, -1), 2, h, m, o, s, st), "null scratch": L.cl_grad_norm(bufs(p), cnt(4), 1, h, m, o, None, st),
        "null hyper": L.cl_grad_norm(bufs(p), cnt(4), 1, None, m, o, s, st), "null out": L.cl_grad_norm(bufs(p), cnt(4), 1, h, m, None, s, st),
        "null buffer, count>0": L.cl_grad_norm(bufs(p, None), cnt(4, 4), 2, h, m, o, s, st),
    }
    torch.cuda.synchronize()
    assert {k: v for k, v in calls.items() if v != 1} == {}
    assert _probe(hip)["id"] == 0 and out.tolist() == [PATTERN, PATTERN] and float(scratch.abs().sum()) == 0.0
    # a null max_norm is tracking only, a null buffer with count 0 is fine
    assert L.cl_grad_norm(bufs(p, None), cnt(64, 0), 2, h, None, o, s, st) == 0
    torch.cuda.synchronize()
    assert abs(float(out[0]) - float(g.double().norm())) <= 2 * G.ulp32(float(out[0])) and float(out[1]) == 1.0


# ------------------------------------------------------------------------------------------------ cl_adamw_dev_clip

class _Guarded:
    def __init__(self, init):
        n = init.numel()
        self.buf = torch.full((n + 128,), PATTERN, device="cuda")
        self.view = self.buf[64:64 + n]
        self.view.copy_(init)

    def intact(self):
        return bool((self.buf[:64] == PATTERN).all()) and bool((self.buf[64 + self.view.numel():] == PATTERN).all())


@pytest.mark.parametrize("n", G.ADAMW_N)
def test_adamw_dev_clip(n):
    hip = _hip()
    H = R.ADAMW_HYPER
    ops = G.adamw_ops(n)
    hyper = torch.tensor([H[k] for k in ("lr", "beta1", "beta2", "eps", "wd", "gscale")], dtype=torch.float32).cuda()
    step = torch.tensor([2], dtype=torch.int32).cuda()
    g = ops["g"].cuda()

    def run(coef):
        pmv = [_Guarded(ops[k]) for k in "pmv"]
        if coef is None:
            hip.adamw_dev(pmv[0].view, g, pmv[1].view, pmv[2].view, hyper, step)
            want_id = "EW_ADAMW_DEV"
        else:
            clip = torch.tensor([123.0, coef], dtype=torch.float32).cuda()
            hip.adamw_dev_clip(pmv[0].view, g, pmv[1].view, pmv[2].view, hyper, step, clip)
            want_id = "EW_ADAMW_DEV_CLIP"
        torch.cuda.synchronize()
        assert _probe(hip) == dict(id=_ew_id(want_id), dtype=-1, gx=R.ew_grid(n), gy=1, gz=1, threads=256, form=0, aux=0)
        assert all(t.intact() for t in pmv) and int(step[0]) == 2
        return [t.view.cpu().clone() for t in pmv]

    plain, one = run(None), run(1.0)
    for k, a, b in zip("pmv", plain, one):
        assert torch.equal(a, b) and R.same_bits(a, b), f"coef 1.0f: {k} differs from cl_adamw_dev"
    coef = float(np.float32(0.37))
    got = run(coef)
    state = (ops["p"], ops["m"], ops["v"])
    flags = G.adamw_flags(got, G.adamw_specs(state, ops["g"], 2, H["gscale"], coef))
    assert flags == [], flags
    assert not torch.equal(got[1], plain[1]), "the coefficient must reach the moments"
    # and the unclipped result is outside that bound: the gate sees the coefficient
    assert G.adamw_flags(plain, G.adamw_specs(state, ops["g"], 2, H["gscale"], coef)) != []


# ------------------------------------------------------------------------------------------------ the optimizer step

def _tiny(dtype=torch.float32):
    from tests.test_gpu_trainer_graph import _model
    m = _model().cuda().train()
    m.set_engine_dtype(dtype)
    return m


def _steps(n=4):
    """n micro-batches (z, ctx, hint, t, noise), the same in every leg."""
    from tests.test_gpu_trainer_graph import B, H, _batches
    g = torch.Generator().manual_seed(11)
    out = []
    for b in _batches(n, seed=9):
        t = torch.randint(0, 1000, (B,), generator=g).cuda()
        out.append((b["z"], b["ctx"], b["hint_z"], t, torch.randn(B, 4, H, H, generator=g).cuda()))
    return out


def _backward(m, opt, batch):
    z, ctx, hint, t, noise = batch
    opt.zero_grad()
    loss, _ = m.p_losses(z, {"c_crossattn": [ctx], "c_concat": [hint]}, t, noise=noise)
    loss.backward()
    return float(loss.detach())


def _state(opt):
    return [t.clone() for ex, st in zip(opt.executors, opt._states) for t in (ex.tr.flat, st.m, st.v)] + [opt._step_dev.clone()]


def _restore(opt, snap):
    live = [t for ex, st in zip(opt.executors, opt._states) for t in (ex.tr.flat, st.m, st.v)] + [opt._step_dev]
    for a, b in zip(live, snap):
        a.copy_(b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_off_and_far_above_are_todays_step_bit_for_bit(dtype):
    """Four steps; at each, from the same state and gradient: the step with the feature off, with a threshold far above the norm,
    and with tracking alone -- the same parameters and moments, bit for bit."""
    m = _tiny(dtype)
    opt = m.configure_optimizers()
    for batch in _steps(4):
        _backward(m, opt, batch)
        before = _state(opt)
        results = []
        for setting in (dict(max_grad_norm=None, track_grad_norm=False), dict(max_grad_norm=1e9, track_grad_norm=False),
                        dict(max_grad_norm=None, track_grad_norm=True)):
            _restore(opt, before)
            opt.max_grad_norm, opt.track_grad_norm = setting["max_grad_norm"], setting["track_grad_norm"]
            opt.step()
            torch.cuda.synchronize()
            results.append(_state(opt))
            if opt.norm_enabled:
                norm, coef = (float(v) for v in opt.last_grad_norm())
                want = float(torch.cat([ex.tr.flat_grad for ex in opt.executors]).double().norm())
                assert coef == 1.0 and abs(norm - want) <= 2 * G.ulp32(want), (norm, want, coef)
        for other in results[1:]:
            assert all(torch.equal(a, b) for a, b in zip(results[0], other))
        assert not torch.equal(results[0][0], before[0]), "the step moved nothing"
    assert int(opt._step) == 4


def _replica_run(max_norm):
    """Four engine steps (fp32) next to clip_grad_norm_ + torch.optim.AdamW on fp32 clones fed the engine's own flat gradient:
    per step (engine parameters, replica parameters, norm, coef) on the CPU."""
    m = _tiny()
    opt = m.configure_optimizers()
    opt.max_grad_norm = max_norm
    (ex,) = opt.executors
    g0 = opt.param_groups[0]
    p = torch.nn.Parameter(ex.tr.flat.detach().clone())
    ref = torch.optim.AdamW([p], lr=g0["lr"], betas=g0["betas"], eps=g0["eps"], weight_decay=g0["weight_decay"])
    out = []
    for batch in _steps(4):
        _backward(m, opt, batch)
        p.grad = ex.tr.flat_grad.detach().clone()
        norm = float(torch.nn.utils.clip_grad_norm_([p], max_norm if max_norm else float("inf")))
        opt.step()
        ref.step()
        torch.cuda.synchronize()
        mine = tuple(float(v) for v in opt.last_grad_norm()) if opt.norm_enabled else (None, None)
        out.append((ex.tr.flat.detach().cpu().clone(), p.detach().cpu().clone(), norm, mine))
    return out


def test_acting_clip_follows_torch_within_twice_the_unclipped_error():
    """Comparator rule: the engine against the torch replica with clipping ON may differ by twice what the same comparison shows
    with clipping OFF (measured here, per step) plus one fp32 ulp of the parameter."""
    off = _replica_run(None)
    threshold = 0.5 * off[0][2]
    on = _replica_run(threshold)
    worst = []
    for s, ((e0, r0, _, _), (e1, r1, norm_t, (norm, coef))) in enumerate(zip(off, on)):
        assert norm_t > threshold and coef < 1.0, f"step {s + 1}: clipping did not act (norm {norm_t}, threshold {threshold})"
        assert abs(norm - norm_t) <= 1e-6 * norm_t, (norm, norm_t)      # torch's own norm is an fp32 tree reduction: ~log2(n) 2^-24
        want_coef = G.coef32(np.float32(norm), threshold)
        assert np.float32(coef) == want_coef
        err_off = float((e0 - r0).abs().max())
        err_on = (e1 - r1).abs()
        ulp = torch.from_numpy(np.spacing(np.abs(r1.numpy())))
        over = err_on - (2 * err_off + ulp)
        worst.append(dict(step=s + 1, err_off=err_off, err_on=float(err_on.max()), threshold=threshold, norm=norm, coef=coef))
        print(f"[grad clip] step {s + 1}: engine against torch, max abs error {err_off:.3e} off, {float(err_on.max()):.3e} on "
              f"(norm {norm:.5f}, coef {coef:.5f})")
        assert not bool((over > 0).any()), worst[-1]
    assert not torch.equal(on[-1][0], off[-1][0]), "clipping changed nothing"
    path = os.path.join(ROOT, "profiles", "grad_clip", "parity_measured.jsonl")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as f:
        f.write(json.dumps(dict(test="acting_clip_vs_torch", model="tiny fine-tune, fp32", steps=worst)) + "\n")


# ------------------------------------------------------------------------------------------------ Trainer, eager and replayed

_RUNS = {}


def _fit(graph_step, steps, acc, clip, track=False):
    from ctrlora_amd.trainer import Trainer
    from tests.test_gpu_trainer_graph import SEED, _batches, _model
    key = (repr(graph_step), steps, acc, clip, track)
    if key not in _RUNS:
        tr = Trainer(max_steps=steps, accumulate_grad_batches=acc, precision=32, default_root_dir="run", log_every_n_steps=1,
                     graph_step=graph_step, gradient_clip_val=clip, track_grad_norm=2 if track else -1)
        torch.manual_seed(SEED)
        tr.fit(_model(), _batches(steps * acc))
        torch.cuda.synchronize()
        params = {k: v.detach().float().cpu().clone() for k, v in tr.model.control_model.named_parameters()}
        _RUNS[key] = (tr, [v for _, v in tr.logged], params, [v for _, v in tr.logged_grad_norm])
    return _RUNS[key]


def _threshold(acc=1):
    """Half the first step's norm of the unclipped eager run (tracking alone), so that clipping acts."""
    _, _, _, norms = _fit(False, 4, acc, None, track=True)
    assert len(norms) == 4 and all(n > 0 for n in norms)
    return 0.5 * norms[0]


@pytest.mark.parametrize("form", ["one-acc1", "one-acc2", "segmented-acc2"])
def test_trainer_replays_the_clipped_step(form):
    from tests.test_gpu_trainer_graph import GATE, _assert_same
    acc = 2 if form.endswith("acc2") else 1
    clip = _threshold(acc)
    graph_step = dict(split_graphs="segmented", bucket_bytes=256 << 10, reduce_fn=lambda buf: None) if form.startswith("segmented") else True
    _, want_l, want_p, want_n = _fit(False, 4, acc, clip)
    tr, losses, params, norms = _fit(graph_step, 4, acc, clip)
    assert tr.graph_replays > 0 and tr.graph_replays == 4 - tr.graph_eager_steps and int(tr.optimizer._step) == 4
    assert tr.graph_mode == ("segmented" if form.startswith("segmented") else "one")
    assert tr.optimizer.max_grad_norm == clip and tr.optimizer.norm_enabled
    _assert_same(f"clipped, {form}: graph against eager", (losses, params), (want_l, want_p))
    # train/grad_norm as logged from the replayed run is the eager run's, and clipping acted on every step of both
    assert len(norms) == len(want_n) == 4 and all(n > clip for n in norms + want_n), (clip, norms, want_n)
    assert all(abs(a - b) <= GATE * abs(b) for a, b in zip(norms, want_n)), (norms, want_n)
    assert tr.model.last_logged["train/grad_norm"] == norms[-1] and "train/loss" in tr.model.last_logged
    # and the clipped trajectory is not the free one
    _, _, free_p, _ = _fit(False, 4, 1, None, track=True)
    if acc == 1:
        assert max(rel_l2(params[k], free_p[k]) for k in params) > 10 * GATE


def test_threshold_change_between_replays_needs_no_recapture():
    from ctrlora_amd.train import GraphedTrainStep
    m = _tiny()
    opt = m.configure_optimizers()
    opt.max_grad_norm = 1e9
    batches = _steps(4)
    gs = GraphedTrainStep(m, opt, *batches[0], warmup=0, capture=False)
    gs.eager(*batches[0])
    gs.capture()
    graphs = [id(s[0]) for s in gs.segments]
    gs(*batches[1])
    torch.cuda.synchronize()
    norm, coef = (float(v) for v in opt.last_grad_norm())
    assert coef == 1.0 and norm > 0
    opt.max_grad_norm = 0.25 * norm
    gs(*batches[2])
    torch.cuda.synchronize()
    norm2, coef2 = (float(v) for v in opt.last_grad_norm())
    assert np.float32(coef2) == G.coef32(np.float32(norm2), 0.25 * norm) and coef2 < 1.0
    opt.max_grad_norm = None                     # off again: the captured norm stays, as tracking
    opt.track_grad_norm = True
    gs(*batches[3])
    torch.cuda.synchronize()
    assert float(opt.last_grad_norm()[1]) == 1.0
    assert [id(s[0]) for s in gs.segments] == graphs and int(opt._step) == 4


# ------------------------------------------------------------------------------------------------ pre-training

def test_pretraining_norm_covers_base_and_active_banks_and_replays():
    from ctrlora_amd.train import GraphedPretrainStep
    from tests.golden.make_golden_pretrain import LR, TASKS, step_inputs
    from tests.test_pretrain import _model
    seq = ["hed", "canny", "hed", "hed", "canny", "canny", "hed", "canny"]
    cu = lambda v: v.cuda()
    results = []
    threshold = None
    for graphed in (False, True):
        m, cfg = _model(torch.bfloat16)
        m.learning_rate = LR * 0.1
        opt = m.configure_optimizers()
        opt.track_grad_norm = True            # the eager leg sets the threshold from its first step's norm, below
        opt.max_grad_norm = threshold
        cm = m.control_model
        inp0 = step_inputs(cfg, 0)
        g = GraphedPretrainStep(m, opt, cu(inp0["z"]), cu(inp0["ctx"]), cu(inp0["hint_z"]), cu(inp0["t"]), cu(inp0["noise"])) if graphed else None
        losses, norms = [], []
        for i, task in enumerate(seq):
            inp = step_inputs(cfg, i % 3)
            z, ctx, hint, t, noise = cu(inp["z"]), cu(inp["ctx"]), cu(inp["hint_z"]), cu(inp["t"]), cu(inp["noise"])
            if graphed:
                losses.append(float(g(task, z, ctx, hint, t, noise)))
            else:
                opt.zero_grad()
                loss3 = m.engine_train_step(z, {"c_crossattn": [ctx], "c_concat": [hint], "task": task}, t, noise)
                # the torch replica: every parameter whose .grad is not None in the reference = base + the banks used so far
                active = list(dict.fromkeys(list(opt.active) + [task]))
                grads = [p.grad for n, p in cm.named_parameters() if "lora_layer" not in n and not n.startswith("loras_dict.")]
                grads += [getattr(lora, part).weight.grad for t_ in TASKS if t_ in active for lora in cm.loras_dict[t_] for part in ("down", "up")]
                want = float(torch.norm(torch.stack([gr.detach().double().norm() for gr in grads if gr is not None])))
                if threshold is None:
                    threshold = opt.max_grad_norm = 0.5 * want          # half the first step's norm: clipping acts
                opt.step()
                losses.append(float(loss3[2]))
                assert opt.active == active
                got = float(opt.last_grad_norm()[0])
                assert abs(got - want) <= 1e-6 * want, (i, task, got, want)
            norms.append(tuple(float(v) for v in opt.last_grad_norm()))
        torch.cuda.synchronize()
        params = {n: p.detach().float().cpu().clone() for n, p in m.control_model.named_parameters()}
        results.append((losses, params, norms, None if g is None else (len(g.graphs), g.eager_steps)))
        del m, opt, g
    (l_e, p_e, n_e, _), (l_g, p_g, n_g, info) = results
    assert info[0] == 2 and info[1] <= 4, info
    assert all(c < 1.0 for _, c in n_e), f"clipping must act: {n_e}"
    assert all(abs(a - b) <= 1e-5 * abs(a) for a, b in zip(l_e, l_g)), (l_e, l_g)
    assert all(abs(a[0] - b[0]) <= 1e-5 * a[0] and abs(a[1] - b[1]) <= 1e-5 * a[1] for a, b in zip(n_e, n_g)), (n_e, n_g)
    worst = max(rel_l2(p_g[n], p_e[n]) for n in p_e)
    assert worst < 1e-5, worst


# ------------------------------------------------------------------------------------------------ the script, end to end

def test_finetune_script_with_graph_and_grad_clip(tmp_path_factory, monkeypatch):
    """scripts/train_ctrlora_finetune.py --graph --grad_clip 1.0 for 50 steps (the script logs every 50th): replays, and a logged
    train/grad_norm."""
    import sys
    from tests.test_gpu_trainer_graph import _load
    out = str(tmp_path_factory.mktemp("synth_grad_clip"))
    mod = _load(os.path.join(ROOT, "tests", "tools", "make_synthetic_assets.py"), "make_synthetic_assets")
    monkeypatch.setattr(sys, "argv", ["make_synthetic_assets.py", "--out", out, "--n", "4"])
    mod.main()
    monkeypatch.setenv("CTRLORA_SYNTHETIC_TOKENIZER", "1")
    train = _load(os.path.join(ROOT, "scripts", "train_ctrlora_finetune.py"), "train_ctrlora_finetune")
    tr = train.main(["--dataroot", os.path.join(out, "custom"), "--config", os.path.join(out, "finetune_narrow.yaml"),
                     "--sd_ckpt", os.path.join(out, "sd_synth.ckpt"), "--cn_ckpt", os.path.join(out, "basecn_synth.ckpt"), "--graph",
                     "--grad_clip", "1.0", "--bs", "2", "--max_steps", "50", "--precision", "16", "--num_workers", "0",
                     "--img_logger_freq", "1000", "--ckpt_logger_freq", "1000", "--lr", "1e-4", "-n", "g_clip"])
    torch.cuda.synchronize()
    assert tr.global_step == 50 and int(tr.optimizer._step) == 50
    assert tr.graph_mode == "one" and tr.graph_replays == 50 - tr.graph_eager_steps and tr.graph_replays > 0
    assert tr.optimizer.max_grad_norm == 1.0 and tr.gradient_clip_val == 1.0
    ((step, norm),) = tr.logged_grad_norm
    assert step == 50 and norm == norm and 0.0 < norm < float("inf")
    assert tr.model.last_logged["train/grad_norm"] == norm and "train/loss" in tr.model.last_logged
    coef = float(tr.optimizer.last_grad_norm()[1])
    assert np.float32(coef) == G.coef32(np.float32(norm), 1.0)
