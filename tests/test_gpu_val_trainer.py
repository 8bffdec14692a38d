"""Validation by timestep band on an MI355X, through the model and the Trainer.

Model: bench.build_model(..., tiny=True) (width 64, context 96, rank 32), B = 2, latent 16 x 16, the set-up of
tests/test_gpu_trainer_graph.py: batches are dicts with ready z, ctx, hint_z and get_input hands them through.  The validation set
is three full batches and a ragged one (7 samples).

  (a) an eager validation run and a GraphedEvalStep run (first batch eager, one capture, two replays, the ragged batch eager at
      its own size) give the same table bits, fp32 and bf16;
  (b) val/loss_simple is the mean of the per-sample l2 losses the test forms on the same triples with the model's own pieces
      (q_sample, apply_model, and the reduction p_losses runs on the GPU, cl_p_losses_mse with its per-sample output): within one
      fp32 rounding of the mean, 2^-24 relative, in fp32 -- the sums are fp64 on both sides, only their order differs -- and in
      bf16, where the bound is one bf16 rounding, 2^-9.  The per-sample losses also agree with an independent fp64 reduction of the
      same eps to the bound of the kernel's fp32 sum of positive terms: 2 + 1 + 6 + 2 + 16 + 1 = 28 roundings (the difference, which
      counts twice in its square, the square, the wave tree, the four waves, the 16 slices in order, the division),
      28 * 2^-24 relative;
  (c) graph_step=True, five optimizer steps with a validation run every two steps against five steps without: in fp32, with the
      fixed-order weight gradients (hip.WGRAD_F32_DETERMINISTIC: the default accumulates with float atomics in arrival order),
      the same bits in every parameter and every logged loss; in bf16, whose weight gradients always use atomics, within twice the
      spread of two runs without validation or the project's 1e-4 gate, whichever is larger.  As many replays as without
      validation, one capture of the training step, one of the validation step;
  (d) val_ema at decay 0.5: the _ema table differs from the live one, the masters are restored bit for bit, the training
      trajectory is that of a run without val_ema;
  (e) loss_bands: the table logged over each log interval has the bits of the host restatement applied to the per-sample losses
      and timesteps of the interval's steps, in the eager loop and under graph_step;
  (f) scripts/train_ctrlora_finetune.py --graph --val_every, from images and from a latent cache of the validation set.
"""
import json
import os
import sys
import time

import pytest
import torch

from tests.test_gpu_trainer_graph import _load, _params, _spread
from tests.util import ROOT

pytestmark = pytest.mark.gpu

B, H, CTX_DIM, SEED, GATE = 2, 16, 96, 7, 1e-4
DTYPES = {32: torch.float32, 16: torch.bfloat16}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(autouse=True)
def _workdir(tmp_path, monkeypatch):
    _need_gpu()
    monkeypatch.chdir(tmp_path)          # configure_optimizers writes ./tmp/finetune_trainable_params.txt, the trainer ./run


def _batches(n, seed=5, sizes=None):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g).cuda()
    sizes = sizes or [B] * n
    return [dict(z=mk(b, 4, H, H), ctx=mk(b, 77, CTX_DIM), hint_z=mk(b, 4, H, H) * 0.9) for b in sizes]


def _val_set():
    return _batches(4, seed=31, sizes=[B, B, B, 1])


def _model(ema=False):
    import bench

    def mutate(p):
        if ema:
            p.update(use_ema=True, ema_decay=0.5)

    m = bench.build_model("ctrlora_finetune_sd15_rank128.yaml", 0, tiny=True, mutate=mutate)
    m.learning_rate = 1e-3
    m.get_input = lambda batch, k, *a, **kw: (batch["z"], {"c_crossattn": [batch["ctx"]], "c_concat": [batch["hint_z"]]})
    return m


def _ready(precision, ema=False):
    m = _model(ema).cuda().train()
    m.set_engine_dtype(DTYPES[precision])
    return m, m.configure_optimizers()


def _fit(steps, precision=32, graph_step=True, model=None, callbacks=(), log_every=1, **kw):
    from ctrlora_amd.trainer import Trainer
    m = _model() if model is None else model
    val = kw.pop("val", None)
    tr = Trainer(max_steps=steps, precision=precision, callbacks=list(callbacks), default_root_dir="run",
                 log_every_n_steps=log_every, graph_step=graph_step, **kw)
    torch.manual_seed(SEED)
    tr.fit(m, _batches(steps), val_dataloaders=val)
    torch.cuda.synchronize()
    return tr


def _bits_equal(a, b):
    from tests import val_ref as V
    return V.same_bits(a.cpu(), b.cpu())


@pytest.mark.parametrize("precision", [32, 16], ids=["fp32", "bf16"])
def test_a_b_eager_and_graphed_runs_agree_and_the_mean_is_the_per_sample_mean(precision):
    from ctrlora_amd import hip
    from ctrlora_amd.validation import GraphedEvalStep, ValPlan, run_validation, table_logs
    m, _ = _ready(precision)
    plan = ValPlan(m.num_timesteps, nbands=10, seed=3)
    t0 = time.time()
    eager = run_validation(m, _val_set(), plan)
    assert m.training, "the module is back in train()"
    step = GraphedEvalStep(m, plan.nbands)
    rng = (torch.get_rng_state(), torch.cuda.get_rng_state())
    graphed = run_validation(m, _val_set(), plan, step=step)
    again = run_validation(m, _val_set(), plan, step=step)
    torch.cuda.synchronize()
    print(f"[val] precision {precision}: three runs of 7 samples in {time.time() - t0:.2f} s; total row {eager[-1].tolist()}")
    assert torch.equal(torch.get_rng_state(), rng[0]) and torch.equal(torch.cuda.get_rng_state(), rng[1])
    assert (step.eager_steps, step.captures, step.replays) == (1 + 2, 1, 2 + 3), (step.eager_steps, step.captures, step.replays)
    assert eager[-1, 0] == 7.0 and eager[:10, 0].tolist() == [1.0] * 7 + [0.0] * 3
    print(f"[val] precision {precision}: rows (= samples, one per band) whose sums differ, eager against graphed: "
          f"{(eager[:, 1] != graphed[:, 1]).nonzero().flatten().tolist()}, against the all-replay run: "
          f"{(eager[:, 1] != again[:, 1]).nonzero().flatten().tolist()}")
    assert _bits_equal(eager, graphed), (eager.cpu() - graphed.cpu()).abs().max()
    assert _bits_equal(eager, again), "a run that replays every batch, the first one included"
    assert m.engine()._rec is None and not m.loss_weights_pinned
    # (b)
    m.eval()
    per_all, ref_all, js = [], [], 0
    stream = plan.noise_stream(0, (4, H, H))
    with torch.no_grad():
        for b in _val_set():
            z, cond = m.get_input(b, m.first_stage_key)
            idx = list(range(js, js + z.shape[0]))
            js += z.shape[0]
            t, noise = plan.timesteps(idx).cuda(), stream.take(idx).cuda()
            eps = m.apply_model(m.q_sample(z, t, noise), t, cond).float().contiguous()
            out3, scratch = torch.empty(3, device="cuda"), torch.empty(16 * z.shape[0], device="cuda")
            per = torch.empty(z.shape[0], device="cuda")
            hip.p_losses_mse(eps, noise, None, t, None, out3, scratch, per_sample=per)
            per_all.append(per.double().cpu())
            ref_all.append(((eps.double() - noise.double()) ** 2).mean(dim=(1, 2, 3)).cpu())
    m.train()
    per_all, ref_all = torch.cat(per_all), torch.cat(ref_all)
    want = float(per_all.mean())
    got = table_logs(eager, plan)["val/loss_simple"]
    rel = abs(got - want) / want
    kernel_rel = float(((per_all - ref_all).abs() / ref_all).max())
    bound = 2.0 ** -24 if precision == 32 else 2.0 ** -9
    print(f"[val] precision {precision}: val/loss_simple {got!r}, mean of the per-sample losses {want!r}, relative difference "
          f"{rel:.3e} (bound {bound:.3e}); per-sample against an fp64 reduction: {kernel_rel:.3e} (bound {28 * 2.0 ** -24:.3e})")
    assert rel <= bound, (got, want, rel)
    if precision == 32:
        assert kernel_rel <= 28 * 2.0 ** -24, kernel_rel
    se = table_logs(eager, plan)["val/loss_simple_se"]
    assert abs(se - float(per_all.std() / 7 ** 0.5)) <= 1e-6 * se


def _count_captures(monkeypatch):
    from ctrlora_amd.train import GraphedTrainStep
    n = []
    real = GraphedTrainStep.capture
    monkeypatch.setattr(GraphedTrainStep, "capture", lambda self: (n.append(1), real(self))[1])
    return n


@pytest.mark.parametrize("precision", [32, 16], ids=["fp32", "bf16"])
def test_c_validation_inside_a_graphed_fit_leaves_the_trajectory_alone(precision, monkeypatch):
    from ctrlora_amd import hip
    if precision == 32:
        monkeypatch.setattr(hip, "WGRAD_F32_DETERMINISTIC", True)
    captures = _count_captures(monkeypatch)
    off = _fit(5, precision)
    n_off = len(captures)
    on = _fit(5, precision, val=_val_set(), val_check_interval=2)
    assert n_off == 1 and len(captures) == 2, "one capture of the training step per fit: validation causes no re-capture"
    assert [s for s, _ in on.logged_val] == [2, 4, 5] and not off.logged_val
    assert on.graph_replays == off.graph_replays == 3 and on.graph_eager_steps == off.graph_eager_steps == 2
    assert on._val_step is not None and on._val_step.captures == 1 and on._val_step.eager_steps == 1 + 3 and on._val_step.replays == 3 * 3 - 1
    assert int(on.optimizer._step) == 5 and not torch.cuda.is_current_stream_capturing()
    l_on, l_off = [v for _, v in on.logged], [v for _, v in off.logged]
    p_on, p_off = _params(on), _params(off)
    dl, dp = _spread(l_on, p_on, l_off, p_off)
    print(f"[val] precision {precision}: validation on against off: max rel loss diff {dl:.3e}, max param rel-L2 {dp:.3e}")
    if precision == 32:
        assert l_on == l_off, (l_on, l_off)
        assert all(torch.equal(p_on[k], p_off[k]) for k in p_off), [k for k in p_off if not torch.equal(p_on[k], p_off[k])][:5]
    else:
        again = _fit(5, precision)
        fl, fp = _spread([v for _, v in again.logged], _params(again), l_off, p_off)
        print(f"[val] bf16 off against off, same seed: max rel loss diff {fl:.3e}, max param rel-L2 {fp:.3e}")
        assert dl <= max(2 * fl, GATE) and dp <= max(2 * fp, GATE), (dl, dp, fl, fp)
    rows = [json.loads(ln) for ln in open(os.path.join(on.log_dir, "val_log.jsonl"))]
    assert [r["global_step"] for r in rows] == [2, 4, 5] and all(r["val/loss_simple"] > 0 for r in rows)
    vals = [logs["val/loss_simple"] for _, logs in on.logged_val]
    assert len(set(vals)) == 3, f"the weights moved between the runs: {vals}"


def test_c_eager_fit_validates_on_the_engine_without_a_graph(monkeypatch):
    """graph_step off: the same runs through eager launches of engine_eval_step; the tables of a run are those of the graphed fit
    when the trajectories are (fp32, fixed-order weight gradients are not needed for that: the first run precedes any difference
    only in step order, so only its presence and the trajectory are checked here)."""
    from ctrlora_amd import hip
    monkeypatch.setattr(hip, "WGRAD_F32_DETERMINISTIC", True)
    off = _fit(3, 32, graph_step=False)
    on = _fit(3, 32, graph_step=False, val=_val_set(), val_check_interval=2, save_best=True)
    assert on._val_step is None and on._val_on_engine and [s for s, _ in on.logged_val] == [2, 3]
    assert [v for _, v in on.logged] == [v for _, v in off.logged]
    p_on, p_off = _params(on), _params(off)
    assert all(torch.equal(p_on[k], p_off[k]) for k in p_off)
    assert os.path.exists(os.path.join(on.checkpoint_callback.dirpath, "best.ckpt"))


@pytest.mark.parametrize("precision", [32, 16], ids=["fp32", "bf16"])
def test_d_val_ema_fills_a_second_table_and_restores_the_masters(precision, monkeypatch):
    from ctrlora_amd import hip
    if precision == 32:
        monkeypatch.setattr(hip, "WGRAD_F32_DETERMINISTIC", True)
    plain = _fit(4, precision, model=_model(ema=True), val=_val_set(), val_check_interval=2)
    ema = _fit(4, precision, model=_model(ema=True), val=_val_set(), val_check_interval=2, val_ema=True)
    assert ema.val_tables.shape == (2, 11, 3) and plain.val_tables.shape == (1, 11, 3)
    assert not _bits_equal(ema.val_tables[0], ema.val_tables[1]), "decay 0.5 after four steps: the average is not the live weights"
    assert ema.val_tables[1, -1, 0] == 7.0 and not ema.model.model_ema.in_scope
    for _, logs in ema.logged_val:
        assert "val/loss_simple_ema" in logs and "val/loss_simple_se_ema" in logs and "val/loss_simple/t0-99_ema" in logs
        assert logs["val/loss_simple_ema"] != logs["val/loss_simple"]
    ex = ema.model.control_model.executor()
    if precision == 32:
        assert torch.equal(ex.tr.flat, plain.model.control_model.executor().tr.flat), "the masters are restored bit for bit"
        assert [v for _, v in ema.logged] == [v for _, v in plain.logged]
        assert _bits_equal(ema.val_tables[0], plain.val_tables[0])
    # the scope itself, measured directly: masters before == masters after, and the packs follow (a run gives the live bits again)
    from ctrlora_amd.validation import run_validation
    before = ex.tr.flat.clone()
    live = run_validation(ema.model, _val_set(), ema.val_plan, step=ema._val_step)
    with ema.model.ema_scope():
        inside = run_validation(ema.model, _val_set(), ema.val_plan, step=ema._val_step)
    after = run_validation(ema.model, _val_set(), ema.val_plan, step=ema._val_step)
    assert torch.equal(ex.tr.flat, before) and _bits_equal(live, after) and not _bits_equal(live, inside)
    assert _bits_equal(live, ema.val_tables[0]) and _bits_equal(inside, ema.val_tables[1])


@pytest.mark.parametrize("graph_step", [False, True], ids=["eager", "replayed"])
def test_e_training_loss_bands_are_the_host_restatement_of_the_steps_losses(graph_step):
    from ctrlora_amd.validation import accumulate_bands, new_table
    seen = []

    class Keep:
        def on_train_batch_end(self, trainer, module, outputs, batch, batch_idx):
            per, t = trainer._train_bands.last
            seen.append((per.detach().clone().cpu(), t.detach().clone().cpu()))

    tr = _fit(6, 32, graph_step=graph_step, callbacks=[Keep()], log_every=2, loss_bands=10)
    assert [s for s, _ in tr.logged_train_bands] == [2, 4, 6] and len(seen) == 6
    if graph_step:
        assert tr.graph_replays == 4 and tr.graph_eager_steps == 2
    assert tr.model.train_loss_bands is None, "the table leaves the model with the fit"
    for k, (_, tab) in enumerate(tr.logged_train_bands):
        want = new_table(10)
        for per, t in seen[2 * k:2 * k + 2]:
            assert per.shape == (B,) and t.shape == (B,)
            accumulate_bands(per, t, 1000, 10, want)
        assert _bits_equal(tab, want), (k, tab, want)
        assert tab[-1, 0] == 2.0 * B
    assert len({float(p[0]) for p, _ in seen}) == 6, "six different batches"
    keys = [k for k in tr.model.last_logged if k.startswith("train/loss_simple/t")]
    assert keys and all(tr.model.last_logged[k] > 0 for k in keys)
    # the mean over an interval's band rows is the mean of the logged loss_simple of its steps, to fp32 rounding
    per, _ = seen[-1]
    assert abs(float(per.double().mean()) - tr.logged[-1][1]) <= 2.0 ** -22 * tr.logged[-1][1]


# ---------------------------------------------------------------------------------------------------- the script, end to end

@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    _need_gpu()
    out = str(tmp_path_factory.mktemp("synth_val"))
    mod = _load(os.path.join(ROOT, "tests", "tools", "make_synthetic_assets.py"), "make_synthetic_assets")
    argv, sys.argv = sys.argv, ["make_synthetic_assets.py", "--out", out, "--n", "4"]
    try:
        mod.main()
    finally:
        sys.argv = argv
    mp = pytest.MonkeyPatch()
    try:
        mp.setenv("CTRLORA_SYNTHETIC_TOKENIZER", "1")
        mp.chdir(tmp_path_factory.mktemp("cache_tool_cwd"))
        cache = os.path.join(out, "latents_bf16")
        _load(os.path.join(ROOT, "scripts", "tool_cache_latents.py"), "tool_cache_latents").main(
            ["--dataroot", os.path.join(out, "custom"), "--config", os.path.join(out, "finetune_narrow.yaml"),
             "--sd_ckpt", os.path.join(out, "sd_synth.ckpt"), "--out", cache, "--bs", "4", "--precision", "16"])
    finally:
        mp.undo()
    return out, cache


@pytest.mark.parametrize("cached", [False, True], ids=["live", "val_latent_cache"])
def test_f_finetune_script_with_val_every(assets, cached, monkeypatch):
    """--graph --val_every 2 --val_ema --save_best --loss_bands 4 for five steps; the validation set is the synthetic set itself
    (4 pairs, two batches), read from its images or from its latent cache."""
    out, cache = assets
    monkeypatch.setenv("CTRLORA_SYNTHETIC_TOKENIZER", "1")
    train = _load(os.path.join(ROOT, "scripts", "train_ctrlora_finetune.py"), "train_ctrlora_finetune")
    root = os.path.join(out, "custom")
    args = ["--dataroot", root, "--config", os.path.join(out, "finetune_narrow.yaml"), "--sd_ckpt", os.path.join(out, "sd_synth.ckpt"),
            "--cn_ckpt", os.path.join(out, "basecn_synth.ckpt"), "--graph", "--bs", "2", "--max_steps", "5", "--precision", "16",
            "--num_workers", "0", "--img_logger_freq", "1000", "--ckpt_logger_freq", "1000", "--lr", "1e-4", "--ema_decay", "0.9",
            "-n", "v_cached" if cached else "v_live", "--val_dataroot", root, "--val_every", "2", "--val_bands", "4", "--val_repeats", "2",
            "--val_seed", "1", "--val_ema", "--save_best", "--loss_bands", "4"] + (["--val_latent_cache", cache] if cached else [])
    t0 = time.time()
    tr = train.main(args)
    torch.cuda.synchronize()
    print(f"[val] script --graph --val_every ({'val latent cache' if cached else 'live first stage'}): {time.time() - t0:.1f} s wall")
    assert tr.global_step == 5 and tr.graph_replays == 5 - tr.graph_eager_steps and tr.graph_replays > 0
    assert [s for s, _ in tr.logged_val] == [2, 4, 5]
    assert tr.val_tables.shape == (2, 5, 3) and tr.val_tables[0, -1, 0] == 8.0 and tr.val_tables[0, :4, 0].tolist() == [2.0] * 4
    assert tr._val_step is not None and tr._val_step.captures == 1 and tr._val_step.replays > 0
    rows = [json.loads(ln) for ln in open(os.path.join(tr.log_dir, "val_log.jsonl"))]
    assert len(rows) == 3 and all(r["val/loss_simple"] > 0 and r["val/loss_simple_ema"] > 0 for r in rows)
    assert set(rows[0]) >= {"val/loss_simple/t0-249", "val/loss_simple/t750-999_ema", "val/loss_simple_se", "global_step"}
    assert os.path.exists(os.path.join(tr.checkpoint_callback.dirpath, "best.ckpt"))
    assert tr.val_plan.seed == 1 and tr.val_plan.repeats == 2 and tr.val_plan.nbands == 4
    assert not torch.cuda.is_current_stream_capturing()

    def without(flag):
        k = args.index(flag)
        return args[:k] + args[k + 2:]

    with pytest.raises(SystemExit, match="--val_every needs a validation set"):
        train.main(without("--val_dataroot"))
    with pytest.raises(SystemExit, match="--val_ema needs --ema_decay"):
        train.main(without("--ema_decay"))
