"""What validation by timestep band costs, on one MI355X.

    python tools/bench_val.py [--iters 50] [--rounds 12] [--warmup 4] [--batch 8] [--samples 256] [--tiny]

Workload: bench.py's model (configs/ctrlora_finetune_sd15_rank128.yaml, random weights, bf16 engine mode), B = 8, 64 x 64 latents.

  (a) kernels: cl_loss_bands (B samples, 10 bands) next to the cl_p_losses_mse pair it follows (no d_eps, with per_sample), hot,
      isolated, each between HIP events, alternating in one run; medians of --iters and each leg's min and max.
  (b) the forward-only validation step (ControlFinetuneLDM.engine_eval_step): launched eagerly against replayed as one hipGraph
      (ctrlora_amd.validation.GraphedEvalStep), and against the replayed training step of the same process (GraphedTrainStep,
      loss_bands off: the launch list of the step before this feature existed).  Legs alternate; medians of --rounds.
  (c) the replayed training step with Trainer(loss_bands=10)'s table attached against without: twin models, the legs alternating
      step by step, medians of --rounds.  Criterion: the on leg's median lies within the off leg's own min .. max.
  (d) wall time of one validation run of --samples samples, 10 bands, inside a graph_step fit of the Trainer, with and without
      val_ema: host clock around Trainer._validate ending in a device synchronise, after the fit's own runs have captured and
      warmed the validation graph; median of 3.  The batches are ready latents: the first stage and the text encoder, which a
      real run pays per batch outside the graph, are not in this number.

Writes profiles/val/bench_val.json and prints it as ONE JSON line.  No GPU, no number: the tool fails."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn, iters):
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def _leg_us(ms):
    return dict(us=round(statistics.median(ms) * 1e3, 2), us_min_max=[round(min(ms) * 1e3, 2), round(max(ms) * 1e3, 2)], samples=len(ms))


def _leg_ms(ms, B):
    med = statistics.median(ms)
    return dict(ms_per_step=round(med, 3), images_per_s=round(B * 1e3 / med, 2), ms_min_max=[round(min(ms), 3), round(max(ms), 3)],
                steps_timed=len(ms))


def kernels(B, H, iters):
    import torch
    from ctrlora_amd import hip
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    eps, noise = (torch.randn(B, 4, H, H, generator=g).to(dev) for _ in range(2))
    t = torch.randint(0, 1000, (B,), generator=g).to(dev)
    out3, scratch, per = torch.empty(3, device=dev), torch.empty(16 * B, device=dev), torch.empty(B, device=dev)
    acc = hip.zero_(torch.empty(11, 3, dtype=torch.float64, device=dev))
    nv = torch.full((1,), B, dtype=torch.int32, device=dev)
    legs = dict(p_losses_mse_pair=lambda: hip.p_losses_mse(eps, noise, None, t, None, out3, scratch, per_sample=per),
                loss_bands=lambda: hip.loss_bands(per, t, 1000, 10, acc),
                loss_bands_n_valid=lambda: hip.loss_bands(per, t, 1000, 10, acc, n_valid=nv))
    for _ in range(5):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(iters):
        for k, fn in legs.items():
            ms[k] += _timed(fn, 1)
    return dict(samples_per_launch=B, bands=10, elements_per_sample=4 * H * H, **{k: _leg_us(v) for k, v in ms.items()})


def steps(models, opts, B, H, rounds, warmup):
    """(b) and (c): four legs alternating step by step -- eval eager, eval replayed, train replayed without / with the bands."""
    import torch
    import bench
    from ctrlora_amd.train import GraphedTrainStep, LossBands
    from ctrlora_amd.validation import GraphedEvalStep
    dev = torch.device("cuda", 0)
    m_off, m_on = models["off"], models["on"]
    data = bench.synth(B, H, m_off.control_model.context_dim, dev, 1234, 4)
    five = lambda k: (data["z"][k], data["ctx"][k], data["hint"][k], data["t"][k], data["noise"][k])
    m_on.train_loss_bands = LossBands(m_on.num_timesteps, 10, dev)
    train = {name: GraphedTrainStep(models[name], opts[name], *five(0)) for name in ("off", "on")}
    ev = GraphedEvalStep(m_off, 10)
    ev(*five(0))
    ev(*five(1))                      # eager, then the capture and its first replay
    acc = torch.zeros(11, 3, dtype=torch.float64, device=dev)

    def eval_eager(k):
        z, ctx, hint, t, noise = five(k)
        m_off.engine_eval_step(z, {"c_crossattn": [ctx], "c_concat": [hint]}, t, noise, acc)

    legs = dict(eval_eager=eval_eager, eval_replayed=lambda k: ev(*five(k)), train_off=lambda k: train["off"](*five(k)),
                train_bands_on=lambda k: train["on"](*five(k)))
    ms = {k: [] for k in legs}
    for i in range(warmup + rounds):
        for name, fn in legs.items():
            ms[name] += _timed(lambda: fn(i % 4), 1)
    out = {k: _leg_ms(v[warmup:], B) for k, v in ms.items()}
    assert ev.captures == 1 and ev.replays >= rounds
    tab = m_on.train_loss_bands.read_and_clear()
    assert float(tab[-1, 0]) == B * (warmup + rounds + train["on"].warmup_steps), "one cl_loss_bands launch per step of the on leg"
    m_on.train_loss_bands = None
    out["eval_replayed_over_eval_eager"] = round(out["eval_replayed"]["ms_per_step"] / out["eval_eager"]["ms_per_step"], 4)
    out["eval_replayed_over_train_replayed"] = round(out["eval_replayed"]["ms_per_step"] / out["train_off"]["ms_per_step"], 4)
    out["bands_on_minus_off_ms"] = round(out["train_bands_on"]["ms_per_step"] - out["train_off"]["ms_per_step"], 3)
    lo, hi = out["train_off"]["ms_min_max"]
    out["bands_on_median_within_off_min_max"] = bool(lo <= out["train_bands_on"]["ms_per_step"] <= hi)
    return out


def validation_run(tiny, B, H, samples):
    """(d): a graph_step fit with an EMA, then Trainer._validate timed with val_ema off and on."""
    import torch
    import bench
    from ctrlora_amd.trainer import Trainer
    dev = torch.device("cuda", 0)
    m = bench.build_model("ctrlora_finetune_sd15_rank128.yaml", 0, tiny=tiny, mutate=lambda p: p.update(use_ema=True, ema_decay=0.99))
    m.learning_rate = 1e-5
    m.get_input = lambda batch, k, *a, **kw: (batch["z"], {"c_crossattn": [batch["ctx"]], "c_concat": [batch["hint_z"]]})
    n = max(1, samples // B)
    d = bench.synth(B, H, m.control_model.context_dim, dev, 77, n)
    val = [dict(z=d["z"][k], ctx=d["ctx"][k], hint_z=d["hint"][k]) for k in range(n)]
    tr = Trainer(max_steps=4, precision=16, default_root_dir=tempfile.mkdtemp(prefix="bench_val_"), log_every_n_steps=1000,
                 graph_step=True, val_check_interval=2, val_ema=True)
    tr.fit(m, val[:4], val_dataloaders=val)
    out = dict(samples=n * B, batches=n, bands=10, runs_in_fit=len(tr.logged_val), eval_graph_replays=tr._val_step.replays)
    for name, flag in (("live_only", False), ("with_val_ema", True)):
        tr.val_ema = flag
        ts = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr._validate(m)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        out[name] = dict(wall_s=round(statistics.median(ts), 4), wall_s_min_max=[round(min(ts), 4), round(max(ts), 4)],
                         ms_per_batch=round(statistics.median(ts) * 1e3 / (n * (2 if flag else 1)), 3))
    out["val_loss_simple"] = tr.logged_val[-1][1]["val/loss_simple"]
    return out


def main(argv=None):
    import torch
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50, help="timed launches per kernel")
    ap.add_argument("--rounds", type=int, default=12, help="timed steps per leg")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--samples", type=int, default=256, help="validation samples of (d)")
    ap.add_argument("--tiny", action="store_true", help="narrow model, 16 x 16 latents (rehearsal of the path, not a result)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "val", "bench_val.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_val needs a GPU: a CPU run measures nothing about the engine")
    dev = torch.device("cuda", 0)
    H = 16 if args.tiny else 64
    models, opts = {}, {}
    for name in ("off", "on"):
        m = bench.build_model("ctrlora_finetune_sd15_rank128.yaml", 0, tiny=args.tiny).to(dev).train()
        m.set_engine_dtype(torch.bfloat16)
        m.learning_rate = 1e-5
        models[name], opts[name] = m, bench.configure_optimizers(m)
    res = dict(metric="validation by timestep band: cl_loss_bands next to the p_losses pair, the forward-only step eager / replayed / "
                      "against the replayed training step, the training step with and without loss_bands, one validation run; one MI355X",
               rank=128, dtype="bfloat16", batch=args.batch, latent=f"{H}x{H}", tiny=bool(args.tiny),
               kernels=kernels(args.batch, H, args.iters),
               step=steps(models, opts, args.batch, H, args.rounds, args.warmup))
    del models, opts
    torch.cuda.empty_cache()
    res["validation_run"] = validation_run(args.tiny, args.batch, H, args.samples)
    res["method"] = ("kernels: hot launches between HIP events, alternating, medians with min and max; steps: the four legs alternating "
                     "step by step in one process, HIP events around each, medians with min and max; validation run: host clock "
                     "around Trainer._validate ending in a device synchronise, median of 3")
    res["not_measured"] = ("the parent commit's bench.py step in the same process (the train_off leg launches the same kernels); the "
                           "first stage and the text encoder of a validation batch; more than one GPU")
    if not args.tiny:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
