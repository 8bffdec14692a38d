"""What the device-side EMA of the trained weights costs, on one MI355X.

    python tools/bench_ema.py [--iters 50] [--rounds 12] [--warmup 4] [--batch 8] [--tiny]

Workload: bench.py's model (configs/ctrlora_finetune_sd15_rank128.yaml, random weights, bf16 engine mode), B = 8, 64 x 64 latents.

  (a) kernels: cl_ema_update over the model's real flat master buffer next to the cl_adamw_dev launch it follows, and cl_swap over
      the same pair of buffers (ema_scope's exchange), hot, isolated, each between HIP events, alternating in one run; medians of
      --iters.  Achieved bytes / s from the algorithm's bytes: 12 n for the EMA (shadow read and written, p read), 28 n for AdamW
      (p, m, v read and written, g read), 16 n for the swap.  By bytes the EMA launch is 12 / 28 = 0.43 of the AdamW launch.
  (b) the replayed step (ctrlora_amd.train.GraphedTrainStep, one graph) with the EMA off and on: two twin models, the legs
      alternating step by step in one process, each step between HIP events; medians of --rounds after --warmup.  The "off" leg
      launches what the optimizer launched before the feature existed.

Writes profiles/ema/bench_ema.json and prints it as ONE JSON line.  There is no pass / fail number.  No GPU, no number: the tool
fails."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EMA_DECAY = 0.9999


def _timed(fn, iters):
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def kernels(opt, iters):
    import torch
    from ctrlora_amd import hip
    (ex,), (st,) = opt.executors, opt._states
    g = ex.tr.flat_grad
    n = g.numel()
    g.normal_(0.0, 1e-3)
    p, m, v = ex.tr.flat.clone(), st.m.clone(), st.v.clone()          # copies: the model is used again afterwards
    shadow = p.clone()
    step = torch.ones(1, dtype=torch.int32, device=g.device)
    decay = torch.tensor(EMA_DECAY, dtype=torch.float32, device=g.device)
    count = torch.tensor(1000, dtype=torch.int32, device=g.device)
    adam = lambda: hip.adamw_dev(p, g, m, v, opt._hyper, step)
    ema = lambda: hip.ema_update(shadow, p, decay, count)
    swap = lambda: hip.swap_(shadow, p)
    for _ in range(5):
        adam(); ema(); swap(); swap()
    torch.cuda.synchronize()
    t = dict(adamw=[], ema=[], swap=[])
    for _ in range(iters):                                            # alternating, one sample each per round
        t["adamw"] += _timed(adam, 1)
        t["ema"] += _timed(ema, 1)
        t["swap"] += _timed(swap, 1)
    if iters % 2:
        swap()
    med = {k: statistics.median(x) for k, x in t.items()}
    tb_s = lambda nbytes, ms: round(nbytes * n / (ms * 1e-3) / 1e12, 3)
    return dict(elements=n, buffer_mb=round(4 * n / 1e6, 2), adamw_dev_us=round(med["adamw"] * 1e3, 2),
                ema_update_us=round(med["ema"] * 1e3, 2), swap_us=round(med["swap"] * 1e3, 2),
                adamw_dev_tb_s=tb_s(28, med["adamw"]), ema_update_tb_s=tb_s(12, med["ema"]), swap_tb_s=tb_s(16, med["swap"]),
                ema_over_adamw=round(med["ema"] / med["adamw"], 3), ema_over_adamw_by_bytes=round(12 / 28, 3), iters=iters)


def steps(models, opts, B, H, rounds, warmup):
    import torch
    import bench
    from ctrlora_amd.train import GraphedTrainStep
    dev = torch.device("cuda", 0)
    legs = {}
    for name in ("off", "on"):
        m, opt = models[name], opts[name]
        data = bench.synth(B, H, m.control_model.context_dim, dev, 1234, 4)
        gs = GraphedTrainStep(m, opt, data["z"][0], data["ctx"][0], data["hint"][0], data["t"][0], data["noise"][0])
        legs[name] = (gs, data, [])
    for i in range(warmup + rounds):
        for name in ("off", "on"):
            gs, data, ms = legs[name]
            k = i % 4
            ms += _timed(lambda: gs(data["z"][k], data["ctx"][k], data["hint"][k], data["t"][k], data["noise"][k]), 1)
    out = {}
    for name, (gs, _, ms) in legs.items():
        ms = ms[warmup:]
        med = statistics.median(ms)
        out[name] = dict(ms_per_step=round(med, 3), images_per_s=round(B * 1e3 / med, 2), ms_min_max=[round(min(ms), 3), round(max(ms), 3)],
                         steps_timed=len(ms), loss=round(float(gs.loss), 5))
    ema = models["on"].model_ema
    assert opts["on"].ema is ema and opts["off"].ema is None
    out["on"].update(num_updates=int(ema.num_updates), optimizer_steps=int(opts["on"]._step))
    assert out["on"]["num_updates"] == out["on"]["optimizer_steps"]
    out["on_minus_off_ms"] = round(out["on"]["ms_per_step"] - out["off"]["ms_per_step"], 3)
    return out


def main(argv=None):
    import torch
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50, help="timed launches per kernel")
    ap.add_argument("--rounds", type=int, default=12, help="timed replayed steps per leg")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--tiny", action="store_true", help="narrow model, 16 x 16 latents (rehearsal of the path, not a result)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema", "bench_ema.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_ema needs a GPU: a CPU run measures nothing about the engine")
    dev = torch.device("cuda", 0)
    models, opts = {}, {}
    for name in ("off", "on"):
        mutate = (lambda p: p.update(use_ema=True, ema_decay=EMA_DECAY)) if name == "on" else None
        m = bench.build_model("ctrlora_finetune_sd15_rank128.yaml", 0, tiny=args.tiny, mutate=mutate).to(dev).train()
        m.set_engine_dtype(torch.bfloat16)
        m.learning_rate = 1e-5
        models[name], opts[name] = m, bench.configure_optimizers(m)
    res = dict(metric="EMA of the trained weights on the device: isolated kernel times and the replayed optimizer step with the EMA off / on, one MI355X",
               rank=128, dtype="bfloat16", batch=args.batch, latent="16x16" if args.tiny else "64x64", tiny=bool(args.tiny),
               ema_decay=EMA_DECAY, kernels=kernels(opts["off"], args.iters),
               step=steps(models, opts, args.batch, 16 if args.tiny else 64, args.rounds, args.warmup),
               method="kernels: hot launches between HIP events, the three kernels alternating, medians; step: GraphedTrainStep replays of "
                      "two twin models alternating step by step in one process, HIP events around each replay, medians")
    if not args.tiny:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
