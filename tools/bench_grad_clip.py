"""What device-side gradient clipping costs, on one MI355X.

    python tools/bench_grad_clip.py [--iters 50] [--rounds 12] [--warmup 4] [--batch 8] [--tiny]

Workload: bench.py's model (configs/ctrlora_finetune_sd15_rank128.yaml, random weights, bf16 engine mode), B = 8, 64 x 64 latents.

  (a) kernels: cl_grad_norm (both launches) over the model's real flat gradient buffer next to cl_adamw_dev over the same buffer,
      hot, isolated, each between HIP events, alternating in one run; medians of --iters.  The criterion: the norm's two launches
      take no longer than the AdamW launch they precede.  Achieved bytes / s from the algorithm's bytes: 4 n for the norm, 28 n
      for AdamW (p, m, v read and written, g read).
  (b) the replayed step (ctrlora_amd.train.GraphedTrainStep, one graph) with clipping off and on: two twin models, the legs
      alternating step by step in one process, each step between HIP events; medians of --rounds after --warmup.  The "off" leg
      launches what the optimizer launched before the feature existed.

Writes profiles/grad_clip/bench_grad_clip.json and prints it as ONE JSON line.  No GPU, no number: the tool fails."""
import argparse
import json
import os
import statistics
import sys

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


def kernels(model, opt, iters):
    import torch
    from ctrlora_amd import hip
    (ex,), (st,) = opt.executors, opt._states
    g = ex.tr.flat_grad
    n = g.numel()
    g.normal_(0.0, 1e-3)
    p, m, v = ex.tr.flat.clone(), st.m.clone(), st.v.clone()          # copies: the model is used again afterwards
    step = torch.ones(1, dtype=torch.int32, device=g.device)
    out = torch.zeros(2, device=g.device)
    mx = torch.ones(1, device=g.device)
    scratch = torch.empty(hip.grad_norm_scratch_floats(1), device=g.device)
    norm = lambda: hip.grad_norm([g], opt._hyper, mx, out, scratch)
    adam = lambda: hip.adamw_dev(p, g, m, v, opt._hyper, step)
    clip = lambda: hip.adamw_dev_clip(p, g, m, v, opt._hyper, step, out)
    for _ in range(5):
        norm(); adam(); clip()
    torch.cuda.synchronize()
    t = dict(norm=[], adamw=[], adamw_clip=[])
    for _ in range(iters):                                            # alternating, one sample each per round
        t["norm"] += _timed(norm, 1)
        t["adamw"] += _timed(adam, 1)
        t["adamw_clip"] += _timed(clip, 1)
    med = {k: statistics.median(x) for k, x in t.items()}
    want = float(g.double().norm())
    assert abs(float(out[0]) - want) <= 1e-6 * want, (float(out[0]), want)
    return dict(elements=n, buffer_mb=round(4 * n / 1e6, 2),
                grad_norm_us=round(med["norm"] * 1e3, 2), adamw_dev_us=round(med["adamw"] * 1e3, 2),
                adamw_dev_clip_us=round(med["adamw_clip"] * 1e3, 2),
                grad_norm_tb_s=round(4 * n / (med["norm"] * 1e-3) / 1e12, 3), adamw_dev_tb_s=round(28 * n / (med["adamw"] * 1e-3) / 1e12, 3),
                norm_over_adamw=round(med["norm"] / med["adamw"], 3), criterion_met=bool(med["norm"] <= med["adamw"]), iters=iters)


def steps(models, opts, B, H, rounds, warmup):
    import torch
    import bench
    from ctrlora_amd.train import GraphedTrainStep
    dev = torch.device("cuda", 0)
    legs = {}
    for name in ("off", "on"):
        m, opt = models[name], opts[name]
        data = bench.synth(B, H, m.control_model.context_dim, dev, 1234, 4)
        if name == "on":
            opt.max_grad_norm = 1.0
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
    norm, coef = (float(v) for v in opts["on"].last_grad_norm())
    out["on"].update(last_grad_norm=round(norm, 5), last_coef=round(coef, 5))
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_clip", "bench_grad_clip.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_grad_clip needs a GPU: a CPU run measures nothing about the engine")
    dev = torch.device("cuda", 0)
    models, opts = {}, {}
    for name in ("off", "on"):
        m = bench.build_model("ctrlora_finetune_sd15_rank128.yaml", 0, tiny=args.tiny).to(dev).train()
        m.set_engine_dtype(torch.bfloat16)
        m.learning_rate = 1e-5
        models[name], opts[name] = m, bench.configure_optimizers(m)
    res = dict(metric="gradient norm + clip on the device: isolated kernel times and the replayed optimizer step with clipping off / on, one MI355X",
               rank=128, dtype="bfloat16", batch=args.batch, latent="16x16" if args.tiny else "64x64", tiny=bool(args.tiny),
               kernels=kernels(models["off"], opts["off"], args.iters),
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
