"""What the per-timestep loss weights and the Huber loss cost, on one MI355X.

    python tools/bench_loss.py [--iters 50] [--rounds 12] [--warmup 4] [--batch 8] [--tiny] [--out FILE]

Workload: bench.py's model (configs/ctrlora_finetune_sd15_rank128.yaml, random weights, bf16 engine mode), B = 8, 64 x 64 latents.

  (a) kernels: cl_p_losses_w with a Min-SNR table (gamma 5) and the Huber loss next to cl_p_losses_mse, on the model's own
      [B, 4, 64, 64] eps against the noise, d_eps written, hot, isolated, each call (both of its launches) between HIP events,
      alternating in one run; medians of --iters.
  (b) the replayed step (ctrlora_amd.train.GraphedTrainStep, one graph) of two twin models, one plain (it launches cl_p_losses_mse,
      what the step launched before the feature existed), one with min_snr_gamma = 5 and loss_type "huber" (cl_p_losses_w): the
      legs alternate step by step in one process, each step between HIP events; medians of --rounds after --warmup.  The
      comparator is the off leg of this run: `on_inside_off_spread` says whether the on leg's median lies within the off leg's own
      smallest and largest sample.

Writes profiles/loss_weight/bench_loss.json (or --out; a --tiny rehearsal writes only where --out says) and prints it as ONE JSON
line.  No GPU, no number: the tool fails."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OBJECTIVE = dict(min_snr_gamma=5.0, loss_type="huber", huber_delta=1.0)


def _timed(fn, iters):
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def kernels(model_on, data, iters):
    import torch
    from ctrlora_amd import hip
    m = model_on
    z, ctx, hint, t, noise = (data[k][0] for k in ("z", "ctx", "hint", "t", "noise"))
    with torch.no_grad():
        eps = m.apply_model(m.q_sample(z, t, noise), t, {"c_crossattn": [ctx], "c_concat": [hint]}).float().contiguous()
    target, t = noise.float().contiguous(), t.long().contiguous()
    B = eps.shape[0]
    out = torch.empty(3, device=eps.device)
    scratch = torch.empty(16 * B, device=eps.device)
    d_eps = torch.empty_like(eps)
    mse = lambda: hip.p_losses_mse(eps, target, d_eps, t, m.lvlb_weights, out, scratch, 1.0, 1.0, 0.0)
    wtd = lambda: hip.p_losses_w(eps, target, d_eps, t, m.lvlb_weights, out, scratch, 1.0, 1.0, 0.0, wt=m.loss_weights, kind=1,
                                 delta=m.huber_delta)
    for _ in range(5):
        mse(); wtd()
    torch.cuda.synchronize()
    ts = dict(mse=[], w=[])
    for _ in range(iters):                                            # alternating, one sample each per round
        ts["mse"] += _timed(mse, 1)
        ts["w"] += _timed(wtd, 1)
    med = {k: statistics.median(v) for k, v in ts.items()}
    d = (eps - target).abs()
    n = eps.numel()
    return dict(shape=list(eps.shape), elements=n, bytes_moved=12 * n,
                p_losses_mse_us=round(med["mse"] * 1e3, 2), p_losses_w_us=round(med["w"] * 1e3, 2),
                p_losses_mse_us_min_max=[round(min(ts["mse"]) * 1e3, 2), round(max(ts["mse"]) * 1e3, 2)],
                p_losses_w_us_min_max=[round(min(ts["w"]) * 1e3, 2), round(max(ts["w"]) * 1e3, 2)],
                w_minus_mse_us=round((med["w"] - med["mse"]) * 1e3, 2), huber_inner_share=round(float((d <= m.huber_delta).float().mean()), 4),
                iters=iters)


def steps(models, opts, datas, rounds, warmup):
    from ctrlora_amd.train import GraphedTrainStep
    legs = {}
    for name in ("off", "on"):
        m, opt, data = models[name], opts[name], datas[name]
        gs = GraphedTrainStep(m, opt, data["z"][0], data["ctx"][0], data["hint"][0], data["t"][0], data["noise"][0])
        legs[name] = (gs, data, [])
    for i in range(warmup + rounds):
        for name in ("off", "on"):
            gs, data, ms = legs[name]
            k = i % 4
            ms += _timed(lambda: gs(data["z"][k], data["ctx"][k], data["hint"][k], data["t"][k], data["noise"][k]), 1)
    out = {}
    B = datas["off"]["z"][0].shape[0]
    for name, (gs, _, ms) in legs.items():
        ms = ms[warmup:]
        med = statistics.median(ms)
        out[name] = dict(ms_per_step=round(med, 3), images_per_s=round(B * 1e3 / med, 2), ms_min_max=[round(min(ms), 3), round(max(ms), 3)],
                         steps_timed=len(ms), loss=round(float(gs.loss), 5))
    lo, hi = out["off"]["ms_min_max"]
    out["on_minus_off_ms"] = round(out["on"]["ms_per_step"] - out["off"]["ms_per_step"], 3)
    out["on_inside_off_spread"] = bool(lo <= out["on"]["ms_per_step"] <= hi)
    return out


def main(argv=None):
    import torch
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50, help="timed calls per kernel")
    ap.add_argument("--rounds", type=int, default=12, help="timed replayed steps per leg")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--tiny", action="store_true", help="narrow model, 16 x 16 latents (rehearsal of the path, not a result)")
    ap.add_argument("--out", default=None, help="default: profiles/loss_weight/bench_loss.json; with --tiny nothing is written")
    args = ap.parse_args(argv)
    if args.out is None and not args.tiny:
        args.out = os.path.join(ROOT, "profiles", "loss_weight", "bench_loss.json")
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss needs a GPU: a CPU run measures nothing about the engine")
    dev = torch.device("cuda", 0)
    H = 16 if args.tiny else 64
    models, opts, datas = {}, {}, {}
    for name in ("off", "on"):
        mutate = (lambda p: p.update(OBJECTIVE)) if name == "on" else None
        m = bench.build_model("ctrlora_finetune_sd15_rank128.yaml", 0, tiny=args.tiny, mutate=mutate).to(dev).train()
        m.set_engine_dtype(torch.bfloat16)
        m.learning_rate = 1e-5
        models[name], opts[name] = m, bench.configure_optimizers(m)
        datas[name] = bench.synth(args.batch, H, m.control_model.context_dim, dev, 1234, 4)
    assert models["off"].loss_weights is None and models["on"].loss_weights is not None
    res = dict(metric="per-timestep loss weights (Min-SNR, gamma 5) + Huber loss on the device: isolated kernel times and the replayed "
                      "optimizer step with both off / on, one MI355X",
               rank=128, dtype="bfloat16", batch=args.batch, latent=f"{H}x{H}", tiny=bool(args.tiny), objective=OBJECTIVE,
               kernels=kernels(models["on"], datas["on"], args.iters),
               step=steps(models, opts, datas, args.rounds, args.warmup),
               method="kernels: hot calls between HIP events, the two entry points alternating, medians; step: GraphedTrainStep replays "
                      "of two twin models alternating step by step in one process, HIP events around each replay, medians")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
