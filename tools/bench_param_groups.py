"""What parameter groups and the device learning-rate schedule cost, on one MI355X.

    python tools/bench_param_groups.py [--iters 50] [--rounds 12] [--warmup 4] [--batch 8] [--tiny]

Workload: bench.py's model (configs/ctrlora_finetune_sd15_rank128.yaml, random weights, bf16 engine mode), B = 8, 64 x 64 latents.

  (a) kernels: cl_adamw_dev_groups against cl_adamw_dev over the model's real flat master buffer (copies of it), with G = 4 and the
      chunk -> group map that --lora_plus_ratio + --no_decay_norm_bias produce on this model (three groups in use, one row spare),
      and with G = 1; hot, isolated, each between HIP events, the three launches alternating in one run; medians of --iters and
      each leg's min and max.  The grouped launch moves the same 28 bytes per element plus 1 / 64 byte of map.
      Criterion: the grouped median lies within cl_adamw_dev's own min .. max over its --iters samples of the same run.
  (b) the cl_lr_schedule launch on its own, the same way.
  (c) the replayed step (ctrlora_amd.train.GraphedTrainStep, one graph) with both features off against both on (groups as in (a),
      a cosine schedule with warm-up as a device table): two twin models, the legs alternating step by step in one process, each
      step between HIP events; medians of --rounds after --warmup.  The "off" leg launches what the optimizer launched before the
      features existed.  Criterion: the on leg's median lies within the off leg's own min .. max over its --rounds samples.

Writes profiles/param_groups/bench_param_groups.json and prints it as ONE JSON line; the two criteria are recorded as booleans
next to the numbers, whatever they come out as.  What LoRA+ or a warm-up does to sample quality is not measured here.  No GPU, no
number: the tool fails."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RULES = [{"name": "lora_up", "match": ["lora_layer.up."], "lr_scale": 16.0},
         {"name": "no_decay", "match": ["norm", ".bias"], "weight_decay": 0.0}]


def _timed(fn, iters):
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def _leg(ms, nbytes=None):
    med = statistics.median(ms)
    out = dict(us=round(med * 1e3, 2), us_min_max=[round(min(ms) * 1e3, 2), round(max(ms) * 1e3, 2)], samples=len(ms))
    if nbytes is not None:
        out["tb_s"] = round(nbytes / (med * 1e-3) / 1e12, 3)
    return out


def kernels(opt_on, iters):
    import torch
    from ctrlora_amd import hip
    (ex,), (st,) = opt_on.executors, opt_on._states
    g = ex.tr.flat_grad
    n = g.numel()
    g.normal_(0.0, 1e-3)
    p, m, v = ex.tr.flat.clone(), st.m.clone(), st.v.clone()          # copies: the model is used again afterwards
    step = torch.ones(1, dtype=torch.int32, device=g.device)
    cg3 = opt_on._chunk_group[0]
    table4 = torch.cat([opt_on._hyper_table, opt_on._hyper_table[:1]]).contiguous()        # G = 4: the three groups in use + a spare row
    table1 = opt_on._hyper_table[:1].contiguous()
    cg1 = torch.zeros_like(cg3)
    lr_table = torch.full((1000, 4), 1e-5, dtype=torch.float32, device=g.device)
    sched_table = table4.clone()
    legs = dict(adamw_dev=lambda: hip.adamw_dev(p, g, m, v, table1[0], step),
                groups_g4=lambda: hip.adamw_dev_groups(p, g, m, v, table4, cg3, step),
                groups_g1=lambda: hip.adamw_dev_groups(p, g, m, v, table1, cg1, step),
                lr_schedule=lambda: hip.lr_schedule(sched_table, lr_table, step))
    for _ in range(5):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in legs}
    for _ in range(iters):                                            # alternating, one sample each per round
        for k, fn in legs.items():
            t[k] += _timed(fn, 1)
    nbytes = 28 * n
    out = dict(elements=n, buffer_mb=round(4 * n / 1e6, 2), chunks=int(cg3.numel()),
               chunks_per_group=[int((cg3 == k).sum()) for k in range(3)], group_changes=int((cg3[1:] != cg3[:-1]).sum()),
               adamw_dev=_leg(t["adamw_dev"], nbytes), adamw_dev_groups_g4=_leg(t["groups_g4"], nbytes + n // 64),
               adamw_dev_groups_g1=_leg(t["groups_g1"], nbytes + n // 64), lr_schedule=_leg(t["lr_schedule"]), iters=iters)
    lo, hi = out["adamw_dev"]["us_min_max"]
    for k in ("adamw_dev_groups_g4", "adamw_dev_groups_g1"):
        out[k]["over_adamw_dev"] = round(out[k]["us"] / out["adamw_dev"]["us"], 4)
        out[k]["median_within_adamw_dev_min_max"] = bool(lo <= out[k]["us"] <= hi)
    return out


def steps(models, opts, scheds, B, H, rounds, warmup):
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
            if scheds[name] is not None:
                scheds[name].step()               # the host mirror, as the Trainer keeps it: outside the timed region
    out = {}
    for name, (gs, _, ms) in legs.items():
        ms = ms[warmup:]
        med = statistics.median(ms)
        out[name] = dict(ms_per_step=round(med, 3), images_per_s=round(B * 1e3 / med, 2), ms_min_max=[round(min(ms), 3), round(max(ms), 3)],
                         steps_timed=len(ms), loss=round(float(gs.loss), 5))
    on = opts["on"]
    assert on._chunk_group is not None and on._lr_table is not None and opts["off"]._chunk_group is None and opts["off"]._lr_table is None
    done = int(on._step)
    want = on._lr_table[min(done - 1, on._lr_table.shape[0] - 1)]
    assert torch.equal(on.last_lr(), want), "the replayed step did not follow the table"
    out["on"].update(groups=on.group_names, optimizer_steps=done, last_lr=[float(x) for x in on.last_lr().cpu()])
    out["on_minus_off_ms"] = round(out["on"]["ms_per_step"] - out["off"]["ms_per_step"], 3)
    lo, hi = out["off"]["ms_min_max"]
    out["on_median_within_off_min_max"] = bool(lo <= out["on"]["ms_per_step"] <= hi)
    return out


def main(argv=None):
    import torch
    import bench
    from ctrlora_amd.lr_schedule import compile_lambda_lr
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50, help="timed launches per kernel")
    ap.add_argument("--rounds", type=int, default=12, help="timed replayed steps per leg")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--tiny", action="store_true", help="narrow model, 16 x 16 latents (rehearsal of the path, not a result)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "param_groups", "bench_param_groups.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_param_groups needs a GPU: a CPU run measures nothing about the engine")
    dev = torch.device("cuda", 0)
    total = 1000
    sched_cfg = {"target": "ctrlora_amd.lr_schedule.WarmupDecay",
                 "params": dict(kind="cosine", warmup_steps=100, total_steps=total, min_ratio=0.1)}
    models, opts, scheds = {}, {}, {}
    for name in ("off", "on"):
        mutate = (lambda p: p.update(optim_groups=RULES, scheduler_config=sched_cfg)) if name == "on" else None
        m = bench.build_model("ctrlora_finetune_sd15_rank128.yaml", 0, tiny=args.tiny, mutate=mutate).to(dev).train()
        m.set_engine_dtype(torch.bfloat16)
        m.learning_rate = 1e-5
        ret = bench.configure_optimizers(m)
        if name == "on":
            (opt,), (entry,) = ret
            opt.set_lr_schedule(compile_lambda_lr(entry["scheduler"], total))
            scheds[name] = entry["scheduler"]
        else:
            opt, scheds[name] = ret, None
        models[name], opts[name] = m, opt
    res = dict(metric="parameter groups and a device learning-rate schedule in the fused AdamW: isolated kernel times and the replayed "
                      "optimizer step with both off / both on, one MI355X",
               rank=128, dtype="bfloat16", batch=args.batch, latent="16x16" if args.tiny else "64x64", tiny=bool(args.tiny),
               rules=RULES, schedule=sched_cfg["params"], kernels=kernels(opts["on"], args.iters),
               step=steps(models, opts, scheds, args.batch, 16 if args.tiny else 64, args.rounds, args.warmup),
               method="kernels: hot launches between HIP events, the launches alternating, medians with each leg's min and max; step: "
                      "GraphedTrainStep replays of two twin models alternating step by step in one process, HIP events around each "
                      "replay, medians with each leg's min and max",
               not_measured="what LoRA+ or a warm-up does to sample quality")
    if not args.tiny:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
