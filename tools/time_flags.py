"""ms / optimizer step of LoRA fine-tuning for the four (norm_trainable, zero_trainable) combinations at the benchmark shape
(configs/ctrlora_finetune_sd15_rank128.yaml, batch 8, latent 64x64, bf16, GraphedTrainStep = one hipGraph replay per step),
all from one process so that the rows are comparable:

    python tools/time_flags.py [--steps 30] [--warmup 5] [--batch 8] [--latent 64] [--out profiles/flags/time_flags.json]

Prints one JSON line: per combination the median and minimum ms/step over `steps` replays, the trainable tensor count and
the flat buffer size."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def time_combo(nt, zt, args):
    import bench
    from ctrlora_amd.train import GraphedTrainStep

    def mutate(p):
        p["control_stage_config"]["params"].update(norm_trainable=nt, zero_trainable=zt)

    model = bench.build_model("ctrlora_finetune_sd15_rank128.yaml", 0, mutate=mutate).cuda().train()
    model.set_engine_dtype(torch.bfloat16)
    model.learning_rate = 1e-5
    opt = model.configure_optimizers()
    ex = model.control_model.executor()
    d = bench.synth(args.batch, args.latent, 768, "cuda", 99, 1)
    z, ctx, hint, t, noise = d["z"][0], d["ctx"][0], d["hint"][0], d["t"][0], d["noise"][0]
    g = GraphedTrainStep(model, opt, z, ctx, hint, t, noise, warmup=2)
    for _ in range(args.warmup):
        g(z, ctx, hint, t, noise)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        loss = g(z, ctx, hint, t, noise)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    assert torch.isfinite(loss)
    ms.sort()
    row = dict(norm_trainable=nt, zero_trainable=zt, ms_median=round(ms[len(ms) // 2], 3), ms_min=round(ms[0], 3),
               trainables=len(ex.tr.items), flat_floats=int(ex.tr.numel))
    del g, opt, model
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    rows = [time_combo(nt, zt, args) for nt, zt in ((True, True), (False, True), (True, False), (False, False))]
    res = dict(shape=dict(batch=args.batch, latent=args.latent, dtype="bf16", rank=128, steps=args.steps), rows=rows,
               device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
