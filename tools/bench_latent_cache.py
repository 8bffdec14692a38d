"""What `--latent_cache` saves per optimizer step, measured: `get_input` + `training_step` + backward + AdamW from image batches
(two VAE encodes of B 512 x 512 images per step) against the same step from cached posteriors, on one MI355X.

    python tools/bench_latent_cache.py [--rounds 12] [--warmup 3] [--bs 8] [--tiny]

Workload: bench.py's model (configs/ctrlora_finetune_sd15_rank128.yaml, random weights, bf16 engine mode) with an SD-shaped
AutoencoderKL as first stage, B = 8, rank 128, synthetic images; the text context is a given tensor (the text encoder is about
1 % of the step and the same in both legs).  Method: the two legs alternate, step by step, inside one process (live, cached,
live, cached, ...), every step between a device synchronise and the next, host clock; the medians of `--rounds` steps per leg
after `--warmup` rounds.  The cached leg's batches hold the posteriors of exactly the live leg's images.  Prints ONE JSON line.
No GPU, no number: the tool fails.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    import torch
    import bench
    from ldm.models.autoencoder import AutoencoderKL
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bs", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--tiny", action="store_true", help="narrow model and VAE, 128 x 128 images (rehearsal of the path, not a result)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_latent_cache needs a GPU: a CPU run measures nothing about the engine")
    dev, dtype, B = torch.device("cuda", 0), torch.bfloat16, args.bs
    size = 128 if args.tiny else args.size
    model = bench.build_model("ctrlora_finetune_sd15_rank128.yaml", 0, tiny=args.tiny)
    dd = dict(attn_resolutions=[], ch=64 if args.tiny else 128, ch_mult=[1, 2, 4, 4], double_z=True, dropout=0.0, in_channels=3,
              num_res_blocks=2, out_ch=3, resolution=256, z_channels=4)
    torch.manual_seed(0)
    model.first_stage_model = AutoencoderKL(ddconfig=dd, lossconfig=dict(target="torch.nn.Identity"), embed_dim=4).eval()
    model.scale_factor = 0.18215
    model = model.to(dev).train()
    model.set_engine_dtype(dtype)
    model.learning_rate = 1e-5
    opt = bench.configure_optimizers(model)
    g = torch.Generator().manual_seed(1)
    nb = 2
    ctx = [torch.randn(B, 77, model.control_model.context_dim, generator=g).to(dev) for _ in range(nb)]
    live = [dict(jpg=torch.rand(B, size, size, 3, generator=g) * 2 - 1, hint=torch.rand(B, size, size, 3, generator=g), txt=ctx[i])
            for i in range(nb)]
    cached = []
    with torch.no_grad():
        for b in live:
            mom = []
            for k in ("jpg", "hint"):
                post = model.encode_first_stage(b[k].to(dev).permute(0, 3, 1, 2).contiguous().float())
                mom.append(torch.cat([post.mean, post.std], 1).float().cpu())
            cached.append(dict(jpg_moments=mom[0], hint_moments=mom[1], txt=b["txt"]))
    assert "_enc" in model.first_stage_model.__dict__, "the first stage did not run on the engine's VAE encoder"

    def step(batch):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.zero_grad()
        loss = model.training_step(batch, 0)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, loss

    times = {"live": [], "cached": []}
    for r in range(args.warmup + args.rounds):
        for leg, batches in (("live", live), ("cached", cached)):
            dt, loss = step(batches[r % nb])
            assert torch.isfinite(loss), (leg, r)
            if r >= args.warmup:
                times[leg].append(dt)
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps(dict(
        metric="fine-tuning images/s from image batches (live VAE encodes) and from cached posteriors (--latent_cache)",
        live_images_per_s=round(B / med["live"], 2), cached_images_per_s=round(B / med["cached"], 2),
        speedup=round(med["live"] / med["cached"], 3), live_ms_per_step=round(med["live"] * 1e3, 2),
        cached_ms_per_step=round(med["cached"] * 1e3, 2),
        live_ms_min_max=[round(min(times["live"]) * 1e3, 2), round(max(times["live"]) * 1e3, 2)],
        cached_ms_min_max=[round(min(times["cached"]) * 1e3, 2), round(max(times["cached"]) * 1e3, 2)],
        batch=B, image=f"{size}x{size}", rank=128, dtype="bfloat16", rounds=args.rounds, warmup=args.warmup, tiny=bool(args.tiny),
        step="get_input + training_step + backward + fused AdamW, eager launches, one synchronise per step",
        method="legs alternate step by step in one process; medians", loss=round(float(loss.detach()), 5))))


if __name__ == "__main__":
    main()
