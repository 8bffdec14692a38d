"""Encode a paired-image dataset once, for `scripts/train_ctrlora_finetune.py --latent_cache DIR`.

    python scripts/tool_cache_latents.py --dataroot ./data/my_condition --config ./configs/ctrlora_finetune_sd15_rank128.yaml \\
        --sd_ckpt ./ckpts/sd15/v1-5-pruned.ckpt --out ./data/my_condition/latents [--bs 16] [--precision 32]

Walks `CustomDataset(dataroot, drop_rate=0)` in index order, runs the model's first stage (the engine's VAE encoder, on the
GPU) on every target and condition image and stores the POSTERIORS, mean and std, not a sample: training then draws a fresh
sample per step, as the live path does.  Format and checks: ctrlora_amd/latent_cache.py.  `--precision` is the engine mode
the encoder runs in and must be the one training will use (train_ctrlora_finetune.py's default is 32).  Images of differing
sizes are refused; MultiGen20M and pre-training (random crops) have no cache.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def get_parser():
    p = argparse.ArgumentParser(description="cache the first-stage posteriors of a CustomDataset")
    p.add_argument("--dataroot", type=str, required=True, help="path to dataset (prompt.json, source/, target/)")
    p.add_argument("--config", type=str, required=True, help="path to model config file")
    p.add_argument("--sd_ckpt", type=str, required=True, help="path to pretrained stable diffusion checkpoint (carries the VAE)")
    p.add_argument("--out", type=str, required=True, help="directory of the cache")
    p.add_argument("--bs", type=int, default=16, help="images per encoder call")
    p.add_argument("--precision", type=int, default=32, help="engine mode of the encoder: 32, or 16 for bf16 (as when training)")
    return p


def main(argv=None):
    import torch
    from cldm.model import create_model, load_state_dict
    from ctrlora_amd import latent_cache
    from datasets.custom_dataset import CustomDataset
    args = get_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("tool_cache_latents runs the engine's VAE encoder and needs a GPU")
    dataset = CustomDataset(args.dataroot, drop_rate=0)
    model = create_model(args.config).cpu()
    sd = load_state_dict(args.sd_ckpt, location="cpu")
    own = model.state_dict()
    first = {k: v for k, v in sd.items() if k.startswith("first_stage_model.") and k in own}
    if not first:
        raise KeyError(f"{args.sd_ckpt} carries no first_stage_model weights")
    model.load_state_dict(first, strict=False)
    dtype = torch.float32 if str(args.precision) in ("32", "32-true") else torch.bfloat16
    fingerprint = latent_cache.state_fingerprint(model.first_stage_model)
    model = model.cuda().eval()
    model.set_engine_dtype(dtype)
    meta = latent_cache.build_cache(dataset, model.encode_first_stage, args.out, bs=args.bs, device=model.device,
                                    engine_dtype=latent_cache.dtype_name(dtype), fingerprint=fingerprint)
    print(f"Cached {meta['N']} posterior pairs of shape {meta['latent_shape']} ({meta['engine_dtype']}) in {args.out}")
    return meta


if __name__ == "__main__":
    main()
