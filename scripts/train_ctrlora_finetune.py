"""LoRA fine-tuning on a new condition -- command line of the reference's scripts/train_ctrlora_finetune.py:22-129
(same flags), on the MI355X engine with a Lightning-free loop.

    torchrun --nproc-per-node 8 scripts/train_ctrlora_finetune.py --dataroot ./data/my_condition \\
        --config ./configs/ctrlora_finetune_sd15_rank128.yaml --sd_ckpt ./ckpts/sd15/v1-5-pruned.ckpt \\
        --cn_ckpt ./ckpts/ctrlora-basecn/ctrlora_sd15_basecn700k.ckpt --bs 8 --precision 16 --max_steps 1000

One process per GPU (the reference lets Lightning spawn them: strategy='ddp', devices=-1); `--precision 32` runs the
fp32 parity mode of the engine, 16 / bf16 the bf16-storage mode.
"""
import argparse
import datetime
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TASKS = ["hed", "canny", "seg", "depth", "normal", "openpose", "hedsketch", "bbox", "outpainting", "inpainting", "blur",
         "grayscale"]


def get_parser():
    p = argparse.ArgumentParser(description="args")
    # dataset
    p.add_argument("--dataroot", type=str, required=True, help="path to dataset")
    p.add_argument("--drop_rate", type=float, default=0.3, help="drop rate for classifier-free guidance")
    p.add_argument("--multigen20m", action="store_true", default=False, help="use multigen20m dataset")
    p.add_argument("--task", type=str, choices=TASKS, help="task name")
    p.add_argument("--subset", type=int, default=0, help="train on a subset of the dataset")
    # model
    p.add_argument("--config", type=str, required=True, help="path to model config file")
    p.add_argument("--sd_ckpt", type=str, required=True, help="path to pretrained stable diffusion checkpoint")
    p.add_argument("--cn_ckpt", type=str, required=True, help="path to pretrained controlnet checkpoint")
    # training
    p.add_argument("-n", "--name", type=str, help="experiment name")
    p.add_argument("--lr", type=float, default=1e-5, help="learning rate")
    p.add_argument("--bs", type=int, default=1, help="batchsize per device")
    p.add_argument("--max_steps", type=int, default=100000, help="max training steps")
    p.add_argument("--gradacc", type=int, default=1, help="gradient accumulation")
    p.add_argument("--precision", type=int, default=32, help="precision")
    p.add_argument("--save_memory", action="store_true", default=False, help="accepted for compatibility (no effect: "
                   "the engine's attention never materialises the score matrix)")
    p.add_argument("--img_logger_freq", type=int, default=1000, help="img logger freq")
    p.add_argument("--ckpt_logger_freq", type=int, default=1000, help="ckpt logger freq")
    p.add_argument("--num_workers", type=int, default=None,
                   help="DataLoader worker processes (default: the reference's 16, capped at the host's cores); every epoch "
                        "forks them again, which is slow from a process with a large address space")
    p.add_argument("--latent_cache", type=str, default=None,
                   help="directory written by scripts/tool_cache_latents.py for this dataroot: train from the stored first-stage "
                        "posteriors, so that no step runs the VAE encoder (CustomDataset only; off by default)")
    p.add_argument("--graph", action="store_true", default=False,
                   help="capture the optimizer step (forward, loss, backward, gradient exchange points, AdamW, re-pack) as "
                        "hipGraphs after two eagerly launched steps and replay it for every later batch instead of launching its "
                        "~1900 kernels from Python; the data loading, the first stage and the text encoder stay outside the "
                        "capture (GPU only; works with --latent_cache, --gradacc and torchrun; off by default)")
    p.add_argument("--grad_clip", type=float, default=0.0,
                   help="clip the global L2 norm of the gradients to this value before every optimizer step, on the device and "
                        "inside the step (Trainer(gradient_clip_val=)); 0 = off (the default)")
    p.add_argument("--track_grad_norm", action="store_true", default=False,
                   help="log the global L2 norm of the gradients as train/grad_norm without clipping (off by default)")
    p.add_argument("--ema_decay", type=_ema_decay, default=0.0,
                   help="keep an exponential moving average of the trained weights with this decay (LitEma's rule, warm-up "
                        "included; 0.9999 is its default), updated on the device inside every optimizer step and saved in the "
                        "checkpoints as model_ema.*; extract it with tool_extract_weights.py --ema; 0 = off (the default)")
    add_loss_args(p)
    add_lr_args(p)
    add_val_args(p)
    return p


def add_val_args(p):
    """Held-out validation by timestep band and the training-side bands (ctrlora_amd.validation; fine-tuning only); all off by
    default.  None of the flags is in the reference, whose validation_step draws t at random."""
    p.add_argument("--val_dataroot", type=str, default=None,
                   help="a held-out dataset laid out like --dataroot (CustomDataset); read in order, with prompt drop-out off")
    p.add_argument("--val_latent_cache", type=str, default=None,
                   help="directory written by scripts/tool_cache_latents.py for --val_dataroot: validate from the stored "
                        "first-stage posteriors")
    p.add_argument("--val_every", type=_non_negative_int, default=0,
                   help="run validation every N optimizer steps and once at the end: a fixed set of (image, t, noise) triples, "
                        "the plain l2 loss as val/loss_simple with its standard error and per timestep band, on the device "
                        "(replayed as one hipGraph per batch under --graph), logged to val_log.jsonl; 0 = off (the default)")
    p.add_argument("--val_batches", type=_non_negative_int, default=0, help="validate on the first M batches only; 0 = all")
    p.add_argument("--val_bands", type=int, default=10, help="timestep bands of the validation loss (1 .. 64)")
    p.add_argument("--val_repeats", type=int, default=1,
                   help="passes over the validation set; pass r moves every sample on by r bands and draws other noise")
    p.add_argument("--val_seed", type=int, default=0, help="seed of the validation plan's noise and of its forked generators")
    p.add_argument("--val_ema", action="store_true", default=False,
                   help="validate the EMA weights too (inside ema_scope(), keys with the suffix _ema); needs --ema_decay")
    p.add_argument("--save_best", action="store_true", default=False,
                   help="write best.ckpt whenever val/loss_simple (val/loss_simple_ema with --val_ema) improves")
    p.add_argument("--loss_bands", type=int, default=0,
                   help="break the TRAINING loss down by K timestep bands with one more small launch inside the step (this "
                        "rank's samples only), logged as train/loss_simple/t{lo}-{hi} where the loss is logged; 0 = off")


def check_val_args(args):
    """The refusals of the validation flags, each with its reason, before anything is loaded."""
    if args.val_every > 0 and not args.val_dataroot:
        raise SystemExit("--val_every needs a validation set: give --val_dataroot (and optionally --val_latent_cache)")
    if args.val_latent_cache and not args.val_dataroot:
        raise SystemExit("--val_latent_cache needs --val_dataroot: the cache stores the posteriors, the prompts come from the dataset")
    if args.val_ema and not args.ema_decay > 0.0:
        raise SystemExit("--val_ema needs --ema_decay: without it there are no EMA weights to validate")
    if (args.val_ema or args.save_best) and not args.val_every > 0:
        raise SystemExit("--val_ema / --save_best need --val_every N: they act on a validation run")
    if not 1 <= args.val_bands <= 64 or args.val_repeats < 1 or not 0 <= args.loss_bands <= 64:
        raise SystemExit("--val_bands and --loss_bands take 1 .. 64 bands (--loss_bands 0 = off), --val_repeats >= 1")


def build_val_dataloader(args):
    """The validation set in order, prompt drop-out off, the last batch kept; the Trainer splits it over the ranks by index."""
    from torch.utils.data import DataLoader
    if args.val_latent_cache:
        from datasets.cached_latents import CachedLatentDataset
        dataset = CachedLatentDataset(args.val_dataroot, args.val_latent_cache, drop_rate=0.0)
    else:
        from datasets.custom_dataset import CustomDataset
        dataset = CustomDataset(args.val_dataroot, drop_rate=0.0)
    workers = min(16, os.cpu_count() or 1) if getattr(args, "num_workers", None) is None else max(0, args.num_workers)
    return dataset, DataLoader(dataset, num_workers=workers, batch_size=args.bs, shuffle=False, drop_last=False)


def add_lr_args(p):
    """Learning-rate schedule and optimizer parameter groups (fine-tuning only); all off by default.  The groups and the flags are
    not in the reference; the scheduler takes the path of its LatentDiffusion.configure_optimizers (a LambdaLR per step)."""
    p.add_argument("--lr_schedule", choices=("constant", "linear", "cosine"), default=None,
                   help="move the learning rate along this curve over --max_steps (after --lr_warmup_steps of linear warm-up, "
                        "down to --lr_min_ratio x --lr); the curve lives in device memory and is read inside the optimizer step, "
                        "so it works under --graph without a copy between replays (default: a fixed learning rate)")
    p.add_argument("--lr_warmup_steps", type=_non_negative_int, default=0,
                   help="optimizer steps of linear warm-up, step n (from 0) at (n + 1) / N of the rate; alone it implies "
                        "--lr_schedule constant")
    p.add_argument("--lr_min_ratio", type=_unit_interval, default=0.0,
                   help="where the linear and cosine curves end, as a fraction of --lr")
    p.add_argument("--lora_plus_ratio", type=_positive_float, default=None,
                   help="LoRA+: train the LoRA up matrices (lora_layer.up.) at this multiple of --lr, as a parameter group of "
                        "their own inside the same fused AdamW launch (default: one learning rate)")
    p.add_argument("--no_decay_norm_bias", action="store_true", default=False,
                   help="no weight decay on the norm layers and the biases: a parameter group with weight_decay 0 (applied "
                        "after the LoRA+ rule)")


def _non_negative_int(text):
    value = int(text)
    if value < 0:
        raise argparse.ArgumentTypeError(f"{text}: a number of steps >= 0")
    return value


def _unit_interval(text):
    value = float(text)
    if not 0.0 <= value <= 1.0:
        raise argparse.ArgumentTypeError(f"{text}: a ratio in [0, 1]")
    return value


def _positive_float(text):
    value = float(text)
    if not value > 0.0 or value != value or value == float("inf"):
        raise argparse.ArgumentTypeError(f"{text}: a finite ratio > 0")
    return value


def lr_model_params(max_steps, lr_schedule=None, lr_warmup_steps=0, lr_min_ratio=0.0, lora_plus_ratio=None,
                    no_decay_norm_bias=False) -> dict:
    """The flags of add_lr_args: what create_model overrides in the config's model.params; nothing at the defaults."""
    out = {}
    if lr_schedule is not None or lr_warmup_steps > 0:
        out["scheduler_config"] = {"target": "ctrlora_amd.lr_schedule.WarmupDecay",
                                   "params": {"kind": lr_schedule or "constant", "warmup_steps": int(lr_warmup_steps),
                                              "total_steps": int(max_steps), "min_ratio": float(lr_min_ratio)}}
    rules = []
    if lora_plus_ratio is not None:
        rules.append({"name": "lora_up", "match": ["lora_layer.up."], "lr_scale": float(lora_plus_ratio)})
    if no_decay_norm_bias:
        rules.append({"name": "no_decay", "match": ["norm", ".bias"], "weight_decay": 0.0})
    if rules:
        out["optim_groups"] = rules
    return out


def add_loss_args(p):
    """The flags of the training objective (the same three as in train_ctrlora_pretrain.py); none of them is in the reference."""
    p.add_argument("--min_snr_gamma", type=float, default=0.0,
                   help="weight each sample's loss by min(SNR_t, gamma) / SNR_t (Min-SNR-gamma; 5 is the paper's value), on the "
                        "device and inside the step; 0 = off (the default)")
    p.add_argument("--loss", choices=("l2", "huber"), default=None,
                   help="the per-element loss: l2, or torch's huber_loss with --huber_delta (default: the config's loss_type)")
    p.add_argument("--huber_delta", type=float, default=None,
                   help="the Huber loss's threshold between its quadratic and its linear branch (default: the config's, 1.0)")


def loss_model_params(min_snr_gamma: float = 0.0, loss=None, huber_delta=None) -> dict:
    """--min_snr_gamma / --loss / --huber_delta: what create_model overrides in the config's model.params; nothing at the
    defaults.  The model's constructor refuses a negative gamma and a non-positive delta."""
    out = {}
    if min_snr_gamma != 0.0:
        out["min_snr_gamma"] = float(min_snr_gamma)
    if loss is not None:
        out["loss_type"] = loss
    if huber_delta is not None:
        out["huber_delta"] = float(huber_delta)
    return out


def val_trainer_args(args, model) -> dict:
    """The validation flags as Trainer arguments; nothing at the defaults."""
    out = {}
    if args.val_every > 0:
        from ctrlora_amd.validation import ValPlan
        out.update(val_check_interval=args.val_every, limit_val_batches=args.val_batches or None, val_ema=args.val_ema,
                   save_best=args.save_best,
                   val_plan=ValPlan(model.num_timesteps, nbands=args.val_bands, seed=args.val_seed, repeats=args.val_repeats))
    if args.loss_bands > 0:
        out["loss_bands"] = args.loss_bands
    return out


def _ema_decay(text):
    value = float(text)
    if not 0.0 <= value <= 1.0:
        raise argparse.ArgumentTypeError(f"--ema_decay {text}: a decay lies in [0, 1] (0 = off)")
    return value


def ema_model_params(ema_decay: float) -> dict:
    """--ema_decay F with F in (0, 1]: what create_model overrides in the config's model.params; nothing for 0."""
    return dict(use_ema=True, ema_decay=float(ema_decay)) if ema_decay > 0.0 else {}


def init_weights(model, sd_weights: dict, control_weights: dict, report_dir: str = "./tmp"):
    """Initialise a fine-tune model from an SD checkpoint and a Base-ControlNet checkpoint
    (train_ctrlora_finetune.py:76-113): every SD tensor the model has is taken; of the ControlNet checkpoint every
    `control_model` tensor the model has EXCEPT keys containing 'lora' (fresh LoRA layers are trained: A ~ N(0, 1/r),
    B = 0).  Returns ((copied_sd, missing_sd), (copied_cn, missing_cn)); the four lists are also written to
    `report_dir` under the reference's file names."""
    scratch = model.state_dict()
    copied_sd = [k for k in sd_weights if k in scratch]
    missing_sd = [k for k in sd_weights if k not in scratch]
    for k in copied_sd:
        scratch[k] = sd_weights[k].clone()
    cn_keys = [k for k in control_weights if "control_model" in k]
    missing_cn = [k for k in cn_keys if k not in scratch]
    copied_cn = [k for k in cn_keys if k in scratch and "lora" not in k]
    for k in copied_cn:
        scratch[k] = control_weights[k].clone()
    model.load_state_dict(scratch, strict=True)
    if getattr(model, "use_ema", False):
        model.reseed_ema()      # `scratch` carried the construction-time shadows along: the average starts at the loaded weights
    if report_dir:
        os.makedirs(report_dir, exist_ok=True)
        for name, keys in (("finetune_missing_keys_sd", missing_sd), ("finetune_copied_keys_sd", copied_sd),
                           ("finetune_missing_keys_cn", missing_cn), ("finetune_copied_keys_cn", copied_cn)):
            with open(os.path.join(report_dir, name + ".txt"), "w") as f:
                f.write("\n".join(keys))
    return (copied_sd, missing_sd), (copied_cn, missing_cn)


def build_dataloader(args, world_size: int, rank: int):
    from torch.utils.data import DataLoader, DistributedSampler, Subset
    cache = getattr(args, "latent_cache", None)
    if cache and args.multigen20m:
        raise ValueError("--latent_cache cannot be combined with --multigen20m: MultiGen20M crops at random, so its images "
                         "differ from epoch to epoch and their posteriors cannot be stored")
    if cache:
        from datasets.cached_latents import CachedLatentDataset
        dataset = CachedLatentDataset(args.dataroot, cache, drop_rate=args.drop_rate)
    elif args.multigen20m:
        from datasets.multigen20m import MultiGen20M
        dataset = MultiGen20M(path_json=os.path.join(args.dataroot, "json_files", f"aesthetics_plus_all_group_{args.task}_all.json"),
                              path_meta=args.dataroot, task=args.task, drop_rate=args.drop_rate)
    else:
        from datasets.custom_dataset import CustomDataset
        dataset = CustomDataset(args.dataroot, drop_rate=args.drop_rate)
    if args.subset > 0:
        dataset = Subset(dataset, range(args.subset))
    sampler = DistributedSampler(dataset, num_replicas=world_size, rank=rank, shuffle=True) if world_size > 1 else None
    workers = min(16, os.cpu_count() or 1) if getattr(args, "num_workers", None) is None else max(0, args.num_workers)
    loader = DataLoader(dataset, num_workers=workers, batch_size=args.bs, shuffle=sampler is None,
                        sampler=sampler, drop_last=True)
    return dataset, loader


def main(argv=None):
    import gc
    from cldm.logger import CheckpointEveryNSteps, ImageLogger
    from cldm.model import create_model, load_state_dict
    from ctrlora_amd.trainer import Trainer
    args = get_parser().parse_args(argv)
    check_val_args(args)
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    dataset, loader = build_dataloader(args, world, rank)
    val_loader = None
    if args.val_every > 0:
        val_set, val_loader = build_val_dataloader(args)
        if rank == 0:
            print("Validation set size:", len(val_set))
    if rank == 0:
        print("Dataset size:", len(dataset))
        print("Number of devices:", world)
        print("Batch size per device:", args.bs)
        print("Gradient accumulation:", args.gradacc)
        print("Total batch size:", args.bs * world * args.gradacc)
    model = create_model(args.config, params={**ema_model_params(args.ema_decay),
                                              **loss_model_params(args.min_snr_gamma, args.loss, args.huber_delta),
                                              **lr_model_params(args.max_steps, args.lr_schedule, args.lr_warmup_steps,
                                                                args.lr_min_ratio, args.lora_plus_ratio,
                                                                args.no_decay_norm_bias)}).cpu()
    model.learning_rate = args.lr
    model.sd_locked = True
    model.only_mid_control = False
    init_weights(model, load_state_dict(args.sd_ckpt, location="cpu"), load_state_dict(args.cn_ckpt, location="cpu"))
    print(f"Successfully initialize SD from {args.sd_ckpt}")
    print(f"Successfully initialize ControlNet from {args.cn_ckpt}")
    if args.latent_cache:
        from ctrlora_amd import latent_cache
        import torch
        latent_cache.check_model(latent_cache.load_meta(args.latent_cache), model,
                                 torch.float32 if str(args.precision) in ("32", "32-true") else torch.bfloat16)
        print(f"Training from the latent cache {args.latent_cache}: the first stage encodes nothing")
    if args.val_every > 0 and args.val_latent_cache:
        from ctrlora_amd import latent_cache
        import torch
        latent_cache.check_model(latent_cache.load_meta(args.val_latent_cache), model,
                                 torch.float32 if str(args.precision) in ("32", "32-true") else torch.bfloat16)
    gc.collect()
    name = args.name or datetime.datetime.now().strftime("%Y-%m-%d-%H-%M-%S")
    trainer = Trainer(max_steps=args.max_steps, accumulate_grad_batches=args.gradacc, precision=args.precision,
                      callbacks=[ImageLogger(batch_frequency=args.img_logger_freq),
                                 CheckpointEveryNSteps(save_step_frequency=args.ckpt_logger_freq)],
                      default_root_dir=os.path.join("runs", name), graph_step=bool(args.graph),
                      gradient_clip_val=args.grad_clip or None, track_grad_norm=2 if args.track_grad_norm else -1,
                      **val_trainer_args(args, model))
    trainer.fit(model, loader, val_dataloaders=val_loader)
    if trainer.logged_val and rank == 0:
        step, logs = trainer.logged_val[-1]
        print(f"[trainer] val/loss_simple at step {step}: {logs['val/loss_simple']:.5f} ({len(trainer.logged_val)} runs, "
              f"{os.path.join(trainer.log_dir, 'val_log.jsonl')})")
    if args.graph and rank == 0:
        print(f"[trainer] graph mode '{trainer.graph_mode}': {trainer.graph_replays} optimizer steps replayed, "
              f"{trainer.graph_eager_steps} launched eagerly")
    if trainer.logged_grad_norm and rank == 0:
        print(f"[trainer] train/grad_norm at step {trainer.logged_grad_norm[-1][0]}: {trainer.logged_grad_norm[-1][1]:.5f}")
    return trainer


if __name__ == "__main__":
    main()
