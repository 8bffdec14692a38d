"""Learning-rate schedules for fine-tuning: the factor a `torch.optim.lr_scheduler.LambdaLR` multiplies the base lr by, and the
same curve as a table the engine's optimizer keeps in device memory (`ctrlora_amd.train._FlatAdamW.set_lr_schedule`), so that a
captured optimizer step follows it without a host-to-device copy between replays.

A `scheduler_config` names `WarmupDecay` the way the reference's names `ldm.lr_scheduler.LambdaLinearScheduler`
(ldm/models/diffusion/ddpm.py:1288-1299): `instantiate_from_config(cfg).schedule` is the `lr_lambda`.
"""
from __future__ import annotations

import math

import torch

KINDS = ("constant", "linear", "cosine")


class WarmupDecay:
    """Linear warm-up over `warmup_steps` optimizer steps, then `kind` down to `min_ratio` at `total_steps`, flat beyond.

        n < warmup_steps:   (n + 1) / warmup_steps
        otherwise, with q = min(1, (n - warmup_steps) / max(1, total_steps - warmup_steps)):
            constant   1
            linear     1 - (1 - min_ratio) q
            cosine     min_ratio + (1 - min_ratio) * 0.5 * (1 + cos(pi q))

    `n` counts from 0: LambdaLR calls the lambda with 0 for the first optimizer step."""

    def __init__(self, kind: str, warmup_steps: int, total_steps: int, min_ratio: float = 0.0):
        if kind not in KINDS:
            raise ValueError(f"kind '{kind}': one of {KINDS}")
        if int(warmup_steps) != warmup_steps or warmup_steps < 0:
            raise ValueError(f"warmup_steps={warmup_steps!r}: a whole number >= 0")
        if int(total_steps) != total_steps or total_steps < 1:
            raise ValueError(f"total_steps={total_steps!r}: a whole number >= 1")
        if not 0.0 <= float(min_ratio) <= 1.0:
            raise ValueError(f"min_ratio={min_ratio!r}: a ratio in [0, 1]")
        self.kind, self.warmup_steps, self.total_steps = kind, int(warmup_steps), int(total_steps)
        self.min_ratio = float(min_ratio)

    def schedule(self, n, **kwargs) -> float:
        n = int(n)
        if n < self.warmup_steps:
            return (n + 1) / self.warmup_steps
        q = min(1.0, (n - self.warmup_steps) / max(1, self.total_steps - self.warmup_steps))
        if self.kind == "constant":
            return 1.0
        if self.kind == "linear":
            return 1.0 - (1.0 - self.min_ratio) * q
        return self.min_ratio + (1.0 - self.min_ratio) * 0.5 * (1.0 + math.cos(math.pi * q))

    __call__ = schedule


def compile_lambda_lr(scheduler, total_steps: int) -> torch.Tensor:
    """The curve of a LambdaLR as an fp32 [total_steps, G] table: entry [n, k] = base_lr_k * lambda_k(n), computed in Python
    floats exactly as `LambdaLR.get_lr` computes what it writes into `param_groups[k]["lr"]` for optimizer step n + 1, then
    rounded to fp32 once.  The scheduler is not stepped."""
    from torch.optim.lr_scheduler import LambdaLR
    if not isinstance(scheduler, LambdaLR):
        raise TypeError(f"compile_lambda_lr takes a LambdaLR, not {type(scheduler).__name__}: only a lambda of the step number "
                        "can be tabulated ahead of the run")
    if int(total_steps) < 1:
        raise ValueError(f"total_steps={total_steps!r}: at least one row")
    rows = [[base_lr * lmbda(n) for lmbda, base_lr in zip(scheduler.lr_lambdas, scheduler.base_lrs)]
            for n in range(int(total_steps))]
    return torch.tensor(rows, dtype=torch.float64).to(torch.float32)
