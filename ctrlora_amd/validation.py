"""Held-out validation loss by timestep band (not in the reference, whose `validation_step`, ddpm.py:457-463, logs one mean at
random t; `DDPM.validation_step` here mirrors that one).

A validation run evaluates a FIXED set of (x, t, noise) triples (`ValPlan`), so two checkpoints differ by their weights only,
and breaks the plain l2 loss down by timestep band in a small fp64 table {count, sum, sum of squares} per band plus a total
row.  On the GPU the table is filled by `cl_loss_bands` behind `ControlFinetuneLDM.engine_eval_step` (eager, or one hipGraph
replayed per batch: `GraphedEvalStep`); on the CPU, or for a model without the engine path, by `accumulate_bands`, the host
restatement with the same bits.  The loss is always l2 without per-timestep weights, whatever the training objective.

Nothing here moves the training trajectory: every draw of a run is made inside `torch.random.fork_rng` seeded from the plan
(the first-stage posterior samples of `get_input`, the cached-posterior draws) or on the plan's own CPU generators (the
q_sample noise); the global CPU generator and the device generator are where training left them when the run returns.
"""
from __future__ import annotations

import json
import math
import os
from typing import List, Optional, Sequence

import torch

ROW = 3      # count, sum, sum of squares


def band_of(t: int, T: int, nbands: int) -> int:
    """min(clamp(t, 0, T - 1) * nbands // T, nbands - 1): the band of timestep t (cl_loss_bands' rule)."""
    t = min(max(int(t), 0), T - 1)
    return min(t * nbands // T, nbands - 1)


def band_ranges(T: int, nbands: int) -> List[tuple]:
    """[(lo, hi)] inclusive timestep range of every band: band(t) == k  <=>  lo_k <= t <= hi_k."""
    lo = [-(-k * T // nbands) for k in range(nbands + 1)]       # ceil(k T / nbands)
    return [(lo[k], lo[k + 1] - 1) for k in range(nbands)]


def new_table(nbands: int, device="cpu") -> torch.Tensor:
    return torch.zeros(nbands + 1, ROW, dtype=torch.float64, device=device)


def accumulate_bands(per_sample, t, T: int, nbands: int, acc: torch.Tensor, n_valid=None) -> torch.Tensor:
    """The host restatement of cl_loss_bands: acc (fp64 [nbands + 1][3] on the CPU) += {1, x, x^2} of every counted sample, in
    index order, in fp64 from the fp32 loss.  n_valid: None or an int / one-element tensor; the first clamp(n_valid, 0, B) count."""
    assert 1 <= nbands <= min(T, 64) and tuple(acc.shape) == (nbands + 1, ROW) and acc.dtype == torch.float64
    x = torch.as_tensor(per_sample).detach().to("cpu", torch.float32).reshape(-1).double().tolist()   # Python floats are fp64
    tt = torch.as_tensor(t).detach().to("cpu").reshape(-1).tolist()
    B = len(x)
    assert len(tt) == B
    nv = B if n_valid is None else min(max(int(n_valid), 0), B)
    rows = acc.tolist()
    for b in range(nv):
        xb = x[b]
        for row in (band_of(tt[b], T, nbands), nbands):
            r = rows[row]
            r[0] += 1.0
            r[1] += xb
            r[2] += xb * xb
    acc.copy_(torch.tensor(rows, dtype=torch.float64))
    return acc


class ValPlan:
    """Which (t, noise) validation sample j gets in pass r: t = grid[(j + r) % nbands] with grid[k] = (2k + 1) T // (2 nbands),
    the middle of band k, and the j-th draw of a CPU generator seeded from (seed, r).  j is the sample's index in the
    validation SET, so the triples do not depend on the batch size or on how the set is split over ranks."""

    def __init__(self, num_timesteps: int, nbands: int = 10, seed: int = 0, repeats: int = 1):
        T, nbands, repeats = int(num_timesteps), int(nbands), int(repeats)
        if T < 1 or not 1 <= nbands <= min(T, 64):
            raise ValueError(f"ValPlan: nbands={nbands} must lie in 1 .. min(num_timesteps={T}, 64)")
        if repeats < 1:
            raise ValueError(f"ValPlan: repeats={repeats} must be >= 1")
        self.num_timesteps, self.nbands, self.seed, self.repeats = T, nbands, int(seed), repeats
        self.grid = [(2 * k + 1) * T // (2 * nbands) for k in range(nbands)]

    def timesteps(self, indices: Sequence[int], r: int = 0) -> torch.Tensor:
        return torch.tensor([self.grid[(int(j) + r) % self.nbands] for j in indices], dtype=torch.long)

    def pass_seed(self, r: int) -> int:
        return (self.seed * 1000003 + r) % (1 << 63)

    def noise_stream(self, r: int, shape) -> "_NoiseStream":
        return _NoiseStream(self.pass_seed(r), tuple(shape))

    def noise(self, indices: Sequence[int], r: int, shape) -> torch.Tensor:
        """The noise of samples `indices` (increasing) in pass r, from a fresh stream: [len(indices), *shape]."""
        return self.noise_stream(r, shape).take(indices)

    def fork_seed(self) -> int:
        return (self.seed * 1000003 + 999983) % (1 << 63)

    def labels(self) -> List[str]:
        return [f"t{lo}-{hi}" for lo, hi in band_ranges(self.num_timesteps, self.nbands)]


class _NoiseStream:
    """Draws of one pass in index order, one sample per torch.randn call; samples that are skipped (another rank's) are drawn
    and dropped, so sample j's noise is the same however the set is split."""

    def __init__(self, seed, shape):
        self.gen, self.shape, self.next = torch.Generator().manual_seed(seed), shape, 0

    def take(self, indices):
        out = []
        for j in indices:
            assert j >= self.next, "validation samples are visited in increasing index order"
            while self.next <= j:
                e = torch.randn(self.shape, generator=self.gen)
                self.next += 1
            out.append(e)
        return torch.stack(out) if out else torch.empty((0,) + self.shape)


def table_logs(table: torch.Tensor, plan: ValPlan, prefix: str = "val", suffix: str = "") -> dict:
    """{prefix/loss_simple, prefix/loss_simple_se, prefix/loss_simple/t{lo}-{hi}} (+ suffix) of a [nbands + 1][3] table: the
    total row's mean, its standard error sqrt(var / n) with the unbiased variance, and every populated band's mean."""
    tab = table.detach().to("cpu", torch.float64).tolist()
    n, s1, s2 = tab[plan.nbands]
    logs = {}
    mean = s1 / n if n > 0 else float("nan")
    var = max(s2 - n * mean * mean, 0.0) / (n - 1) if n > 1 else float("nan")
    logs[f"{prefix}/loss_simple{suffix}"] = mean
    logs[f"{prefix}/loss_simple_se{suffix}"] = math.sqrt(var / n) if n > 1 and math.isfinite(var) else float("nan")
    for label, (cnt, b1, _) in zip(plan.labels(), tab):
        if cnt > 0:
            logs[f"{prefix}/loss_simple/{label}{suffix}"] = b1 / cnt
    return logs


def engine_eval_refusal(model, device) -> Optional[str]:
    """Why the validation step cannot run on the engine (the host path is taken then), or None."""
    if torch.device(device).type != "cuda":
        return "not on a GPU"
    if not callable(getattr(model, "engine_eval_step", None)):
        return f"{type(model).__name__} has no engine_eval_step"
    return None


class GraphedEvalStep:
    """`engine_eval_step` as ONE hipGraph over static inputs (`_StaticInputs` of ctrlora_amd.train) and a table that lives as
    long as this object.  The first batch runs eagerly (it sizes every buffer and fixes the shape), the capture follows
    (capturing executes nothing) and every later batch of that shape replays.  A ragged last batch -- any batch of another
    shape -- runs EAGERLY at its own size: padded to the captured shape (cl_loss_bands' n_valid exists for that) it would go
    through the products of another batch size, which in bf16 are other tile configurations with other roundings, and the
    table would no longer have the bits of the eager path.  The graph holds no address of the training step's buffers beyond
    the weights, which ema_scope() swaps in place: it stays valid next to a captured training step and inside the scope."""

    def __init__(self, model, nbands: int):
        self.model, self.nbands = model, int(nbands)
        dev = model.device
        self.acc = new_table(nbands, dev)
        self._static = self.graph = None
        self.replays = self.eager_steps = self.captures = 0

    def clear(self):
        from . import hip
        hip.zero_(self.acc)

    def _run(self, tensors):
        z, ctx, hint, t, noise = tensors
        self.model.engine_eval_step(z, {"c_crossattn": [ctx], "c_concat": [hint]}, t, noise, self.acc)

    def __call__(self, z, ctx, hint, t, noise):
        from .train import _StaticInputs
        tensors = (z, ctx, hint, t, noise)
        if self._static is None:                      # the first batch: eager, and the shape that is captured
            self._static = _StaticInputs(*tensors)
            self._run(tensors)
            self.eager_steps += 1
            return
        if not self._static.matches(*tensors):
            self._run(tensors)
            self.eager_steps += 1
            return
        self._static.load(*tensors)
        if self.graph is None:
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self._run(self._static.tensors)
            self.captures += 1
        self.graph.replay()
        self.replays += 1


def shard_loader(loader, rank: int, world: int):
    """The loader of rank `rank`'s share of the validation set: samples j = rank, rank + world, ... in order, no padding
    duplicates (a rank may get one sample fewer than another).  The k-th sample a rank sees is sample rank + k * world of the
    set.  One process: the loader as it is (any iterable of batches, visited in order)."""
    if world <= 1:
        return loader
    if not hasattr(loader, "dataset"):
        raise ValueError("validation under several ranks needs a DataLoader (its dataset is split by index), not "
                         f"{type(loader).__name__}")
    from torch.utils.data import DataLoader, Subset
    idx = list(range(rank, len(loader.dataset), world))
    return DataLoader(Subset(loader.dataset, idx), batch_size=loader.batch_size, shuffle=False, num_workers=loader.num_workers,
                      collate_fn=loader.collate_fn, drop_last=False)


@torch.no_grad()
def run_validation(model, loader, plan: ValPlan, step: Optional[GraphedEvalStep] = None, limit_batches: Optional[int] = None,
                   rank: int = 0, world: int = 1, on_engine: Optional[bool] = None, device=None) -> torch.Tensor:
    """One pass over the validation loader under the plan.  Returns the rank-local fp64 table: on the model's device (not read
    here) on the engine path, on the CPU on the host path.  `step`: a GraphedEvalStep (its table is cleared, filled and
    returned as a clone) or None for eager launches.  The module is put in eval() for the run and back after; all draws are
    forked (module docstring)."""
    dev = torch.device(device) if device is not None else model.device
    if on_engine is None:
        on_engine = engine_eval_refusal(model, dev) is None
    T, nb = plan.num_timesteps, plan.nbands
    loader = shard_loader(loader, rank, world)
    world = max(1, world)
    was_training = model.training
    model.eval()
    devices = [dev] if dev.type == "cuda" else []
    try:
        with torch.random.fork_rng(devices=devices):
            torch.manual_seed(plan.fork_seed())
            if on_engine:
                if step is not None:
                    step.clear()
                    acc = step.acc
                else:
                    from . import hip
                    acc = hip.zero_(torch.empty(nb + 1, ROW, dtype=torch.float64, device=dev))
            else:
                acc = new_table(nb)
            streams, seen = None, 0
            for bi, batch in enumerate(loader):
                if limit_batches is not None and bi >= limit_batches:
                    break
                z, cond = model.get_input(batch, model.first_stage_key)
                n = int(z.shape[0])
                js = [rank + (seen + i) * world for i in range(n)]
                seen += n
                if streams is None:
                    streams = [plan.noise_stream(r, z.shape[1:]) for r in range(plan.repeats)]
                if on_engine:
                    hint = model._hint_latent(cond)
                    cc = cond["c_crossattn"]
                    ctx = cc[0] if len(cc) == 1 else torch.cat(cc, 1)
                for r in range(plan.repeats):
                    t = plan.timesteps(js, r).to(dev)
                    noise = streams[r].take(js).to(dev)
                    if not on_engine:
                        x_noisy = model.q_sample(x_start=z, t=t, noise=noise)
                        out = model.apply_model(x_noisy, t, cond)
                        per = ((out.float() - noise.float()) ** 2).mean(dim=tuple(range(1, out.dim())))
                        accumulate_bands(per, t, T, nb, acc)
                    elif step is not None:
                        step(z, ctx, hint, t, noise)
                    else:
                        model.engine_eval_step(z, {"c_crossattn": [ctx], "c_concat": [hint]}, t, noise, acc)
            if seen == 0 and world == 1:
                raise RuntimeError("empty validation dataloader")
            return acc.clone() if step is not None and on_engine else acc
    finally:
        model.train(was_training)


def reduce_tables(table: torch.Tensor, world: int) -> torch.Tensor:
    """The ranks' fp64 tables all-gathered and added in rank order: every rank ends with the same bits."""
    if world <= 1:
        return table
    import torch.distributed as dist
    parts = [torch.empty_like(table) for _ in range(world)]
    dist.all_gather(parts, table.contiguous())
    total = parts[0].clone()
    for p in parts[1:]:
        total += p
    return total


def append_jsonl(path: str, row: dict):
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "a") as f:
        f.write(json.dumps(row) + "\n")
