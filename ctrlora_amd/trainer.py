"""A Lightning-free training loop with the pieces of `pl.Trainer` the reference's train scripts use
(scripts/train_ctrlora_finetune.py:122-129: strategy='ddp', accumulate_grad_batches, max_steps, precision,
callbacks, default_root_dir).

One process per GPU: launch with `torchrun --nproc-per-node N script.py ...` (RANK / LOCAL_RANK / WORLD_SIZE from
the environment, backend "nccl" = RCCL); the only collective is the all-reduce of the flat LoRA gradient buffer
(`ctrlora_amd.parallel.GradAllReduce`), suppressed on non-final gradient-accumulation micro-steps.  The model is
any module with the LightningModule-style hooks the reference's LDM classes expose: `training_step(batch,
batch_idx) -> loss`, `configure_optimizers()`, optionally `set_engine_dtype`, `dp`, `log_images`.

Semantics kept from Lightning 1.5: the loss of each micro-batch is divided by `accumulate_grad_batches`;
`global_step` counts OPTIMIZER steps; callbacks get `on_train_batch_end(trainer, module, outputs, batch, batch_idx)`
after every micro-batch and `on_batch_end(trainer, module)` (what `CheckpointEveryNSteps` hooks); checkpoints are
`{"state_dict", "global_step", "epoch", "optimizer_states"}` and resumable with `fit(..., ckpt_path=)`.

`gradient_clip_val` / `gradient_clip_algorithm` / `track_grad_norm` carry Lightning 1.5's names: clipping by the global L2
norm of the gradients before the optimizer step (once per optimizer step, after the exchange and the last accumulation
micro-step), and / or tracking that norm as `train/grad_norm`.  The engine's optimizers do both on the device inside their own
step (`ctrlora_amd.train._FlatAdamW`), so it replays with the rest of a captured step; any other optimizer goes through
`torch.nn.utils.clip_grad_norm_`.  Clipping by value is not offered.

Learning-rate schedulers: `configure_optimizers()` may return a bare optimizer, `[opt]`, `([opt], [sched | {"scheduler": sched,
"interval": "step"}])` or `{"optimizer": opt, "lr_scheduler": sched | {...}}` (Lightning's forms, one optimizer).  The scheduler
is stepped once per OPTIMIZER step, after the last accumulation micro-step; `"interval": "epoch"` is refused.  For an engine
optimizer a `LambdaLR` is compiled to a table of `max_steps` rows that the optimizer keeps in device memory and reads inside its
own (captured) step (`_FlatAdamW.set_lr_schedule`); the host scheduler is still stepped, as the mirror that is logged (`train/lr`,
or `train/lr/<group>` with parameter groups) and saved (`lr_schedulers` in the checkpoint).  Any other scheduler class moves the
lr on the host (`scheduler.step()` + `sync_hyper()`), which `graph_step` refuses.

`graph_step=True` (LoRA fine-tuning on a GPU only; off by default) replays the optimizer step as hipGraphs
(`ctrlora_amd.train.GraphedTrainStep`) instead of launching its ~1900 kernels one by one: see `Trainer._fit_graphed`.

Validation (`fit(..., val_dataloaders=)` with `val_check_interval=N` optimizer steps; off by default; `ctrlora_amd.validation`):
a fixed plan of (sample, t, noise) triples, the plain l2 loss by timestep band in a small fp64 table filled on the device
(`cl_loss_bands`), read once per run; `val_ema` repeats the run inside `ema_scope()`, `save_best` writes `best.ckpt` on
improvement, `limit_val_batches` caps a run.  A run forks every generator it draws on: training continues on the numbers it
would have had.  `loss_bands=K` breaks the training loss down the same way, inside the step, rank-local.  See `Trainer._validate`.
"""
from __future__ import annotations

import os
from typing import Optional, Sequence

import torch


class _CheckpointDir:
    """`trainer.checkpoint_callback.dirpath` / `.filename` as the reference's callbacks read them."""

    def __init__(self, dirpath):
        self.dirpath, self.filename = dirpath, "last.ckpt"


_GRAPH_OPTIONS = ("split_graphs", "bucket_bytes", "reduce_fn", "warm_steps")


def graph_step_refusal(model) -> Optional[str]:
    """Why `graph_step` cannot run this model, in one line, or None.  Checked before the first step: nothing falls back to
    the eager loop in the middle of a run."""
    cm = getattr(model, "control_model", None)
    if callable(getattr(model, "init_data_parallel", None)) or hasattr(cm, "switch_lora"):
        return ("multi-task pre-training switches the LoRA bank from step to step (ctrlora_amd.train.GraphedPretrainStep is "
                "single-process): it keeps the eager loop")
    if not callable(getattr(model, "engine_train_step", None)):
        return f"{type(model).__name__} has no engine_train_step (the step without torch.autograd that a capture needs)"
    if getattr(model, "loss_type", "l2") not in ("l2", "huber"):       # "huber": cl_p_losses_w, not in the reference
        return f"engine_train_step computes the l2 loss only, the model's loss_type is '{model.loss_type}'"
    if float(getattr(model, "original_elbo_weight", 0.0)) != 0.0:
        return f"engine_train_step leaves the elbo term out, the model's original_elbo_weight is {model.original_elbo_weight}"
    return None


def validation_refusal(model) -> Optional[str]:
    """Why this model cannot be validated / banded by the Trainer, in one line, or None."""
    cm = getattr(model, "control_model", None)
    if callable(getattr(model, "init_data_parallel", None)) or hasattr(cm, "switch_lora"):
        return ("multi-task pre-training has one LoRA bank per task and no held-out set per bank: validation and loss bands are "
                "built for fine-tuning only (ControlFinetuneLDM)")
    return None


class Trainer:
    def __init__(self, max_steps: int = 100000, accumulate_grad_batches: int = 1, precision=32,
                 callbacks: Sequence = (), default_root_dir: str = "runs/default", device: Optional[str] = None,
                 strategy: str = "ddp", accelerator: str = "gpu", devices=-1, log_every_n_steps: int = 50,
                 graph_step=False, gradient_clip_val=None, gradient_clip_algorithm: str = "norm", track_grad_norm=-1,
                 val_check_interval: int = 0, limit_val_batches: Optional[int] = None, val_plan=None, val_ema: bool = False,
                 save_best: bool = False, loss_bands: int = 0):
        self.max_steps = int(max_steps)
        if int(val_check_interval) < 0:
            raise ValueError(f"val_check_interval={val_check_interval!r} counts optimizer steps: >= 0 (0 = off)")
        if limit_val_batches is not None and int(limit_val_batches) < 1:
            raise ValueError(f"limit_val_batches={limit_val_batches!r} must be None (all) or >= 1")
        if not 0 <= int(loss_bands) <= 64:
            raise ValueError(f"loss_bands={loss_bands!r} must lie in 0 .. 64 (0 = off)")
        self.val_check_interval = int(val_check_interval)
        self.limit_val_batches = None if limit_val_batches is None else int(limit_val_batches)
        self.val_plan, self.val_ema, self.save_best, self.loss_bands = val_plan, bool(val_ema), bool(save_best), int(loss_bands)
        self.logged_val = []            # (global_step, {"val/loss_simple": ..., "val/loss_simple/t0-99": ..., ...}) per validation run
        self.logged_train_bands = []    # (global_step, fp64 table [loss_bands + 1][3] of the interval) at log_every_n_steps
        self.best_val = float("inf")    # the monitored validation loss of best.ckpt (save_best)
        self.val_tables = None          # the fp64 tables of the latest run: [1 or 2 (live, EMA)][nbands + 1][3], reduced over ranks
        self._val_loader = self._val_step = self._train_bands = None
        self._val_on = self._val_on_engine = False
        self._val_last_step = -1
        if gradient_clip_algorithm != "norm":
            raise ValueError(f"gradient_clip_algorithm='{gradient_clip_algorithm}' is not supported: gradients are clipped by their "
                             "global L2 norm only ('norm'); clipping by value is not offered")
        if track_grad_norm not in (-1, 2, 2.0):
            raise ValueError(f"track_grad_norm={track_grad_norm!r}: -1 (off) or 2 (the L2 norm) only")
        if gradient_clip_val is not None and not float(gradient_clip_val) >= 0.0:
            raise ValueError(f"gradient_clip_val={gradient_clip_val!r} must be None or >= 0 (0 = off)")
        self.gradient_clip_val = float(gradient_clip_val) if gradient_clip_val else 0.0      # 0.0 = off
        self.track_grad_norm = track_grad_norm != -1
        self._norm_on = self._norm_in_opt = False       # decided in fit(), once the optimizer exists
        self.logged_grad_norm = []      # (global_step, norm) at log_every_n_steps, where the loss is read too
        self.accumulate_grad_batches = max(1, int(accumulate_grad_batches))
        self.precision = precision
        self.callbacks = list(callbacks)
        self.default_root_dir = default_root_dir
        self.log_every_n_steps = log_every_n_steps
        self.world_size = int(os.environ.get("WORLD_SIZE", "1"))
        self.global_rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        self.device = torch.device(device) if device is not None else torch.device("cuda", self.local_rank)
        self.log_dir = os.path.join(default_root_dir, "lightning_logs", "version_0")
        self.checkpoint_callback = _CheckpointDir(os.path.join(self.log_dir, "checkpoints"))
        self.global_step = 0
        self.current_epoch = 0
        self.model = None
        self.optimizer = None
        self.lr_scheduler = None        # the one scheduler configure_optimizers() returned, or None
        self._lr_on_device = False      # an engine optimizer reads the compiled curve from device memory
        self.logged_lr = []             # (global_step, {"train/lr[/<group>]": lr the step used}) at log_every_n_steps
        self.logged = []
        # graph_step: False = the eager loop; True or a dict of options = captured steps (_fit_graphed)
        self.graph_step = bool(graph_step) or isinstance(graph_step, dict)
        self._graph_opts = dict(graph_step) if isinstance(graph_step, dict) else {}
        unknown = set(self._graph_opts) - set(_GRAPH_OPTIONS)
        if unknown:
            raise ValueError(f"graph_step: unknown option(s) {sorted(unknown)}; known: {list(_GRAPH_OPTIONS)}")
        if self.graph_step and self.device.type != "cuda":
            raise ValueError(f"graph_step needs a GPU: a hipGraph cannot be captured on device '{self.device}'")
        self.graph_replays = 0          # optimizer steps whose every micro-step was a replay
        self.graph_eager_steps = 0      # optimizer steps with at least one eagerly launched micro-step (warm-up, other shapes)
        self.graph_mode = "off"         # "one" | "segmented" once the step object exists

    # ------------------------------------------------------------------ helpers
    @property
    def is_global_zero(self):
        return self.global_rank == 0

    def engine_dtype(self):
        return torch.float32 if str(self.precision) in ("32", "32-true") else torch.bfloat16

    def _call(self, hook, *args):
        for cb in self.callbacks:
            fn = getattr(cb, hook, None)
            if callable(fn):
                fn(self, *args)

    def _init_distributed(self, model):
        if self.world_size <= 1:
            return
        import torch.distributed as dist
        if not dist.is_initialized():
            os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
            backend = "nccl" if self.device.type == "cuda" else "gloo"
            dist.init_process_group(backend, **({"device_id": self.device} if backend == "nccl" else {}))
        # what Lightning's DDP wrapper does at wrap time: every rank starts from rank 0's parameters and buffers
        # (the LoRA down-projections are drawn from an unseeded N(0, 1/r) in every process)
        self.broadcast_module_state(model)
        if callable(getattr(model, "init_data_parallel", None)) and self.device.type == "cuda":
            model.init_data_parallel()           # pre-training: bank-sparse exchange (base buffer + live LoRA banks)
        elif hasattr(model, "control_model") and hasattr(model.control_model, "executor") and self.device.type == "cuda":
            from ctrlora_amd.parallel import GradAllReduce
            model.dp = GradAllReduce([model.control_model.executor()])

    @staticmethod
    def broadcast_module_state(model, src: int = 0):
        """In-place broadcast of all parameters and buffers from rank `src` (no-op without a process group)."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return
        with torch.no_grad():
            for t in list(model.parameters()) + list(model.buffers()):
                if t.numel():
                    dist.broadcast(t.data, src)

    def save_checkpoint(self, path):
        if not self.is_global_zero:
            return
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        opt_state = self.optimizer.state_dict() if hasattr(self.optimizer, "state_dict") else None
        ck = {"state_dict": self.model.state_dict(), "global_step": self.global_step,
              "epoch": self.current_epoch, "optimizer_states": [opt_state]}
        if self.lr_scheduler is not None:
            ck["lr_schedulers"] = [self.lr_scheduler.state_dict()]      # Lightning's key
        torch.save(ck, path)

    def _restore_model(self, ckpt_path):
        """Model part of a resume: BEFORE the executors / optimizer are built (they snapshot the weights)."""
        ck = torch.load(ckpt_path, map_location="cpu", weights_only=False)
        self.model.load_state_dict(ck["state_dict"], strict=True)
        self.global_step, self.current_epoch = int(ck.get("global_step", 0)), int(ck.get("epoch", 0))
        return ck

    def _restore_optimizer(self, ck):
        st = (ck.get("optimizer_states") or [None])[0]
        if st is not None and hasattr(self.optimizer, "load_state_dict"):
            self.optimizer.load_state_dict(st)
        saved = (ck.get("lr_schedulers") or [None])[0]
        if self.lr_scheduler is not None and saved is not None:
            self.lr_scheduler.load_state_dict(saved)      # the step count: the curve continues where the checkpoint left it

    @staticmethod
    def unpack_optimizers(ret):
        """What `configure_optimizers()` returned -> (optimizer, scheduler or None).  One optimizer, at most one scheduler."""
        opts, scheds = ret, []
        if isinstance(ret, dict):
            opts, scheds = ret["optimizer"], ret.get("lr_scheduler")
        elif isinstance(ret, (list, tuple)) and len(ret) == 2 and all(isinstance(x, (list, tuple)) for x in ret):
            opts, scheds = ret
        opts = list(opts) if isinstance(opts, (list, tuple)) else [opts]
        scheds = [] if scheds is None else list(scheds) if isinstance(scheds, (list, tuple)) else [scheds]
        if len(opts) != 1 or len(scheds) > 1:
            raise ValueError(f"configure_optimizers() returned {len(opts)} optimizers and {len(scheds)} schedulers: this loop "
                             "drives one optimizer and at most one scheduler")
        sched = scheds[0] if scheds else None
        if isinstance(sched, dict):
            interval, freq = sched.get("interval", "step"), int(sched.get("frequency", 1))
            if interval != "step" or freq != 1:
                raise ValueError(f"lr scheduler with interval='{interval}', frequency={freq}: the scheduler is stepped once per "
                                 "optimizer step ('step', 1); a run is bounded by max_steps, not by epochs")
            sched = sched["scheduler"]
        return opts[0], sched

    def _set_up_lr_schedule(self):
        """Before the first step (and so before any capture): hand an engine optimizer the LambdaLR's curve as a device table."""
        from torch.optim.lr_scheduler import LambdaLR
        from ctrlora_amd.train import _FlatAdamW
        sched = self.lr_scheduler
        self._lr_on_device = False
        if sched is None or not isinstance(self.optimizer, _FlatAdamW) or self.device.type != "cuda":
            return
        if isinstance(sched, LambdaLR):
            from ctrlora_amd.lr_schedule import compile_lambda_lr
            self.optimizer.set_lr_schedule(compile_lambda_lr(sched, self.max_steps))
            self._lr_on_device = True
        elif self.graph_step:
            raise ValueError(f"graph_step refused: a {type(sched).__name__} moves the learning rate on the host, a copy to the "
                             "device between replays that makes the host wait for the step before; only a LambdaLR is compiled "
                             "to a device table")

    def _lr_logs(self):
        """The learning rate(s) of the host mirror, under `train/lr` or, with parameter groups, `train/lr/<group>`."""
        groups = self.optimizer.param_groups
        if len(groups) == 1:
            return {"train/lr": float(groups[0]["lr"])}
        return {f"train/lr/{g.get('name', k)}": float(g["lr"]) for k, g in enumerate(groups)}

    def _step_lr(self, model, step, log):
        """After optimizer step `step` (1-based): log the lr it used, then move the scheduler on to the next step's."""
        if self.lr_scheduler is None:
            return {}
        logs = self._lr_logs() if log else {}
        if log:
            self.logged_lr.append((step, logs))
        self.lr_scheduler.step()
        if not self._lr_on_device and hasattr(self.optimizer, "sync_hyper"):
            self.optimizer.sync_hyper()
        return logs

    # ------------------------------------------------------------------ the loop
    def fit(self, model, train_dataloader, ckpt_path: Optional[str] = None, val_dataloaders=None):
        self.model = model
        self._check_validation_options(model, val_dataloaders)
        if self.graph_step:
            why = graph_step_refusal(model)
            if why is not None:
                raise ValueError("graph_step refused: " + why)
        if self.device.type == "cuda":
            torch.cuda.set_device(self.device)
        model.to(self.device).train()
        if hasattr(model, "set_engine_dtype"):
            model.set_engine_dtype(self.engine_dtype())
        ck = self._restore_model(ckpt_path) if ckpt_path else None
        self._init_distributed(model)
        self.optimizer, self.lr_scheduler = self.unpack_optimizers(model.configure_optimizers())
        if ck is not None:
            self._restore_optimizer(ck)
        self._set_up_grad_norm()
        self._set_up_lr_schedule()
        if self.graph_step and self._norm_on and not self._norm_in_opt:
            raise ValueError(f"graph_step with gradient clipping needs an engine optimizer, not {type(self.optimizer).__name__}")
        self._set_up_validation(model, val_dataloaders)
        try:
            if self.graph_step:
                self._fit_graphed(model, train_dataloader)
            else:
                self._fit_eager(model, train_dataloader)
            if self._val_on and self._val_last_step != self.global_step:
                self._validate(model)           # once at the end of fit, unless the last step's own run was it
        finally:
            if self._train_bands is not None:
                model.train_loss_bands = None
        self._call("on_train_end", model)
        return self

    def _fit_eager(self, model, train_dataloader):
        acc = self.accumulate_grad_batches
        dp = getattr(model, "dp", None)
        # an EMA of the trained weights (model.model_ema: ldm.modules.ema.ModelEma) that the optimizer does not carry inside its
        # own step (a CPU run, a plain torch optimizer) is updated here, by the module's host restatement
        ema_on_host = getattr(model, "model_ema", None) is not None and getattr(self.optimizer, "ema", None) is None
        self.optimizer.zero_grad()
        micro = 0
        while self.global_step < self.max_steps:
            sampler = getattr(train_dataloader, "sampler", None)
            if hasattr(sampler, "set_epoch"):
                sampler.set_epoch(self.current_epoch)
            seen = 0
            for batch_idx, batch in enumerate(train_dataloader):
                seen += 1
                last = (micro + 1) % acc == 0
                if dp is not None:
                    dp.enabled = last                      # exchange gradients on the final micro-step only
                loss = model.training_step(batch, batch_idx)
                (loss / acc).backward()
                micro += 1
                if last:
                    norm = self._clip_torch() if self._norm_on and not self._norm_in_opt else None
                    self.optimizer.step()
                    if ema_on_host:
                        model.model_ema(model)      # once per optimizer step, like the engine optimizer's own update
                    if self._norm_in_opt:
                        norm = self.optimizer.last_grad_norm()[0]
                    self.optimizer.zero_grad()
                    self.global_step += 1
                    model.global_step = self.global_step
                    log = self.global_step % self.log_every_n_steps == 0
                    lr_logs = self._step_lr(model, self.global_step, log)
                    if log:
                        self._log_grad_norm(model, norm, self.global_step, more=lr_logs)
                    if self.is_global_zero and self.global_step % self.log_every_n_steps == 0:
                        self.logged.append((self.global_step, float(loss.detach())))
                        print(f"[trainer] step {self.global_step} epoch {self.current_epoch} loss {float(loss.detach()):.5f}")
                    self._after_optimizer_step(model)
                self._call("on_train_batch_end", model, {"loss": loss.detach()}, batch, batch_idx)
                self._call("on_batch_end", model)
                if self.global_step >= self.max_steps:
                    break
            if seen == 0:
                raise RuntimeError("empty dataloader")
            self.current_epoch += 1
            model.current_epoch = self.current_epoch

    # ------------------------------------------------------------------ gradient norm: clip and / or track
    def _set_up_grad_norm(self):
        """Before the first step: an engine optimizer takes the settings and does the work inside its own step (eager or
        captured); any other optimizer is clipped by `_clip_torch` in the eager loop."""
        from ctrlora_amd.train import _FlatAdamW
        self._norm_on = self.gradient_clip_val > 0.0 or self.track_grad_norm
        self._norm_in_opt = self._norm_on and isinstance(self.optimizer, _FlatAdamW)
        if self._norm_in_opt:
            self.optimizer.max_grad_norm = self.gradient_clip_val if self.gradient_clip_val > 0.0 else None
            self.optimizer.track_grad_norm = self.track_grad_norm
            self.optimizer.sync_hyper()

    def _clip_torch(self):
        """torch.nn.utils.clip_grad_norm_ over the optimizer's parameters; tracking alone measures with an infinite threshold."""
        params = [p for g in self.optimizer.param_groups for p in g["params"] if p.grad is not None]
        max_norm = self.gradient_clip_val if self.gradient_clip_val > 0.0 else float("inf")
        return torch.nn.utils.clip_grad_norm_(params, max_norm)

    def _log_grad_norm(self, model, norm, step, extra=None, more=None):
        """`train/grad_norm` of optimizer step `step` (and `more`: the learning rates) through the model's log_dict (with `extra`,
        or else with what the model logged last): called at the steps where the loss is read on the host already."""
        more = dict(more or {})
        if norm is not None:
            norm = float(norm)
            self.logged_grad_norm.append((step, norm))
            more["train/grad_norm"] = norm
        if more and callable(getattr(model, "log_dict", None)):
            prev = extra if extra is not None else getattr(model, "last_logged", None)
            model.log_dict({**(prev if isinstance(prev, dict) else {}), **more})

    # ------------------------------------------------------------------ the loop, optimizer step as hipGraph replays
    def _make_graph_step(self, model, tensors):
        """The step object of `_fit_graphed`: nothing run, nothing captured yet."""
        from ctrlora_amd.train import GraphedTrainStep
        o = self._graph_opts
        acc = self.accumulate_grad_batches
        return GraphedTrainStep(model, self.optimizer, *tensors, warmup=0, capture=False, accumulate=acc > 1, grad_scale=1.0 / acc,
                                split_graphs=o.get("split_graphs"), bucket_bytes=o.get("bucket_bytes", 32 << 20),
                                reduce_fn=o.get("reduce_fn"))

    @torch.no_grad()
    def _graph_inputs(self, model, batch):
        """Everything of a micro-step that is NOT replayed, in the eager path's order: get_input (first stage or cached
        posteriors: CPU-generator draws, target first; text encoder), the hint latent (second CPU-generator draw), then t and the
        q_sample noise on the device generator with LatentDiffusion.forward's and p_losses' own calls -- one seed, one stream of
        numbers in both modes."""
        z, cond = model.get_input(batch, model.first_stage_key)
        hint = model._hint_latent(cond)
        cc = cond["c_crossattn"]
        ctx = cc[0] if len(cc) == 1 else torch.cat(cc, 1)
        t = torch.randint(0, model.num_timesteps, (z.shape[0],), device=model.device).long()
        noise = torch.randn_like(z)
        return z, ctx, hint, t, noise

    def _fit_graphed(self, model, train_dataloader):
        """`fit` with graph_step on.  Per micro-batch: `_graph_inputs` outside any capture, then the forward + loss + backward
        (and, on the last micro-batch of an optimizer step, the gradient exchange and AdamW + re-pack) through the step object.

        No batch is spent on warm-up: the first `warm_steps` (default 2) optimizer steps of this fit launch eagerly on the same
        direct path, each micro-step on its own batch; the graphs are captured (capturing executes nothing) before the next one
        and replayed from there on.  A batch whose tensor shapes are not the captured ones is launched eagerly too, and counted:
        `graph_eager_steps` / `graph_replays` count optimizer steps.  Accumulation (Lightning 1.5): the first micro-step clears
        the gradients, every micro-step's gradient is scaled by 1 / acc, the exchange and the optimizer follow the last one.
        The host is not synchronized here beyond what the eager loop does (log_dict, the logged loss)."""
        acc = self.accumulate_grad_batches
        warm = max(0, int(self._graph_opts.get("warm_steps", 2)))
        step = None
        micro = steps_here = 0
        launched_eagerly = False
        while self.global_step < self.max_steps:
            sampler = getattr(train_dataloader, "sampler", None)
            if hasattr(sampler, "set_epoch"):
                sampler.set_epoch(self.current_epoch)
            seen = 0
            for batch_idx, batch in enumerate(train_dataloader):
                seen += 1
                first, last = micro % acc == 0, (micro + 1) % acc == 0
                tensors = self._graph_inputs(model, batch)
                if step is None:
                    step = self._graph_step_obj = self._make_graph_step(model, tensors)
                    self.graph_mode = "one" if step.mode == "one" else "segmented"
                if first and not step.captured and steps_here >= warm and step.matches(*tensors):
                    step.capture()
                replay = step.captured and step.matches(*tensors)
                loss3 = (step.micro if replay else step.eager)(*tensors, first=first, last=last)
                launched_eagerly |= not replay
                micro += 1
                loss3 = loss3.clone()                   # a replay overwrites its output: callbacks may keep theirs
                loss = loss3[2]
                losses = {"train/loss_simple": loss3[0], "train/loss_vlb": loss3[1], "train/loss": loss}
                log = last and (self.global_step + 1) % self.log_every_n_steps == 0
                lr_logs = self._step_lr(model, self.global_step + 1, log) if last else {}
                if log and (self._norm_in_opt or lr_logs):
                    self._log_grad_norm(model, self.optimizer.last_grad_norm()[0] if self._norm_in_opt else None,
                                        self.global_step + 1, extra=losses, more=lr_logs)
                else:
                    model.log_dict(losses)
                if last:
                    self.global_step += 1
                    steps_here += 1
                    model.global_step = self.global_step
                    if launched_eagerly:
                        self.graph_eager_steps += 1
                    else:
                        self.graph_replays += 1
                    launched_eagerly = False
                    if self.is_global_zero and self.global_step % self.log_every_n_steps == 0:
                        self.logged.append((self.global_step, float(loss)))
                        print(f"[trainer] step {self.global_step} epoch {self.current_epoch} loss {float(loss):.5f}")
                    self._after_optimizer_step(model)
                self._call("on_train_batch_end", model, {"loss": loss}, batch, batch_idx)
                self._call("on_batch_end", model)
                if self.global_step >= self.max_steps:
                    break
            if seen == 0:
                raise RuntimeError("empty dataloader")
            self.current_epoch += 1
            model.current_epoch = self.current_epoch

    # ------------------------------------------------------------------ validation by timestep band; training-side bands
    def _check_validation_options(self, model, val_dataloaders):
        """The refusals, before anything is built or moved."""
        if self.val_check_interval > 0 and val_dataloaders is None:
            raise ValueError(f"val_check_interval={self.val_check_interval} without val_dataloaders: there is nothing to validate on")
        wants = (self.val_check_interval > 0 and val_dataloaders is not None) or self.loss_bands > 0
        why = validation_refusal(model) if wants else None
        if why is not None:
            raise ValueError("validation / loss_bands refused: " + why)
        if self.val_ema and getattr(model, "model_ema", None) is None:
            raise ValueError("val_ema without an EMA of the trained weights (use_ema / --ema_decay): there is no second set of "
                             "weights to validate")
        if (self.val_ema or self.save_best) and not (self.val_check_interval > 0 and val_dataloaders is not None):
            raise ValueError("val_ema / save_best need validation: val_check_interval > 0 and val_dataloaders")

    def _set_up_validation(self, model, val_dataloaders):
        """After the optimizer exists: which path a validation run takes, the plan, the training-side band table."""
        from ctrlora_amd import validation as V
        from ctrlora_amd.train import _FlatAdamW
        engine_opt = isinstance(self.optimizer, _FlatAdamW) and self.device.type == "cuda"
        self._val_on = self.val_check_interval > 0 and val_dataloaders is not None
        self._val_loader, self._val_step, self._val_last_step = val_dataloaders, None, -1
        if self._val_on:
            if isinstance(val_dataloaders, (list, tuple)) and val_dataloaders and hasattr(val_dataloaders[0], "dataset"):
                if len(val_dataloaders) != 1:
                    raise ValueError(f"{len(val_dataloaders)} validation dataloaders: this loop validates on one set")
                self._val_loader = val_dataloaders[0]
            if self.val_plan is None:
                self.val_plan = V.ValPlan(model.num_timesteps)
            if self.val_plan.num_timesteps != model.num_timesteps:
                raise ValueError(f"val_plan is laid out for {self.val_plan.num_timesteps} timesteps, the model has {model.num_timesteps}")
            # the engine path (cl_loss_bands behind engine_eval_step) needs the engine's optimizer to own the weights; any other
            # set-up runs the same loop through apply_model and the host restatement
            self._val_on_engine = engine_opt and V.engine_eval_refusal(model, self.device) is None
            if self._val_on_engine and self.graph_step:
                self._val_step = V.GraphedEvalStep(model, self.val_plan.nbands)
        self._train_bands = None
        if self.loss_bands > 0:
            if not engine_opt or not hasattr(type(model), "train_loss_bands"):
                raise ValueError("loss_bands refused: the table is filled by the engine's loss kernels inside the training step (a "
                                 "GPU, an engine optimizer and a model with p_losses on the engine)")
            from ctrlora_amd.train import LossBands
            self._train_bands = model.train_loss_bands = LossBands(model.num_timesteps, self.loss_bands, self.device)

    def _after_optimizer_step(self, model):
        """Right after optimizer step `global_step` was counted and logged: the interval's training bands, a validation run."""
        if self._train_bands is not None and self.global_step % self.log_every_n_steps == 0:
            self._log_train_bands(model)
        if self._val_on and self.global_step % self.val_check_interval == 0:
            self._validate(model)

    def _log_train_bands(self, model):
        """`train/loss_simple/t{lo}-{hi}`: the mean of this rank's per-sample training losses per timestep band since the last
        read (rank-local: no exchange), read and cleared where the loss is read on the host already."""
        from ctrlora_amd import validation as V
        tab = self._train_bands.read_and_clear()
        self.logged_train_bands.append((self.global_step, tab))
        labels = [f"t{lo}-{hi}" for lo, hi in V.band_ranges(self._train_bands.num_timesteps, self._train_bands.nbands)]
        logs = {f"train/loss_simple/{lab}": float(row[1] / row[0]) for lab, row in zip(labels, tab) if float(row[0]) > 0}
        if callable(getattr(model, "log_dict", None)):
            prev = getattr(model, "last_logged", None)
            model.log_dict({**(prev if isinstance(prev, dict) else {}), **logs})
        return logs

    def _validate(self, model):
        """One validation run (ctrlora_amd.validation): the live weights, with val_ema the EMA weights inside ema_scope() into a
        second table; the tables are exchanged over the ranks and read ONCE; logged through model.log_dict, into `logged_val`
        and as one JSON line of <log_dir>/val_log.jsonl; with save_best, best.ckpt when the monitored loss improved."""
        from ctrlora_amd import validation as V
        plan = self.val_plan
        self._call("on_validation_start", model)
        kw = dict(step=self._val_step, limit_batches=self.limit_val_batches, rank=self.global_rank, world=self.world_size,
                  on_engine=self._val_on_engine, device=self.device)
        tabs = [V.run_validation(model, self._val_loader, plan, **kw)]
        if self.val_ema:
            with model.ema_scope():
                tabs.append(V.run_validation(model, self._val_loader, plan, **kw))
        both = torch.stack(tabs)
        if self.world_size > 1:
            import torch.distributed as dist
            if dist.get_backend() == "nccl":
                both = both.to(self.device)
            both = V.reduce_tables(both, self.world_size)
        both = both.cpu()                      # the one read of a run
        self.val_tables = both
        logs = V.table_logs(both[0], plan)
        if self.val_ema:
            logs.update(V.table_logs(both[1], plan, suffix="_ema"))
        self._val_last_step = self.global_step
        self.logged_val.append((self.global_step, logs))
        if callable(getattr(model, "log_dict", None)):
            model.log_dict(logs)
        if self.is_global_zero:
            import math
            row = {"global_step": self.global_step, "epoch": self.current_epoch}
            row.update({k: (v if math.isfinite(v) else None) for k, v in logs.items()})
            V.append_jsonl(os.path.join(self.log_dir, "val_log.jsonl"), row)
            print(f"[trainer] step {self.global_step} val/loss_simple {logs['val/loss_simple']:.5f} "
                  f"+- {logs['val/loss_simple_se']:.5f}" +
                  (f"  ema {logs['val/loss_simple_ema']:.5f}" if self.val_ema else ""))
        if self.save_best:
            monitored = logs["val/loss_simple_ema" if self.val_ema else "val/loss_simple"]
            if monitored < self.best_val:
                self.best_val = monitored
                self.save_checkpoint(os.path.join(self.checkpoint_callback.dirpath, "best.ckpt"))
        self._call("on_validation_end", model)
        return logs
