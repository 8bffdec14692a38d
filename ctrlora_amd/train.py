"""Training glue between torch.autograd / torch.optim and the HIP engine.

  * ApplyModelFn   -- one autograd node for the whole ControlNet+UNet pass: forward records,
                      backward runs the hand-written backward and fills the flat fp32 gradient buffers
                      (the trainable nn.Parameters' .grad are views of those buffers).
  * PLossFn        -- p_losses' reduction {loss_simple, loss_vlb, loss} + d loss / d eps, one deterministic kernel pair
                      (ddpm.py:902-918 with logvar = 0).
  * FusedAdamW     -- torch.optim.AdamW semantics (cldm_ctrlora_finetune.py:105) as ONE kernel over the
                      flat master/grad buffers, followed by the re-pack of the trainables; with `attach_ema()` the EMA of
                      the trained weights (ldm/modules/ema.py) is one more kernel per bank inside the same step.  torch's
                      parameter groups (up to 8: cl_adamw_dev_groups, still one launch per bank) and a learning-rate curve kept
                      in device memory (`set_lr_schedule`: cl_lr_schedule inside the step) are part of the same step.
  * PretrainAdamW  -- the same over the base buffer and every LoRA bank that has joined (both: _FlatAdamW + _AdamState).
  * bind_trainables -- re-points the ControlNet's trainable nn.Parameters at the flat buffers.
  * GraphedTrainStep -- the optimizer step as hipGraph replays of the pieces capture_plan() lists.
"""
from __future__ import annotations

from functools import partial
from typing import List, NamedTuple, Sequence

import torch

from . import hip


def bind_trainables(module: torch.nn.Module, executor) -> List[torch.nn.Parameter]:
    """After this, optimizer updates on the module's trainable Parameters update the engine's fp32
    masters in place, and the engine's backward fills their .grad."""
    params = dict(module.named_parameters())
    out = []
    for t in executor.tr.items:
        p = params[t.name]
        p.data = t.param_view(t.master)        # conv weights: a permuted view of the [O][9][I] master storage
        p.grad = t.param_view(t.grad)
        p.requires_grad_(True)
        out.append(p)
    return out


def bind_bank(params_by_name, bank) -> List[torch.nn.Parameter]:
    """Point one LoRA bank's nn.Parameters (name -> Parameter, names as in the bank's TrainableSet) at its flat buffers."""
    out = []
    for t in bank.items:
        p = params_by_name[t.name]
        p.data = t.master
        p.grad = t.grad
        p.requires_grad_(True)
        out.append(p)
    return out


def trainables_version(params: Sequence[torch.nn.Parameter]) -> int:
    return sum(p._version for p in params)


class ApplyModelFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, engine, x_noisy, t, context, hints, scales, weights, only_mid, on_backward):
        ctx.engine, ctx.on_backward = engine, on_backward
        return engine.forward(x_noisy, t, context, hints, control_scales=scales, lora_weights=weights, record=True,
                              only_mid_control=only_mid)

    @staticmethod
    def backward(ctx, d_eps):
        ctx.engine.backward(d_eps)
        if ctx.on_backward is not None:
            ctx.on_backward()
        return (None,) * 10


def p_losses_launch(eps, target, t, lvlb, grad_scale, w_simple, w_elbo, wt=None, kind=0, delta=1.0, bands=None):
    """The p_losses reduction of one step, for PLossFn and engine_train_step: allocates the 3-vector {loss_simple, loss_vlb,
    loss}, the kernels' scratch (16 floats per sample) and d loss / d eps (times `grad_scale`), and launches cl_p_losses_mse
    when there is no weight table and the loss is l2, cl_p_losses_w otherwise.  `eps` is fp32 and contiguous.  Returns
    (out, d_eps).  `bands` (None = the launches above and nothing else): a `LossBands` whose table takes the step's per-sample
    losses by timestep band, one cl_loss_bands launch more."""
    target, t = target.float().contiguous(), t.long().contiguous()
    out = torch.empty(3, dtype=torch.float32, device=eps.device)
    scratch = torch.empty(16 * eps.shape[0], dtype=torch.float32, device=eps.device)
    d_eps = torch.empty_like(eps)
    per = None if bands is None else torch.empty(eps.shape[0], dtype=torch.float32, device=eps.device)
    if wt is None and kind == 0:
        hip.p_losses_mse(eps, target, d_eps, t, lvlb, out, scratch, float(grad_scale), float(w_simple), float(w_elbo), per_sample=per)
    else:
        hip.p_losses_w(eps, target, d_eps, t, lvlb, out, scratch, float(grad_scale), float(w_simple), float(w_elbo),
                       per_sample=per, wt=wt, kind=kind, delta=delta)
    if bands is not None:
        hip.loss_bands(per, t, bands.num_timesteps, bands.nbands, bands.acc)
        bands.last = (per, t)
    return out, d_eps


class LossBands:
    """Training-side telemetry (Trainer(loss_bands=N)): a device fp64 table [nbands + 1][3] that every p_losses launch of a
    training step adds its per-sample losses to (cl_loss_bands), inside the captured step where there is one.  `last` = the
    (per_sample, t) device tensors of the latest launch; after a replay they hold that replay's values.  Rank-local."""

    def __init__(self, num_timesteps, nbands, device):
        self.num_timesteps, self.nbands = int(num_timesteps), int(nbands)
        self.acc = hip.zero_(torch.empty(self.nbands + 1, 3, dtype=torch.float64, device=device))
        self.last = None

    def read_and_clear(self):
        tab = self.acc.cpu()
        hip.zero_(self.acc)
        return tab


class PLossFn(torch.autograd.Function):
    """LatentDiffusion.p_losses' reduction (ddpm.py:902-918 with logvar = 0) as ONE deterministic HIP reduction:
    returns the 3-vector {loss_simple, loss_vlb, loss = w_simple * loss_simple + w_elbo * loss_vlb} and keeps
    d(w_simple * loss_simple) / d eps for the backward (the elbo term is not differentiated; its weight is 0 in
    every CtrLoRA config and the caller checks that).  `wt` (a per-timestep weight table, e.g. Min-SNR-gamma) and `kind` 1
    (Huber with `delta`) go through cl_p_losses_w; without either the call is cl_p_losses_mse (p_losses_launch)."""

    @staticmethod
    def forward(ctx, eps, target, t, lvlb, w_simple, w_elbo, wt=None, kind=0, delta=1.0, bands=None):
        out, d_eps = p_losses_launch(eps.float().contiguous(), target, t, lvlb, 1.0, w_simple, w_elbo, wt, kind, delta, bands)
        ctx.save_for_backward(d_eps)
        return out

    @staticmethod
    def backward(ctx, g):
        (d_eps,) = ctx.saved_tensors
        return d_eps * g[2], None, None, None, None, None, None, None, None, None


class _AdamState:
    """The Adam state of ONE TrainableSet: the flat moments `m`, `v` (in the order of `ts.flat`) and a device step counter --
    its own, or one handed in that several states share.  `legacy(src)` is the owning optimizer's rule for a moment saved as
    one flat tensor: it returns the [(offset here, offset in src, numel)] to copy, or raises."""

    def __init__(self, ts, step=None, legacy=None):
        self.ts, self.legacy = ts, legacy
        self.m, self.v = torch.zeros_like(ts.flat), torch.zeros_like(ts.flat)
        self.step = torch.zeros(1, dtype=torch.int32, device=ts.flat.device) if step is None else step

    def __getitem__(self, key):          # state["m" | "v" | "step"]
        return getattr(self, key)

    def _by_name(self, buf):
        return ((t.name, buf[t.offset:t.offset + t.master.numel()]) for t in self.ts.items)

    def export(self):
        """Moments BY PARAMETER NAME: the order of the flat buffers is an implementation detail of a build / dtype (the bf16
        engine keeps the grouped emb_layers factors at the tail, nets.py), a checkpoint must not depend on it."""
        return dict(m={n: x.clone() for n, x in self._by_name(self.m)}, v={n: x.clone() for n, x in self._by_name(self.v)},
                    step=int(self.step.item()))

    def check(self, src, allow_surplus):
        """Raise if `src` = {m, v, step} cannot be loaded; nothing is written."""
        int(src["step"])
        for key in ("m", "v"):
            if not isinstance(src[key], dict):
                self.legacy(src[key])
                continue
            missing = [t.name for t in self.ts.items if t.name not in src[key]]
            if missing:
                raise KeyError(f"optimizer state lacks {len(missing)} tensors, e.g. {missing[:3]}")
            surplus = [] if allow_surplus else sorted(set(src[key]) - set(self.ts.by_name))
            if surplus:
                raise KeyError(f"optimizer state holds {len(surplus)} tensors this model does not train, "
                               f"e.g. {surplus[:3]} (norm_trainable / zero_trainable differ from the checkpoint's?)")

    def load(self, src):
        """Copy a checked `src` in."""
        for key in ("m", "v"):
            dst, saved = self[key], src[key]
            if isinstance(saved, dict):
                for name, x in self._by_name(dst):
                    x.copy_(saved[name].reshape(-1))
            else:
                saved = saved.reshape(-1)
                for here, there, k in self.legacy(saved):
                    dst[here:here + k].copy_(saved[there:there + k])
        self.step.fill_(int(src["step"]))


def _load_states(pairs):
    """[(state, src, allow_surplus)]: every check before the first copy, so a refused state dict leaves the optimizer -- step
    counters included -- as it was (e.g. a resume under other norm_trainable / zero_trainable flags)."""
    for st, src, allow_surplus in pairs:
        st.check(src, allow_surplus)
    for st, src, _ in pairs:
        st.load(src)


def _legacy_rounds_1_3(ex, src):
    """FusedAdamW: a flat moment tensor saved by rounds 1-3.  Those builds laid the trainables out in `ex.legacy_item_names`
    order (backward-completion order without the emb_layers hoist), every tensor padded to 64 floats
    (packing.TrainableSet.materialize); the tensors are found by walking that order and go to today's offsets."""
    from .engine.packing import rup
    names = getattr(ex, "legacy_item_names", None) or [t.name for t in ex.tr.items]
    by_name = {t.name: t for t in ex.tr.items}
    if sorted(names) != sorted(by_name):
        raise KeyError("the legacy optimizer state does not describe this model's trainable set")
    off, spans = 0, []
    for n in names:
        k = by_name[n].master.numel()
        spans.append((by_name[n].offset, off, k))
        off += rup(k, 64)
    if off != src.numel():
        raise ValueError(f"legacy optimizer state holds {src.numel()} floats, the legacy layout of this model has {off}")
    return spans


def _legacy_format_1(ts, src):
    """PretrainAdamW format 1 (rounds 2-4): the raw flat buffer; only valid for an unchanged layout -- check what can be."""
    if src.numel() != ts.flat.numel():
        raise ValueError(f"flat optimizer state of {src.numel()} floats does not fit this build's {ts.flat.numel()}")
    return [(0, 0, src.numel())]


def build_chunk_group(items, numel, group_of, ngroups):
    """The uint8 map cl_adamw_dev_groups reads, on the host: entry c = the group of elements [64 c, 64 c + 64) of a flat buffer
    of `numel` floats laid out by packing.TrainableSet.materialize (every tensor starts on a 64-float boundary and owns its
    padding).  `items`: the Trainables, `group_of`: name -> group index.  Refuses what the kernel would have to clamp."""
    from .engine.packing import rup
    if not 1 <= ngroups <= hip.ADAMW_MAX_GROUPS:
        raise ValueError(f"{ngroups} parameter groups: the grouped AdamW launch takes 1 to {hip.ADAMW_MAX_GROUPS}")
    if numel % hip.ADAMW_CHUNK:
        raise ValueError(f"a flat buffer of {numel} floats is not a whole number of {hip.ADAMW_CHUNK}-float chunks")
    out = torch.zeros(numel // hip.ADAMW_CHUNK, dtype=torch.uint8)
    for t in items:
        if t.name not in group_of:
            raise ValueError(f"trainable tensor '{t.name}' is in no parameter group")
        k, n = int(group_of[t.name]), 1
        for s in t.shape:
            n *= s
        if not 0 <= k < ngroups:
            raise ValueError(f"'{t.name}' names group {k}, the table has {ngroups}")
        if t.offset % hip.ADAMW_CHUNK or t.offset + rup(n, hip.ADAMW_CHUNK) > numel:
            raise ValueError(f"'{t.name}' at offset {t.offset} ({n} floats) does not sit on whole chunks of the flat buffer")
        out[t.offset // hip.ADAMW_CHUNK:(t.offset + rup(n, hip.ADAMW_CHUNK)) // hip.ADAMW_CHUNK] = k
    return out


class _FlatAdamW(torch.optim.Optimizer):
    """What the two optimizers over the engine's flat buffers share; a subclass launches its kernels in `_update()` and
    `zero_grad()`.  `params` are the bound nn.Parameters (kept in param_groups for scheduler / checkpoint compatibility); step
    counts and hyper-parameters live in DEVICE memory (cl_adamw_dev), so that `step()` can be captured in a hipGraph and
    replayed.

    Parameter groups: `params` may be torch's list of group dicts (up to 8; an optional "name" each).  The hyper-parameters are a
    [G, 6] device table, one row {lr, beta1, beta2, eps, weight_decay, grad_scale} per group; `_hyper` is row 0 (the whole table
    of a one-group optimizer, as before).  `sync_hyper()` (automatic outside capture) pushes every row that changed on the host.
    `grad_scale` is common to all groups.  What a subclass launches with more than one group is its own business (FusedAdamW:
    cl_adamw_dev_groups); with one group nothing changes.

    Learning-rate schedule: a host scheduler that moves `param_groups[k]["lr"]` reaches the device with the next `sync_hyper()`,
    a host-to-device copy between replays.  `set_lr_schedule(table)` keeps the whole curve in device memory instead: an fp32
    [T, G] table whose row `step - 1` cl_lr_schedule writes into the lr column right after the step's cl_tick, inside the captured
    step.  While a table is set the device owns the lr column (`sync_hyper()` leaves it alone) and `param_groups[k]["lr"]` is a
    mirror for logs and checkpoints; `last_lr()` is the column itself.  Setting or dropping a table changes what is launched: do
    it before a capture, not after (refused); copying new values into a table of the same shape is allowed between replays.

    Global gradient norm (torch.nn.utils.clip_grad_norm_ with norm_type 2, on the device): `max_grad_norm` (None or <= 0: off)
    clips, `track_grad_norm` measures without clipping.  With either on, `_update()` opens with cl_grad_norm over the buffers the
    step updates and runs cl_adamw_dev_clip in place of cl_adamw_dev; `last_grad_norm()` returns (norm, coef) as device tensors.
    The threshold lives in device memory and follows `sync_hyper()`'s rule, so a schedule may move it between replays.  Turning
    the feature on or off changes what is launched: do it before a capture, not after.  With both off nothing changes."""

    def __init__(self, params, device, lr, betas, eps, weight_decay, grad_scale):
        super().__init__(list(params), dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        G = len(self.param_groups)
        if G > hip.ADAMW_MAX_GROUPS:
            raise ValueError(f"{G} parameter groups: the device table holds at most {hip.ADAMW_MAX_GROUPS}")
        if G > 1:
            for k, g in enumerate(self.param_groups):
                g.setdefault("name", "default" if k == 0 else f"group{k}")
            names = self.group_names
            if len(set(names)) != G:
                raise ValueError(f"parameter groups need distinct names, got {names}")
        self.grad_scale = grad_scale
        self._hyper_table = torch.zeros(G, 6, dtype=torch.float32, device=device)
        self._hyper = self._hyper_table[0]        # group 0's row: the table of a one-group optimizer, and grad_scale for cl_grad_norm
        self._hyper_host = [None] * G
        self._lr_table = None         # set_lr_schedule: fp32 [T, G] in device memory
        self._captured = False        # a capture has recorded this optimizer's launches
        self.max_grad_norm, self.track_grad_norm = None, False
        self._max_norm = torch.zeros(1, dtype=torch.float32, device=device)      # the threshold; 0 = tracking only
        self._max_norm_host = 0.0
        self.grad_norm_out = torch.tensor([0.0, 1.0], dtype=torch.float32, device=device)     # {norm, coef} of the last step
        self._norm_scratch = None
        self.pre_step_hook = None     # e.g. DP: wait for the gradient all-reduce
        self.sync_hyper()

    @property
    def group_names(self):
        return [g.get("name", "default") for g in self.param_groups]

    def sync_hyper(self):
        """Push every group's {lr, betas, eps, weight_decay, grad_scale} to the device if they changed (host -> device copy:
        call it OUTSIDE graph capture / between replays).  With a device schedule set the lr column is the device's."""
        scheduled = self._lr_table is not None
        for k, g in enumerate(self.param_groups):
            cur = (float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]),
                   float(self.grad_scale))
            old = self._hyper_host[k]
            if scheduled and old is not None:
                if cur[1:] != old[1:]:
                    self._hyper_table[k, 1:].copy_(torch.tensor(cur[1:], dtype=torch.float32))
                self._hyper_host[k] = (old[0],) + cur[1:]         # old[0]: the last lr the HOST wrote
            elif cur != old:
                self._hyper_table[k].copy_(torch.tensor(cur, dtype=torch.float32))
                self._hyper_host[k] = cur
        mx = float(self.max_grad_norm) if self.max_grad_norm is not None and self.max_grad_norm > 0 else 0.0
        if mx != self._max_norm_host:
            self._max_norm.copy_(torch.tensor([mx], dtype=torch.float32))
            self._max_norm_host = mx
        if self.norm_enabled and self._norm_scratch is None:      # allocated here: never inside a capture
            self._norm_scratch = torch.empty(hip.grad_norm_scratch_floats(), dtype=torch.float32, device=self._hyper.device)

    def set_lr_schedule(self, table):
        """Keep the learning-rate curve in device memory: `table` is fp32 [T, G] (row s - 1 = the groups' lr of optimizer step s,
        the last row holds beyond T; `ctrlora_amd.lr_schedule.compile_lambda_lr` makes one from a LambdaLR), or [T], the same lr
        for every group, or None = no device schedule (the host's `param_groups[k]["lr"]` goes back to the device).  A table of
        the shape already set is copied into the same tensor, which a captured step keeps reading."""
        G = len(self.param_groups)
        if table is None:
            if self._lr_table is None:
                return
            if self._captured:
                raise RuntimeError("set_lr_schedule(None) after a capture: the captured step launches cl_lr_schedule; drop the "
                                   "schedule before capturing")
            self._lr_table = None
            self._hyper_host = [None] * G
            self.sync_hyper()
            return
        t = torch.as_tensor(table, dtype=torch.float32).detach()
        if t.dim() == 1:
            t = t[:, None].expand(t.shape[0], G)
        if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] != G:
            raise ValueError(f"a learning-rate table is [T] or [T, {G}] (one column per parameter group) with T >= 1, got "
                             f"{tuple(t.shape)}")
        if self._lr_table is not None and self._lr_table.shape == t.shape:
            self._lr_table.copy_(t)
            return
        if self._captured:
            raise RuntimeError("set_lr_schedule after a capture: " + ("the captured step holds the address and length of the table "
                               "it was recorded with; only a table of the same shape can replace its values" if self._lr_table
                               is not None else "the captured step does not launch cl_lr_schedule; set the schedule before capturing"))
        self._lr_table = t.to(self._hyper_table.device).contiguous().clone()

    def last_lr(self):
        """The groups' learning rates as the device has them (a view of the table's lr column; no synchronization)."""
        return self._hyper_table[:, 0]

    def _tick_and_schedule(self, step):
        """One tick of `step` and, with a device schedule, this step's learning rates, before any AdamW launch."""
        hip.tick(step)
        if self._lr_table is not None:
            hip.lr_schedule(self._hyper_table, self._lr_table, step)

    @property
    def norm_enabled(self) -> bool:
        return bool(self.track_grad_norm) or (self.max_grad_norm is not None and self.max_grad_norm > 0)

    def last_grad_norm(self):
        """(norm, coef) of the last step as device tensors (views of `grad_norm_out`; no synchronization): the norm of
        grad_scale x the gradient before clipping, and the factor the step applied (1 when it did not clip)."""
        return self.grad_norm_out[0], self.grad_norm_out[1]

    def _grad_norm(self, bufs) -> bool:
        """Opens `_update()`: with the norm on, launch cl_grad_norm over `bufs` into `grad_norm_out` and return True."""
        if not self.norm_enabled:
            return False
        if len(bufs) > hip.GRAD_NORM_MAX_BUFS:
            raise ValueError(f"the gradient norm covers at most {hip.GRAD_NORM_MAX_BUFS} flat buffers, the step has {len(bufs)}")
        assert self._norm_scratch is not None, "sync_hyper() has not run since the gradient norm was turned on"
        hip.grad_norm(bufs, self._hyper, self._max_norm, self.grad_norm_out, self._norm_scratch)
        return True

    def _adamw(self, flat, grad, st, step, clip, chunk_group=None):
        """The update of ONE flat buffer with the state `st` and the device counter `step`: the one place that picks the entry
        point -- a chunk map: cl_adamw_dev_groups, else `clip` (what `_grad_norm()` returned): cl_adamw_dev_clip, else
        cl_adamw_dev."""
        if chunk_group is not None:
            hip.adamw_dev_groups(flat, grad, st.m, st.v, self._hyper_table, chunk_group, step, self.grad_norm_out if clip else None)
        elif clip:
            hip.adamw_dev_clip(flat, grad, st.m, st.v, self._hyper, step, self.grad_norm_out)
        else:
            hip.adamw_dev(flat, grad, st.m, st.v, self._hyper, step)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        if self.pre_step_hook is not None:
            self.pre_step_hook()
        if not torch.cuda.is_available() or not torch.cuda.is_current_stream_capturing():
            self.sync_hyper()
        else:
            self._captured = True         # from here on what `_update()` launches is fixed (set_lr_schedule)
        self._update()
        return loss

    def _saved_param_groups(self):
        return [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]

    def _check_group_structure(self, sd):
        """Raise if `sd` was saved under other parameter groups; nothing is written."""
        saved = [g.get("name", "default") for g in (sd.get("param_groups") or [{}])]
        if saved != self.group_names:
            raise ValueError(f"optimizer state was saved with the parameter groups {saved}, this optimizer has "
                             f"{self.group_names}: resume with the group options of the run that wrote it")

    def _restore_param_groups(self, sd):
        """Resume: the saved hyper-parameters (a scheduler may have moved lr) replace the constructor's, then go to the device
        (under a device schedule the lr is a mirror only: the restored step counter puts the device back on the curve)."""
        for g, saved in zip(self.param_groups, sd.get("param_groups") or []):
            for k, v in saved.items():
                if k != "params":
                    g[k] = v
        self.sync_hyper()


class FusedAdamW(_FlatAdamW):
    """AdamW over the engine's flat buffers for fine-tuning: one HIP kernel per ControlNet bank, all banks on ONE step
    counter, each followed by the re-pack of its trainables.  With more than one parameter group (`params` a list of group
    dicts, e.g. LoRA+'s higher lr for the up matrices, no weight decay on norms and biases) the kernel is cl_adamw_dev_groups:
    still one launch per bank, every 64-float chunk of the flat buffer under its own group's row (`_chunk_group`, one uint8 map
    per bank, built here from the bank's offsets and the groups the bound parameters were put in)."""

    def __init__(self, params, executors, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale: float = 1.0):
        self.executors = list(executors)
        dev = self.executors[0].tr.flat.device
        super().__init__(params, dev, lr, betas, eps, weight_decay, grad_scale)
        self._step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self._states = [_AdamState(ex.tr, self._step_dev, partial(_legacy_rounds_1_3, ex)) for ex in self.executors]
        self.ema, self._ema_flats = None, None
        self._chunk_group = self._build_chunk_groups() if len(self.param_groups) > 1 else None

    def _build_chunk_groups(self):
        """One chunk -> group map per bank, in device memory (allocated here: never inside a capture).  A bound parameter is a
        view of its tensor's master storage (bind_trainables), so the storage address says which tensor a parameter is."""
        group_at = {}
        for k, g in enumerate(self.param_groups):
            for p in g["params"]:
                group_at[p.data_ptr()] = k        # torch has refused a parameter in two groups already
        maps = []
        for ex in self.executors:
            missing = [t.name for t in ex.tr.items if t.master.data_ptr() not in group_at]
            if missing:
                raise ValueError(f"{len(missing)} trainable tensors are in no parameter group, e.g. {missing[:3]}")
            group_of = {t.name: group_at[t.master.data_ptr()] for t in ex.tr.items}
            cg = build_chunk_group(ex.tr.items, ex.tr.flat.numel(), group_of, len(self.param_groups))
            maps.append(cg.to(ex.tr.flat.device))
        return maps

    def attach_ema(self, ema, flats):
        """EMA of the trained weights inside the step (ldm.modules.ema.ModelEma bound to the executors; `flats`: its flat shadow
        buffer per bank, laid out like that bank's masters).  From here on `_update()` ticks `ema.num_updates` once per optimizer
        step and follows every bank's AdamW launch with cl_ema_update on the updated masters -- after the last accumulation
        micro-step and after the gradient exchange, like the rest of the step, so every rank computes the same shadows and
        nothing is exchanged.  `ema.decay` lives in device memory and follows `sync_hyper()`'s rule (ModelEma.set_decay).
        Attaching changes what is launched: do it before a capture, not after.  Without it nothing changes."""
        flats = list(flats)
        assert len(flats) == len(self.executors)
        for ex, f in zip(self.executors, flats):
            assert f.dtype == torch.float32 and f.shape == ex.tr.flat.shape and f.device == ex.tr.flat.device
        assert ema.decay.device == ema.num_updates.device == self._hyper.device
        self.ema, self._ema_flats = ema, flats
        self.sync_hyper()

    def sync_hyper(self):
        super().sync_hyper()
        if getattr(self, "ema", None) is not None:
            self.ema.sync()

    @torch.no_grad()
    def step(self, closure=None):
        if self.ema is not None and self.ema.in_scope:
            raise RuntimeError("opt.step() inside ema_scope(): the masters hold the EMA weights, a step would train the average "
                               "and average the result; leave the scope first")
        return super().step(closure)

    _step = property(lambda self: int(self._step_dev.item()))
    _m = property(lambda self: [st.m for st in self._states])
    _v = property(lambda self: [st.v for st in self._states])

    def _update(self):
        clip = self._grad_norm([ex.tr.flat_grad for ex in self.executors])
        self._tick_and_schedule(self._step_dev)     # one tick per optimizer step, however many banks follow; then this step's lr
        ema = self.ema
        if ema is not None and ema.use_num_updates:
            hip.tick(ema.num_updates)     # LitEma counts before it averages; without the warm-up the count stays at -1
        for k, (ex, st) in enumerate(zip(self.executors, self._states)):
            self._adamw(ex.tr.flat, ex.tr.flat_grad, st, self._step_dev, clip,
                        self._chunk_group[k] if self._chunk_group is not None else None)
            if ema is not None:
                hip.ema_update(self._ema_flats[k], ex.tr.flat, ema.decay, ema.num_updates)
            ex.repack()

    def zero_grad(self, set_to_none: bool = False):
        # .grad tensors are views of flat_grad: zero in place, they must stay attached
        for ex in self.executors:
            hip.zero_(ex.tr.flat_grad)

    def state_dict(self):
        saved = [st.export() for st in self._states]
        return dict(step=self._step, format="by_name", m=[s["m"] for s in saved], v=[s["v"] for s in saved],
                    param_groups=self._saved_param_groups())

    def load_state_dict(self, sd):
        assert len(sd["m"]) == len(self._states), "optimizer state was saved for a different number of ControlNet banks"
        self._check_group_structure(sd)
        _load_states([(st, dict(m=m, v=v, step=sd["step"]), False) for st, m, v in zip(self._states, sd["m"], sd["v"])])
        self._restore_param_groups(sd)


class PretrainAdamW(_FlatAdamW):
    """torch.optim.AdamW over ALL ControlNet parameters as the reference's multi-task pre-training uses it
    (cldm/cldm_ctrlora_pretrain.py:174-182, torch 1.13 / Lightning 1.5 semantics), on the engine's flat buffers:

      * the shared (base) parameters are updated every step;
      * a task's LoRA bank joins the update the first time it receives a gradient (before that its .grad is None and
        torch skips it); from then on it is updated EVERY step -- with a zero gradient when another task ran, because
        `optimizer.zero_grad()` of that torch version zero-fills instead of setting None: weight decay and the decaying
        first moment keep moving it.  Each bank therefore has its own step counter (bias correction).

    `mark_used(task)` is called by the model when a task's bank took part in a backward pass."""

    def __init__(self, params, executor, banks, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale=1.0):
        self.executor, self.executors, self.banks = executor, [executor], dict(banks)
        super().__init__(params, executor.tr.flat.device, lr, betas, eps, weight_decay, grad_scale)
        if len(self.param_groups) > 1:
            raise NotImplementedError("PretrainAdamW takes one parameter group: groups are built for fine-tuning only "
                                      "(FusedAdamW), as the EMA is")
        mk = lambda ts: _AdamState(ts, legacy=partial(_legacy_format_1, ts))
        self._base = mk(executor.tr)
        self._bank_state = {k: mk(ts) for k, ts in self.banks.items()}
        self.active = []                 # tasks whose bank has received a gradient at least once, in order of first use

    def set_lr_schedule(self, table):
        if table is not None:
            raise NotImplementedError("PretrainAdamW has no device learning-rate schedule: every bank counts its own steps; "
                                      "built for fine-tuning only (FusedAdamW), as the EMA is")

    def mark_used(self, task):
        if task not in self.active:
            self.active.append(task)

    _step = property(lambda self: int(self._base.step.item()))

    def _update(self):
        sets = [(self.executor.tr, self._base)] + [(self.banks[k], self._bank_state[k]) for k in self.active]
        # the norm runs over the parameters whose .grad is not None in the reference: the base and every active bank, an idle
        # one with its zero gradient
        clip = self._grad_norm([ts.flat_grad for ts, _ in sets])
        for ts, st in sets:
            hip.tick(st.step)
            self._adamw(ts.flat, ts.flat_grad, st, st.step, clip)
        self.executor.repack()

    def zero_grad(self, set_to_none: bool = False):
        hip.zero_(self.executor.tr.flat_grad)
        for task in self.active:
            hip.zero_(self.banks[task].flat_grad)

    def state_dict(self):
        """Format 2: moments by parameter name, like FusedAdamW."""
        return dict(format="by_name", version=2, base=self._base.export(),
                    banks={k: st.export() for k, st in self._bank_state.items()}, active=list(self.active),
                    param_groups=self._saved_param_groups())

    def load_state_dict(self, sd):
        if set(sd["banks"]) != set(self._bank_state):
            raise KeyError(f"optimizer state holds banks {sorted(sd['banks'])}, the model has {sorted(self._bank_state)}")
        active = list(sd["active"])
        _load_states([(self._base, sd["base"], True)] + [(self._bank_state[k], src, True) for k, src in sd["banks"].items()])
        self.active = active
        self._restore_param_groups(sd)


class Piece(NamedTuple):
    """One captured piece of an optimizer step (capture_plan)."""
    kind: str                 # "Z" = zero_grad, "F" = forward + loss + backward, "B" = opt.step()
    segmented: bool = False   # F: the stage-cut segment graphs instead of one graph
    tag: object = None        # F: what is exchanged after it -- None, "all", or "per-segment" (int tags, then "tails")
    zero: bool = False        # F: clears the gradients itself
    with_opt: bool = False    # F: opt.step() is captured inside the same graph (there is no B)


def capture_plan(mode: str, accumulate: bool) -> List[Piece]:
    """The pieces of one GraphedTrainStep in capture and replay order, always [Z] F [B]: Z iff `accumulate` (else F clears
    the gradients itself), B as a graph of its own except in ("one", no accumulation), where opt.step() closes F's graph."""
    tag = {"one": None, "two": "all", "segmented": "per-segment"}[mode]
    fused = mode == "one" and not accumulate
    f = Piece("F", segmented=mode == "segmented", tag=tag, zero=not accumulate, with_opt=fused)
    return ([Piece("Z")] if accumulate else []) + [f] + ([] if fused else [Piece("B")])


class _StaticInputs:
    """The five tensors (z, ctx, hint, t, noise) a captured step reads: clones made once, refilled before every replay."""

    def __init__(self, *tensors):
        self.tensors = tuple(x.clone() for x in tensors)

    def load(self, *tensors):
        for dst, src in zip(self.tensors, tensors):
            dst.copy_(src)

    def matches(self, *tensors) -> bool:
        return all(a.shape == b.shape and a.dtype == b.dtype for a, b in zip(tensors, self.tensors))


class GraphedTrainStep:
    """One optimizer step of LoRA fine-tuning as hipGraph replays.

    The eager step is ~1900 kernel launches driven from Python through ctypes; at ~40 ms per step the host
    becomes the bottleneck.  Everything in the step has static shapes and no host dependence (the optimizer's
    step counter and hyper-parameters are device-resident), so it is captured once and replayed.

    One rank:      ONE graph = zero_grad -> p_losses forward -> hand-written backward -> fused AdamW + re-pack.
    Data parallel: the backward is cut at ControlNet stage boundaries into SEGMENT graphs -- a new segment starts
                   whenever the gradient slice finalised so far (the flat buffer is laid out in backward-completion
                   order) has reached `bucket_bytes`:

        graph S0 : zero_grad, forward, UNet-decoder backward, ControlNet middle + deepest stages
        RCCL     : async all-reduce of flat_grad[bucket 0]            } runs on RCCL's stream while
        graph S1 : the next ControlNet stages                          } graph S1 is executing
        RCCL     : async all-reduce of flat_grad[bucket 1]  ...
        graph SN : remaining stages; then every rank waits for its collectives
        graph B  : fused AdamW (grad_scale = 1 / world) + re-pack

    so the LoRA-only gradient exchange overlaps the remaining backward as in the eager path, with collectives kept
    OUT of the captured regions.  `split_graphs`: None = segmented iff world > 1; "segmented" / True force that
    structure on one rank (tests); "two" = the old A | all-reduce | B form; False = one graph.
    `model` is a ControlFinetuneLDM-like module (engine_train_step or p_losses / dp / control_model), `opt` its
    FusedAdamW.

    For a training loop (ctrlora_amd.trainer.Trainer): `warmup=0, capture=False` builds the object without
    running or capturing anything, `eager(...)` runs one micro-step with ordinary launches on the same direct path, and
    `capture()` records the graphs once the allocations are warm.  `accumulate=True` captures the step as three pieces in
    every mode (capture_plan) and `micro(..., first=, last=)` replays [Z] F [B].  `grad_scale` multiplies d loss / d eps in
    every pass (1 / accumulate_grad_batches); a by-value kernel argument, constant for a run, so baked into the capture."""

    def __init__(self, model, opt, z, cond_txt, hint, t, noise, warmup: int = 2, split_graphs=None,
                 bucket_bytes: int = 32 << 20, reduce_fn=None, capture_error_mode=None, grad_scale: float = 1.0,
                 accumulate: bool = False, capture: bool = True):
        import torch.distributed as dist
        self.model, self.opt = model, opt
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        # With a process group alive, RCCL's watchdog thread polls events while this thread captures: only calls made
        # by the capturing thread may invalidate the capture ("thread_local"); single-process keeps the strict default.
        self.capture_error_mode = capture_error_mode or ("thread_local" if self.world > 1 else "global")
        if split_graphs is None:
            split_graphs = self.world > 1
        self.mode = mode = {True: "segmented", "segmented": "segmented", "two": "two"}.get(split_graphs, "one")
        self._static = _StaticInputs(z, cond_txt, hint, t, noise)
        self.loss = self.loss3 = None
        if model.dp is not None:
            model.dp.enabled = False    # no collectives inside the captured regions: this class issues them itself
        # reduce_fn(tensor_slice) -> work handle with .wait() or None; default: RCCL SUM all-reduce, asynchronous
        if reduce_fn is None:
            from .parallel import all_reduce_slice, payload_dtype_from_env
            payload = payload_dtype_from_env()       # CTRLORA_DP_PAYLOAD=bf16: half the bytes per bucket

            world = self.world               # not `self`: a closure over it would make this object a reference cycle, and
                                             # its graphs would go only when the cycle collector runs, possibly inside a capture

            def reduce_fn(buf):
                if dist.is_initialized() and world > 1:
                    return all_reduce_slice(buf, None, payload)
                return None
        self._reduce_fn = reduce_fn
        self.grad_scale, self.accumulate, self.bucket_bytes = float(grad_scale), bool(accumulate), bucket_bytes
        opt.pre_step_hook = None          # the exchange it would wait for is issued by this class
        self._side = side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self._fwd_bwd(self._static.tensors)
                if mode != "one":
                    self._reduce_all()
                opt.step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.segments = []               # [(graph, executor index or None, lo, hi)]
        self.g_z = self.g_b = None       # the Z and B pieces, where capture_plan has them
        self.captured, self.warmup_steps = False, warmup
        if capture:
            self.capture()

    def _fwd_bwd(self, tensors, zero=True):
        """[zero_grad,] forward, loss, backward on `tensors` = (z, ctx, hint, t, noise): the gradients are ADDED to the flat
        buffer.  Returns (loss scalar, {loss_simple, loss_vlb, loss} or None without the direct path), device tensors."""
        z, ctx, hint, t, noise = tensors
        model, gs = self.model, self.grad_scale
        if zero:
            self.opt.zero_grad()
        cond = {"c_crossattn": [ctx], "c_concat": [hint]}
        direct = getattr(model, "engine_train_step", None)
        if direct is not None:
            # p_losses + backward without autograd: the captured region holds hand-written kernel nodes only
            # (no ATen launch, no memset node); out = {loss_simple, loss_vlb, loss}
            loss3 = direct(z, cond, t, noise) if gs == 1.0 else direct(z, cond, t, noise, grad_scale=gs)
            return loss3[2], loss3
        loss, _ = model.p_losses(z, cond, t, noise=noise)
        (loss if gs == 1.0 else loss * gs).backward()
        return loss.detach(), None

    def _reduce_all(self):
        works = [self._reduce_fn(ex.tr.flat_grad) for ex in self.opt.executors]
        for w in works:
            if w is not None:
                w.wait()

    def eager(self, z, cond_txt, hint, t, noise, first: bool = True, last: bool = True):
        """One micro-step with ordinary launches on the caller's tensors (any shapes): what a replay computes, for the steps
        that warm the allocations before capture() and for batches whose shapes are not the captured ones.  Runs on this
        object's side stream, fenced against the current stream on both ends.  Returns {loss_simple, loss_vlb, loss} where the
        model has the direct path, else the loss scalar."""
        self._refuse_in_ema_scope()
        cur = torch.cuda.current_stream()
        self._side.wait_stream(cur)
        with torch.cuda.stream(self._side):
            loss, loss3 = self._fwd_bwd((z, cond_txt, hint, t, noise), zero=first)
            out = loss3 if loss3 is not None else loss
            if last:
                if self.mode != "one":
                    self._reduce_all()
                self.opt.step()
        cur.wait_stream(self._side)
        return out

    def capture(self):
        """Record the graphs on the static tensors.  Capturing executes nothing."""
        assert not self.captured, "captured already"
        opt = self.opt
        torch.cuda.synchronize()
        opt.sync_hyper()
        self._pool = torch.cuda.graph_pool_handle()      # every piece of this step object allocates from one pool
        for piece in capture_plan(self.mode, self.accumulate):
            if piece.kind == "Z":
                self.g_z = self._capture(opt.zero_grad)
            elif piece.kind == "B":
                self.g_b = self._capture(opt.step)
            else:
                def fwd_bwd():
                    self.loss, self.loss3 = self._fwd_bwd(self._static.tensors, zero=piece.zero)
                    if piece.with_opt:
                        opt.step()
                if piece.segmented:
                    self._capture_segments(fwd_bwd, max(1, self.bucket_bytes // 4))
                else:
                    self.segments.append((self._capture(fwd_bwd), piece.tag, 0, 0))
        self.captured = True

    def _capture(self, fn):
        """Record what `fn` launches as a new graph in this step object's pool."""
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, pool=self._pool, capture_error_mode=self.capture_error_mode):
            fn()
        return g

    def _capture_segments(self, fwd_bwd, bucket_elems):
        """Capture forward + backward as consecutive graphs that end where a gradient bucket is complete.  The
        executors' stage-completion hook (ControlNetE._done -> on_stage_done(start, end), called after the stage's last
        kernel was enqueued) closes the running capture and opens the next one in the same memory pool."""
        import gc
        execs = list(self.opt.executors)
        saved_hooks = [ex.on_stage_done for ex in execs]
        # what `torch.cuda.graph` does on entry, which this path does not go through: a collection DURING the capture that
        # reached an unreferenced graph, stream or pool block would destroy it from the capturing thread, which a capture forbids
        gc.collect()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        state = {"g": None, "lo": {id(ex): 0 for ex in execs}, "hi": {id(ex): 0 for ex in execs}}

        def begin():
            state["g"] = torch.cuda.CUDAGraph()
            state["g"].capture_begin(pool=self._pool, capture_error_mode=self.capture_error_mode)

        def end(tag, lo, hi):
            state["g"].capture_end()
            self.segments.append((state["g"], tag, lo, hi))
            state["g"] = None

        def make_hook(i, ex):
            def on_stage(start, stop):
                k = id(ex)
                if start != state["hi"][k]:
                    return                                  # out-of-order report: left to the final flush
                state["hi"][k] = stop
                if stop - state["lo"][k] >= bucket_elems and stop < ex.tr.numel:
                    end(i, state["lo"][k], stop)
                    state["lo"][k] = stop
                    begin()
            return on_stage

        for i, ex in enumerate(execs):
            ex.on_stage_done = make_hook(i, ex)
        try:
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                begin()
                fwd_bwd()
                # whatever has not been handed out yet (the tail of every bank) goes with the last segment
                g_last = state["g"]
                g_last.capture_end()
                tails = [(i, state["lo"][id(ex)], ex.tr.numel) for i, ex in enumerate(execs) if state["lo"][id(ex)] < ex.tr.numel]
                self.segments.append((g_last, "tails", tails, 0))
            torch.cuda.current_stream().wait_stream(stream)
            torch.cuda.synchronize()
        except BaseException:
            # leave no stream in capture mode behind: the caller falls back to eager launches on this device
            g_open, state["g"] = state["g"], None
            if g_open is not None:
                try:
                    with torch.cuda.stream(stream):
                        g_open.capture_end()
                except Exception:
                    pass
            self.segments = []
            raise
        finally:
            for ex, h in zip(execs, saved_hooks):
                ex.on_stage_done = h

    def _refuse_in_ema_scope(self):
        """A replay does not pass through opt.step(): the same refusal, before anything is enqueued."""
        ema = getattr(self.opt, "ema", None)
        if ema is not None and ema.in_scope:
            raise RuntimeError("a training step inside ema_scope(): the masters hold the EMA weights, a step would train the "
                               "average and average the result; leave the scope first")

    def matches(self, z, cond_txt, hint, t, noise) -> bool:
        """Do these tensors have the shapes and dtypes the graphs were captured on?"""
        return self._static.matches(z, cond_txt, hint, t, noise)

    def __call__(self, z, cond_txt, hint, t, noise):
        self.micro(z, cond_txt, hint, t, noise)
        return self.loss

    def micro(self, z, cond_txt, hint, t, noise, first: bool = True, last: bool = True):
        """Replay one micro-step of an optimizer step and return the loss 3-vector (overwritten by the next replay).
        `first`: clear the gradients before; `last`: exchange the gradient buckets between the segments and run the optimizer
        piece after.  Without accumulate=True there is one form only, the whole optimizer step."""
        assert self.accumulate or (first and last), "captured as one optimizer step per replay: build with accumulate=True"
        self._refuse_in_ema_scope()
        self._static.load(z, cond_txt, hint, t, noise)
        if first and self.g_z is not None:
            self.g_z.replay()
        if last:
            self.opt.sync_hyper()
            replay_with_exchange(self.segments, self.g_b, self.opt.executors, self._reduce_fn)
        else:
            for g, _, _, _ in self.segments:      # gradients stay local until the last micro-step
                g.replay()
        return self.loss3


def _replay_step_start(g):
    """Replay the first captured piece of an optimizer step.  The step's optimizer piece re-packs the trainables, so caches
    of the old copies are stale: WEIGHTS_GENERATION moves before anything is enqueued."""
    from .engine.nets import WEIGHTS_GENERATION
    WEIGHTS_GENERATION[0] += 1
    g.replay()


def replay_with_exchange(segments, g_opt, execs, reduce_fn):
    """One optimizer step from captured pieces (anything with .replay()): every segment is enqueued, and right after
    a segment that completes a gradient bucket the reduction of that slice of the flat buffer is issued
    (`reduce_fn(slice)` -> handle with .wait() or None) -- it runs while the NEXT segment executes; all handles are waited for
    before the optimizer piece.  segments: [(graph, tag, lo, hi)], tag None = nothing to exchange, "all" = every executor's
    whole buffer, "tails" = lo is [(executor index, start, stop)], an int = that executor's [lo, hi) slice."""
    works = []
    for k, (g, tag, lo, hi) in enumerate(segments):
        if k == 0:
            _replay_step_start(g)
        else:
            g.replay()
        if tag is None:
            continue
        if tag == "all":
            works += [reduce_fn(ex.tr.flat_grad) for ex in execs]
        elif tag == "tails":
            works += [reduce_fn(execs[i].tr.flat_grad[a:b]) for i, a, b in lo]
        else:
            works.append(reduce_fn(execs[tag].tr.flat_grad[lo:hi]))   # overlaps the next segment's replay
    for w in works:
        if w is not None:
            w.wait()
    if g_opt is not None:
        g_opt.replay()


class GraphedPretrainStep:
    """One optimizer step of multi-task Base-ControlNet pre-training (cldm/cldm_ctrlora_pretrain.py:95-111,174-182) as a
    hipGraph replay: ONE GRAPH PER TASK, all in one memory pool.  A task's graph is self-contained:

        re-pack of that task's LoRA bank into the shared packed copies (the bank switch)  ->  zero_grad  ->  p_losses
        forward + hand-written backward (base weights + that bank)  ->  PretrainAdamW (base + every active bank)  ->  re-pack

    so replaying graphs in any task order is the eager sequence.  PretrainAdamW updates every bank that has EVER received a
    gradient, so the set of active banks is part of what a graph captured: while banks are still joining (a task's first
    step) the step runs eagerly, and graphs are (re-)captured once the active set is what they would bake in.  After a
    replay the host-side bank pointers are moved without another re-pack, so eager code that follows sees a consistent
    executor.  Single process (the data-parallel exchange of pre-training is eager: `_PretrainDP`)."""

    def __init__(self, model, opt, z, cond_txt, hint, t, noise):
        self.model, self.opt = model, opt
        self._static = _StaticInputs(z, cond_txt, hint, t, noise)
        self.graphs = {}             # task -> (graph, loss 3-vector)
        self._active_at_capture = None
        self._pool = None
        self.eager_steps = 0

    def _step(self, task):
        cm = self.model.control_model
        cm.switch_lora(task)
        cm.executor().switch_bank(cm.bank(task), force=True)      # the graph's first kernel: this bank -> packed copies
        self.opt.zero_grad()
        z, ctx, hint, t, noise = self._static.tensors
        loss3 = self.model.engine_train_step(z, {"c_crossattn": [ctx], "c_concat": [hint], "task": task}, t, noise)
        self.opt.step()
        return loss3

    def __call__(self, task, z, cond_txt, hint, t, noise):
        self._static.load(z, cond_txt, hint, t, noise)
        opt = self.opt
        if task not in opt.active:                      # the bank joins the optimizer in this step: eager
            self.eager_steps += 1
            return self._step(task)[2]
        if self._active_at_capture != tuple(opt.active):   # the active set changed: every captured optimizer piece is stale
            self.graphs.clear()
            self._active_at_capture = tuple(opt.active)
        ent = self.graphs.get(task)
        if ent is None:
            opt.sync_hyper()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                done = self._step(task).clone()         # warm-up of this task's allocation pattern: it IS this call's step
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            self.eager_steps += 1
            with torch.cuda.graph(g, pool=self._pool):
                loss3 = self._step(task)                # capture does not execute
            if self._pool is None:
                self._pool = g.pool()
            self.graphs[task] = (g, loss3)
            return done[2]
        opt.sync_hyper()
        _replay_step_start(ent[0])
        self.model.control_model.switch_lora(task, repacked=True)
        return ent[1][2]
