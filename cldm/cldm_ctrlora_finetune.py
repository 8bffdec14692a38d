"""CtrLoRA fine-tuning classes (API of the reference's cldm/cldm_ctrlora_finetune.py)."""
import os

import torch
import torch.nn as nn

from cldm.cldm import ControlLDM, ControlNet
from cldm.ddim_hacked import DDIMSampler
from cldm.lora import LoRACompatibleLinear, LoRALinearLayer


def swap_linears(root: nn.Module, make_lora, skip=()):
    """Replace every nn.Linear below `root` by a LoRACompatibleLinear carrying the same weights
    (cldm_ctrlora_finetune.py:21-38).  Returns the new modules in named_modules order."""
    out = []
    for name, m in list(root.named_modules()):
        if not isinstance(m, nn.Linear) or isinstance(m, LoRACompatibleLinear) or any(s in name for s in skip):
            continue
        new = LoRACompatibleLinear(m.in_features, m.out_features, lora_layer=make_lora(m))
        new.weight.data.copy_(m.weight.data)
        if m.bias is not None:
            new.bias.data.copy_(m.bias.data)
        else:
            new.bias = None
        *path, leaf = name.split(".")
        parent = root
        for p in path:
            parent = parent.get_submodule(p)
        parent._modules[leaf] = new
        out.append(new)
    return out


_REFERENCE_TOP_LEVEL = ("time_embed", "input_blocks", "zero_convs", "middle_block", "middle_block_out")


def _reference_module_rank(name: str) -> int:
    """Position of a parameter's top-level module in the reference ControlNet's registration order (stable sort key)."""
    head = name.split(".", 1)[0]
    return _REFERENCE_TOP_LEVEL.index(head) if head in _REFERENCE_TOP_LEVEL else len(_REFERENCE_TOP_LEVEL)


MAX_OPTIM_GROUPS = 8      # the rows of the optimizer's device table (ctrlora_amd.hip.ADAMW_MAX_GROUPS)


def assign_optim_groups(names, rules):
    """Split the trained tensors into optimizer parameter groups (not in the reference: its fine-tuning has one group).
    `rules`: a list of {name, match: [substrings], lr_scale: 1.0, weight_decay: None}, applied to `names` in order -- a name
    joins the FIRST rule one of whose substrings it contains; the names no rule takes form group 0, "default".  Returns
    [{name, lr_scale, weight_decay, names}], "default" first, then the rules in their order.  A rule that matches nothing is a
    mistake in the rule, not an empty group: ValueError."""
    groups = [dict(name="default", lr_scale=1.0, weight_decay=None, names=[])]
    for r in rules:
        r = dict(r)
        unknown = set(r) - {"name", "match", "lr_scale", "weight_decay"}
        if unknown or "name" not in r or not r.get("match"):
            raise ValueError(f"optim_groups rule {r}: keys are name, match (a non-empty list of substrings), lr_scale, weight_decay")
        match = [r["match"]] if isinstance(r["match"], str) else [str(m) for m in r["match"]]
        lr_scale = float(r.get("lr_scale", 1.0))
        wd = r.get("weight_decay")
        if not lr_scale > 0.0 or (wd is not None and not float(wd) >= 0.0):
            raise ValueError(f"optim_groups rule '{r['name']}': lr_scale must be > 0 and weight_decay None or >= 0")
        groups.append(dict(name=str(r["name"]), match=match, lr_scale=lr_scale, weight_decay=None if wd is None else float(wd),
                           names=[]))
    if len({g["name"] for g in groups}) != len(groups):
        raise ValueError(f"optim_groups: the group names {[g['name'] for g in groups]} must differ ('default' is group 0)")
    if len(groups) > MAX_OPTIM_GROUPS:
        raise ValueError(f"optim_groups: {len(groups)} groups with 'default', at most {MAX_OPTIM_GROUPS}")
    for n in names:
        hit = next((g for g in groups[1:] if any(m in n for m in g["match"])), groups[0])
        hit["names"].append(n)
    for g in groups[1:]:
        if not g["names"]:
            raise ValueError(f"optim_groups rule '{g['name']}' (match {g['match']}) takes none of the {len(names)} trained "
                             "tensors: an earlier rule took them all, or nothing carries such a name")
    for g in groups:
        g.pop("match", None)
    return groups


class ControlNetFinetune(ControlNet):
    def __init__(self, ft_with_lora=True, lora_rank=128, norm_trainable=True, zero_trainable=True, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.ft_with_lora, self.lora_rank = ft_with_lora, lora_rank
        self.norm_trainable, self.zero_trainable = norm_trainable, zero_trainable
        del self.input_hint_block                                     # :19
        if ft_with_lora:
            swap_linears(self, lambda m: LoRALinearLayer(m.in_features, m.out_features, rank=lora_rank))
        # ft_with_lora=False (configs/ctrlora_finetune_sd15_full.yaml): plain linears, EVERY ControlNet parameter trains
        # (:100-103) -- the engine then forms all weight gradients, as in pre-training
        self.train_all_weights = not ft_with_lora

    def forward(self, hint, timesteps, context, **kwargs):
        """13 zero-conv outputs for a 4-channel latent hint (:40-54)."""
        return self._latent_forward(hint, timesteps, context)


class ControlFinetuneLDM(ControlLDM):
    """`use_ema: True` (with `ema_decay`, default LitEma's 0.9999) keeps an exponential moving average of the TRAINED weights
    in `self.model_ema` (ldm.modules.ema.ModelEma: LitEma's buffers, key rule and arithmetic).  Two deliberate differences from
    the reference's wiring (ddpm.py:85-88, 194-207, 441-443), which shadows `self.model` -- the frozen UNet -- from its
    construction-time values: the shadowed set is `trainable_names()`, what `configure_optimizers()` hands to FusedAdamW, and a
    load_state_dict whose source carries no `model_ema.*` key re-seeds the shadows from the loaded weights (the reference's
    reset_ema).  The update runs once per OPTIMIZER step, inside the optimizer's own step (the reference's on_train_batch_end
    runs after every micro-batch)."""
    supports_ema = True
    # `optim_groups` (a list of assign_optim_groups rules; None = one group, the state dict of before) and `scheduler_config`
    # (a target with `.schedule(n)`, e.g. ctrlora_amd.lr_schedule.WarmupDecay) are honoured by configure_optimizers().

    # ---- EMA of the trained weights
    def _ema_named_params(self):
        """Model-relative name -> Parameter of the shadowed set, in trainable_names() order."""
        params = dict(self.control_model.named_parameters())
        return {"control_model." + n: params[n] for n in self.trainable_names()}

    def _build_ema(self):
        from ldm.modules.ema import ModelEma
        self.model_ema = ModelEma(self._ema_named_params(), decay=self.ema_decay)
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._ema_after_load())

    def _ema_after_load(self):
        if self.model_ema.source_had_keys():
            self.model_ema.touched = True      # restored like any buffer
        else:
            done = int(self.model_ema.num_updates)
            if done > 0:
                print(f"[ema] load_state_dict without model_ema.* keys: the average of {done} updates is discarded, the shadows "
                      "start again from the loaded weights")
            self.reseed_ema()

    @torch.no_grad()
    def reseed_ema(self):
        """Shadows := the trained weights as they are now, num_updates := 0."""
        self.model_ema.seed(self._ema_named_params())

    def _bind_ema(self):
        """With the executor built: the shadows as views of one flat buffer laid out like its flat masters (idempotent)."""
        ex = self.control_model.executor()
        return ex, self.model_ema.bind(ex, prefix="control_model.")

    def _ema_enter(self):
        ema = self.model_ema
        if ema.in_scope:
            raise RuntimeError("ema_scope() is not re-entrant")
        if self.device.type == "cuda":
            from ctrlora_amd import hip
            ex, shadow = self._bind_ema()
            hip.swap_(ex.tr.flat, shadow)      # no tensor moves: a step captured before the scope replays correctly after it
            ex.repack()
        else:
            params = list(self._ema_named_params().values())
            ema.store(params)
            ema.copy_to(self._ema_named_params())
        ema.in_scope = True

    def _ema_exit(self):
        ema = self.model_ema
        if self.device.type == "cuda":
            from ctrlora_amd import hip
            ex, shadow = self._bind_ema()
            hip.swap_(ex.tr.flat, shadow)
            ex.repack()
        else:
            ema.restore(list(self._ema_named_params().values()))
        ema.in_scope = False

    @torch.no_grad()
    def sample_log(self, cond, batch_size, ddim, ddim_steps, **kwargs):
        b, c, h, w = cond["c_concat"][0].shape
        shape = (self.channels, h // 8, w // 8) if c != self.channels else (self.channels, h, w)
        return DDIMSampler(self).sample(ddim_steps, batch_size, shape, cond, verbose=False, **kwargs)

    def apply_model(self, x_noisy, t, cond, *args, **kwargs):
        """:67-82 -- ControlNet on the hint latent, residuals * control_scales, frozen UNet."""
        assert isinstance(cond, dict)
        cond_txt = torch.cat(cond["c_crossattn"], 1)
        if cond["c_concat"] is None:
            return self._run(x_noisy, t, cond_txt, None)
        return self._run(x_noisy, t, cond_txt, [self._hint_latent(cond)])

    @torch.no_grad()
    def engine_train_step(self, x_start, cond, t, noise, grad_scale=1.0):
        """p_losses (ddpm.py:885-920) + backward of the loss WITHOUT torch.autograd: q_sample, apply_model with
        recording, the p_losses reduction with d loss / d eps, the hand-written backward -- every launch is one of
        this library's kernels, so the whole thing is capturable as a hipGraph with no ATen nodes
        (ctrlora_amd.train.GraphedTrainStep).  Returns the device 3-vector {loss_simple, loss_vlb, loss}; gradients
        land in the flat buffer the optimizer's parameters view.  `grad_scale` multiplies d loss / d eps (not the three
        returned scalars): 1 / accumulate_grad_batches under gradient accumulation, what `(loss / acc).backward()` does."""
        from ctrlora_amd import hip
        from ctrlora_amd.train import p_losses_launch
        if self.loss_type not in hip.LOSS_KINDS or self.original_elbo_weight != 0.:
            raise NotImplementedError("engine_train_step: l2 loss without the elbo term (every CtrLoRA config)")
        x_noisy = self.q_sample(x_start=x_start, t=t, noise=noise)
        cc = cond["c_crossattn"]
        cond_txt = cc[0] if len(cc) == 1 else torch.cat(cc, 1)
        hints = [self._hint_latent(cond)]
        self._sync_trainables()
        eng = self.engine()
        eps = eng.forward(x_noisy, t, cond_txt, hints, control_scales=list(self.control_scales), record=True,
                          only_mid_control=self.only_mid_control)
        # with a per-timestep weight table (min_snr_gamma / set_loss_weights) and / or the Huber loss: cl_p_losses_w
        out, d_eps = p_losses_launch(eps, noise, t, self.lvlb_weights, grad_scale, self.l_simple_weight, 0.0, wt=self.loss_weights,
                                     kind=hip.LOSS_KINDS[self.loss_type], delta=self.huber_delta, bands=self.train_loss_bands)
        if torch.cuda.is_current_stream_capturing():
            self.loss_weights_pinned = True       # the graph holds the table's address, or the kernel that has none
        eng.backward(d_eps)
        if self.dp is not None:
            self.dp.on_backward_done()
        return out

    @torch.no_grad()
    def engine_eval_step(self, x_start, cond, t, noise, acc, n_valid=None):
        """One forward-only validation step (ctrlora_amd.validation; not in the reference): q_sample, the engine forward
        without recording, the plain l2 reduction without d loss / d eps and without per-timestep weights (cl_p_losses_mse,
        whatever the training objective is), and cl_loss_bands adding the per-sample losses to `acc` (device fp64
        [nbands + 1][3]).  `n_valid`: None or a device int32, the leading samples that count (a padded batch).  Every launch
        is one of this library's kernels, so the step is capturable; it leaves the recorded forward of a training step, the
        gradient buffers and `loss_weights_pinned` alone.  Returns the per-sample losses (device fp32 [B])."""
        from ctrlora_amd import hip
        t = t.long().contiguous()
        noise = noise.float().contiguous()
        x_noisy = self.q_sample(x_start=x_start, t=t, noise=noise)
        cc = cond["c_crossattn"]
        cond_txt = cc[0] if len(cc) == 1 else torch.cat(cc, 1)
        hints = [self._hint_latent(cond)]
        if not torch.cuda.is_current_stream_capturing():
            self._sync_trainables()
        eng = self.engine()
        # the text context changes from batch to batch: the context K / V cache of the samplers must stay off
        assert not eng.cache_context_kv, "engine_eval_step inside a sampler's context_kv scope"
        eps = eng.forward(x_noisy, t, cond_txt, hints, control_scales=list(self.control_scales), record=False,
                          only_mid_control=self.only_mid_control)
        B = eps.shape[0]
        out = torch.empty(3, dtype=torch.float32, device=eps.device)
        scratch = torch.empty(16 * B, dtype=torch.float32, device=eps.device)
        per = torch.empty(B, dtype=torch.float32, device=eps.device)
        hip.p_losses_mse(eps, noise, None, t, None, out, scratch, 1.0, 1.0, 0.0, per_sample=per)
        hip.loss_bands(per, t, self.num_timesteps, acc.shape[0] - 1, acc, n_valid=n_valid)
        return per

    def trainable_names(self):
        """Name filter of :84-108 (LoRA layers; zero convs incl. middle_block_out; `norm` layers)."""
        cm = self.control_model
        names = []
        # the reference registers time_embed and input_blocks BEFORE zero_convs (cldm/cldm.py:48-282), this mirror after:
        # walk the top-level modules in the reference's order, so that the list (and the file configure_optimizers writes)
        # comes out in its order
        for n, _ in sorted(cm.named_parameters(), key=lambda kv: _reference_module_rank(kv[0])):
            assert "input_hint" not in n
            if not cm.ft_with_lora:
                assert "lora_layer" not in n
                names.append(n)
            elif "lora_layer" in n:
                names.append(n)
            elif ("zero_convs" in n or "middle_block_out" in n) and cm.zero_trainable:
                names.append(n)
            elif "norm" in n and cm.norm_trainable:
                names.append(n)
        return names

    def configure_optimizers(self):
        from ctrlora_amd.train import FusedAdamW
        cm = self.control_model
        names = self.trainable_names()
        os.makedirs("./tmp", exist_ok=True)
        with open("./tmp/finetune_trainable_params.txt", "w") as f:
            f.write("\n".join(names) + "\n")
        ex = cm.executor()
        bound = dict(zip([t.name for t in ex.tr.items], cm.__dict__["_bound"]))
        # the executor was built with the same two flags (ControlNet.executor): its flat buffer holds exactly the filtered set
        assert set(names) == set(bound), "engine trainable set differs from the reference's name filter"
        params = [bound[n] for n in names]
        print(f"Optimizable params: {sum(p.numel() for p in params) / 1e6:.1f}M")
        world = 1 if self.dp is None else self.dp.world_size
        if self.optim_groups is not None:
            # torch's list-of-dicts form: "default" takes the constructor's lr and weight decay, a rule scales / replaces them
            params = []
            for g in assign_optim_groups(names, list(self.optim_groups)):
                d = dict(params=[bound[n] for n in g["names"]], name=g["name"], lr=self.learning_rate * g["lr_scale"])
                if g["weight_decay"] is not None:
                    d["weight_decay"] = g["weight_decay"]
                params.append(d)
                print(f"Parameter group '{g['name']}': {len(g['names'])} tensors, lr x {g['lr_scale']:g}"
                      + ("" if g["weight_decay"] is None else f", weight decay {g['weight_decay']:g}"))
        opt = FusedAdamW(params, [ex], lr=self.learning_rate, grad_scale=1.0 / world)
        if self.dp is not None:
            opt.pre_step_hook = self.dp.wait
        if self.use_ema:
            opt.attach_ema(self.model_ema, [self._bind_ema()[1]])
        if self.scheduler_config is None:
            return opt
        # the reference's shape (LatentDiffusion.configure_optimizers, ddpm.py:1288-1299): a LambdaLR stepped once per optimizer
        # step; the Trainer compiles it to a device table for an engine optimizer (ctrlora_amd.lr_schedule.compile_lambda_lr)
        from torch.optim.lr_scheduler import LambdaLR
        from ldm.util import instantiate_from_config
        sched = instantiate_from_config(self.scheduler_config)
        print("Setting up LambdaLR scheduler...")
        return [opt], [{"scheduler": LambdaLR(opt, lr_lambda=sched.schedule), "interval": "step", "frequency": 1}]
