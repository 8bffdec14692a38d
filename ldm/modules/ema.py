"""Exponential moving average of trained weights (API of the reference's ldm/modules/ema.py: LitEma -- same buffers, same
key rule, same arithmetic, same method names), pointed at what CtrLoRA fine-tuning actually trains.

Buffers, as LitEma registers them: `decay` (fp32 scalar), `num_updates` (torch.int scalar; 0, or -1 for "no warm-up"), and one
shadow per tracked parameter under the parameter's name with the dots removed.  One update, all in fp32, every operation
rounded once:

    num_updates += 1                                              (only while num_updates >= 0)
    d   = min(decay, (1 + num_updates) / (10 + num_updates))      (decay itself while num_updates < 0)
    omd = 1 - d
    shadow -= omd * (shadow - parameter)

`forward()` is that update in plain torch: the host restatement, for a step taken by anything but an engine optimizer.  On
the GPU the engine's optimizer runs the same three operations as one launch per flat buffer inside its own step
(cl_ema_update: ctrlora_amd.train.FusedAdamW), on the tensors `bind()` installs: the shadows become views of ONE flat fp32
buffer laid out like the executor's flat masters, and `decay` / `num_updates` are the device scalars the kernel reads.
"""
from typing import Dict, Iterable, Tuple, Union

import torch
from torch import nn

Named = Union[nn.Module, Dict[str, torch.Tensor], Iterable[Tuple[str, torch.Tensor]]]


def shadow_key(name: str) -> str:
    """LitEma's buffer name of parameter `name`: '.' is not allowed in a buffer name, so the dots go."""
    return name.replace(".", "")


def _named(src: Named, trainable_only: bool):
    if isinstance(src, nn.Module):
        return [(n, p) for n, p in src.named_parameters() if p.requires_grad or not trainable_only]
    return list(src.items()) if isinstance(src, dict) else list(src)


def _note_source(module, state_dict, prefix, *_):
    module._had_keys = any(k.startswith(prefix) for k in state_dict)


class ModelEma(nn.Module):
    """Shadows of `named_params`: an nn.Module (its parameters with requires_grad, as LitEma takes them) or (name, tensor) pairs /
    a dict, shadowed in the order given."""

    def __init__(self, named_params: Named, decay: float = 0.9999, use_num_updates: bool = True):
        super().__init__()
        decay = float(decay)
        if not 0.0 <= decay <= 1.0:
            raise ValueError("Decay must be between 0 and 1")
        self.register_buffer("decay", torch.tensor(decay, dtype=torch.float32))
        self.register_buffer("num_updates", torch.tensor(0 if use_num_updates else -1, dtype=torch.int))
        self.use_num_updates = bool(use_num_updates)
        self.m_name2s_name = {}
        for name, p in _named(named_params, trainable_only=True):
            key = shadow_key(name)
            if key in self._buffers:
                raise ValueError(f"shadow name '{key}' of parameter '{name}' is taken already")
            self.m_name2s_name[name] = key
            self.register_buffer(key, p.detach().clone())
        self.collected_params = []
        self._decay_host = None       # a value set_decay() took that sync() has not pushed yet
        self.touched = False          # updated or loaded since the last seeding: bind() then keeps the values
        self.in_scope = False         # inside ema_scope(): the weights ARE the shadows, an optimizer step must not run
        self.flat, self._bound_to = None, None      # once bound: the flat shadow buffer and the executor it mirrors
        self._had_keys = False
        self._register_load_state_dict_pre_hook(_note_source, with_module=True)     # a plain function: no cycle through self

    # ---- state

    def source_had_keys(self) -> bool:
        """Did the source of the last load_state_dict that reached this module carry any of its keys?"""
        return self._had_keys

    def shadows(self) -> Dict[str, torch.Tensor]:
        """Parameter name -> shadow tensor, in the shadowed order."""
        return {n: self._buffers[k] for n, k in self.m_name2s_name.items()}

    def reset_num_updates(self):
        self.num_updates.zero_()      # in place: a bound counter is read by address

    def set_decay(self, decay: float):
        """Host side of a decay change; it reaches the buffer with the next sync() (the optimizer's sync_hyper())."""
        decay = float(decay)
        if not 0.0 <= decay <= 1.0:
            raise ValueError("Decay must be between 0 and 1")
        self._decay_host = decay

    def sync(self):
        """Push a changed decay to the buffer (a host -> device copy once bound: outside graph capture / between replays)."""
        if self._decay_host is not None:
            self.decay.copy_(torch.tensor(self._decay_host, dtype=torch.float32))
            self._decay_host = None

    @torch.no_grad()
    def seed(self, named_params: Named):
        """Shadows := parameters, num_updates := 0 (kept at -1 without the warm-up): the reference's reset_ema."""
        if self.flat is not None:
            self.flat.copy_(self._bound_to.tr.flat)       # the masters ARE the parameters; the zero padding comes along
        else:
            src = dict(_named(named_params, trainable_only=False))
            for name, key in self.m_name2s_name.items():
                self._buffers[key].copy_(src[name].detach())
        if int(self.num_updates) > 0:
            self.reset_num_updates()
        self.touched = False

    # ---- the update, on the host
    @torch.no_grad()
    def forward(self, named_params: Named):
        self.sync()
        decay = self.decay
        if self.num_updates >= 0:
            self.num_updates += 1
            warm = (1 + self.num_updates) / (10 + self.num_updates)       # int / int: fp32
            decay = warm if warm < decay else decay                       # Python's min(decay, warm)
        omd = 1.0 - decay
        src = dict(_named(named_params, trainable_only=False))
        for name, key in self.m_name2s_name.items():
            s = self._buffers[key]
            s.sub_(omd * (s - src[name].detach().to(s.dtype)))
        self.touched = True

    # ---- LitEma's swap-in / swap-out for modules without an engine
    @torch.no_grad()
    def copy_to(self, named_params: Named):
        dst = dict(_named(named_params, trainable_only=False))
        for name, key in self.m_name2s_name.items():
            dst[name].data.copy_(self._buffers[key])

    def store(self, parameters):
        self.collected_params = [p.detach().clone() for p in parameters]

    @torch.no_grad()
    def restore(self, parameters):
        for saved, p in zip(self.collected_params, parameters):
            p.data.copy_(saved)
        self.collected_params = []

    # ---- the engine's form
    @torch.no_grad()
    def bind(self, executor, prefix: str = ""):
        """Re-point the shadows at one flat fp32 buffer laid out like `executor.tr.flat` (same offsets, same padding; a conv
        weight in the master's [O][9][I_pad] storage behind a view of the Parameter's shape), the way bind_trainables binds the
        Parameters.  `prefix` + an executor trainable's name is the shadowed parameter's name.  Untouched shadows are seeded
        from the masters; updated or loaded ones keep their values.  Idempotent per executor: the flat buffer's address never
        changes afterwards."""
        tr = executor.tr
        if self.flat is not None and self._bound_to is executor:
            return self.flat
        if sorted(prefix + t.name for t in tr.items) != sorted(self.m_name2s_name):
            raise ValueError("the executor's trainable set is not the shadowed set")
        keep = self.touched or self.flat is not None      # a binding to an earlier executor holds the values too
        flat = torch.zeros_like(tr.flat)
        dev = flat.device
        if not keep:
            flat.copy_(tr.flat)
            if int(self.num_updates) > 0:
                self.reset_num_updates()
        for t in tr.items:
            key = self.m_name2s_name[prefix + t.name]
            view = t.param_view(flat[t.offset:t.offset + t.master.numel()].view(t.shape))
            if keep:
                view.copy_(self._buffers[key].to(device=dev, dtype=torch.float32))
            self._buffers[key] = view
        self._buffers["decay"] = self.decay.to(dev)
        self._buffers["num_updates"] = self.num_updates.to(dev)
        self.flat, self._bound_to = flat, executor
        return flat

    def _apply(self, fn, *args, **kwargs):
        """A move (.to / .cpu / .cuda) gives every buffer storage of its own: the binding is gone, the values stay."""
        before = self._buffers.get("num_updates")
        out = super()._apply(fn, *args, **kwargs)
        if self.flat is not None and self._buffers.get("num_updates") is not before:
            self.flat, self._bound_to, self.touched = None, None, True
        return out
