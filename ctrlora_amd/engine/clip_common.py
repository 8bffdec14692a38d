"""What the two CLIP towers share (vit.py: ClipVisionE, clip_text.py: ClipTextE), each stated once: the state-dict walk and the
packing of an encoder layer, the width refusals, the executor base (construction, the in-place weight refresh), the pre-LN layer
as a launch sequence, and ExecutorHost, the nn.Module mixin that owns a lazily built executor.

Modules restated by both towers (behaviour, not code; transformers/models/clip/modeling_clip.py):

  CLIPEncoderLayer   :353-384  pre-LN: x + out_proj(attn(LN1 x)); x + fc2(act(fc1(LN2 x)))            (encoder_layer)
  CLIPAttention      :280-335  softmax(q k^T d^-1/2) v, q | k | v as ONE product (pack_layers: qkv_w / qkv_b); the mask, the
                               d_head and the kernel are the tower's (`attend`)
  CLIPMLP            :338-350  fc1 with the activation in the product's epilogue, fc2 with the residual

Per tower: the embeddings, the residual stream's dtype and which buffer is src / mid / out of a layer, the attention launch,
the activation, and everything after the last layer.
"""
from __future__ import annotations

import os
from typing import Dict, List

import torch

from .. import hip

K_GRAIN = 32                                 # cl_gemm's K granularity in bf16 (16 in fp32): 3 * 14 * 14 = 588 -> 608

# encoder.layers.{i}.* in the HF modules' own order
LAYER_MODULES = ("self_attn.k_proj", "self_attn.v_proj", "self_attn.q_proj", "self_attn.out_proj", "layer_norm1", "mlp.fc1", "mlp.fc2",
                 "layer_norm2")


def layer_state_keys(prefix: str, L: int) -> List[str]:
    """The state-dict keys of `prefix`encoder.layers.0 .. L-1, in the module's order."""
    return [f"{prefix}encoder.layers.{i}.{m}.{p}" for i in range(L) for m in LAYER_MODULES for p in ("weight", "bias")]


def pack_layers(sd: Dict[str, torch.Tensor], prefix: str, L: int, f, fc1_scale: float = 1.0) -> List[dict]:
    """Per layer, the tensors the launches of encoder_layer read: f(key) is the caller's cast of sd[key]; q | k | v concatenated
    into one [3D, D] weight / [3D] bias; fc1's weight and bias times fc1_scale in f's dtype (clip_text.py: quick_gelu)."""
    s = (lambda t: t * fc1_scale) if fc1_scale != 1.0 else (lambda t: t)
    layers = []
    for i in range(L):
        p = f"{prefix}encoder.layers.{i}."
        a = p + "self_attn."
        layers.append(dict(
            ln1_g=f(p + "layer_norm1.weight"), ln1_b=f(p + "layer_norm1.bias"),
            qkv_w=torch.cat([f(a + n + "_proj.weight") for n in "qkv"], 0), qkv_b=torch.cat([f(a + n + "_proj.bias") for n in "qkv"], 0),
            o_w=f(a + "out_proj.weight"), o_b=f(a + "out_proj.bias"),
            ln2_g=f(p + "layer_norm2.weight"), ln2_b=f(p + "layer_norm2.bias"),
            fc1_w=s(f(p + "mlp.fc1.weight")), fc1_b=s(f(p + "mlp.fc1.bias")),
            fc2_w=f(p + "mlp.fc2.weight"), fc2_b=f(p + "mlp.fc2.bias")))
    return layers


def check_d_head(c: dict, d_heads, which: str):
    D, H = c["hidden_size"], c["num_attention_heads"]
    if D % H or D // H not in d_heads:
        raise ValueError(f"num_attention_heads = {H} with hidden_size = {D}: d_head {D / H:g} is not {which}")


def check_widths(c: dict):
    for k in ("hidden_size", "intermediate_size"):
        if c[k] % K_GRAIN:
            raise ValueError(f"{k} = {c[k]} is not a multiple of {K_GRAIN} (K granularity of the products)")
    if c["projection_dim"] % 8:
        raise ValueError(f"projection_dim = {c['projection_dim']} is not a multiple of 8")


def supported(check_config, *args) -> bool:
    """check_config(*args) did not raise."""
    try:
        check_config(*args)
        return True
    except ValueError:
        return False


class ClipExecutor:
    """Base of the two executors.  `cfg` is the tower's check_config(config), evaluated by the caller before anything here
    touches the GPU (the refusals need none).  A subclass states pack(state_dict) and WEIGHTS, and sets self.w itself."""
    WEIGHTS = ()                             # the packed tensors stored in the engine dtype; everything else stays fp32

    def __init__(self, cfg: dict, state_dict: Dict[str, torch.Tensor], dtype, device=None):
        self.cfg = cfg
        if dtype not in (torch.bfloat16, torch.float32):
            raise ValueError(f"dtype = {dtype}: the engine stores bf16 or fp32")
        hip.lib()
        self.dtype = dtype
        self.device = torch.device(device if device is not None else next(iter(state_dict.values())).device)
        self.D, self.H, self.F, self.L = cfg["hidden_size"], cfg["num_attention_heads"], cfg["intermediate_size"], cfg["num_hidden_layers"]
        self.eps = float(cfg["layer_norm_eps"])
        self._buf: Dict[object, dict] = {}

    def _to_device(self, packed: dict, weight_keys) -> dict:
        mv = lambda k, t: t.to(device=self.device, dtype=self.dtype if k in weight_keys else torch.float32).contiguous()
        out = {k: mv(k, t) for k, t in packed.items() if k != "layers"}
        out["layers"] = [{k: mv(k, t) for k, t in lay.items()} for lay in packed["layers"]]
        return out

    def load(self, state_dict: Dict[str, torch.Tensor]):
        """Refresh the packed weights in place (the address rule of engine/packing.py: a captured graph keeps replaying them)."""
        new = self.pack(state_dict)
        for k, t in new.items():
            if k != "layers":
                self.w[k].copy_(t)
        for old, lay in zip(self.w["layers"], new["layers"]):
            for k, t in lay.items():
                old[k].copy_(t)


def encoder_layer(lay: dict, src, mid, out, qkv, m, *, norm, attend, act, alpha=1.0, qkv_alpha=1.0, qkv_alpha_n=0, atomic=False):
    """One pre-LN layer as its seven steps: LN -> qkv product -> attention -> out_proj + residual -> LN -> fc1 + activation ->
    fc2 + residual.  norm(src, gamma, beta) is the caller's LayerNorm and returns what the product reads; attend(qkv) is its
    attention launch and returns the heads' output.  The stream goes src -> mid -> out through the products' residual epilogue;
    with atomic both products ADD onto the fp32 stream in place (cl_gemm's atomic mode), and mid and out are src."""
    hip.gemm(norm(src, lay["ln1_g"], lay["ln1_b"]), lay["qkv_w"], qkv, bias=lay["qkv_b"], alpha=qkv_alpha, alpha_n=qkv_alpha_n)
    a = attend(qkv)
    if atomic:
        hip.gemm(a, lay["o_w"], mid, bias=lay["o_b"], atomic=True)
    else:
        hip.gemm(a, lay["o_w"], mid, bias=lay["o_b"], residual=src, beta=1.0)
    hip.gemm(norm(mid, lay["ln2_g"], lay["ln2_b"]), lay["fc1_w"], m, bias=lay["fc1_b"], act=act, alpha=alpha)
    if atomic:
        hip.gemm(m, lay["fc2_w"], out, bias=lay["fc2_b"], atomic=True)
    else:
        hip.gemm(m, lay["fc2_w"], out, bias=lay["fc2_b"], residual=mid, beta=1.0)
    return out


class ExecutorHost:
    """Mixin of the nn.Modules that run on an executor (cldm/style_helpers.py: CLIPVisionEncoder, CLIPTextEncoder;
    ldm/modules/encoders/modules.py: FrozenCLIPEmbedder).  The executor is built on first use from the state dict, the config
    and the device of _engine_source(), lives in self.__dict__[ENGINE_SLOT] -- not a registered child, not in the state dict --
    is dropped when the parameters move or the engine dtype changes, and is refreshed IN PLACE by load_state_dict (the address
    rule of engine/packing.py: a captured graph keeps replaying the packed weights)."""
    ENGINE_SLOT = None                       # "_vit" / "_txt"
    ENGINE_CLASS = None                      # ClipVisionE / ClipTextE

    def _init_engine_host(self, dtype=None):
        """dtype None: CTRLORA_ENGINE_DTYPE (f32 / fp32 / float32), bf16 without it."""
        self.engine_dtype = dtype
        self.use_engine = True
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._refresh_engine())

    def _engine_source(self):
        return self

    def set_engine_dtype(self, dtype):
        self.engine_dtype = dtype
        self.invalidate_engine()

    def invalidate_engine(self):
        self.__dict__.pop(self.ENGINE_SLOT, None)

    def _refresh_engine(self):
        """load_state_dict after the first forward: the executor's packed weights are refreshed in place."""
        ex = self.__dict__.get(self.ENGINE_SLOT)
        if ex is not None:
            src = self._engine_source()
            if ex.device != next(src.parameters()).device:
                self.invalidate_engine()
            else:
                ex.load(src.state_dict())

    def _apply(self, fn, *args, **kwargs):      # .to() / .cuda() / .float(): the packed copies follow the parameters
        self.invalidate_engine()
        return super()._apply(fn, *args, **kwargs)

    def engine(self):
        ex = self.__dict__.get(self.ENGINE_SLOT)
        if ex is None:
            dtype = self.engine_dtype
            if dtype is None:
                env = os.environ.get("CTRLORA_ENGINE_DTYPE", "bf16").lower()
                dtype = torch.float32 if env in ("f32", "fp32", "float32") else torch.bfloat16
            src = self._engine_source()
            ex = self.ENGINE_CLASS(src.state_dict(), src.config, dtype, next(src.parameters()).device)
            self.__dict__[self.ENGINE_SLOT] = ex
        return ex
