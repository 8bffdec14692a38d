"""CLIP text encoder (CLIPTextModel / CLIPTextModelWithProjection in HF layout: ViT-L/14 text for the prompt, ViT-H/14 text for the
style app's negative content prompt) on the HIP kernels.  The sibling of vit.py: what the two share is in clip_common.py.

Where the reference calls it: FrozenCLIPEmbedder encodes every prompt (ldm/modules/encoders/modules.py:88-131); the style app
encodes the negative content prompt with CLIPTextModelWithProjection (app/gradio_ctrlora_style_transfer.py:395-403).  Modules
restated (behaviour, not code; transformers/models/clip/modeling_clip.py):

  CLIPTextEmbeddings   token_embedding(input_ids) + position_embedding                      (cl_clip_text_embed)
  CLIPEncoderLayer     the layer both towers walk: clip_common.py (encoder_layer, pack_layers)
  CLIPAttention        causal: softmax_{j <= i}(q k^T d^-1/2) v                              (cl_attention_causal_fwd, d_head 64)
  CLIPMLP              "gelu": the exact GELU epilogue (cl_gemm act 4).  "quick_gelu", x sigmoid(1.702 x), is the SiLU epilogue
                       by algebra: quick_gelu(x) = silu(1.702 x) / 1.702 -- fc1's weight and bias are packed multiplied by
                       1.702 (in fp32, before the cast to the engine dtype) and the product runs with act = SiLU,
                       alpha = 1 / 1.702 (the epilogue order is bias -> activation -> alpha)
  CLIPTextModel        final_layer_norm of every row; pooler_output = the row at argmax(input_ids) when eos_token_id == 2 (the
                       legacy configs), otherwise at the first position equal to eos_token_id  (cl_gather_rows)
  CLIPTextModelWithProjection   text_projection (no bias) of the pooled rows -> text_embeds (fp32)

Inference only.  Activations are token-major [B*N, D]; every buffer is allocated once per (B, N) and reused, so a forward is a
fixed launch sequence over fixed addresses (hipGraph-capturable; load() refreshes the packed weights in place).  The residual
stream is fp32 in both engine dtypes.  In fp32 every launch is fp32 and the residual enters through the product's epilogue.
In bf16 the products and the attention are bf16 and the stream stays fp32, as under HF's bf16 autocast -- a bf16 stream rounds
the whole residual twice a layer, which alone put the encoder at 1.3 .. 1.5 x the autocast module's error: LayerNorm runs on
the fp32 kernels and cl_pack2d rounds its output once for the product that follows; out_proj and fc2 ADD onto the stream
(cl_gemm's fp32 atomic mode with one K split: every element is added once, so the result does not depend on the order).
The packing (pack_clip_text) and clip_text_forward_torch, a torch restatement of the launch sequence, run on the CPU.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from .. import hip
from . import clip_common as cc

D_HEAD = 64                                  # csrc/attention_causal.hip
MAX_TOKENS = 128
QUICK_GELU = 1.702
OUTPUTS = ("last_hidden_state", "pooler_output", "text_embeds", "hidden_state")

_FIELDS = ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "max_position_embeddings",
           "layer_norm_eps", "hidden_act", "eos_token_id", "projection_dim")
_DEFAULTS = dict(layer_norm_eps=1e-5, eos_token_id=49407, projection_dim=512)      # CLIPTextConfig's own


def config_fields(config) -> dict:
    """The fields of a CLIPTextConfig (or a dict with the same names) that shape the encoder."""
    if isinstance(config, dict):           # a dict may leave out what CLIPTextConfig defaults
        return {k: config[k] if k in config else _DEFAULTS[k] for k in _FIELDS}
    return {k: getattr(config, k) for k in _FIELDS}


def check_config(config, attention_mask: Optional[torch.Tensor] = None) -> dict:
    """config_fields(config), or ValueError naming what the executor does not cover."""
    c = config_fields(config)
    if c["hidden_act"] not in ("gelu", "quick_gelu"):
        raise ValueError(f"hidden_act = {c['hidden_act']!r}: the executor has the exact GELU and (through SiLU) the quick_gelu epilogue only")
    cc.check_d_head(c, (D_HEAD,), f"{D_HEAD} (the causal kernel's)")
    if not 1 <= c["max_position_embeddings"] <= MAX_TOKENS:
        raise ValueError(f"max_position_embeddings = {c['max_position_embeddings']}: the causal kernel takes 1 .. {MAX_TOKENS} tokens")
    cc.check_widths(c)
    if attention_mask is not None and not bool((attention_mask == 1).all()):
        raise ValueError("attention_mask is not all ones: the causal kernel has no padding mask")
    return c


def supported(config, attention_mask: Optional[torch.Tensor] = None) -> bool:
    return cc.supported(check_config, config, attention_mask)


def state_keys(config, prefix: str = "text_model.", projection: bool = False) -> List[str]:
    """The state-dict keys of an HF CLIP text model with this config, in the module's order: `prefix` is "text_model." where the
    text tower is a child (CLIPTextModelWithProjection) and "" where it is the module itself; projection adds
    text_projection.weight."""
    c = config_fields(config)
    keys = [prefix + "embeddings.token_embedding.weight", prefix + "embeddings.position_embedding.weight"]
    keys += cc.layer_state_keys(prefix, c["num_hidden_layers"])
    keys += [prefix + "final_layer_norm.weight", prefix + "final_layer_norm.bias"]
    return keys + (["text_projection.weight"] if projection else [])


def _prefix(sd) -> str:
    for p in ("text_model.", ""):
        if p + "embeddings.token_embedding.weight" in sd:
            return p
    raise KeyError("no embeddings.token_embedding.weight (with or without the text_model. prefix) in the state dict")


def pack_clip_text(sd: Dict[str, torch.Tensor], config) -> dict:
    """Tensors in the layout the executor's launches read, on the state dict's device, in fp32 (fp64 where the state dict is
    fp64): q | k | v of a layer concatenated into one [3D, D] weight / [3D] bias; with quick_gelu fc1's weight and bias times
    1.702 (module docstring); text_projection.weight as proj_w where the state dict has one."""
    c = config_fields(config)
    f = lambda k: sd[k].detach().to(torch.float64 if sd[k].dtype == torch.float64 else torch.float32)
    t = _prefix(sd)
    s1 = QUICK_GELU if c["hidden_act"] == "quick_gelu" else 1.0
    out = dict(tok=f(t + "embeddings.token_embedding.weight"), pos=f(t + "embeddings.position_embedding.weight"),
               fin_g=f(t + "final_layer_norm.weight"), fin_b=f(t + "final_layer_norm.bias"),
               layers=cc.pack_layers(sd, t, c["num_hidden_layers"], f, fc1_scale=s1))
    if "text_projection.weight" in sd:
        out["proj_w"] = f("text_projection.weight")
    return out


def pooled_index(ids: torch.Tensor, eos_token_id: int) -> torch.Tensor:
    """The position of the pooled row of every sample [B]: both branches of CLIPTextModel.forward."""
    if eos_token_id == 2:
        return ids.argmax(-1)
    return (ids == eos_token_id).int().argmax(-1)


def _layers_needed(L: int, want, hidden_idx) -> tuple:
    """(hidden-state index k in [0, L] or None, layers to run)."""
    unknown = set(want) - set(OUTPUTS)
    if unknown or not want:
        raise ValueError(f"want = {tuple(want)!r}: a non-empty subset of {OUTPUTS}")
    k = None
    if "hidden_state" in want:
        if hidden_idx is None or not -(L + 1) <= hidden_idx <= L:
            raise ValueError(f"hidden_idx = {hidden_idx}: hidden_states has {L + 1} entries")
        k = hidden_idx % (L + 1)
    return k, (k if set(want) == {"hidden_state"} else L)


def clip_text_forward_torch(packed: dict, ids: torch.Tensor, config, want=("last_hidden_state",), hidden_idx: Optional[int] = None) -> dict:
    """The executor's launch sequence in torch, in the packed tensors' dtype: {name: tensor} for the names in `want`
    (hidden_state = HF's hidden_states[hidden_idx], the residual stream after that many layers)."""
    c = config_fields(config)
    F = torch.nn.functional
    B, N = ids.shape
    D, H, L, eps = c["hidden_size"], c["num_attention_heads"], c["num_hidden_layers"], float(c["layer_norm_eps"])
    k, nlayers = _layers_needed(L, want, hidden_idx)
    act, alpha = (F.silu, 1.0 / QUICK_GELU) if c["hidden_act"] == "quick_gelu" else (F.gelu, 1.0)
    h = (packed["tok"][ids.clamp(0, c["vocab_size"] - 1)] + packed["pos"][:N]).reshape(B * N, D)
    keep = torch.ones(N, N, dtype=torch.bool, device=ids.device).tril()
    out = {}
    if k == 0:
        out["hidden_state"] = h.reshape(B, N, D)
    for i, lay in enumerate(packed["layers"][:nlayers]):
        x = F.layer_norm(h, (D,), lay["ln1_g"], lay["ln1_b"], eps)
        q, kk, v = (t.reshape(B, N, H, D_HEAD).permute(0, 2, 1, 3) for t in (x @ lay["qkv_w"].t() + lay["qkv_b"]).split(D, 1))
        s = (q @ kk.transpose(-1, -2) * D_HEAD ** -0.5).masked_fill(~keep, float("-inf"))
        a = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(B * N, D)
        h = h + a @ lay["o_w"].t() + lay["o_b"]
        x = F.layer_norm(h, (D,), lay["ln2_g"], lay["ln2_b"], eps)
        m = act(x @ lay["fc1_w"].t() + lay["fc1_b"]) * alpha
        h = h + m @ lay["fc2_w"].t() + lay["fc2_b"]
        if k == i + 1:
            out["hidden_state"] = h.reshape(B, N, D)
    if nlayers == L and set(want) != {"hidden_state"}:
        last = F.layer_norm(h, (D,), packed["fin_g"], packed["fin_b"], eps)
        pooled = last[torch.arange(B, device=ids.device) * N + pooled_index(ids, c["eos_token_id"])]
        out.update(last_hidden_state=last.reshape(B, N, D), pooler_output=pooled)
        if "text_embeds" in want:
            out["text_embeds"] = pooled @ packed["proj_w"].t()
    return {n: out[n] for n in want}


_WEIGHTS = ("proj_w", "qkv_w", "o_w", "fc1_w", "fc2_w")       # engine dtype; everything else stays fp32


class ClipTextE(cc.ClipExecutor):
    """CLIPTextModel(.WithProjection).forward: input_ids [B, N] int64 -> the outputs named in `want`."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], config, dtype, device=None):
        super().__init__(check_config(config), state_dict, dtype, device)
        c = self.cfg
        self.scale = float(D_HEAD) ** -0.5
        self.quick = c["hidden_act"] == "quick_gelu"
        self.w = self._to_device(self.pack(state_dict), _WEIGHTS)
        assert tuple(self.w["pos"].shape) == (c["max_position_embeddings"], self.D) and self.w["tok"].shape[0] == c["vocab_size"]
        self.forwards = 0                                # forwards that ran on the engine (what the tests read)

    def pack(self, state_dict: Dict[str, torch.Tensor]) -> dict:
        return pack_clip_text(state_dict, self.cfg)

    def load(self, state_dict: Dict[str, torch.Tensor]):
        if ("text_projection.weight" in state_dict) != ("proj_w" in self.w):
            raise ValueError("the state dict gains or loses text_projection.weight: build a new executor")
        super().load(state_dict)

    def _buffers(self, B: int, N: int) -> dict:
        b = self._buf.get((B, N))
        if b is None:
            D, F = self.D, self.F
            new = lambda r, c, dt=None: torch.empty((r, c), dtype=dt or self.dtype, device=self.device)
            f32 = torch.float32
            b = dict(ids=torch.zeros((B, N), dtype=torch.long, device=self.device), h=[new(B * N, D, f32) for _ in range(3)],
                     hid=new(B * N, D, f32), x=new(B * N, D), qkv=new(B * N, 3 * D), a=new(B * N, D), m=new(B * N, F),
                     last=new(B * N, D, f32), pooled=new(B, D, f32), base=torch.arange(B, device=self.device) * N,
                     rows=torch.zeros(B, dtype=torch.long, device=self.device))
            if self.dtype != f32:          # LayerNorm's fp32 output before its one rounding; the pooled rows as the projection reads them
                b.update(x32=new(B * N, D, f32), pooled_lo=new(B, D))
            if "proj_w" in self.w:
                b["embeds"] = new(B, self.w["proj_w"].shape[0], torch.float32)
            self._buf[(B, N)] = b
        return b

    @torch.no_grad()
    def forward(self, input_ids: torch.Tensor, want=("last_hidden_state",), hidden_idx: Optional[int] = None) -> dict:
        """{name: tensor} for the names in `want`, all fp32: last_hidden_state [B, N, D], pooler_output [B, D], text_embeds
        [B, projection_dim], hidden_state = HF's hidden_states[hidden_idx] [B, N, D] (only the layers it needs run when nothing
        else is wanted).  All are the executor's own buffers: the next forward at the same (B, N) overwrites them."""
        if input_ids.dim() != 2 or input_ids.dtype != torch.long:
            raise ValueError(f"input_ids: an int64 [B, N] tensor, not {input_ids.dtype} {tuple(input_ids.shape)}")
        B, N = input_ids.shape
        c = self.cfg
        if not 1 <= N <= c["max_position_embeddings"] or B < 1:
            raise ValueError(f"input_ids {tuple(input_ids.shape)}: 1 .. {c['max_position_embeddings']} tokens (max_position_embeddings)")
        k, nlayers = _layers_needed(self.L, want, hidden_idx)
        if "text_embeds" in want and "proj_w" not in self.w:
            raise ValueError("text_embeds: the state dict has no text_projection.weight")
        if not input_ids.is_cuda and (int(input_ids.min()) < 0 or int(input_ids.max()) >= c["vocab_size"]):
            raise ValueError(f"input_ids outside [0, {c['vocab_size']})")          # (device ids: the kernel clamps)
        D, H, w, b = self.D, self.H, self.w, self._buffers(B, N)
        ids = b["ids"]
        ids.copy_(input_ids)
        x, qkv, a, m = b["x"], b["qkv"], b["a"], b["m"]
        mixed = self.dtype != torch.float32
        act, alpha = (hip.ACT_SILU, 1.0 / QUICK_GELU) if self.quick else (hip.ACT_GELU, 1.0)

        def norm(src, g, bt):              # LayerNorm of the fp32 stream -> x in the engine dtype
            if mixed:
                return hip.pack2d(hip.layernorm_fwd(src, b["x32"], g, bt, self.eps), x)
            return hip.layernorm_fwd(src, x, g, bt, self.eps)

        attend = lambda qkv: hip.attention_causal(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], a, B, H, N, D_HEAD, self.scale)
        layer = lambda lay, src, mid, out: cc.encoder_layer(lay, src, mid, out, qkv, m, norm=norm, attend=attend, act=act, alpha=alpha,
                                                            atomic=mixed)

        cur = b["hid"] if k == 0 and not mixed else b["h"][0]
        hip.clip_text_embed(ids, w["tok"], w["pos"], cur)
        if mixed and k == 0:
            hip.axpby(cur, b["hid"], 1.0, 0.0)
        for i, lay in enumerate(w["layers"][:nlayers]):
            if mixed:                      # the stream is updated in place: cur += branch, twice
                layer(lay, cur, cur, cur)
                if k == i + 1:
                    hip.axpby(cur, b["hid"], 1.0, 0.0)
            else:
                out = b["hid"] if k == i + 1 else (b["h"][1] if cur is b["h"][0] else b["h"][0])
                cur = layer(lay, cur, b["h"][2], out)
        res = {}
        if k is not None:
            res["hidden_state"] = b["hid"].view(B, N, D)
        if set(want) != {"hidden_state"}:
            hip.layernorm_fwd(cur, b["last"], w["fin_g"], w["fin_b"], self.eps)
            res["last_hidden_state"] = b["last"].view(B, N, D)
            if "pooler_output" in want or "text_embeds" in want:
                torch.add(b["base"], pooled_index(ids, c["eos_token_id"]), out=b["rows"])
                hip.gather_rows(b["last"], b["rows"], b["pooled"])
                res["pooler_output"] = b["pooled"]
            if "text_embeds" in want:
                hip.gemm(hip.pack2d(b["pooled"], b["pooled_lo"]) if mixed else b["pooled"], w["proj_w"], b["embeds"], out_f32=True)
                res["text_embeds"] = b["embeds"]
        self.forwards += 1
        return {n: res[n] for n in want}

    __call__ = forward
