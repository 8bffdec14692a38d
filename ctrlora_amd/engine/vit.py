"""CLIP vision encoder (the image encoder of IP-Adapter for SD1.5: OpenCLIP ViT-H/14 in HF layout) on the HIP kernels.

Where the reference calls it: the style app encodes the style image once per request
(app/gradio_ctrlora_style_transfer.py:392-409: CLIPImageProcessor -> CLIPVisionModelWithProjection(...).image_embeds ->
ImageProjModel).  Modules restated (behaviour, not code; transformers/models/clip/modeling_clip.py):

  CLIPVisionEmbeddings  :138-218  patch_embedding (stride-P P x P conv, no bias) as patch rows x one linear product,
                                  class embedding in front, + position_embedding (cl_vit_patch_rows, cl_vit_tokens)
  CLIPVisionModel       :594-656  pre_layrnorm (the upstream spelling) -> encoder -> post_layernorm of the class rows
  CLIPEncoderLayer      :353-384  pre-LN: x + out_proj(attn(LN1 x)); x + fc2(gelu(fc1(LN2 x)))
  CLIPAttention         :280-335  no mask: softmax(q k^T d^-1/2) v, q | k | v as ONE product (q pre-scaled in bf16)
  CLIPMLP               :338-350  fc1 with the exact GELU in the product's epilogue (cl_gemm act 4), fc2 with the residual
  CLIPVisionModelWithProjection :898-957  visual_projection (no bias) of the pooled class rows -> image_embeds

Inference only.  Activations are token-major [B*T, D] in the engine dtype; every buffer is allocated once per batch size and
reused, so a forward is a fixed launch sequence over fixed addresses (hipGraph-capturable; load() refreshes the packed weights
in place).  The packing (pack_clip_vision) and its torch restatement of the patch rows run on the CPU.
"""
from __future__ import annotations

from typing import Dict, List

import torch

from .. import hip
from .packing import rup

ATTN_D_HEADS = (8, 16, 32, 40, 80, 160)      # csrc/attention_fwd.hip: dispatch_dh, csrc/attention_tr.hip: attn_fwd_tr
K_GRAIN = 32                                 # cl_gemm's K granularity in bf16 (16 in fp32): 3 * 14 * 14 = 588 -> 608

_FIELDS = ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "num_channels", "image_size",
           "patch_size", "projection_dim", "layer_norm_eps", "hidden_act")


def config_fields(config) -> dict:
    """The fields of a CLIPVisionConfig (or a dict with the same names) that shape the encoder."""
    get = (lambda k: config[k]) if isinstance(config, dict) else (lambda k: getattr(config, k))
    return {k: get(k) for k in _FIELDS}


def check_config(config) -> dict:
    """config_fields(config), or ValueError naming the field the executor does not cover."""
    c = config_fields(config)
    if c["hidden_act"] != "gelu":
        raise ValueError(f"hidden_act = {c['hidden_act']!r}: the executor has the exact (erf) GELU epilogue only")
    if c["image_size"] % c["patch_size"]:
        raise ValueError(f"image_size = {c['image_size']} is not a multiple of patch_size = {c['patch_size']}")
    D, H = c["hidden_size"], c["num_attention_heads"]
    if D % H or D // H not in ATTN_D_HEADS:
        raise ValueError(f"num_attention_heads = {H} with hidden_size = {D}: d_head {D / H:g} is not one of {ATTN_D_HEADS}")
    for k in ("hidden_size", "intermediate_size"):
        if c[k] % K_GRAIN:
            raise ValueError(f"{k} = {c[k]} is not a multiple of {K_GRAIN} (K granularity of the products)")
    if c["projection_dim"] % 8:
        raise ValueError(f"projection_dim = {c['projection_dim']} is not a multiple of 8")
    return c


def supported(config) -> bool:
    try:
        check_config(config)
        return True
    except ValueError:
        return False


def state_keys(config) -> List[str]:
    """The state-dict keys of an HF CLIPVisionModelWithProjection with this config (what pack_clip_vision reads)."""
    c = config_fields(config)
    v = "vision_model."
    keys = [v + "embeddings.class_embedding", v + "embeddings.patch_embedding.weight", v + "embeddings.position_embedding.weight",
            v + "pre_layrnorm.weight", v + "pre_layrnorm.bias"]
    for i in range(c["num_hidden_layers"]):
        p = f"{v}encoder.layers.{i}."
        for m in ("self_attn.k_proj", "self_attn.v_proj", "self_attn.q_proj", "self_attn.out_proj", "layer_norm1", "mlp.fc1", "mlp.fc2",
                  "layer_norm2"):
            keys += [p + m + ".weight", p + m + ".bias"]
    return keys + [v + "post_layernorm.weight", v + "post_layernorm.bias", "visual_projection.weight"]


def patch_kpad(config) -> int:
    c = config_fields(config)
    return rup(c["num_channels"] * c["patch_size"] ** 2, K_GRAIN)


def patch_rows_torch(pixel_values: torch.Tensor, P: int, Kpad: int) -> torch.Tensor:
    """What cl_vit_patch_rows writes, in torch: [B, C, S, S] -> [B (S/P)^2, Kpad], columns (c, py, px), zero pad."""
    B, C, S, _ = pixel_values.shape
    G = S // P
    rows = pixel_values.reshape(B, C, G, P, G, P).permute(0, 2, 4, 1, 3, 5).reshape(B * G * G, C * P * P)
    return torch.nn.functional.pad(rows, (0, Kpad - C * P * P))


def pack_clip_vision(sd: Dict[str, torch.Tensor], config) -> dict:
    """fp32 tensors in the layout the executor's products read (on the state dict's device): the patch weight flattened
    (c, py, px) and zero-padded to patch_kpad columns, q | k | v of a layer concatenated into one [3D, D] weight / [3D] bias."""
    c = config_fields(config)
    f = lambda k: sd[k].detach().float()
    v = "vision_model."
    D, Kp = c["hidden_size"], patch_kpad(config)
    pw = f(v + "embeddings.patch_embedding.weight").reshape(D, -1)
    out = dict(patch_w=torch.nn.functional.pad(pw, (0, Kp - pw.shape[1])), cls=f(v + "embeddings.class_embedding").reshape(D),
               pos=f(v + "embeddings.position_embedding.weight"), pre_g=f(v + "pre_layrnorm.weight"), pre_b=f(v + "pre_layrnorm.bias"),
               post_g=f(v + "post_layernorm.weight"), post_b=f(v + "post_layernorm.bias"), proj_w=f("visual_projection.weight"),
               layers=[])
    for i in range(c["num_hidden_layers"]):
        p = f"{v}encoder.layers.{i}."
        a = p + "self_attn."
        out["layers"].append(dict(
            ln1_g=f(p + "layer_norm1.weight"), ln1_b=f(p + "layer_norm1.bias"),
            qkv_w=torch.cat([f(a + n + "_proj.weight") for n in "qkv"], 0), qkv_b=torch.cat([f(a + n + "_proj.bias") for n in "qkv"], 0),
            o_w=f(a + "out_proj.weight"), o_b=f(a + "out_proj.bias"),
            ln2_g=f(p + "layer_norm2.weight"), ln2_b=f(p + "layer_norm2.bias"),
            fc1_w=f(p + "mlp.fc1.weight"), fc1_b=f(p + "mlp.fc1.bias"), fc2_w=f(p + "mlp.fc2.weight"), fc2_b=f(p + "mlp.fc2.bias")))
    return out


_WEIGHTS = ("patch_w", "proj_w", "qkv_w", "o_w", "fc1_w", "fc2_w")       # engine dtype; everything else stays fp32


class ClipVisionE:
    """CLIPVisionModelWithProjection.forward: pixel_values (B, C, S, S) fp32 -> image_embeds (B, projection_dim) fp32."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], config, dtype, device=None):
        self.cfg = check_config(config)                 # (before anything touches the GPU: the refusals need none)
        if dtype not in (torch.bfloat16, torch.float32):
            raise ValueError(f"dtype = {dtype}: the engine stores bf16 or fp32")
        hip.lib()
        c = self.cfg
        self.dtype = dtype
        self.device = torch.device(device if device is not None else next(iter(state_dict.values())).device)
        self.D, self.H, self.F, self.L = c["hidden_size"], c["num_attention_heads"], c["intermediate_size"], c["num_hidden_layers"]
        self.P, self.S, self.C = c["patch_size"], c["image_size"], c["num_channels"]
        self.T = (self.S // self.P) ** 2 + 1
        self.dh = self.D // self.H
        self.scale = float(self.dh) ** -0.5
        self.eps = float(c["layer_norm_eps"])
        self.Kpad = patch_kpad(c)
        from .blocks import PRESCALE_Q
        self.prescaled = PRESCALE_Q and dtype == torch.bfloat16       # CL_ATTN_Q_PRESCALED: as the UNet's self-attentions
        self.w = self._to_device(pack_clip_vision(state_dict, c))
        assert tuple(self.w["pos"].shape) == (self.T, self.D), (tuple(self.w["pos"].shape), self.T, self.D)
        self._buf: Dict[int, dict] = {}

    def _to_device(self, packed: dict) -> dict:
        mv = lambda k, t: t.to(device=self.device, dtype=self.dtype if k in _WEIGHTS else torch.float32).contiguous()
        out = {k: mv(k, t) for k, t in packed.items() if k != "layers"}
        out["layers"] = [{k: mv(k, t) for k, t in lay.items()} for lay in packed["layers"]]
        return out

    def load(self, state_dict: Dict[str, torch.Tensor]):
        """Refresh the packed weights in place (the address rule of engine/packing.py: a captured graph keeps replaying them)."""
        new = pack_clip_vision(state_dict, self.cfg)
        for k, t in new.items():
            if k != "layers":
                self.w[k].copy_(t)
        for old, lay in zip(self.w["layers"], new["layers"]):
            for k, t in lay.items():
                old[k].copy_(t)

    def _buffers(self, B: int) -> dict:
        b = self._buf.get(B)
        if b is None:
            D, T, F = self.D, self.T, self.F
            new = lambda r, c, dt=None: torch.empty((r, c), dtype=dt or self.dtype, device=self.device)
            b = dict(rows=new(B * (T - 1), self.Kpad), pe=new(B * (T - 1), D), h=[new(B * T, D) for _ in range(3)], x=new(B * T, D),
                     qkv=new(B * T, 3 * D), a=new(B * T, D), m=new(B * T, F), pooled=new(B, D),
                     embeds=new(B, self.cfg["projection_dim"], torch.float32))
            if self.dtype == torch.float32:       # the fp32 kernels' V^T scratch at a fixed address (hip.attention checks its shape)
                b["vt"] = torch.empty((B, D, rup(T, 64)), dtype=self.dtype, device=self.device)
            self._buf[B] = b
        return b

    @torch.no_grad()
    def forward(self, pixel_values: torch.Tensor, output_hidden_states: bool = False):
        """image_embeds [B, projection_dim] fp32; with output_hidden_states also the penultimate hidden state [B, T, D] in the
        engine dtype (HF's hidden_states[-2]: what IP-Adapter-Plus reads).  Both are the executor's own buffers: the next
        forward at the same batch size overwrites them."""
        B, C, S, S2 = pixel_values.shape
        if (C, S, S2) != (self.C, self.S, self.S):
            raise ValueError(f"pixel_values {tuple(pixel_values.shape)}: the model takes (B, {self.C}, {self.S}, {self.S}) (image_size)")
        px = pixel_values.to(device=self.device, dtype=torch.float32).contiguous()
        D, T, H, w, b = self.D, self.T, self.H, self.w, self._buffers(B)
        hA, hB, hC = b["h"]
        x, qkv, a, m = b["x"], b["qkv"], b["a"], b["m"]
        # embeddings: patch rows -> patch product -> class row + position embedding; pre_layrnorm
        hip.vit_patch_rows(px, b["rows"], self.P)
        hip.gemm(b["rows"], w["patch_w"], b["pe"])
        hip.vit_tokens(b["pe"], w["cls"], w["pos"], hB, B)
        hip.layernorm_fwd(hB, hA, w["pre_g"], w["pre_b"], self.eps)
        qa = self.scale * 1.4426950408889634 if self.prescaled else 1.0
        for i, lay in enumerate(w["layers"]):
            out = hC if i == self.L - 1 else hA          # hA keeps the penultimate hidden state
            hip.layernorm_fwd(hA, x, lay["ln1_g"], lay["ln1_b"], self.eps)
            hip.gemm(x, lay["qkv_w"], qkv, bias=lay["qkv_b"], alpha=qa, alpha_n=D if self.prescaled else 0)
            q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
            hip.attention(q, k, v, a, None, B, H, T, T, self.dh, self.scale, q_prescaled=self.prescaled, vt=b.get("vt"))
            hip.gemm(a, lay["o_w"], hB, bias=lay["o_b"], residual=hA, beta=1.0)
            hip.layernorm_fwd(hB, x, lay["ln2_g"], lay["ln2_b"], self.eps)
            hip.gemm(x, lay["fc1_w"], m, bias=lay["fc1_b"], act=hip.ACT_GELU)
            hip.gemm(m, lay["fc2_w"], out, bias=lay["fc2_b"], residual=hB, beta=1.0)
        last = hC if self.L > 0 else hA
        # post_layernorm of the class rows only (row b T of every sample), then visual_projection
        hip.layernorm_fwd(last.view(B, T * D)[:, :D], b["pooled"], w["post_g"], w["post_b"], self.eps)
        hip.gemm(b["pooled"], w["proj_w"], b["embeds"], out_f32=True)
        if output_hidden_states:
            return b["embeds"], hA.view(B, T, D)
        return b["embeds"]

    __call__ = forward
