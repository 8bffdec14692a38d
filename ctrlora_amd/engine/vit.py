"""CLIP vision encoder (the image encoder of IP-Adapter for SD1.5: OpenCLIP ViT-H/14 in HF layout) on the HIP kernels.

Where the reference calls it: the style app encodes the style image once per request
(app/gradio_ctrlora_style_transfer.py:392-409: CLIPImageProcessor -> CLIPVisionModelWithProjection(...).image_embeds ->
ImageProjModel).  Modules restated (behaviour, not code; transformers/models/clip/modeling_clip.py):

  CLIPVisionEmbeddings  :138-218  patch_embedding (stride-P P x P conv, no bias) as patch rows x one linear product,
                                  class embedding in front, + position_embedding (cl_vit_patch_rows, cl_vit_tokens)
  CLIPVisionModel       :594-656  pre_layrnorm (the upstream spelling) -> encoder -> post_layernorm of the class rows
  CLIPEncoderLayer, CLIPAttention, CLIPMLP      the layer both towers walk: clip_common.py (encoder_layer, pack_layers).  Here:
                                  no mask (cl_attention_fwd*, q pre-scaled by the qkv product in bf16), the exact GELU in fc1's
                                  epilogue (cl_gemm act 4), the stream in the engine dtype over three rotating buffers
  CLIPVisionModelWithProjection :898-957  visual_projection (no bias) of the pooled class rows -> image_embeds

Inference only.  Activations are token-major [B*T, D] in the engine dtype; every buffer is allocated once per batch size and
reused, so a forward is a fixed launch sequence over fixed addresses (hipGraph-capturable; load() refreshes the packed weights
in place).  The packing (pack_clip_vision) and its torch restatement of the patch rows run on the CPU.
"""
from __future__ import annotations

from typing import Dict, List

import torch

from .. import hip
from . import clip_common as cc
from .clip_common import K_GRAIN
from .packing import rup

ATTN_D_HEADS = (8, 16, 32, 40, 80, 160)      # csrc/attention_fwd.hip: dispatch_dh, csrc/attention_tr.hip: attn_fwd_tr

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
    cc.check_d_head(c, ATTN_D_HEADS, f"one of {ATTN_D_HEADS}")
    cc.check_widths(c)
    return c


def supported(config) -> bool:
    return cc.supported(check_config, config)


def state_keys(config) -> List[str]:
    """The state-dict keys of an HF CLIPVisionModelWithProjection with this config (what pack_clip_vision reads)."""
    c = config_fields(config)
    v = "vision_model."
    keys = [v + "embeddings.class_embedding", v + "embeddings.patch_embedding.weight", v + "embeddings.position_embedding.weight",
            v + "pre_layrnorm.weight", v + "pre_layrnorm.bias"]
    keys += cc.layer_state_keys(v, c["num_hidden_layers"])
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
    return dict(patch_w=torch.nn.functional.pad(pw, (0, Kp - pw.shape[1])), cls=f(v + "embeddings.class_embedding").reshape(D),
               pos=f(v + "embeddings.position_embedding.weight"), pre_g=f(v + "pre_layrnorm.weight"), pre_b=f(v + "pre_layrnorm.bias"),
               post_g=f(v + "post_layernorm.weight"), post_b=f(v + "post_layernorm.bias"), proj_w=f("visual_projection.weight"),
               layers=cc.pack_layers(sd, v, c["num_hidden_layers"], f))


_WEIGHTS = ("patch_w", "proj_w", "qkv_w", "o_w", "fc1_w", "fc2_w")       # engine dtype; everything else stays fp32


class ClipVisionE(cc.ClipExecutor):
    """CLIPVisionModelWithProjection.forward: pixel_values (B, C, S, S) fp32 -> image_embeds (B, projection_dim) fp32."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], config, dtype, device=None):
        super().__init__(check_config(config), state_dict, dtype, device)
        c = self.cfg
        self.P, self.S, self.C = c["patch_size"], c["image_size"], c["num_channels"]
        self.T = (self.S // self.P) ** 2 + 1
        self.dh = self.D // self.H
        self.scale = float(self.dh) ** -0.5
        self.Kpad = patch_kpad(c)
        from .blocks import PRESCALE_Q
        self.prescaled = PRESCALE_Q and dtype == torch.bfloat16       # CL_ATTN_Q_PRESCALED: as the UNet's self-attentions
        self.w = self._to_device(self.pack(state_dict), _WEIGHTS)
        assert tuple(self.w["pos"].shape) == (self.T, self.D), (tuple(self.w["pos"].shape), self.T, self.D)

    def pack(self, state_dict: Dict[str, torch.Tensor]) -> dict:
        return pack_clip_vision(state_dict, self.cfg)

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
        qa, qn = (self.scale * 1.4426950408889634, D) if self.prescaled else (1.0, 0)
        norm = lambda src, g, bt: hip.layernorm_fwd(src, x, g, bt, self.eps)
        attend = lambda qkv: hip.attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], a, None, B, H, T, T, self.dh, self.scale,
                                           q_prescaled=self.prescaled, vt=b.get("vt"))
        for i, lay in enumerate(w["layers"]):            # hA keeps the penultimate hidden state
            cc.encoder_layer(lay, hA, hB, hC if i == self.L - 1 else hA, qkv, m, norm=norm, attend=attend, act=hip.ACT_GELU,
                             qkv_alpha=qa, qkv_alpha_n=qn)
        last = hC if self.L > 0 else hA
        # post_layernorm of the class rows only (row b T of every sample), then visual_projection
        hip.layernorm_fwd(last.view(B, T * D)[:, :D], b["pooled"], w["post_g"], w["post_b"], self.eps)
        hip.gemm(b["pooled"], w["proj_w"], b["embeds"], out_f32=True)
        if output_hidden_states:
            return b["embeds"], hA.view(B, T, D)
        return b["embeds"]

    __call__ = forward
