"""What the style-transfer app does around the model (reference app/gradio_ctrlora_style_transfer.py), as library code.

  ImageProjModel        (:93-111) CLIP image embeds -> `clip_extra_context_tokens` image-prompt tokens (Linear + LayerNorm);
                        the unconditional branch uses ImageProjModel(zeros) (:405-409)
  ip_layer_names        the 16 IPCrossAttention layers in the checkpoint's order (what the app's ip_layers.txt lists)
  ip_adapter_state      (:114-129 change_key) IP-Adapter checkpoint keys -> the UNet's to_k_ip / to_v_ip: processor
                        indices 1, 3, ..., 31 go to the layers in order
  ip_scale_state        (:131-172 load_state_dict_ip) the per-layer ip_scale entries of the app's three targets
  CLIPVisionEncoder     (:387-391) the IP-Adapter image encoder, CLIPVisionModelWithProjection, built from its config; on a GPU
                        under no_grad it runs on the HIP engine (ctrlora_amd/engine/vit.py)
  CLIPTextEncoder       (:395-400) the text side of the same CLIP, CLIPTextModelWithProjection, built from its config; on a GPU
                        under no_grad it runs on the HIP engine (ctrlora_amd/engine/clip_text.py)
  style_image_tokens    (:392-409) style image -> CLIPImageProcessor -> image_embeds [- scale * the negative content prompt's
                        text_embeds (:401-403)] -> ImageProjModel: the conditional and the unconditional (zero-embeds) tokens
                        that go in as c_ip
"""
import os
from types import SimpleNamespace
from typing import Dict, List

import torch
import torch.nn as nn

from ctrlora_amd.engine import clip_text, vit
from ctrlora_amd.engine.clip_common import ExecutorHost

IP_SCALE_TARGETS = {
    # every IPCrossAttention of the SD1.5 UNet
    "Load original IP-Adapter": ["input_blocks.1.1", "input_blocks.2.1", "input_blocks.4.1", "input_blocks.5.1",
                                 "input_blocks.7.1", "input_blocks.8.1", "middle_block.1"]
                                + [f"output_blocks.{i}.1" for i in range(3, 12)],
    "Load only style blocks": ["output_blocks.3.1", "output_blocks.4.1", "output_blocks.5.1"],
    "Load style+layout block": ["input_blocks.7.1", "input_blocks.8.1", "output_blocks.3.1", "output_blocks.4.1",
                                "output_blocks.5.1"],
}


class ImageProjModel(nn.Module):
    def __init__(self, cross_attention_dim=768, clip_embeddings_dim=1024, clip_extra_context_tokens=4):
        super().__init__()
        self.generator = None
        self.cross_attention_dim = cross_attention_dim
        self.clip_extra_context_tokens = clip_extra_context_tokens
        self.proj = nn.Linear(clip_embeddings_dim, clip_extra_context_tokens * cross_attention_dim)
        self.norm = nn.LayerNorm(cross_attention_dim)

    def forward(self, image_embeds):
        tokens = self.proj(image_embeds).reshape(-1, self.clip_extra_context_tokens, self.cross_attention_dim)
        return self.norm(tokens)


def ip_layer_names(unet: nn.Module, prefix: str = "model.diffusion_model.") -> List[str]:
    """Module names (`prefix` + '...attn2') of the UNet's IPCrossAttention layers in IP-Adapter checkpoint order: the
    encoder's and the decoder's in module order, then the middle block's (the diffusers processor order -- down, up, mid
    -- that the app's ip_layers.txt follows)."""
    from ldm.modules.attention_ip import IPCrossAttention
    names = [n for n, m in unet.named_modules() if isinstance(m, IPCrossAttention)]
    return [prefix + n for n in names if not n.startswith("middle_block.")] + \
           [prefix + n for n in names if n.startswith("middle_block.")]


def ip_adapter_state(ip_state: Dict[str, torch.Tensor], layer_names: List[str]) -> Dict[str, torch.Tensor]:
    """An IP-Adapter checkpoint's 'ip_adapter' dict ('{n}.to_k_ip.weight', '{n}.to_v_ip.weight') -> state-dict entries of
    the UNet layers: layer i takes processor 2 i + 1 (the attn2 processors; the even ones are the self-attentions')."""
    out = {}
    for i, name in enumerate(layer_names):
        for w in ("to_k_ip", "to_v_ip"):
            out[f"{name}.{w}.weight"] = ip_state[f"{2 * i + 1}.{w}.weight"]
    return out


def ip_scale_state(target: str, ip_scale: float, prefix: str = "model.diffusion_model.") -> Dict[str, torch.Tensor]:
    """The ip_scale entries load_state_dict_ip loads for `target` (one of IP_SCALE_TARGETS); other layers keep theirs."""
    return {f"{prefix}{b}.transformer_blocks.0.attn2.ip_scale": torch.tensor(ip_scale) for b in IP_SCALE_TARGETS[target]}


# OpenCLIP ViT-H/14 in HF layout: the image encoder IP-Adapter for SD1.5 ships (its image_encoder/config.json)
VIT_H_14 = dict(hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=16, num_channels=3,
                image_size=224, patch_size=14, hidden_act="gelu", layer_norm_eps=1e-5, projection_dim=1024)


def _hf_config(cls, default: dict, sub_key: str, config):
    """config as a `cls` (CLIPVisionConfig / CLIPTextConfig): None is `default`; a model directory gives its config.json
    only (the `sub_key` entry where the file is a whole CLIPConfig)."""
    if config is None:
        return cls(**default)
    if isinstance(config, cls):
        return config
    if isinstance(config, dict):
        return cls(**config)
    if isinstance(config, (str, os.PathLike)) and os.path.isdir(config):
        import json
        with open(os.path.join(config, "config.json")) as f:
            d = json.load(f)
        d = d.get(sub_key, d)
        known = cls().to_dict()
        return cls(**{k: v for k, v in d.items() if k in known and k not in ("model_type", "transformers_version")})
    raise TypeError(f"config: a {cls.__name__}, a dict or a directory with config.json, not {type(config).__name__}")


def _vision_config(config):
    from transformers import CLIPVisionConfig
    return _hf_config(CLIPVisionConfig, VIT_H_14, "vision_config", config)


class CLIPVisionEncoder(ExecutorHost, nn.Module):
    """CLIPVisionModelWithProjection under HF's own state-dict keys (`vision_model.*`, `visual_projection.weight`), so an
    IP-Adapter image_encoder/ checkpoint loads with strict=True.  Built from a config (default: ViT-H/14), never from a hub
    name: nothing is downloaded, the weights come from load_state_dict.  On a GPU under no_grad, with a config the executor
    covers (ctrlora_amd/engine/vit.py: check_config), forward runs on the HIP engine in `engine_dtype` (bf16 unless
    set_engine_dtype / CTRLORA_ENGINE_DTYPE says fp32); otherwise (CPU, autograd, other configs) it is the plain HF module."""
    ENGINE_SLOT, ENGINE_CLASS = "_vit", vit.ClipVisionE

    def __init__(self, config=None):
        super().__init__()
        from transformers import CLIPVisionModelWithProjection
        self.config = _vision_config(config)
        hf = CLIPVisionModelWithProjection(self.config).eval()
        self.vision_model, self.visual_projection = hf.vision_model, hf.visual_projection      # HF's keys, no extra prefix
        self.__dict__["_hf"] = hf                                                              # (not a registered child)
        self._init_engine_host()

    def _on_engine(self, pixel_values):
        return (self.use_engine and pixel_values.is_cuda and not torch.is_grad_enabled() and vit.supported(self.config)
                and tuple(pixel_values.shape[1:]) == (self.config.num_channels, self.config.image_size, self.config.image_size))

    def forward(self, pixel_values, output_hidden_states=False):
        """An object with .image_embeds [B, projection_dim] (and .hidden_states when asked: HF's tuple from the plain module;
        from the engine a tuple whose [-2] is the penultimate hidden state -- the one entry IP-Adapter-Plus reads -- and
        None elsewhere)."""
        if not self._on_engine(pixel_values):
            return self._hf(pixel_values=pixel_values, output_hidden_states=output_hidden_states)
        if not output_hidden_states:
            return SimpleNamespace(image_embeds=self.engine().forward(pixel_values).clone(), hidden_states=None)
        emb, pen = self.engine().forward(pixel_values, output_hidden_states=True)
        hs = [None] * (self.config.num_hidden_layers + 1)
        hs[-2] = pen.float()
        return SimpleNamespace(image_embeds=emb.clone(), hidden_states=tuple(hs))


# the text tower of the same OpenCLIP ViT-H/14 (laion/CLIP-ViT-H-14-laion2B-s32B-b79K in HF layout, the model the app loads)
VIT_H_14_TEXT = dict(vocab_size=49408, hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16,
                     max_position_embeddings=77, hidden_act="gelu", layer_norm_eps=1e-5, projection_dim=1024)


def _text_config(config):
    from transformers import CLIPTextConfig
    return _hf_config(CLIPTextConfig, VIT_H_14_TEXT, "text_config", config)


class CLIPTextEncoder(ExecutorHost, nn.Module):
    """CLIPTextModelWithProjection under HF's own state-dict keys (`text_model.*`, `text_projection.weight`).  Built from a
    config (default: the ViT-H/14 text tower), never from a hub name: nothing is downloaded, the weights come from
    load_state_dict.  On a GPU under no_grad, with a config the executor covers (ctrlora_amd/engine/clip_text.py: check_config)
    and no padding mask, forward runs on the HIP engine in `engine_dtype` (bf16 unless set_engine_dtype / CTRLORA_ENGINE_DTYPE
    says fp32); otherwise (CPU, autograd, other configs, use_engine = False) it is the plain HF module."""
    ENGINE_SLOT, ENGINE_CLASS = "_txt", clip_text.ClipTextE

    def __init__(self, config=None):
        super().__init__()
        from transformers import CLIPTextModelWithProjection
        self.config = _text_config(config)
        hf = CLIPTextModelWithProjection(self.config).eval()
        self.text_model, self.text_projection = hf.text_model, hf.text_projection              # HF's keys, no extra prefix
        self.__dict__["_hf"] = hf                                                              # (not a registered child)
        self._init_engine_host()

    def _on_engine(self, input_ids, attention_mask):
        return (self.use_engine and input_ids.is_cuda and not torch.is_grad_enabled() and clip_text.supported(self.config, attention_mask)
                and input_ids.dim() == 2 and 1 <= input_ids.shape[1] <= self.config.max_position_embeddings)

    def forward(self, input_ids, attention_mask=None):
        """An object with .text_embeds [B, projection_dim] and .last_hidden_state [B, N, hidden_size] (fresh tensors in the
        parameters' dtype)."""
        if not self._on_engine(input_ids, attention_mask):
            return self._hf(input_ids=input_ids, attention_mask=attention_mask)
        out = self.engine().forward(input_ids, want=("text_embeds", "last_hidden_state"))
        pdt = next(self.parameters()).dtype
        return SimpleNamespace(text_embeds=out["text_embeds"].to(pdt, copy=True), last_hidden_state=out["last_hidden_state"].to(pdt, copy=True))


def style_image_tokens(encoder, image_proj, images, processor=None, neg_content_embeds=None, neg_content_scale=1.0):
    """(tokens, uncond_tokens), each [B, clip_extra_context_tokens, cross_attention_dim]: what the app computes from the style
    image (:392-409) -- processor(images).pixel_values -> encoder(...).image_embeds -> image_proj(embeds) and
    image_proj(zeros_like(embeds)) -- ready to be passed as c_ip in cond / un_cond.  images: a PIL image or a uint8 HWC
    array, or a list of them.  processor: a CLIPImageProcessor (default: CLIPImageProcessor()).  neg_content_embeds: the
    text_embeds of a negative content prompt (CLIPTextEncoder): neg_content_scale times them is taken off the image embeds
    before image_proj (:401-403); the unconditional tokens are the same either way."""
    if processor is None:
        from transformers import CLIPImageProcessor
        processor = CLIPImageProcessor()
    dev = next(encoder.parameters()).device
    pixel_values = processor(images=images, return_tensors="pt").pixel_values.to(dev)
    with torch.no_grad():
        embeds = encoder(pixel_values).image_embeds
        pdt = next(image_proj.parameters()).dtype
        embeds = embeds.to(device=next(image_proj.parameters()).device, dtype=pdt)
        if neg_content_embeds is not None:
            embeds = embeds - neg_content_scale * neg_content_embeds.to(device=embeds.device, dtype=pdt)
        return image_proj(embeds), image_proj(torch.zeros_like(embeds))
