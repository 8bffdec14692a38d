"""What the style-transfer app does around the model (reference app/gradio_ctrlora_style_transfer.py), as library code.

  ImageProjModel        (:93-111) CLIP image embeds -> `clip_extra_context_tokens` image-prompt tokens (Linear + LayerNorm);
                        the unconditional branch uses ImageProjModel(zeros) (:405-409)
  ip_layer_names        the 16 IPCrossAttention layers in the checkpoint's order (what the app's ip_layers.txt lists)
  ip_adapter_state      (:114-129 change_key) IP-Adapter checkpoint keys -> the UNet's to_k_ip / to_v_ip: processor
                        indices 1, 3, ..., 31 go to the layers in order
  ip_scale_state        (:131-172 load_state_dict_ip) the per-layer ip_scale entries of the app's three targets
"""
from typing import Dict, List

import torch
import torch.nn as nn

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
