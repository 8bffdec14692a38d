"""SD1.5 UNet with IP-Adapter cross-attentions (API of the reference's ldm/modules/diffusionmodules/openaimodel_ip.py).

The same module tree as openaimodel.UNetModel, built from the transformer of ldm/modules/attention_ip.py: `attn2` of every
transformer block is an IPCrossAttention, so the state dict gains `to_k_ip`, `to_v_ip` and `ip_scale` in each of the 16
cross-attentions.  The HIP executor (ctrlora_amd.engine.UNetE) recognises those keys.
"""
from ldm.modules.attention_ip import SpatialTransformer
from ldm.modules.diffusionmodules.openaimodel import (Downsample, EngineHost, ResBlock, TimestepBlock,  # noqa: F401
                                                      TimestepEmbedSequential, Upsample)
from ldm.modules.diffusionmodules.openaimodel import UNetModel as _PlainUNet


class UNetModel(_PlainUNet):
    st_cls = SpatialTransformer
