"""Parameter containers of the IP-Adapter UNet transformer (API of the reference's ldm/modules/attention_ip.py).

IPCrossAttention (:196-289) is CrossAttention plus frozen `to_k_ip` / `to_v_ip` projections of the image-prompt tokens
and an `ip_scale` buffer (default 0, part of the state dict).  Its forward is
    to_out(softmax(s q k_txt^T) v_txt + ip_scale * softmax(s q k_ip^T) v_ip)
with two separate softmaxes; the HIP engine runs it as one launch (cl_attention_fwd_ip, ctrlora_amd/engine/blocks.py
AttnE).  Only `attn2` of every BasicTransformerBlock is an IPCrossAttention (:422-520); `attn1` stays plain.
"""
import torch
import torch.nn as nn

from ldm.modules.attention import BasicTransformerBlock as _PlainBlock
from ldm.modules.attention import CrossAttention, FeedForward, GEGLU, SpatialTransformer as _PlainST, _EngineExecuted

__all__ = ["CrossAttention", "FeedForward", "GEGLU", "IPCrossAttention", "BasicTransformerBlock", "SpatialTransformer"]


class IPCrossAttention(_EngineExecuted):
    def __init__(self, query_dim, context_dim=None, heads=8, dim_head=64, dropout=0.):
        super().__init__()
        inner = dim_head * heads
        context_dim = query_dim if context_dim is None else context_dim
        self.scale = dim_head ** -0.5
        self.heads = heads
        self.to_q = nn.Linear(query_dim, inner, bias=False)
        self.to_k = nn.Linear(context_dim, inner, bias=False)
        self.to_v = nn.Linear(context_dim, inner, bias=False)
        self.to_k_ip = nn.Linear(context_dim, inner, bias=False)
        self.to_v_ip = nn.Linear(context_dim, inner, bias=False)
        self.register_buffer("ip_scale", torch.tensor(0.0))
        self.to_out = nn.Sequential(nn.Linear(inner, query_dim), nn.Dropout(dropout))


class BasicTransformerBlock(_PlainBlock):
    def __init__(self, dim, n_heads, d_head, dropout=0., context_dim=None, gated_ff=True, checkpoint=True,
                 disable_self_attn=False):
        super().__init__(dim, n_heads, d_head, dropout, context_dim, gated_ff, checkpoint, disable_self_attn)
        self.attn2 = IPCrossAttention(query_dim=dim, context_dim=context_dim, heads=n_heads, dim_head=d_head,
                                      dropout=dropout)


class SpatialTransformer(_PlainST):
    """attention.SpatialTransformer with the IP-Adapter block (depth 1, conv proj_in / proj_out: checked by the parent)."""

    def __init__(self, in_channels, n_heads, d_head, depth=1, dropout=0., context_dim=None, disable_self_attn=False,
                 use_linear=False, use_checkpoint=True):
        super().__init__(in_channels, n_heads, d_head, depth, dropout, context_dim, disable_self_attn, use_linear,
                         use_checkpoint)
        if isinstance(context_dim, (list, tuple)):
            context_dim = context_dim[0]
        self.transformer_blocks = nn.ModuleList(
            [BasicTransformerBlock(n_heads * d_head, n_heads, d_head, dropout=dropout, context_dim=context_dim,
                                   disable_self_attn=disable_self_attn)])
