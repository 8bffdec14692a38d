"""Reference and same-storage comparator for the first-stage engine (ctrlora_amd/engine/vae.py).  Helpers only: nothing here is
collected, and nothing imports the GPU library.

REFERENCE.  An fp64 restatement, from the behaviour of ldm/modules/diffusionmodules/model.py (ResnetBlock :97-149, AttnBlock
:152-202, Downsample :80-84, Upsample :61-69, Encoder :452-543, Decoder :546-650) and ldm/models/autoencoder.py:70-84, of each
thing engine/vae.py builds: resblock(), attn(), downsample(), upsample(), conv_in / conv_out, the two weight transformations
(fold_conv_out: conv_out followed by quant_conv as ONE 3x3; post_quant_padded: the 1x1 post_quant_conv as a zero-padded 32 x 32
linear), encoder() and decoder().  Tensors are NCHW, the state dict has AutoencoderKL's keys; everything is evaluated in the
dtype of the tensors it is given (the tests feed fp64), with no cast anywhere.

COMPARATOR.  The same functions with Mode(round=True) round to the engine dtype exactly at the tensors the engine STORES in that
dtype between launches (read off engine/vae.py):

  every block     the GroupNorm (+ swish) outputs; every conv / linear output (the shortcut of a nin_shortcut block sits in the
                  output buffer before conv2 adds onto it: rounded once there, once after the add); the block output
  attention       hn, the fused q | k | v, P after the fp32 softmax of the fp32 scores (S is never rounded), a = P v, the output
  encoder         the image tokens (nchw_to_tok writes the engine dtype), conv_in, every block, the Downsample output, norm_out
  decoder         the latent tokens, post_quant, conv_in, every block, the Upsample output, norm_out

Not rounded: biases and norm parameters (fp32 in the engine), the fp32 moments / image that conv_out stores with out_f32.  Weights
are read rounded (the packed copies); the folded conv_out is round(Q . W_c): ONE rounding, of the fp32 product.

DEFECTS.  Mode(defect=...) plants one deliberate mistake (tests/test_vae_reference_model.py measures that the gate of
tests/test_gpu_vae_conformance.py sees each of them):

  s2a_other_side  Downsample padded (1, 0, 1, 0) instead of (0, 1, 0, 1)      s2a_symmetric  Downsample as stride 2, pad 1
  attn_scale      softmax scale off by sqrt 2                                    attn_kv0       K / V of image 0 used for every image
  fold_bias       Q . b_c missing from the folded conv_out bias                   nin_skip       nin_shortcut output not added
  up_shift        Upsample reads its source one pixel down / right               p_tail         the last 32 columns of P not normalised
  gn_eps          GroupNorm eps 1e-5 instead of 1e-6 (below every gate: listed as undetectable, never dropped silently)
"""
from __future__ import annotations

import dataclasses
from typing import Optional

import torch
import torch.nn.functional as F

TINY = dict(double_z=True, z_channels=4, resolution=64, in_channels=3, out_ch=3, ch=32, ch_mult=(1, 2, 4, 4), num_res_blocks=1,
            attn_resolutions=[], dropout=0.0)
SD_WIDTHS = dict(ch=128, ch_mult=(1, 2, 4, 4), z_channels=4)          # the shipped first stage: 128 / 256 / 512 / 512 channels
DEFECTS = ("s2a_other_side", "s2a_symmetric", "attn_scale", "attn_kv0", "fold_bias", "nin_skip", "up_shift", "p_tail")
UNDETECTABLE = ("gn_eps",)


@dataclasses.dataclass(frozen=True)
class Mode:
    round: bool = False                      # False: the exact evaluation
    dtype: torch.dtype = torch.bfloat16      # what `round` rounds to: the engine dtype
    defect: Optional[str] = None


EXACT = Mode()


def S(m: Mode, x):
    """A tensor the engine stores in its dtype."""
    return x.to(m.dtype).to(x.dtype) if m.round else x


def gn(sd, p, x, m: Mode = EXACT, swish=True):
    eps = 1e-5 if m.defect == "gn_eps" else 1e-6
    y = F.group_norm(x, 32, sd[p + ".weight"], sd[p + ".bias"], eps)
    return S(m, y * torch.sigmoid(y) if swish else y)


def conv3(sd, p, x, m: Mode = EXACT, **kw):
    """The 3x3 product before its epilogue's residual / store: packed (rounded) weight, fp32 bias."""
    return F.conv2d(x, S(m, sd[p + ".weight"]), sd[p + ".bias"], **kw)


def conv1(sd, p, x, m: Mode = EXACT):
    W = sd[p + ".weight"]
    return F.conv2d(x, S(m, W.reshape(W.shape[0], W.shape[1], 1, 1)), sd[p + ".bias"])


def resblock(sd, p, x, m: Mode = EXACT):
    h = gn(sd, p + ".norm1", x, m)
    h = S(m, conv3(sd, p + ".conv1", h, m, padding=1))
    h = gn(sd, p + ".norm2", h, m)
    if p + ".nin_shortcut.weight" in sd:
        sk = S(m, conv1(sd, p + ".nin_shortcut", x, m))
        if m.defect == "nin_skip":
            sk = torch.zeros_like(sk)
        return S(m, conv3(sd, p + ".conv2", h, m, padding=1) + sk)
    return S(m, conv3(sd, p + ".conv2", h, m, padding=1) + x)


def attn(sd, p, x, m: Mode = EXACT):
    """Single head over all C channels, one image at a time: softmax(q k^T C^-0.5) v, proj_out, residual."""
    B, C, H, W = x.shape
    N = H * W
    hn = gn(sd, p + ".norm", x, m, swish=False)
    q, k, v = (S(m, conv1(sd, f"{p}.{n}", hn, m)).reshape(B, C, N).transpose(1, 2) for n in ("q", "k", "v"))     # [B, N, C]
    scale = float(C) ** -0.5 * (2.0 ** 0.5 if m.defect == "attn_scale" else 1.0)
    out = []
    for b in range(B):
        kv = 0 if m.defect == "attn_kv0" else b
        s = (q[b] @ k[kv].t()) * scale
        e = torch.exp(s - s.amax(1, keepdim=True))
        P = e / e.sum(1, keepdim=True)
        if m.defect == "p_tail":
            P = torch.cat([P[:, :N - 32], e[:, N - 32:]], 1)
        out.append(S(m, S(m, P) @ v[kv]))
    a = torch.stack(out).transpose(1, 2).reshape(B, C, H, W)
    return S(m, conv1(sd, p + ".proj_out", a, m) + x)


def downsample(sd, p, x, m: Mode = EXACT):
    """Downsample: one zero column on the right and one zero row at the bottom, then 3x3 stride 2 without padding."""
    if m.defect == "s2a_other_side":
        return S(m, conv3(sd, p + ".conv", F.pad(x, (1, 0, 1, 0)), m, stride=2))
    if m.defect == "s2a_symmetric":
        return S(m, conv3(sd, p + ".conv", x, m, stride=2, padding=1))
    return S(m, conv3(sd, p + ".conv", F.pad(x, (0, 1, 0, 1)), m, stride=2))


def upsample(sd, p, x, m: Mode = EXACT):
    """Upsample: nearest x2 (output pixel (y, x) reads source (y // 2, x // 2)), then 3x3 stride 1 pad 1."""
    up = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    if m.defect == "up_shift":
        up = torch.cat([up[:, :, 1:], up[:, :, -1:]], 2)
        up = torch.cat([up[:, :, :, 1:], up[:, :, :, -1:]], 3)
    return S(m, conv3(sd, p + ".conv", up, m, padding=1))


# ------------------------------------------------------------------------------------------------ the weight transformations

def fold_conv_out(sd, m: Mode = EXACT, prefix=""):
    """Encoder conv_out (3x3) followed by quant_conv (1x1) as ONE 3x3: (weight [2 embed, C, 3, 3], bias [2 embed]).  Exact: the
    1x1 is pointwise, so it composes with every tap (and with the zero padding: Q . 0 = 0, while the bias enters after it)."""
    Wc, bc = sd[prefix + "encoder.conv_out.weight"], sd[prefix + "encoder.conv_out.bias"]
    Q = sd[prefix + "quant_conv.weight"]
    Q = Q.reshape(Q.shape[0], -1)
    Wf = torch.einsum("po,oikl->pikl", Q, Wc)
    bf = sd[prefix + "quant_conv.bias"] + (0 if m.defect == "fold_bias" else Q @ bc)
    return S(m, Wf), bf


def post_quant_padded(sd, m: Mode = EXACT, prefix=""):
    """post_quant_conv (1x1, embed -> z_channels) as the zero-padded 32 x 32 linear the decoder launches: (W [32, 32], b [32])."""
    pw = sd[prefix + "post_quant_conv.weight"]
    zc, emb = pw.shape[0], pw.shape[1]
    Wp = torch.zeros(32, 32, dtype=pw.dtype, device=pw.device)
    Wp[:zc, :emb] = pw.reshape(zc, emb)
    bp = torch.zeros(32, dtype=pw.dtype, device=pw.device)
    bp[:zc] = sd[prefix + "post_quant_conv.bias"]
    return S(m, Wp), bp


def post_quant(sd, z, m: Mode = EXACT, prefix=""):
    """The padded linear on the latent's 32-column token rows (columns past embed are zero): NCHW in, NCHW [B, z_channels] out."""
    B, C, H, W = z.shape
    Wp, bp = post_quant_padded(sd, m, prefix)
    tok = torch.zeros(B * H * W, 32, dtype=z.dtype, device=z.device)
    tok[:, :C] = S(m, z).permute(0, 2, 3, 1).reshape(-1, C)
    zq = S(m, tok @ Wp.t() + bp)
    zc = sd[prefix + "post_quant_conv.weight"].shape[0]
    assert not zq[:, zc:].any(), "the pad columns of the padded linear stay zero"
    return zq[:, :zc].reshape(B, H, W, zc).permute(0, 3, 1, 2)


def enc_conv_out(sd, hn, m: Mode = EXACT, prefix=""):
    """The folded conv_out on the norm_out output: the fp32 moments (not rounded)."""
    Wf, bf = fold_conv_out(sd, m, prefix)
    return F.conv2d(hn, Wf, bf, padding=1)


def enc_conv_out_unfused(sd, hn, prefix=""):
    """What the fold restates: the 3x3 conv_out, then the 1x1 quant_conv."""
    y = F.conv2d(hn, sd[prefix + "encoder.conv_out.weight"], sd[prefix + "encoder.conv_out.bias"], padding=1)
    return F.conv2d(y, sd[prefix + "quant_conv.weight"], sd[prefix + "quant_conv.bias"])


# ------------------------------------------------------------------------------------------------ encoder / decoder

def encoder(sd, cfg, x, m: Mode = EXACT, prefix="", taps=None):
    """AutoencoderKL.encode up to the posterior moments [B, 2 embed, H / 8, W / 8].  taps: a dict that receives every block's
    (input, output) by name."""
    e = prefix + "encoder"
    t = (lambda n, i, o: taps.__setitem__(n, (i, o))) if taps is not None else (lambda n, i, o: None)
    ch_mult, nrb = tuple(cfg["ch_mult"]), cfg["num_res_blocks"]
    h = S(m, conv3(sd, e + ".conv_in", S(m, x), m, padding=1))
    for i in range(len(ch_mult)):
        for j in range(nrb):
            h0, h = h, resblock(sd, f"{e}.down.{i}.block.{j}", h, m)
            t(f"down.{i}.block.{j}", h0, h)
        if i != len(ch_mult) - 1:
            h0, h = h, downsample(sd, f"{e}.down.{i}.downsample", h, m)
            t(f"down.{i}.downsample", h0, h)
    for name, fn in (("mid.block_1", resblock), ("mid.attn_1", attn), ("mid.block_2", resblock)):
        h0, h = h, fn(sd, f"{e}.{name}", h, m)
        t(name, h0, h)
    hn = gn(sd, e + ".norm_out", h, m)
    out = enc_conv_out(sd, hn, m, prefix)
    t("conv_out", hn, out)
    return out


def decoder(sd, cfg, z, m: Mode = EXACT, prefix="", taps=None):
    """AutoencoderKL.decode: z [B, embed, h, w] -> image [B, 3, 8 h, 8 w] (fp32 in the engine: not rounded)."""
    d = prefix + "decoder"
    t = (lambda n, i, o: taps.__setitem__(n, (i, o))) if taps is not None else (lambda n, i, o: None)
    ch_mult, nrb = tuple(cfg["ch_mult"]), cfg["num_res_blocks"]
    h = S(m, conv3(sd, d + ".conv_in", post_quant(sd, z, m, prefix), m, padding=1))
    for name, fn in (("mid.block_1", resblock), ("mid.attn_1", attn), ("mid.block_2", resblock)):
        h0, h = h, fn(sd, f"{d}.{name}", h, m)
        t(name, h0, h)
    for i in reversed(range(len(ch_mult))):
        for j in range(nrb + 1):
            h0, h = h, resblock(sd, f"{d}.up.{i}.block.{j}", h, m)
            t(f"up.{i}.block.{j}", h0, h)
        if i != 0:
            h0, h = h, upsample(sd, f"{d}.up.{i}.upsample", h, m)
            t(f"up.{i}.upsample", h0, h)
    hn = gn(sd, d + ".norm_out", h, m)
    return conv3(sd, d + ".conv_out", hn, m, padding=1)


# ------------------------------------------------------------------------------------------------ weights and inputs

def make_model(cfg=TINY, seed=0, embed_dim=4):
    """The repository's AutoencoderKL with weights at the scale of a trained network instead of torch's defaults: unit-gain convs,
    norm gains around 1, biases of 0.1 -- so that no branch of a block is negligible next to the other (a defect in a branch that
    carries 1 % of the output would pass any relative gate)."""
    from ldm.models.autoencoder import AutoencoderKL
    m = AutoencoderKL(ddconfig=dict(cfg), lossconfig=dict(target="torch.nn.Identity"), embed_dim=embed_dim).eval()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if "norm" in k:
                v.copy_(1.0 + 0.2 * torch.randn(v.shape, generator=g) if k.endswith("weight") else 0.1 * torch.randn(v.shape, generator=g))
            elif k.endswith("bias"):
                v.copy_(0.1 * torch.randn(v.shape, generator=g))
            else:
                fan = v[0].numel()
                v.copy_(torch.randn(v.shape, generator=g) * fan ** -0.5)
    return m


def state64(model, device="cpu"):
    return {k: v.detach().to(device=device, dtype=torch.float64) for k, v in model.state_dict().items()}


def image(B, H, W, seed=0, device="cpu"):
    """B DIFFERENT smooth images in [-1, 1] (fp32 values, as the data loader hands them over): low-frequency waves whose phase and
    direction change with the sample, plus a little noise.  Smooth on purpose: a one-pixel shift of a smooth image is the defect
    an aggregate tolerance is most likely to miss."""
    g = torch.Generator().manual_seed(1000 + seed)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    out = torch.empty(B, 3, H, W)
    for b in range(B):
        for c in range(3):
            f = 0.15 + 0.25 * torch.rand(4, generator=g)
            ph = 6.28 * torch.rand(2, generator=g)
            out[b, c] = 0.45 * torch.sin(f[0] * y + f[1] * x + ph[0]) + 0.45 * torch.cos(f[2] * y - f[3] * x + ph[1])
    out += 0.05 * torch.randn(out.shape, generator=g)
    return out.clamp(-1, 1).to(device)


def latent(B, h, w, seed=0, device="cpu", C=4):
    return torch.randn(B, C, h, w, generator=torch.Generator().manual_seed(2000 + seed)).to(device)


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / (b.norm() + 1e-30))
