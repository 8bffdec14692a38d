"""CLIP vision encoder of the style path, host side (no GPU): the packing the executor's products read
(ctrlora_amd/engine/vit.py), the nn.Module mirror and the token helper (cldm/style_helpers.py).  The comparator is always the HF
CLIPVisionModelWithProjection with seeded random weights, built here from a config."""
import json

import numpy as np
import pytest
import torch

from tests.util import rel_l2

TINY = dict(hidden_size=160, intermediate_size=640, num_hidden_layers=2, num_attention_heads=2, num_channels=3, image_size=70,
            patch_size=14, hidden_act="gelu", layer_norm_eps=1e-5, projection_dim=64)


def hf_model(cfg, seed=0):
    """HF module with seeded weights off their init scale: norm gammas / betas and every bias get seeded random factors, so a
    dropped bias or beta shows (HF initialises biases to 0 and gammas to 1)."""
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    torch.manual_seed(seed)
    m = CLIPVisionModelWithProjection(CLIPVisionConfig(**cfg)).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("norm.weight") or n.endswith("norm1.weight") or n.endswith("norm2.weight"):
                p.copy_(1.0 + 0.3 * torch.randn(p.shape, generator=g))
            elif n.endswith(".bias"):
                p.copy_(0.2 * torch.randn(p.shape, generator=g))
            elif n.endswith("_proj.weight") or n.endswith("fc1.weight") or n.endswith("fc2.weight") or n == "visual_projection.weight":
                p.copy_(torch.randn(p.shape, generator=g) * p.shape[1] ** -0.5)          # unit-gain products
            elif n.endswith("patch_embedding.weight"):
                p.copy_(torch.randn(p.shape, generator=g) * (p[0].numel() ** -0.5))
            elif n.endswith("position_embedding.weight") or n.endswith("class_embedding"):
                p.copy_(0.5 * torch.randn(p.shape, generator=g))
    return m


def test_patch_rows_times_padded_weight_is_the_patch_convolution():
    """Rows ordered (c, py, px) and zero-padded 588 -> 608, times the flattened zero-padded weight == nn.Conv2d(3, D, 14, 14,
    bias=False) to fp32 rounding (gate: 2 K 2^-24 of the magnitude sum, the suite's fp32 accumulation bound)."""
    from ctrlora_amd.engine import vit
    g = torch.Generator().manual_seed(3)
    D, P = 160, 14
    conv = torch.nn.Conv2d(3, D, P, P, bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g))
    for B, S in ((2, 70), (1, 224)):
        cfg = dict(TINY, image_size=S)
        Kpad = vit.patch_kpad(cfg)
        assert Kpad == 608 and Kpad % vit.K_GRAIN == 0
        x = torch.randn(B, 3, S, S, generator=g)
        rows = vit.patch_rows_torch(x, P, Kpad)
        assert rows.shape == (B * (S // P) ** 2, Kpad) and not rows[:, 588:].any()
        # column (c, py, px) of row (b, gy, gx) is pixel (b, c, gy P + py, gx P + px)
        b, gy, gx, c, py, px = B - 1, 2, 3, 1, 5, 13
        assert rows[(b * (S // P) + gy) * (S // P) + gx, (c * P + py) * P + px] == x[b, c, gy * P + py, gx * P + px]
        pw = torch.nn.functional.pad(conv.weight.detach().reshape(D, -1), (0, Kpad - 588))
        got = rows @ pw.t()
        with torch.no_grad():
            want = conv(x).flatten(2).transpose(1, 2).reshape(-1, D)
        mag = rows.abs() @ pw.abs().t()
        assert bool(((got - want).abs() <= 2 * 588 * 2.0 ** -24 * mag).all()), float((got - want).abs().max())


def test_packing_keys_and_qkv_concatenation():
    from cldm.style_helpers import CLIPVisionEncoder
    from ctrlora_amd.engine import vit
    m = hf_model(TINY)
    sd = m.state_dict()
    assert set(vit.state_keys(TINY)) == set(sd) and len(vit.state_keys(TINY)) == len(sd)
    assert "vision_model.pre_layrnorm.weight" in sd                       # the upstream spelling
    p = vit.pack_clip_vision(sd, TINY)
    D = TINY["hidden_size"]
    assert p["patch_w"].shape == (D, 608) and not p["patch_w"][:, 588:].any()
    assert torch.equal(p["patch_w"][:, :588], sd["vision_model.embeddings.patch_embedding.weight"].reshape(D, 588))
    assert len(p["layers"]) == TINY["num_hidden_layers"]
    for i, lay in enumerate(p["layers"]):
        a = f"vision_model.encoder.layers.{i}.self_attn."
        assert lay["qkv_w"].shape == (3 * D, D) and lay["qkv_b"].shape == (3 * D,)
        for j, n in enumerate("qkv"):
            assert torch.equal(lay["qkv_w"][j * D:(j + 1) * D], sd[a + n + "_proj.weight"])
            assert torch.equal(lay["qkv_b"][j * D:(j + 1) * D], sd[a + n + "_proj.bias"])
        assert torch.equal(lay["fc1_b"], sd[f"vision_model.encoder.layers.{i}.mlp.fc1.bias"])
    # every key of the state dict reaches the packed form (none is silently dropped)
    flat = [t for k, t in p.items() if k != "layers"] + [t for lay in p["layers"] for t in lay.values()]
    assert sum(t.numel() for t in flat) == sum(t.numel() for t in sd.values()) + D * (608 - 588)
    # strict=True both ways
    enc = CLIPVisionEncoder(TINY)
    assert set(enc.state_dict()) == set(sd)
    enc.load_state_dict(sd, strict=True)
    m2 = hf_model(TINY, seed=9)
    m2.load_state_dict(enc.state_dict(), strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in m2.state_dict().items())


def test_packed_weights_restate_the_hf_forward():
    """The executor's step list (ctrlora_amd/engine/vit.py: ClipVisionE.forward) evaluated in fp64 torch on the PACKED tensors
    equals the HF module in fp64: what the packing means, independent of any kernel."""
    from ctrlora_amd.engine import vit
    m = hf_model(TINY).double()
    x = torch.randn(2, 3, 70, 70, generator=torch.Generator().manual_seed(1)).double()
    with torch.no_grad():
        o = m(pixel_values=x, output_hidden_states=True)
    p = vit.pack_clip_vision({k: v.double() for k, v in m.state_dict().items()}, TINY)
    dd = lambda t: t.double()
    F = torch.nn.functional
    D, H, B = 160, 2, 2
    T = 26
    pe = vit.patch_rows_torch(x, 14, 608) @ dd(p["patch_w"]).t()
    h = torch.cat([dd(p["cls"]).expand(B, 1, D), pe.reshape(B, T - 1, D)], 1) + dd(p["pos"])
    h = F.layer_norm(h, (D,), dd(p["pre_g"]), dd(p["pre_b"]), 1e-5)
    hs = [h]
    for lay in p["layers"]:
        xq = F.layer_norm(h, (D,), dd(lay["ln1_g"]), dd(lay["ln1_b"]), 1e-5)
        qkv = xq @ dd(lay["qkv_w"]).t() + dd(lay["qkv_b"])
        q, k, v = (t.reshape(B, T, H, D // H).transpose(1, 2) for t in qkv.split(D, -1))
        a = (torch.softmax(q @ k.transpose(-1, -2) * (D // H) ** -0.5, -1) @ v).transpose(1, 2).reshape(B, T, D)
        h = h + a @ dd(lay["o_w"]).t() + dd(lay["o_b"])
        xm = F.layer_norm(h, (D,), dd(lay["ln2_g"]), dd(lay["ln2_b"]), 1e-5)
        h = h + F.gelu(xm @ dd(lay["fc1_w"]).t() + dd(lay["fc1_b"])) @ dd(lay["fc2_w"]).t() + dd(lay["fc2_b"])
        hs.append(h)
    emb = F.layer_norm(h[:, 0], (D,), dd(p["post_g"]), dd(p["post_b"]), 1e-5) @ dd(p["proj_w"]).t()
    assert rel_l2(emb, o.image_embeds) < 1e-12 and rel_l2(hs[-2], o.hidden_states[-2]) < 1e-12
    assert len(o.hidden_states) == len(hs)


def test_encoder_on_the_cpu_is_the_hf_module_bit_for_bit():
    from cldm.style_helpers import CLIPVisionEncoder
    m = hf_model(TINY)
    enc = CLIPVisionEncoder(TINY)
    enc.load_state_dict(m.state_dict(), strict=True)
    x = torch.randn(2, 3, 70, 70, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        want = m(pixel_values=x, output_hidden_states=True)
        got = enc(x, output_hidden_states=True)
        assert torch.equal(got.image_embeds, want.image_embeds)
        assert len(got.hidden_states) == 3 and all(torch.equal(a, b) for a, b in zip(got.hidden_states, want.hidden_states))
        assert torch.equal(enc(x).image_embeds, want.image_embeds)
    # autograd stays available (the plain module)
    enc(x).image_embeds.sum().backward()
    assert enc.visual_projection.weight.grad is not None


def test_config_forms(tmp_path):
    from transformers import CLIPVisionConfig
    from cldm.style_helpers import VIT_H_14, _vision_config
    c = _vision_config(None)                  # the default: ViT-H/14 as IP-Adapter for SD1.5 ships it (no module is built here)
    assert (c.hidden_size, c.num_attention_heads, c.intermediate_size, c.num_hidden_layers, c.patch_size, c.image_size,
            c.projection_dim, c.hidden_act, c.layer_norm_eps) == (1280, 16, 5120, 32, 14, 224, 1024, "gelu", 1e-5)
    assert VIT_H_14["hidden_size"] // VIT_H_14["num_attention_heads"] == 80
    assert _vision_config(CLIPVisionConfig(**TINY)).hidden_size == 160 and _vision_config(TINY).projection_dim == 64
    (tmp_path / "config.json").write_text(json.dumps(dict(TINY, model_type="clip_vision_model", architectures=["CLIPVisionModelWithProjection"])))
    d = _vision_config(str(tmp_path))
    assert (d.hidden_size, d.image_size, d.projection_dim) == (160, 70, 64)
    with pytest.raises(TypeError):
        _vision_config(3)


@pytest.mark.parametrize("size", [(300, 200), (224, 224)])
def test_style_image_tokens_is_the_apps_sequence(size):
    """processor -> image_embeds -> image_proj(embeds), image_proj(zeros_like(embeds)), written out with HF calls."""
    from transformers import CLIPImageProcessor
    from cldm.style_helpers import CLIPVisionEncoder, ImageProjModel, style_image_tokens
    cfg = dict(TINY, image_size=224)          # CLIPImageProcessor()'s default crop
    m = hf_model(cfg)
    enc = CLIPVisionEncoder(cfg)
    enc.load_state_dict(m.state_dict(), strict=True)
    torch.manual_seed(4)
    proj = ImageProjModel(cross_attention_dim=32, clip_embeddings_dim=64, clip_extra_context_tokens=4)
    img = np.random.default_rng(5).integers(0, 256, size=(size[0], size[1], 3), dtype=np.uint8)
    tokens, uncond = style_image_tokens(enc, proj, img)
    with torch.no_grad():
        px = CLIPImageProcessor()(images=[img], return_tensors="pt").pixel_values
        embeds = m(px).image_embeds
        want, want_u = proj(embeds), proj(torch.zeros_like(embeds))
    assert tokens.shape == (1, 4, 32) and torch.equal(tokens, want) and torch.equal(uncond, want_u)
    from PIL import Image
    t2, u2 = style_image_tokens(enc, proj, Image.fromarray(img), processor=CLIPImageProcessor())
    assert torch.equal(t2, want) and torch.equal(u2, want_u)


def test_executor_refuses_what_it_does_not_cover():
    from ctrlora_amd.engine import vit
    sd = {}
    for field, bad in (("hidden_act", dict(TINY, hidden_act="quick_gelu")),
                       ("image_size", dict(TINY, image_size=72)),
                       ("num_attention_heads", dict(TINY, num_attention_heads=8))):      # d_head 20
        with pytest.raises(ValueError, match=field):
            vit.ClipVisionE(sd, bad, torch.bfloat16)
        assert not vit.supported(bad)
    assert vit.supported(TINY) and vit.check_config(TINY)["hidden_size"] == 160
