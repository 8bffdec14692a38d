"""CLIP text encoder on the CPU: the packing and the torch restatement of the executor's launch sequence
(ctrlora_amd/engine/clip_text.py) against the HF module in fp64; the refusals; the two public classes, which are the plain HF
path on the CPU; the negative-content arithmetic of style_image_tokens.  No kernel is launched here."""
import numpy as np
import pytest
import torch

from ctrlora_amd.engine import clip_text as T

# hidden 128 = 2 heads of 64, MLP 256, 2 layers, vocab 1000, 77 positions
TINY = dict(vocab_size=1000, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
            max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, projection_dim=64, eos_token_id=999,
            bos_token_id=998, pad_token_id=999)
_MODELS = {}


def hf_text_model(cfg, seed=0, projection=True):
    """HF module with seeded weights off their init scale (biases, norm gammas / betas random, unit-gain products), so a dropped
    bias or beta shows.  Cached: callers must not change it."""
    key = (tuple(sorted(cfg.items())), seed, projection)
    if key not in _MODELS:
        from transformers import CLIPTextConfig, CLIPTextModel, CLIPTextModelWithProjection
        torch.manual_seed(seed)
        m = (CLIPTextModelWithProjection if projection else CLIPTextModel)(CLIPTextConfig(**cfg)).eval()
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            for n, p in m.named_parameters():
                if n.endswith("norm.weight") or n.endswith("norm1.weight") or n.endswith("norm2.weight"):
                    p.copy_(1.0 + 0.3 * torch.randn(p.shape, generator=g))
                elif n.endswith(".bias"):
                    p.copy_(0.2 * torch.randn(p.shape, generator=g))
                elif n.endswith("_proj.weight") or n.endswith("fc1.weight") or n.endswith("fc2.weight") or n == "text_projection.weight":
                    p.copy_(torch.randn(p.shape, generator=g) * p.shape[1] ** -0.5)
                elif n.endswith("embedding.weight"):
                    p.copy_(torch.randn(p.shape, generator=g) * 0.7)
        _MODELS[key] = m
    return _MODELS[key]


def make_ids(cfg, B, N, seed=3):
    """[B, N] ids: BOS, words, the end-of-text id at a different place in every sample, then padding with it (as the tokenizer
    pads); for eos_token_id == 2 the end-of-text id is the vocabulary's largest, as in the legacy configs."""
    g = torch.Generator().manual_seed(seed + 10 * N)
    eot = cfg["vocab_size"] - 1 if cfg["eos_token_id"] == 2 else cfg["eos_token_id"]
    ids = torch.randint(3, cfg["vocab_size"] - 2, (B, N), generator=g)
    for b in range(B):
        ids[b, max(1, N - 1 - b * max(1, N // 8)):] = eot
    ids[:, 0] = cfg["vocab_size"] - 2
    if N == 1:
        ids[:, 0] = eot
    return ids


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


@pytest.mark.parametrize("N", [77, 5])
@pytest.mark.parametrize("eos", [999, 2])
@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
def test_torch_restatement_equals_hf_in_fp64(act, eos, N):
    cfg = dict(TINY, hidden_act=act, eos_token_id=eos)
    m = hf_text_model(cfg)
    ids = make_ids(cfg, 3, N)
    m.double()
    try:
        with torch.no_grad():
            want = m(input_ids=ids, output_hidden_states=True)
            pooled = m.text_model(input_ids=ids).pooler_output
        packed = T.pack_clip_text(m.state_dict(), cfg)
    finally:
        m.float()
    assert packed["tok"].dtype == torch.float64
    names = ("last_hidden_state", "pooler_output", "text_embeds")
    got = T.clip_text_forward_torch(packed, ids, cfg, want=names)
    assert _rel(got["last_hidden_state"], want.last_hidden_state) < 1e-10
    assert _rel(got["pooler_output"], pooled) < 1e-10 and _rel(got["text_embeds"], want.text_embeds) < 1e-10
    assert tuple(got["pooler_output"].shape) == (3, 128) and tuple(got["text_embeds"].shape) == (3, 64)
    # the pooled row is where the end-of-text id first stands, a different place in every sample
    idx = T.pooled_index(ids, eos)
    eot = cfg["vocab_size"] - 1 if eos == 2 else eos
    assert bool((ids[torch.arange(3), idx] == eot).all()) and bool((idx > 0).all()) and len(set(idx.tolist())) == 3
    for k in (0, 1, 2, -1, -2):
        h = T.clip_text_forward_torch(packed, ids, cfg, want=("hidden_state",), hidden_idx=k)["hidden_state"]
        assert _rel(h, want.hidden_states[k]) < 1e-10, k
    both = T.clip_text_forward_torch(packed, ids, cfg, want=("hidden_state", "last_hidden_state"), hidden_idx=1)
    assert _rel(both["hidden_state"], want.hidden_states[1]) < 1e-10 and _rel(both["last_hidden_state"], want.last_hidden_state) < 1e-10


def test_quick_gelu_is_packed_into_fc1_in_fp32():
    cfg = dict(TINY)
    sd = hf_text_model(cfg).state_dict()
    p = T.pack_clip_text(sd, cfg)
    assert p["tok"].dtype == torch.float32
    w = sd["text_model.encoder.layers.1.mlp.fc1.weight"]
    assert torch.equal(p["layers"][1]["fc1_w"], w * 1.702) and torch.equal(p["layers"][1]["fc1_b"], sd["text_model.encoder.layers.1.mlp.fc1.bias"] * 1.702)
    g = T.pack_clip_text(hf_text_model(dict(cfg, hidden_act="gelu")).state_dict(), dict(cfg, hidden_act="gelu"))
    assert torch.equal(g["layers"][1]["fc1_w"], hf_text_model(dict(cfg, hidden_act="gelu")).state_dict()["text_model.encoder.layers.1.mlp.fc1.weight"])
    x = torch.linspace(-6, 6, 101, dtype=torch.float64)
    assert float((torch.nn.functional.silu(1.702 * x) / 1.702 - x * torch.sigmoid(1.702 * x)).abs().max()) < 1e-15
    assert tuple(p["layers"][0]["qkv_w"].shape) == (384, 128) and tuple(p["layers"][0]["qkv_b"].shape) == (384,)


def test_state_keys_are_the_hf_modules():
    assert T.state_keys(TINY, projection=True) == list(hf_text_model(TINY).state_dict().keys())
    plain = hf_text_model(TINY, projection=False)
    prefix = "text_model." if any(k.startswith("text_model.") for k in plain.state_dict()) else ""
    assert T.state_keys(TINY, prefix=prefix) == list(plain.state_dict().keys())
    packed = T.pack_clip_text(plain.state_dict(), TINY)                 # either layout packs; no projection here
    assert "proj_w" not in packed and len(packed["layers"]) == 2


@pytest.mark.parametrize("change,word", [
    (dict(num_attention_heads=4), "d_head"), (dict(hidden_size=160, num_attention_heads=2), "d_head"),
    (dict(hidden_act="gelu_new"), "hidden_act"), (dict(max_position_embeddings=129), "max_position_embeddings"),
    (dict(hidden_size=64 * 3 + 0, num_attention_heads=3, intermediate_size=200), "intermediate_size"),
    (dict(projection_dim=60), "projection_dim")])
def test_check_config_refuses(change, word):
    cfg = dict(TINY, **change)
    with pytest.raises(ValueError, match=word):
        T.check_config(cfg)
    assert not T.supported(cfg)


def test_check_config_accepts_and_refuses_a_padding_mask():
    from transformers import CLIPTextConfig
    assert T.supported(TINY) and T.supported(CLIPTextConfig(**TINY)) and T.supported(dict(TINY, max_position_embeddings=128))
    assert T.supported(dict(TINY, hidden_size=768, num_attention_heads=12, intermediate_size=3072))           # ViT-L/14 text
    assert T.supported(dict(TINY, hidden_size=1024, num_attention_heads=16, intermediate_size=4096, hidden_act="gelu"))   # ViT-H/14 text
    ones = torch.ones(2, 7, dtype=torch.long)
    assert T.supported(TINY, ones)
    ones[1, 5:] = 0
    with pytest.raises(ValueError, match="attention_mask"):
        T.check_config(TINY, ones)
    with pytest.raises(ValueError, match="hidden_idx"):
        T.clip_text_forward_torch({}, torch.zeros(1, 3, dtype=torch.long), TINY, want=("hidden_state",), hidden_idx=3)
    with pytest.raises(ValueError, match="want"):
        T.clip_text_forward_torch({}, torch.zeros(1, 3, dtype=torch.long), TINY, want=("logits",))


@pytest.mark.parametrize("layer,idx", [("last", None), ("pooled", None), ("hidden", -2)])
def test_frozen_clip_embedder_on_the_cpu_is_the_hf_path(layer, idx, monkeypatch):
    monkeypatch.setenv("CTRLORA_SYNTHETIC_TOKENIZER", "1")
    import warnings
    from ldm.modules.encoders.modules import FrozenCLIPEmbedder
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        enc = FrozenCLIPEmbedder(version="no-such-local-model", device="cpu", layer=layer, layer_idx=idx)
    assert enc.use_engine and enc.engine_dtype == torch.float32
    text = ["a photo of a cat", "two dogs"]
    got = enc(text)
    ids = enc._tokens(text)
    with torch.no_grad():
        out = enc.transformer(input_ids=ids, output_hidden_states=True)
    want = dict(last=out.last_hidden_state, pooled=out.pooler_output[:, None, :], hidden=out.hidden_states[-2])[layer]
    assert torch.equal(got, want) and got.dtype == torch.float32
    assert "_txt" not in enc.__dict__                                   # no executor was built: forwards == 0


def test_clip_text_encoder_on_the_cpu_is_the_hf_path(tmp_path):
    import json
    from cldm.style_helpers import VIT_H_14_TEXT, CLIPTextEncoder, _text_config
    d = _text_config(None)
    assert (d.hidden_size, d.num_attention_heads, d.num_hidden_layers, d.intermediate_size, d.hidden_act, d.projection_dim, d.vocab_size,
            d.max_position_embeddings) == (1024, 16, 24, 4096, "gelu", 1024, 49408, 77) and T.supported(VIT_H_14_TEXT | dict(eos_token_id=2))
    (tmp_path / "config.json").write_text(json.dumps(dict(text_config=dict(TINY, model_type="clip_text_model"))))
    assert _text_config(str(tmp_path)).hidden_size == 128
    with pytest.raises(TypeError):
        _text_config(3)
    m = hf_text_model(TINY)
    enc = CLIPTextEncoder(TINY)
    assert list(enc.state_dict().keys()) == list(m.state_dict().keys())
    enc.load_state_dict(m.state_dict(), strict=True)
    ids = make_ids(TINY, 2, 9)
    with torch.no_grad():
        got, want = enc(ids), m(input_ids=ids)
    assert torch.equal(got.text_embeds, want.text_embeds) and torch.equal(got.last_hidden_state, want.last_hidden_state)
    assert "_txt" not in enc.__dict__ and enc.use_engine and enc.engine_dtype is None


def test_style_image_tokens_negative_content_is_the_apps_arithmetic():
    from transformers import CLIPImageProcessor
    from cldm.style_helpers import CLIPVisionEncoder, ImageProjModel, style_image_tokens
    from tests.test_clip_vision_cpu import TINY as VTINY, hf_model
    proc = CLIPImageProcessor(size={"shortest_edge": 70}, crop_size={"height": 70, "width": 70})
    torch.manual_seed(6)
    proj = ImageProjModel(cross_attention_dim=32, clip_embeddings_dim=VTINY["projection_dim"])
    enc = CLIPVisionEncoder(VTINY)
    enc.load_state_dict(hf_model(VTINY).state_dict(), strict=True)
    img = np.random.default_rng(8).integers(0, 256, size=(90, 80, 3), dtype=np.uint8)
    base, base_u = style_image_tokens(enc, proj, img, processor=proc)
    none, none_u = style_image_tokens(enc, proj, img, processor=proc, neg_content_embeds=None, neg_content_scale=0.5)
    assert torch.equal(base, none) and torch.equal(base_u, none_u)
    neg = torch.randn(1, VTINY["projection_dim"], generator=torch.Generator().manual_seed(2))
    got, got_u = style_image_tokens(enc, proj, img, processor=proc, neg_content_embeds=neg, neg_content_scale=0.5)
    with torch.no_grad():
        embeds = enc(proc(images=img, return_tensors="pt").pixel_values).image_embeds.clone()
        neg_content_emb = neg.clone()
        neg_content_emb *= 0.5
        embeds -= neg_content_emb                                       # app/gradio_ctrlora_style_transfer.py:401-403
        want = proj(embeds)
    assert torch.equal(got, want) and torch.equal(got_u, base_u) and not torch.equal(got, base)
