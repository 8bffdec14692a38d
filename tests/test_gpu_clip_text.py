"""CLIP text encoder on the GPU (ctrlora_amd/engine/clip_text.py; include/ctrlora_hip.h: cl_clip_text_embed, cl_gather_rows,
cl_attention_causal_fwd).  Comparators: torch for the two layout kernels, the HF CLIPTextModelWithProjection with seeded weights
(tests/test_clip_text_cpu.py: hf_text_model) in fp64 on the CPU for the whole encoder, the same classes with use_engine = False
for the public interface.

  1. token embedding / row gather: exact (fp32) / one rounding (bf16), out-of-range ids clamped, guard rows untouched
  2. whole encoder, tiny (both activations, 77 and 5 tokens) and at ViT-L width
  3. FrozenCLIPEmbedder, CLIPTextEncoder and style_image_tokens with a negative content prompt
  4. hipGraph capture; load_state_dict refreshes the packed weights
"""
import numpy as np
import pytest
import torch

from tests import gemm_ref as G
from tests.test_clip_text_cpu import TINY, hf_text_model, make_ids
from tests.test_gpu_bench_shapes import K_CMP, _need_gpu, _record
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
GATE_F32 = 1e-4            # the project's fp32 whole-model gate (tests/test_gpu_bench_shapes.py, tests/test_gpu_clip_vision.py)
NAMES = ("last_hidden_state", "pooler_output", "text_embeds")


# ------------------------------------------------------------------------------------------------ 1. embedding / gather

@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("B,T,D", [(2, 77, 128), (3, 5, 776), (1, 1, 8)])
def test_token_embedding_and_row_gather(B, T, D, dtype):
    _need_gpu()
    from ctrlora_amd import hip
    g = torch.Generator().manual_seed(B * 100 + T)
    vocab = 301
    tok, pos = torch.randn(vocab, D, generator=g).cuda(), torch.randn(77, D, generator=g).cuda()
    ids = torch.randint(0, vocab, (B, T), generator=g)
    ids[0, 0], ids[-1, -1] = 0, vocab - 1
    want = (tok.double()[ids.cuda()] + pos.double()[:T]).reshape(B * T, D).float().to(dtype)      # fp32 add exact in fp64, ONE rounding
    og = G.Guarded(B * T, D, dtype, "cuda")
    hip.clip_text_embed(ids.cuda(), tok, pos, og.view)
    torch.cuda.synchronize()
    assert torch.equal(og.view, want) and og.check() == dict(guard_rows=0, pad_elems=0, nan_left=0)
    og2 = G.Guarded(B * T, D, dtype, "cuda")
    hip.clip_text_embed(ids, tok, pos, og2.view)                       # ids from the host: checked there, then the same launch
    torch.cuda.synchronize()
    assert torch.equal(og2.view, want)
    # ids outside [0, vocab) on the device are clamped by the kernel (nothing is read out of range); from the host they are refused
    wild = ids.clone()
    wild[0, 0], wild[-1, -1] = -5, vocab + 10 ** 6
    og3 = G.Guarded(B * T, D, dtype, "cuda")
    hip.clip_text_embed(wild.cuda(), tok, pos, og3.view)
    torch.cuda.synchronize()
    assert torch.equal(og3.view, want) and og3.check() == dict(guard_rows=0, pad_elems=0, nan_left=0)
    with pytest.raises(hip.HipError, match="token id"):
        hip.clip_text_embed(wild, tok, pos, og3.view)
    # gather: rows of a padded source into a guarded destination, indices clamped
    src = G.padded(want, 24)
    rows = torch.tensor([B * T - 1, 0, B * T + 7, -3][:max(1, min(4, B + 1))], dtype=torch.long)
    gg = G.Guarded(rows.numel(), D, dtype, "cuda")
    hip.gather_rows(src, rows.cuda(), gg.view)
    torch.cuda.synchronize()
    assert torch.equal(gg.view, want[rows.clamp(0, B * T - 1).cuda()]) and gg.check() == dict(guard_rows=0, pad_elems=0, nan_left=0)
    with pytest.raises(hip.HipError, match="code 1"):                  # D % 8
        hip.gather_rows(src[:, :D - 4], rows.cuda(), gg.view[:, :D - 4])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. whole encoder

_REF = {}


def _reference(cfg, B, N, seed=0):
    """(HF module fp32 on the CPU, ids, fp64 outputs by name): computed once per (config, B, N)."""
    key = (tuple(sorted(cfg.items())), B, N, seed)
    if key not in _REF:
        m = hf_text_model(cfg, seed)
        ids = make_ids(cfg, B, N)
        m.double()
        try:
            with torch.no_grad():
                o = m(input_ids=ids, output_hidden_states=True)
                pooled = m.text_model(input_ids=ids).pooler_output
        finally:
            m.float()
        _REF[key] = (m, ids, dict(last_hidden_state=o.last_hidden_state.clone(), pooler_output=pooled.clone(),
                                  text_embeds=o.text_embeds.clone(), hidden_1=o.hidden_states[1].clone()))
    return _REF[key]


def _whole_encoder(cfg, B, N, tag):
    from ctrlora_amd.engine.clip_text import ClipTextE
    m, ids, ref = _reference(cfg, B, N)
    idg = ids.cuda()
    res = {}
    for dtype in (F32, BF):
        ex = ClipTextE(m.state_dict(), cfg, dtype, "cuda")
        out = ex.forward(idg, want=NAMES)
        torch.cuda.synchronize()
        assert all(out[n].dtype == F32 for n in NAMES) and ex.forwards == 1        # (the residual stream is fp32 in both dtypes)
        for n in NAMES:
            assert tuple(out[n].shape) == tuple(ref[n].shape), n
        res[dtype] = {n: rel_l2(out[n], ref[n]) for n in NAMES}
        alloc = torch.cuda.memory_allocated()
        ex.forward(idg, want=NAMES)                                     # buffers are reused: no allocation after the first call
        assert torch.cuda.memory_allocated() == alloc
        h1 = ex.forward(ids, want=("hidden_state",), hidden_idx=1)["hidden_state"]     # ids from the host; one layer runs
        torch.cuda.synchronize()
        res[dtype]["hidden_1"] = rel_l2(h1, ref["hidden_1"])
        del ex
    # the same-precision comparator: the HF module under bf16 autocast on the same GPU, against the same fp64 reference
    mg = m.cuda()
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=BF):
            oc = mg(input_ids=idg)
            pc = mg.text_model(input_ids=idg).pooler_output
    finally:
        m.cpu()
    cmp_ = dict(last_hidden_state=rel_l2(oc.last_hidden_state, ref["last_hidden_state"]), pooler_output=rel_l2(pc, ref["pooler_output"]),
                text_embeds=rel_l2(oc.text_embeds, ref["text_embeds"]))
    print(f"clip text {tag}: fp32 {res[F32]}, bf16 {res[BF]}, HF bf16 autocast {cmp_}")
    _record("clip_text_whole", tag=tag, B=B, N=N, f32=res[F32], bf16=res[BF], cmp=cmp_)
    for n in NAMES + ("hidden_1",):
        assert res[F32][n] < GATE_F32, (n, res[F32])
    for n in NAMES:
        assert res[BF][n] < K_CMP * cmp_[n], (n, res[BF], cmp_)


@pytest.mark.parametrize("N", [77, 5])
@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
def test_tiny_encoder_vs_hf_fp64(act, N):
    """D 128 (2 heads of 64), MLP 256, 2 layers, projection 64, B = 2.  fp32: rel-L2 < 1e-4 (the fp32 whole-model gate); bf16:
    K_CMP x the HF module under bf16 autocast measured here against the same fp64 reference."""
    _need_gpu()
    _whole_encoder(dict(TINY, hidden_act=act), 2, N, f"tiny-{act}-{N}")


def test_vit_l_width_encoder_vs_hf_fp64():
    """D 768, 12 heads, MLP 3072, 2 layers, 77 tokens, B = 2, the legacy eos_token_id = 2 pooling: the prompt encoder's width."""
    _need_gpu()
    cfg = dict(TINY, hidden_size=768, num_attention_heads=12, intermediate_size=3072, projection_dim=768, eos_token_id=2)
    _whole_encoder(cfg, 2, 77, "vit-l-width-2-layers")


# ------------------------------------------------------------------------------------------------ 3. through the classes

_FROZEN = []


def _frozen():
    """One FrozenCLIPEmbedder on the GPU (ViT-L/14 text from its config), random weights loaded through load_state_dict."""
    if not _FROZEN:
        import warnings
        from ldm.modules.encoders.modules import FrozenCLIPEmbedder
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            enc = FrozenCLIPEmbedder(version="no-such-local-model", device="cuda").cuda()
        g = torch.Generator().manual_seed(11)
        sd = {}
        for k, v in enc.state_dict().items():
            if k.endswith("norm.weight") or k.endswith("norm1.weight") or k.endswith("norm2.weight"):
                sd[k] = 1.0 + 0.2 * torch.randn(v.shape, generator=g)
            elif k.endswith(".bias"):
                sd[k] = 0.1 * torch.randn(v.shape, generator=g)
            else:
                sd[k] = v.cpu()
        enc.load_state_dict(sd, strict=True)
        _FROZEN.append(enc)
    return _FROZEN[0]


@pytest.mark.parametrize("layer,idx", [("last", None), ("pooled", None), ("hidden", -2)])
def test_frozen_clip_embedder_runs_on_the_engine(layer, idx, monkeypatch):
    _need_gpu()
    monkeypatch.setenv("CTRLORA_SYNTHETIC_TOKENIZER", "1")
    enc = _frozen()
    enc.layer, enc.layer_idx = layer, idx
    text = ["a photo of a cat sitting on a red sofa", "two dogs"]
    try:
        before = enc.__dict__["_txt"].forwards if "_txt" in enc.__dict__ else 0
        enc.use_engine = False
        want = enc(text)
        assert (enc.__dict__["_txt"].forwards if "_txt" in enc.__dict__ else 0) == before          # the HF path ran
        enc.use_engine = True
        got = enc(text)
        again = enc.encode(text)
    finally:
        enc.use_engine, enc.layer, enc.layer_idx = True, "last", None
    ex = enc.__dict__["_txt"]
    assert ex.forwards == before + 2 and ex.dtype == F32, "the GPU call must have run on the engine, in fp32 by default"
    assert got.dtype == want.dtype == F32 and tuple(got.shape) == tuple(want.shape) == ((2, 1, 768) if layer == "pooled" else (2, 77, 768))
    assert got.data_ptr() != again.data_ptr() and torch.equal(got, again)          # fresh tensors, not the executor's buffers
    e = rel_l2(got, want)
    _record("clip_text_frozen_embedder", layer=layer, rel=e)
    assert e < GATE_F32, e


def test_clip_text_encoder_and_negative_content_tokens_through_the_tiny_style_model():
    _need_gpu()
    from transformers import CLIPImageProcessor
    from cldm.style_helpers import CLIPTextEncoder, CLIPVisionEncoder, ImageProjModel, style_image_tokens
    from ctrlora_amd.engine import CtrLoRAEngine, NetCfg
    from oracle import arch
    from tests.test_clip_vision_cpu import TINY as VTINY, hf_model
    from tests.test_gpu_style_ip import _tiny_ip_state
    ucfg = arch.TINY
    assert TINY["projection_dim"] == VTINY["projection_dim"]
    mt = hf_text_model(TINY)
    ids = make_ids(TINY, 1, 9)                                          # the app's tokenizer call does not pad: 9 tokens
    txt = CLIPTextEncoder(TINY).cuda()
    txt.load_state_dict(mt.state_dict(), strict=True)
    txt.set_engine_dtype(F32)
    with torch.no_grad():
        txt.use_engine = False
        want_t = txt(ids.cuda())
        txt.use_engine = True
        got_t = txt(ids.cuda(), attention_mask=torch.ones_like(ids).cuda())
        assert txt.__dict__["_txt"].forwards == 1
        masked = txt(ids.cuda(), attention_mask=torch.tensor([[1] * 8 + [0]]).cuda())      # a padding mask: the HF path
        assert txt.__dict__["_txt"].forwards == 1 and masked.text_embeds.shape == got_t.text_embeds.shape
    e_t = (rel_l2(got_t.text_embeds, want_t.text_embeds), rel_l2(got_t.last_hidden_state, want_t.last_hidden_state))
    assert got_t.text_embeds.dtype == F32 and tuple(got_t.text_embeds.shape) == (1, 64) and max(e_t) < GATE_F32, e_t
    # style image -> embeds - scale * text_embeds -> tokens, against the plain HF modules on the CPU
    proc = CLIPImageProcessor(size={"shortest_edge": 70}, crop_size={"height": 70, "width": 70})
    torch.manual_seed(6)
    proj = ImageProjModel(cross_attention_dim=ucfg.context_dim, clip_embeddings_dim=VTINY["projection_dim"])
    img = np.random.default_rng(8).integers(0, 256, size=(300, 200, 3), dtype=np.uint8)
    mv = hf_model(VTINY)
    plain = CLIPVisionEncoder(VTINY)
    plain.load_state_dict(mv.state_dict(), strict=True)
    with torch.no_grad():
        neg_cpu = mt(input_ids=ids).text_embeds
    want, want_u = style_image_tokens(plain, proj, img, processor=proc, neg_content_embeds=neg_cpu, neg_content_scale=0.5)
    base, _ = style_image_tokens(plain, proj, img, processor=proc)
    enc = CLIPVisionEncoder(VTINY).cuda()
    enc.load_state_dict(mv.state_dict(), strict=True)
    enc.set_engine_dtype(F32)
    proj_g = ImageProjModel(cross_attention_dim=ucfg.context_dim, clip_embeddings_dim=VTINY["projection_dim"]).cuda()
    proj_g.load_state_dict(proj.state_dict())
    tokens, uncond = style_image_tokens(enc, proj_g, img, processor=proc, neg_content_embeds=got_t.text_embeds, neg_content_scale=0.5)
    e = (rel_l2(tokens, want), rel_l2(uncond, want_u))
    _record("clip_text_style_tokens", text_embeds=e_t[0], tokens=e[0], uncond=e[1])
    assert tokens.is_cuda and tuple(tokens.shape) == (1, 4, ucfg.context_dim) and max(e) < GATE_F32, e
    assert rel_l2(want, base) > 1e-2                                    # the negative prompt moved the tokens
    # ... as c_ip through one forward of the tiny style model
    ncfg = NetCfg(ucfg.in_channels, ucfg.out_channels, ucfg.model_channels, ucfg.channel_mult, ucfg.num_res_blocks,
                  ucfg.attention_resolutions, ucfg.num_heads, ucfg.context_dim)
    g = torch.Generator().manual_seed(5)
    B, Hh = 1, 16
    z, hint = torch.randn(B, 4, Hh, Hh, generator=g).cuda(), torch.randn(B, 4, Hh, Hh, generator=g).cuda()
    ctx = torch.randn(B, 77, ucfg.context_dim, generator=g).cuda()
    t = torch.randint(0, 1000, (B,), generator=g).cuda()
    sd_un, _ = _tiny_ip_state(ucfg, 3, [1.0, 0.0, 0.6])
    eng = CtrLoRAEngine(sd_un, [arch.make_state(arch.controlnet_shapes(ucfg), 3)], ncfg, dtype=F32, device="cuda:0", need_bwd=False)
    e_none = eng.forward(z, t, ctx, [hint]).clone()
    e_ip = eng.forward(z, t, ctx, [hint], context_ip=tokens.contiguous())
    torch.cuda.synchronize()
    assert torch.isfinite(e_ip).all() and rel_l2(e_ip, e_none) > 1e-3


# ------------------------------------------------------------------------------------------------ 4. capture and reload

@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_forward_is_capturable_and_load_state_dict_refreshes(dtype):
    _need_gpu()
    from cldm.style_helpers import CLIPTextEncoder
    from ctrlora_amd.engine.clip_text import ClipTextE
    m, ids, ref = _reference(dict(TINY), 2, 77)
    idg = ids.cuda()
    ex = ClipTextE(m.state_dict(), TINY, dtype, "cuda")
    first = ex.forward(idg, want=NAMES)
    eager = {n: first[n].clone() for n in NAMES}
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ex.forward(idg, want=NAMES)
    for _ in range(3):
        for n in NAMES:
            out[n].fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(out[n], eager[n]) for n in NAMES)
    # other weights, refreshed in place: the captured launch sequence reads them
    m2 = hf_text_model(TINY, seed=5)
    ex.load(m2.state_dict())
    graph.replay()
    torch.cuda.synchronize()
    m2.double()
    try:
        with torch.no_grad():
            want2 = m2(input_ids=ids).text_embeds.clone()
    finally:
        m2.float()
    gate = GATE_F32 if dtype == F32 else 3e-2      # (bf16: the whole-model tolerance of smoke(); the point here is "the new weights")
    assert rel_l2(out["text_embeds"], want2) < gate and rel_l2(out["text_embeds"], eager["text_embeds"]) > 0.1
    del graph
    # the nn.Module: load_state_dict after the first forward changes the next one
    enc = CLIPTextEncoder(TINY).cuda()
    enc.set_engine_dtype(dtype)
    enc.load_state_dict(m.state_dict(), strict=True)
    with torch.no_grad():
        a = enc(idg).text_embeds
        assert torch.equal(a, eager["text_embeds"])
        enc.load_state_dict(m2.state_dict(), strict=True)
        b = enc(idg).text_embeds
    assert enc.__dict__["_txt"].forwards == 2
    assert rel_l2(b, want2) < gate and rel_l2(b, a) > 0.1
