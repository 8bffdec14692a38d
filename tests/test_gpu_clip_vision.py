"""CLIP vision encoder of the style path on the GPU (ctrlora_amd/engine/vit.py; include/ctrlora_hip.h: cl_gemm act 4,
cl_vit_patch_rows, cl_vit_tokens).  Comparators: the fp64 contract of tests/gemm_ref.py for the product, fp64 torch for the
layout kernels and the attention, the HF CLIPVisionModelWithProjection with seeded weights (tests/test_clip_vision_cpu.py:
hf_model) in fp64 on the CPU for the whole encoder.

  1. exact-GELU epilogue: by rule and under every forced configuration, element-wise, inside canary buffers
  2. patch rows / token assembly: exact (fp32) / one rounding (bf16), pad columns zero, guard rows untouched
  3. attention at query counts that are no multiple of 64 (d_head 80; the UNet levels all have N % 64 == 0)
  4. / 5. whole encoder, tiny and at ViT-H width          6. style image -> c_ip -> the tiny style model
  7. hipGraph capture; load_state_dict refreshes the packed weights
"""
import math

import numpy as np
import pytest
import torch

from tests import gemm_ref as G
from tests.test_clip_vision_cpu import TINY, hf_model
from tests.test_gpu_bench_shapes import K_CMP, _need_gpu, _record
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
ACT_GELU = 4
# max |gelu'(x)| = gelu'(sqrt 2) = Phi(sqrt 2) + sqrt 2 phi(sqrt 2) = 0.9214 + 0.2076 = 1.1290
LIP_GELU_EXACT = 1.13
# fp32 whole-model gate of tests/test_gpu_bench_shapes.py (eps of the fp32 engine against the reference: 1e-4)
GATE_F32 = 1e-4
LOG2E = 1.4426950408889634


# ------------------------------------------------------------------------------------------------ 1. GELU epilogue

GELU_SHAPES = [(52, 640, 160, 0), (514, 5120, 1280, 0), (257, 640, 160, 32)]


def _gelu_cases(M, N, K1, K2, dtype):
    """[(name, case with act = 4, fp64 reference, bound)] -- references computed once, shared by every launch of the case.
    bound = u_out |ref| + kappa (1.13 |alpha| mag_pre + |beta| |residual|), kappa = 2 K 2^-24: the suite's pre-activation bound
    2 K 2^-24 mag (tests/gemm_ref.py, check 2) times max |gelu'| < 1.13, plus one output rounding.  K counts the accumulated
    terms like gemm_ref.k_total: K1 + K2, one per epilogue operand / factor, three for the activation (erf, sum, product);
    erff is used (csrc/common.h: gelu_f), not gelu_as, so no approximation term is added."""
    from tests.test_gpu_gemm_conformance import _rand
    r = _rand(M + N + K1 + K2 + (7 if dtype == F32 else 0))
    o = dict(a1=r(M, K1, dtype=dtype), w1=r(N, K1, sc=K1 ** -0.5, dtype=dtype))
    if K2:
        o.update(a2=r(M, K2, dtype=dtype), w2=r(N, K2, sc=K2 ** -0.5, dtype=dtype))
    bias, res = r(N, sc=0.5), r(M, N, dtype=dtype)
    out = []
    for name, kw in (("bias", dict(bias=bias)), ("nobias", dict()),
                     ("bias+residual+alpha", dict(bias=bias, residual=res, alpha=0.7, beta=-0.5))):
        pre = G.make_case(**o, bias=kw.get("bias"))                      # the sum the activation sees
        s = G.gemm_ref64(pre)
        mag = G.gemm_ref64(pre, absolute=True)
        al, be = kw.get("alpha", 1.0), kw.get("beta", 0.0)
        ref = 0.5 * s * (1.0 + torch.erf(s * 0.5 ** 0.5)) * al
        mag = LIP_GELU_EXACT * abs(al) * mag
        if "residual" in kw:
            ref = ref + be * res.double()
            mag = mag + abs(be) * res.double().abs()
        kt = K1 + K2 + sum(1 for k in ("bias", "residual", "alpha", "beta") if k in kw) + 3
        u_out = 2.0 ** -8 if dtype == BF else 0.0
        bound = u_out * ref.abs() + 2.0 * kt * 2.0 ** -24 * mag
        out.append((name, G.make_case(**o, act=ACT_GELU, **kw), ref, bound))
    return out


def _check(guard, ref, bound):
    err = (guard.view.double() - ref).abs()
    bad = ~(err <= bound)                                            # a NaN is a violation
    ratio = float((err / bound.clamp_min(1e-300)).nan_to_num(nan=math.inf).max())
    can = guard.check()
    return int(bad.sum()), ratio, can["guard_rows"] + can["pad_elems"] + can["nan_left"]


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("M,N,K1,K2", GELU_SHAPES)
def test_gelu_epilogue_by_rule_and_under_every_forced_configuration(M, N, K1, K2, dtype):
    """A forced configuration either meets the bound or refuses (CL_EINVAL): never an un-activated product.  (A forced id of the
    x-stationary / loader-consumer kernels, which have no GELU epilogue, hands the product to the rules.)"""
    _need_gpu()
    from ctrlora_amd import hip
    from tests.test_gpu_gemm_conformance import CONFIGS, _forced, _launch
    worst, accepted, refused, bad = 0.0, set(), [], []
    for name, c, ref, bound in _gelu_cases(M, N, K1, K2, dtype):
        for cfg in (-1,) + CONFIGS:
            try:
                with _forced(cfg, 0):
                    guard = _launch(c)
            except hip.HipError as e:
                assert "code 1" in str(e), (cfg, str(e))
                assert cfg >= 0, "the rules must take every shape"
                refused.append((name, cfg))
                continue
            torch.cuda.synchronize()
            viol, ratio, canary = _check(guard, ref, bound)
            worst = max(worst, ratio)
            accepted.add((name, cfg))
            if viol or canary:
                bad.append((name, cfg, viol, ratio, canary))
        assert any(n == name and cfg >= 0 for n, cfg in accepted), (name, "no forced configuration accepts the shape")
    print(f"gelu epilogue ({M}, {N}, {K1}+{K2}) {dtype}: launches {len(accepted)}, refused {len(refused)}, worst err/bound {worst:.3f}")
    _record("clip_gelu_epilogue", shape=[M, N, K1, K2], dtype=str(dtype), launches=len(accepted), refused=len(refused),
            err_over_bound=worst, failures=[str(b) for b in bad])
    assert not bad, bad


def test_gelu_bound_separates_the_unactivated_product():
    """The derived bound is tight enough to catch a launch that skipped the activation (what a kernel outside the shared
    epilogue would return), and atomic / LayerNorm-prologue launches with act 4 are refused."""
    _need_gpu()
    from ctrlora_amd import hip
    from tests.test_gpu_gemm_conformance import _launch
    name, c, ref, bound = _gelu_cases(52, 640, 160, 0, BF)[0]
    plain = dict(c, act=G.ACT_NONE)
    guard = _launch(plain)
    torch.cuda.synchronize()
    viol, ratio, _ = _check(guard, ref, bound)
    assert viol > 0.3 * ref.numel() and ratio > 10, (viol, ratio)
    with pytest.raises(hip.HipError, match="code 1"):
        _launch(dict(c, atomic=True, c0=0.0, out_dtype=F32))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. patch rows / tokens

@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("B,S", [(2, 70), (1, 224)])
def test_patch_rows_and_tokens(B, S, dtype):
    _need_gpu()
    from ctrlora_amd import hip
    from ctrlora_amd.engine import vit
    g = torch.Generator().manual_seed(S + B)
    P, C, D = 14, 3, 160
    Kpad = vit.patch_kpad(dict(TINY, image_size=S))
    R = B * (S // P) ** 2
    px = torch.randn(B, C, S, S, generator=g).cuda()
    want = vit.patch_rows_torch(px, P, Kpad)
    guard = G.Guarded(R, Kpad, dtype, "cuda")
    hip.vit_patch_rows(px, guard.view, P)
    torch.cuda.synchronize()
    assert torch.equal(guard.view, want.to(dtype))                   # exact in fp32, ONE rounding in bf16
    assert not guard.view[:, C * P * P:].any()                       # pad columns exactly zero
    assert guard.check() == dict(guard_rows=0, pad_elems=0, nan_left=0)
    # tokens: cls + pos[0] | patch + pos[1 + i], fp32 add, one rounding -- against fp64
    T = R // B + 1
    patch = torch.randn(R, D, generator=g).cuda().to(dtype)
    patch_ld = G.padded(patch, 24)                                   # a leading dimension of its own
    cls, pos = torch.randn(D, generator=g).cuda(), torch.randn(T, D, generator=g).cuda()
    ref = torch.cat([cls.double().expand(B, 1, D), patch.double().reshape(B, T - 1, D)], 1) + pos.double()
    tg = G.Guarded(B * T, D, dtype, "cuda")
    hip.vit_tokens(patch_ld, cls, pos, tg.view, B)
    torch.cuda.synchronize()
    assert torch.equal(tg.view, ref.reshape(B * T, D).float().to(dtype))
    assert tg.check() == dict(guard_rows=0, pad_elems=0, nan_left=0)


def test_vit_entry_points_refuse_bad_arguments():
    _need_gpu()
    from ctrlora_amd import hip
    px = torch.zeros(1, 3, 72, 72, device="cuda")
    with pytest.raises(hip.HipError, match="code 1"):                # S % P != 0
        hip.vit_patch_rows(px, torch.empty(25, 608, device="cuda"), 14)
    with pytest.raises(hip.HipError, match="code 1"):                # Kpad < C P P
        hip.vit_patch_rows(torch.zeros(1, 3, 70, 70, device="cuda"), torch.empty(25, 584, device="cuda"), 14)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. ragged attention

def _attn_ref(q, k, v, B, H, N, dh):
    hd = lambda x: x.double().reshape(B, N, H, dh).permute(0, 2, 1, 3)
    o = torch.softmax(hd(q) @ hd(k).transpose(-1, -2) * dh ** -0.5, -1) @ hd(v)
    return o.permute(0, 2, 1, 3).reshape(B * N, H * dh)


@pytest.mark.parametrize("B,H", [(2, 2), (1, 16)])
@pytest.mark.parametrize("N", [26, 82, 257])
def test_attention_at_ragged_query_counts(N, B, H):
    """d_head 80, N = Nkv not a multiple of 64: bf16 through cl_attention_fwd_v2 with a plain and with a pre-scaled Q, fp32
    through cl_attention_fwd (whose contract has no pre-scaled Q: CL_EINVAL, include/ctrlora_hip.h).  Gates: bf16 the O gate of
    the d_head-80 rows of tests/test_gpu_bench_shapes.py (6e-3); fp32 the 1e-5 of tests/test_gpu_style_ip.py's fp32 attention.
    O is a view into a padded buffer: rows beyond B N and pad columns untouched; two launches bit-identical."""
    _need_gpu()
    from ctrlora_amd import hip
    dh = 80
    inner, scale = H * dh, dh ** -0.5
    g = torch.Generator().manual_seed(N * 31 + H)
    q32, k32, v32 = (torch.randn(B * N, inner, generator=g).cuda() for _ in range(3))
    errs = {}
    # fp32
    want = _attn_ref(q32, k32, v32, B, H, N, dh)
    kpad = (N + 63) // 64 * 64
    vt = torch.empty(B, inner, kpad, device="cuda")
    hip.transpose(v32, vt, B, N, inner, kpad)
    outs = []
    for _ in range(2):
        og = G.Guarded(B * N, inner, F32, "cuda")
        hip.attention_fwd(q32, k32, vt, og.view, None, B, H, N, N, dh, scale)
        torch.cuda.synchronize()
        assert og.check() == dict(guard_rows=0, pad_elems=0, nan_left=0)
        outs.append(og.buf.view(torch.int32).clone())
    assert torch.equal(outs[0], outs[1])
    errs["f32"] = rel_l2(og.view, want)
    assert errs["f32"] <= 1e-5, errs
    # bf16, both Q contracts
    kb, vb = k32.to(BF), v32.to(BF)
    for pre in (False, True):
        qb = (q32 * (scale * LOG2E)).to(BF) if pre else q32.to(BF)
        q_true = qb.double() / (scale * LOG2E) if pre else qb.double()
        want_b = _attn_ref(q_true, kb, vb, B, H, N, dh)
        outs = []
        for _ in range(2):
            og = G.Guarded(B * N, inner, BF, "cuda")
            hip.attention_fwd_v2(qb, kb, vb, og.view, None, B, H, N, N, dh, scale, q_prescaled=pre)
            torch.cuda.synchronize()
            assert og.check() == dict(guard_rows=0, pad_elems=0, nan_left=0)
            outs.append(og.buf.view(torch.int16).clone())
        assert torch.equal(outs[0], outs[1])
        errs["bf16_prescaled" if pre else "bf16"] = rel_l2(og.view, want_b)
    _record("clip_attention_ragged", shape=[dh, N, B, H], **errs)
    assert max(errs["bf16"], errs["bf16_prescaled"]) < 6e-3, errs


# ------------------------------------------------------------------------------------------------ 4. / 5. whole encoder

_REF = {}


def _reference(cfg, B, seed=0):
    """(HF module fp32 on the CPU, pixel_values, fp64 image_embeds, fp64 penultimate hidden state): computed once per config."""
    key = (tuple(sorted(cfg.items())), B, seed)
    if key not in _REF:
        m = hf_model(cfg, seed)
        S = cfg["image_size"]
        x = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(seed + 17))
        with torch.no_grad():
            o = m.double()(pixel_values=x.double(), output_hidden_states=True)
        m.float()
        _REF[key] = (m, x, o.image_embeds.clone(), o.hidden_states[-2].clone())
    return _REF[key]


def _whole_encoder(cfg, B, tag):
    from ctrlora_amd.engine.vit import ClipVisionE
    m, x, emb64, pen64 = _reference(cfg, B)
    xg = x.cuda()
    res = {}
    for dtype in (F32, BF):
        ex = ClipVisionE(m.state_dict(), cfg, dtype, "cuda")
        emb, pen = ex.forward(xg, output_hidden_states=True)
        torch.cuda.synchronize()
        assert emb.dtype == F32 and tuple(emb.shape) == tuple(emb64.shape) and tuple(pen.shape) == tuple(pen64.shape)
        res[dtype] = (rel_l2(emb, emb64), rel_l2(pen, pen64))
        alloc = torch.cuda.memory_allocated()
        ex.forward(xg)                                               # buffers are reused: no allocation after the first call
        assert torch.cuda.memory_allocated() == alloc
        del ex
    # the same-precision comparator: the HF module under bf16 autocast on the same GPU, against the same fp64 reference
    mg = m.cuda()
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):
        oc = mg(pixel_values=xg, output_hidden_states=True)
    cmp_ = (rel_l2(oc.image_embeds, emb64), rel_l2(oc.hidden_states[-2], pen64))
    m.cpu()
    print(f"clip vision {tag}: fp32 {res[F32]}, bf16 {res[BF]}, HF bf16 autocast {cmp_}")
    _record("clip_vision_whole", tag=tag, B=B, embeds_f32=res[F32][0], hidden_f32=res[F32][1], embeds_bf16=res[BF][0],
            hidden_bf16=res[BF][1], cmp_embeds=cmp_[0], cmp_hidden=cmp_[1])
    assert res[F32][0] < GATE_F32 and res[F32][1] < GATE_F32, res
    assert res[BF][0] < K_CMP * cmp_[0] and res[BF][1] < K_CMP * cmp_[1], (res[BF], cmp_)


@pytest.mark.parametrize("S", [70, 126])
def test_tiny_encoder_vs_hf_fp64(S):
    """D 160 (2 heads of 80), MLP 640, 2 layers, projection 64; 26 and 82 tokens, B = 2.  fp32: rel-L2 < 1e-4 (the fp32
    whole-model gate); bf16: K_CMP x the HF module under bf16 autocast measured here against the same fp64 reference."""
    _need_gpu()
    _whole_encoder(dict(TINY, image_size=S), 2, f"tiny-{S}")


def test_vit_h_width_encoder_vs_hf_fp64():
    """D 1280, 16 heads, MLP 5120, 2 layers, S = 224 (257 tokens), B = 2: the production width of every product."""
    _need_gpu()
    cfg = dict(TINY, hidden_size=1280, num_attention_heads=16, intermediate_size=5120, image_size=224, projection_dim=1024)
    _whole_encoder(cfg, 2, "vit-h-width-2-layers")


# ------------------------------------------------------------------------------------------------ 6. pipeline

def test_style_image_to_c_ip_through_the_tiny_style_model():
    _need_gpu()
    from transformers import CLIPImageProcessor
    from cldm.style_helpers import CLIPVisionEncoder, ImageProjModel, style_image_tokens
    from ctrlora_amd.engine import CtrLoRAEngine, NetCfg
    from oracle import arch
    from tests.test_gpu_style_ip import _tiny_ip_state
    ucfg = arch.TINY
    m = hf_model(TINY)
    proc = CLIPImageProcessor(size={"shortest_edge": 70}, crop_size={"height": 70, "width": 70})
    torch.manual_seed(6)
    proj = ImageProjModel(cross_attention_dim=ucfg.context_dim, clip_embeddings_dim=TINY["projection_dim"])
    img = np.random.default_rng(8).integers(0, 256, size=(300, 200, 3), dtype=np.uint8)
    plain = CLIPVisionEncoder(TINY)
    plain.load_state_dict(m.state_dict(), strict=True)
    want, want_u = style_image_tokens(plain, proj, img, processor=proc)            # the plain HF module, fp32, CPU
    enc = CLIPVisionEncoder(TINY).cuda()
    enc.load_state_dict(m.state_dict(), strict=True)
    enc.set_engine_dtype(F32)
    proj_g = ImageProjModel(cross_attention_dim=ucfg.context_dim, clip_embeddings_dim=TINY["projection_dim"]).cuda()
    proj_g.load_state_dict(proj.state_dict())
    tokens, uncond = style_image_tokens(enc, proj_g, img, processor=proc)
    assert "_vit" in enc.__dict__, "the GPU call must have run on the engine"
    e = rel_l2(tokens, want)
    _record("clip_style_tokens", tokens=e, uncond=rel_l2(uncond, want_u))
    assert tokens.is_cuda and tuple(tokens.shape) == (1, 4, ucfg.context_dim) and e < GATE_F32 and rel_l2(uncond, want_u) < GATE_F32
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
    e_none = eng.forward(z, t, ctx, [hint])
    e_ip = eng.forward(z, t, ctx, [hint], context_ip=tokens.contiguous())
    torch.cuda.synchronize()
    assert torch.isfinite(e_ip).all() and rel_l2(e_ip, e_none) > 1e-3


# ------------------------------------------------------------------------------------------------ 7. capture

@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_forward_is_capturable_and_load_state_dict_refreshes(dtype):
    _need_gpu()
    from cldm.style_helpers import CLIPVisionEncoder
    from ctrlora_amd.engine.vit import ClipVisionE
    m, x, emb64, _ = _reference(dict(TINY), 2)
    xg = x.cuda()
    ex = ClipVisionE(m.state_dict(), TINY, dtype, "cuda")
    eager = ex.forward(xg).clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ex.forward(xg)
    replays = []
    for _ in range(3):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        replays.append(out.clone())
    assert all(torch.equal(r, eager) for r in replays)
    # other weights, refreshed in place: the captured launch sequence reads them
    m2 = hf_model(TINY, seed=5)
    ex.load(m2.state_dict())
    graph.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        want2 = m2.double()(pixel_values=x.double()).image_embeds
    gate = GATE_F32 if dtype == F32 else 3e-2      # (bf16: the whole-model tolerance of smoke(); the point here is "the new weights")
    assert rel_l2(out, want2) < gate and rel_l2(out, eager) > 0.1
    del graph
    # the nn.Module: load_state_dict after the first forward changes the next one
    enc = CLIPVisionEncoder(TINY).cuda()
    enc.set_engine_dtype(dtype)
    enc.load_state_dict(m.state_dict(), strict=True)
    with torch.no_grad():
        a = enc(xg).image_embeds
        assert torch.equal(a, eager)
        enc.load_state_dict(m2.float().state_dict(), strict=True)
        b = enc(xg).image_embeds
    assert rel_l2(b, want2) < gate and rel_l2(b, a) > 0.1
