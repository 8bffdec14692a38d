"""IP-Adapter spatial + style control on the GPU.

  * cl_attention_fwd_ip (csrc/attention_tr.hip attn_fwd_tr_ip_kernel, csrc/attention_fwd.hip attn_fwd_ip_kernel) against
    fp64 torch of the reference's IPCrossAttention arithmetic (ldm/modules/attention_ip.py:196-289 of the reference: two
    separate softmaxes, out = softmax(s q k^T) v + ip_scale * softmax(s q k_ip^T) v_ip) at every d_head of the forward
    family, the SD1.5 query counts, 77 text keys, Nip in {1, 4, 16, 64}, ip_scale in {0, 0.5, 1}; bf16 gated by the
    error of the plain cl_attention_fwd_v2 at the same shape, measured in the same test (the element-wise conformance suite
    of both kernels -- layouts, canaries, launch forms -- is tests/test_gpu_attention_ip_conformance.py);
  * the engine: with every ip_scale at 0 or without image-prompt tokens, eps is torch.equal to the plain UNet's; with
    them, the image-prompt layers change eps and bf16 follows fp32.
"""
import math

import pytest
import torch

from tests.util import rel_l2

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _ref(q, k, v, kip, vip, B, H, N, Nkv, Nip, dh, scale, alpha):
    """fp64; q [B*N, H*dh] holds the TRUE q (the caller divides a pre-scaled q back)."""
    def heads(x, n):
        return x.double().reshape(B, n, H, dh).permute(0, 2, 1, 3)
    qh = heads(q, N)
    o1 = torch.softmax(qh @ heads(k, Nkv).transpose(-1, -2) * scale, -1) @ heads(v, Nkv)
    o2 = torch.softmax(qh @ heads(kip, Nip).transpose(-1, -2) * scale, -1) @ heads(vip, Nip)
    return (o1 + alpha * o2).permute(0, 2, 1, 3).reshape(B * N, H * dh)


# (d_head, heads, N): SD1.5 levels (320 / 640 / 1280 channels at 8 heads; latent 64 -> N 4096 ... 64, latent 16 / 32 ->
# the smaller levels) and the tiny-width test models' d_heads
# (B * H * ceil(N / 128) >= 512 selects the two-fragment form for d_head <= 80: the B = 32 entries are the CFG batch of
# the benchmark shape and reach it at every d_head)
SHAPES = [(2, 40, 8, 4096), (2, 40, 8, 256), (2, 80, 8, 1024), (32, 80, 8, 1024), (2, 80, 8, 64), (2, 160, 8, 256),
          (2, 160, 8, 64), (2, 160, 8, 16), (2, 8, 4, 256), (32, 8, 4, 512), (2, 16, 4, 64), (32, 16, 4, 512),
          (2, 32, 4, 1024), (32, 32, 4, 512)]


@pytest.mark.parametrize("B,dh,H,N", SHAPES)
def test_attention_fwd_ip_vs_fp64(B, dh, H, N):
    _need_gpu()
    from ctrlora_amd import hip
    g = torch.Generator().manual_seed(dh * 1000 + N + B)
    Nkv, dev = 77, "cuda"
    inner, scale = H * dh, dh ** -0.5
    for Nip in (1, 4, 16, 64):
        q32 = torch.randn(B * N, inner, generator=g)
        k32, v32 = torch.randn(B * Nkv, inner, generator=g), torch.randn(B * Nkv, inner, generator=g)
        kip32, vip32 = torch.randn(B * Nip, inner, generator=g), torch.randn(B * Nip, inner, generator=g)
        for alpha in (0.0, 0.5, 1.0):
            want = _ref(q32, k32, v32, kip32, vip32, B, H, N, Nkv, Nip, dh, scale, alpha)
            # fp32 (parity mode): V / V_ip transposed and zero padded to 64 keys, as cl_attention_fwd
            q, k, kip = q32.to(dev), k32.to(dev), kip32.to(dev)
            vt = torch.zeros(B, inner, 128, device=dev)
            vt[:, :, :Nkv] = v32.to(dev).reshape(B, Nkv, inner).transpose(1, 2)
            vti = torch.zeros(B, inner, 64, device=dev)
            vti[:, :, :Nip] = vip32.to(dev).reshape(B, Nip, inner).transpose(1, 2)
            o = torch.empty(B * N, inner, device=dev)
            hip.attention_fwd_ip(q, k, vt, kip, vti, o, B, H, N, Nkv, Nip, dh, scale, alpha)
            e32 = rel_l2(o.cpu(), want)
            assert e32 <= 1e-5, (dh, N, Nip, alpha, e32)
            # bf16, plain and pre-scaled q
            bq, bk, bv = q32.bfloat16(), k32.bfloat16(), v32.bfloat16()
            bki, bvi = kip32.bfloat16(), vip32.bfloat16()
            want_b = _ref(bq, bk, bv, bki, bvi, B, H, N, Nkv, Nip, dh, scale, alpha)
            plain_ref = _ref(bq, bk, bv, bki, bvi, B, H, N, Nkv, Nip, dh, scale, 0.0)
            ob = torch.empty(B * N, inner, dtype=torch.bfloat16, device=dev)
            hip.attention_fwd_v2(bq.to(dev), bk.to(dev), bv.to(dev), ob, None, B, H, N, Nkv, dh, scale)
            e_plain = rel_l2(ob.cpu(), plain_ref)
            for pre in (False, True):
                qq = (q32 * (scale * LOG2E)).bfloat16() if pre else bq
                wb = want_b if not pre else _ref((qq.double() / (scale * LOG2E)), bk, bv, bki, bvi, B, H, N, Nkv, Nip,
                                                 dh, scale, alpha)
                ob.zero_()
                hip.attention_fwd_ip(qq.to(dev), bk.to(dev), bv.to(dev), bki.to(dev), bvi.to(dev), ob, B, H, N, Nkv,
                                     Nip, dh, scale, alpha, q_prescaled=pre)
                e = rel_l2(ob.cpu(), wb)
                assert math.isfinite(e) and e <= 2.0 * e_plain + 1e-3, (dh, N, Nip, alpha, pre, e, e_plain)
    torch.cuda.synchronize()


def test_attention_fwd_ip_rejects_bad_arguments():
    _need_gpu()
    from ctrlora_amd import hip
    B, H, N, Nkv, dh, dev = 1, 2, 64, 77, 40, "cuda"
    x = lambda r: torch.zeros(r, H * dh, dtype=torch.bfloat16, device=dev)
    o = x(N)
    for Nip in (0, 65):
        with pytest.raises(RuntimeError):
            hip.attention_fwd_ip(x(N), x(Nkv), x(Nkv), x(max(Nip, 1)), x(max(Nip, 1)), o, B, H, N, Nkv, Nip, dh,
                                 dh ** -0.5, 1.0)


def _tiny_ip_state(cfg, seed, scales):
    """Tiny-width UNet state with IP-Adapter weights in every attn2 and ip_scale = scales[i] in module order."""
    from oracle import arch
    sd = arch.make_state(arch.unet_shapes(cfg), seed)
    g = torch.Generator().manual_seed(seed + 1)
    names = sorted({k.rsplit(".", 2)[0] for k in sd if ".attn2.to_k.weight" in k},
                   key=lambda n: [k for k in sd].index(n + ".to_k.weight"))
    for i, n in enumerate(names):
        w = sd[n + ".to_k.weight"]
        sd[n + ".to_k_ip.weight"] = torch.randn(w.shape, generator=g) * float(w.std())
        sd[n + ".to_v_ip.weight"] = torch.randn(w.shape, generator=g) * float(w.std())
        sd[n + ".ip_scale"] = torch.tensor(float(scales[i % len(scales)]))
    return sd, names


def test_engine_ip_scale_zero_and_no_context_are_the_plain_unet():
    _need_gpu()
    from ctrlora_amd.engine import CtrLoRAEngine, NetCfg
    from ldm.models.diffusion.guided_loop import context_kv
    from oracle import arch
    cfg = arch.TINY
    ncfg = NetCfg(cfg.in_channels, cfg.out_channels, cfg.model_channels, cfg.channel_mult, cfg.num_res_blocks,
                  cfg.attention_resolutions, cfg.num_heads, cfg.context_dim)
    g = torch.Generator().manual_seed(5)
    B, Hh = 2, 16
    z, hint = torch.randn(B, 4, Hh, Hh, generator=g).cuda(), torch.randn(B, 4, Hh, Hh, generator=g).cuda()
    ctx = torch.randn(B, 77, cfg.context_dim, generator=g).cuda()
    cip = torch.randn(B, 4, cfg.context_dim, generator=g).cuda()
    t = torch.randint(0, 1000, (B,), generator=g).cuda()
    sd_cn = arch.make_state(arch.controlnet_shapes(cfg), 3)
    sd_plain = arch.make_state(arch.unet_shapes(cfg), 3)
    sd_zero, _ = _tiny_ip_state(cfg, 3, [0.0])
    sd_mixed, names = _tiny_ip_state(cfg, 3, [1.0, 0.0, 0.6])
    for dtype in (torch.float32, torch.bfloat16):
        plain = CtrLoRAEngine(sd_plain, [sd_cn], ncfg, dtype=dtype, device="cuda:0", need_bwd=False)
        e_plain = plain.forward(z, t, ctx, [hint])
        zero = CtrLoRAEngine(sd_zero, [sd_cn], ncfg, dtype=dtype, device="cuda:0", need_bwd=False)
        assert torch.equal(zero.forward(z, t, ctx, [hint], context_ip=cip), e_plain)
        mixed = CtrLoRAEngine(sd_mixed, [sd_cn], ncfg, dtype=dtype, device="cuda:0", need_bwd=False)
        assert len(mixed.unet.ip_layers) == len(names)
        assert torch.equal(mixed.forward(z, t, ctx, [hint]), e_plain)
        e_ip = mixed.forward(z, t, ctx, [hint], context_ip=cip)
        assert rel_l2(e_ip, e_plain) > 1e-3          # the image prompt reaches eps
        # the per-key cache of a sampling run gives the same eps as the uncached pass
        with context_kv(mixed):
            assert torch.equal(mixed.forward(z, t, ctx, [hint], context_ip=cip), e_ip)
            assert torch.equal(mixed.forward(z, t, ctx, [hint], context_ip=cip), e_ip)
        if dtype == torch.float32:
            e32 = e_ip
        else:
            assert rel_l2(e_ip, e32) < 3e-2, rel_l2(e_ip, e32)
    torch.cuda.synchronize()
