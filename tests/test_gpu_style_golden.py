"""IP-Adapter style control on the GPU against the reference fixture (tests/golden/make_golden_style.py), class-API path.

  * cldm_style.ControlledUnetModel (tiny width, mixed per-layer ip_scale) with and without image-prompt tokens, and
    ControlInferenceLDM.apply_model with c_ip, built from configs/inference/ctrlora_style_sd15_rank128_1lora.yaml: fp32
    at the 1e-5 level, bf16 within k x the bf16-vs-fp32 distance of the same engine (and an absolute bound);
  * graphed DDIM (S = 10, B = 2, CFG 7.5, c_ip in both branches) equals the eager sampler, replays stably, and a changed
    ip_scale or newly loaded to_k_ip / to_v_ip weights re-capture instead of replaying a stale graph.
"""
import os

import pytest
import torch

from tests.util import GOLDEN, rel_l2

pytestmark = pytest.mark.gpu
PREFIX = "model.diffusion_model."


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _gold():
    return torch.load(os.path.join(GOLDEN, "style_tiny.pt"), weights_only=False)


def _style_model(dtype):
    import bench
    from oracle import arch
    from tests.golden.make_golden_style import SEED, ip_weights
    model = bench.build_model("inference/ctrlora_style_sd15_rank128_1lora.yaml", 0, tiny=True).cuda().eval()
    unet = model.model.diffusion_model
    shapes = arch.unet_shapes(arch.TINY)
    sd = arch.make_state(shapes, SEED)
    sd.update(ip_weights([k for k in unet.state_dict()], shapes, SEED))
    unet.load_state_dict(sd, strict=True)
    model.set_engine_dtype(dtype)
    return model


def test_style_unet_and_apply_model_vs_reference():
    _need_gpu()
    g = _gold()
    inp = {k: v.cuda() for k, v in g["inputs"].items()}
    got = {}
    for dtype in (torch.float32, torch.bfloat16):
        model = _style_model(dtype)
        unet = model.model.diffusion_model
        with torch.no_grad():
            e_ip = unet(inp["z"], timesteps=inp["t"], context=[[inp["ctx"], inp["ip"]]])
            e_txt = unet(inp["z"], timesteps=inp["t"], context=[[inp["ctx"], None]])
            cond = dict(c_crossattn=[inp["ctx"]], c_concat=[None], c_ip=[inp["ip"]])
            e_am = model.apply_model(inp["z"], inp["t"], cond)
        got[dtype] = (e_ip, e_txt, e_am)
        del model
    refs = (g["eps_ip"], g["eps_txt"], g["apply_model_ip"])
    assert rel_l2(refs[0], refs[1]) > 1e-2                  # the image prompt matters at this scale pattern
    for name, a32, a16, ref in zip(("eps_ip", "eps_txt", "apply_model"), got[torch.float32], got[torch.bfloat16], refs):
        e32, e16, cmp = rel_l2(a32, ref), rel_l2(a16, ref), rel_l2(a16, a32)
        print(f"[style] {name}: fp32 {e32:.2e}  bf16 {e16:.2e}  bf16-vs-fp32 {cmp:.2e}")
        assert e32 < 2e-5, (name, e32)
        assert e16 < 1.5 * cmp + 1e-4 and e16 < 3e-2, (name, e16, cmp)


def test_style_graphed_ddim_matches_eager_and_recaptures():
    _need_gpu()
    from cldm.ddim_hacked import DDIMSampler
    from ctrlora_amd.engine import nets
    from oracle import arch
    cfg = arch.TINY
    model = _style_model(torch.float32)
    B, H, S = 2, 16, 10
    g = torch.Generator().manual_seed(9)
    hint = torch.randn(B, 4, H, H, generator=g).cuda()
    ip, ip_u = torch.randn(B, 4, cfg.context_dim, generator=g).cuda(), torch.zeros(B, 4, cfg.context_dim).cuda()
    cond = {"c_concat": [hint], "c_crossattn": [torch.randn(B, 77, cfg.context_dim, generator=g).cuda()], "c_ip": [ip]}
    unc = {"c_concat": [hint], "c_crossattn": [torch.randn(B, 77, cfg.context_dim, generator=g).cuda()], "c_ip": [ip_u]}
    x_T = torch.randn(B, 4, H, H, generator=g).cuda()

    def run(s, c=cond, u=unc):
        return s.sample(S, B, (4, H, H), c, verbose=False, eta=0.0, x_T=x_T, unconditional_guidance_scale=7.5,
                        unconditional_conditioning=u)[0]

    from ldm.models.diffusion.guided_loop import cat_conds
    both = cat_conds(cond, unc)
    assert both is not None and both["c_ip"][0].shape[0] == 2 * B      # c_ip rides the 2B CFG batch
    eager = DDIMSampler(model)
    eager.use_graph = False
    a_eager = run(eager)
    sampler = DDIMSampler(model)
    sampler.reuse_graph = True
    a0 = run(sampler)
    assert rel_l2(a0, a_eager) < 1e-5, rel_l2(a0, a_eager)
    a1 = run(sampler)
    assert sampler.graph_hits == 1 and rel_l2(a1, a0) < 1e-6
    # without c_ip the samples are the plain UNet's
    plain = {k: v for k, v in cond.items() if k != "c_ip"}, {k: v for k, v in unc.items() if k != "c_ip"}
    assert rel_l2(run(DDIMSampler(model), *plain), a0) > 1e-3
    # (1) a changed ip_scale (load_state_dict of the scale buffers, as the app's targets do)
    from cldm.style_helpers import ip_scale_state
    model.load_state_dict(ip_scale_state("Load only style blocks", 0.9), strict=False)
    hits = sampler.graph_hits
    b0 = run(sampler)
    assert sampler.graph_hits == hits, "a changed ip_scale must not replay the old graph"
    assert rel_l2(b0, run(DDIMSampler(model))) < 1e-5 and rel_l2(b0, a0) > 1e-4
    # (2) newly loaded IP-Adapter weights
    gen = nets.WEIGHTS_GENERATION[0]
    sd = model.model.diffusion_model.state_dict()
    new = {PREFIX + k: v * 1.5 for k, v in sd.items() if k.endswith("to_v_ip.weight")}
    model.load_state_dict(new, strict=False)
    hits = sampler.graph_hits
    c0 = run(sampler)
    assert sampler.graph_hits == hits, "reloaded ip weights must not replay the old graph"
    assert rel_l2(c0, run(DDIMSampler(model))) < 1e-5 and rel_l2(c0, b0) > 1e-4
    assert nets.WEIGHTS_GENERATION[0] >= gen
    torch.cuda.synchronize()
