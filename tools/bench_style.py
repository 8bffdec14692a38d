"""Cost of IP-Adapter style control at the benchmark's DDIM shape (B = 16, CFG 7.5, latent 64, SD1.5 width, bf16).

    python tools/bench_style.py [--S 50] [--rounds 5]      # DDIM steps/s with and without the image prompt, alternated
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_style.py --kernels
                                                          # kernel times: one eager CFG pass with ip, one without
    python tools/bench_style.py --with-encoder [--images 1] [--layers 32] [--encoder-dtype bf16]
                                                          # the style image's encode (CLIP ViT-H/14, seeded weights): the engine
                                                          # against the HF module on the same GPU in the same dtype, alternated
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_style.py --with-encoder --kernels   # its per-kernel split

Both legs sample from the same model (IP-Adapter weights in all 16 cross-attentions, every ip_scale 1) with the same
tensors; "without" drops `c_ip` from both conditionings, which is the plain multi-LoRA inference.  Each leg keeps its own
captured step graph (sampler.reuse_graph) and the legs alternate, so clock drift hits both.  One JSON line.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build(B=16, H=64, Nip=4):
    import bench
    from cldm.style_helpers import ip_scale_state
    model = bench.build_model("inference/ctrlora_style_sd15_rank128_1lora.yaml", 0).cuda().eval()
    g = torch.Generator().manual_seed(11)
    sd = model.model.diffusion_model.state_dict()
    ip = {"model.diffusion_model." + k: (torch.randn(v.shape, generator=g) * 0.02).to(v.device)
          for k, v in sd.items() if k.endswith("_ip.weight")}
    ip.update(ip_scale_state("Load original IP-Adapter", 1.0))
    model.load_state_dict(ip, strict=False)
    model.set_engine_dtype(torch.bfloat16)
    cd = model.control_model.context_dim
    hint = torch.randn(B, 4, H, H, generator=g).cuda()
    cond = {"c_concat": [hint], "c_crossattn": [torch.randn(B, 77, cd, generator=g).cuda()],
            "c_ip": [torch.randn(B, Nip, cd, generator=g).cuda()]}
    unc = {"c_concat": [hint], "c_crossattn": [torch.randn(B, 77, cd, generator=g).cuda()],
           "c_ip": [torch.zeros(B, Nip, cd).cuda()]}
    x_T = torch.randn(B, 4, H, H, generator=g).cuda()
    return model, cond, unc, x_T


def encoder_leg(a):
    """Encode of `--images` style images: ClipVisionE (ctrlora_amd/engine/vit.py) against the same HF module on the same GPU
    in the same dtype, alternated round by round; medians of per-call times (each call synchronised: an encode is one
    request of the app, not a stream of them).  Also the fp32 parity of the engine against the HF module on this GPU."""
    from cldm.style_helpers import VIT_H_14, CLIPVisionEncoder
    dtype = torch.float32 if a.encoder_dtype in ("f32", "fp32") else torch.bfloat16
    torch.manual_seed(0)
    enc = CLIPVisionEncoder(dict(VIT_H_14, num_hidden_layers=a.layers)).cuda().eval()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():                   # off the init scale: gammas, betas and biases that matter
        for n, p in enc.named_parameters():
            if n.endswith(".bias"):
                p.copy_((0.1 * torch.randn(p.shape, generator=g)).to(p.device))
            elif "norm" in n and n.endswith(".weight"):
                p.copy_((1.0 + 0.1 * torch.randn(p.shape, generator=g)).to(p.device))
    enc.set_engine_dtype(dtype)
    x = torch.randn(a.images, 3, 224, 224, generator=g).cuda()
    hf = enc._hf
    hf_t = CLIPVisionEncoder(enc.config).cuda().eval() if dtype != torch.float32 else None
    if hf_t is not None:                    # the app's form: the module's weights in the low-precision dtype
        hf_t.load_state_dict(enc.state_dict())
        hf_t = hf_t._hf.to(dtype)
    run_hf = (lambda: hf(pixel_values=x).image_embeds) if hf_t is None else (lambda: hf_t(pixel_values=x.to(dtype)).image_embeds)
    with torch.no_grad():
        run_eng = lambda: enc(x).image_embeds
        if a.kernels:
            for _ in range(3):
                run_eng()
            torch.cuda.synchronize()
            print(json.dumps(dict(tool="bench_style", mode="encoder-kernels", layers=a.layers, images=a.images, passes=3)))
            return
        legs = {"engine": run_eng, "hf": run_hf}
        for f in legs.values():
            for _ in range(3):
                f()
        times = {n: [] for n in legs}
        for _ in range(a.rounds):
            for n, f in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                times[n].append(time.perf_counter() - t0)
        med = {n: sorted(v)[len(v) // 2] for n, v in times.items()}
        # parity on this GPU: fp32 engine against the fp32 HF module
        enc.set_engine_dtype(torch.float32)
        e32, want = enc(x).image_embeds.double(), hf(pixel_values=x).image_embeds.double()
        par = float((e32 - want).norm() / want.norm())
        enc.set_engine_dtype(dtype)
        low = float((run_eng().double() - want).norm() / want.norm())
        low_hf = float((run_hf().double() - want).norm() / want.norm())
    print(json.dumps(dict(tool="bench_style", mode="encoder", layers=a.layers, images=a.images, dtype=str(dtype), rounds=a.rounds,
                          engine_ms=round(1e3 * med["engine"], 3), hf_ms=round(1e3 * med["hf"], 3),
                          hf_over_engine=round(med["hf"] / med["engine"], 3), all_engine_ms=[round(1e3 * t, 3) for t in times["engine"]],
                          all_hf_ms=[round(1e3 * t, 3) for t in times["hf"]], embeds_rel_l2_fp32_vs_hf_fp32=par,
                          embeds_rel_l2_engine_vs_hf_fp32=low, embeds_rel_l2_hf_lowp_vs_hf_fp32=low_hf)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--with-encoder", action="store_true", help="time the style image's CLIP encode instead of the DDIM legs")
    ap.add_argument("--images", type=int, default=1)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--encoder-dtype", default="bf16")
    a = ap.parse_args()
    if a.with_encoder:
        return encoder_leg(a)
    from cldm.ddim_hacked import DDIMSampler
    B, H = 16, 64
    model, cond, unc, x_T = build(B, H)
    drop = lambda c: {k: v for k, v in c.items() if k != "c_ip"}
    legs = {"ip": (cond, unc), "plain": (drop(cond), drop(unc))}
    if a.kernels:
        t = torch.full((2 * B,), 500, dtype=torch.long, device="cuda")
        x = torch.cat([x_T, x_T])
        with torch.no_grad():
            for name, (c, u) in legs.items():
                both = {k: [torch.cat([p, q]) for p, q in zip(c[k], u[k])] for k in c}
                for _ in range(3):
                    model.apply_model(x, t, both)
        torch.cuda.synchronize()
        print(json.dumps(dict(tool="bench_style", mode="kernels", passes_per_leg=3)))
        return
    samplers = {}
    for name in legs:
        samplers[name] = s = DDIMSampler(model)
        s.reuse_graph = True
    run = lambda name, S: samplers[name].sample(S, B, (4, H, H), legs[name][0], verbose=False, eta=0.0, x_T=x_T,
                                                unconditional_guidance_scale=7.5, unconditional_conditioning=legs[name][1])
    for name in legs:
        run(name, 6)
        run(name, a.S)
        run(name, a.S)
    times = {n: [] for n in legs}
    for _ in range(a.rounds):
        for name in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out, _ = run(name, a.S)
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
            assert torch.isfinite(out).all()
    med = {n: sorted(v)[len(v) // 2] for n, v in times.items()}
    sps = {n: a.S / med[n] for n in legs}
    print(json.dumps(dict(tool="bench_style", B=B, latent=H, cfg=7.5, S=a.S, rounds=a.rounds,
                          steps_per_s_ip=round(sps["ip"], 3), steps_per_s_plain=round(sps["plain"], 3),
                          slowdown_pct=round(100.0 * (med["ip"] / med["plain"] - 1.0), 2),
                          graph_hits={n: samplers[n].graph_hits for n in legs})))


if __name__ == "__main__":
    main()
