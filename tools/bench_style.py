"""Cost of IP-Adapter style control at the benchmark's DDIM shape (B = 16, CFG 7.5, latent 64, SD1.5 width, bf16).

    python tools/bench_style.py [--S 50] [--rounds 5]      # DDIM steps/s with and without the image prompt, alternated
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_style.py --kernels
                                                          # kernel times: one eager CFG pass with ip, one without

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
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
