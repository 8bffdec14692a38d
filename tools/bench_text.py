"""Encode time of the CLIP text encoders: the engine (ctrlora_amd/engine/clip_text.py) against the HF module on the same GPU.

    python tools/bench_text.py [--B 16] [--N 77] [--dtype bf16|f32] [--models vit-l,vit-h] [--iters 50] [--warmup 10] [--layers L]

ViT-L/14 text (FrozenCLIPEmbedder: 768 / 12 heads / 12 layers / quick_gelu) and ViT-H/14 text (the style app's negative content
prompt: 1024 / 16 heads / 24 layers / gelu), seeded weights, B = 16 prompts of N = 77 tokens.  Four legs per model, alternated
round by round so clock drift hits all of them: engine eager, engine as ONE graph replay, HF eager, HF as one graph replay (the
HF module in the engine's dtype: its weights cast for bf16, as the app does for fp16).  HIP events around every call, `--warmup`
unrecorded rounds, medians of `--iters`.  Also the rel-L2 of each leg's last_hidden_state against the fp32 HF module on this
GPU.  One JSON line per model.  No test gates on these numbers.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MODELS = {
    "vit-l": dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
                  max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, projection_dim=768),
    "vit-h": dict(vocab_size=49408, hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16,
                  max_position_embeddings=77, hidden_act="gelu", layer_norm_eps=1e-5, projection_dim=1024),
}


def _graphed(fn):
    """fn captured once (after a side-stream warm-up, as torch.cuda.graph asks); returns (replay, the captured output)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    return graph.replay, out


def bench_model(name, a):
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    from ctrlora_amd.engine.clip_text import ClipTextE
    dtype = torch.float32 if a.dtype in ("f32", "fp32") else torch.bfloat16
    cfg = dict(MODELS[name])
    if a.layers:
        cfg["num_hidden_layers"] = a.layers
    torch.manual_seed(0)
    hf32 = CLIPTextModelWithProjection(CLIPTextConfig(**cfg)).eval()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():                   # off the init scale: gammas, betas and biases that matter
        for n, p in hf32.named_parameters():
            if n.endswith(".bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif "norm" in n and n.endswith(".weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
    hf32 = hf32.cuda()
    ids = torch.randint(1, cfg["vocab_size"] - 2, (a.B, a.N), generator=g)
    ids[:, -1] = cfg["vocab_size"] - 1
    ids = ids.cuda()
    ex = ClipTextE(hf32.state_dict(), cfg, dtype, "cuda")
    hf = hf32 if dtype == torch.float32 else CLIPTextModelWithProjection(CLIPTextConfig(**cfg)).eval().cuda()
    if hf is not hf32:
        hf.load_state_dict(hf32.state_dict())
        hf = hf.to(dtype)
    want = ("last_hidden_state", "text_embeds")
    with torch.no_grad():
        run_eng = lambda: ex.forward(ids, want=want)["last_hidden_state"]
        run_hf = lambda: hf(input_ids=ids).last_hidden_state
        ref = hf32(input_ids=ids).last_hidden_state.double()
        rel = lambda t: float((t.double() - ref).norm() / ref.norm())
        parity = dict(engine=rel(run_eng()), hf=rel(run_hf()))
        eng_replay, eng_out = _graphed(run_eng)
        hf_replay, hf_out = _graphed(run_hf)
        legs = {"engine_eager": run_eng, "engine_graph": eng_replay, "hf_eager": run_hf, "hf_graph": hf_replay}
        times = {n: [] for n in legs}
        for it in range(a.warmup + a.iters):
            for n, f in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                if it >= a.warmup:
                    times[n].append(e0.elapsed_time(e1))
        parity.update(engine_graph=rel(eng_out), hf_graph=rel(hf_out))
    med = {n: sorted(v)[len(v) // 2] for n, v in times.items()}
    print(json.dumps(dict(tool="bench_text", model=name, layers=cfg["num_hidden_layers"], B=a.B, N=a.N, dtype=str(dtype), iters=a.iters,
                          warmup=a.warmup, median_ms={n: round(t, 4) for n, t in med.items()},
                          min_ms={n: round(min(v), 4) for n, v in times.items()}, max_ms={n: round(max(v), 4) for n, v in times.items()},
                          hf_over_engine_eager=round(med["hf_eager"] / med["engine_eager"], 3),
                          hf_over_engine_graph=round(med["hf_graph"] / med["engine_graph"], 3),
                          last_hidden_rel_l2_vs_hf_fp32=parity, engine_forwards=ex.forwards)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--N", type=int, default=77)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--models", default="vit-l,vit-h")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--layers", type=int, default=0, help="override the number of layers (0: the model's own)")
    a = ap.parse_args()
    for name in a.models.split(","):
        bench_model(name, a)


if __name__ == "__main__":
    main()
