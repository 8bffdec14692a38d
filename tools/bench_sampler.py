"""DDIM with 50 steps against DPM-Solver++ with 20 at the benchmark's DDIM shape (B = 16, CFG 7.5, latent 64, SD1.5 width, bf16).

    python tools/bench_sampler.py [--rounds 5] [--ddim-steps 50] [--dpm-steps 20] [--plms-steps 0] [--out FILE]

Both legs sample from the same model with the same tensors through one sample() call each, as a one-shot user pays it:
the first step eager, the second captured as a hipGraph, the rest replayed (neither leg keeps a graph across calls: the
DPM-Solver++ sampler has no reuse_graph, so DDIM's stays off here and its figure is the "cold" one of bench.py, not the
headline).  A call ends in a device synchronise and is timed with the host clock; both legs run once untimed at their
timed length, then alternate round by round so that clock drift hits both; the medians are reported.  ms per step is
ms per batch over the number of steps, so it carries each leg's share of the eager step and the capture.  One JSON line;
a missing GPU is an error, not a fallback.  Whether 20 DPM-Solver++ steps match the quality of 50 DDIM steps is the
solver paper's claim (arXiv:2211.01095), not something this tool measures.  --plms-steps N > 0 adds a PLMS leg of N steps
(N + 1 model evaluations: its first iteration makes two, both eager) to the same rounds; 0, the default, leaves it out.

    python tools/bench_sampler.py --masked [--rounds 5] [--ddim-steps 50] [--out FILE]

--masked measures the image-editing paths of DDIMSampler instead, at the same shape and in the same manner: sample(mask=, x0=)
on the replayed loop, the same call with use_graph = False (every step driven from Python: q_sample, three ATen broadcasts,
the model, the update -- what a masked run cost before the blend kernel), and the unmasked replayed loop as the yardstick; then
decode() of the last half of the schedule (t_start = steps // 2), replayed and with use_graph = False.  The forward-process
noise is drawn at every step (q_noise = None), as a user's run draws it.
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--dpm-steps", type=int, default=20)
    ap.add_argument("--plms-steps", type=int, default=0, help="add a PLMS leg of this many steps (0: none)")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--tiny", action="store_true", help="narrow model: a rehearsal of the tool, not a measurement")
    ap.add_argument("--masked", action="store_true", help="measure masked sampling and decode(), replayed against eager")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_sampler.py needs a GPU: a CPU timing says nothing about the samplers")
    import bench
    from cldm.ddim_hacked import DDIMSampler
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    B, H = a.batch, 64
    model = bench.build_model("inference/ctrlora_sd15_rank128_1lora.yaml", 0, tiny=a.tiny).cuda().eval()
    model.set_engine_dtype(torch.bfloat16)
    cd = model.control_model.context_dim
    g = torch.Generator().manual_seed(7)
    hint = torch.randn(B, 4, H, H, generator=g).cuda()
    cond = {"c_concat": [hint], "c_crossattn": [torch.randn(B, 77, cd, generator=g).cuda()]}
    unc = {"c_concat": [hint], "c_crossattn": [torch.randn(B, 77, cd, generator=g).cuda()]}
    x_T = torch.randn(B, 4, H, H, generator=g).cuda()
    legs = {"ddim": (DDIMSampler(model), a.ddim_steps), "dpm": (DPMSolverSampler(model), a.dpm_steps)}
    if a.plms_steps > 0:
        from ldm.models.diffusion.plms import PLMSSampler
        legs["plms"] = (PLMSSampler(model), a.plms_steps)

    if a.masked:
        return masked_legs(a, model, cond, unc, x_T, g)

    def run(name):
        sampler, S = legs[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, _ = sampler.sample(S, B, (4, H, H), cond, verbose=False, eta=0.0, x_T=x_T, unconditional_guidance_scale=7.5,
                                unconditional_conditioning=unc)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert bool(torch.isfinite(out).all()), name
        return dt

    for name in legs:           # warm-up at the timed length: code objects, allocator, the capture path
        run(name)
    times = {name: [] for name in legs}
    for _ in range(a.rounds):
        for name in legs:
            times[name].append(run(name))
    res = dict(metric="ms per batch of one sample() call (eager first step + capture + replays), CFG 7.5, both passes batched",
               batch=B, latent=H, dtype="bf16", rounds=a.rounds, tiny=bool(a.tiny), gpu=torch.cuda.get_device_name(0))
    for name, (_, S) in legs.items():
        ts = sorted(times[name])
        med = ts[len(ts) // 2]
        res[name] = dict(steps=S, ms_per_batch=round(med * 1e3, 2), ms_per_step=round(med / S * 1e3, 3),
                         min_ms_per_batch=round(ts[0] * 1e3, 2), max_ms_per_batch=round(ts[-1] * 1e3, 2))
    res["dpm_over_ddim_batch_time"] = round(res["dpm"]["ms_per_batch"] / res["ddim"]["ms_per_batch"], 4)
    res["dpm_over_ddim_step_time"] = round(res["dpm"]["ms_per_step"] / res["ddim"]["ms_per_step"], 4)
    if "plms" in legs:
        res["plms_over_ddim_batch_time"] = round(res["plms"]["ms_per_batch"] / res["ddim"]["ms_per_batch"], 4)
        res["plms_over_ddim_step_time"] = round(res["plms"]["ms_per_step"] / res["ddim"]["ms_per_step"], 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def masked_legs(a, model, cond, unc, x_T, g):
    from cldm.ddim_hacked import DDIMSampler
    B, H, S = a.batch, x_T.shape[-1], a.ddim_steps
    x0 = torch.randn(B, 4, H, H, generator=g).cuda()
    mask = torch.zeros(1, 1, H, H).cuda()
    mask[..., : H // 2] = 1.0                       # keep the left half
    t_start = S // 2

    def sampler(use_graph):
        s = DDIMSampler(model)
        s.use_graph = use_graph
        return s

    kw = dict(verbose=False, eta=0.0, x_T=x_T, unconditional_guidance_scale=7.5, unconditional_conditioning=unc)

    def decode(s):
        s.make_schedule(S, ddim_eta=0.0, verbose=False)
        return s.decode(x_T, cond, t_start, unconditional_guidance_scale=7.5, unconditional_conditioning=unc)

    legs = {
        "masked_graphed": (S, lambda: sampler(True).sample(S, B, (4, H, H), cond, mask=mask, x0=x0, **kw)[0]),
        "masked_eager": (S, lambda: sampler(False).sample(S, B, (4, H, H), cond, mask=mask, x0=x0, **kw)[0]),
        "unmasked_graphed": (S, lambda: sampler(True).sample(S, B, (4, H, H), cond, **kw)[0]),
        "decode_graphed": (t_start, lambda: decode(sampler(True))),
        "decode_eager": (t_start, lambda: decode(sampler(False))),
    }

    def run(name):
        import contextlib
        import io
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):          # decode() announces its step count
            out = legs[name][1]()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert bool(torch.isfinite(out).all()), name
        return dt

    for name in legs:           # warm-up at the timed length
        run(name)
    times = {name: [] for name in legs}
    for _ in range(a.rounds):
        for name in legs:
            times[name].append(run(name))
    res = dict(metric="ms per batch of one sample() / decode() call, CFG 7.5, both passes batched; graphed = eager first step + "
                      "capture + replays, eager = use_graph False", batch=B, latent=H, dtype="bf16", rounds=a.rounds,
               tiny=bool(a.tiny), gpu=torch.cuda.get_device_name(0))
    for name, (steps, _) in legs.items():
        ts = sorted(times[name])
        med = ts[len(ts) // 2]
        res[name] = dict(steps=steps, ms_per_batch=round(med * 1e3, 2), ms_per_step=round(med / steps * 1e3, 3),
                         min_ms_per_batch=round(ts[0] * 1e3, 2), max_ms_per_batch=round(ts[-1] * 1e3, 2))
    ratio = lambda p, q: round(res[p]["ms_per_batch"] / res[q]["ms_per_batch"], 4)
    res["masked_graphed_over_masked_eager"] = ratio("masked_graphed", "masked_eager")
    res["masked_graphed_over_unmasked_graphed"] = ratio("masked_graphed", "unmasked_graphed")
    res["decode_graphed_over_decode_eager"] = ratio("decode_graphed", "decode_eager")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
