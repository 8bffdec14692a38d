"""What `scripts/train_ctrlora_finetune.py --graph` changes per optimizer step, measured through the loop the script runs:
`ctrlora_amd.trainer.Trainer.fit` with graph_step off (every kernel launched from Python) and on (the step replayed from
hipGraphs), on one MI355X.

    python tools/bench_train_script.py [--rounds 12] [--warmup 4] [--bs 1 8] [--tiny]

Workload: bench.py's model (configs/ctrlora_finetune_sd15_rank128.yaml, random weights, bf16 engine mode), one twin per leg;
synthetic batches that carry latents the way a `--latent_cache` run gets them -- the posterior moments of target and condition
(CPU fp32, 64 x 64 latents) and the text context as a given tensor -- so `get_input` does the two CPU-generator draws, the
pinned copies and the pair kernel, and no VAE or text encoder runs.  Method: the two fits run in two threads of ONE process that
hand the GPU to each other batch by batch (eager step, graph step, eager step, ...); a step is timed on the host clock from a
device synchronise before its batch is handed out to a device synchronise after the loop asks for the next one, so it holds
get_input, the draws, the step, log_dict and the callbacks.  Medians of `--rounds` steps per leg after `--warmup` rounds (the
graph leg launches its first two steps eagerly and captures before the third).  For the graph leg the host time from the batch
to the replay call (get_input + draws) and the GPU time of copies + replay (HIP events) are reported next to the wall time.
Writes profiles/train_graph/bench_train_graph.json and prints it as ONE JSON line.  No GPU, no number: the tool fails.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Turns:
    """Round-robin baton between the legs' threads; a leg that has finished (or failed) drops out."""

    def __init__(self, names):
        self.cv, self.names, self.i = threading.Condition(), list(names), 0

    def take(self, name):
        with self.cv:
            self.cv.wait_for(lambda: self.names[self.i % len(self.names)] == name)

    def give(self, name, leave=False):
        with self.cv:
            if leave:
                holder = self.names[self.i % len(self.names)]
                k = self.names.index(name)
                self.names.remove(name)
                if not self.names:
                    self.i = 0
                elif holder == name:
                    self.i = k % len(self.names)            # the baton goes to the leg that was next
                else:
                    self.i = self.names.index(holder)
            else:
                self.i = (self.i + 1) % len(self.names)
            self.cv.notify_all()


class TimedLoader:
    """Hands out `n` batches, each when it is this leg's turn, and times what the loop does with it."""

    def __init__(self, name, batches, n, turns):
        self.name, self.batches, self.n, self.turns = name, batches, n, turns
        self.ms, self.t_start = [], None

    def __iter__(self):
        import torch
        for i in range(self.n):
            self.turns.take(self.name)
            torch.cuda.synchronize()
            self.t_start = time.perf_counter()
            try:
                yield self.batches[i % len(self.batches)]
            finally:                       # the loop asked for the next batch, or closed the iterator after its last step
                torch.cuda.synchronize()
                self.ms.append((time.perf_counter() - self.t_start) * 1e3)
                self.turns.give(self.name)


def run_pair(models, B, args, work):
    import torch
    from ctrlora_amd.trainer import Trainer
    dev = torch.device("cuda", 0)
    n = args.warmup + args.rounds
    g = torch.Generator().manual_seed(100 + B)
    h = 16 if args.tiny else 64
    cd = models["eager"].control_model.context_dim

    def moments():
        return torch.cat([torch.randn(B, 4, h, h, generator=g), 0.05 + 0.1 * torch.rand(B, 4, h, h, generator=g)], 1)

    batches = [dict(jpg_moments=moments(), hint_moments=moments(), txt=torch.randn(B, 77, cd, generator=g).to(dev)) for _ in range(3)]
    turns = Turns(["eager", "graph"])
    legs, errors = {}, []
    split = []                              # graph leg: (host ms from the batch to the replay call, start event, end event)

    def leg(name):
        loader = TimedLoader(name, batches, n, turns)
        tr = Trainer(max_steps=n, precision=16, default_root_dir=os.path.join(work, f"{name}_b{B}"), log_every_n_steps=10 ** 9,
                     graph_step=(name == "graph"))
        if name == "graph":
            make = tr._make_graph_step

            def instrumented(model, tensors):
                step = make(model, tensors)
                real = step.micro

                def micro(*a, **k):
                    host = (time.perf_counter() - loader.t_start) * 1e3
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out = real(*a, **k)
                    e1.record()
                    split.append((host, e0, e1))
                    return out
                step.micro = micro
                return step
            tr._make_graph_step = instrumented
        legs[name] = (tr, loader)
        turns.take(name)                    # the set-up inside fit (engine build, optimizer) runs under the baton as well
        try:
            tr.fit(models[name], loader)
        except BaseException as e:          # the other leg must not wait for a baton that never comes
            errors.append((name, e))
        finally:
            turns.give(name, leave=True)

    threads = [threading.Thread(target=leg, args=(k,), name=k) for k in ("eager", "graph")]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise RuntimeError(f"leg {errors[0][0]} failed: {errors[0][1]!r}") from errors[0][1]
    torch.cuda.synchronize()
    out = dict(batch=B)
    for name, (tr, loader) in legs.items():
        ms = loader.ms[args.warmup:]
        assert len(ms) == args.rounds and tr.global_step == n
        med = statistics.median(ms)
        out[name] = dict(ms_per_step=round(med, 2), images_per_s=round(B * 1e3 / med, 2), ms_min_max=[round(min(ms), 2), round(max(ms), 2)],
                         steps_timed=len(ms), loss=round(float(models[name].last_logged["train/loss"]), 5))
    trg = legs["graph"][0]
    assert trg.graph_mode == "one" and trg.graph_eager_steps == 2 and trg.graph_replays == n - 2, "the graph leg did not replay"
    timed = split[-args.rounds:]
    host = statistics.median(s[0] for s in timed)
    gpu = statistics.median(s[1].elapsed_time(s[2]) for s in timed)
    out["graph"].update(replays=trg.graph_replays, eager_steps=trg.graph_eager_steps,
                        host_ms_batch_to_replay=round(host, 2), replay_gpu_ms=round(gpu, 2),
                        ms_outside_replay=round(out["graph"]["ms_per_step"] - gpu, 2))
    out["speedup"] = round(out["eager"]["ms_per_step"] / out["graph"]["ms_per_step"], 3)
    return out


def main(argv=None):
    import torch
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12, help="timed optimizer steps per leg")
    ap.add_argument("--warmup", type=int, default=4, help="untimed steps per leg before them (at least 3: two eager steps and the capture)")
    ap.add_argument("--bs", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--tiny", action="store_true", help="narrow model, 16 x 16 latents (rehearsal of the path, not a result)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_graph", "bench_train_graph.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_script needs a GPU: a CPU run measures nothing about the engine")
    if args.rounds < 12 or args.warmup < 3:
        raise SystemExit("at least 12 timed steps per leg after at least 3 warm-up steps")
    models = {}
    for name in ("eager", "graph"):
        m = bench.build_model("ctrlora_finetune_sd15_rank128.yaml", 0, tiny=args.tiny)
        m.scale_factor, m.learning_rate = 0.18215, 1e-5
        models[name] = m
    prev = os.getcwd()
    with tempfile.TemporaryDirectory(prefix="ctrlora_bench_train_") as work:
        os.chdir(work)                      # configure_optimizers writes ./tmp, the trainer its run directory
        try:
            results = [run_pair(models, B, args, work) for B in args.bs]
        finally:
            os.chdir(prev)
    res = dict(
        metric="ms per optimizer step of Trainer.fit, eager launches against hipGraph replay (--graph), one MI355X",
        results=results, rank=128, dtype="bfloat16", latent="16x16" if args.tiny else "64x64", tiny=bool(args.tiny),
        rounds=args.rounds, warmup=args.warmup,
        step="get_input from posterior moments (two CPU draws, pinned copies, pair kernel) + t / noise draws + forward + loss + "
             "backward + fused AdamW + re-pack + log_dict, as Trainer.fit runs it",
        method="two fits in two threads of one process alternate batch by batch; host clock between device synchronises; medians; "
               "replay_gpu_ms = HIP events around the copies into the static tensors and the replay")
    if not args.tiny:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
