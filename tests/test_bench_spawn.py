"""`python bench.py --gpus N` without a launcher starts its own ranks: the command it builds, the
pass-through of rank 0's JSON line, and the single retry with --no-graph when the hipGraph data-parallel run fails.
No GPU, no processes: subprocess.run is replaced -- except in the last test, which really starts two ranks (gloo)."""
import os
import json
import subprocess
import sys
import types

import bench


def _fake_run(results, calls):
    def run(cmd, env=None, stdout=None, text=None):
        calls.append((list(cmd), dict(env or {})))
        rc, out = results[min(len(calls) - 1, len(results) - 1)]
        return types.SimpleNamespace(returncode=rc, stdout=out)
    return run


def test_spawn_builds_the_torchrun_command_and_passes_the_line_through(monkeypatch, capsys):
    calls = []
    line = json.dumps({"metric": "512x512 LoRA-finetune images/sec", "value": 1.0, "n_gpus": 4})
    monkeypatch.setattr(subprocess, "run", _fake_run([(0, "Optimizable params: 36.9M\n" + line + "\n")], calls))
    rc = bench.spawn_ranks(4, ["--gpus", "4", "--steps", "7", "--warmup", "2"])
    assert rc == 0 and len(calls) == 1
    cmd, env = calls[0]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    assert cmd[-6:] == ["--gpus", "4", "--steps", "7", "--warmup", "2"] and cmd[-7].endswith("bench.py")
    assert env.get("HSA_ENABLE_IPC_MODE_LEGACY") == "0"
    assert capsys.readouterr().out.strip() == line          # exactly ONE JSON line on stdout


def test_spawn_retries_once_without_graphs_when_the_graph_run_fails(monkeypatch, capsys):
    calls = []
    line = json.dumps({"metric": "m", "value": 2.0, "config": {"launch": "eager"}})
    monkeypatch.setattr(subprocess, "run", _fake_run([(1, "Traceback ...\n"), (0, line + "\n")], calls))
    rc = bench.spawn_ranks(8, ["--gpus", "8"])
    assert rc == 0 and len(calls) == 2
    assert "--no-graph" not in calls[0][0] and calls[1][0][-1] == "--no-graph"
    assert capsys.readouterr().out.strip() == line
    # a second failure is reported, not retried again
    calls.clear()
    monkeypatch.setattr(subprocess, "run", _fake_run([(1, "boom\n")], calls))
    assert bench.spawn_ranks(2, ["--gpus", "2"]) != 0 and len(calls) == 2


def test_main_self_spawns_only_without_a_launcher(monkeypatch):
    seen = {}
    monkeypatch.setattr(bench, "spawn_ranks", lambda n, argv: seen.setdefault("n", n) and 0 or 0)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    monkeypatch.delenv("RANK", raising=False); monkeypatch.delenv("WORLD_SIZE", raising=False)
    try:
        bench.main()
    except SystemExit as e:
        assert e.code == 0
    assert seen.get("n") == 2


def test_two_real_ranks_through_spawn_ranks_rendezvous_allreduce_and_print_one_line():
    """`python bench.py --gpus 2 --dist-dry-run` as a user would type it: bench.py starts its own two ranks under
    torch.distributed.run (spawn_ranks), they rendezvous on 127.0.0.1 (gloo on this CPU-only host, RCCL on a GPU node),
    all-reduce a bucket per step inside the timed region's barrier / MAX bracket, and rank 0 prints exactly one JSON line."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dist-dry-run", "--steps", "3", "--warmup", "1"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["dry_run"] and out["steps"] == 3 and out["allreduce_sum_correct_on_every_rank"]
    assert out["backend"] in ("gloo", "nccl") and out["value"] > 0


def test_eight_real_ranks_through_spawn_ranks_dry_run():
    """The first 8-rank contact, without GPUs (VERDICT r5 next #8a): `python bench.py --gpus 8 --dist-dry-run` starts eight real
    torch.distributed.run ranks (gloo here, RCCL on a GPU node), which rendezvous on 127.0.0.1, all-reduce a bucket per step inside
    the measured region's barrier / MAX bracket, and rank 0 prints one JSON line that carries the rank count it saw."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "8", "--dist-dry-run", "--steps", "3", "--warmup", "1"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 8 and out["world"] == 8 and out["dry_run"] and out["allreduce_sum_correct_on_every_rank"]
    assert len(out["ms_per_step_by_rank"]) == 8 and all(v > 0 for v in out["ms_per_step_by_rank"])


def test_static_artefacts_the_bench_quotes_carry_commit_and_source_hash(tmp_path):
    """every static number in the bench line (HBM traffic of the dominant kernel, its in-step rocprof time, the
    stock comparator) names the commit it was measured at and is flagged `stale` when csrc/gemm.hip has changed since."""
    import json
    import bench
    r = bench.dominant_kernel_rocprof()
    assert r is not None and {"us_per_launch", "table", "measured_at_commit", "source_sha256_then", "source_sha256_now", "stale"} <= set(r)
    assert r["stale"] == (r["source_sha256_then"] != r["source_sha256_now"])
    with open(os.path.join(bench.ROOT, "profiles", "dominant_kernel_traffic.json")) as f:
        t = json.load(f)
    p = bench.provenance(t)
    assert p["measured_at_commit"] and p["source_sha256_then"] and p["stale"] == (p["source_sha256_then"] != bench.src_hash("ctrlora_amd/csrc/gemm.hip"))
    assert bench.provenance({})["stale"] and bench.provenance(None)["stale"]            # nothing recorded = stale
    ips, src = bench.stock_reference()
    assert ips > 0 and src.startswith("profiles/")


def test_dump_outputs_writes_a_fixed_sample_of_the_last_step(tmp_path):
    """`--dump-outputs DIR`: loss (float64) and the same DUMP_SAMPLE positions of the fp32 master trainables and their gradient
    (float32) in every run, whatever the buffer size; well under the 64 MB an output set may take."""
    import numpy as np
    import torch
    n = bench.DUMP_SAMPLE + 12345
    exs = [types.SimpleNamespace(tr=types.SimpleNamespace(flat=torch.arange(m, dtype=torch.float32) + off,
                                                          flat_grad=-torch.arange(m, dtype=torch.float32) - off))
           for m, off in ((n - 1000, 0), (1000, n - 1000))]
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), torch.tensor(0.25), exs)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["grads.npy", "loss.npy", "params.npy"]
    loss, p, g = (np.load(tmp_path / "a" / f) for f in ("loss.npy", "params.npy", "grads.npy"))
    assert loss.dtype == np.float64 and float(loss) == 0.25
    assert p.dtype == g.dtype == np.float32 and p.shape == g.shape == (bench.DUMP_SAMPLE,)
    assert np.all(np.diff(p) > 0) and p[-1] < n and np.array_equal(g, -p)      # distinct ascending positions of both executors
    assert p[-1] >= n - 1000                                                    # the second executor's buffer is sampled too
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) < 64 << 20
    small = [types.SimpleNamespace(tr=types.SimpleNamespace(flat=torch.ones(10), flat_grad=torch.zeros(10)))]
    bench.dump_outputs(str(tmp_path / "c"), torch.tensor(1.0), small)
    assert np.load(tmp_path / "c" / "params.npy").shape == (10,)


def test_optimizer_setup_writes_nothing_into_the_working_directory(tmp_path, monkeypatch):
    """configure_optimizers() writes its trainable-name report to ./tmp (as the reference does): the benchmark runs it from a
    throw-away directory, so a read-only checkout works and the checkout stays untouched; the working directory comes back."""
    monkeypatch.chdir(tmp_path)
    seen = {}

    class M:
        def configure_optimizers(self):
            seen["cwd"] = os.getcwd()
            os.makedirs("./tmp", exist_ok=True)
            with open("./tmp/finetune_trainable_params.txt", "w") as f:
                f.write("x\n")
            return "opt"

    assert bench.configure_optimizers(M()) == "opt"
    assert os.getcwd() == str(tmp_path) and os.listdir(tmp_path) == []
    assert seen["cwd"] != str(tmp_path) and not os.path.exists(seen["cwd"])

    class Boom:
        def configure_optimizers(self):
            raise RuntimeError("boom")

    try:
        bench.configure_optimizers(Boom())
    except RuntimeError:
        pass
    assert os.getcwd() == str(tmp_path)
