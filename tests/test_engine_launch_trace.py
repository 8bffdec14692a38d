"""Every launch a whole ControlNet + UNet pass issues, argument for argument, against a recorded trace -- on the CPU, with the
recording stand-in of tests/test_engine_launch_sequence.py in place of libctrlora_hip.so (no kernel runs).

blocks.py / nets.py decide per LoRACompatibleLinear how its product runs (folded, live LoRA, grouped) and which of W / Wm /
Wt / A / Bt ... feeds it.  A product that reads W where it should read Wm has the right shape and the wrong numbers, so a
change to that seam is checked here before it reaches a GPU: tests/golden/engine_launch_trace.json holds, per scenario, the
number of launches and a sha256 per block of 32 consecutive launches of the CANONICAL trace:

  * every call is (entry point, arguments); GemmParams and the WgradDesc array are decoded field by field, float arguments
    are rounded through c_float;
  * while a scenario runs, every tensor whose address is taken is kept alive, so no address is ever reused and a pointer's
    identity does not depend on the allocator;
  * a pointer that is the address of a tensor held by a packing object (LinearW, LoraGroup, Conv3W, NormW, Trainable) becomes
    "<field>#<n>" -- n counts the distinct addresses of that field in order of first appearance -- so W, Wm, Wt, A, Bt, gamma,
    _geglu[0], _phase[up2] ... are told apart even at equal shapes; any other pointer becomes "p#<n>"; null stays null.

The golden file is a recording of the engine, not a derivation: it changes only with a pull request that means to change what
is launched.  To compare two checkouts launch by launch, dump a scenario in each and diff the files:

    python -m tests.test_engine_launch_trace --dump wide64-bf16-training trace.json
    python -m tests.test_engine_launch_trace --write-golden        # regenerate tests/golden/engine_launch_trace.json
"""
import ctypes as C
import functools
import hashlib
import json
import os
import sys

import pytest
import torch

from ctrlora_amd import hip
from ctrlora_amd.engine import blocks, nets
from ctrlora_amd.engine.model import CtrLoRAEngine
from ctrlora_amd.engine.packing import Conv3W, LinearW, LoraGroup, NormW, Trainable
from oracle import arch
from tests.test_engine_launch_sequence import Recorder

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_launch_trace.json")
CPU = torch.device("cpu")
BATCH, SIDE, TOKENS, WINDOW = 2, 16, 77, 32
PACKED = (LinearW, LoraGroup, Conv3W, NormW, Trainable)


def wide(rank):
    return arch.ArchCfg(model_channels=320, channel_mult=(1, 2), num_res_blocks=1, attention_resolutions=(1, 2), context_dim=96,
                        lora_rank=rank)


ARCHS = {"tiny": arch.TINY, "wide64": wide(64), "wide32": wide(32)}
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
# id -> (architecture, dtype, passes, nets.GROUP_LORA)
SCENARIOS = {f"{a}-{d}-{p}": (a, d, p, True) for a in ARCHS for d in DTYPES for p in ("inference", "training")}
SCENARIOS.update({f"tiny-{d}-pretraining": ("tiny", d, "pretraining", True) for d in DTYPES})
SCENARIOS.update({f"wide64-bf16-{p}-ungrouped": ("wide64", "bf16", p, False) for p in ("inference", "training")})
assert len(SCENARIOS) == 16


@functools.lru_cache(maxsize=None)
def states(name):
    cfg = ARCHS[name]
    return arch.make_state(arch.controlnet_shapes(cfg), 1), arch.make_state(arch.unet_shapes(cfg), 2)


def netcfg(c):
    return nets.NetCfg(c.in_channels, c.out_channels, c.model_channels, c.channel_mult, c.num_res_blocks,
                       c.attention_resolutions, c.num_heads, c.context_dim)


# --------------------------------------------------------------------------- recording

def record(scenario):
    """Run one scenario against the recording stand-in: (raw calls, {address: field name of the packing object holding it})."""
    a, d, passes, group_lora = SCENARIOS[scenario]
    cfg, dtype = ARCHS[a], DTYPES[d]
    sd_cn, sd_un = states(a)
    alive = []
    real_data_ptr = torch.Tensor.data_ptr

    def data_ptr(self):
        alive.append(self)
        return real_data_ptr(self)

    with pytest.MonkeyPatch.context() as mp:
        rec = Recorder({})
        mp.setattr(hip, "_lib", rec)
        mp.setattr(hip, "stream", lambda: 0)
        for name, value in (("_workspace", None), ("_zero_pages", {}), ("_stream_ws", {}), ("XS_ENABLED", True),
                            ("LN_PROLOGUE", True), ("WGRAD_F32_DETERMINISTIC", False)):
            mp.setattr(hip, name, value)
        for name in ("PRESCALE_Q", "CONV_PHASE", "WGRAD_ROW3"):
            mp.setattr(blocks, name, True)
        mp.setattr(nets, "GROUP_LORA", group_lora)
        mp.setattr(nets, "HOIST_EMB_BWD", True)
        for name in ("CTRLORA_MERGE_LORA", "CTRLORA_BATCH_EMB"):
            mp.delenv(name, raising=False)
        mp.setattr(torch.Tensor, "data_ptr", data_ptr)
        hip.ensure_workspace(CPU)
        train = passes != "inference"
        unet = nets.UNetE(sd_un, netcfg(cfg), dtype, CPU, need_bwd=train)
        cn = nets.ControlNetE(sd_cn, netcfg(cfg), dtype, CPU, need_bwd=train, train_all=passes == "pretraining")
        eng = CtrLoRAEngine.from_executors(unet, [cn])
        eng.overlap_streams = eng.overlap_wgrad = False          # the streams need a GPU
        rec.clear()                                              # (registration and the constructors' re-pack are not the pass)
        g = torch.Generator().manual_seed(3)
        x, hint, d_eps = (torch.randn(BATCH, 4, SIDE, SIDE, generator=g) for _ in range(3))
        context = torch.randn(BATCH, TOKENS, cfg.context_dim, generator=g)
        t = torch.tensor([10, 500])
        eng.forward(x, t, context, [hint], record=train)
        if train:
            eng.backward(d_eps)
    return rec.calls, packed_fields([unet, cn], real_data_ptr)


def packed_fields(roots, data_ptr):
    """{address: field name} over every packing object reachable from the executors, in a fixed walk order.  Where two fields
    share an address (a group and its first member, a trainable norm's gamma and its master) the first one walked names it,
    packed copies before Trainables."""
    found, seen = [], set()

    def walk(o):
        if id(o) in seen or isinstance(o, torch.Tensor):
            return
        seen.add(id(o))
        if isinstance(o, PACKED):
            found.append(o)
        if isinstance(o, dict):
            o = list(o.values())
        if isinstance(o, (list, tuple)):
            for v in o:
                walk(v)
        elif type(o).__module__.startswith("ctrlora_amd") and hasattr(o, "__dict__"):
            walk(vars(o))

    walk(roots)
    names = {}
    for o in sorted(found, key=lambda o: isinstance(o, Trainable)):          # (stable: the walk order within each class)
        for attr, v in vars(o).items():
            items = v.items() if isinstance(v, dict) else enumerate(v) if isinstance(v, (list, tuple)) else None
            if isinstance(v, torch.Tensor):
                names.setdefault(data_ptr(v), attr)
            elif items is not None:
                for k, e in items:
                    if isinstance(e, torch.Tensor):
                        names.setdefault(data_ptr(e), f"{attr}[{k}]")
    return names


# --------------------------------------------------------------------------- canonical form

def canonical(calls, names):
    tokens, counts = {}, {}

    def pointer(v):
        if not v:
            return None
        if v not in tokens:
            field = names.get(v, "p")
            counts[field] = counts.get(field, 0) + 1
            tokens[v] = f"{field}#{counts[field]}"
        return tokens[v]

    def value(ctype, v):
        if ctype is C.c_void_p:
            return pointer(v)
        return C.c_float(v).value if ctype is C.c_float else int(v)

    def struct(cls, d):
        return {f: value(ctype, d[f]) for f, ctype in cls._fields_}

    out = []
    for name, args in calls:
        sig = hip._SIGS[name]
        assert len(sig) == len(args), (name, len(sig), len(args))
        row = []
        for ctype, v in zip(sig, args):
            if isinstance(v, dict):
                row.append(struct(hip.GemmParams, v))
            elif isinstance(v, list):
                row.append([struct(hip.WgradDesc, d) for d in v])
            else:
                row.append(value(ctype, v))
        out.append([name, row])
    return out


def digest(trace):
    blocks_ = [trace[i:i + WINDOW] for i in range(0, len(trace), WINDOW)]
    return {"launches": len(trace),
            "sha256": [hashlib.sha256(json.dumps(b, sort_keys=True).encode()).hexdigest() for b in blocks_]}


def gemms(trace):
    return [row[0] for name, row in trace if name == "cl_gemm"]


# --------------------------------------------------------------------------- the test

@pytest.mark.parametrize("scenario", list(SCENARIOS))
def test_engine_issues_the_recorded_launches(scenario):
    with open(GOLDEN) as f:
        want = json.load(f)[scenario]
    trace = canonical(*record(scenario))
    got = digest(trace)
    # a scenario must not pass while having lost the launch forms it exists for
    g = gemms(trace)
    if scenario in ("wide64-bf16-inference", "wide32-bf16-inference"):
        assert any(p["act"] == hip.ACT_GEGLU_SPLIT and p["ln_gamma"] for p in g), "no x-stationary GEGLU with a LayerNorm prologue"
        assert any(p["act"] == hip.ACT_GEGLU for p in g), "no tile GEGLU"
        assert any(p["act"] == hip.ACT_NONE and p["ln_gamma"] for p in g), "no plain product with a LayerNorm prologue"
        assert not any(p["a2_group_n"] for p in g), "a folded pass has no live LoRA segment to group"
    if scenario in ("wide64-bf16-training", "wide32-bf16-training"):
        assert any(p["a2_group_n"] for p in g), "no grouped LoRA product"
        # u = dy B of a group: one grouped launch at rank 64, one product per member below the narrowest tile
        assert any(p["a1_group_n"] for p in g) == (scenario == "wide64-bf16-training")
    if scenario == "wide64-bf16-training-ungrouped":
        assert not any(p["a1_group_n"] or p["a2_group_n"] for p in g)
    assert got["launches"] == want["launches"], f"{scenario}: {got['launches']} launches, recorded {want['launches']}"
    bad = [i for i, (a, b) in enumerate(zip(got["sha256"], want["sha256"])) if a != b]
    assert not bad, (f"{scenario}: launches {bad[0] * WINDOW} .. {min(bad[0] * WINDOW + WINDOW, got['launches']) - 1} differ from "
                     f"the recorded trace ({len(bad)} of {len(want['sha256'])} windows differ; --dump writes the full trace)")


def main(argv):
    if argv[:1] == ["--dump"] and len(argv) == 3 and argv[1] in SCENARIOS:
        with open(argv[2], "w") as f:
            for row in canonical(*record(argv[1])):
                f.write(json.dumps(row, sort_keys=True) + "\n")
    elif argv == ["--write-golden"]:
        gold = {s: digest(canonical(*record(s))) for s in SCENARIOS}
        with open(GOLDEN, "w") as f:
            json.dump(gold, f, indent=1, sort_keys=True)
            f.write("\n")
    else:
        sys.exit("usage: --dump SCENARIO FILE | --write-golden\nscenarios: " + " ".join(SCENARIOS))


if __name__ == "__main__":
    main(sys.argv[1:])
