"""Every launch a whole forward of the two CLIP executors issues (ctrlora_amd/engine/vit.py: ClipVisionE,
ctrlora_amd/engine/clip_text.py: ClipTextE), argument for argument, against a recorded trace -- on the CPU, with the recording
stand-in of tests/test_engine_launch_sequence.py in place of libctrlora_hip.so (no kernel runs), the way
tests/test_engine_launch_trace.py records the UNet.

Both towers walk the same pre-LN layer over different buffers: the vision side rotates hA / hB / hC in the engine dtype (hA
keeps the penultimate state), the fp32 text side rotates h[0] / h[1] / hid with h[2] in the middle, the bf16 text side adds onto
one fp32 stream in place.  A product that writes hB where it should write hC has the right shape and the wrong numbers, so
tests/golden/clip_launch_trace.json holds, per scenario, the entry point and a sha256 of every launch of the CANONICAL trace:

  * every call is (entry point, arguments); GemmParams is decoded field by field, float arguments are rounded through c_float;
  * while a scenario runs, every tensor whose address is taken is kept alive, so no address is ever reused;
  * a pointer into a tensor of the executor's packed weights becomes "w.<key>" / "w.layers[<i>].<key>", a pointer into one of
    its buffers "buf.<key>" / "buf.<key>[<i>]" (with "+<bytes>" behind it where it points past the tensor's start: the k and v
    columns of qkv); any other pointer becomes "p#<n>" in order of first appearance; null stays null.

pooler_output and text_embeds are not recorded: hip.gather_rows asks for a row index on the GPU.  The golden file is a recording
of the executors, not a derivation: it changes only with a pull request that means to change what is launched.

    python -m tests.test_clip_launch_trace --dump text-quick_gelu-bf16-N77-last trace.json
    python -m tests.test_clip_launch_trace --write-golden [FILE]      # default: tests/golden/clip_launch_trace.json
"""
import collections
import ctypes as C
import functools
import hashlib
import json
import os
import sys

import pytest
import torch

from ctrlora_amd import hip
from ctrlora_amd.engine import blocks
from ctrlora_amd.engine.clip_text import ClipTextE
from ctrlora_amd.engine.vit import ClipVisionE
from tests.test_clip_text_cpu import TINY as TEXT_TINY, hf_text_model, make_ids
from tests.test_clip_vision_cpu import TINY as VISION_TINY, hf_model
from tests.test_engine_launch_sequence import Recorder

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_launch_trace.json")
CPU = torch.device("cpu")
BATCH = 2
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
WANTS = {"last": (("last_hidden_state",), None), "hid0": (("hidden_state",), 0), "hid1": (("hidden_state",), 1),
         "hid-1": (("hidden_state",), -1), "last+hid1": (("last_hidden_state", "hidden_state"), 1)}

# id -> ("vision", dtype, num_hidden_layers, output_hidden_states) | ("text", hidden_act, dtype, N, want)
SCENARIOS = {f"vision-{d}-L{L}-{'hidden' if ohs else 'embeds'}": ("vision", d, L, ohs)
             for d in DTYPES for L in (2, 1) for ohs in (False, True)}
SCENARIOS.update({f"text-{act}-{d}-N{N}-{w}": ("text", act, d, N, w)
                  for act in ("quick_gelu", "gelu") for d in DTYPES for N in (7, 77) for w in WANTS})
assert len(SCENARIOS) == 8 + 40


@functools.lru_cache(maxsize=None)
def vision_state(L):
    return hf_model(dict(VISION_TINY, num_hidden_layers=L)).state_dict()


# --------------------------------------------------------------------------- recording

def record(scenario):
    """Run one scenario against the recording stand-in: (raw calls, [(first byte, bytes, name)] of the executor's tensors)."""
    s = SCENARIOS[scenario]
    alive = []
    real_data_ptr = torch.Tensor.data_ptr

    def data_ptr(self):
        alive.append(self)
        return real_data_ptr(self)

    with pytest.MonkeyPatch.context() as mp:
        rec = Recorder({})
        mp.setattr(hip, "_lib", rec)
        mp.setattr(hip, "stream", lambda: 0)
        for name, value in (("_workspace", None), ("_zero_pages", {}), ("_stream_ws", {})):
            mp.setattr(hip, name, value)
        mp.setattr(blocks, "PRESCALE_Q", True)
        mp.setattr(torch.Tensor, "data_ptr", data_ptr)
        hip.ensure_workspace(CPU)
        if s[0] == "vision":
            _, d, L, ohs = s
            cfg = dict(VISION_TINY, num_hidden_layers=L)
            ex = ClipVisionE(vision_state(L), cfg, DTYPES[d], CPU)
            px = torch.randn(BATCH, cfg["num_channels"], cfg["image_size"], cfg["image_size"], generator=torch.Generator().manual_seed(1))
            rec.clear()
            out = ex.forward(px, output_hidden_states=ohs)
            assert isinstance(out, tuple) == ohs
        else:
            _, act, d, N, w = s
            cfg = dict(TEXT_TINY, hidden_act=act)
            ex = ClipTextE(hf_text_model(cfg).state_dict(), cfg, DTYPES[d], CPU)
            want, hidden_idx = WANTS[w]
            rec.clear()
            out = ex.forward(make_ids(cfg, BATCH, N), want=want, hidden_idx=hidden_idx)
            assert tuple(out) == want and ex.forwards == 1
        (buffers,) = ex._buf.values()           # one batch size ran
    return rec.calls, ranges(ex.w, buffers, real_data_ptr)


def ranges(w, buffers, data_ptr):
    out = []

    def add(name, t):
        if isinstance(t, torch.Tensor):
            assert t.is_contiguous(), name
            out.append((data_ptr(t), t.numel() * t.element_size(), name))

    for k, t in w.items():
        if k == "layers":
            for i, lay in enumerate(t):
                for kk, tt in lay.items():
                    add(f"w.layers[{i}].{kk}", tt)
        else:
            add(f"w.{k}", t)
    for k, t in buffers.items():
        if isinstance(t, (list, tuple)):
            for i, tt in enumerate(t):
                add(f"buf.{k}[{i}]", tt)
        else:
            add(f"buf.{k}", t)
    return out


# --------------------------------------------------------------------------- canonical form

def canonical(calls, named):
    tokens = {}

    def pointer(v):
        if not v:
            return None
        for start, size, name in named:
            if start <= v < start + size:
                return name if v == start else f"{name}+{v - start}"
        if v not in tokens:
            tokens[v] = f"p#{len(tokens) + 1}"
        return tokens[v]

    def value(ctype, v):
        if ctype is C.c_void_p:
            return pointer(v)
        return C.c_float(v).value if ctype is C.c_float else int(v)

    out = []
    for name, args in calls:
        sig = hip._SIGS[name]
        assert len(sig) == len(args), (name, len(sig), len(args))
        row = []
        for ctype, v in zip(sig, args):
            if isinstance(v, dict):
                row.append({f: value(ct, v[f]) for f, ct in hip.GemmParams._fields_})
            else:
                row.append(value(ctype, v))
        out.append([name, row])
    return out


def digest(trace):
    return {"launches": [name for name, _ in trace],
            "sha256": [hashlib.sha256(json.dumps(row, sort_keys=True).encode()).hexdigest() for row in trace]}


# --------------------------------------------------------------------------- the test

@pytest.mark.parametrize("scenario", list(SCENARIOS))
def test_executor_issues_the_recorded_launches(scenario):
    with open(GOLDEN) as f:
        want = json.load(f)[scenario]
    trace = canonical(*record(scenario))
    got = digest(trace)
    # a scenario must not pass while having lost the forms it exists for
    g = [row[0] for name, row in trace if name == "cl_gemm"]
    if scenario.startswith("vision-bf16"):
        assert any(p["alpha_n"] == VISION_TINY["hidden_size"] and p["alpha"] != 1.0 for p in g), "no pre-scaled q columns"
    if scenario.startswith("vision"):
        assert {p["C"] for p in g} >= {"buf.h[1]", "buf.h[2]", "buf.embeds"}, "the rotation's buffers are not told apart"
    if scenario.startswith("text") and "-bf16-" in scenario and not scenario.endswith("hid0"):
        assert any(p["atomic"] and p["C"] == "buf.h[0]" and not p["residual"] for p in g), "no in-place add onto the fp32 stream"
    if scenario.startswith("text") and "-fp32-" in scenario and not scenario.endswith("hid0"):
        assert any(p["residual"] == "buf.h[2]" and p["beta"] == 1.0 for p in g) and not any(p["atomic"] for p in g)
    if scenario == "text-quick_gelu-bf16-N77-last":
        assert collections.Counter(got["launches"]) == dict(cl_gemm=8, cl_layernorm_fwd=5, cl_pack2d=4, cl_attention_causal_fwd=2,
                                                            cl_clip_text_embed=1)
    assert got["launches"] == want["launches"], f"{scenario}: launches {got['launches']}, recorded {want['launches']}"
    bad = [i for i, (a, b) in enumerate(zip(got["sha256"], want["sha256"])) if a != b]
    assert not bad, (f"{scenario}: launches {bad} differ from the recorded trace (first: {trace[bad[0]]}; --dump writes the "
                     f"full trace)")


def main(argv):
    if argv[:1] == ["--dump"] and len(argv) == 3 and argv[1] in SCENARIOS:
        with open(argv[2], "w") as f:
            for row in canonical(*record(argv[1])):
                f.write(json.dumps(row, sort_keys=True) + "\n")
    elif argv[:1] == ["--write-golden"] and len(argv) <= 2:
        gold = {s: digest(canonical(*record(s))) for s in SCENARIOS}
        with open(argv[1] if len(argv) == 2 else GOLDEN, "w") as f:
            json.dump(gold, f, indent=1, sort_keys=True)
            f.write("\n")
    else:
        sys.exit("usage: --dump SCENARIO FILE | --write-golden [FILE]\nscenarios: " + " ".join(SCENARIOS))


if __name__ == "__main__":
    main(sys.argv[1:])
