"""Shared pieces of the norm_trainable / zero_trainable tests (test_flags_cpu.py, test_gpu_flags.py)."""
import os

import torch

from tests.util import GOLDEN

# (norm_trainable, zero_trainable): the three combinations tests/golden/flags_tiny.pt records
COMBOS = [(False, True), (True, False), (False, False)]


def combo_key(nt, zt):
    return f"norm{int(nt)}_zero{int(zt)}"


def load_flags_golden():
    return torch.load(os.path.join(GOLDEN, "flags_tiny.pt"), weights_only=False)


def sample_idx(numel, n):
    """Index rule of the fixture's grad_vals (tests/golden/make_golden_flags.py)."""
    return torch.linspace(0, numel - 1, min(n, numel)).long()


def netcfg(c):
    from ctrlora_amd.engine import NetCfg
    return NetCfg(c.in_channels, c.out_channels, c.model_channels, c.channel_mult, c.num_res_blocks,
                  c.attention_resolutions, c.num_heads, c.context_dim)


def selected(name, nt, zt):
    """The reference's filter for ft_with_lora=True (cldm_ctrlora_finetune.py:90-100), restated on a parameter name."""
    if "lora_layer" in name:
        return True
    if "zero_convs" in name or "middle_block_out" in name:
        return zt
    return "norm" in name and nt


def digest_close(t, d, tol):
    """The gate tests/test_oracle_golden.py puts on model_tiny's digests."""
    f = t.detach().float().flatten().cpu()
    assert list(t.shape) == d["shape"]
    vals = f[torch.tensor(d["idx"])]
    scale = max(d["l2"] / max(1, f.numel()) ** 0.5, 1e-12)
    assert abs(float(f.double().norm()) - d["l2"]) <= tol * max(d["l2"], 1e-12) * 10
    assert float((vals - torch.tensor(d["vals"])).abs().max()) <= tol * 50 * scale + 1e-9


def flag_mutator(nt, zt):
    """bench.build_model(mutate=...): the two flags as ordinary control_stage_config params, as a YAML would set them."""
    def mutate(p):
        p["control_stage_config"]["params"].update(norm_trainable=nt, zero_trainable=zt)
    return mutate
