"""tests/loss_ref.py checked on the CPU: the fp64 contract against torch's own losses and autograd, the rounding model inside its
bounds on every case, every mutation of the model outside them, the Min-SNR table against the closed form, and the refusals of
cl_p_losses_w, which return before any launch."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ew_ref as R
from tests import loss_ref as LR


def _model_as_got(p, ops, mutate=None):
    return LR.model_plosses_w(p, ops, mutate)


def test_contract_matches_torch_losses_and_autograd():
    for name in ("plosses_w-3x4099-huber-wt", "plosses_w-8x256-l2-wt", "plosses_w-3x15-huber-nowt"):
        p = LR.CASE[name]
        ops = LR.make_ops(p)
        e = ops["eps"].double().requires_grad_(True)
        tgt = ops["target"].double()
        per = (F.huber_loss(e, tgt, reduction="none", delta=p["delta"]) if p["kind"] else F.mse_loss(e, tgt, reduction="none")).mean(1)
        w = ops["wt"].double()[ops["t"]] if p["wt"] else torch.ones_like(per)
        weighted = (w * per).mean()
        (p["gscale"] * p["w_simple"] * weighted).backward()
        ref = LR.ref_plosses_w(dict(p, lvlb=True), ops)
        lv = (ops["lvlb"].double()[ops["t"]] * per).mean()
        want = torch.stack([per.mean(), lv, p["w_simple"] * weighted + p["w_elbo"] * lv]).detach()
        assert float((ref["out"] - want).abs().max()) < 1e-14
        assert float((ref["per_sample"] - per.detach()).abs().max()) < 1e-14
        assert float((ref["d_eps"] - e.grad).abs().max()) <= 1e-14 * float(e.grad.abs().max())


@pytest.mark.parametrize("p", LR.CASES, ids=[c["name"] for c in LR.CASES])
def test_rounding_model_passes_its_own_gates(p):
    ops = LR.make_ops(p)
    specs = LR.eval_plosses_w(dict(p, d_eps=True, per_sample=True), ops)
    res = R.check(specs, {k: s["model"] for k, s in specs.items()})
    assert set(res) == {"out", "per_sample", "d_eps"} and not R.failures(res), R.failures(res)


def test_case_table_covers_what_it_claims():
    assert len(LR.CASES) == 60 and {(c["B"], c["per"]) for c in LR.CASES} == set(LR.SHAPES)
    for kind in (0, 1):
        for wt in (False, True):
            rows = [c for c in LR.CASES if c["kind"] == kind and c["wt"] == wt]
            assert {(c["d_eps"], c["lvlb"], c["per_sample"]) for c in rows} == {(a, b, c) for a in (False, True) for b in (False, True)
                                                                              for c in (False, True)}
    assert all(c["gscale"] != 1.0 for c in LR.CASES)
    ts = [LR.case_t(c) for c in LR.CASES]
    assert any(0 in t.tolist() and LR.T - 1 in t.tolist() and len(set(t.tolist())) < len(t) for t in ts)
    assert {int(t[0]) for c, t in zip(LR.CASES, ts) if c["B"] == 1} == {0, LR.T - 1}
    for c in LR.CASES:
        ops = LR.make_ops(c)
        a = (ops["eps"] - ops["target"]).abs()
        if c["per"] >= 256:
            assert min(LR.huber_shares(c, ops)) >= 0.25, (c["name"], LR.huber_shares(c, ops))
        elif c["per"] >= 4:
            assert all(bool((a[b] == 1.0).any() and (a[b] < 1.0).any() and (a[b] > 1.0).any()) for b in range(c["B"])), c["name"]
    small = torch.cat([(LR.make_ops(c)["eps"] - LR.make_ops(c)["target"])[:, 0] for c in LR.CASES if c["per"] == 1 and c["kind"] == 1])
    assert bool((small.abs() == 1.0).any() and (small.abs() < 1.0).any() and (small.abs() > 1.0).any())


MUTANT_CASES = {
    "drop_weight": ["plosses_w-3x4099-l2-wt", "plosses_w-8x16-huber-wt", "plosses_w-1x256-l2-wt"],
    "weight_on_out0": ["plosses_w-3x4099-l2-wt", "plosses_w-8x15-huber-wt"],
    "huber_no_half_delta": ["plosses_w-3x4099-huber-nowt", "plosses_w-8x16-huber-wt", "plosses_w-1x256-huber-wt"],
    "no_clamp": ["plosses_w-3x4099-huber-nowt", "plosses_w-8x16-huber-wt", "plosses_w-3x256-huber-wt"],
    "no_inv_B": ["plosses_w-3x4099-l2-wt", "plosses_w-8x16-huber-nowt", "plosses_w-3x1-l2-nowt"],
}
MUTANT_HITS = {"drop_weight": {"out", "d_eps"}, "weight_on_out0": {"out"}, "huber_no_half_delta": {"out", "per_sample"},
               "no_clamp": {"d_eps"}, "no_inv_B": {"d_eps"}}


@pytest.mark.parametrize("mutate", LR.MUTATIONS)
def test_every_mutation_violates_the_bound(mutate):
    assert set(MUTANT_CASES) == set(LR.MUTATIONS)
    for name in MUTANT_CASES[mutate]:
        p = dict(LR.CASE[name], d_eps=True, per_sample=True)
        ops = LR.make_ops(p)
        specs = LR.eval_plosses_w(p, ops)
        bad = {f[0] for f in R.failures(R.check(specs, _model_as_got(p, ops, mutate)))}
        assert bad == MUTANT_HITS[mutate], (mutate, name, bad)


def _sd15_acp64():
    from ldm.modules.diffusionmodules.util import make_beta_schedule
    betas = make_beta_schedule("linear", 1000, linear_start=0.00085, linear_end=0.0120, cosine_s=8e-3)
    assert betas.dtype == np.float64
    return np.cumprod(1.0 - betas, axis=0)


def test_min_snr_table_matches_the_closed_form_on_the_models_schedule():
    import bench
    acp = _sd15_acp64()
    snr = acp / (1.0 - acp)
    for gamma in (1.0, 5.0, 20.0):
        m = bench.build_model("ctrlora_finetune_sd15_rank128.yaml", 0, tiny=True, mutate=lambda p: p.update(min_snr_gamma=gamma))
        assert m.num_timesteps == 1000 and torch.equal(m.alphas_cumprod, torch.tensor(acp, dtype=torch.float32)), "the SD1.5 schedule"
        w = m.loss_weights
        assert w.dtype == torch.float32 and w.shape == (1000,)
        want = LR.min_snr_ref(acp, gamma)
        assert torch.equal(w, want.float()), "fp64 closed form, rounded once"
        assert float((w.double() - want).abs().max()) <= 2.0 ** -24
        if gamma == 5.0:
            assert int((w == 1.0).sum()) > 0 and int((w < 1.0).sum()) > 0 and float(w.min()) > 0.0
            assert int((w == 1.0).sum()) == int((snr <= 5.0).sum())
    for gamma in (float(snr.max()), 2.0 * float(snr.max()), 1e30):
        m = bench.build_model("ctrlora_finetune_sd15_rank128.yaml", 0, tiny=True, mutate=lambda p: p.update(min_snr_gamma=gamma))
        assert torch.equal(m.loss_weights, torch.ones(1000)), "gamma at or above the largest SNR: exact ones"


def test_refusals_are_decided_on_the_host():
    """Every refusal of cl_p_losses_w returns CL_EINVAL before anything touches a GPU: the pointers are never read, and the launch
    record stays empty."""
    from ctrlora_amd import build, hip
    build.build(verbose=False)
    L = hip.lib()
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 15) & ~15
    N = None
    w = lambda *a: L.cl_p_losses_w(*a)
    # (eps, target, d_eps, t, lvlb, out, per_sample, scratch, B, per, gscale, w_simple, w_elbo, wt, kind, delta, stream)
    calls = {
        # the refusals of cl_p_losses_mse
        "null eps": w(N, p, N, N, N, p, N, p, 1, 1, 1.0, 1.0, 0.0, N, 0, 1.0, N),
        "null target": w(p, N, N, N, N, p, N, p, 1, 1, 1.0, 1.0, 0.0, N, 0, 1.0, N),
        "null out": w(p, p, N, N, N, N, N, p, 1, 1, 1.0, 1.0, 0.0, N, 0, 1.0, N),
        "null scratch": w(p, p, N, N, N, p, N, N, 1, 1, 1.0, 1.0, 0.0, N, 0, 1.0, N),
        "B=0": w(p, p, N, N, N, p, N, p, 0, 1, 1.0, 1.0, 0.0, N, 0, 1.0, N),
        "B=65536": w(p, p, N, N, N, p, N, p, 65536, 1, 1.0, 1.0, 0.0, N, 0, 1.0, N),
        "per=0": w(p, p, N, N, N, p, N, p, 1, 0, 1.0, 1.0, 0.0, N, 0, 1.0, N),
        "lvlb without t": w(p, p, N, N, p, p, N, p, 1, 1, 1.0, 1.0, 0.0, N, 0, 1.0, N),
        # its own
        "wt without t": w(p, p, N, N, N, p, N, p, 1, 1, 1.0, 1.0, 0.0, p, 0, 1.0, N),
        "kind=2": w(p, p, N, p, N, p, N, p, 1, 1, 1.0, 1.0, 0.0, N, 2, 1.0, N),
        "kind=-1": w(p, p, N, p, N, p, N, p, 1, 1, 1.0, 1.0, 0.0, N, -1, 1.0, N),
        "huber delta=0": w(p, p, N, p, N, p, N, p, 1, 1, 1.0, 1.0, 0.0, N, 1, 0.0, N),
        "huber delta<0": w(p, p, N, p, N, p, N, p, 1, 1, 1.0, 1.0, 0.0, N, 1, -1.0, N),
        "huber delta=inf": w(p, p, N, p, N, p, N, p, 1, 1, 1.0, 1.0, 0.0, N, 1, math.inf, N),
        "huber delta=nan": w(p, p, N, p, N, p, N, p, 1, 1, 1.0, 1.0, 0.0, N, 1, math.nan, N),
    }
    wrong = {k: v for k, v in calls.items() if v != 1}
    assert not wrong, wrong
    out = (ctypes.c_int * 8)(*([7] * 8))
    assert L.cl_debug_ew_last_launch(out) == 0 and list(out) == [0] * 8
