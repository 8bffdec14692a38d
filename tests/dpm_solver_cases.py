"""Shared by tests/test_dpm_solver_cpu.py and tests/test_gpu_dpm_solver.py: the fixture of the UNMODIFIED reference's
DPM-Solver++ runs (tests/golden/dpm_solver.pt, written by tests/golden/make_golden_dpm_solver.py), the analytic eps model it
was generated with, and the comparison every fixture case gets."""
import os
from types import SimpleNamespace

import torch

from tests.util import GOLDEN, rel_l2

TOL = 1e-5          # the project's ENC_TOL for a restated sampler against the reference's fp32 trajectory
TIME_TOL = 1.3e-4   # two fp32 ulps at 1000: the reference forms (t - 1/1000) * 1000 in fp32, the table in fp64

_FIXTURE = []


def fixture():
    if not _FIXTURE:
        _FIXTURE.append(torch.load(os.path.join(GOLDEN, "dpm_solver.pt"), weights_only=False))
    return _FIXTURE[0]


def case_names(min_steps=1):
    return [k for k, v in fixture()["cases"].items() if v["S"] >= min_steps]


class AnalyticModel:
    """eps(x, t, c) = tanh(0.7 x + 0.001 t) * c with the sampler-facing attributes of an LDM.  The conditioning is a (B,)
    tensor or a dict {"c_crossattn": [tensor], ...}.  Every Python-level call logs its batch size; every EXECUTION (a graph replay
    included, which does not call Python) appends t[0] to a log held on the tensors' device."""
    num_timesteps = 1000
    parameterization = "eps"

    def __init__(self, device="cpu", with_engine=False):
        self.device = torch.device(device)
        self.alphas_cumprod = fixture()["alphas_cumprod"].clone()
        self.betas = torch.zeros(1, device=self.device)
        self.calls = []
        self.tlog = torch.zeros(256, dtype=torch.float32, device=self.device)
        self.k = torch.zeros(1, dtype=torch.long, device=self.device)
        if with_engine:      # what the sampler asks of an engine around its loop
            eng = SimpleNamespace(cache_context_kv=False, reset_context_cache=lambda: None)
            self.engine = lambda: eng

    def apply_model(self, x, t, c):
        assert t.is_floating_point() and t.shape == (x.shape[0],)
        if isinstance(c, dict):
            c = c["c_crossattn"][0]
        self.calls.append(int(x.shape[0]))
        self.tlog.index_copy_(0, self.k, t[:1].float())
        self.k += 1
        return torch.tanh(0.7 * x + 0.001 * t.float().view(-1, 1, 1, 1)) * c.view(-1, 1, 1, 1)

    def executed_times(self):
        return self.tlog[:int(self.k)].cpu().tolist()


def run_case(name, device="cpu", use_graph=False, conds="tensor", with_engine=False, steps=None):
    """Run fixture case `name` through our sampler.  conds: 'tensor' | 'dict' | 'different' (dicts of different structure).
    steps: another number of steps than the case's (no reference result then).  Returns (result, model, case)."""
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    case = fixture()["cases"][name]
    model = AnalyticModel(device, with_engine)
    s = DPMSolverSampler(model)
    s.order, s.skip_type, s.use_graph = case["order"], case["skip_type"], use_graph
    c, uc = case["c"].to(device), case["uc"].to(device)
    if conds != "tensor":
        c, uc = {"c_crossattn": [c]}, {"c_crossattn": [uc]}
        if conds == "different":
            uc["extra"] = [uc["c_crossattn"][0]]
    x_T = case["x_T"].to(device)
    out, aux = s.sample(case["S"] if steps is None else steps, x_T.shape[0], tuple(x_T.shape[1:]), c, verbose=False, x_T=x_T,
                        unconditional_guidance_scale=case["scale"], unconditional_conditioning=uc)
    assert aux is None and out.shape == x_T.shape and out.dtype == torch.float32
    return out, model, case


def check_case(out, model, case, passes=1):
    """Result, model times and batch sizes against the reference's record.  passes = 2: guidance as two passes of B."""
    S, B = case["S"], case["x_T"].shape[0]
    times = model.executed_times()
    assert len(times) == S * passes
    times = times[::passes]
    want_b = B if (passes == 2 or case["scale"] == 1.0) else 2 * B
    assert model.calls and all(b == want_b for b in model.calls)
    if passes == 1:
        assert want_b == case["batch_sizes"][0]
    if case["result"] is None:
        # the reference raised part-way (order 3 with fewer than 15 steps, see the generator): the calls it made first
        # still pin the time grid; the result can only be checked for being a finite sample
        assert case["reference_error"].startswith("ValueError") and 0 < len(case["times"]) < S
        times = times[:len(case["times"])]
        assert bool(torch.isfinite(out).all())
    else:
        assert len(case["times"]) == S and case["batch_sizes"] == [case["batch_sizes"][0]] * S
        err = rel_l2(out, case["result"])
        print(f"rel_l2 {err:.3e}")
        assert err < TOL, err
    worst = max(abs(a - b) for a, b in zip(times, case["times"]))
    print(f"max |t - t_ref| {worst:.3e}")
    assert worst < TIME_TOL, worst
