"""Shared by tests/test_plms_cpu.py and tests/test_gpu_plms.py: the fixture of the UNMODIFIED reference's PLMS runs
(tests/golden/plms.pt, written by tests/golden/make_golden_plms.py), the analytic eps model it was generated with (LONG
timesteps, a q_sample with the fixture's fixed noise), the comparison every fixture case gets, and the restatement of
cl_plms_step's arithmetic with its element-wise gate."""
import os
from types import SimpleNamespace

import numpy as np
import torch

from tests.util import GOLDEN, rel_l2

TOL = 1e-5          # the project's ENC_TOL for a restated sampler against the reference's fp32 trajectory

_FIXTURE = []


def fixture():
    if not _FIXTURE:
        _FIXTURE.append(torch.load(os.path.join(GOLDEN, "plms.pt"), weights_only=False))
    return _FIXTURE[0]


def case_names(min_steps=1, max_steps=10 ** 9, masked=False):
    return [k for k, v in fixture()["cases"].items() if min_steps <= v["S"] <= max_steps and ("mask" in v) == masked]


class AnalyticModel:
    """eps(x, t, c) = tanh(0.7 x + 0.001 t) * c with the sampler-facing attributes of an LDM; t is a LONG tensor.  The
    conditioning is a (B,) tensor or a dict {"c_crossattn": [tensor], ...}.  Every Python-level call logs its batch size; every
    EXECUTION (a graph replay included, which does not call Python) appends t[0] to a log held on the tensors' device."""
    num_timesteps = 1000
    parameterization = "eps"

    def __init__(self, device="cpu", with_engine=False, q_noise=None):
        self.device = torch.device(device)
        self.alphas_cumprod = fixture()["alphas_cumprod"].clone()
        self.alphas_cumprod_prev = torch.cat([torch.ones(1), self.alphas_cumprod[:-1]])
        self.betas = torch.zeros(1, device=self.device)
        self.q_noise = None if q_noise is None else q_noise.to(self.device)
        self.calls = []
        self.tlog = torch.zeros(256, dtype=torch.long, device=self.device)
        self.k = torch.zeros(1, dtype=torch.long, device=self.device)
        if with_engine:      # what the sampler asks of an engine around its loop
            eng = SimpleNamespace(cache_context_kv=False, reset_context_cache=lambda: None)
            self.engine = lambda: eng

    def apply_model(self, x, t, c):
        assert t.dtype == torch.long and t.shape == (x.shape[0],)
        if isinstance(c, dict):
            c = c["c_crossattn"][0]
        self.calls.append(int(x.shape[0]))
        self.tlog.index_copy_(0, self.k, t[:1])
        self.k += 1
        return torch.tanh(0.7 * x + 0.001 * t.float().view(-1, 1, 1, 1)) * c.view(-1, 1, 1, 1)

    def q_sample(self, x_start, t):
        ac = self.alphas_cumprod.to(x_start.device)
        return ac.sqrt()[t].view(-1, 1, 1, 1) * x_start + (1. - ac).sqrt()[t].view(-1, 1, 1, 1) * self.q_noise

    def executed_times(self):
        return self.tlog[:int(self.k)].cpu().tolist()


def run_case(name, device="cpu", use_graph=False, conds="tensor", with_engine=False):
    """Run fixture case `name` through our sampler.  conds: 'tensor' | 'dict' | 'different' (dicts of different structure).
    Returns (result, intermediates, model, case)."""
    from ldm.models.diffusion.plms import PLMSSampler
    case = fixture()["cases"][name]
    model = AnalyticModel(device, with_engine, case.get("q_noise"))
    s = PLMSSampler(model)
    s.use_graph = use_graph
    c, uc = case["c"].to(device), case["uc"].to(device)
    if conds != "tensor":
        c, uc = {"c_crossattn": [c]}, {"c_crossattn": [uc]}
        if conds == "different":
            uc["extra"] = [uc["c_crossattn"][0]]
    x_T = case["x_T"].to(device)
    masked = {k: case[k].to(device) for k in ("mask", "x0") if k in case}
    out, inter = s.sample(case["S"], x_T.shape[0], tuple(x_T.shape[1:]), c, verbose=False, x_T=x_T,
                          log_every_t=case["log_every_t"], unconditional_guidance_scale=case["scale"],
                          unconditional_conditioning=uc, **masked)
    assert out.shape == x_T.shape and out.dtype == torch.float32
    return out, inter, model, case


def check_case(out, inter, model, case, passes=1, python_calls=None):
    """Result, intermediates, model times and batch sizes against the reference's record.  passes = 2: guidance as two passes
    of B.  python_calls: how many of the S + 1 evaluations called Python (all of them unless a captured step replays)."""
    S, B = case["S"], case["x_T"].shape[0]
    assert len(case["times"]) == S + 1
    times = model.executed_times()
    assert len(times) == (S + 1) * passes
    assert times[::passes] == case["times"] and times[passes - 1::passes] == case["times"]       # integers: exactly
    n_py = (S + 1 if python_calls is None else python_calls) * passes
    if passes == 1:
        assert model.calls == case["batch_sizes"][:n_py], model.calls       # 2B under guidance, B without
    else:
        assert case["scale"] != 1.0 and model.calls == [B] * n_py, model.calls
    err = rel_l2(out, case["result"])
    print(f"rel_l2 {err:.3e}")
    assert err < TOL, err
    for key in ("x_inter", "pred_x0"):
        assert len(inter[key]) == len(case[key]), (key, len(inter[key]), len(case[key]))
        worst = max(rel_l2(a, b) for a, b in zip(inter[key], case[key]))
        print(f"{key}: {len(inter[key])} entries, worst rel_l2 {worst:.3e}")
        assert worst < TOL, (key, worst)


# ------------------------------------------------------------------------------------------------ cl_plms_step's arithmetic

MULTISTEP, START, FINISH = 0, 1, 2
AB = {1: ((3., -1.), 2.), 2: ((23., -16., 5.), 12.), 3: ((55., -59., 37., -9.), 24.)}     # Adams-Bashforth 2, 3, 4
E = 2.0 ** -24
ROUNDINGS = 16


def plms_step_ref(x, e_c, e_u, row, scale, phase, olds, dtype=torch.float64, weights=None):
    """The contract of cl_plms_step (include/ctrlora_hip.h) on one fp32 table row {a_t, a_prev, sigma_t, sqrt(1 - a_t)} and fp32
    operands, evaluated in `dtype`: fp64 is the reference, fp32 the rounding model (every operation of the formula rounded
    once, no contraction).  olds: MULTISTEP [o1, o2, o3][:order]; FINISH [hist[0]]; START [].  Returns e (what the history
    slot receives), x_out, pred_x0 and, for each, mag = the sum of the absolute values of the terms of its formula with the
    mags of its operands propagated (tests/ew_ref.py).  weights: another AB table (negative control)."""
    c = lambda v: v.detach().cpu().to(dtype)
    a_t, a_prev, sigma, s1m = (torch.tensor(float(v), dtype=dtype) for v in row)
    x, e_c = c(x), c(e_c)
    if e_u is None:
        e, mag_e = e_c, e_c.abs()
    else:
        u, s = c(e_u), torch.tensor(float(np.float32(scale)), dtype=dtype)
        e = u + s * (e_c - u)
        mag_e = u.abs() + s.abs() * (e_c.abs() + u.abs())
    olds = [c(o) for o in olds]
    if phase == FINISH:
        ep, mag_ep = (olds[0] + e) / 2, (olds[0].abs() + mag_e) / 2
    elif phase == START:
        ep, mag_ep = e, mag_e
    else:
        w, d = (weights or AB)[len(olds)]
        ep, mag_ep = w[0] * e, abs(w[0]) * mag_e
        for wj, o in zip(w[1:], olds):
            ep, mag_ep = ep + wj * o, mag_ep + abs(wj) * o.abs()
        ep, mag_ep = ep / d, mag_ep / d
    sqrt_at, sqrt_ap, dirc = a_t.sqrt(), a_prev.sqrt(), (1. - a_prev - sigma * sigma).sqrt()
    pred_x0, mag_p = (x - s1m * ep) / sqrt_at, (x.abs() + s1m * mag_ep) / sqrt_at
    x_out, mag_x = sqrt_ap * pred_x0 + dirc * ep, sqrt_ap * mag_p + dirc * mag_ep
    return dict(e=e, x_out=x_out, pred_x0=pred_x0, mag=dict(e=mag_e.double(), x_out=mag_x.double(), pred_x0=mag_p.double()))


def violations(got, ref, key):
    """Elements of output `key` outside |got - ref| <= ROUNDINGS * 2^-24 * mag, and the largest ratio to that bound."""
    err = (got.detach().cpu().double().reshape(-1) - ref[key].double().reshape(-1)).abs()
    bound = ROUNDINGS * E * ref["mag"][key].reshape(-1)
    return int((err > bound).sum()), float((err / bound.clamp_min(1e-300)).max())


def plms_refusals(L, p, q):
    """Every refusal of cl_plms_step / cl_plms_step_dev as {label: return code}; p, q: two distinct valid addresses (never
    read: a refusal is decided on the host before anything is launched)."""
    N = None
    step = lambda x=p, e_c=p, coef=p, it=1, S=4, phase=0, hist=p, x_out=q, n=8: L.cl_plms_step(
        x, e_c, N, coef, it, S, phase, 7.5, hist, x_out, N, n, N)
    dev = lambda x=p, e_c=p, coef=p, cursor=p, S=4, hist=p, x_out=q, n=8: L.cl_plms_step_dev(
        x, e_c, N, coef, cursor, S, 7.5, hist, x_out, N, n, N)
    return {
        "S<1": step(it=0, S=0, phase=1), "iter<0": step(it=-1), "iter==S": step(it=4), "phase<0": step(phase=-1),
        "phase>2": step(phase=3), "start iter!=0": step(it=1, phase=1), "finish iter!=0": step(it=2, phase=2),
        "multistep iter==0": step(it=0, phase=0), "null x": step(x=N), "null e_c": step(e_c=N), "null coef": step(coef=N),
        "null hist": step(hist=N), "null x_out": step(x_out=N), "n<0": step(n=-1), "start x_out==x": step(it=0, phase=1, x_out=p),
        "dev S<2": dev(S=1), "dev null x": dev(x=N), "dev null e_c": dev(e_c=N), "dev null coef": dev(coef=N),
        "dev null cursor": dev(cursor=N), "dev null hist": dev(hist=N), "dev null x_out": dev(x_out=N), "dev n<0": dev(n=-1),
    }
