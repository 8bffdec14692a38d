"""Shared by tests/test_ddim_edit_cpu.py and tests/test_gpu_ddim_edit.py (helpers only: nothing here is collected): the
contract of cl_qsample_blend in fp64 with its element-wise gate, its fp32 rounding model and two negative controls, the fixture
of the UNMODIFIED reference's masked DDIM runs (tests/golden/ddim_edit.pt, written by tests/golden/make_golden_ddim_edit.py),
the analytic eps model it was generated with, and the comparison every fixture case gets.

Contract (include/ctrlora_hip.h), on the operands AS STORED:
    out[b, c, p] = (sqrt_ac[t_b] x0 + sqrt_1mac[t_b] noise) m + (1 - m) x,   m = mask[(per_b ? b : 0), (per_c ? c : 0), p],
    t_b clamped to [0, T - 1].
Gate, element-wise with zero violations:  |got - ref| <= 6 * 2^-24 * mag.  mag = the sum of the absolute values of the terms of
the formula with the mags of its operands propagated (tests/ew_ref.py): (|sa x0| + |s1 noise|) |m| + (1 + |m|) |x|.  6 = the
fp32 roundings of the contract: two products and a sum (q), the product q m, the difference 1 - m, the product with x; the
closing sum is the sixth on either path (each element passes through at most five before it).  Derived, not measured.
"""
import os
from types import SimpleNamespace

import torch

from tests.util import GOLDEN, rel_l2

E = 2.0 ** -24
ROUNDINGS = 6
TOL = 1e-5          # the project's ENC_TOL for a restated sampler against the reference's fp32 trajectory
LAYOUTS = ((True, True), (True, False), (False, True), (False, False))       # (mask per sample, mask per channel)


def mask_shape(B, C, hw, per_b, per_c):
    return (B if per_b else 1, C if per_c else 1) + tuple(hw)


def _coef(tab, t, dtype, nd):
    T = tab.numel()
    return tab.detach().cpu().to(dtype)[t.detach().cpu().clamp(0, T - 1)].view(-1, *([1] * (nd - 1)))


def blend_ref(x0, noise, t, sqrt_ac, sqrt_1mac, mask, x):
    """(ref, mag) of the contract in fp64; the operands are fp32 tensors of [B, C, ...] (mask broadcastable), t long [B]."""
    c = lambda v: v.detach().cpu().double()
    sa, s1 = _coef(sqrt_ac, t, torch.float64, x0.dim()), _coef(sqrt_1mac, t, torch.float64, x0.dim())
    x0, noise, m, x = c(x0), c(noise), c(mask), c(x)
    ref = (sa * x0 + s1 * noise) * m + (1.0 - m) * x
    mag = ((sa * x0).abs() + (s1 * noise).abs()) * m.abs() + (1.0 + m.abs()) * x.abs()
    return ref, mag


def blend_model32(x0, noise, t, sqrt_ac, sqrt_1mac, mask, x, control=None):
    """The fp32 rounding model, every op of the formula rounded once: q = rn(rn(sa x0) + rn(s1 n)), out = rn(rn(q m) +
    rn(rn(1 - m) x)).  control (negative controls): 'fma' contracts sa x0 + rn(s1 n) into one rounding; 'one_minus' does not
    round 1 - m before the product with x."""
    f = lambda v: v.detach().cpu().float()
    sa, s1 = _coef(sqrt_ac, t, torch.float32, x0.dim()), _coef(sqrt_1mac, t, torch.float32, x0.dim())
    x0, noise, m, x = f(x0), f(noise), f(mask), f(x)
    if control == "fma":
        q = (sa.double() * x0.double() + (s1 * noise).double()).float()       # the fp32 product is exact in fp64
    else:
        q = sa * x0 + s1 * noise
    if control == "one_minus":
        kx = ((1.0 - m.double()) * x.double()).float()
    else:
        kx = (1.0 - m) * x
    return q * m + kx


def violations(got, ref, mag):
    """Elements outside |got - ref| <= ROUNDINGS * 2^-24 * mag, and the largest ratio to that bound."""
    err = (got.detach().cpu().double() - ref).abs().reshape(-1)
    bound = (ROUNDINGS * E * mag).reshape(-1)
    ok_zero = (bound == 0) & (err == 0)
    ratio = torch.where(ok_zero, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return int((err > bound).sum()), float(ratio.max())


def make_operands(B, C, hw, per_b, per_c, seed, T=1000, soft_mask=True):
    """Seeded operands of one blend on the CPU: Gaussian x0 / noise / x, the linear-beta tables, a per-sample time, and a mask
    with exact zeros and ones besides values in between (a soft mask is a legitimate use: feathered edges)."""
    g = torch.Generator().manual_seed(seed)
    shape = (B, C) + tuple(hw)
    x0, noise, x = (torch.randn(*shape, generator=g) for _ in range(3))
    ms = mask_shape(B, C, hw, per_b, per_c)
    m = torch.rand(*ms, generator=g)
    if soft_mask:
        # (torch.rand draws multiples of 2^-24, for which 1 - m is exact: the square root has low-order bits)
        m = torch.where(m < 0.3, torch.zeros_like(m), torch.where(m > 0.7, torch.ones_like(m), torch.rand(*ms, generator=g).sqrt() * 0.5))
    else:
        m = (m > 0.5).float()
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, T, dtype=torch.float64) ** 2
    ac = torch.cumprod(1 - betas, 0)
    t = torch.randint(0, T, (B,), generator=g)
    return dict(x0=x0, noise=noise, x=x, mask=m, t=t, sqrt_ac=ac.sqrt().float(), sqrt_1mac=(1 - ac).sqrt().float())


def torch_blend(o):
    """The eager loop's arithmetic in torch ops on whatever device the operands live on: q_sample (ddpm.py) then
    img_orig * mask + (1. - mask) * img."""
    nd = o["x0"].dim()
    sa = o["sqrt_ac"][o["t"]].view(-1, *([1] * (nd - 1)))
    s1 = o["sqrt_1mac"][o["t"]].view(-1, *([1] * (nd - 1)))
    q = sa * o["x0"] + s1 * o["noise"]
    return q * o["mask"] + (1. - o["mask"]) * o["x"]


# ------------------------------------------------------------------------------------------------ the reference's masked runs

_FIXTURE = []


def fixture():
    if not _FIXTURE:
        _FIXTURE.append(torch.load(os.path.join(GOLDEN, "ddim_edit.pt"), weights_only=False))
    return _FIXTURE[0]


def case_names(min_steps=1, max_steps=10 ** 9):
    return [k for k, v in fixture()["cases"].items() if min_steps <= v["S"] <= max_steps]


class AnalyticModel:
    """eps(x, t, c) = tanh(0.7 x + 0.001 t) * c with the sampler-facing attributes of an LDM, the fp32 tables q_sample reads
    and q_sample(x_start, t, noise=None) itself.  Every Python-level call logs its batch size; every EXECUTION (a graph replay
    included, which does not call Python) appends t[0] to a log held on the tensors' device.  with_engine: what the samplers
    ask of an engine around and inside a replayed loop.  tables=False: a model without q_sample's tables."""
    num_timesteps = 1000
    parameterization = "eps"

    def __init__(self, device="cpu", with_engine=False, tables=True):
        fx = fixture()
        self.device = torch.device(device)
        self.alphas_cumprod = fx["alphas_cumprod"].clone()
        self.alphas_cumprod_prev = torch.cat([torch.ones(1), self.alphas_cumprod[:-1]])
        self.betas = torch.zeros(1, device=self.device)
        self._sa = fx["sqrt_alphas_cumprod"].to(self.device)
        self._s1 = fx["sqrt_one_minus_alphas_cumprod"].to(self.device)
        if tables:
            self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod = self._sa, self._s1
        self.calls = []
        self.tlog = torch.zeros(256, dtype=torch.long, device=self.device)
        self.k = torch.zeros(1, dtype=torch.long, device=self.device)
        if with_engine:
            eng = SimpleNamespace(cache_context_kv=False, reset_context_cache=lambda: None, detach_context_cache=lambda: None,
                                  unet=SimpleNamespace(ip_layers=()))
            self.engine = lambda: eng

    def apply_model(self, x, t, c):
        assert t.dtype == torch.long and t.shape == (x.shape[0],)
        if isinstance(c, dict):
            c = c["c_crossattn"][0]
        self.calls.append(int(x.shape[0]))
        self.tlog.index_copy_(0, self.k, t[:1])
        self.k += 1
        return torch.tanh(0.7 * x + 0.001 * t.float().view(-1, 1, 1, 1)) * c.view(-1, 1, 1, 1)

    def q_sample(self, x_start, t, noise=None):
        noise = torch.randn_like(x_start) if noise is None else noise
        return self._sa[t].view(-1, 1, 1, 1) * x_start + self._s1[t].view(-1, 1, 1, 1) * noise

    def executed_times(self):
        return self.tlog[:int(self.k)].cpu().tolist()


def run_case(name, device="cpu", use_graph=False, with_engine=False, tables=True, mask=None, S=None):
    """Run fixture case `name` through DDIMSampler.sample with the case's fixed forward-process noise.  mask / S: another mask
    or step count than the case's (for the paths that must stay eager).  Returns (result, intermediates, model, case)."""
    from cldm.ddim_hacked import DDIMSampler
    case = fixture()["cases"][name]
    model = AnalyticModel(device, with_engine, tables)
    s = DDIMSampler(model)
    s.use_graph = use_graph
    s.q_noise = case["q_noise"].to(device)
    x_T = case["x_T"].to(device)
    mask = (case["mask"] if mask is None else mask).to(device)
    out, inter = s.sample(case["S"] if S is None else S, x_T.shape[0], tuple(x_T.shape[1:]), case["c"].to(device), verbose=False,
                          x_T=x_T, eta=0.0, log_every_t=case["log_every_t"], unconditional_guidance_scale=case["scale"],
                          unconditional_conditioning=case["uc"].to(device), mask=mask, x0=case["x0"].to(device))
    assert out.shape == x_T.shape and out.dtype == torch.float32
    return out, inter, model, case


def check_case(out, inter, model, case, python_steps=None):
    """Result, intermediates, model times and batch sizes against the reference's record.  python_steps: how many of the S
    steps called Python (all of them unless a captured step replays).  Returns the worst rel_l2."""
    S, B = case["S"], case["x_T"].shape[0]
    passes = 1 if case["scale"] == 1.0 else 2
    assert len(case["times"]) == S * passes
    assert model.executed_times() == case["times"]                   # integers: exactly
    n_py = (S if python_steps is None else python_steps) * passes
    assert model.calls == case["batch_sizes"][:n_py] == [B] * n_py, model.calls
    worst = rel_l2(out, case["result"])
    for key in ("x_inter", "pred_x0"):
        assert len(inter[key]) == len(case[key]), (key, len(inter[key]), len(case[key]))
        worst = max([worst] + [rel_l2(a, b) for a, b in zip(inter[key], case[key])])
    print(f"S {S} cfg {case['scale']}: worst rel_l2 against the reference's run {worst:.3e} (gate {TOL:g})")
    assert worst < TOL, worst
    return worst


def blend_refusals(L, p, q, r):
    """Every refusal of cl_qsample_blend as {label: return code}; p, q, r: three valid, distinct, non-overlapping device
    addresses with room for the call's 64 floats (never read: a refusal is decided on the host before anything is launched).
    out = r unless stated."""
    N = None

    def call(x0=p, noise=p, t=p, sa=p, s1=p, T=1000, mask=q, pb=1, pc=1, x=q, out=r, B=2, C=4, HW=8):
        return L.cl_qsample_blend(x0, noise, t, sa, s1, T, mask, pb, pc, x, out, B, C, HW, N)

    return {
        "null x0": call(x0=N), "null noise": call(noise=N), "null t": call(t=N), "null sqrt_ac": call(sa=N), "null sqrt_1mac": call(s1=N),
        "null mask": call(mask=N), "null x": call(x=N), "null out": call(out=N), "B<0": call(B=-1), "C<1": call(C=0), "HW<1": call(HW=0),
        "T<1": call(T=0), "out is x0": call(x0=r), "out is noise": call(noise=r), "out is mask": call(mask=r),
        "out inside x0": call(x0=r - 16), "out overlaps x in part": call(x=r + 16),
    }
