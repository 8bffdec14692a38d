"""Golden vectors for the PLMS sampler from the UNMODIFIED reference (ldm/models/diffusion/plms.py; build container only).

    python tests/golden/make_golden_plms.py        # writes tests/golden/plms.pt

PLMSSampler.sample is driven on the CPU by the analytic eps model of dpm_solver.pt with per-sample scale TENSORS as
conditionings (the reference batches guidance as torch.cat([unconditional, conditional])): eps(x, t, c) =
tanh(0.7 x + 0.001 t) * c, c = 1.0 (conditional) / 0.6 (unconditional).  The masked case gives the stub model a q_sample with
a FIXED noise tensor, sqrt_ac[t] x0 + sqrt_1mac[t] noise, stored with the case, so that it can be repeated anywhere.  Every
case holds its inputs, the reference's result, both lists of intermediates and the time and batch size of every model call.
S = 3 is not a case: the reference's own make_ddim_timesteps selects timestep 1000 there (range(0, 1000, 333) has four entries)
and raises IndexError.  The fixture holds inputs and the reference's outputs only.
"""
import contextlib
import inspect
import io
import os
import sys

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import make_golden as G   # noqa: E402  (helpers only: use_reference_packages / install_stubs)

SHAPES = ((2, 4, 8, 8), (3, 4, 5, 7))        # 512 elements, and a ragged 420 (the grid-stride tail)
CASES = ((20, 7.5), (1, 7.5), (2, 3.0), (4, 3.0), (5, 7.5), (10, 1.0), (50, 7.5), (20, 1.0))     # (S, guidance scale)
MASKED = (10, 7.5)
log_every = lambda S: max(2, S // 2)      # keeps a middle index besides 0 and S - 1 (the default 100 would not)


def main():
    G.install_stubs()
    G.use_reference_packages()
    from ldm.models.diffusion.ddpm import DDPM
    from ldm.models.diffusion.plms import PLMSSampler
    m = DDPM.__new__(DDPM)
    nn.Module.__init__(m)
    m.v_posterior = 0.0
    m.parameterization = "eps"
    m.register_schedule(beta_schedule="linear", timesteps=1000, linear_start=0.00085, linear_end=0.0120)

    calls = []

    def eps_model(x, t, c):
        assert t.dtype == torch.long and bool((t == t.reshape(-1)[0]).all())
        calls.append((int(t.reshape(-1)[0]), int(x.shape[0])))
        return torch.tanh(0.7 * x + 0.001 * t.float().view(-1, 1, 1, 1)) * c.view(-1, 1, 1, 1)

    class Stub:
        num_timesteps = 1000
        device = torch.device("cpu")
        parameterization = "eps"
        q_noise = None

        def q_sample(self, x_start, t):
            sa = self.alphas_cumprod.sqrt()[t].view(-1, 1, 1, 1)
            s1 = (1. - self.alphas_cumprod).sqrt()[t].view(-1, 1, 1, 1)
            return sa * x_start + s1 * self.q_noise

    stub = Stub()
    for k in ("betas", "alphas_cumprod", "alphas_cumprod_prev"):
        setattr(stub, k, getattr(m, k).clone())
    stub.apply_model = eps_model
    PLMSSampler.register_buffer = lambda self, n, a: setattr(self, n, a)    # the reference moves buffers to "cuda"

    def run(fn, *a, **k):
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            return fn(*a, **k)

    g = torch.Generator().manual_seed(31)
    x_T = {s: torch.randn(*s, generator=g) for s in SHAPES}
    out = dict(alphas_cumprod=stub.alphas_cumprod.clone(), cases={},
               sample_params=list(inspect.signature(PLMSSampler.sample).parameters))

    def one(name, shape, S, scale, **masked):
        x, B = x_T[shape].clone(), shape[0]
        del calls[:]
        res, inter = run(PLMSSampler(stub).sample, S, B, shape[1:], torch.full((B,), 1.0), x_T=x, verbose=False,
                         log_every_t=log_every(S), unconditional_guidance_scale=scale,
                         unconditional_conditioning=torch.full((B,), 0.6), **masked)
        assert len(calls) == S + 1 and bool(torch.isfinite(res).all())
        # no clones: the lists open with x_T itself and x_inter closes with the result, and torch.save stores a tensor once
        out["cases"][name] = dict(x_T=x, c=torch.full((B,), 1.0), uc=torch.full((B,), 0.6), S=S, scale=scale,
                                  log_every_t=log_every(S), result=res, x_inter=list(inter["x_inter"]),
                                  pred_x0=list(inter["pred_x0"]), times=[t for t, _ in calls],
                                  batch_sizes=[b for _, b in calls], **{k: v.clone() for k, v in masked.items()})

    n = 0
    for S, scale in CASES:
        # the first case runs on both shapes, the others alternate
        for shape in (SHAPES if n == 0 else (SHAPES[n % 2],)):
            one(f"S{S}_cfg{scale}_n{x_T[shape].numel()}", shape, S, scale)
        n += 1
    shape = SHAPES[0]
    mask = torch.zeros(shape[0], 1, *shape[2:])
    mask[..., : shape[3] // 2] = 1.0                      # a half plane keeps x0, the other half is sampled
    stub.q_noise = torch.randn(*shape, generator=g)
    one(f"masked_S{MASKED[0]}_cfg{MASKED[1]}_n{x_T[shape].numel()}", shape, *MASKED, mask=mask,
        x0=torch.randn(*shape, generator=g))
    out["cases"][next(reversed(out["cases"]))]["q_noise"] = stub.q_noise.clone()
    torch.save(out, f"{HERE}/plms.pt")
    print("[golden] plms.pt written;", {k: v["times"][:4] for k, v in out["cases"].items()}, out["sample_params"])


if __name__ == "__main__":
    main()
