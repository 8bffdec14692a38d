"""Golden vectors for the DPM-Solver++ sampler from the UNMODIFIED reference
(ldm/models/diffusion/dpm_solver/{sampler,dpm_solver}.py; build container only).

    python tests/golden/make_golden_dpm_solver.py        # writes tests/golden/dpm_solver.pt

The solver is driven by the analytic eps model of ddim_codec.pt with per-sample scale TENSORS as conditionings (the
reference batches guidance as torch.cat([unconditional, conditional])): eps(x, t, c) = tanh(0.7 x + 0.001 t) * c,
c = 1.0 (conditional) / 0.6 (unconditional).  `sampler` cases go through DPMSolverSampler.sample (order 2, time_uniform,
lower_order_final); `solver` cases through DPM_Solver.sample over model_wrapper (predict_x0=True, multistep) for the orders
and the time grid the sampler class does not expose.  Every case holds its inputs, the reference's result, and the model
input time and batch size of every model call (a case the reference itself cannot run keeps `result` = None and the error).  The fixture holds inputs and the reference's outputs only.
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
SAMPLER_CASES = ((20, 7.5), (20, 1.0), (10, 7.5), (4, 3.0), (50, 7.5))                      # (S, guidance scale)
SOLVER_CASES = ((3, 20, "time_uniform"), (3, 8, "time_uniform"), (1, 10, "time_uniform"), (2, 10, "time_quadratic"))
SOLVER_SCALE = 7.5


def main():
    G.install_stubs()
    G.use_reference_packages()
    from ldm.models.diffusion.ddpm import DDPM
    from ldm.models.diffusion.dpm_solver import dpm_solver as D
    from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler
    m = DDPM.__new__(DDPM)
    nn.Module.__init__(m)
    m.v_posterior = 0.0
    m.parameterization = "eps"
    m.register_schedule(beta_schedule="linear", timesteps=1000, linear_start=0.00085, linear_end=0.0120)

    calls = []

    def eps_model(x, t, c):
        calls.append((float(t.reshape(-1)[0]), int(x.shape[0]), bool((t == t.reshape(-1)[0]).all())))
        return torch.tanh(0.7 * x + 0.001 * t.float().view(-1, 1, 1, 1)) * c.view(-1, 1, 1, 1)

    class Stub:
        num_timesteps = 1000
        device = torch.device("cpu")
        parameterization = "eps"

    stub = Stub()
    for k in ("betas", "alphas_cumprod", "alphas_cumprod_prev"):
        setattr(stub, k, getattr(m, k).clone())
    stub.apply_model = eps_model
    DPMSolverSampler.register_buffer = lambda self, n, a: setattr(self, n, a)    # the reference moves buffers to "cuda"

    def run(fn, *a, **k):
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            return fn(*a, **k)

    g = torch.Generator().manual_seed(23)
    x_T = {s: torch.randn(*s, generator=g) for s in SHAPES}
    out = dict(alphas_cumprod=stub.alphas_cumprod.clone(), cases={},
               sample_params=list(inspect.signature(DPMSolverSampler.sample).parameters))

    def record(name, x, S, scale, order, skip_type, res):
        assert len(calls) == S and all(same for _, _, same in calls)
        B = x.shape[0]
        out["cases"][name] = dict(x_T=x.clone(), c=torch.full((B,), 1.0), uc=torch.full((B,), 0.6), S=S, scale=scale, order=order,
                                  skip_type=skip_type, result=res.clone(), times=[t for t, _, _ in calls],
                                  batch_sizes=[b for _, b, _ in calls])

    n = 0
    for S, scale in SAMPLER_CASES:
        # the first case runs on both shapes, the others alternate
        for shape in (SHAPES if n == 0 else (SHAPES[n % 2],)):
            x = x_T[shape]
            B = shape[0]
            del calls[:]
            res, _ = run(DPMSolverSampler(stub).sample, S, B, shape[1:], torch.full((B,), 1.0), x_T=x.clone(),
                         unconditional_guidance_scale=scale, unconditional_conditioning=torch.full((B,), 0.6))
            record(f"sampler_S{S}_cfg{scale}_n{x.numel()}", x, S, scale, 2, "time_uniform", res)
        n += 1
    for order, S, skip_type in SOLVER_CASES:
        shape = SHAPES[n % 2]
        x = x_T[shape]
        B = shape[0]
        ns = D.NoiseScheduleVP("discrete", alphas_cumprod=stub.alphas_cumprod)
        fn = D.model_wrapper(lambda x_, t_, c_: eps_model(x_, t_, c_), ns, model_type="noise", guidance_type="classifier-free",
                             condition=torch.full((B,), 1.0), unconditional_condition=torch.full((B,), 0.6),
                             guidance_scale=SOLVER_SCALE)
        del calls[:]
        name = f"solver_o{order}_S{S}_{skip_type}_n{x.numel()}"
        try:
            with torch.no_grad():
                res = run(D.DPM_Solver(fn, ns, predict_x0=True, thresholding=False).sample, x.clone(), steps=S,
                          skip_type=skip_type, method="multistep", order=order, lower_order_final=True)
        except ValueError as e:
            # order 3 with S < 15: lower_order_final asks the second-order update for the last steps and hands it the
            # three-entry history (dpm_solver.py:1061-1067 -> :740 "too many values to unpack"), so the reference has no
            # result for this case.  The inputs and the calls it made before raising are kept; `result` is None.
            out["cases"][name] = dict(x_T=x.clone(), c=torch.full((B,), 1.0), uc=torch.full((B,), 0.6), S=S, scale=SOLVER_SCALE,
                                      order=order, skip_type=skip_type, result=None, reference_error=f"{type(e).__name__}: {e}",
                                      times=[t for t, _, _ in calls], batch_sizes=[b for _, b, _ in calls])
            n += 1
            continue
        record(name, x, S, SOLVER_SCALE, order, skip_type, res)
        n += 1
    torch.save(out, f"{HERE}/dpm_solver.pt")
    print("[golden] dpm_solver.pt written;", list(out["cases"]), out["sample_params"])


if __name__ == "__main__":
    main()
