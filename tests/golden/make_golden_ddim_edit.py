"""Golden vectors for MASKED DDIM sampling from the UNMODIFIED reference (cldm/ddim_hacked.py:123-178; build container only).

    python tests/golden/make_golden_ddim_edit.py        # writes tests/golden/ddim_edit.pt

DDIMSampler.sample(mask=, x0=) is driven on the CPU by the analytic eps model of plms.pt with per-sample scale TENSORS as
conditionings: eps(x, t, c) = tanh(0.7 x + 0.001 t) * c, c = 1.0 (conditional) / 0.6 (unconditional); the reference evaluates
the two guidance passes one after the other, B each.  The stub model's q_sample uses a FIXED noise tensor stored with the case,
sqrt_ac[t] x0 + sqrt_1mac[t] noise, so that a run can be repeated anywhere.  Masks (1 = keep x0): 'B1' = (B, 1, H, W), a half
plane per sample (left half for even samples, top half for odd ones); '11' = (1, 1, H, W), a frame two cells wide.  eta = 0.
Every case holds its inputs, the reference's result, both lists of intermediates and the time and batch size of every model
call.  The fixture holds inputs and the reference's outputs only.
"""
import contextlib
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

SHAPES = ((2, 4, 8, 8), (3, 4, 5, 7))        # 512 elements, and a ragged 420 (HW = 35: the scalar form of the blend)
CASES = ((4, 1.0), (4, 7.5), (10, 1.0), (10, 7.5), (20, 1.0), (20, 7.5))     # (S, guidance scale)
log_every = lambda S: max(2, S // 2)      # keeps a middle index besides 0 and S - 1 (the default 100 would not)


def make_mask(kind, shape):
    B, _, H, W = shape
    if kind == "B1":
        m = torch.zeros(B, 1, H, W)
        for b in range(B):
            if b % 2 == 0:
                m[b, :, :, : W // 2] = 1.0
            else:
                m[b, :, : H // 2, :] = 1.0
        return m
    m = torch.ones(1, 1, H, W)
    m[:, :, 2:H - 2, 2:W - 2] = 0.0
    return m


def main():
    G.install_stubs()
    G.use_reference_packages()
    from ldm.models.diffusion.ddpm import DDPM
    from cldm.ddim_hacked import DDIMSampler
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
            sa = self.sqrt_alphas_cumprod[t].view(-1, 1, 1, 1)
            s1 = self.sqrt_one_minus_alphas_cumprod[t].view(-1, 1, 1, 1)
            return sa * x_start + s1 * self.q_noise

    stub = Stub()
    for k in ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod"):
        setattr(stub, k, getattr(m, k).clone())
    stub.apply_model = eps_model
    DDIMSampler.register_buffer = lambda self, n, a: setattr(self, n, a)    # the reference moves buffers to "cuda"

    def run(fn, *a, **k):
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            return fn(*a, **k)

    g = torch.Generator().manual_seed(47)
    draw = lambda s: torch.randn(*s, generator=g)
    inputs = {s: dict(x_T=draw(s), x0=draw(s), q_noise=draw(s)) for s in SHAPES}
    out = dict(alphas_cumprod=stub.alphas_cumprod.clone(), sqrt_alphas_cumprod=stub.sqrt_alphas_cumprod.clone(),
               sqrt_one_minus_alphas_cumprod=stub.sqrt_one_minus_alphas_cumprod.clone(), cases={})
    for n, (S, scale) in enumerate(CASES):
        shape, kind = SHAPES[n % 2], ("B1", "11")[(n // 2 + n) % 2]
        B, inp = shape[0], inputs[shape]
        mask = make_mask(kind, shape)
        stub.q_noise = inp["q_noise"]
        del calls[:]
        res, inter = run(DDIMSampler(stub).sample, S, B, shape[1:], torch.full((B,), 1.0), x_T=inp["x_T"].clone(), verbose=False,
                         eta=0.0, log_every_t=log_every(S), unconditional_guidance_scale=scale,
                         unconditional_conditioning=torch.full((B,), 0.6), mask=mask, x0=inp["x0"].clone())
        passes = 1 if scale == 1.0 else 2
        assert len(calls) == S * passes and bool(torch.isfinite(res).all())
        keep = mask.expand(B, shape[1], *shape[2:]) == 1.0
        # no clones: torch.save stores a tensor once (x_inter opens with x_T and closes with the result)
        out["cases"][f"S{S}_cfg{scale}_{kind}_n{inp['x_T'].numel()}"] = dict(
            x_T=inp["x_T"], x0=inp["x0"], q_noise=inp["q_noise"], mask=mask, c=torch.full((B,), 1.0), uc=torch.full((B,), 0.6),
            S=S, scale=scale, log_every_t=log_every(S), result=res, x_inter=list(inter["x_inter"]), pred_x0=list(inter["pred_x0"]),
            times=[t for t, _ in calls], batch_sizes=[b for _, b in calls])
        assert not torch.equal(res[keep], inp["x0"][keep])      # the last step runs after the last blend: no region is x0 itself
    torch.save(out, f"{HERE}/ddim_edit.pt")
    print("[golden] ddim_edit.pt written;", {k: v["times"][:4] for k, v in out["cases"].items()})


if __name__ == "__main__":
    main()
