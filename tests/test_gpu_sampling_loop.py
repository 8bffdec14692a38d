"""The DDIM sampler's captured-step loop against its eager loop on the MI355X (run with -m gpu), and the two launches of the
fused DDIM update against each other.

The graphed loop (ldm/models/diffusion/guided_loop.run_steps) runs the kernels of the eager loop: the same engine launches,
and cl_ddim_step_dev / cl_ddim_step share one device body.  With eta = 0 the eager loop's sigma * noise term adds exact zeros.
So the two paths must agree BIT FOR BIT, and the Python-level apply_model calls must be 2 per pass for the graphed loop
(one eager step, one capture) against S for the eager one.
"""
import pytest
import torch

from tests import ew_ref

pytestmark = pytest.mark.gpu

B, SCALE = 2, 7.5


@pytest.fixture(scope="module")
def tiny():
    """The tiny drop-in model as the `tiny` fixture of tests/test_gpu_dpm_solver.py builds it (fp32 engine), seeded inputs."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ctrlora_amd import hip
    hip.lib()           # raises if the HIP library is missing: no silent fallback
    import bench
    from oracle import arch
    from tests.golden.make_golden import inputs_for
    cfg = arch.TINY
    model = bench.build_model("ctrlora_finetune_sd15_rank128.yaml", 0, tiny=True).cuda().eval()
    model.set_engine_dtype(torch.float32)
    inp = inputs_for(cfg, B, 16, 8)
    g = torch.Generator().manual_seed(1)
    x_T = torch.randn(B, 4, 16, 16, generator=g).cuda()
    ctx_u = torch.randn(B, 77, cfg.context_dim, generator=g).cuda()
    cond = {"c_crossattn": [inp["ctx"].cuda()], "c_concat": [inp["hint_z"].cuda()]}
    unc = {"c_crossattn": [ctx_u], "c_concat": [inp["hint_z"].cuda()]}
    return dict(model=model, x_T=x_T, cond=cond, unc=unc)


def _ddim(t, monkeypatch, S, use_graph, batch_cfg):
    """One DDIMSampler.sample(); returns (x, batch size of every Python-level apply_model call)."""
    from cldm.ddim_hacked import DDIMSampler
    model, calls = t["model"], []
    inner = model.apply_model

    def counted(x, ts, c, *a, **k):
        calls.append(int(x.shape[0]))
        return inner(x, ts, c, *a, **k)

    monkeypatch.setattr(model, "apply_model", counted)
    s = DDIMSampler(model)
    s.use_graph, s.batch_cfg = use_graph, batch_cfg
    try:
        out, _ = s.sample(S, B, (4, 16, 16), t["cond"], verbose=False, eta=0.0, x_T=t["x_T"], unconditional_guidance_scale=SCALE,
                          unconditional_conditioning=t["unc"])
    finally:
        monkeypatch.undo()
    return out, calls


@pytest.mark.parametrize("batch_cfg", [True, False])
def test_ddim_graphed_loop_gives_the_bits_of_the_eager_loop(tiny, monkeypatch, batch_cfg):
    S = 4
    passes, nb = (1, 2 * B) if batch_cfg else (2, B)
    graphed, calls_g = _ddim(tiny, monkeypatch, S, True, batch_cfg)
    eager, calls_e = _ddim(tiny, monkeypatch, S, False, batch_cfg)
    print(f"batch_cfg {batch_cfg}: Python calls graphed {len(calls_g)} eager {len(calls_e)}; "
          f"max |graphed - eager| {float((graphed - eager).abs().max()):.3e}")
    assert calls_g == [nb] * (2 * passes)           # one eager step, one capture; the other S - 2 steps are replays
    assert calls_e == [nb] * (S * passes)
    assert bool(torch.isfinite(graphed).all()) and float(graphed.std()) > 0
    assert torch.equal(graphed, eager)


def test_ddim_three_steps_take_the_eager_loop(tiny, monkeypatch):
    """A loop of 3 steps.  sample(S = 3) cannot make one on a 1000-step schedule (uniform spacing selects the 4 times 1, 334,
    667, 1000, the last outside the schedule, as in the reference), so the loop is ddim_sampling over the first 3 of the
    S = 4 schedule's times, which is how the reference's callers shorten a run."""
    from cldm.ddim_hacked import DDIMSampler
    model, calls = tiny["model"], []
    inner = model.apply_model
    monkeypatch.setattr(model, "apply_model", lambda x, ts, c: (calls.append(int(x.shape[0])), inner(x, ts, c))[1])
    s = DDIMSampler(model)
    assert s.use_graph and s.batch_cfg
    s.make_schedule(4, ddim_eta=0.0, verbose=False)
    out, _ = s.ddim_sampling(tiny["cond"], (B, 4, 16, 16), x_T=tiny["x_T"], timesteps=4, unconditional_guidance_scale=SCALE,
                             unconditional_conditioning=tiny["unc"])
    monkeypatch.undo()
    assert calls == [2 * B] * 3
    assert bool(torch.isfinite(out).all())


@pytest.mark.parametrize("n", [420, 512])          # not a multiple of a block of 256 / a whole number of blocks
def test_ddim_step_device_cursor_gives_the_bits_of_the_host_index(n):
    """cl_ddim_step_dev with the cursor at i against cl_ddim_step on row S - 1 - i (the row mapping of ddim_sampling):
    one device body, so x_prev and pred_x0 are bit-identical, with and without the unconditional eps."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ctrlora_amd import hip
    hip.lib()
    S = 20
    coef = ew_ref.ddim_table(S=S, eta=0.5)[0].contiguous().cuda()
    assert coef.shape == (S, 4) and bool((coef[:, 2] != 0).any())
    g = torch.Generator().manual_seed(n)
    x, e_c, e_u, noise = (torch.randn(n, generator=g).cuda() for _ in range(4))
    cursor = torch.zeros(1, dtype=torch.int32, device="cuda")
    rows = set()
    for i in (0, 3, S - 1):
        for u in (e_u, None):
            xp, p0, xd, pd = (torch.full((n,), float("nan"), device="cuda") for _ in range(4))
            hip.ddim_step(x, e_c, u, noise, coef, S - 1 - i, SCALE, xp, p0)
            cursor.fill_(i)
            hip.ddim_step_dev(x, e_c, u, noise, coef, cursor, S, SCALE, xd, pd)
            assert bool(torch.isfinite(xp).all()) and bool(torch.isfinite(p0).all())
            assert torch.equal(xd, xp) and torch.equal(pd, p0), (n, i, u is None)
            rows.add(xp.cpu().numpy().tobytes())
    assert len(rows) == 6                           # every row and guidance form gave another result: the row was really read
    torch.cuda.synchronize()
