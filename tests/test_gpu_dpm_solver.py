"""DPM-Solver++ on the MI355X (run with -m gpu): the float timestep embedding (cl_timestep_embedding_f), the fused multistep
update (cl_dpmpp_step / cl_dpmpp_step_dev / cl_dpm_set_t), the sampler's eager and graphed loops against runs of the
UNMODIFIED reference (tests/golden/dpm_solver.pt), the whole model against the CPU oracle, and scripts/sample.py --sampler dpm.

Gates: kernels 2e-6 (the gates of cl_timestep_embedding and cl_ddim_step); the sampler on the analytic model 1e-5 (ENC_TOL);
the whole model in fp32 5e-4 on the trajectory and 1e-4 on one eps (the gates of the DDIM trajectory and of eps in
tests/test_gpu_parity.py); bf16: the deviation of the DPM-Solver++ trajectory at most 1.5 x the deviation of our bf16 DDIM
trajectory from its own oracle, both measured here.
"""
import glob
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from tests.dpm_solver_cases import case_names, check_case, fixture, run_case
from tests.util import ROOT, rel_l2

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ctrlora_amd import hip
    hip.lib()           # raises if the HIP library is missing: no silent fallback


# ------------------------------------------------------------------------------ cl_timestep_embedding_f

def test_timestep_embedding_f_matches_oracle_and_the_long_kernel_bit_for_bit():
    _need_gpu()
    from ctrlora_amd import hip
    from oracle import ref_model as R
    half = 160
    freqs = torch.exp(-math.log(10000.0) * torch.arange(0, half, dtype=torch.float32) / half).cuda()
    t = torch.tensor([0.0, 0.5, 17.0, 949.05, 999.0], dtype=torch.float32)
    out = torch.full((5, 2 * half), float("nan"), device="cuda")
    hip.timestep_embedding_f(t.cuda(), freqs, out)
    err = float((out.cpu() - R.timestep_embedding(t, 2 * half)).abs().max())
    print(f"max abs err {err:.3e}")
    assert err < 2e-6
    out_bf = torch.zeros((5, 2 * half), dtype=torch.bfloat16, device="cuda")
    hip.timestep_embedding_f(t.cuda(), freqs, out_bf)
    assert torch.equal(out_bf, out.to(torch.bfloat16))              # one rounding of the fp32 value
    ti = torch.tensor([0, 1, 17, 949, 999], dtype=torch.long).cuda()
    for dtype in (torch.float32, torch.bfloat16):
        a = torch.zeros((5, 2 * half), dtype=dtype, device="cuda")
        b = torch.ones((5, 2 * half), dtype=dtype, device="cuda")
        hip.timestep_embedding(ti, freqs, a)
        hip.timestep_embedding_f(ti.float(), freqs, b)
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------ cl_dpmpp_step

def _step64(x, e_c, e_u, row, scale, h1, h2):
    """The update of one step in fp64 on the fp32 table row {alpha, sigma, cx, c0, c1, c2, ...}."""
    alpha, sigma, cx, c0, c1, c2 = (float(v) for v in row[:6])
    d = lambda v: v.double().cpu()
    e = d(e_c) if e_u is None else d(e_u) + float(np.float32(scale)) * (d(e_c) - d(e_u))
    m = (d(x) - sigma * e) / alpha
    xn = cx * d(x) + c0 * m
    if c1 != 0.0:
        xn = xn + c1 * d(h1)
    if c2 != 0.0:
        xn = xn + c2 * d(h2)
    return xn, m


@pytest.mark.parametrize("n", [420, 512])
def test_dpmpp_step_orders_history_aliasing_and_device_cursor(n):
    """Steps 0..3 of an order-3 table (orders 1, 2, 3, 3) over a history ring pre-filled with NaN: every step against the
    fp64 restatement; a zero coefficient's slot is not read; x_next aliasing x and the device-cursor launch give the bits of
    the plain host-index call."""
    _need_gpu()
    from ctrlora_amd import hip
    from ldm.models.diffusion.dpm_solver.sampler import dpmpp_table
    S, scale = 20, 7.5
    _, tab64, orders = dpmpp_table(fixture()["alphas_cumprod"], S, order=3)
    assert orders[:4] == [1, 2, 3, 3]
    tab = torch.as_tensor(tab64).float().contiguous()
    coef = tab.cuda()
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g).cuda()
    hist = torch.full((3, n), float("nan"), device="cuda")
    cursor = torch.zeros(1, dtype=torch.int32, device="cuda")
    for i in range(4):
        e_c, e_u = torch.randn(n, generator=g).cuda(), (torch.randn(n, generator=g).cuda() if i != 2 else None)
        before = hist.clone()
        h1, h2 = before[(i + 2) % 3], before[(i + 1) % 3]
        x_next, p0 = torch.empty_like(x), torch.empty_like(x)
        hip.dpmpp_step(x, e_c, e_u, coef, i, scale, hist, x_next, p0)
        assert bool(torch.isfinite(x_next).all()) and bool(torch.isfinite(p0).all())      # no NaN slot was read
        want_x, want_m = _step64(x, e_c, e_u, tab[i], scale, h1, h2)
        errs = rel_l2(x_next, want_x), rel_l2(p0, want_m), rel_l2(hist[i % 3], want_m)
        print(f"n {n} step {i} order {orders[i]}: rel_l2 x_next {errs[0]:.2e} pred_x0 {errs[1]:.2e} hist {errs[2]:.2e}")
        assert max(errs) < 2e-6, errs
        assert torch.equal(hist[i % 3], p0)
        for k in (1, 2):                                            # the other two slots are untouched (NaN until written)
            s = (i + k) % 3
            assert torch.equal(hist[s].isnan(), before[s].isnan()) and torch.equal(hist[s].nan_to_num(), before[s].nan_to_num())
        if i == 0:
            assert bool(hist[1:].isnan().all())
        if i == 1:
            assert bool(hist[2].isnan().all())                      # order 2 read only the slot step 0 wrote
        # x_next aliasing x
        xa, ha = x.clone(), before.clone()
        hip.dpmpp_step(xa, e_c, e_u, coef, i, scale, ha, xa, None)
        assert torch.equal(xa, x_next) and torch.equal(ha[i % 3], hist[i % 3])
        # device cursor at i
        xd, hd, pd = torch.empty_like(x), before.clone(), torch.empty_like(x)
        cursor.fill_(i)
        hip.dpmpp_step_dev(x, e_c, e_u, coef, cursor, S, scale, hd, xd, pd)
        assert torch.equal(xd, x_next) and torch.equal(pd, p0) and torch.equal(hd[i % 3], hist[i % 3])
        x = x_next
    # time of the step under the cursor, clamped to the last row
    ts = torch.zeros(7, device="cuda")
    for cur in (0, 3, S - 1, S + 5):
        cursor.fill_(cur)
        hip.dpm_set_t(coef, cursor, S, ts)
        assert torch.equal(ts.cpu(), torch.full((7,), float(tab[min(cur, S - 1), 6])))
    # the host-index form refuses what it cannot index
    L = hip.lib()
    args = lambda index, S_: (x.data_ptr(), x.data_ptr(), None, coef.data_ptr(), index, S_, scale, hist.data_ptr(),
                              x_next.data_ptr(), None, n, hip.stream())
    assert L.cl_dpmpp_step(*args(S, S)) == 1 and L.cl_dpmpp_step(*args(-1, S)) == 1 and L.cl_dpmpp_step(*args(0, 0)) == 1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ the sampler against the reference's runs

@pytest.mark.parametrize("name", case_names())
def test_fixture_case_eager(name):
    _need_gpu()
    out, model, case = run_case(name, device="cuda", use_graph=False, with_engine=True)
    assert len(model.calls) == case["S"]                            # every step called the model from Python
    check_case(out, model, case)


@pytest.mark.parametrize("name", case_names(min_steps=4))
def test_fixture_case_graphed_equals_eager(name):
    _need_gpu()
    out, model, case = run_case(name, device="cuda", use_graph=True, with_engine=True)
    assert len(model.calls) == 2                                    # one eager step, one capture; the rest replayed
    check_case(out, model, case)
    eager, _, _ = run_case(name, device="cuda", use_graph=False, with_engine=True)
    assert torch.equal(out, eager)


def test_three_steps_take_the_eager_loop_and_models_without_engine_too():
    _need_gpu()
    name = "sampler_S4_cfg3.0_n420"
    cpu, _, _ = run_case(name, steps=3)
    out, model, _ = run_case(name, device="cuda", use_graph=True, with_engine=True, steps=3)
    assert len(model.calls) == 3 and len(model.executed_times()) == 3
    assert rel_l2(out, cpu) < 1e-5
    out4, model4, case = run_case(name, device="cuda", use_graph=True, with_engine=False)
    assert len(model4.calls) == 4
    check_case(out4, model4, case)


def test_dict_and_structurally_different_conditionings_on_the_gpu():
    _need_gpu()
    name = "sampler_S10_cfg7.5_n512"
    for graph in (False, True):
        ref, _, case = run_case(name, device="cuda", use_graph=graph, with_engine=True)
        out, model, _ = run_case(name, device="cuda", use_graph=graph, with_engine=True, conds="dict")
        check_case(out, model, case)
        assert torch.equal(out, ref)
        out2, model2, _ = run_case(name, device="cuda", use_graph=graph, with_engine=True, conds="different")
        check_case(out2, model2, case, passes=2)
        assert torch.equal(out2, ref)


# ------------------------------------------------------------------------------ whole model

S_MODEL, SCALE_MODEL = 6, 7.5


def _restated_dpmpp_2m(eps_fn, alphas_cumprod, S, x_T, scale):
    """DPM-Solver++(2M) written from the method (arXiv:2211.01095, Alg. 2) in its difference form, not from the sampler's
    coefficient table: uniform time grid, fp64 schedule, fp32 state, first step and (S < 15) last step of first order.
    eps_fn(x, t_float, cond: bool)."""
    ac = alphas_cumprod.double().numpy()
    N = ac.shape[0]
    t = np.linspace(1.0, 1.0 / N, S + 1)
    log_a = np.interp(t, np.arange(1, N + 1) / N, 0.5 * np.log(ac))
    alpha, sigma = np.exp(log_a), np.sqrt(1.0 - np.exp(2.0 * log_a))
    lam = log_a - np.log(sigma)
    f = lambda v: torch.tensor(float(v), dtype=torch.float32)
    x, prev, times = x_T, None, []
    for i in range(S):
        t_in = torch.full((x.shape[0],), (t[i] - 1.0 / N) * 1000.0, dtype=torch.float32)
        times.append(float(t_in[0]))
        e_c, e_u = eps_fn(x, t_in, True), eps_fn(x, t_in, False)
        e = e_u + scale * (e_c - e_u)
        m = (x - f(sigma[i]) * e) / f(alpha[i])
        h = lam[i + 1] - lam[i]
        a_phi = alpha[i + 1] * np.expm1(-h)
        x_new = f(sigma[i + 1] / sigma[i]) * x - f(a_phi) * m
        if prev is not None and not (S < 15 and i == S - 1):
            r0 = (lam[i] - lam[i - 1]) / h
            x_new = x_new - f(0.5 * a_phi / r0) * (m - prev)
        x, prev = x_new, m
    return x, times


@pytest.fixture(scope="module")
def tiny():
    """The tiny drop-in model of test_api_training_step_and_ddim_through_the_drop_in_classes, its weights for the oracle,
    seeded inputs, and the oracle's fp32 DPM-Solver++ trajectory (computed once, read by both dtype tests)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import bench
    from oracle import arch, ref_model as R
    from tests.golden.make_golden import inputs_for
    cfg = arch.TINY
    model = bench.build_model("ctrlora_finetune_sd15_rank128.yaml", 0, tiny=True).cuda().eval()
    sd_cn = {k: v.detach().cpu().clone() for k, v in model.control_model.state_dict().items()}
    sd_un = {k: v.detach().cpu().clone() for k, v in model.model.diffusion_model.state_dict().items()}
    inp = inputs_for(cfg, 2, 16, 8)
    g = torch.Generator().manual_seed(1)
    x_T = torch.randn(2, 4, 16, 16, generator=g)
    ctx_u = torch.randn(2, 77, cfg.context_dim, generator=g)
    cu = lambda v: v.cuda()
    cond = {"c_crossattn": [cu(inp["ctx"])], "c_concat": [cu(inp["hint_z"])]}
    unc = {"c_crossattn": [cu(ctx_u)], "c_concat": [cu(inp["hint_z"])]}

    def eps_fn(x, t, c):
        with torch.no_grad():
            return R.apply_model(sd_cn, sd_un, cfg, x, t, inp["ctx"] if c else ctx_u, inp["hint_z"])

    ref, times = _restated_dpmpp_2m(eps_fn, model.alphas_cumprod.detach().cpu(), S_MODEL, x_T, SCALE_MODEL)
    return dict(model=model, eps_fn=eps_fn, x_T=x_T, cond=cond, unc=unc, ref=ref, times=times, inp=inp)


def _dpm_sample(t, use_graph):
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    s = DPMSolverSampler(t["model"])
    s.use_graph = use_graph
    out, aux = s.sample(S_MODEL, 2, (4, 16, 16), t["cond"], verbose=False, x_T=t["x_T"].cuda(),
                        unconditional_guidance_scale=SCALE_MODEL, unconditional_conditioning=t["unc"])
    assert aux is None
    return out


def test_whole_model_fp32_trajectory_graph_and_untruncated_time(tiny):
    _need_gpu()
    from oracle import ref_model as R
    model = tiny["model"]
    model.set_engine_dtype(torch.float32)
    assert abs(tiny["times"][1] - 999.0 * (1.0 - 1.0 / S_MODEL)) < 1e-3      # 832.5: not an integer
    graphed = _dpm_sample(tiny, True)
    err = rel_l2(graphed, tiny["ref"])
    print(f"fp32 DPM-Solver++ S={S_MODEL} CFG {SCALE_MODEL}: rel_l2 vs the oracle's restatement {err:.3e}")
    assert err < 5e-4
    assert torch.equal(graphed, _dpm_sample(tiny, False))
    # one forward at a non-integer time: the oracle's eps, and NOT the eps of the truncated time
    x = tiny["x_T"]
    t_f = torch.full((2,), 949.05, dtype=torch.float32)
    with torch.no_grad():
        e_f = model.apply_model(x.cuda(), t_f.cuda(), tiny["cond"])
        e_i = model.apply_model(x.cuda(), torch.full((2,), 949, dtype=torch.long).cuda(), tiny["cond"])
    want = tiny["eps_fn"](x, t_f, True)
    err_f, gap = rel_l2(e_f, want), rel_l2(e_f, e_i)
    print(f"eps at t = 949.05: rel_l2 vs oracle {err_f:.3e}; vs eps at t = 949 {gap:.3e}")
    assert err_f < 1e-4
    assert gap > 1e-4


def test_whole_model_bf16_deviates_like_ddim(tiny):
    """DESIGN 1d quotes both figures.  First-order DPM-Solver++ is the DDIM update, so the two samplers should amplify the
    bf16 error of eps alike: 1.5 x is the margin the project gives sampled trajectories."""
    _need_gpu()
    from cldm.ddim_hacked import DDIMSampler
    from oracle import ref_model as R
    model = tiny["model"]
    model.set_engine_dtype(torch.bfloat16)
    try:
        d_dpm = rel_l2(_dpm_sample(tiny, True), tiny["ref"])
        ddim, _ = DDIMSampler(model).sample(S_MODEL, 2, (4, 16, 16), tiny["cond"], verbose=False, eta=0.0, x_T=tiny["x_T"].cuda(),
                                            unconditional_guidance_scale=SCALE_MODEL, unconditional_conditioning=tiny["unc"])
        eps_long = lambda x, t, c: tiny["eps_fn"](x, t, c)
        ddim_ref, _ = R.ddim_sample(eps_long, R.make_schedule(), S_MODEL, tiny["x_T"], scale=SCALE_MODEL, uncond=True)
        d_ddim = rel_l2(ddim, ddim_ref)
    finally:
        model.set_engine_dtype(torch.float32)
    print(f"bf16 S={S_MODEL} CFG {SCALE_MODEL}: DPM-Solver++ vs fp32 restatement {d_dpm:.3e}; DDIM vs its oracle {d_ddim:.3e}")
    assert d_dpm < 1.5 * d_ddim, (d_dpm, d_ddim)


# ------------------------------------------------------------------------------ scripts/sample.py --sampler dpm

def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_sample_script_dpm_end_to_end_and_default_unchanged(tmp_path, monkeypatch):
    """`--sampler dpm` writes a finite, non-constant image through the real first stage; without the flag main() writes
    the bytes that DDIMSampler through sample_dataset -- the script as it was -- writes."""
    _need_gpu()
    import sys
    monkeypatch.setenv("CTRLORA_SYNTHETIC_TOKENIZER", "1")
    assets = str(tmp_path / "synth")
    tool = _load(os.path.join(ROOT, "tests", "tools", "make_synthetic_assets.py"), "make_synthetic_assets")
    monkeypatch.setattr(sys, "argv", ["make_synthetic_assets.py", "--out", assets, "--n", "1"])
    tool.main()
    from cldm.ddim_hacked import DDIMSampler
    from cldm.model import create_model, load_state_dict
    from datasets.custom_dataset import CustomDataset
    from torch.utils.data import Subset
    cfg, data = os.path.join(assets, "finetune_narrow.yaml"), os.path.join(assets, "custom")
    torch.manual_seed(3)
    model = create_model(cfg).cpu()
    ckpt = str(tmp_path / "full.ckpt")
    torch.save({"state_dict": model.state_dict()}, ckpt)
    sample = _load(os.path.join(ROOT, "scripts", "sample.py"), "sample")
    argv = lambda d, *extra: ["--dataroot", data, "--config", cfg, "--ckpt", ckpt, "--n_samples", "1", "--save_dir",
                              str(tmp_path / d), "--ddim_steps", "4", *extra]
    assert sample.get_parser().parse_args(argv("x")).sampler == "ddim"
    # the script as it was: DDIMSampler handed to sample_dataset
    model.load_state_dict(load_state_dict(ckpt, location="cpu"), strict=True)
    model = model.cuda().eval()
    torch.manual_seed(5)
    sample.sample_dataset(model, DDIMSampler(model), Subset(CustomDataset(data), range(1)), sample.get_parser().parse_args(argv("was")))
    del model
    torch.manual_seed(5)
    sample.main(argv("ddim"))
    torch.manual_seed(5)
    sample.main(argv("dpm", "--sampler", "dpm"))
    png = lambda d: open(glob.glob(str(tmp_path / d / "sample" / "*.png"))[0], "rb").read()
    assert png("ddim") == png("was")
    assert png("dpm") != png("ddim")
    from PIL import Image
    img = np.asarray(Image.open(glob.glob(str(tmp_path / "dpm" / "sample" / "*.png"))[0]))
    assert img.shape[-1] == 3 and img.std() > 0, "the sampled image is constant"
    assert open(tmp_path / "dpm" / "prompt.txt").read().count("\n") == 1
