"""PLMS on the MI355X (run with -m gpu): the fused update (cl_plms_step / cl_plms_step_dev) element-wise against its fp64
contract, the sampler's eager and graphed loops against runs of the UNMODIFIED reference (tests/golden/plms.pt), the whole
model against the CPU oracle, and scripts/sample.py --sampler plms.

Gates: the kernel element-wise, |got - ref| <= 16 * 2^-24 * mag with zero violations (tests/plms_cases.py; derived, see
test_plms_step_phases_orders_history_aliasing_and_device_cursor); the sampler on the analytic model 1e-5 (ENC_TOL); the whole
model in fp32 5e-4 on the trajectory; bf16: at most 1.5 x the deviation of the same restated PLMS loop with the oracle's eps
under bf16 autocast, measured here.
"""
import glob
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import plms_cases as P
from tests.plms_cases import case_names, check_case, run_case
from tests.util import ROOT, rel_l2

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ctrlora_amd import hip
    hip.lib()           # raises if the HIP library is missing: no silent fallback


# ------------------------------------------------------------------------------ cl_plms_step

def _same(a, b):
    """Equal bits, NaN where NaN."""
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num())


def _guided_bits(slot, e_c, e_u, scale):
    """Is every element of `slot` one of the two fp32 evaluations of e_u + scale (e_c - e_u): product and sum rounded
    separately, or contracted into one fused multiply-add (the compiler may choose either)?  Without guidance: e_c itself."""
    if e_u is None:
        return torch.equal(slot, e_c)
    d = (e_c - e_u).double()                                    # the difference, rounded to fp32
    s = float(np.float32(scale))
    fused = (e_u.double() + s * d).float()                      # the fp32 product is exact in fp64: one rounding of the sum
    plain = e_u + (s * d).float()
    return bool(((slot == fused) | (slot == plain)).all())


def _check(got, ref, key, label):
    bad, ratio = P.violations(got, ref, key)
    print(f"{label} {key}: violations {bad}, largest |err| / bound {ratio:.3f}")
    assert bad == 0, (label, key, bad, ratio)
    assert bool(torch.isfinite(got).all()), (label, key)        # no NaN slot was read


@pytest.mark.parametrize("n", [420, 512])
def test_plms_step_phases_orders_history_aliasing_and_device_cursor(n):
    """Iterations 0 (phases 1 and 2), 1, 2, 3, 4 of a 20-step table at guidance 7.5 over a history ring pre-filled with NaN.
    Every output against the fp64 restatement formed from the fp32 table row and the fp32 inputs, element-wise:
        |got - ref| <= 16 * 2^-24 * mag,   mag = sum of the absolute values of the terms of the formula (tests/ew_ref.py),
    propagated through guidance, the multistep sum, pred_x0 and x_prev.  16 counts the fp32 roundings on the longest path
    (x_out of a fourth-order step): guidance 3, the multistep sum 5 (one product, three sums, the division), pred_x0 4
    (sqrt(a_t), the product, the difference, the quotient), x_prev 3 (sqrt(a_prev), the product, the sum) = 15, plus one for
    the direction coefficient.  The bound is derived, not measured; a contraction into fused multiply-adds only removes
    roundings.  No NaN reaches an output (only the slots of the order are read); the slot written is iter % 4 and holds the
    guided eps; the other three are untouched and phase 2 leaves all four; x_out aliasing x and the device-cursor launch give
    the bits of the host-index launch; the cursor clamps to [1, S - 1]."""
    _need_gpu()
    from ctrlora_amd import hip
    from ldm.models.diffusion.plms import PLMSSampler
    S, scale = 20, 7.5
    s = PLMSSampler(P.AnalyticModel())
    s.make_schedule(S, verbose=False)
    tab = s.coef_table.cpu()
    coef = tab.cuda().contiguous()
    g = torch.Generator().manual_seed(n)
    r = lambda: torch.randn(n, generator=g).cuda()
    x = r()
    hist = torch.full((4, n), float("nan"), device="cuda")
    cursor = torch.zeros(1, dtype=torch.int32, device="cuda")
    # ---- iteration 0, phase 1: the predictor
    e_c, e_u = r(), r()
    x_pred, keep = torch.empty_like(x), torch.full_like(x, 3.0)
    hip.plms_step(x, e_c, e_u, coef, 0, hip.PLMS_START, scale, hist, x_pred, keep)
    ref = P.plms_step_ref(x, e_c, e_u, tab[S - 1], scale, P.START, [])
    _check(x_pred, ref, "x_out", "start")
    _check(hist[0], ref, "e", "start")
    assert _guided_bits(hist[0], e_c, e_u, scale)
    assert bool(hist[1:].isnan().all()) and bool((keep == 3.0).all())          # pred_x0 is not written by the start
    # ---- iteration 0, phase 2: the evaluation at the predictor finishes the iteration on the ORIGINAL x
    e_c, e_u = r(), r()
    before = hist.clone()
    x_out, p0 = torch.empty_like(x), torch.empty_like(x)
    hip.plms_step(x, e_c, e_u, coef, 0, hip.PLMS_FINISH, scale, hist, x_out, p0)
    ref = P.plms_step_ref(x, e_c, e_u, tab[S - 1], scale, P.FINISH, [before[0]])
    _check(x_out, ref, "x_out", "finish")
    _check(p0, ref, "pred_x0", "finish")
    assert _same(hist, before)
    xa = x.clone()
    hip.plms_step(xa, e_c, e_u, coef, 0, hip.PLMS_FINISH, scale, hist, xa, None)
    assert torch.equal(xa, x_out) and _same(hist, before)
    x = x_out
    # ---- iterations 1 .. 4: orders 2, 3, 4, 4
    for i in range(1, 5):
        e_c, e_u = r(), (r() if i != 2 else None)               # iteration 2 runs without guidance
        before = hist.clone()
        order = min(i, 3)
        olds = [before[(i - j) % 4] for j in range(1, order + 1)]
        x_out, p0 = torch.empty_like(x), torch.empty_like(x)
        hip.plms_step(x, e_c, e_u, coef, i, hip.PLMS_MULTISTEP, scale, hist, x_out, p0)
        ref = P.plms_step_ref(x, e_c, e_u, tab[S - 1 - i], scale, P.MULTISTEP, olds)
        label = f"n {n} iteration {i} order {order + 1}"
        _check(x_out, ref, "x_out", label)
        _check(p0, ref, "pred_x0", label)
        _check(hist[i % 4], ref, "e", label)
        assert _guided_bits(hist[i % 4], e_c, e_u, scale)
        for k in (1, 2, 3):                                     # the other three slots are untouched (NaN until written)
            assert _same(hist[(i + k) % 4], before[(i + k) % 4])
        if i == 1:
            assert bool(hist[2:].isnan().all())                 # order 2 read only slot 0
        if i == 2:
            assert bool(hist[3].isnan().all())
        # x_out aliasing x
        xa, ha = x.clone(), before.clone()
        hip.plms_step(xa, e_c, e_u, coef, i, hip.PLMS_MULTISTEP, scale, ha, xa, None)
        assert torch.equal(xa, x_out) and _same(ha, hist)
        # device cursor at i
        if i <= 3:
            xd, hd, pd = torch.empty_like(x), before.clone(), torch.empty_like(x)
            cursor.fill_(i)
            hip.plms_step_dev(x, e_c, e_u, coef, cursor, S, scale, hd, xd, pd)
            assert torch.equal(xd, x_out) and torch.equal(pd, p0) and _same(hd, hist)
        x = x_out
    # ---- the cursor further on, and clamped at both ends: cursor 7, 0 -> 1, S + 5 -> S - 1
    full = torch.randn(4, n, generator=g).cuda()
    e_c, e_u = r(), r()
    for cur, it in ((7, 7), (0, 1), (S + 5, S - 1)):
        hh, xh, ph = full.clone(), torch.empty_like(x), torch.empty_like(x)
        hip.plms_step(x, e_c, e_u, coef, it, hip.PLMS_MULTISTEP, scale, hh, xh, ph)
        hd, xd, pd = full.clone(), torch.empty_like(x), torch.empty_like(x)
        cursor.fill_(cur)
        hip.plms_step_dev(x, e_c, e_u, coef, cursor, S, scale, hd, xd, pd)
        assert torch.equal(xd, xh) and torch.equal(pd, ph) and torch.equal(hd, hh), (cur, it)
        assert not torch.equal(hh[it % 4], full[it % 4])
    torch.cuda.synchronize()
    # ---- refusals, by return code alone: nothing is launched for them
    wrong = {k: v for k, v in P.plms_refusals(hip.lib(), x.data_ptr(), x_out.data_ptr()).items() if v != 1}
    assert not wrong, wrong
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ the sampler against the reference's runs

@pytest.mark.parametrize("name", case_names())
def test_fixture_case_eager(name):
    _need_gpu()
    out, inter, model, case = run_case(name, device="cuda", use_graph=False, with_engine=True)
    assert len(model.calls) == case["S"] + 1                        # every evaluation called the model from Python
    check_case(out, inter, model, case)


@pytest.mark.parametrize("name", case_names(min_steps=4))
def test_fixture_case_graphed_equals_eager(name):
    _need_gpu()
    out, inter, model, case = run_case(name, device="cuda", use_graph=True, with_engine=True)
    assert len(model.calls) == 4            # iteration 0's two, iteration 1 eager, iteration 2's capture; the rest replayed
    check_case(out, inter, model, case, python_calls=4)             # S + 1 executed times, equal to the reference's
    eager, inter_e, _, _ = run_case(name, device="cuda", use_graph=False, with_engine=True)
    assert torch.equal(out, eager)
    for key in ("x_inter", "pred_x0"):
        assert len(inter[key]) == len(inter_e[key]) and all(torch.equal(a, b) for a, b in zip(inter[key], inter_e[key]))


@pytest.mark.parametrize("name", case_names(max_steps=2))
def test_fewer_than_four_steps_take_the_eager_loop(name):
    _need_gpu()
    out, inter, model, case = run_case(name, device="cuda", use_graph=True, with_engine=True)
    assert len(model.calls) == case["S"] + 1
    check_case(out, inter, model, case)


def test_a_model_without_engine_takes_the_eager_loop():
    _need_gpu()
    out, inter, model, case = run_case("S4_cfg3.0_n420", device="cuda", use_graph=True, with_engine=False)
    assert len(model.calls) == 5
    check_case(out, inter, model, case)


@pytest.mark.parametrize("name", case_names(masked=True))
def test_masked_case_on_the_gpu_takes_the_eager_loop(name):
    _need_gpu()
    out, inter, model, case = run_case(name, device="cuda", use_graph=True, with_engine=True)
    assert len(model.calls) == case["S"] + 1
    check_case(out, inter, model, case)


def test_dict_and_structurally_different_conditionings_on_the_gpu():
    _need_gpu()
    name = "S10_cfg1.0_n420"
    check_case(*run_case(name, device="cuda", use_graph=True, with_engine=True, conds="dict"), python_calls=4)
    name = "S5_cfg7.5_n512"
    for graph in (False, True):
        n_py = 4 if graph else None
        ref, _, _, case = run_case(name, device="cuda", use_graph=graph, with_engine=True)
        out, inter, model, _ = run_case(name, device="cuda", use_graph=graph, with_engine=True, conds="dict")
        check_case(out, inter, model, case, python_calls=n_py)
        assert torch.equal(out, ref)
        out2, inter2, model2, _ = run_case(name, device="cuda", use_graph=graph, with_engine=True, conds="different")
        check_case(out2, inter2, model2, case, passes=2, python_calls=n_py)
        assert torch.equal(out2, ref)


def test_p_sample_plms_on_the_gpu_gives_the_loop_s_iterations():
    """The stand-alone iteration, chained by hand with the reference's old_eps bookkeeping, is the eager loop bit for bit."""
    _need_gpu()
    from ldm.models.diffusion.plms import PLMSSampler
    name = "S5_cfg7.5_n512"
    want, _, _, case = run_case(name, device="cuda", use_graph=False, with_engine=True)
    s = PLMSSampler(P.AnalyticModel("cuda"))
    S = case["S"]
    s.make_schedule(S, verbose=False)
    x, c, uc, old = case["x_T"].cuda(), case["c"].cuda(), case["uc"].cuda(), []
    for i in range(S):
        steps = np.flip(s.ddim_timesteps)
        t, t_next = (torch.full((x.shape[0],), int(steps[j]), dtype=torch.long, device="cuda") for j in (i, min(i + 1, S - 1)))
        x, _, e = s.p_sample_plms(x, c, t, S - 1 - i, unconditional_guidance_scale=case["scale"], unconditional_conditioning=uc,
                                  old_eps=old, t_next=t_next)
        old = (old + [e])[-3:]
    assert torch.equal(x, want)


# ------------------------------------------------------------------------------ whole model

S_MODEL, SCALE_MODEL = 5, 7.5       # the smallest run that reaches the fourth order and replays twice


def _restated_plms(eps_fn, alphas_cumprod, S, x_T, scale):
    """PLMS written from the method (Liu et al., arXiv:2202.09778, eq. 12 with the transfer of eq. 11; the first step their
    pseudo improved Euler), not from the sampler class: uniform timesteps 1 + k (1000 // S), fp32 state.
    eps_fn(x, t_long, cond: bool) -> eps on x's device."""
    ac = alphas_cumprod.double()
    steps = [1 + k * (ac.shape[0] // S) for k in range(S)]
    f = lambda v: torch.tensor(float(v), dtype=torch.float32, device=x_T.device)

    def eps(x, step):
        t = torch.full((x.shape[0],), step, dtype=torch.long, device=x.device)
        e_c, e_u = eps_fn(x, t, True), eps_fn(x, t, False)
        return e_u + scale * (e_c - e_u)

    def transfer(x, e, k):
        a_t, a_prev = ac[steps[k]], (ac[steps[k - 1]] if k > 0 else ac[0])
        x0 = (x - f((1 - a_t).sqrt()) * e) / f(a_t.sqrt())
        return f(a_prev.sqrt()) * x0 + f((1 - a_prev).sqrt()) * e

    x, es = x_T, []
    for k in reversed(range(S)):
        e = eps(x, steps[k])
        if len(es) == 0:
            ep = (e + eps(transfer(x, e, k), steps[max(k - 1, 0)])) / 2
        elif len(es) == 1:
            ep = (3 * e - es[-1]) / 2
        elif len(es) == 2:
            ep = (23 * e - 16 * es[-1] + 5 * es[-2]) / 12
        else:
            ep = (55 * e - 59 * es[-1] + 37 * es[-2] - 9 * es[-3]) / 24
        es.append(e)
        x = transfer(x, ep, k)
    return x


@pytest.fixture(scope="module")
def tiny():
    """The tiny drop-in model of tests/test_gpu_dpm_solver.py, its weights for the oracle, seeded inputs, and the oracle's
    fp32 PLMS trajectory (computed once on the CPU, read by both dtype tests)."""
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
    ac = model.alphas_cumprod.detach().cpu()

    def eps_fn(x, t, c):
        with torch.no_grad():
            return R.apply_model(sd_cn, sd_un, cfg, x, t, inp["ctx"] if c else ctx_u, inp["hint_z"])

    cn, un = ({k: v.cuda() for k, v in sd.items()} for sd in (sd_cn, sd_un))

    def eps_bf16(x, t, c):      # the same oracle on the GPU under bf16 autocast: the same-precision comparator
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return R.apply_model(cn, un, cfg, x, t, cu(inp["ctx"] if c else ctx_u), cu(inp["hint_z"])).float()

    ref = _restated_plms(eps_fn, ac, S_MODEL, x_T, SCALE_MODEL)
    return dict(model=model, x_T=x_T, cond=cond, unc=unc, ref=ref, ac=ac, eps_bf16=eps_bf16)


def _plms_sample(t, use_graph):
    from ldm.models.diffusion.plms import PLMSSampler
    s = PLMSSampler(t["model"])
    s.use_graph = use_graph
    out, inter = s.sample(S_MODEL, 2, (4, 16, 16), t["cond"], verbose=False, x_T=t["x_T"].cuda(),
                          unconditional_guidance_scale=SCALE_MODEL, unconditional_conditioning=t["unc"])
    assert list(s.ddim_timesteps) == [1, 201, 401, 601, 801] and len(inter["x_inter"]) == 3
    return out


def test_whole_model_fp32_trajectory_and_graph(tiny):
    _need_gpu()
    model = tiny["model"]
    model.set_engine_dtype(torch.float32)
    graphed = _plms_sample(tiny, True)
    err = rel_l2(graphed, tiny["ref"])
    print(f"fp32 PLMS S={S_MODEL} CFG {SCALE_MODEL}: rel_l2 vs the oracle's restatement {err:.3e}")
    assert err < 5e-4
    assert torch.equal(graphed, _plms_sample(tiny, False))


def test_whole_model_bf16_deviates_like_the_bf16_oracle(tiny):
    """DESIGN 1d quotes both figures.  The comparator is the restated PLMS loop itself with the oracle's eps under bf16
    autocast (not the DDIM deviation: the fourth-order weights amplify the noise of eps more than DDIM's update does); 1.5 x is
    the margin the project gives sampled trajectories."""
    _need_gpu()
    model = tiny["model"]
    model.set_engine_dtype(torch.bfloat16)
    try:
        d_ours = rel_l2(_plms_sample(tiny, True), tiny["ref"])
    finally:
        model.set_engine_dtype(torch.float32)
    d_cmp = rel_l2(_restated_plms(tiny["eps_bf16"], tiny["ac"], S_MODEL, tiny["x_T"].cuda(), SCALE_MODEL), tiny["ref"])
    print(f"bf16 PLMS S={S_MODEL} CFG {SCALE_MODEL}: engine vs fp32 restatement {d_ours:.3e}; "
          f"bf16-autocast oracle vs fp32 restatement {d_cmp:.3e}")
    assert d_ours <= 1.5 * d_cmp, (d_ours, d_cmp)


# ------------------------------------------------------------------------------ scripts/sample.py --sampler plms

def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_sample_script_plms_end_to_end_and_default_unchanged(tmp_path, monkeypatch):
    """`--sampler plms` writes a finite, non-constant image through the real first stage that differs from DDIM's; without
    the flag main() writes the bytes that DDIMSampler through sample_dataset -- the script as it was -- writes."""
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
    # A freshly built UNet ends in a zero-initialised convolution: eps == 0 at every step, and with an eps that does not
    # change from step to step every Adams-Bashforth combination IS that eps, so PLMS would write DDIM's bytes.  Give the
    # checkpoint an output layer that answers to its input.
    out_conv = model.model.diffusion_model.out[-1]
    assert float(out_conv.weight.abs().max()) == 0.0
    with torch.no_grad():
        out_conv.weight.normal_(0.0, 0.05)
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
    sample.main(argv("plms", "--sampler", "plms"))
    png = lambda d: open(glob.glob(str(tmp_path / d / "sample" / "*.png"))[0], "rb").read()
    assert png("ddim") == png("was")
    assert png("plms") != png("ddim")
    from PIL import Image
    img = np.asarray(Image.open(glob.glob(str(tmp_path / "plms" / "sample" / "*.png"))[0]))
    assert img.shape[-1] == 3 and np.isfinite(img.astype(np.float64)).all() and img.std() > 0, "the sampled image is constant"
    assert open(tmp_path / "plms" / "prompt.txt").read().count("\n") == 1
