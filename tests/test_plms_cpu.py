"""PLMS sampler (ldm/models/diffusion/plms.py) on CPU tensors: the loop, its bookkeeping and its intermediates against runs
of the UNMODIFIED reference (tests/golden/plms.pt) through the plain-torch update that tensors outside the engine take; the
public surface (parameter names, refusals, conditionings, p_sample_plms, scripts/sample.py's flag); and a CPU model of the
arithmetic of cl_plms_step under the element-wise gate the GPU test applies.  The fused kernel and the graphed loop are checked
on the GPU (tests/test_gpu_plms.py)."""
import importlib.util
import inspect
import os

import pytest
import torch

from tests import plms_cases as P
from tests.plms_cases import AnalyticModel, case_names, check_case, fixture, run_case
from tests.util import ROOT, rel_l2


@pytest.mark.parametrize("name", case_names())
def test_fixture_case_on_cpu(name):
    """rel-L2 < 1e-5 against the reference's result and every kept intermediate; the S + 1 model times and batch sizes (2B
    under guidance, B otherwise) are the reference's exactly."""
    check_case(*run_case(name))


def test_the_fixture_covers_the_start_up_orders_and_the_masked_case():
    steps = sorted({fixture()["cases"][k]["S"] for k in case_names()})
    assert steps == [1, 2, 4, 5, 10, 20, 50]
    assert {fixture()["cases"][k]["scale"] for k in case_names()} == {7.5, 3.0, 1.0}
    assert fixture()["cases"]["S20_cfg7.5_n512"]["times"][:4] == [951, 901, 901, 851]
    assert fixture()["cases"]["S1_cfg7.5_n420"]["times"] == [1, 1]
    assert len(case_names(masked=True)) == 1


@pytest.mark.parametrize("name", case_names(masked=True))
def test_masked_case_on_cpu(name):
    out, inter, model, case = run_case(name)
    check_case(out, inter, model, case)
    keep = case["mask"].expand_as(out) == 0          # the sampled half differs from x0, so the mask acted
    assert rel_l2(out[keep], case["x0"][keep]) > 0.1


def test_sample_has_the_reference_parameter_names_and_the_loop_switches():
    from ldm.models.diffusion.plms import PLMSSampler
    assert list(inspect.signature(PLMSSampler.sample).parameters) == fixture()["sample_params"]
    s = PLMSSampler(AnalyticModel())
    assert (s.use_graph, s.batch_cfg, s.hoist_hint_encode) == (True, True, True)
    for fn in ("make_schedule", "plms_sampling", "p_sample_plms"):
        assert callable(getattr(s, fn))


def test_unsupported_settings_raise():
    from ldm.models.diffusion.plms import PLMSSampler
    x, c = torch.zeros(1, 4, 2, 2), torch.ones(1)
    run = lambda **kw: PLMSSampler(AnalyticModel()).sample(4, 1, (4, 2, 2), c, verbose=False, x_T=x, **kw)
    run()
    with pytest.raises(ValueError, match="ddim_eta must be 0 for PLMS"):
        run(eta=0.1)
    for kw in (dict(quantize_x0=True), dict(score_corrector=object()), dict(dynamic_threshold=0.9)):
        with pytest.raises(NotImplementedError):
            run(**kw)
    s = PLMSSampler(AnalyticModel())
    s.make_schedule(4, verbose=False)
    with pytest.raises(NotImplementedError):
        s.plms_sampling(c, (1, 4, 2, 2), x_T=x, ddim_use_original_steps=True)
    v = AnalyticModel()
    v.parameterization = "v"
    with pytest.raises(NotImplementedError):
        PLMSSampler(v).sample(4, 1, (4, 2, 2), c, verbose=False, x_T=x)
    run(temperature=0.5, noise_dropout=0.3)            # accepted: eta = 0 leaves them nothing to act on


def test_dict_and_structurally_different_conditionings_give_the_tensor_result():
    name = "S10_cfg1.0_n420"
    check_case(*run_case(name, conds="dict"))          # no guidance: one pass of B whatever the structure
    name = "S5_cfg7.5_n512"
    ref, _, _, case = run_case(name)
    out, inter, model, _ = run_case(name, conds="dict")
    check_case(out, inter, model, case)
    assert torch.equal(out, ref)
    out2, inter2, model2, _ = run_case(name, conds="different")
    check_case(out2, inter2, model2, case, passes=2)
    assert torch.equal(out2, ref)            # samples are independent: two passes of B are the batch of 2B


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_p_sample_plms_stand_alone_against_fp64(k):
    """One iteration with a history of k earlier eps on row 7 of a 10-step table, against the method in fp64."""
    from ldm.models.diffusion.plms import PLMSSampler
    model = AnalyticModel()
    s = PLMSSampler(model)
    s.make_schedule(10, verbose=False)
    g = torch.Generator().manual_seed(40 + k)
    x = torch.randn(2, 4, 5, 7, generator=g)
    old = [0.3 * torch.randn(2, 4, 5, 7, generator=g) for _ in range(k)]
    c, uc, scale, index = torch.full((2,), 1.0), torch.full((2,), 0.6), 7.5, 7
    t = torch.full((2,), int(s.ddim_timesteps[index]), dtype=torch.long)
    t_next = torch.full((2,), int(s.ddim_timesteps[index - 1]), dtype=torch.long)
    x_prev, pred_x0, e_t = s.p_sample_plms(x, c, t, index, unconditional_guidance_scale=scale, unconditional_conditioning=uc,
                                           old_eps=list(old), t_next=t_next)
    assert model.calls == ([4, 4] if k == 0 else [4]) and len(old) == k

    def eps64(x_, t_):
        f = lambda cc: torch.tanh(0.7 * x_ + 0.001 * float(t_[0])) * cc
        return f(0.6) + scale * (f(1.0) - f(0.6))

    row = [float(v) for v in s.coef_table[index]]

    def upd64(x_, e_):
        p0 = (x_ - row[3] * e_) / row[0] ** 0.5
        return row[1] ** 0.5 * p0 + (1.0 - row[1] - row[2] ** 2) ** 0.5 * e_, p0

    x64, o = x.double(), [v.double() for v in old]
    e = eps64(x64, t)
    if k == 0:
        ep = (e + eps64(upd64(x64, e)[0], t_next)) / 2
    elif k == 1:
        ep = (3 * e - o[-1]) / 2
    elif k == 2:
        ep = (23 * e - 16 * o[-1] + 5 * o[-2]) / 12
    else:
        ep = (55 * e - 59 * o[-1] + 37 * o[-2] - 9 * o[-3]) / 24
    want_x, want_p = upd64(x64, ep)
    errs = rel_l2(x_prev, want_x), rel_l2(pred_x0, want_p), rel_l2(e_t, e)
    print(f"history {k}: rel_l2 x_prev {errs[0]:.2e} pred_x0 {errs[1]:.2e} e_t {errs[2]:.2e}")
    assert max(errs) < 2e-6, errs


def test_sample_script_accepts_plms_and_defaults_to_ddim():
    spec = importlib.util.spec_from_file_location("sample", os.path.join(ROOT, "scripts", "sample.py"))
    sample = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sample)
    base = ["--dataroot", "d", "--config", "c", "--ckpt", "k", "--save_dir", "s"]
    assert sample.get_parser().parse_args(base).sampler == "ddim"
    assert sample.get_parser().parse_args(base + ["--sampler", "plms"]).sampler == "plms"
    assert sample.get_parser().parse_args(base + ["--sampler", "dpm"]).sampler == "dpm"
    from ldm.models.diffusion.plms import PLMSSampler
    assert isinstance(sample.make_sampler(AnalyticModel(), "plms"), PLMSSampler)
    assert type(sample.make_sampler(AnalyticModel())).__name__ == "DDIMSampler"


def test_kernel_refusals_are_decided_on_the_host():
    """Return code 1 for everything include/ctrlora_hip.h lists, with host addresses and no GPU: nothing is launched (the
    launch record stays empty), and an empty call is CL_OK without a launch either."""
    import ctypes
    from ctrlora_amd import build, hip
    build.build(verbose=False)
    L = hip.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    wrong = {k: v for k, v in P.plms_refusals(L, p, p + 64).items() if v != 1}
    assert not wrong, wrong
    out = (ctypes.c_int * 8)(*([7] * 8))
    assert L.cl_debug_ew_last_launch(out) == 0 and list(out) == [0] * 8
    assert L.cl_plms_step(p, p, None, p, 1, 4, 0, 7.5, p, p, None, 0, None) == 0
    assert L.cl_plms_step(p, p, None, p, 0, 1, 2, 7.5, p, p, None, 0, None) == 0          # finish may alias
    assert L.cl_plms_step_dev(p, p, None, p, p, 2, 7.5, p, p, None, 0, None) == 0
    assert hip.lib().cl_abi_version() == 7 and (hip.PLMS_MULTISTEP, hip.PLMS_START, hip.PLMS_FINISH) == (0, 1, 2)
    assert "cl_plms_step" in hip.EXPORTED and "cl_plms_step_dev" in hip.EXPORTED


# ------------------------------------------------------------------------------ the arithmetic of cl_plms_step, on the CPU

def _kernel_cases():
    """(label, x, e_c, e_u, row, scale, phase, olds) over every row of a 20-step table: the three phases, the three multistep
    orders, with and without guidance, n = 420."""
    from ldm.models.diffusion.plms import PLMSSampler
    s = PLMSSampler(AnalyticModel())
    s.make_schedule(20, verbose=False)
    g = torch.Generator().manual_seed(9)
    r = lambda: torch.randn(420, generator=g)
    for index in range(20):
        row = s.coef_table[index]
        for phase, order in ((P.START, 0), (P.FINISH, 1), (P.MULTISTEP, 1), (P.MULTISTEP, 2), (P.MULTISTEP, 3)):
            for guided in (True, False):
                yield (f"row {index} phase {phase} order {order} guided {guided}", r(), r(), r() if guided else None, row, 7.5,
                       phase, [r() for _ in range(order)])


def test_fp32_model_of_the_kernel_stays_inside_the_gate():
    """|fp32 - fp64| <= 16 * 2^-24 * mag element-wise with zero violations, for every output of every phase and order.  16
    counts the fp32 roundings on the longest path (x_out of a fourth-order step): guidance 3 (difference, product, sum), the
    multistep sum 5 (a product, three sums, the division), pred_x0 4 (sqrt(a_t), the product with sqrt(1 - a_t), the
    difference, the quotient), x_prev 3 (sqrt(a_prev), the product, the sum) = 15, and one to spare for the direction
    coefficient's own two roundings entering through the shorter branch.  Derived, not measured."""
    worst = 0.0
    for label, x, e_c, e_u, row, scale, phase, olds in _kernel_cases():
        ref = P.plms_step_ref(x, e_c, e_u, row, scale, phase, olds)
        got = P.plms_step_ref(x, e_c, e_u, row, scale, phase, olds, dtype=torch.float32)
        for key in ("e", "x_out", "pred_x0"):
            bad, ratio = P.violations(got[key], ref, key)
            assert bad == 0, (label, key, bad, ratio)
            worst = max(worst, ratio)
    print(f"largest |err| / bound over the table: {worst:.3f}")
    assert worst < 1.0


def test_the_gate_catches_wrong_forms():
    """Third-order weights at the fourth order, and a finishing phase that took e_n for the stored e (what a phase 2 that wrote
    e_n into the history would compute from then on), both fall outside the gate in most elements."""
    wrong_ab = dict(P.AB)
    wrong_ab[3] = ((23., -16., 5., 0.), 12.)
    caught = {"ab": 0, "finish": 0}
    for label, x, e_c, e_u, row, scale, phase, olds in _kernel_cases():
        ref = P.plms_step_ref(x, e_c, e_u, row, scale, phase, olds)
        if phase == P.MULTISTEP and len(olds) == 3:
            got = P.plms_step_ref(x, e_c, e_u, row, scale, phase, olds, dtype=torch.float32, weights=wrong_ab)
            assert P.violations(got["x_out"], ref, "x_out")[0] > 0.9 * x.numel(), label
            caught["ab"] += 1
        if phase == P.FINISH:
            e_n = P.plms_step_ref(x, e_c, e_u, row, scale, P.START, [], dtype=torch.float32)["e"]
            got = P.plms_step_ref(x, e_c, e_u, row, scale, phase, [e_n], dtype=torch.float32)       # hist[0] overwritten by e_n
            assert P.violations(got["x_out"], ref, "x_out")[0] > 0.9 * x.numel(), label
            caught["finish"] += 1
    assert caught == {"ab": 40, "finish": 40}
