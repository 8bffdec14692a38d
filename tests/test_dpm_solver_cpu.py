"""DPM-Solver++ sampler (ldm/models/diffusion/dpm_solver) on CPU tensors: the coefficient table and the loop bookkeeping
against runs of the UNMODIFIED reference (tests/golden/dpm_solver.pt), through the plain-torch update that tensors outside
the engine take.  The fused kernel, the graphed loop and the float timestep embedding are checked on the GPU
(tests/test_gpu_dpm_solver.py)."""
import inspect

import pytest
import torch

from tests.dpm_solver_cases import AnalyticModel, case_names, check_case, fixture, run_case


@pytest.mark.parametrize("name", case_names())
def test_fixture_case_on_cpu(name):
    """rel-L2 < 1e-5 against the reference's result, its model times within two fp32 ulps at 1000, its batch sizes (2B
    under guidance, B otherwise)."""
    out, model, case = run_case(name)
    check_case(out, model, case)


def test_sample_has_the_reference_parameter_names():
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    assert list(inspect.signature(DPMSolverSampler.sample).parameters) == fixture()["sample_params"]
    s = DPMSolverSampler(AnalyticModel())
    assert (s.order, s.skip_type, s.use_graph, s.batch_cfg, s.hoist_hint_encode) == (2, "time_uniform", True, True, True)


def test_step_orders_follow_start_up_and_lower_order_final():
    from ldm.models.diffusion.dpm_solver.sampler import dpmpp_table
    ac = fixture()["alphas_cumprod"]
    assert dpmpp_table(ac, 8, 3)[2] == [1, 2, 3, 3, 3, 3, 2, 1]
    assert dpmpp_table(ac, 4, 2)[2] == [1, 2, 2, 1]
    assert dpmpp_table(ac, 15, 3)[2] == [1, 2] + [3] * 13          # 15 steps and more: no lower-order finish
    t, tab, _ = dpmpp_table(ac, 20, 2)
    assert t[0] == 1.0 and abs(t[-1] - 1e-3) < 1e-15 and tab.shape == (20, 8)
    assert abs(tab[1, 6] - 949.05) < 1e-9 and tab[0, 6] == 999.0
    # a term that is not part of the step has a coefficient of exactly zero: the kernel does not read its history slot
    assert tab[0, 4] == 0.0 and tab[0, 5] == 0.0 and (tab[1:, 4] != 0).all() and (tab[:, 5] == 0).all()


def test_dict_and_structurally_different_conditionings_give_the_tensor_result():
    name = "sampler_S10_cfg7.5_n512"
    ref, _, case = run_case(name)
    out, model, _ = run_case(name, conds="dict")
    check_case(out, model, case)
    assert torch.equal(out, ref)
    out2, model2, _ = run_case(name, conds="different")
    check_case(out2, model2, case, passes=2)
    assert torch.equal(out2, ref)            # samples are independent: two passes of B are the batch of 2B


def test_unsupported_settings_raise():
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    x = torch.zeros(1, 4, 2, 2)
    c = torch.ones(1)

    def run(S, **attrs):
        s = DPMSolverSampler(AnalyticModel())
        for k, v in attrs.items():
            setattr(s, k, v)
        return s.sample(S, 1, (4, 2, 2), c, verbose=False, x_T=x)

    with pytest.raises(NotImplementedError):
        run(10, skip_type="logSNR")
    with pytest.raises(ValueError):
        run(10, skip_type="bogus")
    with pytest.raises(ValueError):
        run(10, order=4)
    with pytest.raises(ValueError):
        run(2, order=3)
    run(3, order=3)
