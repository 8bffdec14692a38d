"""Masked sampling / img2img without a GPU: the rounding model of cl_qsample_blend against torch's q_sample-then-blend on the
CPU (bit for bit, all four mask layouts) with negative controls, the fp64 contract's gate on that model, the sampler's eager
masked loop against the UNMODIFIED reference's runs (tests/golden/ddim_edit.pt), the host rules of api's editing modes, and the
C-ABI entry with its ctypes signature."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import ddim_edit_ref as R

SHAPES = ((1, 1, (1,)), (3, 4, (35,)), (2, 4, (8, 8)), (3, 4, (5, 7)))


@pytest.mark.parametrize("per_b,per_c", R.LAYOUTS)
def test_rounding_model_is_torch_qsample_then_blend_bit_for_bit(per_b, per_c):
    """Every op rounded once IS what torch's separate elementwise ops give; a contracted sum or an unrounded 1 - m is not."""
    differs = {"fma": 0, "one_minus": 0}
    for n, (B, C, hw) in enumerate(SHAPES):
        o = R.make_operands(B, C, hw, per_b, per_c, seed=100 + n)
        want = R.torch_blend(o)
        args = (o["x0"], o["noise"], o["t"], o["sqrt_ac"], o["sqrt_1mac"], o["mask"], o["x"])
        got = R.blend_model32(*args)
        assert got.dtype == torch.float32 and torch.equal(got, want), (B, C, hw)
        ref, mag = R.blend_ref(*args)
        bad, ratio = R.violations(got, ref, mag)
        assert bad == 0 and ratio <= 1.0, (bad, ratio)
        for control in differs:
            differs[control] += int((R.blend_model32(*args, control=control) != want).sum())
    print("elements the negative controls change:", differs)
    assert differs["fma"] > 0 and differs["one_minus"] > 0


def test_contract_clamps_the_time_and_broadcasts_the_mask():
    o = R.make_operands(3, 4, (5, 7), True, False, seed=7)
    args = lambda t: (o["x0"], o["noise"], t, o["sqrt_ac"], o["sqrt_1mac"], o["mask"], o["x"])
    inside, _ = R.blend_ref(*args(torch.tensor([0, 999, 999])))
    outside, _ = R.blend_ref(*args(torch.tensor([-5, 1000, 123456])))
    assert torch.equal(inside, outside)
    # mask 1 keeps q_sample(x0), mask 0 keeps x
    ones, zeros = torch.ones_like(o["mask"]), torch.zeros_like(o["mask"])
    q = R.torch_blend({**o, "mask": ones})
    assert torch.equal(R.blend_model32(o["x0"], o["noise"], o["t"], o["sqrt_ac"], o["sqrt_1mac"], ones, o["x"]), q)
    assert torch.equal(R.blend_model32(o["x0"], o["noise"], o["t"], o["sqrt_ac"], o["sqrt_1mac"], zeros, o["x"]), o["x"])


def test_q_noise_reaches_q_sample_only_when_it_is_set():
    """The eager loop (a CPU latent always takes it) calls model.q_sample(x0, ts) as it always did while q_noise is None, and
    q_sample(x0, ts, noise=q_noise) once the attribute is set.  The model stops the run at that call: the fused update that
    would follow is a HIP kernel."""
    from cldm.ddim_hacked import DDIMSampler
    case = R.fixture()["cases"][R.case_names()[0]]
    seen = []

    class Model(R.AnalyticModel):
        def q_sample(self, x_start, t, **kw):
            seen.append(dict(kw))
            raise StopIteration

    s = DDIMSampler(Model())
    assert s.q_noise is None
    kw = dict(verbose=False, x_T=case["x_T"], eta=0.0, unconditional_guidance_scale=case["scale"],
              unconditional_conditioning=case["uc"], mask=case["mask"], x0=case["x0"])
    with pytest.raises(StopIteration):
        s.sample(case["S"], case["x_T"].shape[0], tuple(case["x_T"].shape[1:]), case["c"], **kw)
    s.q_noise = case["q_noise"]
    with pytest.raises(StopIteration):
        s.sample(case["S"], case["x_T"].shape[0], tuple(case["x_T"].shape[1:]), case["c"], **kw)
    assert seen[0] == {} and list(seen[1]) == ["noise"] and seen[1]["noise"] is case["q_noise"]


def test_fixture_holds_the_cases_the_gpu_suite_needs():
    cases = R.fixture()["cases"]
    assert {(v["S"], v["scale"]) for v in cases.values()} == {(S, c) for S in (4, 10, 20) for c in (1.0, 7.5)}
    shapes = {(tuple(v["x_T"].shape), tuple(v["mask"].shape)) for v in cases.values()}
    assert shapes == {((2, 4, 8, 8), (2, 1, 8, 8)), ((2, 4, 8, 8), (1, 1, 8, 8)), ((3, 4, 5, 7), (3, 1, 5, 7)), ((3, 4, 5, 7), (1, 1, 5, 7))}
    for v in cases.values():
        assert set(v["mask"].unique().tolist()) == {0.0, 1.0} and len(v["times"]) == v["S"] * (1 if v["scale"] == 1.0 else 2)


def test_mask_replayable_rule():
    """Which masked runs may enter the replayed loop, decided on shapes and attributes alone (devices mocked by a CPU run:
    a CPU tensor never qualifies)."""
    from cldm.ddim_hacked import DDIMSampler
    s = DDIMSampler(R.AnalyticModel())
    img = torch.zeros(2, 4, 8, 8)
    assert not s._mask_replayable(torch.ones(2, 1, 8, 8), torch.zeros(2, 4, 8, 8), img)      # CPU tensors: the eager loop
    assert not s._mask_replayable(torch.ones(2, 1, 8, 8), None, img)
    assert s._q_tables() is None                                                              # CPU tables do not qualify


# ------------------------------------------------------------------------------------------------ api host logic

def test_api_latent_mask_rule():
    import api
    mk = np.zeros((16, 24), np.uint8)
    mk[3, 9] = 255               # one marked pixel marks its whole 8 x 8 cell (0, 1)
    mk[8:16, 16:24] = 1          # any non-zero value marks
    keep = api.latent_keep_mask(mk, 2, 3)
    assert keep.shape == (1, 1, 2, 3) and keep.dtype == torch.float32
    assert keep[0, 0].tolist() == [[1.0, 0.0, 1.0], [1.0, 1.0, 0.0]]                          # 1 = keep
    assert float(api.latent_keep_mask(np.zeros((16, 24), np.uint8), 2, 3).min()) == 1.0
    with pytest.raises(ValueError):
        api.latent_keep_mask(mk, 2, 2)
    with pytest.raises(ValueError):
        api.latent_keep_mask(mk.astype(np.float32), 2, 3)
    with pytest.raises(ValueError):
        api.latent_keep_mask(np.zeros((16, 24, 3), np.uint8), 2, 3)


def test_api_t_enc_rule_and_argument_errors():
    import api
    assert api.img2img_steps(0.6, 20) == 12 and api.img2img_steps(0.999, 20) == 19 and api.img2img_steps(0.5, 50) == 25
    assert api.img2img_steps(0.05, 20) == 1
    with pytest.raises(ValueError):
        api.img2img_steps(0.04, 20)                      # int(0.8) == 0: no step to run
    img, mk = np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8), np.uint8)
    assert api.check_edit_args(None, 1.0, None) == "plain" and api.check_edit_args(img, 1.0, None) == "plain"
    assert api.check_edit_args(img, 0.5, None) == "img2img" and api.check_edit_args(img, 1.0, mk) == "masked"
    for bad in ((img, 0.5, mk), (None, 1.0, mk), (None, 0.5, None), (img, 0.0, None), (img, 1.5, None)):
        with pytest.raises(ValueError):
            api.check_edit_args(*bad)
    a = np.arange(10 * 12 * 3, dtype=np.uint8).reshape(10, 12, 3)
    assert np.array_equal(api.center_crop_to(a, 8, 8), a[1:9, 2:10])
    with pytest.raises(ValueError):
        api.center_crop_to(a, 16, 8)
    assert api.load_image(a[:, :, 0]).shape == (10, 12, 3)


def test_api_signatures_append_the_editing_arguments_with_inert_defaults():
    import api
    want = [("init_image", None), ("strength", 1.0), ("mask_image", None), ("composite", True)]
    for fn in (api.CtrLoRA.sample, api.CtrLoRA.sample_1lora, api.CtrLoRA.sample_2loras, api.CtrLoRA._run):
        ps = list(inspect.signature(fn).parameters.values())[-4:]
        assert [(p.name, p.default) for p in ps] == want, fn.__name__


def test_sample_script_init_strength_flag_defaults_to_off():
    import importlib.util
    import os
    from tests.util import ROOT
    spec = importlib.util.spec_from_file_location("sample_cli", os.path.join(ROOT, "scripts", "sample.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    base = ["--dataroot", "d", "--config", "c", "--ckpt", "k", "--save_dir", "s"]
    assert mod.get_parser().parse_args(base).init_strength == 1.0
    assert mod.get_parser().parse_args(base + ["--init_strength", "0.5"]).init_strength == 0.5


# ------------------------------------------------------------------------------------------------ the C-ABI entry

def test_qsample_blend_is_declared_exported_and_bound():
    from ctrlora_amd import build, hip
    assert "cl_qsample_blend" in hip.EXPORTED
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert hip._SIGS["cl_qsample_blend"] == [P, P, P, P, P, I, P, I, I, P, P, I, I, L, P]
    lib = ctypes.CDLL(build.build(verbose=False))
    assert hasattr(lib, "cl_qsample_blend") and lib.cl_abi_version() == 7
    # refusals are decided on the host: no device is needed to see them
    fn = lib.cl_qsample_blend
    fn.argtypes = hip._SIGS["cl_qsample_blend"]
    assert fn(None, None, None, None, None, 1000, None, 1, 1, None, None, 2, 4, 8, None) == 1          # null pointers
    assert fn(None, None, None, None, None, 1000, None, 1, 1, None, None, 0, 4, 8, None) == 0          # B == 0: nothing to do
    assert fn(None, None, None, None, None, 0, None, 1, 1, None, None, 0, 4, 8, None) == 1             # T < 1
    with pytest.raises(ValueError):
        z = torch.zeros(2, 4, 8, 8)
        hip.qsample_blend(z, z, torch.zeros(2, dtype=torch.long), torch.zeros(10), torch.zeros(10), torch.zeros(2, 2, 8, 8), z, z)
