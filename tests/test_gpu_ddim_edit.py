"""Masked sampling, DDIM inversion and img2img on the replayed DDIM loop, on the MI355X (run with -m gpu).

  1. cl_qsample_blend element-wise against its fp64 contract (|got - ref| <= 6 * 2^-24 * mag, zero violations: derived in
     tests/ddim_edit_ref.py), bit-equal to cl_qsample followed by the three torch ops, with canary guards, the launch record and
     every refusal;
  2. DDIMSampler.sample(mask=, x0=) against runs of the UNMODIFIED reference (tests/golden/ddim_edit.pt): the eager loop within
     ENC_TOL = 1e-5, the replayed loop with the bits of the eager loop and 2 Python-level steps;
  3. the whole tiny fp32 model: masked sample / decode / encode replayed against eager, torch.equal; reuse_graph; seeds;
  4. api.CtrLoRA end to end on the tiny model: img2img, a masked run with and without compositing, inert defaults.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import ddim_edit_ref as R
from tests import ew_ref
from tests.util import ROOT

pytestmark = pytest.mark.gpu

GUARD = 64                  # floats on either side of an output (a multiple of 4: the view keeps the buffer's alignment)
PATTERN = -7.25


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ctrlora_amd import hip
    hip.lib()           # raises if the HIP library is missing: no silent fallback
    return hip


def _probe(hip):
    out = (ctypes.c_int * 8)()
    assert hip.lib().cl_debug_ew_last_launch(out) == 0
    return dict(zip(ew_ref.PROBE_FIELDS, list(out)))


def _ew_id(name):
    """The value of an EW_* enumerator of csrc/elementwise.h (the enum counts from 1)."""
    src = open(os.path.join(ROOT, "ctrlora_amd", "csrc", "elementwise.h")).read()
    body = re.search(r"enum \{(.*?)\};", src, flags=re.S).group(1)
    names = [w.split("=")[0].strip() for w in body.replace("\n", " ").split(",") if w.strip()]
    return names.index(name) + 1


class _Canary:
    """A contiguous fp32 output of `shape` inside a buffer of a fixed pattern; `shift` floats move it off 16-byte alignment."""

    def __init__(self, shape, shift=0, init=None):
        n = int(np.prod(shape))
        self.buf = torch.full((2 * GUARD + n + shift,), PATTERN, device="cuda")
        self.lo, self.hi = GUARD + shift, GUARD + shift + n
        self.view = self.buf[self.lo:self.hi].view(*shape)
        self.view.copy_(init) if init is not None else self.view.fill_(float("nan"))

    def guards_intact(self):
        return bool((self.buf[:self.lo] == PATTERN).all()) and bool((self.buf[self.hi:] == PATTERN).all())


def _shifted(t, shift):
    """A contiguous copy of t that starts `shift` floats past an aligned address."""
    buf = torch.empty(t.numel() + shift, device="cuda", dtype=t.dtype)
    v = buf[shift:].view(t.shape)
    v.copy_(t)
    return v


# (name, B, C, hw, pointer shift in floats, expected form): the single element, HW % 4 != 0 (scalar), the vector form, the vector
# shape at a misaligned pointer (scalar), and a size whose grid-stride loop iterates twice in the vector form
KERNEL_SHAPES = (("1x1x1", 1, 1, (1,), 0, 0), ("3x4x35", 3, 4, (35,), 0, 0), ("2x4x64", 2, 4, (64,), 0, 1),
                 ("2x4x64-misaligned", 2, 4, (64,), 1, 0), ("wrap", 2, 4, (4 * (ew_ref.WRAP // 8) + 4 * 77,), 0, 1))


@pytest.mark.parametrize("name,B,C,hw,shift,form", KERNEL_SHAPES, ids=[s[0] for s in KERNEL_SHAPES])
def test_qsample_blend_against_fp64_torch_bits_canary_and_record(name, B, C, hw, shift, form):
    hip = _need_gpu()
    n = B * C * int(np.prod(hw))
    assert ew_ref.wraps(n // 4 if form else n) == (name == "wrap")
    worst = 0.0
    for k, (per_b, per_c) in enumerate(R.LAYOUTS):
        o = R.make_operands(B, C, hw, per_b, per_c, seed=500 + k)
        # a time per sample; the last sample's (and, alone, the only one's) lies outside the table on alternating sides
        o["t"][-1] = (1000 + 37) if k % 2 else -3
        d = {key: v.cuda() for key, v in o.items()}
        if shift:
            d["x0"] = _shifted(d["x0"], shift)              # one misaligned operand is enough to force the scalar form
        ref, mag = R.blend_ref(o["x0"], o["noise"], o["t"], o["sqrt_ac"], o["sqrt_1mac"], o["mask"], o["x"])
        out = _Canary(o["x"].shape)
        before = {key: v.clone() for key, v in d.items()}
        got = hip.qsample_blend(d["x0"], d["noise"], d["t"], d["sqrt_ac"], d["sqrt_1mac"], d["mask"], d["x"], out.view)
        rec = _probe(hip)
        torch.cuda.synchronize()
        bad, ratio = R.violations(got, ref, mag)
        worst = max(worst, ratio)
        assert bad == 0, (name, per_b, per_c, bad, ratio)
        assert out.guards_intact() and not bool(torch.isnan(out.view).any())
        assert all(torch.equal(d[key], before[key]) for key in d)
        # the record: id, form, the two mask flags (a dimension of size 1 is broadcast), the grid of ew_grid
        want_aux = int(o["mask"].shape[0] != 1) | (int(o["mask"].shape[1] != 1) << 1)
        assert rec["id"] == _ew_id("EW_QSAMPLE_BLEND") and rec["form"] == form and rec["aux"] == want_aux, rec
        assert (rec["gx"], rec["gy"], rec["gz"], rec["threads"], rec["dtype"]) == (ew_ref.ew_grid(n // 4 if form else n), 1, 1, 256, -1)
        # the bits of cl_qsample followed by the three torch ops, with the time clamped as the kernel clamps it
        tc = d["t"].clamp(0, 999)
        q = hip.qsample(d["x0"].contiguous(), d["noise"], tc, d["sqrt_ac"], d["sqrt_1mac"], torch.empty_like(d["x"]))
        eager = q * d["mask"] + (1. - d["mask"]) * d["x"]
        assert torch.equal(got, eager), (name, per_b, per_c, int((got != eager).sum()))
        assert torch.equal(got.cpu(), R.blend_model32(o["x0"], o["noise"], o["t"], o["sqrt_ac"], o["sqrt_1mac"], o["mask"], o["x"]))
        # out aliasing x: in place, the same bits, guards intact
        inplace = _Canary(o["x"].shape, init=d["x"])
        hip.qsample_blend(d["x0"], d["noise"], d["t"], d["sqrt_ac"], d["sqrt_1mac"], d["mask"], inplace.view, inplace.view)
        torch.cuda.synchronize()
        assert torch.equal(inplace.view, got) and inplace.guards_intact()
    print(f"{name}: largest |err| / (6 * 2^-24 * mag) over the four mask layouts {worst:.3f}")


def test_qsample_blend_misaligned_output_takes_the_scalar_form():
    hip = _need_gpu()
    o = R.make_operands(2, 4, (64,), True, False, seed=77)
    d = {key: v.cuda() for key, v in o.items()}
    out = _Canary(o["x"].shape, shift=3)
    got = hip.qsample_blend(d["x0"], d["noise"], d["t"], d["sqrt_ac"], d["sqrt_1mac"], d["mask"], d["x"], out.view)
    rec = _probe(hip)
    torch.cuda.synchronize()
    assert rec["form"] == 0 and out.guards_intact()
    assert torch.equal(got.cpu(), R.torch_blend(o))


def test_qsample_blend_refusals_launch_and_write_nothing():
    hip = _need_gpu()
    L = hip.lib()
    bufs = [_Canary((1024,)) for _ in range(3)]
    for b in bufs:
        b.view.fill_(PATTERN)
    p, q, r = (b.view.data_ptr() + 1024 for b in bufs)            # 256 floats in: room on both sides for the overlap rows
    # a good launch first, so that the record holds something a refusal has to clear
    o = {key: v.cuda() for key, v in R.make_operands(2, 4, (8,), True, True, seed=1).items()}
    hip.qsample_blend(o["x0"], o["noise"], o["t"], o["sqrt_ac"], o["sqrt_1mac"], o["mask"], o["x"], torch.empty_like(o["x"]))
    assert _probe(hip)["id"] == _ew_id("EW_QSAMPLE_BLEND")
    wrong = {k: v for k, v in R.blend_refusals(L, p, q, r).items() if v != 1}
    assert not wrong, wrong
    assert _probe(hip) == dict(zip(ew_ref.PROBE_FIELDS, [0] * 8))            # a refused call leaves id = 0
    assert L.cl_qsample_blend(None, None, None, None, None, 1000, None, 1, 1, None, None, 0, 4, 8, None) == 0      # B == 0
    assert _probe(hip)["id"] == 0
    torch.cuda.synchronize()
    assert all(bool((b.buf == PATTERN).all()) for b in bufs)
    z = torch.zeros(2, 4, 8, 8, device="cuda")
    with pytest.raises(ValueError):
        hip.qsample_blend(z, z, torch.zeros(2, dtype=torch.long, device="cuda"), o["sqrt_ac"], o["sqrt_1mac"],
                          torch.zeros(2, 2, 8, 8, device="cuda"), z, torch.empty_like(z))
    with pytest.raises(hip.HipError):                            # out aliasing x0 through the binding
        hip.qsample_blend(z, z.clone(), torch.zeros(2, dtype=torch.long, device="cuda"), o["sqrt_ac"], o["sqrt_1mac"],
                          torch.zeros(1, 1, 8, 8, device="cuda"), z.clone(), z)


# ------------------------------------------------------------------------------ the sampler against the reference's runs

@pytest.fixture(scope="module")
def eager_runs():
    """Every fixture case through the eager loop on the GPU, once: read by the tests below and left unchanged."""
    _need_gpu()
    return {name: R.run_case(name, device="cuda", use_graph=False, with_engine=True) for name in R.case_names()}


@pytest.mark.parametrize("name", R.case_names())
def test_fixture_case_eager(name, eager_runs):
    out, inter, model, case = eager_runs[name]
    R.check_case(out, inter, model, case)                    # prints the measured worst rel_l2


@pytest.mark.parametrize("name", R.case_names(min_steps=4))
def test_fixture_case_replayed_gives_the_bits_of_the_eager_loop(name, eager_runs):
    out, inter, model, case = R.run_case(name, device="cuda", use_graph=True, with_engine=True)
    R.check_case(out, inter, model, case, python_steps=2)    # one eager step, one capture; the other S - 2 are replays
    eager, inter_e = eager_runs[name][:2]
    assert torch.equal(out, eager)
    for key in ("x_inter", "pred_x0"):
        assert len(inter[key]) == len(inter_e[key]) and all(torch.equal(a, b) for a, b in zip(inter[key], inter_e[key]))


def test_runs_that_stay_on_the_eager_loop(eager_runs):
    _need_gpu()
    name = "S4_cfg7.5_11_n420"
    out, inter, model, case = eager_runs[name]
    passes = 2
    # a model without the tables of q_sample
    o2, i2, m2, _ = R.run_case(name, device="cuda", use_graph=True, with_engine=True, tables=False)
    assert len(m2.calls) == case["S"] * passes and torch.equal(o2, out)
    # a mask of another layout: broadcast over H (B, 1, 1, W) -- torch broadcasts it, the kernel has no such form
    col = case["mask"][:, :, :1, :].clone()
    o3, _, m3, _ = R.run_case(name, device="cuda", use_graph=True, with_engine=True, mask=col)
    assert len(m3.calls) == case["S"] * passes and bool(torch.isfinite(o3).all())
    o3e, _, _, _ = R.run_case(name, device="cuda", use_graph=False, with_engine=True, mask=col)
    assert torch.equal(o3, o3e)
    # fewer than 4 steps: S = 2 (times 1, 501)
    o4, _, m4, _ = R.run_case(name, device="cuda", use_graph=True, with_engine=True, S=2)
    assert len(m4.calls) == 2 * passes and m4.executed_times() == [501, 501, 1, 1] and bool(torch.isfinite(o4).all())
    # no engine
    o5, _, m5, _ = R.run_case(name, device="cuda", use_graph=True, with_engine=False)
    assert len(m5.calls) == case["S"] * passes and torch.equal(o5, out)


# ------------------------------------------------------------------------------ whole model

B, SCALE, LAT = 2, 7.5, (4, 16, 16)


@pytest.fixture(scope="module")
def tiny():
    """The tiny drop-in model as tests/test_gpu_sampling_loop.py builds it (fp32 engine), seeded inputs, a half-plane mask."""
    hip = _need_gpu()
    import bench
    from oracle import arch
    from tests.golden.make_golden import inputs_for
    cfg = arch.TINY
    model = bench.build_model("ctrlora_finetune_sd15_rank128.yaml", 0, tiny=True).cuda().eval()
    model.set_engine_dtype(torch.float32)
    inp = inputs_for(cfg, B, 16, 8)
    g = torch.Generator().manual_seed(1)
    draw = lambda *s: torch.randn(*s, generator=g).cuda()
    x_T, ctx_u, x0, q_noise = draw(B, *LAT), draw(B, 77, cfg.context_dim), draw(B, *LAT), draw(B, *LAT)
    cond = {"c_crossattn": [inp["ctx"].cuda()], "c_concat": [inp["hint_z"].cuda()]}
    unc = {"c_crossattn": [ctx_u], "c_concat": [inp["hint_z"].cuda()]}
    mask = torch.zeros(1, 1, 16, 16, device="cuda")
    mask[..., :8] = 1.0
    return dict(model=model, x_T=x_T, cond=cond, unc=unc, x0=x0, q_noise=q_noise, mask=mask, hip=hip)


def _counted(t, monkeypatch, use_graph, fn, q_noise=True, reuse=False):
    """fn(sampler) with the Python-level apply_model calls counted; returns (fn's result, batch size of every call, sampler)."""
    from cldm.ddim_hacked import DDIMSampler
    model, calls = t["model"], []
    inner = model.apply_model

    def counted(x, ts, c, *a, **k):
        calls.append(int(x.shape[0]))
        return inner(x, ts, c, *a, **k)

    monkeypatch.setattr(model, "apply_model", counted)
    s = DDIMSampler(model)
    s.use_graph, s.reuse_graph = use_graph, reuse
    s.q_noise = t["q_noise"] if q_noise else None
    try:
        return fn(s), calls, s
    finally:
        monkeypatch.undo()


def _masked(t, S=4, mask=None):
    return lambda s: s.sample(S, B, LAT, t["cond"], verbose=False, eta=0.0, x_T=t["x_T"], unconditional_guidance_scale=SCALE,
                              unconditional_conditioning=t["unc"], mask=t["mask"] if mask is None else mask, x0=t["x0"])[0]


def test_whole_model_masked_sample_replayed_equals_eager(tiny, monkeypatch):
    S = 4
    graphed, calls_g, _ = _counted(tiny, monkeypatch, True, _masked(tiny, S))
    eager, calls_e, _ = _counted(tiny, monkeypatch, False, _masked(tiny, S))
    assert calls_g == [2 * B] * 2 and calls_e == [2 * B] * S
    assert bool(torch.isfinite(graphed).all()) and float(graphed.std()) > 0
    assert torch.equal(graphed, eager)
    plain, _, _ = _counted(tiny, monkeypatch, True, lambda s: s.sample(
        S, B, LAT, tiny["cond"], verbose=False, eta=0.0, x_T=tiny["x_T"], unconditional_guidance_scale=SCALE,
        unconditional_conditioning=tiny["unc"])[0])
    assert not torch.equal(plain, graphed)                       # the mask did something


def test_whole_model_decode_replayed_equals_eager(tiny, monkeypatch):
    def dec(s):
        s.make_schedule(8, ddim_eta=0.0, verbose=False)
        seen = []
        out = s.decode(tiny["x_T"], tiny["cond"], 4, unconditional_guidance_scale=SCALE, unconditional_conditioning=tiny["unc"],
                       callback=seen.append)
        assert seen == [0, 1, 2, 3]
        return out

    graphed, calls_g, _ = _counted(tiny, monkeypatch, True, dec)
    eager, calls_e, _ = _counted(tiny, monkeypatch, False, dec)
    assert calls_g == [2 * B] * 2 and calls_e == [2 * B] * 4
    assert bool(torch.isfinite(graphed).all()) and torch.equal(graphed, eager)
    # three steps stay eager; use_original_steps stays refused
    short, calls_s, s = _counted(tiny, monkeypatch, True, lambda s: (s.make_schedule(8, ddim_eta=0.0, verbose=False),
                                                                      s.decode(tiny["x_T"], tiny["cond"], 3))[1])
    assert calls_s == [B] * 3
    with pytest.raises(NotImplementedError):
        s.decode(tiny["x_T"], tiny["cond"], 4, use_original_steps=True)


@pytest.mark.parametrize("scale", [1.0, SCALE])
def test_whole_model_encode_replayed_equals_eager(tiny, monkeypatch, scale):
    def enc(s):
        s.make_schedule(8, ddim_eta=0.0, verbose=False)
        seen = []
        x, info = s.encode(tiny["x0"], tiny["cond"], 4, return_intermediates=2, unconditional_guidance_scale=scale,
                           unconditional_conditioning=tiny["unc"] if scale != 1.0 else None, callback=seen.append)
        assert seen == [0, 1, 2, 3]
        return x, info

    (xg, ig), calls_g, _ = _counted(tiny, monkeypatch, True, enc)
    (xe, ie), calls_e, _ = _counted(tiny, monkeypatch, False, enc)
    nb = B if scale == 1.0 else 2 * B
    assert calls_g == [nb] * 2 and calls_e == [nb] * 4
    assert bool(torch.isfinite(xg).all()) and torch.equal(xg, xe) and not torch.equal(xg, tiny["x0"])
    assert sorted(ig) == sorted(ie) == ["intermediate_steps", "intermediates", "x_encoded"]
    assert ig["intermediate_steps"] == ie["intermediate_steps"] == [0, 2, 3]
    assert torch.equal(ig["x_encoded"], xg) and len(ig["intermediates"]) == 3
    assert all(torch.equal(a, b) for a, b in zip(ig["intermediates"], ie["intermediates"]))
    assert torch.equal(ig["intermediates"][-1], xg)


def test_whole_model_reuse_graph_hits_on_the_same_mask_only(tiny, monkeypatch):
    other = tiny["mask"].clone()

    def three(s):
        a = _masked(tiny, 4)(s)
        hits_a = s.graph_hits
        b = _masked(tiny, 4)(s)
        hits_b = s.graph_hits
        c = _masked(tiny, 4, mask=other)(s)
        return a, b, c, (hits_a, hits_b, s.graph_hits)

    (a, b, c, hits), calls, _ = _counted(tiny, monkeypatch, True, three, reuse=True)
    assert hits == (0, 1, 1)                                     # the second call replays the kept graph; another mask tensor re-captures
    assert calls == [2 * B] * 4                                  # two Python steps for the first and for the third call
    assert torch.equal(a, b) and torch.equal(a, c)               # (the other mask holds the same values)


def test_whole_model_masked_replay_is_reproducible_under_a_seed(tiny, monkeypatch):
    def seeded(s):
        torch.manual_seed(11)
        return _masked(tiny, 4)(s)

    a, calls, _ = _counted(tiny, monkeypatch, True, seeded, q_noise=False)
    b, _, _ = _counted(tiny, monkeypatch, True, seeded, q_noise=False)
    assert calls == [2 * B] * 2 and torch.equal(a, b)
    fixed, _, _ = _counted(tiny, monkeypatch, True, seeded)
    assert not torch.equal(a, fixed)                             # the drawn noise is not the fixed one
    e, _, _ = _counted(tiny, monkeypatch, False, seeded, q_noise=False)
    # not promised, reported for DESIGN 1d: the eager loop also draws the update's noise at every step (eta = 0 included)
    print("replayed and eager masked loops land on the same generator stream:", bool(torch.equal(a, e)))


# ------------------------------------------------------------------------------ scripts/sample.py --init_strength

def test_sample_script_init_strength_runs_img2img_from_the_target_image(tmp_path, monkeypatch):
    """`--init_strength 0.5` of 8 steps noises the dataset's target image to step 4 and runs the 4 remaining steps (replayed:
    2 Python-level model calls) through the real first stage; the image differs from the one sampled from noise.  The flag is
    refused with a sampler that has no decode()."""
    _need_gpu()
    import glob
    import importlib.util
    import sys

    def load(path, name):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod

    monkeypatch.setenv("CTRLORA_SYNTHETIC_TOKENIZER", "1")
    assets = str(tmp_path / "synth")
    tool = load(os.path.join(ROOT, "tests", "tools", "make_synthetic_assets.py"), "make_synthetic_assets")
    monkeypatch.setattr(sys, "argv", ["make_synthetic_assets.py", "--out", assets, "--n", "1"])
    tool.main()
    from cldm.ddim_hacked import DDIMSampler
    from cldm.model import create_model
    from datasets.custom_dataset import CustomDataset
    from torch.utils.data import Subset
    cfg, data = os.path.join(assets, "finetune_narrow.yaml"), os.path.join(assets, "custom")
    torch.manual_seed(3)
    model = create_model(cfg).cpu()
    with torch.no_grad():                       # the zero-initialised output convolution would make eps == 0 at every step
        model.model.diffusion_model.out[-1].weight.normal_(0.0, 0.05)
    model = model.cuda().eval()
    sample = load(os.path.join(ROOT, "scripts", "sample.py"), "sample")
    argv = lambda d, *extra: ["--dataroot", data, "--config", cfg, "--ckpt", "unused", "--n_samples", "1", "--save_dir",
                              str(tmp_path / d), "--ddim_steps", "8", *extra]
    calls = []
    inner = model.apply_model
    monkeypatch.setattr(model, "apply_model", lambda x, ts, c, *a, **k: (calls.append(int(x.shape[0])), inner(x, ts, c, *a, **k))[1])
    ds = Subset(CustomDataset(data), range(1))
    torch.manual_seed(5)
    sample.sample_dataset(model, DDIMSampler(model), ds, sample.get_parser().parse_args(argv("noise")))
    n_plain = len(calls)
    torch.manual_seed(5)
    sample.sample_dataset(model, DDIMSampler(model), ds, sample.get_parser().parse_args(argv("i2i", "--init_strength", "0.5")))
    assert n_plain == 2 and len(calls) == 4                     # both runs replay: one eager step and one capture each
    from PIL import Image
    png = lambda d: np.asarray(Image.open(glob.glob(str(tmp_path / d / "sample" / "*.png"))[0]))
    a, b = png("noise"), png("i2i")
    assert a.shape == b.shape and b.std() > 0 and not np.array_equal(a, b)
    with pytest.raises(SystemExit):
        sample.main(argv("refused", "--init_strength", "0.5", "--sampler", "plms"))


# ------------------------------------------------------------------------------ api.CtrLoRA end to end

@pytest.fixture(scope="module")
def ctr():
    """api.CtrLoRA around the tiny inference model, filled through its own load sequence (tests/test_gpu_parity.py).  The
    benchmark builder replaces VAE and CLIP by Identity, so the three methods the API calls on them get deterministic
    stand-ins on the instance: an 8 x 8 average pool / nearest up-sampling as first stage, a seeded context as text encoder."""
    _need_gpu()
    import api
    import bench
    from oracle import arch
    cfg = arch.TINY
    m = bench.build_model("inference/ctrlora_sd15_rank128_1lora.yaml", 0, tiny=True)
    m.model.diffusion_model.load_state_dict(arch.make_state(arch.unet_shapes(cfg), 5), strict=True)
    sd = {"control_model." + k: v for k, v in arch.make_state(arch.controlnet_shapes(cfg), 6).items()}
    c = api.CtrLoRA(num_loras=1)
    c.load_weights(m, cn_state_dict=sd, lora_state_dicts=[sd])
    m = m.cuda().eval()
    m.set_engine_dtype(torch.float32)

    def encode(x):       # [n, 3, H, W] in [-1, 1] (or a condition image in [0, 1]) -> [n, 4, H / 8, W / 8]
        z = torch.nn.functional.avg_pool2d(x.float(), 8)
        return torch.cat([z, z.mean(1, keepdim=True)], 1) / m.scale_factor

    def decode(z):
        return torch.nn.functional.interpolate(z[:, :3].float(), scale_factor=8, mode="nearest")

    def text(prompts):
        g = torch.Generator().manual_seed(len(prompts[0]) + 1)
        return torch.randn(1, 77, cfg.context_dim, generator=g).repeat(len(prompts), 1, 1).cuda()

    m.encode_first_stage, m.decode_first_stage, m.get_learned_conditioning = encode, decode, text
    c.model = m
    return c


def test_api_img2img_masked_composite_and_inert_defaults(ctr, monkeypatch):
    g = np.random.default_rng(3)
    H = W = 128
    cond_img = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    init = g.integers(0, 256, (H + 8, W + 4, 3), dtype=np.uint8)          # larger: centre-cropped to the condition image
    init_c = init[4:4 + H, 2:2 + W]
    calls = []
    inner = ctr.model.apply_model
    monkeypatch.setattr(ctr.model, "apply_model", lambda x, ts, c, *a, **k: (calls.append(int(x.shape[0])), inner(x, ts, c, *a, **k))[1])
    run = lambda **kw: (torch.manual_seed(3), np.stack([np.asarray(im) for im in ctr.sample_1lora(cond_img, "a prompt", "", 1, 8, 7.5, **kw)]))[1]
    # defaults are inert
    plain = run()
    assert plain.shape == (1, H, W, 3) and plain.dtype == np.uint8 and plain.std() > 0
    assert np.array_equal(plain, run(init_image=None, strength=1.0, mask_image=None, composite=True))
    assert np.array_equal(plain, run(init_image=init))                    # strength 1.0 and no mask: sampling from noise
    # img2img: t_enc = int(0.75 * 8) = 6 steps from the noised image, replayed (2 Python-level steps)
    del calls[:]
    i2i = run(init_image=init, strength=0.75)
    assert calls == [2] * 2, calls
    assert i2i.shape == plain.shape and not np.array_equal(i2i, plain) and i2i.std() > 0
    # a weaker edit stays closer to the image it started from
    weak = run(init_image=init, strength=0.5)
    dist = lambda a: float(np.abs(a[0].astype(np.float64) - init_c).mean())
    print(f"mean |result - init|: strength 0.5 {dist(weak):.2f}, 0.75 {dist(i2i):.2f}, from noise {dist(plain):.2f}")
    # masked: repaint a rectangle that is not aligned to the 8 x 8 cells
    marked = np.zeros((H, W), np.uint8)
    marked[30:70, 41:90] = 255
    del calls[:]
    comp = run(init_image=init, mask_image=marked)
    assert calls == [2] * 2, calls                                        # the full schedule, replayed
    assert np.array_equal(comp[0][marked == 0], init_c[marked == 0])      # unmarked pixels are the init image's own
    assert not np.array_equal(comp[0][marked != 0], init_c[marked != 0])
    raw = run(init_image=init, mask_image=marked, composite=False)
    assert np.array_equal(raw[0][marked != 0], comp[0][marked != 0]) and not np.array_equal(raw, comp)
    with pytest.raises(ValueError):
        run(init_image=init, mask_image=marked, strength=0.5)
    with pytest.raises(ValueError):
        run(mask_image=marked)
    with pytest.raises(ValueError):
        run(init_image=init, strength=0.01)                               # t_enc == 0
