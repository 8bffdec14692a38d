"""Latent cache on an MI355X.

Kernel (cl_posterior_sample_pair, csrc/elementwise.hip), EXACT tier: out = scale * (mean + std * e) bit for bit against the three
torch fp32 ops on the device -- sizes 1, 3, a multiple of 4, a multiple of 4 plus 1, the SD latent of a batch of 16, and sizes past
one sweep of the largest grid (tests/ew_ref.py: WRAP_N) in the scalar and in the 16-byte form; one tensor and two; every operand
in turn offset by 4 bytes (scalar path).  Outputs sit inside guard rows and pad columns (tests/gemm_ref.py: Guarded); the launch
probe must report what the launcher's transcription below predicts; the refusals return 1 and write nothing.

Whole step: on the synthetic assets (narrow config, 4 pairs) `training_step` + backward on batch 0 from CustomDataset and from
CachedLatentDataset, same torch and numpy seeds, in fp32 and in bf16 engine mode: the latents, the loss and the flat gradient
buffer are bit-equal (same deterministic encoder, same draws, exact arithmetic; the fp32 weight gradients in their opt-in fixed-order form,
hip.WGRAD_F32_DETERMINISTIC, which has a kernel-level check of its own below).

End to end: scripts/tool_cache_latents.py, then scripts/train_ctrlora_finetune.py --latent_cache for three steps with the image
logger: a checkpoint and a PNG are written and AutoencoderKL.encode is never called.
"""
import ctypes
import glob
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from tests import ew_ref as R
from tests.util import ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda"
EW_POSTERIOR_PAIR = 34          # csrc/elementwise.h: appended after EW_GATHER_ROWS (33)
SCALE = 0.18215


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _probe():
    from ctrlora_amd import hip
    out = (ctypes.c_int * 8)()
    assert hip.lib().cl_debug_ew_last_launch(out) == 0
    return dict(zip(R.PROBE_FIELDS, list(out)))


def _operands(B, per, seed, off):
    """(mom, e) on the device; `off` = set of names whose first element sits 4 bytes past a 16-byte boundary."""
    g = torch.Generator().manual_seed(seed)
    mom = torch.cat([torch.randn(B, per, generator=g), torch.rand(B, per, generator=g) * 2 + 1e-3], 1)
    e = torch.randn(B, per, generator=g)

    def place(t, shifted):
        buf = torch.empty(t.numel() + 4, device=DEV)
        v = buf[1:1 + t.numel()] if shifted else buf[:t.numel()]
        v.copy_(t.reshape(-1))
        assert v.data_ptr() % 16 == (4 if shifted else 0)
        return v.view(t.shape)
    return place(mom, "mom" in off), place(e, "e" in off)


def _guarded_out(n, shifted):
    """A flat output of n floats inside Guarded's guard rows / pad columns; shifted: it starts 4 bytes past a 16-byte boundary (the
    element before it stays NaN and is counted out)."""
    g = R.Guarded(1, n + (1 if shifted else 0), torch.float32, DEV)
    v = g.view[0, 1:] if shifted else g.view[0]
    assert v.is_contiguous() and v.numel() == n and v.data_ptr() % 16 == (4 if shifted else 0)
    return g, v


def _want(mom, e, per):
    p = mom[:, per:] * e                 # three torch fp32 ops on the device, each rounded once
    s = mom[:, :per] + p
    return SCALE * s


CASES = [(1, 1), (1, 3), (2, 4 * 8 * 8), (3, 4 * 24 * 16 + 1), (16, 4 * 64 * 64), (1, R.WRAP_N), (1, 4 * R.WRAP_N)]
OFFSETS = [(), ("mom_a",), ("e_a",), ("out_a",), ("e_b",), ("mom_b", "out_b")]


def _run_case(B, per, pair, off):
    from ctrlora_amd import hip
    L = hip.lib()
    names = ("a", "b") if pair else ("a",)
    ops, outs = {}, {}
    for i, t in enumerate(names):
        sh = {k.split("_")[0] for k in off if k.endswith("_" + t)}
        ops[t] = _operands(B, per, 10 + i, sh)
        outs[t] = _guarded_out(B * per, "out" in sh)
    ptrs = []
    for t in ("a", "b"):
        ptrs += [ops[t][0].data_ptr(), ops[t][1].data_ptr(), outs[t][1].data_ptr()] if t in ops else [None, None, None]
    rc = L.cl_posterior_sample_pair(*ptrs, B, per, SCALE, hip.stream())
    probe = _probe()
    torch.cuda.synchronize()
    assert rc == 0
    vec = per % 4 == 0 and not off
    nw = B * (per // 4 if vec else per) * len(names)
    want_probe = dict(id=EW_POSTERIOR_PAIR, dtype=-1, gx=R.ew_grid(nw), gy=1, gz=1, threads=256, form=int(vec), aux=len(names))
    assert probe == want_probe, (probe, want_probe)
    if per >= R.WRAP_N:
        assert R.wraps(nw), "the wrap rows must iterate the grid-stride loop twice"
    for t in names:
        g, v = outs[t]
        chk = g.check()
        shifted = v.data_ptr() % 16 == 4
        assert chk["guard_rows"] == 0 and chk["pad_elems"] == 0 and chk["nan_left"] == (1 if shifted else 0), (t, chk)
        want = _want(ops[t][0], ops[t][1], per).reshape(-1)
        diff = int((v.view(torch.int32) != want.view(torch.int32)).sum())
        print(f"[posterior pair] B={B} per={per} tensors={len(names)} off={off} tensor {t}: {diff} of {v.numel()} elements differ")
        assert torch.equal(v, want), (t, diff)


@pytest.mark.parametrize("pair", [False, True], ids=["single", "pair"])
@pytest.mark.parametrize("B,per", CASES, ids=[f"{b}x{p}" for b, p in CASES])
def test_pair_kernel_is_bit_exact_inside_guards(B, per, pair):
    _need_gpu()
    _run_case(B, per, pair, ())


@pytest.mark.parametrize("off", OFFSETS[1:], ids=["+".join(o) for o in OFFSETS[1:]])
@pytest.mark.parametrize("B,per", [(2, 4 * 8 * 8), (16, 4 * 64 * 64)], ids=["2x256", "16x16384"])
def test_pair_kernel_operand_offset_by_four_bytes_takes_the_scalar_path(B, per, off):
    _need_gpu()
    _run_case(B, per, any(k.endswith("_b") for k in off) or "e_a" in off, off)


def test_pair_kernel_has_no_fma_contraction():
    """mean = -(std * e rounded to fp32): the rounded product followed by the rounded sum gives exactly 0, a contracted
    std * e + mean gives the product's rounding error, nonzero in most elements."""
    _need_gpu()
    from ctrlora_amd import hip
    g = torch.Generator().manual_seed(4)
    n = 4096
    std = (1 + torch.rand(n, generator=g)).to(DEV)
    e = (1 + torch.rand(n, generator=g)).to(DEV)
    mean = -(std * e)
    fused = (mean.double() + std.double() * e.double()).float()      # exact in fp64, rounded once: what an FMA returns
    assert int((fused != 0).sum()) > n // 2, "the operands do not tell an FMA from two roundings"
    for per, B in ((n, 1), (n // 4 - 1, 1)):                         # the 16-byte form, and the scalar form on a prefix
        out = torch.full((B, per), float("nan"), device=DEV)
        m = torch.cat([mean[:per], std[:per]]).reshape(1, 2 * per).contiguous()
        hip.posterior_sample_pair(m, e[:per].reshape(1, per).contiguous(), out, SCALE)
        assert int((out != 0).sum()) == 0, (per, int((out != 0).sum()))


def test_pair_kernel_refusals_return_one_and_write_nothing():
    _need_gpu()
    from ctrlora_amd import hip
    L = hip.lib()
    B, per = 2, 64
    (mom, e), (g, v) = _operands(B, per, 1, ()), _guarded_out(B * per, False)
    (mom2, e2), (g2, v2) = _operands(B, per, 2, ()), _guarded_out(B * per, False)
    p = lambda t: t.data_ptr()
    N, st = None, hip.stream()
    full = (p(mom), p(e), p(v))
    calls = {
        "null mom_a": (N, p(e), p(v), N, N, N, B, per), "null e_a": (p(mom), N, p(v), N, N, N, B, per),
        "null out_a": (p(mom), p(e), N, N, N, N, B, per), "B = 0": full + (N, N, N, 0, per), "B < 0": full + (N, N, N, -1, per),
        "per = 0": full + (N, N, N, B, 0), "per < 0": full + (N, N, N, B, -4),
        "b without e": full + (p(mom2), N, p(v2), B, per), "b without out": full + (p(mom2), p(e2), N, B, per),
        "b without mom": full + (N, p(e2), p(v2), B, per), "b out only": full + (N, N, p(v2), B, per),
    }
    for what, a in calls.items():
        assert L.cl_posterior_sample_pair(*a, SCALE, st) == 1, what
        assert _probe()["id"] == 0, what
    torch.cuda.synchronize()
    for gg in (g, g2):
        chk = gg.check()
        assert chk["guard_rows"] == 0 and chk["pad_elems"] == 0 and chk["nan_left"] == B * per, chk
    with pytest.raises(hip.HipError, match="cl_posterior_sample_pair"):
        hip.posterior_sample_pair(mom.reshape(B, 2 * per)[:0], e[:0], v.reshape(B, per)[:0], SCALE)


WG_SHAPES = [(320, 128, 8192), (128, 320, 8192), (1280, 128, 160), (32, 288, 2048)]     # (N, K, Mp): LoRA up / down at the 64x64 level
                                                                                            # of a batch of 2, at 8x8, a conv tap


@pytest.mark.parametrize("N,K,Mp", WG_SHAPES, ids=[f"{n}x{k}x{m}" for n, k, m in WG_SHAPES])
def test_opt_in_fp32_weight_gradient_adds_onto_dw_reproducibly_and_matches_fp64(N, K, Mp, monkeypatch):
    """hip.weight_grad with WGRAD_F32_DETERMINISTIC: dW += scale * dyT xT^T in place, onto a non-zero dW that is a column slice of a
    wider buffer (as the taps of a conv gradient are).  Element-wise against fp64 with the bound of an fp32 sum of Mp + 1 terms in
    any order, (Mp + 1) 2^-24 (sum |terms|) (Higham, Accuracy and Stability, eq. 4.4); two launches give the same bits; the
    columns beside the slice keep theirs; a misaligned dW is refused."""
    _need_gpu()
    from ctrlora_amd import hip
    monkeypatch.setattr(hip, "WGRAD_F32_DETERMINISTIC", True)
    g = torch.Generator().manual_seed(N + K + Mp)
    dyT, xT = torch.randn(N, Mp, generator=g).to(DEV), torch.randn(K, Mp, generator=g).to(DEV)
    base = torch.randn(N, K + 16, generator=g).to(DEV)
    scale = 0.37
    outs = []
    for _ in range(2):
        buf = base.clone()
        hip.weight_grad(dyT, xT, buf[:, 8:8 + K], scale)
        torch.cuda.synchronize()
        outs.append(buf)
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0][:, :8], base[:, :8]) and torch.equal(outs[0][:, 8 + K:], base[:, 8 + K:])
    ref = scale * (dyT.double() @ xT.double().t()) + base[:, 8:8 + K].double()
    mag = abs(scale) * (dyT.double().abs() @ xT.double().abs().t()) + base[:, 8:8 + K].double().abs()
    err = (outs[0][:, 8:8 + K].double() - ref).abs()
    bound = (Mp + 1) * 2.0 ** -24 * mag
    print(f"[fp32 wgrad opt-in {N}x{K}x{Mp}] worst err / bound {float((err / bound).max()):.3e}")
    assert int((err > bound).sum()) == 0
    with pytest.raises(hip.HipError, match="16-byte aligned"):
        hip.weight_grad(dyT, xT, base.clone()[:, 1:1 + K], scale)


def test_cached_get_input_is_refused_inside_a_stream_capture(monkeypatch):
    _need_gpu()
    from tests.test_training_scripts import _tiny_ldm
    m = _tiny_ldm(0).cuda()
    mom = torch.ones(2, 8, 4, 4)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="inside a hipGraph capture"):
        m.get_input(dict(jpg_moments=mom, hint_moments=mom, txt=["a", "b"]), m.first_stage_key)


# ------------------------------------------------------------------------------------------------ whole step, end to end

def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _script(name):
    return _load(os.path.join(ROOT, "scripts", name + ".py"), name)


@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    _need_gpu()
    out = str(tmp_path_factory.mktemp("synth_latent_cache"))
    mod = _load(os.path.join(ROOT, "tests", "tools", "make_synthetic_assets.py"), "make_synthetic_assets")
    argv, sys.argv = sys.argv, ["make_synthetic_assets.py", "--out", out, "--n", "4"]
    try:
        mod.main()
    finally:
        sys.argv = argv
    return out


@pytest.fixture(scope="module")
def model(assets, tmp_path_factory):
    from cldm.model import create_model, load_state_dict
    train = _script("train_ctrlora_finetune")
    m = create_model(os.path.join(assets, "finetune_narrow.yaml")).cpu()
    m.learning_rate, m.sd_locked, m.only_mid_control = 1e-4, True, False
    train.init_weights(m, load_state_dict(os.path.join(assets, "sd_synth.ckpt")), load_state_dict(os.path.join(assets, "basecn_synth.ckpt")),
                       report_dir=str(tmp_path_factory.mktemp("init_report")))
    return m.cuda().train()


@pytest.fixture(scope="module", params=[torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def step_pair(request, assets, model, tmp_path_factory):
    """Batch 0 through get_input and through training_step + backward, once from CustomDataset and once from a cache built over
    the same images in the same engine mode, under the same torch and numpy seeds; computed once per dtype."""
    from torch.utils.data import DataLoader
    from ctrlora_amd import hip, latent_cache as LC
    from datasets.cached_latents import CachedLatentDataset
    from datasets.custom_dataset import CustomDataset
    from ldm.models.autoencoder import AutoencoderKL
    dtype, work = request.param, tmp_path_factory.mktemp("step_pair")
    mp = pytest.MonkeyPatch()
    try:
        mp.setenv("CTRLORA_SYNTHETIC_TOKENIZER", "1")
        # bits are compared: the fp32 mode's weight gradients in their fixed-order form (off by default; bf16 does not use it)
        mp.setattr(hip, "WGRAD_F32_DETERMINISTIC", True)
        mp.chdir(work)                                            # configure_optimizers writes ./tmp/finetune_trainable_params.txt
        root, cache = os.path.join(assets, "custom"), str(work / "cache")
        model.set_engine_dtype(dtype)
        opt = model.configure_optimizers()
        LC.build_cache(CustomDataset(root, drop_rate=0), model.encode_first_stage, cache, bs=2, device=model.device,
                       engine_dtype=LC.dtype_name(dtype), fingerprint=LC.state_fingerprint(model.first_stage_model))
        cached_ds = CachedLatentDataset(root, cache, drop_rate=0.5)
        LC.check_model(cached_ds.meta, model, dtype)
        assert cached_ds.meta["latent_shape"] == [4, 64, 64] and cached_ds.meta["engine_dtype"] == LC.dtype_name(dtype)
        live_ds = CustomDataset(root, drop_rate=0.5)
        flat = model.control_model.executor().tr.flat_grad
        encodes = []
        real_encode = AutoencoderKL.encode
        mp.setattr(AutoencoderKL, "encode", lambda self, t: (encodes.append(1), real_encode(self, t))[1])
        out = {}
        for name, ds in (("live", live_ds), ("cached", cached_ds)):
            def batch0():
                torch.manual_seed(11)
                np.random.seed(3)
                return next(iter(DataLoader(ds, batch_size=2, shuffle=False, num_workers=0)))
            z, cond = model.get_input(batch0(), model.first_stage_key)
            hint_z = model._hint_latent(cond)                    # live: the draw apply_model makes; cached: passes through
            opt.zero_grad()
            batch, before = batch0(), len(encodes)
            loss = model.training_step(batch, 0)
            loss.backward()
            torch.cuda.synchronize()
            out[name] = dict(z=z.clone(), hint_z=hint_z.clone(), ctx=cond["c_crossattn"][0].clone(), loss=loss.detach().clone(),
                             grad=flat.clone(), txt=list(batch["txt"]), encodes=len(encodes) - before)
        ndiff = int((out["live"]["grad"].view(torch.int32) != out["cached"]["grad"].view(torch.int32)).sum())
        print(f"[latent cache {LC.dtype_name(dtype)}] loss live {float(out['live']['loss'])!r} cached {float(out['cached']['loss'])!r}; "
              f"{ndiff} of {flat.numel()} gradient elements differ, max |diff| "
              f"{float((out['live']['grad'] - out['cached']['grad']).abs().max()):.3e}, max |grad| {float(out['live']['grad'].abs().max()):.3e}")
        return out
    finally:
        mp.undo()


def test_cached_batch_gives_the_live_latents_and_runs_no_encode(step_pair):
    """get_input from the cache returns the live path's z and the hint latent apply_model would draw, bit for bit, with the same
    prompts (drop-out stream) and context, and the cached training step never calls the first stage's encode."""
    live, cached = step_pair["live"], step_pair["cached"]
    assert live["txt"] == cached["txt"] and torch.equal(live["ctx"], cached["ctx"])
    assert live["encodes"] == 2 and cached["encodes"] == 0
    assert live["z"].shape == (2, 4, 64, 64) and torch.isfinite(live["z"]).all()
    assert torch.equal(live["z"], cached["z"])
    assert torch.equal(live["hint_z"], cached["hint_z"]) and not torch.equal(live["z"], live["hint_z"])


def test_loss_from_the_cache_equals_the_live_step_bit_for_bit(step_pair):
    live, cached = step_pair["live"], step_pair["cached"]
    assert torch.isfinite(live["loss"]) and float(live["loss"]) > 0
    assert torch.equal(live["loss"], cached["loss"])


def test_flat_gradient_buffer_from_the_cache_equals_the_live_step_bit_for_bit(step_pair):
    """Both steps run with hip.WGRAD_F32_DETERMINISTIC on (step_pair): the default fp32 weight gradient accumulates with float
    atomics, whose order of arrival is not a function of the inputs, so its bits cannot be compared between any two steps."""
    live, cached = step_pair["live"], step_pair["cached"]
    assert float(live["grad"].abs().sum()) > 0
    assert torch.equal(live["grad"], cached["grad"])


def test_finetune_script_trains_from_a_cache_without_encoding(assets, tmp_path, monkeypatch):
    monkeypatch.setenv("CTRLORA_SYNTHETIC_TOKENIZER", "1")
    monkeypatch.chdir(tmp_path)
    from ldm.models.autoencoder import AutoencoderKL
    cfg, root, cache = os.path.join(assets, "finetune_narrow.yaml"), os.path.join(assets, "custom"), str(tmp_path / "latents")
    sd = os.path.join(assets, "sd_synth.ckpt")
    encodes = []
    real_encode = AutoencoderKL.encode
    monkeypatch.setattr(AutoencoderKL, "encode", lambda self, t: (encodes.append(int(t.shape[0])), real_encode(self, t))[1])
    meta = _script("tool_cache_latents").main(["--dataroot", root, "--config", cfg, "--sd_ckpt", sd, "--out", cache, "--bs", "4",
                                               "--precision", "16"])
    assert meta["N"] == 4 and meta["engine_dtype"] == "bf16" and encodes == [4, 4]        # targets, then conditions
    assert sorted(os.listdir(cache)) == ["hint_moments.npy", "meta.json", "target_moments.npy"]
    del encodes[:]
    train = _script("train_ctrlora_finetune")
    args = ["--dataroot", root, "--config", cfg, "--sd_ckpt", sd, "--cn_ckpt", os.path.join(assets, "basecn_synth.ckpt"), "--bs", "2",
            "--precision", "16", "--ckpt_logger_freq", "2", "--lr", "1e-4", "-n", "lc", "--num_workers", "0",
            "--latent_cache", cache, "--max_steps", "3", "--img_logger_freq", "2"]
    train.main(args)
    assert encodes == [], "the first stage encoded during a run from the latent cache"
    cks = sorted(glob.glob(os.path.join("runs", "lc", "**", "*.ckpt"), recursive=True))
    assert cks, "CheckpointEveryNSteps wrote nothing"
    ck = torch.load(cks[-1], map_location="cpu", weights_only=False)
    assert int(ck["global_step"]) == 3
    up = [v for k, v in ck["state_dict"].items() if k.endswith("lora_layer.up.weight")]
    assert up and all(torch.isfinite(v).all() for v in up) and any(float(v.abs().sum()) > 0 for v in up)     # B = 0 at the start: it trained
    pngs = glob.glob(os.path.join("runs", "lc", "**", "*.png"), recursive=True)
    keys = {os.path.basename(os.path.dirname(p)) for p in pngs}
    assert {"reconstruction", "control", "conditioning"} <= keys and any(k.startswith("samples_cfg_scale") for k in keys), keys
    from PIL import Image
    ctrl = np.asarray(Image.open([p for p in pngs if os.path.basename(os.path.dirname(p)) == "control"][0]))
    assert ctrl.ndim == 3 and ctrl.shape[-1] == 3 and ctrl.std() > 0, "the decoded hint latent is constant"
