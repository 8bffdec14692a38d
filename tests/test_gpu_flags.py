"""ControlNetFinetune's norm_trainable / zero_trainable switches on the GPU (run with -m gpu on an MI355X).

Every test goes through ControlFinetuneLDM.configure_optimizers() with at least one flag off -- the call that raised
NotImplementedError before the flags reached the engine.  References: tests/golden/flags_tiny.pt (the UNMODIFIED
reference's optimizer list, eps, gradients and AdamW step per combination, tests/golden/make_golden_flags.py) and the
CPU oracle.

Gates: fp32 = the `tiny` fp32 row of test_gpu_parity.py::test_engine_forward_backward_vs_oracle_and_reference_golden
(eps 1e-4, gradients 5e-4 rel-L2).  bf16 = DESIGN section 1a's comparator rule as tests/test_gpu_bench_shapes.py states
it: k x the oracle's own bf16-autocast gap measured in the same test, k = 1.3 (eps, median gradient) and 1.5 (worst
gradient)."""
import glob
import importlib.util
import os
import sys

import pytest
import torch

from tests.flags_common import COMBOS, combo_key, digest_close, flag_mutator, load_flags_golden, netcfg, sample_idx, selected
from tests.util import ROOT, rel_l2

pytestmark = pytest.mark.gpu

TOL_EPS_F32, TOL_GRAD_F32 = 1e-4, 5e-4


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ctrlora_amd import hip
    hip.lib()


def _model(nt, zt, dtype, sd_cn=None, sd_un=None, lr=1e-4, tiny=True, config="ctrlora_finetune_sd15_rank128.yaml"):
    """The drop-in path with the two flags as control_stage_config params; weights = the key-addressed draw when given."""
    import bench
    m = bench.build_model(config, 0, tiny=tiny, mutate=flag_mutator(nt, zt))
    if sd_cn is not None:
        m.control_model.load_state_dict(sd_cn, strict=True)
        m.model.diffusion_model.load_state_dict(sd_un, strict=True)
    m = m.cuda().train()
    m.set_engine_dtype(dtype)
    m.learning_rate = lr
    return m


def _frozen_cn(model, nt, zt):
    return {n: p for n, p in model.control_model.named_parameters() if not selected(n, nt, zt)}


def _packed_frozen_ok(ex, sd_cn, nt, zt):
    """Packed copies of the frozen norms / zero convs against the loaded values (storage dtype rounding applied once)."""
    ok = True
    names = sorted(k[:-len(".weight")] for k in sd_cn if ("zero_convs" in k or "middle_block_out" in k) and k.endswith(".weight"))
    order = [f"zero_convs.{k}.0" for k in range(len(ex.zero) - 1)] + ["middle_block_out.0"]
    assert sorted(order) == names
    if not zt:
        for z, n in zip(ex.zero, order):
            w = sd_cn[n + ".weight"].reshape(z.N, z.K).cuda()
            ok &= torch.equal(z.W, w.to(z.W.dtype)) and torch.equal(z.Wt, w.t().to(z.W.dtype))
            ok &= torch.equal(z.bias, sd_cn[n + ".bias"].cuda()) and z.tW is None and z.tb is None
    if not nt:
        # every norm of the network (the ResBlocks' GroupNorms are frozen under any flags) still holds the loaded values
        from oracle.arch import _is_norm_key
        ok &= all(w.tg is None and w.ggamma is None and w.gbeta is None for w in ex._b.norms)
        for leaf, pick in ((".weight", lambda w: w.gamma), (".bias", lambda w: w.beta)):
            want = sorted((v.numel(), float(v.double().sum())) for k, v in sd_cn.items() if _is_norm_key(k) and k.endswith(leaf))
            ok &= sorted((pick(w).numel(), float(pick(w).double().sum())) for w in ex._b.norms) == want
    return bool(ok)


def _fixture_inputs():
    from oracle import arch
    from tests.golden.make_golden import inputs_for
    g = load_flags_golden()
    meta = g["meta"]
    cfg = arch.TINY
    inp = inputs_for(cfg, meta["B"], meta["H"], meta["seed"])
    sd_cn = arch.make_state(arch.controlnet_shapes(cfg), meta["seed"])
    sd_un = arch.make_state(arch.unet_shapes(cfg), meta["seed"])
    return g, meta, cfg, inp, sd_cn, sd_un


def _oracle_grads(cfg, sd_cn, sd_un, inp, names):
    from oracle import ref_model as R
    sd = {k: v.clone().requires_grad_(k in names) for k, v in sd_cn.items()}
    loss, eps = R.p_losses(sd, sd_un, cfg, R.make_schedule(), inp["z"], inp["t"], inp["ctx"], inp["hint_z"], inp["noise"])
    loss.backward()
    return float(loss.detach()), eps.detach(), {k: sd[k].grad for k in names}


# ------------------------------------------------------------------------------ gradients

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("nt,zt", COMBOS)
def test_flags_eps_and_selected_gradients_vs_fixture_and_oracle(nt, zt, dtype):
    _need_gpu()
    g, meta, cfg, inp, sd_cn, sd_un = _fixture_inputs()
    gold = g["combos"][combo_key(nt, zt)]
    m = _model(nt, zt, dtype, sd_cn, sd_un, lr=meta["lr"])
    opt = m.configure_optimizers()
    ex = m.control_model.executor()
    names = gold["trainable_names"]
    with open("./tmp/finetune_trainable_params.txt") as f:
        assert f.read().split() == names                                   # the reference's list, in its order
    assert sorted(t.name for t in ex.tr.items) == sorted(names)
    # the flat gradient buffer has no span for a frozen tensor
    assert ex.tr.flat_grad.numel() == ex.tr.numel == sum((t.master.numel() + 63) // 64 * 64 for t in ex.tr.items)
    cu = lambda v: v.cuda()
    cond = {"c_crossattn": [cu(inp["ctx"])], "c_concat": [cu(inp["hint_z"])]}
    opt.zero_grad()
    loss, _ = m.p_losses(cu(inp["z"]), cond, cu(inp["t"]), noise=cu(inp["noise"]))
    loss.backward()
    with torch.no_grad():
        eps = m.apply_model(m.q_sample(cu(inp["z"]), cu(inp["t"]), cu(inp["noise"])), cu(inp["t"]), cond)
    torch.cuda.synchronize()
    loss_o, eps_o, grads_o = _oracle_grads(cfg, sd_cn, sd_un, inp, names)
    params = dict(m.control_model.named_parameters())
    e_fix, e_orc = rel_l2(eps, gold["eps"]), rel_l2(eps, eps_o)
    errs = sorted(((rel_l2(params[n].grad, grads_o[n]), n) for n in names), reverse=True)
    fix = sorted(((rel_l2(params[n].grad.flatten().cpu()[sample_idx(params[n].numel(), meta["n_sampled"])],
                          gold["grad_vals"][n]["vals"]), n) for n in names), reverse=True)
    med = errs[len(errs) // 2][0]
    print(f"[flags {combo_key(nt, zt)} {dtype}] eps vs fixture {e_fix:.3e} vs oracle {e_orc:.3e}; gradients vs oracle worst "
          f"{errs[0][0]:.3e} ({errs[0][1]}) median {med:.3e}; vs fixture samples worst {fix[0][0]:.3e} ({fix[0][1]}); "
          f"loss {float(loss):.6f} / {gold['loss']:.6f}")
    # frozen ControlNet parameters received no gradient at all
    assert all(p.grad is None for p in _frozen_cn(m, nt, zt).values())
    if dtype == torch.float32:
        assert e_fix < TOL_EPS_F32 and e_orc < TOL_EPS_F32
        assert abs(float(loss) - gold["loss"]) < 1e-4 * gold["loss"]
        assert errs[0][0] < TOL_GRAD_F32, errs[:5]
        assert fix[0][0] < TOL_GRAD_F32, fix[:5]
        for n in names:
            digest_close(params[n].grad, gold["grad_digest"][n], TOL_GRAD_F32)
        # one AdamW step against the reference's
        opt.step()
        torch.cuda.synchronize()
        for n, d in gold["adamw_digest"].items():
            digest_close(params[n].detach(), d, 1e-5)
    else:
        from tests.test_gpu_bench_shapes import K_CMP, K_CMP_MAX, _oracle_on_gpu
        _, eps_c, grads_c = _oracle_on_gpu(cfg, sd_cn, sd_un, inp["z"], inp["t"], inp["ctx"], inp["hint_z"], inp["noise"],
                                           autocast=torch.bfloat16)
        ce = sorted((rel_l2(grads_c[n], grads_o[n]) for n in names), reverse=True)
        c_eps, c_max, c_med = rel_l2(eps_c, eps_o), ce[0], ce[len(ce) // 2]
        print(f"[flags {combo_key(nt, zt)} bf16 comparator] eps {c_eps:.3e} worst {c_max:.3e} median {c_med:.3e}")
        assert e_orc < K_CMP * c_eps and errs[0][0] < K_CMP_MAX * c_max and med < K_CMP * c_med, \
            (e_orc, errs[0], med, c_eps, c_max, c_med)
        opt.step()
        torch.cuda.synchronize()
    # the optimizer step left every frozen ControlNet tensor alone: master (module parameter) and packed copy
    for n, p in _frozen_cn(m, nt, zt).items():
        assert torch.equal(p.detach().cpu(), sd_cn[n]), n
    assert _packed_frozen_ok(ex, sd_cn, nt, zt)


# ------------------------------------------------------------------------------ launches

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("nt,zt", COMBOS + [(True, True)])
def test_backward_forms_no_weight_or_bias_gradient_for_a_frozen_tensor(nt, zt, dtype, monkeypatch):
    """Every weight-gradient problem and every bias column sum of one backward, recorded at the launch wrappers: their
    destinations are exactly the LoRA factors (+ the 13 zero-conv weights / biases when those train) inside the flat buffer."""
    _need_gpu()
    from ctrlora_amd import hip
    g, meta, cfg, inp, sd_cn, sd_un = _fixture_inputs()
    m = _model(nt, zt, dtype, sd_cn, sd_un)
    opt = m.configure_optimizers()
    ex = m.control_model.executor()
    wdst, bdst = [], []
    real_w, real_g, real_c = hip.weight_grad, hip.weight_grad_tn_group, hip.colsum
    lo, hi = ex.tr.flat_grad.data_ptr(), ex.tr.flat_grad.data_ptr() + 4 * ex.tr.numel

    def weight_grad(dyT, xT, dW, scale=1.0):
        wdst.append(dW.data_ptr())
        return real_w(dyT, xT, dW, scale)

    def weight_grad_tn_group(problems):
        wdst.extend(p[2].data_ptr() for p in problems)
        return real_g(problems)

    def colsum(x, out, B, HW, scale=1.0):
        if lo <= out.data_ptr() < hi:
            bdst.append(out.data_ptr())
        return real_c(x, out, B, HW, scale)

    monkeypatch.setattr(hip, "weight_grad", weight_grad)
    monkeypatch.setattr(hip, "weight_grad_tn_group", weight_grad_tn_group)
    monkeypatch.setattr(hip, "colsum", colsum)
    cu = lambda v: v.cuda()
    opt.zero_grad()
    m.engine_train_step(cu(inp["z"]), {"c_crossattn": [cu(inp["ctx"])], "c_concat": [cu(inp["hint_z"])]}, cu(inp["t"]),
                        cu(inp["noise"]))
    torch.cuda.synchronize()
    by_ptr = {t.grad.data_ptr(): t.name for t in ex.tr.items}
    assert all(p in by_ptr for p in wdst), "a weight gradient was formed outside the trainable set"
    w_names = sorted(by_ptr[p] for p in wdst)
    expect = sorted(n for n in by_ptr.values() if "lora_layer" in n or (n.endswith(".weight") and "norm" not in n))
    assert w_names == expect                                     # each exactly once
    zero_w = [n for n in w_names if "zero_convs" in n or "middle_block_out" in n]
    zero_b = [by_ptr[p] for p in bdst]
    print(f"[flags {combo_key(nt, zt)} {dtype}] weight-gradient problems {len(wdst)} (zero convs {len(zero_w)}), "
          f"bias column sums {len(zero_b)}")
    assert len(zero_w) == (13 if zt else 0) and len(w_names) == 164 + (13 if zt else 0)
    assert sorted(zero_b) == sorted(n for n in by_ptr.values() if n.endswith(".bias") and "norm" not in n)
    assert len(zero_b) == (13 if zt else 0)
    # norm gradients: written only when the norms train
    norm_g = [t for t in ex.tr.items if "norm" in t.name and "lora_layer" not in t.name]
    assert len(norm_g) == (56 if nt else 0)
    assert all(float(t.grad.abs().sum()) > 0 for t in norm_g)


# ------------------------------------------------------------------------------ three optimizer steps, eager and graphed

@pytest.mark.parametrize("nt,zt", COMBOS)
def test_three_steps_eager_and_graphed_agree_and_frozen_tensors_never_move(nt, zt):
    """As test_gpu_parity.py::test_graphed_train_step_matches_eager_steps requires (losses within 1e-4 relative, parameters
    within 1e-4 rel-L2), for every selected tensor; every frozen ControlNet tensor stays torch.equal to its loaded value."""
    _need_gpu()
    from ctrlora_amd.train import GraphedTrainStep
    g, meta, cfg, inp, sd_cn, sd_un = _fixture_inputs()
    gold = g["combos"][combo_key(nt, zt)]
    cu = lambda v: v.cuda()
    cond = {"c_crossattn": [cu(inp["ctx"])], "c_concat": [cu(inp["hint_z"])]}
    ma = _model(nt, zt, torch.float32, sd_cn, sd_un, lr=meta["lr"])
    oa = ma.configure_optimizers()
    pa = dict(ma.control_model.named_parameters())
    losses = []
    for step in range(3):
        oa.zero_grad()
        loss, _ = ma.p_losses(cu(inp["z"]), cond, cu(inp["t"]), noise=cu(inp["noise"]))
        loss.backward()
        oa.step()
        losses.append(float(loss))
        if step == 0:       # the reference's AdamW step on the selected tensors
            for n, d in gold["adamw_digest"].items():
                digest_close(pa[n].detach(), d, 1e-5)
    mb = _model(nt, zt, torch.float32, sd_cn, sd_un, lr=meta["lr"])
    ob = mb.configure_optimizers()
    args = (cu(inp["z"]), cu(inp["ctx"]), cu(inp["hint_z"]), cu(inp["t"]), cu(inp["noise"]))
    gs = GraphedTrainStep(mb, ob, *args, warmup=2)                   # steps 1-2 run eagerly inside
    l3 = float(gs(*args))
    torch.cuda.synchronize()
    assert ob._step == 3 and oa._step == 3
    assert abs(l3 - losses[2]) < 1e-4 * abs(losses[2]) and losses[2] != losses[1]
    pb = dict(mb.control_model.named_parameters())
    worst = max((rel_l2(pb[n].detach(), pa[n].detach().cpu()), n) for n in gold["trainable_names"])
    moved = min(rel_l2(pa[n].detach(), sd_cn[n]) for n in gold["trainable_names"])
    print(f"[flags {combo_key(nt, zt)}] graphed vs eager after 3 steps: worst {worst[0]:.3e} ({worst[1]}); least-moved selected "
          f"tensor {moved:.3e}")
    assert worst[0] < 1e-4, worst
    assert moved > 0.0
    for m in (ma, mb):
        for n, p in _frozen_cn(m, nt, zt).items():
            assert torch.equal(p.detach().cpu(), sd_cn[n]), n
        assert _packed_frozen_ok(m.control_model.executor(), sd_cn, nt, zt)


@pytest.mark.parametrize("nt,zt,dtype", [(False, True, torch.float32), (True, False, torch.bfloat16), (False, False, torch.float32),
                                         (False, False, torch.bfloat16)])
def test_segmented_graph_step_hands_out_every_slice_of_the_reduced_buffer_once(nt, zt, dtype):
    """test_gpu_parity.py::test_segmented_graph_step_hands_out_every_gradient_slice_once_and_matches_eager on the reduced
    buffer (stages without a trainable report nothing and cut no segment)."""
    _need_gpu()
    from ctrlora_amd.train import GraphedTrainStep
    g, meta, cfg, inp, sd_cn, sd_un = _fixture_inputs()
    cu = lambda v: v.cuda()
    cond = {"c_crossattn": [cu(inp["ctx"])], "c_concat": [cu(inp["hint_z"])]}
    ma = _model(nt, zt, dtype, sd_cn, sd_un, lr=1e-3)
    oa = ma.configure_optimizers()
    losses = []
    for _ in range(3):
        oa.zero_grad()
        loss, _ = ma.p_losses(cu(inp["z"]), cond, cu(inp["t"]), noise=cu(inp["noise"]))
        loss.backward()
        oa.step()
        losses.append(float(loss))
    mb = _model(nt, zt, dtype, sd_cn, sd_un, lr=1e-3)
    ob = mb.configure_optimizers()
    ex = mb.control_model.executor()
    handed = []

    def fake_reduce(buf):
        off = (buf.data_ptr() - ex.tr.flat_grad.data_ptr()) // 4
        handed.append((off, off + buf.numel()))
        return None

    args = (cu(inp["z"]), cu(inp["ctx"]), cu(inp["hint_z"]), cu(inp["t"]), cu(inp["noise"]))
    gs = GraphedTrainStep(mb, ob, *args, warmup=1, split_graphs="segmented", bucket_bytes=256 << 10, reduce_fn=fake_reduce,
                          capture_error_mode="thread_local")
    assert gs.mode == "segmented" and len(gs.segments) >= 3
    handed.clear()
    l2 = float(gs(*args))
    spans = sorted(handed)
    assert spans[0][0] == 0 and spans[-1][1] == ex.tr.numel
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:])), spans
    assert handed == spans
    l3 = float(gs(*args))
    tol = 1e-4 if dtype == torch.float32 else 2e-3
    assert abs(l2 - losses[1]) < tol * abs(losses[1]) and abs(l3 - losses[2]) < tol * abs(losses[2])
    for n, p in _frozen_cn(mb, nt, zt).items():
        assert torch.equal(p.detach().cpu(), sd_cn[n]), n


# ------------------------------------------------------------------------------ SD1.5 width, LoRA only

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sd15_width_lora_only_vs_oracle(dtype):
    """Both flags off at SD1.5 width, latent 16, on the weights / inputs of the rank-128 fixture (model_sd15.pt: seed 5,
    B = 1): the 246-tensor layout shrinks to the 164 LoRA factors; eps and every gradient against the oracle."""
    _need_gpu()
    import os as _os
    from oracle import arch
    from tests.golden.make_golden import inputs_for
    from tests.util import GOLDEN
    meta = torch.load(_os.path.join(GOLDEN, "model_sd15.pt"), weights_only=False)["meta"]
    cfg = arch.SD15
    inp = inputs_for(cfg, meta["B"], meta["H"], meta["seed"])
    sd_cn = arch.make_state(arch.controlnet_shapes(cfg), meta["seed"])
    sd_un = arch.make_state(arch.unet_shapes(cfg), meta["seed"])
    m = _model(False, False, dtype, sd_cn, sd_un, tiny=False)
    opt = m.configure_optimizers()
    ex = m.control_model.executor()
    names = [t.name for t in ex.tr.items]
    assert len(names) == 164 and all("lora_layer" in n for n in names)
    full = sum((int(torch.tensor(s).prod()) + 63) // 64 * 64 for k, s in arch.controlnet_shapes(cfg).items() if arch.is_trainable(k))
    assert ex.tr.numel < full and ex.tr.numel == sum((t.master.numel() + 63) // 64 * 64 for t in ex.tr.items)
    order = ex.backward_stage_order()
    assert order[0][0] == 0 and order[-1][1] == ex.tr.numel and all(a[1] == b[0] for a, b in zip(order, order[1:]))
    # the bucket plan at its true size: what GradAllReduce launches from the stage hook + the final flush covers the buffer once
    from ctrlora_amd.parallel import GradAllReduce
    launched = []
    dp = GradAllReduce([ex])
    dp.world_size = 2
    dp._launch = lambda e, lo, hi: launched.append((lo, hi)) if hi > lo else None
    m.dp = dp
    cu = lambda v: v.cuda()
    opt.zero_grad()
    m.engine_train_step(cu(inp["z"]), {"c_crossattn": [cu(inp["ctx"])], "c_concat": [cu(inp["hint_z"])]}, cu(inp["t"]),
                        cu(inp["noise"]))
    torch.cuda.synchronize()
    assert launched[0][0] == 0 and launched[-1][1] == ex.tr.numel and all(a[1] == b[0] for a, b in zip(launched, launched[1:]))
    with torch.no_grad():
        eps = m.apply_model(m.q_sample(cu(inp["z"]), cu(inp["t"]), cu(inp["noise"])), cu(inp["t"]),
                            {"c_crossattn": [cu(inp["ctx"])], "c_concat": [cu(inp["hint_z"])]})
    from tests.test_gpu_bench_shapes import K_CMP, K_CMP_MAX, _oracle_on_gpu
    _, eps_o, grads_o = _oracle_on_gpu(cfg, sd_cn, sd_un, inp["z"], inp["t"], inp["ctx"], inp["hint_z"], inp["noise"])
    e = rel_l2(eps, eps_o)
    errs = sorted(((rel_l2(t.grad, grads_o[t.name]), t.name) for t in ex.tr.items), reverse=True)
    med = errs[len(errs) // 2][0]
    print(f"[flags sd15 lora-only {dtype}] buckets {launched}; eps {e:.3e}; gradients worst {errs[0][0]:.3e} ({errs[0][1]}) "
          f"median {med:.3e}")
    if dtype == torch.float32:
        assert e < TOL_EPS_F32 and errs[0][0] < TOL_GRAD_F32, (e, errs[:5])
    else:
        _, eps_c, grads_c = _oracle_on_gpu(cfg, sd_cn, sd_un, inp["z"], inp["t"], inp["ctx"], inp["hint_z"], inp["noise"],
                                           autocast=torch.bfloat16)
        ce = sorted((rel_l2(grads_c[n], grads_o[n]) for n in names), reverse=True)
        c_eps, c_max, c_med = rel_l2(eps_c, eps_o), ce[0], ce[len(ce) // 2]
        print(f"[flags sd15 lora-only bf16 comparator] eps {c_eps:.3e} worst {c_max:.3e} median {c_med:.3e}")
        assert e < K_CMP * c_eps and errs[0][0] < K_CMP_MAX * c_max and med < K_CMP * c_med, (e, errs[0], med, c_eps, c_max, c_med)
    frozen = _frozen_cn(m, False, False)
    assert all(p.grad is None for p in frozen.values())


# ------------------------------------------------------------------------------ scripts end to end

def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    out = str(tmp_path_factory.mktemp("synth_flags"))
    spec = importlib.util.spec_from_file_location("make_synthetic_assets", os.path.join(ROOT, "tests", "tools", "make_synthetic_assets.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    argv, sys.argv = sys.argv, ["make_synthetic_assets.py", "--out", out, "--n", "4"]
    try:
        mod.main()
    finally:
        sys.argv = argv
    return out


def test_finetune_script_with_frozen_norms_checkpoint_resume_extract_and_sample(assets, tmp_path, monkeypatch):
    """tests/test_gpu_scripts.py's finetune row with `norm_trainable: false` in the YAML: train, checkpoint, resume, extract,
    sample; the norm layers keep the Base ControlNet's values through all of it, and a resume with the flag flipped fails."""
    import yaml
    monkeypatch.setenv("CTRLORA_SYNTHETIC_TOKENIZER", "1")
    monkeypatch.chdir(tmp_path)
    with open(os.path.join(assets, "finetune_narrow.yaml")) as f:
        y = yaml.safe_load(f)
    y["model"]["params"]["control_stage_config"]["params"]["norm_trainable"] = False
    cfg = str(tmp_path / "finetune_narrow_frozen_norms.yaml")
    with open(cfg, "w") as f:
        yaml.safe_dump(y, f)
    train = _script("train_ctrlora_finetune")
    args = ["--dataroot", os.path.join(assets, "custom"), "--config", cfg, "--sd_ckpt", os.path.join(assets, "sd_synth.ckpt"),
            "--cn_ckpt", os.path.join(assets, "basecn_synth.ckpt"), "--bs", "2", "--max_steps", "3", "--precision", "16",
            "--ckpt_logger_freq", "2", "--img_logger_freq", "100", "--lr", "1e-4", "-n", "flags", "--num_workers", "0"]
    train.main(args)
    cks = sorted(glob.glob(os.path.join("runs", "flags", "**", "*.ckpt"), recursive=True))
    assert cks, "CheckpointEveryNSteps wrote nothing"
    ck = torch.load(cks[-1], map_location="cpu", weights_only=False)
    assert int(ck["global_step"]) == 3
    base = torch.load(os.path.join(assets, "basecn_synth.ckpt"), map_location="cpu", weights_only=False)
    base = base.get("state_dict", base)
    is_norm = lambda k: k.startswith("control_model.") and "norm" in k and "lora_layer" not in k
    norms = [k for k in ck["state_dict"] if is_norm(k)]
    assert norms and all(k in base for k in norms)
    assert all(torch.equal(ck["state_dict"][k], base[k]) for k in norms), "a frozen norm moved during training"
    zeros = [k for k in ck["state_dict"] if k.startswith("control_model.zero_convs") and k in base]
    assert zeros and any(not torch.equal(ck["state_dict"][k], base[k]) for k in zeros)       # (the zero convs did train)
    st = ck["optimizer_states"][0]
    assert st["format"] == "by_name" and not any("norm" in k and "lora_layer" not in k for k in st["m"][0])
    assert sorted(st["m"][0]) == sorted(k[len("control_model."):] for k in ck["state_dict"]
                                        if k.startswith("control_model.") and selected(k, False, True))
    # ---- resume with the same flags: the fit continues from step 3 to step 4
    from cldm.model import create_model
    from ctrlora_amd.trainer import Trainer
    _, loader = train.build_dataloader(train.get_parser().parse_args(args), 1, 0)
    model2 = create_model(cfg).cpu()
    model2.learning_rate = 1e-4
    tr = Trainer(max_steps=4, precision=16, default_root_dir=os.path.join("runs", "flags_resume"))
    tr.fit(model2, loader, ckpt_path=cks[-1])
    assert tr.global_step == 4 and int(tr.optimizer._step) == 4
    sd2 = model2.state_dict()
    assert all(torch.equal(sd2[k].cpu(), base[k]) for k in norms)
    # ---- resume with the flag flipped, either way: loud
    model3 = create_model(os.path.join(assets, "finetune_narrow.yaml")).cpu()          # norm_trainable: true
    model3.learning_rate = 1e-4
    with pytest.raises(KeyError, match="optimizer state lacks"):
        Trainer(max_steps=4, precision=16, default_root_dir=os.path.join("runs", "flags_flip")).fit(model3, loader, ckpt_path=cks[-1])
    y["model"]["params"]["control_stage_config"]["params"]["zero_trainable"] = False
    cfg_lean = str(tmp_path / "finetune_narrow_lora_only.yaml")
    with open(cfg_lean, "w") as f:
        yaml.safe_dump(y, f)
    model4 = create_model(cfg_lean).cpu()
    model4.learning_rate = 1e-4
    with pytest.raises(KeyError, match="does not train"):
        Trainer(max_steps=4, precision=16, default_root_dir=os.path.join("runs", "flags_flip2")).fit(model4, loader, ckpt_path=cks[-1])
    del model3, model4
    # ---- extract: the file carries the frozen norm values unchanged
    out_w = str(tmp_path / "extracted.ckpt")
    _script("tool_extract_weights").main(["-t", "lora", "--ckpt", cks[-1], "--save_path", out_w])
    ext = torch.load(out_w, map_location="cpu", weights_only=False)
    ext = ext.get("state_dict", ext)
    ext_norms = [k for k in ext if is_norm(k)]
    assert len(ext_norms) == len(norms) and all(torch.equal(ext[k], base[k]) for k in ext_norms)
    # ---- the extracted file loads into ControlNetInference through the api load sequence (base ControlNet, then the LoRA file):
    # bank 0 carries the Base ControlNet's norms (frozen during training) and the TRAINED zero convs, and runs on the engine
    import api
    tools = importlib.util.spec_from_file_location("make_synthetic_assets", os.path.join(ROOT, "tests", "tools", "make_synthetic_assets.py"))
    msa = importlib.util.module_from_spec(tools)
    tools.loader.exec_module(msa)
    cfg_inf = msa.narrow("inference/ctrlora_sd15_rank128_1lora.yaml", str(tmp_path / "inference_narrow.yaml"))
    mi = create_model(cfg_inf).cpu()
    api.CtrLoRA(num_loras=1).load_weights(mi, cn_state_dict=base, lora_state_dicts=[ext])
    bank = mi.control_model.bank_state(0)
    pre = "control_model."
    bank_norms = [k for k in bank if is_norm(pre + k)]
    bank_zero = [k for k in bank if "zero_convs" in k or "middle_block_out" in k]
    assert len(bank_norms) == len(norms) and all(torch.equal(bank[k], base[pre + k]) for k in bank_norms)
    assert bank_zero and all(torch.equal(bank[k], ck["state_dict"][pre + k]) for k in bank_zero)
    assert any(not torch.equal(bank[k], base[pre + k]) for k in bank_zero)
    mi = mi.cuda().eval()
    mi.set_engine_dtype(torch.bfloat16)
    mi.control_model.switch_lora(0)
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        outs_i = mi.control_model(torch.randn(1, 4, 16, 16, generator=gen).cuda(), torch.tensor([500]).cuda(),
                                  torch.randn(1, 77, mi.control_model.context_dim, generator=gen).cuda())
    assert len(outs_i) == 13 and all(torch.isfinite(o).all() and float(o.abs().sum()) > 0 for o in outs_i)
    del mi
    # ---- sample.py's loop on the checkpoint
    sample = _script("sample")
    sargs = sample.get_parser().parse_args(["--dataroot", os.path.join(assets, "custom"), "--config", cfg, "--ckpt", cks[-1],
                                            "--n_samples", "1", "--save_dir", str(tmp_path / "samples"), "--ddim_steps", "4"])
    from cldm.ddim_hacked import DDIMSampler
    from datasets.custom_dataset import CustomDataset
    from torch.utils.data import Subset
    m3 = model2.cuda().eval()
    sample.sample_dataset(m3, DDIMSampler(m3), Subset(CustomDataset(os.path.join(assets, "custom")), range(1)), sargs)
    outs = glob.glob(str(tmp_path / "samples" / "sample" / "*.png"))
    assert outs
    import numpy as np
    from PIL import Image
    img = np.asarray(Image.open(outs[0]))
    assert img.shape[-1] == 3 and img.std() > 0, "the sampled image is constant"
