"""GPU parity at the shipped LoRA ranks 64, 256 and 512 (configs/ctrlora_finetune_sd15_rank{64,256,512}.yaml and
configs/inference/ctrlora_sd15_rank{64,256,512}_1lora.yaml): every other GPU parity row runs at r = 128 or r = 32.

The rank is K2, the length of the second K segment of the fused LoRACompatibleLinear product (cldm/lora.py:285-291), and it steers
dispatch: the x-stationary kernel and the natural-order GEGLU fusion take K2 in {0, 128} only (csrc/gemm.hip, csrc/gemm_xs.hip,
hip.xs_geglu_ok), the launch table keys on K2 (ctrlora_amd/gemm_tuned_gfx950.json: rows chosen on time alone), the ring of a tile
kernel sees ks2 = K2 / KPS stages after ks1 (one stage at 64; more than ks1 at 512 on the 320-wide level), the grouped q | k | v
products multiply the group index by K2, the weight-gradient tiles meet an r-wide edge.

  * whole model, forward + backward, fp32 and bf16, vs fixtures of the UNMODIFIED reference (tests/golden/model_sd15_32_r*.pt,
    `make_golden.py --only-sd15-r{64,256,512}`: SD1.5 width, B = 2, latent 32x32 -> M = 2048 / 512 / 128 / 32), with the launch
    tags (csrc/debug_hooks.h) proving that products with K2 = r ran in both directions;
  * the rank-512 inference executor (largest fold) vs the oracle;
  * kernel level at the production M, with the low-rank branch drawn at the SAME magnitude as the main product (A ~ K^-1/2,
    B ~ r^-1/2), so that one lost 64-column stage of the second segment moves y by 0.25 .. 0.5 instead of 1e-2: fused linear
    forward / data gradient / dA / dB, the second segment alone (W = 0), every row of the launch table with K2 in
    {32, 64, 256, 512}, and the dispatch claims (no x-stationary kernel, no natural-order GEGLU at these ranks) as assertions.

Gates are the project's existing ones (imported where they have a name).  The oracle is the checker only.
"""
import json
import os

import pytest
import torch

from tests.gemm_ref import TOL_F32, TOL_ONE_ROUNDING, _f32_gate, _rel, _tags
from tests.util import GOLDEN, rel_l2
from tests.test_gpu_bench_shapes import (BF16_EPS, BF16_GRAD_MAX, BF16_GRAD_MEDIAN, K_CMP, K_CMP_MAX, _bf, _comparator_vs, _need_gpu,
                                         _netcfg, _record)

pytestmark = pytest.mark.gpu

RANKS = (64, 256, 512)
# (TOL_ONE_ROUNDING = 2.5e-3, one bf16 rounding of the result, and TOL_F32 = 2e-5, fp32-accumulated products of exact operands, live in
# tests/gemm_ref.py with _tags, _rel and _f32_gate: the cl_gemm conformance suite shares them)
# y / dx (5e-3) and dA / dB (8e-3) with the low-rank intermediate itself rounded to bf16: test_lora_fused_linear_production_shapes.
# At these draws the contract (fp32 accumulation, t and u rounded to bf16, bf16 outputs) emulated on the CPU gives 2.0e-3 and
# 1.7e-3 at every rank and shape; the last half-stage of t zeroed gives 0.25 .. 0.50
TOL_Y, TOL_W = 5e-3, 8e-3

SHAPES = [(32768, 320, 320), (8192, 640, 640), (2048, 1280, 1280), (32768, 320, 2560), (32768, 1280, 320), (8 * 77, 768, 320),
          (512, 1280, 1280), (8, 1280, 1280)]
SQUARE = SHAPES[:3]


# ------------------------------------------------------------------------------ whole model, forward + backward, per rank

@pytest.mark.parametrize("rank,dtype", [pytest.param(r, d, id=f"{r}-{str(d).split('.')[1]}") for r in RANKS
                                        for d in (torch.float32, torch.bfloat16)])
def test_sd15_latent32_forward_backward_vs_reference_golden_at_rank(rank, dtype):
    """SD1.5 width at rank 64 / 256 / 512, B = 2, latent 32x32 (M = 2048 / 512 / 128 / 32 rows per level: more than one row
    tile at the top, the ragged small-M launch paths at the bottom): eps, loss and all 246 trainable gradients vs the
    unmodified reference's, structured as test_rank32_sd15_latent64_bs1_forward_backward_vs_reference_golden.

    Measured on an MI355X (eps / worst gradient / median gradient / worst norm): fp32 1e-6 / 5e-6 / 2e-6 / 1e-6 at all three
    ranks.  bf16, with the bf16-autocast oracle of the same test in brackets: rank 64 9.1e-3 / 3.8e-2 / 1.53e-2 / 4.7e-3
    [1.13e-2 / 4.5e-2 / 1.70e-2]; rank 256 9.5e-3 / 3.8e-2 / 1.35e-2 / 2.8e-3 [1.16e-2 / 4.6e-2 / 1.55e-2]; rank 512 9.8e-3 /
    3.8e-2 / 1.54e-2 / 4.3e-3 [1.20e-2 / 4.7e-2 / 1.74e-2].  The fixtures hold 224 sampled entries per gradient: over 64 the
    sampled rel-L2 of dB [10240, 512] of middle_block.1 ff.net.0.proj read 7.2e-2 (comparator 6.4e-2) where the WHOLE tensor, against
    the fp32 engine, is at 3.2e-2 (comparator 3.7e-2; worst whole tensor 3.7e-2 / 4.0e-2, the engine below the comparator on all
    246) -- an estimator too noisy for a maximum over 246 tensors, not an error of the step."""
    _need_gpu()
    from dataclasses import replace
    from ctrlora_amd.engine import CtrLoRAEngine
    from oracle import arch, ref_model as R
    from tests.golden.make_golden import inputs_for
    gold = torch.load(os.path.join(GOLDEN, f"model_sd15_32_r{rank}.pt"), weights_only=False)
    meta = gold["meta"]
    assert (meta["B"], meta["H"], meta["cfg"]["lora_rank"]) == (2, 32, rank)
    cfg = replace(arch.SD15, lora_rank=rank)
    inp = inputs_for(cfg, meta["B"], meta["H"], meta["seed"])
    sd_cn = arch.make_state(arch.controlnet_shapes(cfg), meta["seed"])
    sd_un = arch.make_state(arch.unet_shapes(cfg), meta["seed"])
    eng = CtrLoRAEngine(sd_un, [sd_cn], _netcfg(cfg), dtype=dtype, device="cuda")
    x_noisy = R.q_sample(R.make_schedule(), inp["z"], inp["t"], inp["noise"])
    assert torch.equal(x_noisy, gold["x_noisy"])
    cu = lambda v: v.cuda()
    with _tags() as tags:
        eps = eng.forward(cu(x_noisy), cu(inp["t"]), cu(inp["ctx"]), [cu(inp["hint_z"])], record=True)
        torch.cuda.synchronize()
        n_fwd, sigs_fwd = tags.launches(K2=rank)
        e_eps = rel_l2(eps, gold["eps"])
        loss = float(((eps.cpu() - inp["noise"]) ** 2).mean())
        eng.zero_grad()
        tags.restart()
        eng.backward(2.0 * (eps - cu(inp["noise"])) / eps.numel())
        torch.cuda.synchronize()
        n_bwd, sigs_bwd = tags.launches(K2=rank)
    # the rank reached the kernels in both directions (y = x W^T + t B^T and dx = dy W + u A carry it as K2): no merged-weight
    # path ran in its place
    assert sigs_fwd < 255 and sigs_bwd < 255, (sigs_fwd, sigs_bwd)
    assert n_fwd >= 1 and n_bwd >= 1, (n_fwd, n_bwd)
    gs = gold["grad_sampled"]
    items = eng.controls[0].tr.items
    assert len(items) == 246 and set(t.name for t in items) == set(gs)
    errs, norm_errs = [], []
    for t in items:
        g = gs[t.name]
        got = t.grad.detach().float().flatten().cpu()
        assert list(t.grad.shape) == g["shape"]
        errs.append((rel_l2(got[g["idx"]], g["vals"]), t.name))
        norm_errs.append(abs(float(got.double().norm()) - g["l2"]) / (g["l2"] + 1e-30))
    errs.sort(reverse=True)
    med = errs[len(errs) // 2][0]
    _record(f"sd15_32_rank{rank}_vs_reference", dtype=str(dtype), eps=e_eps, loss=loss, loss_ref=gold["loss"],
            grad_max=errs[0][0], grad_max_name=errs[0][1], grad_median=med, grad_norm_max=max(norm_errs),
            launches_k2_fwd=n_fwd, launches_k2_bwd=n_bwd, signatures_fwd=sigs_fwd, signatures_bwd=sigs_bwd)
    if dtype == torch.float32:
        assert e_eps < 1e-4 and abs(loss - gold["loss"]) < 1e-4 * gold["loss"], (e_eps, loss, gold["loss"])
        assert errs[0][0] < 5e-4 and max(norm_errs) < 5e-4, (errs[:5], max(norm_errs))
    else:
        # gate = k x the bf16-autocast oracle's error against the same reference tensors, measured here
        c_eps, c_max, c_med = _comparator_vs(
            gold["eps"], lambda n, g: rel_l2(g.flatten().cpu()[gs[n]["idx"]], gs[n]["vals"]), cfg, sd_cn, sd_un,
            inp["z"], inp["t"], inp["ctx"], inp["hint_z"], inp["noise"])
        _record(f"sd15_32_rank{rank}_comparator", eps=c_eps, grad_max=c_max, grad_median=c_med)
        assert e_eps < K_CMP * c_eps and errs[0][0] < K_CMP_MAX * c_max and med < K_CMP * c_med, (e_eps, errs[0], med, c_eps, c_max, c_med)
        assert e_eps < BF16_EPS and abs(loss - gold["loss"]) < 2e-2 * gold["loss"], (e_eps, loss, gold["loss"])
        assert errs[0][0] < BF16_GRAD_MAX and med < BF16_GRAD_MEDIAN and max(norm_errs) < BF16_GRAD_MAX, (errs[:5], med, max(norm_errs))


def test_inference_executor_rank512_latent32_eps_vs_oracle():
    """inference/ctrlora_sd15_rank512_1lora.yaml (the largest fold: Wm = W + B A over r = 512): eps of the inference executor at
    latent 32x32, B = 4, with and without the context K/V cache, vs the fp32 oracle; the bf16-autocast oracle beside it.  Same
    form and gates as test_inference_executor_sd15_latent64_eps_vs_oracle."""
    _need_gpu()
    import bench
    from ldm.models.diffusion.guided_loop import context_kv
    from oracle import arch
    from tests.test_gpu_parity_r3 import _oracle_eps
    from dataclasses import replace
    cfg = replace(arch.SD15, lora_rank=512)
    model = bench.build_model("inference/ctrlora_sd15_rank512_1lora.yaml", 0).cuda().eval()
    model.set_engine_dtype(torch.bfloat16)
    sd_cn = {k: v.detach().clone() for k, v in model.control_model.bank_state(0).items()}
    sd_un = {k: v.detach().clone() for k, v in model.model.diffusion_model.state_dict().items()}
    downs = [v for k, v in sd_cn.items() if k.endswith("lora_layer.down.weight")]
    assert downs and all(v.shape[0] == 512 for v in downs)
    eng = model.engine()
    assert all(cn.merge_lora for cn in eng.controls) and eng.controls[0]._b.linears[0].W32 is not None
    g = torch.Generator().manual_seed(23)
    B, H = 4, 32
    x, hint = torch.randn(B, 4, H, H, generator=g).cuda(), (torch.randn(B, 4, H, H, generator=g) * 0.9).cuda()
    ctx = torch.randn(B, 77, cfg.context_dim, generator=g).cuda()
    t = torch.randint(0, 1000, (B,), generator=g).cuda()
    cond = {"c_concat": [hint], "c_crossattn": [ctx]}
    eps = model.apply_model(x, t, cond)
    ref = _oracle_eps(cfg, sd_cn, sd_un, x, t, ctx, hint)
    e = rel_l2(eps, ref)
    with context_kv(eng):
        model.apply_model(x, t, cond)
        eps_kv = model.apply_model(x, t, cond)
    e_kv = rel_l2(eps_kv, ref)
    cmp_ = rel_l2(_oracle_eps(cfg, sd_cn, sd_un, x, t, ctx, hint, autocast=True), ref)
    _record("inference_rank512_eps_vs_oracle", B=B, H=H, eps=e, eps_kv_cached=e_kv, comparator_bf16_autocast=cmp_)
    assert e < BF16_EPS and e_kv < BF16_EPS, (e, e_kv)
    assert rel_l2(eps_kv, eps) < 1e-6
    assert e < 1.3 * cmp_ + 1e-3, (e, cmp_)


# ------------------------------------------------------------------------------ fused LoRA linear at the production M

def _lora_linear(M, K, N, r, dtype, zero_main=False):
    """One LoRACompatibleLinear through the engine's own calls.  Returns the packed operands (what the kernels read) and outputs."""
    from ctrlora_amd.engine.blocks import Ctx, linear_bwd_data, linear_bwd_lora, linear_fwd
    from ctrlora_amd.engine.packing import LinearW, TrainableSet
    g = torch.Generator().manual_seed(M + K + N + r)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    bias = torch.randn(N, generator=g) * 0.1
    A = torch.randn(r, K, generator=g) / K ** 0.5            # t = x A^T ~ N(0, 1)
    Bm = torch.randn(N, r, generator=g) / r ** 0.5           # t B^T ~ N(0, 1): the variance of x W^T
    if zero_main:
        W, bias = torch.zeros(N, K), torch.zeros(N)
    tr = TrainableSet()
    L = LinearW(W, bias, dtype, "cuda", True)
    tA, tB = tr.declare("a", A.shape), tr.declare("b", Bm.shape)
    L.attach_lora(tA, tB, "cuda")
    tr.materialize({"a": A, "b": Bm}, "cuda")
    L.repack()
    assert L.r == r and tuple(L.A.shape) == (r, K) and tuple(L.B.shape) == (N, r) and L.A.dtype == dtype
    ctx = Ctx(dtype, torch.device("cuda"), True)
    x = torch.randn(M, K, generator=g)
    dy = torch.randn(M, N, generator=g)
    x, dy = (_bf(x).cuda(), _bf(dy).cuda()) if dtype == torch.bfloat16 else (x.cuda(), dy.cuda())
    y, t = linear_fwd(ctx, L, x)
    out = dict(L=L, x=x, dy=dy, y=y, t=t)
    if not zero_main:
        dx, u = linear_bwd_data(ctx, L, dy)
        linear_bwd_lora(ctx, L, x, t, dy, u)
        ctx.flush_wgrad()
        out.update(dx=dx, u=u, dA=tA.grad, dB=tB.grad)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("M,K,N,dtype", [(M, K, N, torch.bfloat16) for M, K, N in SHAPES] + [(M, K, N, torch.float32) for M, K, N in SQUARE],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_lora_fused_linear_full_magnitude_branch(M, K, N, dtype, r):
    """LoRACompatibleLinear forward / data gradient / dA / dB (linear_fwd, linear_bwd_data, linear_bwd_lora + flush_wgrad) at the
    (M, K, N) of test_lora_fused_linear_production_shapes for r = 64 / 256 / 512, the low-rank branch at the magnitude of the main
    product.  (1) vs fp64 of the whole expression on the same operands: the existing 5e-3 / 8e-3 (bf16; t and u are themselves
    rounded) and 2e-5 (fp32).  (2) vs fp64 on the kernel's OWN t and u: y and dx are then one rounding away (2.5e-3), and
    dA = u^T x, dB = dy^T t are pure fp32-accumulated products of exact operands (2e-5, see _f32_gate)."""
    _need_gpu()
    from ctrlora_amd import hip
    with _tags() as tags:
        o = _lora_linear(M, K, N, r, dtype)
        n_k2, _ = tags.launches(K2=r, M=M)
    assert n_k2 >= 2, n_k2                              # the forward product and the data gradient both carried K2 = r
    L, x, dy, t, u = o["L"], o["x"], o["dy"], o["t"], o["u"]
    W64, A64, B64, b64 = L.W.double(), L.A.double(), L.B.double(), L.bias.double()
    x64, dy64, t64, u64 = x.double(), dy.double(), t.double(), u.double()
    # (1) the whole expression
    t_ref, u_ref = x64 @ A64.t(), dy64 @ B64
    whole = dict(y=_rel(o["y"], x64 @ W64.t() + b64 + t_ref @ B64.t()), dx=_rel(o["dx"], dy64 @ W64 + u_ref @ A64),
                 dA=_rel(o["dA"], u_ref.t() @ x64), dB=_rel(o["dB"], dy64.t() @ t_ref))
    # (2) on the kernel's own intermediates
    own = dict(t=_rel(t, t_ref), u=_rel(u, u_ref), y=_rel(o["y"], x64 @ W64.t() + b64 + t64 @ B64.t()),
               dx=_rel(o["dx"], dy64 @ W64 + u64 @ A64))
    own["dA"], gate_dA, torch_dA = _f32_gate(o["dA"], u64.t() @ x64, u.t(), x)
    own["dB"], gate_dB, torch_dB = _f32_gate(o["dB"], dy64.t() @ t64, dy.t(), t)
    rec = dict(shape=[M, K, N, r], dtype=str(dtype), whole=whole, own=own, gate_dA=gate_dA, gate_dB=gate_dB,
               torch_f32_dA=torch_dA, torch_f32_dB=torch_dB)
    if dtype == torch.bfloat16:
        _record("lora_linear_ranks", **rec)
        assert whole["y"] < TOL_Y and whole["dx"] < TOL_Y and whole["dA"] < TOL_W and whole["dB"] < TOL_W, whole
        assert max(own["t"], own["u"], own["y"], own["dx"]) < TOL_ONE_ROUNDING, own
        assert own["dA"] < gate_dA and own["dB"] < gate_dB, (own, gate_dA, gate_dB)
    else:
        # fp32 engine mode (other templates): every output is an fp32-accumulated product; same reference, 2e-5 on all four
        gy = _f32_gate(o["y"], x64 @ W64.t() + b64 + t64 @ B64.t(), torch.cat([x, t], 1), torch.cat([L.W, L.B], 1).t())
        gx = _f32_gate(o["dx"], dy64 @ W64 + u64 @ A64, torch.cat([dy, u], 1), torch.cat([L.W, L.A], 0))
        rec.update(gate_y=gy[1], gate_dx=gx[1], torch_f32_y=gy[2], torch_f32_dx=gx[2])
        _record("lora_linear_ranks", **rec)
        assert own["y"] < gy[1] and own["dx"] < gx[1] and own["dA"] < gate_dA and own["dB"] < gate_dB, (own, gy, gx, gate_dA, gate_dB)
        assert whole["y"] < gy[1] and whole["dx"] < gx[1] and whole["dA"] < gate_dA and whole["dB"] < gate_dB, (whole, gy, gx, gate_dA, gate_dB)
        assert own["t"] < TOL_F32 and own["u"] < TOL_F32, own


@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("M,K,N", SHAPES)
def test_lora_second_segment_in_isolation(M, K, N, r):
    """W = 0 and bias = 0: y = t B^T exactly, every stage of the second K segment is the whole signal (the first segment still
    runs its ks1 stages, on zeros).  vs fp64 on the kernel's own bf16 t: one output rounding."""
    _need_gpu()
    with _tags() as tags:
        o = _lora_linear(M, K, N, r, torch.bfloat16, zero_main=True)
        n_k2, _ = tags.launches(K2=r, M=M, N=N, K1=K)
    assert n_k2 == 1, n_k2
    L = o["L"]
    assert float(L.W.abs().max()) == 0.0 and float(L.bias.abs().max()) == 0.0
    e_t = _rel(o["t"], o["x"].double() @ L.A.double().t())
    e_y = _rel(o["y"], o["t"].double() @ L.B.double().t())
    _record("lora_second_segment_alone", shape=[M, K, N, r], t=e_t, y=e_y)
    assert e_t < TOL_ONE_ROUNDING and e_y < TOL_ONE_ROUNDING, (e_t, e_y)


# ------------------------------------------------------------------------------ every tabled signature of these ranks

def _table_rows():
    from ctrlora_amd import hip
    with open(hip.GEMM_TABLE_PATH) as f:
        return [tuple(int(v) for v in row[:9]) for row in json.load(f)["entries"] if int(row[5]) in (32,) + RANKS]


_ROWS = _table_rows()


def test_launch_table_holds_rows_of_these_ranks():
    assert _ROWS and {row[5] for row in _ROWS} >= set(RANKS), sorted({row[5] for row in _ROWS})


@pytest.mark.parametrize("row", _ROWS, ids=lambda r: "-".join(str(v) for v in r))
def test_tabled_signature_of_a_lora_rank_vs_fp64(row):
    """Every row [dtype, mode, M, N, K1, K2, geglu, cfg, splitk] of ctrlora_amd/gemm_tuned_gfx950.json with K2 in
    {32, 64, 256, 512} -- (cfg, splitk) pairs the autotuner chose on time alone -- launched as exactly that product, with the
    table loaded as the engine loads it, vs fp64 on the same operands (the second segment at full magnitude).  Read from the
    file: rows of a later tuning run are covered without an edit."""
    _need_gpu()
    from ctrlora_amd import hip
    dtype_id, mode, M, N, K1, K2, geglu, cfg, sk = row
    assert mode == hip.LINEAR, "a second K segment exists in linear mode only (csrc/gemm.hip)"
    assert not geglu, "a GEGLU row of these ranks: extend this test with the permuted-row reference (packing.LinearW.geglu_pack)"
    assert os.environ.get("CTRLORA_GEMM_TUNED", "1") != "0" and "CTRLORA_GEMM_TABLE" not in os.environ
    assert hip.lib().cl_gemm_tune_size() >= len(_ROWS)
    dtype = {hip.BF16: torch.bfloat16, hip.F32: torch.float32}[dtype_id]
    g = torch.Generator().manual_seed(M + N + K1 + K2)
    mk = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(dtype).cuda()
    x, W, A, B2 = mk(M, K1), mk(N, K1, sc=K1 ** -0.5), mk(K2, K1, sc=K1 ** -0.5), mk(N, K2, sc=K2 ** -0.5)
    t = torch.empty(M, K2, dtype=dtype, device="cuda")
    y = torch.full((M, N), float("nan"), dtype=dtype, device="cuda")
    hip.gemm(x, A, t)
    with _tags() as tags:
        hip.gemm(x, W, y, a2=t, w2=B2)
        torch.cuda.synchronize()
        n, _ = tags.launches(dtype=dtype_id, mode=mode, M=M, N=N, K1=K1, K2=K2, act=hip.ACT_NONE, residual=0)
    assert n == 1, (n, hip.gemm_tags())
    ref = x.double() @ W.double().t() + t.double() @ B2.double().t()
    e_t = _rel(t, x.double() @ A.double().t())
    if dtype == torch.bfloat16:
        e, gate, e_torch = _rel(y, ref), TOL_ONE_ROUNDING, None
    else:
        e, gate, e_torch = _f32_gate(y, ref, torch.cat([x, t], 1), torch.cat([W, B2], 1).t())
    _record("tabled_signature", row=list(row), y=e, t=e_t, gate=gate, torch_f32=e_torch)
    assert e < gate and e_t < gate, (e, e_t, gate)


# ------------------------------------------------------------------------------ dispatch claims

def test_no_x_stationary_kernel_and_no_natural_order_geglu_at_these_ranks():
    """The x-stationary kernel (csrc/gemm_xs.hip) has instances for K2 in {0, 128} only.  (1) hip.xs_geglu_ok says so; (2) a
    launch-table entry (here: the forced configuration 34) naming it for K1 in {320, 640} with K2 = 64 / 256 / 512 costs speed,
    never correctness: the built-in rules run the product; (3) ACT_GEGLU_SPLIT, which only that kernel computes, is refused
    (include/ctrlora_hip.h: cl_gemm_params.act)."""
    _need_gpu()
    from ctrlora_amd import hip
    L = hip.lib()
    for r in RANKS:
        for K in (320, 640):
            for M in (128, 2048, 8192, 32768, 131072):
                assert not hip.xs_geglu_ok(M, K, r), (M, K, r)
    assert hip.XS_ENABLED and hip.xs_geglu_ok(32768, 320, 128) and hip.xs_geglu_ok(32768, 320, 0)     # (the claim is about the rank)
    g = torch.Generator().manual_seed(7)
    mk = lambda *s, sc=1.0: _bf(torch.randn(*s, generator=g) * sc).cuda()
    M = 4096
    for K1 in (320, 640):
        for r in RANKS:
            N = 4 * K1
            x, W, A, B2, bias = mk(M, K1), mk(N, K1, sc=K1 ** -0.5), mk(r, K1, sc=K1 ** -0.5), mk(N, r, sc=r ** -0.5), torch.randn(N, generator=g).cuda()
            t = torch.empty(M, r, dtype=torch.bfloat16, device="cuda")
            hip.gemm(x, A, t)
            y = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device="cuda")
            try:
                L.cl_gemm_force_config(34)
                hip.gemm(x, W, y, a2=t, w2=B2, bias=bias)
            finally:
                L.cl_gemm_force_config(-1)
            torch.cuda.synchronize()
            e = _rel(y, x.double() @ W.double().t() + t.double() @ B2.double().t() + bias.double())
            _record("xs_forced_falls_back", shape=[M, K1, N, r], y=e)
            assert e < TOL_ONE_ROUNDING, (K1, r, e)
            half = torch.empty(M, N // 2, dtype=torch.bfloat16, device="cuda")
            with pytest.raises(hip.HipError):
                hip.gemm(x, W, half, a2=t, w2=B2, bias=bias, act=hip.ACT_GEGLU_SPLIT, N=N)
