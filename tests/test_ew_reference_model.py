"""The fp64 contract, the rounding model, the gates, the host-logic transcription and the case table of the elementwise / layout
conformance suite, on the CPU (tests/ew_ref.py; the GPU half is tests/test_gpu_ew_conformance.py).

  * the closed forms match fp64 autograd (GEGLU, SiLU, the MSE gradient) and oracle.ref_model (timestep_embedding, q_sample,
    ddim_step, adamw_step);
  * the rounding model passes its tier on every row, and needs no more than the constants the module records;
  * the table reaches the required set of forms (a deleted row fails);
  * negative controls: each planted defect is flagged;
  * every refusal of the launchers is decided on the host.
"""
import ctypes
import math

import torch

from tests import ew_ref as R

BF, F32 = R.BF, R.F32
ROW = {r["name"]: r for r in R.CASES}


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


def test_closed_forms_match_fp64_autograd():
    F = torch.nn.functional
    row = ROW["geglu_bwd-257x320"]
    ops = R.make_ops(row, F32)
    h = ops["h"].double().requires_grad_(True)
    a, g = h[:, :320], h[:, 320:]
    y = a * F.gelu(g)
    y.backward(ops["dout"].double())
    assert _rel(R.evaluate(ROW["geglu_fwd-257x320"], F32, R.make_ops(ROW["geglu_fwd-257x320"], F32))["out"]["ref"],
                (lambda o: o["h"].double()[:, :320] * F.gelu(o["h"].double()[:, 320:]))(R.make_ops(ROW["geglu_fwd-257x320"], F32))) < 1e-14
    assert _rel(R.evaluate(row, F32, ops)["dh"]["ref"], h.grad) < 1e-13
    row = ROW["silu_bwd-257x320"]
    ops = R.make_ops(row, F32)
    x = ops["x"].double().requires_grad_(True)
    y = F.silu(x)
    y.backward(ops["dy"].double())
    assert _rel(R.evaluate(row, F32, ops)["dx"]["ref"], x.grad) < 1e-13
    assert _rel(R.eval_silu_fwd(row["p"], F32, ops)["y"]["ref"], y.detach()) < 1e-14
    row = ROW["mse-1280-d1"]
    ops = R.make_ops(row, F32)
    e = ops["eps"].double().requires_grad_(True)
    loss = F.mse_loss(e, ops["target"].double())
    (loss * row["p"]["gscale"]).backward()
    sp = R.evaluate(row, F32, ops)
    assert _rel(sp["loss"]["ref"], loss.detach().reshape(1)) < 1e-14 and _rel(sp["d_eps"]["ref"], e.grad) < 1e-14
    row = ROW["plosses-3x4117"]
    ops = R.make_ops(row, F32)
    e = ops["eps"].double().requires_grad_(True)
    ls = ((e - ops["target"].double()) ** 2).mean(1).mean()
    (ls * row["p"]["w_simple"] * row["p"]["gscale"]).backward()
    sp = R.eval_plosses(dict(row["p"], d_eps=True), F32, ops)
    assert _rel(sp["out"]["ref"][0], ls.detach()) < 1e-14 and _rel(sp["d_eps"]["ref"], e.grad) < 1e-14


def test_closed_forms_match_the_oracle():
    from oracle import ref_model as O
    row = ROW["timestep-5x160"]
    ops = R.make_ops(row, F32)
    want = O.timestep_embedding(ops["t"], 320)
    sp = R.eval_timestep(row["p"], F32, ops)["out"]
    assert torch.equal(ops["freqs"], torch.exp(-math.log(10000.0) * torch.arange(0, 160, dtype=torch.float32) / 160))
    assert float((sp["ref"] - want.double()).abs().max()) < R.TSTEP_ABS
    row = ROW["qsample-3x1000"]
    ops = R.make_ops(row, F32)
    sched = O.make_schedule()
    assert _rel(ops["sqrt_ac"], sched["sqrt_alphas_cumprod"]) < 1e-7 and _rel(ops["sqrt_1mac"], sched["sqrt_one_minus_alphas_cumprod"]) < 1e-7
    own = dict(sqrt_alphas_cumprod=ops["sqrt_ac"], sqrt_one_minus_alphas_cumprod=ops["sqrt_1mac"])
    want = O.q_sample(own, ops["z"].reshape(3, 1000, 1, 1), ops["t"], ops["noise"].reshape(3, 1000, 1, 1)).reshape(3, 1000)
    assert R.same_bits(R.evaluate(row, F32, ops)["out"]["exact"], want)
    ds = O.make_ddim_schedule(sched, 20, eta=0.5)
    coef, ts = R.ddim_table(20, 0.5)
    assert torch.equal(ts, torch.as_tensor(ds["timesteps"])) and _rel(coef[:, 0], ds["alphas"]) < 1e-7
    assert _rel(coef[:, 1], torch.as_tensor(ds["alphas_prev"])) < 1e-7 and _rel(coef[:, 2], torch.as_tensor(ds["sigmas"])) < 1e-6
    for name in ("ddim-1000-i19-a0", "ddim-1000-i0-a1", "ddim-1000-i0-a0", "ddim-1000-i19-a1"):
        row = ROW[name]
        p, ops = row["p"], R.make_ops(row, F32)
        c = ops["coef"][p["index"]]
        xp, p0 = O.ddim_step(ops["x"].double(), ops["e_c"].double(), ops["e_u"].double() if p["e_u"] else None, p["scale"], c[0], c[1], c[2], c[3],
                             ops["noise"].double() if p["noise"] else None)
        sp = R.evaluate(row, F32, ops)
        assert _rel(sp["x_prev"]["ref"], xp) < 1e-6, name          # (the oracle takes sqrt of the fp32 coefficients in fp32)
        if p["pred_x0"]:
            assert _rel(sp["pred_x0"]["ref"], p0) < 1e-6
    row = ROW["adamw-1000"]
    ops = R.make_ops(row, F32)
    H = {k: float(torch.tensor(v, dtype=torch.float32)) for k, v in R.ADAMW_HYPER.items()}      # the hyper-parameters as stored
    st = (ops["p"], ops["m"], ops["v"])
    for step in (1, 2, 3):
        sp = R.eval_adamw_step(st, ops["g"], step)
        p1, m1, v1 = O.adamw_step(st[0].double(), ops["g"].double() * H["gscale"], st[1].double(), st[2].double(), step, H["lr"], H["beta1"], H["beta2"],
                                  H["eps"], H["wd"])
        assert _rel(sp["p"]["ref"], p1) < 1e-7 and _rel(sp["m"]["ref"], m1) < 1e-7 and _rel(sp["v"]["ref"], v1) < 1e-6
        st = tuple(sp[k]["model"] for k in ("p", "m", "v"))


def test_rounding_model_passes_every_row_within_the_recorded_constants():
    worst = R.measure_constants()
    for fam, (need, who) in worst.items():
        print(fam, "need", round(need, 3), who, "recorded", R.MEASURED[fam], "need / c", need / R.C_GATE[fam] if R.C_GATE[fam] else 0.0)
        # the recorded constant is what was measured (same draws on every machine; 2 % for a different libm)
        assert need <= R.MEASURED[fam] * 1.02 + 1e-9, (fam, need, who)
        assert need >= R.MEASURED[fam] * 0.5, (fam, need, who)
        assert need <= R.C_GATE[fam] / R.MARGIN * 1.02 + 1e-9
    # and with the gate's own constants: every row of every tier, zero violations, exact rows bit for bit
    for row in R.CASES:
        for dt in row["dtypes"]:
            if dt is None or row["kern"] not in R.EVAL or "wrap" in row["tags"]:
                continue
            ops = R.make_ops(row, dt)
            sp = R.evaluate(row, dt, ops)
            got = {k: (s["exact"] if "exact" in s else s["model"]) for k, s in sp.items()}
            assert not R.failures(R.check(sp, got)), row["name"]


def test_table_reaches_the_required_forms():
    got = R.covered_forms()
    assert R.REQUIRED_FORMS <= got, sorted(R.REQUIRED_FORMS - got, key=str)
    # a deleted row is noticed
    for victim, form in ((lambda r: r["name"].startswith("colsum-600x3x8"), ("colsum", "B>512")),
                         (lambda r: r["name"].startswith("colsum-2x70x2056"), ("colsum", "c8>256")),
                         (lambda r: r["kern"] == "plosses" and r["p"]["per"] < 16, ("plosses", "empty_chunk")),
                         (lambda r: r["kern"] == "plosses" and r["p"]["per"] > 4096, ("plosses", "multi_trip")),
                         (lambda r: r["name"] == "vit_patch-nopair", ("vit_patch_rows", "nopair")),
                         (lambda r: r["name"].startswith("mse-65836"), ("mse", "cap256"))):
        rows = [r for r in R.CASES if not victim(r)]
        assert len(rows) < len(R.CASES) and form not in R.covered_forms(rows), form
    # the transcription on the shapes the issue names
    f = R.colsum_form(1, 5000, 320, 64 << 20)
    assert (f["VX"], f["PY"], f["dead"], f["nchunk"], f["partial"]) == (40, 6, 16, 79, True)
    assert R.colsum_form(2, 70, 2056, 0)["passes"] == 2 and R.colsum_form(600, 3, 8, 64 << 20)["nchunk"] == 1
    assert R.zero_form(3, 33) == dict(head=13, nvec=1, tail=4, grid=1) and R.zero_form(9, 5) == dict(head=5, nvec=0, tail=0, grid=1)
    assert R.ew_grid(R.WRAP) == 4096 and not R.wraps(R.WRAP) and R.wraps(R.WRAP + 1) and R.mse_blocks(65836) == 256
    assert R.plosses_chunks(15).count((0, 0)) == 1 and max(b - a for a, b in R.plosses_chunks(4117)) > 256


def _flagged(row, dt, name, got, ops=None):
    ops = R.make_ops(row, dt) if ops is None else ops
    sp = R.evaluate(row, dt, ops)
    full = {k: (s["exact"] if "exact" in s else s["model"]) for k, s in sp.items()}
    assert not R.failures(R.check(sp, full)), "the control's baseline must pass"
    full[name] = got
    return bool(R.failures(R.check(sp, full)))


def test_negative_controls():
    # a transpose that skips its last ragged row
    row = ROW["transpose-f32bf16-3x65x63-pad72"]
    ops = R.make_ops(row, BF)
    good = R.evaluate(row, BF, ops)["out"]["exact"].clone()
    good[:, :, 64] = 0
    assert _flagged(row, BF, "out", good, ops)
    for dt in (BF, F32):
        # a geglu that swaps the halves; tanh-GELU instead of erf
        row = ROW["geglu_fwd-257x320"]
        ops = R.make_ops(row, dt)
        a, g = ops["h"][:, :320].float(), ops["h"][:, 320:].float()
        assert _flagged(row, dt, "out", (g * R._gelu32(a)).to(dt), ops)
        assert _flagged(row, dt, "out", (a * torch.nn.functional.gelu(g, approximate="tanh")).to(dt), ops)
        # a softmax that normalises over N rounded up to 1024 (the pad reads as score 0)
        row = ROW["softmax-5x1020-s1.000"]
        ops = R.make_ops(row, dt)
        s = torch.cat([ops["S"], torch.zeros(5, 4)], 1)
        assert _flagged(row, dt, "P", torch.softmax(s, 1)[:, :1020].to(dt), ops)
        # a colsum that misses the last chunk
        row = ROW["colsum-3x65x24-ws1-gauss"]
        ops = R.make_ops(row, dt)
        x = ops["in"].float().reshape(3, 65, 24)
        assert _flagged(row, dt, "out", ops["out0"] + 0.5 * x[:, :64].sum(1), ops)
        # a beta = 0 path that multiplies the old output (NaN-filled)
        row = ROW["tok_to_nchw-set-3x63x65"]
        ops = R.make_ops(row, dt)
        good = R.evaluate(row, dt, ops)["out"]["exact"]
        assert _flagged(row, dt, "out", good + 0.0 * torch.full_like(good, float("nan")), ops)
        # one element 4 output ulps off (z = 20: the planted element)
        row = ROW["silu_fwd-3x24"]
        ops = R.make_ops(row, dt)
        y = R.evaluate(row, dt, ops)["y"]["model"].clone()
        R.bits(y)[0, 0] += 4
        assert float(ops["x"][0, 0]) == 20.0 and _flagged(row, dt, "y", y, ops)
        row = ROW["tok_to_nchw-acc-3x63x65"]
        ops = R.make_ops(row, dt)
        y = R.evaluate(row, dt, ops)["out"]["model"].clone()
        R.bits(y)[1, 7, 3] += 4
        assert _flagged(row, dt, "out", y, ops)
    # a plosses that drops the remainder per % 16
    row = ROW["plosses-3x4117"]
    ops = R.make_ops(row, F32)
    d = (ops["eps"] - ops["target"])[:, :4117 - 4117 % 16]
    sb = (d * d).sum(1) / 4117
    sp = R.eval_plosses(dict(row["p"], per_sample=True), F32, ops)
    assert R.failures(R.check(sp, dict(per_sample=sb)))
    # a truncating, not RNE, bf16 conversion on the tie row
    row = ROW["pack2d-77x320-pad325"]
    ops = R.make_ops(row, BF)
    trunc = torch.zeros(77, 325, dtype=BF)
    trunc[:, :320] = (ops["in"].view(torch.int32) & -65536).view(F32).to(BF)
    assert _flagged(row, BF, "out", trunc, ops)
    assert float(ops["in"].reshape(-1)[7]) == 1.01171875 and float(R.evaluate(row, BF, ops)["out"]["exact"].reshape(-1)[7]) == 1.015625
    # a pad column written: the canary of tests/gemm_ref.Guarded
    g = R.Guarded(3, 8, BF, "cpu")
    g.view.fill_(1.0)
    assert g.check() == dict(guard_rows=0, pad_elems=0, nan_left=0)
    g.buf[R.GUARD_ROWS + 1, 8] = 0.0
    assert g.check()["pad_elems"] == 1


def test_refusals_are_decided_on_the_host():
    """Every refusal returns CL_EINVAL before anything touches a GPU, so it can be shown here: the pointers are never read.  The probe
    reports id 0 afterwards and refuses a null pointer itself.  (That a refused call RESETS the record of an earlier launch needs a
    launch: tests/test_gpu_ew_conformance.py.)"""
    from ctrlora_amd import build, hip
    build.build(verbose=False)
    L = hip.lib()
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 15) & ~15
    q = p + 2                                                     # not 16-byte aligned
    N = None
    calls = {
        # dtype other than bf16 / fp32, in every typed launcher
        "geglu_fwd dtype": L.cl_geglu_fwd(2, p, 16, p, 8, 1, 8, N), "geglu_bwd dtype": L.cl_geglu_bwd(2, p, 16, p, 8, p, 16, 1, 8, N),
        "silu_fwd dtype": L.cl_silu_fwd(-1, p, p, 8, N), "silu_bwd dtype": L.cl_silu_bwd(7, p, p, p, 8, N),
        "axpby dtype": L.cl_axpby(2, p, 8, p, 8, 1, 8, 1.0, 0.0, N), "nchw_to_tok dtype": L.cl_nchw_to_tok(2, p, p, 8, 1, 8, 8, 1, N),
        "tok_to_nchw dtype": L.cl_tok_to_nchw(2, p, 8, p, 1, 8, 1, 1.0, 0.0, N), "colsum dtype": L.cl_colsum(2, p, 8, p, 8, 1, 1, 8, 1.0, N),
        "pool2x2 dtype": L.cl_pool2x2(2, p, 8, p, 8, 1, 1, 1, 8, 0, N), "pack2d dtype": L.cl_pack2d(2, p, 8, p, 8, 1, 8, 8, N),
        "repack dtype": L.cl_repack(2, p, p, p, 1, 1, N), "timestep dtype": L.cl_timestep_embedding(2, p, p, p, 2, 1, 1, N),
        "timestep_f dtype": L.cl_timestep_embedding_f(2, p, p, p, 2, 1, 1, N), "conv_tap dtype": L.cl_conv_tap_gather(2, p, 8, p, 8, 1, 1, 1, 1, 1, 8, 0, 1, 1, N),
        "softmax dtype": L.cl_softmax_rows(2, p, 4, p, 4, 1, 4, 1.0, N), "transpose dtype": L.cl_transpose(0, 1, p, 1, 1, p, 1, 1, 1, 1, 1, 1, N),
        "vit_patch dtype": L.cl_vit_patch_rows(2, p, p, 8, 1, 1, 2, 2, 8, N), "vit_tokens dtype": L.cl_vit_tokens(2, p, 8, p, p, p, 8, 1, 2, 8, N),
        # colsum: the two that divided by zero, and the widths
        "colsum B=0": L.cl_colsum(0, p, 8, p, 8, 0, 1, 8, 1.0, N), "colsum HW=0": L.cl_colsum(0, p, 8, p, 8, 1, 0, 8, 1.0, N),
        "colsum C<8": L.cl_colsum(0, p, 8, p, 8, 1, 1, 0, 1.0, N), "colsum ldi<C": L.cl_colsum(0, p, 8, p, 16, 1, 1, 16, 1.0, N),
        "colsum ldo<C": L.cl_colsum(0, p, 16, p, 8, 1, 1, 16, 1.0, N),
        # leading dimension smaller than the width
        "geglu_fwd ldh<2F": L.cl_geglu_fwd(0, p, 8, p, 8, 1, 8, N), "geglu_fwd ldo<F": L.cl_geglu_fwd(0, p, 32, p, 8, 1, 16, N),
        "geglu_bwd ldh<2F": L.cl_geglu_bwd(0, p, 8, p, 8, p, 16, 1, 8, N), "geglu_bwd lddo<F": L.cl_geglu_bwd(0, p, 32, p, 8, p, 32, 1, 16, N),
        "geglu_bwd lddh<2F": L.cl_geglu_bwd(0, p, 16, p, 8, p, 8, 1, 8, N),
        "axpby ldx<C": L.cl_axpby(0, p, 8, p, 16, 1, 16, 1.0, 0.0, N), "axpby ldy<C": L.cl_axpby(0, p, 16, p, 8, 1, 16, 1.0, 0.0, N),
        "pool2x2 ldi<C": L.cl_pool2x2(0, p, 8, p, 16, 1, 1, 1, 16, 0, N), "pool2x2 ldo<C": L.cl_pool2x2(0, p, 16, p, 8, 1, 1, 1, 16, 0, N),
        "conv_tap ldx<C": L.cl_conv_tap_gather(0, p, 8, p, 16, 1, 1, 1, 1, 1, 16, 0, 1, 1, N), "conv_tap ldo<C": L.cl_conv_tap_gather(0, p, 16, p, 8, 1, 1, 1, 1, 1, 16, 0, 1, 1, N),
        "pack2d ldi<C": L.cl_pack2d(0, p, 4, p, 8, 1, 8, 8, N), "softmax lds<N": L.cl_softmax_rows(0, p, 4, p, 8, 1, 8, 1.0, N),
        "softmax ldp<N": L.cl_softmax_rows(0, p, 8, p, 4, 1, 8, 1.0, N), "softmax N<4": L.cl_softmax_rows(0, p, 4, p, 4, 1, 0, 1.0, N),
        # base pointers that are not 16-byte aligned
        "geglu_fwd align h": L.cl_geglu_fwd(0, q, 16, p, 8, 1, 8, N), "geglu_fwd align out": L.cl_geglu_fwd(0, p, 16, q, 8, 1, 8, N),
        "geglu_bwd align": L.cl_geglu_bwd(0, p, 16, q, 8, p, 16, 1, 8, N), "silu_fwd align": L.cl_silu_fwd(0, q, p, 8, N),
        "silu_bwd align": L.cl_silu_bwd(0, p, p, q, 8, N), "axpby align": L.cl_axpby(0, p, 8, q, 8, 1, 8, 1.0, 0.0, N),
        "pool2x2 align": L.cl_pool2x2(0, q, 8, p, 8, 1, 1, 1, 8, 0, N), "conv_tap align": L.cl_conv_tap_gather(0, p, 8, q, 8, 1, 1, 1, 1, 1, 8, 0, 1, 1, N),
        "colsum align": L.cl_colsum(0, q, 8, p, 8, 1, 1, 8, 1.0, N), "softmax align S": L.cl_softmax_rows(0, q, 4, p, 4, 1, 4, 1.0, N),
        "softmax align P": L.cl_softmax_rows(0, p, 4, q, 4, 1, 4, 1.0, N), "vit_tokens align": L.cl_vit_tokens(0, p, 8, q, p, p, 8, 1, 2, 8, N),
        "vit_patch align": L.cl_vit_patch_rows(0, q, p, 8, 1, 1, 2, 2, 8, N),
        # the 64-tile kernels: batch outside 1 .. 65535, empty dimensions
        "transpose Bt=0": L.cl_transpose(0, 0, p, 1, 1, p, 1, 1, 0, 1, 1, 1, N), "transpose Bt=65536": L.cl_transpose(0, 0, p, 1, 1, p, 1, 1, 65536, 1, 1, 1, N),
        "transpose R=0": L.cl_transpose(0, 0, p, 1, 1, p, 1, 1, 1, 0, 1, 1, N), "transpose C=0": L.cl_transpose(0, 0, p, 1, 1, p, 1, 1, 1, 1, 0, 1, N),
        "nchw_to_tok B=0": L.cl_nchw_to_tok(0, p, p, 8, 0, 8, 8, 1, N), "nchw_to_tok B=65536": L.cl_nchw_to_tok(0, p, p, 8, 65536, 8, 8, 1, N),
        "nchw_to_tok HW=0": L.cl_nchw_to_tok(0, p, p, 8, 1, 8, 8, 0, N), "nchw_to_tok Cin=0": L.cl_nchw_to_tok(0, p, p, 8, 1, 0, 8, 1, N),
        "tok_to_nchw B=0": L.cl_tok_to_nchw(0, p, 8, p, 0, 8, 1, 1.0, 0.0, N), "tok_to_nchw B=65536": L.cl_tok_to_nchw(0, p, 8, p, 65536, 8, 1, 1.0, 0.0, N),
        "tok_to_nchw C=0": L.cl_tok_to_nchw(0, p, 8, p, 1, 0, 1, 1.0, 0.0, N), "tok_to_nchw HW=0": L.cl_tok_to_nchw(0, p, 8, p, 1, 8, 0, 1.0, 0.0, N),
        # the two embeddings agree on empty and overflowing input
        "timestep B=0": L.cl_timestep_embedding(0, p, p, p, 2, 0, 1, N), "timestep_f B=0": L.cl_timestep_embedding_f(0, p, p, p, 2, 0, 1, N),
        "timestep half=0": L.cl_timestep_embedding(0, p, p, p, 2, 1, 0, N), "timestep overflow": L.cl_timestep_embedding(0, p, p, p, 1 << 20, 1 << 16, 1 << 16, N),
        "timestep_f overflow": L.cl_timestep_embedding_f(0, p, p, p, 1 << 20, 1 << 16, 1 << 16, N),
        # conv_tap_gather
        "conv_tap stride=0": L.cl_conv_tap_gather(0, p, 8, p, 8, 1, 1, 1, 1, 1, 8, 0, 0, 1, N), "conv_tap B=0": L.cl_conv_tap_gather(0, p, 8, p, 8, 0, 1, 1, 1, 1, 8, 0, 1, 1, N),
        "conv_tap Hout=0": L.cl_conv_tap_gather(0, p, 8, p, 8, 1, 1, 1, 0, 1, 8, 0, 1, 1, N), "conv_tap C=0": L.cl_conv_tap_gather(0, p, 8, p, 8, 1, 1, 1, 1, 1, 0, 0, 1, 1, N),
        # null required pointers
        "geglu_fwd null": L.cl_geglu_fwd(0, N, 16, p, 8, 1, 8, N), "silu_fwd null": L.cl_silu_fwd(0, p, N, 8, N), "axpby null": L.cl_axpby(0, N, 8, p, 8, 1, 8, 1.0, 0.0, N),
        "transpose null": L.cl_transpose(0, 0, N, 1, 1, p, 1, 1, 1, 1, 1, 1, N), "nchw_to_tok null": L.cl_nchw_to_tok(0, p, N, 8, 1, 8, 8, 1, N),
        "tok_to_nchw null": L.cl_tok_to_nchw(0, N, 8, p, 1, 8, 1, 1.0, 0.0, N), "colsum null": L.cl_colsum(0, p, 8, N, 8, 1, 1, 8, 1.0, N),
        "pool2x2 null": L.cl_pool2x2(0, N, 8, p, 8, 1, 1, 1, 8, 0, N), "pack2d null": L.cl_pack2d(0, N, 8, p, 8, 1, 8, 8, N), "repack null": L.cl_repack(0, p, N, p, 1, 1, N),
        "timestep null": L.cl_timestep_embedding(0, N, p, p, 2, 1, 1, N), "qsample null": L.cl_qsample(p, p, N, p, p, p, 1, 1, N),
        "mse null": L.cl_mse_loss(p, p, N, N, 1, 1.0, N), "plosses null": L.cl_p_losses_mse(p, N, N, N, N, p, N, p, 1, 1, 1.0, 1.0, 0.0, N),
        "plosses lvlb without t": L.cl_p_losses_mse(p, p, N, N, p, p, N, p, 1, 1, 1.0, 1.0, 0.0, N), "zero null": L.cl_zero(N, 4, N), "tick null": L.cl_tick(N, N),
        "conv_tap null": L.cl_conv_tap_gather(0, p, 8, N, 8, 1, 1, 1, 1, 1, 8, 0, 1, 1, N), "softmax null": L.cl_softmax_rows(0, N, 4, p, 4, 1, 4, 1.0, N),
        "ddim_step null": L.cl_ddim_step(p, N, N, N, p, 0, 1.0, p, N, 1, N), "ddim_step index<0": L.cl_ddim_step(p, p, N, N, p, -1, 1.0, p, N, 1, N),
        "ddim_step_dev null": L.cl_ddim_step_dev(p, p, N, N, p, N, 1, 1.0, p, N, 1, N), "ddim_set_t null": L.cl_ddim_set_t(p, N, 1, p, 1, N),
        "adamw null": L.cl_adamw(p, p, N, p, 1, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1, 1.0, N), "adamw_dev null": L.cl_adamw_dev(p, p, p, p, 1, N, p, N),
        "dpmpp_step null": L.cl_dpmpp_step(p, p, N, p, 0, 1, 1.0, N, p, N, 1, N), "dpmpp_step_dev null": L.cl_dpmpp_step_dev(p, p, N, p, N, 1, 1.0, p, p, N, 1, N),
        "dpm_set_t null": L.cl_dpm_set_t(p, N, 1, p, 1, N), "vit_patch null": L.cl_vit_patch_rows(0, N, p, 8, 1, 1, 2, 2, 8, N),
        "vit_tokens null": L.cl_vit_tokens(0, p, 8, N, p, p, 8, 1, 2, 8, N),
        # grid limits: the batch of colsum / p_losses is grid.y, the column tiles of the 64-tile kernels are grid.y
        "colsum B=65536": L.cl_colsum(0, p, 8, p, 8, 65536, 1, 8, 1.0, N), "plosses B=65536": L.cl_p_losses_mse(p, p, N, N, N, p, N, p, 65536, 1, 1.0, 1.0, 0.0, N),
        "transpose C tiles": L.cl_transpose(0, 0, p, 1, 1, p, 1, 1, 1, 1, 65535 * 64 + 1, 1, N),
        "nchw_to_tok C tiles": L.cl_nchw_to_tok(0, p, p, 65535 * 64 + 1, 1, 1, 65535 * 64 + 1, 1, N),
        "tok_to_nchw C tiles": L.cl_tok_to_nchw(0, p, 8, p, 1, 65535 * 64 + 1, 1, 1.0, 0.0, N),
        "timestep ldo<2half": L.cl_timestep_embedding(0, p, p, p, 1, 1, 1, N), "qsample B<0": L.cl_qsample(p, p, p, p, p, p, -1, 1, N),
        "adamw n<0": L.cl_adamw(p, p, p, p, -1, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1, 1.0, N),
        # refusals the launchers already had
        "silu_fwd n%8": L.cl_silu_fwd(0, p, p, 4, N), "axpby C%8": L.cl_axpby(0, p, 8, p, 8, 1, 4, 1.0, 0.0, N), "softmax N>8192": L.cl_softmax_rows(0, p, 8196, p, 8196, 1, 8196, 1.0, N),
        "transpose Rpad<R": L.cl_transpose(0, 0, p, 1, 1, p, 8, 8, 1, 2, 1, 1, N), "pack2d Cpad<C": L.cl_pack2d(0, p, 8, p, 8, 1, 8, 4, N),
        "plosses B=0": L.cl_p_losses_mse(p, p, N, N, N, p, N, p, 0, 1, 1.0, 1.0, 0.0, N), "conv_tap tap=9": L.cl_conv_tap_gather(0, p, 8, p, 8, 1, 1, 1, 1, 1, 8, 9, 1, 1, N),
        "dpm_set_t S=0": L.cl_dpm_set_t(p, p, 0, p, 1, N),
    }
    wrong = {k: v for k, v in calls.items() if v != 1}
    assert not wrong, wrong
    out = (ctypes.c_int * 8)(*([7] * 8))
    assert L.cl_debug_ew_last_launch(out) == 0 and list(out) == [0] * 8
    assert L.cl_debug_ew_last_launch(None) == 1
    # an empty call of the flat kernels stays CL_OK (an empty tensor's data pointer is null) -- nothing is read or written
    assert L.cl_zero(N, 0, N) == 0 and L.cl_repack(0, N, N, N, 0, 0, N) == 0
