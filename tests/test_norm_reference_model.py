"""The fp64 contract, the rounding model, the gates and the case table of the normalisation conformance suite, on the CPU
(tests/norm_ref.py; the GPU half is tests/test_gpu_norm_conformance.py).

  * the closed-form gradients of norm_ref64 match fp64 autograd;
  * norm_model passes the element-wise gate on every gated row, and needs no more than the constants the module records;
  * the table reaches the required set of launch forms (a deleted row fails);
  * negative controls: each planted defect is flagged by the check named for it.
"""
import torch

from tests import norm_ref as R

BF, F32 = R.BF, R.F32
ROW = {r["name"]: r for r in R.CASES}


def test_closed_forms_match_fp64_autograd():
    for name, silu, eps in (("gn2-2x70x320", True, 1e-5), ("gn2-2x70x320", False, 1e-6), ("gn1-2x70x384-g48", True, 1e-5), ("ln-77x320", False, 1e-5)):
        row = ROW[name]
        case = R.make_case(row, F32, silu, eps)
        ref = R.norm_ref64(case, bounds=False)
        x = case["x"].double().requires_grad_(True)
        g, b = case["gamma"].double().requires_grad_(True), case["beta"].double().requires_grad_(True)
        if row["family"] == "ln":
            y = torch.nn.functional.layer_norm(x, (row["D"],), g, b, eps)
        else:
            B, HW, C, G = (row[k] for k in ("B", "HW", "C", "G"))
            y = torch.nn.functional.group_norm(x.view(B, HW, C).permute(0, 2, 1), G, g, b, eps).permute(0, 2, 1).reshape(B * HW, C)
            if silu:
                y = torch.nn.functional.silu(y)
        y.backward(case["dy"].double())
        rel = lambda a, c: float((a - c).norm() / c.norm())
        assert rel(ref["y"], y.detach()) < 1e-13
        assert rel(ref["dx"] - case["accum"].double(), x.grad) < 1e-12
        assert rel(ref["dx0"], x.grad) < 1e-12
        assert rel(ref["dgamma"] - case["dgamma0"].double(), g.grad) < 1e-12 and rel(ref["dbeta"] - case["dbeta0"].double(), b.grad) < 1e-12


def test_rounding_model_passes_the_gate_on_every_row_within_the_recorded_constants():
    lowest = {}
    worst = R.measure_constants(lowest=lowest)
    eob = {}
    for fam, w in worst.items():
        need = max(v for v, _ in w.values())
        print(fam, "need per output:", {k: (round(v, 3), n) for k, (v, n) in w.items()}, "recorded:", R.MEASURED[fam])
        # the range of the model's err / bound over the rows, per output, in units of the stat part: need / c_stat
        print(fam, "need / c_stat, smallest .. largest row:",
              {k: "%.3f .. %.3f" % (lowest[fam][k][0] / R.C_STAT[fam], v / R.C_STAT[fam]) for k, (v, _) in w.items()})
        # the recorded constant is what was measured (same draws on every machine; 2 % for a different libm / BLAS)
        assert need <= R.MEASURED[fam] * 1.02 and need >= R.MEASURED[fam] * 0.5, (fam, need, R.MEASURED[fam])
        eob[fam] = need / R.C_STAT[fam]
    # err / bound of the model's stat part: at most 1 / MARGIN by construction
    print("largest need / c_stat:", eob)
    assert all(v <= 1.02 / R.MARGIN for v in eob.values())


def test_degenerate_row_keeps_the_gates_that_can_hold():
    """HW C/G = 1 (var = 0, dx = 0): the model passes the element-wise gates in both dtypes and the bf16 rel-L2 gate of y, which
    stays; only fp32 y and dx (whose reference is 0) go without a rel-L2 gate."""
    row = ROW["gn2-1x1x8-g8"]
    for dt in (BF, F32):
        for silu, eps in R.VARIANTS:
            case = R.make_case(row, dt, silu, eps)
            assert case["degenerate"]
            res = R.check_outputs(case, R.norm_ref64(case), R.norm_model(case, dt), dt)
            assert not R.failures(res), (dt, silu, R.failures(res))
            assert ("rel_gate" in res["y"]) == (dt == BF) and "rel_gate" not in res["dx"] and "rel_gate" in res["dgamma"]


def test_table_reaches_the_required_launch_forms():
    got = R.covered_forms()
    required = {
        # one launch: (dtype, side, CB, LPR, NV)
        ("gn1", "bf16", "fwd", 40, 8, 1), ("gn1", "bf16", "bwd", 40, 8, 2), ("gn1", "f32", "fwd", 40, 8, 1), ("gn1", "f32", "bwd", 40, 8, 2),
        ("gn1", "bf16", "fwd", 8, 8, 1), ("gn1", "bf16", "fwd", 80, 16, 1), ("gn1", "bf16", "fwd", 120, 16, 2), ("gn1", "bf16", "bwd", 120, 16, 4),
        ("gn1", "bf16", "fwd", 40, 8, 2), ("gn1", "bf16", "fwd", 40, 8, 4), ("gn1", "bf16", "fwd", 40, 8, 8), ("gn1", "bf16", "fwd", 40, 8, 16),
        ("gn1", "f32", "fwd", 40, 8, 2), ("gn1", "f32", "fwd", 40, 8, 4), ("gn1", "f32", "fwd", 40, 8, 8),
        ("gn1", "bf16", "bwd", 40, 8, 4), ("gn1", "bf16", "bwd", 40, 8, 8), ("gn1", "bf16", "bwd", 40, 8, 16),
        ("gn1", "f32", "bwd", 40, 8, 4), ("gn1", "f32", "bwd", 40, 8, 8), ("gn1", "bf16", "fwd", 80, 16, 16),
        ("gn1", "padding_waves"), ("gn1", "threshold"), ("groups", 64), ("groups", 48), ("groups", 1), ("groups", 8), ("groups", 128),
        # two launches: (side, VX, PY, passes)
        ("gn2", "fwd", 40, 6, 1), ("gn2", "bwd", 40, 6, 1), ("gn2", "fwd", 320, 1, 1), ("gn2", "bwd", 320, 1, 1), ("gn2", "fwd", 4, 64, 1),
        ("gn2", "fwd", 16, 16, 1), ("gn2", "bwd", 16, 16, 1), ("gn2", "fwd", 160, 1, 1), ("gn2", "bwd", 160, 1, 1),
        ("gn2", "fwd", 1, 256, 1), ("gn2", "bwd", 1, 256, 1),
        ("chunks", 1), ("chunks", 2), ("chunks", 18), ("chunks", 164), ("chunks", 253),
        # three launches: trainable backward of the two-launch rows, two and three channel passes, G > 64, finalize rounds
        ("gn3", "bwd", 40, 6, 1), ("gn3", "bwd", 320, 1, 1), ("gn3", "bwd", 4, 64, 1), ("gn3", "bwd", 16, 16, 1), ("gn3", "bwd", 1, 256, 1),
        ("gn3", "fwd", 320, 1, 2), ("gn3", "bwd", 320, 1, 2), ("gn3", "fwd", 320, 1, 3), ("gn3", "bwd", 320, 1, 3), ("gn3", "fwd", 64, 4, 1),
        ("gn3", "finalize_rounds", 4),
        # conditioning rows, per form and dtype
        ("cond", 8.0, 1, "bf16"), ("cond", 8.0, 1, "f32"), ("cond", 8.0, 2, "bf16"), ("cond", 8.0, 2, "f32"), ("cond", 8.0, 3, "bf16"),
        ("cond", 8.0, 3, "f32"), ("cond", 64.0, 1, "f32"), ("cond", 64.0, 2, "f32"), ("cond", 64.0, 3, "f32"),
        # LayerNorm: (NV, RPI, ragged / whole / cap)
        ("ln", 1, 4, "ragged"), ("ln", 2, 2, "ragged"), ("ln", 3, 1, "ragged"), ("ln", 1, 4, "cap"), ("ln", 2, 2, "cap"), ("ln", 3, 1, "cap"),
    }
    assert required <= got, sorted(required - got, key=str)
    # the backward of a shape lands on another form than its forward (bf16 3 x 1030 x 1280), and fp32 leaves earlier (HW 520)
    assert R.gn_form(3, 1030, 1280, 32, BF, False)["form"] == 1 and R.gn_form(3, 1030, 1280, 32, BF, True)["form"] == 2
    assert R.gn_form(3, 520, 1280, 32, F32, False)["form"] == 1 and R.gn_form(3, 520, 1280, 32, F32, True)["form"] == 2
    assert R.gn_form(3, 520, 1280, 32, BF, True)["form"] == 1
    assert {D for D in (8, 64, 320, 512, 520, 640, 1024, 1032, 1280, 1536)} == {r["D"] for r in R.CASES if r["family"] == "ln" and not r["cap"]}
    assert all(R.gn_form(r["B"], r["HW"], r["C"], r["G"], BF, b, t, forced3=True)["form"] == 3
               for r in R.CASES if r["family"] == "gn" for b, t in ((False, False), (True, False)))


def _viol(case, ref, got, dt, key):
    return R.check_outputs(case, ref, got, dt)[key]["violations"]


def test_negative_controls_are_flagged_by_the_check_named_for_them():
    row = ROW["gn2-2x70x320"]
    B, HW, C, G = (row[k] for k in ("B", "HW", "C", "G"))
    cg = C // G
    for dt in (BF, F32):
        case = R.make_case(row, dt, True, 1e-5)
        ref = R.norm_ref64(case)
        good = R.norm_model(case, dt)
        assert not R.failures(R.check_outputs(case, ref, good, dt))

        def planted(xs, sample_shift=0, trainable_drop=False):
            """norm_model on a case whose STATISTICS come from xs (the output pass still reads the true x)."""
            alt = R.norm_model(dict(case, x=xs.to(dt)), dt)
            mean, rstd = alt["mean"].roll(sample_shift, 0), alt["rstd"].roll(sample_shift, 0)
            sc = (rstd.repeat_interleave(cg, 1) * case["gamma"])[:, None]
            z = (case["x"].float().view(B, HW, C) - mean.repeat_interleave(cg, 1)[:, None]) * sc + case["beta"]
            return dict(y=(z * torch.sigmoid(z)).to(dt).reshape(B * HW, C), mean=alt["mean"], rstd=alt["rstd"])

        x3 = case["x"].float().view(B, HW, C)
        # one pixel row left out of the statistics (its neighbour, pixel 16, counted twice in its place: n stays, the sums move)
        xs = x3.clone()
        xs[0, 17] = x3[0, 16]
        got = planted(xs.reshape(B * HW, C))
        assert _viol(case, ref, got, dt, "mean") >= G // 2 and _viol(case, ref, got, dt, "rstd") >= G // 2
        assert _viol(case, ref, got, dt, "y") > 0
        # the group boundary one channel off
        got = planted(x3.roll(-1, 2).reshape(B * HW, C))
        assert _viol(case, ref, got, dt, "mean") >= G and _viol(case, ref, got, dt, "y") > HW
        # the neighbouring sample's stats used: the stats themselves are right, the output is not
        got = planted(x3.reshape(B * HW, C), sample_shift=1)
        got["mean"], got["rstd"] = good["mean"], good["rstd"]
        assert _viol(case, ref, got, dt, "mean") == 0 and _viol(case, ref, got, dt, "y") > B * HW * C // 2
        # the last chunk's partial dropped (2 chunks of 35 pixels: the sums lose the second, n stays)
        g = R.gn_geom(B, HW, C)
        assert g["nchunk"] == 2
        xs = x3.clone()
        xs[:, g["ppc"] * (g["nchunk"] - 1):] = 0
        got = planted(xs.reshape(B * HW, C))
        assert _viol(case, ref, got, dt, "mean") == B * G and _viol(case, ref, got, dt, "rstd") == B * G
        # dgamma missing the last row
        xh = (x3.double().view(B, HW, G, cg) - ref["mean"][:, None, :, None]) * ref["rstd"][:, None, :, None]
        z = case["gamma"].double() * xh.reshape(B, HW, C) + case["beta"].double()
        s = torch.sigmoid(z)
        dz = case["dy"].double().view(B, HW, C) * s * (1 + z * (1 - s))
        short = dict(good, dgamma=(ref["dgamma"] - (dz * xh.reshape(B, HW, C))[-1, -1]).float(), dbeta=(ref["dbeta"] - dz[-1, -1]).float())
        assert _viol(case, ref, short, dt, "dgamma") > C // 2 and _viol(case, ref, short, dt, "dbeta") > C // 2
        assert _viol(case, ref, short, dt, "dx") == 0
        # a NaN left
        y = good["y"].clone()
        y[5, 7] = float("nan")
        assert _viol(case, ref, dict(good, y=y), dt, "y") == 1
    # one element 4 output ulps off (bf16: an output ulp is 2^-7 of the value)
    case = R.make_case(row, BF, True, 1e-5)
    ref, good = R.norm_ref64(case), R.norm_model(case, BF)
    y = good["y"].clone()
    i = int(y.abs().argmax())
    flat = y.view(-1).view(torch.int16)
    flat[i] += 4
    r = R.check_outputs(case, ref, dict(good, y=y), BF)["y"]
    assert r["violations"] == 1 and r["first"]["index"] == i and r["rel"] < R.REL_GATES[BF]["y"]     # the whole-tensor gate does not see it
    # a pad column or a guard row written: the canary
    for dt in (BF, F32):
        gd = R.Guarded(10, 16, dt, "cpu", j=4)
        gd.view.zero_()
        assert gd.check() == dict(guard_rows=0, pad_elems=0, nan_left=0)
        gd.buf[R.GUARD_ROWS + 3, 16] = 1.0
        assert gd.check()["pad_elems"] == 1
        gd.buf[R.GUARD_ROWS - 1, 2] = 1.0
        gd.buf[R.GUARD_ROWS + 10, 0] = 1.0
        assert gd.check()["guard_rows"] == 2
        gd.view[4, 4] = float("nan")
        assert gd.check()["nan_left"] == 1


def test_layernorm_negative_controls():
    row = ROW["ln-77x320"]
    for dt in (BF, F32):
        case = R.make_case(row, dt, False, 1e-5)
        ref, good = R.norm_ref64(case), R.norm_model(case, dt)
        assert not R.failures(R.check_outputs(case, ref, good, dt))
        # the neighbouring row's stats; dgamma missing the last row (77 = 4 x 19 + 1: the ragged row of the RPI-4 kernel)
        x, M, D = case["x"].float(), row["M"], row["D"]
        y = ((x - good["mean"].roll(1)[:, None]) * good["rstd"].roll(1)[:, None] * case["gamma"] + case["beta"]).to(dt)
        assert _viol(case, ref, dict(good, y=y), dt, "y") > M * D // 2
        xh = (x.double() - ref["mean"][:, None]) * ref["rstd"][:, None]
        short = dict(good, dgamma=(ref["dgamma"] - (case["dy"].double() * xh)[-1]).float())
        assert _viol(case, ref, short, dt, "dgamma") > D // 2


def test_refusals_are_decided_on_the_host():
    """Every refusal of the four entry points returns CL_EINVAL before anything touches a GPU, so it can be shown here: the
    pointers are never read.  cl_debug_norm_last_launch reports kind 0 afterwards -- as it does from start-up: that a refused call
    RESETS the record of an earlier launch needs a launch, and is shown in tests/test_gpu_norm_conformance.py -- and refuses a null
    pointer itself.  C = 10240 (C / 8 = 4 x 320) meets no rule but C <= 8192."""
    import ctypes
    from ctrlora_amd import build, hip
    build.build(verbose=False)
    L = hip.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)

    def probe():
        out = (ctypes.c_int * 12)(*([7] * 12))
        assert L.cl_debug_norm_last_launch(out) == 0
        return list(out)

    gnf = lambda C=320, G=32, ldx=320, ldy=320: L.cl_groupnorm_silu_fwd(hip.BF16, p, ldx, p, ldy, p, p, 2, 6, C, G, 1e-5, 1, p, p, None)
    gnb = lambda C=320, G=32, ldx=320, lddy=320, ldacc=320, lddx=320, a=p, dg=p, db=p: L.cl_groupnorm_silu_bwd(
        hip.BF16, p, ldx, p, lddy, a, ldacc, p, lddx, p, p, p, 2, 6, C, G, 1, dg, db, p, None)
    lnf = lambda D=320, ldx=320, ldy=320: L.cl_layernorm_fwd(hip.BF16, p, ldx, p, ldy, p, p, 12, D, 1e-5, p, None)
    lnb = lambda D=320, ldx=320, lddy=320, ldacc=320, lddx=320, a=p, dg=p, db=p: L.cl_layernorm_bwd(
        hip.BF16, p, ldx, p, lddy, a, ldacc, p, lddx, p, p, 12, D, dg, db, None)
    calls = [gnf(C=324, G=4), gnf(G=48), gnf(ldx=324), gnf(ldy=324), gnf(C=4096, ldx=4096, ldy=4096), gnf(C=10240, ldx=10240, ldy=10240),
             gnb(C=324, G=4), gnb(G=48), gnb(ldx=324), gnb(lddy=324), gnb(lddx=324), gnb(ldacc=324), gnb(C=4096, ldx=4096, lddy=4096, ldacc=4096, lddx=4096), gnb(C=10240, ldx=10240, lddy=10240, ldacc=10240, lddx=10240),
             gnb(db=None), gnb(dg=None), lnf(D=324), lnf(D=1544, ldx=1544, ldy=1544), lnf(ldx=324), lnf(ldy=324), lnb(D=324),
             lnb(D=1544), lnb(ldx=324), lnb(lddy=324), lnb(lddx=324), lnb(ldacc=324), lnb(db=None), lnb(dg=None)]
    assert calls == [1] * len(calls), calls
    assert probe() == [0] * 12
    assert L.cl_debug_norm_last_launch(None) == 1
