"""The one-launch GroupNorm with one workgroup per (sample, group) (csrc/norm.hip gng_*; bf16; NORM_FORM_GROUP = 5).

  * forced small shapes (cl_debug_groupnorm_group(2): whenever the slab fits): B = 2, HW = 70 / 520 (fewer / more pixels than
    threads, both ragged), every vector width (C / G = 10, 30: 4 bytes; 20, 60: 8 bytes; 40: 16 bytes; C = 2560 at G = 64), SiLU on
    and off, backward with and without accum, trainable and frozen, and one case in the engine's concat layout: the element-wise
    gate of tests/norm_ref.py with zero violations, guards and pads untouched, ws NaN-filled before and after, y / stats / dx
    bit-identical across two launches, the probe against a transcription of gng_geom;
  * the rule: what the production shapes report under mode 1, and that cl_debug_groupnorm_form(1, 0) / (0, 0), mode 0 and fp32
    never reach the form;
  * [8, 320, 4096] and [8, 1920, 1024] forward and backward against torch in fp64 with the gates of
    test_groupnorm_one_launch_production_shapes;
  * on the CPU: the listing of norm.hip holds no scratch and no spill for any gng_* kernel, and each fits 4 waves per SIMD, the
    budget the 1024-thread workgroups assume.
"""
import os
import shutil
import sys

import pytest
import torch

from tests import norm_ref as R
from tests.norm_ref import Guarded, check_outputs, make_case, padded
from tests.util import ROOT, rel_l2

BF, F32 = R.BF, R.F32
DEV = "cuda"
FORM_GROUP = 5
NV_TABLE = (6, 16, 22, 64)
FWD_DW = BWD_DW = 64                      # GNG_FWD_DW / GNG_BWD_DW: dwords of slab per lane
BWD_NV = 16                                # GNG_BWD_NV: the backward's largest NV
MAX_WAVES, MAX_CG, MIN_HW, MIN_WG = 16, 128, 256, 192
PRODUCTION = [(4096, 320), (4096, 640), (4096, 960), (1024, 320), (1024, 640), (1024, 960), (1024, 1280), (1024, 1920),
              (256, 640), (256, 1280), (256, 1920), (256, 2560)]


def gng_geom(B, HW, C, G, bwd, mode):
    """Transcription of gng_geom (csrc/norm.hip) for bf16 with the launch-form switches at their defaults: None = not taken."""
    if mode == 0 or C % G:
        return None
    cg = C // G
    if cg % 2 or cg > MAX_CG:
        return None
    if mode == 1 and not gng_rule(B, HW, C, G, bwd):
        return None
    vw = 4 if cg % 8 == 0 else 2 if cg % 4 == 0 else 1
    vpr = cg // (2 * vw)
    nw = MAX_WAVES
    while nw and (64 * nw) % vpr:
        nw -= 1
    if not nw:
        return None
    nv = (HW * vpr + 64 * nw - 1) // (64 * nw)
    NV = next((t for t in NV_TABLE if nv <= t), None)
    if NV is None or NV * vw * (2 if bwd else 1) > (BWD_DW if bwd else FWD_DW) or (bwd and NV > BWD_NV):
        return None
    return dict(VW=vw, VPR=vpr, NW=nw, NV=NV, cg=cg)


def gng_rule(B, HW, C, G, bwd):
    return HW >= MIN_HW and B * G >= MIN_WG


def gng_probe(B, G, geom, bwd):
    return dict(kind=R.GN_BWD if bwd else R.GN_FWD, form=FORM_GROUP, dtype=0, nv=geom["NV"], lpr_rpi=geom["VPR"], threads=64 * geom["NW"],
                cb_vx=geom["cg"], chunks=0, grid_x=B * G, grid_y=1, colsum=0, passes=1)


def _helpers():
    from tests import test_gpu_norm_conformance as T
    return T


def _row(i, B, HW, C, G):
    # make_case seeds its generator from the row's place in norm_ref's table: borrow the name (hence the seed) of row i
    return dict(name=R.CASES[i]["name"], family="gn", B=B, HW=HW, C=C, G=G, cond=None, gated=True)


def _mode(m):
    from ctrlora_amd import hip
    assert hip.lib().cl_debug_groupnorm_group(m) == 0


_SMALL = [(C, 32) for C in (320, 640, 960, 1280, 1920)] + [(2560, 64)]


def _run_forced(row, silu, concat=False):
    """Forward twice, then every backward twice, under mode 2; returns the list of complaints."""
    from ctrlora_amd import hip
    T = _helpers()
    B, HW, C, G = (row[k] for k in ("B", "HW", "C", "G"))
    rows, nws, eps = B * HW, hip.groupnorm_ws(B, HW, C), (1e-5 if silu else 1e-6)
    assert nws == R.gn_ws_floats(B, HW, C)
    case = make_case(row, BF, silu, eps, DEV)
    ref = R.norm_ref64(case)
    ref0 = R.without_accum(ref)
    bad = []
    if concat:
        xs = T._Slice(rows, C, BF, T.X_OFF, case["x"])
        x = xs.view
    else:
        x = padded(case["x"], 8)
    dy, acc = padded(case["dy"], 16), padded(case["accum"], 24)

    def judge(tag, got, reference, canary, form, bwd):
        want = gng_probe(B, G, gng_geom(B, HW, C, G, bwd, 2), bwd)
        res = check_outputs(case, reference, got, BF)
        f = R.failures(res)
        mism = {k: (form[k], v) for k, v in want.items() if form[k] != v}
        if f or canary or mism:
            bad.append((tag, dict(failures=f, canary=canary, form_mismatch=mism)))

    outs = []
    for rep in range(2):
        gy = T._Slice(rows, C, BF, T.Y_OFF) if concat else Guarded(rows, C, BF, DEV, j=4)
        st, ws = T._Vec(B * G * 2), T._Vec(nws)
        hip.groupnorm_fwd(x, gy.view, case["gamma"], case["beta"], B, HW, eps, silu, st.view, ws.view, groups=G)
        outs.append((gy, st, ws, T._probe()))
    (gy, st, ws, form), (gy2, st2, ws2, form2) = outs
    gbad = (lambda o: o.bad()) if concat else T._gbad
    canary = sum(gbad(o[0]) + o[1].bad() + o[2].bad(nan_ok=True) for o in outs) + (xs.bad() if concat else 0)
    canary += int((~torch.isnan(ws.view)).sum()) + int((~torch.isnan(ws2.view)).sum())          # the form never touches ws
    mean, rstd = st.view.view(B, G, 2)[:, :, 0], st.view.view(B, G, 2)[:, :, 1]
    judge(f"fwd silu={int(silu)}", dict(y=gy.view, mean=mean, rstd=rstd), ref, canary, form, False)
    if form2 != form or not (torch.equal(T._bits(gy.buf), T._bits(gy2.buf)) and torch.equal(st.buf.view(torch.int32), st2.buf.view(torch.int32))):
        bad.append(("fwd", "two launches differ"))
    modes = [(True, False)] if concat else [(a, t) for a in (True, False) for t in (False, True)]
    for with_acc, train in modes:
        outs = []
        for rep in range(2):
            gdx = T._Slice(rows, C, BF, T.DX_OFF) if concat else Guarded(rows, C, BF, DEV, j=5)
            ws = T._Vec(nws)
            dg, db = (T._Vec(C, case["dgamma0"]), T._Vec(C, case["dbeta0"])) if train else (None, None)
            hip.groupnorm_bwd(x, dy, gdx.view, case["gamma"], case["beta"], st.view, B, HW, silu, ws.view, accum=acc if with_acc else None,
                              dgamma=dg.view if train else None, dbeta=db.view if train else None, groups=G)
            outs.append((gdx, ws, dg, db, T._probe()))
        (gdx, ws, dg, db, form), (gdx2, _, _, _, form2) = outs
        canary = sum(gbad(o[0]) + o[1].bad(nan_ok=True) + int((~torch.isnan(o[1].view)).sum()) + (o[2].bad() + o[3].bad() if train else 0)
                     for o in outs)
        canary += st.bad() + gbad(gy) + (xs.bad() if concat else 0)
        got = dict(dx=gdx.view, dgamma=dg.view if train else None, dbeta=db.view if train else None)
        tag = f"bwd silu={int(silu)} accum={int(with_acc)} train={int(train)}"
        judge(tag, got, ref if with_acc else ref0, canary, form, True)
        if form2 != form or not torch.equal(T._bits(gdx.buf), T._bits(gdx2.buf)):
            bad.append((tag, "two launches differ"))
    torch.cuda.synchronize()
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("silu", [True, False], ids=["silu", "plain"])
@pytest.mark.parametrize("HW", [70, 520])
@pytest.mark.parametrize("C,G", _SMALL, ids=[f"c{c}g{g}" for c, g in _SMALL])
def test_forced_small_shapes_pass_the_elementwise_gate(C, G, HW, silu):
    T = _helpers()
    T._need_gpu()
    i = _SMALL.index((C, G)) * 2 + (HW == 520)
    assert gng_geom(2, HW, C, G, False, 2) and gng_geom(2, HW, C, G, True, 2)          # the slab fits: the case reaches the form
    _mode(2)
    try:
        bad = _run_forced(_row(i, 2, HW, C, G), silu)
    finally:
        _mode(1)
    assert not bad, (len(bad), bad[:6])


@pytest.mark.gpu
def test_forced_concat_layout_four_byte_vectors():
    """x, y and dx as column slices at offsets 168 / 72 / 200 of wider buffers of 1e3: segment bases aligned to 4 bytes and no more."""
    T = _helpers()
    T._need_gpu()
    _mode(2)
    try:
        bad = _run_forced(_row(12, 2, 520, 320, 32), True, concat=True)
    finally:
        _mode(1)
    assert not bad, (len(bad), bad[:6])


def _launch_pair(B, HW, C, G, dtype, bufs=None):
    """One forward and one frozen backward with accum on plain buffers; returns (probe fwd, probe bwd, y, dx, stats)."""
    from ctrlora_amd import hip
    T = _helpers()
    if bufs is None:
        g = torch.Generator().manual_seed(C + HW)
        mk = lambda: (torch.randn(B * HW, C, generator=g) * 1.5 + 0.3).to(dtype).to(DEV)
        bufs = dict(x=mk(), dy=mk(), acc=mk(), gamma=(1 + 0.2 * torch.randn(C, generator=g)).to(DEV), beta=(0.2 * torch.randn(C, generator=g)).to(DEV))
    y, dx = torch.empty_like(bufs["x"]), torch.empty_like(bufs["x"])
    stats, ws = torch.empty(B, G, 2, device=DEV), torch.zeros(hip.groupnorm_ws(B, HW, C), device=DEV)
    hip.groupnorm_fwd(bufs["x"], y, bufs["gamma"], bufs["beta"], B, HW, 1e-5, True, stats, ws, groups=G)
    pf = T._probe()
    hip.groupnorm_bwd(bufs["x"], bufs["dy"], dx, bufs["gamma"], bufs["beta"], stats, B, HW, True, ws, accum=bufs["acc"], groups=G)
    pb = T._probe()
    return pf, pb, y, dx, stats, bufs


@pytest.mark.gpu
def test_rule_takes_the_recorded_classes_and_the_switches_turn_it_off():
    from ctrlora_amd import hip
    T = _helpers()
    T._need_gpu()
    L = hip.lib()
    B, G = 8, 32
    wrong = []
    for HW, C in PRODUCTION:
        pf, pb, *_ = _launch_pair(B, HW, C, G, BF)
        for bwd, p in ((False, pf), (True, pb)):
            geom = gng_geom(B, HW, C, G, bwd, 1)
            if geom:
                want = gng_probe(B, G, geom, bwd)
                if any(p[k] != v for k, v in want.items()):
                    wrong.append((HW, C, bwd, p, want))
            elif p["form"] not in (1, 2, 3) or p != R.gn_form(B, HW, C, G, BF, bwd):
                wrong.append((HW, C, bwd, p, "old form expected"))
    assert not wrong, wrong
    # the classes the record names: every forward, and every backward but the three at 64x64 -- C = 640 / 960 exceed
    # the register budget, C = 320 measured slower from HBM -- which report the two-launch form also when forced
    taken = {(HW, C, bwd) for HW, C in PRODUCTION for bwd in (False, True) if gng_geom(B, HW, C, G, bwd, 1)}
    assert {(HW, C, bwd) for HW, C in PRODUCTION for bwd in (False, True)} - taken == {(4096, C, True) for C in (320, 640, 960)}
    assert all(gng_geom(B, 4096, C, G, True, 2) is None for C in (320, 640, 960))
    assert gng_geom(B, 64, 1280, G, False, 1) is None and gng_geom(4, 1024, 640, G, False, 1) is None    # < 256 pixels; < 192 workgroups
    # switches: three launches / one-launch forms off / mode 0 report an old form at a shape the rule takes; mode 2 as well under them
    HW, C = 1024, 640
    assert gng_geom(B, HW, C, G, False, 1) and gng_geom(B, HW, C, G, True, 1)
    seen = []
    try:
        for three, one, mode in ((1, 0, 1), (0, 0, 1), (1, 0, 2), (0, 0, 2), (0, 1, 0)):
            assert L.cl_debug_groupnorm_form(three, one) == 0 and L.cl_debug_groupnorm_group(mode) == 0
            pf, pb, *_ = _launch_pair(B, HW, C, G, BF)
            seen.append((three, one, mode, pf["form"], pb["form"]))
    finally:
        L.cl_debug_groupnorm_form(0, 1)
        L.cl_debug_groupnorm_group(1)
    assert all(f in (1, 2, 3) and b in (1, 2, 3) for _, _, _, f, b in seen), seen
    assert [s[3] for s in seen[:2]] == [3, 2], seen                                   # (1, 0): three launches; (0, 0): two
    # fp32 never takes it, by rule or forced
    try:
        for mode, (b_, hw_, c_) in ((1, (8, 1024, 320)), (2, (2, 520, 320))):
            _mode(mode)
            pf, pb, *_ = _launch_pair(b_, hw_, c_, G, F32)
            assert pf["form"] in (1, 2, 3) and pb["form"] in (1, 2, 3), (mode, pf, pb)
    finally:
        _mode(1)
    assert L.cl_debug_groupnorm_group(3) == 1 and L.cl_debug_groupnorm_group(-1) == 1  # unknown codes are refused
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("HW,C", [(4096, 320), (1024, 1920)])
def test_production_shapes_against_fp64(HW, C):
    """[8, 320, 4096] (the forward's 22 four-byte vectors per lane; its backward is a class the record leaves on the two-launch
    form, and is gated here all the same) and [8, 1920, 1024] (the backward's largest slab) with SiLU and accum vs torch in fp64:
    rel-L2 6e-3 forward, 1.2e-2 backward; statistics within 1e-5 of the older form's."""
    T = _helpers()
    T._need_gpu()
    B, G = 8, 32
    out, bufs = {}, None
    try:
        for mode in (2, 0):
            _mode(mode)
            pf, pb, y, dx, stats, bufs = _launch_pair(B, HW, C, G, BF, bufs)
            torch.cuda.synchronize()
            out[mode] = (pf, pb, y, dx, stats)
    finally:
        _mode(1)
    pf, pb, y, dx, stats = out[2]
    assert pf["form"] == FORM_GROUP and (pb["form"] == FORM_GROUP) == bool(gng_geom(B, HW, C, G, True, 2)) == (HW == 1024)
    assert out[0][0]["form"] in (1, 2) and out[0][1]["form"] in (1, 2)
    xr = bufs["x"].double().reshape(B, HW, C).permute(0, 2, 1).requires_grad_(True)
    yr = torch.nn.functional.silu(torch.nn.functional.group_norm(xr, G, bufs["gamma"].double(), bufs["beta"].double(), 1e-5))
    yr.backward(bufs["dy"].double().reshape(B, HW, C).permute(0, 2, 1))
    y_ref = yr.detach().permute(0, 2, 1).reshape(B * HW, C)
    dx_ref = xr.grad.permute(0, 2, 1).reshape(B * HW, C) + bufs["acc"].double()
    e_y, e_dx, e_st = rel_l2(y, y_ref), rel_l2(dx, dx_ref), rel_l2(stats, out[0][4])
    print(f"gng [8, {C}, {HW}]: rel-L2 y", e_y, "dx", e_dx, "stats vs two-launch", e_st)
    assert e_y < 6e-3 and e_dx < 1.2e-2 and e_st < 1e-5, (e_y, e_dx, e_st)
    assert rel_l2(y, out[0][2]) < 6e-3 and rel_l2(dx, out[0][3]) < 1.2e-2


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_group_kernels_hold_no_scratch_and_fit_four_waves_per_simd(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    rows = [k for k in kr.collect(sources=["norm.hip"], outdir=str(tmp_path)) if k["name"].startswith("gng_")]
    names = {k["name"] for k in rows}
    fwd = [(1, 6), (1, 16), (1, 22), (1, 64), (2, 6), (2, 16), (2, 22), (4, 6), (4, 16)]
    bwd = [(1, 6), (1, 16), (2, 6), (2, 16), (4, 6)]
    want = {f"gng_{d}_kernel<{s}, {vw}, {nv}>" for d, forms in (("fwd", fwd), ("bwd", bwd)) for vw, nv in forms for s in ("true", "false")}
    assert names == want, (sorted(names - want), sorted(want - names))
    # every instantiated pair is within the budget, and the transcription reaches no pair that is not instantiated
    assert all(vw * nv <= FWD_DW for vw, nv in fwd) and all(2 * vw * nv <= BWD_DW and nv <= BWD_NV for vw, nv in bwd)
    bad = [(k["name"], k["arch_vgpr"], k["waves_simd"], k.get("private_segment_fixed_size"), k.get("vgpr_spill_count"), k.get("sgpr_spill_count"))
           for k in rows if k["flag"] or k["waves_simd"] < 4 or k.get("agpr_count", 0)]
    assert not bad, bad
