"""Kernel-level conformance of csrc/wgrad.hip (ctypes -> C ABI): every launch form cl_weight_grad_tn / cl_weight_grad_tn_group can
choose, element-wise against the fp64 contract (tests/wgrad_ref.py, whose case table names the form every row was written for).

Per row and tier (exact: small integers, bit-equal to the contract in any summation order; rounding: Gaussian inputs through the
element-wise gate |got - ref| <= u |ref| + c u mag, zero violations) the call is launched twice, and

  * the probe (cl_debug_wgrad_last_launch / _last_problem) equals the transcription of the host split rule, per call and per problem:
    kind, tiles, steps per split, splits, slab offset, first workgroup, first reduce workgroup, group launch;
  * the two launches are bit-equal;
  * canaries: dW is a column slice of a guarded fp32 buffer (guard rows above and below, pad columns -- for the row-of-three form the
    columns between 3 K and lddw) that must stay bit-identical; dy and x are slices of NaN-filled buffers (pad columns, guard rows
    above and below) and the workspace is NaN-filled before every call, so a read outside an operand or of a slab element no
    workgroup wrote reaches the result, which must stay finite; on the small side-stream workspaces the bytes past the registered
    size must stay untouched.

Workspace rows run on a side stream bound to a small workspace (cap, fall-back to direct accumulation, early flush); ring rows under
cl_debug_wgrad_ring(4 / 6), restored to 3.  cl_colsum and the fp32 family's route cl_conv_tap_gather -> cl_transpose -> cl_weight_grad
ride along with the exact tier.  The W < 8 row-of-three shapes are refusals and are never launched.
"""
import ctypes
import json
import time

import pytest
import torch

from tests import wgrad_ref as R
from tests.test_gpu_bench_shapes import _need_gpu, _record

pytestmark = pytest.mark.gpu

BF, F32 = R.BF, R.F32
DEV = "cuda"
NAN = float("nan")
NAN_BITS = 0x7FC00000
WS_FILL = 8 << 20           # bytes of the default workspace NaN-filled before a call (every row needs far less: asserted)
SIDE_BYTES = 1 << 20
_STATS = {}
_T0 = [None]
_SIDE = {}


def _probe():
    from ctrlora_amd import hip
    L = hip.lib()
    out = (ctypes.c_int * 32)()
    assert L.cl_debug_wgrad_last_launch(out) == 0
    v = list(out)
    call = dict(zip(R.CALL_FIELDS, v[:8]))
    groups = [tuple(v[8 + 3 * g:11 + 3 * g]) for g in range(min(call["groups"], R.REC_GROUPS))]
    probs = []
    one = (ctypes.c_long * 12)()
    for i in range(call["problems"]):
        assert L.cl_debug_wgrad_last_problem(i, one) == 0
        probs.append(dict(zip(R.PROB_FIELDS, list(one))))
    assert L.cl_debug_wgrad_last_problem(call["problems"], one) == 1
    return call, groups, probs


def _nanpad(t, pad):
    """t as a view into a NaN-filled buffer: `pad` NaN columns beside it, GUARD_ROWS NaN rows above and below."""
    g = R.GUARD_ROWS
    buf = torch.full((t.shape[0] + 2 * g, t.shape[1] + pad), NAN, dtype=t.dtype, device=DEV)
    buf[g:g + t.shape[0], :t.shape[1]] = t
    return buf[g:g + t.shape[0], :t.shape[1]]


def _side():
    """The suite's side stream and its 1 MiB workspace (re-registered at the size a row asks for)."""
    from ctrlora_amd import hip
    if not _SIDE:
        st = torch.cuda.Stream()
        hip.bind_stream_workspace(st, nbytes=SIDE_BYTES)
        _SIDE.update(st=st, buf=hip._stream_ws[st.cuda_stream])
    return _SIDE["st"], _SIDE["buf"]


def _gbad(g):
    c = g.check()
    return c["guard_rows"] + c["pad_elems"] + c["nan_left"]


def _launch(row, descs, bufs, dws, stream):
    from ctrlora_amd import hip
    L = hip.lib()
    zp = hip.zero_page(torch.device(DEV)).data_ptr()
    if row["single"]:
        (d,) = descs
        b, w = bufs[0], dws[0]
        return L.cl_weight_grad_tn(hip.BF16, b["dy"].data_ptr(), b["dy"].stride(0), b["x"].data_ptr(), b["x"].stride(0), w.view.data_ptr(), w.ld,
                                   d["M"], d["N"], d["K"], d["alpha"], zp, stream)
    arr = (hip.WgradDesc * len(descs))()
    for sd, d in zip(arr, descs):
        b, w = bufs[d["unit"]], dws[d["unit"]]
        full = dict(d, lddy=b["dy"].stride(0), ldx=b["x"].stride(0), lddw=w.ld)
        R.fill_desc(sd, full, b["dy"].data_ptr(), b["x"].data_ptr(), w.view[:, d["col0"]:].data_ptr())
    return L.cl_weight_grad_tn_group(hip.BF16, len(descs), ctypes.cast(arr, ctypes.c_void_p), zp, stream)


def _run_row(row):
    from ctrlora_amd import hip
    L = hip.lib()
    pl = R.row_plan(row)
    descs = R.row_descs(row)
    want_probs = [{k: p[k] for k in R.PROB_FIELDS} for p in pl["problems"]]
    cs = R.unit_c(row, pl)
    bad = []
    stats = _STATS.setdefault(row["units"][0]["kind"] if len({u["kind"] for u in row["units"]}) == 1 else "mixed",
                              dict(launches=0, violations=0, exact_mismatches=0, canary=0, form_mismatches=0, eob=0.0))
    if row["ws"] is not None:
        st, wsb = _side()
        assert L.cl_set_stream_workspace(st.cuda_stream, wsb.data_ptr(), row["ws"]) == 0
        wsf, fill = wsb.view(torch.float32), SIDE_BYTES
    else:
        st = torch.cuda.current_stream()
        hip.ensure_workspace(DEV)
        wsf, fill = hip._workspace[:WS_FILL].view(torch.float32), WS_FILL
        assert all(p["slab_off"] + p["splits"] * (3 if p["row3"] else 1) * p["N"] * p["K"] * 4 <= WS_FILL for p in pl["problems"])
    assert L.cl_debug_wgrad_ring(row["ring"]) == 0
    try:
        for tier in ("exact", "gauss"):
            ops = R.make_operands(row, tier)
            refs = R.row_ref64(row, ops)                                  # once per tier, shared by both launches
            bufs = [dict(dy=_nanpad(o["dy"].to(DEV), 16), x=_nanpad(o["x"].to(DEV), 24)) for o in ops]
            outs = []
            for rep in range(2):
                dws = [R.Guarded(u["N"], u["cols"], F32, DEV, fill=0.0, j=1 + ui % 3) for ui, u in enumerate(row["units"])]
                for w, o in zip(dws, ops):
                    w.view.copy_(o["dW0"])
                wsf.fill_(NAN)
                torch.cuda.synchronize()
                with torch.cuda.stream(st):
                    rc = _launch(row, descs, bufs, dws, st.cuda_stream)
                torch.cuda.synchronize()
                assert rc == 0, (row["name"], rc)
                outs.append((dws, _probe()))
            (dws, (call, groups, probs)), (dws2, form2) = outs
            stats["launches"] += 2
            if call != pl["call"] or groups != pl["groups"][:R.REC_GROUPS] or probs != want_probs:
                stats["form_mismatches"] += 1
                bad.append((row["name"], tier, "form", call, pl["call"], groups, pl["groups"],
                            [(a, b) for a, b in zip(probs, want_probs) if a != b][:3]))
            if form2 != (call, groups, probs) or not all(torch.equal(a.buf.view(torch.int32), b.buf.view(torch.int32)) for a, b in zip(dws, dws2)):
                bad.append((row["name"], tier, "two launches differ"))
            canary = sum(_gbad(w) for w in dws + dws2)
            if row["ws"] is not None:                                     # nothing past the registered size was written
                canary += int((wsf.view(torch.int32)[row["ws"] // 4:] != NAN_BITS).sum())
            stats["canary"] += canary
            if canary:
                bad.append((row["name"], tier, "canary", canary, [w.check() for w in dws]))
            for ui, (w, (ref, mag)) in enumerate(zip(dws, refs)):
                got = w.view.cpu()
                if tier == "exact":
                    n = int((got.double() != ref).sum())
                    stats["exact_mismatches"] += n
                    if n:
                        i = (got.double() != ref).nonzero()[0].tolist()
                        bad.append((row["name"], "exact", ui, n, i, float(got[tuple(i)]), float(ref[tuple(i)])))
                else:
                    res = R.check(got, ref, mag, cs[ui])
                    r = res["dW"]
                    print(f"{row['name']} unit {ui} c {cs[ui]:.2f} err/bound {r['err_over_bound']:.3f} need {r['need']:.3f} rel {r['rel']:.2e}")
                    stats["violations"] += r["violations"]
                    stats["eob"] = max(stats["eob"], r["err_over_bound"])
                    _record("wgrad_conformance", row=row["name"], unit=ui, eob=r["err_over_bound"], need=r["need"], rel=r["rel"])
                    if R.failures(res):
                        bad.append((row["name"], "gate", ui, R.failures(res)))
    finally:
        L.cl_debug_wgrad_ring(R.RING)
        if row["ws"] is not None:
            L.cl_set_stream_workspace(_SIDE["st"].cuda_stream, _SIDE["buf"].data_ptr(), SIDE_BYTES)
    return bad


@pytest.mark.parametrize("row", [pytest.param(r, id=r["name"]) for r in R.CASES])
def test_row_launches_the_form_it_names_and_passes_both_tiers(row):
    _need_gpu()
    if _T0[0] is None:
        _T0[0] = time.time()
    bad = _run_row(row)
    assert not bad, (len(bad), bad[:6])


def test_refusals_launch_nothing_and_touch_nothing():
    """Arguments outside the contract: CL_EINVAL, the probe at "nothing" although a launch preceded the call, dW and its guards
    bit-identical -- for the valid members of a refused mixed group too.  Every refusal is decided on the host before any launch
    (tests/test_wgrad_reference_model.py shows the same calls without a GPU): none of these calls reaches the GPU.  The buffers are
    large enough for every shape a descriptor names."""
    _need_gpu()
    from ctrlora_amd import hip
    L = hip.lib()
    hip.ensure_workspace(DEV)
    st = hip.stream()
    zp = hip.zero_page(torch.device(DEV)).data_ptr()
    dy = torch.ones(40064, 32, dtype=BF, device=DEV)
    x = torch.ones(40064, 32, dtype=BF, device=DEV)
    dW = R.Guarded(16, 216, F32, DEV, fill=1.0)
    before = dW.buf.view(torch.int32).clone()
    dy2, x2 = torch.ones(32, 8, dtype=BF, device=DEV), torch.ones(32, 8, dtype=BF, device=DEV)
    dW2 = torch.zeros(8, 8, device=DEV)
    wrong = []
    for name, ds in R.REFUSALS:
        hip.weight_grad_tn(dy2, x2, dW2)                 # a launch that succeeds in front of every refusal: the refused call resets the record
        assert _probe()[0]["ran"] == 1
        arr = (hip.WgradDesc * len(ds))()
        for sd, d in zip(arr, ds):
            R.fill_desc(sd, d, dy.data_ptr(), x.data_ptr(), dW.view.data_ptr())
        rc = L.cl_weight_grad_tn_group(hip.BF16, len(ds), ctypes.cast(arr, ctypes.c_void_p), zp, st)
        call, groups, probs = _probe()
        if rc != 1 or any(call.values()) or groups or probs:
            wrong.append((name, rc, call))
    entry = {"dtype f32": lambda: L.cl_weight_grad_tn(hip.F32, dy.data_ptr(), 32, x.data_ptr(), 32, dW.view.data_ptr(), dW.ld, 64, 16, 24, 1.0, zp, st),
             "zero page null": lambda: L.cl_weight_grad_tn(hip.BF16, dy.data_ptr(), 32, x.data_ptr(), 32, dW.view.data_ptr(), dW.ld, 64, 16, 24, 1.0, None, st),
             "single lddw < K": lambda: L.cl_weight_grad_tn(hip.BF16, dy.data_ptr(), 32, x.data_ptr(), 32, dW.view.data_ptr(), 16, 64, 16, 24, 1.0, zp, st),
             "single dy null": lambda: L.cl_weight_grad_tn(hip.BF16, None, 32, x.data_ptr(), 32, dW.view.data_ptr(), dW.ld, 64, 16, 24, 1.0, zp, st),
             "descs null": lambda: L.cl_weight_grad_tn_group(hip.BF16, 1, None, zp, st)}
    for name, call_ in entry.items():
        hip.weight_grad_tn(dy2, x2, dW2)
        rc = call_()
        if rc != 1 or any(_probe()[0].values()):
            wrong.append((name, rc))
    torch.cuda.synchronize()
    assert not wrong, wrong
    assert torch.equal(before, dW.buf.view(torch.int32))
    assert float(dW2[0, 0]) == 32.0 * (len(R.REFUSALS) + len(entry))          # the launches in between did run
    assert L.cl_debug_wgrad_last_launch(None) == 1


def _with_workspace(on):
    from ctrlora_amd import hip
    L = hip.lib()
    if on:
        if hip._workspace is None:
            hip.ensure_workspace(DEV)
        else:
            hip._chk(L.cl_set_workspace(hip._workspace.data_ptr(), hip.WORKSPACE_BYTES), "cl_set_workspace")
    else:
        hip._chk(L.cl_set_workspace(None, 0), "cl_set_workspace")


@pytest.mark.parametrize("case", [pytest.param(c, id=c["name"]) for c in R.COLSUM_CASES])
def test_colsum_is_exact_on_both_paths(case):
    """cl_colsum, both dtypes, with the workspace (block partials + finishing kernel where a sample has several chunks) and without
    (fp32 atomics): column sums of integers in [-2, 2] ONTO small integers, scale a power of two -- bit-equal to fp64 in any order.
    The input is a slice of a wider buffer (pad columns hold PAD_FILL), out a view into a guarded buffer; the workspace is NaN-filled."""
    _need_gpu()
    from ctrlora_amd import hip
    B, HW, C_, scale = case["B"], case["HW"], case["C"], case["scale"]
    assert HW * 2 * abs(scale) + 8 < 2 ** 24
    g = torch.Generator().manual_seed(9000 + R.COLSUM_CASES.index(case))
    xi = torch.randint(-2, 3, (B * HW, C_), generator=g)
    o0 = torch.randint(-8, 9, (B, C_), generator=g).float()
    ref = o0.double() + scale * xi.double().view(B, HW, C_).sum(1)
    hip.ensure_workspace(DEV)
    saved = hip._workspace
    bad = []
    stats = _STATS.setdefault("colsum", dict(launches=0, exact_mismatches=0, canary=0))
    try:
        for dt in (BF, F32):
            x = R.padded(xi.to(dt).to(DEV), 8)
            for wsp in (True, False):
                _with_workspace(wsp)
                want = R.colsum_form(B, HW, C_, hip.WORKSPACE_BYTES if wsp else 0)
                outs = []
                for rep in range(2):
                    out = R.Guarded(B, C_, F32, DEV, fill=0.0, j=2)
                    out.view.copy_(o0)
                    hip._workspace[:WS_FILL].view(torch.float32).fill_(NAN)
                    hip.colsum(x, out.view, B, HW, scale)
                    torch.cuda.synchronize()
                    outs.append(out)
                stats["launches"] += 2
                n = int((outs[0].view.cpu().double() != ref).sum())
                canary = _gbad(outs[0]) + _gbad(outs[1])
                stats["exact_mismatches"] += n
                stats["canary"] += canary
                if n or canary or not torch.equal(outs[0].buf.view(torch.int32), outs[1].buf.view(torch.int32)):
                    bad.append((case["name"], str(dt), want, n, canary))
    finally:
        torch.cuda.synchronize()
        hip._workspace = saved
        hip._chk(hip.lib().cl_set_workspace(saved.data_ptr(), hip.WORKSPACE_BYTES), "cl_set_workspace")
    assert not bad, bad


@pytest.mark.parametrize("case", [pytest.param(c, id=c["name"]) for c in R.F32_ROUTE_CASES])
def test_fp32_route_gather_transpose_weight_grad_is_exact(case):
    """The fp32 family's weight gradient of a 3x3 conv as Ctx.wgrad runs it: cl_conv_tap_gather -> cl_transpose (both operands) ->
    cl_weight_grad, all nine taps, on small integers.  The gather is exact (bit-equal to an index gather); so is the product."""
    _need_gpu()
    from ctrlora_amd import hip
    hip.ensure_workspace(DEV)
    u = case["unit"]
    row = dict(name=case["name"], units=[u])
    (o,) = R.make_operands(row, "exact")
    ((ref, _),) = R.row_ref64(row, [o])
    x, dy = o["x"].float().to(DEV), o["dy"].float().to(DEV)
    M, N, K, Mp = u["M"], u["N"], u["K"], (u["M"] + 31) // 32 * 32
    dW = R.Guarded(N, u["cols"], F32, DEV, fill=0.0, j=2)
    dW.view.copy_(o["dW0"])
    dyT = torch.full((N, Mp), NAN, device=DEV)
    hip.transpose(dy, dyT, 1, M, N, Mp)
    bad = []
    for d in R.unit_descs(u):
        xs = R.Guarded(M, K, F32, DEV, j=1)
        hip.conv_tap_gather(x, xs.view, u["B"], u["Hin"], u["Win"], u["Hout"], u["Wout"], d["tap"], u["stride"], 1)
        idx = R.gather_index(d)
        want = torch.where((idx >= 0)[:, None], o["x"].float()[idx.clamp_min(0)], torch.zeros(M, K))
        if not torch.equal(xs.view.cpu(), want) or _gbad(xs):
            bad.append(("gather", d["tap"], xs.check()))
        xT = torch.full((K, Mp), NAN, device=DEV)
        hip.transpose(xs.view, xT, 1, M, K, Mp)
        hip.weight_grad(dyT, xT, dW.view[:, d["col0"]:d["col0"] + K], u["alpha"])
    torch.cuda.synchronize()
    n = int((dW.view.cpu().double() != ref).sum())
    s = _STATS.setdefault("f32route", dict(launches=0, exact_mismatches=0, canary=0))
    s["launches"] += 28
    s["exact_mismatches"] += n
    s["canary"] += _gbad(dW)
    assert not bad and n == 0 and _gbad(dW) == 0, (bad, n, dW.check())


def test_zz_wgrad_conformance_summary():
    """Launch counts, worst err / bound per kind and the wall time of this file, for DESIGN.md."""
    _need_gpu()
    wall = None if _T0[0] is None else time.time() - _T0[0]
    print("wgrad conformance:", json.dumps(_STATS), "wall_s:", wall, "c:", R.C)
    _record("wgrad_conformance_summary", stats=_STATS, wall_s=wall, rows=len(R.CASES), c=R.C)
    for name, s in _STATS.items():
        assert s.get("violations", 0) == 0 and s["exact_mismatches"] == 0 and s["canary"] == 0 and s.get("form_mismatches", 0) == 0, (name, s)
        assert s.get("eob", 0.0) <= 1.0, (name, s)
