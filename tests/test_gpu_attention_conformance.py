"""Kernel-level conformance of the four attention files (ctypes -> C ABI): every launch form the launchers of attention_tr.hip,
attention_fwd.hip, attention_fwd40.hip and attention_bwd.hip can choose, element-wise against the fp64 contract
(tests/attn_ref.py, whose case table names the form every row was written for).

Per row: the forward twice (bit-identical), then the backward with delta fused and as a separate launch, with dK / dV and with
both NULL.  After every launch the probe cl_debug_attention_last_launch must report the form the row names -- a threshold
edit that moves a row onto another kernel fails here instead of passing on the wrong kernel -- and every output passes

  * the element-wise gate |got - ref| <= u |ref| + c_x u mag_x + score_x with zero violations, lse its absolute gate;
  * the project's rel-L2 gates;
  * the canary: outputs are NaN-filled views into guarded buffers (64 guard rows, pad columns), every operand a padded copy
    with a leading dimension of its own, lse / delta at lse_stride = rup(N, 64) + 64 with canary floats beyond rup(N, 64) and a
    canary row of floats either side; afterwards no guard changed and no NaN is left.

Every bf16 transpose-free row runs in the engine's layouts as well: Q / K / V column slices of one [rows, 3 inner] buffer and
dq / dk / dv slices of another (self-attention shapes), K / V slices of [rows, 2 inner] and dk / dv slices of one buffer.
Measured maxima go through _record (test_zz_attention_conformance_summary).
"""
import ctypes
import json
import time

import pytest
import torch

from tests import attn_ref as A
from tests.test_gpu_bench_shapes import _need_gpu, _record

pytestmark = pytest.mark.gpu

BF, F32 = A.BF, A.F32
CANARY = -7.5e8            # lse / delta floats that no launch may touch
_STATS = {}
_T0 = [None]


def _probe():
    from ctrlora_amd import hip
    out = (ctypes.c_int * 16)()
    assert hip.lib().cl_debug_attention_last_launch(out) == 0
    return dict(zip(A.PROBE_FIELDS, list(out)))


def _note(dtype, res, launches=1):
    if _T0[0] is None:
        _T0[0] = time.time()
    s = _STATS.setdefault("bf16" if dtype == BF else "f32", dict(launches=0, violations=0, canary=0))
    s["launches"] += launches
    for k, r in res.items():
        s["violations"] += r["violations"]
        s["eob_" + k] = max(s.get("eob_" + k, 0.0), r["err_over_bound"])
        if "rel" in r:
            s["rel_" + k] = max(s.get("rel_" + k, 0.0), r["rel"])
        if "max_abs" in r:
            s["lse_abs"] = max(s.get("lse_abs", 0.0), r["max_abs"])


class _RowVec:
    """lse or delta: [B, H, lse_stride] inside a float buffer with a canary row either side and canary floats beyond rup(N, 64)."""

    def __init__(self, B, H, N):
        self.N, self.live, self.stride = N, A.rup(N), A.rup(N) + 64
        self.buf = torch.full((B * H + 2, self.stride), CANARY, dtype=torch.float32, device="cuda")
        self.buf[1:-1, :self.live] = float("nan")
        self.view = self.buf[1:-1].view(B, H, self.stride)

    def check(self):
        """(canary floats that changed, NaNs left in the N live entries)."""
        changed = int((self.buf[0] != CANARY).sum()) + int((self.buf[-1] != CANARY).sum()) + int((self.buf[1:-1, self.live:] != CANARY).sum())
        return changed + int(torch.isnan(self.view[:, :, :self.N]).sum())


class _Scratch:
    """row_ws: B H lse_stride 32 bytes, 16-byte aligned, 256 guard bytes either side."""

    def __init__(self, nbytes):
        self.buf = torch.full((nbytes + 512,), 0x5A, dtype=torch.uint8, device="cuda")
        self.view = self.buf[256:256 + nbytes]

    def check(self):
        return int((self.buf[:256] != 0x5A).sum()) + int((self.buf[-256:] != 0x5A).sum())


def _guard_bad(g):
    c = g.check()
    return c["guard_rows"] + c["pad_elems"]


def _operands(case, layout):
    """(q, k, v, do) views for a layout; pads step by 8 elements in bf16 and 4 in fp32, PAD_FILL behind every row."""
    st = 8 if case["dtype"] == BF else 4
    inner = case["H"] * case["dh"]
    if layout == "qkv3":
        buf = A.padded(torch.cat([case["q"], case["k"], case["v"]], 1), st)
        q, k, v = buf[:, :inner], buf[:, inner:2 * inner], buf[:, 2 * inner:3 * inner]
    elif layout == "kv2":
        buf = A.padded(torch.cat([case["k"], case["v"]], 1), 2 * st)
        q, k, v = A.padded(case["q"], st), buf[:, :inner], buf[:, inner:2 * inner]
    else:
        q, k, v = A.padded(case["q"], st), A.padded(case["k"], 2 * st), A.padded(case["v"], 3 * st)
    return q, k, v, A.padded(case["do"], 4 * st)


def _grads(case, layout, dkv):
    """(guards, dq, dk, dv): NaN-filled views; dk = dv = None unless dkv -- but in the fused layouts their slices stay in the
    buffer, and must then still be NaN after the launch."""
    B, N, Nkv, dt = case["B"], case["N"], case["Nkv"], case["dtype"]
    inner = case["H"] * case["dh"]
    if layout == "qkv3":
        g = A.Guarded(B * N, 3 * inner, dt, "cuda", j=6)
        sl = [g.view[:, i * inner:(i + 1) * inner] for i in range(3)]
        return [g], sl[0], sl[1], sl[2]
    gq = A.Guarded(B * N, inner, dt, "cuda", j=6)
    if layout == "kv2":
        g = A.Guarded(B * Nkv, 2 * inner, dt, "cuda", j=7)
        return [gq, g], gq.view, g.view[:, :inner], g.view[:, inner:]
    if not dkv:
        return [gq], gq.view, None, None
    gk, gv = A.Guarded(B * Nkv, inner, dt, "cuda", j=7), A.Guarded(B * Nkv, inner, dt, "cuda", j=8)
    return [gq, gk, gv], gq.view, gk.view, gv.view


def _expect(row, fuse, dkv):
    e = dict(row["bwd"])
    if not dkv:
        e.update(row["bwd_nodkv"])
    if row["dtype"] == BF and row["entry"] != "t":
        e["delta_launch"] = 0 if fuse else 1
        if not fuse:
            if e["family"] == A.FAM_FOLD:                      # the fold needs the fused delta: tile-synchronous kernels instead
                e = dict(kind=2, family=A.FAM_TR, dh=row["dh"], delta_launch=1, dkv_ran=int(dkv))
            elif "bits" in e:
                e["bits_mask"] = ~A.BIT_PRIO                   # the s_setprio dQ kernel is a fused-delta form
    return e


def _form_mismatch(got, want):
    mask = want.get("bits_mask", -1)
    return {k: (got[k], v) for k, v in want.items() if k != "bits_mask" and ((got[k] & mask) != (v & mask) if k == "bits" else got[k] != v)}


def _run_row(row):
    """All launches of one row; returns the list of failures (empty = the row passes)."""
    from ctrlora_amd import hip
    L = hip.lib()
    case = A.make_case(row, "cuda")
    ref = A.attn_ref64(case)
    B, H, N, Nkv, dh, dt, sc, pre = (case[k] for k in ("B", "H", "N", "Nkv", "dh", "dtype", "scale", "prescaled"))
    inner, entry = H * dh, row["entry"]
    bad = []

    def judge(tag, got, guards, vecs, form, want):
        res = A.check_outputs(case, ref, got, dt)
        _note(dt, res)
        canary = sum(_guard_bad(g) for g in guards) + sum(v.check() for v in vecs)
        nan = sum(int(torch.isnan(t).sum()) for k, t in got.items() if t is not None and k != "lse")
        _STATS["bf16" if dt == BF else "f32"]["canary"] += canary + nan
        mism = _form_mismatch(form, want)
        f = A.failures(res)
        if f or canary or nan or mism:
            bad.append((row["name"], tag, dict(failures=f, canary=canary, nan_left=nan, form_mismatch=mism,
                                               eob={k: r["err_over_bound"] for k, r in res.items()})))
        _record("attention_conformance", row=row["name"], launch=tag, form={k: form[k] for k in ("family", "fwd_frags", "dq_frags", "dkv_frags", "bits")},
                eob={k: r["err_over_bound"] for k, r in res.items()}, rel={k: r["rel"] for k, r in res.items() if "rel" in r})

    layouts = ["padded"] if entry != "v2" else ["padded", "kv2"] + (["qkv3"] if N == Nkv else [])
    pads = (0, 64) if entry == "t" else (0,)
    assert L.cl_debug_attention_variant(row["variant"]) == 0
    try:
        for layout in layouts:
            for extra in pads:
                tag0 = layout + (f"+pad{extra}" if entry == "t" else "")
                q, k, v, do = _operands(case, layout)
                if entry == "t":
                    npad, kpad = A.rup(N) + extra, A.rup(Nkv) + extra
                    vt = hip._transposed(v, B, Nkv, inner, kpad)
                # ---- forward, twice
                outs = []
                for rep in range(2):
                    go, lse = A.Guarded(B * N, inner, dt, "cuda", j=5), _RowVec(B, H, N)
                    if entry == "v2":
                        hip.attention_fwd_v2(q, k, v, go.view, lse.view, B, H, N, Nkv, dh, sc, q_prescaled=pre)
                    elif entry == "t":
                        hip.attention_fwd(q, k, vt, go.view, lse.view, B, H, N, Nkv, dh, sc)
                    else:
                        hip.attention(q, k, v, go.view, lse.view, B, H, N, Nkv, dh, sc, q_prescaled=pre)
                    outs.append((go, lse, _probe()))
                (go, lse, form), (go2, lse2, _) = outs
                judge(tag0 + ":fwd", dict(o=go.view, lse=lse.view[:, :, :N]), [go], [lse], form, row["fwd"])
                if not (torch.equal(go.buf.view(torch.int16 if dt == BF else torch.int32), go2.buf.view(torch.int16 if dt == BF else torch.int32))
                        and torch.equal(lse.view[:, :, :N], lse2.view[:, :, :N])):
                    bad.append((row["name"], tag0 + ":fwd", "two launches differ bitwise"))
                # ---- backward
                modes = [(1, True), (1, False)] if (layout != "padded" or entry != "v2") else [(1, True), (0, True), (1, False), (0, False)]
                if entry == "t":
                    qt, dot = hip._transposed(q, B, N, inner, npad), hip._transposed(do, B, N, inner, npad)
                    kt = hip._transposed(k, B, Nkv, inner, kpad)
                for fuse, dkv in modes:
                    guards, dq, dk, dv = _grads(case, layout, dkv)
                    delta = _RowVec(B, H, N)
                    ws = _Scratch(B * H * lse.stride * 32) if row["row_ws"] else None
                    assert L.cl_debug_attention_fuse_delta(fuse) == 0
                    try:
                        a_dk, a_dv = (dk, dv) if dkv else (None, None)
                        if entry == "v2":
                            hip.attention_bwd_v2(q, k, v, go.view, do, lse.view, delta.view, dq, a_dk, a_dv, B, H, N, Nkv, dh, sc,
                                                 q_prescaled=pre, row_ws=None if ws is None else ws.view)
                        elif entry == "t":
                            hip.attention_bwd(q, k, v, go.view, do, qt, dot, kt, lse.view, delta.view, dq, a_dk, a_dv, B, H, N, Nkv, dh, sc)
                        else:
                            hip.attention_backward(q, k, v, go.view, do, lse.view, delta.view, dq, a_dk, a_dv, B, H, N, Nkv, dh, sc,
                                                   q_prescaled=pre)
                    finally:
                        L.cl_debug_attention_fuse_delta(1)
                    form = _probe()
                    got = dict(dq=dq, dk=dk if dkv else None, dv=dv if dkv else None)
                    tag = f"{tag0}:bwd fuse={fuse} dkv={int(dkv)}"
                    judge(tag, got, guards + [go], [delta, lse], form, _expect(row, fuse, dkv))
                    if ws is not None and ws.check():
                        bad.append((row["name"], tag, "row_ws guard bytes changed"))
                    if not dkv and dk is not None and not (bool(torch.isnan(dk).all()) and bool(torch.isnan(dv).all())):
                        bad.append((row["name"], tag, "dk / dv slices written although NULL was passed"))
        torch.cuda.synchronize()
    finally:
        L.cl_debug_attention_variant(0)
        L.cl_debug_attention_fuse_delta(1)
    return bad


@pytest.mark.parametrize("group", A.GROUPS)
def test_every_row_launches_the_form_it_names_and_passes_the_gates(group):
    _need_gpu()
    rows = [r for r in A.CASES if A.group_of(r) == group]
    assert rows
    bad = []
    for row in rows:
        bad += _run_row(row)
    print(f"attention conformance {group}: rows {len(rows)}", json.dumps(_STATS))
    assert not bad, (len(bad), bad[:12])


def test_refusals_launch_nothing_and_touch_nothing():
    """Arguments outside the contract: CL_EINVAL, no kernel launched (the probe reports kind 0), outputs bit-identical."""
    _need_gpu()
    from ctrlora_amd import hip
    L = hip.lib()
    row = next(r for r in A.CASES if r["name"] == "tr1-dh40-70x77-pre")
    case = A.make_case(row, "cuda")
    B, H, N, Nkv, dh, sc = (case[k] for k in ("B", "H", "N", "Nkv", "dh", "scale"))
    inner = H * dh
    q, k, v, do = _operands(case, "padded")
    go, lse, delta = A.Guarded(B * N, inner, BF, "cuda", j=5), _RowVec(B, H, N), _RowVec(B, H, N)
    hip.attention_fwd_v2(q, k, v, go.view, lse.view, B, H, N, Nkv, dh, sc, q_prescaled=True)
    guards, dq, dk, dv = _grads(case, "padded", True)
    ws = _Scratch(B * H * lse.stride * 32)
    go2, lse2 = A.Guarded(B * N, inner, BF, "cuda", j=5), _RowVec(B, H, N)          # target of the launches between the refusals
    outs = [go.buf, lse.buf, delta.buf, ws.buf] + [g.buf for g in guards]
    bits = lambda t: t.view(torch.int16) if t.dtype == BF else (t.view(torch.int32) if t.dtype == F32 else t)
    before = [bits(t).clone() for t in outs]
    st = hip.stream()
    P = lambda t: None if t is None else t.data_ptr()

    def fwd(q=q, k=k, v=v, o=go.view, ldq=None, ldk=None, ldv=None, ldo=None, dh_=dh, flags=1, dtype=hip.BF16, stride=None):
        return L.cl_attention_fwd_v2(dtype, P(q), ldq or q.stride(0), P(k), ldk or k.stride(0), P(v), ldv or v.stride(0), P(o),
                                     ldo or o.stride(0), P(lse.view), stride or lse.stride, B, H, N, Nkv, dh_, sc, flags, st)

    def bwd(ldq=None, lddo=None, lddq=None, lddk=None, stride=None, dk_=dk, dv_=dv, ws_=ws.view.data_ptr(), dh_=dh, flags=1, ldv=None):
        return L.cl_attention_bwd_v2(hip.BF16, P(q), ldq or q.stride(0), P(k), k.stride(0), P(v), ldv or v.stride(0), P(go.view), go.ld,
                                     P(do), lddo or do.stride(0), P(lse.view), P(delta.view), stride or lse.stride, P(dq),
                                     lddq or dq.stride(0), P(dk_), lddk or dk.stride(0), P(dv_), dv.stride(0), B, H, N, Nkv, dh_, sc,
                                     flags, ws_, st)

    calls = {
        "fwd ldq not 16-byte aligned": lambda: fwd(ldq=q.stride(0) + 4),
        "fwd ldk not 16-byte aligned": lambda: fwd(ldk=k.stride(0) + 2),
        "fwd ldv not 16-byte aligned": lambda: fwd(ldv=v.stride(0) + 1),
        "fwd ldo not 16-byte aligned": lambda: fwd(ldo=go.ld + 4),
        "fwd d_head 64": lambda: fwd(dh_=64),
        "fwd lse_stride % 64": lambda: fwd(stride=lse.stride - 32),
        "fwd lse_stride < N": lambda: fwd(stride=64),
        "fwd unknown flag bit": lambda: fwd(flags=3),
        "fwd fp32 on the transpose-free entry": lambda: fwd(dtype=hip.F32),
        "bwd ldq not 16-byte aligned": lambda: bwd(ldq=q.stride(0) + 4),
        "bwd ldv not 16-byte aligned": lambda: bwd(ldv=v.stride(0) + 4),
        "bwd lddo not 16-byte aligned": lambda: bwd(lddo=do.stride(0) + 4),
        "bwd lddq not 16-byte aligned": lambda: bwd(lddq=dq.stride(0) + 4),
        "bwd lddk not 16-byte aligned": lambda: bwd(lddk=dk.stride(0) + 4),
        "bwd lse_stride % 64": lambda: bwd(stride=lse.stride - 32),
        "bwd lse_stride < N": lambda: bwd(stride=64),
        "bwd dK without dV": lambda: bwd(dv_=None),
        "bwd dV without dK": lambda: bwd(dk_=None),
        "bwd misaligned row_ws": lambda: bwd(ws_=ws.view.data_ptr() + 4),
        "bwd d_head 64": lambda: bwd(dh_=64),
        "bwd unknown flag bit": lambda: bwd(flags=2),
    }
    # the transposed family refuses a pre-scaled q: it has no flags argument, so nothing can ask for it through the C ABI;
    # hip.attention / hip.attention_backward refuse it for fp32 before any call
    f32 = dict(case, dtype=F32, q=case["q"].float(), k=case["k"].float(), v=case["v"].float(), do=case["do"].float())
    o32, lse32 = A.Guarded(B * N, inner, F32, "cuda", j=5), _RowVec(B, H, N)
    b32 = bits(o32.buf).clone()
    with pytest.raises(AssertionError):
        hip.attention(f32["q"], f32["k"], f32["v"], o32.view, lse32.view, B, H, N, Nkv, dh, sc, q_prescaled=True)
    with pytest.raises(AssertionError):
        hip.attention_backward(f32["q"], f32["k"], f32["v"], o32.view, f32["do"], lse32.view, lse32.view, o32.view, None, None, B, H, N,
                               Nkv, dh, sc, q_prescaled=True)
    vt = torch.zeros(B, inner, 128, dtype=F32, device="cuda")
    calls["transposed fwd nkv_pad % 64"] = lambda: L.cl_attention_fwd(hip.F32, P(f32["q"]), inner, P(f32["k"]), inner, P(vt), 96, P(o32.view),
                                                                     o32.ld, P(lse32.view), lse32.stride, B, H, N, Nkv, dh, sc, st)
    calls["transposed fwd d_head 64"] = lambda: L.cl_attention_fwd(hip.F32, P(f32["q"]), inner, P(f32["k"]), inner, P(vt), 128, P(o32.view),
                                                                  o32.ld, P(lse32.view), lse32.stride, B, H, N, Nkv, 64, sc, st)
    calls["transposed fwd ldq not 16-byte aligned"] = lambda: L.cl_attention_fwd(hip.F32, P(f32["q"]), inner + 2, P(f32["k"]), inner, P(vt), 128,
                                                                                P(o32.view), o32.ld, P(lse32.view), lse32.stride, B, H, N, Nkv,
                                                                                dh, sc, st)
    t32 = lambda stride=None, npad=128, ldq=inner, dk_=True, dv_=True: L.cl_attention_bwd(
        hip.F32, P(f32["q"]), ldq, P(f32["k"]), inner, P(f32["v"]), inner, P(o32.view), o32.ld, P(f32["do"]), inner, P(vt), P(vt), npad,
        P(vt), 128, P(lse32.view), P(lse32.view), stride or lse32.stride, P(dq32.view), dq32.ld, P(dq32.view) if dk_ else None, dq32.ld,
        P(dq32.view) if dv_ else None, dq32.ld, B, H, N, Nkv, dh, sc, st)
    dq32 = A.Guarded(B * max(N, Nkv), inner, F32, "cuda", j=6)
    bq32 = bits(dq32.buf).clone()
    calls["transposed fwd lse_stride % 64"] = lambda: L.cl_attention_fwd(hip.F32, P(f32["q"]), inner, P(f32["k"]), inner, P(vt), 128,
                                                                        P(o32.view), o32.ld, P(lse32.view), lse32.stride - 32, B, H, N, Nkv,
                                                                        dh, sc, st)
    calls["transposed fwd lse_stride < N"] = lambda: L.cl_attention_fwd(hip.F32, P(f32["q"]), inner, P(f32["k"]), inner, P(vt), 128,
                                                                       P(o32.view), o32.ld, P(lse32.view), 64, B, H, N, Nkv, dh, sc, st)
    calls["transposed bwd lse_stride % 64"] = lambda: t32(stride=lse32.stride - 32)
    calls["transposed bwd lse_stride < N"] = lambda: t32(stride=64)
    calls["transposed bwd n_pad % 64"] = lambda: t32(npad=96)
    calls["transposed bwd ldq not 16-byte aligned"] = lambda: t32(ldq=inner + 2)
    calls["transposed bwd dK without dV"] = lambda: t32(dv_=False)
    wrong = []
    for name, call in calls.items():
        # a launch that succeeds in front of every refusal: the record must be reset by the refused call itself
        hip.attention_fwd_v2(q, k, v, go2.view, lse2.view, B, H, N, Nkv, dh, sc, q_prescaled=True)
        assert _probe()["kind"] == 1
        rc = call()
        kind = _probe()["kind"]
        if rc != 1 or kind != 0:
            wrong.append((name, rc, kind))
    torch.cuda.synchronize()
    assert not wrong, wrong
    assert all(torch.equal(a, bits(t)) for a, t in zip(before, outs)) and torch.equal(b32, bits(o32.buf)) and torch.equal(bq32, bits(dq32.buf))
    assert lse32.check() == B * H * N                     # still all NaN inside, canaries whole
    assert L.cl_debug_attention_last_launch(None) == 1


def test_zz_attention_conformance_summary():
    """Maxima per dtype and the wall time of this file, for DESIGN.md."""
    _need_gpu()
    wall = None if _T0[0] is None else time.time() - _T0[0]
    print("attention conformance:", json.dumps(_STATS), "wall_s:", wall)
    _record("attention_conformance_summary", stats=_STATS, wall_s=wall, rows=len(A.CASES), constants={str(k): v for k, v in A.C.items()},
            lse_bound={str(k): v for k, v in A.LSE_BOUND.items()})
    for name, s in _STATS.items():
        assert s["violations"] == 0 and s["canary"] == 0, (name, s)
        assert all(v <= 1.0 for k, v in s.items() if k.startswith("eob_")), (name, s)
