"""Kernel-level conformance of the two image-prompt attention kernels behind cl_attention_fwd_ip: attn_fwd_tr_ip_kernel<DH, QW>
(csrc/attention_tr.hip, bf16) and attn_fwd_ip_kernel<float, DH, 1, BKV> (csrc/attention_fwd.hip, fp32).  Every row of the case table
of tests/attn_ip_ref.py, element-wise against the fp64 contract with zero violations, plus the rel-L2 gate.

Per row: the launch in the "pad" layout (every operand a padded copy with a row pitch of its own, whole 16-byte units) and, bf16,
again in the engine's layout (k | v column slices of one [B Nkv, 2 inner] buffer, k_ip | v_ip of one [B Nip, 2 inner] buffer, at
the engine's pitch 2 inner: AttnE.project_context / project_ip).  K, V, K_ip, V_ip (fp32: K, K_ip and both V^T scratches) lie between
NaN guard rows; the fp32 V^T scratches keep the zero padding of the contract up to rup(., 64) and hold NaN in any pitch beyond it;
O is a NaN-filled view into a guarded buffer.  After the launch no guard, pad or operand changed, no NaN is left in O, the probe
cl_debug_attention_last_launch reports the form the ROW names (family, dtype, d_head, query fragments per wave, grid, fp32 key-tile
width), and a second launch into a fresh buffer gives the same bits.  fp32 rows go once more through hip.attention(..., ip=...), the
engine's path with its two cl_transpose calls, bit-identical to the direct call.  Measured maxima go through _record
(test_zz_attention_ip_conformance_summary).
"""
import ctypes
import json
import time

import pytest
import torch

from tests import attn_ip_ref as R
from tests.attn_ref import GUARD_ROWS, PAD_FILL
from tests.test_gpu_bench_shapes import _need_gpu, _record

pytestmark = pytest.mark.gpu

BF, F32 = R.BF, R.F32
_STATS = {}
_T0 = [None]


def _probe():
    from ctrlora_amd import hip
    out = (ctypes.c_int * 16)()
    assert hip.lib().cl_debug_attention_last_launch(out) == 0
    return dict(zip(R.PROBE_FIELDS, list(out)))


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def _note(dtype, res=None, launches=0, canary=0):
    if _T0[0] is None:
        _T0[0] = time.time()
    s = _STATS.setdefault("bf16" if dtype == BF else "f32", dict(launches=0, violations=0, canary=0, err_over_bound=0.0, excess=0.0, rel=0.0))
    s["launches"] += launches
    s["canary"] += canary
    if res is not None:
        s["violations"] += res["violations"]
        for k in ("err_over_bound", "excess", "rel"):
            s[k] = max(s[k], res[k])


def _rows_between_guards(parts, pad, guard=GUARD_ROWS):
    """The 2-D operands `parts` (same row count) side by side in one [rows + 2 guard, sum of widths + pad] buffer: NaN guard rows
    before the first and after the last row, PAD_FILL in the pad columns.  Returns (buffer, the views of the parts)."""
    rows, dt = parts[0].shape[0], parts[0].dtype
    width = sum(p.shape[1] for p in parts)
    buf = torch.full((rows + 2 * guard, width + pad), float("nan"), dtype=dt, device="cuda")
    buf[guard:guard + rows, width:] = PAD_FILL
    views, c0 = [], 0
    for p in parts:
        views.append(buf[guard:guard + rows, c0:c0 + p.shape[1]])
        views[-1].copy_(p)
        c0 += p.shape[1]
    return buf, views


def _vt_between_guards(v, B, n, inner, pitch):
    """fp32 V^T scratch [B, inner, pitch] of the row-major v [B n, inner]: zero up to rup(n, 64) as the contract demands, NaN in any
    pitch beyond it, NaN guard rows before the first and after the last of its B inner rows.  Returns (buffer, the 3-D view)."""
    buf = torch.full((B * inner + 2 * GUARD_ROWS, pitch), float("nan"), dtype=v.dtype, device="cuda")
    live = buf[GUARD_ROWS:GUARD_ROWS + B * inner].view(B, inner, pitch)
    live[:, :, :R.rup(n)] = 0.0
    live[:, :, :n] = v.reshape(B, n, inner).transpose(1, 2)
    return buf, live


def _operands(case, row, layout):
    """(q, k, v, k_ip, v_ip as cl_attention_fwd_ip takes them, every buffer behind them)."""
    dt = case["dtype"]
    B, H, Nkv, Nip, dh = (case[k] for k in ("B", "H", "Nkv", "Nip", "dh"))
    inner, st = H * dh, 8 if dt == BF else 4                   # pads step by 16 bytes
    d = {k: case[k].cuda() for k in ("q", "k", "v", "k_ip", "v_ip")}
    qb, (q,) = _rows_between_guards([d["q"]], st, guard=0)
    if dt == BF and layout == "engine":
        kvb, (k, v) = _rows_between_guards([d["k"], d["v"]], 0)
        ipb, (k_ip, v_ip) = _rows_between_guards([d["k_ip"], d["v_ip"]], 0)
        assert k.stride(0) == v.stride(0) == k_ip.stride(0) == v_ip.stride(0) == 2 * inner
        return q, k, v, k_ip, v_ip, [qb, kvb, ipb]
    kb, (k,) = _rows_between_guards([d["k"]], 2 * st)
    kib, (k_ip,) = _rows_between_guards([d["k_ip"]], 4 * st)
    if dt == BF:
        vb, (v,) = _rows_between_guards([d["v"]], 3 * st)
        vib, (v_ip,) = _rows_between_guards([d["v_ip"]], 5 * st)
    else:
        vb, v = _vt_between_guards(d["v"], B, Nkv, inner, row["vt_pads"][0])
        vib, v_ip = _vt_between_guards(d["v_ip"], B, Nip, inner, row["vt_pads"][1])
    return q, k, v, k_ip, v_ip, [qb, kb, vb, kib, vib]


def _want_form(row):
    dt, B, H, N = row["dtype"], row["B"], row["H"], row["N"]
    per = 64 * row["fwd_frags"]
    want = dict(kind=1, family=R.FAM_TR_IP, dtype=0 if dt == BF else 1, dh=row["dh"], fwd_frags=row["fwd_frags"],
                grid_fwd=(N + per - 1) // per * H * B)
    if dt == F32:
        want["tile"] = row["tile"]
    return want


@pytest.mark.parametrize("row", R.CASES, ids=[r["name"] for r in R.CASES])
def test_every_row_launches_the_form_it_names_and_passes_the_gates(row):
    _need_gpu()
    from ctrlora_amd import hip
    case = R.make_case(row)
    ref = R.ip_ref64(case)
    B, H, N, Nkv, Nip, dh, dt, sc, a, pre = (case[k] for k in ("B", "H", "N", "Nkv", "Nip", "dh", "dtype", "scale", "ip_scale", "prescaled"))
    inner, want = H * dh, _want_form(row)
    bad = []
    for layout in (("pad", "engine") if dt == BF else ("pad",)):
        q, k, v, k_ip, v_ip, bufs = _operands(case, row, layout)
        before = [_bits(b).clone() for b in bufs]
        outs = []
        for _ in range(2):
            og = R.Guarded(B * N, inner, dt, "cuda", j=5)
            hip.attention_fwd_ip(q, k, v, k_ip, v_ip, og.view, B, H, N, Nkv, Nip, dh, sc, a, q_prescaled=pre)
            outs.append((og, _probe()))
        torch.cuda.synchronize()
        (og, form), (og2, form2) = outs
        res = R.check(og.view.cpu(), ref, dt)
        chk = og.check()
        changed = sum(int(not torch.equal(b0, _bits(b))) for b0, b in zip(before, bufs))
        canary = chk["guard_rows"] + chk["pad_elems"] + chk["nan_left"] + changed
        _note(dt, res, launches=2, canary=canary)
        print(f"attention ip {row['name']} {layout}: err/bound {res['err_over_bound']:.3f} excess {res['excess']:.3f} rel {res['rel']:.3e}")
        _record("attention_ip_conformance", row=row["name"], layout=layout, err_over_bound=res["err_over_bound"], excess=res["excess"],
                rel=res["rel"], violations=res["violations"], form={k_: form[k_] for k_ in ("family", "fwd_frags", "grid_fwd", "tile")})
        mism = {k_: (f[k_], w) for f in (form, form2) for k_, w in want.items() if f[k_] != w}
        if chk != dict(guard_rows=0, pad_elems=0, nan_left=0) or changed:
            bad.append((layout, "canary", chk, "operand buffers changed: %d" % changed))
        if not R.passes(res):
            bad.append((layout, "gate", res))
        if mism:
            bad.append((layout, "form", mism))
        if not torch.equal(_bits(og.buf), _bits(og2.buf)):
            bad.append((layout, "two launches differ bitwise"))
        if dt == F32:
            # the engine's path: row-major v / v_ip, the two transposes made by hip.attention itself
            vb, (v_rm,) = _rows_between_guards([case["v"].cuda()], 12)
            vib, (vi_rm,) = _rows_between_guards([case["v_ip"].cuda()], 20)
            og3 = R.Guarded(B * N, inner, dt, "cuda", j=5)
            hip.attention(q, k, v_rm, og3.view, None, B, H, N, Nkv, dh, sc, ip=(k_ip, vi_rm, Nip, a))
            form3 = _probe()
            torch.cuda.synchronize()
            _note(dt, launches=1)
            if not torch.equal(_bits(og.buf), _bits(og3.buf)):
                bad.append((layout, "hip.attention(ip=...) differs bitwise from the direct call"))
            if any(form3[k_] != w for k_, w in want.items()):
                bad.append((layout, "form through hip.attention", form3))
    assert not bad, bad


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_one_text_key_and_one_image_key_is_exact_algebra(dtype):
    """Nkv = Nip = 1: both softmaxes are 1 whatever the scores, so O[b, i] = v[b, 0] + ip_scale v_ip[b, 0].  ip_scale = 1 and v, v_ip
    positive multiples of 1/4 up to 2: the product by P = 1 and the sum (<= 4, a multiple of 1/4) are exact in bf16 and fp32, so the
    output is asserted bit for bit.  (Positive: the bf16 kernel forms P = exp2(fma(s, c, -fl(s c))), which may be one fp32 ulp off 1;
    that ulp cannot move a sum that is representable in bf16 with bits to spare, but it would show in a sum that cancels to 0.)
    N = 70: a ragged last query block at every d_head."""
    _need_gpu()
    from ctrlora_amd import hip
    B, H, N = 2, 2, 70
    for i, dh in enumerate(R.ALL_DH):
        inner, sc = H * dh, dh ** -0.5
        g = torch.Generator().manual_seed(4100 + i)
        q, k, k_ip = (torch.randn(B * n, inner, generator=g).to(dtype).cuda() for n in (N, 1, 1))
        v, v_ip = ((torch.randint(1, 9, (B, inner), generator=g) / 4.0).to(dtype).cuda() for _ in range(2))
        want = (v.double() + v_ip.double()).to(dtype).repeat_interleave(N, 0)
        for pre in ((False, True) if dtype == BF else (False,)):
            og = R.Guarded(B * N, inner, dtype, "cuda", j=5)
            if dtype == BF:
                hip.attention_fwd_ip(q, k, v, k_ip, v_ip, og.view, B, H, N, 1, 1, dh, sc, 1.0, q_prescaled=pre)
            else:
                _, vt = _vt_between_guards(v, B, 1, inner, 64)
                _, vti = _vt_between_guards(v_ip, B, 1, inner, 64)
                hip.attention_fwd_ip(q, k, vt, k_ip, vti, og.view, B, H, N, 1, 1, dh, sc, 1.0)
            form = _probe()
            torch.cuda.synchronize()
            _note(dtype, launches=1)
            assert og.check() == dict(guard_rows=0, pad_elems=0, nan_left=0), (dh, pre)
            assert torch.equal(og.view, want), (dh, pre, float((og.view.double() - want.double()).abs().max()))
            assert form["family"] == R.FAM_TR_IP and form["dh"] == dh and form["grid_fwd"] == 2 * H * B


def test_refusals_return_an_error_and_write_nothing():
    """Argument checks only: every buffer is valid, allocated and zero, with room before and behind every pointer, so that a check
    that failed to refuse could still not fault.  A launch that succeeds stands in front of every refusal: the refused call itself
    must reset the record."""
    _need_gpu()
    from ctrlora_amd import hip
    L = hip.lib()
    B, H, N, Nkv, Nip, dh = 1, 2, 64, 77, 4, 40
    inner, sc, st = H * dh, dh ** -0.5, hip.stream()
    wrong = []
    for dtype in (BF, F32):
        d = hip.dt(torch.empty(0, dtype=dtype))
        x = torch.zeros(1024, 256, dtype=dtype, device="cuda")
        p = x[256:].data_ptr()                                          # 256 allocated rows before every operand, 768 behind
        og, og2 = R.Guarded(N, inner, dtype, "cuda"), R.Guarded(N, inner, dtype, "cuda")
        ldv, ldv2 = (256, 256) if dtype == BF else (128, 64)
        odd = 132 if dtype == BF else 130                               # 264 / 520 bytes: no multiple of 16

        def call(O=og, nip=Nip, dh_=dh, H_=H, flags=0, ldkip=256, ldv_=ldv, ldv2_=ldv2):
            return L.cl_attention_fwd_ip(d, p, 256, p, 256, p, ldv_, p, ldkip, p, ldv2_, O.view.data_ptr(), O.ld, B, H_, N, Nkv, nip, dh_, sc,
                                         1.0, flags, st)

        calls = {"Nip 0": lambda: call(nip=0), "Nip 65": lambda: call(nip=65), "d_head 64": lambda: call(dh_=64, H_=1),
                 "unknown flag bit": lambda: call(flags=2), "K_ip pitch not whole 16 bytes": lambda: call(ldkip=odd)}
        if dtype == F32:
            calls.update({"fp32 with the pre-scaled flag": lambda: call(flags=1), "fp32 ldv2 = 96": lambda: call(ldv2_=96),
                          "fp32 ldv2 < Nip": lambda: call(ldv2_=0), "fp32 nkv_pad < Nkv": lambda: call(ldv_=64)})
        for name, refused in calls.items():
            assert call(O=og2) == 0 and _probe()["family"] == R.FAM_TR_IP, name     # the same call with nothing wrong is taken
            rc = refused()
            kind = _probe()["kind"]
            if rc != 1 or kind != 0:
                wrong.append((str(dtype), name, rc, kind))
        torch.cuda.synchronize()
        assert og.check() == dict(guard_rows=0, pad_elems=0, nan_left=N * inner), (dtype, og.check())
        assert og2.check() == dict(guard_rows=0, pad_elems=0, nan_left=0)
        _note(dtype, launches=len(calls))
    assert not wrong, wrong
    z = torch.zeros(256, inner, dtype=BF, device="cuda")
    with pytest.raises(hip.HipError, match="code 1"):                    # and through the wrapper
        hip.attention_fwd_ip(z[:N], z[:Nkv], z[:Nkv], z[:65], z[:65], z[128:128 + N], B, H, N, Nkv, 65, dh, sc, 1.0)
    assert not bool(z.any())


def test_zz_attention_ip_conformance_summary():
    """Maxima per dtype, the launch count and the wall time of this file, for DESIGN.md."""
    _need_gpu()
    wall = None if _T0[0] is None else time.time() - _T0[0]
    print("attention ip conformance:", json.dumps(_STATS), "wall_s:", wall)
    _record("attention_ip_conformance_summary", stats=_STATS, wall_s=wall, rows=len(R.CASES), constants={str(k): v for k, v in R.C_O.items()})
    for name, s in _STATS.items():
        assert s["violations"] == 0 and s["canary"] == 0 and s["err_over_bound"] <= 1.0, (name, s)
