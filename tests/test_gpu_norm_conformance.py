"""Kernel-level conformance of csrc/norm.hip (ctypes -> C ABI): every launch form cl_groupnorm_silu_fwd / _bwd and
cl_layernorm_fwd / _bwd can choose, element-wise against the fp64 contract (tests/norm_ref.py, whose case table names the form
every row was written for).

Per row, dtype and (SiLU, eps) pair: the forward twice, then every backward (accum given / NULL x trainable / frozen) twice.
After every launch the probe cl_debug_norm_last_launch must report the form the transcription of the launchers names -- an edit
to GN1_MIN_WG or gn_two_pass_ok that moves a row onto another kernel fails here -- and every output passes

  * the element-wise gate |got - ref| <= u |ref| + fixed + c_stat stat with zero violations;
  * the project's rel-L2 gates;
  * the canary: y / dx are NaN-filled views into guarded buffers (64 guard rows, pad columns), x / dy / accum padded copies, all
    five with a leading dimension of their own; stats, dgamma / dbeta and ws (exactly cl_groupnorm_ws_floats floats, NaN-filled:
    a kernel that reads a slot no kernel of the call wrote carries the NaN to an output) sit between guard floats; afterwards no
    guard or pad changed and no NaN is left in an output;
  * y, stats and dx bit-identical between the two launches (dgamma / dbeta on the workspace + finish path of the LayerNorm).

GroupNorm rows of the one- and two-launch forms run again under cl_debug_groupnorm_form(1, 0) (three launches); every bf16 row,
GroupNorm and LayerNorm, also runs in the engine's concat layout (x, y and dx column slices, at offsets 168 / 72 / 200 so that
their base is 16-byte aligned and no more, of [rows, C + 320] buffers whose other columns hold 1e3): the forward and the frozen
backward with accum.  Measured maxima go through _record (test_zz_norm_conformance_summary).
"""
import ctypes
import json
import time

import pytest
import torch

from tests import norm_ref as R
from tests.test_gpu_bench_shapes import _need_gpu, _record

pytestmark = pytest.mark.gpu

BF, F32 = R.BF, R.F32
CANARY = -7.5e8
DEV = "cuda"
GF = 64                     # guard floats either side of stats / ws / dgamma / dbeta
X_OFF, Y_OFF, DX_OFF = 168, 72, 200   # concat layout: column offsets, multiples of 8 and odd multiples of 8 (16 bytes in bf16)
_STATS = {}
_T0 = [None]
_K4000 = {}


def _probe():
    from ctrlora_amd import hip
    out = (ctypes.c_int * 12)()
    assert hip.lib().cl_debug_norm_last_launch(out) == 0
    return dict(zip(R.PROBE_FIELDS, list(out)))


class _Vec:
    """n floats between GF canary floats either side; the live part holds `init` (NaN = must be written)."""

    def __init__(self, n, init=float("nan")):
        self.n = n
        self.buf = torch.full((n + 2 * GF,), CANARY, dtype=torch.float32, device=DEV)
        self.view = self.buf[GF:GF + n]
        if torch.is_tensor(init):
            self.view.copy_(init)
        else:
            self.view.fill_(init)

    def bad(self, nan_ok=False):
        c = int((self.buf[:GF] != CANARY).sum()) + int((self.buf[GF + self.n:] != CANARY).sum())
        return c + (0 if nan_ok else int(torch.isnan(self.view).sum()))


class _Slice:
    """An [M, C] view at column `off` of a [M + 2 guard rows, C + 320] buffer of 1e3 (the decoder's concat buffers)."""

    def __init__(self, M, C, dtype, off, src=None):
        self.buf = torch.full((M + 2 * R.GUARD_ROWS, C + 320), R.PAD_FILL, dtype=dtype, device=DEV)
        self.view = self.buf[R.GUARD_ROWS:R.GUARD_ROWS + M, off:off + C]
        if src is None:
            self.view.fill_(float("nan"))
        else:
            self.view.copy_(src)
        self.mask = torch.ones_like(self.buf, dtype=torch.bool)
        self.mask[R.GUARD_ROWS:R.GUARD_ROWS + M, off:off + C] = False

    def bad(self):
        return int((self.buf[self.mask] != R.PAD_FILL).sum()) + int(torch.isnan(self.view).sum())


def _gbad(g):
    c = g.check()
    return c["guard_rows"] + c["pad_elems"] + c["nan_left"]


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def _note(dt, res, gated, launches):
    s = _STATS.setdefault("bf16" if dt == BF else "f32", dict(launches=0, violations=0, canary=0))
    s["launches"] += launches
    if not gated:
        return
    for k, r in res.items():
        s["violations"] += r["violations"]
        s["eob_" + k] = max(s.get("eob_" + k, 0.0), r["err_over_bound"])
        if "rel_gate" in r:
            s["rel_" + k] = max(s.get("rel_" + k, 0.0), r["rel"])


def _mismatch(got, want):
    return {k: (got[k], v) for k, v in want.items() if got[k] != v}


class _Judge:
    def __init__(self, row, dt):
        self.row, self.dt, self.bad = row, dt, []

    def __call__(self, tag, case, ref, got, canary, form, want, launches=2):
        res = R.check_outputs(case, ref, got, self.dt)
        gated = self.row["gated"]
        _note(self.dt, res, gated, launches)
        _STATS["bf16" if self.dt == BF else "f32"]["canary"] += canary
        mism = _mismatch(form, want)
        f = R.failures(res) if gated else []
        eob = {k: r["err_over_bound"] for k, r in res.items()}
        if f or canary or mism:
            self.bad.append((self.row["name"], tag, dict(failures=f, canary=canary, form_mismatch=mism, eob=eob)))
        _record("norm_conformance", row=self.row["name"], dtype=str(self.dt), launch=tag, form={k: form[k] for k in ("kind", "form", "nv", "chunks")},
                eob=eob, rel={k: r["rel"] for k, r in res.items()})
        return res


_REF = {}


def _case_ref(row, dt, silu, eps):
    """(case, reference, reference without accum) of a row: computed once, shared by the plain, concat and three-launch runs."""
    key = (row["name"], dt, silu)
    if key not in _REF:
        while len(_REF) >= 2:
            _REF.pop(next(iter(_REF)))
        case = R.make_case(row, dt, silu, eps, DEV)
        ref = R.norm_ref64(case)
        _REF[key] = (case, ref, R.without_accum(ref))
    return _REF[key]


def _gn_stats(view, B, G):
    s = view.view(B, G, 2)
    return s[:, :, 0], s[:, :, 1]


def _run_gn(row, dt, forced3=False, concat=False):
    from ctrlora_amd import hip
    B, HW, C, G = (row[k] for k in ("B", "HW", "C", "G"))
    rows, nws = B * HW, hip.groupnorm_ws(B, HW, C)
    assert nws == R.gn_ws_floats(B, HW, C)
    judge = _Judge(row, dt)
    tag0 = ("forced3:" if forced3 else "") + ("concat:" if concat else "")
    for silu, eps in R.VARIANTS:
        case, ref, ref0 = _case_ref(row, dt, silu, eps)
        if concat:
            xs = _Slice(rows, C, dt, X_OFF, case["x"])
            x = xs.view
            dy, acc = R.padded(case["dy"], 16), R.padded(case["accum"], 24)
        else:
            x, dy, acc = R.padded(case["x"], 8), R.padded(case["dy"], 16), R.padded(case["accum"], 24)
        want = R.gn_form(B, HW, C, G, dt, False, forced3=forced3)
        outs = []
        for rep in range(2):
            gy = _Slice(rows, C, dt, Y_OFF) if concat else R.Guarded(rows, C, dt, DEV, j=4)
            st, ws = _Vec(B * G * 2), _Vec(nws)
            hip.groupnorm_fwd(x, gy.view, case["gamma"], case["beta"], B, HW, eps, silu, st.view, ws.view, groups=G)
            outs.append((gy, st, ws, _probe()))
        (gy, st, ws, form), (gy2, st2, _, form2) = outs
        mean, rstd = _gn_stats(st.view, B, G)
        canary = sum((o[0].bad() if concat else _gbad(o[0])) + o[1].bad() + o[2].bad(nan_ok=True) for o in outs)
        canary += xs.bad() if concat else 0
        res = judge(f"{tag0}fwd silu={int(silu)}", case, ref, dict(y=gy.view, mean=mean, rstd=rstd), canary, form, want)
        if form2 != form or not (torch.equal(_bits(gy.buf), _bits(gy2.buf)) and torch.equal(st.buf.view(torch.int32), st2.buf.view(torch.int32))):
            judge.bad.append((row["name"], tag0 + "fwd", "two launches differ"))
        if not row["gated"]:
            ref32 = torch.nn.functional.group_norm(case["x"].view(B, HW, C).permute(0, 2, 1).float(), G, case["gamma"], case["beta"], eps)
            ref32 = ref32.permute(0, 2, 1).reshape(rows, C).double()
            if silu:
                ref32 = ref32 * torch.sigmoid(ref32)
            tg = R.gate(ref32, ref["y"], ref["fixed_y"], ref["stat_y"], R.E, R.C_STAT["gn"])
            _K4000[f"{tag0}{row['name']} silu={int(silu)}"] = dict(
                kappa=float(ref["kappa"].max()), ours_eob={k: r["err_over_bound"] for k, r in res.items()},
                ours_rel_y=res["y"]["rel"], ours_maxabs_y=float((gy.view.double() - ref["y"]).abs().max()),
                torch_eob_y=tg["err_over_bound"], torch_rel_y=tg["rel"], torch_maxabs_y=float((ref32 - ref["y"]).abs().max()))
        # ---- backward: accum given / NULL x trainable / frozen (concat layout: frozen with accum only)
        modes = [(True, False)] if concat else [(a, t) for a in (True, False) for t in (False, True)]
        for with_acc, train in modes:
            want = R.gn_form(B, HW, C, G, dt, True, trainable=train, forced3=forced3)
            outs = []
            for rep in range(2):
                gdx = _Slice(rows, C, dt, DX_OFF) if concat else R.Guarded(rows, C, dt, DEV, j=5)
                ws = _Vec(nws)
                dg, db = (_Vec(C, case["dgamma0"]), _Vec(C, case["dbeta0"])) if train else (None, None)
                hip.groupnorm_bwd(x, dy, gdx.view, case["gamma"], case["beta"], st.view, B, HW, silu, ws.view,
                                  accum=acc if with_acc else None, dgamma=dg.view if train else None, dbeta=db.view if train else None, groups=G)
                outs.append((gdx, ws, dg, db, _probe()))
            (gdx, ws, dg, db, form), (gdx2, _, _, _, form2) = outs
            canary = sum((o[0].bad() if concat else _gbad(o[0])) + o[1].bad(nan_ok=True) + (o[2].bad() + o[3].bad() if train else 0) for o in outs)
            canary += st.bad() + (xs.bad() + gy.bad() if concat else _gbad(gy))
            got = dict(dx=gdx.view, dgamma=dg.view if train else None, dbeta=db.view if train else None)
            judge(f"{tag0}bwd silu={int(silu)} accum={int(with_acc)} train={int(train)}", case, ref if with_acc else ref0, got, canary, form, want)
            if form2 != form or not torch.equal(_bits(gdx.buf), _bits(gdx2.buf)):
                judge.bad.append((row["name"], tag0 + "bwd", "two launches differ"))
    torch.cuda.synchronize()
    return judge.bad


def _with_workspace(on):
    """Register (or unregister) the library's scratch; _run_ln puts back what was registered before when it is done."""
    from ctrlora_amd import hip
    L = hip.lib()
    if on:
        if hip._workspace is None:
            hip.ensure_workspace(DEV)
        else:
            hip._chk(L.cl_set_workspace(hip._workspace.data_ptr(), hip.WORKSPACE_BYTES), "cl_set_workspace")
    else:
        hip._chk(L.cl_set_workspace(None, 0), "cl_set_workspace")


def _run_ln_concat(row, case, ref, judge):
    """The bf16 LayerNorm in the concat layout: x, y and dx column slices of [M, D + 320] buffers of 1e3; the forward (with stats)
    and the frozen backward with accum, each twice, on the same form and against the same reference as the plain run."""
    from ctrlora_amd import hip
    M, D = row["M"], row["D"]
    x = _Slice(M, D, BF, X_OFF, case["x"])
    dy, acc = R.padded(case["dy"], 16), R.padded(case["accum"], 24)
    outs = []
    for rep in range(2):
        gy, st = _Slice(M, D, BF, Y_OFF), _Vec(M * 2)
        hip.layernorm_fwd(x.view, gy.view, case["gamma"], case["beta"], 1e-5, st.view)
        outs.append((gy, st, _probe()))
    (gy, st, form), (gy2, st2, form2) = outs
    canary = gy.bad() + gy2.bad() + st.bad() + st2.bad() + x.bad()
    judge("concat:fwd", case, ref, dict(y=gy.view, mean=st.view.view(M, 2)[:, 0], rstd=st.view.view(M, 2)[:, 1]), canary, form,
          R.ln_form(M, D, BF, False))
    if form2 != form or not (torch.equal(_bits(gy.buf), _bits(gy2.buf)) and torch.equal(st.buf.view(torch.int32), st2.buf.view(torch.int32))):
        judge.bad.append((row["name"], "concat:fwd", "two launches differ"))
    outs = []
    for rep in range(2):
        gdx = _Slice(M, D, BF, DX_OFF)
        hip.layernorm_bwd(x.view, dy, gdx.view, case["gamma"], st.view, accum=acc)
        outs.append((gdx, _probe()))
    (gdx, form), (gdx2, form2) = outs
    canary = gdx.bad() + gdx2.bad() + st.bad() + x.bad() + gy.bad()
    judge("concat:bwd accum=1 train=0", case, ref, dict(dx=gdx.view), canary, form, R.ln_form(M, D, BF, True))
    if form2 != form or not torch.equal(_bits(gdx.buf), _bits(gdx2.buf)):
        judge.bad.append((row["name"], "concat:bwd", "two launches differ"))


def _run_ln(row, dt, no_stats=False):
    from ctrlora_amd import hip
    M, D = row["M"], row["D"]
    judge = _Judge(row, dt)
    case = R.make_case(row, dt, False, 1e-5, DEV)
    ref = R.norm_ref64(case)
    ref0 = R.without_accum(ref)
    x, dy, acc = R.padded(case["x"], 8), R.padded(case["dy"], 16), R.padded(case["accum"], 24)
    outs = []
    for rep in range(2):
        gy, st = R.Guarded(M, D, dt, DEV, j=4), _Vec(M * 2)
        hip.layernorm_fwd(x, gy.view, case["gamma"], case["beta"], 1e-5, None if (no_stats and rep) else st.view)
        outs.append((gy, st, _probe()))
    (gy, st, form), (gy2, st2, form2) = outs
    canary = _gbad(gy) + _gbad(gy2) + st.bad() + (st2.bad(nan_ok=True) if no_stats else st2.bad())
    judge("fwd", case, ref, dict(y=gy.view, mean=st.view.view(M, 2)[:, 0], rstd=st.view.view(M, 2)[:, 1]), canary, form, R.ln_form(M, D, dt, False))
    if form2 != form or not torch.equal(_bits(gy.buf), _bits(gy2.buf)):
        judge.bad.append((row["name"], "fwd", "two launches differ"))
    if no_stats:
        if not bool(torch.isnan(st2.view).all()):
            judge.bad.append((row["name"], "fwd", "stats written although NULL was passed"))
    elif not torch.equal(st.buf.view(torch.int32), st2.buf.view(torch.int32)):
        judge.bad.append((row["name"], "fwd", "stats of two launches differ"))
    modes = [(a, t, True) for a in (True, False) for t in (False, True)] + ([(True, True, False)] if row["cap"] else [])
    saved = hip._workspace
    try:
        for with_acc, train, wsp in modes:
            _with_workspace(wsp)
            want = R.ln_form(M, D, dt, True, trainable=train, workspace=wsp, ws_bytes=hip.WORKSPACE_BYTES)
            outs = []
            for rep in range(2):
                gdx = R.Guarded(M, D, dt, DEV, j=5)
                dg, db = (_Vec(D, case["dgamma0"]), _Vec(D, case["dbeta0"])) if train else (None, None)
                hip.layernorm_bwd(x, dy, gdx.view, case["gamma"], st.view, accum=acc if with_acc else None,
                                  dgamma=dg.view if train else None, dbeta=db.view if train else None)
                outs.append((gdx, dg, db, _probe()))
            (gdx, dg, db, form), (gdx2, dg2, db2, form2) = outs
            canary = sum(_gbad(o[0]) + (o[1].bad() + o[2].bad() if train else 0) for o in outs) + st.bad()
            got = dict(dx=gdx.view, dgamma=dg.view if train else None, dbeta=db.view if train else None)
            tag = f"bwd accum={int(with_acc)} train={int(train)} ws={int(wsp)}"
            judge(tag, case, ref if with_acc else ref0, got, canary, form, want)
            if form2 != form or not torch.equal(_bits(gdx.buf), _bits(gdx2.buf)):
                judge.bad.append((row["name"], tag, "two launches differ"))
            if train and wsp and not (torch.equal(dg.view, dg2.view) and torch.equal(db.view, db2.view)):
                judge.bad.append((row["name"], tag, "dgamma / dbeta differ on the workspace + finish path"))
        if dt == BF:
            _with_workspace(True)
            _run_ln_concat(row, case, ref, judge)
    finally:
        torch.cuda.synchronize()
        hip._workspace = saved
        if saved is not None:
            hip._chk(hip.lib().cl_set_workspace(saved.data_ptr(), hip.WORKSPACE_BYTES), "cl_set_workspace")
        else:
            hip._chk(hip.lib().cl_set_workspace(None, 0), "cl_set_workspace")
    return judge.bad


_PARAMS = [pytest.param(r, dt, id=f"{r['name']}-{'bf16' if dt == BF else 'f32'}") for r in R.CASES for dt in r["dtypes"]]


@pytest.mark.parametrize("row,dtype", _PARAMS)
def test_row_launches_the_form_it_names_and_passes_the_gates(row, dtype):
    _need_gpu()
    if _T0[0] is None:
        _T0[0] = time.time()
    from ctrlora_amd import hip
    L = hip.lib()
    if row["family"] == "ln":
        bad = _run_ln(row, dtype, no_stats=(row["name"] == "ln-77x320"))
    else:
        bad = _run_gn(row, dtype)
        if dtype == BF:
            bad += _run_gn(row, dtype, concat=True)
        if any(R.gn_form(row["B"], row["HW"], row["C"], row["G"], dtype, b, t)["form"] != 3 for b, t in ((False, False), (True, False), (True, True))):
            assert L.cl_debug_groupnorm_form(1, 0) == 0
            try:
                bad += _run_gn(row, dtype, forced3=True)
            finally:
                L.cl_debug_groupnorm_form(0, 1)
    assert not bad, (len(bad), bad[:8])


def test_refusals_launch_nothing_and_touch_nothing():
    """Arguments outside the contract: CL_EINVAL, no kernel launched (the probe reports kind 0), outputs bit-identical.  Every
    refusal is decided on the host before any launch: none of these calls reaches the GPU.  C = 10240 isolates the C <= 8192
    limit: C / 8 = 4 x 320, so the rule that refuses C = 4096 (channel passes must be whole) lets it through."""
    _need_gpu()
    from ctrlora_amd import hip
    L = hip.lib()
    st = hip.stream()
    dev = DEV
    B, HW, Cmax = 2, 6, 10240      # every buffer holds the widest C a call names
    M = B * HW
    x = torch.randn(M, Cmax + 64, device=dev).bfloat16()
    dy, acc = torch.randn_like(x), torch.randn_like(x)
    y, dx = R.Guarded(M, Cmax + 64, BF, dev, j=1), R.Guarded(M, Cmax + 64, BF, dev, j=2)
    gam, bet = torch.ones(Cmax, device=dev), torch.zeros(Cmax, device=dev)
    stats, ws, dg, db = _Vec(4096), _Vec(1 << 20, 0.0), _Vec(Cmax, 1.0), _Vec(Cmax, 2.0)
    outs = [y.buf, dx.buf, stats.buf, ws.buf, dg.buf, db.buf]
    before = [_bits(t).clone() for t in outs]
    P = lambda t: None if t is None else t.data_ptr()
    ld = x.stride(0)

    def gnf(C=320, G=32, ldx=ld, ldy=y.ld):
        return L.cl_groupnorm_silu_fwd(hip.BF16, P(x), ldx, P(y.view), ldy, P(gam), P(bet), B, HW, C, G, 1e-5, 1, P(stats.view), P(ws.view), st)

    def gnb(C=320, G=32, ldx=ld, lddy=ld, ldacc=ld, lddx=dx.ld, a=acc, dg_=dg.view, db_=db.view):
        return L.cl_groupnorm_silu_bwd(hip.BF16, P(x), ldx, P(dy), lddy, P(a), ldacc, P(dx.view), lddx, P(gam), P(bet), P(stats.view), B, HW, C, G,
                                       1, P(dg_), P(db_), P(ws.view), st)

    def lnf(D=320, ldx=ld, ldy=y.ld):
        return L.cl_layernorm_fwd(hip.BF16, P(x), ldx, P(y.view), ldy, P(gam), P(bet), M, D, 1e-5, P(stats.view), st)

    def lnb(D=320, ldx=ld, lddy=ld, ldacc=ld, lddx=dx.ld, a=acc, dg_=dg.view, db_=db.view):
        return L.cl_layernorm_bwd(hip.BF16, P(x), ldx, P(dy), lddy, P(a), ldacc, P(dx.view), lddx, P(gam), P(stats.view), M, D, P(dg_), P(db_), st)

    calls = {
        "gn fwd C % 8": lambda: gnf(C=324, G=4), "gn fwd C % G": lambda: gnf(C=320, G=48), "gn fwd ldx % 8": lambda: gnf(ldx=ld + 4),
        "gn fwd ldy % 8": lambda: gnf(ldy=y.ld + 4), "gn fwd C = 4096": lambda: gnf(C=4096), "gn fwd C > 8192": lambda: gnf(C=10240),
        "gn bwd C % 8": lambda: gnb(C=324, G=4), "gn bwd C % G": lambda: gnb(C=320, G=48), "gn bwd ldx % 8": lambda: gnb(ldx=ld + 4),
        "gn bwd lddy % 8": lambda: gnb(lddy=ld + 4), "gn bwd lddx % 8": lambda: gnb(lddx=dx.ld + 4), "gn bwd ldacc % 8": lambda: gnb(ldacc=ld + 4),
        "gn bwd C = 4096": lambda: gnb(C=4096), "gn bwd C > 8192": lambda: gnb(C=10240),
        "gn bwd dgamma without dbeta": lambda: gnb(db_=None), "gn bwd dbeta without dgamma": lambda: gnb(dg_=None),
        "ln fwd D % 8": lambda: lnf(D=324), "ln fwd D = 1544": lambda: lnf(D=1544), "ln fwd ldx % 8": lambda: lnf(ldx=ld + 4),
        "ln fwd ldy % 8": lambda: lnf(ldy=y.ld + 4),
        "ln bwd D % 8": lambda: lnb(D=324), "ln bwd D = 1544": lambda: lnb(D=1544), "ln bwd ldx % 8": lambda: lnb(ldx=ld + 4),
        "ln bwd lddy % 8": lambda: lnb(lddy=ld + 4), "ln bwd lddx % 8": lambda: lnb(lddx=dx.ld + 4), "ln bwd ldacc % 8": lambda: lnb(ldacc=ld + 4),
        "ln bwd dgamma without dbeta": lambda: lnb(db_=None), "ln bwd dbeta without dgamma": lambda: lnb(dg_=None),
    }
    # a launch that succeeds in front of every refusal (into buffers of its own): the refused call itself must reset the record
    x2 = torch.randn(8, 64, device=dev).bfloat16()
    y2, g2, b2 = torch.empty_like(x2), torch.ones(64, device=dev), torch.zeros(64, device=dev)
    wrong = []
    for name, call in calls.items():
        hip.layernorm_fwd(x2, y2, g2, b2)
        assert _probe()["kind"] == R.LN_FWD
        rc = call()
        kind = _probe()["kind"]
        if rc != 1 or kind != 0:
            wrong.append((name, rc, kind))
    torch.cuda.synchronize()
    assert not wrong, wrong
    assert all(torch.equal(a, _bits(t)) for a, t in zip(before, outs))
    # a misaligned ldacc is no error when there is no accum to read
    gx = R.Guarded(M, 320, BF, dev, j=2)
    hip.layernorm_fwd(x[:, :320], y.view[:, :320], gam[:320], bet[:320], 1e-5, stats.view[:2 * M])
    assert L.cl_layernorm_bwd(hip.BF16, P(x), ld, P(dy), ld, None, ld + 4, P(gx.view), gx.ld, P(gam), P(stats.view), M, 320, None, None, st) == 0
    assert _probe()["kind"] == R.LN_BWD and _gbad(gx) == 0
    assert L.cl_debug_norm_last_launch(None) == 1


def test_zz_norm_conformance_summary():
    """Maxima per dtype, the kappa ~ 4000 figures beside torch's own fp32 group_norm, and the wall time of this file, for DESIGN.md."""
    _need_gpu()
    wall = None if _T0[0] is None else time.time() - _T0[0]
    print("norm conformance:", json.dumps(_STATS), "wall_s:", wall)
    print("kappa 4000:", json.dumps(_K4000))
    _record("norm_conformance_summary", stats=_STATS, kappa4000=_K4000, wall_s=wall, rows=len(R.CASES), c_stat=R.C_STAT)
    for name, s in _STATS.items():
        assert s["violations"] == 0 and s["canary"] == 0, (name, s)
        assert all(v <= 1.0 for k, v in s.items() if k.startswith("eob_")), (name, s)
