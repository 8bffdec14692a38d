"""Every engine block (ctrlora_amd/engine/blocks.py: ResBlockE, SpatialTransformerE and the launches they compose), forward
and backward, against the fp64 reference of tests/block_ref.py -- one test per (case, dtype, variant) of block_ref.RUNS.

Numeric gates, on every output of the run (block output, dx, dsemb / the de_slot slice, every trainable gradient under its
state-dict name through Trainable.param_view):
  bf16   rel-L2(engine, fp64) <= 2 x rel-L2(comparator, fp64), the comparator (block_ref.Mode(round=True): bf16 rounding at
         the engine's stored tensors of that run's mode) evaluated in the same test on the same inputs.  2: the floor is
         reproducible to 1.3x across seeds and a 2 % defect reaches 3.3x or more (tests/test_block_reference_model.py).
         An output the storage model leaves exact (comparator error 0: the last layer's bias gradient, a column sum of the
         bf16 upstream gradient) is an fp32 accumulation and takes the fp32 family's gradient gate.
  fp32   the parity-mode gates of test_gpu_parity.py: 1e-4 on activations, 5e-4 on gradients.

Exact checks: output and dx are written through out= into gemm_ref.Guarded buffers (no NaN left, no guard touched); the inputs
and every saved tensor are bit-identical after backward; flat_grad is exactly 0 outside the expected slices (alignment padding
included) and non-zero inside each; a second backward without zero_grad gives twice the first (rel-L2 1e-5).
"""
import time

import pytest
import torch

from tests import block_ref as BR
from tests.gemm_ref import Guarded
from tests.test_gpu_bench_shapes import _need_gpu, _record

pytestmark = pytest.mark.gpu

SEED = 1
GATE = 2.0
F32_ACT, F32_GRAD = 1e-4, 5e-4
_RESULTS = {}
_T0 = [None]


def _tensors(o):
    if torch.is_tensor(o):
        return [o]
    if isinstance(o, (tuple, list)):
        return [t for e in o for t in _tensors(e)]
    return []


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("run", BR.RUNS, ids=lambda r: r.id)
def test_block(run, monkeypatch):
    _need_gpu()
    from ctrlora_amd import hip
    from ctrlora_amd.engine import blocks
    if _T0[0] is None:
        _T0[0] = time.time()
    case = BR.CASES[run.case]
    bf = run.dtype == "bf16"
    dtype = torch.bfloat16 if bf else torch.float32
    dev = torch.device("cuda")
    if run.variant == "ln-off":
        monkeypatch.setattr(hip, "LN_PROLOGUE", False)
    ips = 0.6 if run.ip else None
    e_pre = run.case == "rb-frozen"
    sd, inp = BR.make_sd(case, SEED, ips), BR.make_inputs(case, SEED)
    ref = BR.reference(run.case, SEED, e_pre, ips, run.backward)
    B, H, W, M = case.B, case.H, case.W, case.M

    blk, _, sets = BR.build_block(case, sd, dtype, need_bwd=case.train != "infer")
    ctx = blocks.Ctx(dtype, dev, run.record)
    actual, want = BR.predicates(run, blk, ctx), dict(run.expect)
    asserted = {k: v for k, v in want.items() if k in actual}
    assert {k: actual[k] for k in asserted} == asserted, (actual, want)
    names = BR.gated(run, sd)
    params = [n for n in names if n in sd]
    assert {t.name for ts in sets for t in ts.items} == set(BR.trainable_names(case, sd))

    cu = lambda t: t.to(dtype).to(dev).contiguous()
    x, dout = cu(BR.tok(inp["x"])), cu(BR.tok(inp["dout"]))
    out_g, dx_g = Guarded(M, case.cout, dtype, dev), Guarded(M, case.cin, dtype, dev)
    ins = dict(x=x, dout=dout)
    deslot = run.variant == "deslot"
    if case.kind == "res":
        ins["semb"] = cu(inp["semb"])
        e_arg = None
        if e_pre:
            ins["e_wide"] = cu(inp["e_wide"])
            e_arg = ins["e_wide"][:, BR.E_OFF:BR.E_OFF + case.cout]
        fwd = lambda c_: blk.fwd(c_, x, ins["semb"], B, H, W, out=out_g.view, e_pre=e_arg)
    else:
        ins["c"] = cu(inp["c"].reshape(-1, BR.CTX_DIM))
        kv = blk.attn2.project_context(ctx, ins["c"]) if case.train == "frozen" else None      # the UNet's context K / V
        ip = None
        if run.ip:
            ins["c_ip"] = cu(inp["c_ip"].reshape(-1, BR.CTX_DIM))
            ip = blk.attn2.project_ip(ctx, ins["c_ip"]) + (BR.NIP,)
        fwd = lambda c_, ip_=ip: blk.fwd(c_, x, ins["c"], B, H, W, BR.NCTX, out=out_g.view, kv_cache=kv, ip=ip_)
    out, saved = fwd(ctx)
    torch.cuda.synchronize()
    got = dict(out=out_g.view.clone())
    guards = dict(out=out_g.check())
    assert (saved is not None) == run.record

    state = {}

    def backward():
        """One block backward on fresh accumulation targets (the weight-gradient queue is left to the caller)."""
        if case.kind == "res":
            state["dsemb"] = cu(inp["dsemb0"]) if (case.train != "frozen" and not deslot) else None
            state["de_wide"] = inp["de_wide0"].float().to(dev) if deslot else None
            slot = state["de_wide"][:, BR.E_OFF:BR.E_OFF + case.cout] if deslot else None
            return blk.bwd(ctx, dout, saved, B, H, W, dsemb=state["dsemb"], need_emb_grads=case.train != "frozen",
                           out=dx_g.view, de_slot=slot)
        return blk.bwd(ctx, dout, saved, B, H, W, BR.NCTX, out=dx_g.view)

    def finish():
        ctx.flush_wgrad()          # what ControlNetE._done does at the end of a stage
        ctx.retire_wgrad()
        torch.cuda.synchronize()

    exact = {}
    if run.backward:
        if run.variant == "wstream":
            ctx.wstream = hip.side_stream(dev)      # engine/model.py: self._side, with its registered split-K scratch
        before = {k: v.clone() for k, v in ins.items()}
        saved_t = _tensors(saved)
        saved_before = [t.clone() for t in saved_t]
        for ts in sets:
            ts.flat_grad.zero_()
        backward()
        queued = len(ctx._wq)
        finish()
        got["dx"] = dx_g.view.clone()
        guards["dx"] = dx_g.check()
        exact["inputs_changed"] = [k for k, v in ins.items() if not _same(v, before[k])]
        exact["saved_changed"] = [i for i, (a, b_) in enumerate(zip(saved_t, saved_before)) if not _same(a, b_)]
        if state.get("dsemb") is not None:
            got["dsemb"] = state["dsemb"].clone()
        if deslot:
            wide, wide0 = state["de_wide"], inp["de_wide0"].float().to(dev)
            got["de"] = wide[:, BR.E_OFF:BR.E_OFF + case.cout].clone()
            keep = torch.ones_like(wide, dtype=torch.bool)
            keep[:, BR.E_OFF:BR.E_OFF + case.cout] = False
            exact["de_outside_changed"] = int((wide[keep] != wide0[keep]).sum())
        # flat gradient buffers: expected slices non-zero, everything else (alignment padding included) exactly zero
        g1 = [ts.flat_grad.clone() for ts in sets]
        outside, empty = 0, []
        for ts, g in zip(sets, g1):
            mask = torch.zeros_like(g, dtype=torch.bool)
            for t in ts.items:
                if t.name in params:
                    n = t.grad.numel()
                    mask[t.offset:t.offset + n] = True
                    if not bool((g[t.offset:t.offset + n] != 0).any()):
                        empty.append(t.name)
                    got[t.name] = t.param_view(t.grad).clone()
            outside += int((g[~mask] != 0).sum())
        exact["flat_outside_nonzero"], exact["flat_empty_slices"] = outside, empty
        # the += contract: a second backward from the same saved state, nothing zeroed.  (Flushed in between, as every stage of
        # the trunk is: one grouped launch takes ONE problem per dW -- its reduce pass adds the slab sum without atomics.)
        if sets:
            backward()
            finish()
            exact["twice_rel"] = max(BR.rel(ts.flat_grad, 2.0 * g) for ts, g in zip(sets, g1))
            if bf and run.variant != "wstream":
                if "wq_per_bwd" in want:
                    assert queued == want["wq_per_bwd"], queued
                if want.get("wq_auto_flush"):        # 32 problems in one backward: the flush at 24 fires inside the block
                    assert queued == 32 - 24, queued
        ctx.wstream = None

    # ---- extra forwards of particular runs
    if run.case == "rb-frozen":
        o2, s2 = fwd(blocks.Ctx(dtype, dev, False))
        torch.cuda.synchronize()
        assert s2 is None and _same(o2, got["out"])
    if run.variant == "norecord":
        o2, s2 = fwd(blocks.Ctx(dtype, dev, True))
        torch.cuda.synchronize()
        assert s2 is not None
        got["out_recorded"] = o2.clone()
    if run.ip:
        # ip_scale = 0: bit-identical to the same block run without an image prompt
        blk0, _, _ = BR.build_block(case, BR.make_sd(case, SEED, 0.0), dtype)
        assert not blk0.attn2.ip_live()
        c0 = blocks.Ctx(dtype, dev, False)
        kv0 = blk0.attn2.project_context(c0, ins["c"])
        a, _ = blk0.fwd(c0, x, ins["c"], B, H, W, BR.NCTX, kv_cache=kv0, ip=ip)
        b_, _ = blk0.fwd(c0, x, ins["c"], B, H, W, BR.NCTX, kv_cache=kv0, ip=None)
        torch.cuda.synchronize()
        assert _same(a, b_)

    # ---- figures first, then the assertions
    cmp_ = BR.evaluate(case, sd, inp, run.mode, e_pre=e_pre, ip=run.ip, backward=run.backward) if bf else None
    rows, fails = {}, []
    for k in names:
        r, c_ = ref[k], (None if cmp_ is None else cmp_[k])
        if k == "de":      # the slot accumulates: pre-fill + d emb_out
            pre = inp["de_wide0"][:, BR.E_OFF:BR.E_OFF + case.cout].double()
            r, c_ = pre + r, (None if c_ is None else pre + c_)
        g = got[k].reshape(r.shape) if got[k].numel() == r.numel() else got[k]
        e = BR.rel(g, r)
        if bf:
            f = BR.rel(c_, r)
            rows[k] = dict(engine=e, comparator=f, ratio=(e / f if f > 0 else None))
            if (e > GATE * f) if f > 0 else (e > F32_GRAD):
                fails.append(k)
        else:
            rows[k] = dict(engine=e)
            if e > (F32_ACT if k == "out" else F32_GRAD):
                fails.append(k)
    if run.variant == "norecord":
        # two bf16 evaluations of one function, each within the gate of the exact one, differ by no more than the gate:
        # independent roundings add in quadrature (sqrt(2) x floor), the fused GEGLU only removes one rounding
        rows["out_recorded"] = dict(engine=BR.rel(got["out_recorded"], got["out"]), comparator=rows["out"]["comparator"])
        if rows["out_recorded"]["engine"] > GATE * rows["out"]["comparator"]:
            fails.append("out_recorded")
    for k, v in rows.items():
        print(f"{run.id:28s} {k:70s} " + " ".join(f"{a}={b:.3e}" if isinstance(b, float) else f"{a}={b}" for a, b in v.items()))
    print(run.id, "guards", guards, "exact", exact)
    if bf:
        wk = max((k for k in rows if rows[k].get("ratio") is not None), key=lambda k: rows[k]["ratio"])
        worst = dict(output=wk, **rows[wk])
    else:
        wk = max(rows, key=lambda k: rows[k]["engine"])
        worst = dict(output=wk, engine=rows[wk]["engine"], out=rows["out"]["engine"])
    _RESULTS[run.id] = worst
    _record("block_conformance/" + run.id, predicates=asserted, failed=fails, exact={k: v for k, v in exact.items()}, **worst)

    for g in guards.values():
        assert g == dict(guard_rows=0, pad_elems=0, nan_left=0), guards
    assert not exact.get("inputs_changed") and not exact.get("saved_changed"), exact
    assert not exact.get("de_outside_changed"), exact
    assert not exact.get("flat_outside_nonzero") and not exact.get("flat_empty_slices"), exact
    assert exact.get("twice_rel", 0.0) <= 1e-5, exact
    assert not fails, {k: rows[k] for k in fails}


def test_zz_block_conformance_summary():
    """Wall time of the block tests of this session, the worst engine / comparator ratio per bf16 run, the fp32 maxima."""
    _need_gpu()
    wall = None if _T0[0] is None else time.time() - _T0[0]
    bf = {k: v for k, v in _RESULTS.items() if "ratio" in v}
    f32 = {k: v for k, v in _RESULTS.items() if "ratio" not in v}
    _record("block_conformance/summary", wall_s=wall, runs=len(_RESULTS),
            worst_ratio={k: (v["ratio"], v["output"]) for k, v in bf.items()},
            f32_out_max=max((v["out"] for v in f32.values()), default=None),
            f32_worst={k: (v["engine"], v["output"]) for k, v in f32.items()})
    assert all(v["ratio"] <= GATE for v in bf.values())
