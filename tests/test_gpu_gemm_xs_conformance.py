"""Kernel-level conformance of the x-stationary streaming product (csrc/gemm_xs.hip, launch configuration 34) through cl_gemm:
all 16 instantiations of gemm_xs_kernel -- K1 in {320, 640} x K2 in {0, 128} x {plain, residual, act 3}, and the LayerNorm
prologue x K1 x {plain, act 3} -- element-wise against the fp64 contract of tests/gemm_ref.py at the small shapes where its
per-row, per-block and per-chunk arithmetic can go wrong (tests/xs_ref.py: CASES).

Every row is launched with configuration 34 and its run count forced, twice, and gets: the four checks of tests/gemm_ref.py with
the derived widenings of the two x-stationary-only forms (zero violations), the statistics gate on ln_stats (a guarded [M, 2]
fp32 buffer), bit-identical buffers from the two launches, and a launch-tag record equal to what the transcription of the
launcher says: ceil(M / 128) groups nsplit workgroups of 256 threads.  The output is a NaN-filled view in a guarded buffer; every
operand has a row pitch of its own, and its pad holds NaN (the kernel reads operands through whole 16-byte vectors inside their
width).  In-place residual rows (C == residual) are compared bit for bit with the out-of-place launch."""
import json
import time

import pytest
import torch

from tests import gemm_ref as G
from tests import xs_ref as X
from tests.gemm_ref import _tags
from tests.test_gpu_bench_shapes import _need_gpu, _record

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
_STATS = {}
_T0 = [None]


class _forced:
    def __init__(self, cfg, runs):
        self.cfg, self.runs = cfg, runs

    def __enter__(self):
        from ctrlora_amd import hip
        L = hip.lib()
        L.cl_gemm_force_config(self.cfg)
        L.cl_gemm_force_splitk(self.runs)

    def __exit__(self, *exc):
        from ctrlora_amd import hip
        L = hip.lib()
        L.cl_gemm_force_config(-1)
        L.cl_gemm_force_splitk(0)
        return False


def _sig(c):
    from ctrlora_amd import hip
    return dict(dtype=hip.BF16, mode=c["mode"], M=c["M"], N=c["N"], K1=c["K1"], K2=c["K2"], act=c["act"], residual=int(c["residual"] is not None))


def _launch(c, fill, inplace=False, stats=True):
    """One cl_gemm call of the case: (output guard, statistics guard or None, launches of its signature, (workgroups, wg_size))."""
    from ctrlora_amd import hip
    guard = G.Guarded(c["M"], c["out_cols"], BF, "cuda")
    sg, ln = None, None
    if c["ln"] is not None:
        sg = G.Guarded(c["M"], 2, F32, "cuda", j=0) if stats else None
        ln = (c["ln"][0], c["ln"][1], c["ln"][2], None if sg is None else sg.view)
    if inplace:
        guard.view.copy_(c["residual"])
        res = guard.view
    else:
        res = G.padded(c["residual"], G.PAD_RES, fill)
    with _tags() as tags:
        hip.gemm(G.padded(c["a1"], G.PAD_A1, fill), G.padded(c["w1"], 8, fill), guard.view, a2=G.padded(c["a2"], G.PAD_A2, fill),
                 w2=G.padded(c["w2"], 16, fill), bias=c["bias"], residual=res, alpha=c["alpha"], beta=c["beta"], act=c["act"], k1=c["K1"],
                 N=c["N"], a2_group_n=c["a2_group_n"], alpha_n=c["alpha_n"], ln=ln)
        torch.cuda.synchronize()
        n, _ = tags.launches(**_sig(c))
        grid = [(t["workgroups"], t["wg_size"]) for t in hip.gemm_tags() if all(t[k] == v for k, v in _sig(c).items())]
    return guard, sg, n, (grid[0] if grid else None)


def _bits(guard):
    return guard.buf.view(torch.int16 if guard.buf.dtype == BF else torch.int32)


def _note(family, res, sres, launches):
    s = _STATS.setdefault(family, dict(launches=0, err_over_bound=0.0, rel=0.0, amb_rows=0.0, stat_err_over_bound=0.0, violations=0,
                                       canary=0, bit_diffs=0, form_mismatches=0, wall_s=0.0))
    s["launches"] += launches
    s["err_over_bound"] = max(s["err_over_bound"], res["err_over_bound"])
    s["rel"] = max(s["rel"], res["rel"])
    s["amb_rows"] = max(s["amb_rows"], res.get("amb_rows", 0.0))
    s["violations"] += res["violations"]
    s["canary"] += res["guard_rows"] + res["pad_elems"] + res["nan_left"]
    if sres is not None:
        s["stat_err_over_bound"] = max(s["stat_err_over_bound"], sres["err_over_bound"])
        s["violations"] += sres["violations"]
        s["canary"] += sres["guard_rows"] + sres["nan_left"]
    return s


def _one_row(row):
    """The launches and checks of one row of the table: a list of failures (empty = the row holds)."""
    t0 = time.time()
    c = X.build_case(row, "cuda")
    how_o, form_o = X.form_of(row)
    bad = []
    assert how_o == "xs", row["name"]                       # every row of the table is a product the kernel takes
    with _forced(34, row["nsplit"]):
        g1, s1, n1, grid1 = _launch(c, NAN, stats=row["stats"])
        g2, s2, n2, grid2 = _launch(c, NAN, stats=row["stats"])
    res = G.run_checks(c, g1.view, g1)
    sres = None
    if s1 is not None:
        sres = X.stats_gate(c, s1.view)
        sres.update({k: v for k, v in s1.check().items() if k != "pad_elems"})
        if sres["violations"] or sres["guard_rows"] or sres["nan_left"]:
            bad.append(("statistics", sres))
        if not torch.equal(_bits(s1), _bits(s2)):
            bad.append(("statistics differ between two launches",))
    st = _note(row["family"], res, sres, 2)
    f = G.failures(res)
    if f:
        bad.append((f, {k: res[k] for k in ("rel", "gate", "violations", "err_over_bound", "first_violation", "guard_rows", "pad_elems", "nan_left")}))
    if not torch.equal(_bits(g1), _bits(g2)):
        st["bit_diffs"] += 1
        bad.append(("two launches differ",))
    want = (form_o["workgroups"], 256)
    if not (n1 == 1 and n2 == 1 and grid1 == want and grid2 == want):
        st["form_mismatches"] += 1
        bad.append(("launch form", dict(launches=(n1, n2), grid=(grid1, grid2), transcription=want, form=form_o)))
    if row["inplace"]:
        # in place (C == residual), as the transformer block calls it: the four checks, the same form, and bit for bit the
        # out-of-place launch -- at M = 129 and 300 whole waves hold copies of row M - 1, which must not store
        with _forced(34, row["nsplit"]):
            gi, _, ni, gridi = _launch(c, NAN, inplace=True)
        resi = G.run_checks(c, gi.view, gi)
        _note(row["family"], resi, None, 1)
        if G.failures(resi):
            bad.append(("in place", G.failures(resi), {k: resi[k] for k in ("rel", "violations", "err_over_bound", "first_violation")}))
        if ni != 1 or gridi != want:
            st["form_mismatches"] += 1
            bad.append(("in place: launch form", ni, gridi, want))
        if not torch.equal(gi.view, g1.view):
            st["bit_diffs"] += 1
            bad.append(("in place differs from out of place", int((gi.view != g1.view).sum())))
    st["wall_s"] += time.time() - t0
    return bad, res, sres, form_o


@pytest.mark.parametrize("family", X.FAMILIES)
def test_x_stationary_family_elementwise_vs_fp64(family):
    _need_gpu()
    if _T0[0] is None:
        _T0[0] = time.time()
    rows = [r for r in X.CASES if r["family"] == family]
    failed = []
    for row in rows:
        bad, res, sres, form = _one_row(row)
        if bad:
            failed.append((row["name"], bad))
            _record("gemm_xs_conformance_row_failed", row=row["name"], failures=str(bad))
    s = _STATS[family]
    print("xs conformance", family, json.dumps(s))
    _record("gemm_xs_conformance_family", family=family, rows=len(rows), **s)
    assert not failed, failed


def test_zz_xs_conformance_summary():
    """One line for the file."""
    _need_gpu()
    wall = None if _T0[0] is None else time.time() - _T0[0]
    tot = dict(launches=sum(s["launches"] for s in _STATS.values()), err_over_bound=max([s["err_over_bound"] for s in _STATS.values()] or [0.0]),
               rel=max([s["rel"] for s in _STATS.values()] or [0.0]), amb_rows=max([s["amb_rows"] for s in _STATS.values()] or [0.0]),
               stat_err_over_bound=max([s["stat_err_over_bound"] for s in _STATS.values()] or [0.0]),
               violations=sum(s["violations"] for s in _STATS.values()), canary=sum(s["canary"] for s in _STATS.values()),
               bit_diffs=sum(s["bit_diffs"] for s in _STATS.values()), form_mismatches=sum(s["form_mismatches"] for s in _STATS.values()))
    print("xs conformance:", json.dumps(tot), "rows:", len(X.CASES), "wall_s:", wall)
    _record("gemm_xs_conformance_summary", rows=len(X.CASES), families=len(_STATS), wall_s=wall, **tot)
    for fam, s in _STATS.items():
        assert s["violations"] == 0 and s["canary"] == 0 and s["bit_diffs"] == 0 and s["form_mismatches"] == 0 and s["err_over_bound"] <= 1.0, (fam, s)
