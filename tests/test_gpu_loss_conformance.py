"""Kernel-level conformance of cl_p_losses_w (ctypes -> C ABI): every case of tests/loss_ref.py element-wise against the fp64
contract, inside the canary buffers of tests/test_gpu_ew_conformance.py.

Per case the call is launched twice into fresh buffers: NaN-filled views (out, per_sample, d_eps, scratch) inside buffers of a fixed
bit pattern, G guard elements either side.  After every launch the probe must report the entry point's record, no guard and no
operand may have changed and no NaN may be left in an output; the gated outputs pass tests/loss_ref's bounds with zero violations;
the two launches give the same bits.  Then, bit for bit: wt == NULL with l2 against cl_p_losses_mse, and a captured launch replayed
after t and wt were overwritten in place against an eager launch on the new values."""
import pytest
import torch

from tests import ew_ref as R
from tests import loss_ref as LR
from tests.test_gpu_bench_shapes import _need_gpu, _record
from tests.test_gpu_ew_conformance import _Out, _lib, _p, _probe

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = torch.float32
IDS = [c["name"] for c in LR.CASES]


class _Call:
    """One prepared launch: operands as flat device copies, outputs as canary views; static, so it can be captured."""

    def __init__(self, p, ops, api="w"):
        self.p, self.api = p, api
        self.ops = {k: ops[k].to(DEV).contiguous().clone() for k in ("eps", "target", "t", "lvlb", "wt")}
        B, per = p["B"], p["per"]
        self.outs = dict(out=_Out((3,), F32), scratch=_Out((16 * B,), F32))
        if p["per_sample"]:
            self.outs["per_sample"] = _Out((B,), F32)
        if p["d_eps"]:
            self.outs["d_eps"] = _Out((B, per), F32)

    def view(self, k):
        return self.outs[k].view if k in self.outs else None

    def __call__(self):
        L, st = _lib()
        p, o = self.p, self.ops
        args = (_p(o["eps"]), _p(o["target"]), _p(self.view("d_eps")), _p(o["t"]), _p(o["lvlb"]) if p["lvlb"] else None,
                _p(self.view("out")), _p(self.view("per_sample")), _p(self.view("scratch")), p["B"], p["per"], p["gscale"], p["w_simple"],
                p["w_elbo"])
        if self.api == "mse":
            return L.cl_p_losses_mse(*args, st)
        return L.cl_p_losses_w(*args, _p(o["wt"]) if p["wt"] else None, p["kind"], p["delta"], st)

    def want(self):
        form = 0 if self.api == "mse" else 4 | (self.p["kind"] << 1) | int(self.p["wt"])
        return R.probe("plosses", None, (16, self.p["B"]), form=form)

    def launch(self):
        """(canary count, probe) of one eager launch."""
        snap = {k: R.bits(v).clone() for k, v in self.ops.items()}
        rc = self()
        assert rc == 0, ("return code", rc)
        pr = _probe()
        torch.cuda.synchronize()
        return self.canary(snap), pr

    def canary(self, snap):
        n = sum(h.guards() if k == "scratch" else h.bad() for k, h in self.outs.items())
        return n + sum(int((R.bits(v) != snap[k]).sum()) for k, v in self.ops.items())

    def same_bits(self, other, keys=("out", "per_sample", "d_eps")):
        return {k: R.same_bits(self.outs[k].view, other.outs[k].view) for k in keys if k in self.outs}


@pytest.mark.parametrize("p", LR.CASES, ids=IDS)
def test_every_case_against_the_fp64_contract(p):
    _need_gpu()
    ops = LR.make_ops(p, DEV)
    if p["kind"] == 1 and p["per"] >= 256:
        assert min(LR.huber_shares(p, ops)) >= 0.25, LR.huber_shares(p, ops)       # erf(0.5) = 0.52 inside
    specs = LR.eval_plosses_w(p, ops)
    runs = [_Call(p, ops) for _ in range(2)]
    results = [c.launch() for c in runs]
    for c, (canary, pr) in zip(runs, results):
        assert canary == 0, ("canary", canary)
        assert pr == c.want(), (pr, c.want())
        res = R.check(specs, {k: c.outs[k].view for k in specs})
        print(p["name"], {k: (r["violations"], round(r["err_over_bound"], 4)) for k, r in res.items()})
        _record("loss_conformance", case=p["name"], eob={k: r["err_over_bound"] for k, r in res.items()})
        assert set(res) == set(specs) and not R.failures(res), R.failures(res)
    assert all(R.same_bits(runs[0].outs[k].buf, runs[1].outs[k].buf) for k in runs[0].outs), "two launches differ"


@pytest.mark.parametrize("B,per", LR.SHAPES, ids=[f"{B}x{per}" for B, per in LR.SHAPES])
@pytest.mark.parametrize("lvlb", [False, True], ids=["nolvlb", "lvlb"])
def test_no_table_l2_has_the_bits_of_p_losses_mse(B, per, lvlb):
    _need_gpu()
    p = dict(LR.CASE[f"plosses_w-{B}x{per}-l2-nowt"], d_eps=True, per_sample=True, lvlb=lvlb)
    ops = LR.make_ops(p, DEV)
    new, old = _Call(p, ops, "w"), _Call(p, ops, "mse")
    (c_new, pr_new), (c_old, pr_old) = new.launch(), old.launch()
    assert c_new == 0 and c_old == 0 and pr_new == new.want() and pr_old == old.want()
    same = new.same_bits(old)
    assert same == dict(out=True, per_sample=True, d_eps=True), same
    assert torch.equal(new.outs["d_eps"].view, old.outs["d_eps"].view) and torch.equal(new.outs["out"].view, old.outs["out"].view)
    assert torch.equal(new.outs["per_sample"].view, old.outs["per_sample"].view)


REPLAY = ["plosses_w-3x4099-l2-wt", "plosses_w-3x4099-huber-wt", "plosses_w-8x15-huber-wt", "plosses_w-8x256-l2-wt", "plosses_w-1x16-huber-wt"]


@pytest.mark.parametrize("name", REPLAY)
def test_a_captured_launch_follows_t_and_wt(name):
    """Captured once; t and wt are then overwritten in place and the graph replayed: the bits of an eager launch on the new values,
    and other bits than before."""
    _need_gpu()
    p = dict(LR.CASE[name], d_eps=True, per_sample=True, lvlb=True)
    ops = LR.make_ops(p, DEV)
    cap = _Call(p, ops)
    canary, _ = cap.launch()                                   # eager first: the code object is loaded before the capture
    assert canary == 0
    first = {k: cap.outs[k].view.clone() for k in ("out", "per_sample", "d_eps")}
    snap = {k: R.bits(v).clone() for k, v in cap.ops.items()}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert cap() == 0
    for k in ("out", "per_sample", "d_eps", "scratch"):
        cap.outs[k].view.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert cap.canary(snap) == 0
    assert all(torch.equal(cap.outs[k].view, first[k]) for k in first), "a replay on unchanged inputs gives the eager bits"
    # new values, in place: other timesteps (T - 1 - t) and another table
    new_t = (LR.T - 1 - ops["t"]).to(DEV)
    new_wt = torch.flip(ops["wt"], (0,)).to(DEV) * 0.5 + 0.25
    cap.ops["t"].copy_(new_t)
    cap.ops["wt"].copy_(new_wt)
    snap = {k: R.bits(v).clone() for k, v in cap.ops.items()}
    for k in ("out", "per_sample", "d_eps", "scratch"):
        cap.outs[k].view.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert cap.canary(snap) == 0
    eager = _Call(p, dict(ops, t=new_t, wt=new_wt))
    canary, pr = eager.launch()
    assert canary == 0 and pr == eager.want()
    same = cap.same_bits(eager)
    assert same == dict(out=True, per_sample=True, d_eps=True), same
    assert not torch.equal(cap.outs["d_eps"].view, first["d_eps"]) and not torch.equal(cap.outs["out"].view, first["out"])
    specs = LR.eval_plosses_w(p, dict(ops, t=new_t, wt=new_wt))
    res = R.check(specs, {k: cap.outs[k].view for k in specs})
    assert not R.failures(res), R.failures(res)


def test_refused_call_launches_nothing():
    """A refusal after a good launch: CL_EINVAL, the record reset, no output touched."""
    _need_gpu()
    p = dict(LR.CASE["plosses_w-3x16-huber-wt"], d_eps=True, per_sample=True)
    ops = LR.make_ops(p, DEV)
    good = _Call(p, ops)
    assert good.launch()[0] == 0
    for bad in (dict(kind=2), dict(delta=0.0), dict(delta=float("inf")), dict(B=0)):
        c = _Call(p, ops)
        c.p = dict(p, **bad)
        assert c() == 1
        assert _probe() == dict.fromkeys(R.PROBE_FIELDS, 0)
        torch.cuda.synchronize()
        assert all(h.guards() == 0 and bool(torch.isnan(h.view).all()) for h in c.outs.values()), bad
