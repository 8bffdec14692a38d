"""Kernel-level conformance of cl_loss_bands (ctypes -> C ABI) on an MI355X: every case of tests/val_ref.py bit for bit on all
3 (nbands + 1) doubles against the fp64 Python loop (NaNs canonicalised: tests/val_ref.canon), the table sitting between guard
rows of a fixed bit pattern that must not change, the operands untouched, the launch record as predicted, two launches of one
case giving the same bits.  Then every refusal (nothing launched, nothing written), and a captured launch replayed after
per_sample, t and *n_valid were overwritten in place."""
import ctypes

import pytest
import torch

from tests import val_ref as V

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 8                    # guard rows of 3 doubles before and after the table
PATTERN = 0x7FF4DEADBEEF0123  # a signalling-NaN pattern no sum produces
EW_LOSS_BANDS = 44           # csrc/elementwise.h
IDS = [c["name"] for c in V.CASES]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ctrlora_amd import hip
    return hip.lib(), hip.stream()


def _probe():
    from ctrlora_amd import hip
    out = (ctypes.c_int * 8)()
    assert hip.lib().cl_debug_ew_last_launch(out) == 0
    return dict(zip(("id", "dtype", "gx", "gy", "gz", "threads", "form", "aux"), list(out)))


class _Call:
    """One prepared launch on static device buffers: acc is a view between guard rows."""

    def __init__(self, c, x, t, acc0):
        self.c = c
        nb = c["nbands"]
        self.x, self.t = x.to(DEV).contiguous().clone(), t.to(DEV).contiguous().clone()
        self.raw = torch.full(((nb + 1 + 2 * GUARD) * 3,), PATTERN, dtype=torch.int64, device=DEV)
        self.acc = self.raw.view(torch.float64)[GUARD * 3:(GUARD + nb + 1) * 3].view(nb + 1, 3)
        self.acc.copy_(acc0)
        nv = c["n_valid"]
        self.nv = None if nv is None else torch.tensor([nv], dtype=torch.int32, device=DEV)

    def __call__(self, **over):
        L, st = _need_gpu()
        c = self.c
        a = dict(x=self.x.data_ptr(), t=self.t.data_ptr(), B=c["B"], T=c["T"], nbands=c["nbands"],
                 nv=None if self.nv is None else self.nv.data_ptr(), acc=self.acc.data_ptr())
        a.update(over)
        return L.cl_loss_bands(a["x"], a["t"], a["B"], a["T"], a["nbands"], a["nv"], a["acc"], st)

    def guards_bad(self):
        n = GUARD * 3
        return int((self.raw[:n] != PATTERN).sum()) + int((self.raw[-n:] != PATTERN).sum())

    def want(self):
        return dict(id=EW_LOSS_BANDS, dtype=-1, gx=1, gy=1, gz=1, threads=128, form=int(self.nv is not None), aux=self.c["nbands"])


def _bits(t):
    return t.contiguous().view({4: torch.int32, 8: torch.int64}[t.element_size()]).clone()


@pytest.mark.parametrize("c", V.CASES, ids=IDS)
def test_every_case_has_the_bits_of_the_fp64_loop(c):
    _need_gpu()
    x, t, acc0 = V.make_ops(c)
    ref = V.reference(c["name"])
    runs = [_Call(c, x, t, acc0) for _ in range(2)]
    for call in runs:
        sx, stt = _bits(call.x), _bits(call.t)
        assert call() == 0
        assert _probe() == call.want(), (_probe(), call.want())
        torch.cuda.synchronize()
        assert call.guards_bad() == 0, "a guard row changed"
        assert torch.equal(_bits(call.x), sx) and torch.equal(_bits(call.t), stt), "an operand changed"
        got = call.acc.cpu()
        diff = (V.canon(got) != V.canon(ref)).nonzero().tolist()
        print(c["name"], "rows differing:", diff[:6], "total row", got[-1].tolist(), "ref", ref[-1].tolist())
        assert V.same_bits(got, ref), diff[:10]
    assert torch.equal(runs[0].raw, runs[1].raw) or V.same_bits(runs[0].acc.cpu(), runs[1].acc.cpu()), "two launches differ"


@pytest.mark.parametrize("name", ["B65-nb10-random", "edges-nb7", "B3-nvalid1", "nan-and-inf", "B1025"])
def test_two_consecutive_launches_add_twice(name):
    """The second launch starts from what the first left: the reference applied to its own result."""
    _need_gpu()
    c = V.CASE[name]
    x, t, acc0 = V.make_ops(c)
    once = V.reference(name)
    twice = torch.tensor(V.ref_bands(x.double().tolist(), t.tolist(), c["T"], c["nbands"], c["n_valid"], once.tolist()),
                         dtype=torch.float64)
    call = _Call(c, x, t, acc0)
    assert call() == 0 and call() == 0
    torch.cuda.synchronize()
    assert call.guards_bad() == 0 and V.same_bits(call.acc.cpu(), twice)
    assert not V.same_bits(once, twice) or c["n_valid"] == 0


def test_refusals_launch_nothing_and_write_nothing():
    L, st = _need_gpu()
    c = V.CASE["B65-nb10-random"]
    x, t, acc0 = V.make_ops(c)
    good = _Call(c, x, t, acc0)
    assert good() == 0
    torch.cuda.synchronize()
    call = _Call(c, x, t, acc0)
    before = call.raw.clone()
    bad = [dict(x=None), dict(t=None), dict(acc=None), dict(B=0), dict(B=-1), dict(B=65536), dict(T=0), dict(T=-3),
           dict(nbands=0), dict(nbands=-1), dict(nbands=65), dict(T=5, nbands=6), dict(acc=call.acc.data_ptr() + 4),
           dict(acc=call.acc.data_ptr() + 1)]
    for over in bad:
        assert call(**over) == 1, over
        assert _probe() == dict.fromkeys(("id", "dtype", "gx", "gy", "gz", "threads", "form", "aux"), 0), over
    torch.cuda.synchronize()
    assert torch.equal(call.raw, before), "a refused call wrote"
    # the limits themselves are accepted: B = 65535 is the largest batch, nbands = min(T, 64) the most bands
    big = dict(V.CASE["B65-nb10-random"], B=65535, nbands=64, n_valid=None)
    xb, tb = torch.ones(65535), torch.arange(65535) % 1000
    cb = _Call(big, xb, tb, torch.zeros(65, 3, dtype=torch.float64))
    assert cb() == 0
    torch.cuda.synchronize()
    assert cb.guards_bad() == 0 and float(cb.acc[-1, 0]) == 65535.0 == float(cb.acc[-1, 1]) == float(cb.acc[:-1, 0].sum())
    c3 = _Call(dict(c, T=5, nbands=5), x, t % 5, torch.zeros(6, 3, dtype=torch.float64))
    assert c3() == 0


def test_a_captured_launch_follows_per_sample_t_and_n_valid():
    """Captured once with a device n_valid; the three are then overwritten in place and the graph replayed, twice: the table
    follows, with the bits of the reference applied to the same sequence of inputs."""
    _need_gpu()
    c = dict(V.CASE["B65-nb10-random"], n_valid=65)
    x, t, acc0 = V.make_ops(c)
    call = _Call(c, x, t, acc0)
    assert call() == 0                                   # eager first: the code object is loaded before the capture
    torch.cuda.synchronize()
    want = V.reference("B65-nb10-random")
    assert V.same_bits(call.acc.cpu(), want)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert call() == 0
    torch.cuda.synchronize()
    assert V.same_bits(call.acc.cpu(), want), "capturing executes nothing"
    for k, nv in enumerate((40, 7)):
        g = torch.Generator().manual_seed(7 + k)
        x2 = torch.rand(c["B"], generator=g) * 3.0
        t2 = torch.randint(0, c["T"], (c["B"],), generator=g)
        call.x.copy_(x2)
        call.t.copy_(t2)
        call.nv.fill_(nv)
        graph.replay()
        torch.cuda.synchronize()
        want = torch.tensor(V.ref_bands(x2.double().tolist(), t2.tolist(), c["T"], c["nbands"], nv, want.tolist()), dtype=torch.float64)
        assert call.guards_bad() == 0
        assert V.same_bits(call.acc.cpu(), want), (k, nv)
        assert float(call.acc[-1, 0]) == float(acc0[-1, 0]) + 65 + (40 if k == 0 else 47)


def test_the_python_wrapper_and_the_host_restatement_agree():
    """ctrlora_amd.hip.loss_bands (what the model calls) against ctrlora_amd.validation.accumulate_bands, after hip.zero_."""
    _need_gpu()
    from ctrlora_amd import hip
    from ctrlora_amd.validation import accumulate_bands, new_table
    c = V.CASE["B130-nb10-random"]
    x, t, _ = V.make_ops(c)
    acc = torch.full((11, 3), 5.0, dtype=torch.float64, device=DEV)
    hip.zero_(acc)
    nv = torch.tensor([100], dtype=torch.int32, device=DEV)
    hip.loss_bands(x.to(DEV), t.to(DEV), 1000, 10, acc, n_valid=nv)
    hip.loss_bands(x.to(DEV), t.to(DEV), 1000, 10, acc)
    host = new_table(10)
    accumulate_bands(x, t, 1000, 10, host, n_valid=100)
    accumulate_bands(x, t, 1000, 10, host)
    assert V.same_bits(acc.cpu(), host) and float(host[-1, 0]) == 230.0
