"""Cases, seeded inputs and the runner of the step's bit-pattern golden (helpers only: nothing here is collected).  Used by
tests/golden/make_golden_step_bits.py, which records tests/golden/step_bits.pt from a build of ANOTHER commit, and by
tests/test_gpu_step_bits.py, which holds the library under test to that record.

The AdamW update and the p_losses reduction are each written once in csrc/elementwise.hip, so the tests that compare two entry
points with each other compare one expression with itself.  What the bits ARE is kept here instead: every output of every case
below as the int32 pattern of its floats, recorded through the C ABI alone (ctypes; torch only owns the device memory).

AdamW, every step of STEPS on every size it can run at --
    n = 1              under one 64-float chunk
    n = 1000           ragged: 15 chunks and 40 elements (the one-group entries only: cl_adamw_dev_groups needs whole chunks)
    n = 64 * 33        whole chunks
    n = 2^20 + 64      one more chunk than the largest grid covers in one trip: a second trip of the grid-stride loop
    cl_adamw, cl_adamw_dev, cl_adamw_dev_clip (coefficient 1.0 and 0.37), cl_adamw_dev_groups (4 groups, a map that changes group
    at every chunk, clip none or 0.37)
p_losses, B = 3, per = 1000 (1000 / 16 is no integer: ragged slices) --
    cl_p_losses_mse with and without lvlb; cl_p_losses_w for table / no table x l2 / Huber (delta 0.5), lvlb given, per_sample
    requested

Every buffer sits between 64-float guards.  run_cases() returns {case: {output: int32 tensor}} and asserts on the way that g, the
hyper table, the map, the inputs of the loss and every guard came back untouched.  An output is recorded as its SHA-256; the
pattern itself is kept as well (once per distinct pattern: m' and v' do not depend on the step, and several entry points agree)
at the smallest sizes an entry point runs at -- n = 1 and n = 1000 for the one-group entries, n = 64 * 33 for the grouped one,
every p_losses case -- which keeps the file under 200 KB.
"""
import functools
import hashlib

import torch

GUARD = 1e30
SIZES = [1, 1000, 64 * 33, (1 << 20) + 64]
STEPS = [1, 2, 1000]
COEF = 0.37
NGROUPS = 4
KEEP_ONE_GROUP, KEEP_GROUPED = (1, 1000), (64 * 33,)          # sizes whose patterns are stored, not only their digests
HYPER_KEYS = ("lr", "beta1", "beta2", "eps", "wd", "gscale")
LOSS_B, LOSS_PER, LOSS_T, HUBER_DELTA = 3, 1000, 1000, 0.5
LOSS_SCALARS = dict(gscale=0.5, w_simple=1.25, w_elbo=0.5)


def rows(ngroups=NGROUPS):
    """Hyper rows that differ in every one of lr / betas / eps / weight decay; grad_scale is common to all groups.  Row 0 is the
    `hyper` of the one-group entries."""
    return [(1e-3 * (1 + 0.7 * k), 0.9 - 0.05 * k, 0.999 - 0.01 * k, 1e-8 * 10 ** k, 1e-2 * k + 1e-2, 1.0 / 128) for k in range(ngroups)]


def table(ngroups=NGROUPS):
    return torch.tensor(rows(ngroups), dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def adam_state(n):
    """p, g, m, v (v >= 0) of n elements from a seeded CPU generator (cached: callers do not write them)."""
    g = torch.Generator().manual_seed(7000 + n % 9973)
    return (torch.randn(n, generator=g), torch.randn(n, generator=g) * 64, torch.randn(n, generator=g) * 0.1,
            torch.rand(n, generator=g) * 0.01)


def chunk_map(n):
    return (torch.arange(n // 64) % NGROUPS).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def loss_inputs():
    g = torch.Generator().manual_seed(7919)
    eps, target = torch.randn(LOSS_B, LOSS_PER, generator=g), torch.randn(LOSS_B, LOSS_PER, generator=g)
    t = torch.tensor([0, 417, LOSS_T - 1], dtype=torch.int64)
    lvlb = torch.rand(LOSS_T, generator=g) * 2e-3 + 1e-5
    wt = torch.rand(LOSS_T, generator=g) * 0.9 + 0.1
    return dict(eps=eps, target=target, t=t, lvlb=lvlb, wt=wt)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).reshape(-1)


def sha(pattern):
    return hashlib.sha256(pattern.numpy().tobytes()).hexdigest()


def inputs_digest():
    """One digest over every seeded input: a torch whose CPU generators draw other numbers shows here, not as a kernel mismatch."""
    h = hashlib.sha256()
    for n in SIZES:
        for x in adam_state(n):
            h.update(bits(x).numpy().tobytes())
    li = loss_inputs()
    for k in ("eps", "target", "lvlb", "wt"):
        h.update(bits(li[k]).numpy().tobytes())
    h.update(bits(table()).numpy().tobytes())
    return h.hexdigest()


class Guarded:
    """A device copy of `values` between 64-element guards (1e30 for floats, 0xA5 bytes otherwise)."""

    def __init__(self, values):
        values = values.reshape(-1)
        self.n, self.src = values.numel(), values.clone()
        self.fill = GUARD if values.dtype == torch.float32 else {torch.uint8: 0xA5, torch.int64: -6148914691236517206}[values.dtype]
        self.buf = torch.full((64 + self.n + 64,), self.fill, dtype=values.dtype, device="cuda")
        self.view = self.buf[64:64 + self.n]
        self.view.copy_(values)

    @property
    def ptr(self):
        return self.view.data_ptr()

    def guards_intact(self):
        return bool((self.buf[:64] == self.fill).all()) and bool((self.buf[64 + self.n:] == self.fill).all())

    def untouched(self):
        return self.guards_intact() and torch.equal(self.view.cpu().view(torch.uint8), self.src.view(torch.uint8))


def adamw_cases():
    """[(case name, entry point, n, step, clip coefficient or None)]"""
    out = []
    for n in SIZES:
        for step in STEPS:
            out += [(f"adamw/n{n}/s{step}", "cl_adamw", n, step, None), (f"adamw_dev/n{n}/s{step}", "cl_adamw_dev", n, step, None),
                    (f"adamw_dev_clip/n{n}/s{step}/c1.0", "cl_adamw_dev_clip", n, step, 1.0),
                    (f"adamw_dev_clip/n{n}/s{step}/c{COEF}", "cl_adamw_dev_clip", n, step, COEF)]
            if n % 64 == 0:
                out += [(f"adamw_dev_groups/n{n}/s{step}/none", "cl_adamw_dev_groups", n, step, None),
                        (f"adamw_dev_groups/n{n}/s{step}/c{COEF}", "cl_adamw_dev_groups", n, step, COEF)]
    return out


def loss_cases():
    """[(case name, entry point, lvlb given, table given, kind)]"""
    out = [("p_losses_mse/lvlb", "cl_p_losses_mse", True, False, 0), ("p_losses_mse/no_lvlb", "cl_p_losses_mse", False, False, 0)]
    for tab in (True, False):
        for kind in (0, 1):
            out.append((f"p_losses_w/{'table' if tab else 'no_table'}/{'huber' if kind else 'l2'}", "cl_p_losses_w", True, tab, kind))
    return out


def keeps_pattern(case):
    """Is this case's pattern stored in the fixture (True) or only its digest?"""
    if case.startswith("p_losses"):
        return True
    n = int(case.split("/")[1][1:])
    return n in (KEEP_GROUPED if case.startswith("adamw_dev_groups") else KEEP_ONE_GROUP)


def _run_adamw(L, st, entry, n, step, coef):
    p, g, m, v = (Guarded(x) for x in adam_state(n))
    tab = Guarded(table().reshape(-1))
    stepd = torch.tensor([step], dtype=torch.int32, device="cuda")
    clip = None if coef is None else Guarded(torch.tensor([3.25, coef], dtype=torch.float32))
    cmap = None
    if entry == "cl_adamw":
        lr, b1, b2, eps, wd, gs = rows()[0]
        rc = L.cl_adamw(p.ptr, g.ptr, m.ptr, v.ptr, n, lr, b1, b2, eps, wd, step, gs, st)
    elif entry == "cl_adamw_dev":
        rc = L.cl_adamw_dev(p.ptr, g.ptr, m.ptr, v.ptr, n, tab.ptr, stepd.data_ptr(), st)
    elif entry == "cl_adamw_dev_clip":
        rc = L.cl_adamw_dev_clip(p.ptr, g.ptr, m.ptr, v.ptr, n, tab.ptr, stepd.data_ptr(), clip.ptr, st)
    else:
        cmap = Guarded(chunk_map(n))
        rc = L.cl_adamw_dev_groups(p.ptr, g.ptr, m.ptr, v.ptr, n, tab.ptr, NGROUPS, cmap.ptr, stepd.data_ptr(),
                                   None if clip is None else clip.ptr, st)
    assert rc == 0, (entry, n, step, coef, rc)
    torch.cuda.synchronize()
    assert int(stepd) == step, "the step counter was written"
    for name, buf in (("p", p), ("m", m), ("v", v)):
        assert buf.guards_intact(), f"{entry} n={n}: a guard around {name} was written"
    for name, buf in (("g", g), ("the hyper table", tab), ("the clip pair", clip), ("the map", cmap)):
        assert buf is None or buf.untouched(), f"{entry} n={n}: {name} or a guard around it was written"
    return dict(p=bits(p.view), m=bits(m.view), v=bits(v.view))


def _run_loss(L, st, entry, with_lvlb, with_table, kind):
    li = loss_inputs()
    eps, target, t, lvlb, wt = (Guarded(li[k]) for k in ("eps", "target", "t", "lvlb", "wt"))
    nan = float("nan")
    d_eps, out, per_sample, scratch = (Guarded(torch.full((k,), nan)) for k in (LOSS_B * LOSS_PER, 3, LOSS_B, 16 * LOSS_B))
    s = LOSS_SCALARS
    args = (eps.ptr, target.ptr, d_eps.ptr, t.ptr, lvlb.ptr if with_lvlb else None, out.ptr, per_sample.ptr, scratch.ptr, LOSS_B,
            LOSS_PER, s["gscale"], s["w_simple"], s["w_elbo"])
    if entry == "cl_p_losses_mse":
        rc = L.cl_p_losses_mse(*args, st)
    else:
        rc = L.cl_p_losses_w(*args, wt.ptr if with_table else None, kind, HUBER_DELTA, st)
    assert rc == 0, (entry, with_lvlb, with_table, kind, rc)
    torch.cuda.synchronize()
    for name, buf in (("d_eps", d_eps), ("out", out), ("per_sample", per_sample), ("scratch", scratch)):
        assert buf.guards_intact(), f"{entry}: a guard around {name} was written"
    for name, buf in (("eps", eps), ("target", target), ("t", t), ("lvlb", lvlb), ("wt", wt)):
        assert buf.untouched(), f"{entry}: {name} or a guard around it was written"
    return dict(d_eps=bits(d_eps.view), out=bits(out.view), per_sample=bits(per_sample.view), scratch=bits(scratch.view))


def run_cases(L, st):
    """Every case through the C ABI of the loaded library `L` (ctypes, argtypes set) on stream `st`: {case: {output: int32}}."""
    res = {}
    for name, entry, n, step, coef in adamw_cases():
        res[name] = _run_adamw(L, st, entry, n, step, coef)
    for name, entry, with_lvlb, with_table, kind in loss_cases():
        res[name] = _run_loss(L, st, entry, with_lvlb, with_table, kind)
    return res
