"""Reference and case table of the loss-by-timestep-band table (cl_loss_bands, ctrlora_amd.validation.accumulate_bands) and
of ValPlan.  No GPU.

Contract (include/ctrlora_hip.h: cl_loss_bands): acc is double [nbands + 1][3] = {count, sum, sum of squares}, row nbands the
total; a call ADDS, sample by sample in index order, 1, x and x * x formed in fp64 from the fp32 loss x, to the row
band(t) = min(clamp(t, 0, T - 1) * nbands // T, nbands - 1) and to the total row; only the first clamp(n_valid, 0, B) samples
count (n_valid None: all).  `ref_bands` is that sentence as a Python loop over Python floats (IEEE doubles); the comparison is
bit for bit on all 3 (nbands + 1) doubles.  Bits of a NaN: which NaN a sum holds after a NaN went in (payload, sign) is not
part of the contract -- x86 and the GPU propagate payloads differently -- so `canon` maps every NaN to one pattern before
the bits are compared; where a NaN sits IS compared.

`model_bands(mutate=...)` restates the loop with one deliberate mistake each; tests/test_val_reference_model.py shows that
every mistake changes the bits of at least one case, i.e. that the table below can tell them apart.
"""
import math

import torch

T_DEFAULT = 1000
MUTATIONS = ("fp32", "edge", "reverse", "ignore_n_valid", "overwrite", "nan_leak")


def band(t, T, nbands):
    t = min(max(int(t), 0), T - 1)
    return min(t * nbands // T, nbands - 1)


def ref_bands(x, t, T, nbands, n_valid, acc0):
    """x: fp32 losses as Python floats, t: ints, acc0: [nbands + 1][3] Python floats.  Returns the new rows."""
    B = len(x)
    nv = B if n_valid is None else min(max(int(n_valid), 0), B)
    rows = [list(r) for r in acc0]
    for b in range(nv):
        for k in (band(t[b], T, nbands), nbands):
            rows[k][0] += 1.0
            rows[k][1] += x[b]
            rows[k][2] += x[b] * x[b]
    return rows


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def model_bands(x, t, T, nbands, n_valid, acc0, mutate=None):
    """ref_bands, or with mutate one of MUTATIONS: the same loop with one mistake."""
    assert mutate is None or mutate in MUTATIONS
    B = len(x)
    nv = B if (n_valid is None or mutate == "ignore_n_valid") else min(max(int(n_valid), 0), B)
    rows = [[0.0] * 3 for _ in acc0] if mutate == "overwrite" else [list(r) for r in acc0]
    order = range(nv - 1, -1, -1) if mutate == "reverse" else range(nv)
    for b in order:
        k = band(t[b] + 1, T, nbands) if mutate == "edge" else band(t[b], T, nbands)
        hit = (k, nbands)
        if mutate == "nan_leak" and not math.isfinite(x[b]):
            hit = range(nbands + 1)
        for r in hit:
            if mutate == "fp32":
                rows[r][0] = _f32(rows[r][0] + 1.0)
                rows[r][1] = _f32(rows[r][1] + x[b])
                rows[r][2] = _f32(rows[r][2] + _f32(x[b] * x[b]))
            else:
                rows[r][0] += 1.0
                rows[r][1] += x[b]
                rows[r][2] += x[b] * x[b]
    return rows


def ranges(T, nbands):
    lo = [-(-k * T // nbands) for k in range(nbands + 1)]
    return [(lo[k], lo[k + 1] - 1) for k in range(nbands)]


def edge_timesteps(T, nbands):
    """0, T - 1, out of range on both sides, and every band's first and last timestep (for 10 bands of 1000: 99 / 100, ...; for
    7 the values where t * 7 // 1000 steps: 142 / 143, 285 / 286, ...)."""
    vals = [0, T - 1, -1, T]
    for lo, hi in ranges(T, nbands):
        vals += [hi, lo]
    return vals


def _case(name, B, nbands, T=T_DEFAULT, tkind="random", xkind="spread", n_valid=None, acc0="zero", seed=0):
    return dict(name=name, B=B, nbands=nbands, T=T, tkind=tkind, xkind=xkind, n_valid=n_valid, acc0=acc0, seed=seed)


def _cases():
    rows = []
    for B in (1, 3, 64, 65, 130):
        for nb in (1, 7, 10, 64):
            rows.append(_case(f"B{B}-nb{nb}-random", B, nb, acc0="zero" if B % 2 else "nonzero"))
        rows.append(_case(f"B{B}-T3-nb3", B, 3, T=3))
    for nb in (7, 10, 64):
        rows.append(_case(f"edges-nb{nb}", 2 * nb + 4, nb, tkind="edges"))
        rows.append(_case(f"edges-nb{nb}-nonzero", 130, nb, tkind="edges", acc0="nonzero"))
    rows.append(_case("one-band", 65, 10, tkind="one"))
    for B in (3, 65):
        for nv in (0, 1, B, B + 5):
            rows.append(_case(f"B{B}-nvalid{nv}", B, 10, n_valid=nv, acc0="nonzero"))
        rows.append(_case(f"B{B}-nvalid-negative", B, 10, n_valid=-2, acc0="nonzero"))
    rows.append(_case("big-among-ones", 130, 10, tkind="one", xkind="big"))
    rows.append(_case("big-among-ones-random-t", 65, 7, xkind="big"))
    rows.append(_case("nan-and-inf", 64, 10, tkind="edges", xkind="nonfinite", acc0="nonzero"))
    rows.append(_case("nan-and-inf-3", 3, 7, tkind="edges", xkind="nonfinite"))
    # more samples than one staging chunk of the kernel (1024): one over, and several chunks with a ragged tail
    rows.append(_case("B1025", 1025, 10, acc0="nonzero"))
    rows.append(_case("B2500-nvalid2049", 2500, 64, n_valid=2049))
    for i, r in enumerate(rows):
        r["seed"] = 100 + i
    return rows


CASES = _cases()
CASE = {c["name"]: c for c in CASES}


def make_ops(c):
    """(x fp32 [B], t int64 [B], acc0 fp64 [nbands + 1][3]) of a case, on the CPU; the same on every call."""
    g = torch.Generator().manual_seed(c["seed"])
    B, T, nb = c["B"], c["T"], c["nbands"]
    if c["tkind"] == "random":
        t = torch.randint(0, T, (B,), generator=g)
    elif c["tkind"] == "edges":
        e = edge_timesteps(T, nb)
        t = torch.tensor([e[i % len(e)] for i in range(B)])
    else:
        t = torch.full((B,), 150 % T)
    if c["xkind"] == "spread":
        # losses over eight decades: the fp64 sums of squares round, so the order of the additions shows in the bits
        x = torch.exp(torch.rand(B, generator=g, dtype=torch.float64) * 18.4 - 13.8).float()
    elif c["xkind"] == "big":
        x = torch.ones(B)
        x[B // 2] = 1e8                        # fp32 accumulation would drop every 1 after it
    else:
        x = torch.rand(B, generator=g) + 0.5
        x[0] = float("nan")                    # t = 0 in the edge list: band 0
        x[B - 1] = float("inf")
    if c["acc0"] == "zero":
        acc0 = torch.zeros(nb + 1, 3, dtype=torch.float64)
    else:
        acc0 = torch.rand(nb + 1, 3, generator=g, dtype=torch.float64) * 100.0 + 1.0 / 3.0
        acc0[:, 0] = torch.floor(acc0[:, 0])   # counts are whole numbers
    return x, t.long(), acc0


def run(fn, c, **kw):
    """fn (ref_bands / model_bands) on a case's operands -> fp64 tensor [nbands + 1][3]."""
    x, t, acc0 = make_ops(c)
    rows = fn(x.double().tolist(), t.tolist(), c["T"], c["nbands"], c["n_valid"], acc0.tolist(), **kw)
    return torch.tensor(rows, dtype=torch.float64)


_REF = {}


def reference(name):
    """The reference table of a case, computed once and shared (read-only) by the tests."""
    if name not in _REF:
        _REF[name] = run(ref_bands, CASE[name])
    return _REF[name]


def canon(tab):
    """int64 bit patterns with every NaN mapped to one pattern (module docstring)."""
    tab = tab.detach().to("cpu", torch.float64).contiguous()
    bits = tab.view(torch.int64).clone()
    bits[torch.isnan(tab)] = 0x7FF8000000000000
    return bits


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(canon(a), canon(b)))
