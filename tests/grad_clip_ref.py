"""fp64 model of the device-side gradient norm and clip (cl_grad_norm, cl_adamw_dev_clip; include/ctrlora_hip.h) and its case table.

Contract, on the fp32 operands as stored:

    norm = fl32( (double) grad_scale * sqrt( sum over all buffers, sum_i (double) g_i * (double) g_i ) )
    coef = 1.0f                                        when max_norm is None or <= 0 (tracking only)
         = c < 1 ? c : (c != c ? c : 1.0f),  c = fl32(max_norm / fl32(norm + 1e-6f))      otherwise (torch.clamp(c, max=1.0))
    AdamW on g_i * fl32(grad_scale * coef)             (torch.optim.AdamW; tests/ew_ref.eval_adamw_step)

Gates (the GPU suite applies the same ones to the kernels, tests/test_gpu_grad_clip.py):
  * norm within 2 fp32 ulp of the fp64 value rounded to fp32: an fp64 sum of n non-negative terms carries a relative error below
    n 2^-53 in any order (2^-31 for the 2^22 elements of the largest row here; the square root halves it), far below an fp32
    ulp's 2^-24; the square root and the final rounding cost at most one ulp each.  A non-finite reference must be met exactly
    (NaN by NaN, inf by inf);
  * coef bit-equal to the fp32 formula applied to the norm that was actually produced;
  * the AdamW outputs inside the element-wise bound of tests/ew_ref.py's adamw family, evaluated with the effective scale
    fl32(grad_scale * coef) in place of grad_scale.

`model(row, bufs, mutant=...)` restates the contract; the mutants are the mistakes the gates must catch
(tests/test_grad_clip_reference_model.py)."""
import math

import numpy as np
import torch

from tests import ew_ref as R

F32 = torch.float32
BIG = (1 << 20) + 5                     # every workgroup of the partial launch takes more than one grid-stride trip
COUNTS = (0, 1, 7, 257, 4099, BIG)
UNROLL = 3 * (1 << 20) + 13             # long enough for the four-loads-in-flight loop of the partial kernel, plus a remainder
GUARD = 64                              # floats before and after every buffer (a multiple of 4: the view keeps the alignment)
GUARD_FILL = 1e30                       # one guard element in the sum would show at once
MAX_BUFS = 16
MUTANTS = ("drop_last_buffer", "drop_tail", "no_grad_scale", "coef_on_m_only", "fminf")


def _row(name, counts, scale=1.0, max_norm=None, shift=0, span=False, plant=None):
    return dict(name=name, counts=tuple(counts), scale=scale, max_norm=max_norm, shift=shift, span=span, plant=plant)


def _cases():
    rows = [_row(f"one-{n}", (n,), max_norm=(None, 0.0, 0.5, 1e6)[i % 4]) for i, n in enumerate(COUNTS)]
    rows.append(_row("one-big-scale8", (BIG,), scale=1.0 / 8, max_norm=1.0))
    rows.append(_row("one-4099-scale8-track", (4099,), scale=1.0 / 8))
    rows.append(_row("three-a", (7, 0, 4099), max_norm=2.0))
    rows.append(_row("three-b-scale8", (257, BIG, 1), scale=1.0 / 8, max_norm=3.0))
    rows.append(_row("three-last-only", (0, 0, 257), max_norm=1.0))
    rows.append(_row("sixteen", (0, 1, 7, 257, 4099) * 3 + (BIG,), max_norm=5.0))
    rows.append(_row("sixteen-scale8", (4099, 257, 7, 1) * 4, scale=1.0 / 8, max_norm=0.25))
    for shift in (1, 2, 3):             # a view that starts 4 / 8 / 12 bytes past a 16-byte boundary: scalar head, then vectors
        rows.append(_row(f"shift{shift}", (4099, 7, 257), shift=shift, max_norm=1.0))
    rows.append(_row("shift1-short", (2, 3, 1), shift=1, max_norm=0.1))            # shorter than the head: no vector at all
    rows.append(_row("span-1e25", (4099,), span=True, max_norm=1.0))              # fp32 squares would underflow and overflow
    rows.append(_row("span-1e25-three", (257, 4099, 7), span=True, shift=1))
    rows.append(_row("nan", (4099,), max_norm=1.0, plant=("nan", 1234)))
    rows.append(_row("inf", (4099, 7), max_norm=1.0, plant=("inf", 4000)))
    rows.append(_row("unrolled", (UNROLL,), max_norm=100.0))
    return rows


CASES = _cases()
ROW = {r["name"]: r for r in CASES}
# every count the issue lists appears, with 1, 3 and 16 buffers
assert {n for r in CASES for n in r["counts"]} >= set(COUNTS) and {len(r["counts"]) for r in CASES} >= {1, 3, MAX_BUFS}


def make_bufs(row, device="cpu"):
    """[(backing tensor with guards, view the kernel is handed)] for a row; the same numbers on every device."""
    g = torch.Generator().manual_seed(1000 + CASES.index(row))
    out = []
    for b, n in enumerate(row["counts"]):
        if row["span"]:
            vals = torch.pow(10.0, torch.rand(n, generator=g, dtype=torch.float64) * 50 - 25).float()
            vals = vals * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)
        else:
            vals = torch.randn(n, generator=g) * (0.5 + b)
        if row["plant"] is not None and b == 0:
            vals[row["plant"][1]] = float(row["plant"][0])
        back = torch.full((GUARD + row["shift"] + n + GUARD,), GUARD_FILL, dtype=F32)
        back[GUARD + row["shift"]:GUARD + row["shift"] + n] = vals
        back = back.to(device)
        out.append((back, back[GUARD + row["shift"]:GUARD + row["shift"] + n]))
    return out


def guards_intact(back, view):
    lo = (view.data_ptr() - back.data_ptr()) // 4 if view.numel() else None
    if lo is None:
        return bool((back == GUARD_FILL).all())
    return bool((back[:lo] == GUARD_FILL).all()) and bool((back[lo + view.numel():] == GUARD_FILL).all())


def f32(x):
    return np.float32(x)


def coef32(norm32, max_norm, fminf=False):
    """The fp32 clip coefficient for an fp32 norm (a numpy float32), as a numpy float32."""
    if max_norm is None or float(max_norm) <= 0.0:
        return f32(1.0)
    with np.errstate(all="ignore"):
        c = f32(max_norm) / (f32(norm32) + f32(1e-6))
    if fminf:
        return f32(1.0) if not c < f32(1.0) else c            # fminf(1, c): the NaN is lost
    return c if c < f32(1.0) else (c if c != c else f32(1.0))


def norm64(views, scale, mutant=None):
    """(double) fl32(scale) * sqrt(sum g^2) in fp64 as a python float."""
    if mutant == "drop_last_buffer":
        views = views[:-1]
    s = 0.0
    for v in views:
        v = v.detach().cpu()
        if mutant == "drop_tail":
            # what a kernel that forgets the elements after the last full 16-byte vector would read (the head is whatever comes
            # before the first 16-byte boundary; these views are backed by 16-byte aligned storage + GUARD + shift floats)
            head = min(v.numel(), (-(v.storage_offset() % 4)) % 4)
            v = v[:head + (v.numel() - head) // 4 * 4]
        s += float((v.double() * v.double()).sum())
    gs = 1.0 if mutant == "no_grad_scale" else float(f32(scale))
    return gs * math.sqrt(s) if s == s else float("nan")


def ulp32(x):
    return float(np.spacing(np.abs(f32(x))))


def norm_flag(got32, ref64):
    """None when the fp32 norm `got32` meets the fp64 reference, else what is wrong."""
    got, ref = float(got32), float(f32(ref64))
    if ref != ref or math.isinf(ref):
        return None if (got != got if ref != ref else got == ref) else f"norm {got} where the reference is {ref}"
    if not abs(got - ref) <= 2 * ulp32(ref):
        return f"norm {got!r} is {abs(got - ref) / ulp32(ref):.1f} ulp from {ref!r}"
    return None


def coef_flag(got_coef, got_norm, max_norm):
    want = coef32(f32(got_norm), max_norm)
    same = np.array(got_coef, dtype=np.float32).view(np.uint32) == np.array(want, dtype=np.float32).view(np.uint32)
    if want != want:
        same = got_coef != got_coef                       # any NaN: the payload is not part of the contract
    return None if bool(same) else f"coef {float(got_coef)!r} where the fp32 formula gives {float(want)!r} for norm {float(got_norm)!r}"


# ------------------------------------------------------------------------------------------------ AdamW on the clipped gradient

ADAMW_N = (1, 255, 4099)


def adamw_ops(n, device="cpu"):
    g = torch.Generator().manual_seed(77 + n)
    ops = dict(p=torch.randn(n, generator=g) * 0.02, m=torch.randn(n, generator=g) * 1e-3,
               v=torch.rand(n, generator=g) * 1e-5, g=torch.randn(n, generator=g))
    return {k: t.to(device) for k, t in ops.items()}


def effective_scale(scale, coef):
    """fl32(grad_scale * coef): the two scalars are multiplied first."""
    return float(f32(scale) * f32(coef))


def adamw_specs(state, g, step, scale, coef):
    """tests/ew_ref.eval_adamw_step with fl32(scale * coef) in place of its grad_scale: the adamw_dev conformance row's bound,
    evaluated on the clipped gradient."""
    keep = R.ADAMW_HYPER["gscale"]
    R.ADAMW_HYPER["gscale"] = effective_scale(scale, coef)
    try:
        return R.eval_adamw_step(state, g, step)
    finally:
        R.ADAMW_HYPER["gscale"] = keep


def adamw_model(state, g, step, scale, coef, mutant=None):
    """fp64 AdamW step (p, m, v) on g * fl32(scale * coef), rounded to fp32 once; `coef_on_m_only` leaves coef out of v."""
    H = R.ADAMW_HYPER
    lr, b1, b2, eps, wd = (float(f32(H[k])) for k in ("lr", "beta1", "beta2", "eps", "wd"))
    p, m, v = (t.double() for t in state)
    gm = g.double() * effective_scale(scale, coef)
    gv = g.double() * float(f32(scale)) if mutant == "coef_on_m_only" else gm
    m1 = b1 * m + (1 - b1) * gm
    v1 = b2 * v + (1 - b2) * gv * gv
    p1 = p * (1 - lr * wd) - (lr / (1 - b1 ** step)) * m1 / (v1.sqrt() / math.sqrt(1 - b2 ** step) + eps)
    return p1.float(), m1.float(), v1.float()


def adamw_flags(got, specs):
    return R.failures(R.check(specs, dict(zip("pmv", got))))


# ------------------------------------------------------------------------------------------------ the whole model, with mutants

def model(row, views, mutant=None):
    """(norm as numpy float32, coef as numpy float32) the contract gives for a row -- or what a mutant would give."""
    with np.errstate(all="ignore"):
        n32 = f32(norm64(views, row["scale"], mutant))
    return n32, coef32(n32, row["max_norm"], fminf=mutant == "fminf")


def judge(row, views, got_norm, got_coef):
    """The flags of one (norm, coef) result for a row: [] when every gate holds."""
    flags = [norm_flag(got_norm, norm64(views, row["scale"])), coef_flag(got_coef, got_norm, row["max_norm"])]
    return [f for f in flags if f is not None]
