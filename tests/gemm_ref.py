"""Reference model and checks of the cl_gemm conformance suite (helpers only: nothing here is collected).

`gemm_ref64` evaluates the documented contract of cl_gemm_params (include/ctrlora_hip.h) in fp64 on the operands the kernel
reads:

    out = act(a1 . w1^T + a2 . w2^T + bias + rowbias[m // rows_per_batch]) * alpha + beta * residual      (+ C, atomic)

Every launch of the suite gets the same four checks (tests/test_gpu_gemm_conformance.py; tests/test_gemm_reference_model.py
shows on the CPU that each of them bites):

  1. rel-L2 against the project's gates: TOL_ONE_ROUNDING for a bf16 output of exact operands, the fp32 gate (TOL_F32, or
     twice the error of torch's own fp32 evaluation of the same expression where that is larger) for fp32 outputs;
  2. element-wise, zero violations:   |got - ref| <= u_out |ref| + 2 K_total 2^-24 mag
     mag = the same expression with every operand replaced by its absolute value, K_total = the number of accumulated
     terms (taps * K1 + K2 + the epilogue's own roundings), u_out = 2^-8 for a bf16 output (half an ulp), 0 for fp32.
     Derived, not measured: a length-K fp32 sum in ANY order is within K 2^-24 sum|terms| of the exact sum to first order
     (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4); the factor 2 covers the higher-order terms and the
     order the MFMA chain, the split-K slabs and the epilogue happen to use.  An activation multiplies the second term by
     its Lipschitz factor (1.1 for SiLU and GELU); the GEGLU product value * gelu(gate) follows the product rule:
     |gelu(g)| mag_value + 1.1 mag_gate (|value| + second-order term);
  3. canary: the output is a view into a larger buffer (ldc = N + 8, 64 guard rows either side) pre-filled with a fixed
     non-NaN bit pattern, NaN inside the view; afterwards every guard row and pad column is bit-identical and no NaN is left;
  4. (GPU only) exactly one launch of the intended signature in the launch-tag table.

The two forms only the x-stationary kernel has (csrc/gemm_xs.hip) widen the bound of check 2 by terms that
are derived here, never measured:

  * act = ACT_GEGLU_SPLIT (3): h = a1 w1^T [+ a2 w2^T] + bias, out[M, N / 2] = h[:, :N / 2] gelu_exact(h[:, N / 2:]).  The product
    rule above, plus |value| |dgelu(gate)| for the kernel's Abramowitz-Stegun erfc (`dgelu_as`);
  * ln = (gamma, beta, eps): xn = bf16_rne((x - mean) rstd gamma + beta) with fp64 statistics over the K1 stored values, then the
    product on xn.  The kernel rounds xn from an fp32 value, so an element whose fp64 value lies within the fp32 error bound of
    a bf16 tie (tests/norm_ref.py: fixed_y + C_STAT["ln"] stat_y) may round the other way: such elements are `ambiguous` and widen
    the bound by |alpha| sum_k amb[m, k] ulp_bf16(xn[m, k]) |w[n, k]| (through the GEGLU product rule for act 3).  They are never
    skipped.  `ln_parts` records the share of rows that carry a widening; tests/xs_ref.py draws inputs that keep it <= 2 %.
"""
import math

import torch

# one bf16 rounding of the result (2^-9 = 1.95e-3 worst, ~1.7e-3 rms): test_grouped_lora_products_vs_fp64
TOL_ONE_ROUNDING = 2.5e-3
# fp32-accumulated products of exact operands: test_grouped_weight_gradient_production_stage
TOL_F32 = 2e-5

LINEAR, CONV_S1, CONV_S2, CONV_UP2, CONV_T2, CONV_S2A = 0, 1, 2, 3, 4, 5
ACT_NONE, ACT_SILU, ACT_GEGLU, ACT_GEGLU_SPLIT = 0, 1, 2, 3
LIP_SILU, LIP_GELU = 1.1, 1.1
GUARD_ROWS, PAD_COLS = 64, 8
# leading-dimension pads of the operands: all different from the output's, whole 128-byte lines in both dtypes
PAD_A1, PAD_A2, PAD_RES, PAD_RB = 64, 128, 24, 40
PAD_FILL = 1.0e3          # what a kernel reads if it walks an operand with another operand's leading dimension


class _tags:
    """Launch tags (csrc/debug_hooks.h: cl_debug_gemm_tag) on, from an empty table, for the length of a `with` block."""

    def __enter__(self):
        from ctrlora_amd import hip
        L = hip.lib()
        assert L.cl_debug_gemm_tag_clear() == 0 and L.cl_debug_gemm_tag(1) == 0
        return self

    def __exit__(self, *exc):
        from ctrlora_amd import hip
        hip.lib().cl_debug_gemm_tag(0)
        return False

    @staticmethod
    def restart():
        from ctrlora_amd import hip
        assert hip.lib().cl_debug_gemm_tag_clear() == 0

    @staticmethod
    def launches(**sig):
        """(launches of the signatures that match, signatures in the table: 255 = the table is full and says nothing)."""
        from ctrlora_amd import hip
        tags = hip.gemm_tags()
        return sum(t["launches"] for t in tags if all(t[k] == v for k, v in sig.items())), len(tags)


def _rel(a, b):
    """tests.util.rel_l2 without the trip to the host (operands of 32768 x 2560 in fp64)."""
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _f32_gate(got, ref64, a, b):
    """(error, gate, error of torch's own fp32 product) for an fp32-accumulated product a @ b of exact operands: TOL_F32, or twice
    the error of torch.matmul in fp32 on the same operands against the same fp64 reference where THAT is larger (the order of
    32768 fp32 additions is not the kernel's to be blamed for)."""
    e = _rel(got, ref64)
    e_torch = _rel(a.float() @ b.float(), a.double() @ b.double())
    return e, max(TOL_F32, 2 * e_torch), e_torch


# ------------------------------------------------------------------------------------------------ the case

def make_case(a1, w1, *, a2=None, w2=None, bias=None, rowbias=None, rows_per_batch=0, residual=None, alpha=1.0, beta=0.0,
              act=ACT_NONE, mode=LINEAR, conv=None, a1_group_n=0, a2_group_n=0, alpha_n=0, out_f32=False, atomic=False,
              splitk=1, c0=None, N=None, ln=None):
    """One cl_gemm call as plain data.  a1: [M, K1] (linear; [M, G K1] with a1_group_n) or NHWC pixels [B Hin Win, K1] (conv modes,
    conv = (B, Hin, Win, Hout, Wout)); w1: [N, taps K1]; c0: the value C holds before an atomic launch; ln = (gamma [K1], beta [K1],
    eps): a1 holds the un-normalised rows (LayerNorm prologue)."""
    c = dict(a1=a1, w1=w1, a2=a2, w2=w2, bias=bias, rowbias=rowbias, rows_per_batch=rows_per_batch, residual=residual,
             alpha=float(alpha), beta=float(beta), act=act, mode=mode, conv=conv, a1_group_n=a1_group_n, a2_group_n=a2_group_n,
             alpha_n=alpha_n, out_f32=bool(out_f32), atomic=bool(atomic), splitk=splitk, c0=c0, ln=ln)
    c["N"] = w1.shape[0] if N is None else N
    taps = 1 if mode == LINEAR else 9
    c["K1"] = w1.shape[1] // taps
    c["K2"] = 0 if w2 is None else w2.shape[1]
    c["M"] = a1.shape[0] if mode == LINEAR else conv[0] * conv[3] * conv[4]
    c["dtype"] = a1.dtype
    c["out_cols"] = c["N"] // 2 if act in (ACT_GEGLU, ACT_GEGLU_SPLIT) else c["N"]
    c["out_dtype"] = torch.float32 if (out_f32 or atomic) else a1.dtype
    return c


def k_total(c):
    """Accumulated terms of one output element: the K of both segments plus one per rounding the epilogue adds."""
    epi = sum(1 for k in ("bias", "rowbias", "residual") if c[k] is not None) + (c["alpha"] != 1.0) + (c["beta"] not in (0.0, 1.0))
    epi += {ACT_NONE: 0, ACT_SILU: 3, ACT_GEGLU: 6, ACT_GEGLU_SPLIT: 6}[c["act"]]         # exp / erf, the sum and the quotient / products
    if c["atomic"]:
        epi += max(1, c["splitk"])                                  # one fp32 add onto C per split
    return (1 if c["mode"] == LINEAR else 9) * c["K1"] + c["K2"] + epi


def row_chunks(c, budget=1 << 25):
    """Row ranges [lo, hi) that tile [0, M) -- every row, none twice -- small enough for fp64 on the device: whole samples
    in the conv modes (a chunk is then a conv2d over a few images)."""
    M, width = c["M"], max(c["N"], (1 if c["mode"] == LINEAR else 9) * c["K1"] + c["K2"], 1)
    rows = max(256, budget // width)
    if c["mode"] != LINEAR:
        per = c["conv"][3] * c["conv"][4]
        rows = max(1, rows // per) * per
    return [(lo, min(M, lo + rows)) for lo in range(0, M, rows)]


def _conv64(c, a1, w, lo, hi, F):
    """3x3 products of the header's conv modes on samples [lo, hi) / (Hout Wout): a1 NHWC pixels, w [N, (ky, kx, c)]."""
    B, Hin, Win, Hout, Wout = c["conv"]
    K1, N, mode = c["K1"], w.shape[0], c["mode"]
    b0, b1 = lo // (Hout * Wout), hi // (Hout * Wout)
    img = a1.reshape(b1 - b0, Hin, Win, K1).permute(0, 3, 1, 2)          # (a1: the pixels of samples [b0, b1) only)
    w4 = w.reshape(N, 3, 3, K1).permute(0, 3, 1, 2)
    if mode == CONV_S1:
        y = F.conv2d(img, w4, padding=1)
    elif mode == CONV_S2:
        y = F.conv2d(img, w4, stride=2, padding=1)
    elif mode == CONV_UP2:
        y = F.conv2d(F.interpolate(img, scale_factor=2, mode="nearest"), w4, padding=1)
    elif mode == CONV_T2:          # zero-stuffed x2 grid: source pixel (y, x) sits at (2y, 2x), zeros elsewhere
        z = torch.zeros(b1 - b0, K1, Hout, Wout, dtype=img.dtype, device=img.device)
        z[:, :, ::2, ::2] = img
        y = F.conv2d(z, w4, padding=1)
    elif mode == CONV_S2A:         # AutoencoderKL's Downsample: one zero column on the right, one zero row at the bottom, no pad top / left
        y = F.conv2d(F.pad(img, (0, 1, 0, 1)), w4, stride=2)
    else:
        raise ValueError(mode)
    assert tuple(y.shape[2:]) == (Hout, Wout), (tuple(y.shape), c["conv"])
    return y.permute(0, 2, 3, 1).reshape(hi - lo, N)


def ulp_bf16(v):
    """Spacing of the bf16 grid at |v| (fp64 tensor; 0 at v = 0): 2^(floor(log2 |v|) - 7)."""
    _, e = torch.frexp(v)
    return torch.where(v != 0, torch.ldexp(torch.ones_like(v), e - 8), torch.zeros_like(v))


def ln_parts(c):
    """The LayerNorm prologue of a case in fp64 (cached in the case): xn = bf16_rne(y) as double, amb_ulp = ulp_bf16(xn) where y
    lies within its fp32 error bound of a bf16 tie and 0 elsewhere, mean / rstd with the parts of their gates (norm_ref),
    amb_rows = the share of rows with an ambiguous element."""
    if "_ln" not in c:
        from tests import norm_ref as NR
        gamma, beta, eps = c["ln"]
        case = dict(family="ln", M=c["M"], D=c["K1"], silu=False, eps=eps, x=c["a1"], gamma=gamma, beta=beta)
        r = NR.norm_ref64(case, backward=False, bounds=True)
        y = r["y"]
        xn = y.to(torch.bfloat16).double()
        e32 = r["fixed_y"] + NR.C_STAT["ln"] * r["stat_y"]          # what a correct fp32 evaluation may be off by
        u = ulp_bf16(y)
        frac = (y.abs() / u.clamp_min(1e-300)) % 1.0
        dist = (frac - 0.5).abs() * u                                # to the nearest midpoint of two bf16 neighbours
        amb = (dist <= e32) & (y != 0)
        c["_ln"] = dict(xn=xn, amb_ulp=torch.where(amb, ulp_bf16(xn), torch.zeros_like(xn)), mean=r["mean"], rstd=r["rstd"],
                        stat_mean=r["stat_mean"], stat_rstd=r["stat_rstd"], amb_rows=float(amb.any(1).double().mean()),
                        amb_elems=int(amb.sum()))
    return c["_ln"]


# gelu_as (csrc/gemm_xs.hip), to first order in e = 2^-24 from the code:
#   z = |g| 0.7071..                       one rounding (the constant's own is below it): relative e
#   t = rcp(fma(0.3275911, z, 1))          one rounding of the fma, the hardware reciprocal to 1 ulp = 2 e, and the error of z carried
#                                          through (0.3275911 z t <= 1): relative 4 e in all
#   P = ((((a5 t + a4) t + a3) t + a2) t + a1) t     four fma and one product: each rounds a partial sum that is at most
#                                          S(t) = sum |a_i| t^i (the signs alternate), 5 e S(t); the error of t enters as
#                                          |P'(t)| t 4 e <= 4 e S1(t), S1 = sum i |a_i| t^i
#   E = exp2(-1.4427 z z)                  two products for the argument a = z^2 log2 e (2 e a), the error of z twice (2 e a) and
#                                          the constant's rounding (e a / 2): |dE| / E = ln 2 . 4.5 e a = 4.5 e z^2; exp2 itself 1 ulp = 2 e
#   c = P E  (one rounding)  ~ erfc(z)     A&S 7.1.26: |P E - erfc z| <= 1.5e-7 in exact arithmetic
#   gelu = 0.5 g (c or 2 - c)              2 - c and the product: 2 e |gelu|
_AS = (0.254829592, 0.284496736, 1.421413741, 1.453152027, 1.061405429)     # |a_1| .. |a_5|


def dgelu_as(g):
    """|gelu_as(g) - gelu(g)| at most, first order (fp64 tensor in, fp64 tensor out)."""
    e = 2.0 ** -24
    z = g.abs() * (0.5 ** 0.5)
    t = 1.0 / (1.0 + 0.3275911 * z)
    S = sum(a * t ** (i + 1) for i, a in enumerate(_AS))
    S1 = sum((i + 1) * a * t ** (i + 1) for i, a in enumerate(_AS))
    Ex = torch.exp(-z * z)
    cc = torch.erfc(z)
    dc = 1.5e-7 + e * ((5 * S + 4 * S1) * Ex + cc * (4.5 * z * z + 2 + 1))
    gel = 0.5 * g * (1.0 + torch.erf(g * (0.5 ** 0.5)))
    return 0.5 * g.abs() * dc + 2 * e * gel.abs()


def _grouped(a, w, group_n, K):
    """Output columns [g group_n, (g + 1) group_n) read columns [g K, (g + 1) K) of a."""
    G = w.shape[0] // group_n
    return torch.cat([a[:, g * K:(g + 1) * K] @ w[g * group_n:(g + 1) * group_n].t() for g in range(G)], 1)


def gemm_ref64(c, lo=0, hi=None, absolute=False, kappa=0.0, dtype=torch.float64):
    """Rows [lo, hi) of the contract in `dtype` (fp64: the reference; fp32: torch's own evaluation for the fp32 gate).
    absolute = True: the magnitude `mag` of check 2 -- every operand replaced by its absolute value, the activation by its
    Lipschitz bound around the reference (kappa = 2 K_total 2^-24 enters the second-order term of the GEGLU product)."""
    F = torch.nn.functional
    hi = c["M"] if hi is None else hi
    cv = lambda t: None if t is None else t.to(dtype)
    ab = (lambda t: t.abs()) if absolute else (lambda t: t)

    def pre(ab):
        w1 = ab(cv(c["w1"]))[:c["N"]]
        if c["mode"] != LINEAR:
            B, Hin, Win, Hout, Wout = c["conv"]
            assert lo % (Hout * Wout) == 0 and hi % (Hout * Wout) == 0, "conv modes: whole samples"
            a1 = ab(cv(c["a1"][lo // (Hout * Wout) * Hin * Win:hi // (Hout * Wout) * Hin * Win]))
            s = _conv64(c, a1, w1, lo, hi, F)
        elif c["a1_group_n"]:
            s = _grouped(ab(cv(c["a1"][lo:hi])), w1, c["a1_group_n"], c["K1"])
        elif c["ln"] is not None:
            s = ab(ln_parts(c)["xn"][lo:hi].to(dtype)) @ w1.t()
        else:
            s = ab(cv(c["a1"][lo:hi])) @ w1.t()
        if c["a2"] is not None:
            a2, w2 = ab(cv(c["a2"][lo:hi])), ab(cv(c["w2"]))
            s = s + (_grouped(a2, w2, c["a2_group_n"], c["K2"]) if c["a2_group_n"] else a2 @ w2.t())
        if c["bias"] is not None:
            s = s + ab(cv(c["bias"]))
        if c["rowbias"] is not None:
            idx = torch.arange(lo, hi, device=s.device) // c["rows_per_batch"]
            s = s + ab(cv(c["rowbias"])).index_select(0, idx)
        return s

    s = pre(lambda t: t)
    if c["act"] == ACT_SILU:
        v = s * torch.sigmoid(s)
    elif c["act"] == ACT_GEGLU:
        # packing.LinearW.geglu_pack: every 160-column tile = 80 value columns then their 80 gate columns; C is [M, N / 2]
        t = s.reshape(hi - lo, c["N"] // 160, 2, 80)
        val, gate = t[:, :, 0].reshape(hi - lo, -1), t[:, :, 1].reshape(hi - lo, -1)
        gel = 0.5 * gate * (1.0 + torch.erf(gate * (0.5 ** 0.5)))
        v = val * gel
    elif c["act"] == ACT_GEGLU_SPLIT:
        # natural row order, as nn.Linear(dim, 2 inner) holds them: [value | gate]
        val, gate = s[:, :c["N"] // 2], s[:, c["N"] // 2:]
        gel = 0.5 * gate * (1.0 + torch.erf(gate * (0.5 ** 0.5)))
        v = val * gel
    else:
        v = s
    if absolute:
        m = pre(ab)
        if c["act"] == ACT_SILU:
            v = LIP_SILU * m
        elif c["act"] == ACT_GEGLU:
            t = m.reshape(hi - lo, c["N"] // 160, 2, 80)
            mv, mg = t[:, :, 0].reshape(hi - lo, -1), t[:, :, 1].reshape(hi - lo, -1)
            v = gel.abs() * mv + LIP_GELU * mg * (val.abs() + kappa * mv)
        elif c["act"] == ACT_GEGLU_SPLIT:
            mv, mg = m[:, :c["N"] // 2], m[:, c["N"] // 2:]
            v = gel.abs() * mv + LIP_GELU * mg * (val.abs() + kappa * mv)
        else:
            v = m
    if c["alpha"] != 1.0:
        al = abs(c["alpha"]) if absolute else c["alpha"]
        if c["alpha_n"]:
            v = torch.cat([v[:, :c["alpha_n"]] * al, v[:, c["alpha_n"]:]], 1)
        else:
            v = v * al
    if c["residual"] is not None and c["beta"] != 0.0:
        v = v + (abs(c["beta"]) if absolute else c["beta"]) * ab(cv(c["residual"])[lo:hi])
    if c["atomic"] and c["c0"] is not None:
        v = v + (abs(c["c0"]) if absolute else c["c0"])
    return v


def xs_extra(c, lo=0, hi=None):
    """The additive part of the element-wise bound that the x-stationary-only forms need (module docstring), rows [lo, hi):
    None for every other case."""
    if c["ln"] is None and c["act"] != ACT_GEGLU_SPLIT:
        return None
    hi = c["M"] if hi is None else hi
    half = c["N"] // 2
    wid = None
    if c["ln"] is not None:
        wid = ln_parts(c)["amb_ulp"][lo:hi] @ c["w1"].double()[:c["N"]].abs().t()
    if c["act"] == ACT_GEGLU_SPLIT:
        s = gemm_ref64(dict(c, act=ACT_NONE, alpha=1.0, residual=None), lo, hi)          # h, before the activation
        val, gate = s[:, :half], s[:, half:]
        gel = 0.5 * gate * (1.0 + torch.erf(gate * (0.5 ** 0.5)))
        ex = val.abs() * dgelu_as(gate)
        if wid is not None:
            wv, wg = wid[:, :half], wid[:, half:]
            ex = ex + gel.abs() * wv + LIP_GELU * wg * (val.abs() + wv)
        return ex
    al = abs(c["alpha"])
    if c["alpha"] != 1.0 and c["alpha_n"]:
        return torch.cat([wid[:, :c["alpha_n"]] * al, wid[:, c["alpha_n"]:]], 1)
    return wid * al


# ------------------------------------------------------------------------------------------------ canary buffers

def _pattern(dtype):
    """(int dtype of the same width, the fixed bit pattern): finite in both formats (bf16 0x5A5A ~ 1.5e16, fp32 ~ 1.5e16)."""
    return (torch.int16, 0x5A5A) if dtype == torch.bfloat16 else (torch.int32, 0x5A5A5A5A)


class Guarded:
    """An [M, cols] output as a view into a [M + 2 GUARD_ROWS, cols + PAD_COLS j] buffer: guard rows and pad columns hold a fixed
    non-NaN bit pattern, the view NaN (= not written) or `fill` (atomic accumulation)."""

    def __init__(self, M, cols, dtype, device, fill=float("nan"), j=1):
        self.M, self.cols, self.ld = M, cols, cols + PAD_COLS * j
        it, pat = _pattern(dtype)
        self.buf = torch.full((M + 2 * GUARD_ROWS, self.ld), pat, dtype=it, device=device).view(dtype)
        self.view = self.buf[GUARD_ROWS:GUARD_ROWS + M, :cols]
        self.view.fill_(fill)

    def check(self):
        """(guard rows that changed, pad-column elements that changed, NaNs left inside the view)."""
        it, pat = _pattern(self.buf.dtype)
        bits = self.buf.view(it)
        g = GUARD_ROWS
        rows = int((bits[:g] != pat).any(1).sum()) + int((bits[g + self.M:] != pat).any(1).sum())
        pads = int((bits[g:g + self.M, self.cols:] != pat).sum())
        return dict(guard_rows=rows, pad_elems=pads, nan_left=int(torch.isnan(self.view).sum()))


def padded(t, pad, fill=PAD_FILL):
    """A copy of the 2-D tensor t as a view with leading dimension t.shape[1] + pad; the pad holds PAD_FILL (or `fill`: NaN for
    a kernel that reads the operand through whole vectors inside its width only, so that no pad value may reach an output)."""
    if t is None:
        return None
    buf = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


# ------------------------------------------------------------------------------------------------ the checks

def run_checks(c, got, guard=None, budget=1 << 25):
    """Checks 1 - 3 of one launch: a dict of figures (nothing asserted here).  `got` is the [M, out_cols] result."""
    M = c["M"]
    bf16_out = c["out_dtype"] == torch.bfloat16
    u_out = 2.0 ** -8 if bf16_out else 0.0
    kt = k_total(c)
    kappa = 2.0 * kt * 2.0 ** -24
    se = sr = 0.0
    viol, worst, first = 0, 0.0, None
    for lo, hi in row_chunks(c, budget):
        ref = gemm_ref64(c, lo, hi)
        mag = gemm_ref64(c, lo, hi, absolute=True, kappa=kappa)
        g = got[lo:hi].double()
        err = (g - ref).abs()
        se += float((err * err).nan_to_num(nan=0.0).sum())
        sr += float((ref * ref).sum())
        bound = u_out * ref.abs() + kappa * mag
        extra = xs_extra(c, lo, hi)
        if extra is not None:
            bound = bound + extra
        bad = ~(err <= bound)                                  # a NaN in `got` is a violation
        ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0)).nan_to_num(nan=math.inf)
        n = int(bad.sum())
        if n and first is None:
            i = bad.nonzero()[0].tolist()
            first = dict(row=lo + i[0], col=i[1], got=float(g[i[0], i[1]]), ref=float(ref[i[0], i[1]]), bound=float(bound[i[0], i[1]]),
                         rows_hit=int(bad.any(1).sum()))
        viol += n
        worst = max(worst, float(ratio.max()))
    rel = math.sqrt(se) / (math.sqrt(sr) + 1e-30)
    out = dict(rel=rel, gate=TOL_ONE_ROUNDING if bf16_out else TOL_F32, torch_f32=None, violations=viol, err_over_bound=worst,
               first_violation=first, k_total=kt)
    if c["ln"] is not None:
        out["amb_rows"] = ln_parts(c)["amb_rows"]
    if not bf16_out and not rel < out["gate"]:
        # the fp32 gate: twice what torch's own fp32 evaluation of the same expression loses, where that is larger
        s2 = sr2 = 0.0
        for lo, hi in row_chunks(c, budget):
            ref = gemm_ref64(c, lo, hi)
            d = gemm_ref64(c, lo, hi, dtype=torch.float32).double() - ref
            s2 += float((d * d).sum())
            sr2 += float((ref * ref).sum())
        out["torch_f32"] = math.sqrt(s2) / (math.sqrt(sr2) + 1e-30)
        out["gate"] = max(TOL_F32, 2 * out["torch_f32"])
    if guard is not None:
        out.update(guard.check())
    return out


def failures(res):
    """Names of the checks a run_checks() result fails (empty = all of 1 - 3 hold)."""
    bad = []
    if not res["rel"] < res["gate"]:
        bad.append("rel_l2")
    if res["violations"]:
        bad.append("elementwise")
    if res.get("guard_rows") or res.get("pad_elems") or res.get("nan_left"):
        bad.append("canary")
    return bad
