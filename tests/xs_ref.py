"""Launcher transcription, rounding model, gates and case table of the x-stationary conformance suite (helpers only: nothing
here is collected).  The contract itself -- act = ACT_GEGLU_SPLIT and the LayerNorm prologue in fp64, with the derived widenings
of the element-wise bound -- lives in tests/gemm_ref.py beside the rest of cl_gemm's; DESIGN.md section 1k.

  * `accepts` / `xs_form`: what launch_gemm (csrc/gemm.hip) and launch_gemm_xs / launch_xs (csrc/gemm_xs.hip) decide on the host
    for a call: refused, handed to the tile kernels, or launched by the x-stationary kernel as (instance, groups, bpg, nsplit,
    cpw, workgroups).  The CPU test holds it against the library on every refusal, the GPU suite against the launch-tag record.
  * `xs_model`: the kernel's arithmetic with the roundings its code has and no others, in the kernel's order: two-pass
    statistics split over the two half-rows a lane pair holds (k = 16 j + 8 hi .. + 7, `sum += lo + hi` four times per k-step),
    the partner added last, `rsqrt`, the affine map, one bf16 rounding, accumulators that start from the bias and take one
    16-deep MFMA step at a time (the 16 products of a step exact, one fp32 rounding per step), the epilogue in the kernel's
    order (alpha per 32-column block, beta * residual as one fma, gelu_as in fp32).  With `fault=` it is the same kernel with
    one of the mistakes this kernel can make (FAULTS): the negative controls of the CPU test.
  * the statistics gate is norm_ref's: |got - ref| <= e |ref| + c stat, stat_mean = e mean|x|, stat_rstd = e rstd (two-pass).  The
    kernel sums K1 / 2 values in ONE fp32 chain per lane, longer than any chain of cl_layernorm_fwd, so c is measured again on
    the model of THIS order: C_STAT_XS = MARGIN x MEASURED["stat"].  The output bound has no measured part.
  * CASES: the table of tests/test_gpu_gemm_xs_conformance.py, every row with the form it was written to reach.
"""
import math

import torch

from tests import gemm_ref as G
from tests.attn_ref import MARGIN

BF, F32 = torch.bfloat16, torch.float32
E = 2.0 ** -24
XS_PLAIN, XS_RES, XS_GEGLU = 0, 1, 2
EPI_NAME = {XS_PLAIN: "plain", XS_RES: "res", XS_GEGLU: "geglu"}
# (K1, K2) -> (KS1, KS2, RING, MINW): launch_xs_k / launch_xs_ln
K_FORMS = {(320, 0): (20, 0, 3, 2), (320, 128): (20, 8, 2, 2), (640, 0): (40, 0, 3, 1), (640, 128): (40, 8, 3, 1)}
# the 16 instantiations of gemm_xs_kernel: (K1, K2, epilogue, LayerNorm prologue)
INSTANCES = tuple((k1, k2, epi, False) for (k1, k2) in K_FORMS for epi in (XS_PLAIN, XS_RES, XS_GEGLU)) + \
    tuple((k1, 0, epi, True) for k1 in (320, 640) for epi in (XS_PLAIN, XS_GEGLU))

# Measured by measure_constants() on the CPU over every LayerNorm row of CASES (`python -m tests.xs_ref`): the largest c the
# rounding model needs in |model - ref| <= e |ref| + c stat.  Worst rows: rstd 4.208 on ln320-plain-M257-b5-s1-constrow-eps1e-6
# (row 182, an ordinary row: 160 squares in one fp32 chain per lane), mean 0.603 on ln320-geglu-M300-b3-s1.
#                       measured -> C_STAT_XS = 3 x 4.208 = 12.62
MEASURED = {"stat": 4.208, "mean": 0.603, "rstd": 4.208}
C_STAT_XS = MARGIN * MEASURED["stat"]
AMB_ROW_CAP = 0.02

FAULTS = ("half_mean", "half_var", "affine_shift", "swap_halves", "gate_bias_from_value", "prev_residual", "double_residual",
          "drop_k2_tail", "alpha_block", "stats_unwritten")


# ------------------------------------------------------------------------------------------------ the launcher, transcribed

def call_of(c, lda1=None, ldw1=None, ldc=None, lda2=None, ldw2=None, ldr=None, inplace=False, dtype_bf16=None, ln_beta=True):
    """The host-visible fields of one cl_gemm call of a tests.gemm_ref case (pitches default to the widths)."""
    grouped = c["N"] // c["a2_group_n"] if c["a2_group_n"] else 1
    return dict(M=c["M"], N=c["N"], K1=c["K1"], K2=c["K2"], act=c["act"], mode=c["mode"],
                bf16=(c["dtype"] == BF) if dtype_bf16 is None else dtype_bf16, alpha=c["alpha"], alpha_n=c["alpha_n"],
                a1_group_n=c["a1_group_n"], a2_group_n=c["a2_group_n"], residual=c["residual"] is not None, rowbias=c["rowbias"] is not None,
                atomic=c["atomic"], out_f32=c["out_f32"], splitk=c["splitk"], ln=c["ln"] is not None, ln_beta=ln_beta,
                lda1=c["K1"] if lda1 is None else lda1, ldw1=c["K1"] if ldw1 is None else ldw1,
                ldc=c["out_cols"] if ldc is None else ldc, lda2=grouped * c["K2"] if lda2 is None else lda2,
                ldw2=c["K2"] if ldw2 is None else ldw2, ldr=c["N"] if ldr is None else ldr, inplace=inplace)


def _gemm_refuses(p):
    """launch_gemm's own checks that come before the x-stationary-only forms are handed over (linear mode, act 0 / 3 only)."""
    kpb = 32 if p["bf16"] else 16
    if p["K1"] % kpb or p["K2"] % kpb or p["N"] % 8 or p["ldc"] % 8 or p["K1"] <= 0:
        return True
    if p["mode"] != G.LINEAR:
        return p["K2"] > 0 or p["a1_group_n"] > 0 or p["a2_group_n"] > 0      # (with a zero page; conv + K2 / groups)
    if not p["atomic"] and p["splitk"] > 1:
        return True
    if p["a1_group_n"] < 0 or p["a2_group_n"] < 0:
        return True
    if p["alpha_n"] < 0 or p["alpha_n"] % 8 or p["alpha_n"] > p["N"]:
        return True
    if p["a1_group_n"] and p["N"] % p["a1_group_n"]:
        return True
    if p["a2_group_n"] and (p["N"] % p["a2_group_n"] or not p["K2"]):
        return True
    return False


def _xs_refuses(p):
    """launch_gemm_xs: CL_EINVAL = not a product this kernel covers."""
    geglu = p["act"] == G.ACT_GEGLU_SPLIT
    if p["mode"] != G.LINEAR or p["atomic"] or p["out_f32"] or (p["act"] != G.ACT_NONE and not geglu) or p["rowbias"] or p["a1_group_n"]:
        return True
    if p["N"] % (64 if geglu else 32) or p["M"] < 128 or p["alpha_n"] % 32:
        return True
    if geglu and (p["residual"] or p["alpha"] != 1.0 or p["alpha_n"] or p["a2_group_n"]):
        return True
    if p["a2_group_n"] and (p["a2_group_n"] % 32 or p["N"] % p["a2_group_n"] or not p["K2"]):
        return True
    if p["lda1"] % 8 or p["ldw1"] % 8 or p["ldc"] % 8 or (p["K2"] and (p["lda2"] % 8 or p["ldw2"] % 8)) or (p["residual"] and p["ldr"] % 8):
        return True
    if p["ln"]:
        return bool(p["residual"] or p["K2"] or not p["ln_beta"] or p["K1"] not in (320, 640))
    return (p["K1"], p["K2"]) not in K_FORMS


def accepts(p):
    """'refused' (cl_gemm returns CL_EINVAL), 'xs' (the x-stationary kernel launches it when it is asked to: always for act 3
    and the prologue, under configuration 34 otherwise) or 'tiles' (configuration 34 hands the product to the tile kernels)."""
    if _gemm_refuses(p):
        return "refused"
    only = p["act"] == G.ACT_GEGLU_SPLIT or p["ln"]
    if only and not p["bf16"]:
        return "refused"
    if not p["bf16"] or _xs_refuses(p):
        return "refused" if only else "tiles"
    return "xs"


def instance_of(p):
    epi = XS_GEGLU if p["act"] == G.ACT_GEGLU_SPLIT else XS_RES if p["residual"] else XS_PLAIN
    return (p["K1"], p["K2"], epi, bool(p["ln"]))


def xs_form(p, nsplit=0):
    """launch_xs's run rule for an accepted call.  nsplit: the forced run count (cl_gemm_force_splitk), 0 = the launcher's rule."""
    assert accepts(p) == "xs", p
    K1, K2, epi, lnp = inst = instance_of(p)
    KS1, KS2, RING, MINW = K_FORMS[(K1, K2)]
    CPB = 2 if epi == XS_GEGLU else 1
    MAXB = 80 // CPB
    ncols = p["N"] // 2 if epi == XS_GEGLU else p["N"]
    blocks = ncols // 32
    groups = p["N"] // p["a2_group_n"] if p["a2_group_n"] else 1
    bpg = blocks // groups
    rb = (p["M"] + 127) // 128
    forced = nsplit
    if nsplit <= 0:
        want = 256 * MINW if MINW >= 2 else 256
        nsplit = 1
        while rb * groups * nsplit < want and bpg % (nsplit * 2) == 0 and bpg // (nsplit * 2) >= 5:
            nsplit *= 2
    if nsplit > bpg:
        nsplit = bpg
    while bpg % nsplit:
        nsplit -= 1
    before = nsplit
    while bpg // nsplit > MAXB:
        k = nsplit + 1
        while k <= bpg and bpg % k:
            k += 1
        nsplit = k
    cpw = bpg // nsplit
    D, NACC = RING - 1, (4 if epi == XS_GEGLU else 2)
    nch = cpw * CPB
    return dict(instance=inst, RING=RING, D=D, NACC=NACC, CPB=CPB, groups=groups, bpg=bpg, forced=forced, nsplit=nsplit, cpw=cpw,
                nob=cpw, nch=nch, rb=rb, resplit=nsplit != before, workgroups=rb * groups * nsplit, wg_size=256,
                nch_vs_D="<" if nch < D else "=" if nch == D else ">", nch_mod_nacc=nch % NACC,
                smem=RING * 32 * (KS1 + KS2) * 32 + cpw * CPB * 32 * 4 + (2 * 16 * KS1 * 4 if lnp else 0))


# ------------------------------------------------------------------------------------------------ the rounding model

def _gelu_as32(g):
    """gelu_as of csrc/gemm_xs.hip in fp32, operation by operation (fma = one rounding of the fp64 value)."""
    f = lambda t: t.to(F32)
    fma = lambda a, b, c: (a.double() * b.double() + c).to(F32)
    z = f(g.abs() * f(torch.tensor(0.70710678118654752440)))
    t = f(1.0 / fma(f(torch.tensor(0.3275911)), z, 1.0))
    pl = fma(f(torch.tensor(1.061405429)), t, float(f(torch.tensor(-1.453152027))))
    for a in (1.421413741, -0.284496736, 0.254829592):
        pl = fma(pl, t, float(f(torch.tensor(a))))
    arg = f(f(f(torch.tensor(-1.4426950408889634)) * z) * z)
    c = f(f(pl * t) * torch.exp2(arg))
    return f(f(0.5 * g) * torch.where(g < 0, c, f(2.0 - c)))


def _half_row_sums(t):
    """[M, 2]: what lanes (l31, hi = 0 / 1) hold after the kernel's pass over t [M, K] = pairs already formed as the kernel forms
    them.  t: [M, KS, 2, 4] fp32, the four `lo + hi` (or d0 d0 + d1 d1) terms of every k-step and half."""
    s = t.new_zeros(t.shape[0], 2)
    for j in range(t.shape[1]):
        for e in range(4):
            s = s + t[:, j, :, e]
    return s


def xs_model(c, fault=None):
    """(out [M, out_cols] in the output dtype, stats [M, 2] fp32 or None) of the case as gemm_xs_kernel computes it; `fault`: one
    of FAULTS."""
    assert fault is None or fault in FAULTS, fault
    M, N, K1, K2 = c["M"], c["N"], c["K1"], c["K2"]
    dev = c["a1"].device
    geglu, half = c["act"] == G.ACT_GEGLU_SPLIT, c["N"] // 2
    stats = None
    frow = M // 2                                                  # the row a one-row fault hits
    if c["ln"] is not None:
        gamma, beta, eps = c["ln"]
        gamma, beta = gamma.to(F32), beta.to(F32)
        x = c["a1"].to(F32)
        xr = x.reshape(M, K1 // 16, 2, 4, 2)
        invK = torch.tensor(1.0 / K1, dtype=F32)
        s = _half_row_sums(xr[..., 0] + xr[..., 1])
        tot = s[:, 0] if fault == "half_mean" else s[:, 0] + s[:, 1]
        mean = tot * invK
        d = xr - mean.reshape(M, 1, 1, 1, 1)
        q = _half_row_sums(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
        sq = q[:, 0] if fault == "half_var" else q[:, 0] + q[:, 1]
        rstd = torch.rsqrt(sq * invK + torch.tensor(eps, dtype=F32))
        if fault == "affine_shift":
            gamma, beta = torch.roll(gamma, 8), torch.roll(beta, 8)
        a1 = ((x - mean[:, None]) * rstd[:, None] * gamma + beta).to(BF)
        stats = torch.stack([mean, rstd], 1)
        if fault == "stats_unwritten":
            stats[frow] = float("nan")
    else:
        a1 = c["a1"]
    bias = c["bias"].to(F32) if c["bias"] is not None else torch.zeros(N, dtype=F32, device=dev)
    if fault == "gate_bias_from_value":
        bias = torch.cat([bias[:half], bias[:half]])
    acc = bias.repeat(M, 1)
    groups = N // c["a2_group_n"] if c["a2_group_n"] else 1
    gn = N // groups
    fcol = 32 if N >= 64 else 0                                   # first column of the 32-column block a one-block fault hits
    for g in range(groups):
        cols = slice(g * gn, (g + 1) * gn)
        A, W = a1.double(), c["w1"][cols].double()
        if K2:
            A = torch.cat([A, c["a2"][:, g * K2:(g + 1) * K2].double()], 1)
            W = torch.cat([W, c["w2"][cols].double()], 1)
        a = acc[:, cols]
        for j in range((K1 + K2) // 16):
            step = A[:, 16 * j:16 * j + 16] @ W[:, 16 * j:16 * j + 16].t()
            if fault == "drop_k2_tail" and j == (K1 + K2) // 16 - 1 and g == 0:
                step[:, fcol:fcol + 32] = 0
            a = (a.double() + step).to(F32)
        acc[:, cols] = a
    if geglu:
        val, gate = (acc[:, half:], acc[:, :half]) if fault == "swap_halves" else (acc[:, :half], acc[:, half:])
        out = val * _gelu_as32(gate)
    else:
        al = torch.full((N,), c["alpha"], dtype=F32, device=dev)
        if c["alpha_n"] > 0:
            al[c["alpha_n"] + (32 if fault == "alpha_block" else 0):] = 1.0
        out = acc * al
        if c["residual"] is not None:
            b32 = torch.tensor(c["beta"], dtype=F32).double()
            r = c["residual"].double()
            if fault == "prev_residual":
                r = r.clone()
                r[:, fcol:fcol + 32] = c["residual"].double()[:, fcol - 32:fcol] if fcol else r[:, 32:64]
            out = (out.double() + b32 * r).to(F32)
            if fault == "double_residual":
                out[frow] = (acc[frow] * al).double().add(b32 * out[frow].to(BF).double()).to(F32)
    return out.to(c["out_dtype"]), stats


def stats_gate(c, stats, cst=None):
    """The statistics a launch left in ln_stats [M, 2] against fp64, with norm_ref's gates: dict(violations, err_over_bound, need)."""
    from tests import norm_ref as NR
    cst = C_STAT_XS if cst is None else cst
    P = G.ln_parts(c)
    res = dict(violations=0, err_over_bound=0.0, need={})
    for i, k in enumerate(("mean", "rstd")):
        z = torch.zeros_like(P[k])
        g = NR.gate(stats[:, i], P[k], z, P["stat_" + k], E, cst)
        res["violations"] += g["violations"]
        res["err_over_bound"] = max(res["err_over_bound"], g["err_over_bound"])
        res["need"][k] = g["need"]
        if g["first"] is not None:
            res.setdefault("first", (k, g["first"]))
    return res


# ------------------------------------------------------------------------------------------------ the case table

MS = (128, 129, 257, 300)
NOBS = (1, 2, 3, 4, 5, 7)


def _row(name, inst, M, blocks, nsplit, **kw):
    K1, K2, epi, lnp = inst
    r = dict(name=name, inst=inst, M=M, blocks=blocks, nsplit=nsplit, groups=1, alpha=1.0, alpha_n_blocks=0, beta=1.0, bias=True,
             inplace=False, stats=True, eps=1e-5, const_row=False, family=("ln" + str(K1) if lnp else "k%d+%d" % (K1, K2)) + "-" + EPI_NAME[epi])
    r.update(kw)
    return r


def _cases():
    rows = []
    for q, inst in enumerate(INSTANCES):
        K1, K2, epi, lnp = inst
        tag = ("ln%d" % K1 if lnp else "k%d+%d" % (K1, K2)) + "-" + EPI_NAME[epi]
        add = lambda M, blocks, ns, extra="", **kw: rows.append(_row(f"{tag}-M{M}-b{blocks}-s{ns}{extra}", inst, M, blocks, ns, **kw))
        # the run count forced to 1 (cpw = nob) and the launcher's own rule, output blocks 1 .. 7; M rotates so that every
        # (M, nob) pair is met by some instance and every instance meets every M
        for i, nob in enumerate(NOBS):
            add(MS[(i + q) % 4], nob, 1)
            add(MS[(i + q + 2) % 4], nob, 0)
        add(MS[q % 4], 12, 0)                                      # the rule splits: 12 -> 2 runs of 6
        add(MS[(q + 1) % 4], 4, 4)                                 # one block per workgroup: blockIdx.y > 0 and the statistics
        add(MS[(q + 3) % 4], 12, 5)                                # a forced count that does not divide: 5 -> 4 runs of 3
        if K1 == 320 and K2 in (0, 128):                           # a run longer than the bias image, per epilogue family
            if K2 == 0 or epi == XS_PLAIN:
                add(128, 41 if epi == XS_GEGLU else 81, 1)
        if epi != XS_GEGLU:
            if K2:                                                 # q | k | v: 3 groups of 2 blocks, alpha on the first group
                add(MS[(q + 2) % 4], 6, 0, "-grouped", groups=3, alpha=0.31, alpha_n_blocks=2)
                add(MS[q % 4], 6, 2, "-grouped", groups=3, alpha=0.31, alpha_n_blocks=2)
            add(MS[(q + 1) % 4], 5, 1, "-alpha_mid", alpha=0.31, alpha_n_blocks=3)       # alpha_n inside a workgroup's run
            add(MS[(q + 3) % 4], 4, 1, "-alpha_all", alpha=-0.7)
        if epi == XS_RES:
            add(257, 3, 1, "-beta-0.5-nobias", beta=-0.5, bias=False)
            add(300, 2, 1, "-beta-0.5", beta=-0.5)
            add(128, 3, 1, "-inplace", inplace=True)
            add(128, 5, 0, "-inplace-beta-0.5", inplace=True, beta=-0.5)
            add(129, 3, 1, "-inplace-beta-0.5", inplace=True, beta=-0.5)
            add(129, 2, 1, "-inplace-nobias", inplace=True, bias=False)
            add(300, 4, 1, "-inplace", inplace=True)
            add(300, 7, 0, "-inplace-beta-0.5-nobias", inplace=True, beta=-0.5, bias=False)
        if lnp:
            add(129, 3, 1, "-nostats", stats=False)
            add(300, 2, 2, "-eps1e-6", eps=1e-6)
            add(128, 2, 1, "-constrow", const_row=True)
            add(257, 5, 1, "-constrow-eps1e-6", const_row=True, eps=1e-6)
    names = [r["name"] for r in rows]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return rows


CASES = _cases()
FAMILIES = tuple(dict.fromkeys(r["family"] for r in CASES))


def build_case(row, device="cpu"):
    """The operands of a row, drawn on the CPU from a generator seeded by the row's place in the table and rounded once to bf16.
    x ~ N(0, 1) (the prologue rows: 1.7 randn + 0.6, gamma = 1 + 0.3 randn, beta = 0.3 randn), W ~ N(0, 1 / K), the second segment
    at the magnitude of the first, bias 0.1 randn + 0.05, residual ~ N(0, 1).  Prologue rows: a row of x with an element whose
    fp64 LayerNorm value is ambiguous (tests/gemm_ref.py) is drawn again until at most AMB_ROW_CAP of the rows are left with
    one -- decided by the reference alone."""
    K1, K2, epi, lnp = row["inst"]
    M = row["M"]
    g = torch.Generator().manual_seed(77000 + [r["name"] for r in CASES].index(row["name"]))
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    ncols = row["blocks"] * row["groups"] * 32
    N = 2 * ncols if epi == XS_GEGLU else ncols
    kw = dict(act=G.ACT_GEGLU_SPLIT if epi == XS_GEGLU else G.ACT_NONE, alpha=row["alpha"], alpha_n=32 * row["alpha_n_blocks"])
    w1 = rn(N, K1, sc=K1 ** -0.5).to(BF)
    if K2:
        kw.update(a2=rn(M, K2 * row["groups"]).to(BF), w2=rn(N, K2, sc=K2 ** -0.5).to(BF))
        if row["groups"] > 1:
            kw.update(a2_group_n=N // row["groups"])
    if row["bias"]:
        kw.update(bias=rn(N, sc=0.1) + 0.05)
    if epi == XS_RES:
        kw.update(residual=rn(M, N).to(BF), beta=row["beta"])
    if lnp:
        x = (rn(M, K1, sc=1.7) + 0.6).to(BF)
        gamma, beta = 1 + rn(K1, sc=0.3), rn(K1, sc=0.3)
        if row["const_row"]:
            x[M - 1] = 0.7578125
        keep = int(AMB_ROW_CAP * M) - (1 if row["const_row"] else 0)
        for _ in range(64):
            probe = G.make_case(x, w1[:32], ln=(gamma, beta, row["eps"]))
            bad = (G.ln_parts(probe)["amb_ulp"] != 0).any(1)
            if row["const_row"]:
                bad[M - 1] = False
            idx = bad.nonzero().flatten()[keep:]
            if not len(idx):
                break
            x[idx] = (rn(len(idx), K1, sc=1.7) + 0.6).to(BF)
        else:
            raise AssertionError("no draw under the ambiguous-row cap: " + row["name"])
        kw.update(ln=(gamma, beta, row["eps"]))
    else:
        x = rn(M, K1).to(BF)
    c = G.make_case(x, w1, **kw)
    if device != "cpu":
        mv = lambda t: t.to(device) if torch.is_tensor(t) else t
        for k in ("a1", "w1", "a2", "w2", "bias", "residual"):
            c[k] = mv(c[k])
        if c["ln"] is not None:
            c["ln"] = (c["ln"][0].to(device), c["ln"][1].to(device), c["ln"][2])
    return c


def form_of(row, c=None):
    """(what `accepts` says: 'xs' for every row, the launch form) for a row of the table under forced configuration 34 with the
    row's run count."""
    K1, K2, epi, lnp = row["inst"]
    ncols = row["blocks"] * row["groups"] * 32
    N = 2 * ncols if epi == XS_GEGLU else ncols
    p = dict(M=row["M"], N=N, K1=K1, K2=K2, act=G.ACT_GEGLU_SPLIT if epi == XS_GEGLU else G.ACT_NONE, mode=G.LINEAR, bf16=True,
             alpha=row["alpha"], alpha_n=32 * row["alpha_n_blocks"], a1_group_n=0, a2_group_n=N // row["groups"] if row["groups"] > 1 else 0,
             residual=epi == XS_RES, rowbias=False, atomic=False, out_f32=False, splitk=1, ln=lnp, ln_beta=True,
             lda1=K1 + G.PAD_A1, ldw1=K1 + 8, ldc=ncols + G.PAD_COLS, lda2=K2 * row["groups"] + G.PAD_A2, ldw2=K2 + 16, ldr=N + G.PAD_RES,
             inplace=row["inplace"])
    how = accepts(p)
    return how, (xs_form(p, row["nsplit"]) if how == "xs" else None)


def coverage(rows=None):
    """What the table reaches, from the transcription alone: the set the CPU test compares with the required one."""
    out = set()
    for row in rows if rows is not None else CASES:
        how, f = form_of(row)
        assert how == "xs", row["name"]
        if row["inplace"]:
            out.add(("inplace", f["instance"], row["M"]))
        out.add(("instance", f["instance"]))
        out.add(("ring", f["RING"], "nch" + f["nch_vs_D"] + "D"))
        out.add(("nacc", f["NACC"], f["nch_mod_nacc"]))
        out.add(("M", f["instance"], row["M"]))
        if f["resplit"]:
            out.add(("resplit", EPI_NAME[f["instance"][2]], f["instance"][3]))
        if f["nsplit"] > 1:
            out.add(("runs>1", f["instance"]))
        if f["forced"] and f["forced"] != f["nsplit"] and not f["resplit"]:
            out.add(("forced_count_clamped", f["instance"]))
        if f["groups"] > 1:
            out.add(("grouped", f["instance"], f["nsplit"]))
        if row["alpha_n_blocks"] and row["groups"] == 1 and 0 < row["alpha_n_blocks"] % f["cpw"]:
            out.add(("alpha_n_mid_run", f["instance"]))
    return out


def measure_constants(rows=None):
    """{'mean' | 'rstd': (largest c the model needs, row)} over the prologue rows of the table (CPU)."""
    worst = {"mean": (0.0, ""), "rstd": (0.0, "")}
    for row in rows if rows is not None else CASES:
        if not row["inst"][3]:
            continue
        c = build_case(row)
        need = stats_gate(c, xs_model(c)[1], cst=0.0)["need"]
        for k, v in need.items():
            if v > worst[k][0]:
                worst[k] = (v, row["name"])
    return worst


if __name__ == "__main__":
    import time
    t0 = time.time()
    w = measure_constants()
    print({k: (round(v, 3), n) for k, (v, n) in w.items()}, "-> MEASURED['stat'] =", round(max(v for v, _ in w.values()), 3),
          "C_STAT_XS =", round(MARGIN * max(v for v, _ in w.values()), 3))
    print("rows", len(CASES), "families", len(FAMILIES), "seconds", round(time.time() - t0, 1))
