"""Reference, rounding model, gates and case table of the normalisation conformance suite (helpers only: nothing here is
collected).  Shaped like tests/attn_ref.py; Guarded / padded / PAD_FILL come from tests/gemm_ref.py.

Contract (ctrlora_amd/csrc/norm.hip, include/ctrlora_hip.h).  A statistics group is (sample b, group g) over n = HW C/G elements
for GroupNorm and one row over n = D elements for LayerNorm (the same formulas with B = M, HW = 1, G = 1):

    mean = sum x / n     var = sum (x - mean)^2 / n     rstd = (var + eps)^-1/2     xh = (x - mean) rstd
    z = gamma xh + beta  y = silu(z) or z               stats = (mean, rstd) as float
    dz = dy silu'(z) or dy      s1 = sum gamma dz       s2 = sum gamma dz xh        (over the group)
    dx = rstd (gamma dz - s1 / n - xh s2 / n) [+ accum]
    dgamma_c += sum_{b, p} dz xh        dbeta_c += sum_{b, p} dz                   (ONTO what the vectors hold)

`norm_ref64` evaluates this in fp64 on the operands as stored (tests/test_norm_reference_model.py checks the closed forms
against fp64 autograd) together with the parts of every bound.  `norm_model` is the same computation with the roundings the
kernels document and no others.  GroupNorm: fp32 per-channel sums of x and x^2 (sequential over runs of RUN = 128 pixels, which
is longer than the longest fp32 chain of any launch form), fp64 combine over runs and channels, var = E[x^2] - mean^2 in fp64,
stats stored as float, scale = rstd gamma and shift = beta - mean scale as float, z = x scale + shift and SiLU in fp32, one
output rounding; backward in fp32 element-wise from the float stats, fp32 per-channel sums, fp64 group sums, float k1 / k2 / k3,
one output rounding.  LayerNorm: two-pass fp32 in the kernel's own order (a lane's 8-element vectors v = lane, lane + 64, ...
summed in sequence, then the xor tree over the 64 lanes), rsqrt in fp32.

Element-wise gate, zero violations, e = 2^-24, u = 2^-8 (bf16) or 2^-24 (fp32), the unit roundoff:

    |got - ref| <= u |ref| + fixed + c_stat stat

stat carries the error of the statistics to the output.  dr = e kappa is the relative error of rstd per unit of c_stat, with
kappa = (mean^2 + var + eps) / (var + eps) the conditioning of the sums-of-squares form (1 for the two-pass LayerNorm);
dm = e sqrt(mean^2 + var) that of the mean (LayerNorm: e mean|x|).  exh = |xh| dr + rstd dm is what they do to xh:

    mean: dm            rstd: rstd dr            y: L |gamma| exh,  L = 1.1 (the Lipschitz constant of SiLU) or 1
    dx:   rstd (|gamma| edz + E1 / n + |xh| E2 / n + exh |s2| / n) + dr |dx - accum|
          edz = |dy| |gamma| exh / 2 with SiLU (|silu''| <= 1/2), else 0;  E1 = sum |gamma| edz;  E2 = sum |gamma| (edz |xh| + |dz| exh)
    dgamma: sum (edz |xh| + |dz| exh)        dbeta: sum edz

fixed is derived, first order, and not measured:
  * forward arithmetic: 3 e (|gamma| rstd (|x| + |mean|) + |beta|) L -- the roundings of scale, shift, the product and the sum of
    z = x scale + shift, whose two parts cancel when the mean is large; SiLU adds |y| e (3 + (|z| + 2)(1 - sigmoid z)): the fast
    exponential takes z log2(e) rounded to fp32, an ABSOLUTE error |z| e of the exponent, i.e. a relative one of exp(-z);
  * backward arithmetic: xh to 2 e |xh|, z and silu' recomputed from it, 4 e on the terms of the last expression and on accum;
  * the two fp32 sums of the backward over n terms, as DESIGN.md section 1f bounds a contraction (Higham, Accuracy and Stability of
    Numerical Algorithms, eq. 4.4): 2 n e sum |terms|, carried to dx as rstd (. / n + |xh| . / n);
  * dgamma / dbeta: the same rule over the m = B HW (or M) terms of a column, plus 4 e (|initial| + sum |terms|) for the
    accumulation onto the vectors.

c_stat = MARGIN x the largest value `norm_model` itself needs over the whole table (CASES, every dtype and SiLU / eps pair),
MARGIN = 3 as tests/attn_ref.py.  `python -m tests.norm_ref` measures it on the CPU; the figures are written below.  Nothing here
was fitted to a kernel's output.  The rel-L2 gates the project already holds stay beside it (REL_GATES).
"""
import math

import torch

from tests.attn_ref import MARGIN
from tests.gemm_ref import GUARD_ROWS, PAD_COLS, PAD_FILL, Guarded, padded  # noqa: F401  (re-exported for the GPU suite)

BF, F32 = torch.bfloat16, torch.float32
E = 2.0 ** -24
U = {BF: 2.0 ** -8, F32: 2.0 ** -24}      # unit roundoff of ONE rounding to the output type (bf16: 8 significant bits)
RUN = 128
OUTPUTS = ("y", "mean", "rstd", "dx", "dgamma", "dbeta")

# rel-L2 gates already in use (tests/test_gpu_parity.py, tests/test_gpu_parity_r3.py: 1e-5 in fp32; 6e-3 forward and 1.2e-2
# backward in bf16; dgamma / dbeta 1e-2 whole-vector)
REL_GATES = {BF: dict(y=6e-3, dx=1.2e-2, dgamma=1e-2, dbeta=1e-2), F32: dict(y=1e-5, dx=1e-5, dgamma=1e-2, dbeta=1e-2)}

# Measured by measure_constants() on the CPU over every gated row of CASES: the largest c the rounding model needs in
# |model - ref| <= u |ref| + fixed + c stat, per family.  The gate uses MARGIN x these.
# Worst rows -- GroupNorm: rstd 5.089 and y 4.149 on gn2-2x70x32 fp32 (one channel per group: a group's sums are ONE fp32 chain of
# 70 terms), mean 2.897 there; LayerNorm: rstd 2.054 on ln-1030x8 bf16, mean 2.006 on ln-1030x1032 fp32, y 1.032.  dx, dgamma and
# dbeta of the model pass on their fixed parts alone (need 0; LayerNorm dgamma 0.363).
#                       measured -> c_stat = 3 x:  gn 15.267   ln 6.162
MEASURED = {"gn": 5.089, "ln": 2.054}
C_STAT = {k: MARGIN * v for k, v in MEASURED.items()}

PROBE_FIELDS = ("kind", "form", "dtype", "nv", "lpr_rpi", "threads", "cb_vx", "chunks", "grid_x", "grid_y", "colsum", "passes")
GN_FWD, GN_BWD, LN_FWD, LN_BWD = 1, 2, 3, 4


# ------------------------------------------------------------------------------------------------ launch forms (host logic)
# A transcription of gn_geom / gn1_geom / gn_two_pass_ok / ln_bwd's grid rules (csrc/norm.hip).  The table's builder derives the
# form of every row from it and asserts what the row was written for; the GPU suite asserts it against the probe.

GN1_MIN_WG = 96


def gn_geom(B, HW, C):
    c8 = C // 8
    vx = min(c8, 320)
    py = max(256 // vx, 1)
    want = (1024 + B - 1) // B
    maxc = max(HW // (py * 4), 1)
    nchunk = min(want, maxc, 256)
    ppc = (HW + nchunk - 1) // nchunk
    nchunk = (HW + ppc - 1) // ppc
    return dict(VX=vx, PY=py, threads=vx * py, nchunk=nchunk, ppc=ppc)


def gn1_geom(B, HW, C, G, esize, bwd):
    cg = C // G
    cb = cg
    while cb % 8:
        cb += cg
    if cb > 128 or C % cb:
        return None
    vx = cb // 8
    lpr = 8 if vx <= 8 else 16
    ppw = 64 // lpr
    nw = max(min((HW + ppw - 1) // ppw, 8 if bwd else 16), (cb + 63) // 64)
    nv = (HW + nw * ppw - 1) // (nw * ppw)
    NV = 1 if nv <= 1 else 2 if nv <= 2 else 4 if nv <= 4 else 8 if nv <= 8 else 16
    nblk = C // cb
    if nv > (16 if esize == 2 else 8) or nblk * B < GN1_MIN_WG:
        return None
    return dict(CB=cb, VX=vx, LPR=lpr, NW=nw, NV=NV, nblk=nblk)


def gn_form(B, HW, C, G, dtype, bwd, trainable=False, forced3=False):
    """What cl_debug_norm_last_launch must report for this call (the cooperative form is off)."""
    kind, dt = (GN_BWD if bwd else GN_FWD), (0 if dtype == BF else 1)
    g1 = None if forced3 else gn1_geom(B, HW, C, G, 2 if dtype == BF else 4, bwd)
    if g1:
        return dict(kind=kind, form=1, dtype=dt, nv=g1["NV"], lpr_rpi=g1["LPR"], threads=g1["NW"], cb_vx=g1["CB"], chunks=0,
                    grid_x=g1["nblk"], grid_y=B, colsum=0, passes=1)
    g = gn_geom(B, HW, C)
    two = (not forced3 and C // 8 == g["VX"] and G <= 64 and g["threads"] >= G and g["threads"] >= 64 and not (bwd and trainable))
    return dict(kind=kind, form=2 if two else 3, dtype=dt, nv=0, lpr_rpi=g["PY"], threads=g["threads"], cb_vx=g["VX"],
                chunks=g["nchunk"], grid_x=g["nchunk"], grid_y=B, colsum=0, passes=(C // 8 + g["VX"] - 1) // g["VX"])


def gn_ws_floats(B, HW, C):
    return B * gn_geom(B, HW, C)["nchunk"] * C * 2 + B * C * 4


def ln_form(M, D, dtype, bwd, trainable=False, workspace=True, ws_bytes=64 << 20):
    dt = 0 if dtype == BF else 1
    if not bwd:
        return dict(kind=LN_FWD, form=1, dtype=dt, nv=(D // 8 + 63) // 64, lpr_rpi=1, threads=256, cb_vx=D // 8, chunks=0,
                    grid_x=min((M + 3) // 4, 2048), grid_y=1, colsum=0, passes=1)
    rpi = 4 if D <= 512 else 2 if D <= 1024 else 1
    grid = min((M + 4 * rpi - 1) // (4 * rpi), 2048)
    colsum = 0
    if trainable:
        grid = min(grid, 1024)
        if workspace and grid * 2 * D * 4 <= ws_bytes:
            colsum = 1
        else:
            colsum, grid = 2, min(grid, 512)
    return dict(kind=LN_BWD, form=2 if colsum == 1 else 1, dtype=dt, nv=1 if D <= 512 else 2 if D <= 1024 else 3, lpr_rpi=rpi,
                threads=256, cb_vx=D // 8, chunks=0, grid_x=grid, grid_y=1, colsum=colsum, passes=1)


# ------------------------------------------------------------------------------------------------ reference and bounds

def _geom(case):
    if case["family"] == "ln":
        return case["M"], 1, 1, case["D"]
    return case["B"], case["HW"], case["G"], case["C"] // case["G"]


def _v4(t, case):
    B, HW, G, cg = _geom(case)
    return None if t is None else t.double().reshape(B, HW, G, cg)


def norm_ref64(case, backward=True, bounds=True):
    """fp64 y, mean, rstd [groups], dx, dgamma, dbeta and, with bounds, fixed_<x> and stat_<x> of each (module docstring).
    2-D outputs are [rows, C]; mean / rstd are [B, G] ([M] for LayerNorm)."""
    B, HW, G, cg = _geom(case)
    n, C, ln, silu, eps = HW * cg, G * cg, case["family"] == "ln", case["silu"], case["eps"]
    gs = (1, 3)
    x = _v4(case["x"], case)
    gam, bet = case["gamma"].double().reshape(1, 1, G, cg), case["beta"].double().reshape(1, 1, G, cg)
    mean = x.mean(gs, keepdim=True)
    var = ((x - mean) ** 2).mean(gs, keepdim=True)
    rstd = (var + eps).rsqrt()
    xh = (x - mean) * rstd
    z = gam * xh + bet
    if silu:
        s = torch.sigmoid(z)
        y, ds = z * s, s * (1 + z * (1 - s))
    else:
        s, y, ds = None, z, None
    flat = lambda t: t.reshape(B * HW, C)
    sq = (lambda t: t.reshape(B)) if ln else (lambda t: t.reshape(B, G))
    out = dict(y=flat(y), mean=sq(mean), rstd=sq(rstd), var=sq(var))
    if bounds:
        if ln:
            dr, dm = torch.full_like(mean, E), E * x.abs().mean(gs, keepdim=True)
        else:
            dr, dm = E * (mean ** 2 + var + eps) / (var + eps), E * (mean ** 2 + var).sqrt()
        exh = xh.abs() * dr + rstd * dm
        L = 1.1 if silu else 1.0
        fy = 3 * E * (gam.abs() * rstd * (x.abs() + mean.abs()) + bet.abs()) * L
        if silu:
            fy = fy + y.abs() * E * (3 + (z.abs() + 2) * (1 - s))
        out.update(kappa=sq(dr / E), fixed_y=flat(fy), stat_y=flat(L * gam.abs() * exh), fixed_mean=torch.zeros_like(out["mean"]),
                   stat_mean=sq(dm), fixed_rstd=torch.zeros_like(out["mean"]), stat_rstd=sq(rstd * dr))
    if not backward:
        return out
    dy, acc = _v4(case["dy"], case), _v4(case.get("accum"), case)
    dz = dy * ds if silu else dy
    gdz = gam * dz
    s1, s2 = gdz.sum(gs, keepdim=True), (gdz * xh).sum(gs, keepdim=True)
    core = gdz - s1 / n - xh * s2 / n
    dx = rstd * core
    if acc is not None:
        dx = dx + acc
    cs = lambda t: t.sum((0, 1)).reshape(C)
    dg0, db0 = case["dgamma0"].double(), case["dbeta0"].double()
    out.update(dx=flat(dx), dx0=flat(rstd * core), dgamma=dg0 + cs(dz * xh), dbeta=db0 + cs(dz))
    if bounds:
        e_xh = 2 * E * xh.abs()
        if silu:
            t = 1 - s
            rs_ = ((z.abs() + 2) * t + 2) * E                                   # relative error of the fp32 sigmoid
            e_ds = s * (rs_ * (1 + z.abs() * t + z.abs() * s) + E * (z.abs() + 3 * (1 + z.abs() * t)))
            ez_fix = 3 * E * ((gam * xh).abs() + bet.abs()) + gam.abs() * e_xh
            edz_fix = dy.abs() * (0.5 * ez_fix + e_ds) + E * dz.abs()
            edz_stat = dy.abs() * 0.5 * gam.abs() * exh
        else:
            edz_fix = edz_stat = torch.zeros_like(dz)
        ga = gam.abs()
        gsum = lambda t: t.sum(gs, keepdim=True)
        E1f, E1s = 2 * n * E * gsum(gdz.abs()) + gsum(ga * edz_fix), gsum(ga * edz_stat)
        E2f = 2 * n * E * gsum((gdz * xh).abs()) + gsum(ga * (edz_fix * xh.abs() + dz.abs() * e_xh))
        E2s = gsum(ga * (edz_stat * xh.abs() + dz.abs() * exh))
        fdx0 = rstd * (ga * edz_fix + E1f / n + xh.abs() * E2f / n + e_xh * s2.abs() / n) \
            + 4 * E * rstd * (gdz.abs() + s1.abs() / n + (xh * s2).abs() / n)
        fdx = fdx0 + 4 * E * acc.abs() if acc is not None else fdx0
        sdx = rstd * (ga * edz_stat + E1s / n + xh.abs() * E2s / n + exh * s2.abs() / n) + dr * (rstd * core).abs()
        m = B * HW
        Tg, Tb = cs((dz * xh).abs()), cs(dz.abs())
        out.update(fixed_dx0=flat(fdx0), fixed_dx=flat(fdx), stat_dx=flat(sdx),
                   fixed_dgamma=2 * m * E * Tg + cs(edz_fix * xh.abs() + dz.abs() * e_xh) + 4 * E * (dg0.abs() + Tg),
                   stat_dgamma=cs(edz_stat * xh.abs() + dz.abs() * exh),
                   fixed_dbeta=2 * m * E * Tb + cs(edz_fix) + 4 * E * (db0.abs() + Tb), stat_dbeta=cs(edz_stat))
    return out


# ------------------------------------------------------------------------------------------------ the rounding model

def _run_sums(t):
    """fp32 per-channel sums of t [B, HW, C] (float32), sequential over runs of RUN pixels, fp64 over the runs: [B, C] double."""
    B, HW, C = t.shape
    R = (HW + RUN - 1) // RUN
    if R * RUN != HW:
        t = torch.cat([t, t.new_zeros(B, R * RUN - HW, C)], 1)
    t = t.reshape(B, R, RUN, C)
    s = t.new_zeros(B, R, C)
    for i in range(min(RUN, HW)):
        s = s + t[:, :, i]
    return s.double().sum(1)


def _wave_sum(t, D):
    """The kernel's row sum of t [M, D] (float32): lane l adds its vectors l, l + 64, l + 128 element by element, then the xor
    tree over the 64 lanes."""
    M = t.shape[0]
    d8 = D // 8
    nv = (d8 + 63) // 64
    if nv * 64 != d8:
        t = torch.cat([t, t.new_zeros(M, nv * 512 - D)], 1)
    t = t.reshape(M, nv, 64, 8)
    s = t.new_zeros(M, 64)
    for k in range(nv):
        for e in range(8):
            s = s + t[:, k, :, e]
    idx = torch.arange(64, device=t.device)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, idx ^ o]
    return s[:, 0]


def _silu32(z):
    return z / (1.0 + torch.exp(-z))


def _dsilu32(z):
    s = 1.0 / (1.0 + torch.exp(-z))
    return s * (1.0 + z * (1.0 - s))


def norm_model(case, dtype, backward=True):
    """The contract with the documented roundings (module docstring): what a correct kernel may give at most."""
    f32 = torch.float32
    r = lambda t: t.to(dtype)
    if case["family"] == "ln":
        M, D, eps = case["M"], case["D"], case["eps"]
        x, g, b = case["x"].to(f32), case["gamma"].to(f32), case["beta"].to(f32)
        mean = _wave_sum(x, D) / D
        d = x - mean[:, None]
        rstd = torch.rsqrt(_wave_sum(d * d, D) / D + torch.tensor(eps, dtype=f32, device=x.device))
        out = dict(y=r(d * rstd[:, None] * g + b), mean=mean, rstd=rstd)
        if not backward:
            return out
        dy = case["dy"].to(f32)
        xh = d * rstd[:, None]
        dh = dy * g
        c1, c2 = _wave_sum(dh, D) / D, _wave_sum(dh * xh, D) / D
        gr = rstd[:, None] * (dh - c1[:, None] - xh * c2[:, None])
        if case.get("accum") is not None:
            gr = case["accum"].to(f32) + gr
        out.update(dx=r(gr), dgamma=case["dgamma0"] + _run_sums((dy * xh)[None]).to(f32)[0],
                   dbeta=case["dbeta0"] + _run_sums(dy[None]).to(f32)[0])
        return out
    B, HW, C, G, eps, silu = (case[k] for k in ("B", "HW", "C", "G", "eps", "silu"))
    cg, n = C // G, HW * (C // G)
    x = case["x"].to(f32).reshape(B, HW, C)
    gam, bet = case["gamma"].to(f32), case["beta"].to(f32)
    S, Q = _run_sums(x).reshape(B, G, cg).sum(2), _run_sums(x * x).reshape(B, G, cg).sum(2)
    mean = S / n
    rstd = 1.0 / ((Q / n - mean * mean).clamp_min(0) + eps).sqrt()
    mean_f, rstd_f = mean.to(f32), rstd.to(f32)                                   # stored as float; the backward reads these
    per_c = lambda t: t.repeat_interleave(cg, 1)                                   # [B, G] -> [B, C]
    scd = per_c(rstd_f.double()) * gam.double()                                   # gn1_fwd_kernel: from the float stats
    sc, sh = scd.to(f32), (bet.double() - per_c(mean_f.double()) * scd).to(f32)
    z = x * sc[:, None] + sh[:, None]
    out = dict(y=r(_silu32(z) if silu else z).reshape(B * HW, C), mean=mean_f, rstd=rstd_f)
    if not backward:
        return out
    dy = case["dy"].to(f32).reshape(B, HW, C)
    mu, rs = per_c(mean_f)[:, None], per_c(rstd_f)[:, None]
    xh = (x - mu) * rs
    dz = dy * _dsilu32(xh * gam + bet) if silu else dy
    cs, cq = _run_sums(dz), _run_sums(dz * xh)                                      # [B, C] per-channel sums
    s1 = (gam.double() * cs.to(f32).double()).reshape(B, G, cg).sum(2).to(f32).double()
    s2 = (gam.double() * cq.to(f32).double()).reshape(B, G, cg).sum(2).to(f32).double()
    rd = rstd_f.double()
    k1 = (per_c(rd) * gam.double()).to(f32)[:, None]
    k2, k3 = per_c((rd * s1 / n).to(f32))[:, None], per_c((rd * s2 / n).to(f32))[:, None]
    gr = dz * k1 - k2 - xh * k3
    if case.get("accum") is not None:
        gr = gr + case["accum"].to(f32).reshape(B, HW, C)
    dg, db = case["dgamma0"].clone(), case["dbeta0"].clone()
    for b in range(B):                                                              # one float atomic per channel and sample
        dg, db = dg + cq[b].to(f32), db + cs[b].to(f32)
    out.update(dx=r(gr).reshape(B * HW, C), dgamma=dg, dbeta=db)
    return out


# ------------------------------------------------------------------------------------------------ the gates

def gate(got, ref, fixed, stat, u, c):
    """Element-wise gate of one output: dict(violations, err_over_bound, need = the c at which the worst element would just pass,
    rel, first).  A NaN in `got` is a violation."""
    g = got.double().reshape(ref.shape)
    err = (g - ref).abs()
    base = u * ref.abs() + fixed
    bound = base + c * stat
    bad = ~(err <= bound)
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0)).nan_to_num(nan=math.inf)
    over = err - base
    need = torch.where(over > 0, over / stat.clamp_min(1e-300), torch.zeros_like(over)).nan_to_num(nan=math.inf)
    first, nbad = None, int(bad.sum())
    if nbad:
        i = bad.reshape(-1).nonzero()[0].item()
        first = dict(index=i, got=float(g.reshape(-1)[i]), ref=float(ref.reshape(-1)[i]), bound=float(bound.reshape(-1)[i]))
        if ref.dim() == 2:
            first.update(row=i // ref.shape[1], col=i % ref.shape[1], rows_hit=int(bad.any(1).sum()), cols_hit=int(bad.any(0).sum()))
    e = torch.where(torch.isnan(g), torch.zeros_like(err), err)
    return dict(violations=nbad, err_over_bound=float(ratio.max()), need=float(need.max()), first=first,
                rel=float(e.norm() / (ref.norm() + 1e-30)))


def check_outputs(case, ref, got, dtype, c=None):
    """Gates of every output present in `got`: {name: gate dict}.  mean / rstd / dgamma / dbeta are fp32 in both dtypes."""
    c = C_STAT[case["family"]] if c is None else c
    res = {}
    for k in OUTPUTS:
        if got.get(k) is not None:
            u = U[dtype] if k in ("y", "dx") else E
            res[k] = gate(got[k], ref[k], ref["fixed_" + k], ref["stat_" + k], u, c)
            if k in REL_GATES[dtype]:
                res[k]["rel_gate"] = REL_GATES[dtype][k]
    if case.get("degenerate"):
        # HW C/G = 1: var = 0, xh = 0, dx = 0 exactly, so dx has no reference to be relative to (either dtype).  y = silu?(beta) is
        # reached through x scale - mean scale at rstd = eps^-1/2 (316 or 1000): 2^-24 |x| rstd of absolute error on a value of size
        # |beta| -- the rounding model itself sits at rel-L2 4e-5 .. 2e-4 there, above the fp32 gate of 1e-5 and far below the bf16
        # gate of 6e-3, which therefore stays.  Where a rel-L2 gate is lifted the element-wise gate (its fixed part) is the check.
        res.get("dx", {}).pop("rel_gate", None)
        if dtype == F32:
            res.get("y", {}).pop("rel_gate", None)
    return res


def failures(res):
    bad = []
    for k, r in res.items():
        if r["violations"]:
            bad.append((k, "elementwise", r["violations"], r["err_over_bound"], r["first"]))
        if "rel_gate" in r and not r["rel"] < r["rel_gate"]:
            bad.append((k, "rel_l2", r["rel"], r["rel_gate"]))
    return bad


# ------------------------------------------------------------------------------------------------ the case table
# A GroupNorm row: the shape, how its input is conditioned (cond: mean / spread of every group; None = drawn per group), the
# dtypes it runs in, whether it is gated, and `covers`: the launch forms the row was written for, named
#   <fwd form>/<bwd form frozen>/<bwd form trainable> per dtype  --  1 / 2 / 3 launches, e.g. "1/1/1" or "1/2/3"
# plus the geometry fields the issue names (asserted against the transcription above when the table is built).

def _gn(name, B, HW, C, G=32, cond=None, gated=True, dtypes=(BF, F32), forms=None, expect=None, group="gn1"):
    return dict(name=name, family="gn", group=group, B=B, HW=HW, C=C, G=G, cond=cond, gated=gated, dtypes=dtypes, forms=forms or {},
                expect=expect or {})


def _cases():
    rows = [
        # ---- one-launch rows
        _gn("gn1-3x70x1280", 3, 70, 1280, forms={BF: "1/1/1", F32: "1/1/1"},
            expect={"fwd": dict(cb_vx=40, lpr_rpi=8, nv=1, threads=9, grid_x=32), "bwd": dict(nv=2, threads=8)}),
        _gn("gn1-2x70x1280-below96", 2, 70, 1280, forms={BF: "2/2/3", F32: "2/2/3"}),
        _gn("gn1-3x70x256", 3, 70, 256, forms={BF: "1/1/1", F32: "1/1/1"}, expect={"fwd": dict(cb_vx=8, grid_x=32)}),
        _gn("gn1-3x4x2560", 3, 4, 2560, forms={BF: "1/1/1", F32: "1/1/1"},
            expect={"fwd": dict(cb_vx=80, lpr_rpi=16, threads=2, nv=1), "bwd": dict(threads=2)}),
        _gn("gn1-6x70x1920", 6, 70, 1920, forms={BF: "1/1/1", F32: "1/1/1"}, expect={"fwd": dict(cb_vx=120, lpr_rpi=16, grid_x=16)}),
        _gn("gn1-12x70x960", 12, 70, 960, forms={BF: "1/1/1", F32: "1/1/1"}, expect={"fwd": dict(cb_vx=120, grid_x=8)}),
        _gn("gn1-3x130x1280", 3, 130, 1280, forms={BF: "1/1/1", F32: "1/1/1"}, expect={"fwd": dict(nv=2), "bwd": dict(nv=4)}),
        _gn("gn1-3x260x1280", 3, 260, 1280, forms={BF: "1/1/1", F32: "1/1/1"}, expect={"fwd": dict(nv=4), "bwd": dict(nv=8)}),
        _gn("gn1-3x520x1280", 3, 520, 1280, forms={BF: "1/1/1", F32: "1/2/3"}, expect={"fwd": dict(nv=8), "bwd_bf16": dict(nv=16)}),
        _gn("gn1-3x1030x1280", 3, 1030, 1280, forms={BF: "1/2/3", F32: "2/2/3"}, expect={"fwd_bf16": dict(nv=16, threads=16)}),
        _gn("gn1-3x600x2560", 3, 600, 2560, forms={BF: "1/2/3", F32: "2/2/3"}, expect={"fwd_bf16": dict(nv=16, lpr_rpi=16, cb_vx=80)}),
        _gn("gn1-2x70x2560-g64", 2, 70, 2560, G=64, forms={BF: "1/1/1", F32: "1/1/1"}, expect={"fwd": dict(cb_vx=40, grid_x=64)}),
        _gn("gn1-2x70x384-g48", 2, 70, 384, G=48, forms={BF: "1/1/1", F32: "1/1/1"}, expect={"fwd": dict(cb_vx=8, grid_x=48)}),
        # ---- two-launch rows (frozen backward two-launch, trainable three-launch)
        _gn("gn2-2x70x320", 2, 70, 320, group="gn2", forms={BF: "2/2/3", F32: "2/2/3"}, expect={"fwd": dict(cb_vx=40, lpr_rpi=6, chunks=2)}),
        _gn("gn2-2x70x2560", 2, 70, 2560, group="gn2", forms={BF: "2/2/3", F32: "2/2/3"}, expect={"fwd": dict(cb_vx=320, lpr_rpi=1)}),
        _gn("gn2-2x70x32", 2, 70, 32, group="gn2", forms={BF: "2/2/3", F32: "2/2/3"}, expect={"fwd": dict(cb_vx=4, lpr_rpi=64)}),
        _gn("gn2-2x300x512", 2, 300, 512, group="gn2", forms={BF: "2/2/3", F32: "2/2/3"}, expect={"fwd": dict(chunks=18)}),
        _gn("gn2-2x4100x320", 2, 4100, 320, group="gn2", forms={BF: "2/2/3", F32: "2/2/3"}, expect={"fwd": dict(chunks=164)}),
        _gn("gn2-1x16390x128", 1, 16390, 128, group="gn2", forms={BF: "2/2/3", F32: "2/2/3"}, expect={"fwd": dict(lpr_rpi=16, chunks=253)}),
        _gn("gn2-2x5x8-g1", 2, 5, 8, G=1, group="gn2", forms={BF: "2/2/3", F32: "2/2/3"}),
        _gn("gn2-1x1x8-g8", 1, 1, 8, G=8, group="gn2", forms={BF: "2/2/3", F32: "2/2/3"}),
        # ---- three-launch rows
        _gn("gn3-3x70x5120", 3, 70, 5120, group="gn3", forms={BF: "3/3/3", F32: "3/3/3"}, expect={"fwd": dict(passes=2), "bwd": dict(passes=2)}),
        _gn("gn3-1x37x5120", 1, 37, 5120, group="gn3", forms={BF: "3/3/3", F32: "3/3/3"}, expect={"fwd": dict(passes=2)}),
        _gn("gn3-1x37x7680-g8", 1, 37, 7680, G=8, group="gn3", forms={BF: "3/3/3", F32: "3/3/3"}, expect={"fwd": dict(passes=3)}),
        _gn("gn3-1x70x512-g128", 1, 70, 512, G=128, group="gn3", forms={BF: "3/3/3", F32: "3/3/3"}),
        # ---- conditioning: mean = 8 spread (kappa ~ 65) gated in both dtypes, one row per form
        _gn("k65-gn1-3x70x1280", 3, 70, 1280, cond=8.0, group="cond", forms={BF: "1/1/1", F32: "1/1/1"}),
        _gn("k65-gn2-2x300x512", 2, 300, 512, cond=8.0, group="cond", forms={BF: "2/2/3", F32: "2/2/3"}),
        _gn("k65-gn3-1x37x5120", 1, 37, 5120, cond=8.0, group="cond", forms={BF: "3/3/3", F32: "3/3/3"}),
        # ---- mean = 64 spread (kappa ~ 4000), fp32: measured and recorded beside torch's own group_norm, not gated
        _gn("k4000-gn1-3x70x1280", 3, 70, 1280, cond=64.0, gated=False, dtypes=(F32,), group="cond", forms={F32: "1/1/1"}),
        _gn("k4000-gn2-2x300x512", 2, 300, 512, cond=64.0, gated=False, dtypes=(F32,), group="cond", forms={F32: "2/2/3"}),
        _gn("k4000-gn3-1x37x5120", 1, 37, 5120, cond=64.0, gated=False, dtypes=(F32,), group="cond", forms={F32: "3/3/3"}),
    ]
    for D in (8, 64, 320, 512, 520, 640, 1024, 1032, 1280, 1536):
        for M in (1, 5, 77, 1030):
            rows.append(dict(name=f"ln-{M}x{D}", family="ln", group="ln", M=M, D=D, gated=True, dtypes=(BF, F32), cap=False))
    for M, D in ((32773, 64), (16389, 640), (8197, 1280)):
        rows.append(dict(name=f"lncap-{M}x{D}", family="ln", group="lncap", M=M, D=D, gated=True, dtypes=(BF, F32), cap=True))
    for row in rows:
        _assert_row(row)
    return rows


def _assert_row(row):
    """The table's own claims against the transcription of the launchers."""
    if row["family"] == "ln":
        M, D = row["M"], row["D"]
        f = ln_form(M, D, BF, True, True)
        if row["cap"]:
            assert ln_form(M, D, BF, True, False)["grid_x"] == 2048 and f["grid_x"] == 1024, row["name"]
            assert ln_form(M, D, BF, True, True, workspace=False)["grid_x"] == 512
            assert M > 2048 * 4 * f["lpr_rpi"] and M % (4 * f["lpr_rpi"])            # the stride loop runs, and a clamped row exists
        return
    B, HW, C, G = (row[k] for k in ("B", "HW", "C", "G"))
    for dt, s in row["forms"].items():
        got = "%d/%d/%d" % (gn_form(B, HW, C, G, dt, False)["form"], gn_form(B, HW, C, G, dt, True, False)["form"],
                            gn_form(B, HW, C, G, dt, True, True)["form"])
        assert got == s, (row["name"], dt, got, s)
    for key, want in row["expect"].items():
        side, _, only = key.partition("_")
        for dt in row["dtypes"]:
            if only and (only == "bf16") != (dt == BF):
                continue
            f = gn_form(B, HW, C, G, dt, side == "bwd")
            assert all(f[k] == v for k, v in want.items()), (row["name"], key, dt, f, want)


def covered_forms(rows=None):
    """The set of launch forms the table reaches, as tuples the CPU test compares with the required set."""
    out = set()
    for row in rows if rows is not None else CASES:
        if row["family"] == "ln":
            M, D = row["M"], row["D"]
            f = ln_form(M, D, BF, True)
            out.add(("ln", f["nv"], f["lpr_rpi"], "cap" if row["cap"] else ("ragged" if M % (4 * f["lpr_rpi"]) else "whole")))
            continue
        B, HW, C, G = (row[k] for k in ("B", "HW", "C", "G"))
        for dt in row["dtypes"]:
            for bwd, tr in ((False, False), (True, False), (True, True)):
                f = gn_form(B, HW, C, G, dt, bwd, tr)
                tag = "bf16" if dt == BF else "f32"
                if f["form"] == 1:
                    out.add(("gn1", tag, "bwd" if bwd else "fwd", f["cb_vx"], f["lpr_rpi"], f["nv"]))
                    if f["threads"] > (HW + 64 // f["lpr_rpi"] - 1) // (64 // f["lpr_rpi"]):
                        out.add(("gn1", "padding_waves"))
                    if f["grid_x"] * B == GN1_MIN_WG:
                        out.add(("gn1", "threshold"))
                else:
                    out.add(("gn%d" % f["form"], "bwd" if bwd else "fwd", f["cb_vx"], f["lpr_rpi"], f["passes"]))
                    out.add(("chunks", f["chunks"]))
                if G != 32:
                    out.add(("groups", G))
                if f["form"] == 3 and C // G > 256:
                    out.add(("gn3", "finalize_rounds", (C // G + 255) // 256))
                if row["cond"]:
                    out.add(("cond", row["cond"], f["form"], tag))
    return out


CASES = _cases()
GROUPS = ("gn1", "gn2", "gn3", "cond", "ln", "lncap")
VARIANTS = ((True, 1e-5), (False, 1e-6))              # (SiLU, eps): the ResBlock norm and the SpatialTransformer norm


def make_case(row, dtype, silu=True, eps=1e-5, device="cpu"):
    """The operands of a row, drawn on the CPU from a generator seeded by the row's place in the table, rounded ONCE to dtype.
    Every (sample, group) gets a mean in [-2, 2] and a spread in [0.5, 2] of its own (cond: mean = cond x spread, sign drawn),
    gamma = 1 + 0.2 randn, beta = 0.2 randn, dy and accum random, dgamma / dbeta start at non-zero values."""
    g = torch.Generator().manual_seed(5000 + [r["name"] for r in CASES].index(row["name"]))
    if row["family"] == "ln":
        B, HW, G, C = row["M"], 1, 1, row["D"]
    else:
        B, HW, G, C = row["B"], row["HW"], row["G"], row["C"]
    cg = C // G
    sig = 0.5 + 1.5 * torch.rand(B, 1, G, 1, generator=g)
    mu = 4.0 * torch.rand(B, 1, G, 1, generator=g) - 2.0
    if row.get("cond"):
        mu = row["cond"] * sig * torch.where(torch.rand(B, 1, G, 1, generator=g) < 0.5, -1.0, 1.0)
    x = (mu + sig * torch.randn(B, HW, G, cg, generator=g)).reshape(B * HW, C)
    to = lambda t: t.to(dtype).to(device)
    case = dict(family=row["family"], name=row["name"], dtype=dtype, silu=silu and row["family"] == "gn", eps=eps, x=to(x),
                gamma=(1 + 0.2 * torch.randn(C, generator=g)).to(device), beta=(0.2 * torch.randn(C, generator=g)).to(device),
                dy=to(torch.randn(B * HW, C, generator=g)), accum=to(torch.randn(B * HW, C, generator=g)),
                dgamma0=(0.5 + torch.rand(C, generator=g)).to(device), dbeta0=(-0.5 - torch.rand(C, generator=g)).to(device),
                degenerate=row["family"] == "gn" and HW * cg == 1)
    case.update(dict(M=B, D=C) if row["family"] == "ln" else dict(B=B, HW=HW, C=C, G=G))
    return case


def measure_row(row, dtype, silu, eps, device="cpu"):
    """(the c each output of the rounding model needs on this row, case, reference, model outputs)."""
    case = make_case(row, dtype, silu, eps, device)
    ref, mod = norm_ref64(case), norm_model(case, dtype)
    res = check_outputs(case, ref, mod, dtype, c=0.0)
    return {k: r["need"] for k, r in res.items()}, case, ref, mod


def without_accum(ref):
    """The reference of the same call with accum = NULL (dx and its fixed part lose the accum terms)."""
    return dict(ref, dx=ref["dx0"], fixed_dx=ref["fixed_dx0"])


def variants_of(row):
    return VARIANTS if row["family"] == "gn" else ((False, 1e-5),)


def measure_constants(rows=None, lowest=None):
    """{family: {output: (largest need over the gated rows, the row that needs it)}}; `lowest`, a dict, receives the smallest need
    per family and output the same way (the other end of the model's err / bound range)."""
    worst = {"gn": {k: (0.0, "") for k in OUTPUTS}, "ln": {k: (0.0, "") for k in OUTPUTS}}
    for row in rows if rows is not None else CASES:
        if not row["gated"]:
            continue
        for dt in row["dtypes"]:
            for silu, eps in variants_of(row):
                need = measure_row(row, dt, silu, eps)[0]
                for k, v in need.items():
                    tag = "%s %s silu=%d" % (row["name"], "bf16" if dt == BF else "f32", silu)
                    if v > worst[row["family"]][k][0]:
                        worst[row["family"]][k] = (v, tag)
                    if lowest is not None and v < lowest.setdefault(row["family"], {}).get(k, (math.inf, ""))[0]:
                        lowest[row["family"]][k] = (v, tag)
    return worst


if __name__ == "__main__":
    import time
    t0 = time.time()
    for fam, w in measure_constants().items():
        print(fam, {k: (round(v, 3), n) for k, (v, n) in w.items()}, "-> MEASURED =", round(max(v for v, _ in w.values()), 3))
    print("rows", len(CASES), "seconds", round(time.time() - t0, 1))
