"""Reference model, rounding model, gates and case table of the attention conformance suite (helpers only: nothing here is
collected).  Shaped like tests/gemm_ref.py, whose Guarded / padded / PAD_FILL it reuses.

Contract (ctrlora_amd/csrc/attention.h, include/ctrlora_hip.h), per sample b and head h, c = scale log2(e):

    S2 = c q k^T                (log2 domain; a PRE-SCALED q holds q c already, and means q_stored / c)
    P  = softmax_j(S2 ln 2),  lse = log2 sum_j 2^S2,  O = P V
    dP = dO V^T,  delta = sum_d O dO,  dS = P o (dP - delta),  dQ = scale dS K,  dK = scale dS^T Q,  dV = P^T dO

`attn_ref64` evaluates this in fp64 on the operands as stored (closed-form gradients: tests/test_attention_reference_model.py
checks them against autograd) and returns one magnitude per output: the sum of absolute terms of that output's LAST
contraction, the score-gradient terms cancellation-aware:

    mag_o = P |V|      W = P o (|dO V^T| + sum_d |O| |dO|)      mag_dq = scale W |K|      mag_dk = scale W^T |Q|      mag_dv = P^T |dO|

(W carries sum_d |O||dO| and not |delta|: in a row that one key dominates dP - delta cancels to almost nothing while each of
its two parts carries the roundings of O.)

`attn_model` is the same computation with the roundings the kernels document and no others: the unnormalised P = 2^(S2 - max)
rounded to the compute type before P V; O rounded; delta taken from the ROUNDED O; P (recomputed from the saved fp32 lse) and
scale dS rounded before the three backward products; the outputs rounded.  denom_rounded = True is the documented form of the
pre-scaled d_head-40 forward (attention_fwd40.hip): the denominator comes out of the matrix pipe, i.e. it is the sum of the
ROUNDED P.  Scores, maxima, the other denominators and delta are fp32 arithmetic in the kernels and exact here.

Element-wise gate, zero violations:   |got - ref| <= u |ref| + c_x u mag_x + score_x,   u = 2^-9 (bf16), 2^-24 (fp32).
c_x = 3 x the largest (|model - ref| - u |ref|) / (u mag_x) over the whole case table (CASES below), measured on the CPU by
measure_constants() -- `python -m tests.attn_ref` prints them -- and written below next to the measured value.  The factor 3
covers what the model keeps exact: summation order, exp2, fp32 score and denominator arithmetic.
lse: absolute error in log2 units, <= LSE_BOUND[dtype] = 3 x the model's largest |lse - ref| over the table (the denominator
of rounded P, the fp32 rounding of the stored lse) + LSE_SCORE_TERM: (d_head + 2) 2^-24 sum_j P_j c sum_d |q_d k_d|, the
first-order bound of a length-d_head fp32 sum in any order (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4; as
gemm_ref's) propagated through d lse / d S2_j = P_j -- the model keeps the scores exact, so its error cannot stand for that one.

score_x is the same named rounding -- the fp32 arithmetic of the scores: the d_head-term sum, the multiply by c, the subtraction of
the maximum -- carried to the outputs.  A score off by delta_ij <= eps ms_ij, eps = (d_head + 2) 2^-24, ms_ij = c sum_d |q_id k_jd|,
moves the normalised P_ij by at most ln 2 P_ij (delta_ij + sum_k P_ik delta_ik): with Ps = P o (ms + mag_s),
    score_o = ln2 eps Ps |V|     score_dv = ln2 eps Ps^T |dO|     WS = ln2 eps Ps o |dP - delta| + P o sum_d score_o |dO|
    score_dq = scale WS |K|      score_dk = scale WS^T |Q|        (the second part of WS: delta is formed from the O that carries score_o)
Derived, not measured, and first order like the lse term.  Without it the fp32 kernels miss the gate (MI355X: o err / bound up to
6.17 at c_o u mag alone, dk 1.30, dv 1.81, dq 0.99, while rel-L2 stays at 6e-7 and lse within 1.4e-6): P = 2^(S2 - max) turns an
ABSOLUTE score error of |S2| 2^-24 ~ 5e-7 into a RELATIVE error of P of the same size, eight fp32 ulps, key by key.  Beside
u = 2^-9 the term is a few per cent of the bf16 bound (err / bound <= 0.72 there with or without it).
"""
import math

import torch

from tests.gemm_ref import GUARD_ROWS, PAD_COLS, PAD_FILL, Guarded, padded  # noqa: F401  (re-exported for the GPU suite)

LOG2E = 1.4426950408889634
BF, F32 = torch.bfloat16, torch.float32
U = {BF: 2.0 ** -9, F32: 2.0 ** -24}

# rel-L2 gates the project already holds (tests/test_gpu_bench_shapes.py, tests/test_gpu_clip_vision.py, the engine's
# fp32 parity gate 5e-4 for the backward)
REL_GATES = {BF: dict(o=6e-3, dq=1e-2, dk=1e-2, dv=1e-2), F32: dict(o=1e-5, dq=5e-4, dk=5e-4, dv=5e-4)}

# Measured by measure_constants() on the CPU over every row of CASES (both denominators of the bf16 forward); the gate uses
# MARGIN x these.  Worst rows -- bf16: o 2.618 fwd40-spike, dq 1.995 tr1-dh16-129x3-pre, dk 2.139 and dv 2.828 fwd40-std4,
# lse 2.586e-3 tr1-dh160-129x3-pre (three keys: log2(1 + 2^-9) = 2.8e-3 is the most one rounded P can move a denominator);
# fp32: o 0.713 t-f32-dh32-129x3, dq 2.159 t-f32-dh8-65x65, dk 3.042 t-f32-dh32-64x320, dv 3.622 t-f32-dh160-64x320 (P is
# recomputed from the fp32-ROUNDED lse: 2^-24 |lse| ln 2 on every P of a row), lse 4.767e-7 t-f32-dh8-64x128.
#                     measured -> c_x = 3 x:  o 7.854   dq 5.985   dk 6.417   dv 8.484   lse 7.759e-3
MEASURED = {BF: dict(o=2.618, dq=1.995, dk=2.139, dv=2.828, lse=2.5863e-3),
            #                                 o 2.139   dq 6.477   dk 9.126   dv 10.866  lse 1.4301e-6
            F32: dict(o=0.713, dq=2.159, dk=3.042, dv=3.622, lse=4.7669e-7)}
MARGIN = 3.0
C = {dt: {k: MARGIN * v for k, v in m.items() if k != "lse"} for dt, m in MEASURED.items()}
LSE_BOUND = {dt: MARGIN * m["lse"] for dt, m in MEASURED.items()}

# launch families and bits of cl_debug_attention_last_launch (ctrlora_amd/csrc/debug_hooks.h)
FAM_TR, FAM_TR_IP, FAM_HYB, FAM_FWD40, FAM_FOLD, FAM_TRANSPOSED = 1, 2, 3, 4, 5, 6
BIT_TAIL, BIT_TQ, BIT_TK, BIT_PRIO = 1, 2, 4, 8
PROBE_FIELDS = ("kind", "family", "dtype", "dh", "fwd_frags", "dq_frags", "dkv_frags", "bits", "lookahead", "remap", "delta_launch",
                "dkv_ran", "grid_fwd", "grid_dq", "grid_dkv", "tile")


def rup(n, m=64):
    return (n + m - 1) // m * m


# ------------------------------------------------------------------------------------------------ reference and model

def _split(x, B, n, H, dh):
    return x.reshape(B, n, H, dh).permute(0, 2, 1, 3)


def _back(x):
    B, H, n, dh = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * n, H * dh)


def _operands(case):
    B, H, N, Nkv, dh = (case[k] for k in ("B", "H", "N", "Nkv", "dh"))
    c = case["scale"] * LOG2E
    q = case["q"].double()
    if case["prescaled"]:
        q = q / c
    return (_split(q, B, N, H, dh), _split(case["k"].double(), B, Nkv, H, dh), _split(case["v"].double(), B, Nkv, H, dh),
            _split(case["do"].double(), B, N, H, dh), c)


def attn_ref64(case, mags=True):
    """fp64 o, dq [B N, inner], dk, dv [B Nkv, inner], lse [B, H, N] (log2 domain) and, with mags, mag_<x> of each and
    mag_s = sum_j P_j c sum_d |q_d k_d| (the score term of the lse gate)."""
    Q, K, V, DO, c = _operands(case)
    sc = case["scale"]
    S2 = torch.einsum("bhid,bhjd->bhij", Q, K) * c
    m = S2.amax(-1, keepdim=True)
    pu = torch.exp2(S2 - m)
    l = pu.sum(-1, keepdim=True)
    P = pu / l
    O = P @ V
    dP = DO @ V.transpose(-1, -2)
    delta = (O * DO).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    out = dict(o=_back(O), lse=(m + torch.log2(l)).squeeze(-1), dq=_back(sc * (dS @ K)), dk=_back(sc * (dS.transpose(-1, -2) @ Q)),
               dv=_back(P.transpose(-1, -2) @ DO))
    if mags:
        W = P * (dP.abs() + (O.abs() * DO.abs()).sum(-1, keepdim=True))
        out.update(mag_o=_back(P @ V.abs()), mag_dq=_back(sc * (W @ K.abs())), mag_dk=_back(sc * (W.transpose(-1, -2) @ Q.abs())),
                   mag_dv=_back(P.transpose(-1, -2) @ DO.abs()))
        # the fp32 score arithmetic carried to the outputs (module docstring)
        ms = torch.einsum("bhid,bhjd->bhij", Q.abs(), K.abs()) * c
        mag_s = (P * ms).sum(-1, keepdim=True)
        le = math.log(2.0) * (case["dh"] + 2) * 2.0 ** -24
        Ps = P * (ms + mag_s)
        so = le * (Ps @ V.abs())
        WS = le * Ps * (dP - delta).abs() + P * (so * DO.abs()).sum(-1, keepdim=True)
        out.update(mag_s=mag_s.squeeze(-1), score_o=_back(so), score_dv=_back(le * (Ps.transpose(-1, -2) @ DO.abs())),
                   score_dq=_back(sc * (WS @ K.abs())), score_dk=_back(sc * (WS.transpose(-1, -2) @ Q.abs())))
    return out


def attn_model(case, dtype, denom_rounded=False, backward=True):
    """The contract with the documented roundings (module docstring), in fp64 between them."""
    r = lambda x: x.to(dtype).double()
    Q, K, V, DO, c = _operands(case)
    sc = case["scale"]
    S2 = torch.einsum("bhid,bhjd->bhij", Q, K) * c
    m = S2.amax(-1, keepdim=True)
    pu = torch.exp2(S2 - m)
    pr = r(pu)
    l = pr.sum(-1, keepdim=True) if denom_rounded else pu.sum(-1, keepdim=True)
    lse = (m + torch.log2(l)).float().double()                 # the saved lse is fp32 in both families
    O = r((pr @ V) / l)
    out = dict(o=_back(O), lse=lse.squeeze(-1))
    if backward:
        P = torch.exp2(S2 - lse)
        delta = (O * DO).sum(-1, keepdim=True)
        dSr = r(sc * P * (DO @ V.transpose(-1, -2) - delta))
        Pr = r(P)
        out.update(dq=_back(r(dSr @ K)), dk=_back(r(dSr.transpose(-1, -2) @ Q)), dv=_back(r(Pr.transpose(-1, -2) @ DO)))
    return out


# ------------------------------------------------------------------------------------------------ the gates

def gate(got, ref, mag, u, c, score=0.0):
    """Element-wise gate of one output: dict(violations, err_over_bound, excess = max (err - u |ref|) / (u mag), rel, first).
    rel = |got - ref|_2 / |ref|_2, or / |mag|_2 where the reference is identically zero up to fp64 noise (degenerate)."""
    g = got.double()
    err = (g - ref).abs()
    bound = u * ref.abs() + c * u * mag + score
    bad = ~(err <= bound)                                  # a NaN in `got` is a violation
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0)).nan_to_num(nan=math.inf)
    excess = ((err - u * ref.abs()) / (u * mag).clamp_min(1e-300)).nan_to_num(nan=math.inf)
    first = None
    n = int(bad.sum())
    if n:
        i = bad.nonzero()[0].tolist()
        first = dict(row=i[0], col=i[1], got=float(g[i[0], i[1]]), ref=float(ref[i[0], i[1]]), bound=float(bound[i[0], i[1]]),
                     rows_hit=int(bad.any(1).sum()), cols_hit=int(bad.any(0).sum()))
    e = torch.where(torch.isnan(g), torch.zeros_like(err), err)
    # rel-L2 needs a reference with digits of its own.  Over ONE key the softmax is constant, so dq = dk = 0 exactly and the
    # fp64 reference is its own cancellation residue (~1e-17 of its terms): there the error is taken relative to the terms.
    degenerate = bool(ref.norm() <= 2.0 ** -40 * mag.norm())
    return dict(violations=n, err_over_bound=float(ratio.max()), excess=float(excess.max()), degenerate=degenerate,
                rel=float(e.norm() / ((mag.norm() if degenerate else ref.norm()) + 1e-30)), first=first)


def lse_gate(got, ref, mag_s, dtype, dh):
    """Absolute error of lse [B, H, N] in log2 units against LSE_BOUND[dtype] + the score term (module docstring)."""
    err = (got.double() - ref).abs()
    bound = LSE_BOUND[dtype] + (dh + 2) * 2.0 ** -24 * mag_s
    bad = ~(err <= bound)
    return dict(violations=int(bad.sum()), err_over_bound=float((err / bound).nan_to_num(nan=math.inf).max()),
                max_abs=float(err.nan_to_num(nan=math.inf).max()))


def check_outputs(case, ref, got, dtype):
    """Gates of every output present in `got` (o / dq / dk / dv 2-D, lse [B, H, N]): {name: gate dict}."""
    res = {}
    for k in ("o", "dq", "dk", "dv"):
        if got.get(k) is not None:
            res[k] = gate(got[k], ref[k], ref["mag_" + k], U[dtype], C[dtype][k], ref["score_" + k])
            res[k]["rel_gate"] = REL_GATES[dtype][k]
    if got.get("lse") is not None:
        res["lse"] = lse_gate(got["lse"], ref["lse"], ref["mag_s"], dtype, case["dh"])
    return res


def failures(res):
    bad = []
    for k, r in res.items():
        if r["violations"]:
            bad.append((k, "elementwise", r["violations"], r["err_over_bound"], r.get("first")))
        if "rel_gate" in r and not r["rel"] < r["rel_gate"]:
            bad.append((k, "rel_l2", r["rel"], r["rel_gate"]))
    return bad


# ------------------------------------------------------------------------------------------------ the case table
# A row: the call (entry, dtype, shape, q contract, debug variant, row scratch), how its operands are drawn (q/k std, spike),
# and the launch FORM it was written for, as the probe reports it: fwd = the forward's fields, bwd = the backward's fields with
# dK / dV wanted and delta fused (the default); bwd_nodkv = fields that differ when dK = dV = NULL.  The suite derives only what
# follows from the debug hook it sets itself (a separate delta launch under fuse_delta(0), which also rules the fold out).

ALL_DH = (8, 16, 32, 40, 80, 160)
# the issue's pairs, and (70, 64): a query tail over whole key tiles (TQ without TK), which none of them has
TAILSET = ((1, 1), (64, 64), (70, 77), (64, 63), (65, 65), (129, 3), (64, 128), (64, 320), (70, 64))
FORMS = ("tr1", "tr2", "hyb", "hyb_la3", "hyb_noremap", "fwd40", "fwd40_spike", "fwd40_large_logits", "bwd_tq0_tk0", "bwd_tq0_tk1",
         "bwd_tq1_tk0", "bwd_tq1_tk1", "bwd_dq2", "bwd_dq1_dkv2", "bwd_dkv2_tail", "bwd_prio", "bwd_variant1", "fold", "fold_dkv4",
         "fold_nodkv_only", "fold_miss_no_ws", "fold_miss_nkv192", "fold_miss_bh511", "fold_miss_tails", "transposed_f32_tile64",
         "transposed_f32_tile32", "transposed_bf16_q1", "transposed_bf16_q2", "wrapper_bf16", "wrapper_f32")


def _tailbits(N, Nkv):
    return (BIT_TQ if N % 64 else 0) | (BIT_TK if Nkv % 64 else 0)


def _row(name, forms, entry, dtype, dh, B, H, N, Nkv, prescaled=False, variant=0, row_ws=False, q_std=1.0, spike=False, fwd=None,
         bwd=None, bwd_nodkv=None):
    return dict(name=name, forms=tuple(forms), entry=entry, dtype=dtype, dh=dh, B=B, H=H, N=N, Nkv=Nkv, prescaled=prescaled,
                variant=variant, row_ws=row_ws, q_std=q_std, spike=spike, fwd=fwd, bwd=bwd, bwd_nodkv=bwd_nodkv or {})


def _tr_fwd(dh, frags, Nkv, N, BH):
    per = 64 * frags
    return dict(kind=1, family=FAM_TR, dh=dh, fwd_frags=frags, bits=BIT_TAIL if Nkv % 64 else 0, grid_fwd=(N + per - 1) // per * BH)


def _tr_bwd(dh, N, Nkv, BH, dq, dkv, prio=False):
    return dict(kind=2, family=FAM_TR, dh=dh, dq_frags=dq, dkv_frags=dkv, dkv_ran=1, delta_launch=0,
                bits=_tailbits(N, Nkv) | (BIT_PRIO if prio else 0), grid_dq=(N + 64 * dq - 1) // (64 * dq) * BH,
                grid_dkv=(Nkv + 64 * dkv - 1) // (64 * dkv) * BH)


_NODKV = dict(dkv_ran=0, dkv_frags=0, grid_dkv=0)


def _cases():
    rows = []
    tq = lambda N, Nkv: "bwd_tq%d_tk%d" % (N % 64 != 0, Nkv % 64 != 0)
    # A. tile-synchronous forward and backward, one fragment: every d_head, the tail set, both q contracts (2 samples x 2 heads)
    for dh in ALL_DH:
        for N, Nkv in TAILSET:
            for pre in (False, True):
                rows.append(_row(f"tr1-dh{dh}-{N}x{Nkv}-{'pre' if pre else 'plain'}", ["tr1", tq(N, Nkv)], "v2", BF, dh, 2, 2, N, Nkv,
                                 prescaled=pre, row_ws=pre and dh == 40, fwd=_tr_fwd(dh, 1, Nkv, N, 4),
                                 bwd=_tr_bwd(dh, N, Nkv, 4, 1, 1), bwd_nodkv=_NODKV))
    # B. two fragments per wave at >= 512 workgroups of 128 rows (forward: d_head <= 80; backward: d_head <= 40), and the
    # other side of each edge.  B x H = 32 x 16 = 512, 7 x 73 = 511, 16 x 16 = 256.
    for i, dh in enumerate((8, 16, 32, 40, 80)):
        two = 2 if dh <= 40 else 1
        for j, (B, H, N, Nkv, ffr, dqf, dkvf, extra) in enumerate((
                (32, 16, 128, 77, 2, two, two, ["bwd_dq2", "bwd_dkv2_tail"]),
                (32, 16, 128, 128, 2, two, two, ["bwd_dq2"]),
                (7, 73, 128, 77, 1, 1, 1, []),
                (7, 73, 128, 128, 1, 1, 1, []),
                (16, 16, 200, 77, 2, two, 1, ["bwd_dq2"]),
                (16, 16, 200, 128, 2, two, 1, ["bwd_dq2"]),
                (16, 16, 128, 200, 1, 1, two, ["bwd_dq1_dkv2"]))):
            pre = (i + j) % 2 == 1
            rows.append(_row(f"tr2-dh{dh}-{B}x{H}-{N}x{Nkv}-{'pre' if pre else 'plain'}",
                             ["tr2" if ffr == 2 else "tr1", tq(N, Nkv)] + (extra if dh <= 40 else []), "v2", BF, dh, B, H, N, Nkv,
                             prescaled=pre, row_ws=pre and dh == 40, fwd=_tr_fwd(dh, ffr, Nkv, N, B * H),
                             bwd=_tr_bwd(dh, N, Nkv, B * H, dqf, dkvf), bwd_nodkv=_NODKV))
    # variants 11 (s_setprio backward: the two-fragment kernels carry it) and 1 (tile-synchronous kernels only)
    for dh in (16, 40):
        rows.append(_row(f"prio-dh{dh}", ["bwd_prio", "tr2"], "v2", BF, dh, 32, 16, 128, 77, variant=11, fwd=_tr_fwd(dh, 2, 77, 128, 512),
                         bwd=_tr_bwd(dh, 128, 77, 512, 2, 2, prio=True), bwd_nodkv=_NODKV))
    for dh in (40, 80):
        two = 2 if dh <= 40 else 1
        rows.append(_row(f"variant1-dh{dh}", ["bwd_variant1", "tr2"], "v2", BF, dh, 16, 16, 256, 128, variant=1,
                         fwd=_tr_fwd(dh, 2, 128, 256, 256), bwd=_tr_bwd(dh, 256, 128, 256, two, 1), bwd_nodkv=_NODKV))
    # C. hybrid forward: d_head 40 / 80, N % 256 == 0, whole key tiles (2, an odd number, five: the ring wraps), >= 256 workgroups
    hyb = lambda dh, la, remap, grid: dict(kind=1, family=FAM_HYB, dh=dh, fwd_frags=4, lookahead=la, remap=remap, grid_fwd=grid)
    for dh in (40, 80):
        two = 2 if dh <= 40 else 1
        for Nkv in (128, 192, 320):
            dkvf = two if (Nkv + 127) // 128 * 256 >= 512 else 1
            rows.append(_row(f"hyb-dh{dh}-256x{Nkv}", ["hyb"], "v2", BF, dh, 16, 16, 256, Nkv, fwd=hyb(dh, 2, 1, 256),
                             bwd=_tr_bwd(dh, 256, Nkv, 256, two, dkvf), bwd_nodkv=_NODKV))
        rows.append(_row(f"hyb-dh{dh}-bh255", ["tr1"], "v2", BF, dh, 15, 17, 256, 128, fwd=_tr_fwd(dh, 1, 128, 256, 255),
                         bwd=_tr_bwd(dh, 256, 128, 255, 1, 1), bwd_nodkv=_NODKV))
        rows.append(_row(f"hyb-dh{dh}-noremap", ["hyb_noremap"], "v2", BF, dh, 13, 10, 512, 192, fwd=hyb(dh, 2, 0, 260),
                         bwd=_tr_bwd(dh, 512, 192, 130, two, 1), bwd_nodkv=_NODKV))
        rows.append(_row(f"hyb-dh{dh}-la3", ["hyb_la3"], "v2", BF, dh, 16, 16, 256, 320, variant=13, fwd=hyb(dh, 3, 1, 256),
                         bwd=_tr_bwd(dh, 256, 320, 256, two, two), bwd_nodkv=_NODKV))
    rows.append(_row("hyb-dh80-pre", ["hyb"], "v2", BF, 80, 16, 16, 256, 192, prescaled=True, fwd=hyb(80, 2, 1, 256),
                     bwd=_tr_bwd(80, 256, 192, 256, 1, 1), bwd_nodkv=_NODKV))
    for variant, la in ((13, 3), (14, 2)):          # pre-scaled d_head 40: these two skip the fwd40 kernel
        rows.append(_row(f"hyb-dh40-pre-v{variant}", ["hyb_la3" if la == 3 else "hyb"], "v2", BF, 40, 16, 16, 256, 320, prescaled=True,
                         variant=variant, fwd=hyb(40, la, 1, 256), bwd=_tr_bwd(40, 256, 320, 256, 2, 2), bwd_nodkv=_NODKV))
    # D. pre-scaled d_head-40 forward: the hybrid shapes; a spike in the last key tile (second pass); large logits.
    # Backward of these rows: row scratch given; the fold needs N % 128 = Nkv % 128 = 0 and 512 two-fragment workgroups on
    # both sides -- Nkv = 128 gives 256 key workgroups: no fold with dK, fold without
    f40 = lambda remap, grid: dict(kind=1, family=FAM_FWD40, dh=40, fwd_frags=4, remap=remap, grid_fwd=grid)
    fold = lambda N, Nkv, BH, dkvf=2: dict(kind=2, family=FAM_FOLD, dh=40, dq_frags=2, dkv_frags=dkvf, dkv_ran=1, delta_launch=0, bits=0,
                                            grid_dq=N // 128 * BH, grid_dkv=Nkv // (64 * dkvf) * BH)
    fold_nodkv = lambda N, BH: dict(family=FAM_FOLD, dq_frags=2, grid_dq=N // 128 * BH, **_NODKV)
    for Nkv in (128, 192, 320):
        dkvf = 2 if (Nkv + 127) // 128 * 256 >= 512 else 1
        rows.append(_row(f"fwd40-256x{Nkv}", ["fwd40"] + (["fold_nodkv_only"] if Nkv == 128 else []), "v2", BF, 40, 16, 16, 256, Nkv,
                         prescaled=True, row_ws=True, fwd=f40(1, 256), bwd=_tr_bwd(40, 256, Nkv, 256, 2, dkvf),
                         bwd_nodkv=fold_nodkv(256, 256) if Nkv == 128 else _NODKV))
    rows.append(_row("fwd40-bh255", ["tr1"], "v2", BF, 40, 15, 17, 256, 128, prescaled=True, row_ws=True, fwd=_tr_fwd(40, 1, 128, 256, 255),
                     bwd=_tr_bwd(40, 256, 128, 255, 1, 1), bwd_nodkv=_NODKV))
    rows.append(_row("fwd40-noremap", ["fwd40"], "v2", BF, 40, 13, 10, 512, 192, prescaled=True, row_ws=True, fwd=f40(0, 260),
                     bwd=_tr_bwd(40, 512, 192, 130, 2, 1), bwd_nodkv=_NODKV))
    rows.append(_row("fwd40-spike", ["fwd40_spike"], "v2", BF, 40, 16, 16, 256, 320, prescaled=True, row_ws=True, spike=True,
                     fwd=f40(1, 256), bwd=_tr_bwd(40, 256, 320, 256, 2, 2), bwd_nodkv=_NODKV))
    rows.append(_row("fwd40-std4", ["fwd40_large_logits"], "v2", BF, 40, 16, 16, 256, 320, prescaled=True, row_ws=True, q_std=4.0,
                     fwd=f40(1, 256), bwd=_tr_bwd(40, 256, 320, 256, 2, 2), bwd_nodkv=_NODKV))
    # E. fold backward (-lse / -delta through the matrix products) and its near misses, which must fall back and still pass
    rows.append(_row("fold-128x128", ["fold", "tr2"], "v2", BF, 40, 32, 16, 128, 128, prescaled=True, row_ws=True,
                     fwd=_tr_fwd(40, 2, 128, 128, 512), bwd=fold(128, 128, 512), bwd_nodkv=fold_nodkv(128, 512)))
    rows.append(_row("fold-128x256-v21", ["fold_dkv4"], "v2", BF, 40, 32, 16, 128, 256, prescaled=True, row_ws=True, variant=21,
                     fwd=_tr_fwd(40, 2, 256, 128, 512), bwd=fold(128, 256, 512, 4), bwd_nodkv=fold_nodkv(128, 512)))
    rows.append(_row("fold-miss-no-ws", ["fold_miss_no_ws"], "v2", BF, 40, 32, 16, 128, 128, prescaled=True, row_ws=False,
                     fwd=_tr_fwd(40, 2, 128, 128, 512), bwd=_tr_bwd(40, 128, 128, 512, 2, 2), bwd_nodkv=_NODKV))
    rows.append(_row("fold-miss-nkv192", ["fold_miss_nkv192"], "v2", BF, 40, 32, 16, 128, 192, prescaled=True, row_ws=True,
                     fwd=_tr_fwd(40, 2, 192, 128, 512), bwd=_tr_bwd(40, 128, 192, 512, 2, 2), bwd_nodkv=_NODKV))
    rows.append(_row("fold-miss-bh511", ["fold_miss_bh511"], "v2", BF, 40, 7, 73, 128, 128, prescaled=True, row_ws=True,
                     fwd=_tr_fwd(40, 1, 128, 128, 511), bwd=_tr_bwd(40, 128, 128, 511, 1, 1), bwd_nodkv=_NODKV))
    rows.append(_row("fold-miss-tails", ["fold_miss_tails"], "v2", BF, 40, 32, 16, 120, 128, prescaled=True, row_ws=True,
                     fwd=_tr_fwd(40, 2, 128, 120, 512), bwd=_tr_bwd(40, 120, 128, 512, 2, 2), bwd_nodkv=_NODKV))
    # F. transposed family (cl_attention_fwd / cl_attention_bwd): fp32 at every d_head (64-key tiles, 32 at d_head >= 80), the
    # tail set; bf16 with one and two query fragments.  The suite runs each row at n_pad / nkv_pad = rup(., 64) and + 64.
    tfw = lambda dt, dh, fr, N, BH: dict(kind=1, family=FAM_TRANSPOSED, dtype=0 if dt == BF else 1, dh=dh, fwd_frags=fr,
                                         tile=32 if (dt == F32 and dh >= 80) else 64, grid_fwd=(N + 64 * fr - 1) // (64 * fr) * BH)
    tbw = lambda dt, dh, N, Nkv, BH: dict(kind=2, family=FAM_TRANSPOSED, dtype=0 if dt == BF else 1, dh=dh, dq_frags=1, dkv_frags=1,
                                          dkv_ran=1, delta_launch=1, tile=32 if (dt == F32 and dh >= 80) else 64, bits=_tailbits(N, Nkv),
                                          grid_dq=(N + 63) // 64 * BH, grid_dkv=(Nkv + 63) // 64 * BH)
    for dh in ALL_DH:
        for N, Nkv in TAILSET:
            rows.append(_row(f"t-f32-dh{dh}-{N}x{Nkv}", ["transposed_f32_tile32" if dh >= 80 else "transposed_f32_tile64"], "t", F32, dh,
                             2, 2, N, Nkv, fwd=tfw(F32, dh, 1, N, 4), bwd=tbw(F32, dh, N, Nkv, 4), bwd_nodkv=_NODKV))
    for N, Nkv in TAILSET:                     # bf16, one query fragment: the tail set at d_head 40
        rows.append(_row(f"t-bf16-dh40-{N}x{Nkv}", ["transposed_bf16_q1"], "t", BF, 40, 2, 2, N, Nkv, fwd=tfw(BF, 40, 1, N, 4),
                         bwd=tbw(BF, 40, N, Nkv, 4), bwd_nodkv=_NODKV))
    rows.append(_row("t-bf16-dh160-q1", ["transposed_bf16_q1"], "t", BF, 160, 2, 2, 70, 77, fwd=tfw(BF, 160, 1, 70, 4),
                     bwd=tbw(BF, 160, 70, 77, 4), bwd_nodkv=_NODKV))
    for dh in (40, 160):
        rows.append(_row(f"t-bf16-dh{dh}-q2", ["transposed_bf16_q2"], "t", BF, dh, 32, 16, 128, 77, fwd=tfw(BF, dh, 2, 128, 512),
                         bwd=tbw(BF, dh, 128, 77, 512), bwd_nodkv=_NODKV))
    # G. through hip.attention / hip.attention_backward (they build the transposes and the row scratch): one ragged shape
    rows.append(_row("wrap-bf16", ["wrapper_bf16"], "wrap", BF, 40, 2, 2, 70, 77, prescaled=True, fwd=_tr_fwd(40, 1, 77, 70, 4),
                     bwd=_tr_bwd(40, 70, 77, 4, 1, 1), bwd_nodkv=_NODKV))
    rows.append(_row("wrap-f32", ["wrapper_f32"], "wrap", F32, 40, 2, 2, 70, 77, fwd=tfw(F32, 40, 1, 70, 4), bwd=tbw(F32, 40, 70, 77, 4),
                     bwd_nodkv=_NODKV))
    return rows


CASES = _cases()
GROUPS = ("tr1", "tr2", "prio", "variant1", "hyb", "fwd40", "fold", "t", "wrap")


def group_of(row):
    return row["name"].split("-")[0]


def make_case(row, device="cpu"):
    """The operands of a row, drawn on the CPU from a generator seeded by the row's place in the table (the same numbers on
    every device), rounded ONCE to the row's dtype.  spike: the last 16 keys of every sample line up with its first queries
    (as tests/test_gpu_bench_shapes.py:_attention_case builds it): scores jump by ~80 nats in the last key tile."""
    B, H, N, Nkv, dh, dt = (row[k] for k in ("B", "H", "N", "Nkv", "dh", "dtype"))
    inner = H * dh
    g = torch.Generator().manual_seed(1000 + [r["name"] for r in CASES].index(row["name"]))
    mk = lambda n, s=1.0: torch.randn(B * n, inner, generator=g) * s
    q32, k32, v32, do32 = mk(N, row["q_std"]), mk(Nkv, row["q_std"]), mk(Nkv), mk(N)
    if row["spike"]:
        kk = k32.reshape(B, Nkv, inner)
        kk[:, -16:, :] = q32.reshape(B, N, inner)[:, :16, :] * 6.0
        k32 = kk.reshape(B * Nkv, inner)
    scale = dh ** -0.5
    q = (q32 * (scale * LOG2E)) if row["prescaled"] else q32
    to = lambda x: x.to(dt).to(device)
    return dict(B=B, H=H, N=N, Nkv=Nkv, dh=dh, scale=scale, prescaled=row["prescaled"], dtype=dt, q=to(q), k=to(k32), v=to(v32),
                do=to(do32))


def measure_row(row, device="cpu"):
    """(excess per output and |lse error| of the rounding model on one row: the figures the constants are 3 x the maxima of,
    the case, its reference, the model's outputs)."""
    case = make_case(row, device)
    dt = row["dtype"]
    ref = attn_ref64(case)
    out, full = dict(o=0.0, dq=0.0, dk=0.0, dv=0.0, lse=0.0), None
    for denom_rounded in ((False, True) if dt == BF else (False,)):
        mod = attn_model(case, dt, denom_rounded=denom_rounded, backward=not denom_rounded)
        full = full or mod
        for k in mod:
            if k == "lse":
                out[k] = max(out[k], float((mod[k] - ref[k]).abs().max()))
            else:
                out[k] = max(out[k], gate(mod[k], ref[k], ref["mag_" + k], U[dt], 1.0)["excess"])
    return out, case, ref, full


def measure_constants(rows=CASES):
    worst = {BF: dict(o=(0.0, ""), dq=(0.0, ""), dk=(0.0, ""), dv=(0.0, ""), lse=(0.0, "")),
             F32: dict(o=(0.0, ""), dq=(0.0, ""), dk=(0.0, ""), dv=(0.0, ""), lse=(0.0, ""))}
    for row in rows:
        m = measure_row(row)[0]
        for k, v in m.items():
            if v > worst[row["dtype"]][k][0]:
                worst[row["dtype"]][k] = (v, row["name"])
    return worst


if __name__ == "__main__":
    import time
    t0 = time.time()
    for dt, w in measure_constants().items():
        print(dt, {k: (round(v, 6 if k == "lse" else 3) if k != "lse" else v, n) for k, (v, n) in w.items()})
    print("rows", len(CASES), "seconds", round(time.time() - t0, 1))
