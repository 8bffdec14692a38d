"""Reference model, rounding model, gate and case table of the two image-prompt attention kernels behind cl_attention_fwd_ip:
attn_fwd_tr_ip_kernel<DH, QW> (csrc/attention_tr.hip, bf16) and attn_fwd_ip_kernel<float, DH, 1, BKV> (csrc/attention_fwd.hip,
fp32).  Helpers only: nothing here is collected.  The method is tests/attn_ref.py's, whose gate(), U, REL_GATES, MARGIN, Guarded and
padded it reuses; shaped like tests/attn_causal_ref.py.

Contract (include/ctrlora_hip.h: cl_attention_fwd_ip; hip.attention_fwd_ip), per sample b and head h, c = scale log2(e):

    S1 = c q k^T,  S2 = c q k_ip^T  (log2 domain; a PRE-SCALED q holds q c already, and means q_stored / c)
    O  = softmax_j(S1 ln 2) V + ip_scale softmax_j(S2 ln 2) V_ip              two SEPARATE softmaxes; Nip keys per sample

`ip_ref64` evaluates this in fp64 on the operands as stored and returns, with P1 / P2 the two softmaxes,

    mag_o   = P1 |V| + |ip_scale| P2 |V_ip|
    score_o = ln2 eps ((P1 o (ms1 + mag_s1)) |V| + |ip_scale| (P2 o (ms2 + mag_s2)) |V_ip|)

attn_ref's score term (the fp32 arithmetic of the scores carried to the output: eps = (d_head + 2) 2^-24, ms_ij = c sum_d |q_id k_jd|,
mag_s = sum_j P_j ms_j), evaluated for each softmax and summed with the weights of the contract.

`ip_model` is the contract with the roundings each kernel documents and no others, fp64 between them.
  bf16 (the comment above attn_fwd_tr_ip_kernel): the unnormalised P1 = 2^(S1 - max) is rounded to bf16 before P1 V; the text part is
    normalised by the UNROUNDED l1 = sum_j P1; the image-prompt row is whole within its one tile, so P2 ip_scale / l2 is rounded to
    bf16 before it multiplies V_ip; the same accumulators end as O1 / l1 + ip_scale O2 / l2 and are rounded once on the store.
  fp32 (the comment above attn_fwd_ip_kernel): the unnormalised P of both parts is rounded to fp32 before its product; O1 / l1 is set
    aside when the first image-prompt tile starts and the running max / sum restart; the epilogue adds ip_scale O2 / l2 and the sum is
    rounded once on the store.

Element-wise gate, zero violations, every case:   |got - ref| <= u |ref| + c_o u mag_o + score_o,   u = 2^-9 (bf16), 2^-24 (fp32)
c_o = MARGIN x the rounding model's worst (|model - ref| - u |ref|) / (u mag_o) over CASES, per dtype, measured on the CPU by
measure_constants() (`python -m tests.attn_ip_ref` prints it) and written below next to the measured value; MARGIN = 3 as in attn_ref:
it covers what the model keeps exact -- summation order, exp2, the fp32 score, denominator and epilogue arithmetic.  Nothing is fitted
to a kernel's output.  The rel-L2 gate is REL_GATES[dtype]["o"]: 6e-3 (bf16), 1e-5 (fp32).

`ip_model(..., defect=...)` evaluates the same rounding model with one planted defect (DEFECTS below); tests/
test_attention_ip_reference_model.py shows that each of them fails the gate on a named row.
"""
import math

import torch

from tests.attn_ref import (ALL_DH, BF, F32, FAM_TR_IP, LOG2E, MARGIN, PROBE_FIELDS, REL_GATES, U, Guarded, gate,  # noqa: F401
                            padded, rup)                                          # (re-exported for the GPU suite)

# measured by measure_constants() on the CPU over every row of CASES -- worst rows: bf16 2.021 (bf16-dh40-65x77x16-std4), fp32 0.438
# (f32-dh40-65x77x16-std4): large logits leave a few keys per row, so the rounded P do not average out
#                                    -> c_o = 3 x:  bf16 6.063   fp32 1.314
MEASURED = {BF: 2.021, F32: 0.438}
C_O = {dt: MARGIN * v for dt, v in MEASURED.items()}

IP_SCALES = (0.0, 0.6, 1.0)
# (N, Nkv, Nip): one, two and three 64-key text tiles (the bf16 kernel parks the image-prompt tile in LDS buffer ntiles & 1: either
# buffer, prefetched behind a first, a middle and an only text tile); a ragged last query block (N % 16 != 0: the min(row, N - 1)
# clamp on Q, the row < N guard on the store); Nip on and off a 16-key fragment edge, one key, and the maximum 64
TAILSET = ((1, 1, 1), (64, 64, 64), (63, 65, 3), (65, 77, 4), (70, 77, 16), (16, 77, 1), (129, 128, 17), (64, 129, 63), (130, 154, 4))

DEFECTS = ("joint", "nip_minus", "nip_plus", "scale_both", "scale_dropped", "wrong_buffer", "sample_stride", "double_c")


# ------------------------------------------------------------------------------------------------ the case table
# A row: the call (dtype, shape, q contract, ip_scale, for fp32 the two V^T key pitches), how its operands are drawn (q_std), and the
# launch FORM it was written for, as the probe reports it: fwd_frags (query fragments per wave: attn_fwd_tr_ip_kernel<DH, 2> for
# d_head <= 80 at >= 512 workgroups of 128 rows, <DH, 1> otherwise; fp32 always 1) and, fp32, the key-tile width (32 for d_head >= 80).

def _row(name, dtype, dh, B, H, N, Nkv, Nip, ip_scale, prescaled=False, q_std=1.0, fwd_frags=1, vt_pads=None):
    assert 1 <= Nip <= 64 and not (prescaled and dtype == F32)
    return dict(name=name, dtype=dtype, dh=dh, B=B, H=H, N=N, Nkv=Nkv, Nip=Nip, ip_scale=ip_scale, prescaled=prescaled, q_std=q_std,
                fwd_frags=fwd_frags, tile=None if dtype == BF else (32 if dh >= 80 else 64),
                vt_pads=None if dtype == BF else (vt_pads or (rup(Nkv), 64)))


def _cases():
    rows = []
    # A. the tail set at every d_head: bf16 with both q contracts, fp32 (2 samples x 2 heads).  ip_scale rotates over IP_SCALES with
    # the row's place in the table, one step per d_head, per shape and per variant (all three loop lengths are multiples of 3: a
    # plain index % 3 would pin one ip_scale to every variant)
    for i, dh in enumerate(ALL_DH):
        for j, (N, Nkv, Nip) in enumerate(TAILSET):
            for k, (dt, tag, pre) in enumerate(((BF, "bf16", False), (BF, "bf16", True), (F32, "f32", False))):
                rows.append(_row(f"{tag}-dh{dh}-{N}x{Nkv}x{Nip}" + ("" if dt == F32 else ("-pre" if pre else "-plain")), dt, dh, 2, 2, N,
                                 Nkv, Nip, IP_SCALES[(i + j + k) % 3], prescaled=pre))
    # B. large logits (q and k of standard deviation 4: scores of ~100 log2 units at d_head 40)
    rows.append(_row("bf16-dh40-65x77x16-std4", BF, 40, 2, 2, 65, 77, 16, 0.6, q_std=4.0))
    rows.append(_row("f32-dh40-65x77x16-std4", F32, 40, 2, 2, 65, 77, 16, 0.6, q_std=4.0))
    # C. bf16, two query fragments per wave: ceil(N / 128) H B >= 512 and d_head <= 80.  32 x 8 x 2 = 512; 31 x 8 x 2 = 496 is one
    # step under it, and d_head 160 has no two-fragment instantiation
    for i, dh in enumerate((8, 16, 32, 40, 80)):
        for j, (B, H, N, Nkv, Nip, frags) in enumerate(((32, 8, 130, 77, 4, 2), (32, 8, 255, 77, 64, 2), (31, 8, 130, 77, 4, 1))):
            pre = (i + j) % 2 == 1
            rows.append(_row(f"bf16-q{frags}-dh{dh}-{B}x{H}-{N}x{Nkv}x{Nip}-{'pre' if pre else 'plain'}", BF, dh, B, H, N, Nkv, Nip,
                             IP_SCALES[1 + (i + j) % 2], prescaled=pre, fwd_frags=frags))
    rows.append(_row("bf16-q1-dh160-32x8-130x77x4-plain", BF, 160, 32, 8, 130, 77, 4, 1.0, fwd_frags=1))
    # D. fp32, 32-key tiles (d_head >= 80): Nkv / Nip on and one past a tile (Nip 33 .. 64 is TWO image-prompt tiles behind the
    # softmax restart at t == nt1), each at the tight V^T key pitches and at pitches with room behind the zero padding
    for dh in (80, 160):
        for N, Nkv, Nip in ((65, 32, 32), (65, 33, 33), (65, 77, 64)):
            for extra, ld2 in ((0, 64), (64, 128)):
                rows.append(_row(f"f32-t32-dh{dh}-{N}x{Nkv}x{Nip}-p{extra}", F32, dh, 2, 2, N, Nkv, Nip, 0.6 if extra else 1.0,
                                 vt_pads=(rup(Nkv) + extra, ld2)))
    return rows


CASES = _cases()
_INDEX = {r["name"]: i for i, r in enumerate(CASES)}


def by_name(name):
    return CASES[_INDEX[name]]


def make_case(row, device="cpu"):
    """Operands of a row, drawn on the CPU from a generator seeded by the row's place in the table (the same numbers on every
    device), rounded ONCE to the row's dtype."""
    B, H, N, Nkv, Nip, dh, dt = (row[k] for k in ("B", "H", "N", "Nkv", "Nip", "dh", "dtype"))
    inner, scale = H * dh, dh ** -0.5
    g = torch.Generator().manual_seed(9000 + _INDEX[row["name"]])
    mk = lambda n, s=1.0: torch.randn(B * n, inner, generator=g) * s
    q32, k32, v32, ki32, vi32 = mk(N, row["q_std"]), mk(Nkv, row["q_std"]), mk(Nkv), mk(Nip, row["q_std"]), mk(Nip)
    if row["prescaled"]:
        q32 = q32 * (scale * LOG2E)
    to = lambda x: x.to(dt).to(device)
    return dict(B=B, H=H, N=N, Nkv=Nkv, Nip=Nip, dh=dh, scale=scale, ip_scale=row["ip_scale"], prescaled=row["prescaled"], dtype=dt,
                q=to(q32), k=to(k32), v=to(v32), k_ip=to(ki32), v_ip=to(vi32))


# ------------------------------------------------------------------------------------------------ reference and model

def _split(x, B, n, H, dh):
    return x.double().cpu().reshape(B, n, H, dh).permute(0, 2, 1, 3)


def _back(x):
    B, H, n, dh = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * n, H * dh)


def _operands(case):
    B, H, N, Nkv, Nip, dh = (case[k] for k in ("B", "H", "N", "Nkv", "Nip", "dh"))
    c = case["scale"] * LOG2E
    Q = _split(case["q"], B, N, H, dh)
    if case["prescaled"]:
        Q = Q / c
    return (Q, _split(case["k"], B, Nkv, H, dh), _split(case["v"], B, Nkv, H, dh), _split(case["k_ip"], B, Nip, H, dh),
            _split(case["v_ip"], B, Nip, H, dh), c)


def _scores(Q, K, c):
    return torch.einsum("bhid,bhjd->bhij", Q, K) * c


def _softmax(S2):
    """(unnormalised 2^(S2 - max), its row sum)."""
    pu = torch.exp2(S2 - S2.amax(-1, keepdim=True))
    return pu, pu.sum(-1, keepdim=True)


def ip_ref64(case):
    """fp64 o [B N, H dh], mag_o and score_o (module docstring)."""
    Q, K, V, K2, V2, c = _operands(case)
    le =math.log(2.0) * (case["dh"] + 2) * 2.0 ** -24
    o = mag = score = 0.0
    for Kx, Vx, w in ((K, V, 1.0), (K2, V2, case["ip_scale"])):
        pu, l = _softmax(_scores(Q, Kx, c))
        P = pu / l
        ms = _scores(Q.abs(), Kx.abs(), c)
        mag_s = (P * ms).sum(-1, keepdim=True)
        o = o + w * (P @ Vx)
        mag = mag + abs(w) * (P @ Vx.abs())
        score = score + abs(w) * le * ((P * (ms + mag_s)) @ Vx.abs())
    return dict(o=_back(o), mag_o=_back(mag), score_o=_back(score))


def ip_model(case, dtype, defect=None):
    """The contract with the documented roundings (module docstring), fp64 between them: o [B N, H dh].  defect: one of DEFECTS --
      joint          one softmax over the text and the image-prompt keys together
      nip_minus      the Nip mask one short: key Nip - 1 dropped
      nip_plus       the Nip mask one long: the repeated row Nip - 1 of the staged tile counted as a key
      scale_both     ip_scale applied to the text part as well
      scale_dropped  ip_scale not applied
      wrong_buffer   the image-prompt scores taken from the other LDS buffer: the last text tile's keys (rows past Nkv repeat row
                     Nkv - 1, as the DMA stages them) under the Nip mask
      sample_stride  k_ip / v_ip of sample b read at row b Nkv instead of b Nip (wrapped into the operand: the model must stay
                     inside its arrays)
      double_c       on a pre-scaled row, the image-prompt scores multiplied by c = scale log2(e) once more"""
    assert defect is None or defect in DEFECTS
    r = lambda x: x.to(dtype).double()
    Q, K, V, K2, V2, c = _operands(case)
    B, H, Nkv, Nip, dh = (case[k] for k in ("B", "H", "Nkv", "Nip", "dh"))
    a1, a2 = 1.0, case["ip_scale"]
    if defect == "nip_minus":
        assert Nip >= 2
        K2, V2 = K2[:, :, :-1], V2[:, :, :-1]
    elif defect == "nip_plus":
        assert Nip < 64
        K2, V2 = torch.cat([K2, K2[:, :, -1:]], 2), torch.cat([V2, V2[:, :, -1:]], 2)
    elif defect == "wrong_buffer":
        idx = ((Nkv - 1) // 64 * 64 + torch.arange(Nip)).clamp_max(Nkv - 1)
        K2 = K[:, :, idx]
    elif defect == "sample_stride":
        idx = (torch.arange(B)[:, None] * Nkv + torch.arange(Nip)[None, :]) % (B * Nip)              # [B, Nip] rows of the flat operand
        flat = lambda x: x.double().cpu().reshape(B * Nip, H, dh)[idx].permute(0, 2, 1, 3)
        K2, V2 = flat(case["k_ip"]), flat(case["v_ip"])
    elif defect == "scale_both":
        a1 = a2
    elif defect == "scale_dropped":
        a2 = 1.0
    S1, S2 = _scores(Q, K, c), _scores(Q, K2, c)
    if defect == "double_c":
        assert case["prescaled"]
        S2 = S2 * c
    if defect == "joint":
        m = torch.maximum(S1.amax(-1, keepdim=True), S2.amax(-1, keepdim=True))
        pu1, pu2 = torch.exp2(S1 - m), torch.exp2(S2 - m)
        l1 = l2 = pu1.sum(-1, keepdim=True) + pu2.sum(-1, keepdim=True)
    else:
        (pu1, l1), (pu2, l2) = _softmax(S1), _softmax(S2)
    if dtype == BF:
        return _back(r(a1 * (r(pu1) @ V) / l1 + r(pu2 * (a2 / l2)) @ V2))
    return _back(r(a1 * (r(pu1) @ V) / l1 + a2 * (r(pu2) @ V2) / l2))


# ------------------------------------------------------------------------------------------------ the gate

def check(got, ref, dtype):
    """The element-wise gate of one output and its rel-L2 gate: attn_ref.gate()'s dict + rel_gate."""
    res = gate(got, ref["o"], ref["mag_o"], U[dtype], C_O[dtype], ref["score_o"])
    res["rel_gate"] = REL_GATES[dtype]["o"]
    return res


def passes(res):
    return res["violations"] == 0 and res["rel"] < res["rel_gate"]


def measure_row(row):
    """(excess of the rounding model on one row: the figure c_o is MARGIN x the maximum of, the case, its reference)."""
    case = make_case(row)
    ref = ip_ref64(case)
    return gate(ip_model(case, row["dtype"]), ref["o"], ref["mag_o"], U[row["dtype"]], 1.0)["excess"], case, ref


def measure_constants(rows=CASES):
    worst = {BF: (0.0, ""), F32: (0.0, "")}
    for row in rows:
        e = measure_row(row)[0]
        if e > worst[row["dtype"]][0]:
            worst[row["dtype"]] = (e, row["name"])
    return worst


if __name__ == "__main__":
    import time
    t0 = time.time()
    for dt, (v, n) in measure_constants().items():
        print(dt, round(v, 3), n)
    print("rows", len(CASES), "seconds", round(time.time() - t0, 1))
