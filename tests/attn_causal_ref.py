"""Reference model, rounding model, gate and case table of the causal attention kernel (csrc/attention_causal.hip; helpers only:
nothing here is collected).  The method is tests/attn_ref.py's, whose gate(), U, REL_GATES, Guarded and padded it reuses.

Contract (include/ctrlora_hip.h: cl_attention_causal_fwd), per sample b and head h, c = scale log2(e):

    S2 = c q k^T (log2 domain),   P = softmax over j <= i of S2 ln 2,   O = P V          (N queries = N keys, d_head 64)

`causal_ref64` evaluates this in fp64 on the operands as stored and returns mag_o = P |V| and the score term of attn_ref:
a score off by delta_ij <= eps ms_ij, eps = (d_head + 2) 2^-24, ms_ij = c sum_d |q_id k_jd| (the fp32 arithmetic of the scores),
moves the normalised P_ij by at most ln 2 P_ij (delta_ij + sum_k P_ik delta_ik):  score_o = ln2 eps (P o (ms + mag_s)) |V|.

`causal_model` is the contract with the roundings the kernel documents and no others: the unnormalised P = 2^(S2 - max) rounded to
the compute type before P V (the denominator is the sum of the UNROUNDED exponentials), O rounded once.

Element-wise gate, zero violations, every case:   |got - ref| <= u |ref| + c_o u mag_o + score_o,   u = 2^-9 (bf16), 2^-24 (fp32)
c_o = MARGIN x the rounding model's worst (|model - ref| - u |ref|) / (u mag_o) over CASES, measured on the CPU by
measure_constants() (`python -m tests.attn_causal_ref` prints it) and written below next to the measured value; MARGIN = 3 as in
attn_ref: it covers what the model keeps exact -- summation order, exp2, the fp32 score and denominator arithmetic.  The rel-L2
gate is REL_GATES[dtype]["o"]: 6e-3 (bf16), 1e-5 (fp32).
"""
import math

import torch

from tests.attn_ref import BF, F32, LOG2E, REL_GATES, U, Guarded, gate, padded  # noqa: F401  (re-exported for the GPU suite)

MARGIN = 3.0
# measured by measure_constants() on the CPU over every row of CASES -- worst rows: bf16 2.143 (bf16-b1h12-n77), fp32 0.686
# (f32-b1h12-n128)                   -> c_o = 3 x:  bf16 6.429   fp32 2.058
MEASURED = {BF: 2.143, F32: 0.686}
C_O = {dt: MARGIN * v for dt, v in MEASURED.items()}

FAM_CAUSAL = 7
DH = 64
NS = (1, 16, 17, 63, 64, 65, 77, 127, 128)   # one key; fragment edge; tile edge; second query block (one full + one diagonal tile);
BHS = ((2, 2), (1, 12))                      # the product's 77; the maximum


def _cases():
    rows = []
    for dt, tag in ((BF, "bf16"), (F32, "f32")):
        for B, H in BHS:
            for N in NS:
                rows.append(dict(name=f"{tag}-b{B}h{H}-n{N}", dtype=dt, B=B, H=H, N=N, q_std=1.0))
        rows.append(dict(name=f"{tag}-b2h2-n77-q4", dtype=dt, B=2, H=2, N=77, q_std=4.0))      # large logits
    return rows


CASES = _cases()


def make_case(row, device="cpu"):
    """Operands of a row, drawn on the CPU from a generator seeded by the row's place in the table, rounded once to its dtype."""
    B, H, N, dt = row["B"], row["H"], row["N"], row["dtype"]
    g = torch.Generator().manual_seed(7000 + [r["name"] for r in CASES].index(row["name"]))
    mk = lambda s=1.0: (torch.randn(B * N, H * DH, generator=g) * s).to(dt).to(device)
    return dict(B=B, H=H, N=N, dh=DH, scale=DH ** -0.5, dtype=dt, q=mk(row["q_std"]), k=mk(), v=mk())


def _split(x, B, N, H):
    return x.double().reshape(B, N, H, DH).permute(0, 2, 1, 3)


def _back(x):
    B, H, N, dh = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * N, H * dh)


def _scores(case, keep=None):
    """(S2 with -inf where the mask drops a key, the mask, Q, K, V, c).  keep: [N, N] bool, default j <= i."""
    B, H, N = case["B"], case["H"], case["N"]
    Q, K, V = (_split(case[n], B, N, H) for n in "qkv")
    c = case["scale"] * LOG2E
    if keep is None:
        keep = torch.ones(N, N, dtype=torch.bool).tril()
    S2 = (torch.einsum("bhid,bhjd->bhij", Q, K) * c).masked_fill(~keep, -math.inf)
    return S2, keep, Q, K, V, c


def causal_ref64(case, keep=None):
    """fp64 o [B N, H dh], mag_o and score_o (module docstring).  keep: another mask, for the tests that show the gate bites."""
    S2, keep, Q, K, V, c = _scores(case, keep)
    pu = torch.exp2(S2 - S2.amax(-1, keepdim=True))
    P = pu / pu.sum(-1, keepdim=True)
    ms = torch.einsum("bhid,bhjd->bhij", Q.abs(), K.abs()) * c
    mag_s = (P * ms).sum(-1, keepdim=True)
    le = math.log(2.0) * (DH + 2) * 2.0 ** -24
    return dict(o=_back(P @ V), mag_o=_back(P @ V.abs()), score_o=_back(le * ((P * (ms + mag_s)) @ V.abs())))


def causal_model(case, dtype):
    """The contract with the documented roundings, fp64 between them."""
    r = lambda x: x.to(dtype).double()
    S2, keep, Q, K, V, c = _scores(case)
    pu = torch.exp2(S2 - S2.amax(-1, keepdim=True))
    return _back(r((r(pu) @ V) / pu.sum(-1, keepdim=True)))


def check(got, ref, dtype):
    """The element-wise gate of one output and its rel-L2 gate: attn_ref.gate()'s dict + rel_gate."""
    res = gate(got, ref["o"], ref["mag_o"], U[dtype], C_O[dtype], ref["score_o"])
    res["rel_gate"] = REL_GATES[dtype]["o"]
    return res


def passes(res):
    return res["violations"] == 0 and res["rel"] < res["rel_gate"]


def measure_row(row):
    case = make_case(row)
    ref = causal_ref64(case)
    return gate(causal_model(case, row["dtype"]), ref["o"], ref["mag_o"], U[row["dtype"]], 1.0)["excess"], case, ref


def measure_constants(rows=CASES):
    worst = {BF: (0.0, ""), F32: (0.0, "")}
    for row in rows:
        e = measure_row(row)[0]
        if e > worst[row["dtype"]][0]:
            worst[row["dtype"]] = (e, row["name"])
    return worst


if __name__ == "__main__":
    for dt, (v, n) in measure_constants().items():
        print(dt, round(v, 3), n)
