"""Contract, rounding model, gates and case table of cl_p_losses_w (helpers only: nothing here is collected).  Shaped like the
p_losses part of tests/ew_ref.py, whose gate, spec / check machinery and measured constant of the "loss" family are reused.

Contract (include/ctrlora_hip.h), evaluated in fp64 on the operands as stored, d = eps - target, per = elements of a sample:

    rho(d)   = d^2                                                     (kind 0, l2)
             = |d| <= delta ? d^2 / 2 : delta (|d| - delta / 2)        (kind 1, Huber = F.huber_loss(reduction='none', delta))
    rho'(d)  = 2 d   |   clamp(d, -delta, delta)
    l_b      = mean over the sample of rho(d)                          per_sample[b] = l_b      (unweighted)
    out      = (mean_b l_b,  mean_b lvlb[t_b] l_b,  w_simple mean_b (wt[t_b] l_b) + w_elbo out[1])
    d_eps    = gscale w_simple wt[t_b] rho'(d) / (per B)               wt == NULL: all ones

Bounds.  They are the forms tests/ew_ref.eval_plosses uses, derived there (sums over n terms: n e sum |terms|) and not measured:
`out` gets (per + 16 + B) e mag, per_sample (per + 16) e l_b, d_eps the element-wise e-based spec (FLOOR + c e |ref|, c the "loss"
family's constant).  One more e is allowed for each extra rounded factor a case brings: the weight (a product with wt[t_b]: in
the finishing sum of out[2], in the coefficient of d_eps) and Huber's branch / clamp (0.5 d^2 or delta (|d| - delta / 2) have one
rounded operation more than d^2; the clamp selects among values that are a rounding apart at |d| = delta).  rho and rho' are
continuous, so an element whose fp32 d falls on the other side of delta than its fp64 d moves the result by no more than the
rounding of d itself.  The rule is zero violations.
"""
import torch

from tests import ew_ref as R

F32 = torch.float32
E, FLOOR = R.E, R.FLOOR
T = 12                               # entries of the weight / lvlb tables of the cases
DELTA = 1.0
PLANT = (1.0, 0.25, -3.0, -1.0)      # d planted where per is small: |d| == delta, inside, outside, |d| == delta
MUTATIONS = ("drop_weight", "weight_on_out0", "huber_no_half_delta", "no_clamp", "no_inv_B")


def rho64(d, kind, delta):
    if kind == 0:
        return d * d, 2 * d
    a = d.abs()
    return torch.where(a <= delta, 0.5 * d * d, delta * (a - 0.5 * delta)), d.clamp(-delta, delta)


def ref_plosses_w(p, ops):
    """fp64: dict(out [3], per_sample [B], d_eps [B, per], mag [3] = the sums of absolute terms behind `out`)."""
    B, per, gs, ws, we = p["B"], p["per"], p["gscale"], p["w_simple"], p["w_elbo"]
    d = ops["eps"].double() - ops["target"].double()
    r, dr = rho64(d, p["kind"], p["delta"])
    sb = r.sum(1) / per
    lw = ops["lvlb"].double()[ops["t"]] if p["lvlb"] else torch.zeros_like(sb)
    w = ops["wt"].double()[ops["t"]] if p["wt"] else torch.ones_like(sb)
    ls, lv, lwt = sb.mean(), (lw * sb).mean(), (w * sb).mean()
    lva = (lw.abs() * sb).mean()
    return dict(out=torch.stack([ls, lv, ws * lwt + we * lv]), mag=torch.stack([ls, lva, abs(ws) * lwt + abs(we) * lva]),
                per_sample=sb, d_eps=gs * ws * w[:, None] * dr / (per * B))


def model_plosses_w(p, ops, mutate=None):
    """The kernel's arithmetic in torch fp32 (one rounding per operation, the kernel's grouping of the factors), or one of
    MUTATIONS of it: what the gate has to reject."""
    assert mutate is None or mutate in MUTATIONS
    B, per, gs, ws, we, kind, delta = p["B"], p["per"], p["gscale"], p["w_simple"], p["w_elbo"], p["kind"], p["delta"]
    f = lambda v: torch.tensor(float(v), dtype=F32)
    d = ops["eps"] - ops["target"]
    if kind == 0:
        r, dr = d * d, d
    else:
        a = d.abs()
        outer = f(delta) * (a if mutate == "huber_no_half_delta" else a - f(0.5) * f(delta))
        r = torch.where(a <= delta, f(0.5) * d * d, outer)
        dr = d if mutate == "no_clamp" else d.clamp(-delta, delta)
    sb = r.sum(1) / per
    lw = ops["lvlb"][ops["t"]] if p["lvlb"] else torch.zeros_like(sb)
    w = ops["wt"][ops["t"]] if p["wt"] and mutate != "drop_weight" else None
    ls, lv = sb.sum() / B, (lw * sb).sum() / B
    lwt = ls if w is None else (w * sb).sum() / B
    out = torch.stack([lwt if mutate == "weight_on_out0" else ls, lv, f(ws) * lwt + f(we) * lv])
    gm = (f(2.0 if kind == 0 else 1.0) * f(gs) * f(ws) / (f(per) * f(1 if mutate == "no_inv_B" else B))).to(d.device)
    g = gm.expand(B) if w is None else gm * w
    return dict(out=out, per_sample=sb, d_eps=dr * g[:, None])


def eval_plosses_w(p, ops, mutate=None):
    """{output: tests/ew_ref.spec} of the outputs the case asks for, `model` being model_plosses_w(mutate)."""
    B, per = p["B"], p["per"]
    ref, model = ref_plosses_w(p, ops), model_plosses_w(p, ops, mutate)
    extra = int(p["wt"]) + int(p["kind"] == 1)
    out = dict(out=R.spec(ref["out"], ref["mag"], (per + 16 + B + extra) * E * ref["mag"], model["out"], E, "loss"))
    if p["per_sample"]:
        sb = ref["per_sample"]
        out["per_sample"] = R.spec(sb, sb, (per + 16 + int(p["kind"] == 1)) * E * sb, model["per_sample"], E, "loss")
    if p["d_eps"]:
        de = ref["d_eps"]
        out["d_eps"] = R.spec(de, de.abs(), FLOOR + extra * E * de.abs(), model["d_eps"], E, "loss")
    return out


# ------------------------------------------------------------------------------------------------ cases

SHAPES = [(B, per) for B in (1, 3, 8) for per in (1, 15, 16, 256, 4099)]


def _cases():
    rows = []
    for kind in (0, 1):
        for wt in (False, True):
            for i, (B, per) in enumerate(SHAPES):
                k = i + 3 * kind + 5 * int(wt)          # every (d_eps, lvlb, per_sample) combination under every (kind, wt)
                rows.append(dict(name=f"plosses_w-{B}x{per}-{'huber' if kind else 'l2'}-{'wt' if wt else 'nowt'}", seed=len(rows),
                                 B=B, per=per, kind=kind, wt=wt, d_eps=bool(k & 1), lvlb=bool(k & 2), per_sample=bool(k & 4),
                                 delta=DELTA, gscale=128.0, w_simple=0.7, w_elbo=0.3))
    return rows


CASES = _cases()
CASE = {c["name"]: c for c in CASES}


def case_t(p):
    """The timesteps of a case: 0, T - 1 and a repeated value, as far as B holds them."""
    B = p["B"]
    if B == 1:
        return torch.tensor([0 if p["seed"] % 2 else T - 1])
    if B == 3:
        return torch.tensor([0, T - 1, 0]) if p["seed"] % 2 else torch.tensor([T - 1, T - 1, 0])
    g = torch.Generator().manual_seed(977 + p["seed"])
    return torch.cat([torch.tensor([0, T - 1, 5, 5]), torch.randint(0, T, (B - 4,), generator=g)])


def make_ops(p, device="cpu"):
    """Standard normal eps / target (drawn on the CPU from a generator seeded by the case).  Where per < 256 elements are planted
    so that d takes PLANT's values exactly: both sides of delta and |d| == delta."""
    g = torch.Generator().manual_seed(4242 + p["seed"])
    B, per = p["B"], p["per"]
    eps, target = torch.randn(B, per, generator=g), torch.randn(B, per, generator=g)
    if per < 256:
        n = min(per, len(PLANT))
        for b in range(B):
            for i in range(n):
                target[b, i] = 0.5
                eps[b, i] = 0.5 + PLANT[(i + b + p["seed"]) % len(PLANT)]
    wt = torch.rand(T, generator=g) * 1.5 + 0.1
    wt[T - 1], wt[5] = 0.0, 1.0
    lvlb = torch.randn(T, generator=g).abs()
    ops = dict(eps=eps, target=target, t=case_t(p), wt=wt, lvlb=lvlb)
    return {k: v.to(device) for k, v in ops.items()}


def huber_shares(p, ops):
    """(share of elements with |d| <= delta, share beyond)."""
    a = (ops["eps"] - ops["target"]).abs()
    inner = float((a <= p["delta"]).float().mean())
    return inner, 1.0 - inner


def min_snr_ref(alphas_cumprod64, gamma):
    """The closed form in fp64 (torch): min(SNR, gamma) / SNR, SNR = acp / (1 - acp)."""
    acp = torch.as_tensor(alphas_cumprod64, dtype=torch.float64)
    snr = acp / (1.0 - acp)
    return torch.minimum(snr, torch.tensor(float(gamma), dtype=torch.float64)) / snr
