"""Contract, rounding model, gates, host-logic transcription and case table of the elementwise / layout conformance suite
(helpers only: nothing here is collected).  Shaped like tests/norm_ref.py and tests/wgrad_ref.py; Guarded / padded / PAD_FILL /
GUARD_ROWS come from tests/gemm_ref.py, MARGIN from tests/attn_ref.py.

Contract (ctrlora_amd/csrc/elementwise.hip, include/ctrlora_hip.h), evaluated in fp64 on the operands AS STORED.  Inputs are normal
numbers or zero: subnormal inputs are not part of the contract (the conversion rows add +-0, +-inf, the largest finite fp32 and exact
ties between bf16 neighbours).

    geglu fwd    out = a gelu(g), (a | g) = the halves of a row of h, gelu(g) = g/2 (1 + erf(g / sqrt 2))
    geglu bwd    da = d gelu(g),  dg = d a (cdf(g) + g pdf(g))
    silu fwd/bwd y = z sigmoid(z),  dx = dy s (1 + z (1 - s))
    axpby        y = a x + b y   (b = 0: y is not read)
    pool2x2      out (+)= the sum of the 2 x 2 block          colsum   out[b, c] += scale sum_p in[b HW + p, c]
    transpose / nchw_to_tok / tok_to_nchw / pack2d / repack / conv_tap_gather / vit_patch_rows: moves with zero fill and ONE rounding
    tok_to_nchw  out = alpha in + beta out   (beta = 0: out is not read)
    softmax_rows p = softmax(scale s) over the N columns of a row
    timestep embedding  (cos | sin)(arg), arg = the fp32 product float(t_b) freqs[k] -- one rounding, reproduced exactly
    qsample      two rounded fp32 products and a rounded sum (bit-exact against torch fp32)
    mse_loss     loss = sum d^2 / n, d_eps = 2 d gscale / n, d = eps - target
    p_losses_mse per_sample_b = mean d_b^2, out = (mean_b, mean_b lvlb[t_b] ., w_simple . + w_elbo .), d_eps = 2 gscale w_simple d / (per B)
    ddim_step    e = u + s (e_c - u); p0 = (x - s1m e) / sqrt a_t; x_prev = sqrt a_prev p0 + sqrt(1 - a_prev - sigma^2) e + sigma noise
    adamw        torch.optim.AdamW, decoupled decay, bias correction, g scaled by grad_scale
    dpmpp_step   e as ddim; m = (x - sigma e) / alpha; hist[i % 3] = m; x_next = cx x + c0 m + c1 hist[(i + 2) % 3] + c2 hist[(i + 1) % 3]
    zero / tick / ddim_set_t / dpm_set_t: byte clear, counter += 1, broadcast of one table entry at a clamped cursor

Two tiers.  EXACT (bit for bit after the single RNE rounding): every pure move, zero, tick, the two set_t, qsample against torch
fp32, and axpby / pool2x2 / colsum / vit_tokens on small integers (every partial sum exact in fp32, every result exact in bf16).
GATED (Gaussian inputs), element-wise with zero violations, e = 2^-24, u = 2^-8 (bf16) or 2^-24 (fp32):

    |got - ref| <= u |ref| + fixed + c e mag

mag = the sum of the absolute values of the terms of the formula (so that cancelling terms are covered).  fixed is derived, first
order, and not measured:
  * erf argument: g 0.70710678f carries two roundings, |erf'(x)| |x| 2e on erf;
  * the fast exponential (tests/norm_ref.py): SiLU |y| e (3 + (|z| + 2)(1 - s)); dSiLU its e_ds; dGELU's pdf = exp(-g^2/2) takes
    (2 t + 3) e relative, t = g^2 / 2 (t rounded, t log2(e) rounded, the hardware exponential to one ulp);
  * FLOOR = 2^-126: results below it flush to zero, and exp(-z) overflows past z = -88.7, where z sigmoid(z) < |z| 2^-128: the
    floor is FLOOR (1 + |z|) on the extreme rows;
  * softmax: the exp2 argument (|s| + |max|) scale log2(e) e per rounding (two: scale log2(e) and the product), of the element and
    of the row's largest such term (through the sum); 2e for the hardware exp2 (one ulp), twice (element and sum); 2e for the
    reciprocal and the product; L e for the sum, L = 4 ceil(N / 1024) + 8 the longest chain of additions; all relative to p;
  * colsum / mse / p_losses sums over n terms: n e sum |terms| (Higham eq. 4.4); colsum adds onto `out` once
    (finishing kernel) or once per pixel chunk (atomics), each a rounding of the running value: adds e (|out| + sum |terms|);
  * ddim: sqrt(1 - a_prev - sigma^2) loses (1 + a_prev + 2 sigma^2) / (1 - a_prev - sigma^2) e / 2 relative;
  * adamw: the bias corrections 1 - beta^step cancel: (beta1^s / bc1 + beta2^s / (2 bc2)) 3e relative on the update term (powf to
    one ulp and the subtraction).
c = MARGIN x the largest value the CPU rounding model (`model` of every evaluate_* below: the same formulas in torch fp32 with the
one output rounding) needs over the table, per family; `python -m tests.ew_ref` measures it.  Nothing is fitted to a kernel's
output.  The timestep embeddings keep the project's own 2e-6 absolute gate (tests/test_gpu_parity.py) plus u |ref| in bf16.
"""
import math

import torch

from tests.attn_ref import MARGIN
from tests.gemm_ref import GUARD_ROWS, PAD_COLS, PAD_FILL, Guarded, padded  # noqa: F401  (re-exported for the GPU suite)
from tests.norm_ref import gate as _gate

BF, F32 = torch.bfloat16, torch.float32
E = 2.0 ** -24
U = {BF: 2.0 ** -8, F32: 2.0 ** -24}
FLOOR = 2.0 ** -126
LOG2E = 1.4426950408889634
TSTEP_ABS = 2e-6
WRAP = 4096 * 256                       # work items one sweep of ew_grid's largest grid covers
WRAP_N = WRAP + 77                      # a wrap row: every thread iterates twice or not, plus a ragged remainder

# Measured by measure_constants() on the CPU over every gated row of CASES: the largest c the rounding model needs, per family,
# and the row that set it.  The gate uses MARGIN x these.
MEASURED = {
    "geglu": 2.034,     # geglu_bwd-257x320 f32 dh
    "silu": 0.0,        # every row passes on its fixed part
    "axpby": 1.376,     # axpby-gauss-257x320 f32 y
    "tok": 0.0,         # exact products, one rounding: u |ref| alone
    "softmax": 0.0,     # every row passes on its fixed part
    "colsum": 0.0,      # every row passes on its fixed part
    "loss": 1.659,      # mse-255-d1 f32 d_eps
    "ddim": 2.293,      # ddim-1000-i19-a1 f32 pred_x0
    "adamw": 1.298,     # adamw-wrap f32 v
    "dpm": 4.471,       # dpmpp_step_dev-wrap f32 x_next (four terms, a quotient inside: seven roundings over 2^20 elements)
}
C_GATE = {k: MARGIN * v for k, v in MEASURED.items()}

EW_IDS = ("none", "geglu_fwd", "geglu_bwd", "silu_fwd", "silu_bwd", "axpby", "transpose", "nchw_to_tok", "tok_to_nchw", "timestep",
          "timestep_f", "qsample", "mse", "plosses", "zero", "conv_tap", "softmax", "ddim_step", "tick", "adamw_dev", "ddim_set_t",
          "ddim_step_dev", "dpmpp_step", "dpmpp_step_dev", "dpm_set_t", "adamw", "pool2x2", "colsum", "repack", "pack2d",
          "vit_patch_rows", "vit_tokens")
EW = {n: i for i, n in enumerate(EW_IDS)}
PROBE_FIELDS = ("id", "dtype", "gx", "gy", "gz", "threads", "form", "aux")


# ------------------------------------------------------------------------------------------------ host logic (transcription)

def ew_grid(nvec, threads=256):
    return min(max((nvec + threads - 1) // threads, 1), 4096)


def wraps(nvec):
    """Does a grid-stride loop over nvec work items iterate twice in some thread?"""
    return nvec > ew_grid(nvec) * 256


def colsum_form(B, HW, C, ws_bytes):
    nchunk = min((HW + 63) // 64, (512 + B - 1) // B)
    ppc = (HW + nchunk - 1) // nchunk
    nchunk = (HW + ppc - 1) // ppc
    c8 = C // 8
    vx = min(256, c8)
    py = 256 // vx
    partial = nchunk > 1 and ws_bytes > 0 and B * nchunk * C * 4 <= ws_bytes
    return dict(nchunk=nchunk, ppc=ppc, VX=vx, PY=py, dead=256 - vx * py, passes=(c8 + vx - 1) // vx, partial=partial,
                want_one=(512 + B - 1) // B == 1)


def zero_form(addr, nbytes):
    head = min((16 - (addr & 15)) & 15, nbytes)
    nvec = (nbytes - head) // 16
    return dict(head=head, nvec=nvec, tail=nbytes - head - nvec * 16, grid=ew_grid(max(nvec, 16)))


def vit_pair(P, S):
    return P % 2 == 0 and S % 2 == 0


def mse_blocks(n):
    return min(ew_grid(n), 256)


def plosses_chunks(per):
    return [(per * c // 16, per * (c + 1) // 16) for c in range(16)]


def tile_grid(rows, cols, batch):
    return ((rows + 63) // 64, (cols + 63) // 64, batch)


def probe(id_, dtype=None, grid=(1, 1, 1), threads=256, form=0, aux=0):
    g = tuple(grid) + (1,) * (3 - len(tuple(grid)))
    return dict(id=EW[id_], dtype=-1 if dtype is None else (0 if dtype == BF else 1), gx=g[0], gy=g[1], gz=g[2], threads=threads,
                form=form, aux=aux)


# ------------------------------------------------------------------------------------------------ gate

def gate(got, ref, fixed, mag, u, c):
    """tests/norm_ref.gate with stat = e mag: dict(violations, err_over_bound, need, rel, first)."""
    ref = ref.double()
    fixed = fixed if torch.is_tensor(fixed) else torch.full_like(ref, float(fixed))
    return _gate(got, ref, fixed.double(), E * mag.double(), u, c)


def spec(ref, mag, fixed, model, u, fam):
    return dict(ref=ref, mag=mag, fixed=fixed, model=model, u=u, fam=fam)


def exact(want):
    return dict(exact=want)


def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


# ------------------------------------------------------------------------------------------------ contract + rounding model
# evaluate_<kernel>(p, dt, ops) -> {output name: spec(...) or exact(...)}; runs on whatever device the operands live on.

SQ2, SQPI = math.sqrt(2.0), math.sqrt(math.pi)


def _gelu_parts(g):
    x = g / SQ2
    erf = torch.erf(x)
    pdf = torch.exp(-0.5 * g * g) / math.sqrt(2 * math.pi)
    earg = (2 / SQPI) * torch.exp(-x * x) * x.abs() * 2 * E          # error of erf through its argument's two roundings
    return erf, pdf, earg


def _gelu32(g):
    return 0.5 * g * (1.0 + torch.erf(g * 0.70710678118654752440))


def eval_geglu_fwd(p, dt, ops):
    F = p["F"]
    h = ops["h"]
    a, g = h[:, :F].double(), h[:, F:].double()
    erf, _, earg = _gelu_parts(g)
    ref = a * 0.5 * g * (1 + erf)
    mag = a.abs() * 0.5 * g.abs() * (1 + erf.abs())
    fixed = a.abs() * 0.5 * g.abs() * earg + FLOOR
    a32, g32 = h[:, :F].float(), h[:, F:].float()
    return dict(out=spec(ref, mag, fixed, (a32 * _gelu32(g32)).to(dt), U[dt], "geglu"))


def eval_geglu_bwd(p, dt, ops):
    F = p["F"]
    h, d = ops["h"], ops["dout"].double()
    a, g = h[:, :F].double(), h[:, F:].double()
    erf, pdf, earg = _gelu_parts(g)
    gel_mag = 0.5 * g.abs() * (1 + erf.abs())
    da = d * 0.5 * g * (1 + erf)
    dg = d * a * (0.5 * (1 + erf) + g * pdf)
    t = 0.5 * g * g
    da_s = (d.abs() * gel_mag, d.abs() * 0.5 * g.abs() * earg + FLOOR)
    dg_s = ((d * a).abs() * (0.5 * (1 + erf.abs()) + g.abs() * pdf),
            (d * a).abs() * (0.5 * earg + g.abs() * pdf * (2 * t + 3) * E) + FLOOR * (1 + (d * a * g).abs()))
    a32, g32, d32 = h[:, :F].float(), h[:, F:].float(), ops["dout"].float()
    cdf32 = 0.5 * (1.0 + torch.erf(g32 * 0.70710678118654752440))
    pdf32 = 0.39894228040143267794 * torch.exp(-0.5 * g32 * g32)
    model = torch.cat([d32 * _gelu32(g32), d32 * a32 * (cdf32 + g32 * pdf32)], 1).to(dt)
    return dict(dh=spec(torch.cat([da, dg], 1), torch.cat([da_s[0], dg_s[0]], 1), torch.cat([da_s[1], dg_s[1]], 1), model, U[dt], "geglu"))


def _sig_parts(z):
    s = torch.sigmoid(z)
    t = torch.sigmoid(-z)                    # 1 - s without cancellation
    return s, t


def eval_silu_fwd(p, dt, ops):
    z = ops["x"].double()
    s, t = _sig_parts(z)
    y = z * s
    fixed = y.abs() * E * (3 + (z.abs() + 2) * t) + FLOOR * (1 + z.abs())
    z32 = ops["x"].float()
    return dict(y=spec(y, y.abs(), fixed, (z32 / (1.0 + torch.exp(-z32))).to(dt), U[dt], "silu"))


def eval_silu_bwd(p, dt, ops):
    z, dy = ops["x"].double(), ops["dy"].double()
    s, t = _sig_parts(z)
    ds = s * (1 + z * t)
    za = z.abs()
    rs_ = ((za + 2) * t + 2) * E                                       # relative error of the fp32 sigmoid (tests/norm_ref.py)
    e_ds = s * (rs_ * (1 + za * t + za * s) + E * (za + 3 * (1 + za * t)))
    mag = dy.abs() * s * (1 + za * t)
    fixed = dy.abs() * e_ds + FLOOR * (1 + za) * (1 + dy.abs())
    z32, d32 = ops["x"].float(), ops["dy"].float()
    s32 = 1.0 / (1.0 + torch.exp(-z32))
    return dict(dx=spec(dy * ds, mag, fixed, (d32 * (s32 * (1.0 + z32 * (1.0 - s32)))).to(dt), U[dt], "silu"))


def eval_axpby(p, dt, ops):
    a, b = p["a"], p["b"]
    x32 = ops["x"].float()
    if b == 0.0:
        m32 = torch.tensor(a, dtype=F32, device=x32.device) * x32
        ref, mag = a * ops["x"].double(), (a * ops["x"].double()).abs()
    else:
        y32 = ops["y"].float()
        m32 = torch.tensor(a, dtype=F32, device=x32.device) * x32 + torch.tensor(b, dtype=F32, device=x32.device) * y32
        ref = a * ops["x"].double() + b * ops["y"].double()
        mag = (a * ops["x"].double()).abs() + (b * ops["y"].double()).abs()
    if p["ints"]:
        return dict(y=exact(ref.to(dt)))
    return dict(y=spec(ref, mag, 0.0, m32.to(dt), U[dt], "axpby"))


def eval_pool2x2(p, dt, ops):
    B, H, W, C = p["B"], p["H"], p["W"], p["C"]
    x = ops["in"].double().reshape(B, H, 2, W, 2, C)
    s = x.sum((2, 4)).reshape(B * H * W, C)
    if p["acc"]:
        s = s + ops["out0"].double()
    return dict(out=exact(s.to(dt)))


def conv_tap_index(p):
    """(source row or -1) of every output row of conv_tap_gather."""
    B, Hin, Win, Hout, Wout, tap, stride, pad = (p[k] for k in ("B", "Hin", "Win", "Hout", "Wout", "tap", "stride", "pad"))
    ky, kx = tap // 3, tap % 3
    m = torch.arange(B * Hout * Wout)
    ox, oy, ob = m % Wout, (m // Wout) % Hout, m // (Wout * Hout)
    iy, ix = oy * stride + ky - pad, ox * stride + kx - pad
    ok = (iy >= 0) & (iy < Hin) & (ix >= 0) & (ix < Win)
    return torch.where(ok, (ob * Hin + iy) * Win + ix, torch.full_like(m, -1))


def eval_conv_tap(p, dt, ops):
    idx = conv_tap_index(p).to(ops["x"].device)
    out = ops["x"][idx.clamp_min(0)] * (idx >= 0).to(dt)[:, None]
    return dict(out=exact(out + 0.0))                                  # (-0 x 0 -> +0 is not wanted: a skipped row is +0)


def eval_vit_patch_rows(p, dt, ops):
    B, C, S, P, Kpad = (p[k] for k in ("B", "C", "S", "P", "Kpad"))
    G = S // P
    px = ops["px"].reshape(B, C, G, P, G, P).permute(0, 2, 4, 1, 3, 5).reshape(B * G * G, C * P * P)
    out = torch.zeros(B * G * G, Kpad, dtype=dt, device=px.device)
    out[:, :C * P * P] = px.to(dt)
    return dict(out=exact(out))


def eval_vit_tokens(p, dt, ops):
    B, T, D = p["B"], p["T"], p["D"]
    patch = ops["patch"].float().reshape(B, T - 1, D)
    tok = torch.cat([ops["cls"].reshape(1, 1, D).expand(B, 1, D), patch], 1) + ops["pos"][None]
    return dict(out=exact(tok.reshape(B * T, D).to(dt)))


def eval_transpose(p, dt, ops):
    Bt, R, C, Rpad = p["Bt"], p["R"], p["C"], p["Rpad"]
    out = torch.zeros(Bt, C, Rpad, dtype=p["odt"], device=ops["in"].device)
    out[:, :, :R] = ops["in"].permute(0, 2, 1).to(p["odt"])
    return dict(out=exact(out))


def eval_nchw_to_tok(p, dt, ops):
    B, Cin, Cpad, HW = p["B"], p["Cin"], p["Cpad"], p["HW"]
    out = torch.zeros(B * HW, Cpad, dtype=dt, device=ops["in"].device)
    out[:, :Cin] = ops["in"].permute(0, 2, 1).reshape(B * HW, Cin).to(dt)
    return dict(out=exact(out))


def eval_tok_to_nchw(p, dt, ops):
    B, C, HW, al, be = p["B"], p["C"], p["HW"], p["alpha"], p["beta"]
    x = ops["in"].reshape(B, HW, C).permute(0, 2, 1)
    if be == 0.0 and al == 1.0:
        return dict(out=exact(x.float().contiguous()))
    ref = al * x.double() + be * ops["out0"].double()
    mag = (al * x.double()).abs() + (be * ops["out0"].double()).abs()
    return dict(out=spec(ref, mag, 0.0, (al * x.float() + be * ops["out0"]).contiguous(), E, "tok"))


def eval_pack2d(p, dt, ops):
    R, C, Cpad = p["R"], p["C"], p["Cpad"]
    out = torch.zeros(R, Cpad, dtype=dt, device=ops["in"].device)
    out[:, :C] = ops["in"].to(dt)
    return dict(out=exact(out))


def eval_repack(p, dt, ops):
    outs = {}
    for i, m in enumerate(p["mats"]):
        outs[f"dst{i}"] = exact(ops[f"src{i}"].to(dt))
        if m["T"]:
            outs[f"dstT{i}"] = exact(ops[f"src{i}"].t().contiguous().to(dt))
    return outs


def softmax_chain(N):
    return 4 * ((N + 1023) // 1024) + 8


def eval_softmax(p, dt, ops):
    N, scale = p["N"], p["scale"]
    s = ops["S"].double()
    pr = torch.softmax(s * scale, 1)
    mx = s.max(1, keepdim=True).values
    arg = (s.abs() + mx.abs()) * scale * LOG2E * E * 2
    fixed = pr * (arg + arg.max(1, keepdim=True).values + 6 * E + softmax_chain(N) * E) + FLOOR
    s32 = ops["S"]
    sl2 = torch.tensor(scale, dtype=F32, device=s32.device) * 1.4426950408889634
    ex = torch.exp2(s32 * sl2 - s32.max(1, keepdim=True).values * sl2)
    model = (ex * (1.0 / ex.sum(1, keepdim=True))).to(dt)
    return dict(P=spec(pr, pr, fixed, model, U[dt], "softmax"))


def eval_colsum(p, dt, ops):
    B, HW, C, scale = p["B"], p["HW"], p["C"], p["scale"]
    x = ops["in"].double().reshape(B, HW, C)
    ref = ops["out0"].double() + scale * x.sum(1)
    if p["ints"]:
        return dict(out=exact(ref.float()))
    mabs = abs(scale) * x.abs().sum(1)
    model = ops["out0"] + scale * ops["in"].float().reshape(B, HW, C).sum(1)
    f = colsum_form(B, HW, C, (64 << 20) if p["ws"] else 0)
    adds = 1 if f["partial"] else f["nchunk"]
    mag = ops["out0"].double().abs() + mabs
    return dict(out=spec(ref, mag, (HW + 2) * E * mabs + adds * E * mag, model, E, "colsum"))


def eval_mse(p, dt, ops):
    n, gs = p["n"], p["gscale"]
    d = ops["eps"].double() - ops["target"].double()
    loss = (d * d).sum() / n
    d32 = ops["eps"] - ops["target"]
    inv = torch.tensor(1.0, dtype=F32, device=d32.device) / n
    out = dict(loss=spec(loss.reshape(1), loss.reshape(1), ((n + 256) * E * loss).reshape(1), ((d32 * d32).sum() * inv).reshape(1), E, "loss"))
    if p["d_eps"]:
        ref = 2 * d * gs / n
        out["d_eps"] = spec(ref, ref.abs(), FLOOR, 2.0 * d32 * inv * gs, E, "loss")
    return out


def eval_plosses(p, dt, ops):
    B, per, gs, ws, we = p["B"], p["per"], p["gscale"], p["w_simple"], p["w_elbo"]
    d = ops["eps"].double() - ops["target"].double()
    sb = (d * d).sum(1) / per
    lw = ops["lvlb"].double()[ops["t"]] if p["lvlb"] else torch.zeros_like(sb)
    ls, lv = sb.mean(), (lw * sb).mean()
    ref = torch.stack([ls, lv, ws * ls + we * lv])
    mag = torch.stack([ls, (lw.abs() * sb).mean(), abs(ws) * ls + abs(we) * (lw.abs() * sb).mean()])
    d32 = ops["eps"] - ops["target"]
    sb32 = (d32 * d32).sum(1) / per
    lw32 = ops["lvlb"][ops["t"]] if p["lvlb"] else torch.zeros_like(sb32)
    ls32, lv32 = sb32.sum() / B, (lw32 * sb32).sum() / B
    out = dict(out=spec(ref, mag, (per + 16 + B) * E * mag, torch.stack([ls32, lv32, ws * ls32 + we * lv32]), E, "loss"))
    if p["per_sample"]:
        out["per_sample"] = spec(sb, sb, (per + 16) * E * sb, sb32, E, "loss")
    if p["d_eps"]:
        gm = 2 * gs * ws / (per * B)
        gm32 = torch.tensor(2.0 * gs, dtype=F32) * torch.tensor(ws, dtype=F32) / (torch.tensor(float(per), dtype=F32) * torch.tensor(float(B), dtype=F32))
        out["d_eps"] = spec(d * gm, (d * gm).abs(), FLOOR, d32 * gm32.to(d32.device), E, "loss")
    return out


def make_freqs(half):
    return torch.exp(-math.log(10000.0) * torch.arange(0, half, dtype=F32) / half)


def eval_timestep(p, dt, ops):
    """ref of both variants; `model` is torch's fp32 cos / sin of the same fp32 argument."""
    t = ops["t"].float()
    arg = t[:, None] * ops["freqs"][None]                              # ONE fp32 rounding, as the kernels and the reference form it
    ref = torch.cat([torch.cos(arg.double()), torch.sin(arg.double())], 1)
    model = torch.cat([torch.cos(arg), torch.sin(arg)], 1).to(dt)
    return dict(out=dict(ref=ref, mag=torch.zeros_like(ref), fixed=torch.full_like(ref, TSTEP_ABS), model=model,
                         u=U[dt] if dt == BF else 0.0, fam=None))


def eval_qsample(p, dt, ops):
    B, per = p["B"], p["per"]
    a = ops["sqrt_ac"][ops["t"]].reshape(B, 1)
    b = ops["sqrt_1mac"][ops["t"]].reshape(B, 1)
    return dict(out=exact(a * ops["z"] + b * ops["noise"]))


def ddim_table(S=20, eta=0.5):
    """[S][4] fp32 = {a_t, a_prev, sigma_t, sqrt(1 - a_t)}: the linear-beta DDPM schedule sampled uniformly, as the sampler builds it."""
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2
    ac = torch.cumprod(1 - betas, 0).float().double()
    ts = torch.arange(0, 1000, 1000 // S) + 1
    a = ac[ts]
    ap = torch.cat([ac[:1], ac[ts[:-1]]])
    sig = eta * torch.sqrt((1 - ap) / (1 - a) * (1 - a / ap))
    return torch.stack([a, ap, sig, torch.sqrt(1 - a)], 1).float(), ts


def eval_ddim(p, dt, ops):
    row = ops["coef"][p["index"]]
    a_t, a_p, sg, s1m = (float(v) for v in row)
    x, ec = ops["x"].double(), ops["e_c"].double()
    if p["e_u"]:
        u, sc = ops["e_u"].double(), p["scale"]
        e, me = u + sc * (ec - u), u.abs() + abs(sc) * (ec.abs() + u.abs())
    else:
        e, me = ec, ec.abs()
    sat, sap, rad = math.sqrt(a_t), math.sqrt(a_p), 1 - a_p - sg * sg
    dr = math.sqrt(rad)
    p0 = (x - s1m * e) / sat
    mp0 = (x.abs() + s1m * me) / sat
    xp, mxp = sap * p0 + dr * e, sap * mp0 + dr * me
    fixed = e.abs() * dr * 0.5 * E * (1 + a_p + 2 * sg * sg) / rad + FLOOR
    f = lambda v: torch.tensor(v, dtype=F32, device=x.device)
    x32, e32 = ops["x"], ops["e_c"]
    if p["e_u"]:
        e32 = ops["e_u"] + f(p["scale"]) * (e32 - ops["e_u"])
    p032 = (x32 - f(s1m) * e32) / torch.sqrt(f(a_t))
    xp32 = torch.sqrt(f(a_p)) * p032 + torch.sqrt(f(1.0) - f(a_p) - f(sg) * f(sg)) * e32
    if p["noise"]:
        xp, mxp = xp + sg * ops["noise"].double(), mxp + sg * ops["noise"].double().abs()
        xp32 = xp32 + f(sg) * ops["noise"]
    out = dict(x_prev=spec(xp, mxp, fixed, xp32, E, "ddim"))
    if p["pred_x0"]:
        out["pred_x0"] = spec(p0, mp0, FLOOR, p032, E, "ddim")
    return out


ADAMW_HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-2, gscale=1.0 / 128)


def eval_adamw_step(state, g, step, device=None):
    """One AdamW step from `state` = (p, m, v) as stored (fp32): {p, m, v: spec}."""
    f32 = lambda v: float(torch.tensor(v, dtype=F32))
    lr, b1, b2, eps, wd, gs = (f32(ADAMW_HYPER[k]) for k in ("lr", "beta1", "beta2", "eps", "wd", "gscale"))
    p, m, v = (t.double() for t in state)
    gi = g.double() * gs
    m1, mm1 = b1 * m + (1 - b1) * gi, b1 * m.abs() + (1 - b1) * gi.abs()
    v1 = b2 * v + (1 - b2) * gi * gi
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    den = v1.sqrt() / math.sqrt(bc2) + eps
    upd = (lr / bc1) * m1 / den
    p1 = p * (1 - lr * wd) - upd
    mupd = (lr / bc1) * mm1 / den
    fixed = mupd * (b1 ** step / bc1 + 0.5 * b2 ** step / bc2) * 3 * E + FLOOR
    t = lambda x: torch.tensor(x, dtype=F32, device=g.device)
    p32, m32, v32 = state
    g32 = g * t(gs)
    pm = p32 * (t(1.0) - t(lr) * t(wd))
    mo = t(b1) * m32 + (t(1.0) - t(b1)) * g32
    vo = t(b2) * v32 + (t(1.0) - t(b2)) * g32 * g32
    bc1f = t(1.0) - torch.pow(t(b1), t(float(step)))
    bc2s = torch.sqrt(t(1.0) - torch.pow(t(b2), t(float(step))))
    pm = pm - (t(lr) / bc1f) * mo / (torch.sqrt(vo) / bc2s + t(eps))
    return dict(p=spec(p1, p.abs() * (1 + lr * wd) + mupd, fixed, pm, E, "adamw"),
                m=spec(m1, mm1, FLOOR, mo, E, "adamw"), v=spec(v1, v1, FLOOR, vo, E, "adamw"))


def clamp_ddim(S, cursor):
    return max(0, S - 1 - cursor)


def clamp_dpm(S, cursor):
    return min(max(cursor, 0), S - 1)


def dpm_table(S=20):
    """[S][8] fp32 = {alpha, sigma, cx, c0, c1, c2, t_in, 0}: alpha / sigma of the linear-beta schedule on a uniform grid; the update
    coefficients are plain numbers of the size the solver's are (orders 1, 2, 3, 3, ...: c1 = 0 in row 0, c2 = 0 in rows 0 and 1)."""
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2
    ac = torch.cumprod(1 - betas, 0)
    t = 999 - torch.arange(S) * (1000 // S)
    i = torch.arange(S, dtype=torch.float64)
    tab = torch.zeros(S, 8, dtype=torch.float64)
    tab[:, 0], tab[:, 1] = ac[t].sqrt(), (1 - ac[t]).sqrt()
    tab[:, 2], tab[:, 3] = 0.9 - 0.01 * i, 0.25 + 0.02 * i
    tab[1:, 4] = -0.12 - 0.003 * i[1:]
    tab[2:, 5] = 0.03 + 0.001 * i[2:]
    tab[:, 6] = t.double() - 0.05 * i
    return tab.float()


def eval_dpmpp(p, dt, ops):
    """The fp64 restatement of one step (tests/test_gpu_dpm_solver.py: _step64) with the parts of its bound."""
    i = p["index"]
    alpha, sigma, cx, c0, c1, c2 = (float(v) for v in ops["coef"][i, :6])
    sc = float(torch.tensor(p["scale"], dtype=F32))
    x, ec, u = ops["x"].double(), ops["e_c"].double(), ops["e_u"].double()
    h1, h2 = ops["hist"][(i + 2) % 3].double(), ops["hist"][(i + 1) % 3].double()
    e, me = u + sc * (ec - u), u.abs() + abs(sc) * (ec.abs() + u.abs())
    m, mm = (x - sigma * e) / alpha, (x.abs() + sigma * me) / alpha
    xn = cx * x + c0 * m + c1 * h1 + c2 * h2
    mxn = (cx * x).abs() + abs(c0) * mm + (c1 * h1).abs() + (c2 * h2).abs()
    f = lambda v: torch.tensor(v, dtype=F32, device=x.device)
    e32 = ops["e_u"] + f(sc) * (ops["e_c"] - ops["e_u"])
    m32 = (ops["x"] - f(sigma) * e32) / f(alpha)
    xn32 = f(cx) * ops["x"] + f(c0) * m32 + f(c1) * ops["hist"][(i + 2) % 3] + f(c2) * ops["hist"][(i + 1) % 3]
    return dict(x_next=spec(xn, mxn, FLOOR, xn32, E, "dpm"), pred_x0=spec(m, mm, FLOOR, m32, E, "dpm"), hist_slot=spec(m, mm, FLOOR, m32, E, "dpm"))


EVAL = dict(dpmpp_step=eval_dpmpp, dpmpp_step_dev=eval_dpmpp, geglu_fwd=eval_geglu_fwd, geglu_bwd=eval_geglu_bwd, silu_fwd=eval_silu_fwd, silu_bwd=eval_silu_bwd, axpby=eval_axpby,
            pool2x2=eval_pool2x2, conv_tap=eval_conv_tap, vit_patch_rows=eval_vit_patch_rows, vit_tokens=eval_vit_tokens,
            transpose=eval_transpose, nchw_to_tok=eval_nchw_to_tok, tok_to_nchw=eval_tok_to_nchw, pack2d=eval_pack2d, repack=eval_repack,
            softmax=eval_softmax, colsum=eval_colsum, mse=eval_mse, plosses=eval_plosses, timestep=eval_timestep, qsample=eval_qsample,
            ddim_step=eval_ddim)


# ------------------------------------------------------------------------------------------------ the case table
# A row: name, kern, p (the call's parameters), dtypes, tags (the forms it was written for; asserted when the table is built).

def _row(name, kern, dtypes=(BF, F32), tags=(), **p):
    return dict(name=name, kern=kern, dtypes=tuple(dtypes), tags=set(tags), p=p)


SPECIALS_F32 = [0.0, -0.0, math.inf, -math.inf, 3.4028234663852886e38, -3.4028234663852886e38,
                1.00390625, 1.01171875, -1.00390625, 257.0, 259.0, 1.0 + 2.0 ** -8 + 2.0 ** -20]
# 1.00390625 = 1 + 2^-8: the tie between bf16 1.0 and 1.0078125 (even: down); 1.01171875 = 1 + 3 2^-8: tie, even is UP
# (1.015625); 257 / 259: ties at the 2^8 binade (256 / 260); the last one lies just above a tie (up)


def _cases():
    rows = []
    # ---- vector-8 row kernels
    for Wd in (8, 24, 320):
        for M in (1, 3, 257):
            rows.append(_row(f"geglu_fwd-{M}x{Wd}", "geglu_fwd", M=M, F=Wd))
            rows.append(_row(f"geglu_bwd-{M}x{Wd}", "geglu_bwd", M=M, F=Wd))
            rows.append(_row(f"silu_fwd-{M}x{Wd}", "silu_fwd", M=M, C=Wd))
            rows.append(_row(f"silu_bwd-{M}x{Wd}", "silu_bwd", M=M, C=Wd))
            rows.append(_row(f"axpby-b0-{M}x{Wd}", "axpby", M=M, C=Wd, a=2.0, b=0.0, ints=True, tags={"b0_nan"}))
            rows.append(_row(f"axpby-inplace-{M}x{Wd}", "axpby", M=M, C=Wd, a=2.0, b=-3.0, ints=True, tags={"inplace"}))
            B, H, W = {1: (1, 1, 1), 3: (3, 1, 1), 257: (1, 257, 1)}[M]
            rows.append(_row(f"pool-set-{M}x{Wd}", "pool2x2", B=B, H=H, W=W, C=Wd, acc=0, tags={"acc0_nan"}))
            rows.append(_row(f"pool-acc-{M}x{Wd}", "pool2x2", B=B, H=H, W=W, C=Wd, acc=1, tags={"acc1"}))
    rows.append(_row("axpby-gauss-3x24", "axpby", M=3, C=24, a=0.7, b=-1.3, ints=False, tags={"inplace"}))
    rows.append(_row("axpby-gauss-257x320", "axpby", M=257, C=320, a=0.7, b=-1.3, ints=False, tags={"inplace"}))
    rows.append(_row("pool-set-2x3x2x24", "pool2x2", B=2, H=3, W=2, C=24, acc=0))
    for stride in (1, 2):
        for tap in range(9):
            Hin, Win = 5, 4
            rows.append(_row(f"tap{tap}-s{stride}", "conv_tap", B=2, Hin=Hin, Win=Win, Hout=(Hin - 1) // stride + 1,
                             Wout=(Win - 1) // stride + 1, C=24 if tap % 2 else 8, tap=tap, stride=stride, pad=1))
    rows.append(_row("vit_tokens-2x3x24", "vit_tokens", B=2, T=3, D=24))
    rows.append(_row("vit_tokens-1x5x8", "vit_tokens", B=1, T=5, D=8))
    rows.append(_row("vit_patch-pair", "vit_patch_rows", B=2, C=3, S=8, P=4, Kpad=56, tags={"pair"}))
    rows.append(_row("vit_patch-nopair", "vit_patch_rows", B=1, C=1, S=9, P=3, Kpad=16, tags={"nopair"}))
    # one wrap row per kernel, bf16 only
    wr = dict(dtypes=(BF,), tags={"wrap"})
    rows += [_row("geglu_fwd-wrap", "geglu_fwd", M=WRAP_N, F=8, **wr), _row("geglu_bwd-wrap", "geglu_bwd", M=WRAP_N, F=8, **wr),
             _row("silu_fwd-wrap", "silu_fwd", M=WRAP_N, C=8, **wr), _row("silu_bwd-wrap", "silu_bwd", M=WRAP_N, C=8, **wr),
             _row("axpby-wrap", "axpby", M=WRAP_N, C=8, a=2.0, b=-3.0, ints=True, **wr),
             _row("pool-wrap", "pool2x2", B=1, H=WRAP_N, W=1, C=8, acc=0, **wr),
             _row("tap-wrap", "conv_tap", B=1, Hin=WRAP_N, Win=1, Hout=WRAP_N, Wout=1, C=8, tap=1, stride=1, pad=1, **wr),
             _row("vit_tokens-wrap", "vit_tokens", B=1, T=WRAP_N, D=8, **wr),
             _row("vit_patch-wrap", "vit_patch_rows", B=1, C=1, S=2050, P=2, Kpad=8, **wr)]
    # ---- 64-tile kernels
    shapes = [(1, 1, 1, 1), (63, 65, 64, 3), (64, 64, 64, 1), (65, 63, 72, 3), (130, 1, 136, 1), (1, 130, 8, 3), (130, 130, 130, 1),
              (60, 5, 128, 3), (63, 64, 63, 1)]
    for R, C, Rpad, Bt in shapes:
        for idt, odt, tg in ((F32, BF, "f32bf16"), (F32, F32, "f32f32"), (BF, BF, "bf16bf16")):
            rows.append(_row(f"transpose-{tg}-{Bt}x{R}x{C}-pad{Rpad}", "transpose", dtypes=(odt,), Bt=Bt, R=R, C=C, Rpad=Rpad, idt=idt, odt=odt,
                             tags={"empty_tile"} if (Rpad + 63) // 64 > (R + 63) // 64 else set()))
    for Cin, HW, Cpad, B in shapes:
        rows.append(_row(f"nchw_to_tok-{B}x{Cin}x{HW}-pad{Cpad}", "nchw_to_tok", B=B, Cin=Cin, Cpad=Cpad, HW=HW,
                         tags={"empty_tile"} if (Cpad + 63) // 64 > (Cin + 63) // 64 else set()))
        rows.append(_row(f"tok_to_nchw-set-{B}x{Cin}x{HW}", "tok_to_nchw", B=B, C=Cin, HW=HW, alpha=1.0, beta=0.0, tags={"beta0_nan"}))
        rows.append(_row(f"tok_to_nchw-acc-{B}x{Cin}x{HW}", "tok_to_nchw", B=B, C=Cin, HW=HW, alpha=0.5, beta=2.0))
    # ---- repack / pack2d
    mats = [dict(R=1, C=1, T=True, sld=0), dict(R=31, C=33, T=True, sld=40), dict(R=32, C=32, T=False, sld=0), dict(R=33, C=31, T=True, sld=0),
            dict(R=64, C=8, T=False, sld=11), dict(R=320, C=128, T=True, sld=0)]
    rows.append(_row("repack-6", "repack", mats=mats))
    for R in (1, 77):
        for C, Cpad in ((7, 7), (7, 12), (320, 320), (320, 325)):
            rows.append(_row(f"pack2d-{R}x{C}-pad{Cpad}", "pack2d", R=R, C=C, Cpad=Cpad))
    # ---- softmax_rows
    for N in (4, 252, 1020, 1024, 1028, 4096, 8192):
        for M in (1, 5):
            for scale in (1.0, 512.0 ** -0.5):
                rows.append(_row(f"softmax-{M}x{N}-s{scale:.3f}", "softmax", M=M, N=N, scale=scale))
    # ---- colsum: every shape with and without a workspace, integers (exact) and Gaussian (gated)
    for B, HW, C in ((1, 1, 8), (2, 50, 64), (3, 63, 24), (3, 64, 24), (3, 65, 24), (1, 5000, 320), (600, 3, 8), (2, 70, 2056)):
        for ws in (True, False):
            for ints in (True, False):
                rows.append(_row(f"colsum-{B}x{HW}x{C}-ws{int(ws)}-{'int' if ints else 'gauss'}", "colsum", B=B, HW=HW, C=C, ws=ws,
                                 ints=ints, scale=0.5))
    # ---- losses
    k = 0
    for per in (1, 15, 16, 17, 4117, 16384):
        for B in (1, 3):
            rows.append(_row(f"plosses-{B}x{per}", "plosses", dtypes=(F32,), B=B, per=per, d_eps=bool(k & 1), lvlb=bool(k & 2),
                             per_sample=bool(k & 4) != bool(k & 1), gscale=128.0, w_simple=0.7, w_elbo=0.3))
            k += 1
    for i, n in enumerate((1, 255, 1280, 65536 + 300)):
        for d in (False, True):
            rows.append(_row(f"mse-{n}-d{int(d)}", "mse", dtypes=(F32,), n=n, d_eps=d, gscale=128.0))
    # ---- zero: one row per byte count, each at pointer offsets 0 .. 15
    for nb in (0, 1, 15, 16, 17, 31, 33, 4101):
        rows.append(_row(f"zero-{nb}", "zero", dtypes=(None,), nbytes=nb))
    rows.append(_row("zero-wrap", "zero", dtypes=(None,), nbytes=(WRAP_N) * 16 + 5, tags={"wrap"}))
    # ---- timestep embeddings
    for B in (1, 5):
        for half in (1, 160, 257):
            rows.append(_row(f"timestep-{B}x{half}", "timestep", B=B, half=half))
    # ---- samplers / optimizer / cursors
    for B, per in ((1, 1), (3, 1000)):
        rows.append(_row(f"qsample-{B}x{per}", "qsample", dtypes=(F32,), B=B, per=per))
    k = 0
    for n in (1, 1000):
        for index in (0, 19):
            for alias in (False, True):
                rows.append(_row(f"ddim-{n}-i{index}-a{int(alias)}", "ddim_step", dtypes=(F32,), n=n, index=index, S=20, alias=alias, scale=7.5,
                                 e_u=bool(k & 1), noise=bool(k & 2), pred_x0=bool(k & 4)))
                k += 3
    for n in (1, 1000):
        rows.append(_row(f"adamw-{n}", "adamw", dtypes=(F32,), n=n))
    rows.append(_row("adamw-wrap", "adamw", dtypes=(F32,), n=WRAP_N, tags={"wrap"}))
    for n in (1, 300):
        rows.append(_row(f"cursors-{n}", "cursors", dtypes=(None,), n=n, S=20))
    # ---- DPM-Solver++: one wrap row per entry point (their own tests hold the orders, the ring and the skipped slots at small n)
    for k in ("dpmpp_step", "dpmpp_step_dev"):
        rows.append(_row(f"{k}-wrap", k, dtypes=(F32,), n=WRAP_N, index=4, S=20, scale=7.5, tags={"wrap"}))
    for r in rows:
        _assert_row(r)
    return rows


def work_items(row):
    """Work items of the row's grid-stride loop (None: the kernel has no such loop)."""
    k, p = row["kern"], row["p"]
    if k in ("geglu_fwd", "geglu_bwd"):
        return p["M"] * (p["F"] // 8)
    if k in ("silu_fwd", "silu_bwd", "axpby"):
        return p["M"] * (p["C"] // 8)
    if k == "pool2x2":
        return p["B"] * p["H"] * p["W"] * (p["C"] // 8)
    if k == "conv_tap":
        return p["B"] * p["Hout"] * p["Wout"] * (p["C"] // 8)
    if k == "vit_tokens":
        return p["B"] * p["T"] * (p["D"] // 8)
    if k == "vit_patch_rows":
        return p["B"] * (p["S"] // p["P"]) ** 2 * (p["Kpad"] // 8)
    if k == "pack2d":
        return p["R"] * p["Cpad"]
    if k == "adamw":
        return p["n"]
    if k in ("ddim_step", "dpmpp_step", "dpmpp_step_dev"):
        return p["n"]
    if k == "qsample":
        return p["B"] * p["per"]
    if k == "zero":
        return zero_form(0, p["nbytes"])["nvec"]
    return None


def _assert_row(row):
    n = work_items(row)
    if n is not None:
        assert wraps(n) == ("wrap" in row["tags"]), (row["name"], n)
    p = row["p"]
    if row["kern"] == "vit_patch_rows" and "wrap" not in row["tags"]:
        assert vit_pair(p["P"], p["S"]) == ("pair" in row["tags"]), row["name"]


def covered_forms(rows=None):
    """The set of forms the table reaches, as tuples the CPU test compares with the required set."""
    out = set()
    for row in rows if rows is not None else CASES:
        k, p = row["kern"], row["p"]
        n = work_items(row)
        if n is not None:
            out.add((k, "wrap" if wraps(n) else "nowrap"))
        if k == "colsum":
            f = colsum_form(p["B"], p["HW"], p["C"], (64 << 20) if p["ws"] else 0)
            out.add(("colsum", "multi" if f["nchunk"] > 1 else "one", "partial" if f["partial"] else "atomic"))
            if f["passes"] > 1:
                out.add(("colsum", "c8>256"))
            if f["want_one"]:
                out.add(("colsum", "B>512"))
            if f["dead"]:
                out.add(("colsum", "idle_lanes"))
        if k == "zero":
            for off in range(16):
                f = zero_form(off, p["nbytes"])
                out.add(("zero", "head" if f["head"] else "nohead", "tail" if f["tail"] else "notail"))
        if k == "vit_patch_rows":
            out.add(("vit_patch_rows", "pair" if vit_pair(p["P"], p["S"]) else "nopair"))
        if k == "plosses":
            ch = plosses_chunks(p["per"])
            if any(a == b for a, b in ch):
                out.add(("plosses", "empty_chunk"))
            if any(b - a > 256 for a, b in ch):
                out.add(("plosses", "multi_trip"))
            out.update({("plosses", "d_eps", p["d_eps"]), ("plosses", "lvlb", p["lvlb"]), ("plosses", "per_sample", p["per_sample"])})
        if k == "mse":
            out.add(("mse", "cap256" if ew_grid(p["n"]) > 256 else "nocap"))
            if p["n"] > mse_blocks(p["n"]) * 256:
                out.add(("mse", "multi_trip"))
        if k in ("transpose", "nchw_to_tok") and "empty_tile" in row["tags"]:
            out.add((k, "empty_tile"))
        if k == "ddim_step":
            out.update({("ddim", "e_u", p["e_u"]), ("ddim", "noise", p["noise"]), ("ddim", "pred_x0", p["pred_x0"]), ("ddim", "alias", p["alias"]),
                        ("ddim", "index", p["index"])})
    return out


REQUIRED_FORMS = (
    {(k, w) for k in ("geglu_fwd", "geglu_bwd", "silu_fwd", "silu_bwd", "axpby", "pool2x2", "conv_tap", "vit_tokens", "vit_patch_rows", "adamw", "zero")
     for w in ("wrap", "nowrap")}
    | {("colsum", "one", "atomic"), ("colsum", "multi", "partial"), ("colsum", "multi", "atomic"), ("colsum", "c8>256"), ("colsum", "B>512"),
       ("colsum", "idle_lanes")}
    | {("zero", h, t) for h in ("head", "nohead") for t in ("tail", "notail")}
    | {("vit_patch_rows", "pair"), ("vit_patch_rows", "nopair"), ("plosses", "empty_chunk"), ("plosses", "multi_trip"), ("mse", "cap256"),
       ("mse", "nocap"), ("mse", "multi_trip"), ("transpose", "empty_tile"), ("nchw_to_tok", "empty_tile")}
    | {("plosses", k, v) for k in ("d_eps", "lvlb", "per_sample") for v in (True, False)}
    | {("ddim", k, v) for k in ("e_u", "noise", "pred_x0", "alias") for v in (True, False)} | {("ddim", "index", 0), ("ddim", "index", 19)}
    | {("dpmpp_step", "wrap"), ("dpmpp_step_dev", "wrap")})


# ------------------------------------------------------------------------------------------------ operands

def _seed(row):
    return 9000 + [r["name"] for r in CASES].index(row["name"])


def _plant(t, vals):
    """Put `vals` at the front of the first row(s) of t where it has room for all of them."""
    if t.numel() >= len(vals):
        t.view(-1)[:len(vals)] = torch.tensor(vals, dtype=t.dtype)
    return t


def make_ops(row, dt, device="cpu"):
    """The operands of a row in the storage type, drawn on the CPU from a generator seeded by the row's place in the table."""
    g = torch.Generator().manual_seed(_seed(row))
    k, p = row["kern"], row["p"]
    rn = lambda *s: torch.randn(*s, generator=g)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
    o = {}
    if k in ("geglu_fwd", "geglu_bwd"):
        h = rn(p["M"], 2 * p["F"]) * 1.5
        if p["F"] >= 8:
            h[0, p["F"]:p["F"] + 4] = torch.tensor([20.0, -20.0, 90.0, -90.0])       # the gate half
        o["h"] = h.to(dt)
        if k == "geglu_bwd":
            o["dout"] = rn(p["M"], p["F"]).to(dt)
    elif k in ("silu_fwd", "silu_bwd"):
        x = rn(p["M"], p["C"]) * 2
        x[0, :4] = torch.tensor([20.0, -20.0, 90.0, -90.0])
        o["x"] = x.to(dt)
        if k == "silu_bwd":
            o["dy"] = rn(p["M"], p["C"]).to(dt)
    elif k == "axpby":
        if p["ints"]:
            o["x"], o["y"] = ri(-8, 8, p["M"], p["C"]).to(dt), ri(-8, 8, p["M"], p["C"]).to(dt)
        else:
            o["x"], o["y"] = rn(p["M"], p["C"]).to(dt), rn(p["M"], p["C"]).to(dt)
    elif k == "pool2x2":
        o["in"] = ri(-8, 8, p["B"] * 4 * p["H"] * p["W"], p["C"]).to(dt)
        o["out0"] = ri(-8, 8, p["B"] * p["H"] * p["W"], p["C"]).to(dt)
    elif k == "conv_tap":
        o["x"] = rn(p["B"] * p["Hin"] * p["Win"], p["C"]).to(dt)
    elif k == "vit_tokens":
        o["patch"] = ri(-8, 8, p["B"] * (p["T"] - 1), p["D"]).to(dt)
        o["cls"], o["pos"] = ri(-8, 8, p["D"]), ri(-8, 8, p["T"], p["D"])
    elif k == "vit_patch_rows":
        o["px"] = _plant(rn(p["B"], p["C"], p["S"], p["S"]), SPECIALS_F32)
    elif k == "transpose":
        t = rn(p["Bt"], p["R"], p["C"])
        o["in"] = (_plant(t, SPECIALS_F32) if p["idt"] == F32 else t).to(p["idt"])
    elif k == "nchw_to_tok":
        o["in"] = _plant(rn(p["B"], p["Cin"], p["HW"]), SPECIALS_F32)
    elif k == "tok_to_nchw":
        o["in"] = rn(p["B"] * p["HW"], p["C"]).to(dt)
        o["out0"] = rn(p["B"], p["C"], p["HW"])
    elif k == "pack2d":
        o["in"] = _plant(rn(p["R"], p["C"]), SPECIALS_F32)
    elif k == "repack":
        for i, m in enumerate(p["mats"]):
            o[f"src{i}"] = _plant(rn(m["R"], m["C"]), SPECIALS_F32)
    elif k == "softmax":
        S = rn(p["M"], p["N"]) * 4
        if p["M"] > 2:
            S[1] = -30.0                                  # a constant row far below 0: a pad read as score 0 would dominate it
            S[2, p["N"] // 2] = 60.0
        o["S"] = S
    elif k == "colsum":
        n = (p["B"] * p["HW"], p["C"])
        o["in"] = (ri(-4, 4, *n) if p["ints"] else rn(*n)).to(dt)
        o["out0"] = ri(-8, 8, p["B"], p["C"]) if p["ints"] else rn(p["B"], p["C"])
    elif k == "mse":
        o["eps"], o["target"] = rn(p["n"]), rn(p["n"])
    elif k == "plosses":
        o["eps"], o["target"] = rn(p["B"], p["per"]), rn(p["B"], p["per"])
        o["t"] = torch.randint(0, 1000, (p["B"],), generator=g)
        o["lvlb"] = torch.rand(1000, generator=g) + 0.1
    elif k == "timestep":
        tv = [999] if p["B"] == 1 else [0, 1, 17, 999, 500]
        o["t"] = torch.tensor(tv, dtype=torch.long)
        o["tf"] = torch.tensor([949.05] if p["B"] == 1 else [0.5, 1.25, 17.75, 899.1, 499.9], dtype=F32)
        o["freqs"] = make_freqs(p["half"])
    elif k == "qsample":
        o["z"], o["noise"] = rn(p["B"], p["per"]), rn(p["B"], p["per"])
        o["t"] = torch.randint(0, 1000, (p["B"],), generator=g)
        betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2
        ac = torch.cumprod(1 - betas, 0)
        o["sqrt_ac"], o["sqrt_1mac"] = ac.sqrt().float(), (1 - ac).sqrt().float()
    elif k == "ddim_step":
        o["x"], o["e_c"], o["e_u"], o["noise"] = rn(p["n"]), rn(p["n"]), rn(p["n"]), rn(p["n"])
        o["coef"] = ddim_table(p["S"])[0]
    elif k in ("dpmpp_step", "dpmpp_step_dev"):
        o["x"], o["e_c"], o["e_u"] = rn(p["n"]), rn(p["n"]), rn(p["n"])
        o["hist"] = rn(3, p["n"])
        o["hist"][p["index"] % 3] = float("nan")              # the slot this step writes: must not be read
        o["coef"] = dpm_table(p["S"])
    elif k == "adamw":
        o["p"], o["g"] = rn(p["n"]) * 0.1, rn(p["n"]) * 128 * 0.01
        o["m"], o["v"] = rn(p["n"]) * 0.01, (rn(p["n"]) * 0.01) ** 2 + 1e-8
    return {n: t.to(device) for n, t in o.items()}


CASES = []
CASES = _cases()
GATED_FAMILIES = tuple(MEASURED)


def evaluate(row, dt, ops):
    return EVAL[row["kern"]](row["p"], dt, ops)


def check(specs, got, c=None):
    """{output: gate dict or dict(exact_mismatch=n)} of the outputs in `got` against evaluate()'s specs."""
    res = {}
    for k, s in specs.items():
        if k not in got:
            continue
        if "exact" in s:
            w = s["exact"]
            g = got[k].reshape(w.shape)
            res[k] = dict(exact_mismatch=int((bits(g) != bits(w)).sum()) if g.dtype == w.dtype else -1)
        else:
            cc = 0.0 if s["fam"] is None else (C_GATE[s["fam"]] if c is None else c)
            res[k] = gate(got[k], s["ref"], s["fixed"], s["mag"], s["u"], cc)
    return res


def failures(res):
    bad = []
    for k, r in res.items():
        if r.get("exact_mismatch"):
            bad.append((k, "bits", r["exact_mismatch"]))
        if r.get("violations"):
            bad.append((k, "elementwise", r["violations"], r["err_over_bound"], r["first"]))
    return bad


def adamw_rows():
    return [r for r in CASES if r["kern"] == "adamw"]


def model_needs(row, dt):
    """{(family, output): the c the rounding model needs on this row}; exact outputs must match their own definition."""
    out = {}
    if row["kern"] == "adamw":
        ops = make_ops(row, dt)
        st = (ops["p"], ops["m"], ops["v"])
        for step in (1, 2, 3):
            sp = eval_adamw_step(st, ops["g"], step)
            for k, r in check(sp, {k: s["model"] for k, s in sp.items()}, c=0.0).items():
                out[("adamw", k)] = max(out.get(("adamw", k), 0.0), r["need"])
            st = tuple(sp[k]["model"] for k in ("p", "m", "v"))
        return out
    if row["kern"] not in EVAL:
        return out
    ops = make_ops(row, dt)
    sp = evaluate(row, dt, ops)
    for k, r in check(sp, {k: s["model"] for k, s in sp.items() if "model" in s}, c=0.0).items():
        if sp[k]["fam"] is not None:
            out[(sp[k]["fam"], k)] = r["need"]
        else:
            assert r["violations"] == 0, (row["name"], k, r)
    return out


def measure_constants(rows=None):
    """{family: (largest need of the rounding model over the table, the row and output that needs it)}."""
    worst = {f: (0.0, "") for f in MEASURED}
    for row in rows if rows is not None else CASES:
        for dt in row["dtypes"]:
            if dt is None:
                continue
            for (fam, k), v in model_needs(row, dt).items():
                if v > worst[fam][0]:
                    worst[fam] = (v, "%s %s %s" % (row["name"], "bf16" if dt == BF else "f32", k))
    return worst


if __name__ == "__main__":
    import time
    t0 = time.time()
    for fam, (v, who) in measure_constants().items():
        print("%-8s need %.3f (%s)  recorded %.3f  -> c = %.3f" % (fam, v, who, MEASURED[fam], C_GATE[fam]))
    print("rows", len(CASES), "seconds", round(time.time() - t0, 1))
