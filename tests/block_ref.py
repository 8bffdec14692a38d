"""Reference, same-storage comparator and case table for the engine BLOCKS (ctrlora_amd/engine/blocks.py: ResBlockE,
SpatialTransformerE and the linear / group / weight-gradient helpers they compose).  No GPU imports at module level.

REFERENCE.  resblock() / spatial_transformer(): the arithmetic of oracle/ref_model.py's functions of the same names (same state
dict keys), evaluated in whatever dtype the tensors have -- the tests feed fp64 -- with no cast anywhere (ref_model.group_norm
casts to fp32 and is not used).  Gradients come from autograd over these functions.

COMPARATOR.  The same functions with Mode(round=True): a `store` hook rounds to bf16 in forward and rounds the incoming gradient
to bf16 in backward, at exactly the tensors the engine writes as bf16 between launches (read off blocks.py):

  ResBlock   h1 = silu(GN(x)); t_e = semb A^T and e_out; h2 = conv1 + emb; h3 = silu(GN(h2)); skip(x) (it sits in `out` before
             conv2 adds to it); out.  Backward: dh3, dh2, de (the fp32 column sum de32 is NOT rounded, its packed copy is), u_e,
             dh1, dskip, dx; dsemb = round(prefill + gradient).
  Attention  t = x A^T, q (after the d_head^-0.5 log2(e) scale when pre-scaled: one rounding of the scaled value, and dq is
             the rounded gradient of the TRUE q), k, v, a, t_o, out (+ residual).  Backward: the same tensors' gradients.
  ST         xn = GN(x), h0, LN outputs, p (unfused GEGLU only), gg, t_f, h3, out.  Backward likewise; every residual
             gradient is added before the one rounding (accum=).

Not rounded: biases, norm parameters, statistics, lse, de32 / de_slot, every weight-gradient accumulator (fp32 in the engine).
Weights are read rounded (the packed copies) with a straight-through gradient (fp32 accumulators); a folded weight is
round(W32 + B A), ONE rounding, from the fp32 factors.

Two modes that store less than the training pass:
  * fused GEGLU (x-stationary or tile kernel): the 8C-wide pre-activation stays in the fp32 accumulators -- not rounded;
  * LayerNorm as the prologue of the product that reads it: the normalised tensor is never STORED, but the kernel still rounds
    it to bf16 -- the matrix instruction's operand (csrc/gemm_xs.hip packs the normalised pair before the product) -- and the
    backward pass stores d(LN(x)) before layernorm_bwd reads it.  So the comparator rounds at the same two points as for a
    materialised norm; the launch FORM differs (the cases assert it), the storage model does not.

CASES.  CASES / RUNS: the smallest shapes at which each launch-sequence branch of blocks.py is still taken; every run names
the predicates it relies on (`expect`), evaluated by predicates() and asserted before anything runs.
"""
from __future__ import annotations

import dataclasses
import functools
from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

from oracle import arch

P = "blk"                      # state-dict prefix of the block under test
HEADS, NCTX, CTX_DIM, NIP = 8, 77, 768, 4
CFG = arch.ArchCfg(model_channels=320, context_dim=CTX_DIM, lora_rank=0)      # time_embed_dim 1280 for every case
LOG2E = 1.4426950408889634
TB = P + ".transformer_blocks.0"


def rbf(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(x.dtype)


class _Store(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.bwd = bwd
        return rbf(x) if fwd else x.clone()

    @staticmethod
    def backward(ctx, g):
        return (rbf(g) if ctx.bwd else g), None, None


class _StoreScaled(torch.autograd.Function):
    """q stored as round(q * alpha); the engine's dq is the rounded gradient of the true q."""
    @staticmethod
    def forward(ctx, q, alpha):
        ctx.alpha = alpha
        return rbf(q * alpha)

    @staticmethod
    def backward(ctx, g):
        return rbf(g * ctx.alpha), None


class _GegluSwapped(torch.autograd.Function):
    """DEFECT: value * gelu(gate) whose backward hands the value's gradient to the gate and the gate's to the value."""
    @staticmethod
    def forward(ctx, val, gate):
        ctx.save_for_backward(val, gate)
        return val * F.gelu(gate)

    @staticmethod
    def backward(ctx, g):
        val, gate = ctx.saved_tensors
        with torch.enable_grad():
            v, t = val.detach().requires_grad_(True), gate.detach().requires_grad_(True)
            dv, dt = torch.autograd.grad(v * F.gelu(t), (v, t), g)
        return dt, dv


@dataclasses.dataclass(frozen=True)
class Mode:
    round: bool = False            # False: the exact evaluation
    lora: str = "live"             # "live": second K segment (t stored) | "folded": round(W32 + B A)
    geglu: str = "unfused"         # "unfused": p stored | "xs" / "tile": fused, p stays in the accumulators
    prescale: bool = False         # q stored after the d_head^-0.5 log2(e) scale (bf16 attention kernels)
    defect: Optional[str] = None   # DEFECTS key: a deliberately wrong block (CPU defect-detection test only)


EXACT = Mode()
DEFECTS = ("scale", "lora", "residual", "accum", "rowbias", "geglu_swap")


def S(m: Mode, x, fwd=True, bwd=True):
    return _Store.apply(x, fwd, bwd) if m.round else x


def Wr(m: Mode, w):
    """A packed weight: rounded once, straight-through gradient (the accumulators are fp32)."""
    return _Store.apply(w, True, False) if m.round else w


def linear(sd, m: Mode, name: str, x):
    """x W^T + b (+ (x A^T) B^T): the product of blocks.linear_fwd before its epilogue's residual / store."""
    W = sd[name + ".weight"]
    W = W.reshape(W.shape[0], -1)
    b = sd.get(name + ".bias")
    dn = name + ".lora_layer.down.weight"
    drop = m.defect == "lora" and (name.endswith("attn1.to_v") or name.endswith("emb_layers.1"))
    if dn in sd and not drop:
        A, B = sd[dn], sd[name + ".lora_layer.up.weight"]
        if m.lora == "folded":
            y = x @ Wr(m, W + B @ A).t()
        else:
            t = S(m, x @ Wr(m, A).t())
            y = x @ Wr(m, W).t() + t @ Wr(m, B).t()
    else:
        y = x @ Wr(m, W).t()
    return y if b is None else y + b


# ----------------------------------------------------------------------------------------------- ResBlock

def resblock(sd, p, x, emb, m: Mode = EXACT, semb=None, e_pre=None, taps=None):
    """ResBlock._forward (openaimodel.py:254-274), x NCHW.  semb: silu(emb) given directly (what the engine takes);
    e_pre: the emb_layers output given directly; taps["e_out"]: the tensor whose gradient is d emb_out before any rounding."""
    def gn(n, t):
        return F.group_norm(t, 32, sd[n + ".weight"], sd[n + ".bias"], 1e-5)

    def conv(n, t):
        return F.conv2d(t, Wr(m, sd[n + ".weight"]), sd[n + ".bias"], padding=1)

    h1 = S(m, F.silu(gn(p + ".in_layers.0", x)))
    if e_pre is None:
        e = S(m, linear(sd, m, p + ".emb_layers.1", F.silu(emb) if semb is None else semb))
    else:
        e = e_pre
    if taps is not None:
        taps["e_out"] = e
    h2 = conv(p + ".in_layers.2", h1)
    if m.defect != "rowbias":
        h2 = h2 + e[:, :, None, None]
    h2 = S(m, h2)
    h3 = S(m, F.silu(gn(p + ".out_layers.0", h2)))
    xs = x.detach() if m.defect == "accum" else S(m, x, fwd=False)      # dskip is stored before GroupNorm's backward adds it
    if p + ".skip_connection.weight" in sd:
        r = S(m, F.conv2d(xs, Wr(m, sd[p + ".skip_connection.weight"]), sd[p + ".skip_connection.bias"]))
    else:
        r = xs
    h = conv(p + ".out_layers.3", h3)
    return S(m, h if m.defect == "residual" else h + r)


# ----------------------------------------------------------------------------------------------- SpatialTransformer

def _attention(sd, m: Mode, p, xq, c, B, heads, residual, ip=None):
    q = linear(sd, m, p + ".to_q", xq)
    k, v = S(m, linear(sd, m, p + ".to_k", c)), S(m, linear(sd, m, p + ".to_v", c))
    inner = q.shape[1]
    dh = inner // heads
    scale = float(dh) ** -0.5
    if m.round and m.prescale:
        qa = scale * LOG2E
        q = _StoreScaled.apply(q, qa) / qa
    else:
        q = S(m, q)
    if m.defect == "scale":
        scale *= 1.02

    def hd(t):
        return t.reshape(B, t.shape[0] // B, heads, dh).permute(0, 2, 1, 3)

    qh = hd(q)
    o = (qh @ hd(k).transpose(-1, -2) * scale).softmax(-1) @ hd(v)
    if ip is not None:
        k_ip, v_ip = S(m, linear(sd, m, p + ".to_k_ip", ip)), S(m, linear(sd, m, p + ".to_v_ip", ip))
        o = o + float(sd[p + ".ip_scale"]) * ((qh @ hd(k_ip).transpose(-1, -2) * scale).softmax(-1) @ hd(v_ip))
    a = S(m, o.permute(0, 2, 1, 3).reshape(xq.shape[0], inner))
    y = linear(sd, m, p + ".to_out.0", a)
    return S(m, y if residual is None else y + residual)


def spatial_transformer(sd, p, x, ctx, heads, ip=None, m: Mode = EXACT):
    """SpatialTransformer.forward, use_linear=False (attention.py:321-340), x NCHW, ctx [B, Nkv, context_dim].
    ip: image-prompt tokens [B, Nip, context_dim] -> softmax(text) V + ip_scale * softmax(ip) V_ip (blocks.AttnE.fwd)."""
    B, C, H, W = x.shape
    tb = p + ".transformer_blocks.0"
    xn = S(m, F.group_norm(x, 32, sd[p + ".norm.weight"], sd[p + ".norm.bias"], 1e-6))
    h0 = S(m, linear(sd, m, p + ".proj_in", xn.permute(0, 2, 3, 1).reshape(B * H * W, C)))

    def ln(i, t):
        return S(m, F.layer_norm(t, (C,), sd[f"{tb}.norm{i}.weight"], sd[f"{tb}.norm{i}.bias"], 1e-5))

    c = ctx.reshape(-1, ctx.shape[-1])
    n1 = ln(1, h0)
    h1 = _attention(sd, m, tb + ".attn1", n1, n1, B, heads, None if m.defect == "residual" else h0)
    h2 = _attention(sd, m, tb + ".attn2", ln(2, h1), c, B, heads, h1.detach() if m.defect == "accum" else h1,
                    ip=None if ip is None else ip.reshape(-1, ip.shape[-1]))
    pz = linear(sd, m, tb + ".ff.net.0.proj", ln(3, h2))
    if m.geglu == "unfused":
        pz = S(m, pz)
    val, gate = pz.chunk(2, dim=-1)
    gg = S(m, _GegluSwapped.apply(val, gate) if m.defect == "geglu_swap" else val * F.gelu(gate))
    h3 = S(m, linear(sd, m, tb + ".ff.net.2", gg) + h2)
    y = linear(sd, m, p + ".proj_out", h3).reshape(B, H, W, C).permute(0, 3, 1, 2)
    return S(m, y + x)


# ----------------------------------------------------------------------------------------------- cases

@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    kind: str                  # "res" | "st"
    cin: int
    cout: int
    B: int
    H: int
    W: int
    rank: int                  # LoRA rank in the state dict (0: none)
    train: str                 # "ft" fine-tune | "frozen" (UNet) | "pre" (train_all) | "infer" (LoRA folded, no backward)

    @property
    def M(self):
        return self.B * self.H * self.W


# rb-pre / rb-pre-row3 are wider than the branch alone needs (64 ch at 8x8, 32 ch at 64x64 would take it): at those sizes the
# comparator's error on the per-channel GroupNorm / bias gradients moved by up to 1.8x between seeds, and with one channel per
# group d emb_out is identically zero (GroupNorm removes a per-sample, per-channel constant).  At 128 ch, 16x16 and 256 ch,
# B = 2, 64x64 every gated output's floor is reproducible to 1.3x (test_block_reference_model.py holds them to 1.5x).
CASES = {c.name: c for c in (
    Case("rb-ft", "res", 320, 320, 2, 8, 8, 64, "ft"),
    Case("rb-ft-skip", "res", 320, 640, 3, 6, 4, 64, "ft"),
    Case("rb-frozen", "res", 640, 320, 2, 8, 8, 0, "frozen"),
    Case("rb-pre", "res", 128, 128, 2, 16, 16, 0, "pre"),
    Case("rb-pre-row3", "res", 256, 256, 2, 64, 64, 0, "pre"),
    Case("st-ft-r64", "st", 320, 320, 2, 8, 8, 64, "ft"),
    Case("st-ft-r32", "st", 640, 640, 2, 8, 8, 32, "ft"),
    Case("st-ft-ragged", "st", 320, 320, 3, 6, 4, 128, "ft"),
    Case("st-ft-1280", "st", 1280, 1280, 2, 4, 4, 64, "ft"),
    Case("st-frozen-train-320", "st", 320, 320, 2, 8, 8, 0, "frozen"),
    Case("st-frozen-train-640", "st", 640, 640, 2, 8, 8, 0, "frozen"),
    Case("st-infer-xs", "st", 320, 320, 2, 8, 8, 128, "infer"),
    Case("st-infer-tile", "st", 640, 640, 2, 8, 8, 64, "infer"),
    Case("st-ip", "st", 320, 320, 2, 8, 8, 0, "frozen"),
    Case("st-pre", "st", 320, 320, 2, 8, 8, 64, "pre"),
)}


@dataclasses.dataclass(frozen=True)
class Run:
    """One parametrised GPU test: a case, a dtype, a variant and the launch-form predicates it relies on."""
    case: str
    dtype: str                 # "bf16" | "f32"
    variant: str = ""          # "" | "deslot" | "wstream" | "ln-off" | "norecord"
    expect: Tuple[Tuple[str, object], ...] = ()
    record: bool = True
    backward: bool = True
    ip: bool = False

    @property
    def id(self):
        return "-".join(s for s in (self.case, self.dtype, self.variant) if s)

    @property
    def mode(self) -> Mode:
        """The comparator's storage model of this run (bf16 runs only)."""
        e = dict(self.expect)
        geglu = "xs" if e.get("xs_geglu") else "tile" if e.get("tile_geglu") else "unfused"
        return Mode(round=True, lora="folded" if e.get("folded") else "live", geglu=geglu, prescale=True)


def _st_ft(r64, grouped=True):
    return (("grouped", grouped), ("grp_r64", r64), ("ln_fusable1", False), ("ln_fusable2", False), ("ln3_fused", False),
            ("xs_geglu", False), ("tile_geglu", False), ("folded", False))


_ST_FT_F32 = (("grouped", False), ("ln_fusable1", False), ("ln_fusable2", False), ("ln3_fused", False), ("xs_geglu", False),
              ("tile_geglu", False), ("folded", False))
_ST_FROZEN = (("fused_qkv", True), ("ln_fusable1", True), ("ln_fusable2", True), ("ln3_fused", True), ("xs_geglu", False),
              ("tile_geglu", False), ("folded", False))
_ST_FROZEN_MAT = (("fused_qkv", True), ("ln_fusable1", False), ("ln_fusable2", False), ("ln3_fused", False),
                  ("xs_geglu", False), ("tile_geglu", False), ("folded", False))
_RB = (("row3", False),)

# The bf16 weight-gradient queue: a pre-training ResBlock queues 2 x 9 single-tap problems + the emb linear's dW = 19 (7 in
# the row-of-three-taps form), below the automatic flush at 24; st-pre queues 32 in one backward (ten LoRA'd linears x
# (dB, dA, dW) + proj_in / proj_out), so there the flush fires inside the block and 8 problems are left for the stage's own.
RUNS = (
    Run("rb-ft", "bf16", "", _RB), Run("rb-ft", "f32", "", _RB),
    Run("rb-ft", "bf16", "deslot", _RB), Run("rb-ft", "f32", "deslot", _RB),
    Run("rb-ft", "bf16", "wstream", _RB),
    Run("rb-ft-skip", "bf16", "", _RB), Run("rb-ft-skip", "f32", "", _RB),
    Run("rb-ft-skip", "bf16", "deslot", _RB),
    Run("rb-frozen", "bf16", "", _RB),
    Run("rb-pre", "bf16", "", _RB + (("wq_per_bwd", 19),)), Run("rb-pre", "f32", "", _RB),
    Run("rb-pre-row3", "bf16", "", (("row3", True), ("wq_per_bwd", 7))),
    Run("st-ft-r64", "bf16", "", _st_ft(True)), Run("st-ft-r64", "f32", "", _ST_FT_F32),
    Run("st-ft-r64", "bf16", "wstream", _st_ft(True)),
    Run("st-ft-r64", "bf16", "norecord", (("grouped", True), ("ln_fusable1", False), ("ln_fusable2", False),
                                          ("ln3_fused", False), ("xs_geglu", False), ("tile_geglu", True), ("folded", False)),
        record=False, backward=False),
    Run("st-ft-r32", "bf16", "", _st_ft(False)),
    Run("st-ft-ragged", "bf16", "", _st_ft(True)), Run("st-ft-ragged", "f32", "", _ST_FT_F32),
    Run("st-ft-1280", "bf16", "", _st_ft(True)),
    Run("st-frozen-train-320", "bf16", "", _ST_FROZEN), Run("st-frozen-train-320", "bf16", "ln-off", _ST_FROZEN_MAT),
    Run("st-frozen-train-640", "bf16", "", _ST_FROZEN),
    Run("st-frozen-train-320", "f32", "", _ST_FROZEN_MAT),
    Run("st-infer-xs", "bf16", "", (("grouped", True), ("ln_fusable1", True), ("ln_fusable2", True), ("ln3_fused", True),
                                    ("xs_geglu", True), ("tile_geglu", False), ("folded", True)), record=False, backward=False),
    Run("st-infer-tile", "bf16", "", (("grouped", True), ("ln_fusable1", True), ("ln_fusable2", True), ("ln3_fused", False),
                                      ("xs_geglu", False), ("tile_geglu", True), ("folded", True)), record=False, backward=False),
    Run("st-ip", "bf16", "", (("fused_qkv", True), ("ln_fusable1", True), ("ln_fusable2", True), ("ln3_fused", True),
                              ("xs_geglu", True), ("tile_geglu", False), ("folded", False), ("ip_live", True)),
        record=False, backward=False, ip=True),
    Run("st-pre", "bf16", "", _st_ft(True) + (("wq_auto_flush", True),)), Run("st-pre", "f32", "", _ST_FT_F32),
)
RUN_BY_ID = {r.id: r for r in RUNS}


def trainable_names(case: Case, sd):
    """What nets._Builder declares for this case: every tensor under train_all, LoRA factors and `norm` layers when fine-tuning
    (nets.is_trainable_name), nothing for the frozen UNet."""
    if case.train == "pre":
        return sorted(k for k, v in sd.items() if v.dim() > 0)
    if case.train in ("ft", "infer"):        # (the folded inference executor declares them too: its repack reads the masters)
        return sorted(k for k in sd if "lora_layer" in k or "norm" in k)
    return []


def gated(run: Run, sd):
    """Names of the outputs the numeric gates apply to (keys of evaluate()'s result)."""
    c = CASES[run.case]
    if not run.backward:
        return ["out"]
    names, tn = ["out", "dx"], trainable_names(c, sd)
    if c.kind == "res" and c.train != "frozen":
        if run.variant == "deslot":            # d emb_out lands in the slot; the emb linear's backward is hoisted out of the block
            names.append("de")
            tn = [k for k in tn if "emb_layers" not in k]
        else:
            names.append("dsemb")
    return names + tn


def pure_predicates(run: Run) -> Dict[str, object]:
    """The part of `expect` that is plain Python arithmetic on the case's shape (no packed object needed): hip.xs_ln_ok,
    hip.xs_geglu_ok, the row-of-three-taps condition of blocks.conv3_bwd_weight and the weight-gradient queue's length."""
    from ctrlora_amd import hip
    from ctrlora_amd.engine import blocks
    c = CASES[run.case]
    bf = run.dtype == "bf16"
    out: Dict[str, object] = {}
    if c.kind == "res":
        out["row3"] = bool(blocks.WGRAD_ROW3 and bf and c.train == "pre" and c.M % 32 == 0 and c.W % 64 == 0)
        if c.train == "pre" and bf:
            out["wq_per_bwd"] = 2 * (3 if out["row3"] else 9) + 1          # two convs + the emb linear's dense weight
        return out
    folded = c.train == "infer" and not run.record
    live = c.rank > 0 and not folded
    dense = run.record and c.train == "pre"
    lora_in = live or dense
    C = c.cin
    ok = lambda N, act=hip.ACT_NONE: bool(bf and not lora_in and hip.xs_ln_ok(c.M, N, C, act))
    grouped = c.rank > 0 and bf and c.train != "frozen"
    fused = c.train == "frozen"
    out["ln_fusable1"] = ok(3 * C) if (fused or grouped) else False
    out["ln_fusable2"] = ok(C)
    xs = bool(not run.record and bf and hip.xs_geglu_ok(c.M, C, 0 if folded else c.rank))
    tile = not xs and not run.record and (8 * C) % 320 == 0 and (4 * C) % 80 == 0
    out["xs_geglu"], out["tile_geglu"] = xs, tile
    out["ln3_fused"] = (not tile) and ok(8 * C, hip.ACT_GEGLU_SPLIT if xs else hip.ACT_NONE)
    out["folded"] = folded
    if c.rank and c.train != "frozen" and bf:
        out["grp_r64"] = c.rank % 64 == 0
    if c.train == "pre" and bf:
        out["wq_auto_flush"] = 10 * 3 + 2 >= 24       # ten LoRA'd linears (dB, dA, dW) + proj_in / proj_out
    return out


# ----------------------------------------------------------------------------------------------- state and inputs

def make_sd(case: Case, seed: int, ip_scale: Optional[float] = None) -> Dict[str, torch.Tensor]:
    shapes: Dict[str, tuple] = {}
    meta = dict(cin=case.cin, cout=case.cout) if case.kind == "res" else dict(ch=case.cin, heads=HEADS, d_head=case.cin // HEADS)
    arch._layer_shapes(shapes, case.kind, P, meta, CFG, case.rank)
    if ip_scale is not None:
        shapes[TB + ".attn2.to_k_ip.weight"] = (case.cin, CTX_DIM)
        shapes[TB + ".attn2.to_v_ip.weight"] = (case.cin, CTX_DIM)
    sd = arch.make_state(shapes, seed)
    if ip_scale is not None:
        sd[TB + ".attn2.ip_scale"] = torch.tensor(float(ip_scale))
    return sd


def make_inputs(case: Case, seed: int) -> Dict[str, torch.Tensor]:
    """Unit-scale inputs and an upstream gradient of scale numel^-0.5, all bf16-representable (both engine dtypes read the same
    values); non-zero pre-fills for every accumulation target."""
    g = torch.Generator().manual_seed(1000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    B, H, W = case.B, case.H, case.W
    d = dict(x=rbf(rn(B, case.cin, H, W)))
    dout = rn(B, case.cout, H, W)
    d["dout"] = rbf(dout * dout.numel() ** -0.5)
    if case.kind == "res":
        ted = CFG.time_embed_dim
        d["semb"] = rbf(rn(B, ted))
        d["e_wide"] = rbf(rn(B, case.cout + 192))                     # rb-frozen: e_pre = columns [64, 64 + cout) of it
        d["dsemb0"] = rbf(rn(B, ted) * (B * ted) ** -0.5)
        d["de_wide0"] = rn(B, case.cout + 192) * (B * case.cout) ** -0.5
    else:
        d["c"] = rbf(rn(B, NCTX, CTX_DIM))
        d["c_ip"] = rbf(rn(B, NIP, CTX_DIM))
    return d


E_OFF = 64


def tok(x: torch.Tensor) -> torch.Tensor:
    """NCHW -> token-major [B H W, C]."""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def evaluate(case: Case, sd, inp, m: Mode, *, e_pre=False, ip=False, backward=True) -> Dict[str, torch.Tensor]:
    """Every output of the block, token-major, in fp64: out, dx, and per state-dict name the parameter gradients;
    ResBlock: "dsemb" = pre-fill + gradient (rounded once under m.round), "de" = d emb_out (unrounded fp32 column sum)."""
    sd64 = {k: v.double() for k, v in sd.items()}
    leaves = {k: v.requires_grad_(True) for k, v in sd64.items() if v.dim() > 0}
    x = inp["x"].double().requires_grad_(True)
    res: Dict[str, torch.Tensor] = {}
    taps: Dict[str, torch.Tensor] = {}
    extra = {}
    if case.kind == "res":
        if e_pre:
            e_leaf = inp["e_wide"][:, E_OFF:E_OFF + case.cout].double().requires_grad_(True)
            out = resblock(sd64, P, x, None, m, e_pre=e_leaf, taps=taps)
        else:
            extra["semb"] = inp["semb"].double().requires_grad_(True)
            out = resblock(sd64, P, x, None, m, semb=extra["semb"], taps=taps)
    else:
        out = spatial_transformer(sd64, P, x, inp["c"].double(), HEADS, ip=inp["c_ip"].double() if ip else None, m=m)
    res["out"] = tok(out.detach())
    if not backward:
        return res
    names = list(leaves)
    if case.kind == "res":
        extra["e_out"] = taps["e_out"]          # (the leaf e_pre itself, or the stored emb_out: its gradient is de32)
    ins = [x] + [leaves[k] for k in names] + list(extra.values())
    grads = torch.autograd.grad((out * inp["dout"].double()).sum(), ins, allow_unused=True)
    dx = grads[0]
    res["dx"] = tok(rbf(dx) if m.round else dx)
    for k, g in zip(names, grads[1:1 + len(names)]):
        if g is not None:
            res[k] = g
    by = dict(zip(extra, grads[1 + len(names):]))
    if case.kind == "res" and by["e_out"] is not None:
        res["de"] = by["e_out"]
    if "semb" in by:
        ds = inp["dsemb0"].double() + (0 if by["semb"] is None else by["semb"])
        res["dsemb"] = rbf(ds) if m.round else ds
    return res


@functools.lru_cache(maxsize=None)
def reference(case_name: str, seed: int, e_pre=False, ip_scale: Optional[float] = None, backward=True):
    """The exact fp64 evaluation, computed once per (case, seed, form) and shared: treat the result as read-only."""
    case = CASES[case_name]
    return evaluate(case, make_sd(case, seed, ip_scale), make_inputs(case, seed), EXACT, e_pre=e_pre, ip=ip_scale is not None,
                    backward=backward)


def rel(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


# ----------------------------------------------------------------------------------------------- engine side (GPU)

def build_block(case: Case, sd, dtype, need_bwd=True):
    """The block built the way the engine builds it: nets._Builder(...).res() / .st(), TrainableSet.materialize, then
    ControlNetE.repack itself (one descriptor-table re-pack over linears, LoRA factors and trainable convs; merge_lora where
    the executor folds).  Frozen blocks follow UNetE.__init__ (no trainable set, lora=False).  Returns (block, builder, sets)."""
    from ctrlora_amd.engine import nets
    from ctrlora_amd.engine.packing import TrainableSet
    dev = torch.device("cuda")
    if case.train == "frozen":
        b = nets._Builder(sd, "", dtype, dev, need_bwd, None)
        blk = b.res(P, case.cin, case.cout) if case.kind == "res" else b.st(P, case.cin, HEADS, False)
        return blk, b, []
    train_all = case.train == "pre"
    tr = TrainableSet()
    tr_lora = TrainableSet() if train_all else tr
    b = nets._Builder(sd, "", dtype, dev, need_bwd, tr, tr_lora, train_all, True, True)
    merge = not need_bwd                                   # ControlNetE: merge_lora defaults to "built without a backward"
    b.fold_lora = merge
    blk = b.res(P, case.cin, case.cout) if case.kind == "res" else b.st(P, case.cin, HEADS, True)
    tr.items.reverse()                                     # backward-completion order, as ControlNetE lays the buffer out
    sets = [tr] + ([tr_lora] if (train_all and tr_lora.items) else [])
    for ts in sets:
        ts.materialize(dict(sd), dev)

    class _Net(nets.ControlNetE):
        def __init__(self):
            pass

    net = _Net()
    net._b, net.tr, net.tr_lora, net.dtype, net.device, net.merge_lora = b, tr, (tr_lora if tr_lora.items else tr), dtype, dev, merge
    net.repack()
    return blk, b, sets


def predicates(run: Run, blk, ctx) -> Dict[str, object]:
    """The launch-form predicates of blocks.py for this block and context, as the block's own fwd / bwd evaluate them."""
    from ctrlora_amd import hip
    from ctrlora_amd.engine import blocks
    c = CASES[run.case]
    bf = ctx.dtype == torch.bfloat16
    out: Dict[str, object] = {}
    if c.kind == "res":
        out["row3"] = bool(blk.conv1.tW is not None and blocks.WGRAD_ROW3 and bf and c.M % 32 == 0 and c.W % 64 == 0)
        return out
    M, L = c.M, blk.ff_proj
    out["ln_fusable1"], out["ln_fusable2"] = blk.attn1.ln_fusable(ctx, M), blk.attn2.ln_fusable(ctx, M)
    xs = bool(not ctx.record and bf and L.N % 64 == 0 and hip.xs_geglu_ok(M, L.K, 0 if blocks.folded(ctx, L) else L.r))
    tile = bool(not xs and not ctx.record and L.geglu_ok())
    out["xs_geglu"], out["tile_geglu"] = xs, tile
    out["ln3_fused"] = bool(not tile and blocks.ln_prologue_ok(ctx, M, L.N, L.K, blocks.input_live(ctx, L),
                                                               hip.ACT_GEGLU_SPLIT if xs else hip.ACT_NONE))
    out["folded"] = bool(blocks.folded(ctx, L))
    out["grouped"] = blk.attn1.group is not None and bf
    out["fused_qkv"] = blk.attn1.fused_qkv is not None
    if blk.attn1.group is not None:
        out["grp_r64"] = blk.attn1.group.r % 64 == 0
    out["ip_live"] = blk.attn2.ip_live()
    return out
