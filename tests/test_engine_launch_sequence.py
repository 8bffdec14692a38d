"""Which C entry points the engine's attention and weight-gradient call sites issue, in which order and with which arguments,
per engine dtype -- on the CPU, against a recording stand-in for libctrlora_hip.so (no kernel runs; tensors live on "cpu" and
only their addresses, strides and shapes reach the stand-in).

bf16 takes the transpose-free kernels (cl_attention_fwd_v2 / _bwd_v2 / _fwd_ip, cl_weight_grad_tn_group); fp32 takes the parity
kernels, which read materialised, zero-padded transposes (cl_transpose -> cl_attention_fwd / _bwd / _fwd_ip, cl_transpose x2 ->
cl_weight_grad, with cl_conv_tap_gather in front for a 3x3 tap).  A wrong pad width, a key pitch or an lse stride that disagrees
between two calls is silent on the GPU (the fp32 kernels read out of their tiles), so every number this seam decides is written
out below as a literal: nothing here is a multiple of 64 (N = 70, Nkv = 77, Nip = 4, T = 26), so both 70 and 77 pad to 128, the
image-prompt V to 64 and the weight-gradient rows 140 / 154 to 160.  Every transposed scratch must also lie inside an allocation
that holds Bt * C * Rpad elements."""
import ctypes as C

import pytest
import torch

from ctrlora_amd import hip
from ctrlora_amd.engine import blocks, vit
from ctrlora_amd.engine.packing import Conv3W, LinearW, Trainable
from tests.test_clip_vision_cpu import TINY

BF16, F32 = hip.BF16, hip.F32
DTYPES = [torch.float32, torch.bfloat16]
B, HEADS, DH, N, NKV, NIP, R = 2, 2, 8, 70, 77, 4, 4
INNER, CTX_DIM = HEADS * DH, 24
SCALE = float(DH) ** -0.5
CPU = torch.device("cpu")


def f32(x):
    return C.c_float(x).value


class Recorder:
    """Stands in for the loaded library: every attribute is an entry point that records (name, args) and returns 0.
    cl_gemm's GemmParams and the descriptor array of cl_weight_grad_tn_group are decoded while the call is live."""

    def __init__(self, allocs):
        self.calls = []
        self.allocs = allocs          # address -> bytes of the torch.empty() allocation that starts there
        self.scratch = []             # per cl_transpose: bytes allocated at its destination (None: not a fresh allocation)
        self.row_ws = []              # per cl_attention_bwd_v2: bytes allocated at row_ws (None: no row_ws)

    def __getattr__(self, name):
        def entry(*args):
            if name == "cl_gemm":
                p = args[0]._obj
                args = ({f: getattr(p, f) for f, _ in hip.GemmParams._fields_},) + args[1:]
            elif name == "cl_weight_grad_tn_group":
                arr = C.cast(args[2], C.POINTER(hip.WgradDesc))
                args = args[:2] + ([{f: getattr(arr[i], f) for f, _ in hip.WgradDesc._fields_} for i in range(args[1])],) + args[3:]
            elif name == "cl_transpose":           # (sizes are looked up while the call is live: a released scratch's address is reused)
                self.scratch.append(self.allocs.get(args[5]))
            elif name == "cl_attention_bwd_v2":
                self.row_ws.append(self.allocs.get(args[27]))
            self.calls.append((name, args))
            return 0
        return entry

    def names(self):
        return [n for n, _ in self.calls]

    def of(self, name):
        return [a for n, a in self.calls if n == name]

    def clear(self):
        self.calls, self.scratch, self.row_ws = [], [], []


@pytest.fixture
def rec(monkeypatch):
    allocs = {}
    real_empty = torch.empty

    def empty(*a, **k):
        t = real_empty(*a, **k)
        allocs[t.data_ptr()] = t.numel() * t.element_size()
        return t

    r = Recorder(allocs)
    monkeypatch.setattr(torch, "empty", empty)
    monkeypatch.setattr(hip, "_lib", r)
    monkeypatch.setattr(hip, "stream", lambda: 0)
    monkeypatch.setattr(hip, "_workspace", None)
    monkeypatch.setattr(hip, "_zero_pages", {})
    monkeypatch.setattr(hip, "_stream_ws", {})
    monkeypatch.setattr(blocks, "PRESCALE_Q", True)
    hip.ensure_workspace(CPU)         # (the once-per-process registration is not part of any sequence below)
    assert r.names() == ["cl_set_workspace"]
    r.clear()
    return r


def esz(dtype):
    return 4 if dtype == torch.float32 else 2


def rnd(rows, cols, dtype):
    return torch.randn(rows, cols).to(dtype)


def linear(n, k, dtype, r=0, bias=True):
    L = LinearW(torch.randn(n, k), torch.randn(n) if bias else None, dtype, CPU, need_bwd=True)
    if r:
        tA, tB = Trainable("a", (r, k)), Trainable("b", (n, r))
        for t in (tA, tB):
            t.master, t.grad = torch.zeros(t.shape), torch.zeros(t.shape)
        L.attach_lora(tA, tB, CPU)
    return L


def check_transposes(rec, dtype, want):
    """want: per cl_transpose (src, ldi, bsi, Bt, R, C, Rpad).  The destination is [Bt][C][Rpad] in the engine dtype and must be
    an allocation of its own that holds Bt * C * Rpad elements."""
    got = rec.of("cl_transpose")
    assert len(got) == len(want)
    d = hip.dt_of(dtype)
    for a, room, (src, ldi, bsi, Bt, R_, C_, Rpad) in zip(got, rec.scratch, want):
        assert a[:5] == (d, d, src, ldi, bsi) and a[6:] == (Rpad, C_ * Rpad, Bt, R_, C_, Rpad, 0), (a, src, ldi, bsi, Bt, R_, C_, Rpad)
        assert room is not None and room >= Bt * C_ * Rpad * esz(dtype), (room, Bt, C_, Rpad)
    return [a[5] for a in got]


# --------------------------------------------------------------------------- attention

def self_attn(dtype):
    """Frozen-UNet form: q | k | v one product, so q, k, v are column blocks of one [M, 48] tensor (row stride 48)."""
    return blocks.AttnE(linear(INNER, INNER, dtype), linear(INNER, INNER, dtype), linear(INNER, INNER, dtype),
                        linear(INNER, INNER, dtype, r=R), HEADS, True, fused_qkv=linear(3 * INNER, INNER, dtype))


def cross_attn(dtype, r=R, fused_kv=False):
    return blocks.AttnE(linear(INNER, INNER, dtype, r=r), linear(INNER, CTX_DIM, dtype, r=r), linear(INNER, CTX_DIM, dtype, r=r),
                        linear(INNER, INNER, dtype, r=r), HEADS, False,
                        fused_kv=linear(2 * INNER, CTX_DIM, dtype) if fused_kv else None)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_self_attention_fwd_bwd(rec, dtype):
    torch.manual_seed(0)
    e, bf = esz(dtype), dtype == torch.bfloat16
    at = self_attn(dtype)
    ctx = blocks.Ctx(dtype, CPU, True)
    x = rnd(B * N, INNER, dtype)
    out, saved = at.fwd(ctx, x, None, B, N, N, residual=x)
    xn, c, q, k, v, a, lse, tq, tk, tv, to_ = saved
    assert tuple(lse.shape) == (B, HEADS, 128) and lse.dtype == torch.float32
    assert (q.stride(0), k.data_ptr() - q.data_ptr(), v.data_ptr() - q.data_ptr()) == (48, 16 * e, 32 * e)
    g = rec.of("cl_gemm")[0][0]
    assert (g["C"], g["ldc"], g["M"], g["N"], g["K1"]) == (q.data_ptr(), 48, 140, 48, 16)
    assert (g["alpha"], g["alpha_n"]) == ((f32(SCALE * 1.4426950408889634), 16) if bf else (1.0, 0))
    if bf:
        assert rec.names() == ["cl_gemm", "cl_attention_fwd_v2", "cl_gemm", "cl_gemm"]
        assert rec.of("cl_attention_fwd_v2") == [(BF16, q.data_ptr(), 48, k.data_ptr(), 48, v.data_ptr(), 48, a.data_ptr(), 16,
                                                  lse.data_ptr(), 128, 2, 2, 70, 70, 8, SCALE, 1, 0)]
    else:
        assert rec.names() == ["cl_gemm", "cl_transpose", "cl_attention_fwd", "cl_gemm", "cl_gemm"]
        vt, = check_transposes(rec, dtype, [(v.data_ptr(), 48, 3360, 2, 70, 16, 128)])
        assert rec.scratch == [2 * 16 * 128 * 4]
        assert rec.of("cl_attention_fwd") == [(F32, q.data_ptr(), 48, k.data_ptr(), 48, vt, 128, a.data_ptr(), 16,
                                               lse.data_ptr(), 128, 2, 2, 70, 70, 8, SCALE, 0)]
    assert rec.of("cl_gemm")[-1][0]["A1"] == a.data_ptr()

    rec.clear()
    dout = rnd(B * N, INNER, dtype)
    at.bwd(ctx, dout, saved, B, N, N)
    ctx.flush_wgrad()
    da = rec.of("cl_gemm")[1][0]["C"]
    if bf:
        assert rec.names() == ["cl_gemm", "cl_gemm", "cl_attention_bwd_v2", "cl_gemm", "cl_weight_grad_tn_group"]
        bw, = rec.of("cl_attention_bwd_v2")
        dq = bw[14]
        assert bw == (BF16, q.data_ptr(), 48, k.data_ptr(), 48, v.data_ptr(), 48, a.data_ptr(), 16, da, 16, lse.data_ptr(), bw[12], 128,
                      dq, 48, dq + 16 * e, 48, dq + 32 * e, 48, 2, 2, 70, 70, 8, SCALE, 1, None, 0)      # (row_ws: d_head 40 only)
        grp, = rec.of("cl_weight_grad_tn_group")
        assert grp[:2] == (BF16, 2) and [(d["M"], d["N"], d["K"], d["tap"]) for d in grp[2]] == [(140, 16, 4, -1), (140, 4, 16, -1)]
    else:
        assert rec.names() == (["cl_gemm", "cl_gemm"] + ["cl_transpose", "cl_transpose", "cl_weight_grad"] * 2
                               + ["cl_transpose"] * 3 + ["cl_attention_bwd", "cl_gemm"])
        qt, dot, kt = check_transposes(rec, dtype, [(dout.data_ptr(), 16, 2240, 1, 140, 16, 160), (to_.data_ptr(), 4, 560, 1, 140, 4, 160),
                                                    (rec.of("cl_gemm")[0][0]["C"], 4, 560, 1, 140, 4, 160), (a.data_ptr(), 16, 2240, 1, 140, 16, 160),
                                                    (q.data_ptr(), 48, 3360, 2, 70, 16, 128), (da, 16, 1120, 2, 70, 16, 128),
                                                    (k.data_ptr(), 48, 3360, 2, 70, 16, 128)])[4:]
        assert rec.scratch[4:] == [2 * 16 * 128 * 4] * 3
        bw, = rec.of("cl_attention_bwd")
        dq = bw[19]
        assert bw == (F32, q.data_ptr(), 48, k.data_ptr(), 48, v.data_ptr(), 48, a.data_ptr(), 16, da, 16, qt, dot, 128, kt, 128,
                      lse.data_ptr(), bw[17], 128, dq, 48, dq + 16 * e, 48, dq + 32 * e, 48, 2, 2, 70, 70, 8, SCALE, 0)
    assert bw[12 if bf else 17] not in (None, 0, lse.data_ptr())          # delta: a buffer of its own
    assert rec.of("cl_gemm")[-1][0]["A1"] == dq and rec.of("cl_gemm")[-1][0]["lda1"] == 48


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_cross_attention_fwd_bwd(rec, dtype):
    torch.manual_seed(1)
    bf = dtype == torch.bfloat16
    at = cross_attn(dtype)
    ctx = blocks.Ctx(dtype, CPU, True)
    x, cc = rnd(B * N, INNER, dtype), rnd(B * NKV, CTX_DIM, dtype)
    out, saved = at.fwd(ctx, x, cc, B, N, NKV, residual=x)
    xn, c, q, k, v, a, lse, tq, tk, tv, to_ = saved
    assert tuple(lse.shape) == (B, HEADS, 128)
    gq = rec.of("cl_gemm")[1][0]
    assert (gq["C"], gq["alpha"], gq["alpha_n"]) == (q.data_ptr(), f32(SCALE * 1.4426950408889634) if bf else 1.0, 0)
    if bf:
        assert rec.names() == ["cl_gemm"] * 6 + ["cl_attention_fwd_v2"] + ["cl_gemm"] * 2
        assert rec.of("cl_attention_fwd_v2") == [(BF16, q.data_ptr(), 16, k.data_ptr(), 16, v.data_ptr(), 16, a.data_ptr(), 16,
                                                  lse.data_ptr(), 128, 2, 2, 70, 77, 8, SCALE, 1, 0)]
    else:
        assert rec.names() == ["cl_gemm"] * 6 + ["cl_transpose", "cl_attention_fwd"] + ["cl_gemm"] * 2
        vt, = check_transposes(rec, dtype, [(v.data_ptr(), 16, 1232, 2, 77, 16, 128)])
        assert rec.scratch == [2 * 16 * 128 * 4]
        assert rec.of("cl_attention_fwd") == [(F32, q.data_ptr(), 16, k.data_ptr(), 16, vt, 128, a.data_ptr(), 16,
                                               lse.data_ptr(), 128, 2, 2, 70, 77, 8, SCALE, 0)]

    rec.clear()
    dout = rnd(B * N, INNER, dtype)
    at.bwd(ctx, dout, saved, B, N, NKV)
    ctx.flush_wgrad()
    da = rec.of("cl_gemm")[1][0]["C"]
    if bf:
        assert rec.names() == ["cl_gemm", "cl_gemm", "cl_attention_bwd_v2"] + ["cl_gemm"] * 4 + ["cl_weight_grad_tn_group"]
        bw, = rec.of("cl_attention_bwd_v2")
        dq, dk, dv = bw[14], bw[16], bw[18]
        assert bw == (BF16, q.data_ptr(), 16, k.data_ptr(), 16, v.data_ptr(), 16, a.data_ptr(), 16, da, 16, lse.data_ptr(), bw[12], 128,
                      dq, 16, dk, 16, dv, 16, 2, 2, 70, 77, 8, SCALE, 1, None, 0)
        grp, = rec.of("cl_weight_grad_tn_group")
        assert grp[:2] == (BF16, 8)
        assert [(d["dy"], d["x"], d["dW"], d["M"], d["N"], d["K"], d["scale"], d["tap"]) for d in grp[2]] == [
            (dout.data_ptr(), to_.data_ptr(), at.o.tB.grad.data_ptr(), 140, 16, 4, 1.0, -1),
            (rec.of("cl_gemm")[0][0]["C"], a.data_ptr(), at.o.tA.grad.data_ptr(), 140, 4, 16, 1.0, -1),
            (dq, tq.data_ptr(), at.q.tB.grad.data_ptr(), 140, 16, 4, 1.0, -1),
            (rec.of("cl_gemm")[2][0]["C"], xn.data_ptr(), at.q.tA.grad.data_ptr(), 140, 4, 16, 1.0, -1),
            (dk, tk.data_ptr(), at.k.tB.grad.data_ptr(), 154, 16, 4, 1.0, -1),
            (rec.of("cl_gemm")[4][0]["C"], c.data_ptr(), at.k.tA.grad.data_ptr(), 154, 4, 24, 1.0, -1),
            (dv, tv.data_ptr(), at.v.tB.grad.data_ptr(), 154, 16, 4, 1.0, -1),
            (rec.of("cl_gemm")[5][0]["C"], c.data_ptr(), at.v.tA.grad.data_ptr(), 154, 4, 24, 1.0, -1)]
    else:
        lora = ["cl_transpose", "cl_transpose", "cl_weight_grad"] * 2
        assert rec.names() == (["cl_gemm", "cl_gemm"] + lora + ["cl_transpose"] * 3 + ["cl_attention_bwd"] + ["cl_gemm", "cl_gemm"] + lora
                               + ["cl_gemm"] + lora + ["cl_gemm", "cl_transpose", "cl_transpose", "cl_weight_grad", "cl_transpose", "cl_weight_grad"])
        bw, = rec.of("cl_attention_bwd")
        dq, dk, dv = bw[19], bw[21], bw[23]
        gm = [g[0]["C"] for g in rec.of("cl_gemm")]        # uo, da, uq, dxn, uk, uv
        ts = check_transposes(rec, dtype, [
            (dout.data_ptr(), 16, 2240, 1, 140, 16, 160), (to_.data_ptr(), 4, 560, 1, 140, 4, 160),
            (gm[0], 4, 560, 1, 140, 4, 160), (a.data_ptr(), 16, 2240, 1, 140, 16, 160),
            (q.data_ptr(), 16, 1120, 2, 70, 16, 128), (da, 16, 1120, 2, 70, 16, 128), (k.data_ptr(), 16, 1232, 2, 77, 16, 128),
            (dq, 16, 2240, 1, 140, 16, 160), (tq.data_ptr(), 4, 560, 1, 140, 4, 160),
            (gm[2], 4, 560, 1, 140, 4, 160), (xn.data_ptr(), 16, 2240, 1, 140, 16, 160),
            (dk, 16, 2464, 1, 154, 16, 160), (tk.data_ptr(), 4, 616, 1, 154, 4, 160),
            (gm[4], 4, 616, 1, 154, 4, 160), (c.data_ptr(), 24, 3696, 1, 154, 24, 160),
            (dv, 16, 2464, 1, 154, 16, 160), (tv.data_ptr(), 4, 616, 1, 154, 4, 160),
            (gm[5], 4, 616, 1, 154, 4, 160)])
        assert rec.scratch[4:7] == [2 * 16 * 128 * 4] * 3
        assert bw == (F32, q.data_ptr(), 16, k.data_ptr(), 16, v.data_ptr(), 16, a.data_ptr(), 16, da, 16, ts[4], ts[5], 128, ts[6], 128,
                      lse.data_ptr(), bw[17], 128, dq, 16, dk, 16, dv, 16, 2, 2, 70, 77, 8, SCALE, 0)
        wg = rec.of("cl_weight_grad")
        assert wg == [(F32, ts[0], 160, ts[1], 160, at.o.tB.grad.data_ptr(), 4, 16, 4, 160, 1.0, 0),
                      (F32, ts[2], 160, ts[3], 160, at.o.tA.grad.data_ptr(), 16, 4, 16, 160, 1.0, 0),
                      (F32, ts[7], 160, ts[8], 160, at.q.tB.grad.data_ptr(), 4, 16, 4, 160, 1.0, 0),
                      (F32, ts[9], 160, ts[10], 160, at.q.tA.grad.data_ptr(), 16, 4, 16, 160, 1.0, 0),
                      (F32, ts[11], 160, ts[12], 160, at.k.tB.grad.data_ptr(), 4, 16, 4, 160, 1.0, 0),
                      (F32, ts[13], 160, ts[14], 160, at.k.tA.grad.data_ptr(), 24, 4, 24, 160, 1.0, 0),
                      (F32, ts[15], 160, ts[16], 160, at.v.tB.grad.data_ptr(), 4, 16, 4, 160, 1.0, 0),
                      (F32, ts[17], 160, ts[14], 160, at.v.tA.grad.data_ptr(), 24, 4, 24, 160, 1.0, 0)]      # c^T: the cached copy
    assert bw[12 if bf else 17] not in (None, 0, lse.data_ptr())


def test_bf16_backward_row_workspace_is_for_prescaled_d_head_40_only(rec, monkeypatch):
    """row_ws (32 bytes per lse slot) goes to cl_attention_bwd_v2 exactly when q is pre-scaled and d_head is 40."""
    dtype, heads, dh = torch.bfloat16, 2, 40
    for prescale, want_ws in ((True, True), (False, False)):
        monkeypatch.setattr(blocks, "PRESCALE_Q", prescale)
        at = blocks.AttnE(*(linear(heads * dh, heads * dh, dtype) for _ in range(4)), heads, True,
                          fused_qkv=linear(3 * heads * dh, heads * dh, dtype))
        ctx = blocks.Ctx(dtype, CPU, True)
        x = rnd(B * N, heads * dh, dtype)
        _, saved = at.fwd(ctx, x, None, B, N, N, residual=x)
        rec.clear()
        at.bwd(ctx, rnd(B * N, heads * dh, dtype), saved, B, N, N)
        bw, = rec.of("cl_attention_bwd_v2")
        assert bw[13] == 128 and bw[20:28] == (2, 2, 70, 70, 40, float(dh) ** -0.5, int(prescale), bw[27])
        assert (bw[27] is not None) == want_ws and rec.row_ws == [B * heads * 128 * 32 if want_ws else None]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_image_prompt_attention_fwd(rec, dtype):
    """Frozen UNet, inference: k | v and k_ip | v_ip are column blocks of [.., 32] products (row stride 32)."""
    torch.manual_seed(2)
    bf, e = dtype == torch.bfloat16, esz(dtype)
    at = cross_attn(dtype, r=0, fused_kv=True)
    at.kv_ip, at.ip_scale = linear(2 * INNER, CTX_DIM, dtype, bias=False), 0.5
    ctx = blocks.Ctx(dtype, CPU, False)
    x, cc, c_ip = rnd(B * N, INNER, dtype), rnd(B * NKV, CTX_DIM, dtype), rnd(B * NIP, CTX_DIM, dtype)
    k_ip, v_ip = at.project_ip(ctx, c_ip)
    assert (k_ip.stride(0), v_ip.data_ptr() - k_ip.data_ptr()) == (32, 16 * e)
    rec.clear()
    out, saved = at.fwd(ctx, x, cc, B, N, NKV, residual=x, ip=(k_ip, v_ip, NIP))
    assert saved is None
    gq, gkv, go = (g[0] for g in rec.of("cl_gemm"))
    q, k, a = gq["C"], gkv["C"], go["A1"]
    v = k + 16 * e
    assert (gq["ldc"], gkv["ldc"], gkv["N"], gkv["M"]) == (16, 32, 32, 154)
    assert (gq["alpha"], gq["alpha_n"]) == (f32(SCALE * 1.4426950408889634) if bf else 1.0, 0)
    if bf:
        assert rec.names() == ["cl_gemm", "cl_gemm", "cl_attention_fwd_ip", "cl_gemm"]
        assert rec.of("cl_attention_fwd_ip") == [(BF16, q, 16, k, 32, v, 32, k_ip.data_ptr(), 32, v_ip.data_ptr(), 32, a, 16,
                                                  2, 2, 70, 77, 4, 8, SCALE, 0.5, 1, 0)]
    else:
        assert rec.names() == ["cl_gemm", "cl_gemm", "cl_transpose", "cl_transpose", "cl_attention_fwd_ip", "cl_gemm"]
        vt, vt_ip = check_transposes(rec, dtype, [(v, 32, 2464, 2, 77, 16, 128), (v_ip.data_ptr(), 32, 128, 2, 4, 16, 64)])
        assert rec.scratch == [2 * 16 * 128 * 4, 2 * 16 * 64 * 4]
        assert rec.of("cl_attention_fwd_ip") == [(F32, q, 16, k, 32, vt, 128, k_ip.data_ptr(), 32, vt_ip, 64, a, 16,
                                                  2, 2, 70, 77, 4, 8, SCALE, 0.5, 0, 0)]
    # without a live image prompt the same call is the plain cross-attention
    at.ip_scale = 0.0
    rec.clear()
    at.fwd(ctx, x, cc, B, N, NKV, residual=x, ip=(k_ip, v_ip, NIP))
    assert rec.names() == (["cl_gemm", "cl_gemm", "cl_attention_fwd_v2", "cl_gemm"] if bf else
                           ["cl_gemm", "cl_gemm", "cl_transpose", "cl_attention_fwd", "cl_gemm"])
    assert rec.of("cl_attention_fwd_v2" if bf else "cl_attention_fwd")[0][9:11] == (None, 0)      # no lse without a backward


# --------------------------------------------------------------------------- weight gradients

def group_rows(rec, n):
    grp, = rec.of("cl_weight_grad_tn_group")
    assert grp[:2] == (BF16, n) and grp[4] == 0 and grp[3] == hip.zero_page(CPU).data_ptr()
    return grp[2]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_linear_bwd_lora(rec, dtype):
    torch.manual_seed(3)
    M = B * N
    L = linear(32, 16, dtype, r=R)
    ctx = blocks.Ctx(dtype, CPU, True)
    x, t, dy, u = rnd(M, 16, dtype), rnd(M, R, dtype), rnd(M, 32, dtype), rnd(M, R, dtype)
    blocks.linear_bwd_lora(ctx, L, x, t, dy, u)
    if dtype == torch.bfloat16:
        assert rec.names() == []                         # queued: one grouped launch per block
        ctx.flush_wgrad()
        assert rec.names() == ["cl_weight_grad_tn_group"]
        rows = group_rows(rec, 2)
        want = dict(lddy=32, ldx=4, lddw=4, M=140, N=32, K=4, scale=1.0, tap=-1, dy=dy.data_ptr(), x=t.data_ptr(), dW=L.tB.grad.data_ptr())
        assert {f: rows[0][f] for f in want} == want
        want = dict(lddy=4, ldx=16, lddw=16, M=140, N=4, K=16, scale=1.0, tap=-1, dy=u.data_ptr(), x=x.data_ptr(), dW=L.tA.grad.data_ptr())
        assert {f: rows[1][f] for f in want} == want
    else:
        assert rec.names() == ["cl_transpose", "cl_transpose", "cl_weight_grad"] * 2
        ts = check_transposes(rec, dtype, [(dy.data_ptr(), 32, 4480, 1, 140, 32, 160), (t.data_ptr(), 4, 560, 1, 140, 4, 160),
                                           (u.data_ptr(), 4, 560, 1, 140, 4, 160), (x.data_ptr(), 16, 2240, 1, 140, 16, 160)])
        assert rec.scratch == [32 * 160 * 4, 4 * 160 * 4, 4 * 160 * 4, 16 * 160 * 4]
        assert rec.of("cl_weight_grad") == [(F32, ts[0], 160, ts[1], 160, L.tB.grad.data_ptr(), 4, 32, 4, 160, 1.0, 0),
                                            (F32, ts[2], 160, ts[3], 160, L.tA.grad.data_ptr(), 16, 4, 16, 160, 1.0, 0)]
        ctx.flush_wgrad()
        assert len(rec.calls) == 6                       # nothing was queued
    rec.clear()
    blocks.linear_bwd_lora(ctx, linear(32, 16, dtype), x, None, dy, None)      # no LoRA: nothing to do
    ctx.flush_wgrad()
    assert rec.names() == []


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_dense_bwd_weight(rec, dtype):
    torch.manual_seed(4)
    M = B * N
    L = linear(32, 16, dtype)
    tW, tb = Trainable("w", (32, 16, 1, 1)), Trainable("b", (32,))
    for t in (tW, tb):
        t.master, t.grad = torch.zeros(t.shape), torch.zeros(t.shape)
    L.attach_trainable_weight(tW, tb)
    ctx = blocks.Ctx(dtype, CPU, True)
    x, dy = rnd(M, 16, dtype), rnd(M, 32, dtype)
    blocks.dense_bwd_weight(ctx, L, x, dy, B, N, 0.25)
    ctx.flush_wgrad()
    colsum = (hip.dt_of(dtype), dy.data_ptr(), 32, tb.grad.data_ptr(), 32, 1, 140, 32, 0.25, 0)
    if dtype == torch.bfloat16:
        assert rec.names() == ["cl_colsum", "cl_weight_grad_tn_group"]
        row, = group_rows(rec, 1)
        want = dict(lddy=32, ldx=16, lddw=16, M=140, N=32, K=16, scale=0.25, tap=-1, dy=dy.data_ptr(), x=x.data_ptr(), dW=tW.grad.data_ptr())
        assert {f: row[f] for f in want} == want
    else:
        assert rec.names() == ["cl_transpose", "cl_transpose", "cl_weight_grad", "cl_colsum"]
        ts = check_transposes(rec, dtype, [(dy.data_ptr(), 32, 4480, 1, 140, 32, 160), (x.data_ptr(), 16, 2240, 1, 140, 16, 160)])
        assert rec.scratch == [32 * 160 * 4, 16 * 160 * 4]
        assert rec.of("cl_weight_grad") == [(F32, ts[0], 160, ts[1], 160, tW.grad.data_ptr(), 16, 32, 16, 160, 0.25, 0)]
    assert rec.of("cl_colsum") == [colsum]


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_conv3_bwd_weight(rec, dtype, stride):
    """Cin = Cout = 32 on a 6 x 6 grid: nine single-tap problems (the row-of-three form needs Win % 64 == 0)."""
    torch.manual_seed(5)
    Cc, Hin = 32, 6
    Ho = Hin // stride
    Mo, Mp = B * Ho * Ho, {1: 96, 2: 32}[stride]          # 72 -> 96 rows, 18 -> 32
    cw = Conv3W(torch.randn(Cc, Cc, 3, 3), torch.randn(Cc), dtype, CPU, True)
    tW, tb = Trainable("w", (Cc, 9 * Cc), conv=(Cc, Cc, Cc)), Trainable("b", (Cc,))
    for t in (tW, tb):
        t.master, t.grad = torch.zeros(t.shape), torch.zeros(t.shape)
    cw.attach_trainable(tW, tb)
    ctx = blocks.Ctx(dtype, CPU, True)
    x, dy = rnd(B * Hin * Hin, Cc, dtype), rnd(Mo, Cc, dtype)
    blocks.conv3_bwd_weight(ctx, cw, x, dy, B, Hin, Hin, mode=hip.CONV_S2 if stride == 2 else hip.CONV_S1)
    ctx.flush_wgrad()
    gw = tW.grad.data_ptr()
    assert rec.of("cl_colsum") == [(hip.dt_of(dtype), dy.data_ptr(), 32, tb.grad.data_ptr(), 32, 1, Mo, 32, 1.0, 0)]
    if dtype == torch.bfloat16:
        assert rec.names() == ["cl_colsum", "cl_weight_grad_tn_group"]
        rows = group_rows(rec, 9)
        for t, d in enumerate(rows):
            want = dict(dy=dy.data_ptr(), lddy=32, x=x.data_ptr(), ldx=32, dW=gw + t * 32 * 4, lddw=288, M=Mo, N=32, K=32, scale=1.0,
                        tap=t, Hin=6, Win=6, Hout=Ho, Wout=Ho, stride=stride, pad=1)
            assert {f: d[f] for f in want} == want
    else:
        assert rec.names() == (["cl_conv_tap_gather", "cl_transpose", "cl_transpose", "cl_weight_grad"]
                               + ["cl_conv_tap_gather", "cl_transpose", "cl_weight_grad"] * 8 + ["cl_colsum"])
        gathers = rec.of("cl_conv_tap_gather")
        xs = [g[3] for g in gathers]
        assert len(set(xs)) == 9                         # every tap's operand stays alive while its transpose is cached
        for t, g in enumerate(gathers):
            assert g == (F32, x.data_ptr(), 32, xs[t], 32, 2, 6, 6, Ho, Ho, 32, t, stride, 1, 0)
            assert rec.allocs[xs[t]] >= Mo * 32 * 4
        ts = check_transposes(rec, dtype, [(dy.data_ptr(), 32, Mo * 32, 1, Mo, 32, Mp)] + [(p, 32, Mo * 32, 1, Mo, 32, Mp) for p in xs])
        assert rec.scratch == [32 * Mp * 4] * 10
        assert rec.of("cl_weight_grad") == [(F32, ts[0], Mp, ts[1 + t], Mp, gw + t * 32 * 4, 288, 32, 32, Mp, 1.0, 0) for t in range(9)]


def test_frozen_conv_has_no_weight_gradient(rec):
    cw = Conv3W(torch.randn(32, 32, 3, 3), torch.randn(32), torch.float32, CPU, True)
    ctx = blocks.Ctx(torch.float32, CPU, True)
    blocks.conv3_bwd_weight(ctx, cw, rnd(72, 32, torch.float32), rnd(72, 32, torch.float32), B, 6, 6)
    ctx.flush_wgrad()
    assert rec.calls == []


# --------------------------------------------------------------------------- CLIP vision encoder

def clip_state(cfg):
    D, F, P, Cn = cfg["hidden_size"], cfg["intermediate_size"], cfg["patch_size"], cfg["num_channels"]
    T = (cfg["image_size"] // P) ** 2 + 1
    shape = {"embeddings.class_embedding": (D,), "embeddings.patch_embedding.weight": (D, Cn, P, P),
             "embeddings.position_embedding.weight": (T, D), "visual_projection.weight": (cfg["projection_dim"], D),
             "mlp.fc1.weight": (F, D), "mlp.fc1.bias": (F,), "mlp.fc2.weight": (D, F)}
    sd = {}
    for key in vit.state_keys(cfg):
        s = next((v for k, v in shape.items() if key.endswith(k)), None)
        sd[key] = torch.randn(s if s is not None else ((D, D) if key.endswith("_proj.weight") else (D,)))
    return sd


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_clip_vision_forward(rec, dtype):
    """One layer of the TINY encoder: D = 160, 2 heads of 80, T = 26 tokens (pads to 64), q | k | v blocks of a [52, 480] product."""
    torch.manual_seed(6)
    bf, e = dtype == torch.bfloat16, esz(dtype)
    cfg = dict(TINY, num_hidden_layers=1)
    enc = vit.ClipVisionE(clip_state(cfg), cfg, dtype, device="cpu")
    px = torch.randn(B, 3, 70, 70)
    rec.clear()
    enc.forward(px)
    first = list(rec.calls)
    attn = ["cl_attention_fwd_v2"] if bf else ["cl_transpose", "cl_attention_fwd"]
    assert rec.names() == (["cl_vit_patch_rows", "cl_gemm", "cl_vit_tokens", "cl_layernorm_fwd"]
                           + ["cl_layernorm_fwd", "cl_gemm"] + attn + ["cl_gemm", "cl_layernorm_fwd", "cl_gemm", "cl_gemm"]
                           + ["cl_layernorm_fwd", "cl_gemm"])
    gqkv, go = rec.of("cl_gemm")[1][0], rec.of("cl_gemm")[2][0]
    q, a = gqkv["C"], go["A1"]
    k, v = q + 160 * e, q + 320 * e
    sc = 80.0 ** -0.5
    assert (gqkv["M"], gqkv["N"], gqkv["K1"], gqkv["ldc"]) == (52, 480, 160, 480)
    assert (gqkv["alpha"], gqkv["alpha_n"]) == ((f32(sc * 1.4426950408889634), 160) if bf else (1.0, 0))
    if bf:
        assert rec.of("cl_attention_fwd_v2") == [(BF16, q, 480, k, 480, v, 480, a, 160, None, 0, 2, 2, 26, 26, 80, sc, 1, 0)]
    else:
        vt, = check_transposes(rec, dtype, [(v, 480, 12480, 2, 26, 160, 64)])
        assert rec.scratch == [2 * 160 * 64 * 4]
        assert rec.of("cl_attention_fwd") == [(F32, q, 480, k, 480, vt, 64, a, 160, None, 0, 2, 2, 26, 26, 80, sc, 0)]
    # a forward is a fixed launch sequence over fixed addresses: the second one repeats the first call for call
    rec.clear()
    enc.forward(px)
    assert rec.calls == first
