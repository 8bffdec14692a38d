"""Kernel-level conformance of csrc/elementwise.hip (ctypes -> C ABI): every row of the case table of tests/ew_ref.py, element-wise
against the fp64 contract.

Per row and dtype the call is launched twice into fresh buffers.  After every launch the probe cl_debug_ew_last_launch must report
what the transcription of the launchers (ew_ref: ew_grid, colsum_form, zero_form, vit_pair, mse_blocks) predicts, and

  * the exact tier is compared bit for bit, the gated tier element-wise (|got - ref| <= u |ref| + fixed + c e mag, zero violations);
  * the canary holds: every output is a NaN-filled (or initialised, where the kernel accumulates) view into a buffer of a fixed
    bit pattern -- guard rows, pad columns, guard elements -- every operand a padded copy with a leading dimension of its own whose
    pad holds NaN (so does the gap between the batches of a transpose source and between the matrices of the repack master: a
    pad value that reaches an output, even through a product with zero or a masked lane, shows), and any workspace and the
    p_losses scratch are NaN-filled; afterwards no guard, pad or operand changed and no NaN is left in an output;
  * the two launches give the same bits (not the atomic colsum path and cl_mse_loss, which are gated only).

bf16 rows of the strided vector-8 kernels run again as column slices, starting at a nonzero multiple of 8, of wider buffers.  There
the other columns hold PAD_FILL (1e3), not NaN: in the engine's concat buffers they are a neighbour's finite data, and a kernel that
walks a slice with the wrong leading dimension or offset reads exactly such values.
"""
import ctypes
import json
import time

import pytest
import torch

from tests import ew_ref as R
from tests.gemm_ref import _pattern
from tests.test_gpu_bench_shapes import _need_gpu, _record

pytestmark = pytest.mark.gpu

BF, F32 = R.BF, R.F32
DEV = "cuda"
G = 64                       # guard elements either side of a flat output
NAN = float("nan")
_STATS = dict(cases=0, launches=0, violations=0, exact_mismatch=0, canary=0, form_mismatch=0, rerun_diff=0)
_T0 = [None]
_CANARY = {torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A, torch.uint8: 0xA5}


def _probe():
    from ctrlora_amd import hip
    out = (ctypes.c_int * 8)()
    assert hip.lib().cl_debug_ew_last_launch(out) == 0
    return dict(zip(R.PROBE_FIELDS, list(out)))


def _D(dt):
    return 0 if dt == BF else 1


class _Out:
    """An output view of any shape / strides inside a flat buffer of a fixed bit pattern (G guard elements either side); the view holds
    `init` (NaN = must be written; a tensor = what an accumulating kernel starts from)."""

    def __init__(self, shape, dtype, strides=None, init=NAN, extra=0):
        shape = tuple(shape)
        if strides is None:
            strides, s = [], 1
            for n in reversed(shape):
                strides.insert(0, s)
                s *= n
        span = 1 + sum((n - 1) * s for n, s in zip(shape, strides)) if all(shape) else 0
        if dtype in (BF, F32):
            it, pat = _pattern(dtype)
            self.raw = torch.full((span + extra + 2 * G,), pat, dtype=it, device=DEV)
            self.buf = self.raw.view(dtype)
        else:
            it, pat = dtype, _CANARY[dtype]
            self.raw = self.buf = torch.full((span + extra + 2 * G,), pat, dtype=dtype, device=DEV)
        self.pat = pat
        self.view = torch.as_strided(self.buf, shape, strides, G)
        self.mask = torch.ones(self.raw.shape, dtype=torch.bool, device=DEV)
        torch.as_strided(self.mask, shape, strides, G).fill_(False)
        if torch.is_tensor(init):
            self.view.copy_(init)
        else:
            self.view.fill_(init if dtype in (BF, F32) else 0x33)

    def guards(self):
        return int((self.raw[self.mask] != self.pat).sum())

    def bad(self):
        return self.guards() + (int(torch.isnan(self.view).sum()) if self.view.is_floating_point() else 0)


class _G2:
    """tests/gemm_ref.Guarded behind the same interface."""

    def __init__(self, M, cols, dtype, j=1, init=NAN):
        self.g = R.Guarded(M, cols, dtype, DEV, fill=NAN if torch.is_tensor(init) else init, j=j)
        self.view, self.buf = self.g.view, self.g.buf
        if torch.is_tensor(init):
            self.view.copy_(init)

    def bad(self):
        c = self.g.check()
        return c["guard_rows"] + c["pad_elems"] + c["nan_left"]


class _Slice2:
    """An [M, C] output as a column slice at `off` (a nonzero multiple of 8) of a [M + 2 guard rows, C + 320] buffer of PAD_FILL."""

    def __init__(self, M, C, dtype, off, init=NAN):
        self.buf = torch.full((M + 2 * R.GUARD_ROWS, C + 320), R.PAD_FILL, dtype=dtype, device=DEV)
        self.view = self.buf[R.GUARD_ROWS:R.GUARD_ROWS + M, off:off + C]
        if torch.is_tensor(init):
            self.view.copy_(init)
        else:
            self.view.fill_(init)
        self.mask = torch.ones_like(self.buf, dtype=torch.bool)
        self.mask[R.GUARD_ROWS:R.GUARD_ROWS + M, off:off + C] = False

    def bad(self):
        return int((self.buf[self.mask] != R.PAD_FILL).sum()) + int(torch.isnan(self.view).sum())


class _Ctx:
    def __init__(self, lay="pad"):
        self.lay, self.ops, self.outs, self.call, self.want, self.nondet, self.nslice = lay, [], {}, None, None, False, 0

    def IN(self, t, pad=8, fill=NAN):
        """A 2-D operand with a leading dimension of its own (pad layout) or as a column slice of a wider buffer (slice layout)."""
        t = t.to(DEV)
        if self.lay == "slice":
            self.nslice += 1
            off = 8 * (2 * self.nslice + 1)
            buf = torch.full((t.shape[0], t.shape[1] + 320), R.PAD_FILL, dtype=t.dtype, device=DEV)
            v = buf[:, off:off + t.shape[1]]
        else:
            buf = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=t.dtype, device=DEV)
            v = buf[:, :t.shape[1]]
        v.copy_(t)
        self.ops.append(buf)
        return v

    def FLAT(self, t):
        t = t.to(DEV).contiguous().clone()
        self.ops.append(t)
        return t

    def OUT(self, name, M, cols, dt, j=1, init=NAN):
        if self.lay == "slice":
            self.nslice += 1
            h = _Slice2(M, cols, dt, 8 * (2 * self.nslice + 1), init)
        else:
            h = _G2(M, cols, dt, j, init)
        self.outs[name] = h
        return h.view

    def OUTF(self, name, shape, dt, init=NAN, strides=None, extra=0):
        h = _Out(shape, dt, strides, init, extra)
        self.outs[name] = h
        return h.view


def _lib():
    from ctrlora_amd import hip
    return hip.lib(), hip.stream()


def _p(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------ one prep per kernel

def prep_geglu_fwd(row, dt, ops, lay):
    L, st = _lib()
    p, c = row["p"], _Ctx(lay)
    h, out = c.IN(ops["h"], 8), c.OUT("out", p["M"], p["F"], dt, 4)
    c.call = lambda: L.cl_geglu_fwd(_D(dt), _p(h), h.stride(0), _p(out), out.stride(0), p["M"], p["F"], st)
    c.want = R.probe("geglu_fwd", dt, (R.ew_grid(p["M"] * (p["F"] // 8)),))
    return c


def prep_geglu_bwd(row, dt, ops, lay):
    L, st = _lib()
    p, c = row["p"], _Ctx(lay)
    h, d, dh = c.IN(ops["h"], 8), c.IN(ops["dout"], 16), c.OUT("dh", p["M"], 2 * p["F"], dt, 3)
    c.call = lambda: L.cl_geglu_bwd(_D(dt), _p(h), h.stride(0), _p(d), d.stride(0), _p(dh), dh.stride(0), p["M"], p["F"], st)
    c.want = R.probe("geglu_bwd", dt, (R.ew_grid(p["M"] * (p["F"] // 8)),))
    return c


def prep_silu_fwd(row, dt, ops, lay):
    L, st = _lib()
    p, c = row["p"], _Ctx()
    n = p["M"] * p["C"]
    x, y = c.FLAT(ops["x"]), c.OUTF("y", (p["M"], p["C"]), dt)
    c.call = lambda: L.cl_silu_fwd(_D(dt), _p(x), _p(y), n, st)
    c.want = R.probe("silu_fwd", dt, (R.ew_grid(n // 8),))
    return c


def prep_silu_bwd(row, dt, ops, lay):
    L, st = _lib()
    p, c = row["p"], _Ctx()
    n = p["M"] * p["C"]
    x, dy, dx = c.FLAT(ops["x"]), c.FLAT(ops["dy"]), c.OUTF("dx", (p["M"], p["C"]), dt)
    c.call = lambda: L.cl_silu_bwd(_D(dt), _p(x), _p(dy), _p(dx), n, st)
    c.want = R.probe("silu_bwd", dt, (R.ew_grid(n // 8),))
    return c


def prep_axpby(row, dt, ops, lay):
    L, st = _lib()
    p, c = row["p"], _Ctx(lay)
    x = c.IN(ops["x"], 16)
    y = c.OUT("y", p["M"], p["C"], dt, 2, init=NAN if p["b"] == 0.0 else ops["y"].to(DEV))
    c.call = lambda: L.cl_axpby(_D(dt), _p(x), x.stride(0), _p(y), y.stride(0), p["M"], p["C"], p["a"], p["b"], st)
    c.want = R.probe("axpby", dt, (R.ew_grid(p["M"] * (p["C"] // 8)),))
    return c


def prep_pool2x2(row, dt, ops, lay):
    L, st = _lib()
    p, c = row["p"], _Ctx(lay)
    rows = p["B"] * p["H"] * p["W"]
    x = c.IN(ops["in"], 24)
    out = c.OUT("out", rows, p["C"], dt, 2, init=ops["out0"].to(DEV) if p["acc"] else NAN)
    c.call = lambda: L.cl_pool2x2(_D(dt), _p(x), x.stride(0), _p(out), out.stride(0), p["B"], p["H"], p["W"], p["C"], p["acc"], st)
    c.want = R.probe("pool2x2", dt, (R.ew_grid(rows * (p["C"] // 8)),))
    return c


def prep_conv_tap(row, dt, ops, lay):
    L, st = _lib()
    p, c = row["p"], _Ctx(lay)
    rows = p["B"] * p["Hout"] * p["Wout"]
    x, out = c.IN(ops["x"], 8), c.OUT("out", rows, p["C"], dt, 3)
    c.call = lambda: L.cl_conv_tap_gather(_D(dt), _p(x), x.stride(0), _p(out), out.stride(0), p["B"], p["Hin"], p["Win"], p["Hout"], p["Wout"],
                                          p["C"], p["tap"], p["stride"], p["pad"], st)
    c.want = R.probe("conv_tap", dt, (R.ew_grid(rows * (p["C"] // 8)),))
    return c


def prep_vit_tokens(row, dt, ops, lay):
    L, st = _lib()
    p, c = row["p"], _Ctx(lay)
    patch, cls, pos = c.IN(ops["patch"], 8), c.FLAT(ops["cls"]), c.FLAT(ops["pos"])
    out = c.OUT("out", p["B"] * p["T"], p["D"], dt, 2)
    c.call = lambda: L.cl_vit_tokens(_D(dt), _p(patch), patch.stride(0), _p(cls), _p(pos), _p(out), out.stride(0), p["B"], p["T"], p["D"], st)
    c.want = R.probe("vit_tokens", dt, (R.ew_grid(p["B"] * p["T"] * (p["D"] // 8)),))
    return c


def prep_vit_patch_rows(row, dt, ops, lay):
    L, st = _lib()
    p, c = row["p"], _Ctx(lay)
    Gd = p["S"] // p["P"]
    px, out = c.FLAT(ops["px"]), c.OUT("out", p["B"] * Gd * Gd, p["Kpad"], dt, 2)
    c.call = lambda: L.cl_vit_patch_rows(_D(dt), _p(px), _p(out), out.stride(0), p["B"], p["C"], p["S"], p["P"], p["Kpad"], st)
    c.want = R.probe("vit_patch_rows", dt, (R.ew_grid(p["B"] * Gd * Gd * (p["Kpad"] // 8)),), form=int(R.vit_pair(p["P"], p["S"])))
    return c


def prep_transpose(row, dt, ops, lay):
    L, st = _lib()
    p, c = row["p"], _Ctx()
    Bt, Rr, C, Rpad = p["Bt"], p["R"], p["C"], p["Rpad"]
    ldi = C + 3
    bsi = Rr * ldi + 5                                                      # bsi != R ldi
    src = torch.full((Bt * bsi,), NAN, dtype=p["idt"], device=DEV)
    torch.as_strided(src, (Bt, Rr, C), (bsi, ldi, 1)).copy_(ops["in"].to(DEV))
    c.ops.append(src)
    ldo = Rpad + 8
    bso = C * ldo + 16
    out = c.OUTF("out", (Bt, C, Rpad), p["odt"], strides=(bso, ldo, 1))
    c.call = lambda: L.cl_transpose(_D(p["idt"]), _D(p["odt"]), _p(src), ldi, bsi, _p(out), ldo, bso, Bt, Rr, C, Rpad, st)
    c.want = R.probe("transpose", p["odt"], R.tile_grid(Rpad, C, Bt), form=_D(p["idt"]))
    return c


def prep_nchw_to_tok(row, dt, ops, lay):
    L, st = _lib()
    p, c = row["p"], _Ctx()
    x, out = c.FLAT(ops["in"]), c.OUT("out", p["B"] * p["HW"], p["Cpad"], dt, 2)
    c.call = lambda: L.cl_nchw_to_tok(_D(dt), _p(x), _p(out), out.stride(0), p["B"], p["Cin"], p["Cpad"], p["HW"], st)
    c.want = R.probe("nchw_to_tok", dt, R.tile_grid(p["HW"], p["Cpad"], p["B"]))
    return c


def prep_tok_to_nchw(row, dt, ops, lay):
    L, st = _lib()
    p, c = row["p"], _Ctx()
    x = c.IN(ops["in"], 3)
    out = c.OUTF("out", (p["B"], p["C"], p["HW"]), F32, init=NAN if p["beta"] == 0.0 else ops["out0"].to(DEV))
    c.call = lambda: L.cl_tok_to_nchw(_D(dt), _p(x), x.stride(0), _p(out), p["B"], p["C"], p["HW"], p["alpha"], p["beta"], st)
    c.want = R.probe("tok_to_nchw", dt, R.tile_grid(p["HW"], p["C"], p["B"]))
    return c


def prep_pack2d(row, dt, ops, lay):
    L, st = _lib()
    p, c = row["p"], _Ctx()
    x, out = c.IN(ops["in"], 3), c.OUT("out", p["R"], p["Cpad"], dt, 2)
    c.call = lambda: L.cl_pack2d(_D(dt), _p(x), x.stride(0), _p(out), out.stride(0), p["R"], p["C"], p["Cpad"], st)
    c.want = R.probe("pack2d", dt, (R.ew_grid(p["R"] * p["Cpad"]),))
    return c


def prep_repack(row, dt, ops, lay):
    L, st = _lib()
    p, c = row["p"], _Ctx()
    offs, off = [], 7
    for m in p["mats"]:
        offs.append(off)
        off += m["R"] * (m["sld"] or m["C"]) + 5
    flat = torch.full((off,), NAN, dtype=F32, device=DEV)
    desc, prefix = [], [0]
    for i, m in enumerate(p["mats"]):
        Rr, C, sld = m["R"], m["C"], m["sld"] or m["C"]
        torch.as_strided(flat, (Rr, C), (sld, 1), offs[i]).copy_(ops[f"src{i}"].to(DEV))
        d = c.OUT(f"dst{i}", Rr, C, dt, 1 + i % 3)
        dT = c.OUT(f"dstT{i}", C, Rr, dt, 2 + i % 2) if m["T"] else None
        desc.append([offs[i], (Rr << 32) | C, _p(d), _p(dT) or 0, m["sld"], d.stride(0), dT.stride(0) if m["T"] else 0, 0])
        prefix.append(prefix[-1] + ((Rr + 31) // 32) * ((C + 31) // 32))
    c.ops.append(flat)
    dd = c.FLAT(torch.tensor(desc, dtype=torch.long))
    pf = c.FLAT(torch.tensor(prefix, dtype=torch.int32))
    c.call = lambda: L.cl_repack(_D(dt), _p(flat), _p(dd), _p(pf), len(desc), prefix[-1], st)
    c.want = R.probe("repack", dt, (prefix[-1],))
    return c


def prep_softmax(row, dt, ops, lay):
    L, st = _lib()
    p, c = row["p"], _Ctx()
    S = c.IN(ops["S"], 4, fill=NAN)
    P = c.OUT("P", p["M"], p["N"], dt, 2)
    c.call = lambda: L.cl_softmax_rows(_D(dt), _p(S), S.stride(0), _p(P), P.stride(0), p["M"], p["N"], p["scale"], st)
    c.want = R.probe("softmax", dt, (p["M"],))
    return c


def prep_colsum(row, dt, ops, lay):
    from ctrlora_amd import hip
    L, st = _lib()
    p, c = row["p"], _Ctx()
    x = c.IN(ops["in"], 16)
    out = c.OUT("out", p["B"], p["C"], F32, 2, init=ops["out0"].to(DEV))
    f = R.colsum_form(p["B"], p["HW"], p["C"], hip.WORKSPACE_BYTES if p["ws"] else 0)
    c.call = lambda: L.cl_colsum(_D(dt), _p(x), x.stride(0), _p(out), out.stride(0), p["B"], p["HW"], p["C"], p["scale"], st)
    c.want = R.probe("colsum", dt, (f["nchunk"], p["B"]), form=1 if f["partial"] else 2, aux=f["nchunk"])
    c.nondet = not f["partial"] and f["nchunk"] > 1
    return c


def prep_mse(row, dt, ops, lay):
    L, st = _lib()
    p, c = row["p"], _Ctx()
    e, t = c.FLAT(ops["eps"]), c.FLAT(ops["target"])
    loss = c.OUTF("loss", (1,), F32)
    d = c.OUTF("d_eps", (p["n"],), F32) if p["d_eps"] else None
    c.call = lambda: L.cl_mse_loss(_p(e), _p(t), _p(d), _p(loss), p["n"], p["gscale"], st)
    c.want = R.probe("mse", None, (R.mse_blocks(p["n"]),), aux=R.mse_blocks(p["n"]))
    c.nondet = True
    return c


def prep_plosses(row, dt, ops, lay):
    L, st = _lib()
    p, c = row["p"], _Ctx()
    e, t = c.FLAT(ops["eps"]), c.FLAT(ops["target"])
    ts, lv = c.FLAT(ops["t"]), c.FLAT(ops["lvlb"])
    out = c.OUTF("out", (3,), F32)
    ps = c.OUTF("per_sample", (p["B"],), F32) if p["per_sample"] else None
    d = c.OUTF("d_eps", (p["B"], p["per"]), F32) if p["d_eps"] else None
    scratch = c.OUTF("scratch", (16 * p["B"],), F32)
    c.call = lambda: L.cl_p_losses_mse(_p(e), _p(t), _p(d), _p(ts), _p(lv) if p["lvlb"] else None, _p(out), _p(ps), _p(scratch), p["B"], p["per"],
                                       p["gscale"], p["w_simple"], p["w_elbo"], st)
    c.want = R.probe("plosses", None, (16, p["B"]))
    return c


def prep_qsample(row, dt, ops, lay):
    L, st = _lib()
    p, c = row["p"], _Ctx()
    z, nz, t, a, b = (c.FLAT(ops[k]) for k in ("z", "noise", "t", "sqrt_ac", "sqrt_1mac"))
    out = c.OUTF("out", (p["B"], p["per"]), F32)
    c.call = lambda: L.cl_qsample(_p(z), _p(nz), _p(t), _p(a), _p(b), _p(out), p["B"], p["per"], st)
    c.want = R.probe("qsample", None, (R.ew_grid(p["B"] * p["per"]),))
    return c


def prep_ddim(row, dt, ops, lay, cursor=None):
    """cursor = None: the host-index form; an int: the device-cursor form with that cursor."""
    L, st = _lib()
    p, c = row["p"], _Ctx()
    n = p["n"]
    ec, coef = c.FLAT(ops["e_c"]), c.FLAT(ops["coef"])
    eu = c.FLAT(ops["e_u"]) if p["e_u"] else None
    nz = c.FLAT(ops["noise"]) if p["noise"] else None
    if p["alias"]:
        xp = x = c.OUTF("x_prev", (n,), F32, init=ops["x"].to(DEV))
    else:
        x, xp = c.FLAT(ops["x"]), c.OUTF("x_prev", (n,), F32)
    p0 = c.OUTF("pred_x0", (n,), F32) if p["pred_x0"] else None
    if cursor is None:
        c.call = lambda: L.cl_ddim_step(_p(x), _p(ec), _p(eu), _p(nz), _p(coef), p["index"], p["scale"], _p(xp), _p(p0), n, st)
        c.want = R.probe("ddim_step", None, (R.ew_grid(n),))
    else:
        cur = c.FLAT(torch.tensor([cursor], dtype=torch.int32))
        c.call = lambda: L.cl_ddim_step_dev(_p(x), _p(ec), _p(eu), _p(nz), _p(coef), _p(cur), p["S"], p["scale"], _p(xp), _p(p0), n, st)
        c.want = R.probe("ddim_step_dev", None, (R.ew_grid(n),))
    return c


PREP = dict(geglu_fwd=prep_geglu_fwd, geglu_bwd=prep_geglu_bwd, silu_fwd=prep_silu_fwd, silu_bwd=prep_silu_bwd, axpby=prep_axpby,
            pool2x2=prep_pool2x2, conv_tap=prep_conv_tap, vit_tokens=prep_vit_tokens, vit_patch_rows=prep_vit_patch_rows,
            transpose=prep_transpose, nchw_to_tok=prep_nchw_to_tok, tok_to_nchw=prep_tok_to_nchw, pack2d=prep_pack2d, repack=prep_repack,
            softmax=prep_softmax, colsum=prep_colsum, mse=prep_mse, plosses=prep_plosses, qsample=prep_qsample, ddim_step=prep_ddim)
SLICED = ("geglu_fwd", "geglu_bwd", "axpby", "pool2x2", "conv_tap", "vit_tokens", "vit_patch_rows")


# ------------------------------------------------------------------------------------------------ the harness

def _launch(c):
    """Launch a prepared call once: (canary count, probe)."""
    snap = [R.bits(b).clone() for b in c.ops]
    rc = c.call()
    assert rc == 0, ("return code", rc)
    pr = _probe()
    torch.cuda.synchronize()
    canary = sum(h.guards() if k == "scratch" else h.bad() for k, h in c.outs.items())      # (scratch: empty chunks may stay unwritten)
    canary += sum(int((R.bits(b) != s).sum()) for b, s in zip(c.ops, snap))
    _STATS["launches"] += 1
    return canary, pr


def _judge(name, tag, specs, got, canary, pr, want, bad):
    res = R.check(specs, got)
    f = R.failures(res)
    mism = {k: (pr[k], v) for k, v in want.items() if pr[k] != v} if want is not None else {}
    _STATS["violations"] += sum(r.get("violations", 0) for r in res.values())
    _STATS["exact_mismatch"] += sum(abs(r.get("exact_mismatch", 0)) for r in res.values())
    _STATS["canary"] += canary
    _STATS["form_mismatch"] += bool(mism)
    eob = {k: r["err_over_bound"] for k, r in res.items() if "err_over_bound" in r}
    for k, v in eob.items():
        key = "eob_" + (specs[k]["fam"] or "timestep")
        _STATS[key] = max(_STATS.get(key, 0.0), v)
    if f or canary or mism or set(specs) - set(res):
        bad.append((name, tag, dict(failures=f, canary=canary, form_mismatch=mism, missing=sorted(set(specs) - set(res)))))
    _record("ew_conformance", row=name, launch=tag, eob=eob)


def _run_generic(row, dt, lay="pad"):
    bad = []
    ops = R.make_ops(row, dt, DEV)
    specs = R.evaluate(row, dt, ops)
    runs = []
    for rep in range(2):
        c = PREP[row["kern"]](row, dt, ops, lay)
        canary, pr = _launch(c)
        runs.append((c, canary, pr))
    c, canary, pr = runs[0]
    got = {k: h.view for k, h in c.outs.items()}
    _judge(row["name"], lay, specs, got, canary + runs[1][1], pr, c.want, bad)
    if runs[1][2] != pr:
        bad.append((row["name"], lay, "probe differs between two launches"))
    if not c.nondet:
        for k in specs:
            if not R.same_bits(c.outs[k].buf, runs[1][0].outs[k].buf):
                _STATS["rerun_diff"] += 1
                bad.append((row["name"], lay, k, "two launches differ"))
    else:                                                                   # gated only: the second launch passes the same gates
        _judge(row["name"], lay + ":2", specs, {k: h.view for k, h in runs[1][0].outs.items()}, 0, runs[1][2], c.want, bad)
    return bad


def _with_workspace(on):
    from ctrlora_amd import hip
    L = hip.lib()
    if on:
        if hip._workspace is None:
            hip.ensure_workspace(DEV)
        else:
            hip._chk(L.cl_set_workspace(hip._workspace.data_ptr(), hip.WORKSPACE_BYTES), "cl_set_workspace")
        hip._workspace.view(torch.float32).fill_(NAN)
    else:
        hip._chk(L.cl_set_workspace(None, 0), "cl_set_workspace")


def _run_colsum(row, dt):
    from ctrlora_amd import hip
    saved = hip._workspace
    try:
        _with_workspace(row["p"]["ws"])
        return _run_generic(row, dt)
    finally:   # restore the registration exactly as it was
        torch.cuda.synchronize()
        hip._workspace = saved
        if saved is not None:
            hip._chk(hip.lib().cl_set_workspace(saved.data_ptr(), hip.WORKSPACE_BYTES), "cl_set_workspace")
        else:
            hip._chk(hip.lib().cl_set_workspace(None, 0), "cl_set_workspace")


def _run_ddim(row, dt):
    """Host-index form twice (generic), then the device-cursor form: the same bits; index 0 also with a cursor past the end."""
    bad = _run_generic(row, dt)
    p = row["p"]
    ops = R.make_ops(row, dt, DEV)
    host = prep_ddim(row, dt, ops, "pad")
    _launch(host)
    for cursor in [p["S"] - 1 - p["index"]] + ([p["S"] + 3] if p["index"] == 0 else []):
        dev = prep_ddim(row, dt, ops, "pad", cursor=cursor)
        canary, pr = _launch(dev)
        mism = {k: (pr[k], v) for k, v in dev.want.items() if pr[k] != v}
        _STATS["canary"] += canary
        _STATS["form_mismatch"] += bool(mism)
        same = all(R.same_bits(host.outs[k].buf, dev.outs[k].buf) for k in host.outs)
        if canary or mism or not same:
            bad.append((row["name"], f"dev cursor={cursor}", dict(canary=canary, form_mismatch=mism, same_bits=same)))
    return bad


def _run_adamw(row, dt):
    """Three consecutive steps of cl_adamw and of cl_adamw_dev (cl_tick before each), every step against the fp64 step from the state
    the device held before it; the whole sequence twice: the same bits."""
    L, st = _lib()
    n, H, bad = row["p"]["n"], R.ADAMW_HYPER, []
    ops = R.make_ops(row, dt, DEV)
    for form in ("adamw", "adamw_dev"):
        finals = []
        for rep in range(2):
            c = _Ctx()
            g = c.FLAT(ops["g"])
            pmv = [c.OUTF(k, (n,), F32, init=ops[k]) for k in ("p", "m", "v")]
            hyper = c.FLAT(torch.tensor([H[k] for k in ("lr", "beta1", "beta2", "eps", "wd", "gscale")], dtype=F32))
            step = c.OUTF("step", (1,), torch.int32, init=torch.zeros(1, dtype=torch.int32))
            for s in (1, 2, 3):
                before = tuple(t.clone() for t in pmv)
                if form == "adamw":
                    c.call = lambda: L.cl_adamw(*[_p(t) for t in (pmv[0], g, pmv[1], pmv[2])], n, H["lr"], H["beta1"], H["beta2"], H["eps"], H["wd"], s, H["gscale"], st)
                else:
                    assert L.cl_tick(_p(step), st) == 0 and _probe() == R.probe("tick", None, (1,), threads=1)
                    c.call = lambda: L.cl_adamw_dev(*[_p(t) for t in (pmv[0], g, pmv[1], pmv[2])], n, _p(hyper), _p(step), st)
                canary, pr = _launch(c)
                if rep == 0:
                    specs = R.eval_adamw_step(before, g, s)
                    _judge(row["name"], f"{form} step {s}", specs, dict(zip("pmv", pmv)), canary, pr, R.probe(form, None, (R.ew_grid(n),)), bad)
            if form == "adamw_dev" and int(step[0]) != 3:
                bad.append((row["name"], "tick", int(step[0])))
            finals.append([c.outs[k].buf.clone() for k in ("p", "m", "v")])
        if not all(R.same_bits(a, b) for a, b in zip(*finals)):
            _STATS["rerun_diff"] += 1
            bad.append((row["name"], form, "two runs differ"))
    return bad


def _run_zero(row, dt):
    L, st = _lib()
    nb, bad = row["p"]["nbytes"], []
    offs = (0, 5) if "wrap" in row["tags"] else range(16)
    for off in offs:
        buf = torch.empty((nb + 2 * G + 16,), dtype=torch.uint8, device=DEV)
        assert buf.data_ptr() % 16 == 0
        ptr = buf.data_ptr() + G + off
        f = R.zero_form(ptr, nb)
        assert f == R.zero_form(off, nb)
        for rep in range(2):
            buf.fill_(0xA5)                                                 # refilled: the second launch has to clear it again
            rc = L.cl_zero(ptr, nb, st)
            pr = _probe()
            want = R.probe("zero", None, (f["grid"],), form=(1 if f["head"] else 0) | (2 if f["tail"] else 0), aux=f["nvec"]) if nb else R.probe("none", 0, (0, 0, 0), 0)
            if nb == 0:
                want["dtype"] = 0
            torch.cuda.synchronize()
            inside = int((buf[G + off:G + off + nb] != 0).sum())
            outside = int((buf[:G + off] != 0xA5).sum()) + int((buf[G + off + nb:] != 0xA5).sum())
            _STATS["launches"] += 1
            _STATS["canary"] += outside
            _STATS["exact_mismatch"] += inside
            if rc or pr != want or inside or outside:
                _STATS["form_mismatch"] += pr != want
                bad.append((row["name"], off, dict(rc=rc, probe=pr, want=want, not_cleared=inside, canary=outside)))
    return bad


def _run_timestep(row, dt):
    """The long variant (gated), the float variant at the same integer-valued times (the long variant's bits) and at fractional times."""
    L, st = _lib()
    p, bad = row["p"], []
    ops = R.make_ops(row, dt, DEV)
    B, half = p["B"], p["half"]
    res = {}
    for tag, fn, id_, t in (("long", L.cl_timestep_embedding, "timestep", ops["t"]), ("float-int", L.cl_timestep_embedding_f, "timestep_f", ops["t"].float()),
                            ("float-frac", L.cl_timestep_embedding_f, "timestep_f", ops["tf"])):
        specs = R.eval_timestep(p, dt, dict(ops, t=t))
        outs = []
        for rep in range(2):
            c = _Ctx()
            tt, fr = c.FLAT(t), c.FLAT(ops["freqs"])
            out = c.OUT("out", B, 2 * half, dt, 3)
            c.call = lambda: fn(_D(dt), _p(tt), _p(fr), _p(out), out.stride(0), B, half, st)
            canary, pr = _launch(c)
            outs.append((c, canary, pr))
        c, canary, pr = outs[0]
        _judge(row["name"], tag, specs, dict(out=c.outs["out"].view), canary + outs[1][1], pr, R.probe(id_, dt, ((B * half + 255) // 256,)), bad)
        if not R.same_bits(c.outs["out"].buf, outs[1][0].outs["out"].buf):
            _STATS["rerun_diff"] += 1
            bad.append((row["name"], tag, "two launches differ"))
        res[tag] = c.outs["out"].view.clone()
    if not R.same_bits(res["long"], res["float-int"]):
        bad.append((row["name"], "the float variant at integer-valued t does not give the long variant's bits"))
    return bad


def _run_cursors(row, dt):
    """cl_tick, cl_ddim_set_t and cl_dpm_set_t, bit for bit: cursor inside the table, at its end and past it (clamped)."""
    L, st = _lib()
    n, S, bad = row["p"]["n"], row["p"]["S"], []
    g = torch.Generator().manual_seed(31)
    table = torch.randint(1, 1000, (S,), generator=g).to(DEV)
    coef = torch.randn(S, 8, generator=g).to(DEV)
    cnt = _Out((1,), torch.int32, init=torch.tensor([41], dtype=torch.int32))
    for k in range(2):
        rc = L.cl_tick(_p(cnt.view), st)
        if rc or _probe() != R.probe("tick", None, (1,), threads=1) or int(cnt.view[0]) != 42 + k or cnt.bad():
            bad.append((row["name"], "tick", rc, int(cnt.view[0])))
        _STATS["launches"] += 1
    for cursor in (5, S - 1, S + 3):
        cur = torch.tensor([cursor], dtype=torch.int32, device=DEV)
        for rep in range(2):
            ts = _Out((n,), torch.int64)
            tf = _Out((n,), F32)
            rc1 = L.cl_ddim_set_t(_p(table), _p(cur), S, _p(ts.view), n, st)
            p1 = _probe()
            rc2 = L.cl_dpm_set_t(_p(coef), _p(cur), S, _p(tf.view), n, st)
            p2 = _probe()
            torch.cuda.synchronize()
            w1 = table[R.clamp_ddim(S, cursor)].expand(n)
            w2 = coef[R.clamp_dpm(S, cursor), 6].expand(n)
            ok = (rc1 == 0 and rc2 == 0 and p1 == R.probe("ddim_set_t", None, (1,)) and p2 == R.probe("dpm_set_t", None, (1,))
                  and torch.equal(ts.view, w1) and R.same_bits(tf.view, w2.contiguous()) and not ts.bad() and not tf.bad())
            _STATS["launches"] += 2
            if not ok:
                _STATS["exact_mismatch"] += 1
                bad.append((row["name"], "set_t", cursor, rc1, rc2, p1, p2, ts.bad(), tf.bad()))
    return bad


def prep_dpmpp(row, ops, dev):
    """One DPM-Solver++ step with x_next aliasing x; dev: the row comes from a device cursor."""
    L, st = _lib()
    p, c = row["p"], _Ctx()
    n = p["n"]
    ec, eu, coef = c.FLAT(ops["e_c"]), c.FLAT(ops["e_u"]), c.FLAT(ops["coef"])
    x = c.OUTF("x_next", (n,), F32, init=ops["x"])
    hist = c.OUTF("hist", (3, n), F32, init=ops["hist"])
    p0 = c.OUTF("pred_x0", (n,), F32)
    if dev:
        cur = c.FLAT(torch.tensor([p["index"]], dtype=torch.int32))
        c.call = lambda: L.cl_dpmpp_step_dev(_p(x), _p(ec), _p(eu), _p(coef), _p(cur), p["S"], p["scale"], _p(hist), _p(x), _p(p0), n, st)
        c.want = R.probe("dpmpp_step_dev", None, (R.ew_grid(n),))
    else:
        c.call = lambda: L.cl_dpmpp_step(_p(x), _p(ec), _p(eu), _p(coef), p["index"], p["S"], p["scale"], _p(hist), _p(x), _p(p0), n, st)
        c.want = R.probe("dpmpp_step", None, (R.ew_grid(n),))
    return c


def _run_dpmpp(row, dt):
    """The entry point the row names twice (same bits), gated against the fp64 step; the ring slots the step does not write keep their
    bits; the device-cursor row also runs the host-index form once and must give its bits."""
    p, bad = row["p"], []
    ops = R.make_ops(row, dt, DEV)
    specs = R.evaluate(row, dt, ops)
    dev = row["kern"] == "dpmpp_step_dev"
    runs = []
    for form_dev in ([True, True, False] if dev else [False, False]):
        c = prep_dpmpp(row, ops, form_dev)
        canary, pr = _launch(c)
        runs.append((c, canary, pr))
    slot = p["index"] % 3
    for i, (c, canary, pr) in enumerate(runs):
        hist = c.outs["hist"].view
        got = dict(x_next=c.outs["x_next"].view, pred_x0=c.outs["pred_x0"].view, hist_slot=hist[slot])
        _judge(row["name"], f"launch {i}", specs, got, canary, pr, c.want, bad)
        kept = all(R.same_bits(hist[k], ops["hist"][k]) for k in range(3) if k != slot)
        if not kept or not R.same_bits(hist[slot], c.outs["pred_x0"].view):
            _STATS["canary"] += 1
            bad.append((row["name"], f"launch {i}", "history ring", dict(other_slots_kept=kept)))
        if i and not all(R.same_bits(c.outs[k].buf, runs[0][0].outs[k].buf) for k in c.outs):
            _STATS["rerun_diff"] += 1
            bad.append((row["name"], f"launch {i}", "bits differ from the first launch"))
    return bad


SPECIAL = dict(dpmpp_step=_run_dpmpp, dpmpp_step_dev=_run_dpmpp, colsum=_run_colsum, ddim_step=_run_ddim, adamw=_run_adamw, zero=_run_zero, timestep=_run_timestep, cursors=_run_cursors)
_PARAMS = [pytest.param(r, dt, id=f"{r['name']}" + ("" if dt is None else "-bf16" if dt == BF else "-f32")) for r in R.CASES for dt in r["dtypes"]]


@pytest.mark.parametrize("row,dtype", _PARAMS)
def test_row_passes_its_tier_and_launches_the_form_the_transcription_predicts(row, dtype):
    _need_gpu()
    if _T0[0] is None:
        _T0[0] = time.time()
    _STATS["cases"] += 1
    k = row["kern"]
    bad = SPECIAL[k](row, dtype) if k in SPECIAL else _run_generic(row, dtype)
    if k in SLICED and dtype == BF and "wrap" not in row["tags"]:
        bad += _run_generic(row, dtype, lay="slice")
    assert not bad, (len(bad), bad[:6])


def test_refusals_reset_the_record_and_touch_nothing():
    """A refused call after a good launch: CL_EINVAL, the probe reports id 0, the output keeps its bits.  Every refusal is decided on
    the host before any launch (tests/test_ew_reference_model.py shows the whole list with pointers that are never read)."""
    _need_gpu()
    L, st = _lib()
    x = torch.randn(8, 64, device=DEV).bfloat16()
    y = _G2(8, 64, BF, 1, init=torch.zeros(8, 64).bfloat16())
    good = lambda: L.cl_axpby(0, _p(x), 64, _p(y.view), y.view.stride(0), 8, 64, 1.0, 0.0, st)
    calls = {
        "dtype": lambda: L.cl_axpby(2, _p(x), 64, _p(y.view), y.view.stride(0), 8, 64, 1.0, 0.0, st),
        "ld < width": lambda: L.cl_axpby(0, _p(x), 56, _p(y.view), y.view.stride(0), 8, 64, 1.0, 0.0, st),
        "misaligned": lambda: L.cl_axpby(0, _p(x) + 2, 64, _p(y.view), y.view.stride(0), 8, 56, 1.0, 0.0, st),
        "null": lambda: L.cl_axpby(0, None, 64, _p(y.view), y.view.stride(0), 8, 64, 1.0, 0.0, st),
        "colsum B = 0": lambda: L.cl_colsum(0, _p(x), 64, _p(y.view), 64, 0, 8, 64, 1.0, st),
        "transpose batch": lambda: L.cl_transpose(0, 0, _p(x), 64, 512, _p(y.view), y.view.stride(0), 0, 65536, 8, 64, 8, st),
    }
    wrong = []
    for name, call in calls.items():
        assert good() == 0 and _probe()["id"] == R.EW["axpby"]
        torch.cuda.synchronize()
        before = R.bits(y.buf).clone()
        rc = call()
        pr = _probe()
        torch.cuda.synchronize()
        if rc != 1 or pr != dict.fromkeys(R.PROBE_FIELDS, 0) or not torch.equal(before, R.bits(y.buf)):
            wrong.append((name, rc, pr))
    assert not wrong, wrong
    assert L.cl_debug_ew_last_launch(None) == 1


def test_zz_ew_conformance_summary():
    """Cases, launches, violations, canary changes and the wall time of this file, for DESIGN.md 1j."""
    _need_gpu()
    wall = None if _T0[0] is None else time.time() - _T0[0]
    print("ew conformance:", json.dumps(_STATS), "wall_s:", wall)
    _record("ew_conformance_summary", stats=_STATS, wall_s=wall, rows=len(R.CASES), c=R.C_GATE)
    for k in ("violations", "exact_mismatch", "canary", "form_mismatch", "rerun_diff"):
        assert _STATS[k] == 0, (k, _STATS)
    assert all(v <= 1.0 for k, v in _STATS.items() if k.startswith("eob_")), _STATS
