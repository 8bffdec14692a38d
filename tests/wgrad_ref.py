"""Reference, rounding model, transcription of the host split rule, gates and case table of the weight-gradient conformance suite
(helpers only: nothing here is collected, nothing here imports a GPU).  Shaped like tests/norm_ref.py; Guarded / PAD_FILL come from
tests/gemm_ref.py, gate / failures from tests/norm_ref.py.

Contract (ctrlora_amd/csrc/wgrad.hip, csrc/gemm.h: WgradDesc, include/ctrlora_hip.h: cl_wgrad_desc), on the bf16 values as stored:

    dW[n, k] = dW0[n, k] + alpha sum_m dy[m, n] x[row(m, tap), k]                        (fp32, accumulated)

    tap = -1        row(m) = m                                                           (plain dy^T x)
    tap = 0 .. 8    m = (b, oy, ox) on the Hout x Wout grid, ky = tap / 3, kx = tap % 3,
                    row = (b, oy stride + ky - pad, ox stride + kx - pad) of the Hin x Win input, zero outside the image
    tap = 16 + ky   the three taps (ky, 0 .. 2) at stride 1, pad 1 from one problem: tap kx lands K floats further on in a row of dW

`wgrad_ref64` evaluates this in fp64 together with mag = |dW0| + |alpha| sum |dy| |x| per element (tests/test_wgrad_reference_model.py
checks the conv forms against fp64 autograd of conv2d).  `plan` is a line-for-line transcription of launch_wgrad_tn_group /
launch_wgrad_group_kind: validation, the split rule with its two fall-backs (workspace cap, early flush) and the flush at 24
descriptors; it gives what cl_debug_wgrad_last_launch / _last_problem must report.  `wgrad_model` is the contract with the roundings
the kernels document and no others: bf16 products exact in fp32, fp32 accumulation in step order within a split (the order INSIDE
an MFMA is not documented; it is modelled as sequential over m), the slabs summed in split order in fp32, one multiply by alpha and
one add onto dW0.

Two tiers, every row:
  * exact: dy, x integers in [-2, 2], dW0 a small integer, alpha a power of two (or 0) -- every partial sum is an integer below 2^24,
    so ANY summation order gives the same bits: torch.equal against the fp64 contract.  The row builder asserts
    M 4 |alpha| + |dW0| < 2^24.
  * rounding: Gaussian inputs, |got - ref| <= u |ref| + c u mag element-wise with zero violations, u = 2^-24.  c = MARGIN x the largest
    value the rounding MODEL needs over the whole table against the fp64 contract (`python -m tests.wgrad_ref`, CPU; MARGIN = 3 as
    tests/attn_ref.py).  Nothing is fitted to a kernel's output.  The worst case of n-term fp32 summation gives c <= M + splits + 2; the
    gate of a row uses the smaller of the two (unit_c; the row builder asserts it).

The bias gradient cl_colsum (workspace partials + finish, or atomics) and the fp32 family's route cl_conv_tap_gather -> cl_transpose
-> cl_weight_grad ride in the same table with the exact tier only (column sums / products of small integers).
"""
import math

import torch

from tests.attn_ref import MARGIN
from tests.gemm_ref import GUARD_ROWS, PAD_COLS, PAD_FILL, Guarded, padded  # noqa: F401  (re-exported for the GPU suite)
from tests.norm_ref import failures, gate  # noqa: F401

BF, F32 = torch.bfloat16, torch.float32
U = 2.0 ** -24

# knobs of csrc/wgrad.hip (g_wgrad_blocks, g_wgrad_min_steps, g_wgrad_row3_blocks, g_wgrad_ring, g_wgrad_rows) and its limits
BLOCKS, MIN_STEPS, ROW3_BLOCKS, RING, ROWS = 512, 8, 512, 3, 32
WGRAD_MAX_PROBS = 24
ROW3_RING = 8
REC_GROUPS = 8
WORKSPACE_BYTES = 64 << 20            # ctrlora_amd/hip.py: WORKSPACE_BYTES, the default stream's scratch
CALL_FIELDS = ("ran", "tn_launches", "row3_launches", "reduce_launches", "problems", "groups", "ring", "rows")
PROB_FIELDS = ("row3", "tiles", "per", "splits", "slab_off", "blk0", "red0", "group", "desc", "M", "N", "K")

# Measured by measure_constants() on the CPU over every row of CASES: the largest c the rounding model needs in
# |model - ref| <= u |ref| + c u mag: 1.968 on tn-unsplit-m256 (one fp32 chain of 256 terms, the longest of the table; the split
# rows break theirs into chains of at most 12 steps x 32).  The gate uses c = MARGIN x this = 5.90, and on the rows where the
# derivable worst case M + splits + 2 is smaller (M = 1: 4) that instead (unit_c).
MEASURED = 1.968
C = MARGIN * MEASURED


# ------------------------------------------------------------------------------------------------ descriptors

def _plain(M, N, K, alpha=1.0):
    return dict(kind="plain", M=M, N=N, K=K, alpha=alpha, cols=K, Mx=M)


def _taps(B, Hin, Win, stride, N, K, alpha=1.0, cin=None):
    """The nine single-tap problems of one 3x3 conv, pad 1: dW is [N][9][K]; cin: input channels that are not zero padding."""
    Hout, Wout = (Hin - 1) // stride + 1, (Win - 1) // stride + 1
    return dict(kind="taps", B=B, Hin=Hin, Win=Win, Hout=Hout, Wout=Wout, stride=stride, pad=1, M=B * Hout * Wout, N=N, K=K,
                alpha=alpha, cols=9 * K, Mx=B * Hin * Win, cin=cin)


def _row3(B, H, W, N, K, alpha=1.0, kys=(0, 1, 2)):
    """Row-of-three problems (tap = 16 + ky) of one stride-1 conv: dW is [N][len(kys)][3][K]."""
    return dict(kind="row3", B=B, Hin=H, Win=W, Hout=H, Wout=W, stride=1, pad=1, M=B * H * W, N=N, K=K, alpha=alpha,
                cols=3 * K * len(kys), Mx=B * H * W, kys=tuple(kys))


def unit_descs(unit, ui=0):
    """The descriptors of a unit, in the order they go into the call: dict(unit, col0, width, tap, M, N, K, alpha, conv fields)."""
    base = dict(unit=ui, M=unit["M"], N=unit["N"], K=unit["K"], alpha=unit["alpha"])
    if unit["kind"] == "plain":
        return [dict(base, tap=-1, col0=0, width=unit["K"], Hin=0, Win=0, Hout=0, Wout=0, stride=0, pad=0)]
    geo = {k: unit[k] for k in ("Hin", "Win", "Hout", "Wout", "stride", "pad")}
    if unit["kind"] == "taps":
        return [dict(base, tap=t, col0=t * unit["K"], width=unit["K"], **geo) for t in range(9)]
    return [dict(base, tap=16 + ky, col0=3 * unit["K"] * i, width=3 * unit["K"], **geo) for i, ky in enumerate(unit["kys"])]


def row_descs(row):
    return [d for ui, u in enumerate(row["units"]) for d in unit_descs(u, ui)]


# ------------------------------------------------------------------------------------------------ the host rule (transcription)

def refused(d):
    """wgrad_desc_ok of csrc/wgrad.hip, negated: does the launcher refuse this descriptor?  lddy / ldx / lddw default to the
    tightest legal values; `null` names pointers that are null, `dw_misaligned` a dW that is not 16-byte aligned."""
    N, K, M = d["N"], d["K"], d["M"]
    lddy, ldx = d.get("lddy", N), d.get("ldx", K)
    lddw = d.get("lddw", 3 * K if d["tap"] >= 16 else K)
    null = d.get("null", ())
    if N % 8 or K % 8 or lddy % 8 or ldx % 8 or lddw % 4 or N < 8 or K < 8 or d.get("dw_misaligned"):
        return True
    if "dy" in null or "x" in null or "dW" in null or lddy < N or ldx < K:
        return True
    Hin, Win, Hout, Wout, stride, pad, tap = (d[k] for k in ("Hin", "Win", "Hout", "Wout", "stride", "pad", "tap"))
    if tap >= 16:
        return bool(tap > 18 or stride != 1 or pad != 1 or Hin != Hout or Win != Wout or Hout <= 0 or Wout <= 0 or Hin > 32767
                    or Win > 32767 or M % (Hout * Wout) or M % 32 or not (Wout % 32 == 0 or Wout in (8, 16)) or K % 4 or lddw < 3 * K)
    if lddw < K:
        return True
    return bool(tap > 8 or (tap >= 0 and (Hin <= 0 or Win <= 0 or Hout <= 0 or Wout <= 0 or Hin > 32767 or Win > 32767 or Hout > 32767
                                          or Wout > 32767 or pad < 0 or pad > 32767 or stride < 1 or stride > 2 or M % (Hout * Wout))))


def _cdiv(a, b):
    return (a + b - 1) // b


def plan(descs, ws_bytes=WORKSPACE_BYTES, blocks=BLOCKS, min_steps=MIN_STEPS, row3_blocks=ROW3_BLOCKS, ring=RING, rows_knob=ROWS):
    """What one call of cl_weight_grad_tn_group launches: None when it is refused, else dict(call = the fields of
    cl_debug_wgrad_last_launch, groups = [(row3, workgroups, reduce workgroups)], problems = [the fields of _last_problem, plus
    capped / fallback / why the group before it was flushed]).  Descriptors with M, N or K <= 0 are skipped."""
    live = [d for d in descs if d["M"] > 0 and d["N"] > 0 and d["K"] > 0]
    if any(refused(d) for d in live):
        return None
    call = dict(ran=0, tn_launches=0, row3_launches=0, reduce_launches=0, problems=0, groups=0, ring=0, rows=0)
    out = dict(call=call, groups=[], problems=[], flushes=[])
    for row3 in (False, True):
        if any((d["tap"] >= 16) == row3 for d in descs):
            _plan_kind(descs, row3, ws_bytes, blocks, min_steps, row3_blocks, ring, rows_knob, out)
    return out


def _plan_kind(descs, row3, ws_bytes, blocks, min_steps, row3_blocks, ring, rows_knob, out):
    NT = 3 if row3 else 1
    mine = [(i, d) for i, d in enumerate(descs) if (d["tap"] >= 16) == row3 and d["M"] > 0 and d["N"] > 0 and d["K"] > 0]
    tiles_all = sum(_cdiv(d["N"], 128) * _cdiv(d["K"], 128) for _, d in mine)
    if tiles_all == 0:
        return
    rows = 32 if row3 else (64 if rows_knob == 64 else 32)
    steps_all = sum(_cdiv(d["N"], 128) * _cdiv(d["K"], 128) * _cdiv(d["M"], rows) for _, d in mine)
    want_blocks = row3_blocks if row3 else blocks
    per = _cdiv(steps_all, want_blocks)
    if row3:
        max_steps = max(_cdiv(d["M"], rows) for _, d in mine)
        smax = max(1, want_blocks // tiles_all)
        per = _cdiv(max_steps, smax)
    per = max(per, max(1, min_steps * 32 // rows))
    call = out["call"]
    state = dict(n=0, nblocks=0, nred=0, ws_used=0, pending=[])

    def flush(why):
        call["ran"], call["ring"], call["rows"] = 1, (ROW3_RING if row3 else ring), rows
        call["row3_launches" if row3 else "tn_launches"] += 1
        call["reduce_launches"] += 1 if state["nred"] > 0 else 0
        for p in state["pending"]:
            p["group"] = call["groups"]
        out["problems"] += state["pending"]
        out["groups"].append((int(row3), state["nblocks"], state["nred"]))
        out["flushes"].append(why)
        call["problems"] += len(state["pending"])
        call["groups"] += 1
        state.update(n=0, nblocks=0, nred=0, ws_used=0, pending=[])

    for i, d in mine:
        tn, tk, steps = _cdiv(d["N"], 128), _cdiv(d["K"], 128), _cdiv(d["M"], rows)
        slab = NT * d["N"] * d["K"] * 4
        splits = _cdiv(steps, per)
        pp = _cdiv(steps, splits)
        splits = first = _cdiv(steps, pp)
        need = splits * slab if splits > 1 else 0
        capped = fallback = False
        if need > ws_bytes:
            splits = asked = max(ws_bytes // slab, 1)
            pp = _cdiv(steps, splits)
            splits = _cdiv(steps, pp)
            need = splits * slab if splits > 1 else 0
            capped, fallback = splits > 1, splits == 1
        if state["n"] == WGRAD_MAX_PROBS or state["ws_used"] + need > ws_bytes:
            flush("max" if state["n"] == WGRAD_MAX_PROBS else "ws")
        state["pending"].append(dict(row3=int(row3), tiles=tn * tk, per=pp, splits=splits, slab_off=state["ws_used"] if splits > 1 else -1,
                                     blk0=state["nblocks"], red0=state["nred"], group=0, desc=i, M=d["M"], N=d["N"], K=d["K"],
                                     capped=capped, fallback=fallback, first=first, asked=asked if (capped or fallback) else first))
        state["n"] += 1
        state["nblocks"] += tn * tk * splits
        if splits > 1:
            state["nred"] += _cdiv(NT * d["N"] * (d["K"] // 4), 256)
        state["ws_used"] += (need + 255) & ~255
    if state["n"]:
        flush("end")


# ------------------------------------------------------------------------------------------------ contract, model

def gather_index(d, kx=None):
    """Input row of every output row m of a conv descriptor, -1 outside the image (the gather definition of csrc/gemm.h)."""
    tap = d["tap"]
    ky, kx = (tap - 16, kx) if tap >= 16 else (tap // 3, tap % 3)
    m = torch.arange(d["M"])
    ox, t2 = m % d["Wout"], m // d["Wout"]
    oy, b = t2 % d["Hout"], t2 // d["Hout"]
    iy, ix = oy * d["stride"] + ky - d["pad"], ox * d["stride"] + kx - d["pad"]
    ok = (iy >= 0) & (iy < d["Hin"]) & (ix >= 0) & (ix < d["Win"])
    return torch.where(ok, (b * d["Hin"] + iy) * d["Win"] + ix, torch.full_like(m, -1))


def _gathered(d, x, defect=None):
    """The x operand of each [N, K] block of a descriptor, [M, K] each, in x's dtype (1 block, or 3 for tap >= 16)."""
    if d["tap"] < 0:
        return [x[:d["M"]]]
    out = []
    for kx in ((0, 1, 2) if d["tap"] >= 16 else (None,)):
        kk = kx
        if defect == "swapkx":
            if d["tap"] >= 16:
                kk = 2 - kx
            else:
                d = dict(d, tap=(d["tap"] // 3) * 3 + 2 - d["tap"] % 3)
        idx = gather_index(d, kk)
        if d["tap"] >= 16 and defect in ("halo", "xt40"):
            r = torch.arange(d["M"]) % 32
            seg = min(d["Wout"], 32)
            if defect == "halo":      # the pixel left of a segment (tap kx = 0) and right of it (kx = 2) never loaded
                idx = torch.where(((kx == 0) & (r % seg == 0)) | ((kx == 2) & (r % seg == seg - 1)), torch.full_like(idx, -1), idx)
            else:                     # only 40 rows of the x tile exist: row (r / seg)(seg + 2) + r % seg + kx
                idx = torch.where((r // seg) * (seg + 2) + r % seg + kx >= 40, torch.full_like(idx, -1), idx)
        g = x[idx.clamp_min(0)]
        out.append(torch.where((idx >= 0)[:, None], g, torch.zeros_like(g)))
    return out


def wgrad_ref64(d, dy, x, dW0):
    """fp64 (dW, mag) of one descriptor: [N, width] each.  dW0 is the [N, width] slice the descriptor accumulates onto."""
    a, dyd = float(d["alpha"]), dy[:d["M"]].double()
    xs = [g.double() for g in _gathered(d, x)]
    s = torch.cat([dyd.t() @ g for g in xs], 1)
    sa = torch.cat([dyd.abs().t() @ g.abs() for g in xs], 1)
    return dW0.double() + a * s, dW0.double().abs() + abs(a) * sa


def wgrad_model(d, p, dy, x, dW0, defect=None):
    """The documented roundings of one descriptor launched as plan entry p (per, splits): float32 [N, width]."""
    M, per, splits = d["M"], p["per"], p["splits"]
    alpha = torch.tensor(float(d["alpha"]), dtype=F32)
    dyf = dy[:M].float()
    blocks = []
    steps = _cdiv(M, 32)
    if defect == "ragged" and M % 32:
        steps -= 1
    for g in _gathered(d, x, defect):
        gf = g.float()
        slabs = []
        for z in range(splits):
            acc = torch.zeros(d["N"], d["K"], dtype=F32)
            for m in range(z * per * 32, min(M, min(steps, (z + 1) * per) * 32)):
                acc = acc + dyf[m][:, None] * gf[m][None, :]
            slabs.append(acc)
        if defect == "alpha_per_split" and splits > 1:      # the running sum scaled and added once per split, not once at the end
            a, o = torch.zeros_like(slabs[0]), None
            for v in slabs:
                a = a + v
                o = a * alpha if o is None else o + a * alpha
            blocks.append(o)
            continue
        a = torch.zeros_like(slabs[0])
        for z, v in enumerate(slabs):
            if not (defect == "skipslab" and z == 1):
                a = a + v
        blocks.append(a * alpha)
    return dW0.float() + torch.cat(blocks, 1)


# ------------------------------------------------------------------------------------------------ the case table

def _row(name, units, ws=None, ring=RING, single=False, covers=()):
    return dict(name=name, family="wgrad", units=units, ws=ws, ring=ring, single=single, covers=tuple(covers))


NK5 = ((8, 264), (120, 8), (128, 136), (136, 120), (264, 128))      # N, K in {8, 120, 128, 136, 264}: clamp at N - 8, partial tiles
ALPHAS = (1.0, 0.5, -2.0, 0.0)
SLAB128 = 128 * 128 * 4


def _small(n, split_at):
    """n small plain problems, those at the indices split_at with M = 512 (two splits), alphas in turn."""
    return [_plain(512 if i in split_at else 33, 8, 16 if i % 2 else 8, ALPHAS[i % 3]) for i in range(n)]


def _cases():
    rows = []
    # ---- tn kernel, unsplit: every M with the five (N, K) pairs as one call; M = 1, 33, 256 also through cl_weight_grad_tn
    for M in (1, 31, 32, 33, 255, 256):
        rows.append(_row(f"tn-unsplit-m{M}", [_plain(M, N, K, ALPHAS[i % 4]) for i, (N, K) in enumerate(NK5)], covers=("tn", "unsplit")))
    for M, (N, K) in ((1, (8, 8)), (33, (136, 120)), (256, (264, 128))):
        rows.append(_row(f"tn-single-m{M}-{N}x{K}", [_plain(M, N, K)], single=True, covers=("tn", "unsplit", "single")))
    # ---- tn kernel, split
    rows.append(_row("tn-split-m512", [_plain(512, 128, 128)], single=True, covers=("tn", "split", dict(splits=2, per=8))))
    rows.append(_row("tn-split-m549", [_plain(549, 128, 128, 0.5)], covers=("tn", "split", "ragged", dict(splits=3, per=6))))
    rows.append(_row("tn-split-m530", [_plain(530, 136, 120, -2.0)], covers=("tn", "split", "ragged", "uneven", dict(splits=3, per=6))))
    rows.append(_row("tn-split-m800-264x8", [_plain(800, 264, 8)], covers=("tn", "split", dict(splits=4, per=7, tiles=3))))
    # ---- single taps: all nine, stride 1 and 2
    for s in (1, 2):
        rows.append(_row(f"taps-s{s}-2x8x8", [_taps(2, 8, 8, s, 16, 24)], covers=("taps", "unsplit")))
        rows.append(_row(f"taps-s{s}-3x4x8", [_taps(3, 4, 8, s, 136, 32, 0.5)], covers=("taps", "unsplit", "nonsquare")))
        rows.append(_row(f"taps-s{s}-1x1x32", [_taps(1, 1, 32, s, 8, 136)], covers=("taps", "unsplit", "h1")))
        rows.append(_row(f"taps-s{s}-2x8x8-cin4", [_taps(2, 8, 8, s, 16, 32, cin=4)], covers=("taps", "unsplit", "cin4")))
    rows.append(_row("taps-s1-8x8x8-split", [_taps(8, 8, 8, 1, 16, 24, -2.0)], covers=("taps", "split", dict(splits=2))))
    rows.append(_row("taps-s2-8x16x16-split", [_taps(8, 16, 16, 2, 16, 24)], covers=("taps", "split", dict(splits=2))))
    # ---- row of three
    rows.append(_row("row3-w8-4x2x8", [_row3(4, 2, 8, 8, 32)], covers=("row3", "unsplit", "w8", "spans_samples")))
    rows.append(_row("row3-w16-1x2x16", [_row3(1, 2, 16, 136, 136, 0.5)], covers=("row3", "unsplit", "w16", "m32")))
    rows.append(_row("row3-w32-1x1x32", [_row3(1, 1, 32, 8, 136)], covers=("row3", "unsplit", "w32", "h1", "m32")))
    rows.append(_row("row3-w64-1x1x64", [_row3(1, 1, 64, 136, 32, -2.0)], covers=("row3", "unsplit", "w64", "h1")))
    rows.append(_row("row3-w96-1x1x96", [_row3(1, 1, 96, 8, 32)], covers=("row3", "unsplit", "w96", "h1")))
    rows.append(_row("row3-w64-1x3x64", [_row3(1, 3, 64, 16, 32)], covers=("row3", "unsplit", "w64")))
    rows.append(_row("row3-w16-2x16x16-split", [_row3(2, 16, 16, 8, 32)], covers=("row3", "split", "w16", dict(splits=2))))
    rows.append(_row("row3-w32-1x24x32-split-ky1", [_row3(1, 24, 32, 16, 136, 0.5, kys=(1,))], covers=("row3", "split", "w32", "lddw>3K", dict(splits=3))))
    # ---- groups
    rows.append(_row("group-25", _small(25, (3, 24)), covers=("flush24",)))
    rows.append(_row("group-49", _small(49, (5, 24, 30, 48)), covers=("flush24",)))
    rows.append(_row("group-mixed", [_plain(33, 136, 120, 0.5), _taps(2, 8, 8, 1, 16, 24), _row3(4, 2, 8, 8, 32, -2.0), _plain(512, 8, 8)],
                     covers=("mixed",)))
    rows.append(_row("group-interleaved", [_plain(512, 128, 8), _plain(31, 8, 8, 0.5), _plain(549, 8, 136, -2.0), _plain(1, 16, 16), _plain(512, 16, 8, 0.0)],
                     covers=("interleaved",)))
    rows.append(_row("group-alphas", [_plain(65, 16, 24, a) for a in ALPHAS], covers=("alphas",)))
    # ---- workspace forms, on a side stream bound to a small workspace
    rows.append(_row("ws-cap-m549", [_plain(549, 128, 128)], ws=2 * SLAB128, covers=("capped", dict(splits=2, per=9))))
    rows.append(_row("ws-fallback-m549", [_plain(549, 128, 128, 0.5)], ws=SLAB128 - 256, covers=("fallback", dict(splits=1))))
    rows.append(_row("ws-earlyflush-2xm512", [_plain(512, 128, 128), _plain(512, 128, 128, -2.0)], ws=2 * SLAB128, covers=("early_flush",)))
    # steps = 81: first estimate 11 splits; 10 slabs fit -> 9 steps per split -> 9 splits (the recomputed count is SMALLER than asked).
    # Uncapped this cannot happen: per' = ceil(steps / splits) <= per, so ceil(steps / per') >= splits.
    rows.append(_row("ws-cap-recompute-m2592", [_plain(2592, 8, 8)], ws=10 * 256, covers=("capped", "recompute_smaller", dict(splits=9, per=9))))
    rows.append(_row("ws-taps-earlyflush", [_taps(8, 8, 8, 1, 16, 24)], ws=3 * 3072, covers=("early_flush", "taps")))
    rows.append(_row("ws-row3-cap", [_row3(1, 24, 32, 8, 32, kys=(1,))], ws=2 * 3072, covers=("capped", "row3", dict(splits=2, per=12))))
    rows.append(_row("ws-row3-fallback", [_row3(1, 24, 32, 8, 32, 0.5, kys=(1,))], ws=3072 - 256, covers=("fallback", "row3", dict(splits=1))))
    rows.append(_row("ws-row3-earlyflush", [_row3(2, 16, 16, 8, 32)], ws=2 * 3072, covers=("early_flush", "row3")))
    # ---- ring depths 4 and 6 (tn kernel: plain and taps; the row-of-three kernel has one ring, 8, and runs beside them)
    for ring in (4, 6):
        rows.append(_row(f"ring{ring}-tn-split-m549", [_plain(549, 128, 128, 0.5)], ring=ring, covers=("ring", "tn")))
        rows.append(_row(f"ring{ring}-taps-split", [_taps(8, 8, 8, 1, 16, 24)], ring=ring, covers=("ring", "taps")))
        rows.append(_row(f"ring{ring}-row3-split", [_row3(2, 16, 16, 8, 32)], ring=ring, covers=("ring", "row3")))
        rows.append(_row(f"ring{ring}-tn-m33", [_plain(33, 136, 120)], ring=ring, covers=("ring", "short")))   # fewer steps than slots
    for row in rows:
        _assert_row(row)
    return rows


def row_plan(row):
    return plan(row_descs(row), ws_bytes=row["ws"] if row["ws"] is not None else WORKSPACE_BYTES, ring=row["ring"])


def row_forms(row):
    """The forms a row reaches, derived from the transcription (what _assert_row and the CPU test read)."""
    pl = row_plan(row)
    assert pl is not None, row["name"]
    f = set()
    for p in pl["problems"]:
        kind = "row3" if p["row3"] else ("taps" if row_descs(row)[p["desc"]]["tap"] >= 0 else "tn")
        f.add((kind, "split" if p["splits"] > 1 else "unsplit"))
        if p["capped"]:
            f.add(("capped", kind))
            if p["splits"] < p["asked"]:
                f.add(("recompute_smaller",))
        if p["fallback"]:
            f.add(("fallback", kind))
        if p["splits"] > 1 and p["M"] % 32:
            f.add(("ragged_split", kind))
        if p["splits"] > 1 and _cdiv(p["M"], 32) % p["per"]:
            f.add(("uneven_split", kind))
        if p["group"] > 0 and p["splits"] > 1:
            f.add(("slab_in_later_group",))
    for why in pl["flushes"]:
        f.add(("flush", why))
    kinds = {k for k, _ in [t for t in f if len(t) == 2 and t[0] in ("tn", "taps", "row3")]}
    if len(kinds) == 3:
        f.add(("mixed",))
    sp = [p["splits"] > 1 for p in pl["problems"] if p["group"] == 0]
    if len(sp) >= 4 and all(a != b for a, b in zip(sp, sp[1:])):
        f.add(("interleaved",))
    if row["ring"] != RING:
        f |= {("ring", row["ring"], k) for k in kinds}
    for u in row["units"]:
        if u["kind"] == "taps":
            f.add(("taps", "stride", u["stride"]))
        if u["kind"] == "row3":
            f.add(("row3", "W", u["Wout"]))
    return f


def unit_c(row, pl=None):
    """The gate constant of each unit of a row: MARGIN x MEASURED, or the derivable worst case of n-term fp32 summation
    (M + splits + 2: M products, the slabs, alpha and the add onto dW0) where that is smaller."""
    pl = pl or row_plan(row)
    descs = row_descs(row)
    return [min([C] + [float(p["M"] + p["splits"] + 2) for p in pl["problems"] if descs[p["desc"]]["unit"] == ui])
            for ui in range(len(row["units"]))]


def exact_inputs_ok(unit):
    """Every partial sum of the exact tier is an integer below 2^24: |dy|, |x| <= 2, |dW0| <= 8."""
    return unit["M"] * 4 * abs(unit["alpha"]) + 8 < 2 ** 24


def _assert_row(row):
    """The table's own claims against the transcription of the launcher."""
    pl = row_plan(row)
    name = row["name"]
    assert pl is not None and pl["call"]["ran"] == 1, name
    descs = row_descs(row)
    assert len(pl["problems"]) == len(descs) and sorted(p["desc"] for p in pl["problems"]) == list(range(len(descs))), name
    forms = row_forms(row)
    cov = row["covers"]
    want = [c for c in cov if isinstance(c, dict)]
    tags = [c for c in cov if not isinstance(c, dict)]
    p0 = pl["problems"][0]
    for w in want:
        assert all(p0[k] == v for k, v in w.items()), (name, w, p0)
    kind = next((t for t in tags if t in ("tn", "taps", "row3")), None)
    for t in tags:
        if t in ("split", "unsplit") and kind:
            assert (kind, t) in forms, (name, t, forms)
        elif t in ("capped", "fallback"):
            assert any(f[0] == t for f in forms), (name, t, forms)
        elif t == "early_flush":
            assert ("flush", "ws") in forms, (name, forms)
        elif t == "flush24":
            assert ("flush", "max") in forms and ("slab_in_later_group",) in forms, (name, forms)
            second = [p for p in pl["problems"] if p["group"] == 1]
            assert second[0]["blk0"] == 0 and second[0]["red0"] == 0 and second[0]["desc"] == WGRAD_MAX_PROBS, name
        elif t in ("mixed", "interleaved", "recompute_smaller"):
            assert (t,) in forms, (name, t, forms)
        elif t == "ragged":
            assert ("ragged_split", kind) in forms, (name, forms)
        elif t == "uneven":
            assert ("uneven_split", kind) in forms, (name, forms)
        elif t == "ring":
            assert row["ring"] in (4, 6), name
    for p in pl["problems"]:
        steps = _cdiv(p["M"], 32)
        assert (p["splits"] - 1) * p["per"] < steps <= p["splits"] * p["per"], (name, p)        # every split owns at least one step
        if row["ws"] is not None and p["splits"] > 1:
            assert p["slab_off"] + p["splits"] * (3 if p["row3"] else 1) * p["N"] * p["K"] * 4 <= row["ws"], (name, p)
    assert all(exact_inputs_ok(u) for u in row["units"]), name
    assert all(0 < c <= C and all(c <= p["M"] + p["splits"] + 2 for p in pl["problems"] if descs[p["desc"]]["unit"] == ui)
               for ui, c in enumerate(unit_c(row, pl))), name                                     # never above the derivable worst case
    if row["single"]:
        assert len(row["units"]) == 1 and row["units"][0]["kind"] == "plain", name


def covered_forms(rows=None):
    out = set()
    for row in rows if rows is not None else CASES:
        out |= row_forms(row)
    return out


# ------------------------------------------------------------------------------------------------ operands, measuring

def make_operands(row, tier, device="cpu"):
    """Per unit dict(dy [M, N] bf16, x [Mx, K] bf16, dW0 [N, cols] fp32), drawn on the CPU from a generator seeded by the row's place
    in the table.  tier "exact": integers (module docstring); "gauss": standard normal, rounded once to bf16."""
    names = [r["name"] for r in CASES]
    g = torch.Generator().manual_seed(7000 + names.index(row["name"]) if row["name"] in names else 6999)
    ops = []
    for u in row["units"]:
        if tier == "exact":
            dy = torch.randint(-2, 3, (u["M"], u["N"]), generator=g).to(BF)
            x = torch.randint(-2, 3, (u["Mx"], u["K"]), generator=g).to(BF)
            dW0 = torch.randint(-8, 9, (u["N"], u["cols"]), generator=g).float()
        else:
            dy = torch.randn(u["M"], u["N"], generator=g).to(BF)
            x = torch.randn(u["Mx"], u["K"], generator=g).to(BF)
            dW0 = torch.randn(u["N"], u["cols"], generator=g)
        if u.get("cin"):
            x[:, u["cin"]:] = 0
        ops.append(dict(dy=dy.to(device), x=x.to(device), dW0=dW0.to(device)))
    return ops


def row_ref64(row, ops):
    """Per unit (ref, mag), [N, cols] double: every descriptor of the unit onto its columns of dW0."""
    out = []
    for ui, u in enumerate(row["units"]):
        o = ops[ui]
        ref, mag = o["dW0"].double().clone(), o["dW0"].double().abs()
        for d in unit_descs(u, ui):
            c = slice(d["col0"], d["col0"] + d["width"])
            ref[:, c], mag[:, c] = wgrad_ref64(d, o["dy"], o["x"], o["dW0"][:, c])
        out.append((ref, mag))
    return out


def row_model(row, ops, defect=None):
    pl = row_plan(row)
    descs = row_descs(row)
    out = [o["dW0"].float().clone() for o in ops]
    for p in pl["problems"]:
        d = descs[p["desc"]]
        o = ops[d["unit"]]
        c = slice(d["col0"], d["col0"] + d["width"])
        out[d["unit"]][:, c] = wgrad_model(d, p, o["dy"], o["x"], o["dW0"][:, c], defect)
    return out


def check(got, ref, mag, c):
    """The rounding-tier gate of one unit's dW at the unit's constant c (unit_c): {"dW": gate dict} for failures()."""
    return {"dW": gate(got, ref, torch.zeros_like(ref), U * mag, U, c)}


def measure_constants(rows=None):
    """(largest c the rounding model needs over the rows, the row that needs it); the exact tier of the model is asserted on the way."""
    worst = (0.0, "")
    for row in rows if rows is not None else CASES:
        ops = make_operands(row, "exact")
        for (ref, _), mod in zip(row_ref64(row, ops), row_model(row, ops)):
            assert torch.equal(mod.double(), ref), row["name"]
        ops = make_operands(row, "gauss")
        for (ref, mag), mod in zip(row_ref64(row, ops), row_model(row, ops)):
            need = check(mod, ref, mag, c=0.0)["dW"]["need"]
            if need > worst[0]:
                worst = (need, row["name"])
    return worst


# ------------------------------------------------------------------------------------------------ cl_colsum, fp32 route

def colsum_form(B, HW, C_, ws_bytes):
    """colsum() of csrc/elementwise.hip: chunks per sample, pixels per chunk, the path (partials + finish / atomics) and whether the
    C / 8 vectors of a row exceed the 256 lanes of a workgroup (a second pass over the columns)."""
    nchunk = min(_cdiv(HW, 64), _cdiv(512, B))
    ppc = _cdiv(HW, nchunk)
    nchunk = _cdiv(HW, ppc)
    partial = nchunk > 1 and ws_bytes > 0 and B * nchunk * C_ * 4 <= ws_bytes
    return dict(nchunk=nchunk, ppc=ppc, path="partial" if partial else "atomic", passes=_cdiv(C_ // 8, 256))


COLSUM_CASES = [dict(name=f"colsum-{B}x{HW}x{C_}", family="colsum", B=B, HW=HW, C=C_, scale=s)
                for B, HW, C_, s in ((1, 1, 8, 1.0), (3, 1, 320, 0.5), (3, 63, 320, 1.0), (1, 63, 2056, -2.0), (1, 64, 2056, 1.0), (3, 64, 8, 1.0),
                                     (3, 65, 8, 0.5), (1, 65, 320, 1.0), (3, 65, 2056, 1.0), (3, 4096, 320, -2.0), (1, 4096, 2056, 0.5))]
# one exact-tier row per stride for cl_conv_tap_gather -> cl_transpose -> cl_weight_grad (fp32; all nine taps of each)
F32_ROUTE_CASES = [dict(name=f"f32route-s{s}", family="f32route", unit=_taps(2, 8, 8, s, 16, 32)) for s in (1, 2)]

CASES = []
CASES.extend(_cases())


# ------------------------------------------------------------------------------------------------ refusals
# Every call the launcher must refuse (CL_EINVAL, nothing launched, the probe at "nothing", no dW touched), as descriptor lists over
# three base descriptors.  `refused` above is asserted to agree when the table is built.  The W < 8 row-of-three shapes were accepted
# before and computed a wrong gradient (the x tile holds 40 rows, W = 4 needs 48); they are tested as refusals and never launched.

def _rbase():
    plain = dict(M=64, N=16, K=24, alpha=1.0, tap=-1, Hin=0, Win=0, Hout=0, Wout=0, stride=0, pad=0, lddy=32, ldx=32, lddw=32)
    tap = dict(plain, tap=4, Hin=8, Win=8, Hout=8, Wout=8, stride=1, pad=1, lddw=9 * 24)
    r3 = dict(tap, tap=17)
    return plain, tap, r3


def refusal_cases():
    """[(name, [descriptors])]: exactly one descriptor of each list is bad; the others are valid."""
    plain, tap, r3 = _rbase()
    one = lambda name, base, **kw: (name, [dict(base, **kw)])
    cases = [
        # ---- refused before this suite existed
        one("N % 8", plain, N=12), one("K % 8", plain, K=20), one("N < 8", plain, N=4), one("K < 8", plain, K=4),
        one("lddy % 8", plain, lddy=36), one("ldx % 8", plain, ldx=36), one("lddw % 4", plain, lddw=34), one("dW misaligned", plain, dw_misaligned=True),
        one("tap 9", tap, tap=9), one("tap 15", tap, tap=15), one("tap 19", r3, tap=19), one("tap Hin 0", tap, Hin=0), one("tap Win 0", tap, Win=0),
        one("tap Hin > 32767", tap, Hin=40000), one("tap stride 3", tap, stride=3), one("tap stride 0", tap, stride=0),
        one("tap M % (Hout Wout)", tap, M=72), one("row3 stride 2", r3, stride=2), one("row3 pad 0", r3, pad=0), one("row3 Hin != Hout", r3, Hin=16),
        one("row3 Win != Wout", r3, Win=16), one("row3 M % 32", r3, M=16, Hin=2, Hout=2), one("row3 Wout 24", r3, M=96, Hin=4, Hout=4, Win=24, Wout=24),
        one("row3 lddw < 3 K", r3, lddw=64),
        # ---- new with this suite
        one("row3 Wout 4", r3, M=32, Hin=8, Hout=8, Win=4, Wout=4), one("row3 Wout 2", r3, M=32, Hin=16, Hout=16, Win=2, Wout=2),
        one("row3 Wout 1", r3, M=32, Hin=32, Hout=32, Win=1, Wout=1),
        one("tap Hout > 32767", tap, M=40000, Hout=40000, Wout=1), one("tap Wout > 32767", tap, M=40000, Hout=1, Wout=40000),
        one("tap Hout Wout overflows int", tap, Hout=65536, Wout=65536), one("tap Hout < 0", tap, Hout=-8, Wout=-8),
        one("tap pad < 0", tap, pad=-1), one("tap pad > 32767", tap, pad=40000),
        one("lddw < K", plain, lddw=16), one("tap lddw < K", tap, lddw=16), one("lddy < N", plain, lddy=8), one("ldx < K", plain, ldx=16),
        one("tap ldx < K", tap, ldx=16), one("row3 lddy < N", r3, lddy=8),
        one("null dy", plain, null=("dy",)), one("null x", plain, null=("x",)), one("null dW", plain, null=("dW",)), one("row3 null x", r3, null=("x",)),
        # ---- atomic refusal: the valid members of a refused group stay untouched, whatever their kind and place
        ("mixed: bad row3 after two taps", [dict(tap), dict(tap, tap=0), dict(r3, tap=19)]),
        ("mixed: row3 Wout 4 after a tap and a plain", [dict(tap), dict(plain), dict(r3, M=32, Hin=8, Hout=8, Win=4, Wout=4)]),
        ("mixed: bad tap after a row3", [dict(r3), dict(tap, pad=-1)]),
        ("mixed: bad plain between taps", [dict(tap), dict(plain, lddw=16), dict(tap, tap=8)]),
    ]
    for name, ds in cases:
        assert sum(map(refused, ds)) == 1 and plan(ds) is None, name
    return cases


def fill_desc(sd, d, dy, x, dW):
    """Set the fields of a ctypes cl_wgrad_desc from a descriptor dict and the three addresses."""
    null = d.get("null", ())
    sd.dy, sd.x = (None if "dy" in null else dy), (None if "x" in null else x)
    sd.dW = None if "dW" in null else dW + (4 if d.get("dw_misaligned") else 0)
    sd.lddy, sd.ldx, sd.lddw = d["lddy"], d["ldx"], d["lddw"]
    sd.M, sd.N, sd.K, sd.scale = d["M"], d["N"], d["K"], d["alpha"]
    sd.tap, sd.Hin, sd.Win, sd.Hout, sd.Wout, sd.stride, sd.pad = (d[k] for k in ("tap", "Hin", "Win", "Hout", "Wout", "stride", "pad"))


REFUSALS = refusal_cases()


if __name__ == "__main__":
    import time
    t0 = time.time()
    need, name = measure_constants()
    print("largest need %.4f on %s -> MEASURED = %.3f, c = %.3f" % (need, name, need, MARGIN * need))
    print("rows", len(CASES), "descriptors", sum(len(row_descs(r)) for r in CASES), "seconds", round(time.time() - t0, 1))
