"""Host restatement of the grouped AdamW step (cl_adamw_dev_groups + cl_lr_schedule), in fp64 and in fp32 torch, built on
tests/ew_ref.eval_adamw_step applied once per parameter group.

Contract (ctrlora_amd/csrc/elementwise.hip, include/ctrlora_hip.h): a flat fp32 buffer of n = 64 C elements, a uint8 map
`chunk_group[C]` naming the group of each 64-float chunk, a table `rows[G]` of {lr, beta1, beta2, eps, wd, gscale}.  Element i takes
the one-group AdamW step with the row of group min(chunk_group[i // 64], G - 1); with a clip coefficient its gscale is
fl32(gscale * coef); with a learning-rate table [T][G] the row's lr for optimizer step s (from 1) is table[min(s - 1, T - 1)][k].
"""
import torch

from tests import ew_ref as R

CHUNK = 64
KEYS = ("lr", "beta1", "beta2", "eps", "wd", "gscale")


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def row(lr, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-2, gscale=1.0):
    return dict(lr=lr, beta1=beta1, beta2=beta2, eps=eps, wd=wd, gscale=gscale)


def table(rows):
    """The [G, 6] fp32 table the kernel reads."""
    return torch.tensor([[r[k] for k in KEYS] for r in rows], dtype=torch.float32)


def lr_row(step, T):
    """cl_lr_schedule's row for the counter value `step` (after the tick): LambdaLR's indexing, clamped at both ends."""
    return min(max(step - 1, 0), T - 1)


def scheduled_rows(rows, lr_table, step):
    if lr_table is None:
        return rows
    r = lr_row(step, lr_table.shape[0])
    return [dict(rw, lr=float(lr_table[r, k])) for k, rw in enumerate(rows)]


def element_groups(chunk_group, ngroups):
    """Per element: the group the kernel uses (an entry >= ngroups is clamped to the last group)."""
    return chunk_group.to(torch.int64).clamp(max=ngroups - 1).repeat_interleave(CHUNK)


def runs(chunk_group, ngroups):
    """[(first element, one past the last, group)] of the contiguous runs of chunks with one (clamped) group."""
    g = chunk_group.to(torch.int64).clamp(max=ngroups - 1).tolist()
    out, lo = [], 0
    for c in range(1, len(g) + 1):
        if c == len(g) or g[c] != g[lo]:
            out.append((lo * CHUNK, c * CHUNK, g[lo]))
            lo = c
    return out


def _one_group(state, g, step, rw, coef):
    keep = dict(R.ADAMW_HYPER)
    try:
        R.ADAMW_HYPER.update(rw)
        if coef is not None:      # the two scalars are multiplied first, in fp32 (cl_adamw_dev_clip)
            R.ADAMW_HYPER["gscale"] = float(torch.tensor(rw["gscale"], dtype=torch.float32) * torch.tensor(coef, dtype=torch.float32))
        return R.eval_adamw_step(state, g, step)
    finally:
        R.ADAMW_HYPER.clear()
        R.ADAMW_HYPER.update(keep)


def eval_grouped_step(state, g, step, rows, chunk_group, coef=None, lr_table=None):
    """One grouped step from `state` = (p, m, v) as stored (fp32, flat, n = 64 * len(chunk_group)): {p, m, v: {ref: fp64,
    model: the fp32 torch restatement}}, every element from the one-group step of its own group."""
    n = state[0].numel()
    assert n == chunk_group.numel() * CHUNK and g.numel() == n
    rows = scheduled_rows(rows, lr_table, step)
    eg = element_groups(chunk_group, len(rows))
    out = {}
    for k, rw in enumerate(rows):
        sel = eg == k
        if not bool(sel.any()):
            continue
        sp = _one_group(state, g, step, rw, coef)
        for key in ("p", "m", "v"):
            dst = out.setdefault(key, dict(u=sp[key]["u"], fam=sp[key]["fam"]))
            for field in ("ref", "mag", "fixed", "model"):       # the one-group spec's own bound travels with its elements
                src = sp[key][field]
                src = src if torch.is_tensor(src) else torch.full((n,), float(src), dtype=torch.float64)
                dst.setdefault(field, torch.zeros(n, dtype=src.dtype))[sel] = src[sel]
    return out


def layout(sizes):
    """Offsets of tensors of `sizes` elements, each padded to whole chunks (packing.TrainableSet.materialize), and the total."""
    offs, off = [], 0
    for s in sizes:
        offs.append(off)
        off += (s + CHUNK - 1) // CHUNK * CHUNK
    return offs, off


def chunk_map(sizes, groups):
    offs, total = layout(sizes)
    cg = torch.zeros(total // CHUNK, dtype=torch.uint8)
    for s, o, k in zip(sizes, offs, groups):
        cg[o // CHUNK:(o + (s + CHUNK - 1) // CHUNK * CHUNK) // CHUNK] = k
    return cg
