"""fp32 restatement of LitEma's update (ldm/modules/ema.py of the reference), in numpy, one rounding per operation: what
cl_ema_update must reproduce bit for bit (tests/test_gpu_ema.py) and what tests/test_ema_reference_model.py checks against the
fixture tests/golden/ema.pt, which the unmodified reference wrote (tests/golden/make_golden_ema.py).

    u   = num_updates AFTER this update's increment (negative: no warm-up, no increment)
    d   = min(decay, (1 + u) / (10 + u)) for u >= 0, decay for u < 0       -- Python's min: the second wins only if smaller
    omd = 1 - d
    s   = s - omd * (s - p)

Two near misses are kept next to it, to show that the fixture tells them apart: the product contracted into the last difference
(one rounding instead of two), and the textbook form d * s + omd * p.
"""
import os

import numpy as np
import torch

from tests.util import GOLDEN

F = np.float32
FIXTURE = os.path.join(GOLDEN, "ema.pt")


def shadow_key(name: str) -> str:
    return name.replace(".", "")


def decay_at(decay, u: int) -> np.float32:
    d = F(decay)
    if u >= 0:
        w = F(1 + u) / F(10 + u)
        d = w if w < d else d
    return d


def update(s: np.ndarray, p: np.ndarray, decay, u: int) -> np.ndarray:
    """The shadow after one update; s, p float32 arrays, u already advanced."""
    assert s.dtype == np.float32 and p.dtype == np.float32
    with np.errstate(all="ignore"):
        omd = F(1.0) - decay_at(decay, u)
        diff = s - p
        step = omd * diff
        return s - step


def update_contracted(s, p, decay, u):
    """NOT the update: omd * (s - p) enters the last difference unrounded, as a fused multiply-add would have it."""
    omd = F(1.0) - decay_at(decay, u)
    diff = (s - p).astype(np.float64)
    return (s.astype(np.float64) - np.float64(omd) * diff).astype(np.float32)      # the fp64 product of two fp32 is exact


def update_lerp(s, p, decay, u):
    """NOT the update: d * s + (1 - d) * p, the same value in exact arithmetic and other bits in fp32."""
    d = decay_at(decay, u)
    omd = F(1.0) - d
    return d * s + omd * p


def bits(a) -> np.ndarray:
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b) -> bool:
    x, y = bits(a), bits(b)
    return x.shape == y.shape and bool((x == y).all())


def load_fixture():
    return torch.load(FIXTURE, map_location="cpu", weights_only=False)


def replay(run, step_fn=update):
    """Re-run one fixture run with `step_fn`: [{shadow key: float32 array}] after every update, and the counts."""
    cfg, names = run["cfg"], run["names"]
    shadows = {k: run["init"][n].numpy().copy() for n, k in names.items()}
    u = -1 if not cfg["use_num_updates"] else (cfg["preset"] if cfg["preset"] is not None else 0)
    out, counts = [], []
    for params in run["params"]:
        if u >= 0:
            u += 1
        shadows = {k: step_fn(shadows[k], params[n].numpy(), cfg["decay"], u) for n, k in names.items()}
        out.append(shadows)
        counts.append(u)
    return out, counts


def trajectory(start: torch.Tensor, params, decay, u0: int = 0):
    """Shadows of a recorded parameter trajectory: `start` the seed, `params` the parameters after every optimizer step (CPU fp32
    tensors of one shape); returns the shadow after the last one as a tensor, counting from u0."""
    s = start.detach().cpu().numpy().astype(np.float32).copy()
    u = u0
    for p in params:
        u += 1
        s = update(s, p.detach().cpu().numpy().astype(np.float32), decay, u)
    return torch.from_numpy(s)
