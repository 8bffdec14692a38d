"""What DDIMSampler (cldm/ddim_hacked.py), DPMSolverSampler (dpm_solver/sampler.py) and PLMSSampler (plms.py) share: how two
conditionings become one batch, one classifier-free-guidance evaluation, the scopes around a sampling loop (context K/V cache,
hint encode) and the protocol that captures one step as a hipGraph and replays it.  The samplers keep what differs: tables,
update kernels, the eager loops and their public API."""
import contextlib

import torch

# Order of the halves of a batched guidance call.  DDIM sampling batches [cond; uncond]; DDIM inversion, DPM-Solver++ and PLMS batch
# [uncond; cond] as the reference does.  The halves are independent samples, but the order sets the rows of every GEMM and
# with them possibly the bits, so each path keeps the order it has always had.
COND_FIRST, UNCOND_FIRST = "cond_first", "uncond_first"


def cat_conds(c, u):
    """Batch two conditioning dicts (or lists of dicts) along dim 0; None if their structure differs."""
    if isinstance(c, dict) and isinstance(u, dict) and c.keys() == u.keys():
        out = {}
        for k in c:
            a, b = c[k], u[k]
            if isinstance(a, list) and isinstance(b, list) and len(a) == len(b) and all(
                    torch.is_tensor(x) and torch.is_tensor(y) and x.shape == y.shape for x, y in zip(a, b)):
                out[k] = [torch.cat([x, y], 0) for x, y in zip(a, b)]
            elif a is None and b is None:
                out[k] = None
            elif isinstance(a, str) and a == b:
                out[k] = a
            else:
                return None
        return out
    if isinstance(c, (list, tuple)) and isinstance(u, (list, tuple)) and len(c) == len(u):
        parts = [cat_conds(a, b) for a, b in zip(c, u)]
        return None if any(p is None for p in parts) else parts
    return None


def batch_conds(cond, uncond, order, cat_tensors):
    """The conditioning of ONE call of 2B for both guidance passes, or None: the passes then run one after the other.
    cat_tensors: bare tensors are batched with torch.cat (DDIM inversion, DPM-Solver++); DDIM sampling runs them as two passes."""
    if uncond is None:
        return None
    first, second = (cond, uncond) if order == COND_FIRST else (uncond, cond)
    if torch.is_tensor(first) and torch.is_tensor(second):
        return torch.cat([first, second]) if cat_tensors else None
    return cat_conds(first, second)


def guided_eps(model, x, ts, cond, uncond, both, order):
    """(eps_cond, eps_uncond or None) of one step.  uncond None: no guidance, one call of B.  both (batch_conds): one call of
    2B whose halves lie in `order`; ts has B entries and is doubled here, or already 2B (a device-side time written by the
    step's own kernel).  Otherwise cond then uncond, B each."""
    if uncond is None:
        return model.apply_model(x, ts, cond), None
    if both is None:
        return model.apply_model(x, ts, cond), model.apply_model(x, ts, uncond)
    b = x.shape[0]
    e = model.apply_model(torch.cat([x, x], 0), torch.cat([ts, ts], 0) if ts.shape[0] == b else ts, both)
    return (e[:b], e[b:]) if order == COND_FIRST else (e[b:], e[:b])


def engine_of(model):
    """The model's engine, or None for a model that has none (plain torch, CPU)."""
    return model.engine() if callable(getattr(model, "engine", None)) else None


@contextlib.contextmanager
def context_kv(eng):
    """The text context is constant over a sampling loop: project K/V of every cross-attention once.  Leaves the flag cleared
    and the cache empty however the loop ends.  A caller that keeps a captured graph takes the cached products with
    eng.detach_context_cache() before it leaves the scope (the graph reads them by address)."""
    if eng is not None:
        eng.cache_context_kv = True
        eng.reset_context_cache()
    try:
        yield eng
    finally:
        if eng is not None:
            eng.cache_context_kv = False
            eng.reset_context_cache()


def hint_scope(model, hoist):
    """Condition images do not change during a run: VAE-encode them once (ControlLDM.hint_cache), if asked and offered."""
    scope = getattr(model, "hint_cache", None) if hoist else None
    return scope() if callable(scope) else contextlib.nullcontext()


def capture(body):
    """body() captured as a hipGraph; capturing does not execute it.  Returns the graph: replay() runs it."""
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    return graph


def run_steps(body, S, after_step=None, graph=None, keep_graph=False):
    """S executions of a step body() whose state (cursor, time, sample) lives on the device.  Step 0 runs eagerly (it fills the
    context K/V cache and sizes every buffer), step 1 is captured and that capture replayed, the rest replay: 2 Python-level
    executions of body however large S is.  With a kept `graph` every step is a replay.  after_step(i) follows every step.
    keep_graph: hand the graph back (the caller then holds everything it reads by address); otherwise wait for the last
    replay before the graph and its buffers are released, and return None."""
    for i in range(S):
        if graph is None and i == 0:
            body()
        else:
            if graph is None:
                graph = capture(body)
            graph.replay()
        if after_step is not None:
            after_step(i)
    if keep_graph:
        return graph
    torch.cuda.synchronize()
    return None
